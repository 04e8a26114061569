// ticon.hip -- the TICON stage of the reference's H-optimus + TICON extractor as ONE call on a batch of tile embeddings.
//
// src/stamp/preprocessing/extractor/ticon.py: `HOptimusTICON.forward` :691-718 pushes every tile's embedding ALONE (one token, coordinates
// (0, 0)) through `EncoderDecoder.forward` :543-562.  With a single key the ALiBi attention (:183-215) returns its value whatever the
// bias, so a block is  x += g1 * proj(v_proj(LN1(x)));  x += g2 * fc2(silu(x1) * x2), (x1 | x2) = fc1(LN2(x))  (:290-343, :54-77) -- row-wise
// fp32 work on [n_tiles][dim]: exact-fp32 MFMA products (amds_linear_f32 / amds_bgemm_f32), LayerNorm and activation kernels.
//
// SLIDE mode (amds_ticon_slide_forward): the same `EncoderDecoder.forward` on ALL tiles of a slide with their coordinates -- every tile attends to the others
// under the pre-softmax distance bias of `Attention.forward` :183-215.  The MIL `vit` head's recipe: fp32 residual stream, 16-bit MFMA GEMMs on zero-padded
// weights (q | k | v stacked, heads padded to 64 channels), amds_attention_distbias for the attention, SWIGLU and RESIDUAL (LayerScale) epilogues.
#include <algorithm>
#include "model_call.h"

namespace amds {
namespace {
struct TcPlan { size_t e, x, t, u, total; };

int tc_plan(const amds_ticon_weights* w, int B, TcPlan* p) {
    AMDS_REQUIRE(w, "amds_ticon: null weights");
    AMDS_REQUIRE(w->in_dim > 0 && w->dim > 0 && w->dim % 4 == 0 && w->hidden > 0 && w->hidden % 2 == 0 && w->depth >= 0 && B >= 0, "amds_ticon: bad configuration");
    Arena ar;
    p->e = ar.take((size_t)B * w->in_dim * 4);
    p->x = ar.take((size_t)B * w->dim * 4);
    p->t = ar.take((size_t)B * w->dim * 4);
    p->u = ar.take((size_t)B * std::max(w->hidden, w->dim) * 4);
    p->total = ar.off;
    return AMDS_OK;
}

__global__ void __launch_bounds__(256) tc_f16_to_f32_kernel(const f16* __restrict__ src, float* __restrict__ dst, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (float)src[i];
}

// ---- slide mode -------------------------------------------------------------------------------------------------------------------------------------------
struct TsPlan {
    int Fp, Dp, Ha, Da, Hp;      // (the MLP's padded width is TICON's own Hp, not PadDims::FFp)
    size_t a, x, h, qkv, att, u, total;
};

int ts_plan(const amds_ticon_slide_cfg* c, int B, int T, TsPlan* p) {
    AMDS_REQUIRE(c, "amds_ticon_slide: null configuration");
    AMDS_REQUIRE(c->in_dim > 0 && c->dim > 0 && c->heads > 0 && c->hidden > 0 && c->hidden % 2 == 0 && c->depth >= 0, "amds_ticon_slide: bad configuration");
    AMDS_REQUIRE(c->dim % c->heads == 0 && c->dim / c->heads <= 64 && c->dim % 4 == 0 && c->dim <= 8192,
                 "amds_ticon_slide: needs dim %% heads == 0, head_dim <= 64, dim %% 4 == 0 and dim <= 8192 (dim=%d, heads=%d)", c->dim, c->heads);
    AMDS_REQUIRE(c->dtype == AMDS_F16 || c->dtype == AMDS_BF16, "amds_ticon_slide: operand dtype must be f16 or bf16");
    AMDS_REQUIRE(B >= 0 && B <= 65535 && T > 0, "amds_ticon_slide: bad shape slides=%d tiles=%d", B, T);
    const PadDims pd = pad_dims(c->in_dim, c->dim, c->hidden, c->heads);
    p->Fp = pd.Fp; p->Dp = pd.Dp; p->Ha = pd.Ha; p->Da = pd.Da;
    p->Hp = round_up(c->hidden / 2, 128);
    AMDS_REQUIRE((long)T * 3 * p->Ha * 128 < (1L << 31), "amds_ticon_slide: %d tiles of %d heads: a slide's q | k | v rows must stay below 2 GB", T, p->Ha);
    const size_t M = (size_t)B * T;
    AMDS_REQUIRE(M < ((size_t)1 << 31), "amds_ticon_slide: %zu token rows do not fit the 32-bit row index", M);
    Arena ar;
    p->a = ar.take(M * p->Fp * 2);                     // staged embeddings, 16-bit, zero padded columns
    p->x = ar.take(M * p->Dp * 4);                     // residual stream fp32
    p->h = ar.take(M * p->Dp * 2);                     // LayerNorm output / the input projection's hidden
    p->qkv = ar.take(M * 3 * p->Da * 2);               // (first: fp32 scratch of the input projection, 6 Da >= 4 Dp bytes per row)
    p->att = ar.take(M * p->Da * 2);
    p->u = ar.take(M * p->Hp * 2);
    p->total = ar.off;
    return AMDS_OK;
}

// the input projection's activation: fp32 fc1 rows -> silu -> 16-bit operand rows of fc2 (padding columns: silu(0) = 0)
template <typename TO>
__global__ void __launch_bounds__(256) ts_silu_cast_kernel(const float* __restrict__ src, TO* __restrict__ dst, long n4) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
        typename Act<TO>::vec4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = Act<TO>::from_f32(silu(v[e]));
        reinterpret_cast<typename Act<TO>::vec4*>(dst)[i] = w;
    }
}
}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_ticon_tile_workspace_bytes(const amds_ticon_weights* w_host, int n_tiles) {
    TcPlan p;
    if (tc_plan(w_host, n_tiles, &p) != AMDS_OK) return 0;
    return p.total;
}

extern "C" int amds_ticon_tile_forward(const amds_ticon_weights* w_host, const void* emb, int emb_dtype, void* out, int out_dtype, int n_tiles, void* ws,
                                       size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(w_host, "amds_ticon_tile_forward: null weights");
    if (n_tiles == 0) return AMDS_OK;
    AMDS_REQUIRE(emb && out && ws, "amds_ticon_tile_forward: null pointer");
    const amds_ticon_weights& w = *w_host;
    TcPlan p;
    RC(tc_plan(w_host, n_tiles, &p));
    AMDS_REQUIRE(w.in_fc1_w && w.in_fc1_b && w.in_fc2_w && w.in_fc2_b && w.in_norm_w && w.in_norm_b && w.norm_w && w.norm_b && (w.depth == 0 || w.blocks_host),
                 "amds_ticon_tile_forward: incomplete weights");
    AMDS_REQUIRE((emb_dtype == AMDS_F32 || emb_dtype == AMDS_F16) && (out_dtype == AMDS_F32 || out_dtype == AMDS_F16), "amds_ticon_tile_forward: bad dtype");
    if (ws_bytes < p.total) {
        set_error("amds_ticon_tile_forward: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_ticon_tile_forward: workspace must be 256-byte aligned");
    if (n_tiles == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    const int B = n_tiles, D = w.dim, Hh = w.hidden, H2 = w.hidden / 2;
    const float* e = reinterpret_cast<const float*>(emb);
    if (emb_dtype == AMDS_F16) {
        const long n = (long)B * w.in_dim;
        float* ef = reinterpret_cast<float*>(base + p.e);
        hipLaunchKernelGGL(tc_f16_to_f32_kernel, dim3((unsigned)std::min<long>(4096, (n + 255) / 256)), dim3(256), 0, st, (const f16*)emb, ef, n);
        AMDS_LAUNCH_CHECK("tc_f16_to_f32_kernel");
        e = ef;
    }
    float *x = reinterpret_cast<float*>(base + p.x), *t = reinterpret_cast<float*>(base + p.t), *u = reinterpret_cast<float*>(base + p.u);
    // input projection: Linear, SiLU, Linear, LayerNorm (:94-98)
    RC(amds_linear_f32(e, w.in_fc1_w, w.in_fc1_b, u, B, D, w.in_dim, 0, stream));
    RC(amds_mlp_act_f32(u, D, B, D, 2, stream));
    RC(amds_linear_f32(u, w.in_fc2_w, w.in_fc2_b, t, B, D, D, 0, stream));
    RC(amds_layernorm(t, D, w.in_norm_w, w.in_norm_b, x, D, B, D, 1e-5f, AMDS_F32, stream));
    for (int l = 0; l < w.depth; ++l) {
        const amds_ticon_block& b = w.blocks_host[l];
        AMDS_REQUIRE(b.ln1_w && b.ln1_b && b.v_w && b.v_b && b.proj_w && b.proj_b && b.ln2_w && b.ln2_b && b.fc1_w && b.fc1_b && b.fc2_w && b.fc2_b,
                     "amds_ticon_tile_forward: incomplete weights of block %d", l);
        RC(amds_layernorm(x, D, b.ln1_w, b.ln1_b, t, D, B, D, 1e-5f, AMDS_F32, stream));
        RC(amds_linear_f32(t, b.v_w, b.v_b, u, B, D, D, 0, stream));                                                       // one key: attention = value
        RC(bgemm_f32_exact(u, D, 0, 0, b.proj_w, D, 0, 0, 1, x, D, 0, 0, 1, 1, B, D, D, 1.0f, 0.0f, b.proj_b, 1, stream));    // x += g1 * proj(v)
        RC(amds_layernorm(x, D, b.ln2_w, b.ln2_b, t, D, B, D, 1e-5f, AMDS_F32, stream));
        RC(amds_linear_f32(t, b.fc1_w, b.fc1_b, u, B, Hh, D, 0, stream));
        RC(amds_mlp_act_f32(u, Hh, B, H2, 1, stream));                                                                     // u[:, :H2] = silu(x1) * x2
        RC(bgemm_f32_exact(u, Hh, 0, 0, b.fc2_w, H2, 0, 0, 1, x, D, 0, 0, 1, 1, B, D, H2, 1.0f, 0.0f, b.fc2_b, 1, stream));   // x += g2 * fc2(.)
    }
    return amds_layernorm(x, D, w.norm_w, w.norm_b, out, D, B, D, 1e-5f, out_dtype, stream);
}

// ---- slide mode ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t amds_ticon_slide_workspace_bytes(const amds_ticon_slide_cfg* cfg_host, int n_slides, int n_tiles) {
    TsPlan p;
    if (ts_plan(cfg_host, n_slides, n_tiles, &p) != AMDS_OK) return 0;
    return p.total;
}

extern "C" int amds_ticon_slide_forward(const amds_ticon_slide_cfg* cfg_host, const amds_ticon_slide_weights* w_host, const void* emb, int emb_dtype,
                                        const float* coords, void* out, int out_dtype, int n_slides, int n_tiles, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(cfg_host && w_host && emb && coords && out && ws, "amds_ticon_slide_forward: null pointer");
    const amds_ticon_slide_cfg& c = *cfg_host;
    const amds_ticon_slide_weights& w = *w_host;
    TsPlan p;
    RC(ts_plan(cfg_host, n_slides, n_tiles, &p));
    AMDS_REQUIRE(w.in_fc1_w && w.in_fc1_b && w.in_fc2_w && w.in_fc2_b && w.in_norm_w && w.in_norm_b && w.slopes && w.norm_w && w.norm_b && (c.depth == 0 || w.blocks_host),
                 "amds_ticon_slide_forward: incomplete weights");
    for (int l = 0; l < c.depth; ++l) {
        const amds_ticon_slide_block& b = w.blocks_host[l];
        AMDS_REQUIRE(b.ln1_w && b.ln1_b && b.in_w && b.in_b && b.proj_w && b.proj_b && b.ln2_w && b.ln2_b && b.fc1_w && b.fc1_b && b.fc2_w && b.fc2_b,
                     "amds_ticon_slide_forward: incomplete weights of block %d", l);
    }
    AMDS_REQUIRE((emb_dtype == AMDS_F32 || emb_dtype == AMDS_F16) && (out_dtype == AMDS_F32 || out_dtype == AMDS_F16), "amds_ticon_slide_forward: bad dtype");
    if (ws_bytes < p.total) {
        set_error("amds_ticon_slide_forward: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_ticon_slide_forward: workspace must be 256-byte aligned");
    const bool staged = !(emb_dtype == c.dtype && c.in_dim == p.Fp);
    AMDS_REQUIRE(staged || ((uintptr_t)emb & 15) == 0, "amds_ticon_slide_forward: operand-form embeddings must be 16-byte aligned");
    AMDS_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)coords & 7) == 0, "amds_ticon_slide_forward: out must be 16-byte, coords 8-byte aligned");
    if (n_slides == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    const int B = n_slides, T = n_tiles, D = c.dim, Dp = p.Dp, Da = p.Da, Hp = p.Hp, dt = c.dtype;
    const int M = B * T;
    float* x = reinterpret_cast<float*>(base + p.x);
    void *h = base + p.h, *qkv = base + p.qkv, *att = base + p.att, *u = base + p.u;
    float* f = reinterpret_cast<float*>(qkv);
    // The GEMM kernel is chosen from ONE slide's rows, so a slide's features do not depend on how many slides share the call (amds_gemm_ex: the
    // 256-row kernels sum in another order than the 128-row one)
    auto gemm = [&](const void* A, long lda, const void* W, long ldw, int N, int K, int epi, void* o, long ldo, const float* bias, const float* scale) {
        const int cfg = default_gemm_cfg(T, N, K) == 0 ? 0 : -1;
        return amds_gemm_ex(cfg, A, lda, W, ldw, M, N, K, dt, epi, o, ldo, bias, scale, nullptr, 0, 0, 0, 1.0f, stream);
    };

    // the embeddings as 16-bit operand rows of pitch Fp (already in that form when dtype and pitch agree)
    const void* a = emb;
    if (staged) {
        RC(stage_rows_dt(emb, emb_dtype, c.in_dim, base + p.a, dt, p.Fp, M, c.in_dim, stream));
        a = base + p.a;
    }
    // input projection: Linear, SiLU, Linear, LayerNorm (:94-98); the two fp32 intermediates live in the qkv region
    RC(gemm(a, p.Fp, w.in_fc1_w, p.Fp, Dp, p.Fp, AMDS_EPI_BIAS_F32, f, Dp, w.in_fc1_b, nullptr));
    {
        const long n4 = (long)M * Dp / 4;
        const dim3 grid((unsigned)std::min<long>(8192, (n4 + 255) / 256));
        dispatch_16(dt, [&](auto t) {
            typedef AMDS_TAG_T(t) TO;
            hipLaunchKernelGGL((ts_silu_cast_kernel<TO>), grid, dim3(256), 0, st, (const float*)f, (TO*)h, n4);
        });
        AMDS_LAUNCH_CHECK("ts_silu_cast_kernel");
    }
    RC(gemm(h, Dp, w.in_fc2_w, Dp, Dp, Dp, AMDS_EPI_BIAS_F32, f, Dp, w.in_fc2_b, nullptr));
    if (Dp != D) {      // LayerNorm writes the first D columns only: the GEMMs read all Dp of h, the RESIDUAL epilogue all Dp of x
        AMDS_HIP(hipMemsetAsync(x, 0, (size_t)M * Dp * 4, st));
        AMDS_HIP(hipMemsetAsync(h, 0, (size_t)M * Dp * 2, st));
    }
    RC(amds_layernorm(f, Dp, w.in_norm_w, w.in_norm_b, x, Dp, M, D, 1e-5f, AMDS_F32, stream));
    for (int l = 0; l < c.depth; ++l) {
        const amds_ticon_slide_block& b = w.blocks_host[l];
        RC(amds_layernorm(x, Dp, b.ln1_w, b.ln1_b, h, Dp, M, D, 1e-5f, dt, stream));
        RC(gemm(h, Dp, b.in_w, Dp, 3 * Da, Dp, AMDS_EPI_BIAS, qkv, 3 * Da, b.in_b, nullptr));
        RC(amds_attention_distbias(qkv, coords, w.slopes, att, B, T, p.Ha, dt, stream));
        RC(gemm(att, Da, b.proj_w, Da, Dp, Da, AMDS_EPI_RESIDUAL, x, Dp, b.proj_b, b.g1));                 // x += g1 * proj(attn)   (:336-341, :262)
        RC(amds_layernorm(x, Dp, b.ln2_w, b.ln2_b, h, Dp, M, D, 1e-5f, dt, stream));
        RC(gemm(h, Dp, b.fc1_w, Dp, 2 * Hp, Dp, AMDS_EPI_SWIGLU, u, Hp, b.fc1_b, nullptr));                // u = silu(x1) * x2      (:73-75)
        RC(gemm(u, Hp, b.fc2_w, Hp, Dp, Hp, AMDS_EPI_RESIDUAL, x, Dp, b.fc2_b, b.g2));                     // x += g2 * fc2(u)       (:342)
    }
    return amds_layernorm(x, Dp, w.norm_w, w.norm_b, out, D, M, D, 1e-5f, out_dtype, stream);            // enc_norm (:506)
}
