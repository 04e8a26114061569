// barspoon.hip -- the deploy / validation forward of the reference's barspoon head (`EncDecTransformer`) as ONE call:
// bags of tile features + tile positions -> one logit vector per target.
//
// Restates src/stamp/modeling/models/barspoon.py in eval mode:
//   projector (Linear + ReLU) :171, sinusoidal encoding of the tile positions added :173-186,
//   pre-norm nn.TransformerEncoder over the tiles :188 (per layer: x += SA(LN1(x)); x += W2 relu(W1 LN2(x))),
//   one learned class token per target decoded against the tile tokens by a pre-norm nn.TransformerDecoder :190-193
//   (per layer: t += SA(LN1(t)); t += MHA(LN2(t), memory = tiles); t += W2 relu(W1 LN3(t))), one Linear head per target :196-203.
// The tile side (projector, encoder, the K / V projections of the cross-attention: everything with a tile dimension) runs on the 16-bit
// MFMA GEMMs and the streaming attention kernel, with the zero-padded weight layout of the MIL `vit` head (amds_mil_vit_layer: widths to
// 256, heads to 64 channels); the class-token side (n_targets rows per bag) runs in exact fp32 (amds_bgemm_f32).  The cross-attention is
// its own kernel: one fp32 query row per (bag, target, head) streamed over the bag's 16-bit keys / values with an online softmax.
// The launch sequences of one encoder and one decoder layer (bs_encoder_layer, bs_decoder_layer) and the heads serve this dense call and the ragged one
// (barspoon_ragged.hip) alike; a BsCall (barspoon_common.h) says how a call reaches its bags and which GEMM kernel id it passes.
#include <algorithm>
#include <type_traits>
#include "barspoon_common.h"

namespace amds {
namespace {

// x[r][c] += PE(pos[r])[c] for c < D:  [ sin(px / f_i) | sin(py / f_i) | cos(px / f_i) | cos(py / f_i) ],  i < D / 4,  f_i = pe_div[i] (:173-186)
__global__ void __launch_bounds__(256) pos_encoding_add_kernel(float* __restrict__ x, int Dp, int D, const float* __restrict__ pos, const float* __restrict__ pe_div,
                                                                long rows) {
    const int q = D / 4;
    const long total = rows * D;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const long r = i / D;
        const int c = (int)(i - r * D);
        const int blk = c / q, f = c - blk * q;                // blk: 0 sin x, 1 sin y, 2 cos x, 3 cos y
        const float a = pos[2 * r + (blk & 1)] / pe_div[f];
        x[r * Dp + c] += blk < 2 ? sinf(a) : cosf(a);
    }
}

__global__ void __launch_bounds__(256) broadcast_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, long per_bag, long total) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) dst[i] = src[i % per_bag];
}

// Cross-attention of the class tokens: out[b][j][h*hd..] = softmax(q[b][j][h*hd..] . K_b,h^T / sqrt(hd)) V_b,h.  q fp32 [B][nt][D]; kv 16-bit
// [B*T][2*Db], K of head h at columns 64h.., V at Db + 64h.. (channels >= hd are zero padding).  One wave per (b, j, h): lane l streams the keys
// l, l + 64, ... with its own running (max, sum, o[64]); the 64 partial states are merged once at the end.
//
// VARLEN (barspoon_ragged.hip): the fifth argument is the per-call table instead of the fixed tile count -- bag b's keys / values are the rows bags[b].x ..
// bags[b].x + bags[b].y - 1 of the packed kv (varlen_plan_kernel with extra_rows = 0; a clamped-empty bag streams nothing) instead of b * Tn .. b * Tn + Tn - 1.
// Per (b, j, h) the arithmetic is the fixed form's, whatever the bag's neighbours.
template <typename T, bool VARLEN = false>
__global__ void __launch_bounds__(256) cross_attention_kernel(const float* __restrict__ q, const T* __restrict__ kv, float* __restrict__ out, int B,
                                                               std::conditional_t<VARLEN, const int2*, int> Tn_or_bags, int nt, int H, int hd, int D, int Db) {
    typedef T vec8 __attribute__((ext_vector_type(8)));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= (long)B * nt * H) return;                      // whole waves leave; no workgroup barrier below
    const int h = (int)(item % H);
    const long bj = item / H;
    const int b = (int)(bj / nt);
    int Tn;
    long row0 = 0;                                             // VARLEN: first tile row of this bag
    if constexpr (VARLEN) {
        const int2 bg = Tn_or_bags[b];
        row0 = bg.x;
        Tn = bg.y;
    } else {
        Tn = Tn_or_bags;
    }
    const float* qr = q + bj * D + (long)h * hd;
    const float sc = rsqrtf((float)hd) * 1.44269504088896340736f;          // log2 domain
    float qv[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) qv[e] = e < hd ? qr[e] * sc : 0.f;
    float m = -INFINITY, l = 0.f, o[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) o[e] = 0.f;
    const long ld = 2L * Db;
    const T* kb = VARLEN ? kv + row0 * ld + 64 * h : kv + (long)b * Tn * ld + 64 * h;
    for (int t = lane; t < Tn; t += 64) {
        const T* kr = kb + t * ld;
        float s = 0.f;
#pragma unroll
        for (int pz = 0; pz < 8; ++pz) {
            const vec8 kk = *reinterpret_cast<const vec8*>(kr + 8 * pz);
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(qv[8 * pz + e], (float)kk[e], s);
        }
        const float mn = fmaxf(m, s);
        const float corr = exp2f(m - mn), pw = exp2f(s - mn);
        l = l * corr + pw;
        const T* vr = kr + Db;
#pragma unroll
        for (int pz = 0; pz < 8; ++pz) {
            const vec8 vv = *reinterpret_cast<const vec8*>(vr + 8 * pz);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[8 * pz + e] = fmaf(o[8 * pz + e], corr, pw * (float)vv[e]);
        }
        m = mn;
    }
    // merge the 64 lanes' states
    float mg = m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mg = fmaxf(mg, __shfl_xor(mg, off, 64));
    const float w = m == -INFINITY ? 0.f : exp2f(m - mg);
    l *= w;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off, 64);
    const float inv = 1.0f / l;
    float* orow = out + bj * D + (long)h * hd;
#pragma unroll
    for (int e = 0; e < 64; ++e) {
        float v = o[e] * w;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0 && e < hd) orow[e] = v * inv;
    }
}

}  // namespace

int pos_encoding_add(float* x, int Dp, int D, const float* pos, const float* pe_div, long rows, hipStream_t st) {
    const long total = rows * D;
    hipLaunchKernelGGL(pos_encoding_add_kernel, dim3((unsigned)std::min<long>(8192, (total + 255) / 256)), dim3(256), 0, st, x, Dp, D, pos, pe_div, rows);
    AMDS_LAUNCH_CHECK("pos_encoding_add_kernel");
    return AMDS_OK;
}

int broadcast_rows(const float* src, float* dst, long per_bag, long total, hipStream_t st) {
    hipLaunchKernelGGL(broadcast_rows_kernel, dim3((unsigned)std::min<long>(4096, (total + 255) / 256)), dim3(256), 0, st, src, dst, per_bag, total);
    AMDS_LAUNCH_CHECK("broadcast_rows_kernel");
    return AMDS_OK;
}

int bs_dims(const char* who, const amds_barspoon_cfg* c, BsPlan* p) {
    AMDS_REQUIRE(c, "%s: null config", who);
    AMDS_REQUIRE(c->n_feats > 0 && c->dim > 0 && c->enc_heads > 0 && c->dec_heads > 0 && c->ff > 0 && c->enc_layers >= 0 && c->dec_layers >= 0 && c->n_targets > 0,
                 "%s: bad config", who);
    AMDS_REQUIRE(c->dim % c->enc_heads == 0 && c->dim % c->dec_heads == 0, "%s: d_model=%d has to be divisible by the head counts (%d, %d)", who, c->dim,
                 c->enc_heads, c->dec_heads);
    AMDS_REQUIRE(c->dim / c->enc_heads <= 64 && c->dim / c->dec_heads <= 64 && c->dim % 4 == 0, "%s: needs head_dim <= 64 and d_model %% 4 == 0", who);
    AMDS_REQUIRE(c->n_targets <= 1024, "%s: %d targets", who, c->n_targets);
    AMDS_REQUIRE(c->dtype == AMDS_F16 || c->dtype == AMDS_BF16, "%s: operand dtype must be f16 or bf16", who);
    static_cast<PadDims&>(*p) = pad_dims(c->n_feats, c->dim, c->ff, c->enc_heads);      // encoder self-attention: padded heads
    p->Hb = c->dec_heads; p->Db = 64 * p->Hb;                        // cross-attention K / V: decoder heads padded to 64 channels
    p->hd_e = c->dim / c->enc_heads; p->hd_d = c->dim / c->dec_heads;
    p->nt = c->n_targets;
    return AMDS_OK;
}

void bs_arena(const amds_barspoon_cfg* c, int n_bags, size_t M, size_t table_bytes, BsPlan* p) {
    const size_t M2 = (size_t)n_bags * p->nt, D = c->dim;
    Arena ar;
    p->a = ar.take(M * p->Fp * 2);
    p->x = ar.take(M * p->Dp * 4);
    p->h = ar.take(M * p->Dp * 2);
    p->qkv = ar.take(M * 3 * p->Da * 2);
    p->att = ar.take(M * p->Da * 2);
    p->u = ar.take(M * p->FFp * 2);
    p->kv = ar.take(M * 2 * p->Db * 2);
    p->tok = ar.take(M2 * D * 4);
    p->th = ar.take(M2 * D * 4);
    p->tqkv = ar.take(M2 * 3 * D * 4);
    p->tsc = ar.take((size_t)n_bags * p->Hb * p->nt * p->nt * 4);
    p->to = ar.take(M2 * D * 4);
    p->tq = ar.take(M2 * D * 4);
    p->tu = ar.take(M2 * (size_t)c->ff * 4);
    p->table = ar.off;
    if (table_bytes) ar.take(table_bytes);
    p->total = ar.off;
}

BsBufs bs_bufs(void* ws, const BsPlan& p) {
    char* base = reinterpret_cast<char*>(ws);
    auto f = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    return BsBufs{f(p.x), base + p.h, base + p.qkv, base + p.att, base + p.u, base + p.kv, f(p.tok), f(p.th), f(p.tqkv), f(p.tsc), f(p.to), f(p.tq), f(p.tu)};
}

namespace {

int bs_plan(const amds_barspoon_cfg* c, int Bb, int T, BsPlan* p) {
    RC(bs_dims("amds_barspoon", c, p));
    AMDS_REQUIRE(Bb >= 0 && T > 0, "amds_barspoon: bad shape bags=%d tiles=%d", Bb, T);
    bs_arena(c, Bb, (size_t)Bb * T, 0, p);
    return AMDS_OK;
}

// (+)= over the class rows of the call: y[M2][N] += x[M2][K] w[N][K]^T + bias.  Dense: one product over all M2 rows.  Ragged: the bag is the batch dimension
// (nt rows each) -- amds_bgemm_f32 picks its tile kernel from M, so each bag's rows then go through the dispatch of its own one-bag call by construction.
int tok_lin_acc(const BsCall& k, int nt, const float* x, const float* w, const float* bias, float* y, int N, int K, void* st) {
    if (k.table) return bg(x, K, (long)nt * K, 0, w, K, 0, 0, 1, y, N, (long)nt * N, 0, k.n_bags, 1, nt, N, K, 1.0f, bias, 1, st);
    return bg(x, K, 0, 0, w, K, 0, 0, 1, y, N, 0, 0, 1, 1, k.n_bags * nt, N, K, 1.0f, bias, 1, st);
}

int cross_attention_launch(const BsCall& k, const BsPlan& p, int dt, const float* tq, const void* kv, float* to, int D, hipStream_t st) {
    const long items = (long)k.n_bags * p.nt * p.Hb;
    const dim3 grid((unsigned)((items + 3) / 4)), block(256);
    if (k.table) {
        const int2* bags = varlen_table_bags(k.table);
        if (dt == AMDS_F16)
            hipLaunchKernelGGL((cross_attention_kernel<f16, true>), grid, block, 0, st, tq, (const f16*)kv, to, k.n_bags, bags, p.nt, p.Hb, p.hd_d, D, p.Db);
        else
            hipLaunchKernelGGL((cross_attention_kernel<bf16, true>), grid, block, 0, st, tq, (const bf16*)kv, to, k.n_bags, bags, p.nt, p.Hb, p.hd_d, D, p.Db);
        AMDS_LAUNCH_CHECK("cross_attention_kernel<varlen>");
        return AMDS_OK;
    }
    if (dt == AMDS_F16)
        hipLaunchKernelGGL((cross_attention_kernel<f16>), grid, block, 0, st, tq, (const f16*)kv, to, k.n_bags, k.T, p.nt, p.Hb, p.hd_d, D, p.Db);
    else
        hipLaunchKernelGGL((cross_attention_kernel<bf16>), grid, block, 0, st, tq, (const bf16*)kv, to, k.n_bags, k.T, p.nt, p.Hb, p.hd_d, D, p.Db);
    AMDS_LAUNCH_CHECK("cross_attention_kernel");
    return AMDS_OK;
}

}  // namespace

// pre-norm layers on the 16-bit MFMA path, the MIL `vit` head's layer with ReLU (:188)
int bs_encoder_layer(const BsCall& k, const BsPlan& p, const amds_barspoon_cfg& c, const amds_mil_vit_layer& L, int l, const BsBufs& b, void* stream) {
    const int D = c.dim, Dp = p.Dp, dt = c.dtype, M = (int)k.M;
    AMDS_REQUIRE(enc_layer_complete(L), "%s: incomplete weights of encoder layer %d", k.who, l);
    RC(amds_layernorm(b.x, Dp, L.ln1_w, L.ln1_b, b.h, Dp, M, D, 1e-5f, dt, stream));
    RC(amds_gemm_ex(k.gemm_cfg(3 * p.Da, Dp), b.h, Dp, L.in_w, Dp, M, 3 * p.Da, Dp, dt, AMDS_EPI_BIAS, b.qkv, 3 * p.Da, L.in_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream));
    if (k.table) RC(attention_varlen_launch(b.qkv, nullptr, nullptr, b.att, k.table, k.n_bags, k.M, p.Ha, dt, (hipStream_t)stream));
    else RC(amds_attention(b.qkv, b.att, k.n_bags, k.T, p.Ha, dt, stream));
    RC(amds_gemm_ex(k.gemm_cfg(Dp, p.Da), b.att, p.Da, L.out_w, p.Da, M, Dp, p.Da, dt, AMDS_EPI_RESIDUAL, b.x, Dp, L.out_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream));
    RC(amds_layernorm(b.x, Dp, L.ln2_w, L.ln2_b, b.h, Dp, M, D, 1e-5f, dt, stream));
    RC(amds_gemm_ex(k.gemm_cfg(p.FFp, Dp), b.h, Dp, L.fc1_w, Dp, M, p.FFp, Dp, dt, AMDS_EPI_BIAS_RELU, b.u, p.FFp, L.fc1_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream));
    return amds_gemm_ex(k.gemm_cfg(Dp, p.FFp), b.u, p.FFp, L.fc2_w, p.FFp, M, Dp, p.FFp, dt, AMDS_EPI_RESIDUAL, b.x, Dp, L.fc2_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream);
}

// the class tokens, fp32 (:190-193)
int bs_decoder_layer(const BsCall& k, const BsPlan& p, const amds_barspoon_cfg& c, const amds_barspoon_dec_layer& L, int l, const BsBufs& b, void* stream) {
    const int Bb = k.n_bags, D = c.dim, Dp = p.Dp, dt = c.dtype, nt = p.nt, Hd = p.Hb, hd = p.hd_d, FF = c.ff;
    const long M2 = (long)Bb * nt;
    float *tok = b.tok, *th = b.th, *tqkv = b.tqkv, *tsc = b.tsc, *to = b.to, *tq = b.tq, *tu = b.tu;
    const float sa_scale = (float)(1.0 / sqrt((double)hd));
    AMDS_REQUIRE(L.ln1_w && L.ln1_b && L.sa_in_w && L.sa_in_b && L.sa_out_w && L.sa_out_b && L.ln2_w && L.ln2_b && L.ca_q_w && L.ca_q_b && L.ca_kv_w && L.ca_kv_b &&
                 L.ca_out_w && L.ca_out_b && L.ln3_w && L.ln3_b && L.fc1_w && L.fc1_b && L.fc2_w && L.fc2_b, "%s: incomplete weights of decoder layer %d", k.who, l);
    // t += SA(LN1(t)): self-attention among the nt class tokens of a bag
    RC(amds_layernorm(tok, D, L.ln1_w, L.ln1_b, th, D, (int)M2, D, 1e-5f, AMDS_F32, stream));
    RC(amds_linear_f32(th, L.sa_in_w, L.sa_in_b, tqkv, (int)M2, 3 * D, D, 0, stream));
    RC(bg(tqkv, 3 * D, (long)nt * 3 * D, hd, tqkv + D, 3 * D, (long)nt * 3 * D, hd, 1, tsc, nt, (long)Hd * nt * nt, (long)nt * nt, Bb, Hd, nt, nt, hd, sa_scale, nullptr, 0,
          stream));
    RC(amds_softmax_rows(tsc, (long)Bb * Hd * nt, nt, stream));
    RC(bg(tsc, nt, (long)Hd * nt * nt, (long)nt * nt, tqkv + 2 * D, 3 * D, (long)nt * 3 * D, hd, 0, to, D, (long)nt * D, hd, Bb, Hd, nt, hd, nt, 1.0f, nullptr, 0, stream));
    RC(tok_lin_acc(k, nt, to, L.sa_out_w, L.sa_out_b, tok, D, D, stream));
    // t += MHA(LN2(t), memory): queries from the class tokens, keys / values from the tile tokens
    RC(amds_layernorm(tok, D, L.ln2_w, L.ln2_b, th, D, (int)M2, D, 1e-5f, AMDS_F32, stream));
    RC(amds_linear_f32(th, L.ca_q_w, L.ca_q_b, tq, (int)M2, D, D, 0, stream));
    RC(amds_gemm_ex(k.gemm_cfg(2 * p.Db, Dp), b.h, Dp, L.ca_kv_w, Dp, (int)k.M, 2 * p.Db, Dp, dt, AMDS_EPI_BIAS, b.kv, 2 * p.Db, L.ca_kv_b, nullptr, nullptr, 0, 0, 0, 1.0f,
                    stream));
    RC(cross_attention_launch(k, p, dt, tq, b.kv, to, D, (hipStream_t)stream));
    RC(tok_lin_acc(k, nt, to, L.ca_out_w, L.ca_out_b, tok, D, D, stream));
    // t += W2 relu(W1 LN3(t))
    RC(amds_layernorm(tok, D, L.ln3_w, L.ln3_b, th, D, (int)M2, D, 1e-5f, AMDS_F32, stream));
    RC(amds_linear_f32(th, L.fc1_w, L.fc1_b, tu, (int)M2, FF, D, 1, stream));
    return tok_lin_acc(k, nt, tu, L.fc2_w, L.fc2_b, tok, D, FF, stream);
}

// target j reads its own class-token row of every bag; logits [n_bags][sum n_out], target j at its column offset (:196-203)
int bs_heads(const BsCall& k, const BsPlan& p, const amds_barspoon_cfg& c, const amds_barspoon_weights& w, const float* tok, float* logits, void* stream) {
    const int nt = p.nt, D = c.dim;
    int total_out = 0;
    for (int j = 0; j < nt; ++j) {
        AMDS_REQUIRE(w.n_out_host[j] > 0 && w.head_w_host[j] && w.head_b_host[j], "%s: head %d missing", k.who, j);
        total_out += w.n_out_host[j];
    }
    int col = 0;
    for (int j = 0; j < nt; ++j) {
        const float* t = tok + (size_t)j * D;
        const int n = w.n_out_host[j];
        if (k.table) RC(bg(t, nt * D, (long)nt * D, 0, w.head_w_host[j], D, 0, 0, 1, logits + col, total_out, total_out, 0, k.n_bags, 1, 1, n, D, 1.0f, w.head_b_host[j], 0, stream));
        else RC(bg(t, nt * D, 0, 0, w.head_w_host[j], D, 0, 0, 1, logits + col, total_out, 0, 0, 1, 1, k.n_bags, n, D, 1.0f, w.head_b_host[j], 0, stream));
        col += n;
    }
    return AMDS_OK;
}

}  // namespace amds

using namespace amds;

extern "C" size_t amds_barspoon_workspace_bytes(const amds_barspoon_cfg* cfg_host, int n_bags, int n_tiles) {
    BsPlan p;
    if (bs_plan(cfg_host, n_bags, n_tiles, &p) != AMDS_OK) return 0;
    return p.total;
}

extern "C" int amds_barspoon_forward(const amds_barspoon_cfg* cfg_host, const amds_barspoon_weights* w_host, const void* bags, int bags_dtype,
                                     const float* positions, float* logits, int n_bags, int n_tiles, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(cfg_host && w_host && bags && logits && ws, "amds_barspoon_forward: null pointer");
    const amds_barspoon_cfg& c = *cfg_host;
    const amds_barspoon_weights& w = *w_host;
    BsPlan p;
    RC(bs_plan(cfg_host, n_bags, n_tiles, &p));
    AMDS_REQUIRE(w.proj_w && w.proj_b && w.class_tokens && w.head_w_host && w.head_b_host && w.n_out_host && (c.enc_layers == 0 || w.enc_layers_host) &&
                 (c.dec_layers == 0 || w.dec_layers_host), "amds_barspoon_forward: incomplete weights");
    AMDS_REQUIRE(!c.positional_encoding || (positions && w.pe_div), "amds_barspoon_forward: positional_encoding=True needs tile positions");
    AMDS_REQUIRE(bags_dtype == AMDS_F32 || bags_dtype == AMDS_F16 || bags_dtype == AMDS_BF16, "amds_barspoon_forward: bad bags dtype %d", bags_dtype);
    if (ws_bytes < p.total) {
        set_error("amds_barspoon_forward: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_barspoon_forward: workspace must be 256-byte aligned");
    if (n_bags == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    const int D = c.dim, Dp = p.Dp, dt = c.dtype, nt = p.nt;
    const long M = (long)n_bags * n_tiles, M2 = (long)n_bags * nt;
    AMDS_REQUIRE(M < (1L << 31) - 65536, "amds_barspoon_forward: %ld tile rows do not fit the 32-bit row index", M);
    const BsBufs b = bs_bufs(ws, p);
    const BsCall k{"amds_barspoon_forward", n_bags, n_tiles, M, nullptr};

    // ---- projector: Linear + ReLU (:171), positional encodings (:173-186)
    const void* a = bags;
    if (!(bags_dtype == dt && c.n_feats == p.Fp)) {
        RC(stage_rows_dt(bags, bags_dtype, c.n_feats, base + p.a, dt, p.Fp, M, c.n_feats, stream));
        a = base + p.a;
    }
    RC(amds_gemm(a, p.Fp, w.proj_w, p.Fp, (int)M, Dp, p.Fp, dt, AMDS_EPI_BIAS_RELU_F32, b.x, Dp, w.proj_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream));
    if (c.positional_encoding) RC(pos_encoding_add(b.x, Dp, D, positions, w.pe_div, M, st));
    if (Dp != D) AMDS_HIP(hipMemsetAsync(b.h, 0, (size_t)M * Dp * 2, st));      // LayerNorm writes the first D columns only

    // ---- encoder (:188)
    for (int l = 0; l < c.enc_layers; ++l) RC(bs_encoder_layer(k, p, c, w.enc_layers_host[l], l, b, stream));
    // the encoder's output as the 16-bit A operand of every decoder layer's K / V projection (no final norm: nn.TransformerEncoder(norm=None))
    if (c.dec_layers > 0) RC(amds_cast_pad(b.x, Dp, b.h, Dp, (int)M, Dp, dt, stream));

    // ---- decoder (:190-193): the class tokens, fp32
    RC(broadcast_rows(w.class_tokens, b.tok, (long)nt * D, M2 * D, st));
    for (int l = 0; l < c.dec_layers; ++l) RC(bs_decoder_layer(k, p, c, w.dec_layers_host[l], l, b, stream));
    // ---- heads (:196-203)
    return bs_heads(k, p, c, w, b.tok, logits, stream);
}
