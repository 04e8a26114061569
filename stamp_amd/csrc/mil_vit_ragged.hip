// mil_vit_ragged.hip -- the inference forward of the MIL `vit` head over RAGGED bags: N bags of different lengths packed without padding, one call,
// each bag's logits as its own amds_mil_vit_forward call gives them.
//
// The reference has no form of this: its validation / deploy loaders run one bag per batch (src/stamp/modeling/train.py:467-477, `bag_size=None`,
// `batch_size=1`; src/stamp/modeling/deploy.py:390-456), and padding + its `mask` does not isolate bags (vision_tranformer.py:359-368 blocks a pair only when
// BOTH tokens are padded).  Layout: bag i owns tile rows offsets[i] .. offsets[i+1] - 1 of the packed [total_tiles][n_feats] tensor; its token rows, class
// token first, start at offsets[i] + i of the [total_tiles + n_bags] token-major tensors.  Everything per row (staging, GEMMs, LayerNorms) runs as in
// mil_vit.hip on those M rows; what couples rows of one bag -- attention, the class-token placement and the class-row tail -- reads the per-call table
// (attention_flash.hip, varlen_plan_kernel) built once from the device offsets.
//
// Same bits as the per-bag calls: the attention kernels are the fixed-pitch ones with a per-bag base and length; a GEMM row depends on the kernel that
// computes it, and the library's default picks the kernel by M (include/amdstamp.h, amds_gemm_ex: ids 12 / 13 differ from 0 in the last bits).  So each
// GEMM runs on the kernel the longest bag's own call would pick when that is kernel 0 (then every shorter bag's call picks it too), and by shape otherwise --
// a bag whose own call leaves kernel 0 shares a call bit-identically only when it is alone (amds_mil_vit_ragged_max_shared_tiles; the Python grouping sends it
// alone).  n_bags == 1 is the per-bag call's shape exactly.  The rule is ragged_cfg (model_call.h), shared with barspoon_ragged.hip.
#include "model_call.h"

namespace amds {

namespace {

struct RaggedPlan : PadDims {
    size_t a, x, h, qkv, att, u, xc, hc, qc, oc, cls, coords, table, total;
};

int ragged_plan(const amds_mil_vit_cfg* c, int n, long total_tiles, int max_tiles, RaggedPlan* p) {
    if (amds_mil_vit_workspace_bytes(c, 1, 1) == 0) return AMDS_ERR_INVALID;        // the config checks of amds_mil_vit_forward (message set there)
    AMDS_REQUIRE(n >= 0 && n <= 65535 && total_tiles >= 0 && max_tiles >= 0 && max_tiles < (1 << 30),
                 "amds_mil_vit_forward_ragged: bad shape n_bags=%d total_tiles=%ld max_tiles=%d", n, total_tiles, max_tiles);
    static_cast<PadDims&>(*p) = pad_dims(c->n_feats, c->dim, c->ff, c->heads);
    const size_t M = (size_t)total_tiles + n, Mt = (size_t)total_tiles;
    Arena ar;
    p->a = ar.take(Mt * p->Fp * 2);                    // staged tiles, 16-bit, zero padded columns
    p->x = ar.take(M * p->Dp * 4);                     // residual stream fp32
    p->h = ar.take(M * p->Dp * 2);                     // LayerNorm output
    p->qkv = ar.take(M * 3 * p->Da * 2);
    p->att = ar.take(M * p->Da * 2);
    p->u = ar.take(M * p->FFp * 2);
    p->xc = ar.take((size_t)n * p->Dp * 4);            // class rows, compact: residual | LayerNorm output | query | attention output
    p->hc = ar.take((size_t)n * p->Dp * 2);
    p->qc = ar.take((size_t)n * p->Da * 2);
    p->oc = ar.take((size_t)n * p->Da * 2);
    p->cls = ar.take((size_t)n * c->dim * 4);
    p->coords = ar.take(M * 2 * 4);
    p->table = ar.take(varlen_table_bytes(n, total_tiles));
    p->total = ar.off;
    return AMDS_OK;
}

// the bag owning token row r: the last bag whose first row is <= r (rows of the table ascend for well-formed offsets; for others the search still ends in range)
__device__ __forceinline__ int bag_of_row(const int2* __restrict__ bags, int n, long r) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (bags[mid].x <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// x rows: each bag's class token in front of its projected tiles; coords with the class token at (0, 0) (vision_tranformer.py:347-351).  One block per token
// row; a row no bag covers (only for malformed offsets) is left alone.  Tile row of token (bag b, s >= 1) = first token row - b + s - 1 < total_tiles.
__global__ void __launch_bounds__(128) prefix_cls_ragged_kernel(const float* __restrict__ cls, const float* __restrict__ proj, float* __restrict__ x, int Dp,
                                                                 const float* __restrict__ coords, float* __restrict__ coords_out, const int2* __restrict__ bags,
                                                                 int n) {
    const long row = blockIdx.x;
    const int b = __builtin_amdgcn_readfirstlane(bag_of_row(bags, n, row));
    const int2 bg = bags[b];
    const long s = row - bg.x;
    if (s < 0 || s >= bg.y) return;
    const long t = (long)bg.x - b + s - 1;
    const f32x4* src = reinterpret_cast<const f32x4*>(s == 0 ? cls : proj + t * Dp);
    f32x4* dst = reinterpret_cast<f32x4*>(x + row * Dp);
    for (int c = threadIdx.x; c < Dp / 4; c += 128) dst[c] = src[c];
    if (coords_out && threadIdx.x == 0) {
        float2 cw = make_float2(0.f, 0.f);
        if (s != 0) cw = *reinterpret_cast<const float2*>(coords + 2 * t);
        *reinterpret_cast<float2*>(coords_out + 2 * row) = cw;
    }
}

// class rows of x (fp32) and, when h != NULL, of the LayerNorm output h (16-bit) into the compact [n][Dp] buffers.  One block per bag.
__global__ void __launch_bounds__(128) gather_cls_kernel(const float* __restrict__ x, const uint16_t* __restrict__ h, int Dp, const int2* __restrict__ bags,
                                                          float* __restrict__ xc, uint16_t* __restrict__ hc) {
    const int b = blockIdx.x;
    const long row = __builtin_amdgcn_readfirstlane(bags[b].x);
    const f32x4* xs = reinterpret_cast<const f32x4*>(x + row * Dp);
    f32x4* xd = reinterpret_cast<f32x4*>(xc + (long)b * Dp);
    for (int c = threadIdx.x; c < Dp / 4; c += 128) xd[c] = xs[c];
    if (h) {
        const u32x4* hs = reinterpret_cast<const u32x4*>(h + row * Dp);
        u32x4* hd = reinterpret_cast<u32x4*>(hc + (long)b * Dp);
        for (int c = threadIdx.x; c < Dp / 8; c += 128) hd[c] = hs[c];
    }
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_mil_vit_ragged_workspace_bytes(const amds_mil_vit_cfg* cfg_host, int n_bags, long total_tiles, int max_tiles) {
    RaggedPlan p;
    if (!cfg_host || ragged_plan(cfg_host, n_bags, total_tiles, max_tiles, &p) != AMDS_OK) return 0;
    return p.total;
}

extern "C" int amds_mil_vit_ragged_max_shared_tiles(const amds_mil_vit_cfg* cfg_host) {
    RaggedPlan p;
    if (!cfg_host) { set_error("amds_mil_vit_ragged_max_shared_tiles: null pointer"); return -1; }
    if (ragged_plan(cfg_host, 1, 1, 1, &p) != AMDS_OK) return -1;
    // the token GEMMs of a bag of T tiles: the projection on T rows, qkv / out / fc1 / fc2 / k|v on T + 1; monotone in T
    auto shared = [&](int T) {
        return default_gemm_cfg(T, p.Dp, p.Fp) == 0 && default_gemm_cfg(T + 1, 3 * p.Da, p.Dp) == 0 && default_gemm_cfg(T + 1, 2 * p.Da, p.Dp) == 0 &&
               default_gemm_cfg(T + 1, p.Dp, p.Da) == 0 && default_gemm_cfg(T + 1, p.FFp, p.Dp) == 0 && default_gemm_cfg(T + 1, p.Dp, p.FFp) == 0;
    };
    return ragged_max_shared(shared, 32767);        // longer bags take the full last block in their own call (cls_tail, mil_vit.hip)
}

extern "C" int amds_mil_vit_forward_ragged(const amds_mil_vit_cfg* cfg_host, const amds_mil_vit_weights* w_host, const void* feats, int feats_dtype,
                                           const float* coords, const int* offsets, float* logits, int n_bags, long total_tiles, int max_tiles, void* ws,
                                           size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(cfg_host && w_host && feats && offsets && logits && ws, "amds_mil_vit_forward_ragged: null pointer");
    const amds_mil_vit_cfg& c = *cfg_host;
    const amds_mil_vit_weights& w = *w_host;
    RaggedPlan p;
    int rc = ragged_plan(cfg_host, n_bags, total_tiles, max_tiles, &p);
    if (rc != AMDS_OK) return rc;
    AMDS_REQUIRE(w.class_token && w.proj_w && w.proj_b && w.norm_w && w.norm_b && w.head_w && (c.layers == 0 || w.layers_host),
                 "amds_mil_vit_forward_ragged: incomplete weights");
    AMDS_REQUIRE(!c.alibi || coords, "amds_mil_vit_forward_ragged: use_alibi=True needs coords");
    AMDS_REQUIRE(feats_dtype == AMDS_F32 || feats_dtype == AMDS_F16 || feats_dtype == AMDS_BF16, "amds_mil_vit_forward_ragged: bad feats dtype %d", feats_dtype);
    const long M = total_tiles + n_bags, Mt = total_tiles;
    AMDS_REQUIRE(M * (long)p.FFp < (1L << 40) && M < (1L << 31), "amds_mil_vit_forward_ragged: %ld token rows do not fit the 32-bit row index", M);
    AMDS_REQUIRE(FA_SPAN_OK(max_tiles + 1, p.Ha), "amds_mil_vit_forward_ragged: max_tiles=%d: a bag's q | k | v rows exceed the 2 GB of a buffer descriptor",
                 max_tiles);
    if (ws_bytes < p.total) {
        set_error("amds_mil_vit_forward_ragged: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_mil_vit_forward_ragged: workspace must be 256-byte aligned");
    if (n_bags == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    const int Bn = n_bags, D = c.dim, Dp = p.Dp, dt = c.dtype;
    const long S = (long)max_tiles + 1;             // token rows of the longest bag
    float* x = reinterpret_cast<float*>(base + p.x);
    void* h = base + p.h;
    void* qkv = base + p.qkv;
    void* att = base + p.att;
    void* u = base + p.u;
    float* xc = reinterpret_cast<float*>(base + p.xc);
    void* hc = base + p.hc;
    void* qc = base + p.qc;
    void* oc = base + p.oc;
    float* cls = reinterpret_cast<float*>(base + p.cls);
    float* cw = c.alibi ? reinterpret_cast<float*>(base + p.coords) : nullptr;
    void* table = base + p.table;
    const int2* bags = varlen_table_bags(table);

    if ((rc = varlen_table_build(offsets, Bn, total_tiles, max_tiles, 1, table, st)) != AMDS_OK) return rc;
    // project_features (as mil_vit.hip)
    const void* a = feats;
    if (Mt > 0 && !(feats_dtype == dt && c.n_feats == p.Fp)) {
        if ((rc = stage_rows_dt(feats, feats_dtype, c.n_feats, base + p.a, dt, p.Fp, Mt, c.n_feats, stream)) != AMDS_OK) return rc;
        a = base + p.a;
    }
    float* proj = reinterpret_cast<float*>(qkv);
    if ((rc = amds_gemm_ex(ragged_cfg(Bn, max_tiles, p.Dp, p.Fp), a, p.Fp, w.proj_w, p.Fp, (int)Mt, Dp, p.Fp, dt, AMDS_EPI_BIAS_GELU_F32, proj, Dp, w.proj_b,
                           nullptr, nullptr, 0, 0, 0, 1.0f, stream)) != AMDS_OK) return rc;
    hipLaunchKernelGGL(prefix_cls_ragged_kernel, dim3((unsigned)M), dim3(128), 0, st, w.class_token, proj, x, Dp, coords, cw, bags, Bn);
    AMDS_LAUNCH_CHECK("prefix_cls_ragged_kernel");
    if (Dp != D) AMDS_HIP(hipMemsetAsync(h, 0, (size_t)M * Dp * 2, st));      // LayerNorm writes the first D columns only

    // the class-row tail exactly where every bag's own call takes it: ALiBi never; otherwise when the longest bag has S <= 32768 tokens (a longer bag is sent
    // alone by the host, so its own call and this one agree)
    const bool cls_tail = ctx_mil_cls_tail() && !c.alibi && S <= 32768;
    const int cq = ragged_cfg(Bn, 1, p.Da, p.Dp), co = ragged_cfg(Bn, 1, Dp, p.Da), c1 = ragged_cfg(Bn, 1, p.FFp, Dp), c2 = ragged_cfg(Bn, 1, Dp, p.FFp);
    bool tail_done = false;
    for (int l = 0; l < c.layers && rc == AMDS_OK; ++l) {
        const amds_mil_vit_layer& L = w.layers_host[l];
        AMDS_REQUIRE(enc_layer_complete(L) && (!c.alibi || L.head_scale), "amds_mil_vit_forward_ragged: incomplete weights of layer %d", l);
        if ((rc = amds_layernorm(x, Dp, L.ln1_w, L.ln1_b, h, Dp, (int)M, D, 1e-5f, dt, stream)) != AMDS_OK) break;
        if (cls_tail && l == c.layers - 1) {
            // keys | values of every token; query, attention, output projection and MLP of the class rows alone, gathered into compact buffers
            const int esz = 2;
            const char* w_kv = reinterpret_cast<const char*>(L.in_w) + (size_t)p.Da * Dp * esz;
            char* qkv_kv = reinterpret_cast<char*>(qkv) + (size_t)p.Da * esz;
            if ((rc = amds_gemm_ex(ragged_cfg(Bn, S, 2 * p.Da, Dp), h, Dp, w_kv, Dp, (int)M, 2 * p.Da, Dp, dt, AMDS_EPI_BIAS, qkv_kv, 3 * p.Da, L.in_b + p.Da,
                                   nullptr, nullptr, 0, 0, 0, 1.0f, stream)) != AMDS_OK) break;
            hipLaunchKernelGGL(gather_cls_kernel, dim3(Bn), dim3(128), 0, st, x, (const uint16_t*)h, Dp, bags, xc, (uint16_t*)hc);
            AMDS_LAUNCH_CHECK("gather_cls_kernel");
            if ((rc = amds_gemm_ex(cq, hc, Dp, L.in_w, Dp, Bn, p.Da, Dp, dt, AMDS_EPI_BIAS, qc, p.Da, L.in_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream)) != AMDS_OK) break;
            if ((rc = attention_row_varlen_launch(qc, p.Da, qkv, oc, p.Da, table, Bn, max_tiles, p.Ha, dt, st)) != AMDS_OK) break;
            if ((rc = amds_gemm_ex(co, oc, p.Da, L.out_w, p.Da, Bn, Dp, p.Da, dt, AMDS_EPI_RESIDUAL, xc, Dp, L.out_b, nullptr, nullptr, 0, 0, 0, 1.0f,
                                   stream)) != AMDS_OK) break;
            if ((rc = amds_layernorm(xc, Dp, L.ln2_w, L.ln2_b, hc, Dp, Bn, D, 1e-5f, dt, stream)) != AMDS_OK) break;
            if ((rc = amds_gemm_ex(c1, hc, Dp, L.fc1_w, Dp, Bn, p.FFp, Dp, dt, AMDS_EPI_BIAS_GELU, u, p.FFp, L.fc1_b, nullptr, nullptr, 0, 0, 0, 1.0f,
                                   stream)) != AMDS_OK) break;
            rc = amds_gemm_ex(c2, u, p.FFp, L.fc2_w, p.FFp, Bn, Dp, p.FFp, dt, AMDS_EPI_RESIDUAL, xc, Dp, L.fc2_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream);
            tail_done = true;
            continue;
        }
        if ((rc = amds_gemm_ex(ragged_cfg(Bn, S, 3 * p.Da, Dp), h, Dp, L.in_w, Dp, (int)M, 3 * p.Da, Dp, dt, AMDS_EPI_BIAS, qkv, 3 * p.Da, L.in_b, nullptr,
                               nullptr, 0, 0, 0, 1.0f, stream)) != AMDS_OK) break;
        rc = c.alibi ? attention_varlen_launch(qkv, cw, L.head_scale, att, table, Bn, total_tiles, p.Ha, dt, st)
                     : attention_varlen_launch(qkv, nullptr, nullptr, att, table, Bn, total_tiles, p.Ha, dt, st);
        if (rc != AMDS_OK) break;
        if ((rc = amds_gemm_ex(ragged_cfg(Bn, S, Dp, p.Da), att, p.Da, L.out_w, p.Da, (int)M, Dp, p.Da, c.alibi ? AMDS_BF16 : dt, AMDS_EPI_RESIDUAL, x, Dp,
                               L.out_b, nullptr, nullptr, 0, 0, 0, 1.0f, stream)) != AMDS_OK) break;
        if ((rc = amds_layernorm(x, Dp, L.ln2_w, L.ln2_b, h, Dp, (int)M, D, 1e-5f, dt, stream)) != AMDS_OK) break;
        if ((rc = amds_gemm_ex(ragged_cfg(Bn, S, p.FFp, Dp), h, Dp, L.fc1_w, Dp, (int)M, p.FFp, Dp, dt, AMDS_EPI_BIAS_GELU, u, p.FFp, L.fc1_b, nullptr, nullptr,
                               0, 0, 0, 1.0f, stream)) != AMDS_OK) break;
        rc = amds_gemm_ex(ragged_cfg(Bn, S, Dp, p.FFp), u, p.FFp, L.fc2_w, p.FFp, (int)M, Dp, p.FFp, dt, AMDS_EPI_RESIDUAL, x, Dp, L.fc2_b, nullptr, nullptr, 0,
                          0, 0, 1.0f, stream);
    }
    if (rc != AMDS_OK) return rc;
    if (!tail_done) {
        hipLaunchKernelGGL(gather_cls_kernel, dim3(Bn), dim3(128), 0, st, x, (const uint16_t*)nullptr, Dp, bags, xc, (uint16_t*)nullptr);
        AMDS_LAUNCH_CHECK("gather_cls_kernel");
    }
    // final LayerNorm on the class rows, then the head in exact fp32
    if ((rc = amds_layernorm(xc, Dp, w.norm_w, w.norm_b, cls, D, Bn, D, 1e-5f, AMDS_F32, stream)) != AMDS_OK) return rc;
    return amds_linear_f32(cls, w.head_w, w.head_b, logits, Bn, c.classes, D, 0, stream);
}
