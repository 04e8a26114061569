// abmil.hip -- the gated-attention MIL head (CHIEF's CHIEFModel as a classifier, a CLAM-SB style attention-MIL network): eval forward, training forward and
// backward, one call each, ragged by construction (x [total_rows][F], device row_offsets int64 [bags + 1]).
//
// Reference: src/stamp/encoding/encoder/chief.py:27-89 (CHIEFModel: Linear(F, L) -> ReLU -> Dropout(0.25) -> Attn_Net_Gated; softmax over the tiles, :77-79;
// WSI_feature_transformed = A @ h, :80; classifiers = Linear(L, n_classes), :56) and :255-275 (Attn_Net_Gated: tanh and sigmoid branches, each with Dropout(0.25),
// their product through Linear(D, 1)); the backward is what autograd derives from cross_entropy(classifiers(WSI_feature_transformed)).
//
// Per row the head is three products (fc; a | b as ONE stacked [2D][L] product; their dx / dW forms in the backward) -- those go through amds_bgemm_f32, so the
// head follows amds_set_matmul_precision like TransMIL.  What couples the rows of a bag lives in the kernels below: gate + dropouts + score per row, softmax over
// the bag's rows, pooling of h, the classifier rows, and the backward of those.  No floating-point atomics: every sum is a lane butterfly, an in-order loop or a
// fixed-order merge of per-wave partials, so a call is reproducible bit for bit.
//
// Batch independence of the eval forward: amds_bgemm_f32 picks its kernel by M (bgemm_f32_row_class, transmil.hip).  Every product of the forwards therefore runs
// on the call's rows padded with zero rows to a multiple of AB_ROW_PAD = 256: M is then always >= 96, > 64 and a multiple of 64 / 128 / 256 -- ONE row class
// whatever the call holds --, and a row's bits depend on (N, K) alone.  Everything else of the forward is per row or per bag.  There is no shared-length limit.
//
// Dropout sites (header): stream ids 1 (h), 2 (a), 3 (g); element index row * cols + col over the call's packed rows.
#include <algorithm>
#include "model_call.h"

namespace amds {
namespace {
constexpr int AB_ROW_PAD = 256;
constexpr uint32_t AB_SID_H = 1, AB_SID_A = 2, AB_SID_G = 3;

struct AbDims { int F, L, D, C, bags; long rows, rows_p; };

int ab_dims(const amds_abmil_cfg* c, int bags, long rows, AbDims* d, const char* who) {
    AMDS_REQUIRE(c, "%s: null config", who);
    AMDS_REQUIRE(c->n_feats >= 1 && c->L >= 1 && c->D >= 1 && c->classes >= 1, "%s: bad config n_feats=%d L=%d D=%d classes=%d (every width must be >= 1)", who,
                 c->n_feats, c->L, c->D, c->classes);
    AMDS_REQUIRE(c->n_feats <= 65536 && c->L <= 65536 && c->D <= 32768 && c->classes <= 65536,
                 "%s: bad config n_feats=%d L=%d D=%d classes=%d (n_feats, L, classes <= 65536, D <= 32768)", who, c->n_feats, c->L, c->D, c->classes);
    AMDS_REQUIRE((long)2 * c->D * c->L <= (1L << 30) && (long)c->L * c->n_feats <= (1L << 30), "%s: L=%d with n_feats=%d, D=%d (a weight matrix holds at most 2^30 elements)",
                 who, c->L, c->n_feats, c->D);
    AMDS_REQUIRE(bags >= 1 && bags <= (1 << 24), "%s: bags=%d (1 <= bags <= 2^24)", who, bags);
    AMDS_REQUIRE(rows >= bags, "%s: total_rows=%ld < bags=%d (every bag holds at least one row)", who, rows, bags);
    AMDS_REQUIRE(rows <= 65535L * 64 - AB_ROW_PAD, "%s: total_rows=%ld (at most 65535 * 64 - %d rows a call: one launch's row tiles)", who, rows, AB_ROW_PAD);
    d->F = c->n_feats; d->L = c->L; d->D = c->D; d->C = c->classes; d->bags = bags; d->rows = rows; d->rows_p = round_up(rows, (long)AB_ROW_PAD);
    return AMDS_OK;
}

// the stacked gate operand every call builds in its workspace: [2D][L] weights (a above b) and [2D] biases
struct AbStack { size_t wab, bab; };
// eval workspace: staged rows, h, the gate branches, scores, probabilities, the pooled rows
struct AbEvalWs { size_t xs, h, ab, s, p, m; AbStack k; size_t total; };
void ab_eval_ws(const AbDims& d, AbEvalWs* w) {
    Arena ar;
    w->xs = ar.take((size_t)d.rows_p * d.F * 4); w->h = ar.take((size_t)d.rows_p * d.L * 4); w->ab = ar.take((size_t)d.rows_p * 2 * d.D * 4);
    w->s = ar.take((size_t)d.rows * 4); w->p = ar.take((size_t)d.rows * 4); w->m = ar.take((size_t)d.bags * d.L * 4);
    w->k.wab = ar.take((size_t)2 * d.D * d.L * 4); w->k.bab = ar.take((size_t)2 * d.D * 4);
    w->total = ar.off;
}
// heat-map workspace: the eval workspace, then r [rows_p][L] and the bag of every row
struct AbHeatWs { AbEvalWs e; size_t r, rowbag, total; };
void ab_heat_ws(const AbDims& d, AbHeatWs* w) {
    ab_eval_ws(d, &w->e);
    Arena ar;
    ar.off = w->e.total;
    w->r = ar.take((size_t)d.rows_p * d.L * 4); w->rowbag = ar.take((size_t)d.rows * 4);
    w->total = ar.off;
}
// saved state of a training forward: h (after ReLU and dropout), tanh | sigmoid BEFORE their dropouts, score and probability per row; the pooled row per bag
struct AbSaved { size_t h, tg, s, p, m, total; };
void ab_saved(const AbDims& d, AbSaved* s) {
    Arena ar;
    s->h = ar.take((size_t)d.rows_p * d.L * 4); s->tg = ar.take((size_t)d.rows_p * 2 * d.D * 4);
    s->s = ar.take((size_t)d.rows * 4); s->p = ar.take((size_t)d.rows * 4); s->m = ar.take((size_t)d.bags * d.L * 4);
    s->total = ar.off;
}
// The weight-gradient products sum over every row of the call.  As ONE product with K = rows_p their few output tiles ([L][F], [2D][L]) leave most CUs idle (the
// finding behind transmil_core._wgrad), so the rows are cut into chunks of kc rows -- at most 32 of them, kc a multiple of 256 fixed by rows_p alone --, one product
// per chunk into fp32 partials (a batched launch for the whole chunks, one more for a shorter last chunk), then a fixed-order sum over the chunks (amds_colsum).
struct AbSplit { int kc, n_full, tail, parts; };
AbSplit ab_split(long rows_p) {
    AbSplit sp;
    sp.kc = (int)std::max<long>(AB_ROW_PAD, round_up((rows_p + 31) / 32, (long)AB_ROW_PAD));
    sp.n_full = (int)(rows_p / sp.kc);
    sp.tail = (int)(rows_p - (long)sp.n_full * sp.kc);
    sp.parts = sp.n_full + (sp.tail ? 1 : 0);
    return sp;
}
// training workspace: the forward needs xs and the stack; the backward xs, the stack, dab, dh, g, ds, rowbag, dM, the dw_c products, the weight-gradient partials
// and column-sum scratch
struct AbTrainWs { size_t xs, dab, dh, g, ds, rowbag, dm, prod, part, cs; AbStack k; size_t total, cs_bytes; };
void ab_train_ws(const AbDims& d, AbTrainWs* w) {
    Arena ar;
    const AbSplit sp = ab_split(d.rows_p);
    const size_t wmax = std::max((size_t)2 * d.D * d.L, (size_t)d.L * d.F);
    w->xs = ar.take((size_t)d.rows_p * d.F * 4);
    w->k.wab = ar.take((size_t)2 * d.D * d.L * 4); w->k.bab = ar.take((size_t)2 * d.D * 4);
    w->dab = ar.take((size_t)d.rows_p * 2 * d.D * 4); w->dh = ar.take((size_t)d.rows_p * d.L * 4);
    w->g = ar.take((size_t)d.rows * 4); w->ds = ar.take((size_t)d.rows * 4); w->rowbag = ar.take((size_t)d.rows * 4);
    w->dm = ar.take((size_t)d.bags * d.L * 4); w->prod = ar.take((size_t)d.rows * d.D * 4); w->part = ar.take((size_t)sp.parts * wmax * 4);
    size_t cs = amds_colsum_workspace_bytes((int)d.rows_p, std::max(d.L, d.D));
    cs = std::max(cs, wmax * 4);                                   // (up to 33 partials are one chunk of amds_colsum: its check asks for one row of columns)
    w->cs_bytes = std::max<size_t>(cs, 4); w->cs = ar.take(w->cs_bytes);
    w->total = ar.off;
}

// ---- staging: [rows][F] of any float type -> fp32 [rows_p][F], the padding rows zero ------------------------------------------------------------------------
template <typename TI>
__global__ void __launch_bounds__(256) ab_stage_kernel(const TI* __restrict__ src, float* __restrict__ dst, long n_real, long n_all) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n_all; i += stride) dst[i] = i < n_real ? (float)src[i] : 0.f;
}
// h = drop_1(relu(z)) in place over [rows_p][L]; the padding rows (relu(b_fc) after the product) are set to zero
__global__ void __launch_bounds__(256) ab_relu_drop_kernel(float* __restrict__ h, long n_real, long n_all, uint64_t seed, uint32_t thr, float scale) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n_all; i += stride) {
        float v = 0.f;
        if (i < n_real) {
            v = fmaxf(h[i], 0.f);
            if (thr) v = drop_keep_flat(seed, AB_SID_H, i, thr) ? v * scale : 0.f;
        }
        h[i] = v;
    }
}
// One wave per row: t = tanh(u), q = sigmoid(v) written back over the pre-activations [rows][2D] (what the backward reads), a = drop_2(t), g = drop_3(q),
// s = w_c . (a o g) + b_c.  Lanes own columns d = lane, lane + 64, ...; the 64 partial sums merge in a fixed xor butterfly.
__global__ void __launch_bounds__(256) ab_gate_score_kernel(float* __restrict__ ab, const float* __restrict__ wc, const float* __restrict__ bc, float* __restrict__ s,
                                                            long rows, int D, uint64_t seed, uint32_t thr, float scale) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                   // (whole waves leave together; no barrier below)
    float* row = ab + r * 2 * D;
    float acc = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float t = tanhf(row[d]);
        const float q = 1.0f / (1.0f + expf(-row[D + d]));
        row[d] = t; row[D + d] = q;
        float a = t, g = q;
        if (thr) {
            const long idx = r * D + d;
            a = drop_keep_flat(seed, AB_SID_A, idx, thr) ? t * scale : 0.f;
            g = drop_keep_flat(seed, AB_SID_G, idx, thr) ? q * scale : 0.f;
        }
        acc = fmaf(wc[d], a * g, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) s[r] = acc + bc[0];
}

__device__ __forceinline__ void ab_bag_range(const long long* __restrict__ offs, int b, int bags, long rows, long* n0, long* n1) {
    long a = offs ? (long)offs[b] : 0, e = offs ? (long)offs[b + 1] : rows;      // (offs NULL: one bag)
    a = a < 0 ? 0 : (a > rows ? rows : a);
    e = e < a ? a : (e > rows ? rows : e);
    *n0 = a; *n1 = e;
}
// sum over the block's 256 threads in a fixed order: the wave butterfly, then the four wave totals added 0 + 1 + 2 + 3; every thread gets the result
__device__ __forceinline__ float ab_block_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ float ab_block_max(float v, float* sh) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
// One workgroup per bag: P = softmax over the bag's scores (chief.py:79).  Depends on the bag's own rows alone.
__global__ void __launch_bounds__(256) ab_softmax_bag_kernel(const float* __restrict__ s, float* __restrict__ p, const long long* __restrict__ offs, int bags, long rows) {
    __shared__ float sh[4];
    long n0, n1;
    ab_bag_range(offs, blockIdx.x, bags, rows, &n0, &n1);
    float mx = -INFINITY;
    for (long n = n0 + threadIdx.x; n < n1; n += 256) mx = fmaxf(mx, s[n]);
    mx = ab_block_max(mx, sh);
    float sum = 0.f;
    for (long n = n0 + threadIdx.x; n < n1; n += 256) sum += expf(s[n] - mx);
    sum = ab_block_sum(sum, sh);
    for (long n = n0 + threadIdx.x; n < n1; n += 256) p[n] = expf(s[n] - mx) / sum;
}
// M[b][l] = sum_n P_n h[n][l]: a workgroup owns 64 columns of one bag; its four waves take the rows n0 + w, n0 + w + 4, ... in order and merge 0 + 1 + 2 + 3.
__global__ void __launch_bounds__(256) ab_pool_kernel(const float* __restrict__ p, const float* __restrict__ h, float* __restrict__ m, const long long* __restrict__ offs,
                                                      int bags, long rows, int L) {
    __shared__ float sh[4][64];
    long n0, n1;
    ab_bag_range(offs, blockIdx.x, bags, rows, &n0, &n1);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = blockIdx.y * 64 + lane;
    float acc = 0.f;
    if (col < L)
        for (long n = n0 + w; n < n1; n += 4) acc = fmaf(p[n], h[n * L + col], acc);
    sh[w][lane] = acc;
    __syncthreads();
    if (w == 0 && col < L) m[(long)blockIdx.x * L + col] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}
// logits[b][c] = W_cls[c] . M[b] + b_cls[c]: one wave per output
__global__ void __launch_bounds__(256) ab_classifier_kernel(const float* __restrict__ m, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out,
                                                            long n_out, int C, int L) {
    const int lane = threadIdx.x & 63;
    const long o = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;
    const long b = o / C;
    const int c = (int)(o - b * C);
    float acc = 0.f;
    for (int l = lane; l < L; l += 64) acc = fmaf(w[(long)c * L + l], m[b * L + l], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[o] = acc + bias[c];
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------------------------------
// dM[b][l] = sum_c dlogits[b][c] W_cls[c][l]
__global__ void __launch_bounds__(256) ab_dpool_kernel(const float* __restrict__ dlg, const float* __restrict__ w, float* __restrict__ dm, long n, int C, int L) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long b = i / L;
    const int l = (int)(i - b * L);
    float acc = 0.f;
    for (int c = 0; c < C; ++c) acc = fmaf(dlg[b * C + c], w[(long)c * L + l], acc);
    dm[i] = acc;
}
// dW_cls[c][l] = sum_b dlogits[b][c] M[b][l] (i < C L) and db_cls[c] = sum_b dlogits[b][c] (C L <= i < C L + C), bags in order
__global__ void __launch_bounds__(256) ab_cls_grad_kernel(const float* __restrict__ dlg, const float* __restrict__ m, float* __restrict__ dw, float* __restrict__ db, int bags,
                                                          int C, int L) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long CL = (long)C * L;
    if (i >= CL + C) return;
    float acc = 0.f;
    if (i < CL) {
        const int c = (int)(i / L), l = (int)(i - (long)c * L);
        for (int b = 0; b < bags; ++b) acc = fmaf(dlg[(long)b * C + c], m[(long)b * L + l], acc);
        dw[i] = acc;
    } else {
        const int c = (int)(i - CL);
        for (int b = 0; b < bags; ++b) acc += dlg[(long)b * C + c];
        db[c] = acc;
    }
}
__global__ void __launch_bounds__(256) ab_rowbag_kernel(int* __restrict__ rowbag, const long long* __restrict__ offs, int bags, long rows) {
    long n0, n1;
    ab_bag_range(offs, blockIdx.x, bags, rows, &n0, &n1);
    for (long n = n0 + threadIdx.x; n < n1; n += 256) rowbag[n] = blockIdx.x;
}
// g_n = h_n . dM_bag(n): one wave per row
__global__ void __launch_bounds__(256) ab_rowdot_kernel(const float* __restrict__ h, const float* __restrict__ dm, const int* __restrict__ rowbag, float* __restrict__ g,
                                                        long rows, int L) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* hr = h + r * L;
    const float* dr = dm + (long)rowbag[r] * L;
    float acc = 0.f;
    for (int l = lane; l < L; l += 64) acc = fmaf(hr[l], dr[l], acc);
    acc = wave_sum(acc);
    if (lane == 0) g[r] = acc;
}
// One workgroup per bag: ds_n = P_n (g_n - sum_k P_k g_k), the softmax's backward
__global__ void __launch_bounds__(256) ab_dscore_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ ds, const long long* __restrict__ offs,
                                                        int bags, long rows) {
    __shared__ float sh[4];
    long n0, n1;
    ab_bag_range(offs, blockIdx.x, bags, rows, &n0, &n1);
    float acc = 0.f;
    for (long n = n0 + threadIdx.x; n < n1; n += 256) acc = fmaf(p[n], g[n], acc);
    acc = ab_block_sum(acc, sh);
    for (long n = n0 + threadIdx.x; n < n1; n += 256) ds[n] = p[n] * (g[n] - acc);
}
// One wave per row of [rows_p]: the gate's derivatives with the masks drawn again, into dab [rows_p][2D] (zero on the padding rows: dab is an operand of
// products over rows_p), and prod[r][d] = ds_r a g (the summands of dw_c) where asked for.
__global__ void __launch_bounds__(256) ab_gate_bwd_kernel(const float* __restrict__ tg, const float* __restrict__ ds, const float* __restrict__ wc, float* __restrict__ dab,
                                                          float* __restrict__ prod, long rows, long rows_p, int D, uint64_t seed, uint32_t thr, float scale) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows_p) return;
    float* out = dab + r * 2 * D;
    if (r >= rows) {
        for (int d = lane; d < 2 * D; d += 64) out[d] = 0.f;
        return;
    }
    const float* row = tg + r * 2 * D;
    const float dsr = ds[r];
    for (int d = lane; d < D; d += 64) {
        const float t = row[d], q = row[D + d];
        float ma = 1.f, mg = 1.f;
        if (thr) {
            const long idx = r * D + d;
            ma = drop_keep_flat(seed, AB_SID_A, idx, thr) ? scale : 0.f;
            mg = drop_keep_flat(seed, AB_SID_G, idx, thr) ? scale : 0.f;
        }
        const float a = t * ma, g = q * mg;
        const float dsw = dsr * wc[d];
        out[d] = dsw * g * ma * (1.f - t * t);
        out[D + d] = dsw * a * mg * q * (1.f - q);
        if (prod) prod[r * D + d] = dsr * (a * g);
    }
}
// dz = [h > 0] scale_1 (dh + P_n dM_bag(n)) in place over [rows_p][L] (h > 0 <=> kept and past the ReLU); zero on the padding rows
__global__ void __launch_bounds__(256) ab_dh_finish_kernel(float* __restrict__ dh, const float* __restrict__ h, const float* __restrict__ p, const float* __restrict__ dm,
                                                           const int* __restrict__ rowbag, long rows, long n_all, int L, float scale) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n_all; i += stride) {
        const long r = i / L;
        float v = 0.f;
        if (r < rows && h[i] > 0.f) {
            const int l = (int)(i - r * L);
            v = fmaf(p[r], dm[(long)rowbag[r] * L + l], dh[i]) * scale;
        }
        dh[i] = v;
    }
}

// ---- heat map (amds_abmil_heatmap) --------------------------------------------------------------------------------------------------------------------------------
// 16 bytes a lane where a row's pitch allows it.  ALIGNED = false: the tensor is a caller's weight (no alignment asked of it), four 4-byte loads.
template <bool ALIGNED>
__device__ __forceinline__ float4 ab_ld4(const float* p) {
    if constexpr (ALIGNED) return *reinterpret_cast<const float4*>(p);
    else return make_float4(p[0], p[1], p[2], p[3]);
}
// One wave per row of [rows_p]: the gate vectors u = w_c o q o (1 - t^2) | v = w_c o t o q o (1 - q) written over the saved t | q (eval: no masks); zero on the
// padding rows -- the buffer is an operand of a product over rows_p.  VEC (D % 4 == 0): lanes own four consecutive columns.
template <bool VEC>
__global__ void __launch_bounds__(256) ab_cam_gate_kernel(float* __restrict__ tq, const float* __restrict__ wc, long rows, long rows_p, int D) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows_p) return;
    float* row = tq + r * 2 * D;
    if (r >= rows) {
        for (int d = lane; d < 2 * D; d += 64) row[d] = 0.f;
        return;
    }
    if constexpr (VEC) {
        for (int d = lane * 4; d < D; d += 256) {
            const float4 t = *reinterpret_cast<const float4*>(row + d), q = *reinterpret_cast<const float4*>(row + D + d), w = ab_ld4<false>(wc + d);
            *reinterpret_cast<float4*>(row + d) = make_float4(w.x * q.x * (1.f - t.x * t.x), w.y * q.y * (1.f - t.y * t.y), w.z * q.z * (1.f - t.z * t.z), w.w * q.w * (1.f - t.w * t.w));
            *reinterpret_cast<float4*>(row + D + d) = make_float4(w.x * t.x * q.x * (1.f - q.x), w.y * t.y * q.y * (1.f - q.y), w.z * t.z * q.z * (1.f - q.z), w.w * t.w * q.w * (1.f - q.w));
        }
    } else {
        for (int d = lane; d < D; d += 64) {
            const float t = row[d], q = row[D + d], w = wc[d];
            row[d] = w * q * (1.f - t * t);
            row[D + d] = w * t * q * (1.f - q);
        }
    }
}
// The three sums of one row for NC classes c0 .. c0 + NC - 1: B = e . r (first group only), A_c = e . W_cls[c], G_c = (h - M) . W_cls[c] with
// e = (h - b_fc) o [h > 0].  Lanes own columns l = 4 lane + 256 k (VEC) or lane + 64 k, each sum in that order, then the wave butterfly.
constexpr int AB_CAM_CG = 4;          // classes per pass over a row
template <int NC, bool VEC, bool WAL>
__device__ __forceinline__ void ab_cam_pass(const float* __restrict__ hr, const float* __restrict__ rr, const float* __restrict__ mb, const float* __restrict__ bf,
                                            const float* __restrict__ W, int L, int lane, bool first, float* B, float (&A)[AB_CAM_CG], float (&G)[AB_CAM_CG]) {
    float b = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) A[c] = G[c] = 0.f;
    if constexpr (VEC) {
        for (int l = lane * 4; l < L; l += 256) {
            const float4 hv = *reinterpret_cast<const float4*>(hr + l), mv = *reinterpret_cast<const float4*>(mb + l), bv = ab_ld4<WAL>(bf + l);
            const float e0 = hv.x > 0.f ? hv.x - bv.x : 0.f, e1 = hv.y > 0.f ? hv.y - bv.y : 0.f, e2 = hv.z > 0.f ? hv.z - bv.z : 0.f, e3 = hv.w > 0.f ? hv.w - bv.w : 0.f;
            if (first) {
                const float4 rv = *reinterpret_cast<const float4*>(rr + l);
                b = fmaf(e0, rv.x, b); b = fmaf(e1, rv.y, b); b = fmaf(e2, rv.z, b); b = fmaf(e3, rv.w, b);
            }
            const float d0 = hv.x - mv.x, d1 = hv.y - mv.y, d2 = hv.z - mv.z, d3 = hv.w - mv.w;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float4 wv = ab_ld4<WAL>(W + (long)c * L + l);
                A[c] = fmaf(e0, wv.x, A[c]); A[c] = fmaf(e1, wv.y, A[c]); A[c] = fmaf(e2, wv.z, A[c]); A[c] = fmaf(e3, wv.w, A[c]);
                G[c] = fmaf(d0, wv.x, G[c]); G[c] = fmaf(d1, wv.y, G[c]); G[c] = fmaf(d2, wv.z, G[c]); G[c] = fmaf(d3, wv.w, G[c]);
            }
        }
    } else {
        for (int l = lane; l < L; l += 64) {
            const float hv = hr[l];
            const float e = hv > 0.f ? hv - bf[l] : 0.f, dm = hv - mb[l];
            if (first) b = fmaf(e, rr[l], b);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float wv = W[(long)c * L + l];
                A[c] = fmaf(e, wv, A[c]);
                G[c] = fmaf(dm, wv, G[c]);
            }
        }
    }
    if (first) *B = wave_sum(b);
#pragma unroll
    for (int c = 0; c < NC; ++c) { A[c] = wave_sum(A[c]); G[c] = wave_sum(G[c]); }
}
// One wave per row (a workgroup's four waves walk the rows 4 blockIdx + w, + 4 gridDim, ...): cam_raw[c][n] = | P_n (A_nc + G_nc B_n) | / F for every class, the
// classes in groups of AB_CAM_CG and a remainder.  G_nc = W_cls[c] . (h_n - M_bag(n)) is g_nc - gbar_c with gbar taken from the POOLED row, the difference formed
// per element before the dot.  LDSW: W_cls [C][L] and b_fc [L] staged in LDS once per workgroup (b_fc is then read from memory once per thread); otherwise both
// are read through the caches.  VEC: L % 4 == 0, 16-byte reads of h, r and M (workspace rows, 16-byte aligned then) and of the LDS copies.
template <bool VEC, bool LDSW>
__global__ void __launch_bounds__(256) ab_cam_kernel(const float* __restrict__ h, const float* __restrict__ rr, const float* __restrict__ p, const float* __restrict__ m,
                                                     const int* __restrict__ rowbag, const float* __restrict__ bfc, const float* __restrict__ wcls, float* __restrict__ cam,
                                                     long rows, int L, int C, float n_feats) {
    extern __shared__ __align__(16) float ab_cam_lds[];
    const float *W = wcls, *bf = bfc;
    if constexpr (LDSW) {
        const long CL = (long)C * L;
        for (long i = threadIdx.x; i < CL; i += 256) ab_cam_lds[i] = wcls[i];
        for (int i = threadIdx.x; i < L; i += 256) ab_cam_lds[CL + i] = bfc[i];
        __syncthreads();
        W = ab_cam_lds; bf = ab_cam_lds + CL;
    }
    const int lane = threadIdx.x & 63;
    for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {          // (no barrier inside: waves run free)
        const float *hr = h + r * L, *rrow = rr + r * L, *mb = m + (long)rowbag[r] * L;
        const float pn = p[r];
        float B = 0.f, A[AB_CAM_CG], G[AB_CAM_CG];
        for (int c0 = 0; c0 < C; c0 += AB_CAM_CG) {
            const int nc = min(AB_CAM_CG, C - c0);
            const float* Wc = W + (long)c0 * L;
            if (nc == 4) ab_cam_pass<4, VEC, VEC && LDSW>(hr, rrow, mb, bf, Wc, L, lane, c0 == 0, &B, A, G);
            else if (nc == 3) ab_cam_pass<3, VEC, VEC && LDSW>(hr, rrow, mb, bf, Wc, L, lane, c0 == 0, &B, A, G);
            else if (nc == 2) ab_cam_pass<2, VEC, VEC && LDSW>(hr, rrow, mb, bf, Wc, L, lane, c0 == 0, &B, A, G);
            else ab_cam_pass<1, VEC, VEC && LDSW>(hr, rrow, mb, bf, Wc, L, lane, c0 == 0, &B, A, G);
            if (lane < nc) {
                float a = A[0], g = G[0];
#pragma unroll
                for (int c = 1; c < AB_CAM_CG; ++c)
                    if (lane == c) { a = A[c]; g = G[c]; }
                cam[(long)(c0 + lane) * rows + r] = fabsf(pn * fmaf(g, B, a)) / n_feats;
            }
        }
    }
}

inline unsigned ab_grid1d(long n) { return (unsigned)std::max<long>(1, std::min<long>(8192, (n + 255) / 256)); }

bool ab_weights_complete(const amds_abmil_weights& w) { return w.fc_w && w.fc_b && w.a_w && w.a_b && w.b_w && w.b_b && w.c_w && w.c_b && w.cls_w && w.cls_b; }

int ab_stage(const void* x, int dt, float* xs, const AbDims& d, hipStream_t st) {
    const long n_real = d.rows * d.F, n_all = d.rows_p * d.F;
    const dim3 grid(ab_grid1d(n_all));
    if (dt == AMDS_F32) hipLaunchKernelGGL((ab_stage_kernel<float>), grid, dim3(256), 0, st, (const float*)x, xs, n_real, n_all);
    else if (dt == AMDS_F16) hipLaunchKernelGGL((ab_stage_kernel<f16>), grid, dim3(256), 0, st, (const f16*)x, xs, n_real, n_all);
    else hipLaunchKernelGGL((ab_stage_kernel<bf16>), grid, dim3(256), 0, st, (const bf16*)x, xs, n_real, n_all);
    AMDS_LAUNCH_CHECK("ab_stage_kernel");
    return AMDS_OK;
}
int ab_stack(const amds_abmil_weights& w, float* wab, float* bab, const AbDims& d, hipStream_t st) {
    const size_t wl = (size_t)d.D * d.L * 4, bl = (size_t)d.D * 4;
    AMDS_HIP(hipMemcpyAsync(wab, w.a_w, wl, hipMemcpyDeviceToDevice, st));
    AMDS_HIP(hipMemcpyAsync(reinterpret_cast<char*>(wab) + wl, w.b_w, wl, hipMemcpyDeviceToDevice, st));
    if (bab) {
        AMDS_HIP(hipMemcpyAsync(bab, w.a_b, bl, hipMemcpyDeviceToDevice, st));
        AMDS_HIP(hipMemcpyAsync(reinterpret_cast<char*>(bab) + bl, w.b_b, bl, hipMemcpyDeviceToDevice, st));
    }
    return AMDS_OK;
}

// The forward's launch sequence, eval (p = 0) and training alike: the same products on the same padded row count, so p = 0 gives the eval path's bits.
int ab_forward_body(const AbDims& d, const amds_abmil_weights& w, const void* x, int dt, const long long* offs, float p_fc, float p_gate, uint64_t seed, float* xs, float* wab,
                    float* bab, float* h, float* ab, float* s, float* p, float* m, float* logits, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const DropParams dh(p_fc), dg(p_gate);
    RC(ab_stage(x, dt, xs, d, st));
    RC(ab_stack(w, wab, bab, d, st));
    RC(amds_bgemm_f32(xs, d.F, 0, 0, w.fc_w, d.F, 0, 0, 1, h, d.L, 0, 0, 1, 1, (int)d.rows_p, d.L, d.F, 1.0f, 0.0f, w.fc_b, 0, stream));
    hipLaunchKernelGGL(ab_relu_drop_kernel, dim3(ab_grid1d(d.rows_p * d.L)), dim3(256), 0, st, h, d.rows * d.L, d.rows_p * d.L, seed, dh.thr, dh.scale);
    AMDS_LAUNCH_CHECK("ab_relu_drop_kernel");
    RC(amds_bgemm_f32(h, d.L, 0, 0, wab, d.L, 0, 0, 1, ab, 2 * d.D, 0, 0, 1, 1, (int)d.rows_p, 2 * d.D, d.L, 1.0f, 0.0f, bab, 0, stream));
    hipLaunchKernelGGL(ab_gate_score_kernel, dim3((unsigned)((d.rows + 3) / 4)), dim3(256), 0, st, ab, w.c_w, w.c_b, s, d.rows, d.D, seed, dg.thr, dg.scale);
    AMDS_LAUNCH_CHECK("ab_gate_score_kernel");
    AMDS_HIP(hipMemsetAsync(p, 0, (size_t)d.rows * 4, st));          // (a row that no bag's offsets cover -- a caller's error -- weighs nothing, here and in the backward)
    hipLaunchKernelGGL(ab_softmax_bag_kernel, dim3((unsigned)d.bags), dim3(256), 0, st, s, p, offs, d.bags, d.rows);
    AMDS_LAUNCH_CHECK("ab_softmax_bag_kernel");
    hipLaunchKernelGGL(ab_pool_kernel, dim3((unsigned)d.bags, (unsigned)cdiv(d.L, 64)), dim3(256), 0, st, p, h, m, offs, d.bags, d.rows, d.L);
    AMDS_LAUNCH_CHECK("ab_pool_kernel");
    const long n_out = (long)d.bags * d.C;
    hipLaunchKernelGGL(ab_classifier_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, st, m, w.cls_w, w.cls_b, logits, n_out, d.C, d.L);
    AMDS_LAUNCH_CHECK("ab_classifier_kernel");
    return AMDS_OK;
}

int ab_check_call(const char* who, const amds_abmil_weights* w, const void* x, int dt, const long long* offs, int bags) {
    AMDS_REQUIRE(w && x, "%s: null pointer", who);
    AMDS_REQUIRE(ab_weights_complete(*w), "%s: incomplete weights", who);
    AMDS_REQUIRE(dt == AMDS_F32 || dt == AMDS_F16 || dt == AMDS_BF16, "%s: bad x dtype %d", who, dt);
    AMDS_REQUIRE(offs || bags == 1, "%s: row_offsets may be NULL only when bags == 1", who);
    return AMDS_OK;
}
// part[c] = dy_c^T act_c for every chunk c of the rows (dy [rows_p][Mo], act [rows_p][No]); with one chunk `part` is the product itself
int ab_wgrad_partials(const float* dy, int Mo, const float* act, int No, const AbSplit& sp, float* part, void* stream) {
    if (sp.n_full)
        RC(amds_bgemm_f32(dy, Mo, (long)sp.kc * Mo, 0, act, No, (long)sp.kc * No, 0, 2, part, No, (long)Mo * No, 0, sp.n_full, 1, Mo, No, sp.kc, 1.0f, 0.0f, nullptr, 0, stream));
    if (sp.tail) {
        const size_t r0 = (size_t)sp.n_full * sp.kc;
        RC(amds_bgemm_f32(dy + r0 * Mo, Mo, 0, 0, act + r0 * No, No, 0, 0, 2, part + (size_t)sp.n_full * Mo * No, No, 0, 0, 1, 1, Mo, No, sp.tail, 1.0f, 0.0f, nullptr, 0, stream));
    }
    return AMDS_OK;
}

bool ab_drop_ok(const amds_abmil_dropout* dr) { return !dr || (dr->p_fc >= 0.f && dr->p_fc < 1.f && dr->p_gate >= 0.f && dr->p_gate < 1.f); }

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_abmil_workspace_bytes(const amds_abmil_cfg* cfg_host, int bags, long total_rows) {
    AbDims d; AbEvalWs w;
    if (ab_dims(cfg_host, bags, total_rows, &d, "amds_abmil_workspace_bytes") != AMDS_OK) return 0;
    ab_eval_ws(d, &w);
    return w.total;
}
extern "C" size_t amds_abmil_train_saved_bytes(const amds_abmil_cfg* cfg_host, int bags, long total_rows) {
    AbDims d; AbSaved s;
    if (ab_dims(cfg_host, bags, total_rows, &d, "amds_abmil_train_saved_bytes") != AMDS_OK) return 0;
    ab_saved(d, &s);
    return s.total;
}
extern "C" size_t amds_abmil_train_workspace_bytes(const amds_abmil_cfg* cfg_host, int bags, long total_rows) {
    AbDims d; AbTrainWs w;
    if (ab_dims(cfg_host, bags, total_rows, &d, "amds_abmil_train_workspace_bytes") != AMDS_OK) return 0;
    ab_train_ws(d, &w);
    return w.total;
}
extern "C" int amds_abmil_row_pad(void) { return AB_ROW_PAD; }

extern "C" int amds_abmil_forward(const amds_abmil_cfg* cfg_host, const amds_abmil_weights* w_host, const void* x, int x_dtype, const long long* row_offsets, int bags,
                                  long total_rows, float* logits, float* attn_raw, float* pooled, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "amds_abmil_forward";
    AbDims d; AbEvalWs k;
    RC(ab_dims(cfg_host, bags, total_rows, &d, who));
    RC(ab_check_call(who, w_host, x, x_dtype, row_offsets, bags));
    AMDS_REQUIRE(logits && ws, "%s: null pointer", who);
    ab_eval_ws(d, &k);
    if (ws_bytes < k.total) { set_error("%s: workspace %zu < required %zu bytes", who, ws_bytes, k.total); return AMDS_ERR_WORKSPACE; }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    char* wk = reinterpret_cast<char*>(ws);
    auto f = [&](size_t off) { return reinterpret_cast<float*>(wk + off); };
    return ab_forward_body(d, *w_host, x, x_dtype, row_offsets, 0.f, 0.f, 0, f(k.xs), f(k.k.wab), f(k.k.bab), f(k.h), f(k.ab), attn_raw ? attn_raw : f(k.s), f(k.p),
                           pooled ? pooled : f(k.m), logits, stream);
}

extern "C" size_t amds_abmil_heatmap_workspace_bytes(const amds_abmil_cfg* cfg_host, int bags, long total_rows) {
    AbDims d; AbHeatWs w;
    if (ab_dims(cfg_host, bags, total_rows, &d, "amds_abmil_heatmap_workspace_bytes") != AMDS_OK) return 0;
    ab_heat_ws(d, &w);
    return w.total;
}

namespace amds {
namespace {
constexpr int AB_CAM_LDS_MAX = 160 * 1024, AB_CAM_GRID_MAX = 2048;          // (2048 workgroups of four waves: eight waves a SIMD on 256 CUs)
// what ab_cam_kernel stages in LDS: W_cls [C][L] and b_fc [L]
inline long ab_cam_lds_bytes(const AbDims& d) { return ((long)d.C * d.L + d.L) * 4; }
// the one step of the Grad-CAM launches that can fail: taken BEFORE the call's first launch, so that a refused call launches nothing
int ab_cam_prepare(const AbDims& d) {
    const long lds = ab_cam_lds_bytes(d);
    if (lds <= 64 * 1024 || lds > AB_CAM_LDS_MAX) return AMDS_OK;
    if (d.L % 4 == 0) AMDS_HIP(lds_opt_in<ab_cam_kernel<true, true>>(AB_CAM_LDS_MAX));
    else AMDS_HIP(lds_opt_in<ab_cam_kernel<false, true>>(AB_CAM_LDS_MAX));
    return AMDS_OK;
}
template <bool VEC, bool LDSW>
int ab_cam_launch(const AbDims& d, int lds, const float* h, const float* r, const float* p, const float* m, const int* rowbag, const amds_abmil_weights& w, float* cam,
                  hipStream_t st) {
    const unsigned grid = (unsigned)std::min<long>((d.rows + 3) / 4, AB_CAM_GRID_MAX);
    hipLaunchKernelGGL((ab_cam_kernel<VEC, LDSW>), dim3(grid), dim3(256), LDSW ? lds : 0, st, h, r, p, m, rowbag, w.fc_b, w.cls_w, cam, d.rows, d.L, d.C, (float)d.F);
    AMDS_LAUNCH_CHECK("ab_cam_kernel");
    return AMDS_OK;
}
}  // namespace
}  // namespace amds

extern "C" int amds_abmil_heatmap(const amds_abmil_cfg* cfg_host, const amds_abmil_weights* w_host, const void* x, int x_dtype, const long long* row_offsets, int bags,
                                  long total_rows, float* logits, float* attn_raw, float* probs, float* cam_raw, float* tile_logits, void* ws, size_t ws_bytes,
                                  void* stream) {
    const char* who = "amds_abmil_heatmap";
    AbDims d; AbHeatWs k;
    RC(ab_dims(cfg_host, bags, total_rows, &d, who));
    RC(ab_check_call(who, w_host, x, x_dtype, row_offsets, bags));
    AMDS_REQUIRE(logits && ws, "%s: null pointer", who);
    AMDS_REQUIRE(!(cam_raw || tile_logits) || d.rows * d.C < (1L << 31), "%s: total_rows=%ld x classes=%d (cam_raw and tile_logits hold fewer than 2^31 elements)", who, d.rows, d.C);
    ab_heat_ws(d, &k);
    if (ws_bytes < k.total) { set_error("%s: workspace %zu < required %zu bytes", who, ws_bytes, k.total); return AMDS_ERR_WORKSPACE; }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const amds_abmil_weights& w = *w_host;
    char* wk = reinterpret_cast<char*>(ws);
    auto f = [&](size_t off) { return reinterpret_cast<float*>(wk + off); };
    float *h = f(k.e.h), *tq = f(k.e.ab), *m = f(k.e.m), *r = f(k.r), *p = probs ? probs : f(k.e.p);
    if (cam_raw) RC(ab_cam_prepare(d));
    RC(ab_forward_body(d, w, x, x_dtype, row_offsets, 0.f, 0.f, 0, f(k.e.xs), f(k.e.k.wab), f(k.e.k.bab), h, tq, attn_raw ? attn_raw : f(k.e.s), p, m, logits, stream));
    if (tile_logits) {          // a tile as a bag of its own: P = 1, M = h_n -- the classifier over the rows of h
        const long n_out = d.rows * d.C;
        hipLaunchKernelGGL(ab_classifier_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, st, h, w.cls_w, w.cls_b, tile_logits, n_out, d.C, d.L);
        AMDS_LAUNCH_CHECK("ab_classifier_kernel");
    }
    if (!cam_raw) return AMDS_OK;
    int* rowbag = reinterpret_cast<int*>(wk + k.rowbag);
    AMDS_HIP(hipMemsetAsync(rowbag, 0, (size_t)d.rows * 4, st));     // (an uncovered row reads bag 0's M with P = 0: in bounds, its score is 0)
    hipLaunchKernelGGL(ab_rowbag_kernel, dim3((unsigned)d.bags), dim3(256), 0, st, rowbag, row_offsets, d.bags, d.rows);
    AMDS_LAUNCH_CHECK("ab_rowbag_kernel");
    if (d.D % 4 == 0) hipLaunchKernelGGL(ab_cam_gate_kernel<true>, dim3((unsigned)(d.rows_p / 4)), dim3(256), 0, st, tq, w.c_w, d.rows, d.rows_p, d.D);
    else hipLaunchKernelGGL(ab_cam_gate_kernel<false>, dim3((unsigned)(d.rows_p / 4)), dim3(256), 0, st, tq, w.c_w, d.rows, d.rows_p, d.D);
    AMDS_LAUNCH_CHECK("ab_cam_gate_kernel");
    // r = [u | v] W_ab: the shape of the backward's dh = dab W_ab, on the padded row count like every product of the head
    RC(amds_bgemm_f32(tq, 2 * d.D, 0, 0, f(k.e.k.wab), d.L, 0, 0, 0, r, d.L, 0, 0, 1, 1, (int)d.rows_p, d.L, 2 * d.D, 1.0f, 0.0f, nullptr, 0, stream));
    const long lds = ab_cam_lds_bytes(d);
    const bool vec = d.L % 4 == 0, in_lds = lds <= AB_CAM_LDS_MAX;
    if (vec && in_lds) return ab_cam_launch<true, true>(d, (int)lds, h, r, p, m, rowbag, w, cam_raw, st);
    if (vec) return ab_cam_launch<true, false>(d, 0, h, r, p, m, rowbag, w, cam_raw, st);
    if (in_lds) return ab_cam_launch<false, true>(d, (int)lds, h, r, p, m, rowbag, w, cam_raw, st);
    return ab_cam_launch<false, false>(d, 0, h, r, p, m, rowbag, w, cam_raw, st);
}

extern "C" int amds_abmil_train_forward(const amds_abmil_cfg* cfg_host, const amds_abmil_weights* w_host, const void* x, int x_dtype, const long long* row_offsets, int bags,
                                        long total_rows, const amds_abmil_dropout* drop_host, float* logits, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes,
                                        void* stream) {
    const char* who = "amds_abmil_train_forward";
    AbDims d; AbSaved s; AbTrainWs k;
    RC(ab_dims(cfg_host, bags, total_rows, &d, who));
    RC(ab_check_call(who, w_host, x, x_dtype, row_offsets, bags));
    AMDS_REQUIRE(logits && saved && ws, "%s: null pointer", who);
    AMDS_REQUIRE(ab_drop_ok(drop_host), "%s: dropout probabilities must lie in [0, 1)", who);
    ab_saved(d, &s);
    ab_train_ws(d, &k);
    if (saved_bytes < s.total || ws_bytes < k.total) {
        set_error("%s: arena %zu / workspace %zu < required %zu / %zu bytes", who, saved_bytes, ws_bytes, s.total, k.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE((((uintptr_t)saved | (uintptr_t)ws) & 255) == 0, "%s: arena and workspace must be 256-byte aligned", who);
    char *sv = reinterpret_cast<char*>(saved), *wk = reinterpret_cast<char*>(ws);
    auto fs = [&](size_t off) { return reinterpret_cast<float*>(sv + off); };
    auto fw = [&](size_t off) { return reinterpret_cast<float*>(wk + off); };
    const float p_fc = drop_host ? drop_host->p_fc : 0.f, p_gate = drop_host ? drop_host->p_gate : 0.f;
    return ab_forward_body(d, *w_host, x, x_dtype, row_offsets, p_fc, p_gate, drop_host ? drop_host->seed : 0, fw(k.xs), fw(k.k.wab), fw(k.k.bab), fs(s.h), fs(s.tg), fs(s.s),
                           fs(s.p), fs(s.m), logits, stream);
}

extern "C" int amds_abmil_train_backward(const amds_abmil_cfg* cfg_host, const amds_abmil_weights* w_host, const void* x, int x_dtype, const long long* row_offsets, int bags,
                                         long total_rows, const amds_abmil_dropout* drop_host, const float* dlogits, const void* saved, size_t saved_bytes,
                                         const amds_abmil_grads* grads_host, float* dx, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "amds_abmil_train_backward";
    AbDims d; AbSaved s; AbTrainWs k;
    RC(ab_dims(cfg_host, bags, total_rows, &d, who));
    RC(ab_check_call(who, w_host, x, x_dtype, row_offsets, bags));
    AMDS_REQUIRE(dlogits && saved && ws, "%s: null pointer", who);
    AMDS_REQUIRE(grads_host || dx, "%s: nothing to compute (no gradient buffers, no dx)", who);
    AMDS_REQUIRE(ab_drop_ok(drop_host), "%s: dropout probabilities must lie in [0, 1)", who);
    const amds_abmil_grads* G = grads_host;
    AMDS_REQUIRE(!G || (G->fc_w && G->fc_b && G->a_w && G->a_b && G->b_w && G->b_b && G->c_w && G->c_b && G->cls_w && G->cls_b), "%s: incomplete gradient buffers", who);
    ab_saved(d, &s);
    ab_train_ws(d, &k);
    if (saved_bytes < s.total || ws_bytes < k.total) {
        set_error("%s: arena %zu / workspace %zu < required %zu / %zu bytes", who, saved_bytes, ws_bytes, s.total, k.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE((((uintptr_t)saved | (uintptr_t)ws) & 255) == 0, "%s: arena and workspace must be 256-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const amds_abmil_weights& w = *w_host;
    const char* sv = reinterpret_cast<const char*>(saved);
    char* wk = reinterpret_cast<char*>(ws);
    auto fs = [&](size_t off) { return reinterpret_cast<const float*>(sv + off); };
    auto fw = [&](size_t off) { return reinterpret_cast<float*>(wk + off); };
    const DropParams dph(drop_host ? drop_host->p_fc : 0.f), dpg(drop_host ? drop_host->p_gate : 0.f);
    const uint64_t seed = drop_host ? drop_host->seed : 0;
    const int L = d.L, D = d.D, C = d.C, F = d.F;
    const float *h = fs(s.h), *tg = fs(s.tg), *p = fs(s.p), *m = fs(s.m);
    float *dab = fw(k.dab), *dh = fw(k.dh), *g = fw(k.g), *ds = fw(k.ds), *dm = fw(k.dm), *wab = fw(k.k.wab);
    int* rowbag = reinterpret_cast<int*>(wk + k.rowbag);
    auto colsum = [&](const float* src, long ld, float* out, long rows, int cols) { return amds_colsum(src, ld, out, (int)rows, cols, AMDS_F32, 0, wk + k.cs, k.cs_bytes, stream); };
    // ---- classifier: dM, dW_cls, db_cls
    hipLaunchKernelGGL(ab_dpool_kernel, dim3((unsigned)cdiv((long)d.bags * L, 256)), dim3(256), 0, st, dlogits, w.cls_w, dm, (long)d.bags * L, C, L);
    AMDS_LAUNCH_CHECK("ab_dpool_kernel");
    if (G) {
        hipLaunchKernelGGL(ab_cls_grad_kernel, dim3((unsigned)cdiv((long)C * L + C, 256)), dim3(256), 0, st, dlogits, m, G->cls_w, G->cls_b, d.bags, C, L);
        AMDS_LAUNCH_CHECK("ab_cls_grad_kernel");
    }
    // ---- pooling and softmax: g_n = h_n . dM, ds_n = P_n (g_n - sum P g)
    AMDS_HIP(hipMemsetAsync(rowbag, 0, (size_t)d.rows * 4, st));     // (an uncovered row reads bag 0's dM with P = 0: in bounds, no effect)
    hipLaunchKernelGGL(ab_rowbag_kernel, dim3((unsigned)d.bags), dim3(256), 0, st, rowbag, row_offsets, d.bags, d.rows);
    AMDS_LAUNCH_CHECK("ab_rowbag_kernel");
    hipLaunchKernelGGL(ab_rowdot_kernel, dim3((unsigned)((d.rows + 3) / 4)), dim3(256), 0, st, h, dm, rowbag, g, d.rows, L);
    AMDS_LAUNCH_CHECK("ab_rowdot_kernel");
    hipLaunchKernelGGL(ab_dscore_kernel, dim3((unsigned)d.bags), dim3(256), 0, st, p, g, ds, row_offsets, d.bags, d.rows);
    AMDS_LAUNCH_CHECK("ab_dscore_kernel");
    // ---- gate: derivatives with the masks drawn again, dw_c, db_c
    float* prod = G ? fw(k.prod) : nullptr;
    hipLaunchKernelGGL(ab_gate_bwd_kernel, dim3((unsigned)(d.rows_p / 4)), dim3(256), 0, st, tg, ds, w.c_w, dab, prod, d.rows, d.rows_p, D, seed, dpg.thr, dpg.scale);
    AMDS_LAUNCH_CHECK("ab_gate_bwd_kernel");
    if (G) {
        RC(colsum(prod, D, G->c_w, d.rows, D));
        RC(colsum(ds, 1, G->c_b, d.rows, 1));
    }
    // ---- a | b: dh = dab Wab, dWab = dab^T h (row chunks, then their fixed-order sum), dbab
    RC(ab_stack(w, wab, nullptr, d, st));
    RC(amds_bgemm_f32(dab, 2 * D, 0, 0, wab, L, 0, 0, 0, dh, L, 0, 0, 1, 1, (int)d.rows_p, L, 2 * D, 1.0f, 0.0f, nullptr, 0, stream));
    const AbSplit sp = ab_split(d.rows_p);
    float* part = fw(k.part);
    if (G) {
        const size_t half = (size_t)D * L;
        RC(ab_wgrad_partials(dab, 2 * D, h, L, sp, part, stream));
        if (sp.parts == 1) {
            AMDS_HIP(hipMemcpyAsync(G->a_w, part, half * 4, hipMemcpyDeviceToDevice, st));
            AMDS_HIP(hipMemcpyAsync(G->b_w, part + half, half * 4, hipMemcpyDeviceToDevice, st));
        } else {
            RC(colsum(part, (long)2 * half, G->a_w, sp.parts, (int)half));
            RC(colsum(part + half, (long)2 * half, G->b_w, sp.parts, (int)half));
        }
        RC(colsum(dab, 2 * D, G->a_b, d.rows_p, D));
        RC(colsum(dab + D, 2 * D, G->b_b, d.rows_p, D));
    }
    // ---- pooling's own share, ReLU and dropout of h: dz = [h > 0] scale (dh + P_n dM)
    hipLaunchKernelGGL(ab_dh_finish_kernel, dim3(ab_grid1d(d.rows_p * L)), dim3(256), 0, st, dh, h, p, dm, rowbag, d.rows, d.rows_p * L, L, dph.scale);
    AMDS_LAUNCH_CHECK("ab_dh_finish_kernel");
    // ---- fc: dW_fc = dz^T x, db_fc, dx = dz W_fc
    if (G) {
        float* xs = fw(k.xs);
        RC(ab_stage(x, x_dtype, xs, d, st));
        if (sp.parts == 1) RC(ab_wgrad_partials(dh, L, xs, F, sp, G->fc_w, stream));
        else {
            RC(ab_wgrad_partials(dh, L, xs, F, sp, part, stream));
            RC(colsum(part, (long)L * F, G->fc_w, sp.parts, L * F));
        }
        RC(colsum(dh, L, G->fc_b, d.rows_p, L));
    }
    if (dx) RC(amds_bgemm_f32(dh, L, 0, 0, w.fc_w, F, 0, 0, 0, dx, F, 0, 0, 1, 1, (int)d.rows, F, L, 1.0f, 0.0f, nullptr, 0, stream));
    return AMDS_OK;
}
