// transmil_ragged.hip -- the deploy / validation forward of the TransMIL head over RAGGED bags: N bags of different tile counts packed without padding, one
// call, every bag computed as the reference computes it at batch 1 (src/stamp/modeling/train.py:467-477: validation with bag_size = None, batch_size = 1;
// src/stamp/modeling/deploy.py:390-456: one bag per forward).  Restates, per bag, what transmil_fwd.hip restates per batch (trans_mil.py):
//   _fc1 (Linear + ReLU)                                                                     :290, :303       once over the packed tile rows
//   wrap-padding to the bag's OWN square grid with its FIRST tiles, class token in front     :306-314         wrap_cls_varlen_kernel
//   front padding of the bag's sequence to ITS multiple of the landmark count                :96-100          (rows kept in the padded layout; zero_pad_rows_kernel)
//   landmarks over l = np / m tokens, sim1 / sim3 / attn3 v / attn1 pinv / merge / res_conv  :113-153         per BUCKET of bags with equal np, the dense kernels
//   sim2, its softmax, the Moore-Penrose chain                                               :23-37, :129     once over all bags ([m, m] whatever the length)
//   the chain's start scaled by the maxima over the bag's OWN 8 head matrices                :26-28 (b = 1)   amds_pinv_init_grouped(group = 8)
//   PPEG on the bag's own side x side grid                                                   :274-283         ppeg_varlen_kernel
//   final LayerNorm on the class rows, _fc2                                                  :322-325         class rows gathered, logits scattered to caller order
// The token buffers hold every bag's np = pad + n rows, bags ordered by np (then caller order), so a bucket is an ordinary [bags][np][dim] tensor and np is a
// multiple of m: the aligned product kernels apply.  The residual stream lives in the same padded layout; its pad rows carry no information (zero after the
// wrap and after PPEG, then whatever to_out adds) and the LayerNorm outputs' pad rows are zeroed before to_qkv, which is what the reference's F.pad gives.
#include <algorithm>
#include <vector>
#include "model_call.h"

namespace amds {
namespace {

constexpr int HEADS = 8, ITERS = 6, CONV_K = 33;          // trans_mil.py:252-254 (heads = 8, pinv_iterations = 6), :52 (residual_conv_kernel = 33)
constexpr int FC1_ROWS = 128;                              // row tile of the bf16 x 3 product kernel: _fc1 runs as whole tiles + one zero-filled tail tile

struct Bucket { int slot0, count, np; long row0; };

struct RgPlan {
    int Cd, d, m, N;
    long tiles, rows;                                      // sum of T, sum of np
    int max_side, max_pad;
    std::vector<amds_transmil_bag> bags;                   // in slot order
    std::vector<Bucket> buckets;
    size_t hf, tail, x, y, yp, qkv, merged, ql, kl, a2, z, z2, xz, t1, t2, av, a1, a3, a1z, scratch, qc, a1c, a1zc, mc, xc, cls, lg, total;
};

int rg_plan(const amds_transmil_cfg* c, int n_bags, const int* tiles, RgPlan* p) {
    AMDS_REQUIRE(c, "amds_transmil_ragged: null config");
    AMDS_REQUIRE(c->n_feats > 0 && c->dim > 0 && c->dim % 8 == 0 && c->classes > 0, "amds_transmil_ragged: bad config (dim_hidden must be a multiple of 8)");
    AMDS_REQUIRE(n_bags >= 0, "amds_transmil_ragged: bad shape bags=%d", n_bags);
    AMDS_REQUIRE(n_bags == 0 || tiles, "amds_transmil_ragged: null tile counts");
    AMDS_REQUIRE((long)n_bags * HEADS <= 65535, "amds_transmil_ragged: %d bags x 8 heads exceed one launch's batch dimension (split the call)", n_bags);
    p->Cd = c->dim;
    p->d = c->dim / HEADS;
    p->m = c->dim / 2;                                              // num_landmarks = dim // 2 (:253)
    p->N = n_bags;
    const int m = p->m;
    std::vector<amds_transmil_bag> caller(n_bags);
    long tile_off = 0;
    for (int i = 0; i < n_bags; ++i) {
        const int T = tiles[i];
        AMDS_REQUIRE(T >= 1, "amds_transmil_ragged: bag %d has %d tiles (empty bag)", i, T);
        AMDS_REQUIRE(T <= (1 << 30), "amds_transmil_ragged: bag %d has %d tiles", i, T);
        amds_transmil_bag& g = caller[i];
        int side = (int)ceil(sqrt((double)T));
        while ((long)side * side < T) ++side;
        while (side > 1 && (long)(side - 1) * (side - 1) >= T) --side;
        const long n = (long)side * side + 1, rem = n % m;
        const long pad = rem > 0 ? m - rem : 0;                      // FRONT padding to a multiple of the landmark count (:96-100)
        AMDS_REQUIRE(n + pad < (1L << 31), "amds_transmil_ragged: bag %d has too many token rows", i);
        g.tile_off = tile_off;
        g.row_off = 0;
        g.tiles = T; g.side = side; g.n = (int)n; g.pad = (int)pad; g.np = (int)(n + pad); g.orig = i;
        tile_off += T;
    }
    p->tiles = tile_off;
    std::vector<int> order(n_bags);
    for (int i = 0; i < n_bags; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return caller[a].np < caller[b].np; });
    p->bags.resize(n_bags);
    p->buckets.clear();
    long row = 0, max_bucket_rows = 0;
    p->max_side = 0; p->max_pad = 0;
    for (int s = 0; s < n_bags; ++s) {
        amds_transmil_bag g = caller[order[s]];
        g.row_off = row;
        if (p->buckets.empty() || p->buckets.back().np != g.np) p->buckets.push_back(Bucket{s, 0, g.np, row});
        ++p->buckets.back().count;
        row += g.np;
        p->max_side = std::max(p->max_side, g.side);
        p->max_pad = std::max(p->max_pad, g.pad);
        p->bags[s] = g;
    }
    p->rows = row;
    AMDS_REQUIRE(row < (1L << 31) && p->tiles < (1L << 31) - FC1_ROWS, "amds_transmil_ragged: %ld token rows / %ld tiles do not fit the 32-bit row index (split the call)", row,
                 p->tiles);
    for (const Bucket& k : p->buckets) max_bucket_rows = std::max(max_bucket_rows, (long)k.count * k.np);
    const size_t N = n_bags, H = HEADS, R = row, Cd = p->Cd, d = p->d, mm = (size_t)m * m, F = c->n_feats;
    const size_t fc1_rows = (size_t)((p->tiles + FC1_ROWS - 1) / FC1_ROWS) * FC1_ROWS;
    Arena ar;
    p->hf = ar.take((size_t)p->tiles * F * 4);                         // the bags as fp32 (fp16 / bf16 input)
    p->tail = ar.take((size_t)FC1_ROWS * F * 4);                       // _fc1's last, partial row tile, zero-filled
    p->x = ar.take(R * Cd * 4);                                        // per padded token row: x, y, yp, merged (4 x dim) + qkv (3 x dim) floats
    p->y = ar.take(R * Cd * 4);
    p->yp = ar.take(R * Cd * 4);
    p->qkv = ar.take(std::max(R * 3 * Cd, fc1_rows * Cd) * 4);         // (_fc1's output lives here before the first to_qkv)
    p->merged = ar.take(R * Cd * 4);
    p->ql = ar.take(N * H * m * d * 4);                                // landmark-sized: the whole call
    p->kl = ar.take(N * H * m * d * 4);
    p->a2 = ar.take(N * H * mm * 4);
    p->z = ar.take(N * H * mm * 4);
    p->z2 = ar.take(N * H * mm * 4);
    p->xz = ar.take(N * H * mm * 4);
    p->t1 = ar.take(N * H * mm * 4);
    p->t2 = ar.take(N * H * mm * 4);
    p->av = ar.take(N * H * m * d * 4);
    p->a1 = ar.take((size_t)max_bucket_rows * H * m * 4);              // token count x landmarks: the largest bucket, re-used bucket after bucket
    p->a3 = ar.take((size_t)max_bucket_rows * H * m * 4);
    p->a1z = ar.take((size_t)max_bucket_rows * H * m * 4);
    p->scratch = ar.take(N * 8);
    p->qc = ar.take(N * Cd * 4);                                       // the class-row tail of layer 2
    p->a1c = ar.take(N * H * m * 4);
    p->a1zc = ar.take(N * H * m * 4);
    p->mc = ar.take(N * Cd * 4);
    p->xc = ar.take(N * Cd * 4);
    p->cls = ar.take(N * Cd * 4);
    p->lg = ar.take(N * (size_t)c->classes * 4);
    p->total = ar.off;
    return AMDS_OK;
}

template <typename TI>
__global__ void __launch_bounds__(256) to_f32_kernel(const TI* __restrict__ src, float* __restrict__ dst, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (float)src[i];
}

// the bag (slot) that owns padded token row `row`: the last record with row_off <= row
__device__ __forceinline__ int slot_of_row(const amds_transmil_bag* __restrict__ tb, int N, long row) {
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb[mid].row_off <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// padded token rows of x [rows][Cd], per bag: `pad` zero rows, the class token, the projected tiles, then the bag's FIRST tiles again up to side^2 (:306-314)
__global__ void __launch_bounds__(128) wrap_cls_varlen_kernel(const float* __restrict__ cls, const float* __restrict__ h, float* __restrict__ x,
                                                              const amds_transmil_bag* __restrict__ tb, int N, int Cd, int relu) {
    const long row = blockIdx.x;
    const amds_transmil_bag g = tb[slot_of_row(tb, N, row)];
    const int s = (int)(row - g.row_off) - g.pad;
    float* dst = x + row * Cd;
    if (s < 0) { for (int c = threadIdx.x; c < Cd; c += 128) dst[c] = 0.f; return; }
    if (s == 0) { for (int c = threadIdx.x; c < Cd; c += 128) dst[c] = cls[c]; return; }
    const float* src = h + (g.tile_off + (s - 1 < g.tiles ? s - 1 : s - 1 - g.tiles)) * Cd;
    if (relu) { for (int c = threadIdx.x; c < Cd; c += 128) dst[c] = fmaxf(src[c], 0.f); return; }      // (h holds the pre-activation of _fc1)
    for (int c = threadIdx.x; c < Cd; c += 128) dst[c] = src[c];
}

// the `pad` FRONT rows of every bag <- 0 (:100: the LayerNorm ran over them too).  grid (max pad, bags)
__global__ void __launch_bounds__(128) zero_pad_rows_kernel(float* __restrict__ y, const amds_transmil_bag* __restrict__ tb, int Cd) {
    const amds_transmil_bag g = tb[blockIdx.y];
    if ((int)blockIdx.x >= g.pad) return;
    float* dst = y + (g.row_off + blockIdx.x) * Cd;
    for (int c = threadIdx.x; c < Cd; c += 128) dst[c] = 0.f;
}

// PPEG with the grid of each bag (reference trans_mil.py:265-283), ppeg_kernel of transmil.hip with the bag's base row and side from the table: a workgroup owns
// 256 channels of one grid row of one bag (grid: channel groups x the LONGEST side x bags; a workgroup past its bag's side leaves at once).  The three depth-wise
// kernels and the identity are one 7 x 7 kernel per channel, built once in LDS and held in 49 registers per lane; the row is swept with a 7 x 7 register window
// that loads one new column per output.  Zero padding at the bag's own border; the class row passes through; the bag's pad rows of y become zero.
__global__ void __launch_bounds__(256) ppeg_varlen_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ w7, const float* __restrict__ b7,
                                                          const float* __restrict__ w5, const float* __restrict__ b5, const float* __restrict__ w3,
                                                          const float* __restrict__ b3, const amds_transmil_bag* __restrict__ tb, int C) {
    constexpr int SWP = 257;                                     // tap pitch (pitch 256 = one bank)
    __shared__ float sw[49 * SWP];
    const amds_transmil_bag g = tb[blockIdx.z];
    const int i = blockIdx.y, Hh = g.side, Ww = g.side;
    if (i >= Hh) return;                                         // (the whole workgroup: before any barrier)
    const int c0 = blockIdx.x * 256, tid = threadIdx.x, c = c0 + tid;
    const int nc = min(256, C - c0);
    for (int idx = tid; idx < 49 * SWP; idx += 256) sw[idx] = 0.f;
    __syncthreads();
    for (int idx = tid; idx < nc * 49; idx += 256) { const int cl = idx / 49, t = idx - cl * 49; sw[t * SWP + cl] = w7[(long)c0 * 49 + idx]; }
    __syncthreads();
    for (int idx = tid; idx < nc * 25; idx += 256) { const int cl = idx / 25, t = idx - cl * 25; sw[((t / 5 + 1) * 7 + t % 5 + 1) * SWP + cl] += w5[(long)c0 * 25 + idx]; }
    __syncthreads();
    for (int idx = tid; idx < nc * 9; idx += 256) { const int cl = idx / 9, t = idx - cl * 9; sw[((t / 3 + 2) * 7 + t % 3 + 2) * SWP + cl] += w3[(long)c0 * 9 + idx]; }
    __syncthreads();
    if (c >= C) return;
    if (i == 0) {
        for (int r = 0; r < g.pad; ++r) y[(g.row_off + r) * C + c] = 0.f;
    }
    const long base = (g.row_off + g.pad) * C;                   // the bag's class row
    if (i == 0) y[base + c] = x[base + c];                       // class token (trans_mil.py:275, 282)
    float w[49];
#pragma unroll
    for (int t = 0; t < 49; ++t) w[t] = sw[t * SWP + tid];
    w[24] += 1.0f;                                               // the identity term
    const float bsum = b7[c] + b5[c] + b3[c];
    float win[7][7];                                             // win[r][q] = x[i + r - 3][j + q - 3]
    const float* xr[7];
    bool rok[7];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const int ii = i + r - 3;
        rok[r] = ii >= 0 && ii < Hh;
        xr[r] = x + base + (long)(1 + (rok[r] ? ii : 0) * Ww) * C + c;
    }
#pragma unroll
    for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const int jj = q - 3;
            win[r][q] = (rok[r] && jj >= 0 && jj < Ww) ? xr[r][(long)jj * C] : 0.f;
        }
    for (int j = 0; j < Ww; ++j) {
        float s = bsum;
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int q = 0; q < 7; ++q) s = fmaf(w[r * 7 + q], win[r][q], s);
        y[base + (long)(1 + i * Ww + j) * C + c] = s;
        const int jn = j + 4;                                    // column entering the window
#pragma unroll
        for (int r = 0; r < 7; ++r) {
#pragma unroll
            for (int q = 0; q < 6; ++q) win[r][q] = win[r][q + 1];
            win[r][6] = (rok[r] && jn < Ww) ? xr[r][(long)jn * C] : 0.f;
        }
    }
}

// row movement by the table, one workgroup per bag.  CLS_ROWS: dst[slot] = the bag's class row of src (row pitch ld, `cols` values from column 0);
// TO_CALLER: dst[orig] = src[slot] (compact rows of `cols` values): the library's bag order back to the caller's.
enum { CLS_ROWS = 0, TO_CALLER = 1 };
__global__ void __launch_bounds__(128) gather_rows_kernel(const float* __restrict__ src, long ld, float* __restrict__ dst, const amds_transmil_bag* __restrict__ tb, int cols,
                                                          int mode) {
    const int s = blockIdx.x;
    const amds_transmil_bag g = tb[s];
    const float* from = mode == CLS_ROWS ? src + (g.row_off + g.pad) * ld : src + (long)s * cols;
    float* to = dst + (long)(mode == CLS_ROWS ? s : g.orig) * cols;
    for (int c = threadIdx.x; c < cols; c += 128) to[c] = from[c];
}

// the residual convolution for the class row of every bag (dwconv_seq_row_kernel of transmil.hip with the bag's base row, np and pad from the table):
// out[slot][head * d + c] += sum_k w[head][k] * v[bag rows][pad + k - taps / 2][head * d + c], positions outside the bag's np rows are zero (:150-151)
__global__ void __launch_bounds__(64) dwconv_cls_varlen_kernel(const float* __restrict__ v, int ldv, const float* __restrict__ w, float* __restrict__ out,
                                                               const amds_transmil_bag* __restrict__ tb, int Cd, int d, int taps) {
    const int slot = blockIdx.y / HEADS, head = blockIdx.y - slot * HEADS;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d) return;
    const amds_transmil_bag g = tb[slot];
    const float* p = v + g.row_off * ldv + head * d + c;
    const float* wk = w + (long)head * taps;
    const int half = taps / 2;
    float s = 0.f;
    for (int k = 0; k < taps; ++k) {
        const int tt = g.pad + k - half;
        if (tt >= 0 && tt < g.np) s = fmaf(wk[k], p[(long)tt * ldv], s);
    }
    out[(long)slot * Cd + head * d + c] += s;
}

int bg(const float* A, int lda, long sAo, long sAi, const float* B, int ldb, long sBo, long sBi, int transb, float* Cm, int ldc, long sCo, long sCi, int outer,
       int inner, int M, int N, int K, float alpha, float diag, const float* bias, int accumulate, void* st) {
    return amds_bgemm_f32(A, lda, sAo, sAi, B, ldb, sBo, sBi, transb, Cm, ldc, sCo, sCi, outer, inner, M, N, K, alpha, diag, bias, accumulate, st);
}

// x += to_out(NystromAttention(LayerNorm(x)))   (:260-263, :81-163 with mask = None, eval mode), x in the padded layout.
// cls_only: the caller reads the class rows of x and nothing else (layer 2: `self.norm(h)[:, 0]`, :319-323): attn1, attn1 pinv, the merge, the residual convolution
// and to_out are computed for that one row per bag, over the whole call, and the updated class rows are left in `xc` [N][Cd] (x itself is not written).
int nystrom_ragged(const RgPlan& p, const amds_transmil_layer& L, float* x, const amds_transmil_bag* tb, char* wk, void* stream, bool cls_only) {
    hipStream_t st = (hipStream_t)stream;
    const int Cd = p.Cd, H = HEADS, m = p.m, d = p.d, N = p.N, R = (int)p.rows;
    float* yp = reinterpret_cast<float*>(wk + p.yp);
    RC(amds_layernorm(x, Cd, L.norm_w, L.norm_b, yp, Cd, R, Cd, 1e-5f, AMDS_F32, stream));
    if (p.max_pad > 0) {
        hipLaunchKernelGGL(zero_pad_rows_kernel, dim3(p.max_pad, N), dim3(128), 0, st, yp, tb, Cd);
        AMDS_LAUNCH_CHECK("zero_pad_rows_kernel");
    }
    float* qkv = reinterpret_cast<float*>(wk + p.qkv);
    RC(bg(yp, Cd, 0, 0, L.qkv_w, Cd, 0, 0, 1, qkv, 3 * Cd, 0, 0, 1, 1, R, 3 * Cd, Cd, 1.0f, 0.0f, nullptr, 0, stream));           // to_qkv (no bias, :64, :104)
    const long sh = d;
    const int ld = 3 * Cd;
    const double scale_d = 1.0 / sqrt((double)d);                                                                                // dim_head ** -0.5 (:61)
    const float scale = (float)scale_d;
    float *ql = reinterpret_cast<float*>(wk + p.ql), *kl = reinterpret_cast<float*>(wk + p.kl);
    const long md = (long)m * d, mm = (long)m * m, hm = (long)H * m;
    for (const Bucket& k : p.buckets) {                                                                                          // landmarks (:113-124), q scaled (:111)
        const float *qp = qkv + k.row0 * ld, *kp = qp + Cd;
        const long sb = (long)k.np * ld;
        const int l = k.np / m;
        RC(amds_landmark_mean(qp, sb, sh, ld, ql + (long)k.slot0 * H * md, k.count, H, m, l, d, (float)(scale_d / l), stream));
        RC(amds_landmark_mean(kp, sb, sh, ld, kl + (long)k.slot0 * H * md, k.count, H, m, l, d, (float)(1.0 / l), stream));
    }
    float *a2 = reinterpret_cast<float*>(wk + p.a2), *z = reinterpret_cast<float*>(wk + p.z), *z2 = reinterpret_cast<float*>(wk + p.z2);
    float *xz = reinterpret_cast<float*>(wk + p.xz), *t1 = reinterpret_cast<float*>(wk + p.t1), *t2 = reinterpret_cast<float*>(wk + p.t2);
    RC(bg(ql, d, H * md, md, kl, d, H * md, md, 1, a2, m, H * mm, mm, N, H, m, m, d, 1.0f, 0.0f, nullptr, 0, stream));             // sim2 = ql kl^T (:129)
    RC(amds_softmax_rows(a2, (long)N * H * m, m, stream));
    // Moore-Penrose iteration (:23-37), started PER BAG: z0 = a2^T / (max col-sum * max row-sum over the bag's 8 head matrices)
    RC(amds_pinv_init_grouped(a2, z, N * H, m, H, wk + p.scratch, stream));
    const int Zall = N * H, Zc = std::min(Zall, 256);                                                                            // (chunks of 256 matrices: transmil_fwd.hip)
    float* z_fin = z;
    for (int c0 = 0; c0 < Zall; c0 += Zc) {
        const int zn = std::min(Zc, Zall - c0);
        const long co = (long)c0 * mm;
        float *zi = z, *zo = z2;
        auto sq = [&](const float* A, const float* B, float* Cm, float alpha, float diag) {
            return bg(A + co, m, mm, 0, B + co, m, mm, 0, 0, Cm + co, m, mm, 0, zn, 1, m, m, m, alpha, diag, nullptr, 0, stream);
        };
        for (int it = 0; it < ITERS; ++it) {
            RC(amds_bgemm_f32_dual(a2 + co, m, mm, 0, zi + co, m, mm, 0, 0, xz + co, t1 + co, m, mm, 0, zn, 1, m, m, m, 1.0f, 0.0f, -1.0f, 7.0f, stream));
            RC(sq(xz, t1, t2, -1.0f, 15.0f));
            RC(sq(xz, t2, t1, -1.0f, 13.0f));
            RC(sq(zi, t1, zo, 0.25f, 0.0f));
            std::swap(zi, zo);
        }
        z_fin = zi;                                                                                                              // (the same buffer for every chunk)
    }
    z = z_fin;
    float *a1 = reinterpret_cast<float*>(wk + p.a1), *a3 = reinterpret_cast<float*>(wk + p.a3), *a1z = reinterpret_cast<float*>(wk + p.a1z);
    float *av = reinterpret_cast<float*>(wk + p.av), *merged = reinterpret_cast<float*>(wk + p.merged);
    for (const Bucket& k : p.buckets) {
        const float *qp = qkv + k.row0 * ld, *kp = qp + Cd, *vp = qp + 2 * Cd;
        const int np = k.np, b = k.count;
        const long sb = (long)np * ld, nm = (long)np * m;
        const float *qlk = ql + (long)k.slot0 * H * md, *klk = kl + (long)k.slot0 * H * md, *zk = z + (long)k.slot0 * H * mm;
        float* avk = av + (long)k.slot0 * H * md;
        RC(bg(qlk, d, H * md, md, kp, ld, sb, sh, 1, a3, np, H * nm, nm, b, H, m, np, d, 1.0f, 0.0f, nullptr, 0, stream));         // sim3 = ql k^T
        RC(amds_softmax_rows(a3, (long)b * H * m, np, stream));
        RC(bg(a3, np, H * nm, nm, vp, ld, sb, sh, 0, avk, d, H * md, md, b, H, m, d, np, 1.0f, 0.0f, nullptr, 0, stream));          // attn3 v
        if (cls_only) continue;
        float* mk = merged + k.row0 * Cd;
        RC(bg(qp, ld, sb, sh, klk, d, H * md, md, 1, a1, m, H * nm, nm, b, H, np, m, d, scale, 0.0f, nullptr, 0, stream));         // sim1 = q kl^T (:126-128)
        RC(amds_softmax_rows(a1, (long)b * H * np, m, stream));                                                                   // :145
        RC(bg(a1, m, H * nm, nm, zk, m, H * mm, mm, 0, a1z, m, H * nm, nm, b, H, np, m, m, 1.0f, 0.0f, nullptr, 0, stream));       // attn1 pinv
        RC(bg(a1z, m, H * nm, nm, avk, d, H * md, md, 0, mk, Cd, (long)np * Cd, d, b, H, np, d, m, 1.0f, 0.0f, nullptr, 0, stream));   // heads merged (:148-153)
        RC(amds_dwconv_seq(vp, sb, sh, ld, L.conv_w, mk, (long)np * Cd, d, Cd, b, H, np, d, CONV_K, stream));                     // + res_conv(v) (:151)
    }
    if (!cls_only)      // to_out (:154-155) over every padded row (a bag's pad rows of x carry nothing), accumulated into the residual stream
        return bg(merged, Cd, 0, 0, L.out_w, Cd, 0, 0, 1, x, Cd, 0, 0, 1, 1, R, Cd, Cd, 1.0f, 0.0f, L.out_b, 1, stream);
    float *qc = reinterpret_cast<float*>(wk + p.qc), *a1c = reinterpret_cast<float*>(wk + p.a1c), *a1zc = reinterpret_cast<float*>(wk + p.a1zc);
    float *mc = reinterpret_cast<float*>(wk + p.mc), *xc = reinterpret_cast<float*>(wk + p.xc);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(N), dim3(128), 0, st, qkv, (long)ld, qc, tb, Cd, (int)CLS_ROWS);
    AMDS_LAUNCH_CHECK("gather_rows_kernel");
    RC(bg(qc, Cd, Cd, sh, kl, d, H * md, md, 1, a1c, m, hm, m, N, H, 1, m, d, scale, 0.0f, nullptr, 0, stream));                   // the class row of sim1
    RC(amds_softmax_rows(a1c, (long)N * H, m, stream));
    RC(bg(a1c, m, hm, m, z, m, H * mm, mm, 0, a1zc, m, hm, m, N, H, 1, m, m, 1.0f, 0.0f, nullptr, 0, stream));                     // one row of attn1 pinv
    RC(bg(a1zc, m, hm, m, av, d, H * md, md, 0, mc, Cd, Cd, d, N, H, 1, d, m, 1.0f, 0.0f, nullptr, 0, stream));                    // merged: [N][Cd], the class rows
    hipLaunchKernelGGL(dwconv_cls_varlen_kernel, dim3(cdiv(d, 64), N * H), dim3(64), 0, st, qkv + 2 * Cd, ld, L.conv_w, mc, tb, Cd, d, CONV_K);
    AMDS_LAUNCH_CHECK("dwconv_cls_varlen_kernel");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(N), dim3(128), 0, st, x, (long)Cd, xc, tb, Cd, (int)CLS_ROWS);
    AMDS_LAUNCH_CHECK("gather_rows_kernel");
    return bg(mc, Cd, Cd, 0, L.out_w, Cd, 0, 0, 1, xc, Cd, Cd, 0, N, 1, 1, Cd, Cd, 1.0f, 0.0f, L.out_b, 1, stream);
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" int amds_transmil_ragged_plan(const amds_transmil_cfg* cfg_host, int n_bags, const int* tiles_host, amds_transmil_bag* table_host) {
    RgPlan p;
    RC(rg_plan(cfg_host, n_bags, tiles_host, &p));
    AMDS_REQUIRE(n_bags == 0 || table_host, "amds_transmil_ragged_plan: null table");
    for (int s = 0; s < n_bags; ++s) table_host[s] = p.bags[s];
    return AMDS_OK;
}

extern "C" size_t amds_transmil_ragged_workspace_bytes(const amds_transmil_cfg* cfg_host, int n_bags, const int* tiles_host) {
    RgPlan p;
    if (rg_plan(cfg_host, n_bags, tiles_host, &p) != AMDS_OK) return 0;
    return p.total;
}

extern "C" int amds_transmil_forward_ragged(const amds_transmil_cfg* cfg_host, const amds_transmil_weights* w_host, const void* feats, int feats_dtype,
                                            const int* tiles_host, const amds_transmil_bag* table_dev, float* logits, int n_bags, void* ws, size_t ws_bytes,
                                            void* stream) {
    AMDS_REQUIRE(cfg_host && w_host, "amds_transmil_forward_ragged: null pointer");
    RgPlan p;
    RC(rg_plan(cfg_host, n_bags, tiles_host, &p));
    if (n_bags == 0) return AMDS_OK;
    AMDS_REQUIRE(feats && table_dev && logits && ws, "amds_transmil_forward_ragged: null pointer");
    const amds_transmil_weights& w = *w_host;
    AMDS_REQUIRE(w.fc1_w && w.fc1_b && w.cls_token && w.norm_w && w.norm_b && w.fc2_w && w.fc2_b && w.ppeg_w7 && w.ppeg_b7 && w.ppeg_w5 && w.ppeg_b5 &&
                 w.ppeg_w3 && w.ppeg_b3, "amds_transmil_forward_ragged: incomplete weights");
    for (int i = 0; i < 2; ++i)
        AMDS_REQUIRE(w.layer[i].norm_w && w.layer[i].norm_b && w.layer[i].qkv_w && w.layer[i].out_w && w.layer[i].out_b && w.layer[i].conv_w,
                     "amds_transmil_forward_ragged: incomplete weights of layer %d", i + 1);
    AMDS_REQUIRE(feats_dtype == AMDS_F32 || feats_dtype == AMDS_F16 || feats_dtype == AMDS_BF16, "amds_transmil_forward_ragged: bad feats dtype %d", feats_dtype);
    if (ws_bytes < p.total) {
        set_error("amds_transmil_forward_ragged: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_transmil_forward_ragged: workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* wk = reinterpret_cast<char*>(ws);
    const int N = n_bags, Cd = p.Cd, F = cfg_host->n_feats, R = (int)p.rows, Tt = (int)p.tiles;
    const float* hf = reinterpret_cast<const float*>(feats);
    if (feats_dtype != AMDS_F32) {                                                        // the reference casts the bag to float (models/__init__.py:308-313)
        const long cnt = (long)Tt * F;
        const int grid = (int)std::min<long>(8192, (cnt + 255) / 256);
        float* dst = reinterpret_cast<float*>(wk + p.hf);
        if (feats_dtype == AMDS_F16) hipLaunchKernelGGL((to_f32_kernel<f16>), dim3(grid), dim3(256), 0, st, (const f16*)feats, dst, cnt);
        else hipLaunchKernelGGL((to_f32_kernel<bf16>), dim3(grid), dim3(256), 0, st, (const bf16*)feats, dst, cnt);
        AMDS_LAUNCH_CHECK("to_f32_kernel");
        hf = dst;
    }
    float *x = reinterpret_cast<float*>(wk + p.x), *y = reinterpret_cast<float*>(wk + p.y);
    float* h1 = reinterpret_cast<float*>(wk + p.qkv);                                    // _fc1 output [tiles][Cd]: scratch (free until the first to_qkv)
    // _fc1 = Linear + ReLU (:303), as in amds_transmil_forward: below torch's "highest" a product like the others (bf16 x 3) with the ReLU riding on the copy into the
    // wrapped sequence, at "highest" the exact-fp32 Linear.  The tiled bf16 x 3 kernel takes whole 128-row tiles only and the packed tile count is arbitrary: the
    // whole tiles come straight from the packed rows, the remainder from one zero-filled tile of its own -- every tile row goes through the same kernel.
    const bool fc1_x3 = ctx_matmul_precision() != AMDS_MATMUL_HIGHEST && Cd % 128 == 0 && F % 32 == 0;
    if (fc1_x3) {
        const int main_rows = Tt / FC1_ROWS * FC1_ROWS, rest = Tt - main_rows;
        if (main_rows) RC(bg(hf, F, 0, 0, w.fc1_w, F, 0, 0, 1, h1, Cd, 0, 0, 1, 1, main_rows, Cd, F, 1.0f, 0.0f, w.fc1_b, 0, stream));
        if (rest) {
            float* tail = reinterpret_cast<float*>(wk + p.tail);
            AMDS_HIP(hipMemsetAsync(tail, 0, (size_t)FC1_ROWS * F * 4, st));
            AMDS_HIP(hipMemcpyAsync(tail, hf + (size_t)main_rows * F, (size_t)rest * F * 4, hipMemcpyDeviceToDevice, st));
            RC(bg(tail, F, 0, 0, w.fc1_w, F, 0, 0, 1, h1 + (size_t)main_rows * Cd, Cd, 0, 0, 1, 1, FC1_ROWS, Cd, F, 1.0f, 0.0f, w.fc1_b, 0, stream));
        }
    } else {
        RC(amds_linear_f32(hf, w.fc1_w, w.fc1_b, h1, Tt, Cd, F, 1, stream));
    }
    hipLaunchKernelGGL(wrap_cls_varlen_kernel, dim3((unsigned)R), dim3(128), 0, st, w.cls_token, h1, x, table_dev, N, Cd, fc1_x3 ? 1 : 0);
    AMDS_LAUNCH_CHECK("wrap_cls_varlen_kernel");
    // layer1, PPEG, layer2 (:317-319)
    RC(nystrom_ragged(p, w.layer[0], x, table_dev, wk, stream, false));
    hipLaunchKernelGGL(ppeg_varlen_kernel, dim3(cdiv(Cd, 256), p.max_side, N), dim3(256), 0, st, x, y, w.ppeg_w7, w.ppeg_b7, w.ppeg_w5, w.ppeg_b5, w.ppeg_w3, w.ppeg_b3,
                       table_dev, Cd);
    AMDS_LAUNCH_CHECK("ppeg_varlen_kernel");
    std::swap(x, y);
    const bool tail_on = ctx_mil_cls_tail() != 0;                                       // (amds_set_mil_cls_tail(0): every row)
    RC(nystrom_ragged(p, w.layer[1], x, table_dev, wk, stream, tail_on));
    // final LayerNorm on the class-token rows, _fc2 (:322-325), the logits back in the caller's order
    float *xc = reinterpret_cast<float*>(wk + p.xc), *cls = reinterpret_cast<float*>(wk + p.cls), *lg = reinterpret_cast<float*>(wk + p.lg);
    if (!tail_on) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3(N), dim3(128), 0, st, x, (long)Cd, xc, table_dev, Cd, (int)CLS_ROWS);
        AMDS_LAUNCH_CHECK("gather_rows_kernel");
    }
    RC(amds_layernorm(xc, Cd, w.norm_w, w.norm_b, cls, Cd, N, Cd, 1e-5f, AMDS_F32, stream));
    RC(amds_linear_f32(cls, w.fc2_w, w.fc2_b, lg, N, cfg_host->classes, Cd, 0, stream));
    hipLaunchKernelGGL(gather_rows_kernel, dim3(N), dim3(128), 0, st, lg, (long)cfg_host->classes, logits, table_dev, cfg_host->classes, (int)TO_CALLER);
    AMDS_LAUNCH_CHECK("gather_rows_kernel");
    return AMDS_OK;
}
