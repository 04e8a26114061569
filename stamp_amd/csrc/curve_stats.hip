// curve_stats.hip -- the threshold curves of a binary classifier (amds_binary_curves): average precision, the precision-recall area, and the ROC and
// precision-recall curves interpolated onto a grid, per problem and batched over problems, because the reference's bands are quantiles over 1000 bootstrap
// resamples of the same curves (reference src/stamp/statistics/roc.py:161-224, src/stamp/statistics/prc.py:26-87) and its per-class table holds
// `average_precision_score` next to AUROC (src/stamp/statistics/categorical.py:65-75).  include/amdstamp.h states the statistic.
//
// Two launches (three with idx):
//   1. curve_rank_kernel, once per BASE problem (every problem without idx, the one resampled problem with idx): item i gets
//          g_i = #{valid j : key(score_j) > key(score_i)},
//      the position at which its tie group starts in the descending order, by counting -- the pair kernel's tile walk (rank_metrics.hip), O(n^2) compares,
//      no sort.  Tied items share one g, so a resample's weights can be added up PER GROUP and no later pass has to look at a score again.
//      code_i = 2 g_i + label_i, or -1 for an invalid item.
//   2. curve_problem_kernel, one workgroup per problem: zero two int32 arrays over the nb positions; add every item's multiplicity at its group's position
//      (integer atomics: the sums do not depend on the order); scan both (positions inside a group repeat their group's cumulative counts, which repeats a
//      curve point and changes nothing below); reduce AP and the PR area; answer the grid points by binary search over the cumulative counts.
//      The arrays live in LDS up to CS_LDS_ITEMS positions and in the workspace above.
// Every decision is an integer compare (order keys, k * N against FP * (G - 1) in 64 bits); fp64 appears only where a ratio is formed, and fp64 sums run
// thread-strided and then over a fixed tree: a call is bitwise reproducible.
#include "launch.h"

namespace amds {
namespace {

constexpr int CS_BLOCK = 256;
constexpr int CS_TJ = 1024;                  // j keys per LDS tile of the rank kernel
constexpr long CS_MAX_ITEMS = 1L << 20;      // n_items and n_base
constexpr int CS_MAX_GRID = 4096;
constexpr long CS_LDS_ITEMS = 12288;         // positions whose two count arrays fit LDS (96 KiB) beside the grid values (32 KiB)
constexpr int CS_RED_BYTES = 64;             // block-reduction scratch

struct cs_plan {
    long nb, bases;           // positions per base problem; base problems
    bool lds;
    int grid_pad;             // grid rounded up to 2 doubles
    long nb_pad;              // nb rounded up to 4 ints
    int lds_bytes;
    size_t code_bytes, cum_bytes, bad_bytes, total;
};

inline size_t cs_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline int cs_lds_bytes(long nb_pad, int grid_pad, bool lds) { return grid_pad * 8 + CS_RED_BYTES + (lds ? (int)(nb_pad * 8) : 0); }

// the limits, with the message the two exports share; `who` prefixes it
inline bool cs_make_plan(const char* who, bool with_idx, long n_base, long n_items, int n_problems, int grid, cs_plan* p) {
    if (n_items < 1 || n_items > CS_MAX_ITEMS) {
        set_error("%s: n_items=%ld outside [1, %ld]", who, n_items, CS_MAX_ITEMS);
        return false;
    }
    if (n_problems < 1 || (long)n_problems * n_items >= (1L << 31)) {
        set_error("%s: n_problems=%d: needs n_problems >= 1 and n_problems * n_items < 2^31 (n_items=%ld)", who, n_problems, n_items);
        return false;
    }
    if (with_idx && (n_base < 1 || n_base > CS_MAX_ITEMS)) {
        set_error("%s: n_base=%ld outside [1, %ld]", who, n_base, CS_MAX_ITEMS);
        return false;
    }
    if (grid != 0 && (grid < 2 || grid > CS_MAX_GRID)) {
        set_error("%s: grid=%d: needs 0 or 2 <= grid <= %d", who, grid, CS_MAX_GRID);
        return false;
    }
    p->nb = with_idx ? n_base : n_items;
    p->bases = with_idx ? 1 : n_problems;
    p->lds = p->nb <= CS_LDS_ITEMS;
    p->grid_pad = (grid + 1) & ~1;
    p->nb_pad = (p->nb + 3) & ~3L;
    p->lds_bytes = cs_lds_bytes(p->nb_pad, p->grid_pad, p->lds);
    p->code_bytes = cs_align((size_t)p->bases * p->nb * sizeof(int32_t));
    p->cum_bytes = p->lds ? 0 : cs_align((size_t)n_problems * 2 * p->nb * sizeof(int32_t));
    p->bad_bytes = cs_align(((size_t)n_problems + 1) * sizeof(int64_t));          // per problem, then the call's total
    p->total = p->code_bytes + p->cum_bytes + p->bad_bytes;
    return true;
}

// fp32's own order on unsigned integers, -0 and +0 on one key: the rule of rk_key (rank_metrics.hip).  A valid key is never 0 (key(-inf) = 0x007FFFFF).
__device__ __forceinline__ unsigned cs_key(float x) {
    unsigned b = __float_as_uint(x);
    if ((b << 1) == 0) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// grid (base problems, i tiles).  code[base][i] = 2 * #{valid j: score_j > score_i} + label_i, -1 for an invalid item.
__global__ void __launch_bounds__(CS_BLOCK) curve_rank_kernel(const float* __restrict__ score, long s_item, long s_prob, const uint8_t* __restrict__ label,
                                                              long l_prob, long nb, int32_t* __restrict__ code) {
    __shared__ unsigned tile[CS_TJ];
    score += (long)blockIdx.x * s_prob;
    label += (long)blockIdx.x * l_prob;
    code += (long)blockIdx.x * nb;
    const long i = (long)blockIdx.y * CS_BLOCK + threadIdx.x;
    unsigned ki = 0xFFFFFFFFu;                 // (nothing is above it: an item that is not there counts nothing)
    int lab = -1;
    if (i < nb) {
        const float s = score[i * s_item];
        const unsigned l = label[i];
        if (s == s && l <= 1u) ki = cs_key(s), lab = (int)l;
    }
    unsigned g = 0;
    for (long j0 = 0; j0 < nb; j0 += CS_TJ) {
        const int cnt = (int)(nb - j0 < CS_TJ ? nb - j0 : CS_TJ);
        const int padded = (cnt + 7) & ~7;
        __syncthreads();                       // (the previous tile is still being read)
        for (int t = threadIdx.x; t < padded; t += CS_BLOCK) {
            unsigned k = 0u;                   // an invalid or absent j is above nothing
            if (t < cnt) {
                const float s = score[(j0 + t) * s_item];
                if (s == s && label[j0 + t] <= 1u) k = cs_key(s);
            }
            tile[t] = k;
        }
        __syncthreads();
        unsigned c = 0;
#pragma unroll 8
        for (int t = 0; t < padded; ++t) c += (unsigned)(tile[t] > ki);          // one address for the whole wave: a broadcast
        g += c;
    }
    if (i < nb) code[i] = lab < 0 ? -1 : (int)(g * 2u + (unsigned)lab);
}

// fixed-order fold over the workgroup: butterfly inside each wave (every lane ends with the same bits: + commutes), then the four waves in index order
template <typename T>
__device__ __forceinline__ T cs_block_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// grid (problems).  Dynamic LDS: grid values [grid_pad] f64 | reduction scratch | with LDS_ARRAYS: cumulative positives [nb_pad], negatives [nb_pad] int32.
template <bool LDS_ARRAYS>
__global__ void __launch_bounds__(CS_BLOCK) curve_problem_kernel(const int32_t* __restrict__ code, long code_prob, const int32_t* __restrict__ idx, long nb,
                                                                 long nb_pad, long n, int G, int grid_pad, int32_t* cum, long long* __restrict__ counts,
                                                                 double* __restrict__ scalars, double* __restrict__ roc, double* __restrict__ pr,
                                                                 long long* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_smem[];
    double* gv = (double*)cs_smem;
    double* red = gv + grid_pad;
    unsigned long long* wsum = (unsigned long long*)red;
    const long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* cTP;
    int* cFP;
    if constexpr (LDS_ARRAYS) {
        cTP = (int*)(cs_smem + (size_t)grid_pad * 8 + CS_RED_BYTES);
        cFP = cTP + nb_pad;
    } else {
        cTP = cum + p * 2 * nb;
        cFP = cTP + nb;
    }
    for (long t = tid; t < nb; t += CS_BLOCK) cTP[t] = 0, cFP[t] = 0;
    __syncthreads();

    // multiplicities, at the position where the item's tie group starts
    const int32_t* crow = code + p * code_prob;
    const int32_t* irow = idx ? idx + p * n : nullptr;
    long long nbad = 0;
    for (long k = tid; k < n; k += CS_BLOCK) {
        long src = k;
        if (irow) {
            src = irow[k];
            if (src < 0 || src >= nb) {       // range-checked before any use
                ++nbad;
                continue;
            }
        }
        const int c = crow[src];
        if (c >= 0) atomicAdd((c & 1) ? &cTP[c >> 1] : &cFP[c >> 1], 1);
    }
    __syncthreads();

    // inclusive scan of both arrays, a tile of CS_BLOCK positions at a time; one 64-bit lane value carries both counts (each < 2^21)
    unsigned long long carry = 0;
    for (long t0 = 0; t0 < nb; t0 += CS_BLOCK) {
        const long t = t0 + tid;
        unsigned long long v = t < nb ? ((unsigned long long)(unsigned)cTP[t] << 32) | (unsigned)cFP[t] : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        unsigned long long pre = carry;
        for (int w = 0; w < wave; ++w) pre += wsum[w];
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        v += pre;
        if (t < nb) cTP[t] = (int)(v >> 32), cFP[t] = (int)(unsigned)v;
        __syncthreads();
    }
    const long long P = (long long)(carry >> 32), N = (long long)(carry & 0xFFFFFFFFull);
    const long long bad_all = cs_block_sum(nbad, (long long*)red);
    if (tid == 0) counts[p * 2] = P, counts[p * 2 + 1] = N, bad[p] = bad_all;
    __syncthreads();                           // (the scratch is reused below)

    if (P == 0 || N == 0) {                    // undefined: every value is NaN (uniform over the workgroup)
        const double nan = __longlong_as_double(0x7FF8000000000000LL);
        if (tid < 3) scalars[p * 3 + tid] = nan;
        for (int k = tid; k < G; k += CS_BLOCK) {
            if (roc) roc[p * G + k] = nan;
            if (pr) pr[p * G + k] = nan;
        }
        return;
    }

    // AP and the area under the problem's own precision-recall curve: the terms of the positions where TP rises (a repeated point has width 0)
    const double dP = (double)P;
    double ap = 0.0, area = 0.0;
    for (long t = tid; t < nb; t += CS_BLOCK) {
        const int tp = cTP[t], fp = cFP[t];
        const int tp0 = t ? cTP[t - 1] : 0, fp0 = t ? cFP[t - 1] : 0;
        if (tp > tp0) {
            const double prec = (double)tp / (double)(tp + fp);
            const double prec0 = (tp0 + fp0) ? (double)tp0 / (double)(tp0 + fp0) : 1.0;
            const double dr = (double)(tp - tp0) / dP;
            ap += dr * prec;
            area += dr * ((prec + prec0) * 0.5);
        }
    }
    ap = cs_block_sum(ap, red);
    area = cs_block_sum(area, red);
    double garea = __longlong_as_double(0x7FF8000000000000LL);

    if (G >= 2) {
        const long long S = G - 1;
        for (int k = tid; k < G; k += CS_BLOCK) {
            if (roc) {
                const long long target = (long long)k * N;
                long lo = 0, hi = nb;          // -> the number of positions with FP * (G - 1) <= k * N
                while (lo < hi) {
                    const long mid = (lo + hi) >> 1;
                    if ((long long)cFP[mid] * S <= target) lo = mid + 1;
                    else hi = mid;
                }
                double val = 1.0;
                if (lo < nb) {
                    const int tpj = lo ? cTP[lo - 1] : 0, fpj = lo ? cFP[lo - 1] : 0;
                    const int tp1 = cTP[lo], fp1 = cFP[lo];
                    const double frac = ((double)target / (double)S - (double)fpj) / (double)(fp1 - fpj);
                    val = ((double)tpj + frac * (double)(tp1 - tpj)) / dP;
                }
                roc[p * G + k] = val;
            }
            {
                const long long target = (long long)k * P;
                long lo = 0, hi = nb;          // -> the number of positions with TP * (G - 1) <= k * P
                while (lo < hi) {
                    const long mid = (lo + hi) >> 1;
                    if ((long long)cTP[mid] * S <= target) lo = mid + 1;
                    else hi = mid;
                }
                const int tpj = lo ? cTP[lo - 1] : 0, fpj = lo ? cFP[lo - 1] : 0;
                const double precj = (tpj + fpj) ? (double)tpj / (double)(tpj + fpj) : 1.0;
                double val = precj;
                if (lo < nb) {
                    const int tp1 = cTP[lo], fp1 = cFP[lo];
                    const double prec1 = (double)tp1 / (double)(tp1 + fp1);
                    const double frac = ((double)target / (double)S - (double)tpj) / (double)(tp1 - tpj);
                    val = precj + frac * (prec1 - precj);
                }
                gv[k] = val;
                if (pr) pr[p * G + k] = val;
            }
        }
        __syncthreads();
        double acc = 0.0;
        for (int k = tid; k < G - 1; k += CS_BLOCK) acc += ((double)(k + 1) / (double)S - (double)k / (double)S) * ((gv[k] + gv[k + 1]) * 0.5);
        garea = cs_block_sum(acc, red);
    }
    if (tid == 0) scalars[p * 3] = ap, scalars[p * 3 + 1] = area, scalars[p * 3 + 2] = garea;
}

// one workgroup: the problems' out-of-range counts -> bad[problems]
__global__ void __launch_bounds__(CS_BLOCK) curve_bad_kernel(long long* __restrict__ bad, long problems) {
    __shared__ long long red[4];
    long long acc = 0;
    for (long p = threadIdx.x; p < problems; p += CS_BLOCK) acc += bad[p];
    acc = cs_block_sum(acc, red);
    if (threadIdx.x == 0) bad[problems] = acc;
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_binary_curves_workspace_bytes(long n_base, long n_items, int n_problems, int grid) {
    cs_plan p;
    if (n_base < 0) {
        set_error("amds_binary_curves: n_base=%ld: 0 without idx, the base problem's size with it", n_base);
        return 0;
    }
    return cs_make_plan("amds_binary_curves", n_base > 0, n_base, n_items, n_problems, grid, &p) ? p.total : 0;
}

extern "C" int amds_binary_curves(const float* score, long score_item_stride, long score_problem_stride, const uint8_t* label, long label_problem_stride,
                                  const int32_t* idx, long n_base, long n_items, int n_problems, int grid, int64_t* counts, double* scalars, double* roc_grid,
                                  double* pr_grid, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(score && label && counts && scalars && ws, "amds_binary_curves: null pointer");
    cs_plan p;
    if (!cs_make_plan("amds_binary_curves", idx != nullptr, n_base, n_items, n_problems, grid, &p)) return AMDS_ERR_INVALID;
    AMDS_REQUIRE(grid >= 2 || (!roc_grid && !pr_grid), "amds_binary_curves: grid=0 with a grid output");
    AMDS_REQUIRE(score_item_stride >= 1 && score_problem_stride >= 0 && label_problem_stride >= 0, "amds_binary_curves: bad strides score %ld / %ld label %ld",
                 score_item_stride, score_problem_stride, label_problem_stride);
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_binary_curves: workspace not 256-byte aligned");
    if (ws_bytes < p.total) {
        set_error("amds_binary_curves: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    int32_t* code = (int32_t*)ws;
    int32_t* cum = p.lds ? nullptr : (int32_t*)((char*)ws + p.code_bytes);
    long long* bad = (long long*)((char*)ws + p.code_bytes + p.cum_bytes);
    const unsigned i_tiles = (unsigned)((p.nb + CS_BLOCK - 1) / CS_BLOCK);          // <= 4096
    hipLaunchKernelGGL(curve_rank_kernel, dim3((unsigned)p.bases, i_tiles), dim3(CS_BLOCK), 0, st, score, score_item_stride, idx ? 0L : score_problem_stride,
                       label, idx ? 0L : label_problem_stride, p.nb, code);
    AMDS_LAUNCH_CHECK("curve_rank_kernel");
    const long code_prob = idx ? 0 : p.nb;
    if (p.lds) {
        AMDS_HIP(lds_opt_in<curve_problem_kernel<true>>(cs_lds_bytes((CS_LDS_ITEMS + 3) & ~3L, CS_MAX_GRID, true)));
        hipLaunchKernelGGL(curve_problem_kernel<true>, dim3((unsigned)n_problems), dim3(CS_BLOCK), (size_t)p.lds_bytes, st, code, code_prob, idx, p.nb, p.nb_pad,
                           n_items, grid, p.grid_pad, cum, (long long*)counts, scalars, roc_grid, pr_grid, bad);
    } else {
        hipLaunchKernelGGL(curve_problem_kernel<false>, dim3((unsigned)n_problems), dim3(CS_BLOCK), (size_t)p.lds_bytes, st, code, code_prob, idx, p.nb, p.nb_pad,
                           n_items, grid, p.grid_pad, cum, (long long*)counts, scalars, roc_grid, pr_grid, bad);
    }
    AMDS_LAUNCH_CHECK("curve_problem_kernel");
    if (!idx) return AMDS_OK;
    hipLaunchKernelGGL(curve_bad_kernel, dim3(1), dim3(CS_BLOCK), 0, st, bad, (long)n_problems);
    AMDS_LAUNCH_CHECK("curve_bad_kernel");
    long long n_bad = 0;
    AMDS_HIP(hipMemcpyAsync(&n_bad, bad + n_problems, sizeof n_bad, hipMemcpyDeviceToHost, st));
    AMDS_HIP(hipStreamSynchronize(st));
    AMDS_REQUIRE(n_bad == 0, "amds_binary_curves: %lld index value(s) lie outside [0, %ld)", n_bad, n_base);
    return AMDS_OK;
}
