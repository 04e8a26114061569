// survival_stats.hip -- the reference's survival and regression reports as two batched entry points.
//   amds_survival_groups:    two risk groups split at a cut-off, per problem the two-sample log-rank sums (O, E, V), the Kaplan-Meier curve of each group on a
//                            grid of times, the at-risk table, the median survival times and the comparable pairs (reference
//                            src/stamp/statistics/survival.py:16-87, 116-157);
//   amds_regression_moments: the eight moments R^2, Pearson r, MAE, RMSE and the fitted line are formed from (src/stamp/statistics/regression.py:14-39, 70).
// Batched over problems, because the bands of a Kaplan-Meier plot and the intervals of every number are quantiles over bootstrap resamples of the same
// statistic.  include/amdstamp.h states the statistics.
//
// amds_survival_groups, two launches (three with a grid, one more with idx), built like curve_stats.hip:
//   1. surv_rank_kernel, once per BASE problem (every problem without idx, the one resampled problem with idx): item i gets
//          pos_i = #{valid j : key(time_j) < key(time_i)},
//      the position at which its tie group starts in the ascending order of time, by counting -- the pair kernel's tile walk (rank_metrics.hip), O(n^2)
//      compares, no sort.  code_i = 2 pos_i + event_i, or -1 for an invalid item; tpos[pos_i] = time_i (tied items store the same bits).
//   2. surv_grid_kernel (grid > 0): every grid time x is ranked against the same items the same way: le = #{valid j : time_j <= x}, lt = #{... < x}.  The
//      items with time <= x are then exactly the positions below le, so a grid point is answered by two array reads and no search.
//   3. surv_problem_kernel, one workgroup per problem: zero four int32 arrays over the nb positions (deaths and exits of LOW and HIGH); add every item's
//      multiplicity at its position (integer atomics: the sums do not depend on the order); prefix-scan all four (the risk set at a position is the group's
//      total minus the exits before it); reduce E, V and the comparable pairs; scan the two survival products; find the medians; answer the grid.
//      The arrays live in LDS up to SV_LDS_ITEMS positions and in the workspace above.
// Every decision is an integer compare (order keys, counts) or the fp64 compare of a score with the cut-off; fp64 appears where a ratio is formed from
// integers, and fp64 sums and products run thread-strided or lane-scanned and then over a fixed tree: a call is bitwise reproducible.
#include "launch.h"

namespace amds {
namespace {

constexpr int SV_BLOCK = 256;
constexpr int SV_TJ = 1024;                  // j keys per LDS tile of the rank kernels
constexpr long SV_MAX_ITEMS = 1L << 20;      // n_items and n_base
constexpr int SV_MAX_GRID = 4096;
constexpr int SV_RED_BYTES = 128;            // block-reduction and scan scratch
// positions whose six arrays (two fp64 products, four int32 counts: 32 B per position) fit the 160 KiB of a CU's LDS beside the scratch:
// 5000 * 32 + 128 = 160128 <= 163840
constexpr long SV_LDS_ITEMS = 5000;
constexpr int SV_POS_BYTES = 32;

struct sv_plan {
    long nb, bases, units;    // positions per base problem; base problems; problems whose grid is ranked on its own
    bool lds;
    long nb_pad;              // nb rounded up to 4
    int lds_bytes;
    size_t code_bytes, tpos_bytes, gpos_bytes, arr_bytes, bad_bytes, total;
};

inline size_t sv_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline int sv_lds_bytes(long nb_pad, bool lds) { return SV_RED_BYTES + (lds ? (int)(nb_pad * SV_POS_BYTES) : 0); }

// the limits, with the message the two exports share
inline bool sv_make_plan(const char* who, bool with_idx, long n_base, long n_items, int n_problems, int grid, bool grid_shared, sv_plan* p) {
    if (n_items < 1 || n_items > SV_MAX_ITEMS) {
        set_error("%s: n_items=%ld outside [1, %ld]", who, n_items, SV_MAX_ITEMS);
        return false;
    }
    if (n_problems < 1 || (long)n_problems * n_items >= (1L << 31)) {
        set_error("%s: n_problems=%d: needs n_problems >= 1 and n_problems * n_items < 2^31 (n_items=%ld)", who, n_problems, n_items);
        return false;
    }
    if (with_idx && (n_base < 1 || n_base > SV_MAX_ITEMS)) {
        set_error("%s: n_base=%ld outside [1, %ld]", who, n_base, SV_MAX_ITEMS);
        return false;
    }
    if (grid != 0 && (grid < 2 || grid > SV_MAX_GRID)) {
        set_error("%s: grid=%d: needs 0 or 2 <= grid <= %d", who, grid, SV_MAX_GRID);
        return false;
    }
    p->nb = with_idx ? n_base : n_items;
    p->bases = with_idx ? 1 : n_problems;
    p->units = (with_idx && grid_shared) ? 1 : n_problems;
    p->lds = p->nb <= SV_LDS_ITEMS;
    p->nb_pad = (p->nb + 3) & ~3L;
    p->lds_bytes = sv_lds_bytes(p->nb_pad, p->lds);
    p->code_bytes = sv_align((size_t)p->bases * p->nb * sizeof(int32_t));
    p->tpos_bytes = sv_align((size_t)p->bases * p->nb * sizeof(float));
    p->gpos_bytes = sv_align((size_t)p->units * grid * 2 * sizeof(int32_t));
    p->arr_bytes = p->lds ? 0 : sv_align((size_t)n_problems * p->nb_pad * SV_POS_BYTES);
    p->bad_bytes = sv_align(((size_t)n_problems + 1) * sizeof(int64_t));          // per problem, then the call's total
    p->total = p->code_bytes + p->tpos_bytes + p->gpos_bytes + p->arr_bytes + p->bad_bytes;
    return true;
}

// fp32's own order on unsigned integers, -0 and +0 on one key: the rule of rk_key (rank_metrics.hip).  The largest key of a non-NaN value is
// key(+inf) = 0xFF800000, so 0xFFFFFFFF is above every valid key.
__device__ __forceinline__ unsigned sv_key(float x) {
    unsigned b = __float_as_uint(x);
    if ((b << 1) == 0) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ bool sv_valid(float s, float t, unsigned e) { return s == s && t == t && e <= 1u; }

// the tile walk both rank kernels share: over the nb items of one base problem, lt = #{valid j : key(time_j) < kq}, le = #{valid j : key(time_j) <= kq}
__device__ __forceinline__ void sv_count(const float* __restrict__ score, long s_item, const float* __restrict__ time, const uint8_t* __restrict__ event, long nb,
                                         unsigned kq, unsigned* tile, unsigned* lt_out, unsigned* le_out) {
    unsigned lt = 0, le = 0;
    for (long j0 = 0; j0 < nb; j0 += SV_TJ) {
        const int cnt = (int)(nb - j0 < SV_TJ ? nb - j0 : SV_TJ);
        const int padded = (cnt + 7) & ~7;
        __syncthreads();                       // (the previous tile is still being read)
        for (int t = threadIdx.x; t < padded; t += SV_BLOCK) {
            unsigned k = 0xFFFFFFFFu;          // an invalid or absent j is below nothing
            if (t < cnt) {
                const float tm = time[j0 + t];
                if (sv_valid(score[(j0 + t) * s_item], tm, event[j0 + t])) k = sv_key(tm);
            }
            tile[t] = k;
        }
        __syncthreads();
        unsigned a = 0, b = 0;
#pragma unroll 8
        for (int t = 0; t < padded; ++t) {
            const unsigned k = tile[t];        // one address for the whole wave: a broadcast
            a += (unsigned)(k < kq);
            b += (unsigned)(k <= kq);
        }
        lt += a;
        le += b;
    }
    *lt_out = lt;
    *le_out = le;
}

// grid (base problems, i tiles).  code[base][i] = 2 * #{valid j: time_j < time_i} + event_i, -1 for an invalid item; tpos[base][position] = the time there.
__global__ void __launch_bounds__(SV_BLOCK) surv_rank_kernel(const float* __restrict__ score, long s_item, long s_prob, const float* __restrict__ time,
                                                             long t_prob, const uint8_t* __restrict__ event, long e_prob, long nb, int32_t* __restrict__ code,
                                                             float* __restrict__ tpos) {
    __shared__ unsigned tile[SV_TJ];
    score += (long)blockIdx.x * s_prob;
    time += (long)blockIdx.x * t_prob;
    event += (long)blockIdx.x * e_prob;
    code += (long)blockIdx.x * nb;
    tpos += (long)blockIdx.x * nb;
    const long i = (long)blockIdx.y * SV_BLOCK + threadIdx.x;
    unsigned ki = 0u;                          // (nothing is below it: an item that is not there counts nothing)
    int ev = -1;
    if (i < nb) {
        const float tm = time[i];
        const unsigned e = event[i];
        if (sv_valid(score[i * s_item], tm, e)) ki = sv_key(tm), ev = (int)e;
    }
    unsigned lt, le;
    sv_count(score, s_item, time, event, nb, ki, tile, &lt, &le);
    if (i < nb) {
        code[i] = ev < 0 ? -1 : (int)(lt * 2u + (unsigned)ev);
        // the key's own value (-0 stored as +0): every item of a tie group stores the same bits
        if (ev >= 0) tpos[lt] = __uint_as_float((ki & 0x80000000u) ? (ki ^ 0x80000000u) : ~ki);
    }
}

// grid (grid units, g tiles).  gpos[unit][k] = {#{valid j: time_j <= x_k}, #{valid j: time_j < x_k}} over the unit's base problem, {-1, -1} for a NaN x_k.
__global__ void __launch_bounds__(SV_BLOCK) surv_grid_kernel(const float* __restrict__ score, long s_item, long s_prob, const float* __restrict__ time,
                                                             long t_prob, const uint8_t* __restrict__ event, long e_prob, long nb,
                                                             const float* __restrict__ grid_times, long g_prob, int G, int32_t* __restrict__ gpos) {
    __shared__ unsigned tile[SV_TJ];
    score += (long)blockIdx.x * s_prob;
    time += (long)blockIdx.x * t_prob;
    event += (long)blockIdx.x * e_prob;
    grid_times += (long)blockIdx.x * g_prob;
    gpos += (long)blockIdx.x * G * 2;
    const int k = blockIdx.y * SV_BLOCK + threadIdx.x;
    unsigned kq = 0u;
    bool ok = false;
    if (k < G) {
        const float x = grid_times[k];
        if (x == x) kq = sv_key(x), ok = true;
    }
    unsigned lt, le;
    sv_count(score, s_item, time, event, nb, kq, tile, &lt, &le);
    if (k < G) gpos[2 * k] = ok ? (int)le : -1, gpos[2 * k + 1] = ok ? (int)lt : -1;
}

// fixed-order folds over the workgroup: butterfly inside each wave (every lane ends with the same bits), then the four waves in index order
template <typename T>
__device__ __forceinline__ T sv_block_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ long sv_block_min(long v, long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long u = __shfl_xor(v, o);
        v = u < v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long m = red[0];
    for (int w = 1; w < 4; ++w) m = red[w] < m ? red[w] : m;
    return m;
}

// the knife edge of the median: a product that equals 1/2 as a rational may round to either side of it (include/amdstamp.h, MEDIAN)
#define SV_HALF (0.5 * (1.0 + 0x1p-30))

// grid (problems).  Dynamic LDS: scratch [SV_RED_BYTES] | with LDS_ARRAYS: survival products LOW, HIGH [nb_pad] f64, then cumulative deaths LOW, exits LOW,
// deaths HIGH, exits HIGH [nb_pad] int32.  Group 0 = LOW, 1 = HIGH.
template <bool LDS_ARRAYS>
__global__ void __launch_bounds__(SV_BLOCK) surv_problem_kernel(const int32_t* __restrict__ code, const float* __restrict__ tpos, long code_prob,
                                                                const float* __restrict__ score, long s_item, long s_prob, const double* __restrict__ cutoff,
                                                                long c_prob, const int32_t* __restrict__ idx, long nb, long nb_pad, long n,
                                                                const int32_t* __restrict__ gpos, long gpos_prob, int G, unsigned char* arrays,
                                                                long long* __restrict__ counts, double* __restrict__ logrank, double* __restrict__ median,
                                                                long long* __restrict__ pairs, double* __restrict__ km, long long* __restrict__ table,
                                                                long long* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sv_smem[];
    double* red = (double*)sv_smem;
    unsigned long long* wsum = (unsigned long long*)sv_smem;          // [2][4]
    const long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* mine = LDS_ARRAYS ? sv_smem + SV_RED_BYTES : arrays + (size_t)p * nb_pad * SV_POS_BYTES;
    double* S0 = (double*)mine;
    double* S1 = S0 + nb_pad;
    int* cD0 = (int*)(S1 + nb_pad);
    int* cX0 = cD0 + nb_pad;
    int* cD1 = cX0 + nb_pad;
    int* cX1 = cD1 + nb_pad;
    for (long t = tid; t < nb; t += SV_BLOCK) cD0[t] = 0, cX0[t] = 0, cD1[t] = 0, cX1[t] = 0;
    __syncthreads();

    // multiplicities, at the position where the item's tie group starts
    const int32_t* crow = code + p * code_prob;
    const float* srow = score + p * s_prob;
    const int32_t* irow = idx ? idx + p * n : nullptr;
    const double cut = cutoff[p * c_prob];
    long long nbad = 0;
    for (long k = tid; k < n; k += SV_BLOCK) {
        long src = k;
        if (irow) {
            src = irow[k];
            if (src < 0 || src >= nb) {       // range-checked before any use
                ++nbad;
                continue;
            }
        }
        const int c = crow[src];
        if (c < 0) continue;
        const bool high = (double)srow[src * s_item] > cut;          // exact for an fp32 score and a midpoint cut-off; a NaN cut-off sends everything LOW
        atomicAdd(high ? &cX1[c >> 1] : &cX0[c >> 1], 1);
        if (c & 1) atomicAdd(high ? &cD1[c >> 1] : &cD0[c >> 1], 1);
    }
    __syncthreads();

    // inclusive scan of the four arrays, a tile of SV_BLOCK positions at a time; one 64-bit lane value carries a group's two counts (each <= 2^20)
    unsigned long long carry0 = 0, carry1 = 0;
    for (long t0 = 0; t0 < nb; t0 += SV_BLOCK) {
        const long t = t0 + tid;
        unsigned long long v0 = t < nb ? ((unsigned long long)(unsigned)cD0[t] << 32) | (unsigned)cX0[t] : 0ull;
        unsigned long long v1 = t < nb ? ((unsigned long long)(unsigned)cD1[t] << 32) | (unsigned)cX1[t] : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u0 = __shfl_up(v0, o), u1 = __shfl_up(v1, o);
            if (lane >= o) v0 += u0, v1 += u1;
        }
        if (lane == 63) wsum[wave] = v0, wsum[4 + wave] = v1;
        __syncthreads();
        unsigned long long pre0 = carry0, pre1 = carry1;
        for (int w = 0; w < wave; ++w) pre0 += wsum[w], pre1 += wsum[4 + w];
        carry0 += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        carry1 += wsum[4] + wsum[5] + wsum[6] + wsum[7];
        v0 += pre0;
        v1 += pre1;
        if (t < nb) cD0[t] = (int)(v0 >> 32), cX0[t] = (int)(unsigned)v0, cD1[t] = (int)(v1 >> 32), cX1[t] = (int)(unsigned)v1;
        __syncthreads();
    }
    const long long N0 = (long long)(carry0 & 0xFFFFFFFFull), D0 = (long long)(carry0 >> 32);
    const long long N1 = (long long)(carry1 & 0xFFFFFFFFull), D1 = (long long)(carry1 >> 32);
    const long long bad_all = sv_block_sum(nbad, (long long*)red);
    if (tid == 0) {
        long long* c = counts + p * 6;
        c[0] = N0, c[1] = D0, c[2] = N0 - D0, c[3] = N1, c[4] = D1, c[5] = N1 - D1;
        bad[p] = bad_all;
    }

    // the terms of every position, and each group's factor of the survival product
    double e_sum = 0.0, v_sum = 0.0;
    long long pair_sum = 0;
    for (long t = tid; t < nb; t += SV_BLOCK) {
        const long long x0p = t ? cX0[t - 1] : 0, x1p = t ? cX1[t - 1] : 0;
        const long long d0 = cD0[t] - (t ? cD0[t - 1] : 0), d1 = cD1[t] - (t ? cD1[t - 1] : 0);
        const long long n0 = N0 - x0p, n1 = N1 - x1p;          // at risk: the group's total minus the exits before this position
        const long long nk = n0 + n1, dk = d0 + d1, xk = (cX0[t] - x0p) + (cX1[t] - x1p);
        if (dk > 0) {                                          // (then nk >= dk > 0)
            e_sum += (double)(dk * n1) / (double)nk;
            if (nk > 1) v_sum += ((double)(dk * (nk - dk)) / (double)(nk - 1)) * ((double)n1 / (double)nk) * ((double)n0 / (double)nk);
            pair_sum += dk * (nk - xk);
        }
        S0[t] = d0 > 0 ? (double)(n0 - d0) / (double)n0 : 1.0;          // exactly 0 when the whole risk set dies
        S1[t] = d1 > 0 ? (double)(n1 - d1) / (double)n1 : 1.0;
    }
    e_sum = sv_block_sum(e_sum, red);
    v_sum = sv_block_sum(v_sum, red);
    pair_sum = sv_block_sum(pair_sum, (long long*)red);
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    if (tid == 0) {
        const bool both = N0 > 0 && N1 > 0;
        logrank[p * 3] = both ? (double)D1 : nan, logrank[p * 3 + 1] = both ? e_sum : nan, logrank[p * 3 + 2] = both ? v_sum : nan;
        if (pairs) pairs[p] = pair_sum;
    }
    __syncthreads();                           // (the factors are complete, the scratch is free)

    // inclusive product scan of the two factor arrays: lanes, then waves in index order, then the carry
    double* wprod = red;                       // [2][4]
    double pc0 = 1.0, pc1 = 1.0;
    for (long t0 = 0; t0 < nb; t0 += SV_BLOCK) {
        const long t = t0 + tid;
        double v0 = t < nb ? S0[t] : 1.0, v1 = t < nb ? S1[t] : 1.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u0 = __shfl_up(v0, o), u1 = __shfl_up(v1, o);
            if (lane >= o) v0 *= u0, v1 *= u1;
        }
        if (lane == 63) wprod[wave] = v0, wprod[4 + wave] = v1;
        __syncthreads();
        double pre0 = pc0, pre1 = pc1;
        for (int w = 0; w < wave; ++w) pre0 *= wprod[w], pre1 *= wprod[4 + w];
        pc0 *= ((wprod[0] * wprod[1]) * wprod[2]) * wprod[3];
        pc1 *= ((wprod[4] * wprod[5]) * wprod[6]) * wprod[7];
        if (t < nb) S0[t] = pre0 * v0, S1[t] = pre1 * v1;
        __syncthreads();
    }

    // medians: the first position with a death of the group at which the product is at or below one half (the product falls only at such positions, and
    // an item stands there, so tpos holds its time)
    long m0 = nb, m1 = nb;
    for (long t = tid; t < nb; t += SV_BLOCK) {
        if (S0[t] <= SV_HALF && cD0[t] > (t ? cD0[t - 1] : 0) && t < m0) m0 = t;
        if (S1[t] <= SV_HALF && cD1[t] > (t ? cD1[t - 1] : 0) && t < m1) m1 = t;
    }
    m0 = sv_block_min(m0, (long*)red);
    m1 = sv_block_min(m1, (long*)red);
    if (tid == 0) {
        const float* trow = tpos + p * code_prob;
        const double inf = __longlong_as_double(0x7FF0000000000000LL);
        median[p * 2] = N0 == 0 ? nan : (m0 < nb ? (double)trow[m0] : inf);
        median[p * 2 + 1] = N1 == 0 ? nan : (m1 < nb ? (double)trow[m1] : inf);
    }

    // the grid: the items with time <= x are the positions below le, those with time < x the positions below lt
    const int32_t* grow = gpos + p * gpos_prob;
    for (int k = tid; k < G; k += SV_BLOCK) {
        const int le = grow[2 * k], lt = grow[2 * k + 1];
        if (km) {
            double* o = km + (p * 2) * G + k;
            o[0] = (le < 0 || N0 == 0) ? nan : (le ? S0[le - 1] : 1.0);
            o[G] = (le < 0 || N1 == 0) ? nan : (le ? S1[le - 1] : 1.0);
        }
        if (table) {
            long long* o0 = table + ((p * 2) * G + k) * 3;
            long long* o1 = o0 + (long)G * 3;
            if (le < 0) {
                o0[0] = o0[1] = o0[2] = o1[0] = o1[1] = o1[2] = -1;
            } else {
                const long long dd0 = le ? cD0[le - 1] : 0, dd1 = le ? cD1[le - 1] : 0;
                o0[0] = N0 - (lt ? cX0[lt - 1] : 0), o0[1] = dd0, o0[2] = (le ? cX0[le - 1] : 0) - dd0;
                o1[0] = N1 - (lt ? cX1[lt - 1] : 0), o1[1] = dd1, o1[2] = (le ? cX1[le - 1] : 0) - dd1;
            }
        }
    }
}

// one workgroup: the problems' out-of-range counts -> bad[problems]
__global__ void __launch_bounds__(SV_BLOCK) surv_bad_kernel(long long* __restrict__ bad, long problems) {
    __shared__ long long red[4];
    long long acc = 0;
    for (long p = threadIdx.x; p < problems; p += SV_BLOCK) acc += bad[p];
    acc = sv_block_sum(acc, red);
    if (threadIdx.x == 0) bad[problems] = acc;
}

// grid (problems).  Two passes in fp64, each thread-strided and then folded over the fixed tree: the means, then the sums centred on them.
__global__ void __launch_bounds__(SV_BLOCK) regression_moments_kernel(const float* __restrict__ truth, long t_item, long t_prob, const float* __restrict__ pred,
                                                                      long p_item, long p_prob, const int32_t* __restrict__ idx, long nb, long n,
                                                                      double* __restrict__ moments, long long* __restrict__ bad) {
    __shared__ double red[4];
    const long p = blockIdx.x;
    const int32_t* irow = idx ? idx + p * n : nullptr;
    if (!idx) truth += p * t_prob, pred += p * p_prob;
    long long cnt = 0, nbad = 0;
    double st = 0.0, sp = 0.0;
    for (long k = threadIdx.x; k < n; k += SV_BLOCK) {
        long src = k;
        if (irow) {
            src = irow[k];
            if (src < 0 || src >= nb) {       // range-checked before any use
                ++nbad;
                continue;
            }
        }
        const float a = truth[src * t_item], b = pred[src * p_item];
        if (a == a && b == b) ++cnt, st += (double)a, sp += (double)b;
    }
    const long long n_ok = sv_block_sum(cnt, (long long*)red);
    const long long bad_all = sv_block_sum(nbad, (long long*)red);
    st = sv_block_sum(st, red);
    sp = sv_block_sum(sp, red);
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    const double mt = n_ok ? st / (double)n_ok : nan, mp = n_ok ? sp / (double)n_ok : nan;
    double sxx = 0.0, syy = 0.0, sxy = 0.0, sae = 0.0, sse = 0.0;
    for (long k = threadIdx.x; k < n; k += SV_BLOCK) {
        long src = k;
        if (irow) {
            src = irow[k];
            if (src < 0 || src >= nb) continue;
        }
        const float a = truth[src * t_item], b = pred[src * p_item];
        if (a == a && b == b) {
            const double dt = (double)a - mt, dp = (double)b - mp, r = (double)b - (double)a;
            sxx += dt * dt, syy += dp * dp, sxy += dt * dp, sae += fabs(r), sse += r * r;
        }
    }
    sxx = sv_block_sum(sxx, red);
    syy = sv_block_sum(syy, red);
    sxy = sv_block_sum(sxy, red);
    sae = sv_block_sum(sae, red);
    sse = sv_block_sum(sse, red);
    if (threadIdx.x == 0) {
        double* o = moments + p * 8;
        o[0] = (double)n_ok, o[1] = mt, o[2] = mp, o[3] = sxx, o[4] = syy, o[5] = sxy, o[6] = sae, o[7] = sse;
        bad[p] = bad_all;
    }
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_survival_groups_workspace_bytes(long n_base, long n_items, int n_problems, int grid, int grid_shared) {
    sv_plan p;
    if (n_base < 0) {
        set_error("amds_survival_groups: n_base=%ld: 0 without idx, the base problem's size with it", n_base);
        return 0;
    }
    return sv_make_plan("amds_survival_groups", n_base > 0, n_base, n_items, n_problems, grid, grid_shared != 0, &p) ? p.total : 0;
}

extern "C" int amds_survival_groups(const float* score, long score_item_stride, long score_problem_stride, const float* time, long time_problem_stride,
                                    const uint8_t* event, long event_problem_stride, const double* cutoff, long cutoff_problem_stride, const int32_t* idx,
                                    long n_base, long n_items, int n_problems, const float* grid_times, long grid_problem_stride, int grid, int64_t* counts,
                                    double* logrank, double* median, int64_t* pairs, double* km, int64_t* at_risk, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(score && time && event && cutoff && counts && logrank && median && ws, "amds_survival_groups: null pointer");
    AMDS_REQUIRE(grid_problem_stride >= 0, "amds_survival_groups: grid_problem_stride=%ld: needs 0 (one grid for all problems) or more", grid_problem_stride);
    sv_plan p;
    if (!sv_make_plan("amds_survival_groups", idx != nullptr, n_base, n_items, n_problems, grid, grid_problem_stride == 0, &p)) return AMDS_ERR_INVALID;
    AMDS_REQUIRE(grid >= 2 ? grid_times != nullptr : (!grid_times && !km && !at_risk), "amds_survival_groups: grid=%d %s", grid,
                 grid >= 2 ? "without grid_times" : "with grid_times or a grid output");
    AMDS_REQUIRE(score_item_stride >= 1 && score_problem_stride >= 0 && time_problem_stride >= 0 && event_problem_stride >= 0 &&
                     (cutoff_problem_stride == 0 || cutoff_problem_stride == 1),
                 "amds_survival_groups: bad strides score %ld / %ld time %ld event %ld cutoff %ld", score_item_stride, score_problem_stride, time_problem_stride,
                 event_problem_stride, cutoff_problem_stride);
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_survival_groups: workspace not 256-byte aligned");
    if (ws_bytes < p.total) {
        set_error("amds_survival_groups: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int32_t* code = (int32_t*)w;
    float* tpos = (float*)(w + p.code_bytes);
    int32_t* gpos = (int32_t*)(w + p.code_bytes + p.tpos_bytes);
    unsigned char* arrays = p.lds ? nullptr : (unsigned char*)(w + p.code_bytes + p.tpos_bytes + p.gpos_bytes);
    long long* bad = (long long*)(w + p.code_bytes + p.tpos_bytes + p.gpos_bytes + p.arr_bytes);
    const long sp = idx ? 0L : score_problem_stride, tp = idx ? 0L : time_problem_stride, ep = idx ? 0L : event_problem_stride;
    const unsigned i_tiles = (unsigned)((p.nb + SV_BLOCK - 1) / SV_BLOCK);          // <= 4096
    hipLaunchKernelGGL(surv_rank_kernel, dim3((unsigned)p.bases, i_tiles), dim3(SV_BLOCK), 0, st, score, score_item_stride, sp, time, tp, event, ep, p.nb, code,
                       tpos);
    AMDS_LAUNCH_CHECK("surv_rank_kernel");
    if (grid >= 2) {
        const unsigned g_tiles = (unsigned)((grid + SV_BLOCK - 1) / SV_BLOCK);
        hipLaunchKernelGGL(surv_grid_kernel, dim3((unsigned)p.units, g_tiles), dim3(SV_BLOCK), 0, st, score, score_item_stride, sp, time, tp, event, ep, p.nb,
                           grid_times, grid_problem_stride, grid, gpos);
        AMDS_LAUNCH_CHECK("surv_grid_kernel");
    }
    const long code_prob = idx ? 0 : p.nb;
    const long gpos_prob = p.units == 1 ? 0 : (long)grid * 2;
    if (p.lds) {
        AMDS_HIP(lds_opt_in<surv_problem_kernel<true>>(sv_lds_bytes((SV_LDS_ITEMS + 3) & ~3L, true)));
        hipLaunchKernelGGL(surv_problem_kernel<true>, dim3((unsigned)n_problems), dim3(SV_BLOCK), (size_t)p.lds_bytes, st, code, tpos, code_prob, score,
                           score_item_stride, sp, cutoff, cutoff_problem_stride, idx, p.nb, p.nb_pad, n_items, gpos, gpos_prob, grid, arrays,
                           (long long*)counts, logrank, median, (long long*)pairs, km, (long long*)at_risk, bad);
    } else {
        hipLaunchKernelGGL(surv_problem_kernel<false>, dim3((unsigned)n_problems), dim3(SV_BLOCK), (size_t)p.lds_bytes, st, code, tpos, code_prob, score,
                           score_item_stride, sp, cutoff, cutoff_problem_stride, idx, p.nb, p.nb_pad, n_items, gpos, gpos_prob, grid, arrays,
                           (long long*)counts, logrank, median, (long long*)pairs, km, (long long*)at_risk, bad);
    }
    AMDS_LAUNCH_CHECK("surv_problem_kernel");
    if (!idx) return AMDS_OK;
    hipLaunchKernelGGL(surv_bad_kernel, dim3(1), dim3(SV_BLOCK), 0, st, bad, (long)n_problems);
    AMDS_LAUNCH_CHECK("surv_bad_kernel");
    long long n_bad = 0;
    AMDS_HIP(hipMemcpyAsync(&n_bad, bad + n_problems, sizeof n_bad, hipMemcpyDeviceToHost, st));
    AMDS_HIP(hipStreamSynchronize(st));
    AMDS_REQUIRE(n_bad == 0, "amds_survival_groups: %lld index value(s) lie outside [0, %ld)", n_bad, n_base);
    return AMDS_OK;
}

static bool rg_check(long n_base, bool with_idx, long n_items, int n_problems) {
    if (n_items < 1 || n_items >= (1L << 31)) {
        set_error("amds_regression_moments: n_items=%ld outside [1, 2^31)", n_items);
        return false;
    }
    if (n_problems < 1) {
        set_error("amds_regression_moments: n_problems=%d: needs n_problems >= 1", n_problems);
        return false;
    }
    if (with_idx && (n_base < 1 || n_base >= (1L << 31))) {
        set_error("amds_regression_moments: n_base=%ld outside [1, 2^31)", n_base);
        return false;
    }
    return true;
}

extern "C" size_t amds_regression_moments_workspace_bytes(long n_base, long n_items, int n_problems) {
    if (n_base < 0) {
        set_error("amds_regression_moments: n_base=%ld: 0 without idx, the base problem's size with it", n_base);
        return 0;
    }
    return rg_check(n_base, n_base > 0, n_items, n_problems) ? sv_align(((size_t)n_problems + 1) * sizeof(int64_t)) : 0;
}

extern "C" int amds_regression_moments(const float* truth, long truth_item_stride, long truth_problem_stride, const float* pred, long pred_item_stride,
                                       long pred_problem_stride, const int32_t* idx, long n_base, long n_items, int n_problems, double* moments, void* ws,
                                       size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(truth && pred && moments && ws, "amds_regression_moments: null pointer");
    if (!rg_check(n_base, idx != nullptr, n_items, n_problems)) return AMDS_ERR_INVALID;
    AMDS_REQUIRE(truth_item_stride >= 1 && pred_item_stride >= 1 && truth_problem_stride >= 0 && pred_problem_stride >= 0,
                 "amds_regression_moments: bad strides truth %ld / %ld pred %ld / %ld", truth_item_stride, truth_problem_stride, pred_item_stride,
                 pred_problem_stride);
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_regression_moments: workspace not 256-byte aligned");
    const size_t need = sv_align(((size_t)n_problems + 1) * sizeof(int64_t));
    if (ws_bytes < need) {
        set_error("amds_regression_moments: workspace %zu < required %zu bytes", ws_bytes, need);
        return AMDS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    long long* bad = (long long*)ws;
    hipLaunchKernelGGL(regression_moments_kernel, dim3((unsigned)n_problems), dim3(SV_BLOCK), 0, st, truth, truth_item_stride, truth_problem_stride, pred,
                       pred_item_stride, pred_problem_stride, idx, idx ? n_base : n_items, n_items, moments, bad);
    AMDS_LAUNCH_CHECK("regression_moments_kernel");
    if (!idx) return AMDS_OK;
    hipLaunchKernelGGL(surv_bad_kernel, dim3(1), dim3(SV_BLOCK), 0, st, bad, (long)n_problems);
    AMDS_LAUNCH_CHECK("surv_bad_kernel");
    long long n_bad = 0;
    AMDS_HIP(hipMemcpyAsync(&n_bad, bad + n_problems, sizeof n_bad, hipMemcpyDeviceToHost, st));
    AMDS_HIP(hipStreamSynchronize(st));
    AMDS_REQUIRE(n_bad == 0, "amds_regression_moments: %lld index value(s) lie outside [0, %ld)", n_bad, n_base);
    return AMDS_OK;
}
