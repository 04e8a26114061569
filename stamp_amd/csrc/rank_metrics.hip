// rank_metrics.hip -- exact pair counts of the concordance statistic (amds_concordance_counts): the validation C-index the reference selects survival
// epochs on (reference src/stamp/modeling/models/__init__.py:662-715, src/stamp/modeling/train.py:521-540) and, with event = (y == c), time = (y != c), the
// one-vs-rest AUROC (src/stamp/statistics/categorical.py:65-68); batched over problems, because the reference's intervals are bootstrap resamples of the same
// statistic (src/stamp/statistics/roc.py:161-214).  Integers only: no atomics, no N x N tensor, bitwise reproducible.
//
// Every item is turned into two 32-bit ORDER KEYS when it is loaded.  key(x) maps the non-NaN fp32 values onto unsigned integers in fp32's own order with
// -0 and +0 on one key, so `key(a) < key(b)` IS the fp32 compare `a < b` (and == is ==), denormals included.  The permissibility test
//     event_i == 1 && (time_i < time_j || (time_i == time_j && event_j == 0))
// then is ONE unsigned compare  ki < kj  with
//     ki = key(time_i)                      for a valid item with event 1,   0xFFFFFFFF otherwise  (as `i` it starts no pair),
//     kj = key(time_j) + (event_j == 0)     for a valid item,                0          otherwise  (as `j` it ends no pair);
// the largest key of a non-NaN value is key(+inf) = 0xFF800000, so the +1 cannot wrap and 0xFFFFFFFF is below nothing.
#include "common.h"

namespace amds {
namespace {

constexpr int RK_BLOCK = 256;          // i items per workgroup, one per thread, in registers
constexpr int RK_TJ = 1024;            // j items per LDS tile (8 KiB)
constexpr int RK_MAX_CHUNKS = 64;      // j chunks per problem (grid.y)
constexpr long RK_CHUNK_ITEMS = 4096;  // a j chunk is this long until RK_MAX_CHUNKS of them no longer cover the problem
constexpr int RK_PART = 5;             // int64 per workgroup partial: concordant, tied, permissible, valid i items, out-of-range indices

struct rk_plan {
    long i_tiles, chunk;      // workgroups along i; j items per chunk (a multiple of RK_TJ)
    int j_chunks;
    size_t part_bytes, total;
};

inline size_t rk_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline void rk_make_plan(long n, long problems, rk_plan* p) {
    p->i_tiles = (n + RK_BLOCK - 1) / RK_BLOCK;
    long chunks = (n + RK_CHUNK_ITEMS - 1) / RK_CHUNK_ITEMS;
    if (chunks > RK_MAX_CHUNKS) chunks = RK_MAX_CHUNKS;
    p->chunk = ((n + chunks - 1) / chunks + RK_TJ - 1) / RK_TJ * RK_TJ;
    p->j_chunks = (int)((n + p->chunk - 1) / p->chunk);
    p->part_bytes = rk_align((size_t)problems * p->i_tiles * p->j_chunks * RK_PART * sizeof(int64_t));
    p->total = p->part_bytes + rk_align(sizeof(int64_t));          // + the call's out-of-range index count
}

__device__ __forceinline__ unsigned rk_key(float x) {
    unsigned b = __float_as_uint(x);
    if ((b << 1) == 0) b = 0;                                       // -0 -> +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct rk_item {
    unsigned kt_i, kt_j, ks;
    int valid, bad_index;
};

// item `pos` of problem `p`: position -> base item (through idx, range-checked before any use) -> the three values -> keys
__device__ __forceinline__ rk_item rk_load(const float* __restrict__ score, long s_item, const float* __restrict__ time, const uint8_t* __restrict__ event,
                                           const int32_t* __restrict__ idx_row, long n_base, long pos) {
    rk_item it = {0xFFFFFFFFu, 0u, 0u, 0, 0};
    long src = pos;
    if (idx_row) {
        src = idx_row[pos];
        if (src < 0 || src >= n_base) {
            it.bad_index = 1;
            return it;
        }
    }
    const float s = score[src * s_item], t = time[src];
    const unsigned e = event[src];
    if (s != s || t != t || e > 1u) return it;
    const unsigned kt = rk_key(t);
    it.valid = 1;
    it.ks = rk_key(s);
    it.kt_i = e ? kt : 0xFFFFFFFFu;
    it.kt_j = kt + (e ? 0u : 1u);
    return it;
}

// fixed-order fold of one 64-bit count over the workgroup: butterfly inside each wave, then the four wave results in index order
__device__ __forceinline__ long long rk_block_sum(long long v, long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// grid (i tiles, j chunks, problems of this launch).  part[problem][i tile][j chunk][RK_PART].
__global__ void __launch_bounds__(RK_BLOCK) concordance_pairs_kernel(const float* __restrict__ score, long s_item, long s_prob, const float* __restrict__ time,
                                                                     long t_prob, const uint8_t* __restrict__ event, long e_prob,
                                                                     const int32_t* __restrict__ idx, long n_base, long n, long chunk, int p0,
                                                                     long long* __restrict__ part) {
    __shared__ uint2 tile[RK_TJ];          // .x = kj, .y = score key
    __shared__ long long red[4];
    const int p = p0 + blockIdx.z;
    const int32_t* idx_row = idx ? idx + (long)p * n : nullptr;
    if (!idx) {
        score += (long)p * s_prob;
        time += (long)p * t_prob;
        event += (long)p * e_prob;
    }
    const long i = (long)blockIdx.x * RK_BLOCK + threadIdx.x;
    rk_item me = {0xFFFFFFFFu, 0u, 0u, 0, 0};
    if (i < n) me = rk_load(score, s_item, time, event, idx_row, n_base, i);
    const unsigned ki = me.kt_i, si = me.ks;

    long long conc = 0, tied = 0, perm = 0;
    const long j_begin = (long)blockIdx.y * chunk;
    const long j_end = j_begin + chunk < n ? j_begin + chunk : n;
    for (long j0 = j_begin; j0 < j_end; j0 += RK_TJ) {
        const int cnt = (int)(j_end - j0 < RK_TJ ? j_end - j0 : RK_TJ);
        const int padded = (cnt + 7) & ~7;
        __syncthreads();                   // (the previous tile is still being read)
        for (int t = threadIdx.x; t < padded; t += RK_BLOCK) {
            uint2 v = make_uint2(0u, 0u);
            if (t < cnt) {
                const rk_item it = rk_load(score, s_item, time, event, idx_row, n_base, j0 + t);
                v = make_uint2(it.kt_j, it.ks);
            }
            tile[t] = v;
        }
        __syncthreads();
        unsigned c = 0, e = 0, q = 0;      // 32-bit inside a tile: at most RK_TJ each
#pragma unroll 8
        for (int t = 0; t < padded; ++t) {
            const uint2 v = tile[t];       // one address for the whole wave: a broadcast
            const unsigned ok = ki < v.x;
            q += ok;
            c += ok & (unsigned)(si > v.y);
            e += ok & (unsigned)(si == v.y);
        }
        conc += c;
        tied += e;
        perm += q;
    }
    const bool first = blockIdx.y == 0;    // each i item is counted once per problem
    const long long r0 = rk_block_sum(conc, red), r1 = rk_block_sum(tied, red), r2 = rk_block_sum(perm, red);
    const long long r3 = rk_block_sum(first ? me.valid : 0, red), r4 = rk_block_sum(first ? me.bad_index : 0, red);
    if (threadIdx.x == 0) {
        long long* o = part + (((long)blockIdx.z * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * RK_PART;
        o[0] = r0, o[1] = r1, o[2] = r2, o[3] = r3, o[4] = r4;
    }
}

// one workgroup per problem: its partials summed in a fixed order -> counts[problem][4]; the out-of-range count stays in part[problem][0][0][4]
__global__ void __launch_bounds__(RK_BLOCK) concordance_fold_kernel(long long* __restrict__ part, long per_problem, long long* __restrict__ counts) {
    __shared__ long long red[4];
    long long* mine = part + (long)blockIdx.x * per_problem * RK_PART;
    long long acc[RK_PART] = {0, 0, 0, 0, 0};
    for (long w = threadIdx.x; w < per_problem; w += RK_BLOCK)
#pragma unroll
        for (int k = 0; k < RK_PART; ++k) acc[k] += mine[w * RK_PART + k];
    long long r[RK_PART];
#pragma unroll
    for (int k = 0; k < RK_PART; ++k) r[k] = rk_block_sum(acc[k], red);
    __syncthreads();                       // (every read of this problem's partials is done)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) counts[(long)blockIdx.x * 4 + k] = r[k];
        mine[4] = r[4];
    }
}

// one workgroup: the problems' out-of-range counts -> *total
__global__ void __launch_bounds__(RK_BLOCK) concordance_bad_kernel(const long long* __restrict__ part, long per_problem, long problems, long long* __restrict__ total) {
    __shared__ long long red[4];
    long long acc = 0;
    for (long p = threadIdx.x; p < problems; p += RK_BLOCK) acc += part[p * per_problem * RK_PART + 4];
    acc = rk_block_sum(acc, red);
    if (threadIdx.x == 0) *total = acc;
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_concordance_workspace_bytes(long n_items, int n_problems) {
    if (n_items < 1 || n_items >= (1L << 31) || n_problems < 1) return 0;
    rk_plan p;
    rk_make_plan(n_items, n_problems, &p);
    return p.total;
}

extern "C" int amds_concordance_counts(const float* score, long score_item_stride, long score_problem_stride, const float* time, long time_problem_stride,
                                       const uint8_t* event, long event_problem_stride, const int32_t* idx, long n_base, long n_items, int n_problems,
                                       int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(score && time && event && counts && ws, "amds_concordance_counts: null pointer");
    AMDS_REQUIRE(n_items >= 1 && n_items < (1L << 31) && n_problems >= 1, "amds_concordance_counts: bad shape n_items=%ld n_problems=%d", n_items, n_problems);
    AMDS_REQUIRE(score_item_stride >= 1 && score_problem_stride >= 0 && time_problem_stride >= 0 && event_problem_stride >= 0,
                 "amds_concordance_counts: bad strides score %ld / %ld time %ld event %ld", score_item_stride, score_problem_stride, time_problem_stride,
                 event_problem_stride);
    AMDS_REQUIRE(!idx || (n_base >= 1 && n_base < (1L << 31)), "amds_concordance_counts: bad base size %ld", n_base);
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_concordance_counts: workspace not 256-byte aligned");
    rk_plan p;
    rk_make_plan(n_items, n_problems, &p);
    if (ws_bytes < p.total) {
        set_error("amds_concordance_counts: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    long long* part = (long long*)ws;
    long long* bad_dev = (long long*)((char*)ws + p.part_bytes);
    const long per_problem = p.i_tiles * p.j_chunks;
    for (int p0 = 0; p0 < n_problems; p0 += 65535) {          // (grid.z holds 65535 problems)
        const int batch = n_problems - p0 < 65535 ? n_problems - p0 : 65535;
        hipLaunchKernelGGL(concordance_pairs_kernel, dim3((unsigned)p.i_tiles, (unsigned)p.j_chunks, (unsigned)batch), dim3(RK_BLOCK), 0, st, score,
                           score_item_stride, score_problem_stride, time, time_problem_stride, event, event_problem_stride, idx, n_base, n_items, p.chunk, p0,
                           part + (long)p0 * per_problem * RK_PART);
        AMDS_LAUNCH_CHECK("concordance_pairs_kernel");
    }
    hipLaunchKernelGGL(concordance_fold_kernel, dim3((unsigned)n_problems), dim3(RK_BLOCK), 0, st, part, per_problem, (long long*)counts);
    AMDS_LAUNCH_CHECK("concordance_fold_kernel");
    if (!idx) return AMDS_OK;
    hipLaunchKernelGGL(concordance_bad_kernel, dim3(1), dim3(RK_BLOCK), 0, st, part, per_problem, (long)n_problems, bad_dev);
    AMDS_LAUNCH_CHECK("concordance_bad_kernel");
    long long bad = 0;
    AMDS_HIP(hipMemcpyAsync(&bad, bad_dev, sizeof bad, hipMemcpyDeviceToHost, st));
    AMDS_HIP(hipStreamSynchronize(st));
    AMDS_REQUIRE(bad == 0, "amds_concordance_counts: %lld index value(s) lie outside [0, %ld)", bad, n_base);
    return AMDS_OK;
}
