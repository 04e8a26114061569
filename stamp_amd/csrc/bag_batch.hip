// bag_batch.hip -- a whole training batch of fixed-size bags out of a feature store that stays in HBM, in ONE launch:
//   * amds_bag_batch_gather   bags_out[b][i] = cast(vp(float(store[idx[b][i]]))), zero rows for idx = -1, zero columns cols..out_ld, coordinates alongside
//                             (reference src/stamp/modeling/data.py:811-862 `_to_fixed_size_bag` + the `.float()` of :617, for n_bags bags at once; the
//                             optional vp is src/stamp/modeling/transforms.py:5-29 with counter-based shifts)
//   * amds_bag_batch_shifts   the shifts that call draws, as u8, for tests
//   * amds_bag_plan           an epoch's bag indices (the idx the gather takes) in one launch: randperm(rows)[:bag_size] per patient as a keyed bijection
// One wave per output row (a row of the store is one contiguous run: 2 KiB at 1 024 fp16 features), lanes over 8-element chunks: 16-byte loads and
// stores when the pitches allow it, element-wise otherwise.  Every offset is 64-bit: the store is meant to exceed 4 GiB.  No atomics; a pure function
// of its arguments.
#include "launch.h"

namespace amds {

// Number of low mantissa bits to clear in output element e (e = (row of the batch) * cols + column): uniform on [0, k), k = 23 - min_fraction_bits.
// The dropout hash of common.h, 16 bits per element: (h16 * k) >> 16 takes each value with probability within 2^-16 of 1 / k.
__device__ __forceinline__ uint32_t vp_shift_of(uint32_t pair_bits, int odd, uint32_t k) { return (((pair_bits >> (odd ? 16 : 0)) & 0xFFFFu) * k) >> 16; }
__device__ __forceinline__ uint32_t vp_shift(uint64_t seed, uint32_t stream, long e, uint32_t k) {
    const uint32_t key = drop_rowkey(seed, stream, (uint64_t)(e >> 16));
    return vp_shift_of(drop_pair_bits(key, (uint32_t)(e & 0xFFFF) >> 1), (int)(e & 1), k);
}
__device__ __forceinline__ float vp_mask(float v, uint32_t s) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) & (~0u << s)); }

template <typename T> struct V8 { typedef T type __attribute__((ext_vector_type(8))); };

// VEC: store_ld and out_ld are multiples of 8 elements and both bases 16-byte aligned; a lane owns the chunk [c0, c0 + 8) of its wave's row, the chunk that
// straddles `cols` reads its valid elements one by one and the chunks behind it only store zeros.  !VEC: a lane owns single elements.
template <typename TI, typename TO, bool VEC>
__global__ void __launch_bounds__(256) bag_batch_gather_kernel(const TI* __restrict__ store, long store_ld, const float* __restrict__ store_coords,
                                                               const long* __restrict__ idx, TO* __restrict__ out, long out_ld, float* __restrict__ coords_out,
                                                               long n_rows, int cols, uint32_t k, uint64_t seed, uint32_t stream) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long)gridDim.x * 4;
    for (long r = wave; r < n_rows; r += n_waves) {
        const long src = idx[r];
        const bool real = src >= 0;
        const TI* s = store + (real ? src : 0) * store_ld;
        TO* d = out + r * out_ld;
        const long e_row = r * (long)cols;
        if (coords_out && lane < 2) coords_out[r * 2 + lane] = real ? store_coords[src * 2 + lane] : 0.f;
        if constexpr (VEC) {
            typedef typename V8<TI>::type vi;
            typedef typename V8<TO>::type vo;
            for (int c0 = lane * 8; c0 < (int)out_ld; c0 += 512) {
                float v[8];
                const bool full = c0 + 8 <= cols;
                if (real && full) {
                    const vi a = *reinterpret_cast<const vi*>(s + c0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (real && c0 + j < cols) ? (float)s[c0 + j] : 0.f;
                }
                if (k && real && c0 < cols) {
                    const long e0 = e_row + c0;
                    if (full && (e0 & 7) == 0) {                        // aligned: one row key, one hash per element pair
                        const uint32_t key = drop_rowkey(seed, stream, (uint64_t)(e0 >> 16));
                        const uint32_t p0 = (uint32_t)(e0 & 0xFFFF) >> 1;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint32_t bits = drop_pair_bits(key, p0 + q);
                            v[2 * q] = vp_mask(v[2 * q], vp_shift_of(bits, 0, k));
                            v[2 * q + 1] = vp_mask(v[2 * q + 1], vp_shift_of(bits, 1, k));
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (c0 + j < cols) v[j] = vp_mask(v[j], vp_shift(seed, stream, e0 + j, k));
                    }
                }
                vo o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (TO)v[j];
                *reinterpret_cast<vo*>(d + c0) = o;
            }
        } else {
            for (int c = lane; c < (int)out_ld; c += 64) {
                float v = (real && c < cols) ? (float)s[c] : 0.f;
                if (k && real && c < cols) v = vp_mask(v, vp_shift(seed, stream, e_row + c, k));
                d[c] = (TO)v;
            }
        }
    }
}

__global__ void __launch_bounds__(256) bag_batch_shifts_kernel(uint8_t* __restrict__ shifts, long n, uint32_t k, uint64_t seed, uint32_t stream) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) shifts[i] = (uint8_t)(k ? vp_shift(seed, stream, i, k) : 0u);
}

// ---- amds_bag_plan: randperm(rows)[:bag_size] per patient as a keyed bijection of [0, rows) -------------------------------------------------------------
// A balanced Feistel network on 2 * half bits (half = ceil(bits / 2), bits = max(2, ceil(log2 rows))), cycle-walked into [0, rows).  Round keys: murmur
// finalisers of the patient key drop_rowkey(seed, epoch, p) and the round number; round function: fmix32(half ^ round key) & mask.  12 rounds: the few-round
// networks are visibly unfair on domains of 4 .. 64 values (DESIGN.md section 4.31 has the table); the cost is bag_size hash chains per patient and epoch.
constexpr int PLAN_ROUNDS = 12;

__device__ __forceinline__ uint32_t plan_feistel(uint32_t x, const uint32_t (&rk)[PLAN_ROUNDS], int half, uint32_t mask) {
    uint32_t L = x >> half, R = x & mask;
#pragma unroll
    for (int r = 0; r < PLAN_ROUNDS; ++r) {
        const uint32_t t = L ^ (fmix32(R ^ rk[r]) & mask);
        L = R;
        R = t;
    }
    return (L << half) | R;
}

// One thread per entry (b, j) of idx.  The walk starts at j < rows and the network is a bijection of [0, domain): the orbit of j returns to [0, rows) after at
// most domain - rows + 1 applications (the values it visits outside are distinct), which is the loop's trip limit.
__global__ void __launch_bounds__(256) bag_plan_kernel(const int* __restrict__ offsets, const long* __restrict__ patients, long* __restrict__ idx,
                                                       long* __restrict__ sizes, long n_entries, int bag_size, uint64_t seed, uint32_t epoch) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n_entries; i += stride) {
        const long b = i / bag_size;
        const int j = (int)(i - b * bag_size);
        const long p = patients[b];
        const int o = offsets[p];
        const int rows = offsets[p + 1] - o;
        const int m = rows < bag_size ? rows : bag_size;
        if (j == 0) sizes[b] = m > 0 ? m : 0;
        long v = -1;
        if (j < m) {
            const int bits = rows <= 4 ? 2 : 32 - __builtin_clz((uint32_t)(rows - 1));
            const int half = (bits + 1) >> 1;
            const uint32_t mask = (1u << half) - 1u;
            const uint64_t limit = (1ull << (2 * half)) - (uint64_t)rows + 1ull;
            const uint32_t key = drop_rowkey(seed, epoch, (uint64_t)p);
            uint32_t rk[PLAN_ROUNDS];
#pragma unroll
            for (int r = 0; r < PLAN_ROUNDS; ++r) rk[r] = fmix32(key ^ ((uint32_t)(r + 1) * 0x9E3779B1u));
            uint32_t x = (uint32_t)j;
            for (uint64_t s = 0; s < limit; ++s) {
                x = plan_feistel(x, rk, half, mask);
                if (x < (uint32_t)rows) break;
            }
            if (x < (uint32_t)rows) v = (long)o + (long)x;
        }
        idx[i] = v;
    }
}

template <typename TI, typename TO>
static void launch_gather(bool vec, dim3 grid, hipStream_t st, const void* store, long store_ld, const float* store_coords, const long* idx, void* out, long out_ld,
                          float* coords_out, long n_rows, int cols, uint32_t k, uint64_t seed, uint32_t stream_id) {
    if (vec)
        hipLaunchKernelGGL((bag_batch_gather_kernel<TI, TO, true>), grid, dim3(256), 0, st, (const TI*)store, store_ld, store_coords, idx, (TO*)out, out_ld, coords_out,
                           n_rows, cols, k, seed, stream_id);
    else
        hipLaunchKernelGGL((bag_batch_gather_kernel<TI, TO, false>), grid, dim3(256), 0, st, (const TI*)store, store_ld, store_coords, idx, (TO*)out, out_ld, coords_out,
                           n_rows, cols, k, seed, stream_id);
}

}  // namespace amds

using namespace amds;

#define VP_BITS_OK(b) ((b) >= 0 && (b) <= 22)

extern "C" int amds_bag_batch_gather(const void* store, long store_ld, int store_dtype, const float* store_coords, const long* idx, void* bags_out, long out_ld,
                                     int out_dtype, float* coords_out, int n_bags, int bag_size, int cols, int vp_min_fraction_bits, uint64_t seed,
                                     uint32_t stream_id, void* stream) {
    AMDS_REQUIRE(store && idx && bags_out, "amds_bag_batch_gather: null pointer (store, idx and bags_out are required)");
    AMDS_REQUIRE((store_coords == nullptr) == (coords_out == nullptr), "amds_bag_batch_gather: null pointer (store_coords and coords_out come together or not at all)");
    AMDS_REQUIRE(n_bags >= 0, "amds_bag_batch_gather: n_bags=%d must be >= 0", n_bags);
    AMDS_REQUIRE(bag_size >= 1, "amds_bag_batch_gather: bag_size=%d must be >= 1", bag_size);
    AMDS_REQUIRE(cols >= 1 && store_ld >= cols, "amds_bag_batch_gather: store_ld=%ld < cols=%d (or cols < 1)", store_ld, cols);
    AMDS_REQUIRE(out_ld >= cols, "amds_bag_batch_gather: out_ld=%ld < cols=%d", out_ld, cols);
    AMDS_REQUIRE(out_ld < (1L << 31), "amds_bag_batch_gather: out_ld=%ld does not fit 31 bits", out_ld);
    AMDS_REQUIRE(VP_BITS_OK(vp_min_fraction_bits), "amds_bag_batch_gather: vp_min_fraction_bits=%d outside 0..22 (0 = off)", vp_min_fraction_bits);
    const bool pair_ok = (store_dtype == AMDS_F16 && (out_dtype == AMDS_F32 || out_dtype == AMDS_F16 || out_dtype == AMDS_BF16)) ||
                         (store_dtype == AMDS_F32 && out_dtype == AMDS_F32);
    AMDS_REQUIRE(pair_ok, "amds_bag_batch_gather: unsupported dtype pair %d -> %d (f16 -> f32 / f16 / bf16, f32 -> f32)", store_dtype, out_dtype);
    if (n_bags == 0) return AMDS_OK;
    const long n_rows = (long)n_bags * bag_size;
    const uint32_t k = vp_min_fraction_bits ? (uint32_t)(23 - vp_min_fraction_bits) : 0u;
    const bool vec = store_ld % 8 == 0 && out_ld % 8 == 0 && ((uintptr_t)store & 15) == 0 && ((uintptr_t)bags_out & 15) == 0;
    const dim3 grid((unsigned)min((long)8192, (n_rows + 3) / 4));
    hipStream_t st = (hipStream_t)stream;
    if (store_dtype == AMDS_F32)
        launch_gather<float, float>(vec, grid, st, store, store_ld, store_coords, idx, bags_out, out_ld, coords_out, n_rows, cols, k, seed, stream_id);
    else if (out_dtype == AMDS_F32)
        launch_gather<f16, float>(vec, grid, st, store, store_ld, store_coords, idx, bags_out, out_ld, coords_out, n_rows, cols, k, seed, stream_id);
    else if (out_dtype == AMDS_F16)
        launch_gather<f16, f16>(vec, grid, st, store, store_ld, store_coords, idx, bags_out, out_ld, coords_out, n_rows, cols, k, seed, stream_id);
    else
        launch_gather<f16, bf16>(vec, grid, st, store, store_ld, store_coords, idx, bags_out, out_ld, coords_out, n_rows, cols, k, seed, stream_id);
    AMDS_LAUNCH_CHECK("bag_batch_gather_kernel");
    return AMDS_OK;
}

extern "C" int amds_bag_batch_shifts(uint8_t* shifts, int n_bags, int bag_size, int cols, int vp_min_fraction_bits, uint64_t seed, uint32_t stream_id,
                                     void* stream) {
    AMDS_REQUIRE(shifts, "amds_bag_batch_shifts: null pointer");
    AMDS_REQUIRE(n_bags >= 0 && bag_size >= 1 && cols >= 1, "amds_bag_batch_shifts: bad sizes n_bags=%d bag_size=%d cols=%d", n_bags, bag_size, cols);
    AMDS_REQUIRE(VP_BITS_OK(vp_min_fraction_bits), "amds_bag_batch_shifts: vp_min_fraction_bits=%d outside 0..22 (0 = off)", vp_min_fraction_bits);
    if (n_bags == 0) return AMDS_OK;
    const long n = (long)n_bags * bag_size * cols;
    const uint32_t k = vp_min_fraction_bits ? (uint32_t)(23 - vp_min_fraction_bits) : 0u;
    hipLaunchKernelGGL(bag_batch_shifts_kernel, dim3((unsigned)min((long)4096, (n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, shifts, n, k, seed, stream_id);
    AMDS_LAUNCH_CHECK("bag_batch_shifts_kernel");
    return AMDS_OK;
}

extern "C" int amds_bag_plan(const int* offsets, const long* patients, long* idx, long* sizes, int n, int bag_size, uint64_t seed, uint32_t epoch, void* stream) {
    AMDS_REQUIRE(offsets && patients && idx && sizes, "amds_bag_plan: null pointer");
    AMDS_REQUIRE(n >= 0, "amds_bag_plan: n=%d must be >= 0", n);
    AMDS_REQUIRE(bag_size >= 1, "amds_bag_plan: bag_size=%d must be >= 1", bag_size);
    if (n == 0) return AMDS_OK;
    const long n_entries = (long)n * bag_size;
    hipLaunchKernelGGL(bag_plan_kernel, dim3((unsigned)min((long)4096, (n_entries + 255) / 256)), dim3(256), 0, (hipStream_t)stream, offsets, patients, idx, sizes,
                       n_entries, bag_size, seed, epoch);
    AMDS_LAUNCH_CHECK("bag_plan_kernel");
    return AMDS_OK;
}
