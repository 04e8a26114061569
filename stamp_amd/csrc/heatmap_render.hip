// heatmap_render.hip -- the pixel work of the reference's heat-map `raw/` images (src/stamp/heatmaps/__init__.py): colour-map look-up and x`scale` pixel
// replication of the per-category score images (:500-529, 600-609, 683-717), the class map (:241-258, 437-448) and `_create_overlay` (:261-284).
// Every result is a fixed function of its inputs: integer look-ups, one fp32 multiply, binary64 blends.  No atomics, no reductions.
// hipcc contracts a * b + c into an FMA by default; a fused blend changes bytes, so contraction is off for this file (the blend is written with plain
// operators: the __dmul_rn / __dadd_rn of the HIP headers are plain operators themselves and would be contracted like any other).
#include "common.h"
#pragma clang fp contract(off)

namespace amds {
namespace {

constexpr int MAX_LUT = 256;

// the look-up table packed to one little-endian RGBA word per entry, in LDS; entries past n_lut repeat the last one
__device__ __forceinline__ void load_lut(const uint8_t* __restrict__ lut, int n_lut, uint32_t* slut) {
    for (int i = threadIdx.x; i < MAX_LUT; i += blockDim.x) {
        const uint8_t* e = lut + 4 * (i < n_lut ? i : n_lut - 1);
        slut[i] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
    }
    __syncthreads();
}

// matplotlib's Colormap.__call__ on a float, then uint8(rgba * 255): NaN -> the "bad" colour (0, 0, 0, 0); x < 0 -> "under" = lut[0];
// x * N >= N -> lut[N - 1] (x == 1 and "over"); else lut[(int)(x * N)], the product rounded to fp32 like numpy's in-place `xa *= N`
__device__ __forceinline__ uint32_t lut_rgb(const uint32_t* slut, int n_lut, float x) {
    if (x != x) return 0u;
    if (x < 0.f) return slut[0];
    const float f = x * (float)n_lut;
    return slut[f >= (float)n_lut ? n_lut - 1 : (int)f];
}

// the rows (category c, row y of H) a workgroup row takes, gridDim.y apart, without a division per step
struct RowWalk {
    unsigned H, step_c, step_y, c, y;
    __device__ explicit RowWalk(unsigned H_) : H(H_), step_c(gridDim.y / H_), step_y(gridDim.y % H_), c(blockIdx.y / H_), y(blockIdx.y % H_) {}
    __device__ void next() {
        c += step_c;
        y += step_y;
        if (y >= H) {
            y -= H;
            ++c;
        }
    }
};

// One thread per output column, the rows (category-major) strided over gridDim.y.  MODE 0: float argument through the colour map; MODE 1: integer
// class index.  cell != NULL: the sources are per tile ([C][n]) and cell[cy * w + cx] names the tile (< 0 or >= n: no tile -> argument 0, alpha 0);
// cell == NULL: the sources are images ([C][h][w]).
template <int MODE>
__global__ void __launch_bounds__(256) raster_kernel(const void* __restrict__ src, const float* __restrict__ alpha_src, const int* __restrict__ cell,
                                                     const uint8_t* __restrict__ lut, int n_lut, uint32_t* __restrict__ out, int C, long n, int h, int w,
                                                     int scale) {
    __shared__ uint32_t slut[MAX_LUT];
    load_lut(lut, n_lut, slut);
    const unsigned W = (unsigned)w * scale, H = (unsigned)h * scale;          // (both < 2^31: the entry checks)
    const unsigned ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= W) return;
    const int cx = (int)(ox / (unsigned)scale);
    const long per_cat = cell ? n : (long)h * w;
    RowWalk rw(H);
    for (; rw.c < (unsigned)C; rw.next()) {
        const long c = rw.c, r = c * H + rw.y;
        const int cy = (int)(rw.y / (unsigned)scale);
        long at = (long)cy * w + cx;
        if (cell) {
            const int t = cell[at];
            at = (t >= 0 && t < n) ? t : -1;
        }
        uint32_t px;
        if (at < 0) {
            px = slut[0] & 0x00FFFFFFu;
        } else {
            const long i = c * per_cat + at;
            uint32_t rgb;
            if (MODE == 0) {
                rgb = lut_rgb(slut, n_lut, ((const float*)src)[i]);
            } else {
                const int k = ((const int32_t*)src)[i];
                rgb = slut[k < 0 ? 0 : (k >= n_lut ? n_lut - 1 : k)];
            }
            px = (rgb & 0x00FFFFFFu) | (alpha_src[i] > 0.f ? 0xFF000000u : 0u);
        }
        out[r * W + ox] = px;
    }
}

// `_create_overlay`: one thread per thumbnail column, the rows (category-major) strided over gridDim.y.  The score image is sampled at
// [ytab[y] * scale][xtab[x] * scale] (table entries clamped into the grid: never an address outside it).  binary64 as numpy: s = byte / 255.0,
// t = thumb / 255.0, o = alpha * s + (1 - alpha) * t where the sampled alpha byte > 0, else t; out = (uint8)(o * 255.0), truncating.
__global__ void __launch_bounds__(256) overlay_kernel(const uint32_t* __restrict__ score, const uint8_t* __restrict__ thumb, const int* __restrict__ ytab,
                                                      const int* __restrict__ xtab, double alpha, double one_minus_alpha, uint8_t* __restrict__ out, int C,
                                                      int h, int w, int scale, int th, int tw) {
    __shared__ double unit[256];                       // byte / 255.0, one IEEE division per entry
    unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    const long x = (long)blockIdx.x * 256 + threadIdx.x;
    if (x >= tw) return;
    int sx = xtab[x];
    sx = sx < 0 ? 0 : (sx >= w ? w - 1 : sx);
    const long W = (long)w * scale, H = (long)h * scale;
    RowWalk rw((unsigned)th);
    for (; rw.c < (unsigned)C; rw.next()) {
        const long c = rw.c, y = rw.y, r = c * th + y;
        int sy = ytab[y];
        sy = sy < 0 ? 0 : (sy >= h ? h - 1 : sy);
        const uint32_t s = score[(c * H + (long)sy * scale) * W + (long)sx * scale];
        const uint8_t* tp = thumb + (y * tw + x) * 3;
        uint8_t* op = out + (r * tw + x) * 3;
        const bool blend = (s >> 24) != 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double t = unit[tp[ch]];
            double o = t;
            if (blend) {
                const double a = alpha * unit[(s >> (8 * ch)) & 0xFFu];
                const double b = one_minus_alpha * t;
                o = a + b;
            }
            op[ch] = (uint8_t)(int)(o * 255.0);
        }
    }
}

unsigned row_blocks(long rows) { return (unsigned)(rows < 4096 ? rows : 4096); }

int raster_launch(int mode, const char* who, const void* src, const float* alpha_src, const int* cell, const uint8_t* lut, int n_lut, uint8_t* out, int C,
                  long n, int h, int w, int scale, void* stream) {
    AMDS_REQUIRE(src && alpha_src && lut && out, "%s: null pointer", who);
    AMDS_REQUIRE(((uintptr_t)out & 3) == 0, "%s: out must be 4-byte aligned", who);
    AMDS_REQUIRE(C >= 1 && h >= 1 && w >= 1 && scale >= 1 && n_lut >= 1 && n_lut <= MAX_LUT && (long)h * w < (1L << 31) - 1 && (long)h * scale < (1L << 31) &&
                     (long)w * scale < (1L << 31) && (!cell || (n >= 1 && n < (1L << 31))) && (double)C * h * w * scale * scale < (double)(1L << 44),
                 "%s: bad shape C=%d n=%ld h=%d w=%d scale=%d n_lut=%d", who, C, n, h, w, scale, n_lut);
    const long W = (long)w * scale, rows = (long)h * scale * C;
    const dim3 grid((unsigned)((W + 255) / 256), row_blocks(rows));
    if (mode == 0)
        hipLaunchKernelGGL(raster_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, src, alpha_src, cell, lut, n_lut, (uint32_t*)out, C, n, h, w, scale);
    else
        hipLaunchKernelGGL(raster_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, alpha_src, cell, lut, n_lut, (uint32_t*)out, C, n, h, w, scale);
    AMDS_LAUNCH_CHECK("raster_kernel");
    return AMDS_OK;
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" int amds_heatmap_raster(const float* arg, const float* alpha_src, const int* cell, const uint8_t* lut, int n_lut, uint8_t* out, int n_cat, long n,
                                   int h, int w, int scale, void* stream) {
    return raster_launch(0, "amds_heatmap_raster", arg, alpha_src, cell, lut, n_lut, out, n_cat, n, h, w, scale, stream);
}

extern "C" int amds_heatmap_classmap(const int32_t* top, const float* alpha_src, const int* cell, const uint8_t* lut, int n_lut, uint8_t* out, long n, int h,
                                     int w, int scale, void* stream) {
    return raster_launch(1, "amds_heatmap_classmap", top, alpha_src, cell, lut, n_lut, out, 1, n, h, w, scale, stream);
}

extern "C" int amds_heatmap_overlay(const uint8_t* score, const uint8_t* thumb, const int32_t* ytab, const int32_t* xtab, double alpha, uint8_t* out, int n_cat,
                                    int h, int w, int scale, int th, int tw, void* stream) {
    AMDS_REQUIRE(score && thumb && ytab && xtab && out, "amds_heatmap_overlay: null pointer");
    AMDS_REQUIRE(((uintptr_t)score & 3) == 0, "amds_heatmap_overlay: score must be 4-byte aligned");
    AMDS_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "amds_heatmap_overlay: alpha %g outside [0, 1] (the bytes of a blend outside [0, 255] are not defined)", alpha);
    AMDS_REQUIRE(n_cat >= 1 && h >= 1 && w >= 1 && scale >= 1 && th >= 1 && tw >= 1 && (long)h * scale < (1L << 31) && (long)w * scale < (1L << 31) &&
                     (double)n_cat * h * w * scale * scale < (double)(1L << 44) && (double)n_cat * th * tw < (double)(1L << 44),
                 "amds_heatmap_overlay: bad shape C=%d h=%d w=%d scale=%d th=%d tw=%d", n_cat, h, w, scale, th, tw);
    const dim3 grid((unsigned)(((long)tw + 255) / 256), row_blocks((long)th * n_cat));
    hipLaunchKernelGGL(overlay_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uint32_t*)score, thumb, ytab, xtab, alpha, 1.0 - alpha, out, n_cat, h, w,
                       scale, th, tw);
    AMDS_LAUNCH_CHECK("overlay_kernel");
    return AMDS_OK;
}
