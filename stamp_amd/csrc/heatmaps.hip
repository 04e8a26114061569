// heatmaps.hip -- the per-slide heat-map arithmetic around amds_mil_vit_gradcam (csrc/mil_vit_train.hip): the softmax over the tiles and the scatter of per-tile
// values onto the slide's tile grid (reference src/stamp/heatmaps/__init__.py:55-56 and `_vals_to_im` :142-156).  Both are small and deterministic: no float atomics.
#include "common.h"

namespace amds {
namespace {

// fixed-order block reductions over 1024 threads (16 waves): butterfly inside a wave, then the 16 wave results in index order by every thread
template <bool MAX>
__device__ __forceinline__ float block_reduce_1024(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o);
        v = MAX ? fmaxf(v, u) : v + u;
    }
    __syncthreads();                                  // (red may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) r = MAX ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// one workgroup per class: max over the tiles, sum of exp, then out[t][c] = exp(in[c][t] - max) / sum
__global__ void __launch_bounds__(1024) softmax_over_tiles_kernel(const float* __restrict__ in, float* __restrict__ out, int classes, long n) {
    __shared__ float red[16];
    const int c = blockIdx.x;
    const float* x = in + (long)c * n;
    float m = -INFINITY;
    for (long t = threadIdx.x; t < n; t += 1024) m = fmaxf(m, x[t]);
    m = block_reduce_1024<true>(m, red);
    float s = 0.f;
    for (long t = threadIdx.x; t < n; t += 1024) s += expf(x[t] - m);
    s = block_reduce_1024<false>(s, red);
    const float inv = 1.0f / s;
    for (long t = threadIdx.x; t < n; t += 1024) out[t * classes + c] = expf(x[t] - m) * inv;
}

// pass 1: cell[y * w + x] = max tile index that names the cell (cells start at -1); out-of-grid coordinates are counted into cell[h * w], never dereferenced
__global__ void __launch_bounds__(256) scatter_cells_kernel(const int64_t* __restrict__ xy, int* __restrict__ cell, long n, int h, int w) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t x = xy[2 * t], y = xy[2 * t + 1];
    if (x < 0 || x >= w || y < 0 || y >= h) {
        atomicAdd(cell + (long)h * w, 1);
        return;
    }
    atomicMax(cell + y * w + x, (int)t);
}

// pass 2: out[cell][:] = vals[winner][:], zeros where no tile names the cell
__global__ void __launch_bounds__(256) scatter_copy_kernel(const float* __restrict__ vals, const int* __restrict__ cell, float* __restrict__ out, long cells, int k) {
    const long total = cells * k;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long ce = i / k;
        const int t = cell[ce];
        out[i] = t >= 0 ? vals[(long)t * k + (i - ce * k)] : 0.f;
    }
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" int amds_softmax_over_tiles(const float* in, float* out, int classes, long n, void* stream) {
    AMDS_REQUIRE(in && out, "amds_softmax_over_tiles: null pointer");
    AMDS_REQUIRE(classes >= 1 && classes <= 65535 && n >= 1 && n < (1L << 31), "amds_softmax_over_tiles: bad shape classes=%d n=%ld", classes, n);
    hipLaunchKernelGGL(softmax_over_tiles_kernel, dim3(classes), dim3(1024), 0, (hipStream_t)stream, in, out, classes, n);
    AMDS_LAUNCH_CHECK("softmax_over_tiles_kernel");
    return AMDS_OK;
}

// pass 1 of both entries: every cell -1, the out-of-grid count 0, then the winners
static int scatter_cells_launch(const int64_t* xy, int* cell_ws, long n, int h, int w, hipStream_t st) {
    const long cells = (long)h * w;
    AMDS_HIP(hipMemsetAsync(cell_ws, 0xff, (size_t)cells * 4, st));              // every cell -1
    AMDS_HIP(hipMemsetAsync(cell_ws + cells, 0, 4, st));                         // the out-of-grid count
    hipLaunchKernelGGL(scatter_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xy, cell_ws, n, h, w);
    AMDS_LAUNCH_CHECK("scatter_cells_kernel");
    return AMDS_OK;
}

// the one host read of both entries: the out-of-grid count
static int scatter_cells_check(const char* who, const int* cell_ws, long n, int h, int w, hipStream_t st) {
    int bad = 0;
    AMDS_HIP(hipMemcpyAsync(&bad, cell_ws + (long)h * w, 4, hipMemcpyDeviceToHost, st));
    AMDS_HIP(hipStreamSynchronize(st));
    AMDS_REQUIRE(bad == 0, "%s: %d of %ld coordinates lie outside the %d x %d grid", who, bad, n, w, h);
    return AMDS_OK;
}

extern "C" int amds_scatter_grid(const float* vals, const int64_t* xy, float* out, int* cell_ws, long n, int k, int h, int w, void* stream) {
    AMDS_REQUIRE(vals && xy && out && cell_ws, "amds_scatter_grid: null pointer");
    AMDS_REQUIRE(n >= 1 && n < (1L << 31) && k >= 1 && h >= 1 && w >= 1 && (long)h * w < (1L << 31) - 1 && (long)h * w * k < (1L << 40),
                 "amds_scatter_grid: bad shape n=%ld k=%d h=%d w=%d", n, k, h, w);
    hipStream_t st = (hipStream_t)stream;
    const long cells = (long)h * w;
    if (const int rc = scatter_cells_launch(xy, cell_ws, n, h, w, st)) return rc;
    const long blocks = (cells * k + 255) / 256;
    hipLaunchKernelGGL(scatter_copy_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, vals, cell_ws, out, cells, k);
    AMDS_LAUNCH_CHECK("scatter_copy_kernel");
    return scatter_cells_check("amds_scatter_grid", cell_ws, n, h, w, st);
}

extern "C" int amds_scatter_cells(const int64_t* xy, int* cell_ws, long n, int h, int w, void* stream) {
    AMDS_REQUIRE(xy && cell_ws, "amds_scatter_cells: null pointer");
    AMDS_REQUIRE(n >= 1 && n < (1L << 31) && h >= 1 && w >= 1 && (long)h * w < (1L << 31) - 1, "amds_scatter_cells: bad shape n=%ld h=%d w=%d", n, h, w);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = scatter_cells_launch(xy, cell_ws, n, h, w, st)) return rc;
    return scatter_cells_check("amds_scatter_cells", cell_ws, n, h, w, st);
}
