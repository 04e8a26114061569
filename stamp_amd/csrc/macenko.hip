// macenko.hip -- Macenko stain normalisation of decoded RGB tiles, one workgroup per tile, the tile staged ONCE through LDS.
// BASELINE.json's north_star names the step ("tile decode + Macenko colour-norm + background reject ... staging RGB tiles through LDS with
// coalesced HBM writes"); the reference (KatherLab/STAMP v2.5.0) does not contain it, so this is an OPTIONAL stage, off by
// default, and its parity is UNPINNED: it is checked against oracle/macenko.py, a restatement of the published algorithm (Macenko et al.,
// ISBI 2009) with the conventions stated there.
//   pass 1  OD = -log((I + 1) / Io) per pixel; pixels with any channel below beta are unstained; sums for cov(OD) over the stained ones
//   fit     eigenvectors of the 3 x 3 covariance (Jacobi, double, one lane); the plane of the two largest
//   pass 2  angle histogram of the stained pixels in that plane -> alpha / (100 - alpha) percentiles -> the two stain vectors, 2 x 3 pseudo-inverse
//   pass 3  concentrations C = pinv * OD of ALL pixels -> two histograms -> 99th percentiles -> scale to the reference maxima
//   pass 4  I' = Io * exp(-HERef * C'), floor, clip, written back into the LDS tile and stored with 16-byte rows
// HBM traffic: 150 528 B in + 150 528 B out per tile (the algorithmic minimum); everything else is LDS / VALU.
#include "launch.h"

namespace amds {

constexpr int MK_T = 1024;                 // threads per tile
constexpr int MK_HB = 2048;                // angle bins over [0, pi]; the two concentration histograms use 1024 each
constexpr float MK_CMAX = 8.0f;            // concentration histogram range [0, 8)

__device__ __forceinline__ void mk_od(const unsigned char* p, float inv_io, float od[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) od[c] = -__logf(((float)p[c] + 1.0f) * inv_io);
}

// symmetric 3 x 3 eigen-decomposition by cyclic Jacobi (double): eigenvalues ascending in w, eigenvectors in the columns of v
__device__ void mk_eigh3(double a[3][3], double w[3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        if (off < 1e-18) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(a[p][q]) < 1e-300) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq; }
                for (int k = 0; k < 3; ++k) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk; }
                for (int k = 0; k < 3; ++k) { const double vkp = v[k][p], vkq = v[k][q]; v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq; }
            }
    }
    for (int i = 0; i < 3; ++i) w[i] = a[i][i];
    for (int i = 0; i < 2; ++i)                      // sort ascending (3 elements)
        for (int j = 0; j < 2 - i; ++j)
            if (w[j] > w[j + 1]) {
                const double tw = w[j]; w[j] = w[j + 1]; w[j + 1] = tw;
                for (int k = 0; k < 3; ++k) { const double tv = v[k][j]; v[k][j] = v[k][j + 1]; v[k][j + 1] = tv; }
            }
}

// value at the q-quantile of a histogram (linear inside the bin), counts in h[0..nb), range [lo, lo + nb * width)
__device__ float mk_quantile(const unsigned* h, int nb, float lo, float width, float total, float q) {
    const float target = q * (total - 1.0f);          // numpy's linear-interpolation rank
    float cum = 0.f;
    for (int b = 0; b < nb; ++b) {
        const float c = (float)h[b];
        if (cum + c > target) return lo + width * ((float)b + (c > 0.f ? (target - cum + 0.5f) / c : 0.5f));
        cum += c;
    }
    return lo + width * nb;
}

__global__ void __launch_bounds__(MK_T) macenko_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, float* __restrict__ fit_out,
                                                       int npix, float Io, float alpha, float beta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* tile = smem;
    const int tile_bytes = npix * 3, tile_pad = (tile_bytes + 15) & ~15;
    unsigned* hist = reinterpret_cast<unsigned*>(smem + tile_pad);                  // MK_HB bins
    float* red = reinterpret_cast<float*>(hist + MK_HB);                             // [16 waves][10] + fit parameters [32]
    float* fit = red + 16 * 10;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char* src = in + (long)blockIdx.x * tile_bytes;
    unsigned char* dst = out + (long)blockIdx.x * tile_bytes;
    for (int i = tid * 16; i < tile_bytes; i += MK_T * 16) {
        if (i + 16 <= tile_bytes && (((uintptr_t)(src + i)) & 15) == 0) *reinterpret_cast<u32x4*>(tile + i) = *reinterpret_cast<const u32x4*>(src + i);
        else for (int k = i; k < min(i + 16, tile_bytes); ++k) tile[k] = src[k];
    }
    for (int i = tid; i < MK_HB; i += MK_T) hist[i] = 0u;
    __syncthreads();
    const float inv_io = 1.0f / Io;
    // ---- pass 1: moments of the stained pixels ----
    float acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.f;
    for (int p = tid; p < npix; p += MK_T) {
        float od[3];
        mk_od(tile + p * 3, inv_io, od);
        if (od[0] >= beta && od[1] >= beta && od[2] >= beta) {
            acc[0] += 1.f; acc[1] += od[0]; acc[2] += od[1]; acc[3] += od[2];
            acc[4] += od[0] * od[0]; acc[5] += od[0] * od[1]; acc[6] += od[0] * od[2]; acc[7] += od[1] * od[1]; acc[8] += od[1] * od[2]; acc[9] += od[2] * od[2];
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) { const float s = wave_sum(acc[k]); if (lane == 0) red[wave * 10 + k] = s; }
    __syncthreads();
    if (tid == 0) {
        double m[10];
        for (int k = 0; k < 10; ++k) { double s = 0; for (int w8 = 0; w8 < MK_T / 64; ++w8) s += red[w8 * 10 + k]; m[k] = s; }
        const double n = m[0];
        fit[0] = (float)n;
        if (n >= 16.0) {
            const double mu[3] = {m[1] / n, m[2] / n, m[3] / n};
            double a[3][3], w[3], v[3][3];
            const double sxx[3][3] = {{m[4], m[5], m[6]}, {m[5], m[7], m[8]}, {m[6], m[8], m[9]}};
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) a[i][j] = (sxx[i][j] - n * mu[i] * mu[j]) / (n - 1.0);       // np.cov: unbiased
            mk_eigh3(a, w, v);
            double e1[3] = {v[0][1], v[1][1], v[2][1]}, e2[3] = {v[0][2], v[1][2], v[2][2]};
            if (e2[0] + e2[1] + e2[2] < 0) for (int k = 0; k < 3; ++k) e2[k] = -e2[k];
            for (int k = 0; k < 3; ++k) { fit[1 + k] = (float)e1[k]; fit[4 + k] = (float)e2[k]; }
        }
    }
    __syncthreads();
    const float nst = fit[0];
    if (nst < 16.f) {                                // background tile: passed through unchanged
        for (int i = tid * 16; i < tile_bytes; i += MK_T * 16) {
            if (i + 16 <= tile_bytes && (((uintptr_t)(dst + i)) & 15) == 0) *reinterpret_cast<u32x4*>(dst + i) = *reinterpret_cast<const u32x4*>(tile + i);
            else for (int k = i; k < min(i + 16, tile_bytes); ++k) dst[k] = tile[k];
        }
        if (fit_out && tid < 8) fit_out[(long)blockIdx.x * 8 + tid] = 0.f;
        return;
    }
    // ---- pass 2: angle histogram of the stained pixels in the (e1, e2) plane ----
    {
        const float e1x = fit[1], e1y = fit[2], e1z = fit[3], e2x = fit[4], e2y = fit[5], e2z = fit[6];
        const float bw = 3.14159265358979f / MK_HB;
        for (int p = tid; p < npix; p += MK_T) {
            float od[3];
            mk_od(tile + p * 3, inv_io, od);
            if (od[0] >= beta && od[1] >= beta && od[2] >= beta) {
                const float t0 = od[0] * e1x + od[1] * e1y + od[2] * e1z, t1 = od[0] * e2x + od[1] * e2y + od[2] * e2z;
                float phi = atan2f(t1, t0);
                phi = fminf(fmaxf(phi, 0.f), 3.14159f);
                atomicAdd(&hist[min((int)(phi / bw), MK_HB - 1)], 1u);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float bw = 3.14159265358979f / MK_HB;
        const float lo = mk_quantile(hist, MK_HB, 0.f, bw, nst, alpha * 0.01f), hi = mk_quantile(hist, MK_HB, 0.f, bw, nst, 1.0f - alpha * 0.01f);
        float vmin[3], vmax[3];
        for (int k = 0; k < 3; ++k) { vmin[k] = fit[1 + k] * cosf(lo) + fit[4 + k] * sinf(lo); vmax[k] = fit[1 + k] * cosf(hi) + fit[4 + k] * sinf(hi); }
        const bool first = vmin[0] > vmax[0];
        float h0[3], h1[3];
        for (int k = 0; k < 3; ++k) { h0[k] = first ? vmin[k] : vmax[k]; h1[k] = first ? vmax[k] : vmin[k]; }
        // pseudo-inverse of HE [3 x 2]: (HE^T HE)^-1 HE^T
        const float a = h0[0] * h0[0] + h0[1] * h0[1] + h0[2] * h0[2], b = h0[0] * h1[0] + h0[1] * h1[1] + h0[2] * h1[2], d = h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2];
        const float det = a * d - b * b, ia = d / det, ib = -b / det, id = a / det;
        for (int k = 0; k < 3; ++k) { fit[8 + k] = ia * h0[k] + ib * h1[k]; fit[11 + k] = ib * h0[k] + id * h1[k]; fit[16 + k] = h0[k]; fit[19 + k] = h1[k]; }
    }
    __syncthreads();
    for (int i = tid; i < MK_HB; i += MK_T) hist[i] = 0u;
    __syncthreads();
    // ---- pass 3: concentration histograms of ALL pixels ----
    const float p00 = fit[8], p01 = fit[9], p02 = fit[10], p10 = fit[11], p11 = fit[12], p12 = fit[13];
    {
        const float cw = MK_CMAX / (MK_HB / 2);
        for (int p = tid; p < npix; p += MK_T) {
            float od[3];
            mk_od(tile + p * 3, inv_io, od);
            const float c0 = p00 * od[0] + p01 * od[1] + p02 * od[2], c1 = p10 * od[0] + p11 * od[1] + p12 * od[2];
            atomicAdd(&hist[min(max((int)(c0 / cw), 0), MK_HB / 2 - 1)], 1u);
            atomicAdd(&hist[MK_HB / 2 + min(max((int)(c1 / cw), 0), MK_HB / 2 - 1)], 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float cw = MK_CMAX / (MK_HB / 2);
        const float m0 = mk_quantile(hist, MK_HB / 2, 0.f, cw, (float)npix, 0.99f), m1 = mk_quantile(hist + MK_HB / 2, MK_HB / 2, 0.f, cw, (float)npix, 0.99f);
        fit[14] = 1.9705f / fmaxf(m0, 1e-6f);
        fit[15] = 1.0308f / fmaxf(m1, 1e-6f);
        fit[22] = m0; fit[23] = m1;
    }
    __syncthreads();
    // ---- pass 4: rebuild with the reference stain vectors, in place in LDS, then 16-byte stores ----
    {
        const float s0 = fit[14], s1 = fit[15];
        for (int p = tid; p < npix; p += MK_T) {
            float od[3];
            mk_od(tile + p * 3, inv_io, od);
            const float c0 = (p00 * od[0] + p01 * od[1] + p02 * od[2]) * s0, c1 = (p10 * od[0] + p11 * od[1] + p12 * od[2]) * s1;
            const float r = Io * __expf(-(0.5626f * c0 + 0.2159f * c1)), g = Io * __expf(-(0.7201f * c0 + 0.8012f * c1)), bl = Io * __expf(-(0.4062f * c0 + 0.5581f * c1));
            tile[p * 3] = (unsigned char)fminf(fmaxf(floorf(r), 0.f), 255.f);
            tile[p * 3 + 1] = (unsigned char)fminf(fmaxf(floorf(g), 0.f), 255.f);
            tile[p * 3 + 2] = (unsigned char)fminf(fmaxf(floorf(bl), 0.f), 255.f);
        }
    }
    __syncthreads();
    for (int i = tid * 16; i < tile_bytes; i += MK_T * 16) {
        if (i + 16 <= tile_bytes && (((uintptr_t)(dst + i)) & 15) == 0) *reinterpret_cast<u32x4*>(dst + i) = *reinterpret_cast<const u32x4*>(tile + i);
        else for (int k = i; k < min(i + 16, tile_bytes); ++k) dst[k] = tile[k];
    }
    if (fit_out && tid < 8) fit_out[(long)blockIdx.x * 8 + tid] = tid < 6 ? fit[16 + tid] : fit[22 + tid - 6];     // HE (haematoxylin, eosin), maxC
}

}  // namespace amds

using namespace amds;

extern "C" int amds_macenko_normalize_u8(const uint8_t* tiles, uint8_t* out, float* fit_out, int B, int H, int W, float Io, float alpha, float beta, void* stream) {
    AMDS_REQUIRE(B >= 0 && H > 0 && W > 0 && Io > 1.f && alpha > 0.f && alpha < 50.f && beta >= 0.f, "amds_macenko_normalize_u8: bad arguments");
    if (B == 0) return AMDS_OK;
    AMDS_REQUIRE(tiles && out && tiles != out, "amds_macenko_normalize_u8: null / aliased pointer");
    const int npix = H * W;
    const size_t lds = (((size_t)npix * 3 + 15) & ~(size_t)15) + MK_HB * 4 + (16 * 10 + 32) * 4;
    AMDS_REQUIRE(lds <= 160 * 1024, "amds_macenko_normalize_u8: a %d x %d tile does not fit in LDS", H, W);
    AMDS_HIP(lds_opt_in<macenko_kernel>(160 * 1024));
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(PROF_OTHER, 2.0 * B * npix * 3, st);
    hipLaunchKernelGGL(macenko_kernel, dim3(B), dim3(MK_T), lds, st, tiles, out, fit_out, npix, Io, alpha, beta);
    AMDS_LAUNCH_CHECK("macenko_kernel");
    return AMDS_OK;
}
