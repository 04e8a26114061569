// objective.hip -- the training objectives on the [batch, outputs] fp32 logits of every head (stamp_amd/losses.py states the reference lines):
//   amds_objective_step: a batch's scalar loss, d(loss)/d(logits), whether the loss has a gradient at all, and the epoch's running sums -- ONE launch;
//   amds_objective_rows: the loss of every row on its own (validation: N one-row batches in one launch).
// include/amdstamp.h states the formulas.  How they run:
//   * CE: one wave per row, lanes strided over the classes; the maximum, sum(exp), sum(w y) and sum(w y (x - max)) fold over an xor butterfly, so every lane
//     holds the same bits.  `ce_row` is the one function both entries call: a row's value depends on that row and the weights alone.  amds_objective_step is
//     one workgroup: wave w walks rows w, w + 4, ... and adds their losses in that order, the four waves fold in index order.
//   * L1: one lane per row; the step's sum is thread-strided, then the same fold.
//   * Cox (Efron, Breslow): one workgroup of 1024 lanes with the batch in LDS (32 bytes per item).  No sort: item i walks all j once for its risk-set sum
//     R_i = sum(e_j : t_j >= t_i), its tie group's event sum D_i, event count d_i and its own place r_i among the tied events (by item index); the
//     gradient walks all i once more.  Both walks add in index order.  e_j = exp(lh_j - max lh), in fp64.
// Everything but the loads and the stores is fp64 (a few thousand values: the rate does not matter), rounded to fp32 once; contraction is off for the whole
// file, so the two entries cannot round one row differently.  No atomics: a call is bitwise reproducible.
#include "launch.h"

#pragma clang fp contract(off)

namespace amds {
namespace {

constexpr int OB_BLOCK = 256;                // CE and L1
constexpr int OB_WAVES = OB_BLOCK / 64;
constexpr int CX_BLOCK = 1024;               // Cox
constexpr int CX_WAVES = CX_BLOCK / 64;
constexpr int CX_MAX_ITEMS = 4096;
constexpr int CX_RED_BYTES = 256;            // fold scratch in front of the item arrays
constexpr int CX_ITEM_BYTES = 32;            // e, 1/Q, f/Q (fp64), time (fp32), event (int32)

inline int cx_lds_bytes(int n) { return CX_RED_BYTES + ((n + 1) & ~1) * CX_ITEM_BYTES; }

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// butterfly inside each wave (every lane ends with the same bits), then the waves in index order
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    return s;
}

// the dlogits scale: the host factor, then the device one -- the last multiplications
__device__ __forceinline__ float ob_scaled(float v, float scale, const float* __restrict__ scale_dev) {
    v *= scale;
    return scale_dev ? v * scale_dev[0] : v;
}

struct CeRow {
    float mx;           // max_c x_c
    double s, wy;       // sum_c exp(x_c - mx), sum_c w_c y_c
    double loss;        // sum_c -w_c y_c log p_c
};

// one wave, all 64 lanes; every lane returns the same bits
__device__ __forceinline__ CeRow ce_row(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w, int C) {
    const int lane = threadIdx.x & 63;
    CeRow r;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    double s = 0.0, wy = 0.0, dot = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)x[c] - (double)mx;
        const double a = (double)(w ? w[c] : 1.0f) * (double)y[c];
        s += exp(d);
        wy += a;
        dot += a * d;
    }
    r.mx = mx;
    r.s = wave_sum(s);
    r.wy = wave_sum(wy);
    r.loss = r.wy * log(r.s) - wave_sum(dot);          // sum_c a_c (log s - (x_c - mx))
    return r;
}

__device__ __forceinline__ void ob_finish(float loss, int grad, int B, float* __restrict__ loss_out, int32_t* __restrict__ has_grad, double* __restrict__ acc) {
    loss_out[0] = loss;
    has_grad[0] = grad;
    if (acc) acc[0] += (double)loss * (double)B, acc[1] += (double)B;
}

// one workgroup
__global__ void __launch_bounds__(OB_BLOCK) ce_step_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w, int B, int C,
                                                           float scale, const float* __restrict__ scale_dev, float* __restrict__ loss, float* __restrict__ dx,
                                                           int32_t* __restrict__ has_grad, double* __restrict__ acc) {
    __shared__ double red[OB_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum = 0.0;
    for (int n = wave; n < B; n += OB_WAVES) {
        const float* xr = x + (long)n * C;
        const float* yr = y + (long)n * C;
        const CeRow r = ce_row(xr, yr, w, C);
        sum += r.loss;
        for (int c = lane; c < C; c += 64) {
            const double p = exp((double)xr[c] - (double)r.mx) / r.s;
            const double a = (double)(w ? w[c] : 1.0f) * (double)yr[c];
            dx[(long)n * C + c] = ob_scaled((float)((p * r.wy - a) / (double)B), scale, scale_dev);
        }
    }
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int k = 1; k < OB_WAVES; ++k) s += red[k];
        ob_finish((float)(s / (double)B), 1, B, loss, has_grad, acc);
    }
}

// grid (ceil(N / 4)): one wave per row
__global__ void __launch_bounds__(OB_BLOCK) ce_rows_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ w, long N, int C,
                                                           float* __restrict__ out) {
    const long n = (long)blockIdx.x * OB_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;          // (a whole wave leaves: no barrier follows)
    const CeRow r = ce_row(x + n * C, y + n * C, w, C);
    if ((threadIdx.x & 63) == 0) out[n] = (float)r.loss;
}

// one workgroup
__global__ void __launch_bounds__(OB_BLOCK) l1_step_kernel(const float* __restrict__ p, const float* __restrict__ t, int B, float scale,
                                                           const float* __restrict__ scale_dev, float* __restrict__ loss, float* __restrict__ dp,
                                                           int32_t* __restrict__ has_grad, double* __restrict__ acc) {
    __shared__ double red[OB_WAVES];
    double sum = 0.0;
    const float g = (float)(1.0 / (double)B);
    for (int n = threadIdx.x; n < B; n += OB_BLOCK) {
        const double d = (double)p[n] - (double)t[n];
        sum += fabs(d);
        dp[n] = ob_scaled(d > 0.0 ? g : (d < 0.0 ? -g : 0.0f), scale, scale_dev);
    }
    sum = block_sum<OB_WAVES>(sum, red);
    if (threadIdx.x == 0) ob_finish((float)(sum / (double)B), 1, B, loss, has_grad, acc);
}

__global__ void __launch_bounds__(OB_BLOCK) l1_rows_kernel(const float* __restrict__ p, const float* __restrict__ t, long N, float* __restrict__ out) {
    const long n = (long)blockIdx.x * OB_BLOCK + threadIdx.x;
    if (n < N) out[n] = (float)fabs((double)p[n] - (double)t[n]);
}

// one workgroup.  Dynamic LDS: scratch [CX_RED_BYTES] | e, 1/Q, f/Q [n_pad] fp64 | time [n_pad] fp32 | event [n_pad] int32.
// te = [n][2]: time, event (an event is any value other than 0).
__global__ void __launch_bounds__(CX_BLOCK) cox_step_kernel(const float* __restrict__ lh, const float* __restrict__ te, int n, int efron, float scale,
                                                            const float* __restrict__ scale_dev, float* __restrict__ loss, float* __restrict__ dlh,
                                                            int32_t* __restrict__ has_grad, double* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ob_smem[];
    const int n_pad = (n + 1) & ~1;
    double* red = (double*)ob_smem;
    double* e = (double*)(ob_smem + CX_RED_BYTES);
    double* iq = e + n_pad;
    double* fq = iq + n_pad;
    float* tm = (float*)(fq + n_pad);
    int* ev = (int*)(tm + n_pad);
    const int tid = threadIdx.x;

    float mx = -INFINITY;
    for (int j = tid; j < n; j += CX_BLOCK) {
        tm[j] = te[2 * j];
        ev[j] = te[2 * j + 1] != 0.0f;
        mx = fmaxf(mx, lh[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float* redf = (float*)red;
    if ((tid & 63) == 0) redf[tid >> 6] = mx;
    __syncthreads();
    mx = redf[0];
    for (int k = 1; k < CX_WAVES; ++k) mx = fmaxf(mx, redf[k]);
    for (int j = tid; j < n; j += CX_BLOCK) e[j] = exp((double)lh[j] - (double)mx);
    __syncthreads();

    // every event's term (lh_i - mx) - log Q_i, Q_i = R_i - (r_i / d_i) D_i (Efron; Breslow: Q_i = R_i)
    double tsum = 0.0;
    int n_ev = 0, n_grp = 0;
    for (int i = tid; i < n; i += CX_BLOCK) {
        double q_inv = 0.0, f_q = 0.0;
        if (ev[i]) {
            const float ti = tm[i];
            double R = 0.0, D = 0.0;
            int d = 0, r = 0;
            for (int j = 0; j < n; ++j) {          // one address for the whole wave: broadcasts
                const float tj = tm[j];
                const double ej = e[j];
                const bool tie = tj == ti && ev[j];
                R += tj >= ti ? ej : 0.0;
                D += tie ? ej : 0.0;
                d += tie;
                r += tie && j < i;
            }
            const double f = efron ? (double)r / (double)d : 0.0;
            const double Q = R - f * D;
            tsum += ((double)lh[i] - (double)mx) - log(Q);
            q_inv = 1.0 / Q;
            f_q = f / Q;
            ++n_ev;
            n_grp += r == 0;
        }
        iq[i] = q_inv;
        fq[i] = f_q;
    }
    tsum = block_sum<CX_WAVES>(tsum, red);
    n_ev = block_sum<CX_WAVES>(n_ev, (int*)red);
    n_grp = block_sum<CX_WAVES>(n_grp, (int*)red);          // (its barriers also publish iq and fq)
    // Efron: the mean over the distinct event times (with no tie at all these are the events: the reference's first branch); Breslow: over the events
    const double terms = (double)(efron ? n_grp : n_ev);

    for (int k = tid; k < n; k += CX_BLOCK) {
        double g = 0.0;
        if (n_ev > 0) {
            const float tk = tm[k];
            double A = 0.0, Bk = 0.0;
            for (int i = 0; i < n; ++i) {
                const float ti = tm[i];
                A += ti <= tk ? iq[i] : 0.0;
                Bk += ti == tk ? fq[i] : 0.0;
            }
            const double evk = ev[k] ? 1.0 : 0.0;
            g = (e[k] * (A - evk * Bk) - evk) / terms;
        }
        dlh[k] = ob_scaled((float)g, scale, scale_dev);
    }
    if (tid == 0) ob_finish(n_ev > 0 ? (float)((0.0 - tsum) / terms) : 0.0f, n_ev > 0, n, loss, has_grad, acc);
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" int amds_objective_max_items(void) { return CX_MAX_ITEMS; }

extern "C" int amds_objective_step(int kind, const float* logits, const float* targets, const float* weight, int B, int C, float scale, const float* scale_dev,
                                   float* loss, float* dlogits, int32_t* has_grad, double* epoch_acc, void* stream) {
    AMDS_REQUIRE(kind >= AMDS_OBJ_CE && kind <= AMDS_OBJ_COX_BRESLOW, "amds_objective_step: kind=%d is none of CE, L1, COX_EFRON, COX_BRESLOW", kind);
    AMDS_REQUIRE(logits && targets && loss && dlogits && has_grad, "amds_objective_step: null pointer");
    AMDS_REQUIRE(B >= 1 && C >= 1 && (long)B * C < (1L << 31), "amds_objective_step: B=%d C=%d: needs B, C >= 1 and B * C < 2^31", B, C);
    AMDS_REQUIRE(kind == AMDS_OBJ_CE || (C == 1 && !weight), "amds_objective_step: kind=%d takes one output per item and no class weights (C=%d)", kind, C);
    hipStream_t st = (hipStream_t)stream;
    if (kind == AMDS_OBJ_CE) {
        hipLaunchKernelGGL(ce_step_kernel, dim3(1), dim3(OB_BLOCK), 0, st, logits, targets, weight, B, C, scale, scale_dev, loss, dlogits, has_grad, epoch_acc);
        AMDS_LAUNCH_CHECK("ce_step_kernel");
    } else if (kind == AMDS_OBJ_L1) {
        hipLaunchKernelGGL(l1_step_kernel, dim3(1), dim3(OB_BLOCK), 0, st, logits, targets, B, scale, scale_dev, loss, dlogits, has_grad, epoch_acc);
        AMDS_LAUNCH_CHECK("l1_step_kernel");
    } else {
        AMDS_REQUIRE(B <= CX_MAX_ITEMS, "amds_objective_step: B=%d items, a Cox objective takes at most %d", B, CX_MAX_ITEMS);
        AMDS_HIP(lds_opt_in<cox_step_kernel>(cx_lds_bytes(CX_MAX_ITEMS)));
        hipLaunchKernelGGL(cox_step_kernel, dim3(1), dim3(CX_BLOCK), (size_t)cx_lds_bytes(B), st, logits, targets, B, kind == AMDS_OBJ_COX_EFRON ? 1 : 0, scale,
                           scale_dev, loss, dlogits, has_grad, epoch_acc);
        AMDS_LAUNCH_CHECK("cox_step_kernel");
    }
    return AMDS_OK;
}

extern "C" int amds_objective_rows(int kind, const float* logits, const float* targets, const float* weight, long N, int C, float* out, void* stream) {
    AMDS_REQUIRE(kind == AMDS_OBJ_CE || kind == AMDS_OBJ_L1, "amds_objective_rows: kind=%d: per-row values exist for CE and L1 (a one-item Cox batch is constant)",
                 kind);
    AMDS_REQUIRE(logits && targets && out, "amds_objective_rows: null pointer");
    AMDS_REQUIRE(N >= 1 && C >= 1 && N < (1L << 31) && N * C < (1L << 40), "amds_objective_rows: N=%ld C=%d: needs 1 <= N < 2^31, C >= 1, N * C < 2^40", N, C);
    AMDS_REQUIRE(kind == AMDS_OBJ_CE || (C == 1 && !weight), "amds_objective_rows: L1 takes one output per row and no class weights (C=%d)", C);
    hipStream_t st = (hipStream_t)stream;
    if (kind == AMDS_OBJ_CE) {
        hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)((N + OB_WAVES - 1) / OB_WAVES)), dim3(OB_BLOCK), 0, st, logits, targets, weight, N, C, out);
        AMDS_LAUNCH_CHECK("ce_rows_kernel");
    } else {
        hipLaunchKernelGGL(l1_rows_kernel, dim3((unsigned)((N + OB_BLOCK - 1) / OB_BLOCK)), dim3(OB_BLOCK), 0, st, logits, targets, N, out);
        AMDS_LAUNCH_CHECK("l1_rows_kernel");
    }
    return AMDS_OK;
}
