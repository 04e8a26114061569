// mlp.hip -- the slide- / patient-level heads (reference src/stamp/modeling/models/mlp.py:6-62: `MLP` = (Linear -> ReLU -> Dropout) x (num_layers - 1) -> Linear, :24-32;
// `Linear` = the chain with num_layers = 1, :47-62): eval forward, training forward and backward, ONE library call each.
//
// The products are a family of exact-fp32 SKINNY products on v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain), written for rows <= 64 and correct for any row count:
//   forward   y  = x W^T    (mlp_fwd_kernel)    bias, ReLU and the dropout mask in the epilogue
//   backward  dx = dz W     (mlp_dx_kernel)     ReLU' . mask applied where the product is produced: what it stores IS the next dz
//             dW = dz^T x   (mlp_dw_kernel)     db = the column sums of dz from the same launch (one more accumulator against a column of ones)
// A wave owns one 16 x 16 output tile; operands go straight from memory to registers (at these shapes an operand is read once per wave: an LDS round trip is overhead), a lane
// holding four consecutive elements of the contraction index, which feed four INDEPENDENT accumulator chains merged ((0 + 1) + 2) + 3 at the end.  The weights are read in
// place in torch's [out][in] layout and need no alignment beyond 4 bytes (16-byte loads are used where pointer and pitch allow them; the bits are the same).
//
// Decomposition of the forward: K is cut into slices of MLP_KS = 256 columns, a rule of K alone.  With rows <= MLP_SPLIT_ROWS the slices of a tile run as separate
// workgroups (a launch is bound by one workgroup's latency here, so the chain is what to shorten) into fp32 slabs, and mlp_combine_kernel sums the slabs IN SLICE ORDER and
// applies the epilogue; with more rows one wave walks the slices itself, every slice from a zero accumulator, and adds them in the same order -- the same bits.  No
// floating-point atomics anywhere.  A logits row therefore depends on that row's features and the weights only: not on the row count, the row's position or the other rows.
//
// Dropout: the library's counter-based rule with the keying of the module path (stamp_amd.mil._DropoutF32Fn): site = index of the hidden layer, element = row * cols + col of
// the call's batch.  The backward regenerates the masks; the saved block holds the hidden activations a_i = drop(relu(z_i)) only (a_i > 0 <=> kept and past the ReLU).
#include <algorithm>
#include "model_call.h"

namespace amds {
namespace {
constexpr int MLP_MAX_LAYERS = 8;
constexpr int MLP_KS = 256;                 // columns of K per slice of the forward
constexpr int MLP_SPLIT_ROWS = 64;          // up to here the slices of a forward tile are workgroups of their own
constexpr long MLP_MAX_ROWS = 1L << 22;

struct MlpDims { int F, H, C, L; long rows; int in[MLP_MAX_LAYERS], out[MLP_MAX_LAYERS]; };

int mlp_dims(const amds_mlp_cfg* c, long rows, MlpDims* d, const char* who) {
    AMDS_REQUIRE(c, "%s: null config", who);
    AMDS_REQUIRE(c->num_layers >= 1 && c->num_layers <= MLP_MAX_LAYERS, "%s: num_layers=%d (1 <= num_layers <= %d)", who, c->num_layers, MLP_MAX_LAYERS);
    AMDS_REQUIRE(c->dim_input >= 1 && c->dim_output >= 1 && (c->num_layers == 1 || c->dim_hidden >= 1), "%s: bad config dim_input=%d dim_hidden=%d dim_output=%d (every width must be >= 1)",
                 who, c->dim_input, c->dim_hidden, c->dim_output);
    AMDS_REQUIRE(c->dim_input <= 65536 && c->dim_hidden <= 65536 && c->dim_output <= 65536, "%s: bad config dim_input=%d dim_hidden=%d dim_output=%d (every width <= 65536)", who,
                 c->dim_input, c->dim_hidden, c->dim_output);
    AMDS_REQUIRE(rows >= 0 && rows <= MLP_MAX_ROWS, "%s: rows=%ld (0 <= rows <= 2^22)", who, rows);
    d->F = c->dim_input; d->H = c->num_layers > 1 ? c->dim_hidden : 1; d->C = c->dim_output; d->L = c->num_layers; d->rows = rows;
    for (int i = 0; i < d->L; ++i) {
        d->in[i] = i == 0 ? d->F : d->H;
        d->out[i] = i == d->L - 1 ? d->C : d->H;
    }
    return AMDS_OK;
}
inline int mlp_slices(int K) { return cdiv(K, MLP_KS); }
inline bool mlp_split(const MlpDims& d, int layer) { return d.rows <= MLP_SPLIT_ROWS && mlp_slices(d.in[layer]) > 1; }
size_t mlp_slab_bytes(const MlpDims& d) {
    size_t n = 0;
    for (int i = 0; i < d.L; ++i)
        if (mlp_split(d, i)) n = std::max(n, (size_t)mlp_slices(d.in[i]) * d.rows * d.out[i] * 4);
    return n;
}
// eval workspace: two hidden activations (ping-pong) and the slabs
struct MlpEvalWs { size_t act[2], slab, total; };
void mlp_eval_ws(const MlpDims& d, MlpEvalWs* w) {
    Arena ar;
    const size_t a = d.L > 1 ? (size_t)d.rows * d.H * 4 : 0;
    w->act[0] = ar.take(a); w->act[1] = ar.take(a); w->slab = ar.take(mlp_slab_bytes(d));
    w->total = std::max<size_t>(ar.off, 256);
}
// saved state of a training forward: a_i [rows][H] per hidden layer
struct MlpSaved { size_t act[MLP_MAX_LAYERS], total; };
void mlp_saved(const MlpDims& d, MlpSaved* s) {
    Arena ar;
    for (int i = 0; i + 1 < d.L; ++i) s->act[i] = ar.take((size_t)d.rows * d.H * 4);
    s->total = std::max<size_t>(ar.off, 256);
}
// training workspace: the forward's slabs; the backward's two dz buffers (ping-pong)
struct MlpTrainWs { size_t slab, dz[2], total; };
void mlp_train_ws(const MlpDims& d, MlpTrainWs* w) {
    Arena ar;
    const size_t a = d.L > 1 ? (size_t)d.rows * d.H * 4 : 0;
    w->slab = ar.take(mlp_slab_bytes(d)); w->dz[0] = ar.take(a); w->dz[1] = ar.take(a);
    w->total = std::max<size_t>(ar.off, 256);
}

// ---- operand loads -------------------------------------------------------------------------------------------------------------------------------------------------
// four consecutive elements p[0 .. 3] of a row as fp32, element e taken when k + e < K (zero otherwise; ok = false: all zero).  VEC: one 16-byte (fp16: 8-byte) load, the
// caller guarantees alignment and K % 4 == 0.  fp16 -> fp32 is exact.
template <typename T, bool VEC>
__device__ __forceinline__ f32x4 mlp_ld4(const T* __restrict__ p, bool ok, int k, int K) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!ok) return v;
    if constexpr (VEC) {
        if (k < K) {
            if constexpr (std::is_same_v<T, float>) v = *reinterpret_cast<const f32x4*>(p);
            else {
                const f16x4 h = *reinterpret_cast<const f16x4*>(p);
                v = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) v[e] = (float)p[e];
    }
    return v;
}
__device__ __forceinline__ f32x4 mlp_merge(const f32x4 (&acc)[4]) { return ((acc[0] + acc[1]) + acc[2]) + acc[3]; }
// bias, ReLU, dropout: the forward's epilogue (shared by the direct kernel and the slab combine, so both give the same bits)
__device__ __forceinline__ float mlp_epilogue(float v, float b, int relu, long idx, uint64_t seed, uint32_t site, uint32_t thr, float scale) {
    v = v + b;
    if (relu) v = fmaxf(v, 0.f);
    if (thr) v = drop_keep_flat(seed, site, idx, thr) ? v * scale : 0.f;
    return v;
}

// ---- y = x W^T ---------------------------------------------------------------------------------------------------------------------------------------------------------
// X [M][K] (pitch ldx), W [N][K] dense.  Wave t of the launch owns the 16 x 16 tile (t % tiles_m, t / tiles_m): the four waves of a workgroup share a W tile.
// DIRECT: every slice in turn, then the epilogue -> out [M][N].  Otherwise slice blockIdx.y alone -> slab[blockIdx.y][M][N], raw.
template <typename TX, bool VEC, bool DIRECT>
__global__ void __launch_bounds__(256) mlp_fwd_kernel(const TX* __restrict__ X, long ldx, const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ out,
                                                      long M, int N, int K, int nsl, int relu, uint64_t seed, uint32_t site, uint32_t thr, float scale) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const long tiles_m = (M + 15) / 16, tiles_n = (N + 15) / 16;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tiles_m * tiles_n) return;                       // (whole waves leave together; no barrier below)
    const long m0 = (t % tiles_m) * 16;
    const int n0 = (int)(t / tiles_m) * 16;
    const long row = m0 + l15;
    const int n = n0 + l15;
    const bool rok = row < M, nok = n < N;
    const TX* xr = X + (rok ? row : 0) * ldx;
    const float* wr = W + (long)(nok ? n : 0) * K;
    f32x4 total = {0.f, 0.f, 0.f, 0.f};
    const int s0 = DIRECT ? 0 : (int)blockIdx.y, s1 = DIRECT ? nsl : s0 + 1;
    for (int s = s0; s < s1; ++s) {
        f32x4 acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kend = min(K, (s + 1) * MLP_KS);
        for (int k0 = s * MLP_KS; k0 < kend; k0 += 16) {
            const int kb = k0 + 4 * g;
            const f32x4 a = mlp_ld4<TX, VEC>(xr + kb, rok, kb, K);
            const f32x4 b = mlp_ld4<float, VEC>(wr + kb, nok, kb, K);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc[e], 0, 0, 0);
        }
        const f32x4 part = mlp_merge(acc);
        total = s == s0 ? part : total + part;
    }
    if (!nok) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long m = m0 + 4 * g + r;
        if (m >= M) continue;
        const long idx = m * N + n;
        if constexpr (DIRECT) out[idx] = mlp_epilogue(total[r], bias[n], relu, idx, seed, site, thr, scale);
        else out[(long)blockIdx.y * M * N + idx] = total[r];
    }
}
// out[m][n] = epilogue(slab[0] + slab[1] + ... in slice order)
__global__ void __launch_bounds__(256) mlp_combine_kernel(const float* __restrict__ slab, int nsl, const float* __restrict__ bias, float* __restrict__ out, long MN, int N, int relu,
                                                          uint64_t seed, uint32_t site, uint32_t thr, float scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    float v = slab[i];
    for (int s = 1; s < nsl; ++s) v = v + slab[(long)s * MN + i];
    out[i] = mlp_epilogue(v, bias[(int)(i % N)], relu, i, seed, site, thr, scale);
}

// ---- dx = dz W ---------------------------------------------------------------------------------------------------------------------------------------------------------
// dz [M][N] dense, W [N][K] dense -> out [M][K] dense.  MASK: out = [act > 0] . keep . scale . (dz W) with act [M][K] the saved activation of the layer below and the keep
// mask of its dropout site drawn again -- the product's store is the next layer's dz.
template <bool MASK>
__global__ void __launch_bounds__(256) mlp_dx_kernel(const float* __restrict__ dz, const float* __restrict__ W, float* __restrict__ out, const float* __restrict__ act, long M, int N,
                                                     int K, uint64_t seed, uint32_t site, uint32_t thr, float scale) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const long tiles_m = (M + 15) / 16, tiles_k = (K + 15) / 16;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tiles_m * tiles_k) return;
    const long m0 = (t % tiles_m) * 16;
    const int k0 = (int)(t / tiles_m) * 16;
    const long row = m0 + l15;
    const int kc = k0 + l15;
    const bool rok = row < M, kok = kc < K;
    const float* dr = dz + (rok ? row : 0) * N;
    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int nb0 = 0; nb0 < N; nb0 += 16) {
        const int nb = nb0 + 4 * g;
        const f32x4 a = mlp_ld4<float, false>(dr + nb, rok, nb, N);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float b = (kok && nb + e < N) ? W[(long)(nb + e) * K + kc] : 0.f;
            acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b, acc[e], 0, 0, 0);
        }
    }
    const f32x4 v = mlp_merge(acc);
    if (!kok) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long m = m0 + 4 * g + r;
        if (m >= M) continue;
        const long idx = m * K + kc;
        float o = v[r];
        if constexpr (MASK) {
            const bool keep = act[idx] > 0.f && (thr == 0 || drop_keep_flat(seed, site, idx, thr));
            o = keep ? (thr ? o * scale : o) : 0.f;
        }
        out[idx] = o;
    }
}

// ---- dW = dz^T x, db = colsum(dz) -----------------------------------------------------------------------------------------------------------------------------------
// dz [M][N] dense, X [M][K] (pitch ldx) -> dW [N][K] dense; the waves of the first column tile also write db [N].  Rows are summed in order, 16 a step.
template <typename TX>
__global__ void __launch_bounds__(256) mlp_dw_kernel(const float* __restrict__ dz, const TX* __restrict__ X, long ldx, float* __restrict__ dW, float* __restrict__ db, long M, int N,
                                                     int K) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const long tiles_n = (N + 15) / 16, tiles_k = (K + 15) / 16;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tiles_n * tiles_k) return;
    const int k0 = (int)(t % tiles_k) * 16, n0 = (int)(t / tiles_k) * 16;
    const int n = n0 + l15, kc = k0 + l15;
    const bool nok = n < N, kok = kc < K, bias_tile = k0 == 0;          // (wave-uniform)
    f32x4 acc[4], accb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = accb[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long mb0 = 0; mb0 < M; mb0 += 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long m = mb0 + 4 * g + e;
            const bool mok = m < M;
            const float a = (mok && nok) ? dz[m * N + n] : 0.f;
            const float b = (mok && kok) ? (float)X[m * ldx + kc] : 0.f;
            acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[e], 0, 0, 0);
            if (bias_tile) accb[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, accb[e], 0, 0, 0);
        }
    }
    const f32x4 v = mlp_merge(acc), vb = mlp_merge(accb);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nn = n0 + 4 * g + r;
        if (nn >= N) continue;
        if (kok) dW[(long)nn * K + kc] = v[r];
        if (bias_tile && l15 == 0) db[nn] = vb[r];
    }
}

inline bool mlp_al(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline unsigned mlp_grid(long tiles) { return (unsigned)((tiles + 3) / 4); }

// one layer of the forward: out [rows][N] = epilogue(X W^T)
template <typename TX>
int mlp_layer_fwd(const TX* X, long ldx, const float* W, const float* bias, float* out, float* slab, long M, int N, int K, bool split, int relu, uint64_t seed, uint32_t site,
                  const DropParams& dp, hipStream_t st) {
    const int nsl = mlp_slices(K);
    const bool vec = K % 4 == 0 && ldx % 4 == 0 && mlp_al(X, sizeof(TX) * 4) && mlp_al(W, 16);
    const long tiles = ((M + 15) / 16) * (long)cdiv(N, 16);
    const dim3 grid(mlp_grid(tiles), split ? nsl : 1);
    if (split) {
        if (vec) hipLaunchKernelGGL((mlp_fwd_kernel<TX, true, false>), grid, dim3(256), 0, st, X, ldx, W, bias, slab, M, N, K, nsl, relu, seed, site, dp.thr, dp.scale);
        else hipLaunchKernelGGL((mlp_fwd_kernel<TX, false, false>), grid, dim3(256), 0, st, X, ldx, W, bias, slab, M, N, K, nsl, relu, seed, site, dp.thr, dp.scale);
        AMDS_LAUNCH_CHECK("mlp_fwd_kernel");
        const long MN = M * N;
        hipLaunchKernelGGL(mlp_combine_kernel, dim3((unsigned)cdiv(MN, 256)), dim3(256), 0, st, slab, nsl, bias, out, MN, N, relu, seed, site, dp.thr, dp.scale);
        AMDS_LAUNCH_CHECK("mlp_combine_kernel");
        return AMDS_OK;
    }
    if (vec) hipLaunchKernelGGL((mlp_fwd_kernel<TX, true, true>), grid, dim3(256), 0, st, X, ldx, W, bias, out, M, N, K, nsl, relu, seed, site, dp.thr, dp.scale);
    else hipLaunchKernelGGL((mlp_fwd_kernel<TX, false, true>), grid, dim3(256), 0, st, X, ldx, W, bias, out, M, N, K, nsl, relu, seed, site, dp.thr, dp.scale);
    AMDS_LAUNCH_CHECK("mlp_fwd_kernel");
    return AMDS_OK;
}

// The forward's launch sequence, eval (p = 0) and training alike: act[i] receives hidden layer i's activation.
int mlp_forward_body(const MlpDims& d, const amds_mlp_weights& w, const void* x, int dt, long ldx, float p, uint64_t seed, float* const* act, float* slab, float* logits,
                     hipStream_t st) {
    const DropParams dp(p), none(0.f);
    for (int i = 0; i < d.L; ++i) {
        const bool last = i == d.L - 1;
        float* out = last ? logits : act[i];
        const bool split = mlp_split(d, i);
        const DropParams& q = last ? none : dp;
        if (i == 0) {
            if (dt == AMDS_F32) RC(mlp_layer_fwd((const float*)x, ldx, w.w[0], w.b[0], out, slab, d.rows, d.out[0], d.in[0], split, !last, seed, 0, q, st));
            else RC(mlp_layer_fwd((const f16*)x, ldx, w.w[0], w.b[0], out, slab, d.rows, d.out[0], d.in[0], split, !last, seed, 0, q, st));
        } else {
            RC(mlp_layer_fwd((const float*)act[i - 1], (long)d.H, w.w[i], w.b[i], out, slab, d.rows, d.out[i], d.in[i], split, !last, seed, (uint32_t)i, q, st));
        }
    }
    return AMDS_OK;
}

int mlp_check_call(const char* who, const MlpDims& d, const amds_mlp_weights* w, const void* x, int dt, long ldx) {
    AMDS_REQUIRE(w && (x || d.rows == 0), "%s: null pointer", who);
    for (int i = 0; i < d.L; ++i) AMDS_REQUIRE(w->w[i] && w->b[i], "%s: incomplete weights (layer %d)", who, i);
    AMDS_REQUIRE(dt == AMDS_F32 || dt == AMDS_F16, "%s: bad x dtype %d (AMDS_F32 or AMDS_F16)", who, dt);
    AMDS_REQUIRE(ldx >= d.F, "%s: row stride %ld < dim_input %d", who, ldx, d.F);
    AMDS_REQUIRE(mlp_al(x, dt == AMDS_F32 ? 4 : 2), "%s: x is not aligned to its element size", who);
    return AMDS_OK;
}
bool mlp_p_ok(float p) { return p >= 0.f && p < 1.f; }

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" int amds_mlp_max_layers(void) { return MLP_MAX_LAYERS; }

extern "C" size_t amds_mlp_workspace_bytes(const amds_mlp_cfg* cfg_host, long rows) {
    MlpDims d; MlpEvalWs w;
    if (mlp_dims(cfg_host, rows, &d, "amds_mlp_workspace_bytes") != AMDS_OK) return 0;
    mlp_eval_ws(d, &w);
    return w.total;
}
extern "C" size_t amds_mlp_train_saved_bytes(const amds_mlp_cfg* cfg_host, long rows) {
    MlpDims d; MlpSaved s;
    if (mlp_dims(cfg_host, rows, &d, "amds_mlp_train_saved_bytes") != AMDS_OK) return 0;
    mlp_saved(d, &s);
    return s.total;
}
extern "C" size_t amds_mlp_train_workspace_bytes(const amds_mlp_cfg* cfg_host, long rows) {
    MlpDims d; MlpTrainWs w;
    if (mlp_dims(cfg_host, rows, &d, "amds_mlp_train_workspace_bytes") != AMDS_OK) return 0;
    mlp_train_ws(d, &w);
    return w.total;
}

extern "C" int amds_mlp_forward(const amds_mlp_cfg* cfg_host, const amds_mlp_weights* w_host, const void* x, int x_dtype, long ld_x, long rows, float* logits, void* ws,
                                size_t ws_bytes, void* stream) {
    const char* who = "amds_mlp_forward";
    MlpDims d; MlpEvalWs k;
    RC(mlp_dims(cfg_host, rows, &d, who));
    RC(mlp_check_call(who, d, w_host, x, x_dtype, ld_x));
    AMDS_REQUIRE((logits || rows == 0) && ws, "%s: null pointer", who);
    mlp_eval_ws(d, &k);
    if (ws_bytes < k.total) { set_error("%s: workspace %zu < required %zu bytes", who, ws_bytes, k.total); return AMDS_ERR_WORKSPACE; }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    if (rows == 0) return AMDS_OK;
    char* wk = reinterpret_cast<char*>(ws);
    float* act[MLP_MAX_LAYERS];
    for (int i = 0; i < MLP_MAX_LAYERS; ++i) act[i] = reinterpret_cast<float*>(wk + k.act[i & 1]);
    return mlp_forward_body(d, *w_host, x, x_dtype, ld_x, 0.f, 0, act, reinterpret_cast<float*>(wk + k.slab), logits, (hipStream_t)stream);
}

extern "C" int amds_mlp_train_forward(const amds_mlp_cfg* cfg_host, const amds_mlp_weights* w_host, const void* x, int x_dtype, long ld_x, long rows, float p, uint64_t seed,
                                      float* logits, void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "amds_mlp_train_forward";
    MlpDims d; MlpSaved s; MlpTrainWs k;
    RC(mlp_dims(cfg_host, rows, &d, who));
    RC(mlp_check_call(who, d, w_host, x, x_dtype, ld_x));
    AMDS_REQUIRE((logits || rows == 0) && saved && ws, "%s: null pointer", who);
    AMDS_REQUIRE(mlp_p_ok(p), "%s: the dropout probability must lie in [0, 1)", who);
    mlp_saved(d, &s);
    mlp_train_ws(d, &k);
    if (saved_bytes < s.total || ws_bytes < k.total) {
        set_error("%s: saved block %zu / workspace %zu < required %zu / %zu bytes", who, saved_bytes, ws_bytes, s.total, k.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE((((uintptr_t)saved | (uintptr_t)ws) & 255) == 0, "%s: saved block and workspace must be 256-byte aligned", who);
    if (rows == 0) return AMDS_OK;
    char *sv = reinterpret_cast<char*>(saved), *wk = reinterpret_cast<char*>(ws);
    float* act[MLP_MAX_LAYERS] = {};
    for (int i = 0; i + 1 < d.L; ++i) act[i] = reinterpret_cast<float*>(sv + s.act[i]);
    return mlp_forward_body(d, *w_host, x, x_dtype, ld_x, p, seed, act, reinterpret_cast<float*>(wk + k.slab), logits, (hipStream_t)stream);
}

extern "C" int amds_mlp_train_backward(const amds_mlp_cfg* cfg_host, const amds_mlp_weights* w_host, const void* x, int x_dtype, long ld_x, long rows, float p, uint64_t seed,
                                       const float* dlogits, const void* saved, size_t saved_bytes, const amds_mlp_grads* grads_host, int need_dx, float* dx, void* ws,
                                       size_t ws_bytes, void* stream) {
    const char* who = "amds_mlp_train_backward";
    MlpDims d; MlpSaved s; MlpTrainWs k;
    RC(mlp_dims(cfg_host, rows, &d, who));
    RC(mlp_check_call(who, d, w_host, x, x_dtype, ld_x));
    AMDS_REQUIRE((dlogits || rows == 0) && saved && ws, "%s: null pointer", who);
    AMDS_REQUIRE(grads_host || need_dx, "%s: nothing to compute (no gradient buffers, no dx)", who);
    AMDS_REQUIRE(!need_dx || dx || rows == 0, "%s: need_dx without a dx buffer", who);
    AMDS_REQUIRE(mlp_p_ok(p), "%s: the dropout probability must lie in [0, 1)", who);
    const amds_mlp_grads* G = grads_host;
    if (G)
        for (int i = 0; i < d.L; ++i) AMDS_REQUIRE(G->w[i] && G->b[i] && mlp_al(G->w[i], 4) && mlp_al(G->b[i], 4), "%s: incomplete gradient buffers (layer %d)", who, i);
    mlp_saved(d, &s);
    mlp_train_ws(d, &k);
    if (saved_bytes < s.total || ws_bytes < k.total) {
        set_error("%s: saved block %zu / workspace %zu < required %zu / %zu bytes", who, saved_bytes, ws_bytes, s.total, k.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE((((uintptr_t)saved | (uintptr_t)ws) & 255) == 0, "%s: saved block and workspace must be 256-byte aligned", who);
    if (rows == 0) {          // no row: every sum is empty
        hipStream_t st0 = (hipStream_t)stream;
        if (G)
            for (int i = 0; i < d.L; ++i) {
                AMDS_HIP(hipMemsetAsync(G->w[i], 0, (size_t)d.out[i] * d.in[i] * 4, st0));
                AMDS_HIP(hipMemsetAsync(G->b[i], 0, (size_t)d.out[i] * 4, st0));
            }
        return AMDS_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    const amds_mlp_weights& w = *w_host;
    const char* sv = reinterpret_cast<const char*>(saved);
    char* wk = reinterpret_cast<char*>(ws);
    const DropParams dp(p);
    const long M = d.rows;
    const float* dz = dlogits;                                   // [M][out[i]] of the layer being walked
    for (int i = d.L - 1; i >= 0; --i) {
        const int N = d.out[i], K = d.in[i];
        const long tiles_w = (long)cdiv(N, 16) * cdiv(K, 16);
        if (G) {
            if (i > 0) hipLaunchKernelGGL((mlp_dw_kernel<float>), dim3(mlp_grid(tiles_w)), dim3(256), 0, st, dz, reinterpret_cast<const float*>(sv + s.act[i - 1]), (long)d.H, G->w[i],
                                          G->b[i], M, N, K);
            else if (x_dtype == AMDS_F32) hipLaunchKernelGGL((mlp_dw_kernel<float>), dim3(mlp_grid(tiles_w)), dim3(256), 0, st, dz, (const float*)x, ld_x, G->w[0], G->b[0], M, N, K);
            else hipLaunchKernelGGL((mlp_dw_kernel<f16>), dim3(mlp_grid(tiles_w)), dim3(256), 0, st, dz, (const f16*)x, ld_x, G->w[0], G->b[0], M, N, K);
            AMDS_LAUNCH_CHECK("mlp_dw_kernel");
        }
        const long tiles_x = ((M + 15) / 16) * (long)cdiv(K, 16);
        if (i > 0) {          // the next dz: ReLU' . mask of hidden layer i - 1 in the product's store
            float* nxt = reinterpret_cast<float*>(wk + k.dz[i & 1]);
            hipLaunchKernelGGL((mlp_dx_kernel<true>), dim3(mlp_grid(tiles_x)), dim3(256), 0, st, dz, w.w[i], nxt, reinterpret_cast<const float*>(sv + s.act[i - 1]), M, N, K, seed,
                               (uint32_t)(i - 1), dp.thr, dp.scale);
            AMDS_LAUNCH_CHECK("mlp_dx_kernel");
            dz = nxt;
        } else if (need_dx) {
            hipLaunchKernelGGL((mlp_dx_kernel<false>), dim3(mlp_grid(tiles_x)), dim3(256), 0, st, dz, w.w[0], dx, (const float*)nullptr, M, N, K, seed, 0u, 0u, 1.0f);
            AMDS_LAUNCH_CHECK("mlp_dx_kernel");
        }
    }
    return AMDS_OK;
}
