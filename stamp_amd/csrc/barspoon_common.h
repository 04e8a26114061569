// barspoon_common.h -- what the deploy call (barspoon.hip) and the training calls (barspoon_train.hip) of the barspoon head share: the two small kernels
// of the tile / class-token set-up (defined in barspoon.hip) behind their launchers, and the exact-fp32 products of the class-token side.
#pragma once
#include "model_call.h"

namespace amds {

// x[r][c] += PE(pos[r])[c] for c < D (reference barspoon.py:173-186); min(8192, rows * D / 256) blocks
int pos_encoding_add(float* x, int Dp, int D, const float* pos, const float* pe_div, long rows, hipStream_t st);
// dst[i] = src[i % per_bag], i < total: the class tokens of every bag; min(4096, total / 256) blocks
int broadcast_rows(const float* src, float* dst, long per_bag, long total, hipStream_t st);

// exact-fp32 batched product (amds_bgemm_f32's argument order without `diag`)
inline int bg(const float* A, int lda, long sAo, long sAi, const float* B, int ldb, long sBo, long sBi, int tflags, float* Cm, int ldc, long sCo, long sCi,
              int outer, int inner, int M, int N, int K, float alpha, const float* bias, int accumulate, void* st) {
    return bgemm_f32_exact(A, lda, sAo, sAi, B, ldb, sBo, sBi, tflags, Cm, ldc, sCo, sCi, outer, inner, M, N, K, alpha, 0.0f, bias, accumulate, st);
}
// y[M][N] = x[M][K] w[N][K]^T + bias;   dx[M][K] = dy[M][N] w[N][K];   dw[N][K] = dy[M][N]^T x[M][K]
inline int lin(const float* x, const float* w, const float* bias, float* y, long M, int N, int K, void* st) {
    return bg(x, K, 0, 0, w, K, 0, 0, 1, y, N, 0, 0, 1, 1, (int)M, N, K, 1.0f, bias, 0, st);
}
inline int lin_dx(const float* dy, const float* w, float* dx, long M, int N, int K, void* st) {
    return bg(dy, N, 0, 0, w, K, 0, 0, 0, dx, K, 0, 0, 1, 1, (int)M, K, N, 1.0f, nullptr, 0, st);
}
inline int lin_dw(const float* dy, const float* x, float* dw, long M, int N, int K, void* st) {
    return bg(dy, N, 0, 0, x, K, 0, 0, 2, dw, K, 0, 0, 1, 1, N, K, (int)M, 1.0f, nullptr, 0, st);
}

}  // namespace amds
