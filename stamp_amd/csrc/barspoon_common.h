// barspoon_common.h -- what the deploy calls (barspoon.hip dense, barspoon_ragged.hip ragged) and the training calls (barspoon_train.hip) of the barspoon
// head share: the two small kernels of the tile / class-token set-up (defined in barspoon.hip) behind their launchers, the exact-fp32 products of the
// class-token side, and -- for the two deploy calls -- the plan of the workspace and the launch sequences of one encoder and one decoder layer.
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

// ---- the deploy forward, dense and ragged (barspoon.hip) ----------------------------------------------------------------------------------------------------
// Offsets of one call's buffers in the caller's workspace: the tile side over `rows` tile rows, the class-token side over n_bags * nt rows, and (ragged) the
// per-call table of the VARLEN kernels behind them.
struct BsPlan : PadDims {
    int Hb, Db, hd_e, hd_d, nt;
    size_t a, x, h, qkv, att, u, kv, tok, th, tqkv, tsc, to, tq, tu, table, total;
};
// the config checks of every barspoon call and the padded dimensions; `who` names the entry in the messages
int bs_dims(const char* who, const amds_barspoon_cfg* c, BsPlan* p);
// the arena over `rows` tile rows of n_bags bags (+ table_bytes at its end); bs_dims first
void bs_arena(const amds_barspoon_cfg* c, int n_bags, size_t rows, size_t table_bytes, BsPlan* p);

struct BsBufs {
    float* x;                                   // residual stream of the tiles, fp32 [rows][Dp]
    void *h, *qkv, *att, *u, *kv;               // 16-bit tile-side operands
    float *tok, *th, *tqkv, *tsc, *to, *tq, *tu;        // class-token side, fp32
};
BsBufs bs_bufs(void* ws, const BsPlan& p);

// How one call reaches its bags.  Dense: n_bags bags of T tiles at a fixed pitch.  Ragged (table != NULL): bag i = the rows the table names (varlen_table_build
// with extra_rows = 0: no class token among the tile rows), T = the longest bag.  The ragged call keeps every bag on the kernels of its own one-bag call:
// 16-bit GEMMs by ragged_cfg over the longest bag (model_call.h), the exact-fp32 products of the class tokens with the bag as the batch dimension.
struct BsCall {
    const char* who;
    int n_bags, T;
    long M;                                     // tile rows of the call
    const void* table;
    int gemm_cfg(int N, int K) const { return table ? ragged_cfg(n_bags, T, N, K) : -1; }
};
// one pre-norm encoder layer over the call's tile rows: x += SA(LN1(x)); x += W2 relu(W1 LN2(x))
int bs_encoder_layer(const BsCall& k, const BsPlan& p, const amds_barspoon_cfg& c, const amds_mil_vit_layer& L, int l, const BsBufs& b, void* stream);
// one pre-norm decoder layer over the class tokens, memory = b.h (the encoder's output, 16-bit): t += SA(LN1(t)); t += MHA(LN2(t), memory); t += W2 relu(W1 LN3(t))
int bs_decoder_layer(const BsCall& k, const BsPlan& p, const amds_barspoon_cfg& c, const amds_barspoon_dec_layer& L, int l, const BsBufs& b, void* stream);
// logits[bag][col ..] = heads.<j>(class token j of the bag), every target; checks the head pointers
int bs_heads(const BsCall& k, const BsPlan& p, const amds_barspoon_cfg& c, const amds_barspoon_weights& w, const float* tok, float* logits, void* stream);

}  // namespace amds
