// model_call.h -- host-only helpers shared by the "one C call" model entries (mil_vit*.hip, barspoon*.hip, ticon.hip, transmil_*.hip, nystrom_train.hip):
// the padded operand layout of the MIL heads, the arena arithmetic of their plans, the status chain, the GEMM kernel rule of the ragged calls.  The launch
// sequences stay with the entries.
#pragma once
#include <algorithm>
#include <cstdint>
#include "launch.h"

namespace amds {

inline int round_up(int n, int m) { return (n + m - 1) / m * m; }
inline long round_up(long n, long m) { return (n + m - 1) / m * m; }
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// offsets of a plan's regions in one caller-owned buffer: every region starts 256-byte aligned, `off` ends as the buffer's size
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off += align256(bytes); return o; }
};

// the first failing status leaves the entry; nothing is launched behind it
#define RC(call)                          \
    do {                                  \
        int rc__ = (call);                \
        if (rc__ != AMDS_OK) return rc__; \
    } while (0)

// The padded operand layout of the MIL heads (amds_mil_vit_layer): feature, model and feed-forward widths rounded up to 256 (the GEMMs' K / N tiles), heads
// to 4 (amds_attention wants H % 4 == 0) of 64 channels each.  Bags are staged as zero-padded 16-bit rows of pitch Fp (stage_rows_dt, elementwise.hip);
// LayerNorm writes the first D columns of its output only, so an entry with Dp != D zeroes that buffer once.
struct PadDims { int Fp, Dp, FFp, Ha, Da; };
inline PadDims pad_dims(int n_feats, int dim, int ff, int heads) {
    PadDims p;
    p.Fp = round_up(n_feats, 256);
    p.Dp = round_up(dim, 256);
    p.FFp = round_up(ff, 256);
    p.Ha = round_up(heads, 4);
    p.Da = 64 * p.Ha;
    return p;
}

// the 12 pointers every user of an encoder layer needs; what only one caller needs (head_scale, bias_scale, inv_running_mean) stays with it
inline bool enc_layer_complete(const amds_mil_vit_layer& L) {
    return L.ln1_w && L.ln1_b && L.in_w && L.in_b && L.out_w && L.out_b && L.ln2_w && L.ln2_b && L.fc1_w && L.fc1_b && L.fc2_w && L.fc2_b;
}
// the transposed 16-bit matrices of a training pack (the backward's dx GEMMs)
inline bool enc_layer_has_transposes(const amds_mil_vit_layer& L) { return L.in_wt && L.out_wt && L.fc1_wt && L.fc2_wt; }

// A GEMM of a training step: amds_gemm_ex's kernel -2 = by shape, with a ragged last row tile as its own small launch (M = bags x 1025 token rows is
// never a multiple of 256).
inline int gemm_train(int dt, const void* A, long lda, const void* W, long ldw, long M, int N, int K, int epi, void* out, long ldo, const float* bias, void* st) {
    return amds_gemm_ex(-2, A, lda, W, ldw, (int)M, N, K, dt, epi, out, ldo, bias, nullptr, nullptr, 0, 0, 0, 1.0f, st);
}

// attention_flash.hip addresses one bag's q | k | v rows under one buffer descriptor (2 GB): the ragged calls check their longest bag against it
#define FA_SPAN_OK(T, H) ((long)(T) * 3 * (H) * 128 < (1L << 31))

// GEMM kernel of a ragged call (mil_vit_ragged.hip, barspoon_ragged.hip) whose bags have at most `rows` rows in this GEMM.  A GEMM row depends on the kernel
// that computes it and the library's default picks the kernel by M, so the call runs on the kernel the longest bag's own call would pick when that is kernel 0
// (then every shorter bag's call picks it too), and by shape otherwise; one bag alone is its own call's shape exactly.
inline int ragged_cfg(int n_bags, long rows, int N, int K) {
    if (n_bags == 1) return -1;
    return default_gemm_cfg((int)std::min(rows, (long)INT32_MAX), N, K) == 0 ? 0 : -1;
}
// the longest bag all of whose GEMMs (shared(T): every shape of a bag of T tiles picks kernel 0; monotone in T) stay on kernel 0, at most `cap`
template <typename F>
inline int ragged_max_shared(F shared, int cap) {
    if (!shared(1)) return cap;                     // a fixed kernel (AMDS_GEMM_CFG): every M gives the same rows
    if (shared(cap)) return cap;
    int lo = 1, hi = cap;                           // shared(lo), !shared(hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (shared(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace amds
