// common.h -- shared device/host helpers for libamdstamp (gfx950 only).
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <atomic>
#include "../../include/amdstamp.h"

namespace amds {

typedef _Float16 f16;
typedef __bf16 bf16;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- error plumbing (host) -------------------------------------------------------------------
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
#define AMDS_HIP(...)                                                   \
    do {                                                                \
        hipError_t e__ = (__VA_ARGS__);                                 \
        if (e__ != hipSuccess) return amds::hip_fail(e__, #__VA_ARGS__); \
    } while (0)
#define AMDS_REQUIRE(cond, ...)              \
    do {                                     \
        if (!(cond)) {                       \
            amds::set_error(__VA_ARGS__);    \
            return AMDS_ERR_INVALID;         \
        }                                    \
    } while (0)
#define AMDS_LAUNCH_CHECK(name)                                   \
    do {                                                          \
        hipError_t e__ = hipGetLastError();                       \
        if (e__ != hipSuccess) return amds::hip_fail(e__, name);  \
    } while (0)

// ---- per-dtype traits ------------------------------------------------------------------------
template <typename T> struct Act;
template <> struct Act<f16> {
    typedef f16x8 vec8;
    typedef f16x4 vec4;
    static __device__ __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma16(vec8 a, vec8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    // accumulator pinned to the AGPR half of the register file ("a" constraint); accumulate chains need no wait states
    static __device__ __forceinline__ void mfma32_agpr(vec8 a, vec8 b, f32x16& c) {
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
    static __device__ __forceinline__ void mfma16_agpr(vec8 a, vec8 b, f32x4& c) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
    static __device__ __forceinline__ f16 from_f32(float x) { return (f16)x; }
    // two v_cvt_pk_f16_f32 (element-wise conversion loops compile to v_cvt_f16_f32 + v_pack / v_alignbit: 2.5x the instructions)
    static __device__ __forceinline__ vec4 from_f32x4(f32x4 v) { return __builtin_convertvector(v, vec4); }
    static __device__ __forceinline__ float to_f32(f16 x) { return (float)x; }
};
template <> struct Act<bf16> {
    typedef bf16x8 vec8;
    typedef bf16x4 vec4;
    static __device__ __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma16(vec8 a, vec8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void mfma32_agpr(vec8 a, vec8 b, f32x16& c) {
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
    static __device__ __forceinline__ void mfma16_agpr(vec8 a, vec8 b, f32x4& c) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
    static __device__ __forceinline__ bf16 from_f32(float x) { return (bf16)x; }
    static __device__ __forceinline__ vec4 from_f32x4(f32x4 v) { return __builtin_convertvector(v, vec4); }
    static __device__ __forceinline__ float to_f32(bf16 x) { return (float)x; }
};

// v_fma_mix_f32 with 16-bit sources taken straight from the halves of packed registers (the compiler folds fma(fpext a, 1, fpext b) to two conversions + an add):
//   mix_add_hh<HA, HB>(a, b) = float(half HA of a) + float(half HB of b);   mix_sub_fh<HC>(v, c) = v - float(half HC of c).   fp16 only (no bf16 form).
template <int HA, int HB>
__device__ __forceinline__ float mix_add_hh(unsigned a, unsigned b) {
    float d;
    if constexpr (HA == 0 && HB == 0) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b));
    else if constexpr (HA == 1 && HB == 1) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b));
    else if constexpr (HA == 0 && HB == 1) asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b));
    else asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
template <int HC>
__device__ __forceinline__ float mix_sub_fh(float v, unsigned c) {
    float d;
    if constexpr (HC == 0) asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(c), "v"(v));
    else asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(c), "v"(v));
    return d;
}

// exact-erf GELU (nn.GELU default), evaluated in fp32
__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
// GELU for fp16/bf16 OUTPUTS: erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, i.e. below half an ulp of the
// 16-bit result everywhere the result is not itself ~1e-7) -- 1 rcp + 1 exp + 7 fma instead of ocml erff's ~45
// instructions, which cost 28 % of the fc1 GEMM when evaluated on all 257 x 4096 outputs per tile and layer.
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __expf(-z * z);
    const float erf_abs = fmaf(-p * t, e, 1.0f);          // erf(|x|/sqrt2)
    const float h = 0.5f * x;
    return fmaf(copysignf(erf_abs, x), h, h);             // 0.5 x (1 + erf(x/sqrt2))
}
// erf-GELU without transcendentals, for 16-bit outputs on VALU-bound epilogues:  gelu(x) = x (1/2 + xc R(xc^2)),  xc = clamp(x, +-3 sqrt2),
// R of degree 8.  Derivation (tools/gelu_poly_fit.py): erf(z) ~ zc P(u) on |z| <= 3 with u = 2 zc^2 / 9 - 1, P near-minimax (Lawson-weighted
// least squares) under the CONSTRAINT 3 P(1) = 1 -- the approximation saturates at +-1, so beyond the clamp gelu is 0 or x to 2e-8 |x| (an
// unconstrained fit leaves 0.5 |x| (1 - erf(zmax)) there, which grows with |x|: massive activations); then re-expanded in t = xc^2 with the 1/sqrt2
// of z = x / sqrt2 and the 1/2 folded in, and R[0], R[1] moved by -6 / +1 ulp so that the fp32 FMA chain lands on xc R(18) = -+1/2 at the clamp.
// |gelu error| <= 1.4e-5 |x| <= 5.6e-5: 6 % of half an fp16 ulp of the result where it is largest.  Round 3 (end): degree 11 in u on |z| <= 3.25
// (2.2e-6 |x|) was 100x finer than a 16-bit output can hold, and this epilogue's VALU work is un-overlapped (one wave per SIMD): per pair of
// outputs 2 v_med3 + 1 v_pk_mul (t) + 8 v_pk_fma (Horner) + 1 v_pk_fma + 1 v_pk_mul, against 2 + 2 + 2 + 11 + 3 before; fc1's launch 2 353 -> 2 230 us.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// Round 5 (verdict r04 item 1 (f)): degree 8 -> 7.  |gelu error| <= 1.9e-4 (4.6e-5 |x|) = a tenth of half an fp16 ulp of the result where it is largest (degree 8: 5.6e-5,
// 3 %); stored features move by 0.3 % of their own error (ViT-L/16 4.879e-4 -> 4.896e-4 vs the fp32 oracle); one packed fma fewer per pair of outputs: headline +0.6-0.75 %
// (profiles/r05_gelu_degree_ab.txt, alternating over two boxes).  Degree 6 (7.8e-4, 40 % of half an ulp, features +6 %) is no faster than 7 and stays a build switch:
// make GELU_DEG=8 / 6; coefficients: tools/gelu_poly_fit.py 3.0 <degree>.
#ifndef AMDS_GELU_DEG
#define AMDS_GELU_DEG 7
#endif
constexpr int GELU_DEG = AMDS_GELU_DEG;
constexpr float GELU_XMAX = 4.242640495300293f;
#if AMDS_GELU_DEG == 8
constexpr float GELU_R[GELU_DEG + 1] = {3.989038765e-01f, -6.635002047e-02f, 9.821003303e-03f, -1.110561891e-03f, 9.383271390e-05f,
                                        -5.674323347e-06f, 2.286626994e-07f, -5.434610983e-09f, 5.714419563e-11f};
#elif AMDS_GELU_DEG == 7
constexpr float GELU_R[GELU_DEG + 1] = {3.987607062e-01f, -6.595215201e-02f, 9.502778761e-03f, -9.971429827e-04f, 7.251269562e-05f,
                                        -3.410153795e-06f, 9.214582519e-08f, -1.077705258e-09f};
#elif AMDS_GELU_DEG == 6
constexpr float GELU_R[GELU_DEG + 1] = {3.982334733e-01f, -6.480728090e-02f, 8.793668821e-03f, -8.053584024e-04f, 4.606616494e-05f,
                                        -1.466691856e-06f, 1.968182417e-08f};
#else
#error "AMDS_GELU_DEG must be 6, 7 or 8"
#endif
// the same polynomial on NC independent 2-vectors, Horner steps interleaved across them: one wave per SIMD (4-wave GEMM) has
// nobody to hide the dependent v_pk_fma latency behind, so a single chain runs at a fraction of the VALU rate
template <int NC>
__device__ __forceinline__ void gelu_erf_poly2_n(f32x2 (&x)[NC]) {
    f32x2 xc[NC], t[NC], p[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        // v_med3_f32 per element; elementwise min(max()) also canonicalises its input (one v_max_f32 x, x more per element)
        xc[k] = f32x2{__builtin_amdgcn_fmed3f(x[k][0], -GELU_XMAX, GELU_XMAX), __builtin_amdgcn_fmed3f(x[k][1], -GELU_XMAX, GELU_XMAX)};
        t[k] = xc[k] * xc[k];
        p[k] = f32x2{GELU_R[GELU_DEG], GELU_R[GELU_DEG]};
    }
#pragma unroll
    for (int i = GELU_DEG - 1; i >= 0; --i)
#pragma unroll
        for (int k = 0; k < NC; ++k) p[k] = p[k] * t[k] + GELU_R[i];
#pragma unroll
    for (int k = 0; k < NC; ++k) x[k] = x[k] * (xc[k] * p[k] + 0.5f);
}
__device__ __forceinline__ f32x2 gelu_erf_poly2(f32x2 x) {
    f32x2 q[1] = {x};
    gelu_erf_poly2_n<1>(q);
    return q[0];
}
// x * sigmoid(x) for 16-bit outputs: v_rcp_f32 (1 ulp) instead of the IEEE division `x / (1 + e)` expands to (v_div_scale x 2, v_rcp, 5 fma,
// v_div_fmas, v_div_fixup: 11 of the 17 VALU instructions per output of the SWIGLU epilogue, which is un-overlapped like the GELU one)
__device__ __forceinline__ float silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// silu(g) * v on two outputs at once: the multiply in front of v_exp_f32, the + 1 behind it and both products as packed instructions (2 + 2 transcendental
// instructions per pair instead of 4 + 2 + 2; the SWIGLU epilogue is un-overlapped vector work like the GELU one).  exp(-g) = exp2(g * (-log2 e)).
__device__ __forceinline__ f32x2 silu_mul2(f32x2 g, f32x2 v) {
    const f32x2 a = g * f32x2{-1.44269504088896340736f, -1.44269504088896340736f};
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])} + f32x2{1.0f, 1.0f};
    return g * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])} * v;
}

// Sum over the 32 lanes that share lane >> 5; every lane gets the total.  Every step is an XOR butterfly (lane ^ 1, ^ 2, ^ 7, ^ 15, ^ 16:
// quad_perm, row_half_mirror, row_mirror, ds_swizzle -- five independent masks), so the association tree is a fixed partition of the
// lanes into cosets and the result does not change when the values are permuted by lane -> lane ^ c.  The GEMM epilogue needs that:
// it holds a row's columns in lane l31 ^ (row & 31), and a row's statistics must not depend on where the row sits in its tile.
__device__ __forceinline__ float half_wave_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));                      // lane ^ 16
    return v;
}
// Eight (sum, sum of squares) pairs per lane -> for each of the 8 rows the total over the 32 lanes sharing lane >> 5, by recursive halving:
// a lane gives away half of its rows at each of the first three steps (lane ^ 16: v_permlane16_swap; ^ 15, ^ 7: DPP mirrors) and ends with ONE row, which the last two
// steps (lane ^ 1, ^ 2) complete: 8 + 4 + 2 + 2 exchanges instead of 8 x 5.  Returns the pair of row  4 * bit4 + 2 * bit3 + bit2  of the
// lane index (so lanes with (lane & 3) == 0 hold each row once).  Same coset tree as half_wave_sum: invariant under lane -> lane ^ c.
__device__ __forceinline__ f32x2 half_wave_sum8(const f32x2 (&v)[8], int lane) {
    auto dpp = [](float x, auto ctrl_c) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl_c)::value, 0xF, 0xF, true));
    };
    typedef std::integral_constant<int, 0x140> MIRROR;
    typedef std::integral_constant<int, 0x141> HALF_MIRROR;
    typedef std::integral_constant<int, 0xB1> XOR1;
    typedef std::integral_constant<int, 0x4E> XOR2;
    const bool b3 = lane & 8, b2 = lane & 4;
    f32x2 a[4], b[2], c;
    // lane ^ 16 by v_permlane16_swap (gfx950): it swaps the odd 16-lane rows of its first operand with the even rows of its second, so
    // with (rows j, rows 4 + j) as operands every lane ends up with its own value of the row it keeps and its partner's value of the
    // same row -- no selects, no LDS pipe.
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            // inline asm: with this toolchain the __builtin_amdgcn_permlane16_swap result pair reads element 0 twice (r[0] + r[1] compiles
            // to v + v: tools/ubench/hws8_check.hip); the nops cover the VALU-write -> permlane-read and permlane-write -> VALU-read distances
            // the compiler's hazard recogniser cannot see inside asm
            float lo = v[j][e], hi4 = v[4 + j][e];
            asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo), "+v"(hi4));
            a[j][e] = lo + hi4;
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const f32x2 keep = b3 ? a[2 + j] : a[j], send = b3 ? a[j] : a[2 + j];
        b[j] = keep + f32x2{dpp(send[0], MIRROR{}), dpp(send[1], MIRROR{})};
    }
    {
        const f32x2 keep = b2 ? b[1] : b[0], send = b2 ? b[0] : b[1];
        c = keep + f32x2{dpp(send[0], HALF_MIRROR{}), dpp(send[1], HALF_MIRROR{})};
    }
    c += f32x2{dpp(c[0], XOR1{}), dpp(c[1], XOR1{})};
    c += f32x2{dpp(c[0], XOR2{}), dpp(c[1], XOR2{})};
    return c;
}

// The same recursive halving inside one DPP row of 16 lanes (lane ^ 15, ^ 7, ^ 1 give rows away, ^ 2 completes; four independent masks, so again a fixed
// coset tree: invariant under lane -> lane ^ c, c < 16).  Returns the pair of row  4 * bit3 + 2 * bit2 + bit0  of the lane index: the lanes with
// (lane & 2) == 0 hold each of the 8 rows once per 16 lanes.  No cross-row instruction, no nops.
__device__ __forceinline__ f32x2 row16_sum8(const f32x2 (&v)[8], int lane) {
    auto dpp = [](float x, auto ctrl_c) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl_c)::value, 0xF, 0xF, true));
    };
    typedef std::integral_constant<int, 0x140> MIRROR;
    typedef std::integral_constant<int, 0x141> HALF_MIRROR;
    typedef std::integral_constant<int, 0xB1> XOR1;
    typedef std::integral_constant<int, 0x4E> XOR2;
    const bool b3 = lane & 8, b2 = lane & 4, b0 = lane & 1;
    f32x2 a[4], b[2], c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x2 keep = b3 ? v[4 + j] : v[j], send = b3 ? v[j] : v[4 + j];
        a[j] = keep + f32x2{dpp(send[0], MIRROR{}), dpp(send[1], MIRROR{})};
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const f32x2 keep = b2 ? a[2 + j] : a[j], send = b2 ? a[j] : a[2 + j];
        b[j] = keep + f32x2{dpp(send[0], HALF_MIRROR{}), dpp(send[1], HALF_MIRROR{})};
    }
    {
        const f32x2 keep = b0 ? b[1] : b[0], send = b0 ? b[0] : b[1];
        c = keep + f32x2{dpp(send[0], XOR1{}), dpp(send[1], XOR1{})};
    }
    c += f32x2{dpp(c[0], XOR2{}), dpp(c[1], XOR2{})};
    return c;
}

// maximum over the 32 lanes that share lane >> 5 (the butterfly of half_wave_sum: four DPP steps and one ds_swizzle, no ds_bpermute round trips)
__device__ __forceinline__ float half_wave_max(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- dropout bits (training) --------------------------------------------------------------------
// Counter-based, so forward and backward regenerate the SAME mask from (seed, stream, element index) and nothing T x T or
// M x FF is stored.  One 32-bit hash (murmur3 finaliser over a per-row key) serves the element PAIR (2j, 2j+1) of a row, 16
// bits each:  keep  <=>  bits16 >= thr16,  thr16 = round(p * 65536)  ->  P(drop) = thr16 / 65536 (p = 0.5, 0.25 exact),
// kept values are scaled by 65536 / (65536 - thr16).  `stream` separates the dropout sites of one training step.
// Token distances of the ALiBi term: v_sqrt_f32 (1 ulp) instead of the correctly rounded sqrtf, which the compiler expands into ~18 VALU instructions around the
// same v_sqrt_f32 -- 60 % of the ALiBi forward's VALU stream, in kernels that are VALU-issue-bound; the distance is rounded to 16 bits as an MFMA operand right after.
__device__ __forceinline__ float dist_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __host__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __host__ __forceinline__ uint32_t drop_rowkey(uint64_t seed, uint32_t stream, uint64_t row) {
    const uint32_t a = fmix32((uint32_t)seed ^ (uint32_t)row ^ (stream * 0x9E3779B1u));
    return fmix32(a + (uint32_t)(seed >> 32) + (uint32_t)(row >> 32) * 0x7FEB352Du);
}
// 32 mask bits of a (row, element pair): ONE multiply between two 16-bit xor-shifts of (row key ^ pair x golden ratio).  The row key carries the mixing (two murmur
// finalisers of seed / stream / row); the per-pair step was a third murmur finaliser until round 6 -- two quarter-rate v_mul_lo_u32 + five VALU per pair, a third of
// the attention forward's vector time.  This form: one multiply + two SDWA xors.  Checked on 16.7 M mask bits per setting (tools/dropout_hash_stats.py): keep rate,
// covariances between neighbouring keys / pair halves / rows / diagonals and the spread of row and column means all within 3 sigma of a fair Bernoulli source.
__device__ __host__ __forceinline__ uint32_t drop_mix(uint32_t h) {
    h ^= h >> 16; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __host__ __forceinline__ uint32_t drop_pair_bits(uint32_t rowkey, uint32_t pair) { return drop_mix(rowkey ^ (pair * 0x9E3779B1u)); }
__device__ __host__ __forceinline__ bool drop_keep(uint32_t pair_bits, int odd, uint32_t thr16) {
    return ((pair_bits >> (odd ? 16 : 0)) & 0xFFFFu) >= thr16;
}
// elementwise sites: the flat tensor is cut into rows of 65536 elements
__device__ __forceinline__ bool drop_keep_flat(uint64_t seed, uint32_t stream, long idx, uint32_t thr16) {
    const uint32_t key = drop_rowkey(seed, stream, (uint64_t)(idx >> 16));
    return drop_keep(drop_pair_bits(key, (uint32_t)(idx & 0xFFFF) >> 1), (int)(idx & 1), thr16);
}
static inline uint32_t drop_thr16(float p) { const long t = lroundf(p * 65536.0f); return (uint32_t)(t < 0 ? 0 : (t > 65535 ? 65535 : t)); }
static inline float drop_scale(uint32_t thr16) { return 65536.0f / (float)(65536u - thr16); }

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
// async 16-byte global -> LDS copy; LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)lds_wave_base, 16, 0, 0);
}

// the same copy in buffer form (buffer_load_dwordx4 v, s[rsrc], soffset offen lds): byte offset = voffset (per lane) + soffset
// (wave-uniform); out-of-range offsets read as 0.  Wrapped in a __device__ function: called directly inside some kernel
// templates the builtin makes the HOST-side instantiation silently invalid (no stub emitted, undefined symbol at load time).
__device__ __forceinline__ void bufl16(__amdgpu_buffer_rsrc_t rsrc, void* lds_wave_base, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)lds_wave_base, 16, voffset, soffset, 0, 0);
}

// ---- live per-kernel timing (HIP events on the launch stream; off unless amds_profile_enable(ctx, 1)) ----
}  // namespace amds
struct amds_ctx;
namespace amds {
enum ProfKind { PROF_GEMM = 0, PROF_ATTN = 1, PROF_LN = 2, PROF_OTHER = 3, PROF_GEMM_F32 = 4, PROF_GEMM_FP8 = 5, PROF_NKINDS = 6 };
struct ProfRec { hipEvent_t a, b; int kind; double work; bool closed; };
extern std::atomic<int> g_prof_any;            // number of contexts whose profiler is on (fast path: one relaxed load per launch)
int prof_begin(int kind, double work, hipStream_t st, amds_ctx** ctx_out);
void prof_end(amds_ctx* ctx, int slot, hipStream_t st);
int ctx_side_stream(amds_ctx* c, hipStream_t* side, hipEvent_t* ev_in, hipEvent_t* ev_out);
amds_ctx* ctx_of_current_device();
int ctx_matmul_precision();      // of the current device's context (AMDS_MATMUL_HIGHEST without one)
int ctx_mil_cls_tail();          // of the current device's context (the AMDS_MIL_CLS_TAIL environment default without one)
int device_cu_count();           // multiprocessor count of the current device, cached per device
constexpr int MAX_DEV = 64;      // devices per process that per-device state (contexts, CU counts, launch.h's LDS opt-ins) has room for
struct ProfScope {
    hipStream_t st; amds_ctx* ctx = nullptr; int slot = -1;
    ProfScope(int kind, double work, hipStream_t s) : st(s) { if (g_prof_any.load(std::memory_order_relaxed) > 0) slot = prof_begin(kind, work, s, &ctx); }
    ~ProfScope() { if (slot >= 0) prof_end(ctx, slot, st); }
};

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// dtype-taking forms of C entries whose ABI fixes bf16 (the MIL `vit` training step at float32_matmul_precision "high" runs them on fp16 tensors)
int gelu_dropout_fwd_rows_dt(const void* z, long ldz, void* u, long ldu, long rows, int cols, long row_mul, int dtype, float p, uint64_t seed, uint32_t stream_id, void* stream);
int gelu_dropout_bwd_rows_dt(const void* z, long ldz, const void* du, long ldu, void* dz, long lddz, long rows, int cols, long row_mul, int dtype, float p, uint64_t seed,
                             uint32_t stream_id, void* stream);
int dropout_cast_bwd_rows_dt(const float* dx, long ldx, void* dy, long ldy, long rows, int cols, long row_mul, int dtype, float p, uint64_t seed, uint32_t stream_id, void* stream);
int layernorm_bwd_partials_dt(const float* dy, long dy_stride, const float* x, long x_stride, const float* mean, const float* rstd, const float* gamma, float* dx,
                              long dx_stride, int add_skip, float* dgamma_part, float* dbeta_part, int rows, int cols, void* dx16, long dx16_stride, int dx16_dtype, float p,
                              uint64_t seed, uint32_t stream_id, void* stream);
int attention_alibi_fwd_train_dt(const void* qkv, const float* coords, const float* inv_running_mean, const float* bias_scale, void* out, void* u, void* osm, float* lse,
                                 int B, int T, int H, int dtype, void* stream);
int attention_alibi_bwd_dt(const void* qkv, const void* osm, const void* u, const void* dout, const float* lse, const float* coords, const float* bias_scale,
                           const float* dist_scale, float* dq_sum_ws, float* dbs_part, void* dqkv, int B, int T, int H, int dtype, void* stream);
int nystrom_attn_fwd_ex(const amds_transmil_layer* w_host, int dim, const float* y, float* x_res, int n_bags, int n_tokens, float p_drop, uint64_t seed, uint32_t stream_id,
                        void* saved, size_t saved_bytes, int cls_only, void* stream);
int nystrom_attn_bwd_ex(const amds_transmil_layer* w_host, int dim, const float* dx, float* dy, const amds_nystrom_grads* grads_host, int n_bags, int n_tokens, float p_drop,
                        uint64_t seed, uint32_t stream_id, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, int cls_only, void* stream);
int pinv_absmax_accumulate(const float* x, int nmat, int n, unsigned* mx2, int group, void* stream);          // transmil.hip: the halves of amds_pinv_init
int pinv_init_preset(const float* x, float* z, int nmat, int n, const unsigned* mx2, int group, void* stream);
unsigned bgemm_f32_row_class(long M);          // transmil.hip: what amds_bgemm_f32's choice of kernel takes from the row count
int layernorm_bwd_cast_dt(const float* dy, long dy_stride, const float* x, long x_stride, const float* mean, const float* rstd, const float* gamma, float* dx, long dx_stride,
                          int add_skip, float* dgamma, float* dbeta, int accumulate_params, int rows, int cols, void* ws, size_t ws_bytes, void* dx16, long dx16_stride,
                          int dx16_dtype, float p, uint64_t seed, uint32_t stream_id, void* stream);
// the MIL heads' bag staging (elementwise.hip): [rows][F] fp32 / f16 / bf16 of pitch ld_src -> zero-padded f16 / bf16 rows of pitch Fp; min(8192, total / 256) blocks
int stage_rows_dt(const void* src, int src_dtype, long ld_src, void* dst, int dst_dtype, int Fp, long rows, int F, void* stream);

// amds_bgemm_f32 on the exact-fp32 MFMA whatever amds_set_matmul_precision says (transmil.hip): for the paths that promise exact fp32
// ragged (variable-length) bags without padding, attention_flash.hip: a table built once per call from device offsets [n_bags + 1] (tile counts; bag i's
// token rows, class token first, start at offsets[i] + i; extra_rows = 0: no class token, bag i's rows are offsets[i] .. offsets[i+1] - 1), lengths clamped
// to [0, max_tiles] and rows to the buffers on the device
long varlen_work_items(int n_bags, long total_tiles);
size_t varlen_table_bytes(int n_bags, long total_tiles);
int varlen_table_build(const int* offsets, int n_bags, long total_tiles, int max_tiles, int extra_rows, void* table, hipStream_t st);
const int2* varlen_table_bags(const void* table);      // int2 {first token row, token count} per bag
int attention_varlen_launch(const void* qkv, const float* coords, const float* head_scale, void* out, const void* table, int n_bags, long total_tiles,
                            int H, int dtype, hipStream_t st);           // coords != NULL: ALiBi (out bf16)
int attention_row_varlen_launch(const void* q, long ldq, const void* qkv, void* out, long ldo, const void* table, int n_bags, int max_tiles, int H,
                                int dtype, hipStream_t st);
int default_gemm_cfg(int M, int N, int K);
int bgemm_f32_exact(const float* A, int lda, long sAo, long sAi, const float* B, int ldb, long sBo, long sBi, int transb, float* Cm, int ldc, long sCo, long sCi,
                    int outer, int inner, int M, int N, int K, float alpha, float diag, const float* bias, int accumulate, void* stream);
}  // namespace amds
