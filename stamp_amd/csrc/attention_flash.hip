// attention_flash.hip -- multi-head self-attention for ANY sequence length (head_dim 64): the MIL heads attend over
// a whole bag (T+1 = 1025 tokens in training, up to tens of thousands at deploy time, where the reference simply
// materialises the T x T matrix -- src/stamp/modeling/models/__init__.py:286-313 disables the mask "to reduce
// memory").  Reference op: nn.MultiheadAttention / F.scaled_dot_product_attention at
// src/stamp/modeling/models/vision_tranformer.py:191, 217-227 (mask = None path).
//
// One workgroup = 128 queries (4 waves x 32) of one (bag, head); K / V stream through LDS in tiles of 64 keys,
// double buffered by LDS-DMA (row-major images; V^T fragments by transpose reads; see attention_vit.hip for the layout
// rules: S^T = K Q^T keeps a query's scores in one lane, the key order inside 16-key groups is such that P is
// already the MFMA B operand).  Scores never leave registers: N^2 is never materialised, K/V are re-read once per
// 128-query block (L2-resident: 2 x T x 128 B per head).
#include <optional>
#include "launch.h"

namespace amds {

constexpr int FA_KT = 64;                       // keys per tile
constexpr int FA_K_BYTES = FA_KT * 128;         // a row-major image of 64 keys (K, and V alike): 8 KB
constexpr int FA_C_BYTES = FA_KT * 8;            // key coordinates (float2) of a tile, ALiBi variant only

// ALIBI: the reference's MultiHeadALiBi (src/stamp/modeling/models/vision_tranformer.py:42-74): the distance bias is
// SUBTRACTED FROM THE PROBABILITIES (after the softmax):  out = softmax(q k^T/8) v  -  s_h * cdist(c_q, c_k) v,
// s_h = bias_scale_h / running_mean_h.  The second product is accumulated by a third MFMA chain on the same V^T
// fragments; distances are evaluated in fp32 from the token coordinates in registers (no T x T tensor).
// TO: output element type.  The ALiBi variant always writes bf16: its second term sums |V| over ALL keys with weights
// of order 1-10 (no softmax normalisation), which overflows fp16 (65504) on long bags; bf16 has the fp32 range.
//
// MASK: the reference's `mask != None` path (vision_tranformer.py:355-381), restated literally.  pad[b][t] (u8, class token
// included at t = 0 and never padded) marks padded tiles; blocked(q, k) = (pad[q] & pad[k]) | (q > 0 & k == 0): padded queries
// do not see padded keys, tiles never see the class token (:363-367) -- an UNpadded query still attends to every key, padded or
// not, exactly as the reference's outer-product mask does.  nn.MultiheadAttention branch: blocked scores are -inf before the
// softmax, and because the reference hands MultiheadAttention `attn_mask.repeat(heads, 1, 1)` (:224), (bag b, head h) is masked
// with the pad row of bag (b*H + h) % B.  ALiBi branch (:62-70): the softmax runs over ALL keys, blocked products are zeroed
// afterwards, and the distance term is dropped on the class-token row and column (alibi_mask, :370-372); mask row = bag b.
// DROP (plain attention, training): nn.MultiheadAttention's dropout on the attention probabilities: out = drop(P) v with the
// normaliser and the saved log-sum-exp those of the undropped P; mask bits from (seed, stream, (b,h,q), k) -- common.h drop_*.
// Data path (round 6; the first form -- global -> registers -> LDS with a transposing store pass for V, 42 KB and 146-161 registers -- is kept as text in
// tools/ubench/attic/attention_first_forms/, A/B in profiles/r06_attn_bwd_ab.txt: same bits, -7.5 %): K and V tiles by buffer-form LDS-DMA (no staging registers),
// the V^T fragments of the P V product by ds_read_b64_tr_b16 transpose reads of the row-major V image, two 16 KB stages, a raw s_barrier per tile; 121-128 registers:
// four workgroups per CU (ALiBi: 211, two).  16-byte chunk c of key row k sits at chunk c ^ attn_swz(k): row reads and transpose reads are both conflict-free.
#define FA_TR8(out, a00, a01, a10, a11, imm)                                                                                              \
    asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%12\n\tds_read_b64_tr_b16 %1, %10 offset:%12\n\t"                                  \
                 "ds_read_b64_tr_b16 %2, %9 offset:%12\n\tds_read_b64_tr_b16 %3, %11 offset:%12\n\t"                                   \
                 "ds_read_b64_tr_b16 %4, %8 offset:%13\n\tds_read_b64_tr_b16 %5, %10 offset:%13\n\t"                                   \
                 "ds_read_b64_tr_b16 %6, %9 offset:%13\n\tds_read_b64_tr_b16 %7, %11 offset:%13\n\ts_waitcnt lgkmcnt(0)"               \
                 : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3]), "=&v"(out[4]), "=&v"(out[5]), "=&v"(out[6]), "=&v"(out[7])  \
                 : "v"(a00), "v"(a01), "v"(a10), "v"(a11), "n"(imm), "n"((imm) + 2048)                                                  \
                 : "memory")
// the LDS-DMA addresses one bag's q | k | v rows through a buffer descriptor: 32-bit byte offsets
#define FA_SPAN_OK(T, H) ((long)(T) * 3 * (H) * 128 < (1L << 31))
__device__ __forceinline__ int attn_swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

// VARLEN (inference, plain or ALiBi; no MASK / DROP / lse): ragged bags packed without padding (amds_attention_varlen).  The grid is a flattened list of
// (bag, 128-query block) work items built once per call from the bag offsets (varlen_plan_kernel): blockIdx.x indexes `vwork`, item = {first token row of
// the bag, its token count Tn, q block, -}; Tn = 0 marks the slack at the end of the list (the host sizes the grid by a bound, not by the device-side sum).
// Everything else is the fixed-pitch kernel: the same arithmetic per (bag, head, query) whatever the bag's neighbours.
//
// DBIAS (inference; no ALIBI / MASK / DROP / VARLEN): the distance bias INSIDE the softmax, TICON's `Attention` (src/stamp/preprocessing/extractor/ticon.py:183-215,
// :152-154):  out = softmax(q k^T / 8 - slope_h * |c_q - c_k|) v,  slope_h = head_scale[h] (get_slopes :102-119).  Key coordinates are staged like the ALiBi
// variant's, the query's stay in registers, distances are fp32 and the logit is formed in the log2 domain before the running maximum (the bias moves the maximum).
// Keys past the sequence get -inf AFTER the bias: their zero V rows would not make a finite weight harmless to the normaliser.
template <typename T, bool ALIBI, typename TO = T, bool MASK = false, bool DROP = false, bool VARLEN = false, bool DBIAS = false>
__global__ void __launch_bounds__(256, 2) attn_flash_kernel(const T* __restrict__ qkv, TO* __restrict__ out, int Tn, int H,
                                                            const float* __restrict__ coords, const float* __restrict__ head_scale,
                                                            float* __restrict__ lse_out, const float* __restrict__ out_scale = nullptr,
                                                            TO* __restrict__ u_out = nullptr, TO* __restrict__ osm_out = nullptr,
                                                            const uint8_t* __restrict__ pad = nullptr, uint64_t seed = 0, uint32_t drop_stream = 0,
                                                            uint32_t thr16 = 0, float keep_scale = 1.f, int mask_heads = 0,
                                                            const int4* __restrict__ vwork = nullptr) {
    static_assert(!(VARLEN && (MASK || DROP)), "the ragged form is the inference forward only");
    static_assert(!(DBIAS && (ALIBI || MASK || DROP || VARLEN)), "the pre-softmax distance bias is a plain inference forward");
    constexpr bool COORDS = ALIBI || DBIAS;                              // token coordinates are staged with the K / V tiles
    typedef typename Act<T>::vec8 vec8;
    constexpr int F2_STAGE = 2 * FA_K_BYTES + FA_C_BYTES;                // K rows | V rows | key coordinates (ALiBi)
    __shared__ __attribute__((aligned(16))) char smem[2 * F2_STAGE + (MASK ? 2 * FA_KT : 0)];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y;
    int qblk = blockIdx.x;
    long row0 = (long)b * Tn;                                            // first token row of this bag
    if constexpr (VARLEN) {
        const int4 wk = vwork[blockIdx.x];
        Tn = __builtin_amdgcn_readfirstlane(wk.y);
        if (Tn <= 0) return;                                             // whole workgroup, before any barrier
        row0 = __builtin_amdgcn_readfirstlane(wk.x);
        qblk = __builtin_amdgcn_readfirstlane(wk.z);
    }
    const int Dm = H * 64;
    const long ld = 3L * Dm;
    const T* base = qkv + row0 * ld + h * 64;
    const int ntile = (Tn + FA_KT - 1) / FA_KT;

    // LDS-DMA (attention_train.hip, attn_bwd_dkdv2_kernel): wave w requests 8-row pieces w and w + 4 of the K and V images, rows past the sequence read as 0;
    // ALiBi: the tile's 128 coordinate dwords by waves 0 and 1.  Only the padding flags (bytes at an odd stride) still travel through a register.
    const __amdgpu_buffer_rsrc_t rsrc_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base + Dm), 0, (int)((((long)Tn - 1) * ld + 64) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base + 2 * Dm), 0, (int)((((long)Tn - 1) * ld + 64) * 2), 0x00020000);
    const float* cbase = COORDS ? coords + row0 * 2 : nullptr;
    const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(COORDS ? cbase : head_scale), 0, COORDS ? Tn * 8 : 0, 0x00020000);
    uint8_t mreg = 0;
    const uint8_t* prow = nullptr;
    if constexpr (MASK) prow = pad + (long)(ALIBI ? b : (int)(((long)b * mask_heads + min(h, mask_heads - 1)) % gridDim.z)) * Tn;
    const int drow_ = wave * 8 + (lane >> 3);
    const int vo = drow_ * (int)ld * 2 + (((lane & 7) ^ attn_swz(drow_)) << 4);
    auto stage_load = [&](int j, int buf) {
        char* sK = smem + buf * F2_STAGE;
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
            bufl16(rsrc_k, sK + (wave + 4 * pc) * 1024, vo, (j * FA_KT + 32 * pc) * (int)ld * 2);
            bufl16(rsrc_v, sK + FA_K_BYTES + (wave + 4 * pc) * 1024, vo, (j * FA_KT + 32 * pc) * (int)ld * 2);
        }
        if constexpr (COORDS) {
            if (wave < 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_c, (lptr_t)(sK + 2 * FA_K_BYTES + wave * 256), 4, lane * 4, j * FA_KT * 8 + wave * 256, 0, 0);
        }
        if constexpr (MASK) {
            mreg = 1;
            if (tid < FA_KT && j * FA_KT + tid < Tn) mreg = prow[j * FA_KT + tid];
        }
    };
    auto stage_store = [&](int buf) {
        if constexpr (MASK) {
            if (tid < FA_KT) (smem + 2 * F2_STAGE + buf * FA_KT)[tid] = (char)mreg;
        }
    };

    // this wave's 32 queries
    const int q = qblk * 128 + wave * 32 + l31;
    const int qc = min(q, Tn - 1);
    vec8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const vec8*>(base + (long)qc * ld + (ks * 2 + hi) * 8);

    f32x16 o[2], o2[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[dt][r] = 0.f; o2[dt][r] = 0.f; }
    float mrun = -INFINITY, l = 0.f;
    float xq = 0.f, yq = 0.f, sh = 0.f;
    if constexpr (COORDS) { xq = cbase[(long)qc * 2]; yq = cbase[(long)qc * 2 + 1]; sh = head_scale[h]; }
    if constexpr (DBIAS) sh *= 1.44269504088896340736f;                  // the bias joins the scores in the log2 domain
    const float sc = 0.125f * 1.44269504088896340736f;
    const int swz = attn_swz(l31);
    // transpose reads of the V image (attention_train.hip): lane i of 16-lane group g hands in (key row (i >> 2) of the 4, 8-byte piece i & 3 of its 32 bytes)
    unsigned tra[2][2];
    {
        const int i16 = lane & 15, gd = (lane >> 4) & 1;
#pragma unroll
        for (int w = 0; w < 2; ++w)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const int row = hi * 4 + w * 8 + (i16 >> 2);
                const int lc = dt * 4 + gd * 2 + ((i16 & 3) >> 1);
                tra[w][dt] = (unsigned)(size_t)smem + FA_K_BYTES + row * 128 + ((lc ^ attn_swz(row)) << 4) + (i16 & 1) * 8;
            }
    }
    int flip = F2_STAGE;
    bool qpad = false;
    if constexpr (MASK) qpad = prow[qc] != 0;
    uint32_t rowkey = 0;
    if constexpr (DROP) rowkey = drop_rowkey(seed, drop_stream, (uint64_t)(((long)b * H + h) * Tn + qc));

    const bool wave_live = qblk * 128 + wave * 32 < Tn;
    stage_load(0, 0);
    stage_store(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int j = 0; j < ntile; ++j) {
        const int buf = j & 1;
        if (j + 1 < ntile) stage_load(j + 1, buf ^ 1);
        const char* sK = smem + buf * F2_STAGE;
        const char* sV = sK + FA_K_BYTES;
        const char* sM = smem + 2 * F2_STAGE + buf * FA_KT;
        // A wave whose 32 queries all lie past the sequence (T = 1025 = 8 blocks of 128 + ONE query: three of the ninth block's four waves) only helps staging:
        // its issue slots go to the workgroup that shares the CU (the ninth block was 11 % of the launch for 0.1 % of the queries)
        if (wave_live) {
        f32x16 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const vec8 kf = *reinterpret_cast<const vec8*>(sK + (t * 32 + l31) * 128 + (((ks * 2 + hi) ^ swz) << 4));
                s[t] = Act<T>::mfma32(kf, qf[ks], s[t]);
            }
        }
        const int key0 = j * FA_KT;
        const bool ragged = key0 + FA_KT > Tn;
        if constexpr (DBIAS) {               // s <- log2(e) * (s / 8 - slope_h * dist): from here on the scores are final logits in the log2 domain
            const float* sC = reinterpret_cast<const float*>(sV + FA_K_BYTES);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kl = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const float dx = xq - sC[kl * 2], dy = yq - sC[kl * 2 + 1];
                    s[t][r] = fmaf(s[t][r], sc, -sh * dist_sqrt(fmaf(dx, dx, dy * dy)));
                }
        }
        if (ragged) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= Tn) s[t][r] = -INFINITY;
                }
        }
        uint32_t blocked = 0;            // bit t*16 + r: this (query, key) product is masked out
        uint32_t nodist = 0;             // ALiBi: bit t*16 + r: no distance term either (alibi_mask: blocked, or the class token's row / column)
        if constexpr (MASK) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kl = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const bool bl = (qpad && sM[kl] != 0) || (q > 0 && key0 + kl == 0);
                    blocked |= (bl ? 1u : 0u) << (t * 16 + r);
                    if constexpr (ALIBI) nodist |= ((bl || q == 0 || key0 + kl == 0) ? 1u : 0u) << (t * 16 + r);
                    if (!ALIBI && bl) s[t][r] = -INFINITY;
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float mnew = fmaxf(mrun, DBIAS ? mx : mx * sc);
        float msafe = mnew;
        if constexpr (MASK) msafe = (mnew == -INFINITY) ? 0.f : mnew;       // a query whose keys so far are all blocked
        const float alpha = __builtin_amdgcn_exp2f(mrun - msafe);
        mrun = mnew;
        mnew = msafe;
        float ls = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(DBIAS ? s[t][r] - mnew : fmaf(s[t][r], sc, -mnew));
                s[t][r] = p;
                ls += p;
            }
        l = l * alpha + ls;
        if constexpr (MASK && ALIBI) {       // softmax over all keys, blocked products zeroed afterwards (:66-68)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((blocked >> (t * 16 + r)) & 1u) s[t][r] = 0.f;
        }
        if constexpr (DROP) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const int k = key0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;      // even key, its partner k + 1 sits in register r + 1
                    const uint32_t bits = drop_pair_bits(rowkey, (uint32_t)k >> 1);
                    s[t][r] = drop_keep(bits, 0, thr16) ? s[t][r] * keep_scale : 0.f;
                    s[t][r + 1] = drop_keep(bits, 1, thr16) ? s[t][r + 1] * keep_scale : 0.f;
                }
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            u32x2 tv[8];                    // V^T fragment [ks*4 + dt*2 + w]: keys 16 ks + 8 w + 4 hi + 0..3 of the tile's half t, feature dt*32 + l31
            if (t == 0) FA_TR8(tv, tra[0][0], tra[0][1], tra[1][0], tra[1][1], 0); else FA_TR8(tv, tra[0][0], tra[0][1], tra[1][0], tra[1][1], 4096);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                vec8 pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = Act<T>::from_f32(s[t][ks * 8 + e]);
                vec8 bf;
                if constexpr (ALIBI) {
                    const float* sC = reinterpret_cast<const float*>(sV + FA_K_BYTES);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = ks * 8 + e;
                        const int kl = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        const float dx = xq - sC[kl * 2], dy = yq - sC[kl * 2 + 1];
                        float dist = dist_sqrt(dx * dx + dy * dy) * sh;
                        // (no bounds test: a key past the sequence has zero coordinates -- a finite distance -- and a zero V row)
                        if constexpr (MASK)     // AND with a sign-extended bit: as selects, the 32 conditions were held as wave masks and spilled the scalar file
                            dist = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, dist) & ~(uint32_t)(-(int32_t)((nodist >> (t * 16 + r)) & 1u)));
                        bf[e] = Act<T>::from_f32(dist);
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const vec8 vf = __builtin_bit_cast(vec8, u32x4{tv[ks * 4 + dt * 2][0], tv[ks * 4 + dt * 2][1], tv[ks * 4 + dt * 2 + 1][0], tv[ks * 4 + dt * 2 + 1][1]});
                    o[dt] = Act<T>::mfma32(vf, pf, o[dt]);
                    if constexpr (ALIBI) o2[dt] = Act<T>::mfma32(vf, bf, o2[dt]);
                }
            }
        }
        }
        if (j + 1 < ntile) stage_store(buf ^ 1);
        tra[0][0] += flip; tra[0][1] += flip; tra[1][0] += flip; tra[1][1] += flip;
        flip = -flip;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // the next tile has landed, this wave's reads of the current one are done
        __builtin_amdgcn_s_barrier();
    }
    l += __shfl_xor(l, 32, 64);
    if (lse_out && q < Tn && hi == 0) lse_out[((long)b * H + h) * Tn + q] = mrun + log2f(l);   // log2-domain log-sum-exp
    if (q < Tn) {
        const float inv = 1.0f / l;
        const float osc = (ALIBI && out_scale) ? out_scale[h] : 1.0f;
        TO* orow = out + (row0 + q) * Dm + h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                typename Act<TO>::vec4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = Act<TO>::from_f32(o[dt][4 * g + e] * inv - (ALIBI ? osc * o2[dt][4 * g + e] : 0.f));
                *reinterpret_cast<typename Act<TO>::vec4*>(orow + dt * 32 + 8 * g + 4 * hi) = w;
                if constexpr (ALIBI) {
                    if (u_out) {       // training: U = sum_k (dist / running_mean) v and the softmax part alone (out = Osm - bias_scale * U;
                                       // Osm cannot be rebuilt from the rounded out and U: |U| >> |Osm| cancels catastrophically)
                        const long off = (row0 + q) * Dm + h * 64 + dt * 32 + 8 * g + 4 * hi;
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = Act<TO>::from_f32(o2[dt][4 * g + e]);
                        *reinterpret_cast<typename Act<TO>::vec4*>(u_out + off) = w;
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = Act<TO>::from_f32(o[dt][4 * g + e] * inv);
                        *reinterpret_cast<typename Act<TO>::vec4*>(osm_out + off) = w;
                    }
                }
            }
    }
}



// sum over the 8 lanes that share lane >> 3 (every lane gets it): xor 1, xor 2 (quad_perm), xor 7 (row_half_mirror)
__device__ __forceinline__ float sum8_dpp(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    return v;
}

// ---- ONE query row per (bag, head) against all keys / values of the bag: the class token's attention in the LAST layer of the MIL `vit` head -----------------
// The head reads only the class token's final row (reference vision_tranformer.py: `self.mlp_head(x[:, 0])` behind the last block), so the last block needs keys and
// values of every token but queries, output projection and MLP of the class rows alone (amds_mil_vit_forward).  One 256-thread workgroup per (bag, head): scores
// (thread = key, the 128-byte key row against the query in registers) into LDS, block maximum and sum, then the weighted value sum with thread = (4 dims, one of 16 key
// phases) and a 16-way LDS reduction.  fp32 throughout; q [B][ldq] and out [B][ldo] are 16-bit rows of the heads' 64-channel slices.
// DROP / lse: the training forward's form (amds_attention_fwd_train for query row `qrow` of every bag): dropout on the attention probabilities with the bits of
// the blocked kernel (row key of (bag, head, qrow), one hash per key pair), the log2-domain log-sum-exp of the UNdropped softmax into lse[(b H + h) T + qrow].
// VARLEN (inference): bag b's keys / values are the token rows vbags[b].x .. vbags[b].x + vbags[b].y - 1 of the packed qkv (varlen_plan_kernel; Tn is then the
// launch's LDS bound, the bag's own count comes from the table); q / out stay compact [n_bags][ldq] / [n_bags][ldo].
template <typename T, bool DROP = false, bool VARLEN = false>
__global__ void __launch_bounds__(256) attn_row_kernel(const T* __restrict__ q, long ldq, const T* __restrict__ qkv, T* __restrict__ out, long ldo, int Tn, int H,
                                                       float* __restrict__ lse = nullptr, int qrow = 0, uint64_t seed = 0, uint32_t drop_stream = 0,
                                                       uint32_t thr16 = 0, float keep_scale = 1.f, const int2* __restrict__ vbags = nullptr) {
    static_assert(!(VARLEN && DROP), "the ragged form is the inference forward only");
    typedef typename Act<T>::vec8 vec8;
    typedef typename Act<T>::vec4 vec4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    long row0 = (long)b * Tn;
    if constexpr (VARLEN) {
        const int2 bg = vbags[b];
        row0 = __builtin_amdgcn_readfirstlane(bg.x);
        Tn = min(__builtin_amdgcn_readfirstlane(bg.y), Tn);
        if (Tn <= 0) return;
    }
    extern __shared__ __attribute__((aligned(16))) float sS[];          // [Tn] scores -> weights | [16][64] partial outputs | [8] reductions
    float* sRed = sS + ((Tn + 3) & ~3);
    float* sW = sRed + 16 * 64;
    const int Dm = H * 64;
    const long ld = 3L * Dm;
    const T* base = qkv + row0 * ld + h * 64;
    // scores: eight lanes per key, one 16-byte chunk of the 128-byte key row each (a wave reads eight whole rows per instruction), the dot product summed over
    // the eight lanes by DPP.  (One key per thread -- 64 lanes on 64 different rows per instruction -- ran at 2.9 TB/s.)
    const int sub = tid & 7, kk = tid >> 3;
    float qc[8];
    {
        const vec8 v = *reinterpret_cast<const vec8*>(q + (long)b * ldq + h * 64 + sub * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qc[e] = Act<T>::to_f32(v[e]);
    }
    const float sc = 0.125f * 1.44269504088896340736f;
    float mx = -INFINITY;
    for (int key = kk; key < Tn; key += 32) {
        const vec8 v = *reinterpret_cast<const vec8*>(base + (long)key * ld + Dm + sub * 8);
        float a0 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a0 = fmaf(qc[e], Act<T>::to_f32(v[e]), a0);
        const float sv = sum8_dpp(a0) * sc;
        if (sub == 0) sS[key] = sv;
        mx = fmaxf(mx, sv);
    }
    mx = wave_max(mx);
    if (lane == 0) sW[wave] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(sW[0], sW[1]), fmaxf(sW[2], sW[3]));
    float ls = 0.f;
    for (int key = tid; key < Tn; key += 256) {
        const float pw = __builtin_amdgcn_exp2f(sS[key] - m);
        sS[key] = pw;
        ls += pw;
    }
    ls = wave_sum(ls);
    if (lane == 0) sW[4 + wave] = ls;
    __syncthreads();
    const float l = (sW[4] + sW[5]) + (sW[6] + sW[7]);
    if (lse && tid == 0) lse[((long)b * H + h) * Tn + qrow] = m + log2f(l);
    uint32_t rowkey = 0;
    if constexpr (DROP) rowkey = drop_rowkey(seed, drop_stream, (uint64_t)(((long)b * H + h) * Tn + qrow));
    const int d4 = (tid & 15) * 4, ph = tid >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int key = ph; key < Tn; key += 16) {
        const vec4 v = *reinterpret_cast<const vec4*>(base + (long)key * ld + 2 * Dm + d4);
        float pw = sS[key];
        if constexpr (DROP) pw = drop_keep(drop_pair_bits(rowkey, (uint32_t)key >> 1), key & 1, thr16) ? pw * keep_scale : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(pw, Act<T>::to_f32(v[e]), acc[e]);
    }
    *reinterpret_cast<f32x4*>(sRed + ph * 64 + d4) = acc;
    __syncthreads();
    if (tid < 64) {
        float o = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) o += sRed[k * 64 + tid];
        out[(long)b * ldo + h * 64 + tid] = Act<T>::from_f32(o / l);
    }
}


// Backward of the one-query attention above for query row `qrow` of every bag, when NO other query row of the block has a gradient (the last block of the MIL
// `vit` head): the whole dqkv tensor of the block in one pass -- dK_k = dS_k q / 8 and dV_k = (M o P)_k dO are rank-1 in the one query, dQ is zero but for that
// row.  dS_k = P_k (M_k dP_k - D), dP_k = dO . v_k, D = dO . O (O the dropped output, as stored), P from the saved log-sum-exp; M regenerated from the counters.
template <typename T, bool DROP>
__global__ void __launch_bounds__(256) attn_row_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ o, long ldo, const T* __restrict__ dout, long ldd,
                                                           const float* __restrict__ lse, T* __restrict__ dqkv, int Tn, int H, int qrow, uint64_t seed,
                                                           uint32_t drop_stream, uint32_t thr16, float keep_scale) {
    typedef typename Act<T>::vec8 vec8;
    typedef typename Act<T>::vec4 vec4;
    extern __shared__ __attribute__((aligned(16))) float sS[];          // [Tn] dS | [16][64] partial dq
    float* sRed = sS + ((Tn + 3) & ~3);
    const int tid = threadIdx.x;
    const int h = blockIdx.x, b = blockIdx.y;
    const int Dm = H * 64;
    const long ld = 3L * Dm;
    const T* base = qkv + (long)b * Tn * ld + h * 64;
    T* dbase = dqkv + (long)b * Tn * ld + h * 64;
    // eight lanes per key, one 16-byte chunk of each 128-byte row (q, k, v in; dQ, dK, dV out): whole rows per instruction, the two dot products by DPP
    const int sub = tid & 7, kk = tid >> 3;
    float qc[8], gc[8];
    float Dq = 0.f;
    {
        const vec8 qv = *reinterpret_cast<const vec8*>(base + (long)qrow * ld + sub * 8);
        const vec8 gv = *reinterpret_cast<const vec8*>(dout + (long)b * ldd + h * 64 + sub * 8);
        const vec8 ov = *reinterpret_cast<const vec8*>(o + (long)b * ldo + h * 64 + sub * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qc[e] = Act<T>::to_f32(qv[e]);
            gc[e] = Act<T>::to_f32(gv[e]);
            Dq = fmaf(gc[e], Act<T>::to_f32(ov[e]), Dq);
        }
        Dq = sum8_dpp(Dq);
    }
    const float sc = 0.125f * 1.44269504088896340736f;
    const float L = lse[((long)b * H + h) * Tn + qrow];
    uint32_t rowkey = 0;
    if constexpr (DROP) rowkey = drop_rowkey(seed, drop_stream, (uint64_t)(((long)b * H + h) * Tn + qrow));
    for (int key = kk; key < Tn; key += 32) {
        const T* krow = base + (long)key * ld + Dm + sub * 8;
        const vec8 kv = *reinterpret_cast<const vec8*>(krow), vv = *reinterpret_cast<const vec8*>(krow + Dm);
        float s0 = 0.f, p0 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s0 = fmaf(qc[e], Act<T>::to_f32(kv[e]), s0);
            p0 = fmaf(gc[e], Act<T>::to_f32(vv[e]), p0);
        }
        s0 = sum8_dpp(s0);
        p0 = sum8_dpp(p0);
        const float pk = __builtin_amdgcn_exp2f(s0 * sc - L);
        float mk = 1.f;
        if constexpr (DROP) mk = drop_keep(drop_pair_bits(rowkey, (uint32_t)key >> 1), key & 1, thr16) ? keep_scale : 0.f;
        const float dS = pk * (mk * p0 - Dq), pw = pk * mk, dk = dS * 0.125f;
        if (sub == 0) sS[key] = dS;
        T* drow = dbase + (long)key * ld + sub * 8;
        vec8 wq, wk, wv;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            wq[e] = (T)0.f;
            wk[e] = Act<T>::from_f32(dk * qc[e]);
            wv[e] = Act<T>::from_f32(pw * gc[e]);
        }
        if (key != qrow) *reinterpret_cast<vec8*>(drow) = wq;                      // (the query row's own dQ is written below)
        *reinterpret_cast<vec8*>(drow + Dm) = wk;
        *reinterpret_cast<vec8*>(drow + 2 * Dm) = wv;
    }
    __syncthreads();
    const int d4 = (tid & 15) * 4, ph = tid >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int key = ph; key < Tn; key += 16) {
        const vec4 kv = *reinterpret_cast<const vec4*>(base + (long)key * ld + Dm + d4);
        const float dS = sS[key];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(dS, Act<T>::to_f32(kv[e]), acc[e]);
    }
    *reinterpret_cast<f32x4*>(sRed + ph * 64 + d4) = acc;
    __syncthreads();
    if (tid < 64) {
        float dq = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) dq += sRed[k * 64 + tid];
        dbase[(long)qrow * ld + tid] = Act<T>::from_f32(dq * 0.125f);
    }
}

// ---- the one-query attention WITH the ALiBi distance term (training; reference vision_tranformer.py:42-74 with mask = None, i.e. alibi_mask = None: the class
// row carries the term too, :349-351 puts the class token at (0, 0)):  out = sum_k (p_k - bias_scale_h d_k) v_k,  d_k = |c_q - c_k| / running_mean_h.
// Saves, like the blocked kernel, the softmax part Osm = sum_k p_k v_k and U = sum_k d_k v_k (rows of the (bag, qrow) token) and the log-sum-exp.  fp32 distances
// (the blocked kernel rounds them to 16 bits for its MFMA).  No dropout: nn.MultiheadAttention's rate does not exist on the ALiBi path (:124-154).
template <typename T>
__global__ void __launch_bounds__(256) attn_row_alibi_kernel(const T* __restrict__ qkv, const float* __restrict__ coords, const float* __restrict__ inv_rm,
                                                             const float* __restrict__ bias_scale, T* __restrict__ out, T* __restrict__ u_out, T* __restrict__ osm_out,
                                                             float* __restrict__ lse, int Tn, int H, int qrow) {
    typedef typename Act<T>::vec8 vec8;
    typedef typename Act<T>::vec4 vec4;
    extern __shared__ __attribute__((aligned(16))) float sS[];          // [Tn] scores -> weights | [Tn] scaled distances | 2 x [16][64] partial sums | [8] reductions
    const int Tp = (Tn + 3) & ~3;
    float* sD = sS + Tp;
    float* sRed = sD + Tp;
    float* sW = sRed + 2 * 16 * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    const int Dm = H * 64;
    const long ld = 3L * Dm;
    const T* base = qkv + (long)b * Tn * ld + h * 64;
    const float* cb = coords + (long)b * Tn * 2;
    const float xq = cb[2 * qrow], yq = cb[2 * qrow + 1], irm = inv_rm[h];
    const int sub = tid & 7, kk = tid >> 3;
    float qc[8];
    {
        const vec8 v = *reinterpret_cast<const vec8*>(base + (long)qrow * ld + sub * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qc[e] = Act<T>::to_f32(v[e]);
    }
    const float sc = 0.125f * 1.44269504088896340736f;
    float mx = -INFINITY;
    for (int key = kk; key < Tn; key += 32) {
        const vec8 v = *reinterpret_cast<const vec8*>(base + (long)key * ld + Dm + sub * 8);
        float a0 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a0 = fmaf(qc[e], Act<T>::to_f32(v[e]), a0);
        const float sv = sum8_dpp(a0) * sc;
        if (sub == 0) {
            sS[key] = sv;
            const float dx = xq - cb[2 * key], dy = yq - cb[2 * key + 1];
            sD[key] = dist_sqrt(dx * dx + dy * dy) * irm;
        }
        mx = fmaxf(mx, sv);
    }
    mx = wave_max(mx);
    if (lane == 0) sW[wave] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(sW[0], sW[1]), fmaxf(sW[2], sW[3]));
    float ls = 0.f;
    for (int key = tid; key < Tn; key += 256) {
        const float pw = __builtin_amdgcn_exp2f(sS[key] - m);
        sS[key] = pw;
        ls += pw;
    }
    ls = wave_sum(ls);
    if (lane == 0) sW[4 + wave] = ls;
    __syncthreads();
    const float l = (sW[4] + sW[5]) + (sW[6] + sW[7]);
    if (tid == 0) lse[((long)b * H + h) * Tn + qrow] = m + log2f(l);
    const int d4 = (tid & 15) * 4, ph = tid >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acu = {0.f, 0.f, 0.f, 0.f};
    for (int key = ph; key < Tn; key += 16) {
        const vec4 v = *reinterpret_cast<const vec4*>(base + (long)key * ld + 2 * Dm + d4);
        const float pw = sS[key], dk = sD[key];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float vf = Act<T>::to_f32(v[e]);
            acc[e] = fmaf(pw, vf, acc[e]);
            acu[e] = fmaf(dk, vf, acu[e]);
        }
    }
    *reinterpret_cast<f32x4*>(sRed + ph * 64 + d4) = acc;
    *reinterpret_cast<f32x4*>(sRed + 1024 + ph * 64 + d4) = acu;
    __syncthreads();
    if (tid < 64) {
        float o = 0.f, uu = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { o += sRed[k * 64 + tid]; uu += sRed[1024 + k * 64 + tid]; }
        o /= l;
        const long at = ((long)b * Tn + qrow) * Dm + h * 64 + tid;
        out[at] = Act<T>::from_f32(o - bias_scale[h] * uu);
        u_out[at] = Act<T>::from_f32(uu);
        osm_out[at] = Act<T>::from_f32(o);
    }
}

// Its backward when no other query row of the block has a gradient: dV_k = (p_k - dist_scale_h d_k) dO with dist_scale_h = bias_scale_h / running_mean_h folded
// into d_k's factor below, dS_k = p_k (dO . v_k - dO . Osm), dK_k = dS_k q / 8, dQ = sum_k dS_k k_k / 8 on the query row alone, and
// dbs[b][h] = - dO . U: summed over the bags it is the gradient of bias_scale_h.
template <typename T>
__global__ void __launch_bounds__(256) attn_row_alibi_bwd_kernel(const T* __restrict__ qkv, const T* __restrict__ osm, const T* __restrict__ u, const T* __restrict__ dout,
                                                                 const float* __restrict__ lse, const float* __restrict__ coords, const float* __restrict__ bias_scale,
                                                                 const float* __restrict__ inv_rm, T* __restrict__ dqkv, float* __restrict__ dbs, int Tn, int H, int qrow) {
    typedef typename Act<T>::vec8 vec8;
    typedef typename Act<T>::vec4 vec4;
    extern __shared__ __attribute__((aligned(16))) float sS[];          // [Tn] dS | [16][64] partial dq
    float* sRed = sS + ((Tn + 3) & ~3);
    const int tid = threadIdx.x;
    const int h = blockIdx.x, b = blockIdx.y;
    const int Dm = H * 64;
    const long ld = 3L * Dm;
    const T* base = qkv + (long)b * Tn * ld + h * 64;
    T* dbase = dqkv + (long)b * Tn * ld + h * 64;
    const float* cb = coords + (long)b * Tn * 2;
    const float xq = cb[2 * qrow], yq = cb[2 * qrow + 1], dsc = bias_scale[h] * inv_rm[h];
    const int sub = tid & 7, kk = tid >> 3;
    float qc[8], gc[8];
    float Dq = 0.f, gu = 0.f;
    {
        const long at = ((long)b * Tn + qrow) * Dm + h * 64 + sub * 8;
        const vec8 qv = *reinterpret_cast<const vec8*>(base + (long)qrow * ld + sub * 8);
        const vec8 gv = *reinterpret_cast<const vec8*>(dout + at);
        const vec8 ov = *reinterpret_cast<const vec8*>(osm + at);
        const vec8 uv = *reinterpret_cast<const vec8*>(u + at);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qc[e] = Act<T>::to_f32(qv[e]);
            gc[e] = Act<T>::to_f32(gv[e]);
            Dq = fmaf(gc[e], Act<T>::to_f32(ov[e]), Dq);
            gu = fmaf(gc[e], Act<T>::to_f32(uv[e]), gu);
        }
        Dq = sum8_dpp(Dq);
        gu = sum8_dpp(gu);
    }
    if (tid == 0) dbs[(long)b * H + h] = -gu;
    const float sc = 0.125f * 1.44269504088896340736f;
    const float L = lse[((long)b * H + h) * Tn + qrow];
    for (int key = kk; key < Tn; key += 32) {
        const T* krow = base + (long)key * ld + Dm + sub * 8;
        const vec8 kv = *reinterpret_cast<const vec8*>(krow), vv = *reinterpret_cast<const vec8*>(krow + Dm);
        float s0 = 0.f, p0 = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s0 = fmaf(qc[e], Act<T>::to_f32(kv[e]), s0);
            p0 = fmaf(gc[e], Act<T>::to_f32(vv[e]), p0);
        }
        s0 = sum8_dpp(s0);
        p0 = sum8_dpp(p0);
        const float pk = __builtin_amdgcn_exp2f(s0 * sc - L);
        const float dx = xq - cb[2 * key], dy = yq - cb[2 * key + 1];
        const float dS = pk * (p0 - Dq), pw = pk - dsc * dist_sqrt(dx * dx + dy * dy), dk = dS * 0.125f;
        if (sub == 0) sS[key] = dS;
        T* drow = dbase + (long)key * ld + sub * 8;
        vec8 wq, wk, wv;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            wq[e] = (T)0.f;
            wk[e] = Act<T>::from_f32(dk * qc[e]);
            wv[e] = Act<T>::from_f32(pw * gc[e]);
        }
        if (key != qrow) *reinterpret_cast<vec8*>(drow) = wq;
        *reinterpret_cast<vec8*>(drow + Dm) = wk;
        *reinterpret_cast<vec8*>(drow + 2 * Dm) = wv;
    }
    __syncthreads();
    const int d4 = (tid & 15) * 4, ph = tid >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int key = ph; key < Tn; key += 16) {
        const vec4 kv = *reinterpret_cast<const vec4*>(base + (long)key * ld + Dm + d4);
        const float dS = sS[key];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(dS, Act<T>::to_f32(kv[e]), acc[e]);
    }
    *reinterpret_cast<f32x4*>(sRed + ph * 64 + d4) = acc;
    __syncthreads();
    if (tid < 64) {
        float dq = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) dq += sRed[k * 64 + tid];
        dbase[(long)qrow * ld + tid] = Act<T>::from_f32(dq * 0.125f);
    }
}

// ---- ragged bags: the per-call table of the VARLEN kernels ---------------------------------------------------------------------------------------------------
// One workgroup: bag i = tiles offsets[i] .. offsets[i+1] - 1, clamped so that a malformed array cannot address outside the buffers (offsets to [0, total],
// lengths to [0, max_tiles]); its Tn = len + extra_rows token rows start at row offsets[i] + i * extra_rows < total + n_bags * extra_rows.  extra_rows = 1: a
// class token in front of every bag (the MIL `vit` head); 0: the tile rows alone (barspoon's encoder; an empty bag then has no work item).  Then the flattened
// (bag, q block) list: an exclusive scan of the per-bag block counts (256 thread chunks + an LDS scan), each thread writes its bags' items, the slack up to `nwork` gets
// Tn = 0.  Items past `nwork` (only possible for overlapping, malformed offsets) are dropped.
__global__ void __launch_bounds__(256) varlen_plan_kernel(const int* __restrict__ offsets, int n, long total, int max_tiles, int extra_rows,
                                                          int2* __restrict__ bags, int4* __restrict__ work, long nwork) {
    __shared__ long ssum[256];
    const int tid = threadIdx.x;
    const int per = (n + 255) / 256;
    const int i0 = min(n, tid * per), i1 = min(n, i0 + per);
    auto bag = [&](int i) {
        const long a = min(max((long)offsets[i], 0L), total), e = min(max((long)offsets[i + 1], 0L), total);
        const long len = min(max(e - a, 0L), (long)max_tiles);
        return make_int2((int)(a + (long)i * extra_rows), (int)(len + extra_rows));
    };
    long acc = 0;
    for (int i = i0; i < i1; ++i) {
        const int2 bg = bag(i);
        bags[i] = bg;
        acc += (bg.y + 127) / 128;
    }
    ssum[tid] = acc;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const long v = tid >= s ? ssum[tid - s] : 0;
        __syncthreads();
        ssum[tid] += v;
        __syncthreads();
    }
    long g = ssum[tid] - acc;
    const long used = min(ssum[255], nwork);
    for (int i = i0; i < i1; ++i) {
        const int2 bg = bag(i);
        const int nb = (bg.y + 127) / 128;
        for (int k = 0; k < nb && g < nwork; ++k, ++g) work[g] = make_int4(bg.x, bg.y, k, 0);
    }
    for (long k = used + tid; k < nwork; k += 256) work[k] = make_int4(0, 0, 0, 0);
}

namespace {
inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
}  // namespace

// sum over bags of ceil((len + 1) / 128) <= (total + n + 127 n) / 128; without the class-token row (extra_rows = 0) the sum is no larger
long varlen_work_items(int n_bags, long total_tiles) { return (total_tiles + 128L * n_bags) / 128 + 1; }
size_t varlen_table_bytes(int n_bags, long total_tiles) { return al256((size_t)n_bags * 8) + al256((size_t)varlen_work_items(n_bags, total_tiles) * 16); }
const int2* varlen_table_bags(const void* table) { return reinterpret_cast<const int2*>(table); }

int varlen_table_build(const int* offsets, int n_bags, long total_tiles, int max_tiles, int extra_rows, void* table, hipStream_t st) {
    char* t = reinterpret_cast<char*>(table);
    hipLaunchKernelGGL(varlen_plan_kernel, dim3(1), dim3(256), 0, st, offsets, n_bags, total_tiles, max_tiles, extra_rows, reinterpret_cast<int2*>(t),
                       reinterpret_cast<int4*>(t + al256((size_t)n_bags * 8)), varlen_work_items(n_bags, total_tiles));
    AMDS_LAUNCH_CHECK("varlen_plan_kernel");
    return AMDS_OK;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------------------------------
// The optional arguments of attn_flash_kernel; an entry names those of its variant and leaves the rest off.
struct FlashOpt {
    const float* coords = nullptr;          // ALIBI: token coordinates and the per-head factor of the distance (1 / running mean; inference: bias scale folded in)
    const float* head_scale = nullptr;
    float* lse = nullptr;                   // training: log-sum-exp per query
    const float* bias_scale = nullptr;      // ALiBi training: out = Osm - bias_scale U, both saved
    void* u = nullptr;
    void* osm = nullptr;
    const uint8_t* pad = nullptr;           // MASK
    int mask_heads = 0;
    float p = 0.f;                          // DROP
    uint64_t seed = 0;
    uint32_t stream_id = 0;
    const int4* vwork = nullptr;            // VARLEN: the work list and its length (the grid's x; T is then unused)
    unsigned n_work = 0;
};

// One launch of the streaming kernel: grid, profiler scope and the dtype ladder.  The variant is the entry's (template flags), the operand type the call's;
// OUT_AS_IN = false: bf16 out / U / Osm whatever the operands (the ALiBi forms, see the kernel comment).  `who` names the entry in the dtype message.
template <bool ALIBI, bool MASK = false, bool DROP = false, bool VARLEN = false, bool OUT_AS_IN = !ALIBI, bool DBIAS = false>
static int flash_launch(const char* who, const char* kname, const void* qkv, void* out, int B, int T, int H, int dtype, const FlashOpt& o, hipStream_t st) {
    const dim3 grid(VARLEN ? o.n_work : (unsigned)((T + 127) / 128), H, B), block(256);
    std::optional<ProfScope> prof;          // (the ragged forms are timed by their callers)
    if constexpr (!VARLEN) prof.emplace(PROF_ATTN, (ALIBI ? 6.0 : 4.0) * B * H * (double)T * T * 64, st);
    const DropParams d(o.p);
    const bool ok = dispatch_16(dtype, [&](auto t) {
        typedef AMDS_TAG_T(t) TI;
        typedef std::conditional_t<OUT_AS_IN, TI, bf16> TO;
        hipLaunchKernelGGL((attn_flash_kernel<TI, ALIBI, TO, MASK, DROP, VARLEN, DBIAS>), grid, block, 0, st, (const TI*)qkv, (TO*)out, T, H, o.coords, o.head_scale, o.lse,
                           o.bias_scale, (TO*)o.u, (TO*)o.osm, o.pad, o.seed, o.stream_id, d.thr, d.scale, o.mask_heads, o.vwork);
    });
    if (!ok) { set_error("%s: bad dtype %d", who, dtype); return AMDS_ERR_INVALID; }
    AMDS_LAUNCH_CHECK(kname);
    return AMDS_OK;
}

int attention_varlen_launch(const void* qkv, const float* coords, const float* head_scale, void* out, const void* table, int n_bags, long total_tiles,
                            int H, int dtype, hipStream_t st) {
    FlashOpt o;
    o.vwork = reinterpret_cast<const int4*>(reinterpret_cast<const char*>(table) + al256((size_t)n_bags * 8));
    o.n_work = (unsigned)varlen_work_items(n_bags, total_tiles);
    o.coords = coords;
    o.head_scale = head_scale;
    if (coords) return flash_launch<true, false, false, true>("attention_varlen_launch", "attn_flash_kernel<alibi, varlen>", qkv, out, 1, 0, H, dtype, o, st);
    return flash_launch<false, false, false, true>("attention_varlen_launch", "attn_flash_kernel<varlen>", qkv, out, 1, 0, H, dtype, o, st);
}

// One launch of the one-query kernel (q rows at pitch ldq from element q_off, out rows at pitch ldo from element o_off, one per bag);
// LDS: [T] weights | [16][64] partial sums | [8] reductions
template <bool DROP, bool VARLEN = false>
static int row_launch(const char* who, const char* kname, const void* q, long q_off, long ldq, const void* qkv, void* out, long o_off, long ldo, int B, int T, int H,
                      int dtype, float* lse, int qrow, float p, uint64_t seed, uint32_t stream_id, const int2* bags, hipStream_t st) {
    const size_t lds = ((size_t)((T + 3) & ~3) + 16 * 64 + 8) * 4;
    const DropParams d(p);
    int rc = AMDS_OK;
    const bool ok = dispatch_16(dtype, &rc, [&](auto t) -> int {
        typedef AMDS_TAG_T(t) TT;
        AMDS_HIP(lds_opt_in<attn_row_kernel<TT, DROP, VARLEN>>(140 * 1024));
        hipLaunchKernelGGL((attn_row_kernel<TT, DROP, VARLEN>), dim3(H, B), dim3(256), lds, st, (const TT*)q + q_off, ldq, (const TT*)qkv, (TT*)out + o_off, ldo, T, H, lse,
                           qrow, seed, stream_id, d.thr, d.scale, bags);
        AMDS_LAUNCH_CHECK(kname);
        return AMDS_OK;
    });
    if (!ok) { set_error("%s: bad dtype %d", who, dtype); return AMDS_ERR_INVALID; }
    return rc;
}

int attention_row_varlen_launch(const void* q, long ldq, const void* qkv, void* out, long ldo, const void* table, int n_bags, int max_tiles, int H, int dtype,
                                hipStream_t st) {
    return row_launch<false, true>("attention_row_varlen_launch", "attn_row_kernel<varlen>", q, 0, ldq, qkv, out, 0, ldo, n_bags, max_tiles + 1, H, dtype, nullptr, 0, 0.f, 0,
                                   0, varlen_table_bags(table), st);
}

}  // namespace amds

using namespace amds;

extern "C" int amds_attention(const void* qkv, void* out, int B, int T, int H, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && out, "amds_attention: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H), "amds_attention: bad shape B=%d T=%d H=%d", B, T, H);
    if (B == 0) return AMDS_OK;
    return flash_launch<false>("amds_attention", "attn_flash_kernel", qkv, out, B, T, H, dtype, FlashOpt{}, (hipStream_t)stream);
}

extern "C" int amds_attention_row(const void* q, long ldq, const void* qkv, void* out, long ldo, int B, int T, int H, int dtype, void* stream) {
    AMDS_REQUIRE(q && qkv && out, "amds_attention_row: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && T <= 32768 && H > 0 && H <= 65535 && B <= 65535 && ldq >= H * 64 && ldo >= H * 64 && ldq % 8 == 0, "amds_attention_row: bad shape B=%d T=%d H=%d", B, T, H);
    if (B == 0) return AMDS_OK;
    return row_launch<false>("amds_attention_row", "attn_row_kernel", q, 0, ldq, qkv, out, 0, ldo, B, T, H, dtype, nullptr, 0, 0.f, 0, 0, nullptr, (hipStream_t)stream);
}

extern "C" int amds_attention_row_fwd_train(const void* qkv, void* out, float* lse, int B, int T, int H, int qrow, int dtype, float p, uint64_t seed,
                                            uint32_t stream_id, void* stream) {
    AMDS_REQUIRE(qkv && out && lse, "amds_attention_row_fwd_train: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && T <= 32768 && H > 0 && H <= 65535 && B <= 65535 && qrow >= 0 && qrow < T && p >= 0.f && p < 1.f,
                 "amds_attention_row_fwd_train: bad arguments B=%d T=%d H=%d row=%d p=%f", B, T, H, qrow, p);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "amds_attention_row_fwd_train: bad dtype %d", dtype);
    if (B == 0) return AMDS_OK;
    const long Dm = (long)H * 64, ldq = (long)T * 3 * Dm, ldo = (long)T * Dm;
    const long q_off = (long)qrow * 3 * Dm, o_off = (long)qrow * Dm;      // the query row and its output row inside the [B][T] tensors
    const char *who = "amds_attention_row_fwd_train", *kname = "attn_row_kernel<train>";
    if (p > 0.f) return row_launch<true>(who, kname, qkv, q_off, ldq, qkv, out, o_off, ldo, B, T, H, dtype, lse, qrow, p, seed, stream_id, nullptr, (hipStream_t)stream);
    return row_launch<false>(who, kname, qkv, q_off, ldq, qkv, out, o_off, ldo, B, T, H, dtype, lse, qrow, 0.f, seed, stream_id, nullptr, (hipStream_t)stream);
}

extern "C" int amds_attention_row_bwd_train(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int T, int H, int qrow,
                                            int dtype, float p, uint64_t seed, uint32_t stream_id, void* stream) {
    AMDS_REQUIRE(qkv && out && dout && lse && dqkv, "amds_attention_row_bwd_train: null pointer");
    AMDS_REQUIRE(B > 0 && T > 0 && T <= 32768 && H > 0 && H <= 65535 && B <= 65535 && qrow >= 0 && qrow < T && p >= 0.f && p < 1.f,
                 "amds_attention_row_bwd_train: bad arguments B=%d T=%d H=%d row=%d p=%f", B, T, H, qrow, p);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "amds_attention_row_bwd_train: bad dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)((T + 3) & ~3) + 16 * 64) * 4;
    const long Dm = (long)H * 64, ldo = (long)T * Dm;
    const DropParams d(p);
    auto launch = [&](auto t, auto drop) -> int {
        typedef AMDS_TAG_T(t) TT;
        constexpr bool DR = decltype(drop)::value;
        AMDS_HIP(lds_opt_in<attn_row_bwd_kernel<TT, DR>>(140 * 1024));
        hipLaunchKernelGGL((attn_row_bwd_kernel<TT, DR>), dim3(H, B), dim3(256), lds, st, (const TT*)qkv, (const TT*)out + (long)qrow * Dm, ldo,
                           (const TT*)dout + (long)qrow * Dm, ldo, lse, (TT*)dqkv, T, H, qrow, seed, stream_id, d.thr, d.scale);
        AMDS_LAUNCH_CHECK("attn_row_bwd_kernel");
        return AMDS_OK;
    };
    int rc = AMDS_OK;                                                    // the dtype was checked above: the ladder cannot come back false
    dispatch_16(dtype, &rc, [&](auto t) { return p > 0.f ? launch(t, std::true_type{}) : launch(t, std::false_type{}); });
    return rc;
}

extern "C" int amds_attention_row_alibi_fwd_train(const void* qkv, const float* coords, const float* inv_running_mean, const float* bias_scale, void* out, void* u,
                                                  void* osm, float* lse, int B, int T, int H, int qrow, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && coords && inv_running_mean && bias_scale && out && u && osm && lse, "amds_attention_row_alibi_fwd_train: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && T <= 16384 && H > 0 && H <= 65535 && B <= 65535 && qrow >= 0 && qrow < T, "amds_attention_row_alibi_fwd_train: bad arguments B=%d T=%d H=%d row=%d",
                 B, T, H, qrow);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "amds_attention_row_alibi_fwd_train: bad dtype %d", dtype);
    if (B == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)2 * ((T + 3) & ~3) + 2 * 16 * 64 + 8) * 4;
    int rc = AMDS_OK;                                                    // the dtype was checked above: the ladder cannot come back false
    dispatch_16(dtype, &rc, [&](auto t) -> int {
        typedef AMDS_TAG_T(t) TT;
        AMDS_HIP(lds_opt_in<attn_row_alibi_kernel<TT>>(140 * 1024));
        hipLaunchKernelGGL((attn_row_alibi_kernel<TT>), dim3(H, B), dim3(256), lds, st, (const TT*)qkv, coords, inv_running_mean, bias_scale, (TT*)out, (TT*)u, (TT*)osm, lse, T, H, qrow);
        AMDS_LAUNCH_CHECK("attn_row_alibi_kernel");
        return AMDS_OK;
    });
    return rc;
}

extern "C" int amds_attention_row_alibi_bwd_train(const void* qkv, const void* osm, const void* u, const void* dout, const float* lse, const float* coords,
                                                  const float* bias_scale, const float* inv_running_mean, void* dqkv, float* dbs, int B, int T, int H, int qrow, int dtype,
                                                  void* stream) {
    AMDS_REQUIRE(qkv && osm && u && dout && lse && coords && bias_scale && inv_running_mean && dqkv && dbs, "amds_attention_row_alibi_bwd_train: null pointer");
    AMDS_REQUIRE(B > 0 && T > 0 && T <= 32768 && H > 0 && H <= 65535 && B <= 65535 && qrow >= 0 && qrow < T, "amds_attention_row_alibi_bwd_train: bad arguments B=%d T=%d H=%d row=%d",
                 B, T, H, qrow);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "amds_attention_row_alibi_bwd_train: bad dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)((T + 3) & ~3) + 16 * 64) * 4;
    int rc = AMDS_OK;                                                    // the dtype was checked above: the ladder cannot come back false
    dispatch_16(dtype, &rc, [&](auto t) -> int {
        typedef AMDS_TAG_T(t) TT;
        AMDS_HIP(lds_opt_in<attn_row_alibi_bwd_kernel<TT>>(140 * 1024));
        hipLaunchKernelGGL((attn_row_alibi_bwd_kernel<TT>), dim3(H, B), dim3(256), lds, st, (const TT*)qkv, (const TT*)osm, (const TT*)u, (const TT*)dout, lse, coords, bias_scale,
                           inv_running_mean, (TT*)dqkv, dbs, T, H, qrow);
        AMDS_LAUNCH_CHECK("attn_row_alibi_bwd_kernel");
        return AMDS_OK;
    });
    return rc;
}

extern "C" int amds_attention_alibi(const void* qkv, const float* coords, const float* head_scale, void* out, int B, int T,
                                    int H, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && out && coords && head_scale, "amds_attention_alibi: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H), "amds_attention_alibi: bad shape B=%d T=%d H=%d", B, T, H);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.coords = coords;
    o.head_scale = head_scale;
    return flash_launch<true>("amds_attention_alibi", "attn_flash_kernel<alibi>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}

// TICON's attention (kernel comment, DBIAS): the distance bias before the softmax; out in the operand type
extern "C" int amds_attention_distbias(const void* qkv, const float* coords, const float* slopes, void* out, int B, int T, int H, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && out && coords && slopes, "amds_attention_distbias: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H), "amds_attention_distbias: bad shape B=%d T=%d H=%d", B, T, H);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.coords = coords;
    o.head_scale = slopes;
    return flash_launch<false, false, false, false, true, true>("amds_attention_distbias", "attn_flash_kernel<distbias>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}

// forward that also stores L[b][h][q] = log2(sum_k exp2(s_qk * log2(e)/8)) for amds_attention_bwd
extern "C" int amds_attention_fwd_lse(const void* qkv, void* out, float* lse, int B, int T, int H, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && out && lse, "amds_attention_fwd_lse: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H), "amds_attention_fwd_lse: bad shape B=%d T=%d H=%d", B, T, H);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.lse = lse;
    return flash_launch<false>("amds_attention_fwd_lse", "attn_flash_kernel<lse>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}

// Training forward of the ALiBi attention (reference vision_tranformer.py:42-74 in train mode): head_scale = 1 / running_mean
// (already updated by the caller, :24-29), out = softmax(q k^T / 8) v - bias_scale_h * U with U = sum_k (dist / running_mean) v.
// Saves what the backward needs: L = log2-sum-exp per query, U and the softmax part Osm -- all three bf16 from the C entry, in the operand type itself
// (out_as_in) from the dtype-taking form at AMDS_F16: the training step at float32_matmul_precision "high".
static int alibi_fwd_train(const void* qkv, const float* coords, const float* inv_running_mean, const float* bias_scale, void* out, void* u, void* osm, float* lse,
                           int B, int T, int H, int dtype, bool out_as_in, void* stream) {
    const char* who = "amds_attention_alibi_fwd_train";
    AMDS_REQUIRE(qkv && coords && inv_running_mean && bias_scale && out && u && osm && lse, "%s: null pointer", who);
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H), "%s: bad shape B=%d T=%d H=%d", who, B, T, H);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.coords = coords;
    o.head_scale = inv_running_mean;
    o.lse = lse;
    o.bias_scale = bias_scale;
    o.u = u;
    o.osm = osm;
    if (out_as_in) return flash_launch<true, false, false, false, true>(who, "attn_flash_kernel<alibi,train,f16>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
    return flash_launch<true>(who, "attn_flash_kernel<alibi,train>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}
extern "C" int amds_attention_alibi_fwd_train(const void* qkv, const float* coords, const float* inv_running_mean, const float* bias_scale,
                                              void* out_bf16, void* u_bf16, void* osm_bf16, float* lse, int B, int T, int H, int dtype, void* stream) {
    return alibi_fwd_train(qkv, coords, inv_running_mean, bias_scale, out_bf16, u_bf16, osm_bf16, lse, B, T, H, dtype, false, stream);
}
int amds::attention_alibi_fwd_train_dt(const void* qkv, const float* coords, const float* inv_running_mean, const float* bias_scale, void* out, void* u, void* osm,
                                       float* lse, int B, int T, int H, int dtype, void* stream) {
    return alibi_fwd_train(qkv, coords, inv_running_mean, bias_scale, out, u, osm, lse, B, T, H, dtype, dtype == AMDS_F16, stream);
}

// `mask != None` forward of the reference (vision_tranformer.py:355-381; pinned by the reference's tests/test_model.py:28-32): pad u8 [B][T]
// with the class token included at t = 0 (never padded).  See the kernel comment for the literal blocking rule.
extern "C" int amds_attention_masked(const void* qkv, const uint8_t* pad, void* out, int B, int T, int H, int mask_heads, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && out && pad, "amds_attention_masked: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H) && mask_heads > 0 && mask_heads <= H, "amds_attention_masked: bad shape B=%d T=%d H=%d mask_heads=%d", B, T, H, mask_heads);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.pad = pad;
    o.mask_heads = mask_heads;
    return flash_launch<false, true>("amds_attention_masked", "attn_flash_kernel<mask>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}

extern "C" int amds_attention_alibi_masked(const void* qkv, const float* coords, const float* head_scale, const uint8_t* pad, void* out, int B, int T,
                                           int H, int dtype, void* stream) {
    AMDS_REQUIRE(qkv && out && coords && head_scale && pad, "amds_attention_alibi_masked: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H), "amds_attention_alibi_masked: bad shape B=%d T=%d H=%d", B, T, H);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.coords = coords;
    o.head_scale = head_scale;
    o.pad = pad;
    return flash_launch<true, true>("amds_attention_alibi_masked", "attn_flash_kernel<alibi,mask>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}

// Training forward of nn.MultiheadAttention with dropout p on the attention probabilities (vision_tranformer.py:191: the `dropout`
// constructor argument reaches MultiheadAttention; train mode): out = drop(P) v; lse as amds_attention_fwd_lse.  p = 0 is that call.
extern "C" int amds_attention_fwd_train(const void* qkv, void* out, float* lse, int B, int T, int H, int dtype, float p, uint64_t seed,
                                        uint32_t stream_id, void* stream) {
    if (p == 0.f) return amds_attention_fwd_lse(qkv, out, lse, B, T, H, dtype, stream);
    AMDS_REQUIRE(qkv && out && lse, "amds_attention_fwd_train: null pointer");
    AMDS_REQUIRE(B >= 0 && T > 0 && H > 0 && H <= 65535 && B <= 65535 && FA_SPAN_OK(T, H) && p > 0.f && p < 1.f, "amds_attention_fwd_train: bad arguments B=%d T=%d H=%d p=%f", B, T, H, p);
    if (B == 0) return AMDS_OK;
    FlashOpt o;
    o.lse = lse;
    o.p = p;
    o.seed = seed;
    o.stream_id = stream_id;
    return flash_launch<false, false, true>("amds_attention_fwd_train", "attn_flash_kernel<drop>", qkv, out, B, T, H, dtype, o, (hipStream_t)stream);
}


// ---- ragged bags (include/amdstamp.h, "ragged bags") ------------------------------------------------------------------------------------------------------------
extern "C" size_t amds_attention_varlen_workspace_bytes(int n_bags, long total_tiles) {
    if (n_bags < 0 || total_tiles < 0) return 0;
    return varlen_table_bytes(n_bags, total_tiles);
}

static int varlen_check(const char* who, const void* qkv, const int* offsets, const void* out, int n_bags, long total_tiles, int max_tiles, int H, int dtype,
                        const void* ws, size_t ws_bytes, int t_limit, int extra_rows = 1) {
    AMDS_REQUIRE(qkv && offsets && out && ws, "%s: null pointer", who);
    AMDS_REQUIRE(n_bags >= 0 && n_bags <= 65535 && total_tiles >= 0 && max_tiles >= 0 && max_tiles + extra_rows <= t_limit && H > 0 && H <= 65535 &&
                 total_tiles + (long)n_bags * extra_rows < (1L << 31) && FA_SPAN_OK(max_tiles + extra_rows, H),
                 "%s: bad shape n_bags=%d total_tiles=%ld max_tiles=%d H=%d (a bag's q | k | v rows must stay below the 2 GB of a buffer descriptor)", who, n_bags,
                 total_tiles, max_tiles, H);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "%s: bad dtype %d", who, dtype);
    const size_t need = varlen_table_bytes(n_bags, total_tiles);
    if (ws_bytes < need) {
        set_error("%s: workspace %zu < required %zu bytes", who, ws_bytes, need);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    return AMDS_OK;
}

extern "C" int amds_attention_varlen(const void* qkv, const int* offsets, void* out, int n_bags, long total_tiles, int max_tiles, int H, int dtype, void* ws,
                                     size_t ws_bytes, void* stream) {
    int rc = varlen_check("amds_attention_varlen", qkv, offsets, out, n_bags, total_tiles, max_tiles, H, dtype, ws, ws_bytes, 1 << 30);
    if (rc != AMDS_OK || n_bags == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = varlen_table_build(offsets, n_bags, total_tiles, max_tiles, 1, ws, st)) != AMDS_OK) return rc;
    return attention_varlen_launch(qkv, nullptr, nullptr, out, ws, n_bags, total_tiles, H, dtype, st);
}

// the class-token-less layout (barspoon's encoder): bag i = rows offsets[i] .. offsets[i+1] - 1 of qkv / out [total_rows]; the same kernel on a table built
// with extra_rows = 0
extern "C" int amds_attention_varlen_rows(const void* qkv, const int* offsets, void* out, int n_bags, long total_rows, int max_rows, int H, int dtype, void* ws,
                                          size_t ws_bytes, void* stream) {
    int rc = varlen_check("amds_attention_varlen_rows", qkv, offsets, out, n_bags, total_rows, max_rows, H, dtype, ws, ws_bytes, 1 << 30, 0);
    if (rc != AMDS_OK || n_bags == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = varlen_table_build(offsets, n_bags, total_rows, max_rows, 0, ws, st)) != AMDS_OK) return rc;
    return attention_varlen_launch(qkv, nullptr, nullptr, out, ws, n_bags, total_rows, H, dtype, st);
}

extern "C" int amds_attention_alibi_varlen(const void* qkv, const float* coords, const float* head_scale, const int* offsets, void* out, int n_bags,
                                           long total_tiles, int max_tiles, int H, int dtype, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(coords && head_scale, "amds_attention_alibi_varlen: null pointer");
    int rc = varlen_check("amds_attention_alibi_varlen", qkv, offsets, out, n_bags, total_tiles, max_tiles, H, dtype, ws, ws_bytes, 1 << 30);
    if (rc != AMDS_OK || n_bags == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = varlen_table_build(offsets, n_bags, total_tiles, max_tiles, 1, ws, st)) != AMDS_OK) return rc;
    return attention_varlen_launch(qkv, coords, head_scale, out, ws, n_bags, total_tiles, H, dtype, st);
}

extern "C" int amds_attention_row_varlen(const void* q, long ldq, const void* qkv, const int* offsets, void* out, long ldo, int n_bags, long total_tiles,
                                         int max_tiles, int H, int dtype, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(q, "amds_attention_row_varlen: null pointer");
    int rc = varlen_check("amds_attention_row_varlen", qkv, offsets, out, n_bags, total_tiles, max_tiles, H, dtype, ws, ws_bytes, 32768);
    if (rc != AMDS_OK) return rc;
    AMDS_REQUIRE(ldq >= H * 64 && ldo >= H * 64 && ldq % 8 == 0, "amds_attention_row_varlen: bad pitches ldq=%ld ldo=%ld", ldq, ldo);
    if (n_bags == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = varlen_table_build(offsets, n_bags, total_tiles, max_tiles, 1, ws, st)) != AMDS_OK) return rc;
    return attention_row_varlen_launch(q, ldq, qkv, out, ldo, ws, n_bags, max_tiles, H, dtype, st);
}
