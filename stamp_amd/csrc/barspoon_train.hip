// barspoon_train.hip -- the TRAINING forward and backward of the reference's barspoon head (`EncDecTransformer`), one call each.
//
// Forward = the train-mode form of src/stamp/modeling/models/barspoon.py:164-205 (torch's pre-norm nn.TransformerEncoder / nn.TransformerDecoder with their
// dropout sites live; the reference instantiates them with torch's default dropout = 0.1, barspoon.py:118-162); backward = what autograd derives from it
// (`LitMilClassificationMixin.step`, barspoon.py:263-321 -> loss.backward()).  Like mil_vit_train.hip both are launch sequences over kernels the library
// exposes one by one: the tile side (projector, encoder, the K | V projections of the cross-attention) on 16-bit MFMA operands with fp32 accumulation /
// residual stream / gradients, in the zero-padded layout of the MIL `vit` head; the class-token side (n_targets rows per bag) in exact fp32 (amds_bgemm_f32's
// exact form) in both directions.  New here: the training cross-attention (a few fp32 queries against T 16-bit keys / values, dropout on the probabilities)
// and its backward.  Activations live in ONE caller-owned arena (`saved`, read-only after the forward), gradients go to caller-owned fp32 buffers, every
// reduction over tiles runs through fixed-order partials (no float atomics), nothing is allocated and the host never waits for the device.
#include <algorithm>
#include <vector>
#include "barspoon_common.h"

namespace amds {
namespace {

constexpr int CA_KEYS = 256;       // keys per workgroup of the cross-attention backward (one per lane)
constexpr int CA_JB = 16;          // queries per pass of that kernel (the LDS tile of dS)
constexpr int CA_KPITCH = 72;      // LDS pitch of a key row in elements (64 channels + 16 bytes: rows start on different banks, 16-byte aligned)

// ---- training cross-attention, forward: one wave per (bag, target, head), lane l streams the keys l, l + 64, ... with its own running (max, sum, o[64]);
// the 64 partial states are merged once at the end (the deploy kernel's form; barspoon.hip).  `l` sums the UNDROPPED probabilities (the softmax's
// normaliser and lse), `o` the kept ones times the keep scale.
template <typename T>
__global__ void __launch_bounds__(256) cross_attn_fwd_train_kernel(const float* __restrict__ q, const T* __restrict__ kv, float* __restrict__ out, float* __restrict__ lse,
                                                                    int B, int Tn, int nt, int H, int hd, int D, int Db, uint64_t seed, uint32_t sid, uint32_t thr,
                                                                    float scale) {
    typedef T vec8 __attribute__((ext_vector_type(8)));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + wave;
    if (item >= (long)B * nt * H) return;                      // whole waves leave; no workgroup barrier below
    const int h = (int)(item % H);
    const long bj = item / H;
    const int b = (int)(bj / nt), j = (int)(bj - (long)b * nt);
    const float* qr = q + bj * D + (long)h * hd;
    const float sc = rsqrtf((float)hd) * 1.44269504088896340736f;          // log2 domain
    const long row = ((long)b * H + h) * nt + j;
    const uint32_t key = drop_rowkey(seed, sid, (uint64_t)row);
    float qv[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) qv[e] = e < hd ? qr[e] * sc : 0.f;
    float m = -INFINITY, l = 0.f, o[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) o[e] = 0.f;
    const long ld = 2L * Db;
    const T* kb = kv + (long)b * Tn * ld + 64 * h;
    for (int t = lane; t < Tn; t += 64) {
        const T* kr = kb + t * ld;
        float s = 0.f;
#pragma unroll
        for (int pz = 0; pz < 8; ++pz) {
            const vec8 kk = *reinterpret_cast<const vec8*>(kr + 8 * pz);
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(qv[8 * pz + e], (float)kk[e], s);
        }
        const float mn = fmaxf(m, s);
        const float corr = exp2f(m - mn), pw = exp2f(s - mn);
        l = l * corr + pw;
        const bool keep = drop_keep(drop_pair_bits(key, (uint32_t)t >> 1), t & 1, thr);
        const float pd = keep ? pw * scale : 0.f;
        const T* vr = kr + Db;
#pragma unroll
        for (int pz = 0; pz < 8; ++pz) {
            const vec8 vv = *reinterpret_cast<const vec8*>(vr + 8 * pz);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[8 * pz + e] = fmaf(o[8 * pz + e], corr, pd * (float)vv[e]);
        }
        m = mn;
    }
    float mg = m;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mg = fmaxf(mg, __shfl_xor(mg, off, 64));
    const float w = m == -INFINITY ? 0.f : exp2f(m - mg);
    l *= w;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off, 64);
    const float inv = 1.0f / l;
    float* orow = out + bj * D + (long)h * hd;
#pragma unroll
    for (int e = 0; e < 64; ++e) {
        float v = o[e] * w;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0 && e < hd) orow[e] = v * inv;
    }
    if (lane == 0) lse[row] = mg + log2f(l);
}

// ---- training cross-attention, backward.  One workgroup per (bag, head, chunk of 256 keys), one key per lane: the lane holds its K and V rows (2 x 128 bytes,
// read once with 16-byte loads) and the fp32 dK / dV rows it will write once; ALL nt queries of the (bag, head) pass by in tiles of CA_JB, staged in LDS and
// read as broadcasts.  Per (key, query): s = q . k, p = exp2(s - lse), dp = keep * scale * (dout . v), ds = p (dp - delta), dV += keep * scale * p * dout,
// dK += ds * q / sqrt(hd) -- no cross-lane step.  dq needs the sum over keys: ds goes to LDS as a [CA_JB][256] tile and a second phase forms
// dq[j][d] = sum_t ds[j][t] K[t][d] from the K rows kept in LDS (lane = channel d, a fixed order over t), written as this chunk's partial; the partials are
// summed in chunk order by cross_attn_dq_reduce_kernel.  delta[j] = dout[j] . out[j] (it equals sum_t p dp also under dropout).
template <typename T>
__global__ void __launch_bounds__(256) cross_attn_bwd_train_kernel(const float* __restrict__ q, const T* __restrict__ kv, const float* __restrict__ out,
                                                                    const float* __restrict__ dout, const float* __restrict__ lse, T* __restrict__ dkv, long lddkv,
                                                                    float* __restrict__ dq_part, int Tn, int nt, int H, int hd, int D, int Db, int nchunk,
                                                                    uint64_t seed, uint32_t sid, uint32_t thr, float scale) {
    typedef T vec8 __attribute__((ext_vector_type(8)));
    __shared__ __attribute__((aligned(16))) T Ks[CA_KEYS * CA_KPITCH];
    __shared__ __attribute__((aligned(16))) float dSs[CA_JB * CA_KEYS];
    __shared__ __attribute__((aligned(16))) float q_s[CA_JB * 64];
    __shared__ __attribute__((aligned(16))) float do_s[CA_JB * 64];
    __shared__ float lse_s[CA_JB], dl_s[CA_JB];
    const int tid = threadIdx.x, chunk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int t = chunk * CA_KEYS + tid;
    const bool live = t < Tn;
    vec8 kk[8], vv[8];
    {
        const T* kr = kv + ((long)b * Tn + (live ? t : 0)) * (2L * Db) + 64 * h;
#pragma unroll
        for (int pz = 0; pz < 8; ++pz) {
            vec8 zero;
#pragma unroll
            for (int e = 0; e < 8; ++e) zero[e] = (T)0.f;
            kk[pz] = live ? *reinterpret_cast<const vec8*>(kr + 8 * pz) : zero;
            vv[pz] = live ? *reinterpret_cast<const vec8*>(kr + Db + 8 * pz) : zero;
            *reinterpret_cast<vec8*>(&Ks[tid * CA_KPITCH + 8 * pz]) = kk[pz];
        }
    }
    float dK[64], dV[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) dK[e] = dV[e] = 0.f;
    const float rs = rsqrtf((float)hd);
    const float sc = rs * 1.44269504088896340736f;
    const long bh = (long)b * H + h;
    for (int j0 = 0; j0 < nt; j0 += CA_JB) {
        const int jb = min(CA_JB, nt - j0);
        __syncthreads();                                       // the previous tile's second phase has read dSs / Ks; (first pass: Ks is complete)
        for (int i = tid; i < CA_JB * 64; i += 256) {
            const int jj = i >> 6, e = i & 63;
            const bool ok = jj < jb && e < hd;
            const long o = ((long)b * nt + j0 + jj) * D + (long)h * hd + e;
            q_s[i] = ok ? q[o] * sc : 0.f;
            do_s[i] = ok ? dout[o] : 0.f;
        }
        if (tid < jb) {
            const long o = ((long)b * nt + j0 + tid) * D + (long)h * hd;
            float dl = 0.f;
            for (int e = 0; e < hd; ++e) dl = fmaf(dout[o + e], out[o + e], dl);
            dl_s[tid] = dl;
            lse_s[tid] = lse[bh * nt + j0 + tid];
        }
        __syncthreads();
        for (int jj = 0; jj < jb; ++jj) {
            const float* qj = q_s + jj * 64;
            const float* dj = do_s + jj * 64;
            float s = 0.f, dpv = 0.f;
#pragma unroll
            for (int pz = 0; pz < 8; ++pz)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s = fmaf(qj[8 * pz + e], (float)kk[pz][e], s);
                    dpv = fmaf(dj[8 * pz + e], (float)vv[pz][e], dpv);
                }
            const float p = live ? exp2f(s - lse_s[jj]) : 0.f;
            const uint32_t key = drop_rowkey(seed, sid, (uint64_t)(bh * nt + j0 + jj));
            const bool keep = drop_keep(drop_pair_bits(key, (uint32_t)t >> 1), t & 1, thr);
            const float pd = keep ? p * scale : 0.f;
            const float ds = p * ((keep ? dpv * scale : 0.f) - dl_s[jj]);
            const float dsk = ds * rs;                          // dq = sum_t ds K / sqrt(hd)
            const float dsq = ds * 0.69314718055994530942f;     // dK = ds q / sqrt(hd), and q_s carries log2(e) / sqrt(hd)
#pragma unroll
            for (int e = 0; e < 64; ++e) {
                dV[e] = fmaf(pd, dj[e], dV[e]);
                dK[e] = fmaf(dsq, qj[e], dK[e]);
            }
            dSs[jj * CA_KEYS + tid] = dsk;
        }
        __syncthreads();
        {
            const int d = tid & 63;
            for (int jj = tid >> 6; jj < jb; jj += 4) {
                const float* dsr = dSs + jj * CA_KEYS;
                float acc = 0.f;
#pragma unroll 8
                for (int tt = 0; tt < CA_KEYS; ++tt) acc = fmaf(dsr[tt], (float)Ks[tt * CA_KPITCH + d], acc);
                dq_part[((bh * nchunk + chunk) * nt + j0 + jj) * 64 + d] = acc;
            }
        }
    }
    if (live) {
        T* kr = dkv + ((long)b * Tn + t) * lddkv + 64 * h;
#pragma unroll
        for (int pz = 0; pz < 8; ++pz) {
            vec8 a, c;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                a[e] = (T)dK[8 * pz + e];
                c[e] = (T)dV[8 * pz + e];
            }
            *reinterpret_cast<vec8*>(kr + 8 * pz) = a;
            *reinterpret_cast<vec8*>(kr + Db + 8 * pz) = c;
        }
    }
}

// dq[b][j][h hd + d] = sum over the chunks, in chunk order, of part[b][h][chunk][j][d]
__global__ void __launch_bounds__(256) cross_attn_dq_reduce_kernel(const float* __restrict__ part, float* __restrict__ dq, int B, int nt, int H, int hd, int nchunk) {
    const int D = H * hd;
    const long n = (long)B * nt * D;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % D);
        const long bj = i / D;
        const int j = (int)(bj % nt);
        const long b = bj / nt;
        const int h = c / hd, d = c - h * hd;
        const float* p = part + (((b * H + h) * nchunk) * nt + j) * 64 + d;
        float acc = 0.f;
        for (int k = 0; k < nchunk; ++k) acc += p[(long)k * nt * 64];
        dq[i] = acc;
    }
}

struct Dims : PadDims {
    int F, D, He, Hd, FF, Le, Ld, nt, pe, dt;
    int Db, KVp, hd_d, Bb, T, nchunk;
    long M, M2;
};

int make_dims(const amds_barspoon_cfg* c, int Bb, int T, Dims* d) {
    AMDS_REQUIRE(c, "amds_barspoon_train: null config");
    AMDS_REQUIRE(c->n_feats > 0 && c->dim > 0 && c->enc_heads > 0 && c->dec_heads > 0 && c->ff > 0 && c->enc_layers >= 0 && c->enc_layers <= 1024 &&
                 c->dec_layers >= 0 && c->dec_layers <= 1024 && c->n_targets > 0, "amds_barspoon_train: bad config");
    AMDS_REQUIRE(c->dim % c->enc_heads == 0 && c->dim % c->dec_heads == 0, "amds_barspoon_train: d_model=%d has to be divisible by the head counts (%d, %d)", c->dim,
                 c->enc_heads, c->dec_heads);
    AMDS_REQUIRE(c->dim / c->enc_heads <= 64 && c->dim / c->dec_heads <= 64 && c->dim % 4 == 0, "amds_barspoon_train: needs head_dim <= 64 and d_model %% 4 == 0");
    AMDS_REQUIRE(c->n_targets <= 1024, "amds_barspoon_train: %d targets", c->n_targets);
    AMDS_REQUIRE(c->dtype == AMDS_F16 || c->dtype == AMDS_BF16, "amds_barspoon_train: the training step runs on bf16 or fp16 operands (cfg.dtype = AMDS_BF16 / AMDS_F16)");
    AMDS_REQUIRE(Bb > 0 && T > 0 && Bb <= 65535 && (long)Bb * c->dec_heads <= 65535, "amds_barspoon_train: bad shape bags=%d tiles=%d", Bb, T);
    d->F = c->n_feats; d->D = c->dim; d->He = c->enc_heads; d->Hd = c->dec_heads; d->FF = c->ff; d->Le = c->enc_layers; d->Ld = c->dec_layers;
    d->nt = c->n_targets; d->pe = c->positional_encoding != 0; d->dt = c->dtype;
    static_cast<PadDims&>(*d) = pad_dims(d->F, d->D, d->FF, d->He);
    d->Db = 64 * d->Hd; d->KVp = round_up(2 * d->Db, 256); d->hd_d = d->D / d->Hd;
    d->Bb = Bb; d->T = T; d->nchunk = (T + CA_KEYS - 1) / CA_KEYS;
    d->M = (long)Bb * T; d->M2 = (long)Bb * d->nt;
    AMDS_REQUIRE(d->M < (1L << 31) - 65536, "amds_barspoon_train: %ld tile rows do not fit the 32-bit row index", d->M);
    AMDS_REQUIRE(d->M2 * std::max(3 * d->D, d->FF) < (1L << 31), "amds_barspoon_train: %ld class-token rows are too many", d->M2);
    return AMDS_OK;
}

struct EncOff { size_t h1, mu1, rs1, qkv, att, lse, x_mid, h2, mu2, rs2, z, u; };
struct DecOff { size_t th1, mu1, rs1, tqkv, P, Pd, to, t_mid1, th2, mu2, rs2, tq, kv, clse, co, t_mid2, th3, mu3, rs3, tz, tu; };
struct SavedPlan {
    size_t a, zp, x0, x_bytes, xe16, y, tok0, tok_bytes, ty, total;
    std::vector<EncOff> enc;
    std::vector<DecOff> dec;
};

void plan_saved(const Dims& d, SavedPlan* p) {
    Arena ar;
    const size_t M = d.M, M2 = d.M2, D = d.D;
    p->a = ar.take(M * d.Fp * 2);
    p->zp = ar.take(M * d.Dp * 2);
    p->x_bytes = align256(M * d.Dp * 4);
    p->x0 = ar.take(p->x_bytes * (d.Le + 1));
    p->xe16 = ar.take(M * d.Dp * 2);
    p->y = ar.take(M * d.Dp * 4);                                   // scratch of the forward's `x + drop(y)` sites
    p->enc.resize(d.Le);
    for (int l = 0; l < d.Le; ++l) {
        EncOff& o = p->enc[l];
        o.h1 = ar.take(M * d.Dp * 2); o.mu1 = ar.take(M * 4); o.rs1 = ar.take(M * 4);
        o.qkv = ar.take(M * 3 * d.Da * 2); o.att = ar.take(M * d.Da * 2); o.lse = ar.take((size_t)d.Bb * d.Ha * d.T * 4);
        o.x_mid = ar.take(M * d.Dp * 4);
        o.h2 = ar.take(M * d.Dp * 2); o.mu2 = ar.take(M * 4); o.rs2 = ar.take(M * 4);
        o.z = ar.take(M * d.FFp * 2); o.u = ar.take(M * d.FFp * 2);
    }
    p->tok_bytes = align256(M2 * D * 4);
    p->tok0 = ar.take(p->tok_bytes * (d.Ld + 1));
    p->ty = ar.take(M2 * D * 4);
    p->dec.resize(d.Ld);
    const size_t pp = (size_t)d.Bb * d.Hd * d.nt * d.nt * 4;
    for (int l = 0; l < d.Ld; ++l) {
        DecOff& o = p->dec[l];
        o.th1 = ar.take(M2 * D * 4); o.mu1 = ar.take(M2 * 4); o.rs1 = ar.take(M2 * 4);
        o.tqkv = ar.take(M2 * 3 * D * 4); o.P = ar.take(pp); o.Pd = ar.take(pp); o.to = ar.take(M2 * D * 4); o.t_mid1 = ar.take(M2 * D * 4);
        o.th2 = ar.take(M2 * D * 4); o.mu2 = ar.take(M2 * 4); o.rs2 = ar.take(M2 * 4);
        o.tq = ar.take(M2 * D * 4); o.kv = ar.take(M * 2 * d.Db * 2); o.clse = ar.take((size_t)d.Bb * d.Hd * d.nt * 4); o.co = ar.take(M2 * D * 4);
        o.t_mid2 = ar.take(M2 * D * 4);
        o.th3 = ar.take(M2 * D * 4); o.mu3 = ar.take(M2 * 4); o.rs3 = ar.take(M2 * 4);
        o.tz = ar.take(M2 * (size_t)d.FF * 4); o.tu = ar.take(M2 * (size_t)d.FF * 4);
    }
    p->total = ar.off;
}

struct WsPlan {
    size_t dx, dh, g16, du, dz, datt, dqkv, dqs, dkv, part, cs, lnb, dt, dy, d1, d2, dth, dP, dtq, dqp, total;
    size_t cs_bytes, lnb_bytes, dqp_bytes;
};

void plan_ws(const Dims& d, int split_k, WsPlan* p) {
    Arena ar;
    const size_t M = d.M, M2 = d.M2, D = d.D;
    p->dx = ar.take(M * d.Dp * 4);
    p->dh = ar.take(M * d.Dp * 4);
    p->g16 = ar.take(M * d.Dp * 2);
    p->du = ar.take(M * d.FFp * 2);
    p->dz = ar.take(M * d.FFp * 2);
    p->datt = ar.take(M * d.Da * 2);
    p->dqkv = ar.take(M * 3 * d.Da * 2);
    p->dqs = ar.take((size_t)d.Bb * d.Ha * d.T * 4);
    p->dkv = ar.take(M * d.KVp * 2);
    const size_t nk = std::max(std::max(std::max((size_t)3 * d.Da * d.Dp, (size_t)d.FFp * d.Dp), std::max((size_t)d.Dp * d.Da, (size_t)d.Dp * d.Fp)), (size_t)d.KVp * d.Dp);
    p->part = ar.take(nk * split_k * 4);
    size_t cs = amds_colsum_workspace_bytes(split_k, (int)std::min<size_t>(nk, 0x7fffffff));
    const int wide[] = {d.Dp, d.FFp, 3 * d.Da, d.KVp};
    for (int w : wide) cs = std::max(cs, amds_colsum_workspace_bytes((int)d.M, w));
    const int narrow[] = {d.D, d.FF, 3 * d.D};
    for (int w : narrow) cs = std::max(cs, amds_colsum_workspace_bytes((int)d.M2, w));
    cs = std::max(cs, amds_colsum_workspace_bytes(d.Bb, (int)std::min<long>((long)d.nt * d.D, 0x7fffffff)));
    p->cs_bytes = std::max<size_t>(cs, 4);
    p->cs = ar.take(p->cs_bytes);
    p->lnb_bytes = std::max<size_t>(std::max(amds_layernorm_bwd_workspace_bytes((int)d.M, d.D), amds_layernorm_bwd_workspace_bytes((int)d.M2, d.D)), 4);
    p->lnb = ar.take(p->lnb_bytes);
    p->dt = ar.take(M2 * D * 4);
    p->dy = ar.take(M2 * D * 4);
    p->d1 = ar.take(M2 * (size_t)std::max(d.FF, 3 * d.D) * 4);
    p->d2 = ar.take(M2 * (size_t)std::max(d.FF, d.D) * 4);
    p->dth = ar.take(M2 * D * 4);
    p->dP = ar.take((size_t)d.Bb * d.Hd * d.nt * d.nt * 4);
    p->dtq = ar.take(M2 * D * 4);
    p->dqp_bytes = std::max<size_t>(amds_cross_attention_bwd_workspace_bytes(d.Bb, d.T, d.nt, d.Hd), 4);
    p->dqp = ar.take(p->dqp_bytes);
    p->total = ar.off;
}

bool weights_ok(const Dims& d, const amds_barspoon_train_weights* tw, bool backward) {
    const amds_barspoon_weights& w = tw->w;
    if (!(w.proj_w && w.proj_b && w.class_tokens && w.head_w_host && w.head_b_host && w.n_out_host && (d.Le == 0 || w.enc_layers_host) &&
          (d.Ld == 0 || (w.dec_layers_host && tw->ca_kv_wt_host))))
        return false;
    for (int l = 0; l < d.Le; ++l) {
        const amds_mil_vit_layer& L = w.enc_layers_host[l];
        if (!enc_layer_complete(L) || (backward && !enc_layer_has_transposes(L))) return false;
    }
    for (int l = 0; l < d.Ld; ++l) {
        const amds_barspoon_dec_layer& L = w.dec_layers_host[l];
        if (!(L.ln1_w && L.ln1_b && L.sa_in_w && L.sa_in_b && L.sa_out_w && L.sa_out_b && L.ln2_w && L.ln2_b && L.ca_q_w && L.ca_q_b && L.ca_kv_w && L.ca_kv_b &&
              L.ca_out_w && L.ca_out_b && L.ln3_w && L.ln3_b && L.fc1_w && L.fc1_b && L.fc2_w && L.fc2_b && tw->ca_kv_wt_host[l]))
            return false;
    }
    for (int j = 0; j < d.nt; ++j)
        if (!(w.n_out_host[j] > 0 && w.head_w_host[j] && w.head_b_host[j])) return false;
    return true;
}

int ca_fwd(const float* q, const void* kv, float* out, float* lse, int B, int T, int nt, int H, int hd, int dt, float p, uint64_t seed, uint32_t sid, hipStream_t st) {
    const DropParams dp(p);
    const long items = (long)B * nt * H;
    const unsigned grid = (unsigned)((items + 3) / 4);
    dispatch_16(dt, [&](auto t) {
        typedef AMDS_TAG_T(t) Tt;
        hipLaunchKernelGGL((cross_attn_fwd_train_kernel<Tt>), dim3(grid), dim3(256), 0, st, q, (const Tt*)kv, out, lse, B, T, nt, H, hd, H * hd, 64 * H, seed, sid, dp.thr,
                           dp.scale);
    });
    AMDS_LAUNCH_CHECK("cross_attn_fwd_train_kernel");
    return AMDS_OK;
}

int ca_bwd(const float* q, const void* kv, const float* out, const float* dout, const float* lse, float* dq, void* dkv, long ld_dkv, int B, int T, int nt, int H, int hd,
           int dt, float p, uint64_t seed, uint32_t sid, float* part, hipStream_t st) {
    const DropParams dp(p);
    const int nchunk = (T + CA_KEYS - 1) / CA_KEYS;
    dispatch_16(dt, [&](auto t) {
        typedef AMDS_TAG_T(t) Tt;
        hipLaunchKernelGGL((cross_attn_bwd_train_kernel<Tt>), dim3(nchunk, H, B), dim3(256), 0, st, q, (const Tt*)kv, out, dout, lse, (Tt*)dkv, ld_dkv, part, T, nt, H, hd,
                           H * hd, 64 * H, nchunk, seed, sid, dp.thr, dp.scale);
    });
    AMDS_LAUNCH_CHECK("cross_attn_bwd_train_kernel");
    const long n = (long)B * nt * H * hd;
    hipLaunchKernelGGL(cross_attn_dq_reduce_kernel, dim3((unsigned)std::min<long>(4096, (n + 255) / 256)), dim3(256), 0, st, part, dq, B, nt, H, hd, nchunk);
    AMDS_LAUNCH_CHECK("cross_attn_dq_reduce_kernel");
    return AMDS_OK;
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" int amds_cross_attention_fwd_train(const float* q, const void* kv, float* out, float* lse, int B, int T, int nt, int H, int hd, int dtype, float p,
                                              uint64_t seed, uint32_t stream_id, void* stream) {
    AMDS_REQUIRE(q && kv && out && lse, "amds_cross_attention_fwd_train: null pointer");
    AMDS_REQUIRE(B > 0 && T > 0 && nt > 0 && H > 0 && hd > 0 && hd <= 64 && p >= 0.f && p < 1.f && (long)B * T < (1L << 31) && (long)B * nt * H < (1L << 31),
                 "amds_cross_attention_fwd_train: bad arguments B=%d T=%d nt=%d H=%d hd=%d p=%f", B, T, nt, H, hd, (double)p);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "amds_cross_attention_fwd_train: dtype must be f16 or bf16");
    AMDS_REQUIRE(((uintptr_t)kv & 15) == 0, "amds_cross_attention_fwd_train: kv must be 16-byte aligned");
    return ca_fwd(q, kv, out, lse, B, T, nt, H, hd, dtype, p, seed, stream_id, (hipStream_t)stream);
}

extern "C" size_t amds_cross_attention_bwd_workspace_bytes(int B, int T, int nt, int H) {
    if (B <= 0 || T <= 0 || nt <= 0 || H <= 0) return 0;
    return (size_t)B * H * ((T + CA_KEYS - 1) / CA_KEYS) * nt * 64 * 4;
}

extern "C" int amds_cross_attention_bwd_train(const float* q, const void* kv, const float* out, const float* dout, const float* lse, float* dq, void* dkv, long ld_dkv,
                                              int B, int T, int nt, int H, int hd, int dtype, float p, uint64_t seed, uint32_t stream_id, void* ws, size_t ws_bytes,
                                              void* stream) {
    AMDS_REQUIRE(q && kv && out && dout && lse && dq && dkv && ws, "amds_cross_attention_bwd_train: null pointer");
    AMDS_REQUIRE(B > 0 && T > 0 && nt > 0 && H > 0 && hd > 0 && hd <= 64 && p >= 0.f && p < 1.f && B <= 65535 && H <= 65535 && (long)B * T < (1L << 31),
                 "amds_cross_attention_bwd_train: bad arguments B=%d T=%d nt=%d H=%d hd=%d p=%f", B, T, nt, H, hd, (double)p);
    AMDS_REQUIRE(dtype == AMDS_F16 || dtype == AMDS_BF16, "amds_cross_attention_bwd_train: dtype must be f16 or bf16");
    AMDS_REQUIRE(ld_dkv >= 128L * H && ld_dkv % 8 == 0 && (((uintptr_t)kv | (uintptr_t)dkv) & 15) == 0, "amds_cross_attention_bwd_train: bad dkv pitch or alignment");
    const size_t need = amds_cross_attention_bwd_workspace_bytes(B, T, nt, H);
    if (ws_bytes < need) {
        set_error("amds_cross_attention_bwd_train: workspace %zu < required %zu bytes", ws_bytes, need);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 15) == 0, "amds_cross_attention_bwd_train: workspace must be 16-byte aligned");
    return ca_bwd(q, kv, out, dout, lse, dq, dkv, ld_dkv, B, T, nt, H, hd, dtype, p, seed, stream_id, reinterpret_cast<float*>(ws), (hipStream_t)stream);
}

extern "C" size_t amds_barspoon_train_saved_bytes(const amds_barspoon_cfg* cfg_host, int n_bags, int n_tiles) {
    Dims d;
    if (make_dims(cfg_host, n_bags, n_tiles, &d) != AMDS_OK) return 0;
    SavedPlan p;
    plan_saved(d, &p);
    return p.total;
}

extern "C" size_t amds_barspoon_train_workspace_bytes(const amds_barspoon_cfg* cfg_host, int n_bags, int n_tiles, int split_k) {
    Dims d;
    if (make_dims(cfg_host, n_bags, n_tiles, &d) != AMDS_OK) return 0;
    if (split_k <= 0 || split_k > 1024) { set_error("amds_barspoon_train: bad split_k=%d", split_k); return 0; }
    WsPlan p;
    plan_ws(d, split_k, &p);
    return p.total;
}

extern "C" int amds_barspoon_train_forward(const amds_barspoon_cfg* cfg_host, const amds_barspoon_train_weights* w_host, const void* bags, int bags_dtype,
                                           const float* positions, const amds_barspoon_dropout* drop_host, float* logits, int n_bags, int n_tiles, void* saved,
                                           size_t saved_bytes, void* stream) {
    AMDS_REQUIRE(cfg_host && w_host && bags && logits && saved && drop_host, "amds_barspoon_train_forward: null pointer");
    Dims d;
    RC(make_dims(cfg_host, n_bags, n_tiles, &d));
    const amds_barspoon_weights& w = w_host->w;
    AMDS_REQUIRE(weights_ok(d, w_host, false), "amds_barspoon_train_forward: incomplete weights");
    AMDS_REQUIRE(!d.pe || (positions && w.pe_div), "amds_barspoon_train_forward: positional_encoding=True needs tile positions");
    AMDS_REQUIRE(bags_dtype == AMDS_F32 || bags_dtype == AMDS_F16 || bags_dtype == AMDS_BF16, "amds_barspoon_train_forward: bad bags dtype %d", bags_dtype);
    const float p = drop_host->p;
    AMDS_REQUIRE(p >= 0.f && p < 1.f, "amds_barspoon_train_forward: dropout rate %f is outside [0, 1)", (double)p);
    SavedPlan sp;
    plan_saved(d, &sp);
    if (saved_bytes < sp.total) {
        set_error("amds_barspoon_train_forward: saved-activation arena %zu < required %zu bytes", saved_bytes, sp.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)saved & 255) == 0, "amds_barspoon_train_forward: arena must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* sv = reinterpret_cast<char*>(saved);
    const uint64_t seed = drop_host->seed;
    const int dt = d.dt, Dp = d.Dp, Da = d.Da, FFp = d.FFp, Fp = d.Fp, D = d.D, Bb = d.Bb, T = d.T, Ha = d.Ha, nt = d.nt, Hd = d.Hd, hd = d.hd_d, FF = d.FF;
    const long M = d.M, M2 = d.M2;
    auto gemm = [&](const void* A, long lda, const void* W, long ldw, long Mr, int N, int K, int epi, void* out, long ldo, const float* bias) -> int {
        return gemm_train(dt, A, lda, W, ldw, Mr, N, K, epi, out, ldo, bias, stream);
    };

    // ---- projector: Linear + ReLU (:171), positional encodings (:173-186); no dropout
    void* a = sv + sp.a;
    if (bags_dtype == dt && Fp == d.F) AMDS_HIP(hipMemcpyAsync(a, bags, (size_t)M * Fp * 2, hipMemcpyDeviceToDevice, st));
    else RC(stage_rows_dt(bags, bags_dtype, d.F, a, dt, Fp, M, d.F, stream));
    void* zp = sv + sp.zp;
    float* x = reinterpret_cast<float*>(sv + sp.x0);
    float* y = reinterpret_cast<float*>(sv + sp.y);
    RC(gemm(a, Fp, w.proj_w, Fp, M, Dp, Fp, AMDS_EPI_BIAS, zp, Dp, w.proj_b));
    RC(amds_relu_dropout_fwd(zp, x, M * Dp, dt, AMDS_F32, 0.f, 0, 0, stream));
    if (d.pe) RC(pos_encoding_add(x, Dp, D, positions, w.pe_div, M, st));

    // ---- encoder (:188): x += drop(SA(LN1(x)));  x += drop(W2 drop(relu(W1 LN2(x))))
    for (int l = 0; l < d.Le; ++l) {
        const amds_mil_vit_layer& L = w.enc_layers_host[l];
        const EncOff& o = sp.enc[l];
        float* x_in = reinterpret_cast<float*>(sv + sp.x0 + (size_t)l * sp.x_bytes);
        float* x_out = reinterpret_cast<float*>(sv + sp.x0 + (size_t)(l + 1) * sp.x_bytes);
        float* x_mid = reinterpret_cast<float*>(sv + o.x_mid);
        void *h1 = sv + o.h1, *h2 = sv + o.h2, *qkv = sv + o.qkv, *att = sv + o.att, *z = sv + o.z, *u = sv + o.u;
        float* lse = reinterpret_cast<float*>(sv + o.lse);
        const uint32_t sid = 10u * l;
        if (Dp != D) {      // LayerNorm writes the first D columns only
            AMDS_HIP(hipMemsetAsync(h1, 0, (size_t)M * Dp * 2, st));
            AMDS_HIP(hipMemsetAsync(h2, 0, (size_t)M * Dp * 2, st));
        }
        // (p = 0: the LayerNorm kernel also writes x_mid = x_in, which the out-projection's residual epilogue then updates in place)
        RC(amds_layernorm_train_copy(x_in, Dp, L.ln1_w, L.ln1_b, h1, Dp, reinterpret_cast<float*>(sv + o.mu1), reinterpret_cast<float*>(sv + o.rs1), (int)M, D, 1e-5f, dt,
                                     p > 0.f ? nullptr : x_mid, Dp, Dp, stream));
        RC(gemm(h1, Dp, L.in_w, Dp, M, 3 * Da, Dp, AMDS_EPI_BIAS, qkv, 3 * Da, L.in_b));
        RC(amds_attention_fwd_train(qkv, att, lse, Bb, T, Ha, dt, p, seed, sid + 1, stream));
        if (p > 0.f) {
            RC(gemm(att, Da, L.out_w, Da, M, Dp, Da, AMDS_EPI_BIAS_F32, y, Dp, L.out_b));
            RC(amds_dropout_add(y, Dp, x_in, Dp, x_mid, Dp, M, Dp, p, seed, sid + 4, stream));
        } else {
            RC(gemm(att, Da, L.out_w, Da, M, Dp, Da, AMDS_EPI_RESIDUAL, x_mid, Dp, L.out_b));
        }
        RC(amds_layernorm_train_copy(x_mid, Dp, L.ln2_w, L.ln2_b, h2, Dp, reinterpret_cast<float*>(sv + o.mu2), reinterpret_cast<float*>(sv + o.rs2), (int)M, D, 1e-5f, dt,
                                     p > 0.f ? nullptr : x_out, Dp, Dp, stream));
        RC(gemm(h2, Dp, L.fc1_w, Dp, M, FFp, Dp, AMDS_EPI_BIAS, z, FFp, L.fc1_b));
        RC(amds_relu_dropout_fwd(z, u, M * FFp, dt, dt, p, seed, sid + 2, stream));
        if (p > 0.f) {
            RC(gemm(u, FFp, L.fc2_w, FFp, M, Dp, FFp, AMDS_EPI_BIAS_F32, y, Dp, L.fc2_b));
            RC(amds_dropout_add(y, Dp, x_mid, Dp, x_out, Dp, M, Dp, p, seed, sid + 3, stream));
        } else {
            RC(gemm(u, FFp, L.fc2_w, FFp, M, Dp, FFp, AMDS_EPI_RESIDUAL, x_out, Dp, L.fc2_b));
        }
    }
    // the encoder's output as the 16-bit A operand of every decoder layer's K | V projection (no final norm: nn.TransformerEncoder(norm=None))
    const float* x_enc = reinterpret_cast<const float*>(sv + sp.x0 + (size_t)d.Le * sp.x_bytes);
    void* xe16 = sv + sp.xe16;
    if (d.Ld > 0) RC(amds_cast_pad(x_enc, Dp, xe16, Dp, (int)M, Dp, dt, stream));

    // ---- decoder (:190-193): the class tokens, exact fp32
    float* ty = reinterpret_cast<float*>(sv + sp.ty);
    RC(broadcast_rows(w.class_tokens, reinterpret_cast<float*>(sv + sp.tok0), (long)nt * D, M2 * D, st));
    const float sa_scale = (float)(1.0 / sqrt((double)hd));
    for (int l = 0; l < d.Ld; ++l) {
        const amds_barspoon_dec_layer& L = w.dec_layers_host[l];
        const DecOff& o = sp.dec[l];
        const uint32_t sid = 5000u + 10u * l;
        float* t_in = reinterpret_cast<float*>(sv + sp.tok0 + (size_t)l * sp.tok_bytes);
        float* t_out = reinterpret_cast<float*>(sv + sp.tok0 + (size_t)(l + 1) * sp.tok_bytes);
        auto F = [&](size_t off) { return reinterpret_cast<float*>(sv + off); };
        float *th1 = F(o.th1), *tqkv = F(o.tqkv), *P = F(o.P), *Pd = F(o.Pd), *to = F(o.to), *t_mid1 = F(o.t_mid1), *th2 = F(o.th2), *tq = F(o.tq), *co = F(o.co);
        float *t_mid2 = F(o.t_mid2), *th3 = F(o.th3), *tz = F(o.tz), *tu = F(o.tu), *clse = F(o.clse);
        void* kv = sv + o.kv;
        // t += drop(SA(LN1(t))): self-attention among the nt class tokens of a bag, dropout on its probabilities
        RC(amds_layernorm_train(t_in, D, L.ln1_w, L.ln1_b, th1, D, F(o.mu1), F(o.rs1), (int)M2, D, 1e-5f, AMDS_F32, stream));
        RC(lin(th1, L.sa_in_w, L.sa_in_b, tqkv, M2, 3 * D, D, stream));
        RC(bg(tqkv, 3 * D, (long)nt * 3 * D, hd, tqkv + D, 3 * D, (long)nt * 3 * D, hd, 1, P, nt, (long)Hd * nt * nt, (long)nt * nt, Bb, Hd, nt, nt, hd, sa_scale, nullptr, 0,
              stream));
        RC(amds_softmax_rows(P, (long)Bb * Hd * nt, nt, stream));
        RC(amds_attention_dropout_rows(P, Pd, (long)Bb * Hd * nt, nt, p, seed, sid + 1, stream));
        RC(bg(Pd, nt, (long)Hd * nt * nt, (long)nt * nt, tqkv + 2 * D, 3 * D, (long)nt * 3 * D, hd, 0, to, D, (long)nt * D, hd, Bb, Hd, nt, hd, nt, 1.0f, nullptr, 0, stream));
        RC(lin(to, L.sa_out_w, L.sa_out_b, ty, M2, D, D, stream));
        RC(amds_dropout_add(ty, D, t_in, D, t_mid1, D, M2, D, p, seed, sid + 2, stream));
        // t += drop(MHA(LN2(t), memory)): queries from the class tokens, keys / values from the tile tokens
        RC(amds_layernorm_train(t_mid1, D, L.ln2_w, L.ln2_b, th2, D, F(o.mu2), F(o.rs2), (int)M2, D, 1e-5f, AMDS_F32, stream));
        RC(lin(th2, L.ca_q_w, L.ca_q_b, tq, M2, D, D, stream));
        RC(gemm(xe16, Dp, L.ca_kv_w, Dp, M, 2 * d.Db, Dp, AMDS_EPI_BIAS, kv, 2 * d.Db, L.ca_kv_b));
        RC(ca_fwd(tq, kv, co, clse, Bb, T, nt, Hd, hd, dt, p, seed, sid + 3, st));
        RC(lin(co, L.ca_out_w, L.ca_out_b, ty, M2, D, D, stream));
        RC(amds_dropout_add(ty, D, t_mid1, D, t_mid2, D, M2, D, p, seed, sid + 4, stream));
        // t += drop(W2 drop(relu(W1 LN3(t))))
        RC(amds_layernorm_train(t_mid2, D, L.ln3_w, L.ln3_b, th3, D, F(o.mu3), F(o.rs3), (int)M2, D, 1e-5f, AMDS_F32, stream));
        RC(lin(th3, L.fc1_w, L.fc1_b, tz, M2, FF, D, stream));
        RC(amds_relu_dropout_fwd(tz, tu, M2 * FF, AMDS_F32, AMDS_F32, p, seed, sid + 5, stream));
        RC(lin(tu, L.fc2_w, L.fc2_b, ty, M2, D, FF, stream));
        RC(amds_dropout_add(ty, D, t_mid2, D, t_out, D, M2, D, p, seed, sid + 6, stream));
    }
    // ---- heads (:196-203): target j reads its own class-token row of every bag
    const float* tok = reinterpret_cast<const float*>(sv + sp.tok0 + (size_t)d.Ld * sp.tok_bytes);
    int total_out = 0;
    for (int j = 0; j < nt; ++j) total_out += w.n_out_host[j];
    int col = 0;
    for (int j = 0; j < nt; ++j) {
        RC(bg(tok + (size_t)j * D, nt * D, 0, 0, w.head_w_host[j], D, 0, 0, 1, logits + col, total_out, 0, 0, 1, 1, Bb, w.n_out_host[j], D, 1.0f, w.head_b_host[j], 0, stream));
        col += w.n_out_host[j];
    }
    return AMDS_OK;
}

extern "C" int amds_barspoon_train_backward(const amds_barspoon_cfg* cfg_host, const amds_barspoon_train_weights* w_host, const float* dlogits,
                                            const amds_barspoon_dropout* drop_host, int n_bags, int n_tiles, const void* saved, size_t saved_bytes,
                                            const amds_barspoon_grads* grads_host, int split_k, void* ws, size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(cfg_host && w_host && dlogits && saved && drop_host && ws && grads_host, "amds_barspoon_train_backward: null pointer");
    AMDS_REQUIRE(split_k > 0 && split_k <= 1024, "amds_barspoon_train_backward: bad split_k=%d", split_k);
    Dims d;
    RC(make_dims(cfg_host, n_bags, n_tiles, &d));
    const amds_barspoon_weights& w = w_host->w;
    AMDS_REQUIRE(weights_ok(d, w_host, true), "amds_barspoon_train_backward: incomplete weights (the training pack carries the transposed 16-bit matrices)");
    const float p = drop_host->p;
    AMDS_REQUIRE(p >= 0.f && p < 1.f, "amds_barspoon_train_backward: dropout rate %f is outside [0, 1)", (double)p);
    const amds_barspoon_grads& G = *grads_host;
    AMDS_REQUIRE(G.proj_w && G.proj_b && G.class_tokens && G.head_w_host && G.head_b_host && (d.Le == 0 || G.enc_layers_host) && (d.Ld == 0 || G.dec_layers_host),
                 "amds_barspoon_train_backward: incomplete gradient buffers");
    for (int l = 0; l < d.Le; ++l) {
        const amds_mil_vit_layer_grads& g = G.enc_layers_host[l];
        AMDS_REQUIRE(g.ln1_w && g.ln1_b && g.in_w && g.in_b && g.out_w && g.out_b && g.ln2_w && g.ln2_b && g.fc1_w && g.fc1_b && g.fc2_w && g.fc2_b,
                     "amds_barspoon_train_backward: incomplete gradient buffers of encoder layer %d", l);
    }
    for (int l = 0; l < d.Ld; ++l) {
        const amds_barspoon_dec_layer_grads& g = G.dec_layers_host[l];
        AMDS_REQUIRE(g.ln1_w && g.ln1_b && g.sa_in_w && g.sa_in_b && g.sa_out_w && g.sa_out_b && g.ln2_w && g.ln2_b && g.ca_q_w && g.ca_q_b && g.ca_kv_w && g.ca_kv_b &&
                     g.ca_out_w && g.ca_out_b && g.ln3_w && g.ln3_b && g.fc1_w && g.fc1_b && g.fc2_w && g.fc2_b,
                     "amds_barspoon_train_backward: incomplete gradient buffers of decoder layer %d", l);
    }
    for (int j = 0; j < d.nt; ++j) AMDS_REQUIRE(G.head_w_host[j] && G.head_b_host[j], "amds_barspoon_train_backward: gradient buffers of head %d missing", j);
    SavedPlan sp;
    plan_saved(d, &sp);
    WsPlan wp;
    plan_ws(d, split_k, &wp);
    if (saved_bytes < sp.total || ws_bytes < wp.total) {
        set_error("amds_barspoon_train_backward: arena %zu / workspace %zu < required %zu / %zu bytes", saved_bytes, ws_bytes, sp.total, wp.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE((((uintptr_t)saved | (uintptr_t)ws) & 255) == 0, "amds_barspoon_train_backward: arena and workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const char* sv = reinterpret_cast<const char*>(saved);
    char* wk = reinterpret_cast<char*>(ws);
    const uint64_t seed = drop_host->seed;
    const int dt = d.dt, Dp = d.Dp, Da = d.Da, FFp = d.FFp, Fp = d.Fp, D = d.D, Bb = d.Bb, T = d.T, Ha = d.Ha, nt = d.nt, Hd = d.Hd, hd = d.hd_d, FF = d.FF, KVp = d.KVp;
    const long M = d.M, M2 = d.M2;
    auto gemm = [&](const void* A, long lda, const void* W, long ldw, long Mr, int N, int K, int epi, void* out, long ldo, const float* bias) -> int {
        return gemm_train(dt, A, lda, W, ldw, Mr, N, K, epi, out, ldo, bias, stream);
    };
    auto Wf = [&](size_t off) { return reinterpret_cast<float*>(wk + off); };
    auto Sf = [&](size_t off) { return reinterpret_cast<const float*>(sv + off); };
    float *dx = Wf(wp.dx), *dh = Wf(wp.dh), *part = Wf(wp.part), *dqs = Wf(wp.dqs);
    void *g16 = wk + wp.g16, *du = wk + wp.du, *dz = wk + wp.dz, *datt = wk + wp.datt, *dqkv = wk + wp.dqkv, *dkv = wk + wp.dkv, *cs = wk + wp.cs, *lnb = wk + wp.lnb;
    float *dtk = Wf(wp.dt), *dy = Wf(wp.dy), *d1 = Wf(wp.d1), *d2 = Wf(wp.d2), *dth = Wf(wp.dth), *dP = Wf(wp.dP), *dtq = Wf(wp.dtq), *dqp = Wf(wp.dqp);
    auto colsum = [&](const void* xx, long ld, float* out, long rows, int cols, int dtype) -> int {
        return amds_colsum(xx, ld, out, (int)rows, cols, dtype, 0, cs, wp.cs_bytes, stream);
    };
    // dW[N][K] = dy^T x over the tile rows: split_k fp32 partials, summed in a fixed order
    auto wgrad = [&](const void* dyy, long ld_dy, const void* xx, long ld_x, int Nn, int Kk, float* out) -> int {
        RC(amds_wgrad_tn(dyy, ld_dy, xx, ld_x, M, Nn, Kk, split_k, dt, part, stream));
        return amds_colsum(part, (long)Nn * Kk, out, split_k, Nn * Kk, AMDS_F32, 0, cs, wp.cs_bytes, stream);
    };
    auto ln_bwd32 = [&](const float* dyy, const float* xx, const float* mu, const float* rs, const float* gamma, float* dxo, float* dgamma, float* dbeta) -> int {
        return amds_layernorm_bwd(dyy, D, xx, D, mu, rs, gamma, dxo, D, 1, dgamma, dbeta, 0, (int)M2, D, lnb, wp.lnb_bytes, stream);
    };

    // ---- heads (:196-203)
    const float* tok = Sf(sp.tok0 + (size_t)d.Ld * sp.tok_bytes);
    int total_out = 0;
    for (int j = 0; j < nt; ++j) total_out += w.n_out_host[j];
    int col = 0;
    for (int j = 0; j < nt; ++j) {
        const int no = w.n_out_host[j];
        RC(bg(dlogits + col, total_out, 0, 0, tok + (size_t)j * D, nt * D, 0, 0, 2, G.head_w_host[j], D, 0, 0, 1, 1, no, D, Bb, 1.0f, nullptr, 0, stream));      // dW = dlogits^T t
        RC(colsum(dlogits + col, total_out, G.head_b_host[j], Bb, no, AMDS_F32));
        RC(bg(dlogits + col, total_out, 0, 0, w.head_w_host[j], D, 0, 0, 0, dtk + (size_t)j * D, nt * D, 0, 0, 1, 1, Bb, D, no, 1.0f, nullptr, 0, stream));      // dt = dlogits W
        col += no;
    }

    // ---- decoder (:190-193), exact fp32; the gradient of the encoder's output accumulates in dx (fp32) over the layers' K | V projections
    AMDS_HIP(hipMemsetAsync(dx, 0, (size_t)M * Dp * 4, st));
    if (d.Ld > 0 && KVp != 2 * d.Db) AMDS_HIP(hipMemsetAsync(dkv, 0, (size_t)M * KVp * 2, st));       // the kernel writes the first 2 Db columns only
    const float sa_scale = (float)(1.0 / sqrt((double)hd));
    for (int l = d.Ld - 1; l >= 0; --l) {
        const amds_barspoon_dec_layer& L = w.dec_layers_host[l];
        const amds_barspoon_dec_layer_grads& g = G.dec_layers_host[l];
        const DecOff& o = sp.dec[l];
        const uint32_t sid = 5000u + 10u * l;
        const float* t_in = Sf(sp.tok0 + (size_t)l * sp.tok_bytes);
        const float *th1 = Sf(o.th1), *tqkv = Sf(o.tqkv), *P = Sf(o.P), *Pd = Sf(o.Pd), *to = Sf(o.to), *t_mid1 = Sf(o.t_mid1), *th2 = Sf(o.th2), *tq = Sf(o.tq), *co = Sf(o.co);
        const float *t_mid2 = Sf(o.t_mid2), *th3 = Sf(o.th3), *tz = Sf(o.tz), *tu = Sf(o.tu), *clse = Sf(o.clse);
        const void* kv = sv + o.kv;
        // feed-forward: t_out = t_mid2 + drop6(W2 drop5(relu(W1 LN3(t_mid2))))
        RC(amds_dropout_cast_bwd(dtk, D, dy, D, M2, D, AMDS_F32, p, seed, sid + 6, stream));
        RC(lin_dw(dy, tu, g.fc2_w, M2, D, FF, stream));
        RC(colsum(dy, D, g.fc2_b, M2, D, AMDS_F32));
        RC(lin_dx(dy, L.fc2_w, d1, M2, D, FF, stream));                                                // d(tu) [M2][FF]
        RC(amds_relu_dropout_bwd(tz, d1, d2, M2 * FF, AMDS_F32, AMDS_F32, AMDS_F32, p, seed, sid + 5, stream));   // d(tz)
        RC(lin_dw(d2, th3, g.fc1_w, M2, FF, D, stream));
        RC(colsum(d2, FF, g.fc1_b, M2, FF, AMDS_F32));
        RC(lin_dx(d2, L.fc1_w, dth, M2, FF, D, stream));
        RC(ln_bwd32(dth, t_mid2, Sf(o.mu3), Sf(o.rs3), L.ln3_w, dtk, g.ln3_w, g.ln3_b));
        // cross-attention: t_mid2 = t_mid1 + drop4(Wo MHA(Wq LN2(t_mid1), K | V of the tiles))
        RC(amds_dropout_cast_bwd(dtk, D, dy, D, M2, D, AMDS_F32, p, seed, sid + 4, stream));
        RC(lin_dw(dy, co, g.ca_out_w, M2, D, D, stream));
        RC(colsum(dy, D, g.ca_out_b, M2, D, AMDS_F32));
        RC(lin_dx(dy, L.ca_out_w, d2, M2, D, D, stream));                                              // d(co)
        RC(ca_bwd(tq, kv, co, d2, clse, dtq, dkv, KVp, Bb, T, nt, Hd, hd, dt, p, seed, sid + 3, dqp, st));
        RC(wgrad(dkv, KVp, sv + sp.xe16, Dp, KVp, Dp, g.ca_kv_w));
        RC(colsum(dkv, KVp, g.ca_kv_b, M, KVp, dt));
        RC(gemm(dkv, KVp, w_host->ca_kv_wt_host[l], KVp, M, Dp, KVp, AMDS_EPI_RESIDUAL, dx, Dp, nullptr));     // d(x_enc) += dK|dV W_kv
        RC(lin_dw(dtq, th2, g.ca_q_w, M2, D, D, stream));
        RC(colsum(dtq, D, g.ca_q_b, M2, D, AMDS_F32));
        RC(lin_dx(dtq, L.ca_q_w, dth, M2, D, D, stream));
        RC(ln_bwd32(dth, t_mid1, Sf(o.mu2), Sf(o.rs2), L.ln2_w, dtk, g.ln2_w, g.ln2_b));
        // self-attention: t_mid1 = t_in + drop2(Wo (drop1(P) V)),  P = softmax(Q K^T / sqrt(hd))
        RC(amds_dropout_cast_bwd(dtk, D, dy, D, M2, D, AMDS_F32, p, seed, sid + 2, stream));
        RC(lin_dw(dy, to, g.sa_out_w, M2, D, D, stream));
        RC(colsum(dy, D, g.sa_out_b, M2, D, AMDS_F32));
        RC(lin_dx(dy, L.sa_out_w, d2, M2, D, D, stream));                                              // d(to)
        float* dtqkv = d1;                                                                              // [M2][3 D]
        const long sq = (long)nt * 3 * D, sp2 = (long)Hd * nt * nt, spi = (long)nt * nt;
        RC(bg(d2, D, (long)nt * D, hd, tqkv + 2 * D, 3 * D, sq, hd, 1, dP, nt, sp2, spi, Bb, Hd, nt, nt, hd, 1.0f, nullptr, 0, stream));            // d(Pd) = d(to) V^T
        RC(bg(Pd, nt, sp2, spi, d2, D, (long)nt * D, hd, 2, dtqkv + 2 * D, 3 * D, sq, hd, Bb, Hd, nt, hd, nt, 1.0f, nullptr, 0, stream));           // dV = Pd^T d(to)
        RC(amds_attention_dropout_rows(dP, dP, (long)Bb * Hd * nt, nt, p, seed, sid + 1, stream));
        RC(amds_softmax_rows_bwd(P, dP, (long)Bb * Hd * nt, nt, stream));                                                                          // dS
        RC(bg(dP, nt, sp2, spi, tqkv + D, 3 * D, sq, hd, 0, dtqkv, 3 * D, sq, hd, Bb, Hd, nt, hd, nt, sa_scale, nullptr, 0, stream));               // dQ = dS K / sqrt(hd)
        RC(bg(dP, nt, sp2, spi, tqkv, 3 * D, sq, hd, 2, dtqkv + D, 3 * D, sq, hd, Bb, Hd, nt, hd, nt, sa_scale, nullptr, 0, stream));               // dK = dS^T Q / sqrt(hd)
        RC(lin_dw(dtqkv, th1, g.sa_in_w, M2, 3 * D, D, stream));
        RC(colsum(dtqkv, 3 * D, g.sa_in_b, M2, 3 * D, AMDS_F32));
        RC(lin_dx(dtqkv, L.sa_in_w, dth, M2, 3 * D, D, stream));
        RC(ln_bwd32(dth, t_in, Sf(o.mu1), Sf(o.rs1), L.ln1_w, dtk, g.ln1_w, g.ln1_b));
    }
    // the class tokens: every bag reads the same nt rows
    RC(colsum(dtk, (long)nt * D, G.class_tokens, Bb, nt * D, AMDS_F32));

    // ---- encoder (:188) and projector (:171).  Without a decoder layer nothing reaches them: exact zeros.
    if (d.Ld == 0) {
        AMDS_HIP(hipMemsetAsync(G.proj_w, 0, (size_t)Dp * Fp * 4, st));
        AMDS_HIP(hipMemsetAsync(G.proj_b, 0, (size_t)Dp * 4, st));
        for (int l = 0; l < d.Le; ++l) {
            const amds_mil_vit_layer_grads& g = G.enc_layers_host[l];
            AMDS_HIP(hipMemsetAsync(g.ln1_w, 0, (size_t)D * 4, st)); AMDS_HIP(hipMemsetAsync(g.ln1_b, 0, (size_t)D * 4, st));
            AMDS_HIP(hipMemsetAsync(g.ln2_w, 0, (size_t)D * 4, st)); AMDS_HIP(hipMemsetAsync(g.ln2_b, 0, (size_t)D * 4, st));
            AMDS_HIP(hipMemsetAsync(g.in_w, 0, (size_t)3 * Da * Dp * 4, st)); AMDS_HIP(hipMemsetAsync(g.in_b, 0, (size_t)3 * Da * 4, st));
            AMDS_HIP(hipMemsetAsync(g.out_w, 0, (size_t)Dp * Da * 4, st)); AMDS_HIP(hipMemsetAsync(g.out_b, 0, (size_t)Dp * 4, st));
            AMDS_HIP(hipMemsetAsync(g.fc1_w, 0, (size_t)FFp * Dp * 4, st)); AMDS_HIP(hipMemsetAsync(g.fc1_b, 0, (size_t)FFp * 4, st));
            AMDS_HIP(hipMemsetAsync(g.fc2_w, 0, (size_t)Dp * FFp * 4, st)); AMDS_HIP(hipMemsetAsync(g.fc2_b, 0, (size_t)Dp * 4, st));
        }
        return AMDS_OK;
    }
    for (int l = d.Le - 1; l >= 0; --l) {
        const amds_mil_vit_layer& L = w.enc_layers_host[l];
        const amds_mil_vit_layer_grads& g = G.enc_layers_host[l];
        const EncOff& o = sp.enc[l];
        const uint32_t sid = 10u * l;
        const float* x_in = Sf(sp.x0 + (size_t)l * sp.x_bytes);
        const float* x_mid = Sf(o.x_mid);
        const void *h1 = sv + o.h1, *h2 = sv + o.h2, *qkv = sv + o.qkv, *att = sv + o.att, *z = sv + o.z, *u = sv + o.u;
        // feed-forward: x_out = x_mid + drop3(W2 drop2(relu(W1 LN2(x_mid))))
        RC(amds_dropout_cast_bwd(dx, Dp, g16, Dp, M, Dp, dt, p, seed, sid + 3, stream));
        RC(gemm(g16, Dp, L.fc2_wt, Dp, M, FFp, Dp, AMDS_EPI_BIAS, du, FFp, nullptr));
        RC(wgrad(g16, Dp, u, FFp, Dp, FFp, g.fc2_w));
        RC(colsum(g16, Dp, g.fc2_b, M, Dp, dt));
        RC(amds_relu_dropout_bwd(z, du, dz, M * FFp, dt, dt, dt, p, seed, sid + 2, stream));
        RC(gemm(dz, FFp, L.fc1_wt, FFp, M, Dp, FFp, AMDS_EPI_BIAS_F32, dh, Dp, nullptr));
        RC(wgrad(dz, FFp, h2, Dp, FFp, Dp, g.fc1_w));
        RC(colsum(dz, FFp, g.fc1_b, M, FFp, dt));
        RC(layernorm_bwd_cast_dt(dh, Dp, x_mid, Dp, Sf(o.mu2), Sf(o.rs2), L.ln2_w, dx, Dp, 1, g.ln2_w, g.ln2_b, 0, (int)M, D, lnb, wp.lnb_bytes, nullptr, 0, dt, 0.f, 0, 0,
                                 stream));
        // self-attention: x_mid = x_in + drop4(Wo attention(W_in LN1(x_in)))
        RC(amds_dropout_cast_bwd(dx, Dp, g16, Dp, M, Dp, dt, p, seed, sid + 4, stream));
        RC(gemm(g16, Dp, L.out_wt, Dp, M, Da, Dp, AMDS_EPI_BIAS, datt, Da, nullptr));
        RC(wgrad(g16, Dp, att, Da, Dp, Da, g.out_w));
        RC(colsum(g16, Dp, g.out_b, M, Dp, dt));
        RC(amds_attention_bwd_train(qkv, att, datt, Sf(o.lse), dqs, dqkv, Bb, T, Ha, dt, p, seed, sid + 1, stream));
        RC(wgrad(dqkv, 3 * Da, h1, Dp, 3 * Da, Dp, g.in_w));
        RC(colsum(dqkv, 3 * Da, g.in_b, M, 3 * Da, dt));
        RC(gemm(dqkv, 3 * Da, L.in_wt, 3 * Da, M, Dp, 3 * Da, AMDS_EPI_BIAS_F32, dh, Dp, nullptr));
        RC(layernorm_bwd_cast_dt(dh, Dp, x_in, Dp, Sf(o.mu1), Sf(o.rs1), L.ln1_w, dx, Dp, 1, g.ln1_w, g.ln1_b, 0, (int)M, D, lnb, wp.lnb_bytes, nullptr, 0, dt, 0.f, 0, 0,
                                 stream));
    }
    // projector: x0 = relu(zp) + PE
    RC(amds_relu_dropout_bwd(sv + sp.zp, dx, g16, M * Dp, dt, AMDS_F32, dt, 0.f, 0, 0, stream));
    RC(wgrad(g16, Dp, sv + sp.a, Fp, Dp, Fp, G.proj_w));
    RC(colsum(g16, Dp, G.proj_b, M, Dp, dt));
    return AMDS_OK;
}
