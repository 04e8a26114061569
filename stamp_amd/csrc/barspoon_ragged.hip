// barspoon_ragged.hip -- the deploy / validation forward of the barspoon head over RAGGED bags: N bags of different lengths packed without padding, one call,
// each bag's logits as its own amds_barspoon_forward call gives them.
//
// The reference has no form of this: it validates and deploys barspoon like every head, full bags at one bag per batch (src/stamp/modeling/train.py:467-477;
// src/stamp/modeling/models/barspoon.py:327-344).  Layout: bag i owns rows offsets[i] .. offsets[i+1] - 1 of the packed [total_tiles][n_feats] tensor and of
// every tile-major buffer -- barspoon's encoder has no class token among its rows, so the per-call table (attention_flash.hip, varlen_plan_kernel) is built
// with extra_rows = 0.  Everything per row (staging, projector, position encoding, LayerNorms, GEMMs) runs as in barspoon.hip on the total_tiles rows; what
// couples the rows of one bag reads the table: the encoder's self-attention (attn_flash_kernel<VARLEN>) and the class tokens' cross-attention
// (cross_attention_kernel<VARLEN>).  The launch sequences of a layer are barspoon.hip's own (bs_encoder_layer / bs_decoder_layer).
//
// Same bits as the per-bag calls.  Tile side: as mil_vit_ragged.hip, every 16-bit GEMM runs on the kernel the longest bag's own call would pick when that is
// kernel 0 and by shape otherwise (ragged_cfg, model_call.h); a bag whose own call leaves kernel 0 shares a call bit-identically only when it is alone
// (amds_barspoon_ragged_max_shared_tiles; the Python grouping sends it alone).  Class-token side: amds_bgemm_f32 picks its tile kernel from M, so the products
// over the class rows run with the bag as the batch dimension (M = n_targets per bag) -- each bag goes through its one-bag call's dispatch by construction.
#include "barspoon_common.h"

namespace amds {
namespace {

int ragged_plan(const amds_barspoon_cfg* c, int n, long total_tiles, int max_tiles, BsPlan* p) {
    RC(bs_dims("amds_barspoon", c, p));
    AMDS_REQUIRE(n >= 0 && n <= 65535 && total_tiles >= n && max_tiles >= (n > 0) && max_tiles < (1 << 30),
                 "amds_barspoon_forward_ragged: bad shape n_bags=%d total_tiles=%ld max_tiles=%d (every bag has at least one tile)", n, total_tiles, max_tiles);
    // the self-attention among the class tokens is one batched fp32 product over (bag, head): amds_bgemm_f32 takes 65535 batches
    AMDS_REQUIRE((long)n * c->dec_heads <= 65535, "amds_barspoon_forward_ragged: n_bags=%d x %d decoder heads exceed the 65535 batches of one fp32 product", n,
                 c->dec_heads);
    bs_arena(c, n, (size_t)total_tiles, varlen_table_bytes(n, total_tiles), p);
    return AMDS_OK;
}

}  // namespace
}  // namespace amds

using namespace amds;

extern "C" size_t amds_barspoon_ragged_workspace_bytes(const amds_barspoon_cfg* cfg_host, int n_bags, long total_tiles, int max_tiles) {
    BsPlan p;
    if (ragged_plan(cfg_host, n_bags, total_tiles, max_tiles, &p) != AMDS_OK) return 0;
    return p.total;
}

extern "C" int amds_barspoon_ragged_max_shared_tiles(const amds_barspoon_cfg* cfg_host) {
    BsPlan p;
    if (bs_dims("amds_barspoon", cfg_host, &p) != AMDS_OK) return -1;
    // the tile GEMMs of a bag of T tiles: projector, qkv / out / fc1 / fc2 of an encoder layer, k|v of a decoder layer; monotone in T
    auto shared = [&](int T) {
        return default_gemm_cfg(T, p.Dp, p.Fp) == 0 && default_gemm_cfg(T, 3 * p.Da, p.Dp) == 0 && default_gemm_cfg(T, p.Dp, p.Da) == 0 &&
               default_gemm_cfg(T, p.FFp, p.Dp) == 0 && default_gemm_cfg(T, p.Dp, p.FFp) == 0 && default_gemm_cfg(T, 2 * p.Db, p.Dp) == 0;
    };
    return ragged_max_shared(shared, (1 << 30) - 1);
}

extern "C" int amds_barspoon_forward_ragged(const amds_barspoon_cfg* cfg_host, const amds_barspoon_weights* w_host, const void* feats, int feats_dtype,
                                            const float* positions, const int* offsets, float* logits, int n_bags, long total_tiles, int max_tiles, void* ws,
                                            size_t ws_bytes, void* stream) {
    AMDS_REQUIRE(cfg_host && w_host && feats && offsets && logits && ws, "amds_barspoon_forward_ragged: null pointer");
    const amds_barspoon_cfg& c = *cfg_host;
    const amds_barspoon_weights& w = *w_host;
    BsPlan p;
    RC(ragged_plan(cfg_host, n_bags, total_tiles, max_tiles, &p));
    AMDS_REQUIRE(w.proj_w && w.proj_b && w.class_tokens && w.head_w_host && w.head_b_host && w.n_out_host && (c.enc_layers == 0 || w.enc_layers_host) &&
                 (c.dec_layers == 0 || w.dec_layers_host), "amds_barspoon_forward_ragged: incomplete weights");
    AMDS_REQUIRE(!c.positional_encoding || (positions && w.pe_div), "amds_barspoon_forward_ragged: positional_encoding=True needs tile positions");
    AMDS_REQUIRE(feats_dtype == AMDS_F32 || feats_dtype == AMDS_F16 || feats_dtype == AMDS_BF16, "amds_barspoon_forward_ragged: bad feats dtype %d", feats_dtype);
    const long M = total_tiles;
    AMDS_REQUIRE(M < (1L << 31) - 65536, "amds_barspoon_forward_ragged: %ld tile rows do not fit the 32-bit row index", M);
    AMDS_REQUIRE(FA_SPAN_OK(max_tiles, p.Ha), "amds_barspoon_forward_ragged: max_tiles=%d: a bag's q | k | v rows exceed the 2 GB of a buffer descriptor", max_tiles);
    if (ws_bytes < p.total) {
        set_error("amds_barspoon_forward_ragged: workspace %zu < required %zu bytes", ws_bytes, p.total);
        return AMDS_ERR_WORKSPACE;
    }
    AMDS_REQUIRE(((uintptr_t)ws & 255) == 0, "amds_barspoon_forward_ragged: workspace must be 256-byte aligned");
    if (n_bags == 0) return AMDS_OK;
    hipStream_t st = (hipStream_t)stream;
    char* base = reinterpret_cast<char*>(ws);
    const int D = c.dim, Dp = p.Dp, dt = c.dtype, nt = p.nt;
    const long M2 = (long)n_bags * nt;
    const BsBufs b = bs_bufs(ws, p);
    void* table = base + p.table;
    const BsCall k{"amds_barspoon_forward_ragged", n_bags, max_tiles, M, table};

    RC(varlen_table_build(offsets, n_bags, total_tiles, max_tiles, 0, table, st));
    // ---- projector and positional encodings: per row, as barspoon.hip
    const void* a = feats;
    if (!(feats_dtype == dt && c.n_feats == p.Fp)) {
        RC(stage_rows_dt(feats, feats_dtype, c.n_feats, base + p.a, dt, p.Fp, M, c.n_feats, stream));
        a = base + p.a;
    }
    RC(amds_gemm_ex(k.gemm_cfg(Dp, p.Fp), a, p.Fp, w.proj_w, p.Fp, (int)M, Dp, p.Fp, dt, AMDS_EPI_BIAS_RELU_F32, b.x, Dp, w.proj_b, nullptr, nullptr, 0, 0, 0, 1.0f,
                    stream));
    if (c.positional_encoding) RC(pos_encoding_add(b.x, Dp, D, positions, w.pe_div, M, st));
    if (Dp != D) AMDS_HIP(hipMemsetAsync(b.h, 0, (size_t)M * Dp * 2, st));      // LayerNorm writes the first D columns only

    for (int l = 0; l < c.enc_layers; ++l) RC(bs_encoder_layer(k, p, c, w.enc_layers_host[l], l, b, stream));
    if (c.dec_layers > 0) RC(amds_cast_pad(b.x, Dp, b.h, Dp, (int)M, Dp, dt, stream));

    RC(broadcast_rows(w.class_tokens, b.tok, (long)nt * D, M2 * D, st));
    for (int l = 0; l < c.dec_layers; ++l) RC(bs_decoder_layer(k, p, c, w.dec_layers_host[l], l, b, stream));
    return bs_heads(k, p, c, w, b.tok, logits, stream);
}
