"""The planners of the one-call model entries, on the host: workspace / arena sizes of fixed configurations as literal byte counts, and the refusals
of configurations no plan exists for.  No kernel runs; the numbers pin the padded layout (widths to 256, heads to 4 x 64 channels) and the 256-byte
arena arithmetic, so a change to either shows up here before it shows up as a too-small workspace on a GPU."""
import ctypes as C

import pytest

from stamp_amd import _lib

F16, BF16, F32 = _lib.F16, _lib.BF16, _lib.F32

# (n_feats, dim, heads, ff, classes, layers, alibi, dtype), (bags, tiles) -> workspace, ragged workspace, train arena, train workspace split_k 1 / 32, Grad-CAM workspace
VIT = [
    ((200, 96, 3, 160, 2, 2, 1, F16), (2, 37), (350976, 356352, 1405440, 5831168, 139786752, 434432)),
    ((200, 96, 3, 160, 2, 2, 1, F16), (64, 1024), (302867200, 302975232, 1213756416, 618237184, 752323840, 372372736)),
    ((256, 256, 8, 512, 2, 2, 0, BF16), (1, 1), (15360, 19200, 47360, 10045440, 270092288, 24320)),
    ((256, 256, 8, 512, 2, 2, 0, BF16), (64, 1024), (470844160, 471017728, 1484594176, 970433536, 1230480384, 577350656)),
    ((256, 256, 8, 512, 2, 0, 0, F16), (2, 37), (546816, 554240, 310528, 4734720, 69484288, 676096)),
]
# (n_feats, dim, enc_heads, dec_heads, ff, enc_layers, dec_layers, n_targets, positional_encoding, dtype), (bags, tiles) -> workspace, train arena, train workspace 1 / 32
BARSPOON = [
    ((200, 96, 3, 8, 160, 2, 2, 3, 1, F16), (2, 37), (513280, 1566208, 2701824, 35207680)),
    ((200, 96, 3, 8, 160, 2, 2, 3, 1, F16), (2, 300), (4014336, 12102656, 6768384, 39274240)),
    ((256, 256, 8, 8, 512, 1, 1, 3, 1, BF16), (64, 1024), (605767680, 979810816, 715344896, 764103680)),
]
# (in_dim, dim, heads, hidden, depth, dtype), (slides, tiles) -> workspace
TICON_SLIDE = [((200, 96, 3, 160, 2, F16), (2, 37), 322048), ((1536, 1536, 24, 4096, 2, BF16), (64, 1024), 1879048192)]
# (in_dim, dim, hidden, depth), tiles -> workspace
TICON_TILE = [((200, 96, 160, 0), 37, 82176), ((1536, 1536, 4096, 2), 65536, 2281701376)]
# (n_feats, dim, classes, train_cls_tail), (bags, tiles) -> workspace, train arena, train workspace
TRANSMIL = [((200, 96, 3, 1), (2, 37), (2385920, 12525568, 3120128)), ((200, 96, 3, 1), (64, 1024), (575873280, 1446447104, 637884416))]
TRANSMIL_RAGGED = [([5, 1, 70], 2629632), ([1], 956928), ([1024, 1025, 3, 300], 15919104), ([], 102400)]
# dim, (bags, tokens) -> saved, workspace
NYSTROM = [(96, (2, 37), (5484544, 1987072)), (96, (64, 1025), (620912896, 505490176))]


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _refused(lib, size, text):
    assert size == 0 and text in lib.amds_last_error(), (size, lib.amds_last_error())


@pytest.mark.parametrize("cfg,shape,want", VIT)
def test_vit_head_plans(lib, cfg, shape, want):
    c, (B, T) = C.byref(_lib.MilVitCfg(*cfg)), shape
    got = (lib.amds_mil_vit_workspace_bytes(c, B, T), lib.amds_mil_vit_ragged_workspace_bytes(c, B, B * T, T), lib.amds_mil_vit_train_saved_bytes(c, B, T),
           lib.amds_mil_vit_train_workspace_bytes(c, B, T, 1), lib.amds_mil_vit_train_workspace_bytes(c, B, T, 32), lib.amds_mil_vit_gradcam_workspace_bytes(c, B, T))
    assert got == want


@pytest.mark.parametrize("cfg,shape,want", BARSPOON)
def test_barspoon_plans(lib, cfg, shape, want):
    c, (B, T) = C.byref(_lib.BarspoonCfg(*cfg)), shape
    got = (lib.amds_barspoon_workspace_bytes(c, B, T), lib.amds_barspoon_train_saved_bytes(c, B, T), lib.amds_barspoon_train_workspace_bytes(c, B, T, 1),
           lib.amds_barspoon_train_workspace_bytes(c, B, T, 32))
    assert got == want


def test_ticon_transmil_and_nystrom_plans(lib):
    for cfg, (B, T), want in TICON_SLIDE:
        assert lib.amds_ticon_slide_workspace_bytes(C.byref(_lib.TiconSlideCfg(*cfg)), B, T) == want
    for (ind, dim, hid, dep), n, want in TICON_TILE:
        assert lib.amds_ticon_tile_workspace_bytes(C.byref(_lib.TiconWeights(in_dim=ind, dim=dim, hidden=hid, depth=dep)), n) == want
    for cfg, (B, T), want in TRANSMIL:
        c = C.byref(_lib.TransMilCfg(*cfg))
        assert (lib.amds_transmil_workspace_bytes(c, B, T), lib.amds_transmil_train_saved_bytes(c, B, T), lib.amds_transmil_train_workspace_bytes(c, B, T)) == want
    c = C.byref(_lib.TransMilCfg(200, 96, 3, 1))
    for tiles, want in TRANSMIL_RAGGED:
        assert lib.amds_transmil_ragged_workspace_bytes(c, len(tiles), (C.c_int * max(len(tiles), 1))(*tiles)) == want
    for dim, (B, n), want in NYSTROM:
        assert (lib.amds_nystrom_attn_saved_bytes(dim, B, n), lib.amds_nystrom_attn_workspace_bytes(dim, B, n)) == want


def test_refused_configurations(lib):
    vit = lambda *cfg: C.byref(_lib.MilVitCfg(*cfg))  # noqa: E731
    ok = (200, 96, 3, 160, 2, 2, 1, F16)
    # head_dim > 64, dim % heads != 0, a 32-bit operand type, split_k outside 1..1024
    _refused(lib, lib.amds_mil_vit_workspace_bytes(vit(256, 520, 8, 512, 2, 2, 0, F16), 2, 37), b"amds_mil_vit: needs head_dim <= 64")
    _refused(lib, lib.amds_mil_vit_ragged_workspace_bytes(vit(256, 520, 8, 512, 2, 2, 0, F16), 2, 74, 37), b"amds_mil_vit: needs head_dim <= 64")
    _refused(lib, lib.amds_mil_vit_train_saved_bytes(vit(256, 520, 8, 512, 2, 2, 0, F16), 2, 37), b"amds_mil_vit_train: needs head_dim <= 64")
    _refused(lib, lib.amds_mil_vit_workspace_bytes(vit(256, 100, 3, 512, 2, 2, 0, F16), 2, 37), b"dim_model=100 has to be divisible by n_heads=3")
    _refused(lib, lib.amds_mil_vit_gradcam_workspace_bytes(vit(256, 100, 3, 512, 2, 2, 0, F16), 2, 37), b"dim_model=100 has to be divisible by n_heads=3")
    _refused(lib, lib.amds_mil_vit_workspace_bytes(vit(256, 256, 8, 512, 2, 2, 0, F32), 2, 37), b"operand dtype must be f16 or bf16")
    _refused(lib, lib.amds_mil_vit_train_workspace_bytes(vit(256, 256, 8, 512, 2, 2, 0, F32), 2, 37, 4), b"the training step runs on bf16 or fp16 operands")
    _refused(lib, lib.amds_mil_vit_train_workspace_bytes(vit(*ok), 2, 37, 0), b"amds_mil_vit_train: bad split_k=0")
    _refused(lib, lib.amds_mil_vit_train_workspace_bytes(vit(*ok), 2, 37, 2000), b"amds_mil_vit_train: bad split_k=2000")
    _refused(lib, lib.amds_mil_vit_workspace_bytes(vit(*ok), 2, 0), b"bad shape bags=2 tiles=0")
    _refused(lib, lib.amds_mil_vit_ragged_workspace_bytes(vit(*ok), 70000, 100, 10), b"bad shape n_bags=70000")
    bs = lambda *cfg: C.byref(_lib.BarspoonCfg(*cfg))  # noqa: E731
    _refused(lib, lib.amds_barspoon_workspace_bytes(bs(256, 520, 8, 8, 512, 1, 1, 3, 1, F16), 2, 37), b"amds_barspoon: needs head_dim <= 64")
    _refused(lib, lib.amds_barspoon_train_saved_bytes(bs(256, 520, 8, 8, 512, 1, 1, 3, 1, F16), 2, 37), b"amds_barspoon_train: needs head_dim <= 64")
    _refused(lib, lib.amds_barspoon_workspace_bytes(bs(256, 100, 3, 8, 512, 1, 1, 3, 1, F16), 2, 37), b"d_model=100 has to be divisible by the head counts (3, 8)")
    _refused(lib, lib.amds_barspoon_workspace_bytes(bs(256, 256, 8, 8, 512, 1, 1, 3, 1, F32), 2, 37), b"operand dtype must be f16 or bf16")
    _refused(lib, lib.amds_barspoon_train_workspace_bytes(bs(256, 256, 8, 8, 512, 1, 1, 3, 1, F16), 2, 37, 0), b"amds_barspoon_train: bad split_k=0")
    _refused(lib, lib.amds_barspoon_workspace_bytes(None, 1, 1), b"amds_barspoon: null config")
    _refused(lib, lib.amds_ticon_slide_workspace_bytes(C.byref(_lib.TiconSlideCfg(256, 100, 3, 512, 2, F16)), 2, 37), b"(dim=100, heads=3)")
    _refused(lib, lib.amds_ticon_slide_workspace_bytes(C.byref(_lib.TiconSlideCfg(256, 256, 8, 512, 2, F32)), 2, 37), b"operand dtype must be f16 or bf16")
    _refused(lib, lib.amds_ticon_tile_workspace_bytes(C.byref(_lib.TiconWeights(in_dim=200, dim=98, hidden=160, depth=1)), 5), b"amds_ticon: bad configuration")
    _refused(lib, lib.amds_transmil_workspace_bytes(C.byref(_lib.TransMilCfg(8, 60, 2, 0)), 2, 37), b"dim_hidden must be a multiple of 8")
    _refused(lib, lib.amds_transmil_train_saved_bytes(C.byref(_lib.TransMilCfg(8, 60, 2, 0)), 2, 37), b"amds_transmil_train: bad config")
    _refused(lib, lib.amds_transmil_ragged_workspace_bytes(C.byref(_lib.TransMilCfg(200, 96, 3, 1)), 3, (C.c_int * 3)(5, 0, 7)), b"bag 1 has 0 tiles (empty bag)")
    _refused(lib, lib.amds_nystrom_attn_saved_bytes(60, 2, 37), b"dim=60 must be a positive multiple of 8")
    _refused(lib, lib.amds_nystrom_attn_workspace_bytes(96, 9000, 2), b"9000 bags x 8 heads exceed")
