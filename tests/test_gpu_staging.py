"""The bag staging every MIL head shares (stage_rows_dt, csrc/elementwise.hip): one dtype ladder behind amds_mil_vit_forward, amds_barspoon_train_forward
(p = 0) and amds_ticon_slide_forward.  The inputs hold values of a 16-bit type, so the 16-bit operand rows the first GEMM reads are the same whether the
caller hands them over in that type or up-cast to fp32 -- the results must agree bit for bit; a wrong source or destination type in the ladder breaks that.
No tolerance is involved."""
import pytest
import torch

from stamp_amd import barspoon as bs
from stamp_amd import mil_core
from stamp_amd.barspoon import EncDecTransformer
from stamp_amd.mil import VisionTransformer
from stamp_amd.ticon import HipTiconSlide

pytestmark = pytest.mark.gpu

B, T, D, H, FF = 2, 37, 64, 2, 128
ACTS = [torch.float16, torch.bfloat16]


def _vit(gpu, F, act):
    torch.manual_seed(1)
    model = VisionTransformer(dim_output=3, dim_input=F, dim_model=D, n_layers=1, n_heads=H, dim_feedforward=FF, dropout=0.0, use_alibi=False)
    tensors = dict(model.named_parameters())
    pk = mil_core.PackedVit(model.dims, lambda n: tensors[n].detach().to(gpu, torch.float32), act, train=False)
    return lambda x, pos: mil_core.forward_infer(pk, x, None, None)


def _barspoon(gpu, F, act):
    torch.manual_seed(2)
    model = EncDecTransformer(F, {"a": 2, "b": 3, "c": 2}, d_model=D, num_encoder_heads=H, num_decoder_heads=H, num_encoder_layers=1, num_decoder_layers=1,
                              dim_feedforward=FF)
    tensors = dict(model.named_parameters())
    pack = bs.TrainPack(model, lambda n: tensors[n].detach().to(gpu, torch.float32), act, gpu)
    return lambda x, pos: bs.train_forward(pack, x, pos, p=0.0, seed=0)[0]


def _ticon(gpu, F, act):
    g = torch.Generator().manual_seed(3)
    sd = {}

    def lin(name, n, k):
        sd[name + ".weight"], sd[name + ".bias"] = torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g) * 0.02

    def norm(name):
        sd[name + ".weight"], sd[name + ".bias"] = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)

    p = "input_proj_dict.input_proj_hoptimus1."
    lin(p + "fc1", D, F), lin(p + "fc2", D, D), norm(p + "norm"), norm("enc_norm")
    b = "encoder.blocks.0."
    norm(b + "residual1.norm"), norm(b + "residual2.norm")
    for n in ("q_proj", "k_proj", "v_proj", "proj"):
        lin(b + "residual1.fn." + n, D, D)
    lin(b + "residual2.fn.fc1", FF, D), lin(b + "residual2.fn.fc2", D, FF // 2)
    model = HipTiconSlide(sd, device=gpu, dtype=act, heads=H, check=False)
    return lambda x, pos: model(x, pos)


ENTRIES = {"vit": (_vit, ACTS), "barspoon_train": (_barspoon, ACTS), "ticon_slide": (_ticon, [torch.float16])}      # entry -> (builder, 16-bit input types it accepts)


@pytest.fixture(scope="module")
def runs():
    """(entry, feature width, operand type) -> the packed model's call, built once; released with the module"""
    cache: dict = {}

    def get(gpu, entry, F, act):
        k = (entry, F, act)
        if k not in cache:
            cache[k] = ENTRIES[entry][0](torch.device(gpu), F, act)
        return cache[k]

    yield get
    cache.clear()


def _inputs(gpu, F, dt_in):
    g = torch.Generator().manual_seed(F + (1 if dt_in == torch.bfloat16 else 0))
    x = torch.randn(B, T, F, generator=g).to(dt_in).to(gpu)
    pos = torch.randint(0, 40, (B, T, 2), generator=g).float().to(gpu)
    return x, pos


@pytest.mark.parametrize("act", ACTS, ids=["f16", "bf16"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_staged_and_padded_input_of_every_dtype_gives_the_fp32_inputs_bits(gpu, runs, entry, act):
    """Feature width 200: staged and zero padded to 256 whatever the input type."""
    run = runs(gpu, entry, 200, act)
    for dt_in in ENTRIES[entry][1]:
        x, pos = _inputs(gpu, 200, dt_in)
        got, want = run(x, pos), run(x.float(), pos)
        assert bool(torch.isfinite(want).all()) and want.abs().max().item() > 0
        assert torch.equal(got, want), (entry, act, dt_in, (got.float() - want.float()).abs().max().item())


@pytest.mark.parametrize("entry,act", [(e, a) for e in ENTRIES for a in ENTRIES[e][1]], ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_operand_form_input_skips_the_staging_and_gives_the_fp32_inputs_bits(gpu, runs, entry, act):
    """Feature width 256 in the operand type: the rows are the first GEMM's operand as they are (the deploy calls read them in place, the training call copies
    them into its arena); the fp32 input of the same values goes through the staging kernel.  (amds_ticon_slide_forward takes fp32 / fp16 embeddings only, so its
    bf16 operands are always staged: the case above.)"""
    run = runs(gpu, entry, 256, act)
    x, pos = _inputs(gpu, 256, act)
    got, want = run(x, pos), run(x.float(), pos)
    assert bool(torch.isfinite(want).all()) and want.abs().max().item() > 0
    assert torch.equal(got, want), (entry, act, (got.float() - want.float()).abs().max().item())
