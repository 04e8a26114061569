"""The reference's H-optimus-1 + TICON tile extractor (src/stamp/preprocessing/extractor/ticon.py: `HOptimusTICON` :626-718, factory `ticon()`
:721-741, `ExtractorName.TICON`) on the HIP path.

Stage 1 is the ViT-g/14 trunk the package already runs (`stamp_amd.vit.PRESETS["h_optimus_0"]`: H-optimus-0 and -1 share the architecture and the
normalisation constants, h_optimus_1.py:15-32).  Stage 2 -- TICON's `EncoderDecoder` called with ONE token per tile and zero coordinates, as
the reference's `forward` does (:697-718) -- is `HipTiconTile`: one library call (`amds_ticon_tile_forward`, csrc/ticon.hip) in exact fp32 on the
batch of tile embeddings.  With a single key the attention returns its value, so only `v_proj` and `proj` of every attention module carry
arithmetic; `q_proj` / `k_proj`, the decoder and the output projections of the checkpoint are not on this path and are ignored.

SLIDE mode -- what the model is for: all tiles of a slide as one sequence with their coordinates, every tile attending to the others under the
distance bias of `Attention.forward` (:183-215) -- is `HipTiconSlide` (`amds_ticon_slide_forward`, csrc/ticon.hip: 16-bit MFMA GEMMs on an fp32
residual stream, the streaming attention with the bias inside the softmax), and `contextualise_features` applies it to a tile-feature file.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, h5io, ops
from .vit import PRESETS, FeatureRangeError, HipViT



class HipTiconTile(nn.Module):
    """TICON on single tiles: `forward(emb [B, in_dim] f16 / f32 on the GPU) -> [B, dim]` (f32, or f16 with `out_dtype=torch.float16`).
    `state_dict`: the `EncoderDecoder`'s own (the reference strips the checkpoint's "backbone." prefix, ticon.py:614-619); `key`: which input
    projection to use ("hoptimus1" in the reference's extractor)."""

    def __init__(self, state_dict: dict[str, torch.Tensor], *, key: str = "hoptimus1", device="cuda", out_dtype: torch.dtype = torch.float32) -> None:
        super().__init__()
        self.device_ = torch.device(device)
        if self.device_.type != "cuda":
            raise RuntimeError("HipTiconTile runs on the GPU only (no CPU fallback)")
        self.key, self.out_dtype = key, out_dtype
        p = f"input_proj_dict.input_proj_{key}."
        need = [p + n for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "norm.weight", "norm.bias")] + ["enc_norm.weight", "enc_norm.bias"]
        missing = [k for k in need if k not in state_dict]
        if missing:
            raise KeyError(f"TICON state_dict lacks {missing}")
        g = lambda n: state_dict[n].detach().to(self.device_, torch.float32).contiguous()  # noqa: E731
        self._keep: list[torch.Tensor] = []

        def T(t: torch.Tensor) -> int:
            t = t.contiguous()
            self._keep.append(t)
            return t.data_ptr()

        depth = 0
        while f"encoder.blocks.{depth}.residual1.norm.weight" in state_dict:
            depth += 1
        self.in_dim, self.dim = state_dict[p + "fc1.weight"].shape[1], state_dict[p + "fc1.weight"].shape[0]
        self.hidden = state_dict["encoder.blocks.0.residual2.fn.fc1.weight"].shape[0] if depth else 2
        self.depth = depth
        self._blocks = (_lib.TiconBlock * max(depth, 1))()
        for l in range(depth):
            b = f"encoder.blocks.{l}."
            g1 = g(b + "residual1.gamma") if (b + "residual1.gamma") in state_dict else torch.ones(self.dim, device=self.device_)
            g2 = g(b + "residual2.gamma") if (b + "residual2.gamma") in state_dict else torch.ones(self.dim, device=self.device_)
            self._blocks[l] = _lib.TiconBlock(T(g(b + "residual1.norm.weight")), T(g(b + "residual1.norm.bias")), T(g(b + "residual1.fn.v_proj.weight")),
                                              T(g(b + "residual1.fn.v_proj.bias")), T(g(b + "residual1.fn.proj.weight") * g1[:, None]), T(g(b + "residual1.fn.proj.bias") * g1),
                                              T(g(b + "residual2.norm.weight")), T(g(b + "residual2.norm.bias")), T(g(b + "residual2.fn.fc1.weight")),
                                              T(g(b + "residual2.fn.fc1.bias")), T(g(b + "residual2.fn.fc2.weight") * g2[:, None]), T(g(b + "residual2.fn.fc2.bias") * g2))
        self._w = _lib.TiconWeights(self.in_dim, self.dim, self.hidden, depth, T(g(p + "fc1.weight")), T(g(p + "fc1.bias")), T(g(p + "fc2.weight")), T(g(p + "fc2.bias")),
                                    T(g(p + "norm.weight")), T(g(p + "norm.bias")), self._blocks, T(g("enc_norm.weight")), T(g("enc_norm.bias")))

    @torch.no_grad()
    def forward(self, emb: torch.Tensor) -> torch.Tensor:
        if not emb.is_cuda:
            raise RuntimeError("HipTiconTile needs its input on the GPU (no CPU fallback)")
        if emb.dim() != 2 or emb.shape[1] != self.in_dim:
            raise ValueError(f"expected tile embeddings [batch, {self.in_dim}], got {tuple(emb.shape)}")
        if emb.dtype not in (torch.float32, torch.float16):
            emb = emb.float()
        emb = emb.contiguous()
        B, dev = emb.shape[0], emb.device
        lib = _lib.lib()
        need = lib.amds_ticon_tile_workspace_bytes(C.byref(self._w), B)
        if need == 0 and B > 0:
            _lib.check(-1, "ticon_tile_workspace_bytes")
        ws = ops.scratch("ticon", dev, need)
        out = torch.empty(B, self.dim, dtype=self.out_dtype, device=dev)
        _lib.check(lib.amds_ticon_tile_forward(C.byref(self._w), emb.data_ptr(), ops._DT[emb.dtype], out.data_ptr(), ops._DT[self.out_dtype], B, ws.data_ptr(), ws.numel(),
                                               ops._stream()), "ticon_tile_forward")
        return out


class HipHOptimusTicon(nn.Module):
    """`HOptimusTICON` of the reference (ticon.py:626-718): u8 tiles [B, 224, 224, 3] (or what `HipViT` accepts) -> fp16 features [B, 1536]:
    the H-optimus trunk, then TICON on every tile alone.  `vit_state_dict`: timm names of "bioptimus/H-optimus-1" (:634-641);
    `ticon_state_dict`: the TICON backbone (:680-688)."""

    def __init__(self, vit_state_dict: dict[str, torch.Tensor], ticon_state_dict: dict[str, torch.Tensor], *, device="cuda", chunk: int = 512, vit_cfg=None) -> None:
        super().__init__()
        self.vit = HipViT(vit_cfg or PRESETS["h_optimus_0"], vit_state_dict, device=device, chunk=chunk)
        self.ticon = HipTiconTile(ticon_state_dict, key="hoptimus1", device=device, out_dtype=torch.float16)
        if self.ticon.in_dim != self.vit.cfg.dim:
            raise ValueError(f"TICON's hoptimus1 projection takes {self.ticon.in_dim}-d embeddings, the trunk gives {self.vit.cfg.dim}")

    @torch.no_grad()
    def forward(self, tiles: torch.Tensor) -> torch.Tensor:
        return self.ticon(self.vit(tiles))


def alibi_slopes(heads: int) -> list[float]:
    """The per-head slopes of ALiBi (Press et al., "Train Short, Test Long", 2022): for 2^a heads the geometric sequence r, r^2, ... with
    r = 2^(-8 / heads); otherwise those of the largest power of two m <= heads, then every second slope of the 2m-head sequence.  This is what the
    reference's `get_slopes` (ticon.py:102-119) computes; 24 heads: the 16-head sequence + 8 of the 32-head one."""
    def pow2(m: int) -> list[float]:
        r = 2.0 ** (-(2.0 ** -(math.log2(m) - 3)))
        return [r * r ** i for i in range(m)]

    if heads < 1:
        raise ValueError(f"heads must be positive, got {heads}")
    m = 1 << (heads.bit_length() - 1)
    return pow2(m) if m == heads else pow2(m) + pow2(2 * m)[0::2][: heads - m]


class HipTiconSlide(nn.Module):
    """TICON on whole slides: `forward(emb [N, in_dim] | [B, N, in_dim], coords [N, 2] | [B, N, 2]) -> [N, dim] | [B, N, dim]` (`out_dtype`), every
    slide of a batch with the same N.  `state_dict`: the `EncoderDecoder`'s own, as for `HipTiconTile`; `key`: any `input_proj_<key>` it holds;
    `heads`: the checkpoint does not store it -- default dim / 64 (the published model: 1536 / 24).  `coords`: in the unit the model was trained on.
    `dtype`: the MFMA operand type.  `check=True`: `amds_check_finite` on every result; non-finite fp16 features (an intermediate left the fp16
    range) are recomputed on bf16 operands -- from then on for this object, with one warning -- and `FeatureRangeError` is raised when that does not
    help (`HipViT`'s policy).  GPU only, inference only."""

    def __init__(self, state_dict: dict[str, torch.Tensor], *, key: str = "hoptimus1", device="cuda", dtype: torch.dtype = torch.float16,
                 out_dtype: torch.dtype = torch.float32, check: bool = True, heads: int | None = None) -> None:
        super().__init__()
        self.device_ = torch.device(device)
        if self.device_.type != "cuda":
            raise RuntimeError("HipTiconSlide runs on the GPU only (no CPU fallback)")
        if out_dtype not in (torch.float32, torch.float16):
            raise ValueError(f"out_dtype must be float32 or float16, got {out_dtype}")
        p = f"input_proj_dict.input_proj_{key}."
        need = [p + n for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "norm.weight", "norm.bias")] + ["enc_norm.weight", "enc_norm.bias"]
        missing = [k for k in need if k not in state_dict]
        if missing:
            raise KeyError(f"TICON state_dict lacks {missing}")
        self.key, self.out_dtype, self.check = key, out_dtype, check
        self.dim, self.in_dim = state_dict[p + "fc1.weight"].shape
        self.heads = heads if heads is not None else self.dim // 64
        if self.heads < 1 or self.dim % self.heads or self.dim // self.heads > 64:
            raise ValueError(f"dim {self.dim} with {self.heads} heads: head_dim must divide dim and be <= 64 (pass heads=)")
        depth = 0
        while f"encoder.blocks.{depth}.residual1.norm.weight" in state_dict:
            depth += 1
        self.depth = depth
        self.hidden = state_dict["encoder.blocks.0.residual2.fn.fc1.weight"].shape[0] if depth else 2
        self._sd = state_dict
        self._pack(dtype)

    def _pack(self, dtype: torch.dtype) -> None:
        """Padded device weights in the layout of `amds_ticon_slide_weights` (include/amdstamp.h) with `dtype` operands."""
        sd, dev = self._sd, self.device_
        D, H, hd, H2 = self.dim, self.heads, self.dim // self.heads, self.hidden // 2
        up = lambda n, m: (n + m - 1) // m * m  # noqa: E731
        Fp, Dp, Ha, Hp = up(self.in_dim, 256), up(D, 256), up(H, 4), up(H2, 128)
        Da = 64 * Ha
        self._keep: list[torch.Tensor] = []
        g = lambda n: sd[n].detach().to(dev, torch.float32)  # noqa: E731

        def keep(t: torch.Tensor) -> int:
            self._keep.append(t)
            return t.data_ptr()

        def mat(w: torch.Tensor, R: int, Cc: int) -> int:           # fp32 [r, c] -> dtype [R][Cc], zero padded
            return keep(ops.cast_pad(F.pad(w, (0, Cc - w.shape[1], 0, R - w.shape[0])), Cc, dtype))

        def vec(v: torch.Tensor, n: int) -> int:
            return keep(F.pad(v, (0, n - v.numel())).contiguous())

        qs = 8.0 / math.sqrt(hd)                                    # the kernel scales scores by 1 / 8
        self._blocks = (_lib.TiconSlideBlock * max(self.depth, 1))()
        for l in range(self.depth):
            b = f"encoder.blocks.{l}."
            a = b + "residual1.fn."
            w3 = torch.stack([g(a + f"{n}_proj.weight").view(H, hd, D) for n in "qkv"])                  # [3, H, hd, D]
            b3 = torch.stack([g(a + f"{n}_proj.bias").view(H, hd) for n in "qkv"])
            w3, b3 = F.pad(w3, (0, 0, 0, 64 - hd, 0, Ha - H)), F.pad(b3, (0, 64 - hd, 0, Ha - H))
            w3[0] *= qs
            b3[0] *= qs
            pw = F.pad(g(a + "proj.weight").view(D, H, hd), (0, 64 - hd, 0, Ha - H)).reshape(D, Da)
            m = b + "residual2.fn."
            f1w, f1b = g(m + "fc1.weight"), g(m + "fc1.bias")
            f1w = torch.cat([F.pad(f1w[:H2], (0, Dp - D, 0, Hp - H2)), F.pad(f1w[H2:], (0, Dp - D, 0, Hp - H2))])   # x1 rows | x2 rows, each Hp
            f1b = torch.cat([F.pad(f1b[:H2], (0, Hp - H2)), F.pad(f1b[H2:], (0, Hp - H2))])
            g1 = vec(g(b + "residual1.gamma"), Dp) if (b + "residual1.gamma") in sd else None
            g2 = vec(g(b + "residual2.gamma"), Dp) if (b + "residual2.gamma") in sd else None
            self._blocks[l] = _lib.TiconSlideBlock(
                keep(g(b + "residual1.norm.weight").contiguous()), keep(g(b + "residual1.norm.bias").contiguous()),
                mat(w3.reshape(3 * Da, D), 3 * Da, Dp), keep(b3.reshape(3 * Da).contiguous()), mat(pw, Dp, Da), vec(g(a + "proj.bias"), Dp), g1,
                keep(g(b + "residual2.norm.weight").contiguous()), keep(g(b + "residual2.norm.bias").contiguous()),
                mat(ops.pack_swiglu_rows(f1w), 2 * Hp, Dp), keep(ops.pack_swiglu_rows(f1b.reshape(-1, 1)).reshape(-1).contiguous()),
                mat(g(m + "fc2.weight"), Dp, Hp), vec(g(m + "fc2.bias"), Dp), g2)
        p = f"input_proj_dict.input_proj_{self.key}."
        slopes = torch.tensor(alibi_slopes(H), dtype=torch.float32, device=dev)
        self._w = _lib.TiconSlideWeights(mat(g(p + "fc1.weight"), Dp, Fp), vec(g(p + "fc1.bias"), Dp), mat(g(p + "fc2.weight"), Dp, Dp), vec(g(p + "fc2.bias"), Dp),
                                         keep(g(p + "norm.weight").contiguous()), keep(g(p + "norm.bias").contiguous()), vec(slopes, Ha), self._blocks,
                                         keep(g("enc_norm.weight").contiguous()), keep(g("enc_norm.bias").contiguous()))
        self._cfg = _lib.TiconSlideCfg(self.in_dim, D, H, self.hidden, self.depth, ops.act_code(dtype))
        self.dtype = dtype

    def _run(self, emb: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
        B, N = emb.shape[:2]
        lib = _lib.lib()
        need = lib.amds_ticon_slide_workspace_bytes(C.byref(self._cfg), B, N)
        if need == 0 and B > 0:
            _lib.check(-1, "ticon_slide_workspace_bytes")
        ws = ops.scratch("ticon_slide", emb.device, need)
        out = ops.alloc((B, N, self.dim), self.out_dtype, emb.device)
        _lib.check(lib.amds_ticon_slide_forward(C.byref(self._cfg), C.byref(self._w), emb.data_ptr(), ops._DT[emb.dtype], coords.data_ptr(), out.data_ptr(),
                                                ops._DT[self.out_dtype], B, N, ws.data_ptr(), ws.numel(), ops._stream()), "ticon_slide_forward")
        return out

    def _finite(self, x: torch.Tensor) -> bool:
        cnt = torch.zeros(1, dtype=torch.int32, device=x.device)
        host = C.c_int(0)
        rc = _lib.lib().amds_check_finite(x.data_ptr(), x.numel(), ops._DT[x.dtype], cnt.data_ptr(), C.byref(host), ops._stream())
        if rc != _lib.ERR_RANGE:
            _lib.check(rc, "check_finite")
        return rc != _lib.ERR_RANGE

    @torch.no_grad()
    def forward(self, emb: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
        if not (emb.is_cuda and coords.is_cuda):
            raise RuntimeError("HipTiconSlide needs its inputs on the GPU (no CPU fallback)")
        flat = emb.dim() == 2
        if flat:
            emb, coords = emb[None], coords[None]
        if emb.dim() != 3 or emb.shape[2] != self.in_dim or emb.shape[1] < 1 or coords.shape != (*emb.shape[:2], 2):
            raise ValueError(f"expected embeddings [(B,) N, {self.in_dim}] with N >= 1 and coordinates [(B,) N, 2], got {tuple(emb.shape)} and {tuple(coords.shape)}")
        if emb.dtype not in (torch.float32, torch.float16):
            emb = emb.float()
        emb, coords = emb.contiguous(), coords.float().contiguous()
        out = self._run(emb, coords)
        if self.check and out.numel() and not self._finite(out):
            if self.dtype == torch.float16:
                warnings.warn("HipTiconSlide: non-finite features on fp16 operands (an intermediate left the fp16 range); this object now runs on bf16 "
                              "operands (8 bits of mantissa: outside the 1e-3 parity bar)", RuntimeWarning, stacklevel=2)
                self._pack(torch.bfloat16)
                out = self._run(emb, coords)
            if not self._finite(out):
                raise FeatureRangeError(f"HipTiconSlide: non-finite features on {self.dtype} operands")
        return out[0] if flat else out


def contextualise_features(model: HipTiconSlide, src_h5, dst_h5, *, coord_scale: float | None = None) -> None:
    """Tile-feature file -> tile-feature file of the same tiles, every feature contextualised by the others of its slide (`model` in slide mode).
    The output has the reference's layout (`h5io.write_tile_features`) with the source's coordinates and tile size; `extractor` becomes
    "<source extractor>+ticon".

    `coord_scale` turns the file's micrometre coordinates into the model's unit.  Default 1 / tile_size_um: neighbouring tiles are 1 apart.  That
    is an ASSUMPTION about the published checkpoint -- the reference only ever calls the model with zero coordinates (ticon.py:697-718) and does not
    say in which unit it was trained; pass `coord_scale=` when you know better."""
    from .encoder import AMDSTAMP_VERSION, STAMP_FORMAT_VERSION, code_hash

    feats, ci, attrs = h5io.read_tile_features(src_h5)
    if coord_scale is None:
        if not ci.tile_size_um:
            raise ValueError(f"{src_h5} does not state its tile size: pass coord_scale=")
        coord_scale = 1.0 / ci.tile_size_um
    dev = model.device_
    emb = torch.from_numpy(feats).to(dev)
    coords = torch.from_numpy(ci.coords_um.astype("float32")).to(dev) * float(coord_scale)
    out = model(emb, coords)
    h5io.write_tile_features(dst_h5, out.cpu().numpy(), ci.coords_um, extractor=f"{attrs.get('extractor', '')}+ticon", tile_size_um=ci.tile_size_um,
                             tile_size_px=int(ci.tile_size_px or 0), code_hash=code_hash()[:8], stamp_version=STAMP_FORMAT_VERSION,
                             amdstamp_version=AMDSTAMP_VERSION)
