"""TICON in slide mode, restated in torch for the tests -- TEST INFRASTRUCTURE ONLY.

Reference: src/stamp/preprocessing/extractor/ticon.py -- `EncoderDecoder.forward` :543-562 -> `forward_features` :485-541 with dec_layer=None on ALL
tiles of a slide: `input_proj_<key>` (ProjectionMlp :80-99), the encoder's blocks (Block :290-343: x += gamma1 * Attention(LN(x)); x += gamma2 *
Mlp(LN(x))), `enc_norm` :506.  `Attention.forward` :183-215 with `scaled_dot_product_attention_custom` :122-156: per head h
    softmax(q k^T / sqrt(head_dim) - slope_h * ||c_q - c_k||_2) v,    slope = get_slopes(heads) :102-119 (fp32 numbers).
Pinned by tests/golden/ticon_slide.npz and its parts (ticon_slide.*.npz), produced by running the reference's own classes (tools/make_golden.py::golden_ticon_slide).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = Path(__file__).resolve().parent.parent / "golden"
PARTS = ("", ".out64", ".b", ".a0", ".a1")          # the cases | their float64 outputs | model b's weights | model a's (two files): each below 1 MiB
MODELS = ("a", "b")
_FIXTURE: dict | None = None


def _unplane(p: np.ndarray, dtype) -> np.ndarray:
    """uint8 byte planes [itemsize, ...] (little endian) -> the array they were cut from."""
    return np.ascontiguousarray(np.moveaxis(p, 0, -1)).view(dtype)[..., 0]


def _from_order(i: np.ndarray) -> np.ndarray:
    return np.where(i >= 0, i, -i | (1 << 31)).astype(np.uint32).view(np.float32)


def _order(f: np.ndarray) -> np.ndarray:
    b = f.view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF))


def load_fixture() -> dict:
    """{"slopes": {heads: fp32 array}, "a" / "b": {"dim", "heads", "depth", "keys", "sd": state dict (fp32 tensors),
    "cases": {name: {"key", "emb" fp32, "coords" fp32, "out" fp32, "out64" float64}}}} -- decoded once, shared by the tests, never modified."""
    global _FIXTURE
    if _FIXTURE is not None:
        return _FIXTURE
    z = {}
    for suffix in PARTS:
        with np.load(GOLDEN / f"ticon_slide{suffix}.npz") as f:
            z.update({k: f[k] for k in f.files})
    fx: dict = {"slopes": {h: z[f"slopes_{h}"] for h in (3, 6, 24)}}
    for tag in MODELS:
        dim, heads, depth = (int(v) for v in z[f"{tag}_hparams"])
        sd = {}
        for k in z:
            if k.startswith(f"{tag}_wb:"):
                bits = _unplane(z[k], np.uint16).astype(np.uint32) << 16
                sd[k.split(":", 1)[1]] = torch.from_numpy(bits.view(np.float32).copy())
            elif k.startswith(f"{tag}_w:"):
                sd[k.split(":", 1)[1]] = torch.from_numpy(z[k].copy())
        cases = {}
        for k in z:
            if k.startswith(f"{tag}_") and k.endswith("_out64"):
                name = k[len(tag) + 1:-len("_out64")]
                c = f"{tag}_{name}"
                out64 = _unplane(z[k], np.float64)
                out = _from_order(_order(out64.astype(np.float32)) + z[f"{c}_outulp"].astype(np.int64))
                cases[name] = {"key": str(z[f"{c}_key"]), "emb": torch.from_numpy(z[f"{c}_emb"].astype(np.float32)), "coords": torch.from_numpy(z[f"{c}_coords"].copy()),
                               "out": torch.from_numpy(out.copy()), "out64": torch.from_numpy(out64.copy())}
        fx[tag] = {"dim": dim, "heads": heads, "depth": depth, "keys": [str(k) for k in z[f"{tag}_keys"]], "sd": sd, "cases": cases}
    _FIXTURE = fx
    return fx


def distbias_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, coords: torch.Tensor, slopes: torch.Tensor, scale: float) -> torch.Tensor:
    """q, k, v [B, H, N, hd], coords [B, N, 2], slopes [H] -> [B, H, N, hd] in q's dtype (:201-212, :152-156; materialises [B, H, N, N])."""
    c = coords.to(q.dtype)
    dist = torch.sqrt(((c[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1))
    w = q @ k.transpose(-2, -1) * scale - slopes.to(q.dtype)[None, :, None, None] * dist[:, None]
    return torch.softmax(w, dim=-1) @ v


def ticon_slide_forward(emb: torch.Tensor, coords: torch.Tensor, sd: dict, key: str, heads: int, slopes, eps: float = 1e-5) -> torch.Tensor:
    """emb [B, N, in_dim], coords [B, N, 2] -> [B, N, D]: what `EncoderDecoder(x=emb, relative_coords=coords, tile_encoder_key=key)` returns, in emb's dtype."""
    sd = {k: v.to(emb.dtype) for k, v in sd.items()}
    slopes = torch.as_tensor(slopes)
    p = f"input_proj_dict.input_proj_{key}."
    x = F.linear(F.silu(F.linear(emb, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])      # :94-98
    B, N, D = x.shape
    hd = D // heads
    x = F.layer_norm(x, (D,), sd[p + "norm.weight"], sd[p + "norm.bias"], eps)
    l = 0
    while f"encoder.blocks.{l}.residual1.norm.weight" in sd:
        b = f"encoder.blocks.{l}."
        h = F.layer_norm(x, (D,), sd[b + "residual1.norm.weight"], sd[b + "residual1.norm.bias"], eps)
        q, k, v = (F.linear(h, sd[b + f"residual1.fn.{n}_proj.weight"], sd[b + f"residual1.fn.{n}_proj.bias"]).reshape(B, N, heads, hd).transpose(1, 2)
                   for n in "qkv")                                                                                                # :197-199
        o = distbias_attention(q, k, v, coords, slopes, hd ** -0.5).transpose(1, 2).reshape(B, N, D)
        x = x + sd[b + "residual1.gamma"] * F.linear(o, sd[b + "residual1.fn.proj.weight"], sd[b + "residual1.fn.proj.bias"])       # :262
        h = F.layer_norm(x, (D,), sd[b + "residual2.norm.weight"], sd[b + "residual2.norm.bias"], eps)
        u = F.linear(h, sd[b + "residual2.fn.fc1.weight"], sd[b + "residual2.fn.fc1.bias"])
        x1, x2 = u.chunk(2, dim=-1)                                                                                               # :73-75
        x = x + sd[b + "residual2.gamma"] * F.linear(F.silu(x1) * x2, sd[b + "residual2.fn.fc2.weight"], sd[b + "residual2.fn.fc2.bias"])
        l += 1
    return F.layer_norm(x, (D,), sd["enc_norm.weight"], sd["enc_norm.bias"], eps)                                                  # :506
