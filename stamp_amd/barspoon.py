"""The reference's barspoon head (`EncDecTransformer`, src/stamp/modeling/models/barspoon.py:27-205; `ModelName.BARSPOON` of the train registry,
src/stamp/modeling/registry.py:18-25) on the HIP path -- deploy / validation forward.

Same constructor, same module tree and therefore the same state_dict keys as the reference class (the torch containers `nn.TransformerEncoder`
/ `nn.TransformerDecoder` are instantiated as parameter holders and never called): a checkpoint's `model.*` entries load with
`load_state_dict(strict=True)`.  `forward(tile_tokens, tile_positions)` -> `{target_label: logits [batch, n_out]}` is ONE library call
(`amds_barspoon_forward`, csrc/barspoon.hip): the tile side on the 16-bit MFMA path (weights zero-padded like the MIL `vit` head's), the class
tokens in exact fp32.  `forward` is eval + no-grad only (a forward that needs gradients raises); TRAINING this head (the reference's
`LitMilClassificationMixin.step`, :263-321) goes through `forward_train`: one torch.autograd.Function whose forward and backward are
`amds_barspoon_train_forward` / `amds_barspoon_train_backward` (csrc/barspoon_train.hip), `.grad` of every nn.Parameter in the reference's shapes.
`stamp_amd.barspoon_train.HipBarspoonTrainer` drives it with the reference's loss and optimiser.
`forward_ragged(bags, positions)` is the same deploy forward over bags of DIFFERENT lengths packed without padding (`amds_barspoon_forward_ragged`,
csrc/barspoon_ragged.hip): one call per group of bags, each bag's logits bit-identical to its own `forward` call.
"""
from __future__ import annotations

import ctypes as C
import math
import re

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, ops
from .mil_core import PackedVit, VitDims, layer_prefix



def sanitize(x: str) -> str:
    return re.sub(r"[^A-Za-z0-9_]", "_", x)                    # barspoon.py:351-352


_ENC_MAP = {"0.norm.": "norm1.", "0.mhsa.in_proj_": "self_attn.in_proj_", "0.mhsa.out_proj.": "self_attn.out_proj.", "1.0.": "norm2.", "1.1.": "linear1.",
            "1.4.": "linear2."}
_DEC_FP32 = (("ln1_w", "norm1.weight"), ("ln1_b", "norm1.bias"), ("sa_in_w", "self_attn.in_proj_weight"), ("sa_in_b", "self_attn.in_proj_bias"),
             ("sa_out_w", "self_attn.out_proj.weight"), ("sa_out_b", "self_attn.out_proj.bias"), ("ln2_w", "norm2.weight"), ("ln2_b", "norm2.bias"),
             ("ca_out_w", "multihead_attn.out_proj.weight"), ("ca_out_b", "multihead_attn.out_proj.bias"), ("ln3_w", "norm3.weight"), ("ln3_b", "norm3.bias"),
             ("fc1_w", "linear1.weight"), ("fc1_b", "linear1.bias"), ("fc2_w", "linear2.weight"), ("fc2_b", "linear2.bias"))


def _up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


# ---- the decoder's K | V projection: rows D .. 3 D of multihead_attn.in_proj <-> [2 Db][Dp], K heads then V heads, each padded to 64 channels ----
def pad_kv_w(w_kv: torch.Tensor, Hd: int, D: int, Dp: int) -> torch.Tensor:
    hd = D // Hd
    return F.pad(w_kv.view(2, Hd, hd, D), (0, Dp - D, 0, 64 - hd)).reshape(2 * 64 * Hd, Dp).contiguous()


def pad_kv_b(b_kv: torch.Tensor, Hd: int, D: int) -> torch.Tensor:
    hd = D // Hd
    return F.pad(b_kv.view(2, Hd, hd), (0, 64 - hd)).reshape(2 * 64 * Hd).contiguous()


def unpad_kv_w(g: torch.Tensor, Hd: int, D: int) -> torch.Tensor:
    """gradient [KVp][Dp] (KVp >= 2 Db) -> [2 D][D]"""
    hd = D // Hd
    return g[: 2 * 64 * Hd].view(2, Hd, 64, g.shape[1])[:, :, :hd, :D].reshape(2 * D, D)


def unpad_kv_b(g: torch.Tensor, Hd: int, D: int) -> torch.Tensor:
    hd = D // Hd
    return g[: 2 * 64 * Hd].view(2, Hd, 64)[:, :, :hd].reshape(2 * D)


def dropout_rate(model: "EncDecTransformer") -> float:
    """The one dropout rate of the module's torch containers (every nn.Dropout and both kinds of nn.MultiheadAttention); ValueError if they disagree."""
    rates = {}
    for name, m in list(model.transformer_encoder.named_modules(prefix="transformer_encoder")) + list(model.transformer_decoder.named_modules(prefix="transformer_decoder")):
        if isinstance(m, nn.Dropout):
            rates[name] = float(m.p)
        elif isinstance(m, nn.MultiheadAttention):
            rates[name] = float(m.dropout)
    vals = set(rates.values())
    if len(vals) > 1:
        raise ValueError(f"HIP barspoon trains with ONE dropout rate for all sites; the module's containers disagree: {sorted(vals)} "
                         f"({', '.join(f'{k}={v}' for k, v in sorted(rates.items()) if v != min(vals))})")
    return vals.pop() if vals else 0.0


class EncDecTransformer(nn.Module):
    def __init__(self, d_features: int, target_n_outs: dict[str, int], *, d_model: int = 512, num_encoder_heads: int = 8, num_decoder_heads: int = 8,
                 num_encoder_layers: int = 2, num_decoder_layers: int = 2, dim_feedforward: int = 2048, positional_encoding: bool = True) -> None:
        super().__init__()
        # the reference's module tree (:118-162), as parameter containers
        self.projector = nn.Sequential(nn.Linear(d_features, d_model), nn.ReLU())
        enc = nn.TransformerEncoderLayer(d_model=d_model, nhead=num_encoder_heads, dim_feedforward=dim_feedforward, batch_first=True, norm_first=True)
        self.transformer_encoder = nn.TransformerEncoder(enc, num_layers=num_encoder_layers, enable_nested_tensor=False)
        self.target_labels = target_n_outs.keys()
        self.class_tokens = nn.ParameterDict({sanitize(t): torch.rand(d_model) for t in target_n_outs})
        dec = nn.TransformerDecoderLayer(d_model=d_model, nhead=num_decoder_heads, dim_feedforward=dim_feedforward, batch_first=True, norm_first=True)
        self.transformer_decoder = nn.TransformerDecoder(dec, num_layers=num_decoder_layers)
        self.heads = nn.ModuleDict({sanitize(t): nn.Linear(in_features=d_model, out_features=n) for t, n in target_n_outs.items()})
        self.positional_encoding = positional_encoding
        self.d_features, self.d_model, self.dim_feedforward = d_features, d_model, dim_feedforward
        self.num_encoder_heads, self.num_decoder_heads = num_encoder_heads, num_decoder_heads
        self.num_encoder_layers, self.num_decoder_layers = num_encoder_layers, num_decoder_layers
        self.target_n_outs = dict(target_n_outs)
        if d_model % num_encoder_heads or d_model % num_decoder_heads or d_model // num_encoder_heads > 64 or d_model // num_decoder_heads > 64 or d_model % 4:
            raise NotImplementedError("HIP barspoon needs head_dim <= 64 in both stacks and d_model % 4 == 0")
        self._pack_key = None
        self.fp16_overflow_events = 0           # fp16 training steps that were re-run on bf16 operands; not part of the state_dict

    def _enc_get(self, g, dev):
        """The encoder stack under the MIL `vit` head's parameter names (zero-padded by PackedVit); `g(name)` -> fp32 device tensor of a parameter."""
        D = self.d_model

        def vit_get(name: str) -> torch.Tensor:
            if name.startswith("project_features.0."):
                return g("projector.0." + name.rsplit(".", 1)[1])
            for l in range(self.num_encoder_layers):
                p = layer_prefix(l)
                if name.startswith(p):
                    rest = name[len(p):]
                    for a, b in _ENC_MAP.items():
                        if rest.startswith(a):
                            return g(f"transformer_encoder.layers.{l}.{b}{rest[len(a):]}")
            f32 = dict(dtype=torch.float32, device=dev)
            return {"class_token": torch.zeros(D, **f32), "transformer.norm.weight": torch.ones(D, **f32), "transformer.norm.bias": torch.zeros(D, **f32),
                    "mlp_head.0.weight": torch.zeros(1, D, **f32), "mlp_head.0.bias": torch.zeros(1, **f32)}[name]

        return vit_get

    # ---- device weights, rebuilt when a parameter changed ---------------------------------------------------------------------------
    def _pack(self, dev):
        tensors = dict(self.named_parameters())
        key = (str(dev), tuple((t.data_ptr(), t._version) for t in tensors.values()))
        if self._pack_key == key:
            return self._packed
        pack = _Pack(self, lambda n: tensors[n].detach().to(dev, torch.float32), torch.float16, dev, train=False)
        self._packed, self._pack_key = pack, key
        return pack

    def forward(self, tile_tokens: torch.Tensor, tile_positions: torch.Tensor) -> dict[str, torch.Tensor]:
        if not tile_tokens.is_cuda:
            raise RuntimeError("HIP barspoon needs bags on the GPU (no CPU fallback)")
        if self.training or (torch.is_grad_enabled() and (tile_tokens.requires_grad or any(p.requires_grad for p in self.parameters()))):
            raise NotImplementedError("HIP barspoon: only the deploy / validation forward is built -- call it under .eval() and torch.no_grad() "
                                      "(training this head is not implemented)")
        if tile_tokens.dim() != 3 or tile_tokens.shape[-1] != self.d_features:
            raise ValueError(f"tile_tokens must be [batch, tile, {self.d_features}], got {tuple(tile_tokens.shape)}")
        Bb, T, _ = tile_tokens.shape
        dev = tile_tokens.device
        if self.positional_encoding and (tile_positions is None or tile_positions.shape != (Bb, T, 2)):
            raise ValueError(f"tile_positions must be [batch, tile, 2] = {(Bb, T, 2)}")
        x = tile_tokens if tile_tokens.dtype in ops._DT else tile_tokens.float()
        x = x.contiguous()
        pos = tile_positions.to(dev, torch.float32).contiguous() if tile_positions is not None else None
        pack = self._pack(dev)
        cfg, wc, no, total = pack.cfg, pack.wc, pack.no, pack.total_out
        lib = _lib.lib()
        need = lib.amds_barspoon_workspace_bytes(C.byref(cfg), Bb, T)
        if need == 0:
            _lib.check(-1, "barspoon_workspace_bytes")
        ws = ops.scratch("barspoon", dev, need)
        logits = torch.empty(Bb, total, dtype=torch.float32, device=dev)
        _lib.check(lib.amds_barspoon_forward(C.byref(cfg), C.byref(wc), x.data_ptr(), ops._DT[x.dtype], pos.data_ptr() if pos is not None else None,
                                             logits.data_ptr(), Bb, T, ws.data_ptr(), ws.numel(), ops._stream()), "barspoon_forward")
        return self._split_targets(logits, no)

    # ---- ragged inference forward: N bags of different lengths, no padding, one call per group -----------------------------------------------
    def max_shared_tiles(self, device) -> int:
        """Longest bag that shares a ragged call with others and keeps its own call's bits (amds_barspoon_ragged_max_shared_tiles); a longer bag runs alone."""
        n = int(_lib.lib().amds_barspoon_ragged_max_shared_tiles(C.byref(self._pack(torch.device(device)).cfg)))
        if n < 0:
            _lib.check(-1, "barspoon_ragged_max_shared_tiles")
        return n

    def _split_targets(self, logits: torch.Tensor, no) -> dict[str, torch.Tensor]:
        out, col = {}, 0
        for j, t in enumerate(self.target_labels):
            out[t] = logits[:, col:col + no[j]]
            col += no[j]
        return out

    def forward_ragged(self, bags, positions=None, *, bags_per_call: int | None = None, max_rows_per_call: int = 1 << 62) -> dict[str, torch.Tensor]:
        """Bags of DIFFERENT lengths without padding: lists of [T_i, d_features] (and [T_i, 2] positions) tensors -> `{target: logits [N, n_out]}` in the
        list's order, bag i's rows bit-identical to `forward(bags[i][None], positions[i][None])`.  Validated and grouped on the host (`mil_core.group_bags`
        with extra_rows=0: at most `bags_per_call` bags and `max_rows_per_call` tile rows per call, a bag longer than `max_shared_tiles` runs alone), ONE
        library call per group (amds_barspoon_forward_ragged, csrc/barspoon_ragged.hip).  Inference only: eval mode under torch.no_grad() /
        inference_mode()."""
        from . import mil_core
        if self.training or torch.is_grad_enabled():
            raise RuntimeError("forward_ragged is the inference forward: call it in eval mode (.eval()) under torch.no_grad() or torch.inference_mode()")
        bags = list(bags)
        pl = list(positions) if positions is not None else None
        if pl is not None and not self.positional_encoding:
            pl = None                                                # `forward` ignores them too
        try:
            lengths = mil_core._validate_bags(bags, pl, self.d_features, False)
        except ValueError as e:
            raise ValueError(str(e).replace("coords", "positions")) from None
        if self.positional_encoding and bags and pl is None:
            raise ValueError("positional_encoding=True needs the tile positions of every bag")
        if bags and not all(b.is_cuda for b in bags):
            raise RuntimeError("HIP barspoon needs bags on the GPU (no CPU fallback)")
        dev = bags[0].device if bags else next(self.parameters()).device
        if not bags:
            return {t: torch.empty(0, n, dtype=torch.float32, device=dev) for t, n in self.target_n_outs.items()}
        # one fp32 product of the call is batched over (bag, decoder head): 65535 batches
        per_call = min(bags_per_call or len(bags), 65535 // self.num_decoder_heads)
        outs = []
        for a, e in mil_core.group_bags(lengths, per_call, max_rows_per_call, self.max_shared_tiles(dev), extra_rows=0):
            rb = mil_core.pack_bags(bags[a:e], None if pl is None else pl[a:e], n_feats=self.d_features, device=dev)
            outs.append(self._ragged_call(rb))
        return self._split_targets(outs[0] if len(outs) == 1 else torch.cat(outs, dim=0), self._pack(dev).no)

    def _ragged_call(self, rb) -> torch.Tensor:
        """Packed bags -> logits [n_bags, total outputs]: ONE amds_barspoon_forward_ragged."""
        dev = rb.feats.device
        pack = self._pack(dev)
        cfg, wc = pack.cfg, pack.wc
        lib = _lib.lib()
        n, total, mx = rb.n_bags, rb.total_tiles, rb.max_tiles
        need = lib.amds_barspoon_ragged_workspace_bytes(C.byref(cfg), n, total, mx)
        if need == 0:
            _lib.check(-1, "barspoon_ragged_workspace_bytes")
        ws = ops.scratch("barspoon_ragged", dev, need)
        logits = torch.empty(n, pack.total_out, dtype=torch.float32, device=dev)
        pos = rb.coords if self.positional_encoding else None
        _lib.check(lib.amds_barspoon_forward_ragged(C.byref(cfg), C.byref(wc), rb.feats.data_ptr(), ops._DT[rb.feats.dtype],
                                                    pos.data_ptr() if pos is not None else None, rb.offsets.data_ptr(), logits.data_ptr(), n,
                                                    total, mx, ws.data_ptr(), ws.numel(), ops._stream()), "barspoon_forward_ragged")
        return logits

    def forward_infer_ragged(self, rb) -> dict[str, torch.Tensor]:
        """Bags that are already packed (`mil_core.RaggedBags`, e.g. a view of a resident cohort: `ResidentCohort.ragged_group`) -> `{target: logits}` in
        ONE library call, nothing copied.  Grouping is the caller's: a bag longer than `max_shared_tiles` keeps its own call's bits only when alone.
        Inference only, like `forward_ragged`."""
        if self.training or torch.is_grad_enabled():
            raise RuntimeError("forward_infer_ragged is the inference forward: call it in eval mode (.eval()) under torch.no_grad() or torch.inference_mode()")
        if rb.n_bags == 0:
            return {t: torch.empty(0, n, dtype=torch.float32, device=rb.feats.device) for t, n in self.target_n_outs.items()}
        if not rb.feats.is_cuda or rb.feats.dim() != 2 or rb.feats.shape[1] != self.d_features or not rb.feats.is_contiguous() or rb.feats.dtype not in ops._DT:
            raise ValueError(f"packed bags must be a contiguous [tiles, {self.d_features}] f16 / bf16 / f32 tensor on the GPU")
        if self.positional_encoding and rb.coords is None:
            raise ValueError("positional_encoding=True needs the tile positions of every bag")
        return self._split_targets(self._ragged_call(rb), self._pack(rb.feats.device).no)

    # ---- training (the reference's `LitMilClassificationMixin.step`, barspoon.py:263-321) -------------------------------------------------
    def forward_train(self, tile_tokens: torch.Tensor, tile_positions: torch.Tensor, *, seed: int | None = None,
                      dropout: float | bool | None = None) -> dict[str, torch.Tensor]:
        """The train-mode forward, differentiable: `{target: logits}` whose `.backward()` fills `.grad` of every nn.Parameter in the reference's shapes
        (one torch.autograd.Function over the two library calls), so torch optimisers work on the module unchanged.  Dropout rate: the module's torch
        containers' (ValueError if they disagree); `dropout=False` switches every site off, a float overrides the rate.  `seed`: the step's mask seed
        (None: drawn from torch's CPU generator).  16-bit operands by torch's float32_matmul_precision: "medium" -> bf16, otherwise fp16 with a 2^10
        scale on dlogits that is undone in fp32; a non-finite fp16 result re-runs the step on bf16 operands (`fp16_overflow_events` counts them)."""
        if not tile_tokens.is_cuda:
            raise RuntimeError("HIP barspoon needs bags on the GPU (no CPU fallback)")
        if tile_tokens.dim() != 3 or tile_tokens.shape[-1] != self.d_features:
            raise ValueError(f"tile_tokens must be [batch, tile, {self.d_features}], got {tuple(tile_tokens.shape)}")
        Bb, T, _ = tile_tokens.shape
        if self.positional_encoding and (tile_positions is None or tuple(tile_positions.shape) != (Bb, T, 2)):
            raise ValueError(f"tile_positions must be [batch, tile, 2] = {(Bb, T, 2)}")
        p = dropout_rate(self)
        if dropout is False:
            p = 0.0
        elif dropout is not None and dropout is not True:
            p = float(dropout)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout rate {p} is outside [0, 1)")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0.0 else 0            # torch's CPU generator: reproducible under torch.manual_seed
        names = [n for n, _ in self.named_parameters()]
        params = [q for _, q in self.named_parameters()]
        pos = tile_positions if self.positional_encoding else None
        holder = _Holder()
        if torch.is_grad_enabled() and any(q.requires_grad for q in params):
            logits = _BarspoonFunction.apply(tile_tokens, pos, holder, self, p, int(seed), tuple(names), *params)
        else:
            with torch.no_grad():
                logits = _BarspoonFunction.forward(tile_tokens, pos, holder, self, p, int(seed), tuple(names), *params)
        out, col = {}, 0
        for t, n in self.target_n_outs.items():
            out[t] = logits[:, col:col + n]
            col += n
        return out


# ---- the training step's functional core: pack, forward, backward (each ONE library call) -----------------------------------------------------
class _Pack:
    """Device operands of one packing and the C structs over them (amds_barspoon_cfg, amds_barspoon_weights and what they point to): the encoder in the MIL
    `vit` head's padded pack, the decoder's fp32 tensors, each decoder layer's K | V projection padded and cast.  `train` (a training step): the encoder's
    pack carries W^T too, the K | V rows are padded to KVp and their transposed copies go into amds_barspoon_train_weights; without it (the deploy forward,
    `EncDecTransformer._pack`) `wc` is the plain amds_barspoon_weights.  `get(name)` -> fp32 device tensor of a parameter."""

    def __init__(self, model: EncDecTransformer, get, act: torch.dtype, dev, *, train: bool) -> None:
        self.act, self.dev = act, dev
        D, Hd, FF = model.d_model, model.num_decoder_heads, model.dim_feedforward
        self.dims = VitDims(F=model.d_features, D=D, H=model.num_encoder_heads, FF=FF, C=1, L=model.num_encoder_layers, alibi=False)
        g = lambda n: get(n).contiguous()  # noqa: E731
        self.pk = PackedVit(self.dims, model._enc_get(g, dev), act, train=train)
        self.pk.c_structs()
        enc_layers = self.pk._c[2]
        self.keep: list = []

        def T(t):
            self.keep.append(t)
            return t.data_ptr()

        Dp = self.dims.Dp
        Ld = model.num_decoder_layers
        self.dec = (_lib.BarspoonDecLayer * max(Ld, 1))()
        if train:
            self.KVp = _up(2 * 64 * Hd, 256)
            self.kvt = (C.c_void_p * max(Ld, 1))()
        for l in range(Ld):
            p = f"transformer_decoder.layers.{l}."
            w, b = g(p + "multihead_attn.in_proj_weight"), g(p + "multihead_attn.in_proj_bias")
            kvw, kvb = pad_kv_w(w[D:], Hd, D, Dp), pad_kv_b(b[D:], Hd, D)
            if train:
                kvw = F.pad(kvw, (0, 0, 0, self.KVp - kvw.shape[0])).contiguous()                            # [KVp][Dp], rows >= 2 Db zero
            kv16 = ops.cast_pad(kvw, Dp, act)
            fields = {k: T(g(p + n)) for k, n in _DEC_FP32}
            fields.update(ca_q_w=T(w[:D].contiguous()), ca_q_b=T(b[:D].contiguous()), ca_kv_w=T(kv16), ca_kv_b=T(kvb))
            self.dec[l] = _lib.BarspoonDecLayer(**fields)
            if train:
                self.kvt[l] = T(kv16.t().contiguous())                                                       # [Dp][KVp]
        labels = [sanitize(t) for t in model.target_labels]
        nt = len(labels)
        self.hw, self.hb, self.no = (C.c_void_p * nt)(), (C.c_void_p * nt)(), (C.c_int * nt)()
        for j, t in enumerate(labels):
            self.hw[j], self.hb[j], self.no[j] = T(g(f"heads.{t}.weight")), T(g(f"heads.{t}.bias")), model.heads[t].out_features
        self.total_out = sum(self.no)
        ct = torch.stack([g(f"class_tokens.{t}") for t in labels]).contiguous()
        pe = (100_000 ** (torch.arange(D // 4, dtype=torch.float32) / D)).to(dev).contiguous()              # :176-178, in torch's own fp32 arithmetic
        base = _lib.BarspoonWeights(self.pk.w["proj_w"].data_ptr(), self.pk.m["proj_b"].data_ptr(), enc_layers, T(ct), self.dec, self.hw, self.hb, self.no, T(pe))
        self.wc = _lib.BarspoonTrainWeights(base, self.kvt) if train else base
        self.cfg = _lib.BarspoonCfg(model.d_features, D, model.num_encoder_heads, Hd, FF, model.num_encoder_layers, Ld, nt, int(bool(model.positional_encoding)),
                                    ops.act_code(act))


class TrainPack(_Pack):
    """The pack of one training step (16-bit W and W^T of the encoder, K | V projections padded, cast and transposed)."""

    def __init__(self, model: EncDecTransformer, get, act: torch.dtype, dev) -> None:
        super().__init__(model, get, act, dev, train=True)
        self.model = model


def train_forward(pack: TrainPack, tile_tokens: torch.Tensor, tile_positions: torch.Tensor | None, *, p: float, seed: int):
    """-> (logits fp32 [Bb, sum n_out], saved).  ONE library call (amds_barspoon_train_forward); `saved` holds the activation arena the backward reads."""
    Bb, T, Fd = tile_tokens.shape
    dev = tile_tokens.device
    x = tile_tokens if tile_tokens.dtype in ops._DT else tile_tokens.float()
    x = x.contiguous()
    pos = tile_positions.to(dev, torch.float32).contiguous() if tile_positions is not None else None
    lib = _lib.lib()
    need = lib.amds_barspoon_train_saved_bytes(C.byref(pack.cfg), Bb, T)
    if need == 0:
        _lib.check(-1, "barspoon_train_saved_bytes")
    arena = ops.alloc(need, torch.uint8, dev)
    logits = ops.alloc((Bb, pack.total_out), torch.float32, dev)
    drop = _lib.BarspoonDropout(float(p), int(seed) & (2 ** 64 - 1))
    _lib.check(lib.amds_barspoon_train_forward(C.byref(pack.cfg), C.byref(pack.wc), x.data_ptr(), ops._DT[x.dtype], pos.data_ptr() if pos is not None else None,
                                               C.byref(drop), logits.data_ptr(), Bb, T, arena.data_ptr(), arena.numel(), ops._stream()), "barspoon_train_forward")
    return logits, dict(arena=arena, shape=(Bb, T, Fd), drop=drop)


def grad_layout(pack: TrainPack) -> list[tuple[str, tuple]]:
    """(key, padded shape) of every gradient buffer of amds_barspoon_grads, in the order of the flat buffer."""
    d, m = pack.dims, pack.model
    D, FF = m.d_model, m.dim_feedforward
    out = [("proj_w", (d.Dp, d.Fp)), ("proj_b", (d.Dp,)), ("class_tokens", (len(pack.no), D))]
    for l in range(d.L):
        out += [(f"enc{l}.{k}", sh) for k, sh in (("ln1_w", (D,)), ("ln1_b", (D,)), ("in_w", (3 * d.Da, d.Dp)), ("in_b", (3 * d.Da,)), ("out_w", (d.Dp, d.Da)),
                                                  ("out_b", (d.Dp,)), ("ln2_w", (D,)), ("ln2_b", (D,)), ("fc1_w", (d.FFp, d.Dp)), ("fc1_b", (d.FFp,)),
                                                  ("fc2_w", (d.Dp, d.FFp)), ("fc2_b", (d.Dp,)))]
    shapes = dict(ln1_w=(D,), ln1_b=(D,), sa_in_w=(3 * D, D), sa_in_b=(3 * D,), sa_out_w=(D, D), sa_out_b=(D,), ln2_w=(D,), ln2_b=(D,), ca_q_w=(D, D), ca_q_b=(D,),
                  ca_kv_w=(pack.KVp, d.Dp), ca_kv_b=(pack.KVp,), ca_out_w=(D, D), ca_out_b=(D,), ln3_w=(D,), ln3_b=(D,), fc1_w=(FF, D), fc1_b=(FF,), fc2_w=(D, FF),
                  fc2_b=(D,))
    for l in range(m.num_decoder_layers):
        out += [(f"dec{l}.{k}", shapes[k]) for k, _ in _lib.BarspoonDecLayerGrads._fields_]
    for j in range(len(pack.no)):
        out += [(f"head{j}.w", (pack.no[j], D)), (f"head{j}.b", (pack.no[j],))]
    return out


def unpad_grads(pack: TrainPack, B: dict) -> dict[str, torch.Tensor]:
    """Padded gradient buffers (grad_layout's keys) -> {parameter name: gradient in the reference's shape}: padding sliced off, the query scale of padded
    encoder heads undone (PackedVit.unpad_*)."""
    m, d, pk = pack.model, pack.dims, pack.pk
    D, FF, Fd, Hd = m.d_model, m.dim_feedforward, m.d_features, m.num_decoder_heads
    G = {"projector.0.weight": B["proj_w"][:D, :Fd], "projector.0.bias": B["proj_b"][:D]}
    for l in range(d.L):
        p, e = f"transformer_encoder.layers.{l}.", f"enc{l}."
        G[p + "self_attn.in_proj_weight"] = pk.unpad_in_w(B[e + "in_w"]).reshape(3 * D, D)
        G[p + "self_attn.in_proj_bias"] = pk.unpad_in_b(B[e + "in_b"]).reshape(3 * D)
        G[p + "self_attn.out_proj.weight"], G[p + "self_attn.out_proj.bias"] = pk.unpad_out_w(B[e + "out_w"]), B[e + "out_b"][:D]
        G[p + "linear1.weight"], G[p + "linear1.bias"] = B[e + "fc1_w"][:FF, :D], B[e + "fc1_b"][:FF]
        G[p + "linear2.weight"], G[p + "linear2.bias"] = B[e + "fc2_w"][:D, :FF], B[e + "fc2_b"][:D]
        G[p + "norm1.weight"], G[p + "norm1.bias"], G[p + "norm2.weight"], G[p + "norm2.bias"] = B[e + "ln1_w"], B[e + "ln1_b"], B[e + "ln2_w"], B[e + "ln2_b"]
    for j, t in enumerate(m.target_labels):
        t = sanitize(t)
        G[f"class_tokens.{t}"] = B["class_tokens"][j]
        G[f"heads.{t}.weight"], G[f"heads.{t}.bias"] = B[f"head{j}.w"], B[f"head{j}.b"]
    for l in range(m.num_decoder_layers):
        p, e = f"transformer_decoder.layers.{l}.", f"dec{l}."
        for k, n in _DEC_FP32:
            G[p + n] = B[e + k]
        G[p + "multihead_attn.in_proj_weight"] = torch.cat([B[e + "ca_q_w"], unpad_kv_w(B[e + "ca_kv_w"], Hd, D)])
        G[p + "multihead_attn.in_proj_bias"] = torch.cat([B[e + "ca_q_b"], unpad_kv_b(B[e + "ca_kv_b"], Hd, D)])
    return G


def train_backward(pack: TrainPack, saved: dict, dlogits: torch.Tensor, *, split_k: int = 32, unscale: float = 1.0) -> dict[str, torch.Tensor]:
    """-> {parameter name: fp32 gradient in the reference's shape}.  ONE library call (amds_barspoon_train_backward) into one flat padded buffer.
    `unscale`: the power of two dlogits carries (fp16 operands); the padded buffers are divided by it in fp32 before they are sliced."""
    Bb, T, _ = saved["shape"]
    dev = dlogits.device
    dlogits = dlogits.contiguous().float()
    if tuple(dlogits.shape) != (Bb, pack.total_out):
        raise ValueError(f"dlogits must be {(Bb, pack.total_out)}, got {tuple(dlogits.shape)}")
    lib = _lib.lib()
    need = lib.amds_barspoon_train_workspace_bytes(C.byref(pack.cfg), Bb, T, split_k)
    if need == 0:
        _lib.check(-1, "barspoon_train_workspace_bytes")
    ws = ops.scratch("barspoon_train", dev, need)
    layout = grad_layout(pack)
    al = lambda n: (n + 63) // 64 * 64  # noqa: E731   (256-byte aligned sub-buffers)
    flat = ops.alloc(sum(al(math.prod(sh)) for _, sh in layout), torch.float32, dev)
    B, off = {}, 0
    for k, sh in layout:
        n = math.prod(sh)
        B[k] = flat[off:off + n].view(sh)
        off += al(n)
    d, m = pack.dims, pack.model
    eg = (_lib.MilVitLayerGrads * max(d.L, 1))()
    for l in range(d.L):
        eg[l] = _lib.MilVitLayerGrads(**{k: B[f"enc{l}.{k}"].data_ptr() for k, _ in _lib.MilVitLayerGrads._fields_ if k != "bias_scale"})
    dg = (_lib.BarspoonDecLayerGrads * max(m.num_decoder_layers, 1))()
    for l in range(m.num_decoder_layers):
        dg[l] = _lib.BarspoonDecLayerGrads(**{k: B[f"dec{l}.{k}"].data_ptr() for k, _ in _lib.BarspoonDecLayerGrads._fields_})
    nt = len(pack.no)
    hw, hb = (C.c_void_p * nt)(), (C.c_void_p * nt)()
    for j in range(nt):
        hw[j], hb[j] = B[f"head{j}.w"].data_ptr(), B[f"head{j}.b"].data_ptr()
    gc = _lib.BarspoonGrads(B["proj_w"].data_ptr(), B["proj_b"].data_ptr(), eg, B["class_tokens"].data_ptr(), dg, hw, hb)
    arena = saved["arena"]
    _lib.check(lib.amds_barspoon_train_backward(C.byref(pack.cfg), C.byref(pack.wc), dlogits.data_ptr(), C.byref(saved["drop"]), Bb, T, arena.data_ptr(), arena.numel(),
                                                C.byref(gc), split_k, ws.data_ptr(), ws.numel(), ops._stream()), "barspoon_train_backward")
    if unscale != 1.0:
        torch._foreach_mul_(list(B.values()), 1.0 / unscale)
    return unpad_grads(pack, B)


class _Holder:
    """Carrier of the forward's pack and saved activations to the backward (a non-tensor input of the Function)."""
    pack = None
    saved = None
    loss_scale = 1.0
    rerun_bf16 = None


def _finite(ts) -> bool:
    """One device-to-host read: are all values of these tensors finite?  (a norm is non-finite as soon as one element is)"""
    return bool(torch.isfinite(torch.stack(torch._foreach_norm(list(ts)))).all())


class _BarspoonFunction(torch.autograd.Function):
    @staticmethod
    def forward(x, pos, holder, model, p, seed, names, *params):
        P = dict(zip(names, params))
        dev = x.device
        get = lambda n: P[n].detach().to(dev, torch.float32)  # noqa: E731
        # operand type by torch's own flag, as the MIL `vit` head: "medium" -> bf16; "high" (the reference's training setting, train.py:519) / "highest" -> fp16
        act = torch.bfloat16 if torch.get_float32_matmul_precision() == "medium" else torch.float16

        def run(dt):
            pack = TrainPack(model, get, dt, dev)
            return (pack, *train_forward(pack, x.detach(), None if pos is None else pos.detach(), p=p, seed=seed))

        pack, logits, saved = run(act)
        if act == torch.float16 and not _finite([logits]):          # an fp16 activation overflowed: the same step (same masks) on bf16 operands
            model.fp16_overflow_events += 1
            act = torch.bfloat16
            pack, logits, saved = run(act)
        holder.pack, holder.saved, holder.loss_scale, holder.model = pack, saved, (1.0 if act == torch.bfloat16 else 1024.0), model
        holder.rerun_bf16 = (lambda: run(torch.bfloat16)) if act == torch.float16 else None
        return logits

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.holder, ctx.names = inputs[2], inputs[6]

    @staticmethod
    def backward(ctx, dlogits):
        h = ctx.holder
        sc = h.loss_scale
        G = train_backward(h.pack, h.saved, dlogits * sc if sc != 1.0 else dlogits, unscale=sc)      # un-scaled in fp32
        if sc != 1.0:
            if not _finite(G.values()):                               # an fp16 gradient overflowed: this step on bf16 operands (fp32's range)
                h.model.fp16_overflow_events += 1
                h.pack, _, h.saved = h.rerun_bf16()
                h.loss_scale = 1.0
                G = train_backward(h.pack, h.saved, dlogits)
        gp = [G[n].contiguous() if ctx.needs_input_grad[7 + i] else None for i, n in enumerate(ctx.names)]
        return (None, None, None, None, None, None, None, *gp)


def step_masks(model: EncDecTransformer, Bb: int, T: int, p: float, seed: int, device) -> dict[str, torch.Tensor]:
    """Every keep mask of one training step, rebuilt from (p, seed, shapes) with the library's own generators, in the reference's shapes (padding sliced
    off) -- for parity tests.  Keys: enc{l}.attn [Bb, He, T, T], enc{l}.ff1 [Bb, T, FF], enc{l}.ff2 / enc{l}.sa [Bb, T, D]; dec{l}.attn [Bb, Hd, nt, nt],
    dec{l}.sa / .ca / .ff2 [Bb, nt, D], dec{l}.cattn [Bb, Hd, nt, T], dec{l}.ff1 [Bb, nt, FF] (stream ids: include/amdstamp.h, barspoon training)."""
    from . import train_ops as Tr
    D, FF, He, Hd, nt = model.d_model, model.dim_feedforward, model.num_encoder_heads, model.num_decoder_heads, len(model.target_n_outs)
    Dp, FFp, Ha = _up(D, 256), _up(FF, 256), _up(He, 4)
    flat = lambda rows, cols, keep, sid: Tr.dropout_mask(Bb * rows * cols, p, seed, sid, device).view(Bb, rows, cols)[..., :keep].bool()  # noqa: E731
    out = {}
    for l in range(model.num_encoder_layers):
        out[f"enc{l}.attn"] = Tr.attention_dropout_mask(Bb, Ha, T, p, seed, 10 * l + 1, device)[:, :He].bool()
        out[f"enc{l}.ff1"], out[f"enc{l}.ff2"], out[f"enc{l}.sa"] = flat(T, FFp, FF, 10 * l + 2), flat(T, Dp, D, 10 * l + 3), flat(T, Dp, D, 10 * l + 4)
    for l in range(model.num_decoder_layers):
        s = 5000 + 10 * l
        out[f"dec{l}.attn"] = Tr.attention_dropout_mask_rows(Bb * Hd * nt, nt, p, seed, s + 1, device).view(Bb, Hd, nt, nt).bool()
        out[f"dec{l}.cattn"] = Tr.attention_dropout_mask_rows(Bb * Hd * nt, T, p, seed, s + 3, device).view(Bb, Hd, nt, T).bool()
        out[f"dec{l}.sa"], out[f"dec{l}.ca"], out[f"dec{l}.ff2"] = flat(nt, D, D, s + 2), flat(nt, D, D, s + 4), flat(nt, D, D, s + 6)
        out[f"dec{l}.ff1"] = flat(nt, FF, FF, s + 5)
    return out
