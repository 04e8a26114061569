"""The gated-attention MIL head on the HIP path: `GatedAttentionMIL` (module) and `HipAbmilTrainer` (flat-buffer trainer).

The network is CHIEF's `CHIEFModel` used as a classifier (reference src/stamp/encoding/encoder/chief.py:27-89, `Attn_Net_Gated` :255-275), a CLAM-SB style
attention-MIL head: ``Linear(F, L) -> ReLU -> Dropout(0.25) -> Attn_Net_Gated(L, D)`` gives a score per tile and the transformed tiles h; softmax over the
tiles (:77-79); ``WSI_feature_transformed = A @ h`` (:80) feeds ``classifiers = Linear(L, n_classes)`` (:56).  The parameter tree and its state-dict keys are
the reference's (`attention_net.0.*`, `attention_net.3.attention_{a,b}.0.*`, `attention_net.3.attention_c.*`, `classifiers.*`), so CHIEF's pretrained attention
network loads (`from_chief`) and can be fine-tuned on a cohort.  Out of scope: the un-gated `Attn_Net`, the instance classifiers, CHIEF's text branch.

Everything runs in the library (csrc/abmil.hip): `amds_abmil_forward` (eval), `amds_abmil_train_forward` / `amds_abmil_train_backward` (ONE call each),
`amds_abmil_heatmap` (`heatmap_scores`: logits, attention, Grad-CAM of all classes and per-tile logits of one or many slides in ONE call).
Every call is ragged by construction -- packed rows plus int64 row offsets --, a dense [B, N, F] batch is equal offsets.  The three products per row follow
`torch.get_float32_matmul_precision()` exactly as TransMIL does ("highest": exact fp32 MFMA; below: bf16 x 3, `ops.sync_float32_matmul_precision`).  A bag's
eval logits do not depend on what else is in the call, at every length (include/amdstamp.h), so `forward_ragged` groups by count and rows alone.
Dropout: the reference's three sites (h, tanh branch, sigmoid branch; p = 0.25) with the library's counter-based masks, stream ids 1, 2, 3
(`dropout_masks` reads them back).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib, mil_core, ops
from . import train_ops as T
from .flat_trainer import FlatTrainer

CHIEF_SIZES = {"xs": (384, 256, 256), "small": (768, 512, 256), "big": (1024, 512, 384), "large": (2048, 1024, 512)}      # chief.py:38-43
# amds_abmil_weights field -> state-dict key
KEYS = {"fc_w": "attention_net.0.weight", "fc_b": "attention_net.0.bias",
        "a_w": "attention_net.3.attention_a.0.weight", "a_b": "attention_net.3.attention_a.0.bias",
        "b_w": "attention_net.3.attention_b.0.weight", "b_b": "attention_net.3.attention_b.0.bias",
        "c_w": "attention_net.3.attention_c.weight", "c_b": "attention_net.3.attention_c.bias",
        "cls_w": "classifiers.weight", "cls_b": "classifiers.bias"}
MAX_ROWS_PER_CALL = 65535 * 64 - 256          # include/amdstamp.h: the rows one library call takes


def _cfg(dims) -> "_lib.AbmilCfg":
    return _lib.AbmilCfg(*[int(v) for v in dims])


def _need(fn, cfg, bags: int, rows: int, what: str) -> int:
    n = fn(C.byref(cfg), int(bags), int(rows))
    if n == 0:
        _lib.check(-1, what)
    return n


def _weights_struct(get) -> tuple["_lib.AbmilWeights", dict]:
    """amds_abmil_weights over contiguous fp32 device tensors; `get(key)` returns one.  The dict keeps them alive."""
    w, keep = _lib.AbmilWeights(), {}
    for field, key in KEYS.items():
        t = get(key)
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
        keep[key] = t
        setattr(w, field, t.data_ptr())
    return w, keep


def _offsets(lengths, dev) -> torch.Tensor:
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + int(n))
    return torch.tensor(offs, dtype=torch.int64).to(dev)


def _drop_struct(p_fc: float, p_gate: float, seed: int) -> "_lib.AbmilDropout":
    return _lib.AbmilDropout(float(p_fc), float(p_gate), int(seed) & (2 ** 64 - 1))


def _rows(x: torch.Tensor, dims) -> torch.Tensor:
    ops._dev(x)
    if x.dim() != 2 or x.shape[1] != dims[0]:
        raise ValueError(f"packed rows must be [rows, {dims[0]}], got {tuple(x.shape)}")
    if x.dtype not in ops._DT:
        x = x.float()
    return x.contiguous()


def forward_infer(w, dims, x: torch.Tensor, offsets: torch.Tensor, n_bags: int, *, return_attn: bool = False, return_pooled: bool = False):
    """Packed rows [rows, F] + int64 device offsets [n_bags + 1] -> logits [n_bags, C] (+ raw scores [rows], pooled [n_bags, L]): amds_abmil_forward."""
    x = _rows(x, dims)
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    ws = ops.scratch("abmil", dev, _need(lib.amds_abmil_workspace_bytes, cfg, n_bags, rows, "abmil_workspace_bytes"))
    logits = torch.empty(n_bags, dims[3], dtype=torch.float32, device=dev)
    attn = torch.empty(rows, dtype=torch.float32, device=dev) if return_attn else None
    pooled = torch.empty(n_bags, dims[1], dtype=torch.float32, device=dev) if return_pooled else None
    ops.sync_float32_matmul_precision()
    _lib.check(lib.amds_abmil_forward(C.byref(cfg), C.byref(w), x.data_ptr(), ops._DT[x.dtype], offsets.data_ptr(), n_bags, rows, logits.data_ptr(), ops._p(attn),
                                      ops._p(pooled), ws.data_ptr(), ws.numel(), ops._stream()), "abmil_forward")
    out = (logits,) + ((attn,) if return_attn else ()) + ((pooled,) if return_pooled else ())
    return out if len(out) > 1 else logits


def heatmap_scores(w, dims, x: torch.Tensor, offsets: torch.Tensor, n_bags: int, *, want_cam: bool = True, want_tiles: bool = True) -> dict:
    """Packed rows [rows, F] + int64 device offsets [n_bags + 1] -> dict(logits [n_bags, C], attn_raw [rows], probs [rows] (the softmax weights),
    cam_raw [C, rows] or None, tile_logits [rows, C] or None) in ONE library call (amds_abmil_heatmap): the eval forward's bits, the Grad-CAM scores of all
    classes before the softmax over the tiles (reference src/stamp/heatmaps/__init__.py:43-54) in closed form, and every tile's logits as a bag of its own
    (:417-427).  An output that is not wanted costs nothing."""
    x = _rows(x, dims)
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    ws = ops.scratch("abmil_heatmap", dev, _need(lib.amds_abmil_heatmap_workspace_bytes, cfg, n_bags, rows, "abmil_heatmap_workspace_bytes"))
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"logits": new(n_bags, dims[3]), "attn_raw": new(rows), "probs": new(rows), "cam_raw": new(dims[3], rows) if want_cam else None,
           "tile_logits": new(rows, dims[3]) if want_tiles else None}
    ops.sync_float32_matmul_precision()
    _lib.check(lib.amds_abmil_heatmap(C.byref(cfg), C.byref(w), x.data_ptr(), ops._DT[x.dtype], offsets.data_ptr(), n_bags, rows, out["logits"].data_ptr(),
                                      out["attn_raw"].data_ptr(), out["probs"].data_ptr(), ops._p(out["cam_raw"]), ops._p(out["tile_logits"]), ws.data_ptr(), ws.numel(),
                                      ops._stream()), "abmil_heatmap")
    return out


def forward_train(w, dims, x: torch.Tensor, offsets: torch.Tensor, n_bags: int, *, p_fc: float, p_gate: float, seed: int):
    """-> (logits [n_bags, C], saved): amds_abmil_train_forward.  `saved` holds what `backward` needs (the arena, the rows themselves, the dropout setting)."""
    x = _rows(x, dims)
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    arena = ops.alloc(_need(lib.amds_abmil_train_saved_bytes, cfg, n_bags, rows, "abmil_train_saved_bytes"), torch.uint8, dev)
    ws = ops.scratch("abmil_train", dev, _need(lib.amds_abmil_train_workspace_bytes, cfg, n_bags, rows, "abmil_train_workspace_bytes"))
    logits = torch.empty(n_bags, dims[3], dtype=torch.float32, device=dev)
    drop = _drop_struct(p_fc, p_gate, seed)
    ops.sync_float32_matmul_precision()
    _lib.check(lib.amds_abmil_train_forward(C.byref(cfg), C.byref(w), x.data_ptr(), ops._DT[x.dtype], offsets.data_ptr(), n_bags, rows, C.byref(drop), logits.data_ptr(),
                                            arena.data_ptr(), arena.numel(), ws.data_ptr(), ws.numel(), ops._stream()), "abmil_train_forward")
    return logits, dict(arena=arena, x=x, offsets=offsets, n_bags=n_bags, dims=tuple(dims), w=w, drop=drop)


def backward(saved: dict, dlogits: torch.Tensor, *, grads: "_lib.AbmilGrads | None" = None, need_params: bool = True, need_x: bool = False):
    """amds_abmil_train_backward.  grads: an amds_abmil_grads over the caller's buffers (the trainer's flat G); without one and need_params, fresh tensors are
    returned by state-dict key.  -> (G or None, dx [rows, F] or None)."""
    x, dims, n_bags = saved["x"], saved["dims"], saved["n_bags"]
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    Fd, L, D, Cc = dims
    G = None
    if grads is None and need_params:
        shapes = {"fc_w": (L, Fd), "fc_b": (L,), "a_w": (D, L), "a_b": (D,), "b_w": (D, L), "b_b": (D,), "c_w": (1, D), "c_b": (1,), "cls_w": (Cc, L), "cls_b": (Cc,)}
        G = {KEYS[f]: ops.alloc(s, torch.float32, dev) for f, s in shapes.items()}
        grads = _lib.AbmilGrads()
        for f in shapes:
            setattr(grads, f, G[KEYS[f]].data_ptr())
    dx = ops.alloc((rows, Fd), torch.float32, dev) if need_x else None
    ws = ops.scratch("abmil_train", dev, _need(lib.amds_abmil_train_workspace_bytes, cfg, n_bags, rows, "abmil_train_workspace_bytes"))
    dlogits = dlogits.detach().to(dev, torch.float32).contiguous()
    ops.sync_float32_matmul_precision()
    _lib.check(lib.amds_abmil_train_backward(C.byref(cfg), C.byref(saved["w"]), x.data_ptr(), ops._DT[x.dtype], saved["offsets"].data_ptr(), n_bags, rows,
                                             C.byref(saved["drop"]), dlogits.data_ptr(), saved["arena"].data_ptr(), saved["arena"].numel(),
                                             C.byref(grads) if grads is not None else None, ops._p(dx), ws.data_ptr(), ws.numel(), ops._stream()), "abmil_train_backward")
    return G, dx


def dropout_masks(rows: int, dims, p_fc: float, p_gate: float, seed: int, device="cuda") -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The keep masks (0/1, uint8) of a training call over `rows` packed rows: ([rows, L] for h, [rows, D] for a, [rows, D] for g), read back through
    amds_dropout_mask with the head's stream ids 1, 2, 3.  The multipliers are mask * amds_dropout_keep_scale(p)."""
    _, L, D, _ = dims
    return (T.dropout_mask(rows * L, p_fc, seed, 1, device).view(rows, L), T.dropout_mask(rows * D, p_gate, seed, 2, device).view(rows, D),
            T.dropout_mask(rows * D, p_gate, seed, 3, device).view(rows, D))


class _Holder:
    saved = None


class _AbmilFunction(torch.autograd.Function):
    """logits = f(rows, parameters) over the two training calls."""

    @staticmethod
    def forward(x, offsets, n_bags, model, p, seed, holder, *params):
        dev = x.device
        P = dict(zip([n for n, _ in model.named_parameters()], params))
        w, _keep = _weights_struct(lambda k: P[k].detach().to(dev, torch.float32).contiguous())
        logits, saved = forward_train(w, model.dims, x.detach(), offsets, n_bags, p_fc=p, p_gate=p, seed=seed)
        saved["keep"] = _keep
        holder.saved = saved
        return logits

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.holder, ctx.names = inputs[6], tuple(n for n, _ in inputs[3].named_parameters())
        ctx.x_dtype = inputs[0].dtype

    @staticmethod
    def backward(ctx, dlogits):
        need_x = ctx.needs_input_grad[0]
        need_params = any(ctx.needs_input_grad[7:])
        if not (need_x or need_params):
            return (None,) * (7 + len(ctx.names))
        G, dx = backward(ctx.holder.saved, dlogits, need_params=need_params, need_x=need_x)
        gp = [G[n] if need_params and ctx.needs_input_grad[7 + i] else None for i, n in enumerate(ctx.names)]
        return (dx.to(ctx.x_dtype) if need_x else None, None, None, None, None, None, None, *gp)


class _AttnNetGatedParams(nn.Module):
    """The parameter tree of the reference's `Attn_Net_Gated` (chief.py:255-275): attention_a / attention_b are Sequentials whose entry 0 is the Linear."""

    def __init__(self, L: int, D: int) -> None:
        super().__init__()
        self.attention_a = nn.Sequential(nn.Linear(L, D))
        self.attention_b = nn.Sequential(nn.Linear(L, D))
        self.attention_c = nn.Linear(D, 1)


class GatedAttentionMIL(nn.Module):
    """CHIEF's gated attention network as a MIL classifier head on the HIP path (module docstring).  State-dict keys = the reference's `CHIEFModel`
    restricted to `attention_net.*` and `classifiers.*`; initialisation as its `initialize_weights` (Xavier-normal weights, zero biases)."""

    def __init__(self, dim_input: int, dim_hidden: int = 512, dim_attention: int = 256, dim_output: int = 2, dropout: float = 0.25) -> None:
        super().__init__()
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must lie in [0, 1)")
        # entries 1 and 2 of the reference's Sequential are ReLU and Dropout: no parameters, kept so that entry 3 is the gated attention net
        self.attention_net = nn.Sequential(nn.Linear(dim_input, dim_hidden), nn.ReLU(), nn.Dropout(dropout), _AttnNetGatedParams(dim_hidden, dim_attention))
        self.classifiers = nn.Linear(dim_hidden, dim_output)
        self.dims = (dim_input, dim_hidden, dim_attention, dim_output)
        self.n_classes = dim_output
        self.dropout = float(dropout)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight)
                nn.init.zeros_(m.bias)

    @classmethod
    def from_chief(cls, size_arg: str, state_dict: dict, dim_output: int = 2, dropout: float = 0.25) -> "GatedAttentionMIL":
        """CHIEF's checkpoint (or any dict holding its `attention_net.*` tensors) -> a head of that geometry: the attention network is loaded; `classifiers.*`
        is kept when its shape fits [dim_output, L] and stays freshly initialised otherwise; every other key (instance classifiers, text branch) is ignored."""
        if size_arg not in CHIEF_SIZES:
            raise ValueError(f"size_arg must be one of {sorted(CHIEF_SIZES)}, got {size_arg!r}")
        Fd, L, D = CHIEF_SIZES[size_arg]
        model = cls(Fd, L, D, dim_output, dropout)
        own = model.state_dict()
        load = {}
        for k, v in own.items():
            if k not in state_dict:
                if k.startswith("attention_net."):
                    raise KeyError(f"state_dict lacks {k}")
                continue
            t = torch.as_tensor(state_dict[k])
            if tuple(t.shape) != tuple(v.shape):
                if k.startswith("attention_net."):
                    raise ValueError(f"{k}: shape {tuple(t.shape)} does not fit size_arg {size_arg!r} ({tuple(v.shape)})")
                continue
            load[k] = t.to(v.dtype)
        if ("classifiers.weight" in load) != ("classifiers.bias" in load):
            load.pop("classifiers.weight", None), load.pop("classifiers.bias", None)
        own.update(load)
        model.load_state_dict(own)
        return model

    def _c_weights(self, dev):
        """amds_abmil_weights over fp32 device copies of the parameters, rebuilt when a parameter changed (version counters)."""
        tensors = dict(self.named_parameters())
        key = (str(dev), tuple((t.data_ptr(), t._version) for t in tensors.values()))
        if getattr(self, "_cw_key", None) != key:
            self._cw, self._cw_keep = _weights_struct(lambda k: tensors[k].detach().to(dev, torch.float32).contiguous())
            self._cw_key = key
        return self._cw

    def _check_infer(self, what: str) -> None:
        if self.training or torch.is_grad_enabled():
            raise RuntimeError(f"{what} is the inference forward: call it in eval mode (.eval()) under torch.no_grad() or torch.inference_mode()")

    def forward(self, bags: torch.Tensor, coords: torch.Tensor | None = None, mask: torch.Tensor | None = None) -> torch.Tensor:
        """bags [B, N, F] -> logits [B, dim_output].  `coords` is accepted and ignored (the network has no positional term).  `mask` is refused: the
        reference's network has none, and ragged bags go through `forward_ragged`.  eval + no_grad: amds_abmil_forward; otherwise ONE autograd.Function over
        the two training calls (dropout live in train mode), `loss.backward()` fills `.grad` and, when `bags` requires it, `bags.grad`."""
        if mask is not None:
            raise ValueError("GatedAttentionMIL takes no mask: bags of different lengths go through forward_ragged (a list of [N_i, F] tensors)")
        if not bags.is_cuda:
            raise RuntimeError("HIP GatedAttentionMIL needs bags on the GPU (no CPU fallback)")
        if bags.dim() != 3 or bags.shape[-1] != self.dims[0]:
            raise ValueError(f"bags must be [batch, tile, {self.dims[0]}], got {tuple(bags.shape)}")
        B, N, Fd = bags.shape
        if B < 1 or N < 1:
            raise ValueError("empty batch or empty bag")
        offsets = _offsets([N] * B, bags.device)
        x = bags.reshape(B * N, Fd)
        need_grad = torch.is_grad_enabled() and (bags.requires_grad or any(p.requires_grad for p in self.parameters()))
        if self.training or need_grad:
            live = self.training and self.dropout > 0
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if live else 0
            args = (x, offsets, B, self, self.dropout if live else 0.0, seed, _Holder(), *[p for _, p in self.named_parameters()])
            if need_grad:
                return _AbmilFunction.apply(*args)
            with torch.no_grad():
                return _AbmilFunction.forward(*args)
        return forward_infer(self._c_weights(bags.device), self.dims, x, offsets, B)

    def forward_infer_ragged(self, rb: "mil_core.RaggedBags") -> torch.Tensor:
        """Bags that are already packed (`mil_core.pack_bags`, `ResidentCohort.ragged_group`) -> logits [n_bags, dim_output] in ONE library call."""
        self._check_infer("forward_infer_ragged")
        if rb.n_bags == 0:
            return torch.empty(0, self.n_classes, dtype=torch.float32, device=rb.feats.device)
        return forward_infer(self._c_weights(rb.feats.device), self.dims, rb.feats, rb.offsets.to(torch.int64), rb.n_bags)

    def forward_ragged(self, bags, coords=None, *, bags_per_call: int | None = None, max_rows_per_call: int = MAX_ROWS_PER_CALL) -> torch.Tensor:
        """Bags of DIFFERENT lengths: a list of [N_i, dim_input] tensors -> logits [len(bags), dim_output] in the list's order, row i bit-identical to bag i's
        own call.  At most `bags_per_call` bags and `max_rows_per_call` rows per library call (`mil_core.group_bags` with no class-token row and no
        shared-length limit beyond its own; default: as few calls as the library's row limit allows).  `coords` is accepted and ignored."""
        self._check_infer("forward_ragged")
        bags = list(bags)
        lengths = mil_core._validate_bags(bags, None, self.dims[0], False)
        if not bags:
            return torch.empty(0, self.n_classes, dtype=torch.float32, device=next(self.parameters()).device)
        if not bags[0].is_cuda:
            raise RuntimeError("HIP GatedAttentionMIL needs bags on the GPU (no CPU fallback)")
        outs = []
        for a, e in group_bags(lengths, bags_per_call or len(bags), max_rows_per_call):
            outs.append(self.forward_infer_ragged(mil_core.pack_bags(bags[a:e], n_feats=self.dims[0])))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def heatmap_scores(self, bags, *, want_cam: bool = True, want_tiles: bool = True, bags_per_call: int | None = None,
                       max_rows_per_call: int = MAX_ROWS_PER_CALL) -> dict:
        """One slide [N, dim_input] or a list of slides [N_i, dim_input] -> the dict of `heatmap_scores` over the slides' rows back to back (logits
        [slides, C], attn_raw / probs [rows], cam_raw [C, rows], tile_logits [rows, C]), one library call per group of `forward_ragged`'s grouping (default: as
        few calls as the library's row limit allows).  A slide's values are bit for bit those of its own call.  eval + no_grad only, like `forward_ragged`."""
        self._check_infer("heatmap_scores")
        bags = [bags] if isinstance(bags, torch.Tensor) else list(bags)
        lengths = mil_core._validate_bags(bags, None, self.dims[0], False)
        if not bags:
            raise ValueError("heatmap_scores needs at least one slide")
        if not bags[0].is_cuda:
            raise RuntimeError("HIP GatedAttentionMIL needs bags on the GPU (no CPU fallback)")
        outs = []
        for a, e in group_bags(lengths, bags_per_call or len(bags), max_rows_per_call):
            x = bags[a] if e - a == 1 else mil_core.pack_bags(bags[a:e], n_feats=self.dims[0]).feats
            outs.append(heatmap_scores(self._c_weights(x.device), self.dims, x, _offsets(lengths[a:e], x.device), e - a, want_cam=want_cam, want_tiles=want_tiles))
        if len(outs) == 1:
            return outs[0]
        cat = {"logits": 0, "attn_raw": 0, "probs": 0, "cam_raw": 1, "tile_logits": 0}
        return {k: None if outs[0][k] is None else torch.cat([o[k] for o in outs], dim=d) for k, d in cat.items()}

    @torch.no_grad()
    def attention(self, bag: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """One bag [N, dim_input] -> (softmax weights [N], raw scores [N]) of the eval forward (what CHIEF reports as `attention_raw`, chief.py:77-84)."""
        if bag.dim() != 2:
            raise ValueError(f"bag must be [tiles, {self.dims[0]}], got {tuple(bag.shape)}")
        _, raw = forward_infer(self._c_weights(bag.device), self.dims, bag, _offsets([bag.shape[0]], bag.device), 1, return_attn=True)
        return torch.softmax(raw, dim=0), raw


def group_bags(lengths, bags_per_call: int, max_rows_per_call: int = MAX_ROWS_PER_CALL) -> list[tuple[int, int]]:
    """Consecutive bags -> [start, end) groups of one library call each: `mil_core.group_bags` without a class-token row, rows capped at the library's limit.
    A bag's logits do not depend on its group, so the grouping is a matter of memory alone."""
    return mil_core.group_bags(lengths, bags_per_call, min(int(max_rows_per_call), MAX_ROWS_PER_CALL), mil_core.MAX_SOLO_TILES, 0)


class HipAbmilTrainer(FlatTrainer):
    """Training of `GatedAttentionMIL` without autograd through the network: the `flat_trainer.FlatTrainer` of this head (the flat `P` / `G` / `m` / `v`
    buffers, their views, the step protocol and the schedule are described there).  One `step` runs around amds_abmil_train_forward / _backward;
    amds_abmil_weights / amds_abmil_grads are built ONCE over the views (the library asks for no alignment of a weight or gradient tensor), so there is nothing
    to refresh after a step.  fp32's range throughout: no loss scale.  `mil_train.fit` is the epoch loop."""

    valid_max_rows_per_call = 262144

    def __init__(self, model: GatedAttentionMIL, *, device="cuda", max_lr: float = 1e-4, div_factor: float = 25.0, total_steps: int = 1000,
                 weight_decay: float = 0.01, dropout: bool | None = None, sched_interval: str = "epoch") -> None:
        """dropout: None = the module's rate at all three sites (train mode); False = off (deterministic steps)."""
        super().__init__(model, device, max_lr=max_lr, div_factor=div_factor, total_steps=total_steps, weight_decay=weight_decay, sched_interval=sched_interval)
        self.dims = tuple(model.dims)
        self.p_drop = model.dropout if (dropout is None or dropout) else 0.0
        if self.dev.type == "cuda":
            self._w, self._w_keep = _weights_struct(self.p)
            self._gc = _lib.AbmilGrads()
            for field, key in KEYS.items():
                setattr(self._gc, field, self.g(key).data_ptr())

    def _check(self, bags: torch.Tensor) -> None:
        if not bags.is_cuda:
            raise RuntimeError("HipAbmilTrainer needs bags on the GPU (no CPU fallback)")
        if bags.shape[-1] != self.dims[0]:
            raise ValueError(f"bags must be [..., {self.dims[0]}], got {tuple(bags.shape)}")

    @property
    def dropout_live(self) -> bool:
        return self.p_drop > 0

    def _check_bags(self, bags: torch.Tensor) -> None:
        """bags [Bb, T, F] fp16 / bf16 / fp32 on the GPU (taken as stored: the library converts while it stages)."""
        if bags.dim() != 3:
            raise ValueError(f"bags must be [batch, tile, {self.dims[0]}], got {tuple(bags.shape)}")
        self._check(bags)

    def _forward_train(self, bags, coords, seed):
        Bb, Tn, Fd = bags.shape
        return forward_train(self._w, self.dims, bags.reshape(Bb * Tn, Fd), _offsets([Tn] * Bb, self.dev), Bb, p_fc=self.p_drop, p_gate=self.p_drop, seed=seed)

    def _backward(self, saved, dlogits) -> None:
        backward(saved, dlogits, grads=self._gc)

    @torch.no_grad()
    def predict(self, bags: torch.Tensor, coords: torch.Tensor | None = None) -> torch.Tensor:
        """[Bb, T, F] -> logits [Bb, C]: the eval forward on the current `P`, bit for bit what `self.model.eval()` gives after `sync_to_model()`."""
        self._check(bags)
        Bb, Tn, Fd = bags.shape
        return forward_infer(self._w, self.dims, bags.reshape(Bb * Tn, Fd), _offsets([Tn] * Bb, self.dev), Bb)

    @torch.no_grad()
    def predict_ragged(self, bags, coords=None) -> torch.Tensor:
        """A list of [T_i, F] bags in ONE library call -> logits [N, C], row i bit-identical to bag i's own call; grouping is the caller's."""
        bags = list(bags)
        if not bags:
            return torch.empty(0, self.dims[3], dtype=torch.float32, device=self.dev)
        for b in bags:
            self._check(b)
        return self.predict_infer_ragged(mil_core.pack_bags(bags, n_feats=self.dims[0]))

    @torch.no_grad()
    def predict_infer_ragged(self, rb) -> torch.Tensor:
        """Bags that are already packed (`ResidentCohort.ragged_group`: a view of the resident store) -> logits [n_bags, C] in ONE library call."""
        if rb.n_bags == 0:
            return torch.empty(0, self.dims[3], dtype=torch.float32, device=self.dev)
        self._check(rb.feats)
        return forward_infer(self._w, self.dims, rb.feats, rb.offsets.to(torch.int64), rb.n_bags)

    def max_shared_tiles(self) -> int:
        """No bag is too long to share a call (include/amdstamp.h: one row class at every length): `mil_core.group_bags`'s own limit."""
        return mil_core.MAX_SOLO_TILES

    def group_valid_bags(self, lengths, per_call: int) -> list[tuple[int, int]]:
        """The hook of `mil_train.fit(valid_bags_per_call=)`: consecutive validation bags -> [start, end) groups, at most `valid_max_rows_per_call` rows a call."""
        return group_bags(lengths, per_call, self.valid_max_rows_per_call)


__all__ = ["GatedAttentionMIL", "HipAbmilTrainer", "CHIEF_SIZES", "KEYS", "forward_infer", "forward_train", "backward", "heatmap_scores", "dropout_masks", "group_bags"]
