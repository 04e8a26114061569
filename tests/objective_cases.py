"""The case list of the objective tests (test_cpu_objective_oracle.py, test_gpu_objective.py): name -> (kind, logits fp32 [B, C], targets fp32 as
amds_objective_step takes them, class weights fp32 [C] or None), all CPU tensors, drawn from fixed seeds.

CE   (B, C) in CE_SHAPES x {soft, one-hot} x {no weights, weights with one 0}; N(0, 3^2) logits, and +-80 logits where only the max shift keeps softmax finite.
L1   B in L1_SIZES, a third of the rows with p == t exactly.
Cox  Efron and Breslow, B in COX_SIZES + the limit: every time pattern with ~60 % events, plus all-events, one-event-at-the-largest-time and no-event on
     tied integer times, and one case with scores x 30 (range about +-90), where the reference's unshifted fp32 exp overflows."""
from __future__ import annotations

import torch

from objective_oracle import CE, COX_BRESLOW, COX_EFRON, L1

CE_SHAPES = [(1, 2), (2, 3), (63, 2), (64, 2), (65, 5), (257, 33), (3, 1024)]
L1_SIZES = [1, 64, 65, 257]
COX_SIZES = [1, 2, 7, 64, 65, 300]
COX_LIMIT = 4096          # amds_objective_max_items(), asserted by the GPU test
NINE = ([1, 2, 3, 4, 5, 5, 6, 7, 7], [1, 1, 1, 1, 0, 0, 1, 0, 0])          # ties among censored items only, events unique


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def ce_case(B: int, C: int, soft: bool, weighted: bool, big: bool, seed: int):
    g = _gen(seed)
    if big:
        x = (torch.randint(0, 2, (B, C), generator=g).float() * 2 - 1) * 80 + torch.randn(B, C, generator=g)
    else:
        x = torch.randn(B, C, generator=g) * 3
    if soft:
        y = torch.softmax(torch.randn(B, C, generator=g), dim=1)
    else:
        y = torch.nn.functional.one_hot(torch.randint(0, C, (B,), generator=g), C).float()
    w = None
    if weighted:
        w = torch.rand(C, generator=g) + 0.5
        w[int(torch.randint(0, C, (1,), generator=g))] = 0.0
    return CE, x, y, w


def l1_case(B: int, seed: int):
    g = _gen(seed)
    p = torch.randn(B, 1, generator=g) * 2
    t = torch.randn(B, generator=g) * 2
    t[::3] = p[::3, 0]
    return L1, p, t, None


def cox_times(pattern: str, B: int, g: torch.Generator):
    """-> (time [B], event [B] or None when the pattern leaves the events to the event pattern)."""
    if pattern == "distinct":
        return (torch.randperm(B, generator=g).float() + 1) * 0.5, None
    if pattern == "ties":
        return torch.randint(1, max(B // 4, 2), (B,), generator=g).float(), None
    if pattern == "equal":
        return torch.full((B,), 3.0), None
    assert pattern == "censored_ties"          # events at unique times, censored items in tied pairs at times of their own
    t, e = torch.tensor(NINE[0]).float(), torch.tensor(NINE[1]).float()
    reps = -(-B // 9)
    t = torch.cat([t + 10 * r for r in range(reps)])[:B]
    e = e.repeat(reps)[:B]
    perm = torch.randperm(B, generator=g)
    return t[perm], e[perm]


def cox_events(pattern: str, time: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    B = time.numel()
    if pattern == "most":
        return (torch.rand(B, generator=g) < 0.6).float()
    if pattern == "all":
        return torch.ones(B)
    if pattern == "none":
        return torch.zeros(B)
    assert pattern == "last"
    e = torch.zeros(B)
    e[int(time.argmax())] = 1.0
    return e


def cox_case(kind: int, B: int, times: str, events: str, seed: int, score_scale: float = 1.0):
    g = _gen(seed)
    t, e = cox_times(times, B, g)
    if e is None:
        e = cox_events(events, t, g)
    s = torch.randn(B, 1, generator=g) * score_scale
    return kind, s, torch.stack([t, e], 1), None


def torch_loss(kind, logits, targets, weight, dtype=torch.float64):
    """`stamp_amd.losses` as the trainers call it, in `dtype` on the CPU -> (loss tensor, d loss / d logits or None where the loss has no gradient)."""
    from stamp_amd import losses
    x = logits.to(dtype).clone().requires_grad_(True)
    y = targets.to(dtype)
    if kind == CE:
        loss = losses.weighted_cross_entropy(x, y, None if weight is None else weight.to(dtype))
    elif kind == L1:
        loss = losses.l1_loss(x, y)
    elif kind == COX_EFRON:
        loss = losses.neg_partial_log_likelihood(x.squeeze(-1), y[:, 0], y[:, 1])          # (cox_survival_loss without its cast to fp32)
    else:
        loss = losses.cox_breslow_loss(x, y[:, 0], y[:, 1])
    g = torch.autograd.grad(loss, x, allow_unused=True)[0] if loss.requires_grad else None
    return loss.detach(), g


def cases(limit: int = COX_LIMIT) -> dict:
    out, seed = {}, 1000
    for B, C in CE_SHAPES:
        for soft in (True, False):
            for weighted in (False, True):
                for big in (False, True):
                    seed += 1
                    out[f"ce-{B}x{C}-{'soft' if soft else 'onehot'}-{'w' if weighted else 'now'}-{'pm80' if big else 'n3'}"] = ce_case(B, C, soft, weighted, big, seed)
    for B in L1_SIZES:
        seed += 1
        out[f"l1-{B}"] = l1_case(B, seed)
    for kind, kn in ((COX_EFRON, "efron"), (COX_BRESLOW, "breslow")):
        for B in COX_SIZES + [limit]:
            for times in ("distinct", "ties", "equal", "censored_ties"):
                seed += 1
                out[f"{kn}-{B}-{times}-most"] = cox_case(kind, B, times, "most", seed)
            for events in ("all", "last", "none"):
                seed += 1
                out[f"{kn}-{B}-ties-{events}"] = cox_case(kind, B, "ties", events, seed)
        seed += 1
        out[f"{kn}-300-ties-most-x30"] = cox_case(kind, 300, "ties", "most", seed, score_scale=30.0)
    return out
