"""numpy restatement of amds_bag_plan's permutation (stamp_amd/csrc/bag_batch.hip), integers only; shared by test_cpu_bag_plan.py and test_gpu_bag_plan.py.

    bits = max(2, ceil(log2 rows)), half = ceil(bits / 2), mask = 2^half - 1, domain = 2^(2 half)
    key  = drop_rowkey(seed, epoch, p)                      (common.h: two murmur finalisers of seed / stream / row)
    rk_r = fmix32(key ^ (r + 1) * 0x9E3779B1)               r = 0 .. ROUNDS - 1
    F(x): (L, R) = (x >> half, x & mask); ROUNDS times (L, R) = (R, L ^ (fmix32(R ^ rk_r) & mask)); x = L << half | R
    pi(j) = F applied to j until the value is < rows        (cycle walking; at most domain - rows + 1 applications)

Everything is vectorised over keys (leading axis) and positions (trailing axis); `rounds` is a parameter so that the tests can build few-round mutants."""
import numpy as np

ROUNDS = 12          # PLAN_ROUNDS of bag_batch.hip
_U32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & _U32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _U32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _U32
    h ^= h >> np.uint64(16)
    return h


def drop_rowkey(seed, stream, row):
    seed, stream, row = (np.asarray(v, dtype=np.uint64) for v in (seed, stream, row))
    a = fmix32((seed & _U32) ^ (row & _U32) ^ ((stream * np.uint64(0x9E3779B1)) & _U32))
    return fmix32((a + (seed >> np.uint64(32)) + (((row >> np.uint64(32)) * np.uint64(0x7FEB352D)) & _U32)) & _U32)


def geometry(rows: int):
    """-> (half, mask, domain) for a patient of `rows` rows (rows >= 1)."""
    bits = max(2, int(rows - 1).bit_length())
    half = (bits + 1) // 2
    return half, (1 << half) - 1, 1 << (2 * half)


def round_keys(seed, epoch, p, rounds: int = ROUNDS):
    """uint64 [..., rounds] for broadcastable seed / epoch / p."""
    key = drop_rowkey(seed, epoch, p)
    r = (np.arange(1, rounds + 1, dtype=np.uint64) * np.uint64(0x9E3779B1)) & _U32
    return fmix32(key[..., None] ^ r)


def feistel(x, rk, half: int):
    """One application of the network: x uint64 [K, n] (values < domain), rk uint64 [K, rounds]."""
    mask = np.uint64((1 << half) - 1)
    L, R = x >> np.uint64(half), x & mask
    for r in range(rk.shape[-1]):
        L, R = R, L ^ (fmix32(R ^ rk[..., r:r + 1]) & mask)
    return (L << np.uint64(half)) | R


def permute(rows: int, n: int, rk, return_steps: bool = False):
    """pi(0 .. n - 1) for every key: int64 [K, n], rk uint64 [K, rounds]; with return_steps also the largest number of applications any entry took.
    Raises if an entry needs more than the stated bound of domain - rows + 1 applications."""
    half, _, domain = geometry(rows)
    K = rk.shape[0]
    x = np.broadcast_to(np.arange(n, dtype=np.uint64), (K, n)).copy()
    todo = np.ones((K, n), dtype=bool)
    steps = 0
    while todo.any():
        if steps >= domain - rows + 1:
            raise AssertionError(f"cycle walk past its bound of {domain - rows + 1} applications (rows={rows})")
        kk, jj = np.nonzero(todo)
        y = feistel(x[kk, jj][:, None], rk[kk], half)[:, 0]
        x[kk, jj] = y
        todo[kk, jj] = y >= rows
        steps += 1
    out = x.astype(np.int64)
    return (out, steps) if return_steps else out


def bag_plan(offsets, patients, bag_size: int, seed: int, epoch: int, rounds: int = ROUNDS):
    """What amds_bag_plan writes: (idx int64 [n, bag_size], sizes int64 [n])."""
    offsets = np.asarray(offsets, dtype=np.int64)
    patients = np.asarray(patients, dtype=np.int64)
    idx = np.full((len(patients), bag_size), -1, dtype=np.int64)
    sizes = np.zeros(len(patients), dtype=np.int64)
    for b, p in enumerate(patients.tolist()):
        rows = int(offsets[p + 1] - offsets[p])
        m = min(rows, bag_size)
        sizes[b] = m
        if m:
            rk = round_keys(np.uint64(seed & (2 ** 64 - 1)), np.uint64(epoch), np.uint64(p), rounds)[None, :]
            idx[b, :m] = offsets[p] + permute(rows, m, rk)[0]
    return idx, sizes


def keyed_samples(rows: int, bag: int, n_keys: int, rounds: int = ROUNDS, key_seed: int = 0):
    """int64 [n_keys, bag]: the first `bag` entries of the permutation of `rows` under n_keys different (seed, epoch) pairs at patient 7 -- 64-bit seeds
    from numpy's generator, epochs 0 .. 15."""
    rng = np.random.default_rng(key_seed)
    seeds = rng.integers(0, 2 ** 63, n_keys, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n_keys, dtype=np.uint64)
    epochs = (np.arange(n_keys, dtype=np.uint64) % np.uint64(16))
    return permute(rows, bag, round_keys(seeds, epochs, np.uint64(7), rounds))


def torch_samples(rows: int, bag: int, n_keys: int):
    """The control: `torch.randperm(rows)[:bag]`, n_keys times from torch's global generator (seed it before)."""
    import torch
    return np.stack([torch.randperm(rows)[:bag].numpy() for _ in range(n_keys)])


def z_scores(samples, rows: int) -> dict:
    """Chi-square statistics of samples int64 [M, bag] (each row: the first `bag` entries of a permutation of range(rows)), each reduced to
    z = (chi2 - nu) / sqrt(2 nu):
      inclusion  per-row inclusion counts (skipped where bag == rows): variance M (b/r)(1 - b/r) per cell, the sum scaled by (r - 1) / r, nu = r - 1
      first      counts of the first entry, nu = r - 1
      pair       rows <= 100 and bag >= 2: ordered (first, second) pair counts over the r (r - 1) possible pairs, nu = r (r - 1) - 1"""
    M, b = samples.shape
    r = rows
    out = {}
    if b < r:
        cnt = np.bincount(samples.reshape(-1), minlength=r).astype(np.float64)
        q = b / r
        chi = ((cnt - M * q) ** 2).sum() / (M * q * (1 - q)) * (r - 1) / r
        out["inclusion"] = (chi - (r - 1)) / np.sqrt(2 * (r - 1))
    cnt = np.bincount(samples[:, 0], minlength=r).astype(np.float64)
    chi = ((cnt - M / r) ** 2).sum() / (M / r)
    out["first"] = (chi - (r - 1)) / np.sqrt(2 * (r - 1))
    if r <= 100 and b >= 2:
        cnt = np.bincount(samples[:, 0] * r + samples[:, 1], minlength=r * r).astype(np.float64).reshape(r, r)
        assert np.trace(cnt) == 0
        e = M / (r * (r - 1))
        off = ~np.eye(r, dtype=bool)
        chi = ((cnt[off] - e) ** 2).sum() / e
        nu = r * (r - 1) - 1
        out["pair"] = (chi - nu) / np.sqrt(2 * nu)
    return out
