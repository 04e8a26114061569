"""The attention family on inputs whose softmax is NOT diffuse, judged per tensor (tests/attn_cases.py; the bars are proved in test_cpu_attention_bars.py).

Every entry point runs on every builder -- gaussian, planted, ascending, descending, saturated, uniform -- at the smallest shapes that cross every structure
of the kernels (T in {1, 64, 65, 193, 321}, B = 2, H = 3: one key; a full tile; a tile + 1; 4 key tiles with one key in the last and a second query block; 6 tiles =
both LDS stage parities twice, 3 query blocks), plus one planted case at the training length (1, 1025, 2).  Against fp64 on the same rounded operands:
out, lse, dq, dk, dv (u, osm, d bias_scale, dkv where the form has them), each on its own: |got - ref| in L2 and in max-abs <= 4 x (forward) or 8 x (backward) the
error the rounding model has on that very case and tensor (plus the fp32 accumulation term, attn_cases' docstring).  The bar comes from the references alone.  Each
entry is called twice and must give equal bits.

One line per (entry, case, dtype, tensor) is printed: `sharp| entry case dtype tensor  rel-L2  model's rel-L2  kernel/model  err/bar (L2)  err/bar (max)`;
profiles/attention_sharp_errors.txt is that table from one run, condensed by tools/sharp_table.py."""
import functools

import pytest
import torch

import attn_cases as A
from stamp_amd import _lib, ops
from stamp_amd import train_ops as TO

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
P_DROP, SEED, SID = 0.25, 4242, 21


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


class Table:
    """Collects the verdicts of one test: prints every line, fails at the end with all misses."""

    def __init__(self):
        self.misses = []
        print()                     # the table's lines start at column 0 whatever pytest printed before

    def add(self, entry, case, dt, got, model, ref, names=None):
        for n, (rl2, rmx, rel, mrel) in A.judge(got, model, ref, names).items():
            ratio = rel / mrel if mrel > 0 and rel < float("inf") else float("nan")
            print(f"sharp| {entry:34s} {case:22s} {_name(dt)} {n:4s} {rel:10.3e} {mrel:10.3e} {ratio:8.2f} {rl2:8.3f} {rmx:8.3f}")
            if not (rl2 <= 1.0 and rmx <= 1.0):
                self.misses.append((entry, case, _name(dt), n, f"rel {rel:.3e} model {mrel:.3e} err/bar L2 {rl2:.2f} max {rmx:.2f}"))

    def same_bits(self, entry, case, a, b):
        for x, y in zip(a, b):
            if not torch.equal(x, y):
                self.misses.append((entry, case, "two calls differ"))

    def close(self):
        assert not self.misses, "\n".join(str(m) for m in self.misses)


@functools.lru_cache(maxsize=None)
def _case(name, B, T, H, dt, hd=64, dout_scale=1.0):
    """The rounded operands of one case on the GPU: (qkv, dout, q, k, v, g) -- packed 16-bit tensors and their fp64 per-head views."""
    dev = torch.device("cuda:0")
    qkv = A.make_qkv(name, B, T, H, dt, seed=1, hd=hd).to(dev)
    dout = A.make_dout(B, T, H, dt, seed=1, hd=hd, scale=dout_scale).to(dev)
    q, k, v = A.unpack_qkv(qkv, B, T, H, hd)
    return qkv, dout, q, k, v, A.heads(dout, B, T, H, hd)


@functools.lru_cache(maxsize=None)
def _plain_refs(name, B, T, H, dt):
    """(reference, rounding model) of the plain form without dropout, shared by the forward, the backward and the ragged test."""
    _, _, q, k, v, g = _case(name, B, T, H, dt)
    return A.reference(q, k, v, g), A.flash(q, k, v, g, dt=dt)


def _label(name, B, T, H):
    return f"{name}({B},{T},{H})"


def _grads(dqkv, B, T, H):
    dq, dk, dv = A.unpack_qkv(dqkv, B, T, H)
    return dict(dq=dq, dk=dk, dv=dv)


# ---- the plain streaming forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_attention_and_fwd_lse_and_bwd(gpu, dt):
    """amds_attention; amds_attention_fwd_lse / amds_attention_bwd."""
    lib, code, tab = _lib.lib(), ops.act_code(dt), Table()
    for name, B, T, H in A.stream_cases():
        qkv, dout, *_ = _case(name, B, T, H, dt)
        ref, model = _plain_refs(name, B, T, H, dt)
        lab = _label(name, B, T, H)
        outs = []
        for _ in range(2):
            out = torch.empty(B * T, H * 64, dtype=dt, device=gpu)
            _lib.check(lib.amds_attention(_p(qkv), _p(out), B, T, H, code, _st()), "attention")
            outs.append(out)
        tab.same_bits("amds_attention", lab, outs[:1], outs[1:])
        tab.add("amds_attention", lab, dt, dict(out=A.heads(outs[0], B, T, H)), model, ref, ["out"])
        out, lse = TO.attention_fwd_lse(qkv, B, T, H)
        out2, lse2 = TO.attention_fwd_lse(qkv, B, T, H)
        tab.same_bits("amds_attention_fwd_lse", lab, (out, lse), (out2, lse2))
        tab.add("amds_attention_fwd_lse", lab, dt, dict(out=A.heads(out, B, T, H), lse=lse.double()), model, ref, ["out", "lse"])
        dqkv = TO.attention_bwd(qkv, out, dout, lse, B, T, H)
        tab.same_bits("amds_attention_bwd", lab, [dqkv], [TO.attention_bwd(qkv, out, dout, lse, B, T, H)])
        tab.add("amds_attention_bwd", lab, dt, _grads(dqkv, B, T, H), model, ref, ["dq", "dk", "dv"])
    tab.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_train_with_dropout(gpu, dt):
    """amds_attention_fwd_train / _bwd_train at p = 0.25; the multiplier is the kernels' own mask (amds_attention_dropout_mask) x amds_dropout_keep_scale."""
    lib, tab = _lib.lib(), Table()
    for name, B, T, H in A.stream_cases():
        qkv, dout, q, k, v, g = _case(name, B, T, H, dt)
        mult = TO.attention_dropout_mask(B, H, T, P_DROP, SEED, SID, gpu).double() * lib.amds_dropout_keep_scale(P_DROP)
        ref, model = A.reference(q, k, v, g, mult=mult), A.flash(q, k, v, g, mult=mult, dt=dt)
        lab = _label(name, B, T, H)
        out, lse = TO.attention_fwd_train(qkv, B, T, H, P_DROP, SEED, SID)
        tab.same_bits("amds_attention_fwd_train", lab, (out, lse), TO.attention_fwd_train(qkv, B, T, H, P_DROP, SEED, SID))
        tab.add("amds_attention_fwd_train", lab, dt, dict(out=A.heads(out, B, T, H), lse=lse.double()), model, ref, ["out", "lse"])
        dqkv = TO.attention_bwd_train(qkv, out, dout, lse, B, T, H, P_DROP, SEED, SID)
        tab.same_bits("amds_attention_bwd_train", lab, [dqkv], [TO.attention_bwd_train(qkv, out, dout, lse, B, T, H, P_DROP, SEED, SID)])
        tab.add("amds_attention_bwd_train", lab, dt, _grads(dqkv, B, T, H), model, ref, ["dq", "dk", "dv"])
    tab.close()


# ---- the one-query forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_attention_row_forms(gpu, dt):
    """amds_attention_row; amds_attention_row_fwd_train / _row_bwd_train at p = 0 and 0.25 (query row 0: in `planted` it attends to the LAST key); the rows of dQ
    off the query row must be zero."""
    lib, code, tab = _lib.lib(), ops.act_code(dt), Table()
    for name, B, T, H in A.stream_cases():
        qkv, dout, q, k, v, g = _case(name, B, T, H, dt)
        D, lab = H * 64, _label(name, B, T, H)
        q1, g1 = q[:, :, :1], g[:, :, :1]
        for p in (0.0, P_DROP):
            mult = None
            if p > 0:
                mult = TO.attention_dropout_mask(B, H, T, p, SEED, SID, gpu)[:, :, :1].double() * lib.amds_dropout_keep_scale(p)
            ref, model = A.reference(q1, k, v, g1, mult=mult), A.flash(q1, k, v, g1, mult=mult, dt=dt, round_p=False)
            if p == 0:
                qrow = qkv.view(B, T, 3 * D)[:, 0, :D].contiguous()
                outs = []
                for _ in range(2):
                    o = torch.empty(B, D, dtype=dt, device=gpu)
                    _lib.check(lib.amds_attention_row(_p(qrow), D, _p(qkv), _p(o), D, B, T, H, code, _st()), "attention_row")
                    outs.append(o)
                tab.same_bits("amds_attention_row", lab, outs[:1], outs[1:])
                tab.add("amds_attention_row", lab, dt, dict(out=A.heads(outs[0], B, 1, H)), model, ref, ["out"])
            runs = []
            for _ in range(2):
                out, lse = torch.zeros(B * T, D, dtype=dt, device=gpu), torch.zeros(B, H, T, dtype=torch.float32, device=gpu)
                dqkv = torch.empty(B * T, 3 * D, dtype=dt, device=gpu)
                _lib.check(lib.amds_attention_row_fwd_train(_p(qkv), _p(out), _p(lse), B, T, H, 0, code, p, SEED, SID, _st()), "row_fwd_train")
                _lib.check(lib.amds_attention_row_bwd_train(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), B, T, H, 0, code, p, SEED, SID, _st()), "row_bwd_train")
                runs.append((out, lse, dqkv))
            tab.same_bits("amds_attention_row_fwd/bwd_train", lab, runs[0], runs[1])
            out, lse, dqkv = runs[0]
            gr = _grads(dqkv, B, T, H)
            if T > 1 and bool((gr["dq"][:, :, 1:] != 0).any()):
                tab.misses.append(("amds_attention_row_bwd_train", lab, "dQ off the query row is not zero"))
            got = dict(out=A.heads(out, B, T, H)[:, :, :1], lse=lse.double()[:, :, :1], dq=gr["dq"][:, :, :1], dk=gr["dk"], dv=gr["dv"])
            tab.add(f"amds_attention_row_fwd_train p={p}", lab, dt, got, model, ref, ["out", "lse"])
            tab.add(f"amds_attention_row_bwd_train p={p}", lab, dt, got, model, ref, ["dq", "dk", "dv"])
    tab.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_row_alibi_forms(gpu, dt):
    """amds_attention_row_alibi_fwd_train / _bwd_train, query row 0 (the class token at the origin): out, U, Osm, lse, dq, dk, dv and d bias_scale."""
    lib, code, tab = _lib.lib(), ops.act_code(dt), Table()
    for name, B, T, H in A.stream_cases():
        qkv, dout, q, k, v, g = _case(name, B, T, H, dt, dout_scale=0.5)
        D, lab = H * 64, _label(name, B, T, H)
        coords, (bs, rm) = A.make_coords(B, T, 1).to(gpu), tuple(t.to(gpu) for t in A.make_alibi_scales(H, 1))
        rform, mform = A.alibi_train_form(coords, bs, rm)
        rform["post"], mform["post"] = rform["post"][:, :, :1], mform["post"][:, :, :1]
        mform.update(out_dt="dt", round_p=False)
        q1, g1 = q[:, :, :1], g[:, :, :1]
        ref, model = A.reference(q1, k, v, g1, **rform), A.flash(q1, k, v, g1, dt=dt, **mform)
        inv_rm = (1.0 / rm).contiguous()
        runs = []
        for _ in range(2):
            out, u, osm = (torch.zeros(B * T, D, dtype=dt, device=gpu) for _ in range(3))
            lse, dqkv, dbs = torch.zeros(B, H, T, dtype=torch.float32, device=gpu), torch.empty(B * T, 3 * D, dtype=dt, device=gpu), torch.empty(B, H, dtype=torch.float32, device=gpu)
            _lib.check(lib.amds_attention_row_alibi_fwd_train(_p(qkv), _p(coords), _p(inv_rm), _p(bs), _p(out), _p(u), _p(osm), _p(lse), B, T, H, 0, code, _st()), "fwd")
            _lib.check(lib.amds_attention_row_alibi_bwd_train(_p(qkv), _p(osm), _p(u), _p(dout), _p(lse), _p(coords), _p(bs), _p(inv_rm), _p(dqkv), _p(dbs), B, T, H, 0, code,
                                                              _st()), "bwd")
            runs.append((out, u, osm, lse, dqkv, dbs))
        tab.same_bits("amds_attention_row_alibi", lab, runs[0], runs[1])
        out, u, osm, lse, dqkv, dbs = runs[0]
        gr = _grads(dqkv, B, T, H)
        if T > 1 and bool((gr["dq"][:, :, 1:] != 0).any()):
            tab.misses.append(("amds_attention_row_alibi_bwd_train", lab, "dQ off the query row is not zero"))
        got = dict(out=A.heads(out, B, T, H)[:, :, :1], u=A.heads(u, B, T, H)[:, :, :1], osm=A.heads(osm, B, T, H)[:, :, :1], lse=lse.double()[:, :, :1],
                   dq=gr["dq"][:, :, :1], dk=gr["dk"], dv=gr["dv"], dbs=dbs.double().sum(0))
        tab.add("amds_attention_row_alibi_fwd_train", lab, dt, got, model, ref, ["out", "u", "osm", "lse"])
        tab.add("amds_attention_row_alibi_bwd_train", lab, dt, got, model, ref, ["dq", "dk", "dv", "dbs"])
    tab.close()


# ---- ALiBi, masks, the distance bias ---------------------------------------------------------------------------------------------------------------------
def test_attention_alibi_train(gpu):
    """amds_attention_alibi_fwd_train / amds_attention_alibi_bwd (bf16 only): out, U, Osm, lse, dq, dk, dv, d bias_scale."""
    dt, tab = torch.bfloat16, Table()
    for name, B, T, H in A.stream_cases():
        qkv, dout, q, k, v, g = _case(name, B, T, H, dt, dout_scale=0.5)
        lab = _label(name, B, T, H)
        coords, (bs, rm) = A.make_coords(B, T, 1).to(gpu), tuple(t.to(gpu) for t in A.make_alibi_scales(H, 1))
        rform, mform = A.alibi_train_form(coords, bs, rm)
        ref, model = A.reference(q, k, v, g, **rform), A.flash(q, k, v, g, dt=dt, **mform)
        inv_rm, ds = (1.0 / rm).contiguous(), (bs / rm).contiguous()
        runs = []
        for _ in range(2):
            out, u, osm, lse = TO.attention_alibi_fwd_train(qkv, coords, inv_rm, bs, B, T, H)
            dqkv, dbs = TO.attention_alibi_bwd(qkv, osm, u, dout, lse, coords, bs, ds, B, T, H)
            runs.append((out, u, osm, lse, dqkv, dbs))
        tab.same_bits("amds_attention_alibi_fwd_train/_bwd", lab, runs[0], runs[1])
        out, u, osm, lse, dqkv, dbs = runs[0]
        got = dict(out=A.heads(out, B, T, H), u=A.heads(u, B, T, H), osm=A.heads(osm, B, T, H), lse=lse.double(), dbs=dbs.double().reshape(H), **_grads(dqkv, B, T, H))
        tab.add("amds_attention_alibi_fwd_train", lab, dt, got, model, ref, ["out", "u", "osm", "lse"])
        tab.add("amds_attention_alibi_bwd", lab, dt, got, model, ref, ["dq", "dk", "dv", "dbs"])
    tab.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_masked_and_alibi_inference(gpu, dt):
    """amds_attention_masked (the literal mask, mask_heads = H: the pad row of bag (b H + h) % B), amds_attention_alibi and amds_attention_alibi_masked (bf16 out)."""
    lib, code, tab = _lib.lib(), ops.act_code(dt), Table()
    for name, B, T, H in A.stream_cases():
        qkv, _, q, k, v, _ = _case(name, B, T, H, dt)
        D, lab = H * 64, _label(name, B, T, H)
        pad = A.make_pad(B, T, 1).to(gpu)
        coords, (bs, rm) = A.make_coords(B, T, 1).to(gpu), tuple(t.to(gpu) for t in A.make_alibi_scales(H, 1))
        hs = (bs / rm).contiguous()
        bl = dict(blocked=A.literal_mask(pad, B, T, H, mask_heads=H))
        forms = {"amds_attention_masked": (bl, bl, dt),
                 "amds_attention_alibi": A.alibi_infer_form(coords, hs) + (torch.bfloat16,),
                 "amds_attention_alibi_masked": A.alibi_infer_form(coords, hs, A.literal_mask(pad, B, T, H)) + (torch.bfloat16,)}
        for entry, (rform, mform, odt) in forms.items():
            ref, model = A.reference(q, k, v, **rform), A.flash(q, k, v, dt=dt, **mform)
            outs = []
            for _ in range(2):
                out = torch.empty(B * T, D, dtype=odt, device=gpu)
                if entry == "amds_attention_masked":
                    rc = lib.amds_attention_masked(_p(qkv), _p(pad), _p(out), B, T, H, H, code, _st())
                elif entry == "amds_attention_alibi":
                    rc = lib.amds_attention_alibi(_p(qkv), _p(coords), _p(hs), _p(out), B, T, H, code, _st())
                else:
                    rc = lib.amds_attention_alibi_masked(_p(qkv), _p(coords), _p(hs), _p(pad), _p(out), B, T, H, code, _st())
                _lib.check(rc, entry)
                outs.append(out)
            tab.same_bits(entry, lab, outs[:1], outs[1:])
            tab.add(entry, lab, dt, dict(out=A.heads(outs[0], B, T, H)), model, ref, ["out"])
    tab.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_distbias(gpu, dt):
    """amds_attention_distbias: TICON's bias inside the softmax, integer grid coordinates in [0, 40), slopes 1/2, 1/4, 1/8."""
    lib, code, tab = _lib.lib(), ops.act_code(dt), Table()
    for name, B, T, H in A.stream_cases():
        qkv, _, q, k, v, _ = _case(name, B, T, H, dt)
        lab = _label(name, B, T, H)
        coords = torch.randint(0, 40, (B, T, 2), generator=torch.Generator().manual_seed(T)).float().to(gpu)
        slopes = torch.tensor([0.5, 0.25, 0.125][:H], device=gpu)
        form = A.distbias_form(coords, slopes)
        ref, model = A.reference(q, k, v, **form), A.flash(q, k, v, dt=dt, **form)
        outs = []
        for _ in range(2):
            out = torch.empty(B * T, H * 64, dtype=dt, device=gpu)
            _lib.check(lib.amds_attention_distbias(_p(qkv), _p(coords), _p(slopes), _p(out), B, T, H, code, _st()), "distbias")
            outs.append(out)
        tab.same_bits("amds_attention_distbias", lab, outs[:1], outs[1:])
        tab.add("amds_attention_distbias", lab, dt, dict(out=A.heads(outs[0], B, T, H)), model, ref, ["out"])
    tab.close()


# ---- ragged bags ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_attention_varlen_forms(gpu, dt):
    """amds_attention_varlen, amds_attention_alibi_varlen, amds_attention_row_varlen (a class token in front of every bag) and amds_attention_varlen_rows (none):
    bags of 1, 64, 65, 193 and 321 token rows in ONE call per builder, every bag with its own planted map / boosted keys; each bag against fp64 on its own rows."""
    lib, code, tab, H = _lib.lib(), ops.act_code(dt), Table(), A.STREAM_BH[1]
    lens, D = list(A.STREAM_T), A.STREAM_BH[1] * 64
    n, M, mx = len(lens), sum(lens), max(lens)
    offs = torch.tensor([sum(t - 1 for t in lens[:i]) for i in range(n + 1)], dtype=torch.int32, device=gpu)          # tiles behind the class tokens
    offs_rows = torch.tensor([sum(lens[:i]) for i in range(n + 1)], dtype=torch.int32, device=gpu)                  # rows, no class token
    need, need_rows = lib.amds_attention_varlen_workspace_bytes(n, M - n), lib.amds_attention_varlen_workspace_bytes(n, M)
    coords = [A.make_coords(1, t, 1).to(gpu) for t in lens]
    cflat = torch.cat([c[0] for c in coords], 0).contiguous()
    hs = (lambda bs, rm: (bs / rm).to(gpu).contiguous())(*A.make_alibi_scales(H, 1))
    for name in A.BUILDERS:
        bags = [_case(name, 1, t, H, dt) for t in lens]
        qkv = torch.cat([b[0] for b in bags], 0).contiguous()
        qrows = torch.cat([b[0][:1, :D] for b in bags], 0).contiguous()
        runs = []
        for _ in range(2):
            ws = [torch.empty(max(need, need_rows, 16), dtype=torch.uint8, device=gpu) for _ in range(4)]
            o_plain, o_rows = torch.empty(M, D, dtype=dt, device=gpu), torch.empty(M, D, dtype=dt, device=gpu)
            o_alibi, o_row = torch.empty(M, D, dtype=torch.bfloat16, device=gpu), torch.empty(n, D, dtype=dt, device=gpu)
            _lib.check(lib.amds_attention_varlen(_p(qkv), _p(offs), _p(o_plain), n, M - n, mx - 1, H, code, _p(ws[0]), need, _st()), "attention_varlen")
            _lib.check(lib.amds_attention_alibi_varlen(_p(qkv), _p(cflat), _p(hs), _p(offs), _p(o_alibi), n, M - n, mx - 1, H, code, _p(ws[1]), need, _st()), "alibi_varlen")
            _lib.check(lib.amds_attention_row_varlen(_p(qrows), D, _p(qkv), _p(offs), _p(o_row), D, n, M - n, mx - 1, H, code, _p(ws[2]), need, _st()), "row_varlen")
            _lib.check(lib.amds_attention_varlen_rows(_p(qkv), _p(offs_rows), _p(o_rows), n, M, mx, H, code, _p(ws[3]), need_rows, _st()), "varlen_rows")
            runs.append((o_plain, o_alibi, o_row, o_rows))
        tab.same_bits("amds_attention_*varlen*", name, runs[0], runs[1])
        o_plain, o_alibi, o_row, o_rows = runs[0]
        r0 = 0
        for i, t in enumerate(lens):
            _, _, q, k, v, _ = bags[i]
            ref, model = _plain_refs(name, 1, t, H, dt)
            lab = f"{name} bag of {t}"
            tab.add("amds_attention_varlen", lab, dt, dict(out=A.heads(o_plain[r0:r0 + t], 1, t, H)), model, ref, ["out"])
            tab.add("amds_attention_varlen_rows", lab, dt, dict(out=A.heads(o_rows[r0:r0 + t], 1, t, H)), model, ref, ["out"])
            rform, mform = A.alibi_infer_form(coords[i], hs)
            tab.add("amds_attention_alibi_varlen", lab, dt, dict(out=A.heads(o_alibi[r0:r0 + t], 1, t, H)), A.flash(q, k, v, dt=dt, **mform), A.reference(q, k, v, **rform), ["out"])
            q1 = q[:, :, :1]
            tab.add("amds_attention_row_varlen", lab, dt, dict(out=A.heads(o_row[i:i + 1], 1, 1, H)), A.flash(q1, k, v, dt=dt, round_p=False), A.reference(q1, k, v), ["out"])
            r0 += t
    tab.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_cls_f32(gpu, dt):
    """amds_attention_cls_f32 (T <= 288): ONE fp32 query row per (bag, head) -- the builder's query 0 before any rounding -- against the 16-bit keys / values, fp32
    out; T = 1, 65, 257, 261 at head dim 64 and T = 257 at head dim 80."""
    lib, code, tab, B, H = _lib.lib(), ops.act_code(dt), Table(), 2, 2
    for name in A.BUILDERS:
        for T, hd in ((1, 64), (65, 64), (257, 64), (261, 64), (257, 80)):
            qkv, _, _, k, v, _ = _case(name, B, T, H, dt, hd)
            D, lab = H * hd, f"{name}({B},{T},{H}) hd={hd}"
            q32 = A.build(name, B, T, H, 1, hd=hd)[0][:, :, :1].to(gpu)                    # [B, H, 1, hd] fp32 (the draw behind the packed tensor's q)
            qrow = q32.permute(0, 2, 1, 3).reshape(B, D).contiguous()
            ref, model = A.reference(q32, k, v), A.flash(q32, k, v, dt=dt, round_p=False, out_dt=None)
            outs = []
            for _ in range(2):
                out = torch.empty(B, D, dtype=torch.float32, device=gpu)
                _lib.check(lib.amds_attention_cls_f32(_p(qrow), D, _p(qkv), _p(out), D, B, T, H, hd, code, _st()), "attention_cls_f32")
                outs.append(out)
            tab.same_bits("amds_attention_cls_f32", lab, outs[:1], outs[1:])
            tab.add("amds_attention_cls_f32", lab, dt, dict(out=A.heads(outs[0], B, 1, H, hd)), model, ref, ["out"])
    tab.close()


# ---- cross attention ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nt", [5, 32, 33])
def test_cross_attention(gpu, dt, nt):
    """amds_cross_attention_fwd_train / _bwd_train at p = 0.25: fp32 queries (query counts on both sides of 32) against 16-bit K | V of 65 and 321 keys; out, lse, dq
    in fp32, dkv in the 16-bit type.  fp32 arithmetic throughout (barspoon_train.hip:58, :158): the model rounds dkv at the store and nothing else."""
    lib, tab, B, H, hd = _lib.lib(), Table(), 2, 3, 64
    for name in A.BUILDERS:
        for T in (65, 321):
            qf, kf, vf = A.build(name, B, T, H, seed=2, Tq=nt)
            kv = torch.stack((kf, vf), 0).permute(1, 3, 0, 2, 4).reshape(B * T, 2 * H * 64).to(dt).to(gpu)
            qx = qf.permute(0, 2, 1, 3).reshape(B, nt, H * hd).contiguous().to(gpu)
            dox = torch.randn(B, nt, H * hd, generator=torch.Generator().manual_seed(nt + T)).to(gpu)
            k, v = kv.double().view(B, T, 2, H, 64).permute(2, 0, 3, 1, 4)
            q, g = qx.double().view(B, nt, H, hd).permute(0, 2, 1, 3), dox.double().view(B, nt, H, hd).permute(0, 2, 1, 3)
            mult = TO.attention_dropout_mask_rows(B * H * nt, T, P_DROP, SEED, 5003, gpu).view(B, H, nt, T).double() * lib.amds_dropout_keep_scale(P_DROP)
            ref = A.reference(q, k, v, g, mult=mult)
            model = A.flash(q, k, v, g, mult=mult, dt=dt, round_p=False, out_dt=None, dq_dt=None)
            lab = f"{name}({B},{T},{H}) nt={nt}"
            runs = []
            for _ in range(2):
                out, lse = TO.cross_attention_fwd_train(qx, kv, B, T, nt, H, hd, P_DROP, SEED, 5003)
                dq, dkv = TO.cross_attention_bwd_train(qx, kv, out, dox, lse, B, T, nt, H, hd, P_DROP, SEED, 5003)
                runs.append((out, lse, dq, dkv))
            tab.same_bits("amds_cross_attention", lab, runs[0], runs[1])
            out, lse, dq, dkv = runs[0]
            dk, dv = dkv.double().view(B, T, 2, H, 64).permute(2, 0, 3, 1, 4)
            got = dict(out=out.double().view(B, nt, H, hd).permute(0, 2, 1, 3), lse=lse.double(), dq=dq.double().view(B, nt, H, hd).permute(0, 2, 1, 3), dk=dk, dv=dv)
            tab.add("amds_cross_attention_fwd_train", lab, dt, got, model, ref, ["out", "lse"])
            tab.add("amds_cross_attention_bwd_train", lab, dt, got, model, ref, ["dq", "dk", "dv"])
    tab.close()


# ---- the tile encoder's kernels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,hd", [(257, 64), (261, 64), (257, 80)])
def test_attention_vit(gpu, dt, T, hd):
    """amds_attention_vit at T = 257 and 261 (the T = 257 kernel and the 256 + R pipeline) and head dim 80 through amds_attention_vit_hd; forward only."""
    lib, code, tab, B, H = _lib.lib(), ops.act_code(dt), Table(), 2, 2
    for name in A.BUILDERS:
        qkv, _, q, k, v, _ = _case(name, B, T, H, dt, hd)
        ref, model = A.reference(q, k, v), A.flash(q, k, v, dt=dt)
        outs = []
        for _ in range(2):
            out = torch.empty(B * T, H * hd, dtype=dt, device=gpu)
            if hd == 64:
                rc = lib.amds_attention_vit(_p(qkv), _p(out), B, T, H, code, _st())
            else:
                rc = lib.amds_attention_vit_hd(_p(qkv), _p(out), B, T, H, hd, code, _st())
            _lib.check(rc, "attention_vit")
            outs.append(out)
        entry = "amds_attention_vit" if hd == 64 else "amds_attention_vit_hd(80)"
        tab.same_bits(entry, name, outs[:1], outs[1:])
        tab.add(entry, f"{name}({B},{T},{H})", dt, dict(out=A.heads(outs[0], B, T, H, hd)), model, ref, ["out"])
    tab.close()
