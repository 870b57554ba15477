"""A-ViT past 208 tokens on the MI355X: the chunked halting step and its backward (include/peekvit_hip_avit_long.h) bit for bit
against the resident pair up to 256 tokens and against the fp64 restatement of tests/avit_packed_train_ref.py above, guarded buffers, the eval
forward against the reference fixtures of scripts/make_golden_avit_long.py, and one long fused and one long packed training step against the fp64
composite replaying their halting decisions."""
import json
import os

import numpy as np
import pytest
import torch

import avit_packed_train_ref as pref
import avit_train_ref as ref
import test_hip_avit_train as dense_t
from conftest import GOLDEN, rel_l2
from peekvit_amd import synth

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "avit_long_meta.json")))
THR, U, GS, GC = dense_t.THR, dense_t.U, dense_t.GS, dense_t.GC
_dev = dense_t._dev
_h_err = dense_t._h_err
SAFE = 1e-3          # every token's c' is at least this far from the threshold in fp64, so fp32 and fp64 decide alike


# ---- inputs of one packed step -----------------------------------------------------------------------------------------------------------------------
def _channel0(c, below, last, g, keep_below=0.98):
    """fp32 channel 0 of the block output for running tokens whose halting sums are c (fp64, each in [0.05, 0.9)): the gate argument that puts
    c' = c + h at a target inside [c + 0.05, keep_below] (`below`: the token goes on) or [1.0, c + 0.95] (it halts).  With `last` h does not enter c'."""
    u = torch.rand(c.shape, generator=g).double()
    target = torch.where(below, (c + 0.05) + u * (keep_below - (c + 0.05)), 1.0 + u * (c - 0.05).clamp(min=0))
    h = torch.rand(c.shape, generator=g).double() * 0.9 + 0.05 if last else target - c
    assert bool(((h > 0.01) & (h < 0.99)).all())
    return ((torch.log(h / (1 - h)) + GC) / GS).float()


def _inputs(B, S, D, n_cls, last, kinds, seed, keep_below=0.98):
    """fp32 inputs of one packed step on the CPU: (y [R, D], seg, nh, pos, (c, R, rho, counter, m), acc).  kinds[b] describes image b:
    "norep" every token still runs and about 3 in 4 go on - among them, always, the two on either side of every multiple of 256, so the survivors
    straddle every chunk boundary of the token walk and of the row walk; "mixed" running tokens and a representative row; "onlyrep" the segment is
    the representative row alone; "keepall" every running token goes on (with a representative row before); "haltall" every running token halts.
    Asserts in fp64, for EVERY token, that c' (c of a token without a row) is at least SAFE from the threshold."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, S)
    for b, k in enumerate(kinds):
        if k == "norep":
            m[b] = 1
        elif k in ("mixed", "keepall", "haltall"):
            m[b] = (torch.rand(S, generator=g) < 0.7).float()
            m[b, :n_cls], m[b, S - 1] = 1, 0          # the class tokens run, at least one token is halted
    below = torch.rand(B, S, generator=g) < 0.75
    for b, k in enumerate(kinds):
        if k == "haltall":
            below[b] = False
        elif k == "keepall":
            below[b] = True
        elif k == "norep":
            edge = torch.tensor(list(range(256, S, 256)), dtype=torch.long)
            below[b, edge], below[b, edge - 1] = True, True
            below[b, 1] = False                        # ... and at least one token halts
    c_run = 0.05 + torch.rand(B, S, generator=g).double() * 0.35
    y0 = _channel0(c_run, below, last, g, keep_below)
    c = torch.where(m == 1, c_run.float(), torch.full((B, S), 1.5))
    yd = torch.randn(B, S, D, generator=g)
    yd[:, :, 0] = torch.where(m == 1, y0, (torch.rand(B, S, generator=g) * 8 - 4 + GC) / GS)
    h = torch.sigmoid(yd[:, :, 0].double() * GS - GC)
    c1 = torch.where(m == 1, c.double() + (torch.ones_like(h) if last else h), c.double())
    assert bool(((c1 - THR).abs() >= SAFE).all()), "a token within 1e-3 of the threshold"
    if not last:
        assert bool(((c1 < THR) == below)[m == 1].all())
    R, rho = torch.rand(B, S, generator=g), torch.rand(B, S, generator=g) * 3
    counter = torch.randint(1, 6, (B, S), generator=g).float()
    acc = torch.randn(B, n_cls, D, generator=g)
    live = m == 1
    rows, pos, seg, nh = [], [], [0], []
    for b in range(B):
        idx = live[b].nonzero()[:, 0]
        rows.append(yd[b, idx])
        pos += idx.tolist()
        if len(idx) < S:
            rows.append(yd[b, (~live[b]).nonzero()[0, 0]][None])
            pos.append(-1)
        nh.append(S - len(idx))
        seg.append(len(pos))
    return torch.cat(rows), torch.tensor(seg, dtype=torch.int32), torch.tensor(nh, dtype=torch.int32), torch.tensor(pos, dtype=torch.int32), \
        (c, R, rho, counter, m), acc


def _run_fwd(step, y, seg, nh, pos, state, acc, last, dev, **kw):
    out = step(y.to(dev), seg.to(dev), nh.to(dev), pos.to(dev), *(t.to(dev) for t in state), acc.to(dev), GS, GC, THR, bool(last), **kw)
    torch.cuda.synchronize()
    return out


NAMES = ["c", "R", "rho", "counter", "m", "acc", "h_part", "sv", "ycls", "x_next", "rs_next", "seg_next", "nh_next", "lm_next", "pos_next", "totals", "src_next"]


def _flat(out):
    """{name: CPU tensor} of everything a step wrote (the row arrays cut to the rows written); a save that was not asked for is absent."""
    st, acc1, h_part, sv, ycls, nxt = out
    d = dict(zip(NAMES[:9], [*st, acc1, h_part, sv, ycls]))
    if nxt is not None:
        r = int(nxt[6][0])
        d.update(x_next=nxt[0][:r], rs_next=nxt[1][:r], seg_next=nxt[2], nh_next=nxt[3], lm_next=nxt[4][:r], pos_next=nxt[5][:r], totals=nxt[6],
                 src_next=None if nxt[7] is None else nxt[7][:r])
    return {k: v.cpu() for k, v in d.items() if v is not None}


def _same_bits(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


KINDS5 = ["norep", "mixed", "onlyrep", "haltall", "keepall"]


# ---- forward, S <= 256: the resident step's bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [17, 197, 208, 256])
def test_long_step_has_the_resident_steps_bits_up_to_256_tokens(S, D, last):
    """pv_avit_pack_step_long against pv_avit_pack_step_train on the same inputs, B = 5 (no halted token / mixed / a one-row segment / every token
    halts / every token goes on), one or two class tokens: every output bit for bit - h_part too, whose order at one chunk is the resident one
    (include/peekvit_hip_avit_long.h) - and the inference step (no saves) writes the same bits into everything else."""
    from peekvit_amd import ops
    dev = _dev()
    n_cls = 1 + (S + D + last) % 2
    inp = _inputs(5, S, D, n_cls, last, KINDS5, seed=S * 10 + D + last)
    a = _flat(_run_fwd(ops.avit_pack_step_train, *inp, last, dev))
    b = _flat(_run_fwd(ops.avit_pack_step_long, *inp, last, dev))
    _same_bits(a, b, "long vs resident")
    nosave = _flat(_run_fwd(ops.avit_pack_step_long, *inp, last, dev, save=False))
    assert not {"sv", "ycls", "src_next"} & set(nosave)
    _same_bits({k: v for k, v in b.items() if k not in ("sv", "ycls", "src_next")}, nosave, "inference step")
    if not last:
        seg_n = a["seg_next"]
        assert int(seg_n[3] - seg_n[2]) == 1 and int(seg_n[4] - seg_n[3]) == 1          # onlyrep, haltall: one-row segments
        assert int(a["nh_next"][0]) > 0 and int(seg_n[1] - seg_n[0]) > 1


# ---- forward, S > 256: the torch restatement ----------------------------------------------------------------------------------------------------------
def _check_forward(inp, out, st64, last, S):
    """tests/test_hip_avit_packed_train.py's checks of the resident step's outputs, on a flat dict: integers, flags, copied rows exact; the float
    state and acc within bounds made of the kernel's own operations; h_part within S * 2^-24 relative of the fp64 sum (the worst case of ANY fp32
    summation order of non-negative terms - the terms' own errors, a few 2^-24 each, disappear in it)."""
    y, seg, nh, pos, state, acc = inp
    c, R, rho, counter, m = state
    B, n_cls, D = acc.shape
    c64, R64, rho64, cnt64, m64 = st64["state"]
    assert torch.equal(out["counter"].double(), cnt64) and torch.equal(out["m"].double(), m64)
    assert torch.equal(out["sv"][2].double(), st64["sv"][2]), "flags"
    gone = m == 0
    for got, src in ((out["c"], c), (out["R"], R), (out["rho"], rho), (out["counter"], counter)):
        assert torch.equal(got[gone], src[gone])
    live = pos >= 0
    img = pref._row_image(seg.long(), y.shape[0])
    lb, lp = img[live], pos[live].long()
    h64, w64 = st64["sv"][0], st64["sv"][1]
    h_err = _h_err(y[:, 0].double(), h64)
    assert ((out["sv"][0].double() - h64).abs() <= h_err).all()
    hh_err = torch.zeros_like(h_err) if last else h_err
    assert ((out["c"][lb, lp].double() - c64[lb, lp]).abs() <= hh_err[live] + 2 * U * c64[lb, lp].abs()).all()
    assert ((out["R"][lb, lp].double() - R64[lb, lp]).abs() <= hh_err[live] + 2 * U * (R[lb, lp].double().abs() + 1)).all()
    assert ((out["rho"].double() - rho64).abs() <= 4 * U * rho64.abs()).all()
    w_err = hh_err + 4 * U * w64.abs()
    assert ((out["sv"][1].double() - w64).abs() <= w_err).all() and torch.equal(out["sv"][1][~live], torch.zeros(int((~live).sum())))
    w_cls, werr_cls, y_cls = torch.zeros(B, n_cls, dtype=torch.float64), torch.zeros(B, n_cls, dtype=torch.float64), torch.zeros(B, n_cls, D)
    is_cls = live & (pos < n_cls)
    w_cls[img[is_cls], pos[is_cls].long()], werr_cls[img[is_cls], pos[is_cls].long()] = w64[is_cls], w_err[is_cls]
    y_cls[img[is_cls], pos[is_cls].long()] = y[is_cls]
    assert torch.equal(out["ycls"], y_cls)
    acc_tol = y_cls.double().abs() * werr_cls[:, :, None] + 3 * U * (acc.double().abs() + (y_cls.double() * w_cls[:, :, None]).abs())
    assert ((out["acc"].double() - st64["acc"]).abs() <= acc_tol + 1e-30).all()
    no_cls_row = torch.ones(B, n_cls, dtype=torch.bool)
    no_cls_row[img[is_cls], pos[is_cls].long()] = False
    assert torch.equal(out["acc"][no_cls_row], acc[no_cls_row])
    hp, hp64 = out["h_part"].double(), st64["h_part"]
    print("h_part relative error", ((hp - hp64).abs() / hp64).tolist(), "bound", S * U)
    assert ((hp - hp64).abs() <= S * U * hp64).all()
    if last:
        assert "x_next" not in out
        return
    r_next, longest = out["totals"].tolist()
    assert (r_next, longest) == st64["totals"]
    assert torch.equal(out["seg_next"].long(), st64["seg_next"]) and torch.equal(out["nh_next"].long(), st64["nh_next"])
    assert torch.equal(out["pos_next"].long(), st64["pos_next"]) and torch.equal(out["src_next"].long(), st64["src_next"])
    assert torch.equal(out["rs_next"].double(), st64["rs_next"])
    # x_next: bit-copies of the source rows, the zero row where the table says so
    src = st64["src_next"]
    base = seg.long()[pref._row_image(st64["seg_next"], r_next)]
    want = torch.where((src >= 0)[:, None], y[(base + src.clamp(min=0))], torch.zeros(1, D))
    assert torch.equal(out["x_next"].view(torch.int32), want.view(torch.int32)), "copied rows / zero rows"
    rep = st64["pos_next"] < 0
    n = st64["nh_next"][pref._row_image(st64["seg_next"], r_next)][rep]
    assert torch.equal(out["lm_next"][~rep], torch.zeros(int((~rep).sum())))
    lm64 = torch.log(n.double())                                                        # logf(n) on the representative row: 2 ulp on top of n's rounding,
    assert ((out["lm_next"][rep].double() - lm64).abs() <= 4 * U * lm64).all()          # tests/test_hip_avit_packed_train.py's allowance


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("S", [257, 258, 513, 4096])
def test_long_step_against_the_torch_restatement_past_256_tokens(S, last):
    """B = 3, D = 64, two class tokens: image 0 has every token running and its survivors straddle every chunk boundary, image 1 keeps all its
    rows (with a representative row before), image 2 halts all of them.  Two runs bit-identical; the inference step writes the same bits."""
    from peekvit_amd import ops
    dev = _dev()
    kinds = ["norep", "keepall", "haltall"]
    inp = _inputs(3, S, 64, 2, last, kinds, seed=S + last)
    y, seg, nh, pos, state, acc = inp
    st64 = pref.pack_step_fwd(y.double(), seg, nh, pos, tuple(t.double() for t in state), acc.double(), GS, GC, THR, bool(last))
    out = _flat(_run_fwd(ops.avit_pack_step_long, *inp, last, dev))
    _same_bits(out, _flat(_run_fwd(ops.avit_pack_step_long, *inp, last, dev)), "two runs")
    nosave = _flat(_run_fwd(ops.avit_pack_step_long, *inp, last, dev, save=False))
    _same_bits({k: v for k, v in out.items() if k not in ("sv", "ycls", "src_next")}, nosave, "inference step")
    _check_forward(inp, out, st64, last, S)
    if last:
        return
    # the cases the images were chosen for
    seg_n, src = st64["seg_next"], st64["src_next"]
    mine = src[int(seg_n[0]):int(seg_n[1])]
    for edge in range(256, S, 256):
        assert edge - 1 in mine and edge in mine, edge                              # survivors on both sides of every chunk boundary
    assert int(seg[1] - seg[0]) == S and int(st64["nh_next"][0]) > 0 and int(mine[-1]) == -1          # S rows in, the survivors and one zero row out
    assert int(seg_n[2] - seg_n[1]) == int(seg[2] - seg[1]) and int(st64["nh_next"][1]) == int(nh[1])          # keeps all its rows
    assert int(seg_n[3] - seg_n[2]) == 1 and int(st64["nh_next"][2]) == S                                       # halts all its rows


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------------
def _bwd_args(B, S, D, n_cls, r_next, last, seed):
    g = torch.Generator().manual_seed(seed)
    g_next = None if last else torch.randn(r_next, D, generator=g)
    return g_next, torch.randn(B, S, generator=g), torch.randn(B, S, generator=g), torch.randn(B, n_cls, D, generator=g), \
        torch.randn(1, generator=g) * 50, torch.randn(B, generator=g)


def _run_bwd(bwd, fw, tables, args, D, last, dev, with_gh=True):
    """(dy, dy16, dR, G') of one backward on the forward `fw`'s own saved tables."""
    seg, nh, pos = tables
    _, _, _, sv, ycls, nxt = fw
    g_next, gR, grho, gacc, gh, G = args
    Gd = G.to(dev).clone()
    dy, dy16, dR = bwd(None if last else g_next.to(dev), seg.to(dev), nh.to(dev), pos.to(dev), None if last else nxt[2], None if last else nxt[7], sv,
                       ycls, gR.to(dev), grho.to(dev), gacc.to(dev), gh.to(dev) if with_gh else None, Gd, D, GS, bool(last))
    torch.cuda.synchronize()
    return {"dy": dy.cpu(), "dy16": dy16.cpu().view(torch.int16), "dR": dR.cpu(), "G": Gd.cpu()}


@pytest.mark.parametrize("with_gh", [True, False])
@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("S,D", [(17, 64), (197, 128), (256, 64)])
def test_long_backward_has_the_resident_backwards_bits_up_to_256_tokens(S, D, last, with_gh):
    """pv_avit_pack_step_long_bwd against pv_avit_pack_step_bwd on the resident forward's tables: dy, its 16-bit copy, dR and G bit for bit, in
    both operand builds, with merged rows, surviving rows and representative rows among the five images."""
    from peekvit_amd import engine, ops
    dev = _dev()
    n_cls = 1 + (S + last) % 2
    inp = _inputs(5, S, D, n_cls, last, KINDS5, seed=S * 7 + D + last)
    y, seg, nh, pos, state, acc = inp
    fw = _run_fwd(ops.avit_pack_step_train, *inp, last, dev)
    fl = fw[3][2].cpu().long()
    assert last or (((fl & pref.MERGED) != 0).any() and ((fl & pref.NOT_REACHED) != 0).any())
    assert ((fl & pref.REP) != 0).any()
    args = _bwd_args(5, S, D, n_cls, 0 if last else int(fw[5][6][0]), last, seed=S + D)
    for mode in ("bf16", "f16"):
        with engine.precision(mode):
            a = _run_bwd(ops.avit_pack_step_bwd, fw, (seg, nh, pos), args, D, last, dev, with_gh)
            b = _run_bwd(ops.avit_pack_step_long_bwd, fw, (seg, nh, pos), args, D, last, dev, with_gh)
        for k in a:          # (dy16 is held as int16 already; the fp32 arrays are compared as words, so a NaN or a -0 cannot hide)
            assert torch.equal(a[k] if k == "dy16" else a[k].view(torch.int32), b[k] if k == "dy16" else b[k].view(torch.int32)), (mode, k)


def _check_backward(inp, st64, args, got, last):
    """tests/test_hip_avit_packed_train.py's tolerances for the resident backward, against the fp64 restatement."""
    y, seg, nh, pos, state, acc = inp
    c, R, rho, counter, m = state
    g_next, gR, grho, gacc, gh, G = args
    B, n_cls, D = gacc.shape
    S = c.shape[1]
    dy64, dR64, G64 = pref.pack_step_bwd(st64, None if last else g_next.double(), gR.double(), grho.double(), gacc.double(),
                                         gh.double()[0] if B > 1 else None, G.double())
    dy, dR, G1 = got["dy"], got["dR"], got["G"]
    live = pos >= 0
    img = pref._row_image(seg.long(), y.shape[0])
    fl = st64["sv"][2].long()
    merged = (fl & pref.MERGED) != 0
    h64, w64 = st64["sv"][0], st64["sv"][1]
    h_err = _h_err(y[:, 0].double(), h64)
    gate = GS * h64 * (1 - h64)
    gate_err = GS * ((1 - 2 * h64).abs() * h_err + 3 * U * h64 * (1 - h64))
    coef = torch.zeros(B, dtype=torch.float64)
    coef[1:] = gh.double().abs() / ((B - 1) * S)
    plain = torch.ones(y.shape[0], D, dtype=torch.bool)
    plain[:, 0] = False
    plain[live & (pos < n_cls)] = False
    if not last:
        src = st64["src_next"]
        base = seg.long()[pref._row_image(st64["seg_next"], len(src))]
        kept = src >= 0
        rows = (base + src)[kept]
        assert torch.equal(torch.where(plain[rows], dy[rows], torch.zeros(())), torch.where(plain[rows], g_next[kept], torch.zeros(())))
        assert merged.sum() > 0 and (dy[merged][plain[merged]] == 0).all()
    else:
        assert (dy[plain] == 0).all()
    assert (dy[~live][:, 1:] == 0).all()
    rep_b = img[~live]
    G_tol = torch.zeros(B, dtype=torch.float64)
    G_tol[rep_b] = gate_err[~live] * coef[rep_b] + 4 * U * (G.double().abs()[rep_b] + coef[rep_b] * gate[~live])
    assert ((G1.double() - G64).abs() <= G_tol).all() and torch.equal(G1[G_tol == 0], G[G_tol == 0])
    n = nh.double()[rep_b]
    assert ((dy[~live][:, 0].double() - dy64[~live][:, 0]).abs() <= n * G_tol[rep_b] + 2 * U * dy64[~live][:, 0].abs()).all()
    lb, lp = img[live], pos[live].long()
    is_cls = pos[live] < n_cls
    yc, ga = torch.zeros(int(live.sum()), D, dtype=torch.float64), torch.zeros(int(live.sum()), D, dtype=torch.float64)
    yc[is_cls], ga[is_cls] = y[live][is_cls].double(), gacc.double()[lb[is_cls], lp[is_cls]]
    dot_abs = (ga * yc).abs().sum(-1)
    dot_err = D * U * dot_abs
    nr = ((fl[live] & pref.NOT_REACHED) != 0).double()
    reached = ((fl[live] & pref.REACHED) != 0).double()
    live_nr = 0.0 if last else nr
    gRl, grhol = gR.double()[lb, lp], grho.double()[lb, lp]
    assert ((dR[lb, lp].double() - dR64[lb, lp]).abs() <= reached * dot_err + 4 * U * (gRl.abs() + grhol.abs() + dot_abs)).all()
    assert torch.equal(dR[m == 0], gR[m == 0])
    dh_abs = coef[lb] + live_nr * (gRl.abs() + dot_abs)
    tol_d0 = gate_err[live] * dh_abs + gate[live] * (live_nr * dot_err + 4 * U * dh_abs)
    hh_err = torch.zeros_like(h_err) if last else h_err
    w_err = (nr * hh_err[live]) + 4 * U * w64[live].abs()
    tol = 2 * U * dy64[live].abs() + 1e-30 + ga.abs() * w_err[:, None] + 2 * U * ga.abs() * w64[live].abs()[:, None]
    passed = torch.zeros(int(live.sum()), dtype=torch.float64) if last else merged[live].double() * G.double().abs()[lb]
    tol[:, 0] += tol_d0 + 2 * U * (passed + dh_abs * gate[live])
    assert ((dy[live].double() - dy64[live]).abs() <= tol).all(), float(((dy[live].double() - dy64[live]).abs() - tol).max())
    return G64


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("S", [257, 513, 4096])
def test_long_backward_against_fp64_past_256_tokens(S, last):
    """pv_avit_pack_step_long_bwd on the long forward's own saved tables against the fp64 restatement, the resident backward's tolerances; the
    16-bit copy is the rounded dy; two runs bit-identical."""
    from peekvit_amd import _lib, ops
    dev = _dev()
    inp = _inputs(3, S, 64, 2, last, ["norep", "mixed", "haltall"], seed=3 * S + last)
    y, seg, nh, pos, state, acc = inp
    st64 = pref.pack_step_fwd(y.double(), seg, nh, pos, tuple(t.double() for t in state), acc.double(), GS, GC, THR, bool(last))
    fw = _run_fwd(ops.avit_pack_step_long, *inp, last, dev)
    args = _bwd_args(3, S, 64, 2, 0 if last else st64["totals"][0], last, seed=S)
    got = _run_bwd(ops.avit_pack_step_long_bwd, fw, (seg, nh, pos), args, 64, last, dev)
    again = _run_bwd(ops.avit_pack_step_long_bwd, fw, (seg, nh, pos), args, 64, last, dev)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"
    assert torch.equal(got["dy16"], got["dy"].to(_lib.operand_dtype()).view(torch.int16)), "dy16 is not the rounded dy"
    _check_backward(inp, st64, args, got, last)


def test_G_chained_over_three_layers_past_256_tokens():
    """Three halting steps at S = 257 chained forward through the kernel's own tables (the last with `last`), then their backwards from the last
    to the first with ONE G buffer updated in place: every layer's dy, dR and G against the fp64 restatement walking the same chain."""
    from peekvit_amd import ops
    dev = _dev()
    B, S, D, n_cls = 3, 257, 64, 2
    g = torch.Generator().manual_seed(11)
    inp = _inputs(B, S, D, n_cls, 0, ["norep", "mixed", "keepall"], seed=5, keep_below=0.5)
    layers = []
    for i in range(3):
        last = i == 2
        y, seg, nh, pos, state, acc = inp
        st64 = pref.pack_step_fwd(y.double(), seg, nh, pos, tuple(t.double() for t in state), acc.double(), GS, GC, THR, last)
        fw = _run_fwd(ops.avit_pack_step_long, *inp, last, dev)
        layers.append((inp, st64, fw, last))
        if last:
            break
        out = _flat(fw)
        assert torch.equal(out["seg_next"].long(), st64["seg_next"]) and torch.equal(out["pos_next"].long(), st64["pos_next"])
        # the next layer's block output: fresh rows, channel 0 placed from the kernel's own fp32 state
        seg2, nh2, pos2 = out["seg_next"], out["nh_next"], out["pos_next"]
        st2 = tuple(out[k] for k in ("c", "R", "rho", "counter", "m"))
        r2 = int(out["totals"][0])
        y2 = torch.randn(r2, D, generator=g)
        img = pref._row_image(seg2.long(), r2)
        live = pos2 >= 0
        c_run = st2[0][img[live], pos2[live].long()].double()
        assert i == 1 or bool((c_run <= 0.5 + 1e-6).all())          # (layer 0's survivors stopped at keep_below; the last layer's h does not enter c')
        below = torch.rand(int(live.sum()), generator=g) < 0.7
        y2[live, 0] = _channel0(c_run, below, i + 1 == 2, g)
        y2[~live, 0] = (torch.rand(int((~live).sum()), generator=g) * 8 - 4 + GC) / GS
        h = torch.sigmoid(y2[live, 0].double() * GS - GC)
        assert bool((((c_run + (1.0 if i + 1 == 2 else h)) - THR).abs() >= SAFE).all())
        inp = (y2, seg2, nh2, pos2, st2, out["acc"])
    G = torch.zeros(B)
    G64 = torch.zeros(B, dtype=torch.float64)
    g_next = None
    for i in (2, 1, 0):
        inp, st64, fw, last = layers[i]
        r_next = 0 if last else st64["totals"][0]
        args = list(_bwd_args(B, S, D, n_cls, r_next, last, seed=20 + i))
        args[5] = G
        got = _run_bwd(ops.avit_pack_step_long_bwd, fw, inp[1:4], tuple(args), D, last, dev)
        G64_new = _check_backward(inp, st64, tuple(args), got, last)
        G = got["G"]
        assert ((G.double() - G64_new).abs() <= 1e-5 * (G64_new.abs() + 1e-3)).all()
    assert bool((G[1:] != 0).all()), "no score term reached G"


# ---- guarded buffers ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [257, 4096])
def test_both_kernels_stay_inside_buffers_sized_as_the_header_states(S):
    """Every row array sized exactly R (R' for g_next) rows and followed by sentinel rows, the tables by sentinel words: after the step and its
    backward through ctypes every sentinel is untouched."""
    import ctypes as C
    from peekvit_amd import _lib
    dev = _dev()
    B, D, n_cls, PAD, SENT = 3, 64, 2, 64, 1232.0          # (a value bf16 and fp16 hold exactly)
    inp = _inputs(B, S, D, n_cls, 0, ["norep", "mixed", "haltall"], seed=S)
    y, seg, nh, pos, state, acc = inp
    st64 = pref.pack_step_fwd(y.double(), seg, nh, pos, tuple(t.double() for t in state), acc.double(), GS, GC, THR, False)
    R, Rn = y.shape[0], st64["totals"][0]

    def guarded(n, dtype=torch.float32):
        t = torch.full((n + PAD,), SENT if dtype.is_floating_point else 77, dtype=dtype, device=dev)
        return t

    f32, i32 = torch.float32, torch.int32
    bufs = {"out": guarded(5 * B * S), "acc_out": guarded(B * n_cls * D), "h_part": guarded(B), "x_next": guarded(R * D), "rs": guarded(R), "seg_next": guarded(B + 1, i32),
            "nh_next": guarded(B, i32), "lm": guarded(R), "pos_next": guarded(R, i32), "totals": guarded(2, i32), "sv": guarded(3 * R), "ycls": guarded(B * n_cls * D),
            "src_next": guarded(R, i32)}
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    yd, segd, nhd, posd, accd = y.to(dev), seg.to(dev), nh.to(dev), pos.to(dev), acc.to(dev)
    sd = [t.to(dev) for t in state]
    lib = _lib.load()
    o = bufs["out"]
    rc = lib.pv_avit_pack_step_long(p(yd), p(segd), p(nhd), p(posd), B, S, D, R, *[p(t) for t in sd], *[p(o, 4 * k * B * S) for k in range(5)], p(accd),
                                    p(bufs["acc_out"]), n_cls, p(bufs["h_part"]), GS, GC, THR, 0, p(bufs["x_next"]), p(bufs["rs"]), p(bufs["seg_next"]),
                                    p(bufs["nh_next"]), p(bufs["lm"]), p(bufs["pos_next"]), p(bufs["totals"]), p(bufs["sv"]), p(bufs["ycls"]), p(bufs["src_next"]),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and bufs["totals"][:2].tolist() == list(st64["totals"])
    g_next, gR, grho, gacc, gh, G = (t.to(dev) if t is not None else None for t in _bwd_args(B, S, D, n_cls, Rn, False, seed=1))
    g_next_g = guarded(Rn * D)
    g_next_g[:Rn * D] = g_next.reshape(-1)
    b2 = {"dy": guarded(R * D), "dy16": guarded(R * D, _lib.operand_dtype()), "dR": guarded(B * S), "G": guarded(B)}
    b2["G"][:B] = G
    rc = lib.pv_avit_pack_step_long_bwd(p(g_next_g), p(segd), p(nhd), p(posd), p(bufs["seg_next"]), p(bufs["src_next"]), p(bufs["sv"]), p(bufs["ycls"]), p(gR),
                                        p(grho), p(gacc), p(gh), p(b2["G"]), p(b2["dy"]), p(b2["dy16"]), p(b2["dR"]), B, S, D, R, Rn, n_cls, GS, 0,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    for name, t in {**bufs, **b2}.items():
        tail = t[-PAD:]
        assert bool((tail == (SENT if t.dtype.is_floating_point else 77)).all()), name
    # rows behind R' of the next packed input are not written either
    assert bool((bufs["x_next"][Rn * D:] == SENT).all()) and bool((bufs["pos_next"][Rn:] == 77).all()) and bool((bufs["src_next"][Rn:] == 77).all())
    assert torch.isfinite(b2["dy"][:R * D]).all() and bool((b2["dy"][:R * D] != SENT).all())


# ---- the eval forward against the reference fixtures ---------------------------------------------------------------------------------------------------
def _long_model(name, dev, train=False):
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    case = META["cases"][name]
    model = AdaptiveVisionTransformer(**case["kwargs"])
    model = model.train() if train else model.eval()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(case["synth_cfg"], seed=case["seed"]).items()}, strict=True)
    return model.to(dev) if dev is not None else model


def _long_images(name, batch=None, seed=None):
    case = META["cases"][name]
    return torch.from_numpy(synth.synth_images(batch or case["batch"], case["kwargs"]["image_size"], seed=case["seed"] if seed is None else seed, name="avit"))


def _entering(counter, S):
    """Longest packed segment ENTERING every layer, from a forward's own counter_token [B, S] (layer 0: S)."""
    L = int(META["cases"]["avit_long_226"]["kwargs"]["num_layers"])
    out = [S]
    for l in range(1, L):
        live = (counter > l).sum(dim=1)
        out.append(int((live + (live < S).long()).max()))
    return out


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_long_model_matches_the_reference_fixture(name, mode, monkeypatch):
    """The HIP eval forward (PEEKVIT_AMD_BACKEND=hip: no composite behind it) against the REAL reference's outputs, on the images whose
    counter_token equals the reference's - at least half of them (tests/test_hip_avit.py's cap; the fp64 composite agrees on all of them,
    tests/test_avit_long_host.py).  Logits within BASELINE's 1e-3 in f16 and that file's 8e-3 in bf16, rho_token within its 2e-2, the layer scores
    within its 5e-3.  Streaming ragged attention exactly in the layers whose longest segment exceeds 208 rows, the resident weighted kernel below;
    pv_avit_pack_step_long once per layer and no pv_act_step; fewer rows than L * B * S."""
    from peekvit_amd import engine, ops
    dev = _dev()
    monkeypatch.setenv("PEEKVIT_AMD_BACKEND", "hip")
    g = np.load(os.path.join(GOLDEN, "avit_long.npz"))
    case = META["cases"][name]
    model, x = _long_model(name, dev), _long_images(name).to(dev)
    B, S, L = case["batch"], case["tokens"], case["kwargs"]["num_layers"]
    long0, rows0 = engine.avit_long_layers, engine.act_rows
    with torch.no_grad(), engine.precision(mode), ops.KernelTimer() as kt:
        logits = model(x)
    torch.cuda.synchronize()
    enc = model.encoder
    depth = enc.counter_token.cpu()
    same = (depth.numpy() == g[name + "/counter_token"]).all(axis=1)
    err = rel_l2(logits[torch.from_numpy(same)], g[name + "/logits"][same]) if same.any() else float("nan")
    hs = torch.stack(enc.halting_score_layer).cpu().numpy()
    print(f"\n{name} [{mode}]: images agreeing {int(same.sum())}/{B}, tokens differing {int((depth.numpy() != g[name + '/counter_token']).sum())}, "
          f"logits rel L2 on them {err:.3g}, scores max abs {np.abs(hs - g[name + '/halting_score_layer']).max():.3g}")
    seq = [r[0] for r in kt.records]
    entering = _entering(depth, S)
    attn = [n for n in seq if n.startswith("pv_attention")]
    assert attn == ["pv_attention_varlen_w_stream_bf16" if n > 208 else "pv_attention_varlen_w_bf16" for n in entering], (attn, entering)
    assert seq.count("pv_avit_pack_step_long") == L and "pv_act_step" not in seq
    assert engine.avit_long_layers - long0 == sum(n > 208 for n in entering) >= 1
    assert engine.act_rows - rows0 < L * B * S
    assert same.mean() >= 0.5, f"{int(same.sum())} of {B} images decide every token as the reference does"
    assert err < (1e-3 if mode == "f16" else 8e-3), err
    assert np.allclose(enc.rho_token.cpu().numpy()[same], g[name + "/rho_token"][same], atol=2e-2)
    assert np.allclose(hs, g[name + "/halting_score_layer"], atol=5e-3)


def test_a_197_token_model_runs_the_launches_it_ran():
    """Unchanged behaviour below the bound: the eval forward of a 197-token model records pv_act_step and nothing named _long or _w_; its packed
    training step records pv_avit_pack_step_train / pv_avit_pack_step_bwd and nothing named _long or _stream."""
    from peekvit_amd import engine, ops
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    dev = _dev()
    torch.manual_seed(0)
    kw = dict(image_size=112, patch_size=8, num_layers=3, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10, gate_center=2.0)
    model = AdaptiveVisionTransformer(**kw).to(dev)
    assert model.seq_length == 197
    x = torch.randn(3, 3, 112, 112, generator=torch.Generator().manual_seed(1)).to(dev)
    long0 = engine.avit_long_layers
    with torch.no_grad(), engine.precision("f16"), ops.KernelTimer() as kt:
        model.eval()(x)
    torch.cuda.synchronize()
    seq = [r[0] for r in kt.records]
    assert seq.count("pv_act_step") == 3 and "pv_attention_varlen_bf16" in seq and not [n for n in seq if "_long" in n or "varlen_w" in n], seq
    assert engine.avit_long_layers == long0
    model.train().set_packed_training(True)
    assert model._packed_training_ok() and not model._long_packed_training_ok()
    with ops.KernelTimer() as kt:
        torch.nn.functional.cross_entropy(model(x), torch.arange(3, device=dev)).backward()
    torch.cuda.synchronize()
    seq = [r[0] for r in kt.records]
    assert seq.count("pv_avit_pack_step_train") == 3 and seq.count("pv_avit_pack_step_bwd") == 3
    assert not [n for n in seq if "_long" in n or "_stream" in n], seq


# ---- training ------------------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def _train_case(name, heads, switch, mode="auto", kind="yaml", B=3):
    """One training step of the fixture model `name` (its dims with `heads` heads) with switch "fused" or "packed", and its fp64 replay
    (tests/avit_train_ref.py: the composite in fp64 taking the step's own halting decisions).  Cached: the fused figures stand next to the packed ones."""
    key = (name, heads, switch, mode, kind)
    if key in _cache:
        return _cache[key]
    from peekvit_amd import engine, ops, train_engine
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    dev = _dev()
    case = META["cases"][name]
    kw = dict(case["kwargs"], num_heads=heads)
    cfg = dict(case["synth_cfg"], num_heads=heads)
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(cfg, seed=case["seed"]).items()}

    def make():
        m = AdaptiveVisionTransformer(**kw).train()
        m.load_state_dict(sd, strict=True)
        return m
    x, labels = _long_images(name, batch=B), torch.arange(B) % 10
    model = make().to(dev)
    getattr(model, f"set_{switch}_training")(True)
    rows0, dense0, long0 = engine.avit_train_rows, engine.avit_train_dense_rows, engine.avit_train_long_layers
    with engine.precision(mode), ops.KernelTimer() as kt:
        logits = model(x.to(dev))
        enc = model.encoder
        loss = ref.loss_terms(kind, logits, labels.to(dev), enc.rho_token, enc.halting_score_layer)
        loss.backward()
        skipped, operand = train_engine.last_step_skipped(model), train_engine.pass_operand(model)
    torch.cuda.synchronize()
    counter = enc.counter_token.detach().cpu()
    m64 = make().double()
    lg64, rho64, sc64, cnt64, _ = ref.model_forward(m64, x, counter=counter)
    assert torch.equal(cnt64, counter.double())
    loss64 = ref.loss_terms(kind, lg64, labels, rho64, sc64)
    loss64.backward()
    gp = dict(model.named_parameters())
    names = [n for n, p in m64.named_parameters() if p.grad is not None]
    assert not [n for n in names if gp[n].grad is None]
    got = torch.cat([gp[n].grad.detach().cpu().double().reshape(-1) for n in names])
    want = torch.cat([p.grad.reshape(-1) for n, p in m64.named_parameters() if p.grad is not None])
    with torch.no_grad():
        free = ref.model_forward(make().double(), x)[3]
    r = {"logits": rel_l2(logits, lg64), "rho": rel_l2(enc.rho_token, rho64), "scores": rel_l2(torch.stack(enc.halting_score_layer), torch.stack(sc64)),
         "loss": float(loss.detach()), "loss64": float(loss64.detach()), "grad": float((got - want).norm() / float(want.norm())),
         "finite": bool(torch.isfinite(got).all()), "skipped": skipped, "operand": operand, "seq": [rec[0] for rec in kt.records],
         "flipped": float((counter.double() != free).double().mean()), "counter": counter, "S": model.seq_length, "L": len(enc.layers),
         "dense_rows": engine.avit_train_dense_rows - dense0, "rows": engine.avit_train_rows - rows0, "long_layers": engine.avit_train_long_layers - long0,
         "last_rows": list(engine.avit_train_last_rows) if switch == "packed" else None}
    _cache[key] = r
    return r


def _show(r):
    return {k: r[k] for k in ("logits", "rho", "scores", "loss", "loss64", "grad", "flipped", "skipped", "operand")}


@pytest.mark.parametrize("name,heads", [("avit_long_226", 2), ("avit_long_442", 4), ("avit_long_442", 2)])
def test_long_fused_training_step_against_the_fp64_replay(name, heads):
    """set_fused_training at 226 tokens (head dim 64) and 442 tokens (head dims 32 and 64), cross-entropy + the two A-ViT losses, fp16 operands under
    the loss scale: logits within 1e-3 and the complete gradient within 2e-3 of the fp64 composite replaying the step's decisions (the README's
    training contract); pv_avit_act_fwd and the streaming attention backward in the kernel record (the parent runs the composite here)."""
    r = _train_case(name, heads, "fused")
    print(name, heads, "fused", _show(r))
    seq = r["seq"]
    assert seq.count("pv_avit_act_fwd") == r["L"] and seq.count("pv_avit_act_bwd") == r["L"], sorted(set(seq))
    assert seq.count("pv_attention_stream_bwd16_bf16") == r["L"], sorted(set(seq))
    assert r["finite"] and not r["skipped"] and r["operand"] == "f16"
    assert r["flipped"] <= 0.03, r["flipped"]          # the replay must not hide a broken halting kernel
    assert r["logits"] < 1e-3, r["logits"]
    assert r["grad"] < 2e-3, r["grad"]


@pytest.mark.parametrize("name", ["avit_long_226", "avit_long_257", "avit_long_442"])
def test_long_packed_training_step_against_the_fp64_replay_and_the_long_fused_path(name):
    """set_packed_training at 226, 257 and 442 tokens (head dim 64) against the same replay, the same bounds, next to the long fused path on the same
    inputs: every packed error at most 1.5 x the fused one + 1e-4 (tests/test_hip_avit_packed_train.py's margin between its two paths).  The rows
    per layer start at B * S and never grow; the chunked step and its backward once per layer, the resident pair never; the attention pair streams
    exactly in the layers whose longest segment exceeds 208 rows."""
    p = _train_case(name, 2, "packed")
    d = _train_case(name, 2, "fused")
    print(name, "packed", _show(p), "fused", _show(d), "rows per layer", p["last_rows"])
    L, S = p["L"], p["S"]
    seq = p["seq"]
    assert seq.count("pv_avit_pack_step_long") == L and seq.count("pv_avit_pack_step_long_bwd") == L, sorted(set(seq))
    assert "pv_avit_pack_step_train" not in seq and "pv_avit_pack_step_bwd" not in seq and "pv_avit_act_fwd" not in seq
    entering = _entering(p["counter"], S)
    fw = [n for n in seq if n in ("pv_attention_varlen_w_stream_lse_bf16", "pv_attention_varlen_w_lse_bf16")]
    bw = [n for n in seq if n in ("pv_attention_varlen_w_stream_bwd16_bf16", "pv_attention_varlen_w_bwd16_bf16")]
    assert fw == ["pv_attention_varlen_w_stream_lse_bf16" if n > 208 else "pv_attention_varlen_w_lse_bf16" for n in entering], (fw, entering)
    assert bw == ["pv_attention_varlen_w_stream_bwd16_bf16" if n > 208 else "pv_attention_varlen_w_bwd16_bf16" for n in reversed(entering)], (bw, entering)
    assert p["long_layers"] == sum(n > 208 for n in entering) >= 1
    rows = p["last_rows"]
    assert len(rows) == L and rows[0] == 3 * S and all(a >= b for a, b in zip(rows, rows[1:])) and rows[-1] < 3 * S
    assert p["dense_rows"] == L * 3 * S and p["rows"] == sum(rows)
    assert p["finite"] and not p["skipped"] and p["operand"] == "f16"
    assert p["flipped"] <= 0.03, p["flipped"]
    assert p["logits"] < 1e-3 and p["grad"] < 2e-3, (p["logits"], p["grad"])
    assert abs(p["loss"] - p["loss64"]) < dense_t._bound("auto", "loss") * abs(p["loss64"]), (p["loss"], p["loss64"])
    for what in ("logits", "rho", "scores", "grad"):
        assert p[what] <= 1.5 * d[what] + 1e-4, (what, p[what], d[what])


def test_an_overflowing_long_packed_step_is_dropped_like_the_resident_one():
    """Inputs beyond fp16's range in the fp16 pass at 226 tokens: the step is dropped - every .grad is None and last_step_skipped is true - on the
    long packed path and the long fused one alike."""
    import warnings
    from peekvit_amd import engine, train_engine
    dev = _dev()
    x = (_long_images("avit_long_226", batch=2) * 1.0e6).to(dev)
    labels = torch.arange(2, device=dev)
    with engine.precision("auto"):
        for switch in ("fused", "packed"):
            m = _long_model("avit_long_226", dev, train=True)
            getattr(m, f"set_{switch}_training")(True)
            assert train_engine.pass_operand(m) == "f16"
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                torch.nn.functional.cross_entropy(m(x), labels).backward()
                assert train_engine.last_step_skipped(m), switch
            assert all(p.grad is None for p in m.parameters()), switch
