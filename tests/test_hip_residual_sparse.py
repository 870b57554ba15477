"""ResidualViT exact token compaction on the MI355X (include/peekvit_hip_sparse.h): the weighted ragged attention
(pv_attention_varlen_w_bf16) against fp64 and against dense attention over physically repeated rows, the gate + compaction step
(pv_residual_pack_step) against the torch restatement of tests/residual_sparse_ref.py, and the model forward with compaction on against the
real reference's golden outputs, the stock-op composite, and its own dense path."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from peekvit_amd import synth
import residual_sparse_ref as R

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "residualvit_sparse_meta.json")))
TOL_CONTRACT = 1e-3
MODES = ("bf16", "f16")
# unit roundoff of the 16-bit operand types (bf16: 8 significand bits, fp16: 11): what one rounding to nearest of a probability / an
# output element costs, relative
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
EXTRA = dict(gate_type="sigmoid", gate_temp=1, add_budget_token="learnable", gate_threshold=0.5)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _model(name, gate_bias, gate_gain=None, dev=None):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    cfg = synth.MODEL_CONFIGS[name]
    extra = dict(EXTRA, gate_bias=gate_bias)
    m = ResidualVisionTransformer(**cfg, **extra)
    scfg = dict(cfg, **extra)
    sd = synth.synth_state_dict(scfg, "residualvit") if gate_gain is None else synth.residual_sparse_state_dict(scfg, gate_gain=gate_gain)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m.eval()
    return scfg, (m.to(dev) if dev is not None else m)


def _sparse_model(dev):
    return _model(META["model"], META["kwargs"]["gate_bias"], META["gate_gain"], dev)


def _counters():
    from peekvit_amd import engine
    return engine.sparse_rows, engine.sparse_dense_rows, engine.sparse_syncs, engine.sparse_dense_forwards


# ---- weighted ragged attention -------------------------------------------------------------------------------------------------
def _packed_qkv(lens, H, dh, seed, dtype, dev):
    g = torch.Generator().manual_seed(seed)
    R_, D = sum(lens), H * dh
    qkv = torch.randn(R_, 3 * D, generator=g)
    qkv[:, :D] *= dh ** -0.5
    qkv[:, 2 * D:].clamp_(-3.5, 3.5)
    return qkv.to(dtype).to(dev)


def _mults(lens, seed, hi=197):
    g = torch.Generator().manual_seed(seed)
    mult = torch.randint(1, hi + 1, (sum(lens),), generator=g)
    mult[torch.rand(sum(lens), generator=g) < 0.6] = 1
    return mult


def _attn_bound(mode, qkv, D):
    """|out - exact| of one output element: the probabilities are rounded to the operand type once (relative U16 each, so U16 * max|v| on a
    convex combination), the output once more (U16 * |out| <= U16 * max|v|); q, k, v are exact 16-bit inputs and everything between is fp32
    (exp2 and the sums: ~1e-6 relative, covered by the 1e-5)."""
    return 2 * U16[mode] * float(qkv[:, 2 * D:].abs().max()) + 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_attention_w_matches_fp64_with_random_multiplicities(mode):
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    H, dh = 12, 64
    lens = [2, 3, 15, 16, 17, 33, 100, 197, 198, 208, 64, 1]
    seg = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
    mult = _mults(lens, 5)
    lm = torch.log(mult.float()).to(dev)
    with engine.precision(mode):
        qkv = _packed_qkv(lens, H, dh, 3, _lib.operand_dtype(), dev)
        out = torch.full((sum(lens), H * dh), float("nan"), dtype=qkv.dtype, device=dev)
        ops.attention_varlen_w(qkv, out, seg, lm, max(lens), H, dh)
        torch.cuda.synchronize()
    ref = R.attention_w_ref(qkv.double().cpu(), seg, torch.log(mult.double()), H)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max())
    print(f"\nattention_w {mode}: max |err| {err:.3g} (bound {_attn_bound(mode, qkv, H * dh):.3g})")
    assert err <= _attn_bound(mode, qkv, H * dh)


@pytest.mark.parametrize("mode", MODES)
def test_attention_w_equals_dense_attention_over_repeated_rows(mode):
    """A key of multiplicity n = that key physically n times in pv_attention_bf16's dense sequence."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    B, H, dh, S = 9, 6, 64, 197
    g = torch.Generator().manual_seed(17)
    lens, mults = [], []
    for b in range(B):
        L = int(torch.randint(3, 60, (1,), generator=g))
        cut = torch.sort(torch.randperm(S - 1, generator=g)[:L - 1] + 1).values.tolist()       # S split into L positive parts
        mults += [hi - lo for lo, hi in zip([0] + cut, cut + [S])]
        lens.append(L)
    mult = torch.tensor(mults)
    seg = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv = _packed_qkv(lens, H, dh, 23, dt, dev)
        out = torch.empty((sum(lens), H * dh), dtype=dt, device=dev)
        ops.attention_varlen_w(qkv, out, seg, torch.log(mult.float()).to(dev), max(lens), H, dh)
        rep = torch.repeat_interleave(torch.arange(sum(lens)), mult).to(dev)
        dense_in = qkv[rep].contiguous()
        assert dense_in.shape[0] == B * S
        dense = torch.empty((B * S, H * dh), dtype=dt, device=dev)
        ops.attention(dense_in, dense, B, S, H, dh)
        torch.cuda.synchronize()
    first = torch.cumsum(mult, 0) - mult                       # the first copy of every packed row
    a, d = out.double().cpu(), dense.double().cpu()[first]
    err = float((a - d).abs().max())
    print(f"\nattention_w vs repeated rows {mode}: max |diff| {err:.3g}")
    assert err <= 2 * _attn_bound(mode, qkv, H * dh)             # (each side within the bound of the exact value)


@pytest.mark.parametrize("nkt", range(1, 14))
def test_attention_w_every_tile_bound(nkt):
    """Every NKT instantiation (longest segment 16 nkt and 16 nkt - 15), batches on both sides of pv_bh_map's grouped branch, length-1 and
    length-2 segments with large multiplicities; and a segment's rows do not depend on where in the batch it sits."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    B, H = ((8, 1), (13, 6), (67, 12))[nkt % 3]
    dh = 64
    for longest in (16 * nkt, 16 * nkt - 15):
        g = torch.Generator().manual_seed(100 * nkt + longest)
        lens = torch.randint(1, longest + 1, (B,), generator=g)
        lens[torch.randperm(B, generator=g)[:2]] = longest
        lens[torch.randperm(B, generator=g)[:2]] = torch.tensor([1, min(2, longest)])
        lens[0] = longest
        lens = lens.tolist()
        mult = _mults(lens, nkt, hi=255)
        seg = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
        perm = [B - 1] + list(range(1, B - 1)) + [0]
        lens2 = [lens[i] for i in perm]
        seg2 = torch.tensor([0] + list(np.cumsum(lens2)), dtype=torch.int32, device=dev)
        for mode in MODES:
            with engine.precision(mode):
                dt = _lib.operand_dtype()
                qkv = _packed_qkv(lens, H, dh, nkt, dt, dev)
                lm = torch.log(mult.float()).to(dev)
                out = torch.full((sum(lens), H * dh), float("nan"), dtype=dt, device=dev)
                ops.attention_varlen_w(qkv, out, seg, lm, longest, H, dh)
                qkv2 = torch.cat([qkv[int(seg[i]):int(seg[i + 1])] for i in perm]).contiguous()
                lm2 = torch.cat([lm[int(seg[i]):int(seg[i + 1])] for i in perm]).contiguous()
                out2 = torch.full_like(out, float("nan"))
                ops.attention_varlen_w(qkv2, out2, seg2, lm2, longest, H, dh)
                torch.cuda.synchronize()
            ref = R.attention_w_ref(qkv.double().cpu(), seg, torch.log(mult.double()), H)
            got = out.double().cpu()
            assert torch.isfinite(got).all()
            err = float((got - ref).abs().max())
            assert err <= _attn_bound(mode, qkv, H * dh), f"nkt={nkt} longest={longest} B={B} H={H} {mode}: max |err| {err:.3g} vs fp64"
            L0 = lens[0]
            assert torch.equal(out2[-L0:], out[:L0]), "image 0's rows moved to image B-1"
            assert torch.equal(out2[:lens[B - 1]], out[-lens[B - 1]:]), "image B-1's rows moved to image 0"


def test_attention_w_refuses_what_it_does_not_take():
    from peekvit_amd import _lib, ops
    import ctypes as C
    dev = _dev()
    lib = _lib.load("bf16")
    qkv = torch.zeros((4, 3 * 64), dtype=torch.bfloat16, device=dev)
    out = torch.full((4, 64), 7.0, dtype=torch.bfloat16, device=dev)
    seg = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    lm = torch.zeros(4, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(ops.raw_stream(0))
    assert lib.pv_attention_varlen_w_bf16(p(qkv), p(out), p(seg), p(lm), 1, 209, 1, 64, None, s) == -2      # PV_ERR_UNSUPPORTED
    assert lib.pv_attention_varlen_w_bf16(p(qkv), p(out), p(seg), p(lm), 1, 4, 2, 32, None, s) == -2
    assert lib.pv_attention_varlen_w_bf16(p(qkv), p(out), p(seg), None, 1, 4, 1, 64, None, s) == -1           # PV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                       # nothing was launched


# ---- gate + compaction step ----------------------------------------------------------------------------------------------------
def _pack_inputs(B, N, D, seed, gain=3.0, min_margin=1e-4, dense=False):
    """A packed row matrix as a later layer sees it: segments of 2 .. N + 2 rows, every middle row standing for one or more of the image's N
    tokens.  Built on the CPU; rows whose gate margin |sigmoid - thr| is under `min_margin` in fp32 are redrawn until none is left (a
    condition on the inputs: the live / collapsed decision of every row is then the same in any arithmetic that is 1e-4 accurate).
    dense: the layer-0 state instead - every segment has all N + 2 rows, token t is row t + 1, every multiplicity is 1."""
    g = torch.Generator().manual_seed(seed)
    n_mid = torch.full((B,), N) if dense else torch.randint(0, N + 1, (B,), generator=g)
    n_mid[0] = N
    if B > 1 and not dense:
        n_mid[B - 1] = 0
    if B > 2 and not dense:
        n_mid[1] = min(1, N)
    lens = (n_mid + 2).tolist()
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Rr = int(seg[-1])
    tok_row = np.zeros((B, N), dtype=np.int64)
    mult = np.ones(Rr, dtype=np.int64)
    for b in range(B):
        k = lens[b] - 2
        if k == 0:
            tok_row[b] = 0          # (no middle row: such an image's tokens are not looked up by the model; the kernels clamp)
            continue
        rows = torch.cat([torch.arange(k), torch.randint(0, k, (N - k,), generator=g)])
        rows = (rows if dense else rows[torch.randperm(N, generator=g)]) + 1
        tok_row[b] = rows.numpy()
        mult[seg[b] + 1:seg[b] + 1 + k] = np.bincount(rows.numpy() - 1, minlength=k)
    x = torch.randn(Rr, D, generator=g)
    wg = torch.randn(D, generator=g) * gain / D ** 0.5
    wb = torch.randn(D, generator=g) / D ** 0.5
    bg, bb = 0.05, -0.02
    for _ in range(50):
        margin = R.pack_step_ref(x, seg, mult, tok_row, wg, bg, wb, bb, 1.0, 0.0)["margin"]
        bad = torch.nonzero(margin < 10 * min_margin).reshape(-1)
        if bad.numel() == 0:
            break
        x[bad] = torch.randn(bad.numel(), D, generator=g)
    else:
        raise AssertionError("rejection sampling did not converge")
    return x, seg, mult, tok_row, wg, bg, wb, bb


def _run_pack_step(x, seg, mult, tok_row, wg, bg, wb, bb, dev, ln=None):
    from peekvit_amd import ops, _lib
    B, N = tok_row.shape
    Rr, D = x.shape
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    nxt = (torch.full((Rr, D), float("nan"), device=dev), torch.full((Rr,), float("nan"), device=dev),
           torch.full((Rr,), -7, dtype=torch.int32, device=dev), torch.full((Rr,), float("nan"), device=dev),
           torch.full((B + 1,), -7, dtype=torch.int32, device=dev), torch.full((B, N), -7, dtype=torch.int32, device=dev))
    mask = torch.full((B, N), float("nan"), device=dev)
    thr = torch.full((B,), float("nan"), device=dev)
    totals = torch.full((2,), -7, dtype=torch.int32, device=dev)
    h = None
    if ln is not None:
        h = torch.full((Rr, D), float("nan"), dtype=_lib.operand_dtype(), device=dev)
        ln = (f32(ln[0]), f32(ln[1]), ln[2], h)
    ops.residual_pack_step(x.to(dev), i32(seg), i32(mult), i32(tok_row), f32(wg), f32([bg]), f32(wb), f32([bb]), 1.0, 0.0, nxt, mask, thr,
                           totals, ln=ln)
    torch.cuda.synchronize()
    return nxt, mask, thr, totals, h


def _check_pack_step(B, N, D, seed, dev, mode="f16"):
    from peekvit_amd import engine
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_inputs(B, N, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    with engine.precision(mode):
        nxt, mask, thr, totals, h = _run_pack_step(x, seg, mult, tok_row, wg, bg, wb, bb, dev, ln=(gamma, beta, 1e-6))
    # the reference in fp64 on the GPU (the production size is 1.2 GB of fp32 rows)
    xd = x.to(dev).double()
    ref = R.pack_step_ref(xd, seg, mult, tok_row, wg.to(dev), bg, wb.to(dev), bb, 1.0, 0.0)
    Rn, longest = ref["totals"]
    # integer tables: exactly equal
    assert totals.tolist() == [Rn, longest]
    assert np.array_equal(nxt[4].cpu().numpy(), ref["seg_next"])
    assert np.array_equal(nxt[2][:Rn].cpu().numpy(), ref["mult_next"])
    has_mid = np.diff(seg) > 2
    assert np.array_equal(nxt[5].cpu().numpy()[has_mid], ref["tok_row_next"][has_mid])
    assert int(ref["mult_next"].sum()) == int(mult.sum())                     # no token is lost or counted twice
    # masks and thresholds: fp32 rounding.  A wave sums its D products as 64 lane chains of D / 256 fused terms and a 6-level tree:
    # |error of the logit| <= (D / 256 + 7) u32 sum|x_i w_i| (u32 = 2^-24); the sigmoid is 1/4-Lipschitz and costs a few ulps itself.
    u32 = 2.0 ** -24
    depth = D / 256 + 7
    img = torch.from_numpy(np.repeat(np.arange(B), np.diff(seg))).to(dev)
    tol_thr = 0.25 * depth * u32 * (xd[torch.from_numpy(seg[1:] - 1).to(dev)].abs() @ wb.to(dev).double().abs()) + 8 * u32
    assert bool(((thr.double() - ref["thr_out"]).abs() <= tol_thr).all())
    tol_row = 0.25 * depth * u32 * (xd.abs() @ wg.to(dev).double().abs()) + 8 * u32 + tol_thr[img]
    tok_abs = torch.from_numpy(seg[:-1, None] + tok_row).to(dev)
    hm = torch.from_numpy(has_mid).to(dev)
    dm = (mask.double() - ref["mask_out"]).abs()
    assert bool((dm <= tol_row[tok_abs])[hm].all()), f"mask error {float(dm[hm].max()):.3g}"
    assert bool(((mask == 0) == (ref["mask_out"] == 0))[hm].all())
    rs_err = (nxt[1][:Rn].double() - ref["row_scale_next"]).abs()
    assert float(rs_err.max()) <= float(tol_row.max())
    # log_mult = logf(mult), exactly 0 at multiplicity 1.  HIP documents its device logf to 1 - 2 ulp and hipcc may lower it to the hardware
    # log2 (1 ulp) times ln 2 (two more roundings): 4 ulp = 2^-21 relative, i.e. < 3e-6 absolute at multiplicity 198 - the attention kernel's
    # own exp2 of the score it is added to is no more accurate than that
    lm64 = torch.log(nxt[2][:Rn].double())
    lerr = (nxt[3][:Rn].double() - lm64).abs()
    print(f"log_mult: worst error {float((lerr / lm64.clamp(min=1e-30)).max()) * 2 ** 23:.2f} ulp")
    assert bool((lerr <= 2.0 ** -21 * lm64).all())
    # rows: mask * x (one more fp32 rounding), zero rows exactly zero
    zero = ref["row_scale_next"] == 0
    assert bool((nxt[0][:Rn][zero] == 0).all()) and bool((nxt[1][:Rn][zero] == 0).all())
    scale_tol = float(tol_row.max())
    xe = (nxt[0][:Rn].double() - ref["x_next"]).abs()
    assert bool((xe <= scale_tol * float(xd.abs().max()) + 2 * u32 * ref["x_next"].abs()).all()), f"x_next error {float(xe.max()):.3g}"
    # row_scale * LN1 in the operand type: one 16-bit rounding of a value bounded by |gamma| sqrt(D) ... here |LN| < 8
    ln_ref = ref["row_scale_next"][:, None] * torch.nn.functional.layer_norm(ref["x_next"], (D,), gamma.to(dev).double(), beta.to(dev).double(), 1e-6)
    he = (h[:Rn].double() - ln_ref).abs()
    assert bool((he <= U16[mode] * ln_ref.abs() + 8.0 * scale_tol + 1e-5).all()), f"ln_out error {float(he.max()):.3g}"
    assert bool((h[:Rn][zero] == 0).all())
    return Rn, int(seg[-1])


@pytest.mark.parametrize("B,N,D", [(1, 1, 128), (3, 16, 128), (7, 5, 256), (33, 196, 384), (5, 206, 768), (1030, 7, 128)])
def test_pack_step_small_sizes(B, N, D):
    dev = _dev()
    for mode in MODES:
        _check_pack_step(B, N, D, 7 * B + N, dev, mode)


def test_pack_step_production_size():
    """B = 2048 images of up to 198 rows, D = 768."""
    dev = _dev()
    Rn, Rin = _check_pack_step(2048, 196, 768, 99, dev)
    print(f"\npack step at production size: {Rin} rows in, {Rn} rows out")
    assert Rn < Rin


DENSE_SEED = {(3, 5, 128): 0, (2, 9, 516): 0}       # (chosen on the CPU: the fp64 reference has a live and a collapsed token in every image)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N,D", sorted(DENSE_SEED))
def test_pack_step_on_dense_segments_gives_the_dense_gate_bits(B, N, D, mode):
    """On a packed matrix in its layer-0 state (every segment holds all N + 2 rows, multiplicity 1, token t in row t + 1) the packed gate sees what
    pv_residual_gate sees, and both take their arithmetic from the same functions of pv_rows.h: thresholds, masks and every kept row of both
    planes agree bit for bit; the tokens the gate zeroes share one row of exact zeros."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    S = N + 2
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_inputs(B, N, D, DENSE_SEED[(B, N, D)], dense=True)
    assert np.array_equal(np.diff(seg), np.full(B, S)) and bool((mult == 1).all()) and np.array_equal(tok_row, np.tile(np.arange(1, N + 1), (B, 1)))
    ref_mask = R.pack_step_ref(x.double(), seg, mult, tok_row, wg, bg, wb, bb, 1.0, 0.0)["mask_out"].reshape(B, N)
    assert bool((ref_mask > 0).any(dim=1).all()) and bool((ref_mask == 0).any(dim=1).all())      # before any launch
    g = torch.Generator().manual_seed(1)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(-1).to(dev).contiguous()
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    with engine.precision(mode):
        nxt, mask, thr, totals, h = _run_pack_step(x, seg, mult, tok_row, wg, bg, wb, bb, dev, ln=(gamma, beta, 1e-6))
        xd = x.to(dev).reshape(B, S, D)
        xo = torch.full_like(xd, float("nan"))
        hd = torch.full((B * S, D), float("nan"), dtype=_lib.operand_dtype(), device=dev)
        thr_d = torch.full((B,), float("nan"), device=dev)
        mask_d, _ = ops.residual_gate(xd, xo, f32(wg), f32([bg]), f32(wb), f32([bb]), 1.0, 0.0, thr_out=thr_d, ln=(f32(gamma), f32(beta), 1e-6, hd))
        torch.cuda.synchronize()
    assert torch.equal(bits(thr), bits(thr_d))
    assert torch.equal(bits(mask), bits(mask_d.reshape(B, N)))
    assert bool(((mask > 0).cpu() == (ref_mask > 0)).all())
    x_next, seg_next, tok_next = nxt[0], nxt[4].tolist(), nxt[5].cpu()
    hd = hd.reshape(B, S, D)
    for b in range(B):
        d0, Ln = seg_next[b], seg_next[b + 1] - seg_next[b]
        live = mask[b].cpu() > 0
        assert Ln == 2 + int(live.sum()) + 1
        pairs = [(0, 0), (Ln - 1, S - 1)] + [(int(tok_next[b, t]), t + 1) for t in range(N) if live[t]]
        assert len({j for j, _ in pairs}) == len(pairs) and all(0 <= j < Ln for j, _ in pairs)
        for j, i in pairs:
            assert torch.equal(bits(x_next[d0 + j]), bits(xo[b, i])), (b, j, i)
            assert torch.equal(bits(h[d0 + j]), bits(hd[b, i])), (b, j, i)
        dead = {int(tok_next[b, t]) for t in range(N) if not live[t]}
        assert dead == {Ln - 2}                                                     # one row for all of them, in front of the budget row
        assert bool((bits(x_next[d0 + Ln - 2]) == 0).all()) and bool((bits(h[d0 + Ln - 2]) == 0).all())


def test_pack_step_refuses_bad_arguments():
    from peekvit_amd import _lib
    dev = _dev()
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_inputs(2, 4, 128, 1)
    with pytest.raises(_lib.PeekvitHipError):
        _run_pack_step(x[:, :126].contiguous(), seg, mult, tok_row, wg[:126], bg, wb[:126], bb, dev)          # D % 4
    big = np.zeros((2, 207), dtype=np.int64)
    with pytest.raises(_lib.PeekvitHipError):
        _run_pack_step(x, seg, mult, big, wg, bg, wb, bb, dev)                                                # N + 2 > 208


# ---- model ---------------------------------------------------------------------------------------------------------------------
def _forward(m, x, mode="auto"):
    from peekvit_amd import engine
    with torch.no_grad(), engine.precision(mode):
        return m(x)


TOL_SAME = 1.5e-3        # fp16-operand logits against the oracle with the SAME rounding points (tests/test_hip_models.py: rounding noise ~6e-4 plus
                         # fp32 summation order, exp2 softmax, table GELU)


def _left_behind(m):
    masks = torch.stack([blk.mask.cpu() for blk in m.encoder.layers]).numpy()
    thr = torch.stack([blk.residual_gate.threshold.cpu() for blk in m.encoder.layers])
    return masks, thr


@pytest.mark.parametrize("tag,name,gb", [("vit_micro_gb0", "vit_micro", 0), ("vit_b_16", "vit_b_16", 10)])
def test_model_parity_on_the_existing_residualvit_fixtures(golden, tag, name, gb):
    """Compaction on, twice per budget.  Mode `auto` (the default path): the contract against the real reference's logits; on the 2-layer toy
    the self-check may escalate, and then the dense path answers - so the explicit `f16` mode follows, where nothing can answer but the packed
    kernels: packed rows must have run, against the oracle with the same rounding points (the toy does not meet 1e-3 of the fp32 reference on
    plain fp16 operands even densely: tests/test_hip_models.py::test_residualvit_parity)."""
    from oracle import vit_oracle as O
    from peekvit_amd import engine
    dev = _dev()
    g = golden("residualvit")
    cfg, m = _model(name, gb, dev=dev)
    m.set_token_compaction(True)
    x_cpu = torch.from_numpy(synth.synth_images(2, cfg["image_size"], seed=0))
    x = x_cpu.to(dev)
    sd = synth.synth_state_dict(cfg, "residualvit")
    sd64 = {k: torch.from_numpy(v.copy()).double() for k, v in sd.items()}
    L, S = cfg["num_layers"], synth.seq_length(cfg) + 1

    def check_state(masks, thr, b, what):
        assert masks.shape == g[f"{tag}_b{b}_masks"].shape
        assert thr.shape == (L, 2, 1, 1) and bool(((thr > 0) & (thr < 1)).all())
        merr = float(np.abs(masks - g[f"{tag}_b{b}_masks"]).max())
        terr = float(np.abs(thr.view(L, -1).double().numpy() - thr64.numpy()).max())
        print(f"{what}: masks {merr:.3g} from the reference's, thresholds {terr:.3g} from the fp64 oracle's")
        assert merr < 2e-3                                                      # every block's mask vs the REAL reference's
        assert np.abs(masks[0] - g[f"{tag}_b{b}_masks"][0]).max() < 1e-5        # first block sees fp32-identical input
        assert terr < 5e-3                                                      # every block's threshold vs the oracle's (as the masks in test_residualvit_parity)

    for b in (0.2, 0.5, 1.0):
        m.set_budget(b)
        _, _, thr64, _ = R.dense_forward(x_cpu.double(), sd64, cfg, b)          # the oracle's dense forward op by op in fp64: thresholds [L, B]
        # ---- the default path ----
        r0, d0, s0, f0 = _counters()
        logits = _forward(m, x).cpu().numpy()
        r1, d1, s1, f1 = _counters()
        packed_answered = engine.last_forward_guarded() and r1 > r0 and f1 == f0
        err = rel_l2(logits, g[f"{tag}_b{b}_logits"])
        print(f"\n{tag} budget {b} auto: logits {err:.3g}, rows {r1 - r0} of {d1 - d0}, dense forwards {f1 - f0}, packed answered {packed_answered}")
        assert err < TOL_CONTRACT
        check_state(*_left_behind(m), b, "  auto")
        if gb == 10:
            # nothing is masked: every packed forward ran exactly the dense rows, and it is the packed path that answered
            assert packed_answered, "the packed path did not produce the answer"
            assert r1 - r0 == d1 - d0 and (d1 - d0) % (L * 2 * S) == 0
        # ---- fp16 operands, no guard: the packed kernels or an error ----
        r0, d0, s0, f0 = _counters()
        l16 = _forward(m, x, "f16").cpu().numpy()
        r1, d1, s1, f1 = _counters()
        assert r1 > r0 and f1 == f0 and s1 - s0 == L and d1 - d0 == L * 2 * S, "the packed path did not run"
        assert sum(engine.sparse_last_rows) == r1 - r0
        same = O.residualvit_forward(x_cpu, sd, cfg, b, "f16").numpy()
        e_same, e_ref = rel_l2(l16, same), rel_l2(l16, g[f"{tag}_b{b}_logits"])
        print(f"{tag} budget {b} f16: logits {e_same:.3g} from the same-rounding oracle, {e_ref:.3g} from the reference, rows {r1 - r0} of {d1 - d0}")
        assert e_same < TOL_SAME
        check_state(*_left_behind(m), b, "  f16")
        if bool((g[f"{tag}_b{b}_masks"] == 0).any()):
            assert r1 - r0 < d1 - d0, "tokens are masked and no row was saved"
        else:
            assert r1 - r0 == d1 - d0
        if name == "vit_b_16":
            assert e_ref < TOL_CONTRACT


def test_model_parity_on_the_sparse_fixture(golden):
    from peekvit_amd import engine
    dev = _dev()
    g = golden("residualvit_sparse")
    cfg, m = _sparse_model(dev)
    m.set_token_compaction(True)
    x = torch.from_numpy(synth.synth_images(META["batch"], cfg["image_size"], seed=0)).to(dev)
    L, S = cfg["num_layers"], synth.seq_length(cfg) + 1
    for b in META["budgets"]:
        m.set_budget(b)
        r0, d0, s0, f0 = _counters()
        logits = _forward(m, x).cpu().numpy()
        r1, d1, s1, f1 = _counters()
        assert engine.last_forward_guarded() and r1 > r0, "the packed path did not produce the answer"
        masks = torch.stack([blk.mask.cpu() for blk in m.encoder.layers]).numpy()
        thr = torch.stack([blk.residual_gate.threshold.cpu() for blk in m.encoder.layers])
        assert thr.shape == (L, META["batch"], 1, 1) and bool(((thr > 0) & (thr < 1)).all())
        err = rel_l2(logits, g[f"b{b}_logits"])
        merr = float(np.abs(masks - g[f"b{b}_masks"]).max())
        terr = float(np.abs(thr.view(L, -1).numpy() - g[f"b{b}_thresholds"]).max())
        share = sum(engine.sparse_last_rows) / float(L * META["batch"] * S)
        sure = g[f"b{b}_margin"] >= META["margin"]
        flips = int(((masks[..., 0] == 0) != (g[f"b{b}_masks"][..., 0] == 0))[sure].sum())
        print(f"\nsparse fixture budget {b}: logits {err:.3g}, masks {merr:.3g}, thresholds {terr:.3g}, rows share {share:.3f} "
              f"(fp64 {float(g[f'b{b}_rows_share']):.3f}), state flips among sure tokens {flips}, left out {1 - sure.mean():.4f}")
        assert err < TOL_CONTRACT
        assert merr < 2e-3
        assert terr < 5e-3
        assert 1 - sure.mean() <= META["max_excluded_fraction"]
        assert flips == 0, "a token with a gate margin of 5e-3 or more is collapsed / live where the reference has it live / collapsed"
        # only a left-out (block, image, token) entry can resolve differently, and it moves at most one row in each of the <= L later blocks:
        # 1 / (B S) of the share per entry, which is L N / S <= L times its weight in the left-out fraction
        assert abs(share - float(g[f"b{b}_rows_share"])) <= L * (1 - sure.mean()) + 1e-9
        assert s1 - s0 >= L


def test_large_batch_against_gpu_composite(monkeypatch):
    """ViT-B/16 dims at batch 2048, the sparse weights: compacting forward (fp16 operands) vs the fp32 stock-op composite on the same GPU."""
    from peekvit_amd import engine
    dev = _dev()
    cfg, m = _sparse_model(dev)
    m.set_budget(0.5)
    x = torch.randn(2048, 3, 224, 224, generator=torch.Generator().manual_seed(11)).to(dev)
    monkeypatch.setenv("PEEKVIT_AMD_BACKEND", "torch")
    with torch.no_grad():
        ref = torch.cat([m(x[i:i + 256]) for i in range(0, 2048, 256)])
    ref_zero = torch.stack([blk.mask for blk in m.encoder.layers])          # (of the last chunk)
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND")
    m.set_token_compaction(True)
    r0, d0, s0, f0 = _counters()
    got = _forward(m, x, "f16")
    r1, d1, s1, f1 = _counters()
    err = rel_l2(got, ref)
    print(f"\nbatch 2048: logits rel L2 {err:.3g}, rows run {r1 - r0} of {d1 - d0} ({(r1 - r0) / (d1 - d0):.3f}), syncs {s1 - s0}")
    assert f1 == f0 and s1 - s0 == cfg["num_layers"]
    assert r1 - r0 < d1 - d0, "compaction ran as many rows as the dense path"
    assert err < 1e-3
    masks = torch.stack([blk.mask for blk in m.encoder.layers])
    assert masks.shape == (cfg["num_layers"], 2048, 196, 1)
    assert float((masks[:, -256:] - ref_zero).abs().max()) < 2e-3


def test_off_restores_the_dense_bits_and_budget_and_batch_changes():
    from peekvit_amd import engine
    dev = _dev()
    cfg, never = _sparse_model(dev)
    _, m = _sparse_model(dev)
    xs = {n: torch.from_numpy(synth.synth_images(n, cfg["image_size"], seed=n)).to(dev) for n in (1, 3, 5)}
    for n, b in ((3, 0.5), (5, 0.2), (1, 0.8), (3, 0.8)):
        never.set_budget(b)
        m.set_budget(b)
        dense = _forward(never, xs[n], "f16")
        dmask = torch.stack([blk.mask for blk in never.encoder.layers])
        m.set_token_compaction(True)
        assert m.token_compaction
        r0 = engine.sparse_rows
        packed = _forward(m, xs[n], "f16")
        assert engine.sparse_rows > r0
        pmask = torch.stack([blk.mask for blk in m.encoder.layers])
        assert packed.shape == dense.shape and pmask.shape == dmask.shape == (cfg["num_layers"], n, 196, 1)
        # both are fp16-operand forwards of the same model: each within the contract of the fp32 reference, so within twice that of each other
        assert rel_l2(packed, dense) < 2 * TOL_CONTRACT, (n, b)
        assert float((pmask - dmask).abs().max()) < 4e-3
        m.set_token_compaction(False)
        assert not m.token_compaction
        r0 = engine.sparse_rows
        off = _forward(m, xs[n], "f16")
        assert engine.sparse_rows == r0
        assert torch.equal(off, dense), "compaction off is not the dense forward bit for bit"
        assert torch.equal(torch.stack([blk.mask for blk in m.encoder.layers]), dmask)


def test_successive_forwards_on_different_images_are_not_replayed():
    from peekvit_amd import engine, autograph
    dev = _dev()
    cfg, m = _sparse_model(dev)
    assert autograph.launch_bound(m, 2)              # (what auto-graph captures after a few clean eager forwards of the dense model)
    m.set_token_compaction(True)
    m.set_budget(0.5)
    _, dense = _sparse_model(dev)
    dense.set_budget(0.5)
    outs = []
    for seed in range(8):
        x = torch.from_numpy(synth.synth_images(2, cfg["image_size"], seed=seed)).to(dev)
        r0, n0 = engine.sparse_rows, autograph.replays
        y = _forward(m, x).clone()
        assert engine.sparse_rows > r0 and engine.last_forward_guarded() and autograph.replays == n0, seed
        assert rel_l2(y, _forward(dense, x)) < 2 * TOL_CONTRACT, seed          # (the dense model next to it may well be replayed)
        outs.append(y)
    assert not engine.guard_state(m).graphs
    assert all(not torch.equal(outs[0], o) for o in outs[1:])


def test_hook_under_encoder_forces_the_dense_path():
    from peekvit_amd import engine
    dev = _dev()
    cfg, m = _sparse_model(dev)
    m.set_token_compaction(True)
    m.set_budget(0.5)
    x = torch.from_numpy(synth.synth_images(3, cfg["image_size"], seed=4)).to(dev)
    seen = []
    h = m.encoder.layers[5].register_forward_hook(lambda mod, inp, out: seen.append((tuple(inp[0].shape), tuple(out.shape))))
    r0, d0, s0, f0 = _counters()
    y = _forward(m, x)
    r1, d1, s1, f1 = _counters()
    h.remove()
    assert seen == [((3, 198, cfg["hidden_dim"]), (3, 198, cfg["hidden_dim"]))], seen
    assert r1 == r0 and f1 == f0 + 1
    y2 = _forward(m, x)
    assert engine.sparse_rows > r1
    assert rel_l2(y2, y) < 2 * TOL_CONTRACT
    # an edited encoder.layers: dense path as well
    keep = m.encoder.layers[3]
    m.encoder.layers[3] = torch.nn.Identity()
    f2 = engine.sparse_dense_forwards
    r2 = engine.sparse_rows
    _forward(m, x)
    assert engine.sparse_dense_forwards == f2 + 1 and engine.sparse_rows == r2
    m.encoder.layers[3] = keep


def test_graphed_forward_raises():
    from peekvit_amd import _lib
    from peekvit_amd.graph import GraphedForward
    dev = _dev()
    cfg, m = _model("vit_micro", 0, dev=dev)
    m.set_budget(0.5)
    m.set_token_compaction(True)
    x = torch.from_numpy(synth.synth_images(2, cfg["image_size"], seed=0)).to(dev)
    with pytest.raises(_lib.PeekvitHipError, match="token compaction"):
        GraphedForward(m, x)
    m.set_token_compaction(False)
    g = GraphedForward(m, x)
    assert g(x).shape == (2, cfg["num_classes"])
