"""ResidualViT exact token compaction past 208 rows per image on the MI355X (include/peekvit_hip_sparse_long.h): the streaming
ragged attention (pv_attention_varlen_w_stream_bf16) against fp64, against dense attention over physically repeated rows and - bit for bit - against
the streaming forward it extends; the chunked gate + compaction step (pv_residual_pack_step_long) against the torch restatement of
tests/residual_sparse_ref.py and - bit for bit - against pv_residual_pack_step; the model forward with compaction on at 227, 402 and 786 rows against
the real reference's golden outputs and its own dense path.  Helpers, bounds and tolerances are tests/test_hip_residual_sparse.py's."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from peekvit_amd import synth
import residual_sparse_ref as R
from test_hip_residual_sparse import (MODES, U16, TOL_CONTRACT, _attn_bound, _counters, _dev, _forward, _mults, _pack_inputs, _packed_qkv,
                                      _run_pack_step)

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "residualvit_sparse_long_meta.json")))
RESIDENT = 208            # PV_SPARSE_MAX_LEN: the longest segment of the LDS-resident kernels


def _seg(lens, dev):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)


# ---- streaming ragged attention ------------------------------------------------------------------------------------------------
ATTN_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 208, 209, 257, 402, 417, 1025]


@pytest.mark.parametrize("mode", MODES)
def test_attention_stream_matches_fp64_with_random_multiplicities(mode):
    """Every segment length around the 64-key block and the 208-row switch in ONE call; multiplicities 1 .. 4096 (about 60 % ones), with a weighted
    key in the first and in the last key block of every segment; rows behind the last segment are not written; a larger max_len changes no bit."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    H, dh = 2, 64
    lens = ATTN_LENS
    seg = _seg(lens, dev)
    mult = _mults(lens, 5, hi=4096)
    g = torch.Generator().manual_seed(6)
    for s0, L in zip(np.cumsum([0] + lens[:-1]), lens):
        mult[s0 + int(torch.randint(0, min(L, 64), (1,), generator=g))] = int(torch.randint(2, 4097, (1,), generator=g))      # first key block
        last0 = (L - 1) // 64 * 64
        mult[s0 + last0 + int(torch.randint(0, L - last0, (1,), generator=g))] = int(torch.randint(2, 4097, (1,), generator=g))  # last key block
    lm = torch.log(mult.float()).to(dev)
    Rr, spare = sum(lens), 7
    with engine.precision(mode):
        qkv = _packed_qkv(lens, H, dh, 3, _lib.operand_dtype(), dev)
        out = torch.full((Rr + spare, H * dh), float("nan"), dtype=qkv.dtype, device=dev)
        ops.attention_varlen_w_stream(qkv, out, seg, lm, max(lens), H, dh)
        out2 = torch.full_like(out, float("nan"))
        ops.attention_varlen_w_stream(qkv, out2, seg, lm, max(lens) + 200, H, dh)
        torch.cuda.synchronize()
    assert bool(torch.isnan(out[Rr:]).all()) and bool(torch.isnan(out2[Rr:]).all()), "rows behind the last segment were written"
    ref = R.attention_w_ref(qkv.double().cpu(), seg, torch.log(mult.double()), H)
    got = out[:Rr].double().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    per_seg = [float(err[a:b].max()) for a, b in zip(np.cumsum([0] + lens[:-1]), np.cumsum(lens))]
    print(f"\nattention_w_stream {mode}: max |err| {float(err.max()):.3g} (bound {_attn_bound(mode, qkv, H * dh):.3g}); per segment "
          + " ".join(f"{L}:{e:.2g}" for L, e in zip(lens, per_seg)))
    assert float(err.max()) <= _attn_bound(mode, qkv, H * dh)
    assert torch.equal(out[:Rr].view(torch.int16), out2[:Rr].view(torch.int16)), "a larger max_len changed the result"


@pytest.mark.parametrize("mode", MODES)
def test_attention_stream_equals_dense_attention_over_repeated_rows(mode):
    """A key of multiplicity n = that key physically n times in pv_attention_bf16's dense sequence; one segment has 300 packed rows."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    B, H, dh, S = 3, 2, 64, 577
    g = torch.Generator().manual_seed(17)
    lens, mults = [300, int(torch.randint(209, 400, (1,), generator=g)), 40], []
    for L in lens:
        cut = torch.sort(torch.randperm(S - 1, generator=g)[:L - 1] + 1).values.tolist()       # S split into L positive parts
        mults += [hi - lo for lo, hi in zip([0] + cut, cut + [S])]
    mult = torch.tensor(mults)
    seg = _seg(lens, dev)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv = _packed_qkv(lens, H, dh, 23, dt, dev)
        out = torch.empty((sum(lens), H * dh), dtype=dt, device=dev)
        ops.attention_varlen_w_stream(qkv, out, seg, torch.log(mult.float()).to(dev), max(lens), H, dh)
        rep = torch.repeat_interleave(torch.arange(sum(lens)), mult).to(dev)
        dense_in = qkv[rep].contiguous()
        assert dense_in.shape[0] == B * S
        dense = torch.empty((B * S, H * dh), dtype=dt, device=dev)
        ops.attention(dense_in, dense, B, S, H, dh)
        torch.cuda.synchronize()
    first = torch.cumsum(mult, 0) - mult                       # the first copy of every packed row
    a, d = out.double().cpu(), dense.double().cpu()[first]
    err = float((a - d).abs().max())
    print(f"\nattention_w_stream vs repeated rows {mode}: max |diff| {err:.3g}")
    assert err <= 2 * _attn_bound(mode, qkv, H * dh)             # (each side within the bound of the exact value)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [65, 209, 417])
def test_attention_stream_has_the_bits_of_the_streaming_forward(S, mode):
    """Equal segments, log_mult = 0: the kernel it extends (pv_attn_stream_kernel through ops.attention_stream), bit for bit."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    B, H, dh = 3, 2, 64
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv = _packed_qkv([S] * B, H, dh, S, dt, dev)
        out = torch.full((B * S, H * dh), float("nan"), dtype=dt, device=dev)
        ops.attention_varlen_w_stream(qkv, out, _seg([S] * B, dev), torch.zeros(B * S, device=dev), S, H, dh)
        want = torch.full_like(out, float("nan"))
        lse = torch.empty((B, H, S), dtype=torch.float32, device=dev)
        ops.attention_stream(qkv, want, lse, B, S, H, dh)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


def test_attention_stream_refuses_what_it_does_not_take():
    from peekvit_amd import _lib, ops
    dev = _dev()
    lib = _lib.load("bf16")
    qkv = torch.zeros((5, 3 * 64), dtype=torch.bfloat16, device=dev)
    out = torch.full((4, 64), 7.0, dtype=torch.bfloat16, device=dev)
    seg = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    lm = torch.zeros(4, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    s = C.c_void_p(ops.raw_stream(0))
    f = lib.pv_attention_varlen_w_stream_bf16
    assert f(p(qkv), p(out), p(seg), p(lm), 1, 4, 2, 32, None, s) == -2           # PV_ERR_UNSUPPORTED: head dim
    assert f(p(qkv), p(out), p(seg), p(lm), 1, 4, 1, 128, None, s) == -2
    assert f(p(qkv), p(out), p(seg), p(lm), 1, 4097, 1, 64, None, s) == -2        # max_len
    assert f(p(qkv), p(out), p(seg), p(lm), 1 << 29, 4096, 1, 64, None, s) == -2  # grid above 2^31 - 1
    for args in ((None, p(out), p(seg), p(lm)), (p(qkv), None, p(seg), p(lm)), (p(qkv), p(out), None, p(lm)), (p(qkv), p(out), p(seg), None)):
        assert f(*args, 1, 4, 1, 64, None, s) == -1                               # PV_ERR_INVALID_ARG: null
    assert f(p(qkv), p(out), p(seg), p(lm), 0, 4, 1, 64, None, s) == -1 and f(p(qkv), p(out), p(seg), p(lm), 1, 0, 1, 64, None, s) == -1
    assert f(p(qkv), p(out), p(seg), p(lm), 1, 4, 0, 64, None, s) == -1
    assert f(p(qkv, 2), p(out), p(seg), p(lm), 1, 4, 1, 64, None, s) == -1        # misaligned qkv (16 bytes), out (8), tables (4)
    assert f(p(qkv), p(out, 2), p(seg), p(lm), 1, 4, 1, 64, None, s) == -1
    assert f(p(qkv), p(out), p(seg, 2), p(lm), 1, 4, 1, 64, None, s) == -1 and f(p(qkv), p(out), p(seg), p(lm, 2), 1, 4, 1, 64, None, s) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                       # nothing was launched
    assert f(p(qkv), p(out), p(seg), p(lm), 1, 4, 1, 64, None, s) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())                       # (the accepted call does write: v = 0)


# ---- chunked gate + compaction step --------------------------------------------------------------------------------------------
def _pack_inputs_lens(lens, N, D, seed, gain=3.0, min_margin=1e-4):
    """test_hip_residual_sparse._pack_inputs with the segment lengths given: segments of lens[b] rows (2 .. N + 2), every middle row standing for
    one or more of the image's N tokens.  Built on the CPU; rows whose gate margin |sigmoid - thr| is under 10 * min_margin in the fp64 reference
    are redrawn until none is left, so every margin of the reference is >= 1e-4 with room to spare and nothing is left out of the comparison."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Rr = int(seg[-1])
    tok_row = np.zeros((B, N), dtype=np.int64)
    mult = np.ones(Rr, dtype=np.int64)
    for b in range(B):
        k = lens[b] - 2
        assert 0 <= k <= N
        if k == 0:
            continue                # (no middle row: such an image's tokens are not looked up by the model; the kernels clamp)
        rows = torch.cat([torch.arange(k), torch.randint(0, k, (N - k,), generator=g)])[torch.randperm(N, generator=g)] + 1
        tok_row[b] = rows.numpy()
        mult[seg[b] + 1:seg[b] + 1 + k] = np.bincount(rows.numpy() - 1, minlength=k)
    x = torch.randn(Rr, D, generator=g)
    wg = torch.randn(D, generator=g) * gain / D ** 0.5
    wb = torch.randn(D, generator=g) / D ** 0.5
    bg, bb = 0.05, -0.02
    for _ in range(50):
        margin = R.pack_step_ref(x.double(), seg, mult, tok_row, wg.double(), bg, wb.double(), bb, 1.0, 0.0)["margin"]
        bad = torch.nonzero(margin < 10 * min_margin).reshape(-1)
        if bad.numel() == 0:
            break
        x[bad] = torch.randn(bad.numel(), D, generator=g)
    else:
        raise AssertionError("rejection sampling did not converge")
    assert float(margin.min()) >= min_margin
    return x, seg, mult, tok_row, wg, bg, wb, bb


def _run_long(monkeypatch, *args, **kw):
    """test_hip_residual_sparse._run_pack_step with the long entry point in the wrapper's place (the same buffers, pre-fills and call)."""
    from peekvit_amd import ops
    with monkeypatch.context() as mp:
        mp.setattr(ops, "residual_pack_step", ops.residual_pack_step_long)
        return _run_pack_step(*args, **kw)


PACK_CASES = {"chunk_edges": ([2, 3, 255, 256, 257, 258, 511, 512, 513, 769, 1025, 1026], 1024, 128),
              "just_past_resident": ([211, 2, 150], 209, 256),
              "longest": ([4096, 2049], 4094, 128)}


@pytest.mark.parametrize("with_ln", [True, False])
@pytest.mark.parametrize("case", sorted(PACK_CASES))
def test_pack_step_long_against_the_restatement(monkeypatch, case, with_ln):
    """Integer tables and totals exactly, float outputs within test_hip_residual_sparse._check_pack_step's tolerances, with and without ln_out."""
    from peekvit_amd import engine
    dev = _dev()
    lens, N, D = PACK_CASES[case]
    B = len(lens)
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_inputs_lens(lens, N, D, 7 * B + N)
    g = torch.Generator().manual_seed(1)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    xd = x.to(dev).double()
    ref = R.pack_step_ref(xd, seg, mult, tok_row, wg.to(dev), bg, wb.to(dev), bb, 1.0, 0.0)
    Rn, longest = ref["totals"]
    u32 = 2.0 ** -24
    depth = D / 256 + 7                                   # (the error model of the wave's dot product: see _check_pack_step)
    img = torch.from_numpy(np.repeat(np.arange(B), np.diff(seg))).to(dev)
    tol_thr = 0.25 * depth * u32 * (xd[torch.from_numpy(seg[1:] - 1).to(dev)].abs() @ wb.to(dev).double().abs()) + 8 * u32
    tol_row = 0.25 * depth * u32 * (xd.abs() @ wg.to(dev).double().abs()) + 8 * u32 + tol_thr[img]
    tok_abs = torch.from_numpy(seg[:-1, None] + tok_row).to(dev)
    has_mid = np.diff(seg) > 2
    hm = torch.from_numpy(has_mid).to(dev)
    for mode in MODES:
        with engine.precision(mode):
            nxt, mask, thr, totals, h = _run_long(monkeypatch, x, seg, mult, tok_row, wg, bg, wb, bb, dev, ln=(gamma, beta, 1e-6) if with_ln else None)
        assert totals.tolist() == [Rn, longest]
        assert np.array_equal(nxt[4].cpu().numpy(), ref["seg_next"])
        assert np.array_equal(nxt[2][:Rn].cpu().numpy(), ref["mult_next"])
        assert np.array_equal(nxt[5].cpu().numpy()[has_mid], ref["tok_row_next"][has_mid])
        assert int(ref["mult_next"].sum()) == int(mult.sum())                     # no token is lost or counted twice
        assert bool(((thr.double() - ref["thr_out"]).abs() <= tol_thr).all())
        dm = (mask.double() - ref["mask_out"]).abs()
        assert bool((dm <= tol_row[tok_abs])[hm].all()), f"mask error {float(dm[hm].max()):.3g}"
        assert bool(((mask == 0) == (ref["mask_out"] == 0))[hm].all())
        rs_err = (nxt[1][:Rn].double() - ref["row_scale_next"]).abs()
        assert float(rs_err.max()) <= float(tol_row.max())
        lm64 = torch.log(nxt[2][:Rn].double())
        assert bool(((nxt[3][:Rn].double() - lm64).abs() <= 2.0 ** -21 * lm64).all())
        zero = ref["row_scale_next"] == 0
        assert bool((nxt[0][:Rn][zero] == 0).all()) and bool((nxt[1][:Rn][zero] == 0).all())
        scale_tol = float(tol_row.max())
        xe = (nxt[0][:Rn].double() - ref["x_next"]).abs()
        assert bool((xe <= scale_tol * float(xd.abs().max()) + 2 * u32 * ref["x_next"].abs()).all()), f"x_next error {float(xe.max()):.3g}"
        assert bool(torch.isnan(nxt[0][Rn:]).all()) and bool((nxt[2][Rn:] == -7).all()), "rows behind R' were written"
        if with_ln:
            ln_ref = ref["row_scale_next"][:, None] * torch.nn.functional.layer_norm(ref["x_next"], (D,), gamma.to(dev).double(), beta.to(dev).double(), 1e-6)
            he = (h[:Rn].double() - ln_ref).abs()
            assert bool((he <= U16[mode] * ln_ref.abs() + 8.0 * scale_tol + 1e-5).all()), f"ln_out error {float(he.max()):.3g}"
            assert bool((h[:Rn][zero] == 0).all())
    print(f"\npack step long {case}: {int(seg[-1])} rows in, {Rn} out, longest next segment {longest}")
    assert Rn < int(seg[-1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N,D", [(7, 5, 256), (5, 206, 768)])
def test_pack_step_long_has_the_bits_of_the_resident_step(monkeypatch, B, N, D, mode):
    from peekvit_amd import engine
    dev = _dev()
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_inputs(B, N, D, 7 * B + N)
    g = torch.Generator().manual_seed(1)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.05 * torch.randn(D, generator=g)
    bits = lambda t: t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])
    for ln in ((gamma, beta, 1e-6), None):
        with engine.precision(mode):
            a = _run_pack_step(x, seg, mult, tok_row, wg, bg, wb, bb, dev, ln=ln)
            b = _run_long(monkeypatch, x, seg, mult, tok_row, wg, bg, wb, bb, dev, ln=ln)
        (nxt_a, mask_a, thr_a, tot_a, h_a), (nxt_b, mask_b, thr_b, tot_b, h_b) = a, b
        assert tot_a.tolist() == tot_b.tolist() and tot_a[0] > 0
        # whole buffers, the untouched pre-filled tails included: the long step writes exactly what the resident step writes
        for name, ta, tb in [("x_next", nxt_a[0], nxt_b[0]), ("row_scale_next", nxt_a[1], nxt_b[1]), ("mult_next", nxt_a[2], nxt_b[2]),
                             ("log_mult_next", nxt_a[3], nxt_b[3]), ("seg_next", nxt_a[4], nxt_b[4]), ("tok_row_next", nxt_a[5], nxt_b[5]),
                             ("mask_out", mask_a, mask_b), ("thr_out", thr_a, thr_b)] + ([("ln_out", h_a, h_b)] if ln is not None else []):
            assert torch.equal(bits(ta), bits(tb)), name


def test_pack_step_long_refuses_more_rows_than_it_holds(monkeypatch):
    from peekvit_amd import _lib
    dev = _dev()
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_inputs(2, 4, 128, 1)
    ok = np.zeros((2, 4094), dtype=np.int64)
    _run_long(monkeypatch, x, seg, mult, ok, wg, bg, wb, bb, dev)                                                # N + 2 = 4096
    with pytest.raises(_lib.PeekvitHipError):
        _run_long(monkeypatch, x, seg, mult, np.zeros((2, 4095), dtype=np.int64), wg, bg, wb, bb, dev)           # N + 2 = 4097


# ---- model ---------------------------------------------------------------------------------------------------------------------
def _long_model(size, dev):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    cfg = dict(META["dims"], image_size=size)
    scfg = dict(cfg, **META["kwargs"])
    m = ResidualVisionTransformer(**scfg)
    sd = synth.residual_sparse_state_dict(scfg, gate_gain=META["gate_gain"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return scfg, m.eval().to(dev)


def _left(m):
    masks = torch.stack([blk.mask.cpu() for blk in m.encoder.layers]).numpy()
    thr = torch.stack([blk.residual_gate.threshold.cpu() for blk in m.encoder.layers])
    return masks, thr.view(len(m.encoder.layers), -1).numpy()


def _record_attention(monkeypatch):
    """(kernel, max_len) of every ragged attention launch, in order."""
    from peekvit_amd import ops
    calls = []
    for name in ("attention_varlen_w", "attention_varlen_w_stream"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name: (calls.append((_name, a[4])), _real(*a))[1])
    return calls


@pytest.mark.parametrize("size", META["sizes"])
def test_model_parity_on_the_long_sparse_fixture(golden, monkeypatch, size):
    """Mode `auto`, compaction on, against the real reference at 227 rows (120 px) and 402 rows (160 px).

    The packed path must have produced the answer; every layer's attention is the streaming kernel exactly when the longest segment the host read
    for it exceeds 208 rows, and `engine.sparse_long_layers` grows by the number of such layers.  (At 120 px the gates leave at most ~135 rows per
    image behind the first pack step - scripts/make_golden_residual_sparse_long.py prints the rows per layer - so there that number is 0 by the
    fixture's own data: the long PACK STEP runs in every layer, the attention stays resident.  At 160 px the count must be positive.)"""
    from peekvit_amd import engine, ops
    dev = _dev()
    g = golden("residualvit_sparse_long")
    cfg, m = _long_model(size, dev)
    _, dense = _long_model(size, dev)
    m.set_token_compaction(True)
    x = torch.from_numpy(synth.synth_images(META["batch"], size, seed=0)).to(dev)
    L, S = cfg["num_layers"], synth.seq_length(cfg) + 1
    assert S == META["size"][str(size)]["rows"] > RESIDENT
    calls = _record_attention(monkeypatch)
    steps = []
    real_long = ops.residual_pack_step_long
    monkeypatch.setattr(ops, "residual_pack_step_long", lambda *a, **k: (steps.append(1), real_long(*a, **k))[1])
    for b in META["budgets"]:
        key = f"s{size}_b{b}_"
        m.set_budget(b)
        dense.set_budget(b)
        _forward(dense, x)
        dmasks, dthr = _left(dense)
        merr_d = float(np.abs(dmasks - g[key + "masks"]).max())
        terr_d = float(np.abs(dthr - g[key + "thresholds"]).max())
        del calls[:], steps[:]
        r0, d0, s0, f0 = _counters()
        n0 = engine.sparse_long_layers
        logits = _forward(m, x).cpu().numpy()
        r1, d1, s1, f1 = _counters()
        n1 = engine.sparse_long_layers
        assert engine.last_forward_guarded() and r1 > r0 and f1 == f0, "the packed path did not produce the answer"
        assert len(steps) >= L and len(steps) % L == 0, "the long pack step did not run in every layer"
        longest = engine.sparse_last_max_len
        assert len(longest) == L == len(engine.sparse_last_rows) and len(calls) >= L
        for i, (name, max_len) in enumerate(calls[-L:]):
            assert max_len == longest[i] and 2 <= max_len <= S
            assert (name == "attention_varlen_w_stream") == (max_len > RESIDENT), f"layer {i}: {name} at longest segment {max_len}"
        streamed = sum(name == "attention_varlen_w_stream" for name, _ in calls)
        assert n1 - n0 == streamed and streamed == sum(ml > RESIDENT for _, ml in calls)
        if size == 160:
            assert n1 > n0, "no layer ran the streaming kernel at 402 rows per image"
        masks, thr = _left(m)
        assert thr.shape == (L, META["batch"]) and bool(((thr > 0) & (thr < 1)).all())
        err = rel_l2(logits, g[key + "logits"])
        merr = float(np.abs(masks - g[key + "masks"]).max())
        terr = float(np.abs(thr - g[key + "thresholds"]).max())
        share = sum(engine.sparse_last_rows) / float(L * META["batch"] * S)
        sure = g[key + "margin"] >= META["margin"]
        flips = int(((masks[..., 0] == 0) != (g[key + "masks"][..., 0] == 0))[sure].sum())
        print(f"\n{size} px budget {b}: logits {err:.3g}, masks {merr:.3g} (dense HIP forward {merr_d:.3g}), thresholds {terr:.3g} (dense {terr_d:.3g}), "
              f"rows share {share:.3f} (fp64 {float(g[key + 'rows_share']):.3f}), longest segments {longest}, streamed layers {n1 - n0}, "
              f"state flips among sure tokens {flips}, left out {1 - sure.mean():.4f}")
        assert err < TOL_CONTRACT
        # the project's bounds; where the parent's dense HIP forward itself exceeds one on this model, 1.5 x its measured error instead
        assert merr < (2e-3 if merr_d < 2e-3 else 1.5 * merr_d)
        assert terr < (5e-3 if terr_d < 5e-3 else 1.5 * terr_d)
        assert 1 - sure.mean() <= META["max_excluded_fraction"]
        assert flips == 0, "a token with a gate margin of 5e-3 or more is collapsed / live where the reference has it live / collapsed"
        assert abs(share - float(g[key + "rows_share"])) <= L * (1 - sure.mean()) + 1e-9
        assert s1 - s0 >= L


CASES_DENSE = [(160, 1, 0.2), (160, 3, 0.8), (160, 5, 0.2), (160, 5, 0.8), (160, 1, 0.8), (160, 3, 0.2), (224, 2, 0.5)]


def test_packed_forward_against_the_models_own_dense_forward():
    """Mode `f16` (nothing can answer but the packed kernels): 402 rows at batches 1, 3, 5 and budgets 0.2 / 0.8, 786 rows at batch 2."""
    from peekvit_amd import engine
    dev = _dev()
    models = {}
    for size, n, b in CASES_DENSE:
        if size not in models:
            models[size] = (_long_model(size, dev)[1], _long_model(size, dev)[1])
        never, m = models[size]
        cfg = dict(META["dims"], image_size=size)
        L, S = cfg["num_layers"], synth.seq_length(cfg) + 1
        x = torch.from_numpy(synth.synth_images(n, size, seed=n)).to(dev)
        never.set_budget(b)
        m.set_budget(b)
        dense = _forward(never, x, "f16")
        dmask = torch.stack([blk.mask for blk in never.encoder.layers])
        m.set_token_compaction(True)
        r0, d0, s0, f0 = _counters()
        n0 = engine.sparse_long_layers
        packed = _forward(m, x, "f16")
        r1, d1, s1, f1 = _counters()
        assert r1 > r0 and f1 == f0 and s1 - s0 == L and d1 - d0 == L * n * S, "the packed path did not run"
        assert r1 - r0 < d1 - d0, "tokens are masked and no row was saved"
        assert engine.sparse_long_layers - n0 == sum(ml > RESIDENT for ml in engine.sparse_last_max_len) > 0
        pmask = torch.stack([blk.mask for blk in m.encoder.layers])
        assert packed.shape == dense.shape and pmask.shape == dmask.shape == (L, n, S - 2, 1)
        e, me = rel_l2(packed, dense), float((pmask - dmask).abs().max())
        print(f"\n{size} px batch {n} budget {b}: logits {e:.3g}, masks {me:.3g}, rows {r1 - r0} of {d1 - d0}, longest segments {engine.sparse_last_max_len}")
        # both are fp16-operand forwards of the same model: each within the contract of the fp32 reference, so within twice that of each other
        assert e < 2 * TOL_CONTRACT, (size, n, b)
        assert me < 4e-3
        m.set_token_compaction(False)
        r0 = engine.sparse_rows
        off = _forward(m, x, "f16")
        assert engine.sparse_rows == r0
        assert torch.equal(off, dense), "compaction off is not the dense forward bit for bit"
        assert torch.equal(torch.stack([blk.mask for blk in m.encoder.layers]), dmask)


def test_graphed_forward_still_raises():
    from peekvit_amd import _lib
    from peekvit_amd.graph import GraphedForward
    dev = _dev()
    cfg, m = _long_model(160, dev)
    m.set_budget(0.5)
    m.set_token_compaction(True)
    x = torch.from_numpy(synth.synth_images(2, 160, seed=0)).to(dev)
    with pytest.raises(_lib.PeekvitHipError, match="token compaction"):
        GraphedForward(m, x)
