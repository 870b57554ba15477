"""ResidualViT training on the packed rows past 208 rows per image, on the GPU (include/peekvit_hip_sparse_long_train.h), in
both operand libraries: the streaming ragged attention pair against fp64, the weighted key the resident kernel's test would miss, continuity with the
resident pair up to 208 rows, the chunked pack step for training and its backward against fp64 autograd, and one training step of the model.

Every output has trailing rows that belong to no segment, filled with NaN, which must still be NaN afterwards."""
import math
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_l2
from peekvit_amd import ops
import residual_sparse_train_ref as T
import test_residual_sparse_long_train_host as long_host
import test_residual_sparse_train_host as host
from test_hip_attn_stream import CAP
from test_hip_residual_sparse_train import (DEV, EXTRA_ROWS, IMAGES, KNEE, LAYOUTS, MODES, TRAIN_MODES, WEIGHTS, H, DH, D, _attn_inputs, _complete, _gpu_model,
                                            _gpu_step, _guarded, _margins, _pack_case, _ref_step, _restated_ragged, _same_grads, _untouched)

pytestmark = pytest.mark.gpu
RESIDENT = 208
SEGMENTS = [1, 2, 63, 64, 65, 127, 128, 129, 208, 209, 257, 402, 417, 1025]          # section 33's: every edge of the 64-key block, both sides of 208 and 256


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the streaming ragged attention pair
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_pair(qkv, dout, seg, lm, lens, dt, max_len=None, fwd=None, bwd=None, forward=None):
    """One forward + backward with guarded outputs: (out, lse, g16, part, delta).  `forward`: (out, lse) of another forward, for the backward alone."""
    fwd, bwd = fwd or ops.attention_varlen_w_stream_lse, bwd or ops.attention_varlen_w_stream_bwd16
    Rr, B = sum(lens), len(lens)
    max_len = max_len or max(lens)
    nb = (max_len + 63) // 64
    out, lse, g16 = _guarded(Rr, D, dt), _guarded(Rr, H), _guarded(Rr, 3 * D, dt)
    part, delta = _guarded(B * nb, 3 * D), _guarded(Rr, H)
    n0 = ops.launch_count
    if forward is None:
        fwd(qkv, out, lse, seg, lm, max_len, H, DH)
    else:
        out[:Rr], lse[:Rr] = forward
        n0 -= 1
    bwd(qkv, dout, out, lse, seg, lm, g16, max_len, H, DH, DH ** -0.5, dbias_partial=part[:B * nb], delta_ws=delta)
    assert ops.launch_count - n0 == 2
    torch.cuda.synchronize()
    assert all(_untouched(f, n) for f, n in ((out, Rr), (lse, Rr), (g16, Rr), (part, B * nb), (delta, Rr)))
    return out[:Rr], lse[:Rr], g16[:Rr], part[:B * nb], delta[:Rr]


def _backward_errors(g16, restated, ref_g):
    return {name: (rel_l2(g16[:, i * D:(i + 1) * D].float(), ref_g[:, i * D:(i + 1) * D]), rel_l2(restated[:, i * D:(i + 1) * D], ref_g[:, i * D:(i + 1) * D]))
            for i, name in enumerate("qkv")}


def _check_backward(errs, mode, what):
    for name, (err, base) in errs.items():
        print(f"{what} d{name}: rel L2 {err:.3g} (restated on stock ops {base:.3g})")
    for name, (err, base) in errs.items():
        assert err <= 2.0 * base + 1e-5, (what, name, err, base)
        assert err < CAP[mode], (what, name, err)


def _check_bias_partials(part, g16, seg, lens, nb):
    """Per (image, 64-row block) the column sums of the STORED values; a block beyond its segment holds zeros."""
    v, p, segn = g16.double().cpu(), part.double().cpu(), seg.cpu().numpy()
    for b, n in enumerate(lens):
        for blk in range(nb):
            lo, hi = int(segn[b]) + min(blk * 64, n), int(segn[b]) + min(blk * 64 + 64, n)
            want, mag = v[lo:hi].sum(0), v[lo:hi].abs().sum(0)
            assert ((p[b * nb + blk] - want).abs() <= 64 * 2.0 ** -24 * mag).all(), (b, blk)


def _dominant_share(q64, lm64, seg, lens):
    """The smallest probability the dominant key of _attn_inputs holds in any row."""
    worst, segn = 1.0, seg.cpu().numpy()
    for b, n in enumerate(lens):
        s0, j = int(segn[b]), (n * 2) // 3
        qh, kh = (q64[s0:s0 + n, i * D:(i + 1) * D].reshape(n, H, DH).transpose(0, 1) for i in range(2))
        p = torch.softmax(qh @ kh.transpose(-1, -2) + lm64[s0:s0 + n], dim=-1)
        worst = min(worst, float(p[..., j].min()))
    return worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_streaming_ragged_attention_pair_against_fp64(weights, mode):
    """One call over segments of 1 .. 1025 rows.  Bounds: the resident pair's (tests/test_hip_residual_sparse_train.py) - forward |lse| 1e-4 and out
    6e-3; backward twice the stock-op restatement with the kernels' rounding points + 1e-5, and CAP; bias partials 64 * 2^-24 of the summed
    magnitudes."""
    from peekvit_amd import _lib, engine
    lens = SEGMENTS
    Rr = sum(lens)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout, seg, lm = _attn_inputs(lens, weights, dt, seed=35 + WEIGHTS.index(weights))
        out, lse, g16, part, delta = res = _run_pair(qkv, dout, seg, lm, lens, dt)
        again = _run_pair(qkv, dout, seg, lm, lens, dt)
        assert all(torch.equal(a, b) for a, b in zip(again, res))                                   # two runs: identical bits
        # the forward shares the inference kernel's body: the same `out`, bit for bit
        inf = torch.empty((Rr, D), dtype=dt, device=DEV)
        ops.attention_varlen_w_stream(qkv[:Rr], inf, seg, lm[:Rr], max(lens), H, DH)
        assert torch.equal(inf, out)
        # a larger bound changes no bit: more (empty) blocks per image, zero partial rows for them
        wide = _run_pair(qkv, dout, seg, lm, lens, dt, max_len=1100)
        assert all(torch.equal(a, b) for a, b in zip((wide[0], wide[1], wide[2], wide[4]), (out, lse, g16, delta)))
        nb, nbw = (max(lens) + 63) // 64, (1100 + 63) // 64
        pw = wide[3].view(len(lens), nbw, 3 * D)
        assert nbw > nb and torch.equal(pw[:, :nb], part.view(len(lens), nb, 3 * D)) and bool((pw[:, nb:] == 0).all())
        q64, lm64 = qkv[:Rr].double().cpu(), lm[:Rr].double().cpu()
        ref_out, ref_lse = T.attention_w_train_ref(q64, seg.cpu(), lm64, H)
        ref_g, _ = T.attention_w_backward_ref(q64, dout[:Rr].cpu(), seg.cpu(), lm64, H, DH ** -0.5)
        if weights == "dominant":
            assert _dominant_share(q64, lm64, seg, lens) >= 0.99                                    # the case's own precondition
        e_lse, e_out = float((lse.double().cpu() - ref_lse).abs().max()), rel_l2(out.float(), ref_out)
        print(f"\nstreaming ragged forward {weights} {mode}: |lse - fp64| max {e_lse:.3g}, out rel L2 {e_out:.3g}")
        assert e_lse < 1e-4
        assert e_out < 6e-3
        restated = _restated_ragged(qkv[:Rr], dout[:Rr], out, seg, lm[:Rr], dt)
        _check_backward(_backward_errors(g16, restated, ref_g), mode, f"streaming ragged backward {weights} {mode}")
        _check_bias_partials(part, g16, seg, lens, nb)


@pytest.mark.parametrize("mode", MODES)
def test_a_weighted_key_beyond_row_255_is_seen(mode):
    """The resident dQ kernel asks one thread per key whether a segment carries a weight: 256 keys.  A 402-row segment whose only weight sits at row
    300 and a 1025-row one with its only weight at row 1024 must get delta = sum_k p dP (fp64 reference; the backward's bound: twice the fp32
    restatement + 1e-5, and CAP); the unweighted 300-row segment between them keeps delta = sum_d dO O of the stored output (fp32 sum of 64
    products: 64 * 2^-24 of the summed magnitudes)."""
    from peekvit_amd import _lib, engine
    lens = [402, 300, 1025]
    Rr = sum(lens)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout, seg, lm = _attn_inputs(lens, "none", dt, seed=7)
        lm[300] = math.log(150.0)
        lm[402 + 300 + 1024] = math.log(2.0)
        out, lse, g16, part, delta = _run_pair(qkv, dout, seg, lm, lens, dt)
        q64, lm64 = qkv[:Rr].double().cpu(), lm[:Rr].double().cpu()
        _, ref_delta = T.attention_w_backward_ref(q64, dout[:Rr].cpu(), seg.cpu(), lm64, H, DH ** -0.5)
        ref_delta = ref_delta.reshape(Rr, H)
        segn = seg.cpu().numpy()
        stored = (dout[:Rr].float() * out.float()).view(Rr, H, DH)
        for b, n in enumerate(lens):
            sl = slice(int(segn[b]), int(segn[b + 1]))
            got = delta[sl].double().cpu()
            if b == 1:
                want, mag = stored[sl].sum(-1).double().cpu(), stored[sl].abs().sum(-1).double().cpu()
                assert bool(((got - want).abs() <= 64 * 2.0 ** -24 * mag + 1e-30).all())
                continue
            # sum_k p dP on stock ops in fp32, the kernel's formula
            q, k, v = (qkv[sl, i * D:(i + 1) * D].float().reshape(n, H, DH).transpose(0, 1) for i in range(3))
            do = dout[sl].float().reshape(n, H, DH).transpose(0, 1)
            P = torch.softmax(q @ k.transpose(-1, -2) + lm[sl], dim=-1)
            restated = (P * (do @ v.transpose(-1, -2))).sum(-1).transpose(0, 1).double().cpu()
            err, base = rel_l2(got, ref_delta[sl]), rel_l2(restated, ref_delta[sl])
            from_stored = rel_l2(stored[sl].sum(-1).double().cpu(), ref_delta[sl])
            print(f"\nsegment of {n} rows {mode}: delta rel L2 {err:.3g} (fp32 restatement {base:.3g}; from the stored output it would be {from_stored:.3g})")
            assert err <= 2.0 * base + 1e-5 and err < CAP[mode], (n, err, base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_up_to_208_rows_the_streaming_pair_continues_the_resident_one(layout, weights, mode):
    """Every segment <= 208: on the resident forward's results the streaming backward has the resident backward's bits in all of its outputs; the
    two forwards' lse agree to 1e-4 (they sum in different orders); and either forward under the other backward stays inside the pair's bounds."""
    from peekvit_amd import _lib, engine
    lens = LAYOUTS[layout]
    Rr = sum(lens)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout, seg, lm = _attn_inputs(lens, weights, dt, seed=len(layout) + WEIGHTS.index(weights))
        res = _run_pair(qkv, dout, seg, lm, lens, dt, fwd=ops.attention_varlen_w_lse, bwd=ops.attention_varlen_w_bwd16)
        stream = _run_pair(qkv, dout, seg, lm, lens, dt)
        # the resident forward under the streaming backward / the streaming forward under the resident backward
        cross_a = _run_pair(qkv, dout, seg, lm, lens, dt, forward=res[:2])
        cross_b = _run_pair(qkv, dout, seg, lm, lens, dt, bwd=ops.attention_varlen_w_bwd16, forward=stream[:2])
        for k, p, q in zip(("dqkv16", "dbias_partial", "delta_ws"), cross_a[2:], res[2:]):
            assert torch.equal(p, q), k                                                             # bit for bit
        e = float((stream[1] - res[1]).abs().max())
        print(f"\n{layout} {weights} {mode}: |lse streaming - lse resident| max {e:.3g}")
        assert e < 1e-4
        q64, lm64 = qkv[:Rr].double().cpu(), lm[:Rr].double().cpu()
        ref_g, _ = T.attention_w_backward_ref(q64, dout[:Rr].cpu(), seg.cpu(), lm64, H, DH ** -0.5)
        for tag, got in (("resident forward + streaming backward", cross_a), ("streaming forward + resident backward", cross_b),
                         ("streaming forward + streaming backward", stream)):
            restated = _restated_ragged(qkv[:Rr], dout[:Rr], got[0], seg, lm[:Rr], dt)
            _check_backward(_backward_errors(got[2], restated, ref_g), mode, f"{tag} {layout} {weights} {mode}")
            _check_bias_partials(got[3], got[2], seg, lens, (max(lens) + 63) // 64)


def test_entry_points_refuse_bad_arguments():
    long_host.check_argument_validation()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the chunked pack step for training and its backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _long_pack_case(lens, N, Dm, seed, multi, all_live=None, all_dead=None):
    """A packed input of len(lens) images of lens[b] rows that stand for N tokens each.  multi: {image: [(row of the segment, live), ...]} - the rows
    that take the image's surplus tokens (multiplicity > 1); every other row between class and budget row stands for one token.  Image `all_live`
    masks nothing, image `all_dead` everything, the others a random 40 %.  The gate reads (almost only) coordinate 0, well away from the threshold
    on either side, as test_hip_residual_sparse_train._pack_case builds it; the token -> row table is a random permutation."""
    g = torch.Generator().manual_seed(seed)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Rr, B = int(seg[-1]), len(lens)
    x = torch.randn(Rr, Dm, generator=g)
    wg = torch.randn(Dm, generator=g) * 0.02
    wg[0] = 2.0
    wb = torch.randn(Dm, generator=g) * 0.02
    bg, bb = torch.tensor([0.1]), torch.tensor([-0.2])
    mult = np.ones(Rr, dtype=np.int64)
    tok_row = np.zeros((B, N), dtype=np.int64)
    for b, L in enumerate(lens):
        mid = L - 2
        if mid == 0:
            continue                                  # (no token row at all: the table points at the class row, whose mask is the constant 1)
        mu = np.ones(mid, dtype=np.int64)
        live = (torch.rand(mid, generator=g) < 0.6).numpy()
        fixed = b in (all_live, all_dead)
        if fixed:
            live[:] = b == all_live
        spots = multi.get(b, [(mid, True)])
        surplus = N - mid
        assert surplus >= 0 and (surplus == 0 or spots)
        for k, (r, lv) in enumerate(spots):
            share = surplus // len(spots) + (surplus % len(spots) if k == 0 else 0)
            mu[r - 1] += share
            if surplus and not fixed:
                live[r - 1] = lv
        assert int(mu.sum()) == N
        rows = np.repeat(np.arange(1, mid + 1), mu)
        s0 = int(seg[b])
        mult[s0 + 1:s0 + 1 + mid] = mu
        sign = torch.from_numpy(np.where(live, 1.0, -1.0)).float()
        x[s0 + 1:s0 + 1 + mid, 0] = (1.5 + 0.5 * torch.rand(mid, generator=g)) * sign
        tok_row[b, torch.randperm(N, generator=g).numpy()] = rows
    return x, seg, mult, tok_row, wg, bg, wb, bb


PACK_CASES = {
    # name -> (segment lengths, N, D, rows of multiplicity > 1 per image, the image that masks nothing, the image that masks everything)
    "n1024": ([2, 3, 255, 256, 257, 258, 511, 512, 513, 769, 1025, 1026], 1024, 128,
              {2: [(100, True), (250, False)], 3: [(254, True)], 4: [(255, False)], 5: [(256, True)], 6: [(300, True), (509, False)], 7: [(257, False), (510, True)],
               8: [(400, True)], 9: [(300, True), (600, False), (767, True)], 10: [(600, True)]}, 11, 3),
    "n209": ([211, 2, 150], 209, 256, {2: [(7, True), (148, False)]}, 0, None),
    "n4094": ([4096, 2049], 4094, 128, {1: [(300, True), (700, True), (1500, False), (2047, True)]}, 0, None),
}


def _alloc_step(Rr, B, N, Dm):
    x_next, rs_next, lm_next = _guarded(Rr, Dm), _guarded(Rr, 1), _guarded(Rr, 1)
    mult_next, src_next = torch.full((Rr,), -7, dtype=torch.int32, device=DEV), torch.full((Rr,), -7, dtype=torch.int32, device=DEV)
    seg_next, tok_next = torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV)
    mask_out, thr_out, totals = torch.empty((B, N), device=DEV), torch.empty(B, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    mask_row, gate_arg = torch.empty(Rr, device=DEV), torch.empty(Rr, device=DEV)
    return dict(x_next=x_next, rs_next=rs_next, lm_next=lm_next, mult_next=mult_next, src_next=src_next, seg_next=seg_next, tok_next=tok_next,
                mask_out=mask_out, thr_out=thr_out, totals=totals, mask_row=mask_row, gate_arg=gate_arg)


def _train_step(op, dev_in, a):
    op(*dev_in, 1.0, 0.0, (a["x_next"], a["rs_next"].view(-1), a["mult_next"], a["lm_next"].view(-1), a["seg_next"], a["tok_next"]), a["mask_out"],
       a["thr_out"], a["totals"], a["mask_row"], a["gate_arg"], a["src_next"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(PACK_CASES))
def test_pack_step_long_train_and_its_backward_against_fp64_autograd(case, mode):
    """tests/test_hip_residual_sparse_train.py's pack-step test past 208 rows.  Forward: every result shared with the inference entry is bit-equal to
    it, the integer tables and src_next are exact against the restatement, sigmoid(gate_arg) within 1e-6.  Backward against fp64 autograd: rows
    that only move are exact; every reduced quantity gets twice the error of the same formula in stock fp32 ops + one fp32 ulp of its scale."""
    from peekvit_amd import engine
    lens, N, Dm, multi, all_live, all_dead = PACK_CASES[case]
    x, seg, mult, tok_row, wg, bg, wb, bb = _long_pack_case(lens, N, Dm, seed=N + Dm, multi=multi, all_live=all_live, all_dead=all_dead)
    Rr, B = x.shape[0], len(lens)
    gen = torch.Generator().manual_seed(N + 1)
    G, drs, dmask = torch.randn(Rr, Dm, generator=gen), torch.randn(Rr, generator=gen), torch.randn(B, N, generator=gen)
    ref, gref = _ref_step(x, seg, mult, tok_row, wg, bg, wb, bb, G, drs, dmask, torch.float64)
    _, g32 = _ref_step(x, seg, mult, tok_row, wg, bg, wb, bb, G, drs, dmask, torch.float32)
    Rn = ref["x_next"].shape[0]
    # the case's own preconditions
    assert float(ref["margin"][torch.isfinite(ref["margin"])].min()) >= 1e-3
    live_rows = (ref["mask_row"].detach() > 0).numpy()
    spots = [(b, r, lv) for b, sp in multi.items() if b != all_dead for r, lv in sp]
    assert all(int(mult[seg[b] + r]) > 1 and bool(live_rows[seg[b] + r]) is lv for b, r, lv in spots)
    if case != "n209":               # live rows of several tokens beyond row 256 and beyond row 512
        assert any(256 < r <= 512 and lv for _, r, lv in spots) and any(r > 512 and lv for _, r, lv in spots)
    assert live_rows[seg[all_live] + 1:seg[all_live + 1] - 1].all() and lens[all_live] > 3           # an image that masks nothing
    if all_dead is not None:
        assert not live_rows[seg[all_dead] + 1:seg[all_dead + 1] - 1].any() and lens[all_dead] > 3   # ... and one that masks everything
    with engine.precision(mode):
        dev = lambda t, dt=torch.float32: torch.as_tensor(t).to(dt).to(DEV).contiguous()
        xd, segd, multd, tokd = dev(x), dev(seg, torch.int32), dev(mult, torch.int32), dev(tok_row, torch.int32)
        wgd, bgd, wbd, bbd = dev(wg), dev(bg), dev(wb), dev(bb)
        a = _alloc_step(Rr, B, N, Dm)
        n0 = ops.launch_count
        _train_step(ops.residual_pack_step_long_train, (xd, segd, multd, tokd, wgd, bgd, wbd, bbd), a)
        assert ops.launch_count - n0 == 1
        x_next, src_next, seg_next, tok_next, mult_next, mask_row, gate_arg, thr_out = (a[k] for k in ("x_next", "src_next", "seg_next", "tok_next", "mult_next",
                                                                                                      "mask_row", "gate_arg", "thr_out"))
        # ... and the inference entry on the same inputs: the same results, bit for bit
        i = _alloc_step(Rr, B, N, Dm)
        ops.residual_pack_step_long(xd, segd, multd, tokd, wgd, bgd, wbd, bbd, 1.0, 0.0,
                                    (i["x_next"], i["rs_next"].view(-1), i["mult_next"], i["lm_next"].view(-1), i["seg_next"], i["tok_next"]), i["mask_out"],
                                    i["thr_out"], i["totals"], mask_row=i["mask_row"])
        torch.cuda.synchronize()
        assert a["totals"].tolist() == [Rn, ref["totals"][1]] == i["totals"].tolist()
        for k in ("x_next", "rs_next", "lm_next", "mult_next"):
            assert torch.equal(a[k][:Rn], i[k][:Rn]), k
        for k in ("mask_row", "mask_out", "thr_out", "seg_next", "tok_next"):
            assert torch.equal(a[k], i[k]), k
        assert _untouched(x_next, Rr) and bool(torch.isnan(x_next[Rn:]).all()) and bool((src_next[Rn:] == -7).all()) and bool((mult_next[Rn:] == -7).all())
        assert bool(torch.isnan(a["rs_next"][Rn:]).all()) and bool(torch.isnan(a["lm_next"][Rn:]).all())
        # the tables against the restatement
        assert seg_next.cpu().tolist() == ref["seg_next"].tolist() and np.array_equal(tok_next.cpu().numpy(), ref["tok_row_next"])
        assert mult_next[:Rn].cpu().tolist() == ref["mult_next"].tolist()
        src_rel = ref["src"].numpy().copy()
        img_next = np.repeat(np.arange(B), np.diff(ref["seg_next"]))
        src_rel[src_rel >= 0] -= seg[img_next[src_rel >= 0]]
        assert src_next[:Rn].cpu().tolist() == src_rel.tolist()
        sig = torch.sigmoid(gate_arg.double().cpu())
        mid = torch.isfinite(ref["margin"])
        assert float((sig[mid] - ref["sig"].detach()[mid]).abs().max()) < 1e-6 and bool((gate_arg.cpu()[~mid] == 0).all())
        assert float((x_next[:Rn].double().cpu() - ref["x_next"].detach()).abs().max()) < 1e-5
        # backward
        Gd, drsd, dmd = _guarded(Rn, Dm), dev(drs), dev(dmask)
        Gd[:Rn] = dev(G[:Rn])
        args = (xd, segd, tokd, mask_row, gate_arg, thr_out, seg_next, src_next, Gd, drsd, dmd, wgd, wbd, 1.0)
        out1 = ops.residual_pack_step_long_bwd(*args)
        out2 = ops.residual_pack_step_long_bwd(*args)
        none = ops.residual_pack_step_long_bwd(*args[:10], None, *args[11:])                       # no mask gradient: the dmask terms drop out
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(out1, out2))                                   # two runs: identical bits
        dx, dm_row, dwg, dbg, dwb, dbb = (t.double().cpu() for t in out1)
        dm_none = none[1].double().cpu()
    ulp = 2.0 ** -23
    dead = torch.ones(Rr, dtype=torch.bool)
    dead[ref["src"][ref["src"] >= 0]] = False
    cls = torch.from_numpy(seg[:-1])
    # rows that only move: the class rows are copies, merged rows are exactly zero
    assert torch.equal(dx[cls].float(), G[torch.from_numpy(ref["seg_next"][:-1])]) and bool((dx[dead] == 0).all()) and bool(dead.any())
    assert bool((dm_row[dead] == 0).all()) and bool((dm_row[cls] == 0).all())
    live = ~dead
    live[cls] = False
    live[torch.from_numpy(seg[1:] - 1)] = False
    dm64 = gref["mask_row"]
    got = {"dx": dx, "dm_row": dm_row[live], "dwg": dwg, "dbg": dbg, "dwb": dwb, "dbb": dbb}
    want = {"dx": gref["x"], "dm_row": dm64[live], "dwg": gref["wg"], "dbg": gref["bg"].reshape(1), "dwb": gref["wb"], "dbb": gref["bb"].reshape(1)}
    stock = {"dx": g32["x"], "dm_row": g32["mask_row"][live], "dwg": g32["wg"], "dbg": g32["bg"].reshape(1), "dwb": g32["wb"], "dbb": g32["bb"].reshape(1)}
    for k in got:
        e_hip = float((got[k] - want[k]).abs().max())
        e_stock = float((stock[k].double() - want[k]).abs().max())
        scale = float(want[k].abs().max())
        print(f"pack step backward {case} {mode} {k}: max |err| {e_hip:.3g} (stock fp32 ops {e_stock:.3g}, scale {scale:.3g})")
        assert e_hip <= 2.0 * e_stock + ulp * scale, (k, e_hip, e_stock, scale)
    assert float(want["dwg"].abs().max()) > 0 and float(want["dwb"].abs().max()) > 0 and float(dm64[live].abs().min()) > 0
    # the mask gradient reaches a live row of several tokens as the sum over its tokens: without it dm_row differs exactly there and elsewhere too
    assert bool((dm_none[live] != dm_row[live]).any())


CONTINUITY = {"n20": (128, None),
              "n206": (768, ([208, 2, 3, 100, 150], 206, {2: [(1, True)], 3: [(5, True), (90, False)], 4: [(100, True), (148, False)]}, 0, None))}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CONTINUITY))
def test_up_to_208_rows_the_long_pack_step_has_the_resident_bits(case, mode):
    """(B, N, D) = (5, 20, 128), the resident test's own case, and (5, 206, 768): every output of pv_residual_pack_step_long_train and of
    pv_residual_pack_step_long_bwd is bit-equal to pv_residual_pack_step_train's / pv_residual_pack_step_bwd's."""
    from peekvit_amd import engine
    Dm, spec = CONTINUITY[case]
    if spec is None:
        x, seg, mult, tok_row, wg, bg, wb, bb = _pack_case(Dm, seed=Dm)
        N, B = tok_row.shape[1], len(IMAGES)
    else:
        lens, N, multi, all_live, all_dead = spec
        x, seg, mult, tok_row, wg, bg, wb, bb = _long_pack_case(lens, N, Dm, seed=N, multi=multi, all_live=all_live, all_dead=all_dead)
        B = len(lens)
    Rr = x.shape[0]
    assert B == 5 and N + 2 <= RESIDENT
    gen = torch.Generator().manual_seed(N)
    G, drs, dmask = torch.randn(Rr, Dm, generator=gen), torch.randn(Rr, generator=gen), torch.randn(B, N, generator=gen)
    with engine.precision(mode):
        dev = lambda t, dt=torch.float32: torch.as_tensor(t).to(dt).to(DEV).contiguous()
        dev_in = (dev(x), dev(seg, torch.int32), dev(mult, torch.int32), dev(tok_row, torch.int32), dev(wg), dev(bg), dev(wb), dev(bb))
        a, r = _alloc_step(Rr, B, N, Dm), _alloc_step(Rr, B, N, Dm)
        _train_step(ops.residual_pack_step_long_train, dev_in, a)
        _train_step(ops.residual_pack_step_train, dev_in, r)
        torch.cuda.synchronize()
        Rn = a["totals"].tolist()[0]
        assert a["totals"].tolist() == r["totals"].tolist() and 2 * B <= Rn < Rr
        for k in a:
            same = (a[k][:Rn], r[k][:Rn]) if k in ("x_next", "rs_next", "lm_next", "mult_next", "src_next") else (a[k], r[k])
            assert torch.equal(*same), k
            assert torch.equal(a[k].isnan() if a[k].is_floating_point() else a[k] == -7, r[k].isnan() if r[k].is_floating_point() else r[k] == -7), k
        Gd = _guarded(Rn, Dm)
        Gd[:Rn] = dev(G[:Rn])
        for dm in (dev(dmask), None):
            args = (dev_in[0], dev_in[1], dev_in[3], a["mask_row"], a["gate_arg"], a["thr_out"], a["seg_next"], a["src_next"], Gd, dev(drs), dm, dev_in[4],
                    dev_in[6], 1.0)
            n0 = ops.launch_count
            got = ops.residual_pack_step_long_bwd(*args)
            n1 = ops.launch_count
            want = ops.residual_pack_step_bwd(*args)
            assert n1 - n0 == ops.launch_count - n1                                                 # the sibling's launch count
            torch.cuda.synchronize()
            for k, p, q in zip(("dx", "dm_row", "dwg", "dbg", "dwb", "dbb"), got, want):
                assert torch.equal(p, q), (k, dm is None)
            assert float(got[0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. one training step of the model past 208 rows against the fp64 composite; the switch off again; an overflowing step
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TRAIN_MODES)
@pytest.mark.parametrize("name", list(long_host.CASES))
def test_packed_training_step_past_208_rows_against_the_fp64_composite(name, mode):
    """tests/test_hip_residual_sparse_train.py's step test on the three cases of tests/test_residual_sparse_long_train_host.py (which holds their
    preconditions): loss, logits and the complete gradient of one packed step against the fp64 composite at the same budgets, each within the
    larger of the README's training tolerance (1e-3 forward, 2e-3 gradients) and 1.5 x what the dense HIP training path measures on the same
    inputs here.  Which layers streamed is read from the engine's counters."""
    from peekvit_amd import engine, train_engine
    cfg, m64, x, y, budgets = long_host.build(name)
    streams = long_host.CASES[name][6]
    ref_loss, ref_logits, ref_masks, ref_grads = host.dense_step(m64, x, y)
    ref_grads = {k: (torch.zeros_like(p) if ref_grads[k] is None else ref_grads[k]) for k, p in m64.named_parameters()}
    margins = _margins(m64, x)
    excluded = [mg < KNEE for mg in margins]
    share = float(torch.cat([e.reshape(-1) for e in excluded]).double().mean())
    assert share <= 0.05, share                      # (checked on the CPU for the chosen seeds: the reference itself stays under the cap)
    xg, yg = x.float().to(DEV), y.to(DEV)
    L, rows = cfg["num_layers"], ref_masks[0].shape[1] + 2
    with engine.precision(mode):
        dense = _gpu_step(_gpu_model(cfg, m64, budgets), xg, yg)
        mp = _gpu_model(cfg, m64, budgets)
        assert mp.compact_training is False and mp.set_compact_training(True) is mp and mp.compact_training is True
        n0, r0, d0, s0 = engine.sparse_train_dense_forwards, engine.sparse_rows, engine.sparse_dense_rows, engine.sparse_syncs
        l0, i0 = engine.sparse_train_long_layers, engine.sparse_long_layers
        packed = _gpu_step(mp, xg, yg)
        assert engine.sparse_train_dense_forwards == n0                                     # the packed path ran
        assert engine.sparse_rows - r0 < engine.sparse_dense_rows - d0 == L * x.shape[0] * rows
        assert engine.sparse_syncs - s0 == L
        longest = engine.sparse_last_max_len
        print(f"\n{name} {mode}: longest segment per layer {longest}, rows per layer {engine.sparse_last_rows}")
        assert [ml > RESIDENT for ml in longest] == streams and len(engine.sparse_last_rows) == L
        assert engine.sparse_train_long_layers - l0 == sum(streams) and engine.sparse_long_layers == i0       # (the inference counter is another one)
        assert not train_engine.last_step_skipped(mp)
        # the switch off again: the dense step, bit for bit
        n1 = engine.sparse_train_dense_forwards
        off = _gpu_step(mp.set_compact_training(False), xg, yg)
        assert engine.sparse_train_dense_forwards == n1 and engine.sparse_train_long_layers - l0 == sum(streams)
        assert off[0] == dense[0] and torch.equal(off[1], dense[1]) and _same_grads(off[4], dense[4])
    gref = _complete(ref_grads, ref_grads)
    errs = {}
    for tag, got in (("dense", dense), ("packed", packed)):
        errs[tag] = (abs(got[0] - float(ref_loss)) / abs(float(ref_loss)), rel_l2(got[1], ref_logits), rel_l2(_complete(got[4], ref_grads), gref))
    print(f"{name} {mode}: loss / logits / complete gradient vs fp64 - dense HIP {errs['dense'][0]:.3g} / {errs['dense'][1]:.3g} / {errs['dense'][2]:.3g}, "
          f"packed {errs['packed'][0]:.3g} / {errs['packed'][1]:.3g} / {errs['packed'][2]:.3g}; tokens within {KNEE} of the knee {share:.4f}")
    for i, tol in enumerate((1e-3, 1e-3, 2e-3)):
        assert errs["packed"][i] <= max(tol, 1.5 * errs["dense"][i]), (i, errs)
    for md, mpk, td, tpk, ex in zip(dense[2], packed[2], dense[3], packed[3], excluded):
        keep = ~ex.to(DEV)
        assert mpk.shape == md.shape and mpk.requires_grad is False
        assert torch.equal((mpk[..., 0] == 0)[keep], (md[..., 0] == 0)[keep])
        assert float((mpk[..., 0] - md[..., 0])[keep].abs().max()) < KNEE and float((tpk - td).abs().max()) < KNEE
    assert any(bool((mk == 0).any()) for mk in packed[2])


def test_an_overflowing_packed_step_past_208_rows_is_dropped_like_the_dense_one():
    """Inputs scaled beyond fp16's range in the fp16 pass at 402 rows: the step is dropped - every .grad is None and last_step_skipped is true - with
    the switch on exactly as with it off."""
    from peekvit_amd import engine, train_engine
    cfg, m64, x, y, budgets = long_host.build("all_stream")
    xg, yg = (x.float() * 1.0e6).to(DEV), y.to(DEV)
    with engine.precision("auto"):
        for on in (False, True):
            m = _gpu_model(cfg, m64, budgets).set_compact_training(on)
            assert train_engine.pass_operand(m) == "f16"
            n0 = engine.sparse_train_dense_forwards
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                torch.nn.functional.cross_entropy(m(xg), yg).backward()
                assert train_engine.last_step_skipped(m), on
            assert all(p.grad is None for p in m.parameters()), on
            assert engine.sparse_train_dense_forwards == n0                                 # (on: the packed path took it; off: nothing to count)
