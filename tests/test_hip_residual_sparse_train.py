"""ResidualViT training on the packed rows, the kernels on the GPU (include/peekvit_hip_sparse_train.h), in both operand
libraries: the ragged weighted attention forward with row statistics and its backward against fp64 (tests/residual_sparse_train_ref.py), and the
pack step for training and its backward against fp64 autograd of the differentiable restatement of pack_step_ref.

Every output has trailing rows that belong to no segment, filled with NaN, which must still be NaN afterwards."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2
from peekvit_amd import ops
import residual_sparse_ref as R
import residual_sparse_train_ref as T
from test_hip_attn_stream import CAP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["bf16", "f16"]
NAN = float("nan")
H, DH = 2, 64
D = H * DH
EXTRA_ROWS = 2          # rows behind the last segment: inputs exist, outputs must stay NaN
LAYOUTS = {"1-17-65-208": [1, 17, 65, 208], "64-128-2-208": [64, 128, 2, 208]}
WEIGHTS = ["none", "mixed", "dominant"]


def _guarded(rows, cols, dtype=torch.float32):
    """(rows + EXTRA_ROWS, cols) filled with NaN; the kernels see the whole buffer but own only the first `rows` rows."""
    return torch.full((rows + EXTRA_ROWS, cols), NAN, dtype=dtype, device=DEV)


def _untouched(full, rows):
    return bool(torch.isnan(full[rows:].float()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. ragged weighted attention: forward with statistics, backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _attn_inputs(lens, weights, dt, seed):
    """qkv 16-bit [R + EXTRA_ROWS, 3 D] (q pre-scaled), dout, seg int32 [B + 1], log_mult fp32 [R + EXTRA_ROWS].  `dominant`: one key per segment is
    alpha * u for a direction u that every query shares a component of, and carries ln 150: it holds >= 0.99 of every row's probability."""
    g = torch.Generator().manual_seed(seed)
    Rr = sum(lens)
    seg = np.concatenate([[0], np.cumsum(lens)])
    rows = Rr + EXTRA_ROWS
    bf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).float()
    qkv = bf(rows, 3 * D)
    lm = torch.zeros(rows)
    if weights == "mixed":
        choice = torch.randint(0, 3, (rows,), generator=g)
        lm = torch.tensor([0.0, math.log(2.0), math.log(150.0)])[choice]
    if weights == "dominant":
        u = torch.zeros(D)
        u[0::DH] = 1.0                      # the first coordinate of every head
        qkv[:, 0:D:DH] = 12.0               # (before the 1 / 8 below: every query has exactly 1.5 along u in each head)
        for b, n in enumerate(lens):
            # the other keys' scores are ~ N(0, 1.8^2): their log-sum-exp is about ln(n - 1) + 1.6.  The key is scaled so that its score plus
            # ln 150 lies 6.1 above that: p ~ 0.997, and 0.99 or more in every row (asserted where the case is used) - the least extreme case
            # that meets that condition.  (Beyond it the fp16 build meets a floor of its own: p is recomputed from the fp32 statistics, whose
            # rounding eps ~ 2e-6 is common to a row's keys and reaches dS of the dominant key as eps / (1 - p))
            alpha = max(6.1 + math.log(max(n - 1, 1)) + 1.6 - math.log(150.0), 0.0) / 1.5
            j = int(seg[b]) + (n * 2) // 3
            qkv[j, D:2 * D] = (alpha * u).to(torch.bfloat16).float()
            lm[j] = math.log(150.0)
    qkv[:, :D] *= DH ** -0.5
    dout = bf(rows, D, scale=0.1)
    return qkv.to(dt).to(DEV), dout.to(dt).to(DEV), torch.from_numpy(seg.astype(np.int32)).to(DEV), lm.to(DEV)


def _run_attention(qkv, dout, seg, lm, lens, dt):
    Rr, B, max_len = sum(lens), len(lens), max(lens)
    nb = (max_len + 63) // 64
    out, lse, g16 = _guarded(Rr, D, dt), _guarded(Rr, H), _guarded(Rr, 3 * D, dt)
    part, delta = _guarded(B * nb, 3 * D), _guarded(Rr, H)
    n0 = ops.launch_count
    ops.attention_varlen_w_lse(qkv, out, lse, seg, lm, max_len, H, DH)
    ops.attention_varlen_w_bwd16(qkv, dout, out, lse, seg, lm, g16, max_len, H, DH, DH ** -0.5, dbias_partial=part[:B * nb], delta_ws=delta)
    assert ops.launch_count - n0 == 2
    torch.cuda.synchronize()
    assert all(_untouched(f, n) for f, n in ((out, Rr), (lse, Rr), (g16, Rr), (part, B * nb), (delta, Rr)))
    return out[:Rr], lse[:Rr], g16[:Rr], part[:B * nb], delta[:Rr]


def _restated_ragged(qkv, dout, out16, seg, lm, dt):
    """The backward on stock ops in fp32 with the kernels' rounding points (test_hip_rank_train._restated_weighted per segment): P rounded to the
    operand type for dV, dS rounded for dQ and dK; delta from p and dP in fp32 in a segment with a weight, from the 16-bit output otherwise."""
    res = torch.zeros((qkv.shape[0], 3 * D), device=DEV)
    seg = seg.cpu().numpy()
    for b in range(len(seg) - 1):
        s0, s1 = int(seg[b]), int(seg[b + 1])
        n = s1 - s0
        q, k, v = (qkv[s0:s1, i * D:(i + 1) * D].float().reshape(n, H, DH).transpose(0, 1) for i in range(3))
        do = dout[s0:s1].float().reshape(n, H, DH).transpose(0, 1)
        P = torch.softmax(q @ k.transpose(-1, -2) + lm[s0:s1], dim=-1)
        dP = do @ v.transpose(-1, -2)
        if bool((lm[s0:s1] != 0).any()):
            delta = (P * dP).sum(-1, keepdim=True)
        else:
            delta = (do * out16[s0:s1].float().reshape(n, H, DH).transpose(0, 1)).sum(-1, keepdim=True)
        dS = (P * (dP - delta)).to(dt).float()
        dv = P.to(dt).float().transpose(-1, -2) @ do
        dq, dk = (dS @ k) * DH ** -0.5, dS.transpose(-1, -2) @ q
        res[s0:s1] = torch.cat([t.transpose(0, 1).reshape(n, D) for t in (dq, dk, dv)], dim=-1)
    return res.to(dt).float()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ragged_weighted_attention_forward_and_backward_against_fp64(layout, weights, mode):
    """Bounds: those tests/test_hip_rank_train.py::test_weighted_stream_attention applies to the uniform weighted pair - forward |lse| 1e-4 and out
    6e-3; backward twice the stock-op restatement with the kernels' rounding points + 1e-5, and CAP; bias partials 64 * 2^-24 of the summed
    magnitudes."""
    from peekvit_amd import _lib, engine
    lens = LAYOUTS[layout]
    Rr, B = sum(lens), len(lens)
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout, seg, lm = _attn_inputs(lens, weights, dt, seed=len(layout) + WEIGHTS.index(weights))
        out, lse, g16, part, delta = _run_attention(qkv, dout, seg, lm, lens, dt)
        again = _run_attention(qkv, dout, seg, lm, lens, dt)
        assert all(torch.equal(a, b) for a, b in zip(again, (out, lse, g16, part, delta)))          # two runs: identical bits
        # the forward shares the inference kernel's body: the same `out`, bit for bit
        inf = torch.empty((Rr, D), dtype=dt, device=DEV)
        ops.attention_varlen_w(qkv[:Rr], inf, seg, lm[:Rr], max(lens), H, DH)
        assert torch.equal(inf, out)
        q64, lm64 = qkv[:Rr].double().cpu(), lm[:Rr].double().cpu()
        ref_out, ref_lse = T.attention_w_train_ref(q64, seg.cpu(), lm64, H)
        ref_g, _ = T.attention_w_backward_ref(q64, dout[:Rr].cpu(), seg.cpu(), lm64, H, DH ** -0.5)
        if weights == "dominant":
            # the case's own precondition: the weighted key holds >= 0.99 of every row's probability
            segn = seg.cpu().numpy()
            for b, n in enumerate(lens):
                s0, j = int(segn[b]), (n * 2) // 3
                qh, kh = (q64[s0:s0 + n, i * D:(i + 1) * D].reshape(n, H, DH).transpose(0, 1) for i in range(2))
                p = torch.softmax(qh @ kh.transpose(-1, -2) + lm64[s0:s0 + n], dim=-1)
                assert float(p[..., j].min()) >= 0.99, (b, float(p[..., j].min()))
        e_lse, e_out = float((lse.double().cpu() - ref_lse).abs().max()), rel_l2(out.float(), ref_out)
        print(f"\nragged forward {layout} {weights} {mode}: |lse - fp64| max {e_lse:.3g}, out rel L2 {e_out:.3g}")
        assert e_lse < 1e-4
        assert e_out < 6e-3
        restated = _restated_ragged(qkv[:Rr], dout[:Rr], out, seg, lm[:Rr], dt)
        errs = {}
        for i, name in enumerate("qkv"):
            sl = slice(i * D, (i + 1) * D)
            errs[name] = err, base = rel_l2(g16[:, sl].float(), ref_g[:, sl]), rel_l2(restated[:, sl], ref_g[:, sl])
            print(f"ragged backward {layout} {weights} {mode} d{name}: rel L2 {err:.3g} (restated on stock ops {base:.3g})")
        for name, (err, base) in errs.items():
            assert err <= 2.0 * base + 1e-5, (name, err, base)
            assert err < CAP[mode], (name, err)
        # the bias partial rows: per (image, 64-row block) the column sums of the STORED values; a block beyond its segment holds zeros
        nb = (max(lens) + 63) // 64
        v = g16.double()
        segn = seg.cpu().numpy()
        for b, n in enumerate(lens):
            for blk in range(nb):
                lo, hi = int(segn[b]) + min(blk * 64, n), int(segn[b]) + min(blk * 64 + 64, n)
                want, mag = v[lo:hi].sum(0), v[lo:hi].abs().sum(0)
                assert ((part[b * nb + blk].double() - want).abs() <= 64 * 2.0 ** -24 * mag).all(), (b, blk)


def test_attention_entry_points_refuse_bad_arguments():
    import test_residual_sparse_train_host as host
    host.check_attention_argument_validation()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the pack step for training and its backward
# ---------------------------------------------------------------------------------------------------------------------------------
N_TOK = 20
# per image: (multiplicity, live) of every row between the class row and the budget row; the multiplicities of an image add up to N_TOK
IMAGES = [
    [(1, True)] * 20,                                                                   # nothing masked
    [(1, False)] * 20,                                                                  # everything but the class row masked
    [(1, True), (5, True), (7, False), (1, False), (1, True), (1, True), (1, False), (1, True), (1, True), (1, False)],   # class rows: one live, one merging
    [(9, False), (3, True), (4, False), (4, True)],                                     # class rows only
    [(20, True)],                                                                       # one class row for every token, live again
]


def _pack_case(Dm, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [len(im) + 2 for im in IMAGES]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Rr, B = int(seg[-1]), len(IMAGES)
    x = torch.randn(Rr, Dm, generator=g)
    wg = torch.randn(Dm, generator=g) * 0.02
    wg[0] = 2.0
    wb = torch.randn(Dm, generator=g) * 0.02
    bg, bb = torch.tensor([0.1]), torch.tensor([-0.2])
    mult = np.ones(Rr, dtype=np.int64)
    tok_row = np.zeros((B, N_TOK), dtype=np.int64)
    for b, im in enumerate(IMAGES):
        rows = []
        for i, (mu, live) in enumerate(im):
            r = int(seg[b]) + 1 + i
            mult[r] = mu
            # the gate reads (almost only) coordinate 0: well away from the threshold on either side, so fp32 and fp64 agree on who is live
            x[r, 0] = (1.5 + 0.5 * float(torch.rand((), generator=g))) * (1.0 if live else -1.0)
            rows += [1 + i] * mu
        perm = torch.randperm(N_TOK, generator=g).numpy()
        tok_row[b, perm] = np.asarray(rows)
    return x, seg, mult, tok_row, wg, bg, wb, bb


def _ref_step(x, seg, mult, tok_row, wg, bg, wb, bb, G, drs, dmask, dtype):
    """pack_step_train_ref and its autograd in `dtype` on the CPU: (step dict, {name: gradient})."""
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in dict(x=x, wg=wg, bg=bg, wb=wb, bb=bb).items()}
    st = T.pack_step_train_ref(leaves["x"], seg, mult, tok_row, leaves["wg"], leaves["bg"], leaves["wb"], leaves["bb"], 1.0, 0.0)
    Rn = st["x_next"].shape[0]
    loss = (st["x_next"] * G[:Rn].to(dtype)).sum() + (st["row_scale_next"] * drs[:Rn].to(dtype)).sum() + (st["mask_out"] * dmask.to(dtype)).sum()
    names = list(leaves) + ["mask_row"]
    grads = torch.autograd.grad(loss, [leaves[k] for k in leaves] + [st["mask_row"]], allow_unused=True)
    return st, dict(zip(names, grads))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Dm", [128, 768])
def test_pack_step_train_and_its_backward_against_fp64_autograd(Dm, mode):
    """The reference is fp64 autograd of residual_sparse_train_ref.pack_step_train_ref - pack_step_ref's arithmetic and tables
    (tests/test_residual_sparse_train_host.py holds the two equal), written without pack_step_ref's in-place write into relu's output, which autograd
    refuses.  Rows that only move (class rows, rows merged into the zero row) are exact; everything that passes through a reduction (dm_row, the
    live rows' dx through dz, the gate and budget-gate gradients) gets twice the error of the same formula in stock fp32 torch ops against fp64 on
    the same inputs, plus one fp32 ulp of the result's scale."""
    from peekvit_amd import engine
    x, seg, mult, tok_row, wg, bg, wb, bb = _pack_case(Dm, seed=Dm)
    Rr, B = x.shape[0], len(IMAGES)
    gen = torch.Generator().manual_seed(Dm + 1)
    G, drs, dmask = torch.randn(Rr, Dm, generator=gen), torch.randn(Rr, generator=gen), torch.randn(B, N_TOK, generator=gen)
    ref, gref = _ref_step(x, seg, mult, tok_row, wg, bg, wb, bb, G, drs, dmask, torch.float64)
    _, g32 = _ref_step(x, seg, mult, tok_row, wg, bg, wb, bb, G, drs, dmask, torch.float32)
    Rn = ref["x_next"].shape[0]
    with engine.precision(mode):
        dev = lambda t, dt=torch.float32: torch.as_tensor(t).to(dt).to(DEV).contiguous()
        xd, segd, multd, tokd = dev(x), dev(seg, torch.int32), dev(mult, torch.int32), dev(tok_row, torch.int32)
        wgd, bgd, wbd, bbd = dev(wg), dev(bg), dev(wb), dev(bb)
        x_next, rs_next, lm_next = _guarded(Rr, Dm), _guarded(Rr, 1), _guarded(Rr, 1)
        mult_next, src_next = torch.full((Rr,), -7, dtype=torch.int32, device=DEV), torch.full((Rr,), -7, dtype=torch.int32, device=DEV)
        seg_next, tok_next = torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros((B, N_TOK), dtype=torch.int32, device=DEV)
        mask_out, thr_out, totals = torch.empty((B, N_TOK), device=DEV), torch.empty(B, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        mask_row, gate_arg = torch.empty(Rr, device=DEV), torch.empty(Rr, device=DEV)
        ops.residual_pack_step_train(xd, segd, multd, tokd, wgd, bgd, wbd, bbd, 1.0, 0.0,
                                     (x_next, rs_next.view(-1), mult_next, lm_next.view(-1), seg_next, tok_next), mask_out, thr_out, totals, mask_row,
                                     gate_arg, src_next)
        # ... and the inference entry on the same inputs: the same results, bit for bit
        x_inf, rs_inf, lm_inf = torch.empty((Rr, Dm), device=DEV), torch.empty(Rr, device=DEV), torch.empty(Rr, device=DEV)
        mult_inf, seg_inf, tok_inf = torch.empty_like(mult_next), torch.empty_like(seg_next), torch.empty_like(tok_next)
        mo_inf, th_inf, tot_inf, mr_inf = torch.empty_like(mask_out), torch.empty_like(thr_out), torch.empty_like(totals), torch.empty_like(mask_row)
        ops.residual_pack_step(xd, segd, multd, tokd, wgd, bgd, wbd, bbd, 1.0, 0.0, (x_inf, rs_inf, mult_inf, lm_inf, seg_inf, tok_inf), mo_inf, th_inf,
                               tot_inf, mask_row=mr_inf)
        torch.cuda.synchronize()
        assert totals.tolist() == [Rn, ref["totals"][1]] == tot_inf.tolist()
        assert torch.equal(x_next[:Rn], x_inf[:Rn]) and torch.equal(rs_next.view(-1)[:Rn], rs_inf[:Rn]) and torch.equal(mask_row, mr_inf)
        assert torch.equal(mask_out, mo_inf) and torch.equal(thr_out, th_inf) and torch.equal(seg_next, seg_inf) and torch.equal(tok_next, tok_inf)
        assert torch.equal(mult_next[:Rn], mult_inf[:Rn])
        assert _untouched(x_next, Rr) and bool(torch.isnan(x_next[Rn:]).all()) and bool((src_next[Rn:] == -7).all())
        # the tables against the restatement
        assert seg_next.cpu().tolist() == ref["seg_next"].tolist() and tok_next.cpu().numpy().tolist() == ref["tok_row_next"].tolist()
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
        out1 = ops.residual_pack_step_bwd(xd, segd, tokd, mask_row, gate_arg, thr_out, seg_next, src_next, Gd, drsd, dmd, wgd, wbd, 1.0)
        out2 = ops.residual_pack_step_bwd(xd, segd, tokd, mask_row, gate_arg, thr_out, seg_next, src_next, Gd, drsd, dmd, wgd, wbd, 1.0)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out1, out2))                                   # two runs: identical bits
        dx, dm_row, dwg, dbg, dwb, dbb = (t.double().cpu() for t in out1)
    ulp = 2.0 ** -23
    dead = torch.ones(Rr, dtype=torch.bool)
    dead[ref["src"][ref["src"] >= 0]] = False
    cls = torch.from_numpy(seg[:-1])
    # rows that only move: the class rows are copies, merged rows are exactly zero
    assert torch.equal(dx[cls].float(), G[torch.from_numpy(ref["seg_next"][:-1])]) and bool((dx[dead] == 0).all()) and bool(dead.any())
    assert bool((dm_row[dead] == 0).all()) and bool((dm_row[cls] == 0).all())
    # the live rows' mask * G: one multiply in fp32 (their dz * wg part is taken out with the fp64 dz)
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
        print(f"pack step backward D {Dm} {mode} {k}: max |err| {e_hip:.3g} (stock fp32 ops {e_stock:.3g}, scale {scale:.3g})")
        assert e_hip <= 2.0 * e_stock + ulp * scale, (k, e_hip, e_stock, scale)
    assert float(want["dwg"].abs().max()) > 0 and float(want["dwb"].abs().max()) > 0 and float(dm64[live].abs().min()) > 0


def test_pack_step_entry_points_refuse_bad_arguments():
    import test_residual_sparse_train_host as host
    host.check_pack_step_argument_validation()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. one training step of the model on the packed rows against the fp64 composite; 4. fallbacks; 5. an overflowing step
# ---------------------------------------------------------------------------------------------------------------------------------
TRAIN_MODES = ["bf16", "auto"]          # the pass's operand library: bf16, and fp16 under the loss scale (mode "auto")
KNEE = 1e-3


def _gpu_model(cfg, m64, budgets, **over):
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    m = ResidualVisionTransformer(**dict(cfg, **over))
    m.load_state_dict({k: v.float() for k, v in m64.state_dict().items()})
    m = m.to(DEV).train()
    bud = torch.tensor(budgets, dtype=torch.float32)
    m._sample_budget = lambda n: bud.clone()
    return m


def _gpu_step(m, x, y):
    import test_residual_sparse_train_host as host
    from peekvit_amd import losses
    m.zero_grad(set_to_none=True)
    logits = m(x)
    loss = torch.nn.functional.cross_entropy(logits, y) + losses.budget_mse(m, host.LOSS_BUDGET)
    loss.backward()
    torch.cuda.synchronize()
    masks = [blk.mask.detach().clone() for blk in m.encoder.layers]
    thrs = [blk.residual_gate.threshold.detach().reshape(-1).clone() for blk in m.encoder.layers]
    return float(loss.detach()), logits.detach(), masks, thrs, {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _complete(grads, ref):
    """Every parameter gradient as one vector, in the reference's order (a gradient that is None counts as zeros)."""
    return torch.cat([(torch.zeros_like(ref[k], dtype=torch.float64) if grads[k] is None else grads[k].double().cpu()).reshape(-1) for k in ref])


def _margins(m64, x):
    """|sigmoid - threshold| of every token in every block of the fp64 composite: the distance to the relu's knee."""
    out, hooks = [], []
    def pre(blk, inp):
        t = inp[0]
        thr = torch.sigmoid(blk.budget_token_gate(t[:, -1:]))
        sig = torch.sigmoid(blk.residual_gate.projection(t[:, 1:-1]) / blk.residual_gate.temp + blk.residual_gate.sigmoid_bias)
        out.append((sig - thr).abs().squeeze(-1).detach())
    for blk in m64.encoder.layers:
        hooks.append(blk.register_forward_pre_hook(pre))
    with torch.no_grad():
        m64(x)
    for h in hooks:
        h.remove()
    return out


@pytest.mark.parametrize("mode", TRAIN_MODES)
@pytest.mark.parametrize("name", ["micro", "rows198"])
def test_packed_training_step_against_the_fp64_composite(name, mode):
    """Loss, logits and the complete gradient of one packed step against the fp64 composite at the same budgets.  The limit for each is the larger
    of the README's training tolerance (1e-3 forward, 2e-3 gradients) and 1.5 x what the dense HIP training path measures on the same inputs here
    (the factor allows for the weighted-key softmax and the extra 16-bit rounding of packed class rows).  Measured pairs: DESIGN.md section 29."""
    import test_residual_sparse_train_host as host
    from peekvit_amd import engine, train_engine
    cfg, m64, x, y, budgets = host.build(name)
    ref_loss, ref_logits, ref_masks, ref_grads = host.dense_step(m64, x, y)
    ref_grads = {k: (torch.zeros_like(p) if ref_grads[k] is None else ref_grads[k]) for k, p in m64.named_parameters()}
    margins = _margins(m64, x)
    excluded = [mg < KNEE for mg in margins]
    share = float(torch.cat([e.reshape(-1) for e in excluded]).double().mean())
    assert share <= 0.05, share                      # (checked on the CPU for the chosen seeds: the reference itself stays under the cap)
    xg, yg = x.float().to(DEV), y.to(DEV)
    with engine.precision(mode):
        dense = _gpu_step(_gpu_model(cfg, m64, budgets), xg, yg)
        mp = _gpu_model(cfg, m64, budgets)
        assert mp.compact_training is False and mp.set_compact_training(True) is mp and mp.compact_training is True
        n0, r0, d0, s0 = engine.sparse_train_dense_forwards, engine.sparse_rows, engine.sparse_dense_rows, engine.sparse_syncs
        packed = _gpu_step(mp, xg, yg)
        assert engine.sparse_train_dense_forwards == n0                                     # the packed path ran
        assert engine.sparse_rows - r0 < engine.sparse_dense_rows - d0 == cfg["num_layers"] * x.shape[0] * (ref_masks[0].shape[1] + 2)
        assert engine.sparse_syncs - s0 == cfg["num_layers"]
        assert not train_engine.last_step_skipped(mp)
    gref = _complete(ref_grads, ref_grads)
    errs = {}
    for tag, got in (("dense", dense), ("packed", packed)):
        errs[tag] = (abs(got[0] - float(ref_loss)) / abs(float(ref_loss)), rel_l2(got[1], ref_logits), rel_l2(_complete(got[4], ref_grads), gref))
    print(f"\n{name} {mode}: loss / logits / complete gradient vs fp64 - dense HIP {errs['dense'][0]:.3g} / {errs['dense'][1]:.3g} / {errs['dense'][2]:.3g}, "
          f"packed {errs['packed'][0]:.3g} / {errs['packed'][1]:.3g} / {errs['packed'][2]:.3g}; tokens within {KNEE} of the knee {share:.4f}")
    for i, tol in enumerate((1e-3, 1e-3, 2e-3)):
        assert errs["packed"][i] <= max(tol, 1.5 * errs["dense"][i]), (i, errs)
    # masks and thresholds as the dense HIP path leaves them, wherever no token sits at the knee: the same zeros, and values that differ by less
    # than the knee's width (a mask is sigmoid - threshold of rows the two paths round differently by the forward tolerance; sigmoid' <= 1 / 4)
    for md, mpk, td, tpk, ex in zip(dense[2], packed[2], dense[3], packed[3], excluded):
        keep = ~ex.to(DEV)
        assert mpk.shape == md.shape and mpk.requires_grad is False
        assert torch.equal((mpk[..., 0] == 0)[keep], (md[..., 0] == 0)[keep])
        assert float((mpk[..., 0] - md[..., 0])[keep].abs().max()) < KNEE and float((tpk - td).abs().max()) < KNEE
    assert any(bool((mk == 0).any()) for mk in packed[2])


def _same_grads(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k])) for k in a) and set(a) == set(b)


def test_fallbacks_train_through_the_dense_path_bit_for_bit():
    """With the switch on, a forward under dropout, one with a forward hook on a block and one on a model with a removed layer train through the
    dense path: counted, and the dense path's gradients bit for bit.  (Dropout draws: the same seed on both sides.)"""
    import test_residual_sparse_train_host as host
    from peekvit_amd import engine
    cfg, m64, x, y, budgets = host.build("micro")
    xg, yg = x.float().to(DEV), y.to(DEV)

    def pair(edit, stock=False, **over):
        res = []
        for on in (False, True, False):
            m = _gpu_model(cfg, m64, budgets, **over)
            edit(m)
            m.set_compact_training(on)
            n0, r0 = engine.sparse_train_dense_forwards, engine.sparse_rows
            torch.manual_seed(11)
            res.append(_gpu_step(m, xg, yg))
            assert engine.sparse_train_dense_forwards - n0 == (1 if on else 0) and engine.sparse_rows == r0
        off, on, off2 = res
        assert off[0] == on[0] and torch.equal(off[1], on[1])
        assert any(g is not None for g in on[4].values())
        if stock and not _same_grads(off[4], off2[4]):
            # under dropout the whole model trains on stock torch ops, whose backward adds with atomics: two runs of that path with the switch OFF
            # do not repeat their own bits, so "bit for bit" has no meaning there.  The switch then has to stay inside that path's own run-to-run
            # difference (twice it; floor 1e-6, the size of an fp32 reordering)
            worst = lambda u, v: max(rel_l2(u[k], v[k]) for k in u if u[k] is not None and float(v[k].norm()) > 0)
            noise, diff = worst(off2[4], off[4]), worst(on[4], off[4])
            print(f"\nstock-op path: switch off twice {noise:.3g}, on against off {diff:.3g}")
            assert diff <= max(2.0 * noise, 1e-6), (diff, noise)
        else:
            assert _same_grads(off[4], on[4])

    pair(lambda m: None, stock=True, dropout=0.1)
    pair(lambda m: m.encoder.layers[1].register_forward_hook(lambda *a: None))
    def remove(m):
        del m.encoder.layers[1]
    pair(remove)
    # eval mode is not affected by the switch
    m = _gpu_model(cfg, m64, budgets).eval().set_compact_training(True)
    m.set_budget(0.5)
    n0, r0 = engine.sparse_train_dense_forwards, engine.sparse_rows
    with torch.no_grad():
        a = m(xg)
        b = m.set_compact_training(False)(xg)
    assert torch.equal(a, b) and engine.sparse_train_dense_forwards == n0 and engine.sparse_rows == r0


def test_switch_off_is_the_dense_training_step():
    """With the switch off nothing in a training step changes: two dense steps in this process, one on a model that never saw the switch and one on a
    model that had it on and off again, bit for bit."""
    import test_residual_sparse_train_host as host
    cfg, m64, x, y, budgets = host.build("micro")
    xg, yg = x.float().to(DEV), y.to(DEV)
    a = _gpu_step(_gpu_model(cfg, m64, budgets), xg, yg)
    m = _gpu_model(cfg, m64, budgets)
    m.set_compact_training(True).set_compact_training(False)
    b = _gpu_step(m, xg, yg)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and _same_grads(a[4], b[4])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


def test_an_overflowing_packed_step_is_dropped_like_the_dense_paths():
    """Inputs scaled beyond fp16's range in the fp16 pass: the step is dropped - every .grad is None and last_step_skipped is true - with the switch
    on exactly as with it off."""
    import warnings
    import test_residual_sparse_train_host as host
    from peekvit_amd import engine, train_engine
    cfg, m64, x, y, budgets = host.build("micro")
    xg, yg = (x.float() * 1.0e6).to(DEV), y.to(DEV)
    with engine.precision("auto"):
        for on in (False, True):
            m = _gpu_model(cfg, m64, budgets).set_compact_training(on)
            assert train_engine.pass_operand(m) == "f16"
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                torch.nn.functional.cross_entropy(m(xg), yg).backward()
                assert train_engine.last_step_skipped(m), on
            assert all(p.grad is None for p in m.parameters()), on
