"""A-ViT training on the packed live rows on the MI355X: the pack step's two entry points (pv_avit_pack_step_train /
pv_avit_pack_step_bwd) against the fp64 restatement of tests/avit_packed_train_ref.py on the same fp32 inputs, train_engine.avit_packed_block_forward_train against
the fp64 block on the expanded dense rows, and the whole packed training pass (`set_packed_training`) against an fp64 composite that replays the
packed pass's own halting decisions - next to the dense fused pass measured on the same case.

The backward's reference is the restatement's hand-written pack_step_bwd, not autograd of pack_step_fwd: a packed forward has no graph from a merged
row to the next layer's representative row, which is what the scalar G stands for.  tests/test_avit_packed_train_host.py proves that backward, G
included, against dense fp64 autograd to 1e-12."""
import copy
import math

import pytest
import torch

import avit_packed_train_ref as pref
import avit_train_ref as ref
import test_hip_avit_train as dense_t
from conftest import rel_l2

pytestmark = pytest.mark.gpu

THR, U, GS, GC = dense_t.THR, dense_t.U, dense_t.GS, dense_t.GC
_dev = dense_t._dev
_h_err = dense_t._h_err

# ---- the pack step ---------------------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = [(3, 17, 128, 1), (2, 20, 128, 2), (1, 17, 128, 1), (2, 208, 384, 1)]
# what each image's input segment looks like: "norep" every token still runs (no representative row), "mixed" running tokens and a representative,
# "onlyrep" the segment is the representative row alone, "haltall" every running token halts at this step (with or without a representative before)
KINDS = {(3, 17): ["norep", "onlyrep", "haltall_rep"], (2, 20): ["mixed", "onlyrep"], (1, 17): ["haltall_norep"], (2, 208): ["norep", "haltall_rep"]}


def _pack_inputs(B, S, D, n_cls, last, seed):
    """fp32 inputs of one packed step (CPU): (y [R, D], seg, nh, pos, (c, R, rho, counter, m), acc).  Channel 0 of every row puts the gate's argument
    in [-4, 4]; c of a running token is built from the fp64 h so that c' lies in [0.2, 0.98] or [1.0, 1.8] - at least 1e-3 from the threshold, so
    fp32 and fp64 decide alike; a halted token has c = 1.5."""
    g = torch.Generator().manual_seed(seed)
    kinds = KINDS[(B, S)]
    m = torch.zeros(B, S)
    for b, k in enumerate(kinds):
        if k in ("norep", "haltall_norep"):
            m[b] = 1
        elif k in ("mixed", "haltall_rep"):
            m[b] = (torch.rand(S, generator=g) < 0.7).float()
            m[b, 0], m[b, S - 1] = 1, 0          # the class token runs, at least one token is halted
    yd = torch.randn(B, S, D, generator=g)
    yd[:, :, 0] = (torch.rand(B, S, generator=g) * 8 - 4 + GC) / GS
    h = torch.sigmoid(yd[:, :, 0].double() * GS - GC)
    hh = torch.ones_like(h) if last else h
    below = torch.rand(B, S, generator=g) < 0.6
    for b, k in enumerate(kinds):
        if k.startswith("haltall"):
            below[b] = False
    target = torch.where(below, 0.2 + 0.78 * torch.rand(B, S, generator=g), 1.0 + 0.8 * torch.rand(B, S, generator=g)).double()
    c = torch.where(m == 1, (target - hh).float(), torch.full((B, S), 1.5))
    assert (((c.double() + hh) - THR).abs() > 1e-3)[m == 1].all()
    R, rho = torch.rand(B, S, generator=g), torch.rand(B, S, generator=g) * 3
    counter = torch.randint(1, 6, (B, S), generator=g).float()
    acc = torch.randn(B, n_cls, D, generator=g)
    rows, pos, seg, nh = [], [], [0], []
    for b in range(B):
        live = [t for t in range(S) if m[b, t] == 1]
        rows += [yd[b, t] for t in live]
        pos += live
        if len(live) < S:
            rows.append(yd[b, [t for t in range(S) if m[b, t] == 0][0]])
            pos.append(-1)
        nh.append(S - len(live))
        seg.append(len(pos))
    return torch.stack(rows), torch.tensor(seg, dtype=torch.int32), torch.tensor(nh, dtype=torch.int32), torch.tensor(pos, dtype=torch.int32), \
        (c, R, rho, counter, m), acc


def _run_fwd(step, y, seg, nh, pos, state, acc, last, dev):
    out = step(y.to(dev), seg.to(dev), nh.to(dev), pos.to(dev), *(t.to(dev) for t in state), acc.to(dev), GS, GC, THR, bool(last))
    torch.cuda.synchronize()
    return out


def _flat(out):
    st, acc1, h_part, sv, ycls, nxt = out
    ts = [*st, acc1, h_part, sv, ycls]
    if nxt is not None:
        r_next = int(nxt[6][0])
        ts += [nxt[0][:r_next], nxt[1][:r_next], nxt[2], nxt[3], nxt[4][:r_next], nxt[5][:r_next], nxt[6], nxt[7][:r_next]]
    return [t.cpu() for t in ts]


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("B,S,D,n_cls", STEP_SHAPES)
def test_pack_step_forward_against_fp64(B, S, D, n_cls, last):
    """pv_avit_pack_step_train (ops.avit_pack_step_train): counter', m', the flags, every integer table, totals, the zero rows and the copied rows exact;
    every other output within a bound made of the kernel's own operations (U = 2^-24 per fp32 operation, tests/test_hip_avit_train.py's bounds for the
    shared arithmetic); two runs bit-identical."""
    from peekvit_amd import ops
    dev = _dev()
    y, seg, nh, pos, state, acc = _pack_inputs(B, S, D, n_cls, last, seed=B * 1000 + S + last)
    c, R, rho, counter, m = state
    st64 = pref.pack_step_fwd(y.double(), seg, nh, pos, tuple(t.double() for t in state), acc.double(), GS, GC, THR, bool(last))
    out = _run_fwd(ops.avit_pack_step_train, y, seg, nh, pos, state, acc, last, dev)
    again = _run_fwd(ops.avit_pack_step_train, y, seg, nh, pos, state, acc, last, dev)
    assert all(torch.equal(a, b) for a, b in zip(_flat(out), _flat(again))), "two runs differ"
    (c1, R1, rho1, cnt1, m1), acc1, h_part, sv, ycls, nxt = out
    c1, R1, rho1, cnt1, m1, acc1, h_part, sv, ycls = (t.cpu() for t in (c1, R1, rho1, cnt1, m1, acc1, h_part, sv, ycls))
    c64, R64, rho64, cnt64, m64 = st64["state"]
    assert torch.equal(cnt1.double(), cnt64) and torch.equal(m1.double(), m64)
    assert torch.equal(sv[2].double(), st64["sv"][2]), "flags"
    gone = m == 0          # a token without a row: its state is carried over bit for bit
    for got, src in ((c1, c), (R1, R), (rho1, rho), (cnt1, counter)):
        assert torch.equal(got[gone], src[gone])
    live = pos >= 0
    img = pref._row_image(seg.long(), y.shape[0])
    lb, lp = img[live], pos[live].long()
    h64 = st64["sv"][0]
    h_err = _h_err(y[:, 0].double(), h64)
    assert ((sv[0].double() - h64).abs() <= h_err).all()
    hh_err = torch.zeros_like(h_err) if last else h_err
    assert ((c1[lb, lp].double() - c64[lb, lp]).abs() <= hh_err[live] + 2 * U * c64[lb, lp].abs()).all()
    assert ((R1[lb, lp].double() - R64[lb, lp]).abs() <= hh_err[live] + 2 * U * (R[lb, lp].double().abs() + 1)).all()
    assert ((rho1.double() - rho64).abs() <= 4 * U * rho64.abs()).all()
    w64 = st64["sv"][1]
    w_err = hh_err + 4 * U * w64.abs()
    assert ((sv[1].double() - w64).abs() <= w_err).all() and torch.equal(sv[1][~live], torch.zeros(int((~live).sum())))
    # class rows: acc' = acc + y * w, and ycls = the row as read (zeros without a row)
    w_cls, werr_cls, y_cls = torch.zeros(B, n_cls, dtype=torch.float64), torch.zeros(B, n_cls, dtype=torch.float64), torch.zeros(B, n_cls, D)
    is_cls = live & (pos < n_cls)
    w_cls[img[is_cls], pos[is_cls].long()], werr_cls[img[is_cls], pos[is_cls].long()] = w64[is_cls], w_err[is_cls]
    y_cls[img[is_cls], pos[is_cls].long()] = y[is_cls]
    assert torch.equal(ycls, y_cls)
    acc_tol = y_cls.double().abs() * werr_cls[:, :, None] + 3 * U * (acc.double().abs() + (y_cls.double() * w_cls[:, :, None]).abs())
    assert ((acc1.double() - st64["acc"]).abs() <= acc_tol + 1e-30).all()
    no_cls_row = w_cls.new_ones(B, n_cls).bool()
    no_cls_row[img[is_cls], pos[is_cls].long()] = False
    assert torch.equal(acc1[no_cls_row], acc[no_cls_row])
    # the image's h sum: at most S + 2 roundings of partial sums no larger than the sum, on top of the terms' own errors (the representative's n times)
    term = torch.where(live, h64, h64 * nh.double()[img])
    term_err = torch.where(live, h_err, (h_err + U * h64) * nh.double()[img])
    hsum_tol = torch.zeros(B, dtype=torch.float64).index_add_(0, img, term_err) + (S + 2) * U * torch.zeros(B, dtype=torch.float64).index_add_(0, img, term)
    assert ((h_part.double() - st64["h_part"]).abs() <= hsum_tol).all(), (h_part, st64["h_part"], hsum_tol)
    if last:
        assert nxt is None
        return
    x_next, rs_next, seg_next, nh_next, lm_next, pos_next, totals, src_next = (t.cpu() for t in nxt)
    r_next, longest = totals.tolist()
    assert (r_next, longest) == st64["totals"]
    assert torch.equal(seg_next.long(), st64["seg_next"]) and torch.equal(nh_next.long(), st64["nh_next"])
    assert torch.equal(pos_next[:r_next].long(), st64["pos_next"]) and torch.equal(src_next[:r_next].long(), st64["src_next"])
    assert torch.equal(rs_next[:r_next].double(), st64["rs_next"])
    assert torch.equal(x_next[:r_next].double(), st64["x_next"]), "copied rows / zero rows"
    lm64 = st64["lm_next"]
    assert torch.equal(lm_next[:r_next][lm64 == 0], torch.zeros(int((lm64 == 0).sum())))
    assert ((lm_next[:r_next].double() - lm64).abs() <= 4 * U * lm64.abs()).all()          # logf: 2 ulp allowed on top of the rounding of n
    kinds = KINDS[(B, S)]
    for b, k in enumerate(kinds):          # the cases the shapes were chosen for
        n_rows = int(seg_next[b + 1] - seg_next[b])
        if k in ("onlyrep", "haltall_rep", "haltall_norep"):
            assert n_rows == 1 and int(nh_next[b]) == S and int(pos_next[int(seg_next[b])]) == -1
        else:
            assert n_rows > 1


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("B,S,D,n_cls", STEP_SHAPES)
def test_pack_step_backward_against_fp64(B, S, D, n_cls, last):
    """pv_avit_pack_step_bwd (ops.avit_pack_step_bwd) on the forward kernel's own saved tables, with random gradients on every differentiable output and
    a random running G, against the fp64 restatement: a surviving row outside channel 0 and the class rows is its next-row gradient bit for bit, a
    merged row is G e_0 plus the step's own channel-0 term, the representative row n G_new e_0, and G is updated; the 16-bit copy is the rounded dy
    in both operand builds."""
    from peekvit_amd import _lib, engine, ops
    dev = _dev()
    y, seg, nh, pos, state, acc = _pack_inputs(B, S, D, n_cls, last, seed=B * 2000 + S + last)
    c, R, rho, counter, m = state
    st64 = pref.pack_step_fwd(y.double(), seg, nh, pos, tuple(t.double() for t in state), acc.double(), GS, GC, THR, bool(last))
    (_, _, _, _, _), _, _, sv, ycls, nxt = _run_fwd(ops.avit_pack_step_train, y, seg, nh, pos, state, acc, last, dev)
    g = torch.Generator().manual_seed(7 + S)
    r_next = 0 if last else st64["totals"][0]
    g_next = None if last else torch.randn(r_next, D, generator=g)
    gR, grho, gacc, gh, G = (torch.randn(B, S, generator=g), torch.randn(B, S, generator=g), torch.randn(B, n_cls, D, generator=g),
                             torch.randn(1, generator=g) * 50, torch.randn(B, generator=g))
    dy64, dR64, G64 = pref.pack_step_bwd(st64, None if last else g_next.double(), gR.double(), grho.double(), gacc.double(),
                                         gh.double()[0] if B > 1 else None, G.double())
    res = {}
    for mode in ("bf16", "f16"):
        with engine.precision(mode):
            Gd = G.to(dev).clone()
            dy, dy16, dR = ops.avit_pack_step_bwd(None if last else g_next.to(dev), seg.to(dev), nh.to(dev), pos.to(dev), None if last else nxt[2],
                                                  None if last else nxt[7], sv, ycls, gR.to(dev), grho.to(dev), gacc.to(dev),
                                                  gh.to(dev) if B > 1 else None, Gd, D, GS, bool(last))
            torch.cuda.synchronize()
            assert dy16.dtype == _lib.operand_dtype() and torch.equal(dy16, dy.to(dy16.dtype)), f"{mode}: dy16 is not the rounded dy"
        res[mode] = (dy.cpu(), dR.cpu(), Gd.cpu())
    assert all(torch.equal(a, b) for a, b in zip(res["bf16"], res["f16"]))
    dy, dR, G1 = res["bf16"]
    live = pos >= 0
    img = pref._row_image(seg.long(), y.shape[0])
    fl = st64["sv"][2].long()
    merged = (fl & pref.MERGED) != 0
    h64, w64 = st64["sv"][0], st64["sv"][1]
    h_err = _h_err(y[:, 0].double(), h64)
    gate = GS * h64 * (1 - h64)
    gate_err = GS * ((1 - 2 * h64).abs() * h_err + 3 * U * h64 * (1 - h64))
    coef = torch.zeros(B, dtype=torch.float64)
    if B > 1:
        coef[1:] = gh.double().abs() / ((B - 1) * S)
    # exact parts
    plain = torch.ones(y.shape[0], D, dtype=torch.bool)
    plain[:, 0] = False
    plain[live & (pos < n_cls)] = False
    if not last:
        src = st64["src_next"]
        for b in range(B):
            d0, d1, s0 = int(st64["seg_next"][b]), int(st64["seg_next"][b + 1]), int(seg[b])
            for j in range(d0, d1):
                if int(src[j]) >= 0:
                    r = s0 + int(src[j])
                    assert torch.equal(dy[r][plain[r]], g_next[j][plain[r]])
        assert merged.sum() > 0 and (dy[merged][plain[merged]] == 0).all()
    else:
        assert (dy[plain] == 0).all()
    assert (dy[~live][:, 1:] == 0).all()
    # G and the representative rows
    rep_b = img[~live]
    G_tol = torch.zeros(B, dtype=torch.float64)
    G_tol[rep_b] = gate_err[~live] * coef[rep_b] + 4 * U * (G.double().abs()[rep_b] + coef[rep_b] * gate[~live])
    assert ((G1.double() - G64).abs() <= G_tol).all() and torch.equal(G1[G_tol == 0], G[G_tol == 0])
    n = nh.double()[rep_b]
    assert ((dy[~live][:, 0].double() - dy64[~live][:, 0]).abs() <= n * G_tol[rep_b] + 2 * U * dy64[~live][:, 0].abs()).all()
    if B > 1:
        assert (dy64[~live][img[~live] >= 1][:, 0] != 0).all() or (~live).sum() == 0
    # live rows: pv_avit_act_bwd's bounds (tests/test_hip_avit_train.py) with m = 1, plus the pass-through G on a merged row
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


# ---- the block -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halt", ["none", "some", "all_but_class"])
@pytest.mark.parametrize("B,S,D,H", [(2, 17, 128, 2), (2, 197, 192, 3)])
def test_packed_avit_block_against_fp64_on_expanded_rows(B, S, D, H, halt):
    """train_engine.avit_packed_block_forward_train (bf16 operands, as every block function called on its own) against the fp64 block on the expanded dense rows:
    the output of every packed row - the representative's is what every halted token of its image leaves as - dx of the live rows and all twelve
    parameter gradients.  A halted token's output gradient is a e_0, the representative's n a e_0 (non-zero on channel 0 only).  Bounds:
    tests/test_hip_avit_train.py's for the dense block (1.2e-2 per forward row, 3e-2 relative for gradients)."""
    from peekvit_amd import ops, train_engine
    dev = _dev()
    blk = dense_t._micro_block(D, H, dev, seed=S)
    blk64 = copy.deepcopy(blk).double()
    blk = blk.to(dev)
    g = torch.Generator().manual_seed(S + D)
    m = torch.ones(B, S)
    if halt == "some":
        m = (torch.rand(B, S, generator=g) < 0.6).float()
        m[:, 0], m[:, S - 1] = 1, 0
    elif halt == "all_but_class":
        m[:, 1:] = 0
    x = (torch.randn(B, S, D, generator=g) * m[:, :, None]).to(torch.bfloat16).float()
    dout = torch.randn(B, S, D, generator=g)
    a = torch.randn(B, generator=g)
    for b in range(B):
        dout[b, m[b] == 0] = 0
        dout[b, m[b] == 0, 0] = a[b]
    x64 = x.double().requires_grad_(True)
    out64 = ref.block(blk64, x64, m.double())
    out64.backward(dout.double())
    rows, drows, rs, lm, seg, src = [], [], [], [], [0], []
    for b in range(B):
        live = [t for t in range(S) if m[b, t] == 1]
        rows += [x[b, t] for t in live]
        drows += [dout[b, t] for t in live]
        src += [(b, t) for t in live]
        rs += [1.0] * len(live)
        lm += [0.0] * len(live)
        n = S - len(live)
        if n:
            e0 = torch.zeros(D)
            e0[0] = n * a[b]
            rows.append(torch.zeros(D)); drows.append(e0); rs.append(0.0); lm.append(math.log(n))
            src.append((b, [t for t in range(S) if m[b, t] == 0][0]))
        seg.append(len(rows))
    xp = torch.stack(rows).to(dev).requires_grad_(True)
    max_len = max(seg[i + 1] - seg[i] for i in range(B))
    n0 = ops.launch_count
    out = train_engine.avit_packed_block_forward_train(blk, xp, torch.tensor(rs, device=dev), torch.tensor(seg, dtype=torch.int32, device=dev),
                                                       torch.tensor(lm, device=dev), max_len)
    out.backward(torch.stack(drows).to(dev))
    torch.cuda.synchronize()
    assert ops.launch_count - n0 > 20, "the HIP block did not run"
    assert out.shape[0] == len(rows) and (halt == "none") == (len(rows) == B * S)
    bi, ti = torch.tensor([s[0] for s in src]), torch.tensor([s[1] for s in src])
    o, o64 = out.detach().cpu().double(), out64.detach()[bi, ti]
    row_err = (o - o64).norm(dim=-1) / o64.norm(dim=-1)
    assert row_err.max() < 1.2e-2, (float(row_err.max()), int(row_err.argmax()))
    is_live = torch.tensor(rs) == 1
    assert rel_l2(xp.grad.cpu()[is_live], x64.grad[bi, ti][is_live]) < 3e-2
    for (n_, p), (_, p64) in zip(blk.named_parameters(), blk64.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), n_
        assert rel_l2(p.grad, p64.grad) < 3e-2, (n_, rel_l2(p.grad, p64.grad))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
CEILING = dense_t.CEILING


def packed_case(name, mode, kind, seed):
    """dense_t.fused_case with the packed switch: one packed training step of loss `kind` in precision mode `mode` and its fp64 replay."""
    from peekvit_amd import engine, train_engine
    dev = _dev()
    x, labels = dense_t._batch(name, seed)
    model = dense_t._model(name, dev)
    model.set_packed_training(True)
    rows0, dense0 = engine.avit_train_rows, engine.avit_train_dense_rows
    with engine.precision(mode):
        logits = model(x.to(dev))
        enc = model.encoder
        loss = ref.loss_terms(kind, logits, labels.to(dev), enc.rho_token, enc.halting_score_layer)
        loss.backward()
        skipped, operand = train_engine.last_step_skipped(model), train_engine.pass_operand(model)
    assert engine.avit_train_dense_rows - dense0 == len(enc.layers) * x.shape[0] * model.seq_length, "the packed pass did not run"
    counter = enc.counter_token.detach().cpu()
    m64 = dense_t._model(name).double()
    lg64, rho64, sc64, cnt64, _ = ref.model_forward(m64, x, counter=counter)
    assert torch.equal(cnt64, counter.double())
    loss64 = ref.loss_terms(kind, lg64, labels, rho64, sc64)
    loss64.backward()
    gp = dict(model.named_parameters())
    names = [n for n, p in m64.named_parameters() if p.grad is not None]
    missing = [n for n in names if gp[n].grad is None]
    assert not missing, missing
    got = torch.cat([gp[n].grad.detach().cpu().double().reshape(-1) for n in names])
    want = torch.cat([p.grad.reshape(-1) for n, p in m64.named_parameters() if p.grad is not None])
    return {"logits": rel_l2(logits, lg64), "rho": rel_l2(enc.rho_token, rho64), "scores": rel_l2(torch.stack(enc.halting_score_layer), torch.stack(sc64)),
            "loss": float(loss.detach()), "loss64": float(loss64.detach()), "grad": float((got - want).norm() / max(float(want.norm()), 1e-30)),
            "finite": bool(torch.isfinite(got).all()), "skipped": skipped, "operand": operand,
            "row_share": (engine.avit_train_rows - rows0) / (engine.avit_train_dense_rows - dense0),
            "flipped": float((counter.double() != dense_t._free_running(name, seed)).double().mean())}


@pytest.mark.parametrize("kind", ["ce", "ponder", "prior", "yaml"])
@pytest.mark.parametrize("mode", ["auto", "bf16"])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name", ["avit_micro", "avit_cls2_reg2"])
def test_packed_training_step_against_fp64_replay_and_the_dense_fused_path(name, seed, mode, kind):
    """The packed step against the fp64 composite replaying the packed pass's own decisions, and the dense fused path on the same case against its
    replay: every packed error at most 1.5 x the dense one + 1e-4 (room for the ragged attention's different rounding, not for another error
    source), the complete gradient under the file's ceiling 1e-2, and at most 3 % of the tokens deciding differently from the free-running fp64
    composite (the replay must not hide a broken halting kernel).  The loss value: tests/test_hip_avit_train.py's bound for the dense path."""
    p = packed_case(name, mode, kind, seed)
    d = dense_t.fused_case(name, mode, kind, seed)
    print(name, seed, mode, kind, "packed", p, "dense", {k: d[k] for k in ("logits", "rho", "scores", "grad", "flipped")})
    assert p["finite"] and not p["skipped"] and p["operand"] == ("f16" if mode == "auto" else "bf16")
    assert p["flipped"] <= 0.03, p["flipped"]
    for what in ("logits", "rho", "scores", "grad"):
        assert p[what] <= 1.5 * d[what] + 1e-4, (what, p[what], d[what])
    assert p["grad"] < CEILING, p["grad"]
    # (the loss value is one signed number: the dense path's error in it can cancel to nearly nothing, so a ratio to it says nothing.  It is held to
    # the bound the dense fused path's own test holds its loss value to.)
    assert abs(p["loss"] - p["loss64"]) < dense_t._bound(mode, "loss") * abs(p["loss64"]), (p["loss"], p["loss64"])


def test_every_token_halting_after_the_first_layer_packed():
    """avit_allhalt: every token halts after layer 1, so layers 2.. run on one representative row per image."""
    p = packed_case("avit_allhalt", "auto", "yaml", 0)
    d = dense_t.fused_case("avit_allhalt", "auto", "yaml", 0)
    print(p, d)
    assert p["finite"] and not p["skipped"] and p["flipped"] == 0.0 and p["row_share"] < 0.5
    assert p["logits"] <= 1.5 * d["logits"] + 1e-4 and p["grad"] <= 1.5 * d["grad"] + 1e-4 and p["grad"] < CEILING, (p, d)


def _yaml_step(model, x, labels):
    loss = ref.loss_terms("yaml", model(x), labels, model.encoder.rho_token, model.encoder.halting_score_layer)
    loss.backward()
    return loss


def test_packed_pass_launches_the_pack_step_once_per_layer_and_reads_the_host_once_per_layer():
    """ops.KernelTimer around a packed forward + backward: pv_avit_pack_step_train and pv_avit_pack_step_bwd once per layer, the ragged attention pair
    once per layer, none of the dense halting kernels; one host read of the next row count behind every layer that has a next one."""
    from peekvit_amd import engine, ops
    dev = _dev()
    x, labels = dense_t._batch("avit_micro", 0)
    x, labels = x.to(dev), labels.to(dev)
    model = dense_t._model("avit_micro", dev)
    L = len(model.encoder.layers)
    model.set_fused_training(True)
    with ops.KernelTimer() as kt:
        _yaml_step(model, x, labels)
    torch.cuda.synchronize()
    assert "pv_avit_pack_step_train" not in kt.summary() and "pv_avit_pack_step_bwd" not in kt.summary()          # switch off
    model.set_packed_training(True)
    syncs0 = engine.avit_train_syncs
    with ops.KernelTimer() as kt:
        _yaml_step(model, x, labels)
    torch.cuda.synchronize()
    s = {k: v["launches"] for k, v in kt.summary().items()}
    assert s["pv_avit_pack_step_train"] == L and s["pv_avit_pack_step_bwd"] == L, s
    assert s["pv_attention_varlen_w_lse_bf16"] == L and s["pv_attention_varlen_w_bwd16_bf16"] == L, s
    assert "pv_avit_act_fwd" not in s and "pv_avit_act_bwd" not in s and "pv_attention_bf16" not in s, s
    assert engine.avit_train_syncs - syncs0 == L - 1          # the last layer has no next input to size
    rows = engine.avit_train_last_rows
    assert len(rows) == L and rows[0] == x.shape[0] * model.seq_length and all(a >= b for a, b in zip(rows, rows[1:]))


def test_packed_switch_off_is_bit_identical_to_a_model_that_never_had_it():
    dev = _dev()
    x, labels = dense_t._batch("avit_micro", 0)
    x, labels = x.to(dev), labels.to(dev)
    for fused in (False, True):
        a, b = dense_t._model("avit_micro", dev), dense_t._model("avit_micro", dev)
        a.set_fused_training(fused); b.set_fused_training(fused)
        a.set_packed_training(True)
        _yaml_step(a, x, labels)                          # the packed pass leaves its state behind ...
        a.zero_grad(set_to_none=True)
        a.set_packed_training(False)                      # ... and the switch goes off again
        la, lb = _yaml_step(a, x, labels), _yaml_step(b, x, labels)
        assert torch.equal(la, lb), fused
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(p.grad, q.grad), (fused, n)
        assert torch.equal(a.encoder.rho_token, b.encoder.rho_token) and torch.equal(a.encoder.counter_token, b.encoder.counter_token)


def test_two_packed_optimizer_steps_under_the_fp16_loss_scale():
    from peekvit_amd import train_engine
    dev = _dev()
    x, labels = dense_t._batch("avit_micro", 0)
    model = dense_t._model("avit_micro", dev)
    model.set_packed_training(True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    before = model.encoder.layers[0].mlp.fc1.weight.detach().clone()
    for _ in range(2):
        opt.zero_grad()
        loss = _yaml_step(model, x.to(dev), labels.to(dev))
        opt.step()
        assert train_engine.pass_operand(model) == "f16" and not train_engine.last_step_skipped(model)
        assert torch.isfinite(loss)
    assert train_engine.train_state(model).scale > 1.0
    assert not torch.equal(before, model.encoder.layers[0].mlp.fc1.weight)
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_an_overflowing_packed_step_is_dropped_like_the_dense_fused_one():
    """Inputs scaled beyond fp16's range in the fp16 pass: the step is dropped - every .grad is None and last_step_skipped is true - on the packed
    path exactly as on the dense fused one."""
    import warnings
    from peekvit_amd import engine, train_engine
    dev = _dev()
    x, labels = dense_t._batch("avit_micro", 0)
    xg, yg = (x * 1.0e6).to(dev), labels.to(dev)
    with engine.precision("auto"):
        for packed in (False, True):
            m = dense_t._model("avit_micro", dev)
            m.set_fused_training(True)
            m.set_packed_training(packed)
            assert train_engine.pass_operand(m) == "f16"
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                torch.nn.functional.cross_entropy(m(xg), yg).backward()
                assert train_engine.last_step_skipped(m), packed
            assert all(p.grad is None for p in m.parameters()), packed


def test_an_ineligible_model_falls_back_to_the_fused_dense_path_or_the_composite():
    """Head dim 32 (the ragged attention kernels need 64): with the packed switch on, the forward takes the fused dense path when that switch is on
    too - bit for bit that path's result - and the composite otherwise."""
    from peekvit_amd import engine, ops
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    dev = _dev()
    kw = dict(dense_t.META["cases"]["avit_micro"]["kwargs"])
    kw["num_heads"] = kw["hidden_dim"] // 32
    torch.manual_seed(0)
    base = AdaptiveVisionTransformer(**kw).train()
    torch.nn.init.normal_(base.head.weight, std=0.02)
    x, labels = dense_t._batch("avit_micro", 0)
    x, labels = x.to(dev), labels.to(dev)

    def run(fused, packed):
        m = copy.deepcopy(base).to(dev)
        m.set_fused_training(fused)
        m.set_packed_training(packed)
        assert not m._packed_training_ok()
        dense0 = engine.avit_train_dense_rows
        with ops.KernelTimer() as kt:
            logits = m(x)
            torch.nn.functional.cross_entropy(logits, labels).backward()
        torch.cuda.synchronize()
        assert engine.avit_train_dense_rows == dense0 and "pv_avit_pack_step_train" not in kt.summary()
        return logits.detach(), [p.grad for p in m.parameters()], kt.summary()

    for fused in (True, False):
        la, ga, sa = run(fused, True)
        lb, gb, _ = run(fused, False)
        assert ("pv_avit_act_fwd" in sa) == fused
        assert torch.equal(la, lb) and all(torch.equal(p, q) for p, q in zip(ga, gb)), fused
