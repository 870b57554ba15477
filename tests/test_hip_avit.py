"""A-ViT packed halting on the MI355X: the ragged attention (pv_attention_varlen_bf16) against fp64, the halting step (pv_act_step) against a
torch restatement of models/adavit.py:180-217, and the model forward against the reference's golden outputs and the stock-op composite."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from peekvit_amd import synth

pytestmark = pytest.mark.gpu

META = json.load(open(os.path.join(GOLDEN, "avit_meta.json")))
THR = float(torch.tensor(1 - 0.01, dtype=torch.float32))
DELTA = 2e-3        # a token whose running sum c stays this far from 1 - eps at every layer it runs must halt where the reference halts


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _model(name, dev=None, **over):
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    case = META["cases"][name]
    model = AdaptiveVisionTransformer(**dict(case["kwargs"], **over)).eval()
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(case["synth_cfg"], seed=0).items()}
    model.load_state_dict(sd, strict=True)
    return model.to(dev) if dev is not None else model


def _images(name, g=None, batch=None, seed=0):
    case = META["cases"][name]
    if g is not None and "images" in g and batch is None:
        return torch.from_numpy(g["images"])
    return torch.from_numpy(synth.synth_images(batch or case["batch"], case["kwargs"]["image_size"], seed=seed, name="avit"))


# ---- ragged attention -----------------------------------------------------------------------------------------------------
LENS = [1, 2, 15, 16, 17, 197, 208]
HALTED = [0, 3, 0, 7, 1, 0, 0]


def _packed_qkv(lens, H, dh, seed, dtype, dev):
    g = torch.Generator().manual_seed(seed)
    R, D = sum(lens), H * dh
    qkv = torch.randn(R, 3 * D, generator=g)
    qkv[:, :D] *= dh ** -0.5
    return qkv.to(dtype).to(dev)


def _attention_fp64(qkv, lens, nh, H, dh):
    """Dense softmax attention per image in fp64, the last key of an image with nh > 0 repeated nh times."""
    q64 = qkv.double().cpu()
    D = H * dh
    out = torch.zeros(q64.shape[0], D, dtype=torch.float64)
    s0 = 0
    for L, n in zip(lens, nh):
        seg = q64[s0:s0 + L]
        k, v = seg[:, D:2 * D], seg[:, 2 * D:]
        if n > 0:
            k = torch.cat([k, k[-1:].expand(n - 1, -1)])
            v = torch.cat([v, v[-1:].expand(n - 1, -1)])
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            p = torch.softmax(seg[:, sl] @ k[:, sl].T, dim=-1)
            out[s0:s0 + L, sl] = p @ v[:, sl]
        s0 += L
    return out


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_varlen_attention_against_fp64(mode):
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    H, dh = 3, 64
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv = _packed_qkv(LENS, H, dh, 0, dt, dev)
        seg = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int32, device=dev)
        nh = torch.tensor(HALTED, dtype=torch.int32, device=dev)
        out = torch.full((sum(LENS), H * dh), float("nan"), dtype=dt, device=dev)
        ops.attention_varlen(qkv, out, seg, nh, max(LENS), H, dh)
        torch.cuda.synchronize()
    ref = _attention_fp64(qkv, LENS, HALTED, H, dh)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    tol = 1.5e-2 if mode == "bf16" else 2e-3
    err = (got - ref).abs().max().item()
    assert err < tol, f"{mode}: max |err| {err:.3g} vs fp64"
    # the tile bound follows the longest segment: the first five images alone (17 rows at most, two key tiles) give the same rows
    with engine.precision(mode):
        out2 = torch.empty((sum(LENS[:5]), H * dh), dtype=dt, device=dev)
        ops.attention_varlen(qkv[:sum(LENS[:5])].contiguous(), out2, seg[:6].contiguous(), nh[:5].contiguous(), max(LENS[:5]), H, dh)
        torch.cuda.synchronize()
    assert torch.equal(out2, out[:sum(LENS[:5])])


@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_varlen_multiplicity_equals_repeated_keys(mode):
    """A representative key counted n times == dense attention over a segment in which that row really occurs n times."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    H, dh = 2, 64
    live, n = [15, 40, 100, 1], [5, 1, 90, 200]
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        packed_lens = [l + 1 for l in live]
        qkv = _packed_qkv(packed_lens, H, dh, 1, dt, dev)
        seg = torch.tensor(np.concatenate([[0], np.cumsum(packed_lens)]), dtype=torch.int32, device=dev)
        out = torch.empty((sum(packed_lens), H * dh), dtype=dt, device=dev)
        ops.attention_varlen(qkv, out, seg, torch.tensor(n, dtype=torch.int32, device=dev), max(packed_lens), H, dh)
        # dense: every representative row physically repeated n times, no multiplicity
        rows, s0 = [], 0
        for L in packed_lens:
            rows.append(qkv[s0:s0 + L])
            s0 += L
        dense = [torch.cat([r[:-1], r[-1:].expand(k, -1)]) for r, k in zip(rows, n)]
        dlens = [d.shape[0] for d in dense]
        dqkv = torch.cat(dense).contiguous()
        dseg = torch.tensor(np.concatenate([[0], np.cumsum(dlens)]), dtype=torch.int32, device=dev)
        dout = torch.empty((sum(dlens), H * dh), dtype=dt, device=dev)
        ops.attention_varlen(dqkv, dout, dseg, torch.zeros(len(n), dtype=torch.int32, device=dev), max(dlens), H, dh)
        torch.cuda.synchronize()
    s0 = d0 = 0
    tol = 3.2e-2 if mode == "bf16" else 2e-3           # two 16-bit ulps at |out| ~ 2: the two launches sum the same terms in another order
    for L, k in zip(packed_lens, n):
        a = out[s0:s0 + L].double()
        b = torch.cat([dout[d0:d0 + L - 1], dout[d0 + L - 1 + k - 1:d0 + L - 1 + k]]).double()      # live rows + one copy of the representative
        assert (a - b).abs().max().item() < tol
        s0 += L
        d0 += L - 1 + k


# ---- halting step -----------------------------------------------------------------------------------------------------------
def _act_reference(y_full, c, Rr, rho, counter, mask, acc, gs, gc, last, nc):
    """models/adavit.py:180-217 for one layer on the full [B,S] token grid (y_full: the block output of every token)."""
    h = torch.sigmoid(y_full[:, :, 0] * gs - gc)
    he = torch.ones_like(h) if last else h
    m = mask
    c = c + he
    rho = rho + m
    reached = (c > 1 - 0.01).float() * m
    delta1 = y_full * m[..., None] * Rr[..., None] * reached[..., None]
    rho = rho + Rr * reached
    notr = (c < 1 - 0.01).float()
    Rr = Rr - notr * he
    delta2 = y_full * m[..., None] * he[..., None] * notr[..., None]
    counter = counter + notr
    mask = (c < 1 - 0.01).float()
    acc = acc + (delta1 + delta2)[:, :nc]
    return c, Rr, rho, counter, mask, acc, h


def test_act_step_against_torch_restatement():
    from peekvit_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    B, S, D, nc, gs, gc = 6, 40, 128, 2, 10.0, 2.0
    mask = (torch.rand(B, S, generator=g) < 0.7).float()
    mask[0] = 1.0                                      # an image without halted tokens
    mask[1] = 0.0                                      # an image whose tokens have all halted
    mask[1, 0] = 1.0
    c = torch.rand(B, S, generator=g) * 0.9 * mask + (1 - mask) * 1.2
    Rr = 1 - c * mask
    rho = torch.randint(0, 4, (B, S), generator=g).float()
    counter = torch.randint(1, 4, (B, S), generator=g).float()
    acc = torch.randn(B, nc, D, generator=g)
    y_full = torch.randn(B, S, D, generator=g) * 0.3
    # one representative row per image with halted tokens: every halted token of the image gets ITS block output
    rep = torch.randn(B, D, generator=g) * 0.3
    y_full = torch.where(mask[..., None] > 0, y_full, rep[:, None, :])
    rows, pos, seg, nh = [], [], [0], []
    for b in range(B):
        live = torch.nonzero(mask[b]).flatten().tolist()
        rows += [y_full[b, t] for t in live]
        pos += live
        n = S - len(live)
        if n:
            rows.append(rep[b])
            pos.append(-1)
        nh.append(n)
        seg.append(len(pos))
    y = torch.stack(rows)
    for last in (False, True):
        st = [t.clone().to(dev) for t in (c, Rr, rho, counter, mask)]
        acc_d, hp = acc.clone().to(dev), torch.zeros(B, device=dev)
        R = y.shape[0]
        nxt = (torch.full((R, D), float("nan"), device=dev), torch.full((R,), -1.0, device=dev), torch.zeros(B + 1, dtype=torch.int32, device=dev),
               torch.zeros(B, dtype=torch.int32, device=dev), torch.full((R,), -7, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        ops.act_step(y.to(dev), i32(seg), i32(nh), i32(pos), st, acc_d, hp, gs, gc, THR, last, None if last else nxt)
        torch.cuda.synchronize()
        rc, rR, rrho, rcnt, rmask, racc, h = _act_reference(y_full, c, Rr, rho, counter, mask, acc, gs, gc, last, nc)
        live = mask > 0
        got = [t.cpu() for t in st]
        assert torch.equal(got[4][live], rmask[live]) and torch.equal(got[3][live], rcnt[live])          # masks, counter: bit-exact
        assert torch.equal(got[4][~live], mask[~live]) and torch.equal(got[3][~live], counter[~live])   # halted tokens untouched
        for a, b_ in ((got[0], rc), (got[1], rR), (got[2], rrho)):
            assert torch.allclose(a[live], b_[live], rtol=1e-6, atol=1e-6)
        assert torch.allclose(acc_d.cpu(), racc, rtol=1e-6, atol=1e-6)
        assert torch.allclose(hp.cpu(), h.sum(dim=1), rtol=1e-5, atol=1e-5)
        if last:
            continue
        # next packed input: survivors in order, then one zero representative row where anything has halted
        xs, rs, sg, nhn, ps, tot = [t.cpu() for t in nxt]
        new_mask = rmask
        exp_rows, exp_pos, exp_seg, exp_nh = [], [], [0], []
        for b in range(B):
            live_t = torch.nonzero(new_mask[b] > 0).flatten().tolist()
            exp_rows += [y_full[b, t] for t in live_t]
            exp_pos += live_t
            n = S - len(live_t)
            if n:
                exp_rows.append(torch.zeros(D))
                exp_pos.append(-1)
            exp_nh.append(n)
            exp_seg.append(len(exp_pos))
        Rn = len(exp_pos)
        assert tot.tolist() == [Rn, max(np.diff(exp_seg))]
        assert sg.tolist() == exp_seg and nhn.tolist() == exp_nh and ps[:Rn].tolist() == exp_pos
        assert torch.equal(xs[:Rn], torch.stack(exp_rows))
        assert torch.equal(rs[:Rn], (torch.tensor(exp_pos) >= 0).float())


# ---- model level ------------------------------------------------------------------------------------------------------------
def _margins(h_token, thr=THR):
    """Smallest |c - (1 - eps)| over the layers each token runs (from the reference's per-layer h), [B, S]."""
    L, B, S = h_token.shape
    c = np.zeros((B, S), np.float32)
    live = np.ones((B, S), bool)
    mm = np.full((B, S), np.inf)
    for l in range(L - 1):
        c = np.where(live, c + h_token[l], c)
        mm = np.where(live, np.minimum(mm, np.abs(c - np.float32(thr))), mm)
        live &= c < thr
    return mm


def _run_hip(model, x, mode):
    from peekvit_amd import engine, ops
    n0 = ops.launch_count
    with torch.no_grad(), engine.precision(mode):
        out = model(x)
    torch.cuda.synchronize()
    assert ops.launch_count > n0, "HIP kernels did not run"
    return out


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_model_matches_reference_golden(name, golden):
    from peekvit_amd import engine
    dev = _dev()
    g = golden(name)
    model = _model(name, dev)
    x = _images(name, g).to(dev)
    for mode in ("f16", "auto"):
        logits = _run_hip(model, x, mode)
        if mode == "auto":
            # on the micro models the self-check must keep the packed fp16 forward; at 224 it may hand the key to the composite (a measured
            # contract decision: its limit is 9e-4 on the first images) - the f16 pass above has tested the packed forward there
            print(f"\n{name} [auto]: packed forward kept {engine.last_forward_guarded()}, self-check {engine.selfcheck_last}")
            if name in ("avit_micro", "avit_cls2_reg2", "avit_allhalt"):
                assert engine.last_forward_guarded(), "mode auto repeated the forward in the fallback: the packed path's result was not tested"
        enc = model.encoder
        err = rel_l2(logits, g["logits"])
        assert err < 1e-3, f"{name} [{mode}]: logits rel L2 {err:.3g}"
        depth, ref_depth = enc.counter_token.cpu().numpy(), g["counter_token"]
        safe = _margins(g["h_token"]) > DELTA
        if name in ("avit_micro", "avit_allhalt"):
            safe[:] = True
        assert (depth[safe] == ref_depth[safe]).all(), f"{name} [{mode}]: {(depth[safe] != ref_depth[safe]).sum()} token depths differ"
        assert np.allclose(enc.rho_token.cpu().numpy()[safe], g["rho_token"][safe], atol=2e-2)
        hs = torch.stack(enc.halting_score_layer).cpu().numpy()
        assert np.allclose(hs, g["halting_score_layer"], atol=1e-3, equal_nan=True), f"{name} [{mode}]: halting_score_layer"


def test_large_batch_against_gpu_composite():
    """avit_s dims at batch 2048 (gate_center 5): packed forward vs the stock-op composite on the same GPU."""
    from peekvit_amd import engine
    dev = _dev()
    model = _model("avit_s224_gc5", dev)
    x = torch.randn(2048, 3, 224, 224, generator=torch.Generator().manual_seed(11)).to(dev)
    with torch.no_grad():
        ref = model._composite_forward(x)
    ref_depth = model.encoder.counter_token.clone()
    got = _run_hip(model, x, "f16")
    flips = (model.encoder.counter_token != ref_depth).any(dim=1)
    rate = float(flips.float().mean())
    print(f"\navit_s dims, batch 2048: depth-flip rate {rate:.4f} of images ({int(flips.sum())}), mean depth {float(ref_depth.mean()):.2f}")
    assert rate < 0.25
    keep = ~flips
    err = rel_l2(got[keep], ref[keep])
    assert err < 1e-3, f"logits rel L2 {err:.3g} on the {int(keep.sum())} images without depth flips"
    assert engine.act_syncs > 0


def test_batch_size_change_and_modes():
    dev = _dev()
    model = _model("avit_micro", dev)
    for batch, mode, tol in ((5, "f16", 1e-3), (1, "f16", 1e-3), (7, "bf16", 8e-3), (3, "auto", 1e-3)):
        x = _images("avit_micro", batch=batch, seed=batch).to(dev)
        with torch.no_grad():
            ref = model._composite_forward(x)
        ref_depth, ref_rho = model.encoder.counter_token.clone(), model.encoder.rho_token.clone()
        ref_hs = torch.stack(model.encoder.halting_score_layer)
        got = _run_hip(model, x, mode)
        assert model.encoder.counter_token.shape == (batch, model.seq_length)
        same = (model.encoder.counter_token == ref_depth).all(dim=1)
        assert bool(same.float().mean() >= 0.5), mode
        assert rel_l2(got[same], ref[same]) < tol, mode
        hs = torch.stack(model.encoder.halting_score_layer)
        if batch == 1:
            assert torch.isnan(hs).all() and torch.isnan(ref_hs).all()
        else:
            assert torch.allclose(hs, ref_hs, atol=5e-3), mode
        assert torch.allclose(model.encoder.rho_token[same], ref_rho[same], atol=5e-2)


def test_successive_forwards_are_not_replayed():
    """Six batch-8 forwards with different inputs each equal the composite on THAT input: nothing was captured and replayed."""
    from peekvit_amd import engine
    dev = _dev()
    model = _model("avit_micro", dev)
    for i in range(6):
        x = _images("avit_micro", batch=8, seed=100 + i).to(dev)
        with torch.no_grad():
            ref = model._composite_forward(x)
        ref_depth = model.encoder.counter_token.clone()
        got = _run_hip(model, x, "auto")
        same = (model.encoder.counter_token == ref_depth).all(dim=1)
        assert bool(same.any()) and rel_l2(got[same], ref[same]) < 1e-3, i
    st = engine.guard_state(model)
    assert not st.graphs


# ---- production sizes: the scan's three regimes, every ragged-attention tile bound ------------------------------------------------
def _act_case(B, S, D, nc, seed):
    """Packed halting state for B images of S tokens: image kinds by b % 6 - nothing halted, one token left, class token halted, every
    token halted, class token exactly on the threshold, random - plus, in every image with live tokens, tokens whose c + h lands exactly
    on the fp32 threshold (h = sigmoid(0.25 * 8 - 2) = 0.5 exactly, c = THR - 0.5; and c = THR - 1 for the last layer's h = 1)."""
    g = torch.Generator().manual_seed(seed)
    gs, gc = 8.0, 2.0
    mask = (torch.rand(B, S, generator=g) < 0.7).float()
    kind = torch.arange(B) % 6
    mask[kind == 0] = 1.0
    one = torch.nonzero(kind == 1).flatten()
    mask[one] = 0.0
    mask[one, torch.randint(0, S, (one.numel(),), generator=g)] = 1.0
    mask[kind == 2, 0] = 0.0
    mask[kind == 3] = 0.0
    mask[kind == 4, 0] = 1.0
    c = torch.rand(B, S, generator=g) * 0.9
    exact_h = torch.rand(B, S, generator=g) < 0.03                 # c + h == THR at h = 0.5
    exact_h[kind == 4, 0] = True
    exact_1 = (torch.rand(B, S, generator=g) < 0.03) & ~exact_h     # c + 1 == THR (the last layer)
    c = torch.where(exact_h, torch.tensor(THR - 0.5, dtype=torch.float32), c)
    c = torch.where(exact_1, torch.tensor(THR - 1.0, dtype=torch.float32), c)
    c = torch.where(mask > 0, c, torch.tensor(1.2))
    Rr = torch.where(mask > 0, 1 - c, torch.zeros(()))
    rho = torch.randint(0, 4, (B, S), generator=g).float()
    counter = torch.randint(1, 4, (B, S), generator=g).float()
    acc = torch.randn(B, nc, D, generator=g)
    # packed rows: every image's live tokens in order, then one representative row when anything has halted
    n_live = mask.sum(1).long()
    has_rep = (n_live < S).long()
    seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(n_live + has_rep, 0)])
    lb, lt = torch.nonzero(mask > 0, as_tuple=True)
    first = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(n_live, 0)[:-1]])
    live_row = seg[lb] + torch.arange(lb.numel()) - first[lb]
    rep_row = seg[:-1] + n_live                                        # valid where has_rep
    R = int(seg[-1])
    y = torch.randn(R, D, generator=g) * 0.3
    tok_row = torch.full((B, S), -1, dtype=torch.long)
    tok_row[lb, lt] = live_row
    tok_row = torch.where(tok_row >= 0, tok_row, rep_row[:, None].expand(B, S))
    pos = torch.full((R,), -1, dtype=torch.int32)
    pos[live_row] = lt.int()
    y[live_row[exact_h[lb, lt]], 0] = 0.25
    # no other token within 1e-5 of the threshold: the kernel's h and torch.sigmoid may differ in the last bit
    h64 = torch.sigmoid(y[:, 0].double() * gs - gc)[tok_row]
    near = ((c.double() + h64 - THR).abs() < 1e-5) & ~exact_h & (mask > 0)
    near |= ((c.double() + 1.0 - THR).abs() < 1e-5) & ~exact_1 & (mask > 0)
    c = torch.where(near, c - 3e-5, c)
    Rr = torch.where(mask > 0, 1 - c, Rr)
    nh = (S - n_live).int()
    return dict(mask=mask, c=c, Rr=Rr, rho=rho, counter=counter, acc=acc, y=y, seg=seg.int(), nh=nh, pos=pos, tok_row=tok_row, gs=gs, gc=gc,
                exact_h=exact_h & (mask > 0), exact_1=exact_1 & (mask > 0))


@pytest.mark.parametrize("B,S,D,nc", [(1, 197, 384, 1), (1, 256, 384, 16), (64, 256, 384, 16), (65, 197, 384, 2), (65, 256, 384, 1),
                                      (1024, 256, 384, 1), (1025, 197, 384, 16), (2051, 256, 64, 2), (2051, 197, 64, 16)])
def test_act_step_production_sizes(B, S, D, nc):
    """One wave (B <= 64), a carry across waves (B > 64) and several images per thread (B > 1024) of pv_seg_scan_kernel (pv_rows.h), with the
    update and compaction kernels around it: segment table, counts, positions, totals and every next packed row bit-exact."""
    from peekvit_amd import ops
    dev = _dev()
    k = _act_case(B, S, D, nc, seed=B * 7 + S + nc)
    y, seg, nh, pos, tok_row = k["y"], k["seg"], k["nh"], k["pos"], k["tok_row"]
    R = y.shape[0]
    y_col0 = y[:, :1][tok_row]                                          # [B, S, 1]: every token's block output, column 0
    y_cls = y[tok_row[:, :nc]]                                          # [B, nc, D]: the class tokens' rows
    yd = y.to(dev)
    for last in (False, True):
        st = [k[n].clone().to(dev) for n in ("c", "Rr", "rho", "counter", "mask")]
        acc_d, hp = k["acc"].clone().to(dev), torch.zeros(B, device=dev)
        nxt = (torch.full((R, D), float("nan"), device=dev), torch.full((R,), -1.0, device=dev), torch.full((B + 1,), -9, dtype=torch.int32, device=dev),
               torch.full((B,), -9, dtype=torch.int32, device=dev), torch.full((R,), -7, dtype=torch.int32, device=dev),
               torch.full((2,), -9, dtype=torch.int32, device=dev))
        ops.act_step(yd, seg.to(dev), nh.to(dev), pos.to(dev), st, acc_d, hp, k["gs"], k["gc"], THR, last, None if last else nxt)
        torch.cuda.synchronize()
        ins = [k[n] for n in ("c", "Rr", "rho", "counter", "mask")]
        rc, rR, rrho, rcnt, rmask, _, h = _act_reference(y_col0, *ins, k["acc"][:, :, :1] * 0, k["gs"], k["gc"], last, nc)
        racc = _act_reference(y_cls, *[t[:, :nc] for t in ins], k["acc"], k["gs"], k["gc"], last, nc)[5]
        live = k["mask"] > 0
        got = [t.cpu() for t in st]
        assert torch.equal(got[4][live], rmask[live]) and torch.equal(got[3][live], rcnt[live])
        for a, b_ in zip(got, ins):
            assert torch.equal(a[~live], b_[~live])                      # halted tokens untouched
        for a, b_ in ((got[0], rc), (got[1], rR), (got[2], rrho)):
            assert torch.allclose(a[live], b_[live], rtol=1e-6, atol=1e-6)
        assert torch.allclose(acc_d.cpu(), racc, rtol=1e-6, atol=1e-6)
        assert torch.allclose(hp.cpu(), h.sum(dim=1), rtol=1e-5, atol=1e-5)
        ex = k["exact_1"] if last else k["exact_h"]                    # c + h == THR: halts (neither reached nor running), rho + 1 only
        assert bool(ex.any())
        assert (got[4][ex] == 0).all() and torch.equal(got[3][ex], k["counter"][ex]) and torch.equal(got[2][ex], k["rho"][ex] + 1)
        if last:
            continue
        xs, rs, sg, nhn, ps, tot = [t.cpu() for t in nxt]
        surv = rmask > 0
        n_s = surv.sum(1).long()
        Ln = n_s + (n_s < S).long()
        exp_seg = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(Ln, 0)])
        Rn = int(exp_seg[-1])
        sb, stok = torch.nonzero(surv, as_tuple=True)
        first = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(n_s, 0)[:-1]])
        dst = exp_seg[sb] + torch.arange(sb.numel()) - first[sb]
        exp_pos = torch.full((Rn,), -1, dtype=torch.int32)
        exp_pos[dst] = stok.int()
        exp_x = torch.zeros(Rn, D)
        exp_x[dst] = y[tok_row[sb, stok]]
        assert tot.tolist() == [Rn, int(Ln.max())]
        assert torch.equal(sg, exp_seg.int()) and torch.equal(nhn, (S - n_s).int())
        assert torch.equal(ps[:Rn], exp_pos)
        assert torch.equal(xs[:Rn], exp_x)
        assert torch.equal(rs[:Rn], (exp_pos >= 0).float())


MODES_AVIT = ("bf16", "f16")


@pytest.mark.parametrize("nkt", range(1, 14))
def test_varlen_attention_every_tile_bound(nkt):
    """Every NKT instantiation (longest segment 16 nkt and 16 nkt - 15), batches on both sides of pv_bh_map's grouped branch (B >= 8) and its
    remainder, length-1 segments counted up to 255 times; and a segment's rows do not depend on where in the batch it sits."""
    from peekvit_amd import engine, ops, _lib
    dev = _dev()
    B, H = ((8, 1), (13, 6), (67, 12))[nkt % 3]
    dh = 64
    for longest in (16 * nkt, 16 * nkt - 15):
        g = torch.Generator().manual_seed(100 * nkt + longest)
        lens = torch.randint(1, longest + 1, (B,), generator=g)
        lens[torch.randperm(B, generator=g)[:2]] = longest
        ones = torch.randperm(B, generator=g)[:3]
        lens[ones] = 1
        lens[0] = longest
        nh = torch.randint(0, 256, (B,), generator=g) * (torch.rand(B, generator=g) < 0.6)
        nh[ones] = torch.tensor([255, 1, 254])
        lens, nh = lens.tolist(), nh.tolist()
        seg = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
        # the same image placed last: image 0's segment swapped with image B-1's (other row offsets, same max_len)
        perm = [B - 1] + list(range(1, B - 1)) + [0]
        lens2 = [lens[i] for i in perm]
        seg2 = torch.tensor([0] + list(np.cumsum(lens2)), dtype=torch.int32, device=dev)
        for mode in MODES_AVIT:
            with engine.precision(mode):
                dt = _lib.operand_dtype()
                qkv = _packed_qkv(lens, H, dh, nkt, dt, dev)
                qkv[:, 2 * H * dh:].clamp_(-3.5, 3.5)        # |out| < 4, the range in which the absolute tolerances below are set
                out = torch.full((sum(lens), H * dh), float("nan"), dtype=dt, device=dev)
                ops.attention_varlen(qkv, out, seg, torch.tensor(nh, dtype=torch.int32, device=dev), longest, H, dh)
                rows = [qkv[int(seg[i]):int(seg[i + 1])] for i in perm]
                qkv2 = torch.cat(rows).contiguous()
                out2 = torch.full_like(out, float("nan"))
                ops.attention_varlen(qkv2, out2, seg2, torch.tensor([nh[i] for i in perm], dtype=torch.int32, device=dev), longest, H, dh)
                torch.cuda.synchronize()
            ref = _attention_fp64(qkv, lens, nh, H, dh)
            got = out.double().cpu()
            assert torch.isfinite(got).all()
            tol = 1.5e-2 if mode == "bf16" else 2e-3
            err = (got - ref).abs().max().item()
            assert err < tol, f"nkt={nkt} longest={longest} B={B} H={H} {mode}: max |err| {err:.3g} vs fp64"
            L0 = lens[0]
            assert torch.equal(out2[-L0:], out[:L0]), "image 0's rows moved to image B-1"
            assert torch.equal(out2[:lens[B - 1]], out[-lens[B - 1]:]), "image B-1's rows moved to image 0"

