"""RankPointCloudTransformer's eval forward on the MI355X (include/peekvit_hip_rank_infer.h, peekvit_amd.engine.rank_pct_forward).

The two kernels are exact: pv_rank_order_gap against a stable descending sort on the CPU (and against pv_rank_topk_gap, whose bits it promises),
pv_layernorm_gather_f32_bf16 against pv_gather_tokens followed by pv_layernorm_f32_bf16.  The model is held to two statements: the rows it keeps
are exactly the top rows of its own fp32 norms, and its logits are the composite's when the composite keeps those rows (the fp64 composite replays
the recorded rows) - within 1e-3 relative L2 on fp16 operands, the project's inference contract.  Which rows the fp32 composite would have kept
itself is reported, not asserted: DESIGN.md section 18 says why they differ on almost every cloud."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from peekvit_amd import _lib, engine, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))
GUARD = 8                       # sentinel elements behind every output buffer


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. pv_rank_order_gap
# ---------------------------------------------------------------------------------------------------------------------------------
RANK_B = 3
RANK_NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 2049, 4096)          # one key; a wave and its neighbours; both sides of every network size 256 E
FAMILIES = ("random", "equal", "four_values", "specials")


def _ks(N):
    return sorted({0, 1, N // 2, N - 1, N})


@functools.lru_cache(maxsize=None)
def _rank_case(N, family):
    """norms fp32 [RANK_B, N] of a family and their stable descending sort on the CPU (values, indices)."""
    g = _g(N * 11 + FAMILIES.index(family))
    if family == "random":
        v = torch.rand(RANK_B, N, generator=g) * 3 + 0.01
    elif family == "equal":
        v = torch.full((RANK_B, N), 0.75)
    elif family == "four_values":                        # heavy ties: most ranks are decided by the lowest-index-first rule
        v = torch.floor(torch.rand(RANK_B, N, generator=g) * 4) / 4 + 0.25
    else:                                                # one row with +0.0, +inf and the canonical NaN among random values
        v = torch.rand(RANK_B, N, generator=g) * 3 + 0.01
        pos = torch.randperm(N, generator=g)[:min(N, 9)].tolist()
        for j, p in enumerate(pos):
            v[1, p] = (0.0, float("inf"), float("nan"))[j % 3]
    v = v.float().contiguous()
    s = torch.sort(v, dim=1, descending=True, stable=True)
    assert torch.equal(s.indices, torch.argsort(v, dim=1, descending=True, stable=True))
    return v, s.values, s.indices.int()


def _order(lib, stream, norms_d, N, k, gap_fill=None, gap=True):
    """One launch into sentinel-filled buffers -> (rc, keep int32 [B, k] on the CPU, the guard behind it, gap_min on the CPU or None)."""
    B = norms_d.shape[0]
    keep = torch.full((B * k + GUARD,), -1, dtype=torch.int32, device=DEV)
    gm = None
    if gap:
        gm = (torch.full((B,), float("inf")) if gap_fill is None else gap_fill.clone()).to(DEV)
    rc = lib.pv_rank_order_gap(norms_d.data_ptr(), keep.data_ptr(), gm.data_ptr() if gap else None, B, N, k, stream)
    flat = keep.cpu()
    return rc, flat[:B * k].reshape(B, k), flat[B * k:], gm.cpu() if gap else None


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", RANK_NS)
def test_rank_order_exact_against_stable_sort(N, family):
    """keep == torch.argsort(norms.cpu(), descending=True, stable=True)[:, :k] for k in {0, 1, N // 2, N - 1, N}, with and without gap_min, twice
    with identical bits, and equal to ops.rank_topk on the same norms; k = 0 leaves the sentinel-filled buffer alone.  The gap is checked as
    tests/test_hip_token_selection.py checks pv_rank_topk_gap's: +inf comes back as (n[k-1] - n[k]) / n[k-1] evaluated in fp32 on the CPU within
    2^-21 relative, k = N leaves it untouched, a pre-filled value below the gap is kept - and its bits are pv_rank_topk_gap's."""
    lib, stream = _lib.load(), ops.raw_stream(0)
    v, sv, si = _rank_case(N, family)
    vd = v.to(DEV)
    B = RANK_B
    inf = torch.full((B,), float("inf"))
    for k in _ks(N):
        rc, keep, guard, _ = _order(lib, stream, vd, N, k, gap=False)
        assert rc == 0 and bool((guard == -1).all()), (k, rc)
        assert torch.equal(keep, si[:, :k]), f"pv_rank_order_gap N={N} k={k} {family}"
        rc, keep_g, guard, gm = _order(lib, stream, vd, N, k)
        assert rc == 0 and bool((guard == -1).all()), (k, rc)
        assert torch.equal(keep_g, keep), f"N={N} k={k} {family}: another keep list with gap_min"
        rc, keep_2, _, gm_2 = _order(lib, stream, vd, N, k)
        assert rc == 0 and torch.equal(keep_2, keep_g) and torch.equal(gm_2.view(torch.int32), gm.view(torch.int32))          # two runs, identical bits
        # the second oracle: the O(N^2) kernel, keep and gap bit for bit
        if k > 0:                                                                     # (an empty keep tensor has no address for pv_rank_topk_gap)
            gm_t = inf.clone().to(DEV)
            keep_t = ops.rank_topk(vd, k, gm_t)
            assert torch.equal(keep_t.cpu(), keep) and torch.equal(gm_t.cpu().view(torch.int32), gm.view(torch.int32)), (N, k, family)
        assert torch.equal(ops.rank_order(vd, k).cpu(), keep)                          # the wrapper
        if family == "specials":
            continue
        if k == 0 or k == N:
            assert torch.equal(gm, inf), (k, gm)
            continue
        want = (sv[:, k - 1] - sv[:, k]) / sv[:, k - 1]                            # fp32, as the kernel's expression
        err = (gm.double() - want.double()).abs()
        assert bool((err <= 2.0 ** -21 * want.double()).all()), (k, gm, want)
        low = torch.where(want > 0, want * 0.5, torch.full_like(want, -1.0))
        rc, keep_l, _, gm_l = _order(lib, stream, vd, N, k, gap_fill=low)
        assert rc == 0 and torch.equal(keep_l, keep) and torch.equal(gm_l.view(torch.int32), low.view(torch.int32)), (k, gm_l, low)


def test_rank_order_specials_row_order():
    """NaN above +inf above every finite value, +0.0 last, each group by index."""
    row = torch.tensor([[0.0, 2.5, float("nan"), float("inf"), 2.5, 0.0, 1e-40, float("inf"), 7.0, float("nan"), 2.5, 3.4e38, 0.0, 1.0]])
    keep = ops.rank_order(row.to(DEV), row.shape[1]).cpu()
    assert keep.tolist() == torch.argsort(row, dim=1, descending=True, stable=True).tolist()
    assert keep[0, :4].tolist() == [2, 9, 3, 7] and keep[0, -3:].tolist() == [0, 5, 12]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. pv_layernorm_gather_f32_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand", ["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128, 192, 1024])
@pytest.mark.parametrize("S", [2, 13, 130])
def test_layernorm_gather_is_gather_then_layernorm(S, D, operand):
    B = 2
    g = _g(S * 1031 + D)
    x = (torch.randn(B, S, D, generator=g) * 1.7 + 0.3).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
    with engine.precision(operand):
        od = _lib.operand_dtype()
        for k in sorted({0, 1, S - 2, S - 1}):
            keep = torch.stack([torch.randperm(S - 1, generator=g)[:k] for _ in range(B)]).int().to(DEV)          # a random prefix of a permutation
            rows = B * (k + 1)
            xg = ops.gather_tokens(x, keep)
            w16, w32 = torch.empty((rows, D), dtype=od, device=DEV), torch.empty((rows, D), dtype=torch.float32, device=DEV)
            ops.layernorm_f32_bf16(xg, gamma, beta, 1e-5, w16, w32)
            o16 = torch.full((rows * D + GUARD,), -3.0, dtype=od, device=DEV)
            o32 = torch.full((rows * D + GUARD,), -3.0, dtype=torch.float32, device=DEV)
            ops.layernorm_gather_f32_bf16(x, keep, gamma, beta, 1e-5, o16[:rows * D].view(rows, D), o32[:rows * D].view(rows, D))
            torch.cuda.synchronize()
            assert bool((o16[rows * D:] == -3.0).all()) and bool((o32[rows * D:] == -3.0).all()), "written past the last row"
            assert torch.equal(o16[:rows * D].view(torch.int16), w16.view(-1).view(torch.int16)), (S, D, k, operand)
            assert torch.equal(o32[:rows * D].view(torch.int32), w32.view(-1).view(torch.int32)), (S, D, k, operand)
    assert od == (torch.float16 if operand == "f16" else torch.bfloat16)


def test_layernorm_gather_clamps_indices_to_the_image():
    B, S, D = 2, 5, 64
    x = torch.randn(B, S, D, generator=_g(5)).to(DEV)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    bad = torch.tensor([[-7, 99, 2], [4, 1 << 30, -1]], dtype=torch.int32, device=DEV)
    good = torch.tensor([[0, 3, 2], [3, 3, 0]], dtype=torch.int32, device=DEV)
    outs = []
    for keep in (bad, good):
        o16, o32 = torch.empty((B * 4, D), dtype=_lib.operand_dtype(), device=DEV), torch.empty((B * 4, D), dtype=torch.float32, device=DEV)
        ops.layernorm_gather_f32_bf16(x, keep, gamma, beta, 1e-5, o16, o32)
        outs.append((o16, o32))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# RankPointCloudTransformer
# ---------------------------------------------------------------------------------------------------------------------------------
SYNTH_KEYS = ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes", "num_registers", "num_class_tokens")


def _model(cname, kw, device=DEV, dtype=torch.float32):
    from peekvit_amd.models import pct
    m = getattr(pct, cname)(**kw).eval()
    cfg = {k: v for k, v in kw.items() if k in SYNTH_KEYS}
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(cfg, 0).items()}, strict=True)
    return m.to(device=device, dtype=dtype)


def _ranked(info, device=DEV, dtype=torch.float32, fused=True, budget=None):
    m = _model("RankPointCloudTransformer", info["kwargs"], device, dtype)
    m.enable_ranking(info["ranking"])
    m.set_budget(info["budget"] if budget is None else budget)
    if fused:
        m.set_fused_inference(True)
    return m


def _run(model, x, mode, warm=False):
    """(logits, launches) of a no_grad forward in precision mode `mode`; warm: behind one forward that has cast the weights (launches of their own)."""
    if warm:
        with torch.no_grad(), engine.precision(mode):
            model(x)
    n0 = ops.launch_count
    with torch.no_grad(), engine.precision(mode):
        y = model(x).clone()
    torch.cuda.synchronize()
    return y, ops.launch_count - n0


@pytest.mark.parametrize("name", ["pct_n128", "pct_n64r1"])
def test_without_ranking_the_forward_is_pct_forward_bit_for_bit(name):
    """The split of engine._pct_block is exact: a ranking model that does not sort, switch on, gives engine.pct_forward's bits in mode f16."""
    info = META["cases"][name]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, name + ".npz"))["points"]).to(DEV)
    plain = _model("PointCloudTransformer", info["kwargs"])
    ranked = _model("RankPointCloudTransformer", info["kwargs"])
    assert list(ranked.state_dict()) == list(plain.state_dict())
    ranked.enable_ranking(False)
    ranked.set_fused_inference(True)
    with torch.no_grad(), engine.precision("f16"):
        want = engine.pct_forward(plain, x).clone()
    got, n = _run(ranked, x, "f16", warm=True)
    assert n == 1 + 7 * info["kwargs"]["num_layers"] + 2 and torch.equal(got, want)


@functools.lru_cache(maxsize=None)
def _replayed(name, mode):
    """One HIP forward of a rank fixture in `mode` and the fp64 composite REPLAYING its recorded rows: (info, logits, launches, last_keep and last_norms
    per sorting layer, fp64 logits of the replay, the fp64 norms of rows 1.. of every sorting block's input in the replay)."""
    from peekvit_amd.models.pct import RankingPCTBlock
    info = META["rank_cases"][name]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, name + ".npz"))["points"]).to(DEV)
    model = _ranked(info)
    logits, launches = _run(model, x, mode, warm=True)
    keeps = [model.encoder.layers[i].last_keep.clone() for i in info["ranked_layers"]]
    norms = [model.encoder.layers[i].last_norms.clone() for i in info["ranked_layers"]]
    f64 = _ranked(info, dtype=torch.float64, fused=False)
    calls, norms64 = [], []

    def replay(inp):                                     # (as tests/test_hip_rank_train.py::test_one_training_step_with_fused_ranking replays its rows)
        rec = keeps[len(calls)]
        calls.append(1)
        norms64.append(inp[:, 1:].norm(dim=-1))
        return RankingPCTBlock.replayed_order(rec, inp.shape[1])

    stock = RankingPCTBlock.__dict__["sort_order"]
    RankingPCTBlock.sort_order = staticmethod(replay)
    try:
        with torch.no_grad():
            logits64 = f64(x.double()).clone()
    finally:
        RankingPCTBlock.sort_order = stock
    assert len(calls) == len(keeps)
    for i, kp in zip(info["ranked_layers"], keeps):
        assert torch.equal(f64.encoder.layers[i].last_keep, kp)
    return info, logits, launches, keeps, norms, logits64, norms64


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["rankpct_n128", "rankpct_n64r1"])
def test_model_at_equal_decisions(name, mode):
    """(i) last_keep is [B, L_l], starts with row 0, distinct and in range; (ii) it is exactly the stable descending argsort of last_norms cut at L - 1;
    (iii, iv) the logits are within 1e-3 relative L2 of the fp64 composite replaying those rows in mode f16 (bf16: printed, as elsewhere); (v) with e the
    largest relative difference between last_norms and the replay's fp64 norms of the same rows, every kept row's HIP norm is >= every dropped row's, so
    in the replay's norms a dropped row exceeds a kept one by at most a factor (1 + e) / (1 - e): the worst relative inversion is <= 2 e / (1 - e);
    (vi) reported only: the share of clouds whose kept sets are the reference's, and the distance to the golden logits.

    Measured on the MI355X: see DESIGN.md section 25."""
    info, logits, launches, keeps, norms, logits64, norms64 = _replayed(name, mode)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    B = info["batch"]
    S = info["kwargs"]["num_points"] + info["kwargs"].get("num_registers", 0)
    lengths = {"rankpct_n128": [96, 72], "rankpct_n64r1": [33, 17]}[name]
    nl, nr = info["kwargs"]["num_layers"], len(info["ranked_layers"])
    assert launches == 1 + 7 * nl + 2 * nr + 2                          # a sorting block: token_norm and rank_order on top of its seven
    same_sets = torch.ones(B, dtype=torch.bool)
    for li, (i, L, kp, nm, n64) in enumerate(zip(info["ranked_layers"], lengths, keeps, norms, norms64)):
        assert tuple(kp.shape) == (B, L) and kp.dtype == torch.int64 and tuple(nm.shape) == (B, S - 1) and nm.dtype == torch.float32          # (i)
        assert bool((kp[:, 0] == 0).all()) and bool((kp >= 0).all()) and bool((kp < S).all())
        assert all(len(set(row)) == L for row in kp.tolist())
        order = torch.argsort(nm.cpu(), dim=1, descending=True, stable=True)[:, :L - 1]                                                     # (ii)
        assert torch.equal(kp[:, 1:].cpu() - 1, order), f"{name} layer {i}: the kept rows are not the top rows of the forward's own norms"
        e = float(((nm.double() - n64) / n64).abs().max())                                                                                   # (v)
        kept = torch.zeros((B, S - 1), dtype=torch.bool, device=DEV).scatter_(1, kp[:, 1:] - 1, True)
        lo_kept = torch.where(kept, n64, torch.full_like(n64, float("inf"))).min(dim=1).values
        hi_drop = torch.where(kept, torch.full_like(n64, 0.0), n64).max(dim=1).values
        inversion = float(((hi_drop - lo_kept) / lo_kept).clamp_min(0).max()) if L - 1 < S - 1 else 0.0
        print(f"{name} {mode} layer {i}: S = {S} -> L = {L}; norms against the replay's fp64 norms e = {e:.3g}; worst relative inversion across the keep "
              f"boundary {inversion:.3g} (bound 2e/(1-e) = {2 * e / (1 - e):.3g})")
        assert e < 0.5 and inversion <= 2 * e / (1 - e)
        ref_set = torch.from_numpy(z[f"kept_{i}"].astype(np.int64))                                                                        # (vi)
        same_sets &= (torch.sort(kp.cpu(), dim=1).values == ref_set).all(dim=1)
        S = L
    err = rel_l2(logits, logits64)
    print(f"{name} {mode}: logits against the fp64 composite replaying the kept rows {err:.3g}; against the golden logits (the reference's own rows) "
          f"{rel_l2(logits, z['logits']):.3g}; clouds whose kept sets are the reference's in every layer: {int(same_sets.sum())} of {B}")
    assert bool(torch.isfinite(logits).all())
    if mode == "f16":
        assert err <= 1e-3                                                                                                                   # (iv)


@pytest.mark.parametrize("name", ["rankpct_n128", "rankpct_n64r1"])
def test_budget_one_keeps_every_row(name):
    """Every row kept: the decisions are the composite's whatever the norms, so the logits are held to the fp32 composite and to the fp64 composite with no
    replay (mode f16, 1e-3)."""
    info = META["rank_cases"][name]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, name + ".npz"))["points"]).to(DEV)
    model = _ranked(dict(info, ranking=True), budget=1.0)
    y, n = _run(model, x, "f16", warm=True)
    S = info["kwargs"]["num_points"] + info["kwargs"].get("num_registers", 0)
    assert n == 1 + 9 * info["kwargs"]["num_layers"] + 2
    for blk in model.encoder.layers:
        assert tuple(blk.last_keep.shape) == (info["batch"], S) and torch.equal(torch.sort(blk.last_keep, dim=1).values, torch.arange(S, device=DEV).expand(info["batch"], -1))
    with torch.no_grad():
        want32 = _ranked(dict(info, ranking=True), fused=False, budget=1.0)(x)
        want64 = _ranked(dict(info, ranking=True), "cpu", torch.float64, fused=False, budget=1.0)(x.cpu().double())
    e32, e64 = rel_l2(y, want32), rel_l2(y, want64)
    print(f"{name} budget 1.0 f16: against the fp32 composite {e32:.3g}, against the fp64 composite {e64:.3g}")
    assert e32 <= 1e-3 and e64 <= 1e-3


def test_graph_replay_is_bit_identical_to_the_eager_forward():
    from peekvit_amd.graph import GraphedForward
    info = META["rank_cases"]["rankpct_n128"]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "rankpct_n128.npz"))["points"]).to(DEV)
    model = _ranked(info)
    eager, n = _run(model, x, "auto")
    assert n > 0 and engine.last_forward_guarded()
    g = GraphedForward(model, x)
    y = g(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(y, eager) and torch.equal(g(x), eager)
    model.set_budget(0.5)
    g.refresh()
    eager2, _ = _run(model, x, "auto")
    assert not torch.equal(eager2, eager)
    assert torch.equal(g(x), eager2)
    assert [tuple(model.encoder.layers[i].last_keep.shape) for i in info["ranked_layers"]] == [(info["batch"], 64), (info["batch"], 32)]


def test_mode_auto_probes_with_the_replaying_composite(monkeypatch):
    info = META["rank_cases"]["rankpct_n128"]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "rankpct_n128.npz"))["points"]).to(DEV)
    model = _ranked(info)
    probes = []
    stock = type(model)._replay_probe
    monkeypatch.setattr(type(model), "_replay_probe", lambda self, xs: (probes.append(int(xs.shape[0])), stock(self, xs))[1])
    c0, t0 = engine.selfcheck_count, engine.selfcheck_trips
    y, n = _run(model, x, "auto")
    assert probes == [info["batch"]] and engine.selfcheck_count == c0 + 1 and engine.selfcheck_trips == t0
    err, probed, flips = engine.selfcheck_last
    print(f"rankpct_n128 auto: self-check against the replaying composite {err:.3g} on {probed} clouds, {flips} flips")
    assert flips == 0 and probed == info["batch"] and err <= engine.SELFCHECK_LIMIT
    assert engine.last_forward_guarded() and not engine.guard_state(model).unsafe and "x3" not in engine.guard_state(model).verdicts.values()
    keeps = [model.encoder.layers[i].last_keep.clone() for i in info["ranked_layers"]]
    y2, n2 = _run(model, x, "auto")
    assert probes == [info["batch"]] and engine.selfcheck_count == c0 + 1          # the second forward does not probe again
    assert torch.equal(y2, y) and engine.last_forward_guarded() and n2 == 1 + 7 * info["kwargs"]["num_layers"] + 2 * len(keeps) + 2
    yf, _ = _run(model, x, "f16")
    assert torch.equal(yf, y)                                                      # what mode auto returned is the fp16-operand forward
    # the boundaries it reports: one host read after the forward
    n_t, n_i = engine.rank_pct_near_ties, engine.rank_pct_gap_images
    with engine.rank_gaps(info["batch"], DEV) as gap:
        _run(model, x, "f16")
    want = torch.full((info["batch"],), float("inf"))
    S = info["kwargs"]["num_points"]
    for i, L in zip(info["ranked_layers"], (96, 72)):
        s = torch.sort(model.encoder.layers[i].last_norms.cpu(), dim=1, descending=True).values
        want = torch.minimum(want, (s[:, L - 2] - s[:, L - 1]) / s[:, L - 2])
    assert bool(((gap.cpu().double() - want.double()).abs() <= 2.0 ** -21 * want.double()).all())
    ties = engine.rank_pct_note_gaps(gap)
    assert ties == int((gap < engine.RANK_TIE_GAP).sum()) and engine.rank_pct_near_ties == n_t + ties and engine.rank_pct_gap_images == n_i + info["batch"]
    print(f"rankpct_n128: narrowest keep boundary per cloud {[f'{v:.3g}' for v in gap.tolist()]}; {ties} of {info['batch']} under RANK_TIE_GAP = {engine.RANK_TIE_GAP}")


def test_fallbacks_keep_their_path():
    """Switch off, train mode, grads on, CPU tensors, mode bf16x3, a budget that leaves fewer than two rows and a width the GEMMs do not take: the output of
    a model that never had the switch, bit for bit, and no launch of the new kernels."""
    info = META["rank_cases"]["rankpct_n64r1"]
    x = torch.from_numpy(np.load(os.path.join(GOLDEN, "rankpct_n64r1.npz"))["points"]).to(DEV)
    never, model = _ranked(info, fused=False), _ranked(info)
    assert list(model.state_dict()) == list(never.state_dict())
    assert len(list(model.parameters())) == len(list(never.parameters())) and len(list(model.buffers())) == len(list(never.buffers()))

    def same(a, b, xs, mode="f16", grad=False):
        outs = []
        for m in (a, b):
            torch.manual_seed(11)                        # (train mode: the head's dropout)
            n0 = ops.launch_count
            with torch.set_grad_enabled(grad), engine.precision(mode):
                outs.append(m(xs).detach().clone())
            assert m is not b or all(blk.last_norms is None for blk in m.encoder.layers), "the HIP forward ran"
        # (bit patterns: at budget 0.01 the second sorting block of the composite is left with no row at all and the mean over none is NaN, with or
        #  without the switch - torch.equal on the values would call that unequal)
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        return ops.launch_count - n0

    model.set_fused_inference(False)
    assert same(never, model, x) == 0                                                   # switch off
    model.set_fused_inference(True)
    never.train(), model.train()
    same(never, model, x)                                                              # train mode
    never.eval(), model.eval()
    same(never, model, x, grad=True)                                                   # grads on
    assert same(never.cpu(), model.cpu(), x.cpu()) == 0                                # CPU tensors
    never.to(DEV), model.to(DEV)
    assert same(never, model, x, mode="bf16x3") == 0                                   # no split-precision form
    never.set_budget(0.01), model.set_budget(0.01)
    assert not engine.rank_pct_supported(model, x) and same(never, model, x) == 0      # L < 2
    kw = dict(info["kwargs"], hidden_dim=96, mlp_dim=192, num_heads=2)
    wide = dict(info, kwargs=kw)
    never96, model96 = _ranked(wide, fused=False), _ranked(wide)
    assert not engine.rank_pct_supported(model96, x) and same(never96, model96, x) == 0          # D = 96
    # and with everything in place the switch does change the path
    model.set_budget(0.5)
    y, n = _run(model, x, "f16")
    assert n > 0 and all(blk.last_norms is not None for blk in model.encoder.layers)
