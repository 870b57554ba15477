"""The training path of the point-cloud stem on the MI355X (include/peekvit_hip_pct_train.h, peekvit_amd.pct_train): the four entry points
against float64 restatements in plain torch ops, the autograd function inside ARPE against the stock-op composite's autograd, and one
training step of both point-cloud models with the path on and off.

Tolerances of fp32 results follow the rule of tests/test_hip_pct.py: the same computation on stock fp32 torch ops is measured against the
float64 restatement, and the kernel path may be four times as far from it, in relative L2 and in max abs.  A gradient whose true value is 0
(a bias in front of a batch-statistics BatchNorm) is held to max abs alone: a relative error against rounding noise says nothing.
The raw moment rows have no stock-op counterpart with the same summation structure, so their bound comes from the format: a feature is one
fp32 subtraction (one rounding, two in a product of two features), the sums are formed in fp64 and a row is rounded to fp32 once, so
|sum - exact| <= 4 * 2^-24 * sum |terms| (3 roundings and the second-order terms).

Fixture conditions (asserted; another seed where one fails): the k-NN tie condition of test_hip_pct._neighbours, and for every comparison
against autograd the fp32 and fp64 restatements pick the same neighbour in the max for every (query, channel) - a near-tie of the max is a
discontinuity of the gradient, not an error."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from peekvit_amd import ops, pct_train, synth
from test_hip_pct import _four_times, _neighbours, _params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))
U = 2.0 ** -24

# (N, B, k): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    "n16": (16, 3, 1),            # one partly filled wave; the point alone (every difference 0)
    "n48": (48, 3, 3),            # N not a multiple of 64
    "n80": (80, 3, 5),            # two workgroups per image, the second with 16 queries
    "n200": (200, 2, 12),         # four registers of keys
    "n64": (64, 2, 64),           # k = N
    "n1000": (1000, 2, 62),       # sixteen registers; 32 partial rows
    "n4096": (4096, 1, 256),      # the 64-register instantiation, 48 KiB of LDS, k above the lane count
    "dup": (80, 3, 5),            # the duplicate cloud of test_arpe_embed_duplicates_beyond_k: exact ties everywhere
}
SEEDS = {"n1000": 0}
CASES = sorted(SHAPES)


def _points(name):
    N, B, k = SHAPES[name]
    if name == "dup":
        xs = synth.synth_points(B, N, seed=4)
        xs[:, 10:30] = xs[:, 3:4]                          # 21 rows of one coordinate triple, k = 5
        xs[1, 40:52] = xs[1, 0:1]
        return xs
    return synth.synth_points(B, N, seed=SEEDS.get(name, 3))


_CACHE = {}


def _case(name):
    """(x fp32 [B, N, 3], k, ref_idx int64 ascending, tie bool [B, N], idx int16 of pv_arpe_knn), computed once and left unchanged."""
    if name not in _CACHE:
        N, B, k = SHAPES[name]
        x = torch.from_numpy(_points(name)).to(DEV)
        ref_idx, tie, ok = _neighbours(x, k)
        assert ok or name == "n4096", "the cloud violates the tie condition: choose another seed"
        assert int(tie.sum()) <= 32 or name == "dup"
        idx = ops.arpe_knn(x, k)
        torch.cuda.synchronize()
        _CACHE[name] = (x, k, ref_idx, tie, idx)
    return _CACHE[name]


# ---- restatements on stock ops, in any dtype ----
def _feat(x, idx, dtype, shift=None):
    """[x_q - shift, x_q - x_j] for every pair: [B, N, k, 6]."""
    x = x.to(dtype)
    N, k = x.shape[1], idx.shape[-1]
    nb = torch.gather(x.unsqueeze(1).expand(-1, N, -1, -1), 2, idx.long().unsqueeze(-1).expand(-1, -1, -1, 3))
    a = x if shift is None else x - shift.to(dtype)
    return torch.cat([a.unsqueeze(2).expand(-1, -1, k, -1), x.unsqueeze(2) - nb], dim=-1)


def _moments(f):
    """(F [6], G [6, 6]) of pair features f [..., 6]."""
    f = f.reshape(-1, 6)
    return f.sum(0), f.T @ f


def _winner(key):
    """key [B, N, k, 6] -> (position of the lowest-placed exact maximum [B, N, 6], the maximum [B, N, 1, 6])."""
    k = key.shape[2]
    mx = key.max(dim=2, keepdim=True).values
    pos = torch.arange(k, device=key.device).view(1, 1, k, 1).expand_as(key)
    return torch.where(key == mx, pos, k).min(dim=2).values, mx


def _bwd_sums(x, arg, y, g, w1, b1, dtype):
    """A [6], Z [6], C [6, 6] of the backward from the winners `arg`."""
    x, y, g, w1, b1 = (t.to(dtype) for t in (x, y, g, w1, b1))
    B, N, _ = x.shape
    xa = torch.gather(x.unsqueeze(1).expand(-1, N, -1, -1), 2, arg.long().unsqueeze(-1).expand(-1, -1, -1, 3))       # [B, N, 6, 3]
    fs = torch.cat([x.unsqueeze(2).expand(-1, -1, 6, -1), x.unsqueeze(2) - xa], dim=-1)                                # [B, N, 6 (c), 6 (i)]
    zs = (fs * w1.unsqueeze(0).unsqueeze(0)).sum(-1) + b1
    gp = g * torch.where(y > 0, torch.ones_like(y), y + 1)
    return gp.sum((0, 1)), (gp * zs).sum((0, 1)), torch.einsum("bnc,bnci->ci", gp, fs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the entry points
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_knn_lists_equal_the_sort_and_the_eval_kernel(name):
    x, k, ref_idx, tie, idx = _case(name)
    B, N, _ = x.shape
    assert idx.dtype == torch.int16 and tuple(idx.shape) == (B, N, k)
    assert bool((idx[..., 1:] > idx[..., :-1]).all()) if k > 1 else True                  # ascending
    assert bool((idx >= 0).all()) and bool((idx < N).all())
    if name == "dup":
        assert bool((idx.long() == ref_idx).all())           # equal distances are equal bits on both sides: lowest index first, everywhere
    assert bool((idx.long() == ref_idx)[~tie].all()), f"{int(((idx.long() != ref_idx).any(-1) & ~tie).sum())} queries chose other neighbours"
    if k == 1:
        assert bool((idx[..., 0].long() == torch.arange(N, device=DEV)).all())          # the point alone
    # the eval kernel's lists, value for value
    p = _params(4, 1)
    idx_eval = torch.full((B, N, k), -1, dtype=torch.int32, device=DEV)
    ops.arpe_embed(x, p["w1"], p["b1"], p["s1"], p["t1"], p["w2"], p["b2"], p["s2"], p["t2"], k, None, 0, idx_eval)
    assert torch.equal(idx.to(torch.int32), idx_eval)
    # two launches: identical bits, into a buffer that held something else
    idx2 = ops.arpe_knn(x, k, torch.full_like(idx, -1))
    assert torch.equal(idx, idx2)


@pytest.mark.parametrize("moved", [False, True], ids=["origin", "moved"])
@pytest.mark.parametrize("name", CASES)
def test_pair_moments_against_fp64(name, moved):
    x, k, _, _, idx = _case(name)
    if moved:                                         # a cloud far from the origin: its own neighbour lists
        x = (x + torch.tensor([50.0, -30.0, 10.0], device=DEV)).contiguous()
        idx = ops.arpe_knn(x, k)
    B, N, _ = x.shape
    M, G = B * N * k, B * ((N + 63) // 64)
    shift = x.mean(dim=(0, 1))
    part = ops.arpe_pair_moments(x, idx, shift)
    assert tuple(part.shape) == (G, 28) and bool((part[:, 27] == 0).all()) and bool(torch.isfinite(part).all())
    S = part.double().sum(0)
    f64 = _feat(x, idx, torch.float64, shift)
    F64, G64 = _moments(f64)
    Fabs, Gabs = _moments(f64.abs())
    iu = torch.triu_indices(6, 6, device=DEV)
    bound = 4 * U
    eF, eG = (S[:6] - F64).abs() / Fabs.clamp_min(1e-300), (S[6:27] - G64[iu[0], iu[1]]).abs() / Gabs[iu[0], iu[1]].clamp_min(1e-300)
    print(f"moments {name} moved={moved}: |dF| / sum|f| {float(eF.max()):.3g}, |dG| / sum|ff| {float(eG.max()):.3g}, bound {bound:.3g}")
    assert float(eF.max()) <= bound and float(eG.max()) <= bound
    # the finalised statistics of z against F.batch_norm's own fp32 result
    p = _params(4, 2)
    mu, v, Fo, XS = pct_train.finalize_moments(part, shift, p["w1"], p["b1"], M)
    z64 = F.linear(_feat(x, idx, torch.float64), p["w1"].double(), p["b1"].double()).reshape(M, 6)
    z32 = F.linear(_feat(x, idx, torch.float32), p["w1"], p["b1"]).reshape(M, 6)
    rm, rv = torch.zeros(6, device=DEV), torch.zeros(6, device=DEV)
    F.batch_norm(z32, rm, rv, training=True, momentum=1.0)
    _four_times(v, rv * ((M - 1) / M), z64.var(0, unbiased=False), f"variance {name} moved={moved}")
    _four_times(mu, rm, z64.mean(0), f"mean {name} moved={moved}")
    # F about the origin and XS = sigma * sum zhat f
    f0 = _feat(x, idx, torch.float64).reshape(M, 6)
    assert rel_l2(Fo, f0.sum(0)) <= 1e-5 or float((Fo - f0.sum(0)).abs().max()) <= bound * float(f0.abs().sum(0).max())
    assert rel_l2(XS, (z64 - z64.mean(0)).T @ f0) <= 1e-4
    assert torch.equal(part, ops.arpe_pair_moments(x, idx, shift, torch.full_like(part, 7.0)))


def _max_inputs(name):
    x, k, _, _, idx = _case(name)
    p = _params(4, 3)
    s = p["s1"].clone()                               # negative in channels 1 and 4 (_params)
    s[2] = 0.0
    assert int((s < 0).sum()) == 2 and int((s == 0).sum()) == 1
    return x, k, idx, p["w1"], p["b1"], s, p["t1"]


@pytest.mark.parametrize("name", CASES)
def test_pair_max_against_fp64(name):
    x, k, idx, w1, b1, s, t = _max_inputs(name)
    B, N, _ = x.shape
    y, arg = ops.arpe_pair_max(x, idx, w1, b1, s, t)
    assert bool(torch.isfinite(y).all()) and arg.dtype == torch.int16
    f64 = _feat(x, idx, torch.float64)
    z64 = F.linear(f64, w1.double(), b1.double())                                       # [B, N, k, 6]
    key = torch.sign(s).double() * z64
    first, mx = _winner(key)
    # arg: a neighbour; where the maximum is clear of the fp32 rounding of z, THE maximum, the lowest index among equal values
    member = idx.long().unsqueeze(-1) == arg.long().unsqueeze(2)                         # [B, N, k, 6]
    assert bool((member.sum(2) == 1).all())
    tol = 16 * U * F.linear(f64.abs(), w1.double().abs(), b1.double().abs()).max(dim=2, keepdim=True).values
    clear = ((key >= mx - tol) == (key == mx)).all(dim=2)
    want = torch.gather(idx.long(), 2, first)                                            # [B, N, 6]
    print(f"pair max {name}: {float(clear.double().mean()):.4f} of the maxima are clear")
    assert float(clear.double().mean()) >= 0.98 and bool((arg.long() == want)[clear].all())
    assert bool((torch.where(member, key, torch.zeros_like(key)).sum(2) >= (mx - tol).squeeze(2)).all())
    assert bool((arg[..., 2].long() == idx[..., 0].long()).all())                         # scale 0: the lowest-index neighbour
    if name == "dup":
        assert bool(clear.all())                                                         # copies of a point have equal z in any arithmetic
    y64 = F.elu(s.double() * torch.gather(z64, 2, first.unsqueeze(2)).squeeze(2) + t.double())
    y32 = F.elu(F.linear(_feat(x, idx, torch.float32), w1, b1) * s + t).max(dim=2).values
    _four_times(y, y32, y64, f"pair max {name}")
    y2, arg2 = ops.arpe_pair_max(x, idx, w1, b1, s, t, torch.full_like(y, 7.0), torch.full_like(arg, -1))
    assert torch.equal(y, y2) and torch.equal(arg, arg2)


@pytest.mark.parametrize("name", CASES)
def test_pair_bwd_sums_against_fp64(name):
    x, k, idx, w1, b1, s, t = _max_inputs(name)
    B, N, _ = x.shape
    y, arg = ops.arpe_pair_max(x, idx, w1, b1, s, t)          # the kernel's own winners (checked by test_pair_max_against_fp64)
    g = torch.randn(B, N, 6, generator=torch.Generator().manual_seed(N + k)).to(DEV)
    part = ops.arpe_pair_bwd(x, arg, y, g, w1, b1)
    assert tuple(part.shape) == (B * ((N + 63) // 64), 48)
    P = part.double().sum(0)
    ref64, ref32 = _bwd_sums(x, arg, y, g, w1, b1, torch.float64), _bwd_sums(x, arg, y, g, w1, b1, torch.float32)
    for got, r32, r64, what in zip((P[:6], P[6:12], P[12:].view(6, 6)), ref32, ref64, "AZC"):
        _four_times(got, r32, r64, f"pair bwd {name} {what}")
    assert torch.equal(part, ops.arpe_pair_bwd(x, arg, y, g, w1, b1, torch.full_like(part, 7.0)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the autograd function inside ARPE
# ---------------------------------------------------------------------------------------------------------------------------------
STEM = ("lin1.weight", "lin1.bias", "bn1.weight", "bn1.bias", "lin2.weight", "lin2.bias", "bn2.weight", "bn2.bias")


def _arpe(N, k, seed, dtype=torch.float32, momentum=0.1, D=32):
    """An ARPE with every parameter and running statistic drawn from `seed`; bn1.weight has both signs."""
    from peekvit_amd.models.pct import ARPE
    m = ARPE(3, D, N)
    m.k = k
    g = torch.Generator().manual_seed(seed)
    u = lambda *sh: torch.rand(*sh, generator=g) * 2 - 1
    with torch.no_grad():
        m.lin1.weight.copy_(u(6, 6) / 6 ** 0.5); m.lin1.bias.copy_(u(6) / 6 ** 0.5)
        m.bn1.weight.copy_((0.6 + torch.rand(6, generator=g)) * torch.tensor([1., -1., 1., 1., -1., 1.])); m.bn1.bias.copy_(0.3 * u(6))
        m.bn1.running_mean.copy_(0.2 * u(6)); m.bn1.running_var.copy_(0.5 + torch.rand(6, generator=g))
        m.lin2.weight.copy_(u(D, 6) / 6 ** 0.5); m.lin2.bias.copy_(u(D) / 6 ** 0.5)
        m.bn2.weight.copy_((0.6 + torch.rand(D, generator=g)) * torch.sign(u(D))); m.bn2.bias.copy_(0.3 * u(D))
    m.bn1.momentum = momentum
    return m.to(DEV, dtype)


def _same_winners(m32, x):
    """The fixture condition: the fp32 and the fp64 restatement of z pick the same neighbour for every (query, channel)."""
    from peekvit_amd.models.pct import knn_indices
    idx = knn_indices(x, m32.k)
    sg = torch.sign(m32.bn1.weight.detach())
    a = _winner(sg * F.linear(_feat(x, idx, torch.float32), m32.lin1.weight.detach(), m32.lin1.bias.detach()))[0]
    b = _winner(sg.double() * F.linear(_feat(x, idx, torch.float64), m32.lin1.weight.detach().double(), m32.lin1.bias.detach().double()))[0]
    return torch.equal(a, b)


def _stem_run(m, x, R, steps=1):
    """`steps` forwards (the last one with a backward of sum(out * R)): (out, {name: grad}, bn1 running statistics)."""
    for p in m.parameters():
        p.grad = None
    for _ in range(steps):
        out = m(x)
    (out * R.to(out.dtype)).sum().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.named_parameters()}
    return out.detach(), grads, (m.bn1.running_mean.clone(), m.bn1.running_var.clone(), int(m.bn1.num_batches_tracked))


@pytest.mark.parametrize("train,momentum", [(True, 0.1), (True, None), (False, 0.1)], ids=["train", "train-cumulative", "eval-with-grads"])
@pytest.mark.parametrize("N,B,k", [(80, 3, 5), (200, 2, 12)])
def test_arpe_matches_the_composite_autograd(N, B, k, train, momentum, monkeypatch):
    x = torch.from_numpy(synth.synth_points(B, N, seed=3)).to(DEV)
    assert _neighbours(x, k)[2], "the cloud violates the tie condition: choose another seed"
    R = torch.randn(B, N, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    mods = {tag: _arpe(N, k, 11, dt, momentum).train(train) for tag, dt in (("hip", torch.float32), ("stock", torch.float32), ("f64", torch.float64))}
    assert _same_winners(mods["stock"], x), "fp32 and fp64 pick other neighbours in the max: choose another seed"
    for steps in (1, 2):
        res = {}
        for tag, m in mods.items():
            monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip" if tag == "hip" else "torch")
            n0 = pct_train.stem_passes
            res[tag] = _stem_run(m, x.double() if tag == "f64" else x, R, steps=1)          # (the second round is the second forward)
            assert pct_train.stem_passes - n0 == (1 if tag == "hip" else 0), tag
        what = f"ARPE N={N} train={train} momentum={momentum} forward {steps}"
        _four_times(res["hip"][0], res["stock"][0], res["f64"][0], what + " output")
        for n in STEM:
            got, r32, r64 = (res[tag][1][n] for tag in ("hip", "stock", "f64"))
            if train and n in ("lin1.bias", "lin2.bias"):          # true gradient 0 (BatchNorm removes the bias): max abs alone
                m_ref, m_got = float((r32.double() - r64).abs().max()), float((got.double() - r64).abs().max())
                print(f"{what} {n}: max abs {m_got:.3g} (stock fp32 {m_ref:.3g})")
                assert m_got <= 4 * m_ref
                if n == "lin1.bias":
                    assert bool((got == 0).all())
            else:
                _four_times(got, r32, r64, f"{what} {n}")
        (rm, rv, nb), (rm32, rv32, nb32), (rm64, rv64, nb64) = res["hip"][2], res["stock"][2], res["f64"][2]
        assert nb == nb32 == nb64 == (steps if train else 0)
        if train:
            _four_times(rm, rm32, rm64, what + " running_mean")
            _four_times(rv, rv32, rv64, what + " running_var")
        else:
            assert torch.equal(rm, rm32) and torch.equal(rv, rv32)                             # frozen statistics stay


def test_arpe_frozen_parameters_and_fallbacks(monkeypatch):
    N, B, k = 80, 3, 5
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND", raising=False)
    x = torch.from_numpy(synth.synth_points(B, N, seed=3)).to(DEV)
    m = _arpe(N, k, 11).train()
    m.lin1.bias.requires_grad_(False)
    m.bn1.weight.requires_grad_(False)
    n0, b0 = pct_train.stem_passes, pct_train.stem_backwards
    m(x).square().sum().backward()
    assert pct_train.stem_passes == n0 + 1 and pct_train.stem_backwards == b0 + 1
    assert m.lin1.bias.grad is None and m.bn1.weight.grad is None
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in m.named_parameters() if n not in ("lin1.bias", "bn1.weight"))
    # two runs of forward + backward from one state: identical bits
    a, b = _arpe(N, k, 11).train(), _arpe(N, k, 11).train()
    ya, yb = a(x), b(x)
    ya.square().sum().backward(); yb.square().sum().backward()
    assert torch.equal(ya, yb) and all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    assert torch.equal(a.bn1.running_var, b.bn1.running_var)
    # the composite: points that require grad, autocast, no_grad, the knobs
    n0 = pct_train.stem_passes
    xg = x.clone().requires_grad_(True)
    m(xg).sum().backward()
    assert xg.grad is not None and pct_train.stem_passes == n0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        m(x)
    with torch.no_grad():
        m(x)
        m.eval()(x)
    m.train()
    monkeypatch.setenv("PEEKVIT_AMD_BACKEND", "torch")
    m(x)
    monkeypatch.delenv("PEEKVIT_AMD_BACKEND")
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "torch")
    m(x)
    assert pct_train.stem_passes == n0
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    m(x)
    assert pct_train.stem_passes == n0 + 1


def test_saved_tensors_do_not_scale_with_k(monkeypatch):
    monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip")
    B, N = 8, 1024
    m = _arpe(N, 64, 11, D=128).train()
    x = torch.from_numpy(synth.synth_points(B, N, seed=1)).to(DEV)
    y = pct_train.pair_stage(m, x)
    assert "PairStage" in type(y.grad_fn).__name__
    held = sum(t.numel() * t.element_size() for t in y.grad_fn.saved_tensors)
    print(f"saved by the pair stage: {held} bytes, {held / (B * N):.1f} a point; one [B N, k, 6] fp32 tensor: {B * N * 64 * 6 * 4}")
    assert held < B * N * 64 * 6 * 4 and held <= 50 * B * N          # points 12 + y 24 + arg 12 bytes a point, and the 6 x 6 quantities


# ---------------------------------------------------------------------------------------------------------------------------------
# one training step of the models
# ---------------------------------------------------------------------------------------------------------------------------------
ZERO_GRAD = ("embedder.lin1.bias", "embedder.lin2.bias", "head.lin1.bias")          # biases in front of a batch-statistics BatchNorm


def _model(cname, kw, dtype):
    from peekvit_amd.models import pct
    m = getattr(pct, cname)(**kw)
    sd = synth.pct_state_dict({k: v for k, v in kw.items() if k in ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes",
                                                                     "num_registers", "num_class_tokens")}, 0)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        m.embedder.bn1.weight.mul_(torch.tensor([1., -1., 1., 1., -1., 1.]))          # both signs in front of the max
    m.head.dp.p = 0.0          # the head's dropout draws other masks in fp64 than in fp32: off in all three models, it is not under test
    if cname == "RankPointCloudTransformer":
        m.enable_ranking(True)
        m.set_budget(0.5)
    return m.to(DEV, dtype).train()


@pytest.mark.parametrize("cname", ["PointCloudTransformer", "RankPointCloudTransformer"])
def test_one_training_step_with_the_path_on_and_off(cname, monkeypatch):
    from peekvit_amd.models import pct
    kw = dict(META["cases"]["pct_n128"]["kwargs"])
    B, N, L = 16, kw["num_points"], kw["num_layers"]          # (16 clouds: the head's BatchNorm divides by a deviation over the batch)
    x = torch.from_numpy(synth.synth_points(B, N, seed=3)).to(DEV)
    target = (torch.arange(B, device=DEV) * 7 + 1) % kw["num_classes"]
    zero_grad = ZERO_GRAD + (f"encoder.layers.{L - 1}.mlp.fc2.bias",)          # a constant added to every pooled vector: the head's BatchNorm removes it
    kept = {}
    order0 = pct.RankingPCTBlock.sort_order

    def recording(tag):
        def sort_order(inp):
            order = order0(inp)
            keep = 1 + math.ceil((inp.shape[1] - 1) * 0.5)
            kept.setdefault(tag, []).append(torch.sort(order[:, :keep], dim=-1).values)
            return order
        return staticmethod(sort_order)

    models = {tag: _model(cname, kw, dt) for tag, dt in (("hip", torch.float32), ("stock", torch.float32), ("f64", torch.float64))}
    assert _neighbours(x, models["hip"].embedder.k)[2] and _same_winners(models["stock"].embedder, x), "choose another seed"
    eval_model = copy.deepcopy(models["hip"]).eval()
    with torch.no_grad():
        logits0 = eval_model(x).clone()
    out = {}
    for tag, m in models.items():
        monkeypatch.setenv("PEEKVIT_AMD_TRAIN", "hip" if tag == "hip" else "torch")
        monkeypatch.setattr(pct.RankingPCTBlock, "sort_order", recording(tag))
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        n0, b0 = pct_train.stem_passes, pct_train.stem_backwards
        loss = F.cross_entropy(m(x.double() if tag == "f64" else x), target)
        opt.zero_grad()
        loss.backward()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        opt.step()
        torch.cuda.synchronize()
        on = 1 if tag == "hip" else 0
        assert (pct_train.stem_passes - n0, pct_train.stem_backwards - b0) == (on, on), tag          # the counter shows which path ran
        assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
        out[tag] = (loss.detach(), grads)
    monkeypatch.setattr(pct.RankingPCTBlock, "sort_order", staticmethod(order0))
    if cname == "RankPointCloudTransformer":
        assert len(kept["hip"]) == kw["num_layers"]
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(kept["hip"], kept["stock"], kept["f64"])), \
            "the three runs mask other tokens: choose another seed"
    _four_times(out["hip"][0].reshape(1), out["stock"][0].reshape(1), out["f64"][0].reshape(1), f"{cname} loss")
    assert set(out["hip"][1]) == set(out["stock"][1]) == set(out["f64"][1]) and "class_tokens" not in out["hip"][1]
    for n in sorted(out["hip"][1]):
        got, r32, r64 = (out[tag][1][n] for tag in ("hip", "stock", "f64"))
        if n in zero_grad:
            assert float(r64.abs().max()) <= 1e-9 * max(float(g.abs().max()) for g in out["f64"][1].values()), n          # zero indeed
            m_ref, m_got = float((r32.double() - r64).abs().max()), float((got.double() - r64).abs().max())
            print(f"{cname} {n}: max abs {m_got:.3g} (stock fp32 {m_ref:.3g})")
            assert m_got <= 4 * m_ref
        else:
            _four_times(got, r32, r64, f"{cname} {n}")
    # the inference path is unaffected by the calls above
    with torch.no_grad():
        assert torch.equal(eval_model(x), logits0)
