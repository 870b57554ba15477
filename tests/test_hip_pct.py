"""Point-cloud transformer on the MI355X (include/peekvit_hip_pct.h, peekvit_amd.engine.pct_forward): the four entry points against float64
restatements in plain torch ops, then PointCloudTransformer against the reference's golden outputs (scripts/make_golden_pct.py).

Tolerances of the fp32 kernels follow one rule: the same computation on stock fp32 torch ops is measured against the float64 restatement,
and the kernel may be four times as far from it (a different summation order and fused multiply-adds).  The model-level bound is BASELINE's
1e-3 relative L2 on the logits."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from peekvit_amd import _lib, engine, ops, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META = json.load(open(os.path.join(GOLDEN, "pct_meta.json")))
TIE_ULPS = 32


# ---------------------------------------------------------------------------------------------------------------------------------
# pv_arpe_embed
# ---------------------------------------------------------------------------------------------------------------------------------
def _params(D, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    p = dict(w1=u(6, 6) / 6 ** 0.5, b1=u(6) / 6 ** 0.5, s1=(0.6 + torch.rand(6, generator=g)) * torch.tensor([1., -1., 1., 1., -1., 1.]),
             t1=0.3 * u(6), w2=u(D, 6) / 6 ** 0.5, b2=u(D) / 6 ** 0.5, s2=(0.6 + torch.rand(D, generator=g)) * torch.sign(u(D)), t2=0.3 * u(D))
    return {k: v.float().contiguous().to(DEV) for k, v in p.items()}


def _dist32(x):
    """fp32 squared distances, (dx*dx + dy*dy) + dz*dz with every operation rounded: the kernel's definition.  x [B, N, 3] on the GPU."""
    dx = x[:, :, None, 0] - x[:, None, :, 0]
    dy = x[:, :, None, 1] - x[:, None, :, 1]
    dz = x[:, :, None, 2] - x[:, None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _neighbours(x, k):
    """(idx int64 [B, N, k] by a stable (distance, index) sort, ascending index; tie bool [B, N]: more than one candidate within 32 ulp of the
    k-th smallest distance; ok: every such group is copies of one coordinate triple)."""
    d = _dist32(x)
    srt, order = torch.sort(d, dim=-1, stable=True)
    idx = torch.sort(order[..., :k], dim=-1).values
    kth = srt[..., k - 1]
    ulp = torch.from_numpy(np.spacing(kth.cpu().numpy())).to(x.device).double()
    near = (d.double() - kth.double().unsqueeze(-1)).abs() <= TIE_ULPS * ulp.unsqueeze(-1)
    tie = near.sum(-1) > 1
    ok = True
    for b, q in torch.nonzero(tie).tolist():
        c = x[b, near[b, q]]
        ok = ok and bool((c == c[0]).all())
    return idx, tie, ok


def _arpe_torch(x, idx, p, dtype):
    """The stem on stock ops in `dtype`, on given neighbour sets: models/pct.py:84-88 with BatchNorm at eval as scale and shift."""
    x = x.to(dtype)
    P = {k: v.to(dtype) for k, v in p.items()}
    B, N, _ = x.shape
    knn = torch.gather(x.unsqueeze(1).expand(-1, N, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, 3))
    feat = torch.cat([x.unsqueeze(2).expand(-1, -1, idx.shape[-1], -1), x.unsqueeze(2) - knn], dim=-1)
    y = F.elu(F.linear(feat, P["w1"], P["b1"]) * P["s1"] + P["t1"]).max(dim=2).values
    return F.elu(F.linear(y, P["w2"], P["b2"]) * P["s2"] + P["t2"])


def _run_arpe(x, p, k, row_off=0, extra=0):
    B, N, _ = x.shape
    D = p["w2"].shape[0]
    tokens = torch.full((B, row_off + N + extra, D), -777.0, device=DEV)
    idx = torch.full((B, N, k), -1, dtype=torch.int32, device=DEV)
    ops.arpe_embed(x, p["w1"], p["b1"], p["s1"], p["t1"], p["w2"], p["b2"], p["s2"], p["t2"], k, tokens, row_off, idx)
    torch.cuda.synchronize()
    return tokens, idx


def _four_times(got, ref32, ref64, what):
    """got within four times the stock fp32 ops' own distance from the fp64 restatement, in relative L2 and in max abs."""
    e_ref, e_got = rel_l2(ref32, ref64), rel_l2(got, ref64)
    m_ref, m_got = float((ref32.double() - ref64).abs().max()), float((got.double() - ref64).abs().max())
    print(f"{what}: rel L2 {e_got:.3g} (stock fp32 {e_ref:.3g}), max abs {m_got:.3g} (stock fp32 {m_ref:.3g})")
    assert e_got <= 4 * e_ref and m_got <= 4 * m_ref, (what, e_got, e_ref, m_got, m_ref)


@pytest.mark.parametrize("N,B,D,row_off", [(16, 3, 128, 0), (48, 3, 132, 2), (80, 3, 128, 0), (1000, 3, 128, 2), (1024, 3, 260, 0),
                                           (2048, 1, 128, 2), (4096, 1, 128, 0)])
def test_arpe_embed_against_fp64(N, B, D, row_off):
    """Seeds: the first one at which the cloud satisfies the tie condition (scripts/make_golden_pct.py).  A uniform cloud of 4096 points has
    about six queries whose k-th and (k+1)-th distances, of two DISTINCT points, lie within 32 ulp (none of seeds 0 - 59 is free of them), so at
    that size the condition is applied per query: those queries are left out of both comparisons, the other ~4090 are held to them."""
    k = N // 16
    p = _params(D, N)
    x = torch.from_numpy(synth.synth_points(B, N, seed={1000: 0, 2048: 9}.get(N, 3))).to(DEV)
    ref_idx, tie, ok = _neighbours(x, k)
    assert ok or N == 4096, "the cloud violates the tie condition: choose another seed"
    assert int(tie.sum()) <= 32
    tokens, idx = _run_arpe(x, p, k, row_off, extra=1)
    # rows outside [row_off, row_off + N) untouched
    assert bool((tokens[:, :row_off] == -777.0).all()) and bool((tokens[:, row_off + N:] == -777.0).all())
    emb = tokens[:, row_off:row_off + N]
    assert bool(torch.isfinite(emb).all())
    # neighbour sets: ascending, and equal to the stable (distance, index) sort wherever the boundary is not a tie
    assert bool((idx[..., 1:] > idx[..., :-1]).all()) if k > 1 else True
    assert bool((idx.long() == ref_idx)[~tie].all()), f"{int(((idx.long() != ref_idx).any(-1) & ~tie).sum())} queries chose other neighbours"
    if k == 1:
        assert bool((idx[..., 0].long() == torch.arange(N, device=DEV)).all())          # the point alone
    ref64 = _arpe_torch(x, ref_idx, p, torch.float64)
    ref32 = _arpe_torch(x, ref_idx, p, torch.float32)
    _four_times(emb[~tie], ref32[~tie], ref64[~tie], f"arpe N={N} D={D}")
    # two launches on the same input: identical bits
    tokens2, idx2 = _run_arpe(x, p, k, row_off, extra=1)
    assert torch.equal(tokens, tokens2) and torch.equal(idx, idx2)
    # without idx_out: the same tokens
    t3 = torch.full_like(tokens, -777.0)
    ops.arpe_embed(x, p["w1"], p["b1"], p["s1"], p["t1"], p["w2"], p["b2"], p["s2"], p["t2"], k, t3, row_off, None)
    assert torch.equal(tokens, t3)


def test_arpe_embed_duplicates_beyond_k():
    N, B, k, D = 80, 3, 5, 128
    p = _params(D, 5)
    xs = synth.synth_points(B, N, seed=4)
    xs[:, 10:30] = xs[:, 3:4]                          # 21 rows of one coordinate triple, k = 5
    xs[1, 40:52] = xs[1, 0:1]
    x = torch.from_numpy(xs).to(DEV)
    ref_idx, tie, ok = _neighbours(x, k)
    assert ok and int(tie.sum()) >= 20 * B
    tokens, idx = _run_arpe(x, p, k)
    assert bool((idx.long() == ref_idx).all())           # equal distances are equal bits on both sides: lowest index first, everywhere
    _four_times(tokens, _arpe_torch(x, ref_idx, p, torch.float32), _arpe_torch(x, ref_idx, p, torch.float64), "arpe duplicates")


def test_arpe_embed_exact_tie_between_distinct_points_goes_to_the_lowest_index():
    N, k, D, a = 48, 3, 128, 0.25
    g = torch.Generator().manual_seed(9)
    v = torch.randn(2, N, 3, generator=g)
    xs = v / v.norm(dim=-1, keepdim=True) * (0.7 + 0.3 * torch.rand(2, N, 1, generator=g))      # everything else at radius >= 0.7
    for b, (lo, hi) in enumerate(((2, 7), (40, 11))):
        xs[b, 5] = 0.0                                                      # the query
        xs[b, 20] = torch.tensor([0.0, a / 2, 0.0])                        # its nearest other point
        xs[b, lo] = torch.tensor([-a, 0.0, 0.0]) if b == 0 else torch.tensor([0.0, 0.0, a])
        xs[b, hi] = -xs[b, lo]                                               # the same distance, another point
    x = xs.float().contiguous().to(DEV)
    p = _params(D, 6)
    _, idx = _run_arpe(x, p, k)
    assert idx[0, 5].tolist() == [2, 5, 20] and idx[1, 5].tolist() == [5, 11, 20]
    ref_idx, _, _ = _neighbours(x, k)
    assert bool((idx.long() == ref_idx).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# pv_layernorm_f32_bf16
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand", ["bf16", "f16"])
@pytest.mark.parametrize("D,strided", [(128, False), (132, False), (128, True), (516, True)])
def test_layernorm_both_planes(D, strided, operand):
    rows = 301
    g = torch.Generator().manual_seed(D)
    wide = (torch.randn(rows, D + 8, generator=g) * 1.7 + 0.3).to(DEV)
    x = wide[:, :D] if strided else wide[:, :D].contiguous()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
    with engine.precision(operand):
        od = _lib.operand_dtype()
        want = torch.empty((rows, D), dtype=od, device=DEV)
        ops.layernorm_bf16(x.contiguous(), gamma, beta, 1e-5, want)
        o16, o32 = torch.empty((rows, D), dtype=od, device=DEV), torch.empty((rows, D), dtype=torch.float32, device=DEV)
        ops.layernorm_f32_bf16(x, gamma, beta, 1e-5, o16, o32)
    torch.cuda.synchronize()
    assert od == (torch.float16 if operand == "f16" else torch.bfloat16)
    assert torch.equal(o16.view(torch.int16), want.view(torch.int16))
    assert torch.equal(o32.to(od).view(torch.int16), o16.view(torch.int16))          # the fp32 plane is the value before that rounding
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    assert rel_l2(o32, ref) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# pv_mean_pool_f32, pv_pct_head_f32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 65, 1026])
@pytest.mark.parametrize("D", [128, 4])
def test_mean_pool_against_fp64(S, D):
    B = 5
    g = torch.Generator().manual_seed(S * 7 + D)
    x = (torch.randn(B, S, D, generator=g) + 0.5).to(DEV)
    got = ops.mean_pool(x)
    ref64 = x.double().mean(dim=1)
    ref32 = torch.mean(x, dim=1)
    e_ref, e_got = rel_l2(ref32, ref64), rel_l2(got, ref64)
    m_ref, m_got = float((ref32.double() - ref64).abs().max()), float((got.double() - ref64).abs().max())
    print(f"mean pool S={S} D={D}: rel L2 {e_got:.3g} (torch.mean {e_ref:.3g}), max abs {m_got:.3g} ({m_ref:.3g})")
    # the four-times rule; its floor is one rounding of the result itself (half an ulp of the largest mean), which no fp32 output avoids
    half_ulp = float(ref64.abs().max()) * 2.0 ** -24
    assert e_got <= max(4 * e_ref, 2.0 ** -24) and m_got <= max(4 * m_ref, half_ulp)
    assert torch.equal(got, ops.mean_pool(x))


@pytest.mark.parametrize("B", [3, 40])
@pytest.mark.parametrize("D,C", [(128, 40), (4, 3)])
def test_pct_head_against_fp64(B, D, C):
    Hd = D // 2
    g = torch.Generator().manual_seed(B + D)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)
    pooled = torch.randn(B, D, generator=g).to(DEV)
    w1, b1 = (u(Hd, D) / D ** 0.5).to(DEV), (u(Hd) / D ** 0.5).to(DEV)
    s, t = ((0.6 + torch.rand(Hd, generator=g)) * torch.sign(u(Hd))).to(DEV), (0.3 * u(Hd)).to(DEV)
    w2, b2 = (u(C, Hd) / Hd ** 0.5).to(DEV), (u(C) / Hd ** 0.5).to(DEV)
    got = ops.pct_head(pooled, w1, b1, s, t, w2, b2)

    def ref(dt):
        h = F.gelu(F.linear(pooled.to(dt), w1.to(dt), b1.to(dt)) * s.to(dt) + t.to(dt))
        return F.linear(h, w2.to(dt), b2.to(dt))
    _four_times(got, ref(torch.float32), ref(torch.float64), f"pct head B={B} D={D} C={C}")
    assert torch.equal(got[:1], ops.pct_head(pooled[:1].contiguous(), w1, b1, s, t, w2, b2))          # a row does not depend on the batch


# ---------------------------------------------------------------------------------------------------------------------------------
# PointCloudTransformer
# ---------------------------------------------------------------------------------------------------------------------------------
def _synth_cfg(kw):
    return {k: v for k, v in kw.items() if k in ("num_points", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes", "num_registers",
                                                 "num_class_tokens")}


def _model(kw, device=DEV):
    from peekvit.models.pct import PointCloudTransformer
    m = PointCloudTransformer(**kw).eval()
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.pct_state_dict(_synth_cfg(kw), 0).items()}, strict=True)
    return m.to(device)


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        info = META["cases"][name]
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        _CACHE[name] = (_model(info["kwargs"]), torch.from_numpy(z["points"]).to(DEV), torch.from_numpy(z["logits"]), torch.from_numpy(z["embedding"]), info)
    return _CACHE[name]


def _hip(model, x, mode="auto"):
    """The forward in `mode`, with the number of launches it made."""
    n0 = ops.launch_count
    with torch.no_grad(), engine.precision(mode):
        y = model(x)
    torch.cuda.synchronize()
    return y, ops.launch_count - n0


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_model_matches_the_reference_logits(name):
    model, x, logits, emb, info = _case(name)
    y, launches = _hip(model, x)
    L = info["kwargs"]["num_layers"]
    assert launches >= 1 + 7 * L + 2 and engine.last_forward_guarded()          # the kernels ran, and the result is theirs
    err = rel_l2(y, logits)
    print(f"{name}: auto {err:.3g}")
    assert err <= 1e-3
    # the stem alone, fp32: four times as far from the float64 composite as the reference's own embedding is
    with torch.no_grad():
        tok = engine.pct_embed(model, x)
        ref64 = _model(info["kwargs"], "cpu").double().embedder(x.cpu().double())
    nr = info["kwargs"].get("num_registers", 0)
    _four_times(tok[:, nr:].cpu(), emb, ref64, f"{name}: embedding")
    # fp16 / bf16 operands without the self-check: measured, recorded in DESIGN.md section 18; no bound tighter than 1e-3 is asserted on them
    for mode in ("f16", "bf16"):
        ym, n = _hip(model, x, mode)
        print(f"{name}: {mode} {rel_l2(ym, logits):.3g}")
        assert n >= 1 + 7 * L + 2 and bool(torch.isfinite(ym).all()) and rel_l2(ym, logits) < 5e-2
    # bf16x3: the composite, no launch of ours
    y3, n3 = _hip(model, x, "bf16x3")
    assert n3 == 0 and rel_l2(y3, logits) <= 1e-3


def test_model_batch_one_and_two_registers():
    model, x, logits, _, info = _case("pct_n128")
    y, n = _hip(model, x[:1].contiguous())
    assert n > 0 and rel_l2(y, logits[:1]) <= 1e-3
    kw = dict(info["kwargs"], num_registers=2)
    m2 = _model(kw)
    with torch.no_grad():
        want = _model(kw, "cpu")(x.cpu())
    y2, n2 = _hip(m2, x)
    assert n2 > 0 and rel_l2(y2, want) <= 1e-3


def test_graph_replay_is_bit_identical_to_the_eager_forward():
    from peekvit_amd.graph import GraphedForward
    model, x, logits, _, _ = _case("pct_n64r1")
    eager, _ = _hip(model, x)
    eager = eager.clone()
    g = GraphedForward(model, x)
    y = g(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(y, eager) and rel_l2(y, logits) <= 1e-3
    assert torch.equal(g(x), eager)


def test_other_widths():
    x = torch.from_numpy(synth.synth_points(2, 64, seed=1)).to(DEV)
    # dh = 48 runs the kernels
    kw = dict(num_points=64, num_layers=2, num_heads=4, hidden_dim=192, mlp_dim=384, num_classes=10)
    m = _model(kw)
    with torch.no_grad():
        want = _model(kw, "cpu")(x.cpu())
    y, n = _hip(m, x)
    assert n >= 17 and rel_l2(y, want) <= 1e-3
    # a width the GEMMs do not take: the composite, on the GPU
    kw = dict(num_points=64, num_layers=2, num_heads=2, hidden_dim=130, mlp_dim=256, num_classes=10)
    m = _model(kw)
    assert not engine.pct_supported(m)
    with torch.no_grad():
        want = _model(kw, "cpu")(x.cpu())
    y, n = _hip(m, x)
    assert n == 0 and rel_l2(y, want) <= 1e-3
