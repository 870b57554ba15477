"""Routed top-1 mixture of experts on the MI355X (include/peekvit_hip_moe.h, peekvit_amd.engine.moe_forward): the three entry points against
float64 restatements in plain torch ops and against the kernels they must match bit for bit, then VisionTransformerMoE against the reference's
golden outputs (scripts/make_golden_moe.py), the all-ones model against VisionTransformer, hipGraph replay, and a ViT-B/16-sized batch."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from peekvit_amd import _lib, engine, ops, synth
from peekvit_amd._lib import PV_EPI_BIAS_GELU_BF16, PV_EPI_BIAS_RES_F32

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META = json.load(open(os.path.join(GOLDEN, "moe_meta.json")))
T = ops.MOE_TILE_ROWS


def _buffers(M, D, E, xln=True):
    """The outputs of pv_moe_route, each filled with a sentinel no launch writes (NaN for floats; expert ids, offsets and tile owners are
    >= -1, so -7): a row that was never written is visible."""
    Mp = ops.moe_packed_rows(M, E)
    return dict(expert=torch.full((M,), -7, dtype=torch.int32, device=DEV), seg=torch.full((E + 1,), -7, dtype=torch.int32, device=DEV),
                perm=torch.full((Mp,), -7, dtype=torch.int32, device=DEV), tiles=torch.full((Mp // T,), -7, dtype=torch.int32, device=DEV),
                gap=torch.full((M,), float("nan"), dtype=torch.float32, device=DEV),
                probs=torch.full((M, E), float("nan"), dtype=torch.float32, device=DEV),
                xln=torch.full((Mp, D), float("nan"), dtype=_lib.operand_dtype(), device=DEV) if xln else None)


def _route(x, gamma, beta, W, bg, xln=True, eps=1e-5):
    M, D = x.shape
    E = W.shape[0]
    r = _buffers(M, D, E, xln)
    ops.moe_route(x, gamma, beta, eps, W, bg, r["expert"], r["seg"], r["perm"], r["tiles"], xln=r["xln"], gap=r["gap"], probs=r["probs"])
    torch.cuda.synchronize()
    return r


def _raw(t):
    """A tensor's bits as integers (fp32 -> int32, 16-bit operands -> int16)."""
    return t if t.dtype == torch.int32 else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _route_inputs(M, D, E, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, D, generator=g) * 2 + 0.5).to(DEV)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    beta = (0.05 * torch.randn(D, generator=g)).to(DEV)
    W = ((torch.rand(E, D, generator=g) * 2 - 1) / D ** 0.5).to(DEV)
    bg = (0.02 * torch.randn(E, generator=g))
    return x, gamma, beta, W, bg


def _check_layout(r, M, E):
    """seg / perm / tile table: complete, stable, padded to 256 rows, -1 on every pad row."""
    ex = r["expert"].cpu().long()
    seg, perm, tiles = r["seg"].cpu().long(), r["perm"].cpu().long(), r["tiles"].cpu().long()
    Mp = perm.numel()
    assert Mp == ops.moe_packed_rows(M, E) and seg[0] == 0
    assert bool(((ex >= 0) & (ex < E)).all())
    counts = torch.bincount(ex, minlength=E)
    live = torch.zeros(Mp, dtype=torch.bool)
    for e in range(E):
        c = int(counts[e])
        assert int(seg[e + 1] - seg[e]) == (c + T - 1) // T * T
        rows = torch.nonzero(ex == e).flatten()
        assert torch.equal(perm[seg[e]:seg[e] + c], rows)                  # ascending source rows: stable
        live[seg[e]:seg[e] + c] = True
        assert bool((tiles[seg[e] // T:seg[e + 1] // T] == e).all())
    assert bool((perm[~live] == -1).all()) and int(live.sum()) == M
    assert bool((tiles[seg[E] // T:] == -1).all())
    return live


# The first seven: D = 256 (NCH = 1), ids as before D became a parameter.
# "width": every PV_DISPATCH_NCH bucket of the gate and scatter kernels (NCH 1, 2, 3, 4, 8 partly filled, 16 partly filled, 16 full).
# "carry": 1 028 histogram blocks - pv_moe_scan_kernel's running sum crosses into a second 1024-block chunk.
# "tail":  every row to expert 63 of 64 - 16 384 packed rows behind seg[E], a second trip of the 32 shared tail blocks' perm loop.
ROUTE_CASES = [pytest.param(1000, 256, 2, "plain", id="1000-2-plain"), pytest.param(777, 256, 3, "plain", id="777-3-plain"),
               pytest.param(4099, 256, 8, "plain", id="4099-8-plain"), pytest.param(300, 256, 64, "plain", id="300-64-plain"),
               pytest.param(256, 256, 8, "plain", id="256-8-plain"), pytest.param(2000, 256, 8, "empty", id="2000-8-empty"),
               pytest.param(1500, 256, 8, "one", id="1500-8-one"),
               (300, 12, 3, "width"), (777, 260, 3, "width"), (500, 768, 8, "width"), (300, 1024, 4, "width"), (300, 1536, 5, "width"),
               (260, 2052, 2, "width"), (257, 4096, 64, "width"),
               (263000, 64, 5, "carry"), (300, 128, 64, "tail")]


@pytest.mark.parametrize("M,D,E,mode", ROUTE_CASES)
def test_route_against_fp64(M, D, E, mode):
    """Expert = the fp64 argmax on every clear row (fp64 gap > 1e-5), gap within 2e-5 of fp64, one-hot probs, the packed layout in full, the
    packed LayerNorm rows bit-identical to pv_layernorm_bf16, two runs with identical bits.
    How many rows may be unclear.  On the CPU, with this recipe, stock fp32 ops are within 1.4e-6 of the fp64 gap at every "width" shape and
    within 1.1e-6 at the "carry" shape (the gap tolerance keeps a >= 14x margin over the reference's own error), and pick the fp64 expert on
    every row.  No row of a "width" shape has an fp64 gap <= 2e-5: none may be left out as unclear.  13 of the 263 000 "carry" rows have
    one: at most 1 row in 10 000 may be left out."""
    x, gamma, beta, W, bg = _route_inputs(M, D, E, M * 131 + E + (D if mode in ("width", "carry", "tail") else 0))
    if mode == "empty":
        bg[: E // 2] -= 50.0                  # the first half of the experts never wins: empty segments
    if mode in ("one", "tail"):
        bg[E - 1] += 50.0                     # every row to the last expert
    bg = bg.to(DEV)
    r = _route(x, gamma, beta, W, bg)
    # float64 restatement: LayerNorm, gate, top-2
    y = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    logits = y @ W.double().t() + bg.double()
    top = logits.topk(min(2, E), dim=-1).values
    gap64 = (top[:, 0] - top[:, 1]).cpu()
    ex = r["expert"].cpu().long()
    clear = gap64 > 1e-5
    if mode == "width":
        assert bool(clear.all()), f"{int((~clear).sum())} rows left out as unclear"
    if mode == "carry":
        assert int((~clear).sum()) <= M // 10000, f"{int((~clear).sum())} rows left out as unclear"
    assert torch.equal(ex[clear], logits.argmax(-1).cpu()[clear])
    np.testing.assert_allclose(r["gap"].cpu().double().numpy(), gap64.numpy(), rtol=0, atol=2e-5)
    assert torch.equal(r["probs"].cpu(), F.one_hot(ex, E).float())
    if mode == "empty":
        assert int((ex < E // 2).sum()) == 0
    if mode in ("one", "tail"):
        assert bool((ex == E - 1).all())
    live = _check_layout(r, M, E)
    if mode == "tail":                        # one padded segment, then nothing: perm = -1, zero rows, dead tiles all the way to M_pad
        first = (M + T - 1) // T * T
        assert r["seg"].cpu().tolist() == [0] * E + [first] and r["perm"].numel() - first >= 16000
        assert bool((r["perm"][first:] == -1).all()) and bool((r["tiles"][first // T:] == -1).all())
        assert bool((r["xln"][first:].view(torch.int16) == 0).all())
    # the packed LayerNorm rows: pv_layernorm_bf16's rows gathered by perm, bit for bit; zeros on pad rows
    h = torch.empty((M, D), dtype=_lib.operand_dtype(), device=DEV)
    ops.layernorm_bf16(x, gamma, beta, 1e-5, h)
    perm = r["perm"].long()
    xln = r["xln"]
    assert torch.equal(xln[live.to(DEV)].view(torch.int16), h[perm[live.to(DEV)]].view(torch.int16))
    assert bool((xln[~live.to(DEV)].view(torch.int16) == 0).all())
    # two runs: identical bits
    r2 = _buffers(M, D, E)
    ops.moe_route(x, gamma, beta, 1e-5, W, bg, r2["expert"], r2["seg"], r2["perm"], r2["tiles"], xln=r2["xln"], gap=r2["gap"], probs=r2["probs"])
    torch.cuda.synchronize()
    for k in ("expert", "seg", "perm", "tiles", "gap", "probs", "xln"):
        assert torch.equal(r[k].view(torch.int32) if r[k].dtype == torch.float32 else r[k].view(torch.int16) if r[k].dtype != torch.int32 else r[k],
                           r2[k].view(torch.int32) if r2[k].dtype == torch.float32 else r2[k].view(torch.int16) if r2[k].dtype != torch.int32 else r2[k]), k


def test_route_exact_tie_and_single_expert():
    M, D = 700, 128
    x = torch.randn(M, D, generator=torch.Generator().manual_seed(5)).to(DEV)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    for E in (2, 5):
        r = _route(x, gamma, beta, torch.zeros(E, D, device=DEV), torch.full((E,), 0.25, device=DEV), xln=False)     # every logit equal: expert 0
        assert bool((r["expert"] == 0).all()) and bool((r["gap"] == 0).all())
        _check_layout(r, M, E)
    r = {"expert": torch.empty(M, dtype=torch.int32, device=DEV), "seg": torch.empty(2, dtype=torch.int32, device=DEV), "gap": torch.empty(M, device=DEV),
         "perm": torch.empty(ops.moe_packed_rows(M, 1), dtype=torch.int32, device=DEV), "tiles": torch.empty(ops.moe_packed_rows(M, 1) // T, dtype=torch.int32, device=DEV)}
    ops.moe_route(x, gamma, beta, 1e-5, torch.randn(1, D, device=DEV), torch.zeros(1, device=DEV), r["expert"], r["seg"], r["perm"], r["tiles"], gap=r["gap"])
    torch.cuda.synchronize()
    assert bool((r["expert"] == 0).all()) and bool(torch.isinf(r["gap"]).all())
    _check_layout(r, M, 1)


def test_route_strided_input_is_bit_identical_to_contiguous():
    """ldx != D: x is the first D columns of a [M, D + 12] buffer whose other columns are NaN.  Every output of pv_moe_route carries the bits
    of the contiguous call - a row read at the wrong stride, or one element of the padding, would show in all of them."""
    M, D, E, pad = 500, 768, 8, 12
    x, gamma, beta, W, bg = _route_inputs(M, D, E, M * 131 + E + D)
    bg = bg.to(DEV)
    r = _route(x, gamma, beta, W, bg)
    wide = torch.full((M, D + pad), float("nan"), device=DEV)
    wide[:, :D] = x
    r2 = _buffers(M, D, E)
    lib = _lib.load()
    nbytes = int(lib.pv_moe_route_scratch_size(M, E))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    rc = lib.pv_moe_route(wide.data_ptr(), D + pad, M, D, gamma.data_ptr(), beta.data_ptr(), 1e-5, W.data_ptr(), bg.data_ptr(), E,
                          r2["expert"].data_ptr(), r2["gap"].data_ptr(), r2["probs"].data_ptr(), r2["seg"].data_ptr(), r2["perm"].data_ptr(),
                          r2["tiles"].data_ptr(), r2["xln"].data_ptr(), scratch.data_ptr(), nbytes, ops.raw_stream(0))
    assert rc == 0
    torch.cuda.synchronize()
    _check_layout(r2, M, E)
    for k in ("expert", "seg", "perm", "tiles", "gap", "probs", "xln"):
        assert torch.equal(_raw(r[k]), _raw(r2[k])), k


def _manual_layout(counts, M_src, gen):
    """perm / tile table of a hand-made routing: expert e owns counts[e] source rows (drawn without replacement from M_src rows, so some rows
    belong to no expert), segments padded to 256 rows, the worst-case grid of pv_moe_packed_rows."""
    E = len(counts)
    rows = torch.randperm(M_src, generator=gen)
    Mp = ops.moe_packed_rows(M_src, E)
    perm = torch.full((Mp,), -1, dtype=torch.int32)
    tiles = torch.full((Mp // T,), -1, dtype=torch.int32)
    seg, o, k = [0], 0, 0
    for e, c in enumerate(counts):
        perm[o:o + c] = rows[k:k + c].sort().values.int()
        k += c
        n = (c + T - 1) // T * T
        tiles[o // T:(o + n) // T] = e
        o += n
        seg.append(o)
    return perm.to(DEV), tiles.to(DEV), seg


def _gelu16(v):
    return F.gelu(v).to(_lib.operand_dtype())


def test_grouped_gemm_against_fp64_and_sentinels():
    gen = torch.Generator().manual_seed(11)
    counts, M_src, K = [300, 0, 513, 1, 256], 1200, 256
    E = len(counts)
    perm, tiles, seg = _manual_layout(counts, M_src, gen)
    Mp = perm.numel()
    assert int((tiles < 0).sum()) >= 3                       # dead tiles at the worst-case grid
    od = _lib.operand_dtype()
    A = torch.randn(Mp, K, generator=gen).to(od).to(DEV)     # (pad rows hold data too: they must not leak anywhere)
    for N, epi in ((512, PV_EPI_BIAS_GELU_BF16), (384, PV_EPI_BIAS_RES_F32)):
        W = (torch.randn(E, N, K, generator=gen) / K ** 0.5).to(od).to(DEV)
        b = (0.1 * torch.randn(E, N, generator=gen)).to(DEV)
        ref = torch.einsum("mk,enk->emn", A.double(), W.double()) + b.double()[:, None, :]       # [E, Mp, N]
        if epi == PV_EPI_BIAS_GELU_BF16:
            out = torch.full((Mp, N), 1234.0, dtype=od, device=DEV)
            ops.gemm_grouped(A, W, b, out, epi, tiles)
            torch.cuda.synchronize()
            for e in range(E):
                lo, hi = seg[e], seg[e + 1]
                want = F.gelu(ref[e, lo:hi])
                got = out[lo:hi].double()
                assert bool(((got - want).abs() <= 8e-3 * want.abs() + 2e-3).all()), e
            dead = torch.repeat_interleave(tiles < 0, T)
            assert bool((out[dead] == 1234.0).all())                             # dead tiles write nothing
        else:
            res = torch.randn(M_src, N, generator=gen).to(DEV)
            out = torch.full((M_src, N), 777.0, device=DEV)
            ops.gemm_grouped(A, W, b, out, epi, tiles, res=res, perm=perm)
            torch.cuda.synchronize()
            seen = torch.zeros(M_src, dtype=torch.bool)
            for e in range(E):
                lo = seg[e]
                src = perm[lo:lo + counts[e]].long()
                want = res[src].double() + ref[e, lo:lo + counts[e]]
                np.testing.assert_allclose(out[src].double().cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-4)
                seen[src.cpu()] = True
            assert bool((out[~seen.to(DEV)] == 777.0).all())                     # rows no expert owns, and pad rows: never written
            # residual in place (out is res): the routed rows change, nothing else
            res2 = res.clone()
            ops.gemm_grouped(A, W, b, res2, epi, tiles, res=res2, perm=perm)
            torch.cuda.synchronize()
            assert torch.equal(res2[seen.to(DEV)], out[seen.to(DEV)]) and torch.equal(res2[~seen.to(DEV)], res[~seen.to(DEV)])


def test_grouped_gemm_bit_identical_to_per_expert_gemm():
    """Each expert's rows through pv_gemm_bf16 alone (on its 256-row tile kernel) give the grouped GEMM's bits."""
    gen = torch.Generator().manual_seed(12)
    counts, K = [12000, 11300, 13300], 256
    M_src = sum(counts) + 100
    E = len(counts)
    perm, tiles, seg = _manual_layout(counts, M_src, gen)
    Mp = perm.numel()
    od = _lib.operand_dtype()
    A = torch.randn(Mp, K, generator=gen).to(od).to(DEV)
    for N, epi in ((1024, PV_EPI_BIAS_GELU_BF16), (768, PV_EPI_BIAS_RES_F32)):
        W = (torch.randn(E, N, K, generator=gen) / K ** 0.5).to(od).to(DEV)
        b = (0.1 * torch.randn(E, N, generator=gen)).to(DEV)
        assert all(ops.gemm_tile_rows(c, N, K, epi) == 256 for c in counts)
        if epi == PV_EPI_BIAS_GELU_BF16:
            out = torch.empty((Mp, N), dtype=od, device=DEV)
            ops.gemm_grouped(A, W, b, out, epi, tiles)
            for e, c in enumerate(counts):
                one = torch.empty((c, N), dtype=od, device=DEV)
                ops.gemm(A[seg[e]:seg[e] + c].contiguous(), W[e], b[e], one, epi)
                assert torch.equal(out[seg[e]:seg[e] + c].view(torch.int16), one.view(torch.int16)), e
        else:
            res = torch.randn(M_src, N, generator=gen).to(DEV)
            out = torch.zeros((M_src, N), device=DEV)
            ops.gemm_grouped(A, W, b, out, epi, tiles, res=res, perm=perm)
            for e, c in enumerate(counts):
                src = perm[seg[e]:seg[e] + c].long()
                one = torch.empty((c, N), device=DEV)
                ops.gemm(A[seg[e]:seg[e] + c].contiguous(), W[e], b[e], one, epi, res=res[src].contiguous())
                assert torch.equal(out[src].view(torch.int32), one.view(torch.int32)), e


def test_gather_exact():
    gen = torch.Generator().manual_seed(13)
    E, M, D = 4, 1000, 256
    od = _lib.operand_dtype()
    planes = torch.randn(E, M, D, generator=gen).to(od).to(DEV)
    x = torch.randn(M, 64, generator=gen).to(DEV)
    r = _route(x, torch.ones(64, device=DEV), torch.zeros(64, device=DEV), torch.randn(E, 64, generator=gen).to(DEV), torch.zeros(E, device=DEV),
               xln=False)
    out = torch.full((r["perm"].numel(), D), 5.0, dtype=od, device=DEV)
    ops.moe_gather(planes, r["expert"], r["perm"], out)
    torch.cuda.synchronize()
    perm = r["perm"].long()
    live = perm >= 0
    src = perm[live]
    assert torch.equal(out[live].view(torch.int16), planes[r["expert"].long()[src], src].view(torch.int16))
    assert bool((out[~live].view(torch.int16) == 0).all())


@pytest.mark.parametrize("M,D", [(1000, 8), (1000, 264), (40000, 264)])
def test_gather_from_padded_planes_and_past_one_grid_sweep(M, D):
    """src is a view with ld = D + 8 and plane_stride = M * ld + 64 into a larger buffer whose padding holds a pattern that must not appear
    in out; perm / expert from a hand-made layout, so some source rows belong to no expert and some packed rows are pads.  D = 8: one
    16-byte chunk per row.  (40 000, 264): M_pad * D / 8 > 2^20 chunks, a second sweep of the grid-stride loop.
    out[p] = src[expert[perm[p]], perm[p], :D] bit for bit, zeros where perm[p] < 0."""
    gen = torch.Generator().manual_seed(M + D)
    E, ld = 4, D + 8
    counts = [M * 3 // 10, 0, M * 9 // 20 // T * T, 1]           # an empty expert, a segment of whole tiles, a one-row segment
    perm, tiles, seg = _manual_layout(counts, M, gen)
    Mp = perm.numel()
    assert M - sum(counts) > 0 and int((perm < 0).sum()) > 0 and (M < 40000 or Mp * (D // 8) > 2 ** 20)
    expert = torch.full((M,), -1, dtype=torch.int32)            # (rows no expert owns keep -1: perm never names them)
    for e, c in enumerate(counts):
        expert[perm[seg[e]:seg[e] + c].long().cpu()] = e
    expert = expert.to(DEV)
    stride = M * ld + 64
    PAD = 0x7A5A                                                 # a finite 16-bit pattern the data below never holds
    buf = torch.full((E * stride,), PAD, dtype=torch.int16, device=DEV)
    data = torch.randint(-2 ** 15, 2 ** 15, (E, M, D), generator=gen, dtype=torch.int32).to(torch.int16)
    data[data == PAD] = 0
    data = data.to(DEV)
    planes = torch.as_strided(buf, (E, M, D), (stride, ld, 1))
    planes.copy_(data)
    out = torch.full((Mp, D), float("nan"), dtype=_lib.operand_dtype(), device=DEV)
    ops.moe_gather(planes.view(_lib.operand_dtype()), expert, perm, out)
    torch.cuda.synchronize()
    got = out.view(torch.int16)
    live = perm >= 0
    src = perm[live].long()
    assert int(live.sum()) == sum(counts)
    assert torch.equal(got[live], data[expert.long()[src], src])
    assert bool((got[~live] == 0).all())
    assert not bool((got == PAD).any())


# ---- the model ----
def _model(name):
    from peekvit_amd.models.moevit import VisionTransformerMoE
    case = META["cases"][name]
    kw = case["kwargs"]
    model = VisionTransformerMoE(**kw).eval()
    sd = synth.moe_state_dict(case["synth_cfg"], kw.get("mlp_moes"), kw.get("attn_moes"), seed=0, dominant=case["dominant"])
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return model


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_model_matches_reference_golden(name, golden):
    g = golden(name)
    case = META["cases"][name]
    model = _model(name).to(DEV)
    x = torch.from_numpy(g["images"]) if "images" in g else torch.from_numpy(synth.synth_images(case["batch"], case["kwargs"]["image_size"], seed=0, name="moe"))
    n0 = engine.moe_routed_layers
    with torch.no_grad():
        logits = model(x.to(DEV))
    torch.cuda.synchronize()
    moes = model.moes()
    assert engine.last_forward_guarded() and engine.moe_routed_layers - n0 >= len(moes), "the routed kernels did not produce the answer"
    err = rel_l2(logits, g["logits"])
    assert err < 1e-3, err
    near_diff = 0
    for j, m in enumerate(moes):
        gl = g[f"gate_logits_{j}"]
        s = np.sort(gl, axis=-1)
        gap = s[..., -1] - s[..., -2]
        clear = gap > 1e-3 * np.abs(gl).max()
        got = m.gating_probs.cpu().numpy()
        assert got.shape == g[f"gating_probs_{j}"].shape
        assert np.array_equal(got[clear], g[f"gating_probs_{j}"][clear]), (name, j)
        near_diff += int((got[~clear] != g[f"gating_probs_{j}"][~clear]).any(-1).sum())
    print(f"{name}: logits rel L2 {err:.2e}, near-gap tokens routed differently: {near_diff}")


def _vit_keys(sd):
    out = {}
    for k, v in sd.items():
        if "gating_network" in k:
            continue
        k = "class_tokens" if k == "class_token" else k.replace("self_attention.experts.0.", "self_attention.").replace("mlp.experts.0.", "mlp.")
        out[k] = torch.from_numpy(v.copy())
    return out


@pytest.mark.parametrize("batch", [3, 64])
def test_all_ones_model_is_bit_identical_to_vit(batch):
    from peekvit_amd.models.moevit import VisionTransformerMoE
    from peekvit_amd.models.vit import VisionTransformer
    cfg = synth.MODEL_CONFIGS["vit_tiny"]
    kw = {k: cfg[k] for k in ("image_size", "patch_size", "num_layers", "num_heads", "hidden_dim", "mlp_dim", "num_classes")}
    sd = synth.moe_state_dict(kw)
    moe = VisionTransformerMoE(**kw).eval()
    moe.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    vit = VisionTransformer(**kw).eval()
    vit.load_state_dict(_vit_keys(sd))
    moe, vit = moe.to(DEV), vit.to(DEV)
    x = torch.from_numpy(synth.synth_images(batch, kw["image_size"], seed=2)).to(DEV)
    n0 = engine.moe_routed_layers
    with torch.no_grad():
        a = moe(x)
        b = vit(x)
    assert engine.moe_routed_layers == n0 and not moe.moes()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_graph_capture_replay_is_bit_identical():
    from peekvit_amd.graph import GraphedForward
    from peekvit_amd.models.moevit import VisionTransformerMoE
    cfg = dict(image_size=64, patch_size=8, num_layers=4, num_heads=2, hidden_dim=128, mlp_dim=256, num_classes=10)
    mlp_moes = [1, 4, 1, 3]
    model = VisionTransformerMoE(**cfg, mlp_moes=mlp_moes).eval()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.moe_state_dict(cfg, mlp_moes).items()})
    model = model.to(DEV)
    x = torch.from_numpy(synth.synth_images(16, 64, seed=4, name="moe")).to(DEV)
    with torch.no_grad():
        eager = model(x).clone()
        gates = [m.gating_probs.clone() for m in model.moes()]
        gf = GraphedForward(model, x)
        n0 = engine.moe_routed_layers
        replay = gf(x).clone()
    torch.cuda.synchronize()
    assert engine.moe_routed_layers == n0           # (a replay launches no Python)
    assert torch.equal(replay.view(torch.int32), eager.view(torch.int32))
    assert all(torch.equal(m.gating_probs, g) for m, g in zip(model.moes(), gates))


def test_vit_b16_dims_mlp_moe_at_batch_2048():
    from peekvit_amd.models.moevit import VisionTransformerMoE
    torch.manual_seed(0)
    model = VisionTransformerMoE(image_size=224, patch_size=16, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072,
                                 num_classes=1000, mlp_moes=[1, 8] * 6).eval()
    torch.nn.init.normal_(model.head.weight, std=0.02)
    model = model.to(DEV)
    x = torch.randn(2048, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    n0 = engine.moe_routed_layers
    with torch.no_grad():
        logits = model(x)
        torch.cuda.synchronize()
        assert engine.last_forward_guarded() and engine.moe_routed_layers - n0 >= 6
        assert bool(torch.isfinite(logits).all())
        gates = [m.gating_probs[:16].clone() for m in model.moes()]
        ref = model._composite_forward(x[:16])
    err = rel_l2(logits[:16], ref)
    flips = sum(int((a != m.gating_probs).any(-1).sum()) for a, m in zip(gates, model.moes()))
    print(f"ViT-B/16 MoE batch 2048: first 16 images rel L2 vs the composite {err:.2e}, tokens routed differently {flips}")
    assert err < 1e-3
