"""The RankViT selection path on the MI355X, entry point by entry point, at the edges of every loop: pv_token_norm per element against fp64,
pv_rank_topk[_gap] and pv_rank_topk_partials[_gap] exactly against a stable descending sort on the CPU, pv_gather_tokens / pv_scatter_tokens
as pure copies of 32-bit patterns.  A token ranked one place off or a row copied from its neighbour changes WHICH rows exist downstream; a
model-level relative L2 absorbs that, so everything here except the norm is bit equality.

Every call goes through the ctypes binding (as test_hip_entry_points.py::test_rank_topk_without_gap does) so that the test owns the output
buffers: each is filled with a sentinel first (-1 for indices, NaN for floats) and carries a few guard elements behind its last row - a row
the kernel never wrote, or a write past the end, is visible.  The shapes are the smallest that reach each mechanism (the second trip of a
lane loop, the second sweep of a grid-stride loop, N on both sides of the 256-thread workgroup, the declared limits)."""
import functools
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8                       # sentinel elements behind every output buffer
NAN_BITS = 0x7FC00000           # torch's float('nan'): the canonical positive NaN


@pytest.fixture(scope="module")
def hip():
    """(library, raw stream): the loaded bf16-operand library and torch's current stream on cuda:0."""
    from peekvit_amd import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _lib.load(), ops.raw_stream(0)


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------
# 1. pv_token_norm
# ------------------------------------------------------------------------------------------------
# (B, S, D): one token on one lane; 65 chunks (second trip of the lane loop, a single lane active); ViT-B width; the widest row; 17 640 rows
# (pv_stream_grid caps the grid at 4 096 workgroups x 4 rows: a second sweep of the grid-stride loop)
NORM_SHAPES = [(3, 2, 4), (2, 66, 260), (2, 9, 768), (1, 5, 4096), (90, 197, 64)]


@functools.lru_cache(maxsize=None)
def _norm_case(B, S, D):
    """x fp32 [B, S, D]: randn rows times per-row scales from 1e-3 to 1e3; token 0 of image 0 all zero; the last token of the last image
    zero but for 2^-5 in its last element (the last chunk of the row).  Returns (x, fp64 norms [B, S - 1])."""
    g = _g(B * 100003 + S * 101 + D)
    x = torch.randn(B, S, D, generator=g) * torch.pow(10.0, torch.rand(B, S, 1, generator=g) * 6 - 3)
    x[0, 1] = 0.0
    x[B - 1, S - 1] = 0.0
    x[B - 1, S - 1, D - 1] = -(2.0 ** -5)
    ref = x[:, 1:].double().pow(2).sum(-1).sqrt()
    return x, ref


@gpu
@pytest.mark.parametrize("B,S,D", NORM_SHAPES)
def test_token_norm_per_element_against_fp64(hip, B, S, D):
    """Every norm against the fp64 norm of the same fp32 row: |got - ref64| <= (ceil(D / 256) + 10) * 2^-24 * ref64, per element.
    Derivation (unit roundoff u = 2^-24; every term is a square, so nothing cancels and relative errors add):
      a square                              1 rounding
      the adds inside a float4              2 roundings on the longest path  ((x2 + y2) + (z2 + w2))
      the per-lane accumulation             ceil(D / 256) roundings          (one `s +=` per trip of the lane loop)
      the wave butterfly                    6 roundings                      (64 lanes = 6 levels)
    so the sum of squares is within (ceil(D / 256) + 9) u of exact; the square root halves that and adds its own rounding:
    (ceil(D / 256) + 9) / 2 + 1 <= ceil(D / 256) + 10 roundings in all.
    An all-zero row gives exactly +0.0 and a row whose only non-zero is a power of two gives exactly that value."""
    lib, stream = hip
    x, ref = _norm_case(B, S, D)
    rows = B * (S - 1)
    xd = x.to(DEV)
    out = torch.full((rows + GUARD,), float("nan"), device=DEV)
    assert lib.pv_token_norm(xd.data_ptr(), out.data_ptr(), B, S, D, stream) == 0
    flat = out.cpu()
    assert bool(torch.isnan(flat[rows:]).all()), "written past the last row"
    got = flat[:rows].reshape(B, S - 1)
    assert not bool(torch.isnan(got).any()), f"{int(torch.isnan(got).sum())} rows never written"
    err = (got.double() - ref).abs()
    bound = (math.ceil(D / 256) + 10) * 2.0 ** -24 * ref
    worst = float((err / ref.clamp_min(1e-300)).max()) / 2.0 ** -24
    print(f"pv_token_norm {(B, S, D)}: worst element {worst:.2f} u of fp64, bound {math.ceil(D / 256) + 10} u")
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{int(bad.sum())} of {rows} norms beyond the bound; first at {torch.nonzero(bad)[0].tolist()}"
    assert int(got[0, 0].view(torch.int32)) == 0                                   # +0.0, not -0.0 or a denormal
    assert float(got[B - 1, S - 2]) == 2.0 ** -5


@gpu
def test_token_norm_of_class_rows_only_writes_nothing(hip):
    """S = 1: no token to measure - OK, and the output is untouched."""
    lib, stream = hip
    xd = torch.randn(4, 1, 64, generator=_g(3)).to(DEV)
    out = torch.full((GUARD,), float("nan"), device=DEV)
    assert lib.pv_token_norm(xd.data_ptr(), out.data_ptr(), 4, 1, 64, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------
# 2. pv_rank_topk / pv_rank_topk_gap
# ------------------------------------------------------------------------------------------------
RANK_B = 3
RANK_NS = (1, 2, 64, 255, 256, 257, 513, 4096)          # one thread's worth, both sides of the 256-thread workgroup, the declared limit
FAMILIES = ("distinct", "quantised", "nan_inf", "equal")


def _ks(N):
    return sorted({0, 1, N // 2, N - 1, N})


@functools.lru_cache(maxsize=None)
def _rank_case(N, family):
    """norms fp32 [RANK_B, N] of a value family and their stable descending sort on the CPU (values, indices)."""
    g = _g(N * 7 + FAMILIES.index(family))
    if family in ("distinct", "nan_inf"):                # distinct integer parts: no two values of a row are equal after rounding either
        v = torch.stack([(torch.randperm(N, generator=g) + 1 + 0.25 * torch.rand(N, generator=g)) * 0.01 for _ in range(RANK_B)])
        if family == "nan_inf":
            for b in range(RANK_B):
                pos = torch.randperm(N, generator=g)[:min(N, 6)]
                for j, p in enumerate(pos.tolist()):
                    v[b, p] = float("nan") if (j + b) % 2 == 0 else float("inf")
    elif family == "quantised":                          # 8 levels: most ranks are decided by the lowest-index-first rule
        v = torch.floor(torch.rand(RANK_B, N, generator=g) * 8) / 8 + 0.125
    else:
        v = torch.full((RANK_B, N), 0.75)
    v = v.float().contiguous()
    s = torch.sort(v, dim=1, descending=True, stable=True)
    return v, s.values, s.indices.int()


def _sort_key(bits):
    """pv_sort_key of csrc/pv_rowops.hip on uint32 bit patterns (numpy): a larger float, NaN above +inf, is a larger key."""
    bits = bits.astype(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))


def test_sort_key_order_is_torchs_stable_descending_order():
    """No GPU: the kernel's order (key descending, lowest index first among equal keys) restated in numpy against torch.sort(descending=True,
    stable=True) on a row mixing NaN, +inf, ties and 0 - the reference of the exact tests below ranks such rows as the kernel is meant to."""
    row = torch.tensor([0.0, 2.5, float("nan"), float("inf"), 2.5, 0.0, 1e-40, float("inf"), 7.0, float("nan"), 2.5, 3.4e38, 0.0, 1.0])
    assert int(row[2].view(torch.int32)) == NAN_BITS
    keys = _sort_key(row.numpy().view(np.uint32)).astype(np.int64)
    order = np.lexsort((np.arange(len(keys)), -keys))                              # key descending, then index ascending
    assert order.tolist() == torch.sort(row, descending=True, stable=True).indices.tolist()
    assert order.tolist()[:4] == [2, 9, 3, 7]                                      # NaN above +inf, each pair by index


def _rank(lib, stream, norms_d, N, k, gap_fill=None, gap=True):
    """One launch into sentinel-filled buffers -> (rc, keep int32 [B, k] on the CPU, the guard behind it, gap_min on the CPU or None)."""
    B = norms_d.shape[0]
    keep = torch.full((B * k + GUARD,), -1, dtype=torch.int32, device=DEV)
    if gap:
        gm = (torch.full((B,), float("inf")) if gap_fill is None else gap_fill.clone()).to(DEV)
        rc = lib.pv_rank_topk_gap(norms_d.data_ptr(), keep.data_ptr(), gm.data_ptr(), B, N, k, stream)
    else:
        gm = None
        rc = lib.pv_rank_topk(norms_d.data_ptr(), keep.data_ptr(), B, N, k, stream)
    flat = keep.cpu()
    return rc, flat[:B * k].reshape(B, k), flat[B * k:], gm.cpu() if gap else None


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", RANK_NS)
def test_rank_topk_exact_against_stable_sort(hip, N, family):
    """keep == the first k indices of torch.sort(descending=True, stable=True) on the CPU for k in {0, 1, N // 2, N - 1, N}, from pv_rank_topk
    and from pv_rank_topk_gap alike; k = 0 leaves the sentinel-filled buffer alone.
    The gap (finite positive rows): gap_min pre-filled with +inf comes back as (n[k-1] - n[k]) / n[k-1] evaluated in fp32 on the CPU, within
    2^-21 relative (4 ulp: the subtraction and the CPU's division are correctly rounded, hipcc's fp32 division may be its 2.5-ulp form);
    k = N leaves +inf; a pre-filled value below the gap is kept."""
    lib, stream = hip
    v, sv, si = _rank_case(N, family)
    vd = v.to(DEV)
    B = RANK_B
    inf = torch.full((B,), float("inf"))
    for k in _ks(N):
        rc, keep, guard, _ = _rank(lib, stream, vd, N, k, gap=False)
        assert rc == 0 and bool((guard == -1).all()), (k, rc)
        assert torch.equal(keep, si[:, :k]), f"pv_rank_topk N={N} k={k} {family}"
        rc, keep_g, guard, gm = _rank(lib, stream, vd, N, k)
        assert rc == 0 and bool((guard == -1).all()), (k, rc)
        assert torch.equal(keep_g, keep), f"pv_rank_topk_gap N={N} k={k} {family}: another keep list than the plain form"
        if family == "nan_inf":
            continue
        if k == 0 or k == N:
            assert torch.equal(gm, inf), (k, gm)
            continue
        want = (sv[:, k - 1] - sv[:, k]) / sv[:, k - 1]                            # fp32, as the kernel's expression
        err = (gm.double() - want.double()).abs()
        assert bool((err <= 2.0 ** -21 * want.double()).all()), (k, gm, want)
        low = torch.where(want > 0, want * 0.5, torch.full_like(want, -1.0))
        rc, keep_l, _, gm_l = _rank(lib, stream, vd, N, k, gap_fill=low)
        assert rc == 0 and torch.equal(keep_l, keep) and torch.equal(gm_l.view(torch.int32), low.view(torch.int32)), (k, gm_l, low)


@gpu
def test_rank_topk_zero_row_and_mixed_specials(hip):
    """An all-zero row: indices 0 .. k-1 and a gap of exactly 0 (not 0 / 0).  A row mixing NaN, +inf, ties, a denormal and 0: torch's order."""
    lib, stream = hip
    N, k = 70, 9
    v = torch.zeros(2, N)
    g = _g(17)
    v[1] = torch.floor(torch.rand(N, generator=g) * 4) / 4                         # levels 0, .25, .5, .75: zeros among the ties
    v[1, [3, 40]] = float("nan")
    v[1, [0, 69]] = float("inf")
    v[1, 11] = 1e-40
    ref = torch.sort(v, dim=1, descending=True, stable=True).indices.int()
    assert ref[1, :4].tolist() == [3, 40, 0, 69]
    rc, keep, guard, gm = _rank(lib, stream, v.to(DEV), N, k)
    assert rc == 0 and bool((guard == -1).all())
    assert torch.equal(keep, ref[:, :k])
    assert int(gm[0].view(torch.int32)) == 0
    rc, keep, guard, _ = _rank(lib, stream, v.to(DEV), N, N, gap=False)
    assert rc == 0 and torch.equal(keep, ref)


# ------------------------------------------------------------------------------------------------
# 3. pv_rank_topk_partials / pv_rank_topk_partials_gap
# ------------------------------------------------------------------------------------------------
# (B, S, tiles, k): one token; N = 256 / 257 with 3 and the declared 64 tiles; a 24 x 24 patch grid; the declared N = 4096 at k = N and below
PARTIALS_SHAPES = [(3, 2, 1, 1), (2, 257, 3, 128), (2, 258, 64, 1), (2, 578, 6, 289), (1, 4097, 5, 4096), (1, 4097, 5, 2000)]


@functools.lru_cache(maxsize=None)
def _partials_case(B, S, tiles):
    """rowsq fp32 [tiles, B * S] of integers in [0, 1024), every class row 1023 in all tiles (it would rank first if it were read) ->
    (rowsq, the tokens' integer sums fp32 [B, S - 1], their stable descending order, the number of tokens that share their sum with another)."""
    rowsq = torch.randint(0, 1024, (tiles, B * S), generator=_g(1)).float()
    rowsq[:, ::S] = 1023.0
    sums = rowsq.sum(0).reshape(B, S)[:, 1:].contiguous()
    assert float(rowsq.sum(0).max()) < 2 ** 16 and torch.equal(sums.double(), rowsq.double().sum(0).reshape(B, S)[:, 1:])     # exact in any order
    tied = 0
    for b in range(B):
        _, inv, cnt = torch.unique(sums[b], return_inverse=True, return_counts=True)
        tied += int((cnt[inv] > 1).sum())
    return rowsq, sums, torch.sort(sums, dim=1, descending=True, stable=True).indices.int(), tied


def test_partials_reference_does_not_depend_on_rounding():
    """No GPU: why the reference of test_rank_topk_partials_exact_on_integer_sums is exact.  A token's sum over <= 64 tiles of integers below
    1024 is an integer below 2^16, exact in fp32 in any order; the correctly rounded square roots of the integers below 2^16 are distinct floats
    at least 64 ulp apart, so a square root that is a few ulp off still orders them as the integers are ordered.  And the cases hold both
    kinds of image: with seed 1, 0 / 56 / 16 / 227 / 3132 / 3132 tokens share their sum with another token of their image."""
    s = np.sqrt(np.arange(0, 65536, dtype=np.float32)).view(np.int32).astype(np.int64)
    assert int((s[2:] - s[1:-1]).min()) >= 64 and s[1] > s[0]
    tied = [_partials_case(B, S, tiles)[3] for B, S, tiles, _ in PARTIALS_SHAPES]
    assert tied == [0, 56, 16, 227, 3132, 3132], tied
    assert any(t == 0 for t in tied) and any(t > 0 for t in tied)


@gpu
@pytest.mark.parametrize("B,S,tiles,k", PARTIALS_SHAPES)
def test_rank_topk_partials_exact_on_integer_sums(hip, B, S, tiles, k):
    """keep == the first k indices of the stable descending sort of the tokens' integer sums (test_partials_reference_does_not_depend_on_rounding:
    the kernel's fp32 sum is exact and its square root cannot reorder them), 0-based among the S - 1 tokens behind the class row, which is
    1023 in every tile and must never be read as a token.  The plain and the _gap form agree, and pv_rank_topk on the square roots of the same
    sums returns the same list."""
    lib, stream = hip
    rowsq, sums, ref, _ = _partials_case(B, S, tiles)
    N = S - 1
    rd = rowsq.to(DEV)
    keep = torch.full((B * k + GUARD,), -1, dtype=torch.int32, device=DEV)
    assert lib.pv_rank_topk_partials(rd.data_ptr(), tiles, keep.data_ptr(), B, S, k, stream) == 0
    keep_g = torch.full((B * k + GUARD,), -1, dtype=torch.int32, device=DEV)
    gm = torch.full((B,), float("inf"), device=DEV)
    assert lib.pv_rank_topk_partials_gap(rd.data_ptr(), tiles, keep_g.data_ptr(), gm.data_ptr(), B, S, k, stream) == 0
    flat, flat_g, gm = keep.cpu(), keep_g.cpu(), gm.cpu()
    assert bool((flat[B * k:] == -1).all()) and bool((flat_g[B * k:] == -1).all())
    got = flat[:B * k].reshape(B, k)
    assert torch.equal(got, ref[:, :k]), f"{int((got != ref[:, :k]).sum())} of {B * k} kept indices differ from the stable sort of the sums"
    assert torch.equal(flat_g, flat)
    if k < N:
        assert bool(torch.isfinite(gm).all()) and bool((gm >= 0).all()) and bool((gm <= 1).all()), gm
    else:
        assert bool(torch.isinf(gm).all()), gm
    # the same ranking from the norms themselves
    rc, keep_n, guard, _ = _rank(lib, stream, sums.sqrt().to(DEV), N, k, gap=False)
    assert rc == 0 and bool((guard == -1).all()) and torch.equal(keep_n, got)


# ------------------------------------------------------------------------------------------------
# 4. pv_gather_tokens / pv_scatter_tokens
# ------------------------------------------------------------------------------------------------
# (B, S_in, k, D, gather too): nothing kept; one token, one lane; k = S_in - 1; 65 chunks (second trip of the lane loop); ViT-B width; the
# widest row; 17 640 output rows (second sweep of the gather's grid-stride loop); the scatter's declared limit S_in = 16 384 (64 KiB of LDS)
COPY_SHAPES = [(2, 2, 0, 4, True), (2, 2, 1, 4, True), (3, 50, 49, 64, True), (2, 66, 20, 260, True), (2, 9, 4, 768, True), (1, 5, 2, 4096, True),
               (90, 197, 195, 64, True), (2, 16384, 100, 4, False)]


def _bits(shape, g):
    """Random 32-bit patterns (int32): as fp32 they include NaN payloads, infinities and denormals - any arithmetic on the data would show.
    The sentinel's own pattern is taken out so that a row still holding it was certainly never written."""
    v = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    v[v == NAN_BITS] = 0
    return v


@gpu
@pytest.mark.parametrize("B,S_in,k,D,gather", COPY_SHAPES)
def test_gather_scatter_tokens_are_pure_copies(hip, B, S_in, k, D, gather):
    """keep: a random k-subset of every image's tokens in random order.  Compared as int32:
    gather   out[b, 0] = x[b, 0], out[b, 1 + j] = x[b, 1 + keep[b, j]];
    scatter  dx[b, 0] = dy[b, 0], dx[b, 1 + keep[b, i]] = dy[b, 1 + i], every other row +0.0 bits, every row written (NaN sentinel gone);
    round trip: scatter(gather(x)) is x on the class row and the kept rows."""
    lib, stream = hip
    g = _g(B * 1009 + S_in * 13 + k * 7 + D)
    keep = torch.stack([torch.randperm(S_in - 1, generator=g)[:k] for _ in range(B)]).int()
    kd = keep.to(DEV)
    kp = kd.data_ptr() if k else None
    bi = torch.arange(B)[:, None]
    rows = 1 + keep.long()

    def scatter(dy_d):
        dx = torch.full((B * S_in * D + GUARD,), float("nan"), device=DEV)
        assert lib.pv_scatter_tokens(dy_d.data_ptr(), kp, dx.data_ptr(), B, S_in, k, D, stream) == 0
        flat = dx.view(torch.int32).cpu()
        assert bool((flat[B * S_in * D:] == NAN_BITS).all()), "written past the last row"
        return flat[:B * S_in * D].reshape(B, S_in, D)

    def scattered(src):                         # the definition: src int32 [B, 1 + k, D] -> [B, S_in, D]
        want = torch.zeros((B, S_in, D), dtype=torch.int32)
        want[:, 0] = src[:, 0]
        want[bi, rows] = src[:, 1:]
        return want

    dy = _bits((B, k + 1, D), g)
    got = scatter(dy.to(DEV))
    assert not bool((got == NAN_BITS).all(-1).any()), "rows never written"
    assert torch.equal(got, scattered(dy))
    if not gather:
        return
    x = _bits((B, S_in, D), g)
    xd = x.to(DEV)
    out = torch.full((B * (k + 1) * D + GUARD,), float("nan"), device=DEV)
    assert lib.pv_gather_tokens(xd.data_ptr(), kp, out.data_ptr(), B, S_in, k, D, stream) == 0
    flat = out.view(torch.int32).cpu()
    assert bool((flat[B * (k + 1) * D:] == NAN_BITS).all()), "written past the last row"
    gathered = flat[:B * (k + 1) * D].reshape(B, k + 1, D)
    want = torch.cat([x[:, :1], x[bi, rows]], dim=1)
    assert torch.equal(gathered, want)
    back = scatter(out[:B * (k + 1) * D])
    assert torch.equal(back, scattered(want))
    assert torch.equal(back[:, 0], x[:, 0]) and torch.equal(back[bi, rows], x[bi, rows])
