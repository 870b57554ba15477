"""Exact expectations for the GEMM kernels (pv_gemm_bf16, pv_gemm_tn_bf16, pv_sum_slices_f32) on INTEGER operands, and the comparator that
tests/test_hip_gemm_exact.py (GPU) and tests/test_gemm_exact_host.py (CPU, planted faults) share.  Plain torch; imports without a GPU.

Why integers.  Operand entries are integers in [-a, a] times a power of two, so they are exact in bf16 and in fp16.  The bias, the residual, the
positional rows and the saved derivative plane are integers or eighths; row_scale, qscale and the folded rstd are powers of two, the folded mean a
small integer.  Every product and every partial sum is then a multiple of one power of two g (`gran`) and, while the worst case
max_row(sum |a||w|) + |bias| + |res| stays below 2^24 g, an exactly representable fp32 number IN ANY SUMMATION ORDER: MFMA blocking, split-K and
the tile shape cannot change a bit.  The value before the final conversion is the exact one, so

    fp32 outputs    equal  expected.to(float32)                    (torch.equal)
    16-bit outputs  equal  expected.to(operand dtype) bit for bit  (one round-to-nearest-even, as pv_pack_bf16x2 in both builds)

and there is no tolerance.  `Problem` asserts the conditions on the fp64 reference (never on a kernel's output) and picks a from K so that they hold:
a = min(24, isqrt(48000 / K)), i.e. sum |a||w| <= 48000 < 65504 (the fp16 output range) with outputs of standard deviation ~16000 / sqrt(K), far
above the 2^8 (bf16) / 2^11 (fp16) significant bits of an eighth-grid value, so most 16-bit outputs really are rounded (`rounded_share`, held to
one half by the tests for BIAS_BF16 and GELU_GRAD outputs).  Two kinds of case cannot reach one half, because a sum of the same launch must stay
exact: the row-statistic cases (`small`, a = 1: per row and column tile the sum of squares, in squared grains, stays below 2^24; x16_out is
rounded on 64 (bf16) / 2 (fp16) columns per tile, `_x16_spikes` says why no more) and the fused column sums (`colsum_rounded_share`, reported
only).

GELU is not exact but its pre-activation is: W carries 2^-3 and the bias eighths, the pre-activations lie on the 1/8 grid across the table's
[-5.5, 5.41], and the project's existing elementwise bounds apply per element against fp64 of that exact pre-activation.

Buffers.  Every matrix operand and output is a column-sliced view of a wider buffer: 8 (16-bit) or 4 (fp32) NaN columns to its left (16 bytes: the
base pointer is offset, the row stride is not the row length), at least 8 to its right, one NaN row below.  The comparator checks that every such
sentinel still holds its bits."""
import dataclasses
import math

import torch

from peekvit_amd import _lib

NAN = float("nan")
EPI = {"bias16": _lib.PV_EPI_BIAS_BF16, "gelu": _lib.PV_EPI_BIAS_GELU_BF16, "res": _lib.PV_EPI_BIAS_RES_F32, "pos": _lib.PV_EPI_BIAS_POS_F32,
       "bias32": _lib.PV_EPI_BIAS_F32, "split": _lib.PV_EPI_BIAS_GELU_SPLIT_BF16, "pair": _lib.PV_EPI_BIAS_GELU_PAIR_BF16,
       "grad": _lib.PV_EPI_GELU_GRAD_BF16}
OUT16 = ("bias16", "gelu", "split", "pair", "grad")
PLANES = {"split": 3, "pair": 2}
GELU_LO, GELU_SCALE, GELU_N = -5.5, 64.0 / 11.0, 64          # pv_gelu_table.h: interval i covers [LO + i / SCALE, LO + (i + 1) / SCALE)


@dataclasses.dataclass(frozen=True)
class Case:
    """One GEMM call.  tile: what pv_gemm_tile_rows answers for the call WITHOUT its feature (a feature - rowsq / x16 / fold / colsum - then forces
    the 256-row kernel or the call fails with PV_ERR_UNSUPPORTED; `ln` runs the fused-LayerNorm rows / full-row kernel)."""
    epi: str
    M: int
    N: int
    K: int
    tile: int
    qcols: int = 0
    ksplit: int = 0
    row_scale: bool = False
    res_scaled: bool = False
    inplace: bool = False
    feat: str = ""                 # "", "rowsq", "x16", "fold", "colsum", "ln"
    pos: tuple = ()                # (rows_per_img_in, rows_per_img_out, row_off)

    @property
    def small(self):
        return self.feat in ("rowsq", "x16")

    @property
    def id(self):
        s = f"{self.epi}-{self.M}x{self.N}x{self.K}"
        for k, v in (("q", self.qcols), ("ks", self.ksplit)):
            s += f"-{k}{v}" if v else ""
        for k in ("row_scale", "res_scaled", "inplace"):
            s += f"-{k}" if getattr(self, k) else ""
        return s + (f"-{self.feat}" if self.feat else "")


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------------
def pad_left(dtype):
    return 4 if dtype == torch.float32 else 8


def guarded(rows, cols, dtype, device, fill=None, dense=False):
    """(buffer [rows + 1, 8k], view [rows, cols] at column pad_left): NaN everywhere, `fill` (any float tensor [rows, cols]) copied into the view.
    dense (where a kernel requires ldo = N): no padding columns, the guard row only."""
    left = 0 if dense else pad_left(dtype)
    width = cols if dense else left + cols + 8
    width += 0 if dense else -width % 8
    buf = torch.full((rows + 1, width), NAN, dtype=dtype, device=device)
    view = buf[:rows, left:left + cols]
    if fill is not None:
        view.copy_(fill.to(dtype))
        assert torch.equal(view.double(), fill.double().to(device)), "operand is not exactly representable"
    return buf, view


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- comparator ---------------------------------------------------------------------------------------------------------------------------------
def describe(name, bad, tile=(128, 128)):
    """One finding for a non-empty mask of wrong elements: the first wrong (row, column), how many, and the shape of the wrong set."""
    bad = bad.cpu()
    n = int(bad.sum())
    if n == 0:
        return []
    M, N = bad.shape
    rows, cols = torch.nonzero(bad.any(1)).flatten(), torch.nonzero(bad.any(0)).flatten()
    r0, c0 = int(rows[0]), int(torch.nonzero(bad[int(rows[0])]).flatten()[0])
    shapes = []
    if bool(bad[rows].all()):
        shapes.append(f"{len(rows)} whole row(s)")
    for gsz in (8, 4):
        if N % gsz == 0:
            grp = bad.reshape(M, N // gsz, gsz)
            if bool((grp.any(2) == grp.all(2)).all()) and not shapes:
                shapes.append(f"{int(grp.all(2).sum())} whole {gsz}-column store group(s)")
    ra, rb, ca, cb = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
    if bool(bad[ra:rb, ca:cb].all()) and ra % tile[0] == 0 and (rb % tile[0] == 0 or rb == M) and ca % tile[1] == 0 and (cb % tile[1] == 0 or cb == N):
        shapes.append(f"the {tile[0]}x{tile[1]}-tile-aligned block rows {ra}:{rb} columns {ca}:{cb}")
    return [f"{name}: {n} of {M * N} elements wrong, first at (row {r0}, column {c0}); wrong set: {', '.join(shapes) if shapes else 'scattered'}"
            f" (rows {ra}:{rb}, columns {ca}:{cb})"]


def compare_exact(name, got, expected, tile=(128, 128)):
    """got (fp32 or 16-bit, a view is fine) against the exact fp64 expectation: torch.equal of the fp32 cast / bit equality of the 16-bit cast."""
    exp = expected.to(got.dtype)
    if got.dtype == torch.float32:
        if torch.equal(got, exp):
            return []
        return describe(name, ~(got == exp), tile)
    return describe(name, _bits(got) != _bits(exp), tile)


def compare_bound(name, got, ref, bound, tile=(128, 128)):
    """|got - ref| <= bound per element (fp64; NaN counts as wrong)."""
    return describe(name, ~((got.double() - ref).abs() <= bound), tile)


def check_sentinels(name, buf, rows, cols, untouched_rows=None):
    """The padding columns, the guard row and (POS remap) the output rows the epilogue must not touch still hold the NaN sentinel's bits."""
    left = 0 if buf.shape[1] == cols else pad_left(buf.dtype)            # (a dense buffer has the guard row only)
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:rows, left:left + cols] = False
    if untouched_rows is not None:
        keep[untouched_rows.to(buf.device), left:left + cols] = True
    changed = keep & (_bits(buf) != _bits(torch.full((1,), NAN, dtype=buf.dtype, device=buf.device)))
    n = int(changed.sum())
    if n == 0:
        return []
    r, c = (int(v) for v in torch.nonzero(changed)[0])
    where = "guard row" if r >= rows else "padding column" if not left <= c < left + cols else "untouched output row"
    return [f"{name}: {n} sentinel element(s) overwritten, first at buffer (row {r}, column {c}) = view (row {r}, column {c - left}): {where}"]


def same_bits(name, first, second):
    """Two launches of the same call: identical bits, sentinels included (first, second: whole buffers)."""
    diff = _bits(first) != _bits(second)
    n = int(diff.sum())
    if n == 0:
        return []
    r, c = (int(v) for v in torch.nonzero(diff)[0])
    return [f"{name}: two launches differ in {n} element(s), first at buffer (row {r}, column {c})"]


# ---- operands and expectations ------------------------------------------------------------------------------------------------------------------
def amplitude(case):
    """(a_A, a_W, log2 of W's scale): see the module docstring."""
    if case.epi in ("gelu", "pair", "split"):
        # pre-activation = sum / 8 with standard deviation a_A (a_A + 1) a_W (a_W + 1) / 9 * sqrt(K) / 8: the pair closest to 2.5
        target = (2.5 * 8 * 3) ** 2 / case.K
        aa, aw = min(((x, y) for x in (1, 2, 3) for y in (1, 2, 3, 4) if x <= y), key=lambda p: abs(math.log(p[0] * (p[0] + 1) * p[1] * (p[1] + 1) / target)))
        return aa, aw, -3
    if case.small:
        return 1, 1, 0
    if case.feat == "colsum":          # column sums over thousands of rows: sum |stored| itself must stay below 2^24 / 8, so small products
        a = max(1, math.isqrt(2000 // case.K))
        return a, a, 0
    a = max(1, min(24, math.isqrt((24000 if case.epi == "grad" else 48000) // case.K)))          # (grad: times a derivative plane of up to 2)
    return a, a, 0


def _ints(g, shape, a):
    return torch.randint(-a, a + 1, shape, generator=g).double()


def _pow2(g, n, exps):
    return torch.tensor(exps, dtype=torch.float64)[torch.randint(0, len(exps), (n,), generator=g)].exp2()


X16_SPIKES = {torch.bfloat16: 64, torch.float16: 2}          # columns per 256-wide column tile whose x16_out value needs rounding


def _x16_spikes(g, res, base, dtype):
    """The residual of an x16_out case: on the first X16_SPIKES[dtype] columns of every 256-wide column tile it is chosen so that the OUTPUT
    base + res is a given value on the eighth grid that the 16-bit type cannot hold, so the epilogue's 16-bit conversion really rounds there.
    How many such values a row can carry is bounded by the exact row statistics: a tile's sum of squares, in squared grains, must stay below
    2^24.  bf16 (8 significant bits) needs |value| >= 257 grains: 56 columns at odd 257 .. 399 grains (ulp 2: ties, to even is up for some and
    down for others) and 8 at 513 .. 639 grains that are 1 or 3 modulo 4 (ulp 4: nearest is down / up), ~9 M of the 16.7 M squared grains.
    fp16 (11 bits) needs >= 2049 grains, 4.2 M squared each: no more than three fit, so TWO columns at odd 2049 .. 2149 grains (ties) is what an
    fp16 x16 case can check: 2 of 256 outputs."""
    M, N = res.shape
    j = torch.arange(N) % 256
    odd = lambda lo, hi: (lo + 2 * torch.randint(0, (hi - lo) // 2 + 1, (M, N), generator=g)).double()          # noqa: E731
    if dtype == torch.bfloat16:
        grains = torch.where(j < 8, odd(513, 639), odd(257, 399))
    else:
        grains = odd(2049, 2149)
    sign = 2.0 * torch.randint(0, 2, (M, N), generator=g).double() - 1
    target = (sign * grains / 8).to(res.device)
    return torch.where((j < X16_SPIKES[dtype]).to(res.device), target - base, res)


def gelu_intervals(pre):
    """The table intervals that pre-activations INSIDE the table's range fall into (values beyond its ends are clamped by the kernel and count
    for no interval here)."""
    idx = ((pre - GELU_LO) * GELU_SCALE).floor().long()
    return set(idx[(idx >= 0) & (idx < GELU_N)].unique().tolist())


class Problem:
    """Operands (guarded views on `device`), the keyword arguments of ops.gemm, and the exact fp64 expectations of one Case."""

    def __init__(self, case, dtype, device, seed=0):
        c, self.case, self.dtype, self.device = case, case, dtype, device
        M, N, K = c.M, c.N, c.K
        g = torch.Generator().manual_seed(1000 * seed + M * 7 + N * 3 + K)
        aa, aw, wexp = amplitude(c)
        A, W = _ints(g, (M, K), aa), _ints(g, (N, K), aw) * 2.0 ** wexp
        eighths = lambda shape, lim: _ints(g, shape, 8 * lim) / 8                                       # noqa: E731
        gelu = c.epi in ("gelu", "pair", "split")
        bias = None if c.epi == "grad" or c.feat == "fold" else (_ints(g, (N,), 3) if c.small else eighths((N,), 1 if gelu else 8))
        self.a_buf, self.a = guarded(M, K, dtype, device, A)
        self.w_buf, self.w = guarded(N, K, dtype, device, W)
        self.bias = None if bias is None else bias.float().to(device)
        A, W = A.to(device), W.to(device)
        bias64 = torch.zeros(N, dtype=torch.float64, device=device) if bias is None else bias.to(device)
        gran, worst = 2.0 ** (wexp - 3), (A.abs() @ W.abs().t()).max().item() + float(bias64.abs().max())
        self.kw, self.expected, self.untouched = {}, {}, None
        self.out_dtype = dtype if c.epi in OUT16 else torch.float32
        self.out_rows, self.out_cols = M, N * PLANES.get(c.epi, 1)
        self.res = self.res_fill = None
        out_scale = 1.0
        if c.ksplit > 1:                                                # fp32 slices, the bias in slice 0 only; their sum through pv_sum_slices_f32
            assert c.epi == "bias32" and K % (64 * c.ksplit) == 0
            ks = K // c.ksplit
            sl = [A[:, t * ks:(t + 1) * ks] @ W[:, t * ks:(t + 1) * ks].t() + (bias64 if t == 0 else 0.0) for t in range(c.ksplit)]
            self.expected["slices"] = torch.stack(sl)
            self.expected["sum"] = A @ W.t() + bias64
            self.kw["ksplit"] = c.ksplit
        elif c.epi in ("bias16", "bias32") and c.feat != "fold":
            e = A @ W.t() + bias64
            e[:, :c.qcols] *= 0.25
            self.kw.update(qcols=c.qcols, qscale=0.25)
            self.expected["out"] = e
        elif c.epi == "res" or c.feat == "ln":
            res = (_ints(g, (M, N), 3) if c.small else eighths((M, N), 8)).to(device)
            # (row-statistic cases: no row_scale of 2, which would quadruple the squares)
            rs = _pow2(g, M, (-1, 0, -2) if c.small else (-1, 0, 1, -2)).to(device) if c.row_scale else torch.ones(M, dtype=torch.float64, device=device)
            base = rs[:, None] * (A @ W.t() + bias64)
            if c.feat == "x16":
                res = _x16_spikes(g, res, base, dtype)
            self.res_fill = res
            e = base + (rs[:, None] if c.res_scaled else 1.0) * res
            worst, gran, out_scale = worst + float(res.abs().max()), gran * (0.25 if c.row_scale else 1.0), 2.0 if c.row_scale else 1.0
            self.expected["out"] = e
            if not c.inplace:
                self.res_buf, self.res = guarded(M, N, torch.float32, device, res)
            if c.row_scale:
                self.kw["row_scale"] = rs.float()
            if c.res_scaled:
                self.kw["res_scaled"] = True
            tiles = (N + 255) // 256
            per_tile = lambda v: torch.stack([v[:, t * 256:(t + 1) * 256].sum(1) for t in range(tiles)])      # noqa: E731
            # exact in any summation order: per row and column tile, the sum of squares counted in squared grains of THAT row stays below 2^24
            # (the grain: row_scale times an integer where the residual is one, eighths with the x16 cases' residual)
            grain = torch.full_like(rs, 0.125) if c.feat == "x16" else rs.clamp(max=1.0)
            if c.feat in ("rowsq", "x16"):
                assert torch.equal(torch.round(e / grain[:, None]) * grain[:, None], e)
                assert float((per_tile(e * e) / (grain * grain)).max()) < 2 ** 24, f"{c.id}: a row's sum of squares leaves the exact range"
            if c.feat == "rowsq":
                self.expected["rowsq"] = per_tile(e * e)
            if c.feat == "x16":
                self.expected["x16"] = e
                self.x16_rounded_share = float((e.to(dtype).double() != e).double().mean())
                self.expected["rowstat"] = torch.stack([per_tile(e), per_tile(e * e)], dim=2)
            if c.feat == "ln":
                self.ln = (torch.ones(N, device=device), torch.zeros(N, device=device), 1e-5)
        elif c.epi == "pos":
            rpi, rpo, off = c.pos
            pos = eighths((rpo, N), 8).to(device)
            m = torch.arange(M, device=device)
            orow = (m // rpi) * rpo + off + m % rpi
            self.out_rows = ((M + rpi - 1) // rpi) * rpo
            e = torch.full((self.out_rows, N), NAN, dtype=torch.float64, device=device)
            e[orow] = A @ W.t() + bias64 + pos[off + m % rpi]
            worst += float(pos.abs().max())
            self.orow, self.expected["out"] = orow, e
            self.untouched = torch.tensor(sorted(set(range(self.out_rows)) - set(orow.tolist())), dtype=torch.long)
            self.kw.update(pos=pos.float().contiguous(), rows_per_img_in=rpi, rows_per_img_out=rpo, row_off=off)
        elif c.feat == "fold":                                           # consumer of the folded LayerNorm: rstd (acc - mean c1) + c2, then the q-scale
            assert c.epi == "bias16"
            mean, rstd = _ints(g, (M,), 3).to(device), _pow2(g, M, (0, -1)).to(device)
            c1, c2 = W.sum(1), (_ints(g, (N,), 128) / 16).to(device)            # (sixteenths: an fp16 output above 128 is rounded as well)
            e = rstd[:, None] * (A @ W.t() - mean[:, None] * c1) + c2
            e[:, :c.qcols] *= 0.25
            worst, gran = worst + 3 * float(c1.abs().max()) + 8, 2.0 ** -5              # (sixteenths times rstd >= 1/2)
            self.kw.update(fold=(torch.stack([mean, rstd], 1).float().contiguous(), c1.float().contiguous(), c2.float().contiguous()), qcols=c.qcols, qscale=0.25)
            self.expected["out"] = e
        elif gelu:
            pre = A @ W.t() + bias64
            y = torch.nn.functional.gelu(pre)
            self.pre = pre
            if c.epi == "gelu":
                self.expected["gelu"] = y
            elif c.epi == "pair":
                self.expected["gelu"] = y
                self.expected["dgelu"] = 0.5 * torch.erfc(-pre / math.sqrt(2.0)) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
            else:
                self.expected["gelu"] = y                               # (split: hi against the bound, lo and the third plane against the kernel's own y)
        elif c.epi == "grad":                                            # (a . w^T) * the saved derivative plane (16-bit, strided), rounded once
            if c.feat == "colsum":
                plane, gran = (2 * _ints(g, (M, N), 8).clamp(max=7) + 1) / 8, 2.0 ** -3
            else:              # odd 32nds in [-63/32, 63/32]: six more significant bits in every product, so fp16 outputs are rounded as well
                plane, gran = (2 * _ints(g, (M, N), 32).clamp(max=31) + 1) / 32, 2.0 ** -5
            self.res_buf, self.res = guarded(M, N, dtype, device, plane)
            e = (A @ W.t()) * plane.to(device)
            worst = worst * 2
            self.expected["out"] = e
            if c.feat == "colsum":
                stored = e.to(dtype).double()
                assert float(stored.abs().sum(0).max()) / gran < 2 ** 24
                self.expected["colsum"] = stored.sum(0)
        else:
            raise ValueError(c)
        # the conditions of the integer argument, on the reference
        self.worst, self.gran = worst, gran
        assert worst / gran < 2 ** 24, f"{c.id}: worst case {worst} / {gran} is not below 2^24"
        if self.out_dtype == torch.float16 or (c.feat == "x16" and dtype == torch.float16):
            assert worst * out_scale < 65504, f"{c.id}: worst case {worst * out_scale} leaves the fp16 range"
        self.rounded_share = None
        if c.epi in ("bias16", "grad"):
            e = self.expected["out"]
            share = float((e.to(dtype).double() != e).double().mean())
            if c.feat == "colsum":          # reported, not held to one half: these cases trade rounding for exact sums over thousands of rows
                self.colsum_rounded_share = share
            else:
                self.rounded_share = share
        if gelu:
            self.intervals = gelu_intervals(self.pre)
            self.intervals_hit = len(self.intervals)

    # -- launching ----------------------------------------------------------------------------------------------------------------------------
    def fresh_outputs(self):
        """NaN-filled output buffers of one launch: {name: (buffer, view)}."""
        c, dev, o = self.case, self.device, {}
        if c.ksplit > 1:
            o["slices"] = guarded(c.ksplit * c.M, c.N, torch.float32, dev)       # (split-K slices are M * ldo apart: one padded stack, ldo > N)
            return o
        o["out"] = guarded(self.out_rows, self.out_cols, self.out_dtype, dev, self.res_fill if c.inplace else None, dense=c.feat == "ln")
        tiles = (c.N + 255) // 256
        if c.feat == "rowsq":
            o["rowsq"] = (torch.full((tiles, c.M), NAN, device=dev),) * 2
        if c.feat == "x16":
            o["x16"] = (torch.full((c.M, c.N), NAN, dtype=self.dtype, device=dev),) * 2
            o["rowstat"] = (torch.full((tiles, c.M, 2), NAN, device=dev),) * 2
        if c.feat == "colsum":
            o["colsum"] = (torch.full((c.N,), NAN, device=dev),) * 2
        if c.feat == "ln":
            o["ln"] = (torch.full((c.M, c.N), NAN, dtype=self.dtype, device=dev),) * 2
        return o

    def launch(self, ops, o):
        c, kw = self.case, dict(self.kw)
        out = self.slices_view(o) if c.ksplit > 1 else o["out"][1]
        if c.epi == "res":
            kw["res"] = out if c.inplace else self.res
        if c.epi == "grad":
            kw["res"] = self.res
        if c.feat == "rowsq":
            kw["rowsq_out"] = o["rowsq"][1]
        if c.feat == "x16":
            kw.update(x16_out=o["x16"][1], rowstat_out=o["rowstat"][1])
        if c.feat == "colsum":
            kw["colsum_out"] = o["colsum"][1]
        if c.feat == "ln":
            kw["ln"] = (*self.ln, o["ln"][1], None)
        ops.gemm(self.a, self.w, self.bias, out, EPI[c.epi], M=c.M, **kw)

    def slices_view(self, o):
        """The [ksplit, M, N] view of the padded slice stack (row stride ldo = the buffer's width, slice stride M * ldo)."""
        c, (buf, _) = self.case, o["slices"]
        left = pad_left(torch.float32)
        return buf[:c.ksplit * c.M].view(c.ksplit, c.M, buf.shape[1])[:, :, left:left + c.N]

    def emulate(self, o):
        """What a correct kernel leaves in the outputs: the expectation rounded once (the host test plants its faults into this)."""
        c, E, N = self.case, self.expected, self.case.N
        if c.ksplit > 1:
            o["slices"][1].copy_(E["slices"].view(c.ksplit * c.M, N))
            return o
        out = o["out"][1]
        if c.epi == "pos":
            out[self.orow] = E["out"][self.orow].to(out.dtype)
        elif c.epi in ("gelu", "pair", "split"):
            y = E["gelu"].to(out.dtype)
            out[:, :N] = y
            if c.epi == "pair":
                out[:, N:] = E["dgelu"].to(out.dtype)
            if c.epi == "split":
                out[:, N:2 * N] = (E["gelu"] - y.double()).to(out.dtype)
                out[:, 2 * N:] = y
        else:
            out.copy_(E["out"])
        for name in ("rowsq", "x16", "rowstat", "colsum"):
            if name in o:
                o[name][1].copy_(E[name])
        if "ln" in o:
            o["ln"][1].zero_()
        return o

    def query_fields(self, o):
        """The members of pv_gemm_args the kernel choice depends on, for ops.gemm_tile_rows (features excluded: see Case)."""
        c = self.case
        f = dict(lda=self.a.stride(0), ldw=self.w.stride(0), ldo=o["slices" if c.ksplit > 1 else "out"][1].stride(0), qcols=self.kw.get("qcols", 0), ksplit=c.ksplit)
        if c.epi in ("res", "grad"):
            f["ldr"] = o["out"][1].stride(0) if c.inplace else self.res.stride(0)
        if c.epi == "pos":
            f.update(pos=16, rows_per_img_in=c.pos[0], rows_per_img_out=c.pos[1], row_off=c.pos[2])
        return f

    # -- comparing ----------------------------------------------------------------------------------------------------------------------------
    def findings(self, o, tile):
        """Every exact / bounded comparison and every sentinel of one launch's outputs."""
        c, E, f, t2 = self.case, self.expected, [], (tile, tile)
        if c.ksplit > 1:
            return (check_sentinels("slices", o["slices"][0], c.ksplit * c.M, c.N) +
                    compare_exact("slices", o["slices"][1], E["slices"].view(c.ksplit * c.M, c.N), t2))
        buf, out = o["out"]
        f += check_sentinels("out", buf, self.out_rows, self.out_cols, self.untouched)
        N = c.N
        if c.epi == "pos":
            f += compare_exact("out", out[self.orow], E["out"][self.orow], t2)
        elif c.epi == "gelu":
            f += compare_bound("gelu", out, E["gelu"], 0.006 * E["gelu"].abs() + 2e-5, t2)
        elif c.epi == "pair":
            f += compare_bound("gelu", out[:, :N], E["gelu"], 0.006 * E["gelu"].abs() + 2e-5, t2)
            f += compare_bound("dgelu", out[:, N:], E["dgelu"], 1.0e-4 + 1.13 * 2.0 ** -8, t2)
        elif c.epi == "split":
            hi, lo, third = out[:, :N], out[:, N:2 * N], out[:, 2 * N:]
            y = hi.double() + lo.double()                               # the kernel's own y, to 2^-16
            f += compare_bound("gelu (hi + lo)", y, E["gelu"], 0.006 * E["gelu"].abs() + 2e-5, t2)
            # hi is the 16-bit rounding of a value within 2^-16 |y| of that y: at most half an ulp of hi (+ that slack) away from it
            p, emin = (7, -126) if self.dtype == torch.bfloat16 else (10, -14)
            ulp = torch.exp2(torch.floor(torch.log2(hi.double().abs().clamp(min=2.0 ** emin))) - p)
            f += compare_bound("hi vs rounded (hi + lo)", hi, y, 0.5 * ulp + 2.0 ** -16 * y.abs(), t2)
            f += describe("third plane vs hi", _bits(third) != _bits(hi), t2)
        else:
            f += compare_exact("out", out, E["out"], t2)
        if c.feat == "rowsq":
            f += compare_exact("rowsq", o["rowsq"][1], E["rowsq"], (1, tile))
        if c.feat == "x16":
            f += compare_exact("x16", o["x16"][1], E["x16"], t2)
            f += compare_exact("rowstat", o["rowstat"][1].view(-1, 2 * c.M), E["rowstat"].reshape(-1, 2 * c.M), (1, 2 * tile))
        if c.feat == "colsum":
            f += compare_exact("colsum", o["colsum"][1].view(1, N), E["colsum"].view(1, N), (1, tile))
        if c.feat == "ln":          # every row was normalised: a kernel without the fused LayerNorm would leave the NaN fill
            f += describe("ln (written and finite)", ~torch.isfinite(o["ln"][1]), t2)
        return f


def build(case, dtype, device):
    """The case's Problem.  At least half of an exactly checked 16-bit output must really need rounding; with a handful of outputs (M = 1, N = 4)
    one draw can miss that by chance, so the builder takes the first of eight seeds that meets it (the same one on every machine: the operands
    come from a seeded CPU generator).  The callers assert the share."""
    for seed in range(8):
        P = Problem(case, dtype, device, seed)
        if P.rounded_share is None or P.rounded_share >= 0.5:
            break
    return P


def tn_problem(K, M, N, ks, dtype, device):
    """pv_gemm_tn_bf16: part[t] = a[K_t, M]^T . b[K_t, N], slices of whole 128-row blocks, the last one takes the remainder.  Both operands strided
    guarded views; returns (a, b, expected slices [ks, M, N] fp64)."""
    g = torch.Generator().manual_seed(K + M + N)
    amp = max(1, min(24, math.isqrt(48000 // K)))
    A, B = _ints(g, (K, M), amp), _ints(g, (K, N), amp)
    assert K * amp * amp < 2 ** 24
    _, a = guarded(K, M, dtype, device, A)
    _, b = guarded(K, N, dtype, device, B)
    A, B = A.to(device), B.to(device)
    kslice = K // 128 // ks * 128
    bounds = [t * kslice for t in range(ks)] + [K]
    return a, b, torch.stack([A[bounds[t]:bounds[t + 1]].t() @ B[bounds[t]:bounds[t + 1]] for t in range(ks)])


# ---- the cases of tests/test_hip_gemm_exact.py (shared with the host test, which checks the builder's conditions for each) -------------------------
def _k128_cases():
    """128^2 kernel: every epilogue of the dispatcher's switch at the row, column and K edges: M in {1, 127, 129} x N in {4, 132, 256} (N = 4 and
    132: a four-column last tile behind the clamp n = N - 4) x K in {64, 128, 192}."""
    shapes = [(M, N, K) for M in (1, 127, 129) for N in (4, 132, 256) for K in (64, 128, 192)]
    out = []
    for M, N, K in shapes:
        for epi in ("gelu", "pair", "split", "grad"):
            out.append(Case(epi, M, N, K, 128))
        for epi in ("bias16", "bias32"):
            for q in sorted({0, 4, 68, N}):
                if q <= N:
                    out.append(Case(epi, M, N, K, 128, qcols=q))
        out += [Case("res", M, N, K, 128), Case("res", M, N, K, 128, row_scale=True), Case("res", M, N, K, 128, inplace=True)]
        if N not in (256, 384, 512):          # (the dispatcher refuses res_scaled at the full-row kernel's widths, whatever M)
            out.append(Case("res", M, N, K, 128, row_scale=True, res_scaled=True))
    # POS: row_off = 2, rows_per_img_out > rows_per_img_in + row_off, M ends mid-image
    out += [Case("pos", 129, 132, 128, 128, pos=(50, 55, 2)), Case("pos", 127, 256, 64, 128, pos=(50, 55, 2)), Case("pos", 1, 4, 192, 128, pos=(50, 55, 2))]
    # split-K with the bias in slice 0 only
    out += [Case("bias32", 129, 132, 128, 128, ksplit=2), Case("bias32", 127, 256, 192, 128, ksplit=3), Case("bias32", 1, 4, 384, 128, ksplit=3)]
    return out


def _k256_feature_cases():
    """256^2 kernel, one tile per workgroup, through the features only it has (they force it at any M).  N % 256 == 128 is the clamped, guarded
    last column tile; qcols = 136 is a multiple of 8 that is not a tile edge."""
    out = []
    for M, N, K in [(1, 256, 128), (255, 384, 384), (257, 640, 128), (257, 256, 384), (1, 640, 384), (255, 640, 128)]:
        out += [Case("res", M, N, K, 128, feat="rowsq"), Case("res", M, N, K, 128, feat="x16"), Case("res", M, N, K, 128, feat="x16", row_scale=True)]
        out += [Case("bias16", M, N, K, 128, feat="fold", qcols=q) for q in ((0, 136) if N > 136 else (0,))]
    return out


# 16 x 8 = 128 tiles with a last row tile of one row, two K-tiles; N % 256 == 128: 26 x 5 = 130 tiles, a quarter of the last column tile empty
K256_PLAIN_SHAPES = [(15 * 256 + 1, 2048, 128), (25 * 256 + 1, 1152, 256)]


def _k256_plain_cases():
    out = []
    for M, N, K in K256_PLAIN_SHAPES:
        out += [Case(epi, M, N, K, 256) for epi in ("gelu", "pair", "split", "grad", "bias32", "res")] + [Case("grad", M, N, K, 256, feat="colsum")]
        out += [Case("bias16", M, N, K, 256, qcols=136), Case("res", M, N, K, 256, row_scale=True, res_scaled=True), Case("res", M, N, K, 256, inplace=True),
                Case("pos", M, N, K, 256, pos=(196, 199, 2))]
    return out


K128_CASES, K256_FEATURE_CASES, K256_PLAIN_CASES = _k128_cases(), _k256_feature_cases(), _k256_plain_cases()
K256_SPLITK_CASES = [Case("bias32", 769, 2048, 256, 256, ksplit=2)]          # M N >= 256^2, 4 x 8 tiles x 2 slices = 64 workgroups, slices of two K-tiles
LN_CASES = [Case("res", 257, 768, 128, 128, feat="ln"), Case("res", 63, 384, 128, 128, feat="ln"), Case("res", 129, 384, 128, 128, feat="ln")]
TN_CASES = [(128, 128, 128, 1), (640, 128, 256, 2), (896, 256, 128, 3)]


def persistent_case(cus, epi):
    """At least 2 x CUs tiles of 256 x 256 at K = 256: the prefetching persistent launch."""
    return Case(epi, 256 * ((2 * cus + 7) // 8) + 1, 2048, 256, 256, qcols=136 if epi == "bias16" else 0)
