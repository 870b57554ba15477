"""CPU side of the exact GEMM tests (tests/test_hip_gemm_exact.py): the builder's conditions hold for every case the GPU file runs, the comparator
passes a correct output and finds every planted fault, and the dispatcher keeps the 256-row kernels inside the row strides their 32-bit per-lane
offsets can address (asked through pv_gemm_tile_rows, which never launches).

For each planted fault the test also measures what the OLDER tests would have said: the same fault planted into the correctly rounded output of
Gaussian operands at (M, N, K) = (394, 2304, 768) of test_hip_ops.GEMM_SHAPES, as rel_l2 against fp64, next to their cap (3e-3 on 16-bit outputs,
2e-6 on fp32 ones).  The verdicts are printed (pytest -s) and recorded in DESIGN.md section 28; nothing is presumed about them here."""
import math

import pytest
import torch

import gemm_exact_ref as R
from conftest import rel_l2
from peekvit_amd import ops

DTYPES = [torch.bfloat16, torch.float16]
MI355X_CUS = 256
PV_ERR_UNSUPPORTED = -2              # include/peekvit_hip.h
GPU_CASES = (R.K128_CASES + R.K256_FEATURE_CASES + R.K256_PLAIN_CASES + R.K256_SPLITK_CASES + R.LN_CASES +
             [R.persistent_case(MI355X_CUS, "bias16"), R.persistent_case(MI355X_CUS, "res")])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_builder_conditions_hold_for_every_gpu_case(dtype):
    """Problem() asserts the integer argument's conditions on the fp64 reference while it builds (worst case below 2^24 grains, inside the fp16
    range, row-statistic and column sums below 2^24); here on top: at least half of the BIAS_BF16 / GELU_GRAD outputs needed rounding (the
    column-sum cases excepted), x16_out is rounded on as many columns as its exact row statistics allow, every large GELU case hits all 64 table
    intervals with in-range pre-activations (and all cases together do), no two cases share an id, and a correct output passes the comparator."""
    assert len({c.id for c in GPU_CASES}) == len(GPU_CASES)
    hit = set()
    for c in GPU_CASES:
        P = R.build(c, dtype, "cpu")
        if P.rounded_share is not None:
            assert P.rounded_share >= 0.5, (c.id, P.rounded_share)
        if c.feat == "x16":
            assert P.x16_rounded_share >= R.X16_SPIKES[dtype] / 256, (c.id, P.x16_rounded_share)
        if hasattr(P, "intervals_hit"):
            assert c.M * c.N < 16384 or P.intervals_hit == R.GELU_N, (c.id, P.intervals_hit)
            hit |= P.intervals
        if c.M * c.N <= 257 * 640:
            o = P.emulate(P.fresh_outputs())
            assert P.findings(o, 128) == [], c.id
            assert all(R.same_bits(k, o[k][0], P.emulate(P.fresh_outputs())[k][0]) == [] for k in o)
    assert len(hit) == R.GELU_N
    for K, M, N, ks in R.TN_CASES:
        a, b, exp = R.tn_problem(K, M, N, ks, dtype, "cpu")
        assert a.stride(0) > M and b.stride(0) > N and torch.equal(exp.sum(0), a.double().t() @ b.double())


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------------
FAULT_CASE = R.Case("bias16", 129, 256, 192, 128, qcols=68)
SPLITK_CASE = R.Case("bias32", 129, 132, 128, 128, ksplit=2)


def _truncate(x64, dtype):
    """Round toward zero to the 16-bit type (what a conversion that drops the low bits does)."""
    r = x64.to(dtype)
    over = r.double().abs() > x64.abs()
    return (r.view(torch.int16) - over.to(torch.int16)).view(dtype)       # one ulp toward zero: the bit pattern minus one, whatever the sign


def _plant(fault, out, buf, exp64, dtype, qcols=68, qscale=0.25):
    """Plant one fault into a correct output (view `out` of `buf`; exp64: its fp64 expectation, q-scaled up to column qcols)."""
    if fault == "zeroed 4-column group":
        out[77, 132:136] = 0
    elif fault == "one element off by one ulp":
        out.view(torch.int16)[100, 201] += 1
    elif fault == "truncation instead of round-to-nearest-even":
        out.copy_(_truncate(exp64, dtype))
    elif fault == "q-scale on one 8-column chunk too many":
        out[:, qcols:qcols + 8] = (exp64[:, qcols:qcols + 8] * qscale).to(dtype)
    elif fault == "write into a padding column":
        buf[5, R.pad_left(dtype) + out.shape[1]] = 1.0
    elif fault == "write into the guard row":
        buf[out.shape[0], R.pad_left(dtype) + 3] = 1.0
    elif fault == "two exchanged rows":
        out[[40, 41]] = out[[41, 40]]
    else:
        raise ValueError(fault)


FAULTS = ["zeroed 4-column group", "one element off by one ulp", "truncation instead of round-to-nearest-even", "q-scale on one 8-column chunk too many",
          "write into a padding column", "write into the guard row", "two exchanged rows"]
_gauss = {}


def _gaussian(dtype):
    """Correctly rounded output of Gaussian operands at (394, 2304, 768) and its fp64 reference (q-scale 0.125 on a third of the columns, as
    test_gemm_epilogues), computed once per type."""
    if dtype not in _gauss:
        g = torch.Generator().manual_seed(7)
        M, N, K = 394, 2304, 768
        a = torch.randn(M, K, generator=g).to(dtype).double()
        w = ((torch.rand(N, K, generator=g) * 2 - 1) / math.sqrt(K)).to(dtype).double()
        bias = ((torch.rand(N, generator=g) * 2 - 1) * 0.1).double()
        ref = a @ w.t() + bias
        _gauss[dtype] = (ref, bias)
    return _gauss[dtype]


def _old_verdict(fault, dtype):
    """rel_l2 of the fault planted into the correctly rounded Gaussian output, against the older tests' cap."""
    ref, bias = _gaussian(dtype)
    q = (ref.shape[1] // 3) // 4 * 4
    exp = ref.clone()
    exp[:, :q] *= 0.125
    buf, out = R.guarded(*exp.shape, dtype, "cpu", None)
    out.copy_(exp)
    base = rel_l2(out, exp)
    _plant(fault, out, buf, exp, dtype, qcols=q, qscale=0.125)
    return base, rel_l2(out, exp)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("fault", FAULTS)
def test_comparator_finds_planted_fault(fault, dtype):
    P = R.build(FAULT_CASE, dtype, "cpu")
    o = P.emulate(P.fresh_outputs())
    assert P.findings(o, 128) == []
    buf, out = o["out"]
    _plant(fault, out, buf, P.expected["out"], dtype)
    found = P.findings(o, 128)
    assert len(found) == 1, found
    print(f"\n[{dtype}] {fault}: {found[0]}")
    where = {"zeroed 4-column group": "first at (row 77, column 132); wrong set: 1 whole 4-column store group(s)",
             "one element off by one ulp": "1 of 33024 elements wrong, first at (row 100, column 201)",
             "q-scale on one 8-column chunk too many": "first at (row 0, column 68)",
             "write into a padding column": "padding column", "write into the guard row": "guard row",
             "two exchanged rows": "2 whole row(s)"}
    assert where.get(fault, "elements wrong") in found[0]
    if fault == "q-scale on one 8-column chunk too many":
        assert "(rows 0:129, columns 68:76)" in found[0]
    base, err = _old_verdict(fault, dtype)
    print(f"[{dtype}] {fault}: rel_l2 at (394, 2304, 768) {err:.2e} (correctly rounded: {base:.2e}) -> the old 3e-3 cap {'PASSES' if err < 3e-3 else 'fails'} it")


def test_comparator_finds_bias_added_to_split_k_slice_1():
    P = R.build(SPLITK_CASE, torch.bfloat16, "cpu")
    o = P.emulate(P.fresh_outputs())
    assert P.findings(o, 128) == []
    M = SPLITK_CASE.M
    o["slices"][1][M:2 * M] += P.bias
    found = P.findings(o, 128)
    assert len(found) == 1 and "first at (row 129, column" in found[0], found
    # what the older tests see: only the SUM of the slices, against the 2e-6 cap of fp32 outputs
    ref, bias = _gaussian(torch.bfloat16)
    err = rel_l2((ref + bias).float(), ref)
    print(f"\nbias added to slice 1 as well: {found[0]}\nrel_l2 of the summed slices at (394, 2304, 768) {err:.2e} -> the old 2e-6 cap {'PASSES' if err < 2e-6 else 'fails'} it")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_comparator_finds_a_truncating_x16_conversion(dtype):
    """x16_out is the 16-bit rounding of the fp32 output.  The row statistics of the same launch must stay exact, which leaves room for 64 (bf16) or
    2 (fp16) values per 256-wide column tile that the type cannot hold (gemm_exact_ref._x16_spikes): enough for the comparator to see a conversion
    that truncates, on the very first row."""
    case = next(c for c in R.K256_FEATURE_CASES if c.feat == "x16" and c.M == 257 and c.N == 640 and not c.row_scale)
    P = R.build(case, dtype, "cpu")
    o = P.emulate(P.fresh_outputs())
    assert P.findings(o, 256) == []
    o["x16"][1].copy_(_truncate(P.expected["x16"], dtype))
    found = P.findings(o, 256)
    assert len(found) == 1 and found[0].startswith("x16:") and "first at (row 0, column" in found[0], found
    print(f"\n[{dtype}] truncating x16_out ({P.x16_rounded_share:.4f} of its values need rounding): {found[0]}")


def test_gemm_tile_rows_refuses_a_misspelt_member():
    from peekvit_amd._lib import PeekvitHipError
    with pytest.raises(PeekvitHipError):
        ops.gemm_tile_rows(256, 256, 128, R.EPI["res"], lad=1024)


# ---- the 256-row kernels' stride limits ----------------------------------------------------------------------------------------------------------
def test_dispatcher_keeps_256_row_kernels_inside_their_stride_limits():
    """pv_gemm256_tile addresses its operands with a 64-bit block base + (uint32_t)(row * (int)ld + chunk * 8) * 2u, row <= 255, chunk <= 7: lda and
    ldw up to (2^31 - 1 - 56) / 255 = 8421504; its pipelined 16-bit epilogue walks one uint32 byte offset to row 255, chunk 31 (+ N for the pair's
    second plane): 255 ldo + 248 + N_pair <= 2^31 - 1.  One step (8 elements) past a limit pv_gemm_tile_rows never answers 256 - the 128^2 kernel,
    whose addressing is 64-bit, or PV_ERR_UNSUPPORTED where only a 256-row kernel can serve the call - and one step inside it answers as before.
    Nothing is launched (fake aligned pointers)."""
    E = R.EPI
    M, N, K = 4096, 2048, 128                                         # 16 x 8 = 128 tiles: the 256^2 kernel for every epilogue
    lim = (2 ** 31 - 1 - 56) // 255
    assert lim == 8421504 and lim % 8 == 0
    for name in ("bias16", "gelu", "pair", "split", "grad", "bias32", "res"):
        assert ops.gemm_tile_rows(M, N, K, E[name]) == 256
        for ld in ("lda", "ldw"):
            assert ops.gemm_tile_rows(M, N, K, E[name], **{ld: lim}) == 256, (name, ld)
            assert ops.gemm_tile_rows(M, N, K, E[name], **{ld: lim + 8}) == 128, (name, ld)
        assert ops.gemm_tile_rows(M, N, K, E[name], lda=lim + 8, ksplit=2 if name == "bias32" else 0) == 128
    for name, extra in (("bias16", 0), ("gelu", 0), ("pair", N)):
        inside = (2 ** 31 - 1 - 248 - extra) // 255 // 8 * 8
        assert 255 * inside + 248 + extra <= 2 ** 31 - 1 < 255 * (inside + 8) + 248 + extra
        assert ops.gemm_tile_rows(M, N, K, E[name], ldo=inside) == 256, name
        assert ops.gemm_tile_rows(M, N, K, E[name], ldo=inside + 8) == 128, name
    for name in ("bias32", "res", "split", "grad"):                  # fp32 outputs and the one-pass 16-bit stores index rows in 64 bits
        assert ops.gemm_tile_rows(M, N, K, E[name], ldo=lim + 8, ldr=lim + 8) == 256, name
    # the fused-LayerNorm rows kernel stages through the same tile: refused, not rerouted; the full-row kernel (64-bit staging) is not limited
    ln = dict(ln_out=16, ln_gamma=16, ln_beta=16)
    inside_rows, inside_full = ops.gemm_tile_rows(M, 768, K, E["res"], lda=lim, **ln), ops.gemm_tile_rows(M, 384, K, E["res"], lda=lim, **ln)
    assert inside_rows > 0 and inside_full > 0
    assert ops.gemm_tile_rows(M, 768, K, E["res"], lda=lim + 8, **ln) == PV_ERR_UNSUPPORTED
    assert ops.gemm_tile_rows(M, 768, K, E["res"], ldw=lim + 8, **ln) == PV_ERR_UNSUPPORTED
    assert ops.gemm_tile_rows(M, 384, K, E["res"], lda=lim + 8, **ln) == inside_full
