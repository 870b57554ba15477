"""Every GEMM kernel on the GPU, ELEMENT BY ELEMENT against an exact expectation, in both operand types, on strided and guarded buffers.

The older GEMM tests assert a whole-tensor relative L2 (3e-3 on 16-bit outputs), which a zeroed store group, a truncating conversion or a q-scale
applied one chunk too far pass (tests/test_gemm_exact_host.py plants them), or bit identity between kernels, which proves that they agree, not that
either is right.  Here the operands are integers (gemm_exact_ref: every partial sum is an exact fp32 number in any summation order), so

    fp32 outputs     torch.equal to the fp64 expectation cast to fp32
    16-bit outputs   bit-equal to the expectation rounded once to the operand type
    GELU planes      per element inside the project's existing bounds (0.006 |ref| + 2e-5; 1.0e-4 + 1.13 * 2^-8 for gelu') against fp64 of the
                     EXACT pre-activation, every table interval hit where the output has 16 K elements or more
    every launch     NaN padding columns, the NaN guard row and the rows a remap skips untouched; two launches bit-identical; one launch per call

Each case first asks the dispatcher (ops.gemm_tile_rows, the case's own strides) which tile it would take and asserts the tile the case is meant
for, so a dispatcher change cannot silently move it.  A feature of the 256-row kernel (rowsq_out, x16_out + rowstat_out, fold) is not part of that
query (pv_gemm_tile_rows answers for the plain call); with it the dispatcher takes the 256-row kernel or returns PV_ERR_UNSUPPORTED, so a successful
launch ran that kernel - and only that kernel writes rowsq_out, x16_out, rowstat_out or applies the fold: had the call fallen through to the 128^2
kernel, those outputs would still hold their NaN fill (the fold: a plain product) and the comparison would fail.  Likewise the fused LayerNorm's
output must be written and finite in every row.

Shapes that differ from the first choice, because the dispatcher does not give that one to the kernel under test:
  * features at N = 128: a single 256-wide column tile half empty is refused (n_ok: at most a quarter of the last tile may be empty); N = 256 instead;
  * colsum_out at a small M: ops.gemm fuses the column sums only where the plain call takes the 256-row kernel, so the fused column sums run at the
    two plain 256^2 shapes (with small products: the sums over thousands of rows must stay exact);
  * 256^2 with N % 256 == 128: (6401, 1152, 256), 26 x 5 = 130 tiles;
  * res_scaled on the 128^2 kernel at N = 4 and 132 only: the dispatcher refuses it at the full-row kernel's widths (N = 256), whatever M.
DESIGN.md section 28 has the case table and what the run measured."""
import pytest
import torch

import gemm_exact_ref as R
from peekvit_amd import _lib, engine, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bf16", "f16"]
FEATURES_256 = ("rowsq", "x16", "fold", "colsum")


def _run(case, mode):
    """Build, ask the dispatcher, launch twice, compare: returns (problem, first launch's outputs)."""
    with engine.precision(mode):
        P = R.build(case, _lib.operand_dtype(), DEV)
        o1, o2 = P.fresh_outputs(), P.fresh_outputs()
        assert ops.gemm_tile_rows(case.M, case.N, case.K, R.EPI[case.epi], **P.query_fields(o1)) == case.tile
        if P.rounded_share is not None:
            print(f"{case.id} [{mode}]: {P.rounded_share:.2f} of the outputs needed rounding")
            assert P.rounded_share >= 0.5
        if case.feat == "x16":          # as many rounded x16_out values as the exact row statistics leave room for (gemm_exact_ref._x16_spikes)
            assert P.x16_rounded_share >= R.X16_SPIKES[P.dtype] / 256
        if hasattr(P, "intervals_hit") and case.M * case.N >= 16384:
            assert P.intervals_hit == R.GELU_N
        n0 = ops.launch_count
        P.launch(ops, o1)
        assert ops.launch_count - n0 == (2 if case.feat == "colsum" else 1)          # (ops.gemm sums the per-tile column sums in a second launch)
        P.launch(ops, o2)
        torch.cuda.synchronize()
        findings = P.findings(o1, 256 if case.tile == 256 or case.feat in FEATURES_256 else 128)
        for name in o1:
            findings += R.same_bits(name, o1[name][0], o2[name][0])
        assert not findings, "\n".join(findings)
    return P, o1


def _sum_of_slices(P, o, mode):
    """The slices through pv_sum_slices_f32: exact as well."""
    c = P.case
    with engine.precision(mode):
        buf, out = R.guarded(c.M, c.N, torch.float32, DEV, dense=True)
        n0 = ops.launch_count
        ops.sum_slices(P.slices_view(o).contiguous(), out)
        assert ops.launch_count - n0 == 1
        findings = R.compare_exact("sum of slices", out, P.expected["sum"]) + R.check_sentinels("sum of slices", buf, c.M, c.N)
        assert not findings, "\n".join(findings)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.K128_CASES, ids=lambda c: c.id)
def test_gemm128_every_epilogue_exact(case, mode):
    """pv_gemm_bf16 on the 128^2 kernel (pv_gemm_tile_rows says so for every case), every epilogue of the dispatcher's switch: M in {1, 127, 129}
    x N in {4, 132, 256} (a four-column last tile behind the clamp n = N - 4) x K in {64, 128, 192}, the q-scale boundary at 0 / 4 / 68 / N, the
    residual without / with row_scale / res_scaled / in place, the positional remap (row_off = 2, 55 > 50 + 2 output rows per image, M ending
    mid-image), split-K 2 and 3 (the bias in slice 0 only, every slice exact, and their sum through ops.sum_slices)."""
    P, o = _run(case, mode)
    if case.ksplit > 1:
        _sum_of_slices(P, o, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.K256_FEATURE_CASES, ids=lambda c: c.id)
def test_gemm256_features_exact(case, mode):
    """pv_gemm_bf16 on the 256^2 kernel, one tile per workgroup, through the features only it has: M in {1, 255, 257}, N in {256, 384, 640}
    (N % 256 == 128: the clamped, guarded last column tile), K in {128, 384}.  rowsq_out[tile][m] and rowstat_out[tile][m] = (sum, sum of
    squares) exact per column tile, x16_out = the 16-bit rounding of the fp32 output, the fold consumer rstd (acc - mean c1) + c2 with the q-scale
    ending at column 136."""
    _run(case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.K256_PLAIN_CASES, ids=lambda c: c.id)
def test_gemm256_plain_epilogues_exact(case, mode):
    """pv_gemm_bf16 on the 256^2 kernel (pv_gemm_tile_rows says so for every case) with the plain epilogues, which need 128 tiles:
    (3841, 2048, 128) - a last row tile of ONE row, two K-tiles, the shortest loop the kernel accepts - and (6401, 1152, 256) with the ragged last
    column tile; every epilogue, the pair and the gelu' product with its strided derivative plane (and the fused column sums) included.  K < 256
    or fewer than 2 x CUs tiles: one tile per workgroup.  Expectation in fp64 on the GPU."""
    _run(case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("epi", ["bias16", "res"])
def test_gemm256_persistent_launch_exact(epi, mode):
    """pv_gemm_bf16, the prefetching persistent launch of the 256^2 kernel: at least 2 x CUs tiles (the device's own count) and K = 256.  The
    other epilogues are tied to the one-tile kernel bit for bit by test_gemm_persistent_launch_is_bit_identical."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = R.persistent_case(cus, epi)
    assert ((case.M + 255) // 256) * (case.N // 256) >= 2 * cus and case.K >= 256
    _run(case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.K256_SPLITK_CASES, ids=lambda c: c.id)
def test_gemm256_split_k_exact(case, mode):
    """pv_gemm_bf16, 256^2 split-K (M N >= 256^2 and tiles x ksplit >= 64): exact slices, the bias in slice 0 only, and their exact sum."""
    P, o = _run(case, mode)
    _sum_of_slices(P, o, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: c.id)
def test_gemm_fused_layernorm_fp32_output_exact(case, mode):
    """pv_gemm_bf16 with the fused LayerNorm: the rows kernel (N = 768, M = 257) and the full-row kernel (N = 384, M in {63, 129}), strided res,
    ldo = N as the kernels require.  Only the fp32 output is exact; the LayerNorm output (two launches bit-identical here) is tied to
    pv_layernorm_bf16 by test_gemm_fused_layernorm_bit_identical_to_separate_kernels."""
    _run(case, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,M,N,ks", R.TN_CASES)
def test_gemm_tn_exact(K, M, N, ks, mode):
    """pv_gemm_tn_bf16: exact per slice (uneven last slice at 640 / 2 and 896 / 3 blocks of 128) and summed, both operands strided guarded views,
    ldo > N (the slices are the first N columns of a [ks, M, N + 8] buffer with NaN around them)."""
    with engine.precision(mode):
        a, b, exp = R.tn_problem(K, M, N, ks, _lib.operand_dtype(), DEV)
        parts = []
        for _ in range(2):
            buf = torch.full((ks * M + 1, N + 8), R.NAN, device=DEV)
            part = buf[:ks * M].view(ks, M, N + 8)[:, :, :N]
            n0 = ops.launch_count
            ops.gemm_tn(a, b, part, ks)
            assert ops.launch_count - n0 == 1
            parts.append((buf, part))
        buf, part = parts[0]
        findings = R.compare_exact("slices", part.reshape(ks * M, N), exp.view(ks * M, N), (256, 256)) + R.same_bits("slices", buf, parts[1][0])
        pad = buf.clone()
        pad[:ks * M, :N] = R.NAN
        findings += R.same_bits("padding columns and guard row", pad, torch.full_like(pad, R.NAN))
        dense, (obuf, out) = part.contiguous(), R.guarded(M, N, torch.float32, DEV, dense=True)
        ops.sum_slices(dense, out)
        findings += R.compare_exact("sum of slices", out, exp.sum(0)) + R.check_sentinels("sum of slices", obuf, M, N)
        assert not findings, "\n".join(findings)
