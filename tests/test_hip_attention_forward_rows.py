"""Every attention FORWARD kernel on the GPU, per ROW against fp64, at every instantiation its dispatcher can select and in both operand types: the
LDS-resident kernel (pv_attn_kernel: 3 head widths x 26 tile counts, without and with the row statistics), its workgroup-to-(image, head) map, the
streaming kernel (six widths, with statistics, with a weighted last key), the class-row forward (pv_attn_rows_kernel) and the two fp32-input kernels
of the fallback modes (pv_attn_f32_kernel, pv_attn_split_kernel).

The older tests assert a whole-tensor relative L2, which one wrong row of a 197-row image passes (tests/test_attn_forward_ref_host.py plants such
faults).  Here every (image, head, row) is measured against its own norm (attn_backward_ref.row_err) and the level is set by a stock-op restatement
with the kernel's rounding points (attn_backward_ref.restated_forward and relatives; the module's docstring names the points per kernel), never by
the kernel:

    max over rows of e(kernel)  <=  2 x max over rows of e(restated) + 1e-5                                     (attn_backward_ref.row_condition)
    max |lse - fp64|            <=  2 x max |lse_restated - fp64| + 2 fp32 ulps at the case's largest |lse|    (attn_backward_ref.lse_condition)

Every input is a view of a buffer with one NaN row behind it, every output has a NaN guard row that must still be NaN; results are finite; two
launches give identical bits; each call is one launch.  Families: gaussian, and at the ragged lengths "spread" (q, k times 6: scores over tens of
units) and "edge" (the k rows of the last key and of the first key of the last tile times 3).  DESIGN.md section 26 has what these tests measured."""
import math

import pytest
import torch

import attn_backward_ref as R
from test_hip_attention_backward_rows import _guarded, _kept, _out
from peekvit_amd import _lib, engine, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bf16", "f16"]
NAN = float("nan")
LN7 = math.log(7.0)


def _lengths(tiles):
    return (2, 13, 16) if tiles == 1 else (16 * tiles - 15, 16 * tiles - 3, 16 * tiles)          # one row in the last tile, a ragged tile, a full one


def _qkv(B, S, H, dh, family="gaussian", tile=16):
    return _guarded(R.inputs(B, S, H, dh, _lib.operand_dtype(), family, DEV, first_of_last=tile * ((S + tile - 1) // tile - 1))[0])


def _forward(call, B, S, H, dh, with_lse):
    """Two launches of call(out, lse) into guarded NaN buffers and the common checks: (out [B, S, D], lse [B, H, S] or None)."""
    D, dt = H * dh, _lib.operand_dtype()
    runs = []
    for _ in range(2):
        o_buf, out = _out((B, S, D), dt)
        l_buf, lse = _out((B * H, S), torch.float32) if with_lse else (None, None)
        n0 = ops.launch_count
        call(out, lse.view(B, H, S) if with_lse else None)
        assert ops.launch_count == n0 + 1
        runs.append((o_buf, out, l_buf, lse))
    torch.cuda.synchronize()
    (o_buf, out, l_buf, lse), second = runs
    assert _kept(o_buf) and (not with_lse or _kept(l_buf)), (S, dh)
    assert torch.equal(out, second[1]) and (not with_lse or torch.equal(lse, second[3]))          # two launches: identical bits
    return out, (lse.view(B, H, S) if with_lse else None)


def _check(label, out, lse, qkv, B, S, H, dh, family, block=None, tail=0.0, images=None):
    """The row condition of `out` (and the lse condition of `lse`) against fp64, levels from the kernel's restatement; `images`: a slice of the batch."""
    if images is not None:
        out, qkv, lse = out[images], qkv[images], (None if lse is None else lse[images])
        B = out.shape[0]
    ref, lse64 = R.fp64_forward(qkv, B, S, H, dh, tail)
    rs, rs_lse = R.restated_forward(qkv, B, S, H, dh, tail_log_mult=tail, block=block)
    bad = R.row_condition(label, R.forward_row_errors(out, ref, B, S, H, dh), R.forward_row_errors(rs, ref, B, S, H, dh), prefix="")
    if lse is not None:
        bad += R.lse_condition(label, lse, rs_lse, lse64)
        if family == "gaussian":
            assert float((lse.double() - lse64).abs().max()) < 1e-4, label          # the project's absolute bound (not for "spread": fp32 alone reaches 6e-5 there)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the resident kernel: pv_attn_kernel<DH, NKT, LSE>, S <= 416
# ---------------------------------------------------------------------------------------------------------------------------------
def _resident(B, S, H, dh, family, label, images=None):
    """ops.attention without and with lse=: identical outputs, the row and the lse condition.  (qkv, out)."""
    qkv = _qkv(B, S, H, dh, family)
    out, _ = _forward(lambda o, l: ops.attention(qkv, o, B, S, H, dh), B, S, H, dh, False)
    out2, lse = _forward(lambda o, l: ops.attention(qkv, o, B, S, H, dh, lse=l), B, S, H, dh, True)
    assert torch.equal(out, out2), label                                              # the statistics change no output bit
    for im in ([None] if images is None else images):
        _check(label + ("" if im is None else f" images {im.start}.."), out, lse, qkv, B, S, H, dh, family, images=im)
    return qkv, out


RESIDENT = [(dh, t) for dh in (32, 48, 64) for t in range(1, 27)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh,tiles", RESIDENT, ids=[f"dh{dh}-{t}tiles" for dh, t in RESIDENT])
def test_resident_forward_rows_every_instantiation(dh, tiles, mode):
    """pv_attention_bf16 and pv_attention_lse_bf16 at NKT = tiles: every staging-iteration count, wait immediate, partial last iteration, q tiles per wave
    and the K = 16 tail of odd tile counts."""
    with engine.precision(mode):
        for S in _lengths(tiles):
            for family in (("gaussian", "spread", "edge") if S == 16 * tiles - 3 else ("gaussian",)):
                _resident(3, S, 2, dh, family, f"resident {family} dh {dh} S {S} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh", [32, 48, 64])
def test_resident_forward_of_a_single_token(dh, mode):
    """pv_attention_bf16 / pv_attention_lse_bf16 at S = 1: p = 1 and l = 1, the output row IS v; lse = s log2(e) within the lse condition."""
    B, S, H = 3, 1, 2
    D = H * dh
    with engine.precision(mode):
        qkv, out = _resident(B, S, H, dh, "gaussian", f"resident gaussian dh {dh} S 1 {mode}")
    assert torch.equal(out, qkv[..., 2 * D:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh", [32, 48, 64])
def test_resident_forward_with_statistics_refuses_a_length_past_its_range(dh, mode):
    """pv_attention_lse_bf16 at S = 417: the streaming kernel behind pv_attention_bf16 keeps no statistics."""
    B, S, H = 3, 417, 2
    with engine.precision(mode):
        qkv = _qkv(B, S, H, dh)
        o_buf, out = _out((B, S, H * dh), _lib.operand_dtype())
        l_buf, lse = _out((B * H, S), torch.float32)
        with pytest.raises(_lib.PeekvitHipError):
            ops.attention(qkv, out, B, S, H, dh, lse=lse.view(B, H, S))
        torch.cuda.synchronize()
    assert bool(torch.isnan(o_buf.float()).all()) and bool(torch.isnan(l_buf).all())            # nothing was stored


# ---------------------------------------------------------------------------------------------------------------------------------
# b. pv_bh_map: workgroups of complete groups of eight images are dealt image-first, the rest head-first
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H", [(13, 6), (67, 12)])
@pytest.mark.parametrize("tiles", [2, 13])
@pytest.mark.parametrize("dh", [32, 48, 64])
def test_resident_forward_maps_workgroups_to_images_and_heads(dh, tiles, B, H, mode):
    """pv_attention_bf16 / pv_attention_lse_bf16 from B = 8 on: the first and the last four images hold the row condition (the grouped branch and
    the remainder), and image 0 has the bits of the same image run alone (B = 1: the remainder branch only)."""
    S = 16 * tiles - 3
    with engine.precision(mode):
        qkv, out = _resident(B, S, H, dh, "gaussian", f"map B {B} H {H} dh {dh} S {S} {mode}", images=(slice(0, 4), slice(B - 4, B)))
        first = _guarded(qkv[:1].clone())
        alone, _ = _forward(lambda o, l: ops.attention(first, o, 1, S, H, dh), 1, S, H, dh, False)
    assert torch.equal(out[:1], alone)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the streaming kernel: pv_attn_stream_kernel<DH, LSE, W>, 64-key blocks with an online softmax
# ---------------------------------------------------------------------------------------------------------------------------------
NINE = (1, 2, 63, 64, 65, 127, 129, 200, 449)
STREAM = [("plain", dh) for dh in (32, 48, 64, 80, 96, 128)] + [(v, dh) for v in ("lse", "w") for dh in (32, 48, 64)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant,dh", STREAM, ids=[f"{v}-dh{dh}" for v, dh in STREAM])
def test_streaming_forward_rows_every_instantiation(variant, dh, mode):
    """plain: pv_attention_bf16 past S = 416 (dh 32 / 48 / 64) and at every length (dh 80 / 96 / 128).  lse: ops.attention_stream.  w: ops.attention_stream_w
    with tail_log_mult 0 (the unweighted kernel's bits) and ln 7 (the fp64 reference adds ln 7 to the last key's score).  Past 416 the kernel with
    statistics stores pv_attention_bf16's bits."""
    B, H = 3, 2
    lengths = (417, 448, 449) if variant == "plain" and dh <= 64 else NINE
    with engine.precision(mode):
        for S in lengths:
            for family in (("gaussian", "spread", "edge") if S in (65, 449) else ("gaussian",)):
                qkv = _qkv(B, S, H, dh, family, tile=64)
                label = f"streaming {variant} {family} dh {dh} S {S} {mode}"
                if variant == "plain":
                    out, _ = _forward(lambda o, l: ops.attention(qkv, o, B, S, H, dh), B, S, H, dh, False)
                    _check(label, out, None, qkv, B, S, H, dh, family, block=64)
                    continue
                out, lse = _forward(lambda o, l: ops.attention_stream(qkv, o, l, B, S, H, dh), B, S, H, dh, True)
                if S > 416:
                    plain, _ = _forward(lambda o, l: ops.attention(qkv, o, B, S, H, dh), B, S, H, dh, False)
                    assert torch.equal(out, plain), label
                if variant == "lse":
                    _check(label, out, lse, qkv, B, S, H, dh, family, block=64)
                    continue
                w0, lse0 = _forward(lambda o, l: ops.attention_stream_w(qkv, o, l, B, S, H, dh, 0.0), B, S, H, dh, True)
                assert torch.equal(w0, out) and torch.equal(lse0, lse), label                       # a weight of 1: the unweighted kernel's bits
                w7, lse7 = _forward(lambda o, l: ops.attention_stream_w(qkv, o, l, B, S, H, dh, LN7), B, S, H, dh, True)
                _check(label + " weight 1", w0, lse0, qkv, B, S, H, dh, family, block=64)
                _check(label + " weight 7", w7, lse7, qkv, B, S, H, dh, family, block=64, tail=LN7)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the class-row forward: pv_attn_rows_kernel, one wave per (image, head, query row), 64 / CPL keys per step
# ---------------------------------------------------------------------------------------------------------------------------------
KEYS_PER_STEP = {32: 16, 48: 8, 64: 8, 80: 4, 96: 4, 128: 4}          # KPI = 64 / CPL, CPL = 4 / 8 / 16 lanes per key for dh / 8 <= 4 / 8 / 16 chunks


def _class_rows(B, S, H, dh, nq, label, peaked=False):
    D, dt = H * dh, _lib.operand_dtype()
    q, kv, _ = R.rows_inputs(B, S, H, dh, dt, peaked, DEV, nq=nq)
    q = _guarded(q)
    wide_kv = torch.full((B * S + 1, 2 * D + 8), NAN, dtype=dt, device=DEV)                  # kv and out: views of wider buffers with a NaN row behind
    wide_kv[:B * S, :2 * D] = kv
    kv = wide_kv[:B * S, :2 * D]
    runs = []
    for _ in range(2):
        wide = torch.full((B * nq + 1, D + 8), NAN, dtype=dt, device=DEV)
        n0 = ops.launch_count
        ops.attention_rows(q, kv, wide[:B * nq, :D], B, S, nq, H, dh)
        assert ops.launch_count == n0 + 1
        runs.append(wide)
    torch.cuda.synchronize()
    wide, second = runs
    out = wide[:B * nq, :D]
    assert bool(torch.isfinite(out.float()).all()), label
    assert bool(torch.isnan(wide[B * nq:].float()).all()) and bool(torch.isnan(wide[:, D:].float()).all())          # the guard row and the pad columns
    assert torch.equal(out, second[:B * nq, :D])
    qh = q.view(B, nq, H, dh).transpose(1, 2)
    kh, vh = (kv[:, i * D:(i + 1) * D].reshape(B, S, H, dh).transpose(1, 2) for i in (0, 1))
    ref = torch.softmax(qh.double() @ kh.double().transpose(-1, -2), -1) @ vh.double()
    rs, _ = R.attend_restated(qh.float() @ kh.float().transpose(-1, -2), vh.float(), dt, p16=False)          # restated_forward(p16=False)'s core
    got = out.view(B, nq, H, dh).transpose(1, 2)
    bad = R.row_condition(label, {"out": R.row_err(got.float(), ref)}, {"out": R.row_err(rs.to(dt).float(), ref)}, what="(image, head, query)", prefix="")
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("dh", [32, 48, 64, 80, 96, 128])
def test_class_row_forward_rows(dh, nq, mode):
    """pv_attention_rows_bf16: 3 x 2 x nq waves (the last workgroup has idle waves), lengths around the keys of one step and of four steps."""
    step = KEYS_PER_STEP[dh]
    with engine.precision(mode):
        for S in sorted({1, 2, step - 1, step, step + 1, 4 * step + 1, 257}):
            _class_rows(3, S, 2, dh, nq, f"class-row gaussian dh {dh} nq {nq} S {S} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [1, 3])
def test_class_row_forward_on_peaked_rows(nq, mode):
    """pv_attention_rows_bf16 with the query rows times 12: the probability sits on one key."""
    with engine.precision(mode):
        _class_rows(3, 197, 2, 64, nq, f"class-row peaked dh 64 nq {nq} S 197 {mode}", peaked=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. the fp32-input kernels of the fallback modes: pv_attn_f32_kernel and pv_attn_split_kernel, one instantiation per tile count
# ---------------------------------------------------------------------------------------------------------------------------------
F32 = [(dh, t) for dh in (48, 64) for t in range(1, 14)] + [(32, t) for t in range(1, 27)]
F32_IDS = [f"dh{dh}-{t}tiles" for dh, t in F32]


def _fp32_launch(op, qkv, B, S, H, dh, width):
    """Two launches of an fp32-input kernel into guarded [B S, width] outputs of the operand type and the common checks."""
    runs = []
    for _ in range(2):
        o_buf, out = _out((B * S, width), _lib.operand_dtype())
        n0 = ops.launch_count
        op(qkv, out, B, S, H, dh)
        assert ops.launch_count == n0 + 1
        runs.append((o_buf, out))
    torch.cuda.synchronize()
    assert _kept(runs[0][0]) and torch.equal(runs[0][1], runs[1][1])
    return runs[0][1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh,tiles", F32, ids=F32_IDS)
def test_fp32_forward_rows_every_tile_count(dh, tiles, mode):
    """pv_attention_f32_split: the hi plane twice, hi + lo per row against fp64 on the fp32 inputs; the floor 2^-20 is the fp32 summation-order term
    sqrt(416) 2^-24, all the error this kernel has."""
    B, S, H = 3, 16 * tiles - 3, 2
    D = H * dh
    with engine.precision(mode):
        qkv = _guarded(R.inputs32(B, S, H, dh, device=DEV))
        planes = _fp32_launch(ops.attention_f32, qkv, B, S, H, dh, 3 * D).view(B, S, 3 * D)
        assert torch.equal(planes[..., :D], planes[..., 2 * D:])
        got = planes[..., :D].double() + planes[..., D:2 * D].double()
        rs = R.restated_forward_f32(qkv, B, S, H, dh, _lib.operand_dtype()).double()
        ref = R.fp64_forward(qkv, B, S, H, dh)[0]
        bad = R.row_condition(f"fp32 gaussian dh {dh} S {S} {mode}", R.forward_row_errors(got, ref, B, S, H, dh),
                              R.forward_row_errors(rs[..., :D] + rs[..., D:2 * D], ref, B, S, H, dh), prefix="", floor=2.0 ** -20)
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh,tiles", F32, ids=F32_IDS)
def test_split_score_forward_rows_every_tile_count(dh, tiles, mode):
    """pv_attention_split_bf16 on Gaussian fp32 inputs and with q, k times 6, against the restatement with its two-halves scores."""
    B, S, H = 3, 16 * tiles - 3, 2
    with engine.precision(mode):
        for amp in (1.0, 6.0):
            qkv = _guarded(R.inputs32(B, S, H, dh, amp, DEV))
            out = _fp32_launch(lambda x, o, *a: ops.attention_split(x.view(B * S, -1), o, *a), qkv, B, S, H, dh, H * dh).view(B, S, H * dh)
            rs = R.restated_forward_split(qkv, B, S, H, dh, _lib.operand_dtype())
            ref = R.fp64_forward(qkv, B, S, H, dh)[0]
            bad = R.row_condition(f"split x{amp:g} dh {dh} S {S} {mode}", R.forward_row_errors(out, ref, B, S, H, dh),
                                  R.forward_row_errors(rs, ref, B, S, H, dh), prefix="")
            assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh,S", [(64, 221), (48, 221), (32, 429)])
@pytest.mark.parametrize("entry", ["f32", "split"])
def test_fp32_input_forwards_refuse_one_tile_count_past_their_range(entry, dh, S, mode):
    """pv_attention_f32_split and pv_attention_split_bf16 at 14 (dh 48 / 64) and 27 (dh 32) tiles: refused, nothing stored."""
    B, H = 3, 2
    with engine.precision(mode):
        qkv = _guarded(R.inputs32(B, S, H, dh, device=DEV))
        o_buf, out = _out((B * S, (3 if entry == "f32" else 1) * H * dh), _lib.operand_dtype())
        with pytest.raises(_lib.PeekvitHipError):
            if entry == "f32":
                ops.attention_f32(qkv, out, B, S, H, dh)
            else:
                ops.attention_split(qkv.view(B * S, -1), out, B, S, H, dh)
        torch.cuda.synchronize()
    assert bool(torch.isnan(o_buf.float()).all())
