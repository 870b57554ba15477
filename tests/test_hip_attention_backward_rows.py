"""Every attention backward kernel of the training path on the GPU, per ROW against fp64: the two-pass kernels (pv_attention_bwd_bf16) at every
instantiation the dispatcher can select, the persistent kernel (pv_attention_bwd_lse_bf16), the class-row backward (pv_attention_rows_bwd_bf16) and
the streaming backward, in both operand types, on Gaussian inputs and on inputs with peaked rows.

The whole-tensor relative L2 of the older tests cannot see one wrong row of a 197-row image (tests/test_attn_backward_ref_host.py plants such
faults).  Here every (image, head, row) is measured against its own norm (attn_backward_ref.row_err) and the level is set by the stock-op
restatement with the kernel's rounding points (attn_backward_ref.restated, whose docstring names them per kernel), never by the kernel:

    max over rows of e(kernel)  <=  2 x max over rows of e(restated) + 1e-5        (attn_backward_ref.row_condition)

Every input is a view of a buffer with one NaN row behind the last image, every output has one NaN row behind it that must still be NaN; results
are finite; two launches give identical bits.  DESIGN.md section 24 has what these tests measured."""
import pytest
import torch

import attn_backward_ref as R
from conftest import rel_l2
from peekvit_amd import _lib, engine, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bf16", "f16"]
NAN = float("nan")


def _guarded(t):
    """A copy of t ([..., C], any leading shape) as a view of a buffer with one trailing row of NaN."""
    C = t.shape[-1]
    buf = torch.full((t.numel() // C + 1, C), NAN, dtype=t.dtype, device=t.device)
    buf[:-1] = t.reshape(-1, C)
    return buf[:-1].view(t.shape)


def _out(shape, dtype):
    """An output of `shape` ([..., C]) filled with NaN, as a view of a buffer with one more row: (buffer, view)."""
    C = shape[-1]
    n = 1
    for d in shape[:-1]:
        n *= d
    buf = torch.full((n + 1, C), NAN, dtype=dtype, device=DEV)
    return buf, buf[:-1].view(shape)


def _kept(*bufs):
    """Finite up to the guard row, the guard row still NaN."""
    return all(bool(torch.isfinite(b[:-1].float()).all()) and bool(torch.isnan(b[-1:].float()).all()) for b in bufs)


def _inputs(B, S, H, dh, family, seed=None):
    qkv, dout = R.inputs(B, S, H, dh, _lib.operand_dtype(), family, DEV, seed)
    return _guarded(qkv), _guarded(dout)


def _lengths(tiles):
    return (2, 13, 16) if tiles == 1 else (16 * tiles - 15, 16 * tiles - 3, 16 * tiles)          # one row in the last tile, a ragged tile, a full one


def _assert_rows(label, got, qkv, dout, B, S, H, dh, qscale, delta_from, store16=True, images=None, thirds=R.THIRDS):
    """The row condition of `got` [B, S, 3 D] against fp64, level from the kernel's restatement; `images`: a slice of the batch to check."""
    if images is not None:
        got, qkv, dout = got[images], qkv[images], dout[images]
        B = got.shape[0]
    ref = R.fp64(qkv, dout, B, S, H, dh, qscale)[2]
    e_k = R.row_errors(got.float(), ref, B, S, H, dh)
    e_r = R.row_errors(R.restated(qkv, dout, B, S, H, dh, qscale, delta_from, store16=store16), ref, B, S, H, dh)
    bad = R.row_condition(label, {n: e_k[n] for n in thirds}, e_r)
    assert not bad, bad
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the two-pass kernels: pv_attn_bwd2_kernel (1 .. 13 tiles) and pv_attn_bwd_kernel (dh 32, 14 .. 26 tiles)
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_pass(B, S, H, dh, family="gaussian"):
    """Two launches with the bias sums and one without, the common checks; (qkv, dout, dqkv) for the row condition."""
    D, qscale, dt = H * dh, dh ** -0.5, _lib.operand_dtype()
    qkv, dout = _inputs(B, S, H, dh, family)
    runs = []
    for with_bias in (True, True, False):
        g_buf, g = _out((B, S, 3 * D), dt)
        b_buf, dbp = _out((B, 3 * D), torch.float32)
        n0 = ops.launch_count
        ops.attention_bwd(qkv, dout, g, B, S, H, dh, qscale, dbias_partial=dbp if with_bias else None)
        assert ops.launch_count == n0 + 1
        runs.append((g_buf, g, b_buf, dbp))
    torch.cuda.synchronize()
    (g_buf, g, b_buf, dbp), second, nobias = runs
    assert _kept(g_buf, b_buf), (S, dh)
    assert torch.equal(g, second[1]) and torch.equal(dbp, second[3])                # two launches: identical bits
    assert torch.equal(g, nobias[1]) and bool(torch.isnan(nobias[2]).all())          # without the bias sums: the same dqkv, nothing else stored
    assert rel_l2(dbp, g.double().sum(1)) < 2e-6                                     # per-image column sums of exactly the stored values
    return qkv, dout, g


TWO_PASS = [(dh, t) for dh in (48, 64) for t in range(1, 14)] + [(32, t) for t in range(1, 27)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh,tiles", TWO_PASS, ids=[f"dh{dh}-{t}tiles" for dh, t in TWO_PASS])
def test_two_pass_backward_rows_every_instantiation(dh, tiles, mode):
    B, H = 3, 2
    with engine.precision(mode):
        for S in _lengths(tiles):
            qkv, dout, g = _two_pass(B, S, H, dh)
            _assert_rows(f"two-pass gaussian dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, "pdp")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh", [32, 48, 64])
def test_two_pass_backward_of_a_single_token(dh, mode):
    """S = 1: p = 1, dV = dO within the row condition, and dS = p (dP - delta) = 0 up to the rounding of delta: |dq_r|, |dk_r| <= 2^-8 |dout_r| |v| max(|k|, |q|)
    (2^-8 covers a delta formed from a 16-bit output; this kernel's fp32 delta leaves exact zeros)."""
    B, S, H = 3, 1, 2
    D = H * dh
    with engine.precision(mode):
        qkv, dout, g = _two_pass(B, S, H, dh)
        _assert_rows(f"two-pass gaussian dh {dh} S 1 {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, "pdp", thirds="v")
    q, k, v = (R.heads(t, B, S, H, dh).double().norm(dim=-1) for t in qkv.split(D, dim=-1))
    bound = 2.0 ** -8 * R.heads(dout, B, S, H, dh).double().norm(dim=-1) * v * torch.maximum(k, q)
    dq, dk, _ = (R.heads(t, B, S, H, dh).double().norm(dim=-1) for t in g.split(D, dim=-1))
    print(f"two-pass S 1 dh {dh} {mode}: max |dq_r| {float(dq.max()):.3g}, max |dk_r| {float(dk.max()):.3g}, smallest bound {float(bound.min()):.3g}")
    assert bool((dq <= bound).all()) and bool((dk <= bound).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh,S", [(64, 209), (48, 209), (32, 417)])
def test_two_pass_backward_refuses_a_length_past_its_range(dh, S, mode):
    B, H = 3, 2
    D = H * dh
    with engine.precision(mode):
        qkv, dout = _inputs(B, S, H, dh, "gaussian")
        g_buf, g = _out((B, S, 3 * D), _lib.operand_dtype())
        b_buf, dbp = _out((B, 3 * D), torch.float32)
        with pytest.raises(_lib.PeekvitHipError):
            ops.attention_bwd(qkv, dout, g, B, S, H, dh, dh ** -0.5, dbias_partial=dbp)
        torch.cuda.synchronize()
    assert bool(torch.isnan(g_buf.float()).all()) and bool(torch.isnan(b_buf).all())            # nothing was stored


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the persistent kernel: pv_attn_bwd5_kernel from the forward's output and row statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def _persistent(B, S, H, dh, family="gaussian"):
    D, qscale, dt = H * dh, dh ** -0.5, _lib.operand_dtype()
    assert ops.attention_bwd_lse_supported(S, dh)
    qkv, dout = _inputs(B, S, H, dh, family)
    a_buf, att = _out((B, S, D), dt)
    l_buf, lse = _out((B * H, S), torch.float32)
    ops.attention(qkv, att, B, S, H, dh, lse=lse.view(B, H, S))                        # the forward with its statistics comes first
    runs = []
    for with_bias in (True, True, False):
        g_buf, g = _out((B, S, 3 * D), dt)
        b_buf, dbp = _out((B, 3 * D), torch.float32)
        n0 = ops.launch_count
        ops.attention_bwd_lse(qkv, dout, att, lse.view(B, H, S), g, B, S, H, dh, qscale, dbias_partial=dbp if with_bias else None)
        assert ops.launch_count == n0 + 1
        runs.append((g_buf, g, b_buf, dbp))
    torch.cuda.synchronize()
    (g_buf, g, b_buf, dbp), second, nobias = runs
    assert _kept(a_buf, l_buf, g_buf, b_buf), (S, dh)
    assert torch.equal(g, second[1]) and torch.equal(dbp, second[3])
    assert torch.equal(g, nobias[1]) and bool(torch.isnan(nobias[2]).all())
    # the bias thirds in closed form: column sums of exactly the stored dQ; sum_k dS[q, k] = D - D = 0; sum_k P[q, k] = 1, i.e. the column sums of dout
    assert rel_l2(dbp[:, :D], g[..., :D].double().sum(1)) < 2e-6
    assert float(dbp[:, D:2 * D].abs().max()) == 0.0
    assert rel_l2(dbp[:, 2 * D:], dout.double().sum(1)) < 2e-6
    return qkv, dout, g


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh", [48, 64])
@pytest.mark.parametrize("tiles", [9, 10, 11, 12, 13])
def test_persistent_backward_rows_every_instantiation(tiles, dh, mode):
    with engine.precision(mode):
        for S in _lengths(tiles):
            qkv, dout, g = _persistent(3, S, 2, dh)
            _assert_rows(f"persistent gaussian dh {dh} S {S} {mode}", g, qkv, dout, 3, S, 2, dh, dh ** -0.5, "out")
        # 300 items on 256 CUs: a workgroup walks several; the first and the last four images = the items of a workgroup's first and later trips
        B, S, H = 100, 16 * tiles - 3, 3
        qkv, dout, g = _persistent(B, S, H, dh)
        for images in (slice(0, 4), slice(B - 4, B)):
            _assert_rows(f"persistent gaussian dh {dh} S {S} B 100 images {images.start}.. {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, "out", images=images)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the class-row backward: pv_attn_rows_bwd_kernel, one wave per (image, head), 64 / CPL keys per step
# ---------------------------------------------------------------------------------------------------------------------------------
KEYS_PER_STEP = {32: 16, 48: 8, 64: 8, 96: 4, 128: 4}          # KPI = 64 / CPL, CPL = 4 / 8 / 16 lanes per key for dh / 8 <= 4 / 8 / 16 chunks


def _class_row(B, S, H, dh, label, peaked=False):
    """Forward, two backward launches into guarded buffers (dkv a view of a wider one), the common checks and the row condition: dq per (image, head),
    dk and dv per key row.  S = 1: dq and dk are 0 up to the rounding of delta, bounded as in test_two_pass_backward_of_a_single_token."""
    D, qscale, dt = H * dh, dh ** -0.5, _lib.operand_dtype()
    q, kv, dout = (_guarded(t) for t in R.rows_inputs(B, S, H, dh, dt, peaked, DEV))
    o_buf, out = _out((B, D), dt)
    ops.attention_rows(q, kv, out, B, S, 1, H, dh)
    runs = []
    for _ in range(2):
        q_buf, dq = _out((B, D), dt)
        wide = torch.full((B * S + 1, 2 * D + 8), NAN, dtype=dt, device=DEV)              # row stride wider than 2 D
        n0 = ops.launch_count
        ops.attention_rows_bwd(q, kv, out, dout, dq, wide[:B * S, :2 * D], B, S, H, dh, qscale)
        assert ops.launch_count == n0 + 1
        runs.append((q_buf, dq, wide))
    torch.cuda.synchronize()
    (q_buf, dq, wide), second = runs
    dkv = wide[:B * S, :2 * D]
    assert _kept(o_buf, q_buf) and bool(torch.isfinite(dkv.float()).all())
    assert bool(torch.isnan(wide[B * S:].float()).all()) and bool(torch.isnan(wide[:, 2 * D:].float()).all())          # the guard row and the pad columns
    assert torch.equal(dq, second[1]) and torch.equal(dkv, second[2][:B * S, :2 * D])
    _, rq, rk, rv = R.fp64_rows(q, kv, dout, B, S, H, dh, qscale)

    def errors(gq, gk, gv):
        per_key = lambda t: t.float().reshape(B, S, H, dh).transpose(1, 2)
        return {"q": R.row_err(gq.float().view(B, H, 1, dh), rq.view(B, H, 1, dh)), "k": R.row_err(per_key(gk), per_key(rk)),
                "v": R.row_err(per_key(gv), per_key(rv))}

    e_k = errors(dq, dkv[:, :D], dkv[:, D:])
    e_r = {d: errors(*R.restated_rows(q, kv, dout, B, S, H, dh, qscale, d)) for d in ("out", "pdp")}
    thirds = "v" if S == 1 else R.THIRDS
    bad = R.row_condition(label, {n: e_k[n] for n in thirds}, e_r["out"], what="(image, head, key)")
    assert not bad, bad
    if S == 1:
        norm = lambda t: t.double().reshape(B, H, dh).norm(dim=-1)
        bound = 2.0 ** -8 * norm(dout) * norm(kv[:, D:]) * torch.maximum(norm(kv[:, :D]), norm(q))
        print(f"{label}: max |dq_r| {float(norm(dq).max()):.3g}, max |dk_r| {float(norm(dkv[:, :D]).max()):.3g}, smallest bound {float(bound.min()):.3g}")
        assert bool((norm(dq) <= bound).all()) and bool((norm(dkv[:, :D]) <= bound).all())
    return e_k, e_r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh", [32, 48, 64, 96, 128])
def test_class_row_backward_rows(dh, mode):
    step = KEYS_PER_STEP[dh]
    with engine.precision(mode):
        for S in sorted({1, 2, step - 1, step, step + 1, 257}):
            _class_row(3, S, 2, dh, f"class-row gaussian dh {dh} S {S} {mode}")


# ---------------------------------------------------------------------------------------------------------------------------------
# d. peaked rows: every fifth query row puts its probability on one key
# ---------------------------------------------------------------------------------------------------------------------------------
def _peaked_report(label, got, qkv, dout, B, S, H, dh, qscale, store16):
    """The kernel's worst dq and dk row against fp64 next to both ways to form delta (DESIGN.md section 24's table)."""
    ref = R.fp64(qkv, dout, B, S, H, dh, qscale)[2]
    e_k = R.row_errors(got.float(), ref, B, S, H, dh)
    line = f"PEAKED {label}: kernel dq {R.worst(e_k['q'])[0]:.3g} dk {R.worst(e_k['k'])[0]:.3g}"
    for d in ("pdp", "out"):
        e = R.row_errors(R.restated(qkv, dout, B, S, H, dh, qscale, d, store16=store16), ref, B, S, H, dh)
        line += f"; restated delta from {d} dq {R.worst(e['q'])[0]:.3g} dk {R.worst(e['k'])[0]:.3g}"
    print(line)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", [(33, 48), (197, 64), (401, 32)])
def test_two_pass_backward_on_peaked_rows(S, dh, mode):
    B, H = 3, 2
    with engine.precision(mode):
        qkv, dout, g = _two_pass(B, S, H, dh, "peaked")
        _peaked_report(f"two-pass dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, True)
        _assert_rows(f"two-pass peaked dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, "pdp")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", [(197, 64), (205, 48)])
def test_persistent_backward_on_peaked_rows(S, dh, mode):
    B, H = 3, 2
    with engine.precision(mode):
        qkv, dout, g = _persistent(B, S, H, dh, "peaked")
        _peaked_report(f"persistent dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, True)
        _assert_rows(f"persistent peaked dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, dh ** -0.5, "out")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", [(130, 64), (449, 64)])
def test_streaming_backward_on_peaked_rows(S, dh, mode):
    B, H = 3, 2
    D, qscale = H * dh, dh ** -0.5
    with engine.precision(mode):
        dt = _lib.operand_dtype()
        qkv, dout = _inputs(B, S, H, dh, "peaked")
        a_buf, att = _out((B, S, D), dt)
        l_buf, lse = _out((B * H, S), torch.float32)
        ops.attention_stream(qkv, att, lse.view(B, H, S), B, S, H, dh)
        runs = []
        for _ in range(2):
            g_buf, g = _out((B, S, 3 * D), torch.float32)
            d_buf, delta = _out((B * H, S), torch.float32)
            ops.attention_stream_bwd(qkv, dout, att, lse.view(B, H, S), g, B, S, H, dh, qscale, delta_ws=delta.view(B, H, S))
            runs.append((g_buf, g, d_buf))
        torch.cuda.synchronize()
        (g_buf, g, d_buf), second = runs
        assert _kept(a_buf, l_buf, g_buf, d_buf)
        assert torch.equal(g, second[1]) and torch.equal(d_buf[:-1], second[2][:-1])
        _peaked_report(f"streaming dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, qscale, False)
        _assert_rows(f"streaming peaked dh {dh} S {S} {mode}", g, qkv, dout, B, S, H, dh, qscale, "out", store16=False)


@pytest.mark.parametrize("mode", MODES)
def test_class_row_backward_on_a_peaked_row(mode):
    with engine.precision(mode):
        e_k, e_r = _class_row(3, 197, 2, 64, f"class-row peaked dh 64 S 197 {mode}", peaked=True)
    print(f"PEAKED class-row dh 64 S 197 {mode}: kernel dq {R.worst(e_k['q'])[0]:.3g} dk {R.worst(e_k['k'])[0]:.3g}; "
          + "; ".join(f"restated delta from {d} dq {R.worst(e_r[d]['q'])[0]:.3g} dk {R.worst(e_r[d]['k'])[0]:.3g}" for d in ("pdp", "out")))
