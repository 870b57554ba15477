"""The attention-backward references (tests/attn_backward_ref.py) without a GPU: the restatements stay under the project's whole-tensor caps, the
per-row condition of tests/test_hip_attention_backward_rows.py fails on planted faults that the whole-tensor caps let through, and on peaked rows
the two ways to form delta differ by far more per row than the whole-tensor figure shows."""
import pytest
import torch

import attn_backward_ref as R
from conftest import rel_l2

MODES = ["bf16", "f16"]
LENGTHS = [2, 13, 16, 17, 97, 197, 208, 401, 416]


def _dh(S):
    return 64 if S <= 208 else 32          # the widest head the resident kernels take at that length


def _whole(got, ref, D):
    return [rel_l2(got[..., i * D:(i + 1) * D], ref[..., i * D:(i + 1) * D]) for i in range(3)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", LENGTHS)
def test_restatements_stay_under_the_whole_tensor_caps(S, mode):
    B, H, dh = 3, 2, _dh(S)
    qscale = dh ** -0.5
    qkv, dout = R.inputs(B, S, H, dh, R.DTYPE[mode])
    _, _, ref = R.fp64(qkv, dout, B, S, H, dh, qscale)
    for delta_from in ("pdp", "out"):
        for store16 in (True, False):
            got = R.restated(qkv, dout, B, S, H, dh, qscale, delta_from, store16=store16)
            whole = _whole(got, ref, H * dh)
            rows = {n: R.worst(e)[0] for n, e in R.row_errors(got, ref, B, S, H, dh).items()}
            print(f"S {S} dh {dh} {mode} delta from {delta_from}, 16-bit result {store16}: whole tensor {['%.3g' % w for w in whole]}, worst row {rows}")
            assert torch.isfinite(got).all() and max(whole) < R.CAP[mode]


def _batched(B, S, H, dh, dt, chunk=4):
    """Restated ("pdp", 16-bit result: the two-pass kernel) and fp64 gradients of a batch large enough for one row to hide in, a few images at a time."""
    qscale = dh ** -0.5
    qkv, dout = R.inputs(B, S, H, dh, dt)
    got, ref = [], []
    for b0 in range(0, B, chunk):
        n = min(chunk, B - b0)
        got.append(R.restated(qkv[b0:b0 + n], dout[b0:b0 + n], n, S, H, dh, qscale, "pdp"))
        ref.append(R.fp64(qkv[b0:b0 + n], dout[b0:b0 + n], n, S, H, dh, qscale)[2])
    return torch.cat(got), torch.cat(ref)


_BATCH = {}


def _batch(mode):
    if mode not in _BATCH:
        _BATCH[mode] = _batched(32, 197, 12, 64, R.DTYPE[mode])
    return _BATCH[mode]


def _scaled_row(g, D, dh):
    g[1, 100, 1 * dh:2 * dh] *= 1.1                       # dq of image 1, head 1, row 100: 10 % off


def _zeroed_last_row(g, D, dh):
    g[2, 196, D + 0 * dh:D + 1 * dh] = 0.0                # dk of image 2, head 0: row 196, the last of the ragged tile 192 .. 196


def _swapped_heads(g, D, dh):
    a, b = slice(2 * D + 3 * dh, 2 * D + 4 * dh), slice(2 * D + 7 * dh, 2 * D + 8 * dh)
    row = g[5, 64, a].clone()                             # dv of image 5, row 64: heads 3 and 7 exchanged
    g[5, 64, a] = g[5, 64, b]
    g[5, 64, b] = row


# A fault of relative size f in ONE of N = B H S rows moves a third's whole-tensor figure to about sqrt(base^2 + f^2 / N).  N = 32 x 12 x 197 = 75648:
# f = 0.1 gives 3.6e-4 (under both caps), a zeroed row (f = 1) 3.6e-3 and two exchanged rows (f^2 = 4) 7.3e-3 - under bf16's 1e-2, over fp16's 1.5e-3,
# so fp16 plants the first fault only.
FAULTS = [("bf16", _scaled_row, "q"), ("bf16", _zeroed_last_row, "k"), ("bf16", _swapped_heads, "v"), ("f16", _scaled_row, "q")]


@pytest.mark.parametrize("mode,fault,third", FAULTS, ids=[f"{m}-{f.__name__.strip('_')}" for m, f, _ in FAULTS])
def test_planted_fault_fails_the_row_condition_and_passes_the_whole_tensor_cap(mode, fault, third):
    B, S, H, dh = 32, 197, 12, 64
    D = H * dh
    restated, ref = _batch(mode)
    faulty = restated.clone()
    fault(faulty, D, dh)
    e_r = R.row_errors(restated, ref, B, S, H, dh)
    assert not R.row_condition(f"unchanged {mode}", e_r, e_r)                                   # (the condition holds for the restatement itself)
    whole0, whole = _whole(restated, ref, D), _whole(faulty, ref, D)
    print(f"{fault.__name__} {mode}: whole tensor {['%.3g' % w for w in whole0]} -> {['%.3g' % w for w in whole]} (cap {R.CAP[mode]})")
    assert max(whole) < R.CAP[mode]                                                             # every whole-tensor test we have lets it through
    bad = R.row_condition(f"{fault.__name__} {mode}", R.row_errors(faulty, ref, B, S, H, dh), e_r)
    assert [b[1] for b in bad] == ["d" + third], bad                                            # the row condition names the third ...
    b_, r_ = {"q": (1, 100), "k": (2, 196), "v": (5, 64)}[third]
    assert bad[0][2][0] == b_ and bad[0][2][2] == r_, bad                                       # ... the image and the row


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", [(197, 64), (401, 32)])
def test_peaked_rows_tell_the_two_deltas_apart_where_the_whole_tensor_figure_does_not(S, dh, mode):
    """The gap the GPU file measures: with every fifth query row peaked, delta from the 16-bit output costs the dk rows at least five times the error of
    delta from the fp32 P o dP - and both restatements pass the whole-tensor caps."""
    B, H = 3, 2
    qscale = dh ** -0.5
    qkv, dout = R.inputs(B, S, H, dh, R.DTYPE[mode], family="peaked")
    _, _, ref = R.fp64(qkv, dout, B, S, H, dh, qscale)
    peak = torch.softmax(R.heads(qkv[..., :H * dh].double(), B, S, H, dh) @ R.heads(qkv[..., H * dh:2 * H * dh].double(), B, S, H, dh).transpose(-1, -2), -1)
    print(f"median peak probability of the scaled rows: {float(peak[:, :, 0::5].amax(-1).median()):.3g}, of the others {float(peak[:, :, 1::5].amax(-1).median()):.3g}")
    rows = {}
    for delta_from in ("pdp", "out"):
        got = R.restated(qkv, dout, B, S, H, dh, qscale, delta_from)
        whole = _whole(got, ref, H * dh)
        rows[delta_from] = {n: R.worst(e)[0] for n, e in R.row_errors(got, ref, B, S, H, dh).items()}
        print(f"peaked S {S} dh {dh} {mode} delta from {delta_from}: whole tensor {['%.3g' % w for w in whole]}, worst row {rows[delta_from]}")
        assert max(whole) < R.CAP[mode]
    assert rows["out"]["k"] >= 5.0 * rows["pdp"]["k"]
