"""The attention-forward references (tests/attn_backward_ref.py) without a GPU: two legitimate restatements of the forward agree on the per-row level,
five planted faults break the row condition of tests/test_hip_attention_forward_rows.py by at least 5 x, the first three of them pass the whole-tensor
caps every older forward test asserts, and an lse that is 1e-3 off in one row breaks the lse condition.

The faults are planted into `restated_forward` itself (block = 64 past S = 416, where the streaming kernel runs):
  (i) one row of one head 10 % wrong, (ii) one row zeroed, (iii) two rows exchanged between heads - on Gaussian inputs;
  (iv) key S - 1 left out of one row's softmax, (v) key S - 1 counted twice in one row - on the "edge" family, in the row of (image 1, head 1) whose
  probability on that key the change moves most: a masking slip at the ragged edge hits every row, so a kernel's worst row moves at least as far.
factor = max_r e(faulty) / (2 max_r e(restated) + 1e-5): 1 is the row condition's edge."""
import math

import pytest
import torch

import attn_backward_ref as R
from conftest import rel_l2

MODES = ["bf16", "f16"]
SHAPES = [(197, 64), (401, 32), (449, 64)]
B, H = 3, 2
WHOLE_CAP_BF16 = 6e-3          # test_attention's and the row-maximum test's bound for bf16 against fp64 (tests/test_hip_ops.py)


def _block(S):
    return 64 if S > 416 else None          # the kernel that runs at that length: streaming past 416


def _first_of_last(S):
    tile = 64 if S > 416 else 16
    return tile * ((S + tile - 1) // tile - 1)


_CASES = {}


def _case(S, dh, mode, family):
    """(qkv, restated out, fp64 out, restated lse, fp64 lse) of a shape, computed once."""
    key = (S, dh, mode, family)
    if key not in _CASES:
        qkv, _ = R.inputs(B, S, H, dh, R.DTYPE[mode], family, first_of_last=_first_of_last(S))
        out, lse = R.restated_forward(qkv, B, S, H, dh, block=_block(S))
        ref, lse64 = R.fp64_forward(qkv, B, S, H, dh)
        _CASES[key] = (qkv, out, ref, lse, lse64)
    return _CASES[key]


def _factor(label, faulty, restated, ref, S, dh, Bn=B, Hn=H):
    e_r = R.forward_row_errors(restated, ref, Bn, S, Hn, dh)
    e_f = R.forward_row_errors(faulty, ref, Bn, S, Hn, dh)
    bad = R.row_condition(label, e_f, e_r, prefix="")
    factor = R.worst(e_f["out"])[0] / (2.0 * R.worst(e_r["out"])[0] + 1e-5)
    print(f"{label}: FACTOR {factor:.3g}, worst row at (image, head, row) {R.worst(e_f['out'])[1]}")
    return factor, bad


# ---- the faults: (out [B, S, D], qkv, S, dh) -> the faulty out, and where the worst row must be found ----
def _scaled_row(out, qkv, S, dh):
    out = out.clone()
    out[1, S // 2, 1 * dh:2 * dh] *= 1.1
    return out, (1, 1, S // 2)


def _zeroed_row(out, qkv, S, dh):
    out = out.clone()
    out[2, S - 1, 0:dh] = 0.0                             # the last row of the ragged tile
    return out, (2, 0, S - 1)


def _swapped_heads(out, qkv, S, dh):
    out = out.clone()
    row = out[0, 64, 0:dh].clone()
    out[0, 64, 0:dh] = out[0, 64, dh:2 * dh]
    out[0, 64, dh:2 * dh] = row
    return out, (0, None, 64)


def _tail_key(out, qkv, S, dh, change, moved):
    """One row of (image 1, head 1) recomputed with key S - 1's score changed: the row the change moves most, `moved`(p) of its probability p on that key."""
    D = H * dh
    q, k, v = (R.heads(t, B, S, H, dh) for t in qkv.float().split(D, dim=-1))
    s = q @ k.transpose(-1, -2)
    r = int(moved(torch.softmax(s[1, 1].double(), -1)[:, S - 1]).argmax())
    s[1, 1, r, S - 1] = change(s[1, 1, r, S - 1])
    o, _ = R.attend_restated(s, v, qkv.dtype, block=_block(S))
    faulty = out.clone()
    faulty[1, r, dh:2 * dh] = R.rows(o, B, S, H, dh).to(qkv.dtype).float()[1, r, dh:2 * dh]
    return faulty, (1, 1, r)


def _tail_key_left_out(out, qkv, S, dh):
    return _tail_key(out, qkv, S, dh, lambda s: s * 0.0 - math.inf, lambda p: p)                          # the row loses p of its mass


def _tail_key_twice(out, qkv, S, dh):
    return _tail_key(out, qkv, S, dh, lambda s: s + math.log(2.0), lambda p: p * (1 - p) / (1 + p))     # p -> 2 p / (1 + p)


FAULTS = [(_scaled_row, "gaussian"), (_zeroed_row, "gaussian"), (_swapped_heads, "gaussian"), (_tail_key_left_out, "edge"), (_tail_key_twice, "edge")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", SHAPES)
@pytest.mark.parametrize("family", ["gaussian", "peaked", "spread"])
def test_two_restatements_of_the_forward_agree_on_the_row_level(family, S, dh, mode):
    """(a) p rounded unnormalised (the kernels) against softmax(s) rounded: the row condition holds between the two, either way round."""
    qkv, out, ref, lse, lse64 = _case(S, dh, mode, family)
    other, lse_other = R.restated_forward(qkv, B, S, H, dh, normalised=True)
    e_a, e_b = R.forward_row_errors(out, ref, B, S, H, dh), R.forward_row_errors(other, ref, B, S, H, dh)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert not R.row_condition(f"unnormalised p against normalised P, {family} S {S} dh {dh} {mode}", e_a, e_b, prefix="")
    assert not R.row_condition(f"normalised P against unnormalised p, {family} S {S} dh {dh} {mode}", e_b, e_a, prefix="")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", SHAPES)
@pytest.mark.parametrize("fault,family", FAULTS, ids=[f.__name__.strip("_") for f, _ in FAULTS])
def test_planted_fault_breaks_the_row_condition_five_times_over(fault, family, S, dh, mode):
    """(b)"""
    qkv, out, ref, _, _ = _case(S, dh, mode, family)
    faulty, (b_, h_, r_) = fault(out, qkv, S, dh)
    factor, bad = _factor(f"{fault.__name__} {family} S {S} dh {dh} {mode}", faulty, out, ref, S, dh)
    assert bad and factor >= 5.0, factor
    at = bad[0][2]
    assert at[0] == b_ and at[2] == r_ and h_ in (None, at[1]), (at, (b_, h_, r_))              # the condition names the image, the head and the row


_BIG = {}


def _big():
    """A ViT-B sized batch, a few images at a time: (restated out, fp64 out) [96, 197, 768] in bf16."""
    if not _BIG:
        Bn, S, Hn, dh, chunk = 96, 197, 12, 64, 8
        qkv, _ = R.inputs(Bn, S, Hn, dh, torch.bfloat16)
        got, ref = [], []
        for b0 in range(0, Bn, chunk):
            got.append(R.restated_forward(qkv[b0:b0 + chunk], chunk, S, Hn, dh)[0])
            ref.append(R.fp64_forward(qkv[b0:b0 + chunk], chunk, S, Hn, dh)[0])
        _BIG["v"] = (qkv, torch.cat(got), torch.cat(ref))
    return _BIG["v"]


@pytest.mark.parametrize("fault", [_scaled_row, _zeroed_row, _swapped_heads], ids=lambda f: f.__name__.strip("_"))
def test_planted_faults_pass_the_whole_tensor_cap_at_197_64_bf16(fault):
    """(c) the reason this file exists.  A fault of relative size f in ONE of N = B H S rows moves the whole-tensor figure to sqrt(base^2 + f^2 / N).  At
    B = 3, H = 2 (N = 1182) that lets the 10 % row through (3.7e-3) and, by this arithmetic, cannot let a zeroed row (f = 1: 2.9e-2) or two exchanged rows
    (f^2 = 4: 5.8e-2) through; the older tests' cap applies to any batch, so the three are planted into a batch of 96 x 12 heads, N = 226944:
    sqrt(base^2 + 4 / N) = 4.7e-3 at the restatement's base of 2.2e-3.  The row condition fails on the same tensors by the factors of (b)."""
    S, dh = 197, 64
    if fault is _scaled_row:
        qkv, out, ref, _, _ = _case(S, dh, "bf16", "gaussian")
        faulty, _ = fault(out, qkv, S, dh)
        print(f"{fault.__name__} B 3 H 2: whole tensor {rel_l2(out, ref):.3g} -> {rel_l2(faulty, ref):.3g} (cap {WHOLE_CAP_BF16})")
        assert rel_l2(faulty, ref) < WHOLE_CAP_BF16
        assert _factor(f"{fault.__name__} B 3 H 2", faulty, out, ref, S, dh)[0] >= 5.0
    qkv, out, ref = _big()
    faulty, _ = fault(out, qkv, S, dh)
    whole0, whole = rel_l2(out, ref), rel_l2(faulty, ref)
    print(f"{fault.__name__} B 96 H 12: whole tensor {whole0:.3g} -> {whole:.3g} (cap {WHOLE_CAP_BF16})")
    assert whole < WHOLE_CAP_BF16
    factor, bad = _factor(f"{fault.__name__} B 96 H 12", faulty, out, ref, S, dh, 96, 12)
    assert bad and factor >= 5.0, factor


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,dh", SHAPES)
def test_an_lse_that_is_off_in_one_row_breaks_the_lse_condition(S, dh, mode):
    """(d)"""
    for family in ("gaussian", "spread"):
        _, _, _, lse, lse64 = _case(S, dh, mode, family)
        label = f"{family} S {S} dh {dh} {mode}"
        assert not R.lse_condition(label, lse, lse, lse64)
        faulty = lse.clone()
        faulty[1, 1, S // 2] += 1e-3
        assert R.lse_condition(label + ", one row + 1e-3", faulty, lse, lse64)
        if family == "gaussian":
            assert float((lse.double() - lse64).abs().max()) < 1e-4                             # the project's absolute bound holds for the restatement
