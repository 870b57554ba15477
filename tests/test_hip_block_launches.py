"""The launch sequence of every variant of the training encoder block (peekvit_amd/train_engine.py: EncoderBlockFn behind block_forward_train,
masked_block_forward_train, avit_block_forward_train, avit_packed_block_forward_train and the packed ResidualViT pass), pinned: one forward and one
backward of each under ops.KernelTimer, the recorded (kernel name, member) lists against the literal lists below.

ORIGIN OF THE LISTS: they were recorded by running this file's `run_case` at the commit BEFORE the five block functions (BlockFn, MaskedBlockFn,
AViTBlockFn, PackedMaskedBlockFn, PackedAViTBlockFn) were folded into one forward and one backward body, not from the folded code: they say what
the five copies launched.  A GEMM's member is (N, K, epilogue); `_sym` writes the widths as letters (D, M = 2 D the MLP width, T = 3 D), and in
that spelling both shapes recorded the same lists: at 2 x 17 and 2 x 197 rows every weight gradient takes the transposed-copy path (two
transpositions, the split-K GEMM over the rows padded to 1024, the slice sum), and KernelTimer's name does not tell the persistent attention
backward (S = 197: the forward kept its row statistics) from the two-pass one (S = 17), nor the masked LayerNorm backward from the plain one.
The pv_cast_f32_bf16 / lone pv_transpose_bf16 launches are the 16-bit weight copies (engine.bf16_weight / train_engine.bf16_weight_t), made at
first use: the block is fresh in every case."""
import math

import pytest
import torch

import test_hip_avit_train as dense_t

pytestmark = pytest.mark.gpu

SHAPES = [(2, 17, 128, 2), (2, 197, 192, 3)]
VARIANTS = ["block", "masked", "avit", "packed_masked", "packed_avit"]


def _sym(records, D):
    """[(name, member)] of a KernelTimer's records, GEMM members (N, K, epilogue) with the widths as letters; any other width stays a number."""
    letters = {D: "D", 2 * D: "M", 3 * D: "T"}
    out = []
    for name, _e0, _e1, _flops, _bytes, member in records:
        if member is not None:
            member = tuple(letters.get(v, v) for v in member[:2]) + tuple(member[2:])
        out.append((name, member))
    return out


def _pack(x, dout, m):
    """The packed rows of a 0/1 mask, as tests/test_hip_avit_packed_train.py builds them: every image's live rows, then one representative row (zero
    input, row scale 0, key weight ln n) for its n dead ones.  (rows, their gradient, row scale, log_mult, seg, longest segment)"""
    B, S, D = x.shape
    rows, drows, rs, lm, seg = [], [], [], [], [0]
    for b in range(B):
        live = [t for t in range(S) if m[b, t] == 1]
        rows += [x[b, t] for t in live]
        drows += [dout[b, t] for t in live]
        rs += [1.0] * len(live)
        lm += [0.0] * len(live)
        n = S - len(live)
        if n:
            rows.append(torch.zeros(D)); drows.append(dout[b, [t for t in range(S) if m[b, t] == 0][0]]); rs.append(0.0); lm.append(math.log(n))
        seg.append(len(rows))
    return torch.stack(rows), torch.stack(drows), torch.tensor(rs), torch.tensor(lm), torch.tensor(seg, dtype=torch.int32), \
        max(seg[i + 1] - seg[i] for i in range(B))


def run_case(variant, B, S, D, H, frozen=()):
    """One forward and one backward of `variant` on its own (bf16 operands, no pass): (forward launches, backward launches, out, dx, the row scale's gradient
    or None, the block)."""
    from peekvit_amd import ops, train_engine as te
    dev = dense_t._dev()
    blk = dense_t._micro_block(D, H, dev, seed=S).to(dev)
    for n, p in blk.named_parameters():
        if n.endswith(tuple(frozen)):
            p.requires_grad_(False)
    g = torch.Generator().manual_seed(S + D)
    m = (torch.rand(B, S, generator=g) < 0.6).float()          # about 60 % live rows, the class row live, at least one dead row per image
    m[:, 0], m[:, S - 1] = 1, 0
    x = (torch.randn(B, S, D, generator=g) * m[:, :, None]).to(torch.bfloat16).float()
    dout = torch.randn(B, S, D, generator=g)
    if variant.startswith("packed"):
        xp, dout, rs, lm, seg, max_len = _pack(x, dout, m)
        xg, rs, lm, seg = xp.to(dev).requires_grad_(True), rs.to(dev).requires_grad_(True), lm.to(dev), seg.to(dev)
        md = rs
        if variant == "packed_masked":           # the pack step hands over h1 = row scale * LN1(x): made here, outside the timer
            h1 = ops.layernorm_bf16(xg.detach(), blk.ln_1.weight.detach(), blk.ln_1.bias.detach(), blk.ln_1.eps,
                                    torch.empty(xp.shape, dtype=torch.bfloat16, device=dev), rs.detach())
            run = lambda: te.EncoderBlockFn.apply(blk, xg, rs, True, h1, (seg, lm, max_len), *te.block_params(blk))
        else:
            run = lambda: te.avit_packed_block_forward_train(blk, xg, rs, seg, lm, max_len)
    else:
        xg, md = x.to(dev).requires_grad_(True), m.to(dev).requires_grad_(True)
        run = {"block": lambda: te.block_forward_train(blk, xg), "masked": lambda: te.masked_block_forward_train(blk, xg, md),
               "avit": lambda: te.avit_block_forward_train(blk, xg, md)}[variant]
    dout = dout.to(dev)
    torch.cuda.synchronize()
    n0 = ops.launch_count
    with ops.KernelTimer() as kt:
        out = run()
        n_fw = len(kt.records)
        out.backward(dout)
        torch.cuda.synchronize()
    assert ops.launch_count - n0 == len(kt.records) > n_fw > 0, "the HIP block did not run"
    rec = _sym(kt.records, D)
    return rec[:n_fw], rec[n_fw:], out, xg.grad, md.grad, blk


# ---- what the five copies launched (see the module docstring) -------------------------------------------------------------------------------------
LN, CAST, TR, SUM, COLSUM = ("pv_layernorm_bf16", None), ("pv_cast_f32_bf16", None), ("pv_transpose_bf16", None), ("pv_sum_slices_f32", None), ("pv_colsum_f32", None)
MRES, LNB = ("pv_masked_residual", None), ("pv_layernorm_bwd", None)
ATT, ATT_B = ("pv_attention_bf16", None), ("pv_attention_bwd_bf16", None)
RAG, RAG_B = ("pv_attention_varlen_w_lse_bf16", None), ("pv_attention_varlen_w_bwd16_bf16", None)
IN, OUT_RES, OUT_16, FC1, FC2 = [("pv_gemm_bf16", mb) for mb in (("T", "D", 0), ("D", "D", 2), ("D", "D", 0), ("M", "D", 6), ("D", "M", 2))]
W_M, W_D = [("pv_gemm_bf16[wgrad]", mb) for mb in (("M", 1024, 4), ("D", 1024, 4))]
D_FC2, D_FC1, D_OUT, D_IN = [("pv_gemm_bf16[dgrad]", mb) for mb in (("M", "D", 7), ("D", "M", 0), ("D", "D", 0), ("D", "T", 0))]

FW_PLAIN = [LN, CAST, IN, ATT, CAST, OUT_RES, LN, CAST, FC1, CAST, FC2]                    # BlockFn, AViTBlockFn
FW_MASKED = [LN, CAST, IN, ATT, CAST, OUT_16, MRES, LN, CAST, FC1, CAST, FC2]              # MaskedBlockFn
FW_PACKED_AVIT = [LN, CAST, IN, RAG, CAST, OUT_RES, LN, CAST, FC1, CAST, FC2]              # PackedAViTBlockFn
FW_PACKED_MASKED = [CAST, IN, RAG, CAST, OUT_16, MRES, LN, CAST, FC1, CAST, FC2]           # PackedMaskedBlockFn (h1 is handed in)
BW_RESIDENT = [CAST, TR, TR, W_M, SUM, TR, D_FC2, COLSUM, TR, TR, W_D, SUM, TR, D_FC1, LNB,
               TR, TR, W_D, SUM, TR, D_OUT, ATT_B, COLSUM, TR, TR, W_D, SUM, TR, D_IN, LNB]
BW_RAGGED = [CAST, TR, TR, W_M, SUM, TR, D_FC2, COLSUM, TR, TR, W_D, SUM, TR, D_FC1, LNB,
             TR, TR, W_D, SUM, TR, D_OUT, RAG_B, COLSUM, TR, TR, W_D, SUM, TR, D_IN, LNB]
BW_FROZEN = [CAST, TR, TR, W_M, SUM, TR, D_FC2, COLSUM, TR, D_FC1, LNB,
             TR, TR, W_D, SUM, TR, D_OUT, ATT_B, COLSUM, TR, D_IN, LNB]                    # BlockFn without the fc1 and in-projection weight gradients
EXPECTED = {"block": (FW_PLAIN, BW_RESIDENT), "masked": (FW_MASKED, BW_RESIDENT), "avit": (FW_PLAIN, BW_RESIDENT),
            "packed_masked": (FW_PACKED_MASKED, BW_RAGGED), "packed_avit": (FW_PACKED_AVIT, BW_RAGGED)}


def _check(variant, fw, bw, out, dx, dm, blk, want, frozen=()):
    assert fw == want[0], fw
    assert bw == want[1], bw
    assert torch.isfinite(out).all() and dx is not None and dx.shape == out.shape and torch.isfinite(dx).all()
    if "masked" in variant:          # ResidualViT's row scale carries the gate's graph; A-ViT's comes from comparisons
        assert dm is not None and torch.isfinite(dm).all()
    else:
        assert dm is None
    params = list(blk.named_parameters())
    assert len(params) == 12
    for n, p in params:
        if frozen and n.endswith(frozen):
            assert p.grad is None, n
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("B,S,D,H", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_variant_launches_what_its_own_copy_launched(variant, B, S, D, H):
    fw, bw, out, dx, dm, blk = run_case(variant, B, S, D, H)
    _check(variant, fw, bw, out, dx, dm, blk, EXPECTED[variant])


FROZEN = ("in_proj_weight", "fc1.weight")


@pytest.mark.parametrize("B,S,D,H", SHAPES)
def test_frozen_parameters_skip_their_weight_gradient_launches(B, S, D, H):
    """The `need` path: with the in-projection and fc1 weights frozen their weight-gradient launches are gone and nothing else moves."""
    fw, bw, out, dx, dm, blk = run_case("block", B, S, D, H, frozen=FROZEN)
    _check("block", fw, bw, out, dx, dm, blk, (FW_PLAIN, BW_FROZEN), frozen=FROZEN)
