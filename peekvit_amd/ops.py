"""Tensor-level wrappers over the C ABI (one function per entry point of include/peekvit_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every FLOP of the hot path is done by
libpeekvit_hip.so.  All wrappers launch on torch's CURRENT stream and never synchronise.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import GemmArgs, check

# launch counter: tests assert that the HIP path (not some silent eager path) produced the result
launch_count = 0


class KernelTimer:
    """Per-launch HIP-event timing on the stream the kernels are launched on (bench.py's `roofline` leg).
    `with KernelTimer() as kt:` brackets every C-ABI launch with two events; `kt.summary()` (after a device
    synchronise) returns {kernel: {"launches", "ms", "flops", "bytes"}} where flops/bytes are the ALGORITHMIC
    work of the launches."""

    def __init__(self):
        self.records = []     # (name, start_event, end_event, flops, bytes, member)

    def __enter__(self):
        global _timer
        _timer = self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = None

    def summary(self):
        out = {}
        for name, e0, e1, flops, nbytes, _member in self.records:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out

    def members(self, name):
        """The launches of one kernel name split by `member` (GEMMs: (N, K, epilogue) - the in-projection, out-projection, fc1, fc2 and the
        patch embedding are one C-ABI entry point but different roofline cases): {member: {"launches", "ms", "flops", "bytes"}}."""
        out = {}
        for n, e0, e1, flops, nbytes, member in self.records:
            if n != name:
                continue
            d = out.setdefault(member, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


_timer: Optional[KernelTimer] = None


class _timed:
    """Context manager used by every wrapper: no-op unless a KernelTimer is active."""
    __slots__ = ("name", "flops", "nbytes", "e0", "dev", "member")

    def __init__(self, name, dev, flops=0.0, nbytes=0.0, member=None):
        self.name, self.flops, self.nbytes, self.dev, self.member = name, flops, nbytes, dev, member

    def __enter__(self):
        if _timer is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.dev))

    def __exit__(self, *exc):
        if _timer is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(torch.cuda.current_stream(self.dev))
            _timer.records.append((self.name, self.e0, e1, self.flops, self.nbytes, self.member))


def _stream(t: torch.Tensor):
    """torch's current stream on the tensor's device.  The launch goes to the CURRENT device (kernel attributes such as the > 64 KiB
    LDS opt-in are per device), so a tensor on another device is refused loudly: the model-level entry points make the input's
    device current (`engine.on_device`)."""
    idx = t.device.index
    if idx != torch.cuda.current_device():
        raise _lib.PeekvitHipError(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}: wrap the call in "
                                   "`with torch.cuda.device(tensor.device):`")
    return C.c_void_p(raw_stream(idx))


def raw_stream(device_index: int) -> int:
    """hipStream_t of torch's current stream on that device, without building a torch.cuda.Stream object (~100 launches per forward: the eager
    small-batch path is host-bound)."""
    return torch._C._cuda_getCurrentRawStream(device_index)


# Operand-range guard (fp16-operand library, include/peekvit_hip.h `range_flag`): while `range_flag` holds a 1-element int32 GPU
# tensor the data-dependent operand producers (QKV / GELU GEMM epilogues, the fp32 patch gather) OR 1 into it when a value does
# not fit fp16.  engine.forward_auto zeroes it before and reads it after a forward.
# Per THREAD: another thread's guarded forward has its own flag word.
import threading as _threading
_tls = _threading.local()


def set_range_flag(flag: Optional[torch.Tensor]):
    _tls.range_flag = flag


def current_range_flag() -> Optional[torch.Tensor]:
    return getattr(_tls, "range_flag", None)


def _flag(dev):
    range_flag = current_range_flag()
    return C.c_void_p(range_flag.data_ptr()) if range_flag is not None and range_flag.device == dev else C.c_void_p(0)


def set_flag_word(k: int) -> int:
    """Which word of the flag tensor the ATTENTION launches of the calling thread raise their score bit in (engine.run_layers: 1 + layer index,
    so that a tripped forward knows WHICH layers to repeat in split precision); 0 = the common word.  Returns the previous value."""
    old = getattr(_tls, "flag_word", 0)
    _tls.flag_word = k
    return old


def _attn_flag(dev):
    flag = current_range_flag()
    if flag is None or flag.device != dev:
        return C.c_void_p(0)
    k = getattr(_tls, "flag_word", 0)
    return C.c_void_p(flag.data_ptr() + 4 * (k if k < flag.numel() else 0))


def workspace_bytes(use: int, *dims: int) -> int:
    """Scratch bytes of a C-ABI entry point for the given sizes: the library's own formula (pv_workspace_size, include/peekvit_hip.h PV_WS_*)."""
    arr = (C.c_int64 * len(dims))(*[int(d) for d in dims])
    n = int(_lib.load().pv_workspace_size(int(use), arr, len(dims)))
    if n < 0:
        check(n, "pv_workspace_size")
    return n


def _scratch_f32(use: int, dev, *dims: int) -> torch.Tensor:
    return torch.empty((workspace_bytes(use, *dims) // 4,), dtype=torch.float32, device=dev)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _chk(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.PeekvitHipError(f"{name}: expected a GPU tensor, got {t.device}")
    if t.dtype != dtype:
        raise _lib.PeekvitHipError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.PeekvitHipError(f"{name}: expected a contiguous tensor")
    return t


def _count():
    global launch_count
    launch_count += 1


def cast_bf16(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(src, torch.float32, "src")
    if out is None:
        out = torch.empty(src.shape, dtype=_lib.operand_dtype(), device=src.device)
    with _timed("pv_cast_f32_bf16", src.device, 0.0, 6.0 * src.numel()):
        check(_lib.load().pv_cast_f32_bf16(_ptr(src), _ptr(out), src.numel(), _stream(src)), "pv_cast_f32_bf16")
    _count()
    return out


def patch_embed(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], pos: torch.Tensor, tokens: torch.Tensor, patch: int, row_off: int) -> torch.Tensor:
    """tokens[b, row_off + i, :] = patch_i(x[b]) . w^T + bias + pos[row_off + i, :] in ONE launch (pv_patch_embed_f32: no materialised patch matrix).
    x fp32 [B,C,R,R]; w 16-bit [D, C*P*P]; pos fp32 [>= row_off + Np, D]; tokens fp32 [B, S, D]."""
    _chk(x, torch.float32, "x"); _chk(w, _lib.operand_dtype(), "w"); _chk(pos, torch.float32, "pos"); _chk(tokens, torch.float32, "tokens")
    B, Cc, H, W = x.shape
    _, S, D = tokens.shape
    if H != W or w.shape != (D, Cc * patch * patch) or pos.shape[1] != D or pos.shape[0] < row_off + (H // patch) ** 2:      # (ResidualViT's budget-token row has no positional row)
        raise _lib.PeekvitHipError(f"patch_embed: shapes x {tuple(x.shape)}, w {tuple(w.shape)}, pos {tuple(pos.shape)}, tokens {tuple(tokens.shape)}")
    M = B * (H // patch) ** 2
    with _timed("pv_gemm_bf16", x.device, 2.0 * M * D * w.shape[1], 4.0 * x.numel() + 2.0 * w.numel() + 4.0 * M * D, member=(D, w.shape[1], _lib.PV_EPI_BIAS_POS_F32)):
        check(_lib.load().pv_patch_embed_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(pos), _ptr(tokens), B, Cc, H, patch, D, S, row_off, _flag(x.device), _stream(x)),
              "pv_patch_embed_f32")
    _count()
    return tokens


def im2col(x: torch.Tensor, patch: int, out: torch.Tensor) -> torch.Tensor:
    _chk(x, torch.float32, "x")
    B, Cc, H, W = x.shape
    with _timed("pv_im2col_bf16", x.device, 0.0, 6.0 * x.numel()):
        check(_lib.load().pv_im2col_bf16(_ptr(x), _ptr(out), B, Cc, H, W, patch, _flag(x.device), _stream(x)), "pv_im2col_bf16")
    _count()
    return out


def im2col_u8(x: torch.Tensor, patch: int, out: torch.Tensor, mean, std) -> torch.Tensor:
    """x: uint8 [B,H,W,3] (NHWC) -> bf16 patch matrix of the ToTensor+Normalize'd image."""
    _chk(x, torch.uint8, "x")
    B, H, W, Cc = x.shape
    if Cc != 3:
        raise _lib.PeekvitHipError("uint8 input must be NHWC with 3 channels")
    with _timed("pv_im2col_u8_bf16", x.device, 0.0, 3.0 * x.numel()):
        check(_lib.load().pv_im2col_u8_bf16(_ptr(x), _ptr(out), B, H, W, patch, *[float(v) for v in mean], *[float(v) for v in std],
                                            _stream(x)), "pv_im2col_u8_bf16")
    _count()
    return out


def token_prologue(tokens, special, pos, budget_token, budget: float, n_special: int):
    B, S, D = tokens.shape
    with _timed("pv_token_prologue", tokens.device, 0.0, 0.0):
        check(_lib.load().pv_token_prologue(_ptr(tokens), _ptr(special), _ptr(pos), _ptr(budget_token), float(budget),
                                            B, S, D, n_special, _stream(tokens)), "pv_token_prologue")
    _count()


def layernorm_bf16(x: torch.Tensor, gamma, beta, eps: float, out: torch.Tensor, row_scale=None):
    """x: fp32 [..., D] contiguous -> out bf16 same shape."""
    D = x.shape[-1]
    rows = x.numel() // D
    with _timed("pv_layernorm_bf16", x.device, 0.0, 6.0 * x.numel()):
        check(_lib.load().pv_layernorm_bf16(_ptr(x), D, _ptr(gamma), _ptr(beta), _ptr(row_scale), _ptr(out), rows, D,
                                            float(eps), _stream(x)), "pv_layernorm_bf16")
    _count()
    return out


def gemm(a: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, epilogue: int, *, M=None, res=None,
         row_scale=None, pos=None, rows_per_img_in=0, rows_per_img_out=0, row_off=0, qcols=0, qscale=1.0, ln=None, ksplit=0, tag="", colsum_out=None, x16_out=None, rowstat_out=None, fold=None, rowsq_out=None, res_scaled=False):
    """out = epilogue(a[M,K] . w[N,K]^T).  a, w: bf16 2-D (row stride = shape[-1]).
    ksplit > 1: out is fp32 [ksplit, M, N] partial slices (PV_EPI_BIAS_F32), reduce with sum_slices().
    x16_out / rowstat_out (PV_EPI_BIAS_RES_F32) and fold = (stat [M,2], c1 [N], c2 [N]) (PV_EPI_BIAS_BF16 / _GELU_BF16, bias None): the
    producer / consumer halves of the folded LayerNorm (include/peekvit_hip.h).
    colsum_out (PV_EPI_GELU_GRAD_BF16): fp32 [N] tensor that receives the column sums of the output (bias gradient) - fused into the
    epilogue when the 256-row tile kernel serves the shape, a separate pv_colsum_f32 pass otherwise.
    ln = (gamma, beta, eps, ln_out_bf16, ln_row_scale | None): also emit bf16(LayerNorm(out)) (fused, PV_EPI_BIAS_RES_F32).
    res_scaled (with row_scale, PV_EPI_BIAS_RES_F32): out = row_scale * (res + a.w^T + bias) - ResidualViT with res = the unmasked tokens."""
    K = a.shape[-1]
    if M is None:
        M = a.numel() // K
    N = w.shape[0]
    range_flag = current_range_flag()
    args = GemmArgs(A=a.data_ptr(), W=w.data_ptr(), bias=bias.data_ptr() if bias is not None else 0,
                    out=out.data_ptr(), res=res.data_ptr() if res is not None else 0,
                    row_scale=row_scale.data_ptr() if row_scale is not None else 0,
                    pos=pos.data_ptr() if pos is not None else 0,
                    M=M, N=N, K=K, lda=a.stride(0) if a.dim() == 2 else K, ldw=w.stride(0) if w.dim() == 2 else w.shape[-1],
                    ldo=out.stride(-2) if out.dim() >= 2 else out.shape[-1],
                    ldr=(res.stride(0) if res.dim() == 2 else res.shape[-1]) if res is not None else 0,
                    rows_per_img_in=rows_per_img_in, rows_per_img_out=rows_per_img_out, row_off=row_off,
                    qcols=qcols, qscale=float(qscale), epilogue=epilogue,
                    ln_gamma=ln[0].data_ptr() if ln else 0, ln_beta=ln[1].data_ptr() if ln else 0,
                    ln_row_scale=ln[4].data_ptr() if ln and ln[4] is not None else 0,
                    ln_out=ln[3].data_ptr() if ln else 0, ln_eps=float(ln[2]) if ln else 0.0, ksplit=int(ksplit), colsum_partial=0,
                    x16_out=x16_out.data_ptr() if x16_out is not None else 0, rowstat_out=rowstat_out.data_ptr() if rowstat_out is not None else 0,
                    fold_stat=fold[0].data_ptr() if fold else 0, fold_c1=fold[1].data_ptr() if fold else 0, fold_c2=fold[2].data_ptr() if fold else 0,
                    range_flag=range_flag.data_ptr() if range_flag is not None and range_flag.device == a.device else 0,
                    rowsq_out=rowsq_out.data_ptr() if rowsq_out is not None else 0, res_scaled=int(res_scaled))
    part = None
    if colsum_out is not None and _lib.load().pv_gemm_tile_rows(C.byref(args)) == 256:
        part = _scratch_f32(_lib.PV_WS_GEMM_COLSUM_PARTIAL, a.device, M, N).view((M + 255) // 256, N)
        args.colsum_partial = part.data_ptr()
    # algorithmic bytes: both operands once, the output once (+ the residual rows it adds, + the 16-bit copies the fused / folded LayerNorm forms emit)
    nbytes = 2.0 * (M * K + N * K) + out.element_size() * M * N * (2 if res is not None else 1) + (2.0 * M * N if ln else 0.0) + (2.0 * M * N if x16_out is not None else 0.0)
    with _timed("pv_gemm_bf16" + tag, a.device, 2.0 * M * N * K, nbytes, member=(N, K, epilogue)):
        check(_lib.load().pv_gemm_bf16(C.byref(args), _stream(a)), "pv_gemm_bf16")
    _count()
    if colsum_out is not None:
        colsum(part if part is not None else out, colsum_out)
    return out


def rowstat_finalize(partials: torch.Tensor, D: int, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """partials fp32 [tiles, rows, 2] (sum, sum of squares per column tile) -> fp32 [rows, 2] (mean, rstd) of rows of length D."""
    _chk(partials, torch.float32, "partials")
    T, rows, _ = partials.shape
    if out is None:
        out = torch.empty((rows, 2), dtype=torch.float32, device=partials.device)
    with _timed("pv_rowstat_finalize", partials.device, 0.0, 8.0 * (T + 1) * rows):
        check(_lib.load().pv_rowstat_finalize(_ptr(partials), _ptr(out), T, rows, D, float(eps), _flag(partials.device), _stream(partials)), "pv_rowstat_finalize")
    _count()
    return out


def gemm_tn(a: torch.Tensor, b: torch.Tensor, part: torch.Tensor, ksplit: int, tag: str = "[wgrad]"):
    """part[t] = (a[K_t, M])^T . b[K_t, N] over ksplit row slices: weight gradient straight from row-major bf16 activations
    (row-strided 2-D views allowed).  part fp32 [ksplit, M, N], contiguous or the first N columns of a contiguous [ksplit, M, ldo] buffer
    (slices are M * ldo apart); reduce a contiguous one with sum_slices()."""
    K, M = a.shape
    N = b.shape[1]
    ldo = part.stride(1)
    assert b.shape[0] == K and part.shape == (max(ksplit, 1), M, N) and part.stride(2) == 1 and ldo >= N and part.stride(0) == M * ldo
    args = GemmArgs(A=a.data_ptr(), W=b.data_ptr(), bias=0, out=part.data_ptr(), res=0, row_scale=0, pos=0, M=M, N=N, K=K,
                    lda=a.stride(0), ldw=b.stride(0), ldo=ldo, ldr=0, rows_per_img_in=0, rows_per_img_out=0, row_off=0, qcols=0,
                    qscale=1.0, epilogue=_lib.PV_EPI_BIAS_F32, ln_gamma=0, ln_beta=0, ln_row_scale=0, ln_out=0, ln_eps=0.0,
                    ksplit=int(ksplit))
    with _timed("pv_gemm_tn_bf16" + tag, a.device, 2.0 * M * N * K, 2.0 * K * (M + N) + 4.0 * max(ksplit, 1) * M * N):
        check(_lib.load().pv_gemm_tn_bf16(C.byref(args), _stream(a)), "pv_gemm_tn_bf16")
    _count()
    return part


def attention(qkv: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int, dh: int, lse: Optional[torch.Tensor] = None):
    """lse (fp32 [B, H, S], optional; training forward): also receives log2(sum_k exp(s[q,k])) per row, for attention_bwd_lse."""
    with _timed("pv_attention_bf16", qkv.device, 4.0 * B * H * S * S * dh, 8.0 * B * S * H * dh):
        if lse is None:
            check(_lib.load().pv_attention_bf16(_ptr(qkv), _ptr(out), B, S, H, dh, _attn_flag(qkv.device), _stream(qkv)), "pv_attention_bf16")
        else:
            _chk(lse, torch.float32, "lse")
            if lse.numel() != B * H * S:
                raise _lib.PeekvitHipError("attention: lse must hold B * H * S values")
            check(_lib.load().pv_attention_lse_bf16(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, dh, _attn_flag(qkv.device), _stream(qkv)), "pv_attention_lse_bf16")
    _count()
    return out


def attention_bwd_lse_ok(S: int, dh: int) -> bool:
    """Shapes for which the training path takes the persistent backward (pv_attention_bwd_lse_bf16): where it serves (attention_bwd_lse_supported) AND is the
    faster kernel - 10 .. 13 query tiles (S = 197: 1.70 vs 1.97 ms, 177: 1.48 vs 1.64, 158: 1.25 vs 1.32; at 9 tiles, S = 129, the two are equal)."""
    return attention_bwd_lse_supported(S, dh) and S >= 145


def attention_bwd_lse_supported(S: int, dh: int) -> bool:
    """Shapes pv_attention_bwd_lse_bf16 accepts: 9 .. 13 query tiles of 16 (one wave each, at least three waves left for the side work), dh = 48 / 64."""
    return dh in (48, 64) and 129 <= S <= 208


def attention_rows(q: torch.Tensor, kv: torch.Tensor, out: torch.Tensor, B: int, S: int, nq: int, H: int, dh: int):
    """softmax(q k^T) v for the first `nq` rows of every image only: q 16-bit [B*nq, H*dh] (scaled), kv 16-bit [B*S, >= 2*H*dh] (k | v),
    out 16-bit [B*nq, H*dh].  Row strides are taken from the tensors (2-D views of wider buffers allowed)."""
    for t, name in ((q, "q"), (kv, "kv"), (out, "out")):
        if not (t.is_cuda and t.dtype == _lib.operand_dtype() and t.dim() == 2 and t.stride(1) == 1):
            raise _lib.PeekvitHipError(f"attention_rows: {name} must be a 2-D GPU tensor of the operand type with unit column stride")
    if q.shape[0] != B * nq or out.shape[0] != B * nq or kv.shape[0] != B * S or kv.shape[1] < 2 * H * dh:
        raise _lib.PeekvitHipError("attention_rows: shape mismatch")
    with _timed("pv_attention_rows_bf16", q.device, 4.0 * B * H * nq * S * dh, 4.0 * B * S * H * dh + 4.0 * B * nq * H * dh):
        check(_lib.load().pv_attention_rows_bf16(_ptr(q), q.stride(0), _ptr(kv), kv.stride(0), _ptr(out), out.stride(0),
                                                 B, S, nq, H, dh, _attn_flag(q.device), _stream(q)), "pv_attention_rows_bf16")
    _count()
    return out


def attention_rows_bwd(q, kv, out, dout, dq, dkv, B: int, S: int, H: int, dh: int, qscale: float):
    """Backward of attention_rows for one query row per image: q, out, dout, dq 16-bit [B, H*dh]; kv, dkv 16-bit [B*S, >= 2*H*dh]."""
    for t, name in ((q, "q"), (kv, "kv"), (out, "out"), (dout, "dout"), (dq, "dq"), (dkv, "dkv")):
        if not (t.is_cuda and t.dtype == _lib.operand_dtype() and t.dim() == 2 and t.stride(1) == 1):
            raise _lib.PeekvitHipError(f"attention_rows_bwd: {name} must be a 2-D GPU tensor of the operand type with unit column stride")
    if any(t.shape[0] != B for t in (q, out, dout, dq)) or kv.shape[0] != B * S or dkv.shape[0] != B * S:
        raise _lib.PeekvitHipError("attention_rows_bwd: shape mismatch")
    with _timed("pv_attention_rows_bwd_bf16", q.device, 10.0 * B * H * S * dh, 2.0 * 3 * 2 * B * S * H * dh):
        check(_lib.load().pv_attention_rows_bwd_bf16(_ptr(q), q.stride(0), _ptr(kv), kv.stride(0), _ptr(out), out.stride(0), _ptr(dout), dout.stride(0),
                                                     _ptr(dq), dq.stride(0), _ptr(dkv), dkv.stride(0), B, S, 1, H, dh, float(qscale), _stream(q)),
              "pv_attention_rows_bwd_bf16")
    _count()
    return dq, dkv


def cls_pool(x: torch.Tensor, gamma, beta, eps: float, num_cls: int) -> torch.Tensor:
    B, S, D = x.shape
    pooled = torch.empty((B, D), dtype=torch.float32, device=x.device)
    with _timed("pv_cls_pool", x.device, 0.0, 0.0):
        check(_lib.load().pv_cls_pool(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(pooled), B, S, D, num_cls, float(eps),
                                      _stream(x)), "pv_cls_pool")
    _count()
    return pooled


def head(pooled: torch.Tensor, w: torch.Tensor, b) -> torch.Tensor:
    B, D = pooled.shape
    Cn = w.shape[0]
    logits = torch.empty((B, Cn), dtype=torch.float32, device=pooled.device)
    with _timed("pv_head_f32", pooled.device, 2.0 * B * D * Cn, 0.0):
        check(_lib.load().pv_head_f32(_ptr(pooled), _ptr(w), _ptr(b), _ptr(logits), B, D, Cn, _stream(pooled)), "pv_head_f32")
    _count()
    return logits


# ---- backward building blocks ---------------------------------------------------------------------------------------
def sum_slices(partials: torch.Tensor, out: torch.Tensor, accumulate: bool = False, base: Optional[torch.Tensor] = None, ln=None) -> torch.Tensor:
    """out (+)= partials.sum(0); partials fp32 [S, ...] contiguous, out fp32 of the trailing shape.  base (fp32, same shape as out, may be
    out): out = base + partials.sum(0) - the finish of a split-K GEMM with a residual; with ln = (gamma, beta, eps, out16 [rows, D]) the same
    pass also emits the 16-bit LayerNorm of the finished rows (out viewed as [rows, D])."""
    _chk(partials, torch.float32, "partials"); _chk(out, torch.float32, "out")
    S = partials.shape[0]
    with _timed("pv_sum_slices_f32", out.device, 0.0, 4.0 * (S + 1 + (base is not None)) * out.numel()):
        if ln is not None:
            _chk(base, torch.float32, "base"); _chk(ln[3], _lib.operand_dtype(), "ln out")
            D = ln[3].shape[-1]
            assert base.numel() == out.numel() == ln[3].numel() and base.is_contiguous() and out.is_contiguous()
            check(_lib.load().pv_sum_slices_add_ln_f32(_ptr(partials), _ptr(base), _ptr(out), out.numel() // D, D, S, _ptr(ln[0]), _ptr(ln[1]), float(ln[2]),
                                                       _ptr(ln[3]), _stream(out)), "pv_sum_slices_add_ln_f32")
        elif base is not None:
            _chk(base, torch.float32, "base")
            assert base.numel() == out.numel() and base.is_contiguous() and out.is_contiguous()
            check(_lib.load().pv_sum_slices_add_f32(_ptr(partials), _ptr(base), _ptr(out), out.numel(), S, _stream(out)), "pv_sum_slices_add_f32")
        else:
            check(_lib.load().pv_sum_slices_f32(_ptr(partials), _ptr(out), out.numel(), S, int(accumulate), _stream(out)), "pv_sum_slices_f32")
    _count()
    return out


def sum_slices_act(partials: torch.Tensor, out: torch.Tensor, gelu: bool = False, qcols: int = 0, qscale: float = 1.0) -> torch.Tensor:
    """out (16-bit [M, N], contiguous) = gelu(partials.sum(0)) or the sum with the first qcols columns scaled: finish of a split-K fc1 / in-proj."""
    _chk(partials, torch.float32, "partials"); _chk(out, _lib.operand_dtype(), "out")
    S, M, N = partials.shape
    assert out.shape == (M, N)
    with _timed("pv_sum_slices_f32", out.device, 0.0, (4.0 * S + 2.0) * out.numel()):
        check(_lib.load().pv_sum_slices_act_bf16(_ptr(partials), _ptr(out), M, N, S, int(gelu), int(qcols), float(qscale), _flag(out.device), _stream(out)),
              "pv_sum_slices_act_bf16")
    _count()
    return out


def transpose(src: torch.Tensor, out: Optional[torch.Tensor] = None, pad_to: int = 1, colsum_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 [R,C] (row-strided view allowed) -> bf16 [C, ceil(R / pad_to) * pad_to], zero-filled beyond column R."""
    if not (src.is_cuda and src.dtype == _lib.operand_dtype() and src.dim() == 2 and src.stride(1) == 1):
        raise _lib.PeekvitHipError("transpose: expected a 2-D bf16 GPU tensor with unit column stride")
    R, Cc = src.shape
    ldd = (R + pad_to - 1) // pad_to * pad_to
    if out is None:
        out = torch.empty((Cc, ldd), dtype=_lib.operand_dtype(), device=src.device)
    assert out.shape == (Cc, ldd) and out.is_contiguous()
    ws = _scratch_f32(_lib.PV_WS_TRANSPOSE_COLSUM, src.device, R, Cc, ldd) if colsum_out is not None else None
    with _timed("pv_transpose_bf16", src.device, 0.0, 4.0 * src.numel()):
        check(_lib.load().pv_transpose_bf16(_ptr(src), src.stride(0), _ptr(out), R, Cc, ldd, _ptr(colsum_out), _ptr(ws), _stream(src)),
              "pv_transpose_bf16")
    _count()
    return out


def colsum(src: torch.Tensor, out: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """out[C] (+)= src[R,C].sum(0) in fp32; src bf16 or fp32."""
    assert src.dtype in (_lib.operand_dtype(), torch.float32) and src.is_contiguous()
    _chk(out, torch.float32, "out")
    R, Cc = src.shape
    ws = _scratch_f32(_lib.PV_WS_COLSUM, src.device, R, Cc)
    with _timed("pv_colsum_f32", src.device, 0.0, float(src.element_size() * src.numel())):
        check(_lib.load().pv_colsum_f32(_ptr(src), int(src.dtype == _lib.operand_dtype()), _ptr(out), _ptr(ws), R, Cc, int(accumulate),
                                        _stream(src)), "pv_colsum_f32")
    _count()
    return out


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, dres_in, dx_out: Optional[torch.Tensor], dgb: torch.Tensor, eps: float,
                  accumulate: bool = False, dx_bf16: Optional[torch.Tensor] = None):
    """dx_out = (dres_in or 0) + LN'(x)^T dy;  dgb [3,D] (+)= (dgamma, dbeta, colsum(dx)).  x fp32 [rows,D], dy bf16 [rows,D].
    dres_in may be a 16-BIT tensor and dx_out None (only the 16-bit copy dx_bf16 is written): the residual gradient handed over in 16 bits
    between the two LayerNorms of a block (pv_layernorm_bwd16; an option of the training path)."""
    _chk(x, torch.float32, "x"); _chk(dy, _lib.operand_dtype(), "dy"); _chk(dgb, torch.float32, "dgb")
    D = x.shape[-1]
    rows = x.numel() // D
    ws = _scratch_f32(_lib.PV_WS_LAYERNORM_BWD, x.device, rows, D)
    if dx_out is None or (dres_in is not None and dres_in.dtype != torch.float32):
        d16 = dres_in if dres_in is not None and dres_in.dtype != torch.float32 else None
        d32 = dres_in if dres_in is not None and dres_in.dtype == torch.float32 else None
        if d16 is not None:
            _chk(d16, _lib.operand_dtype(), "dres16")
        nb = 4.0 + 2.0 + (4.0 if dx_out is not None else 0.0) + (4.0 if d32 is not None else 0.0) + (2.0 if d16 is not None else 0.0) + (2.0 if dx_bf16 is not None else 0.0)
        with _timed("pv_layernorm_bwd", x.device, 0.0, nb * x.numel()):
            check(_lib.load().pv_layernorm_bwd16(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(d32), _ptr(d16), _ptr(dx_out), _ptr(dx_bf16), _ptr(dgb), _ptr(ws), ws.numel(),
                                                 rows, D, float(eps), int(accumulate), _stream(x)), "pv_layernorm_bwd16")
        _count()
        return dx_out
    _chk(dx_out, torch.float32, "dx_out")
    with _timed("pv_layernorm_bwd", x.device, 0.0, (4.0 + 2.0 + 4.0 + (4.0 if dres_in is not None else 0.0) + (2.0 if dx_bf16 is not None else 0.0)) * x.numel()):
        check(_lib.load().pv_layernorm_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(dres_in) if dres_in is not None else 0, _ptr(dx_out), _ptr(dx_bf16), _ptr(dgb),
                                           _ptr(ws), ws.numel(), rows, D, float(eps), int(accumulate), _stream(x)), "pv_layernorm_bwd")
    _count()
    return dx_out


def layernorm_bwd_masked(x, dy, gamma, beta, row_scale, dres_in, u, dx_out, dx_bf16, scale_copy: bool, dgb, dmask, dmask_accumulate: bool,
                         eps: float):
    """Backward of y = row_scale * LayerNorm(x) (ResidualViT): as layernorm_bwd, plus dmask [rows] (+)= rowdot(dy, LN(x))
    (+ rowdot(dx_out, u) when u is given); dx_bf16 = row_scale * dx_out when scale_copy."""
    _chk(x, torch.float32, "x"); _chk(dy, _lib.operand_dtype(), "dy"); _chk(dx_out, torch.float32, "dx_out")
    _chk(dgb, torch.float32, "dgb"); _chk(dmask, torch.float32, "dmask"); _chk(row_scale, torch.float32, "row_scale")
    D = x.shape[-1]
    rows = x.numel() // D
    ws = _scratch_f32(_lib.PV_WS_LAYERNORM_BWD, x.device, rows, D)
    with _timed("pv_layernorm_bwd", x.device, 0.0, 16.0 * x.numel()):
        check(_lib.load().pv_layernorm_bwd_masked(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(row_scale), _ptr(dres_in), _ptr(u),
                                                  _ptr(dx_out), _ptr(dx_bf16), int(scale_copy), _ptr(dgb), _ptr(dmask), int(dmask_accumulate),
                                                  _ptr(ws), ws.numel(), rows, D, float(eps), _stream(x)), "pv_layernorm_bwd_masked")
    _count()
    return dx_out


def masked_residual(x: torch.Tensor, u: torch.Tensor, row_scale: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out = x + row_scale[row] * u  (x, out fp32 [rows, D]; u 16-bit [rows, D])."""
    _chk(x, torch.float32, "x"); _chk(u, _lib.operand_dtype(), "u"); _chk(out, torch.float32, "out")
    D = x.shape[-1]
    with _timed("pv_masked_residual", x.device, 0.0, 10.0 * x.numel()):
        check(_lib.load().pv_masked_residual(_ptr(x), _ptr(u), _ptr(row_scale), _ptr(out), x.numel() // D, D, _stream(x)), "pv_masked_residual")
    _count()
    return out


def gelu(pre: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(pre, _lib.operand_dtype(), "pre")
    if out is None:
        out = torch.empty_like(pre)
    with _timed("pv_gelu_bf16", pre.device, 0.0, 4.0 * pre.numel()):
        check(_lib.load().pv_gelu_bf16(_ptr(pre), _ptr(out), pre.numel(), _stream(pre)), "pv_gelu_bf16")
    _count()
    return out


def gelu_bwd(pre: torch.Tensor, dg: torch.Tensor, dpre: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(pre, _lib.operand_dtype(), "pre"); _chk(dg, _lib.operand_dtype(), "dg")
    if dpre is None:
        dpre = dg
    with _timed("pv_gelu_bwd_bf16", pre.device, 0.0, 6.0 * pre.numel()):
        check(_lib.load().pv_gelu_bwd_bf16(_ptr(pre), _ptr(dg), _ptr(dpre), pre.numel(), _stream(pre)), "pv_gelu_bwd_bf16")
    _count()
    return dpre


def attention_bwd(qkv: torch.Tensor, dout: torch.Tensor, dqkv: torch.Tensor, B: int, S: int, H: int, dh: int, qscale: float,
                  dbias_partial: Optional[torch.Tensor] = None):
    """dbias_partial (fp32 [B, 3*H*dh], optional) receives the per-image column sums of dqkv."""
    with _timed("pv_attention_bwd_bf16", qkv.device, 14.0 * B * H * S * S * dh, 14.0 * B * S * H * dh):
        check(_lib.load().pv_attention_bwd_bf16(_ptr(qkv), _ptr(dout), _ptr(dqkv), _ptr(dbias_partial), B, S, H, dh, float(qscale),
                                                _stream(qkv)), "pv_attention_bwd_bf16")
    _count()
    return dqkv


def attention_bwd_lse(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dqkv: torch.Tensor, B: int, S: int, H: int, dh: int,
                      qscale: float, dbias_partial: Optional[torch.Tensor] = None):
    """attention_bwd from the forward's output `out` (16-bit [B, S, H*dh]) and row statistics `lse` (attention(..., lse=)): one persistent workgroup per CU."""
    _chk(lse, torch.float32, "lse")
    with _timed("pv_attention_bwd_bf16", qkv.device, 14.0 * B * H * S * S * dh, 16.0 * B * S * H * dh):
        check(_lib.load().pv_attention_bwd_lse_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(dqkv), _ptr(dbias_partial), B, S, H, dh,
                                                    float(qscale), _stream(qkv)), "pv_attention_bwd_lse_bf16")
    _count()
    return dqkv


def _chk_attn_stream(qkv: torch.Tensor, B: int, S: int, H: int, dh: int, what: str, **tensors):
    """Dtypes and element counts of the streaming attention entry points: qkv and the 16-bit tensors in the operand type of the current library,
    (name, tensor, dtype, numel) for the rest."""
    dt = _lib.operand_dtype()
    if min(B, S, H) < 1 or dh not in (32, 48, 64):
        raise _lib.PeekvitHipError(f"{what}: B, S, H >= 1 and dh in (32, 48, 64), got B = {B}, S = {S}, H = {H}, dh = {dh}")
    D = H * dh
    sizes = {"qkv": (dt, B * S * 3 * D), "out": (dt, B * S * D), "dout": (dt, B * S * D), "lse": (torch.float32, B * H * S),
             "dqkv": (torch.float32, B * S * 3 * D)}
    for name, t in dict(qkv=qkv, **tensors).items():
        dtype, n = sizes[name]
        _chk(t, dtype, f"{what}: {name}")
        if t.numel() != n or t.device != qkv.device:
            raise _lib.PeekvitHipError(f"{what}: {name} must hold {n} values on {qkv.device}, got {tuple(t.shape)} on {t.device}")


def attention_stream(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, B: int, S: int, H: int, dh: int):
    """The training forward for ANY S: out (16-bit [B, S, H*dh]) and lse (fp32 [B, H, S] = log2 sum_k exp(s[q, k])) from qkv (16-bit [B, S, 3*H*dh], q
    pre-scaled), always by the streaming kernel (64-key blocks, online softmax)."""
    _chk_attn_stream(qkv, B, S, H, dh, "attention_stream", out=out, lse=lse)
    with _timed("pv_attention_stream_lse_bf16", qkv.device, 4.0 * B * H * S * S * dh, 8.0 * B * S * H * dh + 4.0 * B * H * S):
        check(_lib.load().pv_attention_stream_lse_bf16(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, dh, _attn_flag(qkv.device), _stream(qkv)),
              "pv_attention_stream_lse_bf16")
    _count()
    return out


def attention_stream_bwd(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dqkv: torch.Tensor, B: int, S: int, H: int, dh: int,
                         qscale: float, delta_ws: Optional[torch.Tensor] = None):
    """dqkv (fp32 [B, S, 3*H*dh]; the q third times qscale) from attention_stream's out and lse, for ANY S: two launches (dQ, then dK | dV), no atomics.
    delta_ws (fp32 [B, H, S] scratch, allocated here unless given) holds sum_d dout * out per row afterwards."""
    _chk_attn_stream(qkv, B, S, H, dh, "attention_stream_bwd", dout=dout, out=out, lse=lse, dqkv=dqkv)
    if delta_ws is None:
        delta_ws = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
    else:
        _chk(delta_ws, torch.float32, "attention_stream_bwd: delta_ws")
        if delta_ws.numel() != B * H * S or delta_ws.device != qkv.device:
            raise _lib.PeekvitHipError("attention_stream_bwd: delta_ws must hold B * H * S values on qkv's device")
    with _timed("pv_attention_stream_bwd_bf16", qkv.device, 14.0 * B * H * S * S * dh, 20.0 * B * S * H * dh + 12.0 * B * H * S):
        check(_lib.load().pv_attention_stream_bwd_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(dqkv), _ptr(delta_ws), B, S, H, dh, float(qscale),
                                                       _stream(qkv)), "pv_attention_stream_bwd_bf16")
    _count()
    return dqkv


def attention_stream_bwd16(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dqkv16: torch.Tensor, B: int, S: int, H: int, dh: int,
                           qscale: float, dbias_partial: Optional[torch.Tensor] = None, delta_ws: Optional[torch.Tensor] = None):
    """attention_stream_bwd with a 16-BIT result: dqkv16 (the operand type, [B, S, 3*H*dh]) = that function's fp32 value rounded once.  dbias_partial
    (optional fp32 [B, ceil(S / 64), 3*H*dh]) receives the column sums of the stored values per block of 64 rows: colsum() over its rows ends the bias
    gradient (pv_attention_stream_bwd16_bf16, include/peekvit_hip_pct_block.h)."""
    _chk_attn_stream(qkv, B, S, H, dh, "attention_stream_bwd16", dout=dout, out=out, lse=lse)
    dev, D3 = qkv.device, 3 * H * dh
    _chk(dqkv16, _lib.operand_dtype(), "attention_stream_bwd16: dqkv16")
    if dqkv16.numel() != B * S * D3 or dqkv16.device != dev:
        raise _lib.PeekvitHipError(f"attention_stream_bwd16: dqkv16 must hold {B * S * D3} values on {dev}")
    if dbias_partial is not None:
        _chk(dbias_partial, torch.float32, "attention_stream_bwd16: dbias_partial")
        if dbias_partial.numel() != B * ((S + 63) // 64) * D3 or dbias_partial.device != dev:
            raise _lib.PeekvitHipError("attention_stream_bwd16: dbias_partial must hold B * ceil(S / 64) * 3 * H * dh values on qkv's device")
    if delta_ws is None:
        delta_ws = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    else:
        _chk(delta_ws, torch.float32, "attention_stream_bwd16: delta_ws")
        if delta_ws.numel() != B * H * S or delta_ws.device != dev:
            raise _lib.PeekvitHipError("attention_stream_bwd16: delta_ws must hold B * H * S values on qkv's device")
    with _timed("pv_attention_stream_bwd16_bf16", dev, 14.0 * B * H * S * S * dh, 14.0 * B * S * H * dh + 12.0 * B * H * S):
        check(_lib.load().pv_attention_stream_bwd16_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(dqkv16), _ptr(dbias_partial), _ptr(delta_ws), B, S, H, dh,
                                                         float(qscale), _stream(qkv)), "pv_attention_stream_bwd16_bf16")
    _count()
    return dqkv16


def layernorm_bwd_sum(x: torch.Tensor, dy16: Optional[torch.Tensor], dy32: Optional[torch.Tensor], gamma: torch.Tensor, dx_out: Optional[torch.Tensor],
                      dx16: Optional[torch.Tensor], dgb: torch.Tensor, eps: float, accumulate: bool = False):
    """LayerNorm backward of a gradient that is a SUM: dy = float(dy16) + dy32 in fp32 (either may be None, not both), dx = LN'(x)^T dy into dx_out (fp32)
    and / or dx16 (the operand type); dgb [3, D] (+)= (dgamma, dbeta, colsum of dx - of its 16-bit values when dx16 is given).  x fp32 [rows, D]
    (pv_layernorm_bwd_sum, include/peekvit_hip_pct_block.h)."""
    _chk(x, torch.float32, "layernorm_bwd_sum: x"); _chk(dgb, torch.float32, "layernorm_bwd_sum: dgb"); _chk(gamma, torch.float32, "layernorm_bwd_sum: gamma")
    if (dy16 is None and dy32 is None) or (dx_out is None and dx16 is None):
        raise _lib.PeekvitHipError("layernorm_bwd_sum: one of dy16 / dy32 and one of dx_out / dx16 must be given")
    D = x.shape[-1]
    rows = x.numel() // D
    for name, t, dtype in (("dy16", dy16, _lib.operand_dtype()), ("dy32", dy32, torch.float32), ("dx_out", dx_out, torch.float32), ("dx16", dx16, _lib.operand_dtype())):
        if t is not None:
            _chk(t, dtype, "layernorm_bwd_sum: " + name)
            if t.numel() != rows * D or t.device != x.device:
                raise _lib.PeekvitHipError(f"layernorm_bwd_sum: {name} must hold {rows * D} values on {x.device}")
    if gamma.numel() != D or dgb.numel() != 3 * D:
        raise _lib.PeekvitHipError("layernorm_bwd_sum: gamma must hold D and dgb 3 * D values")
    ws = _scratch_f32(_lib.PV_WS_LAYERNORM_BWD, x.device, rows, D)
    nb = 4.0 + sum(b for t, b in ((dy16, 2.0), (dy32, 4.0), (dx_out, 4.0), (dx16, 2.0)) if t is not None)
    with _timed("pv_layernorm_bwd_sum", x.device, 0.0, nb * x.numel()):
        check(_lib.load().pv_layernorm_bwd_sum(_ptr(x), _ptr(dy16), _ptr(dy32), _ptr(gamma), _ptr(dx_out), _ptr(dx16), _ptr(dgb), _ptr(ws), ws.numel(), rows, D,
                                               float(eps), int(accumulate), _stream(x)), "pv_layernorm_bwd_sum")
    _count()
    return dx_out if dx_out is not None else dx16


def wgrad(dy_t: torch.Tensor, x_t: torch.Tensor, out: torch.Tensor, accumulate: bool = False, ksplit: int = 0) -> torch.Tensor:
    """out[N_out, N_in] (+)= dY^T . X from the TRANSPOSED bf16 activations dy_t [N_out, M], x_t [N_in, M] (split-K over M)."""
    No, M = dy_t.shape
    Ni = x_t.shape[0]
    if ksplit <= 0:
        tiles = ((No + 255) // 256) * ((Ni + 255) // 256)
        ksplit = 1
        while tiles * ksplit < 512 and M % (ksplit * 2 * 128) == 0 and M // (ksplit * 2) >= 1024:
            ksplit *= 2
    part = _scratch_f32(_lib.PV_WS_GEMM_SPLITK, out.device, No, Ni, ksplit).view(ksplit, No, Ni)
    gemm(dy_t, x_t, None, part, _lib.PV_EPI_BIAS_F32, ksplit=ksplit)
    return sum_slices(part, out, accumulate)


# ---- precision mode "bf16x3" ---------------------------------------------------------------------------------------
def split3(src: torch.Tensor, order: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [rows,K] -> bf16 [rows,3K]: order 0 = [hi|lo|hi] (activations), 1 = [hi|hi|lo] (weights)."""
    _chk(src, torch.float32, "src")
    rows, K = src.shape
    if out is None:
        out = torch.empty((rows, 3 * K), dtype=_lib.operand_dtype(), device=src.device)
    with _timed("pv_split3_f32_bf16", src.device, 0.0, 10.0 * src.numel()):
        check(_lib.load().pv_split3_f32_bf16(_ptr(src), _ptr(out), rows, K, order, _stream(src)), "pv_split3_f32_bf16")
    _count()
    return out


def im2col_split(x: torch.Tensor, patch: int, out: torch.Tensor) -> torch.Tensor:
    _chk(x, torch.float32, "x")
    B, Cc, H, W = x.shape
    with _timed("pv_im2col_split_bf16", x.device, 0.0, 10.0 * x.numel()):
        check(_lib.load().pv_im2col_split_bf16(_ptr(x), _ptr(out), B, Cc, H, W, patch, _stream(x)), "pv_im2col_split_bf16")
    _count()
    return out


def layernorm_split(x: torch.Tensor, gamma, beta, eps: float, out: torch.Tensor, row_scale=None):
    D = x.shape[-1]
    rows = x.numel() // D
    with _timed("pv_layernorm_split_bf16", x.device, 0.0, 10.0 * x.numel()):
        check(_lib.load().pv_layernorm_split_bf16(_ptr(x), D, _ptr(gamma), _ptr(beta), _ptr(row_scale), _ptr(out), rows, D,
                                                  float(eps), _stream(x)), "pv_layernorm_split_bf16")
    _count()
    return out


def attention_f32(qkv: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int, dh: int):
    _chk(qkv, torch.float32, "qkv")
    with _timed("pv_attention_f32_split", qkv.device, 4.0 * B * H * S * S * dh, 18.0 * B * S * H * dh):
        check(_lib.load().pv_attention_f32_split(_ptr(qkv), _ptr(out), B, S, H, dh, _stream(qkv)), "pv_attention_f32_split")
    _count()
    return out


def attention_split(qkv: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int, dh: int):
    """Attention with split-operand scores (the local fallback of the score guard): qkv fp32 [B*S, 3*H*dh] (q pre-scaled) -> out 16-bit [B*S, H*dh]."""
    _chk(qkv, torch.float32, "qkv"); _chk(out, _lib.operand_dtype(), "out")
    with _timed("pv_attention_split_bf16", qkv.device, 8.0 * B * H * S * S * dh, 14.0 * B * S * H * dh):
        check(_lib.load().pv_attention_split_bf16(_ptr(qkv), _ptr(out), B, S, H, dh, _stream(qkv)), "pv_attention_split_bf16")
    _count()
    return out


def token_norm(x: torch.Tensor) -> torch.Tensor:
    B, S, D = x.shape
    norms = torch.empty((B, S - 1), dtype=torch.float32, device=x.device)
    with _timed("pv_token_norm", x.device, 0.0, 4.0 * x.numel()):
        check(_lib.load().pv_token_norm(_ptr(x), _ptr(norms), B, S, D, _stream(x)), "pv_token_norm")
    _count()
    return norms


def rank_topk(norms: torch.Tensor, k: int, gap_min: Optional[torch.Tensor] = None) -> torch.Tensor:
    """keep int32 [B,k]; gap_min (fp32 [B], optional) is lowered to each image's relative gap at the keep boundary (include/peekvit_hip.h pv_rank_topk_gap)."""
    B, N = norms.shape
    keep = torch.empty((B, k), dtype=torch.int32, device=norms.device)
    if gap_min is not None:
        _chk(gap_min, torch.float32, "gap_min")
        assert gap_min.numel() == B
    with _timed("pv_rank_topk", norms.device, 0.0, 4.0 * (norms.numel() + B * k)):
        check(_lib.load().pv_rank_topk_gap(_ptr(norms), _ptr(keep), _ptr(gap_min), B, N, k, _stream(norms)), "pv_rank_topk_gap")
    _count()
    return keep


def gemm_tile_rows(M: int, N: int, K: int, epilogue: int, **fields) -> int:
    """The M-tile height (256 or 128) pv_gemm_bf16 would choose for this shape (features such as rowsq_out need 256), or a negative
    PV_ERR_* where it would refuse the call.  Nothing is launched: the pointers are fake aligned addresses.  fields: any other member of
    pv_gemm_args the choice depends on (lda, ldw, ldo, ldr, qcols, ksplit, pos, rows_per_img_in, ...), dense strides by default."""
    args = GemmArgs(A=16, W=16, out=16, res=16, M=M, N=N, K=K, lda=K, ldw=K, ldo=N, ldr=N, qscale=1.0, epilogue=epilogue)
    known = {f[0] for f in GemmArgs._fields_} - {"struct_size"}
    for name, value in fields.items():
        if name not in known:          # (setattr on a ctypes Structure would quietly create a plain attribute)
            raise _lib.PeekvitHipError(f"gemm_tile_rows: pv_gemm_args has no member {name!r}")
        setattr(args, name, value)
    return int(_lib.load().pv_gemm_tile_rows(C.byref(args)))


def rank_topk_partials(rowsq: torch.Tensor, B: int, S: int, k: int, gap_min: Optional[torch.Tensor] = None) -> torch.Tensor:
    """keep int32 [B,k] from a producer GEMM's per-column-tile row sums of squares (rowsq fp32 [tiles, B*S]); gap_min as in rank_topk."""
    _chk(rowsq, torch.float32, "rowsq")
    tiles = rowsq.shape[0]
    keep = torch.empty((B, k), dtype=torch.int32, device=rowsq.device)
    if gap_min is not None:
        _chk(gap_min, torch.float32, "gap_min")
        assert gap_min.numel() == B
    with _timed("pv_rank_topk", rowsq.device, 0.0, 4.0 * (rowsq.numel() + B * k)):
        check(_lib.load().pv_rank_topk_partials_gap(_ptr(rowsq), tiles, _ptr(keep), _ptr(gap_min), B, S, k, _stream(rowsq)), "pv_rank_topk_partials_gap")
    _count()
    return keep


def gather_tokens(x: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    B, S, D = x.shape
    k = keep.shape[1]
    out = torch.empty((B, k + 1, D), dtype=torch.float32, device=x.device)
    with _timed("pv_gather_tokens", x.device, 0.0, 8.0 * B * (k + 1) * D):
        check(_lib.load().pv_gather_tokens(_ptr(x), _ptr(keep), _ptr(out), B, S, k, D, _stream(x)), "pv_gather_tokens")
    _count()
    return out


def scatter_tokens(dy: torch.Tensor, keep: torch.Tensor, S_in: int) -> torch.Tensor:
    """Backward of gather_tokens: dy fp32 [B,1+k,D] -> dx fp32 [B,S_in,D] (zeros at dropped tokens)."""
    _chk(dy, torch.float32, "dy")
    B, k1, D = dy.shape
    dx = torch.empty((B, S_in, D), dtype=torch.float32, device=dy.device)
    with _timed("pv_scatter_tokens", dy.device, 0.0, 4.0 * B * (k1 + S_in) * D):
        check(_lib.load().pv_scatter_tokens(_ptr(dy), _ptr(keep), _ptr(dx), B, S_in, k1 - 1, D, _stream(dy)), "pv_scatter_tokens")
    _count()
    return dx


def residual_gate(x: torch.Tensor, x_out: torch.Tensor, wg, bg, wb, bb, temp: float, sigmoid_bias: float, thr_out: Optional[torch.Tensor] = None,
                  ln=None):
    """Returns (mask [B,N,1], row_scale [B,S]); x_out receives [cls | mask*img | budget]; thr_out (fp32 [B], optional): the thresholds;
    ln = (gamma, beta, eps, out 16-bit [B*S, D]): also row_scale * LayerNorm(x_out) from the same pass."""
    B, S, D = x.shape
    mask = torch.empty((B, S - 2, 1), dtype=torch.float32, device=x.device)
    row_scale = torch.empty((B, S), dtype=torch.float32, device=x.device)
    if ln is not None:
        _chk(ln[3], _lib.operand_dtype(), "ln out")
    with _timed("pv_residual_gate", x.device, 0.0, (8.0 + (2.0 if ln is not None else 0.0)) * x.numel()):
        check(_lib.load().pv_residual_gate(_ptr(x), _ptr(x_out), _ptr(wg), _ptr(bg), _ptr(wb), _ptr(bb), float(temp),
                                           float(sigmoid_bias), _ptr(mask), _ptr(row_scale), _ptr(thr_out),
                                           _ptr(ln[0]) if ln is not None else C.c_void_p(0), _ptr(ln[1]) if ln is not None else C.c_void_p(0),
                                           float(ln[2]) if ln is not None else 0.0, _ptr(ln[3]) if ln is not None else C.c_void_p(0),
                                           B, S, D, _stream(x)),
              "pv_residual_gate")
    _count()
    return mask, row_scale


def residual_gate_bwd(x: torch.Tensor, dxo: torch.Tensor, drow: torch.Tensor, wg, bg, wb, bb, temp: float, sigmoid_bias: float):
    """Backward of residual_gate: returns (dx [B,S,D], dwg [D], dbg [1], dwb [D], dbb [1]) for x, dxo fp32 [B,S,D], drow fp32 [B,S]."""
    _chk(x, torch.float32, "x"); _chk(dxo, torch.float32, "dxo"); _chk(drow, torch.float32, "drow")
    B, S, D = x.shape
    dev = x.device
    dx = torch.empty_like(x)
    dwg_p = torch.empty((B, D), dtype=torch.float32, device=dev)
    dwb_p = torch.empty((B, D), dtype=torch.float32, device=dev)
    scal_p = torch.empty((B, 4), dtype=torch.float32, device=dev)          # (dbg, dbb, 0, 0): four columns for pv_colsum_f32's 16-byte loads
    with _timed("pv_residual_gate_bwd", dev, 0.0, 12.0 * x.numel()):
        check(_lib.load().pv_residual_gate_bwd(_ptr(x), _ptr(dxo), _ptr(drow), _ptr(wg), _ptr(bg), _ptr(wb), _ptr(bb), float(temp), float(sigmoid_bias),
                                               _ptr(dx), _ptr(dwg_p), _ptr(dwb_p), _ptr(scal_p), B, S, D, _stream(x)), "pv_residual_gate_bwd")
    _count()
    dwg = colsum(dwg_p, torch.empty((D,), dtype=torch.float32, device=dev))
    dwb = colsum(dwb_p, torch.empty((D,), dtype=torch.float32, device=dev))
    scal = colsum(scal_p, torch.empty((4,), dtype=torch.float32, device=dev))
    return dx, dwg, scal[0:1], dwb, scal[1:2]


def attention_varlen(qkv: torch.Tensor, out: torch.Tensor, seg_start: torch.Tensor, n_halted: torch.Tensor, max_len: int, H: int, dh: int):
    """A-ViT packed halting: softmax(q k^T) v within every row segment of the packed qkv 16-bit [R, 3*H*dh] -> out 16-bit [R, H*dh]; the last
    key of image b counts n_halted[b] times when that is > 0 (include/peekvit_hip.h pv_attention_varlen_bf16)."""
    _chk(seg_start, torch.int32, "seg_start"); _chk(n_halted, torch.int32, "n_halted")
    B = n_halted.numel()
    R = qkv.shape[0]
    with _timed("pv_attention_varlen_bf16", qkv.device, 4.0 * H * R * max_len * dh, 8.0 * R * H * dh):
        check(_lib.load().pv_attention_varlen_bf16(_ptr(qkv), _ptr(out), _ptr(seg_start), _ptr(n_halted), B, int(max_len), H, dh,
                                                   _attn_flag(qkv.device), _stream(qkv)), "pv_attention_varlen_bf16")
    _count()
    return out


def act_step(y: torch.Tensor, seg_start: torch.Tensor, n_halted: torch.Tensor, pos: torch.Tensor, state, acc: torch.Tensor, h_part: torch.Tensor,
             gate_scale: float, gate_center: float, threshold: float, last: bool, nxt=None):
    """One A-ViT halting step on the packed block output y fp32 [R, D] (include/peekvit_hip.h pv_act_step).  state = (c, r, rho, counter, mask)
    fp32 [B, S], updated in place; acc fp32 [B, num_cls, D]; h_part fp32 [B].  nxt = (x_next, row_scale_next, seg_next, n_halted_next, pos_next,
    totals) receives the next packed input unless `last`."""
    _chk(y, torch.float32, "y")
    for t, name in ((seg_start, "seg_start"), (n_halted, "n_halted"), (pos, "pos")):
        _chk(t, torch.int32, name)
    for t in (*state, acc, h_part):
        _chk(t, torch.float32, "state")
    B, S = state[0].shape
    D = y.shape[-1]
    nxt = nxt if nxt is not None else (None,) * 6
    with _timed("pv_act_step", y.device, 0.0, 8.0 * y.numel() + 20.0 * B * S):
        check(_lib.load().pv_act_step(_ptr(y), _ptr(seg_start), _ptr(n_halted), _ptr(pos), B, S, D, *[_ptr(t) for t in state], _ptr(acc),
                                      acc.shape[1], _ptr(h_part), float(gate_scale), float(gate_center), float(threshold), int(bool(last)),
                                      *[_ptr(t) for t in nxt], _stream(y)), "pv_act_step")
    _count()


# ------------------------------------------------------------------------------------------------
# ResidualViT exact token compaction (include/peekvit_hip_sparse.h)
# ------------------------------------------------------------------------------------------------
def attention_varlen_w(qkv: torch.Tensor, out: torch.Tensor, seg_start: torch.Tensor, log_mult: torch.Tensor, max_len: int, H: int, dh: int):
    """Ragged attention with a weight per key: softmax(q k^T + log_mult) v within every row segment of the packed qkv 16-bit [R, 3*H*dh] -> out
    16-bit [R, H*dh]; log_mult fp32 [R] (ln n for a row that stands for n identical tokens)."""
    _chk(qkv, _lib.operand_dtype(), "qkv"); _chk(out, _lib.operand_dtype(), "out")
    _chk(seg_start, torch.int32, "seg_start"); _chk(log_mult, torch.float32, "log_mult")
    B = seg_start.numel() - 1
    R = qkv.shape[0]
    if qkv.shape[1] != 3 * H * dh or out.shape[0] != R or out.shape[1] != H * dh or log_mult.numel() != R:
        raise _lib.PeekvitHipError(f"attention_varlen_w: shapes qkv {tuple(qkv.shape)}, out {tuple(out.shape)}, log_mult {tuple(log_mult.shape)}")
    with _timed("pv_attention_varlen_w_bf16", qkv.device, 4.0 * H * R * max_len * dh, 8.0 * R * H * dh):
        check(_lib.load().pv_attention_varlen_w_bf16(_ptr(qkv), _ptr(out), _ptr(seg_start), _ptr(log_mult), B, int(max_len), H, dh,
                                                     _attn_flag(qkv.device), _stream(qkv)), "pv_attention_varlen_w_bf16")
    _count()
    return out


def residual_pack_step(x: torch.Tensor, seg_start: torch.Tensor, mult: torch.Tensor, tok_row: torch.Tensor, wg, bg, wb, bb, temp: float,
                       sigmoid_bias: float, nxt, mask_out: torch.Tensor, thr_out: torch.Tensor, totals: torch.Tensor, ln=None, mask_row=None):
    """One gate + compaction step of the packed ResidualViT forward (include/peekvit_hip_sparse.h pv_residual_pack_step).  x fp32 [R, D];
    seg_start int32 [B + 1]; mult int32 [R]; tok_row int32 [B, N]; nxt = (x_next [R, D], row_scale_next [R], mult_next [R], log_mult_next [R],
    seg_next [B + 1], tok_row_next [B, N]); mask_out fp32 [B, N]; thr_out fp32 [B]; totals int32 [2]; ln = (gamma, beta, eps, out 16-bit [R, D])."""
    _chk(x, torch.float32, "x")
    R, D = x.shape
    B, N = tok_row.shape
    x_next, rs_next, mult_next, lm_next, seg_next, tok_next = nxt
    for t, name, n in ((seg_start, "seg_start", B + 1), (mult, "mult", R), (tok_row, "tok_row", B * N), (mult_next, "mult_next", R),
                       (seg_next, "seg_next", B + 1), (tok_next, "tok_row_next", B * N), (totals, "totals", 2)):
        _chk(t, torch.int32, name)
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"residual_pack_step: {name} holds {t.numel()} elements, needs {n}")
    if mask_row is None:
        mask_row = torch.empty((R,), dtype=torch.float32, device=x.device)
    for t, name, n in ((x_next, "x_next", R * D), (rs_next, "row_scale_next", R), (lm_next, "log_mult_next", R), (mask_out, "mask_out", B * N),
                       (thr_out, "thr_out", B), (mask_row, "mask_row", R)):
        _chk(t, torch.float32, name)
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"residual_pack_step: {name} holds {t.numel()} elements, needs {n}")
    if ln is not None:
        _chk(ln[3], _lib.operand_dtype(), "ln out")
        if ln[3].numel() < R * D:
            raise _lib.PeekvitHipError("residual_pack_step: ln out is smaller than [R, D]")
    null = C.c_void_p(0)
    with _timed("pv_residual_pack_step", x.device, 0.0, (12.0 + (2.0 if ln is not None else 0.0)) * x.numel()):
        check(_lib.load().pv_residual_pack_step(_ptr(x), _ptr(seg_start), _ptr(mult), _ptr(tok_row), B, N, D, _ptr(wg), _ptr(bg), _ptr(wb), _ptr(bb),
                                                float(temp), float(sigmoid_bias), _ptr(mask_row), _ptr(x_next), _ptr(rs_next), _ptr(mult_next),
                                                _ptr(lm_next), _ptr(seg_next), _ptr(tok_next), _ptr(mask_out), _ptr(thr_out), _ptr(totals),
                                                _ptr(ln[0]) if ln is not None else null, _ptr(ln[1]) if ln is not None else null,
                                                float(ln[2]) if ln is not None else 0.0, _ptr(ln[3]) if ln is not None else null, _stream(x)),
              "pv_residual_pack_step")
    _count()


# ------------------------------------------------------------------------------------------------
# ResidualViT exact token compaction past 208 rows per image (include/peekvit_hip_sparse_long.h)
# ------------------------------------------------------------------------------------------------
SPARSE_LONG_MAX_LEN = 4096          # PV_SPARSE_LONG_MAX_LEN


def attention_varlen_w_stream(qkv: torch.Tensor, out: torch.Tensor, seg_start: torch.Tensor, log_mult: torch.Tensor, max_len: int, H: int, dh: int):
    """attention_varlen_w for row segments of any length up to 4096: the keys of a segment stream through LDS in blocks of 64 (online softmax)
    instead of staying resident.  Same arguments; `out` rows behind the last segment are not written."""
    _chk(qkv, _lib.operand_dtype(), "qkv"); _chk(out, _lib.operand_dtype(), "out")
    _chk(seg_start, torch.int32, "seg_start"); _chk(log_mult, torch.float32, "log_mult")
    B = seg_start.numel() - 1
    R = qkv.shape[0]
    if qkv.shape[1] != 3 * H * dh or out.shape[0] < R or out.shape[1] != H * dh or log_mult.numel() != R:
        raise _lib.PeekvitHipError(f"attention_varlen_w_stream: shapes qkv {tuple(qkv.shape)}, out {tuple(out.shape)}, log_mult {tuple(log_mult.shape)}")
    with _timed("pv_attention_varlen_w_stream_bf16", qkv.device, 4.0 * H * R * max_len * dh, 8.0 * R * H * dh):
        check(_lib.load().pv_attention_varlen_w_stream_bf16(_ptr(qkv), _ptr(out), _ptr(seg_start), _ptr(log_mult), B, int(max_len), H, dh,
                                                            _attn_flag(qkv.device), _stream(qkv)), "pv_attention_varlen_w_stream_bf16")
    _count()
    return out


def residual_pack_step_long(x: torch.Tensor, seg_start: torch.Tensor, mult: torch.Tensor, tok_row: torch.Tensor, wg, bg, wb, bb, temp: float,
                            sigmoid_bias: float, nxt, mask_out: torch.Tensor, thr_out: torch.Tensor, totals: torch.Tensor, ln=None, mask_row=None):
    """residual_pack_step for images of up to 4096 rows (include/peekvit_hip_sparse_long.h pv_residual_pack_step_long): the same arguments and
    results."""
    _chk(x, torch.float32, "x")
    R, D = x.shape
    B, N = tok_row.shape
    x_next, rs_next, mult_next, lm_next, seg_next, tok_next = nxt
    for t, name, n in ((seg_start, "seg_start", B + 1), (mult, "mult", R), (tok_row, "tok_row", B * N), (mult_next, "mult_next", R),
                       (seg_next, "seg_next", B + 1), (tok_next, "tok_row_next", B * N), (totals, "totals", 2)):
        _chk(t, torch.int32, name)
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"residual_pack_step_long: {name} holds {t.numel()} elements, needs {n}")
    if mask_row is None:
        mask_row = torch.empty((R,), dtype=torch.float32, device=x.device)
    for t, name, n in ((x_next, "x_next", R * D), (rs_next, "row_scale_next", R), (lm_next, "log_mult_next", R), (mask_out, "mask_out", B * N),
                       (thr_out, "thr_out", B), (mask_row, "mask_row", R)):
        _chk(t, torch.float32, name)
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"residual_pack_step_long: {name} holds {t.numel()} elements, needs {n}")
    if ln is not None:
        _chk(ln[3], _lib.operand_dtype(), "ln out")
        if ln[3].numel() < R * D:
            raise _lib.PeekvitHipError("residual_pack_step_long: ln out is smaller than [R, D]")
    null = C.c_void_p(0)
    with _timed("pv_residual_pack_step_long", x.device, 0.0, (12.0 + (2.0 if ln is not None else 0.0)) * x.numel()):
        check(_lib.load().pv_residual_pack_step_long(_ptr(x), _ptr(seg_start), _ptr(mult), _ptr(tok_row), B, N, D, _ptr(wg), _ptr(bg), _ptr(wb), _ptr(bb),
                                                     float(temp), float(sigmoid_bias), _ptr(mask_row), _ptr(x_next), _ptr(rs_next), _ptr(mult_next),
                                                     _ptr(lm_next), _ptr(seg_next), _ptr(tok_next), _ptr(mask_out), _ptr(thr_out), _ptr(totals),
                                                     _ptr(ln[0]) if ln is not None else null, _ptr(ln[1]) if ln is not None else null,
                                                     float(ln[2]) if ln is not None else 0.0, _ptr(ln[3]) if ln is not None else null, _stream(x)),
              "pv_residual_pack_step_long")
    _count()


# ------------------------------------------------------------------------------------------------
# ResidualViT training on the packed rows (include/peekvit_hip_sparse_train.h)
# ------------------------------------------------------------------------------------------------
def _chk_ragged(qkv: torch.Tensor, seg_start: torch.Tensor, log_mult: torch.Tensor, H: int, dh: int, what: str, **like_out):
    """Shapes of a ragged attention call: qkv 16-bit [R, 3 H dh], seg_start int32 [B + 1], log_mult fp32 [R]; like_out: 16-bit [R, H dh] tensors."""
    _chk(qkv, _lib.operand_dtype(), what + ": qkv"); _chk(seg_start, torch.int32, what + ": seg_start"); _chk(log_mult, torch.float32, what + ": log_mult")
    R = qkv.shape[0]
    if qkv.dim() != 2 or qkv.shape[1] != 3 * H * dh or log_mult.numel() != R or seg_start.numel() < 2:
        raise _lib.PeekvitHipError(f"{what}: shapes qkv {tuple(qkv.shape)}, log_mult {tuple(log_mult.shape)}, seg_start {tuple(seg_start.shape)}")
    for name, t in like_out.items():
        _chk(t, _lib.operand_dtype(), f"{what}: {name}")
        if t.numel() != R * H * dh or t.device != qkv.device:
            raise _lib.PeekvitHipError(f"{what}: {name} must hold {R * H * dh} values on {qkv.device}")
    return R, seg_start.numel() - 1


def attention_varlen_w_lse(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, seg_start: torch.Tensor, log_mult: torch.Tensor, max_len: int, H: int, dh: int):
    """attention_varlen_w that also writes the rows' statistics lse fp32 [R, H] (log2 sum exp, the key weights included); `out` has attention_varlen_w's bits."""
    what = "attention_varlen_w_lse"
    R, B = _chk_ragged(qkv, seg_start, log_mult, H, dh, what, out=out)
    _chk(lse, torch.float32, what + ": lse")
    if lse.numel() != R * H or lse.device != qkv.device:
        raise _lib.PeekvitHipError(f"{what}: lse must hold {R * H} values on {qkv.device}")
    with _timed("pv_attention_varlen_w_lse_bf16", qkv.device, 4.0 * H * R * max_len * dh, 8.0 * R * H * dh + 4.0 * R * H):
        check(_lib.load().pv_attention_varlen_w_lse_bf16(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(seg_start), _ptr(log_mult), B, int(max_len), H, dh,
                                                         _attn_flag(qkv.device), _stream(qkv)), "pv_attention_varlen_w_lse_bf16")
    _count()
    return out


def attention_varlen_w_bwd16(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, seg_start: torch.Tensor, log_mult: torch.Tensor,
                             dqkv16: torch.Tensor, max_len: int, H: int, dh: int, qscale: float, dbias_partial: Optional[torch.Tensor] = None,
                             delta_ws: Optional[torch.Tensor] = None):
    """Backward of attention_varlen_w_lse: dqkv16 16-bit [R, 3 H dh] = dq * qscale | dk | dv (the k | v row of a weighted key is the sum over the keys it
    stands for); dbias_partial fp32 [B * ceil(max_len / 64), 3 H dh] (optional): partial column sums of the stored values, every row written."""
    what = "attention_varlen_w_bwd16"
    R, B = _chk_ragged(qkv, seg_start, log_mult, H, dh, what, dout=dout, out=out)
    dev, D3 = qkv.device, 3 * H * dh
    _chk(lse, torch.float32, what + ": lse"); _chk(dqkv16, _lib.operand_dtype(), what + ": dqkv16")
    if lse.numel() != R * H or dqkv16.numel() != R * D3 or dqkv16.device != dev or lse.device != dev:
        raise _lib.PeekvitHipError(f"{what}: lse must hold {R * H} and dqkv16 {R * D3} values on {dev}")
    nb = (int(max_len) + 63) // 64
    if dbias_partial is not None:
        _chk(dbias_partial, torch.float32, what + ": dbias_partial")
        if dbias_partial.numel() != B * nb * D3 or dbias_partial.device != dev:
            raise _lib.PeekvitHipError(what + ": dbias_partial must hold B * ceil(max_len / 64) * 3 * H * dh values on qkv's device")
    if delta_ws is None:
        delta_ws = torch.empty((R, H), dtype=torch.float32, device=dev)
    else:
        _chk(delta_ws, torch.float32, what + ": delta_ws")
        if delta_ws.numel() != R * H or delta_ws.device != dev:
            raise _lib.PeekvitHipError(what + ": delta_ws must hold R * H values on qkv's device")
    with _timed("pv_attention_varlen_w_bwd16_bf16", dev, 14.0 * H * R * max_len * dh, 14.0 * R * H * dh + 12.0 * R * H):
        check(_lib.load().pv_attention_varlen_w_bwd16_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(seg_start), _ptr(log_mult), _ptr(dqkv16),
                                                           _ptr(dbias_partial), _ptr(delta_ws), B, int(max_len), H, dh, float(qscale), _stream(qkv)),
              "pv_attention_varlen_w_bwd16_bf16")
    _count()
    return dqkv16


def residual_pack_step_train(x: torch.Tensor, seg_start: torch.Tensor, mult: torch.Tensor, tok_row: torch.Tensor, wg, bg, wb, bb, temp: float,
                             sigmoid_bias: float, nxt, mask_out: torch.Tensor, thr_out: torch.Tensor, totals: torch.Tensor, mask_row: torch.Tensor,
                             gate_arg: torch.Tensor, src_next: torch.Tensor, ln=None):
    """residual_pack_step for training: the same results, plus mask_row fp32 [R] (the masks of the input rows), gate_arg fp32 [R] (the sigmoid's
    argument of every input row) and src_next int32 [R] (the input row of every written row, relative to its segment; -1: the zero row) - what
    residual_pack_step_bwd reads."""
    what = "residual_pack_step_train"
    _chk(x, torch.float32, what + ": x")
    R, D = x.shape
    B, N = tok_row.shape
    x_next, rs_next, mult_next, lm_next, seg_next, tok_next = nxt
    for t, name, n in ((seg_start, "seg_start", B + 1), (mult, "mult", R), (tok_row, "tok_row", B * N), (mult_next, "mult_next", R),
                       (seg_next, "seg_next", B + 1), (tok_next, "tok_row_next", B * N), (totals, "totals", 2), (src_next, "src_next", R)):
        _chk(t, torch.int32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    for t, name, n in ((x_next, "x_next", R * D), (rs_next, "row_scale_next", R), (lm_next, "log_mult_next", R), (mask_out, "mask_out", B * N),
                       (thr_out, "thr_out", B), (mask_row, "mask_row", R), (gate_arg, "gate_arg", R)):
        _chk(t, torch.float32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    if ln is not None:
        _chk(ln[3], _lib.operand_dtype(), what + ": ln out")
        if ln[3].numel() < R * D:
            raise _lib.PeekvitHipError(what + ": ln out is smaller than [R, D]")
    null = C.c_void_p(0)
    with _timed("pv_residual_pack_step_train", x.device, 0.0, (12.0 + (2.0 if ln is not None else 0.0)) * x.numel()):
        check(_lib.load().pv_residual_pack_step_train(_ptr(x), _ptr(seg_start), _ptr(mult), _ptr(tok_row), B, N, D, _ptr(wg), _ptr(bg), _ptr(wb), _ptr(bb),
                                                      float(temp), float(sigmoid_bias), _ptr(mask_row), _ptr(x_next), _ptr(rs_next), _ptr(mult_next),
                                                      _ptr(lm_next), _ptr(seg_next), _ptr(tok_next), _ptr(mask_out), _ptr(thr_out), _ptr(totals),
                                                      _ptr(ln[0]) if ln is not None else null, _ptr(ln[1]) if ln is not None else null,
                                                      float(ln[2]) if ln is not None else 0.0, _ptr(ln[3]) if ln is not None else null,
                                                      _ptr(gate_arg), _ptr(src_next), _stream(x)), "pv_residual_pack_step_train")
    _count()


def residual_pack_step_bwd(x: torch.Tensor, seg_start: torch.Tensor, tok_row: torch.Tensor, mask_row: torch.Tensor, gate_arg: torch.Tensor, thr: torch.Tensor,
                           seg_next: torch.Tensor, src_next: torch.Tensor, g_next: torch.Tensor, drow_scale: torch.Tensor, dmask: Optional[torch.Tensor],
                           wg, wb, temp: float):
    """Backward of residual_pack_step_train.  x fp32 [R, D] (the step's input), g_next fp32 [>= R', D] and drow_scale fp32 [>= R'] (gradients of x_next and
    row_scale_next), dmask fp32 [B, N] (gradient of the dense mask) or None.  Returns (dx [R, D], dm_row [R], dwg [D], dbg [1], dwb [D], dbb [1]); the
    parameter gradients are summed over the images by colsum, in a fixed order."""
    what = "residual_pack_step_bwd"
    _chk(x, torch.float32, what + ": x"); _chk(g_next, torch.float32, what + ": g_next"); _chk(drow_scale, torch.float32, what + ": drow_scale")
    R, D = x.shape
    B, N = tok_row.shape
    dev = x.device
    for t, name, n in ((seg_start, "seg_start", B + 1), (tok_row, "tok_row", B * N), (seg_next, "seg_next", B + 1), (src_next, "src_next", 1)):
        _chk(t, torch.int32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    for t, name, n in ((mask_row, "mask_row", R), (gate_arg, "gate_arg", R), (thr, "thr", B)):
        _chk(t, torch.float32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    if g_next.dim() != 2 or g_next.shape[1] != D or drow_scale.numel() < g_next.shape[0] or src_next.numel() < g_next.shape[0]:
        raise _lib.PeekvitHipError(f"{what}: g_next {tuple(g_next.shape)}, drow_scale {tuple(drow_scale.shape)}, src_next {tuple(src_next.shape)} for D = {D}")
    if dmask is not None:
        _chk(dmask, torch.float32, what + ": dmask")
        if dmask.numel() != B * N:
            raise _lib.PeekvitHipError(f"{what}: dmask must hold {B * N} values")
    dx = torch.empty_like(x)
    dm_row = torch.empty((R,), dtype=torch.float32, device=dev)
    dwg_p = torch.empty((B, D), dtype=torch.float32, device=dev)
    dwb_p = torch.empty((B, D), dtype=torch.float32, device=dev)
    scal_p = torch.empty((B, 4), dtype=torch.float32, device=dev)          # (dbg, dbb, 0, 0): four columns for pv_colsum_f32's 16-byte loads
    with _timed("pv_residual_pack_step_bwd", dev, 0.0, 4.0 * (x.numel() + 2.0 * g_next.numel())):
        check(_lib.load().pv_residual_pack_step_bwd(_ptr(x), _ptr(seg_start), _ptr(tok_row), _ptr(mask_row), _ptr(gate_arg), _ptr(thr), _ptr(seg_next),
                                                    _ptr(src_next), _ptr(g_next), _ptr(drow_scale), _ptr(dmask), B, N, D, _ptr(wg), _ptr(wb), float(temp),
                                                    _ptr(dx), _ptr(dm_row), _ptr(dwg_p), _ptr(dwb_p), _ptr(scal_p), _stream(x)), "pv_residual_pack_step_bwd")
    _count()
    dwg = colsum(dwg_p, torch.empty((D,), dtype=torch.float32, device=dev))
    dwb = colsum(dwb_p, torch.empty((D,), dtype=torch.float32, device=dev))
    scal = colsum(scal_p, torch.empty((4,), dtype=torch.float32, device=dev))
    return dx, dm_row, dwg, scal[0:1], dwb, scal[1:2]


# ------------------------------------------------------------------------------------------------
# ResidualViT training on the packed rows past 208 rows per image (include/peekvit_hip_sparse_long_train.h): the four ops
# above for row segments of up to SPARSE_LONG_MAX_LEN rows - the same arguments, shape checks, results and launch counts
# ------------------------------------------------------------------------------------------------
def attention_varlen_w_stream_lse(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, seg_start: torch.Tensor, log_mult: torch.Tensor, max_len: int, H: int,
                                  dh: int):
    """attention_varlen_w_stream that also writes the rows' statistics lse fp32 [R, H] (attention_varlen_w_lse's definition: either forward feeds either
    backward); `out` has attention_varlen_w_stream's bits."""
    what = "attention_varlen_w_stream_lse"
    R, B = _chk_ragged(qkv, seg_start, log_mult, H, dh, what, out=out)
    _chk(lse, torch.float32, what + ": lse")
    if lse.numel() != R * H or lse.device != qkv.device:
        raise _lib.PeekvitHipError(f"{what}: lse must hold {R * H} values on {qkv.device}")
    with _timed("pv_attention_varlen_w_stream_lse_bf16", qkv.device, 4.0 * H * R * max_len * dh, 8.0 * R * H * dh + 4.0 * R * H):
        check(_lib.load().pv_attention_varlen_w_stream_lse_bf16(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(seg_start), _ptr(log_mult), B, int(max_len), H, dh,
                                                                _attn_flag(qkv.device), _stream(qkv)), "pv_attention_varlen_w_stream_lse_bf16")
    _count()
    return out


def attention_varlen_w_stream_bwd16(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, seg_start: torch.Tensor,
                                    log_mult: torch.Tensor, dqkv16: torch.Tensor, max_len: int, H: int, dh: int, qscale: float,
                                    dbias_partial: Optional[torch.Tensor] = None, delta_ws: Optional[torch.Tensor] = None):
    """attention_varlen_w_bwd16 for max_len up to 4096: the same arguments and results (bit for bit up to 208); the dQ launch looks for a weighted key over
    the whole segment."""
    what = "attention_varlen_w_stream_bwd16"
    R, B = _chk_ragged(qkv, seg_start, log_mult, H, dh, what, dout=dout, out=out)
    dev, D3 = qkv.device, 3 * H * dh
    _chk(lse, torch.float32, what + ": lse"); _chk(dqkv16, _lib.operand_dtype(), what + ": dqkv16")
    if lse.numel() != R * H or dqkv16.numel() != R * D3 or dqkv16.device != dev or lse.device != dev:
        raise _lib.PeekvitHipError(f"{what}: lse must hold {R * H} and dqkv16 {R * D3} values on {dev}")
    nb = (int(max_len) + 63) // 64
    if dbias_partial is not None:
        _chk(dbias_partial, torch.float32, what + ": dbias_partial")
        if dbias_partial.numel() != B * nb * D3 or dbias_partial.device != dev:
            raise _lib.PeekvitHipError(what + ": dbias_partial must hold B * ceil(max_len / 64) * 3 * H * dh values on qkv's device")
    if delta_ws is None:
        delta_ws = torch.empty((R, H), dtype=torch.float32, device=dev)
    else:
        _chk(delta_ws, torch.float32, what + ": delta_ws")
        if delta_ws.numel() != R * H or delta_ws.device != dev:
            raise _lib.PeekvitHipError(what + ": delta_ws must hold R * H values on qkv's device")
    with _timed("pv_attention_varlen_w_stream_bwd16_bf16", dev, 14.0 * H * R * max_len * dh, 14.0 * R * H * dh + 12.0 * R * H):
        check(_lib.load().pv_attention_varlen_w_stream_bwd16_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(seg_start), _ptr(log_mult), _ptr(dqkv16),
                                                                  _ptr(dbias_partial), _ptr(delta_ws), B, int(max_len), H, dh, float(qscale), _stream(qkv)),
              "pv_attention_varlen_w_stream_bwd16_bf16")
    _count()
    return dqkv16


def residual_pack_step_long_train(x: torch.Tensor, seg_start: torch.Tensor, mult: torch.Tensor, tok_row: torch.Tensor, wg, bg, wb, bb, temp: float,
                                  sigmoid_bias: float, nxt, mask_out: torch.Tensor, thr_out: torch.Tensor, totals: torch.Tensor, mask_row: torch.Tensor,
                                  gate_arg: torch.Tensor, src_next: torch.Tensor, ln=None):
    """residual_pack_step_train for images of up to 4096 rows (pv_residual_pack_step_long_train): the same arguments and results."""
    what = "residual_pack_step_long_train"
    _chk(x, torch.float32, what + ": x")
    R, D = x.shape
    B, N = tok_row.shape
    x_next, rs_next, mult_next, lm_next, seg_next, tok_next = nxt
    for t, name, n in ((seg_start, "seg_start", B + 1), (mult, "mult", R), (tok_row, "tok_row", B * N), (mult_next, "mult_next", R),
                       (seg_next, "seg_next", B + 1), (tok_next, "tok_row_next", B * N), (totals, "totals", 2), (src_next, "src_next", R)):
        _chk(t, torch.int32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    for t, name, n in ((x_next, "x_next", R * D), (rs_next, "row_scale_next", R), (lm_next, "log_mult_next", R), (mask_out, "mask_out", B * N),
                       (thr_out, "thr_out", B), (mask_row, "mask_row", R), (gate_arg, "gate_arg", R)):
        _chk(t, torch.float32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    if ln is not None:
        _chk(ln[3], _lib.operand_dtype(), what + ": ln out")
        if ln[3].numel() < R * D:
            raise _lib.PeekvitHipError(what + ": ln out is smaller than [R, D]")
    null = C.c_void_p(0)
    with _timed("pv_residual_pack_step_long_train", x.device, 0.0, (12.0 + (2.0 if ln is not None else 0.0)) * x.numel()):
        check(_lib.load().pv_residual_pack_step_long_train(_ptr(x), _ptr(seg_start), _ptr(mult), _ptr(tok_row), B, N, D, _ptr(wg), _ptr(bg), _ptr(wb),
                                                           _ptr(bb), float(temp), float(sigmoid_bias), _ptr(mask_row), _ptr(x_next), _ptr(rs_next),
                                                           _ptr(mult_next), _ptr(lm_next), _ptr(seg_next), _ptr(tok_next), _ptr(mask_out), _ptr(thr_out),
                                                           _ptr(totals), _ptr(ln[0]) if ln is not None else null, _ptr(ln[1]) if ln is not None else null,
                                                           float(ln[2]) if ln is not None else 0.0, _ptr(ln[3]) if ln is not None else null,
                                                           _ptr(gate_arg), _ptr(src_next), _stream(x)), "pv_residual_pack_step_long_train")
    _count()


def residual_pack_step_long_bwd(x: torch.Tensor, seg_start: torch.Tensor, tok_row: torch.Tensor, mask_row: torch.Tensor, gate_arg: torch.Tensor,
                                thr: torch.Tensor, seg_next: torch.Tensor, src_next: torch.Tensor, g_next: torch.Tensor, drow_scale: torch.Tensor,
                                dmask: Optional[torch.Tensor], wg, wb, temp: float):
    """residual_pack_step_bwd for images of up to 4096 rows (pv_residual_pack_step_long_bwd): the same arguments and results."""
    what = "residual_pack_step_long_bwd"
    _chk(x, torch.float32, what + ": x"); _chk(g_next, torch.float32, what + ": g_next"); _chk(drow_scale, torch.float32, what + ": drow_scale")
    R, D = x.shape
    B, N = tok_row.shape
    dev = x.device
    for t, name, n in ((seg_start, "seg_start", B + 1), (tok_row, "tok_row", B * N), (seg_next, "seg_next", B + 1), (src_next, "src_next", 1)):
        _chk(t, torch.int32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    for t, name, n in ((mask_row, "mask_row", R), (gate_arg, "gate_arg", R), (thr, "thr", B)):
        _chk(t, torch.float32, f"{what}: {name}")
        if t.numel() < n:
            raise _lib.PeekvitHipError(f"{what}: {name} holds {t.numel()} elements, needs {n}")
    if g_next.dim() != 2 or g_next.shape[1] != D or drow_scale.numel() < g_next.shape[0] or src_next.numel() < g_next.shape[0]:
        raise _lib.PeekvitHipError(f"{what}: g_next {tuple(g_next.shape)}, drow_scale {tuple(drow_scale.shape)}, src_next {tuple(src_next.shape)} for D = {D}")
    if dmask is not None:
        _chk(dmask, torch.float32, what + ": dmask")
        if dmask.numel() != B * N:
            raise _lib.PeekvitHipError(f"{what}: dmask must hold {B * N} values")
    dx = torch.empty_like(x)
    dm_row = torch.empty((R,), dtype=torch.float32, device=dev)
    dwg_p = torch.empty((B, D), dtype=torch.float32, device=dev)
    dwb_p = torch.empty((B, D), dtype=torch.float32, device=dev)
    scal_p = torch.empty((B, 4), dtype=torch.float32, device=dev)          # (dbg, dbb, 0, 0): four columns for pv_colsum_f32's 16-byte loads
    with _timed("pv_residual_pack_step_long_bwd", dev, 0.0, 4.0 * (x.numel() + 2.0 * g_next.numel())):
        check(_lib.load().pv_residual_pack_step_long_bwd(_ptr(x), _ptr(seg_start), _ptr(tok_row), _ptr(mask_row), _ptr(gate_arg), _ptr(thr), _ptr(seg_next),
                                                         _ptr(src_next), _ptr(g_next), _ptr(drow_scale), _ptr(dmask), B, N, D, _ptr(wg), _ptr(wb),
                                                         float(temp), _ptr(dx), _ptr(dm_row), _ptr(dwg_p), _ptr(dwb_p), _ptr(scal_p), _stream(x)),
              "pv_residual_pack_step_long_bwd")
    _count()
    dwg = colsum(dwg_p, torch.empty((D,), dtype=torch.float32, device=dev))
    dwb = colsum(dwb_p, torch.empty((D,), dtype=torch.float32, device=dev))
    scal = colsum(scal_p, torch.empty((4,), dtype=torch.float32, device=dev))
    return dx, dm_row, dwg, scal[0:1], dwb, scal[1:2]


# ------------------------------------------------------------------------------------------------
# routed top-1 mixture of experts (include/peekvit_hip_moe.h)
# ------------------------------------------------------------------------------------------------
MOE_TILE_ROWS = 256


def moe_packed_rows(M: int, E: int) -> int:
    """Worst-case packed row count of pv_moe_route for M rows and E experts ((ceil(M / 256) + E) * 256)."""
    n = int(_lib.load().pv_moe_packed_rows(int(M), int(E)))
    if n < 0:
        check(n, "pv_moe_packed_rows")
    return n


def moe_route(x: torch.Tensor, gamma, beta, eps: float, gate_w, gate_b, expert: torch.Tensor, seg: torch.Tensor, perm: torch.Tensor,
              tile_expert: torch.Tensor, xln: Optional[torch.Tensor] = None, gap: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None):
    """Routing of one MoE layer over the rows of x fp32 [M, D] (include/peekvit_hip_moe.h pv_moe_route): LayerNorm, fp32 gate, argmax; expert
    int32 [M], seg int32 [E+1], perm int32 [M_pad], tile_expert int32 [M_pad / 256], optional xln 16-bit [M_pad, D] (packed LayerNorm rows),
    gap fp32 [M], probs fp32 [M, E].  M_pad = moe_packed_rows(M, E)."""
    _chk(x, torch.float32, "x")
    D = x.shape[-1]
    M = x.numel() // D
    E = gate_w.shape[0]
    for t, name in ((expert, "expert"), (seg, "seg"), (perm, "perm"), (tile_expert, "tile_expert")):
        _chk(t, torch.int32, name)
    nbytes = int(_lib.load().pv_moe_route_scratch_size(M, E))
    if nbytes < 0:
        check(nbytes, "pv_moe_route_scratch_size")
    scratch = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=x.device)
    with _timed("pv_moe_route", x.device, 2.0 * M * D * E, 8.0 * M * D + 2.0 * perm.numel() * D):
        check(_lib.load().pv_moe_route(_ptr(x), D, M, D, _ptr(gamma), _ptr(beta), float(eps), _ptr(gate_w), _ptr(gate_b), E, _ptr(expert), _ptr(gap),
                                       _ptr(probs), _ptr(seg), _ptr(perm), _ptr(tile_expert), _ptr(xln), _ptr(scratch), nbytes, _stream(x)), "pv_moe_route")
    _count()
    return expert


def gemm_grouped(a: torch.Tensor, w: torch.Tensor, bias, out: torch.Tensor, epilogue: int, tile_expert: torch.Tensor, *, res=None, perm=None):
    """Grouped GEMM over packed rows (include/peekvit_hip_moe.h pv_gemm_grouped_bf16): a 16-bit [M_pad, K] packed rows, w 16-bit [E, N, K]
    stacked expert weights, bias fp32 [E, N].  PV_EPI_BIAS_GELU_BF16: out 16-bit [M_pad, N] in packed order.  PV_EPI_BIAS_RES_F32: out / res
    fp32 [rows, N] addressed through perm int32 [M_pad] (pad rows -1: not written)."""
    E, N, K = w.shape
    Mp = a.shape[0]
    range_flag = current_range_flag()
    args = GemmArgs(A=a.data_ptr(), W=w.data_ptr(), bias=bias.data_ptr() if bias is not None else 0, out=out.data_ptr(),
                    res=res.data_ptr() if res is not None else 0, M=Mp, N=N, K=K, lda=a.stride(0), ldw=w.stride(1), ldo=out.stride(0),
                    ldr=res.stride(0) if res is not None else 0, qscale=1.0, epilogue=epilogue,
                    range_flag=range_flag.data_ptr() if range_flag is not None and range_flag.device == a.device else 0)
    rows = out.shape[0] if res is not None else 0
    nbytes = 2.0 * (Mp * K + E * N * K) + out.element_size() * Mp * N * (2 if res is not None else 1)
    with _timed("pv_gemm_grouped_bf16", a.device, 2.0 * Mp * N * K, nbytes, member=(N, K, epilogue)):
        check(_lib.load().pv_gemm_grouped_bf16(C.byref(args), _ptr(tile_expert), Mp // MOE_TILE_ROWS, E, w.stride(0), _ptr(perm), rows, _stream(a)),
              "pv_gemm_grouped_bf16")
    _count()
    return out


def moe_gather(src: torch.Tensor, expert: torch.Tensor, perm: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[p] = src[expert[perm[p]], perm[p]] (zeros where perm[p] < 0): src 16-bit [E, M, D] per-expert planes, out 16-bit [M_pad, D]
    (include/peekvit_hip_moe.h pv_moe_gather_bf16)."""
    E, M, D = src.shape
    _chk(expert, torch.int32, "expert"); _chk(perm, torch.int32, "perm")
    with _timed("pv_moe_gather_bf16", src.device, 0.0, 4.0 * out.numel()):
        check(_lib.load().pv_moe_gather_bf16(_ptr(src), src.stride(0), src.stride(1), _ptr(expert), _ptr(perm), M, out.shape[0], D, E, _ptr(out),
                                             _stream(src)), "pv_moe_gather_bf16")
    _count()
    return out


# ------------------------------------------------------------------------------------------------
# early exit (include/peekvit_hip_ee.h)
# ------------------------------------------------------------------------------------------------
def exit_head(x: torch.Tensor, gamma, beta, eps: float, w: torch.Tensor, b, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One exit head on class row 0 of every image of x fp32 [B, S, D] (pv_exit_head_f32): LayerNorm + fp32 linear -> logits fp32 [B, C],
    bit-identical to cls_pool(num_cls = 1) followed by head()."""
    _chk(x, torch.float32, "x")
    B, S, D = x.shape
    Cn = w.shape[0]
    for t, name, shape in ((gamma, "gamma", (D,)), (beta, "beta", (D,)), (w, "w", (Cn, D))) + (((b, "b", (Cn,)),) if b is not None else ()):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise _lib.PeekvitHipError(f"exit_head: {name} is {tuple(t.shape)}, expected {shape}")
    if out is None:
        out = torch.empty((B, Cn), dtype=torch.float32, device=x.device)
    else:
        _chk(out, torch.float32, "out")
        if tuple(out.shape) != (B, Cn):
            raise _lib.PeekvitHipError(f"exit_head: out is {tuple(out.shape)}, expected {(B, Cn)}")
    with _timed("pv_exit_head_f32", x.device, 2.0 * B * D * Cn, 4.0 * (B * D + Cn * D + B * Cn)):
        check(_lib.load().pv_exit_head_f32(_ptr(x), S * D, _ptr(gamma), _ptr(beta), float(eps), _ptr(w), _ptr(b), _ptr(out), B, D, Cn, _stream(x)),
              "pv_exit_head_f32")
    _count()
    return out


def exit_step(logits: torch.Tensor, live: torch.Tensor, threshold: float, layer: int, out_logits: torch.Tensor, out_layer: torch.Tensor,
              out_conf: torch.Tensor, count: Optional[torch.Tensor] = None):
    """Exit decision of one checked layer (pv_exit_step): logits fp32 [n_live, C] of the live images, live int32 [n_live] their original
    indices (ascending).  Rows with max softmax >= threshold write out_logits fp32 [B, C] / out_layer int64 [B] / out_conf fp32 [B] at their
    original index.  Returns (row_conf fp32 [n_live], next_live int32 [n_live], src_row int32 [n_live], count int32 [1]); the first
    count entries of next_live / src_row describe the survivors, in ascending original index."""
    _chk(logits, torch.float32, "logits"); _chk(live, torch.int32, "live")
    _chk(out_logits, torch.float32, "out_logits"); _chk(out_layer, torch.int64, "out_layer"); _chk(out_conf, torch.float32, "out_conf")
    n, Cn = logits.shape
    Bt = out_logits.shape[0]
    if live.numel() != n or out_logits.shape[1] != Cn or out_layer.numel() != Bt or out_conf.numel() != Bt:
        raise _lib.PeekvitHipError("exit_step: shapes of live / out_logits / out_layer / out_conf do not match")
    dev = logits.device
    row_conf = torch.empty((n,), dtype=torch.float32, device=dev)
    next_live = torch.empty((n,), dtype=torch.int32, device=dev)
    src_row = torch.empty((n,), dtype=torch.int32, device=dev)
    if count is None:
        count = torch.empty((1,), dtype=torch.int32, device=dev)
    else:
        _chk(count, torch.int32, "count")
    with _timed("pv_exit_step", dev, 0.0, 4.0 * n * Cn):
        check(_lib.load().pv_exit_step(_ptr(logits), Cn, _ptr(live), n, Cn, float(threshold), int(layer), _ptr(row_conf), _ptr(out_logits), Cn,
                                       _ptr(out_layer), _ptr(out_conf), Bt, _ptr(next_live), _ptr(src_row), _ptr(count), _stream(logits)),
              "pv_exit_step")
    _count()
    return row_conf, next_live, src_row, count


def gather_images(x: torch.Tensor, src_row: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[j] = x[src_row[j]] over whole images (pv_gather_images_f32): x fp32 [n_in, ...], src_row int32 [n_out]."""
    _chk(x, torch.float32, "x"); _chk(src_row, torch.int32, "src_row")
    n_out = src_row.numel()
    elems = x.numel() // x.shape[0]
    if out is None:
        out = torch.empty((n_out,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    else:
        _chk(out, torch.float32, "out")
        if tuple(out.shape) != (n_out,) + tuple(x.shape[1:]):
            raise _lib.PeekvitHipError(f"gather_images: out is {tuple(out.shape)}, expected {(n_out,) + tuple(x.shape[1:])}")
    with _timed("pv_gather_images_f32", x.device, 0.0, 8.0 * n_out * elems):
        check(_lib.load().pv_gather_images_f32(_ptr(x), x.shape[0], _ptr(src_row), n_out, elems, _ptr(out), _stream(x)), "pv_gather_images_f32")
    _count()
    return out


# ------------------------------------------------------------------------------------------------
# point-cloud transformer (include/peekvit_hip_pct.h)
# ------------------------------------------------------------------------------------------------
def arpe_embed(points: torch.Tensor, w1, b1, bn1_scale, bn1_shift, w2, b2, bn2_scale, bn2_shift, k: int, tokens: Optional[torch.Tensor] = None,
               row_off: int = 0, idx_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ARPE stem in one launch (pv_arpe_embed): points fp32 [B, N, 3] -> rows [row_off, row_off + N) of tokens fp32 [B, S, D].  w1 [6, 6],
    b1 / bn1_scale / bn1_shift [6], w2 [D, 6], b2 / bn2_scale / bn2_shift [D], all fp32 (BatchNorm at eval as scale and shift).
    idx_out int32 [B, N, k], optional: every query's k nearest neighbours in ascending index order."""
    _chk(points, torch.float32, "points")
    if points.dim() != 3 or points.shape[2] != 3:
        raise _lib.PeekvitHipError(f"arpe_embed: points is {tuple(points.shape)}, expected [B, N, 3]")
    B, N, _ = points.shape
    D = w2.shape[0]
    for t, name, shape in ((w1, "w1", (6, 6)), (b1, "b1", (6,)), (bn1_scale, "bn1_scale", (6,)), (bn1_shift, "bn1_shift", (6,)), (w2, "w2", (D, 6)),
                           (b2, "b2", (D,)), (bn2_scale, "bn2_scale", (D,)), (bn2_shift, "bn2_shift", (D,))):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise _lib.PeekvitHipError(f"arpe_embed: {name} is {tuple(t.shape)}, expected {shape}")
    if tokens is None:
        tokens = torch.empty((B, row_off + N, D), dtype=torch.float32, device=points.device)
    _chk(tokens, torch.float32, "tokens")
    if tokens.dim() != 3 or tokens.shape[0] != B or tokens.shape[2] != D:
        raise _lib.PeekvitHipError(f"arpe_embed: tokens is {tuple(tokens.shape)}, expected [{B}, S, {D}]")
    if idx_out is not None:
        _chk(idx_out, torch.int32, "idx_out")
        if tuple(idx_out.shape) != (B, N, k):
            raise _lib.PeekvitHipError(f"arpe_embed: idx_out is {tuple(idx_out.shape)}, expected {(B, N, k)}")
    with _timed("pv_arpe_embed", points.device, 8.0 * B * N * N + 2.0 * B * N * (36.0 * k + 6.0 * D), 12.0 * B * N + 4.0 * B * N * D):
        check(_lib.load().pv_arpe_embed(_ptr(points), _ptr(w1), _ptr(b1), _ptr(bn1_scale), _ptr(bn1_shift), _ptr(w2), _ptr(b2), _ptr(bn2_scale),
                                        _ptr(bn2_shift), _ptr(tokens), _ptr(idx_out), B, N, int(k), D, tokens.shape[1], int(row_off), _stream(points)),
              "pv_arpe_embed")
    _count()
    return tokens


def layernorm_f32_bf16(x: torch.Tensor, gamma, beta, eps: float, out16: torch.Tensor, out32: torch.Tensor):
    """LayerNorm of the rows of x fp32 [..., D] (last stride 1, one row stride) into BOTH out16 (the operand type, contiguous: bit-identical to
    layernorm_bf16's) and out32 fp32 (contiguous: the values before that rounding) - pv_layernorm_f32_bf16."""
    D = x.shape[-1]
    if x.dtype != torch.float32 or not x.is_cuda or x.stride(-1) != 1:
        raise _lib.PeekvitHipError("layernorm_f32_bf16: x must be an fp32 GPU tensor with unit column stride")
    x2 = x if x.dim() == 2 else x.reshape(-1, D) if x.is_contiguous() else None
    if x2 is None:
        raise _lib.PeekvitHipError("layernorm_f32_bf16: a strided x must be 2-D")
    rows, ldx = x2.shape[0], (x2.stride(0) if x2.shape[0] > 1 else max(x2.stride(0), D))
    _chk(out16, _lib.operand_dtype(), "out16"); _chk(out32, torch.float32, "out32")
    if out16.numel() != rows * D or out32.numel() != rows * D:
        raise _lib.PeekvitHipError("layernorm_f32_bf16: out16 / out32 must hold rows * D values")
    with _timed("pv_layernorm_f32_bf16", x.device, 0.0, 10.0 * rows * D):
        check(_lib.load().pv_layernorm_f32_bf16(_ptr(x2), ldx, _ptr(gamma), _ptr(beta), _ptr(out16), _ptr(out32), D, rows, D, float(eps), _stream(x)),
              "pv_layernorm_f32_bf16")
    _count()
    return out16, out32


def mean_pool(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pooled[b, :] = mean over the rows of x[b] (pv_mean_pool_f32): x fp32 [B, S, D] -> fp32 [B, D], deterministic."""
    _chk(x, torch.float32, "x")
    B, S, D = x.shape
    if out is None:
        out = torch.empty((B, D), dtype=torch.float32, device=x.device)
    else:
        _chk(out, torch.float32, "out")
        if tuple(out.shape) != (B, D):
            raise _lib.PeekvitHipError(f"mean_pool: out is {tuple(out.shape)}, expected {(B, D)}")
    with _timed("pv_mean_pool_f32", x.device, 1.0 * B * S * D, 4.0 * B * S * D):
        check(_lib.load().pv_mean_pool_f32(_ptr(x), _ptr(out), B, S, D, _stream(x)), "pv_mean_pool_f32")
    _count()
    return out


def pct_head(pooled: torch.Tensor, w1, b1, bn_scale, bn_shift, w2, b2) -> torch.Tensor:
    """logits = w2 . gelu(bn_scale * (w1 . pooled + b1) + bn_shift) + b2 in fp32 (pv_pct_head_f32): pooled [B, D], w1 [Hd, D], w2 [C, Hd]."""
    _chk(pooled, torch.float32, "pooled")
    B, D = pooled.shape
    Hd, Cn = w1.shape[0], w2.shape[0]
    for t, name, shape in ((w1, "w1", (Hd, D)), (bn_scale, "bn_scale", (Hd,)), (bn_shift, "bn_shift", (Hd,)), (w2, "w2", (Cn, Hd))) + \
            (((b1, "b1", (Hd,)),) if b1 is not None else ()) + (((b2, "b2", (Cn,)),) if b2 is not None else ()):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise _lib.PeekvitHipError(f"pct_head: {name} is {tuple(t.shape)}, expected {shape}")
    logits = torch.empty((B, Cn), dtype=torch.float32, device=pooled.device)
    with _timed("pv_pct_head_f32", pooled.device, 2.0 * B * Hd * (D + Cn), 4.0 * (B * D + Hd * D + Cn * Hd + B * Cn)):
        check(_lib.load().pv_pct_head_f32(_ptr(pooled), _ptr(w1), _ptr(b1), _ptr(bn_scale), _ptr(bn_shift), _ptr(w2), _ptr(b2), _ptr(logits),
                                          B, D, Hd, Cn, _stream(pooled)), "pv_pct_head_f32")
    _count()
    return logits


# ------------------------------------------------------------------------------------------------
# point-cloud stem, training path (include/peekvit_hip_pct_train.h).  The uint16 index arrays of the C ABI are torch.int16 tensors here:
# N <= 4096, so every index is a non-negative int16 as well.
# ------------------------------------------------------------------------------------------------
ARPE_QPB = 64                 # query points per workgroup = per partial row
ARPE_MOMENT_COLS, ARPE_BWD_COLS = 28, 48


def _chk_points(points: torch.Tensor, what: str):
    _chk(points, torch.float32, "points")
    if points.dim() != 3 or points.shape[2] != 3:
        raise _lib.PeekvitHipError(f"{what}: points is {tuple(points.shape)}, expected [B, N, 3]")
    return points.shape[0], points.shape[1]


def _chk_shape(t: torch.Tensor, dtype, name: str, shape, what: str):
    _chk(t, dtype, name)
    if tuple(t.shape) != tuple(shape):
        raise _lib.PeekvitHipError(f"{what}: {name} is {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def arpe_groups(B: int, N: int) -> int:
    """Partial rows of arpe_pair_moments / arpe_pair_bwd: one per 64 query points of an image."""
    return B * ((N + ARPE_QPB - 1) // ARPE_QPB)


def arpe_knn(points: torch.Tensor, k: int, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The k nearest neighbours of every point (pv_arpe_knn): points fp32 [B, N, 3] -> int16 [B, N, k], ascending index order; the neighbours
    arpe_embed chooses."""
    B, N = _chk_points(points, "arpe_knn")
    if idx is None:
        idx = torch.empty((B, N, int(k)), dtype=torch.int16, device=points.device)
    _chk_shape(idx, torch.int16, "idx", (B, N, int(k)), "arpe_knn")
    with _timed("pv_arpe_knn", points.device, 8.0 * B * N * N, 12.0 * B * N + 2.0 * B * N * k):
        check(_lib.load().pv_arpe_knn(_ptr(points), _ptr(idx), B, N, int(k), _stream(points)), "pv_arpe_knn")
    _count()
    return idx


def arpe_pair_moments(points: torch.Tensor, idx: torch.Tensor, shift: torch.Tensor, partial: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Partial first and second moments of the pair features [x_q - shift, x_q - x_j] (pv_arpe_pair_moments): fp32 [G, 28], one row per 64
    query points (6 sums, the 21 products of the upper triangle row by row, one zero)."""
    B, N = _chk_points(points, "arpe_pair_moments")
    _chk(idx, torch.int16, "idx")
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (B, N):
        raise _lib.PeekvitHipError(f"arpe_pair_moments: idx is {tuple(idx.shape)}, expected [{B}, {N}, k]")
    k = idx.shape[2]
    _chk_shape(shift, torch.float32, "shift", (3,), "arpe_pair_moments")
    G = arpe_groups(B, N)
    if partial is None:
        partial = torch.empty((G, ARPE_MOMENT_COLS), dtype=torch.float32, device=points.device)
    _chk_shape(partial, torch.float32, "partial", (G, ARPE_MOMENT_COLS), "arpe_pair_moments")
    with _timed("pv_arpe_pair_moments", points.device, 60.0 * B * N * k, 12.0 * B * N + 2.0 * B * N * k):
        check(_lib.load().pv_arpe_pair_moments(_ptr(points), _ptr(idx), _ptr(shift), _ptr(partial), B, N, k, _stream(points)), "pv_arpe_pair_moments")
    _count()
    return partial


def arpe_pair_max(points: torch.Tensor, idx: torch.Tensor, w1, b1, scale, shift, y: Optional[torch.Tensor] = None,
                  arg: Optional[torch.Tensor] = None):
    """y = elu(scale * z* + shift) fp32 [B, N, 6] and arg int16 [B, N, 6], the neighbour whose z = w1 [x_q, x_q - x_j] + b1 wins each channel
    (pv_arpe_pair_max): the largest z for scale > 0, the smallest for scale < 0, ties and scale == 0 to the lowest index."""
    B, N = _chk_points(points, "arpe_pair_max")
    _chk(idx, torch.int16, "idx")
    if idx.dim() != 3 or tuple(idx.shape[:2]) != (B, N):
        raise _lib.PeekvitHipError(f"arpe_pair_max: idx is {tuple(idx.shape)}, expected [{B}, {N}, k]")
    k = idx.shape[2]
    for t, name, shape in ((w1, "w1", (6, 6)), (b1, "b1", (6,)), (scale, "scale", (6,)), (shift, "shift", (6,))):
        _chk_shape(t, torch.float32, name, shape, "arpe_pair_max")
    if y is None:
        y = torch.empty((B, N, 6), dtype=torch.float32, device=points.device)
    if arg is None:
        arg = torch.empty((B, N, 6), dtype=torch.int16, device=points.device)
    _chk_shape(y, torch.float32, "y", (B, N, 6), "arpe_pair_max")
    _chk_shape(arg, torch.int16, "arg", (B, N, 6), "arpe_pair_max")
    with _timed("pv_arpe_pair_max", points.device, 42.0 * B * N * k, 12.0 * B * N + 2.0 * B * N * k + 36.0 * B * N):
        check(_lib.load().pv_arpe_pair_max(_ptr(points), _ptr(idx), _ptr(w1), _ptr(b1), _ptr(scale), _ptr(shift), _ptr(y), _ptr(arg), B, N, k,
                                           _stream(points)), "pv_arpe_pair_max")
    _count()
    return y, arg


def arpe_pair_bwd(points: torch.Tensor, arg: torch.Tensor, y: torch.Tensor, g: torch.Tensor, w1, b1, partial: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Partial backward sums of the pair stage (pv_arpe_pair_bwd): fp32 [G, 48] = A[6] | Z[6] | C[6, 6] per 64 query points, with
    g' = g * elu'(y): A = sum g', Z = sum g' z*, C = sum g' f* (z*, f* of the winning neighbour arg)."""
    B, N = _chk_points(points, "arpe_pair_bwd")
    _chk_shape(arg, torch.int16, "arg", (B, N, 6), "arpe_pair_bwd")
    _chk_shape(y, torch.float32, "y", (B, N, 6), "arpe_pair_bwd")
    _chk_shape(g, torch.float32, "g", (B, N, 6), "arpe_pair_bwd")
    _chk_shape(w1, torch.float32, "w1", (6, 6), "arpe_pair_bwd")
    _chk_shape(b1, torch.float32, "b1", (6,), "arpe_pair_bwd")
    G = arpe_groups(B, N)
    if partial is None:
        partial = torch.empty((G, ARPE_BWD_COLS), dtype=torch.float32, device=points.device)
    _chk_shape(partial, torch.float32, "partial", (G, ARPE_BWD_COLS), "arpe_pair_bwd")
    with _timed("pv_arpe_pair_bwd", points.device, 200.0 * B * N, 96.0 * B * N):
        check(_lib.load().pv_arpe_pair_bwd(_ptr(points), _ptr(arg), _ptr(y), _ptr(g), _ptr(w1), _ptr(b1), _ptr(partial), B, N, _stream(points)),
              "pv_arpe_pair_bwd")
    _count()
    return partial


# ---- a sorting point-cloud block in train mode (include/peekvit_hip_rank_train.h) --------------------------------------------
def _chk_rank(what: str, dense_shape, k: int, keep: Optional[torch.Tensor], dev):
    """B, S, D, Sc of the row movers: 1 <= k <= S - 1, Sc = k + 1 + (k < S - 1); keep int32 [B, k] on `dev` when given."""
    B, S, D = (int(v) for v in dense_shape)
    if not 1 <= k <= S - 1:
        raise _lib.PeekvitHipError(f"{what}: 1 <= k <= S - 1, got k = {k}, S = {S}")
    if keep is not None:
        _chk(keep, torch.int32, f"{what}: keep")
        if tuple(keep.shape) != (B, k) or keep.device != dev:
            raise _lib.PeekvitHipError(f"{what}: keep must be int32 [{B}, {k}] on {dev}, got {tuple(keep.shape)} on {keep.device}")
    return B, S, D, k + 1 + (1 if k < S - 1 else 0)


def rank_pack(x: torch.Tensor, keep: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 [B, S, D], keep int32 [B, k] (rank_topk's) -> xc fp32 [B, Sc, D]: row 0, the kept rows in keep's order and, when k < S - 1, a zero tail row."""
    _chk(x, torch.float32, "rank_pack: x")
    if x.dim() != 3:
        raise _lib.PeekvitHipError("rank_pack: x must be [B, S, D]")
    B, S, D, Sc = _chk_rank("rank_pack", x.shape, int(keep.shape[-1]), keep, x.device)
    if out is None:
        out = torch.empty((B, Sc, D), dtype=torch.float32, device=x.device)
    _chk(out, torch.float32, "rank_pack: out")
    if out.numel() != B * Sc * D or out.device != x.device:
        raise _lib.PeekvitHipError(f"rank_pack: out must hold {B * Sc * D} values on {x.device}")
    with _timed("pv_rank_pack_f32", x.device, 0.0, 8.0 * B * Sc * D):
        check(_lib.load().pv_rank_pack_f32(_ptr(x), _ptr(keep), _ptr(out), B, S, keep.shape[1], D, _stream(x)), "pv_rank_pack_f32")
    _count()
    return out


def rank_expand(yc: torch.Tensor, S: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """yc fp32 [B, L + 1, D] -> y fp32 [B, S, D] (L < S): the L live rows, then the tail row in every row L .. S - 1."""
    _chk(yc, torch.float32, "rank_expand: yc")
    if yc.dim() != 3 or not 2 <= yc.shape[1] <= S:
        raise _lib.PeekvitHipError(f"rank_expand: yc must be [B, L + 1, D] with 1 <= L < S = {S}, got {tuple(yc.shape)}")
    B, Sc, D = yc.shape
    if out is None:
        out = torch.empty((B, S, D), dtype=torch.float32, device=yc.device)
    _chk(out, torch.float32, "rank_expand: out")
    if out.numel() != B * S * D or out.device != yc.device:
        raise _lib.PeekvitHipError(f"rank_expand: out must hold {B * S * D} values on {yc.device}")
    with _timed("pv_rank_expand_f32", yc.device, 0.0, 4.0 * B * (Sc + S) * D):
        check(_lib.load().pv_rank_expand_f32(_ptr(yc), _ptr(out), B, S, Sc - 1, D, _stream(yc)), "pv_rank_expand_f32")
    _count()
    return out


def rank_reduce(g: torch.Tensor, L: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g fp32 [B, S, D] -> gc fp32 [B, L + 1, D] (1 <= L < S): rows 0 .. L - 1 copied, row L = the sum of rows L .. S - 1 (fixed order, no atomics)."""
    _chk(g, torch.float32, "rank_reduce: g")
    if g.dim() != 3 or not 1 <= L < g.shape[1]:
        raise _lib.PeekvitHipError(f"rank_reduce: g must be [B, S, D] and 1 <= L < S, got {tuple(g.shape)}, L = {L}")
    B, S, D = g.shape
    if out is None:
        out = torch.empty((B, L + 1, D), dtype=torch.float32, device=g.device)
    _chk(out, torch.float32, "rank_reduce: out")
    if out.numel() != B * (L + 1) * D or out.device != g.device:
        raise _lib.PeekvitHipError(f"rank_reduce: out must hold {B * (L + 1) * D} values on {g.device}")
    with _timed("pv_rank_reduce_f32", g.device, 1.0 * B * (S - L) * D, 4.0 * B * (S + L + 1) * D):
        check(_lib.load().pv_rank_reduce_f32(_ptr(g), _ptr(out), B, S, L, D, _stream(g)), "pv_rank_reduce_f32")
    _count()
    return out


def rank_unpack_grad(dxc: torch.Tensor, keep: torch.Tensor, S: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dxc fp32 [B, Sc, D], keep int32 [B, k] -> dx fp32 [B, S, D]: row 0 and the kept rows scattered back, zeros elsewhere (every row written)."""
    _chk(dxc, torch.float32, "rank_unpack_grad: dxc")
    if dxc.dim() != 3:
        raise _lib.PeekvitHipError("rank_unpack_grad: dxc must be [B, Sc, D]")
    B, _, D, Sc = _chk_rank("rank_unpack_grad", (dxc.shape[0], S, dxc.shape[2]), int(keep.shape[-1]), keep, dxc.device)
    if dxc.shape[1] != Sc:
        raise _lib.PeekvitHipError(f"rank_unpack_grad: dxc must have {Sc} rows per image, got {dxc.shape[1]}")
    if out is None:
        out = torch.empty((B, S, D), dtype=torch.float32, device=dxc.device)
    _chk(out, torch.float32, "rank_unpack_grad: out")
    if out.numel() != B * S * D or out.device != dxc.device:
        raise _lib.PeekvitHipError(f"rank_unpack_grad: out must hold {B * S * D} values on {dxc.device}")
    with _timed("pv_rank_unpack_grad_f32", dxc.device, 0.0, 4.0 * B * (Sc + S) * D):
        check(_lib.load().pv_rank_unpack_grad_f32(_ptr(dxc), _ptr(keep), _ptr(out), B, S, keep.shape[1], D, _stream(dxc)), "pv_rank_unpack_grad_f32")
    _count()
    return out


def _chk_row_scale(row_scale: torch.Tensor, rows: int, dev, what: str):
    _chk(row_scale, torch.float32, f"{what}: row_scale")
    if row_scale.numel() != rows or row_scale.device != dev:
        raise _lib.PeekvitHipError(f"{what}: row_scale must hold {rows} values on {dev}")


def layernorm_f32_bf16_masked(x: torch.Tensor, gamma, beta, row_scale: torch.Tensor, eps: float, out16: torch.Tensor, out32: torch.Tensor):
    """layernorm_f32_bf16 on contiguous rows with BOTH planes multiplied by row_scale[row] (fp32 [rows]): 1 changes no bit, 0 leaves zeros."""
    _chk(x, torch.float32, "layernorm_f32_bf16_masked: x")
    D = x.shape[-1]
    rows = x.numel() // D
    _chk(out16, _lib.operand_dtype(), "layernorm_f32_bf16_masked: out16"); _chk(out32, torch.float32, "layernorm_f32_bf16_masked: out32")
    _chk_row_scale(row_scale, rows, x.device, "layernorm_f32_bf16_masked")
    if out16.numel() != rows * D or out32.numel() != rows * D or out16.device != x.device or out32.device != x.device:
        raise _lib.PeekvitHipError("layernorm_f32_bf16_masked: out16 / out32 must hold rows * D values on x's device")
    with _timed("pv_layernorm_f32_bf16_masked", x.device, 0.0, 10.0 * rows * D):
        check(_lib.load().pv_layernorm_f32_bf16_masked(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(row_scale), _ptr(out16), _ptr(out32), rows, D, float(eps),
                                                       _stream(x)), "pv_layernorm_f32_bf16_masked")
    _count()
    return out16, out32


def layernorm_bwd_sum_masked(x: torch.Tensor, dy16: Optional[torch.Tensor], dy32: Optional[torch.Tensor], gamma: torch.Tensor, row_scale: torch.Tensor,
                             dx_out: Optional[torch.Tensor], dx16: Optional[torch.Tensor], dgb: torch.Tensor, eps: float, accumulate: bool = False):
    """layernorm_bwd_sum for y = row_scale[row] * LN(x): the summed dy is multiplied by row_scale[row] (fp32 [rows]), so a row with scale 0 gives
    dx = 0 and adds nothing to dgamma / dbeta; a scale of 1 changes no bit."""
    what = "layernorm_bwd_sum_masked"
    _chk(x, torch.float32, what + ": x"); _chk(dgb, torch.float32, what + ": dgb"); _chk(gamma, torch.float32, what + ": gamma")
    if (dy16 is None and dy32 is None) or (dx_out is None and dx16 is None):
        raise _lib.PeekvitHipError(what + ": one of dy16 / dy32 and one of dx_out / dx16 must be given")
    D = x.shape[-1]
    rows = x.numel() // D
    _chk_row_scale(row_scale, rows, x.device, what)
    for name, t, dtype in (("dy16", dy16, _lib.operand_dtype()), ("dy32", dy32, torch.float32), ("dx_out", dx_out, torch.float32), ("dx16", dx16, _lib.operand_dtype())):
        if t is not None:
            _chk(t, dtype, f"{what}: {name}")
            if t.numel() != rows * D or t.device != x.device:
                raise _lib.PeekvitHipError(f"{what}: {name} must hold {rows * D} values on {x.device}")
    if gamma.numel() != D or dgb.numel() != 3 * D:
        raise _lib.PeekvitHipError(what + ": gamma must hold D and dgb 3 * D values")
    ws = _scratch_f32(_lib.PV_WS_LAYERNORM_BWD, x.device, rows, D)
    nb = 4.0 + sum(b for t, b in ((dy16, 2.0), (dy32, 4.0), (dx_out, 4.0), (dx16, 2.0)) if t is not None)
    with _timed("pv_layernorm_bwd_sum_masked", x.device, 0.0, nb * x.numel()):
        check(_lib.load().pv_layernorm_bwd_sum_masked(_ptr(x), _ptr(dy16), _ptr(dy32), _ptr(gamma), _ptr(row_scale), _ptr(dx_out), _ptr(dx16), _ptr(dgb), _ptr(ws),
                                                      ws.numel(), rows, D, float(eps), int(accumulate), _stream(x)), "pv_layernorm_bwd_sum_masked")
    _count()
    return dx_out if dx_out is not None else dx16


def _chk_tail_log_mult(t: float, what: str) -> float:
    t = float(t)
    if not (0.0 <= t < float("inf")):
        raise _lib.PeekvitHipError(f"{what}: tail_log_mult must be finite and >= 0, got {t}")
    return t


def attention_stream_w(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, B: int, S: int, H: int, dh: int, tail_log_mult: float):
    """attention_stream where key S - 1 of every image stands for exp(tail_log_mult) identical keys: the bias is added to its scores in fp32 (lse includes
    it).  tail_log_mult = 0 gives attention_stream's bits."""
    _chk_attn_stream(qkv, B, S, H, dh, "attention_stream_w", out=out, lse=lse)
    t = _chk_tail_log_mult(tail_log_mult, "attention_stream_w")
    with _timed("pv_attention_stream_lse_w_bf16", qkv.device, 4.0 * B * H * S * S * dh, 8.0 * B * S * H * dh + 4.0 * B * H * S):
        check(_lib.load().pv_attention_stream_lse_w_bf16(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, dh, t, _attn_flag(qkv.device), _stream(qkv)),
              "pv_attention_stream_lse_w_bf16")
    _count()
    return out


def attention_stream_bwd16_w(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dqkv16: torch.Tensor, B: int, S: int, H: int, dh: int,
                             qscale: float, tail_log_mult: float, dbias_partial: Optional[torch.Tensor] = None, delta_ws: Optional[torch.Tensor] = None):
    """attention_stream_bwd16 for attention_stream_w's forward (the same tail_log_mult): row S - 1 of the k | v thirds is the gradient of the shared key, the
    sum over the keys it stands for."""
    what = "attention_stream_bwd16_w"
    _chk_attn_stream(qkv, B, S, H, dh, what, dout=dout, out=out, lse=lse)
    t = _chk_tail_log_mult(tail_log_mult, what)
    dev, D3 = qkv.device, 3 * H * dh
    _chk(dqkv16, _lib.operand_dtype(), what + ": dqkv16")
    if dqkv16.numel() != B * S * D3 or dqkv16.device != dev:
        raise _lib.PeekvitHipError(f"{what}: dqkv16 must hold {B * S * D3} values on {dev}")
    if dbias_partial is not None:
        _chk(dbias_partial, torch.float32, what + ": dbias_partial")
        if dbias_partial.numel() != B * ((S + 63) // 64) * D3 or dbias_partial.device != dev:
            raise _lib.PeekvitHipError(what + ": dbias_partial must hold B * ceil(S / 64) * 3 * H * dh values on qkv's device")
    if delta_ws is None:
        delta_ws = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    else:
        _chk(delta_ws, torch.float32, what + ": delta_ws")
        if delta_ws.numel() != B * H * S or delta_ws.device != dev:
            raise _lib.PeekvitHipError(what + ": delta_ws must hold B * H * S values on qkv's device")
    with _timed("pv_attention_stream_bwd16_w_bf16", dev, 14.0 * B * H * S * S * dh, 14.0 * B * S * H * dh + 12.0 * B * H * S):
        check(_lib.load().pv_attention_stream_bwd16_w_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(dqkv16), _ptr(dbias_partial), _ptr(delta_ws), B, S, H, dh,
                                                           float(qscale), t, _stream(qkv)), "pv_attention_stream_bwd16_w_bf16")
    _count()
    return dqkv16


# ---- a sorting point-cloud block at eval (include/peekvit_hip_rank_infer.h) ---------------------------------------------------
def rank_order(norms: torch.Tensor, k: int, gap_min: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rank_topk by a sort (pv_rank_order_gap): norms fp32 [B, N] -> keep int32 [B, k], the first k indices of the stable descending order (ties to the
    lowest index, NaN above +inf); gap_min (fp32 [B], optional) is lowered to each image's relative gap at the keep boundary.  The bits are rank_topk's."""
    _chk(norms, torch.float32, "rank_order: norms")
    if norms.dim() != 2:
        raise _lib.PeekvitHipError("rank_order: norms must be [B, N]")
    B, N = norms.shape
    if not 0 <= k <= N:
        raise _lib.PeekvitHipError(f"rank_order: 0 <= k <= N, got k = {k}, N = {N}")
    keep = torch.empty((B, k), dtype=torch.int32, device=norms.device)
    if k == 0:                                   # nothing to keep: no launch (and an empty tensor has no address to hand over)
        return keep
    if gap_min is not None:
        _chk(gap_min, torch.float32, "rank_order: gap_min")
        if gap_min.numel() != B or gap_min.device != norms.device:
            raise _lib.PeekvitHipError(f"rank_order: gap_min must hold {B} values on {norms.device}")
    with _timed("pv_rank_order_gap", norms.device, 0.0, 4.0 * (norms.numel() + B * k)):
        check(_lib.load().pv_rank_order_gap(_ptr(norms), _ptr(keep), _ptr(gap_min), B, N, k, _stream(norms)), "pv_rank_order_gap")
    _count()
    return keep


def layernorm_gather_f32_bf16(x: torch.Tensor, keep: torch.Tensor, gamma, beta, eps: float, out16: torch.Tensor, out32: torch.Tensor):
    """layernorm_f32_bf16 of row 0 and the rows 1 + keep[b, j] of every image of x fp32 [B, S, D] (keep int32 [B, k], rank_order's): out16 (the operand
    type) and out32 fp32, both contiguous [B * (1 + k), D] - the bits of gather_tokens followed by layernorm_f32_bf16, without the gathered rows."""
    what = "layernorm_gather_f32_bf16"
    _chk(x, torch.float32, what + ": x")
    if x.dim() != 3:
        raise _lib.PeekvitHipError(what + ": x must be [B, S, D]")
    B, S, D = x.shape
    _chk(keep, torch.int32, what + ": keep")
    if keep.dim() != 2 or keep.shape[0] != B or keep.shape[1] > S - 1 or keep.device != x.device:
        raise _lib.PeekvitHipError(f"{what}: keep must be int32 [{B}, k <= {S - 1}] on {x.device}, got {tuple(keep.shape)} on {keep.device}")
    k = int(keep.shape[1])
    rows = B * (k + 1)
    _chk(out16, _lib.operand_dtype(), what + ": out16"); _chk(out32, torch.float32, what + ": out32")
    if out16.numel() != rows * D or out32.numel() != rows * D or out16.device != x.device or out32.device != x.device:
        raise _lib.PeekvitHipError(what + ": out16 / out32 must hold B * (1 + k) * D values on x's device")
    with _timed("pv_layernorm_gather_f32_bf16", x.device, 0.0, 10.0 * rows * D + 4.0 * B * k):
        check(_lib.load().pv_layernorm_gather_f32_bf16(_ptr(x), _ptr(keep) if k else C.c_void_p(0), _ptr(gamma), _ptr(beta), _ptr(out16), _ptr(out32), B, S, k, D,
                                                       float(eps), _stream(x)), what)
    _count()
    return out16, out32


# ---- A-ViT's halting step in training (include/peekvit_hip_avit_train.h) ---------------------------------------------------------
def _chk_avit(what: str, y: torch.Tensor, acc: torch.Tensor, **state):
    """B, S, D, n_cls of a halting step: y fp32 [B, S, D], acc fp32 [B, n_cls, D], every state tensor fp32 [B, S], all on y's device."""
    _chk(y, torch.float32, what + ": y")
    if y.dim() != 3:
        raise _lib.PeekvitHipError(what + ": y must be [B, S, D]")
    B, S, D = (int(v) for v in y.shape)
    _chk(acc, torch.float32, what + ": acc")
    if acc.dim() != 3 or acc.shape[0] != B or acc.shape[2] != D or not 1 <= acc.shape[1] <= S or acc.device != y.device:
        raise _lib.PeekvitHipError(f"{what}: acc must be fp32 [{B}, n_cls <= {S}, {D}] on {y.device}, got {tuple(acc.shape)} on {acc.device}")
    for name, t in state.items():
        _chk(t, torch.float32, f"{what}: {name}")
        if t.numel() != B * S or t.device != y.device:
            raise _lib.PeekvitHipError(f"{what}: {name} must hold {B * S} values on {y.device}")
    return B, S, D, int(acc.shape[1])


def avit_act_fwd(y: torch.Tensor, c: torch.Tensor, R: torch.Tensor, rho: torch.Tensor, counter: torch.Tensor, m: torch.Tensor, acc: torch.Tensor,
                 gate_scale: float, gate_center: float, threshold: float, last: bool):
    """One A-ViT halting step (pv_avit_act_fwd): y fp32 [B, S, D] becomes the next block's input IN PLACE (halted rows zeroed).  Returns
    ((c', R', rho', counter', m') fp32 [B, S] each, acc' fp32 [B, n_cls, D], h_part fp32 [B] = every image's sum of h, sv fp32 [3, B, S] = (h, w,
    flags) and ycls fp32 [B, n_cls, D] = the class rows of y: the last two are what avit_act_bwd needs)."""
    B, S, D, n_cls = _chk_avit("avit_act_fwd", y, acc, c=c, R=R, rho=rho, counter=counter, m=m)
    dev = y.device
    out = torch.empty((5, B, S), dtype=torch.float32, device=dev)
    acc_out, ycls = torch.empty_like(acc), torch.empty_like(acc)
    h_part = torch.empty((B,), dtype=torch.float32, device=dev)
    sv = torch.empty((3, B, S), dtype=torch.float32, device=dev)
    with _timed("pv_avit_act_fwd", dev, 12.0 * B * S, 4.0 * (14 * B * S + 4 * B * n_cls * D)):
        check(_lib.load().pv_avit_act_fwd(_ptr(y), _ptr(c), _ptr(R), _ptr(rho), _ptr(counter), _ptr(m), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                          _ptr(out[3]), _ptr(out[4]), _ptr(acc), _ptr(acc_out), _ptr(h_part), _ptr(sv), _ptr(ycls), B, S, D, n_cls,
                                          float(gate_scale), float(gate_center), float(threshold), int(bool(last)), _stream(y)), "pv_avit_act_fwd")
    _count()
    return out.unbind(0), acc_out, h_part, sv, ycls


def avit_act_bwd(dy: torch.Tensor, dy16: Optional[torch.Tensor], gR: torch.Tensor, grho: torch.Tensor, gacc: torch.Tensor, gh: Optional[torch.Tensor],
                 sv: torch.Tensor, ycls: torch.Tensor, gate_scale: float, last: bool) -> torch.Tensor:
    """Backward of avit_act_fwd (pv_avit_act_bwd).  dy fp32 [B, S, D]: the gradient of the next block's input on entry, the gradient of y on exit (IN
    PLACE: channel 0 of every row and the class rows change; dy16, the optional 16-bit copy, follows).  gR, grho fp32 [B, S], gacc fp32 [B, n_cls, D],
    gh a one-element fp32 tensor (the layer score's gradient) or None.  Returns dR fp32 [B, S]; the gradients of rho and acc are grho and gacc."""
    B, S, D, n_cls = _chk_avit("avit_act_bwd", dy, gacc, gR=gR, grho=grho)
    _chk(ycls, torch.float32, "avit_act_bwd: ycls"); _chk(sv, torch.float32, "avit_act_bwd: sv")
    if ycls.shape != gacc.shape or sv.numel() != 3 * B * S or ycls.device != dy.device or sv.device != dy.device:
        raise _lib.PeekvitHipError("avit_act_bwd: sv must be [3, B, S] and ycls [B, n_cls, D] on dy's device, as avit_act_fwd returned them")
    if dy16 is not None:
        _chk(dy16, _lib.operand_dtype(), "avit_act_bwd: dy16")
        if dy16.numel() != dy.numel() or dy16.device != dy.device:
            raise _lib.PeekvitHipError("avit_act_bwd: dy16 must be the 16-bit copy of dy")
    if gh is not None:
        _chk(gh, torch.float32, "avit_act_bwd: gh")
        if gh.numel() != 1 or gh.device != dy.device:
            raise _lib.PeekvitHipError("avit_act_bwd: gh must be one fp32 value on dy's device")
    dR = torch.empty((B, S), dtype=torch.float32, device=dy.device)
    with _timed("pv_avit_act_bwd", dy.device, 12.0 * B * S + 4.0 * B * n_cls * D, 4.0 * (8 * B * S + 4 * B * n_cls * D)):
        check(_lib.load().pv_avit_act_bwd(_ptr(dy), _ptr(dy16), _ptr(gR), _ptr(grho), _ptr(gacc), _ptr(gh), _ptr(sv), _ptr(ycls), _ptr(dR), B, S, D, n_cls,
                                          float(gate_scale), int(bool(last)), _stream(dy)), "pv_avit_act_bwd")
    _count()
    return dR


# ---- A-ViT's halting step in training on the packed live rows (include/peekvit_hip_avit_pack_train.h) -----------------------------
def _chk_avit_pack(what: str, y: torch.Tensor, seg_start: torch.Tensor, n_halted: torch.Tensor, pos: torch.Tensor, acc: torch.Tensor, **state):
    """R, D, B, S, n_cls of a packed halting step: y fp32 [R, D], seg_start int32 [B + 1], n_halted int32 [B], pos int32 [>= R], acc fp32 [B, n_cls, D],
    every state tensor fp32 [B, S], all on y's device."""
    _chk(y, torch.float32, what + ": y")
    if y.dim() != 2:
        raise _lib.PeekvitHipError(what + ": y must be [R, D]")
    R, D = (int(v) for v in y.shape)
    dev = y.device
    for t, name in ((seg_start, "seg_start"), (n_halted, "n_halted"), (pos, "pos")):
        _chk(t, torch.int32, f"{what}: {name}")
    B = n_halted.numel()
    _chk(acc, torch.float32, what + ": acc")
    if seg_start.numel() != B + 1 or pos.numel() < R or acc.dim() != 3 or acc.shape[0] != B or acc.shape[2] != D or acc.device != dev:
        raise _lib.PeekvitHipError(f"{what}: seg_start {tuple(seg_start.shape)}, pos {tuple(pos.shape)}, acc {tuple(acc.shape)} for {B} images, y {tuple(y.shape)}")
    S = None
    for name, t in state.items():
        _chk(t, torch.float32, f"{what}: {name}")
        if t.dim() != 2 or t.shape[0] != B or t.device != dev or (S is not None and t.shape[1] != S):
            raise _lib.PeekvitHipError(f"{what}: {name} must be fp32 [{B}, S] on {dev}")
        S = int(t.shape[1])
    return R, D, B, S, int(acc.shape[1])


def avit_pack_step_train(y: torch.Tensor, seg_start: torch.Tensor, n_halted: torch.Tensor, pos: torch.Tensor, c: torch.Tensor, R: torch.Tensor,
                         rho: torch.Tensor, counter: torch.Tensor, m: torch.Tensor, acc: torch.Tensor, gate_scale: float, gate_center: float,
                         threshold: float, last: bool):
    """One A-ViT halting step on the packed block output y fp32 [R, D] (pv_avit_pack_step_train).  Returns ((c', R', rho', counter', m') fp32 [B, S]
    each, acc' fp32 [B, n_cls, D], h_part fp32 [B], sv fp32 [3, R] = (h, w, flags), ycls fp32 [B, n_cls, D], nxt) with nxt = None when `last`, else
    (x_next fp32 [R, D], row_scale_next fp32 [R], seg_next int32 [B + 1], n_halted_next int32 [B], log_mult_next fp32 [R], pos_next int32 [R], totals
    int32 [2] = (R', longest segment), src_next int32 [R]): the first R' rows of the row arrays are written."""
    return _avit_pack_step(lambda *a: _lib.load().pv_avit_pack_step_train(*a), "pv_avit_pack_step_train", "avit_pack_step_train", y, seg_start, n_halted,
                           pos, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last, True)


def avit_pack_step_long(y: torch.Tensor, seg_start: torch.Tensor, n_halted: torch.Tensor, pos: torch.Tensor, c: torch.Tensor, R: torch.Tensor,
                        rho: torch.Tensor, counter: torch.Tensor, m: torch.Tensor, acc: torch.Tensor, gate_scale: float, gate_center: float,
                        threshold: float, last: bool, save: bool = True):
    """avit_pack_step_train for up to AVIT_LONG_MAX_S tokens per image (pv_avit_pack_step_long, include/peekvit_hip_avit_long.h):
    the same arguments and results, bit for bit up to 256 tokens.  `save=False` is the inference step: sv, ycls and nxt[7] (src_next) are None and
    nothing is saved for a backward."""
    return _avit_pack_step(lambda *a: _lib.load().pv_avit_pack_step_long(*a), "pv_avit_pack_step_long", "avit_pack_step_long", y, seg_start, n_halted,
                           pos, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last, save)


AVIT_LONG_MAX_S = 4096              # PV_AVIT_LONG_MAX_S


def _avit_pack_step(run, entry: str, what: str, y, seg_start, n_halted, pos, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last, save):
    """The two packed halting steps behind one set of checks and allocations: `run` calls the library's entry point, `entry` is its name."""
    Rr, D, B, S, n_cls = _chk_avit_pack(what, y, seg_start, n_halted, pos, acc, c=c, R=R, rho=rho, counter=counter, m=m)
    dev, f32, i32 = y.device, torch.float32, torch.int32
    out = torch.empty((5, B, S), dtype=f32, device=dev)
    acc_out = torch.empty_like(acc)
    ycls = torch.empty_like(acc) if save else None
    h_part = torch.empty((B,), dtype=f32, device=dev)
    sv = torch.empty((3, Rr), dtype=f32, device=dev) if save else None
    nxt = None
    if not last:
        nxt = (torch.empty((Rr, D), dtype=f32, device=dev), torch.empty(Rr, dtype=f32, device=dev), torch.empty(B + 1, dtype=i32, device=dev),
               torch.empty(B, dtype=i32, device=dev), torch.empty(Rr, dtype=f32, device=dev), torch.empty(Rr, dtype=i32, device=dev),
               torch.empty(2, dtype=i32, device=dev), torch.empty(Rr, dtype=i32, device=dev) if save else None)
    np_ = [_ptr(t) for t in nxt[:7]] if nxt is not None else [C.c_void_p(0)] * 7
    with _timed(entry, dev, 12.0 * B * S, 4.0 * (2.0 * y.numel() + 14 * B * S + 4 * B * n_cls * D)):
        check(run(_ptr(y), _ptr(seg_start), _ptr(n_halted), _ptr(pos), B, S, D, Rr, _ptr(c), _ptr(R), _ptr(rho), _ptr(counter), _ptr(m), _ptr(out[0]),
                  _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(acc), _ptr(acc_out), n_cls, _ptr(h_part), float(gate_scale), float(gate_center),
                  float(threshold), int(bool(last)), *np_, _ptr(sv), _ptr(ycls), _ptr(nxt[7]) if nxt is not None else C.c_void_p(0), _stream(y)), entry)
    _count()
    return out.unbind(0), acc_out, h_part, sv, ycls, nxt


def avit_pack_step_bwd(g_next: Optional[torch.Tensor], seg_start: torch.Tensor, n_halted: torch.Tensor, pos: torch.Tensor, seg_next: Optional[torch.Tensor],
                       src_next: Optional[torch.Tensor], sv: torch.Tensor, ycls: torch.Tensor, gR: torch.Tensor, grho: torch.Tensor, gacc: torch.Tensor,
                       gh: Optional[torch.Tensor], G: torch.Tensor, D: int, gate_scale: float, last: bool, want16: bool = True):
    """Backward of avit_pack_step_train (pv_avit_pack_step_bwd).  g_next fp32 [R', D] (None with `last`, as seg_next and src_next), gR, grho fp32 [B, S],
    gacc fp32 [B, n_cls, D], gh a one-element fp32 tensor or None, G fp32 [B] UPDATED IN PLACE.  Returns (dy fp32 [R, D], its 16-bit copy or None,
    dR fp32 [B, S])."""
    return _avit_pack_bwd(lambda *a: _lib.load().pv_avit_pack_step_bwd(*a), "pv_avit_pack_step_bwd", g_next, seg_start, n_halted, pos, seg_next, src_next, sv,
                          ycls, gR, grho, gacc, gh, G, D, gate_scale, last, want16)


def _avit_pack_bwd(run, entry: str, g_next, seg_start, n_halted, pos, seg_next, src_next, sv, ycls, gR, grho, gacc, gh, G, D, gate_scale, last, want16):
    """The two packed halting backwards behind one set of checks and allocations: `run` calls the library's entry point, `entry` is its name."""
    what = entry[3:]
    for t, name in ((seg_start, "seg_start"), (n_halted, "n_halted"), (pos, "pos")):
        _chk(t, torch.int32, f"{what}: {name}")
    for t, name in ((sv, "sv"), (ycls, "ycls"), (gR, "gR"), (grho, "grho"), (gacc, "gacc"), (G, "G")):
        _chk(t, torch.float32, f"{what}: {name}")
    dev = sv.device
    B = n_halted.numel()
    if sv.dim() != 2 or sv.shape[0] != 3 or gR.dim() != 2 or gR.shape[0] != B or grho.shape != gR.shape or gacc.shape != ycls.shape or gacc.dim() != 3 or \
            gacc.shape[0] != B or gacc.shape[2] != D or G.numel() != B or seg_start.numel() != B + 1 or pos.numel() < sv.shape[1]:
        raise _lib.PeekvitHipError(f"{what}: sv {tuple(sv.shape)}, gR {tuple(gR.shape)}, grho {tuple(grho.shape)}, gacc {tuple(gacc.shape)}, "
                                   f"ycls {tuple(ycls.shape)}, G {tuple(G.shape)} for {B} images, D = {D}")
    if any(t.device != dev for t in (seg_start, n_halted, pos, ycls, gR, grho, gacc, G)):
        raise _lib.PeekvitHipError(what + ": every tensor must be on sv's device")
    R, S, n_cls, r_next = int(sv.shape[1]), int(gR.shape[1]), int(gacc.shape[1]), 0
    if not last:
        _chk(g_next, torch.float32, what + ": g_next"); _chk(seg_next, torch.int32, what + ": seg_next"); _chk(src_next, torch.int32, what + ": src_next")
        r_next = int(g_next.shape[0])
        if g_next.dim() != 2 or g_next.shape[1] != D or src_next.numel() < r_next or seg_next.numel() != B + 1 or g_next.device != dev:
            raise _lib.PeekvitHipError(f"{what}: g_next {tuple(g_next.shape)}, src_next {tuple(src_next.shape)}, seg_next {tuple(seg_next.shape)}")
    if gh is not None:
        _chk(gh, torch.float32, what + ": gh")
        if gh.numel() != 1 or gh.device != dev:
            raise _lib.PeekvitHipError(what + ": gh must be one fp32 value on sv's device")
    dy = torch.empty((R, D), dtype=torch.float32, device=dev)
    dy16 = torch.empty((R, D), dtype=_lib.operand_dtype(), device=dev) if want16 else None
    dR = torch.empty((B, S), dtype=torch.float32, device=dev)
    with _timed(entry, dev, 12.0 * B * S + 4.0 * B * n_cls * D, 4.0 * (2.5 * dy.numel() + 8 * B * S + 4 * B * n_cls * D)):
        check(run(_ptr(g_next) if not last else C.c_void_p(0), _ptr(seg_start), _ptr(n_halted), _ptr(pos),
                                                _ptr(seg_next) if not last else C.c_void_p(0), _ptr(src_next) if not last else C.c_void_p(0), _ptr(sv),
                                                _ptr(ycls), _ptr(gR), _ptr(grho), _ptr(gacc), _ptr(gh), _ptr(G), _ptr(dy), _ptr(dy16), _ptr(dR), B, S, D, R,
                                                r_next, n_cls, float(gate_scale), int(bool(last)), _stream(sv)), entry)
    _count()
    return dy, dy16, dR


def avit_pack_step_long_bwd(g_next, seg_start, n_halted, pos, seg_next, src_next, sv, ycls, gR, grho, gacc, gh, G, D: int, gate_scale: float, last: bool,
                            want16: bool = True):
    """avit_pack_step_bwd for up to AVIT_LONG_MAX_S tokens per image (pv_avit_pack_step_long_bwd): the same arguments and results,
    bit for bit up to 256 tokens."""
    return _avit_pack_bwd(lambda *a: _lib.load().pv_avit_pack_step_long_bwd(*a), "pv_avit_pack_step_long_bwd", g_next, seg_start, n_halted, pos, seg_next,
                          src_next, sv, ycls, gR, grho, gacc, gh, G, D, gate_scale, last, want16)


# ---- dropout on the training path (include/peekvit_hip_dropout.h) ------------------------------------------------------------
# key and site are 64-bit integers, p a Python float: the mask keep(key, site, row, col) is evaluated by the kernels and never stored.
def _chk_drop(key: int, site: int, p: float, what: str):
    key, site, p = int(key), int(site), float(p)
    if not (0 <= key < 1 << 64 and 0 <= site < 1 << 64):
        raise _lib.PeekvitHipError(f"{what}: key and site are unsigned 64-bit integers, got {key}, {site}")
    if not (0.0 <= p < 1.0):
        raise _lib.PeekvitHipError(f"{what}: p must be in [0, 1), got {p}")
    return key, site, p


def _chk_drop_rows(what: str, D: int, **tensors):
    """(name = (tensor, dtype)) of one element site: contiguous GPU tensors of the same element count on one device; returns the row count."""
    first = None
    for name, (t, dtype) in tensors.items():
        _chk(t, dtype, f"{what}: {name}")
        first = t if first is None else first
        if t.numel() != first.numel() or t.device != first.device or t.shape[-1] != D:
            raise _lib.PeekvitHipError(f"{what}: {name} must hold {first.numel()} values in rows of {D} on {first.device}, got {tuple(t.shape)} on {t.device}")
    if first.numel() < 1:
        raise _lib.PeekvitHipError(f"{what}: empty tensors")
    return first.numel() // D


def dropout_keep(key: int, site: int, rows: int, cols: int, p: float, device) -> torch.Tensor:
    """uint8 [rows, cols]: the 0 / 1 decisions of a site, by the kernels' own device function (tests and debugging)."""
    key, site, p = _chk_drop(key, site, p, "dropout_keep")
    keep = torch.empty((int(rows), int(cols)), dtype=torch.uint8, device=device)
    with _timed("pv_dropout_keep_u8", keep.device, 0.0, float(keep.numel())):
        check(_lib.load().pv_dropout_keep_u8(_ptr(keep), key, site, int(rows), int(cols), p, _stream(keep)), "pv_dropout_keep_u8")
    _count()
    return keep


def dropout_f32(x: torch.Tensor, out: torch.Tensor, key: int, site: int, p: float) -> torch.Tensor:
    """out = x o keep / (1 - p) on fp32 [..., D] read as rows of D; out may be x."""
    key, site, p = _chk_drop(key, site, p, "dropout_f32")
    D = x.shape[-1]
    rows = _chk_drop_rows("dropout_f32", D, x=(x, torch.float32), out=(out, torch.float32))
    with _timed("pv_dropout_f32", x.device, 1.0 * x.numel(), 8.0 * x.numel()):
        check(_lib.load().pv_dropout_f32(_ptr(x), _ptr(out), key, site, rows, D, p, _stream(x)), "pv_dropout_f32")
    _count()
    return out


def dropout_residual(x: torch.Tensor, u: torch.Tensor, out: torch.Tensor, key: int, site: int, p: float) -> torch.Tensor:
    """out = x + float(u) o keep / (1 - p)  (x, out fp32 [rows, D], out may be x; u 16-bit [rows, D]): masked_residual with an element mask."""
    key, site, p = _chk_drop(key, site, p, "dropout_residual")
    D = x.shape[-1]
    rows = _chk_drop_rows("dropout_residual", D, x=(x, torch.float32), u=(u, _lib.operand_dtype()), out=(out, torch.float32))
    with _timed("pv_dropout_residual", x.device, 2.0 * x.numel(), 10.0 * x.numel()):
        check(_lib.load().pv_dropout_residual(_ptr(x), _ptr(u), _ptr(out), key, site, rows, D, p, _stream(x)), "pv_dropout_residual")
    _count()
    return out


def dropout_bwd16(d: torch.Tensor, du: torch.Tensor, key: int, site: int, p: float) -> torch.Tensor:
    """du = round16(float(d) o keep / (1 - p)), 16-bit [rows, D] both, out of place (d survives: it is also the residual hand-over of an fp16 pass)."""
    key, site, p = _chk_drop(key, site, p, "dropout_bwd16")
    D = d.shape[-1]
    rows = _chk_drop_rows("dropout_bwd16", D, d=(d, _lib.operand_dtype()), du=(du, _lib.operand_dtype()))
    if d.data_ptr() == du.data_ptr():
        raise _lib.PeekvitHipError("dropout_bwd16: du must not be d")
    with _timed("pv_dropout_bwd16", d.device, 1.0 * d.numel(), 4.0 * d.numel()):
        check(_lib.load().pv_dropout_bwd16(_ptr(d), _ptr(du), key, site, rows, D, p, _stream(d)), "pv_dropout_bwd16")
    _count()
    return du


def attention_stream_drop(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, B: int, S: int, H: int, dh: int, p: float, key: int, site: int):
    """attention_stream with dropout on the probabilities: the softmax is of all keys (lse is attention_stream's, bit for bit), a dropped probability
    is 0 in the product with V and the survivors carry 1 / (1 - p).  The mask is keep(key, site, (b H + h) S + q, k).  p = 0 gives attention_stream's bits."""
    _chk_attn_stream(qkv, B, S, H, dh, "attention_stream_drop", out=out, lse=lse)
    key, site, p = _chk_drop(key, site, p, "attention_stream_drop")
    # (the generator: two 32-bit multiplies and ~10 integer operations per score, counted as 12)
    with _timed("pv_attention_stream_lse_drop_bf16", qkv.device, 4.0 * B * H * S * S * dh + 12.0 * B * H * S * S, 8.0 * B * S * H * dh + 4.0 * B * H * S):
        check(_lib.load().pv_attention_stream_lse_drop_bf16(_ptr(qkv), _ptr(out), _ptr(lse), B, S, H, dh, p, key, site, _attn_flag(qkv.device), _stream(qkv)),
              "pv_attention_stream_lse_drop_bf16")
    _count()
    return out


def attention_stream_bwd16_drop(qkv: torch.Tensor, dout: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dqkv16: torch.Tensor, B: int, S: int, H: int, dh: int,
                                qscale: float, p: float, key: int, site: int, dbias_partial: Optional[torch.Tensor] = None,
                                delta_ws: Optional[torch.Tensor] = None):
    """attention_stream_bwd16 for attention_stream_drop's forward (the same p, key, site): both launches evaluate the mask again.  p = 0 gives
    attention_stream_bwd16's bits."""
    what = "attention_stream_bwd16_drop"
    _chk_attn_stream(qkv, B, S, H, dh, what, dout=dout, out=out, lse=lse)
    key, site, p = _chk_drop(key, site, p, what)
    dev, D3 = qkv.device, 3 * H * dh
    _chk(dqkv16, _lib.operand_dtype(), what + ": dqkv16")
    if dqkv16.numel() != B * S * D3 or dqkv16.device != dev:
        raise _lib.PeekvitHipError(f"{what}: dqkv16 must hold {B * S * D3} values on {dev}")
    if dbias_partial is not None:
        _chk(dbias_partial, torch.float32, what + ": dbias_partial")
        if dbias_partial.numel() != B * ((S + 63) // 64) * D3 or dbias_partial.device != dev:
            raise _lib.PeekvitHipError(what + ": dbias_partial must hold B * ceil(S / 64) * 3 * H * dh values on qkv's device")
    if delta_ws is None:
        delta_ws = torch.empty((B, H, S), dtype=torch.float32, device=dev)
    else:
        _chk(delta_ws, torch.float32, what + ": delta_ws")
        if delta_ws.numel() != B * H * S or delta_ws.device != dev:
            raise _lib.PeekvitHipError(what + ": delta_ws must hold B * H * S values on qkv's device")
    with _timed("pv_attention_stream_bwd16_drop_bf16", dev, 14.0 * B * H * S * S * dh + 24.0 * B * H * S * S, 14.0 * B * S * H * dh + 12.0 * B * H * S):
        check(_lib.load().pv_attention_stream_bwd16_drop_bf16(_ptr(qkv), _ptr(dout), _ptr(out), _ptr(lse), _ptr(dqkv16), _ptr(dbias_partial), _ptr(delta_ws), B, S, H,
                                                              dh, float(qscale), p, key, site, _stream(qkv)), "pv_attention_stream_bwd16_drop_bf16")
    _count()
    return dqkv16
