"""Training path of the MI355X engine: forward WITH saved activations and the hand-written backward, exposed to PyTorch as
autograd Functions so that the reference's loop (train/train.py:112-121: `out = model(x)`, `loss.backward()`,
`optimizer.step()`) runs unchanged.  Pure plumbing like engine.py: every product / reduction is a C-ABI kernel.

Per encoder block (reference models/vit.py:45-55), R = B*S token rows:
  forward   h1 = LN1(x) | qkv = h1.Win^T+b (q pre-scaled) | att = attention(qkv) | x1 = x + att.Wo^T+b | h2 = LN2(x1)
            [gl | dgl] = fc1 epilogue pair: pre = h2.W1^T+b, gl = gelu(pre), dgl = gelu'(pre) | out = x1 + gl.W2^T+b
                                                                         saved: x, h1, qkv, att, x1, h2, [gl | dgl]
  backward  d2 = bf16(dout)
            dpre = (d2.W2)*dgl         [one GEMM, PV_EPI_GELU_GRAD_BF16]      dW2 = d2^T.gl     db2 = colsum(d2)
            dh2 = dpre.W1      dW1 = dpre^T.h2   db1 = colsum(dpre)
            dx1 = dout + LN2'(dh2)               (dgamma2, dbeta2)
            d1 = bf16(dx1)
            datt = d1.Wo       dWo = d1^T.att    dbo = colsum(d1)
            dqkv = attention'(qkv, datt)
            dh1 = dqkv.Win     dWin = dqkv^T.h1  dbin = colsum(dqkv)
            dx = dx1 + LN1'(dh1)                 (dgamma1, dbeta1)
Data gradients (x.W) are the forward NT GEMM on the transposed bf16 weight; weight gradients (dY^T.X) are the same NT GEMM on
the transposed activations with split-K over the R rows (pv_transpose_bf16 + pv_gemm_bf16 ksplit + pv_sum_slices_f32).
Gradients of 16-bit tensors travel in 16 bits (as under torch autocast); the residual-stream gradient and all parameter
gradients are fp32.

Operand type (round 5).  A MODEL-level training forward in precision mode "auto" runs on IEEE fp16 operands - the library the inference
path uses - so that the training forward sits inside the same 1e-3 contract as evaluation (bf16 operands: 4.7e-3 at ViT-B/16).  fp16
gradients need a LOSS SCALE: everything between the head and the stem - the HIP chain - runs in "scaled space", L * dL/dx, with L a power
of two chosen so that the largest gradient entering the chain sits at 2^7: measured on the golden models (scripts/train_f16_probe.py,
profiles/r05_train_f16_probe.txt) the largest 16-bit gradient inside the chain is 12x the entering one (the class-row gradient fans out
through LN2' and the attention), so the largest value anywhere sits near 1.5e3 - 40x below 65504 - and the smallest per-tensor maximum near 2,
whose typical elements are still 300x above fp16's smallest normal number (the fp16 MFMA flushes subnormal operands).  The chain's boundaries multiply by L (where a gradient enters: behind
the last block, `block.mask` handed to auxiliary losses) or by 1/L (where one leaves: every parameter gradient, the stem, the budget
token) - see enter() / leave() / _unscale() - so autograd and the optimizer only ever see true gradients: the reference's loop
(train/train.py:112-121) runs unchanged.  L follows the entering gradient's measured maximum with one step's delay (the first step reads
it synchronously).  An fp16 overflow anywhere in the chain turns into inf / NaN that propagates to the small per-block reductions every
backward node adds to `TrainPass.chk`.  The verdict is formed ON THE DEVICE at the end of the backward pass (no host synchronisation: the host
keeps queueing the next step) and applied where the step would be taken, by a global optimizer-step pre-hook, the way torch.cuda.amp.GradScaler
does: a FUSED torch optimizer receives it as `found_inf` (its kernel skips the update), any other optimizer has every parameter's `.grad` set to
None behind one event wait, which makes `step()` a no-op; the scale target is lowered when the host gets to read the verdict (at the latest when
the next backward pass starts).  An overflow of the FORWARD (a 16-bit activation beyond 65504: range flag bit 1) sends that model's training to
bf16 operands for good.
Blocks called on their own under autograd (no model-level pass) keep bf16 operands and no scale, as in rounds 1-4.
"""
from __future__ import annotations

import contextlib
import math
import os
import threading
import warnings
import weakref
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from . import _lib, ops
from ._lib import (PV_EPI_BIAS_BF16, PV_EPI_BIAS_F32, PV_EPI_BIAS_GELU_PAIR_BF16, PV_EPI_BIAS_RES_F32, PV_EPI_GELU_GRAD_BF16)
from .engine import _f32, bf16_weight, pver, workspace

# ------------------------------------------------------------------------------------------------------------------------------------
# operand type + loss scale of one training pass (module docstring)
# ------------------------------------------------------------------------------------------------------------------------------------
# PEEKVIT_AMD_TRAIN_OPERAND: "" (default) = fp16 in precision mode "auto", bf16 in mode "bf16"; "bf16" / "f16" force one
_TRAIN_OPERAND = os.environ.get("PEEKVIT_AMD_TRAIN_OPERAND", "")
SCALE_TARGET = float(os.environ.get("PEEKVIT_AMD_TRAIN_SCALE_TARGET", "128"))    # L * max|entering gradient|
# An overflow divides the target by 4; round 5 never raised it again, so a few transient spikes left L 64x lower for the rest of a run - the smallest
# per-tensor gradient maxima then sit in fp16's flush-to-zero range: silent precision loss instead of a skip.  Like GradScaler's
# growth_interval: after this many CONSECUTIVE clean steps the target doubles, up to SCALE_TARGET.
SCALE_GROWTH_INTERVAL = int(os.environ.get("PEEKVIT_AMD_TRAIN_SCALE_GROWTH_INTERVAL", "200"))
_tls = threading.local()
debug_amax = None            # a list: _block_bw appends the maxima of its 16-bit gradients (diagnostics only)
steps_skipped = 0            # training steps skipped because an fp16 gradient overflowed (tests / bench read it)
forward_fallbacks = 0        # models sent to bf16-operand training because their fp16 forward overflowed


class TrainState:
    """What the training path has learnt about one model (plain attribute `_pv_train`)."""
    __slots__ = ("operand", "target", "amax", "scale", "steps", "skipped", "last_skipped", "on_skip", "warned", "pending", "clean", "dropout_record")

    def __init__(self):
        self.operand = None            # None: decided per pass from the precision mode; "bf16": sticky (an fp16 forward overflowed / weights do not fit)
        self.target = SCALE_TARGET
        self.amax = None               # max |gradient entering the chain| of the last finished pass (host float)
        self.scale = 1.0               # L of the last pass
        self.steps, self.skipped, self.last_skipped = 0, 0, False
        self.clean = 0                 # consecutive clean steps since the target was last lowered (the target grows back after SCALE_GROWTH_INTERVAL of them)
        self.on_skip = None            # callable(model) -> None replacing the default "every .grad = None" (dist.OverlappedGradReducer)
        self.warned = False
        self.pending = None            # the last backward pass whose verdict has not been read on the host yet
        self.dropout_record = None     # (key, [(kind, site, p, shape), ...]) of the last pass that ran with fused dropout: enough to rebuild every mask


def train_state(model: nn.Module) -> TrainState:
    st = getattr(model, "_pv_train", None)
    if st is None:
        st = TrainState()
        object.__setattr__(model, "_pv_train", st)
    return st


def last_step_skipped(model: nn.Module) -> bool:
    """Did the last backward through `model` overflow fp16?  Waits for that pass's verdict (one event) and, if it is one to skip and no optimizer
    step has taken care of it yet, drops its gradients (every .grad = None): call it right behind `loss.backward()`."""
    st = train_state(model)
    tp = st.pending
    if tp is not None:
        if tp.resolve() and not tp.applied:
            tp.drop_gradients()
            if tp in _pending_passes:
                _pending_passes.remove(tp)
    return st.last_skipped


class TrainPass:
    """One model-level training forward and the backward passes through its graph."""

    def __init__(self, model: Optional[nn.Module], state: Optional[TrainState], operand: str, device):
        self.model, self.state, self.operand = model, state, operand
        self.scaled = operand == "f16" and model is not None
        self.L = 1.0
        self.active = False
        with torch.inference_mode(False), torch.no_grad():
            self.flag = torch.zeros(1, dtype=torch.int32, device=device) if self.scaled else None
            self.chk = torch.zeros(1, dtype=torch.float32, device=device) if self.scaled else None
        self.fwd_flag = None
        self.amax = None
        self.found, self.host, self.event, self.applied, self.skipped = None, None, None, True, False
        self.stepped = set()           # ids of the model's parameters an optimizer has already stepped (or skipped) under this pass's verdict
        self._pids = None
        # fused dropout (model.set_fused_dropout): one key per pass, the sites numbered in call order
        self.fused_dropout = False
        self.device = device
        self.drop_key = None
        self.drop_sites = []           # (kind, site, p, shape) per site: "input" [B, S, D] | "attention" [B, H, S, S] | "branch" [R, D]

    def drop_site(self, kind: str, p: float, shape) -> Tuple[int, int]:
        """(key, site number) of the pass's next dropout site; the key is drawn when the first site asks for it."""
        if self.drop_key is None:
            self.drop_key = dropout_key(self.device)
        site = len(self.drop_sites)
        self.drop_sites.append((kind, site, float(p), tuple(int(v) for v in shape)))
        return self.drop_key, site

    # -- backward side ---------------------------------------------------------------------------------------------------------
    def begin_backward(self, grad: torch.Tensor, primary: bool) -> float:
        """Called by the boundary nodes: the first one of a backward pass fixes L and queues the end-of-pass callback."""
        if not self.active:
            self.active = True
            st = self.state
            if st.pending is not None and st.pending is not self:
                st.pending.resolve()           # the previous step's verdict and statistics (its event has long fired: the GPU is at least a forward further)
            amax = st.amax
            if amax is None and primary:
                amax = float(grad.detach().abs().max())            # first pass of this model: one synchronous read
            if amax is None or not math.isfinite(amax) or amax <= 0.0:
                self.L = 1.0
            else:
                self.L = 2.0 ** max(min(math.floor(math.log2(st.target / amax)), 40), -40)
            st.scale = self.L
            torch.autograd.Variable._execution_engine.queue_callback(self._finish)
        if primary:
            with torch.no_grad():
                self.amax = grad.detach().abs().max()
        return self.L

    def note(self, t: torch.Tensor):
        """A small fp32 reduction of this node's gradients (LayerNorm-backward column sums, ...): inf / NaN anywhere upstream shows here."""
        if self.scaled:
            with torch.no_grad():
                self.chk.add_(t.sum())

    def _finish(self):
        """End of a backward pass (autograd callback): NO host synchronisation here (round 5, second form - the first one read the check word on
        the spot, which cost small models a third of their training throughput: the host could no longer queue the next step while this one
        runs).  The verdict is formed ON THE DEVICE - `found` = 1.0 if the check word is not finite or the forward raised its overflow bit - and
        copied with the statistics to pinned host memory behind the kernels; who needs it on the host waits for that one event (`resolve`).
        It is APPLIED where the step would otherwise be taken: the global optimizer-step pre-hook below."""
        self.active = False
        with torch.no_grad():
            fwd = (self.fwd_flag if self.fwd_flag is not None else self.flag)
            self.found = torch.logical_or(~torch.isfinite(self.chk), (fwd & 1) != 0).float()          # [1] on the device
            words = torch.cat([self.chk, (self.amax if self.amax is not None else self.chk.new_zeros(())).reshape(1), fwd.float(), self.found])
            self.found = self.found.reshape(())            # (torch's fused optimizers take `found_inf` as a 0-dim tensor, like GradScaler's)
            self.host = torch.empty(4, dtype=torch.float32).pin_memory()
            self.host.copy_(words, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(self.chk.device))
            self.chk = torch.zeros_like(self.chk)          # (a later backward pass through the same graph starts a fresh word)
        self.amax = None
        st = self.state
        if st.pending is not None and st.pending is not self:
            st.pending.resolve()
        st.pending = self
        self.applied = False
        # (a pass some optimizer has already consumed is over once the model's NEXT backward ends: parameters no optimizer owns never complete it)
        _pending_passes[:] = [tp for tp in _pending_passes if not (tp.state is st and tp.stepped)]
        _pending_passes.append(self)
        while len(_pending_passes) > 16:           # (backward passes that no optimizer step ever consumes - gradients taken for their own sake - must not pile up)
            old = _pending_passes.pop(0)
            old.resolve()
            old.applied = True

    def resolve(self) -> bool:
        """Wait for this pass's verdict (one event) and book it: loss-scale statistics, skipped-step counters, the bf16 fallback after a forward
        overflow.  Returns whether the step was one to skip.  Idempotent."""
        global steps_skipped, forward_fallbacks
        if self.host is None:
            return self.skipped
        self.event.synchronize()
        chk, amax, fbits, found = self.host.tolist()
        self.host = None
        st = self.state
        if st.pending is self:
            st.pending = None
        fwd_over = (int(fbits) & 1) != 0
        self.skipped = bool(found)
        if not self.skipped:
            st.steps += 1
            st.last_skipped = False
            if amax > 0.0 and math.isfinite(amax):
                st.amax = amax
            if st.target < SCALE_TARGET and SCALE_GROWTH_INTERVAL > 0:
                st.clean += 1
                if st.clean >= SCALE_GROWTH_INTERVAL:
                    st.target, st.clean = min(st.target * 2.0, SCALE_TARGET), 0
            return False
        st.skipped += 1
        st.last_skipped = True
        st.clean = 0
        steps_skipped += 1
        if fwd_over:
            st.operand = "bf16"
            forward_fallbacks += 1
            warnings.warn("peekvit_amd: a 16-bit activation of the training forward left the fp16 range (|v| > 65504); this step's gradients were "
                          "dropped and this model trains on bf16 operands from now on", RuntimeWarning, stacklevel=2)
        else:
            st.target = max(st.target / 4.0, 2.0)
            st.amax = amax if amax > 0.0 and math.isfinite(amax) else st.amax
            if not st.warned:
                st.warned = True
                warnings.warn(f"peekvit_amd: an fp16 gradient overflowed at loss scale {self.L:g}; this step's gradients were dropped (the optimizer "
                              "step is skipped) and the scale target was lowered", RuntimeWarning, stacklevel=2)
        return True

    def param_ids(self):
        if self._pids is None:
            self._pids = frozenset(id(p) for p in self.model.parameters() if p.requires_grad)
        return self._pids

    def drop_gradients(self):
        """The skip, host form: every .grad = None (torch optimizers and clip_grad_norm_ pass over such parameters), or the owner's own way
        (dist.OverlappedGradReducer: its gradients alias the all-reduce buckets)."""
        if self.applied:
            return
        self.applied = True
        if self.state.on_skip is not None:
            self.state.on_skip(self.model)
        else:
            for p in self.model.parameters():
                p.grad = None


# Passes whose verdict has not been applied to an optimizer step yet.  The global optimizer-step pre-hook applies them: a FUSED torch optimizer
# (`_step_supports_amp_scaling`: the interface torch.cuda.amp.GradScaler uses) is handed the device-side verdict as `found_inf` - its kernel skips
# the update and takes the step count back, no host synchronisation; any other optimizer gets the host form: wait for the verdict, and if the
# step is one to skip set every .grad to None, which makes `step()` a no-op (what GradScaler does for such optimizers, synchronisation included).
_pending_passes: list = []


def book_external_skip(model: nn.Module):
    """A step of `model` is being skipped for a reason its own backward pass did not see (non-finite values in all-reduced gradients)."""
    global steps_skipped
    st = train_state(model)
    st.skipped += 1
    st.last_skipped = True
    st.clean = 0
    steps_skipped += 1


def _optimizer_pre_hook(opt, args, kwargs):
    if not _pending_passes:
        return None
    mine = {id(p) for g in opt.param_groups for p in g["params"]}
    # Round 6: a pass stays pending until EVERY parameter of its model has been stepped under its verdict (or the model's next backward
    # ends).  Round 5 let the first optimizer that shared a parameter with the model consume the pass: a second optimizer over the model's other
    # parameters (backbone / head, gates split off) then found nothing pending and stepped on the overflowed gradients.
    todo = [tp for tp in _pending_passes if (tp.param_ids() & mine) - tp.stepped]
    if not todo:
        return None
    for tp in todo:
        tp.stepped |= tp.param_ids() & mine
        if tp.stepped >= tp.param_ids():
            _pending_passes.remove(tp)
    # The verdict of a pass covers ITS backward.  Whoever sums gradients across ranks afterwards (torch's DistributedDataParallel, a hand-written
    # all-reduce) hands a rank whose own verdict says "clean" the inf / NaN of a rank that overflowed: the gradients this step is about to consume
    # are therefore checked as well (one multi-tensor norm over them - the pass clip_grad_norm_ makes too), on the device for fused optimizers.
    grads = [p.grad for g in opt.param_groups for p in g["params"] if p.grad is not None and p.grad.is_cuda]
    if getattr(opt, "_step_supports_amp_scaling", False):
        # fused optimizer: the device-side verdict travels as `found_inf` - also when the gradients alias an OverlappedGradReducer's buckets
        # (round 5 sent that case to the host form below, whose "every .grad = None" the reducer turns into a no-op: the step then ran)
        found = todo[0].found if len(todo) == 1 else torch.stack([tp.found for tp in todo]).amax(0)
        if grads:
            with torch.no_grad():
                found = torch.maximum(found, (~torch.isfinite(torch.stack(torch._foreach_norm(grads)).sum())).float().to(found.device))
        prev = getattr(opt, "found_inf", None)
        opt._pv_prev_found = prev
        opt.found_inf = found if prev is None else torch.maximum(prev.to(found.device).reshape(()).float(), found)
        opt._pv_found_set = True
        for tp in todo:
            tp.applied = True
        return None
    skipped = False
    for tp in todo:
        if tp.resolve():
            skipped = True
            if tp.state.on_skip is not None and not tp.applied:
                raise RuntimeError("peekvit_amd: this training step overflowed fp16 and must be skipped, but its gradients alias an OverlappedGradReducer's "
                                   "buckets and cannot be dropped for a non-fused optimizer: call optimizer.step() only `if not reducer.skip_step` "
                                   "(or use a fused torch optimizer, which receives the verdict as found_inf)")
            tp.applied = False
            tp.drop_gradients()
        tp.applied = True
    if not skipped and grads:
        with torch.no_grad():
            if not bool(torch.isfinite(torch.stack(torch._foreach_norm(grads)).sum())):       # (non-finite gradients from somewhere else: see above)
                if any(tp.state.on_skip is not None for tp in todo):
                    raise RuntimeError("peekvit_amd: non-finite gradients in an OverlappedGradReducer's buckets at optimizer.step(): check "
                                       "`reducer.skip_step` after finish() (it covers the reduced buckets) or use a fused torch optimizer")
                for tp in todo:
                    book_external_skip(tp.model)
                    tp.applied = False
                    tp.drop_gradients()
    return None


def _optimizer_post_hook(opt, args, kwargs):
    if getattr(opt, "_pv_found_set", False):
        opt.found_inf = opt._pv_prev_found
        opt._pv_found_set = False


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post, register_optimizer_step_pre_hook as _reg_pre
    _reg_pre(_optimizer_pre_hook)
    _reg_post(_optimizer_post_hook)
except ImportError:                    # pragma: no cover - torch < 2.0
    pass


def current_pass() -> Optional[TrainPass]:
    return getattr(_tls, "tp", None)


def pass_operand(model: nn.Module) -> str:
    """The operand type a model-level training forward of `model` uses now."""
    from . import engine
    st = train_state(model)
    if st.operand is not None:
        return st.operand
    if _TRAIN_OPERAND in ("bf16", "f16"):
        return _TRAIN_OPERAND
    return "f16" if engine._PRECISION == "auto" else "bf16"


@contextlib.contextmanager
def _kernels(tp: Optional[TrainPass], operand: Optional[str] = None):
    """Operand library + range flag of a pass on the CALLING thread (the backward runs on autograd's device thread)."""
    op = tp.operand if tp is not None else operand
    if op is None:
        yield
        return
    from . import engine
    old_op = _lib.set_operand(op)
    old_flag = ops.current_range_flag()
    ops.set_range_flag(tp.flag if tp is not None and tp.scaled else None)
    try:
        if tp is not None and tp.scaled:
            with engine.no_param_checks():
                yield
        else:
            yield
    finally:
        _lib.set_operand(old_op)
        ops.set_range_flag(old_flag)


def model_forward_train(model: nn.Module, x: torch.Tensor, body, fused_dropout: bool = False):
    """Run `body()` (embed -> encoder -> pool_and_head_train, recorded by autograd) as one training pass of `model`.  fused_dropout: the blocks and
    the encoder input apply their dropout inside the HIP functions (the caller has checked fused_dropout_ok); a retry after an fp16 overflow of
    the forward is a new pass and draws a new key."""
    from . import engine
    st = train_state(model)
    for _attempt in range(2):
        tp = TrainPass(model, st, pass_operand(model), x.device)
        tp.fused_dropout = bool(fused_dropout)
        old = current_pass()
        _tls.tp = tp
        try:
            with _kernels(tp):
                out = body()
            if fused_dropout:
                st.dropout_record = (tp.drop_key, list(tp.drop_sites))
            if tp.scaled:
                with torch.no_grad():
                    tp.fwd_flag = tp.flag.clone()
            else:
                st.last_skipped = False          # (a pass without a loss scale has nothing to overflow: bf16 has fp32's range)
            return out
        except engine.F16RangeError as e:
            if tp.operand != "f16":
                raise
            st.operand = "bf16"
            warnings.warn(f"peekvit_amd: {e}; this model trains on bf16 operands", RuntimeWarning, stacklevel=2)
        finally:
            _tls.tp = old
    raise AssertionError("unreachable")


class _ScaleGradFn(torch.autograd.Function):
    """Identity whose backward multiplies by L (a gradient ENTERING the scaled chain) or by 1 / L (one LEAVING it)."""

    @staticmethod
    def forward(ctx, x, tp, enter, primary):
        ctx.tp, ctx.enter, ctx.primary = tp, enter, primary
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        tp = ctx.tp
        if ctx.enter:
            L = tp.begin_backward(g, ctx.primary)
            return (g if L == 1.0 else g * L), None, None, None
        L = tp.L
        if ctx.primary:                   # the gradient that leaves through the stem's input: the chain's last word
            tp.note(g.reshape(g.shape[0], -1).sum(0))
        return (g if L == 1.0 else g * (1.0 / L)), None, None, None


def enter(t: torch.Tensor, primary: bool = False, tp: Optional[TrainPass] = None) -> torch.Tensor:
    """Mark `t` as the place where gradients ENTER the scaled HIP chain from stock autograd (forward: identity)."""
    tp = current_pass() if tp is None else tp
    return _ScaleGradFn.apply(t, tp, True, primary) if tp is not None and tp.scaled and t.requires_grad else t


def leave(t: torch.Tensor, primary: bool = False, tp: Optional[TrainPass] = None) -> torch.Tensor:
    """Mark `t` as a place where gradients LEAVE the scaled chain into stock autograd (a stock-op parameter path feeding the chain)."""
    tp = current_pass() if tp is None else tp
    return _ScaleGradFn.apply(t, tp, False, primary) if tp is not None and tp.scaled and t.requires_grad else t


@contextlib.contextmanager
def stock_region():
    """A stretch of stock autograd ops INSIDE a model-level pass (between leave() and enter()): HIP functions called in there are on their
    own - no pass, bf16 operands, true gradients - exactly as when a block is called outside any model forward."""
    old_tp = current_pass()
    _tls.tp = None
    old_op = _lib.set_operand("bf16")
    old_flag = ops.current_range_flag()
    ops.set_range_flag(None)
    try:
        yield
    finally:
        _tls.tp = old_tp
        _lib.set_operand(old_op)
        ops.set_range_flag(old_flag)


def _unscale(tp: Optional[TrainPass], *grads):
    """Parameter gradients leave the chain: one multi-tensor multiply by 1 / L (in place)."""
    if tp is None or not tp.scaled or tp.L == 1.0:
        return
    ts, seen = [], set()
    for g in grads:
        if g is not None and g.data_ptr() not in seen:
            seen.add(g.data_ptr())
            ts.append(g)
    if ts:
        torch._foreach_mul_(ts, 1.0 / tp.L)


_wtcache: Dict[tuple, Tuple["weakref.ref", int, int, torch.Tensor]] = {}


def bf16_weight_t(p: torch.Tensor) -> torch.Tensor:
    """16-bit TRANSPOSE [K, N] of an fp32 [N, K] parameter (the 'weight' of the data-gradient GEMM), cached per version and operand type."""
    key = (id(p), _lib.OPERAND)
    ent = _wtcache.get(key)
    if ent is not None and ent[0]() is p and ent[1] == pver(p) and ent[2] == p.data_ptr():
        return ent[3]
    with torch.inference_mode(False):
        wt = ops.transpose(bf16_weight(p))
    _wtcache[key] = (weakref.ref(p, lambda _r, k=key: _wtcache.pop(k, None)), pver(p), p.data_ptr(), wt)
    return wt


MAX_ROWS = 4096          # rows per image the training path takes: pv_rank_topk's bound (RankViT's ranked layers)


def supported(D: int, H: int, S: int) -> bool:
    """Shapes the dense training blocks cover: dh in {32, 48, 64}, D <= 1024, D % 8 == 0 (the LayerNorm-backward and attention kernels,
    include/peekvit_hip.h) and 1 <= S <= 4096 rows per image.  The row count bounds no kernel of the block but the attention pair, and
    attention_pair() has one for every S: the LDS-resident kernels up to resident_rows(dh) rows, the streaming ones beyond.  A caller whose OTHER
    kernels are bounded by rows states that bound itself: the packed / compact modes and A-ViT's two training passes each have a resident rule (208
    rows, resident_rows(dh) for A-ViT's fused pass) and a long one beside it up to 4096 (DESIGN.md sections 33, 35, 36)."""
    dh = D // H
    return D % H == 0 and dh in (32, 48, 64) and 1 <= S <= MAX_ROWS and D <= 1024 and D % 8 == 0


def resident_rows(dh: int) -> int:
    """The longest image the LDS-resident attention backward holds (pv_attention_bwd_bf16: Q, K, V and dO of one head live in the LDS)."""
    return 416 if dh == 32 else 208


def _pad_rows(R: int) -> int:
    """K of the weight-gradient GEMMs: R rounded up so that up to 32 (big batches) / 8 split-K slices stay multiples of 128."""
    q = 4096 if R >= 65536 else 1024
    return (R + q - 1) // q * q


def _wgrad_transposed(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, accumulate: bool, db=None):
    """out (+)= dy^T . x through transposed copies (any shape): pv_transpose_bf16 x 2 -> NT GEMM with split-K -> slice sum.
    db (optional fp32 [No]): column sums of dy from the same transposition pass."""
    R, No = dy.shape
    Ni = x.shape[1]
    Rp = _pad_rows(R)
    dev = dy.device
    dy_t = ops.transpose(dy, workspace.get("wg_a", (No, Rp), _lib.operand_dtype(), dev), pad_to=Rp, colsum_out=db)
    x_t = ops.transpose(x, workspace.get("wg_b", (Ni, Rp), _lib.operand_dtype(), dev), pad_to=Rp)
    tiles = ((No + 255) // 256) * ((Ni + 255) // 256)
    ksplit = 1
    while ksplit < 32 and tiles * ksplit < 512 and Rp % (ksplit * 2 * 128) == 0:
        ksplit *= 2
    part = workspace.get("wg_part", (ksplit, No, Ni), torch.float32, dev)
    ops.gemm(dy_t, x_t, None, part, PV_EPI_BIAS_F32, ksplit=ksplit, tag="[wgrad]")
    return ops.sum_slices(part, out, accumulate)


_ATTN_BWD = os.environ.get("PEEKVIT_AMD_ATTN_BWD", "lse")          # "lse": the persistent kernel from the forward's row statistics where it applies | "recompute"


def _attn_lse(B: int, S: int, H: int, dh: int, dev):
    """fp32 [B, H, S] for the forward's log-sum-exp rows when the persistent backward kernel serves the shape (ops.attention_bwd_lse_ok), else None."""
    if _ATTN_BWD != "lse" or not ops.attention_bwd_lse_ok(S, dh):
        return None
    return torch.empty((B, H, S), dtype=torch.float32, device=dev)


_SPLITK_MODE = os.environ.get("PEEKVIT_AMD_WGRAD_SPLIT", "balanced")      # "balanced" (r2) | "pow2" (r1)


def _tn_slices(R: int, tiles: int, No: int, Ni: int, cus: int = 256) -> int:
    """Number of split-K slices of the weight-gradient GEMM.  A launch is tiles x slices workgroups of equal length on `cus` CUs, so its
    time is ROUNDS x one workgroup: r1 took the first power of two with >= 512 workgroups (fc1 / fc2: 36 tiles x 16 = 576 = 2.25 rounds -> 3
    rounds at 75 %, out-proj: 9 x 32 = 288 = 1.125 -> 2 rounds at 56 %).  Now: the slice count (<= 32, whole 128-row blocks, the kernel
    gives the last slice the remainder) that minimises rounds x rows-per-slice + the fp32 partial-slab traffic it causes."""
    best, best_t = 1, float("inf")
    for s_ in range(1, 33):
        if R // (s_ * 2) < 256 and s_ > 1:
            break
        rounds = -(-(tiles * s_) // cus)
        t_gemm = rounds * (R / s_) * (2.0 * 256 * 256) / 4.1e12          # one 256^2 tile-row at ~1.05 PFLOP/s / 256 CUs
        t_part = s_ * No * Ni * 8.0 / 5.5e12                              # slabs written once, read once by pv_sum_slices_f32
        if t_gemm + t_part < best_t:
            best, best_t = s_, t_gemm + t_part
    return best


def _wgrad(dy: torch.Tensor, x: torch.Tensor, tag: str, bias_grad: bool = True):
    """(dW fp32 [No, Ni] = dy^T . x,  db fp32 [No] = column sums of dy) for bf16 dy [R, No], x [R, Ni] (row-strided views
    allowed).  128-multiples of features: the TN kernel reads the row-major activations directly, split-K over the rows; the
    < 128 * ksplit tail rows (and every other shape) go through the transposed-copy path."""
    R, No = dy.shape
    Ni = x.shape[1]
    dev = dy.device
    out = torch.empty((No, Ni), dtype=torch.float32, device=dev)
    db = torch.empty((No,), dtype=torch.float32, device=dev) if bias_grad else None
    if No % 128 == 0 and Ni % 128 == 0 and R >= 256 and not _NO_TN:
        tiles = ((No + 255) // 256) * ((Ni + 255) // 256)
        if _SPLITK_MODE == "pow2":
            s_ = 1
            while s_ < 32 and tiles * s_ < 512 and R // (s_ * 2) >= 256:
                s_ *= 2
        else:
            s_ = _tn_slices(R, tiles, No, Ni)
        r_main = R // 128 * 128                      # the TN kernel deals whole 128-row blocks to the slices (last slice: the rest)
        part = workspace.get("wg_part", (s_, No, Ni), torch.float32, dev)
        ops.gemm_tn(dy[:r_main], x[:r_main], part, s_)
        ops.sum_slices(part, out)
        if r_main < R:
            _wgrad_transposed(dy[r_main:], x[r_main:], out, True)
        if bias_grad:
            ops.colsum(dy, db)
        return out, db
    _wgrad_transposed(dy, x, out, False, db)
    return out, db


_NO_TN = os.environ.get("PEEKVIT_AMD_WGRAD", "tn") != "tn"
# The residual gradient at x1 (between the two LayerNorm backward kernels of a block) travels in 16 bits in an fp16 pass: LayerNorm 2's backward
# writes only the 16-bit copy the data / weight-gradient GEMMs read anyway, LayerNorm 1's backward reads that copy as its residual term - 26
# instead of 32 bytes per element through the two kernels that sit at the HBM roofline: 235.2 -> 232.0 ms per ViT-B/16 step (8.71 -> 8.83 k img/s).
# Cost: one fp16 rounding (2^-11, in scaled space) of the residual gradient per block - complete gradients 0.88 - 1.21e-3 from the reference's training
# step instead of 0.36 - 0.98e-3 (asserted 2e-3), gradient norms unchanged (2 - 4e-4).  The block-to-block stream stays fp32.  bf16 passes keep the
# fp32 hand-off (a bf16 rounding per block is 1 %).  PEEKVIT_AMD_TRAIN_DX1=f32 restores it everywhere.
_DX1_16 = os.environ.get("PEEKVIT_AMD_TRAIN_DX1", "16") == "16"


def _bf16_grad(dout: torch.Tensor, buf: torch.Tensor):
    """(bf16 copy of an incoming fp32 gradient, its column sums or None): the producer's LayerNorm-backward kernel already wrote one (attached to the
    very tensor object autograd hands over) unless the gradient comes from stock ops (the head) or was touched since."""
    hand = getattr(dout, "_pv_bf16", None)
    if hand is not None and hand[1] == dout._version and hand[0].numel() == buf.numel():
        return hand[0].view(buf.shape), hand[2]
    return ops.cast_bf16((dout if dout.is_contiguous() else dout.contiguous()).view(buf.shape), buf), None


# The twelve parameters of an encoder block, in the order every block function takes them (behind blk, x and a mask) and returns their gradients.
BLOCK_PARAMS = ("ln1w", "ln1b", "inw", "inb", "ow", "ob", "ln2w", "ln2b", "w1", "b1", "w2", "b2")


def block_params(blk: nn.Module) -> tuple:
    """The parameter tensors of `blk` in BLOCK_PARAMS' order: arguments of the block functions, so that autograd routes their gradients."""
    mha, mlp = blk.self_attention.self_attention, blk.mlp
    return (blk.ln_1.weight, blk.ln_1.bias, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
            blk.ln_2.weight, blk.ln_2.bias, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)


# ---- the two branches of a block's backward, written once: every block function here and in pct_train calls them between its own LayerNorm backwards.
# `need` maps BLOCK_PARAMS to "needs a gradient": frozen parameters (the reference's finetuning trains gates / class tokens / head only,
# train/train.py:100) get None - their weight-gradient GEMMs, a fifth of the step, and bias sums are not computed.  The 16-bit buffers are the
# caller's, so that every path keeps the scratch (or the fresh tensors) it had.
def mlp_backward(blk, d2, pair, h2, need, dpre, dhid, db2=None, db2_always=True):
    """MLP branch: d2 = the 16-bit gradient [R, D] at the block output, pair = the saved [gelu | gelu'], h2 = the saved LayerNorm-2 output.  Fills
    dpre [R, Mh] = (d2 . W2) * gelu' and dhid [R, D] = dpre . W1, returns (dw2, db2, dw1, db1).  db2: fc2 bias sums handed over with d2 (none are
    computed then).  db2_always: with a weight gradient to compute, take the bias sums from the same pass even when b2 needs none."""
    R, D = d2.shape
    Mh = pair.shape[1] // 2
    gl, dgl = pair[:, :Mh], pair[:, Mh:]
    dw2 = None
    if need["w2"]:
        dw2, db2c = _wgrad(d2, gl, "fc2", bias_grad=db2 is None and (db2_always or need["b2"]))
        db2 = db2c if db2 is None else db2
    elif need["b2"] and db2 is None:
        db2 = ops.colsum(d2, torch.empty((D,), dtype=torch.float32, device=d2.device))
    db1 = torch.empty((Mh,), dtype=torch.float32, device=d2.device) if need["b1"] else None
    ops.gemm(d2, bf16_weight_t(blk.mlp.fc2.weight), None, dpre, PV_EPI_GELU_GRAD_BF16, M=R, res=dgl, tag="[dgrad]", colsum_out=db1)   # gelu' fused in the epilogue
    dw1 = _wgrad(dpre, h2, "fc1", bias_grad=False)[0] if need["w1"] else None
    ops.gemm(dpre, bf16_weight_t(blk.mlp.fc1.weight), None, dhid, PV_EPI_BIAS_BF16, M=R, tag="[dgrad]")
    return dw2, db2, dw1, db1


def out_proj_backward(blk, d1, att, need, datt):
    """Out-projection: d1 = the 16-bit gradient at its output (its column sums, the bias gradient, come from the LayerNorm-2 backward that wrote it),
    att the saved attention output.  Fills datt = d1 . Wo, returns dwo."""
    dwo = _wgrad(d1, att, "proj", bias_grad=False)[0] if need["ow"] else None
    ops.gemm(d1, bf16_weight_t(blk.self_attention.self_attention.out_proj.weight), None, datt, PV_EPI_BIAS_BF16, M=d1.shape[0], tag="[dgrad]")
    return dwo


def attn_backward(blk, d1, att, h1, need, datt, dqkv, dhid, dbp, attention_bwd):
    """Attention branch between the two LayerNorm backwards: out_proj_backward, then attention_bwd(datt, dqkv, dbp) - the caller's attention backward,
    which fills dqkv [R, 3 D] and, where dbp is not None (need["inb"]), its per-image bias partial rows - then the in-projection with h1 = the saved
    LayerNorm-1 output.  Fills dhid [R, D] = dqkv . Win, returns (dwo, dwin, dbin)."""
    dwo = out_proj_backward(blk, d1, att, need, datt)
    attention_bwd(datt, dqkv, dbp)
    dbin = ops.colsum(dbp, torch.empty((dqkv.shape[1],), dtype=torch.float32, device=d1.device)) if need["inb"] else None      # sum of the partial rows
    dwin = _wgrad(dqkv, h1, "qkv", bias_grad=False)[0] if need["inw"] else None
    ops.gemm(dqkv, bf16_weight_t(blk.self_attention.self_attention.in_proj_weight), None, dhid, PV_EPI_BIAS_BF16, M=d1.shape[0], tag="[dgrad]")
    return dwo, dwin, dbin


# ---- the encoder block of the ViT family, forward and backward written once.  Its variants differ along two axes only: the
# ATTENTION PAIR, with the row layout it implies (the classes below; attention_pair() picks the dense block's by its row count), and what the ROW
# SCALE m does - nothing (m is None: ViT, RankViT), A-ViT's 0/1 mask on the two LayerNorm outputs, or ResidualViT's mask on the LayerNorm outputs
# and on the attention branch (`scale_branch`).
class _ResidentAttn:
    """The attention pair of B resident images of S rows each (x [B, S, D]): ops.attention, and as attn_backward's callable the persistent kernel on
    the forward's row statistics where the forward kept them (_attn_lse), else the two-pass kernel that recomputes them.  One bias partial row per
    image."""

    def __init__(self, B, S):
        self.B, self.S, self.lse = B, S, None

    def forward(self, qkv, att, H, dh):
        self.lse = _attn_lse(self.B, self.S, H, dh, qkv.device)      # row statistics for the persistent backward kernel (None: the two-pass kernel recomputes them)
        ops.attention(qkv, att, self.B, self.S, H, dh, lse=self.lse)
        return ()                                                    # (nothing for save_for_backward: the statistics stay with this value)

    def backward(self, qkv, att, saved, H, dh, qscale):
        B, S, lse = self.B, self.S, self.lse
        if lse is not None:
            return lambda datt, dqkv, dbp: ops.attention_bwd_lse(qkv, datt, att, lse, dqkv, B, S, H, dh, qscale, dbias_partial=dbp)
        return lambda datt, dqkv, dbp: ops.attention_bwd(qkv, datt, dqkv, B, S, H, dh, qscale, dbias_partial=dbp)

    def bias_rows(self):
        return "bw_dbp", self.B


class _RaggedAttn:
    """The ragged, weighted attention pair of packed rows (x [R, D] in B segments `seg`, the longest of max_len rows): a key counts exp(log_mult)
    times.  The pair is chosen per block call by the longest segment of THIS layer: up to 208 rows the LDS-resident forward and its backward
    (ops.attention_varlen_w_lse / attention_varlen_w_bwd16), above the streaming pair (ops.attention_varlen_w_stream_lse /
    attention_varlen_w_stream_bwd16) - the resident forward is the faster one wherever it can run (section 33).  The
    statistics lse [R, H] and the two tables travel in save_for_backward; one bias partial row per 64 query rows of a segment."""

    def __init__(self, B, max_len):
        from . import engine
        self.B, self.max_len = B, int(max_len)
        self.stream = self.max_len > engine.SPARSE_RESIDENT_MAX_LEN

    def forward(self, qkv, att, H, dh, seg, log_mult):
        lse = torch.empty((qkv.shape[0], H), dtype=torch.float32, device=qkv.device)
        fw = ops.attention_varlen_w_stream_lse if self.stream else ops.attention_varlen_w_lse
        fw(qkv, att, lse, seg, log_mult, self.max_len, H, dh)
        return lse, seg, log_mult

    def backward(self, qkv, att, saved, H, dh, qscale):
        lse, seg, log_mult = saved
        bw = ops.attention_varlen_w_stream_bwd16 if self.stream else ops.attention_varlen_w_bwd16
        return lambda datt, dqkv, dbp: bw(qkv, datt, att, lse, seg, log_mult, dqkv, self.max_len, H, dh, qscale, dbias_partial=dbp)

    def bias_rows(self):
        return "bw_dbp_packed", self.B * ((self.max_len + 63) // 64)


class _StreamDropAttn:
    """The streaming attention pair with dropout on the probabilities (ops.attention_stream_drop / attention_stream_bwd16_drop) for B resident
    images of S rows: the mask is keep(key, site, (b H + h) S + q, k), evaluated again by both backward launches.  One bias partial row per 64
    query rows of an image.  Used only when the attention p is active: with branch or input dropout alone the block keeps attention_pair()'s choice."""

    def __init__(self, B, S, key, site, p):
        self.B, self.S, self.key, self.site, self.p, self.lse = B, S, int(key), int(site), float(p), None

    def forward(self, qkv, att, H, dh):
        self.lse = torch.empty((self.B, H, self.S), dtype=torch.float32, device=qkv.device)
        ops.attention_stream_drop(qkv, att, self.lse, self.B, self.S, H, dh, self.p, self.key, self.site)
        return ()

    def backward(self, qkv, att, saved, H, dh, qscale):
        B, S, lse, p, key, site = self.B, self.S, self.lse, self.p, self.key, self.site
        return lambda datt, dqkv, dbp: ops.attention_stream_bwd16_drop(qkv, datt, att, lse, dqkv, B, S, H, dh, qscale, p, key, site, dbias_partial=dbp)

    def bias_rows(self):
        return "bw_dbp_drop", self.B * ((self.S + 63) // 64)


_RESIDENT_FWD_ROWS = 416          # pv_attention_lse_bf16's bound (the resident-K/V forward), every head width


class _StreamAttn:
    """The attention pair of B resident images of S rows each beyond the resident backward's reach.  Forward: up to 416 rows
    the resident kernel with its row statistics (ops.attention(lse=): today's forward, bit for bit), beyond that the streaming one
    (ops.attention_stream) - both write lse fp32 [B, H, S] = log2 sum_k exp(s[q, k]).  Backward: the two-launch streaming kernels on out and lse
    (ops.attention_stream_bwd16), any S, no atomics.  One bias partial row per 64 query rows of an image, in scratch of its own name."""

    def __init__(self, B, S):
        self.B, self.S, self.lse = B, S, None

    def forward(self, qkv, att, H, dh):
        self.lse = torch.empty((self.B, H, self.S), dtype=torch.float32, device=qkv.device)
        if self.S <= _RESIDENT_FWD_ROWS:
            ops.attention(qkv, att, self.B, self.S, H, dh, lse=self.lse)
        else:
            ops.attention_stream(qkv, att, self.lse, self.B, self.S, H, dh)
        return ()

    def backward(self, qkv, att, saved, H, dh, qscale):
        B, S, lse = self.B, self.S, self.lse
        return lambda datt, dqkv, dbp: ops.attention_stream_bwd16(qkv, datt, att, lse, dqkv, B, S, H, dh, qscale, dbias_partial=dbp)

    def bias_rows(self):
        return "bw_dbp_stream", self.B * ((self.S + 63) // 64)


def attention_pair(B: int, S: int, dh: int):
    """The attention pair of a dense block of B images of S rows, written once: the resident pair wherever it serves (S <= 208, 416 at dh 32 - with
    the persistent backward on the forward's statistics where _attn_lse keeps them), the streaming pair beyond."""
    return _ResidentAttn(B, S) if S <= resident_rows(dh) else _StreamAttn(B, S)


def _block_fw(blk, x, params, attn, tables=(), m=None, scale_branch=False, h1=None, drop=None):
    """The forward's launches on x fp32 [..., D] contiguous, read as R rows: (out of x's shape, the tensors to save).  m (fp32, R values) multiplies both LayerNorm
    outputs per row - for a 0/1 mask LN(x * m) * m == m * LN(x) - and with scale_branch the attention branch as well: the out-projection then
    writes the 16-bit branch output u, which is kept for the mask gradient, and a masked residual add follows; without it the out-projection keeps
    its residual epilogue.  h1 = m * LN1(x), 16-bit [R, D], where the gate kernel or the pack step has emitted it already.  The LayerNorm, GEMM,
    weight-gradient and LayerNorm-backward kernels are row kernels and take any row count; `attn` (tables: its integer tables) knows the layout.
    drop = (key, site, p) of branch dropout (m is None only): the out-projection writes u as with scale_branch and pv_dropout_residual forms
    x1 = x + u o keep / (1 - p); without it the launches are what they were."""
    ln1w, ln1b, _inw, inb, _ow, ob, ln2w, ln2b, _w1, b1, _w2, b2 = params
    assert drop is None or m is None
    D = x.shape[-1]
    R = x.numel() // D
    mha, mlp = blk.self_attention.self_attention, blk.mlp
    H = mha.num_heads
    dh, Mh, dev, bf = D // H, mlp.fc1.out_features, x.device, _lib.operand_dtype()
    if h1 is None or h1.shape != (R, D):
        h1 = ops.layernorm_bf16(x, _f32(ln1w), _f32(ln1b), blk.ln_1.eps, torch.empty((R, D), dtype=bf, device=dev), m)
    qkv = torch.empty((R, 3 * D), dtype=bf, device=dev)
    att = torch.empty((R, D), dtype=bf, device=dev)
    u = torch.empty((R, D), dtype=bf, device=dev) if scale_branch or drop is not None else None
    x1 = torch.empty((R, D), dtype=torch.float32, device=dev)
    h2 = torch.empty((R, D), dtype=bf, device=dev)
    pair = torch.empty((R, 2 * Mh), dtype=bf, device=dev)           # [gelu(pre) | gelu'(pre)]: one fc1 epilogue writes both (round 6: the derivative, not the pre-activation)
    out = torch.empty_like(x)
    ops.gemm(h1, bf16_weight(mha.in_proj_weight), _f32(inb), qkv, PV_EPI_BIAS_BF16, M=R, qcols=D, qscale=float(dh) ** -0.5)
    attn_saved = attn.forward(qkv, att, H, dh, *tables)
    if scale_branch:
        ops.gemm(att, bf16_weight(mha.out_proj.weight), _f32(ob), u, PV_EPI_BIAS_BF16, M=R)
        ops.masked_residual(x, u, m, x1)
    elif drop is not None:
        ops.gemm(att, bf16_weight(mha.out_proj.weight), _f32(ob), u, PV_EPI_BIAS_BF16, M=R)
        ops.dropout_residual(x.view(R, D), u, x1, *drop)
        u = None                                                        # (its backward needs the mask, not the values)
    else:
        ops.gemm(att, bf16_weight(mha.out_proj.weight), _f32(ob), x1, PV_EPI_BIAS_RES_F32, M=R, res=x)
    ops.layernorm_bf16(x1, _f32(ln2w), _f32(ln2b), blk.ln_2.eps, h2, m)
    ops.gemm(h2, bf16_weight(mlp.fc1.weight), _f32(b1), pair, PV_EPI_BIAS_GELU_PAIR_BF16, M=R)
    ops.gemm(pair[:, :Mh], bf16_weight(mlp.fc2.weight), _f32(b2), out, PV_EPI_BIAS_RES_F32, M=R, res=x1)
    return out, (x, m, h1, qkv, att, u, x1, h2, pair) + attn_saved


def _block_bw(blk, saved, attn, need, tp, dout, scale_branch=False, drop=None):
    """The backward's launches for dout fp32 (R * D values): (dx fp32 of x's shape, its 16-bit copy, the column sums of dx, dm of m's shape or None, the twelve
    parameter gradients in BLOCK_PARAMS' order).  With a row scale the LayerNorm backwards are pv_layernorm_bwd_masked, which also forms
    dm = rowdot(dh1, LN1(x)) + rowdot(dh2, LN2(x1)) (+ rowdot(dx1, u) with scale_branch); only scale_branch returns it - A-ViT's mask comes from
    comparisons and has no gradient.  drop = (key, site, p) of the forward's branch dropout: the gradient of the branch output is
    du = round16(d1 o keep / (1 - p)) (pv_dropout_bwd16, out of place: d1 stays the residual hand-over), and the out-projection's bias gradient the
    column sum of the stored du."""
    x, m, h1, qkv, att, u, x1, h2, pair = saved[:9]
    D = x.shape[-1]
    R = x.numel() // D
    H = blk.self_attention.self_attention.num_heads
    dh, Mh, dev, bf, f32 = D // H, pair.shape[1] // 2, x.device, _lib.operand_dtype(), torch.float32
    ws = workspace
    # ---- MLP branch (scratch bw_*: shared by every variant, never with pct_train's pb_*) ------------------
    d2, db2 = _bf16_grad(dout, ws.get("bw_d", (R, D), bf, dev))
    dout = (dout if dout.is_contiguous() else dout.contiguous()).view(R, D)
    db2_handed = db2 is not None
    dpre, dhid = ws.get("bw_dgl", (R, Mh), bf, dev), ws.get("bw_dh", (R, D), bf, dev)
    dw2, db2, dw1, db1 = mlp_backward(blk, d2, pair, h2, need, dpre, dhid, db2)
    # (fp16 pass: the residual gradient at x1 travels to LayerNorm 1's backward as the 16-bit copy the GEMMs read anyway: _DX1_16 above.  fp32 in every
    #  pass under a row scale: the 16-bit hand-over is the unscaled block's alone)
    dx1_16 = m is None and _DX1_16 and bf == torch.float16
    dx1 = None if dx1_16 else ws.get("bw_dx1", (R, D), f32, dev)
    dgb2 = torch.empty((3, D), dtype=f32, device=dev)
    d1 = ws.get("bw_d1", (R, D), bf, dev)
    dm = None
    if m is None:
        ops.layernorm_bwd(x1, dhid, _f32(blk.ln_2.weight), dout, dx1, dgb2, blk.ln_2.eps, dx_bf16=d1)
    else:
        dm = torch.empty_like(m) if scale_branch else ws.get("bw_dm", (R,), f32, dev)      # (not scale_branch: the mask gradient the kernel forms is discarded)
        ops.layernorm_bwd_masked(x1, dhid, _f32(blk.ln_2.weight), _f32(blk.ln_2.bias), m, dout, u, dx1, d1, scale_branch, dgb2, dm, False, blk.ln_2.eps)
    # ---- attention branch (dgb2[2]: the column sums of d1, from the LN2 backward pass, are the out-projection's bias gradient) ----------
    datt, dqkv = ws.get("bw_datt", (R, D), bf, dev), ws.get("bw_dqkv", (R, 3 * D), bf, dev)
    name, rows = attn.bias_rows()
    dbp = ws.get(name, (rows, 3 * D), f32, dev) if need["inb"] else None
    dbo = dgb2[2]
    dbr = d1                             # the 16-bit gradient at the out-projection's output
    if drop is not None:
        dbr = ops.dropout_bwd16(d1, ws.get("bw_du", (R, D), bf, dev), *drop)
        dbo = ops.colsum(dbr, torch.empty((D,), dtype=f32, device=dev)) if need["ob"] else None
    dwo, dwin, dbin = attn_backward(blk, dbr, att, h1, need, datt, dqkv, dhid, dbp, attn.backward(qkv, att, saved[9:], H, dh, float(dh) ** -0.5))
    dx = torch.empty_like(x)
    dgb1 = torch.empty((3, D), dtype=f32, device=dev)
    dxb = torch.empty(x.shape, dtype=bf, device=dev)
    if m is None:
        ops.layernorm_bwd(x, dhid, _f32(blk.ln_1.weight), d1 if dx1_16 else dx1, dx, dgb1, blk.ln_1.eps, dx_bf16=dxb)
    else:
        ops.layernorm_bwd_masked(x, dhid, _f32(blk.ln_1.weight), _f32(blk.ln_1.bias), m, dx1, None, dx, dxb, False, dgb1, dm, scale_branch, blk.ln_1.eps)
    if debug_amax is not None:           # diagnostics (scripts/train_f16_probe.py): the largest 16-bit gradient of every kind in this block, in scaled units
        debug_amax.append({k: float(v.float().abs().max()) for k, v in (("d2", d2), ("dpre", dpre), ("d1", d1), ("datt", datt), ("dqkv", dqkv), ("dh1", dhid), ("dx", dxb))})
    if tp is not None:
        tp.note(dgb1)
    # parameter gradients leave the scaled chain (a handed-over db2 was unscaled by the block that produced it; dm stays inside the chain: it feeds
    # GateFn / PackStepFn)
    _unscale(tp, dgb1, dgb2, dwin, dbin, dwo, dw1, db1, dw2, None if db2_handed else db2, dbo if drop is not None else None)
    return dx, dxb, dgb1[2], (dm if scale_branch else None), (dgb1[0], dgb1[1], dwin, dbin, dwo, dbo, dgb2[0], dgb2[1], dw1, db1, dw2, db2)


class EncoderBlockFn(torch.autograd.Function):
    """One pre-LN encoder block with the MI355X forward + backward (_block_fw / _block_bw), in every variant of the ViT family:
      m None                      the plain block (reference models/vit.py:45-55): x [B, S, D]
      m [B, S], scale_branch      ResidualViT's masked block (reference models/residualvit.py:249-260; m = 1 on the class / budget rows):
                                  x1 = x + m * MHA(m * LN1(x)),  out = x1 + MLP(m * LN2(x1)); dm is returned; h1 may come from the gate kernel
      m [B, S], no scale_branch   A-ViT's block under a 0/1 token mask (reference models/adavit.py:54-79; 1 = still running): x1 = x + MHA(m * LN1(x)),
                                  out = x1 + MLP(m * LN2(x1)).  Dense over all S rows as the reference is: a halted row's input is zero, its output
                                  (the attention of the bias query over all keys, plus mlp(0)) is real, and channel 0 of it feeds the layer's halting
                                  score.  The mask comes from comparisons: no gradient
      ragged = (seg, log_mult, max_len)   either masked kind on packed rows x [R, D], m [R] (0 on a zero / representative row, which leaves as
                                  fc2(gelu(b1)) + b2 on top of its x1) with the ragged attention pair (DESIGN.md sections 29 and 30)."""

    @staticmethod
    def forward(ctx, blk, x, m, scale_branch, h1, ragged, *params):
        x = x.float() if x.dtype != torch.float32 else x
        x = x if x.is_contiguous() else x.contiguous()
        if m is not None:
            m = (m.float() if m.dtype != torch.float32 else m).contiguous()
        mha = blk.self_attention.self_attention
        attn, tables = ((attention_pair(x.shape[0], x.shape[1], x.shape[-1] // mha.num_heads), ()) if ragged is None
                        else (_RaggedAttn(ragged[0].numel() - 1, ragged[2]), ragged[:2]))
        out, saved = _block_fw(blk, x, params, attn, tables, m, scale_branch, h1)
        ctx.blk, ctx.attn, ctx.scale_branch = blk, attn, scale_branch
        ctx.tp, ctx.operand = current_pass(), _lib.current_operand()
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        need = dict(zip(BLOCK_PARAMS, ctx.needs_input_grad[6:18]))          # (needs_input_grad follows forward's argument order: behind blk, x, m, scale_branch, h1, ragged)
        dout = dout.float() if dout.dtype != torch.float32 else dout
        with _kernels(ctx.tp, ctx.operand):
            dx, dxb, colsum, dm, grads = _block_bw(ctx.blk, ctx.saved_tensors, ctx.attn, need, ctx.tp, dout, ctx.scale_branch)
        if dx.dim() == 3:
            # hand-off to the previous block's backward (see _bf16_grad; ActStepFn's backward edits dx and this copy in place and hands them on without
            # the column sums).  Behind a packed block sits a pack step, which reads no hand-off
            dx._pv_bf16 = (dxb, dx._version, colsum)
        return (None, dx, dm, None, None, None) + grads


class DropEncoderBlockFn(torch.autograd.Function):
    """The plain block (m None) of EncoderBlockFn under fused dropout: the same _block_fw / _block_bw, with
      p_attn > 0     the streaming attention pair that drops probabilities (_StreamDropAttn) instead of attention_pair()'s
      p_branch > 0   x1 = x + dropout(out_proj(attention)): the 16-bit branch output u, pv_dropout_residual, pv_dropout_bwd16 in the backward
    The pass numbers the sites and holds the key; nothing of a mask is saved."""

    @staticmethod
    def forward(ctx, blk, x, p_branch, p_attn, *params):
        x = x.float() if x.dtype != torch.float32 else x
        x = x if x.is_contiguous() else x.contiguous()
        B, S, D = x.shape
        tp = current_pass()
        H = blk.self_attention.self_attention.num_heads
        attn = _StreamDropAttn(B, S, *tp.drop_site("attention", p_attn, (B, H, S, S)), p_attn) if p_attn > 0.0 else attention_pair(B, S, D // H)
        drop = (*tp.drop_site("branch", p_branch, (B * S, D)), p_branch) if p_branch > 0.0 else None
        out, saved = _block_fw(blk, x, params, attn, drop=drop)
        ctx.blk, ctx.attn, ctx.drop = blk, attn, drop
        ctx.tp, ctx.operand = tp, _lib.current_operand()
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        need = dict(zip(BLOCK_PARAMS, ctx.needs_input_grad[4:16]))          # (behind blk, x, p_branch, p_attn)
        dout = dout.float() if dout.dtype != torch.float32 else dout
        with _kernels(ctx.tp, ctx.operand):
            dx, dxb, colsum, _dm, grads = _block_bw(ctx.blk, ctx.saved_tensors, ctx.attn, need, ctx.tp, dout, drop=ctx.drop)
        dx._pv_bf16 = (dxb, dx._version, colsum)          # hand-off to the previous block's backward, as EncoderBlockFn's
        return (None, dx, None, None) + grads


def block_forward_train(blk: nn.Module, x: torch.Tensor, dropout: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    """dropout = (p_branch, p_attn), the block's live values inside a pass with fused dropout (block_dropout_p), at least one of them > 0."""
    if dropout is not None and max(dropout) > 0.0:
        return DropEncoderBlockFn.apply(blk, x, float(dropout[0]), float(dropout[1]), *block_params(blk))
    return EncoderBlockFn.apply(blk, x, None, False, None, None, *block_params(blk))


class InputDropoutFn(torch.autograd.Function):
    """The encoder-input site, dropout(tokens + pos_embedding) on fp32 [B, S, D]: pv_dropout_f32 forward and - on the gradient, with the same
    (key, site) - backward.  The 16-bit hand-off of block 0's dx does not survive the mask, so the stem casts the gradient itself."""

    @staticmethod
    def forward(ctx, x, p):
        x = x.float() if x.dtype != torch.float32 else x
        x = x if x.is_contiguous() else x.contiguous()
        tp = current_pass()
        ctx.site = (*tp.drop_site("input", p, x.shape), float(p))
        ctx.tp, ctx.operand = tp, _lib.current_operand()
        return ops.dropout_f32(x, torch.empty_like(x), *ctx.site)

    @staticmethod
    def backward(ctx, g):
        g = (g.float() if g.dtype != torch.float32 else g).contiguous()
        with _kernels(ctx.tp, ctx.operand):
            return ops.dropout_f32(g, torch.empty_like(g), *ctx.site), None          # (a fresh tensor: no _pv_bf16 attribute travels on)


def input_dropout_train(tokens: torch.Tensor, p: float) -> torch.Tensor:
    return InputDropoutFn.apply(tokens, float(p)) if p > 0.0 else tokens


_SM_MASK = (1 << 64) - 1


def _sm64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _SM_MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _SM_MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _SM_MASK
    return z ^ (z >> 31)


def dropout_key(device) -> int:
    """A 64-bit key for one pass's dropout masks from the device's torch generator: a hash of (initial_seed, offset), the offset then advanced by 4
    (the unit of the Philox offset) - host arithmetic only, no synchronisation.  torch.manual_seed(s) reproduces a run bit for bit; two consecutive
    forwards draw different keys."""
    dev = torch.device(device)
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, off = gen.initial_seed(), gen.get_offset()
    gen.set_offset(off + 4)
    return _sm64((seed & _SM_MASK) ^ _sm64(off & _SM_MASK))


def live_dropout_p(model: nn.Module):
    """The p values in force NOW (read from the modules, not from the constructor arguments): the encoder input's, then (branch, attention) per block."""
    enc = model.encoder
    ps = [float(enc.dropout.p)]
    for blk in enc.layers:
        ps.extend(block_dropout_p(blk))
    return ps


def block_dropout_p(blk: nn.Module) -> Tuple[float, float]:
    return float(blk.dropout.p), float(blk.self_attention.self_attention.dropout)


def fused_dropout_ok(x: torch.Tensor, model: nn.Module) -> bool:
    """May this forward take the HIP training path WITH its dropout?  What train_eligible asks apart from "no dropout", a model in train mode, and
    live p values that are all below 1 with at least one above 0 (p = 1 zeroes a site: the composite's business)."""
    if not (model.training and train_eligible(x, model, 0.0)):
        return False
    ps = live_dropout_p(model)
    return all(0.0 <= p < 1.0 for p in ps) and any(p > 0.0 for p in ps)


def dropout_eligible(x: torch.Tensor, module: nn.Module) -> bool:
    """train_eligible's counterpart for a module called INSIDE a model-level pass that runs with fused dropout: its dropout is no reason to leave the
    HIP path.  False outside such a pass (a block called on its own keeps the composite under dropout)."""
    tp = current_pass()
    return tp is not None and tp.fused_dropout and module.training and train_eligible(x, module, 0.0)


def masked_block_forward_train(blk: nn.Module, x: torch.Tensor, mask: torch.Tensor, h1: torch.Tensor = None) -> torch.Tensor:
    """mask: [B,S,1] or [B,S] (carries the gate's autograd graph); h1: mask * LN1(x) as bf16 [B*S, D] when the gate kernel produced it."""
    m = mask.squeeze(-1) if mask.dim() == 3 else mask
    return EncoderBlockFn.apply(blk, x, m, True, h1, None, *block_params(blk))


def avit_block_forward_train(blk: nn.Module, x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """mask: [B,S], 1 = the token is still running (the reference passes its complement)."""
    return EncoderBlockFn.apply(blk, x, mask, False, None, None, *block_params(blk))


def avit_packed_block_forward_train(blk: nn.Module, x: torch.Tensor, row_scale: torch.Tensor, seg: torch.Tensor, log_mult: torch.Tensor,
                                    max_len: int) -> torch.Tensor:
    return EncoderBlockFn.apply(blk, x, row_scale, False, None, (seg, log_mult, max_len), *block_params(blk))


class ActStepFn(torch.autograd.Function):
    """A-ViT's halting step behind a block (reference models/adavit.py:170-217) on one kernel forward and one backward (include/peekvit_hip_avit_train.h):
    (y, c, R, rho, counter, m, acc) -> (x_next, c', R', rho', counter', m', acc', score).  y [B,S,D] is the block output and becomes x_next IN PLACE
    (halted rows zeroed - data only: its gradient is the identity on every row, as with the reference's `.data` masking).  R, rho, acc [B,n_cls,D] and
    the layer's score mean(h[1:]) are differentiable and chained from layer to layer; c, counter and the mask are not."""

    @staticmethod
    def forward(ctx, y, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last):
        B, S, _D = y.shape
        (c1, R1, rho1, cnt1, m1), acc1, h_part, sv, ycls = ops.avit_act_fwd(y, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last)
        score = h_part[1:].sum() / float((B - 1) * S) if B > 1 else h_part.new_full((), float("nan"))      # mean(h[1:]): NaN at B = 1, like the composite
        ctx.cfg = (float(gate_scale), bool(last))
        ctx.tp, ctx.operand = current_pass(), _lib.current_operand()
        ctx.save_for_backward(sv, ycls)
        ctx.mark_dirty(y)
        ctx.mark_non_differentiable(c1, cnt1, m1)
        ctx.set_materialize_grads(False)          # an output nothing reads (x_next behind the last block, R and the score under some losses) arrives as None, not as zeros
        return y, c1, R1, rho1, cnt1, m1, acc1, score

    @staticmethod
    def backward(ctx, gx, _gc, gR, grho, _gcnt, _gm, gacc, gscore):
        sv, ycls = ctx.saved_tensors
        _, B, S = sv.shape
        D, dev, f32 = ycls.shape[2], sv.device, torch.float32
        hand = getattr(gx, "_pv_bf16", None) if gx is not None else None
        if gx is None:                     # behind the last block nothing reads x_next
            gx = torch.zeros((B, S, D), dtype=f32, device=dev)
        elif hand is None or gx.dtype != f32 or not gx.is_contiguous():
            # (edited in place below: only a gradient the next block's backward made for this node - it carries the hand-off - is this node's to edit)
            gx, hand = gx.to(f32, copy=True).contiguous(), None
        dy16 = hand[0] if hand is not None and hand[1] == gx._version and hand[0].numel() == gx.numel() else None
        gR = torch.zeros((B, S), dtype=f32, device=dev) if gR is None else gR.float().contiguous()
        grho = torch.zeros((B, S), dtype=f32, device=dev) if grho is None else grho.float().contiguous()
        gacc = torch.zeros_like(ycls) if gacc is None else gacc.float().contiguous()
        gh = None if gscore is None or B == 1 else gscore.float().reshape(1)
        with _kernels(ctx.tp, ctx.operand):
            dR = ops.avit_act_bwd(gx, dy16, gR, grho, gacc, gh, sv, ycls, *ctx.cfg)
        if hand is not None:               # (the kernel's writes are invisible to _version: the hand-off is renewed by hand, without the column sums it no longer matches)
            del gx._pv_bf16
        if dy16 is not None:
            gx._pv_bf16 = (dy16, gx._version, None)
        return gx, None, dR, grho, None, None, gacc, None, None, None, None


def act_step_train(y, c, R, rho, counter, m, acc, gate_scale: float, gate_center: float, threshold: float, last: bool):
    return ActStepFn.apply(y, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last)


class GateFn(torch.autograd.Function):
    """ResidualViT's sigmoid gate with the learnable budget threshold + the token masking it drives (models/residualvit.py:197-235,
    :47-74, models/blocks.py:62-69), forward and backward on one kernel each: tokens [B,S,D] -> (masked tokens [B,S,D], row_scale [B,S] =
    [1 | mask | 1], thresholds [B]).  row_scale carries the autograd graph of the mask: the masked block (EncoderBlockFn with scale_branch) and any auxiliary
    loss on `block.mask` (a view of it) send their gradients back through it."""

    @staticmethod
    def forward(ctx, x, wg, bg, wb, bb, temp, sbias, ln=None):
        """ln = (gamma, beta, eps) of the masked block's LN1 (detached): the kernel also emits h1 = row_scale * LN1(masked) from the registers
        the rows are in (a constant of this function as far as autograd goes: the block differentiates LN1 from its own input)."""
        x = x.float() if x.dtype != torch.float32 else x
        x = x if x.is_contiguous() else x.contiguous()
        masked = torch.empty_like(x)
        thr = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        h1 = torch.empty((x.shape[0] * x.shape[1], x.shape[2]), dtype=_lib.operand_dtype(), device=x.device) if ln is not None else None
        _mask, rs = ops.residual_gate(x, masked, _f32(wg).view(-1), _f32(bg), _f32(wb).view(-1), _f32(bb), temp, sbias, thr_out=thr,
                                      ln=None if ln is None else (_f32(ln[0]), _f32(ln[1]), float(ln[2]), h1))
        ctx.save_for_backward(x, wg, bg, wb, bb)
        ctx.cfg = (float(temp), float(sbias))
        ctx.tp, ctx.operand = current_pass(), _lib.current_operand()
        if h1 is None:
            h1 = torch.empty((0,), dtype=_lib.operand_dtype(), device=x.device)
        ctx.mark_non_differentiable(thr, h1)
        return masked, rs, thr, h1

    @staticmethod
    def backward(ctx, dmasked, drs, _dthr, _dh1):
        x, wg, bg, wb, bb = ctx.saved_tensors
        B, S, D = x.shape
        dmasked = torch.zeros_like(x) if dmasked is None else (dmasked.float() if dmasked.dtype != torch.float32 else dmasked).contiguous()
        drs = torch.zeros((B, S), dtype=torch.float32, device=x.device) if drs is None else drs.float().contiguous()
        with _kernels(ctx.tp, ctx.operand):
            dx, dwg, dbg, dwb, dbb = ops.residual_gate_bwd(x, dmasked, drs, _f32(wg).view(-1), _f32(bg), _f32(wb).view(-1), _f32(bb), *ctx.cfg)
        if ctx.tp is not None:
            ctx.tp.note(dwg)
        dbg, dbb = dbg.clone(), dbb.clone()        # (views of one 4-element reduction: unscaled as tensors of their own)
        _unscale(ctx.tp, dwg, dbg, dwb, dbb)       # dx stays in the chain
        return dx, dwg.view_as(wg), dbg.view_as(bg), dwb.view_as(wb), dbb.view_as(bb), None, None, None


def gate_forward_train(blk: nn.Module, x: torch.Tensor):
    """(masked tokens, row_scale [B,S], thresholds [B], h1 = row_scale * LN1(masked) as bf16 [B*S, D]) of a ResidualViT block with a sigmoid
    gate and the learnable budget token."""
    g, bgate = blk.residual_gate, blk.budget_token_gate
    return GateFn.apply(x, g.projection.weight, g.projection.bias, bgate.weight, bgate.bias, g.temp, g.sigmoid_bias,
                        (blk.ln_1.weight.detach(), blk.ln_1.bias.detach(), blk.ln_1.eps))


class RowsBlockFn(torch.autograd.Function):
    """The LAST encoder block of a model forward in training, class-token row only: [B,S,D] -> [B,1,D] (engine.block_forward_rows is the
    inference counterpart).  The head reads that row alone (models/vit.py:242-246), so the gradient of every other output row is zero and
    the reference's backward through them multiplies zeros.  All-token work left: LN1, the k|v two thirds of the in-projection and their
    backward; everything else runs on B rows.
      forward   h1 = LN1(x) | kv = h1.Wkv^T+b | q = h1[cls].Wq^T+b (scaled) | att = attention_rows(q, kv) | x1 = x[cls] + att.Wo^T+b
                h2 = LN2(x1) | [gl | dgl] = fc1 pair | out = x1 + gl.W2^T+b                  saved: x, h1, kv, q, att, x1, h2, [gl | dgl]
      backward  as _block_bw on B rows down to datt; (dq, dkv) = attention_rows'(q, kv, att, datt); dWin = [dq^T.h1[cls] ; dkv^T.h1];
                dh1 = dkv.Wkv (+ dq.Wq on the class rows); dx = LN1'(dh1) (+ dx1 on the class rows)."""

    @staticmethod
    def forward(ctx, blk, x, m, ln1w, ln1b, inw, inb, ow, ob, ln2w, ln2b, w1, b1, w2, b2, h1_given=None):
        """m: None, or the ResidualViT row scale [B,S] of a masked block (h1 = m * LN1(x); the class-token rows carry scale 1, so everything
        behind the attention is the unmasked arithmetic)."""
        x = x.float() if x.dtype != torch.float32 else x
        x = x if x.is_contiguous() else x.contiguous()
        B, S, D = x.shape
        mha = blk.self_attention.self_attention
        H = mha.num_heads
        dh = D // H
        Mh = blk.mlp.fc1.out_features
        R, dev, eps, bf = B * S, x.device, blk.ln_1.eps, _lib.operand_dtype()
        qscale = float(dh) ** -0.5
        mrow = None if m is None else (m.float() if m.dtype != torch.float32 else m).contiguous().view(R)
        h1 = torch.empty((R, D), dtype=bf, device=dev)
        kv = torch.empty((R, 2 * D), dtype=bf, device=dev)
        q = torch.empty((B, D), dtype=bf, device=dev)
        att = torch.empty((B, D), dtype=bf, device=dev)
        x1 = torch.empty((B, D), dtype=torch.float32, device=dev)
        h2 = torch.empty((B, D), dtype=bf, device=dev)
        pair = torch.empty((B, 2 * Mh), dtype=bf, device=dev)
        gl = pair[:, :Mh]
        out = torch.empty((B, 1, D), dtype=torch.float32, device=dev)
        w_in = bf16_weight(mha.in_proj_weight)
        if h1_given is not None and h1_given.shape == (R, D):
            h1 = h1_given
        else:
            ops.layernorm_bf16(x, _f32(ln1w), _f32(ln1b), eps, h1, mrow)
        ops.gemm(h1, w_in[D:], _f32(inb)[D:], kv, PV_EPI_BIAS_BF16, M=R)
        ops.gemm(h1.view(B, S, D)[:, 0], w_in[:D], _f32(inb)[:D], q, PV_EPI_BIAS_BF16, M=B, qcols=D, qscale=qscale)
        ops.attention_rows(q, kv, att, B, S, 1, H, dh)
        ops.gemm(att, bf16_weight(mha.out_proj.weight), _f32(ob), x1, PV_EPI_BIAS_RES_F32, M=B, res=x[:, 0])
        ops.layernorm_bf16(x1, _f32(ln2w), _f32(ln2b), blk.ln_2.eps, h2)
        ops.gemm(h2, bf16_weight(blk.mlp.fc1.weight), _f32(b1), pair, PV_EPI_BIAS_GELU_PAIR_BF16, M=B)
        ops.gemm(gl, bf16_weight(blk.mlp.fc2.weight), _f32(b2), out.view(B, D), PV_EPI_BIAS_RES_F32, M=B, res=x1)
        ctx.blk, ctx.dims = blk, (B, S, D, H, dh, Mh, qscale)
        ctx.tp, ctx.operand = current_pass(), _lib.current_operand()
        ctx.masked = mrow is not None
        ctx.save_for_backward(x, h1, kv, q, att, x1, h2, pair, *([mrow] if mrow is not None else []))
        return out

    @staticmethod
    def backward(ctx, dout):
        with _kernels(ctx.tp, ctx.operand):
            return RowsBlockFn._bw(ctx, dout)

    @staticmethod
    def _bw(ctx, dout):
        blk = ctx.blk
        x, h1, kv, q, att, x1, h2, pair = ctx.saved_tensors[:8]
        mrow = ctx.saved_tensors[8] if ctx.masked else None
        B, S, D, H, dh, Mh, qscale = ctx.dims
        mha = blk.self_attention.self_attention
        R, dev, bf, f32 = B * S, x.device, _lib.operand_dtype(), torch.float32
        ws = workspace
        dout = (dout.float() if dout.dtype != f32 else dout).contiguous().view(B, D)
        # ---- MLP branch, class rows: B-row tensors, small enough to be allocated afresh ---------------------------
        need = dict(zip(BLOCK_PARAMS, ctx.needs_input_grad[3:15]))
        d2 = ops.cast_bf16(dout, torch.empty((B, D), dtype=bf, device=dev))
        db2 = dout.sum(0) if need["b2"] and not need["w2"] else None          # (bias alone: B rows, summed from the fp32 gradient itself, not from its 16-bit copy)
        dpre, dhq = torch.empty((B, Mh), dtype=bf, device=dev), torch.empty((B, D), dtype=bf, device=dev)
        dw2, db2, dw1, db1 = mlp_backward(blk, d2, pair, h2, need, dpre, dhq, db2)
        dx1 = torch.empty((B, D), dtype=f32, device=dev)
        dgb2 = torch.empty((3, D), dtype=f32, device=dev)
        d1 = torch.empty((B, D), dtype=bf, device=dev)
        ops.layernorm_bwd(x1, dhq, _f32(blk.ln_2.weight), dout, dx1, dgb2, blk.ln_2.eps, dx_bf16=d1)
        # ---- attention branch: the class-row / all-row split of the in-projection is this function's own ---------
        datt = torch.empty((B, D), dtype=bf, device=dev)
        dwo = out_proj_backward(blk, d1, att, need, datt)
        dq = torch.empty((B, D), dtype=bf, device=dev)
        dkv = ws.get("bw_dqkv", (R, 2 * D), bf, dev)
        ops.attention_rows_bwd(q, kv, att, datt, dq, dkv, B, S, H, dh, qscale)
        dbin = None
        if need["inb"]:
            dbin = torch.empty((3 * D,), dtype=f32, device=dev)
            ops.colsum(dq, dbin[:D])
            ops.colsum(dkv, dbin[D:])
        h1c = h1.view(B, S, D)[:, 0]                                           # LN1 output of the class rows (row-strided view)
        dwin = None
        if need["inw"]:                                                        # frozen in the reference's gates-only finetuning
            dwin = torch.cat([_wgrad(dq, h1c, "q", bias_grad=False)[0], _wgrad(dkv, h1, "qkv", bias_grad=False)[0]], dim=0)
        wt = bf16_weight_t(mha.in_proj_weight)                                 # [D, 3D]
        dhid = ws.get("bw_dh", (R, D), bf, dev)
        ops.gemm(dkv, wt[:, D:], None, dhid, PV_EPI_BIAS_BF16, M=R, tag="[dgrad]")
        dhc = torch.empty((B, D), dtype=bf, device=dev)
        ops.gemm(dq, wt[:, :D], None, dhc, PV_EPI_BIAS_BF16, M=B, tag="[dgrad]")
        dhid.view(B, S, D)[:, 0] += dhc
        dx = torch.empty((B, S, D), dtype=f32, device=dev)
        dgb1 = torch.empty((3, D), dtype=f32, device=dev)
        dxb = torch.empty((B, S, D), dtype=bf, device=dev)
        dm = None
        if mrow is None:
            ops.layernorm_bwd(x.view(R, D), dhid, _f32(blk.ln_1.weight), None, dx.view(R, D), dgb1, blk.ln_1.eps, dx_bf16=dxb)
        else:                                                                  # h1 = m * LN1(x): the mask gradient falls out of the same pass
            dm = torch.empty((R,), dtype=f32, device=dev)
            ops.layernorm_bwd_masked(x.view(R, D), dhid, _f32(blk.ln_1.weight), _f32(blk.ln_1.bias), mrow, None, None, dx.view(R, D), dxb, False,
                                     dgb1, dm, False, blk.ln_1.eps)
            dm = dm.view(B, S)
        dx[:, 0] += dx1                                                        # the residual path exists for the class rows only
        dxb[:, 0] = dx[:, 0]
        dgb1[2] += dx1.sum(0)
        if ctx.tp is not None:
            ctx.tp.note(dgb1)
        _unscale(ctx.tp, dgb1, dgb2, dwin, dbin, dwo, dw1, db1, dw2, db2)
        dx._pv_bf16 = (dxb, dx._version, dgb1[2])
        return (None, dx, dm, dgb1[0], dgb1[1], dwin, dbin, dwo, dgb2[2], dgb2[0], dgb2[1], dw1, db1, dw2, db2, None)


def block_forward_rows_train(blk: nn.Module, x: torch.Tensor, mask: torch.Tensor = None, h1: torch.Tensor = None) -> torch.Tensor:
    return RowsBlockFn.apply(blk, x, mask, *block_params(blk), h1)


class EmbedFn(torch.autograd.Function):
    """Patch embedding + class/register tokens + positional embedding (reference models/vit.py:203-236, :92) with backward:
    dW_conv = dpatch^T . im2col(img), db_conv = colsum(dpatch), dpos = sum_b dtok[b], dcls = dpos[:n_cls]."""

    @staticmethod
    def forward(ctx, model, img, conv_w, conv_b, pos, cls, reg):
        from . import engine
        tokens = engine.embed_tokens(model, img)
        ctx.model = model
        ctx.tp, ctx.operand = current_pass(), _lib.current_operand()
        ctx.has_reg = reg is not None
        ctx.save_for_backward(img)
        return tokens

    @staticmethod
    def backward(ctx, dtok):
        with _kernels(ctx.tp, ctx.operand):
            return EmbedFn._bw(ctx, dtok)

    @staticmethod
    def _bw(ctx, dtok):
        model = ctx.model
        (img,) = ctx.saved_tensors
        dtok = dtok.float() if dtok.dtype != torch.float32 else dtok
        dtok = dtok if dtok.is_contiguous() else dtok.contiguous()
        B, S, D = dtok.shape
        P = model.patch_size
        ncls, nreg = model.num_class_tokens, model.num_registers
        nsp = ncls + nreg
        Np = S - nsp
        dev = dtok.device
        u8 = img.dtype == torch.uint8
        Cin = img.shape[3] if u8 else img.shape[1]
        K = Cin * P * P
        dwc, dbc = None, None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:          # a frozen stem (gates / class tokens / head finetuning) costs nothing here
            dpatch32 = dtok[:, nsp:, :].contiguous().view(B * Np, D)
            dpatch = ops.cast_bf16(dpatch32, workspace.get("bw_dgl", (B * Np, D), _lib.operand_dtype(), dev))
            if ctx.needs_input_grad[2]:
                cols = workspace.get("cols", (B * Np, K), _lib.operand_dtype(), dev)
                if u8:
                    from .engine import IMAGENET_MEAN, IMAGENET_STD
                    ops.im2col_u8(img, P, cols, getattr(model, "input_mean", IMAGENET_MEAN), getattr(model, "input_std", IMAGENET_STD))
                else:
                    ops.im2col(img if img.dtype == torch.float32 else img.float(), P, cols)
                dwc, dbc = _wgrad(dpatch, cols, "conv")
                dwc = dwc.view(model.conv_proj.weight.shape)
            else:
                dbc = ops.colsum(dpatch, torch.empty((D,), dtype=torch.float32, device=dev))
        dpos = ops.colsum(dtok.view(B, S * D), torch.empty((S * D,), dtype=torch.float32, device=dev)).view(1, S, D)
        if ctx.tp is not None:
            ctx.tp.note(dpos)                      # the chain's last word: anything non-finite upstream has reached the token gradient
        _unscale(ctx.tp, dwc, dbc, dpos)
        dcls = dpos[:, :ncls].clone()
        dreg = dpos[:, ncls:nsp].clone() if ctx.has_reg else None
        return (None, None, dwc, dbc, dpos, dcls, dreg)


def embed_tokens_train(model: nn.Module, img: torch.Tensor) -> torch.Tensor:
    if img.requires_grad:
        # someone differentiates with respect to the IMAGE (saliency maps, adversarial examples): EmbedFn has no col2im, so the stem runs on
        # the stock convolution (0.7 % of the FLOPs) and autograd delivers dL/d(image); the blocks behind it stay on the HIP functions
        return leave(model._composite_tokens(img.float() if img.dtype != torch.float32 else img) + model.encoder.pos_embedding, primary=True)
    reg = model.register_tokens if model.num_registers > 0 else None
    return EmbedFn.apply(model, img, model.conv_proj.weight, model.conv_proj.bias, model.encoder.pos_embedding, model.class_tokens, reg)


class SortDropFn(torch.autograd.Function):
    """RankViT ranking + compaction (models/rankvit.py:55-77) with the same HIP kernels as inference (bit-exact keep indices);
    backward scatters the gradient rows back to the kept positions (indices carry no gradient, as with torch.gather)."""

    @staticmethod
    def forward(ctx, x, budget):
        from . import engine
        x = x.float() if x.dtype != torch.float32 else x
        out, keep = engine.sort_and_drop(x, budget)
        ctx.s_in = x.shape[1]
        ctx.save_for_backward(keep)
        ctx.mark_non_differentiable(keep)
        return out, keep

    @staticmethod
    def backward(ctx, dout, _dkeep):
        (keep,) = ctx.saved_tensors
        dout = dout.float() if dout.dtype != torch.float32 else dout
        if keep.shape[1] == 0:                     # budget 0: only the class token went on
            dx = dout.new_zeros((dout.shape[0], ctx.s_in, dout.shape[2]))
            dx[:, :1] = dout
            return dx, None
        return ops.scatter_tokens(dout if dout.is_contiguous() else dout.contiguous(), keep, ctx.s_in), None


def sort_and_drop_train(x: torch.Tensor, budget: float):
    return SortDropFn.apply(x, budget)


def pool_and_head_train(model: nn.Module, tokens: torch.Tensor) -> torch.Tensor:
    """Final LayerNorm on the class-token rows, sum, head: [B, n_cls, D] fp32 stock ops under autograd (0.02 % of the
    step's FLOPs; the gradient re-enters the HIP backward as dL/d(tokens), zero outside the class rows)."""
    tokens = enter(tokens, primary=True)              # stock autograd ends here: the gradient enters the (scaled) HIP chain
    cls = model.encoder.ln(tokens[:, 0:model.num_class_tokens])
    return model.head(cls.sum(dim=1))


def train_eligible(x: torch.Tensor, module: nn.Module, dropout_p: float) -> bool:
    from . import engine
    return (x.is_cuda and x.numel() > 0 and torch.is_grad_enabled() and not (module.training and dropout_p > 0.0) and engine._PRECISION in ("auto", "bf16")
            and os.environ.get("PEEKVIT_AMD_BACKEND", "") != "torch" and os.environ.get("PEEKVIT_AMD_TRAIN", "hip") == "hip")


# ---- ResidualViT training on the packed live rows (include/peekvit_hip_sparse_train.h) ---------------------------------------
# A token whose mask is exactly 0 enters its block as a zero row, leaves it as a constant and receives no gradient, so the packed forward of
# DESIGN.md section 17 under autograd gives the dense step's parameter gradients.  A packed row that stands for n identical tokens carries the total
# gradient of its n members: every row-wise backward below is linear in it.
class PackStepFn(torch.autograd.Function):
    """The gate of one block on the packed rows + the next packed input (pv_residual_pack_step_train; with more than 208 rows per image
    pv_residual_pack_step_long_train), and its backward (pv_residual_pack_step_bwd / pv_residual_pack_step_long_bwd).  x fp32 [R, D] ->
    (x_next [R', D], row_scale_next [R'], dense mask [B, N], thresholds [B], h1 = row_scale_next * LN1(x_next) 16-bit [R', D]).  The integer tables
    of the next layer and the longest segment are left in `info` (a dict): R' is read on the host, the layer's one synchronisation."""

    @staticmethod
    def forward(ctx, x, wg, bg, wb, bb, temp, sbias, seg, mult, tok_row, ln, info):
        from . import engine
        R, D = x.shape
        B, N = tok_row.shape
        dev = x.device
        nxt = (torch.empty((R, D), dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev),
               torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.float32, device=dev),
               torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev))
        mask = torch.empty((B, N), dtype=torch.float32, device=dev)
        thr = torch.empty((B,), dtype=torch.float32, device=dev)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        mask_row, gate_arg = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
        src_next = torch.empty(R, dtype=torch.int32, device=dev)
        h1 = torch.empty((R, D), dtype=_lib.operand_dtype(), device=dev)
        step = ops.residual_pack_step_train if N + 2 <= engine.SPARSE_RESIDENT_MAX_LEN else ops.residual_pack_step_long_train
        step(x, seg, mult, tok_row, _f32(wg).view(-1), _f32(bg), _f32(wb).view(-1), _f32(bb), temp, sbias, nxt, mask, thr, totals, mask_row, gate_arg, src_next,
             ln=(_f32(ln[0]), _f32(ln[1]), float(ln[2]), h1))
        r_next, max_len = totals.tolist()          # (the layer's one host synchronisation: the size of its launches)
        engine.sparse_syncs += 1
        if not 2 * B <= r_next <= R or not 2 <= max_len <= N + 2:
            raise _lib.PeekvitHipError(f"packed training: a pack step reports {r_next} rows, longest segment {max_len} (from {R} rows, {N + 2} tokens)")
        info.update(seg=nxt[4], mult=nxt[2][:r_next], tok_row=nxt[5], log_mult=nxt[3][:r_next], max_len=max_len, rows=r_next)
        ctx.save_for_backward(x, wg, bg, wb, bb, seg, tok_row, mask_row, gate_arg, thr, nxt[4], src_next)
        ctx.temp, ctx.r_next = float(temp), r_next
        ctx.long = N + 2 > engine.SPARSE_RESIDENT_MAX_LEN
        ctx.tp, ctx.operand = current_pass(), _lib.current_operand()
        x_next, rs_next, h1 = nxt[0][:r_next], nxt[1][:r_next], h1[:r_next]
        ctx.mark_non_differentiable(thr, h1)
        return x_next, rs_next, mask, thr, h1

    @staticmethod
    def backward(ctx, dxn, drs, dmask, _dthr, _dh1):
        x, wg, bg, wb, bb, seg, tok_row, mask_row, gate_arg, thr, seg_next, src_next = ctx.saved_tensors
        D, dev, rn = x.shape[1], x.device, ctx.r_next
        dxn = torch.zeros((rn, D), dtype=torch.float32, device=dev) if dxn is None else dxn.float().contiguous()
        drs = torch.zeros((rn,), dtype=torch.float32, device=dev) if drs is None else drs.float().contiguous()
        dmask = None if dmask is None else dmask.float().contiguous()
        with _kernels(ctx.tp, ctx.operand):
            step_bwd = ops.residual_pack_step_long_bwd if ctx.long else ops.residual_pack_step_bwd
            dx, _dm, dwg, dbg, dwb, dbb = step_bwd(x, seg, tok_row, mask_row, gate_arg, thr, seg_next, src_next, dxn, drs, dmask, _f32(wg).view(-1),
                                                   _f32(wb).view(-1), ctx.temp)
        if ctx.tp is not None:
            ctx.tp.note(dwg)
        dbg, dbb = dbg.clone(), dbb.clone()        # (views of one 4-element reduction: unscaled as tensors of their own)
        _unscale(ctx.tp, dwg, dbg, dwb, dbb)       # dx stays in the chain
        return dx, dwg.view_as(wg), dbg.view_as(bg), dwb.view_as(wb), dbb.view_as(bb), None, None, None, None, None, None, None


def residual_forward_packed_train(model: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """One training forward of a ResidualVisionTransformer on its packed live rows, inside model_forward_train's pass: embed_tokens_train, the budget
    row as in the dense path, per layer PackStepFn (one host read of the row count) and the masked EncoderBlockFn on the packed rows, pool_and_head_train on the gathered class
    rows.  Every block's `mask` is the dense [B, N, 1] tensor that carries the graph, `residual_gate.threshold` is set as in the dense path.  The
    caller has checked eligibility (ResidualVisionTransformer._compaction_ok(training=True) up to 208 rows per image, _long_compact_training_ok above)."""
    from . import engine
    tokens = embed_tokens_train(model, x)
    tokens = model._add_budget_token(tokens, wrap=leave)
    B, S, D = tokens.shape
    dev = tokens.device
    seg, mult, tok_row = engine._sparse_initial_tables(B, S, dev)
    xs = tokens.reshape(B * S, D)
    rows, longest = [], []
    for blk in model.encoder.layers:
        g, bgate = blk.residual_gate, blk.budget_token_gate
        info = {}
        xm, rs, mask, thr, h1 = PackStepFn.apply(xs, g.projection.weight, g.projection.bias, bgate.weight, bgate.bias, g.temp, g.sigmoid_bias, seg, mult,
                                                 tok_row, (blk.ln_1.weight.detach(), blk.ln_1.bias.detach(), blk.ln_1.eps), info)
        blk.mask = enter(mask).unsqueeze(-1)       # (auxiliary mask losses: their gradient enters the scaled chain here)
        g.threshold = thr.view(-1, 1, 1)           # what ResidualGate.forward leaves behind (residualvit.py:66)
        seg, mult, tok_row = info["seg"], info["mult"], info["tok_row"]
        rows.append(info["rows"])
        longest.append(info["max_len"])
        engine.sparse_rows += info["rows"]
        engine.sparse_dense_rows += B * S
        engine.sparse_train_long_layers += info["max_len"] > engine.SPARSE_RESIDENT_MAX_LEN
        xs = EncoderBlockFn.apply(blk, xm, rs, True, h1, (seg, info["log_mult"], info["max_len"]), *block_params(blk))
    engine._region.sparse_last_rows = rows
    engine._region.sparse_last_max_len = longest
    cls = xs.index_select(0, seg[:-1].long())      # every image's class row is the first of its segment
    return pool_and_head_train(model, cls.view(B, 1, D))


# ---- A-ViT training on the packed live rows (include/peekvit_hip_avit_pack_train.h) --------------------------------------------
# A halted token enters its block as a zero row and leaves it as the same vector as every other halted token of its image, so one representative row
# (row scale 0, key weight ln n) stands for all n of them, as in the inference forward of section 14.  Its output still feeds the layer's score through
# channel 0; the gradient of that - at this layer and, the masking being invisible to autograd, passed through from every later one - is one scalar per
# image, G, which AViTPackStepFn's backward walks from the last layer to the first.  A packed row that stands for n tokens carries the total gradient
# of its n members (section 29's convention): every row-wise backward below is linear in it.
class AViTPackStepFn(torch.autograd.Function):
    """A-ViT's halting step behind a block on the packed rows + the next packed input (pv_avit_pack_step_train), and its backward
    (pv_avit_pack_step_bwd; with more than 208 tokens per image the chunked pv_avit_pack_step_long / pv_avit_pack_step_long_bwd of DESIGN.md section 36,
    a choice the forward leaves in ctx.long): (y [R, D], c, R, rho, counter, m, acc) -> (x_next [R', D], row_scale_next [R'], c', R', rho', counter', m', acc', score).
    The integer tables of the next layer and the longest segment are left in `info` (a dict): R' is read on the host, the layer's one
    synchronisation (none behind the last layer, which has no next input).  `chain` is a dict the steps of one forward share: it holds G."""

    @staticmethod
    def forward(ctx, y, c, R, rho, counter, m, acc, seg, nh, pos, gate_scale, gate_center, threshold, last, info, chain):
        from . import engine
        Rr, D = y.shape
        B, S = c.shape
        ctx.long = S > engine.AVIT_RESIDENT_MAX_S
        if ctx.long:
            out = ops.avit_pack_step_long(y, seg, nh, pos, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last)
        else:
            out = ops.avit_pack_step_train(y, seg, nh, pos, c, R, rho, counter, m, acc, gate_scale, gate_center, threshold, last)
        (c1, R1, rho1, cnt1, m1), acc1, h_part, sv, ycls, nxt = out
        score = h_part[1:].sum() / float((B - 1) * S) if B > 1 else h_part.new_full((), float("nan"))      # mean(h[1:]): NaN at B = 1, like the composite
        ctx.cfg = (int(D), float(gate_scale), bool(last))
        ctx.tp, ctx.operand, ctx.chain = current_pass(), _lib.current_operand(), chain
        ctx.set_materialize_grads(False)
        if last:
            ctx.r_next = 0
            ctx.save_for_backward(sv, ycls, seg, nh, pos)
            x_next, rs_next = y.new_empty((0, D)), y.new_empty((0,))
        else:
            x_full, rs_full, seg_next, nh_next, lm_next, pos_next, totals, src_next = nxt
            if engine.avit_train_gaps is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            r_next, max_len = totals.tolist()          # (the layer's one host synchronisation: the size of the next layer's launches)
            engine.avit_train_syncs += 1
            if engine.avit_train_gaps is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                engine.avit_train_gaps.append((e0, e1))
            if not B <= r_next <= Rr or not 1 <= max_len <= S:
                raise _lib.PeekvitHipError(f"packed A-ViT training: a pack step reports {r_next} rows, longest segment {max_len} (from {Rr} rows, {S} tokens)")
            info.update(seg=seg_next, nh=nh_next, pos=pos_next[:r_next], log_mult=lm_next[:r_next], max_len=max_len, rows=r_next)
            ctx.r_next = r_next
            ctx.save_for_backward(sv, ycls, seg, nh, pos, seg_next, src_next)
            x_next, rs_next = x_full[:r_next], rs_full[:r_next]
        ctx.mark_non_differentiable(rs_next, c1, cnt1, m1)
        return x_next, rs_next, c1, R1, rho1, cnt1, m1, acc1, score

    @staticmethod
    def backward(ctx, gx, _grs, _gc, gR, grho, _gcnt, _gm, gacc, gscore):
        D, gate_scale, last = ctx.cfg
        saved = ctx.saved_tensors
        sv, ycls, seg, nh, pos = saved[:5]
        seg_next, src_next = (None, None) if last else saved[5:7]
        B, dev, f32 = nh.numel(), sv.device, torch.float32
        if last:
            gx = None
            ctx.chain["G"] = torch.zeros((B,), dtype=f32, device=dev)          # the walk starts here: no later layer
        else:
            gx = torch.zeros((ctx.r_next, D), dtype=f32, device=dev) if gx is None else gx.float().contiguous()
        G = ctx.chain.get("G")
        if G is None:
            raise _lib.PeekvitHipError("packed A-ViT training: a halting step's backward ran before the last layer's")
        S = ctx.chain["S"]
        gR = torch.zeros((B, S), dtype=f32, device=dev) if gR is None else gR.float().contiguous()
        grho = torch.zeros((B, S), dtype=f32, device=dev) if grho is None else grho.float().contiguous()
        gacc = torch.zeros_like(ycls) if gacc is None else gacc.float().contiguous()
        gh = None if gscore is None or B == 1 else gscore.float().reshape(1)
        with _kernels(ctx.tp, ctx.operand):
            if ctx.long:
                dy, dy16, dR = ops.avit_pack_step_long_bwd(gx, seg, nh, pos, seg_next, src_next, sv, ycls, gR, grho, gacc, gh, G, D, gate_scale, last)
            else:
                dy, dy16, dR = ops.avit_pack_step_bwd(gx, seg, nh, pos, seg_next, src_next, sv, ycls, gR, grho, gacc, gh, G, D, gate_scale, last)
        dy._pv_bf16 = (dy16, dy._version, None)          # hand-off to the block's backward (see _bf16_grad)
        return dy, None, dR, grho, None, None, gacc, None, None, None, None, None, None, None, None, None


def avit_pack_step_train(y, c, R, rho, counter, m, acc, seg, nh, pos, gate_scale: float, gate_center: float, threshold: float, last: bool, info: dict,
                         chain: dict):
    return AViTPackStepFn.apply(y, c, R, rho, counter, m, acc, seg, nh, pos, gate_scale, gate_center, threshold, last, info, chain)


def avit_forward_packed_train(model: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """One training forward of an AdaptiveVisionTransformer on its packed live rows, inside model_forward_train's pass: embed_tokens_train, per layer
    EncoderBlockFn (avit_packed_block_forward_train) and AViTPackStepFn (one host read of the next row count), pool_and_head_train on the accumulated class rows.  Leaves behind what
    the fused dense pass leaves: encoder.rho_token and encoder.halting_score_layer entered into the (loss-scaled) chain, encoder.counter_token.  The
    caller has checked eligibility (AdaptiveVisionTransformer._packed_training_ok up to 208 tokens, _long_packed_training_ok above: the chunked pack step,
    and per layer the streaming ragged attention pair while a segment exceeds 208 rows - _RaggedAttn picks it by max_len)."""
    from . import engine
    enc = model.encoder
    n_cls, L = model.num_class_tokens, len(enc.layers)
    tokens = embed_tokens_train(model, x)
    B, S, D = tokens.shape
    dev = tokens.device
    z = torch.zeros((2, B, S), dtype=torch.float32, device=dev)
    o = torch.ones((3, B, S), dtype=torch.float32, device=dev)
    c, rho, R, counter, m = z[0], z[1], o[0], o[1], o[2]
    acc = torch.zeros((B, n_cls, D), dtype=torch.float32, device=dev)
    seg, nh, pos, rs = engine._act_initial_tables(B, S, dev)
    log_mult = torch.zeros((B * S,), dtype=torch.float32, device=dev)
    xs, max_len = tokens.reshape(B * S, D), S
    thr = float(torch.tensor(1 - enc.eps, dtype=torch.float32))     # `c > 1 - eps` compares fp32 c with the fp32-rounded scalar
    chain = {"G": None, "S": S}
    scores, rows = [], []
    for i, blk in enumerate(enc.layers):
        rows.append(int(xs.shape[0]))
        engine.avit_train_rows += rows[-1]
        engine.avit_train_dense_rows += B * S
        engine.avit_train_long_layers += max_len > engine.AVIT_RESIDENT_MAX_S
        y = avit_packed_block_forward_train(blk, xs, rs, seg, log_mult, max_len)
        info = {}
        xs, rs, c, R, rho, counter, m, acc, score = avit_pack_step_train(y, c, R, rho, counter, m, acc, seg, nh, pos, blk.gate_scale, blk.gate_center,
                                                                        thr, i == L - 1, info, chain)
        scores.append(score)
        if i < L - 1:
            seg, nh, pos, log_mult, max_len = info["seg"], info["nh"], info["pos"], info["log_mult"], info["max_len"]
    engine._region.avit_train_last_rows = rows
    enc.rho_token = enter(rho)
    enc.counter_token = counter
    enc.halting_score_layer = [enter(s) for s in scores]
    return pool_and_head_train(model, acc)
