"""Residual-gated ViT with one early-exit head per layer behind the reference's interface (reference models/eeresidualvit.py).

Same constructor kwargs (= configs/model/eeresidualvit.yaml keys), same state-dict keys, same `forward(x[B,3,R,R]) -> [exit_0, ..., exit_{L-1},
final]`: a Python list of L + 1 logit tensors, the exits squeezed as the reference squeezes them ((classes,) at batch 1, the final (1, classes)).
The blocks are this package's ResidualViTBlock, unchanged.  The model does NOT hand num_class_tokens / num_registers to its encoder (the
reference does not either): every block sees one special token and every exit head reads row 0, whatever the model was built with; the
final head still sums num_class_tokens rows.  `current_budget` is a plain float, one budget for the whole batch.

The reference computes every layer for every image and leaves the choice of exit to the caller.  `select_exits` defines that choice once, on
the list (the first checked exit whose max softmax reaches the threshold, else the final head), and `model.early_exit(x, threshold)` is the
same decision taken while the forward runs: on GPU tensors under torch.no_grad() the images that exit leave the batch and the later layers
run on the images that are left (peekvit_amd.engine.ee_forward_exit, include/peekvit_hip_ee.h).  Everything else - CPU tensors, autograd,
train mode, configurations the kernels do not take (engine.ee_supported) and the fallback of precision mode "auto" - is the stock-op
composite below, which restates models/eeresidualvit.py:17-362.
"""
from __future__ import annotations

from typing import List, Literal, NamedTuple, Optional, Sequence, Union

import torch
from torch import nn

from .. import engine
from .residualvit import ResidualViTBlock
from .vit import _ViTBase, _make_layers


class EarlyExitResult(NamedTuple):
    """logits [B, C] of each image's exit, exit_layer int64 [B] (L = the final head), confidence [B] (max softmax of that row).  `live`:
    set by the shrinking-batch forward only - per layer that ran, the original indices of the images it ran on (block i's `mask` covers them)."""
    logits: torch.Tensor
    exit_layer: torch.Tensor
    confidence: torch.Tensor
    live: Optional[list] = None


def _max_softmax(o: torch.Tensor) -> torch.Tensor:
    o = o if o.dtype in (torch.float32, torch.float64) else o.float()
    return torch.softmax(o, dim=-1).max(dim=-1).values


def select_exits(outs: Sequence[torch.Tensor], threshold: float, exit_layers: Optional[Sequence[int]] = None) -> EarlyExitResult:
    """The early-exit decision on a forward's output list [exit_0, ..., exit_{L-1}, final]: image b takes the smallest i in `exit_layers`
    (default: every layer) with max softmax(outs[i][b]) >= threshold, else L (the final head).  Softmax in fp32 (fp64 for fp64 lists) with
    the row maximum subtracted."""
    L = len(outs) - 1
    C = outs[-1].shape[-1]
    rows = [o.reshape(-1, C) for o in outs]                       # (the batch-1 squeeze of the exits undone)
    layers = sorted(range(L) if exit_layers is None else {int(i) for i in exit_layers})
    if any(i < 0 or i >= L for i in layers):
        raise ValueError(f"exit_layers must lie in [0, {L}), got {list(exit_layers)}")
    B = rows[-1].shape[0]
    logits = rows[L].clone()
    conf = _max_softmax(rows[L])
    layer = torch.full((B,), L, dtype=torch.int64, device=logits.device)
    undecided = torch.ones(B, dtype=torch.bool, device=logits.device)
    for i in layers:
        c = _max_softmax(rows[i])
        hit = undecided & (c >= threshold)
        logits[hit] = rows[i][hit].to(logits.dtype)
        conf[hit] = c[hit].to(conf.dtype)
        layer[hit] = i
        undecided &= ~hit
    return EarlyExitResult(logits, layer, conf)


def _worst_slice_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    """The self-check's measure for this model: the largest relative L2 over the LAST-dimension rows' groups - per list element for the
    stacked list [k, L + 1, C] (reduced over images and classes), per image for early-exit logits [k, C]."""
    dims = (0, 2) if got.dim() == 3 else (1,)
    num = (got - ref).double().pow(2).sum(dim=dims).sqrt()
    den = ref.double().pow(2).sum(dim=dims).sqrt()
    ok = den > 0
    return float((num[ok] / den[ok]).max()) if bool(ok.any()) else 0.0


class EEResidualViTEncoder(nn.Module):
    """pos-embedding add, L residual blocks each followed by its exit head on row 0, final LayerNorm (reference models/eeresidualvit.py:17-96)."""

    def __init__(self, seq_length: int, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float,
                 attention_dropout: float, residual_layers: Optional[List] = None, add_input: bool = False,
                 num_class_tokens: int = 1, num_registers: int = 0, gate_type: Literal['gumbel', 'sigmoid'] = 'gumbel',
                 gate_temp: float = 1.0, gate_bias: float = 10.0, gate_threshold: float = 0.5,
                 budget_token: Union[bool, List, Literal['learnable']] = False, num_classes: int = 10):
        super().__init__()
        self.num_layers = num_layers
        self.num_class_tokens, self.num_registers = num_class_tokens, num_registers
        self.num_special_tokens = num_class_tokens + num_registers
        self.budget_token = budget_token
        self.num_classes = num_classes
        self.num_budget_tokens = 0 if not budget_token else 1
        self.pos_embedding = nn.Parameter(torch.empty(1, seq_length, hidden_dim).normal_(std=0.02))
        self.dropout = nn.Dropout(dropout)
        self.layers = _make_layers(
            lambda i: ResidualViTBlock(num_heads, hidden_dim, mlp_dim, dropout, attention_dropout,
                                       skip=residual_layers[i], add_input=add_input,
                                       num_class_tokens=num_class_tokens, num_registers=num_registers,
                                       gate_type=gate_type, temp=gate_temp, gate_bias=gate_bias,
                                       gate_threshold=gate_threshold, budget_token=budget_token), num_layers)
        self.ln = nn.LayerNorm(hidden_dim)
        self.early_exit_heads = nn.ModuleList([nn.Sequential(nn.LayerNorm(hidden_dim), nn.Linear(hidden_dim, self.num_classes))
                                               for _ in range(num_layers)])

    def forward(self, input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        if self.budget_token:
            body, btok = input[:, :-self.num_budget_tokens], input[:, -self.num_budget_tokens:]
            input = torch.cat([body + self.pos_embedding, btok], dim=1)
        else:
            input = input + self.pos_embedding
        input = self.dropout(input)
        early_exits = []
        for i in range(self.num_layers):
            input = self.layers[i](input)
            early_exits.append(self.early_exit_heads[i](input[:, 0:self.num_class_tokens]).squeeze())
        return self.ln(input), early_exits


class EEResidualVisionTransformer(_ViTBase):
    """reference models/eeresidualvit.py:100-362."""

    def __init__(self, image_size: int, patch_size: int, num_layers: int, num_heads: int, hidden_dim: int,
                 mlp_dim: int, dropout: float = 0.0, attention_dropout: float = 0.0, num_classes: int = 1000,
                 representation_size: Optional[int] = None, num_registers: int = 0,
                 residual_layers: Optional[List] = None, add_input: bool = False, num_class_tokens: int = 1,
                 gate_type: Literal['gumbel', 'sigmoid'] = 'gumbel', gate_temp: float = 1.0, gate_bias: float = 10.0,
                 gate_threshold: float = 0.5,
                 add_budget_token: Union[bool, List, Literal['learnable', 'learnable_interpolate']] = False):
        super().__init__()
        seq_length = self._init_stem(image_size, patch_size, hidden_dim, mlp_dim, dropout, attention_dropout,
                                     num_classes, representation_size, num_heads, num_registers, num_class_tokens)
        self.num_layers = num_layers
        self.budget = add_budget_token
        self.add_budget_token = add_budget_token               # (the name peekvit_amd.flops and the harness read on the residual models)
        self.current_budget = None
        self.gate_temp, self.gate_bias = gate_temp, gate_bias
        self.residual_layers = residual_layers or ['attention+mlp'] * num_layers
        if num_registers > 0:
            self.register_tokens = nn.Parameter(torch.zeros(1, num_registers, hidden_dim))
            seq_length += num_registers
        self.num_special_tokens = num_class_tokens + num_registers
        # num_class_tokens / num_registers are NOT passed on (models/eeresidualvit.py:192-208): the encoder and its blocks keep their defaults
        self.encoder = EEResidualViTEncoder(seq_length, num_layers, num_heads, hidden_dim, mlp_dim, dropout, attention_dropout,
                                            residual_layers=self.residual_layers, add_input=add_input, gate_type=gate_type,
                                            gate_temp=gate_temp, gate_bias=gate_bias, gate_threshold=gate_threshold,
                                            budget_token=add_budget_token, num_classes=num_classes)
        self.seq_length = seq_length
        if self.budget:
            self.num_budget_tokens = 1
        if self.budget == 'learnable' or self.budget == 'learnable_interpolate':
            self.learnable_budget_token_1 = nn.Parameter(torch.randn(1, 1, hidden_dim))
            # both exist in either mode (:216-219); 'learnable' only uses the first
            self.learnable_budget_token_2 = nn.Parameter(torch.randn(1, 1, hidden_dim))
        self._init_head()
        # the shrinking-batch forward's shapes depend on the data: never captured as a hipGraph (peekvit_amd.autograph)
        object.__setattr__(self, "_pv_no_autograph", True)
        object.__setattr__(self, "_pv_ee_last", None)
        # early_exit's result is more than the logits tensor (exit layers, confidences, live lists): never on the deferred-flag path, where a
        # guard trip found later would replace the logits alone
        object.__setattr__(self, "_pv_no_defer", True)
        object.__setattr__(self, "_pv_flip_what", "took a different exit layer than the {} arithmetic (a confidence within operand rounding of the threshold)")

    # -- budget token (models/eeresidualvit.py:254-327) --------------------------------------------------------
    def _eval_budget(self):
        if not getattr(self, 'current_budget', False):          # (truthiness, as the reference: budget 0.0 raises too)
            raise ValueError('Budget token not set. Call set_budget() before forward() to evaluate the model on a chosen budget.')
        return self.current_budget

    def _add_budget_token(self, x: torch.Tensor) -> torch.Tensor:
        n = x.shape[0]
        if self.training:
            if isinstance(self.budget, float):
                self.current_budget = self.budget
            elif isinstance(self.budget, (list, tuple)):
                self.current_budget = self.budget[torch.randint(0, len(self.budget), (1,)).item()]
            elif isinstance(self.budget, bool):
                self.current_budget = torch.rand(1, device=x.device).item()
            else:
                self.current_budget = torch.rand(1, device=x.device).item()
        else:
            self._eval_budget()
        if self.budget == 'learnable':
            return torch.cat([x, self.current_budget * self.learnable_budget_token_1.expand(n, -1, -1)], dim=1)
        if self.budget == 'learnable_interpolate':
            return torch.cat([x, self.current_budget * self.learnable_budget_token_1.expand(n, -1, -1)
                              + (1 - self.current_budget) * self.learnable_budget_token_2.expand(n, -1, -1)], dim=1)
        budget_token = torch.empty((n, 1, self.hidden_dim), device=x.device).fill_(self.current_budget)
        self.current_budget = budget_token.mean().item()
        return torch.cat([x, budget_token], dim=1)

    def set_budget(self, budget: float):
        self.current_budget = budget

    # -- forward -------------------------------------------------------------------------------------------------
    def _composite_forward(self, x: torch.Tensor) -> list:
        tokens = self._composite_tokens(x)
        if self.budget:
            tokens = self._add_budget_token(tokens)
        enc, early_exits = self.encoder(tokens)
        return early_exits + [self._composite_head(enc)]

    def _hip_eligible(self, x: torch.Tensor) -> bool:
        return (not self.training and x.dim() == 4 and x.shape[0] > 0 and engine.ee_supported(self)
                and engine.backend_for(x, self, max(self.dropout, self.attention_dropout)) == "hip")

    def _stacked_composite(self, x: torch.Tensor) -> torch.Tensor:
        outs = self._composite_forward(x)
        return torch.stack([o.reshape(x.shape[0], -1) for o in outs], dim=1)

    def _hip_list(self, x: torch.Tensor) -> torch.Tensor:
        """[B, L + 1, C].  Mode "bf16x3" (the guard's fallback and its self-check reference) is the composite, on the GPU."""
        if engine._mode() == "bf16x3":
            return self._stacked_composite(x)
        return engine.ee_forward(self, x)

    def forward(self, x: torch.Tensor):
        self._check_image(x)
        if self._hip_eligible(x):
            if self.budget:
                self._eval_budget()
            out = engine.run_guarded(self, x, lambda: self._hip_list(x), probe=self._hip_list, probe_key=("list", self.current_budget),
                                     probe_metric=_worst_slice_error)
            L = out.shape[1] - 1
            return [out[:, i].squeeze() for i in range(L)] + [out[:, L]]
        return self._composite_forward(x)

    def _hip_exit(self, x: torch.Tensor, threshold: float, exit_layers) -> torch.Tensor:
        if engine._mode() == "bf16x3":
            res = select_exits(self._composite_forward(x), threshold, exit_layers)
            object.__setattr__(self, "_pv_ee_last", (res.exit_layer, res.confidence, None))
            return res.logits
        return engine.ee_forward_exit(self, x, threshold, exit_layers)

    def early_exit(self, x: torch.Tensor, threshold: float, exit_layers: Optional[Sequence[int]] = None) -> EarlyExitResult:
        """select_exits(self(x), threshold, exit_layers) - on the MI355X path taken while the forward runs: the images that exit leave the
        batch, and the layers behind a checked layer run on the survivors only."""
        self._check_image(x)
        L = len(self.encoder.layers)
        layers = None if exit_layers is None else tuple(sorted({int(i) for i in exit_layers}))
        if layers is not None and any(i < 0 or i >= L for i in layers):
            raise ValueError(f"exit_layers must lie in [0, {L}), got {list(exit_layers)}")
        if not self._hip_eligible(x):
            return select_exits(self(x), threshold, layers)
        if self.budget:
            self._eval_budget()
        threshold = float(threshold)
        fn = lambda xs: self._hip_exit(xs, threshold, layers)      # noqa: E731
        # the self-check compares the logits of the images whose exit layer agrees with the probe's
        logits = engine.run_guarded(self, x, lambda: fn(x), probe=fn, probe_key=("exit", self.current_budget, threshold, layers),
                                    probe_state=lambda: [self._pv_ee_last[0]], probe_metric=_worst_slice_error)
        layer, conf, lives = self._pv_ee_last
        return EarlyExitResult(logits, layer, conf, lives)
