"""Vision Transformer with mixture-of-experts layers behind the reference's interface (reference models/moevit.py, VisionTransformerMoE).

Same constructor kwargs (= configs/model/moevit.yaml keys), same state-dict keys, same `forward(x[B,3,R,R]) -> logits[B,num_classes]`, and the
attribute the reference's utils read after a forward (utils/utils.py:57-94 get_moes / get_last_forward_gates): every `MoE` module with more
than one expert holds `gating_probs`, the one-hot fp32 routing [B, S, E] of its last forward.  `mlp_moes` / `attn_moes` are PER-LAYER EXPERT
COUNTS (the reference's docstring calls them layer indices; its code uses them as counts); None means 1 everywhere.  A half with one expert is
the plain MLP / SelfAttention, ungated, but its gate parameters exist as in the reference.  `MoEVisionTransformer` is an alias: the
reference's own configs/model/moevit.yaml names that class, which the reference does not define.

GPU tensors under torch.no_grad() run peekvit_amd.engine.moe_forward: a layer whose halves have one expert each is the ViT block, a routed
half runs each token through its own expert only (pv_moe_route + pv_gemm_grouped_bf16, include/peekvit_hip_moe.h) where the reference runs
every expert on every token and multiplies by the one-hot.  Everything else - CPU tensors, autograd (Gumbel noise in training), precision
mode "bf16x3", a guard trip in mode "auto" and shapes the kernels do not take (engine.moe_supported) - is the stock-op composite below, which
restates models/moevit.py:19-110.
"""
from __future__ import annotations

from abc import ABC
from typing import List, Optional

import torch
from torch import nn

from .. import engine
from .blocks import MLP, GumbelSoftmax, SelfAttention
from .vit import _ViTBase


class MoE(ABC, nn.Module):
    """Marker base class of the mixture-of-experts modules (reference models/moevit.py:19-20): utils/utils.py finds them by isinstance."""


class TopKGate(nn.Module):
    """Linear gate + hard Gumbel softmax: one-hot routing (reference models/moevit.py:23-33)."""

    def __init__(self, input_dim, num_experts):
        super().__init__()
        self.gate = nn.Linear(input_dim, num_experts)
        self.activation = GumbelSoftmax(dim=-1, hard=True)

    def forward(self, x):
        return self.activation(self.gate(x))


class _ExpertsMoE(MoE):
    def forward_one(self, x):
        return self.experts[0](x)

    def forward_moe(self, x):
        torch._assert(x.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {x.shape}")
        self.gating_probs = self.gating_network(x)                                   # batch, seq, experts
        out = torch.stack([expert(x) for expert in self.experts], dim=0)             # every expert on every token, as the reference
        return torch.einsum("ebsd, bse -> bsd", out, self.gating_probs)

    def forward(self, x):
        return self.forward_one(x) if self.num_experts == 1 else self.forward_moe(x)


class MLPMoE(_ExpertsMoE):
    """Mixture of MLP experts (reference models/moevit.py:37-67)."""

    def __init__(self, hidden_dim, mlp_dim, num_experts):
        super().__init__()
        self.gating_network = TopKGate(hidden_dim, num_experts)
        self.num_experts = num_experts
        self.experts = nn.ModuleList([MLP(hidden_dim, mlp_dim) for _ in range(num_experts)])


class AttentionMoE(_ExpertsMoE):
    """Mixture of self-attention experts (reference models/moevit.py:71-102): a routed token's query attends to ITS expert's keys and values
    of all tokens of the image."""

    def __init__(self, input_dim, num_heads, num_experts, dropout=0.0):
        super().__init__()
        self.gating_network = TopKGate(input_dim, num_experts)
        self.num_experts = num_experts
        self.experts = nn.ModuleList([SelfAttention(input_dim, num_heads=num_heads, dropout=dropout) for _ in range(num_experts)])


class _PlainView:
    """The attribute layout engine.block_forward reads (ln_1, self_attention.self_attention, mlp.fc1 / fc2) over a one-expert-per-half block."""
    __slots__ = ("ln_1", "ln_2", "self_attention", "mlp")

    def __init__(self, blk):
        self.ln_1, self.ln_2 = blk.ln_1, blk.ln_2
        self.self_attention, self.mlp = blk.self_attention.experts[0], blk.mlp.experts[0]


class ViTBlockMoE(nn.Module):
    """Pre-LN block whose attention and / or MLP half is a mixture of experts (reference models/moevit.py:106-140)."""

    def __init__(self, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float, attention_dropout: float,
                 mlp_num_experts: int = 1, attn_num_experts: int = 1):
        super().__init__()
        self.num_heads = num_heads
        self._p_drop = max(float(dropout), float(attention_dropout))
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.self_attention = AttentionMoE(hidden_dim, num_heads, attn_num_experts, attention_dropout)
        self.dropout = nn.Dropout(dropout)
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = MLPMoE(hidden_dim=hidden_dim, mlp_dim=mlp_dim, num_experts=mlp_num_experts)
        # engine.run_layers hints, as on ViTBlock (plain attributes, never registered submodules)
        object.__setattr__(self, "_pv_next_ln", None)
        object.__setattr__(self, "_pv_next_ranks", False)

    def _pv_plain(self) -> bool:
        return self.self_attention.num_experts == 1 and self.mlp.num_experts == 1

    def _pv_plain_ln1(self) -> bool:
        """A one-expert block applies ln_1 to its input like a ViTBlock (a producer may hand it over); a routed block normalises itself."""
        return self._pv_plain()

    def _pv_forward_rows(self, input: torch.Tensor, nq: int):
        """Last block of a model forward: the class rows only (engine.block_forward_rows), for a one-expert block; None otherwise."""
        if not self._pv_plain() or input.dim() != 3 or not engine.rows_only_ok(self) or engine.backend_for(input, self, self._p_drop) != "hip":
            return None
        return engine.run_guarded(self, input, lambda: engine.block_forward_rows(_PlainView(self), input, self.ln_1.eps, nq))

    def _composite(self, input: torch.Tensor) -> torch.Tensor:
        x = self.dropout(self.self_attention(self.ln_1(input))) + input
        return x + self.mlp(self.ln_2(x))

    def forward(self, input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        if engine.backend_for(input, self, self._p_drop) == "hip":
            if self._pv_plain():
                return engine.run_guarded(self, input, lambda: engine.block_forward(_PlainView(self), input, self.ln_1.eps,
                                                                                  next_ln=self._pv_next_ln, next_ranks=self._pv_next_ranks))
            if engine._mode() != "bf16x3" and engine.moe_supported(self):
                return engine.run_guarded(self, input, lambda: engine.moe_block_forward(self, input))
        return self._composite(input)


class ViTEncoderMoE(nn.Module):
    """pos-embedding add, L ViTBlockMoE, final LayerNorm (reference models/moevit.py:144-189)."""

    def __init__(self, seq_length: int, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float,
                 attention_dropout: float, mlp_moes: List = None, attn_moes: List = None):
        super().__init__()
        self.mlp_moes = mlp_moes or [1] * num_layers
        self.attn_moes = attn_moes or [1] * num_layers
        self.pos_embedding = nn.Parameter(torch.empty(1, seq_length, hidden_dim).normal_(std=0.02))
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.Sequential(*[ViTBlockMoE(num_heads, hidden_dim, mlp_dim, dropout, attention_dropout,
                                                  mlp_num_experts=self.mlp_moes[i], attn_num_experts=self.attn_moes[i])
                                      for i in range(num_layers)])
        self.ln = nn.LayerNorm(hidden_dim)

    def forward(self, input: torch.Tensor, _pos_added: bool = False, _rows: int = 0):
        """`_pos_added` / `_rows`: private to this package, as on ViTEncoder (the fused patch embedding added pos_embedding; the caller
        reads rows [0, _rows) of every image only)."""
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        if _pos_added:
            return engine.run_layers(self.layers, input, last_rows=_rows)
        return self.ln(self.layers(self.dropout(input + self.pos_embedding)))

    def _composite(self, input: torch.Tensor) -> torch.Tensor:
        x = self.dropout(input + self.pos_embedding)
        for blk in self.layers:
            x = blk._composite(x)
        return self.ln(x)


class VisionTransformerMoE(_ViTBase):
    """ViT classifier with mixture-of-experts layers (reference models/moevit.py:193-312)."""

    def __init__(self, image_size: int, patch_size: int, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int,
                 dropout: float = 0.0, attention_dropout: float = 0.0, num_classes: int = 1000, representation_size: Optional[int] = None,
                 mlp_moes: List = None, attn_moes: List = None):
        super().__init__()
        torch._assert(image_size % patch_size == 0, "Input shape indivisible by patch size!")
        self.image_size, self.patch_size = image_size, patch_size
        self.hidden_dim, self.mlp_dim = hidden_dim, mlp_dim
        self.attention_dropout, self.dropout = attention_dropout, dropout
        self.num_classes, self.representation_size = num_classes, representation_size
        self.num_heads = num_heads
        self.num_layers = num_layers
        self.mlp_moes = mlp_moes or [1] * num_layers
        self.attn_moes = attn_moes or [1] * num_layers
        self.num_registers, self.num_class_tokens = 0, 1            # (the shared stem / head plumbing of _ViTBase reads these)
        self.conv_proj = nn.Conv2d(in_channels=3, out_channels=hidden_dim, kernel_size=patch_size, stride=patch_size)
        seq_length = (image_size // patch_size) ** 2
        self.class_token = nn.Parameter(torch.zeros(1, 1, hidden_dim))
        seq_length += 1
        self.encoder = ViTEncoderMoE(seq_length, num_layers, num_heads, hidden_dim, mlp_dim, dropout, attention_dropout, mlp_moes, attn_moes)
        self.seq_length = seq_length
        self._init_head()
        # a routed forward decides per token which weights run; the MoE modules' gating_probs are per forward.  Such a model is never
        # captured by the automatic hipGraph path (explicit peekvit_amd.graph.GraphedForward capture works: the forward has no host read)
        object.__setattr__(self, "_pv_no_autograph", any(e > 1 for e in self.mlp_moes + self.attn_moes))

    @property
    def class_tokens(self) -> torch.Tensor:
        """The reference's `class_token` under the name the shared ViT plumbing (stem, engine.embed_tokens) reads."""
        return self.class_token

    def moes(self):
        """The MoE modules with more than one expert, in module order (what utils/utils.py get_moes collects)."""
        return [m for m in self.modules() if isinstance(m, MoE) and m.num_experts > 1]

    def forward(self, x: torch.Tensor):
        self._check_image(x)
        if x.shape[0] == 0:
            return x.new_zeros((0, self.num_classes), dtype=torch.float32)
        if engine.backend_for(x, self, max(self.dropout, self.attention_dropout)) == "hip":
            moes = self.moes()
            if not moes:               # every layer is a ViT block: the ViT forward, launch for launch
                return engine.run_guarded(self, x, lambda: engine.forward_split(x, self._hip_forward), probe=self._hip_forward)
            # the self-check compares the logits of the images whose routing agrees with the probe's
            return engine.run_guarded(self, x, lambda: self._hip_forward(x), probe=self._hip_forward,
                                      probe_state=lambda: [m.gating_probs.argmax(-1) for m in moes])
        return self._composite_forward(x)

    def _composite_forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._composite_head(self.encoder._composite(self._composite_tokens(x)))

    def _hip_forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.moes() and (engine._mode() == "bf16x3" or not engine.moe_supported(self)):
            # no split-precision routed forward: the guard's fallback (and its self-check reference) is the composite, on the GPU
            return self._composite_forward(x)
        return engine.moe_forward(self, x)


MoEVisionTransformer = VisionTransformerMoE
