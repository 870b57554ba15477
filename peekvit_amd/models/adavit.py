"""Adaptive Vision Transformer (A-ViT, token-level adaptive computation time) behind the reference's interface (reference models/adavit.py).

Same constructor kwargs (= configs/model/avit_*.yaml keys), same state-dict keys, same `forward(x[B,3,R,R]) -> logits[B,num_classes]`, and the
same module attributes the reference's A-ViT losses read after a forward: `encoder.rho_token`, `encoder.counter_token` ([B,S] fp32) and
`encoder.halting_score_layer` (one 0-dim tensor per layer: the mean token halting score of images 1.. - the reference slices the BATCH there,
so it is NaN at batch 1).

GPU tensors under torch.no_grad() run the "packed halting" forward of peekvit_amd.engine.avit_forward: each layer works on the LIVE token
rows only (plus one zero representative row per image with halted tokens, whose key / value stand for all of them), where the reference
runs all S rows and multiplies the halted ones by zero.  Everything else - CPU tensors, autograd, and the fallback of precision mode "auto" -
is the stock-op composite below, which restates models/adavit.py:54-219.

`set_fused_training(True)` (off by default) moves the forward under autograd on the GPU onto HIP kernels with a hand-written backward
(train_engine.EncoderBlockFn / ActStepFn); the attributes above then hold what the composite would hold, graph included.
`set_packed_training(True)` (off by default) runs that training pass on the packed live rows instead, forward and backward
(train_engine.EncoderBlockFn on the packed rows / AViTPackStepFn).
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn

from .. import engine, train_engine
from .blocks import MLP, SelfAttention
from .vit import _ViTBase


class AViTBlock(nn.Module):
    """Pre-LN block with a per-token halting score (reference models/adavit.py:22-79)."""

    def __init__(self, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float, attention_dropout: float,
                 gate_scale: float = 10, gate_center: float = 30):
        super().__init__()
        self.num_heads, self.hidden_dim, self.mlp_dim = num_heads, hidden_dim, mlp_dim
        self.gate_scale, self.gate_center = gate_scale, gate_center
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.self_attention = SelfAttention(hidden_dim, num_heads, attention_dropout)
        self.dropout = nn.Dropout(dropout)
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = MLP(hidden_dim=hidden_dim, mlp_dim=mlp_dim)

    def forward_act(self, x: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """(block output, [-1, h_token]); `mask` is 1 for HALTED tokens (the encoder passes 1 - mask_token).  The residual stream itself is not
        masked: only the LayerNorm inputs and outputs are (:64-66)."""
        bs, token, _ = x.shape
        if mask is None:
            x = x + self.self_attention(self.ln_1(x))
            x = x + self.mlp(self.ln_2(x))
        else:
            m = (1 - mask).view(bs, token, 1)
            x = x + self.self_attention(self.ln_1(x * m) * m)
            x = x + self.mlp(self.ln_2(x * m) * m)
        halting_score_token = torch.sigmoid(x[:, :, 0] * self.gate_scale - self.gate_center)
        return x, [-1, halting_score_token]


class AViTEncoder(nn.Module):
    """pos-embedding add, L AViTBlocks with token halting, final LayerNorm of the halting-weighted output (reference models/adavit.py:83-219)."""

    def __init__(self, seq_length: int, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float,
                 attention_dropout: float, eps: float = 0.01, gate_scale: float = 10, gate_center: float = 30):
        super().__init__()
        self.eps = eps
        self.pos_embedding = nn.Parameter(torch.empty(1, seq_length, hidden_dim).normal_(std=0.02))
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.ModuleList([AViTBlock(num_heads, hidden_dim, mlp_dim, dropout, attention_dropout, gate_scale, gate_center)
                                     for _ in range(num_layers)])
        self.ln = nn.LayerNorm(hidden_dim)
        self.c_token = None
        self.R_token = None
        self.mask_token = None
        self.rho_token = None
        self.counter_token = None
        self.seq_length = seq_length
        self.halting_score_layer = []

    def forward(self, input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        input = input + self.pos_embedding
        input = self.dropout(input)
        return self.forward_features_act_token(input)

    def _reset_state(self, bs: int, device) -> None:
        """The [B,S] buffers, re-made when the batch size (or device) changes (:146-151, on the input's device instead of .cuda())."""
        shape = (bs, self.seq_length)
        if self.c_token is None or bs != self.c_token.size()[0] or self.c_token.device != device or \
                getattr(self.rho_token, "shape", None) != shape or getattr(self.counter_token, "shape", None) != shape:
            # (also when the packed HIP forward left rho / counter of another batch size behind)
            self.c_token = torch.zeros(bs, self.seq_length, device=device)
            self.R_token = torch.ones(bs, self.seq_length, device=device)
            self.mask_token = torch.ones(bs, self.seq_length, device=device)
            self.rho_token = torch.zeros(bs, self.seq_length, device=device)
            self.counter_token = torch.ones(bs, self.seq_length, device=device)

    def forward_features_act_token(self, x: torch.Tensor):
        bs = x.size()[0]
        self._reset_state(bs, x.device)
        c_token = self.c_token.clone()
        R_token = self.R_token.clone()
        mask_token = self.mask_token.clone()
        self.rho_token = self.rho_token.detach() * 0.
        self.counter_token = self.counter_token.detach() * 0 + 1.
        output = None
        out = x
        self.halting_score_layer = []
        S = self.seq_length
        for i, adaptive_layer in enumerate(self.layers):
            out.data = out.data * mask_token.float().view(bs, S, 1)
            block_output, h_lst = adaptive_layer.forward_act(out, 1. - mask_token.float())
            self.halting_score_layer.append(torch.mean(h_lst[1][1:]))
            out = block_output.clone()
            _, h_token = h_lst
            block_output = block_output * mask_token.float().view(bs, S, 1)
            if i == len(self.layers) - 1:
                h_token = torch.ones(bs, S, device=x.device)
            c_token = c_token + h_token
            self.rho_token = self.rho_token + mask_token.float()
            # case 1: threshold reached in this layer
            reached_token = c_token > 1 - self.eps
            reached_token = reached_token.float() * mask_token.float()
            delta1 = block_output * R_token.view(bs, S, 1) * reached_token.view(bs, S, 1)
            self.rho_token = self.rho_token + R_token * reached_token
            # case 2: threshold not reached
            not_reached_token = c_token < 1 - self.eps
            not_reached_token = not_reached_token.float()
            R_token = R_token - (not_reached_token.float() * h_token)
            delta2 = block_output * h_token.view(bs, S, 1) * not_reached_token.view(bs, S, 1)
            self.counter_token = self.counter_token + not_reached_token
            mask_token = c_token < 1 - self.eps
            output = delta1 + delta2 if output is None else output + (delta1 + delta2)
        return self.ln(output)


class AdaptiveVisionTransformer(_ViTBase):
    """A-ViT classifier (reference models/adavit.py:224-409)."""

    def __init__(self, image_size: int, patch_size: int, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int,
                 dropout: float = 0.0, attention_dropout: float = 0.0, num_classes: int = 1000, representation_size: Optional[int] = None,
                 num_registers: int = 0, num_class_tokens: int = 1, eps: float = 0.01, gate_scale: float = 10, gate_center: float = 30,
                 torch_pretrained_weights: Optional[str] = None, timm_pretrained_weights: Optional[List] = None):
        super().__init__()
        seq_length = self._init_stem(image_size, patch_size, hidden_dim, mlp_dim, dropout, attention_dropout,
                                     num_classes, representation_size, num_heads, num_registers, num_class_tokens)
        self.num_layers = num_layers
        self.eps, self.gate_scale, self.gate_center = eps, gate_scale, gate_center
        if num_registers > 0:
            self.register_tokens = nn.Parameter(torch.zeros(1, num_registers, hidden_dim))
            seq_length += num_registers
        self.encoder = AViTEncoder(seq_length, num_layers, num_heads, hidden_dim, mlp_dim, dropout, attention_dropout, eps,
                                   gate_scale, gate_center)
        self.seq_length = seq_length
        self._init_head()
        self.load_weights(torch_pretrained_weights, timm_pretrained_weights)
        # the packed forward's shapes depend on the data (rows still running per layer): never captured as a hipGraph (peekvit_amd.autograph)
        object.__setattr__(self, "_pv_no_autograph", True)
        object.__setattr__(self, "_pv_act", True)          # engine.run_guarded: images whose depths differ from the probe are act_depth_flips

    def set_fused_training(self, on: bool = True):
        """Opt in: under autograd on the GPU the whole forward runs as one training pass on HIP kernels with a hand-written backward - the ViT's
        stem, per layer train_engine.EncoderBlockFn and train_engine.ActStepFn (the halting step: one kernel forward, one backward), final LayerNorm
        and head on the accumulated class rows.  16-bit operands (fp16 with the loss scale in precision mode "auto", bf16 in
        mode "bf16"), so a token within the operand error of the halting threshold can stop a layer earlier or later than in the fp32 composite.
        Up to the resident attention backward's rows (208, 416 at head dim 32: `_fused_training_ok`) and from there to 4096 tokens
        (`_long_fused_training_ok`, DESIGN.md section 36: the same pass, whose blocks pick the streaming attention pair), head dims 32, 48 and 64.
        Off by default; CPU tensors, dropout, mode "bf16x3", unsupported shapes and `encoder(...)` called on its own keep the composite, and so
        does every forward with the switch off.  No parameter, buffer or state-dict key."""
        object.__setattr__(self, "_pv_fused_training", bool(on))

    def set_packed_training(self, on: bool = True):
        """Opt in: the training pass of set_fused_training on the PACKED live rows - every layer runs the tokens still
        running plus one representative row per image for the halted ones, forward and backward (train_engine.avit_forward_packed_train), with one
        host read of the row count per layer.  Needs what set_fused_training needs plus head dim 64 and at most 16 class tokens (the ragged
        attention kernels' limits).  Up to 208 tokens every layer runs the LDS-resident kernels (`_packed_training_ok`); from 209 to 4096 tokens
        (`_long_packed_training_ok`) the halting step and its backward are the chunked ones and every layer picks its
        attention pair by its own longest segment - streaming above 208 rows, resident once halting has cut every image down to 208
        (`engine.avit_train_long_layers` counts the layers that streamed).  A forward that is not eligible takes the fused dense path if that
        switch is on too, else the composite.  Off by default; no parameter, buffer or state-dict key."""
        object.__setattr__(self, "_pv_packed_training", bool(on))

    def _packed_training_ok(self) -> bool:
        return (train_engine.supported(self.hidden_dim, self.num_heads, self.seq_length) and self.hidden_dim // self.num_heads == 64
                and self.seq_length <= 208 and self.num_class_tokens <= 16 and len(self.encoder.layers) > 0)

    def _fused_training_ok(self) -> bool:
        """The fused dense pass keeps the resident attention pair's rows (208, 416 at head dim 32): the bound is this path's own, stated here."""
        return (train_engine.supported(self.hidden_dim, self.num_heads, self.seq_length)
                and self.seq_length <= train_engine.resident_rows(self.hidden_dim // self.num_heads))

    def _long_packed_training_ok(self) -> bool:
        """`_packed_training_ok` past its 208 tokens, up to the chunked halting step's 4096 (pv_avit_pack_step_long): a rule of its own, so the
        resident rule keeps meaning the resident kernels."""
        return (train_engine.supported(self.hidden_dim, self.num_heads, self.seq_length) and self.hidden_dim // self.num_heads == 64
                and 208 < self.seq_length <= 4096 and self.num_class_tokens <= 16 and len(self.encoder.layers) > 0)

    def _long_fused_training_ok(self) -> bool:
        """The fused dense pass past the resident attention pair's rows: nothing below the rule is bounded by them (EncoderBlockFn picks its pair
        through train_engine.attention_pair, the halting kernels take 4096 rows)."""
        return (train_engine.supported(self.hidden_dim, self.num_heads, self.seq_length)
                and train_engine.resident_rows(self.hidden_dim // self.num_heads) < self.seq_length <= 4096)

    def _packed_train_forward(self, x: torch.Tensor) -> torch.Tensor:
        with engine.on_device(x):
            return train_engine.model_forward_train(self, x, lambda: train_engine.avit_forward_packed_train(self, x))

    def _fused_train_forward(self, x: torch.Tensor) -> torch.Tensor:
        enc = self.encoder
        n_cls, L = self.num_class_tokens, len(enc.layers)

        def body():
            tokens = train_engine.embed_tokens_train(self, x)
            B, S, D = tokens.shape
            z = torch.zeros((2, B, S), dtype=torch.float32, device=tokens.device)
            o = torch.ones((3, B, S), dtype=torch.float32, device=tokens.device)
            c, rho, R, counter, m = z[0], z[1], o[0], o[1], o[2]
            acc = torch.zeros((B, n_cls, D), dtype=torch.float32, device=tokens.device)
            scores = []
            for i, blk in enumerate(enc.layers):
                y = train_engine.avit_block_forward_train(blk, tokens, m)
                tokens, c, R, rho, counter, m, acc, score = train_engine.act_step_train(y, c, R, rho, counter, m, acc, blk.gate_scale, blk.gate_center,
                                                                                        1.0 - enc.eps, i == L - 1)
                scores.append(score)
            # what the composite leaves behind for the A-ViT losses: their gradients enter the (loss-scaled) HIP chain here
            enc.rho_token = train_engine.enter(rho)
            enc.counter_token = counter
            enc.halting_score_layer = [train_engine.enter(s) for s in scores]
            return train_engine.pool_and_head_train(self, acc)

        with engine.on_device(x):
            return train_engine.model_forward_train(self, x, body)

    def forward(self, x: torch.Tensor):
        self._check_image(x)
        if x.shape[0] == 0:
            return x.new_zeros((0, self.num_classes), dtype=torch.float32)
        packed, fused = getattr(self, "_pv_packed_training", False), getattr(self, "_pv_fused_training", False)
        if (packed or fused) and train_engine.train_eligible(x, self, max(self.dropout, self.attention_dropout)):
            if packed and (self._packed_training_ok() or self._long_packed_training_ok()):
                return self._packed_train_forward(x)
            if fused and (self._fused_training_ok() or self._long_fused_training_ok()):
                return self._fused_train_forward(x)
        if engine.backend_for(x, self, max(self.dropout, self.attention_dropout)) == "hip":
            # the self-check compares the logits of the images whose per-token depths (counter_token) agree with the probe's
            return engine.run_guarded(self, x, lambda: self._hip_forward(x), probe=self._hip_forward,
                                      probe_state=lambda: [self.encoder.counter_token])
        return self._composite_forward(x)

    def _composite_forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._composite_head(self.encoder(self._composite_tokens(x)))

    def _hip_forward(self, x: torch.Tensor) -> torch.Tensor:
        if engine._mode() == "bf16x3":
            # there is no split-precision packed forward: the guard's fallback (and its self-check reference) is the composite, on the GPU
            return self._composite_forward(x)
        return engine.avit_forward(self, x)
