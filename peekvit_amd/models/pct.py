"""Point-cloud transformers behind the reference's interface (reference models/pct.py PointCloudTransformer, models/rankpct.py
RankPointCloudTransformer).

Same constructor (names, order, defaults), same state-dict keys, `forward(x[B,N,3]) -> logits[B,num_classes]`.  What the reference does and this
module restates without "fixing" it:

  * `PCTBlock` adds its residuals to the LayerNorm OUTPUT: `x = ln_1(input); x = attn(x) + x; x = mlp(ln_2(x)) + x` (models/pct.py:49-51);
  * there is no positional embedding and no final encoder LayerNorm;
  * `class_tokens` is a parameter the forward never uses; `registers` are prepended; the pooled vector is the mean over ALL rows;
  * the head is `lin2(dropout(gelu(bn1(lin1(x)))))` with dropout 0.5;
  * the stem `ARPE` takes k = int(32 * num_points / 512) nearest neighbours of every point (the point itself included).  The reference calls
    pytorch3d's `knn_points`, whose import it has commented out, so it does not run as shipped; `knn_indices` below is the k-NN used here:
    squared distances from the coordinate differences, (dx*dx + dy*dy) + dz*dz in fp32, exact ties to the lowest index;
  * the reference's configs/model/pct.yaml names `peekvit.models.rankpct.PointCloudTransformer`, which the reference does not define:
    `peekvit.models.rankpct` exports this module's class under that name too.

GPU tensors in eval mode under torch.no_grad() run peekvit_amd.engine.pct_forward: the stem is ONE launch (pv_arpe_embed: nothing but the
[B, N, D] tokens reaches memory), the encoder runs on the GEMM and attention kernels of the image models.  Everything else - CPU tensors,
autograd, train mode (batch-statistics BatchNorm, dropout), precision mode "bf16x3", a guard trip in mode "auto" and shapes the kernels do
not take (engine.pct_supported) - is the stock-op composite below, with one exception:

GPU tensors under autograd (train mode, or eval mode with grads on: fine-tuning with frozen BatchNorm) run the PAIR STAGE of the stem - k-NN,
lin1, bn1, ELU, the max over the neighbours - as one autograd function on HIP kernels, forward and backward (peekvit_amd.pct_train, DESIGN.md
section 20): no [B, N, N] distance matrix, and nothing that scales with k is kept for the backward.  lin2 / bn2, the encoder, the pool and
the head stay stock ops under autograd.  PEEKVIT_AMD_TRAIN=torch (or PEEKVIT_AMD_BACKEND=torch) turns it off; every no_grad forward of the
composite is untouched.

`set_fused_attention(True)` (both models, off by default) additionally moves the attention core of every block under autograd onto the streaming
attention kernels (pct_train.StreamAttention): 16-bit operands, row statistics instead of [B, H, S, S] matrices.

`set_fused_blocks(True)` (both models, off by default) moves every eligible block WHOLE under autograd onto HIP kernels - LayerNorms, linear
layers, GELU, attention core, residual adds, forward and backward (pct_train.PCTBlockFn).

`RankPointCloudTransformer` has the reference's surface (`enable_ranking`, `set_budget`); by default every forward of it is the composite: see
DESIGN.md section 18 for why a 16-bit-operand forward keeps other tokens than the reference on almost every cloud.  Its `set_fused_ranking(True)`
(off by default) moves every SORTING block in train mode whole under autograd onto HIP kernels, on the rows it leaves unmasked plus one row that
stands for all masked ones (pct_train.RankedPCTBlockFn); the ranking there is on the block's fp32 input, as in the composite.
Its `set_fused_inference(True)` (off by default) runs GPU tensors in eval mode under torch.no_grad() in peekvit_amd.engine.rank_pct_forward
(DESIGN.md section 25): PointCloudTransformer's HIP forward whose sorting blocks rank their rows with a sort kernel and read the kept rows through
the ranking in LayerNorm 1, so the cost follows the budget.  The rows that forward keeps are ITS OWN - the top rows of its own fp32 norms, which
carry the 16-bit layers' noise - not the composite's; its logits are the composite's when the composite keeps the same rows, and mode "auto"
checks exactly that: its self-check probe is the composite REPLAYING the kept rows of the forward under check (`_replaying`).
"""
from __future__ import annotations

import contextlib
import math
from typing import List, Optional, Union

import torch
from torch import nn
import torch.nn.functional as F

from .. import engine, pct_train
from .blocks import MLP, SelfAttention

# elements of the largest temporary the composite's k-NN / pair features hold at once (the batch is processed in chunks of images)
_CHUNK_ELEMS = 1 << 25


def knn_indices(x: torch.Tensor, k: int) -> torch.Tensor:
    """The k nearest points of every point of each cloud: x [B, N, 3] -> int64 [B, N, k] in ascending (distance, index) order.  Squared
    distances are (dx*dx + dy*dy) + dz*dz, every operation rounded in x's precision; the point itself is a candidate; exact ties go to the
    lowest index (a non-negative float's bit pattern and the index form one integer key, so no sort has to be stable).  Chunked over the
    batch: never more than _CHUNK_ELEMS elements of [B, N, N] at once."""
    B, N, _ = x.shape
    if not 1 <= k <= N:
        raise ValueError(f"k = {k} neighbours of a cloud of {N} points")
    xd = x.detach()
    out = torch.empty((B, N, k), dtype=torch.int64, device=x.device)
    step = max(1, _CHUNK_ELEMS // (N * N))
    ar = torch.arange(N, dtype=torch.int64, device=x.device)
    ibits = {torch.float32: torch.int32, torch.float64: torch.int64}.get(xd.dtype)
    for b0 in range(0, B, step):
        c = xd[b0:b0 + step]
        dx = c[:, :, None, 0] - c[:, None, :, 0]
        dy = c[:, :, None, 1] - c[:, None, :, 1]
        dz = c[:, :, None, 2] - c[:, None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        if ibits is torch.int32:
            key = d.view(torch.int32).to(torch.int64) * N + ar
            out[b0:b0 + step] = torch.topk(key, k, dim=-1, largest=False, sorted=True).indices
        else:                                               # (fp64 restatements, 16-bit models: a stable sort gives the same order)
            out[b0:b0 + step] = torch.sort(d, dim=-1, stable=True).indices[..., :k]
    return out


class PCTBlock(nn.Module):
    """Transformer block whose residuals are its LayerNorm outputs (reference models/pct.py:20-57)."""

    def __init__(self, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float, attention_dropout: float):
        super().__init__()
        self.num_heads = num_heads
        self.hidden_dim = hidden_dim
        self.mlp_dim = mlp_dim
        self.ln_1 = nn.LayerNorm(hidden_dim)
        self.self_attention = SelfAttention(hidden_dim, num_heads, attention_dropout)
        self.dropout = nn.Dropout(dropout)
        self.ln_2 = nn.LayerNorm(hidden_dim)
        self.mlp = MLP(hidden_dim=hidden_dim, mlp_dim=mlp_dim)
        self.fused_attention = False       # _PCTBase.set_fused_attention: the attention core under autograd on the streaming HIP kernels
        self.fused_block = False           # _PCTBase.set_fused_blocks: the whole block under autograd on HIP kernels (pct_train.PCTBlockFn)

    def _attention(self, x: torch.Tensor) -> torch.Tensor:
        if pct_train.attention_eligible(self, x):
            return pct_train.attention(self.self_attention.self_attention, x)
        return self.self_attention(x)

    def forward(self, input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        if pct_train.block_eligible(self, input):
            return pct_train.block(self, input)
        x = self.ln_1(input)
        x = self._attention(x) + x
        x = self.mlp(self.ln_2(x)) + x
        return x


class RankingPCTBlock(PCTBlock):
    """PCTBlock that, with `sort` on, orders rows 1.. by descending L2 norm (row 0 stays), then at eval keeps the first ceil(S * budget) rows of
    the WHOLE sequence and in training zeroes all but the first ceil((S - 1) * budget) of rows 1.. - before the block, after ln_1 and after ln_2
    (reference models/rankpct.py:19-146).  The reference's argsort is unstable on ties; here ties rank lowest index first."""

    def __init__(self, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float, attention_dropout: float):
        super().__init__(num_heads, hidden_dim, mlp_dim, dropout, attention_dropout)
        self.sort = False
        self.current_budget = 1.0
        self.last_keep = None          # int64 [B, kept]: the input rows the last eval forward with `sort` on kept, in the order it kept them
        self.fused_ranking = False     # RankPointCloudTransformer.set_fused_ranking: a sorting block in train mode whole on HIP kernels, live rows only
        self.last_train_keep = None    # int64 [B, 1 + keep]: row 0, then the input rows the last such forward left unmasked, in rank order
        self.last_norms = None         # fp32 [B, S - 1]: the norms the last HIP eval forward ranked (engine.rank_pct_forward; introspection, tests)
        self._replay_keep = None       # int64 [B, kept] (RankPointCloudTransformer._replaying): the rows an eval forward keeps INSTEAD of ranking its own

    @staticmethod
    def sort_order(input: torch.Tensor) -> torch.Tensor:
        """Row order after sorting: int64 [B, S], row 0 first, then rows 1.. by descending norm."""
        order = torch.argsort(torch.norm(input[:, 1:, :], dim=-1), dim=-1, descending=True, stable=True) + 1
        return torch.cat([torch.zeros_like(order[:, :1]), order], dim=1)

    @staticmethod
    def sort_tokens(input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        order = RankingPCTBlock.sort_order(input)
        return torch.gather(input, 1, order.unsqueeze(-1).expand(-1, -1, input.shape[-1]))

    @staticmethod
    def replayed_order(keep: torch.Tensor, S: int) -> torch.Tensor:
        """A row order int64 [B, S] that starts with the recorded rows `keep` [B, kept]; the remaining rows follow in ascending order."""
        kept = torch.zeros((keep.shape[0], S), dtype=torch.int8, device=keep.device).scatter_(1, keep, 1)
        rest = torch.argsort(kept, dim=1, stable=True)[:, :S - keep.shape[1]]
        return torch.cat([keep, rest], dim=1)

    def mask_tokens(self, input: torch.Tensor):
        if not self.training or not self.sort:
            return input
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        class_token, rest = input[:, 0:1, :], input[:, 1:, :]
        keep = math.ceil(rest.shape[1] * self.current_budget)
        mask = torch.zeros_like(rest)
        mask[:, :keep, :] = 1
        return torch.cat([class_token, rest * mask], dim=1)

    def drop_tokens(self, input: torch.Tensor):
        if self.training or not self.sort:
            return input
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        return input[:, :math.ceil(input.shape[1] * self.current_budget), :]

    def forward(self, input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        if pct_train.ranked_block_eligible(self, input):       # (`sort` and `fused_ranking` on, train mode: ranking, masking and the block on HIP kernels)
            return pct_train.ranked_block(self, input)
        if self.sort:
            order = self.sort_order(input) if self._replay_keep is None or self.training else self.replayed_order(self._replay_keep, input.shape[1])
            input = torch.gather(input, 1, order.unsqueeze(-1).expand(-1, -1, input.shape[-1]))
            if not self.training:
                self.last_keep = order[:, :math.ceil(input.shape[1] * self.current_budget)]
        if pct_train.block_eligible(self, input):       # (never with `sort` on: nothing above or below has touched the rows)
            return pct_train.block(self, input)
        input = self.mask_tokens(input)
        input = self.drop_tokens(input)
        x = self.ln_1(input)
        x = self.mask_tokens(x)
        x = self._attention(x) + x
        x = self.mlp(self.mask_tokens(self.ln_2(x))) + x
        return x

    def set_budget(self, budget: float):
        self.current_budget = budget


class ARPE(nn.Module):
    """Absolute-relative position encoding, the stem (reference models/pct.py:60-90): parameter holder; `forward` is the stock-op composite,
    except that under autograd on the GPU its pair stage (everything up to the max over the neighbours) runs in peekvit_amd.pct_train."""

    def __init__(self, in_channels=3, out_channels=32, npoints=1024):
        super().__init__()
        N0 = 512
        k0 = 32
        self.k = int(k0 * npoints / N0)
        self.lin1 = nn.Linear(2 * in_channels, 2 * in_channels)
        self.lin2 = nn.Linear(2 * in_channels, out_channels)
        self.bn1 = nn.BatchNorm1d(2 * in_channels)
        self.bn2 = nn.BatchNorm1d(out_channels)

    def _pairs(self, x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """[x, x - neighbour] for every (point, neighbour) pair: [B, N, 3], [B, N, k] -> [B * N, k, 6]."""
        B, N, C = x.shape
        knn = torch.gather(x.unsqueeze(1).expand(-1, N, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, C))       # B, N, K, C
        diffs = x.unsqueeze(2) - knn
        feat = torch.cat([x.unsqueeze(2).expand(-1, -1, self.k, -1), diffs], dim=-1)
        return feat.reshape(B * N, self.k, 2 * C)

    def forward(self, x, return_idx: bool = False):
        B, N, C = x.shape
        if not return_idx and pct_train.eligible(self, x):
            # under autograd on the GPU: the pair stage is one autograd function on HIP kernels (batch or frozen statistics by bn1's mode)
            y = pct_train.pair_stage(self, x)
        elif self.training:
            # batch statistics over every pair of the batch: one piece
            idx = knn_indices(x, self.k)
            y = F.elu(self.bn1(self.lin1(self._pairs(x, idx)).transpose(1, 2)).transpose(1, 2))
            y = y.max(dim=1).values
        else:
            step = max(1, _CHUNK_ELEMS // (N * max(N, 8 * 2 * C * self.k)))
            ys, idxs = [], []
            for b0 in range(0, B, step):
                c = x[b0:b0 + step]
                idx = knn_indices(c, self.k)
                y = F.elu(self.bn1(self.lin1(self._pairs(c, idx)).transpose(1, 2)).transpose(1, 2))
                ys.append(y.max(dim=1).values)
                idxs.append(idx)
            y, idx = torch.cat(ys, dim=0), torch.cat(idxs, dim=0)
        y = F.elu(self.bn2(self.lin2(y.view(B, N, 2 * C)).transpose(1, 2)).transpose(1, 2))
        return (y, idx) if return_idx else y


class PCTEncoder(nn.Module):
    """dropout, then the blocks (reference models/pct.py:93-125): no positional embedding, no final LayerNorm."""

    _block = PCTBlock

    def __init__(self, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float, attention_dropout: float):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.ModuleList([self._block(num_heads=num_heads, hidden_dim=hidden_dim, mlp_dim=mlp_dim, dropout=dropout,
                                                 attention_dropout=attention_dropout) for _ in range(num_layers)])

    def forward(self, input: torch.Tensor):
        torch._assert(input.dim() == 3, f"Expected (batch_size, seq_length, hidden_dim) got {input.shape}")
        input = self.dropout(input)
        for layer in self.layers:
            input = layer(input)
        return input


class RankPCTEncoder(PCTEncoder):
    """The encoder of RankPointCloudTransformer (reference models/rankpct.py:184-216; the reference names it PCTEncoder too)."""

    _block = RankingPCTBlock


class Classf_head(nn.Module):
    """lin2(dropout(gelu(bn1(lin1(x))))) (reference models/pct.py:128-143)."""

    def __init__(self, in_channels, n_classes) -> None:
        super().__init__()
        self.in_channels = in_channels
        self.n_classes = n_classes
        self.lin1 = nn.Linear(in_channels, in_channels // 2)
        self.lin2 = nn.Linear(in_channels // 2, n_classes)
        self.bn1 = nn.BatchNorm1d(in_channels // 2)
        self.dp = nn.Dropout(0.5)

    def forward(self, x):
        x = F.gelu(self.bn1(self.lin1(x)))
        x = self.lin2(self.dp(x))
        return x


class _PCTBase(nn.Module):
    _encoder = PCTEncoder

    def __init__(self, num_points: int, num_layers: int, num_heads: int, hidden_dim: int, mlp_dim: int, dropout: float = 0.0,
                 attention_dropout: float = 0.0, num_classes: int = 40, representation_size: Optional[int] = None, num_registers: int = 0,
                 num_class_tokens: int = 1, torch_pretrained_weights: Optional[str] = None):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.mlp_dim = mlp_dim
        self.attention_dropout = attention_dropout
        self.dropout = dropout
        self.num_classes = num_classes
        self.representation_size = representation_size
        self.num_heads = num_heads
        self.num_registers = num_registers
        self.num_class_tokens = num_class_tokens
        self.embedder = ARPE(in_channels=3, out_channels=hidden_dim, npoints=num_points)
        self.class_tokens = nn.Parameter(torch.zeros(1, num_class_tokens, hidden_dim))       # (the forward never uses it, as in the reference)
        if num_registers > 0:
            self.registers = nn.Parameter(torch.zeros(1, num_registers, hidden_dim))
        self.encoder = self._encoder(num_layers=num_layers, num_heads=num_heads, hidden_dim=hidden_dim, mlp_dim=mlp_dim, dropout=dropout,
                                     attention_dropout=attention_dropout)
        self.head = Classf_head(hidden_dim, num_classes)
        if torch_pretrained_weights is not None:
            raise ValueError("torch_pretrained_weights: torchvision has no point-cloud weights, and the reference's adapter is written for "
                             "ViT state dicts")

    def set_fused_attention(self, on: bool = True):
        """Opt in: under autograd on the GPU every block runs its attention core - softmax(q k^T) v - in peekvit_amd.pct_train.StreamAttention, the
        streaming HIP forward and backward with 16-bit operands: nothing of size S^2 is kept for the backward.  Off by default, because it is not the
        stock fp32 ops' arithmetic.  No parameter, buffer or state-dict key; every no_grad forward is unchanged."""
        for blk in self.encoder.layers:
            blk.fused_attention = bool(on)

    def set_fused_blocks(self, on: bool = True):
        """Opt in: under autograd on the GPU every eligible block (pct_train.block_eligible) runs WHOLE - both LayerNorms, the four linear layers,
        GELU, the attention core and both residual adds, forward and backward - in peekvit_amd.pct_train.PCTBlockFn on HIP kernels with 16-bit
        operands and an fp32 residual stream.  Off by default for the reason set_fused_attention is; a block that sorts its
        rows (RankingPCTBlock with `sort` on) keeps the path it has without this switch.  No parameter, buffer or state-dict key; every no_grad
        forward is unchanged."""
        for blk in self.encoder.layers:
            blk.fused_block = bool(on)

    def _process_input(self, x: torch.Tensor) -> torch.Tensor:
        torch._assert(x.dim() == 3, f"Expected (batch_size, num_points, channels) got {x.shape}")
        return self.embedder(x)

    def _composite_forward(self, x: torch.Tensor) -> torch.Tensor:
        """models/pct.py:211-237 on stock ops."""
        x = self._process_input(x)
        b = x.shape[0]
        if self.num_registers > 0:
            x = torch.cat([self.registers.expand(b, -1, -1), x], dim=1)
        x = self.encoder(x)
        x = torch.mean(x, dim=1)
        return self.head(x)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._composite_forward(x)


class PointCloudTransformer(_PCTBase):
    """Point-cloud classifier (reference models/pct.py:146-237)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        torch._assert(x.dim() == 3, f"Expected (batch_size, num_points, channels) got {x.shape}")
        # train mode takes the composite (batch-statistics BatchNorm, the head's dropout 0.5); its stem may run in pct_train
        if not self.training and engine.backend_for(x, self, 0.0) == "hip":
            return engine.run_guarded(self, x, lambda: self._hip_forward(x), probe=self._hip_forward)
        return self._composite_forward(x)

    def _hip_forward(self, x: torch.Tensor) -> torch.Tensor:
        if engine._mode() == "bf16x3" or not engine.pct_supported(self, x):
            # no split-precision form: the guard's fallback (and its self-check reference) is the composite, on the GPU
            return self._composite_forward(x)
        return engine.pct_forward(self, x)


class RankPointCloudTransformer(_PCTBase):
    """Token-ranking point-cloud classifier (reference models/rankpct.py:237-352): the interface and the stock-op composite; opt-in HIP paths for
    training (`set_fused_ranking`) and for eval forwards (`set_fused_inference`, whose kept rows are its own - see the module docstring)."""

    _encoder = RankPCTEncoder
    _fused_inference = False       # set_fused_inference: eval forwards of GPU tensors under no_grad in engine.rank_pct_forward
    _pv_no_defer = True            # (engine.deferred_flags: this forward's result is more than its logits - the blocks' last_keep - so it is not deferred)

    def enable_ranking(self, sort_tokens: Union[bool, List[bool]] = False):
        """Switch the sorting of every block (a bool) or of each block (a list) on or off."""
        if isinstance(sort_tokens, bool):
            sort_tokens = [sort_tokens] * len(self.encoder.layers)
        for blk, sort in zip(self.encoder.layers, sort_tokens):
            blk.sort = sort

    def set_fused_ranking(self, on: bool = True):
        """Opt in: under autograd on the GPU, in train mode, every SORTING block (`enable_ranking`) that pct_train.ranked_block_eligible accepts runs whole
        in peekvit_amd.pct_train.RankedPCTBlockFn - the ranking, the masking and the block's forward and backward on HIP kernels, on the 1 + keep live rows
        plus one row that stands for all masked ones: the cost follows the budget.  Off by default for the reason set_fused_blocks
        is; independent of set_fused_attention / set_fused_blocks (a block that does not sort keeps the path those give it); eval mode is untouched.  No
        parameter, buffer or state-dict key; every no_grad forward is unchanged."""
        for blk in self.encoder.layers:
            blk.fused_ranking = bool(on)

    def set_budget(self, budget: float):
        self.current_budget = budget
        for blk in self.encoder.layers:
            if hasattr(blk, "set_budget"):
                blk.set_budget(budget)

    def set_fused_inference(self, on: bool = True):
        """Opt in: GPU tensors in eval mode under torch.no_grad() run peekvit_amd.engine.rank_pct_forward in PointCloudTransformer's
        precision modes - the stem in one launch, every block on the GEMM and attention kernels, a sorting block on the rows it keeps: its ranking is a sort
        kernel on the fp32 norms of its input, and LayerNorm 1 reads the kept rows through it.  Off by default, because the rows this forward keeps are ITS
        OWN: the norms it ranks carry the 16-bit layers' noise (~5e-4), the keep boundaries of a cloud are 1e-5 .. 2e-4 wide, so it keeps other rows than the
        fp32 composite on almost every cloud.  What it promises instead: the kept rows are exactly the top rows of its own norms
        (`last_keep`, `last_norms` of every sorting block), and the logits are the composite's when the composite keeps those rows - which is what mode "auto"
        measures.  Under `engine.rank_gaps` it leaves each cloud's narrowest keep boundary (engine.rank_pct_note_gaps counts the near-ties).  Everything else -
        CPU tensors, autograd, train mode, mode "bf16x3", a guard trip, shapes engine.rank_pct_supported refuses - is the composite, bit for bit.  No
        parameter, buffer or state-dict key."""
        self._fused_inference = bool(on)

    def _sorting_blocks(self):
        return [blk for blk in self.encoder.layers if blk.sort]

    @contextlib.contextmanager
    def _replaying(self, keeps):
        """Inside, an eval forward of the composite keeps in every sorting block the recorded rows `keeps[i]` (int64 [B, kept], one per sorting block, as
        `last_keep` records them) instead of ranking its own: the arithmetic of another forward's decisions."""
        blocks = self._sorting_blocks()
        assert len(keeps) == len(blocks)
        for blk, kp in zip(blocks, keeps):
            blk._replay_keep = kp
        try:
            yield
        finally:
            for blk in blocks:
                blk._replay_keep = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fused_inference and not self.training and x.dim() == 3 and not torch.is_grad_enabled() and engine.backend_for(x, self, 0.0) == "hip":
            blocks = self._sorting_blocks()
            state = (lambda: [blk.last_keep for blk in blocks]) if blocks else None
            key = repr(([blk.sort for blk in self.encoder.layers], [blk.current_budget for blk in self.encoder.layers]))
            return engine.run_guarded(self, x, lambda: self._hip_forward(x), probe=self._replay_probe, probe_key=key, probe_state=state)
        return self._composite_forward(x)

    def _hip_forward(self, x: torch.Tensor) -> torch.Tensor:
        if engine._mode() == "bf16x3" or not engine.rank_pct_supported(self, x):
            # no split-precision form: the guard's fallback is the composite, on the GPU, with its own ranking
            return self._composite_forward(x)
        return engine.rank_pct_forward(self, x)

    def _replay_probe(self, x: torch.Tensor) -> torch.Tensor:
        """Mode "auto"'s self-check reference for the images x: the composite on the rows the HIP forward keeps for them.  The guard compares arithmetic at
        equal decisions (the blocks' `last_keep` after this call are the replayed rows, so an image whose full-batch forward kept other rows than its
        forward here counts as a flip); comparing against the composite's OWN ranking would find every image flipped, on every forward."""
        if not engine.rank_pct_supported(self, x):
            return self._composite_forward(x)
        with engine.precision("f16"):
            engine.rank_pct_forward(self, x)
        keeps = [blk.last_keep.clone() for blk in self._sorting_blocks()]
        with self._replaying(keeps):
            return self._composite_forward(x)
