"""The dense training path past 208 token rows, without a GPU: what train_engine.supported admits, which attention pair
train_engine.attention_pair picks for (S, dh), the streaming pair's bias-partial rows, and the callers whose OTHER kernels stay bounded by rows
(A-ViT's fused and packed passes, ResidualViT's compact training and token compaction) refusing 227 rows as before."""
import pytest
import torch

from peekvit_amd import train_engine as te


def _was_supported(D, H, S):
    """train_engine.supported as it stood before the streaming pair: the resident attention backward's rows."""
    dh = D // H
    return D % H == 0 and dh in (32, 48, 64) and S <= (416 if dh == 32 else 208) and D <= 1024 and D % 8 == 0


@pytest.mark.parametrize("D,H,S", [(128, 2, 209), (256, 4, 402), (256, 4, 786), (64, 2, 417), (768, 12, 577)])
def test_supported_admits_long_sequences(D, H, S):
    assert not _was_supported(D, H, S)
    assert te.supported(D, H, S)


def test_supported_still_refuses_what_no_kernel_covers():
    assert not te.supported(160, 2, 197)                 # dh 80
    assert not te.supported(1032, 24, 197)               # D = 1032
    assert not te.supported(1088, 17, 197)               # dh 64, D > 1024
    assert not te.supported(128, 2, 0)
    assert not te.supported(128, 2, 4097)
    assert te.supported(128, 2, 1) and te.supported(128, 2, 4096) and te.supported(1024, 16, 4096)
    assert not te.supported(132, 3, 197)                 # dh 44
    assert not te.supported(130, 2, 197)                 # D % H == 0, dh 65


def test_the_resident_pair_wherever_the_path_was_supported_before():
    for dh, H in ((48, 2), (64, 2), (32, 2)):
        D = dh * H
        last = 416 if dh == 32 else 208
        for S in range(1, last + 1):
            assert _was_supported(D, H, S)
            pair = te.attention_pair(3, S, dh)
            assert type(pair) is te._ResidentAttn and (pair.B, pair.S) == (3, S), (S, dh)
            assert pair.bias_rows() == ("bw_dbp", 3)
        assert type(te.attention_pair(3, last + 1, dh)) is te._StreamAttn


@pytest.mark.parametrize("S,dh", [(209, 64), (416, 64), (417, 64), (417, 32), (209, 48), (4096, 64)])
def test_the_streaming_pair_beyond(S, dh):
    pair = te.attention_pair(2, S, dh)
    assert type(pair) is te._StreamAttn and (pair.B, pair.S) == (2, S)


@pytest.mark.parametrize("S", [209, 256, 257])
def test_bias_rows_of_the_streaming_pair(S):
    for B in (1, 5):
        name, rows = te._StreamAttn(B, S).bias_rows()
        assert rows == B * -(-S // 64)
        # scratch of its own: the other pairs' buffers are never resized under them
        assert name not in {te._ResidentAttn(B, 8).bias_rows()[0], te._RaggedAttn(B, 8).bias_rows()[0], te._StreamDropAttn(B, 8, 0, 0, 0.1).bias_rows()[0]}


class _Cuda:
    """What the eligibility rules read of the input tensor."""
    is_cuda, requires_grad = True, False

    def numel(self):
        return 1


def test_row_bounded_callers_still_refuse_227_rows():
    from peekvit_amd.models.adavit import AdaptiveVisionTransformer
    from peekvit_amd.models.residualvit import ResidualVisionTransformer
    avit = AdaptiveVisionTransformer(image_size=240, patch_size=16, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=64, num_classes=10)
    assert avit.seq_length == 226 and te.supported(64, 1, 226)
    assert not avit._fused_training_ok() and not avit._packed_training_ok()
    small = AdaptiveVisionTransformer(image_size=224, patch_size=16, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=64, num_classes=10)
    assert small.seq_length == 197 and small._fused_training_ok() and small._packed_training_ok()
    tiny = AdaptiveVisionTransformer(image_size=160, patch_size=8, num_layers=1, num_heads=2, hidden_dim=64, mlp_dim=64, num_classes=10)
    assert tiny.seq_length == 401 and tiny._fused_training_ok() and not tiny._packed_training_ok()          # head dim 32: 416 rows, as before
    extra = dict(gate_type="sigmoid", gate_temp=1, gate_bias=2, add_budget_token="learnable", gate_threshold=0.5)
    big = ResidualVisionTransformer(image_size=240, patch_size=16, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=64, **extra)
    assert big.seq_length + 1 == 227 and te.supported(64, 1, 227)
    assert not big.eval()._compaction_ok(_Cuda())                                                              # token compaction
    with torch.enable_grad():
        assert not big.train()._compaction_ok(_Cuda(), training=True)                                          # compact training
    ok = ResidualVisionTransformer(image_size=224, patch_size=16, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=64, **extra)
    assert ok.eval()._compaction_ok(_Cuda())
