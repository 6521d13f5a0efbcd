"""Training mode of the fusion layers without a GPU: the surface (the attention-dropout submodule adds no state_dict key) and
the refusal to compute on CPU tensors."""
import pytest
import torch

from mgnns_amd import fusion
from tests import helpers as H


def test_attn_dropout_submodule_keeps_the_state_dict_surface():
    m = fusion.MyMultiHeadAttention(4, 300, 128, dropout=0.2)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == H.mha_shapes(4)
    a = m.slf_attn
    assert isinstance(a.attn_dropout, torch.nn.Dropout) and a.attn_dropout.p == 0.1      # submodules.py:97-103
    assert a.dropout.p == 0.2 and m.pos_ffn.dropout.p == 0.2
    assert a.attention == 'faithful'                            # the mode string keeps its name


def test_training_forward_is_gpu_only():
    m = fusion.MyMultiHeadAttention(4, 300, 128).train()
    q, bank = torch.zeros(2, 300), torch.zeros(2, 5, 300)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(q, bank, bank)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.pos_ffn(torch.zeros(2, 1, 300))
    with pytest.raises(NotImplementedError, match="fp32"):
        m.slf_attn.precision = 'bf16'
        m(q, bank, bank)
