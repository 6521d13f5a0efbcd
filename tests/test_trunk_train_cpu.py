"""Frozen-statistics trunk fine-tuning off the GPU: the opt-in's bookkeeping, the refusals, the ABI surface, and the fp64 reference
of tests/trunk_train_ref.py pinned against plain autograd."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mgnns_amd import _lib, synth, trunk
from mgnns_amd import train as T
from tests import helpers as H
from tests import trunk_train_ref as R
from tests.model_util import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def narrow_stage(inplanes, planes, blocks, stride, salt):
    """A bottleneck stage like trunk.ResNet._make_layer's, `planes` wide, filled with synth.trunk_param_value."""
    down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    st = nn.Sequential(trunk.Bottleneck(inplanes, planes, stride, down), *[trunk.Bottleneck(planes * 4, planes) for _ in range(1, blocks)])
    sd = st.state_dict()
    st.load_state_dict({k: torch.from_numpy(synth.trunk_param_value("layer4." + k, v.shape, salt)) for k, v in sd.items()})
    return st.eval()


def model_with_trunks():
    """mvsa_single_b8 with a ResNet-50 for either trunk (the state_dict surface of a model built with trunks)."""
    cfg = synth.CONFIGS["mvsa_single_b8"]
    pmi, count = synth.synth_pmi(cfg.V, seed=3)
    adj = H.load_golden("adjacency.npz")
    m = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], np.zeros((7, 300), np.float32))
    m.object_features = trunk.ResNetFeatures(trunk.resnet50())
    m.place_features = trunk.ResNetFeatures(trunk.resnet50(365))
    return m


def test_unfreeze_and_freeze_bookkeeping():
    m = model_with_trunks().train()
    assert m.trunks_trainable is False
    assert m.unfreeze_trunks() is m and m.trunks_trainable is True and m.trunk_train_stages == 1
    for t in (m.object_features, m.place_features):
        assert not t.training and all(not mod.training for mod in t.modules())
        for li in range(8):
            want = li == 7
            assert all(p.requires_grad is want for p in t[li].parameters()), li
    m.unfreeze_trunks(stages=3)
    for t in (m.object_features, m.place_features):
        assert [all(p.requires_grad for p in t[li].parameters()) for li in (4, 5, 6, 7)] == [False, True, True, True]
        assert not any(p.requires_grad for li in (0, 1) for p in t[li].parameters())
    keys = set(m.state_dict())
    assert m.freeze_trunks() is m and m.trunks_trainable is False
    assert all(p.requires_grad for t in (m.object_features, m.place_features) for p in t.parameters())
    assert m.object_features.training and m.place_features.training
    assert set(m.state_dict()) == keys                                # the switch adds no state_dict entry
    for bad in (0, 5):
        with pytest.raises(ValueError, match="stages"):
            m.unfreeze_trunks(stages=bad)


def test_unfreeze_without_trunks_and_refusals_off_the_gpu():
    cfg = synth.CONFIGS["mvsa_single_b8"]
    pmi, count = synth.synth_pmi(cfg.V, seed=3)
    adj = H.load_golden("adjacency.npz")
    m = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], np.zeros((7, 300), np.float32))
    m.train().unfreeze_trunks()                                        # nothing to unfreeze: no parameters, no error
    assert m.trunks_trainable and not list(m.object_features.parameters())
    with pytest.raises(RuntimeError, match="without that CNN trunk"):
        m._train_maps(torch.zeros(2, 3, 64, 64), "object_feature", m.object_features)
    m.freeze_trunks()
    with pytest.raises(NotImplementedError, match="feature maps"):
        m._train_maps(torch.zeros(2, 3, 64, 64), "object_feature", m.object_features)
    f = trunk.ResNetFeatures(trunk.resnet50())
    with pytest.raises(RuntimeError, match="running statistics"):
        f.train().forward_train(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="eval-mode"):
        f.train()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="GPU only"):
        f.eval().forward_train(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="stages"):
        f.forward_train(torch.zeros(1, 3, 64, 64), stages=0)
    with pytest.raises(RuntimeError, match="GPU only"):
        T.trunk_stage_forward(narrow_stage(128, 64, 2, 2, 1), torch.zeros(1, 128, 4, 4))


def test_abi_26_on_both_sides_and_the_new_entry_points_are_bound():
    hdr = open(os.path.join(ROOT, "include", "mgnns_hip.h")).read()
    assert int(re.search(r"#define MGNNS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 26
    for name in ("mgnns_conv_transpose_pack_bf16", "mgnns_conv_dgrad_bf16_nhwc", "mgnns_conv_wgrad_bf16_nhwc", "mgnns_conv_bn_unfold",
                 "mgnns_map_grad_relu_nhwc_bf16"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "mgnns_conv_wgrad_workspace_bytes" in _lib.SIZE_GETTERS


@pytest.mark.parametrize("inplanes,blocks,shape,input_grad", [(128, 2, (2, 128, 6, 5), True), (256, 3, (1, 256, 5, 4), False)])
def test_r1_equals_autograd_through_an_fp64_stage_with_the_same_masks(inplanes, blocks, shape, input_grad):
    """Pins the reference: R1 against torch autograd through an fp64 frozen-BatchNorm stage whose ReLUs are the SAVED masks and whose
    activations take the saved values (straight-through, as the bf16 rounding of w' is), differentiated down to the fp32 master
    parameters -- so the unfold formulas are pinned too.  Also: rounding the travelling gradients (R2) moves them by parts in a thousand."""
    st = narrow_stage(inplanes, 64, blocks, 2, 7)
    blks = list(st)
    rs = np.random.RandomState(11)
    x = R.rb(torch.from_numpy(rs.standard_normal(shape)).abs())
    saved = R.forward_cpu(blks, x)
    out_map = saved["blocks"][-1][2]
    dmap = torch.from_numpy(rs.standard_normal(tuple(out_map.shape)))
    folded = [[R.fold_cpu(c, b)[0] for c, b in R.block_layers(blk)] for blk in blks]
    g1, gx1 = R.stage_backward(blks, saved, folded, dmap, round=False, input_grad=input_grad)

    leaves = [[tuple(t.detach().double().requires_grad_(True) for t in (c.weight, b.weight, b.bias)) for c, b in R.block_layers(blk)]
              for blk in blks]
    xl = R.nchw64(saved["x"]).requires_grad_(True)
    ste = lambda value, path: value + (path - path.detach())

    def conv(t, bi, j):
        c, b = R.block_layers(blks[bi])[j]
        w, gamma, beta = leaves[bi][j]
        scale = gamma / torch.sqrt(b.running_var.double() + b.eps)
        wf = ste(folded[bi][j], w * scale[:, None, None, None])
        return F.conv2d(t, wf, beta - b.running_mean.double() * scale, stride=c.stride[0], padding=c.padding[0])
    y = xl
    for bi, blk in enumerate(blks):
        s1, s2, so = (R.nchw64(t) for t in saved["blocks"][bi])
        idn = conv(y, bi, 3) if blk.downsample is not None else y
        o1 = ste(s1, conv(y, bi, 0) * (s1 > 0))
        o2 = ste(s2, conv(o1, bi, 1) * (s2 > 0))
        y = ste(so, (conv(o2, bi, 2) + idn) * (so > 0))
    (y * dmap).sum().backward()
    for bi in range(len(blks)):
        for j, trip in enumerate(leaves[bi]):
            for got, leaf in zip(g1[bi][j], trip):
                assert got.norm() > 0
                assert R.rel_l2(got, leaf.grad) < 1e-12, (bi, j)
    if input_grad:
        assert gx1.norm() > 0 and R.rel_l2(gx1, xl.grad) < 1e-12
    else:
        assert gx1 is None
    g2, _ = R.stage_backward(blks, saved, folded, dmap, round=True, input_grad=input_grad)
    e = max(R.rel_l2(b_, a_) for bi in range(len(blks)) for ta, tb in zip(g1[bi], g2[bi]) for a_, b_ in zip(ta, tb))
    assert 1e-4 < e < 2e-2, e
