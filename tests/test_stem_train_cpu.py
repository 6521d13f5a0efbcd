"""Stem fine-tuning off the GPU: the switch's bookkeeping, the refusals, the ABI surface, and the fp64 reference of
tests/stem_train_ref.py pinned against plain autograd on maps whose pooling windows mostly tie."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mgnns_amd import _lib, ops, synth, trunk
from tests import stem_train_ref as R
from tests.test_trunk_train_cpu import model_with_trunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def filled_stem(salt):
    """(conv1, bn1) of a trunk, filled with synth.trunk_param_value like synth.fill_trunk_ fills a whole trunk."""
    conv, bn = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64)
    for name, mod in (("conv1", conv), ("bn1", bn)):
        mod.load_state_dict({k: torch.from_numpy(synth.trunk_param_value("%s.%s" % (name, k), v.shape, salt)).to(v.dtype)
                             for k, v in mod.state_dict().items()})
    return conv, bn.eval()


@pytest.mark.parametrize("batchnorm", ["frozen", "batch"])
def test_stem_switch_bookkeeping(batchnorm):
    m = model_with_trunks().train()
    keys = set(m.state_dict())
    assert m.trunk_train_stem is False
    assert m.unfreeze_trunks(4, batchnorm=batchnorm, stem=True) is m
    assert m.trunks_trainable is True and m.trunk_train_stages == 4 and m.trunk_train_stem is True
    assert m.trunk_train_batchnorm == batchnorm
    for t in (m.object_features, m.place_features):
        assert not t.training                                             # the container stays in eval
        assert all(p.requires_grad for li in (0, 1, 4, 5, 6, 7) for p in t[li].parameters())
        assert t[0].training is (batchnorm == "batch") and t[1].training is (batchnorm == "batch")
        assert all(mod.training is (batchnorm == "batch") for li in (4, 5, 6, 7) for mod in t[li].modules())
    m.unfreeze_trunks(4, batchnorm=batchnorm)                            # without the stem: conv1 / bn1 are frozen and in eval again
    assert m.trunk_train_stem is False
    for t in (m.object_features, m.place_features):
        assert not any(p.requires_grad for li in (0, 1) for p in t[li].parameters())
        assert not t[0].training and not t[1].training
    m.unfreeze_trunks(4, batchnorm, True)
    assert m.trunk_train_stem is True
    assert m.freeze_trunks() is m and m.trunk_train_stem is False and m.trunks_trainable is False
    assert all(p.requires_grad for t in (m.object_features, m.place_features) for p in t.parameters())
    assert set(m.state_dict()) == keys                                    # the switch adds no state_dict entry


def test_refusals():
    m = model_with_trunks().train()
    f = trunk.ResNetFeatures(trunk.resnet50()).eval()
    for stages in (1, 2, 3):
        with pytest.raises(ValueError, match="stem"):
            m.unfreeze_trunks(stages, stem=True)
        with pytest.raises(ValueError, match="stem"):
            f.forward_train(torch.zeros(1, 3, 64, 64), stages=stages, stem=True)
    assert m.trunk_train_stem is False and m.trunks_trainable is False
    with pytest.raises(ValueError, match="stages"):
        m.unfreeze_trunks(5, stem=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        f.forward_train(torch.zeros(1, 3, 64, 64), stages=4, stem=True)
    img, g = torch.zeros(1, 3, 16, 16), torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.stem_wgrad(img, g)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.maxpool3x3s2_bwd_nhwc(g, torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16), relu_mask=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.stem_conv7(img, torch.zeros(64, ops.STEM_LD, dtype=torch.bfloat16), torch.zeros(64), raw=True)


def test_abi_26_and_the_stem_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mgnns_hip.h")).read()
    assert int(re.search(r"#define MGNNS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 26
    tables = {"mgnns_stem_conv7_raw_fwd": _lib.SIGNATURES, "mgnns_stem_wgrad": _lib.SIGNATURES, "mgnns_maxpool3x3s2_nhwc_bwd": _lib.SIGNATURES,
              "mgnns_stem_wgrad_workspace_bytes": _lib.SIZE_GETTERS}
    for name, table in tables.items():
        assert name in table, name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in the header"
        assert len(decl.group(1).split(",")) == len(table[name]), name
    # the old stem entry keeps its signature
    assert len(re.search(r"\bmgnns_stem_conv7_fwd\s*\(([^;]*)\);", hdr).group(1).split(",")) == len(_lib.SIGNATURES["mgnns_stem_conv7_fwd"]) == 8


def test_first_maximum_rule_is_torchs_on_tied_windows():
    """The reference's pooling backward (explicit strict-> scan) against torch's own max_pool2d autograd where 60 % of the windows tie."""
    rs = np.random.RandomState(5)
    for shape in ((2, 8, 9, 7), (1, 8, 8, 8), (2, 8, 1, 1), (1, 8, 5, 6)):
        x = torch.from_numpy(rs.randint(0, 4, shape).astype(np.float64)).requires_grad_(True)
        y = F.max_pool2d(x, 3, 2, 1)
        gy = torch.from_numpy(rs.standard_normal(tuple(y.shape)))
        (y * gy).sum().backward()
        if shape[2] * shape[3] > 1:
            assert R.tie_fraction(x.detach()) > 0.5
        got = R.maxpool_backward(x.detach(), gy)
        # the same windows route to the same pixels; a pixel that wins several windows adds them in another order (fp64 ulps)
        assert torch.equal(got == 0, x.grad == 0)
        assert float((got - x.grad).abs().max()) <= 4 * 2.0 ** -52 * float(gy.abs().max())


@pytest.mark.parametrize("batch", [False, True], ids=["frozen", "batch"])
def test_r1_equals_fp64_autograd_through_conv_bn_relu_maxpool(batch):
    """Pins the reference: R1 against torch autograd through an fp64 conv2d -> BatchNorm -> ReLU -> max_pool2d(3, 2, 1) whose activations
    take the SAVED values (straight-through, as the bf16 rounding of the weight is) and whose ReLU is the saved mask, down to the fp32
    master parameters; y0 is drawn through a coarse grid so that well over half of the pooling windows tie."""
    conv, bn = filled_stem(4)
    rs = np.random.RandomState(12)
    img = R.rb(torch.from_numpy(rs.standard_normal((2, 3, 21, 26))))
    saved = R.forward_cpu(conv, bn, img, batch, step=1.5)
    y0s = R.nchw64(saved["y0"])
    assert R.tie_fraction(y0s) > 0.5 and (y0s > 0).double().mean() > 0.15
    g_y = torch.from_numpy(rs.standard_normal(tuple(saved["y"].shape)))           # NHWC, as the stage Function hands it over
    r1 = R.stem_backward(conv, bn, saved, g_y, round=False)

    w, gamma, beta = (t.detach().double().requires_grad_(True) for t in (conv.weight, bn.weight, bn.bias))
    ste = lambda value, path: value + (path - path.detach())
    if batch:
        z = ste(R.nchw64(saved["z0"]), F.conv2d(img, ste(R.rb(w.detach()), w), None, stride=2, padding=3))
        o = F.batch_norm(z, None, None, gamma, beta, training=True, eps=bn.eps)
    else:
        scale = gamma / torch.sqrt(bn.running_var.double() + bn.eps)
        wf = ste(R.fold_cpu(conv, bn)[0], w * scale[:, None, None, None])
        o = F.conv2d(img, wf, beta - bn.running_mean.double() * scale, stride=2, padding=3)
    y0 = ste(y0s, o * (y0s > 0))
    y = F.max_pool2d(y0, 3, 2, 1)
    assert torch.equal(y.detach(), R.nchw64(saved["y"]))
    (y * g_y.permute(0, 3, 1, 2)).sum().backward()
    for got, leaf in zip(r1, (w, gamma, beta)):
        assert got.norm() > 0 and got.shape == leaf.shape
        assert R.rel_l2(got, leaf.grad) < 1e-12
    r2 = R.stem_backward(conv, bn, saved, g_y.to(torch.bfloat16), round=True)
    r1b = R.stem_backward(conv, bn, saved, g_y.to(torch.bfloat16), round=False)
    e = max(R.rel_l2(b, a) for a, b in zip(r1b, r2))
    assert 1e-5 < e < 2e-2, e
