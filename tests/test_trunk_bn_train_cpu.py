"""Batch-statistics trunk fine-tuning off the GPU: the opt-in's bookkeeping, the refusals, the ABI surface, and the fp64 reference
of tests/trunk_bn_train_ref.py pinned against plain autograd through F.batch_norm(training=True)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import _lib, ops, trunk
from mgnns_amd import train as T
from tests import trunk_bn_train_ref as R
from tests.test_trunk_train_cpu import model_with_trunks, narrow_stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unfreeze_with_batch_statistics_bookkeeping():
    m = model_with_trunks().train()
    assert m.trunk_train_batchnorm == "frozen"
    keys = set(m.state_dict())
    assert m.unfreeze_trunks(batchnorm="batch") is m
    assert m.trunks_trainable is True and m.trunk_train_stages == 1 and m.trunk_train_batchnorm == "batch"
    for t in (m.object_features, m.place_features):
        assert not t.training                                           # the container stays in eval mode
        for li in range(8):
            top = li == 7
            assert all(mod.training is top for mod in t[li].modules()), li
            assert all(p.requires_grad is top for p in t[li].parameters()), li
    m.unfreeze_trunks(stages=4, batchnorm="batch")
    for t in (m.object_features, m.place_features):
        assert not t.training and not t[0].training and not t[1].training
        assert [t[li].training for li in (4, 5, 6, 7)] == [True] * 4
        assert not any(p.requires_grad for li in (0, 1) for p in t[li].parameters())
    m.unfreeze_trunks()                                                 # the default is frozen statistics: everything back in eval
    assert m.trunk_train_batchnorm == "frozen"
    assert all(not mod.training for t in (m.object_features, m.place_features) for mod in t.modules())
    m.unfreeze_trunks(2, "batch")
    assert m.freeze_trunks() is m and m.trunks_trainable is False and m.trunk_train_batchnorm == "frozen"
    assert m.object_features.training and m.place_features.training
    assert set(m.state_dict()) == keys                                  # the switch adds no state_dict entry
    for bad in ("train", None, True):
        with pytest.raises(ValueError, match="batchnorm"):
            m.unfreeze_trunks(batchnorm=bad)
    assert m.trunk_train_batchnorm == "frozen" and m.trunks_trainable is False


def test_refusals_off_the_gpu():
    f = trunk.ResNetFeatures(trunk.resnet50()).eval()
    with pytest.raises(ValueError, match="batchnorm"):
        f.forward_train(torch.zeros(1, 3, 64, 64), batchnorm="running")
    with pytest.raises(RuntimeError, match="GPU only"):
        f.forward_train(torch.zeros(1, 3, 64, 64), batchnorm="batch")
    st = narrow_stage(128, 64, 2, 2, 1)
    with pytest.raises(ValueError, match="batchnorm"):
        T.trunk_stage_forward(st, torch.zeros(1, 128, 4, 4), batchnorm="both")
    with pytest.raises(RuntimeError, match="GPU only"):
        T.trunk_stage_forward(st, torch.zeros(1, 128, 4, 4), batchnorm="batch")
    z = torch.zeros(4, 64, dtype=torch.bfloat16)
    v = torch.zeros(64)
    for call in (lambda: ops.bn_stats_bf16_nhwc(z, 1e-5), lambda: ops.bn_apply_bf16_nhwc(z, v, v, v, v),
                 lambda: ops.bn_backward_bf16_nhwc(z, z, v, v, v)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_abi_stays_26_and_the_batchnorm_entry_points_are_bound_on_both_sides():
    hdr = open(os.path.join(ROOT, "include", "mgnns_hip.h")).read()
    assert int(re.search(r"#define MGNNS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 26
    for table, names in ((_lib.SIGNATURES, ("mgnns_bn_stats_bf16", "mgnns_bn_apply_bf16", "mgnns_bn_backward_bf16")),
                         (_lib.SIZE_GETTERS, ("mgnns_bn_stats_workspace_bytes", "mgnns_bn_backward_workspace_bytes"))):
        for name in names:
            assert name in table, name
            decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr)
            assert decl, name + " is not declared in the header"
            assert len(decl.group(1).split(",")) == len(table[name]), name
    for name in ("bn_stats_bf16_nhwc", "bn_apply_bf16_nhwc", "bn_backward_bf16_nhwc"):
        assert callable(getattr(ops, name))


@pytest.mark.parametrize("case,input_grad", [("two_blocks", True), ("three_blocks", True), ("two_stages", True)])
def test_r1_equals_autograd_through_batch_norm_in_training_mode(case, input_grad):
    """Pins the reference: R1 against torch autograd through an fp64 stage whose BatchNorm layers are F.batch_norm(training=True) over
    the SAVED z, whose ReLUs are the saved masks and whose activations take the saved values (straight-through, as the bf16 roundings
    of the weight and of z are), input gradient included.  Also: rounding the travelling gradients (R2) moves them by parts in a
    thousand."""
    specs, _, _, _ = R.CASES[case]
    stages = [narrow_stage(*s) for s in specs]
    blks = [b for st in stages for b in st]
    stats0 = [{k: v.clone() for k, v in st.state_dict().items() if "running" in k or "num_batches" in k} for st in stages]
    x, dseed = R.case_input(case)
    saved = R.forward_cpu(blks, x.double())
    assert all(torch.equal(v, st.state_dict()[k]) for st, s0 in zip(stages, stats0) for k, v in s0.items())
    out_map = saved["blocks"][-1]["out"]
    if case == "two_stages":
        assert tuple(out_map.shape) == (2, 256, 3, 3)                  # M = 18 values per channel
    dmap = torch.randn(out_map.shape, generator=torch.Generator().manual_seed(dseed)).double()
    raw = [[R.raw_cpu(c) for c, _ in R.block_layers(blk)] for blk in blks]
    g1, gx1 = R.stage_backward(blks, saved, raw, dmap, round=False, input_grad=input_grad)

    leaves = [[tuple(t.detach().double().requires_grad_(True) for t in (c.weight, b.weight, b.bias)) for c, b in R.block_layers(blk)]
              for blk in blks]
    xl = R.nchw64(saved["x"]).requires_grad_(True)
    ste = lambda value, path: value + (path - path.detach())

    def conv_bn(t, bi, j):
        c, b = R.block_layers(blks[bi])[j]
        w, gamma, beta = leaves[bi][j]
        z = F.conv2d(t, ste(raw[bi][j], w), None, stride=c.stride[0], padding=c.padding[0])
        z = ste(R.nchw64(saved["blocks"][bi]["z"][j]), z)
        return F.batch_norm(z, None, None, gamma, beta, training=True, eps=b.eps)
    y = xl
    for bi, blk in enumerate(blks):
        sv = saved["blocks"][bi]
        s1, s2, so = R.nchw64(sv["o1"]), R.nchw64(sv["o2"]), R.nchw64(sv["out"])
        idn = ste(R.nchw64(sv["idn"]), conv_bn(y, bi, 3)) if blk.downsample is not None else y
        o1 = ste(s1, conv_bn(y, bi, 0) * (s1 > 0))
        o2 = ste(s2, conv_bn(o1, bi, 1) * (s2 > 0))
        y = ste(so, (conv_bn(o2, bi, 2) + idn) * (so > 0))
    (y * dmap).sum().backward()
    for bi in range(len(blks)):
        for j, trip in enumerate(leaves[bi]):
            for got, leaf in zip(g1[bi][j], trip):
                assert got.norm() > 0
                assert R.rel_l2(got, leaf.grad) < 1e-12, (bi, j)
    assert gx1.norm() > 0 and R.rel_l2(gx1, xl.grad) < 1e-12
    g2, gx2 = R.stage_backward(blks, saved, raw, dmap, round=True, input_grad=input_grad)
    e = R.rounding_noise(g1, g2, gx1, gx2)
    print("%s: e = %.3e" % (case, e))
    assert 1e-4 < e < 2e-2, e
