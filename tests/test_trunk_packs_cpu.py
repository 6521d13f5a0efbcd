"""The trunk's per-layer derived packs off the GPU (trunk.layer_pack): what a lookup folds and transposes, counted on
stubs of ops.conv_fold_bn and ops.conv_transpose_pack over CPU tensors.

Weights are updated as an optimizer updates them, in place under no_grad, which moves the tensor's version; an update through
`.data` moves neither the version nor the address and is invisible to every derived pack of the package."""
import pytest
import torch

from mgnns_amd import ops, trunk


@pytest.fixture
def feats(monkeypatch):
    folds, transposes = [], []

    def fold(weight, conv_bias=None, bn=None, stem=False):
        folds.append((weight.data_ptr(), "raw" if bn is None else "folded"))
        return torch.zeros(weight.shape[0], weight[0].numel(), dtype=torch.bfloat16), torch.zeros(weight.shape[0])

    def transpose(wt, k):
        transposes.append(wt)
        return wt.t().contiguous()
    monkeypatch.setattr(ops, "conv_fold_bn", fold)
    monkeypatch.setattr(ops, "conv_transpose_pack", transpose)
    f = trunk.ResNetFeatures(trunk.ResNet((1, 1, 1, 1))).eval()
    f.folds, f.transposes = folds, transposes
    return f


def layers_of(f):
    return [(f[0], f[1])] + [pair for li in range(4, 8) for blk in f[li] for pair in trunk.block_layers(blk)]


def plan_wts(f):
    stem, blocks = f._prepare()
    return [stem[0]] + [pack[0] for packs in blocks for pack in packs]


def test_a_lookup_folds_each_layer_once_and_only_what_changed(feats):
    f = feats
    layers = layers_of(f)
    assert len(layers) == 1 + 4 * 4
    first = plan_wts(f)
    assert sorted(f.folds) == sorted((conv.weight.data_ptr(), "folded") for conv, _ in layers) and not f.transposes
    del f.folds[:]
    assert all(a is b for a, b in zip(plan_wts(f), first)) and not f.folds

    conv, bn = f[7][0].conv2, f[7][0].bn2
    at = [c for c, _ in layers].index(conv)
    with torch.no_grad():
        conv.weight.add_(1)
    second = plan_wts(f)
    assert f.folds == [(conv.weight.data_ptr(), "folded")]
    assert [a is b for a, b in zip(second, first)] == [i != at for i in range(len(layers))]

    # a running statistic is a source of the folded pack and none of the raw pack's
    raw = trunk.layer_pack(conv, bn, 'raw')[0]
    del f.folds[:]
    bn.running_var.add_(1)
    third = plan_wts(f)
    assert f.folds == [(conv.weight.data_ptr(), "folded")]
    assert [a is b for a, b in zip(third, second)] == [i != at for i in range(len(layers))]
    assert trunk.layer_pack(conv, bn, 'raw')[0] is raw and len(f.folds) == 1
    assert not f.transposes


def test_block_packs_hand_out_the_eval_plans_tensors_and_transpose_on_demand(feats):
    f = feats
    blocks = f._prepare()[1]
    del f.folds[:]
    blk, plan = f[7][0], blocks[3]
    packs = trunk.block_packs(blk)
    assert len(packs) == len(plan) == 4
    for pack, (wt, bias, k, s, p) in zip(packs, plan):
        assert pack[0] is wt and pack[1] is bias and pack[3:] == (k, s, p)
    assert not f.folds and len(f.transposes) == 4 and all(t is pack[0] for t, pack in zip(f.transposes, packs))
    again = trunk.block_packs(blk)
    assert all(a[2] is b[2] for a, b in zip(again, packs)) and len(f.transposes) == 4
    # the raw kind folds and transposes on its own, once
    raw = trunk.block_packs_raw(blk)
    assert f.folds == [(conv.weight.data_ptr(), "raw") for conv, _ in trunk.block_layers(blk)] and len(f.transposes) == 8
    assert all(a[0] is b[0] and a[2] is b[2] for a, b in zip(trunk.block_packs_raw(blk), raw)) and len(f.transposes) == 8
    assert all(r[0] is not p[0] for r, p in zip(raw, packs))


def test_refusals_keep_their_text(feats):
    f = feats
    biased = torch.nn.Conv2d(64, 64, 1, bias=True)
    f[4][0].conv1 = biased
    assert f._prepare()[1][0][0][0].shape == (64, 64)                  # eval accepts a convolution with a bias
    with pytest.raises(NotImplementedError, match="convolutions with a bias are not supported"):
        trunk.block_packs(f[4][0])
    with pytest.raises(NotImplementedError, match="convolutions with a bias are not supported"):
        trunk.block_packs_raw(f[4][0])
    f[5][0].downsample[0] = torch.nn.Conv2d(256, 512, 5, stride=2, padding=2, bias=False)
    with pytest.raises(ValueError, match=r"5\.0\.downsample: only square 1x1 / 3x3, dilation 1, groups 1 convolutions are supported"):
        f._prepare()
    with pytest.raises(ValueError, match="bottleneck: only square 1x1 / 3x3"):
        trunk.block_packs(f[5][0])
