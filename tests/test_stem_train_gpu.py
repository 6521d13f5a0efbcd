"""Fine-tuning the trunks' stem on the GPU: the two stem Functions against the fp64 reference computed from what they
saved (tests/stem_train_ref.py), a trunk alone with and without the stem, and the whole model with unfreeze_trunks(4, stem=True).

Backward gates per tensor, relative L2, as tests/test_trunk_train_gpu.py's: with e = |R2 - R1| / |R1| computed here on the CPU (R1:
gradients travel in fp64, R2: rounded to bf16 where the kernels round),  |gpu - R1| <= 2 e |R1|,  |gpu - R2| <= e |R1|.
Measured on the MI355X: e = 1.4e-3 .. 2.2e-3 per tensor, |gpu - R1| / |R1| = e to four digits, |gpu - R2| / |R1| <= 2.2e-7; the running
buffers within 7.1e-8 of the fp64 update (gate 1e-6)."""
import pytest
import torch

from mgnns_amd import ops, synth, trunk
from mgnns_amd import train as T
from tests import stem_train_ref as R
from tests.test_stem_train_cpu import filled_stem
from tests.test_trunk_train_gpu import model_with_trunks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("conv1.weight", "bn1.weight", "bn1.bias")
CASES = {"3x3x30x26": ((3, 3, 30, 26), 5, 1), "2x3x33x47": ((2, 3, 33, 47), 6, 2)}      # shape, salt, index of the frozen parameter


def run_stem(case, batchnorm, frozen=None):
    """One forward + backward of a stem Function -> (conv, bn, saved, g_y, the three gradients, bn's buffers before)."""
    shape, salt, _ = CASES[case]
    conv, bn = (m.to(DEV) for m in filled_stem(salt))
    params = (conv.weight, bn.weight, bn.bias)
    if frozen is not None:
        params[frozen].requires_grad_(False)
    before = {k: v.clone() for k, v in bn.state_dict().items() if "running" in k or "num_batches" in k}
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(salt)).to(DEV)
    keep = []
    y = T.trunk_stem_forward(conv, bn, img, keep=keep, batchnorm=batchnorm)
    saved = keep[0]
    B, _, H, W = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert y.dtype == torch.bfloat16 and y.requires_grad and tuple(y.shape) == (B, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1, 64)
    assert torch.equal(saved["img"], img.to(torch.bfloat16)) and torch.equal(saved["y"], y.detach())
    assert torch.equal(saved["y"], ops.maxpool3x3s2_nhwc(saved["y0"])) and tuple(saved["y0"].shape) == (B, OH, OW, 64)
    g_y = torch.randn(y.shape, generator=torch.Generator().manual_seed(salt + 10)).to(torch.bfloat16).to(DEV)
    y.backward(g_y)
    assert img.grad is None
    return conv, bn, saved, g_y, tuple(p.grad for p in params), before


def check_against_reference(conv, bn, saved, g_y, got, frozen=None):
    r1 = R.stem_backward(conv, bn, saved, g_y, round=False)
    r2 = R.stem_backward(conv, bn, saved, g_y, round=True)
    for i, (name, g, a, b) in enumerate(zip(NAMES, got, r1, r2)):
        if i == frozen:
            assert g is None, name + ": a frozen parameter got a gradient"
            continue
        assert g is not None and g.shape == a.shape and g.dtype == torch.float32, name
        g = g.detach().cpu().double()
        n1 = float(a.norm())
        assert n1 > 0, name + ": the reference gradient is zero"
        e = float((b - a).norm()) / n1
        d1, d2 = float((g - a).norm()) / n1, float((g - b).norm()) / n1
        print("%-14s e = %.3e   |gpu-R1|/|R1| = %.3e   |gpu-R2|/|R1| = %.3e" % (name, e, d1, d2))
        assert e < 2e-2, name + ": the reference's own rounding noise is implausible"
        assert d1 <= 2 * e and d2 <= e, name


@pytest.mark.parametrize("case", sorted(CASES))
def test_frozen_statistics_stem_function(case):
    frozen = CASES[case][2]
    conv, bn, saved, g_y, got, before = run_stem(case, "frozen", frozen)
    # the forward is the eval stem, bit for bit, and moves no statistic
    fold = trunk.ResNetFeatures._fold(conv, bn, stem=True)
    assert torch.equal(saved["y0"], ops.stem_conv7(saved["img"].float(), *fold)) and "z0" not in saved
    assert all(torch.equal(v, bn.state_dict()[k]) for k, v in before.items())
    check_against_reference(conv, bn, saved, g_y, got, frozen)
    # bit-identical on a second run from the same parameters
    again = run_stem(case, "frozen", frozen)[4]
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("case", sorted(CASES))
def test_batch_statistics_stem_function(case):
    frozen = (CASES[case][2] + 1) % 3
    conv, bn, saved, g_y, got, before = run_stem(case, "batch", frozen)
    z = saved["z0"].cpu().double().reshape(-1, 64)
    M, m = z.shape[0], bn.momentum
    mu, var = z.mean(0), z.var(0, unbiased=False)
    mean, rstd = saved["stats"]
    assert ((mean.cpu().double() - mu).abs() <= 1e-5 * torch.maximum(mu.abs(), var.sqrt())).all()
    assert ((rstd.cpu().double() * torch.sqrt(var + bn.eps) - 1).abs() <= 1e-5).all()
    want_m = (1 - m) * before["running_mean"].cpu().double() + m * mu
    want_v = (1 - m) * before["running_var"].cpu().double() + m * var * M / (M - 1)
    dm, dv = (bn.running_mean.cpu().double() - want_m).abs().max(), (bn.running_var.cpu().double() - want_v).abs().max()
    print("running_mean off by %.2e, running_var off by %.2e" % (float(dm), float(dv)))
    assert dm <= 1e-6 and dv <= 1e-6
    assert int(bn.num_batches_tracked) == int(before["num_batches_tracked"]) + 1
    # y0 = relu(bn_apply(z0)): the gate of tests/test_trunk_bn_train_gpu.py
    a = bn.weight.detach().cpu().double() * rstd.cpu().double()
    b = bn.bias.detach().cpu().double() - mean.cpu().double() * a
    pre = a * z + b
    y0 = saved["y0"].cpu().double().reshape(-1, 64)
    slack = 1e-5 * ((a * z).abs() + b.abs())
    assert ((y0 - pre.clamp_min(0)).abs() <= slack + 2.0 ** -8 * pre.clamp_min(0)).all() and (y0[pre < -slack] == 0).all()
    check_against_reference(conv, bn, saved, g_y, got, frozen)
    again = run_stem(case, "batch", frozen)
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(got, again[4]))
    assert all(torch.equal(x, y) for x, y in zip(saved["stats"], again[2]["stats"]))


# ---- a trunk alone ------------------------------------------------------------------------------------------------------------------
def trunk_and_inputs():
    f = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet50(), 1)).to(DEV).eval()
    img = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    dmap = torch.randn(2, 2048, 2, 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    return f, img, dmap


def grads_of(f):
    out = {k: p.grad.clone() for k, p in f.named_parameters() if p.grad is not None}
    f.zero_grad(set_to_none=True)
    return out


def test_trunk_frozen_statistics_with_and_without_the_stem():
    f, img, dmap = trunk_and_inputs()
    map_a = f.forward_train(img, stages=4)
    map_a.backward(dmap)
    ga = grads_of(f)
    map_b = f.forward_train(img, stages=4, stem=True)                       # without the feature: a TypeError at the keyword
    map_b.backward(dmap)
    gb = grads_of(f)
    assert torch.equal(map_a, map_b) and torch.equal(map_a.detach(), f(img))
    stem_keys = {"0.weight", "1.weight", "1.bias"}
    assert set(gb) == set(ga) | stem_keys and not (set(ga) & stem_keys)
    assert all(torch.equal(ga[k], gb[k]) for k in ga)
    assert all(torch.isfinite(gb[k]).all() and gb[k].abs().max() > 0 for k in stem_keys)
    assert gb["0.weight"].shape == (64, 3, 7, 7)


def test_trunk_batch_statistics_with_the_stem():
    f, img, dmap = trunk_and_inputs()
    for li in (0, 1, 4, 5, 6, 7):
        f[li].train()
    buf0 = {k: v.clone() for k, v in f[1].state_dict().items() if "running" in k or "num_batches" in k}
    out = f.forward_train(img, stages=4, batchnorm="batch", stem=True)
    out.backward(dmap)
    g = grads_of(f)
    assert all(torch.isfinite(g[k]).all() and g[k].abs().max() > 0 for k in ("0.weight", "1.weight", "1.bias"))
    assert len(g) == len(list(f.parameters()))
    buf1 = f[1].state_dict()
    assert not torch.equal(buf1["running_mean"], buf0["running_mean"]) and not torch.equal(buf1["running_var"], buf0["running_var"])
    assert int(buf1["num_batches_tracked"]) == int(buf0["num_batches_tracked"]) + 1
    with torch.no_grad():
        after = f(img)
    fresh = trunk.ResNetFeatures(trunk.resnet50()).to(DEV).eval()
    fresh.load_state_dict(f.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(img), after)


# ---- the whole model ----------------------------------------------------------------------------------------------------------------
def test_whole_model_step_with_the_stem():
    model, args, imgs = model_with_trunks()
    with torch.no_grad():
        model.eval()
        before = model(*args[:3], imgs[0], imgs[1], *args[5:]).clone()
    model.train().freeze_text_encoders()
    assert model.unfreeze_trunks(4, stem=True) is model and model.trunk_train_stem is True
    opt = torch.optim.Adam(model.get_config_optim(1e-3, 0.1), lr=1e-3)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(99)
    logits = model(*args[:3], imgs[0], imgs[1], *args[5:])
    logits.square().sum().backward()
    for n in model.TRUNKS:
        for k, p in getattr(model, n).named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n + "." + k
        assert getattr(model, n)[0].weight.grad.abs().max() > 0
    w0 = [getattr(model, n)[0].weight.detach().clone() for n in model.TRUNKS]
    opt.step()
    assert all(not torch.equal(getattr(model, n)[0].weight.detach(), w) for n, w in zip(model.TRUNKS, w0))
    with torch.no_grad():
        model.eval()
        after = model(*args[:3], imgs[0], imgs[1], *args[5:])
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    model.train().freeze_text_encoders()
    assert model.freeze_trunks() is model and model.trunk_train_stem is False
    with pytest.raises(NotImplementedError, match="feature maps"):
        model(*args[:3], imgs[0], imgs[1], *args[5:])
