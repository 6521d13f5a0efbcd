"""Frozen-statistics fine-tuning of the trunks' trailing stages on the GPU: the stage Function against the fp64 reference computed
from the activations it saved (tests/trunk_train_ref.py), and the whole model with unfreeze_trunks().

Gates per parameter tensor, relative L2, with e = |R2 - R1| / |R1| computed here on the CPU (R1: gradients travel in fp64, R2: rounded
to bf16 where the kernels round):  |gpu - R1| <= 2 e |R1|  (the kernels round where R2 rounds; the factor 2 covers summation
order) and  |gpu - R2| <= e |R1|  (another summation order can only flip single bf16 roundings by one ulp)."""
import pytest
import torch

from mgnns_amd import harness, synth, trunk
from mgnns_amd import train as T
from tests import test_model_train_gpu as M
from tests import trunk_train_ref as R
from tests.test_trunk_train_cpu import narrow_stage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("weight", "bn.weight", "bn.bias")


def run_stage(stages, x, dmap_seed, frozen=()):
    """One forward + backward of the stage Function -> (blocks, saved, dmap, gpu grads as the reference lays them out, x.grad)."""
    blocks = [b for st in stages for b in st]
    for p in frozen:
        p.requires_grad_(False)
    stats = {k: v.clone() for st in stages for k, v in st.state_dict().items() if "running" in k or "num_batches" in k}
    keep = []
    out = T.trunk_stage_forward(stages if len(stages) > 1 else stages[0], x, keep=keep)
    assert out.dtype == torch.float32 and out.requires_grad and (out >= 0).all()
    dmap = torch.randn(out.shape, generator=torch.Generator().manual_seed(dmap_seed)).to(DEV)
    out.backward(dmap)
    after = {k: v for st in stages for k, v in st.state_dict().items() if k in stats}
    assert all(torch.equal(stats[k], after[k]) for k in stats)          # running statistics: bit-unchanged
    got = [[tuple(t.grad for t in (c.weight, b.weight, b.bias)) for c, b in R.block_layers(blk)] for blk in blocks]
    assert torch.equal(keep[0]["blocks"][-1][2], out.detach())
    return blocks, keep[0], dmap, got


def check_against_reference(blocks, saved, dmap, got, gx=None, frozen=()):
    packs = [trunk.block_packs(b) for b in blocks]
    folded = [[R.folded_from_pack(c[0], c[3]) for c in pk] for pk in packs]
    r1, x1 = R.stage_backward(blocks, saved, folded, dmap, round=False, input_grad=gx is not None)
    r2, x2 = R.stage_backward(blocks, saved, folded, dmap, round=True, input_grad=gx is not None)
    frozen = {id(p) for p in frozen}
    rows = [("block %d layer %d %s" % (bi, j, NAMES[t]), got[bi][j][t], r1[bi][j][t], r2[bi][j][t],
             id((R.block_layers(blocks[bi])[j][0].weight, R.block_layers(blocks[bi])[j][1].weight, R.block_layers(blocks[bi])[j][1].bias)[t]))
            for bi in range(len(blocks)) for j in range(len(r1[bi])) for t in range(3)]
    if gx is not None:
        rows.append(("stage input", gx, x1, x2, None))
    worst = 0.0
    for name, g, a, b, pid in rows:
        if pid in frozen:
            assert g is None, name + ": a frozen parameter got a gradient"
            continue
        assert g is not None, name + ": no gradient"
        g = g.detach().cpu().double()
        if g.dim() == 4 and g.shape != a.shape:                         # an NHWC bf16 input gradient
            g = g.permute(0, 3, 1, 2)
        n1 = float(a.norm())
        assert n1 > 0, name + ": the reference gradient is zero"
        e = float((b - a).norm()) / n1
        d1, d2 = float((g - a).norm()) / n1, float((g - b).norm()) / n1
        print("%-28s e = %.3e   |gpu-R1|/|R1| = %.3e   |gpu-R2|/|R1| = %.3e" % (name, e, d1, d2))
        assert e < 2e-2, name + ": the reference's own rounding noise is implausible"
        assert d1 <= 2 * e and d2 <= e, name
        worst = max(worst, e)
    print("largest e: %.3e" % worst)


def test_two_block_stage_nchw_input_with_input_gradient_and_frozen_parameters():
    st = narrow_stage(128, 64, 2, 2, 3).to(DEV)
    x = torch.randn(3, 128, 12, 10, generator=torch.Generator().manual_seed(1)).abs().to(DEV).requires_grad_(True)
    frozen = (st[0].conv2.weight, st[0].bn1.bias, st[1].bn3.weight)
    blocks, saved, dmap, got = run_stage([st], x, 2, frozen)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    check_against_reference(blocks, saved, dmap, got, gx=x.grad, frozen=frozen)


def test_three_block_stage_nhwc_bf16_input():
    st = narrow_stage(256, 64, 3, 2, 4).to(DEV)
    x = torch.randn(2, 9, 7, 256, generator=torch.Generator().manual_seed(5)).abs().to(torch.bfloat16).to(DEV)
    blocks, saved, dmap, got = run_stage([st], x, 6)
    assert torch.equal(saved["x"], x)
    check_against_reference(blocks, saved, dmap, got)
    # bit-identical from call to call, and an NHWC input that requires a gradient gets one in its own layout and dtype
    for p in st.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    _, _, _, again = run_stage([st], xg, 6)
    assert all(torch.equal(a, b) for ba, bb in zip(got, again) for la, lb in zip(ba, bb) for a, b in zip(la, lb))
    assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == torch.bfloat16


def test_two_chained_stages_the_gradient_crosses_the_stage_boundary():
    a, b = narrow_stage(128, 64, 2, 2, 8).to(DEV), narrow_stage(256, 64, 2, 2, 9).to(DEV)
    x = torch.randn(2, 128, 9, 11, generator=torch.Generator().manual_seed(7)).abs().to(DEV)
    blocks, saved, dmap, got = run_stage([a, b], x, 8)
    assert len(blocks) == 4 and tuple(saved["blocks"][-1][2].shape) == (2, 256, 3, 3)
    check_against_reference(blocks, saved, dmap, got)


# ---- the whole model ------------------------------------------------------------------------------------------------------------
def model_with_trunks(B=2):
    cfg, model, inp = M.make("mvsa_single_b8", B=B)
    model.object_features = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet50(), 1)).to(DEV)
    model.place_features = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet50(365), 2)).to(DEV)
    model.train().freeze_text_encoders()
    args = list(harness.call_args(inp, DEV))
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randn(B, 3, 448, 448, generator=g).to(DEV) for _ in range(2)]
    return model, args, imgs


def layer4_grads(model):
    return {n + "." + k: p.grad.clone() for n in model.TRUNKS for k, p in getattr(model, n)[7].named_parameters() if p.grad is not None}


def test_whole_model_step_with_unfrozen_trunks():
    model, args, imgs = model_with_trunks()
    assert model.unfreeze_trunks() is model
    with torch.no_grad():
        model.eval()
        before = model(*args[:3], imgs[0], imgs[1], *args[5:]).clone()
        model.train().freeze_text_encoders().unfreeze_trunks()
    lr, lrp = 1e-3, 0.1
    opt = torch.optim.Adam(model.get_config_optim(lr, lrp), lr=lr)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(99)
    logits = model(*args[:3], imgs[0], imgs[1], *args[5:])
    logits.square().sum().backward()
    got = layer4_grads(model)
    n4 = sum(1 for n in model.TRUNKS for _ in getattr(model, n)[7].parameters())
    assert len(got) == n4 and all(torch.isfinite(v).all() and v.abs().max() > 0 for v in got.values())
    for n in model.TRUNKS:
        t = getattr(model, n)
        assert all(p.grad is None for li in (0, 1, 4, 5, 6) for p in t[li].parameters())
    others = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None and "_features." not in k}

    # the composition: eval-trunk maps fed as leaves under the same seed, then the trunk's stage alone on the maps' gradients
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        maps = [model.object_features(imgs[0]), model.place_features(imgs[1])]
    maps = [m.requires_grad_(True) for m in maps]
    torch.manual_seed(99)
    logits2 = model(*args[:3], maps[0], maps[1], *args[5:])
    assert torch.equal(logits2, logits)
    logits2.square().sum().backward()
    for k, p in model.named_parameters():
        if "_features." not in k and p.grad is not None:
            assert torch.equal(p.grad, others[k]), k
    assert not layer4_grads(model)
    for n, img, m in zip(model.TRUNKS, imgs, maps):
        out = getattr(model, n).forward_train(img)
        assert torch.equal(out.detach(), m.detach())
        out.backward(m.grad)
    alone = layer4_grads(model)
    assert alone.keys() == got.keys()
    for k in got:
        assert torch.equal(alone[k], got[k]), k

    w0 = {k: p.detach().clone() for n in model.TRUNKS for k, p in getattr(model, n)[7].named_parameters()}
    stats = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    opt.step()
    moved = [not torch.equal(p.detach(), w0[k]) for n in model.TRUNKS for k, p in getattr(model, n)[7].named_parameters()]
    assert all(moved)
    sd = model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in stats.items())
    with torch.no_grad():
        model.eval()
        after = model(*args[:3], imgs[0], imgs[1], *args[5:])
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    model.train().freeze_text_encoders()
    assert model.freeze_trunks() is model
    with pytest.raises(NotImplementedError, match="feature maps"):
        model(*args[:3], imgs[0], imgs[1], *args[5:])


def test_mixed_input_images_for_one_trunk_and_maps_for_the_other():
    model, args, imgs = model_with_trunks()
    model.unfreeze_trunks()
    torch.manual_seed(5)
    logits = model(*args[:3], imgs[0], args[4], *args[5:])
    logits.square().sum().backward()
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in model.object_features[7].parameters())
    assert all(p.grad is None for p in model.place_features.parameters())
    # a model without trunks says so
    cfg, bare, inp = M.make("mvsa_single_b8", B=2)
    bare.unfreeze_trunks()
    with pytest.raises(RuntimeError, match="without that CNN trunk"):
        bare(*args[:3], imgs[0], args[4], *args[5:])
