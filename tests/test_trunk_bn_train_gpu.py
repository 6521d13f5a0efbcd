"""Batch-statistics fine-tuning of the trunks' trailing stages on the GPU: the stage Function's forward against fp64 over what it
saved, its backward against the fp64 reference computed from the same (tests/trunk_bn_train_ref.py), and the whole model with
unfreeze_trunks(batchnorm='batch').

Backward gates per tensor, relative L2, as tests/test_trunk_train_gpu.py's: with e = |R2 - R1| / |R1| computed here on the CPU (R1:
gradients travel in fp64, R2: rounded to bf16 where the kernels round),  |gpu - R1| <= 2 e |R1|,  |gpu - R2| <= e |R1|,  e < 2e-2."""
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import trunk
from mgnns_amd import train as T
from tests import trunk_bn_train_ref as R
from tests.test_trunk_train_cpu import narrow_stage
from tests.test_trunk_train_gpu import layer4_grads, model_with_trunks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("weight", "bn.weight", "bn.bias")
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def buffers_of(blocks):
    return [[{n: getattr(bn, n).clone() for n in BUFFERS} for _, bn in R.block_layers(b)] for b in blocks]


def run_stage(case, x, freeze=None):
    """One forward + backward of the stage Function in batch mode -> (blocks, saved, dmap, gpu grads as the reference lays them out,
    the parameters freeze(blocks) named, which were frozen)."""
    stages = [narrow_stage(*s).to(DEV) for s in R.CASES[case][0]]
    blocks = [b for st in stages for b in st]
    frozen = tuple(freeze(blocks)) if freeze else ()
    for p in frozen:
        p.requires_grad_(False)
    before = buffers_of(blocks)
    keep = []
    out = T.trunk_stage_forward(stages if len(stages) > 1 else stages[0], x, keep=keep, batchnorm="batch")
    assert out.dtype == torch.float32 and out.requires_grad and (out >= 0).all()
    saved = keep[0]
    assert torch.equal(saved["blocks"][-1]["out"], out.detach())
    check_running_buffers(blocks, saved, before)
    dmap = torch.randn(out.shape, generator=torch.Generator().manual_seed(R.CASES[case][3])).to(DEV)
    out.backward(dmap)
    got = [[tuple(t.grad for t in (c.weight, b.weight, b.bias)) for c, b in R.block_layers(blk)] for blk in blocks]
    return blocks, saved, dmap, got, frozen


def check_running_buffers(blocks, saved, before):
    """running_* = the update formula over the saved z (to the statistics kernel's 1e-5, scaled by the momentum); one more batch."""
    for blk, sv, b0 in zip(blocks, saved["blocks"], before):
        for (_, bn), z, (mean, rstd), old in zip(R.block_layers(blk), sv["z"], sv["stats"], b0):
            z64 = z.cpu().double().reshape(-1, z.shape[-1])
            M, m = z64.shape[0], bn.momentum
            mu, var = z64.mean(0), z64.var(0, unbiased=False)
            assert ((mean.cpu().double() - mu).abs() <= 1e-5 * torch.maximum(mu.abs(), var.sqrt())).all()
            assert ((rstd.cpu().double() * torch.sqrt(var + bn.eps) - 1).abs() <= 1e-5).all()
            want_m = (1 - m) * old["running_mean"].cpu().double() + m * mu
            want_v = (1 - m) * old["running_var"].cpu().double() + m * var * M / (M - 1)
            assert ((bn.running_mean.cpu().double() - want_m).abs() <= 1e-6 * want_m.abs() + m * 1e-5 * torch.maximum(mu.abs(), var.sqrt())).all()
            assert ((bn.running_var.cpu().double() - want_v).abs() <= 1e-6 * want_v + m * 2e-5 * (var + bn.eps) * M / (M - 1)).all()
            assert int(bn.num_batches_tracked) == int(old["num_batches_tracked"]) + 1


def check_forward(blocks, saved):
    """Every saved z against the fp64 convolution of the saved input with the raw bf16 pack (2^-8 |ref| + 1e-6 sum |x w|), every saved
    activation against bn_apply's gate (2^-8 |ref| + 1e-5 (|a z| + |b| + |res|); fp32 map: the second term only; exact zeros below)."""
    x_in = R.nchw64(saved["x"])
    for blk, sv, pk in zip(blocks, saved["blocks"], [trunk.block_packs_raw(b) for b in blocks]):
        layers = R.block_layers(blk)
        o1, o2, out, idn = (R.nchw64(sv[k]) for k in ("o1", "o2", "out", "idn"))
        ins = [x_in, o1, o2, x_in]
        outs = [(o1, None, True), (o2, None, True), (out, idn, True), (idn, None, False)]
        if len(layers) == 3:
            assert sv["idn"] is (saved["x"] if blk is blocks[0] else prev_out)
        for j, (conv, bn) in enumerate(layers):
            w = R.raw_from_pack(pk[j][0], pk[j][3])
            geo = dict(stride=conv.stride[0], padding=conv.padding[0])
            z = R.nchw64(sv["z"][j])
            ref = F.conv2d(ins[j], w, None, **geo)
            mag = F.conv2d(ins[j].abs(), w.abs(), None, **geo)
            assert ((z - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6 * mag).all(), j
            mean, rstd = sv["stats"][j]
            y, res, relu = outs[j]
            a = R.vec(bn.weight) * R.vec(rstd)
            b = R.vec(bn.bias) - R.vec(mean) * a
            pre = a * z + b + (0 if res is None else res)
            slack = 1e-5 * ((a * z).abs() + b.abs() + (0 if res is None else res.abs()))
            want = pre.clamp_min(0) if relu else pre
            rounded = sv["out"].dtype == torch.bfloat16 or y is not out
            assert ((y - want).abs() <= slack + (2.0 ** -8 * want.abs() if rounded else 0)).all(), j
            if relu:
                assert (y[pre < -slack] == 0).all(), j
        x_in, prev_out = out, sv["out"]


def check_against_reference(blocks, saved, dmap, got, gx=None, frozen=()):
    raw = [[R.raw_from_pack(c[0], c[3]) for c in trunk.block_packs_raw(b)] for b in blocks]
    r1, x1 = R.stage_backward(blocks, saved, raw, dmap, round=False, input_grad=gx is not None)
    r2, x2 = R.stage_backward(blocks, saved, raw, dmap, round=True, input_grad=gx is not None)
    frozen = {id(p) for p in frozen}
    rows = []
    for bi, blk in enumerate(blocks):
        for j, (c, b) in enumerate(R.block_layers(blk)):
            for t, p in enumerate((c.weight, b.weight, b.bias)):
                rows.append(("block %d layer %d %s" % (bi, j, NAMES[t]), got[bi][j][t], r1[bi][j][t], r2[bi][j][t], id(p)))
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
    x = R.case_input("two_blocks")[0].to(DEV).requires_grad_(True)
    pick = lambda blocks: (blocks[0].conv2.weight, blocks[0].bn1.bias, blocks[1].bn3.weight, blocks[0].downsample[1].weight)
    blocks, saved, dmap, got, frozen = run_stage("two_blocks", x, pick)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32
    check_forward(blocks, saved)
    check_against_reference(blocks, saved, dmap, got, gx=x.grad, frozen=frozen)


def test_three_block_stage_nhwc_bf16_input_and_bit_identical_repeat():
    x = R.case_input("three_blocks")[0].permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    blocks, saved, dmap, got, _ = run_stage("three_blocks", x)
    assert torch.equal(saved["x"], x)
    check_forward(blocks, saved)
    check_against_reference(blocks, saved, dmap, got)
    # bit-identical from call to call (fresh stages: the same parameters), and an NHWC input that requires a gradient gets one in
    # its own layout and dtype
    xg = x.clone().requires_grad_(True)
    _, saved2, _, again, _ = run_stage("three_blocks", xg)
    assert all(torch.equal(a, b) for ba, bb in zip(got, again) for la, lb in zip(ba, bb) for a, b in zip(la, lb))
    assert all(torch.equal(a, b) for sa, sb in zip(saved["blocks"], saved2["blocks"]) for pa, pb in zip(sa["stats"], sb["stats"])
               for a, b in zip(pa, pb))
    assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == torch.bfloat16


def test_two_chained_stages_with_eighteen_values_per_channel_at_the_top():
    x = R.case_input("two_stages")[0].to(DEV)
    blocks, saved, dmap, got, _ = run_stage("two_stages", x)
    assert len(blocks) == 4 and tuple(saved["blocks"][-1]["out"].shape) == (2, 256, 3, 3)
    check_forward(blocks, saved)
    check_against_reference(blocks, saved, dmap, got)


# ---- the whole model ------------------------------------------------------------------------------------------------------------
def trunk_buffers(model, layers):
    return {"%s.%d.%s" % (n, li, k): v.clone() for n in model.TRUNKS for li in layers for k, v in getattr(model, n)[li].state_dict().items()
            if k.split(".")[-1] in BUFFERS}


def train_grads(model, args, imgs, seed):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    logits = model(*args[:3], imgs[0], imgs[1], *args[5:])
    logits.square().sum().backward()
    return logits.detach(), layer4_grads(model)


def test_whole_model_step_with_batch_statistics():
    model, args, imgs = model_with_trunks()
    with torch.no_grad():
        model.eval()
        before = model(*args[:3], imgs[0], imgs[1], *args[5:]).clone()            # also fills the trunks' folded-weight plans
    model.train().freeze_text_encoders()
    assert model.unfreeze_trunks(batchnorm="batch") is model
    opt = torch.optim.Adam(model.get_config_optim(1e-3, 0.1), lr=1e-3)
    top0, low0 = trunk_buffers(model, (7,)), trunk_buffers(model, (1, 4, 5, 6))
    logits, got = train_grads(model, args, imgs, 99)
    n4 = sum(1 for n in model.TRUNKS for _ in getattr(model, n)[7].parameters())
    assert len(got) == n4 and all(torch.isfinite(v).all() and v.abs().max() > 0 for v in got.values())
    for n in model.TRUNKS:
        assert all(p.grad is None for li in (0, 1, 4, 5, 6) for p in getattr(model, n)[li].parameters())
    # layer4's running statistics moved, by one batch; the stem's and layer1-3's did not
    top1 = trunk_buffers(model, (7,))
    for k, v in top0.items():
        if k.endswith("num_batches_tracked"):
            assert int(top1[k]) == int(v) + 1, k
        else:
            assert not torch.equal(top1[k], v), k
    assert all(torch.equal(v, low0[k]) for k, v in trunk_buffers(model, (1, 4, 5, 6)).items())

    # the composition: the trunks' maps fed as leaves under the same seed, then each trunk's stage alone on its map's gradient
    outs = [getattr(model, n).forward_train(img, 1, batchnorm="batch") for n, img in zip(model.TRUNKS, imgs)]
    maps = [o.detach().clone().requires_grad_(True) for o in outs]
    model.zero_grad(set_to_none=True)
    torch.manual_seed(99)
    logits2 = model(*args[:3], maps[0], maps[1], *args[5:])
    assert torch.equal(logits2, logits)
    logits2.square().sum().backward()
    assert not layer4_grads(model)
    for o, m in zip(outs, maps):
        o.backward(m.grad)
    alone = layer4_grads(model)
    assert alone.keys() == got.keys() and all(torch.equal(alone[k], got[k]) for k in got)

    opt.step()
    with torch.no_grad():
        model.eval()
        after = model(*args[:3], imgs[0], imgs[1], *args[5:]).clone()
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    # the eval forward refolded the moved statistics and parameters: a fresh model loaded from the trained state_dict agrees bit for bit
    fresh, _, _ = model_with_trunks()
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        fresh.eval()
        assert torch.equal(fresh(*args[:3], imgs[0], imgs[1], *args[5:]), after)

    # the default path in the same process: plain unfreeze_trunks() is batchnorm='frozen', bit for bit, and moves no statistic
    fresh.train().freeze_text_encoders().unfreeze_trunks()
    assert fresh.trunk_train_batchnorm == "frozen"
    stats = trunk_buffers(fresh, (1, 4, 5, 6, 7))
    l_a, g_a = train_grads(fresh, args, imgs, 7)
    fresh.unfreeze_trunks(batchnorm="frozen")
    l_b, g_b = train_grads(fresh, args, imgs, 7)
    assert torch.equal(l_a, l_b) and g_a.keys() == g_b.keys() and len(g_a) == n4 and all(torch.equal(g_a[k], g_b[k]) for k in g_a)
    assert all(torch.equal(v, stats[k]) for k, v in trunk_buffers(fresh, (1, 4, 5, 6, 7)).items())
