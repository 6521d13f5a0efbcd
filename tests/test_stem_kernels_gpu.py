"""The stem's training kernels (csrc/stem_train.hip), each against fp64 over the same stored operands.

stem_wgrad      |dW' - ref| <= 1e-6 sum |g x| and |db' - ref| <= 1e-6 sum |g| per entry (the fp32-chain gate of DESIGN.md 13), a second
                call bit-identical, and a g that is zero but for one pixel landing in exactly the right 147 x 64 entries, exactly
                (a product of two bf16 values is exact in fp32).  Measured on the MI355X: the largest |dW' - ref| / sum |g x| over
                the five shapes is 7.4e-8 (at 7 x 7) and the largest |db' - ref| / sum |g| is 6.4e-9.
maxpool bwd     |got - ref| <= 2^-8 |ref| + 1e-6 sum |g_y of the pixel's windows| against fp64 max_pool2d autograd on the CPU, exactly 0
                where the reference is 0, and the channel sums of g_x and g_y agree within the summed slack without the mask.
raw stem        z0 against the fp64 convolution of the bf16 operands within 2^-8 |ref| + 1e-6 sum |x w|; the folded entry's output is
                bit for bit what it was before any of the new entries ran."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import _lib, ops
from tests import stem_train_ref as R
from tests.test_stem_train_cpu import filled_stem

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (4, 200, 300): OH x OW = 100 x 150 -> 13 x 5 tiles of 8 x 32 per image, 260 tiles; more than the 256 workgroups the kernel
# starts at most, so each workgroup walks two tiles and the split yields 130 partials (the other shapes: one partial per tile).
WGRAD_SHAPES = [(1, 7, 7), (2, 15, 13), (1, 16, 16), (3, 22, 70), (4, 200, 300)]
WGRAD_PARTIALS = {(1, 7, 7): 1, (2, 15, 13): 2, (1, 16, 16): 1, (3, 22, 70): 12, (4, 200, 300): 130}


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def patches(img_bf16):
    """bf16 image [B,3,H,W] -> the convolution's patches as fp64 [B, 147, OH*OW] with k = (kh, kw, c)."""
    B = img_bf16.shape[0]
    cols = F.unfold(img_bf16.cpu().double(), 7, padding=3, stride=2)                 # k = (c, kh, kw)
    return cols.view(B, 3, 7, 7, -1).permute(0, 2, 3, 1, 4).reshape(B, 147, -1)


@functools.lru_cache(maxsize=None)
def wgrad_case(shape):
    """(img fp32, g bf16 NHWC) on the GPU and the fp64 reference (dW, db, sum |g x|, sum |g|), computed once per shape."""
    B, H, W = shape
    OH, OW = out_hw(H, W)
    gen = torch.Generator().manual_seed(B * 1000 + H)
    img = torch.randn(B, 3, H, W, generator=gen)
    g = torch.randn(B, OH, OW, 64, generator=gen).to(torch.bfloat16)
    X = patches(img.to(torch.bfloat16))
    G = g.double().view(B, OH * OW, 64)
    dW = torch.bmm(X, G).sum(0).t()
    mag = torch.bmm(X.abs(), G.abs()).sum(0).t()
    return img.to(DEV), g.to(DEV), dW.contiguous(), G.sum(dim=(0, 1)), mag.contiguous(), G.abs().sum(dim=(0, 1))


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_wgrad_against_fp64_and_bit_identical_repeat(shape):
    img, g, dW, db, mag, gmag = wgrad_case(shape)
    nbytes = _lib.lib().mgnns_stem_wgrad_workspace_bytes(*shape)
    assert nbytes // (64 * 160 * 4) == WGRAD_PARTIALS[shape] and nbytes % (64 * 160 * 4) == 0
    got_w, got_b = ops.stem_wgrad(img, g)
    assert got_w.shape == (64, 147) and got_b.shape == (64,) and got_w.dtype == got_b.dtype == torch.float32
    ew = (got_w.cpu().double() - dW).abs()
    eb = (got_b.cpu().double() - db).abs()
    print("stem_wgrad %s: max |dW' - ref| / sum|g x| = %.2e, max |db' - ref| / sum|g| = %.2e, partials %d"
          % (shape, float((ew / mag).max()), float((eb / gmag).max()), WGRAD_PARTIALS[shape]))
    assert (ew <= 1e-6 * mag).all()
    assert (eb <= 1e-6 * gmag).all()
    again_w, again_b = ops.stem_wgrad(img, g)
    assert torch.equal(again_w, got_w) and torch.equal(again_b, got_b)


@pytest.mark.parametrize("shape", [(3, 22, 70), (2, 15, 13), (1, 7, 7)], ids=lambda s: "x".join(map(str, s)))
def test_stem_wgrad_of_a_single_pixel_lands_in_exactly_the_right_entries(shape):
    """g is zero except in one pixel of the LAST image: dW'[o, (kh, kw, c)] = g[o] * bf16(img[c, 2 oh + kh - 3, 2 ow + kw - 3]) or 0 where
    the tap is padding, exactly; db' = g, exactly.  Pixels: the four corners (padding taps), and one past the first tile boundary in
    both directions where the shape has one."""
    img = wgrad_case(shape)[0]
    B, H, W = shape
    OH, OW = out_hw(H, W)
    xb = img[B - 1].to(torch.bfloat16).double().cpu()
    xp = F.pad(xb, (3, 3, 3, 3))
    vals = torch.randn(64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    pixels = {(0, 0), (0, OW - 1), (OH - 1, 0), (OH - 1, OW - 1), (min(8, OH - 1), min(32, OW - 1))}
    for oh, ow in sorted(pixels):
        g = torch.zeros(B, OH, OW, 64, dtype=torch.bfloat16)
        g[B - 1, oh, ow] = vals
        got_w, got_b = ops.stem_wgrad(img, g.to(DEV))
        tap = xp[:, 2 * oh:2 * oh + 7, 2 * ow:2 * ow + 7].permute(1, 2, 0).reshape(147)          # (kh, kw, c)
        want = vals.double()[:, None] * tap[None, :]
        assert torch.equal(got_w.cpu().double(), want), (oh, ow)
        assert torch.equal(got_b.cpu().double(), vals.double()), (oh, ow)


def test_stem_wgrad_refuses_what_its_neighbours_refuse():
    img, g = wgrad_case((2, 15, 13))[:2]
    with pytest.raises(ValueError, match="does not match"):
        ops.stem_wgrad(img, g[:, :-1].contiguous())
    with pytest.raises(TypeError):
        ops.stem_wgrad(img, g.float())
    with pytest.raises(ValueError, match="H, W >= 7"):
        ops.stem_wgrad(img[:, :, :6].contiguous(), g)
    with pytest.raises(ValueError, match="contiguous"):
        ops.stem_wgrad(img.transpose(2, 3), g)
    dW, db = ops.stem_wgrad(img[:0], g[:0])                                                   # an empty batch: zeros
    assert not dW.any() and not db.any()


# ---- max-pool backward ------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 9, 7, 64), (1, 8, 8, 64), (3, 12, 10, 8), (1, 1, 1, 64), (2, 5, 6, 128)]


def window_sum(gy_abs, H, W):
    """sum of |g_y| over the windows each input pixel belongs to: [B,C,OH,OW] -> [B,C,H,W]."""
    B, C, OH, OW = gy_abs.shape
    rep = gy_abs.reshape(B, C, 1, OH * OW).expand(B, C, 9, OH * OW).reshape(B, C * 9, OH * OW)
    full = F.fold(rep, (2 * OH + 1, 2 * OW + 1), 3, stride=2)
    return full[:, :, 1:1 + H, 1:1 + W]


@functools.lru_cache(maxsize=None)
def pool_case(shape, tied):
    """x, g_y (bf16 NHWC, CPU) and fp64 max_pool2d autograd's gradient [B,C,H,W] with the slack's window sums."""
    B, H, W, C = shape
    rs = np.random.RandomState(H * 31 + W + (7 if tied else 0))
    if tied:
        x = torch.from_numpy(np.array([-1.0, 0.0, 0.5, 1.5])[rs.randint(0, 4, shape)])            # a four-value grid including 0
    else:
        x = torch.from_numpy(rs.standard_normal(shape))
    x = x.to(torch.bfloat16)
    OH, OW = out_hw(H, W)
    gy = torch.from_numpy(rs.standard_normal((B, OH, OW, C))).to(torch.bfloat16)
    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    g64 = gy.double().permute(0, 3, 1, 2).contiguous()
    (F.max_pool2d(x64, 3, 2, 1) * g64).sum().backward()
    if tied and H * W > 1:
        assert R.tie_fraction(x64.detach()) > 0.5
    return x, gy, x64.detach(), g64, x64.grad, window_sum(g64.abs(), H, W)


@pytest.mark.parametrize("relu_mask", [False, True], ids=["plain", "relu_mask"])
@pytest.mark.parametrize("tied", [True, False], ids=["tied", "distinct"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_backward_against_fp64_autograd(shape, tied, relu_mask):
    x, gy, x64, g64, ref, wsum = pool_case(shape, tied)
    if relu_mask:
        ref = ref * (x64 > 0)
    got = ops.maxpool3x3s2_bwd_nhwc(x.to(DEV), gy.to(DEV), relu_mask=relu_mask)
    assert got.shape == x.shape and got.dtype == torch.bfloat16
    got = got.cpu().double().permute(0, 3, 1, 2)
    slack = 2.0 ** -8 * ref.abs() + 1e-6 * wsum
    assert ((got - ref).abs() <= slack).all()
    assert (got[ref == 0] == 0).all()
    if not relu_mask:
        assert ((got.sum(dim=(0, 2, 3)) - g64.sum(dim=(0, 2, 3))).abs() <= slack.sum(dim=(0, 2, 3))).all()
    else:
        assert (got[x64 <= 0] == 0).all()


def test_maxpool_backward_refusals():
    x, gy = (t.to(DEV) for t in pool_case((2, 9, 7, 64), True)[:2])
    with pytest.raises(ValueError, match="pooled shape"):
        ops.maxpool3x3s2_bwd_nhwc(x, gy[:, :-1].contiguous())
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.maxpool3x3s2_bwd_nhwc(x[..., :4].contiguous(), gy[..., :4].contiguous())
    with pytest.raises(TypeError):
        ops.maxpool3x3s2_bwd_nhwc(x.float(), gy)
    assert ops.maxpool3x3s2_bwd_nhwc(x[:0], gy[:0]).shape == (0, 9, 7, 64)


# ---- the stem forward that stops before BatchNorm ---------------------------------------------------------------------------------
def test_raw_stem_forward_and_the_folded_entry_is_untouched():
    conv, bn = filled_stem(3)
    conv, bn = conv.to(DEV), bn.to(DEV)
    folded = ops.conv_fold_bn(conv.weight.detach(), None, (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps),
                              stem=True)
    raw = ops.conv_fold_bn(conv.weight.detach(), None, None, stem=True)
    assert not raw[1].any()
    w64 = conv.weight.detach().to(torch.bfloat16).double().cpu()
    # the raw pack holds bf16(conv1.weight) in the stem's (c, kh, kw) order
    assert torch.equal(raw[0][:, :147].double().cpu(), w64.reshape(64, 147)) and not raw[0][:, 147:].any()
    for shape in ((1, 7, 7), (2, 15, 13), (3, 22, 70)):
        img = wgrad_case(shape)[0]
        before = ops.stem_conv7(img, *folded).clone()
        z0 = ops.stem_conv7(img, *raw, raw=True)
        OH, OW = out_hw(*shape[1:])
        assert z0.shape == (shape[0], OH, OW, 64) and z0.dtype == torch.bfloat16
        x64 = img.to(torch.bfloat16).double().cpu()
        ref = F.conv2d(x64, w64, None, stride=2, padding=3)
        mag = F.conv2d(x64.abs(), w64.abs(), None, stride=2, padding=3)
        got = z0.cpu().double().permute(0, 3, 1, 2)
        assert ((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6 * mag).all()
        assert (got < 0).any()                                                               # no ReLU
        # the new entries in between, then the old entry again: bit for bit what it gave before
        ops.stem_wgrad(img, z0)
        ops.maxpool3x3s2_bwd_nhwc(z0, ops.maxpool3x3s2_nhwc(z0), relu_mask=True)
        assert torch.equal(ops.stem_conv7(img, *folded), before)
        # and the folded entry is still bias + ReLU on the folded pack
        wf = folded[0][:, :147].double().cpu().view(64, 3, 7, 7)
        want = torch.relu(F.conv2d(x64, wf, folded[1].double().cpu(), stride=2, padding=3))
        magf = F.conv2d(x64.abs(), wf.abs(), None, stride=2, padding=3) + folded[1].double().cpu().abs()[None, :, None, None]
        assert ((before.cpu().double().permute(0, 3, 1, 2) - want).abs() <= 2.0 ** -8 * want + 1e-6 * magf).all()
