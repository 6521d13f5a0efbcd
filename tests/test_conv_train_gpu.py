"""The trunk backward's kernels (csrc/conv_train.hip) at the smallest shapes that can still go wrong, same operands on both sides:
the fp64 reference gets the very bf16 values the kernels read.  Gates (derived):
  dgrad       |got - ref| <= 2^-7 |ref| + 1e-6 sum|dY w'|   one bf16 rounding of the exact value + fp32 accumulation slack
  wgrad, db'  |got - ref| <= 1e-6 sum|dY X|                 fp32 chains (0.75-3.5e-7 of the magnitude sum measured up to K = 4096)
  BN unfold   1e-6 of the sum of magnitudes"""
import functools

import numpy as np
import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

from mgnns_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, H, W, Cin, Cout, k, stride): H, W = the convolution's input; pad = k // 2
GEOMETRIES = [
    (2, 5, 7, 64, 128, 1, 1),        # M = 70: less than one tile
    (3, 12, 10, 64, 64, 3, 1),       # M = 360: crosses a 256-row tile, all four borders
    (2, 9, 7, 128, 64, 3, 2),        # odd extents, OH x OW = 5 x 4
    (1, 8, 8, 64, 64, 3, 2),         # even extents: the last row and column receive fewer taps
    (2, 9, 7, 128, 256, 1, 2),       # the downsample: dX exactly zero at skipped pixels
    (1, 2, 2, 2048, 512, 1, 1),      # the product's channel depths at M = 4: below one MFMA k-step of pixels for wgrad
    (1, 2, 2, 512, 2048, 1, 1),
    (4, 14, 14, 64, 64, 3, 1),       # M = 784: two shares of the pixel reduction (512 pixels per share at least)
]
IDS = ["%dx%dx%d_%dto%d_k%ds%d" % g for g in GEOMETRIES]


def bf16_values(rs, shape, scale=1.0):
    return torch.from_numpy((scale * rs.standard_normal(shape)).astype(np.float32)).to(torch.bfloat16)


def nchw(t):
    return t.to(torch.float64).permute(0, 3, 1, 2).contiguous()


def out_hw(H, W, k, s):
    p = k // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def case(geom):
    """Operands (bf16, CPU) and fp64 references of one geometry, computed once and shared."""
    B, H, W, Cin, Cout, k, s = geom
    rs = np.random.RandomState(sum(geom))
    OH, OW = out_hw(H, W, k, s)
    x = bf16_values(rs, (B, H, W, Cin)).abs()                     # post-ReLU like: it doubles as the mask's source
    mask = torch.where(bf16_values(rs, (B, H, W, Cin)) > 0, x, torch.zeros_like(x))
    add = bf16_values(rs, (B, H, W, Cin))
    dy = bf16_values(rs, (B, OH, OW, Cout))
    wt = bf16_values(rs, (Cout, k * k * Cin), (2.0 / (k * k * Cin)) ** 0.5)
    w64 = wt.to(torch.float64).view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    kw = dict(stride=s, padding=k // 2)
    shape = (B, Cin, H, W)
    dx = conv2d_input(shape, w64, nchw(dy), **kw).permute(0, 2, 3, 1)
    dx_mag = conv2d_input(shape, w64.abs(), nchw(dy).abs(), **kw).permute(0, 2, 3, 1)
    dw = conv2d_weight(nchw(x), w64.shape, nchw(dy), **kw).permute(0, 2, 3, 1).reshape(Cout, -1)
    dw_mag = conv2d_weight(nchw(x).abs(), w64.shape, nchw(dy).abs(), **kw).permute(0, 2, 3, 1).reshape(Cout, -1)
    db = dy.to(torch.float64).sum(dim=(0, 1, 2))
    db_mag = dy.to(torch.float64).abs().sum(dim=(0, 1, 2))
    return dict(x=x, mask=mask, add=add, dy=dy, wt=wt, dx=dx, dx_mag=dx_mag, dw=dw, dw_mag=dw_mag, db=db, db_mag=db_mag)


def check_dgrad(got, ref, mag, what):
    err = (got.cpu().to(torch.float64) - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + 1e-6 * mag
    worst = float((err - bound).max())
    print("%s: max err %.3e, max (err - bound) %.3e" % (what, float(err.max()), worst))
    assert worst <= 0, what


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_dgrad_with_and_without_mask_and_add(geom):
    B, H, W, Cin, Cout, k, s = geom
    c = case(geom)
    dy, wt = c["dy"].to(DEV), c["wt"].to(DEV)
    wT = ops.conv_transpose_pack(wt, k)
    assert torch.equal(wT.cpu(), c["wt"].view(Cout, k * k, Cin).permute(2, 1, 0).reshape(Cin, -1))
    mask, add = c["mask"].to(DEV), c["add"].to(DEV)
    keep = (c["mask"] > 0)
    for use_mask in (False, True):
        for use_add in (False, True):
            kw = dict(mask=mask if use_mask else None, add=add if use_add else None)
            got = ops.conv_dgrad_bf16_nhwc(dy, wT, (H, W), k, s, k // 2, **kw)
            again = ops.conv_dgrad_bf16_nhwc(dy, wT, (H, W), k, s, k // 2, **kw)
            assert torch.equal(got, again)                           # bit-identical from call to call
            ref, mag = c["dx"], c["dx_mag"]
            if use_add:
                ref, mag = ref + c["add"].to(torch.float64), mag + c["add"].to(torch.float64).abs()
            if use_mask:
                ref, mag = ref * keep, mag * keep
                assert (got.cpu()[~keep] == 0).all()
            assert ref.abs().max() > 0
            check_dgrad(got, ref, mag, "dgrad %s mask=%s add=%s" % (geom, use_mask, use_add))
    if k == 1 and s == 2:                                            # pixels no output reads: exactly zero
        got = ops.conv_dgrad_bf16_nhwc(dy, wT, (H, W), k, s, 0).cpu()
        skipped = torch.ones(H, W, dtype=torch.bool)
        skipped[::2, ::2] = False
        assert (got[:, skipped] == 0).all() and (got[:, ~skipped] != 0).any()


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_wgrad_and_bias_gradient(geom):
    B, H, W, Cin, Cout, k, s = geom
    c = case(geom)
    x, dy = c["x"].to(DEV), c["dy"].to(DEV)
    dw, db = ops.conv_wgrad_bf16_nhwc(x, dy, k, s, k // 2)
    dw2, db2 = ops.conv_wgrad_bf16_nhwc(x, dy, k, s, k // 2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert dw.dtype == db.dtype == torch.float32 and tuple(dw.shape) == (Cout, k * k * Cin)
    err = (dw.cpu().to(torch.float64) - c["dw"]).abs()
    print("wgrad %s: max err / magnitude %.3e" % (geom, float((err / c["dw_mag"].clamp_min(1e-30)).max())))
    assert c["dw"].abs().max() > 0 and (err <= 1e-6 * c["dw_mag"]).all()
    err = (db.cpu().to(torch.float64) - c["db"]).abs()
    assert c["db"].abs().max() > 0 and (err <= 1e-6 * c["db_mag"]).all()


def test_the_784_pixel_case_takes_two_shares():
    from mgnns_amd import _lib
    L = _lib.lib()
    assert L.mgnns_conv_wgrad_workspace_bytes(4, 14, 14, 64, 64, 3, 3, 1, 1) == 2 * (64 * 576 + 64) * 4
    assert L.mgnns_conv_wgrad_workspace_bytes(3, 12, 10, 64, 64, 3, 3, 1, 1) == 0        # M = 360: one share, no workspace


@pytest.mark.parametrize("k,s,H,W", [(3, 1, 6, 5), (3, 2, 7, 6), (1, 2, 5, 5)])
def test_one_hot_operands_land_on_single_taps(k, s, H, W):
    """A transposed or flipped tap that a tolerance on random data can hide: a one-hot dY against a one-hot X gives ONE tap of dW',
    and a one-hot dY against a filter of distinct tap values gives the filter's footprint in dX, tap (kh, kw) at input pixel
    (oh s - p + kh, ow s - p + kw)."""
    Cin = Cout = 64
    p = k // 2
    OH, OW = out_hw(H, W, k, s)
    oh, ow, o, c = OH - 2, 1, 37, 5
    dy = torch.zeros(1, OH, OW, Cout, dtype=torch.bfloat16)
    dy[0, oh, ow, o] = 1.0
    for kh in range(k):
        for kw in range(k):
            ih, iw = oh * s - p + kh, ow * s - p + kw
            assert 0 <= ih < H and 0 <= iw < W
            x = torch.zeros(1, H, W, Cin, dtype=torch.bfloat16)
            x[0, ih, iw, c] = 2.0
            dw, db = ops.conv_wgrad_bf16_nhwc(x.to(DEV), dy.to(DEV), k, s, p)
            want = torch.zeros(Cout, k, k, Cin)
            want[o, kh, kw, c] = 2.0
            assert torch.equal(dw.cpu().view(Cout, k, k, Cin), want), (kh, kw)
            assert db.cpu()[o] == 1.0 and db.cpu().sum() == 1.0
    wt = torch.zeros(Cout, k, k, Cin)
    wt[o, :, :, c] = torch.arange(1, k * k + 1, dtype=torch.float32).view(k, k)
    wT = ops.conv_transpose_pack(wt.view(Cout, -1).to(torch.bfloat16).to(DEV), k)
    dx = ops.conv_dgrad_bf16_nhwc(dy.to(DEV), wT, (H, W), k, s, p).cpu().float()
    want = torch.zeros(1, H, W, Cin)
    for kh in range(k):
        for kw in range(k):
            want[0, oh * s - p + kh, ow * s - p + kw, c] = wt[o, kh, kw, c]
    assert torch.equal(dx, want)


def test_empty_batch_and_refusals():
    wT = torch.zeros(64, 9 * 64, dtype=torch.bfloat16, device=DEV)
    dx = ops.conv_dgrad_bf16_nhwc(torch.zeros(0, 6, 5, 64, dtype=torch.bfloat16, device=DEV), wT, (6, 5), 3, 1, 1)
    assert tuple(dx.shape) == (0, 6, 5, 64)
    e = torch.zeros(0, 6, 5, 64, dtype=torch.bfloat16, device=DEV)
    dw, db = ops.conv_wgrad_bf16_nhwc(e, e, 3, 1, 1)
    assert tuple(dw.shape) == (64, 576) and not dw.any() and not db.any()
    g = ops.map_grad_relu_nhwc(torch.zeros(0, 64, 2, 2, device=DEV), torch.zeros(0, 64, 2, 2, device=DEV))
    assert tuple(g.shape) == (0, 2, 2, 64)
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r"powers of two.*C_in=96"):
        ops.conv_wgrad_bf16_nhwc(z(1, 4, 4, 96), z(1, 4, 4, 64), 1, 1, 0)
    with pytest.raises(RuntimeError, match=r"powers of two.*C_in=96.*H=4 W=4"):
        ops.conv_dgrad_bf16_nhwc(z(1, 4, 4, 64), z(96, 64), (4, 4), 1, 1, 0)
    with pytest.raises(RuntimeError, match=r"1x1 or 3x3 \(got 5x5"):
        ops.conv_wgrad_bf16_nhwc(z(1, 8, 8, 64), z(1, 8, 8, 64), 5, 1, 2)
    with pytest.raises(RuntimeError, match=r"1x1 or 3x3 \(got 5x5"):
        ops.conv_dgrad_bf16_nhwc(z(1, 8, 8, 64), z(64, 25 * 64), (8, 8), 5, 1, 2)
    with pytest.raises(RuntimeError, match=r"stride 3"):
        ops.conv_dgrad_bf16_nhwc(z(1, 2, 2, 64), z(64, 64), (4, 4), 1, 3, 0)
    off = z(4 * 4 * 64 + 4)[4:].view(1, 4, 4, 64)                  # 8 bytes past a 16-byte boundary
    with pytest.raises(RuntimeError, match=r"16-byte aligned \(B=1 H=4 W=4 C_in=64 C_out=64\)"):
        ops.conv_dgrad_bf16_nhwc(off, z(64, 64), (4, 4), 1, 1, 0)
    with pytest.raises(RuntimeError, match=r"16-byte aligned \(B=1 H=4 W=4 C_in=64 C_out=64\)"):
        ops.conv_wgrad_bf16_nhwc(off, z(1, 4, 4, 64), 1, 1, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.conv_wgrad_bf16_nhwc(torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16), z(1, 4, 4, 64), 1, 1, 0)


@pytest.mark.parametrize("Cout,Cin,k", [(64, 128, 3), (256, 64, 1)])
def test_bn_unfold_matches_fp64(Cout, Cin, k):
    rs = np.random.RandomState(Cout + k)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    w, dwp, dbp = f(Cout, Cin, k, k), f(Cout, k * k * Cin), f(Cout)
    gamma, mean, var, eps = f(Cout), f(Cout), torch.from_numpy(rs.uniform(0.5, 1.5, Cout).astype(np.float32)), 1e-5
    dev = lambda t: t.to(DEV)
    dW, dg, dbeta = ops.conv_bn_unfold(dev(dwp), dev(dbp), dev(w), (dev(gamma), dev(mean), dev(var), eps))
    again = ops.conv_bn_unfold(dev(dwp), dev(dbp), dev(w), (dev(gamma), dev(mean), dev(var), eps))
    assert all(torch.equal(a, b) for a, b in zip((dW, dg, dbeta), again))
    d = lambda t: t.to(torch.float64)
    r = 1.0 / torch.sqrt(d(var) + eps)
    g64 = d(dwp).view(Cout, k, k, Cin).permute(0, 3, 1, 2)
    want_dW = (d(gamma) * r)[:, None, None, None] * g64
    prod = d(w) * g64
    want_dg = r * (prod.sum(dim=(1, 2, 3)) - d(mean) * d(dbp))
    mag_dg = r * (prod.abs().sum(dim=(1, 2, 3)) + (d(mean) * d(dbp)).abs())
    assert ((dW.cpu().to(torch.float64) - want_dW).abs() <= 1e-6 * want_dW.abs()).all()
    assert ((dg.cpu().to(torch.float64) - want_dg).abs() <= 1e-6 * mag_dg).all() and want_dg.abs().max() > 0
    assert torch.equal(dbeta.cpu(), dbp)
    only = ops.conv_bn_unfold(dev(dwp), dev(dbp), dev(w), (dev(gamma), dev(mean), dev(var), eps), want=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], dg)


def test_map_gradient_entry_matches_torch():
    rs = np.random.RandomState(4)
    fmap = torch.from_numpy(rs.standard_normal((3, 72, 3, 5)).astype(np.float32)).clamp_min(0).to(DEV)
    dmap = torch.from_numpy(rs.standard_normal((3, 72, 3, 5)).astype(np.float32)).to(DEV)
    g = ops.map_grad_relu_nhwc(fmap, dmap)
    want = torch.where(fmap > 0, dmap, torch.zeros_like(dmap)).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    assert g.dtype == torch.bfloat16 and torch.equal(g, want) and (g == 0).any() and (g != 0).any()
