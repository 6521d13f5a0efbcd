"""fp64 CPU reference of the stem's backward GIVEN the forward, the counterpart of tests/trunk_train_ref.py and
tests/trunk_bn_train_ref.py: gradients are computed from exactly what the stem Functions saved -- the ReLU's mask is `y0 > 0`, the
pool's argmax is taken from the saved y0 by the first-maximum rule (row-major scan of a window's valid positions, strict >), the
convolution's input is the kept bf16 image, and in batch mode the BatchNorm sees the saved z0 and (mean, rstd).

Two forms: R1 carries the gradients between layers in fp64; R2 (round=True) rounds them to bf16 where the kernels round: g_y0 after
the pool's backward and the mask, and g_z0 after the BatchNorm's backward.  Sums (dW, dgamma, dbeta) are never rounded.

`saved` is what train.TrunkStemFunction hands to keep=: {"img": [B,3,H,W] bf16, "y0", "y": NHWC bf16} and,
in batch mode, {"z0": NHWC bf16, "stats": (mean, rstd)}."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

from tests.trunk_bn_train_ref import bn_backward
from tests.trunk_train_ref import fold_cpu, nchw64, rb, rel_l2, unfold  # noqa: F401  (shared helpers)

NEG = float("-inf")


def pool_windows(x):
    """x [B,C,H,W] fp64 -> the 3x3 / stride 2 / pad 1 windows as [B, C, 9, OH*OW], positions in row-major (dh, dw) order and padding
    as -inf (never a maximum: every window holds at least one valid position)."""
    B, C, H, W = x.shape
    # the pool needs rows -1 .. 2 (OH - 1) + 1: pad by one in front and by whatever that leaves behind (0 or 1)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (1, 2 * OW - W, 1, 2 * OH - H), value=NEG)
    return F.unfold(xp, 3, stride=2).view(B, C, 9, OH * OW), xp.shape[2:], (OH, OW)


def first_max(win):
    """The first maximum of every window by an explicit scan with a strict > (torch.argmax is not relied upon)."""
    best = win[:, :, 0]
    idx = torch.zeros(best.shape, dtype=torch.int64)
    for p in range(1, 9):
        better = win[:, :, p] > best
        best = torch.where(better, win[:, :, p], best)
        idx = torch.where(better, torch.full_like(idx, p), idx)
    # a window whose first positions are padding starts at -inf: its index is that of the first position above -inf, which the
    # strict > found, unless every valid value is -inf itself (not the case for finite activations)
    return idx


def maxpool_backward(x, gy):
    """Backward of max_pool2d(3, 2, 1): x [B,C,H,W] (the pool's input), gy [B,C,OH,OW] -> gx like x, fp64."""
    B, C, H, W = x.shape
    win, padded, (OH, OW) = pool_windows(x)
    idx = first_max(win)
    hot = torch.zeros_like(win).scatter_(2, idx[:, :, None], gy.reshape(B, C, 1, OH * OW))
    gxp = F.fold(hot.view(B, C * 9, OH * OW), padded, 3, stride=2)
    return gxp[:, :, 1:1 + H, 1:1 + W].contiguous()


def tie_fraction(x):
    """The share of windows whose maximum is attained more than once."""
    win = pool_windows(x)[0]
    return float(((win == win.max(dim=2, keepdim=True).values).sum(dim=2) > 1).double().mean())


def stem_backward(conv, bn, saved, g_y, round=False):
    """-> (dW like conv.weight, dgamma, dbeta), fp64.  g_y: the gradient of the pooled output, NHWC (as the stage Function returns
    it) or NCHW.  Frozen statistics when `saved` has no "z0", batch statistics when it has."""
    q = rb if round else (lambda t: t)
    img = saved["img"].detach().cpu().double()
    y0 = nchw64(saved["y0"])
    g = g_y.detach().cpu().double()
    if g.shape[1:] != y0.shape[1:2] + ((y0.shape[2] - 1) // 2 + 1, (y0.shape[3] - 1) // 2 + 1):
        g = g.permute(0, 3, 1, 2)
    g_y0 = q(maxpool_backward(y0, g) * (y0 > 0))
    shape = conv.weight.shape
    if "z0" not in saved:
        dwp = conv2d_weight(img, shape, g_y0, stride=2, padding=3)
        return unfold(dwp, g_y0.sum(dim=(0, 2, 3)), conv, bn)
    mean, rstd = saved["stats"]
    gz, dgamma, dbeta = bn_backward(g_y0, nchw64(saved["z0"]), mean, rstd, bn.weight, q)
    return conv2d_weight(img, shape, gz, stride=2, padding=3), dgamma, dbeta


def grid(t, step=0.5):
    """t on a coarse grid (multiples of `step`, exact in bf16): what makes most of a map's pooling windows tie."""
    return torch.round(t / step) * step


def forward_cpu(conv, bn, img, batch, step=0.5):
    """A stem forward on the CPU for tests that run without a GPU: img [B,3,H,W] fp64 (bf16 valued) -> `saved` in the layout the
    Functions keep, with y0 drawn through grid(): more than half of the windows then hold their maximum twice or more."""
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    saved = {"img": img.to(torch.bfloat16)}
    if batch:
        z0 = rb(F.conv2d(img, rb(conv.weight.detach().double()), None, stride=2, padding=3))
        mean = z0.mean(dim=(0, 2, 3))
        rstd = 1.0 / torch.sqrt(z0.var(dim=(0, 2, 3), unbiased=False) + bn.eps)
        a = (bn.weight.detach().double() * rstd)[None, :, None, None]
        pre = a * z0 + (bn.bias.detach().double() - mean * bn.weight.detach().double() * rstd)[None, :, None, None]
        saved["z0"], saved["stats"] = nhwc(z0), (mean, rstd)
    else:
        wf, bf = fold_cpu(conv, bn)
        pre = F.conv2d(img, wf, bf, stride=2, padding=3)
    y0 = grid(torch.relu(pre), step)
    saved["y0"] = nhwc(y0)
    saved["y"] = nhwc(F.max_pool2d(y0, 3, 2, 1))
    return saved
