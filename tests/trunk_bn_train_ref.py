"""fp64 CPU reference of the trunk stages' batch-statistics backward GIVEN the forward, the counterpart of
tests/trunk_train_ref.py: gradients are computed from exactly what the stage Function saved -- the pre-normalisation outputs z, the
activations (masks are `saved > 0`), the per-layer (mean, rstd) and the raw bf16 weights -- so the bf16 forward's own error is neither
charged to the backward nor able to hide its errors.

Two forms: R1 carries the gradients between layers in fp64; R2 (round=True) rounds them to bf16 where the kernels round: the masked
map gradient at the entry, every g_z a BatchNorm backward returns, and every data gradient after its add and mask (the downsample's
data gradient on its own, before it is added).  Sums (dgamma, dbeta, dW) are never rounded.

`saved` is what train.TrunkStageFunction hands to keep= in 'batch' mode: {"x", "blocks": [{"z": [...], "stats": [(mean, rstd), ...],
"o1", "o2", "out", "idn"}]}, z and stats in block_layers order."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from tests.trunk_train_ref import block_layers, folded_from_pack, nchw64, rb, rel_l2  # noqa: F401  (shared helpers)

raw_from_pack = folded_from_pack       # a raw pack has the folded pack's layout: [Cout, (kh, kw, c)] bf16


def raw_cpu(conv):
    """bf16(conv.weight) as fp64 [Cout, Cin, k, k]: what trunk.block_packs_raw holds."""
    return rb(conv.weight.detach().double())


def vec(t):
    return t.detach().cpu().double()[None, :, None, None]


def bn_apply(z, mean, rstd, bn):
    """gamma (z - mean) rstd + beta the way the kernel forms it: a z + b with a = gamma rstd, b = beta - mean a (fp64 here)."""
    a = vec(bn.weight) * vec(rstd)
    return a * z + (vec(bn.bias) - vec(mean) * a)


def forward_cpu(blocks, x):
    """A bf16-rounded batch-statistics forward on the CPU, for tests that run without a GPU: x NCHW fp64 (already bf16 valued) ->
    `saved` in the layout the stage Function keeps (NHWC bf16, the last output an fp32 NCHW map), with the statistics of the ROUNDED z
    left in fp64 so that plain autograd through F.batch_norm sees the very same numbers.  Leaves the modules' buffers alone."""
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    saved = {"x": nhwc(x), "blocks": []}
    y = x
    for i, blk in enumerate(blocks):
        layers = block_layers(blk)

        def conv_bn(t, j, residual=None, relu=True):
            c, bn = layers[j]
            z = rb(F.conv2d(t, raw_cpu(c), None, stride=c.stride[0], padding=c.padding[0]))
            mean = z.mean(dim=(0, 2, 3))
            rstd = 1.0 / torch.sqrt(z.var(dim=(0, 2, 3), unbiased=False) + bn.eps)
            o = bn_apply(z, mean, rstd, bn)
            if residual is not None:
                o = o + residual
            return z, (mean, rstd), torch.relu(o) if relu else o
        zs, sts = [None] * len(layers), [None] * len(layers)
        idn = y
        if len(layers) == 4:
            zs[3], sts[3], idn = conv_bn(y, 3, relu=False)
            idn = rb(idn)
        zs[0], sts[0], o1 = conv_bn(y, 0)
        o1 = rb(o1)
        zs[1], sts[1], o2 = conv_bn(o1, 1)
        o2 = rb(o2)
        zs[2], sts[2], out = conv_bn(o2, 2, residual=idn)
        last = i == len(blocks) - 1
        y = out.float().double() if last else rb(out)
        saved["blocks"].append({"z": [nhwc(z) for z in zs], "stats": sts, "o1": nhwc(o1), "o2": nhwc(o2),
                                "out": out.float() if last else nhwc(y), "idn": nhwc(idn)})
    return saved


def bn_backward(g, z, mean, rstd, gamma, q):
    """-> (g_z, dgamma, dbeta) of training-mode BatchNorm, differentiated through the statistics; q rounds g_z."""
    xhat = (z - vec(mean)) * vec(rstd)
    M = z.numel() // z.shape[1]
    dbeta = g.sum(dim=(0, 2, 3))
    dgamma = (g * xhat).sum(dim=(0, 2, 3))
    gz = vec(gamma) * vec(rstd) * (g - dbeta[None, :, None, None] / M - xhat * dgamma[None, :, None, None] / M)
    return q(gz), dgamma, dbeta


def stage_backward(blocks, saved, raw, dmap, round=False, input_grad=False):
    """-> (grads, gx): grads[block][layer] = (dW, dgamma, dbeta) fp64 in block_layers order, gx = the gradient of the stage input
    (NCHW fp64) or None.  raw[block][layer] = bf16(conv.weight) as [Cout, Cin, k, k] fp64; dmap: the gradient of the output map."""
    q = rb if round else (lambda t: t)
    x0 = nchw64(saved["x"])
    outs = [nchw64(b["out"]) for b in saved["blocks"]]
    g = q(torch.where(outs[-1] > 0, dmap.detach().cpu().double(), torch.zeros((), dtype=torch.float64)))
    grads = [None] * len(blocks)
    for bi in range(len(blocks) - 1, -1, -1):
        layers = block_layers(blocks[bi])
        geo = [dict(stride=c.stride[0], padding=c.padding[0]) for c, _ in layers]
        w = raw[bi]
        sv = saved["blocks"][bi]
        zs = [nchw64(t) for t in sv["z"]]
        x_in = outs[bi - 1] if bi else x0
        o1, o2 = nchw64(sv["o1"]), nchw64(sv["o2"])
        out = [None] * len(layers)

        def layer(j, inp, gy):
            gz, dg, db = bn_backward(gy, zs[j], sv["stats"][j][0], sv["stats"][j][1], layers[j][1].weight, q)
            out[j] = (conv2d_weight(inp, w[j].shape, gz, **geo[j]), dg, db)
            return gz
        gz3 = layer(2, o2, g)
        gzd = layer(3, x_in, g) if len(layers) == 4 else None
        gz2 = layer(1, o1, q(conv2d_input(o2.shape, w[2], gz3, **geo[2]) * (o2 > 0)))
        gz1 = layer(0, x_in, q(conv2d_input(o1.shape, w[1], gz2, **geo[1]) * (o1 > 0)))
        grads[bi] = out
        if bi == 0 and not input_grad:
            return grads, None
        other = q(conv2d_input(x_in.shape, w[3], gzd, **geo[3])) if gzd is not None else g
        gx = conv2d_input(x_in.shape, w[0], gz1, **geo[0]) + other
        g = q(gx * (x_in > 0) if bi else gx)
    return grads, g


def rounding_noise(r1, r2, x1=None, x2=None):
    """e = the largest |R2 - R1| / |R1| over the gradient tensors."""
    e = max(rel_l2(b, a) for ba, bb in zip(r1, r2) for la, lb in zip(ba, bb) for a, b in zip(la, lb))
    return max(e, rel_l2(x2, x1)) if x1 is not None else e


# the three stage inputs both test files use: (stage widths as narrow_stage arguments, input shape NCHW, input seed, dmap seed)
CASES = {
    "two_blocks": ([(128, 64, 2, 2, 3)], (3, 128, 12, 10), 1, 2),
    "three_blocks": ([(256, 64, 3, 2, 4)], (2, 256, 9, 7), 5, 6),
    "two_stages": ([(128, 64, 2, 2, 8), (256, 64, 2, 2, 9)], (2, 128, 9, 11), 7, 8),
}


def case_input(name):
    """The case's stage input as NCHW fp32 with bf16 values (|N(0,1)|, as a ReLU's output), and its dmap seed."""
    _, shape, seed, dseed = CASES[name]
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).abs().to(torch.bfloat16).float()
    return x, dseed
