"""fp64 CPU reference of the trunk stages' backward GIVEN the forward: the gradients are computed from exactly the
activations the stage Function saved -- masks are `saved > 0`, convolution inputs are the saved bf16 values, weights are the folded
bf16 w' -- so no CPU-side pre-activation can land on the other side of zero and the bf16 forward's own error (3-8 % of the
parameter gradients against an all-fp64 network) is neither charged to the backward nor able to hide its errors.

Two forms: R1 carries the gradients between layers in fp64; R2 (round=True) rounds them to bf16 where the kernels round: the masked
map gradient at the entry and every data gradient after its add and mask (the downsample's data gradient on its own, before it
is added)."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight


def rb(t):
    """Round to bf16 (nearest even) and back to fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def nchw64(t):
    """A saved activation as NCHW fp64: NHWC bf16 tensors are permuted, the fp32 NCHW map is taken as it is."""
    t = t.detach().cpu()
    return t.to(torch.float64) if t.dtype == torch.float32 else t.to(torch.float64).permute(0, 3, 1, 2).contiguous()


def folded_from_pack(wt, k):
    """The folded bf16 weight [Cout, (kh, kw, c)] of ops.conv_fold_bn as [Cout, Cin, k, k] fp64."""
    wt = wt.detach().cpu().to(torch.float64)
    return wt.view(wt.shape[0], k, k, -1).permute(0, 3, 1, 2).contiguous()


def fold_cpu(conv, bn):
    """(w' rounded to bf16 as fp64 [Cout, Cin, k, k], b' fp64) of a frozen-statistics BatchNorm folded into its convolution."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return rb(conv.weight.detach().double() * scale[:, None, None, None]), bn.bias.detach().double() - bn.running_mean.double() * scale


def block_layers(blk):
    layers = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
    if blk.downsample is not None:
        layers.append((blk.downsample[0], blk.downsample[1]))
    return layers


def forward_cpu(blocks, x):
    """A bf16-rounded eval forward on the CPU, for tests that run without a GPU: x NCHW fp64 (already bf16 valued) -> `saved` in
    the layout the stage Function keeps (NHWC bf16, the last output an fp32 NCHW map)."""
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    saved = {"x": nhwc(x), "blocks": []}
    y = x
    for i, blk in enumerate(blocks):
        f = [fold_cpu(c, b) + (c.stride[0], c.padding[0]) for c, b in block_layers(blk)]
        conv = lambda t, j: F.conv2d(t, f[j][0], f[j][1], stride=f[j][2], padding=f[j][3])
        idn = rb(conv(y, 3)) if len(f) == 4 else y
        o1 = rb(torch.relu(conv(y, 0)))
        o2 = rb(torch.relu(conv(o1, 1)))
        out = torch.relu(conv(o2, 2) + idn)
        last = i == len(blocks) - 1
        y = out.float().double() if last else rb(out)
        saved["blocks"].append((nhwc(o1), nhwc(o2), out.float() if last else nhwc(y)))
    return saved


def unfold(dwp, dbp, conv, bn):
    """(dW, dgamma, dbeta) of the fp32 master parameters from the folded pair's gradients, fp64."""
    r = 1.0 / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
    w = conv.weight.detach().cpu().double()
    gamma, mean = bn.weight.detach().cpu().double(), bn.running_mean.detach().cpu().double()
    return ((gamma * r)[:, None, None, None] * dwp, r * ((w * dwp).sum(dim=(1, 2, 3)) - mean * dbp), dbp)


def stage_backward(blocks, saved, folded, dmap, round=False, input_grad=False):
    """-> (grads, gx): grads[block][layer] = (dW, dgamma, dbeta) fp64 in block_layers order, gx = the gradient of the stage input
    (NCHW fp64) or None.  blocks: the Bottlenecks (for geometry and the fp32 master parameters); saved: what the stage Function
    kept; folded[block][layer] = w' as [Cout, Cin, k, k] fp64; dmap: the gradient of the output map."""
    q = rb if round else (lambda t: t)
    x0 = nchw64(saved["x"])
    acts = [tuple(nchw64(t) for t in b) for b in saved["blocks"]]
    g = q(torch.where(acts[-1][2] > 0, dmap.detach().cpu().double(), torch.zeros((), dtype=torch.float64)))
    grads = [None] * len(blocks)
    for bi in range(len(blocks) - 1, -1, -1):
        layers = block_layers(blocks[bi])
        geo = [dict(stride=c.stride[0], padding=c.padding[0]) for c, _ in layers]
        w = folded[bi]
        x_in = acts[bi - 1][2] if bi else x0
        o1, o2, _ = acts[bi]

        def wg(j, inp, gy):
            return unfold(conv2d_weight(inp, w[j].shape, gy, **geo[j]), gy.sum(dim=(0, 2, 3)), *layers[j])
        out = [None] * len(layers)
        out[2] = wg(2, o2, g)
        if len(layers) == 4:
            out[3] = wg(3, x_in, g)
        g2 = q(conv2d_input(o2.shape, w[2], g, **geo[2]) * (o2 > 0))
        out[1] = wg(1, o1, g2)
        g1 = q(conv2d_input(o1.shape, w[1], g2, **geo[1]) * (o1 > 0))
        out[0] = wg(0, x_in, g1)
        grads[bi] = out
        if bi == 0 and not input_grad:
            return grads, None
        other = q(conv2d_input(x_in.shape, w[3], g, **geo[3])) if len(layers) == 4 else g
        gx = conv2d_input(x_in.shape, w[0], g1, **geo[0]) + other
        g = q(gx * (x_in > 0) if bi else gx)
    return grads, g


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
