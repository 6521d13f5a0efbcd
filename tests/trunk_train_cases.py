"""Cases, generators, references, launcher restatements and mutants of the trunk-backward edge sweep: the bottleneck convolutions'
gradients (csrc/conv_train.hip), the stem's (csrc/stem_train.hip) and training-mode BatchNorm (csrc/bn_train.hip).
tests/test_trunk_train_edges_gpu.py runs the kernels on these cases; tests/test_trunk_train_edges_cpu.py checks this file itself (the
restatements against the library's host arithmetic, every case's claim, legality and exactness budget, the references against torch's
autograd in double, and that the wrong kernels below -- the mutants -- would be caught).

Two kinds of operands per case.  "int": small integers, exact in bf16, every partial sum below 2^24, so fp32 accumulation is exact in
ANY order and a kernel must equal the fp64 reference bit for bit.  "gauss": Gaussian values rounded to bf16, under the gates the
kernels' own tests derived.  The references are plain loops over filter taps or windows in the precision of their
operands, not the kernels' index arithmetic: the data gradient scatters where the kernel gathers, the weight gradient multiplies whole
[M, C] patches, the pool scans whole strided slices."""
import numpy as np
import torch

from oracle.bf16_path import bf16_round

EXACT = 1 << 24                         # integers below this are exact in fp32, and so is every sum of them


def ceil_div(a, b):
    return (a + b - 1) // b


def t32(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))


def rbf(t):
    """fp32 values rounded to bf16, as fp32"""
    return t.to(torch.bfloat16).float()


# ---- the host arithmetic of the three files, restated -------------------------------------------------------------------------------------
def conv_train_geometry(B, H, W, Cin, Cout, KH, KW, stride, pad):
    """conv_train_geometry of csrc/conv_train.hip -> (OH, OW), or ValueError with the refusal's key words"""
    pow2_ge64 = lambda c: c >= 64 and c & (c - 1) == 0
    if not (B >= 0 and H > 0 and W > 0):
        raise ValueError("bad dims")
    if not (pow2_ge64(Cin) and pow2_ge64(Cout)):
        raise ValueError("powers of two")
    if (KH, KW) not in ((1, 1), (3, 3)):
        raise ValueError("1x1 or 3x3")
    if not (stride in (1, 2) and 0 <= pad <= KH // 2):
        raise ValueError("bad stride")
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    if not (OH > 0 and OW > 0):
        raise ValueError("empty output")
    if not (B * H * W < (1 << 31) - 256 and B * OH * OW < (1 << 31) - 256):
        raise ValueError("31 bits")
    return OH, OW


WG_SHARE_MIN = 512


def wgrad_shares(M, Cout, K):
    """wgrad_shares -> (nshare, share_len): the pixels of conv_wgrad_kernel's reduction, split over blockIdx.z"""
    tiles = (Cout // 64) * (K // 64)
    want = max(1024 // tiles, 1)
    most = max(ceil_div(M, WG_SHARE_MIN), 1)
    n = min(want, most)
    length = max(ceil_div(ceil_div(M, n), 32) * 32, 32)
    return max(ceil_div(M, length), 1), length


def wgrad_want(Cout, K):
    return max(1024 // ((Cout // 64) * (K // 64)), 1)


def wgrad_workspace_bytes(B, H, W, Cin, Cout, k, stride, pad):
    """mgnns_conv_wgrad_workspace_bytes (0: refused, empty, or one share)"""
    try:
        OH, OW = conv_train_geometry(B, H, W, Cin, Cout, k, k, stride, pad)
    except ValueError:
        return 0
    if B == 0:
        return 0
    K = k * k * Cin
    nshare, _ = wgrad_shares(B * OH * OW, Cout, K)
    return nshare * (Cout * K + Cout) * 4 if nshare > 1 else 0


SW_ROWS, SW_COLS, SW_K, SW_KV, SW_MAX_WG = 8, 32, 160, 147, 256


def stem_wgrad_split(B, OH, OW):
    """stem_wgrad_split -> (ntr, ntc, ntiles, tpw, nwg): 8 x 32 tiles, tpw tiles in a row per workgroup, nwg partials"""
    ntr, ntc = ceil_div(OH, SW_ROWS), ceil_div(OW, SW_COLS)
    ntiles = B * ntr * ntc
    tpw = max(ceil_div(ntiles, SW_MAX_WG), 1)
    return ntr, ntc, ntiles, tpw, ceil_div(ntiles, tpw)


def stem_out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_wgrad_workspace_bytes(B, H, W):
    if B < 0 or H < 7 or W < 7 or B * H * W >= (1 << 31) - 256 or B == 0:
        return 0
    return stem_wgrad_split(B, *stem_out_hw(H, W))[4] * 64 * SW_K * 4


PB_ROWS, PB_COLS = 8, 16


def pool_bwd_tiles(B, H, W, C):
    """the launch of maxpool3x3s2_bwd_kernel -> (ntr, ntc, ncb, workgroups): 8 x 16 pixel tiles x blocks of 64 channels"""
    ntr, ntc, ncb = ceil_div(H, PB_ROWS), ceil_div(W, PB_COLS), ceil_div(C // 8, 8)
    return ntr, ntc, ncb, B * ntr * ntc * ncb


BN_ROWS_MIN, BN_SLABS_MAX, BN_BLOCKS = 16, 256, 2048


def bn_plan(M, C, reduce):
    """bn_plan -> dict(cgb, ry, gx, nslab, slab_len, last = rows of the last slab, dead = channel groups of the last workgroup
    without a channel)"""
    cg, widest = C // 8, 8 if reduce else 32
    cgb = 1
    while cgb < cg and cgb < widest:
        cgb *= 2
    ry, gx = 256 // cgb, ceil_div(cg, cgb)
    want = min(max(BN_BLOCKS // gx, 1), BN_SLABS_MAX)
    most = max(ceil_div(M, ry * BN_ROWS_MIN), 1)
    n = min(want, most)
    slab_len = max(ceil_div(ceil_div(M, n), ry) * ry, ry)
    nslab = max(ceil_div(M, slab_len), 1)
    return dict(cgb=cgb, ry=ry, gx=gx, nslab=nslab, slab_len=slab_len, last=M - (nslab - 1) * slab_len, dead=gx * cgb - cg)


def bn_workspace_bytes(M, C, backward):
    if C <= 0 or C % 8 or M < 2 or M >= (1 << 31) - 65536:
        return 0
    return bn_plan(M, C, True)["nslab"] * 2 * C * 4 + (2 * C * 4 if backward else 0)


# ---- convolution cases --------------------------------------------------------------------------------------------------------------------
def conv_case(k, stride, pad, Cin, Cout, B, H, W):
    return dict(k=k, stride=stride, pad=pad, Cin=Cin, Cout=Cout, B=B, H=H, W=W)


def out_hw(c):
    return (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1


def out_m(c):
    oh, ow = out_hw(c)
    return c["B"] * oh * ow


def in_m(c):
    return c["B"] * c["H"] * c["W"]


def kdim(c):
    return c["k"] * c["k"] * c["Cin"]


# Weight gradient: name -> case; M = output pixels.  WGRAD_CLAIMS: (nshare, share_len, pixels of the last share) by wgrad_shares.
WGRAD_CASES = {
    "odd_m25_one_share": conv_case(1, 1, 0, 64, 64, 1, 5, 5),                   # the pair (24, 25) has one pixel
    "m3_less_than_a_step": conv_case(1, 1, 0, 128, 64, 1, 1, 3),
    "two_shares_odd_last": conv_case(1, 1, 0, 64, 64, 1, 27, 19),               # M = 513
    "three_shares_boundary_in_a_row": conv_case(1, 1, 0, 64, 64, 5, 5, 41),     # M = 1025: 352 = 8 rows of 41 + 24
    "three_shares_3x3": conv_case(3, 1, 1, 64, 64, 5, 5, 41),                   # the same split with padding taps at both boundaries
    "last_share_of_one_pixel": conv_case(1, 1, 0, 64, 64, 1, 1, 7681),
    "cap_want1_3x3_512": conv_case(3, 1, 1, 512, 512, 1, 27, 19),               # K = 4608: 576 tiles, one share however many pixels
    "cap_want4_512to2048": conv_case(1, 1, 0, 512, 2048, 1, 3, 683),            # M = 2049, 256 tiles: 4 shares, not 5
    "k3_cin256_s1": conv_case(3, 1, 1, 256, 64, 2, 5, 7),                       # c0 in {0, 64, 128, 192} inside a tap
    "k3_cin256_s2": conv_case(3, 2, 1, 256, 64, 2, 9, 7),
    "k3_cin512_s2": conv_case(3, 2, 1, 512, 64, 1, 7, 6),
    "k3_pad0_s1": conv_case(3, 1, 0, 64, 64, 2, 7, 8),
    "k3_pad0_s2": conv_case(3, 2, 0, 128, 64, 2, 8, 7),
    "k1_s2_even": conv_case(1, 2, 0, 64, 128, 2, 8, 6),
    "k1_s2_odd": conv_case(1, 2, 0, 64, 128, 2, 9, 7),
    "h1_3x3": conv_case(3, 1, 1, 64, 64, 2, 1, 9),
    "w1_3x3_s2": conv_case(3, 2, 1, 64, 64, 2, 9, 1),
}
WGRAD_CLAIMS = {
    "odd_m25_one_share": (1, 32, 25), "m3_less_than_a_step": (1, 32, 3), "two_shares_odd_last": (2, 288, 225),
    "three_shares_boundary_in_a_row": (3, 352, 321), "three_shares_3x3": (3, 352, 321), "last_share_of_one_pixel": (16, 512, 1),
    "cap_want1_3x3_512": (1, 544, 513), "cap_want4_512to2048": (4, 544, 417), "k3_cin256_s1": (1, 96, 70), "k3_cin256_s2": (1, 64, 40),
    "k3_cin512_s2": (1, 32, 12), "k3_pad0_s1": (1, 64, 60), "k3_pad0_s2": (1, 32, 18), "k1_s2_even": (1, 32, 24), "k1_s2_odd": (1, 64, 40),
    "h1_3x3": (1, 32, 18), "w1_3x3_s2": (1, 32, 10),
}


def wgrad_plan(c):
    M = out_m(c)
    nshare, share_len = wgrad_shares(M, c["Cout"], kdim(c))
    return nshare, share_len, M - (nshare - 1) * share_len


# Data gradient: M = input pixels, 128 per workgroup, 32 per wave.  DGRAD_CLAIMS: (M, workgroups across the pixels).
DGRAD_CASES = {
    "m128_two_images": conv_case(1, 1, 0, 64, 64, 2, 8, 8),
    "m129": conv_case(1, 1, 0, 64, 64, 3, 1, 43),
    "m127": conv_case(1, 1, 0, 64, 64, 1, 1, 127),
    "m1": conv_case(1, 1, 0, 64, 64, 1, 1, 1),
    "cout2048": conv_case(1, 1, 0, 64, 2048, 1, 2, 2),
    "cin2048": conv_case(1, 1, 0, 2048, 64, 1, 2, 2),
    "k3_128to256_tile_spans_images": conv_case(3, 1, 1, 128, 256, 3, 7, 8),     # M = 168: image 2 starts inside workgroup 0
}
for _k, _s, _p in ((1, 1, 0), (1, 2, 0), (3, 1, 0), (3, 1, 1), (3, 2, 0), (3, 2, 1)):       # every (k, stride, pad) the geometry accepts
    DGRAD_CASES["k%ds%dp%d_7x8" % (_k, _s, _p)] = conv_case(_k, _s, _p, 64, 64, 2, 7, 8)     # odd x even
    if _s == 2:
        DGRAD_CASES["k%ds%dp%d_8x7" % (_k, _s, _p)] = conv_case(_k, _s, _p, 64, 64, 2, 8, 7)  # even x odd
DGRAD_CLAIMS = {n: (in_m(c), ceil_div(in_m(c), 128)) for n, c in DGRAD_CASES.items()}
DGRAD_CLAIMS.update({"m128_two_images": (128, 1), "m129": (129, 2), "m127": (127, 1), "m1": (1, 1), "k3_128to256_tile_spans_images": (168, 2)})


def conv_operands(c, kind, seed=0):
    """-> dict of fp32 CPU tensors exact in bf16: x [B, H, W, Cin], dy [B, OH, OW, Cout], wt [Cout, k k Cin] with k = (kh, kw, c),
    add and mask [B, H, W, Cin].  "int": x, dy, wt in -4..4, add in -8..8; "gauss": N(0, 1) rounded to bf16, wt He-scaled, x >= 0 (post
    ReLU).  The mask is x where a coin says so, else one of 0, -0.0 and negative values -- all of which must zero the output."""
    rs = np.random.RandomState(1000 * c["k"] + 100 * c["stride"] + 10 * c["pad"] + c["Cin"] + 7 * c["Cout"] + 13 * c["B"] + 3 * c["H"] + c["W"] + seed)
    oh, ow = out_hw(c)
    xs, ys, K = (c["B"], c["H"], c["W"], c["Cin"]), (c["B"], oh, ow, c["Cout"]), kdim(c)
    if kind == "int":
        x, dy, wt, add = (t32(rs.randint(-4, 5, s)) for s in (xs, ys, (c["Cout"], K), xs))
        add = add * 2
        live = t32(rs.randint(1, 5, xs))
    else:
        x, dy, add = rbf(t32(rs.standard_normal(xs))).abs(), rbf(t32(rs.standard_normal(ys))), rbf(t32(rs.standard_normal(xs)))
        wt = rbf(t32((2.0 / K) ** 0.5 * rs.standard_normal((c["Cout"], K))))
        live = x.clamp_min(2.0 ** -10)
    dead = t32(np.array([0.0, -0.0, -1.0, -0.5], dtype=np.float32)[rs.randint(0, 4, xs)])
    mask = torch.where(t32(rs.randint(0, 2, xs)) > 0, live, dead)
    return dict(x=x, dy=dy, wt=wt, add=add, mask=mask)


def wgrad_budget(c):
    return 16 * out_m(c)


def dgrad_budget(c):
    return 16 * c["k"] * c["k"] * c["Cout"] + 8


def tap_patch(x, c, kh, kw, clamp=False):
    """[M, Cin]: the input pixel that output pixel m reads through tap (kh, kw), zeros where the tap is padding (clamp: the mutant that
    reads the nearest pixel instead)"""
    B, H, W, Cin = x.shape
    oh, ow = out_hw(c)
    ih, iw = torch.arange(oh) * c["stride"] - c["pad"] + kh, torch.arange(ow) * c["stride"] - c["pad"] + kw
    patch = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
    if not clamp:
        ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
        patch = patch * ok[None, :, :, None].to(x.dtype)
    return patch.reshape(-1, Cin)


WGRAD_MUTANTS = ("drop_last", "swap_pair", "clamp", "ignore_c0")


def wgrad_sum(x, dy, c, mutant=None):
    """(dW' [Cout, k k Cin], db' [Cout]) in the precision of x, tap by tap: dW'[o, (kh, kw, c)] = sum_m dY[m, o] X[pixel(m, kh, kw), c].
    Mutants, on the shares wgrad_shares gives: "drop_last" loses the last pixel of every share, "swap_pair" pairs dY of pixel 2q with X
    of pixel 2q + 1 and the other way round (a pixel whose partner lies beyond the share meets zeros), "clamp" reads the nearest pixel
    for a padding tap, "ignore_c0" reads channels 0..63 of a tap for every 64-wide column tile."""
    k, Cin, Cout = c["k"], c["Cin"], c["Cout"]
    M = out_m(c)
    d2 = dy.reshape(M, Cout)
    nshare, share_len = wgrad_shares(M, Cout, kdim(c))
    ends = [min(M, (s + 1) * share_len) for s in range(nshare)]
    if mutant == "drop_last":
        d2 = d2.clone()
        d2[[e - 1 for e in ends]] = 0
    dW = torch.zeros(Cout, k * k * Cin, dtype=x.dtype)
    for kh in range(k):
        for kw in range(k):
            P = tap_patch(x, c, kh, kw, clamp=(mutant == "clamp"))
            if mutant == "swap_pair":
                m = torch.arange(M)
                partner = m ^ 1
                end = torch.tensor(ends)[m // share_len]
                P = P[partner.clamp(max=M - 1)] * (partner < end)[:, None].to(x.dtype)
            if mutant == "ignore_c0":
                P = P[:, :64].repeat(1, Cin // 64)
            tap = kh * k + kw
            dW[:, tap * Cin:(tap + 1) * Cin] = d2.t() @ P
    return dW, d2.sum(0)


def wgrad_ref(x, dy, c, mutant=None):
    return wgrad_sum(x.double(), dy.double(), c, mutant)


DGRAD_MUTANTS = ("no_divisibility", "swap_taps", "add_after_mask")


def dgrad_sum(dy, wt, c):
    """dX [B, H, W, Cin] in the precision of dy, before add and mask, as a SCATTER tap by tap: output pixel (oh, ow) adds dY[b, oh, ow, :]
    w'[:, (kh, kw, :)] to input pixel (oh s - p + kh, ow s - p + kw) -- the transpose of the forward, with no division anywhere"""
    k, s, p, Cin, Cout = c["k"], c["stride"], c["pad"], c["Cin"], c["Cout"]
    B, H, W = c["B"], c["H"], c["W"]
    oh, ow = out_hw(c)
    w4 = wt.reshape(Cout, k, k, Cin)
    dxp = torch.zeros(B, H + 2 * p, W + 2 * p, Cin, dtype=dy.dtype)
    for kh in range(k):
        for kw in range(k):
            dxp[:, kh:kh + s * (oh - 1) + 1:s, kw:kw + s * (ow - 1) + 1:s] += dy @ w4[:, kh, kw, :]
    return dxp[:, p:p + H, p:p + W].contiguous()


def dgrad_gather(dy, wt, c, mutant=None):
    """The same sum as the GATHER the kernel runs: input pixel (ih, iw) takes tap (kh, kw) from oh = (ih + p - kh) / s where that is an
    integer inside the output.  Mutants: "no_divisibility" skips the integer test (the quotient truncates), "swap_taps" multiplies the
    pixel of tap (kh, kw) by the weights of tap (kw, kh)."""
    k, s, p, Cin, Cout = c["k"], c["stride"], c["pad"], c["Cin"], c["Cout"]
    H, W = c["H"], c["W"]
    oh, ow = out_hw(c)
    w4 = wt.reshape(Cout, k, k, Cin)
    dx = torch.zeros(c["B"], H, W, Cin, dtype=dy.dtype)
    for kh in range(k):
        for kw in range(k):
            th, tw = torch.arange(H) + p - kh, torch.arange(W) + p - kw
            qh, qw = torch.div(th, s, rounding_mode="trunc"), torch.div(tw, s, rounding_mode="trunc")
            okh, okw = (th >= 0) & (qh < oh), (tw >= 0) & (qw < ow)
            if mutant != "no_divisibility":
                okh, okw = okh & (qh * s == th), okw & (qw * s == tw)
            g = dy[:, qh.clamp(0, oh - 1)][:, :, qw.clamp(0, ow - 1)] * (okh[:, None] & okw[None, :])[None, :, :, None].to(dy.dtype)
            dx += g @ (w4[:, kw, kh, :] if mutant == "swap_taps" else w4[:, kh, kw, :])
    return dx


def dgrad_epilogue(acc, add, mask, mutant=None):
    """mask > 0 ? acc + add : 0 (add / mask None: absent); "add_after_mask": the mutant that adds to the masked value"""
    if mutant == "add_after_mask":
        v = acc if mask is None else torch.where(mask > 0, acc, torch.zeros_like(acc))
        return v if add is None else v + add
    v = acc if add is None else acc + add
    return v if mask is None else torch.where(mask > 0, v, torch.zeros_like(v))


def dgrad_ref(o, c, use_add, use_mask, mutant=None):
    """fp64 dX of a case's operands, after add and mask, before the bf16 store"""
    dy, wt = o["dy"].double(), o["wt"].double()
    acc = dgrad_gather(dy, wt, c, mutant) if mutant in ("no_divisibility", "swap_taps") else dgrad_sum(dy, wt, c)
    return dgrad_epilogue(acc, o["add"].double() if use_add else None, o["mask"].double() if use_mask else None, mutant)


def transpose_pack_ref(wt, taps):
    """wT[c, (tap, o)] = wt[o, (tap, c)]"""
    Cout = wt.shape[0]
    return wt.reshape(Cout, taps, -1).permute(2, 1, 0).reshape(-1, taps * Cout).contiguous()


# ---- transpose pack, BatchNorm unfold, the map gradient's entry ------------------------------------------------------------------------------
PACK_CASES = [(72, 40, 3), (8, 24, 1), (64, 64, 3), (1, 1, 1), (40, 8, 7)]               # (Cout, Cin, k): any dims
UNFOLD_CASES = [(72, 40, 3), (24, 8, 1), (8, 72, 3), (3, 300, 1)]                        # K = 360, 8, 648, 300: around the 256 threads
MAP_CASES = [(2, 8, 3, 5), (3, 72, 1, 1), (2, 72, 3, 3), (1, 24, 7, 37), (5, 8, 1, 1)]   # (B, C, h, w): C = 8, P = 1, odd P


def unfold_operands(Cout, Cin, k, seed=0):
    rs = np.random.RandomState(Cout + 3 * Cin + k + seed)
    f = lambda *s: t32(rs.standard_normal(s))
    return dict(w=f(Cout, Cin, k, k), dwp=f(Cout, k * k * Cin), dbp=f(Cout), gamma=f(Cout), mean=f(Cout),
                var=t32(rs.uniform(0.5, 1.5, Cout)), eps=1e-5)


def unfold_sum(w, dwp, dbp, gamma, mean, var, eps):
    """conv_bn_unfold in the precision of w -> (dW [Cout, Cin, k, k], dgamma, dbeta, magnitude sum of dgamma)"""
    Cout, Cin, k, _ = w.shape
    r = 1.0 / torch.sqrt(var + eps)
    g = dwp.reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)
    prod = w * g
    dg = r * (prod.sum(dim=(1, 2, 3)) - mean * dbp)
    mag = r * (prod.abs().sum(dim=(1, 2, 3)) + (mean * dbp).abs())
    return (gamma * r)[:, None, None, None] * g, dg, dbp.clone(), mag


def map_operands(B, C, h, w, seed=0):
    """(map, dmap) fp32 NCHW: the map is post-ReLU like, with exact zeros, -0.0 and a few negative values"""
    rs = np.random.RandomState(B + 5 * C + 11 * h + w + seed)
    fmap = rs.standard_normal((B, C, h, w)).astype(np.float32)
    kind = rs.randint(0, 4, fmap.shape)
    fmap = np.where(kind == 0, np.float32(0.0), np.where(kind == 1, np.float32(-0.0), fmap)).astype(np.float32)
    return t32(fmap), t32(rs.standard_normal((B, C, h, w)))


def map_grad_ref(fmap, dmap):
    """bf16(map > 0 ? dmap : 0) as NHWC, fp64 values"""
    return bf16_round(torch.where(fmap > 0, dmap, torch.zeros_like(dmap)).permute(0, 2, 3, 1).contiguous())


# ---- stem weight gradient ---------------------------------------------------------------------------------------------------------------
# (B, H, W) -> the claim (ntr, ntc, ntiles, tpw, nwg) of stem_wgrad_split on the output extents
STEM_CASES = {
    "7x7_smallest": (1, 7, 7),
    "oh8_ow32_one_tile": (2, 15, 63),
    "oh8_ow32_even_extents": (1, 16, 64),
    "oh9_ow33_four_tiles": (2, 17, 65),
    "two_tiles_per_workgroup_across_images": (87, 15, 129),          # 3 tiles per image, 261 tiles: workgroup 1 starts in image 0, ends in 1
}
STEM_CLAIMS = {
    "7x7_smallest": (1, 1, 1, 1, 1), "oh8_ow32_one_tile": (1, 1, 2, 1, 2), "oh8_ow32_even_extents": (1, 1, 1, 1, 1),
    "oh9_ow33_four_tiles": (2, 2, 8, 1, 8), "two_tiles_per_workgroup_across_images": (1, 3, 261, 2, 131),
}


def stem_operands(B, H, W, kind, seed=0):
    """(img [B, 3, H, W] fp32, g [B, OH, OW, 64] exact in bf16).  "int": img in -256..256 (exact in bf16), g in -1..1; "gauss": N(0, 1)
    img (the kernel rounds it to bf16), g N(0, 1) rounded to bf16"""
    rs = np.random.RandomState(97 * H + W + B + seed)
    oh, ow = stem_out_hw(H, W)
    if kind == "int":
        return t32(rs.randint(-256, 257, (B, 3, H, W))), t32(rs.randint(-1, 2, (B, oh, ow, 64)))
    return t32(rs.standard_normal((B, 3, H, W))), rbf(t32(rs.standard_normal((B, oh, ow, 64))))


def stem_budget(B, H, W):
    oh, ow = stem_out_hw(H, W)
    return 256 * B * oh * ow


def stem_wgrad_sum(img, g):
    """(dW' [64, 147] with k = (kh, kw, c), db' [64]) in the precision of img (already rounded to bf16), tap by tap"""
    B, _, H, W = img.shape
    oh, ow = stem_out_hw(H, W)
    xp = torch.zeros(B, 3, H + 7, W + 7, dtype=img.dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = img
    dW = torch.zeros(64, 7, 7, 3, dtype=img.dtype)
    for kh in range(7):
        for kw in range(7):
            dW[:, kh, kw, :] = torch.einsum("bchw,bhwo->oc", xp[:, :, kh:kh + 2 * oh:2, kw:kw + 2 * ow:2], g)
    return dW.reshape(64, 147), g.sum(dim=(0, 1, 2))


# ---- max-pool backward --------------------------------------------------------------------------------------------------------------------
POOL_HW = [(8, 16), (9, 17), (16, 32), (17, 33), (1, 40), (40, 1)]
POOL_C = (8, 64, 72, 128)
# (ntr, ntc) per extent; ncb = 1, 1, 2, 2 for the four channel counts
POOL_CLAIMS = {(8, 16): (1, 1), (9, 17): (2, 2), (16, 32): (2, 2), (17, 33): (3, 3), (1, 40): (1, 3), (40, 1): (5, 1)}
POOL_NCB = {8: 1, 64: 1, 72: 2, 128: 2}


def pool_operands(B, H, W, C, tied, kind, seed=0):
    """(x [B, H, W, C], g_y [B, OH, OW, C]) fp32 exact in bf16.  tied: x on the four-value grid -1, 0, 0.5, 1.5 (most windows tie, and 0
    meets the ReLU mask), else Gaussian; g_y "int": -8..8 (a pixel sums at most four), "gauss": N(0, 1)"""
    rs = np.random.RandomState(31 * H + W + 3 * C + B + (7 if tied else 0) + seed)
    x = t32(np.array([-1.0, 0.0, 0.5, 1.5])[rs.randint(0, 4, (B, H, W, C))]) if tied else rbf(t32(rs.standard_normal((B, H, W, C))))
    oh, ow = stem_out_hw(H, W)
    gy = t32(rs.randint(-8, 9, (B, oh, ow, C))) if kind == "int" else rbf(t32(rs.standard_normal((B, oh, ow, C))))
    return x, gy


POOL_MUTANTS = ("last_maximum", "loses_window_below", "loses_window_right")


def pool_bwd_sum(x, gy, relu_mask, mutant=None):
    """g_x [B, H, W, C] in the precision of gy: every window scans its nine positions in row-major order (outside the image: -inf) and
    hands g_y to the position of its FIRST maximum; relu_mask zeroes where x <= 0.  Mutants: "last_maximum" (>= for >),
    "loses_window_below" / "loses_window_right": an odd pixel in the last row / column of an 8 x 16 tile does not see the window that
    the next tile owns."""
    B, H, W, C = x.shape
    oh, ow = stem_out_hw(H, W)
    xp = torch.full((B, H + 3, W + 3, C), float("-inf"), dtype=x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    best = torch.full((B, oh, ow, C), float("-inf"), dtype=x.dtype)
    idx = torch.full((B, oh, ow, C), -1, dtype=torch.long)
    for pos in range(9):
        v = xp[:, pos // 3:pos // 3 + 2 * oh:2, pos % 3:pos % 3 + 2 * ow:2]
        better = (v >= best) & (v > float("-inf")) if mutant == "last_maximum" else v > best
        best = torch.where(better, v, best)
        idx = torch.where(better, torch.full_like(idx, pos), idx)
    gxp = torch.zeros(B, H + 3, W + 3, C, dtype=gy.dtype)
    for pos in range(9):
        take = (idx == pos).to(gy.dtype) * gy
        if mutant == "loses_window_below" and pos // 3 == 0:          # the pixel row 2 oh - 1 is the last of its tile when oh % 4 == 0
            take = take * ((torch.arange(oh) % (PB_ROWS // 2) != 0) | (torch.arange(oh) == 0))[None, :, None, None].to(gy.dtype)
        if mutant == "loses_window_right" and pos % 3 == 0:
            take = take * ((torch.arange(ow) % (PB_COLS // 2) != 0) | (torch.arange(ow) == 0))[None, None, :, None].to(gy.dtype)
        gxp[:, pos // 3:pos // 3 + 2 * oh:2, pos % 3:pos % 3 + 2 * ow:2] += take
    gx = gxp[:, 1:1 + H, 1:1 + W]
    return torch.where(x > 0, gx, torch.zeros_like(gx)) if relu_mask else gx.contiguous()


def pool_window_sum(gy_abs, H, W):
    """sum of |g_y| over the windows each input pixel lies in (the Gaussian gate's slack)"""
    B, oh, ow, C = gy_abs.shape
    gxp = torch.zeros(B, H + 3, W + 3, C, dtype=gy_abs.dtype)
    for pos in range(9):
        gxp[:, pos // 3:pos // 3 + 2 * oh:2, pos % 3:pos % 3 + 2 * ow:2] += gy_abs
    return gxp[:, 1:1 + H, 1:1 + W].contiguous()


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------------------
# name -> (shape of z, kinds).  The integer kind needs an even M (see bn_operands).  BN_CLAIMS: (cgb, gx, dead groups, nslab, slab_len,
# rows of the last slab) of the REDUCTION plan bn_plan(M, C, True).
BN_CASES = {
    "c8_one_group_m2": ((2, 8), ("int", "gauss")),
    "c8_one_group_m64": ((64, 8), ("int", "gauss")),                 # a power of two: the backward's g_z is exact too
    "c24_one_dead_group": ((128, 24), ("int", "gauss")),
    "c72_second_workgroup_one_live_group": ((2, 5, 13, 72), ("int", "gauss")),     # M = 130, P = 65: also the fp32 NCHW map across a 64-pixel tile
    "m2_c64": ((2, 64), ("int", "gauss")),
    "slabs17_last_of_2_rows": ((8194, 64), ("int", "gauss")),
    "odd_last_slab": ((1029, 24), ("gauss",)),                      # slabs of 576 and 453 rows
    "c72_nchw_p20": ((3, 4, 5, 72), ("gauss",)),
}
BN_CLAIMS = {
    "c8_one_group_m2": (1, 1, 0, 1, 256, 2), "c8_one_group_m64": (1, 1, 0, 1, 256, 64), "c24_one_dead_group": (4, 1, 1, 1, 128, 128),
    "c72_second_workgroup_one_live_group": (8, 2, 7, 1, 160, 130), "m2_c64": (8, 1, 0, 1, 32, 2),
    "slabs17_last_of_2_rows": (8, 1, 0, 17, 512, 2), "odd_last_slab": (4, 1, 1, 2, 576, 453), "c72_nchw_p20": (8, 2, 7, 1, 64, 60),
}


def bn_mc(shape):
    C = shape[-1]
    return int(np.prod(shape)) // C, C


def bn_plan_tuple(M, C):
    p = bn_plan(M, C, True)
    return p["cgb"], p["gx"], p["dead"], p["nslab"], p["slab_len"], p["last"]


def bn_operands(shape, kind, seed=0):
    """-> dict of fp32 CPU tensors: z, g, residual [shape] exact in bf16, gamma, beta [C], and for "int" the channels' m [C] and a [C].
    "int": row r of z is m_c + a_c (r even) or m_c - a_c (r odd) with integers m_c in -8..8 and a_c in {1, 2, 4}, M even.  A thread of
    the statistics kernel strides by an even number of rows, so it sees ONE value (mean exact, M2 = 0); thread rows and slabs of even
    length then merge to mean m_c and M2 = n a_c^2 exactly in fp64, and the result is mean = m_c, var = a_c^2 with eps = 0, rstd =
    1 / a_c.  xhat is then +-1: with integer gamma in 1..4, beta, g and residual in -4..4 the apply and the backward's sums are exact
    as well, and so is g_z where M is a power of two.  "gauss": z = N(0, 1) (0.5 + U) + N(0, 1) per channel, as tests/test_bn_train_gpu.py
    draws it, g with a ReLU's zeros."""
    M, C = bn_mc(shape)
    rs = np.random.RandomState(M * 7 + C + seed)
    if kind == "int":
        assert M % 2 == 0
        m, a = rs.randint(-8, 9, C), np.array([1, 2, 4])[rs.randint(0, 3, C)]
        sign = np.where(np.arange(M) % 2 == 0, 1, -1)[:, None]
        z = t32(m[None, :] + sign * a[None, :])
        o = dict(z=z, g=t32(rs.randint(-4, 5, (M, C))), residual=t32(rs.randint(-4, 5, (M, C))), gamma=t32(rs.randint(1, 5, C)),
                 beta=t32(rs.randint(-4, 5, C)), m=t32(m), a=t32(a))
    else:
        z = rbf(t32(rs.standard_normal((M, C)) * (0.5 + rs.uniform(size=C)) + rs.standard_normal(C)))
        g = rbf(t32(rs.standard_normal((M, C)) * (rs.uniform(size=(M, C)) > 0.4)))
        o = dict(z=z, g=g, residual=rbf(t32(rs.standard_normal((M, C)))), gamma=t32(0.5 + rs.uniform(size=C)), beta=t32(rs.standard_normal(C)))
    for n in ("z", "g", "residual"):
        o[n] = o[n].reshape(shape)
    return o


BN_MUTANTS = ("skip_last_group", "skip_last_slab")


def _bn_rows(t, C, mutant):
    t = t.reshape(-1, C)
    if mutant == "skip_last_slab":
        p = bn_plan(t.shape[0], C, True)
        t = t[:(p["nslab"] - 1) * p["slab_len"]]
    return t


def bn_stats_sum(z, mutant=None):
    """(mean, biased variance) over all leading axes in the precision of z.  Mutants: "skip_last_slab" leaves the last slab of
    bn_plan's rows out of the sums (the divisor stays M), "skip_last_group" leaves the last eight channels at zero."""
    C = z.shape[-1]
    M = z.numel() // C
    rows = _bn_rows(z, C, mutant)
    mean = rows.sum(0) / M
    var = ((rows - mean) ** 2).sum(0) / M
    if mutant == "skip_last_group":
        mean, var = mean.clone(), var.clone()
        mean[-8:] = 0
        var[-8:] = 0
    return mean, var


def bn_apply_sum(z, mean, rstd, gamma, beta, residual, relu):
    a = gamma * rstd
    v = a * z + (beta - mean * a)
    if residual is not None:
        v = v + residual
    return v.clamp_min(0) if relu else v


def bn_backward_sum(g, z, mean, rstd, gamma, mutant=None):
    """-> (g_z, dgamma, dbeta) in the precision of g; the mutants as in bn_stats_sum"""
    C = z.shape[-1]
    M = z.numel() // C
    xhat = (z - mean) * rstd
    dbeta, dgamma = _bn_rows(g, C, mutant).sum(0), _bn_rows(g * xhat, C, mutant).sum(0)
    if mutant == "skip_last_group":
        dbeta, dgamma = dbeta.clone(), dgamma.clone()
        dbeta[-8:] = 0
        dgamma[-8:] = 0
    return gamma * rstd * (g - dbeta / M - xhat * dgamma / M), dgamma, dbeta
