"""Edge sweep of the trunk's backward kernels: the bottleneck convolutions' data and weight gradients, the transpose pack, the BatchNorm
unfold and the map gradient's entry (csrc/conv_train.hip), the stem's weight gradient and the max-pool backward (csrc/stem_train.hip),
and training-mode BatchNorm (csrc/bn_train.hip), on the cases of tests/trunk_train_cases.py (which
tests/test_trunk_train_edges_cpu.py checks without a GPU).  Every case is named for the split it pins: the pixel shares of the weight
gradient, the 128-pixel workgroups of the data gradient, the stem's 8 x 32 tiles, the pool's 8 x 16 tiles, BatchNorm's channel groups
and slabs.

Every call goes through the raw entry point into canary-padded outputs that must stay intact, then through the ops wrapper, which must
give the same bits, and a second raw call must repeat them.  Two kinds of operands.  Small integers: every product and partial sum is
exact in fp32, so the result must EQUAL the fp64 reference (cast to fp32, or rounded once to bf16 where the kernel stores bf16) in any
summation order -- no tolerance.  Gaussian values rounded to bf16: under the gates the kernels' own tests derived, unchanged
(tests/test_conv_train_gpu.py, tests/test_stem_kernels_gpu.py, tests/test_bn_train_gpu.py); the error of the same
formula in fp32 on the CPU is printed beside each figure."""
import functools

import pytest
import torch

from mgnns_amd import _lib, ops
from oracle.bf16_path import bf16_round
from tests import helpers as H
from tests import trunk_train_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
CANARY, PAD = -7.0, 64           # output buffers carry PAD canary elements either side (a multiple of 16 bytes in both types)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _canary_out(numel, dtype):
    buf = torch.full((numel + 2 * PAD,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + numel]


def _canaries_intact(buf, what):
    n = buf.numel() - 2 * PAD
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all()), "%s wrote outside its output" % what


def _untouched(buf, what):
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all()), "%s wrote to its output" % what


def _bf(t):
    return None if t is None else t.to(BF16).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _workspace(nbytes):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------
def _geom(c):
    return c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["k"], c["stride"], c["pad"]


def _wgrad_raw(c, x, dy):
    """mgnns_conv_wgrad_bf16_nhwc into canary-padded dW' and db' -> (dW', db') after the canaries were checked"""
    K = C.kdim(c)
    nbytes = _lib.lib().mgnns_conv_wgrad_workspace_bytes(*_geom(c))
    ws = _workspace(nbytes)
    bw, dW = _canary_out(c["Cout"] * K, F32)
    bb, db = _canary_out(c["Cout"], F32)
    _lib.call("mgnns_conv_wgrad_bf16_nhwc", _p(x), _p(dy), *_geom(c), dW.data_ptr(), db.data_ptr(), ws.data_ptr() if nbytes else None, nbytes,
              ops._stream())
    _canaries_intact(bw, "wgrad dW'")
    _canaries_intact(bb, "wgrad db'")
    return dW.view(c["Cout"], K).clone(), db.clone()


@functools.lru_cache(maxsize=None)
def _wgrad_refs(name, kind):
    """operands and fp64 references of a case, computed once: (operands, dW', db', sum |dY X|, sum |dY|)"""
    c = C.WGRAD_CASES[name]
    o = C.conv_operands(c, kind)
    dW, db = C.wgrad_ref(o["x"], o["dy"], c)
    mW, mb = (None, None) if kind == "int" else C.wgrad_ref(o["x"].abs(), o["dy"].abs(), c)
    return o, dW, db, mW, mb


@pytest.mark.parametrize("name", list(C.WGRAD_CASES))
def test_wgrad_equals_fp64_on_integers_and_stays_within_its_gate(name):
    """conv_wgrad_kernel + conv_wgrad_reduce_kernel over WGRAD_CASES: an odd pixel count in one share and in the last of two, three
    shares whose boundaries fall inside an image row (1 x 1, and 3 x 3 with padding taps either side of the boundary), a last share of
    one pixel among sixteen, the want = 1024 / tiles cap at 1 and at 4, 3 x 3 at C_in = 256 and 512 (a channel offset inside the tap) at
    both strides, 3 x 3 without padding, 1 x 1 stride 2 on even and odd extents, one-pixel-high and -wide images, fewer pixels than one
    step.  Integers: dW' and db' equal the fp64 sums.  Gaussian: |dW' - ref| <= 1e-6 sum |dY X|, |db' - ref| <= 1e-6 sum |dY|."""
    c = C.WGRAD_CASES[name]
    nshare, share_len, last = C.WGRAD_CLAIMS[name]
    assert C.wgrad_plan(c) == (nshare, share_len, last)
    nbytes = _lib.lib().mgnns_conv_wgrad_workspace_bytes(*_geom(c))
    assert nbytes == (nshare * (c["Cout"] * C.kdim(c) + c["Cout"]) * 4 if nshare > 1 else 0)
    for kind in ("int", "gauss"):
        o, dW64, db64, mW, mb = _wgrad_refs(name, kind)
        x, dy = _bf(o["x"]), _bf(o["dy"])
        dW, db = _wgrad_raw(c, x, dy)
        via = ops.conv_wgrad_bf16_nhwc(x, dy, c["k"], c["stride"], c["pad"])
        _same(via[0], dW, name + ": ops dW' differs from the raw call")
        _same(via[1], db, name + ": ops db' differs from the raw call")
        again = _wgrad_raw(c, x, dy)
        _same(again[0], dW, name + ": dW' not repeatable")
        _same(again[1], db, name + ": db' not repeatable")
        if kind == "int":
            assert float(dW64.abs().max()) <= C.wgrad_budget(c) < C.EXACT and float(dW64.abs().max()) > 0
            assert torch.equal(dW.cpu(), dW64.float()), "%s: dW' differs from the exact sums in %d entries" % (name, int((dW.cpu() != dW64.float()).sum()))
            assert torch.equal(db.cpu(), db64.float()), name + ": db'"
        else:
            fn = lambda xx, dd: C.wgrad_sum(xx, dd, c)
            cpu = H.fp32_cpu_err(fn, o["x"].double(), o["dy"].double())
            ew, eb = (dW.cpu().double() - dW64).abs(), (db.cpu().double() - db64).abs()
            print("%s (%d shares of %d, last %d): max |dW' - ref| / sum|dY X| %.3e, |db' - ref| / sum|dY| %.3e (gate 1e-6); fp32 on the CPU: %.3e, %.3e absolute"
                  % (name, nshare, share_len, last, float((ew / mW.clamp_min(1e-30)).max()), float((eb / mb.clamp_min(1e-30)).max()), cpu[0], cpu[1]))
            assert bool((ew <= 1e-6 * mW).all()) and bool((eb <= 1e-6 * mb).all()), name


# ---- data gradient and the transpose pack -----------------------------------------------------------------------------------------------
def _dgrad_raw(c, dy, wT, mask, add):
    buf, dx = _canary_out(C.in_m(c) * c["Cin"], BF16)
    _lib.call("mgnns_conv_dgrad_bf16_nhwc", _p(dy), c["B"], c["H"], c["W"], c["Cin"], _p(wT), c["Cout"], c["k"], c["k"], c["stride"], c["pad"],
              _p(mask), _p(add), dx.data_ptr(), ops._stream())
    _canaries_intact(buf, "dgrad")
    return dx.view(c["B"], c["H"], c["W"], c["Cin"]).clone()


def _pack_raw(wt, Cout, Cin, k):
    buf, wT = _canary_out(Cout * Cin * k * k, BF16)
    _lib.call("mgnns_conv_transpose_pack_bf16", wt.data_ptr(), Cout, Cin, k, k, wT.data_ptr(), ops._stream())
    _canaries_intact(buf, "transpose pack")
    return wT.view(Cin, k * k * Cout).clone()


@pytest.mark.parametrize("name", list(C.DGRAD_CASES))
def test_dgrad_equals_fp64_on_integers_and_stays_within_its_gate(name):
    """conv_dgrad_kernel over DGRAD_CASES: M = 128, 129, 127 and 1 input pixels, workgroups that span images, every (k, stride, pad) the
    geometry accepts on odd x even and even x odd extents (stride 2: the last row or column meets fewer taps; 3 x 3 without padding: a
    border pixel meets one), C_out and C_in of 64 and 2048, with and without mask and add.  The mask holds 0, -0.0 and negative values,
    which zero the output exactly.  Integers: bf16(exact value after add and mask), bit for bit.  Gaussian: |got - ref| <= 2^-7 |ref| +
    1e-6 (sum |dY w'| + |add|), exactly 0 under the mask."""
    c = C.DGRAD_CASES[name]
    assert (C.in_m(c), C.ceil_div(C.in_m(c), 128)) == C.DGRAD_CLAIMS[name]
    for kind in ("int", "gauss"):
        o = C.conv_operands(c, kind)
        dy, wt, mask, add = (_bf(o[n]) for n in ("dy", "wt", "mask", "add"))
        wT = _pack_raw(wt, c["Cout"], c["Cin"], c["k"])
        _same(ops.conv_transpose_pack(wt, c["k"]), wT, name + ": ops pack differs from the raw call")
        assert torch.equal(wT.float().cpu(), C.transpose_pack_ref(o["wt"], c["k"] ** 2)), name + ": transpose pack"
        acc = C.dgrad_sum(o["dy"].double(), o["wt"].double(), c)
        mag = None if kind == "int" else C.dgrad_sum(o["dy"].double().abs(), o["wt"].double().abs(), c)
        dead = ~(o["mask"] > 0)
        assert bool(dead.any()) and bool((~dead).any())
        for use_mask in (False, True):
            for use_add in (False, True):
                what = "%s %s mask=%s add=%s" % (name, kind, use_mask, use_add)
                m, a = mask if use_mask else None, add if use_add else None
                got = _dgrad_raw(c, dy, wT, m, a)
                _same(ops.conv_dgrad_bf16_nhwc(dy, wT, (c["H"], c["W"]), c["k"], c["stride"], c["pad"], mask=m, add=a), got, what + ": ops differs from raw")
                _same(_dgrad_raw(c, dy, wT, m, a), got, what + ": not repeatable")
                got = got.float().cpu()
                ref = C.dgrad_epilogue(acc, o["add"].double() if use_add else None, o["mask"].double() if use_mask else None)
                assert float(ref.abs().max()) > 0
                if use_mask:
                    assert bool((got[dead] == 0).all()), what + ": a masked element is not zero"
                if c["stride"] == 2 and c["k"] == 1 and not use_add:         # pixels that no output reads
                    skipped = torch.ones(c["H"], c["W"], dtype=torch.bool)
                    skipped[::2, ::2] = False
                    assert bool((got[:, skipped] == 0).all()) and bool((got[:, ~skipped] != 0).any()), what
                if kind == "int":
                    assert float(acc.abs().max()) + 8 <= C.dgrad_budget(c) < C.EXACT
                    want = bf16_round(ref.float()).float()
                    assert torch.equal(got, want), "%s: %d elements differ" % (what, int((got != want).sum()))
                else:
                    mg = mag + o["add"].double().abs() if use_add else mag
                    if use_mask:
                        mg = mg * (~dead)
                    err = (got.double() - ref).abs()
                    bound = 2.0 ** -7 * ref.abs() + 1e-6 * mg
                    worst, ratio = float((err - bound).max()), float((err / bound.clamp_min(1e-300)).max())
                    fn = lambda d, w, ad, ma: C.dgrad_epilogue(C.dgrad_sum(d, w, c), ad if use_add else None, ma if use_mask else None)
                    cpu = H.fp32_cpu_err(fn, o["dy"].double(), o["wt"].double(), o["add"].double(), o["mask"].double())[0]
                    print("%s: max err %.3e, max err / (2^-7 |ref| + 1e-6 mag) %.3f (gate 1); fp32 on the CPU (unrounded) %.3e" % (what, float(err.max()), ratio, cpu))
                    assert worst <= 0, what


@pytest.mark.parametrize("Cout,Cin,k", C.PACK_CASES)
def test_transpose_pack_of_any_dims(Cout, Cin, k):
    """conv_transpose_pack_kernel takes any dims (72 x 3 x 3 x 40, a single element, a 7 x 7 kernel): wT[c, (tap, o)] = wt[o, (tap, c)]"""
    wt = torch.randn(Cout, k * k * Cin, generator=torch.Generator().manual_seed(Cout + Cin)).to(BF16)
    wT = _pack_raw(wt.to(DEV), Cout, Cin, k)
    assert torch.equal(wT.float().cpu(), C.transpose_pack_ref(wt.float(), k * k))
    _same(ops.conv_transpose_pack(wt.to(DEV), k), wT, "ops pack")


@pytest.mark.parametrize("Cout,Cin,k", C.UNFOLD_CASES)
def test_bn_unfold_with_each_output_left_out(Cout, Cin, k):
    """conv_bn_unfold_kernel at dims off every power of two (K = 360, 8, 648, 300 against its 256 threads), with all three outputs and with
    each of dW / dgamma / dbeta left out (the others bit-equal): dW within 1e-6 |want|, dgamma within 1e-6 of its magnitude sum, dbeta =
    db' bit for bit."""
    o = C.unfold_operands(Cout, Cin, k)
    d = {n: v.to(DEV) for n, v in o.items() if torch.is_tensor(v)}
    names = ("w", "dwp", "dbp", "gamma", "mean", "var")
    want_dW, want_dg, want_db, mag = C.unfold_sum(*(o[n].double() for n in names), o["eps"])
    cpu = H.fp32_cpu_err(lambda *a: C.unfold_sum(*a, o["eps"])[:2], *(o[n].double() for n in names))

    def raw(wants):
        bufs = [_canary_out(n, F32) for n in (Cout * Cin * k * k, Cout, Cout)]
        ptrs = [out.data_ptr() if w else None for (_, out), w in zip(bufs, wants)]
        _lib.call("mgnns_conv_bn_unfold", _p(d["dwp"]), _p(d["dbp"]), _p(d["w"]), _p(d["gamma"]), _p(d["mean"]), _p(d["var"]), float(o["eps"]), Cout,
                  Cin, k, k, *ptrs, ops._stream())
        for (buf, out), w in zip(bufs, wants):
            (_canaries_intact if w else _untouched)(buf, "unfold")
        return [out.clone() if w else None for (_, out), w in zip(bufs, wants)]

    full = raw((True, True, True))
    via = ops.conv_bn_unfold(d["dwp"], d["dbp"], d["w"], (d["gamma"], d["mean"], d["var"], o["eps"]))
    for a, b in zip(via, full):
        _same(a.reshape(-1), b, "ops unfold differs from raw")
    for wants in ((False, True, True), (True, False, True), (True, True, False)):
        part = raw(wants)
        for a, b, w in zip(part, full, wants):
            assert (a is None) == (not w) and (a is None or torch.equal(_bits(a), _bits(b))), wants
    dW, dg, dbeta = (t.cpu().double() for t in full)
    ew = float(((dW.view_as(want_dW) - want_dW).abs() / want_dW.abs().clamp_min(1e-30)).max())
    eg = float(((dg - want_dg).abs() / mag).max())
    print("unfold %dx%dx%d: max |dW - ref| / |ref| %.3e, |dgamma - ref| / magnitude %.3e (gates 1e-6); fp32 on the CPU: %.3e, %.3e absolute" % (Cout, Cin, k, ew, eg, cpu[0], cpu[1]))
    assert ew <= 1e-6 and eg <= 1e-6 and torch.equal(dbeta, want_db)


@pytest.mark.parametrize("case", C.MAP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_map_gradient_entry_bit_for_bit(case):
    """map_grad_relu_kernel at C = 8, at C = 72 with one pixel and with an odd pixel count, on a map that holds exact zeros, -0.0 and
    negative values: bf16(map > 0 ? dmap : 0) as NHWC, bit for bit."""
    B, Cc, h, w = case
    fmap, dmap = C.map_operands(*case)
    fd, dd = fmap.to(DEV), dmap.to(DEV)
    buf, g = _canary_out(B * h * w * Cc, BF16)
    _lib.call("mgnns_map_grad_relu_nhwc_bf16", fd.data_ptr(), dd.data_ptr(), B, Cc, h * w, g.data_ptr(), ops._stream())
    _canaries_intact(buf, "map gradient")
    got = g.view(B, h, w, Cc).clone()
    _same(ops.map_grad_relu_nhwc(fd, dd), got, "ops map gradient")
    assert torch.equal(got.float().cpu().double(), C.map_grad_ref(fmap, dmap)) and bool((got != 0).any())
    assert bool((got.cpu()[(fmap <= 0).permute(0, 2, 3, 1)] == 0).all())


# ---- stem weight gradient ---------------------------------------------------------------------------------------------------------------
def _stem_raw(img, g, B, Hh, Ww):
    nbytes = _lib.lib().mgnns_stem_wgrad_workspace_bytes(B, Hh, Ww)
    ws = _workspace(nbytes)
    bw, dW = _canary_out(64 * 147, F32)
    bb, db = _canary_out(64, F32)
    _lib.call("mgnns_stem_wgrad", _p(img), _p(g), B, Hh, Ww, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
    _canaries_intact(bw, "stem dW'")
    _canaries_intact(bb, "stem db'")
    return dW.view(64, 147).clone(), db.clone()


@pytest.mark.parametrize("name", list(C.STEM_CASES))
def test_stem_wgrad_equals_fp64_on_integers_and_stays_within_its_gate(name):
    """stem_wgrad_kernel + stem_wgrad_reduce_kernel: the smallest image, output extents of exactly one 8 x 32 tile (from odd and from even
    image extents) and one past it both ways (four tiles, the second tile row with one live row, the second tile column with one live
    pixel), and 261 tiles on 131 workgroups of two tiles each whose runs cross image boundaries.  Integers (|img| <= 256, g in -1..1):
    dW' and db' equal the fp64 sums.  Gaussian: |dW' - ref| <= 1e-6 sum |g x|, |db' - ref| <= 1e-6 sum |g|, x = bf16(img)."""
    B, Hh, Ww = C.STEM_CASES[name]
    split = C.stem_wgrad_split(B, *C.stem_out_hw(Hh, Ww))
    assert split == C.STEM_CLAIMS[name] and _lib.lib().mgnns_stem_wgrad_workspace_bytes(B, Hh, Ww) == split[4] * 64 * 160 * 4
    for kind in ("int", "gauss"):
        img, g = C.stem_operands(B, Hh, Ww, kind)
        x64 = C.rbf(img).double()
        dW64, db64 = C.stem_wgrad_sum(x64, g.double())
        imgd, gd = img.to(DEV), _bf(g)
        dW, db = _stem_raw(imgd, gd, B, Hh, Ww)
        via = ops.stem_wgrad(imgd, gd)
        _same(via[0], dW, name + ": ops dW' differs from raw")
        _same(via[1], db, name + ": ops db' differs from raw")
        again = _stem_raw(imgd, gd, B, Hh, Ww)
        _same(again[0], dW, name + ": not repeatable")
        _same(again[1], db, name + ": not repeatable")
        if kind == "int":
            assert 0 < float(dW64.abs().max()) <= C.stem_budget(B, Hh, Ww) < C.EXACT
            assert torch.equal(dW.cpu(), dW64.float()), "%s: dW' differs in %d entries" % (name, int((dW.cpu() != dW64.float()).sum()))
            assert torch.equal(db.cpu(), db64.float()), name + ": db'"
        else:
            mW, mb = C.stem_wgrad_sum(x64.abs(), g.double().abs())
            cpu = H.fp32_cpu_err(C.stem_wgrad_sum, x64, g.double())
            ew, eb = (dW.cpu().double() - dW64).abs(), (db.cpu().double() - db64).abs()
            print("stem %s (tiles %s): max |dW' - ref| / sum|g x| %.3e, |db' - ref| / sum|g| %.3e (gate 1e-6); fp32 on the CPU: %.3e, %.3e absolute"
                  % (name, split, float((ew / mW.clamp_min(1e-30)).max()), float((eb / mb.clamp_min(1e-30)).max()), cpu[0], cpu[1]))
            assert bool((ew <= 1e-6 * mW).all()) and bool((eb <= 1e-6 * mb).all()), name


# ---- max-pool backward ------------------------------------------------------------------------------------------------------------------
def _pool_raw(x, gy, relu_mask):
    B, Hh, Ww, Cc = x.shape
    buf, gx = _canary_out(x.numel(), BF16)
    _lib.call("mgnns_maxpool3x3s2_nhwc_bwd", _p(x), _p(gy), B, Hh, Ww, Cc, int(relu_mask), gx.data_ptr(), ops._stream())
    _canaries_intact(buf, "pool backward")
    return gx.view(B, Hh, Ww, Cc).clone()


@pytest.mark.parametrize("hw", C.POOL_HW, ids=lambda s: "%dx%d" % s)
def test_pool_backward_equals_fp64_on_integers_and_stays_within_its_gate(hw):
    """maxpool3x3s2_bwd_kernel on images of exactly one 8 x 16 tile, one past it both ways (the odd pixels in a tile's last row and column
    take their gradient from a window the next tile owns), two and three tiles each way, one pixel high and one pixel wide, at C = 8,
    64, 72 and 128 (one and two channel blocks, the second with one live group), tied and distinct inputs, with and without the ReLU
    mask.  Integer g_y: bf16(the fp64 sum) bit for bit -- a pixel adds at most four values.  Gaussian g_y: |got - ref| <= 2^-8 |ref| +
    1e-6 sum |g_y of the pixel's windows|, exactly 0 where the reference is 0."""
    Hh, Ww = hw
    for Cc in C.POOL_C:
        assert C.pool_bwd_tiles(2, Hh, Ww, Cc)[:3] == C.POOL_CLAIMS[hw] + (C.POOL_NCB[Cc],)
        for tied in (True, False):
            for kind in ("int", "gauss"):
                x, gy = C.pool_operands(2, Hh, Ww, Cc, tied, kind)
                xd, gd = _bf(x), _bf(gy)
                wsum = C.pool_window_sum(gy.double().abs(), Hh, Ww)
                for relu_mask in (False, True):
                    what = "pool %dx%dx%d tied=%s %s relu_mask=%s" % (Hh, Ww, Cc, tied, kind, relu_mask)
                    got = _pool_raw(xd, gd, relu_mask)
                    _same(ops.maxpool3x3s2_bwd_nhwc(xd, gd, relu_mask=relu_mask), got, what + ": ops differs from raw")
                    _same(_pool_raw(xd, gd, relu_mask), got, what + ": not repeatable")
                    got = got.float().cpu().double()
                    ref = C.pool_bwd_sum(x.double(), gy.double(), relu_mask)
                    assert bool((got[ref == 0] == 0).all()), what
                    if relu_mask:
                        assert bool((got[x <= 0] == 0).all()), what
                    if kind == "int":
                        assert torch.equal(got, bf16_round(ref.float())), "%s: %d elements differ" % (what, int((got != bf16_round(ref.float())).sum()))
                    else:
                        err = (got - ref).abs()
                        bound = 2.0 ** -8 * ref.abs() + 1e-6 * wsum
                        worst, ratio = float((err - bound).max()), float((err / bound.clamp_min(1e-300)).max())
                        if Cc == 72:
                            cpu = H.fp32_cpu_err(lambda a, b: C.pool_bwd_sum(a, b, relu_mask), x.double(), gy.double())[0]
                            print("%s: max err %.3e, max err / (2^-8 |ref| + 1e-6 window sum) %.3f (gate 1); fp32 on the CPU (unrounded) %.3e" % (what, float(err.max()), ratio, cpu))
                        assert worst <= 0, what


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
def _bn_stats_raw(z, M, Cc, eps):
    nbytes = _lib.lib().mgnns_bn_stats_workspace_bytes(M, Cc)
    ws = _workspace(nbytes)
    bufs = [_canary_out(Cc, F32) for _ in range(3)]
    _lib.call("mgnns_bn_stats_bf16", _p(z), M, Cc, float(eps), 0.1, *(o.data_ptr() for _, o in bufs), None, None, ws.data_ptr(), nbytes, ops._stream())
    for b, _ in bufs:
        _canaries_intact(b, "bn statistics")
    return [o.clone() for _, o in bufs]


def _bn_apply_raw(z, M, Cc, mean, rstd, gamma, beta, residual, relu, P):
    buf, y = _canary_out(M * Cc, F32 if P else BF16)
    _lib.call("mgnns_bn_apply_bf16", _p(z), M, Cc, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), int(relu), 1 if P else 0, P, y.data_ptr(),
              ops._stream())
    _canaries_intact(buf, "bn apply")
    return y.clone()


def _bn_backward_raw(g, z, M, Cc, mean, rstd, gamma):
    nbytes = _lib.lib().mgnns_bn_backward_workspace_bytes(M, Cc)
    ws = _workspace(nbytes)
    bz, gz = _canary_out(M * Cc, BF16)
    bufs = [_canary_out(Cc, F32) for _ in range(2)]
    _lib.call("mgnns_bn_backward_bf16", _p(g), _p(z), M, Cc, _p(mean), _p(rstd), _p(gamma), gz.data_ptr(), *(o.data_ptr() for _, o in bufs),
              ws.data_ptr(), nbytes, ops._stream())
    for b in [bz] + [b for b, _ in bufs]:
        _canaries_intact(b, "bn backward")
    return gz.clone(), bufs[0][1].clone(), bufs[1][1].clone()


@pytest.mark.parametrize("name", list(C.BN_CASES))
def test_batchnorm_equals_fp64_on_integers_and_stays_within_its_gates(name):
    """bn_stats / bn_apply / bn_backward over BN_CASES: C = 8 (one channel group per workgroup), 24 (a dead group), 72 (a second workgroup
    with one live group), M = 2, 17 slabs with a last slab of 2 rows (most thread rows empty, the finaliser walks more than 8 slabs), an
    odd last slab, the fp32 NCHW map at C = 72 with P = 20 and P = 65, residual and ReLU on and off.

    Integers (rows alternate between m_c + a_c and m_c - a_c, eps = 0; tests/trunk_train_cases.py: bn_operands): mean = m_c and var =
    a_c^2 EXACTLY -- derived from the kernel's (mean, M2) merge in fp64, and the kernel does come out exact, so the argument and the
    kernel agree.  From the exact statistics the apply is exact (bf16 and fp32 NCHW), dbeta and dgamma equal the integer sums, and g_z is
    bf16(exact) where M is a power of two (1 / M is exact then); at other M it is held to the Gaussian gate.
    Gaussian: the gates of tests/test_bn_train_gpu.py -- mean within 1e-5 max(|mean|, std), rstd within 1e-5 relative, outputs within
    2^-8 |ref| + 1e-5 of the magnitudes added, sums within 1e-6 of the sum of magnitudes -- from the kernel's own statistics."""
    shape, kinds = C.BN_CASES[name]
    M, Cc = C.bn_mc(shape)
    assert C.bn_plan_tuple(M, Cc) == C.BN_CLAIMS[name]
    P = shape[1] * shape[2] if len(shape) == 4 else 0
    for kind in kinds:
        o = C.bn_operands(shape, kind)
        eps = 0.0 if kind == "int" else 1e-5
        z, g, res = (_bf(o[n]) for n in ("z", "g", "residual"))
        gamma, beta = o["gamma"].to(DEV), o["beta"].to(DEV)
        z64, g64, r64 = (o[n].double().reshape(M, Cc) for n in ("z", "g", "residual"))
        what = "bn %s %s" % (name, kind)
        # statistics
        mean, rstd, var = _bn_stats_raw(z, M, Cc, eps)
        via = ops.bn_stats_bf16_nhwc(z, eps, want_var=True)
        for a, b in zip(via, (mean, rstd, var)):
            _same(a, b, what + ": ops statistics differ from raw")
        for a, b in zip(_bn_stats_raw(z, M, Cc, eps), (mean, rstd, var)):
            _same(a, b, what + ": statistics not repeatable")
        mean64, var64 = C.bn_stats_sum(z64)
        if kind == "int":
            assert torch.equal(mean.cpu(), o["m"]) and torch.equal(var.cpu(), o["a"] ** 2), what + ": statistics are not exact"
            exact_rstd = torch.equal(rstd.cpu(), 1.0 / o["a"])
            print("%s: mean and var exact; rstd == 1 / a exactly: %s" % (what, exact_rstd))
            assert float((rstd.cpu().double() * o["a"].double() - 1).abs().max()) <= 1e-5
            mean, rstd = o["m"].to(DEV), (1.0 / o["a"]).to(DEV)               # what follows starts from the exact statistics
        else:
            tol = 1e-5 * torch.maximum(mean64.abs(), var64.sqrt())
            err = (mean.cpu().double() - mean64).abs()
            rel = (rstd.cpu().double() * torch.sqrt(var64 + eps) - 1).abs()
            cpu = H.fp32_cpu_err(C.bn_stats_sum, z64)
            print("%s: mean err / (1e-5 max(|mean|, std)) max %.3g, rstd rel max %.3g (gate 1e-5); fp32 on the CPU: mean %.3e, var %.3e absolute"
                  % (what, float((err / tol.clamp_min(1e-300)).max()), float(rel.max()), cpu[0], cpu[1]))
            assert bool((err <= tol).all()) and bool((rel <= 1e-5).all()), what
            assert torch.allclose(rstd, 1.0 / torch.sqrt(var + eps), rtol=5e-7, atol=0)
        mu, rs, ga, be = (t.cpu().double() for t in (mean, rstd, gamma, beta))
        # apply
        for residual in (None, res):
            for relu in (True, False):
                for nchw in ((False, True) if P else (False,)):
                    y = _bn_apply_raw(z, M, Cc, mean, rstd, gamma, beta, residual, relu, P if nchw else 0)
                    y = y.view(shape[0], Cc, shape[1], shape[2]) if nchw else y.view(shape)
                    _same(ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta, residual=residual, relu=relu, out_nchw_f32=nchw), y, what + ": ops apply differs from raw")
                    got = y.cpu().double()
                    got = got.permute(0, 2, 3, 1).reshape(M, Cc) if nchw else got.reshape(M, Cc)
                    r = None if residual is None else r64
                    ref = C.bn_apply_sum(z64, mu, rs, ga, be, r, False)
                    want = ref.clamp_min(0) if relu else ref
                    if kind == "int":
                        assert torch.equal(got, want), "%s apply residual=%s relu=%s nchw=%s" % (what, residual is not None, relu, nchw)
                    else:
                        a = ga * rs
                        slack = 1e-5 * ((a * z64).abs() + (be - mu * a).abs() + (0 if r is None else r.abs()))
                        tol = slack + (0 if nchw else 2.0 ** -8 * want.abs())
                        assert bool(((got - want).abs() <= tol).all()), "%s apply residual=%s relu=%s nchw=%s" % (what, residual is not None, relu, nchw)
                        if relu:
                            assert bool((got[ref < -slack] == 0).all()) and bool((got >= 0).all())
        # backward
        gz, dgamma, dbeta = _bn_backward_raw(g, z, M, Cc, mean, rstd, gamma)
        gz = gz.view(shape)
        via = ops.bn_backward_bf16_nhwc(g, z, mean, rstd, gamma)
        for a, b in zip(via, (gz, dgamma, dbeta)):
            _same(a, b, what + ": ops backward differs from raw")
        for a, b in zip(_bn_backward_raw(g, z, M, Cc, mean, rstd, gamma), (gz.reshape(-1), dgamma, dbeta)):
            _same(a, b, what + ": backward not repeatable")
        gz64, dg64, db64 = C.bn_backward_sum(g64, z64, mu, rs, ga)
        xhat = (z64 - mu) * rs
        got = gz.cpu().double().reshape(M, Cc)
        tol = 2.0 ** -8 * gz64.abs() + 1e-5 * (ga * rs).abs() * (g64.abs() + db64.abs() / M + (xhat * dg64).abs() / M)
        if kind == "int":
            assert torch.equal(dbeta.cpu().double(), db64) and torch.equal(dgamma.cpu().double(), dg64), what + ": the backward's sums are not exact"
            if M & (M - 1) == 0:
                assert torch.equal(got, bf16_round(gz64.float())), what + ": g_z"
        else:
            eb = float(((dbeta.cpu().double() - db64).abs() / g64.abs().sum(0).clamp_min(1e-30)).max())
            eg = float(((dgamma.cpu().double() - dg64).abs() / (g64 * xhat).abs().sum(0).clamp_min(1e-30)).max())
            cpu = H.fp32_cpu_err(lambda a, b: C.bn_backward_sum(a, b, mu.to(a.dtype), rs.to(a.dtype), ga.to(a.dtype)), g64, z64)
            print("%s: |dbeta - ref| / sum|g| %.3e, |dgamma - ref| / sum|g xhat| %.3e (gate 1e-6), max (|g_z - ref| - tol) %.3e (gate 0); fp32 on the CPU: g_z %.3e, dgamma %.3e, dbeta %.3e absolute"
                  % (what, eb, eg, float(((got - gz64).abs() - tol).max()), cpu[0], cpu[1], cpu[2]))
            assert eb <= 1e-6 and eg <= 1e-6, what
        assert bool(((got - gz64).abs() <= tol).all()), what + ": g_z"


# ---- empty batches ----------------------------------------------------------------------------------------------------------------------
def test_empty_batches_write_nothing_or_zero_the_weight_gradients():
    """B == 0 at every entry point that has a batch: the data gradient, the pool backward and the map gradient write nothing; the two
    weight gradients zero dW' and db' (and nothing beyond them)."""
    big = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    f = torch.zeros(1 << 12, device=DEV)
    buf, out = _canary_out(1 << 12, BF16)
    _lib.call("mgnns_conv_dgrad_bf16_nhwc", big.data_ptr(), 0, 6, 5, 64, big.data_ptr(), 64, 3, 3, 1, 1, None, None, out.data_ptr(), ops._stream())
    _lib.call("mgnns_maxpool3x3s2_nhwc_bwd", big.data_ptr(), big.data_ptr(), 0, 9, 8, 72, 1, out.data_ptr(), ops._stream())
    _lib.call("mgnns_map_grad_relu_nhwc_bf16", f.data_ptr(), f.data_ptr(), 0, 72, 6, out.data_ptr(), ops._stream())
    _untouched(buf, "an empty batch")
    bw, dW = _canary_out(64 * 576, F32)
    bb, db = _canary_out(64, F32)
    _lib.call("mgnns_conv_wgrad_bf16_nhwc", None, None, 0, 6, 5, 64, 64, 3, 3, 1, 1, dW.data_ptr(), db.data_ptr(), None, 0, ops._stream())
    _canaries_intact(bw, "wgrad of an empty batch")
    _canaries_intact(bb, "wgrad of an empty batch")
    assert not dW.any() and not db.any()
    bw, dW = _canary_out(64 * 147, F32)
    bb, db = _canary_out(64, F32)
    _lib.call("mgnns_stem_wgrad", None, None, 0, 9, 17, dW.data_ptr(), db.data_ptr(), None, 0, ops._stream())
    _canaries_intact(bw, "stem wgrad of an empty batch")
    _canaries_intact(bb, "stem wgrad of an empty batch")
    assert not dW.any() and not db.any()
    e = torch.zeros(0, 6, 5, 64, dtype=BF16, device=DEV)
    assert tuple(ops.conv_dgrad_bf16_nhwc(e, big[:64 * 576].view(64, 576), (6, 5), 3, 1, 1).shape) == (0, 6, 5, 64)
    dW, db = ops.conv_wgrad_bf16_nhwc(e, e, 3, 1, 1)
    assert tuple(dW.shape) == (64, 576) and not dW.any() and not db.any()
    dW, db = ops.stem_wgrad(torch.zeros(0, 3, 9, 17, device=DEV), torch.zeros(0, 5, 9, 64, dtype=BF16, device=DEV))
    assert tuple(dW.shape) == (64, 147) and not dW.any() and not db.any()
    assert tuple(ops.maxpool3x3s2_bwd_nhwc(torch.zeros(0, 9, 8, 72, dtype=BF16, device=DEV), torch.zeros(0, 5, 4, 72, dtype=BF16, device=DEV)).shape) == (0, 9, 8, 72)
    assert tuple(ops.map_grad_relu_nhwc(torch.zeros(0, 72, 2, 3, device=DEV), torch.zeros(0, 72, 2, 3, device=DEV)).shape) == (0, 2, 3, 72)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
# what, the message, the geometry (defaults: B = 1, 4 x 4, 64 -> 64, 1 x 1, stride 1, pad 0), byte offset of the first operand
CONV_REFUSALS = [
    ("C_in 32", r"powers of two >= 64 \(got C_in=32 ", dict(Cin=32)),
    ("C_in 96", r"powers of two >= 64 \(got C_in=96 ", dict(Cin=96)),
    ("C_out 96", r"powers of two >= 64 \(got C_in=64 C_out=96", dict(Cout=96)),
    ("5 x 5", r"1x1 or 3x3 \(got 5x5", dict(KH=5, KW=5, pad=2, H=8, W=8)),
    ("1 x 3", r"1x1 or 3x3 \(got 1x3", dict(KH=1, KW=3)),
    ("stride 3", r"bad stride 3 / padding 0", dict(stride=3)),
    ("pad 2 at 3 x 3", r"bad stride 1 / padding 2", dict(KH=3, KW=3, pad=2)),
    ("pad 1 at 1 x 1", r"bad stride 1 / padding 1", dict(pad=1)),
    ("empty output", r"empty output \(H=1 W=4 k=3 stride=1 pad=0\)", dict(KH=3, KW=3, H=1)),
    ("empty output at stride 2", r"empty output \(H=2 W=4 k=3 stride=2 pad=0\)", dict(KH=3, KW=3, H=2, stride=2)),   # (2 - 3) / 2 + 1 truncates to 1
    ("operand offset by 8 bytes", r"16-byte aligned \(B=1 H=4 W=4 C_in=64 C_out=64\)", dict(off=8)),
]


@pytest.mark.parametrize("what,match,kw", CONV_REFUSALS, ids=[r[0].replace(" ", "_") for r in CONV_REFUSALS])
def test_conv_refusals_leave_the_outputs_alone(what, match, kw):
    """At each limit plus one both gradients raise and write nothing (every operand is large enough for the call, were it not refused)"""
    big = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    g = dict(dict(B=1, H=4, W=4, Cin=64, Cout=64, KH=1, KW=1, stride=1, pad=0, off=0), **kw)
    geom = (g["B"], g["H"], g["W"], g["Cin"], g["Cout"], g["KH"], g["KW"], g["stride"], g["pad"])
    first = big.data_ptr() + g["off"]
    buf, dx = _canary_out(1 << 12, BF16)
    with pytest.raises(RuntimeError, match="mgnns_conv_dgrad_bf16_nhwc: .*" + match):
        _lib.call("mgnns_conv_dgrad_bf16_nhwc", first, g["B"], g["H"], g["W"], g["Cin"], big.data_ptr(), g["Cout"], g["KH"], g["KW"], g["stride"],
                  g["pad"], None, None, dx.data_ptr(), ops._stream())
    _untouched(buf, what)
    bw, dW = _canary_out(1 << 14, F32)
    ws = _workspace(1 << 20)
    with pytest.raises(RuntimeError, match="mgnns_conv_wgrad_bf16_nhwc: .*" + match):
        _lib.call("mgnns_conv_wgrad_bf16_nhwc", first, big.data_ptr(), *geom, dW.data_ptr(), dW.data_ptr() + 4096 * 4, ws.data_ptr(), ws.numel(), ops._stream())
    _untouched(bw, what)
    assert _lib.lib().mgnns_conv_wgrad_workspace_bytes(*geom) == 0


def test_a_workspace_one_byte_short_is_refused():
    big = torch.zeros(1 << 20, dtype=BF16, device=DEV)
    f = torch.zeros(1 << 16, device=DEV)
    L = _lib.lib()
    ws = _workspace(1 << 22)
    buf, out = _canary_out(1 << 16, F32)
    need = L.mgnns_conv_wgrad_workspace_bytes(1, 27, 19, 64, 64, 1, 1, 1, 0)
    assert need == 2 * (64 * 64 + 64) * 4
    with pytest.raises(RuntimeError, match=r"workspace of %d bytes, %d needed" % (need - 1, need)):
        _lib.call("mgnns_conv_wgrad_bf16_nhwc", big.data_ptr(), big.data_ptr(), 1, 27, 19, 64, 64, 1, 1, 1, 0, out.data_ptr(), out.data_ptr() + 4096 * 4,
                  ws.data_ptr(), need - 1, ops._stream())
    with pytest.raises(RuntimeError, match=r"workspace of 0 bytes, %d needed" % need):
        _lib.call("mgnns_conv_wgrad_bf16_nhwc", big.data_ptr(), big.data_ptr(), 1, 27, 19, 64, 64, 1, 1, 1, 0, out.data_ptr(), out.data_ptr() + 4096 * 4,
                  None, 0, ops._stream())
    need = L.mgnns_stem_wgrad_workspace_bytes(2, 17, 65)
    with pytest.raises(RuntimeError, match=r"workspace of %d bytes, %d needed" % (need - 1, need)):
        _lib.call("mgnns_stem_wgrad", f.data_ptr(), big.data_ptr(), 2, 17, 65, out.data_ptr(), out.data_ptr() + 64 * 147 * 4, ws.data_ptr(), need - 1, ops._stream())
    need = L.mgnns_bn_stats_workspace_bytes(8194, 64)
    with pytest.raises(RuntimeError, match=r"workspace of %d bytes, %d needed" % (need - 1, need)):
        _lib.call("mgnns_bn_stats_bf16", big.data_ptr(), 8194, 64, 1e-5, 0.1, out.data_ptr(), out.data_ptr() + 256, None, None, None, ws.data_ptr(), need - 1,
                  ops._stream())
    need = L.mgnns_bn_backward_workspace_bytes(8194, 64)
    with pytest.raises(RuntimeError, match=r"workspace of %d bytes, %d needed" % (need - 1, need)):
        _lib.call("mgnns_bn_backward_bf16", big.data_ptr(), big.data_ptr(), 8194, 64, f.data_ptr(), f.data_ptr(), f.data_ptr(), out.data_ptr(), None, None,
                  ws.data_ptr(), need - 1, ops._stream())
    _untouched(buf, "a short workspace")


def test_batchnorm_pool_and_stem_refusals_leave_the_outputs_alone():
    big = torch.zeros(1 << 14, dtype=BF16, device=DEV)
    f = torch.zeros(1 << 12, device=DEV)
    ws = _workspace(1 << 16)
    buf, out = _canary_out(1 << 12, F32)
    o = out.data_ptr()
    for M, Cc, match in ((1, 16, r"at least two values per channel \(got M=1 C=16\)"), (4, 12, r"multiple of 8 \(got M=4 C=12\)")):
        with pytest.raises(RuntimeError, match="mgnns_bn_stats_bf16: .*" + match):
            _lib.call("mgnns_bn_stats_bf16", big.data_ptr(), M, Cc, 1e-5, 0.1, o, o + 256, None, None, None, ws.data_ptr(), ws.numel(), ops._stream())
        with pytest.raises(RuntimeError, match="mgnns_bn_apply_bf16: .*" + match):
            _lib.call("mgnns_bn_apply_bf16", big.data_ptr(), M, Cc, f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), None, 1, 0, 0, o, ops._stream())
        with pytest.raises(RuntimeError, match="mgnns_bn_backward_bf16: .*" + match):
            _lib.call("mgnns_bn_backward_bf16", big.data_ptr(), big.data_ptr(), M, Cc, f.data_ptr(), f.data_ptr(), f.data_ptr(), o, o + 4096, o + 8192,
                      ws.data_ptr(), ws.numel(), ops._stream())
        assert _lib.lib().mgnns_bn_stats_workspace_bytes(M, Cc) == 0 and _lib.lib().mgnns_bn_backward_workspace_bytes(M, Cc) == 0
    with pytest.raises(RuntimeError, match=r"16-byte aligned \(M=4 C=16\)"):
        _lib.call("mgnns_bn_stats_bf16", big.data_ptr() + 8, 4, 16, 1e-5, 0.1, o, o + 256, None, None, None, ws.data_ptr(), ws.numel(), ops._stream())
    with pytest.raises(RuntimeError, match=r"need C % 8 == 0 \(B=1 H=4 W=4 C=12\)"):
        _lib.call("mgnns_maxpool3x3s2_nhwc_bwd", big.data_ptr(), big.data_ptr(), 1, 4, 4, 12, 0, o, ops._stream())
    with pytest.raises(RuntimeError, match=r"16-byte aligned"):
        _lib.call("mgnns_maxpool3x3s2_nhwc_bwd", big.data_ptr() + 8, big.data_ptr(), 1, 4, 4, 16, 0, o, ops._stream())
    with pytest.raises(RuntimeError, match=r"need C % 8 == 0 \(B=1 C=12 P=4\)"):
        _lib.call("mgnns_map_grad_relu_nhwc_bf16", f.data_ptr(), f.data_ptr(), 1, 12, 4, o, ops._stream())
    with pytest.raises(RuntimeError, match=r"mgnns_stem_wgrad: bad dims B=1 H=6 W=8"):
        _lib.call("mgnns_stem_wgrad", f.data_ptr(), big.data_ptr(), 1, 6, 8, o, o + 64 * 147 * 4, ws.data_ptr(), ws.numel(), ops._stream())
    with pytest.raises(RuntimeError, match=r"16-byte aligned \(B=1 H=8 W=8\)"):
        _lib.call("mgnns_stem_wgrad", f.data_ptr(), big.data_ptr() + 8, 1, 8, 8, o, o + 64 * 147 * 4, ws.data_ptr(), ws.numel(), ops._stream())
    assert _lib.lib().mgnns_stem_wgrad_workspace_bytes(1, 6, 8) == 0
    _untouched(buf, "a refused call")
    # the wrappers refuse the same shapes before anything is launched
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.bn_stats_bf16_nhwc(big[:48].view(4, 12), 1e-5)
    with pytest.raises(ValueError, match="two values"):
        ops.bn_stats_bf16_nhwc(big[:16].view(1, 16), 1e-5)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.maxpool3x3s2_bwd_nhwc(big[:192].view(1, 4, 4, 12), big[:48].view(1, 2, 2, 12))
    with pytest.raises(ValueError, match="H, W >= 7"):
        ops.stem_wgrad(f[:144].view(1, 3, 6, 8), big[:768].view(1, 3, 4, 64))
