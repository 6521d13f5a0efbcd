"""Edge sweep of the matrix-pipe forward kernels: the dense bf16 GEMM (csrc/gemm_bf16.hip: four tile kernels, two fix-up kernels, the
transpose-cast) and the trunk forward (csrc/conv_bf16.hip: implicit-GEMM convolution, stem, max-pool, BatchNorm fold), on the cases of
tests/matrix_pipe_cases.py (which tests/test_matrix_pipe_edges_cpu.py checks without a GPU).

Two passes.  Small-integer operands: every value is exact in bf16 and every partial sum in fp32, so the kernels must equal the fp64
reference BIT FOR BIT, whatever their summation order -- no tolerance.  Gaussian operands rounded to bf16: against fp64 under the
project's store bounds (bf16 outputs: helpers.within_bf16_store, 2^-8 |want| + 1e-5 max |want|; fp32 outputs: 2^-23 |want| + 1e-5
max |want|); the error of the same formula in fp32 on the CPU is printed beside each figure."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import _lib, ops, synth, trunk
from oracle import trunk_cpu
from oracle.bf16_path import bf16_bits, bf16_round
from tests import helpers as H
from tests import matrix_pipe_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
CANARY, PAD = -7.0, 64           # output buffers carry PAD canary elements either side (a multiple of 16 bytes in both types)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


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


def _path_claim(name):
    """the launcher branch a case is named for, asserted through the restatement where the device has the 256 CUs it was worked out for"""
    if _cus() != 256:
        print("%s: %d CUs, not 256 -- the path claim is not checked here" % (name, _cus()))
        return False
    C.GEMM_CLAIMS[name](C.case_plan(name))
    return True


# ---- dense bf16 GEMM ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.GEMM_CASES))
def test_gemm_integer_operands_equal_fp64_bit_for_bit(name):
    """Every kernel and launcher branch of GEMM_CASES (256 x 128 with the row and the column-split map and its K split + fix-up launch,
    256 x 256 with and without left-over parts, 160 x 256 and 320 x 256 with one and two tiles per workgroup, the transposed store, the
    small no-split products) on integer operands: fp32 and bf16 output x bias or none x the three activations equal the fp64 product
    (torch on the device for the full matrix, the CPU for 64 rows either side of every row-tile boundary) bit for bit; `out=` as a
    column slice of a wider matrix leaves the columns beyond N and the rows before and after bit-unchanged; two calls give equal bits."""
    M, N, K, form, c_tr = C.GEMM_CASES[name]
    _path_claim(name)
    a, bt, bias = C.gemm_operands(name, "int", DEV)
    prod = C.gemm_product(a, bt)
    rows = C.checked_rows(M, C.case_plan(name)["kernel"])
    rows_dev = rows.to(DEV)
    prod_cpu = C.gemm_product(a[rows_dev].cpu(), bt.cpu())
    assert float(prod_cpu.abs().max()) + 8 < C.EXACT
    bias_cpu = bias.cpu()
    ops.gemm_bf16_set_form(form)
    try:
        for dt in (F32, BF16):
            for b, b_cpu in ((None, None), (bias, bias_cpu)):
                for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU2):
                    got = ops.gemm_bf16_nt(a, bt, b, act, out_dtype=dt, transposed_out=c_tr)
                    assert got.dtype == dt and tuple(got.shape) == ((N, M) if c_tr else (M, N))
                    g = got.t() if c_tr else got
                    what = "%s %s bias=%s act=%d" % (name, dt, b is not None, act)
                    assert torch.equal(g.float(), C.gemm_exact(prod, b, act, dt == BF16)), what
                    assert torch.equal(g[rows_dev].float().cpu(), C.gemm_exact(prod_cpu, b_cpu, act, dt == BF16)), what + " (CPU rows)"
            # out= a column slice of a wider matrix, canary rows before and after; and the same bits again
            got = ops.gemm_bf16_nt(a, bt, bias, ops.ACT_LRELU2, out_dtype=dt, transposed_out=c_tr)
            R, Cc = tuple(got.shape)
            wide = torch.full((R + 2, (Cc + 8 + 7) // 8 * 8), CANARY, dtype=dt, device=DEV)
            before = wide.clone()
            out = wide[1:R + 1, :Cc]
            ret = ops.gemm_bf16_nt(a, bt, bias, ops.ACT_LRELU2, out=out, transposed_out=c_tr)
            assert ret.data_ptr() == out.data_ptr()
            assert torch.equal(_bits(out.contiguous()), _bits(got)), "%s %s: out= differs from the plain call" % (name, dt)
            wide[1:R + 1, :Cc] = CANARY
            assert torch.equal(_bits(wide), _bits(before)), "%s %s: out= wrote beyond its [%d, %d] slice" % (name, dt, R, Cc)
    finally:
        ops.gemm_bf16_set_form(-1)


def _gemm_fn(act):
    return lambda a, bt, bias: C.act_ref(a @ bt.t() + bias, act)


@pytest.mark.parametrize("name", list(C.GEMM_CASES))
def test_gemm_gaussian_operands_within_the_store_bound(name):
    """The same cases on Gaussian operands rounded to bf16, bias + LeakyReLU, fp32 and bf16 output, against fp64 (the full matrix on the
    device, 64 rows on the CPU) under the store bounds.  The cases whose last round is cut along K run with and without the workspace:
    both results are within the bound and -- on the 256 CUs the cases were worked out for -- the two fp32 results are NOT bit-equal.
    Without the workspace the launcher cannot split (the same kernel runs whole tiles, or the 256 x 128 kernel replaces the 256 x 256
    one); partial sums added in another order are the only way the bits can differ, so the difference is the evidence that the split
    and its fix-up launch really ran."""
    M, N, K, form, c_tr = C.GEMM_CASES[name]
    on_256 = _path_claim(name)
    a, bt, bias = C.gemm_operands(name, "gauss", DEV)
    act = ops.ACT_LRELU2
    want = C.gemm_f64(C.gemm_product(a, bt), bias, act)
    rows = C.checked_rows(M, C.case_plan(name)["kernel"])
    args = H.f64((a[rows.to(DEV)].cpu(), bt.cpu(), bias.cpu()))
    want_cpu = _gemm_fn(act)(*args)
    print("%s: fp32_cpu_err %.3e on the checked rows, max |want| %.3e" % (name, H.fp32_cpu_err(_gemm_fn(act), *args)[0], float(want_cpu.abs().max())))
    old = ops.GEMM_BF16_KSPLIT
    ops.gemm_bf16_set_form(form)
    try:
        results = {}
        for ws in ((True, False) if name in C.SPLIT_CASES else (True,)):
            ops.GEMM_BF16_KSPLIT = ws
            for dt in (F32, BF16):
                got = ops.gemm_bf16_nt(a, bt, bias, act, out_dtype=dt, transposed_out=c_tr)
                g = got.t() if c_tr else got
                what = "%s %s workspace=%s" % (name, dt, ws)
                C.within_store(g, want, dt == BF16, what)
                C.within_store(g[rows.to(DEV)].cpu(), want_cpu, dt == BF16, what + " (CPU rows)")
                assert torch.equal(_bits(got), _bits(ops.gemm_bf16_nt(a, bt, bias, act, out_dtype=dt, transposed_out=c_tr))), what + ": not repeatable"
                results[ws, dt] = got
        if name in C.SPLIT_CASES and on_256:
            assert not torch.equal(results[True, F32], results[False, F32]), "%s: the K split left no trace in the bits" % name
    finally:
        ops.GEMM_BF16_KSPLIT = old
        ops.gemm_bf16_set_form(-1)


def test_gemm_without_rows():
    a = torch.empty(0, 64, dtype=BF16, device=DEV)
    bt = torch.ones(8, 64, dtype=BF16, device=DEV)
    for dt in (F32, BF16):
        got = ops.gemm_bf16_nt(a, bt, torch.ones(8, device=DEV), out_dtype=dt)
        assert tuple(got.shape) == (0, 8) and got.dtype == dt
    buf, y = _canary_out(256, F32)
    _lib.call("mgnns_gemm_bf16_nt_fwd", bt.data_ptr(), bt.data_ptr(), 0, 8, 64, None, y.data_ptr(), 8, 0, 0, None, 0, ops._stream())
    _untouched(buf, "a product without rows")


# ---- implicit-GEMM convolution --------------------------------------------------------------------------------------------------------
def _conv_raw(c, x, wt, bias, res):
    """the raw entry point into a canary-padded output -> (buffer, output view)"""
    oh, ow = C.conv_out_hw(c)
    buf, y = _canary_out(c["B"] * oh * ow * c["Cout"], F32 if c["nchw"] else BF16)
    _lib.call("mgnns_conv_bf16_nhwc_fwd", x.data_ptr(), c["B"], c["H"], c["W"], c["Cin"], wt.data_ptr(), bias.data_ptr(), c["Cout"],
              c["k"], c["k"], c["stride"], c["pad"], None if res is None else res.data_ptr(), int(c["relu"]), int(c["nchw"]),
              y.data_ptr(), ops._stream())
    return buf, y.view((c["B"], c["Cout"], oh, ow) if c["nchw"] else (c["B"], oh, ow, c["Cout"]))


def _conv_fn(c):
    def fn(x, wt, bias, res=None):
        return C.conv_f64(C.conv_sum(x, wt, bias, c, res), c)
    return fn


@pytest.mark.parametrize("c", C.CONV_CASES, ids=C.conv_id)
def test_conv_equals_fp64_on_integers_and_stays_within_the_store_bound(c):
    """ops.conv_bf16_nhwc / mgnns_conv_bf16_nhwc_fwd over CONV_CASES: C_out on and off both tile widths and beyond 32 column tiles, M
    round one row block, tiles that span images, 36 row blocks, 1 x 1 and 3 x 3 at every padding and stride the entry point takes,
    one-pixel images and outputs, C_in up to 512 (K = 4608), every epilogue.  Integer operands: bit for bit the fp64 sum -> fmaxf ->
    bf16 NHWC or fp32 NCHW.  Gaussian operands: within the store bound of fp64.  The raw entry point writes into a canary-padded
    buffer that must stay intact, and the wrapper gives the same bits."""
    for kind in ("int", "gauss"):
        x, wt, bias, res = C.conv_operands(c, kind)
        dev = [None if t is None else t.to(DEV) for t in (x.to(BF16), wt.to(BF16), bias, None if res is None else res.to(BF16))]
        buf, got = _conv_raw(c, *dev)
        _canaries_intact(buf, C.conv_id(c))
        via_ops = ops.conv_bf16_nhwc(dev[0], dev[1], dev[2], c["k"], c["stride"], c["pad"], residual=dev[3], relu=c["relu"], out_nchw_f32=c["nchw"])
        assert via_ops.dtype == got.dtype and torch.equal(_bits(via_ops), _bits(got.contiguous()))
        y64 = C.conv_ref(x, wt, bias, c, res)
        if kind == "int":
            assert float(y64.abs().max()) < C.EXACT
            assert torch.equal(got.float().cpu(), C.conv_exact(y64, c)), C.conv_id(c)
        else:
            args = H.f64((x, wt, bias) + (() if res is None else (res,)))
            print("%s: fp32_cpu_err %.3e" % (C.conv_id(c), H.fp32_cpu_err(_conv_fn(c), *args)[0]))
            C.within_store(got.cpu(), C.conv_f64(y64, c), not c["nchw"], C.conv_id(c))


def test_conv_of_an_empty_batch():
    wt, bias = torch.ones(72, 64, dtype=BF16, device=DEV), torch.ones(72, device=DEV)
    y = ops.conv_bf16_nhwc(torch.empty(0, 5, 5, 64, dtype=BF16, device=DEV), wt, bias, 1)
    assert tuple(y.shape) == (0, 5, 5, 72)
    y = ops.conv_bf16_nhwc(torch.empty(0, 5, 5, 64, dtype=BF16, device=DEV), wt, bias, 1, stride=2, out_nchw_f32=True)
    assert tuple(y.shape) == (0, 72, 3, 3) and y.dtype == F32
    buf, out = _canary_out(256, BF16)
    _lib.call("mgnns_conv_bf16_nhwc_fwd", wt.data_ptr(), 0, 5, 5, 64, wt.data_ptr(), bias.data_ptr(), 72, 1, 1, 1, 0, None, 1, 0, out.data_ptr(),
              ops._stream())
    _untouched(buf, "a convolution of an empty batch")


# ---- stem and max-pool ----------------------------------------------------------------------------------------------------------------
def _stem_raw(img, wt, bias, raw):
    B, _, Hh, Ww = img.shape
    oh, ow = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
    buf, y = _canary_out(B * oh * ow * 64, BF16)
    if raw:
        _lib.call("mgnns_stem_conv7_raw_fwd", img.data_ptr(), B, Hh, Ww, wt.data_ptr(), y.data_ptr(), ops._stream())
    else:
        _lib.call("mgnns_stem_conv7_fwd", img.data_ptr(), B, Hh, Ww, wt.data_ptr(), bias.data_ptr(), y.data_ptr(), ops._stream())
    return buf, y.view(B, oh, ow, 64)


@pytest.mark.parametrize("Hh", C.STEM_H)
def test_stem_folded_and_raw(Hh):
    """stem_conv7 (bias + ReLU) and its raw form (the convolution alone) on images of Hh x {7, 63, 64, 65, 66}: round the 8-row x 32-column
    workgroup tile, down to the smallest image.  The weights come through conv_fold_bn(w, conv_bias, None, stem=True): scale 1, bias =
    conv_bias.  Integers: bit for bit; Gaussian: within the bf16 store bound of fp64 on the bf16-rounded image and weights."""
    for Ww in C.STEM_W:
        for kind in ("int", "gauss"):
            img, w, cb = C.stem_operands(2, Hh, Ww, kind)
            wt, bias = ops.conv_fold_bn(w.to(DEV), cb.to(DEV), None, stem=True)
            assert torch.equal(bias.cpu(), cb)
            assert torch.equal(_bits(wt), _bits(ops.conv_fold_bn(w.to(DEV), None, None, stem=True)[0]))
            wr, ir = (w, img) if kind == "int" else (bf16_round(w), bf16_round(img))
            assert torch.equal(wt[:, :147].float().cpu().double(), wr.reshape(64, 147).double())
            for raw in (False, True):
                what = "stem %dx%d %s%s" % (Hh, Ww, kind, " raw" if raw else "")
                buf, got = _stem_raw(img.to(DEV), wt, bias, raw)
                _canaries_intact(buf, what)
                assert torch.equal(_bits(ops.stem_conv7(img.to(DEV), wt, bias, raw=raw)), _bits(got))
                y64 = C.stem_ref(ir, wr, None if raw else cb)
                if kind == "int":
                    v = y64.float() if raw else y64.float().clamp_min(0)
                    assert torch.equal(got.float().cpu(), bf16_round(v).float()), what
                else:
                    fn = (lambda i, ww, b: C.stem_sum(i, ww)) if raw else (lambda i, ww, b: C.stem_sum(i, ww, b).clamp_min(0))
                    args = H.f64((ir, wr, cb))
                    print("%s: fp32_cpu_err %.3e" % (what, H.fp32_cpu_err(fn, *args)[0]))
                    H.within_bf16_store(got, fn(*args), what)


@pytest.mark.parametrize("Cc", C.POOL_C)
def test_maxpool_signed_inputs_equal_max_pool2d(Cc):
    """MaxPool2d(3, 2, 1) on signed data whose channels 0..3 are negative everywhere -- a pool that pads with 0 instead of -inf fails every
    border window -- at H, W in {1, 2, 3, 8, 9}: exactly F.max_pool2d."""
    for Hh in C.POOL_HW:
        for Ww in C.POOL_HW:
            x = C.pool_operands(2, Hh, Ww, Cc)
            xg = x.to(BF16).to(DEV)
            oh, ow = (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1
            buf, y = _canary_out(2 * oh * ow * Cc, BF16)
            _lib.call("mgnns_maxpool3x3s2_nhwc_fwd", xg.data_ptr(), 2, Hh, Ww, Cc, y.data_ptr(), ops._stream())
            _canaries_intact(buf, "pool %dx%dx%d" % (Hh, Ww, Cc))
            want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
            assert float(want[..., :4].max()) < 0
            assert torch.equal(y.view(2, oh, ow, Cc).float().cpu(), want), (Hh, Ww, Cc)
            assert torch.equal(ops.maxpool3x3s2_nhwc(xg).float().cpu(), want)


def test_stem_and_pool_of_an_empty_batch():
    _, w, cb = C.stem_operands(1, 7, 7, "int")
    wt, bias = ops.conv_fold_bn(w.to(DEV), cb.to(DEV), None, stem=True)
    empty = torch.empty(0, 3, 9, 17, device=DEV)
    for raw in (False, True):
        assert tuple(ops.stem_conv7(empty, wt, bias, raw=raw).shape) == (0, 5, 9, 64)
    assert tuple(ops.maxpool3x3s2_nhwc(torch.empty(0, 9, 8, 72, dtype=BF16, device=DEV)).shape) == (0, 5, 4, 72)
    buf, y = _canary_out(256, BF16)
    img = torch.ones(1, 3, 9, 17, device=DEV)
    _lib.call("mgnns_stem_conv7_fwd", img.data_ptr(), 0, 9, 17, wt.data_ptr(), bias.data_ptr(), y.data_ptr(), ops._stream())
    _lib.call("mgnns_stem_conv7_raw_fwd", img.data_ptr(), 0, 9, 17, wt.data_ptr(), y.data_ptr(), ops._stream())
    _lib.call("mgnns_maxpool3x3s2_nhwc_fwd", wt.data_ptr(), 0, 9, 8, 72, y.data_ptr(), ops._stream())
    _untouched(buf, "an empty batch")


# ---- fold and transpose-cast ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_fold_bit_for_bit(with_bn, with_bias):
    """conv_fold_bn with and without BatchNorm and conv_bias, both K orders, and -- through the entry point -- rows longer than K (the
    tail must be zero): weights and bias bit for bit (the BatchNorm of fold_operands is dyadic, so no grouping of the bias arithmetic
    rounds; the weights are Gaussian and round for real)."""
    for Cout, Cin, k, stem in ((72, 64, 3, False), (40, 128, 1, False), (64, 3, 7, True)):
        w, cb, bn = C.fold_operands(Cout, Cin, k, with_bn, with_bias)
        d = lambda t: None if t is None else t.to(DEV)
        bn_dev = None if bn is None else tuple(d(t) for t in bn[:4]) + (bn[4],)
        wt, bias = ops.conv_fold_bn(d(w), d(cb), bn_dev, stem=stem)
        want_w, want_b = C.fold_ref(w, cb, bn, stem=stem, ld=ops.STEM_LD if stem else None)
        assert torch.equal(wt.float().cpu(), want_w) and torch.equal(bias.cpu(), want_b), (Cout, Cin, k, stem)
        K = Cin * k * k
        ld = K + 24
        buf, out = _canary_out(Cout * ld, BF16)
        bias2 = torch.full((Cout,), CANARY, device=DEV)
        g, b, m, v = (None,) * 4 if bn is None else bn_dev[:4]
        p = lambda t: None if t is None else t.data_ptr()
        wd, cbd = d(w), d(cb)
        _lib.call("mgnns_conv_fold_bn_bf16", wd.data_ptr(), p(cbd), Cout, Cin, k, k, p(g), p(b), p(m), p(v), 0.0, 1 if stem else 0, ld,
                  out.data_ptr(), bias2.data_ptr(), ops._stream())
        _canaries_intact(buf, "fold")
        assert torch.equal(out.view(Cout, ld).float().cpu(), C.fold_ref(w, cb, bn, stem=stem, ld=ld)[0]) and torch.equal(bias2.cpu(), want_b)


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 65])
def test_transpose_cast_bit_for_bit(rows):
    """transpose_cast_bf16 at rows x {1, 31, 32, 33, 65} columns -- round its 32 x 32 tile -- with the finite values of BF16_SPECIALS (ties
    to even either way, one bit either side of a tie, zeros, denormals, the largest finite values) among Gaussians: the kernels'
    integer rounding bit for bit, the padding to 64 zero."""
    sp = C.finite_specials()
    for cols in (1, 31, 32, 33, 65):
        x = np.random.RandomState(rows * 100 + cols).standard_normal((rows, cols)).astype(np.float32)
        flat = x.reshape(-1)
        n = min(len(sp), flat.size)
        pos = np.random.RandomState(cols).choice(flat.size, n, replace=False)
        flat[pos] = np.roll(sp, rows + cols)[:n]
        y = ops.transpose_cast_bf16(torch.from_numpy(x).to(DEV))
        assert tuple(y.shape) == (cols, C.kpad(rows))
        got = y.view(torch.int16).cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:, :rows], bf16_bits(x.T)), (rows, cols)
        assert not got[:, rows:].any()


# ---- the whole trunk ------------------------------------------------------------------------------------------------------------------
def test_resnet50_on_a_small_odd_image():
    """ResNet-50 on a 2 x 3 x 39 x 71 image (every stage on odd, unequal sizes down to 2 x 3) against the rounding-emulating oracle, under
    the bound of tests/test_trunk_gpu.py."""
    m = synth.fill_trunk_(trunk.resnet50(365), 5).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    feats = trunk.ResNetFeatures(m).to(DEV).eval()
    img = torch.from_numpy(np.random.RandomState(39).standard_normal((2, 3, 39, 71)).astype(np.float32))
    y = feats(img.to(DEV)).cpu()
    ref = trunk_cpu.features_bf16_emulated(sd, img)
    f32 = trunk_cpu.features_fp32(sd, img)
    assert tuple(y.shape) == tuple(ref.shape) == (2, 2048, 2, 3) and y.dtype == F32
    scale = float(f32.abs().max())
    err = float((y - ref).abs().max()) / scale
    print("resnet50 39x71: max err vs the emulated oracle %.3e of max |f32| = %.3g" % (err, scale))
    assert err < 2e-2


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _conv_args(x, wt, bias, y, B=1, Hh=4, Ww=4, Cin=64, Cout=72, k=1, stride=1, pad=0):
    return (x, B, Hh, Ww, Cin, wt, bias, Cout, k, k, stride, pad, None, 1, 0, y, ops._stream())


CONV_REFUSALS = [
    ("C_in 32", r"power of two >= 64 \(got 32\)", dict(Cin=32)),
    ("C_in 96", r"power of two >= 64 \(got 96\)", dict(Cin=96)),
    ("C_out 4", r"C_out % 8 != 0 \(got 4\)", dict(Cout=4)),
    ("5 x 5", r"1x1 or 3x3 \(got 5x5\)", dict(k=5, pad=2, Hh=8, Ww=8)),
    ("pad 2 on 3 x 3", r"bad stride 1 / padding 2", dict(k=3, pad=2)),
    ("pad 1 on 1 x 1", r"bad stride 1 / padding 1", dict(k=1, pad=1)),
    ("stride 0", r"bad stride 0 / padding 0", dict(stride=0)),
    ("empty output", r"empty output", dict(k=3, pad=0, Hh=2, Ww=2)),
    ("empty output at stride 2", r"empty output", dict(k=3, pad=0, Hh=2, Ww=2, stride=2)),     # (2 - 3) / 2 + 1 truncates to one pixel
    ("misaligned x", r"16-byte aligned", dict(off_x=2)),
    ("misaligned y", r"16-byte aligned", dict(off_y=2)),
]


@pytest.mark.parametrize("what,match,kw", CONV_REFUSALS, ids=[r[0].replace(" ", "_") for r in CONV_REFUSALS])
def test_conv_refusals_leave_the_output_alone(what, match, kw):
    big = torch.zeros(1 << 18, dtype=BF16, device=DEV)             # every operand is large enough for the call, were it not refused
    bias = torch.zeros(4160, device=DEV)
    buf, y = _canary_out(1 << 16, BF16)
    kw = dict(kw)
    x_ptr, y_ptr = big.data_ptr() + kw.pop("off_x", 0), y.data_ptr() + kw.pop("off_y", 0)
    with pytest.raises(RuntimeError, match=match):
        _lib.call("mgnns_conv_bf16_nhwc_fwd", *_conv_args(x_ptr, big.data_ptr(), bias.data_ptr(), y_ptr, **kw))
    _untouched(buf, what)


def test_pool_and_stem_refusals_leave_the_output_alone():
    big = torch.zeros(1 << 14, dtype=BF16, device=DEV)
    img, bias = torch.zeros(1, 3, 8, 8, device=DEV), torch.zeros(64, device=DEV)
    buf, y = _canary_out(1 << 14, BF16)
    with pytest.raises(RuntimeError, match=r"need C % 8 == 0 \(B=1 H=4 W=4 C=4\)"):
        _lib.call("mgnns_maxpool3x3s2_nhwc_fwd", big.data_ptr(), 1, 4, 4, 4, y.data_ptr(), ops._stream())
    with pytest.raises(RuntimeError, match=r"mgnns_stem_conv7_fwd: bad dims B=1 H=6 W=8"):
        _lib.call("mgnns_stem_conv7_fwd", img.data_ptr(), 1, 6, 8, big.data_ptr(), bias.data_ptr(), y.data_ptr(), ops._stream())
    with pytest.raises(RuntimeError, match=r"mgnns_stem_conv7_raw_fwd: bad dims B=1 H=8 W=6"):
        _lib.call("mgnns_stem_conv7_raw_fwd", img.data_ptr(), 1, 8, 6, big.data_ptr(), y.data_ptr(), ops._stream())
    _untouched(buf, "a refused pool / stem")


GEMM_REFUSALS = [
    ("N % 4", r"need N % 4 == 0.*N=6 ", dict(N=6, ldc=8)),
    ("Kp % 64", r"Kp % 64 == 0.*Kp=96 ", dict(Kp=96)),
    ("ldc < N", r"ldc=124\)", dict(ldc=124)),
    ("ldc % 4", r"ldc=130\)", dict(ldc=130)),
    ("act 3", r"unknown activation 3", dict(act=3)),
    ("c_bf16 4", r"c_bf16=4", dict(c_bf16=4)),
    ("transposed store, too few rows", r"the transposed store is the 160 x 256 kernel's \(M=1120 ", dict(M=1120, N=256, Kp=320, ldc=1120, c_bf16=2)),
    ("transposed store, short K", r"the transposed store is the 160 x 256 kernel's", dict(M=1121, N=256, Kp=256, ldc=1124, c_bf16=3)),
    ("misaligned A", r"16-byte aligned", dict(off_a=2)),
]


@pytest.mark.parametrize("what,match,kw", GEMM_REFUSALS, ids=[r[0].replace(" ", "_") for r in GEMM_REFUSALS])
def test_gemm_refusals_leave_the_output_alone(what, match, kw):
    big = torch.zeros(1121 * 320, dtype=BF16, device=DEV)
    buf, y = _canary_out(1124 * 256, F32)
    kw = dict(dict(M=64, N=128, Kp=64, ldc=128, c_bf16=0, act=0, off_a=0), **kw)
    with pytest.raises(RuntimeError, match=match):
        _lib.call("mgnns_gemm_bf16_nt_fwd", big.data_ptr() + kw["off_a"], big.data_ptr(), kw["M"], kw["N"], kw["Kp"], None, y.data_ptr(), kw["ldc"],
                  kw["c_bf16"], kw["act"], None, 0, ops._stream())
    _untouched(buf, what)
