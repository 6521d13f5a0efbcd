"""The BatchNorm training kernels (csrc/bn_train.hip) one by one, against fp64 over the same stored operands: the statistics of the
stored bf16 z, the normalise-and-activate sweep from the kernel's own (mean, rstd), and the backward from the same.

Gates (the reasons are DESIGN.md 14's): statistics to 1e-5 (fp32 eps x log2 M ~ 1e-6, ten times margin; E[z^2] - mean^2 from raw fp32
sums misses it by ~6e-3 on channels drawn as 256 + N(0, 1)); outputs to one bf16 rounding, 2^-8 |ref|, plus 1e-5 of the magnitudes
that were added; sums to 1e-6 of the sum of magnitudes."""
import functools

import pytest
import torch

from mgnns_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
SHAPES = [(2, 64), (18, 256), (126, 64), (180, 512), (40, 2048), (4099, 64)]
CASES = ["%dx%d" % s for s in SHAPES] + ["constant_channels", "offset_256"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (z bf16 [M, C] on the GPU, z fp64 on the CPU, fp64 mean, biased variance): the reference, computed once per case."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "constant_channels":                                      # every 7th channel constant: var = 0
        z = torch.randn(180, 512, generator=g) * 1.5 + 0.25
        z[:, ::7] = torch.randn(512, generator=g)[::7]
    elif name == "offset_256":                                           # the mean is 256 times the spread
        z = 256 + torch.randn(4099, 64, generator=g)
    else:
        M, C = map(int, name.split("x"))
        z = torch.randn(M, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    z = z.to(torch.bfloat16)
    z64 = z.double()
    return z.to(DEV), z64, z64.mean(0), z64.var(0, unbiased=False)


@functools.lru_cache(maxsize=None)
def kernel_stats(name):
    z = case(name)[0]
    return ops.bn_stats_bf16_nhwc(z, EPS, want_var=True)


def params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + torch.rand(C, generator=g)).to(DEV), torch.randn(C, generator=g).to(DEV)


@pytest.mark.parametrize("name", CASES)
def test_statistics_against_fp64_of_the_stored_values(name):
    z, z64, mean64, var64 = case(name)
    M, C = z.shape
    mean, rstd, var = kernel_stats(name)
    if name == "constant_channels":
        assert (var64[::7] == 0).all() and (var.cpu()[::7] == 0).all()
    if name == "offset_256":
        assert (mean64 / var64.sqrt()).min() > 100
    tol = 1e-5 * torch.maximum(mean64.abs(), var64.sqrt())
    err = (mean.cpu().double() - mean64).abs()
    rstd64 = 1.0 / torch.sqrt(var64 + EPS)
    rel = (rstd.cpu().double() / rstd64 - 1).abs()
    print("%s: mean err / tol max %.3g, rstd rel max %.3g" % (name, float((err / tol.clamp_min(1e-300)).max()), float(rel.max())))
    assert (err <= tol).all()
    assert (rel <= 1e-5).all()
    assert torch.allclose(rstd, 1.0 / torch.sqrt(var + EPS), rtol=5e-7, atol=0)   # var is the variance rstd was formed from
    # a second call is bit-identical, with and without the variance
    again = ops.bn_stats_bf16_nhwc(z, EPS)
    assert len(again) == 2 and torch.equal(again[0], mean) and torch.equal(again[1], rstd)
    # running buffers: the fp64 update from the kernel's own mean / variance
    g = torch.Generator().manual_seed(3)
    rm0, rv0 = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    for momentum in (0.1, 1.0):
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        versions = rm._version, rv._version
        m2, r2 = ops.bn_stats_bf16_nhwc(z, EPS, running=(rm, rv), momentum=momentum)
        assert torch.equal(m2, mean) and torch.equal(r2, rstd)
        assert rm._version > versions[0] and rv._version > versions[1]  # what derives from the buffers refolds
        want_m = (1 - momentum) * rm0.double() + momentum * mean.cpu().double()
        want_v = (1 - momentum) * rv0.double() + momentum * var.cpu().double() * M / (M - 1)
        assert ((rm.cpu().double() - want_m).abs() <= 1e-6 * want_m.abs()).all(), momentum
        assert ((rv.cpu().double() - want_v).abs() <= 1e-6 * want_v.abs()).all(), momentum
    # without buffers nothing is written
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    ops.bn_stats_bf16_nhwc(z, EPS, momentum=0.1)
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and rm._version == 0


def test_refusals():
    v = torch.ones(16, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.bn_stats_bf16_nhwc(torch.zeros(4, 12, device=DEV, dtype=torch.bfloat16), EPS)
    one = torch.zeros(1, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="two values"):
        ops.bn_stats_bf16_nhwc(one, EPS)
    with pytest.raises(ValueError, match="two values"):
        ops.bn_apply_bf16_nhwc(one, v, v, v, v)
    with pytest.raises(ValueError, match="two values"):
        ops.bn_backward_bf16_nhwc(one, one, v, v, v)
    z = torch.zeros(4, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="momentum"):
        ops.bn_stats_bf16_nhwc(z, EPS, running=(v.clone(), v.clone()), momentum=None)
    with pytest.raises(TypeError):
        ops.bn_stats_bf16_nhwc(z.float(), EPS)
    with pytest.raises(ValueError, match="entries"):
        ops.bn_apply_bf16_nhwc(z, v[:8].contiguous(), v, v, v)
    with pytest.raises(ValueError, match="residual"):
        ops.bn_apply_bf16_nhwc(z, v, v, v, v, residual=z[:2].contiguous())
    with pytest.raises(ValueError, match="OH, OW"):
        ops.bn_apply_bf16_nhwc(z, v, v, v, v, out_nchw_f32=True)


def apply_reference(z64, res64, mean, rstd, gamma, beta):
    """-> (ref before the ReLU, the slack 1e-5 (|a z| + |b| + |res|)) in fp64 from the fp32 statistics and parameters."""
    a = gamma.cpu().double() * rstd.cpu().double()
    b = beta.cpu().double() - mean.cpu().double() * a
    ref = a * z64 + b
    slack = (a * z64).abs() + b.abs()
    if res64 is not None:
        ref = ref + res64
        slack = slack + res64.abs()
    return ref, 1e-5 * slack


def check_apply(y64, ref, slack, relu, rounded):
    want = ref.clamp_min(0) if relu else ref
    tol = slack + (2.0 ** -8 * want.abs() if rounded else 0)
    assert ((y64 - want).abs() <= tol).all()
    if relu:
        assert (y64[ref < -slack] == 0).all() and (y64 >= 0).all()


@pytest.mark.parametrize("name", CASES)
def test_apply_against_fp64_from_the_kernels_own_statistics(name):
    z, z64, _, _ = case(name)
    M, C = z.shape
    mean, rstd, _ = kernel_stats(name)
    gamma, beta = params(C, 5)
    res = torch.randn(M, C, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    for residual in (None, res):
        ref, slack = apply_reference(z64, None if residual is None else residual.double(), mean, rstd, gamma, beta)
        for relu in (True, False):
            r = None if residual is None else residual.to(DEV)
            y = ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta, residual=r, relu=relu)
            assert y.dtype == torch.bfloat16 and y.shape == z.shape
            check_apply(y.cpu().double(), ref, slack, relu, rounded=True)
            assert torch.equal(y, ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta, residual=r, relu=relu))


@pytest.mark.parametrize("shape", [(2, 3, 3, 256), (3, 4, 5, 72), (2, 14, 14, 64)])
def test_apply_writes_the_unrounded_fp32_nchw_map(shape):
    B, OH, OW, C = shape
    assert OH * OW in (9, 20, 196)
    g = torch.Generator().manual_seed(OH * OW)
    z = (torch.randn(*shape, generator=g) * 2 + 0.5).to(torch.bfloat16)
    res = torch.randn(*shape, generator=g).to(torch.bfloat16)
    zd, rd = z.to(DEV), res.to(DEV)
    mean, rstd = ops.bn_stats_bf16_nhwc(zd, EPS)
    assert torch.equal(mean, ops.bn_stats_bf16_nhwc(zd.view(-1, C), EPS)[0])          # [M, C] and NHWC are the same view
    gamma, beta = params(C, 7)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    for residual in (None, rd):
        ref, slack = apply_reference(z.double(), None if residual is None else res.double(), mean, rstd, gamma, beta)
        for relu in (True, False):
            y = ops.bn_apply_bf16_nhwc(zd, mean, rstd, gamma, beta, residual=residual, relu=relu, out_nchw_f32=True)
            assert y.dtype == torch.float32 and tuple(y.shape) == (B, C, OH, OW) and y.is_contiguous()
            check_apply(y.cpu().double(), nchw(ref), nchw(slack), relu, rounded=False)
            assert torch.equal(y, ops.bn_apply_bf16_nhwc(zd, mean, rstd, gamma, beta, residual=residual, relu=relu, out_nchw_f32=True))
            # rounded once, it is the NHWC bf16 output
            yh = ops.bn_apply_bf16_nhwc(zd, mean, rstd, gamma, beta, residual=residual, relu=relu)
            assert torch.equal(nchw(yh), y.to(torch.bfloat16))


@pytest.mark.parametrize("name", CASES)
def test_backward_against_fp64_from_the_saved_statistics(name):
    z, z64, _, _ = case(name)
    M, C = z.shape
    mean, rstd, _ = kernel_stats(name)
    gamma, _ = params(C, 8)
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(M, C, generator=gen) * (torch.rand(M, C, generator=gen) > 0.4)    # as a ReLU's producer leaves it: many zeros
    g = g.to(torch.bfloat16)
    g64, gd = g.double(), g.to(DEV)
    gz, dgamma, dbeta = ops.bn_backward_bf16_nhwc(gd, z, mean, rstd, gamma)
    assert gz.dtype == torch.bfloat16 and gz.shape == z.shape
    mu, rs, ga = mean.cpu().double(), rstd.cpu().double(), gamma.cpu().double()
    xhat = (z64 - mu) * rs
    db64, dg64 = g64.sum(0), (g64 * xhat).sum(0)
    assert ((dbeta.cpu().double() - db64).abs() <= 1e-6 * g64.abs().sum(0)).all()
    assert ((dgamma.cpu().double() - dg64).abs() <= 1e-6 * (g64 * xhat).abs().sum(0)).all()
    ref = ga * rs * (g64 - db64 / M - xhat * dg64 / M)
    tol = 2.0 ** -8 * ref.abs() + 1e-5 * (ga * rs).abs() * (g64.abs() + db64.abs() / M + (xhat * dg64).abs() / M)
    assert ((gz.cpu().double() - ref).abs() <= tol).all()
    # the sums not wanted: g_z bit-equal; a second call: everything bit-equal
    for want in ((False, False), (True, False), (False, True)):
        gz2, dg2, db2 = ops.bn_backward_bf16_nhwc(gd, z, mean, rstd, gamma, want=want)
        assert torch.equal(gz2, gz) and (dg2 is None) == (not want[0]) and (db2 is None) == (not want[1])
        assert dg2 is None or torch.equal(dg2, dgamma)
        assert db2 is None or torch.equal(db2, dbeta)
    again = ops.bn_backward_bf16_nhwc(gd, z, mean, rstd, gamma)
    assert all(torch.equal(a, b) for a, b in zip(again, (gz, dgamma, dbeta)))
