"""Cases, generators, references and the launcher restatement of the matrix-pipe edge sweep: the dense bf16 GEMM (csrc/gemm_bf16.hip)
and the trunk forward kernels (csrc/conv_bf16.hip).  tests/test_matrix_pipe_edges_gpu.py runs the kernels on these cases,
tests/test_matrix_pipe_edges_cpu.py checks this file itself (the restatement against the library's host arithmetic, the references
against torch in double, the exactness budgets, and that wrong kernels -- the mutants below -- would be caught).

The first pass needs no tolerance: operands are small integers, so every value is exact in bf16, every partial sum stays below 2^24
and fp32 accumulation is exact in ANY order -- the kernel must equal the fp64 reference bit for bit.  The second pass uses Gaussian
operands rounded to bf16 against fp64 under the project's bf16-store bound (tests/helpers.py: within_bf16_store)."""
import numpy as np
import torch

from oracle.bf16_path import bf16_round

ACT_NONE, ACT_RELU, ACT_LRELU2 = 0, 1, 2
SLOPE = float(np.float32(0.2))          # mg_act: v > 0 ? v : 0.2f * v, one fp32 multiply
EXACT = 1 << 24                         # integers below this are exact in fp32, and so is every sum of them


def ceil_div(a, b):
    return (a + b - 1) // b


def kpad(k):
    return ceil_div(k, 64) * 64


# ---- the launcher of csrc/gemm_bf16.hip, restated ---------------------------------------------------------------------------------------
K128, K256, K160, K320 = "256x128", "256x256", "160x256", "320x256"
TM, TN, BK, TM2, TN2, TM160, TN160, TM320, TN320 = 256, 128, 64, 256, 256, 160, 256, 320, 256
WORKSPACE_BYTES = 256 * TM2 * TN2 * 4   # mgnns_gemm_bf16_workspace_bytes


def gemm_fits(M, N, Kp, tm):
    return ceil_div(M, tm) >= 8 and N >= 256 and Kp >= 320


def gemm_pick(M, N, Kp, ws_ok, n_cu=256, form=2, c_tr=False, workspace_bytes=WORKSPACE_BYTES):
    """mg_gemm_pick (no device row count): the kernel a product runs on."""
    if c_tr:
        return K160
    per = max(n_cu // 8, 1)
    nrb1, nct1, nrb2, nct2 = ceil_div(M, TM), ceil_div(N, TN), ceil_div(M, TM2), ceil_div(N, TN2)
    elig256 = bool(ws_ok) and nrb2 // 8 * nct2 >= per and N >= TN2 and Kp // BK >= 64 and workspace_bytes >= 8 * per * TM2 * TN2 * 4
    older = K256 if elig256 else K128
    fits160, fits320 = gemm_fits(M, N, Kp, TM160), gemm_fits(M, N, Kp, TM320)
    if form == 1:
        return K160 if fits160 else older
    if form == 3:
        return K320 if fits320 else older
    if form == 0 or not (fits160 or fits320):
        return older
    nk64 = Kp // BK

    def rounds(t, ksplit):
        full, rem = t // per, t % per
        if rem == 0:
            return float(full)
        f = min(per // rem, 8)
        return full + (1.0 / f + 0.0625 if (ksplit and 4 * rem <= per and f * 8 <= nk64) else 1.0)

    def cost(r, rows, fixed):
        return r * (float(Kp // 32) * rows + fixed)

    best = cost(rounds(ceil_div(nrb1, 8) * nct1, bool(ws_ok)), TM + TN, 2100)
    if elig256:
        best = min(best, cost(rounds(ceil_div(nrb2, 8) * nct2, True), TM2 + TN2, 8000))
    pick = older
    if fits160:
        c160 = cost(rounds(ceil_div(ceil_div(M, TM160), 8) * ceil_div(N, TN160), False), TM160 + TN160, 5200) * 1.02
        if c160 < best:
            best, pick = c160, K160
    if fits320:
        c320 = cost(rounds(ceil_div(ceil_div(M, TM320), 8) * ceil_div(N, TN320), False), TM320 + TN320, 8800) * 1.02
        if c320 < best:
            pick = K320
    return pick


def pick_form_code(kernel):
    """what mgnns_gemm_bf16_pick_form answers for a kernel"""
    return {K160: 4, K320: 5}.get(kernel, 0)


def gemm_split(xcd, nrb, nct, rps, jmax, W, nk):
    """mg_gemm_split: (T, full, rem, f) of an XCD of the 256 x 128 kernel."""
    if rps == 0:
        cpx = jmax // nrb
        T = min(max(nct - xcd * cpx, 0), cpx) * nrb
    else:
        T = ((xcd + 1) * nrb // 8 - xcd * nrb // 8) * nct
    full = T // W
    rem = T - full * W
    f = 0
    if rem > 0 and 4 * rem <= W:
        f = min(W // rem, 8)
        if f * 8 > nk:
            f = 0
    return T, full, rem, f


def gemm256_split(T, W, nk):
    """gemm256_split: (full, rem, f) of an XCD of the 256 x 256 kernel; f == 1: the left-over tiles stay whole."""
    full = T // W
    rem = T - full * W
    f = min(W // rem, 8) if rem > 0 else 0
    if f < 2 or f * 4 > nk:
        f = 1 if rem > 0 else 0
    return full, rem, f


def ops_gives_workspace(M, N):
    """ops.gemm_bf16_nt passes the workspace for products of at least 2^20 outputs (GEMM_BF16_KSPLIT on)"""
    return M * N >= (1 << 20)


def gemm_plan(M, N, Kp, ws_ok, n_cu=256, form=0, c_tr=False):
    """mg_launch_gemm_bf16 -> dict(kernel, xcds = [(T, full, rem, f)] per XCD, fixup = a fix-up launch follows, W, and for the 256 x 128
    kernel rps (0 = the column-split map), for the whole-tile kernels most = the most tiles one workgroup walks)."""
    kernel = gemm_pick(M, N, Kp, ws_ok, n_cu, form, c_tr)
    per = max(n_cu // 8, 1)
    nk = Kp // BK
    if kernel == K128:
        nrb, nct = ceil_div(M, TM), ceil_div(N, TN)
        rps, jmax = 1, ceil_div(nrb, 8) * nct
        if nrb < 8 and nct >= 8:
            rps, jmax = 0, nrb * ceil_div(nct, 8)
        W = min(per, jmax)
        xcds = [gemm_split(x, nrb, nct, rps, jmax, W, nk) for x in range(8)]
        on = bool(ws_ok) and WORKSPACE_BYTES >= 8 * W * TM * TN * 4 and any(f for _, _, _, f in xcds)
        if not on:
            xcds = [(T, full, rem, 0) for T, full, rem, _ in xcds]
        return dict(kernel=kernel, xcds=xcds, fixup=on, W=W, rps=rps)
    if kernel == K256:
        nrb, nct = ceil_div(M, TM2), ceil_div(N, TN2)
        xcds = []
        for x in range(8):
            T = ((x + 1) * nrb // 8 - x * nrb // 8) * nct
            xcds.append((T,) + gemm256_split(T, per, nk))
        return dict(kernel=kernel, xcds=xcds, fixup=any(f >= 2 for _, _, _, f in xcds), W=per)
    tm, tn = (TM160, TN160) if kernel == K160 else (TM320, TN320)
    nrb, nct = ceil_div(M, tm), ceil_div(N, tn)
    xcds = [(((x + 1) * nrb // 8 - x * nrb // 8) * nct, 0, 0, 0) for x in range(8)]
    return dict(kernel=kernel, xcds=xcds, fixup=False, W=per, most=max(ceil_div(T, per) for T, _, _, _ in xcds))


def tile_rows(kernel):
    return {K128: TM, K256: TM2, K160: TM160, K320: TM320}[kernel]


# ---- GEMM cases ----------------------------------------------------------------------------------------------------------------------
# name -> (M, N, K, form, transposed store).  K is padded to 64 with zeros.  What each is for -- the claim GEMM_CLAIMS checks -- is
# stated for a 256-CU device.
GEMM_CASES = {
    # 256 x 128 kernel, row map, last round cut along K
    "k128_rows_f4": (2048, 5120, 2048, 0, False),         # (T, full, rem, f) = (40, 1, 8, 4) on every XCD
    "k128_rows_f8_ragged": (1800, 4100, 4096, 0, False),  # (33, 1, 1, 8), ragged M and N
    # 256 x 128 kernel, column-split map (fewer row blocks than XCDs), last round cut along K
    "k128_cols_f8_f4": (1024, 8320, 4096, 0, False),      # seven XCDs (36, 1, 4, 8), the last (8, 0, 8, 4): a split with no full round before it
    "k128_cols_f8_whole_empty": (1792, 4300, 4096, 0, False),   # six XCDs (35, 1, 3, 8), one with 28 whole tiles, one empty
    # 256 x 256 kernel (needs the workspace)
    "k256_no_rem": (8192, 2048, 4096, 0, False),
    "k256_f4_f1": (8300, 2312, 4100, 0, False),
    "k256_f2_f1": (8200, 2700, 4100, 0, False),
    # 160 x 256 and 320 x 256 kernels: the smallest fits, a ragged product where workgroups walk two tiles, the transposed store
    "k160_min": (1121, 256, 320, 1, False),
    "k320_min": (2241, 516, 330, 3, False),
    "k160_two_tiles": (8950, 1100, 330, 1, False),
    "k320_two_tiles": (17900, 1100, 330, 3, False),
    "k160_transposed": (1121, 260, 330, 1, True),
    # no split, small sizes (the 256 x 128 kernel)
    "small_1x4": (1, 4, 64, 0, False),
    "small_255x124": (255, 124, 64, 0, False),
    "small_256x128": (256, 128, 64, 0, False),
    "small_257x132": (257, 132, 128, 0, False),
}
SPLIT_CASES = ("k128_rows_f4", "k128_rows_f8_ragged", "k128_cols_f8_f4", "k128_cols_f8_whole_empty", "k256_f4_f1", "k256_f2_f1")


def case_plan(name, n_cu=256, ws=None):
    M, N, K, form, c_tr = GEMM_CASES[name]
    ws = ops_gives_workspace(M, N) if ws is None else ws
    return gemm_plan(M, N, kpad(K), ws, n_cu, form, c_tr)


def _claim_k128(xcd_sets, rps):
    def check(p):
        assert p["kernel"] == K128 and p["rps"] == rps and p["fixup"], p
        assert sorted(p["xcds"]) == sorted(xcd_sets), p["xcds"]
    return check


def _claim_small(p):
    assert p["kernel"] == K128 and not p["fixup"] and all(f == 0 for _, _, _, f in p["xcds"]), p


def _claim_whole(kernel, most):
    def check(p):
        assert p["kernel"] == kernel and p["most"] == most and not p["fixup"], p
    return check


def _claim_k256(fs):
    def check(p):
        assert p["kernel"] == K256 and sorted(set(f for _, _, _, f in p["xcds"])) == sorted(fs) and p["fixup"] == (max(fs) >= 2), p
    return check


# name -> a check of gemm_plan's answer on 256 CUs: the path the case is named for
GEMM_CLAIMS = {
    "k128_rows_f4": _claim_k128([(40, 1, 8, 4)] * 8, 1),
    "k128_rows_f8_ragged": _claim_k128([(33, 1, 1, 8)] * 8, 1),
    "k128_cols_f8_f4": _claim_k128([(36, 1, 4, 8)] * 7 + [(8, 0, 8, 4)], 0),
    "k128_cols_f8_whole_empty": _claim_k128([(35, 1, 3, 8)] * 6 + [(28, 0, 28, 0), (0, 0, 0, 0)], 0),
    "k256_no_rem": _claim_k256([0]),
    "k256_f4_f1": _claim_k256([4, 1]),
    "k256_f2_f1": _claim_k256([2, 1]),
    "k160_min": _claim_whole(K160, 1),
    "k320_min": _claim_whole(K320, 1),
    "k160_two_tiles": _claim_whole(K160, 2),
    "k320_two_tiles": _claim_whole(K320, 2),
    "k160_transposed": _claim_whole(K160, 1),
    "small_1x4": _claim_small, "small_255x124": _claim_small, "small_256x128": _claim_small, "small_257x132": _claim_small,
}


def gemm_operands(name, kind, device="cpu", rows=None):
    """(A [M, Kp], Bt [N, Kp] bf16, bias [N] fp32) of a case.  kind "int": A in -3..3, Bt in -2..2, bias in -8..8; "gauss": 0.1 N(0, 1)
    rounded to bf16, bias N(0, 1).  Columns K.. of the operands are zero.  rows: only the first `rows` rows of A (the CPU checks)."""
    M, N, K, _, _ = GEMM_CASES[name] if isinstance(name, str) else name
    M = M if rows is None else min(M, rows)
    kp = kpad(K)
    g = torch.Generator(device=device).manual_seed(M * 31 + N * 17 + K)
    if kind == "int":
        a = torch.randint(-3, 4, (M, kp), generator=g, device=device, dtype=torch.int32).to(torch.bfloat16)
        bt = torch.randint(-2, 3, (N, kp), generator=g, device=device, dtype=torch.int32).to(torch.bfloat16)
        bias = torch.randint(-8, 9, (N,), generator=g, device=device, dtype=torch.int32).float()
    else:
        a = (0.1 * torch.randn(M, kp, generator=g, device=device)).to(torch.bfloat16)
        bt = (0.1 * torch.randn(N, kp, generator=g, device=device)).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=device)
    a[:, K:] = 0
    bt[:, K:] = 0
    return a, bt, bias


def gemm_budget(name):
    """the largest |sum| the integer pass can reach: sum_k |a| |b| + |bias|"""
    _, _, K, _, _ = GEMM_CASES[name]
    return 3 * 2 * K + 8


def act_ref(v, act):
    """mg_act in the precision of v: fmaxf, or v > 0 ? v : 0.2f * v as ONE multiply (fp32 v: the kernel's arithmetic)"""
    if act == ACT_RELU:
        return v.clamp_min(0)
    if act == ACT_LRELU2:
        return torch.where(v > 0, v, v * SLOPE)
    return v


def gemm_product(a, bt):
    """fp64 A . Bt^T on the operands' device"""
    return a.double() @ bt.double().t()


def gemm_exact(prod64, bias, act, bf16):
    """The integer pass: the fp64 product -> exactly what the kernel stores: + bias (exact), to fp32 (exact: |sum| < 2^24), the epilogue
    in fp32, the bf16 rounding.  Device tensors round through torch's cast, CPU tensors through oracle.bf16_path.bf16_round (the
    kernels' integer formula): the two must agree with the kernel."""
    v = prod64 if bias is None else prod64 + bias.double()
    v = act_ref(v.float(), act)
    if not bf16:
        return v
    return bf16_round(v).float() if v.device.type == "cpu" else v.to(torch.bfloat16).float()


def gemm_f64(prod64, bias, act):
    """The Gaussian pass: the value before the store, in fp64"""
    return act_ref(prod64 if bias is None else prod64 + bias.double(), act)


def checked_rows(M, kernel, n=64, seed=0):
    """n (or all) row indices that include 0, M - 1 and both sides of every boundary of the kernel's row tiles (as many as fit)"""
    tm = tile_rows(kernel)
    must = [0, M - 1]
    for b in range(tm, M, tm):
        must += [b - 1, b]
    must = sorted(set(r for r in must if 0 <= r < M))
    if len(must) > n:                    # more boundaries than rows to check: the first, the last and an even spread
        idx = np.unique(np.linspace(0, len(must) - 1, n).round().astype(int))
        must = [must[i] for i in idx]
    rest = np.setdiff1d(np.arange(M), must)
    extra = np.random.RandomState(seed + M).choice(rest, size=min(len(rest), n - len(must)), replace=False) if len(must) < n else []
    return torch.as_tensor(sorted(set(must) | set(int(r) for r in extra)), dtype=torch.long)


def store_bound(want, bf16):
    """per element: 2^-8 |want| (bf16 store: helpers.within_bf16_store) or 2^-23 |want| (fp32 store), + 1e-5 max |want|"""
    return want.abs() * 2.0 ** (-8 if bf16 else -23) + 1e-5 * float(want.abs().max())


def within_store(got, want, bf16, what):
    """helpers.within_bf16_store's check (bf16) or its fp32 term, on the tensors' own device; prints the worst ratio before it asserts"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if not want.numel():
        print("%s: empty" % what)
        return 0.0
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    ratio = float(((got - want).abs() / store_bound(want, bf16)).max())
    print("%s: worst |err| / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: off by %.3f x its bound" % (what, ratio)
    return ratio


# GEMM mutants: what a wrong K split would compute (the CPU test shows the integer reference tells them apart)
def gemm_mutant_omits_a_part(a, bt, bias, f, part):
    """K cut into f parts of 64-wide slices as the kernels cut it (part p = slices [p nk / f, (p + 1) nk / f)), one part left out"""
    nk = a.shape[1] // BK
    keep = torch.ones(a.shape[1], dtype=torch.bool)
    keep[part * nk // f * BK:(part + 1) * nk // f * BK] = False
    return a.double()[:, keep] @ bt.double()[:, keep].t() + bias.double()


def gemm_mutant_bias_per_part(a, bt, bias, f):
    return gemm_product(a, bt) + f * bias.double()


# ---- convolution ------------------------------------------------------------------------------------------------------------------------
def conv_case(k, stride, pad, Cin, Cout, B, H, W, res=False, relu=True, nchw=False):
    return dict(k=k, stride=stride, pad=pad, Cin=Cin, Cout=Cout, B=B, H=H, W=W, res=res, relu=relu, nchw=nchw)


def conv_id(c):
    return "k%ds%dp%d_%dto%d_B%d_%dx%d%s%s%s" % (c["k"], c["stride"], c["pad"], c["Cin"], c["Cout"], c["B"], c["H"], c["W"],
                                                 "_res" if c["res"] else "", "" if c["relu"] else "_lin", "_nchw" if c["nchw"] else "")


def conv_out_hw(c):
    return (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1


def conv_m(c):
    oh, ow = conv_out_hw(c)
    return c["B"] * oh * ow


def _conv_cases():
    cs = []
    # C_out across both tile widths (64-wide: <= 64; 128-wide above) x M around one row block, 1 x 1 kernels on a [1, 1, M] strip
    for cout in (8, 40, 64, 72, 104, 136, 264):
        for m in (1, 255, 256, 257):
            cs.append(conv_case(1, 1, 0, 64, cout, 1, 1, m, res=(m == 257), nchw=(m == 255)))
    cs.append(conv_case(1, 1, 0, 64, 4160, 1, 1, 257))              # 33 column tiles (more than an XCD's 32 workgroups), two row blocks
    cs.append(conv_case(3, 1, 1, 64, 72, 7, 3, 3))                  # one tile spans seven images
    cs.append(conv_case(3, 1, 1, 64, 72, 40, 3, 3, res=True))       # M = 360: the tile boundary falls inside image 28
    cs.append(conv_case(1, 1, 0, 64, 8, 1, 1, 256 * 35 + 3))        # 36 row blocks, one column tile
    for stride in (1, 2, 3):                                        # kernel x padding x stride on an odd x even image
        cs.append(conv_case(1, stride, 0, 64, 72, 2, 7, 8))
        for pad in (0, 1):
            cs.append(conv_case(3, stride, pad, 64, 72, 2, 7, 8))
    cs.append(conv_case(3, 2, 1, 64, 40, 2, 8, 7))                  # even x odd under stride 2
    for h, w, pad in ((1, 1, 1), (1, 5, 1), (2, 2, 1), (3, 3, 0)):  # tiny images; 3 x 3 without padding: one output pixel
        cs.append(conv_case(3, 1, pad, 64, 72, 2, h, w))
    cs.append(conv_case(3, 2, 1, 64, 72, 2, 2, 2))
    cs.append(conv_case(1, 1, 0, 128, 104, 2, 5, 5))
    cs.append(conv_case(3, 1, 1, 128, 40, 2, 5, 5))
    cs.append(conv_case(1, 1, 0, 512, 72, 2, 5, 5, res=True))
    cs.append(conv_case(3, 1, 1, 512, 72, 1, 5, 5))                 # K = 4608: 72 slices
    for cout in (40, 104):                                          # every epilogue at a C_out off the tile and M = 300
        for res in (False, True):
            for relu in (False, True):
                for nchw in (False, True):
                    cs.append(conv_case(3, 1, 1, 64, cout, 3, 10, 10, res=res, relu=relu, nchw=nchw))
    return cs


CONV_CASES = _conv_cases()


def conv_operands(c, kind, seed=0):
    """(x [B, H, W, Cin], wt [Cout, k k Cin] with k = (kh, kw, c), bias [Cout], residual [B, OH, OW, Cout] or None), fp32 CPU tensors
    that are exact in bf16 (x, wt, residual).  "int": x in -2..2, ternary wt, bias and residual in -4..4; "gauss": N(0, 1) x and
    residual, He-scaled wt, all rounded to bf16, bias 0.3 N(0, 1)."""
    rs = np.random.RandomState(1000 * c["k"] + 100 * c["stride"] + 10 * c["pad"] + c["Cin"] + 7 * c["Cout"] + 13 * c["B"] + 3 * c["H"] + c["W"] + seed)
    oh, ow = conv_out_hw(c)
    K = c["k"] * c["k"] * c["Cin"]
    xs, rshape = (c["B"], c["H"], c["W"], c["Cin"]), (c["B"], oh, ow, c["Cout"])
    if kind == "int":
        x = rs.randint(-2, 3, xs)
        wt = rs.randint(-1, 2, (c["Cout"], K))
        bias = rs.randint(-4, 5, c["Cout"])
        res = rs.randint(-4, 5, rshape) if c["res"] else None
        t = lambda v: None if v is None else torch.from_numpy(v.astype(np.float32))
        return t(x), t(wt), t(bias), t(res)
    r = lambda v: v.to(torch.bfloat16).float()
    t = lambda shape, s=1.0: torch.from_numpy((s * rs.standard_normal(shape)).astype(np.float32))
    return r(t(xs)), r(t((c["Cout"], K), (2.0 / K) ** 0.5)), t(c["Cout"], 0.3), (r(t(rshape)) if c["res"] else None)


def conv_budget(c):
    return 2 * c["k"] * c["k"] * c["Cin"] + 4 + 4


def conv_sum(x, wt, bias, c, res=None, mutant=None):
    """NHWC convolution of the kernel's formula in the precision of x, tap by tap: y[b, oh, ow, o] = sum_{kh, kw, c} x[b, oh s - p + kh,
    ow s - p + kw, c] wt[o, (kh, kw, c)] (taps outside the image are zero) + bias + residual, before the ReLU / the store.  mutant: "swap"
    (kh and kw exchanged in the pixel), "clamp" (a padded tap reads the nearest pixel instead of zero), "drop" (the last 64-wide K slice
    is left out)."""
    k, s, p, Cin = c["k"], c["stride"], c["pad"], c["Cin"]
    B, H, W, _ = x.shape
    oh, ow = conv_out_hw(c)
    if mutant == "drop":
        wt = wt.clone()
        wt[:, -64:] = 0
    y = torch.zeros(B, oh, ow, wt.shape[0], dtype=x.dtype)
    for kh in range(k):
        for kw in range(k):
            dh, dw = (kw, kh) if mutant == "swap" else (kh, kw)
            ih, iw = torch.arange(oh) * s - p + dh, torch.arange(ow) * s - p + dw
            patch = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
            if mutant != "clamp":
                ok = ((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]
                patch = patch * ok[None, :, :, None].to(x.dtype)
            tap = kh * k + kw
            y += patch @ wt[:, tap * Cin:(tap + 1) * Cin].t()
    y = y + bias
    return y if res is None else y + res


def conv_ref(x, wt, bias, c, res=None, mutant=None):
    """conv_sum in fp64"""
    return conv_sum(x.double(), wt.double(), bias.double(), c, None if res is None else res.double(), mutant)


def conv_exact(y64, c):
    """The integer pass: the fp64 sum -> what the kernel stores: fp32 (exact), fmaxf, then bf16 NHWC or fp32 NCHW"""
    v = y64.float()
    if c["relu"]:
        v = v.clamp_min(0)
    return v.permute(0, 3, 1, 2).contiguous() if c["nchw"] else bf16_round(v).float()


def conv_f64(y64, c):
    v = y64.clamp_min(0) if c["relu"] else y64
    return v.permute(0, 3, 1, 2).contiguous() if c["nchw"] else v


# ---- stem and max-pool ----------------------------------------------------------------------------------------------------------------
STEM_H, STEM_W = (7, 8, 9, 15, 16, 17), (7, 63, 64, 65, 66)      # around the 8-row and 32-column workgroup tile (16 / 64 input pixels)
POOL_HW, POOL_C = (1, 2, 3, 8, 9), (8, 72)


def stem_operands(B, H, W, kind, seed=0):
    """(img [B, 3, H, W], w [64, 3, 7, 7], conv_bias [64]) fp32.  "int": img in -4..4, ternary w, bias in -4..4; "gauss": N(0, 1) img,
    0.12 N(0, 1) w, 0.3 N(0, 1) bias (the kernel rounds img and w to bf16)."""
    rs = np.random.RandomState(97 * H + W + B + seed)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32))
    if kind == "int":
        return t(rs.randint(-4, 5, (B, 3, H, W))), t(rs.randint(-1, 2, (64, 3, 7, 7))), t(rs.randint(-4, 5, 64))
    return t(rs.standard_normal((B, 3, H, W))), t(0.12 * rs.standard_normal((64, 3, 7, 7))), t(0.3 * rs.standard_normal(64))


STEM_BUDGET = 4 * 147 + 4


def stem_sum(img, w, bias=None):
    """7 x 7 / stride 2 / pad 3 convolution in the precision of img, tap by tap, NCHW image -> NHWC [B, OH, OW, 64] (+ bias); before the
    ReLU / the store"""
    B, _, H, W = img.shape
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros(B, 3, H + 6 + 1, W + 6 + 1, dtype=img.dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = img
    y = torch.zeros(B, oh, ow, 64, dtype=img.dtype)
    for kh in range(7):
        for kw in range(7):
            patch = xp[:, :, kh:kh + 2 * oh:2, kw:kw + 2 * ow:2]
            y += torch.einsum("bchw,oc->bhwo", patch, w[:, :, kh, kw])
    return y if bias is None else y + bias


def stem_ref(img, w, bias=None):
    """stem_sum in fp64"""
    return stem_sum(img.double(), w.double(), None if bias is None else bias.double())


def pool_operands(B, H, W, C, seed=0):
    """signed bf16-exact values [B, H, W, C] fp32; channels 0..3 are negative everywhere (every window of theirs is all negative)"""
    rs = np.random.RandomState(11 * H + 5 * W + C + B + seed)
    x = rs.randint(-8, 9, (B, H, W, C)).astype(np.float32) * 0.5
    x[..., :4] = -1.0 - np.abs(x[..., :4])
    return torch.from_numpy(x)


def pool_ref(x, pad_value=float("-inf")):
    """MaxPool2d(3, 2, 1) on NHWC; pad_value 0 is the mutant that pads with zeros"""
    B, H, W, C = x.shape
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((B, H + 3, W + 3, C), pad_value, dtype=x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    y = torch.full((B, oh, ow, C), float("-inf"), dtype=x.dtype)
    for dh in range(3):
        for dw in range(3):
            y = torch.maximum(y, xp[:, dh:dh + 2 * oh:2, dw:dw + 2 * ow:2])
    return y


# ---- fold and transpose-cast ------------------------------------------------------------------------------------------------------------
def fold_operands(Cout, Cin, k, with_bn, with_bias, seed=0):
    """(w [Cout, Cin, k, k], conv_bias or None, (gamma, beta, mean, var, eps) or None).  The BatchNorm is dyadic -- var in {1/4, 1, 4},
    eps 0, gamma / beta / mean / conv_bias multiples of 1/4 -- so scale and the folded bias are exact however the kernel groups them;
    the weights are Gaussian, so w * scale -> bf16 rounds for real."""
    rs = np.random.RandomState(Cout + 3 * Cin + k + seed)
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32))
    w = t(rs.standard_normal((Cout, Cin, k, k)))
    cb = t(rs.randint(-8, 9, Cout) * 0.25) if with_bias else None
    bn = None
    if with_bn:
        bn = (t(rs.choice([-1.5, -0.5, 0.25, 0.75, 1.0, 3.0], Cout)), t(rs.randint(-8, 9, Cout) * 0.25), t(rs.randint(-8, 9, Cout) * 0.25),
              t(rs.choice([0.25, 1.0, 4.0], Cout)), 0.0)
    return w, cb, bn


def fold_ref(w, cb, bn, stem=False, ld=None):
    """conv_fold_bn_kernel in fp32 on the CPU -> (bf16 values [Cout, ld] as fp32, bias [Cout] fp32)"""
    Cout, Cin, KH, KW = w.shape
    scale = torch.ones(Cout) if bn is None else bn[0] / torch.sqrt(bn[3] + np.float32(bn[4]))
    ws = w * scale[:, None, None, None]
    flat = ws.reshape(Cout, -1) if stem else ws.permute(0, 2, 3, 1).reshape(Cout, -1)
    ld = flat.shape[1] if ld is None else ld
    wt = torch.zeros(Cout, ld)
    wt[:, :flat.shape[1]] = bf16_round(flat).float()
    c = torch.zeros(Cout) if cb is None else cb
    return wt, (c if bn is None else bn[1] + (c - bn[2]) * scale)


def finite_specials():
    """the fp32 values of helpers.BF16_SPECIALS that are finite: ties, one bit either side, zeros, denormals, the largest values"""
    from tests.helpers import BF16_SPECIALS
    v = BF16_SPECIALS.view(np.float32)
    return v[np.isfinite(v)]
