"""The measuring stick of tests/test_matrix_pipe_edges_gpu.py, checked without a GPU (tests/matrix_pipe_cases.py): the launcher
restatement against the library's own host arithmetic, the path every GEMM case is named for, the exactness budget of the integer
pass, the references against torch in double, the entry points' constraints, and mutants -- wrong kernels the cases must catch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import _lib
from tests import helpers as H
from tests import matrix_pipe_cases as C


def _bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def test_the_restated_pick_is_the_librarys():
    """gemm_pick (default form) == mgnns_gemm_bf16_pick_form over a grid of shapes round every threshold of mg_gemm_pick, with and
    without the workspace, on 256 CUs and two other device sizes; and every case's shape."""
    L = _lib.lib()
    Ms = (1, 255, 256, 1120, 1121, 2240, 2241, 2560, 2600, 5000, 8191, 8192, 8300, 10000, 16500, 20154)
    Ns = (4, 128, 252, 256, 260, 516, 1024, 1200, 2048, 2312, 5120, 10000)
    Ks = (64, 256, 320, 704, 1024, 2048, 4032, 4096, 4160, 10048)
    shapes = [(M, N, K) for M in Ms for N in Ns for K in Ks] + [(M, N, C.kpad(K)) for M, N, K, _, _ in C.GEMM_CASES.values()]
    seen = set()
    for M, N, Kp in shapes:
        for ws in (0, 1):
            for cu in (256, 304, 64):
                want = L.mgnns_gemm_bf16_pick_form(M, N, Kp, ws, cu)
                got = C.pick_form_code(C.gemm_pick(M, N, Kp, ws, cu, form=2))
                assert got == want, (M, N, Kp, ws, cu, got, want)
                seen.add(want)
    assert seen == {0, 4, 5}
    assert C.WORKSPACE_BYTES == L.mgnns_gemm_bf16_workspace_bytes()


def test_every_gemm_case_reaches_the_path_it_names_on_256_cus():
    """Through the restatement (mg_gemm_pick, mg_gemm_split, gemm256_split, the launcher's map choice): each case of GEMM_CASES runs the
    kernel, the tile map and the K split written next to it -- every kernel, both maps of the 256 x 128 kernel, f in {0, 4, 8}, a split with
    no full round before it, an XCD with whole tiles only and an empty XCD, f in {0, 1, 2, 4} of the 256 x 256 kernel, one and two tiles
    per workgroup of the whole-tile kernels.  Without the workspace no case splits."""
    assert set(C.GEMM_CLAIMS) == set(C.GEMM_CASES)
    for name, claim in C.GEMM_CLAIMS.items():
        claim(C.case_plan(name))
        off = C.case_plan(name, ws=False)
        assert not off["fixup"] and off["kernel"] != C.K256, (name, off)
    kernels = {C.case_plan(n)["kernel"] for n in C.GEMM_CASES}
    assert kernels == {C.K128, C.K256, C.K160, C.K320}
    for name in C.SPLIT_CASES:
        assert C.case_plan(name)["fixup"], name
    # the shapes tests/test_ops_gpu.py relies on: its K-split test at form 0, its 256 x 256 test at form 0
    for M, N, K in ((2048, 5120, 2048), (1800, 4100, 4096), (1024, 8320, 4096), (1792, 4300, 4096)):
        p = C.gemm_plan(M, N, C.kpad(K), True, form=0)
        assert p["kernel"] == C.K128 and any(f > 0 for _, _, _, f in p["xcds"]), (M, N, K, p)
    for M, N, K, split in ((8192, 2048, 4096, False), (10000, 2048, 4200, True), (8300, 2312, 4100, True)):
        p = C.gemm_plan(M, N, C.kpad(K), True, form=0)
        assert p["kernel"] == C.K256 and any(f >= 2 for _, _, _, f in p["xcds"]) == split, (M, N, K, p)
    # ... and what the issue found: by the default form these shapes never reached the kernels their tests name
    assert C.gemm_pick(10000, 1024, 320, True) == C.K160 and C.gemm_pick(10000, 2048, 4224, True) == C.K320
    assert not C.gemm_plan(10000, 1024, 320, True, form=0)["fixup"]          # five slices: a part needs eight


def test_gemm_cases_obey_the_entry_point_and_their_budget():
    for name, (M, N, K, form, c_tr) in C.GEMM_CASES.items():
        assert M > 0 and N % 4 == 0 and form in (0, 1, 3)
        assert not c_tr or C.gemm_fits(M, N, C.kpad(K), C.TM160)
        assert C.gemm_budget(name) < C.EXACT
        a, bt, bias = C.gemm_operands((min(M, 256), min(N, 256), K, form, c_tr), "int")         # (a corner: the generator is the same)
        assert a.shape[1] == bt.shape[1] == C.kpad(K) and a.shape[1] % 64 == 0
        assert float(a.float().abs().max()) <= 3 and float(bt.float().abs().max()) <= 2 and float(bias.abs().max()) <= 8
        assert _bf16_exact(a) and _bf16_exact(bt) and torch.equal(bias, bias.round())
        assert not a[:, K:].any() and not bt[:, K:].any()
        assert len(a.float().unique()) == 7 and len(bt.float().unique()) == 5
        if M * N < 1 << 20:
            g, gt, _ = C.gemm_operands(name, "gauss")
            assert _bf16_exact(g) and g.dtype == torch.bfloat16 and not g[:, K:].any() and not gt[:, K:].any()
        rows = C.checked_rows(M, C.case_plan(name)["kernel"])
        tm = C.tile_rows(C.case_plan(name)["kernel"])
        assert len(rows) == min(M, 64) and rows[0] == 0 and rows[-1] == M - 1 and len(set(rows.tolist())) == len(rows)
        if (M - 1) // tm <= 31:                         # every boundary fits into 64 rows
            for b in range(tm, M, tm):
                assert b - 1 in rows and b in rows, (name, b)


def test_gemm_reference_and_mutants():
    """The integer reference equals torch's own fp64 / fp32 arithmetic, and tells a K split that omits a part or adds the bias once
    per part from the right one -- for every part count the cases reach, on every checked row."""
    a, bt, bias = C.gemm_operands((70, 132, 4100, 0, False), "int")
    prod = C.gemm_product(a, bt)
    assert torch.equal(prod, (a.float() @ bt.float().t()).double())          # exact in fp32 as well
    for act in (C.ACT_NONE, C.ACT_RELU, C.ACT_LRELU2):
        want = C.gemm_exact(prod, bias, act, False)
        v = (prod + bias.double()).float()
        assert torch.equal(want, {0: v, 1: F.relu(v), 2: torch.where(v > 0, v, v * np.float32(0.2))}[act])
        assert torch.equal(C.gemm_exact(prod, bias, act, True), want.to(torch.bfloat16).float())
    assert not torch.equal(C.gemm_exact(prod, bias, C.ACT_LRELU2, True), C.gemm_exact(prod, bias, C.ACT_LRELU2, False))   # the store rounds
    want = prod + bias.double()
    for f in (2, 4, 8):
        for part in range(f):
            bad = C.gemm_mutant_omits_a_part(a, bt, bias, f, part)
            assert (bad != want).any(dim=1).all(), (f, part)                  # every row shows it
        assert (C.gemm_mutant_bias_per_part(a, bt, bias, f) != want).any(dim=1).all()
    # the Gaussian pass would see them too: a missing part is far outside the fp32 bound
    g, gt, gb = C.gemm_operands((70, 132, 4100, 0, False), "gauss")
    ref = C.gemm_f64(C.gemm_product(g, gt), gb, C.ACT_NONE)
    C.within_store(ref.float(), ref, False, "fp32 store of the fp64 value")
    with pytest.raises(AssertionError):
        C.within_store(C.gemm_mutant_omits_a_part(g, gt, gb, 8, 3), ref, False, "mutant")


def test_within_store_is_the_projects_bound():
    rs = np.random.RandomState(5)
    want = torch.from_numpy(rs.standard_normal((40, 50)))
    for got in (C.bf16_round(want), C.bf16_round(want) * (1 + 2.0 ** -7)):
        verdicts = []
        for check in (lambda: H.within_bf16_store(got, want, "helper"), lambda: C.within_store(got, want, True, "cases")):
            try:
                check()
                verdicts.append(True)
            except AssertionError:
                verdicts.append(False)
        assert verdicts[0] == verdicts[1]
    assert float(C.store_bound(want, False).min()) >= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("c", C.CONV_CASES, ids=C.conv_id)
def test_conv_case_is_legal_exact_and_the_reference_is_conv2d(c):
    assert c["Cin"] >= 64 and c["Cin"] & (c["Cin"] - 1) == 0 and c["Cout"] % 8 == 0 and c["stride"] >= 1
    assert (c["k"], c["pad"]) in ((1, 0), (3, 0), (3, 1)) and min(C.conv_out_hw(c)) > 0
    assert C.conv_budget(c) < C.EXACT
    for kind in ("int", "gauss"):
        x, wt, bias, res = C.conv_operands(c, kind)
        assert _bf16_exact(x) and _bf16_exact(wt) and (res is None or _bf16_exact(res)) and (res is not None) == c["res"]
        if kind == "int":
            assert float(x.abs().max()) <= 2 and float(wt.abs().max()) <= 1 and float(bias.abs().max()) <= 4
            assert res is None or float(res.abs().max()) <= 4
        if C.conv_m(c) * c["Cout"] * c["Cin"] > 5e7 and kind == "gauss":
            continue                                                       # (the big strips: one comparison is enough)
        w4 = wt.reshape(c["Cout"], c["k"], c["k"], c["Cin"]).permute(0, 3, 1, 2)
        want = F.conv2d(x.permute(0, 3, 1, 2).double(), w4.double(), bias.double(), c["stride"], c["pad"]).permute(0, 2, 3, 1)
        if res is not None:
            want = want + res.double()
        got = C.conv_ref(x, wt, bias, c, res)
        if kind == "int":
            assert torch.equal(got, want) and float(got.abs().max()) <= C.conv_budget(c)
        else:
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_conv_cases_cover_what_they_are_for():
    cs = C.CONV_CASES
    assert len({C.conv_id(c) for c in cs}) == len(cs)
    assert {c["Cout"] for c in cs} >= {8, 40, 64, 72, 104, 136, 264, 4160}
    for cout in (8, 40, 64, 72, 104, 136, 264):
        assert {C.conv_m(c) for c in cs if c["Cout"] == cout and c["k"] == 1} >= {1, 255, 256, 257}
    assert {(c["k"], c["pad"], c["stride"]) for c in cs} >= {(1, 0, 1), (1, 0, 2), (1, 0, 3)} | {(3, p, s) for p in (0, 1) for s in (1, 2, 3)}
    assert {c["Cin"] for c in cs} == {64, 128, 512} and any(c["k"] == 3 and c["Cin"] == 512 for c in cs)
    assert {(c["H"], c["W"], c["pad"]) for c in cs if c["k"] == 3} >= {(1, 1, 1), (1, 5, 1), (2, 2, 1), (3, 3, 0)}
    assert any(C.conv_m(c) == 256 * 35 + 3 and c["Cout"] == 8 for c in cs)
    assert any(c["B"] == 7 and c["H"] == 3 for c in cs) and any(c["B"] == 40 and (256 % 9) for c in cs)
    for cout in (40, 104):
        combos = {(c["res"], c["relu"], c["nchw"]) for c in cs if c["Cout"] == cout and C.conv_m(c) == 300}
        assert len(combos) == 8


def test_conv_mutants_fail():
    """A convolution with kh and kw exchanged, one that clamps a padded tap, one that drops its last K slice: each differs from the
    integer reference on the cases meant to catch it (3 x 3 for the first two, padded for the second)."""
    for c in C.CONV_CASES:
        if C.conv_m(c) > 400 or c["Cout"] > 300:
            continue
        x, wt, bias, res = C.conv_operands(c, "int")
        want = C.conv_exact(C.conv_ref(x, wt, bias, c, res), dict(c, relu=False))
        differs = lambda m: not torch.equal(C.conv_exact(C.conv_ref(x, wt, bias, c, res, mutant=m), dict(c, relu=False)), want)
        if c["k"] == 1 or c["pad"] == 0 or min(c["H"], c["W"]) >= 2:           # (else the last tap is padding everywhere)
            assert differs("drop"), C.conv_id(c)
        if c["k"] == 3 and (c["H"] >= 3 or c["W"] >= 3):
            assert differs("swap"), C.conv_id(c)
        if c["k"] == 3 and c["pad"] == 1 and max(c["H"], c["W"]) > 1:
            assert differs("clamp"), C.conv_id(c)


def test_stem_and_pool_references_and_the_pool_mutant():
    assert min(C.STEM_H + C.STEM_W) >= 7 and all(c > 0 and c % 8 == 0 for c in C.POOL_C) and min(C.POOL_HW) > 0      # the entry points' limits
    for Hh, Ww in ((7, 7), (8, 63), (9, 66), (17, 64)):
        for kind in ("int", "gauss"):
            img, w, b = C.stem_operands(2, Hh, Ww, kind)
            got = C.stem_ref(img, w, b)
            want = F.conv2d(img.double(), w.double(), b.double(), 2, 3).permute(0, 2, 3, 1)
            assert tuple(got.shape) == (2, (Hh - 1) // 2 + 1, (Ww - 1) // 2 + 1, 64)
            if kind == "int":
                assert torch.equal(got, want) and float(got.abs().max()) <= C.STEM_BUDGET < C.EXACT
                assert _bf16_exact(img) and _bf16_exact(w) and float(img.abs().max()) <= 4
            else:
                assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    caught = 0
    for Hh in C.POOL_HW:
        for Ww in C.POOL_HW:
            for Cc in C.POOL_C:
                x = C.pool_operands(2, Hh, Ww, Cc)
                assert _bf16_exact(x) and float(x[..., :4].max()) < 0 and float(x[..., 4:].abs().max()) > 0
                want = F.max_pool2d(x.permute(0, 3, 1, 2).double(), 3, 2, 1).permute(0, 2, 3, 1).float()
                assert torch.equal(C.pool_ref(x), want)
                zero = C.pool_ref(x, 0.0)
                assert not torch.equal(zero, want), (Hh, Ww, Cc)             # every case has a border window that is all negative
                caught += 1
    assert caught == len(C.POOL_HW) ** 2 * len(C.POOL_C)


def test_fold_reference_is_exact_in_its_bias():
    """The dyadic BatchNorm of fold_operands: scale and the folded bias come out the same in fp32 and in fp64 (no rounding anywhere),
    so a kernel may group or fuse the bias arithmetic as it likes and must still match bit for bit."""
    for with_bn in (False, True):
        for with_bias in (False, True):
            w, cb, bn = C.fold_operands(72, 64, 3, with_bn, with_bias)
            wt, bias = C.fold_ref(w, cb, bn, ld=3 * 3 * 64 + 24)
            assert tuple(wt.shape) == (72, 600) and not wt[:, 576:].any() and _bf16_exact(wt)
            if bn is not None:
                scale = bn[0].double() / torch.sqrt(bn[3].double())
                c = torch.zeros(72).double() if cb is None else cb.double()
                assert torch.equal(bias.double(), bn[1].double() + (c - bn[2].double()) * scale)
                assert torch.equal(wt[:, :576].double(), C.bf16_round((w.double() * scale[:, None, None, None]).float().permute(0, 2, 3, 1).reshape(72, -1)))
    v = C.finite_specials()
    assert len(v) >= 18 and np.isfinite(v).all()
