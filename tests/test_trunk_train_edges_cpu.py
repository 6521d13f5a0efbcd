"""The measuring stick of tests/test_trunk_train_edges_gpu.py, checked without a GPU (tests/trunk_train_cases.py): the restated host
arithmetic against the library's own workspace functions over grids of shapes, the split every case is named for, each case's legality
and exactness budget, the fp64 references against torch's own gradients in double, and mutants -- wrong kernels the cases must catch."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from mgnns_amd import _lib
from tests import trunk_train_cases as C


def _bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def _nchw(t):
    return t.double().permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _conv(family, name, kind):
    """(case, operands) of a convolution case, drawn once"""
    c = (C.WGRAD_CASES if family == "wgrad" else C.DGRAD_CASES)[name]
    return c, C.conv_operands(c, kind)


# ---- the restatements are the library's -------------------------------------------------------------------------------------------------
def test_the_restated_splits_are_the_librarys():
    """wgrad_shares, stem_wgrad_split, bn_plan and conv_train_geometry, through the four workspace functions, over grids that cross
    every threshold (one step, WG_SHARE_MIN, the want = 1024 / tiles cap, 256 stem workgroups, BN's 16 rows per thread and 256 slabs),
    refused and empty shapes included (0 on both sides), and every case of the sweep."""
    L = _lib.lib()
    seen = set()
    strips = (1, 31, 32, 33, 511, 512, 513, 1024, 1025, 2049, 7681, 20000, 600001)
    for Cin, Cout, k in ((64, 64, 1), (64, 64, 3), (128, 256, 3), (512, 512, 3), (512, 2048, 1), (2048, 512, 1), (64, 2048, 3), (96, 64, 1), (64, 32, 1)):
        for stride in (1, 2, 3):
            for pad in (0, 1, 2):
                for B, H in ((1, 1), (3, 2), (0, 4)):
                    for W in strips:
                        want = L.mgnns_conv_wgrad_workspace_bytes(B, H, W, Cin, Cout, k, k, stride, pad)
                        assert C.wgrad_workspace_bytes(B, H, W, Cin, Cout, k, stride, pad) == want, (B, H, W, Cin, Cout, k, stride, pad)
                        if want:
                            seen.add(want // ((Cout * k * k * Cin + Cout) * 4))
    assert seen >= {2, 3, 4, 5, 16} and 512 < max(seen) <= 1024               # share counts up to the cap of a single tile
    assert L.mgnns_conv_wgrad_workspace_bytes(1, 4, 4, 64, 64, 1, 3, 1, 0) == 0          # a 1 x 3 kernel
    for c in C.WGRAD_CASES.values():
        args = (c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["k"], c["stride"], c["pad"])
        assert C.wgrad_workspace_bytes(*args[:6], *args[7:]) == L.mgnns_conv_wgrad_workspace_bytes(*args)
    tpws = set()
    for B in (0, 1, 2, 4, 87, 300):
        for H in (6, 7, 15, 16, 17, 200):
            for W in (6, 7, 63, 64, 65, 66, 129, 300):
                assert C.stem_wgrad_workspace_bytes(B, H, W) == L.mgnns_stem_wgrad_workspace_bytes(B, H, W), (B, H, W)
                if B and H >= 7 and W >= 7:
                    tpws.add(C.stem_wgrad_split(B, *C.stem_out_hw(H, W))[3])
    assert tpws >= {1, 2, 3}
    slabs = set()
    for M in (1, 2, 3, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1029, 4095, 4096, 4097, 8194, 100000, 1 << 20, 5000001):
        for Cc in (0, 8, 12, 16, 24, 64, 72, 256, 264, 512, 2048, 4096):
            assert C.bn_workspace_bytes(M, Cc, False) == L.mgnns_bn_stats_workspace_bytes(M, Cc), (M, Cc)
            assert C.bn_workspace_bytes(M, Cc, True) == L.mgnns_bn_backward_workspace_bytes(M, Cc), (M, Cc)
            if M >= 2 and Cc and Cc % 8 == 0:
                slabs.add(C.bn_plan(M, Cc, True)["nslab"])
    assert slabs >= {1, 2, 17, 256}


def test_every_case_reaches_the_split_it_names():
    assert set(C.WGRAD_CLAIMS) == set(C.WGRAD_CASES) and set(C.DGRAD_CLAIMS) == set(C.DGRAD_CASES)
    for name, c in C.WGRAD_CASES.items():
        assert C.wgrad_plan(c) == C.WGRAD_CLAIMS[name], (name, C.wgrad_plan(c))
    shares = {n: C.WGRAD_CLAIMS[n] for n in C.WGRAD_CASES}
    assert shares["odd_m25_one_share"][2] % 2 == 1 and shares["two_shares_odd_last"][2] % 2 == 1
    assert shares["three_shares_boundary_in_a_row"][1] % 41 != 0 and (2 * shares["three_shares_boundary_in_a_row"][1]) % 41 != 0
    assert C.wgrad_want(512, 4608) == 1 and C.out_m(C.WGRAD_CASES["cap_want1_3x3_512"]) > C.WG_SHARE_MIN
    c = C.WGRAD_CASES["cap_want4_512to2048"]
    assert C.wgrad_want(2048, 512) == 4 < C.ceil_div(C.out_m(c), C.WG_SHARE_MIN)        # the cap, not the pixels, sets the count
    assert {(c["Cin"], c["stride"]) for c in C.WGRAD_CASES.values() if c["k"] == 3} >= {(256, 1), (256, 2), (512, 1), (512, 2)}
    assert {(c["stride"], c["pad"]) for c in C.WGRAD_CASES.values() if c["k"] == 3} >= {(1, 0), (2, 0), (1, 1), (2, 1)}
    assert any(c["H"] == 1 and c["k"] == 3 for c in C.WGRAD_CASES.values()) and any(c["W"] == 1 and c["k"] == 3 for c in C.WGRAD_CASES.values())
    assert min(C.out_m(c) for c in C.WGRAD_CASES.values()) < 32
    for name, c in C.DGRAD_CASES.items():
        assert (C.in_m(c), C.ceil_div(C.in_m(c), 128)) == C.DGRAD_CLAIMS[name], name
    assert {C.in_m(c) for c in C.DGRAD_CASES.values()} >= {1, 127, 128, 129}
    assert {(c["k"], c["stride"], c["pad"]) for c in C.DGRAD_CASES.values()} == {(1, 1, 0), (1, 2, 0), (3, 1, 0), (3, 1, 1), (3, 2, 0), (3, 2, 1)}
    assert {c["Cout"] for c in C.DGRAD_CASES.values()} >= {64, 2048} and {c["Cin"] for c in C.DGRAD_CASES.values()} >= {64, 2048}
    c = C.DGRAD_CASES["k3_128to256_tile_spans_images"]
    assert 128 % (c["H"] * c["W"]) != 0 and c["B"] * c["H"] * c["W"] > 128
    assert set(C.STEM_CLAIMS) == set(C.STEM_CASES)
    for name, (B, H, W) in C.STEM_CASES.items():
        assert C.stem_wgrad_split(B, *C.stem_out_hw(H, W)) == C.STEM_CLAIMS[name], (name, C.stem_wgrad_split(B, *C.stem_out_hw(H, W)))
    B, H, W = C.STEM_CASES["two_tiles_per_workgroup_across_images"]
    ntr, ntc, ntiles, tpw, nwg = C.STEM_CLAIMS["two_tiles_per_workgroup_across_images"]
    assert tpw == 2 and (ntr * ntc) % tpw == 1 and ntiles % tpw == 1          # runs cross images, and the last workgroup has one tile
    assert {C.stem_out_hw(H, W) for _, H, W in C.STEM_CASES.values()} >= {(4, 4), (8, 32), (9, 33)}
    for (H, W), claim in C.POOL_CLAIMS.items():
        for Cc in C.POOL_C:
            assert C.pool_bwd_tiles(2, H, W, Cc) == claim + (C.POOL_NCB[Cc], 2 * claim[0] * claim[1] * C.POOL_NCB[Cc]), (H, W, Cc)
    assert set(C.POOL_CLAIMS) == set(C.POOL_HW)
    assert set(C.BN_CLAIMS) == set(C.BN_CASES)
    for name, (shape, kinds) in C.BN_CASES.items():
        assert C.bn_plan_tuple(*C.bn_mc(shape)) == C.BN_CLAIMS[name], (name, C.bn_plan_tuple(*C.bn_mc(shape)))
    assert C.BN_CLAIMS["odd_last_slab"][5] % 2 == 1 and C.BN_CLAIMS["slabs17_last_of_2_rows"][3] > 16
    assert {C.bn_mc(s)[1] for s, _ in C.BN_CASES.values()} >= {8, 24, 72} and any(C.bn_mc(s)[0] == 2 for s, _ in C.BN_CASES.values())


# ---- legality, budgets, references ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name", [("wgrad", n) for n in C.WGRAD_CASES] + [("dgrad", n) for n in C.DGRAD_CASES])
def test_conv_case_is_legal_exact_and_the_references_are_torchs(family, name):
    c, o = _conv(family, name, "int")
    assert C.conv_train_geometry(c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["k"], c["stride"], c["pad"]) == C.out_hw(c)
    assert max(C.wgrad_budget(c), C.dgrad_budget(c)) < C.EXACT
    assert all(_bf16_exact(t) for t in o.values()) and all(_bf16_exact(t) for t in C.conv_operands(c, "gauss").values())
    assert float(o["x"].abs().max()) <= 4 and float(o["dy"].abs().max()) <= 4 and float(o["wt"].abs().max()) <= 4 and float(o["add"].abs().max()) <= 8
    dead = o["mask"][~(o["mask"] > 0)]
    assert bool(torch.signbit(dead[dead == 0]).any()) and bool((dead < 0).any()) or dead.numel() < 64
    kw = dict(stride=c["stride"], padding=c["pad"])
    w4 = o["wt"].double().reshape(c["Cout"], c["k"], c["k"], c["Cin"]).permute(0, 3, 1, 2).contiguous()
    if family == "wgrad":
        dW, db = C.wgrad_ref(o["x"], o["dy"], c)
        want = conv2d_weight(_nchw(o["x"]), w4.shape, _nchw(o["dy"]), **kw).permute(0, 2, 3, 1).reshape(c["Cout"], -1)
        assert torch.equal(dW, want) and torch.equal(db, o["dy"].double().sum(dim=(0, 1, 2)))
        assert float(dW.abs().max()) <= C.wgrad_budget(c) and float(dW.abs().max()) > 0
        assert torch.equal(dW, C.wgrad_sum(o["x"], o["dy"], c)[0].double())             # the integer sums are exact in fp32 too
    else:
        acc = C.dgrad_sum(o["dy"].double(), o["wt"].double(), c)
        want = conv2d_input((c["B"], c["Cin"], c["H"], c["W"]), w4, _nchw(o["dy"]), **kw).permute(0, 2, 3, 1)
        assert torch.equal(acc, want) and torch.equal(acc, C.dgrad_gather(o["dy"].double(), o["wt"].double(), c))
        assert float(acc.abs().max()) + 8 <= C.dgrad_budget(c)
        assert torch.equal(C.transpose_pack_ref(o["wt"], c["k"] ** 2).reshape(c["Cin"], c["k"], c["k"], c["Cout"]).permute(3, 1, 2, 0).reshape(c["Cout"], -1), o["wt"])
        full = C.dgrad_ref(o, c, True, True)
        assert bool((full[~(o["mask"] > 0)] == 0).all()) and torch.equal(full[o["mask"] > 0], (acc + o["add"].double())[o["mask"] > 0])
        g = C.conv_operands(c, "gauss")
        got = C.dgrad_sum(g["dy"].double(), g["wt"].double(), c)
        w4g = g["wt"].double().reshape(c["Cout"], c["k"], c["k"], c["Cin"]).permute(0, 3, 1, 2).contiguous()
        want = conv2d_input((c["B"], c["Cin"], c["H"], c["W"]), w4g, _nchw(g["dy"]), **kw).permute(0, 2, 3, 1)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_conv_mutants_differ_on_the_cases_built_for_them():
    """On integer operands: a weight gradient that drops the last pixel of a share or swaps the pixels of a pair (every case), that
    clamps a padding tap (3 x 3 with padding) or ignores the channel offset inside a tap (C_in > 64); a data gradient without the
    divisibility test (stride 2), with (kh, kw) swapped (3 x 3) or with add applied after the mask (every case)."""
    caught = {m: 0 for m in C.WGRAD_MUTANTS + C.DGRAD_MUTANTS}
    for name, c in C.WGRAD_CASES.items():
        if C.out_m(c) * c["Cout"] * C.kdim(c) > 3e8:
            continue                                                       # (the big shapes: their small neighbours stand for them)
        _, o = _conv("wgrad", name, "int")
        want = C.wgrad_ref(o["x"], o["dy"], c)
        for m in C.WGRAD_MUTANTS:
            applies = {"drop_last": True, "swap_pair": C.out_m(c) > 1, "clamp": c["k"] == 3 and c["pad"] == 1, "ignore_c0": c["Cin"] > 64}[m]
            bad = C.wgrad_ref(o["x"], o["dy"], c, m)
            assert torch.equal(bad[0], want[0]) != applies, (name, m)
            caught[m] += applies
        assert not torch.equal(C.wgrad_ref(o["x"], o["dy"], c, "drop_last")[1], want[1]), name        # db' loses the pixel too
    for name in ("two_shares_odd_last", "three_shares_boundary_in_a_row", "three_shares_3x3", "k3_cin256_s1", "k3_cin256_s2", "k3_cin512_s2"):
        assert C.out_m(C.WGRAD_CASES[name]) * C.WGRAD_CASES[name]["Cout"] * C.kdim(C.WGRAD_CASES[name]) <= 3e8, name
    for name, c in C.DGRAD_CASES.items():
        _, o = _conv("dgrad", name, "int")
        want = C.dgrad_ref(o, c, True, True)
        for m in C.DGRAD_MUTANTS:
            applies = {"no_divisibility": c["stride"] == 2, "swap_taps": c["k"] == 3, "add_after_mask": True}[m]
            differs = not torch.equal(bf16_of(C.dgrad_ref(o, c, True, True, m)), bf16_of(want))
            assert differs == applies, (name, m)
            caught[m] += applies
    assert all(n >= 2 for n in caught.values()), caught


def bf16_of(v64):
    """what the integer pass compares: the exact value rounded once"""
    return C.bf16_round(v64.float())


def test_pack_unfold_and_map_cases():
    for Cout, Cin, k in C.PACK_CASES:
        wt = torch.arange(Cout * k * k * Cin, dtype=torch.float32).reshape(Cout, -1)
        wT = C.transpose_pack_ref(wt, k * k)
        assert tuple(wT.shape) == (Cin, k * k * Cout)
        for o, tap, ci in ((0, 0, 0), (Cout - 1, k * k - 1, Cin - 1), (Cout // 2, (k * k) // 2, Cin // 3)):
            assert wT[ci, tap * Cout + o] == wt[o, tap * Cin + ci]
    assert any(Cout % 8 and Cin % 8 for Cout, Cin, k in C.PACK_CASES) and any(Cout & (Cout - 1) and Cin & (Cin - 1) for Cout, Cin, k in C.PACK_CASES)
    for Cout, Cin, k in C.UNFOLD_CASES:
        o = C.unfold_operands(Cout, Cin, k)
        d = {n: (v.double().requires_grad_(n in ("w", "gamma")) if torch.is_tensor(v) else v) for n, v in o.items()}
        # the folded pair as the forward forms it: w' = w gamma r in (kh, kw, c) order, b' = beta - mean gamma r (beta drops out of dgamma)
        r = 1.0 / torch.sqrt(d["var"] + d["eps"])
        wp = (d["w"] * (d["gamma"] * r)[:, None, None, None]).permute(0, 2, 3, 1).reshape(Cout, -1)
        bp = -d["mean"] * d["gamma"] * r
        ((wp * d["dwp"]).sum() + (bp * d["dbp"]).sum()).backward()
        dW, dg, dbeta, mag = C.unfold_sum(*(o[n].double() if torch.is_tensor(o[n]) else o[n] for n in ("w", "dwp", "dbp", "gamma", "mean", "var", "eps")))
        assert float((dW - d["w"].grad).abs().max()) <= 1e-12 * float(dW.abs().max())
        assert float((dg - d["gamma"].grad).abs().max()) <= 1e-12 * float(mag.max()) and torch.equal(dbeta, o["dbp"].double())
    assert {c[1] for c in C.MAP_CASES} >= {8, 72} and any(c[1] == 72 and c[2] * c[3] == 1 for c in C.MAP_CASES)
    assert any(c[1] == 72 and (c[2] * c[3]) % 2 == 1 and c[2] * c[3] > 1 for c in C.MAP_CASES)
    for case in C.MAP_CASES:
        fmap, dmap = C.map_operands(*case)
        zeros = fmap[fmap == 0]
        assert bool(torch.signbit(zeros).any()) and bool((~torch.signbit(zeros)).any()) and bool((fmap < 0).any()) or fmap.numel() < 64
        want = C.map_grad_ref(fmap, dmap)
        assert tuple(want.shape) == (case[0], case[2], case[3], case[1]) and bool((want[(fmap <= 0).permute(0, 2, 3, 1)] == 0).all())
        assert torch.equal(want.float(), torch.where(fmap > 0, dmap, torch.zeros(())).permute(0, 2, 3, 1).to(torch.bfloat16).float())


@pytest.mark.parametrize("name", list(C.STEM_CASES))
def test_stem_case_is_legal_exact_and_the_reference_is_torchs(name):
    B, H, W = C.STEM_CASES[name]
    assert H >= 7 and W >= 7 and C.stem_budget(B, H, W) < C.EXACT
    img, g = C.stem_operands(B, H, W, "int")
    assert _bf16_exact(img) and _bf16_exact(g) and 128 < float(img.abs().max()) <= 256 and float(g.abs().max()) == 1
    dW, db = C.stem_wgrad_sum(img.double(), g.double())
    want = conv2d_weight(img.double(), (64, 3, 7, 7), _nchw(g), stride=2, padding=3).permute(0, 2, 3, 1).reshape(64, 147)
    assert torch.equal(dW, want) and torch.equal(db, g.double().sum(dim=(0, 1, 2))) and float(dW.abs().max()) <= C.stem_budget(B, H, W)
    assert torch.equal(C.stem_wgrad_sum(img, g)[0].double(), dW)                                # exact in fp32 in this order too
    if B <= 2:
        img, g = C.stem_operands(B, H, W, "gauss")
        assert _bf16_exact(g) and not _bf16_exact(img)
        x = C.rbf(img).double()
        want = conv2d_weight(x, (64, 3, 7, 7), _nchw(g), stride=2, padding=3).permute(0, 2, 3, 1).reshape(64, 147)
        assert float((C.stem_wgrad_sum(x, g.double())[0] - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("hw", C.POOL_HW, ids=lambda s: "%dx%d" % s)
def test_pool_reference_is_autograd_and_the_mutants_differ(hw):
    H, W = hw
    for Cc in C.POOL_C:
        assert Cc % 8 == 0
        for tied in (True, False):
            x, gy = C.pool_operands(2, H, W, Cc, tied, "int")
            assert _bf16_exact(x) and _bf16_exact(gy) and float(gy.abs().max()) <= 8 and 4 * 8 < C.EXACT
            x64 = _nchw(x).requires_grad_(True)
            (F.max_pool2d(x64, 3, 2, 1) * _nchw(gy)).sum().backward()
            want = x64.grad.permute(0, 2, 3, 1)
            assert torch.equal(C.pool_bwd_sum(x.double(), gy.double(), False), want), (H, W, Cc, tied)
            masked = C.pool_bwd_sum(x.double(), gy.double(), True)
            assert torch.equal(masked, want * (x > 0)) and bool((masked[x <= 0] == 0).all())
            assert float(C.pool_window_sum(gy.abs().double(), H, W).min()) >= 0 and bool((want.abs() <= C.pool_window_sum(gy.abs().double(), H, W)).all())
            for m in C.POOL_MUTANTS:
                applies = {"last_maximum": tied and H * W > 1, "loses_window_below": H > C.PB_ROWS, "loses_window_right": W > C.PB_COLS}[m]
                if m == "last_maximum" and not tied:
                    continue                                               # (bf16 Gaussians tie now and then: no claim either way)
                assert torch.equal(C.pool_bwd_sum(x.double(), gy.double(), False, m), want) != applies, (H, W, Cc, tied, m)


@pytest.mark.parametrize("name", list(C.BN_CASES))
def test_bn_case_is_legal_exact_and_the_references_are_autograd(name):
    shape, kinds = C.BN_CASES[name]
    M, Cc = C.bn_mc(shape)
    assert Cc % 8 == 0 and M >= 2 and ("int" not in kinds or M % 2 == 0)
    for kind in kinds:
        o = C.bn_operands(shape, kind)
        assert all(_bf16_exact(o[n]) for n in ("z", "g", "residual"))
        z, g = o["z"].double().reshape(M, Cc), o["g"].double().reshape(M, Cc)
        mean, var = C.bn_stats_sum(z)
        eps = 0.0 if kind == "int" else 1e-5
        if kind == "int":
            assert torch.equal(mean, o["m"].double()) and torch.equal(var, o["a"].double() ** 2) and 4 * M < C.EXACT
            # the kernel's own (mean, M2) merge in fp64, thread row by thread row and slab by slab, is exact on these rows
            p = C.bn_plan(M, Cc, True)
            for r0 in range(0, M, p["slab_len"]):
                rows = z[r0:r0 + p["slab_len"]]
                assert rows.shape[0] % 2 == 0 and torch.equal(rows.mean(0), o["m"].double())
                assert torch.equal(((rows - rows.mean(0)) ** 2).sum(0), rows.shape[0] * o["a"].double() ** 2)
                assert all(bool((rows[t::p["ry"]] == rows[t]).all()) for t in range(min(p["ry"], rows.shape[0])))
        rstd = 1.0 / torch.sqrt(var + eps)
        zz = z.clone().requires_grad_(True)
        ga, be = o["gamma"].double().requires_grad_(True), o["beta"].double().requires_grad_(True)
        if eps > 0:
            y = F.batch_norm(zz, None, None, ga, be, True, 0.0, eps)
        else:                                                              # (F.batch_norm refuses eps = 0: the same function, composed)
            y = (zz - zz.mean(0)) / torch.sqrt(((zz - zz.mean(0)) ** 2).mean(0)) * ga + be
        assert float((C.bn_apply_sum(z, mean, rstd, ga.detach(), be.detach(), None, False) - y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max())
        (y * g).sum().backward()
        gz, dgamma, dbeta = C.bn_backward_sum(g, z, mean, rstd, ga.detach())
        scale = max(1.0, float(g.abs().sum(0).max()))
        assert float((dgamma - ga.grad).abs().max()) <= 1e-11 * scale and float((dbeta - be.grad).abs().max()) <= 1e-11 * scale
        assert float((gz - zz.grad).abs().max()) <= 1e-11 * max(1.0, float(zz.grad.abs().max()))
        if kind == "int":
            xhat = (z - mean) * rstd
            assert bool((xhat.abs() == 1).all()) and torch.equal(dgamma, (g * xhat).sum(0)) and torch.equal(dgamma, dgamma.round())
            y = C.bn_apply_sum(z, mean, rstd, o["gamma"].double(), o["beta"].double(), o["residual"].double().reshape(M, Cc), True)
            assert torch.equal(y, y.round()) and float(y.abs().max()) <= 4 + 4 + 4 and _bf16_exact(y)
            # mutants: the sums of the backward (integers) tell a skipped channel group or slab apart; so do the statistics for the group
            for m in C.BN_MUTANTS:
                bad = C.bn_backward_sum(g, z, mean, rstd, o["gamma"].double(), m)
                assert not torch.equal(bad[2], dbeta) and not torch.equal(bad[1], dgamma), (name, m)
            assert not torch.equal(C.bn_stats_sum(z, "skip_last_group")[1], var)
