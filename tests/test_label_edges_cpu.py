"""The contract of the label channel's three fused launches, without a GPU: a Python restatement of the exported predicates
(mgnns_label_tail_supported, mgnns_label_tail_bf16_supported, mgnns_label_gcn_supported: csrc/label_tail.hip, csrc/label_gcn.hip) equals
the library's on a grid that holds every limit and its successor; every case of tests/label_edge_cases.py lies inside its predicate and
every refusal outside it, so a table that drifts out of the contract fails here and not on the GPU; and the checks of the cases that need
the references only.  The predicates are host functions: the library loads and answers without a device."""
import itertools

import pytest
import torch

from mgnns_amd import _lib
from oracle import bf16_path as E
from tests import forward_ref as F
from tests import helpers as H
from tests import label_edge_cases as T

LDS = 160 * 1024


# ---- the predicates, restated ------------------------------------------------------------------------------------------------------------
def lt_stride(k):
    """fp32 LDS row stride of the tails: >= k rounded up to 16, == 2 (mod 32)."""
    kp = (k + 15) // 16 * 16
    return kp + (34 - kp % 32) % 32


def lg_sa(k):
    return (k + 15) // 16 * 16 + 4


def lg_sc(k):
    return 4 * ((k + 31) // 32) + 2


def tail_ok(C, NLQ, heads, dh, N5, n_out, K_pool, with_next):
    if not (C > 0 and NLQ > 0 and heads > 0 and 0 < dh <= 64 and N5 > 0 and n_out > 0):
        return False
    if K_pool and K_pool % 4:
        return False
    hid = heads * dh
    if not (hid <= 320 and heads <= 8 and N5 <= 128):
        return False
    if with_next and n_out != hid:
        return False
    if K_pool and lt_stride(NLQ * N5) < lt_stride(512):          # the read-out's 512-wide chunk is staged in the flatten buffer
        return False
    return (16 * (lt_stride(C) + 3 * lt_stride(hid) + lt_stride(NLQ * N5)) + NLQ * hid) * 4 <= LDS


def tail_bf16_ok(C, NLQ, heads, dh, N5, n_out, K_pool, terms, with_next):
    if not (0 < C <= 384 and NLQ > 0 and heads > 0 and 0 < dh <= 64 and 0 < N5 <= 128 and n_out > 0):
        return False
    if terms not in (1, 3) or not (K_pool > 0 and K_pool % 128 == 0):
        return False
    hid = heads * dh
    if not (hid <= 320 and n_out <= 384 and heads <= 8):
        return False
    if with_next and n_out != hid:
        return False
    nh, lo = (4, 1) if terms == 3 else (1, 0)
    sp, sxc, shc, sfc = 4 * (K_pool // 32 // nh) + 2, lg_sc(C), lg_sc(hid), lg_sc(NLQ * N5)
    return (1 + lo) * 16 * (max(sp, sfc) + sxc + shc) * 16 + (2 * 16 * lt_stride(hid) + NLQ * hid) * 4 <= LDS


def gcn_ok(C, K0, N1, N2, split):
    if not (0 < C <= 512 and K0 > 0 and K0 % 4 == 0 and K0 <= 1024):
        return False
    if not (N1 > 0 and N1 % 256 == 0 and N1 <= 1024 and N2 > 0 and N2 % 256 == 0):
        return False
    if C * N2 * 4 >= 2 ** 31:
        return False
    kmax = max(N1, K0)
    tile = 2 * 16 * lg_sc(kmax) * 16 if split else 16 * lg_sa(kmax) * 4
    return tile + 8 * 512 * 8 + 16 <= LDS


def tail_args(c, form):
    """A Tail and one of its forms -> (predicate, its arguments)."""
    nxt = 1 if c.HK else 0
    if form in ("x", "pool"):
        return "tail", (c.C, c.NLQ, c.heads, c.dh, c.N5, c.n_out, c.K_pool if form == "pool" else 0, nxt)
    return "bf16", (c.C, c.NLQ, c.heads, c.dh, c.N5, c.n_out, c.K_pool, 1 if form == "t1" else 3, nxt)


def ask(which, args):
    """(the library's answer, the restatement's)."""
    L = _lib.lib()
    fn, mine = {"tail": (L.mgnns_label_tail_supported, tail_ok), "bf16": (L.mgnns_label_tail_bf16_supported, tail_bf16_ok),
                "gcn": (L.mgnns_label_gcn_supported, gcn_ok)}[which]
    return bool(fn(*args)), bool(mine(*args))


# ---- the restatement equals the library ----------------------------------------------------------------------------------------------------
def test_the_restated_predicates_equal_the_librarys_on_a_grid_of_every_limit_and_its_successor():
    n = 0
    # tails: (heads, dh) pairs reach hid 320 | 321 | 324, heads 8 | 9, dh 64 | 65
    hd = [(5, 60), (5, 64), (8, 40), (9, 4), (1, 64), (1, 65), (3, 107), (6, 54), (1, 1)]
    for C, (heads, dh), N5, n_out, nxt in itertools.product((1, 365, 384, 385, 512, 513), hd, (1, 100, 128, 129),
                                                            (1, 300, 320, 384, 385), (0, 1)):
        for NLQ, K_pool in ((7, 0), (7, 2048), (7, 2046), (7, 2050), (1, 4), (5, 128), (7, 128), (7, 192)):
            lib, mine = ask("tail", (C, NLQ, heads, dh, N5, n_out, K_pool, nxt))
            assert lib == mine, ("tail", C, NLQ, heads, dh, N5, n_out, K_pool, nxt, lib, mine)
            for terms in (1, 3, 2):
                lib, mine = ask("bf16", (C, NLQ, heads, dh, N5, n_out, K_pool, terms, nxt))
                assert lib == mine, ("bf16", C, NLQ, heads, dh, N5, n_out, K_pool, terms, nxt, lib, mine)
            n += 4
    # the fp32 read-out inside: the flatten buffer must hold the 514-float stride of the staged chunk
    for flat in range(470, 520):
        lib, mine = ask("tail", (80, flat, 1, 1, 1, 300, 2048, 0))
        assert lib == mine, ("flat", flat)
    # the LDS edges: C and NLQ of the fp32 tail; K_pool and NLQ of the bf16 tail at both terms, at the golden widths
    for C in range(700, 780):
        assert len(set(ask("tail", (C, 7, 5, 60, 100, 300, 0, 1)))) == 1, C
    for NLQ in range(1, 40):
        assert len(set(ask("tail", (365, NLQ, 5, 60, 100, 300, 0, 1)))) == 1, NLQ
        for terms in (1, 3):
            assert len(set(ask("bf16", (365, NLQ, 5, 60, 100, 300, 2048, terms, 1)))) == 1, (NLQ, terms)
    for K_pool in range(128, 6400, 128):
        for terms, C in itertools.product((1, 3), (80, 365)):
            assert len(set(ask("bf16", (C, 7, 5, 60, 100, 300, K_pool, terms, 1)))) == 1, (K_pool, terms, C)
    for NLQ in range(700, 1000, 5):
        for terms in (1, 3):
            assert len(set(ask("bf16", (16, NLQ, 8, 4, 1, 33, 128, terms, 0)))) == 1, (NLQ, terms)
    # label GCN
    for C, K0, N1, N2, split in itertools.product((0, 1, 512, 513), (0, 4, 6, 300, 1024, 1028), (0, 256, 300, 1024, 1280),
                                                  (0, 256, 300, 2048, 4096), (0, 1)):
        lib, mine = ask("gcn", (C, K0, N1, N2, split))
        assert lib == mine, ("gcn", C, K0, N1, N2, split, lib, mine)
        n += 1
    print("%d grid points" % n)


def test_the_limits_the_tables_name_are_the_largest_values_accepted():
    """... and one edge that is easy to misstate: with the read-out inside the fp32 tail, NLQ * N5 is accepted from 481 on, not from
    497 (the first value whose round-up to 16 reaches 512): the test is lt_stride(NLQ * N5) >= lt_stride(512) = 514, and
    lt_stride(481 .. 496) = 496 + 18 = 514 as well, which holds the staged chunk exactly.  480 is refused.  Both 481 and 496 run on the
    GPU (TAIL_POOL_CASES)."""
    lib = lambda which, *a: ask(which, a)[0]
    gold = (5, 60, 100, 300)
    assert lib("tail", T.F32_C_MAX, 7, *gold, 0, 1) and not lib("tail", T.F32_C_MAX + 1, 7, *gold, 0, 1)
    assert lib("tail", 365, T.F32_NLQ_MAX, *gold, 0, 1) and not lib("tail", 365, T.F32_NLQ_MAX + 1, *gold, 0, 1)
    for terms in (1, 3):
        k, nlq, flat = T.BF16_K_MAX[terms], T.BF16_NLQ_MAX[terms], T.BF16_FLAT_MAX[terms]
        assert lib("bf16", 365, 7, *gold, k, terms, 1) and not lib("bf16", 365, 7, *gold, k + 128, terms, 1)
        assert lib("bf16", 365, nlq, *gold, 2048, terms, 1) and not lib("bf16", 365, nlq + 1, *gold, 2048, terms, 1)
        assert lib("bf16", 16, flat, 8, 4, 1, 33, 128, terms, 0) and not lib("bf16", 16, flat + 1, 8, 4, 1, 33, 128, terms, 0)
    assert [lt_stride(k) for k in (480, 481, 496, 497, 512)] == [482, 514, 514, 514, 514]
    assert [lib("tail", 80, k, 1, 1, 1, 300, 2048, 0) for k in (480, 481, 496, 497, 500)] == [False, True, True, True, True]
    assert lib("gcn", 512, 1024, 1024, 2048, 0) and lib("gcn", 512, 1024, 1024, 2048, 1)


# ---- the tables lie inside the contract, the refusals outside --------------------------------------------------------------------------------
ALL_TAIL = T.TAIL_X_CASES + T.TAIL_POOL_CASES + T.TAIL_BF16_CASES


def test_every_gpu_case_is_accepted_and_every_refusal_rejected():
    for c in ALL_TAIL:
        for form in c.forms:
            which, args = tail_args(c, "t3" if form == "t3c" else form)
            assert ask(which, args) == (True, True), (c, form)
        assert c.B <= 64
    for c in T.GCN_CASES:
        for split in (0, 1):
            assert ask("gcn", (c.C, c.K0, c.N1, c.N2, split)) == (True, True), c
    for what, c, _msg in T.TAIL_REFUSALS:
        assert len(c.forms) == 1
        assert ask(*tail_args(c, c.forms[0])) == (False, False), what
    for what, c, _msg in T.GCN_REFUSALS:
        for split in (0, 1):
            assert ask("gcn", (c.C, c.K0, c.N1, c.N2, split)) == (False, False), what


def test_every_value_of_every_axis_appears():
    def seen(cases, field):
        return {getattr(c, field) for c in cases}
    x, pool, bf = T.TAIL_X_CASES, T.TAIL_POOL_CASES, T.TAIL_BF16_CASES
    assert seen(x, "C") >= {1, 15, 16, 17, 365, T.F32_C_MAX}
    assert {(c.heads, c.dh) for c in x} >= {(1, 1), (8, 4), (3, 11), (5, 60), (5, 64)}
    assert seen(x, "N5") >= {1, 16, 17, 100, 128} and seen(x, "NLQ") >= {1, 2, 7, T.F32_NLQ_MAX}
    assert seen(x, "n_out") >= {1, 33, 300, 384} and seen(x, "B") >= {1, 15, 16, 17, 33, 0}
    assert {(c.HK, c.bias) for c in x if c.HK in (0, 16)} >= {(0, False), (16, False)} and seen(x, "HK") >= {136, 1040}
    assert seen(pool, "K_pool") >= {4, 20, 512, 516, 2048} and seen(pool, "parts") == {1, 2, 3}
    assert {c.NLQ * c.N5 for c in pool} >= {481, 496, 500}
    assert seen(bf, "K_pool") >= {128, 256, 384, 2048, T.BF16_K_MAX[1], T.BF16_K_MAX[3]} and seen(bf, "C") >= {1, 16, 17, 32, 33, 384}
    assert {c.heads * c.dh for c in bf} >= {1, 32, 33, 320} and {c.NLQ * c.N5 for c in bf} >= {1, 32, 33, 700}
    assert {c.n_out for c in bf if not c.HK} >= {1, 33, 384} and {c.n_out for c in bf if c.HK} >= {320}
    assert {(c.HK, c.bias) for c in bf if c.HK and "t3c" in c.forms} >= set(itertools.product((16, 136, 1040, 2048), (True, False)))
    assert seen(bf, "parts") == {1, 2, 3} and seen(bf, "B") >= {1, 16, 17, 33, 64, 0}
    g = T.GCN_CASES
    assert seen(g, "C") >= {1, 8, 9, 16, 17, 64, 65, 512} and seen(g, "K0") == {4, 36, 300, 1024}
    assert seen(g, "N1") == {256, 1024} and seen(g, "N2") == {256, 2048} and seen(g, "adj") == {"gen_A", "rows", "dense"}
    assert seen(g, "query") >= {None, (1, 1, True), (7, 300, False), (16, 2048, True)} and seen(g, "packed") == {True, False}


# ---- checks that need the references only -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL_TAIL, ids=lambda c: "-".join(str(v) for v in c[:11]) + "-" + c.forms[0])
def test_tail_references_are_sound(c):
    """No reference output is all zero, the plain float32-following formula agrees with the oracle's terms = 3, the terms = 1 bound is
    positive, and the float32-CPU error of the reference is printed beside the bound it is to be compared with."""
    d = T.tail_data(c)
    nq = None if d["next_w"] is None else (d["next_w"], d["next_b"])
    parts = d["x"][:, None, :] if "x" in c.forms else d["pooled"]
    Gm = torch.eye(c.C) if "x" in c.forms else d["G"]
    plain = F.label_tail(*H.f64([parts, Gm, d["Q"]]), c.heads, H.f64(T.tail_weights(d)), H.f64(nq))
    base = (T.TERMS3, T.TERMS3) if set(c.forms) & set(T.BF) else (T.TAIL_OUT, T.TAIL_NEXT)
    for i, name in enumerate(("out", "next")):
        r3 = d["ref3"][i]
        if r3 is None:
            assert i == 1 and not c.HK
            continue
        assert tuple(r3.shape) == (c.B, c.HK if i else c.n_out)
        if not c.B:
            continue
        assert torch.isfinite(r3).all() and H.scale(r3) > 0
        assert H.maxerr(plain[i], r3) <= 1e-12 * H.scale(r3)
        err = d["cpu_err"][i]
        print("%s: scale %.3f, float32-CPU error %.3e, bound %.3e" % (name, H.scale(r3), err, base[i] * H.scale(r3)))
        assert 4 * err <= base[i] * H.scale(r3), "%s: 4 x the float32-CPU error %.3e is past the bound" % (name, err)
    if "t1" in c.forms and c.B:
        for b, r1 in zip(T.terms1_bounds(d), d["ref1"]):
            if r1 is not None:
                print("terms = 1 bound %.3e (scale %.3f)" % (b, H.scale(r1)))
                assert b > 0 and H.scale(r1) > 0


@pytest.mark.parametrize("c", T.GCN_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_gcn_references_are_sound(c):
    d = T.gcn_data(c)
    G, Q = d["ref"]
    assert tuple(G.shape) == (c.C, c.N2) and torch.isfinite(G).all() and H.scale(G) > 0
    assert (d["A"].sum(1) > 0).all()
    nnz = d["nnz"].tolist()
    if c.adj == "rows":
        assert nnz[:4] == [1, 4, 3, c.C]
    elif c.adj == "dense":
        assert nnz == [c.C] * c.C
    else:
        assert min(nnz) >= 1 and (c.C < 64 or {n % 2 for n in nnz} == {0, 1})
    errs = d["cpu_err"]
    print("G: scale %.3f, float32-CPU error %.3e, bounds %.3e exact, %.3e split" % (H.scale(G), errs[0], T.GCN_EXACT * H.scale(G), T.GCN_SPLIT * H.scale(G)))
    for mode, base in (("exact", T.GCN_EXACT), ("split", T.GCN_SPLIT)):
        # the reference evaluated in float32 stays inside the bound itself (0.4 of it at most, here): no case has a bound of its own
        assert errs[0] <= base * H.scale(G), "G %s: the float32-CPU error %.3e is past the bound" % (mode, errs[0])
    if c.query is not None:
        assert tuple(Q.shape) == c.query[:2] and H.scale(Q) > 0
        print("Q: scale %.3f, float32-CPU error %.3e, bound %.3e" % (H.scale(Q), errs[1], T.GCN_Q * H.scale(Q)))
        assert 4 * errs[1] <= T.GCN_Q * H.scale(Q), "Q: 4 x the float32-CPU error %.3e is past the bound" % errs[1]


def test_the_oracle_at_terms_1_rounds_and_at_terms_3_does_not():
    """The two ends of the terms = 1 bound differ by bf16-sized rounding noise, not by nothing and not by the output."""
    c = T.TAIL_BF16_CASES[3]
    d = T.tail_data(c)
    for r1, r3 in zip(d["ref1"], d["ref3"]):
        noise = H.maxerr(r1, r3) / H.scale(r3)
        assert 1e-5 < noise < 5e-2, noise
    assert E.bf16_round(torch.tensor([1.00390625])).item() == 1.0          # 1 + 2^-8: a tie, to even
