"""The case tables of the label channel's edge sweep, shared by tests/test_label_edges_cpu.py (which proves every case inside its
predicate and every refusal outside it, without a GPU) and tests/test_label_edges_gpu.py (which runs them), with the float64
references of the cases, computed once per process and shared by the tests that need them.

The three launches -- mgnns_label_tail_fwd, mgnns_label_tail_bf16_fwd (csrc/label_tail.hip) and mgnns_label_gcn_fwd
(csrc/label_gcn.hip) -- take every shape their exported predicates accept, so the cases sit at the predicates' limits and where a
kernel changes path: a GEMM shorter than its prefetch ring (mg_tile_gemm_f32: 4 k-quads of 16; WRing: 10 k-steps of 32 at terms = 1,
4 at terms = 3, 3 in the label GCN), a width that ends inside a 16-column tile or a k-step, more than one round of 24 column tiles, a
cluster rank with no next-query slot or with four of them, adjacency rows of every parity.  Hand-picked, not cross products: every
value of every axis appears at least once.

Bounds.  The ones the suite asserts for the same kernels at the golden shape, relative to the reference's largest magnitude (TAIL_OUT,
TAIL_NEXT, TERMS3, GCN_EXACT, GCN_SPLIT, GCN_Q, CLUSTER below): no case carries a bound of its own.  The float32-CPU error of each
reference (helpers.fp32_cpu_err, printed by both test files) stays below every one of them -- at most 0.06 of a tail's bound; 0.25 to
0.4 of the exact label GCN's 2e-6 at its deepest cases (C = 512 with K0 = N1 = 1024: 1.1e-6 on one host, 7.4e-7 on another, at an
output scale of 1.39), which that kernel meets all the same.  terms = 1 is compared with the oracle that rounds where the kernel
rounds; its bound comes from the reference alone: max|label_tail(terms=1) - label_tail(terms=3)| (the case's whole bf16 rounding noise) + 2^-8 max|reference| (one
rounding flip of an output-scale value).  No bound is set from what a kernel returns."""
import collections
import functools

import numpy as np
import torch

from mgnns_amd import synth
from oracle import bf16_path as E
from tests import forward_ref as F
from tests import helpers as H

TAIL_OUT = 2e-5      # ops.label_tail output (test_fused_label_tail_against_goldens_and_ragged_batches)
TAIL_NEXT = 5e-5     # ... its next query
TERMS3 = 1e-4        # ops.label_tail_bf16 at terms = 3 (test_fused_label_tail_bf16_vs_oracle)
CLUSTER = 1e-5       # cluster form against the single-workgroup form (the same test)
GCN_EXACT = 2e-6     # ops.label_gcn, exact mode (test_persistent_label_gcn_against_goldens_and_the_separate_operators)
GCN_SPLIT = 2e-5     # ... split-bf16 mode
GCN_Q = 1e-5         # ... the projected label query

# The predicates' limits at the golden widths (5 heads of 60, N5 = 100, n_out = 300, NLQ = 7, a next query) -- each the largest value
# accepted, its successor (the next multiple of 128 for K_pool) refused: tests/test_label_edges_cpu.py proves both.
F32_C_MAX = 736           # fp32 tail, read-out given: the largest C
F32_NLQ_MAX = 9           # fp32 tail: the largest NLQ at C = 365
BF16_K_MAX = {1: 2816, 3: 4096}       # bf16 tail: the largest K_pool at C = 365, per terms
BF16_NLQ_MAX = {1: 22, 3: 9}          # bf16 tail: the largest NLQ at C = 365, K_pool = 2048
BF16_FLAT_MAX = {1: 970, 3: 790}      # bf16 tail: the largest NLQ (N5 = 1) at C = 16, 8 heads of 4, n_out = 33, K_pool = 128

# forms: "x" fp32 tail with the read-out given | "pool" fp32 tail with the read-out in the kernel | "t1" bf16 tail at terms = 1 |
# "t3" terms = 3, one workgroup per tile | "t3c" terms = 3, four-workgroup cluster.  HK = 0: no next query.
Tail = collections.namedtuple("Tail", "C NLQ heads dh N5 n_out K_pool parts HK bias B forms")
BF = ("t1", "t3", "t3c")

# read-out given (K_pool here only sizes the product the read-out x is made from on the CPU)
TAIL_X_CASES = [
    Tail(1, 1, 1, 1, 1, 1, 8, 1, 16, False, 1, ("x",)),                # every width one: each GEMM a single k-quad
    Tail(15, 2, 8, 4, 16, 32, 8, 1, 136, True, 15, ("x",)),
    Tail(16, 7, 3, 11, 17, 33, 8, 1, 1040, True, 16, ("x",)),
    Tail(17, 1, 5, 60, 100, 384, 8, 1, 0, False, 17, ("x",)),          # n_out 384: all 24 column tiles of one round
    Tail(17, 2, 5, 60, 16, 400, 8, 1, 0, False, 16, ("x",)),           # n_out 400 (the fp32 tail sets no limit): a second round
    Tail(365, F32_NLQ_MAX, 5, 60, 100, 300, 8, 1, 136, True, 33, ("x",)),
    Tail(F32_C_MAX, 7, 5, 60, 100, 300, 8, 1, 1040, True, 17, ("x",)),
    Tail(365, 7, 5, 64, 128, 320, 8, 1, 16, False, 33, ("x",)),
    Tail(16, 7, 5, 60, 100, 300, 8, 1, 136, True, 0, ("x",)),
]
# read-out in the kernel: K_pool below, at and past the 512-wide staging chunk; NLQ * N5 = 500, and 481 | 496, the two ends of the
# narrowest flatten buffer the 514-float chunk stride still fits (lt_stride(481) = lt_stride(496) = lt_stride(512) = 514)
TAIL_POOL_CASES = [
    Tail(17, 5, 5, 60, 100, 300, 4, 1, 0, False, 1, ("pool",)),
    Tail(80, 13, 3, 11, 37, 33, 20, 2, 16, False, 17, ("pool",)),
    Tail(365, 7, 5, 60, 100, 300, 512, 3, 136, True, 33, ("pool",)),
    Tail(16, 4, 8, 4, 124, 33, 516, 2, 0, False, 16, ("pool",)),
    Tail(365, 7, 5, 60, 100, 300, 2048, 2, 1040, True, 17, ("pool",)),
    Tail(F32_C_MAX, 7, 5, 60, 100, 300, 516, 3, 0, False, 15, ("pool",)),     # 46 column tiles of G: two rounds of 24
]
# bf16 tail.  Next query: 16 wide = one slot of eight column tiles (ranks 1-3 of a cluster own none), 136 = two slots, 1040 = nine (three
# per rank, the last rank none), 2048 = sixteen (four per rank: the second pass of the slot loop)
TAIL_BF16_CASES = [
    Tail(1, 1, 1, 1, 1, 1, 128, 1, 0, False, 1, BF),                   # every width one: each GEMM a single k-step
    Tail(16, 2, 8, 4, 16, 32, 256, 2, 16, True, 16, BF),
    Tail(17, 3, 3, 11, 11, 33, 384, 3, 16, False, 17, BF),
    Tail(32, 7, 5, 60, 100, 300, 2048, 2, 136, True, 33, BF),
    Tail(33, 7, 5, 64, 100, 320, 128, 1, 136, False, 64, BF),
    Tail(384, 7, 5, 60, 100, 384, 2048, 2, 0, False, 17, BF),
    Tail(365, 7, 5, 60, 100, 300, BF16_K_MAX[1], 2, 1040, True, 17, ("t1",)),
    Tail(365, 7, 5, 60, 100, 300, BF16_K_MAX[3], 2, 1040, True, 17, ("t3", "t3c")),
    Tail(80, 7, 5, 60, 100, 300, 2048, 3, 1040, False, 33, BF),
    Tail(365, 7, 5, 60, 100, 300, 2048, 2, 2048, True, 64, BF),
    Tail(80, 7, 5, 60, 100, 300, 256, 1, 2048, False, 1, BF),
    Tail(17, 2, 3, 11, 16, 33, 128, 1, 0, False, 16, BF),
    Tail(365, BF16_NLQ_MAX[1], 5, 60, 100, 300, 2048, 2, 136, True, 16, ("t1",)),
    Tail(365, BF16_NLQ_MAX[3], 5, 60, 100, 300, 2048, 2, 136, True, 16, ("t3", "t3c")),
    Tail(16, BF16_FLAT_MAX[1], 8, 4, 1, 33, 128, 1, 0, False, 1, ("t1",)),
    Tail(16, BF16_FLAT_MAX[3], 8, 4, 1, 33, 128, 1, 0, False, 17, ("t3", "t3c")),
    Tail(80, 7, 5, 60, 100, 300, 2048, 2, 136, True, 0, BF),
]

# adjacency kinds: "gen_A" thresholded counts re-weighted with an identity diagonal (synth.gen_A_from_binary) | "rows" positive weights
# whose normalised adjacency has a row with only its diagonal, a row with an even and a row with an odd number of non-zeros and a fully
# dense row (C >= 4) | "dense" every entry non-zero.  query = (NLQ, HQ, bias) or None.
Gcn = collections.namedtuple("Gcn", "C K0 N1 N2 adj query packed")
GCN_CASES = [
    Gcn(1, 4, 256, 256, "dense", (1, 1, True), True),
    Gcn(8, 36, 256, 2048, "gen_A", None, False),
    Gcn(9, 300, 1024, 256, "rows", (7, 300, False), True),
    Gcn(16, 4, 1024, 2048, "dense", (16, 2048, True), True),
    Gcn(17, 36, 256, 256, "rows", None, True),
    Gcn(64, 300, 1024, 2048, "gen_A", (7, 300, False), True),
    Gcn(65, 1024, 256, 256, "rows", (1, 1, True), False),
    Gcn(512, 36, 256, 256, "dense", None, True),                       # every ELL row holds all 512 slots
    Gcn(512, 1024, 1024, 2048, "gen_A", (16, 2048, True), True),       # every limit at once: two 1024-deep products
]
GCN_GRIDS = (1, 3, 0)


# ---- refusals: (launch, what is over its limit, the arguments, a piece of the launcher's message) --------------------------------------
# tail arguments: a Tail; the fp32 launch takes forms "x" / "pool", the bf16 one "t1" / "t3"
TAIL_REFUSALS = [
    ("C 385 (bf16)", Tail(385, 7, 5, 60, 100, 300, 2048, 1, 0, False, 1, ("t3",)), "bad dims"),
    ("heads 9", Tail(80, 7, 9, 4, 100, 36, 2048, 1, 0, False, 1, ("x",)), "unsupported"),
    ("heads 9 (bf16)", Tail(80, 7, 9, 4, 100, 36, 2048, 1, 0, False, 1, ("t1",)), "unsupported"),
    ("dh 65", Tail(80, 7, 1, 65, 100, 65, 2048, 1, 0, False, 1, ("x",)), "bad dims"),
    ("dh 65 (bf16)", Tail(80, 7, 1, 65, 100, 65, 2048, 1, 0, False, 1, ("t3",)), "bad dims"),
    ("hid 321", Tail(80, 7, 3, 107, 100, 300, 2048, 1, 0, False, 1, ("x",)), "bad dims"),          # 107 > 64 as well: dh first
    ("hid 324", Tail(80, 7, 6, 54, 100, 300, 2048, 1, 0, False, 1, ("x",)), "hidden width"),
    ("hid 324 (bf16)", Tail(80, 7, 6, 54, 100, 300, 2048, 1, 0, False, 1, ("t3",)), "hidden width"),
    ("N5 129", Tail(80, 7, 5, 60, 129, 300, 2048, 1, 0, False, 1, ("x",)), "linear_5 width"),
    ("N5 129 (bf16)", Tail(80, 7, 5, 60, 129, 300, 2048, 1, 0, False, 1, ("t1",)), "bad dims"),
    ("n_out 385 (bf16)", Tail(80, 7, 5, 60, 100, 385, 2048, 1, 0, False, 1, ("t3",)), "output width"),
    ("K_pool % 128 (bf16)", Tail(80, 7, 5, 60, 100, 300, 2112, 1, 0, False, 1, ("t1",)), "K % 128"),
    ("K_pool % 4", Tail(80, 7, 5, 60, 100, 300, 2046, 1, 0, False, 1, ("pool",)), "K % 4"),
    ("n_out != hid with a next query", Tail(80, 7, 5, 60, 100, 299, 2048, 1, 16, True, 1, ("x",)), "query projection needs"),
    ("n_out != hid with a next query (bf16)", Tail(80, 7, 5, 60, 100, 299, 2048, 1, 16, True, 1, ("t3",)), "query projection needs"),
    ("NLQ * N5 480 with the read-out inside", Tail(80, 5, 5, 60, 96, 300, 2048, 1, 0, False, 1, ("pool",)), "too small to stage"),
    ("C past the LDS", Tail(F32_C_MAX + 1, 7, 5, 60, 100, 300, 8, 1, 16, True, 1, ("x",)), "of LDS"),
    ("NLQ past the LDS", Tail(365, F32_NLQ_MAX + 1, 5, 60, 100, 300, 8, 1, 16, True, 1, ("x",)), "of LDS"),
    ("K_pool past the LDS (terms 1)", Tail(365, 7, 5, 60, 100, 300, BF16_K_MAX[1] + 128, 1, 16, True, 1, ("t1",)), "of LDS"),
    ("K_pool past the LDS (terms 3)", Tail(365, 7, 5, 60, 100, 300, BF16_K_MAX[3] + 128, 1, 16, True, 1, ("t3",)), "of LDS"),
    ("NLQ past the LDS (terms 1)", Tail(365, BF16_NLQ_MAX[1] + 1, 5, 60, 100, 300, 2048, 1, 16, True, 1, ("t1",)), "of LDS"),
    ("NLQ past the LDS (terms 3)", Tail(365, BF16_NLQ_MAX[3] + 1, 5, 60, 100, 300, 2048, 1, 16, True, 1, ("t3",)), "of LDS"),
]
GCN_REFUSALS = [
    ("C 513", Gcn(513, 36, 256, 256, "gen_A", None, False), "C=513 unsupported"),
    ("K0 % 4", Gcn(8, 302, 256, 256, "gen_A", None, False), "multiple of 4"),
    ("K0 1028", Gcn(8, 1028, 256, 256, "gen_A", None, False), "multiple of 4"),
    ("N1 % 256", Gcn(8, 36, 300, 256, "gen_A", None, False), "multiples of 256"),
    ("N1 1280", Gcn(8, 36, 1280, 256, "gen_A", None, False), "multiples of 256"),
    ("N2 % 256", Gcn(8, 36, 256, 300, "gen_A", None, False), "multiples of 256"),
]


# ---- case data and references (float64), once per process --------------------------------------------------------------------------------
def tail_weights(case):
    """The generator's parameters under the names of forward_ref.label_tail."""
    p, c = case["p"], case["chan"]
    a = c + "_attention."
    return {"wk": p[a + "w_k.weight"], "bk": p[a + "w_k.bias"], "wv": p[a + "w_v.weight"], "bv": p[a + "w_v.bias"],
            "wfc": p[a + "fc.weight"], "bfc": p[a + "fc.bias"], "w5": p[c + "_linear_5.weight"], "b5": p[c + "_linear_5.bias"],
            "wxl": p[c + "_x_linear.weight"], "bxl": p[c + "_x_linear.bias"]}


@functools.lru_cache(maxsize=None)
def tail_data(c):
    """Tail -> dict: the generated case (helpers.label_tail_case), `x` [B, C] float32 for the form "x" (the read-out, made on the CPU in
    float64 and rounded once: it is the kernel's INPUT there, and the reference starts from the same values through an identity G),
    ref3 = (out, next) of oracle label_tail(terms=3), ref1 the same at terms = 1 (bf16 cases), cpu_err = the float32-CPU error of
    (out, next).  Nothing in it is modified by a test."""
    case = H.label_tail_case(c.C, c.NLQ, c.heads, c.dh, c.N5, c.n_out, c.K_pool, c.parts, c.HK, c.B, c.bias)
    d = dict(case)
    if "x" in c.forms:
        d["x"] = (case["pooled"].double().max(dim=1).values @ case["G"].double().t()).float()
        parts, Gm = d["x"][:, None, :], torch.eye(c.C)
    else:
        parts, Gm = case["pooled"], case["G"]
    src = parts.max(dim=1).values
    d["ref3"] = E.label_tail(case["p"], case["chan"], src, Gm, case["Q"], c.heads, case["next_w"], case["next_b"], terms=3)
    if "t1" in c.forms:
        d["ref1"] = E.label_tail(case["p"], case["chan"], src, Gm, case["Q"], c.heads, case["next_w"], case["next_b"], terms=1)
    nq = None if case["next_w"] is None else (case["next_w"], case["next_b"])
    d["cpu_err"] = H.fp32_cpu_err(lambda *a: F.label_tail(a[0], a[1], a[2], c.heads, a[3], a[4]),
                                  *H.f64([parts, Gm, case["Q"], tail_weights(case), nq]))
    return d


def terms1_bounds(d):
    """(bound of out, bound of next or None) at terms = 1, from the references alone."""
    return [None if r1 is None else H.maxerr(r1, r3) + 2.0 ** -8 * H.scale(r1) for r1, r3 in zip(d["ref1"], d["ref3"])]


def adjacency(kind, C, rs):
    """A [C, C] float32 of one of the three kinds (every row sum positive: no all-zero row)."""
    if kind == "gen_A":
        P = (rs.uniform(size=(C, C)) < min(0.5, 6.0 / C)).astype(np.float64)
        np.fill_diagonal(P, 0)
        return synth.gen_A_from_binary(P)
    if kind == "dense":
        return (rs.uniform(size=(C, C)) + 0.1).astype(np.float32)
    # "rows": row i of the normalised adjacency has its non-zeros where COLUMN i of A has them
    assert C >= 4
    P = rs.uniform(size=(C, C)) < 0.3
    P[:, 0] = False                                  # adjacency row 0: the diagonal alone
    P[:, 1] = False
    P[rs.choice(np.arange(2, C), 3, replace=False), 1] = True      # row 1: 3 + the diagonal = an even count
    P[:, 2] = False
    P[rs.choice(np.array([0, 1] + list(range(3, C))), 2, replace=False), 2] = True      # row 2: 2 + the diagonal = an odd count
    P[:, 3] = True                                   # row 3: fully dense
    np.fill_diagonal(P, True)
    return (P * rs.uniform(0.1, 1.0, size=(C, C))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gcn_data(c):
    """Gcn -> dict(A, inp, w1, w2 ([in, out] layout), query = (label_query, w_q.weight, bias or None) or None: float32 tensors; ref =
    (G, Q) of forward_ref.label_gcn in float64; cpu_err = its float32-CPU error; nnz = non-zeros per row of the normalised adjacency)."""
    rs = np.random.RandomState(c.C * 131 + c.K0 * 7 + c.N1 + c.N2 * 3 + len(c.adj))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    d = {"A": t(adjacency(c.adj, c.C, rs)), "inp": t(0.5 * rs.standard_normal((c.C, c.K0))),
         "w1": t(rs.standard_normal((c.K0, c.N1)) / np.sqrt(c.K0)), "w2": t(rs.standard_normal((c.N1, c.N2)) / np.sqrt(c.N1)), "query": None}
    if c.query is not None:
        nlq, hq, bias = c.query
        d["query"] = (t(rs.standard_normal((nlq, c.K0))), t(rs.standard_normal((hq, c.K0)) / np.sqrt(c.K0)),
                      t(0.5 * rs.standard_normal(hq)) if bias else None)
    args = H.f64([d["A"], d["inp"], d["w1"], d["w2"], d["query"]])
    d["ref"] = F.label_gcn(*args)
    d["cpu_err"] = H.fp32_cpu_err(F.label_gcn, *args)
    d["nnz"] = (F.gen_adj(args[0]) != 0).sum(1)
    return d
