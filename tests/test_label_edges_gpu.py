"""Edge sweep of the label channel's three fused launches, each through its ops.* wrapper: ops.label_tail (mgnns_label_tail_fwd),
ops.label_tail_bf16 (mgnns_label_tail_bf16_fwd: terms = 1, terms = 3, terms = 3 as a four-workgroup cluster) and ops.label_gcn
(mgnns_label_gcn_fwd: exact and split-bf16), at the shapes their predicates accept and the suite's golden-shape tests never reach.
Cases, references and bounds live in tests/label_edge_cases.py (proven inside the predicates by tests/test_label_edges_cpu.py); the
references are float64 on the CPU: oracle/bf16_path.label_tail for both tails, tests/forward_ref.label_gcn for the GCN.  Every test
prints its error beside its bound, and the float32-CPU error of the same reference, before it asserts.

Largest errors seen on an MI355X, as a fraction of the bound (the run that accompanied this file; each test prints its own):
fp32 tail out 0.05, next 0.02, with the read-out given or inside; bf16 tail at terms = 3 out 0.07, next 0.09, the cluster form the
same, cluster against single workgroup 0.32; terms = 1 out 0.01, next 0.08; label GCN exact G 0.65 (1.7e-6 against 2.7e-6 at C = 64,
K0 = 300; 2.1e-6 against 2.8e-6 with every limit at once), split G 0.41, Q 0.01.  Every case passed as the kernels stand."""
import re

import pytest
import torch

from mgnns_amd import ops
from tests import label_edge_cases as T
from tests.helpers import close, label_tail_case, maxerr, scale
from tests.test_forward_edges_gpu import dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ident = lambda c: "-".join(str(v) for v in c[:11])


def composed(case):
    """(Wc, bc) = (W5 . Wfc, W5 . b_fc + b5): the one map the kernels apply for fc and linear_5, composed in float64 and rounded once."""
    p, c = case["p"], case["chan"]
    w5, wfc = p[c + "_linear_5.weight"].double(), p[c + "_attention.fc.weight"].double()
    return (w5 @ wfc).float(), (w5 @ p[c + "_attention.fc.bias"].double() + p[c + "_linear_5.bias"].double()).float()


def packed_tail(case, pack):
    """The `packed` dict of ops.label_tail (pack = ops.pack_weight_f32) or ops.label_tail_bf16 (ops.pack_weight_bf16_split)."""
    w = T.tail_weights(case)
    wc, bc = composed(case)
    return {"wk": pack(dev(w["wk"])), "bk": dev(w["bk"]), "wv": pack(dev(w["wv"])), "bv": dev(w["bv"]), "wc": pack(dev(wc)), "bc": dev(bc),
            "n5": wc.shape[0], "C": w["wk"].shape[1], "xl": pack(dev(w["wxl"])), "bxl": dev(w["bxl"]), "n_out": w["wxl"].shape[0]}


def next_query(c, case, pack):
    return None if not c.HK else (pack(dev(case["next_w"])), dev(case["next_b"]) if c.bias else None, c.HK)


def check_tail(got, refs, bounds, c, what):
    """got: out or (out, next); refs: (out, next or None); bounds: absolute, per output."""
    got = got if isinstance(got, tuple) else (got, None)
    for g, r, b, name in zip(got, refs, bounds, ("out", "next")):
        if r is None:
            assert g is None
            continue
        assert tuple(g.shape) == tuple(r.shape)
        close(g, r, b, "%s %s" % (what, name))


def f32_bounds(c, d):
    return [base * scale(r) if r is not None else None for base, r in zip((T.TAIL_OUT, T.TAIL_NEXT), d["ref3"])]


# ---- fp32 tail ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.TAIL_X_CASES, ids=ident)
def test_label_tail_with_the_read_out_given(c):
    d = T.tail_data(c)
    print("float32-CPU error of the reference (out, next):", d["cpu_err"])
    got = ops.label_tail(dev(d["x"]), dev(d["Q"]), c.heads, packed_tail(d, ops.pack_weight_f32), next_q=next_query(c, d, ops.pack_weight_f32))
    check_tail(got, d["ref3"], f32_bounds(c, d), c, "label_tail")


@pytest.mark.parametrize("c", T.TAIL_POOL_CASES, ids=ident)
def test_label_tail_with_the_read_out_in_the_kernel(c):
    d = T.tail_data(c)
    print("float32-CPU error of the reference (out, next):", d["cpu_err"])
    pk, nq, Q = packed_tail(d, ops.pack_weight_f32), next_query(c, d, ops.pack_weight_f32), dev(d["Q"])
    g_wp = ops.pack_weight_f32(dev(d["G"]))
    got = ops.label_tail(None, Q, c.heads, pk, pooled=dev(d["pooled"]), g_wp=g_wp, next_q=nq)
    check_tail(got, d["ref3"], f32_bounds(c, d), c, "label_tail, read-out inside")
    one = ops.label_tail(None, Q, c.heads, pk, pooled=dev(d["pooled"].max(dim=1, keepdim=True).values), g_wp=g_wp, next_q=nq)
    for a, b in zip(got if c.HK else (got,), one if c.HK else (one,)):
        assert torch.equal(a, b), "a one-part input must equal the max over the parts bit for bit"


# ---- bf16 tail ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.TAIL_BF16_CASES, ids=ident)
def test_label_tail_bf16_all_three_forms(c):
    d = T.tail_data(c)
    print("float32-CPU error of the reference (out, next):", d["cpu_err"])
    sp = ops.pack_weight_bf16_split
    pk, nq, Q, pooled, gp = packed_tail(d, sp), next_query(c, d, sp), dev(d["Q"]), dev(d["pooled"]), sp(dev(d["G"]))
    run = lambda terms, cluster: ops.label_tail_bf16(pooled, gp, Q, c.heads, pk, next_q=nq, terms=terms, cluster=cluster)
    t3 = [None if r is None else T.TERMS3 * scale(r) for r in d["ref3"]]
    if "t1" in c.forms:
        check_tail(run(1, False), d["ref1"], T.terms1_bounds(d), c, "terms = 1")
    single = None
    if "t3" in c.forms:
        single = run(3, False)
        check_tail(single, d["ref3"], t3, c, "terms = 3")
    if "t3c" in c.forms:
        first = run(3, True)
        check_tail(first, d["ref3"], t3, c, "terms = 3, cluster")
        for _ in range(4):
            again = run(3, True)
            for a, b in zip(first if c.HK else (first,), again if c.HK else (again,)):
                assert torch.equal(a, b), "the cluster form must repeat bit for bit"
        if c.B:
            assert all(int(ws[2].abs().sum()) == 0 for ws in pk["_cluster_ws"].values()), "cluster counters not re-armed"
        for a, b, r, name in zip(first if c.HK else (first,), single if c.HK else (single,), d["ref3"], ("out", "next")):
            close(a, b.cpu().double(), T.CLUSTER * scale(r), "cluster against single workgroup, " + name)
    one = dev(d["pooled"].max(dim=1, keepdim=True).values)
    for form in c.forms:
        terms, cluster = (1, False) if form == "t1" else (3, form == "t3c")
        a = ops.label_tail_bf16(one, gp, Q, c.heads, pk, next_q=nq, terms=terms, cluster=cluster)
        b = run(terms, cluster)
        for u, v in zip(a if c.HK else (a,), b if c.HK else (b,)):
            assert torch.equal(u, v), "a one-part input must equal the max over the parts bit for bit (%s)" % form


# ---- label GCN ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["exact", "split"])
@pytest.mark.parametrize("c", T.GCN_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_label_gcn_edges(c, split):
    d = T.gcn_data(c)
    rG, rQ = d["ref"]
    print("float32-CPU error of the reference (G, Q):", d["cpu_err"], "non-zeros per adjacency row: %d .. %d" % (int(d["nnz"].min()), int(d["nnz"].max())))
    mode = "split" if split else "exact"
    A, inp = dev(d["A"]), dev(d["inp"])
    packed = ops.label_gcn_pack(dev(d["w1"]), dev(d["w2"]), split=split)
    query = None if d["query"] is None else tuple(dev(t) for t in d["query"])
    outs = []
    for grid in T.GCN_GRIDS + (0, 0):                              # every grid, then the default twice more: three repeated launches
        G, Gp, Q = ops.label_gcn(A, inp, packed, want_packed_g=c.packed, query=query, grid=grid)
        outs.append((G, Gp, Q))
        assert all(int(ws[:256].view(torch.int32).abs().sum()) == 0 for ws in packed["_scratch"].values()), "queue counters not re-armed"
    G, Gp, Q = outs[0]
    close(G, rG, (T.GCN_SPLIT if split else T.GCN_EXACT) * scale(rG), "label_gcn %s G" % mode)
    if query is None:
        assert Q is None
    else:
        close(Q, rQ, T.GCN_Q * scale(rQ), "label_gcn %s Q" % mode)
    for G2, Gp2, Q2 in outs[1:]:
        assert torch.equal(G2, G), "G must not change by a bit with the grid or from launch to launch"
        assert Q is None or torch.equal(Q2, Q)
        assert Gp is None or (torch.equal(Gp2[0], Gp[0]) and torch.equal(Gp2[1], Gp[1]))
    if c.packed:
        want = ops.pack_weight_bf16_split(G)                        # rows C .. the next multiple of 16 of the image are zero in both
        assert torch.equal(Gp[0], want[0]) and torch.equal(Gp[1], want[1]), "the packed image differs from pack_weight_bf16_split(G)"
    else:
        assert Gp is None


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,c,msg", T.TAIL_REFUSALS, ids=[r[0] for r in T.TAIL_REFUSALS])
def test_the_tails_refuse_each_limit_plus_one_with_their_own_message(what, c, msg):
    """The launchers return before any launch: these calls cost nothing on the GPU."""
    d = label_tail_case(c.C, c.NLQ, c.heads, c.dh, c.N5, c.n_out, c.K_pool, c.parts, c.HK, c.B, c.bias)
    form = c.forms[0]
    pack = ops.pack_weight_f32 if form in ("x", "pool") else ops.pack_weight_bf16_split
    pk, nq, Q = packed_tail(d, pack), next_query(c, d, pack), dev(d["Q"])
    name = "mgnns_label_tail_fwd" if form in ("x", "pool") else "mgnns_label_tail_bf16_fwd"
    with pytest.raises(RuntimeError, match=re.escape(name) + ".*" + re.escape(msg)):
        if form == "x":
            ops.label_tail(dev(torch.zeros(c.B, c.C)), Q, c.heads, pk, next_q=nq)
        elif form == "pool":
            ops.label_tail(None, Q, c.heads, pk, pooled=dev(d["pooled"]), g_wp=pack(dev(d["G"])), next_q=nq)
        else:
            ops.label_tail_bf16(dev(d["pooled"]), pack(dev(d["G"])), Q, c.heads, pk, next_q=nq, terms=1 if form == "t1" else 3, cluster=False)


@pytest.mark.parametrize("split", [False, True], ids=["exact", "split"])
@pytest.mark.parametrize("what,c,msg", T.GCN_REFUSALS, ids=[r[0] for r in T.GCN_REFUSALS])
def test_the_label_gcn_refuses_each_limit_plus_one_with_its_own_message(what, c, msg, split):
    d = T.gcn_data(c)
    packed = ops.label_gcn_pack(dev(d["w1"]), dev(d["w2"]), split=split)
    with pytest.raises(RuntimeError, match=r"mgnns_label_gcn_fwd.*" + re.escape(msg)):
        ops.label_gcn(dev(d["A"]), dev(d["inp"]), packed)
