"""The split-bf16 cluster form of the label tail (ops.label_tail_bf16(terms=3, cluster=True)): four workgroups contract a quarter of
the read-out's K each, the last one to arrive runs K/V, the label loop and x_linear for the tile alone, and the next query is a
second launch behind it (csrc/label_tail.hip).  Nothing waits for anything, so the things that can go wrong are the arrival count
and its re-arm, which rank writes what, and the second launch's share of the column tiles: every case below is run five times over
and compared bit for bit, against the float64 oracle, and against the single-workgroup form.

Cases, reference and bounds are the edge sweep's (tests/label_edge_cases.py: helpers.label_tail_case, oracle/bf16_path.label_tail
in float64, TERMS3 = 1e-4 and CLUSTER = 1e-5 of the reference's largest magnitude), at the golden widths (7 label rows, 5 heads of
60, N5 = 100, 300 out).  B: one ragged tile, one full tile, a tile plus one row, three tiles with a ragged last.  C: under one
column tile, two column tiles, the object channel.  K_pool: the smallest the predicate accepts (one k-step per rank) and 2048.
Next query: none, 128 wide (8 one-wave workgroups of the second launch per tile), 1024 wide (64); its loads without 16-byte
alignment (n_out % 4 != 0) are the edge sweep's cases with 33 outputs."""
import itertools

import pytest
import torch

from mgnns_amd import _lib, ops
from oracle import bf16_path as E
from tests import label_edge_cases as T
from tests.helpers import close, label_tail_case, scale
from tests.test_forward_edges_gpu import dev
from tests.test_label_edges_gpu import check_tail, next_query, packed_tail

pytestmark = pytest.mark.gpu
NLQ, HEADS, DH, N5, N_OUT = 7, 5, 60, 100, 300


def smallest_k_pool():
    """The smallest K_pool mgnns_label_tail_bf16_supported accepts at terms = 3 (the cluster form has no limit of its own)."""
    L = _lib.lib()
    for k in range(4, 4097, 4):
        if L.mgnns_label_tail_bf16_supported(5, NLQ, HEADS, DH, N5, N_OUT, k, 3, 1):
            return k
    raise AssertionError("no K_pool accepted")


K_MIN = 128
CASES = [T.Tail(C, NLQ, HEADS, DH, N5, N_OUT, K, parts, HK, True, B, ("t3c",))
         for B, C, K, parts, HK in itertools.product((1, 16, 17, 33), (5, 17, 80), (K_MIN, 2048), (1, 2), (0, 128, 1024))]
ident = lambda c: "B%d-C%d-K%d-parts%d-HK%d" % (c.B, c.C, c.K_pool, c.parts, c.HK)


def tail_data(c):
    """The generated case with ref3 = (out, next or None) of the float64 oracle, as label_edge_cases.tail_data makes them (not kept:
    every case here is used once)."""
    d = label_tail_case(c.C, c.NLQ, c.heads, c.dh, c.N5, c.n_out, c.K_pool, c.parts, c.HK, c.B, c.bias)
    d["ref3"] = E.label_tail(d["p"], d["chan"], d["pooled"].max(dim=1).values, d["G"], d["Q"], c.heads, d["next_w"], d["next_b"], terms=3)
    return d


def both(r):
    return r if isinstance(r, tuple) else (r,)


def counters_zero(pk):
    return all(int(ws[2].abs().sum()) == 0 for ws in pk["_cluster_ws"].values())


def test_k_min_is_the_smallest_k_pool_the_predicate_accepts():
    assert smallest_k_pool() == K_MIN


@pytest.mark.parametrize("c", CASES, ids=ident)
def test_cluster_tail_against_the_oracle_repeated_and_against_one_workgroup(c):
    d = tail_data(c)
    sp = ops.pack_weight_bf16_split
    pk, nq, Q, pooled, gp = packed_tail(d, sp), next_query(c, d, sp), dev(d["Q"]), dev(d["pooled"]), sp(dev(d["G"]))
    run = lambda cluster: ops.label_tail_bf16(pooled, gp, Q, c.heads, pk, next_q=nq, terms=3, cluster=cluster)
    first = run(True)
    bounds = [None if r is None else T.TERMS3 * scale(r) for r in d["ref3"]]
    check_tail(first, d["ref3"], bounds, c, "terms = 3, cluster")                                      # (a)
    for _ in range(4):                                                                                 # (b): five launches in all
        for a, b in zip(both(first), both(run(True))):
            assert torch.equal(a, b), "the cluster form must repeat bit for bit"
    assert counters_zero(pk), "cluster counters not re-armed"
    for a, b, r, name in zip(both(first), both(run(False)), d["ref3"], ("out", "next")):               # (c)
        close(a, b.cpu().double(), T.CLUSTER * scale(r), "cluster against single workgroup, " + name)


def test_two_tails_on_two_streams_give_what_they_give_one_after_the_other():
    """(d) The forward launches the object and the place tail on two streams, each with a workspace of its own."""
    sp = ops.pack_weight_bf16_split
    tails = []
    for C in (80, 17):
        c = T.Tail(C, NLQ, HEADS, DH, N5, N_OUT, 2048, 2, 1024, True, 33, ("t3c",))
        d = tail_data(c)
        args = (dev(d["pooled"]), sp(dev(d["G"])), dev(d["Q"]), c.heads, packed_tail(d, sp))
        tails.append((args, next_query(c, d, sp)))
    run = lambda t: ops.label_tail_bf16(*t[0], next_q=t[1], terms=3, cluster=True)
    alone = [run(t) for t in tails]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(5):
        got = []
        for t, s in zip(tails, streams):
            with torch.cuda.stream(s):
                got.append(run(t))
        torch.cuda.synchronize()
        for g, a in zip(got, alone):
            assert torch.equal(g[0], a[0]) and torch.equal(g[1], a[1]), "two tails side by side differ from one after the other"
    assert all(counters_zero(t[0][4]) for t in tails), "cluster counters not re-armed"
