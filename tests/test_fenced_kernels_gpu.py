"""Every wrapper family once more at its edge shapes, into fenced, poisoned buffers (tests/fenced_alloc.py): the fenced run must return
the bits of the plain run, and every fence must be intact afterwards.  The reference comparisons of these same cases live in the edge
files this one takes its tables from (imported as modules); nothing here repeats the float64 work.

A case is a function `fn(put)` that builds its inputs from a fixed seed on the host, moves each to the device with `put`, calls the
wrappers and returns a (nested) tuple of tensors.  `same_bits` runs it plainly, then on a fresh side stream inside `fenced(...)` with
`put` = arena.fence_input: every output, workspace, pack, plan and per-stream scratch is then cut out of a 0xFF-filled buffer between
two 4 KiB fences, and every input sits between fences as well.

Outputs left partly unwritten by design: the bit comparison covers the defined part only (the case returns that part).
  wrapper             tensor       defined region          stated at
  gen_adj(want_csr)   col, val     [0, row_ptr[C])         include/mgnns_hip.h, mgnns_gen_adj: "col/val [C*C] capacity"
  dense_to_csr        col, val     [0, row_ptr[C])         include/mgnns_hip.h, mgnns_dense_to_csr: "col/val capacity C*C"
  sq_mha_plan,        plan         header, group records   mgnns_amd/csrc/sq_mha_plan.hpp, above mg_plan::build: "only the plan[0] records in
  sq_mha_split_plan                [0, plan[0]), samples   use are written ... no consumer reads them" (this sweep's finding: the contract was sound
                                                           but unstated; the comment and the wrappers' docstrings now state it)
zeros_bytes buffers that hold more than counters by their stated contract (arena.check(stateful=...)); the case checks the counter part:
  label_gcn           _scratch     counters = first 256 B  mgnns_amd/ops.py, label_gcn: "counters (first 256 B) start at zero"
  label_gcn           memo state   none (a validity flag)  mgnns_amd/ops.py, label_gcn: "valid = 0: the first launch computes"
"""
import itertools
import math

import numpy as np
import pytest
import torch

from mgnns_amd import images, metrics, ops, optim
from tests import helpers as H
from tests import test_forward_edges_gpu as FWD
from tests.fenced_alloc import fenced

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TALLY = {}


def dev(x):
    return None if x is None else torch.as_tensor(x).to(DEV).contiguous()


def flatten(out):
    if out is None:
        return []
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):                            # a `saved` dict: its tensors in key order (the scalars are the case's own)
        return [t for k in sorted(out) for t in flatten(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in flatten(o)]
    return []


def equal_bits(a, b):
    """Same shape, dtype and bits; NaN positions count as equal only where BOTH runs have NaN (any payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(bits)[~na], b.contiguous().view(bits)[~nb])


def forget_stream(stream):
    """Drop the GEMM workspaces ops.py keeps per (device, stream) for `stream`: the next launch there allocates them again."""
    for cache in (ops._gemm_ws, ops._gemm_bf16_ws):
        for key in [k for k in cache if stream.cuda_stream in k[1:]]:
            del cache[key]


def same_bits(fn, family, stateful=()):
    plain = flatten(fn(dev))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                           # a side stream: the per-stream caches (_gemm_ws, scratch slots) allocate again
    forget_stream(side)                                  # (torch hands its streams out of a pool: an earlier case may have had this one)
    with torch.cuda.stream(side):
        with fenced(ops, metrics, optim, images) as arena:
            got = flatten(fn(lambda x: None if x is None else arena.fence_input(dev(x))))
        side.synchronize()
    forget_stream(side)
    assert len(got) == len(plain) and len(plain) > 0
    for i, (a, b) in enumerate(zip(plain, got)):
        assert equal_bits(a, b), "output %d of %d: the fenced, poisoned run differs from the plain run (%s %s)" % (
            i, len(plain), tuple(a.shape), a.dtype)
    arena.check(stateful=stateful)
    c = arena.counts()
    t = TALLY.setdefault(family, {})
    for k, v in c.items():
        t[k] = t.get(k, 0) + v
    print("fenced[%s]: this case %s; family so far %s" % (family, c, t))
    return arena


def pick(table, idx):
    return [table[i] for i in idx]


# =================================================================================================================================
# Forward, fp32 (tables of tests/test_forward_edges_gpu.py)
# =================================================================================================================================
# one case per tile-count class (1 | 2 | 4 | 7 | 10 | 13), every D tail (4, 24, 316, 300, 320), every mask kind, no biases, B = 0
@pytest.mark.parametrize("L,D,Hn,B,kind,bias", pick(FWD.CORE_CASES, [1, 4, 5, 9, 12, 16, 18, 19, 20]))
def test_sq_mha_core(L, D, Hn, B, kind, bias):
    def fn(put):
        d = [put(t) for t in H.core_case(L, D, Hn, B, kind, bias)]
        o, attn = ops.sq_mha_core(d[0], d[1], d[2], Hn, 128, d[3], d[4], d[5], d[6])
        o2, _ = ops.sq_mha_core(d[0], d[1], d[2], Hn, 128, d[3], d[4], d[5], d[6], want_attn=False)
        return o, attn, o2
    same_bits(fn, "forward fp32")


def test_sq_mha_core_fully_masked_sample():
    def fn(put):
        c = H.core_case(100, 300, 8, 5, "ragged", True)
        c[2][2] = 0                                      # documented NaN probabilities: NaN in both runs, at the same places
        d = [put(t) for t in c]
        return ops.sq_mha_core(d[0], d[1], d[2], 8, 128, d[3], d[4], d[5], d[6])
    same_bits(fn, "forward fp32")


# every bank form at small and large L, dk = 4 | 64 | 128 | 132, B = 0
@pytest.mark.parametrize("L,dk,D,Hn,B,bankk,kind", pick(FWD.FOLDED_CASES, [0, 1, 2, 3, 6, 8, 10, 12, 13]))
def test_sq_mha_folded(L, dk, D, Hn, B, bankk, kind):
    def fn(put):
        qh, bank, mask, wk, _, wv, bv = H.core_case(L, D, Hn, B, kind, True, dk=dk)
        if bankk != "f32":
            padded = torch.zeros(B, L, D if bankk == "bf16" else 320, dtype=torch.bfloat16)
            padded[..., :D] = bank.bfloat16()
            bank = padded
        d = [put(t) for t in (qh, bank, mask, wk, wv, bv)]
        o, attn = ops.sq_mha_folded(d[0], d[1], d[2], Hn, dk, d[3], d[4], d[5])
        o2, _ = ops.sq_mha_folded(d[0], d[1], d[2], Hn, dk, d[3], d[4], d[5], want_attn=False)
        return o, attn, o2
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("HK,B,HK_next", FWD.TAIL_CASES)
def test_mha_tail(HK, B, HK_next):
    def fn(put):
        o, q, w, nxt = FWD.tail_case(HK, B, HK_next)
        d = {k: put(v) for k, v in w.items()}
        packed = {"fc_wp": ops.pack_weight_f32(d["fc_w"]), "w1_wp": ops.pack_weight_f32(d["w1"]), "w2_wp": ops.pack_weight_f32(d["w2"])}
        packed.update({k: d[k] for k in ("fc_b", "g1", "be1", "b1", "b2", "g2", "be2")})
        np_ = None if nxt is None else (ops.pack_weight_f32(put(nxt[0])), put(nxt[1]), HK_next)
        return ops.mha_tail(put(o), put(q), packed, 1e-6, np_)
    same_bits(fn, "forward fp32")


# D around 64, 320 | 321, the limits 2 and 1024; no rows, many rows
@pytest.mark.parametrize("D,rows,kind,eps,bound", pick(FWD.LN_CASES, [0, 2, 3, 4, 5, 7, 8, 10, 11, 14]))
def test_layernorm(D, rows, kind, eps, bound):
    def fn(put):
        x, g, b = FWD.ln_case(D, rows, kind)
        return ops.layernorm(put(x), put(g), put(b), eps)
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("D,NL,B", FWD.HEAD_CASES)
def test_classifier_head_and_its_shares_in_every_order(D, NL, B):
    def fn(put):
        feats, w, b = FWD.head_case(D, NL, B)
        df, dw, db = [put(f) for f in feats], put(w), put(b)
        outs = [ops.classifier_head(df, dw, db)]
        for order in itertools.permutations(range(4)):
            state = ops.classifier_head_state(B, NL, 4, DEV)
            for part in order:
                logits = ops.classifier_head_part(df[part], part, 4, dw, db, state)
            outs.append(logits)
        return outs
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("P,N,K,B", FWD.IMG_CASES)
def test_imgbank_pool_and_transpose_pad(P, N, K, B):
    def fn(put):
        rs = np.random.RandomState(P + N + K + B)
        feat = rs.standard_normal((B, K, P)).astype(np.float32)
        feat[:, ::3] = -np.abs(feat[:, ::3]) - 0.5
        w = (0.05 * rs.standard_normal((N, K))).astype(np.float32)
        bias = (0.05 * rs.standard_normal(N)).astype(np.float32)
        df, db = put(feat), put(bias)
        wt = ops.transpose_pad(put(w), ops.IMGBANK_LDW)
        bank, pooled = ops.imgbank_pool(df, wt, db, N)
        bank2, _ = ops.imgbank_pool(df, wt, None, N, want_pool=False)
        return wt, bank, pooled, bank2
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("mask_kind", ["none", "random", "row"])
@pytest.mark.parametrize("dh,heads,NLQ,B", FWD.LABEL_CASES)
def test_label_attn_core(dh, heads, NLQ, B, mask_kind):
    def fn(put):
        rs = np.random.RandomState(dh + 3 * heads + NLQ + B)
        hid = heads * dh
        Q = rs.standard_normal((NLQ, hid)).astype(np.float32)
        K = (3.0 * rs.standard_normal((B, hid))).astype(np.float32)
        V = rs.standard_normal((B, hid)).astype(np.float32)
        mask = None
        if mask_kind != "none":
            mask = (rs.uniform(size=(B, NLQ, heads, dh)) > 0.3).astype(np.float32)
            if mask_kind == "row" and B:
                mask[B - 1, NLQ - 1, heads - 1] = 0
        return ops.label_attn_core(put(Q), put(K), put(V), heads, put(mask))
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("Hn,dv,B", FWD.HEAD_DIFF_CASES)
def test_head_diff(Hn, dv, B):
    def fn(put):
        rs = np.random.RandomState(Hn + dv + B)
        o = rs.standard_normal((B, Hn, dv)).astype(np.float32)
        if B > 1:
            o[1, Hn - 1] = 0
        return ops.head_diff(put(o.reshape(B, Hn * dv)), Hn)           # H = 1: NaN like the reference, in both runs
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("NL,B", [(1, 1), (2, 1000), (3, 5), (64, 1000), (3, 0), (64, 1)])
def test_predict(NL, B):
    def fn(put):
        rs = np.random.RandomState(NL + B)
        logits = (2.0 * rs.standard_normal((B, NL))).astype(np.float32)
        target = rs.randint(0, NL, size=B).astype(np.int64)
        dl, dt = put(logits), put(target)
        probs, pred = metrics.predict(dl)
        conf = put(np.zeros((NL, NL), np.int32))
        probs2, pred2 = metrics.predict(dl, dt, conf)
        _, pred3 = metrics.predict(dl, dt, conf, want_probs=False)
        return probs, pred, probs2, pred2, pred3, conf
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("kind", ["counts", "zero_row", "all_zero"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 365, 512])
def test_gen_adj_dense_to_csr_and_spmm_csr(C, kind):
    """Both CSR builders, and the CSR product on what they built (with and without the bias kernel, F on both sides of a wave)."""
    def fn(put):
        rs = np.random.RandomState(C)
        counts = rs.randint(0, 40, size=(C, C)).astype(np.float64) * (rs.uniform(size=(C, C)) > 0.5)
        nums = counts.max(1) + rs.randint(1, 20, size=C)
        if kind == "zero_row":
            counts[C // 2] = 0
        elif kind == "all_zero":
            counts[:] = 0
        A = FWD.R.gen_A(counts, nums, 0.4).astype(np.float32)
        dA = put(A)
        plain = ops.gen_adj(dA)
        adj, (rp, col, val) = ops.gen_adj(dA, want_csr=True)
        rp2, col2, val2 = ops.dense_to_csr(adj)
        nnz, nnz2 = int(rp[C]), int(rp2[C])
        outs = [plain, adj, rp, col[:nnz], val[:nnz], rp2, col2[:nnz2], val2[:nnz2]]        # the defined part (table above)
        for F_ in (4, 60, 300):
            x = put(rs.standard_normal((C, F_)).astype(np.float32))
            bias = put(rs.standard_normal((1, 1, F_)).astype(np.float32))
            outs.append(ops.spmm_csr((rp, col, val), x, act=ops.ACT_LRELU2))
            outs.append(ops.spmm_csr((rp2, col2, val2), x, act=ops.ACT_RELU, bias=bias))
        return outs
    same_bits(fn, "forward fp32")


def ragged_csr(N, rs, mean=4.0):
    """tests/test_ops_gpu.py's ragged rows: every 7th row empty, one row longer than the 4-wide gather group."""
    per = rs.poisson(mean, size=N)
    per[::7] = 0
    per[1] = min(N, 23)
    rp = np.zeros(N + 1, np.int32)
    rp[1:] = np.cumsum(per)
    col = np.concatenate([np.sort(rs.choice(N, size=k, replace=False)) for k in per] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, col, rs.uniform(-1.0, 1.0, size=col.size).astype(np.float32)


# the wave-per-row kernel, and the slab kernel (X past 6 MiB) with one slab per pass (F <= 512, ending inside a slab) and two
@pytest.mark.parametrize("N,F_", [(37, 300), (3100, 508), (1540, 1028)])
def test_spmm_csr_both_kernels(N, F_):
    def fn(put):
        rs = np.random.RandomState(N + F_)
        csr = tuple(put(a) for a in ragged_csr(N, rs))
        x, bias = put(rs.standard_normal((N, F_)).astype(np.float32)), put(rs.standard_normal(F_).astype(np.float32))
        out = put(np.zeros((N, F_), np.float32))
        return ops.spmm_csr(csr, x, act=ops.ACT_LRELU2), ops.spmm_csr(csr, x, bias=bias), ops.spmm_csr(csr, x, out=out, act=ops.ACT_RELU)
    same_bits(fn, "forward fp32")


@pytest.mark.parametrize("D,n", [(1, 11), (3, 4 * 8192 + 5), (4, 4 * 8192 + 5), (300, 371), (302, 371), (4, 0)])
def test_embedding(D, n):
    def fn(put):
        rs = np.random.RandomState(D + n)
        V = 97
        table = rs.standard_normal((V, D)).astype(np.float32)
        idx = rs.randint(0, V, size=n).astype(np.int64)
        if n:
            idx[0], idx[-1], idx[n // 2] = 0, V - 1, V - 1        # the table's first and last row: next to both of its fences
        return ops.embedding(put(idx), put(table))
    same_bits(fn, "forward fp32")


def lstm_inputs(B, T, kind, seed=None, V=700, E=300, Hh=150):
    """The text-bank case of tests/test_forward_edges_gpu.py (same seeds), plus "trailing": the last samples empty."""
    rs = np.random.RandomState(B * 131 + T if seed is None else seed)
    emb = torch.from_numpy((0.4 * rs.standard_normal((V, E))).astype(np.float32))
    weights = FWD.lstm_weights(rs, E, Hh)
    lens = {"full": np.full(B, T), "ones": np.ones(B, int), "increasing": 1 + np.arange(B), "decreasing": T - np.arange(B),
            "empty": rs.randint(1, T + 1, size=B), "trailing": rs.randint(1, T + 1, size=B)}[kind].astype(np.int64)
    if kind == "empty":
        lens[0] = 0
        if B > 2:
            lens[B // 2] = 0
        lens[B - 1] = T
    if kind == "trailing":
        lens[0] = T
        lens[B - max(1, B // 3):] = 0
    tok = np.zeros((B, T), np.int64)
    for b in range(B):
        tok[b, :lens[b]] = rs.randint(1, V, size=lens[b])
    return torch.from_numpy(tok), torch.from_numpy(lens), emb, weights


# T on both sides of 128, one and many samples, empty samples at the start, in the middle and at the end
@pytest.mark.parametrize("B,T,kind", pick(FWD.LSTM_CASES, [0, 1, 3, 4, 6, 8, 10]) + [(65, 100, "trailing"), (5, 130, "trailing")])
def test_bilstm_f32(B, T, kind):
    def fn(put):
        tok, lens, emb, weights = lstm_inputs(B, T, kind)
        dw = [tuple(put(t) for t in tup) for tup in weights]
        bank = ops.bilstm(put(tok), put(lens), put(emb), dw, 150, 2)
        bank2, bank_bf = ops.bilstm(put(tok), put(lens), put(emb), dw, 150, 2, want_bf16=True, cache=ops.LstmCache())
        return bank, bank2, bank_bf
    same_bits(fn, "forward fp32")


# M = 0, K and N of one, a 16-byte-unaligned K, and the K-split shape (the GEMM workspace of the side stream comes from the arena)
@pytest.mark.parametrize("M,K,N", [(0, 4, 3), (1, 1, 1), (1, 3, 3), (5, 3, 1), (1023, 1025, 257), (4, 2048, 300), (64, 20154, 7)])
def test_linear_and_matmul(M, K, N):
    def fn(put):
        rs = np.random.RandomState(M + 3 * K + N)
        x = put(rs.standard_normal((M, K)).astype(np.float32))
        w = (rs.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
        dw, dwt = put(w), put(np.ascontiguousarray(w.T))
        b, res = put(rs.standard_normal(N).astype(np.float32)), put(rs.standard_normal((M, N)).astype(np.float32))
        outs = []
        for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU2):
            outs += [ops.linear(x, dw, b, act=act, residual=res), ops.linear(x, dw, None, act=act), ops.matmul(x, dwt, act=act)]
        return outs
    same_bits(fn, "forward fp32")


def pmi_arrays(pmi, put):
    return tuple(None if a is None else put(a) for a in pmi.device_arrays("cpu"))


@pytest.mark.parametrize("form", [1, 2, 3])
def test_textgcn_in_every_launch_form(form):
    """The 1024-thread launch, the two launches (short + long documents) and the lean kernel, on lengths on both sides of the 24-token
    cap, empty and full documents, PADs inside; ngram 4 (the unrolled window) and 0 / 6 (the run-time window)."""
    from mgnns_amd import synth

    def fn(put):
        V, T, B = 5000, 100, 96
        pmi, count = synth.synth_pmi(V, seed=6)
        tok, _, _ = synth.synth_tokens(B, T, V, pmi, seed=12)
        rs = np.random.RandomState(3)
        for b, n in ((2, 24), (3, 25), (4, 0), (5, 100), (6, 1), (7, 23), (8, 26)):
            tok[b] = 0
            tok[b, :n] = rs.randint(2, V, size=n)
        tok[9, ::3] = 0
        nh = put((0.1 * rs.standard_normal((V, 300))).astype(np.float32))
        ew = put(rs.uniform(0.5, 1.5, size=(count, 1)).astype(np.float32))
        arrays, dtok = pmi_arrays(pmi, put), put(tok)
        ops.textgcn_set_form(form)
        try:
            return [ops.textgcn(dtok, nh, ew, arrays, ngram) for ngram in (4, 0, 6)] + [ops.textgcn(put(tok[:0]), nh, ew, arrays, 4)]
        finally:
            ops.textgcn_set_form(0)
    same_bits(fn, "forward fp32")


def test_textgcn_explicit_ids_long_rows_and_odd_width():
    from mgnns_amd.pmi import PmiCsr

    def fn(put):
        V, T, B = 400, 64, 9
        rs = np.random.RandomState(21)
        rows, cols = [], []
        for u in range(2, V):
            k = 120 if u % 7 == 0 else rs.randint(0, 12)
            rows += [u] * k
            cols += list(np.sort(rs.choice(np.arange(2, V), size=k, replace=False)))
        pmi = PmiCsr.from_coo(rows, cols, rs.permutation(np.arange(1, len(rows) + 1)), V)
        tok = rs.randint(2, V, size=(B, T)).astype(np.int64)
        tok[0, :] = 7 * (1 + rs.randint(0, 50, size=T))
        tok[1, 10:] = 0
        tok[2, :] = 0
        arrays, dtok, outs = pmi_arrays(pmi, put), put(tok), []
        assert arrays[2] is not None
        for D in (300, 150, 7):
            nh = put((0.1 * rs.standard_normal((V, D))).astype(np.float32))
            ew = put(rs.uniform(0.5, 1.5, size=(len(rows) + 1, 1)).astype(np.float32))
            outs += [ops.textgcn(dtok, nh, ew, arrays, ngram, max_length=T) for ngram in (4, 6)]
        return outs
    same_bits(fn, "forward fp32")


# =================================================================================================================================
# Forward, bf16 and split-bf16 (tables of tests/test_bf16_edges_gpu.py; shapes of tests/test_ops_gpu.py and tests/test_stress_gpu.py)
# =================================================================================================================================
from tests import test_bf16_edges_gpu as BF  # noqa: E402


def plan_defined(plan, B):
    """The defined part of a packing / group plan (table at the top): header and the plan[0] group records in use, sample records."""
    return plan[:4 + 4 * int(plan[0])], plan[4 + 4 * B:]


def host_bf16(t, ld=ops.BANK_LD):
    out = torch.zeros(*t.shape[:-1], ld, dtype=torch.bfloat16)
    out[..., :t.shape[-1]] = t.to(torch.bfloat16)
    return out


# per form: one case per tile-count class, the chip-filling batch, the D tails the packer takes, every mask kind, B = 0
@pytest.mark.parametrize("form,L,D,Hn,B,kind,bias", [(16,) + c for c in pick(BF.CORE16_CASES, [1, 4, 5, 7, 11, 12, 16, 17])] +
                         [(32,) + c for c in pick(BF.CORE32_CASES, [1, 3, 6, 10, 11, 12, 15, 18, 19])])
def test_sq_mha_core_bf16(form, L, D, Hn, B, kind, bias):
    def fn(put):
        qh, bank, mask, wk, bk, wv, bv = BF.faithful_case(L, D, Hn, B, kind, bias)
        wp = ops.pack_kv_weights_bf16(put(wk.float()), put(wv.float()), Hn, 128, form=form)
        dq, dbank, dm, dbk, dbv = put(qh), put(host_bf16(bank)), put(mask), put(bk), put(bv)
        plans = [None]
        if form == 32 and mask is not None and L <= ops.PLAN_MAX_L:
            plans.append(ops.sq_mha_plan(dm))
        outs = [wp] + [plan_defined(p, B) for p in plans[1:]]
        for plan in plans:
            outs += ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, dbk, dbv, plan=plan)
            outs.append(ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, dbk, dbv, want_attn=False, plan=plan)[0])
        return outs
    same_bits(fn, "forward bf16")


@pytest.mark.parametrize("kind,Hn", [("short16", 8), ("short17", 3), ("short33", 2), ("full128", 8), ("rows_first", 1), ("8_9_16_17", 8),
                                     ("holes", 3), ("only_first_or_last", 2), ("dead", 8), ("one", 8), ("empty", 8)])
def test_sq_mha_plan_and_packed_core(kind, Hn):
    def fn(put):
        rs = np.random.RandomState(sum(map(ord, kind)) + Hn)
        mask = BF.plan_mask(kind, rs)
        B, L = mask.shape
        dm = put(mask)
        plan = ops.sq_mha_plan(dm)
        qh = rs.standard_normal((B, Hn * 128)).astype(np.float32)
        bank = torch.from_numpy((1.2 * rs.standard_normal((B, L, 300))).astype(np.float32))
        wk, wv = ((0.05 * rs.standard_normal((Hn * 128, 300))).astype(np.float32) for _ in range(2))
        bv = rs.standard_normal(Hn * 128).astype(np.float32)
        wp = ops.pack_kv_weights_bf16(put(wk), put(wv), Hn, 128, form=32)
        o, attn = ops.sq_mha_core_bf16(put(qh), put(host_bf16(bank)), dm, Hn, 128, wp, None, put(bv), plan=plan)
        return plan_defined(plan, B), o, attn            # dead samples: NaN in both runs
    same_bits(fn, "forward bf16")


@pytest.mark.parametrize("L,D,Hn,B,kind", pick(BF.FOLDED_CASES, [0, 1, 3, 4, 5, 8, 9, 12, 13, 14]))
def test_sq_mha_folded_bf16(L, D, Hn, B, kind):
    def fn(put):
        rs = np.random.RandomState(L * 1000 + D + 7 * Hn + B)
        u = (0.3 * rs.standard_normal((B, Hn * D))).astype(np.float32)
        bank = torch.from_numpy((1.2 * rs.standard_normal((B, L, D))).astype(np.float32))
        mask = H.make_mask(kind, B, L, rs)
        du, dbank, dm = put(u), put(host_bf16(bank)), put(mask)
        c, attn = ops.sq_mha_folded_bf16(du, dbank, dm, Hn, 128)
        c2, _ = ops.sq_mha_folded_bf16(du, dbank, dm, Hn, 128, want_attn=False)
        return c, attn, c2
    same_bits(fn, "forward bf16")


@pytest.mark.parametrize("form,P,K,N,B,bias", [(1,) + c for c in pick(BF.STREAM_CASES, [0, 1, 3, 4, 5, 7, 8, 10, 11, 12])] +
                         [(2,) + c for c in BF.PAIR_CASES] + [(0, 196, 128, 300, 3, True)])
def test_imgbank_pool_bf16(form, P, K, N, B, bias):
    def fn(put):
        feat, w, b = BF.img_case(P, K, N, B, bias)
        wp = ops.pack_imgbank_weights_bf16(put(w))
        df, db = put(feat), put(b)
        ops.imgbank_set_form(form)
        try:
            bank, pooled = ops.imgbank_pool_bf16(df, wp, db, N)
            bank2, halves = ops.imgbank_pool_bf16(df, wp, db, N, combine=False)
        finally:
            ops.imgbank_set_form(0)
        return wp, bank, pooled, bank2, halves
    same_bits(fn, "forward bf16")


# P with one and two region halves, a ragged last tile, N = 17 | 300 | 304
@pytest.mark.parametrize("B,P,N,K", [(5, 196, 300, 2048), (2, 100, 300, 64), (3, 224, 304, 192), (1, 112, 17, 64)])
def test_imgbank_pool_split(B, P, N, K):
    def fn(put):
        feat, w, b = BF.img_case(P, K, N, B, True)
        pair = ops.pack_weight_bf16_split(put(w))
        df, db = put(feat), put(b)
        outs = list(pair)
        outs += ops.imgbank_pool_split(df, pair, db, N)
        if N % 2 == 0:                                   # (the split images need an even N)
            outs += ops.imgbank_pool_split(df, pair, db, N, want_split=True)
            outs += ops.imgbank_pool_split(df, pair, None, N, want_pool=False, want_f32=False, want_split=True)
        return outs
    same_bits(fn, "forward bf16")


@pytest.mark.parametrize("rows", [0, 1, 1000])
@pytest.mark.parametrize("D,ld", [(1, 8), (7, 8), (8, 8), (1, 320), (300, 320), (320, 320)])
def test_cast_pad_split_pad_and_cast_bf16(D, ld, rows):
    def fn(put):
        rs = np.random.RandomState(D + ld + rows)
        x = (rs.standard_normal(rows * D) * 10.0 ** rs.randint(-20, 20, size=rows * D)).astype(np.float32)
        n = min(x.size, H.BF16_SPECIALS.size)
        x[:n] = H.BF16_SPECIALS.view(np.float32)[:n]
        dx = put(x.reshape(rows, D))
        y = ops.cast_pad_bf16(dx, ld)
        finite = put(np.nan_to_num(x, nan=1.0, posinf=2.0, neginf=-2.0).reshape(rows, D))
        sp = ops.split_pad_bf16(finite, ld) if rows else None          # (the split cast takes no empty input)
        return y.view(torch.int16), sp, ops.cast_bf16(dx).view(torch.int16)         # the casts bit for bit, NaN payloads included
    same_bits(fn, "forward bf16")


def split_core_case(Hn, B, L, rs):
    """test_ops_gpu.py's split-core batches: ragged lengths, holes, a sample whose live rows all lie in the SECOND half (L > 112) and
    one whose live rows all lie in the first."""
    wk, wv = ((0.06 * rs.standard_normal((Hn * 128, 300))).astype(np.float32) for _ in range(2))
    bk, bv = ((0.05 * rs.standard_normal(Hn * 128)).astype(np.float32) for _ in range(2))
    qh = rs.standard_normal((B, Hn * 128)).astype(np.float32)
    bank = (1.5 * rs.standard_normal((B, L, 300))).astype(np.float32)
    lens = np.clip(np.round(np.exp(rs.normal(2.4, 0.75, B))), 1, L).astype(int)
    lens[0] = L
    for i, v in enumerate((1, 16, 17, 32)):
        if i + 1 < B:
            lens[i + 1] = min(v, L)
    m = np.zeros((B, L), np.float32)
    for b in range(B):
        m[b, :lens[b]] = 1
    if L > 112 and B > 3:
        m[2, :] = 0
        m[2, 113:L] = 1
        m[3, :] = 1
        m[3, 50:] = 0
    m[B - 1, ::3] = 0
    m[B - 1, 0] = 1
    return qh, bank, m, wk, bk, wv, bv


# one half (L <= 112) and two (113: one row in the second; 208: both full); 16 heads always split over workgroups; a chip-filling batch
@pytest.mark.parametrize("Hn,B,L", [(3, 7, 112), (8, 7, 113), (16, 5, 208), (1, 2, 1), (8, 300, 112), (4, 9, 37)])
def test_sq_mha_core_split_per_sample_and_grouped(Hn, B, L):
    def fn(put):
        qh, bank, m, wk, bk, wv, bv = split_core_case(Hn, B, L, np.random.RandomState(Hn * 1000 + B + L))
        wp = ops.pack_kv_weights_split(put(wk), put(wv), Hn, 128)
        dq, dm, dbk, dbv = put(qh), put(m), put(bk), put(bv)
        sp = ops.split_pad_bf16(put(bank))
        outs = [wp, sp]
        outs += ops.sq_mha_core_split(dq, sp, dm, Hn, 128, wp, dbk, dbv)
        outs += ops.sq_mha_core_split(dq, sp, None, Hn, 128, wp, dbk, None)
        if L <= ops.SPLIT_PLAN_MAX_L:
            plan = ops.sq_mha_split_plan(dm)
            outs += [plan_defined(plan, B), ops.sq_mha_core_split(dq, sp, dm, Hn, 128, wp, dbk, dbv, want_attn=False, plan=plan)[0]]
            if B > 2:
                m2 = m.copy()
                m2[2, :] = 0                             # a sample without a live row: a NaN output row in both runs
                dm2 = put(m2)
                outs.append(ops.sq_mha_core_split(dq, sp, dm2, Hn, 128, wp, dbk, dbv, want_attn=False, plan=ops.sq_mha_split_plan(dm2))[0])
        return outs
    same_bits(fn, "forward bf16")


def tail_weights(rs, HK, put, hk_next):
    n = lambda *s: (0.05 * rs.standard_normal(s)).astype(np.float32)
    fc, w1, w2, wq = put(n(300, HK)), put(n(300, 300)), put(n(300, 300)), put(n(hk_next, 300))
    pk = {"fc_b": put(n(300)), "g1": put(n(300) + 1), "be1": put(n(300)), "b1": put(n(300)), "b2": put(n(300)), "g2": put(n(300) + 1),
          "be2": put(n(300)), "fc": ops.pack_weight_bf16_split(fc), "w1": ops.pack_weight_bf16_split(w1), "w2": ops.pack_weight_bf16_split(w2)}
    bq = put(n(hk_next))
    return pk, (ops.pack_weight_bf16_split(wq), bq, hk_next), (wq, bq)


# a lone sample, a batch that is no multiple of the 16-sample tile, more tiles than one
@pytest.mark.parametrize("Hn,B", [(1, 1), (4, 37), (8, 257)])
def test_mha_tail_bf16_every_term_cluster_and_ksplit(Hn, B):
    def fn(put):
        rs = np.random.RandomState(5 + Hn + B)
        pk, nx, nlin = tail_weights(rs, Hn * 128, put, Hn * 128)
        o, q = put(rs.standard_normal((B, Hn * 128)).astype(np.float32)), put(rs.standard_normal((B, 300)).astype(np.float32))
        outs = []
        for nxt in (nx, None):                           # the forms tests/test_ops_gpu.py holds against their references
            outs += ops.mha_tail_bf16(o, q, pk, 1e-6, nxt, terms=1, ksplit=False)
            for cluster in (0, 2, 3, 8):
                outs += ops.mha_tail_bf16(o, q, pk, 1e-6, nxt, terms=1, ksplit=True, cluster=cluster)
            outs += ops.mha_tail_bf16(o, q, pk, 1e-6, nxt, terms=3, ksplit=False)
            outs += ops.mha_tail_bf16(o, q, pk, 1e-6, nxt, terms=3, ksplit=True)          # with nxt: the one-launch form
        for cluster in (0, 2, 8):
            outs += ops.mha_tail_bf16(o, q, pk, 1e-6, nx, terms=3, ksplit=True, cluster=cluster, next_linear=nlin)
        return outs
    same_bits(fn, "forward bf16")


@pytest.mark.parametrize("Hn,B", [(1, 5), (4, 16), (8, 37), (8, 257)])
def test_mha_tail_c16_every_cluster_and_ksplit(Hn, B):
    def fn(put):
        rs = np.random.RandomState(11 + Hn + B)
        HD = Hn * 300
        pk, nx, _ = tail_weights(rs, HD, put, HD)
        c = host_bf16(torch.from_numpy(rs.standard_normal((B, HD)).astype(np.float32)), (HD + 31) // 32 * 32)
        dc, q = put(c), put(rs.standard_normal((B, 300)).astype(np.float32))
        outs = []
        for cluster, ksplit in ((1, False), (2, False), (4, False), (0, True), (2, True), (4, True), (8, True)):
            outs += ops.mha_tail_c16(dc, q, pk, 1e-6, nx, cluster=cluster, ksplit=ksplit)
            outs += ops.mha_tail_c16(dc, q, pk, 1e-6, None, cluster=cluster, ksplit=ksplit)
        return outs
    same_bits(fn, "forward bf16")


# fold on and off, the bf16 bank beside the fp32 one; empty samples at the start, in the middle and trailing (the slot of pack_tok that
# prep never writes: tests/test_ops_gpu.py had to poison the workspace by hand to see that one)
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "gemm"])
@pytest.mark.parametrize("B,T,kind", [(1, 1, "full"), (2, 130, "full"), (65, 100, "empty"), (8, 24, "trailing"), (64, 100, "trailing"),
                                      (2, 70, "trailing")])
def test_bilstm_bf16_recurrence(B, T, kind, fold):
    def fn(put):
        tok, lens, emb, weights = lstm_inputs(B, T, kind)
        dw = [tuple(put(t) for t in tup) for tup in weights]
        cache = ops.LstmCache()
        dt, dl, de = put(tok), put(lens), put(emb)
        out, out_bf = ops.bilstm(dt, dl, de, dw, 150, 2, want_bf16=True, recurrence="bf16", cache=cache, fold=fold)
        again = ops.bilstm(dt, dl, de, dw, 150, 2, recurrence="bf16", cache=cache, fold=fold)          # the cached packs and table
        return out, out_bf, again, cache.prepack[2], (cache.table[2] if fold else None)
    same_bits(fn, "forward bf16")


def dense_csr(dense):
    rp = np.concatenate([[0], np.cumsum((dense != 0).sum(1))]).astype(np.int32)
    return rp, np.nonzero(dense)[1].astype(np.int32), dense[dense != 0].astype(np.float32)


@pytest.mark.parametrize("geo", [(8, 10, 128), (8, 20, 128), (4, 10, 256), (4, 20, 256)])
def test_spmm_bf16_tiled_geometries(geo):
    """tests/test_stress_gpu.py's small rectangular problem: empty rows, full rows, counts that are no multiple of the block sizes."""
    def fn(put):
        rs = np.random.RandomState(geo[1])
        n, ncols, F_ = 205, 390, 512
        dense = (rs.rand(n, ncols) < 0.1) * rs.rand(n, ncols)
        dense[7] = 0
        dense[n - 1] = 0
        dense[11, :] = rs.rand(ncols)
        dense[12, :] = rs.rand(ncols)
        adj = ops.SparseAdjBf16(tuple(put(a) for a in dense_csr(dense)), n_cols=ncols)
        X = put(torch.from_numpy(rs.randn(ncols, F_).astype(np.float32)).bfloat16())
        return [adj.val, ops.spmm_bf16(adj, X, out_dtype=torch.float32, path="tiled", geometry=geo),
                ops.spmm_bf16(adj, X, act=ops.ACT_LRELU2, path="tiled", geometry=geo), ops.spmm_bf16(adj, X, out_dtype=torch.float32, path="direct")]
    same_bits(fn, "forward bf16")


# odd feature widths (a partial last slab), an odd number of non-zeros (the values travel as dwords), a single row; the four direct variants
@pytest.mark.parametrize("n,F_,dens", [(37, 200, 0.3), (1, 8, 1.0), (300, 136, 0.02), (64, 1096, 0.1)])
def test_spmm_bf16_direct_variants(n, F_, dens):
    from mgnns_amd import stress

    def fn(put):
        rs = np.random.RandomState(9 + n)
        rp, col, val = stress.random_csr(n, dens, seed=n)
        if col.size % 2 == 0:
            rp, col, val = rp.copy(), col[:-1], val[:-1]
            rp[-1] -= 1
        adj = ops.SparseAdjBf16(tuple(put(np.ascontiguousarray(a)) for a in (rp, col, val)))
        X = put(torch.from_numpy(rs.randn(n, F_).astype(np.float32)).bfloat16())
        outs = [adj.val[:adj.nnz]]
        for var in (0, (1 << 30) | (8 << 4), (1 << 30) | (8 << 4) | 5, (1 << 29) | (2 << 8), (1 << 29) | (3 << 8) | 3):
            outs.append(ops.spmm_bf16(adj, X, out_dtype=torch.float32, path="direct", variant=var))
            outs.append(ops.spmm_bf16(adj, X, act=ops.ACT_RELU, path="direct", variant=var))
        return outs
    same_bits(fn, "forward bf16")


def test_dense_adj_matmul_bf16_at_the_smallest_padded_size():
    def fn(put):
        rs = np.random.RandomState(64)
        C, F_ = 37, 24                                   # K = 37 padded to one 64-wide k-block
        adj = ops.cast_pad_bf16(put(rs.rand(C, C).astype(np.float32)), ld=64)
        return adj, ops.dense_adj_matmul_bf16(adj, put(rs.randn(C, F_).astype(np.float32)), act=ops.ACT_LRELU2)
    same_bits(fn, "forward bf16")


# =================================================================================================================================
# Training (tables of tests/test_train_edges_gpu.py, text_train_edge_cases.py, test_bank_grad_split_gpu.py, test_map_grad_gpu.py)
# =================================================================================================================================
from tests import test_bank_grad_split_gpu as BGS  # noqa: E402
from tests import test_map_grad_gpu as MG  # noqa: E402
from tests import test_train_edges_gpu as TR  # noqa: E402
from tests import text_train_edge_cases as TT  # noqa: E402


# L below a wave per row, on both sides of 64 and at 207 | 208; every mask kind and rate; both width pairs' tails; B = 257
@pytest.mark.parametrize("L,Hn,B,Ddk,rate,kind", pick(TR.CORE_CASES, [0, 1, 2, 3, 5, 7, 9, 10, 13, 14, 17]))
def test_train_mha_attn_and_its_backward(L, Hn, B, Ddk, rate, kind):
    D, dk = Ddk

    def fn(put):
        g, qh, bank, wk, wv, bv, G = TR.core_inputs(B, L, D, Hn, dk, seed=B * 1000 + L * 10 + Hn)
        mask = TR.make_mask(kind, B, L, g)
        d = [put(t) for t in (qh, bank, mask, wk, wv, bv, G)]
        o, attn, saved, keep = ops.mha_attn_train(d[0], d[1], d[2], Hn, dk, d[3], d[4], d[5], 5, rate, return_masks=True)
        grads = ops.mha_attn_train_backward(d[6], d[0], d[1], d[2], d[3], d[4], d[5], saved)
        nodb = ops.mha_attn_train_backward(d[6], d[0], d[1], d[2], d[3], d[4], d[5], saved, want_dbank=False)
        return o, attn, saved, keep, grads, nodb
    same_bits(fn, "training")


@pytest.mark.parametrize("where", ["last", "middle", "all"])
def test_train_mha_attn_with_fully_masked_samples(where):
    def fn(put):
        B, L, D, dk, Hn = 6, 50, 300, 128, 4
        g, qh, bank, wk, wv, bv, G = TR.core_inputs(B, L, D, Hn, dk, seed=17)
        mask = TR.make_mask("ragged", B, L, g)
        mask[{"last": [B - 1], "middle": [2], "all": list(range(B))}[where]] = 0
        d = [put(t) for t in (qh, bank, mask, wk, wv, bv, G)]
        o, attn, saved = ops.mha_attn_train(d[0], d[1], d[2], Hn, dk, d[3], d[4], d[5], 3, 0.0)
        return o, attn, saved, ops.mha_attn_train_backward(d[6], d[0], d[1], d[2], d[3], d[4], d[5], saved)
    same_bits(fn, "training")


@pytest.mark.parametrize("D,rows,rate", TR.LN_CASES)
def test_train_dropout_residual_layernorm_and_its_backward(D, rows, rate):
    def fn(put):
        g = torch.Generator().manual_seed(D * 7 + rows)
        x, res = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
        gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
        dy, dy2 = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
        d = [put(t) for t in (x, res, gamma, beta, dy, dy2)]
        outs = []
        for site in (ops.DROP_FC, ops.DROP_FFN):
            y, saved, keep = ops.dropout_residual_layernorm(d[0], d[1], d[2], d[3], 0.5 if D == 2 else 1e-6, 2 ** 62 + D, site, rate,
                                                            return_masks=True)
            outs += [y, saved, keep, ops.dropout_residual_layernorm_backward(d[4], d[2], saved),
                     ops.dropout_residual_layernorm_backward(d[4], d[2], saved, dy2=d[5])]
        return outs
    same_bits(fn, "training")


@pytest.mark.parametrize("M,NK,bias", TR.WGRAD_CASES)
def test_train_wgrad(M, NK, bias):
    def fn(put):
        g = torch.Generator().manual_seed(M + NK[0] + NK[1])
        return ops.wgrad(put(torch.randn(M, NK[0], generator=g)), put(torch.randn(M, NK[1], generator=g)), bias=bias)
    same_bits(fn, "training")


@pytest.mark.parametrize("B,Hn,dh,NLQ,rate", TR.LABEL_CASES)
def test_train_label_attn_and_its_backward(B, Hn, dh, NLQ, rate):
    def fn(put):
        hid = Hn * dh
        g = torch.Generator().manual_seed(B * 101 + Hn * 11 + dh + NLQ)
        Q, K, V = (put(t) for t in (torch.randn(NLQ, hid, generator=g), torch.randn(B, hid, generator=g), torch.randn(B, hid, generator=g)))
        G = put(torch.randn(B, NLQ, hid, generator=g))
        x, saved, keep = ops.label_attn_train(Q, K, V, Hn, 2 ** 64 - 1 - B, rate, return_masks=True)
        return x, saved, keep, ops.label_attn_train_backward(G, Q, K, V, saved)
    same_bits(fn, "training")


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("B,K,P,N", [c[:4] for c in TR.BANK_CASES] + BGS.WGRAD_SHAPES)
def test_train_imgbank_wgrad(B, K, P, N, split):
    def fn(put):
        g = torch.Generator().manual_seed(B * 31 + K + P + N)
        return ops.imgbank_wgrad(put(torch.rand(B, K, P, generator=g)), put(torch.randn(B, P, N, generator=g)), split=split)
    same_bits(fn, "training")


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("B,K,P,N", BGS.DGRAD_SHAPES)
def test_train_imgbank_dgrad_dense_part(B, K, P, N, split):
    def fn(put):
        g = torch.Generator().manual_seed(B * 1000 + P)
        dbank, W = put(torch.randn(B, P, N, generator=g)), put(torch.randn(N, K, generator=g))
        out = put(torch.full((B, K, P), float("nan")))
        return ops.imgbank_dgrad(dbank, W, out=out, split=split), ops.imgbank_dgrad(dbank, W, split=split)
    same_bits(fn, "training")


@pytest.mark.parametrize("P", [1, 49, 196, 208, 250, 260])
def test_train_map_argmax(P):
    def fn(put):
        return ops.map_argmax(put(MG.tied_map(3, 200, P, seed=P))), ops.map_argmax(put(MG.tied_map(1, 13, max(P, 2), seed=5)))
    same_bits(fn, "training")


@pytest.mark.parametrize("split", [False, True], ids=["f32", "split"])
@pytest.mark.parametrize("B,K,hw,N", [(3, 200, (7, 7), 37), (2, 144, (14, 14), 300), (2, 40, (25, 10), 24), (3, 130, (14, 14), 37)])
def test_train_imgbank_dgrad_scatter(B, K, hw, N, split):
    def fn(put):
        P = hw[0] * hw[1]
        g = torch.Generator().manual_seed(B + K + P)
        x = put(MG.tied_map(B, K, P, seed=K))
        dbank, W, dp = put(torch.randn(B, P, N, generator=g)), put(torch.randn(N, K, generator=g)), put(torch.randn(B, K, generator=g))
        arg = ops.map_argmax(x)
        return arg, ops.imgbank_dgrad(dbank, W, dp, arg, split=split), ops.imgbank_dgrad(None, W, dp, arg, positions=P, split=split)
    same_bits(fn, "training")


@pytest.mark.parametrize("c", TT.LSTM_CASES, ids=TT.lstm_id)
def test_train_bilstm_and_its_backward(c):
    def fn(put):
        d = TT.lstm_data(c)
        names = TT.lstm_flat_names(c.layers)
        ws = [tuple(put(d["sd"][n]) for n in names[4 * i:4 * i + 4]) for i in range(2 * c.layers)]
        emb = put(d["emb"])
        bank, saved = ops.bilstm_train(put(d["tok"]), put(d["lens"]), emb, ws, TT.HID, c.layers, d["seed"], c.rate)
        demb, grads = ops.bilstm_train_backward(put(d["G"]), saved, ws, emb)
        return bank, saved["gates"], saved["cells"], demb, grads
    same_bits(fn, "training")


def tg_inputs(c):
    """tests/text_train_edge_cases.tg_data without its pure-Python winners (the reference's part)."""
    n = TT.TG_CASES.index(c)
    rs = np.random.RandomState(2000 + n)
    pmi, count = TT.synth.synth_pmi(TT.TG_V, per_row=TT.TG_V // 4, seed=n)
    nh = rs.randn(TT.TG_V, c.D).astype(np.float32)
    ew = (rs.randn(count) * 1.3 + 0.2).astype(np.float32)
    nh[8] = nh[7]
    ew[pmi[8, 9]] = ew[pmi[7, 9]]
    kinds = (["random"] * 4 + ["short"] * (c.B - 4)) if c.docs == "big" else list(c.docs)
    tok = np.stack([TT._tg_doc(k, c.T, TT.TG_V, rs) for k in kinds])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(600 + n)
        G = torch.randn(c.B, c.D)
    return tok, nh, ew, pmi, G, 4242 + n


@pytest.mark.parametrize("c", TT.TG_CASES, ids=TT.tg_id)
def test_train_textgcn_and_its_backward(c):
    from mgnns_amd.pmi import PmiCsr

    def fn(put):
        tok, nh, ew, pmi, G, seed = tg_inputs(c)
        arrays = pmi_arrays(PmiCsr.coerce(pmi), put)
        dt, dn, de = put(tok), put(nh), put(ew.reshape(-1, 1))
        out, saved = ops.textgcn_train(dt, dn, de, arrays, c.ngram, c.max_length, seed, c.rate)
        grads = ops.textgcn_train_backward(put(G), dt, dn, de, arrays, saved)
        only_nodes = ops.textgcn_train_backward(put(G), dt, dn, de, arrays, saved, need_edges=False)
        return out, saved["presum"], grads, only_nodes
    same_bits(fn, "training")


@pytest.mark.parametrize("c", TT.KS_CASES, ids=lambda c: "D%d-M%d-%s" % c)
def test_train_keyed_row_sum(c):
    def fn(put):
        d = TT.ks_data(c)
        return ops.keyed_row_sum(put(d["keys"]), put(d["vals"]), d["n_out"], skip_below=d["skip"])
    same_bits(fn, "training")


@pytest.mark.parametrize("K,M", TT.GATHER_CASES)
def test_train_gather_rows(K, M):
    def fn(put):
        rs = np.random.RandomState(K + M)
        n_src = TT.GATHER_N_SRC
        src = rs.standard_normal((n_src, K)).astype(np.float32)
        idx = rs.randint(0, n_src, size=max(M, 4)).astype(np.int32)
        if M >= 1000:
            idx[[0, 500, 999]] = (-1, n_src, -1)         # out of range: a zero row, no read next to the table's fences
            idx[1] = n_src - 1
        elif M == 1:
            idx[0] = n_src if K == 301 else -1
        return ops.gather_rows(put(src), put(idx), M)
    same_bits(fn, "training")


@pytest.mark.parametrize("seed", TR.SEEDS)
@pytest.mark.parametrize("n", [1, 37 * 104, 65537])
def test_train_dropout_its_backward_its_mask_and_eltwise(n, seed):
    def fn(put):
        g = torch.Generator().manual_seed(seed % 1000 + n)
        x, dy = put(torch.randn(n, generator=g)), put(torch.randn(n, generator=g))
        outs = []
        for rate in (0.0, 0.5, 1.0):
            y, keep, kb = ops.dropout(x, seed, ops.DROP_HEAD, rate, return_masks=True)
            outs += [y, keep, kb, ops.dropout_backward(dy, keep, rate), ops.dropout_mask(seed, ops.DROP_FFN, rate, (n,), DEV)]
        for op in (ops.ELT_ADD, ops.ELT_RELU_BWD, ops.ELT_LRELU2_BWD):
            outs.append(ops.train_eltwise(op, x, dy))
        return outs
    same_bits(fn, "training")


# =================================================================================================================================
# Step tail (shapes of tests/test_step_tail_gpu.py)
# =================================================================================================================================
CHUNK = optim.CHUNK


@pytest.mark.parametrize("NL", [1, 7, 64])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_step_tail_ce_loss(B, NL):
    def fn(put):
        rng = np.random.default_rng(1000 * B + NL)
        x = rng.standard_normal((B, NL)).astype(np.float32) * 3
        t = rng.integers(0, NL, B)
        ti = t.copy()
        ti[rng.random(B) < 0.4] = ops.CE_IGNORE_INDEX
        bad = t.copy()
        bad[B - 1] = NL                                  # a NaN loss and a NaN last row: nothing behind the row is touched
        dx = put(x)
        return [ops.ce_loss(dx, put(tt)) for tt in (t, ti, np.full(B, ops.CE_IGNORE_INDEX), bad)]
    same_bits(fn, "step tail")


def test_step_tail_grad_sumsq_and_clip_coef():
    def fn(put):
        rng = np.random.default_rng(9)
        sizes = (1, 3, 5, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 2, 37)
        dev_g = [put(rng.standard_normal(n).astype(np.float32)) for n in sizes]
        table_host = optim.chunk_table([(g, g, g, g) for g in dev_g], [0] * len(dev_g))
        n = table_host.shape[0]
        table = put(table_host)
        partial, out = put(np.full(n, -1.0)), put(np.full(2, -1.0, np.float32))          # exactly n partials and two floats: tight fences
        ops.grad_sumsq(table, n, partial)
        ops.grad_clip_coef(partial, n, 3.0, out)
        return partial, out
    same_bits(fn, "step tail")


@pytest.mark.parametrize("coef", [1.0, 0.25])
def test_step_tail_adam_step_direct_with_tables_of_exactly_the_size_used(coef):
    """ops.adam_step on a chunk table of exactly n records and a scalar table of exactly one row: a read past either meets a fence.
    Sizes: one element, one short of and one past a chunk, three chunks and a tail; a norm-only run (row -1) scaled in place."""
    def fn(put):
        rng = np.random.default_rng(11)
        draw = lambda n: put(rng.standard_normal(n).astype(np.float32))
        sizes = (1, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 2)
        fours = [(draw(n), draw(n), put(np.zeros(n, np.float32)), put(np.zeros(n, np.float32))) for n in sizes]
        only = draw(CHUNK + 7)
        table_host = optim.chunk_table(fours + [(only, only, only, only)], [0] * len(sizes) + [-1])
        table = put(table_host)
        groups = put(np.asarray([optim.group_scalars(1e-2, 0.9, 0.999, 1e-8, 0.01, 1)], np.float32))
        ops.adam_step(table, table_host.shape[0], groups, put(np.asarray([coef], np.float32)))
        return fours, only
    same_bits(fn, "step tail")


# the clip engaged, idle and off; a parameter of CHUNK + 5 elements spans two chunk records, the norm-only one three
@pytest.mark.parametrize("max_norm", [0.5, 1e9, None], ids=["clip", "idle", "off"])
def test_step_tail_adam_step_over_fenced_parameters_gradients_and_moments(max_norm):
    def fn(put):
        rng = np.random.default_rng(3)
        draw = lambda n: put(rng.standard_normal(n).astype(np.float32))
        sizes = (CHUNK + 5, 3, 2 * CHUNK + 1, 37, CHUNK)
        params = [torch.nn.Parameter(draw(n)) for n in sizes]
        inside, outside = [params[0], params[1], params[3], params[4]], params[2]
        opt = optim.Adam([dict(params=inside[:2], lr=1e-2, weight_decay=0.01), dict(params=inside[2:], lr=1e-3)], max_norm=max_norm,
                         norm_params=[outside] + inside)
        for p in inside:                                 # the moment buffers between fences too: a store past a chunk's end lands in one
            opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=put(np.zeros(p.numel(), np.float32)), exp_avg_sq=put(np.zeros(p.numel(), np.float32)))
        outs = []
        for s in range(2):
            for p in params:
                p.grad = draw(p.numel())
            opt.step()
            outs += [p.grad.clone() for p in params]
            if max_norm is not None:
                outs += [opt.total_norm.clone(), opt.clip_coef.clone()]
        outs += [p.detach() for p in params]
        outs += [opt.state[p][k] for p in inside for k in ("exp_avg", "exp_avg_sq")]
        return outs
    same_bits(fn, "step tail")


# =================================================================================================================================
# Label channel (tables of tests/label_edge_cases.py)
# =================================================================================================================================
from tests import label_edge_cases as LBL  # noqa: E402
from tests import test_label_edges_gpu as LBLG  # noqa: E402

label_id = lambda c: "-".join(str(v) for v in c[:11])


def label_case(c):
    """The inputs of tests/label_edge_cases.tail_data without its float64 references."""
    d = dict(H.label_tail_case(c.C, c.NLQ, c.heads, c.dh, c.N5, c.n_out, c.K_pool, c.parts, c.HK, c.B, c.bias))
    if "x" in c.forms:
        d["x"] = (d["pooled"].double().max(dim=1).values @ d["G"].double().t()).float()
    return d


def label_packed(d, pack, put):
    w = LBL.tail_weights(d)
    wc, bc = LBLG.composed(d)
    return {"wk": pack(put(w["wk"])), "bk": put(w["bk"]), "wv": pack(put(w["wv"])), "bv": put(w["bv"]), "wc": pack(put(wc)), "bc": put(bc),
            "n5": wc.shape[0], "C": w["wk"].shape[1], "xl": pack(put(w["wxl"])), "bxl": put(w["bxl"]), "n_out": w["wxl"].shape[0]}


def label_next(c, d, pack, put):
    return None if not c.HK else (pack(put(d["next_w"])), put(d["next_b"]) if c.bias else None, c.HK)


@pytest.mark.parametrize("c", LBL.TAIL_X_CASES + LBL.TAIL_POOL_CASES, ids=label_id)
def test_label_tail(c):
    def fn(put):
        d = label_case(c)
        pk, nq, Q = label_packed(d, ops.pack_weight_f32, put), label_next(c, d, ops.pack_weight_f32, put), put(d["Q"])
        if "x" in c.forms:
            return ops.label_tail(put(d["x"]), Q, c.heads, pk, next_q=nq)
        g_wp = ops.pack_weight_f32(put(d["G"]))
        return g_wp, ops.label_tail(None, Q, c.heads, pk, pooled=put(d["pooled"]), g_wp=g_wp, next_q=nq)
    same_bits(fn, "label channel")


@pytest.mark.parametrize("c", LBL.TAIL_BF16_CASES, ids=label_id)
def test_label_tail_bf16_each_terms_and_cluster(c):
    def fn(put):
        d = label_case(c)
        sp = ops.pack_weight_bf16_split
        pk, nq, Q, pooled, gp = label_packed(d, sp, put), label_next(c, d, sp, put), put(d["Q"]), put(d["pooled"]), sp(put(d["G"]))
        outs = list(gp)
        for form in c.forms:
            terms, cluster = (1, False) if form == "t1" else (3, form == "t3c")
            for _ in range(2):                           # twice: the cluster's counters re-arm themselves (arena.check holds them to zero)
                outs.append(ops.label_tail_bf16(pooled, gp, Q, c.heads, pk, next_q=nq, terms=terms, cluster=cluster))
        return outs
    same_bits(fn, "label channel")


@pytest.mark.parametrize("split", [False, True], ids=["exact", "split"])
@pytest.mark.parametrize("c", LBL.GCN_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_label_gcn_every_grid_with_and_without_a_memo(c, split):
    def fn(put):
        d = LBL.gcn_data(c)
        A, inp = put(d["A"]), put(d["inp"])
        packed = ops.label_gcn_pack(put(d["w1"]), put(d["w2"]), split=split)
        query = None if d["query"] is None else tuple(put(t) for t in d["query"])
        outs = [packed["w1"], packed["w2"]]
        for grid in LBL.GCN_GRIDS:
            outs.append(ops.label_gcn(A, inp, packed, want_packed_g=c.packed, query=query, grid=grid))
            # the scratch holds the launch's intermediates behind its counters (table at the top): the counters are re-armed
            assert all(int(ws[:256].view(torch.int32).abs().sum()) == 0 for ws in packed["_scratch"].values())
        memo = {}
        inp2 = put(d["inp"] * 1.5)
        for x in (inp, inp, inp2, inp2, inp):            # miss, hit, miss, hit, miss: a memo launch returns the memo's own buffers
            r = ops.label_gcn(A, x, packed, want_packed_g=c.packed, query=query, memo=memo)
            outs.append([None if t is None else t.clone() for t in flatten(r)])
            outs.append(torch.tensor([ops.label_gcn_memo_flag(memo, want_packed_g=c.packed)]))
        return outs
    same_bits(fn, "label channel", stateful=("label_gcn",))
