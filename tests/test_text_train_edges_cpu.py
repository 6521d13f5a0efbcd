"""The text encoders' training edge sweep, the part that needs no GPU: the extended oracles of tests/text_train_edge_cases.py against
independent statements of the same operations (oracle.restatement.text_gcn_doc; torch.nn.LSTM in float64 over packed sequences), the
masks at the two extreme rates, the tables' axis coverage, the float32-CPU error of every reference against the gate the GPU file
asserts, and a Python restatement of the text GCN's shape limits against the library's exported predicate
(mgnns_textgcn_train_supported, a host function: the library loads and answers without a device)."""
import itertools

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from mgnns_amd import _lib
from oracle import restatement as R
from tests import dropout_ref as DR
from tests import helpers as H
from tests import text_train_edge_cases as T
from tests.test_text_train_cpu import lstm_keep, textgcn_keep, tg_oracle_doc, tg_winners


# ---- the text GCN oracle ---------------------------------------------------------------------------------------------------------------
DOCS = {"repeat": [11] * 40, "distinct": list(range(2, 42)), "padin": [5, 6, 0, 7, 5, 0, 9, 6, 6, 10, 0, 0, 3], "one": [3], "empty": [],
        "tie": [7, 9, 8, 4, 4, 12, 7], "long": list(range(2, 30)) * 3}


@pytest.mark.parametrize("kind", sorted(DOCS))
@pytest.mark.parametrize("ngram", [0, 1, 3, 15])
def test_text_gcn_oracle_equals_the_restatement_at_every_ngram(kind, ngram):
    rs = np.random.RandomState(1)
    pmi, count = T.synth.synth_pmi(48, per_row=12, seed=0)
    nh = rs.randn(48, 9).astype(np.float32)
    ew = (rs.randn(count) * 1.5).astype(np.float32)
    for max_length in (100, 25, 1):                                 # 25 and 1 < len for the long kinds
        got = tg_oracle_doc(DOCS[kind], nh, ew, pmi, ngram, max_length=max_length)
        ref = R.text_gcn_doc(DOCS[kind], nh, ew, pmi, ngram, max_length=max_length)
        np.testing.assert_array_equal(got, ref)


def test_text_gcn_oracle_clamps_ids_like_the_kernels_and_matches_the_restatement_per_document():
    """tg_oracle on raw ids == tg_oracle on pre-clamped ids == the restatement of the clamped documents (rate 0, all signs from the
    sums themselves); a negative id is dropped like PAD, ids V and V + 7 read row V - 1."""
    c = T.TG_CASES[1]
    d = T.tg_data(c)
    assert (d["tok"] >= T.TG_V).sum() == 2 and (d["tok"] < 0).sum() == 1
    ones = torch.ones(c.B, c.D)
    with torch.no_grad():
        raw = T.tg_oracle(d["tok"], d["nh"], d["ew"], d["pmi"], c.ngram, c.max_length, ones, 1, 0.0)[0]
        pre = T.tg_oracle(d["tok_c"], d["nh"], d["ew"], d["pmi"], c.ngram, c.max_length, ones, 1, 0.0, d["winners"])[0]
    assert torch.equal(raw, pre)
    ref = R.text_gcn(d["tok_c"], d["nh"], d["ew"], d["pmi"], c.ngram, c.max_length)
    assert H.maxerr(torch.relu(raw), ref) <= 1e-5 * H.scale(ref)    # the restatement adds in float32
    oob_doc = d["kinds"].index("oob")
    assert T.TG_V - 1 in d["winners"][oob_doc][3] and 0 not in d["winners"][oob_doc][3]


@pytest.mark.parametrize("c", [c for c in T.TG_CASES if "tie" in c.docs], ids=T.tg_id)
def test_the_tie_documents_do_tie_and_the_earlier_position_wins(c):
    d = T.tg_data(c)
    nodes, win, _, t = d["winners"][d["kinds"].index("tie")]
    nh, ew, pmi = d["nh"], d["ew"], d["pmi"]
    assert t[:3] == [7, 9, 8]
    k = nodes.index(9)
    p7 = np.float32(ew[pmi[7, 9]]) * nh[7]
    cands = [i for i in range(len(t)) if any(t[j] == 9 for j in range(max(0, i - c.ngram), min(len(t), i + c.ngram + 1)))]
    tied = p7 == np.max(np.stack([np.float32(ew[pmi[t[i], 9]]) * nh[t[i]] for i in cands]), axis=0)
    assert tied.any(), "the constructed document has no cross-token tie"
    assert (win[k][tied] == 0).all()                                # position 0 (token 7) beats position 2 (token 8)


# ---- the LSTM oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,E", [(1, 1), (2, 1), (1, 7), (2, 7), (1, 300), (2, 300)])
def test_lstm_oracle_equals_torch_lstm_over_packed_sequences(layers, E):
    """Bank and gradients (embedding, every weight and bias) in float64 at rate 0, lengths 0 excluded (pack_padded_sequence takes none);
    ids in range with PAD inside a length."""
    torch.manual_seed(layers * 10 + E)
    B, T_len, V = 6, 9, 20
    lstm = torch.nn.LSTM(E, T.HID, layers, bidirectional=True, batch_first=True).double()
    emb = torch.nn.Embedding(V, E, padding_idx=0).double()
    lens = torch.tensor([9, 1, 4, 9, 2, 7])
    tok = torch.randint(1, V, (B, T_len))
    tok[:, 3] = 0
    for b in range(B):
        tok[b, lens[b]:] = 0
    G = torch.randn(B, T_len, 2 * T.HID, dtype=torch.float64)
    packed = pack_padded_sequence(emb(tok), lens, batch_first=True, enforce_sorted=False)
    want = pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=T_len)[0]
    (want * G).sum().backward()
    names = T.lstm_flat_names(layers)
    e2 = emb.weight.detach().clone().requires_grad_()
    flat = [getattr(lstm, n).detach().clone().requires_grad_() for n in names]
    got = T.lstm_oracle(tok, lens, e2, flat, 0, 0.0, layers)
    (got * G).sum().backward()
    assert H.maxerr(got, want.detach()) <= 1e-12
    assert H.maxerr(e2.grad, emb.weight.grad) <= 1e-11 * max(1.0, H.scale(emb.weight.grad))
    assert float(e2.grad[0].abs().max()) == 0.0
    for n, p in zip(names, flat):
        assert H.maxerr(p.grad, getattr(lstm, n).grad) <= 1e-11 * max(1.0, H.scale(getattr(lstm, n).grad)), n


def test_lstm_oracle_clamps_lengths_and_ids():
    """lens T + 5 -> T, -3 -> 0; ids V and V + 7 -> V - 1, -3 -> 0 (and no gradient for it): the oracle on raw inputs equals the oracle
    on pre-clamped ones, and row V - 1 carries a gradient."""
    c = next(c for c in T.LSTM_CASES if c.lens == "clamped" and c.ids == "oob")
    d = T.lstm_data(c)
    assert int((d["lens"] > c.T).sum()) and int((d["lens"] < 0).sum()) and len(d["oob"]) == 3
    run = lambda tok, lens: T.lstm_oracle(tok, lens, d["emb"].double(), [d["sd"][k].double() for k in T.lstm_flat_names(c.layers)],
                                          d["seed"], c.rate, c.layers)
    assert torch.equal(run(d["tok"], d["lens"]), run(d["tok_c"], d["lens_c"]))
    demb = T.lstm_ref(c)[1]
    assert float(demb[T.LSTM_V - 1].abs().max()) > 0 and float(demb[0].abs().max()) == 0.0
    assert float(demb[40:T.LSTM_V - 1].abs().max()) == 0.0         # ids that never occur


# ---- the masks at the extreme rates --------------------------------------------------------------------------------------------------------
def test_rate_one_drops_everything_and_a_rate_below_the_resolution_keeps_everything():
    assert DR.scale(1.0) == 0.0 and DR.scale(T.TINY_RATE) == 1.0 and np.float32(T.TINY_RATE) > 0
    for c in T.LSTM_CASES:
        if c.rate in (1.0, T.TINY_RATE):
            k = lstm_keep(T.lstm_data(c)["seed"], c.rate, c.B, c.T, 2 * T.HID)
            assert k.all() if c.rate < 1.0 else not k.any(), c
    assert not textgcn_keep(99, 1.0, 64, 300).any() and textgcn_keep(99, T.TINY_RATE, 64, 300).all()
    # the one element a rate below 2^-24 could still drop is u == 0; at rate 1 even the largest u is dropped
    assert not DR.keep(DR.seed_for(5, 17, 0), 5, np.array([17]), T.TINY_RATE)[0]
    assert not DR.keep(DR.seed_for(5, 17, (1 << 64) - 1), 5, np.array([17]), 1.0)[0]


# ---- every value of every axis appears ---------------------------------------------------------------------------------------------------
def test_every_value_of_every_axis_appears():
    seen = lambda cases, f: {getattr(c, f) for c in cases}
    l = T.LSTM_CASES
    assert seen(l, "T") == {1, 2, 33, 130, 230} and seen(l, "E") == {1, 7, 300, 304, 324} and seen(l, "layers") == {1, 2}
    assert seen(l, "B") == {1, 2, 7, 65, 1025, 4097} and all(c.T == 2 for c in l if c.B > 1024)
    assert seen(l, "lens") == {"full", "edges", "flush", "clamped", "efml"} and all(c.T >= 65 for c in l if c.lens == "flush")
    assert seen(l, "ids") == {"pad", "oob"} and seen(l, "rate") == {0.0, 0.5, 1.0, T.TINY_RATE}
    assert {c.layers for c in l if c.rate == 1.0} == {2}
    for c in l:
        d = T.lstm_data(c)
        if c.lens == "flush":
            assert set(d["lens"].tolist()) == set([31, 32, 33, 64, 65][:c.B])
        if c.lens == "efml":
            assert d["lens"][0] == d["lens"][c.B // 2] == d["lens"][-1] == 0 and int((d["lens"] > 0).sum()) == c.B - 3
        if c.T > 1:
            inside = torch.arange(c.T)[None, :] < d["lens_c"][:, None]
            assert int(((d["tok_c"] == 0) & inside).sum()) > 0, "no PAD inside a length"
    g = T.TG_CASES
    assert seen(g, "ngram") == {0, 1, 3, 15} and seen(g, "D") >= {1, 7, 63, 64, 65, 300, 320}
    assert {k for c in g if c.docs != "big" for k in c.docs} >= {"empty", "one", "repeat", "distinct", "padin", "tie", "oob"}
    assert all(c.B <= 4 for c in g if c.docs != "big") and [c for c in g if c.docs == "big"] == [T.Tg(256, 100, 100, 15, 8, "big", 0.5)]
    assert any(c.max_length < c.T for c in g) and seen(g, "rate") == {0.0, 0.5}
    big = g[-1]
    assert big.B * min(big.T, big.max_length) * (2 * big.ngram + 1) > T.KS_CAP
    k = T.KS_CASES
    assert seen(k, "D") == {1, 2, 63, 64, 257} and seen(k, "M") == {1, 262144, 262145, 300000}
    assert seen(k, "pattern") == {"single", "distinct", "span", "skip", "oob"} and T.Ks(1, 300000, "single") in k
    assert {K for K, _ in T.GATHER_CASES} == {1, 300, 301} and {M for _, M in T.GATHER_CASES} == {0, 1, 1000}


def test_the_keyed_sum_cases_are_what_their_patterns_say():
    for c in T.KS_CASES:
        d = T.ks_data(c)
        sk = np.sort(d["keys"].numpy(), kind="stable")
        runs = d["runs"]
        assert d["ref"].shape == (d["n_out"], c.D) and (d["bound"][d["hit"]] > 0).all() and (d["bound"][~d["hit"]] == 0).all()
        assert ((runs <= 2) | (runs >= 300)).all(), "a run length the bound is not made for (see the case table)"
        if c.pattern == "single":
            assert runs.max() == c.M and int(d["hit"].sum()) == 1
        elif c.pattern == "distinct":
            assert runs.max() == 1 and d["hit"].all()
        elif c.pattern == "span":
            lo = int(np.searchsorted(sk, sk[T.KS_CAP]))
            hi = int(np.searchsorted(sk, sk[T.KS_CAP], side="right"))
            assert (lo, hi) == (T.KS_CAP - 150, T.KS_CAP + 150) and not d["hit"][-1]
        elif c.pattern == "skip":
            assert d["skip"] == 3 and (sk < 3).sum() > 0 and not d["hit"][:3].any() and d["hit"][3:40].all() and not d["hit"][40]
        else:
            assert d["n_out"] + 3 in sk and (c.M == 1 or (d["n_out"] in sk and d["hit"].all()))


# ---- the float32-CPU error of each reference --------------------------------------------------------------------------------------------------
def _report(names, ref, f32):
    worst = 0.0
    for n, r, a in zip(names, ref, f32):
        err, sc = H.maxerr(a, r), H.scale(r)
        print("%s: scale %.3e, float32-CPU error %.3e, gate %.3e" % (n, sc, err, T.GATE * sc))
        assert 4 * err <= T.GATE * sc, "%s: 4 x the float32-CPU error %.3e is past the gate %.3e" % (n, err, T.GATE * sc)
        worst = max(worst, err / sc if sc else 0.0)
    print("worst relative float32-CPU error %.2e (a quarter of the gate: %.2e)" % (worst, T.GATE / 4))


@pytest.mark.parametrize("c", T.LSTM_CASES, ids=T.lstm_id)
def test_lstm_references_stay_within_a_quarter_of_the_gate_in_float32(c):
    ref = T.lstm_ref(c)
    assert all(torch.isfinite(r).all() for r in ref) and len(ref) == 2 + 8 * c.layers
    d = T.lstm_data(c)
    pad = torch.arange(c.T)[None, :] >= d["lens_c"][:, None]
    assert float(ref[0][pad].abs().max() if pad.any() else 0.0) == 0.0
    if c.rate == 1.0:                                               # layer 0 and the embedding: exactly zero; layer 1 is not
        assert all(float(r.abs().max()) == 0.0 for r in ref[1:10])
        assert all(H.scale(r) > 0 for r in ref[11:14] + ref[15:18]) and H.scale(ref[10]) == H.scale(ref[14]) == 0.0     # (its input is zero)
    else:                                                           # (a chain of one step has no recurrent input: d weight_hh is zero)
        assert all(H.scale(r) > 0 for n, r in zip(T.lstm_names(c), ref) if "weight_hh" not in n or int(d["lens_c"].max()) > 1)
    _report(T.lstm_names(c), ref, T.lstm_run_ref(c, torch.float32))


@pytest.mark.parametrize("c", T.TG_CASES, ids=T.tg_id)
def test_text_gcn_references_stay_within_a_quarter_of_the_gate_in_float32(c):
    ref = T.tg_run_ref(c, torch.float64)
    assert all(torch.isfinite(r).all() and H.scale(r) > 0 for r in ref)
    d = T.tg_data(c)
    absent = np.setdiff1d(np.arange(T.TG_V), d["tok_c"][:, :min(c.T, c.max_length)])
    assert float(ref[1][absent].abs().max()) == 0.0 and float(ref[1][0].abs().max()) == 0.0
    if any(k == "oob" for k in d["kinds"]):                         # the clamped ids' gradient lands on row V - 1
        assert float(ref[1][T.TG_V - 1].abs().max()) > 0
    _report(("out", "node_hidden", "edge weights"), ref, T.tg_run_ref(c, torch.float32))


# ---- the text GCN's shape predicate ----------------------------------------------------------------------------------------------------------
def ask(T_len, D, ngram, max_length):
    return bool(_lib.lib().mgnns_textgcn_train_supported(T_len, D, ngram, max_length)), T.tg_train_ok(T_len, D, ngram, max_length)


def test_the_restated_predicate_equals_the_librarys_on_a_grid_of_every_limit_and_its_successor():
    n = 0
    for ngram in range(-1, 17):
        lim = T.tg_tm_max(min(max(ngram, 0), 15))
        for T_len, D, ml in itertools.product((0, 1, lim - 1, lim, lim + 1, 8191, 8192, 32767, 32768), (0, 1, 64, 320, 321),
                                              (0, 1, lim, lim + 1, 10 ** 6)):
            lib, mine = ask(T_len, D, ngram, ml)
            assert lib == mine, (T_len, D, ngram, ml, lib, mine)
            n += 1
    print("%d grid points" % n)


def test_the_limits_are_the_ones_the_formula_gives():
    """Unstaged, the backward needs Tm (28 W + 12) + 16 bytes (W = 2 ngram + 1: 8 W of band, 12 of token chains, 20 W of the five
    waves' slot sums): 186 at ngram 15 and 4095 at ngram 0 are the largest Tm accepted, whatever D; the forward alone (no slot sums)
    would take 630 and 8191, the gap in which a step used to die in backward()."""
    assert T.tg_tm_max(15) == 186 and T.tg_tm_max(0) == 4095
    for ngram, lim, fwd in ((15, 186, 630), (0, 4095, 8191)):
        W = 2 * ngram + 1
        assert T.tg_lds(lim, W, 320, False, True) <= T.LDS < T.tg_lds(lim + 1, W, 320, False, True)
        assert T.tg_lds(fwd, W, 320, False, False) <= T.LDS < T.tg_lds(fwd + 1, W, 320, False, False)
        for D in (1, 320):
            assert ask(lim, D, ngram, 10 ** 6) == (True, True) and ask(lim + 1, D, ngram, 10 ** 6) == (False, False)
            assert ask(10 ** 6, D, ngram, lim) == (True, True) and ask(10 ** 6, D, ngram, lim + 1) == (False, False)


def test_every_gpu_case_is_accepted_every_refusal_rejected_and_the_staging_is_what_the_tables_say():
    for i, c in enumerate(T.TG_CASES):
        assert ask(c.T, c.D, c.ngram, c.max_length) == (True, True), c
        Tm = min(c.T, c.max_length)
        if i in T.TG_STAGING:
            assert (T.tg_staged(Tm, c.ngram, c.D, False), T.tg_staged(Tm, c.ngram, c.D, True)) == T.TG_STAGING[i], c
        # the eval kernel (it always stages) takes all of them but the one with both kernels unstaged; the rate-0 cases, which are
        # compared with it at 1e-6, are the ones whose documents have at most 40 nodes: two fp32 sums of n positive terms in different
        # orders differ by about sqrt(n) roundings of the running sum, and at n >= 100 (the long cases, measured on the GPU at rate 0:
        # 1.02e-6 and 1.04e-6 of the output's scale at 100 and 186 nodes) fp32 itself no longer meets 1e-6
        assert T.tg_eval_fits(Tm, c.D, c.ngram) == (T.TG_STAGING.get(i) != (False, False)), c
        if c.rate == 0.0:
            assert T.tg_eval_fits(Tm, c.D, c.ngram) and max(len(w[0]) for w in T.tg_data(c)["winners"]) <= 40, c
    assert set(T.TG_STAGING.values()) == {(True, True), (True, False), (False, False)}
    assert T.TG_CASES[4].ngram == 15 and min(T.TG_CASES[4].T, T.TG_CASES[4].max_length) == T.tg_tm_max(15)
    for what, T_len, D, ngram, ml, _msg in T.TG_REFUSALS:
        assert ask(T_len, D, ngram, ml) == (False, False), what
