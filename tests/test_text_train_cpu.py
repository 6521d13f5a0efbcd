"""Training mode of the text encoders, the parts that need no GPU: the opt-in surface (unfreeze_text_encoders), the refusals that
stay, the two new dropout sites' masks (restated on the host from their documented layouts), and the text GCN oracle the GPU
tests use -- winners by the tie rule (the first in-edge in add_seq_edges order whose fp32 product equals the fp32 max: the smallest
source position), whose forward must equal oracle.restatement.text_gcn_doc."""
import numpy as np
import pytest
import torch

from mgnns_amd import synth
from oracle import restatement as R
from tests import dropout_ref as DR
from tests import helpers as H
from tests.model_util import build_model

DROP_LSTM, DROP_TEXT_GCN = 5, 6


def lstm_index(B, T, H2):
    """DROP_LSTM over [B, T, 2H]: idx = (b*T + t)*2H + j."""
    b, t, j = np.meshgrid(np.arange(B), np.arange(T), np.arange(H2), indexing="ij")
    return (b * T + t) * H2 + j


def lstm_keep(seed, rate, B, T, H2=300):
    return DR.keep(seed, DROP_LSTM, lstm_index(B, T, H2), rate)


def textgcn_keep(seed, rate, B, D):
    return DR.keep(seed, DROP_TEXT_GCN, DR.rows_index(B, D), rate)


def tg_winners(ids, node_hidden, edge_w, pmi, ngram, max_length=100):
    """One document -> (nodes: token ids in first-occurrence order, winners [n_nodes, D]: the source POSITION (in the compacted
    token list) of each (node, feature)'s winning in-edge, edge ids [n_nodes, D], tokens t).  Products in fp32."""
    ids = [int(x) for x in ids][:max_length]
    t = [x for x in ids if x != 0]
    D = node_hidden.shape[1]
    nodes = []
    for v in t:
        if v not in nodes:
            nodes.append(v)
    win = np.zeros((len(nodes), D), np.int64)
    eid = np.zeros((len(nodes), D), np.int64)
    for k, v in enumerate(nodes):
        # in-edges of v in add_seq_edges order: source position ascending; within a source its window edges, then its self loop
        cands = []
        for i, u in enumerate(t):
            if any(t[j] == v for j in range(max(0, i - ngram), min(i + ngram + 1, len(t)))) or u == v:
                cands.append(i)
        prods = np.stack([np.float32(edge_w[pmi[t[i], v]]) * node_hidden[t[i]].astype(np.float32) for i in cands])
        mx = prods.max(axis=0)
        first = np.argmax(prods == mx[None, :], axis=0)       # first candidate reaching the max
        win[k] = np.asarray(cands)[first]
        eid[k] = [pmi[t[i], v] for i in win[k]]
    return nodes, win, eid, t


def tg_oracle_doc(ids, node_hidden, edge_w, pmi, ngram, max_length=100):
    """fp32 forward of one document through the winners: relu(sum over nodes of w[e] h[u])."""
    nodes, win, eid, t = tg_winners(ids, node_hidden, edge_w, pmi, ngram, max_length)
    D = node_hidden.shape[1]
    out = np.zeros(D, np.float32)
    for k in range(len(nodes)):
        src = np.asarray(t)[win[k]]
        out += np.float32(edge_w[eid[k]]) * node_hidden[src, np.arange(D)]
    return np.maximum(out, 0.0)


def _model(cfg_name="mvsa_single_b8"):
    cfg = synth.CONFIGS[cfg_name]
    pmi, count = synth.synth_pmi(cfg.V, seed=3)
    adj = H.load_golden("adjacency.npz")
    return build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], np.zeros((7, 300), np.float32))


def test_unfreeze_and_freeze_round_trip():
    m = _model("mvsa_multiple_b256")
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert len(shapes) == 249                                   # (three layers per fusion stack)
    assert m.text_encoders_trainable is False
    assert m.train().unfreeze_text_encoders() is m
    assert m.text_encoders_trainable is True
    for n in m.TEXT_ENCODERS:
        assert all(p.requires_grad for p in getattr(m, n).parameters()), n
    m._refuse_untrainable()                                    # training mode is allowed with the encoders live
    assert m.freeze_text_encoders() is m
    assert m.text_encoders_trainable is False
    for n in m.TEXT_ENCODERS:
        assert not getattr(m, n).training
        assert not any(p.requires_grad for p in getattr(m, n).parameters()), n
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes


def test_refusals_that_stay_with_the_flag_on():
    m = _model()
    m.train().unfreeze_text_encoders()
    m.set_precision('bf16')
    with pytest.raises(NotImplementedError, match="fp32 only"):
        m._refuse_untrainable()
    m.set_precision('fp32')
    m.is_regu = True
    with pytest.raises(NotImplementedError, match="is_regu"):
        m._refuse_untrainable()
    m.is_regu = False
    m.freeze_text_encoders().lstm.train()
    with pytest.raises(RuntimeError, match="eval.*freeze_text_encoders"):     # flag off: today's refusal
        m._refuse_untrainable()


def test_text_gcn_training_forward_is_gpu_only():
    m = _model()
    tg = m.text_features.train()
    with pytest.raises(RuntimeError, match="GPU only"):
        tg(torch.ones(2, 5, dtype=torch.int64))


@pytest.mark.parametrize("site,layout", [(DROP_LSTM, "lstm"), (DROP_TEXT_GCN, "rows")])
@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_new_sites_keep_binomial_fractions_and_are_independent(site, layout, rate):
    seed = 1234567
    idx = lstm_index(16, 20, 300) if layout == "lstm" else DR.rows_index(256, 300)
    k = DR.keep(seed, site, idx, rate)
    n = k.size
    frac = k.mean()
    assert abs(frac - (1 - rate)) < 5 * np.sqrt(rate * (1 - rate) / n)
    for other in (0, 1, 2, 3, 4, 5, 6):
        if other == site:
            continue
        ko = DR.keep(seed, other, idx, rate)
        corr = np.corrcoef(k.ravel().astype(np.float64), ko.ravel().astype(np.float64))[0, 1]
        assert abs(corr) < 5 / np.sqrt(n), (site, other, corr)
    assert not DR.keep(seed, site, idx, 0.0).size or DR.keep(seed, site, idx, 0.0).all()


def _pmi_small(V=12, seed=0):
    pmi, count = synth.synth_pmi(V, per_row=4, seed=seed)
    return pmi, count


@pytest.mark.parametrize("doc", [[5, 6, 7, 0, 5, 9, 6, 6, 10], [3], [], [0, 0, 4, 4, 4, 0, 2], list(range(2, 12)) * 3])
def test_text_gcn_oracle_equals_the_restatement(doc):
    rs = np.random.RandomState(1)
    pmi, count = _pmi_small()
    nh = rs.randn(12, 8).astype(np.float32)
    ew = (rs.randn(count) * 1.5).astype(np.float32)            # non-unit and negative weights
    for ngram in (1, 2, 3):
        got = tg_oracle_doc(doc, nh, ew, pmi, ngram, max_length=20)
        ref = R.text_gcn_doc(doc, nh, ew, pmi, ngram, max_length=20)
        np.testing.assert_array_equal(got, ref)


def test_text_gcn_tie_rule_picks_the_first_source_position():
    """Two vocabulary rows made identical and unit edge weights: the node's two in-edges from tokens 3 and 4 carry the same
    products, and the winner is the earlier source position."""
    pmi, count = _pmi_small()
    nh = np.random.RandomState(2).randn(12, 6).astype(np.float32)
    nh[4] = nh[3]
    ew = np.ones(count, np.float32)
    doc = [3, 7, 4]                                         # 3 -> 7 <- 4, ngram 1
    nodes, win, eid, t = tg_winners(doc, nh, ew, pmi, 1)
    k = nodes.index(7)
    prods = np.stack([nh[3], nh[7], nh[4]])
    tied = (prods[0] == prods.max(0))
    assert tied.any()
    assert (win[k][tied] == 0).all()                         # position 0 (token 3) wins every tie with position 2 (token 4)
    np.testing.assert_array_equal(tg_oracle_doc(doc, nh, ew, pmi, 1), R.text_gcn_doc(doc, nh, ew, pmi, 1))
