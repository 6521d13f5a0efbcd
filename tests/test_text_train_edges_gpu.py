"""The text encoders' training kernels (csrc/text_train.hip, and the packing and recurrence they take from csrc/lstm.hip) at every
shape their entry points accept, against the float64 references of tests/text_train_edge_cases.py, which also holds the tables and
says where each bound comes from (tests/test_text_train_edges_cpu.py proves both without a GPU): the BiLSTM with one or two layers,
any embedding width, lengths and ids outside their ranges, rates 1 and below the masks' resolution, batches past the packing
kernel's 1024 and 4096 branches; the text GCN staged and unstaged in either kernel, ngram 0 and 15, D from 1 to 320, clamped ids;
the keyed row sum across its grid cap; the row gather; and every refusal at its limit + 1.  Gate of the two encoders: 1e-4 of each
tensor's largest magnitude, as tests/test_text_train_gpu.py asserts."""
import numpy as np
import pytest
import torch

from mgnns_amd import ops
from mgnns_amd import train as T_
from mgnns_amd.pmi import PmiCsr
from tests import helpers as H
from tests import text_train_edge_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID = T.HID


# ---- BiLSTM -------------------------------------------------------------------------------------------------------------------------------
def _modules(c, d):
    lstm = torch.nn.LSTM(c.E, HID, c.layers, bidirectional=True, batch_first=True)
    lstm.load_state_dict(d["sd"])
    emb = torch.nn.Embedding(T.LSTM_V, c.E, padding_idx=0)
    with torch.no_grad():
        emb.weight.copy_(d["emb"])
    return lstm.to(DEV), emb.to(DEV)


def _flat(lstm):
    return [getattr(lstm, n) for n in T.lstm_flat_names(lstm.num_layers)]


def _lstm_run(c, d, tok, lens, rate):
    """[bank, d embedding, d weight ...] of train.bilstm_train_forward + backward under the case's cotangent and seed."""
    lstm, emb = _modules(c, d)
    torch.manual_seed(d["torch_seed"])
    bank = T_.bilstm_train_forward(lstm, emb, tok.to(DEV), lens.to(DEV), rate)
    assert lstm.last_dropout_seed == d["seed"]
    (bank * d["G"].to(DEV)).sum().backward()
    return [bank.detach(), emb.weight.grad] + [p.grad for p in _flat(lstm)], (lstm, emb)


@pytest.mark.parametrize("c", T.LSTM_CASES, ids=T.lstm_id)
def test_bilstm_edge_case_matches_fp64(c):
    d = T.lstm_data(c)
    ref = T.lstm_ref(c)
    got, (lstm, emb) = _lstm_run(c, d, d["tok"], d["lens"], c.rate)
    names = T.lstm_names(c)
    assert len(got) == len(ref) == 2 + 8 * c.layers
    for n, g, r in zip(names, got, ref):
        H.close(g, r, T.GATE, n, rel=True)
    bank, demb = got[0], got[1]
    pad = (torch.arange(c.T)[None, :] >= d["lens_c"][:, None]).to(DEV)
    assert float(bank[pad].abs().max() if pad.any() else 0.0) == 0.0, "padding rows of the bank"
    absent = np.setdiff1d(np.arange(T.LSTM_V), d["tok_c"].numpy()[(~pad).cpu().numpy()])
    assert float(demb[0].abs().max()) == 0.0 and float(demb[torch.from_numpy(absent).to(DEV)].abs().max()) == 0.0
    if c.ids == "oob":
        assert T.LSTM_V - 1 not in absent and float(demb[T.LSTM_V - 1].abs().max()) > 0
    # the same batch with lengths and ids pre-clamped (for the other cases the same batch again: one seed, bit-identical)
    again, _ = _lstm_run(c, d, d["tok_c"], d["lens_c"], c.rate)
    for n, a, b in zip(names, got, again):
        assert torch.equal(a, b), "%s differs from the pre-clamped run" % n
    if c.rate in (0.0, T.TINY_RATE):
        ws = [tuple(t.detach() for t in _flat(lstm)[4 * i:4 * i + 4]) for i in range(2 * c.layers)]
        ev = ops.bilstm(d["tok"].to(DEV), d["lens"].to(DEV), emb.weight.detach(), ws, HID, c.layers, recurrence="f32")
        assert torch.equal(bank, ev)
    if c.rate == T.TINY_RATE:
        zero, _ = _lstm_run(c, d, d["tok"], d["lens"], 0.0)
        for n, a, b in zip(names, got, zero):
            assert torch.equal(a, b), "%s at rate 2^-25 differs from rate 0" % n
    if c.rate == 1.0:
        for n, g in zip(names[1:10], got[1:10]):
            assert float(g.abs().max()) == 0.0, "%s must get exactly zero at rate 1" % n


@pytest.mark.parametrize("B", [1025, 4097])
def test_packing_past_1024_and_4096_samples_keeps_every_chain_in_its_slot(B):
    """lstm_pack_kernel's serial-chunk scan (B > 1024) and its lengths read back from offs (B > 4096), through the eval forward: the
    fp32 recurrence and the bf16 one (which leaves its fused pack + fill + gather launch there), with and without the folded embedding
    table.  A chain does not depend on its neighbours: every sample equals the same sample run in a batch of 64, bit for bit."""
    rs = np.random.RandomState(B)
    T_len, V, E = 2, 50, 300
    torch.manual_seed(B)
    lstm = torch.nn.LSTM(E, HID, 2, bidirectional=True, batch_first=True).to(DEV)
    emb = torch.nn.Embedding(V, E, padding_idx=0).to(DEV).weight.detach()
    ws = [tuple(t.detach() for t in _flat(lstm)[4 * i:4 * i + 4]) for i in range(4)]
    lens = rs.randint(0, 3, size=B)
    lens[[0, 1, 2, B - 1]] = (2, 0, 1, 2)
    tok = rs.randint(1, V, size=(B, T_len))
    for b in range(B):
        tok[b, lens[b]:] = 0
    tok, lens = torch.from_numpy(tok).to(DEV), torch.from_numpy(lens).to(DEV)

    def chunks(**kw):
        return torch.cat([ops.bilstm(tok[i:i + 64], lens[i:i + 64], emb, ws, HID, 2, **kw) for i in range(0, B, 64)])
    for kw in (dict(recurrence="f32"), dict(recurrence="bf16", fold=False), dict(recurrence="bf16", fold=True, cache=ops.LstmCache())):
        want = chunks(**kw)
        if "cache" in kw:
            kw = dict(kw, cache=ops.LstmCache())
        got = ops.bilstm(tok, lens, emb, ws, HID, 2, **kw)
        bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, "%s: samples %s (of %d) differ from their run in a batch of 64" % (kw, bad[:8], len(bad))
    assert float(chunks(recurrence="f32").abs().max()) > 0


# ---- text GCN -------------------------------------------------------------------------------------------------------------------------------
class _TG(torch.nn.Module):
    def __init__(self, d, ngram, max_length):
        super().__init__()
        self.node_hidden = torch.nn.Embedding(*d["nh"].shape)
        self.seq_edge_w = torch.nn.Embedding(d["count"], 1)
        with torch.no_grad():
            self.node_hidden.weight.copy_(torch.from_numpy(d["nh"]))
            self.seq_edge_w.weight.copy_(torch.from_numpy(d["ew"]).view(-1, 1))
        self.edges_matrix, self.ngram, self.max_length = PmiCsr.coerce(d["pmi"]), ngram, max_length


def _tg_run(c, d, tok, nodes=True, edges=True, max_length=None):
    """(out, d node_hidden or None, d edge weights or None, the module) of TextGCNTrainFunction + backward under the case's cotangent."""
    tg = _TG(d, c.ngram, c.max_length if max_length is None else max_length).to(DEV)
    tg.node_hidden.weight.requires_grad_(nodes)
    tg.seq_edge_w.weight.requires_grad_(edges)
    tok = torch.from_numpy(np.ascontiguousarray(tok)).to(DEV)
    out = T_.TextGCNTrainFunction.apply(tok, tg.edges_matrix.device_arrays(tok.device), tg.ngram, tg.max_length, d["seed"], c.rate,
                                        tg.node_hidden.weight, tg.seq_edge_w.weight)
    (out * d["G"].to(DEV)).sum().backward()
    de = tg.seq_edge_w.weight.grad
    return out.detach(), tg.node_hidden.weight.grad, None if de is None else de.view(-1), tg


@pytest.mark.parametrize("c", T.TG_CASES, ids=T.tg_id)
def test_text_gcn_edge_case_matches_fp64(c):
    d = T.tg_data(c)
    out, dn, de, tg = _tg_run(c, d, d["tok"])
    tok = torch.from_numpy(d["tok"]).to(DEV)
    pmi_dev = tg.edges_matrix.device_arrays(tok.device)
    nh, ew = tg.node_hidden.weight.detach(), tg.seq_edge_w.weight.detach()
    _, saved = ops.textgcn_train(tok, nh, ew, pmi_dev, c.ngram, c.max_length, d["seed"], c.rate)
    ref = T.tg_run_ref(c, torch.float64, saved["presum"])
    for n, g, r in zip(("out", "node_hidden grad", "edge weight grad"), (out, dn, de), ref):
        H.close(g, r, T.GATE, n, rel=True)
    Tm = min(c.T, c.max_length)
    if c.rate == 0.0:                                                   # (documents of at most 40 nodes: see the case table)
        H.close(out, ops.textgcn(tok, nh, ew, pmi_dev, c.ngram, c.max_length).double().cpu(), 1e-6, "rate 0 vs eval", rel=True)
    absent = torch.from_numpy(np.setdiff1d(np.arange(T.TG_V), d["tok_c"][:, :Tm])).to(DEV)
    assert float(dn[absent].abs().max()) == 0.0 and float(dn[0].abs().max()) == 0.0
    # ids pre-clamped (for the other cases the same batch again: bit-identical)
    out2, dn2, de2, _ = _tg_run(c, d, d["tok_c"])
    assert torch.equal(out, out2) and torch.equal(dn, dn2) and torch.equal(de, de2)
    if any(k == "oob" for k in d["kinds"]):
        assert T.TG_V - 1 not in absent.tolist() and float(dn[T.TG_V - 1].abs().max()) > 0


@pytest.mark.parametrize("i", [1, 2])
def test_text_gcn_frozen_parameter_gets_none_and_the_other_gradient_is_unchanged(i):
    c = T.TG_CASES[i]
    d = T.tg_data(c)
    out, dn, de, _ = _tg_run(c, d, d["tok"])
    out_n, dn_n, de_n, _ = _tg_run(c, d, d["tok"], edges=False)          # need_edges = False
    out_e, dn_e, de_e, _ = _tg_run(c, d, d["tok"], nodes=False)          # need_nodes = False
    assert de_n is None and dn_e is None
    assert torch.equal(out, out_n) and torch.equal(out, out_e) and torch.equal(dn, dn_n) and torch.equal(de, de_e)


@pytest.mark.parametrize("ngram,T1,T2,flips", [(1, 40, 130, (True, True)), (15, 30, 100, (False, True))])
def test_text_gcn_staged_equals_unstaged(ngram, T1, T2, flips):
    """Staging is decided by min(T, max_length) alone: the same documents at max_length = T = T1 (node rows in LDS) and padded into
    T = T2 (read from the table, in the kernels `flips` names: forward, backward) give the same bits."""
    D, V, B = 320, T.TG_V, 3
    for parts, flip in zip((False, True), flips):
        assert T.tg_staged(T1, ngram, D, parts) and T.tg_staged(T2, ngram, D, parts) == (not flip)
    c = T.Tg(B, T1, T1, ngram, D, ("random", "repeat", "padin"), 0.5)
    rs = np.random.RandomState(T1)
    pmi, count = T.synth.synth_pmi(V, per_row=V // 4, seed=T1)
    tok = np.stack([T._tg_doc(k, T1, V, rs) for k in c.docs])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(T2)
        G = torch.randn(B, D)
    d = dict(nh=rs.randn(V, D).astype(np.float32), ew=(rs.randn(count) * 1.3 + 0.2).astype(np.float32), pmi=pmi, count=count, G=G, seed=31)
    a = _tg_run(c, d, tok)
    padded = np.zeros((B, T2), np.int64)
    padded[:, :T1] = tok
    b = _tg_run(c, d, padded, max_length=T2)
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0 and float(a[2].abs().max()) > 0
    for n, x, y in zip(("out", "node_hidden grad", "edge weight grad"), a[:3], b[:3]):
        assert torch.equal(x, y), n


# ---- keyed row sum and gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.KS_CASES, ids=lambda c: "D%d-M%d-%s" % c)
def test_keyed_row_sum_direct(c):
    d = T.ks_data(c)
    keys, vals = d["keys"].to(DEV), d["vals"].to(DEV)
    got = ops.keyed_row_sum(keys, vals, d["n_out"], skip_below=d["skip"])
    assert tuple(got.shape) == (d["n_out"], c.D) and torch.isfinite(got).all()
    err = (got.double().cpu() - d["ref"]).abs()
    worst = float((err / d["bound"].clamp_min(1e-300)).max()) if d["hit"].any() else 0.0
    print("max err %.3e, worst err / (run length x 2^-24 x max|row|) %.3f, longest run %d" % (float(err.max()), worst, int(d["runs"].max())))
    assert (err <= d["bound"]).all(), "worst err / bound %.3f" % worst
    assert float(got[~d["hit"].to(DEV)].abs().max() if not d["hit"].all() else 0.0) == 0.0, "rows without a key"
    assert torch.equal(got, ops.keyed_row_sum(keys, vals, d["n_out"], skip_below=d["skip"]))


@pytest.mark.parametrize("K,M", T.GATHER_CASES)
def test_gather_rows_direct(K, M):
    rs = np.random.RandomState(K + M)
    n_src = T.GATHER_N_SRC
    src = torch.from_numpy(rs.standard_normal((n_src, K)).astype(np.float32)).to(DEV)
    idx = rs.randint(0, n_src, size=max(M, 4)).astype(np.int32)
    if M >= 1000:
        idx[[0, 500, 999]] = (-1, n_src, -1)
        idx[1] = n_src - 1
    elif M == 1:
        idx[0] = n_src if K == 301 else -1
    idx_t = torch.from_numpy(idx).to(DEV)
    got = ops.gather_rows(src, idx_t, M)
    assert tuple(got.shape) == (M, K)
    ok = (idx[:M] >= 0) & (idx[:M] < n_src)
    want = torch.zeros(M, K)
    want[torch.from_numpy(ok)] = src.cpu()[torch.from_numpy(idx[:M][ok].astype(np.int64))]
    assert torch.equal(got.cpu(), want)
    assert M == 0 or not ok.all()


# ---- refusals, each at the limit + 1 ---------------------------------------------------------------------------------------------------------
def test_bilstm_refusals():
    c = T.LSTM_CASES[2]
    d = T.lstm_data(c)
    lstm, emb = _modules(c, d)
    tok, lens = d["tok_c"].to(DEV), d["lens_c"].to(DEV)
    for rate in (-0.1, 1.01):
        with pytest.raises(ValueError, match="outside \\[0, 1\\]"):
            T_.bilstm_train_forward(lstm, emb, tok, lens, rate)
    with pytest.raises(ValueError, match="text_lens has"):
        T_.bilstm_train_forward(lstm, emb, tok, lens[:-1], 0.0)
    with pytest.raises(RuntimeError, match="hidden_size=151 unsupported"):
        T_.bilstm_train_forward(torch.nn.LSTM(c.E, 151, 2, bidirectional=True, batch_first=True).to(DEV), emb, tok, lens, 0.0)
    with pytest.raises(RuntimeError, match="num_layers=3 unsupported"):
        T_.bilstm_train_forward(torch.nn.LSTM(c.E, HID, 3, bidirectional=True, batch_first=True).to(DEV), emb, tok, lens, 0.0)
    torch.cuda.synchronize()
    T_.bilstm_train_forward(lstm, emb, tok, lens, 1.0).sum().backward()          # the limits themselves run: rate 1, hidden 150, 2 layers


@pytest.mark.parametrize("what,T_len,D,ngram,max_length,msg", T.TG_REFUSALS, ids=[r[0] for r in T.TG_REFUSALS])
def test_text_gcn_refusals_come_from_the_forward(what, T_len, D, ngram, max_length, msg):
    """... the two past the backward's LDS included: a step that could not finish is refused before anything is launched, not in
    backward()."""
    V = 12
    pmi, count = T.synth.synth_pmi(V, per_row=4, seed=0)
    pmi_dev = PmiCsr.coerce(pmi).device_arrays(torch.device(DEV))
    nh = torch.randn(V, D, device=DEV, requires_grad=True)
    ew = torch.randn(count, 1, device=DEV, requires_grad=True)
    tok = torch.randint(1, V, (1, T_len), device=DEV)
    with pytest.raises(RuntimeError, match=msg):
        T_.TextGCNTrainFunction.apply(tok, pmi_dev, ngram, max_length, 1, 0.0, nh, ew)
    torch.cuda.synchronize()
    if "backward" in msg:                                               # the limit itself trains
        lim = T.tg_tm_max(ngram)
        assert min(T_len, max_length) == lim + 1
        out = T_.TextGCNTrainFunction.apply(tok[:, :lim].contiguous(), pmi_dev, ngram, max_length, 1, 0.0, nh, ew)
        out.sum().backward()
        assert torch.isfinite(out).all() and torch.isfinite(nh.grad).all() and torch.isfinite(ew.grad).all() and float(nh.grad.abs().max()) > 0


def test_text_gcn_refuses_a_pmi_map_of_another_vocabulary():
    V, D = 12, 8
    pmi, count = T.synth.synth_pmi(V + 2, per_row=4, seed=0)
    pmi_dev = PmiCsr.coerce(pmi).device_arrays(torch.device(DEV))
    nh = torch.randn(V, D, device=DEV, requires_grad=True)
    ew = torch.randn(count, 1, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="PMI map has %d rows" % (V + 2)):
        T_.TextGCNTrainFunction.apply(torch.ones(1, 4, dtype=torch.int64, device=DEV), pmi_dev, 1, 100, 1, 0.0, nh, ew)
