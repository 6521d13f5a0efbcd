"""Training mode of the text encoders on the GPU (csrc/text_train.hip, mgnns_amd/train.py) against fp64 CPU autograd: the
packed BiLSTM bank (two single-layer bidirectional LSTMs with the site-5 mask between them) and the text GCN (winners from
the fp32 products by the tie rule, then fp64 autograd through a gather), then the whole model with the encoders live.
Gate: 1e-4 of each tensor's largest magnitude."""
import numpy as np
import pytest
import torch

from mgnns_amd import ops, synth
from mgnns_amd import train as T_
from mgnns_amd.pmi import PmiCsr
from tests import dropout_ref as DR
from tests import test_model_train_gpu as MT
from tests.test_text_train_cpu import lstm_keep, textgcn_keep, tg_winners
from tests.text_train_edge_cases import lstm_oracle, tg_oracle      # the oracles, shared with the edge sweep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID = 150


def close(got, ref, what, tol=1e-4):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale + 1e-12, "%s: max err %.3e vs max |ref| %.3e" % (what, err, scale)


# ---- BiLSTM -------------------------------------------------------------------------------------------------------------------
def _lstm_case(B, T_len, pattern, rate, V=500, seed=11):
    rs = np.random.RandomState(seed + B + T_len)
    if pattern == "full":
        lens = np.full(B, T_len)
    elif pattern == "edges":
        lens = np.array([[0, 1, T_len][i % 3] for i in range(B)])
    else:
        lens = rs.randint(0, T_len + 1, size=B)
    tok = rs.randint(1, 40, size=(B, T_len))                        # a small alphabet: tokens repeat across samples
    tok[:, ::7] = 0 if T_len > 1 else tok[:, ::7]                    # PAD inside a length: row 0 must get no gradient
    for b in range(B):
        tok[b, lens[b]:] = 0
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(300, HID, 2, bidirectional=True, batch_first=True, dropout=rate).to(DEV)
    emb = torch.nn.Embedding(V, 300, padding_idx=0).to(DEV)
    return torch.from_numpy(tok).to(DEV), torch.from_numpy(lens).to(DEV), lstm, emb


def _flat(lstm):
    return [getattr(lstm, "%s_l%d%s" % (n, l, s)) for l in range(lstm.num_layers) for s in ("", "_reverse")
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


CASES = [(1, 1, "full"), (1, 50, "full"), (7, 50, "edges"), (7, 100, "ragged"), (64, 50, "ragged"), (64, 100, "edges"),
         (256, 1, "edges"), (256, 100, "ragged"), (256, 100, "full")]


@pytest.mark.parametrize("B,T_len,pattern,rate", [c + (0.0,) for c in CASES] + [c + (0.5,) for c in CASES if c[0] * c[1] < 7000
                                                                                    or c[2] == "ragged"])
def test_bilstm_bank_and_gradients_match_fp64(B, T_len, pattern, rate):
    tok, lens, lstm, emb = _lstm_case(B, T_len, pattern, rate)
    bank = T_.bilstm_train_forward(lstm, emb, tok, lens, rate)
    seed = lstm.last_dropout_seed
    G = torch.randn(B, T_len, 2 * HID, generator=torch.Generator().manual_seed(5)).to(DEV)
    (bank * G).sum().backward()
    emb64 = emb.weight.detach().double().cpu().requires_grad_()
    flat64 = [p.detach().double().cpu().requires_grad_() for p in _flat(lstm)]
    ref = lstm_oracle(tok.cpu(), lens.cpu(), emb64, flat64, seed, rate)
    (ref * G.cpu().double()).sum().backward()
    close(bank.detach(), ref.detach(), "bank")
    for p, r, n in zip(_flat(lstm), flat64, range(16)):
        close(p.grad, r.grad, "lstm weight %d" % n)
    close(emb.weight.grad, emb64.grad, "embedding")
    assert float(emb.weight.grad[0].abs().max()) == 0.0
    if rate == 0.0:
        ws = [tuple(t.detach() for t in _flat(lstm)[4 * i:4 * i + 4]) for i in range(4)]
        ev = ops.bilstm(tok, lens, emb.weight.detach(), ws, HID, 2, recurrence="f32")
        assert torch.equal(bank.detach(), ev)


def test_bilstm_same_seed_is_bit_identical():
    tok, lens, lstm, emb = _lstm_case(64, 50, "ragged", 0.5)
    runs = []
    for _ in range(2):
        lstm.zero_grad(set_to_none=True)
        emb.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        bank = T_.bilstm_train_forward(lstm, emb, tok, lens, 0.5)
        bank.sum().backward()
        runs.append([bank.detach().clone(), emb.weight.grad.clone()] + [p.grad.clone() for p in _flat(lstm)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- text GCN -----------------------------------------------------------------------------------------------------------------
class _TG(torch.nn.Module):
    def __init__(self, V, D, count, pmi, ngram, max_length, rs):
        super().__init__()
        self.node_hidden = torch.nn.Embedding(V, D)
        self.seq_edge_w = torch.nn.Embedding(count, 1)
        with torch.no_grad():
            self.node_hidden.weight.copy_(torch.from_numpy(rs.randn(V, D).astype(np.float32)))
            self.seq_edge_w.weight.copy_(torch.from_numpy((rs.randn(count, 1) * 1.3 + 0.2).astype(np.float32)))
        self.edges_matrix, self.ngram, self.max_length = PmiCsr.coerce(pmi), ngram, max_length


def _docs(B, T_len, V, rs):
    tok = rs.randint(1, V, size=(B, T_len))
    tok[:, 3::5] = tok[:, 1::5][:, :tok[:, 3::5].shape[1]]          # repeated tokens
    tok[0] = 0                                                        # empty
    tok[1, 1:] = 0                                                    # one token
    if B > 2:
        tok[2, 2] = 0                                                 # PAD inside
    return tok


@pytest.mark.parametrize("B,T_len,ngram,max_length", [(6, 12, 1, 100), (9, 30, 3, 20), (32, 100, 2, 100), (256, 100, 3, 100)])
@pytest.mark.parametrize("rate", [0.0, 0.5])
def test_text_gcn_output_and_gradients_match_fp64(B, T_len, ngram, max_length, rate):
    rs = np.random.RandomState(B + T_len)
    V, D = 60, 300
    pmi, count = synth.synth_pmi(V, per_row=6, seed=B)
    tg = _TG(V, D, count, pmi, ngram, max_length, rs).to(DEV)
    docs = _docs(B, T_len, V, rs)
    # a forced cross-token tie: document 3 starts [7, 9, 8], rows 7 and 8 identical, and the two edges 7 -> 9 and 8 -> 9 given
    # one weight, so node 9's in-edges from positions 0 and 2 carry equal products; the tie rule sends the gradient to row 7
    docs[3, :3] = (7, 9, 8)
    with torch.no_grad():
        tg.node_hidden.weight[8] = tg.node_hidden.weight[7]
        tg.seq_edge_w.weight[pmi[8, 9]] = tg.seq_edge_w.weight[pmi[7, 9]]
    nh32 = tg.node_hidden.weight.detach().cpu().numpy()
    ew32 = tg.seq_edge_w.weight.detach().cpu().numpy().reshape(-1)
    nodes, win, _, t = tg_winners(docs[3], nh32, ew32, pmi, ngram, max_length)
    k = nodes.index(9)
    p7 = np.float32(ew32[pmi[7, 9]]) * nh32[7]
    tied = p7 == np.max(np.stack([np.float32(ew32[pmi[t[i], 9]]) * nh32[t[i]] for i in range(len(t))
                                  if any(t[j] == 9 for j in range(max(0, i - ngram), min(len(t), i + ngram + 1)))]), axis=0)
    assert tied.any(), "the constructed document has no cross-token tie"
    assert (win[k][tied] == 0).all()                                  # position 0 (token 7) beats position 2 (token 8)
    tok = torch.from_numpy(docs).to(DEV)
    pmi_dev = tg.edges_matrix.device_arrays(tok.device)
    seed = 99 + B
    out = T_.TextGCNTrainFunction.apply(tok, pmi_dev, ngram, max_length, seed, rate, tg.node_hidden.weight, tg.seq_edge_w.weight)
    _, saved = ops.textgcn_train(tok, tg.node_hidden.weight.detach(), tg.seq_edge_w.weight.detach(), pmi_dev, ngram, max_length,
                                 seed, rate)
    G = torch.randn(B, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    (out * G).sum().backward()
    ref, nh, ew = tg_oracle(tok.cpu().numpy(), nh32, ew32, pmi, ngram, max_length, saved["presum"], seed, rate)
    (ref * G.cpu().double()).sum().backward()
    close(out.detach(), ref.detach(), "text gcn out")
    close(tg.node_hidden.weight.grad, nh.grad, "node_hidden grad")
    close(tg.seq_edge_w.weight.grad.view(-1), ew.grad, "edge weight grad")
    if rate == 0.0:
        ev = ops.textgcn(tok, tg.node_hidden.weight.detach(), tg.seq_edge_w.weight.detach(), pmi_dev, ngram, max_length)
        close(out.detach(), ev, "rate 0 vs eval", tol=1e-6)


# ---- whole model --------------------------------------------------------------------------------------------------------------
NO_GRAD = tuple(p for p in MT.NO_GRAD_PREFIXES if p not in ("lstm.", "embedding.", "text_features.")) + ("text_features.Linear.",)


def _text_ref(p, model, args, inp, seeds):
    """(text feature, text bank) in fp64 from the parameter dict p (leaves), under the masks of the kernels' seeds."""
    tok, lens = args[0].cpu(), args[1].cpu()
    tg = model.text_features
    rate_tg = tg.dropout.p if tg.training else 0.0
    nh32 = p["text_features.node_hidden.weight"].detach().float().numpy()
    ew32 = p["text_features.seq_edge_w.weight"].detach().float().numpy().reshape(-1)
    B, D = tok.shape[0], nh32.shape[1]
    keep = torch.from_numpy(textgcn_keep(seeds[0], rate_tg, B, D)).double() / (1.0 - rate_tg)
    rows = []
    for b in range(B):
        nodes, win, eid, t = tg_winners(tok[b].numpy(), nh32, ew32, tg.edges_matrix, tg.ngram, tg.max_length)
        s = torch.zeros(D, dtype=torch.float64)
        for k in range(len(nodes)):
            src = torch.from_numpy(np.asarray(t, np.int64)[win[k]])
            s = s + p["text_features.seq_edge_w.weight"].view(-1)[torch.from_numpy(eid[k])] * \
                p["text_features.node_hidden.weight"][src, torch.arange(D)]
        rows.append(s)
    tf = torch.relu(torch.stack(rows) * keep)
    flat = [p["lstm.%s_l%d%s" % (n, l, s)] for l in range(2) for s in ("", "_reverse")
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    rate_l = model.lstm.dropout if model.lstm.training else 0.0
    bank = lstm_oracle(tok, lens, p["embedding.weight"], flat, seeds[1], rate_l)
    return tf, bank


@pytest.mark.parametrize("cfg_name,encoders", [("mvsa_single_b8", "train"), ("mvsa_multiple_b256", "train"),
                                                ("mvsa_single_b8", "eval"), ("mvsa_multiple_b256", "eval")])
def test_whole_model_with_live_text_encoders_matches_fp64(cfg_name, encoders):
    """encoders='train': model.train() after unfreezing -- the BiLSTM's and the text GCN's dropout active (sites 5, 6);
    'eval': the encoders trainable but in eval mode (no dropout in them)."""
    torch.manual_seed(1)                  # the modules' dropout seeds come from torch's generator: fixed here, not by test order
    cfg, model, inp = MT.make(cfg_name)
    model.unfreeze_text_encoders()
    if encoders == "train":
        model.train()
        assert model.lstm.training and model.text_features.training and model.lstm.dropout > 0 and model.text_features.dropout.p > 0
    else:
        assert not model.lstm.training and not model.text_features.training
    args = MT.harness.call_args(inp, DEV)
    logits = MT.train_step(model, args)
    B, T_len = args[0].shape
    masks = MT.collect_masks(model, B, T_len, args[3].shape[2] * args[3].shape[3])
    p = MT.ref_params(model)
    tf, bank = _text_ref(p, model, args, inp, (model.text_features.last_dropout_seed, model.lstm.last_dropout_seed))
    ref = MT.model_ref(p, model, (tf, bank, args[2].double().cpu()), inp, masks)
    ref.sum().backward()
    close(logits, ref.detach(), "logits")
    got_none = {k for k, v in model.named_parameters() if v.grad is None}
    assert got_none == {k for k in p if k.startswith(NO_GRAD)}
    for k, v in model.named_parameters():
        if v.grad is not None:
            close(v.grad, p[k].grad, k)


def test_whole_model_determinism_frozen_embedding_and_freeze_again():
    cfg, model, inp = MT.make("mvsa_single_b8")
    model.unfreeze_text_encoders()
    args = MT.harness.call_args(inp, DEV)
    model.train()                         # the encoders' dropout active too
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        lg = MT.train_step(model, args)
        runs.append([lg] + [v.grad.clone() for v in model.parameters() if v.grad is not None])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    first = {n: v.grad.clone() for n, v in model.named_parameters() if v.grad is not None}
    model.embedding.weight.requires_grad_(False)
    torch.manual_seed(21)
    lg = MT.train_step(model, args)
    assert model.embedding.weight.grad is None
    assert torch.equal(lg, runs[0][0])
    now = {n: v.grad for n, v in model.named_parameters() if v.grad is not None}
    assert set(now) == set(first) - {"embedding.weight"}
    for n, g in now.items():
        assert torch.equal(g, first[n]), n
    assert model.lstm.weight_hh_l0.grad is not None and model.text_features.node_hidden.weight.grad is not None
    model.freeze_text_encoders()
    MT.train_step(model, args)
    assert all(v.grad is None for n, v in model.named_parameters() if n.startswith(("lstm.", "embedding.", "text_features.")))
    model.lstm.train()
    with pytest.raises(RuntimeError, match="eval.*freeze_text_encoders"):
        model(*args)


def test_adam_steps_then_eval_uses_the_new_text_weights():
    from oracle import restatement as R
    cfg, model, inp = MT.make("mvsa_single_b8")
    model.unfreeze_text_encoders()
    args = MT.harness.call_args(inp, DEV)
    opt = torch.optim.Adam(model.get_config_optim(1e-3, 0.1), lr=1e-3)
    before = model.lstm.weight_hh_l0.detach().clone()
    with torch.no_grad():
        model.eval()
        model(*args)                      # fills the eval caches with the old weights
    model.train()
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        model(*args).sum().backward()
        opt.step()
    assert not torch.equal(before, model.lstm.weight_hh_l0.detach())
    model.eval()
    with torch.no_grad():
        got = model(*args).cpu()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ti = {k: torch.as_tensor(v) for k, v in inp.items()}
    ref = R.forward(p, ti, model.text_features.edges_matrix, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram,
                    label_query=torch.as_tensor(inp["label_query"]))
    close(got, ref, "eval logits after Adam", tol=1e-4)


# ---- saved state ----------------------------------------------------------------------------------------------------------------
def _freed_after_backward(run):
    """run() -> (output, loss); with the cyclic collector off, the output and the saved state must be gone once the graph is
    dropped: plain reference counting frees them (no cycle through ctx)."""
    import gc
    import weakref
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    gc.disable()
    try:
        out, loss = run()
        ref = weakref.ref(out)
        held = torch.cuda.memory_allocated() - base
        loss.backward()
        del out, loss
        assert ref() is None, "the output outlived its graph"
        torch.cuda.synchronize()
        left = torch.cuda.memory_allocated() - base
    finally:
        gc.enable()
    return held, left


def test_bilstm_saved_state_is_freed_and_inplace_edits_are_caught():
    tok, lens, lstm, emb = _lstm_case(64, 100, "full", 0.5)
    lstm.requires_grad_(False)
    emb.requires_grad_(False)
    lstm.weight_hh_l0.requires_grad_(True)

    def run():
        bank = T_.bilstm_train_forward(lstm, emb, tok, lens, 0.5)
        return bank, bank.sum()
    _freed_after_backward(run)                                        # (allocator warm-up)
    lstm.weight_hh_l0.grad = None
    held, left = _freed_after_backward(run)
    grad = lstm.weight_hh_l0.grad.numel() * 4
    assert held > 50 * 2 ** 20                                        # gates, cells, the layer outputs: ~70 MB here
    assert left <= grad + 4096, "%d bytes of saved state outlived the step" % (left - grad)     # (512-B allocator blocks)
    bank = T_.bilstm_train_forward(lstm, emb, tok, lens, 0.5)
    loss = (bank * 1.0).sum()
    bank.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_text_gcn_saved_state_is_freed():
    rs = np.random.RandomState(3)
    V, D = 60, 300
    pmi, count = synth.synth_pmi(V, per_row=6, seed=3)
    tg = _TG(V, D, count, pmi, 2, 100, rs).to(DEV)
    tok = torch.from_numpy(_docs(64, 100, V, rs)).to(DEV)
    pmi_dev = tg.edges_matrix.device_arrays(tok.device)

    def run():
        out = T_.TextGCNTrainFunction.apply(tok, pmi_dev, 2, 100, 5, 0.5, tg.node_hidden.weight, tg.seq_edge_w.weight)
        return out, out.sum()
    _freed_after_backward(run)
    tg.zero_grad(set_to_none=True)
    held, left = _freed_after_backward(run)
    grads = (tg.node_hidden.weight.numel() + tg.seq_edge_w.weight.numel()) * 4
    assert left <= grads + 4096, "%d bytes of saved state outlived the step" % (left - grads)
