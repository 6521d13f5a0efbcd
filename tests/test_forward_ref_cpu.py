"""tests/forward_ref.py against the committed goldens, at the bounds tests/test_oracle_golden.py asserts for the restatement: the
references the GPU edge tests judge the kernels by cannot drift unseen.  Each function is evaluated in float32 (the goldens'
own precision) and in float64 (what the edge tests feed).  CPU only."""
import numpy as np
import pytest
import torch

from oracle import golden_inputs as GI
from oracle import restatement as R
from tests import forward_ref as F
from tests import helpers as H


def _both(fn):
    """Run fn(cast) with cast = float32 and float64 conversion of a tensor."""
    return [fn(lambda t, d=d: None if t is None else torch.as_tensor(t).to(d)) for d in (torch.float32, torch.float64)]


def test_gen_adj_matches_the_adjacency_goldens():
    g = H.load_golden("adjacency.npz")
    for tag in ("object", "place"):
        for t in (3, 4, 5, 6):
            key = "%s_t%02d" % (tag, t)
            a32, a64 = _both(lambda c: F.gen_adj(c(g[key + "_A"])))
            assert H.maxabs(a32, g[key + "_adj"]) == 0.0
            assert H.relerr(a64, g[key + "_adj"]) < 1e-6
            assert np.array_equal(a64.numpy() != 0, g[key + "_adj"] != 0)


def test_label_gcn_matches_the_image_gcn_goldens():
    g = H.load_golden("image_gcn.npz")
    adj = H.load_golden("adjacency.npz")
    p = H.params_for({"gc1.weight": (300, 1024), "gc2.weight": (1024, 2048)})
    proj = GI.gcn_projection()
    rs = np.random.RandomState(11)
    lq, wq, bq = rs.standard_normal((7, 300)), 0.05 * rs.standard_normal((300, 300)), rs.standard_normal(300)
    for tag, key in (("object", "object_t04"), ("place", "place_t03")):
        X, pooled = GI.image_gcn_case(tag)
        for G, Q in _both(lambda c: F.label_gcn(c(adj[key + "_A"]), c(X), c(p["gc1.weight"]), c(p["gc2.weight"]), (c(lq), c(wq), c(bq)))):
            assert H.relerr(G @ torch.from_numpy(proj).to(G.dtype), g[tag + "_Gproj"]) < 1e-5
            assert H.relerr(torch.from_numpy(pooled).to(G.dtype) @ G.t(), g[tag + "_x"]) < 1e-5
            assert H.maxabs(G, R.image_gcn(torch.from_numpy(adj[key + "_A"]), torch.from_numpy(X), p["gc1.weight"], p["gc2.weight"])) \
                < 1e-5 * float(G.abs().max())
            assert H.maxabs(Q, torch.nn.functional.linear(torch.from_numpy(lq), torch.from_numpy(wq), torch.from_numpy(bq))) < 1e-5
        G0, none = F.label_gcn(*(torch.from_numpy(a) for a in (adj[key + "_A"], X)), p["gc1.weight"], p["gc2.weight"])
        assert none is None and G0.dtype == torch.float32 and tuple(G0.shape) == (X.shape[0], 2048)


def test_layer_norm_matches_the_golden():
    g = H.load_golden("layernorm.npz")
    p = H.params_for({"ln.gamma": (300,), "ln.beta": (300,)})
    y32, y64 = _both(lambda c: F.layer_norm(c(g["x"]), c(p["ln.gamma"]), c(p["ln.beta"])))
    assert H.maxabs(y32, g["y"]) == 0.0
    rows = [r for r in range(g["x"].shape[0]) if r != 3]        # row 3 is constant: 0 / 0-like in the reference itself
    assert H.maxabs(y64[rows], g["y"][rows]) < 2e-6


@pytest.mark.parametrize("Hn,tag,L,masked", GI.MHA_CASES)
def test_attention_core_tail_and_head_diff_match_the_mha_goldens(Hn, tag, L, masked):
    g = H.load_golden("mha.npz")
    name = "h%d_%s" % (Hn, tag)
    p = H.params_for(H.mha_shapes(Hn), prefix=name + ".")
    q, bank, mask = GI.mha_case(Hn, tag, L, masked)
    a, f = name + ".slf_attn.", name + ".pos_ffn."

    def layer(c):
        w = {"fc_w": c(p[a + "fc.weight"]), "fc_b": c(p[a + "fc.bias"]), "g1": c(p[a + "layer_norm.gamma"]),
             "be1": c(p[a + "layer_norm.beta"]), "w1": c(p[f + "w_1.weight"].squeeze(-1)), "b1": c(p[f + "w_1.bias"]),
             "w2": c(p[f + "w_2.weight"].squeeze(-1)), "b2": c(p[f + "w_2.bias"]), "g2": c(p[f + "layer_norm.gamma"]),
             "be2": c(p[f + "layer_norm.beta"])}
        qh = F.linear(c(q), c(p[a + "w_qs.weight"]), c(p[a + "w_qs.bias"]))
        o, attn = F.sq_mha_core(qh, c(bank), c(mask), Hn, 128, c(p[a + "w_ks.weight"]), c(p[a + "w_ks.bias"]),
                                c(p[a + "w_vs.weight"]), c(p[a + "w_vs.bias"]))
        out, qn = F.mha_tail(o, c(q), w, 1e-6, (c(p[a + "w_qs.weight"]), c(p[a + "w_qs.bias"])))
        assert H.maxabs(qn, F.linear(out, c(p[a + "w_qs.weight"]), c(p[a + "w_qs.bias"]))) == 0.0
        return out, attn, o

    for out, attn, o in _both(layer):
        assert H.maxabs(out, g[name + "_out"]) < 2e-5
        assert H.maxabs(attn, g[name + "_attn"]) < 1e-5
        assert attn.shape == (Hn * GI.MHA_B, 1, L)
        if masked:
            m = torch.from_numpy(np.tile(mask, (Hn, 1)))
            assert float((attn[:, 0, :] * (1 - m)).abs().max()) == 0.0
        if Hn > 1:
            assert H.maxabs(F.head_diff(o.view(GI.MHA_B, Hn, 128)), g[name + "_head_diff"]) < 1e-6


def test_label_attention_core_matches_the_goldens():
    g = H.load_golden("label_attention.npz")
    for tag, C in (("object", 80), ("place", 365)):
        p = H.params_for(H.label_attention_shapes(tag, C))
        key = GI.label_attention_key(tag)
        n = tag + "_attention."

        def run(c):
            Q = F.linear(c(g["label_query"]), c(p[n + "w_q.weight"]), c(p[n + "w_q.bias"]))
            K = F.linear(c(key), c(p[n + "w_k.weight"]), c(p[n + "w_k.bias"]))
            V = F.linear(c(key), c(p[n + "w_v.weight"]), c(p[n + "w_v.bias"]))
            y = F.linear(F.label_attn_core(Q, K, V, 5), c(p[n + "fc.weight"]), c(p[n + "fc.bias"]))
            z = F.linear(y, c(p[tag + "_linear_5.weight"]), c(p[tag + "_linear_5.bias"])).reshape(y.shape[0], -1)
            return y, F.linear(z, c(p[tag + "_x_linear.weight"]), c(p[tag + "_x_linear.bias"]))

        for y, z in _both(run):
            assert H.maxabs(y, g[tag + "_y"]) < 1e-5
            assert H.maxabs(z, g[tag + "_z"]) < 1e-5
        # the masked branch has no golden (no call site of the reference passes a mask): pinned to the restatement's
        rs = np.random.RandomState(5)
        mask = torch.from_numpy((rs.uniform(size=(5, 7, 5, 60)) > 0.3).astype(np.float32))
        mask[2, 3] = 0
        f32 = lambda t: torch.as_tensor(t).float()
        Q = F.linear(f32(g["label_query"]), p[n + "w_q.weight"], p[n + "w_q.bias"])
        K = F.linear(f32(key), p[n + "w_k.weight"], p[n + "w_k.bias"])
        V = F.linear(f32(key), p[n + "w_v.weight"], p[n + "w_v.bias"])
        y = F.linear(F.label_attn_core(Q, K, V, 5, mask), p[n + "fc.weight"], p[n + "fc.bias"])
        assert H.maxabs(y, R.label_attention(p, tag + "_attention", f32(g["label_query"]), f32(key), 5, mask)) < 1e-5


def test_text_memory_bank_matches_the_golden_and_the_restatement():
    g = H.load_golden("text_bank.npz")
    V = int(g["V"])
    shapes = {k: s for k, s in H.surface().items() if k.startswith("lstm.")}
    shapes["embedding.weight"] = (V, 300)
    p = H.params_for(shapes)
    tok, lens = torch.from_numpy(g["tok"]), torch.from_numpy(g["lens"])

    def run(c):
        w = [tuple(c(p["lstm.%s_l%d%s" % (n, l, sfx)]) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
             for l in range(2) for sfx in ("", "_reverse")]
        return F.text_memory_bank(c(p["embedding.weight"]), w, tok, lens, 150)

    for bank in _both(run):
        assert H.maxabs(bank, g["bank"]) < 1e-6
        assert H.maxabs(bank, R.text_memory_bank(p, tok, lens)) < 1e-6
        for b, n in enumerate(g["lens"]):
            if n < bank.shape[1]:
                assert float(bank[b, int(n):].abs().max()) == 0.0


def test_image_bank_and_pool_match_the_restatement():
    rs = np.random.RandomState(3)
    feat = np.maximum(rs.standard_normal((2, 2048, 196)), 0).astype(np.float32)
    w = (0.05 * rs.standard_normal((300, 2048))).astype(np.float32)
    bias = (0.05 * rs.standard_normal(300)).astype(np.float32)
    ref = R.img_memory_bank(torch.from_numpy(feat), torch.from_numpy(w), torch.from_numpy(bias))
    pooled_ref = R.max_pool(torch.from_numpy(feat).view(2, 2048, 14, 14))
    for bank, pooled in _both(lambda c: F.imgbank_pool(c(feat), c(w), c(bias))):
        assert H.relerr(bank, ref) < 1e-5
        assert torch.equal(pooled.float(), pooled_ref)


def test_the_small_references_match_torch():
    rs = np.random.RandomState(8)
    logits = torch.from_numpy(rs.standard_normal((50, 7)))
    logits[3, 2] = logits[3, 5] = logits[3].max() + 1                      # a tie: the first index wins
    probs, pred = F.softmax_argmax(logits)
    assert int(pred[3]) == 2 and torch.equal(pred, logits.argmax(1))
    assert H.maxabs(probs.sum(1), torch.ones(50)) < 1e-14
    target = torch.from_numpy(rs.randint(0, 7, size=50))
    conf = F.confusion(target, pred, 7).numpy()
    want = np.zeros((7, 7), np.int64)
    np.add.at(want, (target.numpy(), pred.numpy()), 1)
    assert np.array_equal(conf, want)
    table = torch.from_numpy(rs.standard_normal((20, 3)))
    idx = torch.from_numpy(rs.randint(0, 20, size=(4, 5)))
    assert torch.equal(F.embedding(idx, table), torch.nn.functional.embedding(idx, table))
    o = torch.from_numpy(rs.standard_normal((4, 3, 9)))
    o[1, 2] = 0                                                            # a zero head: the 1e-12 clamp
    assert H.maxabs(F.head_diff(o), R.head_diff(o)) < 1e-15
    feats = [torch.from_numpy(rs.standard_normal((4, 6))) for _ in range(4)]
    w, b = torch.from_numpy(rs.standard_normal((3, 24))), torch.from_numpy(rs.standard_normal(3))
    assert H.maxabs(F.classifier_head(feats, w, b), torch.nn.functional.linear(torch.cat(feats, 1), w, b)) < 1e-14
