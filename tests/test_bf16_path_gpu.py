"""bf16 mode against an oracle that rounds where the kernels round (oracle/bf16_path.py).

The other bf16 tests hold this mode to the fp32 answer inside a band as wide as bf16 noise (2e-2 on the logits); a kernel
that is subtly wrong -- a rounding point moved, truncation for round-to-nearest-even, a bias lost on a ragged tile -- stays
inside that band.  Here every case is compared with the emulation of its own rounding points, and the gate has two levels per
output tensor:
  bulk  a quantile of the elementwise error (GATES) lies within an fp32-order tolerance (summation order; for the whole forward,
        the rounding flips that order causes in a chain of bf16 stages), and
  max   the largest error lies within a flip bound: an intermediate that lands on the other side of a bf16 rounding boundary
        moves by 2^-8 relative, and the change propagates (through up to 230 steps of the LSTM recurrence).
Every gate is set from errors measured on the MI355X over the cases it covers ("measured" next to it)."""
import numpy as np
import pytest
import torch

from mgnns_amd import ops, synth
from oracle import bf16_path as E
from tests import helpers as H
from tests.model_util import build_model, call_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Gates per (case kind, output tensor): (quantile, bulk gate, max gate).  The bulk level is the given quantile of the elementwise
# |error|: the 90th percentile for the operator cases, where it sits at fp32 summation order; the median for the whole forward,
# where the bf16 roundings of 4 x 2 layers, each over rows of 300 - 2400 values, leave few rows without a flip (an fp32 run of
# the emulation itself spreads as far from its fp64 run: median 5e-4, max 6e-3 on the tumemo_b64 stacks).  Bank copies held
# as bf16 use the 99.9th percentile: exact but for single-ulp flips.  Operator gates are 4x, whole-forward gates 2x the worst
# value measured on the MI355X over the kind's cases (noted as "measured bulk / max", with the fp32 network's distance).
GATES = {
    "lstm/rows": (0.9, 3e-5, 3.5e-4),              # measured 7.7e-6 / 8.8e-5 (fp32 network: max 1.7e-3)
    "lstm/bf16": (0.9, 0.0, 7.8e-3),               # measured 0 / 2.0e-3 (single-ulp flips)
    "tail1/out": (0.9, 1e-6, 8.6e-3),              # measured 2.6e-7 / 2.2e-3 (fp32 network: max 1.0e-2)
    "tail1/next": (0.9, 7e-7, 2.2e-2),             # measured 1.8e-7 / 5.5e-3 (fp32 network: max 1.4e-2)
    "c16/out": (0.9, 1.8e-6, 1.3e-2),              # measured 4.7e-7 / 3.4e-3 (fp32 network: max 9.8e-3)
    "c16/next": (0.9, 8e-7, 2.7e-2),               # measured 2.1e-7 / 6.8e-3 (fp32 network: max 1.5e-2)
    "label1/out": (0.9, 6e-5, 9.6e-4),             # measured 1.6e-5 / 2.4e-4 (split-bf16 form: max 1.0e-3)
    "label1/next": (0.9, 2.5e-4, 1.9e-3),          # measured 6.3e-5 / 4.9e-4 (split-bf16 form: max 1.4e-3)
}
_FWD = {                                           # whole forward, faithful / folded: measured bulk / max of the worse of the two
    "text_bank": (0.9, 1e-5, 1.4e-4),              # 5.4e-6 / 7.2e-5
    "text_bank_bf16": (0.9, 0.0, 1.9e-3),          # 0 / 9.8e-4
    "bank_object": (0.999, 0.0, 3.1e-2),           # 0 / 1.6e-2 (one ulp)
    "bank_place": (0.999, 0.0, 6.2e-2),            # 0 / 3.1e-2 (one ulp)
    "object_att": (0.5, 1.8e-5, 1.0e-4),           # 9.0e-6 / 5.4e-5 (split-bf16 channel tail: fp32-class)
    "place_att": (0.5, 1.3e-4, 9.7e-4),            # 6.7e-5 / 4.9e-4
    "tio": (0.5, 2.0e-3, 1.5e-2),                  # 1.0e-3 / 7.7e-3
    "tip": (0.5, 1.9e-3, 1.5e-2),                  # 9.4e-4 / 7.8e-3
    "iot": (0.5, 1.4e-3, 1.3e-2),                  # 7.3e-4 / 6.7e-3
    "ipt": (0.5, 1.2e-3, 1.1e-2),                  # 6.3e-4 / 6.0e-3
    "logits": (0.5, 5.3e-3, 1.4e-2),               # 2.6e-3 / 7.2e-3 (fp32 network: max 1.7e-2)
}
PARTS = tuple(_FWD)
for _att in ("faithful", "folded"):
    for _part, _g in _FWD.items():
        GATES["fwd_%s/%s" % (_att, _part)] = _g


def dev(x):
    return torch.as_tensor(x).to(DEV).contiguous()


def _errs(got, want, quantile):
    d = (got.detach().double().cpu() - torch.as_tensor(want).double()).abs().flatten().numpy()
    if d.size == 0:
        return 0.0, 0.0
    return float(np.quantile(d, quantile)), float(d.max())


def _gate(key, case, got, want):
    """Two-level gate of one output tensor against the emulation; `case` names the case in the failure message."""
    qn, gb, gm = GATES[key]
    bulk, mx = _errs(got, want, qn)
    print("%-28s %-44s bulk(q%g) %.3e  max %.3e  (gates %.1e / %.1e)" % (key, case, qn, bulk, mx, gb, gm))
    assert bulk <= gb and mx <= gm, "%s %s: bulk %.3e (gate %.1e), max %.3e (gate %.1e)" % (key, case, bulk, gb, mx, gm)


# ---------------------------------------------------------------------------------------------------------------------------
# BiLSTM, bf16 recurrence
# ---------------------------------------------------------------------------------------------------------------------------
def _lstm_params(num_layers, V=1000, E_=300, Hd=150):
    shapes = {"embedding.weight": (V, E_)}
    for layer in range(num_layers):
        for sfx in ("", "_reverse"):
            k = "lstm.%%s_l%d%s" % (layer, sfx)
            shapes[k % "weight_ih"] = (4 * Hd, E_ if layer == 0 else 2 * Hd)
            shapes[k % "weight_hh"] = (4 * Hd, Hd)
            shapes[k % "bias_ih"] = (4 * Hd,)
            shapes[k % "bias_hh"] = (4 * Hd,)
    return H.params_for(shapes)


@pytest.mark.parametrize("B,T", [(1, 1), (5, 24), (37, 100), (256, 100), (300, 100), (3, 230)])
@pytest.mark.parametrize("num_layers", [1, 2])
def test_bilstm_bf16_recurrence_matches_emulation(B, T, num_layers):
    """ops.bilstm(recurrence='bf16'), with and without the layer-0 projection folded into the embedding table: the fp32 rows and
    the bf16 side copy against oracle/bf16_path.bilstm (bf16 inputs / W_ih / W_hh / h of every step, fp32 gates and state)."""
    p = _lstm_params(num_layers)
    V = p["embedding.weight"].shape[0]
    rs = np.random.RandomState(100 * B + T + num_layers)
    lens = rs.randint(1, T + 1, size=B)
    lens[0] = T
    if B == 5:
        lens[2] = 0                                  # an empty text between live ones
    tok = rs.randint(1, V, size=(B, T))
    tok[np.arange(T)[None, :] >= lens[:, None]] = 0
    want_rows, want_bf = E.bilstm(p, tok, lens, 150, num_layers)
    weights = []
    for layer in range(num_layers):
        for sfx in ("", "_reverse"):
            k = "lstm.%%s_l%d%s" % (layer, sfx)
            weights.append(tuple(dev(p[k % n]) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
    for fold in (False, True):
        rows, bf = ops.bilstm(dev(tok).long(), dev(lens).long(), dev(p["embedding.weight"]), weights, 150, num_layers,
                              want_bf16=True, recurrence="bf16", cache=ops.LstmCache() if fold else None, fold=fold)
        case = "B=%d T=%d layers=%d fold=%d" % (B, T, num_layers, fold)
        _gate("lstm/rows", case, rows, want_rows)
        _gate("lstm/bf16", case, bf[..., :300].float(), want_bf)
        assert torch.equal(bf[..., :300], rows.to(torch.bfloat16)), case       # the side copy is RNE of the kernel's own rows
        assert torch.equal(bf[..., 300:].float().cpu(), torch.zeros(B, T, 20)), case


# ---------------------------------------------------------------------------------------------------------------------------
# layer tails
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hn", [1, 4, 8])
@pytest.mark.parametrize("B", [1, 37, 256, 300])
def test_mha_tail_bf16_terms1_matches_emulation(Hn, B):
    """ops.mha_tail_bf16(terms=1) -- the tail behind the faithful bf16 attention, bench.py's headline -- in the forms the model can
    select (one launch per tile, a cluster that shares the next projection, the K-split cluster with the projection as a launch of its
    own), with and without the next layer's projection, against oracle/bf16_path.layer_tail."""
    pc = H.params_for(H.mha_shapes(Hn), prefix="t.")
    pn = H.params_for(H.mha_shapes(Hn), prefix="n.")
    rs = np.random.RandomState(7 * Hn + B)
    o = (0.5 * rs.standard_normal((B, Hn * 128))).astype(np.float32)
    q = rs.standard_normal((B, 300)).astype(np.float32)
    a, f = "t.slf_attn.", "t.pos_ffn."
    wq, bq = pn["n.slf_attn.w_qs.weight"], pn["n.slf_attn.w_qs.bias"]
    sp = lambda w: ops.pack_weight_bf16_split(dev(w))
    pk = {"fc": sp(pc[a + "fc.weight"]), "w1": sp(pc[f + "w_1.weight"].squeeze(-1)), "w2": sp(pc[f + "w_2.weight"].squeeze(-1)),
          "fc_b": dev(pc[a + "fc.bias"]), "g1": dev(pc[a + "layer_norm.gamma"]), "be1": dev(pc[a + "layer_norm.beta"]),
          "b1": dev(pc[f + "w_1.bias"]), "b2": dev(pc[f + "w_2.bias"]), "g2": dev(pc[f + "layer_norm.gamma"]),
          "be2": dev(pc[f + "layer_norm.beta"])}
    nx = (sp(wq), dev(bq), Hn * 128)
    want, want_q = E.layer_tail(pc, "t", torch.from_numpy(o), torch.from_numpy(q), pc[a + "fc.weight"], pc[a + "fc.bias"], wq, bq)
    for ksplit, cluster in ((False, 1), (False, 0), (True, 0)):
        for nxt in (nx, None):
            out, qh = ops.mha_tail_bf16(dev(o), dev(q), pk, 1e-6, nxt, terms=1, ksplit=ksplit, cluster=cluster)
            case = "Hn=%d B=%d ksplit=%d cluster=%d next=%d" % (Hn, B, ksplit, cluster, nxt is not None)
            _gate("tail1/out", case, out, want)
            if nxt is not None:
                _gate("tail1/next", case, qh, want_q)


@pytest.mark.parametrize("Hn,B", [(8, 256), (8, 37), (4, 16), (1, 5), (8, 300)])
def test_mha_tail_c16_matches_emulation(Hn, B):
    """ops.mha_tail_c16 (behind the folded attention) in every cluster / K-split form, with and without the next composed query map
    u_next, against oracle/bf16_path.layer_tail on the same bf16 c."""
    g = torch.Generator(device=DEV).manual_seed(11 + Hn)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g) * 0.05
    HD = Hn * 300
    ldc = (HD + 31) // 32 * 32
    c = torch.zeros(B, ldc, device=DEV, dtype=torch.bfloat16)
    c[:, :HD] = torch.randn(B, HD, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(B, 300, device=DEV, generator=g)
    fc, w1, w2, wq = r(300, HD), r(300, 300), r(300, 300), r(HD, 300)
    pk = {"fc_b": r(300), "g1": r(300) + 1, "be1": r(300), "b1": r(300), "b2": r(300), "g2": r(300) + 1, "be2": r(300),
          "fc": ops.pack_weight_bf16_split(fc), "w1": ops.pack_weight_bf16_split(w1), "w2": ops.pack_weight_bf16_split(w2)}
    bq = r(HD)
    nx = (ops.pack_weight_bf16_split(wq), bq, HD)
    cpu = lambda t: t.detach().cpu()
    p = {"t.slf_attn.layer_norm.gamma": cpu(pk["g1"]), "t.slf_attn.layer_norm.beta": cpu(pk["be1"]),
         "t.pos_ffn.w_1.weight": cpu(w1), "t.pos_ffn.w_1.bias": cpu(pk["b1"]), "t.pos_ffn.w_2.weight": cpu(w2),
         "t.pos_ffn.w_2.bias": cpu(pk["b2"]), "t.pos_ffn.layer_norm.gamma": cpu(pk["g2"]), "t.pos_ffn.layer_norm.beta": cpu(pk["be2"])}
    want, want_u = E.layer_tail(p, "t", c[:, :HD].double().cpu(), cpu(q), cpu(fc), cpu(pk["fc_b"]), cpu(wq), cpu(bq), o_point=None)
    for cluster, ksplit in ((1, False), (2, False), (4, False), (0, True), (2, True), (4, True), (8, True)):
        for nxt in (nx, None):
            out, u = ops.mha_tail_c16(c, q, pk, 1e-6, nxt, cluster=cluster, ksplit=ksplit)
            case = "Hn=%d B=%d cluster=%d ksplit=%d next=%d" % (Hn, B, cluster, ksplit, nxt is not None)
            _gate("c16/out", case, out, want)
            if nxt is not None:
                _gate("c16/next", case, u, want_u)


def test_label_tail_bf16_terms1_matches_emulation():
    """ops.label_tail_bf16(terms=1) (model.label_tail_terms = 1) on the cases of test_fused_label_tail_bf16_vs_oracle, against
    oracle/bf16_path.label_tail (every product's operands rounded)."""
    g = H.load_golden("label_attention.npz")
    lq = dev(g["label_query"])
    for tag, C in (("object", 80), ("place", 365)):
        pc = H.params_for(H.label_attention_shapes(tag, C))
        p = {k: dev(v) for k, v in pc.items()}
        a = tag + "_attention."
        Q = ops.linear(lq, p[a + "w_q.weight"], p[a + "w_q.bias"])
        wc = ops.matmul(p[tag + "_linear_5.weight"], p[a + "fc.weight"])
        bc = ops.linear(p[a + "fc.bias"][None, :].contiguous(), p[tag + "_linear_5.weight"], p[tag + "_linear_5.bias"])[0].contiguous()
        sp = lambda w: ops.pack_weight_bf16_split(w.contiguous())
        packed = {"wk": sp(p[a + "w_k.weight"]), "bk": p[a + "w_k.bias"], "wv": sp(p[a + "w_v.weight"]), "bv": p[a + "w_v.bias"],
                  "wc": sp(wc), "bc": bc, "n5": 100, "C": C, "xl": sp(p[tag + "_x_linear.weight"]), "bxl": p[tag + "_x_linear.bias"],
                  "n_out": 300}
        rs = np.random.RandomState(C + 1)
        G = (0.05 * rs.standard_normal((C, 2048))).astype(np.float32)
        wq = (0.05 * rs.standard_normal((1024, 300))).astype(np.float32)
        bq = (0.05 * rs.standard_normal(1024)).astype(np.float32)
        nq = (sp(dev(wq)), dev(bq), 1024)
        Gp = sp(dev(G))
        for B in (1, 17, 64):
            halves = np.maximum(rs.standard_normal((B, 2, 2048)), 0).astype(np.float32)
            want, want_q = E.label_tail(pc, tag, torch.from_numpy(halves.max(axis=1)), torch.from_numpy(G), Q.cpu(), 5,
                                        torch.from_numpy(wq), torch.from_numpy(bq), terms=1)
            z, qh = ops.label_tail_bf16(dev(halves), Gp, Q, 5, packed, next_q=nq, terms=1)
            case = "%s B=%d" % (tag, B)
            _gate("label1/out", case, z, want)
            _gate("label1/next", case, qh, want_q)


# ---------------------------------------------------------------------------------------------------------------------------
# whole forward
# ---------------------------------------------------------------------------------------------------------------------------
def _plan_parts(model, call):
    """The forward's segments one after another on the caller's stream -> the context with every stage's result."""
    plan, ctx = model.forward_plan(*call)
    ctx.prepare()
    for _name, _skey, _deps, fn in plan:
        if fn is not None:
            fn()
    return ctx


def _check_forward(model, inp, idx, pmi, cfg, lq, attention, case):
    """Run the bf16 forward on the whole batch, the emulation on the samples `idx`, and gate every stage in forward order, so that a
    failure names the first stage that departs."""
    model.set_precision("bf16").set_attention(attention)
    call = call_args(inp, DEV)
    ctx = _plan_parts(model, call)
    logits = model(*call)
    ix = torch.as_tensor(idx, device=DEV)
    assert torch.equal(logits[ix], ctx["logits"][ix]), case          # the multi-stream forward == its segments run in order
    sub = {k: torch.as_tensor(v[idx] if k != "label_query" else v) for k, v in inp.items()}
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want, parts = E.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram, label_query=torch.as_tensor(lq),
                            attention=attention, return_parts=True)
    tb = ctx["text_bank"]
    assert torch.equal(tb.bf16[..., :300], tb.f32.to(torch.bfloat16)), case
    got = {"text_bank": tb.f32[ix], "text_bank_bf16": tb.bf16[ix][..., :300].float(),
           "bank_object": ctx["bank_obj"].bf16[ix][..., :300].float(), "bank_place": ctx["bank_place"].bf16[ix][..., :300].float(),
           "object_att": ctx["att_obj"][ix], "place_att": ctx["att_place"][ix],
           "tio": ctx["tio"][ix], "tip": ctx["tip"][ix], "iot": ctx["iot"][ix], "ipt": ctx["ipt"][ix], "logits": logits[ix]}
    parts["logits"] = want
    for part in PARTS:
        _gate("fwd_%s/%s" % (attention, part), case, got[part], parts[part])
    # the existing band against the fp32 network stays as a second check
    assert H.maxabs(logits[ix].cpu(), E.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram,
                                                  label_query=torch.as_tensor(lq), attention=attention, rounding=())) < 2e-2


@pytest.mark.parametrize("attention", ["faithful", "folded"])
@pytest.mark.parametrize("cfg_name", ["mvsa_single_b8", "tumemo_b64", "mvsa_multiple_b256"])
def test_bf16_forward_matches_emulation_on_golden_configs(cfg_name, attention):
    """The three golden configs at their own batch size (the fp64 emulation on at most 32 of the samples)."""
    g = H.load_golden("full_%s.npz" % cfg_name)
    adj = H.load_golden("adjacency.npz")
    cfg = synth.CONFIGS[cfg_name]
    B = int(g["B"])
    pmi, count = synth.synth_pmi(cfg.V, seed=cfg.seed + 17)
    model = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], g["label_query"], DEV)
    inp = synth.make_inputs(cfg, B=B, pmi=pmi)
    idx = np.arange(0, B, max(1, B // 32))
    _check_forward(model, inp, idx, pmi, cfg, g["label_query"], attention, "%s B=%d" % (cfg_name, B))


@pytest.mark.parametrize("attention", ["faithful", "folded"])
def test_bf16_forward_matches_emulation_across_the_imgbank_form_switch(attention):
    """B = 130: past the batch where the bf16 image bank leaves its two-workgroups-per-sample form (2 B <= CUs) for the stream form."""
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    adj = H.load_golden("adjacency.npz")
    lq = H.load_golden("full_mvsa_multiple_b256.npz")["label_query"]
    pmi, count = synth.synth_pmi(cfg.V, seed=cfg.seed + 17)
    model = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], lq, DEV)
    B = 130
    inp = synth.make_inputs(cfg, B=B, seed=77, pmi=pmi)
    idx = np.unique(np.concatenate([np.arange(0, B, 5)[:28], np.arange(B - 4, B)]))
    _check_forward(model, inp, idx, pmi, cfg, lq, attention, "mvsa_multiple B=%d" % B)


@pytest.mark.parametrize("attention", ["faithful", "folded"])
def test_bf16_forward_matches_emulation_on_a_padded_partial_batch(attention):
    """The batch of test_padded_partial_batch_with_trailing_empty_samples: the live samples in front of empty ones."""
    cfg = synth.CONFIGS["tumemo_b64"]
    adj = H.load_golden("adjacency.npz")
    lq = H.load_golden("label_attention.npz")["label_query"]
    pmi, count = synth.synth_pmi(cfg.V, seed=91)
    model = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], lq, DEV)
    B, live = 16, 11
    inp = synth.make_inputs(cfg, B=B, seed=31, pmi=pmi)
    inp["text"][live:] = 0
    inp["text_lens"][live:] = 0
    inp["text_mask"][live:] = 0
    _check_forward(model, inp, np.arange(live), pmi, cfg, lq, attention, "tumemo padded B=%d live=%d" % (B, live))
