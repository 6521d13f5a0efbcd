"""Training mode of the whole model above the CNN trunks and text encoders (csrc/model_train.hip, mgnns_amd/train.py) against
torch autograd in fp64 on the CPU over the reference's formulation (MODEL:88-133, 431-567), composed from oracle.restatement's
pinned pieces.  Dropout uses the masks the kernels drew (rebuilt from each module's last_dropout_seed); the text feature and the
text memory bank are constants from the eval kernels.  Gate: 1e-4 of each tensor's largest magnitude."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import harness, ops, synth
from mgnns_amd.model import Attention, GraphConvolution
from oracle import restatement as R
from tests import dropout_ref as DR
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 300

# parameters the reference's training graph never reaches (MODEL:431-567): gen_adj(A).detach(), the unused GRU, the dead gates
# and linears, the unused text->text attention; plus the frozen text encoders
NO_GRAD_PREFIXES = ("object_A", "place_A", "rnn.", "object_gate.", "place_gate.", "object_linear_1.", "object_linear_2.",
                    "object_linear_3.", "place_linear_1.", "place_linear_2.", "place_linear_3.", "text_object_text_multi_head_att.",
                    "text_place_text_multi_head_att.", "text_features.", "lstm.", "embedding.")
STACKS = ("img_object_text_multi_head_att", "img_place_text_multi_head_att", "text_img_object_multi_head_att",
          "text_img_place_multi_head_att")


def make(cfg_name, rates="reference", B=None, seed=7):
    cfg = synth.CONFIGS[cfg_name]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=B or cfg.B, seed=seed, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV)
    model.train().freeze_text_encoders()
    if rates == 0:
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    return cfg, model, inp


def drop(x, keep, rate):
    return x * keep.to(x.dtype) / (1.0 - rate) if rate < 1.0 else x * 0.0


def mask_of(seed, site, rate, shape):
    return ops.dropout_mask(seed, site, rate, shape, DEV).cpu()


def label_attention_ref(p, prefix, lq, x, n_heads, keep=None, rate=0.0):
    """MODEL:88-133 with dropout on softmax(energy) (the restatement's label_attention plus the mask)."""
    hid = p[prefix + ".w_q.weight"].shape[0]
    dh = hid // n_heads
    Q = F.linear(lq, p[prefix + ".w_q.weight"], p[prefix + ".w_q.bias"])
    K = F.linear(x, p[prefix + ".w_k.weight"], p[prefix + ".w_k.bias"])
    V = F.linear(x, p[prefix + ".w_v.weight"], p[prefix + ".w_v.bias"])
    NLQ, B = Q.shape[0], K.shape[0]
    att = torch.softmax(Q.view(1, NLQ, n_heads, dh) * K.view(B, 1, n_heads, dh) / math.sqrt(dh), dim=-1)
    if keep is not None:
        att = drop(att, keep.view(B, NLQ, n_heads, dh), rate)
    y = (att * V.view(B, 1, n_heads, dh)).reshape(B, NLQ, hid)
    return F.linear(y, p[prefix + ".fc.weight"], p[prefix + ".fc.bias"])


def image_gcn_ref(A, inp, w1, w2):
    adj = R.gen_adj(A.float()).double()
    return R.graph_convolution(F.leaky_relu(R.graph_convolution(inp, adj, w1), 0.2), adj, w2)


def mha_layer_ref(p, pre, q, bank, mask, H_, dk, keeps, rates):
    a, f = pre + ".slf_attn.", pre + ".pos_ffn."
    B, L, _ = bank.shape
    qh = F.linear(q, p[a + "w_qs.weight"], p[a + "w_qs.bias"]).view(B, H_, dk)
    kh = F.linear(bank, p[a + "w_ks.weight"], p[a + "w_ks.bias"]).view(B, L, H_, dk)
    vh = F.linear(bank, p[a + "w_vs.weight"], p[a + "w_vs.bias"]).view(B, L, H_, dk)
    s = torch.einsum("bhd,blhd->bhl", qh, kh) / math.sqrt(dk)
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, float("-inf"))
    ka, kf, kn = keeps
    pd = drop(torch.softmax(s, dim=2), ka.view(H_, B, L).permute(1, 0, 2), rates[0])
    o = torch.einsum("bhl,blhd->bhd", pd, vh).reshape(B, H_ * dk)
    y = R.layer_norm(drop(F.linear(o, p[a + "fc.weight"], p[a + "fc.bias"]), kf, rates[1]) + q, p[a + "layer_norm.gamma"],
                     p[a + "layer_norm.beta"])
    z = F.linear(F.relu(F.linear(y, p[f + "w_1.weight"].squeeze(-1), p[f + "w_1.bias"])), p[f + "w_2.weight"].squeeze(-1),
                 p[f + "w_2.bias"])
    return R.layer_norm(drop(z, kn, rates[2]) + y, p[f + "layer_norm.gamma"], p[f + "layer_norm.beta"])


def collect_masks(model, B, T, P):
    """Every dropout mask of the last training forward, rebuilt from the seeds the modules kept."""
    out = {}
    for st in STACKS:
        L = T if st.startswith("img_") else P
        for i, layer in enumerate(getattr(model, st)):
            sa, ff = layer.slf_attn, layer.pos_ffn
            out["%s.%d" % (st, i)] = (
                (mask_of(sa.last_dropout_seed, ops.DROP_ATTN, sa.attn_dropout.p, (model.n_head * B, 1, L)),
                 mask_of(sa.last_dropout_seed, ops.DROP_FC, sa.dropout.p, (B, D)),
                 mask_of(ff.last_dropout_seed, ops.DROP_FFN, ff.dropout.p, (B, D))),
                (sa.attn_dropout.p, sa.dropout.p, ff.dropout.p))
    for chan in ("object", "place"):
        att = getattr(model, chan + "_attention")
        NLQ = model.label_query.shape[0]
        out[chan + "_attention"] = (mask_of(att.last_dropout_seed, ops.DROP_LABEL_ATTN, att.do.p, (B, NLQ, D)), att.do.p)
    out["head"] = (mask_of(model.last_dropout_seed, ops.DROP_HEAD, model.dropout.p, (B, model.bi_hidden_size)), model.dropout.p)
    return out


def collect_host_masks(model, B, T, P):
    """collect_masks from the host restatement of the hash alone (tests/dropout_ref.py), at each site's documented layout;
    also -> the seed of every module that drops."""
    t = torch.from_numpy
    out, seeds = {}, []
    for st in STACKS:
        L = T if st.startswith("img_") else P
        for i, layer in enumerate(getattr(model, st)):
            sa, ff = layer.slf_attn, layer.pos_ffn
            seeds += [sa.last_dropout_seed, ff.last_dropout_seed]
            out["%s.%d" % (st, i)] = (
                (t(DR.attn_keep(sa.last_dropout_seed, sa.attn_dropout.p, model.n_head, B, L)),
                 t(DR.rows_keep(sa.last_dropout_seed, DR.DROP_FC, sa.dropout.p, B, D)),
                 t(DR.rows_keep(ff.last_dropout_seed, DR.DROP_FFN, ff.dropout.p, B, D))),
                (sa.attn_dropout.p, sa.dropout.p, ff.dropout.p))
    for chan in ("object", "place"):
        att = getattr(model, chan + "_attention")
        seeds.append(att.last_dropout_seed)
        out[chan + "_attention"] = (t(DR.label_keep(att.last_dropout_seed, att.do.p, B, model.label_query.shape[0], D)), att.do.p)
    seeds.append(model.last_dropout_seed)
    out["head"] = (t(DR.rows_keep(model.last_dropout_seed, DR.DROP_HEAD, model.dropout.p, B, model.bi_hidden_size)),
                   model.dropout.p)
    return out, seeds


def model_ref(p, model, consts, inp, masks):
    """fp64 training forward (MODEL:431-567) over the parameter dict p; consts: text feature, text bank, mask (constants)."""
    tf, tbank, tmask = consts
    lq = torch.as_tensor(inp["label_query"]).double()
    B = tf.shape[0]
    feat, bank = {}, {}
    for chan, A in (("object", "object_A"), ("place", "place_A")):
        f = torch.as_tensor(inp[chan + "_feature"]).double()
        bank[chan] = R.img_memory_bank(f, p["liner_img_%s.weight" % chan], p["liner_img_%s.bias" % chan])
        G = image_gcn_ref(p[A].detach(), torch.as_tensor(inp[chan + "_inp"])[0].double(), p["gc1.weight"], p["gc2.weight"])
        x = torch.matmul(R.max_pool(f), G.transpose(0, 1))
        keep, rate = masks[chan + "_attention"]
        y = label_attention_ref(p, chan + "_attention", lq, x, model.object_attention.n_heads, keep, rate)
        feat[chan] = R.label_attention_tail(p, chan, y)

    def stack(name, q, kv, m):
        for i in range(model.stack_num):
            keeps, rates = masks["%s.%d" % (name, i)]
            q = mha_layer_ref(p, "%s.%d" % (name, i), q, kv, m, model.n_head, model.d_kv, keeps, rates)
        return q

    iot = stack("img_object_text_multi_head_att", feat["object"], tbank, tmask)
    ipt = stack("img_place_text_multi_head_att", feat["place"], tbank, tmask)
    tio = stack("text_img_object_multi_head_att", tf, bank["object"], None)
    tip = stack("text_img_place_multi_head_att", tf, bank["place"], None)
    multi = F.linear(torch.cat([tio, tip, iot, ipt], dim=1), p["multi_linear_1.weight"], p["multi_linear_1.bias"])
    keep, rate = masks["head"]
    return F.linear(drop(multi, keep, rate), p["multi_linear_2.weight"], p["multi_linear_2.bias"])


def constants(model, args):
    with torch.no_grad():
        tf = model.text_features(args[0]).double().cpu()
        tbank = model._text_bank(args[0], args[1]).f32.double().cpu()
    return tf, tbank, args[2].double().cpu()


def ref_params(model):
    return {k: v.detach().double().cpu().requires_grad_(v.requires_grad) for k, v in model.named_parameters()}


def close(got, ref, what, tol=1e-4):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    assert err <= tol * scale + 1e-12, "%s: max err %.3e vs max |ref| %.3e" % (what, err, scale)


def train_step(model, args):
    model.zero_grad(set_to_none=True)
    logits = model(*args)
    assert logits.requires_grad
    logits.float().sum().backward()      # (a loss whose gradient is all ones: every logit is tested)
    return logits.detach()


@pytest.mark.parametrize("cfg_name,rates", [(c, r) for c in ("mvsa_single_b8", "tumemo_b64") for r in (0, "reference")]
                         + [("mvsa_multiple_b256", "reference")])          # (the configuration tools/bench_train.py times)
def test_whole_model_gradients_match_fp64(cfg_name, rates):
    cfg, model, inp = make(cfg_name, rates)
    args = harness.call_args(inp, DEV)
    logits = train_step(model, args)
    B, T = args[0].shape
    masks = collect_masks(model, B, T, args[3].shape[2] * args[3].shape[3])
    p = ref_params(model)
    ref = model_ref(p, model, constants(model, args), inp, masks)
    ref.sum().backward()
    close(logits, ref.detach(), "logits")
    got_none = {k for k, v in model.named_parameters() if v.grad is None}
    ref_none = {k for k, v in p.items() if v.grad is None}
    assert got_none == ref_none
    assert got_none == {k for k in p if k.startswith(NO_GRAD_PREFIXES)}
    for k, v in model.named_parameters():
        if v.grad is not None:
            close(v.grad, p[k].grad, k)


def test_whole_model_matches_fp64_under_host_restated_masks():
    """Every module's mask rebuilt from its last_dropout_seed by the host restatement alone: a kernel drawing at a wrong index
    would still agree with ops.dropout_mask (same hash, same mistake) but not with this."""
    cfg, model, inp = make("tumemo_b64")
    args = harness.call_args(inp, DEV)
    logits = train_step(model, args)
    B, T = args[0].shape
    masks, seeds = collect_host_masks(model, B, T, args[3].shape[2] * args[3].shape[3])
    assert len(seeds) == len(set(seeds)) == 4 * 2 * model.stack_num + 3, "two dropping modules drew the same seed"
    p = ref_params(model)
    ref = model_ref(p, model, constants(model, args), inp, masks)
    ref.sum().backward()
    close(logits, ref.detach(), "logits")
    for k, v in model.named_parameters():
        if v.grad is not None:
            close(v.grad, p[k].grad, k)


def padded_batch(rates, B=16, live=11):
    """tumemo_b64 with trailing empty samples, padded as the host pipeline pads a partial batch (batching.BatchAssembler: ids
    0, length 0, mask 0) -- the padding of test_model_gpu.py::test_padded_partial_batch_with_trailing_empty_samples."""
    cfg, model, inp = make("tumemo_b64", rates, B=B, seed=31)
    inp["text"][live:] = 0
    inp["text_lens"][live:] = 0
    inp["text_mask"][live:] = 0
    sub = {k: (v[:live] if k != "label_query" else v) for k, v in inp.items()}
    return model, harness.call_args(inp, DEV), harness.call_args(sub, DEV)


def live_grads(model, args, live):
    model.zero_grad(set_to_none=True)
    logits = model(*args)
    logits[:live].sum().backward()
    return logits.detach(), {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}


def test_trailing_empty_samples_do_not_poison_the_gradients():
    live = 11
    model, args, sub = padded_batch(0)
    logits, g = live_grads(model, args, live)
    ref_logits, ref = live_grads(model, sub, live)
    assert g.keys() == ref.keys() and g
    bad = [k for k, v in g.items() if not torch.isfinite(v).all()]
    assert not bad, "non-finite gradients with padded samples: %s" % bad[:8]
    close(logits[:live], ref_logits, "live logits")
    for k in ref:
        close(g[k], ref[k], k)


def test_trailing_empty_samples_at_reference_rates_then_adam_stay_finite():
    live = 11
    model, args, _ = padded_batch("reference")
    opt = torch.optim.Adam(model.get_config_optim(1e-3, 0.1), lr=1e-3)
    logits, g = live_grads(model, args, live)
    assert torch.isfinite(logits[:live]).all()
    bad = [k for k, v in g.items() if not torch.isfinite(v).all()]
    assert not bad, "non-finite gradients with padded samples: %s" % bad[:8]
    opt.step()
    bad = [k for k, v in model.named_parameters() if not torch.isfinite(v).all()]
    assert not bad, "non-finite weights after an Adam step: %s" % bad[:8]


@pytest.mark.parametrize("cfg_name,B", [("mvsa_single_b8", None), ("tumemo_b64", None), ("tumemo_b64", 1),
                                        ("mvsa_multiple_b256", None)])
def test_training_forward_at_rate_0_equals_the_eval_forward(cfg_name, B):
    """Two independent implementations of one function: the training chain at rate 0 and the fp32 eval forward (default
    attention form)."""
    cfg, model, inp = make(cfg_name, 0, B=B)
    args = harness.call_args(inp, DEV)
    train_logits = model(*args).detach()
    model.eval()
    assert model.precision == "fp32"
    with torch.no_grad():
        eval_logits = model(*args)
    assert torch.isfinite(train_logits).all()
    close(train_logits, eval_logits, "training logits at rate 0 vs eval")


def test_dropout_masks_and_seeds_reproduce_bit_for_bit():
    cfg, model, inp = make("tumemo_b64")
    args = harness.call_args(inp, DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        lg = train_step(model, args)
        runs.append((lg, {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys()
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    B = args[0].shape[0]
    masks = collect_masks(model, B, args[0].shape[1], 196)
    for name in ("object_attention", "place_attention", "head"):
        keep, rate = masks[name]
        n = keep.numel()
        frac = float(keep.float().mean())
        assert rate == 0.5 and abs(frac - 0.5) < 5 * math.sqrt(0.25 / n), (name, frac, n)
    torch.manual_seed(99)
    other = train_step(model, args)
    assert not torch.equal(other, runs[0][0])


def test_bank_weight_gradient_full_size_and_frozen_banks():
    g = torch.Generator(device=DEV).manual_seed(3)
    B, K, P, N = 256, 2048, 196, 300
    X = torch.rand(B, K, P, device=DEV, generator=g)
    dbank = torch.randn(B, P, N, device=DEV, generator=g)
    dW, db = ops.imgbank_wgrad(X, dbank)
    ref_w = torch.einsum("bpo,bcp->oc", dbank.double(), X.double())
    close(dW, ref_w, "dW")
    close(db, dbank.double().sum(dim=(0, 1)), "db")
    dW2, db2 = ops.imgbank_wgrad(X, dbank)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    # odd shapes: K not a multiple of the channel block, P not a multiple of 4, few samples
    X, dbank = torch.rand(3, 200, 49, device=DEV, generator=g), torch.randn(3, 49, 37, device=DEV, generator=g)
    dW, db = ops.imgbank_wgrad(X, dbank)
    close(dW, torch.einsum("bpo,bcp->oc", dbank.double(), X.double()), "dW small")
    close(db, dbank.double().sum(dim=(0, 1)), "db small")
    # frozen banks: no weight gradient (the kernel is not launched), the rest still trains
    cfg, model, inp = make("mvsa_single_b8")
    model.liner_img_object.requires_grad_(False)
    model.liner_img_place.requires_grad_(False)
    calls = []
    real = ops.imgbank_wgrad
    try:
        ops.imgbank_wgrad = lambda *a: calls.append(1) or real(*a)
        train_step(model, harness.call_args(inp, DEV))
    finally:
        ops.imgbank_wgrad = real
    assert not calls
    assert model.liner_img_object.weight.grad is None and model.liner_img_place.bias.grad is None
    assert model.multi_linear_1.weight.grad is not None and model.gc1.weight.grad is not None


@pytest.mark.parametrize("rate", [0.0, 0.5])
def test_label_attention_module_trains_like_fp64(rate):
    torch.manual_seed(5)
    att = Attention(hid_dim=300, image_dim=365, n_heads=5, dropout=rate).to(DEV).train()
    lq = torch.randn(7, 300, device=DEV)
    x = torch.randn(16, 365, device=DEV, requires_grad=True)
    out = att(query=lq, key=x, value=x)
    G = torch.randn_like(out)
    (out * G).sum().backward()
    p = {"a." + k: v.detach().double().cpu().requires_grad_(True) for k, v in att.named_parameters()}
    xr = x.detach().double().cpu().requires_grad_(True)
    keep = mask_of(att.last_dropout_seed, ops.DROP_LABEL_ATTN, rate, (16, 7, 300))
    ref = label_attention_ref(p, "a", lq.double().cpu(), xr, 5, keep, rate)
    if rate == 0.0:
        p32 = {k: v.detach().float() for k, v in p.items()}
        close(ref.detach(), R.label_attention(p32, "a", lq.cpu(), xr.detach().float(), 5), "restatement", tol=1e-5)
    (ref * G.double().cpu()).sum().backward()
    close(out.detach(), ref.detach(), "out")
    close(x.grad, xr.grad, "dx")
    for k, v in att.named_parameters():
        close(v.grad, p["a." + k].grad, k)


@pytest.mark.parametrize("which", ["object_t04_A", "place_t03_A"])
def test_graph_convolution_trains_with_the_transposed_adjacency(which):
    A = torch.as_tensor(H.load_golden("adjacency.npz")[which]).float()
    adj = R.gen_adj(A)                                   # not symmetric: the backward needs adj^T
    C = adj.shape[0]
    torch.manual_seed(6)
    gc1, gc2 = GraphConvolution(300, 1024).to(DEV).train(), GraphConvolution(1024, 2048).to(DEV).train()
    inp = torch.randn(C, 300, device=DEV, requires_grad=True)
    a = adj.to(DEV)
    out = gc2(gc1(inp, a, act=ops.ACT_LRELU2), a)
    G = torch.randn_like(out)
    (out * G).sum().backward()
    w1, w2 = (g.weight.detach().double().cpu().requires_grad_(True) for g in (gc1, gc2))
    xr = inp.detach().double().cpu().requires_grad_(True)
    ref = image_gcn_ref(A, xr, w1, w2)
    (ref * G.double().cpu()).sum().backward()
    close(out.detach(), ref.detach(), "G")
    close(gc1.weight.grad, w1.grad, "dW1")
    close(gc2.weight.grad, w2.grad, "dW2")
    close(inp.grad, xr.grad, "dinp")


def test_adam_steps_track_fp64_and_eval_uses_the_new_weights():
    cfg, model, inp = make("mvsa_single_b8")
    args = harness.call_args(inp, DEV)
    opt = torch.optim.Adam(model.get_config_optim(1e-3, 0.1), lr=1e-3)
    name_of = {id(v): k for k, v in model.named_parameters()}
    p = ref_params(model)
    ref_groups = [{"params": [p[name_of[id(v)]] for v in g["params"]], "lr": g["lr"]}
                  for g in model.get_config_optim(1e-3, 0.1)]
    ref_opt = torch.optim.Adam(ref_groups, lr=1e-3)
    consts = constants(model, args)
    B, T = args[0].shape
    with torch.no_grad():
        model.eval()
        warm = model(*args)                              # fills the eval caches, fp32 and bf16
        model.set_precision("bf16")
        model(*args)
        model.set_precision("fp32")
        model.train().freeze_text_encoders()
    assert warm.isfinite().all()
    for step in range(3):
        logits = train_step(model, args)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 10)
        opt.step()
        masks = collect_masks(model, B, T, 196)
        ref_opt.zero_grad(set_to_none=True)
        ref = model_ref(p, model, consts, inp, masks)
        ref.sum().backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), 10)
        ref_opt.step()
        close(logits, ref.detach(), "logits step %d" % step)
    # Adam normalises every element's step to ~lr: a gradient entry near zero whose fp32 rounding differs from fp64 can move the
    # other way, so single elements may differ by a few lr; the bulk must track (mean), the logits above carry the 1e-4 gate
    lr = 1e-3
    for k, v in model.named_parameters():
        d = (v.detach().double().cpu() - p[k].detach()).abs()
        assert float(d.max()) <= 3 * lr and float(d.mean()) <= 1e-2 * lr, (k, float(d.max()), float(d.mean()))
    model.eval()
    with torch.no_grad():
        got = model(*args).cpu()
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ti = {k: torch.as_tensor(v) for k, v in inp.items()}
        pmi, _ = synth.synth_pmi(cfg.V, seed=2)
        ref = R.forward(sd, ti, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram, label_query=torch.as_tensor(inp["label_query"]))
        assert float((got - ref).abs().max()) < 1e-4
        assert not torch.equal(got, warm.cpu())
        model.set_precision("bf16")
        assert model(*args).isfinite().all()
        model.set_precision("fp32")


def test_training_refusals():
    cfg, model, inp = make("mvsa_single_b8")
    args = list(harness.call_args(inp, DEV))
    model.lstm.eval().requires_grad_(True)               # unfrozen, eval mode
    with pytest.raises(RuntimeError, match="eval.*freeze_text_encoders"):
        model(*args)
    model.freeze_text_encoders()
    model.text_features.train()                          # frozen, training mode (its dropout would apply)
    with pytest.raises(RuntimeError, match="eval"):
        model(*args)
    model.freeze_text_encoders()
    imgs = list(args)
    imgs[3] = torch.zeros(args[0].shape[0], 3, 448, 448, device=DEV)
    with pytest.raises(NotImplementedError, match="feature maps"):
        model(*imgs)
    for prec in ("bf16", "bf16x3"):
        model.set_precision(prec)
        with pytest.raises(NotImplementedError, match="fp32"):
            model(*args)
    model.set_precision("fp32")
    model.is_regu = True
    with pytest.raises(NotImplementedError, match="is_regu"):
        model(*args)
    model.is_regu = False
    assert model(*args).requires_grad


def test_dropout_op_masks_and_backward():
    x = torch.randn(4096, 300, device=DEV)
    y, keep, kb = ops.dropout(x, 77, ops.DROP_HEAD, 0.5, return_masks=True)
    assert torch.equal(kb, ops.dropout_mask(77, ops.DROP_HEAD, 0.5, x.shape, DEV))
    assert torch.equal(y, torch.where(kb, x * 2.0, torch.zeros_like(x)))
    frac = float(kb.float().mean())
    assert abs(frac - 0.5) < 5 * math.sqrt(0.25 / kb.numel())
    dy = torch.randn_like(x)
    assert torch.equal(ops.dropout_backward(dy, keep, 0.5), torch.where(kb, dy * 2.0, torch.zeros_like(dy)))
    a, b = torch.randn(1000, device=DEV), torch.randn(1000, device=DEV)
    assert torch.equal(ops.train_eltwise(ops.ELT_LRELU2_BWD, a, b), torch.where(b > 0, a, 0.2 * a))
    assert np.isclose(ops.dropout_mask(1, ops.DROP_LABEL_ATTN, 0.0, (10,), DEV).float().mean().item(), 1.0)
