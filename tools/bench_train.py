#!/usr/bin/env python
"""Training mode of one MyMultiHeadAttention layer (csrc/mha_train.hip) at B=256, H=4: L=196 unmasked and L=100 masked (ragged
lengths).  HIP events around n calls: the layer's training forward + backward, each new entry point with its algorithmic bytes
and achieved GB/s, and for context the same layer through plain torch autograd (fp32, on the GPU).  One JSON line per case.
The last line is the whole model (csrc/model_train.hip) at mvsa_multiple_b256 in fp32: the training forward + backward step,
the image-bank weight-gradient kernel alone with its % of the 155 TF fp32 matrix peak, and plain torch autograd over the same
formulation.
--text: the text encoders' training (csrc/text_train.hip) at mvsa_multiple_b256 in fp32 -- the whole-model step with frozen and
with trainable encoders, each new kernel alone (with algorithmic bytes or FLOPs), and plain torch autograd over the same text
formulation (nn.LSTM on packed sequences, a scatter-max text GCN).
--maps: the feature maps' gradient (csrc/map_grad.hip) at mvsa_multiple_b256 in fp32 -- the whole-model step without and with
map gradients, imgbank_dgrad alone (dense, and with the max-pool scatter) with its % of the fp32 matrix peak next to imgbank_wgrad
at the same shape, map_argmax alone with its GB/s next to a torch copy of the same bytes, and torch autograd's F.linear
backward-to-input at the same shape.
--bank-precision fp32|bf16x3 (with --model-only or --maps): the model's set_train_bank_precision for the step timings; with
bf16x3, --maps also times the three image-bank products (forward, wgrad, dgrad) in both forms and the whole step in both modes,
alternately in one process, three rounds each, best and all rounds reported (csrc/bank_grad_split.hip).
--trunk: frozen-statistics fine-tuning of the trunks' layer4 (csrc/conv_train.hip) at mvsa_multiple_b256 -- the training step with
precomputed maps against the step with [B,3,448,448] images and unfreeze_trunks() (ResNet-101 / ResNet-50 trunks; --batch N for a
smaller batch), three alternating rounds, and each new kernel alone per layer4 geometry with its FLOPs and share of the 2.5 PF bf16
matrix peak (1x1 layers also algorithmic bytes and TB/s).
--trunk --batchnorm batch: fine-tuning layer4 with batch statistics (csrc/bn_train.hip) -- the step with images under
unfreeze_trunks() against unfreeze_trunks(batchnorm='batch'), three alternating rounds, and each BatchNorm kernel alone at layer4's
[M, C] shapes (M = B*14*14 with C = 512 and 2048, M = B*28*28 with C = 512), alternately with a torch copy_ that moves the same
number of bytes (read + written), three rounds, best quoted, with the ratio kernel / copy; --kernels-only stops after the kernels.
--trunk --stem: fine-tuning the whole trunk, stem included (csrc/stem_train.hip) -- maxpool3x3s2_bwd with the ReLU mask at the stem's
[B,224,224,64] alternately with a torch copy_ of the same bytes, stem_wgrad (with its reduce launch) at [B,3,448,448] alternately with
conv_wgrad at layer4.0.conv2's geometry (its % of the 2.5 PF bf16 peak and the ratio), the raw stem forward next to the folded one, and
the step with images under unfreeze_trunks(4) against unfreeze_trunks(4, stem=True) in each BatchNorm mode; three alternating rounds,
best quoted; --kernels-only stops after the kernels, --batch N sizes everything.
--steps-only K: nothing but K whole-model training steps with map gradients in the chosen bank precision -- the run a kernel
trace is taken of (rocprofv3 --kernel-trace --stats, as tools/prof.sh does for bench.py; table by tools/rocpd_stats.py).
Usage: python tools/bench_train.py [--iters N] [--model-only | --text | --maps | --trunk [--batchnorm batch [--kernels-only]] [--batch N] | --steps-only K] [--bank-precision fp32|bf16x3]"""
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgnns_amd import fusion, ops  # noqa: E402

DEV = "cuda:0"
D, DK = 300, 128


def timeit(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def torch_layer(p, q, bank, mask, H):
    """The reference's formulation in plain torch (K and V projected), training-mode dropout."""
    B, L, _ = bank.shape
    qh = F.linear(q, p["wq"], p["bq"]).view(B, H, DK)
    kh = F.linear(bank, p["wk"], p["bk"]).view(B, L, H, DK)
    vh = F.linear(bank, p["wv"], p["bv"]).view(B, L, H, DK)
    s = torch.einsum("bhd,blhd->bhl", qh, kh) / math.sqrt(DK)
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, float("-inf"))
    pa = F.dropout(torch.softmax(s, dim=2), 0.1)
    o = torch.einsum("bhl,blhd->bhd", pa, vh).reshape(B, H * DK)

    def ln(x, g, b):
        return g * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-6) + b

    y = ln(F.dropout(F.linear(o, p["wfc"], p["bfc"]), 0.1) + q, p["g1"], p["be1"])
    z = F.linear(F.relu(F.linear(y, p["w1"], p["b1"])), p["w2"], p["b2"])
    return ln(F.dropout(z, 0.1) + y, p["g2"], p["be2"])


def case(B, H, L, masked, n):
    torch.manual_seed(0)
    m = fusion.MyMultiHeadAttention(H, D, DK, dropout=0.1).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(1)
    q = torch.randn(B, D, device=DEV, generator=g).requires_grad_(True)
    bank = torch.randn(B, L, D, device=DEV, generator=g).requires_grad_(True)
    G = torch.randn(B, D, device=DEV, generator=g)
    mask, live = None, B * L
    if masked:
        lens = torch.randint(1, L + 1, (B,), device=DEV, generator=g)
        mask = (torch.arange(L, device=DEV)[None, :] < lens[:, None]).float()
        live = int(lens.sum())
    res = {"case": "B%d_H%d_L%d_%s" % (B, H, L, "masked" if masked else "full"), "live_rows": live}

    def layer_fwd():
        return m(q, bank, bank, mask)[0]

    def layer_fwd_bwd():
        out = layer_fwd()
        torch.autograd.backward(out, G)

    res["layer_fwd_us"] = timeit(lambda: layer_fwd(), n)
    res["layer_fwd_bwd_us"] = timeit(layer_fwd_bwd, n)

    # the new entry points on their own, at the layer's shapes
    a = m.slf_attn
    wk, wv, bv = a.w_ks.weight.detach(), a.w_vs.weight.detach(), a.w_vs.bias.detach()
    qh = torch.randn(B, H * DK, device=DEV, generator=g)
    x = bank.detach()
    o, attn, saved = ops.mha_attn_train(qh, x, mask, H, DK, wk, wv, bv, 7, 0.1)
    dO = torch.randn(B, H * DK, device=DEV, generator=g)
    f4 = 4
    xbytes = live * D * f4                                            # one read of the live bank rows
    hbl = H * B * L * f4
    kern = {}
    t = timeit(lambda: ops.mha_attn_train(qh, x, mask, H, DK, wk, wv, bv, 7, 0.1), n)
    by = xbytes + 2 * H * DK * D * f4 + 3 * hbl + hbl // 4 + 3 * H * B * D * f4 + B * H * DK * f4
    kern["mha_train_fwd"] = (t, by)
    t = timeit(lambda: ops.mha_attn_train_backward(dO, qh, x, mask, wk, wv, bv, saved, want_dbank=True), n)
    by = 2 * xbytes + B * L * D * f4 + 3 * hbl + 5 * H * B * D * f4 + 4 * H * DK * D * f4 + 2 * B * H * DK * f4
    kern["mha_train_bwd (bank x2 + dbank)"] = (t, by)
    y = torch.randn(B, D, device=DEV, generator=g)
    gam, bet = a.layer_norm.gamma.detach(), a.layer_norm.beta.detach()
    _, ln_saved = ops.dropout_residual_layernorm(y, y, gam, bet, 1e-6, 3, ops.DROP_FC, 0.1)
    t = timeit(lambda: ops.dropout_residual_layernorm(y, y, gam, bet, 1e-6, 3, ops.DROP_FC, 0.1), n)
    kern["drop_res_ln_fwd"] = (t, 4 * B * D * f4 + B * D)
    t = timeit(lambda: ops.dropout_residual_layernorm_backward(y, gam, ln_saved), n)
    kern["drop_res_ln_bwd"] = (t, 5 * B * D * f4 + B * D)
    t = timeit(lambda: ops.wgrad(y, y), n)
    kern["wgrad 300x300"] = (t, 2 * B * D * f4 + D * D * f4)
    res["kernels"] = {k: {"us": round(v[0], 2), "alg_bytes": v[1], "GB/s": round(v[1] / v[0] / 1e3, 1)} for k, v in kern.items()}

    # plain torch autograd, same layer, fp32 on the GPU
    f = m.pos_ffn
    p = {"wq": a.w_qs.weight, "bq": a.w_qs.bias, "wk": a.w_ks.weight, "bk": a.w_ks.bias, "wv": a.w_vs.weight, "bv": a.w_vs.bias,
         "wfc": a.fc.weight, "bfc": a.fc.bias, "g1": a.layer_norm.gamma, "be1": a.layer_norm.beta,
         "w1": f.w_1.weight.view(D, D), "b1": f.w_1.bias, "w2": f.w_2.weight.view(D, D), "b2": f.w_2.bias,
         "g2": f.layer_norm.gamma, "be2": f.layer_norm.beta}

    def torch_fwd_bwd():
        torch.autograd.backward(torch_layer(p, q, bank, mask, H), G)

    res["torch_fwd_us"] = timeit(lambda: torch_layer(p, q, bank, mask, H), n)
    res["torch_fwd_bwd_us"] = timeit(torch_fwd_bwd, n)
    for k in ("layer_fwd_us", "layer_fwd_bwd_us", "torch_fwd_us", "torch_fwd_bwd_us"):
        res[k] = round(res[k], 1)
    return res


FP32_PEAK = 155e12        # measured exact-f32 MFMA peak of the MI355X


def torch_model(model, tf, tbank, tmask, maps, inps, lq):
    """The reference's training forward (MODEL:88-133, 431-567) in plain fp32 torch over the model's own parameters: the same
    formulation the HIP chain computes (text feature and text bank as constants, every dropout site)."""
    from oracle import restatement as R
    B = tf.shape[0]
    feat, bank = {}, {}
    for tag, chan in (("obj", "object"), ("place", "place")):
        lin, att = getattr(model, "liner_img_" + chan), getattr(model, chan + "_attention")
        f = maps[tag]
        bank[tag] = F.linear(f.reshape(B, f.shape[1], -1).transpose(1, 2), lin.weight, lin.bias)
        adj = R.gen_adj(getattr(model, chan + "_A").detach())
        G = adj @ (F.leaky_relu(adj @ (inps[tag][0] @ model.gc1.weight), 0.2) @ model.gc2.weight)
        x = f.reshape(B, f.shape[1], -1).amax(dim=2) @ G.t()
        nh = att.n_heads
        dh = 300 // nh
        Q, K, V = att.w_q(lq).view(1, -1, nh, dh), att.w_k(x).view(B, 1, nh, dh), att.w_v(x).view(B, 1, nh, dh)
        y = att.fc((F.dropout(torch.softmax(Q * K / math.sqrt(dh), dim=-1), att.do.p) * V).reshape(B, -1, 300))
        feat[tag] = getattr(model, chan + "_x_linear")(getattr(model, chan + "_linear_5")(y).reshape(B, -1))

    def ln(x, g, b):
        return g * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-6) + b

    def layer(m, q, kv, mask):
        a, f = m.slf_attn, m.pos_ffn
        H, dk, L = a.n_head, a.d_k, kv.shape[1]
        qh = a.w_qs(q).view(B, H, dk)
        kh, vh = a.w_ks(kv).view(B, L, H, dk), a.w_vs(kv).view(B, L, H, dk)
        s_ = torch.einsum("bhd,blhd->bhl", qh, kh) / math.sqrt(dk)
        if mask is not None:
            s_ = s_.masked_fill(mask[:, None, :] == 0, float("-inf"))
        o = torch.einsum("bhl,blhd->bhd", F.dropout(torch.softmax(s_, dim=2), a.attn_dropout.p), vh).reshape(B, -1)
        y = ln(F.dropout(a.fc(o), a.dropout.p) + q, a.layer_norm.gamma, a.layer_norm.beta)
        z = F.linear(F.relu(F.linear(y, f.w_1.weight.squeeze(-1), f.w_1.bias)), f.w_2.weight.squeeze(-1), f.w_2.bias)
        return ln(F.dropout(z, f.dropout.p) + y, f.layer_norm.gamma, f.layer_norm.beta)

    def stack(layers, q, kv, mask):
        for m in layers:
            q = layer(m, q, kv, mask)
        return q

    multi = torch.cat([stack(model.text_img_object_multi_head_att, tf, bank["obj"], None),
                       stack(model.text_img_place_multi_head_att, tf, bank["place"], None),
                       stack(model.img_object_text_multi_head_att, feat["obj"], tbank, tmask),
                       stack(model.img_place_text_multi_head_att, feat["place"], tbank, tmask)], dim=1)
    return model.multi_linear_2(F.dropout(model.multi_linear_1(multi), model.dropout.p))


def bank_precision():
    mode = sys.argv[sys.argv.index("--bank-precision") + 1] if "--bank-precision" in sys.argv else "fp32"
    if mode not in ("fp32", "bf16x3"):
        raise SystemExit("bench_train: --bank-precision fp32|bf16x3")
    return mode


def model_case(n):
    from mgnns_amd import harness, synth
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=cfg.B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV).train().freeze_text_encoders()
    model.set_train_bank_precision(bank_precision())
    args = harness.call_args(inp, DEV)
    B = args[0].shape[0]
    G = torch.randn(B, cfg.NL, device=DEV)
    res = {"case": "model_%s_fp32" % cfg.name, "B": B, "bank_precision": model.train_bank_precision}

    def step():
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(model(*args), G)

    res["model_fwd_us"] = timeit(lambda: model(*args), n)
    res["model_fwd_bwd_us"] = timeit(step, n)
    f3 = args[3].float().contiguous().view(B, args[3].shape[1], -1)
    K, P, N = f3.shape[1], f3.shape[2], model.liner_img_object.out_features
    dbank = torch.randn(B, P, N, device=DEV)
    t = timeit(lambda: ops.imgbank_wgrad(f3, dbank), n)
    flop = 2.0 * B * P * K * N
    res["bank_wgrad"] = {"us": round(t, 1), "GFLOP": round(flop / 1e9, 1), "TF/s": round(flop / t / 1e6, 1),
                         "pct_fp32_peak": round(100.0 * flop / t / 1e6 / (FP32_PEAK / 1e12), 1)}
    with torch.no_grad():
        tf = model.text_features(args[0])
        tbank = model._text_bank(args[0], args[1]).f32
    maps = {"obj": args[3].float(), "place": args[4].float()}
    inps = {"obj": args[5].float(), "place": args[6].float()}
    lq = model.label_query.float()

    def torch_step():
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(torch_model(model, tf, tbank, args[2].float(), maps, inps, lq), G)

    res["torch_fwd_bwd_us"] = timeit(torch_step, n)
    for k in ("model_fwd_us", "model_fwd_bwd_us", "torch_fwd_bwd_us"):
        res[k] = round(res[k], 1)
    return res


def text_case(n):
    import numpy as np
    from mgnns_amd import harness, synth
    from mgnns_amd import train as T_
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=cfg.B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV).train().freeze_text_encoders()
    args = harness.call_args(inp, DEV)
    B, T = args[0].shape
    G = torch.randn(B, cfg.NL, device=DEV)
    res = {"case": "text_%s_fp32" % cfg.name, "B": B, "T": T}

    def step():
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(model(*args), G)

    res["model_fwd_bwd_frozen_us"] = timeit(step, n)
    model.unfreeze_text_encoders()
    res["model_fwd_bwd_trainable_us"] = timeit(step, n)
    tok, lens = args[0].long().contiguous(), args[1].to(DEV).long().contiguous()
    rows = int(lens.clamp(0, T).sum())
    emb, lstm = model.embedding.weight.detach(), model.lstm
    ws = [tuple(getattr(lstm, "%s_l%d%s" % (k, l, s)).detach() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
          for l in range(2) for s in ("", "_reverse")]
    rate = lstm.dropout
    bank, saved = ops.bilstm_train(tok, lens, emb, ws, 150, 2, 5, rate)
    t_fwd = timeit(lambda: ops.bilstm_train(tok, lens, emb, ws, 150, 2, 5, rate), n)
    t_eval = timeit(lambda: ops.bilstm(tok, lens, emb, ws, 150, 2, recurrence="f32"), n)
    dbank = torch.randn_like(bank)
    t_bwd = timeit(lambda: ops.bilstm_train_backward(dbank, saved, ws, emb), n)
    dz = torch.empty(rows, 1200, device=DEV)

    def rec():
        ops._lib.call("mgnns_bilstm_train_bwd_rec", ops._p(dbank), ops._p(lens), B, T, ops._p(saved["meta"]), saved["rows"],
                      ops._p(saved["gates"][1]), ops._p(saved["cells"][1]), ops._p(ws[2][1]), ops._p(ws[3][1]), ops._p(dz), ops._stream())
    t_rec = timeit(rec, n)
    res["bilstm"] = {"rows": rows, "eval_fwd_us": round(t_eval, 1), "train_fwd_us": round(t_fwd, 1), "bwd_us": round(t_bwd, 1),
                     "bwd_rec_one_layer_us": round(t_rec, 1),
                     "bwd_rec_MB": round(rows * (600 + 150 + 150 + 1200 + 150) * 4 / 1e6, 1)}
    tg = model.text_features
    pmi_dev = tg.edges_matrix.device_arrays(tok.device)
    nh, ew = tg.node_hidden.weight.detach(), tg.seq_edge_w.weight.detach()
    out, ts = ops.textgcn_train(tok, nh, ew, pmi_dev, tg.ngram, tg.max_length, 5, tg.dropout.p)
    dy = torch.randn_like(out)
    t_tf = timeit(lambda: ops.textgcn_train(tok, nh, ew, pmi_dev, tg.ngram, tg.max_length, 5, tg.dropout.p), n)
    t_tb = timeit(lambda: ops.textgcn_train_backward(dy, tok, nh, ew, pmi_dev, ts), n)
    keys = torch.randint(0, nh.shape[0], (rows,), device=DEV)
    vals = torch.randn(rows, 300, device=DEV)
    t_ks = timeit(lambda: ops.keyed_row_sum(keys, vals, nh.shape[0]), n)
    res["text_gcn"] = {"train_fwd_us": round(t_tf, 1), "bwd_us": round(t_tb, 1),
                       "keyed_sum_rows": rows, "keyed_sum_us": round(t_ks, 1),
                       "keyed_sum_GB/s": round((rows * 300 * 4 * 2 + nh.numel() * 4) / t_ks / 1e3, 1)}
    # plain torch autograd over the same formulation
    tl = torch.nn.LSTM(300, 150, 2, bidirectional=True, batch_first=True, dropout=rate).to(DEV)
    te = torch.nn.Embedding(emb.shape[0], 300, padding_idx=0).to(DEV)
    lens_cpu = lens.clamp(min=1).cpu()

    def torch_lstm():
        x = torch.nn.utils.rnn.pack_padded_sequence(te(tok), lens_cpu, batch_first=True, enforce_sorted=False)
        o, _ = tl(x)
        o, _ = torch.nn.utils.rnn.pad_packed_sequence(o, batch_first=True, total_length=T)
        o.backward(dbank)
    res["torch_lstm_fwd_bwd_us"] = round(timeit(torch_lstm, n), 1)
    toks = tok.cpu().numpy()
    src, dst, eid, doc = [], [], [], []
    node_base = 0
    for b in range(B):
        t = [int(x) for x in toks[b][:tg.max_length] if x != 0]
        nodes = {}
        for v in t:
            nodes.setdefault(v, node_base + len(nodes))
        for i, u in enumerate(t):
            for j in range(max(0, i - tg.ngram), min(len(t), i + tg.ngram + 1)):
                src.append(u); dst.append(nodes[t[j]]); eid.append(tg.edges_matrix[u, t[j]])
        doc += [b] * len(nodes)
        node_base += len(nodes)
    src, dst, eid = (torch.tensor(a, device=DEV, dtype=torch.long) for a in (src, dst, eid))
    doc = torch.tensor(doc, device=DEV, dtype=torch.long)
    tnh = tg.node_hidden.weight.detach().clone().requires_grad_()
    tew = tg.seq_edge_w.weight.detach().clone().requires_grad_()

    def torch_gcn():
        msg = tew[eid] * tnh[src]
        h = torch.full((node_base, 300), -float("inf"), device=DEV).scatter_reduce(0, dst[:, None].expand(-1, 300), msg, "amax")
        s = torch.zeros(B, 300, device=DEV).index_add(0, doc, h)
        torch.relu(F.dropout(s, tg.dropout.p)).backward(dy)
    res["torch_textgcn_fwd_bwd_us"] = round(timeit(torch_gcn, n), 1)
    for k in ("model_fwd_bwd_frozen_us", "model_fwd_bwd_trainable_us"):
        res[k] = round(res[k], 1)
    return res


def maps_case(n):
    from mgnns_amd import harness, synth
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=cfg.B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV).train().freeze_text_encoders()
    mode = bank_precision()
    model.set_train_bank_precision(mode)
    args = list(harness.call_args(inp, DEV))
    plain = list(args)
    B = args[0].shape[0]
    G = torch.randn(B, cfg.NL, device=DEV)
    res = {"case": "maps_%s_fp32" % cfg.name, "B": B, "bank_precision": mode}

    def step():
        model.zero_grad(set_to_none=True)
        args[3].grad = args[4].grad = None
        torch.autograd.backward(model(*args), G)

    res["model_fwd_bwd_us"] = round(timeit(step, n), 1)
    for i in (3, 4):
        args[i] = args[i].detach().clone().requires_grad_(True)
    res["model_fwd_bwd_map_grads_us"] = round(timeit(step, n), 1)
    assert args[3].grad is not None and args[4].grad is not None

    f3 = args[3].detach().float().contiguous().view(B, args[3].shape[1], -1)
    K, P = f3.shape[1], f3.shape[2]
    W = model.liner_img_object.weight.detach()
    N = W.shape[0]
    dbank = torch.randn(B, P, N, device=DEV)
    dpooled = torch.randn(B, K, device=DEV)
    arg = ops.map_argmax(f3)
    flop = 2.0 * B * P * K * N

    def mfma(t):
        return {"us": round(t, 1), "GFLOP": round(flop / 1e9, 1), "TF/s": round(flop / t / 1e6, 1),
                "pct_fp32_peak": round(100.0 * flop / t / 1e6 / (FP32_PEAK / 1e12), 1)}

    # interleaved, so that a clock drift between the two kernels shows in both
    tw, td = [], []
    for _ in range(3):
        tw.append(timeit(lambda: ops.imgbank_wgrad(f3, dbank), n))
        td.append(timeit(lambda: ops.imgbank_dgrad(dbank, W), n))
    res["bank_wgrad"] = dict(mfma(min(tw)), runs_us=[round(t, 1) for t in tw])
    res["bank_dgrad"] = dict(mfma(min(td)), runs_us=[round(t, 1) for t in td], vs_wgrad=round(min(td) / min(tw), 3))
    res["bank_dgrad_with_scatter"] = mfma(timeit(lambda: ops.imgbank_dgrad(dbank, W, dpooled, arg), n))
    res["bank_dgrad_pooled_only_us"] = round(timeit(lambda: ops.imgbank_dgrad(None, W, dpooled, arg, positions=P), n), 1)
    nbytes = f3.numel() * 4
    t = timeit(lambda: ops.map_argmax(f3), n)
    res["map_argmax"] = {"us": round(t, 1), "MB": round(nbytes / 1e6, 1), "GB/s": round(nbytes / t / 1e3, 1)}
    dst = torch.empty_like(f3)
    t = timeit(lambda: dst.copy_(f3), n)
    res["torch_copy_same_bytes"] = {"us": round(t, 1), "read_GB/s": round(nbytes / t / 1e3, 1)}
    del dst
    # torch autograd: the bank as F.linear over the transposed map, backward to the input only
    xt = f3.transpose(1, 2).contiguous().requires_grad_(True)                 # [B, P, K]

    def torch_dgrad():
        xt.grad = None
        torch.autograd.backward(F.linear(xt, W), dbank)
    t_all = timeit(torch_dgrad, n)
    t_fwd = timeit(lambda: F.linear(xt.detach(), W), n)
    res["torch_linear_bwd_to_input_us"] = round(t_all - t_fwd, 1)
    if mode == "bf16x3":
        res["split_vs_fp32"] = split_case(model, args, plain, step, f3, W, dbank, dpooled, arg, n)
    return res


def split_case(model, args, plain, step, f3, W, dbank, dpooled, arg, n):
    """The image bank's three products in both forms, and the whole step in both modes: alternately, three rounds each."""
    lin = model.liner_img_object
    N = W.shape[0]
    wt, wp, bias = model._wt(lin), model._wp_split(lin), lin.bias.detach()
    pairs = {
        "bank_fwd": (lambda: ops.imgbank_pool(f3, wt, bias, N), lambda: ops.imgbank_pool_split(f3, wp, bias, N)),
        "bank_wgrad": (lambda: ops.imgbank_wgrad(f3, dbank), lambda: ops.imgbank_wgrad(f3, dbank, split=True)),
        "bank_dgrad": (lambda: ops.imgbank_dgrad(dbank, W), lambda: ops.imgbank_dgrad(dbank, W, split=True)),
        "bank_dgrad_with_scatter": (lambda: ops.imgbank_dgrad(dbank, W, dpooled, arg),
                                    lambda: ops.imgbank_dgrad(dbank, W, dpooled, arg, split=True)),
    }
    out = {}
    for name, (f32, spl) in pairs.items():
        ta, tb = [], []
        for _ in range(3):
            ta.append(timeit(f32, n))
            tb.append(timeit(spl, n))
        out[name] = {"fp32_us": round(min(ta), 1), "bf16x3_us": round(min(tb), 1), "ratio": round(min(tb) / min(ta), 3),
                     "fp32_runs_us": [round(t, 1) for t in ta], "bf16x3_runs_us": [round(t, 1) for t in tb]}
    leaves = list(args)
    for key, use in (("step_map_grads", leaves), ("step", plain)):
        args[:] = use
        ta, tb, tc = [], [], []
        for _ in range(3):
            model.set_train_bank_precision("fp32")
            ta.append(timeit(step, n))
            model.set_train_bank_precision("bf16x3")
            tb.append(timeit(step, n))
            model.train_bank_split_forward = True
            tc.append(timeit(step, n))
            model.train_bank_split_forward = False
        out[key] = {"fp32_us": round(min(ta), 1), "bf16x3_us": round(min(tb), 1), "ratio": round(min(tb) / min(ta), 3),
                    "bf16x3_split_forward_us": round(min(tc), 1), "fp32_runs_us": [round(t, 1) for t in ta],
                    "bf16x3_runs_us": [round(t, 1) for t in tb], "bf16x3_split_forward_runs_us": [round(t, 1) for t in tc]}
    args[:] = leaves
    return out


BF16_PEAK = 2.5e15        # bf16 MFMA, dense

# layer4 of a bottleneck ResNet at 448 x 448 (its input is 28 x 28 x 1024): (name, H, W, Cin, Cout, k, stride, how many per trunk)
LAYER4 = [("4.0.conv1", 28, 28, 1024, 512, 1, 1, 1), ("4.0.conv2", 28, 28, 512, 512, 3, 2, 1), ("4.0.downsample", 28, 28, 1024, 2048, 1, 2, 1),
          ("4.x.conv3", 14, 14, 512, 2048, 1, 1, 3), ("4.1-2.conv1", 14, 14, 2048, 512, 1, 1, 2), ("4.1-2.conv2", 14, 14, 512, 512, 3, 1, 2)]


def trunk_case(n):
    from mgnns_amd import harness, synth
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    B = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else cfg.B
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV, trunks=True).train().freeze_text_encoders()
    args = list(harness.call_args(inp, DEV))
    G = torch.randn(B, cfg.NL, device=DEV)
    g = torch.Generator().manual_seed(1)
    imgs = list(args)
    for i in (3, 4):
        imgs[i] = torch.randn(B, 3, 448, 448, generator=g).to(DEV)
    res = {"case": "trunk_%s" % cfg.name, "B": B, "device": torch.cuda.get_device_name(0), "iters": n}

    def step(a):
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(model(*a), G)

    with torch.no_grad():
        model.eval()
        fwd = [timeit(lambda: (model.object_features(imgs[3]), model.place_features(imgs[4])), n, warm=1) for _ in range(2)]
        model.train().freeze_text_encoders()
    res["trunks_eval_fwd_us"] = round(min(fwd), 1)
    ta, tb = [], []
    for _ in range(3):
        model.freeze_trunks()
        ta.append(timeit(lambda: step(args), n, warm=1))
        model.unfreeze_trunks()
        tb.append(timeit(lambda: step(imgs), n, warm=1))
    res["step_precomputed_maps_us"] = round(min(ta), 1)
    res["step_images_unfrozen_layer4_us"] = round(min(tb), 1)
    res["step_runs_us"] = {"maps": [round(t, 1) for t in ta], "images": [round(t, 1) for t in tb]}

    kern = {}
    for name, H, W, Cin, Cout, k, s, count in LAYER4:
        p = k // 2
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        x = torch.randn(B, H, W, Cin, device=DEV).to(torch.bfloat16)
        dy = torch.randn(B, OH, OW, Cout, device=DEV).to(torch.bfloat16)
        wT = torch.randn(Cin, k * k * Cout, device=DEV).to(torch.bfloat16)
        flop = 2.0 * B * OH * OW * Cout * Cin * k * k
        td = timeit(lambda: ops.conv_dgrad_bf16_nhwc(dy, wT, (H, W), k, s, p, mask=x), n, warm=1)
        tw = timeit(lambda: ops.conv_wgrad_bf16_nhwc(x, dy, k, s, p), n, warm=1)
        row = {"per_trunk": count, "GFLOP": round(flop / 1e9, 1)}
        for key, t, by in (("dgrad", td, dy.numel() * 2 + 2 * x.numel() * 2 + wT.numel() * 2),
                           ("wgrad", tw, dy.numel() * 2 + x.numel() * 2 + wT.numel() * 4)):
            row[key] = {"us": round(t, 1), "TF/s": round(flop / t / 1e6, 1), "pct_bf16_peak": round(100.0 * flop / t / 1e6 / (BF16_PEAK / 1e12), 2)}
            if k == 1:
                row[key].update({"alg_MB": round(by / 1e6, 1), "TB/s": round(by / t / 1e6, 2)})
        kern[name] = row
        del x, dy, wT
    res["kernels"] = kern
    fmap = torch.randn(B, 2048, 14, 14, device=DEV).clamp_min(0)
    t = timeit(lambda: ops.map_grad_relu_nhwc(fmap, fmap), n, warm=1)
    by = fmap.numel() * 10
    res["map_grad_entry"] = {"us": round(t, 1), "alg_MB": round(by / 1e6, 1), "TB/s": round(by / t / 1e6, 2)}
    w = torch.randn(512, 512, 3, 3, device=DEV)
    v = torch.rand(512, device=DEV) + 0.5
    dwp, dbp = torch.randn(512, 4608, device=DEV), torch.randn(512, device=DEV)
    res["bn_unfold_512x4608_us"] = round(timeit(lambda: ops.conv_bn_unfold(dwp, dbp, w, (v, v, v, 1e-5)), n, warm=1), 1)
    return res


def trunk_bn_case(n):
    from mgnns_amd import harness, synth
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    B = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else cfg.B
    res = {"case": "trunk_batchnorm_%s" % cfg.name, "B": B, "device": torch.cuda.get_device_name(0), "iters": n}

    def against_copy(fn, moved):
        """fn alternately with a copy_ that reads + writes `moved` bytes in all; three rounds, best of each."""
        src = torch.empty(moved // 2, dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)
        tk, tc = [], []
        for _ in range(3):
            tk.append(timeit(fn, n, warm=2))
            tc.append(timeit(lambda: dst.copy_(src), n, warm=2))
        return {"us": round(min(tk), 1), "copy_us": round(min(tc), 1), "ratio": round(min(tk) / min(tc), 3), "moved_MB": round(moved / 1e6, 1),
                "TB/s": round(moved / min(tk) / 1e6, 2), "runs_us": [round(t, 1) for t in tk], "copy_runs_us": [round(t, 1) for t in tc]}

    kern = {}
    for hw, C in ((14, 512), (14, 2048), (28, 512)):
        g = torch.Generator(device=DEV).manual_seed(hw + C)
        z = torch.randn(B, hw, hw, C, device=DEV, generator=g).to(torch.bfloat16)
        gy = torch.randn(B, hw, hw, C, device=DEV, generator=g).to(torch.bfloat16)
        gamma, beta = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        mean, rstd = ops.bn_stats_bf16_nhwc(z, 1e-5)
        nb = z.numel() * 2
        row = {"M": B * hw * hw, "C": C}
        row["bn_stats"] = against_copy(lambda: ops.bn_stats_bf16_nhwc(z, 1e-5, running=(rm, rv)), nb)
        row["bn_apply"] = against_copy(lambda: ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta), 2 * nb)
        row["bn_apply_residual"] = against_copy(lambda: ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta, residual=gy), 3 * nb)
        if C == 2048:
            row["bn_apply_residual_nchw_f32"] = against_copy(
                lambda: ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta, residual=gy, out_nchw_f32=True), 4 * nb)
        row["bn_backward"] = against_copy(lambda: ops.bn_backward_bf16_nhwc(gy, z, mean, rstd, gamma), 5 * nb)   # g, z read twice
        kern["%dx%dx%d" % (hw, hw, C)] = row
        del z, gy
    res["kernels"] = kern
    if "--kernels-only" in sys.argv:
        return res

    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV, trunks=True).train().freeze_text_encoders()
    imgs = list(harness.call_args(inp, DEV))
    G = torch.randn(B, cfg.NL, device=DEV)
    g = torch.Generator().manual_seed(1)
    for i in (3, 4):
        imgs[i] = torch.randn(B, 3, 448, 448, generator=g).to(DEV)

    def step():
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(model(*imgs), G)

    ta, tb = [], []
    for _ in range(3):
        model.unfreeze_trunks()
        ta.append(timeit(step, n, warm=1))
        model.unfreeze_trunks(batchnorm="batch")
        tb.append(timeit(step, n, warm=1))
    res["step_images_frozen_statistics_us"] = round(min(ta), 1)
    res["step_images_batch_statistics_us"] = round(min(tb), 1)
    res["step_ratio"] = round(min(tb) / min(ta), 3)
    res["step_runs_us"] = {"frozen": [round(t, 1) for t in ta], "batch": [round(t, 1) for t in tb]}
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    res["step_batch_peak_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    return res


def trunk_stem_case(n):
    from mgnns_amd import harness, synth
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    B = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else cfg.B
    res = {"case": "trunk_stem_%s" % cfg.name, "B": B, "device": torch.cuda.get_device_name(0), "iters": n}

    def alternately(fa, fb):
        ta, tb = [], []
        for _ in range(3):
            ta.append(timeit(fa, n, warm=2))
            tb.append(timeit(fb, n, warm=2))
        return ta, tb

    gen = torch.Generator(device=DEV).manual_seed(3)
    img = torch.randn(B, 3, 448, 448, device=DEV, generator=gen)
    w = torch.randn(64, 3, 7, 7, device=DEV, generator=gen) * 0.1
    v = torch.rand(64, device=DEV, generator=gen) + 0.5
    folded = ops.conv_fold_bn(w, None, (v, v - 1.0, v - 1.0, v, 1e-5), stem=True)
    raw = ops.conv_fold_bn(w, None, None, stem=True)
    y0 = ops.stem_conv7(img, *folded)
    g_y = torch.randn(B, 112, 112, 64, device=DEV, generator=gen).to(torch.bfloat16)
    g_y0 = ops.maxpool3x3s2_bwd_nhwc(y0, g_y, relu_mask=True)
    kern = {}
    # the pool's backward is a stream: y0 read, g_y read, g_y0 written
    moved = y0.numel() * 2 + g_y.numel() * 2 + y0.numel() * 2
    src = torch.empty(moved // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    tk, tc = alternately(lambda: ops.maxpool3x3s2_bwd_nhwc(y0, g_y, relu_mask=True), lambda: dst.copy_(src))
    kern["maxpool3x3s2_bwd_relu_mask"] = {"us": round(min(tk), 1), "copy_us": round(min(tc), 1), "ratio": round(min(tk) / min(tc), 3),
                                          "moved_MB": round(moved / 1e6, 1), "TB/s": round(moved / min(tk) / 1e6, 2),
                                          "runs_us": [round(t, 1) for t in tk], "copy_runs_us": [round(t, 1) for t in tc]}
    del src, dst
    # stem_wgrad against the one other pixel-contracted weight gradient, at layer4.0.conv2's geometry
    x4 = torch.randn(B, 28, 28, 512, device=DEV, generator=gen).to(torch.bfloat16)
    dy4 = torch.randn(B, 14, 14, 512, device=DEV, generator=gen).to(torch.bfloat16)
    flop_s = 2.0 * B * 224 * 224 * 64 * 147
    flop_4 = 2.0 * B * 14 * 14 * 512 * 512 * 9
    ts, t4 = alternately(lambda: ops.stem_wgrad(img, g_y0), lambda: ops.conv_wgrad_bf16_nhwc(x4, dy4, 3, 2, 1))
    by = img.numel() * 4 + g_y0.numel() * 2
    kern["stem_wgrad"] = {"us": round(min(ts), 1), "GFLOP": round(flop_s / 1e9, 1), "pct_bf16_peak": round(100.0 * flop_s / min(ts) / 1e6 / (BF16_PEAK / 1e12), 2),
                          "alg_MB": round(by / 1e6, 1), "TB/s": round(by / min(ts) / 1e6, 2),
                          "layer4_0_conv2_wgrad_us": round(min(t4), 1), "layer4_0_conv2_GFLOP": round(flop_4 / 1e9, 1),
                          "layer4_0_conv2_pct_bf16_peak": round(100.0 * flop_4 / min(t4) / 1e6 / (BF16_PEAK / 1e12), 2),
                          "ratio": round(min(ts) / min(t4), 3), "runs_us": [round(t, 1) for t in ts], "layer4_0_conv2_runs_us": [round(t, 1) for t in t4]}
    del x4, dy4
    tf, tr = alternately(lambda: ops.stem_conv7(img, *folded), lambda: ops.stem_conv7(img, *raw, raw=True))
    kern["stem_conv7"] = {"folded_us": round(min(tf), 1), "raw_us": round(min(tr), 1)}
    res["kernels"] = kern
    del img, y0, g_y, g_y0
    if "--kernels-only" in sys.argv:
        return res

    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV, trunks=True).train().freeze_text_encoders()
    imgs = list(harness.call_args(inp, DEV))
    G = torch.randn(B, cfg.NL, device=DEV)
    g = torch.Generator().manual_seed(1)
    for i in (3, 4):
        imgs[i] = torch.randn(B, 3, 448, 448, generator=g).to(DEV)

    def step():
        model.zero_grad(set_to_none=True)
        torch.autograd.backward(model(*imgs), G)

    for mode in ("frozen", "batch"):
        ta, tb = [], []
        for _ in range(3):
            model.unfreeze_trunks(4, batchnorm=mode)
            ta.append(timeit(step, n, warm=1))
            model.unfreeze_trunks(4, batchnorm=mode, stem=True)
            tb.append(timeit(step, n, warm=1))
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res["step_%s" % mode] = {"stages4_us": round(min(ta), 1), "stages4_stem_us": round(min(tb), 1), "difference_us": round(min(tb) - min(ta), 1),
                                 "ratio": round(min(tb) / min(ta), 3), "peak_GB_with_stem": round(torch.cuda.max_memory_allocated() / 1e9, 2),
                                 "runs_us": {"stages4": [round(t, 1) for t in ta], "stages4_stem": [round(t, 1) for t in tb]}}
    return res


def steps_only(k):
    from mgnns_amd import harness, synth
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=cfg.B, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV).train().freeze_text_encoders()
    model.set_train_bank_precision(bank_precision())
    args = list(harness.call_args(inp, DEV))
    for i in (3, 4):
        args[i] = args[i].detach().clone().requires_grad_(True)
    G = torch.randn(args[0].shape[0], cfg.NL, device=DEV)
    for _ in range(k):
        model.zero_grad(set_to_none=True)
        args[3].grad = args[4].grad = None
        torch.autograd.backward(model(*args), G)
    torch.cuda.synchronize()
    return {"case": "steps_%s" % cfg.name, "steps": k, "bank_precision": model.train_bank_precision}


def main():
    n = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    if not torch.cuda.is_available():
        raise SystemExit("bench_train: no GPU")
    if "--steps-only" in sys.argv:
        print(json.dumps(steps_only(int(sys.argv[sys.argv.index("--steps-only") + 1]))), flush=True)
        return
    if "--maps" in sys.argv:
        print(json.dumps(maps_case(n)), flush=True)
        return
    if "--trunk" in sys.argv and "--stem" in sys.argv:
        print(json.dumps(trunk_stem_case(n)), flush=True)
        return
    if "--trunk" in sys.argv and "--batchnorm" in sys.argv:
        mode = sys.argv[sys.argv.index("--batchnorm") + 1]
        if mode not in ("frozen", "batch"):
            raise SystemExit("bench_train: --batchnorm frozen|batch")
        print(json.dumps(trunk_case(n) if mode == "frozen" else trunk_bn_case(n)), flush=True)
        return
    if "--trunk" in sys.argv:
        print(json.dumps(trunk_case(n)), flush=True)
        return
    if "--text" in sys.argv:
        print(json.dumps(text_case(n)), flush=True)
        return
    if "--model-only" not in sys.argv:
        for B, H, L, masked in ((256, 4, 196, False), (256, 4, 100, True)):
            print(json.dumps(case(B, H, L, masked, n)), flush=True)
    print(json.dumps(model_case(n)), flush=True)


if __name__ == "__main__":
    main()
