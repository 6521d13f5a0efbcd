"""CPU emulation of the bf16-mode forward (Multi_GCN_Multihead_Att.set_precision('bf16')) -- TEST INFRASTRUCTURE ONLY.

restatement.forward is the fp32 network; this module is the same network with the HIP path's bf16 rounding points, in the
style of trunk_cpu.features_bf16_emulated: every value the kernels round to bf16 is rounded here (round to nearest even, the
kernels' bf16.hpp conversions, torch's .to(torch.bfloat16)), everything else is computed in fp64.  What remains between a
kernel and this emulation is fp32 summation order (~1e-6 relative) and the occasional intermediate that lands on the other side
of a bf16 rounding boundary, so the kernels can be held far tighter than against the fp32 answer.

Stages that stay fp32-class in bf16 mode come from restatement.py unchanged (model.set_precision docstring): the text GCN, the
label GCN (split-bf16 in the persistent launch), the label attention + its tail at model.label_tail_terms = 3 (split-bf16,
csrc/label_tail.hip), softmax, LayerNorms, residuals; the classifier head (fp32).

Rounding points (names = the keys of POINTS; `rounding` selects which are on, default all):
  image bank, csrc/imgbank_bf16.hip (stream form) and imgbank_bf16_pairs.hip (two workgroups per sample, up to half a chip of
  samples, imgbank_bf16.hip:446-448):
    imgbank_x    the feature maps, the GEMM's map operand          imgbank_bf16.hip:229, imgbank_bf16_pairs.hip:105-108
    imgbank_w    liner_img_* weights                               imgbank_bf16.hip:53-69 (pack_w_kernel)
    imgbank_out  the bank is stored as bf16 (fp32 accumulation + bias first; the max-pool reads the fp32 maps, exact)
                                                                   imgbank_bf16.hip:343-363, imgbank_bf16_pairs.hip:303-304
  BiLSTM with the bf16 recurrence, csrc/lstm.hip:
    lstm_x       layer inputs: embedding rows, layer-0 output rows for layer 1   lstm.hip:299-320 (gather cast; lstm_prep_kernel
                 :336 does the same), lstm.hip:619-622 (next_x = mg_bf16_rne_finite(h)); the folded layer-0 table is
                 bf16(emb) . bf16(W_ih0)^T + b_ih0 (lstm.hip:833-853), the same values
    lstm_wih     W_ih                                              lstm.hip:706, 788, 852 (mgnns_cast_pad_bf16)
    lstm_whh     W_hh                                              lstm.hip:410-420 (lstm_pack_whh_kernel)
    lstm_h       h as the A operand of W_hh . h at every step      lstm.hip:606 (s_h = mg_bf16x2(hh, 0)); gates, cell state and
                 the h row itself stay fp32 (lstm.hip:590-607)
    lstm_out     the bank's bf16 side copy RNE(h), read by the fusion attention  lstm.hip:165 (flush_rows)
  faithful attention, csrc/sq_mha_bf16.hip (16x16x32 form) and sq_mha32_bf16.hip (masked / packed form):
    attn_w       W_k, W_v                                          sq_mha_bf16.hip:43-70, sq_mha32_bf16.hip:61-83
                 (the bank is already bf16; qh stays fp32 in LDS, sq_mha_bf16.hip:502; K, V, scores, softmax, o fp32)
  folded attention, csrc/sq_mha_folded_bf16.hip:
    fold_u       the composed query rows u                         sq_mha_folded_bf16.hip:115-124
    fold_p       the probabilities, GEMM 2's A operand             sq_mha_folded_bf16.hip:189
    fold_c       the stored c = P X                                sq_mha_folded_bf16.hip:243
  layer tail, csrc/mha_tail_body.hpp tail_bf16_body<1> (mha_tail_bf16 terms=1) and <1, true> (mha_tail_c16):
    tail_w       fc (or the composed fc . blockdiag(W_v)), w_1, w_2, the next layer's w_qs (or composed query map)
                                                                   mha_tail.hip:267-283 (pack_w_split_kernel: hi = RNE(w))
    tail_o       o as fc's A operand (faithful; c arrives rounded)  mha_tail_body.hpp:196-205
    tail_y       y = LN1(.) as w_1's A operand                     mha_tail_body.hpp:92 (ln_rows_emit), called at :289
    tail_h       relu(w_1 y + b_1) as w_2's A operand              mha_tail_body.hpp:306
    tail_q       the layer output as the next projection's A operand  mha_tail_body.hpp:92 via :350; mha_tail.hip:352
                 (mha_proj_c16_kernel, the K-split forms' projection)
  label tail at terms=1 (model.label_tail_terms = 1, csrc/label_tail.hip label_tail_bf16_kernel<1, 1>), label_tail() below:
    weights (G, w_k, w_v, the composed linear_5 . fc, x_linear, w_q) and every product's A operand: pooled
    (label_tail.hip:425), x (:440-498), o (:558), the flatten buffer (:580), out (:605).

A layer's residuals, LayerNorms, scores, softmax, gates and cell state are never rounded.  The composed maps of the folded path
(fusion.composed_query_map / _tail_pack_folded) are built here in fp64 from the module's fp32 weights (the library builds them
with its fp32 GEMM, then rounds): one more source of rare rounding flips, never a systematic difference.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import restatement as R

POINTS = ("imgbank_x", "imgbank_w", "imgbank_out",
          "lstm_x", "lstm_wih", "lstm_whh", "lstm_h", "lstm_out",
          "attn_w", "fold_u", "fold_p", "fold_c",
          "tail_w", "tail_o", "tail_y", "tail_h", "tail_q")
FAITHFUL_ONLY = ("attn_w", "tail_o")
FOLDED_ONLY = ("fold_u", "fold_p", "fold_c")


def bf16_bits(x):
    """fp32 -> bf16 bit pattern (uint16), round to nearest even: the kernels' integer form (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    (csrc/bf16.hpp: mg_bf16_rne), with NaN kept a quiet NaN as v_cvt_pk_bf16_f32 and torch do."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(a)
    if nan.any():
        r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def bf16_round(t):
    """torch tensor (any float dtype) -> the same values rounded to bf16 through fp32 (the value a kernel holds in fp32 is
    what it rounds), returned as fp64."""
    a = t.detach().to(torch.float32).cpu().numpy()
    b = bf16_bits(a).astype(np.uint32) << 16
    return torch.from_numpy(b.view(np.float32).astype(np.float64)).reshape(t.shape)


class _Rounder:
    def __init__(self, rounding):
        rounding = POINTS if rounding is None else tuple(rounding)
        bad = set(rounding) - set(POINTS)
        if bad:
            raise ValueError("unknown rounding points %s (known: %s)" % (sorted(bad), ", ".join(POINTS)))
        self.on = frozenset(rounding)

    def __call__(self, point, t):
        return bf16_round(t) if point in self.on else t.double()


def _d(t):
    return torch.as_tensor(t).detach().double()


# ---------------------------------------------------------------------------------------------------------------------------
# image bank (csrc/imgbank_bf16.hip)
# ---------------------------------------------------------------------------------------------------------------------------
def img_bank(feat, weight, bias, rounding=None):
    """feat [B, 2048, P] (or [B, 2048, h, w]) -> (bank [B, P, N] fp64, the stored values; pooled [B, 2048] exact max)."""
    rd = _Rounder(rounding)
    f3 = _d(feat).flatten(2)                             # (an empty batch cannot be reshaped through -1)
    x = rd("imgbank_x", f3.permute(0, 2, 1))
    bank = rd("imgbank_out", x @ rd("imgbank_w", weight).t() + _d(bias))
    return bank, f3.max(dim=2).values


# ---------------------------------------------------------------------------------------------------------------------------
# BiLSTM, bf16 recurrence (csrc/lstm.hip lstm_rec_bf16_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def bilstm(p, text, lens, hidden=150, num_layers=2, rounding=None):
    """Embedding + packed bidirectional LSTM with the bf16 recurrence's rounding points.  p: the reference's state_dict names
    (embedding.weight, lstm.weight_ih_l0, ...).  -> (rows [B, T, 2 * hidden] fp64 -- what the kernel keeps in fp32 --, the bf16
    side copy of the last layer as fp64 values; zeros behind each sample's length)."""
    rd = _Rounder(rounding)
    text = torch.as_tensor(text).long()
    lens = torch.as_tensor(lens).long().cpu()
    B, T = text.shape
    Hd = hidden
    x = rd("lstm_x", _d(p["embedding.weight"])[text])
    ar = torch.arange(B)
    out = None
    for layer in range(num_layers):
        out = torch.zeros(B, T, 2 * Hd, dtype=torch.float64)
        for d, sfx in ((0, ""), (1, "_reverse")):
            k = "lstm.%%s_l%d%s" % (layer, sfx)
            wih, whh = rd("lstm_wih", p[k % "weight_ih"]), rd("lstm_whh", p[k % "weight_hh"])
            gx = x @ wih.t() + _d(p[k % "bias_ih"])                                       # [B, T, 4H]
            bhh = _d(p[k % "bias_hh"])
            h = torch.zeros(B, Hd, dtype=torch.float64)
            c = torch.zeros(B, Hd, dtype=torch.float64)
            for s in range(int(lens.max()) if B else 0):
                act = s < lens
                t = torch.full((B,), s, dtype=torch.long) if d == 0 else (lens - 1 - s).clamp(min=0)
                g = gx[ar, t] + bhh + rd("lstm_h", h) @ whh.t()
                i, f, gg, o = g.chunk(4, dim=1)
                c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
                h_new = torch.sigmoid(o) * torch.tanh(c_new)
                c = torch.where(act[:, None], c_new, c)
                h = torch.where(act[:, None], h_new, h)
                idx = act.nonzero().flatten()
                out[idx, t[idx], d * Hd:(d + 1) * Hd] = h_new[idx]
        if layer + 1 < num_layers:
            x = rd("lstm_x", out)
    return out, rd("lstm_out", out)


# ---------------------------------------------------------------------------------------------------------------------------
# fusion layers
# ---------------------------------------------------------------------------------------------------------------------------
def _ln(x, gamma, beta, eps=1e-6):
    """submodules.py:153-156 (unbiased std, eps added to the std), fp64."""
    mu = x.mean(-1, keepdim=True)
    sd = (x - mu).pow(2).sum(-1, keepdim=True).div(x.shape[-1] - 1).sqrt()
    return _d(gamma) * (x - mu) / (sd + eps) + _d(beta)


def composed_query_map(p, pre, n_head, d_kv):
    """fusion.composed_query_map in fp64: (M [H*D, D] = [W_k,h^T W_q,h]_h, c [H*D] = [W_k,h^T b_q,h]_h)."""
    a = pre + ".slf_attn."
    wq, bq, wk = _d(p[a + "w_qs.weight"]), _d(p[a + "w_qs.bias"]), _d(p[a + "w_ks.weight"])
    rows, bias = [], []
    for h in range(n_head):
        sl = slice(h * d_kv, (h + 1) * d_kv)
        rows.append(wk[sl].t() @ wq[sl])
        bias.append(wk[sl].t() @ bq[sl])
    return torch.cat(rows, 0), torch.cat(bias)


def composed_output_map(p, pre, n_head, d_kv):
    """fusion._tail_pack_folded in fp64: (N [D, H*D] = [fc_h W_v,h]_h, fc b_v + b_fc)."""
    a = pre + ".slf_attn."
    fc, wv = _d(p[a + "fc.weight"]), _d(p[a + "w_vs.weight"])
    n = torch.cat([fc[:, h * d_kv:(h + 1) * d_kv] @ wv[h * d_kv:(h + 1) * d_kv] for h in range(n_head)], 1)
    return n, fc @ _d(p[a + "w_vs.bias"]) + _d(p[a + "fc.bias"])


def layer_tail(p, pre, o, q, fc_w, fc_b, next_w=None, next_b=None, rounding=None, o_point="tail_o", eps=1e-6):
    """tail_bf16_body<1>: out = LN2(w_2 relu(w_1 y + b_1) + b_2 + y), y = LN1(fc o + fc_b + q); next = w_next out + b_next.
    fc_w / next_w: the plain fc / w_qs (faithful) or the composed maps (folded).  o: [B, K]; it is rounded as `o_point`
    (None: o arrives as bf16 values already, the c16 form).  -> (out, next or None), fp64."""
    rd = _Rounder(rounding)
    a, f = pre + ".slf_attn.", pre + ".pos_ffn."
    o = _d(o)
    oa = o if o_point is None else rd(o_point, o)
    y = _ln(oa @ rd("tail_w", fc_w).t() + _d(fc_b) + _d(q), p[a + "layer_norm.gamma"], p[a + "layer_norm.beta"], eps)
    w1, w2 = p[f + "w_1.weight"].squeeze(-1), p[f + "w_2.weight"].squeeze(-1)
    h = torch.relu(rd("tail_y", y) @ rd("tail_w", w1).t() + _d(p[f + "w_1.bias"]))
    out = _ln(rd("tail_h", h) @ rd("tail_w", w2).t() + _d(p[f + "w_2.bias"]) + y,
              p[f + "layer_norm.gamma"], p[f + "layer_norm.beta"], eps)
    if next_w is None:
        return out, None
    return out, rd("tail_q", out) @ rd("tail_w", next_w).t() + _d(next_b)


def faithful_core(p, pre, qh, bank, mask, n_head, d_kv, rounding=None):
    """sq_mha_core_bf16 on the bf16 bank values `bank` [B, L, D]: K / V = bank . W^T + b with W_k / W_v rounded, the rest fp64.
    -> (o [B, H*dk], probabilities [B, H, L])."""
    rd = _Rounder(rounding)
    a = pre + ".slf_attn."
    B, L, _ = bank.shape
    bank = _d(bank)
    kh = (bank @ rd("attn_w", p[a + "w_ks.weight"]).t() + _d(p[a + "w_ks.bias"])).view(B, L, n_head, d_kv)
    vh = (bank @ rd("attn_w", p[a + "w_vs.weight"]).t() + _d(p[a + "w_vs.bias"])).view(B, L, n_head, d_kv)
    s = torch.einsum("bhd,blhd->bhl", _d(qh).view(B, n_head, d_kv), kh) / math.sqrt(d_kv)
    if mask is not None:
        s = s.masked_fill(_d(mask)[:, None, :] == 0, float("-inf"))
    pa = torch.softmax(s, dim=2)
    return torch.einsum("bhl,blhd->bhd", pa, vh).reshape(B, n_head * d_kv), pa


def folded_core(u, bank, mask, n_head, d_kv, rounding=None):
    """sq_mha_folded_bf16: u [B, H*D] composed query rows, bank [B, L, D] bf16 values -> (c [B, H*D] as stored, probabilities)."""
    rd = _Rounder(rounding)
    B, L, D = bank.shape
    bank = _d(bank)
    ur = rd("fold_u", u).view(B, n_head, D)
    s = torch.einsum("bhf,blf->bhl", ur, bank) / math.sqrt(d_kv)
    if mask is not None:
        s = s.masked_fill(_d(mask)[:, None, :] == 0, float("-inf"))
    pa = torch.softmax(s, dim=2)
    c = rd("fold_c", torch.einsum("bhl,blf->bhf", rd("fold_p", pa), bank))
    return c.reshape(B, n_head * D), pa


def stack(p, name, q, first, bank, mask, n_head, d_kv, stack_num, attention, rounding=None):
    """fusion.run_stack in bf16 mode.  first: the first layer's projected query (faithful: w_qs(q) + b; folded: the composed
    rows u), as its producer made it.  -> the stack's output [B, 300] fp64."""
    q = _d(q)
    nxt = _d(first)
    for i in range(stack_num):
        pre = "%s.%d" % (name, i)
        last = i + 1 == stack_num
        npre = "%s.%d" % (name, i + 1)
        if attention == "folded":
            c, _ = folded_core(nxt, bank, mask, n_head, d_kv, rounding)
            n, nb = composed_output_map(p, pre, n_head, d_kv)
            nw, nbias = (None, None) if last else composed_query_map(p, npre, n_head, d_kv)
            q, nxt = layer_tail(p, pre, c, q, n, nb, nw, nbias, rounding, o_point=None)
        else:
            o, _ = faithful_core(p, pre, nxt, bank, mask, n_head, d_kv, rounding)
            a = pre + ".slf_attn."
            nw, nbias = (None, None) if last else (p[npre + ".slf_attn.w_qs.weight"], p[npre + ".slf_attn.w_qs.bias"])
            q, nxt = layer_tail(p, pre, o, q, p[a + "fc.weight"], p[a + "fc.bias"], nw, nbias, rounding)
    return q


def first_query(p, name, q, n_head, d_kv, attention):
    """The first layer's query as the model's fp32-class producers make it (first_query / label_tail_bf16 at terms=3)."""
    if attention == "folded":
        m, c = composed_query_map(p, name + ".0", n_head, d_kv)
        return _d(q) @ m.t() + c
    a = name + ".0.slf_attn."
    return _d(q) @ _d(p[a + "w_qs.weight"]).t() + _d(p[a + "w_qs.bias"])


# ---------------------------------------------------------------------------------------------------------------------------
# label tail at terms=1 (csrc/label_tail.hip label_tail_bf16_kernel<1, 1>)
# ---------------------------------------------------------------------------------------------------------------------------
def label_tail(p, chan, pooled, G, Q, n_heads=5, next_w=None, next_b=None, terms=1):
    """The fused channel tail: x = pooled . G^T, K / V, the element-wise label attention, the composed linear_5 . fc, x_linear,
    the next stack's query.  terms=1 rounds every product's operands (fp32 accumulation); terms=3 is fp32-class: no rounding.
    Q: the projected label query [NLQ, hid] (fp32, not rounded: label_tail.hip:546).  -> (out [B, n_out], next or None)."""
    rd = (lambda t: bf16_round(t)) if terms == 1 else _d
    a = chan + "_attention."
    x = rd(pooled) @ rd(G).t()
    xr = rd(x)
    K = xr @ rd(p[a + "w_k.weight"]).t() + _d(p[a + "w_k.bias"])
    V = xr @ rd(p[a + "w_v.weight"]).t() + _d(p[a + "w_v.bias"])
    NLQ, hid = Q.shape
    dh = hid // n_heads
    B = x.shape[0]
    e = (_d(Q)[None] * K[:, None]).view(B, NLQ, n_heads, dh) / math.sqrt(dh)
    o = (torch.softmax(e, dim=-1) * V.view(B, 1, n_heads, dh)).reshape(B, NLQ, hid)
    w5, wfc = _d(p[chan + "_linear_5.weight"]), _d(p[a + "fc.weight"])
    wc, bc = w5 @ wfc, w5 @ _d(p[a + "fc.bias"]) + _d(p[chan + "_linear_5.bias"])
    y = rd(rd(o) @ rd(wc).t() + bc).reshape(B, NLQ * wc.shape[0])           # (an empty batch cannot be reshaped through -1)
    out = y @ rd(p[chan + "_x_linear.weight"]).t() + _d(p[chan + "_x_linear.bias"])
    if next_w is None:
        return out, None
    return out, rd(out) @ rd(next_w).t() + _d(next_b)


# ---------------------------------------------------------------------------------------------------------------------------
# whole forward
# ---------------------------------------------------------------------------------------------------------------------------
def forward(p, inputs, pmi, n_head, d_kv, stack_num, ngram, label_query=None, attention="faithful", rounding=None,
            hidden=150, num_layers=2, return_parts=False):
    """Multi_GCN_Multihead_Att.forward in bf16 mode (identity trunks, model.label_tail_terms = 3, the bf16 LSTM recurrence).
    Arguments as restatement.forward; attention 'faithful' | 'folded'; rounding: the POINTS switched on (None: all; () gives
    the fp32 network in fp64 arithmetic).  -> logits [B, NL] fp64 (, parts)."""
    if attention not in ("faithful", "folded"):
        raise ValueError("attention must be 'faithful' or 'folded'")
    with torch.no_grad():
        text, lens, mask = inputs["text"], inputs["text_lens"], inputs["text_mask"]
        lq = inputs["label_query"] if label_query is None else label_query
        lq = torch.as_tensor(lq)
        parts = {}
        text_feature = _d(R.text_gcn(np.asarray(text), p["text_features.node_hidden.weight"],
                                     p["text_features.seq_edge_w.weight"], pmi, ngram))
        tb, tb16 = bilstm(p, text, lens, hidden, num_layers, rounding)
        bank, att = {}, {}
        for chan, a_key in (("object", "object_A"), ("place", "place_A")):
            feat = torch.as_tensor(inputs[chan + "_feature"])
            bank[chan], pooled = img_bank(feat, p["liner_img_%s.weight" % chan], p["liner_img_%s.bias" % chan], rounding)
            G = R.image_gcn(p[a_key], torch.as_tensor(inputs[chan + "_inp"])[0], p["gc1.weight"], p["gc2.weight"])
            x = pooled.float() @ G.t()
            y = R.label_attention(p, chan + "_attention", lq, x)
            att[chan] = _d(R.label_attention_tail(p, chan, y))
            parts[chan + "_x"] = _d(x)
            parts[chan + "_att"] = att[chan]
        m = _d(mask)
        outs = {}
        for name, stack_name, qsrc, bk, mk in (
                ("iot", "img_object_text_multi_head_att", att["object"], tb16, m),
                ("ipt", "img_place_text_multi_head_att", att["place"], tb16, m),
                ("tio", "text_img_object_multi_head_att", text_feature, bank["object"], None),
                ("tip", "text_img_place_multi_head_att", text_feature, bank["place"], None)):
            first = first_query(p, stack_name, qsrc, n_head, d_kv, attention)
            outs[name] = stack(p, stack_name, qsrc, first, bk, mk, n_head, d_kv, stack_num, attention, rounding)
        multi = torch.cat([outs["tio"], outs["tip"], outs["iot"], outs["ipt"]], dim=1)
        h = multi @ _d(p["multi_linear_1.weight"]).t() + _d(p["multi_linear_1.bias"])
        logits = h @ _d(p["multi_linear_2.weight"]).t() + _d(p["multi_linear_2.bias"])
        if return_parts:
            parts.update(text_feature=text_feature, text_bank=tb, text_bank_bf16=tb16, bank_object=bank["object"],
                         bank_place=bank["place"], multi=multi, **outs)
            return logits, parts
        return logits
