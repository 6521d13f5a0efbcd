"""Plain references of the forward operators, one function per kernel entry point, restated from the formulas of
oracle/restatement.py.  Every function computes in the dtype of its inputs: the GPU edge tests (tests/test_forward_edges_gpu.py)
feed float64, tests/test_forward_ref_cpu.py pins each function to the committed goldens, and the same function evaluated in float32
gives the rounding error a tolerance may be derived from.  No cleverness: torch ops in the order the formulas are written."""
import math

import torch


def linear(x, w, b=None, act=0, residual=None):
    """act(x @ w.T + b) (+ residual); act: 0 none | 1 ReLU | 2 LeakyReLU(0.2)."""
    y = x @ w.t()
    if b is not None:
        y = y + b
    if act == 1:
        y = torch.relu(y)
    elif act == 2:
        y = torch.nn.functional.leaky_relu(y, 0.2)
    return y if residual is None else y + residual


def layer_norm(x, gamma, beta, eps=1e-6):
    """Unbiased std, eps added to the std (restatement.layer_norm)."""
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, keepdim=True)
    return gamma * (x - mean) / (std + eps) + beta


def sq_mha_core(qh, bank, mask, n_head, d_kv, wk, bk, wv, bv):
    """qh [B, H*dk] (projected query), bank [B, L, D], mask [B, L] (0 = pad) or None -> (o [B, H*dk], attn [H*B, 1, L] head-major).
    A sample without a live position has NaN probabilities, like the reference's softmax over -inf."""
    B, L, _ = bank.shape
    H, dk = n_head, d_kv
    kh = linear(bank, wk, bk).view(B, L, H, dk)
    vh = linear(bank, wv, bv).view(B, L, H, dk)
    s = torch.einsum("bhd,blhd->bhl", qh.view(B, H, dk), kh) / math.sqrt(dk)
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, float("-inf"))
    p = torch.softmax(s, dim=2)
    o = torch.einsum("bhl,blhd->bhd", p, vh).reshape(B, H * dk)
    return o, p.permute(1, 0, 2).reshape(H * B, 1, L)


def mha_tail(o, q, w, eps=1e-6, next_q=None):
    """fc + residual + LN + FFN + residual + LN behind the attention core (restatement.mha_layer).  w: dict with fc_w, fc_b, g1, be1,
    w1, b1, w2, b2, g2, be2; next_q = (weight, bias) of the next layer's w_qs -> (out [B, D], qh_next or None)."""
    y = layer_norm(linear(o, w["fc_w"], w["fc_b"]) + q, w["g1"], w["be1"], eps)
    z = linear(torch.relu(linear(y, w["w1"], w["b1"])), w["w2"], w["b2"])
    out = layer_norm(z + y, w["g2"], w["be2"], eps)
    return out, (None if next_q is None else linear(out, next_q[0], next_q[1]))


def head_diff(o):
    """o [B, H, dv] -> [B]: mean over the ordered head pairs i != j of cos^2(o_i, o_j); F.normalize clamps the norm at 1e-12."""
    x = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    c2 = torch.bmm(x, x.permute(0, 2, 1)) ** 2
    H = o.shape[1]
    idx = torch.arange(H)
    c2[:, idx, idx] = 0
    return c2.sum(dim=[1, 2]) / (H * (H - 1))


def classifier_head(feats, w, b):
    """cat(feats, dim=1) @ w.T + b."""
    return linear(torch.cat(list(feats), dim=1), w, b)


def imgbank_pool(feat, w, bias):
    """feat [B, K, P] -> (bank [B, P, N] = feat[b, :, p] . w.T + bias, pooled [B, K] = max over p)."""
    return linear(feat.permute(0, 2, 1), w, bias), feat.max(dim=2).values


def label_attn_core(Q, K, V, n_heads, mask=None):
    """Q [NLQ, hid], K = V [B, hid] -> x [B, NLQ, hid]: softmax over the dh features of each head of Q * K / sqrt(dh), times V
    (restatement.label_attention between its projections).  mask broadcasts against [B, NLQ, heads, dh]; zeros get -1e10."""
    NLQ, hid = Q.shape
    B = K.shape[0]
    dh = hid // n_heads
    e = Q.view(1, NLQ, n_heads, dh) * K.view(B, 1, n_heads, dh) / math.sqrt(dh)
    if mask is not None:
        e = e.masked_fill(mask == 0, -1e10)
    return (torch.softmax(e, dim=-1) * V.view(B, 1, n_heads, dh)).reshape(B, NLQ, hid)


def softmax_argmax(logits):
    """-> (softmax over dim 1, first arg-max of each row)."""
    p = torch.softmax(logits, dim=1)
    return p, p.argmax(dim=1)


def confusion(target, pred, n_labels):
    """Integer confusion matrix, rows = target, columns = prediction."""
    c = torch.zeros(n_labels, n_labels, dtype=torch.int64)
    for t, q in zip(target.tolist(), pred.tolist()):
        c[t, q] += 1
    return c


def gen_adj(A):
    """adj[i, j] = A[j, i] d[i] d[j] with d = rowsum(A)^-1/2: the (A D)^T D of restatement.gen_adj, element by element."""
    d = torch.pow(A.sum(1), -0.5)
    return (A * d[None, :]).t() * d[None, :]


def label_gcn(A, inp, w1, w2, query=None):
    """One channel's label GCN (restatement.image_gcn): adj = gen_adj(A), G = adj @ (LeakyReLU_0.2(adj @ (inp @ w1)) @ w2) with the
    GraphConvolution weights in their [in, out] layout.  query = (label_query, w_q.weight, w_q.bias or None) adds
    Q = w_q(label_query).  -> (G [C, N2], Q or None)."""
    adj = gen_adj(A)
    x1 = torch.nn.functional.leaky_relu(adj @ (inp @ w1), 0.2)
    G = adj @ (x1 @ w2)
    return G, (None if query is None else linear(query[0], query[1], query[2]))


def label_tail(pooled, G, Q, n_heads, w, next_q=None):
    """The channel tail behind the label GCN, map by map as the model runs it: x = max over parts(pooled) . G^T, K / V, the element-wise
    label attention, fc, linear_5, flatten, x_linear, and the next stack's query.  pooled [B, parts, K]; Q [NLQ, hid] the projected label
    query; w: dict with wk, bk, wv, bv, wfc, bfc, w5, b5, wxl, bxl; next_q = (weight, bias or None).  -> (out [B, n_out], next or None).
    The float64 reference of the fused kernels is oracle/bf16_path.label_tail (tests/test_label_edges_cpu.py pins this one to it); this
    one follows the dtype of its inputs, so its float32 evaluation gives the rounding error a bound may be derived from."""
    x = pooled.max(dim=1).values @ G.t()
    o = label_attn_core(Q, linear(x, w["wk"], w["bk"]), linear(x, w["wv"], w["bv"]), n_heads)
    y = linear(linear(o, w["wfc"], w["bfc"]), w["w5"], w["b5"]).reshape(x.shape[0], Q.shape[0] * w["w5"].shape[0])
    out = linear(y, w["wxl"], w["bxl"])
    return out, (None if next_q is None else linear(out, next_q[0], next_q[1]))


def embedding(idx, table):
    return table[idx]


def text_memory_bank(emb, weights, tok, lens, hidden):
    """Embedding -> 2-layer BiLSTM over each sample's first lens[b] tokens -> [B, T, 2*hidden], zeros behind each length
    (restatement.text_memory_bank, written out so that it runs in float64 and takes empty samples).  weights: per (layer,
    direction) the tuple (w_ih, w_hh, b_ih, b_hh), gates in torch's order i, f, g, o."""
    B, T = tok.shape
    x = emb[tok]
    live = (torch.arange(T)[None, :] < lens[:, None]).to(x.dtype)[:, :, None]
    for layer in range(len(weights) // 2):
        out = []
        for direction in range(2):
            w_ih, w_hh, b_ih, b_hh = weights[2 * layer + direction]
            h = x.new_zeros(B, hidden)
            c = x.new_zeros(B, hidden)
            y = x.new_zeros(B, T, hidden)
            for t in (range(T) if direction == 0 else range(T - 1, -1, -1)):
                i, f, g, o = (x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=1)
                c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h2 = torch.sigmoid(o) * torch.tanh(c2)
                m = live[:, t]                                # a sample's state moves only inside its own length
                c = m * c2 + (1 - m) * c
                h = m * h2 + (1 - m) * h
                y[:, t] = m * h2
            out.append(y)
        x = torch.cat(out, dim=2)
    return x
