"""Training mode of the fusion layers: autograd Functions over the HIP kernels of csrc/mha_train.hip.

fusion.MultiHeadAttention and fusion.PositionwiseFeedForward run these when `self.training` is set, with the reference's
semantics (submodules.py:15-139): dropout on the attention probabilities (`attn_dropout`, the reference's
`attention.dropout`), after `fc` and after `w_2` (the layers' own `dropout`), and the custom LayerNorm (unbiased std, eps added
to the std).  Everything is fp32.  The masks are drawn from a counter-based hash of a seed the module draws from torch's default
generator per training forward (kept as `last_dropout_seed`), so torch.manual_seed reproduces a run bit for bit.

The rest of the model trains through the Functions below the fusion layers' (csrc/model_train.hip): the image memory banks
(their weight gradient is the backward's hot path), the label GCN (propagated back with the transposed adjacency), the label
attention with dropout on its probabilities, the channel tails and the classifier with its dropout.  The text encoders train
through their own Functions below once unfrozen.  Feature maps that require a gradient get one (ImgBankFunction,
csrc/map_grad.hip), so a torch trunk in front of the model fine-tunes through torch's own backward; the trunks of
mgnns_amd.trunk fine-tune their trailing bottleneck stages through TrunkStageFunction, at the end of this file: in mode 'frozen'
with frozen BatchNorm statistics (csrc/conv_train.hip, model.unfreeze_trunks()), in mode 'batch' with the statistics of the
batch -- the reference's semantics -- (csrc/bn_train.hip, model.unfreeze_trunks(batchnorm='batch')).  With all four stages
trainable the stem -- conv1, bn1, ReLU, max-pool -- trains too, through TrunkStemFunction in the same two modes
(csrc/stem_train.hip, model.unfreeze_trunks(4, stem=True)): nothing of a trunk is then left frozen.  Both walk a bottleneck once
forward (trunk.run_block) and once backward; the modes differ in one step per layer (_stage_step, _layer_backward), and what a
forward keeps for its backward is one named record (save_record / saved_record).
"""
from types import SimpleNamespace

import torch

from . import ops, trunk


def draw_seed():
    """One 63-bit seed from torch's default (CPU) generator: torch.manual_seed makes the training forwards reproducible."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


class MHATrainFunction(torch.autograd.Function):
    """y1 = LN1(dropout(fc(o)) + q),  o = the folded attention core with attention dropout (returns (y1, attn); attn is the
    probabilities after dropout, [H*B, 1, L], and carries no gradient)."""

    @staticmethod
    def forward(ctx, q, bank, mask, seed, rate_attn, rate_fc, eps, n_head, d_kv, wq, bq, wk, bk, wv, bv, wfc, bfc, g1, be1):
        qh = ops.linear(q, wq, bq)
        o, attn, core = ops.mha_attn_train(qh, bank, mask, n_head, d_kv, wk, wv, bv, seed, rate_attn)
        f = ops.linear(o, wfc, bfc)
        y1, ln = ops.dropout_residual_layernorm(f, q, g1, be1, eps, seed, ops.DROP_FC, rate_fc)
        ctx.core, ctx.ln = core, ln
        ctx.save_for_backward(q, bank, mask, qh, o, wq, wk, bk, wv, bv, wfc, g1)
        ctx.mark_non_differentiable(attn)
        return y1, attn

    @staticmethod
    def backward(ctx, dy1, _dattn):
        q, bank, mask, qh, o, wq, wk, bk, wv, bv, wfc, g1 = ctx.saved_tensors
        dres, df, dg1, dbe1 = ops.dropout_residual_layernorm_backward(dy1.contiguous(), g1, ctx.ln)
        dwfc, dbfc = ops.wgrad(df, o)
        dO = ops.matmul(df, wfc)
        dqh, dwk, dwv, dbv, dbank = ops.mha_attn_train_backward(dO, qh, bank, mask, wk, wv, bv, ctx.core,
                                                                want_dbank=ctx.needs_input_grad[1])
        dwq, dbq = ops.wgrad(dqh, q)
        dq = ops.train_eltwise(ops.ELT_ADD, dres, ops.matmul(dqh, wq))
        return (dq, dbank, None, None, None, None, None, None, None, dwq, dbq, dwk, torch.zeros_like(bk), dwv, dbv, dwfc, dbfc,
                dg1, dbe1)


class FFNTrainFunction(torch.autograd.Function):
    """out = LN2(dropout(w_2 relu(w_1 x + b_1) + b_2) + x) over rows x [N, D]; w_1 / w_2 as [out, in] views of the Conv1d
    weights."""

    @staticmethod
    def forward(ctx, x, seed, rate, eps, w1, b1, w2, b2, g2, be2):
        h = ops.linear(x, w1, b1, act=ops.ACT_RELU)
        f = ops.linear(h, w2, b2)
        out, ln = ops.dropout_residual_layernorm(f, x, g2, be2, eps, seed, ops.DROP_FFN, rate)
        ctx.ln = ln
        ctx.save_for_backward(x, h, w1, w2, g2)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, h, w1, w2, g2 = ctx.saved_tensors
        dres, df, dg2, dbe2 = ops.dropout_residual_layernorm_backward(dout.contiguous(), g2, ctx.ln)
        dw2, db2 = ops.wgrad(df, h)
        dh = ops.train_eltwise(ops.ELT_RELU_BWD, ops.matmul(df, w2), h)
        dw1, db1 = ops.wgrad(dh, x)
        dx = ops.train_eltwise(ops.ELT_ADD, dres, ops.matmul(dh, w1))
        return dx, None, None, None, dw1, db1, dw2, db2, dg2, dbe2


def _refuse_unsupported(mha):
    if mha.precision != 'fp32':
        raise NotImplementedError("training mode runs in fp32 only (precision=%r): set_precision('fp32') before .train()"
                                  % mha.precision)
    if mha.is_regu:
        raise NotImplementedError("training mode does not implement the is_regu head-difference gradient")


def mha_train_forward(mha, q, bank, mask):
    """MultiHeadAttention.forward in training mode: q [B, 1, d]; bank: the fp32 memory bank tensor [B, L, d] (a MemoryBank's
    .f32); mask [B, 1, L] or None -> (out [B, 1, d], attn [H*B, 1, L])."""
    _refuse_unsupported(mha)
    B = q.shape[0]
    if not q.is_cuda:
        raise RuntimeError("q is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % q.device)
    q2 = q.reshape(B, -1).contiguous()
    x = bank.contiguous()
    m2 = None if mask is None else mask.reshape(B, -1).float().contiguous()
    seed = draw_seed()
    mha.last_dropout_seed = seed
    y, attn = MHATrainFunction.apply(q2, x, m2, seed, mha.attn_dropout.p, mha.dropout.p, mha.layer_norm.eps, mha.n_head,
                                     mha.d_k, mha.w_qs.weight, mha.w_qs.bias, mha.w_ks.weight, mha.w_ks.bias, mha.w_vs.weight,
                                     mha.w_vs.bias, mha.fc.weight, mha.fc.bias, mha.layer_norm.gamma, mha.layer_norm.beta)
    return y.view(B, 1, -1), attn


def ffn_train_forward(ffn, x):
    """PositionwiseFeedForward.forward in training mode: x [..., d] -> [..., d]."""
    if not x.is_cuda:
        raise RuntimeError("x is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % x.device)
    shp = x.shape
    x2 = x.reshape(-1, shp[-1]).contiguous()
    seed = draw_seed()
    ffn.last_dropout_seed = seed
    w1 = ffn.w_1.weight.view(ffn.w_1.out_channels, ffn.w_1.in_channels)
    w2 = ffn.w_2.weight.view(ffn.w_2.out_channels, ffn.w_2.in_channels)
    out = FFNTrainFunction.apply(x2, seed, ffn.dropout.p, ffn.layer_norm.eps, w1, ffn.w_1.bias, w2, ffn.w_2.bias,
                                 ffn.layer_norm.gamma, ffn.layer_norm.beta)
    return out.view(shp)


# ---- the model around the fusion stacks (MODEL:431-567) ----------------------------------------------------------------------
class LinearFunction(torch.autograd.Function):
    """y = x W^T + b over rows x [M, K] (b may be None); backward dx = dy W, (dW, db) = wgrad(dy, x)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return ops.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = ops.matmul(dy, w) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = ops.wgrad(dy, x, bias=ctx.has_bias)
        return dx, dw, db


def linear(x, lin_or_w, b=None):
    """LinearFunction over the last axis of x: an nn.Linear, or a weight [N, K] and bias."""
    if isinstance(lin_or_w, torch.nn.Linear):
        lin_or_w, b = lin_or_w.weight, lin_or_w.bias
    shp = x.shape
    y = LinearFunction.apply(x.reshape(-1, shp[-1]).contiguous(), lin_or_w, b)
    return y.view(*shp[:-1], y.shape[-1])


class CrossEntropyFunction(torch.autograd.Function):
    """loss = F.cross_entropy(logits, target) (mean over the targets that are not -100), 0-d fp32; forward and gradient in one launch
    (ops.ce_loss, fp64 inside), backward = the saved dlogits times the upstream gradient."""

    @staticmethod
    def forward(ctx, logits, target):
        loss, dlogits = ops.ce_loss(logits, target)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dlogits, = ctx.saved_tensors
        return dlogits * dloss, None


def cross_entropy(logits, target):
    """nn.CrossEntropyLoss()(logits, target) for logits [B, NL] fp32 (NL <= ops.CE_MAX_NL) and class indices target [B] int64."""
    return CrossEntropyFunction.apply(logits.contiguous(), target.contiguous())


BANK_PRECISIONS = ('fp32', 'bf16x3')


def split_forward_fits(K, P, N):
    """The shapes the split-bf16 bank kernel (ops.imgbank_pool_split) takes; any other map runs the fp32 forward."""
    return K % 64 == 0 and P % 4 == 0 and 0 < P <= 224 and 0 < N <= 304


class ImgBankFunction(torch.autograd.Function):
    """(bank [B, P, N], pooled [B, K]) = the fp32 memory bank and max-pool of a feature map f [B, K, P] (ops.imgbank_pool; wt =
    the bank kernel's transposed weight).  The weight and bias get gradients from ops.imgbank_wgrad (skipped when neither requires
    one).  A map that requires a gradient gets dX = W^T dbank + the max-pool's gradient at each row's first maximum
    (ops.imgbank_dgrad over ops.map_argmax of the saved map, both in the backward only); either incoming gradient may be absent.
    For a map that requires none, pooled is a constant and neither kernel is launched.
    Two optional trailing arguments: mode ('fp32', the default, or 'bf16x3') and w_split (ops.pack_weight_bf16_split of the
    weight, or None).  'bf16x3' runs the three products on the bf16 matrix pipe at fp32-class accuracy: both gradients through
    the split-bf16 kernels at every shape, the forward through ops.imgbank_pool_split where w_split is given and the shape fits
    (split_forward_fits; wt may then be None), else through the fp32 kernel.  pooled is exact in either mode."""

    @staticmethod
    def forward(ctx, f, weight, bias, wt, *mode):
        split = bool(mode) and mode[0] == 'bf16x3'
        if mode and mode[0] not in BANK_PRECISIONS:
            raise ValueError("ImgBankFunction: mode must be one of %s, got %r" % (BANK_PRECISIONS, mode[0]))
        w_split = mode[1] if len(mode) > 1 else None
        N = weight.shape[0]
        if split and w_split is not None and split_forward_fits(f.shape[1], f.shape[2], N):
            bank, halves = ops.imgbank_pool_split(f, w_split, bias.detach(), N, want_pool=True, want_f32=True)
            pooled = halves.amax(dim=1)            # the exact maxima of the two region halves
        else:
            bank, pooled = ops.imgbank_pool(f, wt, bias.detach(), N)
        ctx.split, ctx.extra = split, len(mode)
        ctx.map_grad = ctx.needs_input_grad[0]
        if ctx.map_grad:
            ctx.save_for_backward(f, weight)
            ctx.set_materialize_grads(False)       # an unused bank must not cost a zero-filled dbank
        else:
            ctx.save_for_backward(f)
            ctx.mark_non_differentiable(pooled)
        return bank, pooled

    @staticmethod
    def backward(ctx, dbank, dpooled):
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        rest = (None,) * (1 + ctx.extra)
        sp = (True,) if ctx.split else ()          # (positional: fp32 mode makes today's calls, argument for argument)
        if not ctx.map_grad:
            if not want_w:
                return (None, None, None) + rest
            f, = ctx.saved_tensors
            dw, db = ops.imgbank_wgrad(f, dbank.contiguous(), *sp)
            return (None, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None) + rest
        f, weight = ctx.saved_tensors
        dbank = None if dbank is None else dbank.contiguous()
        dw = db = dx = None
        if want_w and dbank is not None:
            dw, db = ops.imgbank_wgrad(f, dbank, *sp)
        kw = {"split": True} if ctx.split else {}
        if dpooled is not None:
            dx = ops.imgbank_dgrad(dbank, weight, dpooled.contiguous(), ops.map_argmax(f), positions=f.shape[2], **kw)
        elif dbank is not None:
            dx = ops.imgbank_dgrad(dbank, weight, **kw)
        return (dx, dw if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None) + rest


class GCNFunction(torch.autograd.Function):
    """y = act(adj (x W)) with adj as CSR (csr) and its transpose (csr_t); backward dh = act'(dy), ds = adj^T dh,
    dW = x^T ds, dx = ds W^T.  act: ops.ACT_NONE or ops.ACT_LRELU2 (the label GCN's LeakyReLU(0.2), MODEL:462)."""

    @staticmethod
    def forward(ctx, x, w, csr, csr_t, act):
        y = ops.spmm_csr(csr, ops.matmul(x, w), act=act)
        ctx.csr_t, ctx.act = csr_t, act
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dh = dy.contiguous()
        if ctx.act == ops.ACT_LRELU2:
            dh = ops.train_eltwise(ops.ELT_LRELU2_BWD, dh, y)
        elif ctx.act != ops.ACT_NONE:
            raise NotImplementedError("GCNFunction: no backward for activation %d" % ctx.act)
        ds = ops.spmm_csr(ctx.csr_t, dh)
        dw = ops.wgrad(x, ds, bias=False)[0] if ctx.needs_input_grad[1] else None
        dx = ops.linear(ds, w) if ctx.needs_input_grad[0] else None
        return dx, dw, None, None, None


class LabelAttentionFunction(torch.autograd.Function):
    """Attention.forward (MODEL:88-133) in training mode: out [B, NLQ, hid] = fc(dropout(softmax_dh(w_q(lq) w_k(x) / sqrt(dh)))
    w_v(x)); lq [NLQ, hid] is a constant, x [B, C] gets a gradient."""

    @staticmethod
    def forward(ctx, x, lq, seed, rate, n_heads, wq, bq, wk, bk, wv, bv, wfc, bfc):
        Q = ops.linear(lq, wq, bq)
        K = ops.linear(x, wk, bk)
        V = ops.linear(x, wv, bv)
        y, saved = ops.label_attn_train(Q, K, V, n_heads, seed, rate)
        B, NLQ, hid = y.shape
        y2 = y.view(B * NLQ, hid)
        ctx.la = saved
        ctx.save_for_backward(x, lq, wk, wv, wfc, Q, K, V, y2)
        return ops.linear(y2, wfc, bfc).view(B, NLQ, -1)

    @staticmethod
    def backward(ctx, dout):
        x, lq, wk, wv, wfc, Q, K, V, y2 = ctx.saved_tensors
        d2 = dout.reshape(y2.shape[0], -1).contiguous()
        dwfc, dbfc = ops.wgrad(d2, y2)
        dQ, dK, dV = ops.label_attn_train_backward(ops.matmul(d2, wfc), Q, K, V, ctx.la)
        dwq, dbq = ops.wgrad(dQ, lq)
        dwk, dbk = ops.wgrad(dK, x)
        dwv, dbv = ops.wgrad(dV, x)
        dx = ops.train_eltwise(ops.ELT_ADD, ops.matmul(dK, wk), ops.matmul(dV, wv)) if ctx.needs_input_grad[0] else None
        return dx, None, None, None, None, dwq, dbq, dwk, dbk, dwv, dbv, dwfc, dbfc


class DropoutFunction(torch.autograd.Function):
    """Training-mode dropout of x at `site` (ops.dropout); the backward applies the same mask."""

    @staticmethod
    def forward(ctx, x, seed, site, rate):
        y, keep = ops.dropout(x, seed, site, rate)
        ctx.keep, ctx.rate = keep, rate
        return y

    @staticmethod
    def backward(ctx, dy):
        return ops.dropout_backward(dy.contiguous(), ctx.keep, ctx.rate), None, None, None


def label_attention_train_forward(att, query, key, mask=None):
    """model.Attention.forward in training mode: query [NLQ, hid] (the label GloVe: no gradient), key = value [B, C]."""
    if mask is not None:
        raise NotImplementedError("training mode of the label Attention takes no mask (no reference call site passes one)")
    if not key.is_cuda:
        raise RuntimeError("key is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % key.device)
    seed = draw_seed()
    att.last_dropout_seed = seed
    return LabelAttentionFunction.apply(key.contiguous(), query.detach().float().contiguous(), seed, att.do.p, att.n_heads,
                                        att.w_q.weight, att.w_q.bias, att.w_k.weight, att.w_k.bias, att.w_v.weight, att.w_v.bias,
                                        att.fc.weight, att.fc.bias)


def dropout_train_forward(mod, x, site):
    """An nn.Dropout `mod` in training mode at `site`; one seed per call, kept as mod.last_dropout_seed."""
    seed = draw_seed()
    mod.last_dropout_seed = seed
    return DropoutFunction.apply(x.contiguous(), seed, site, mod.p)


# ---- the text encoders (csrc/text_train.hip) ------------------------------------------------------------------------------
class BiLSTMTrainFunction(torch.autograd.Function):
    """bank [B, T, 2H] = the packed 2-layer BiLSTM over the embedded text (ops.bilstm_train) with the inter-layer dropout; gradients
    to the embedding table (row 0, the padding row, gets none) and the 16 LSTM weights / biases.  Every tensor the backward reads
    goes through save_for_backward (the bank is an output: kept in ctx it would form a reference cycle and outlive the step)."""

    TENSORS = ("tok", "lens", "meta", "gates", "cells", "mid", "mid_d", "out")

    @staticmethod
    def forward(ctx, tok, lens, seed, rate, hidden, num_layers, emb, *flat):
        weights = [tuple(flat[4 * i:4 * i + 4]) for i in range(len(flat) // 4)]
        bank, saved = ops.bilstm_train(tok, lens, emb, weights, hidden, num_layers, seed, rate)
        ctx.info = {k: v for k, v in saved.items() if k not in BiLSTMTrainFunction.TENSORS and k != "cat"}
        ctx.n_flat = len(flat)
        ctx.save_for_backward(emb, *flat, *[saved[k] for k in BiLSTMTrainFunction.TENSORS], *[t for c in saved["cat"] for t in c])
        return bank

    @staticmethod
    def backward(ctx, dbank):
        st = ctx.saved_tensors
        nf, nt = ctx.n_flat, len(BiLSTMTrainFunction.TENSORS)
        emb, flat = st[0], st[1:1 + nf]
        saved = dict(ctx.info, **dict(zip(BiLSTMTrainFunction.TENSORS, st[1 + nf:1 + nf + nt])))
        cat = st[1 + nf + nt:]
        saved["cat"] = [(cat[2 * i], cat[2 * i + 1]) for i in range(len(cat) // 2)]
        weights = [tuple(flat[4 * i:4 * i + 4]) for i in range(nf // 4)]
        demb, grads = ops.bilstm_train_backward(dbank, saved, weights, emb, need_emb=ctx.needs_input_grad[6])
        out = [g for tup in grads for g in tup]
        out = [g if ctx.needs_input_grad[7 + i] else None for i, g in enumerate(out)]
        return (None, None, None, None, None, None, demb if ctx.needs_input_grad[6] else None, *out)


class TextGCNTrainFunction(torch.autograd.Function):
    """out [B, D] = relu(dropout(sum over nodes of max over in-edges of w_e h_u)) (ops.textgcn_train); gradients to node_hidden and the
    edge weights through each (node, feature)'s winning in-edge.  Saved tensors go through save_for_backward."""

    @staticmethod
    def forward(ctx, tok, pmi_dev, ngram, max_length, seed, rate, node_hidden, edge_w):
        out, saved = ops.textgcn_train(tok, node_hidden, edge_w, pmi_dev, ngram, max_length, seed, rate)
        ctx.info = {k: v for k, v in saved.items() if k not in ("presum", "win")}
        ctx.save_for_backward(tok, node_hidden, edge_w, saved["presum"], saved["win"], *pmi_dev)
        return out

    @staticmethod
    def backward(ctx, dy):
        tok, node_hidden, edge_w, presum, win, rp, col, eid = ctx.saved_tensors
        saved = dict(ctx.info, presum=presum, win=win)
        dn, de = ops.textgcn_train_backward(dy, tok, node_hidden, edge_w, (rp, col, eid), saved,
                                            need_nodes=ctx.needs_input_grad[6], need_edges=ctx.needs_input_grad[7])
        return None, None, None, None, None, None, dn, (de.view_as(edge_w) if de is not None else None)


def text_gcn_train_forward(tg, doc_ids, rate):
    """Text_GCN.Model's forward with autograd: dropout(rate) before the ReLU (rate = tg.dropout.p in training mode, 0 otherwise); one
    seed per call, kept as tg.last_dropout_seed."""
    if not doc_ids.is_cuda:
        raise RuntimeError("doc_ids is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % doc_ids.device)
    if doc_ids.dim() != 2:
        raise ValueError("doc_ids must be [B,T]")
    seed = draw_seed()
    tg.last_dropout_seed = seed
    tok = doc_ids.long().contiguous()
    return TextGCNTrainFunction.apply(tok, tg.edges_matrix.device_arrays(tok.device), tg.ngram, tg.max_length, seed, rate,
                                      tg.node_hidden.weight, tg.seq_edge_w.weight)


def bilstm_train_forward(lstm, embedding, text, text_lens, rate):
    """The text memory bank with autograd (MODEL:366-398): embedding + packed nn.LSTM `lstm` with dropout(rate) between its layers;
    one seed per call, kept as lstm.last_dropout_seed."""
    if not text.is_cuda:
        raise RuntimeError("text is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % text.device)
    seed = draw_seed()
    lstm.last_dropout_seed = seed
    lens = text_lens.to(device=text.device, dtype=torch.int64).contiguous()
    flat = []
    for layer in range(lstm.num_layers):
        for suffix in ("", "_reverse"):
            flat += [getattr(lstm, "%s_l%d%s" % (n, layer, suffix)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return BiLSTMTrainFunction.apply(text.long().contiguous(), lens, seed, rate, lstm.hidden_size, lstm.num_layers, embedding.weight,
                                     *flat)


# ---- the CNN trunks: stages and stem (csrc/conv_train.hip, bn_train.hip, stem_train.hip) ------------------------
TRUNK_BATCHNORM_MODES = ('frozen', 'batch')
_PACK_KIND = {'frozen': 'folded', 'batch': 'raw'}


class _Saved(int):
    """Where a record's tensor sits among ctx.saved_tensors."""


def _map_record(node, leaf):
    if isinstance(node, SimpleNamespace):
        return SimpleNamespace(**{k: _map_record(v, leaf) for k, v in vars(node).items()})
    if isinstance(node, list):
        return [_map_record(v, leaf) for v in node]
    return leaf(node)


def save_record(ctx, rec):
    """Keep a record -- SimpleNamespaces and lists, nested -- for the backward.  Its tensors go through ctx.save_for_backward (so
    autograd's version check guards parameters and running statistics); what is not a tensor stays where it is."""
    flat = []

    def leaf(v):
        if not torch.is_tensor(v):
            return v
        flat.append(v)
        return _Saved(len(flat) - 1)
    ctx.record = _map_record(rec, leaf)
    ctx.save_for_backward(*flat)


def saved_record(ctx):
    """The record save_record kept, rebuilt over ctx.saved_tensors."""
    st = ctx.saved_tensors
    return _map_record(ctx.record, lambda v: st[v] if isinstance(v, _Saved) else v)


def _batch_norm(z, bn, gamma, beta, **kw):
    """Training-mode BatchNorm of z: the statistics of the batch (ops.bn_stats_bf16_nhwc, which also moves running_mean /
    running_var; num_batches_tracked goes up by one), then gamma, beta, the residual and the ReLU in one sweep
    (ops.bn_apply_bf16_nhwc) -> (activation, mean, rstd)."""
    running = (bn.running_mean, bn.running_var) if bn.track_running_stats and bn.running_mean is not None else None
    mean, rstd = ops.bn_stats_bf16_nhwc(z, bn.eps, running=running, momentum=bn.momentum)
    if running is not None and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return ops.bn_apply_bf16_nhwc(z, mean, rstd, gamma.detach(), beta.detach(), **kw), mean, rstd


def _layer_backward(mode, layer, g, wgrad):
    """The one step of a backward that depends on the mode: from g, the gradient of a layer's output (masked by its ReLU), to the
    gradient of its convolution's output, leaving layer.grads = (dW, dgamma, dbeta) for those of layer.want.  wgrad(gz) ->
    (dW', db') in the pack's layout.  'frozen': BatchNorm is folded into the pack, so the convolution's gradient is g itself and
    ops.conv_bn_unfold takes (dW', db') to the fp32 parameters through the running statistics.  'batch':
    ops.bn_backward_bf16_nhwc differentiates through the statistics of the batch, and dW' of the raw pack is the weight's own
    gradient up to its layout."""
    layer.grads = (None, None, None)
    if mode == 'frozen':
        if any(layer.want):
            layer.grads = ops.conv_bn_unfold(*wgrad(g), layer.w, (layer.gamma, layer.mean, layer.var, layer.eps), want=layer.want)
        return g
    gz, dgamma, dbeta = ops.bn_backward_bf16_nhwc(g, layer.z, layer.mean, layer.rstd, layer.gamma, want=layer.want[1:])
    dw = None
    if layer.want[0]:
        dw = wgrad(gz)[0]
        dw = dw.view(dw.shape[0], layer.k, layer.k, -1).permute(0, 3, 1, 2).contiguous()
    layer.grads = (dw, dgamma, dbeta)
    return gz


def _stage_step(mode, packs, layers, bns, acts):
    """trunk.run_block's step for one block of the stage Function: layer j's activation, kept in acts[j].  'frozen': the eval
    forward's step on the folded packs.  'batch': the raw convolution z, kept in the layer's record with (mean, rstd), then
    _batch_norm."""
    conv = trunk.conv_step(packs)                                    # layer j's convolution on its pack, either kind

    def step(j, t, relu=True, **kw):
        if mode == 'frozen':
            acts[j] = conv(j, t, relu=relu, **kw)
        else:
            layer = layers[j]
            layer.z = conv(j, t, relu=False)
            acts[j], layer.mean, layer.rstd = _batch_norm(layer.z, bns[j], layer.gamma, layer.beta, relu=relu, **kw)
        return acts[j]
    return step


class TrunkStageFunction(torch.autograd.Function):
    """map [B, C, h, w] fp32 = a chain of bottlenecks out = relu(layer3(o2) + idn(x)), o2 = relu(layer2(o1)), o1 = relu(layer1(x)),
    walked by trunk.run_block.  x: NHWC bf16, or NCHW fp32 (converted, as is its gradient).  blocks: the Bottlenecks; params:
    (conv.weight, bn.weight, bn.bias) per trunk.block_layers of each block.
    mode 'frozen' (DESIGN.md 13): a layer is the eval forward's convolution on the folded bf16 weights (packs: trunk.block_packs of
    each block), BatchNorm keeping its running statistics.  keep: None or a list that receives {"x", "blocks": [(o1, o2, out)]}.
    mode 'batch' (DESIGN.md 14), the reference's model.train() semantics: a layer is z = conv(x; bf16(conv.weight)) without a bias
    (packs: trunk.block_packs_raw) and _batch_norm(z).  keep receives {"x", "blocks": [{"z": [z1, z2, z3(, z_d)], "stats":
    [(mean, rstd), ...] -- both in trunk.block_layers order --, "o1", "o2", "out", "idn"}]}.
    Kept for the backward, as one record (save_record): x; per block o1, o2, out; per layer its transposed pack and parameters and
    the running statistics ('frozen') or z, mean, rstd ('batch').
    Backward: dmap is masked by the map and rounded to bf16 NHWC, then per block, last to first, with ' = _layer_backward (which
    also leaves the layer's parameter gradients): g3 = layer3'(g_out), g_d = down'(g_out); g2 = layer2'(dgrad3(g3) masked by o2);
    g1 = layer1'(dgrad2(g2) masked by o1); g_x = dgrad1(g1) + (g_out or dgrad_d(g_d)), masked by x where x is a block's output.
    Gradients travel in bf16 and every sum is fp32; the bf16 roundings of the weights and of z are straight-through.  A parameter
    gets a gradient iff it requires one, and so does x."""

    @staticmethod
    def forward(ctx, x, blocks, packs, keep, mode, *params):
        nchw = x.dtype == torch.float32
        if nchw:
            xh = x.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        elif x.dtype == torch.bfloat16:
            xh = x.detach().contiguous()
        else:
            raise TypeError("TrunkStageFunction: x must be NHWC bfloat16 or NCHW float32, got %s" % x.dtype)
        params = iter(params)
        y, rec, kept = xh, SimpleNamespace(x=xh, blocks=[]), []
        for i, (blk, pk) in enumerate(zip(blocks, packs)):
            bns = [bn for _, bn in trunk.block_layers(blk)]
            layers = [SimpleNamespace(wT=wT, k=k, s=s, p=p, w=next(params), gamma=next(params), beta=next(params))
                      for _, _, wT, k, s, p in pk]
            if mode == 'frozen':
                for layer, bn in zip(layers, bns):
                    layer.mean, layer.var, layer.eps = bn.running_mean, bn.running_var, bn.eps
            acts = {}
            y, idn = trunk.run_block(y, len(pk) == 4, _stage_step(mode, pk, layers, bns, acts), last=i == len(blocks) - 1)
            rec.blocks.append(SimpleNamespace(layers=layers, o1=acts[0], o2=acts[1], out=y))
            if mode == 'frozen':
                kept.append((acts[0], acts[1], y))
            else:
                kept.append({"z": [layer.z for layer in layers], "stats": [(layer.mean, layer.rstd) for layer in layers],
                             "o1": acts[0], "o2": acts[1], "out": y, "idn": idn})
        if keep is not None:
            keep.append({"x": xh, "blocks": kept})
        ctx.nchw, ctx.mode = nchw, mode
        save_record(ctx, rec)
        return y

    @staticmethod
    def backward(ctx, dmap):
        rec = saved_record(ctx)
        need = iter(ctx.needs_input_grad[5:])
        for blk in rec.blocks:
            for layer in blk.layers:
                layer.want = (next(need), next(need), next(need))

        def through(layer, x_in, g):
            return _layer_backward(ctx.mode, layer, g, lambda gz: ops.conv_wgrad_bf16_nhwc(x_in, gz, layer.k, layer.s, layer.p))

        def dgrad(layer, g, x_in, mask=None, add=None):
            return ops.conv_dgrad_bf16_nhwc(g, layer.wT, tuple(x_in.shape[1:3]), layer.k, layer.s, layer.p, mask=mask, add=add)

        g = ops.map_grad_relu_nhwc(rec.blocks[-1].out, dmap.contiguous().float())
        for bi in range(len(rec.blocks) - 1, -1, -1):
            blk = rec.blocks[bi]
            x_in = rec.blocks[bi - 1].out if bi else rec.x
            l1, l2, l3 = blk.layers[:3]
            down = blk.layers[3] if len(blk.layers) == 4 else None
            g3 = through(l3, blk.o2, g)
            gd = through(down, x_in, g) if down is not None else None
            g2 = through(l2, blk.o1, dgrad(l3, g3, blk.o2, mask=blk.o2))
            g1 = through(l1, x_in, dgrad(l2, g2, blk.o1, mask=blk.o1))
            if bi == 0 and not ctx.needs_input_grad[0]:
                g = None
                break
            other = dgrad(down, gd, x_in) if down is not None else g
            g = dgrad(l1, g1, x_in, mask=x_in if bi else None, add=other)
        if g is not None and ctx.nchw:
            g = g.float().permute(0, 3, 1, 2).contiguous()
        return (g, None, None, None, None, *[t for blk in rec.blocks for layer in blk.layers for t in layer.grads])


class TrunkStemFunction(torch.autograd.Function):
    """y [B, OH/2, OW/2, 64] bf16 NHWC = maxpool(y0), y0 = relu(bn1(conv1(img))), the stem of a trunk.
    mode 'frozen': the eval stem, bit for bit (ops.stem_conv7 on the folded pack `pack` = (wt, bias) of trunk.layer_pack(..., stem=True),
    then ops.maxpool3x3s2_nhwc).  keep: None or a list that receives {"img": the image as bf16 (what the convolution multiplied),
    "y0", "y"}.
    mode 'batch': z0 = conv1(bf16(img); bf16(conv1.weight)) without bias or ReLU (ops.stem_conv7(raw=True) on the raw pack) and
    y0 = _batch_norm(z0), which moves bn1's running buffers.  keep receives "z0" and "stats": (mean, rstd) as well.
    Backward, from g_y (bf16 NHWC, the stage Function's unmasked input gradient): g_y0 = ops.maxpool3x3s2_bwd_nhwc(y0, g_y,
    relu_mask=True) -- the pool's first-maximum routing and the ReLU's mask in one rounding --, then _layer_backward over
    ops.stem_wgrad(img, .) gives the gradients of conv1.weight, bn1.weight and bn1.bias; each gets one iff it requires one.  The image
    never gets a gradient (None): no kernel here differentiates the stem with respect to its input."""

    @staticmethod
    def forward(ctx, img, bn, pack, keep, mode, conv_w, gamma, beta):
        imgc = img.detach().contiguous()
        if mode == 'frozen':
            y0, kept = ops.stem_conv7(imgc, *pack), {}
            layer = SimpleNamespace(w=conv_w, gamma=gamma, mean=bn.running_mean, var=bn.running_var, eps=bn.eps)
        else:
            z0 = ops.stem_conv7(imgc, *pack, raw=True)
            y0, mean, rstd = _batch_norm(z0, bn, gamma, beta)
            kept = {"z0": z0, "stats": (mean, rstd)}
            layer = SimpleNamespace(k=7, gamma=gamma, z=z0, mean=mean, rstd=rstd)
        y = ops.maxpool3x3s2_nhwc(y0)
        if keep is not None:
            keep.append({"img": imgc.to(torch.bfloat16), "y0": y0, "y": y, **kept})
        ctx.mode = mode
        save_record(ctx, SimpleNamespace(img=imgc, y0=y0, layer=layer))
        return y

    @staticmethod
    def backward(ctx, g_y):
        want = tuple(ctx.needs_input_grad[5:8])
        if not any(want):
            return (None,) * 8
        rec = saved_record(ctx)
        if g_y.dtype != torch.bfloat16:
            raise TypeError("the stem's backward takes the stage Function's bf16 NHWC input gradient, got %s" % g_y.dtype)
        rec.layer.want = want
        _layer_backward(ctx.mode, rec.layer, ops.maxpool3x3s2_bwd_nhwc(rec.y0, g_y.contiguous(), relu_mask=True),
                        lambda gz: ops.stem_wgrad(rec.img, gz))
        return (None, None, None, None, None, *rec.layer.grads)


def trunk_stem_forward(conv, bn, img, pack=None, keep=None, batchnorm='frozen'):
    """The stem of a trunk -- conv (7x7 / 2 / 3, 3 -> 64, no bias), bn, ReLU, MaxPool2d(3, 2, 1) -- over img [B,3,H,W] fp32 with
    autograd: -> [B, h, w, 64] bf16 NHWC, which requires a gradient iff one of conv.weight, bn.weight, bn.bias does.  pack: the folded
    stem pack if the caller has it (frozen mode), else the conv module's own (trunk.layer_pack)."""
    if batchnorm not in TRUNK_BATCHNORM_MODES:
        raise ValueError("batchnorm must be one of %s, got %r" % (TRUNK_BATCHNORM_MODES, batchnorm))
    if not img.is_cuda:
        raise RuntimeError("img is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % img.device)
    if conv.bias is not None:
        raise NotImplementedError("trunk fine-tuning: convolutions with a bias are not supported (torchvision's have none)")
    if pack is None or batchnorm == 'batch':
        pack = trunk.layer_pack(conv, bn, _PACK_KIND[batchnorm], stem=True)
    return TrunkStemFunction.apply(img, bn, pack[:2], keep, batchnorm, conv.weight, bn.weight, bn.bias)


def trunk_stage_forward(stages, x, keep=None, batchnorm='frozen'):
    """The feature map of `stages` -- an nn.Sequential of trunk.Bottleneck, or a list of such stages run one after the other -- over
    x (NHWC bf16 or NCHW fp32) with autograd (TrunkStageFunction).  batchnorm='frozen': BatchNorm uses and keeps its running
    statistics.  batchnorm='batch': BatchNorm normalises with the statistics of the batch, moves its running buffers and is
    differentiated through the statistics, whatever the blocks' .training flags say."""
    if batchnorm not in TRUNK_BATCHNORM_MODES:
        raise ValueError("batchnorm must be one of %s, got %r" % (TRUNK_BATCHNORM_MODES, batchnorm))
    if not x.is_cuda:
        raise RuntimeError("x is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % x.device)
    if isinstance(stages, torch.nn.Sequential) and all(isinstance(b, trunk.Bottleneck) or hasattr(b, "conv3") for b in stages):
        stages = [stages]
    blocks = [b for st in stages for b in st]
    if not blocks:
        raise ValueError("trunk_stage_forward: no bottleneck blocks")
    params = [t for b in blocks for conv, bn in trunk.block_layers(b) for t in (conv.weight, bn.weight, bn.bias)]
    packs = [trunk.block_packs_raw(b) if batchnorm == 'batch' else trunk.block_packs(b) for b in blocks]
    return TrunkStageFunction.apply(x, blocks, packs, keep, batchnorm, *params)
