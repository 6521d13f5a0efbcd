"""Training mode of the fusion layers: autograd Functions over the HIP kernels of csrc/mha_train.hip.

fusion.MultiHeadAttention and fusion.PositionwiseFeedForward run these when `self.training` is set, with the reference's
semantics (submodules.py:15-139): dropout on the attention probabilities (`attn_dropout`, the reference's
`attention.dropout`), after `fc` and after `w_2` (the layers' own `dropout`), and the custom LayerNorm (unbiased std, eps added
to the std).  Everything is fp32.  The masks are drawn from a counter-based hash of a seed the module draws from torch's default
generator per training forward (kept as `last_dropout_seed`), so torch.manual_seed reproduces a run bit for bit.

The rest of the model trains through the Functions below the fusion layers' (csrc/model_train.hip): the image memory banks
(their weight gradient is the backward's hot path), the label GCN (propagated back with the transposed adjacency), the label
attention with dropout on its probabilities, the channel tails and the classifier with its dropout.  The text encoders train
through the Functions at the end of this file once unfrozen.  Feature maps that require a gradient get one (ImgBankFunction,
csrc/map_grad.hip), so a torch trunk in front of the model fine-tunes through torch's own backward; the trunks of
mgnns_amd.trunk fine-tune their trailing bottleneck stages with frozen BatchNorm statistics through TrunkStageFunction
(csrc/conv_train.hip, model.unfreeze_trunks()), or with the statistics of the batch -- the reference's semantics -- through
TrunkStageBatchNormFunction (csrc/bn_train.hip, model.unfreeze_trunks(batchnorm='batch')).  With all four stages trainable the
stem -- conv1, bn1, ReLU, max-pool -- trains too, through TrunkStemFunction / TrunkStemBatchNormFunction (csrc/stem_train.hip,
model.unfreeze_trunks(4, stem=True)): nothing of a trunk is then left frozen.
"""
import torch

from . import ops


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


# ---- the CNN trunks' trailing stages (csrc/conv_train.hip) ------------------------------------------------------------------
class TrunkStageFunction(torch.autograd.Function):
    """map [B, C, h, w] fp32 = a chain of bottlenecks out = relu(conv3(o2) + idn(x)), o2 = relu(conv2(o1)), o1 = relu(conv1(x)), run by
    the eval forward's kernels on the folded bf16 weights (BatchNorm keeps its running statistics) with x, o1, o2 of every block
    and the map kept for the backward.  x: NHWC bf16, or NCHW fp32 (converted, as is its gradient).  blocks: the Bottlenecks;
    packs: trunk.block_packs of each; keep: None or a list that receives the saved activations {"x", "blocks": [(o1, o2, out)]}
    (what tests compute their reference from); params: (conv.weight, bn.weight, bn.bias) per trunk.block_layers of each block.
    Backward: dmap is masked by the map and rounded to bf16 NHWC, then per block, last to first: weight
    gradients of conv3 and the downsample from g_out; g_o2 = dgrad_conv3(g_out) masked by o2; wgrad conv2; g_o1 =
    dgrad_conv2(g_o2) masked by o1; wgrad conv1; g_x = dgrad_conv1(g_o1) + (g_out or dgrad_down(g_out)), masked by x where x is a
    block's output.  Gradients travel in bf16, accumulate in fp32 and reach the fp32 parameters through ops.conv_bn_unfold;
    a parameter gets one iff it requires one, and so does x."""

    @staticmethod
    def forward(ctx, x, blocks, packs, keep, *params):
        nchw = x.dtype == torch.float32
        if nchw:
            xh = x.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        elif x.dtype == torch.bfloat16:
            xh = x.detach().contiguous()
        else:
            raise TypeError("TrunkStageFunction: x must be NHWC bfloat16 or NCHW float32, got %s" % x.dtype)
        y, acts, stats = xh, [], []
        for i, (blk, pk) in enumerate(zip(blocks, packs)):
            last = i == len(blocks) - 1
            idn = y
            if len(pk) == 4:
                wt, bias, _, k, s, p = pk[3]
                idn = ops.conv_bf16_nhwc(y, wt, bias, k, s, p, relu=False)
            wt, bias, _, k, s, p = pk[0]
            o1 = ops.conv_bf16_nhwc(y, wt, bias, k, s, p)
            wt, bias, _, k, s, p = pk[1]
            o2 = ops.conv_bf16_nhwc(o1, wt, bias, k, s, p)
            wt, bias, _, k, s, p = pk[2]
            y = ops.conv_bf16_nhwc(o2, wt, bias, k, s, p, residual=idn, out_nchw_f32=last)
            acts += [o1, o2, y]
            stats += [t for _, bn in _block_layers(blk) for t in (bn.running_mean, bn.running_var)]
        if keep is not None:
            keep.append({"x": xh, "blocks": [tuple(acts[3 * i:3 * i + 3]) for i in range(len(blocks))]})
        ctx.nchw, ctx.nblk = nchw, len(blocks)
        ctx.geom = [[(k, s, p) for _, _, _, k, s, p in pk] for pk in packs]
        ctx.eps = [[bn.eps for _, bn in _block_layers(blk)] for blk in blocks]
        wTs = [c[2] for pk in packs for c in pk]
        ctx.save_for_backward(xh, *acts, *wTs, *stats, *params)
        return y

    @staticmethod
    def backward(ctx, dmap):
        st = ctx.saved_tensors
        nb = ctx.nblk
        nconv = [len(g) for g in ctx.geom]
        total = sum(nconv)
        xh, acts = st[0], st[1:1 + 3 * nb]
        wTs, stats, params = st[1 + 3 * nb:1 + 3 * nb + total], st[1 + 3 * nb + total:1 + 3 * nb + 3 * total], st[1 + 3 * nb + 3 * total:]
        need = ctx.needs_input_grad[4:]
        grads = [None] * len(params)
        base = [sum(nconv[:i]) for i in range(nb)]

        def weight_grads(bi, ci, x_in, g):
            j = base[bi] + ci
            want = tuple(need[3 * j:3 * j + 3])
            if not any(want):
                return
            k, s, p = ctx.geom[bi][ci]
            dwp, dbp = ops.conv_wgrad_bf16_nhwc(x_in, g, k, s, p)
            grads[3 * j:3 * j + 3] = ops.conv_bn_unfold(dwp, dbp, params[3 * j], (params[3 * j + 1], stats[2 * j], stats[2 * j + 1],
                                                                               ctx.eps[bi][ci]), want=want)

        def data_grad(bi, ci, g, x_in, mask=None, add=None):
            k, s, p = ctx.geom[bi][ci]
            return ops.conv_dgrad_bf16_nhwc(g, wTs[base[bi] + ci], tuple(x_in.shape[1:3]), k, s, p, mask=mask, add=add)

        g = ops.map_grad_relu_nhwc(acts[3 * nb - 1], dmap.contiguous().float())
        for bi in range(nb - 1, -1, -1):
            x_in = acts[3 * bi - 1] if bi else xh
            o1, o2 = acts[3 * bi], acts[3 * bi + 1]
            down = nconv[bi] == 4
            weight_grads(bi, 2, o2, g)
            if down:
                weight_grads(bi, 3, x_in, g)
            g2 = data_grad(bi, 2, g, o2, mask=o2)
            weight_grads(bi, 1, o1, g2)
            g1 = data_grad(bi, 1, g2, o1, mask=o1)
            weight_grads(bi, 0, x_in, g1)
            if bi == 0 and not ctx.needs_input_grad[0]:
                g = None
                break
            other = data_grad(bi, 3, g, x_in) if down else g
            g = data_grad(bi, 0, g1, x_in, mask=x_in if bi else None, add=other)
        if g is not None and ctx.nchw:
            g = g.float().permute(0, 3, 1, 2).contiguous()
        return (g, None, None, None, *grads)


class TrunkStageBatchNormFunction(torch.autograd.Function):
    """TrunkStageFunction with batch statistics, the reference's model.train() semantics for the stages it runs: every
    convolution is z = conv(x; bf16(conv.weight)) without a bias (packs: trunk.block_packs_raw), every BatchNorm normalises z with
    the statistics of the batch (ops.bn_stats_bf16_nhwc, which also moves running_mean / running_var; num_batches_tracked goes up by
    one) and applies gamma, beta, the residual and the ReLU in one sweep (ops.bn_apply_bf16_nhwc); the last block's output is the
    fp32 NCHW map.  Kept for the backward: x, per block z1, o1, z2, o2, z3, out (and the downsample's z_d), and (mean, rstd) per
    layer.  keep: None or a list that receives {"x", "blocks": [{"z": [z1, z2, z3(, z_d)], "stats": [(mean, rstd), ...] -- both in
    trunk.block_layers order --, "o1", "o2", "out", "idn"}]}.  params: (conv.weight, bn.weight, bn.bias) per layer.
    Backward: dmap is masked by the map and rounded to bf16 NHWC; then per block, last to first, with bn' = ops.bn_backward_bf16_nhwc
    (which differentiates through the statistics): g_z3 = bn3'(g_out), g_zd = bn_d'(g_out), dW3 = wgrad(o2, g_z3), dWd = wgrad(x, g_zd),
    g_o2 = dgrad3(g_z3) masked by o2, g_z2 = bn2'(g_o2), dW2 = wgrad(o1, g_z2), g_o1 = dgrad2(g_z2) masked by o1, g_z1 = bn1'(g_o1),
    dW1 = wgrad(x, g_z1), g_x = dgrad1(g_z1) + (g_out or dgrad_d(g_zd)), masked by x where x is a block's output.  The bf16 roundings of
    the weight and of z are straight-through; gradients travel in bf16 and every sum is fp32; dW of the raw pack is the weight's own
    gradient up to its layout.  A parameter gets a gradient iff it requires one, and so does x."""

    @staticmethod
    def forward(ctx, x, blocks, packs, keep, *params):
        nchw = x.dtype == torch.float32
        if nchw:
            xh = x.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        elif x.dtype == torch.bfloat16:
            xh = x.detach().contiguous()
        else:
            raise TypeError("TrunkStageBatchNormFunction: x must be NHWC bfloat16 or NCHW float32, got %s" % x.dtype)

        def bn_layer(z, bn, residual=None, relu=True, out_nchw_f32=False):
            running = (bn.running_mean, bn.running_var) if bn.track_running_stats and bn.running_mean is not None else None
            mean, rstd = ops.bn_stats_bf16_nhwc(z, bn.eps, running=running, momentum=bn.momentum)
            if running is not None and bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
            y = ops.bn_apply_bf16_nhwc(z, mean, rstd, bn.weight.detach(), bn.bias.detach(), residual=residual, relu=relu,
                                       out_nchw_f32=out_nchw_f32)
            return y, (mean, rstd)

        y, acts, stats, kept = xh, [], [], []
        for i, (blk, pk) in enumerate(zip(blocks, packs)):
            layers = _block_layers(blk)
            raw = lambda t, j: ops.conv_bf16_nhwc(t, pk[j][0], pk[j][1], *pk[j][3:], relu=False)
            idn, zd, st_d = y, None, None
            if len(pk) == 4:
                zd = raw(y, 3)
                idn, st_d = bn_layer(zd, layers[3][1], relu=False)
            z1 = raw(y, 0)
            o1, st1 = bn_layer(z1, layers[0][1])
            z2 = raw(o1, 1)
            o2, st2 = bn_layer(z2, layers[1][1])
            z3 = raw(o2, 2)
            y, st3 = bn_layer(z3, layers[2][1], residual=idn, out_nchw_f32=i == len(blocks) - 1)
            zs, sts = [z1, z2, z3], [st1, st2, st3]
            if zd is not None:
                zs.append(zd)
                sts.append(st_d)
            acts += [o1, o2, y] + zs
            stats += [t for s_ in sts for t in s_]
            kept.append({"z": zs, "stats": sts, "o1": o1, "o2": o2, "out": y, "idn": idn})
        if keep is not None:
            keep.append({"x": xh, "blocks": kept})
        ctx.nchw = nchw
        ctx.geom = [[(k, s, p) for _, _, _, k, s, p in pk] for pk in packs]
        wTs = [c[2] for pk in packs for c in pk]
        ctx.save_for_backward(xh, *acts, *stats, *wTs, *params)
        return y

    @staticmethod
    def backward(ctx, dmap):
        st = list(ctx.saved_tensors)
        nconv = [len(g) for g in ctx.geom]
        nb, total = len(nconv), sum(nconv)
        xh = st.pop(0)
        blk_acts = []
        for n in nconv:
            blk_acts.append((st[0], st[1], st[2], st[3:3 + n]))            # o1, o2, out, [z per layer]
            del st[:3 + n]
        stats, wTs, params = st[:2 * total], st[2 * total:3 * total], st[3 * total:]
        need = ctx.needs_input_grad[4:]
        grads = [None] * len(params)
        base = [sum(nconv[:i]) for i in range(nb)]

        def bn_back(bi, ci, g):
            j = base[bi] + ci
            gz, grads[3 * j + 1], grads[3 * j + 2] = ops.bn_backward_bf16_nhwc(
                g, blk_acts[bi][3][ci], stats[2 * j], stats[2 * j + 1], params[3 * j + 1], want=(need[3 * j + 1], need[3 * j + 2]))
            return gz

        def weight_grad(bi, ci, x_in, gz):
            j = base[bi] + ci
            if need[3 * j]:
                k, s, p = ctx.geom[bi][ci]
                dw = ops.conv_wgrad_bf16_nhwc(x_in, gz, k, s, p)[0]
                grads[3 * j] = dw.view(dw.shape[0], k, k, -1).permute(0, 3, 1, 2).contiguous()

        def data_grad(bi, ci, g, x_in, mask=None, add=None):
            k, s, p = ctx.geom[bi][ci]
            return ops.conv_dgrad_bf16_nhwc(g, wTs[base[bi] + ci], tuple(x_in.shape[1:3]), k, s, p, mask=mask, add=add)

        g = ops.map_grad_relu_nhwc(blk_acts[-1][2], dmap.contiguous().float())
        for bi in range(nb - 1, -1, -1):
            x_in = blk_acts[bi - 1][2] if bi else xh
            o1, o2 = blk_acts[bi][0], blk_acts[bi][1]
            down = nconv[bi] == 4
            gz3 = bn_back(bi, 2, g)
            weight_grad(bi, 2, o2, gz3)
            gzd = None
            if down:
                gzd = bn_back(bi, 3, g)
                weight_grad(bi, 3, x_in, gzd)
            gz2 = bn_back(bi, 1, data_grad(bi, 2, gz3, o2, mask=o2))
            weight_grad(bi, 1, o1, gz2)
            gz1 = bn_back(bi, 0, data_grad(bi, 1, gz2, o1, mask=o1))
            weight_grad(bi, 0, x_in, gz1)
            if bi == 0 and not ctx.needs_input_grad[0]:
                g = None
                break
            other = data_grad(bi, 3, gzd, x_in) if down else g
            g = data_grad(bi, 0, gz1, x_in, mask=x_in if bi else None, add=other)
        if g is not None and ctx.nchw:
            g = g.float().permute(0, 3, 1, 2).contiguous()
        return (g, None, None, None, *grads)


TRUNK_BATCHNORM_MODES = ('frozen', 'batch')


# ---- the CNN trunks' stem (csrc/stem_train.hip) -----------------------------------------------------------------
def _stem_gy(g_y, y0):
    if g_y.dtype != torch.bfloat16:
        raise TypeError("the stem's backward takes the stage Function's bf16 NHWC input gradient, got %s" % g_y.dtype)
    return ops.maxpool3x3s2_bwd_nhwc(y0, g_y.contiguous(), relu_mask=True)


class TrunkStemFunction(torch.autograd.Function):
    """y [B, OH/2, OW/2, 64] bf16 NHWC = maxpool(y0), y0 = relu(bn1(conv1(img))) with frozen statistics: the eval stem, bit for bit
    (ops.stem_conv7 on the folded pack `pack` = (wt, bias) of ops.conv_fold_bn(..., stem=True), then ops.maxpool3x3s2_nhwc).  Kept for
    the backward: the fp32 image and y0.  keep: None or a list that receives {"img": the image as bf16 (what the convolution
    multiplied), "y0", "y"}.  Backward, from g_y (bf16 NHWC, the stage Function's unmasked input gradient): g_y0 =
    ops.maxpool3x3s2_bwd_nhwc(y0, g_y, relu_mask=True) -- the pool's first-maximum routing and the ReLU's mask in one rounding --,
    (dW', db') = ops.stem_wgrad(img, g_y0), and ops.conv_bn_unfold gives the gradients of conv1.weight, bn1.weight and bn1.bias; each
    gets one iff it requires one.  The image never gets a gradient (None): no kernel here differentiates the stem with respect to
    its input."""

    @staticmethod
    def forward(ctx, img, bn, pack, keep, conv_w, gamma, beta):
        imgc = img.detach().contiguous()
        y0 = ops.stem_conv7(imgc, *pack)
        y = ops.maxpool3x3s2_nhwc(y0)
        if keep is not None:
            keep.append({"img": imgc.to(torch.bfloat16), "y0": y0, "y": y})
        ctx.eps = bn.eps
        ctx.save_for_backward(imgc, y0, bn.running_mean, bn.running_var, conv_w, gamma)
        return y

    @staticmethod
    def backward(ctx, g_y):
        img, y0, mean, var, conv_w, gamma = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[4:7])
        if not any(want):
            return (None,) * 7
        dwp, dbp = ops.stem_wgrad(img, _stem_gy(g_y, y0))
        return (None, None, None, None, *ops.conv_bn_unfold(dwp, dbp, conv_w, (gamma, mean, var, ctx.eps), want=want))


class TrunkStemBatchNormFunction(torch.autograd.Function):
    """TrunkStemFunction with batch statistics: z0 = conv1(bf16(img); bf16(conv1.weight)) without bias or ReLU (ops.stem_conv7(raw=True)
    on `pack` = ops.conv_fold_bn(w, None, None, stem=True)), (mean, rstd) of z0 over the batch (ops.bn_stats_bf16_nhwc, which moves
    bn1.running_mean / running_var; num_batches_tracked goes up by one), y0 = relu(gamma (z0 - mean) rstd + beta)
    (ops.bn_apply_bf16_nhwc), y = maxpool(y0).  Kept: the image, z0, y0, (mean, rstd); keep receives {"img" (bf16), "z0", "y0", "y",
    "stats": (mean, rstd)}.  Backward: g_y0 as in TrunkStemFunction, (g_z0, dgamma, dbeta) = ops.bn_backward_bf16_nhwc(g_y0, z0, ...)
    through the statistics, dW = ops.stem_wgrad(img, g_z0)[0] re-laid out as conv1.weight (the bf16 rounding of the weight is
    straight-through).  A parameter gets a gradient iff it requires one; the image never does."""

    @staticmethod
    def forward(ctx, img, bn, pack, keep, conv_w, gamma, beta):
        imgc = img.detach().contiguous()
        z0 = ops.stem_conv7(imgc, *pack, raw=True)
        running = (bn.running_mean, bn.running_var) if bn.track_running_stats and bn.running_mean is not None else None
        mean, rstd = ops.bn_stats_bf16_nhwc(z0, bn.eps, running=running, momentum=bn.momentum)
        if running is not None and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        y0 = ops.bn_apply_bf16_nhwc(z0, mean, rstd, gamma.detach(), beta.detach())
        y = ops.maxpool3x3s2_nhwc(y0)
        if keep is not None:
            keep.append({"img": imgc.to(torch.bfloat16), "z0": z0, "y0": y0, "y": y, "stats": (mean, rstd)})
        ctx.save_for_backward(imgc, z0, y0, mean, rstd, gamma)
        return y

    @staticmethod
    def backward(ctx, g_y):
        img, z0, y0, mean, rstd, gamma = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[4:7])
        if not any(want):
            return (None,) * 7
        gz, dgamma, dbeta = ops.bn_backward_bf16_nhwc(_stem_gy(g_y, y0), z0, mean, rstd, gamma, want=want[1:])
        dw = None
        if want[0]:
            dw = ops.stem_wgrad(img, gz)[0].view(64, 7, 7, 3).permute(0, 3, 1, 2).contiguous()
        return (None, None, None, None, dw, dgamma, dbeta)


def stem_pack_raw(conv):
    """(bf16(conv1.weight) in the stem's [64, 160] layout, a zero bias): the pack of batch-statistics fine-tuning, kept on the module
    and rebuilt when the weight changes."""
    from .derived import derived
    store = conv.__dict__.setdefault("_train_packs_raw", {})
    return derived(store, "stem", (conv.weight,), lambda: ops.conv_fold_bn(conv.weight.detach().contiguous(), None, None, stem=True))


def trunk_stem_forward(conv, bn, img, pack=None, keep=None, batchnorm='frozen'):
    """The stem of a trunk -- conv (7x7 / 2 / 3, 3 -> 64, no bias), bn, ReLU, MaxPool2d(3, 2, 1) -- over img [B,3,H,W] fp32 with
    autograd: -> [B, h, w, 64] bf16 NHWC, which requires a gradient iff one of conv.weight, bn.weight, bn.bias does.  pack: the folded
    stem pack if the caller has it (frozen mode), else it is built here."""
    if batchnorm not in TRUNK_BATCHNORM_MODES:
        raise ValueError("batchnorm must be one of %s, got %r" % (TRUNK_BATCHNORM_MODES, batchnorm))
    if not img.is_cuda:
        raise RuntimeError("img is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % img.device)
    if conv.bias is not None:
        raise NotImplementedError("trunk fine-tuning: convolutions with a bias are not supported (torchvision's have none)")
    if batchnorm == 'batch':
        return TrunkStemBatchNormFunction.apply(img, bn, stem_pack_raw(conv), keep, conv.weight, bn.weight, bn.bias)
    if pack is None:
        from .trunk import ResNetFeatures
        pack = ResNetFeatures._fold(conv, bn, stem=True)
    return TrunkStemFunction.apply(img, bn, pack, keep, conv.weight, bn.weight, bn.bias)


def _block_layers(blk):
    from .trunk import block_layers
    return block_layers(blk)


def trunk_stage_forward(stages, x, keep=None, batchnorm='frozen'):
    """The feature map of `stages` -- an nn.Sequential of trunk.Bottleneck, or a list of such stages run one after the other -- over
    x (NHWC bf16 or NCHW fp32) with autograd.  batchnorm='frozen' (TrunkStageFunction): BatchNorm uses and keeps its running
    statistics.  batchnorm='batch' (TrunkStageBatchNormFunction): BatchNorm normalises with the statistics of the batch, moves its
    running buffers and is differentiated through the statistics, whatever the blocks' .training flags say."""
    from .trunk import Bottleneck, block_packs, block_packs_raw
    if batchnorm not in TRUNK_BATCHNORM_MODES:
        raise ValueError("batchnorm must be one of %s, got %r" % (TRUNK_BATCHNORM_MODES, batchnorm))
    if not x.is_cuda:
        raise RuntimeError("x is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % x.device)
    if isinstance(stages, torch.nn.Sequential) and all(isinstance(b, Bottleneck) or hasattr(b, "conv3") for b in stages):
        stages = [stages]
    blocks = [b for st in stages for b in st]
    if not blocks:
        raise ValueError("trunk_stage_forward: no bottleneck blocks")
    params = [t for b in blocks for conv, bn in _block_layers(b) for t in (conv.weight, bn.weight, bn.bias)]
    if batchnorm == 'batch':
        return TrunkStageBatchNormFunction.apply(x, blocks, [block_packs_raw(b) for b in blocks], keep, *params)
    return TrunkStageFunction.apply(x, blocks, [block_packs(b) for b in blocks], keep, *params)
