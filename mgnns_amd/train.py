"""Training mode of the fusion layers: autograd Functions over the HIP kernels of csrc/mha_train.hip.

fusion.MultiHeadAttention and fusion.PositionwiseFeedForward run these when `self.training` is set, with the reference's
semantics (submodules.py:15-139): dropout on the attention probabilities (`attn_dropout`, the reference's
`attention.dropout`), after `fc` and after `w_2` (the layers' own `dropout`), and the custom LayerNorm (unbiased std, eps added
to the std).  Everything is fp32.  The masks are drawn from a counter-based hash of a seed the module draws from torch's default
generator per training forward (kept as `last_dropout_seed`), so torch.manual_seed reproduces a run bit for bit.
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
