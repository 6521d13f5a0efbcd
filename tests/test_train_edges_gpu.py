"""Edge sweeps of the training kernels (csrc/mha_train.hip, csrc/model_train.hip), each through its ops.* wrapper, forward and
backward, against fp64 autograd on the CPU of the same formula, with every dropout mask taken from the host restatement of the
hash (tests/dropout_ref.py) at the documented index rather than from the kernel.  Gate: 1e-4 of each tensor's largest
magnitude.  The grids are hand-picked cases, not cross products: each value of each axis appears, and the cases sit where a
kernel's partition changes (a wave per bank row, 64-float chunks, 16-row tiles, 64-row slabs, the direct bank path)."""
import math

import pytest
import torch

from mgnns_amd import ops
from tests import dropout_ref as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def close(got, ref, what, tol=1e-4):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "%s: non-finite values" % what
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale + 1e-12, "%s: max err %.3e vs max |ref| %.3e" % (what, err, scale)


def drop(x, keep, rate):
    return x * keep.to(x.dtype) / (1.0 - rate) if rate < 1.0 else x * 0.0


def host_attn_keep(seed, rate, H, B, L):
    return torch.from_numpy(DR.attn_keep(seed, rate, H, B, L))


def make_mask(kind, B, L, g):
    """[B, L] float (1 = live) or None."""
    if kind == "none":
        return None
    m = torch.zeros(B, L)
    if kind == "ragged":
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0] = L
        m = (torch.arange(L)[None, :] < lens[:, None]).float()
    elif kind == "first":
        m[:, 0] = 1
    elif kind == "last":
        m[:, L - 1] = 1
    elif kind == "middle":
        m[:, L // 2] = 1
    elif kind == "mod8":                         # rows l = 3 (mod 8): every live row on wave 3 of the bank pass
        m[:, 3::8] = 1
    else:
        raise ValueError(kind)
    return m


# ---- attention core ---------------------------------------------------------------------------------------------------------
def core_ref(qh, bank, mask, wk, wv, bv, H, dk, keep, rate):
    """fp64 attention core over the reference's formulation: K, V projected (b_k drops out of the softmax), softmax over the
    live rows, dropout on the probabilities.  -> (o [B, H*dk], attn [H*B, 1, L])."""
    B, L, D = bank.shape
    kh = (bank @ wk.t()).view(B, L, H, dk)
    vh = (bank @ wv.t() + bv).view(B, L, H, dk)
    s = torch.einsum("bhd,blhd->bhl", qh.view(B, H, dk), kh) / math.sqrt(dk)
    empty = torch.zeros(B, dtype=torch.bool) if mask is None else mask.sum(1) == 0
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, float("-inf")).masked_fill(empty[:, None, None], 0.0)
    # a sample without a live row contributes nothing: the training-mode rule (the reference's softmax would give NaN)
    p = torch.softmax(s, dim=2).masked_fill(empty[:, None, None], 0.0)
    pd = drop(p, keep.view(H, B, L).permute(1, 0, 2), rate)
    o = torch.einsum("bhl,blhd->bhd", pd, vh).reshape(B, H * dk)
    return o, pd.permute(1, 0, 2).reshape(H * B, 1, L)


def core_inputs(B, L, D, H, dk, seed):
    g = torch.Generator().manual_seed(seed)
    qh = torch.randn(B, H * dk, generator=g)
    bank = torch.randn(B, L, D, generator=g)
    wk = torch.randn(H * dk, D, generator=g) / math.sqrt(D)
    wv = torch.randn(H * dk, D, generator=g) / math.sqrt(D)
    bv = torch.randn(H * dk, generator=g)
    G = torch.randn(B, H * dk, generator=g)
    return g, qh, bank, wk, wv, bv, G


def run_core(qh, bank, mask, wk, wv, bv, H, dk, seed, rate, G, want_dbank=True):
    d = [t.to(DEV) if t is not None else None for t in (qh, bank, mask, wk, wv, bv, G)]
    o, attn, saved, keep = ops.mha_attn_train(d[0], d[1], d[2], H, dk, d[3], d[4], d[5], seed, rate, return_masks=True)
    grads = ops.mha_attn_train_backward(d[6], d[0], d[1], d[2], d[3], d[4], d[5], saved, want_dbank=want_dbank)
    return o, attn, keep, grads


def core_check(B, L, D, dk, H, rate, kind, seed=5, mask=None):
    """Forward and backward of the core against fp64 autograd; returns the GPU results."""
    g, qh, bank, wk, wv, bv, G = core_inputs(B, L, D, H, dk, seed=B * 1000 + L * 10 + H)
    if mask is None:
        mask = make_mask(kind, B, L, g)
    o, attn, keep, (dqh, dwk, dwv, dbv, dbank) = run_core(qh, bank, mask, wk, wv, bv, H, dk, seed, rate, G)
    hk = host_attn_keep(seed, rate, H, B, L)
    assert torch.equal(keep.cpu(), hk), "attention keep mask differs from the host restatement"
    r = [t.double().requires_grad_(True) for t in (qh, bank, wk, wv, bv)]
    ro, rattn = core_ref(r[0], r[1], None if mask is None else mask.double(), r[2], r[3], r[4], H, dk, hk, rate)
    (ro * G.double()).sum().backward()
    close(o, ro, "o")
    close(attn, rattn, "attn")
    for got, ref, name in zip((dqh, dbank, dwk, dwv, dbv), r, ("dqh", "dbank", "dWk", "dWv", "dbv")):
        close(got, ref.grad, name)
    if mask is not None:
        assert (dbank.cpu()[mask == 0] == 0).all(), "masked bank rows must get exactly zero"
    return (qh, bank, mask, wk, wv, bv, G), (o, attn, dqh, dwk, dwv, dbv, dbank)


# (L, H, B, (D, dk), rate, mask): every L, H, B, width pair, rate and mask kind of the sweep appears at least once; L < 8 leaves
# waves without a row, L in {63, 64, 65, 207, 208} straddles the lane / wave strides, B = 257 is one more than a full batch
CORE_CASES = [
    (1, 1, 1, (300, 128), 0.0, "none"),
    (1, 5, 2, (316, 132), 0.1, "none"),
    (2, 2, 3, (4, 4), 0.1, "ragged"),
    (2, 8, 257, (4, 4), 0.9, "first"),
    (7, 8, 2, (64, 36), 0.0, "none"),
    (7, 3, 3, (320, 128), 0.9, "last"),
    (8, 5, 2, (316, 132), 0.0, "middle"),
    (8, 8, 3, (300, 128), 1.0, "mod8"),
    (9, 7, 3, (300, 128), 0.1, "first"),
    (63, 8, 3, (64, 36), 0.1, "mod8"),
    (64, 2, 2, (320, 128), 1.0, "ragged"),
    (64, 1, 257, (64, 36), 0.0, "none"),
    (65, 5, 1, (4, 4), 0.9, "none"),
    (65, 8, 3, (300, 128), 0.9, "ragged"),
    (207, 3, 2, (316, 132), 0.1, "mod8"),
    (207, 7, 2, (300, 128), 0.0, "middle"),
    (208, 1, 3, (320, 128), 0.0, "last"),
    (208, 8, 257, (300, 128), 0.1, "ragged"),
]


@pytest.mark.parametrize("L,H,B,Ddk,rate,kind", CORE_CASES)
def test_attention_core_edges_match_fp64(L, H, B, Ddk, rate, kind):
    D, dk = Ddk
    (qh, bank, mask, wk, wv, bv, G), got = core_check(B, L, D, dk, H, rate, kind)
    # want_dbank=False skips dX only; the rerun with the same seed is bit-identical
    o, attn, _, (dqh, dwk, dwv, dbv, dbank) = run_core(qh, bank, mask, wk, wv, bv, H, dk, 5, rate, G, want_dbank=False)
    assert dbank is None
    for a, b, name in zip(got, (o, attn, dqh, dwk, dwv, dbv), ("o", "attn", "dqh", "dWk", "dWv", "dbv")):
        assert torch.equal(a, b), name + " differs on a rerun with the same seed"
    o2, attn2, _, g2 = run_core(qh, bank, mask, wk, wv, bv, H, dk, 5, rate, G)
    assert torch.equal(o2, got[0]) and torch.equal(attn2, got[1])
    for a, b in zip(got[2:], g2):
        assert torch.equal(a, b)


# ---- samples without a live position (the padded rows of a partial batch) --------------------------------------------------
@pytest.mark.parametrize("where", ["last", "middle", "all"])
def test_fully_masked_samples_contribute_nothing(where):
    B, L, D, dk, H = 6, 50, 300, 128, 4
    g, qh, bank, wk, wv, bv, G = core_inputs(B, L, D, H, dk, seed=17)
    mask = make_mask("ragged", B, L, g)
    empty = {"last": [B - 1], "middle": [2], "all": list(range(B))}[where]
    mask[empty] = 0
    live = [b for b in range(B) if b not in empty]
    o, attn, _, (dqh, dwk, dwv, dbv, dbank) = run_core(qh, bank, mask, wk, wv, bv, H, dk, 3, 0.0, G)
    for t, name in ((o, "o"), (attn, "attn"), (dqh, "dqh"), (dwk, "dWk"), (dwv, "dWv"), (dbv, "dbv"), (dbank, "dbank")):
        assert torch.isfinite(t).all(), "%s is not finite with fully masked samples (%s)" % (name, where)
    attn = attn.view(H, B, L)
    for b in empty:
        assert (o[b] == 0).all() and (attn[:, b] == 0).all() and (dbank[b] == 0).all() and (dqh[b] == 0).all()
    if live:
        sub = [t[live] for t in (qh, bank, mask)]
        so, sattn, _, (sdqh, sdwk, sdwv, sdbv, sdbank) = run_core(sub[0], sub[1], sub[2], wk, wv, bv, H, dk, 3, 0.0, G[live])
        close(o[live], so, "o")
        close(attn[:, live].reshape(-1, 1, L), sattn, "attn")
        close(dbank[live], sdbank, "dbank")
        close(dqh[live], sdqh, "dqh")
        for got, ref, name in ((dwk, sdwk, "dWk"), (dwv, sdwv, "dWv"), (dbv, sdbv, "dbv")):
            close(got, ref, name)
    else:
        for t in (dwk, dwv, dbv):
            assert (t == 0).all()
    # and against fp64 with the same rule
    core_check(B, L, D, dk, H, 0.0, None, seed=3, mask=mask)


# ---- dropout + residual + LayerNorm -----------------------------------------------------------------------------------------
def ln_ref(v, gamma, beta, eps):
    return gamma * (v - v.mean(-1, keepdim=True)) / (v.std(-1, keepdim=True) + eps) + beta


LN_CASES = [(2, 1, 0.0), (3, 3, 0.5), (63, 4, 1.0), (64, 5, 0.5), (65, 1000, 0.0), (300, 5, 0.5), (300, 1000, 1.0),
            (1000, 4, 0.5), (1024, 3, 0.0), (1024, 1000, 0.5), (2, 1000, 0.5), (65, 1, 0.5)]


@pytest.mark.parametrize("with_dy2", [False, True])
@pytest.mark.parametrize("D,rows,rate", LN_CASES)
def test_dropout_residual_layernorm_edges_match_fp64(D, rows, rate, with_dy2):
    g = torch.Generator().manual_seed(D * 7 + rows)
    x, res = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    dy, dy2 = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    # at D = 2 the normalised row is +-1/sqrt(2) whatever x is: with the model's eps = 1e-6 the gradient is eps-sized noise, so
    # that width runs with an eps that makes the gradient real
    eps, seed = (0.5 if D == 2 else 1e-6), 2 ** 62 + D
    for site in (ops.DROP_FC, ops.DROP_FFN):
        y, saved, keep = ops.dropout_residual_layernorm(x.to(DEV), res.to(DEV), gamma.to(DEV), beta.to(DEV), eps, seed, site, rate,
                                                        return_masks=True)
        hk = torch.from_numpy(DR.rows_keep(seed, site, rate, rows, D))
        assert torch.equal(keep.cpu(), hk), "LayerNorm keep mask (site %d) differs from the host restatement" % site
        dres, dx, dg, db = ops.dropout_residual_layernorm_backward(dy.to(DEV), gamma.to(DEV), saved,
                                                                   dy2=dy2.to(DEV) if with_dy2 else None)
        r = [t.double().requires_grad_(True) for t in (x, res, gamma, beta)]
        ry = ln_ref(drop(r[0], hk, rate) + r[1], r[2], r[3], eps)
        up = dy.double() + (dy2.double() if with_dy2 else 0.0)
        (ry * up).sum().backward()
        close(y, ry, "y")
        for got, ref, name in ((dx, r[0].grad, "dx"), (dres, r[1].grad, "dres"), (dg, r[2].grad, "dgamma"),
                               (db, r[3].grad, "dbeta")):
            close(got, ref, name)
        if rate > 0:
            assert (dx.cpu()[~hk] == 0).all()


# ---- weight gradient --------------------------------------------------------------------------------------------------------
WGRAD_CASES = [(0, (63, 65), True), (0, (300, 1024), False), (1, (1, 1), True), (15, (63, 65), False), (16, (64, 64), True),
               (17, (300, 1024), True), (63, (1, 1), False), (64, (63, 65), True), (65, (64, 64), False),
               (1023, (300, 1024), True), (1024, (63, 65), True), (1025, (64, 64), True), (1025, (1, 1), False),
               (100000, (63, 65), True), (100000, (1, 1), False)]


@pytest.mark.parametrize("M,NK,bias", WGRAD_CASES)
def test_wgrad_edges_match_fp64(M, NK, bias):
    N, K = NK
    g = torch.Generator().manual_seed(M + N + K)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    dW, db = ops.wgrad(dy.to(DEV), x.to(DEV), bias=bias)
    assert (db is not None) == bias
    if M == 0:
        assert (dW == 0).all() and (db is None or (db == 0).all())
        return
    close(dW, dy.double().t() @ x.double(), "dW", tol=1e-5)
    if bias:
        close(db, dy.double().sum(0), "db", tol=1e-5)
    dW2, db2 = ops.wgrad(dy.to(DEV), x.to(DEV), bias=bias)
    assert torch.equal(dW, dW2) and (not bias or torch.equal(db, db2))


# ---- image-bank weight gradient ---------------------------------------------------------------------------------------------
# (B, K, P, N); direct: B*P <= 32 (one slab, the kernel writes dW and db itself)
BANK_CASES = [(1, 15, 1, 16, True), (1, 128, 32, 320, True), (2, 129, 16, 1, True), (2, 1, 16, 319, True),
              (64, 300, 196, 300, False), (3, 1, 49, 320, False), (5, 127, 7, 16, False), (4, 129, 33, 319, False),
              (0, 128, 196, 300, False)]


@pytest.mark.parametrize("B,K,P,N,direct", BANK_CASES)
def test_imgbank_wgrad_edges_match_fp64(B, K, P, N, direct):
    assert B == 0 or (B * P <= 32) == direct, "the case must stay on the path it is named for"
    g = torch.Generator().manual_seed(B * 31 + K + P + N)
    X = torch.rand(B, K, P, generator=g)
    dbank = torch.randn(B, P, N, generator=g)
    dW, db = ops.imgbank_wgrad(X.to(DEV), dbank.to(DEV))
    if B == 0:
        assert dW.shape == (N, K) and (dW == 0).all() and (db == 0).all()
        return
    close(dW, torch.einsum("bpo,bcp->oc", dbank.double(), X.double()), "dW")
    close(db, dbank.double().sum(dim=(0, 1)), "db")
    dW2, db2 = ops.imgbank_wgrad(X.to(DEV), dbank.to(DEV))
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


# ---- label attention --------------------------------------------------------------------------------------------------------
def label_ref(Q, K, V, H, keep, rate):
    NLQ, hid = Q.shape
    B, dh = K.shape[0], hid // H
    att = torch.softmax(Q.view(1, NLQ, H, dh) * K.view(B, 1, H, dh) / math.sqrt(dh), dim=-1)
    att = drop(att, keep.view(B, NLQ, H, dh), rate)
    return (att * V.view(B, 1, H, dh)).reshape(B, NLQ, hid)


# (B, H, dh, NLQ, rate): B*H not a multiple of 4 (a partial last workgroup), dh from 1 to 64, NLQ from 1
LABEL_CASES = [(3, 5, 60, 7, 0.5), (1, 1, 64, 1, 0.0), (7, 3, 1, 33, 0.5), (5, 1, 7, 7, 1.0), (2, 3, 64, 33, 0.0),
               (64, 5, 60, 1, 0.5), (3, 7, 7, 33, 1.0), (0, 5, 60, 7, 0.5)]


@pytest.mark.parametrize("B,H,dh,NLQ,rate", LABEL_CASES)
def test_label_attention_edges_match_fp64(B, H, dh, NLQ, rate):
    hid = H * dh
    g = torch.Generator().manual_seed(B * 101 + H * 11 + dh + NLQ)
    Q, K, V = torch.randn(NLQ, hid, generator=g), torch.randn(B, hid, generator=g), torch.randn(B, hid, generator=g)
    G = torch.randn(B, NLQ, hid, generator=g)
    seed = 2 ** 64 - 1 - B
    x, saved, keep = ops.label_attn_train(Q.to(DEV), K.to(DEV), V.to(DEV), H, seed, rate, return_masks=True)
    dQ, dK, dV = ops.label_attn_train_backward(G.to(DEV), Q.to(DEV), K.to(DEV), V.to(DEV), saved)
    if B == 0:
        assert x.shape == (0, NLQ, hid) and dQ.shape == (NLQ, hid) and (dQ == 0).all()
        return
    hk = torch.from_numpy(DR.label_keep(seed, rate, B, NLQ, hid))
    assert torch.equal(keep.cpu(), hk), "label attention keep mask differs from the host restatement"
    r = [t.double().requires_grad_(True) for t in (Q, K, V)]
    ref = label_ref(r[0], r[1], r[2], H, hk, rate)
    (ref * G.double()).sum().backward()
    close(x, ref, "x")
    for got, ref_, name in zip((dQ, dK, dV), r, ("dQ", "dK", "dV")):
        close(got, ref_.grad, name)
    x2, saved2 = ops.label_attn_train(Q.to(DEV), K.to(DEV), V.to(DEV), H, seed, rate)
    assert torch.equal(x, x2)
    assert all(torch.equal(a, b) for a, b in zip((dQ, dK, dV), ops.label_attn_train_backward(G.to(DEV), Q.to(DEV), K.to(DEV),
                                                                                          V.to(DEV), saved2)))


# ---- every kernel's applied mask is the host restatement's, bit for bit ----------------------------------------------------
SEEDS = [0, 1, 2 ** 62 - 1, 2 ** 64 - 1]


@pytest.mark.parametrize("seed", SEEDS)
def test_applied_masks_equal_the_host_restatement(seed):
    H, B, L, rate = 8, 37, 13, 0.5
    g = torch.Generator().manual_seed(seed % 1000)
    # attention core: the head index is part of the counter ((h*B + b)*L + l), so no two heads share a mask
    qh, bank = torch.randn(B, H * 4, generator=g).to(DEV), torch.randn(B, L, 16, generator=g).to(DEV)
    wk, wv, bv = (torch.randn(H * 4, 16, generator=g).to(DEV), torch.randn(H * 4, 16, generator=g).to(DEV),
                  torch.randn(H * 4, generator=g).to(DEV))
    _, attn, saved, keep = ops.mha_attn_train(qh, bank, None, H, 4, wk, wv, bv, seed, rate, return_masks=True)
    hk = host_attn_keep(seed, rate, H, B, L)
    assert torch.equal(keep.cpu(), hk)
    assert torch.equal((attn != 0).cpu(), hk)                              # applied: every unmasked probability is > 0
    assert torch.equal(saved["attn"].cpu(), (saved["P"].view(H * B, 1, L) * 2.0 * hk.to(DEV)).cpu())
    # dropout + residual + LayerNorm at both of its sites
    D = 48
    x, res = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    one, zero = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    for site in (ops.DROP_FC, ops.DROP_FFN):
        _, saved_ln, keep = ops.dropout_residual_layernorm(x, res, one, zero, 1e-6, seed, site, rate, return_masks=True)
        hk = torch.from_numpy(DR.rows_keep(seed, site, rate, B, D))
        assert torch.equal(keep.cpu(), hk)
        _, dx, _, _ = ops.dropout_residual_layernorm_backward(torch.randn(B, D, generator=g).to(DEV), one, saved_ln)
        assert not dx.cpu()[~hk].any()
    # label attention
    NLQ, dh = 13, 8
    Q, K, V = (torch.randn(NLQ, H * dh, generator=g).to(DEV), torch.randn(B, H * dh, generator=g).to(DEV),
               torch.randn(B, H * dh, generator=g).to(DEV))
    xl, _, keep = ops.label_attn_train(Q, K, V, H, seed, rate, return_masks=True)
    hk = torch.from_numpy(DR.label_keep(seed, rate, B, NLQ, H * dh))
    assert torch.equal(keep.cpu(), hk)
    assert torch.equal((xl != 0).cpu(), hk)
    # plain dropout and the mask generator, every site
    xd = torch.randn(B, L * H, generator=g).to(DEV)
    y, _, keep = ops.dropout(xd, seed, ops.DROP_HEAD, rate, return_masks=True)
    hk = torch.from_numpy(DR.rows_keep(seed, DR.DROP_HEAD, rate, B, L * H))
    assert torch.equal(keep.cpu(), hk)
    assert torch.equal(y.cpu(), torch.where(hk, xd.cpu() * float(DR.scale(rate)), torch.zeros(())))
    for site in DR.SITES:
        for r in (0.1, 0.9):
            got = ops.dropout_mask(seed, site, r, (H * B, 1, L), DEV).cpu()
            assert torch.equal(got, torch.from_numpy(DR.keep(seed, site, DR.attn_index(H, B, L), r).reshape(H * B, 1, L)))


def test_rates_below_2_pow_minus_24_on_the_device():
    idx = 4321
    zero = DR.seed_for(DR.DROP_FC, idx, 0x00000000FFFFFFFF)        # u == 0 exactly at idx
    for rate, dropped in ((2.0 ** -25, True), (1e-30, True), (0.0, False), (1e-46, False)):
        got = ops.dropout_mask(zero, DR.DROP_FC, rate, (5000,), DEV).cpu()
        assert bool(got[idx]) != dropped, rate
        assert int(got.sum()) == 5000 - int(dropped)
    half = DR.seed_for(DR.DROP_ATTN, 99, 1 << 63)                    # u == 0.5 exactly: kept at rate 0.5
    assert bool(ops.dropout_mask(half, DR.DROP_ATTN, 0.5, (100,), DEV).cpu()[99])


# ---- refusals at each limit + 1 -----------------------------------------------------------------------------------------------
def test_refusals_at_each_limit_plus_one():
    def core(B=2, L=8, D=16, H=2, dk=4, rate=0.1):
        z = torch.zeros
        ops.mha_attn_train(z(B, H * dk, device=DEV), z(B, L, D, device=DEV), None, H, dk, z(H * dk, D, device=DEV),
                           z(H * dk, D, device=DEV), z(H * dk, device=DEV), 1, rate)

    core()
    for kw in (dict(L=209), dict(D=324), dict(D=18), dict(H=9), dict(dk=130), dict(rate=1.5), dict(rate=-0.1)):
        with pytest.raises(ValueError):
            core(**kw)

    def ln(D, rate=0.1):
        x = torch.zeros(4, D, device=DEV)
        ops.dropout_residual_layernorm(x, x, torch.ones(D, device=DEV), torch.zeros(D, device=DEV), 1e-6, 1, ops.DROP_FC, rate)

    ln(2)
    ln(1024)
    for D in (1, 1025):
        with pytest.raises(RuntimeError, match="out of range"):
            ln(D)
    with pytest.raises(ValueError, match="outside"):
        ln(8, rate=1.01)

    def label(dh, rate=0.1):
        Q, K = torch.zeros(3, 2 * dh, device=DEV), torch.zeros(2, 2 * dh, device=DEV)
        ops.label_attn_train(Q, K, K, 2, 1, rate)

    label(64)
    with pytest.raises(ValueError, match="64"):
        label(65)
    with pytest.raises(ValueError, match="outside"):
        label(8, rate=-1e-3)
    ops.imgbank_wgrad(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 4, 320, device=DEV))
    with pytest.raises(RuntimeError, match="N <= 320"):
        ops.imgbank_wgrad(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 4, 321, device=DEV))
    for bad in (1.5, -0.5):
        with pytest.raises(ValueError, match="outside"):
            ops.dropout(torch.zeros(8, device=DEV), 1, ops.DROP_HEAD, bad)
        with pytest.raises(ValueError, match="outside"):
            ops.dropout_mask(1, ops.DROP_HEAD, bad, (8,), DEV)
    torch.cuda.synchronize()                     # nothing was launched out of range: the device is still healthy
    core()
    torch.cuda.synchronize()
