"""Edge sweeps of the exact-fp32 forward kernels, each through its ops.* wrapper, against the plain float64 references of
tests/forward_ref.py (pinned to the goldens by tests/test_forward_ref_cpu.py).  The grids are hand-picked cases, not cross products:
every value of every axis appears, and the cases sit where a kernel's partition changes (the attention core's tile-count classes
1 | 2 | 4 | 7 | 10 | 13, the 20-wide slices of the model dim, the <5> / <16> builds of the row operators, 16-row tiles, the grid cap of
the gather).

Tolerances: bit-exact where the operation is a copy, a max, a count or an arg-max; otherwise the bound the suite asserts for the same
kernel at its golden shape (ATTN, OUT_REL, LINEAR, LAYER, LN, LSTM below).  A case that carries a bound of its own names, in the comment
beside it, the error of the same reference evaluated in float32 on the CPU against float64 (`fp32_cpu_err`, printed by every test): the
bound is 4 x that figure -- the kernel rounds as often as the float32 reference, in another order."""
import itertools
import math

import numpy as np
import pytest
import torch

from mgnns_amd import metrics, ops
from oracle import restatement as R
from tests import forward_ref as F
from tests.helpers import close, core_case, f32, f64, fp32_cpu_err, make_mask, maxerr, scale  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ATTN = 1e-5        # attention probabilities, absolute
# |sum of a probability row - 1|: the float32 probabilities of the float32 reference, summed in float64, are off by at most ROWSUM_FP32
# over the attention cases below (largest at L = 208: 1.44e-7 on one host, 1.50e-7 on another -- torch's float32 reductions depend on
# the CPU; every test prints its own figure); the bound is 4 x that
ROWSUM_FP32 = 1.5e-7
ROWSUM = 4 * ROWSUM_FP32
OUT_REL = 1e-5     # attention output and image bank, relative to the output's largest magnitude
LINEAR = 2e-6      # linear / matmul / classifier head, relative to the output's largest magnitude
LAYER = 2e-5       # layer output behind two LayerNorms, absolute
LN = 2e-6          # LayerNorm, absolute
LSTM = 5e-6        # text bank, absolute
PROBS = 1e-6       # softmax of the logits, absolute


def dev(x):
    return None if x is None else torch.as_tensor(x).to(DEV).contiguous()


# ---- attention core -----------------------------------------------------------------------------------------------------------
def check_attention(o, attn, ro, rattn, mask, H, B, L, what):
    assert tuple(attn.shape) == (H * B, 1, L) and tuple(o.shape) == tuple(ro.shape)
    close(attn, rattn, ATTN, what + " attn")                    # the reference is head-major: row h * B + b
    close(o, ro, OUT_REL, what + " o", rel=True)
    a = attn.cpu().view(H, B, L)
    if mask is not None:
        assert (a[:, mask == 0] == 0).all(), "masked positions must carry exactly zero probability"
    close(a.double().sum(-1), torch.ones(H, B, dtype=torch.float64), ROWSUM, what + " row sums")


def rowsum_fp32_cpu_err(ref, args):
    """|row sum - 1| of the float32 reference's probabilities (summed in float64)."""
    p = ref(*f32(args))[1]
    return float((p.double().sum(-1) - 1).abs().max()) if p.numel() else 0.0


# (L, D, H, B, mask, biases): L on both sides of every tile-count class of the core (1 | 2 | 4 | 7 | 10 | 13 tiles of 16 rows);
# D = 4, 20, 24 (one slice, exactly one, one and a 4-wide tail), 316 (a 16-wide tail), 300, 320.  The class taken follows the last
# live position of a SAMPLE: "none" takes the class of L itself; "ragged" and "single" (B > 1) keep sample 0 at full length and
# "holes" keeps the last position of every sample live, so these reach the class of L as well, next to the smaller ones of the
# shorter samples; "holes" ends with a sample whose only live row is the last row of the last tile
CORE_CASES = [
    (1, 300, 8, 1, "none", True),
    (1, 4, 1, 1, "single", True),
    (15, 4, 1, 5, "ragged", True),
    (16, 20, 3, 1, "tile", False),
    (17, 24, 16, 5, "holes", True),
    (32, 316, 3, 5, "tile", True),
    (17, 300, 3, 1, "none", True),
    (33, 320, 1, 5, "holes", False),
    (33, 300, 3, 1, "none", True),
    (64, 300, 8, 5, "ragged", False),
    (65, 20, 16, 1, "none", True),
    (112, 24, 3, 5, "holes", False),
    (113, 316, 8, 5, "single", True),
    (113, 300, 3, 1, "none", False),
    (161, 300, 3, 1, "none", True),
    (160, 4, 16, 5, "tile", True),
    (161, 320, 3, 5, "ragged", True),
    (207, 300, 1, 5, "holes", True),
    (208, 320, 16, 5, "none", False),
    (208, 300, 8, 5, "single", True),
    (100, 300, 8, 0, "ragged", True),
]


@pytest.mark.parametrize("L,D,H,B,kind,bias", CORE_CASES)
def test_sq_mha_core_edges_match_fp64(L, D, H, B, kind, bias):
    qh, bank, mask, wk, bk, wv, bv = core_case(L, D, H, B, kind, bias)
    ref = lambda *a: F.sq_mha_core(a[0], a[1], a[2], H, 128, *a[3:])
    args = f64([qh, bank, mask, wk, bk, wv, bv])
    print("fp32-CPU error (o, attn):", fp32_cpu_err(ref, *args), "row sums:", rowsum_fp32_cpu_err(ref, args))
    ro, rattn = ref(*args)
    d = [dev(t) for t in (qh, bank, mask, wk, bk, wv, bv)]
    o, attn = ops.sq_mha_core(d[0], d[1], d[2], H, 128, d[3], d[4], d[5], d[6])
    check_attention(o, attn, ro, rattn, mask, H, B, L, "core")
    o2, none = ops.sq_mha_core(d[0], d[1], d[2], H, 128, d[3], d[4], d[5], d[6], want_attn=False)
    assert none is None and torch.equal(o2, o)


@pytest.mark.parametrize("L,H,dead", [(16, 3, 0), (100, 8, 2), (208, 1, 4)])
def test_sq_mha_core_fully_masked_sample_is_nan_and_leaves_the_others_alone(L, H, dead):
    """A sample without a live position: NaN probabilities like the reference's softmax over -inf, an output row of exact zeros (no
    bank row is weighted), and every other sample bit-equal to the same batch run without it."""
    qh, bank, mask, wk, bk, wv, bv = core_case(L, 300, H, 5, "ragged", True)
    mask[dead] = 0
    d = [dev(t) for t in (qh, bank, mask, wk, bk, wv, bv)]
    o, attn = ops.sq_mha_core(d[0], d[1], d[2], H, 128, d[3], d[4], d[5], d[6])
    a = attn.view(H, 5, L)
    assert torch.isnan(a[:, dead]).all() and (o[dead] == 0).all()
    keep = [b for b in range(5) if b != dead]
    o4, attn4 = ops.sq_mha_core(d[0][keep].contiguous(), d[1][keep].contiguous(), d[2][keep].contiguous(), H, 128, d[3], d[4], d[5], d[6])
    assert torch.equal(o[keep], o4) and torch.equal(a[:, keep], attn4.view(H, 4, L))
    _, rattn = F.sq_mha_core(*f64([qh, bank, mask]), H, 128, *f64([wk, bk, wv, bv]))
    assert torch.isnan(rattn.view(H, 5, L)[:, dead]).all()


# (L, dk, D, H, B, bank, mask): bank "f32" | "bf16" (row stride D) | "bf16_320" (row stride 320, zero padded)
FOLDED_CASES = [
    (1, 128, 300, 8, 3, "f32", "none"),
    (16, 4, 4, 1, 2, "f32", "tile"),
    (17, 64, 300, 5, 2, "bf16", "ragged"),
    (32, 132, 320, 8, 3, "bf16_320", "holes"),
    (33, 4, 300, 5, 1, "bf16_320", "none"),
    (64, 128, 4, 8, 2, "bf16", "single"),
    (65, 132, 300, 1, 3, "f32", "holes"),
    (112, 64, 320, 5, 2, "f32", "ragged"),
    (113, 128, 4, 1, 3, "bf16_320", "tile"),
    (160, 4, 320, 8, 2, "bf16", "none"),
    (161, 132, 300, 5, 3, "bf16_320", "single"),
    (208, 64, 300, 8, 2, "f32", "tile"),
    (208, 128, 320, 1, 5, "bf16", "ragged"),
    (100, 128, 300, 8, 0, "f32", "ragged"),
]


@pytest.mark.parametrize("L,dk,D,H,B,bankk,kind", FOLDED_CASES)
def test_sq_mha_folded_edges_match_fp64(L, dk, D, H, B, bankk, kind):
    """The folded kernel against float64 of the UNFOLDED formula (b_k drops out of the softmax); a bf16 bank is judged on its own
    rounded values."""
    qh, bank, mask, wk, _, wv, bv = core_case(L, D, H, B, kind, True, dk=dk)
    if bankk == "f32":
        dbank = dev(bank)
    else:
        ld = D if bankk == "bf16" else 320
        padded = torch.zeros(B, L, ld, dtype=torch.bfloat16)
        padded[..., :D] = bank.bfloat16()
        bank, dbank = padded[..., :D].float(), dev(padded)
    ref = lambda *a: F.sq_mha_core(a[0], a[1], a[2], H, dk, a[3], None, a[4], a[5])
    args = f64([qh, bank, mask, wk, wv, bv])
    print("fp32-CPU error (o, attn):", fp32_cpu_err(ref, *args), "row sums:", rowsum_fp32_cpu_err(ref, args))
    ro, rattn = ref(*args)
    d = [dev(t) for t in (qh, mask, wk, wv, bv)]
    o, attn = ops.sq_mha_folded(d[0], dbank, d[1], H, dk, d[2], d[3], d[4])
    check_attention(o, attn, ro, rattn, mask, H, B, L, "folded")
    o2, none = ops.sq_mha_folded(d[0], dbank, d[1], H, dk, d[2], d[3], d[4], want_attn=False)
    assert none is None and torch.equal(o2, o)


# ---- rest of the layer ----------------------------------------------------------------------------------------------------------
def tail_case(HK, B, HK_next):
    rs = np.random.RandomState(HK * 3 + B)
    n = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    w = {"fc_w": n(300, HK) / math.sqrt(HK), "fc_b": 0.1 * n(300), "g1": 1 + 0.1 * n(300), "be1": 0.1 * n(300),
         "w1": n(300, 300) / math.sqrt(300), "b1": 0.1 * n(300), "w2": n(300, 300) / math.sqrt(300), "b2": 0.1 * n(300),
         "g2": 1 + 0.1 * n(300), "be2": 0.1 * n(300)}
    nxt = (n(HK_next, 300) / math.sqrt(300), 0.1 * n(HK_next)) if HK_next else None
    return n(B, HK), 0.8 * n(B, 300), w, nxt


# (HK, B, HK_next or 0): 1888 is the widest o whose 16-row tile fits the 160 KiB of LDS next to the activation tiles
TAIL_CASES = [(4, 1, 0), (4, 257, 128), (128, 3, 0), (128, 4, 512), (300, 5, 4), (300, 0, 128), (1884, 5, 300), (1888, 4, 0),
              (1888, 257, 1024), (1024, 1, 2048)]


@pytest.mark.parametrize("HK,B,HK_next", TAIL_CASES)
def test_mha_tail_edges_match_fp64_and_the_operator_chain(HK, B, HK_next):
    o, q, w, nxt = tail_case(HK, B, HK_next)
    ref = lambda o_, q_, w_, n_: F.mha_tail(o_, q_, w_, 1e-6, n_)
    args = f64([o, q, w, nxt])
    print("fp32-CPU error (out, qh_next):", fp32_cpu_err(ref, *args))
    rout, rqh = ref(*args)
    d = {k: dev(v) for k, v in w.items()}
    packed = {"fc_wp": ops.pack_weight_f32(d["fc_w"]), "w1_wp": ops.pack_weight_f32(d["w1"]), "w2_wp": ops.pack_weight_f32(d["w2"])}
    packed.update({k: d[k] for k in ("fc_b", "g1", "be1", "b1", "b2", "g2", "be2")})
    np_ = None if nxt is None else (ops.pack_weight_f32(dev(nxt[0])), dev(nxt[1]), HK_next)
    out, qh = ops.mha_tail(dev(o), dev(q), packed, 1e-6, np_)
    close(out, rout, LAYER, "tail out")
    # the same layer as separate launches, the way the golden tests finish it
    y = ops.layernorm(ops.linear(dev(o), d["fc_w"], d["fc_b"], residual=dev(q)), d["g1"], d["be1"])
    z = ops.linear(ops.linear(y, d["w1"], d["b1"], act=ops.ACT_RELU), d["w2"], d["b2"], residual=y)
    chain = ops.layernorm(z, d["g2"], d["be2"])
    close(chain, rout, LAYER, "chain out")
    close(out, chain.cpu(), 2 * LAYER, "tail out vs chain")             # both within LAYER of float64
    if nxt is None:
        assert qh is None
    else:
        # the projection is judged on the kernel's own `out` (itself held to LAYER above), in float64, at the linear bound
        assert tuple(qh.shape) == tuple(rqh.shape)
        close(qh, F.linear(out.cpu().double(), *f64(list(nxt))), LINEAR, "tail qh_next vs fp64 linear(out)", rel=True)
        close(qh, ops.linear(out, dev(nxt[0]), dev(nxt[1])).cpu(), LINEAR, "tail qh_next vs linear(out)", rel=True)


def ln_case(D, rows, kind):
    """Rows of standard deviation 0.15 .. 3 (so the reference is well conditioned); "bigmean": mean 1e3, std 1."""
    rs = np.random.RandomState(D * 7 + rows)
    x = rs.standard_normal((rows, D))
    if rows:
        x = (x - x.mean(1, keepdims=True)) / x.std(1, ddof=1, keepdims=True)
        x = x * (1.0 if kind == "bigmean" else rs.uniform(0.15, 3.0, size=(rows, 1))) + (1e3 if kind == "bigmean" else rs.standard_normal((rows, 1)))
    n = lambda s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    return torch.from_numpy(x.astype(np.float32)), 1 + 0.1 * n(D), 0.1 * n(D)


# (D, rows, kind, eps, bound): D on both sides of 64 (one lane stride), of 320 | 321 (the <5> | <16> builds) and at 2 and 1024
LN_CASES = [
    (2, 1, "plain", 1e-6, LN), (3, 3, "plain", 1e-6, LN), (63, 4, "plain", 1e-3, LN), (64, 5, "plain", 1e-6, LN),
    (65, 1025, "plain", 1e-6, LN), (300, 0, "plain", 1e-6, LN), (300, 5, "plain", 1e-2, LN), (320, 5, "plain", 1e-6, LN),
    (321, 4, "plain", 1e-6, LN), (512, 3, "plain", 1e-3, LN), (1023, 1, "plain", 1e-6, LN), (1024, 1025, "plain", 1e-6, LN),
    # mean 1e3, std 1: the inputs carry 6e-5 of rounding each, which the float32 mean keeps; a one-pass variance would be off by O(1)
    # (the row sum of D values near 1e3 is rounded to a float32 whose half ulp, divided by D, is already 4e-5 of a unit std)
    (2, 4, "bigmean", 1e-6, LN),                 # fp32-CPU error 5.7e-8: the suite's bound holds
    (65, 5, "bigmean", 1e-6, 3.0e-4),            # fp32-CPU error 7.5e-5 -> 4 x = 3.0e-4
    (320, 5, "bigmean", 1e-6, 6.3e-4),           # fp32-CPU error 1.57e-4 -> 4 x = 6.3e-4
    (321, 4, "bigmean", 1e-6, 6.4e-4),           # fp32-CPU error 1.60e-4 -> 4 x = 6.4e-4
    (1024, 5, "bigmean", 1e-3, 3.2e-4),          # fp32-CPU error 8.1e-5 -> 4 x = 3.2e-4
]


@pytest.mark.parametrize("D,rows,kind,eps,bound", LN_CASES)
def test_layernorm_edges_match_fp64(D, rows, kind, eps, bound):
    x, g, b = ln_case(D, rows, kind)
    ref = lambda x_, g_, b_: F.layer_norm(x_, g_, b_, eps)
    args = f64([x, g, b])
    if rows:
        assert float(args[0].std(-1).min()) >= 0.1, "the reference needs rows of standard deviation >= 0.1"
    print("fp32-CPU error:", fp32_cpu_err(ref, *args))
    y = ops.layernorm(dev(x), dev(g), dev(b), eps)
    close(y, ref(*args), bound, "layernorm D=%d" % D)


@pytest.mark.parametrize("D", [2, 300, 321, 1024])
def test_layernorm_constant_row_stays_bounded(D):
    """(x - mean) / (std + eps) of a constant row is 0 / 0-like in the reference itself: only boundedness is comparable."""
    _, g, b = ln_case(D, 1, "plain")
    y = ops.layernorm(dev(torch.full((3, D), 0.37)), dev(g), dev(b)).cpu()
    assert torch.isfinite(y).all()
    assert float((y - b).abs().max()) <= float(g.abs().max()) * D ** 0.5


def head_case(D, NL, B):
    rs = np.random.RandomState(D + 11 * NL + B)
    feats = [torch.from_numpy(rs.standard_normal((B, D)).astype(np.float32)) for _ in range(4)]
    w = torch.from_numpy((rs.standard_normal((NL, 4 * D)) / math.sqrt(4 * D)).astype(np.float32))
    return feats, w, torch.from_numpy(rs.standard_normal(NL).astype(np.float32))


# (D, NL, B): D = 320 | 321 are the two sides of the <5> | <16> builds
HEAD_CASES = [(1, 1, 1), (4, 3, 4), (300, 7, 259), (320, 64, 5), (321, 3, 5), (1024, 7, 4), (1024, 64, 1), (300, 3, 0), (321, 1, 259)]


@pytest.mark.parametrize("D,NL,B", HEAD_CASES)
def test_classifier_head_edges_match_fp64(D, NL, B):
    feats, w, b = head_case(D, NL, B)
    args = f64([feats, w, b])
    print("fp32-CPU error:", fp32_cpu_err(F.classifier_head, *args))
    y = ops.classifier_head([dev(f) for f in feats], dev(w), dev(b))
    assert tuple(y.shape) == (B, NL)
    close(y, F.classifier_head(*args), LINEAR, "classifier head", rel=True)


@pytest.mark.parametrize("D,NL,B", HEAD_CASES)
def test_classifier_head_part_every_order_of_arrival(D, NL, B):
    """The four shares in all 24 orders: the last arriver adds the parts in index order, so every order gives the same bits."""
    feats, w, b = head_case(D, NL, B)
    ref = F.classifier_head(*f64([feats, w, b]))
    df, dw, db = [dev(f) for f in feats], dev(w), dev(b)
    first = None
    for order in itertools.permutations(range(4)):
        state = ops.classifier_head_state(B, NL, 4, DEV)
        for part in order:
            logits = ops.classifier_head_part(df[part], part, 4, dw, db, state)
        assert int(state[1].item()) == 0, "the arrival counter must be re-armed"
        if first is None:
            first = logits.clone()
            close(first, ref, LINEAR, "classifier parts", rel=True)
        assert torch.equal(logits, first), order


# ---- image bank -----------------------------------------------------------------------------------------------------------------
# (P, N, K, B)
IMG_CASES = [(4, 1, 16, 1), (100, 4, 48, 2), (196, 300, 2048, 1), (204, 17, 48, 7), (208, 304, 2048, 2), (208, 300, 16, 0),
             (4, 304, 48, 2), (196, 300, 48, 7)]


@pytest.mark.parametrize("P,N,K,B", IMG_CASES)
def test_imgbank_pool_edges_match_fp64(P, N, K, B):
    rs = np.random.RandomState(P + N + K + B)
    feat = rs.standard_normal((B, K, P)).astype(np.float32)               # negative values: the trunk's ReLU is not assumed
    feat[:, ::3] = -np.abs(feat[:, ::3]) - 0.5                               # all-negative feature rows: a zero-initialised max fails
    w = (0.05 * rs.standard_normal((N, K))).astype(np.float32)
    bias = (0.05 * rs.standard_normal(N)).astype(np.float32)
    args = f64([feat, w, bias])
    print("fp32-CPU error (bank, pooled):", fp32_cpu_err(F.imgbank_pool, *args))
    rbank, rpool = F.imgbank_pool(*args)
    wt = ops.transpose_pad(dev(w), ops.IMGBANK_LDW)
    bank, pooled = ops.imgbank_pool(dev(feat), wt, dev(bias), N)
    close(bank, rbank, OUT_REL, "image bank", rel=True)
    assert torch.equal(pooled.cpu().double(), rpool), "the pooled max is exact"
    bank2, none = ops.imgbank_pool(dev(feat), wt, dev(bias), N, want_pool=False)
    assert none is None and torch.equal(bank2, bank)
    bank3, _ = ops.imgbank_pool(dev(feat), wt, None, N)
    close(bank3, F.imgbank_pool(args[0], args[1], None)[0], OUT_REL, "image bank without bias", rel=True)


# ---- label attention core -------------------------------------------------------------------------------------------------------
# (dh, heads, NLQ, B)
LABEL_CASES = [(1, 1, 1, 1), (7, 5, 3, 6), (60, 5, 11, 6), (64, 8, 3, 1), (64, 1, 11, 6), (60, 8, 1, 0), (1, 8, 11, 6)]


@pytest.mark.parametrize("mask_kind", ["none", "random", "row"])
@pytest.mark.parametrize("dh,heads,NLQ,B", LABEL_CASES)
def test_label_attn_core_edges_match_fp64(dh, heads, NLQ, B, mask_kind):
    rs = np.random.RandomState(dh + 3 * heads + NLQ + B)
    hid = heads * dh
    Q = torch.from_numpy(rs.standard_normal((NLQ, hid)).astype(np.float32))
    K = torch.from_numpy((3.0 * rs.standard_normal((B, hid))).astype(np.float32))
    V = torch.from_numpy(rs.standard_normal((B, hid)).astype(np.float32))
    mask = None
    if mask_kind != "none":
        mask = torch.from_numpy((rs.uniform(size=(B, NLQ, heads, dh)) > 0.3).astype(np.float32))
        if mask_kind == "row" and B:
            mask[B - 1, NLQ - 1, heads - 1] = 0          # every feature of one head masked: a uniform softmax through the -1e10 fill
    ref = lambda q, k, v, m: F.label_attn_core(q, k, v, heads, m)
    args = f64([Q, K, V, mask])
    print("fp32-CPU error:", fp32_cpu_err(ref, *args))
    r = ref(*args)
    x = ops.label_attn_core(dev(Q), dev(K), dev(V), heads, dev(mask))
    assert tuple(x.shape) == (B, NLQ, hid)
    close(x, r, LINEAR, "label attention core", rel=True)
    if mask_kind == "row" and B:
        got = x[B - 1, NLQ - 1, (heads - 1) * dh:].cpu().double()
        close(got, f64(V)[B - 1, (heads - 1) * dh:] / dh, LINEAR, "all-masked head is uniform", rel=True)


# ---- head difference ------------------------------------------------------------------------------------------------------------
# (H, dv, B)
HEAD_DIFF_CASES = [(1, 1, 1), (2, 63, 5), (3, 64, 5), (16, 65, 1), (2, 128, 0), (16, 300, 5), (3, 1, 5), (16, 128, 5)]


@pytest.mark.parametrize("H,dv,B", HEAD_DIFF_CASES)
def test_head_diff_edges_match_fp64(H, dv, B):
    rs = np.random.RandomState(H + dv + B)
    o = rs.standard_normal((B, H, dv)).astype(np.float32)
    if B > 1:
        o[1, H - 1] = 0                                  # a zero head vector: F.normalize's 1e-12 clamp, cosines of exactly 0
    got = ops.head_diff(dev(o.reshape(B, H * dv)), H)
    assert tuple(got.shape) == (B,)
    if H == 1:
        assert torch.isnan(got).all()                    # 0 / 0, like the reference
        assert torch.isnan(F.head_diff(f64(o))).all()
        return
    print("fp32-CPU error:", fp32_cpu_err(F.head_diff, f64(o)))
    close(got, F.head_diff(f64(o)), 1e-6, "head difference")


# ---- evaluation tail ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NL,B", [(1, 1), (2, 1000), (3, 1), (3, 5), (64, 1000), (3, 0), (64, 1), (2, 1), (1, 1000)])
def test_softmax_argmax_edges(NL, B):
    rs = np.random.RandomState(NL + B)
    logits = (2.0 * rs.standard_normal((B, NL))).astype(np.float32)
    if B >= 4 and NL >= 2:
        logits[0] = 1.5                                  # every label tied: index 0
        first = NL // 2 if NL > 2 else 0
        logits[1, NL - 1] = logits[1, first] = logits[1].max() + 1.0        # two exact maxima: the first wins
        logits[2] = -80.0
        logits[2, NL - 1] = 80.0                         # exp(160) overflows float32 unless the maximum is subtracted
        logits[3] = 80.0
        logits[3, 0] = -80.0
    target = rs.randint(0, NL, size=B).astype(np.int64)
    rprobs, rpred = F.softmax_argmax(f64(logits))
    probs, pred = metrics.predict(dev(logits))
    close(probs, rprobs, PROBS, "softmax")
    assert torch.equal(pred.cpu().long(), torch.argmax(probs.cpu(), dim=1)), "arg-max of the kernel's own probabilities, first index"
    # independent of the kernel: the first arg-max of the float32 logits, and the float64 reference's
    assert torch.equal(pred.cpu().long(), torch.from_numpy(logits).argmax(dim=1))
    assert torch.equal(pred.cpu().long(), rpred)
    if B >= 4 and NL >= 2:
        assert pred[:4].cpu().tolist() == [0, first, NL - 1, 1]
    conf = torch.zeros(NL, NL, dtype=torch.int32, device=DEV)
    probs2, pred2 = metrics.predict(dev(logits), dev(target), conf)
    _, pred3 = metrics.predict(dev(logits), dev(target), conf, want_probs=False)          # counted twice
    assert torch.equal(pred2, pred) and torch.equal(pred3, pred) and torch.equal(probs2, probs)
    want = np.zeros((NL, NL), np.int64)
    np.add.at(want, (target, pred.cpu().numpy()), 2)
    assert np.array_equal(conf.cpu().numpy(), want)
    assert np.array_equal(want, 2 * F.confusion(torch.from_numpy(target), rpred, NL).numpy())


# ---- adjacency ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["counts", "zero_row", "all_zero", "threshold"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 365, 512])
def test_gen_adj_and_csr_on_synthetic_cooccurrence(C, kind):
    rs = np.random.RandomState(C)
    counts = rs.randint(0, 40, size=(C, C)).astype(np.float64) * (rs.uniform(size=(C, C)) > 0.5)
    nums = counts.max(1) + rs.randint(1, 20, size=C)
    if kind == "zero_row":
        counts[C // 2] = 0
    elif kind == "all_zero":
        counts[:] = 0
    A = R.gen_A(counts, nums, 2.0 if kind == "threshold" else 0.4).astype(np.float32)
    if kind in ("all_zero", "threshold"):
        assert np.array_equal(A != 0, np.eye(C, dtype=bool))            # only the (1 - gamma) diagonal is left
    ref = F.gen_adj(f64(A))
    adj, (rp, col, val) = ops.gen_adj(dev(A), want_csr=True)
    close(adj, ref, 1e-6, "gen_adj", rel=True)
    adj = adj.cpu().numpy()
    assert np.array_equal(adj != 0, ref.numpy() != 0)
    for rp, col, val in ((rp, col, val), ops.dense_to_csr(dev(adj))):
        rp, col, val = rp.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
        assert rp[0] == 0 and rp[C] == np.count_nonzero(adj)
        dense = np.zeros((C, C), np.float32)
        for i in range(C):
            cs = col[rp[i]:rp[i + 1]]
            assert np.all(np.diff(cs) > 0)
            dense[i, cs] = val[rp[i]:rp[i + 1]]
        assert np.array_equal(dense, adj)


# ---- embedding gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(1, 11), (3, 4 * 8192 + 5), (4, 4 * 8192 + 5), (300, 371), (302, 371), (4, 0)])
@pytest.mark.parametrize("aligned", [True, False])
def test_embedding_edges_are_bit_exact(D, n, aligned):
    rs = np.random.RandomState(D + n)
    V = 97
    table = rs.standard_normal((V, D)).astype(np.float32)
    idx = rs.randint(0, V, size=n).astype(np.int64)
    if n:
        idx[0], idx[-1], idx[n // 2] = 0, V - 1, V - 1
    if aligned:
        dt = dev(table)
    else:                                                # a table whose base address is 4 bytes past a 16-byte boundary: the scalar path
        flat = torch.zeros(V * D + 1, device=DEV)
        flat[1:] = dev(table).reshape(-1)
        dt = flat[1:].view(V, D)
        assert dt.data_ptr() % 16 == 4 and dt.is_contiguous()
    out = ops.embedding(dev(idx), dt)
    assert torch.equal(out.cpu(), F.embedding(torch.from_numpy(idx), torch.from_numpy(table)))


# ---- text bank ------------------------------------------------------------------------------------------------------------------
def lstm_weights(rs, E, Hh):
    return [tuple(torch.from_numpy(rs.uniform(-0.08, 0.08, size=s).astype(np.float32))
                  for s in ((4 * Hh, E if layer == 0 else 2 * Hh), (4 * Hh, Hh), (4 * Hh,), (4 * Hh,)))
            for layer in range(2) for _ in range(2)]


# (B, T, lengths)
LSTM_CASES = [(1, 1, "full"), (2, 2, "ones"), (1, 100, "full"), (2, 130, "full"), (65, 100, "increasing"), (65, 130, "decreasing"),
              (65, 100, "empty"), (2, 100, "empty"), (65, 2, "empty"), (65, 1, "ones"), (2, 130, "ones")]


@pytest.mark.parametrize("B,T,kind", LSTM_CASES)
def test_bilstm_edges_match_fp64(B, T, kind):
    """The fp32 recurrence against the float64 text bank.  "empty": a zero-length sample at the START and in the MIDDLE of the batch
    (not only trailing): its rows are zero and the live samples equal the same samples run alone, bit for bit."""
    rs = np.random.RandomState(B * 131 + T)
    V, E, Hh = 700, 300, 150
    emb = torch.from_numpy((0.4 * rs.standard_normal((V, E))).astype(np.float32))
    weights = lstm_weights(rs, E, Hh)
    lens = {"full": np.full(B, T), "ones": np.ones(B, int), "increasing": 1 + np.arange(B), "decreasing": T - np.arange(B),
            "empty": rs.randint(1, T + 1, size=B)}[kind].astype(np.int64)
    if kind == "empty":
        lens[0] = 0
        if B > 2:
            lens[B // 2] = 0
        lens[B - 1] = T
    assert lens.max() <= T and lens.min() >= 0
    tok = np.zeros((B, T), np.int64)
    for b in range(B):
        tok[b, :lens[b]] = rs.randint(1, V, size=lens[b])
    tok_t, lens_t = torch.from_numpy(tok), torch.from_numpy(lens)
    ref = F.text_memory_bank(f64(emb), f64(weights), tok_t, lens_t, Hh)
    dw = [tuple(dev(t) for t in tup) for tup in weights]
    bank = ops.bilstm(dev(tok_t), dev(lens_t), dev(emb), dw, Hh, 2)
    close(bank, ref, LSTM, "text bank")
    pad = torch.arange(T)[None, :] >= lens_t[:, None]
    assert (bank.cpu()[pad] == 0).all(), "padding rows are exact zeros"
    if kind == "empty":
        live = np.nonzero(lens)[0]
        alone = ops.bilstm(dev(tok_t[live]), dev(lens_t[live]), dev(emb), dw, Hh, 2)
        assert torch.equal(bank[torch.from_numpy(live).to(DEV)], alone)


# ---- linear / matmul ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(0, 4, 3), (1, 1, 1), (1, 3, 3), (1, 4, 1), (5, 3, 1), (0, 1, 1), (1023, 1025, 257)])
def test_linear_and_matmul_edges_match_fp64(M, K, N):
    rs = np.random.RandomState(M + 3 * K + N)
    x = torch.from_numpy(rs.standard_normal((M, K)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(N).astype(np.float32))
    res = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32))
    for act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU2):
        for bias, residual in ((b, res), (b, None), (None, res)):
            args = f64([x, w, bias, act, residual])
            y = ops.linear(dev(x), dev(w), dev(bias), act=act, residual=dev(residual))
            assert tuple(y.shape) == (M, N)
            close(y, F.linear(*args), LINEAR, "linear act=%d" % act, rel=True)
        y = ops.matmul(dev(x), dev(w.t().contiguous()), act=act)
        close(y, F.linear(*f64([x, w, None, act, None])), LINEAR, "matmul act=%d" % act, rel=True)
    print("fp32-CPU error:", fp32_cpu_err(lambda *a: F.linear(*a), *f64([x, w, b]))[0], "of", scale(F.linear(*f64([x, w, b]))))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_forward_refusals_at_each_limit_plus_one():
    """Each limit of the entry points: accepted at the limit, refused one step past it by the library's own error (the message of the
    check that failed), never by a launch."""
    z = lambda *s: torch.zeros(*s, device=DEV)

    def core(L=8, D=16, H=2, B=1):
        ops.sq_mha_core(z(B, H * 128), z(B, L, D), None, H, 128, z(H * 128, D), None, z(H * 128, D), None)

    core(L=208)
    core(D=320)
    for kw, msg in ((dict(L=209), "L=209"), (dict(D=324), "D=324"), (dict(D=302), "D=302")):
        with pytest.raises(RuntimeError, match=msg):
            core(**kw)

    def folded(L=8, D=16, H=2, dk=4, ld=None):
        bank = z(1, L, D) if ld is None else torch.zeros(1, L, ld, device=DEV, dtype=torch.bfloat16)
        ops.sq_mha_folded(z(1, H * dk), bank, None, H, dk, z(H * dk, D), z(H * dk, D), None)

    folded(L=208)
    folded(D=320)
    folded(H=8)
    folded(D=316, ld=320)
    for kw, msg in ((dict(L=209), "L=209"), (dict(D=324), "D=324"), (dict(D=302), "D=302"), (dict(H=9), "H=9"),
                    (dict(dk=6), "dk=6"), (dict(D=320, ld=324), "row stride 324")):
        with pytest.raises(RuntimeError, match=msg):
            folded(**kw)

    def img(P=8, N=8, K=16, ldw=304):
        ops.imgbank_pool(z(1, K, P), z(K, ldw), None, N)

    img(P=208)
    img(N=304)
    for kw, msg in ((dict(P=212), "P=212"), (dict(N=305, ldw=308), "N=305"), (dict(K=24), "K=24"), (dict(P=6), "P=6"),
                    (dict(ldw=300), "ldw=300")):
        with pytest.raises(RuntimeError, match=msg):
            img(**kw)

    ops.layernorm(z(2, 2), z(2), z(2))
    ops.layernorm(z(2, 1024), z(1024), z(1024))
    for D in (1, 1025):
        with pytest.raises(RuntimeError, match="D=%d out of range" % D):
            ops.layernorm(z(2, D), z(D), z(D))

    ops.classifier_head([z(1, 1024)] * 4, z(2, 4096), z(2))
    with pytest.raises(RuntimeError, match="feature width 1025"):
        ops.classifier_head([z(1, 1025)] * 4, z(2, 4100), z(2))
    state = ops.classifier_head_state(1, 2, 4, DEV)
    with pytest.raises(RuntimeError, match="feature width 1025"):
        ops.classifier_head_part(z(1, 1025), 0, 4, z(2, 4100), z(2), state)

    ops.head_diff(z(1, 16 * 4), 16)
    with pytest.raises(RuntimeError, match="n_head=17"):
        ops.head_diff(z(1, 17 * 4), 17)

    metrics.predict(z(1, 64))
    with pytest.raises(RuntimeError, match="NL=65"):
        metrics.predict(z(1, 65))

    ops.label_attn_core(z(1, 2 * 64), z(1, 2 * 64), z(1, 2 * 64), 2)
    with pytest.raises(RuntimeError, match="dh=65"):
        ops.label_attn_core(z(1, 2 * 65), z(1, 2 * 65), z(1, 2 * 65), 2)

    def tail(HK):
        packed = {"fc_wp": ops.pack_weight_f32(z(300, HK)), "w1_wp": ops.pack_weight_f32(z(300, 300)),
                  "w2_wp": ops.pack_weight_f32(z(300, 300))}
        packed.update({k: z(300) for k in ("fc_b", "g1", "be1", "b1", "b2", "g2", "be2")})
        ops.mha_tail(z(1, HK), z(1, 300), packed, 1e-6)

    tail(1888)
    for HK in (1892, 1890, 2048):
        with pytest.raises(RuntimeError, match="n_head\\*d_v=%d unsupported" % HK):
            tail(HK)
    torch.cuda.synchronize()                     # nothing was launched out of range: the device is still healthy
