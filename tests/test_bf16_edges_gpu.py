"""Edge sweeps of the bf16 attention cores (csrc/sq_mha_bf16.hip, sq_mha32_bf16.hip with its packing plan, sq_mha_folded_bf16.hip), the
bf16 image bank (imgbank_bf16.hip, imgbank_bf16_pairs.hip) and cast_pad_bf16, each through its ops.* wrapper, against the float64
references of oracle/bf16_path.py (faithful_core, folded_core, img_bank: pinned off the golden shapes by
tests/test_bf16_edges_ref_cpu.py).  The operands go in ALREADY ROUNDED to bf16 (bf16_round: the kernels' own round to nearest even), so
what is left between a kernel and its reference is fp32 summation order -- and, where a kernel stores bf16, that one rounding.

The grids are hand-picked cases, not cross products, in the manner of tests/test_forward_edges_gpu.py: every value of every axis
appears, and the cases sit where a kernel changes path -- the tile-count classes 1 | 2 | 4 | 7 | 13 (tiles of 16) of the 16x16x32
core and the folded kernel, 1 | 2 | 4 | 7 (tiles of 32) of the 32x32x16 core, a batch on either side of the chip (head pairs split
over workgroups, or one workgroup owning more heads than it keeps probability rows for), the 6 | 7 row-tile split and the <196>
build of the stream image bank, the two region halves of the pair form, the limits of a packing plan.

Tolerances: the bounds the suite asserts for the same kernels at the golden shapes (test_sq_mha_core_bf16: probabilities 2e-5 absolute,
o 2e-5 of its largest magnitude; the folded probabilities 2e-5); a value stored as bf16 is held ELEMENT BY ELEMENT to half a bf16 ulp
of its float64 value + 1e-5 of the tensor's largest magnitude (helpers.within_bf16_store).  Every test prints its error beside its
bound, and the float32-CPU error of the same formula (fp32_cpu_err), before it asserts.  No case needed a bound of its own."""
import numpy as np
import pytest
import torch

from mgnns_amd import ops
from oracle import bf16_path as E
from tests import forward_ref as F
from tests import helpers as H
from tests.helpers import close, core_case, f64, fp32_cpu_err
from tests.test_forward_edges_gpu import ROWSUM, dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ATTN = 2e-5        # attention probabilities, absolute (test_sq_mha_core_bf16, ...folded_bf16_ragged_lengths_and_masked_tiles)
OUT_REL = 2e-5     # attention output, relative to its largest magnitude (test_sq_mha_core_bf16)
PRE = "x"


def bf16_dev(t, ld=ops.BANK_LD):
    """bf16-representable values [..., D] -> the device bank [..., ld] bf16, zero padded (an exact conversion: no kernel involved)."""
    out = torch.zeros(*t.shape[:-1], ld, dtype=torch.bfloat16)
    out[..., :t.shape[-1]] = t.to(torch.bfloat16)
    assert torch.equal(out[..., :t.shape[-1]].double(), t.double())
    return out.to(DEV)


def faithful_case(L, D, H, B, kind, bias):
    """core_case with the bank and the weights rounded to bf16 (float64 tensors holding bf16 values); qh, mask, biases as given."""
    qh, bank, mask, wk, bk, wv, bv = core_case(L, D, H, B, kind, bias)
    return qh, E.bf16_round(bank), mask, E.bf16_round(wk), bk, E.bf16_round(wv), bv


def faithful_ref(qh, bank, mask, wk, bk, wv, bv, Hn):
    """oracle faithful_core -> (o [B, H*128], probabilities head-major [H*B, 1, L] like the kernels' attn)."""
    z = torch.zeros(Hn * 128, dtype=torch.float64)
    a = PRE + ".slf_attn."
    p = {a + "w_ks.weight": wk, a + "w_ks.bias": z if bk is None else bk, a + "w_vs.weight": wv, a + "w_vs.bias": z if bv is None else bv}
    o, pa = E.faithful_core(p, PRE, qh, bank, mask, Hn, 128)
    B, L = bank.shape[:2]
    return o, pa.permute(1, 0, 2).reshape(Hn * B, 1, L)


def print_fp32_cpu_err(qh, bank, mask, wk, bk, wv, bv, Hn):
    ref = lambda *a: F.sq_mha_core(a[0], a[1], a[2], Hn, 128, *a[3:])
    print("fp32-CPU error of the reference (o, attn):", fp32_cpu_err(ref, *f64([qh, bank, mask, wk, bk, wv, bv])))


def check_core(o, attn, ro, rattn, mask, Hn, B, L, what, live=None):
    """The bounds of the faithful cores on the samples `live` (default: all); masked positions exactly zero; row sums."""
    assert tuple(attn.shape) == (Hn * B, 1, L) and tuple(o.shape) == (B, Hn * 128)
    idx = torch.arange(B) if live is None else torch.as_tensor(live, dtype=torch.long)
    a, ra = attn.cpu().view(Hn, B, L)[:, idx], rattn.view(Hn, B, L)[:, idx]
    close(a, ra, ATTN, what + " attn")
    close(o.cpu()[idx], ro[idx], OUT_REL, what + " o", rel=True)
    if mask is not None:
        assert (a[:, torch.as_tensor(mask)[idx] == 0] == 0).all(), "masked positions must carry exactly zero probability"
    close(a.double().sum(-1), torch.ones(Hn, len(idx), dtype=torch.float64), ROWSUM, what + " row sums")


# ---- a. faithful cores ----------------------------------------------------------------------------------------------------------
# (L, D, H, B, mask, biases).  16x16x32 form: L on both sides of every class of mha_core_part's switch (1 | 2 | 4 | 7 | 13 tiles of 16);
# D up to the packer's 320 (316: a 4-wide tail of the last 8-column chunk).  A batch of 257 at L = 17 fills the chip: one workgroup
# owns every head pair (11 and 16 heads: more than the eight probability rows it keeps), smaller batches split the pairs.
CORE16_CASES = [
    (1, 300, 8, 1, "none", True),
    (1, 4, 1, 1, "single", True),
    (15, 4, 2, 5, "ragged", True),
    (16, 20, 3, 1, "tile", False),
    (17, 300, 16, 5, "holes", True),
    (17, 300, 11, 257, "ragged", True),
    (17, 20, 16, 257, "none", False),
    (32, 316, 3, 5, "tile", True),
    (33, 320, 1, 5, "holes", False),
    (64, 300, 8, 5, "ragged", False),
    (65, 20, 11, 1, "none", True),
    (112, 304, 3, 5, "holes", False),
    (113, 316, 8, 5, "single", True),
    (196, 300, 2, 5, "none", False),
    (207, 300, 1, 5, "holes", True),
    (208, 320, 16, 5, "none", False),
    (208, 300, 8, 5, "single", True),
    (100, 300, 8, 0, "ragged", True),
]
# 32x32x16 form: classes 1 | 2 | 4 | 7 tiles of 32 (sq_mha32_core_kernel's n_sel): 32 | 33, 64 | 65, 128 | 129 and the 224-row limit; 97 is
# three tiles inside the 4-tile class; the packer takes D <= 304.  Masked cases with L <= 128 run a second time with a packing plan.
CORE32_CASES = [
    (1, 300, 8, 1, "none", True),
    (8, 4, 1, 1, "single", True),
    (9, 20, 2, 5, "ragged", True),
    (31, 304, 3, 5, "holes", False),
    (32, 300, 16, 1, "tile", True),
    (33, 300, 3, 5, "holes", True),
    (17, 300, 11, 257, "ragged", True),
    (17, 20, 16, 257, "none", False),
    (64, 304, 8, 5, "tile", False),
    (65, 20, 11, 1, "none", True),
    (97, 300, 3, 5, "single", True),
    (128, 300, 8, 5, "ragged", True),
    (129, 4, 1, 5, "holes", True),
    (196, 300, 8, 5, "none", False),
    (208, 300, 2, 5, "single", True),
    (209, 304, 3, 1, "none", True),
    (223, 300, 1, 5, "holes", False),
    (224, 300, 16, 5, "none", True),
    (224, 304, 8, 5, "ragged", False),
    (100, 300, 8, 0, "ragged", True),
]


@pytest.mark.parametrize("form,L,D,Hn,B,kind,bias", [(16,) + c for c in CORE16_CASES] + [(32,) + c for c in CORE32_CASES])
def test_sq_mha_core_bf16_edges_match_fp64(form, L, D, Hn, B, kind, bias):
    """Both builds of the faithful core, one workgroup per sample (and the 32 form once more with a packing plan where it takes one),
    against faithful_core on the same rounded operands.  b_k never enters (softmax invariant) and b_v is guarded for null in every
    kernel (sq_mha_bf16.hip `if (bv)`, sq_mha32_bf16.hip `bv ? bv[d] : 0.f`): `None` biases are legal."""
    qh, bank, mask, wk, bk, wv, bv = faithful_case(L, D, Hn, B, kind, bias)
    print_fp32_cpu_err(qh, bank, mask, wk, bk, wv, bv, Hn)
    ro, rattn = faithful_ref(qh, bank, mask, wk, bk, wv, bv, Hn)
    wp = ops.pack_kv_weights_bf16(dev(wk.float()), dev(wv.float()), Hn, 128, form=form)
    dq, dbank, dm, dbk, dbv = dev(qh), bf16_dev(bank), dev(mask), dev(bk), dev(bv)
    plans = [None]
    if form == 32 and mask is not None and L <= ops.PLAN_MAX_L:
        plans.append(ops.sq_mha_plan(dm))
    for plan in plans:
        what = "core%d%s" % (form, "" if plan is None else " packed")
        o, attn = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, dbk, dbv, plan=plan)
        check_core(o, attn, ro, rattn, mask, Hn, B, L, what)
        o2, none = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, dbk, dbv, want_attn=False, plan=plan)
        assert none is None and torch.equal(o2, o), "want_attn=False must give the same bits"
        o3, attn3 = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, dbk, dbv, plan=plan)
        assert torch.equal(o3, o) and torch.equal(attn3, attn), "a repeated launch must give the same bits"


@pytest.mark.parametrize("form,L,Hn,dead", [(16, 16, 3, 0), (16, 100, 8, 2), (16, 208, 1, 4), (32, 32, 3, 0), (32, 100, 8, 2), (32, 224, 2, 4)])
def test_sq_mha_core_bf16_fully_masked_sample_is_nan_and_leaves_the_others_alone(form, L, Hn, dead):
    """One workgroup per sample: a sample without a live position has NaN probabilities and a NaN output row (0 * inf, like the
    reference's softmax over -inf); every other sample is bit-equal to the same batch launched without it."""
    qh, bank, mask, wk, bk, wv, bv = faithful_case(L, 300, Hn, 5, "ragged", True)
    mask[dead] = 0
    wp = ops.pack_kv_weights_bf16(dev(wk.float()), dev(wv.float()), Hn, 128, form=form)
    dq, dbank, dm, dbk, dbv = dev(qh), bf16_dev(bank), dev(mask), dev(bk), dev(bv)
    o, attn = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, dbk, dbv)
    a = attn.view(Hn, 5, L)
    assert torch.isnan(a[:, dead]).all() and torch.isnan(o[dead]).all()
    keep = [b for b in range(5) if b != dead]
    o4, attn4 = ops.sq_mha_core_bf16(dq[keep].contiguous(), dbank[keep].contiguous(), dm[keep].contiguous(), Hn, 128, wp, dbk, dbv)
    assert torch.equal(o[keep], o4) and torch.equal(a[:, keep], attn4.view(Hn, 4, L))
    ro, rattn = faithful_ref(qh, bank, mask, wk, bk, wv, bv, Hn)
    assert torch.isnan(rattn.view(Hn, 5, L)[:, dead]).all()
    check_core(o, attn, ro, rattn, mask, Hn, 5, L, "core%d next to a dead sample" % form, live=keep)


# ---- b. the plan kernel and the packed launch ---------------------------------------------------------------------------------------
def plan_mask(kind, rs):
    """-> [B, L] float32 mask of a named plan case."""
    def lens_mask(lens, L):
        m = np.zeros((len(lens), L), np.float32)
        for b, n in enumerate(lens):
            m[b, :n] = 1
        return m
    if kind.startswith("short"):                         # every sample <= 8 rows: the 16-sample limit and the 128-row limit together
        return lens_mask(rs.randint(1, 9, size=int(kind[5:])), 20)
    if kind == "full128":                                # one sample per group
        return lens_mask([128, 128, 128], 128)
    if kind == "rows_first":                             # 120 + 8 rows fill a group with two samples
        return lens_mask([120, 8, 8, 8, 120, 8, 1], 128)
    if kind == "8_9_16_17":
        return lens_mask([8, 9, 16, 17, 17, 16, 9, 8], 40)
    if kind == "holes":                                  # holes in front of a live last position
        m = (rs.uniform(size=(5, 64)) > 0.4).astype(np.float32)
        m[:, 63] = 1
        m[:, 0] = 0
        return m
    if kind == "only_first_or_last":
        m = np.zeros((5, 33), np.float32)
        m[0, 0] = m[1, 32] = m[3, 0] = m[4, 32] = 1
        m[2] = 1
        return m
    if kind == "dead":                                   # dead samples at the start, at the end, and as the whole of group 1
        lens = [0] + [8] * 15 + [0] * 16 + list(rs.randint(1, 17, size=7)) + [0]
        return lens_mask(lens, 16)
    if kind == "one":
        return lens_mask([37], 100)
    if kind == "empty":
        return np.zeros((0, 50), np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind,Hn", [("short16", 8), ("short17", 3), ("short33", 2), ("full128", 8), ("rows_first", 1), ("8_9_16_17", 8),
                                     ("holes", 3), ("only_first_or_last", 2), ("dead", 8), ("one", 8), ("empty", 8)])
def test_sq_mha_plan_and_packed_core_match_fp64(kind, Hn):
    """The plan's invariants (helpers.check_plan) and the packed launch against faithful_core at the bounds of the unpacked cores -- not
    only against the unpacked launch.  Dead samples are NaN; the live ones next to them stay finite and correct."""
    rs = np.random.RandomState(sum(map(ord, kind)) + Hn)
    mask = plan_mask(kind, rs)
    B, L = mask.shape
    dm = dev(mask)
    plan = ops.sq_mha_plan(dm)
    groups, off, lv = H.check_plan(plan, mask)
    print("plan %s: %d samples in %d groups, rows %s" % (kind, B, len(groups), [g[2] for g in groups][:8]))
    if kind.startswith("short"):
        assert [g[1] for g in groups][:B // 16] == [16] * (B // 16)                 # the sample limit closes these groups
    if kind == "full128":
        assert [g[1:] for g in groups] == [(1, 128)] * 3
    if kind == "rows_first":
        assert groups[0] == (0, 2, 128)
    if kind == "dead":
        assert groups[0] == (0, 16, 128) and groups[1] == (16, 16, 128) and not mask[16:32].any()
    qh = torch.from_numpy(rs.standard_normal((B, Hn * 128)).astype(np.float32))
    bank = E.bf16_round(torch.from_numpy((1.2 * rs.standard_normal((B, L, 300))).astype(np.float32)))
    wk, wv = (E.bf16_round(torch.from_numpy((0.05 * rs.standard_normal((Hn * 128, 300))).astype(np.float32))) for _ in range(2))
    bv = torch.from_numpy(rs.standard_normal(Hn * 128).astype(np.float32))
    print_fp32_cpu_err(qh, bank, torch.from_numpy(mask), wk, None, wv, bv, Hn)
    ro, rattn = faithful_ref(qh, bank, torch.from_numpy(mask), wk, None, wv, bv, Hn)
    wp = ops.pack_kv_weights_bf16(dev(wk.float()), dev(wv.float()), Hn, 128, form=32)
    dq, dbank, dbv = dev(qh), bf16_dev(bank), dev(bv)
    o, attn = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, None, dbv, plan=plan)
    live = np.nonzero(mask.any(axis=1))[0]
    dead = np.nonzero(~mask.any(axis=1))[0]
    check_core(o, attn, ro, rattn, mask, Hn, B, L, "packed " + kind, live=live)
    if len(dead):
        assert torch.isnan(o.cpu()[dead]).all() and torch.isnan(attn.cpu().view(Hn, B, L)[:, dead]).all()
    o2, none = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, None, dbv, want_attn=False, plan=plan)
    o3, attn3 = ops.sq_mha_core_bf16(dq, dbank, dm, Hn, 128, wp, None, dbv, plan=plan)
    assert none is None
    lt = torch.from_numpy(live).to(DEV)
    assert torch.equal(o2[lt], o[lt]) and torch.equal(o3[lt], o[lt])
    assert torch.equal(attn3.view(Hn, B, L)[:, lt], attn.view(Hn, B, L)[:, lt])


def test_sq_mha_plan_at_the_largest_batch():
    """B = PLAN_MAX_B at L = 8: one workgroup scans the batch with all the LDS the plan kernel may ask for; 256 full groups."""
    rs = np.random.RandomState(4096)
    mask = (rs.uniform(size=(ops.PLAN_MAX_B, 8)) > 0.5).astype(np.float32)
    mask[0] = 0
    mask[-1] = 1
    groups, off, lv = H.check_plan(ops.sq_mha_plan(dev(mask)), mask)
    print("plan of %d samples: %d groups" % (ops.PLAN_MAX_B, len(groups)))
    assert len(groups) == ops.PLAN_MAX_B // 16 and all(g[1:] == (16, 128) for g in groups)


# ---- c. folded bf16 core ------------------------------------------------------------------------------------------------------------
# (L, D, H, B, mask): L as the 16x16x32 core's (row tiles of 16; GEMM 2 walks them in pairs)
FOLDED_CASES = [
    (1, 300, 8, 1, "none"), (15, 4, 1, 5, "ragged"), (16, 20, 3, 1, "tile"), (17, 300, 8, 257, "ragged"), (32, 320, 3, 5, "tile"),
    (33, 4, 1, 5, "holes"), (64, 300, 8, 5, "ragged"), (65, 20, 3, 1, "none"), (112, 320, 1, 5, "holes"), (113, 300, 8, 5, "single"),
    (196, 300, 8, 5, "none"), (207, 20, 3, 5, "holes"), (208, 320, 8, 5, "none"), (208, 300, 1, 5, "single"), (100, 300, 8, 0, "ragged"),
]


@pytest.mark.parametrize("L,D,Hn,B,kind", FOLDED_CASES)
def test_sq_mha_folded_bf16_edges_match_fp64(L, D, Hn, B, kind):
    """Probabilities against folded_core; the stored c ELEMENT BY ELEMENT against float64 on the kernel's own probabilities rounded to
    bf16 (what it feeds its second product) and the bf16 bank -- the weighted sum apart from rounding flips of the probabilities."""
    rs = np.random.RandomState(L * 1000 + D + 7 * Hn + B)
    u = torch.from_numpy((0.3 * rs.standard_normal((B, Hn * D))).astype(np.float32))
    bank = E.bf16_round(torch.from_numpy((1.2 * rs.standard_normal((B, L, D))).astype(np.float32)))
    mask = H.make_mask(kind, B, L, rs)
    tm = None if mask is None else torch.from_numpy(mask)
    _, rp = E.folded_core(u, bank, tm, Hn, 128)                                    # [B, H, L]
    du, dbank, dm = dev(u), bf16_dev(bank), dev(mask)
    c, attn = ops.sq_mha_folded_bf16(du, dbank, dm, Hn, 128)
    ldc = (Hn * D + 31) // 32 * 32
    assert tuple(c.shape) == (B, ldc) and tuple(attn.shape) == (Hn * B, 1, L)
    a = attn.cpu().view(Hn, B, L)
    close(a, rp.permute(1, 0, 2), ATTN, "folded attn")
    if mask is not None:
        assert (a[:, tm == 0] == 0).all(), "masked positions must carry exactly zero probability"
    close(a.double().sum(-1), torch.ones(Hn, B, dtype=torch.float64), ROWSUM, "folded row sums")
    want = torch.einsum("hbl,blf->bhf", E.bf16_round(a), bank).reshape(B, Hn * D)
    H.within_bf16_store(c[:, :Hn * D].float(), want, "folded c")
    assert not c[:, Hn * D:].any(), "columns behind H * D must be exact zeros"
    c2, none = ops.sq_mha_folded_bf16(du, dbank, dm, Hn, 128, want_attn=False)
    c3, attn3 = ops.sq_mha_folded_bf16(du, dbank, dm, Hn, 128)
    assert none is None and torch.equal(c2, c) and torch.equal(c3, c) and torch.equal(attn3, attn)


# ---- d. bf16 image bank -------------------------------------------------------------------------------------------------------------
def img_case(P, K, N, B, bias):
    rs = np.random.RandomState(P + K + 3 * N + B)
    feat = rs.standard_normal((B, K, P)).astype(np.float32)               # signed: the trunk's ReLU is not assumed
    feat[:, ::3] = -np.abs(feat[:, ::3]) - 0.5                               # all-negative feature rows: a zero-initialised max fails
    w = (0.05 * rs.standard_normal((N, K))).astype(np.float32)
    b = (0.05 * rs.standard_normal(N)).astype(np.float32) if bias else None
    return torch.from_numpy(feat), torch.from_numpy(w), None if b is None else torch.from_numpy(b)


def img_run(form, feat, w, b, N):
    wp = ops.pack_imgbank_weights_bf16(dev(w))
    ops.imgbank_set_form(form)
    try:
        bank, pooled = ops.imgbank_pool_bf16(dev(feat), wp, dev(b), N)
        bank2, halves = ops.imgbank_pool_bf16(dev(feat), wp, dev(b), N, combine=False)
    finally:
        ops.imgbank_set_form(0)
    assert torch.equal(bank, bank2), "a repeated launch must give the same bits"
    return bank, pooled, halves


def img_check(form, P, K, N, B, bias):
    feat, w, b = img_case(P, K, N, B, bias)
    zb = torch.zeros(N) if b is None else b
    print("fp32-CPU error of the reference (bank, pooled):", fp32_cpu_err(F.imgbank_pool, E.bf16_round(feat), E.bf16_round(w), zb.double()))
    want, rpool = E.img_bank(feat, w, zb, rounding=("imgbank_x", "imgbank_w"))      # the bank BEFORE its bf16 store
    bank, pooled, halves = img_run(form, feat, w, b, N)
    assert tuple(bank.shape) == (B, P, ops.BANK_LD) and bank.dtype == torch.bfloat16
    assert torch.equal(pooled.cpu().double(), rpool), "the pooled max is exact"
    assert tuple(halves.shape) == (B, 2, K) and torch.equal(halves.cpu().double().amax(dim=1), rpool), "the two halves reduce to the max"
    assert not bank[..., N:].any(), "bank columns >= N must be exact zeros"
    H.within_bf16_store(bank[..., :N].float(), want, "image bank form %d" % form)
    return bank


# stream form (one workgroup per sample).  P: 16 (one row tile), 96 | 100 | 104 | 108 | 112 around the 6 | 7 tile split between the waves,
# 196 (the <196> build: row offsets as immediates), 200 ... 208 (the last tile ragged, then full); K: one trip of the main loop, three, 32
STREAM_CASES = [(16, 64, 1, 1, True), (20, 192, 17, 2, False), (32, 64, 300, 7, True), (96, 192, 304, 1, True), (100, 64, 17, 2, True),
                (104, 2048, 300, 1, False), (108, 64, 304, 2, True), (112, 192, 1, 7, False), (196, 2048, 300, 2, True),
                (200, 64, 17, 1, True), (204, 192, 300, 2, False), (208, 2048, 304, 1, True), (196, 64, 300, 0, True)]
# pair form (two workgroups per sample: regions [0, 104) and [104, P)): the second half from one quad to its six full tiles
PAIR_CASES = [(108, 128, 17, 1, True), (112, 256, 300, 2, False), (120, 2048, 304, 1, True), (196, 2048, 300, 2, True),
              (200, 128, 1, 7, False), (196, 128, 300, 0, True)]


@pytest.mark.parametrize("form,P,K,N,B,bias", [(1,) + c for c in STREAM_CASES] + [(2,) + c for c in PAIR_CASES])
def test_imgbank_pool_bf16_edges_match_fp64(form, P, K, N, B, bias):
    img_check(form, P, K, N, B, bias)


def test_imgbank_pool_bf16_form_by_batch_on_both_sides_of_half_the_chip():
    """Form 0 takes the pair form while 2 B <= compute units and the stream form above: the batch on either side."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (cus // 2, cus // 2 + 1):
        img_check(0, 196, 128, 300, B, True)


@pytest.mark.parametrize("P,K,N,B", [(108, 128, 300, 2), (196, 2048, 300, 1), (200, 256, 17, 7)])
def test_imgbank_forms_agree_to_one_bf16_ulp(P, K, N, B):
    feat, w, b = img_case(P, K, N, B, True)
    b1, p1, _ = img_run(1, feat, w, b, N)
    b2, p2, _ = img_run(2, feat, w, b, N)
    assert torch.equal(p1, p2)
    x, y = b1.float().cpu().double(), b2.float().cpu().double()
    ulp = torch.maximum(x.abs(), y.abs()) * 2.0 ** -7          # a bf16 ulp is at most 2^-7 of the value
    worst = float(((x - y).abs() / ulp.clamp_min(1e-30)).max())
    print("forms 1 and 2: largest difference %.3f ulp (bound 1), %d of %d elements differ" % (worst, int((x != y).sum()), x.numel()))
    assert ((x - y).abs() <= ulp).all()


# ---- e. cast_pad_bf16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1, 1000])
@pytest.mark.parametrize("D,ld", [(1, 8), (7, 8), (8, 8), (1, 320), (8, 320), (300, 320), (320, 320)])
def test_cast_pad_bf16_is_round_to_nearest_even_bit_for_bit(D, ld, rows):
    rs = np.random.RandomState(D + ld + rows)
    x = (rs.standard_normal(rows * D) * 10.0 ** rs.randint(-20, 20, size=rows * D)).astype(np.float32)
    n = min(x.size, H.BF16_SPECIALS.size)
    x[:n] = H.BF16_SPECIALS.view(np.float32)[:n]
    if x.size > 2 * n:                                   # ... and at the end of the last row
        x[-n:] = H.BF16_SPECIALS.view(np.float32)[::-1][:n]
    x = x.reshape(rows, D)
    y = ops.cast_pad_bf16(torch.from_numpy(x).to(DEV), ld)
    assert tuple(y.shape) == (rows, ld) and y.dtype == torch.bfloat16
    got = y.view(torch.int16).cpu().numpy().view(np.uint16)
    want = np.zeros((rows, ld), np.uint16)
    want[:, :D] = E.bf16_bits(x)
    bad = np.argwhere(got != want)
    print("cast_pad_bf16 D=%d ld=%d rows=%d: %d of %d elements differ" % (D, ld, rows, len(bad), want.size))
    assert not len(bad), "first differences (row, col, got, want, input bits): %s" % [
        (int(r), int(c), hex(got[r, c]), hex(want[r, c]), hex(x.view(np.uint32)[r, c]) if c < D else "pad") for r, c in bad[:4]]


# ---- f. refusals --------------------------------------------------------------------------------------------------------------------
def test_bf16_refusals_at_each_limit_plus_one():
    """Each limit of the entry points: accepted at the limit, refused one step past it by the library's (or the wrapper's) own check,
    never by a launch; a valid call behind every refusal still runs."""
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, device=DEV, dtype=dtype)
    refused = pytest.raises((RuntimeError, ValueError))

    def pack(form, D=16, Hn=2):
        return ops.pack_kv_weights_bf16(z(Hn * 128, D), z(Hn * 128, D), Hn, 128, form=form)

    def core(form, L=8, Hn=2, ld=320, wp=None):
        wp = pack(form, Hn=min(Hn, 16)) if wp is None else wp
        ops.sq_mha_core_bf16(z(1, Hn * 128), z(1, L, ld, dtype=torch.bfloat16), None, Hn, 128, wp, None, None)

    for form, lmax, dmax in ((16, 208, 320), (32, 224, 304)):
        core(form, L=lmax)
        core(form, Hn=16)
        pack(form, D=dmax)
        with pytest.raises(RuntimeError, match="L=%d" % (lmax + 1)):
            core(form, L=lmax + 1)
        with pytest.raises(RuntimeError, match="n_head=17"):
            core(form, Hn=17)
        with pytest.raises(RuntimeError, match="D=%d" % (dmax + 1)):
            pack(form, D=dmax + 1)
        for ld in (312, 328):
            with pytest.raises(RuntimeError, match="bank row length %d" % ld):
                core(form, ld=ld)
        core(form)

    ops.sq_mha_plan(z(2, 128))
    with pytest.raises(RuntimeError, match="L=129"):
        ops.sq_mha_plan(z(2, 129))
    with pytest.raises(ValueError, match="batch %d" % (ops.PLAN_MAX_B + 1)):
        ops.sq_mha_plan(z(ops.PLAN_MAX_B + 1, 8))
    mask = torch.ones(2, 129, device=DEV)
    with refused:                                        # a plan of the right size for a mask that is too long
        ops.sq_mha_core_bf16(z(2, 256), z(2, 129, 320, dtype=torch.bfloat16), mask, 2, 128, pack(32), None, None, plan=ops.sq_mha_plan(z(2, 128)))
    ops.sq_mha_core_bf16(z(2, 256), z(2, 128, 320, dtype=torch.bfloat16), mask[:, :128].contiguous(), 2, 128, pack(32), None, None,
                         plan=ops.sq_mha_plan(mask[:, :128].contiguous()))

    def folded(L=8, D=16, Hn=2, ld=320):
        ops.sq_mha_folded_bf16(z(1, Hn * D), z(1, L, ld, dtype=torch.bfloat16), None, Hn, 128)

    folded(L=208)
    folded(D=320)
    folded(Hn=8)
    for kw, msg in ((dict(L=209), "L=209"), (dict(D=324), "D=324"), (dict(D=302), "D=302"), (dict(Hn=9), "H=9")):
        with pytest.raises(RuntimeError, match=msg):
            folded(**kw)
    for ld in (312, 328):
        with pytest.raises(ValueError, match="last dim %d" % ld):
            folded(ld=ld)
    folded()

    def img(P=16, N=8, K=64, n_pack=None, form=0):
        wp = ops.pack_imgbank_weights_bf16(z(N if n_pack is None else n_pack, K))
        ops.imgbank_set_form(form)
        try:
            ops.imgbank_pool_bf16(z(1, K, P), wp, None, N)
        finally:
            ops.imgbank_set_form(0)

    img(P=208)
    img(N=304)
    for kw, msg in ((dict(P=12), "P=12"), (dict(P=212), "P=212"), (dict(P=198), "P=198"), (dict(K=96), "K=96"),
                    (dict(N=305, n_pack=304), "N=305"), (dict(P=198, K=128, form=2), "P=198")):
        with pytest.raises(RuntimeError, match=msg):
            img(**kw)
    with pytest.raises(RuntimeError, match="N=305"):
        ops.pack_imgbank_weights_bf16(z(305, 64))
    img()
    img(P=200, K=128, form=2)

    ops.cast_pad_bf16(z(2, 8), 8)
    for D, ld in ((9, 8), (8, 12)):
        with pytest.raises(RuntimeError, match="D=%d ld=%d" % (D, ld)):
            ops.cast_pad_bf16(z(2, D), ld)
    torch.cuda.synchronize()                     # nothing was launched out of range: the device is still healthy
