"""What tests/test_bf16_edges_gpu.py measures the bf16 kernels with, pinned without a GPU and off the golden shapes: the oracle's
attention cores on rounded operands are the plain formula of tests/forward_ref.py, its rounding helper is torch's bf16 cast on the
special values the cast kernel is fed, and the plan checker accepts a valid plan and refuses one broken in each way."""
import numpy as np
import pytest
import torch

from oracle import bf16_path as E
from tests import forward_ref as F
from tests import helpers as H

# (L, D, H, B, mask, biases): three of the GPU file's edge cases
EDGE_SHAPES = [(17, 20, 3, 5, "holes", True), (113, 316, 2, 3, "single", False), (224, 304, 1, 2, "ragged", True)]


@pytest.mark.parametrize("L,D,Hn,B,kind,bias", EDGE_SHAPES)
def test_faithful_core_on_rounded_operands_is_the_plain_formula(L, D, Hn, B, kind, bias):
    qh, bank, mask, wk, bk, wv, bv = H.core_case(L, D, Hn, B, kind, bias)
    bank, wk, wv = E.bf16_round(bank), E.bf16_round(wk), E.bf16_round(wv)
    z = torch.zeros(Hn * 128, dtype=torch.float64)
    p = {"x.slf_attn.w_ks.weight": wk, "x.slf_attn.w_ks.bias": z if bk is None else bk,
         "x.slf_attn.w_vs.weight": wv, "x.slf_attn.w_vs.bias": z if bv is None else bv}
    o, pa = E.faithful_core(p, "x", qh, bank, mask, Hn, 128)
    assert o.dtype == torch.float64 and tuple(pa.shape) == (B, Hn, L)
    ro, rattn = F.sq_mha_core(*H.f64([qh, bank, mask]), Hn, 128, *H.f64([wk, bk, wv, bv]))
    assert H.maxerr(pa.permute(1, 0, 2).reshape(Hn * B, 1, L), rattn) <= 1e-14
    assert H.maxerr(o, ro) <= 1e-12 * H.scale(ro)
    # rounding the weights is idempotent: the oracle's own rounding point changes nothing on rounded operands
    o2, pa2 = E.faithful_core(p, "x", qh, bank, mask, Hn, 128, rounding=())
    assert torch.equal(o2, o) and torch.equal(pa2, pa)


@pytest.mark.parametrize("L,D,Hn,B,kind,bias", EDGE_SHAPES)
def test_folded_core_on_rounded_operands_is_the_plain_formula(L, D, Hn, B, kind, bias):
    """folded_core is the plain core with identity projections: K = V = the bank for every head, the query rows u, temperature sqrt(d_k).
    Without its inner rounding points it equals tests/forward_ref.sq_mha_core; with them, c is the rounded sum over rounded
    probabilities -- the formula the GPU test rebuilds from the kernel's own probabilities."""
    rs = np.random.RandomState(L + D + Hn)
    u = E.bf16_round(torch.from_numpy((0.3 * rs.standard_normal((B, Hn * D))).astype(np.float32)))
    bank = E.bf16_round(torch.from_numpy((1.2 * rs.standard_normal((B, L, D))).astype(np.float32)))
    mask = H.make_mask(kind, B, L, rs)
    tm = None if mask is None else torch.from_numpy(mask).double()
    eye = torch.eye(D, dtype=torch.float64).repeat(Hn, 1)                # [H * D, D]: every head sees the bank itself
    ro, rattn = F.sq_mha_core(u, bank, tm, Hn, D, eye, None, eye, None)
    c, pa = E.folded_core(u, bank, tm, Hn, D, rounding=())
    assert H.maxerr(pa.permute(1, 0, 2).reshape(Hn * B, 1, L), rattn) <= 1e-14
    assert H.maxerr(c, ro) <= 1e-12 * H.scale(ro)
    c16, pa16 = E.folded_core(u, bank, tm, Hn, D)
    assert torch.equal(pa16, pa)                                          # u is already rounded; the probabilities are never rounded
    want = E.bf16_round(torch.einsum("bhl,blf->bhf", E.bf16_round(pa), bank)).reshape(B, Hn * D)
    assert torch.equal(c16, want)
    H.within_bf16_store(c16, torch.einsum("bhl,blf->bhf", E.bf16_round(pa), bank).reshape(B, Hn * D), "rounded c")


def test_bf16_round_is_torch_bfloat16_on_the_special_values():
    x = H.BF16_SPECIALS.view(np.float32)
    t = torch.from_numpy(x.copy())
    mine, ref = E.bf16_round(t), t.bfloat16().double()
    nan = torch.isnan(t)
    assert int(nan.sum()) == 6 and torch.isnan(mine[nan]).all() and torch.isnan(ref[nan]).all()
    assert torch.equal(mine[~nan], ref[~nan])
    assert torch.equal(torch.signbit(mine[~nan]), torch.signbit(ref[~nan]))                     # -0 stays -0
    bits = E.bf16_bits(x)
    tb = t.bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bits[~nan.numpy()], tb[~nan.numpy()])
    # a NaN keeps its sign and stays a NaN whatever its payload (a carry into the exponent or the sign would make it inf or -0)
    assert all((b & 0x7F80) == 0x7F80 and (b & 0x7F) for b in bits[nan.numpy()])
    assert np.array_equal(bits[nan.numpy()] >> 15, H.BF16_SPECIALS[nan.numpy()] >> 31)
    # ties go to the even neighbour; the largest finite fp32 rounds to inf; denormals below half the smallest bf16 denormal flush to 0
    assert list(bits[:4]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82] and bits[18] == 0x7F80 and bits[9] == 0 and bits[10] == 0 and bits[11] == 2


def _valid_plan():
    """Five samples of a [5, 20] mask: live rows 20, 0 (dead), 3, 9, 1 -> one group of 24 + 8 + 8 + 16 + 8 = 64 rows."""
    mask = np.zeros((5, 20), np.float32)
    mask[0] = 1
    mask[2, :3] = 1
    mask[3, [0, 8]] = 1                                                   # a hole: live rows = last live position + 1 = 9
    mask[4, 0] = 1
    B = 5
    plan = np.zeros(4 + 6 * B, np.int32)
    plan[:4] = [1, B, 8 | (128 << 8) | (16 << 20), 0]
    plan[4:7] = [0, 5, 64]
    for b, (off, lv) in enumerate([(0, 20), (24, 0), (32, 3), (40, 9), (56, 1)]):
        plan[4 + 4 * B + 2 * b: 4 + 4 * B + 2 * b + 2] = [off, lv]
    return plan, mask


def test_plan_checker_accepts_a_valid_plan_and_refuses_each_broken_one():
    plan, mask = _valid_plan()
    groups, off, lv = H.check_plan(plan, mask)
    assert groups == [(0, 5, 64)] and list(off) == [0, 24, 32, 40, 56] and list(lv) == [20, 0, 3, 9, 1]
    two = plan.copy()                                                     # the same samples as two groups: still valid
    two[0] = 2
    two[4:7] = [0, 2, 32]
    two[8:11] = [2, 3, 32]
    two[4 + 20 + 4: 4 + 20 + 10: 2] = [0, 8, 24]
    assert H.check_plan(two, mask)[0] == [(0, 2, 32), (2, 3, 32)]

    def broken(edit, msg, m=mask, base=plan):
        p = base.copy()
        edit(p)
        with pytest.raises(AssertionError, match=msg):
            H.check_plan(p, m)

    def put(i, v):
        return lambda p: p.__setitem__(i, v)

    s = 4 + 4 * 5                                                         # the first sample entry
    broken(put(1, 4), "built for a batch of 4")
    broken(lambda p: p.__setitem__(slice(5, 7), [4, 56]), "exactly one group")                               # the last sample in no group
    broken(lambda p: (p.__setitem__(0, 2), p.__setitem__(slice(8, 11), [0, 1, 24])), "exactly one group")    # sample 0 in two groups
    broken(put(s + 2 * 2, 28), "not 8-aligned")
    broken(put(s + 2 * 2, 40), "its predecessors end at 32")
    broken(put(s + 2 * 3 + 1, 2), "live rows differ")                     # the hole's sample: a count of live positions is wrong
    broken(put(s + 2 * 1 + 1, 1), "live rows differ")                     # a dead sample must say 0
    broken(put(6, 72), "says 72 rows")
    broken(put(5, 6), "runs past the batch")
    # the limits: 17 samples of 8 rows in one group; 136 rows in one group
    m17 = np.zeros((17, 8), np.float32)
    m17[:, 0] = 1
    p17 = np.zeros(4 + 6 * 17, np.int32)
    p17[:7] = [1, 17, 0, 0, 0, 17, 136]
    p17[4 + 4 * 17::2] = 8 * np.arange(17)
    p17[4 + 4 * 17 + 1::2] = 1
    with pytest.raises(AssertionError, match="holds 17 samples"):
        H.check_plan(p17, m17)
    m2 = np.ones((2, 72), np.float32)
    p2 = np.zeros(4 + 6 * 2, np.int32)
    p2[:7] = [1, 2, 0, 0, 0, 2, 144]
    p2[12:16] = [0, 72, 72, 72]
    with pytest.raises(AssertionError, match="holds 144 rows"):
        H.check_plan(p2, m2)
    with pytest.raises(AssertionError, match="plan size"):
        H.check_plan(plan[:-1], mask)
