"""The host restatement of the dropout hash (tests/dropout_ref.py) on its own, without a GPU: it is the splitmix64 finaliser,
its masks keep the binomial fraction at every site, heads, sites and seeds draw uncorrelated masks, and the rate is compared in
float32.  tests/test_train_edges_gpu.py then holds every kernel's applied mask to it bit for bit."""
import math

import numpy as np
import pytest

from tests import dropout_ref as DR

N = 1 << 18


def within_6_sigma(frac, p, n):
    return abs(frac - p) <= 6 * math.sqrt(p * (1 - p) / n)


def test_restatement_is_the_splitmix64_finaliser():
    # seed 0, site 0, idx 0 / 1: the first two outputs of the public splitmix64 generator seeded with 0
    assert int(DR.hash64(0, 0, 0)) == 0xE220A8397B1DCDAF
    assert int(DR.hash64(0, 0, 1)) == 0x6E789E6AA1B965F4
    # the site sits above bit 48 of the counter: (site 1, idx 0) is (site 0, idx 2**48)
    assert int(DR.hash64(5, 1, 0)) == int(DR.hash64(5, 0, 1 << 48))
    # seeds wrap mod 2**64
    assert int(DR.hash64(-1, 2, 7)) == int(DR.hash64((1 << 64) - 1, 2, 7))
    for site, idx, out in [(0, 0, 0), (4, 123456, (1 << 64) - 1), (3, 77, 1 << 40)]:
        assert int(DR.hash64(DR.seed_for(site, idx, out), site, idx)) == out


@pytest.mark.parametrize("rate", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("site", DR.SITES)
def test_keep_fraction_is_binomial(site, rate):
    k = DR.keep(12345 + site, site, np.arange(N), rate)
    assert within_6_sigma(k.mean(), 1 - rate, N), (site, rate, k.mean())


def agreement_ok(a, b, rate):
    p = 1 - rate
    agree = p * p + (1 - p) * (1 - p)
    n = a.size
    got = float((a == b).mean())
    return abs(got - agree) <= 6 * math.sqrt(agree * (1 - agree) / n), got


@pytest.mark.parametrize("rate", [0.1, 0.5, 0.9])
def test_masks_are_uncorrelated_across_heads_sites_and_seeds(rate):
    H, B, L = 8, 64, 196
    ka = DR.keep(3, DR.DROP_ATTN, DR.attn_index(H, B, L), rate)           # [H, B, L]
    for h in range(H - 1):
        ok, got = agreement_ok(ka[h], ka[h + 1], rate)
        assert ok, ("heads", h, got)
    idx = np.arange(N)
    for s in DR.SITES:
        for t in DR.SITES:
            if s < t:
                ok, got = agreement_ok(DR.keep(3, s, idx, rate), DR.keep(3, t, idx, rate), rate)
                assert ok, ("sites", s, t, got)
    for seed in (0, 1, (1 << 62) - 1, (1 << 64) - 2):
        ok, got = agreement_ok(DR.keep(seed, DR.DROP_FC, idx, rate), DR.keep(seed + 1, DR.DROP_FC, idx, rate), rate)
        assert ok, ("seeds", seed, got)
    # neighbouring elements of one site: the counter's low bits mix as well
    k = DR.keep(9, DR.DROP_FFN, idx, rate)
    ok, got = agreement_ok(k[:-1], k[1:], rate)
    assert ok, ("neighbours", got)


def test_rate_0_keeps_everything_and_rate_1_drops_everything():
    idx = np.arange(N)
    for site in DR.SITES:
        assert DR.keep(7, site, idx, 0.0).all()
        assert not DR.keep(7, site, idx, 1.0).any()
    assert DR.scale(0.0) == 1.0 and DR.scale(1.0) == 0.0 and DR.scale(0.5) == 2.0


def test_rates_below_2_pow_minus_24_follow_the_float32_comparison():
    idx = 4321
    zero = DR.seed_for(DR.DROP_FC, idx, 0x00000000FFFFFFFF)     # u == 0 exactly at idx
    tiny = DR.seed_for(DR.DROP_FC, idx, 1 << 40)                 # u == 2**-24, the smallest non-zero u
    assert DR.uniform(zero, DR.DROP_FC, idx) == 0.0
    assert DR.uniform(tiny, DR.DROP_FC, idx) == np.float32(2.0 ** -24)
    for rate in (2.0 ** -25, 1e-30, 2.0 ** -24 * 0.999):
        assert np.float32(rate) > 0
        assert not DR.keep(zero, DR.DROP_FC, idx, rate)          # u = 0 < rate: the only value such a rate drops
        assert DR.keep(tiny, DR.DROP_FC, idx, rate)
    assert np.float32(1e-46) == 0                                # rounds to 0 in float32: keeps even u = 0
    assert DR.keep(zero, DR.DROP_FC, idx, 1e-46)
    assert DR.keep(zero, DR.DROP_FC, idx, 0.0)
    assert not DR.keep(tiny, DR.DROP_FC, idx, 2.0 ** -23)
    assert DR.keep(tiny, DR.DROP_FC, idx, 2.0 ** -24)           # u >= rate: equality keeps
    # every other element of that seed survives a rate below 2**-24
    u = DR.uniform(zero, DR.DROP_FC, np.arange(N))
    k = DR.keep(zero, DR.DROP_FC, np.arange(N), 2.0 ** -25)
    assert u[idx] == 0 and np.array_equal(k, u > 0)


def test_rate_boundary_keeps_equality():
    idx = 99
    half = DR.seed_for(DR.DROP_ATTN, idx, 1 << 63)                # u == 0.5 exactly
    below = DR.seed_for(DR.DROP_ATTN, idx, (1 << 63) - (1 << 40))  # u == 0.5 - 2**-24
    assert DR.keep(half, DR.DROP_ATTN, idx, 0.5)
    assert not DR.keep(below, DR.DROP_ATTN, idx, 0.5)


def test_layouts_name_the_documented_flat_indices():
    H, B, L = 3, 5, 7
    a = DR.attn_index(H, B, L)
    assert a[2, 4, 6] == (2 * B + 4) * L + 6 and a.ravel().tolist() == list(range(H * B * L))
    r = DR.rows_index(4, 9)
    assert r[3, 8] == 3 * 9 + 8 and r.ravel().tolist() == list(range(36))
    la = DR.label_index(2, 3, 10)
    assert la[1, 2, 9] == (1 * 3 + 2) * 10 + 9 and la.ravel().tolist() == list(range(60))
