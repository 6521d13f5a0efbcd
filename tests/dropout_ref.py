"""Host restatement of the training kernels' dropout masks, written from the documented rule and not from the device code:
element `idx` of site `site` is kept iff u >= rate, where u is the top 24 bits of the splitmix64 finaliser of
seed + 0x9E3779B97F4A7C15 * ((site << 48) + idx + 1) (all mod 2**64) divided by 2**24, compared in float32.  Kept values are
scaled by 1 / (1 - rate), and by 0 at rate 1.

The layout functions name the flat index each site draws at (ops.dropout_mask's docstring), so a test can ask for the mask of
head h, sample b, position l instead of trusting the mask a kernel reports about itself."""
import numpy as np

DROP_ATTN, DROP_FC, DROP_FFN, DROP_LABEL_ATTN, DROP_HEAD = 0, 1, 2, 3, 4
SITES = (DROP_ATTN, DROP_FC, DROP_FFN, DROP_LABEL_ATTN, DROP_HEAD)

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
U = np.uint64


def _mix(z):
    z = (z ^ (z >> U(30))) * U(C1)
    z = (z ^ (z >> U(27))) * U(C2)
    return z ^ (z >> U(31))


def hash64(seed, site, idx):
    """The 64-bit finaliser output for element(s) idx (array-like of non-negative ints)."""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):                # arithmetic mod 2**64 is the point
        base = (U(site) << U(48)) + idx + U(1)
        return _mix(U(int(seed) & M64) + U(GOLDEN) * base)


def uniform(seed, site, idx):
    """u in [0, 1) with 24 bits, as float32 (exact)."""
    return (hash64(seed, site, idx) >> U(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep(seed, site, idx, rate):
    """bool array: kept iff u >= rate, the rate rounded to float32 as the C ABI receives it."""
    return uniform(seed, site, idx) >= np.float32(rate)


def scale(rate):
    rate = np.float32(rate)
    return np.float32(1.0) / (np.float32(1.0) - rate) if rate < 1.0 else np.float32(0.0)


# ---- flat layouts of the sites --------------------------------------------------------------------------------------------
def attn_index(H, B, L):
    """DROP_ATTN over [H*B, 1, L]: idx = (h*B + b)*L + l, returned as [H, B, L]."""
    h, b, l = np.meshgrid(np.arange(H), np.arange(B), np.arange(L), indexing="ij")
    return (h * B + b) * L + l


def rows_index(B, D):
    """DROP_FC, DROP_FFN and DROP_HEAD over [B, D]: idx = b*D + d."""
    b, d = np.meshgrid(np.arange(B), np.arange(D), indexing="ij")
    return b * D + d


def label_index(B, NLQ, hid):
    """DROP_LABEL_ATTN over [B, NLQ, hid]: idx = (b*NLQ + n)*hid + j."""
    b, n, j = np.meshgrid(np.arange(B), np.arange(NLQ), np.arange(hid), indexing="ij")
    return (b * NLQ + n) * hid + j


def attn_keep(seed, rate, H, B, L):
    """[H*B, 1, L] bool, the layout ops.mha_attn_train returns."""
    return keep(seed, DROP_ATTN, attn_index(H, B, L), rate).reshape(H * B, 1, L)


def rows_keep(seed, site, rate, B, D):
    return keep(seed, site, rows_index(B, D), rate)


def label_keep(seed, rate, B, NLQ, hid):
    return keep(seed, DROP_LABEL_ATTN, label_index(B, NLQ, hid), rate)


# ---- seeds that put a chosen value at a chosen element (the finaliser is a bijection) -------------------------------------
def _unxorshift(y, s):
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x & M64


def seed_for(site, idx, out):
    """The seed for which hash64(seed, site, idx) == out."""
    z = out & M64
    z = _unxorshift(z, 31)
    z = (z * pow(C2, -1, 1 << 64)) & M64
    z = _unxorshift(z, 27)
    z = (z * pow(C1, -1, 1 << 64)) & M64
    z = _unxorshift(z, 30)
    return (z - GOLDEN * (((site << 48) + idx + 1) & M64)) & M64
