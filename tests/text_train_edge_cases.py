"""The case tables of the text encoders' training edge sweep, shared by tests/test_text_train_edges_cpu.py (which proves the
references and the tables without a GPU) and tests/test_text_train_edges_gpu.py (which runs them), with the float64 references of
the cases, computed once per process and shared by the tests that need them.  Nothing a function here returns is modified by a test.

The kernels (csrc/text_train.hip, and the packing and recurrence of csrc/lstm.hip) take far more than the model's configuration
(E = 300, two layers, T <= 100, B <= 256, D = 300, ngram 1..3), so the cases sit where a kernel changes path: the text GCN with
its node rows staged in LDS or read from the table (decided per kernel: the backward's per-wave slot sums make it drop staging much
earlier), D at the wave boundary of the backward's DPP sums (64 | 65 | 320) and below it (the keyed row sum's other path), ngram
0 and 15, clamped ids; the BiLSTM with one layer, embedding widths that are no multiple of 4 or past 320, more than four bursts of
32 output rows, lengths at the bursts' edges and outside [0, T], and the packing kernel's branches past 1024 and 4096 samples; the
keyed row sum past its grid cap of 262144 sorted positions.  Hand-picked, not cross products: every value of every axis appears at
least once (tests/test_text_train_edges_cpu.py asserts it).

Bounds.  The BiLSTM and the text GCN keep the gate tests/test_text_train_gpu.py asserts for the same kernels: GATE = 1e-4 of each
tensor's largest magnitude; no case carries a bound of its own.  The float32-CPU error of every reference (the same autograd in
float32 on the CPU against float64, per tensor; printed by the CPU file) stays at or below a quarter of that gate.  Measured, the
worst tensor of each case relative to its scale: BiLSTM 7.2e-7 (B = 65, T = 33, two layers), 5e-7 to 6e-7 at T = 130 and 230, at
most 6.2e-7 elsewhere; text GCN 1.04e-6 and 9.0e-7 (its output, sums of 100 and of 186 products), at most 7.5e-7 elsewhere -- 0.04 of the quarter
gate at the most, so no case had to be shortened and T = 230 stays.  At rate 0 the text GCN's output is also compared with the eval kernel
at that test's 1e-6, on the cases whose documents have at most 40 nodes: the two kernels add a document's nodes in different
orders, and at 100 and 186 nodes two fp32 orders differ by 1.02e-6 and 1.04e-6 of the output's scale (measured on the GPU; the
float32-CPU error of the reference's output there is 1.04e-6 and 9.0e-7), which fp32 itself cannot hold to 1e-6 -- so the long-document cases run
at rate 0.5 and are compared with the float64 oracle alone.  The keyed row sum is bounded by fp32 summation alone, from the
reference: run length x 2^-24 x the largest magnitude among the run's rows (see KS_CASES for the run lengths this holds at); the
gather is exact.  No bound is set from what a kernel returns.  (The ReLU signs of the text GCN's reference come from the kernel's
saved pre-dropout sum, as in tests/test_text_train_gpu.py: that decides a branch, it is
not a bound.)"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from mgnns_amd import synth
from tests import dropout_ref as DR
from tests.test_text_train_cpu import lstm_keep, textgcn_keep, tg_winners

GATE = 1e-4              # of each tensor's largest magnitude (tests/test_text_train_gpu.py)
HID = 150
LDS = 160 * 1024
TINY_RATE = 2.0 ** -25   # below the masks' 24-bit resolution: keeps everything, scale 1 / (1 - rate) == 1 in float32


# ---- references: the BiLSTM ---------------------------------------------------------------------------------------------------------
def _lstm_dir(x, lens, wih, whh, bih, bhh, reverse):
    """One direction over padded x [B, T, K] with packed semantics: a chain runs over its own length only."""
    B, T_len, _ = x.shape
    h = x.new_zeros(B, whh.shape[1])
    c = x.new_zeros(B, whh.shape[1])
    outs = [None] * T_len
    for t in (range(T_len - 1, -1, -1) if reverse else range(T_len)):
        m = (lens > t).to(x.dtype).unsqueeze(1)
        z = x[:, t] @ wih.T + bih + h @ whh.T + bhh
        i, f, g, o = z.chunk(4, 1)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h2 = torch.sigmoid(o) * torch.tanh(c2)
        c = m * c2 + (1 - m) * c
        h = m * h2 + (1 - m) * h
        outs[t] = h2 * m
    return torch.stack(outs, 1)


def lstm_oracle(tok, lens, emb, flat, seed, rate, num_layers=2):
    """Bank of the packed BiLSTM of 1 or 2 layers in the dtype of its leaves: emb [V, E] and flat (8 tensors per layer: (w_ih, w_hh,
    b_ih, b_hh) of the forward, then of the reverse direction).  Lengths are clamped to [0, T] and ids as the kernels clamp them
    (< 0 -> 0, >= V -> V - 1); embedding with padding_idx 0 (row 0 is read but gets no gradient).  Between the layers the site-5 mask
    times dropout_ref's scale (1 / (1 - rate) in float32; 0 at rate 1)."""
    B, T_len = tok.shape
    tok = tok.clamp(0, emb.shape[0] - 1)
    lens = lens.clamp(0, T_len)
    x = F.embedding(tok, emb, padding_idx=0)
    for layer in range(num_layers):
        w = flat[8 * layer:8 * layer + 8]
        x = torch.cat([_lstm_dir(x, lens, *w[:4], False), _lstm_dir(x, lens, *w[4:], True)], 2)
        if layer + 1 < num_layers:
            keep = torch.from_numpy(lstm_keep(seed, rate, B, T_len, 2 * w[1].shape[1]))
            x = x * keep.to(x.dtype) * float(DR.scale(rate))
    return x


# ---- references: the text GCN --------------------------------------------------------------------------------------------------------
def clamp_ids(tok, V):
    """Token ids as tg_setup and lstm_fill_kernel clamp them: negative -> 0 (PAD), >= V -> V - 1."""
    return np.clip(np.asarray(tok, dtype=np.int64), 0, V - 1)


def tg_oracle(tok, nh32, ew32, pmi, ngram, max_length, presum, seed, rate, winners=None, dtype=torch.float64):
    """Output and (node_hidden, edge weight) gradient leaves in `dtype`: winners from the fp32 products (tg_winners of
    tests/test_text_train_cpu.py; ids clamped first, a clamped-to-PAD id dropped like any PAD), ReLU signs from `presum` (the
    kernel's fp32 sum), any D, ngram from 0.  winners: the per-document tg_winners results, when the caller has them."""
    nh = torch.from_numpy(nh32).to(dtype).requires_grad_()
    ew = torch.from_numpy(ew32).to(dtype).requires_grad_()
    V, D = nh32.shape
    tok = clamp_ids(tok, V)
    B = tok.shape[0]
    keep = torch.from_numpy(textgcn_keep(seed, rate, B, D)).to(dtype) * float(DR.scale(rate))
    rows = []
    for b in range(B):
        nodes, win, eid, t = winners[b] if winners is not None else tg_winners(tok[b], nh32, ew32, pmi, ngram, max_length)
        s = nh.new_zeros(D)
        for k in range(len(nodes)):
            src = torch.from_numpy(np.asarray(t, np.int64)[win[k]])
            s = s + ew[torch.from_numpy(eid[k])] * nh[src, torch.arange(D)]
        rows.append(s)
    y = torch.stack(rows) * keep
    sign = (presum.cpu() * keep.float() > 0).to(dtype)
    return y * sign, nh, ew


# ---- the text GCN's shape predicate, restated (csrc/text_train.hip: tg_lds, tg_check, mgnns_textgcn_train_supported) ---------------------
def tg_lds(Tm, W, D, stage, parts):
    """Dynamic LDS of a text GCN training kernel in bytes: the staged node rows, the band's weights and edge ids, three int rows and
    four ints, and (parts: the backward) five waves of per-slot sums."""
    return (Tm * D * 4 if stage else 0) + Tm * W * 8 + (3 * Tm + 4) * 4 + (5 * Tm * W * 4 if parts else 0)


def tg_staged(Tm, ngram, D, parts):
    """Whether the forward (parts false) or the backward (parts true) stages the node rows in LDS."""
    return tg_lds(Tm, 2 * ngram + 1, D, True, parts) <= LDS


def tg_train_ok(T, D, ngram, max_length):
    """mgnns_textgcn_train_supported: the backward's limits."""
    if not (T > 0 and 0 < D <= 320 and 0 <= ngram <= 15 and max_length > 0):
        return False
    Tm, W = min(T, max_length), 2 * ngram + 1
    if Tm * W >= 32768:
        return False
    return tg_lds(Tm, W, D, False, True) <= LDS


def tg_tm_max(ngram):
    """The largest min(T, max_length) a training step takes at `ngram`, by the formula."""
    W = 2 * ngram + 1
    return min((LDS - 16) // (28 * W + 12), (32768 - 1) // W)


def tg_eval_fits(Tm, D, ngram):
    """Whether the EVAL kernel (mgnns_textgcn_fwd, csrc/textgcn.hip), which always stages its node rows, takes the shape: the rate-0
    comparison with it runs where it does."""
    D4 = (D + 3) // 4
    C = min(1024 // D4, 16)
    return (Tm * 4 * D4 + C * 4 * D4 + Tm * (2 * ngram + 1)) * 4 + (3 * Tm + 4) * 4 <= LDS


# ---- BiLSTM training cases -------------------------------------------------------------------------------------------------------------
# lens: "full" | "edges" cycling 0, 1, T | "flush" cycling 31, 32, 33, 64, 65 (the edges of the recurrence's bursts of 32 output rows)
# | "clamped" cycling T + 5, -3, (T + 1) // 2, T (the run must equal the pre-clamped one bit for bit) | "efml" random with the first,
# the middle and the last sample empty.  ids: "pad" in range with PAD inside a length | "oob" as "pad" plus one id V, one V + 7 and one
# -3 inside a length (the run must equal the pre-clamped one bit for bit).
Lstm = collections.namedtuple("Lstm", "B T E layers lens ids rate")
LSTM_V = 50
LSTM_CASES = [
    Lstm(1, 1, 300, 2, "full", "pad", 0.0),
    Lstm(2, 2, 1, 1, "full", "pad", 0.0),
    Lstm(7, 33, 7, 2, "edges", "oob", 0.5),
    Lstm(7, 130, 304, 2, "flush", "pad", 0.0),                  # five bursts
    Lstm(2, 230, 324, 1, "flush", "pad", 0.0),                  # one layer: no mid / mid_d anywhere
    Lstm(2, 230, 300, 2, "full", "pad", 0.5),                   # eight bursts, the longest chains
    Lstm(7, 33, 300, 2, "clamped", "pad", 0.5),
    Lstm(65, 33, 7, 2, "efml", "oob", 0.0),
    Lstm(7, 33, 300, 2, "full", "pad", 1.0),                    # layer 0 and the embedding get exactly zero
    Lstm(7, 33, 300, 2, "edges", "pad", TINY_RATE),             # == rate 0 bit for bit
    Lstm(65, 130, 1, 1, "flush", "oob", 0.0),
    Lstm(1025, 2, 7, 2, "edges", "pad", 0.5),                   # lstm_pack_kernel: the serial-chunk scan
    Lstm(4097, 2, 300, 1, "clamped", "oob", 0.0),               # ... with the lengths read back from offs
]


def lstm_id(c):
    return "B%d-T%d-E%d-L%d-%s-%s-r%g" % c


def _lstm_lens(c, rs):
    B, T = c.B, c.T
    cyc = {"full": [T], "edges": [0, 1, T], "flush": [31, 32, 33, 64, 65], "clamped": [T + 5, -3, (T + 1) // 2, T]}
    if c.lens in cyc:
        return np.array([cyc[c.lens][i % len(cyc[c.lens])] for i in range(B)], dtype=np.int64)
    lens = rs.randint(1, T + 1, size=B).astype(np.int64)
    lens[[0, B // 2, B - 1]] = 0
    return lens


@functools.lru_cache(maxsize=None)
def lstm_data(c):
    """Lstm -> dict: tok / lens as the case passes them, tok_c / lens_c pre-clamped, the nn.LSTM's state_dict `sd` and emb [V, E]
    (float32), the cotangent G [B, T, 2H], torch_seed (torch.manual_seed(torch_seed) before the forward makes train.draw_seed return
    `seed`, the kernels' dropout seed) and oob = the (b, t) of the out-of-range ids."""
    from mgnns_amd import train
    B, T, V = c.B, c.T, LSTM_V
    n = LSTM_CASES.index(c)
    rs = np.random.RandomState(1000 + n)
    lens = _lstm_lens(c, rs)
    lens_c = np.clip(lens, 0, T)
    tok = rs.randint(1, 40, size=(B, T)).astype(np.int64)          # a small alphabet: tokens repeat across samples; rows 40 .. never occur
    if T > 1:
        tok[:, ::7] = 0                                             # PAD inside a length: row 0 must get no gradient
    for b in range(B):
        tok[b, lens_c[b]:] = 0
    oob = []
    if c.ids == "oob":
        where = [(b, int(lens_c[b]) - 1) for b in range(B) if lens_c[b] >= 1][:3]
        assert len(where) == 3, "the case has no three samples to carry the out-of-range ids"
        for (b, t), v in zip(where, (V, V + 7, -3)):
            tok[b, t] = v
        oob = where
    torch_seed = 77 + n
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(torch_seed)
        seed = train.draw_seed()
        torch.manual_seed(500 + n)
        lstm = torch.nn.LSTM(c.E, HID, c.layers, bidirectional=True, batch_first=True)
        emb = torch.nn.Embedding(V, c.E, padding_idx=0)
        G = torch.randn(B, T, 2 * HID)
    return dict(tok=torch.from_numpy(tok), lens=torch.from_numpy(lens), tok_c=torch.from_numpy(np.clip(tok, 0, V - 1)),
                lens_c=torch.from_numpy(lens_c), sd={k: v.detach().clone() for k, v in lstm.state_dict().items()},
                emb=emb.weight.detach().clone(), G=G, seed=seed, torch_seed=torch_seed, oob=oob)


def lstm_flat_names(layers):
    return ["%s_l%d%s" % (n, l, s) for l in range(layers) for s in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def lstm_run_ref(c, dtype, rate=None):
    """[bank, d embedding, d weight ...] (8 weights per layer, lstm_flat_names order) of the oracle in `dtype` on the CPU, under the
    cotangent G.  rate: the case's unless given."""
    d = lstm_data(c)
    emb = d["emb"].to(dtype).requires_grad_()
    flat = [d["sd"][k].to(dtype).requires_grad_() for k in lstm_flat_names(c.layers)]
    bank = lstm_oracle(d["tok"], d["lens"], emb, flat, d["seed"], c.rate if rate is None else rate, c.layers)
    (bank * d["G"].to(dtype)).sum().backward()
    return [bank.detach(), emb.grad] + [p.grad for p in flat]


@functools.lru_cache(maxsize=None)
def lstm_ref(c):
    """The float64 reference of the case (lstm_run_ref)."""
    return lstm_run_ref(c, torch.float64)


def lstm_names(c):
    return ["bank", "embedding"] + lstm_flat_names(c.layers)


# ---- text GCN training cases -------------------------------------------------------------------------------------------------------------
# docs: one kind per document -- "empty" | "one" token | "repeat" one token T times (a single node with T occurrences) | "distinct" |
# "padin" PAD inside | "tie" the forced cross-token tie of tests/test_text_train_gpu.py | "random" (with repeats) | "oob" ids V, V + 7 and
# -1 inside (the run must equal the pre-clamped one bit for bit; row V - 1 carries the gradient) -- or "big": 256 documents, four long
# and the rest of at most three tokens, whose B * Tm * (2 ngram + 1) = 793600 band slots drive the edge-weight keyed sum past its grid cap.
Tg = collections.namedtuple("Tg", "B T max_length ngram D docs rate")
TG_V = 200
TG_CASES = [
    Tg(4, 12, 100, 1, 300, ("empty", "one", "padin", "tie"), 0.0),                 # both kernels staged
    Tg(4, 30, 20, 3, 7, ("repeat", "distinct", "padin", "oob"), 0.0),              # max_length < T
    Tg(3, 100, 100, 15, 320, ("distinct", "repeat", "random"), 0.5),               # forward staged, backward unstaged
    Tg(3, 130, 130, 1, 320, ("distinct", "random", "empty"), 0.5),                 # both unstaged (past the eval kernel's limit)
    Tg(2, 186, 200, 15, 65, ("distinct", "random"), 0.5),                          # the backward's largest Tm at ngram 15
    Tg(4, 40, 40, 0, 64, ("repeat", "distinct", "oob", "one"), 0.0),               # ngram 0: every node its own single in-edge
    Tg(4, 33, 100, 3, 1, ("random", "repeat", "padin", "empty"), 0.0),
    Tg(4, 33, 100, 1, 63, ("random", "tie", "oob", "distinct"), 0.5),
    Tg(256, 100, 100, 15, 8, "big", 0.5),
]
# (the pair of kernels' staging the case must have: forward, backward)
TG_STAGING = {0: (True, True), 2: (True, False), 3: (False, False), 4: (True, False)}

# refusals, each at its limit + 1: (what, T, D, ngram, max_length, a piece of the message)
TG_REFUSALS = [
    ("D 321", 8, 321, 1, 100, "D=321 unsupported"),
    ("ngram 16", 8, 300, 16, 100, "ngram=16 unsupported"),
    ("max_length 0", 8, 300, 1, 0, "max_length=0"),
    ("Tm past the backward's LDS at ngram 0", 4096, 4, 0, 10000, "the backward needs"),
    ("Tm past the backward's LDS at ngram 15", 187, 4, 15, 187, "the backward needs"),
]


def tg_id(c):
    return "B%d-T%d-ml%d-g%d-D%d-%s-r%g" % (c.B, c.T, c.max_length, c.ngram, c.D, c.docs if isinstance(c.docs, str) else "+".join(c.docs), c.rate)


def _tg_doc(kind, T, V, rs):
    row = np.zeros(T, np.int64)
    if kind == "one":
        row[0] = 5
    elif kind == "repeat":
        row[:] = 11
    elif kind == "distinct":
        row[:] = rs.permutation(np.arange(2, V))[:T]
    elif kind in ("random", "padin", "tie", "oob", "short"):
        n = T if kind != "short" else rs.randint(0, 4)
        row[:n] = rs.randint(1, V, size=n)
        row[3:n:5] = row[1:n:5][:len(row[3:n:5])]                   # repeated tokens
        if kind == "padin":
            row[[2, 5]] = 0
            row[rs.randint(T // 2, T):] = 0
        elif kind == "tie":
            row[:3] = (7, 9, 8)
        elif kind == "oob":
            row[[1, 3, 4]] = (V, V + 7, -1)
    else:
        assert kind == "empty", kind
    return row


@functools.lru_cache(maxsize=None)
def tg_data(c):
    """Tg -> dict: tok [B, T] as the case passes it and tok_c pre-clamped (numpy int64), nh [V, D] and ew [count] float32 (rows 7 and 8
    of nh identical and the edges 7 -> 9 and 8 -> 9 given one weight: the forced tie), pmi / count, the cotangent G [B, D], seed, and
    winners = tg_winners of every document (the slow, pure-Python part of the reference)."""
    n = TG_CASES.index(c)
    rs = np.random.RandomState(2000 + n)
    V = TG_V
    pmi, count = synth.synth_pmi(V, per_row=V // 4, seed=n)
    nh = rs.randn(V, c.D).astype(np.float32)
    ew = (rs.randn(count) * 1.3 + 0.2).astype(np.float32)           # non-unit and negative weights
    nh[8] = nh[7]
    ew[pmi[8, 9]] = ew[pmi[7, 9]]
    kinds = (["random"] * 4 + ["short"] * (c.B - 4)) if c.docs == "big" else list(c.docs)
    assert len(kinds) == c.B
    tok = np.stack([_tg_doc(k, c.T, V, rs) for k in kinds])
    tok_c = clamp_ids(tok, V)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(600 + n)
        G = torch.randn(c.B, c.D)
    winners = [tg_winners(tok_c[b], nh, ew, pmi, c.ngram, c.max_length) for b in range(c.B)]
    return dict(tok=tok, tok_c=tok_c, nh=nh, ew=ew, pmi=pmi, count=count, G=G, seed=4242 + n, winners=winners, kinds=kinds)


def tg_run_ref(c, dtype, presum=None):
    """[out, d node_hidden, d edge weights] of tg_oracle in `dtype` under the cotangent G.  presum None: the ReLU signs come from the
    float64 sums themselves (the CPU file's use; the GPU file passes the kernel's saved sums)."""
    d = tg_data(c)
    if presum is None:
        with torch.no_grad():
            ones = torch.ones(c.B, c.D)
            presum = tg_oracle(d["tok"], d["nh"], d["ew"], d["pmi"], c.ngram, c.max_length, ones, d["seed"], 0.0, d["winners"])[0].float()
    out, nh, ew = tg_oracle(d["tok"], d["nh"], d["ew"], d["pmi"], c.ngram, c.max_length, presum, d["seed"], c.rate, d["winners"], dtype)
    (out * d["G"].to(dtype)).sum().backward()
    return [out.detach(), nh.grad, ew.grad]


# ---- keyed row sum and gather cases (direct) -------------------------------------------------------------------------------------------------
# patterns: "single" one run of all M rows | "distinct" every key its own | "span" a run of 300 rows from sorted position 262144 - 150
# on, across the grid cap, behind runs of two and in front of runs of one | "skip" keys below skip_below = 3 among the others | "oob" keys
# n_out and n_out + 3 among the others (ignored).
# The bound -- run length x 2^-24 x the largest magnitude among the run's rows -- is exact arithmetic for runs of one (no rounding) and
# of two (one rounding of a sum of at most twice that magnitude); for a long run of independent standard normal rows it is the size of
# the fp32 rounding walk (about 0.4 x run length x 2^-24 x sigma) with a factor of ten to spare.  It is NOT a worst-case bound for short
# runs of three to a few dozen rows (three rows near the largest magnitude, of one sign, may err by 5/3 of it), so the tables hold no
# such runs: every run here has one row, two rows, or at least 300.
KS_CAP = 262144
Ks = collections.namedtuple("Ks", "D M pattern")
KS_CASES = [
    Ks(1, 300000, "single"),
    Ks(2, 262145, "distinct"),
    Ks(63, 300000, "span"),
    Ks(64, 262144, "skip"),
    Ks(2, 300000, "oob"),
    Ks(257, 1, "single"),
    Ks(257, 1, "oob"),
    Ks(63, 262145, "skip"),
]


@functools.lru_cache(maxsize=None)
def ks_data(c):
    """Ks -> dict: keys [M] int64 (unsorted), values [M, D] float32, n_out, skip_below, and from the float64 segmented sum ref
    [n_out, D], bound [n_out, 1] = run length x 2^-24 x the largest magnitude among the run's rows, hit [n_out] bool (a key lands)."""
    rs = np.random.RandomState(3000 + KS_CASES.index(c))
    M, skip = c.M, 0
    if c.pattern == "single":
        keys, n_out = np.full(M, 3, np.int64), 5
    elif c.pattern == "distinct":
        keys, n_out = rs.permutation(M).astype(np.int64), M
    elif c.pattern == "span":
        lo, hi = KS_CAP - 150, KS_CAP + 150
        keys = np.concatenate([np.arange(lo) // 2, np.full(hi - lo, lo // 2 + 1), lo // 2 + 2 + np.arange(M - hi)]).astype(np.int64)
        n_out = int(keys.max()) + 2                                 # the last row of out has no key
        keys = keys[rs.permutation(M)]
    elif c.pattern == "skip":
        keys, n_out, skip = rs.randint(-2, 40, size=M).astype(np.int64), 41, 3
    else:
        keys, n_out = (rs.randint(0, 24, size=M) if M > 1 else np.array([23])).astype(np.int64), 20
        if M > 1:
            keys[:2] = (20, 23)
    vals = rs.standard_normal((M, c.D)).astype(np.float32)
    ok = (keys >= skip) & (keys < n_out)
    ref = np.zeros((n_out, c.D))
    np.add.at(ref, keys[ok], vals[ok].astype(np.float64))
    runs = np.bincount(keys[ok], minlength=n_out)
    big = np.zeros(n_out)
    np.maximum.at(big, keys[ok], np.abs(vals[ok]).max(axis=1).astype(np.float64))
    return dict(keys=torch.from_numpy(keys), vals=torch.from_numpy(vals), n_out=n_out, skip=skip, ref=torch.from_numpy(ref),
                bound=torch.from_numpy(runs * 2.0 ** -24 * big)[:, None], hit=torch.from_numpy(runs > 0), runs=runs)


# (K, M): the index list holds -1 and n_src among its entries wherever M allows
GATHER_CASES = [(1, 1000), (300, 0), (301, 1), (300, 1000), (301, 1000), (1, 1), (1, 0)]
GATHER_N_SRC = 37
