"""Operator wrappers: torch CUDA tensors in, torch CUDA tensors out, all arithmetic in
libmgnns_hip.so on the caller's current stream.  Shape / dtype / device / contiguity are
validated here (the reference's convention is Python exceptions); nothing in this file
computes.
"""
import os

import torch

from . import _lib
from .derived import derived

_C = _lib.CONSTANTS           # the #defines of include/mgnns_hip.h
ACT_NONE, ACT_RELU, ACT_LRELU2 = _C["MGNNS_ACT_NONE"], _C["MGNNS_ACT_RELU"], _C["MGNNS_ACT_LRELU2"]
BANK_LD = 320      # bf16 memory banks are [B, L, 320]: model dim 300 zero padded to 10 MFMA k-steps of 32


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Scratch buffers of the persistent launches are keyed by (capture epoch, launch stream): eager launches on one stream
# are ordered and may share a scratch; every hipGraph capture takes a fresh epoch (mgnns_amd/graph.py), because a captured
# graph can be replayed on any stream next to any other graph of the same model.
_SCRATCH_EPOCH = 0


def new_scratch_epoch():
    global _SCRATCH_EPOCH
    _SCRATCH_EPOCH += 1
    return _SCRATCH_EPOCH


def set_scratch_epoch(e):
    global _SCRATCH_EPOCH
    prev, _SCRATCH_EPOCH = _SCRATCH_EPOCH, int(e)
    return prev


def _scratch_key():
    return (_SCRATCH_EPOCH, _stream())


# Every scratch slot created under a capture epoch is remembered, so that the capture's owner (graph.GraphedForward) can drop
# them when it goes: slot dicts would otherwise pin a slice of the zero pool per (capture, launch) for the life of the process.
_EPOCH_SLOTS = {}


def _scratch_slot_put(slot, key, ws):
    slot[key] = ws
    if key[0]:
        _EPOCH_SLOTS.setdefault(key[0], []).append((slot, key))


def release_scratch_epoch(epoch):
    """Forget the scratch buffers created under `epoch` (its graphs are gone: nothing holds their addresses any more)."""
    for slot, key in _EPOCH_SLOTS.pop(int(epoch), []):
        slot.pop(key, None)


# The layer-level park ("Derived packs and launch scratch"): while any capture is alive, a superseded entry of a
# fusion.py layer cache or an LstmCache is kept here instead of being freed; it empties when the last capture goes.
_LIVE_CAPTURES = 0
_RETIRED = []


def capture_born():
    global _LIVE_CAPTURES
    _LIVE_CAPTURES += 1


def capture_gone():
    global _LIVE_CAPTURES
    if _LIVE_CAPTURES > 0:
        _LIVE_CAPTURES -= 1
    if _LIVE_CAPTURES == 0:
        _RETIRED.clear()


def retire(obj):
    """Park a superseded cache entry while a capture that may hold its addresses is alive."""
    if obj is not None and _LIVE_CAPTURES > 0:
        _RETIRED.append(obj)


# Counters of the persistent / cluster launches start at zero and are left at zero by the kernels themselves (the last
# workgroup re-arms them).  They come out of a pool that is zeroed OUTSIDE any capture: a torch.zeros inside a capture is a
# fill node of the graph -- a 5-8 us launch in front of the kernel on every replay (13 of them per forward, most on the
# bank -> tail -> stack chains).  Slices are handed out once and never reused.
_ZERO_POOL = {}
_ZERO_CHUNK = 64 << 20


def _capturing():
    return torch.cuda.is_current_stream_capturing()


def reserve_zeros(device, nbytes=24 << 20):
    """Make sure the zero pool of `device` has nbytes left (call outside a capture, e.g. right before one)."""
    device = torch.device(device)
    pool = _ZERO_POOL.get(device)
    if (pool is None or pool[1] + nbytes > pool[0].numel()) and not _capturing():
        buf = torch.zeros(max(_ZERO_CHUNK, nbytes), dtype=torch.uint8, device=device)
        torch.cuda.current_stream(device).synchronize()           # zero before any stream uses a slice
        _ZERO_POOL[device] = [buf, 0]


def zeros_bytes(nbytes, device):
    """nbytes of zeroed device memory (256-B aligned) that the caller's kernels keep zero between launches."""
    device = torch.device(device)
    n = (int(nbytes) + 255) // 256 * 256
    pool = _ZERO_POOL.get(device)
    if pool is None or pool[1] + n > pool[0].numel():
        if _capturing():                                          # pool exhausted inside a capture: a fill node, still correct
            return torch.zeros(n, dtype=torch.uint8, device=device)
        reserve_zeros(device, max(n, 24 << 20))
        pool = _ZERO_POOL[device]
    t = pool[0][pool[1]:pool[1] + n]
    pool[1] += n
    return t


def zeros_i32(n, device):
    return zeros_bytes(4 * n, device).view(torch.int32)[:n]


def _scratch_slot(packed, name, fits, make):
    """The scratch of one persistent / cluster launch: packed[name][_scratch_key()], made by make() when there is none or when
    fits(it) -- big enough, on the launch's device -- says no.  make() takes counters from the zero pool (zeros_bytes /
    zeros_i32; a torch.zeros would be a fill node inside a capture).  A superseded buffer goes to packed["_retired"] and
    is never freed while the pack lives: a captured hipGraph may still hold its address.  -> (key, scratch)"""
    slot = packed.setdefault(name, {})
    key = _scratch_key()
    ws = slot.get(key)
    if ws is None or not fits(ws):
        if ws is not None:
            packed.setdefault("_retired", []).append(ws)
        ws = make()
        _scratch_slot_put(slot, key, ws)
    return key, ws


def _cluster_scratch(packed, name, device, tiles, floats):
    """(tiles, exchange scratch of floats(tiles) fp32, 2 counters per tile) for a cluster launch over `tiles` 16-sample tiles."""
    return _scratch_slot(packed, name, lambda ws: ws[0] >= tiles and ws[1].device == device,
                         lambda: (tiles, torch.empty(floats(tiles), device=device, dtype=torch.float32),
                                  zeros_i32(2 * tiles, device)))[1]


class KernelTimer:
    """Opt-in per-launch HIP-event timing (bench.py's roofline leg).  Events are recorded on the stream
    the kernels are launched on (PyTorch's current stream), around the C-ABI call only."""

    def __init__(self, names=None):
        self.names = None if names is None else set(names)
        self.events = {}

    def wants(self, name):
        return self.names is None or name in self.names

    def durations_ms(self):
        """{key: [ms, ...]} -- call after torch.cuda.synchronize()."""
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in self.events.items()}


_TIMER = None


def set_timer(timer):
    global _TIMER
    _TIMER = timer


def _launch(name, *args, key=(), alias=None, wanted=None):
    """_lib.call(name, *args), bracketed by events when the timer wants `name`; they are filed under (name,) + key.
    alias: another entry point's name, by which the timer is asked and under which the events are filed instead;
    wanted: the name the timer is asked by, where only that differs."""
    t = _TIMER
    filed = alias or name
    if t is None or not t.wants(wanted or filed):
        return _lib.call(name, *args)
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    _lib.call(name, *args)
    b.record()
    t.events.setdefault((filed,) + key, []).append((a, b))


def _chk(t, name, dtype=torch.float32, ndim=None):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must be %d-d, got shape %s" % (name, ndim, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _p(t):
    return None if t is None else t.data_ptr()


_gemm_ws = {}


def _gemm_workspace(device):
    """K-split scratch of the GEMM kernels: one buffer per (device, stream) so concurrent streams never share."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    buf = _gemm_ws.get(key)
    if buf is None:
        buf = torch.empty(_lib.lib().mgnns_gemm_workspace_bytes(), dtype=torch.uint8, device=device)
        _gemm_ws[key] = buf
    return buf


# ---- nn.Linear / matmul ---------------------------------------------------------------
def linear(x, weight, bias=None, act=ACT_NONE, residual=None):
    """act(x @ weight.T + bias) (+ residual); x [..., K], weight [N, K]."""
    K = x.shape[-1]
    x2 = _chk(x.reshape(-1, K), "x")
    _chk(weight, "weight", ndim=2)
    if weight.shape[1] != K:
        raise ValueError("weight %s does not match x[..., %d]" % (tuple(weight.shape), K))
    N = weight.shape[0]
    if bias is not None:
        _chk(bias, "bias", ndim=1)
    y = torch.empty(x2.shape[0], N, device=x.device, dtype=torch.float32)
    if residual is not None:
        residual = _chk(residual.reshape(-1, N), "residual")
        if residual.shape[0] != x2.shape[0]:
            raise ValueError("residual rows mismatch")
    ws = _gemm_workspace(x.device)
    _lib.call("mgnns_linear_fwd", _p(x2), x2.shape[0], K, _p(weight), _p(bias), N, _p(residual), _p(y), act, _p(ws), ws.numel(), _stream())
    return y.view(*x.shape[:-1], N)


def classifier_head(feats, weight, bias):
    """logits = cat(feats, dim=1) @ weight.T + bias for the four fusion features [B, D] (MODEL:560-566), one launch, no cat."""
    if len(feats) != 4:
        raise ValueError("classifier_head takes the four fusion features")
    B, D = feats[0].shape
    for i, f in enumerate(feats):
        _chk(f, "feature %d" % i, ndim=2)
        if tuple(f.shape) != (B, D):
            raise ValueError("feature %d shape %s, expected %s" % (i, tuple(f.shape), (B, D)))
    _chk(weight, "weight", ndim=2)
    _chk(bias, "bias", ndim=1)
    NL = weight.shape[0]
    if weight.shape[1] != 4 * D or bias.shape[0] != NL:
        raise ValueError("weight %s / bias %s do not match four [B,%d] features" % (tuple(weight.shape), tuple(bias.shape), D))
    out = torch.empty(B, NL, device=weight.device, dtype=torch.float32)
    _lib.call("mgnns_classifier_head_fwd", _p(feats[0]), _p(feats[1]), _p(feats[2]), _p(feats[3]), B, D, _p(weight), _p(bias), NL, _p(out),
              _stream())
    return out


def classifier_head_state(B, NL, nparts, device):
    """Buffers of one forward's split classifier head (classifier_head_part): parts [nparts,B,NL], arrival counter (zero),
    logits [B,NL]."""
    return (torch.empty(nparts, B, NL, device=device, dtype=torch.float32), zeros_i32(1, device),
            torch.empty(B, NL, device=device, dtype=torch.float32))


def classifier_head_part(feat, part, nparts, weight, bias, state):
    """This feature's share of logits = cat(feats) @ weight.T + bias (mgnns_classifier_part_fwd): call once per feature, from
    whichever stream produced it; the call that finishes last completes state[2] (the logits)."""
    _chk(feat, "feature", ndim=2)
    _chk(weight, "weight", ndim=2)
    _chk(bias, "bias", ndim=1)
    B, D = feat.shape
    parts, counter, logits = state
    NL = weight.shape[0]
    if weight.shape[1] != nparts * D or tuple(parts.shape) != (nparts, B, NL) or tuple(logits.shape) != (B, NL):
        raise ValueError("classifier_head_part: weight %s / state do not match %d features [B=%d,%d]" % (tuple(weight.shape), nparts, B, D))
    _lib.call("mgnns_classifier_part_fwd", _p(feat), int(part), int(nparts), B, D, _p(weight), _p(bias), NL, _p(parts), _p(counter),
              _p(logits), _stream())
    return logits


def matmul(x, w, act=ACT_NONE):
    """act(x @ w); x [M, K], w [K, N] (GraphConvolution weight layout)."""
    _chk(x, "x", ndim=2)
    _chk(w, "w", ndim=2)
    if x.shape[1] != w.shape[0]:
        raise ValueError("matmul shapes %s x %s" % (tuple(x.shape), tuple(w.shape)))
    y = torch.empty(x.shape[0], w.shape[1], device=x.device, dtype=torch.float32)
    ws = _gemm_workspace(x.device)
    _lib.call("mgnns_matmul_fwd", _p(x), x.shape[0], x.shape[1], _p(w), w.shape[1], _p(y), act, _p(ws), ws.numel(), _stream())
    return y


# ---- adjacency ----------------------------------------------------------------------------
def gen_adj(A, want_csr=False):
    """D^-1/2 A^T D^-1/2 (utils/util.py:421-426).  Returns adj, or (adj, (row_ptr, col, val))."""
    _chk(A, "A", ndim=2)
    C = A.shape[0]
    if A.shape[1] != C:
        raise ValueError("A must be square")
    adj = torch.empty_like(A)
    work = torch.empty(C, device=A.device, dtype=torch.float32)
    rp = col = val = None
    if want_csr:
        rp = torch.empty(C + 1, device=A.device, dtype=torch.int32)
        col = torch.empty(C * C, device=A.device, dtype=torch.int32)
        val = torch.empty(C * C, device=A.device, dtype=torch.float32)
    _lib.call("mgnns_gen_adj", _p(A), C, _p(adj), _p(work), _p(rp), _p(col), _p(val), _stream())
    return (adj, (rp, col, val)) if want_csr else adj


def label_gcn_pack(w1, w2, split):
    """GraphConvolution weights W1 [K0,N1], W2 [N1,N2] ([in,out] layout) -> the packed dict label_gcn() takes:
    split = False: exact-fp32 fragment-major buffers; True: (hi, lo) split-bf16 pairs."""
    _chk(w1, "gc1.weight", ndim=2)
    _chk(w2, "gc2.weight", ndim=2)
    if w1.shape[1] != w2.shape[0]:
        raise ValueError("gc1.weight %s / gc2.weight %s do not chain" % (tuple(w1.shape), tuple(w2.shape)))
    w1t, w2t = w1.t().contiguous(), w2.t().contiguous()               # [N, K]: the layout the pack kernels take
    if split:
        a, b = pack_weight_bf16_split(w1t), pack_weight_bf16_split(w2t)
        d = {"w1": a, "w2": b}
    else:
        d = {"w1": (pack_weight_f32(w1t), None), "w2": (pack_weight_f32(w2t), None)}
    d.update(split=bool(split), K0=w1.shape[0], N1=w1.shape[1], N2=w2.shape[1])
    return d


LABEL_GCN_GRID = 0            # workgroups of the persistent label-GCN launch; 0: by batch size (model.forward_plan)


def label_gcn_memo_flag(memo, want_packed_g=False):
    """The verdict of the last memo launch on the current stream / scratch epoch: 1 = hit (nothing was computed), 0 = miss.
    Synchronises (a test's and a tool's question, not the forward's)."""
    st = memo[_scratch_key() + (bool(want_packed_g),)]
    return int(st["state"][:12].view(torch.int32)[1].item())


def label_gcn(A, inp, packed, want_packed_g=False, query=None, grid=0, memo=None):
    """One channel's whole label GCN in one persistent launch (mgnns_label_gcn_fwd): gen_adj + GraphConvolution x 2 (+ the
    label query projection).  A [C,C]; inp [C,K0]; packed = label_gcn_pack(...) (also carries this channel's scratch);
    query = (label_query [NLQ,K0], w_q.weight [HQ,K0], w_q.bias or None).  -> (G [C,N2], (Gp_hi, Gp_lo) or None, Q or None).
    memo: a dict the CALLER owns for exactly one set of weights (A, packed, query): the outputs then live in it, per (scratch
    epoch, launch stream) like the scratch, and a launch whose inp equals -- bit for bit, decided on the device -- the inp they
    were computed from computes nothing and returns them again (mgnns_label_gcn_memo_fwd).  After changing a weight pass a
    fresh dict.  None: today's launch into fresh outputs."""
    _chk(A, "A", ndim=2)
    _chk(inp, "inp", ndim=2)
    C = A.shape[0]
    if A.shape[1] != C or inp.shape[0] != C or inp.shape[1] != packed["K0"]:
        raise ValueError("A %s / inp %s do not match a [C,C] adjacency and [C,%d] label embeddings" %
                         (tuple(A.shape), tuple(inp.shape), packed["K0"]))
    N1, N2 = packed["N1"], packed["N2"]
    L = _lib.lib()
    need = L.mgnns_label_gcn_scratch_bytes(C, N1, N2)
    # the launch's scratch holds its intermediates and its item queue: one per (capture epoch, launch stream), so that two
    # forwards of one model in flight at once -- two streams, two captured graphs -- never share one
    key, ws = _scratch_slot(packed, "_scratch", lambda ws: ws.numel() >= need and ws.device == A.device,
                            lambda: zeros_bytes(need, A.device)[:need])               # counters (first 256 B) start at zero
    st = None
    if memo is not None and _TIMER is not None and _TIMER.wants("mgnns_label_gcn_fwd"):
        memo = None                      # a timed launch is a computing one: a roofline row of the hit path would say nothing
    if memo is not None:
        mkey = key + (bool(want_packed_g),)
        st = memo.get(mkey)
        if st is None:
            mneed = L.mgnns_label_gcn_memo_bytes(C, packed["K0"])
            st = {"state": zeros_bytes(mneed, A.device)[:mneed]}          # valid = 0: the first launch computes
            _scratch_slot_put(memo, mkey, st)
    if st is not None and "G" in st:
        G, gh, gl = st["G"], st["gh"], st["gl"]
    else:
        G = torch.empty(C, N2, device=A.device, dtype=torch.float32)
        gh = gl = None
        if want_packed_g:
            n = L.mgnns_packed_bf16_weight_bytes(C, N2)
            gh = torch.empty(n, dtype=torch.uint8, device=A.device)
            gl = torch.empty(n, dtype=torch.uint8, device=A.device)
    lq = wq = bq = Q = None
    nlq = hq = 0
    if query is not None:
        lq, wq, bq = query
        _chk(lq, "label_query", ndim=2)
        _chk(wq, "w_q.weight", ndim=2)
        if lq.shape[1] != packed["K0"] or wq.shape[1] != packed["K0"]:
            raise ValueError("label_query %s / w_q.weight %s must be [*, %d]" % (tuple(lq.shape), tuple(wq.shape), packed["K0"]))
        if bq is not None:
            _chk(bq, "w_q.bias", ndim=1)
        nlq, hq = lq.shape[0], wq.shape[0]
        Q = st["Q"] if st is not None and "G" in st else torch.empty(nlq, hq, device=A.device, dtype=torch.float32)
    if st is not None:
        if "G" in st and (Q is None) != (st["Q"] is None):
            raise ValueError("label_gcn: one memo serves one query (present or absent)")
        st.update(G=G, gh=gh, gl=gl, Q=Q)
        mem = st["state"]
        _launch("mgnns_label_gcn_memo_fwd", _p(A), C, _p(inp), packed["K0"], 1 if packed["split"] else 0, _p(packed["w1"][0]),
                _p(packed["w1"][1]), N1, _p(packed["w2"][0]), _p(packed["w2"][1]), N2, _p(G), _p(gh), _p(gl), _p(lq), nlq, _p(wq), _p(bq),
                hq, _p(Q), _p(ws), ws.numel(), _p(mem), mem.numel(), int(grid) or LABEL_GCN_GRID, _stream(), key=(C, packed["split"]),
                alias="mgnns_label_gcn_fwd")
        return G, ((gh, gl) if want_packed_g else None), Q
    _launch("mgnns_label_gcn_fwd", _p(A), C, _p(inp), packed["K0"], 1 if packed["split"] else 0, _p(packed["w1"][0]), _p(packed["w1"][1]),
            N1, _p(packed["w2"][0]), _p(packed["w2"][1]), N2, _p(G), _p(gh), _p(gl), _p(lq), nlq, _p(wq), _p(bq), hq, _p(Q), _p(ws),
            ws.numel(), int(grid) or LABEL_GCN_GRID, _stream(), key=(C, packed["split"]))
    return G, ((gh, gl) if want_packed_g else None), Q


def dense_to_csr(m):
    _chk(m, "adj", ndim=2)
    C = m.shape[0]
    if m.shape[1] != C:
        raise ValueError("adj must be square")
    rp = torch.empty(C + 1, device=m.device, dtype=torch.int32)
    col = torch.empty(C * C, device=m.device, dtype=torch.int32)
    val = torch.empty(C * C, device=m.device, dtype=torch.float32)
    _lib.call("mgnns_dense_to_csr", _p(m), C, _p(rp), _p(col), _p(val), _stream())
    return rp, col, val


def spmm_csr(csr, x, act=ACT_NONE, out=None, bias=None):
    """act(adj @ x [+ bias]) with adj in CSR (row_ptr, col, val); x [C, F].  out: optional preallocated [C, F] result;
    bias: GraphConvolution(bias=True)'s [1,1,F] parameter (MODEL:40-41,55-56), any shape with F elements."""
    rp, col, val = csr
    _chk(rp, "row_ptr", torch.int32, 1)
    _chk(col, "col", torch.int32, 1)
    _chk(val, "val", torch.float32, 1)
    _chk(x, "x", ndim=2)
    n = rp.shape[0] - 1
    if out is None:
        y = torch.empty(n, x.shape[1], device=x.device, dtype=torch.float32)
    else:
        y = _chk(out, "out", ndim=2)
        if tuple(y.shape) != (n, x.shape[1]) or y.data_ptr() == x.data_ptr():
            raise ValueError("out must be a [%d, %d] tensor distinct from x" % (n, x.shape[1]))
    if bias is not None:
        bias = _chk(bias.reshape(-1), "bias", ndim=1)
        if bias.shape[0] != x.shape[1]:
            raise ValueError("bias has %d elements, x has %d features" % (bias.shape[0], x.shape[1]))
        _launch("mgnns_spmm_csr_bias_fwd", _p(rp), _p(col), _p(val), n, _p(x), x.shape[1], _p(bias), _p(y), act, _stream(),
                key=(n, x.shape[1]), wanted="mgnns_spmm_csr_fwd")
        return y
    _launch("mgnns_spmm_csr_fwd", _p(rp), _p(col), _p(val), n, _p(x), x.shape[1], _p(y), act, _stream(), key=(n, x.shape[1]))
    return y


# ---- bf16-feature sparse propagation (BASELINE configs[4]) -------------------------------------------------
def cast_bf16(x):
    """fp32 tensor -> bf16 tensor of the same shape (round to nearest even), on the device."""
    _chk(x, "x")
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    if x.numel() == 0:
        return y
    _lib.call("mgnns_cast_bf16", _p(x), x.numel(), _p(y), _stream())
    return y


class SparseAdjBf16:
    """A static sparse adjacency for `spmm_bf16`: CSR with bf16 values on the device, plus -- for graphs with tens of
    non-zeros per row -- the re-ordered entry stream of the LDS-tiled kernel (mgnns_amd/spmm_plan.py), built once per
    feature width on first use.  csr = (row_ptr int32 [n+1], col int32 [nnz], val fp32 or bf16 [nnz]) device tensors."""

    TILED_MIN_AVG_NNZ = 32.0

    def __init__(self, csr, n_cols=None, sort_rows=True):
        """sort_rows: hand the gather kernels the rows SORTED BY LENGTH (+ the map back to the rows of Y): four rows share a
        wave instruction there, and with Poisson row lengths the longest of four sets the pace (configs[4] at density 4e-4:
        21 -> 16 us).  One-off host work on a static adjacency; every row of Y is computed exactly as before."""
        rp, col, val = csr
        _chk(rp, "row_ptr", torch.int32, 1)
        _chk(col, "col", torch.int32, 1)
        if val.dtype == torch.float32:
            val = cast_bf16(_chk(val, "val", torch.float32, 1))
        _chk(val, "val", torch.bfloat16, 1)
        if val.numel() % 2:                                  # the kernels fetch the values as aligned dwords
            val = torch.cat([val, val.new_zeros(1)])[:-1]    # same values, storage readable one element further
        self.row_ptr, self.col, self.val = rp, col, val
        self.n_rows = rp.shape[0] - 1
        self.n_cols = self.n_rows if n_cols is None else int(n_cols)
        self.nnz = int(col.shape[0])
        self._plans = {}
        self._sort_rows = bool(sort_rows) and self.n_rows > 1
        self._sorted = {}                                    # form -> (row_ptr, col, val, row_map) with rows in order of length

    def sorted_for(self, F):
        """(row_ptr, col, val, row_map) for the gather kernel mgnns_spmm_csr_bf16_fwd picks at feature width F, or None
        (sort_rows=False, or all rows equally long).  Rows go in order of LENGTH -- for the ring form (one slab per XCD:
        a wave owns a CONTIGUOUS range of CSR positions) in quads of equal length dealt out with a stride, because sorted end
        to end the last waves would own all the long rows (measured: 33 us instead of 21); the register form deals rows out
        round robin and takes the plain sort."""
        if not self._sort_rows:
            return None
        form = "reg" if ((F + 127) // 128 + 7) // 8 >= 2 else "ring"      # (variant 0 of mgnns_spmm_csr_bf16_fwd)
        if form not in self._sorted:
            import numpy as np
            rph = self.row_ptr.cpu().numpy().astype(np.int64)
            lens = rph[1:] - rph[:-1]
            hit = None
            if lens.min() != lens.max():
                order = np.argsort(lens, kind="stable")                       # CSR position -> row of Y
                nq = self.n_rows // 4
                if form == "ring" and nq > 8:
                    stride = next(p for p in (389, 397, 401, 409, 419, 421, 431, 433) if nq % p)
                    q = (np.arange(nq, dtype=np.int64) * stride) % nq
                    order = np.concatenate([order[:4 * nq].reshape(nq, 4)[q].reshape(-1), order[4 * nq:]])
                rp2 = np.zeros(self.n_rows + 1, np.int64)
                np.cumsum(lens[order], out=rp2[1:])
                src = np.repeat(rph[:-1][order] - rp2[:-1], lens[order]) + np.arange(self.nnz)      # entry k of the sorted CSR <- entry src[k]
                idx = torch.from_numpy(src).to(self.col.device)
                val2 = self.val[:self.nnz][idx]
                if self.nnz % 2:
                    val2 = torch.cat([val2, val2.new_zeros(1)])[:-1]
                dev = self.row_ptr.device
                hit = (torch.from_numpy(rp2.astype(np.int32)).to(dev), self.col[idx].contiguous(), val2.contiguous(),
                       torch.from_numpy(order.astype(np.int32)).to(dev))
            self._sorted[form] = hit
        return self._sorted[form]

    @classmethod
    def block_diagonal(cls, adjs, **kw):
        """The union of independent graphs as ONE adjacency (rows / columns of graph i shifted by the sizes of graphs 0..i-1):
        act(A_i @ X_i) for every i = one launch on the stacked X -- configs[4]'s three channels (MODEL:460-506 runs the object
        and the scene graph one after the other): the fixed cost of a launch is paid once, 21.8 -> 17.4 us per channel."""
        rps, cols, vals, r0, c0, e0 = [], [], [], 0, 0, 0
        for a in adjs:
            rps.append(a.row_ptr[(1 if rps else 0):] + e0)
            cols.append(a.col + c0)
            vals.append(a.val[:a.nnz])
            r0, c0, e0 = r0 + a.n_rows, c0 + a.n_cols, e0 + a.nnz
        return cls((torch.cat(rps).to(torch.int32), torch.cat(cols).to(torch.int32), torch.cat(vals)), n_cols=c0, **kw)

    @property
    def avg_nnz(self):
        return self.nnz / max(1, self.n_rows)

    def plan(self, F, geometry=None):
        """Device copy of the tiled plan for feature width F (built on the host once; the adjacency is static)."""
        from . import spmm_plan
        geo = tuple(geometry) if geometry is not None else spmm_plan.geometry_for(self.n_rows, F)
        hit = self._plans.get(geo)
        if hit is None:
            bits = self.val.view(torch.int16).cpu().numpy().view("uint16")
            pl = spmm_plan.build_tiled_plan(self.row_ptr.cpu().numpy(), self.col.cpu().numpy(), bits, self.n_cols, *geo)
            dev = self.col.device
            hit = (torch.from_numpy(pl.wave_off.view("int32")).to(dev), torch.from_numpy(pl.ent.view("int32")).to(dev), geo)
            self._plans[geo] = hit
        return hit


def spmm_bf16(adj, x, act=ACT_NONE, out=None, out_dtype=torch.bfloat16, path=None, variant=0, geometry=None):
    """act(adj @ x): adj a SparseAdjBf16, x [n_cols, F] bf16 -> [n_rows, F] bf16 (or fp32), fp32 accumulation.
    path: None (by density) | "direct" | "tiled"."""
    if not isinstance(adj, SparseAdjBf16):
        raise TypeError("adj must be a SparseAdjBf16")
    _chk(x, "x", torch.bfloat16, 2)
    if x.shape[0] != adj.n_cols:
        raise ValueError("x has %d rows, the adjacency %d columns" % (x.shape[0], adj.n_cols))
    F = x.shape[1]
    if out is None:
        y = torch.empty(adj.n_rows, F, device=x.device, dtype=out_dtype)
    else:
        y = out
        if y.dtype not in (torch.bfloat16, torch.float32) or tuple(y.shape) != (adj.n_rows, F) or not y.is_contiguous() \
                or not y.is_cuda or y.data_ptr() == x.data_ptr():
            raise ValueError("out must be a contiguous [%d, %d] bf16 / fp32 device tensor distinct from x" % (adj.n_rows, F))
    ybf = 1 if y.dtype == torch.bfloat16 else 0
    if path is None:
        path = "tiled" if (adj.avg_nnz >= SparseAdjBf16.TILED_MIN_AVG_NNZ and F % 256 == 0) else "direct"
    if path == "tiled":
        wo, ent, geo = adj.plan(F, geometry)
        _launch("mgnns_spmm_tiled_bf16_fwd", _p(wo), _p(ent), geo[0], geo[1], geo[2], adj.n_rows, adj.n_cols, _p(x), F, _p(y), ybf, act,
                _stream(), key=(adj.n_rows, F))
    elif path == "direct":
        rp, col, val, rmap = (adj.sorted_for(F) if int(variant) == 0 else None) or (adj.row_ptr, adj.col, adj.val, None)
        _launch("mgnns_spmm_csr_bf16_fwd", _p(rp), _p(col), _p(val), adj.n_rows, adj.nnz, _p(x), F, _p(y), ybf, act, int(variant), _p(rmap),
                _stream(), key=(adj.n_rows, F))
    else:
        raise ValueError("path must be None, 'direct' or 'tiled'")
    return y


# ---- gathers -------------------------------------------------------------------------------
def embedding(idx, table):
    _chk(idx, "idx", torch.int64)
    _chk(table, "table", ndim=2)
    out = torch.empty(*idx.shape, table.shape[1], device=table.device, dtype=torch.float32)
    _lib.call("mgnns_embedding_fwd", _p(idx), idx.numel(), _p(table), table.shape[0], table.shape[1], _p(out), _stream())
    return out


# ---- text memory bank: embedding + packed BiLSTM -----------------------------------------------------
class LstmCache:
    """Derived forms of one nn.LSTM's weights (per-layer [W_ih ; W_ih_reverse], the packed bf16 layouts), owned by the
    module that owns the weights so their lifetime is the module's (a captured hipGraph bakes these pointers in).  Each
    field is one entry of derived.derived (value at index 2), stored in this object's __dict__."""

    def __init__(self):
        self.cat = None
        self.prepack = None
        self.table = None      # the layer-0 input projection folded into the embedding table


def _lstm_derived(cache, slot, sources, build):
    """cache.<slot>, rebuilt when a source changes and parked by retire(); cache None: built per call, nothing stored."""
    return build() if cache is None else derived(vars(cache), slot, sources, build, park=retire)


def _lstm_cat(weights, num_layers, cache):
    """Per layer [W_ih ; W_ih_reverse] and [b_ih ; b_ih_reverse], rebuilt when a weight changes (one input-projection
    GEMM per layer instead of two)."""
    return _lstm_derived(cache, "cat", [t for tup in weights for t in (tup[0], tup[2])], lambda: [
        (torch.cat([weights[2 * l][0], weights[2 * l + 1][0]], 0).contiguous(),
         torch.cat([weights[2 * l][2], weights[2 * l + 1][2]], 0).contiguous()) for l in range(num_layers)])


# bf16 recurrence: the layer-0 input projection folded into the embedding table once per weight version (mgnns_bilstm_bf16_fold_embedding:
# [V, 8 * hidden] fp32, 97 MB for V = 20 154); MGNNS_LSTM_FOLD=0: the projection GEMM on the gathered rows in every forward
LSTM_FOLD_EMBEDDING = os.environ.get("MGNNS_LSTM_FOLD", "1") != "0"


def _lstm_table(emb_table, cat0, hidden, cache):
    """table[v] = bf16(emb[v]) . bf16(W_ih0)^T + b_ih0 for every vocabulary entry; rebuilt when the embedding or layer 0's input
    weights change.  Superseded tables go to the retirement list (a captured graph may still read them)."""
    def build():
        L = _lib.lib()
        V, E = emb_table.shape
        table = torch.empty(V, 8 * hidden, device=emb_table.device, dtype=torch.float32)
        assert table.numel() * 4 == L.mgnns_bilstm_bf16_table_bytes(V, hidden)
        ws = torch.empty(L.mgnns_bilstm_bf16_fold_workspace_bytes(V), dtype=torch.uint8, device=emb_table.device)
        _lib.call("mgnns_bilstm_bf16_fold_embedding", _p(emb_table), V, E, hidden, _p(cat0[0]), _p(cat0[1]), _p(ws), ws.numel(), _p(table),
                  _stream())
        return table
    return _lstm_derived(cache, "table", [emb_table, cat0[0], cat0[1]], build)


def bilstm(tok, lens, emb_table, weights, hidden, num_layers, want_bf16=False, recurrence="f32", cache=None, fold=None):
    """tok [B,T] int64, lens [B] int64 (device), weights = list over (layer, direction) of
    (w_ih, w_hh, b_ih, b_hh) -> [B,T,2*hidden] with zeros behind each sample's length
    (+ the same bank as zero-padded bf16 [B,T,320] when want_bf16).  recurrence="bf16": W_hh . h of every step on the
    bf16 MFMA (bf16 operands, fp32 accumulation and state) instead of the exact fp32 GEMV.
    cache: an LstmCache owned by the module that owns `weights` (None: derived weight forms are rebuilt per call).
    fold (bf16 recurrence; default LSTM_FOLD_EMBEDDING when a cache is given): read the layer-0 input projection out of the
    table folded from the embedding and W_ih once per weight version -- the same rows bit for bit, no GEMM in front of the first
    recurrence."""
    import ctypes
    _chk(tok, "text", torch.int64, 2)
    _chk(lens, "text_lens", torch.int64, 1)
    _chk(emb_table, "embedding.weight", ndim=2)
    B, T = tok.shape
    if lens.shape[0] != B:
        raise ValueError("text_lens has %d entries for batch %d" % (lens.shape[0], B))
    if len(weights) != 2 * num_layers:
        raise ValueError("need %d (layer, direction) weight tuples" % (2 * num_layers))
    for li, tup in enumerate(weights):
        in_dim = emb_table.shape[1] if li < 2 else 2 * hidden
        shapes = ((4 * hidden, in_dim), (4 * hidden, hidden), (4 * hidden,), (4 * hidden,))
        for t, shp in zip(tup, shapes):
            _chk(t, "lstm weight")
            if tuple(t.shape) != shp:
                raise ValueError("lstm weight shape %s, expected %s" % (tuple(t.shape), shp))
    cat = _lstm_cat(weights, num_layers, cache)
    arr = lambda ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    c_wih = arr([c[0].data_ptr() for c in cat])
    c_bih = arr([c[1].data_ptr() for c in cat])
    c_whh = arr([w[1].data_ptr() for w in weights])
    c_bhh = arr([w[3].data_ptr() for w in weights])
    L = _lib.lib()
    nbytes = L.mgnns_bilstm_workspace_bytes(B, T, hidden, num_layers)
    # per call, on the calling stream: a captured forward keeps it alive in the graph's own pool; nothing is shared
    # between models, streams or graphs
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=tok.device)
    out = torch.empty(B, T, 2 * hidden, device=tok.device, dtype=torch.float32)
    out_bf = torch.empty(B, T, BANK_LD, device=tok.device, dtype=torch.bfloat16) if want_bf16 else None
    if recurrence not in ("f32", "bf16"):
        raise ValueError("recurrence must be 'f32' or 'bf16', got %r" % (recurrence,))
    if recurrence == "f32":
        _launch("mgnns_bilstm_fwd", _p(tok), _p(lens), B, T, _p(emb_table), emb_table.shape[0], emb_table.shape[1], hidden, num_layers,
                c_wih, c_bih, c_whh, c_bhh, _p(ws), ws.numel(), _p(out), _p(out_bf), BANK_LD, _stream())
    else:
        # weight layouts of the bf16 kernels: packed once per weight version, off the per-forward path
        def prepack():
            pre = torch.empty(L.mgnns_bilstm_bf16_prepack_bytes(hidden, num_layers), dtype=torch.uint8, device=tok.device)
            _lib.call("mgnns_bilstm_bf16_prepack", c_wih, c_whh, emb_table.shape[1], hidden, num_layers, _p(pre), _stream())
            return pre
        pre = _lstm_derived(cache, "prepack", [t for tup in weights for t in (tup[0], tup[1])], prepack)
        if fold is None:
            fold = LSTM_FOLD_EMBEDDING and cache is not None
        if fold and B <= 1024 and T <= 1024 and emb_table.shape[1] % 4 == 0 and emb_table.shape[1] <= 320:
            table = _lstm_table(emb_table, cat[0], hidden, cache)
            _launch("mgnns_bilstm_bf16_table_fwd", _p(tok), _p(lens), B, T, _p(emb_table), emb_table.shape[0], emb_table.shape[1], hidden,
                    num_layers, c_wih, c_bih, c_whh, c_bhh, _p(ws), ws.numel(), _p(out), _p(out_bf), BANK_LD, _p(pre), _p(table), _stream())
        else:
            _launch("mgnns_bilstm_bf16_fwd", _p(tok), _p(lens), B, T, _p(emb_table), emb_table.shape[0], emb_table.shape[1], hidden,
                    num_layers, c_wih, c_bih, c_whh, c_bhh, _p(ws), ws.numel(), _p(out), _p(out_bf), BANK_LD, _p(pre), _stream())
    return (out, out_bf) if want_bf16 else out


# ---- text GCN --------------------------------------------------------------------------------
def textgcn(tok, node_hidden, edge_w, pmi_dev, ngram, max_length=100):
    """Text_GCN.Model.forward (Text_GCN.py:213-275): tok [B,T] int64 -> [B,D]."""
    _chk(tok, "doc_ids", torch.int64, 2)
    _chk(node_hidden, "node_hidden.weight", ndim=2)
    ew = _chk(edge_w.reshape(-1), "seq_edge_w.weight")
    rp, col, eid = pmi_dev
    _chk(rp, "pmi row_ptr", torch.int32, 1)
    _chk(col, "pmi col", torch.int32, 1)
    if eid is not None:                    # None: ids are positional (eid[k] == k + 1), the kernel derives them
        _chk(eid, "pmi eid", torch.int32, 1)
        if eid.shape != col.shape:
            raise ValueError("pmi eid and col must have the same length")
    B, T = tok.shape
    V, D = node_hidden.shape
    if rp.shape[0] != V + 1:
        raise ValueError("PMI map has %d rows, vocabulary has %d" % (rp.shape[0] - 1, V))
    out = torch.empty(B, D, device=tok.device, dtype=torch.float32)
    _launch("mgnns_textgcn_fwd", _p(tok), B, T, _p(node_hidden), V, D, _p(ew), ew.shape[0], _p(rp), _p(col), _p(eid), int(ngram),
            int(max_length), _p(out), _stream())
    return out


# ---- image bank + pool ---------------------------------------------------------------------------
IMGBANK_LDW = 304


def transpose_pad(w, ld):
    """[rows, cols] -> [cols, ld] transposed, zero padded."""
    _chk(w, "w", ndim=2)
    out = torch.empty(w.shape[1], ld, device=w.device, dtype=torch.float32)
    _lib.call("mgnns_transpose_pad", _p(w), w.shape[0], w.shape[1], _p(out), ld, _stream())
    return out


def imgbank_pool(feat, wt, bias, n_out, want_pool=True):
    """feat [B,K,P]; wt = transpose_pad(liner_img.weight, 304) [K,304] -> bank [B,P,N], pooled [B,K]."""
    _chk(feat, "feature map", ndim=3)
    _chk(wt, "wt", ndim=2)
    B, K, P = feat.shape
    if wt.shape[0] != K:
        raise ValueError("wt rows %d != K %d" % (wt.shape[0], K))
    if bias is not None:
        _chk(bias, "bias", ndim=1)
    bank = torch.empty(B, P, n_out, device=feat.device, dtype=torch.float32)
    pooled = torch.empty(B, K, device=feat.device, dtype=torch.float32) if want_pool else None
    _launch("mgnns_imgbank_pool_fwd", _p(feat), B, K, P, _p(wt), wt.shape[1], _p(bias), n_out, _p(bank), _p(pooled), _stream())
    return bank, pooled


def pack_imgbank_weights_bf16(w):
    """liner_img_*.weight [N, K] fp32 -> MFMA-fragment-major bf16 buffer for imgbank_pool_bf16."""
    _chk(w, "weight", ndim=2)
    L = _lib.lib()
    buf = torch.empty(L.mgnns_imgbank_packed_weight_bytes(w.shape[1]), dtype=torch.uint8, device=w.device)
    _lib.call("mgnns_imgbank_pack_weights_bf16", _p(w), w.shape[0], w.shape[1], _p(buf), _stream())
    return buf


def imgbank_pool_bf16(feat, wp, bias, n_out, combine=True):
    """feat [B,K,P] fp32 -> (bank bf16 [B,P,320], pooled fp32 [B,K]); combine=False: pooled stays as the kernel's two
    per-half maxima [B,2,K] (label_tail takes the max itself: one launch less on the channel's critical chain)."""
    _chk(feat, "feature map", ndim=3)
    _chk(wp, "packed weight", torch.uint8, 1)
    B, K, P = feat.shape
    if bias is not None:
        _chk(bias, "bias", ndim=1)
    bank = torch.empty(B, P, BANK_LD, device=feat.device, dtype=torch.bfloat16)
    pooled = torch.empty(B, K, device=feat.device, dtype=torch.float32)
    work = torch.empty(B, 2, K, device=feat.device, dtype=torch.float32)
    _launch("mgnns_imgbank_pool_bf16_fwd", _p(feat), B, K, P, _p(wp), _p(bias), n_out, _p(bank), BANK_LD, _p(pooled) if combine else None,
            _p(work), _stream())
    return bank, (pooled if combine else work)


def head_diff(o, n_head):
    """o [B, n_head*d_v] (per-head attention outputs) -> [B]: mean over head pairs i != j of cos^2(o_i, o_j)
    (diff_outputs, submodules.py:38-52)."""
    _chk(o, "attention output", ndim=2)
    B = o.shape[0]
    if o.shape[1] % n_head:
        raise ValueError("attention output width %d is not a multiple of n_head=%d" % (o.shape[1], n_head))
    out = torch.empty(B, device=o.device, dtype=torch.float32)
    _launch("mgnns_head_diff_fwd", _p(o), B, n_head, o.shape[1] // n_head, _p(out), _stream())
    return out


def textgcn_set_form(form):
    """0 by batch (default) | 1 one 1024-thread launch | 2 two launches (short + long documents) | 3 the lean kernel (tests)."""
    _lib.call("mgnns_textgcn_set_form", int(form))


def imgbank_set_form(form):
    """Which bf16 image-bank kernel runs: 0 = chosen by the batch (default), 1 = the stream form (one workgroup per sample),
    2 = the pair form (two workgroups per sample) where its shape limits allow.  Process-wide; tests and measurements."""
    _lib.call("mgnns_imgbank_set_form", int(form))


# ---- label attention core ---------------------------------------------------------------------------
def imgbank_pool_split(feat, w_pair, bias, n_out, want_pool=True, want_f32=True, want_split=False):
    """Split-bf16 (fp32-class) image bank + max-pool: feat [B,K,P] fp32, w_pair = pack_weight_bf16_split(liner_img.weight
    [n_out,K]) -> (bank [B,P,n_out] fp32 or None, pooled halves [B,2,K] fp32 or None[, split images bf16 [2,B,P,320] when
    want_split: hi = bf16(bank), lo = bf16(bank - hi), zero padded -- the split-bf16 attention core's operand])."""
    _chk(feat, "feature map", ndim=3)
    B, K, P = feat.shape
    hi, lo = w_pair
    _chk(hi, "packed hi", torch.uint8, 1)
    _chk(lo, "packed lo", torch.uint8, 1)
    if bias is not None:
        _chk(bias, "bias", ndim=1)
    if not (want_f32 or want_split):
        raise ValueError("imgbank_pool_split: nothing to compute (want_f32 or want_split)")
    bank = torch.empty(B, P, n_out, device=feat.device, dtype=torch.float32) if want_f32 else None
    split = torch.empty(2, B, P, BANK_LD, device=feat.device, dtype=torch.bfloat16) if want_split else None
    pooled = torch.empty(B, 2, K, device=feat.device, dtype=torch.float32) if want_pool else None
    _launch("mgnns_imgbank_pool_split_fwd", _p(feat), B, K, P, _p(hi), _p(lo), _p(bias), n_out, _p(bank), _p(pooled),
            _p(split[0]) if want_split else None, _p(split[1]) if want_split else None, _stream(), key=(P,))
    return (bank, pooled, split) if want_split else (bank, pooled)


def label_attn_core(Q, K, V, n_heads, mask=None):
    """x[b,l,:] of Attention.forward between its projections (MODEL:101-131).  mask: anything that broadcasts against the
    energy [B, NLQ, heads, dh] (MODEL:118-119: positions where mask == 0 get -1e10 in front of the softmax over dh)."""
    _chk(Q, "Q", ndim=2)
    _chk(K, "K", ndim=2)
    _chk(V, "V", ndim=2)
    NLQ, hid = Q.shape
    B = K.shape[0]
    if K.shape[1] != hid or V.shape != K.shape or hid % n_heads:
        raise ValueError("label attention shapes Q%s K%s V%s" % (tuple(Q.shape), tuple(K.shape), tuple(V.shape)))
    x = torch.empty(B, NLQ, hid, device=K.device, dtype=torch.float32)
    if mask is not None:
        if mask.device != K.device:
            raise ValueError("mask is on %s, K on %s" % (mask.device, K.device))
        # the byte image of the broadcast mask (layout only: the comparison with 0 and the fill run in the kernel)
        m8 = torch.broadcast_to(mask != 0, (B, NLQ, n_heads, hid // n_heads)).to(torch.uint8).contiguous()
        _lib.call("mgnns_label_attn_core_masked_fwd", _p(Q), _p(K), _p(V), _p(m8), B, NLQ, n_heads, hid // n_heads, _p(x), _stream())
        return x
    _lib.call("mgnns_label_attn_core_fwd", _p(Q), _p(K), _p(V), B, NLQ, n_heads, hid // n_heads, _p(x), _stream())
    return x


def label_tail(x, Q, n_heads, packed, pooled=None, g_wp=None, next_q=None):
    """Fused label-attention tail (mgnns_label_tail_fwd).  Either x [B,C] (the read-out) or pooled [B,parts,K] +
    g_wp = pack_weight_f32(G [C,K]) (read-out computed in the kernel); Q [NLQ,hid] = w_q(label query); packed =
    dict(wk, bk, wv, bv, wc, bc, n5, xl, bxl, n_out, C) with wk/wv/wc/xl = pack_weight_f32 images; next_q = (wq_wp, bq,
    HK) adds qh = w_qs(out) + b.  -> out [B, n_out]  (or (out, qh) with next_q)."""
    _chk(Q, "Q", ndim=2)
    NLQ, hid = Q.shape
    if hid % n_heads:
        raise ValueError("hidden width %d is not a multiple of %d heads" % (hid, n_heads))
    if (x is None) == (g_wp is None):
        raise ValueError("pass either x or (pooled, g_wp)")
    parts = kp = 0
    if x is not None:
        _chk(x, "x", ndim=2)
        B, C = x.shape
    else:
        _chk(pooled, "pooled", ndim=3)
        _chk(g_wp, "packed G", ndim=1)
        B, parts, kp = pooled.shape
        C = packed["C"]
    if C != packed["C"]:
        raise ValueError("read-out width %d does not match the packed w_k / w_v (%d)" % (C, packed["C"]))
    for k in ("wk", "wv", "wc", "xl", "bk", "bv", "bc", "bxl"):
        _chk(packed[k], k, ndim=1)
    out = torch.empty(B, packed["n_out"], device=Q.device, dtype=torch.float32)
    wq = bq = qh = None
    hkn = 0
    if next_q is not None:
        wq, bq, hkn = next_q
        qh = torch.empty(B, hkn, device=Q.device, dtype=torch.float32)
    _launch("mgnns_label_tail_fwd", _p(x), B, C, _p(pooled), parts, kp, _p(g_wp), _p(Q), NLQ, n_heads, hid // n_heads, _p(packed["wk"]),
            _p(packed["bk"]), _p(packed["wv"]), _p(packed["bv"]), _p(packed["wc"]), _p(packed["bc"]), packed["n5"], _p(packed["xl"]),
            _p(packed["bxl"]), packed["n_out"], _p(out), _p(wq), _p(bq), hkn, _p(qh), _stream(), key=(C,))
    return out if next_q is None else (out, qh)


LABEL_TAIL_CLUSTER = True


def label_tail_bf16(pooled, g_pair, Q, n_heads, packed, next_q=None, terms=3, cluster=None):
    """bf16-mode fused channel tail (mgnns_label_tail_bf16_fwd): pooled [B,parts,K] fp32, g_pair = pack_weight_bf16_split(G
    [C,K]); packed = dict(wk, wv, wc, xl = (hi, lo) pairs of pack_weight_bf16_split, bk, bv, bc, bxl, n5, n_out, C);
    next_q = ((hi, lo), bq, HK).  terms = 1 plain bf16 | 3 split-bf16.  cluster: four workgroups per 16-sample tile split the
    read-out, the last to arrive finishes the tile, the next query is a second launch inside the same C call
    (terms = 3; default on, ops.LABEL_TAIL_CLUSTER = False turns it off); the exchange scratch lives in `packed`, one per
    channel, so the two channels' launches never share one.  -> out [B,n_out] (or (out, qh))."""
    import ctypes
    _chk(pooled, "pooled", ndim=3)
    _chk(Q, "Q", ndim=2)
    B, parts, kp = pooled.shape
    NLQ, hid = Q.shape
    if hid % n_heads:
        raise ValueError("hidden width %d is not a multiple of %d heads" % (hid, n_heads))
    pairs = [g_pair, packed["wk"], packed["wv"], packed["wc"], packed["xl"]]
    for k in ("bk", "bv", "bc", "bxl"):
        _chk(packed[k], k, ndim=1)
    out = torch.empty(B, packed["n_out"], device=Q.device, dtype=torch.float32)
    bq = qh = None
    hkn = 0
    if next_q is not None:
        wqp, bq, hkn = next_q
        pairs.append(wqp)
        qh = torch.empty(B, hkn, device=Q.device, dtype=torch.float32)
    ptrs = []
    for h, l in pairs:
        _chk(h, "packed hi", torch.uint8, 1)
        _chk(l, "packed lo", torch.uint8, 1)
        ptrs += [h.data_ptr(), l.data_ptr()]
    ptrs += [None] * (12 - len(ptrs))
    arr = (ctypes.c_void_p * 12)(*ptrs)
    if cluster is None:
        cluster = LABEL_TAIL_CLUSTER
    scratch = counters = None
    if cluster and int(terms) == 3 and B > 0:
        ws = _cluster_scratch(packed, "_cluster_ws", Q.device, (B + 15) // 16, lambda tiles: tiles * 4 * 6144)
        scratch, counters = ws[1], ws[2]
    _launch("mgnns_label_tail_bf16_fwd", _p(pooled), B, parts, kp, packed["C"], int(terms), arr, _p(Q), NLQ, n_heads, hid // n_heads,
            _p(packed["bk"]), _p(packed["bv"]), _p(packed["bc"]), packed["n5"], _p(packed["bxl"]), packed["n_out"], _p(out), _p(bq), hkn,
            _p(qh), _p(scratch), _p(counters), _stream(), key=(packed["C"],))
    return out if next_q is None else (out, qh)


# ---- single-query MHA core -------------------------------------------------------------------------------
def sq_mha_core(qh, bank, mask, n_head, d_kv, wk, bk, wv, bv, want_attn=True):
    _chk(qh, "qh", ndim=2)
    _chk(bank, "memory bank", ndim=3)
    B, L_, D = bank.shape
    if qh.shape != (B, n_head * d_kv):
        raise ValueError("qh shape %s, expected %s" % (tuple(qh.shape), (B, n_head * d_kv)))
    if mask is not None:
        _chk(mask, "mask", ndim=2)
        if mask.shape != (B, L_):
            raise ValueError("mask shape %s, expected %s" % (tuple(mask.shape), (B, L_)))
    for n, t in (("w_ks.weight", wk), ("w_vs.weight", wv)):
        _chk(t, n, ndim=2)
        if t.shape != (n_head * d_kv, D):
            raise ValueError("%s shape %s" % (n, tuple(t.shape)))
    o = torch.empty(B, n_head * d_kv, device=bank.device, dtype=torch.float32)
    attn = torch.empty(n_head * B, 1, L_, device=bank.device, dtype=torch.float32) if want_attn else None
    _launch("mgnns_sq_mha_core_fwd", _p(qh), _p(bank), _p(mask), B, L_, D, n_head, d_kv, _p(wk), _p(bk), _p(wv), _p(bv), _p(o), _p(attn),
            _stream(), key=(L_, mask is not None))
    return o, attn


# The bf16 attention core has two builds: 32 = v_mfma_f32_32x32x16_bf16 (csrc/sq_mha32_bf16.hip; packed masked banks), 16 = the
# 16x16x32 form of rounds 1-3 (csrc/sq_mha_bf16.hip).  The packed weights differ: a pack carries its form as an attribute and
# sq_mha_core_bf16 dispatches on it.
MHA_CORE = 32               # the build that takes a packing plan
MHA_CORE_PLAIN = 16         # one workgroup per sample (no plan): the faster build
MHA_PACKED = True           # masked banks: the live rows of short samples packed into shared workgroups (a plan)


def pack_kv_weights_bf16(wk, wv, n_head, d_kv, form=None):
    """w_ks / w_vs [H*dk, D] fp32 -> MFMA-fragment-major bf16 buffer for sq_mha_core_bf16."""
    _chk(wk, "w_ks.weight", ndim=2)
    _chk(wv, "w_vs.weight", ndim=2)
    form = MHA_CORE if form is None else int(form)
    L = _lib.lib()
    if form == 32:
        buf = torch.empty(L.mgnns_sq_mha32_packed_weight_bytes(n_head), dtype=torch.uint8, device=wk.device)
        _lib.call("mgnns_sq_mha32_pack_weights_bf16", _p(wk), _p(wv), n_head, d_kv, wk.shape[1], _p(buf), _stream())
    else:
        buf = torch.empty(L.mgnns_sq_mha_packed_weight_bytes(n_head), dtype=torch.uint8, device=wk.device)
        _lib.call("mgnns_sq_mha_pack_weights_bf16", _p(wk), _p(wv), n_head, d_kv, wk.shape[1], _p(buf), _stream())
    buf._mg_form = form
    return buf


def sq_mha_plan(mask):
    """Packing plan of a [B, L] mask (L <= 128) for sq_mha_core_bf16(plan=...): which samples share a workgroup.  One launch;
    build it once per batch, every attention launch on that mask takes it.  The buffer holds 4 header ints, B group records of 4
    ints and B sample records of 2; of the group records only the first plan[0] are written (csrc/sq_mha_plan.hpp), the rest
    is unwritten memory that no kernel reads."""
    _chk(mask, "mask", ndim=2)
    B, L_ = mask.shape
    if B > PLAN_MAX_B:
        raise ValueError("sq_mha_plan: batch %d beyond the plan kernel's limit %d (fusion.make_mask_plan falls back to the "
                         "one-workgroup-per-sample core)" % (B, PLAN_MAX_B))
    L = _lib.lib()
    plan = torch.empty(L.mgnns_sq_mha32_plan_ints(B), dtype=torch.int32, device=mask.device)
    _lib.call("mgnns_sq_mha32_plan", _p(mask), B, L_, _p(plan), _stream())
    plan._mg_plan_kind = 'packed'
    return plan


PLAN_MAX_L = 128
PLAN_MAX_B = 4096          # mgnns_sq_mha32_plan: one workgroup scans the batch ((8 B + 4) * 4 bytes of LDS)


def cast_pad_bf16(x, ld=BANK_LD):
    """[..., D] fp32 -> [..., ld] bf16 (round to nearest even), zero padded."""
    D = x.shape[-1]
    x2 = _chk(x.reshape(-1, D), "x")
    y = torch.empty(x2.shape[0], ld, dtype=torch.bfloat16, device=x.device)
    _lib.call("mgnns_cast_pad_bf16", _p(x2), x2.shape[0], D, ld, _p(y), _stream())
    return y.view(*x.shape[:-1], ld)


def sq_mha_core_bf16(qh, bank_bf16, mask, n_head, d_kv, wp, bk, bv, want_attn=True, plan=None):
    """plan: sq_mha_plan(mask) (32x32x16 form, L <= 128) -- the live rows of short samples packed into shared workgroups."""
    _chk(qh, "qh", ndim=2)
    _chk(bank_bf16, "memory bank (bf16)", torch.bfloat16, 3)
    _chk(wp, "packed K/V weights", torch.uint8, 1)
    B, L_, ld = bank_bf16.shape
    if qh.shape != (B, n_head * d_kv):
        raise ValueError("qh shape %s, expected %s" % (tuple(qh.shape), (B, n_head * d_kv)))
    if mask is not None:
        _chk(mask, "mask", ndim=2)
        if mask.shape != (B, L_):
            raise ValueError("mask shape %s, expected %s" % (tuple(mask.shape), (B, L_)))
    o = torch.empty(B, n_head * d_kv, device=qh.device, dtype=torch.float32)
    attn = torch.empty(n_head * B, 1, L_, device=qh.device, dtype=torch.float32) if want_attn else None
    L = _lib.lib()
    form = getattr(wp, "_mg_form", 16)
    if form == 32:
        if plan is not None:
            _chk(plan, "plan", torch.int32, 1)
            # (4 + 6 B ints: the size names the batch the plan was built for -- a plan of another batch is refused here)
            if mask is None or L_ > PLAN_MAX_L or plan.numel() != L.mgnns_sq_mha32_plan_ints(B):
                raise ValueError("a packing plan needs a mask, L <= %d and exactly %d ints (a plan built for this batch size)"
                                 % (PLAN_MAX_L, L.mgnns_sq_mha32_plan_ints(B)))
            if getattr(plan, "_mg_plan_kind", 'packed') != 'packed':       # (the grouped split-bf16 core's plan has the same size)
                raise ValueError("sq_mha_core_bf16 takes the plan sq_mha_plan(mask) returned (got kind %r)"
                                 % plan._mg_plan_kind)
        _launch("mgnns_sq_mha32_core_bf16_fwd", _p(qh), _p(bank_bf16), _p(mask), B, L_, ld, n_head, d_kv, _p(wp), _p(bk), _p(bv), _p(o),
                _p(attn), _p(plan), _stream(), key=(L_, mask is not None), alias="mgnns_sq_mha_core_bf16_fwd")
        return o, attn
    if plan is not None:
        raise ValueError("a packing plan needs the 32x32x16 form of the packed weights")
    _launch("mgnns_sq_mha_core_bf16_fwd", _p(qh), _p(bank_bf16), _p(mask), B, L_, ld, n_head, d_kv, _p(wp), _p(bk), _p(bv), _p(o), _p(attn),
            _stream(), key=(L_, mask is not None))
    return o, attn


def pack_kv_weights_split(wk, wv, n_head, d_kv):
    """w_ks / w_vs [H*dk, D] fp32 -> the split-bf16 (hi image, lo image) fragment-major buffer of sq_mha_core_split."""
    _chk(wk, "w_ks.weight", ndim=2)
    _chk(wv, "w_vs.weight", ndim=2)
    L = _lib.lib()
    buf = torch.empty(L.mgnns_sq_mha_split_packed_weight_bytes(n_head), dtype=torch.uint8, device=wk.device)
    _lib.call("mgnns_sq_mha_pack_weights_split", _p(wk), _p(wv), n_head, d_kv, wk.shape[1], _p(buf), _stream())
    buf._mg_form = "split"
    return buf


def split_pad_bf16(x, ld=BANK_LD):
    """[..., D] fp32 -> bf16 [2, ..., ld]: [0] = hi = bf16(x), [1] = lo = bf16(x - hi), zero padded (x = hi + lo to ~2^-17)."""
    D = x.shape[-1]
    x2 = _chk(x.reshape(-1, D), "x")
    y = torch.empty(2, x2.shape[0], ld, dtype=torch.bfloat16, device=x.device)
    _lib.call("mgnns_split_pad_bf16", _p(x2), x2.shape[0], D, ld, _p(y[0]), _p(y[1]), _stream())
    return y.view(2, *x.shape[:-1], ld)


SPLIT_PLAN_MAX_L = 112


def sq_mha_split_plan(mask):
    """Group plan of a [B, L] mask (L <= 112) for sq_mha_core_split(plan=...): which samples share a workgroup (whole 16-row tiles,
    at most 7 tiles and 7 samples per group).  One launch; once per batch.  Layout and unwritten part as sq_mha_plan's."""
    _chk(mask, "mask", ndim=2)
    B, L_ = mask.shape
    if B > PLAN_MAX_B or L_ > SPLIT_PLAN_MAX_L:
        raise ValueError("sq_mha_split_plan: B=%d (<= %d), L=%d (<= %d)" % (B, PLAN_MAX_B, L_, SPLIT_PLAN_MAX_L))
    L = _lib.lib()
    plan = torch.empty(L.mgnns_sq_mha32_plan_ints(B), dtype=torch.int32, device=mask.device)
    _lib.call("mgnns_sq_mha_split_plan", _p(mask), B, L_, _p(plan), _stream())
    plan._mg_plan_kind = 'grouped'
    return plan


def sq_mha_core_split(qh, bank_split, mask, n_head, d_kv, wp, bk, bv, want_attn=True, plan=None):
    """The faithful attention core on split-bf16 operands (csrc/sq_mha_split_bf16.hip): bank_split = split_pad_bf16(bank)
    [2, B, L, 320], wp = pack_kv_weights_split(...).  plan: sq_mha_split_plan(mask) (masked banks, L <= 112, no attn output): the
    samples of a group share a workgroup.  -> (o [B, H*dk], attn [H*B, 1, L] or None)"""
    _chk(qh, "qh", ndim=2)
    _chk(bank_split, "memory bank (split bf16)", torch.bfloat16, 4)
    _chk(wp, "packed K/V weights", torch.uint8, 1)
    if getattr(wp, "_mg_form", None) != "split":
        raise ValueError("sq_mha_core_split takes pack_kv_weights_split(...) weights")
    two, B, L_, ld = bank_split.shape
    if two != 2:
        raise ValueError("bank_split must be [2, B, L, %d] (hi, lo)" % BANK_LD)
    if qh.shape != (B, n_head * d_kv):
        raise ValueError("qh shape %s, expected %s" % (tuple(qh.shape), (B, n_head * d_kv)))
    if mask is not None:
        _chk(mask, "mask", ndim=2)
        if mask.shape != (B, L_):
            raise ValueError("mask shape %s, expected %s" % (tuple(mask.shape), (B, L_)))
    o = torch.empty(B, n_head * d_kv, device=qh.device, dtype=torch.float32)
    attn = torch.empty(n_head * B, 1, L_, device=qh.device, dtype=torch.float32) if want_attn else None
    L = _lib.lib()
    if plan is not None:
        _chk(plan, "plan", torch.int32, 1)
        if mask is None or L_ > SPLIT_PLAN_MAX_L or want_attn or plan.numel() != L.mgnns_sq_mha32_plan_ints(B):
            raise ValueError("a group plan needs a mask, L <= %d, want_attn=False and exactly %d ints (a plan built for this batch)"
                             % (SPLIT_PLAN_MAX_L, L.mgnns_sq_mha32_plan_ints(B)))
        # the packed bf16 kernel's plan has the SAME size (up to 16 samples / 128 rows per group: past this kernel's LDS maps); only
        # the tensor sq_mha_split_plan returned is taken (a view / clone loses the tag -- the kernel checks the plan's own header word
        # too and raises the library's status word instead of running)
        if getattr(plan, "_mg_plan_kind", None) != 'grouped':
            raise ValueError("sq_mha_core_split takes the plan sq_mha_split_plan(mask) returned (got kind %r)"
                             % getattr(plan, "_mg_plan_kind", None))
    _launch("mgnns_sq_mha_core_split_fwd", _p(qh), _p(bank_split[0]), _p(bank_split[1]), _p(mask), B, L_, ld, n_head, d_kv, _p(wp), _p(bk),
            _p(bv), _p(o), _p(attn), _p(plan), _stream(), key=(L_, mask is not None))
    return o, attn


def sq_mha_folded(qh, bank, mask, n_head, d_kv, wk, wv, bv, want_attn=True):
    """Folded single-query attention (mgnns_sq_mha_folded_fwd): same result as sq_mha_core, K and V never formed.
    bank: fp32 [B, L, D] or bf16 [B, L, ld] (zero padded).  b_k is not needed (it drops out of the softmax)."""
    _chk(qh, "qh", ndim=2)
    is_bf16 = bank.dtype == torch.bfloat16
    _chk(bank, "memory bank", torch.bfloat16 if is_bf16 else torch.float32, 3)
    B, L_, ld = bank.shape
    for n, t in (("w_ks.weight", wk), ("w_vs.weight", wv)):
        _chk(t, n, ndim=2)
    D = wk.shape[1]
    if qh.shape != (B, n_head * d_kv):
        raise ValueError("qh shape %s, expected %s" % (tuple(qh.shape), (B, n_head * d_kv)))
    if wk.shape != (n_head * d_kv, D) or wv.shape != (n_head * d_kv, D):
        raise ValueError("w_ks %s / w_vs %s, expected %s" % (tuple(wk.shape), tuple(wv.shape), (n_head * d_kv, D)))
    if (ld != D) if not is_bf16 else (ld < D):
        raise ValueError("memory bank last dim %d does not match d_model %d" % (ld, D))
    if mask is not None:
        _chk(mask, "mask", ndim=2)
        if mask.shape != (B, L_):
            raise ValueError("mask shape %s, expected %s" % (tuple(mask.shape), (B, L_)))
    o = torch.empty(B, n_head * d_kv, device=qh.device, dtype=torch.float32)
    attn = torch.empty(n_head * B, 1, L_, device=qh.device, dtype=torch.float32) if want_attn else None
    L = _lib.lib()
    nbytes = L.mgnns_sq_mha_folded_workspace_bytes(B, D, n_head)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=qh.device)     # per call: stacks run on four streams
    _launch("mgnns_sq_mha_folded_fwd", _p(qh), _p(bank), int(is_bf16), ld, _p(mask), B, L_, D, n_head, d_kv, _p(wk), _p(wv), _p(bv), _p(ws),
            nbytes, _p(o), _p(attn), _stream(), key=(L_, is_bf16))
    return o, attn


def sq_mha_folded_bf16(u, bank_bf16, mask, n_head, d_kv, want_attn=True):
    """Folded single-query attention on the bf16 matrix pipe (mgnns_sq_mha_folded_bf16_fwd).  u: fp32 [B, H*D] composed query
    rows (fusion.composed_query_map); bank: bf16 [B, L, 320] zero padded -> (c bf16 [B, H*D rounded up to 32] = per-head
    probability-weighted bank rows at h*D, zeros behind H*D: what mha_tail_c16 takes; attn [H*B, 1, L] or None)."""
    _chk(u, "u", ndim=2)
    _chk(bank_bf16, "memory bank", torch.bfloat16, 3)
    B, L_, ld = bank_bf16.shape
    if ld != 320:
        raise ValueError("bf16 memory bank last dim %d, expected 320 (cast_pad_bf16)" % ld)
    if u.shape[0] != B or u.shape[1] % n_head:
        raise ValueError("u shape %s does not match batch %d / %d heads" % (tuple(u.shape), B, n_head))
    D = u.shape[1] // n_head
    if mask is not None:
        _chk(mask, "mask", ndim=2)
        if mask.shape != (B, L_):
            raise ValueError("mask shape %s, expected %s" % (tuple(mask.shape), (B, L_)))
    ldc = (n_head * D + 31) // 32 * 32
    c = torch.empty(B, ldc, device=u.device, dtype=torch.bfloat16)
    attn = torch.empty(n_head * B, 1, L_, device=u.device, dtype=torch.float32) if want_attn else None
    _launch("mgnns_sq_mha_folded_bf16_fwd", _p(u), _p(bank_bf16), _p(mask), B, L_, D, n_head, float(1.0 / (d_kv ** 0.5)), _p(c), ldc,
            _p(attn), _stream(), key=(L_,))
    return c, attn


def pack_weight_f32(w):
    """[N, K] fp32 (nn.Linear layout) -> MFMA-fragment-major fp32 buffer for mha_tail."""
    _chk(w, "weight", ndim=2)
    L = _lib.lib()
    buf = torch.empty(L.mgnns_packed_f32_weight_bytes(w.shape[0], w.shape[1]) // 4, dtype=torch.float32, device=w.device)
    _lib.call("mgnns_pack_weight_f32", _p(w), w.shape[0], w.shape[1], _p(buf), _stream())
    return buf


def mha_tail(o, q, packed, eps, next_packed=None):
    """Fused fc + residual + LN + FFN + residual + LN (+ next layer's w_qs).  `packed` = dict with fc_wp, fc_b,
    g1, be1, w1_wp, b1, w2_wp, b2, g2, be2; next_packed = (wq_wp, bq, HK_next) or None.
    Returns (out [B,300], qh_next [B,HK_next] or None)."""
    _chk(o, "o", ndim=2)
    _chk(q, "q", ndim=2)
    B, HK = o.shape
    if q.shape != (B, 300):
        raise ValueError("q shape %s, expected (%d, 300)" % (tuple(q.shape), B))
    out = torch.empty(B, 300, device=o.device, dtype=torch.float32)
    wq = bq = qh = None
    hkn = 0
    if next_packed is not None:
        wq, bq, hkn = next_packed
        qh = torch.empty(B, hkn, device=o.device, dtype=torch.float32)
    _launch("mgnns_mha_tail_fwd", _p(o), HK, _p(q), B, 300, _p(packed["fc_wp"]), _p(packed["fc_b"]), _p(packed["g1"]), _p(packed["be1"]),
            _p(packed["w1_wp"]), _p(packed["b1"]), _p(packed["w2_wp"]), _p(packed["b2"]), _p(packed["g2"]), _p(packed["be2"]), float(eps),
            _p(out), _p(wq), _p(bq), hkn, _p(qh), _stream())
    return out, qh


def pack_weight_bf16_split(w):
    """[N, K] fp32 -> (hi, lo) MFMA-fragment-major bf16 buffers (w ~ hi + lo) for mha_tail_bf16."""
    _chk(w, "weight", ndim=2)
    L = _lib.lib()
    n = L.mgnns_packed_bf16_weight_bytes(w.shape[0], w.shape[1])
    hi = torch.empty(n, dtype=torch.uint8, device=w.device)
    lo = torch.empty(n, dtype=torch.uint8, device=w.device)
    _lib.call("mgnns_pack_weight_bf16_split", _p(w), w.shape[0], w.shape[1], _p(hi), _p(lo), _stream())
    return hi, lo


def mha_tail_bf16(o, q, packed, eps, next_packed=None, terms=3, cluster=0, ksplit=True, next_linear=None):
    """bf16-MFMA fused tail.  packed: dict with fc, w1, w2 = (hi, lo) buffers and fc_b, g1, be1, b1, b2, g2, be2;
    next_packed = ((hi, lo), bq, HK_next) or None.  ksplit (default on): a tile's cluster of workgroups splits the K
    of fc and exchanges partial sums through scratch owned by `packed` (one per capture epoch and launch stream), the next
    layer's w_qs runs as a second launch (terms == 1: mha_proj_c16; terms == 3: the exact-fp32 GEMM on next_linear = (weight
    [HK_next, 300], bias), which the K-split form needs in place of next_packed); cluster: workgroups per 16-sample tile
    (0 = the library's default)."""
    import ctypes
    _chk(o, "o", ndim=2)
    _chk(q, "q", ndim=2)
    B, HK = o.shape
    if q.shape != (B, 300):
        raise ValueError("q shape %s, expected (%d, 300)" % (tuple(q.shape), B))
    out = torch.empty(B, 300, device=o.device, dtype=torch.float32)
    ptrs = [packed["fc"][0].data_ptr(), packed["fc"][1].data_ptr(), packed["w1"][0].data_ptr(),
            packed["w1"][1].data_ptr(), packed["w2"][0].data_ptr(), packed["w2"][1].data_ptr(), None, None]
    bq = qh = None
    hkn = 0
    use_ks = ksplit and B > 0 and cluster != 1
    if int(terms) == 3 and use_ks and next_packed is not None and next_linear is None:
        use_ks = False                    # (the split-bf16 K split has no packed projection: without next_linear, the one-launch form)
    split_proj = int(terms) == 3 and use_ks and next_linear is not None
    if next_packed is not None and not split_proj:
        (wh, wl), bq, hkn = next_packed
        ptrs[6], ptrs[7] = wh.data_ptr(), wl.data_ptr()
        qh = torch.empty(B, hkn, device=o.device, dtype=torch.float32)
    arr = (ctypes.c_void_p * 8)(*ptrs)
    L = _lib.lib()
    scratch = counters = None
    if use_ks and int(terms) in (1, 3):
        ws = _cluster_scratch(packed, "_cluster_ws_ks", o.device, (B + 15) // 16,
                              lambda tiles: L.mgnns_mha_tail_c16_scratch_floats(16 * tiles, 8))
        scratch, counters = ws[1], ws[2]
    _launch("mgnns_mha_tail_bf16_fwd", _p(o), HK, _p(q), B, 300, int(terms), arr, _p(packed["fc_b"]), _p(packed["g1"]), _p(packed["be1"]),
            _p(packed["b1"]), _p(packed["b2"]), _p(packed["g2"]), _p(packed["be2"]), float(eps), _p(out), _p(bq), hkn, _p(qh), int(cluster),
            _p(scratch), _p(counters), _stream())
    if split_proj:
        qh = linear(out, next_linear[0], next_linear[1])
    return out, qh


def mha_tail_c16(c, q, packed, eps, next_packed=None, cluster=0, ksplit=True):
    """The bf16 fused tail behind sq_mha_folded_bf16 (mgnns_mha_tail_c16_fwd): c bf16 [B, H*300 rounded up to 32];
    packed["fc"] = the composed map fc . blockdiag(W_v); next_packed = ((hi, lo), bias, H*300) of the next layer's composed query
    map or None.  cluster: workgroups per 16-sample tile (0 = the library's default); ksplit (default on): the ranks split the K of
    the first product and exchange partial sums through scratch owned by `packed`, one per (capture epoch, launch stream)."""
    import ctypes
    _chk(c, "c", torch.bfloat16, 2)
    _chk(q, "q", ndim=2)
    B, HC = c.shape
    if q.shape != (B, 300):
        raise ValueError("q shape %s, expected (%d, 300)" % (tuple(q.shape), B))
    out = torch.empty(B, 300, device=c.device, dtype=torch.float32)
    ptrs = [packed["fc"][0].data_ptr(), None, packed["w1"][0].data_ptr(), None, packed["w2"][0].data_ptr(), None, None, None]
    bq = un = None
    hcn = 0
    if next_packed is not None:
        (wh, _wl), bq, hcn = next_packed
        ptrs[6] = wh.data_ptr()
        un = torch.empty(B, hcn, device=c.device, dtype=torch.float32)
    arr = (ctypes.c_void_p * 8)(*ptrs)
    L = _lib.lib()
    scratch = counters = None
    if ksplit and B > 0 and cluster != 1:
        ws = _cluster_scratch(packed, "_cluster_ws", c.device, (B + 15) // 16,
                              lambda tiles: L.mgnns_mha_tail_c16_scratch_floats(16 * tiles, 8))
        scratch, counters = ws[1], ws[2]
    _launch("mgnns_mha_tail_c16_fwd", _p(c), HC, _p(q), B, 300, arr, _p(packed["fc_b"]), _p(packed["g1"]), _p(packed["be1"]),
            _p(packed["b1"]), _p(packed["b2"]), _p(packed["g2"]), _p(packed["be2"]), float(eps), _p(out), _p(bq), hcn, _p(un), int(cluster),
            _p(scratch), _p(counters), _stream())
    return out, un


def layernorm(x, gamma, beta, eps=1e-6):
    D = x.shape[-1]
    x2 = _chk(x.reshape(-1, D), "x")
    _chk(gamma, "gamma", ndim=1)
    _chk(beta, "beta", ndim=1)
    y = torch.empty_like(x2)
    _lib.call("mgnns_layernorm_fwd", _p(x2), x2.shape[0], D, _p(gamma), _p(beta), float(eps), _p(y), _stream())
    return y.view(x.shape)


# ---- dense bf16 GEMM (large graphs / large X.W) -------------------------------------------------------------------------
def _kpad(k):
    return (k + 63) // 64 * 64


def transpose_cast_bf16(x):
    """[K, N] fp32 -> bf16 [N, Kp] (K-contiguous, zero padded to a multiple of 64): the Bt operand of gemm_bf16_nt."""
    _chk(x, "x", ndim=2)
    K, N = x.shape
    y = torch.empty(N, _kpad(K), dtype=torch.bfloat16, device=x.device)
    _lib.call("mgnns_transpose_cast_bf16", _p(x), K, N, y.shape[1], _p(y), _stream())
    return y


GEMM_BF16_KSPLIT = True       # K splits with partial sums in a workspace
_gemm_bf16_ws = {}


def _gemm_bf16_workspace(device):
    """Partial-sum slots + arrival counters of the dense bf16 GEMM's last-round K split: one buffer per (device, capture epoch,
    stream) -- launches on one stream are ordered, a captured graph may replay next to anything.  The K split is a two-launch scheme
    (partial sums, then a fix-up launch that reads exactly the slots the first wrote): no counters, nothing to zero, so the buffer
    is plain torch.empty (64 MB from the zero pool would be a fresh torch.zeros + stream synchronise per request)."""
    key = (str(device),) + _scratch_key()
    ws = _gemm_bf16_ws.get(key)
    if ws is None:
        ws = torch.empty(_lib.lib().mgnns_gemm_bf16_workspace_bytes(), dtype=torch.uint8, device=device)
        _gemm_bf16_ws[key] = ws
        if key[1]:
            _EPOCH_SLOTS.setdefault(key[1], []).append((_gemm_bf16_ws, key))
    return ws


def gemm_bf16_nt(a_bf16, bt_bf16, bias=None, act=ACT_NONE, n_valid=None, out=None, out_dtype=torch.float32, transposed_out=False):
    """act(A . Bt^T + bias): A bf16 [M, Kp], Bt bf16 [N, Kp] (Kp % 64 == 0) -> fp32 or bf16 [M, N].
    out: optional preallocated result; it may be a column slice [M, N] of a wider row-major matrix (row stride = its stride(0)),
    e.g. the K-padded operand of the next product.
    transposed_out (round 6): the result is stored as its transpose [N, M] (`out`, if given, is that [N, M] matrix or a column slice of a
    wider one); bias stays per column n of the product.  For products whose natural orientation has a small M: run the transpose
    (M = the long side) and keep the layout the consumer needs.  Needs ceil(M / 160) >= 8, N >= 256, K >= 320."""
    _chk(a_bf16, "A", torch.bfloat16, 2)
    _chk(bt_bf16, "Bt", torch.bfloat16, 2)
    M, Kp = a_bf16.shape
    N = bt_bf16.shape[0]
    if bt_bf16.shape[1] != Kp or Kp % 64:
        raise ValueError("A %s / Bt %s: K rows must match and be a multiple of 64" % (tuple(a_bf16.shape), tuple(bt_bf16.shape)))
    if bias is not None:
        _chk(bias, "bias", ndim=1)
    shape = (N, M) if transposed_out else (M, N)
    if out is None:
        c = torch.empty(*shape, device=a_bf16.device, dtype=out_dtype)
    else:
        c = out
        if not (torch.is_tensor(c) and c.is_cuda and c.dim() == 2 and tuple(c.shape) == shape and c.stride(1) == 1
                and c.dtype in (torch.float32, torch.bfloat16)):
            raise ValueError("out must be a [%d, %d] fp32 / bf16 device matrix with unit column stride" % shape)
    if transposed_out and ((M + 159) // 160 < 8 or N < 256 or Kp < 320):
        raise ValueError("transposed_out needs ceil(M / 160) >= 8, N >= 256, K >= 320 (M=%d N=%d K=%d)" % (M, N, Kp))
    ws = _gemm_bf16_workspace(a_bf16.device) if (GEMM_BF16_KSPLIT and M * N >= (1 << 20)) else None
    _lib.call("mgnns_gemm_bf16_nt_fwd", _p(a_bf16), _p(bt_bf16), M, N, Kp, _p(bias), _p(c), c.stride(0),
              (1 if c.dtype == torch.bfloat16 else 0) | (2 if transposed_out else 0), act, _p(ws), 0 if ws is None else ws.numel(),
              _stream())
    return c


def gemm_bf16_set_form(form):
    """Tile shape of gemm_bf16_nt (tests / timings): 0 round 4's kernels only, 1 the 160 x 256 kernel whenever the shape
    fits it, 2 by the launcher's estimate (the default), 3 the 320 x 256 kernel whenever it fits; -1 back to the default."""
    _lib.call("mgnns_gemm_bf16_set_form", int(form))


def dense_adj_matmul_bf16(adj_bf16, support, act=ACT_NONE):
    """act(adj @ support) with the DENSE adjacency kept in bf16 ([C, Kp], from cast_pad_bf16(adj, ld=Kp)) and the fp32
    support [C, F] transposed + cast on the fly: the dense counterpart of spmm_csr for graphs that are not sparse."""
    return gemm_bf16_nt(adj_bf16, transpose_cast_bf16(support), None, act)


# ---- f4: ResNet trunks (NHWC bf16 activations) ------------------------------------------------------------------
STEM_LD = 160      # stem weight rows: K = 3*7*7 = 147 zero padded to 5 MFMA k-steps


def conv_fold_bn(weight, conv_bias=None, bn=None, stem=False):
    """Fold an eval-mode BatchNorm (tuple gamma, beta, running_mean, running_var, eps -- or None) into a convolution
    weight [Cout, Cin, KH, KW] fp32 -> (bf16 [Cout, ld] with k = (kh, kw, c), or (c, kh, kw) padded to 160 for the stem;
    fp32 bias [Cout])."""
    _chk(weight, "weight", ndim=4)
    Cout, Cin, KH, KW = weight.shape
    ld = STEM_LD if stem else KH * KW * Cin
    if stem and (Cin, KH, KW) != (3, 7, 7):
        raise ValueError("stem weight must be [Cout, 3, 7, 7], got %s" % (tuple(weight.shape),))
    g = b = m = v = None
    eps = 0.0
    if bn is not None:
        g, b, m, v, eps = bn
        for t, n in ((g, "bn.weight"), (b, "bn.bias"), (m, "bn.running_mean"), (v, "bn.running_var")):
            _chk(t, n, ndim=1)
            if t.shape[0] != Cout:
                raise ValueError("%s has %d entries for %d output channels" % (n, t.shape[0], Cout))
    if conv_bias is not None:
        _chk(conv_bias, "conv_bias", ndim=1)
    wt = torch.empty(Cout, ld, device=weight.device, dtype=torch.bfloat16)
    bias = torch.empty(Cout, device=weight.device, dtype=torch.float32)
    _lib.call("mgnns_conv_fold_bn_bf16", _p(weight), _p(conv_bias), Cout, Cin, KH, KW, _p(g), _p(b), _p(m), _p(v), float(eps),
              1 if stem else 0, ld, _p(wt), _p(bias), _stream())
    return wt, bias


def stem_conv7(img, wt, bias, raw=False):
    """relu(bn1(conv1(img))): img [B,3,H,W] fp32 NCHW -> [B, OH, OW, 64] bf16 NHWC.  raw=True: the convolution alone,
    z = conv1(bf16(img); wt) without bias or ReLU, on the pack conv_fold_bn(w, None, None, stem=True) (the bias is not read)."""
    _chk(img, "img", ndim=4)
    _chk(wt, "wt", torch.bfloat16, 2)
    _chk(bias, "bias", ndim=1)
    B, C, H, W = img.shape
    if C != 3 or tuple(wt.shape) != (64, STEM_LD) or bias.shape[0] != 64:
        raise ValueError("stem expects img [B,3,H,W], wt [64,%d], bias [64]; got %s %s %s"
                         % (STEM_LD, tuple(img.shape), tuple(wt.shape), tuple(bias.shape)))
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64, device=img.device, dtype=torch.bfloat16)
    if raw:
        _launch("mgnns_stem_conv7_raw_fwd", _p(img), B, H, W, _p(wt), _p(y), _stream())
        return y
    _launch("mgnns_stem_conv7_fwd", _p(img), B, H, W, _p(wt), _p(bias), _p(y), _stream())
    return y


def maxpool3x3s2_nhwc(x):
    _chk(x, "x", torch.bfloat16, 4)
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, device=x.device, dtype=torch.bfloat16)
    _launch("mgnns_maxpool3x3s2_nhwc_fwd", _p(x), B, H, W, C, _p(y), _stream())
    return y


def conv_bf16_nhwc(x, wt, bias, ksize, stride=1, pad=0, residual=None, relu=True, out_nchw_f32=False):
    """relu?(conv(x) + bias + residual?): x [B,H,W,Cin] bf16, wt [Cout, k*k*Cin] bf16 (conv_fold_bn) -> [B,OH,OW,Cout]
    bf16, or [B,Cout,OH,OW] fp32 when out_nchw_f32."""
    _chk(x, "x", torch.bfloat16, 4)
    _chk(wt, "wt", torch.bfloat16, 2)
    _chk(bias, "bias", ndim=1)
    B, H, W, Cin = x.shape
    Cout = wt.shape[0]
    if wt.shape[1] != ksize * ksize * Cin or bias.shape[0] != Cout:
        raise ValueError("wt %s / bias %s do not match a %dx%d convolution of %d channels"
                         % (tuple(wt.shape), tuple(bias.shape), ksize, ksize, Cin))
    OH = (H + 2 * pad - ksize) // stride + 1
    OW = (W + 2 * pad - ksize) // stride + 1
    if residual is not None:
        _chk(residual, "residual", torch.bfloat16, 4)
        if tuple(residual.shape) != (B, OH, OW, Cout):
            raise ValueError("residual %s != output %s" % (tuple(residual.shape), (B, OH, OW, Cout)))
    if out_nchw_f32:
        y = torch.empty(B, Cout, OH, OW, device=x.device, dtype=torch.float32)
    else:
        y = torch.empty(B, OH, OW, Cout, device=x.device, dtype=torch.bfloat16)
    _launch("mgnns_conv_bf16_nhwc_fwd", _p(x), B, H, W, Cin, _p(wt), _p(bias), Cout, ksize, ksize, stride, pad, _p(residual),
            1 if relu else 0, 1 if out_nchw_f32 else 0, _p(y), _stream(), key=(ksize, Cin, Cout, stride, OH))
    return y


# ---- f4, training: backward of the bottleneck convolutions (csrc/conv_train.hip) -------------------------------------------
def conv_transpose_pack(wt, ksize):
    """The data gradient's pack of a folded weight: wt [Cout, k*k*Cin] bf16 -> wT [Cin, k*k*Cout] bf16, wT[c,(kh,kw,o)] = wt[o,(kh,kw,c)]."""
    _chk(wt, "wt", torch.bfloat16, 2)
    Cout, K = wt.shape
    if K % (ksize * ksize):
        raise ValueError("wt %s is no %dx%d folded weight" % (tuple(wt.shape), ksize, ksize))
    Cin = K // (ksize * ksize)
    wT = torch.empty(Cin, ksize * ksize * Cout, device=wt.device, dtype=torch.bfloat16)
    _launch("mgnns_conv_transpose_pack_bf16", _p(wt), Cout, Cin, ksize, ksize, _p(wT), _stream())
    return wT


def _conv_out(H, W, ksize, stride, pad):
    return (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1


def conv_dgrad_bf16_nhwc(dy, wT, in_hw, ksize, stride=1, pad=0, mask=None, add=None):
    """Data gradient of conv_bf16_nhwc: dy [B,OH,OW,Cout] bf16, wT [Cin, k*k*Cout] (conv_transpose_pack), in_hw = (H, W) of the
    convolution's input -> dx [B,H,W,Cin] bf16 = (mask > 0 ? sum + add : 0); mask / add [B,H,W,Cin] bf16 or None."""
    _chk(dy, "dy", torch.bfloat16, 4)
    _chk(wT, "wT", torch.bfloat16, 2)
    B, OH, OW, Cout = dy.shape
    H, W = in_hw
    Cin = wT.shape[0]
    if wT.shape[1] != ksize * ksize * Cout or (OH, OW) != _conv_out(H, W, ksize, stride, pad):
        raise ValueError("dy %s / wT %s do not match a %dx%d stride-%d pad-%d convolution of a %dx%d input"
                         % (tuple(dy.shape), tuple(wT.shape), ksize, ksize, stride, pad, H, W))
    for t, n in ((mask, "mask"), (add, "add")):
        if t is not None:
            _chk(t, n, torch.bfloat16, 4)
            if tuple(t.shape) != (B, H, W, Cin):
                raise ValueError("%s %s != input %s" % (n, tuple(t.shape), (B, H, W, Cin)))
    dx = torch.empty(B, H, W, Cin, device=dy.device, dtype=torch.bfloat16)
    _launch("mgnns_conv_dgrad_bf16_nhwc", _p(dy), B, H, W, Cin, _p(wT), Cout, ksize, ksize, stride, pad, _p(mask), _p(add), _p(dx),
            _stream(), key=(ksize, Cin, Cout, stride, OH))
    return dx


def conv_wgrad_bf16_nhwc(x, dy, ksize, stride=1, pad=0):
    """Weight gradient of conv_bf16_nhwc with respect to the FOLDED weight and bias: x [B,H,W,Cin], dy [B,OH,OW,Cout] bf16 ->
    (dW' [Cout, k*k*Cin] fp32 with k = (kh, kw, c), db' [Cout] fp32); pixels reduced in a fixed order."""
    _chk(x, "x", torch.bfloat16, 4)
    _chk(dy, "dy", torch.bfloat16, 4)
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    if tuple(dy.shape[:3]) != (B,) + _conv_out(H, W, ksize, stride, pad):
        raise ValueError("dy %s does not match a %dx%d stride-%d pad-%d convolution of x %s"
                         % (tuple(dy.shape), ksize, ksize, stride, pad, tuple(x.shape)))
    dW = torch.empty(Cout, ksize * ksize * Cin, device=x.device, dtype=torch.float32)
    db = torch.empty(Cout, device=x.device, dtype=torch.float32)
    L = _lib.lib()
    nbytes = L.mgnns_conv_wgrad_workspace_bytes(B, H, W, Cin, Cout, ksize, ksize, stride, pad)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    _launch("mgnns_conv_wgrad_bf16_nhwc", _p(x), _p(dy), B, H, W, Cin, Cout, ksize, ksize, stride, pad, _p(dW), _p(db), _p(ws), nbytes,
            _stream(), key=(ksize, Cin, Cout, stride, dy.shape[1]))
    return dW, db


def conv_bn_unfold(dwp, dbp, weight, bn, want=(True, True, True)):
    """Gradients of the fp32 master parameters from those of the folded pair (conv_wgrad_bf16_nhwc): weight [Cout,Cin,KH,KW],
    bn = (gamma, running_mean, running_var, eps) -> (dW like weight, dgamma [Cout], dbeta [Cout]); want picks which are
    computed (the others are None)."""
    _chk(weight, "weight", ndim=4)
    Cout, Cin, KH, KW = weight.shape
    _chk(dwp, "dwp", ndim=2)
    _chk(dbp, "dbp", ndim=1)
    g, m, v, eps = bn
    for t, n in ((g, "bn.weight"), (m, "bn.running_mean"), (v, "bn.running_var"), (dbp, "dbp")):
        _chk(t, n, ndim=1)
        if t.shape[0] != Cout:
            raise ValueError("%s has %d entries for %d output channels" % (n, t.shape[0], Cout))
    if tuple(dwp.shape) != (Cout, KH * KW * Cin):
        raise ValueError("dwp %s does not match weight %s" % (tuple(dwp.shape), tuple(weight.shape)))
    dW = torch.empty_like(weight) if want[0] else None
    dg = torch.empty(Cout, device=weight.device, dtype=torch.float32) if want[1] else None
    dbeta = torch.empty(Cout, device=weight.device, dtype=torch.float32) if want[2] else None
    _launch("mgnns_conv_bn_unfold", _p(dwp), _p(dbp), _p(weight), _p(g), _p(m), _p(v), float(eps), Cout, Cin, KH, KW, _p(dW), _p(dg),
            _p(dbeta), _stream())
    return dW, dg, dbeta


def map_grad_relu_nhwc(fmap, dmap):
    """The entry of the trunk's backward: fmap (the post-ReLU fp32 NCHW map) and its gradient [B,C,h,w] -> bf16 NHWC
    g = (fmap > 0 ? dmap : 0)."""
    _chk(fmap, "map", ndim=4)
    _chk(dmap, "dmap", ndim=4)
    if fmap.shape != dmap.shape:
        raise ValueError("map %s / dmap %s" % (tuple(fmap.shape), tuple(dmap.shape)))
    B, C, h, w = fmap.shape
    g = torch.empty(B, h, w, C, device=fmap.device, dtype=torch.bfloat16)
    _launch("mgnns_map_grad_relu_nhwc_bf16", _p(fmap), _p(dmap), B, C, h * w, _p(g), _stream())
    return g


# ---- f4, training with batch statistics: BatchNorm over NHWC bf16 activations (csrc/bn_train.hip) ---------------------------
def _bn_rows(t, name):
    """(M, C) of an [..., C] bf16 activation; the refusals the kernels share."""
    _chk(t, name, torch.bfloat16)
    if t.dim() < 2:
        raise ValueError("%s must be [..., C] with at least 2 dimensions, got shape %s" % (name, tuple(t.shape)))
    C = t.shape[-1]
    M = t.numel() // C if C else 0
    if C == 0 or C % 8:
        raise ValueError("%s: the channel count must be a positive multiple of 8, got C=%d" % (name, C))
    if M < 2:
        raise ValueError("%s: batch statistics need at least two values per channel, got %d (shape %s)" % (name, M, tuple(t.shape)))
    return M, C


def _bn_vec(t, name, C):
    _chk(t, name, ndim=1)
    if t.shape[0] != C:
        raise ValueError("%s has %d entries for %d channels" % (name, t.shape[0], C))
    return t


def bn_stats_bf16_nhwc(z, eps, running=None, momentum=0.1, want_var=False):
    """Batch statistics of z [..., C] bf16 over all leading axes -> (mean [C], rstd [C] = 1 / sqrt(var_biased + eps)) fp32, plus
    var_biased when want_var.  running = (running_mean, running_var): updated in place by the same launch, running_mean = (1 - m)
    running_mean + m mean, running_var = (1 - m) running_var + m var_biased M / (M - 1) (num_batches_tracked is the caller's).
    Rows are reduced in an order fixed by the shape: bit-identical from call to call."""
    M, C = _bn_rows(z, "z")
    rm = rv = None
    if running is not None:
        if momentum is None:
            raise NotImplementedError("bn_stats_bf16_nhwc: momentum=None (the cumulative moving average) is not implemented")
        rm, rv = (_bn_vec(t, n, C) for t, n in zip(running, ("running_mean", "running_var")))
    m = 0.0 if momentum is None else float(momentum)
    if not 0.0 <= m <= 1.0:
        raise ValueError("momentum must be in [0, 1], got %r" % (momentum,))
    mean = torch.empty(C, device=z.device, dtype=torch.float32)
    rstd = torch.empty(C, device=z.device, dtype=torch.float32)
    var = torch.empty(C, device=z.device, dtype=torch.float32) if want_var else None
    L = _lib.lib()
    nbytes = L.mgnns_bn_stats_workspace_bytes(M, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    _launch("mgnns_bn_stats_bf16", _p(z), M, C, float(eps), m, _p(mean), _p(rstd), _p(var), _p(rm), _p(rv), _p(ws), nbytes, _stream(),
            key=(M, C))
    if rm is not None:                                  # written in place through their addresses: what derives from them is stale
        torch.autograd.graph.increment_version(rm)
        torch.autograd.graph.increment_version(rv)
    return (mean, rstd, var) if want_var else (mean, rstd)


def bn_apply_bf16_nhwc(z, mean, rstd, gamma, beta, residual=None, relu=True, out_nchw_f32=False):
    """relu?(a z + b + residual?) with a = gamma rstd, b = beta - mean a: z [..., C] bf16 -> bf16 of z's shape, or, with
    out_nchw_f32, z [B, OH, OW, C] -> the unrounded fp32 [B, C, OH, OW] map."""
    M, C = _bn_rows(z, "z")
    for t, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta")):
        _bn_vec(t, n, C)
    if residual is not None:
        _chk(residual, "residual", torch.bfloat16)
        if residual.shape != z.shape:
            raise ValueError("residual %s != z %s" % (tuple(residual.shape), tuple(z.shape)))
    P = 0
    if out_nchw_f32:
        if z.dim() != 4:
            raise ValueError("out_nchw_f32 needs z as [B, OH, OW, C], got shape %s" % (tuple(z.shape),))
        B, OH, OW, _ = z.shape
        P = OH * OW
        y = torch.empty(B, C, OH, OW, device=z.device, dtype=torch.float32)
    else:
        y = torch.empty_like(z)
    _launch("mgnns_bn_apply_bf16", _p(z), M, C, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(residual), 1 if relu else 0,
            1 if out_nchw_f32 else 0, P, _p(y), _stream(), key=(M, C, bool(out_nchw_f32)))
    return y


def bn_backward_bf16_nhwc(g, z, mean, rstd, gamma, want=(True, True)):
    """Backward of training-mode BatchNorm: g (the gradient of its output, already masked by the producer's ReLU) and the saved z,
    both [..., C] bf16 -> (g_z bf16 like z, dgamma [C], dbeta [C]) with xhat = (z - mean) rstd, dbeta = sum g, dgamma = sum g xhat,
    g_z = bf16(gamma rstd (g - dbeta / M - xhat dgamma / M)); want = (dgamma?, dbeta?) picks which sums are returned (else None)."""
    M, C = _bn_rows(z, "z")
    _chk(g, "g", torch.bfloat16)
    if g.shape != z.shape:
        raise ValueError("g %s != z %s" % (tuple(g.shape), tuple(z.shape)))
    for t, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma")):
        _bn_vec(t, n, C)
    gz = torch.empty_like(z)
    dgamma = torch.empty(C, device=z.device, dtype=torch.float32) if want[0] else None
    dbeta = torch.empty(C, device=z.device, dtype=torch.float32) if want[1] else None
    L = _lib.lib()
    nbytes = L.mgnns_bn_backward_workspace_bytes(M, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    _launch("mgnns_bn_backward_bf16", _p(g), _p(z), M, C, _p(mean), _p(rstd), _p(gamma), _p(gz), _p(dgamma), _p(dbeta), _p(ws), nbytes,
            _stream(), key=(M, C))
    return gz, dgamma, dbeta


# ---- f4, training: the stem's backward (csrc/stem_train.hip) ------------------------------------------------------------------
def stem_wgrad(img, g):
    """Weight gradient of the stem convolution: img [B,3,H,W] fp32 NCHW (rounded to bf16 as stem_conv7 rounds it), g [B,OH,OW,64]
    bf16 NHWC (the gradient of the convolution's output) -> (dW' [64,147] fp32 with k = (kh, kw, c) -- the layout conv_bn_unfold
    takes --, db' [64] fp32); pixels reduced in an order fixed by the shape."""
    _chk(img, "img", ndim=4)
    _chk(g, "g", torch.bfloat16, 4)
    B, C, H, W = img.shape
    if C != 3 or H < 7 or W < 7:
        raise ValueError("stem expects img [B,3,H,W] with H, W >= 7, got %s" % (tuple(img.shape),))
    if tuple(g.shape) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64):
        raise ValueError("g %s does not match the stem's output [%d,%d,%d,64] for img %s"
                         % (tuple(g.shape), B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, tuple(img.shape)))
    dW = torch.empty(64, 147, device=img.device, dtype=torch.float32)
    db = torch.empty(64, device=img.device, dtype=torch.float32)
    L = _lib.lib()
    nbytes = L.mgnns_stem_wgrad_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device) if nbytes else None
    _launch("mgnns_stem_wgrad", _p(img), _p(g), B, H, W, _p(dW), _p(db), _p(ws), nbytes, _stream(), key=(H, W))
    return dW, db


def maxpool3x3s2_bwd_nhwc(x, g_y, relu_mask=False):
    """Backward of maxpool3x3s2_nhwc: x [B,H,W,C] bf16 (the pool's input), g_y [B,OH,OW,C] bf16 -> g_x [B,H,W,C] bf16.  A pixel takes
    g_y of the windows whose first maximum it is (row-major scan, strict >: torch's rule), summed in fp32 and rounded once;
    relu_mask=True also zeroes g_x where x <= 0 (a ReLU whose output x is)."""
    _chk(x, "x", torch.bfloat16, 4)
    _chk(g_y, "g_y", torch.bfloat16, 4)
    B, H, W, C = x.shape
    if C == 0 or C % 8:
        raise ValueError("x: the channel count must be a positive multiple of 8, got C=%d" % C)
    if H == 0 or W == 0 or tuple(g_y.shape) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C):
        raise ValueError("g_y %s does not match the pooled shape of x %s" % (tuple(g_y.shape), tuple(x.shape)))
    g_x = torch.empty_like(x)
    _launch("mgnns_maxpool3x3s2_nhwc_bwd", _p(x), _p(g_y), B, H, W, C, 1 if relu_mask else 0, _p(g_x), _stream(), key=(bool(relu_mask),))
    return g_x


# ---- f4, input half: crop + Pillow's bilinear resize + flip + ToTensor + Normalize (csrc/image_prep.hip) -------------------------
IMAGE_DESC = 10           # int64 per image: offset, height, width, crop x, y, w, h, flip, horizontal plan, vertical plan
IMAGE_MAX_EXTENT = 8192
IMAGE_MAX_SIZE = 1024


def _chk_host(t, name, dtype, cols):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor" % name)
    if t.is_cuda:
        raise ValueError("%s is the HOST copy that is validated before the launch; got a tensor on %s" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("%s must be [n,%d], got shape %s" % (name, cols, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def image_prep(pixels, desc, desc_dev, plan_table, plan_table_dev, plan_data, lut, size_h, size_w, out=None):
    """A batch of decoded uint8 HWC images of different sizes -> [B,3,size_h,size_w] fp32, what stem_conv7 reads: crop, Pillow's 8-bit
    bilinear resize, mirror, lut[c][v], in one launch (include/mgnns_hip.h, "f4 (input half)").  pixels: uint8 [n] on the GPU, every
    image on a 16-byte boundary and at least 16 bytes of slack behind the last.  desc [B,10] int64 and plan_table [P,4] int32 are HOST
    tensors, validated here; desc_dev / plan_table_dev are their device copies, which the kernel reads (the caller stages them: this
    function copies nothing and does not synchronise, so it can be captured into a hipGraph over static buffers -- the validation
    then covers the capture's call only, and the kernel's own re-check turns a bad descriptor into NaN).  plan_data: int32 [m] on
    the GPU; lut [3,256] fp32 on the GPU."""
    _chk(pixels, "pixels", torch.uint8, 1)
    _chk_host(desc, "desc", torch.int64, IMAGE_DESC)
    _chk_host(plan_table, "plan_table", torch.int32, 4)
    _chk(desc_dev, "desc_dev", torch.int64, 2)
    _chk(plan_table_dev, "plan_table_dev", torch.int32, 2)
    _chk(plan_data, "plan_data", torch.int32, 1)
    _chk(lut, "lut", ndim=2)
    size_h, size_w = int(size_h), int(size_w)
    if not (1 <= size_h <= IMAGE_MAX_SIZE and 1 <= size_w <= IMAGE_MAX_SIZE):
        raise ValueError("output size %dx%d unsupported (1..%d)" % (size_h, size_w, IMAGE_MAX_SIZE))
    B, P = desc.shape[0], plan_table.shape[0]
    if tuple(desc_dev.shape) != tuple(desc.shape) or tuple(plan_table_dev.shape) != tuple(plan_table.shape):
        raise ValueError("desc_dev %s / plan_table_dev %s must have the shapes of their host copies %s / %s"
                         % (tuple(desc_dev.shape), tuple(plan_table_dev.shape), tuple(desc.shape), tuple(plan_table.shape)))
    if tuple(lut.shape) != (3, 256):
        raise ValueError("lut must be [3,256], got %s" % (tuple(lut.shape),))
    for t, name in ((desc_dev, "desc_dev"), (plan_table_dev, "plan_table_dev"), (plan_data, "plan_data"), (lut, "lut")):
        if t.device != pixels.device:
            raise ValueError("%s is on %s, pixels on %s" % (name, t.device, pixels.device))
    if pixels.data_ptr() % 16:
        raise ValueError("pixels must start on a 16-byte boundary")
    if P:
        o, ks, n, S = plan_table.unbind(1)
        bad = (o < 0) | (ks < 1) | (n < 1) | (n > IMAGE_MAX_EXTENT) | (S < 1) | (o.long() + S.long() * (2 + ks.long()) > plan_data.numel())
        if bool(bad.any()):
            raise ValueError("plan_table row %d is not a plan inside plan_data (%d int32): %s"
                             % (int(bad.nonzero()[0]), plan_data.numel(), plan_table[int(bad.nonzero()[0])].tolist()))
    if B:
        off, H, W, cx, cy, cw, ch, flip, ix, iy = desc.unbind(1)

        def refuse(mask, what):
            if bool(mask.any()):
                i = int(mask.nonzero()[0])
                raise ValueError("image %d: %s (descriptor %s)" % (i, what, desc[i].tolist()))

        refuse((H < 1) | (H > IMAGE_MAX_EXTENT) | (W < 1) | (W > IMAGE_MAX_EXTENT), "source extent outside 1..%d" % IMAGE_MAX_EXTENT)
        refuse((off < 0) | (off % 16 != 0), "offset is not a non-negative multiple of 16")
        # (written without sums that a huge int64 field could wrap)
        refuse(off > pixels.numel() - H * W * 3 - 16, "image plus 16 bytes of slack does not fit the pixel buffer of %d bytes" % pixels.numel())
        refuse((cx < 0) | (cy < 0) | (cw < 1) | (ch < 1) | (cw > W) | (ch > H) | (cx > W - cw) | (cy > H - ch), "crop outside the image")
        refuse((flip != 0) & (flip != 1), "flip must be 0 or 1")
        refuse((ix < 0) | (ix >= P) | (iy < 0) | (iy >= P), "plan index outside 0..%d" % (P - 1))
        pt = plan_table.long()
        refuse((pt[ix, 2] != cw) | (pt[ix, 3] != size_w), "horizontal plan is not for (crop width, %d)" % size_w)
        refuse((pt[iy, 2] != ch) | (pt[iy, 3] != size_h), "vertical plan is not for (crop height, %d)" % size_h)
    if out is None:
        out = torch.empty(B, 3, size_h, size_w, device=pixels.device, dtype=torch.float32)
    else:
        _chk(out, "out", ndim=4)
        if tuple(out.shape) != (B, 3, size_h, size_w) or out.device != pixels.device:
            raise ValueError("out must be [%d,3,%d,%d] on %s, got %s on %s" % (B, size_h, size_w, pixels.device, tuple(out.shape), out.device))
    _launch("mgnns_image_prep_fwd", _p(pixels), pixels.numel(), _p(desc_dev), B, _p(plan_table_dev), P, _p(plan_data), plan_data.numel(),
            _p(lut), size_h, size_w, _p(out), _stream(), key=(size_h, size_w))
    return out


# ---- f4, file half: baseline JPEG files -> the packed RGB8 pixel buffer image_prep reads (csrc/jpeg_decode.hip) --------------------
JPEG_IMG = 16             # int64 per image: kind, width, height, components, Y sampling h, v, MCUs per row, MCU rows, quantisation /
#                           DC / AC table ids (a byte per component), table set, coefficient / plane / pixel offset, end of the padding
JPEG_SEG = 5              # int64 per segment: image, begin, end (bytes in the data buffer), first MCU, MCUs
JPEG_STATUS = {0: "ok", 1: "ran out of data", 2: "invalid Huffman code", 3: "coefficient index above 63",
               4: "record refused by the kernel"}
JPEG_MAX_GAP = 256        # bytes of padding behind an image that the decoder zeroes


class JpegDecodeError(ValueError):
    """Some segments did not decode.  failed: [(image, segment, status word)], segment counted over the batch; pixels: the pixel
    buffer -- every image not named in `failed` is decoded in it.  scans: {segment: the scan's number in its file} for the segments
    of progressive files (jpeg_decode_progressive counts the baseline segments first, then the progressive ones level by level)."""

    def __init__(self, failed, pixels, scans=None):
        self.failed, self.pixels, self.scans = failed, pixels, dict(scans or {})
        by_image = {}
        for i, s, st in failed:
            where = "scan %d, segment %d" % (self.scans[s], s) if s in self.scans else "segment %d" % s
            by_image.setdefault(i, []).append("%s: %s (status %d)" % (where, JPEG_STATUS.get(st, "?"), st))
        ValueError.__init__(self, "JPEG decode failed for %d image(s): %s" % (
            len(by_image), "; ".join("image %d: %s" % (i, ", ".join(v[:4]) + (" ..." if len(v) > 4 else "")) for i, v in sorted(by_image.items()))))


def _jpeg_check_images(img, n_sets, n_q, pixels):
    """The image records of a decode, checked on the host as the kernels check them.  n_q: latched quantisation sets of progressive
    images (kind 2; 0 = none accepted).  -> (refuse, decoded mask, MCUs, blocks per image, workspace elements, plane bytes)"""
    kind, W, H, nc, hs, vs, mcux, mcuy, tq, td, ta, tset, coef_off, plane_off, pix_off, pix_end = img.unbind(1)

    def refuse(mask, what, rec=img, noun="image"):
        if bool(mask.any()):
            i = int(mask.nonzero()[0])
            raise ValueError("%s %d: %s (record %s)" % (noun, i, what, rec[i].tolist()))

    refuse((kind != 0) & (kind != 1) & ((kind != 2) | (n_q == 0)), "kind must be 0 or 1" if n_q == 0 else "kind must be 0, 1 or 2")
    refuse((W < 1) | (W > IMAGE_MAX_EXTENT) | (H < 1) | (H > IMAGE_MAX_EXTENT), "extent outside 1..%d" % IMAGE_MAX_EXTENT)
    refuse((pix_off < 0) | (pix_off % 16 != 0), "pixel offset is not a non-negative multiple of 16")
    refuse((pix_end > pixels.numel()) | (pix_end - pix_off < W * H * 3) | (pix_end - pix_off - W * H * 3 > JPEG_MAX_GAP),
           "pixels and their padding (at most %d bytes) do not fit the pixel buffer of %d bytes" % (JPEG_MAX_GAP, pixels.numel()))
    dec, prog = kind != 0, kind == 2
    sampling_ok = ((nc == 1) & (hs == 1) & (vs == 1)) | ((nc == 3) & (((hs == 1) & (vs == 1)) | ((hs == 2) & ((vs == 1) | (vs == 2)))))
    refuse(dec & ~sampling_ok, "components / sampling not supported")
    hs1, vs1 = hs.clamp(1, 2), vs.clamp(1, 2)
    refuse(dec & ((mcux != (W + 8 * hs1 - 1) // (8 * hs1)) | (mcuy != (H + 8 * vs1 - 1) // (8 * vs1))), "MCU counts do not match the extent")
    refuse(dec & ~prog & ((tset < 0) | (tset >= n_sets)), "table set outside 0..%d" % (n_sets - 1))
    refuse(prog & ((tset < 0) | (tset >= n_q)), "quantisation set outside 0..%d" % (n_q - 1))
    refuse(dec & ~prog & ((tq < 0) | (td < 0) | (ta < 0) | (((tq | td | ta) & ~0x030303) != 0)), "table ids must be 0..3")
    nmcu = mcux * mcuy
    blocks = torch.where(nc == 1, nmcu, nmcu * (hs * vs + 2)) * dec
    refuse(dec & ((coef_off < 0) | (coef_off % 64 != 0) | (plane_off < 0) | (plane_off % 64 != 0)), "workspace offsets must be non-negative multiples of 64")
    coef_elems = int((coef_off * dec + blocks * 64).max())
    plane_bytes = int((plane_off * dec + blocks * 64).max())
    if coef_elems > (1 << 34):
        raise ValueError("the batch needs a coefficient workspace of %d int16 -- decode it in smaller batches" % coef_elems)
    return refuse, dec, nmcu, blocks, coef_elems, plane_bytes


def jpeg_tableset_bytes():
    return int(_lib.lib().mgnns_jpeg_tableset_bytes())


def jpeg_decode(data, img, img_dev, seg, seg_dev, tables, pixels, stages=7, check=True):
    """Decode a batch of parsed baseline JPEG files into `pixels` (include/mgnns_hip.h, "f4 (file half)"): Huffman decoding with one
    lane per segment, dequantisation + jidctint, chroma upsampling + colour conversion, three launches on the current stream.
    data: uint8 [n] on the GPU, the files' bytes; img [B,16] / seg [S,5] int64 are HOST tensors, validated here, img_dev / seg_dev
    their device copies; tables: uint8 [n_sets, jpeg_tableset_bytes()] on the GPU; pixels: uint8 [m] on the GPU, written at the
    records' offsets (an image of kind 0 is skipped: the caller stages its pixels).  With check=True the [S] status words come back
    in one small copy on the current stream and a JpegDecodeError (a ValueError) names every image with a segment that is not ok;
    with check=False nothing synchronises and the status tensor is returned for the caller to read.  -> the status tensor."""
    _chk(data, "data", torch.uint8, 1)
    _chk(pixels, "pixels", torch.uint8, 1)
    _chk(tables, "tables", torch.uint8, 2)
    _chk_host(img, "img", torch.int64, JPEG_IMG)
    _chk_host(seg, "seg", torch.int64, JPEG_SEG)
    _chk(img_dev, "img_dev", torch.int64, 2)
    _chk(seg_dev, "seg_dev", torch.int64, 2)
    B, S, n_sets = img.shape[0], seg.shape[0], tables.shape[0]
    if tuple(img_dev.shape) != tuple(img.shape) or tuple(seg_dev.shape) != tuple(seg.shape):
        raise ValueError("img_dev %s / seg_dev %s must have the shapes of their host copies %s / %s"
                         % (tuple(img_dev.shape), tuple(seg_dev.shape), tuple(img.shape), tuple(seg.shape)))
    if tables.shape[1] != jpeg_tableset_bytes():
        raise ValueError("tables must be [n_sets,%d], got %s" % (jpeg_tableset_bytes(), tuple(tables.shape)))
    for t, name in ((img_dev, "img_dev"), (seg_dev, "seg_dev"), (tables, "tables"), (pixels, "pixels")):
        if t.device != data.device:
            raise ValueError("%s is on %s, data on %s" % (name, t.device, data.device))
    if B > 65535:
        raise ValueError("at most 65535 images per batch, got %d" % B)
    if int(stages) < 1 or int(stages) > 7:
        raise ValueError("stages is a mask of 1 (entropy), 2 (IDCT), 4 (colour), got %s" % (stages,))
    status = torch.zeros(S, dtype=torch.int32, device=data.device)
    if B == 0 or S == 0:
        return status
    refuse, dec, nmcu, blocks, coef_elems, plane_bytes = _jpeg_check_images(img, n_sets, 0, pixels)
    W, H = img[:, 1], img[:, 2]
    si, sb, se, m0, mn = seg.unbind(1)
    refuse((si < 0) | (si >= B), "image index outside the batch", seg, "segment")
    refuse(~dec[si], "segment of an image that is not decoded", seg, "segment")
    refuse((sb < 0) | (sb > se) | (se > data.numel()), "byte range outside the data buffer of %d bytes" % data.numel(), seg, "segment")
    refuse((m0 < 0) | (mn < 1) | (m0 > nmcu[si] - mn), "MCU range outside the image", seg, "segment")
    coef = torch.empty(max(coef_elems, 64), dtype=torch.int16, device=data.device)
    planes = torch.empty(max(plane_bytes, 64), dtype=torch.uint8, device=data.device)
    _launch("mgnns_jpeg_decode_fwd", _p(data), data.numel(), _p(img_dev), B, _p(seg_dev), S, _p(tables), n_sets, _p(coef), coef.numel(),
            _p(planes), planes.numel(), _p(pixels), pixels.numel(), max(int(blocks.max()), 1), max(int((W * H * dec).max()), 1),
            int(stages), _p(status), _stream(), key=(B, S))
    if check:
        st = status.cpu()                      # one small D2H on the current stream; it also ends the workspaces' use
        bad = st.nonzero().flatten().tolist()
        if bad:
            raise JpegDecodeError([(int(si[s]), s, int(st[s])) for s in bad], pixels)
    return status


JPEG_PSEG = 12            # int64 per segment of a progressive scan: image, begin, end, first unit, units, component mask, Ss, Se, Ah, Al,
#                           pool indices (16 bits each: DC of component 0, 1, 2, AC; 0xFFFF = none), the scan's number in its file
JPEG_QSET = 192           # bytes of one latched quantisation set: [3][64], a table per component in natural order
JPEG_MAX_LEVELS = 64


def jpeg_huff_bytes():
    return int(_lib.lib().mgnns_jpeg_huff_bytes())


def jpeg_decode_progressive(data, img, img_dev, seg, seg_dev, tables, pseg, pseg_dev, level_counts, pool, qsets, pixels, stages=7, check=True,
                            _split=0, _layouts=None):
    """Decode a batch that may mix baseline and progressive files into `pixels` (include/mgnns_jpeg_progressive.h): the workspace zeroed, jpeg_decode's entropy kernel over the baseline segments, one launch of the progressive entropy
    kernel per level, then the IDCT and colour kernels over all images -- on the current stream.  As jpeg_decode, and: an image of
    kind 2 is progressive (its table-set field counts `qsets`); pseg [P,12] int64 HOST tensor sorted by level, pseg_dev its device
    copy; level_counts: segments per level (a list); pool: uint8 [n_pool, jpeg_huff_bytes()] and qsets: uint8 [n_q, 192] on the
    GPU; stages: jpeg_decode's mask (1 = every entropy launch).  -> the status tensor [S + P]: the baseline segments' words, then the
    progressive ones' in pseg's order."""
    _chk(data, "data", torch.uint8, 1)
    _chk(pixels, "pixels", torch.uint8, 1)
    _chk(tables, "tables", torch.uint8, 2)
    _chk(pool, "pool", torch.uint8, 2)
    _chk(qsets, "qsets", torch.uint8, 2)
    _chk_host(img, "img", torch.int64, JPEG_IMG)
    _chk_host(seg, "seg", torch.int64, JPEG_SEG)
    _chk_host(pseg, "pseg", torch.int64, JPEG_PSEG)
    _chk(img_dev, "img_dev", torch.int64, 2)
    _chk(seg_dev, "seg_dev", torch.int64, 2)
    _chk(pseg_dev, "pseg_dev", torch.int64, 2)
    B, S, P, n_sets, n_pool, n_q = img.shape[0], seg.shape[0], pseg.shape[0], tables.shape[0], pool.shape[0], qsets.shape[0]
    L = 0
    if _layouts is not None:                   # (jpeg_decode_layouts: the segment records of the images of kind 3, host and device)
        lseg, lseg_dev = _layouts
        _chk_host(lseg, "lseg", torch.int64, JPEG_SEG)
        _chk(lseg_dev, "lseg_dev", torch.int64, 2)
        L = lseg.shape[0]
        if tuple(lseg_dev.shape) != tuple(lseg.shape) or lseg_dev.device != data.device:
            raise ValueError("lseg_dev %s on %s must have the shape of its host copy %s and lie on %s"
                             % (tuple(lseg_dev.shape), lseg_dev.device, tuple(lseg.shape), data.device))
    for host, dev, name in ((img, img_dev, "img_dev"), (seg, seg_dev, "seg_dev"), (pseg, pseg_dev, "pseg_dev")):
        if tuple(dev.shape) != tuple(host.shape):
            raise ValueError("%s %s must have the shape of its host copy %s" % (name, tuple(dev.shape), tuple(host.shape)))
    if tables.shape[1] != jpeg_tableset_bytes() or pool.shape[1] != jpeg_huff_bytes() or qsets.shape[1] != JPEG_QSET:
        raise ValueError("tables must be [n_sets,%d], pool [n_pool,%d], qsets [n_q,%d], got %s, %s, %s" % (
            jpeg_tableset_bytes(), jpeg_huff_bytes(), JPEG_QSET, tuple(tables.shape), tuple(pool.shape), tuple(qsets.shape)))
    for t, name in ((img_dev, "img_dev"), (seg_dev, "seg_dev"), (pseg_dev, "pseg_dev"), (tables, "tables"), (pool, "pool"), (qsets, "qsets"),
                    (pixels, "pixels")):
        if t.device != data.device:
            raise ValueError("%s is on %s, data on %s" % (name, t.device, data.device))
    if B > 65535:
        raise ValueError("at most 65535 images per batch, got %d" % B)
    level_counts = [int(v) for v in level_counts]
    if len(level_counts) > JPEG_MAX_LEVELS or any(v < 0 for v in level_counts) or sum(level_counts) != P:
        raise ValueError("level_counts must be at most %d non-negative counts that add up to the %d progressive segments, got %s"
                         % (JPEG_MAX_LEVELS, P, level_counts))
    if n_pool >= 0xFFFF:
        raise ValueError("at most 65534 tables in the pool, got %d" % n_pool)
    if int(stages) < 1 or int(stages) > 7:
        raise ValueError("stages is a mask of 1 (entropy), 2 (IDCT), 4 (colour), got %s" % (stages,))
    status = torch.zeros(S + P + L, dtype=torch.int32, device=data.device)
    if B == 0 or S + P + L == 0:
        return status
    full = img
    if _layouts is not None:                   # the records of kind 3 have a check of their own; here they count as staged pixels
        img = img.clone()
        img[full[:, 0] == 3, 0] = 0
    refuse, dec, nmcu, blocks, coef_elems, plane_bytes = _jpeg_check_images(img, n_sets, n_q, pixels)
    lblocks = lpixels = 0
    if _layouts is not None:
        lay, lmcu, lb = _jpeg_check_layouts(full, n_sets, refuse)
        li, lb_, le, l0, ln = lseg.unbind(1)
        refuse((li < 0) | (li >= B), "image index outside the batch", lseg, "layout segment")
        refuse(~lay[li], "layout segment of an image that is not of kind 3", lseg, "layout segment")
        refuse((lb_ < 0) | (lb_ > le) | (le > data.numel()), "byte range outside the data buffer of %d bytes" % data.numel(), lseg, "layout segment")
        refuse((l0 < 0) | (ln < 1) | (l0 > lmcu[li] - ln), "MCU range outside the image", lseg, "layout segment")
        if bool(lay.any()):
            coef_elems = max(coef_elems, int(((full[:, 12] + lb * 64) * lay).max()))
            plane_bytes = max(plane_bytes, int(((full[:, 13] + lb * 64) * lay).max()))
            lblocks, lpixels = int(lb.max()), int((full[:, 1] * full[:, 2] * lay).max())
        if coef_elems > (1 << 34):
            raise ValueError("the batch needs a coefficient workspace of %d int16 -- decode it in smaller batches" % coef_elems)
    kind, W, H, nc, hs, vs, mcux = (img[:, k] for k in range(7))
    si, sb, se, m0, mn = seg.unbind(1)
    refuse((si < 0) | (si >= B), "image index outside the batch", seg, "segment")
    refuse(kind[si] != 1, "baseline segment of an image that is not a baseline file", seg, "segment")
    refuse((sb < 0) | (sb > se) | (se > data.numel()), "byte range outside the data buffer of %d bytes" % data.numel(), seg, "segment")
    refuse((m0 < 0) | (mn < 1) | (m0 > nmcu[si] - mn), "MCU range outside the image", seg, "segment")
    pi, pb, pe, u0, un, comps, ss, se_, ah, al, tabs, _ = pseg.unbind(1)
    noun = "progressive segment"
    refuse((pi < 0) | (pi >= B), "image index outside the batch", pseg, noun)
    refuse(kind[pi] != 2, "segment of an image that is not a progressive file", pseg, noun)
    refuse((pb < 0) | (pb > pe) | (pe > data.numel()), "byte range outside the data buffer of %d bytes" % data.numel(), pseg, noun)
    refuse((comps < 1) | (comps > torch.where(nc[pi] == 1, 1, 7)), "component mask outside the frame", pseg, noun)
    single = (comps == 1) | (comps == 2) | (comps == 4)
    refuse(torch.where(ss == 0, se_ != 0, (ss < 1) | (se_ < ss) | (se_ > 63) | ~single), "Ss / Se are no band of a progressive scan", pseg, noun)
    refuse((al < 0) | (al > 13) | ((ah != 0) & (ah != al + 1)), "Ah / Al are no successive approximation", pseg, noun)
    hp, vp, Wp, Hp = hs[pi], vs[pi], W[pi], H[pi]
    hc, vc = torch.where(comps == 1, hp, 1), torch.where(comps == 1, vp, 1)
    units = torch.where(single, ((((Wp * hc + hp - 1) // hp) + 7) // 8) * ((((Hp * vc + vp - 1) // vp) + 7) // 8), nmcu[pi])
    refuse((u0 < 0) | (un < 1) | (u0 > units - un), "unit range outside the scan", pseg, noun)
    t4 = torch.stack([(tabs >> (16 * k)) & 0xFFFF for k in range(4)], 1)
    refuse(((t4 != 0xFFFF) & (t4 >= n_pool)).any(1), "table outside the pool of %d" % n_pool, pseg, noun)
    need = torch.stack([(ss == 0) & (ah == 0) & ((comps >> c) & 1 == 1) for c in range(3)] + [ss != 0], 1)
    refuse((need & (t4 == 0xFFFF)).any(1), "the scan reads a table the record does not name", pseg, noun)
    lv = torch.tensor(level_counts, dtype=torch.int32)
    coef = torch.empty(max(coef_elems, 64), dtype=torch.int16, device=data.device)
    planes = torch.empty(max(plane_bytes, 64), dtype=torch.uint8, device=data.device)
    # (_split: jpeg_decode_split's chunk size -- the same arguments and one more, to the entry point of include/mgnns_jpeg_split.h)
    if _layouts is not None:                   # (include/mgnns_jpeg_layouts.h: the same launches, then those of the images of kind 3)
        _launch("mgnns_jpeg_decode_layouts_fwd", _p(data), data.numel(), _p(img_dev), B, _p(seg_dev) if S else None, S,
                _p(tables) if n_sets else None, n_sets, _p(pseg_dev) if P else None, lv.data_ptr() if len(level_counts) else None,
                len(level_counts), _p(pool) if n_pool else None, n_pool, _p(qsets) if n_q else None, n_q, _p(lseg_dev) if L else None, L,
                _p(coef), coef.numel(), _p(planes), planes.numel(), _p(pixels), pixels.numel(), max(int(blocks.max()), 1),
                max(int((W * H * dec).max()), 1), max(lblocks, 1), max(lpixels, 1), int(stages), _p(status), _stream(), int(_split),
                key=(B, S, tuple(level_counts), L))
    else:
        _launch("mgnns_jpeg_decode_split_fwd" if _split else "mgnns_jpeg_decode_progressive_fwd", _p(data), data.numel(), _p(img_dev), B,
                _p(seg_dev) if S else None, S,
                _p(tables) if n_sets else None, n_sets, _p(pseg_dev) if P else None, lv.data_ptr() if len(level_counts) else None, len(level_counts),
                _p(pool) if n_pool else None, n_pool, _p(qsets) if n_q else None, n_q, _p(coef), coef.numel(), _p(planes), planes.numel(),
                _p(pixels), pixels.numel(), max(int(blocks.max()), 1), max(int((W * H * dec).max()), 1), int(stages), _p(status), _stream(),
                *((int(_split),) if _split else ()), key=(B, S, tuple(level_counts)))
    if check:
        st = status.cpu()                      # one small D2H on the current stream; it also ends the workspaces' use
        bad = st.nonzero().flatten().tolist()
        if bad:
            owner = lambda s: int(si[s]) if s < S else int(pi[s - S]) if s < S + P else int(li[s - S - P])
            raise JpegDecodeError([(owner(s), s, int(st[s])) for s in bad], pixels, {s: int(pseg[s - S, 11]) for s in bad if S <= s < S + P})
    return status


JPEG_SPLIT_CHUNK = 128    # the default chunk of a split scan, in bytes ("Split scans": the sweep)


def jpeg_decode_split(data, img, img_dev, seg, seg_dev, tables, pseg, pseg_dev, level_counts, pool, qsets, pixels, chunk_bytes=JPEG_SPLIT_CHUNK,
                      stages=7, check=True):
    """jpeg_decode_progressive with long baseline segments -- a restart-free scan is one -- decoded by a workgroup each, a lane per
    chunk of `chunk_bytes` bytes (a multiple of 8 in 8..65536; include/mgnns_jpeg_split.h, DESIGN.md 17 "Split scans").  The same
    arguments, validation, workspaces, status tensor and JpegDecodeError, and the same bytes in `pixels`: only the time differs.
    The progressive arguments may be empty (pseg [0,12], no levels, pool [0,n], qsets [0,192])."""
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, int) or chunk_bytes < 8 or chunk_bytes > 65536 or chunk_bytes % 8:
        raise ValueError("chunk_bytes must be a multiple of 8 in 8..65536, got %r" % (chunk_bytes,))
    return jpeg_decode_progressive(data, img, img_dev, seg, seg_dev, tables, pseg, pseg_dev, level_counts, pool, qsets, pixels, stages=stages,
                                   check=check, _split=chunk_bytes)


JPEG_LAYOUT_KIND = 3      # an image record of another component layout: kind 3, width, height, components | colour model << 8, h and v
#                           (a nibble per component), MCUs per row, MCU rows, quantisation / DC / AC table ids (a byte per component,
#                           four of them), table set, coefficient / plane / pixel offset, end of the padding
JPEG_COLOUR_MODELS = {0: "gray", 1: "YCbCr", 2: "RGB", 3: "CMYK", 4: "YCCK"}


def _jpeg_check_layouts(img, n_sets, refuse):
    """The image records of kind 3, checked on the host as the layout kernels check them.  -> (mask of kind 3, MCUs, blocks per image)"""
    kind, W, H, nm, hp, vp, mcux, mcuy, tq, td, ta, tset, coef_off, plane_off = (img[:, k] for k in range(14))
    lay = kind == 3
    nc, model = nm & 0xFF, nm >> 8
    refuse(lay & ((nm < 0) | ((nc != 1) & (nc != 3) & (nc != 4))), "a layout has 1, 3 or 4 components")
    refuse(lay & ~(((nc == 1) & (model == 0)) | ((nc == 3) & ((model == 1) | (model == 2))) | ((nc == 4) & ((model == 3) | (model == 4)))),
           "the colour model does not fit the components")
    refuse(lay & ((hp < 0) | (hp > 0xFFFF) | (vp < 0) | (vp > 0xFFFF)), "sampling factors are a nibble per component")
    h = torch.stack([(hp >> (4 * c)) & 15 for c in range(4)], 1)
    v = torch.stack([(vp >> (4 * c)) & 15 for c in range(4)], 1)
    has = torch.arange(4)[None, :] < nc[:, None]
    refuse(lay & ((has & ((h < 1) | (h > 4) | (v < 1) | (v > 4))) | (~has & ((h != 0) | (v != 0)))).any(1), "sampling factors outside 1..4")
    hmax, vmax = (h * has).max(1).values.clamp(min=1), (v * has).max(1).values.clamp(min=1)
    h1, v1 = torch.where(has, h, 1).clamp(min=1), torch.where(has, v, 1).clamp(min=1)
    refuse(lay & ((hmax[:, None] % h1 != 0) | (vmax[:, None] % v1 != 0)).any(1), "a sampling factor is no integral fraction of the largest")
    bpm = (h * v * has).sum(1)
    refuse(lay & ((bpm > 10) | ((nc == 1) & (bpm != 1))), "more than 10 blocks per MCU, or one component that is not 1 x 1")
    refuse(lay & ((mcux != (W + 8 * hmax - 1) // (8 * hmax)) | (mcuy != (H + 8 * vmax - 1) // (8 * vmax))), "MCU counts do not match the extent")
    refuse(lay & ((tset < 0) | (tset >= n_sets)), "table set outside 0..%d" % (n_sets - 1))
    refuse(lay & ((tq < 0) | (td < 0) | (ta < 0) | (((tq | td | ta) & ~0x03030303) != 0)), "table ids must be 0..3")
    refuse(lay & ((coef_off < 0) | (coef_off % 64 != 0) | (plane_off < 0) | (plane_off % 64 != 0)), "workspace offsets must be non-negative multiples of 64")
    lmcu = mcux * mcuy
    return lay, lmcu, lmcu * bpm * lay


def jpeg_decode_layouts(data, img, img_dev, seg, seg_dev, tables, pseg, pseg_dev, level_counts, pool, qsets, lseg, lseg_dev, pixels,
                        chunk_bytes=0, stages=7, check=True):
    """jpeg_decode_progressive (chunk_bytes = 0) or jpeg_decode_split for a batch that also holds files of other component layouts
    (include/mgnns_jpeg_layouts.h; DESIGN.md 17, "Other component layouts"): CMYK, YCCK, RGB, 4:4:0, 4:1:1 and every other
    interleaved layout of 1, 3 or 4 components.  Such an image is a record of kind 3 (JPEG_LAYOUT_KIND) and its segments are the
    rows of lseg [L,5] (host; lseg_dev its device copy), seg's layout; its tables lie in `tables`.  The launches for the other
    images are the same as without this entry point; three more follow for the images of kind 3, one lane per segment -- these
    segments are never split.  The same validation, workspaces and JpegDecodeError; -> the status tensor [S + P + L]."""
    if chunk_bytes and (isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, int) or chunk_bytes < 8 or chunk_bytes > 65536 or chunk_bytes % 8):
        raise ValueError("chunk_bytes must be 0 or a multiple of 8 in 8..65536, got %r" % (chunk_bytes,))
    return jpeg_decode_progressive(data, img, img_dev, seg, seg_dev, tables, pseg, pseg_dev, level_counts, pool, qsets, pixels, stages=stages,
                                   check=check, _split=int(chunk_bytes or 0), _layouts=(lseg, lseg_dev))


# ---- measurement aid: in-graph timestamps --------------------------------------------------------------------------
_timeline = None         # (slots tensor [uint64 as int64], names list) while tools/graph_timeline.py is recording


def timeline_begin(device, n=64):
    global _timeline
    _timeline = (torch.zeros(n, dtype=torch.int64, device=device), [])
    return _timeline


def timeline_end():
    global _timeline
    t, _timeline = _timeline, None
    return t


def stamp(name):
    """Record `name` at the current point of the current stream (no-op unless a timeline is being recorded)."""
    if _timeline is None:
        return
    slots, names = _timeline
    if len(names) >= slots.numel():
        raise RuntimeError("timeline full")
    names.append(name)
    _lib.call("mgnns_debug_stamp", _p(slots), len(names) - 1, _stream())


# ---- training mode of the fusion layers (csrc/mha_train.hip; fp32, GPU only) ----------------------------------------------
# dropout sites of the counter-based masks: (seed, site, element index) -> keep
DROP_ATTN, DROP_FC, DROP_FFN = 0, 1, 2
# the label Attention's probabilities, the classifier's dropout (model training)
DROP_LABEL_ATTN, DROP_HEAD = _C["MGNNS_DROP_LABEL_ATTN"], _C["MGNNS_DROP_HEAD"]
ELT_ADD, ELT_RELU_BWD, ELT_LRELU2_BWD = _C["MGNNS_ELT_ADD"], _C["MGNNS_ELT_RELU_BWD"], _C["MGNNS_ELT_LRELU2_BWD"]
TRAIN_MAX_L, TRAIN_MAX_D, TRAIN_MAX_H = 208, 320, 8


def _chk_rate(rate):
    rate = float(rate)
    if not 0.0 <= rate <= 1.0:
        raise ValueError("dropout rate %g outside [0, 1]" % rate)
    return rate


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def mha_attn_train(qh, bank, mask, n_head, d_kv, wk, wv, bv, seed, rate, return_masks=False):
    """Training forward of the single-query attention core (mgnns_mha_train_fwd): the folded attention of sq_mha_folded with
    dropout(rate) on the probabilities.  bank fp32 [B, L, D]; mask [B, L] (0 = masked) or None.
    -> (o [B, H*dk], attn [H*B, 1, L] after dropout, saved) (+ keep [H*B, 1, L] bool with return_masks); `saved` is what
    mha_attn_train_backward takes."""
    _chk(qh, "qh", ndim=2)
    _chk(bank, "memory bank", ndim=3)
    B, L_, D = bank.shape
    for n, t in (("w_ks.weight", wk), ("w_vs.weight", wv)):
        _chk(t, n, ndim=2)
    _chk(bv, "w_vs.bias", ndim=1)
    if qh.shape != (B, n_head * d_kv):
        raise ValueError("qh shape %s, expected %s" % (tuple(qh.shape), (B, n_head * d_kv)))
    if wk.shape != (n_head * d_kv, D) or wv.shape != (n_head * d_kv, D) or bv.shape != (n_head * d_kv,):
        raise ValueError("w_ks %s / w_vs %s / b_vs %s do not match H=%d d_kv=%d D=%d" % (tuple(wk.shape), tuple(wv.shape),
                                                                                        tuple(bv.shape), n_head, d_kv, D))
    if not (0 < L_ <= TRAIN_MAX_L and 0 < D <= TRAIN_MAX_D and D % 4 == 0 and 0 < n_head <= TRAIN_MAX_H and d_kv % 4 == 0):
        raise ValueError("training attention supports L <= %d, d_model <= %d (multiple of 4), n_head <= %d, d_kv %% 4 == 0; "
                         "got L=%d d_model=%d n_head=%d d_kv=%d" % (TRAIN_MAX_L, TRAIN_MAX_D, TRAIN_MAX_H, L_, D, n_head, d_kv))
    if mask is not None:
        _chk(mask, "mask", ndim=2)
        if mask.shape != (B, L_):
            raise ValueError("mask shape %s, expected %s" % (tuple(mask.shape), (B, L_)))
    rate = _chk_rate(rate)
    dev, f32 = qh.device, torch.float32
    U = torch.empty(n_head, B, D, device=dev, dtype=f32)
    P = torch.empty(n_head, B, L_, device=dev, dtype=f32)
    attn = torch.empty(n_head * B, 1, L_, device=dev, dtype=f32)
    keep = torch.empty(n_head * B, 1, L_, device=dev, dtype=torch.uint8)
    Z = torch.empty(n_head, B, D, device=dev, dtype=f32)
    SP = torch.empty(n_head, B, device=dev, dtype=f32)
    o = torch.empty(B, n_head * d_kv, device=dev, dtype=f32)
    _launch("mgnns_mha_train_fwd", _p(qh), _p(bank), _p(mask), B, L_, D, n_head, d_kv, _p(wk), _p(wv), _p(bv), _seed64(seed), rate, _p(U),
            _p(P), _p(attn), _p(keep), _p(Z), _p(SP), _p(o), _stream(), key=(L_,))
    saved = dict(U=U, P=P, attn=attn, keep=keep, Z=Z, SP=SP, rate=rate, n_head=n_head, d_kv=d_kv)
    if return_masks:
        return o, attn, saved, keep.bool()
    return o, attn, saved


def mha_attn_train_backward(dO, qh, bank, mask, wk, wv, bv, saved, want_dbank=True):
    """Backward of mha_attn_train (mgnns_mha_train_bwd): one streaming pass pair over the bank.
    -> (dqh [B, H*dk], dWk, dWv [H*dk, D], dbv [H*dk], dbank [B, L, D] or None).  b_k has no gradient (it drops out of the
    softmax)."""
    _chk(dO, "dO", ndim=2)
    _chk(bank, "memory bank", ndim=3)
    B, L_, D = bank.shape
    H, dk = saved["n_head"], saved["d_kv"]
    if dO.shape != (B, H * dk):
        raise ValueError("dO shape %s, expected %s" % (tuple(dO.shape), (B, H * dk)))
    dev, f32 = dO.device, torch.float32
    dqh = torch.empty(B, H * dk, device=dev, dtype=f32)
    dWk = torch.empty(H * dk, D, device=dev, dtype=f32)
    dWv = torch.empty(H * dk, D, device=dev, dtype=f32)
    dbv = torch.empty(H * dk, device=dev, dtype=f32)
    dbank = torch.empty(B, L_, D, device=dev, dtype=f32) if want_dbank else None
    L = _lib.lib()
    nbytes = L.mgnns_mha_train_bwd_workspace_bytes(B, D, H, dk)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    s = saved
    _launch("mgnns_mha_train_bwd", _p(dO), _p(qh), _p(bank), _p(mask), B, L_, D, H, dk, _p(wk), _p(wv), _p(bv), s["rate"], _p(s["U"]),
            _p(s["P"]), _p(s["attn"]), _p(s["keep"]), _p(s["Z"]), _p(s["SP"]), _p(dqh), _p(dWk), _p(dWv), _p(dbv), _p(dbank), _p(ws),
            nbytes, _stream(), key=(L_,))
    return dqh, dWk, dWv, dbv, dbank


def wgrad(dy, x, bias=True):
    """Weight gradient of y = x W^T + b: (dW = dy^T x [N, K], db = dy.sum(0) [N] or None); rows reduced in a fixed order."""
    _chk(dy, "dy", ndim=2)
    _chk(x, "x", ndim=2)
    if dy.shape[0] != x.shape[0]:
        raise ValueError("wgrad rows: dy %s, x %s" % (tuple(dy.shape), tuple(x.shape)))
    M, N = dy.shape
    K = x.shape[1]
    dW = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = torch.empty(N, device=dy.device, dtype=torch.float32) if bias else None
    L = _lib.lib()
    nbytes = L.mgnns_wgrad_workspace_bytes(M, N, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    _launch("mgnns_wgrad_fwd", _p(dy), M, N, _p(x), K, _p(dW), _p(db), _p(ws), nbytes, _stream(), key=(M, N, K))
    return dW, db


def dropout_residual_layernorm(x, res, gamma, beta, eps, seed, site, rate, return_masks=False):
    """y = LayerNorm(dropout(x) + res) with the reference's LayerNorm (unbiased std, eps added to the std), training mode
    (mgnns_drop_res_ln_fwd).  -> (y, saved) (+ keep bool [rows, D] with return_masks)."""
    D = x.shape[-1]
    x2 = _chk(x.reshape(-1, D), "x")
    r2 = _chk(res.reshape(-1, D), "residual")
    _chk(gamma, "gamma", ndim=1)
    _chk(beta, "beta", ndim=1)
    if r2.shape != x2.shape or gamma.shape != (D,) or beta.shape != (D,):
        raise ValueError("dropout_residual_layernorm: x %s, residual %s, gamma %s" % (tuple(x.shape), tuple(res.shape),
                                                                                     tuple(gamma.shape)))
    rate = _chk_rate(rate)
    rows = x2.shape[0]
    y = torch.empty_like(x2)
    xhat = torch.empty_like(x2)
    sig = torch.empty(rows, device=x.device, dtype=torch.float32)
    keep = torch.empty(rows, D, device=x.device, dtype=torch.uint8)
    _launch("mgnns_drop_res_ln_fwd", _p(x2), _p(r2), rows, D, _p(gamma), _p(beta), float(eps), _seed64(seed), int(site), rate, _p(y),
            _p(xhat), _p(sig), _p(keep), _stream(), key=(D,))
    saved = dict(xhat=xhat, sig=sig, keep=keep, rate=rate, eps=float(eps))
    y = y.view(x.shape)
    if return_masks:
        return y, saved, keep.bool()
    return y, saved


def dropout_residual_layernorm_backward(dy, gamma, saved, dy2=None):
    """Backward of dropout_residual_layernorm for dy (+ dy2): (d residual, d x, d gamma, d beta)."""
    xhat = saved["xhat"]
    rows, D = xhat.shape
    dy = _chk(dy.reshape(rows, D), "dy")
    if dy2 is not None:
        dy2 = _chk(dy2.reshape(rows, D), "dy2")
    dres = torch.empty_like(xhat)
    dx = torch.empty_like(xhat)
    dg = torch.empty(D, device=xhat.device, dtype=torch.float32)
    db = torch.empty(D, device=xhat.device, dtype=torch.float32)
    _launch("mgnns_drop_res_ln_bwd", _p(dy), _p(dy2), _p(xhat), _p(saved["sig"]), _p(saved["keep"]), rows, D, _p(gamma), saved["eps"],
            saved["rate"], _p(dres), _p(dx), _p(dg), _p(db), _stream(), key=(D,))
    return dres, dx, dg, db


def train_eltwise(op, a, b):
    """ELT_ADD: a + b;  ELT_RELU_BWD: a * (b > 0) (b = the ReLU's output);  ELT_LRELU2_BWD: b > 0 ? a : 0.2 a (b = the
    LeakyReLU(0.2)'s output or input)."""
    _chk(a, "a")
    _chk(b, "b")
    if a.shape != b.shape:
        raise ValueError("train_eltwise shapes %s / %s" % (tuple(a.shape), tuple(b.shape)))
    y = torch.empty_like(a)
    _launch("mgnns_train_eltwise", int(op), _p(a), _p(b), a.numel(), _p(y), _stream(), key=(op,))
    return y


# ---- training mode of the model around the fusion stacks (csrc/model_train.hip) -----------------------------------------
def imgbank_wgrad(feat, dbank, split=False):
    """Weight gradient of an image memory bank bank[b,p,:] = W feat[b,:,p] + c (mgnns_imgbank_wgrad): feat [B, K, P] in its
    native layout, dbank [B, P, N] -> (dW [N, K], db [N]).  Exact-f32 MFMA, samples reduced in a fixed order.  split: the
    split-bf16 kernel (mgnns_imgbank_wgrad_split: three bf16 MFMAs per product, fp32-class, same contract)."""
    _chk(feat, "feature map", ndim=3)
    _chk(dbank, "dbank", ndim=3)
    B, K, P = feat.shape
    N = dbank.shape[2]
    if tuple(dbank.shape[:2]) != (B, P):
        raise ValueError("dbank %s does not match the feature map %s" % (tuple(dbank.shape), tuple(feat.shape)))
    dW = torch.empty(N, K, device=feat.device, dtype=torch.float32)
    db = torch.empty(N, device=feat.device, dtype=torch.float32)
    L = _lib.lib()
    name = "mgnns_imgbank_wgrad_split" if split else "mgnns_imgbank_wgrad"
    nbytes = getattr(L, name + "_workspace_bytes")(B, K, P, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=feat.device)
    _launch(name, _p(feat), _p(dbank), B, K, P, N, _p(dW), _p(db), _p(ws), nbytes, _stream(), key=(B, P))
    return dW, db


def map_argmax(feat):
    """arg [B, K] (int32) = the first p at which each row feat[b, k, :] of a feature map [B, K, P] attains its maximum
    (mgnns_map_argmax): where the max-pool's gradient goes, ties to the smallest index as in torch's max_pool2d backward."""
    _chk(feat, "feature map", ndim=3)
    B, K, P = feat.shape
    if K <= 0 or P <= 0:
        raise ValueError("feature map %s: need K, P > 0" % (tuple(feat.shape),))
    arg = torch.empty(B, K, device=feat.device, dtype=torch.int32)
    _launch("mgnns_map_argmax", _p(feat), B, K, P, _p(arg), _stream(), key=(B, P))
    return arg


def imgbank_dgrad(dbank, weight, dpooled=None, arg=None, positions=None, out=None, split=False):
    """Gradient with respect to the feature map of an image memory bank and its max-pool (mgnns_imgbank_dgrad):
    dX[b,k,p] = sum_o weight[o,k] dbank[b,p,o] + (p == arg[b,k]) dpooled[b,k] -> dX [B, K, P].  dbank [B, P, N], or None for the
    pooled term alone (then `positions` = P); weight [N, K] (the nn.Linear's); dpooled [B, K] with arg [B, K] int32 (map_argmax),
    or both None; out: a [B, K, P] tensor to write instead of a new one.  Exact-f32 MFMA, bit-identical from call to call.
    split: the split-bf16 kernel (mgnns_imgbank_dgrad_split: three bf16 MFMAs per product, fp32-class, same contract; the
    pooled term alone has no product and runs today's kernel)."""
    _chk(weight, "weight", ndim=2)
    N, K = weight.shape
    if (dpooled is None) != (arg is None):
        raise ValueError("imgbank_dgrad: dpooled and arg come together")
    if dpooled is not None:
        _chk(dpooled, "dpooled", ndim=2)
        _chk(arg, "arg", dtype=torch.int32, ndim=2)
        if dpooled.shape[1] != K or arg.shape != dpooled.shape:
            raise ValueError("dpooled %s / arg %s do not match weight %s" % (tuple(dpooled.shape), tuple(arg.shape),
                                                                             tuple(weight.shape)))
    if dbank is not None:
        _chk(dbank, "dbank", ndim=3)
        B, P = dbank.shape[:2]
        if dbank.shape[2] != N or (dpooled is not None and dpooled.shape[0] != B) or positions not in (None, P):
            raise ValueError("dbank %s does not match weight %s, dpooled %s, positions %s"
                             % (tuple(dbank.shape), tuple(weight.shape), None if dpooled is None else tuple(dpooled.shape), positions))
    elif dpooled is None or positions is None:
        raise ValueError("imgbank_dgrad: without dbank, dpooled / arg and positions (= P) are needed")
    else:
        B, P = dpooled.shape[0], int(positions)
    if P <= 0 or K <= 0 or N <= 0:
        raise ValueError("imgbank_dgrad: need K, P, N > 0 (K=%d P=%d N=%d)" % (K, P, N))
    if out is None:
        dX = torch.empty(B, K, P, device=weight.device, dtype=torch.float32)
    else:
        dX = _chk(out, "out", ndim=3)
        if tuple(dX.shape) != (B, K, P):
            raise ValueError("out %s is not [%d, %d, %d]" % (tuple(dX.shape), B, K, P))
    L = _lib.lib()
    if split and dbank is not None:
        nbytes = L.mgnns_imgbank_dgrad_split_workspace_bytes(B, K, P, N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
        _launch("mgnns_imgbank_dgrad_split", _p(dbank), _p(weight), _p(dpooled), _p(arg), B, K, P, N, _p(dX), _p(ws), nbytes, _stream(),
                key=(B, P))
        return dX
    _launch("mgnns_imgbank_dgrad", _p(dbank), _p(weight), _p(dpooled), _p(arg), B, K, P, N, _p(dX), _stream(), key=(B, P))
    return dX


def label_attn_train(Q, K, V, n_heads, seed, rate, return_masks=False):
    """Training forward of the label attention between its projections (mgnns_label_attn_train_fwd, MODEL:101-131): Q [NLQ,hid],
    K = V's source projections [B, hid] -> (x [B, NLQ, hid] with dropout(rate) on softmax(energy) over each head's dh axis,
    saved) (+ keep [B, NLQ, hid] bool with return_masks)."""
    _chk(Q, "Q", ndim=2)
    _chk(K, "K", ndim=2)
    _chk(V, "V", ndim=2)
    NLQ, hid = Q.shape
    B = K.shape[0]
    if K.shape[1] != hid or V.shape != K.shape or hid % n_heads:
        raise ValueError("label attention shapes Q%s K%s V%s" % (tuple(Q.shape), tuple(K.shape), tuple(V.shape)))
    dh = hid // n_heads
    if dh > 64:
        raise ValueError("training label attention supports head widths up to 64, got %d" % dh)
    rate = _chk_rate(rate)
    x = torch.empty(B, NLQ, hid, device=K.device, dtype=torch.float32)
    P = torch.empty_like(x)
    keep = torch.empty(B, NLQ, hid, device=K.device, dtype=torch.uint8)
    _launch("mgnns_label_attn_train_fwd", _p(Q), _p(K), _p(V), B, NLQ, n_heads, dh, _seed64(seed), rate, _p(x), _p(P), _p(keep), _stream())
    saved = dict(P=P, keep=keep, rate=rate, n_heads=n_heads)
    if return_masks:
        return x, saved, keep.bool()
    return x, saved


def label_attn_train_backward(dx, Q, K, V, saved):
    """Backward of label_attn_train: dx [B, NLQ, hid] -> (dQ [NLQ, hid] summed over the batch in order, dK, dV [B, hid])."""
    NLQ, hid = Q.shape
    B = K.shape[0]
    dx = _chk(dx.reshape(B, NLQ, hid), "dx")
    H = saved["n_heads"]
    dQ = torch.empty(NLQ, hid, device=K.device, dtype=torch.float32)
    dK = torch.empty(B, hid, device=K.device, dtype=torch.float32)
    dV = torch.empty(B, hid, device=K.device, dtype=torch.float32)
    L = _lib.lib()
    nbytes = L.mgnns_label_attn_train_bwd_workspace_bytes(B, NLQ, H, hid // H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=K.device)
    _launch("mgnns_label_attn_train_bwd", _p(dx), _p(Q), _p(K), _p(V), _p(saved["P"]), _p(saved["keep"]), B, NLQ, H, hid // H,
            saved["rate"], _p(dQ), _p(dK), _p(dV), _p(ws), nbytes, _stream())
    return dQ, dK, dV


def dropout(x, seed, site, rate, return_masks=False):
    """Training-mode dropout at `site` (mgnns_dropout_fwd) -> (y, keep bytes) (+ keep bool with return_masks)."""
    _chk(x, "x")
    rate = _chk_rate(rate)
    y = torch.empty_like(x)
    keep = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    _launch("mgnns_dropout_fwd", _p(x), x.numel(), _seed64(seed), int(site), rate, _p(y), _p(keep), _stream())
    if return_masks:
        return y, keep, keep.bool()
    return y, keep


def dropout_backward(dy, keep, rate):
    """dx = dy keep / (1 - rate) (mgnns_dropout_bwd)."""
    _chk(dy, "dy")
    _chk(keep, "keep", torch.uint8)
    if dy.shape != keep.shape:
        raise ValueError("dropout_backward shapes %s / %s" % (tuple(dy.shape), tuple(keep.shape)))
    dx = torch.empty_like(dy)
    _launch("mgnns_dropout_bwd", _p(dy), _p(keep), dy.numel(), _chk_rate(rate), _p(dx), _stream())
    return dx


def dropout_mask(seed, site, rate, shape, device):
    """The keep mask (bool, `shape`) the training kernels draw for `seed` at `site` over a tensor of that shape (mgnns_dropout_mask):
    how tests and tools rebuild a training forward's dropout from the seeds the modules keep (`last_dropout_seed`).  Sites index
    their tensors flat: DROP_ATTN [H*B, 1, L], DROP_FC / DROP_FFN [B, D], DROP_LABEL_ATTN [B, NLQ, hid], DROP_HEAD [B, D]."""
    keep = torch.empty(tuple(shape), device=device, dtype=torch.uint8)
    _launch("mgnns_dropout_mask", _seed64(seed), int(site), _chk_rate(rate), keep.numel(), _p(keep), _stream())
    return keep.bool()


# ---- training mode of the text encoders (csrc/text_train.hip; fp32, GPU only) ---------------------------------------------
# the BiLSTM's inter-layer dropout [B, T, 2H], the text GCN's dropout [B, D]
DROP_LSTM, DROP_TEXT_GCN = _C["MGNNS_DROP_LSTM"], _C["MGNNS_DROP_TEXT_GCN"]


def bilstm_train(tok, lens, emb_table, weights, hidden, num_layers, seed, rate):
    """Training forward of the text bank (mgnns_bilstm_train_fwd): bilstm(recurrence="f32") with dropout(rate) at DROP_LSTM on layer
    0's output before layer 1 (bit for bit the eval bank at rate 0) -> (bank [B, T, 2*hidden], saved for bilstm_train_backward)."""
    import ctypes
    _chk(tok, "text", torch.int64, 2)
    _chk(lens, "text_lens", torch.int64, 1)
    _chk(emb_table, "embedding.weight", ndim=2)
    B, T = tok.shape
    if lens.shape[0] != B:
        raise ValueError("text_lens has %d entries for batch %d" % (lens.shape[0], B))
    if len(weights) != 2 * num_layers:
        raise ValueError("need %d (layer, direction) weight tuples" % (2 * num_layers))
    for t in (w for tup in weights for w in tup):
        _chk(t, "lstm weight")
    rate = _chk_rate(rate)
    dev = tok.device
    rows = max(int(lens.clamp(0, T).sum().item()), 1)      # packed rows (one sync: the saved tensors are sized by it)
    cat = _lstm_cat(weights, num_layers, None)
    arr = lambda ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    G = 4 * hidden
    meta = torch.empty(B + 1 + B + 8 + 2 * B * T, dtype=torch.int32, device=dev)
    gates = torch.empty(num_layers, 2, rows, G, device=dev, dtype=torch.float32)
    cells = torch.empty(num_layers, 2, rows, hidden, device=dev, dtype=torch.float32)
    mid = torch.empty(B, T, 2 * hidden, device=dev, dtype=torch.float32) if num_layers > 1 else None
    mid_d = torch.empty_like(mid) if num_layers > 1 else None
    out = torch.empty(B, T, 2 * hidden, device=dev, dtype=torch.float32)
    L = _lib.lib()
    nbytes = L.mgnns_bilstm_train_workspace_bytes(B, T, hidden)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    _launch("mgnns_bilstm_train_fwd", _p(tok), _p(lens), B, T, _p(emb_table), emb_table.shape[0], emb_table.shape[1], hidden, num_layers,
            arr([c[0].data_ptr() for c in cat]), arr([c[1].data_ptr() for c in cat]), arr([w[1].data_ptr() for w in weights]),
            arr([w[3].data_ptr() for w in weights]), _seed64(seed), rate, _p(meta), rows, _p(gates), _p(cells), _p(mid), _p(mid_d), _p(out),
            _p(ws), ws.numel(), _stream())
    saved = dict(tok=tok, lens=lens, B=B, T=T, rows=rows, n_rows=int(lens.clamp(0, T).sum().item()), hidden=hidden,
                 num_layers=num_layers, seed=seed, rate=rate, meta=meta, gates=gates, cells=cells, mid=mid, mid_d=mid_d, out=out,
                 cat=cat)
    return out, saved


def _bilstm_meta(s):
    B, T = s["B"], s["T"]
    m = s["meta"]
    return m[B + 1 + B + 8: B + 1 + B + 8 + B * T], m[B + 1 + B + 8 + B * T:]      # pack_tok, pack_pos


def gather_rows(src, idx, M):
    """dst [M, K] = src[idx[:M]] (mgnns_gather_rows; idx int32)."""
    _chk(src, "src", ndim=2)
    _chk(idx, "idx", torch.int32)
    dst = torch.empty(M, src.shape[1], device=src.device, dtype=torch.float32)
    _launch("mgnns_gather_rows", _p(src), src.shape[0], src.shape[1], _p(idx), M, _p(dst), _stream())
    return dst


def keyed_row_sum(keys, values, n_out, skip_below=0):
    """out [n_out, D] (zeros where no key lands) = for every key k, the sum of the rows values[r] with keys[r] == k, added in the
    order of a stable sort of the keys (mgnns_keyed_row_sum): the same inputs give bit-identical sums.  keys < skip_below add nothing
    (the embedding's padding row, -1 for empty slots)."""
    values = _chk(values.reshape(values.shape[0], -1), "values")
    keys = keys.reshape(-1).long()
    if keys.shape[0] != values.shape[0]:
        raise ValueError("keyed_row_sum: %d keys for %d rows" % (keys.shape[0], values.shape[0]))
    D = values.shape[1]
    out = torch.zeros(n_out, D, device=values.device, dtype=torch.float32)
    if keys.numel() == 0:
        return out
    sk, perm = torch.sort(keys, stable=True)
    _launch("mgnns_keyed_row_sum", _p(sk.contiguous()), _p(perm.contiguous()), keys.numel(), _p(values), D, values.shape[0],
            int(skip_below), _p(out), n_out, _stream())
    return out


def bilstm_train_backward(dout, saved, weights, emb_table, need_emb=True):
    """Backward of bilstm_train from dbank [B, T, 2H] -> (d embedding.weight [V, E] or None (row 0 stays 0), [per (layer, direction):
    (dW_ih, dW_hh, db_ih, db_hh)]).  Recurrences on the GPU (mgnns_bilstm_train_bwd_rec); weight gradients through wgrad (fixed-order
    reductions), input gradients as one GEMM per layer; layer 1's input gradient goes back through the DROP_LSTM mask."""
    s = saved
    B, T, H, nl, M = s["B"], s["T"], s["hidden"], s["num_layers"], s["n_rows"]
    G = 4 * H
    pack_tok, pack_pos = _bilstm_meta(s)
    grads = [None] * (2 * nl)
    demb = torch.zeros_like(emb_table) if need_emb else None
    if M == 0:
        for li in range(2 * nl):
            grads[li] = tuple(torch.zeros_like(w) for w in weights[li])
        return demb, grads
    dcur = _chk(dout.contiguous(), "dbank")
    for layer in range(nl - 1, -1, -1):
        dz = torch.empty(M, 2 * G, device=dout.device, dtype=torch.float32)
        _launch("mgnns_bilstm_train_bwd_rec", _p(dcur), _p(s["lens"]), B, T, _p(s["meta"]), s["rows"], _p(s["gates"][layer]),
                _p(s["cells"][layer]), _p(weights[2 * layer][1]), _p(weights[2 * layer + 1][1]), _p(dz), _stream())
        hout = s["out"] if layer == nl - 1 else s["mid"]
        hprev = torch.empty(M, 2 * H, device=dout.device, dtype=torch.float32)
        _launch("mgnns_bilstm_train_hprev", _p(hout), _p(s["lens"]), B, T, _p(s["meta"]), M, _p(hprev), _stream())
        x = gather_rows(emb_table, pack_tok, M) if layer == 0 else gather_rows(s["mid_d"].view(B * T, 2 * H), pack_pos, M)
        dwih, dbih = wgrad(dz, x)
        dwhh = wgrad(dz, hprev, bias=False)[0]
        for d in (0, 1):
            db = dbih[d * G:(d + 1) * G]
            grads[2 * layer + d] = (dwih[d * G:(d + 1) * G].contiguous(), dwhh[d * G:(d + 1) * G, d * H:(d + 1) * H].contiguous(),
                                    db.contiguous(), db.clone())
        if layer > 0:
            dx = matmul(dz, s["cat"][layer][0])
            dprev = torch.zeros(B, T, 2 * H, device=dout.device, dtype=torch.float32)
            _launch("mgnns_bilstm_train_unpack_drop", _p(dx), _p(pack_pos), M, B, T, _seed64(s["seed"]), s["rate"], _p(dprev), _stream())
            dcur = dprev
        elif need_emb:
            dx = matmul(dz, s["cat"][0][0])
            demb = keyed_row_sum(pack_tok[:M], dx, emb_table.shape[0], skip_below=1)
    return demb, grads


def textgcn_train(tok, node_hidden, edge_w, pmi_dev, ngram, max_length, seed, rate):
    """Training forward of the text GCN (mgnns_textgcn_train_fwd): relu(dropout(sum over nodes of the max-aggregated states)) with
    dropout(rate) at DROP_TEXT_GCN -> (out [B, D], saved for textgcn_train_backward)."""
    _chk(tok, "doc_ids", torch.int64, 2)
    _chk(node_hidden, "node_hidden.weight", ndim=2)
    ew = _chk(edge_w.reshape(-1), "seq_edge_w.weight")
    rp, col, eid = pmi_dev
    B, T = tok.shape
    V, D = node_hidden.shape
    if rp.shape[0] != V + 1:
        raise ValueError("PMI map has %d rows, vocabulary has %d" % (rp.shape[0] - 1, V))
    rate = _chk_rate(rate)
    Tm = min(T, int(max_length))
    out = torch.empty(B, D, device=tok.device, dtype=torch.float32)
    presum = torch.empty(B, D, device=tok.device, dtype=torch.float32)
    win = torch.empty(B, Tm, D, device=tok.device, dtype=torch.int16)
    if B:
        _launch("mgnns_textgcn_train_fwd", _p(tok), B, T, _p(node_hidden), V, D, _p(ew), ew.shape[0], _p(rp), _p(col), _p(eid), int(ngram),
                int(max_length), _seed64(seed), rate, _p(out), _p(presum), _p(win), _stream())
    return out, dict(presum=presum, win=win, seed=seed, rate=rate, ngram=int(ngram), max_length=int(max_length))


def textgcn_train_backward(dy, tok, node_hidden, edge_w, pmi_dev, saved, need_nodes=True, need_edges=True):
    """Backward of textgcn_train from dy [B, D] -> (d node_hidden [V, D] or None, d edge weights [n_edge_w] or None): each (node,
    feature) sends its gradient through its winning in-edge (the tie rule of textgcn_train); per-document partials summed per key by
    keyed_row_sum."""
    rp, col, eid = pmi_dev
    ew = edge_w.reshape(-1)
    B, T = tok.shape
    V, D = node_hidden.shape
    g = saved["ngram"]
    Tm, W = min(T, saved["max_length"]), 2 * saved["ngram"] + 1
    dn = torch.zeros(V, D, device=tok.device, dtype=torch.float32) if need_nodes else None
    de = torch.zeros(ew.shape[0], device=tok.device, dtype=torch.float32) if need_edges else None
    if B == 0:
        return dn, de
    dy = _chk(dy.contiguous(), "dy")
    R = torch.empty(B, Tm, D, device=tok.device, dtype=torch.float32)
    keyR = torch.empty(B, Tm, device=tok.device, dtype=torch.int32)
    Eg = torch.empty(B, Tm, W, device=tok.device, dtype=torch.float32)
    keyE = torch.empty(B, Tm, W, device=tok.device, dtype=torch.int32)
    _launch("mgnns_textgcn_train_bwd", _p(tok), B, T, _p(node_hidden), V, D, _p(ew), ew.shape[0], _p(rp), _p(col), _p(eid), g,
            saved["max_length"], _seed64(saved["seed"]), saved["rate"], _p(dy), _p(saved["presum"]), _p(saved["win"]), _p(R), _p(keyR),
            _p(Eg), _p(keyE), _stream())
    if need_nodes:
        dn = keyed_row_sum(keyR, R.view(B * Tm, D), V)
    if need_edges:
        de = keyed_row_sum(keyE, Eg.view(-1, 1), ew.shape[0]).view(-1)
    return dn, de


# ---- the tail of a training step: loss, gradient norm, Adam (include/mgnns_step.h, csrc/step_tail.hip) --------
_SC = _lib.STEP_CONSTANTS
STEP_CHUNK = _SC["MGNNS_STEP_CHUNK"]                 # elements of one chunk at most
STEP_CHUNK_WORDS = 5                                 # a chunk record as int64 words: p, g, m, v, n | group << 32
STEP_GROUP_FLOATS = _SC["MGNNS_STEP_GROUP_FLOATS"]   # -(lr / bc1), sqrt(bc2), 1 - b1, b2, 1 - b2, eps, wd, unused
CE_MAX_NL = _SC["MGNNS_CE_MAX_NL"]
CE_IGNORE_INDEX = -100


def ce_loss(logits, target):
    """mgnns_ce_loss_fwd_bwd: (loss 0-d fp32, dlogits [B, NL] fp32) of the mean cross-entropy over the rows whose target is not
    -100, in fp64 inside the kernel and rounded once; dlogits = (softmax - onehot) / n_live.  Any other target outside [0, NL)
    gives a NaN loss and a NaN row (nothing outside the row is touched)."""
    _chk(logits, "logits", ndim=2)
    _chk(target, "target", torch.int64, 1)
    B, NL = logits.shape
    if target.shape[0] != B or target.device != logits.device:
        raise ValueError("target must be [%d] on %s, got %s on %s" % (B, logits.device, tuple(target.shape), target.device))
    if B < 1 or not 1 <= NL <= CE_MAX_NL:
        raise ValueError("ce_loss takes B >= 1 and 1 <= NL <= %d, got logits %s" % (CE_MAX_NL, tuple(logits.shape)))
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits)
    _launch("mgnns_ce_loss_fwd_bwd", _p(logits), _p(target), B, NL, _p(loss), _p(dlogits), _stream())
    return loss, dlogits


def _chk_chunks(chunks, n_chunks):
    _chk(chunks, "chunk table", torch.int64, 2)
    if chunks.shape[1] != STEP_CHUNK_WORDS or not 0 <= n_chunks <= chunks.shape[0]:
        raise ValueError("chunk table must be [>= %d, %d] int64, got %s" % (n_chunks, STEP_CHUNK_WORDS, tuple(chunks.shape)))
    return int(n_chunks)


def grad_sumsq(chunks, n_chunks, partial):
    """mgnns_grad_sumsq: partial[c] = the fp64 sum of g * g over chunk c of the table (mgnns_amd/optim.py builds it)."""
    n = _chk_chunks(chunks, n_chunks)
    _chk(partial, "partial", torch.float64, 1)
    if partial.shape[0] < n or partial.device != chunks.device:
        raise ValueError("partial must hold %d fp64 on %s" % (n, chunks.device))
    _launch("mgnns_grad_sumsq", _p(chunks), n, _p(partial), _stream())
    return partial


def grad_clip_coef(partial, n_chunks, max_norm, out):
    """mgnns_grad_clip_coef: out[0] = total_norm = (float)sqrt(sum of the partials), out[1] = min(1, max_norm / (total_norm + 1e-6))."""
    _chk(partial, "partial", torch.float64, 1)
    _chk(out, "out", ndim=1)
    max_norm = float(max_norm)
    if not 0 <= n_chunks <= partial.shape[0] or out.shape[0] < 2 or out.device != partial.device:
        raise ValueError("grad_clip_coef: %d partials of %d, out %s" % (n_chunks, partial.shape[0], tuple(out.shape)))
    if not max_norm >= 0.0:
        raise ValueError("max_norm=%r must be a number >= 0" % max_norm)
    _launch("mgnns_grad_clip_coef", _p(partial), int(n_chunks), max_norm, _p(out), _stream())
    return out


def adam_step(chunks, n_chunks, groups, clip_coef):
    """mgnns_adam_step: one fused Adam pass over the chunk table with the per-group scalar rows `groups` [R, STEP_GROUP_FLOATS] and
    the gradient coefficient clip_coef (a 1-element fp32 tensor on the device); a run of row -1 only has its gradient multiplied
    by the coefficient in place.  Writes p, exp_avg and exp_avg_sq through their addresses: the caller bumps the parameters'
    versions (optim.Adam.step does)."""
    n = _chk_chunks(chunks, n_chunks)
    _chk(groups, "groups", ndim=2)
    _chk(clip_coef, "clip_coef")
    if groups.shape[1] != STEP_GROUP_FLOATS or groups.shape[0] < 1 or clip_coef.numel() < 1:
        raise ValueError("groups must be [R >= 1, %d] and clip_coef hold one element, got %s and %s"
                         % (STEP_GROUP_FLOATS, tuple(groups.shape), tuple(clip_coef.shape)))
    if groups.device != chunks.device or clip_coef.device != chunks.device:
        raise ValueError("the chunk table, the scalar rows and clip_coef must be on one device")
    _launch("mgnns_adam_step", _p(chunks), n, _p(groups), groups.shape[0], _p(clip_coef), _stream())
