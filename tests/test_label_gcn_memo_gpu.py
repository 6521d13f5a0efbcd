"""The label GCN's device-side memo (csrc/label_gcn.hip: label_gcn_memo_check + the hit word label_gcn_kernel reads at entry;
ops.label_gcn(memo=...); model.label_gcn_memo).  Everything here is bit-for-bit: a hit returns the bits the miss wrote, a miss
writes the bits the launch without a memo writes.  Shapes: C in {17, 80} label classes (one partial 16-row tile + one row / five
full tiles), K0 = 300, the model's widths 1024 / 2048, a grid of 8 workgroups and the default grid."""
import numpy as np
import pytest
import torch

from mgnns_amd import ops, synth
from tests import helpers as H
from tests.model_util import build_model, call_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K0, N1, N2 = 300, 1024, 2048


def dev(x):
    return torch.as_tensor(x).to(DEV).contiguous()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """Bit equality of two (G, (Gp_hi, Gp_lo), Q) results (integers: a NaN must be able to equal itself)."""
    return (torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
            and torch.equal(bits(a[2]), bits(b[2])))


def keep(r):
    """A memo launch returns the memo's own buffers: copy them before the next launch may rewrite them."""
    return r[0].clone(), (r[1][0].clone(), r[1][1].clone()), r[2].clone()


@pytest.fixture(scope="module")
def packs():
    p = H.params_for({"gc1.weight": (K0, N1), "gc2.weight": (N1, N2)})
    w1, w2 = dev(p["gc1.weight"]), dev(p["gc2.weight"])
    rs = np.random.RandomState(11)
    query = (dev(rs.standard_normal((7, K0)).astype(np.float32)), dev((0.05 * rs.standard_normal((300, K0))).astype(np.float32)),
             dev(rs.standard_normal(300).astype(np.float32)))
    return {False: ops.label_gcn_pack(w1, w2, split=False), True: ops.label_gcn_pack(w1, w2, split=True), "query": query}


def case(C):
    rs = np.random.RandomState(100 + C)
    A = ((rs.rand(C, C) < 0.2) * rs.rand(C, C) + np.eye(C)).astype(np.float32)
    return dev(A), dev(rs.standard_normal((C, K0)).astype(np.float32))


class Launcher:
    def __init__(self, packs, split, A, grid):
        self.pack, self.query, self.A, self.grid, self.memo = packs[split], packs["query"], A, grid, {}

    def on(self, X):
        r = ops.label_gcn(self.A, X, self.pack, want_packed_g=True, query=self.query, grid=self.grid, memo=self.memo)
        return keep(r), ops.label_gcn_memo_flag(self.memo, want_packed_g=True)

    def off(self, X):
        return keep(ops.label_gcn(self.A, X, self.pack, want_packed_g=True, query=self.query, grid=self.grid))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("grid", [8, 0])
@pytest.mark.parametrize("C", [17, 80])
def test_hit_is_exact_and_miss_is_not_stale(packs, C, grid, split):
    A, X = case(C)
    L = Launcher(packs, split, A, grid)
    want = L.off(X)
    first, flag = L.on(X)
    assert flag == 0 and same(first, want)                       # the first launch computes: what the launch without a memo writes
    for _ in range(2):
        again, flag = L.on(X)
        assert flag == 1 and same(again, first) and same(again, want)
    # one changed element, the very first and the very last of the table: a miss, the outputs of the changed table; restored: the original
    for r, c in ((0, 0), (C - 1, K0 - 1)):
        X2 = X.clone()
        X2[r, c] += 0.5
        got, flag = L.on(X2)
        assert flag == 0 and same(got, L.off(X2)) and not same(got, first), (r, c)
        got, flag = L.on(X2)
        assert flag == 1 and same(got, L.off(X2)), (r, c)
        back, flag = L.on(X)
        assert flag == 0 and same(back, first), (r, c)
    # the queue counters of the scratch are re-armed by hits and misses alike, the check launch's arrival word too
    assert all(int(ws[:256].view(torch.int32).abs().sum()) == 0 for ws in L.pack["_scratch"].values())
    assert all(int(st["state"][:256].view(torch.int32)[2]) == 0 for st in L.memo.values())


@pytest.mark.parametrize("grid", [8, 0])
@pytest.mark.parametrize("C", [17, 80])
def test_the_compare_is_bitwise(packs, C, grid):
    """A NaN in the table hits (compared as integers), +0 against -0 misses."""
    A, X = case(C)
    L = Launcher(packs, True, A, grid)
    Xn = X.clone()
    Xn[C // 2, 7] = float("nan")
    first, flag = L.on(Xn)
    assert flag == 0 and same(first, L.off(Xn)) and bool(torch.isnan(first[0]).any())
    again, flag = L.on(Xn)
    assert flag == 1 and same(again, first)
    Xz = X.clone()
    Xz[C - 1, 0] = 0.0
    pos, flag = L.on(Xz)
    assert flag == 0
    assert L.on(Xz)[1] == 1
    Xz[C - 1, 0] = -0.0
    neg, flag = L.on(Xz)
    assert flag == 0 and same(neg, L.off(Xz))
    assert L.on(Xz)[1] == 1


# ---- the model: weights keyed on the host, replayed graphs, two forwards in flight, the switch ------------------------------------
@pytest.fixture(scope="module")
def small():
    cfg = synth.CONFIGS["tumemo_b64"]
    adj = H.load_golden("adjacency.npz")
    lq = H.load_golden("label_attention.npz")["label_query"]
    pmi, count = synth.synth_pmi(cfg.V, seed=91)
    model = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], lq, DEV)
    model.set_precision("bf16")
    args = list(call_args(synth.make_inputs(cfg, B=8, seed=5, pmi=pmi), DEV))
    args[1] = args[1].to(DEV)
    return model, args


def eager_off(model, args):
    model.label_gcn_memo = False
    try:
        with torch.no_grad():
            return model(*args).clone()
    finally:
        model.label_gcn_memo = True


def with_inp(args, k, scale):
    a = list(args)
    a[k] = (a[k] * scale).contiguous()
    return a


def test_a_weight_edit_recomputes_in_eager_mode(small):
    model, args = small
    assert model.label_gcn_memo is True
    with torch.no_grad():
        before = model(*args).clone()
        assert torch.equal(model(*args), before) and torch.equal(before, eager_off(model, args))
        for name in ("gc1.weight", "object_A", "place_attention.w_q.weight"):
            w = model.get_parameter(name)
            old = w.detach().clone()
            w.mul_(1.0 + 2.0 ** -6)                                # in place: the version moves, the address does not
            got = model(*args).clone()
            assert torch.equal(got, eager_off(model, args)) and not torch.equal(got, before), name
            w.copy_(old)
            assert torch.equal(model(*args), before), name


def test_replay_follows_copy_inputs(small):
    from mgnns_amd.graph import GraphedForward
    model, args = small
    mod = with_inp(args, 5, 0.5)
    ref, ref_mod = eager_off(model, args), eager_off(model, mod)
    assert not torch.equal(ref, ref_mod)
    gf = GraphedForward(model, args)
    first = gf.replay().clone()
    assert torch.equal(first, ref)
    gf.copy_inputs(*mod)
    assert torch.equal(gf.replay(), ref_mod)                       # (the existing graph == eager test's tolerance: none)
    assert torch.equal(gf.replay(), ref_mod)
    gf.copy_inputs(*args)
    assert torch.equal(gf.replay(), first)


def test_two_forwards_in_flight_keep_their_own_memo(small):
    from mgnns_amd.graph import GraphedPipeline
    model, args = small
    sets = [args, with_inp(args, 6, 0.5), with_inp(args, 6, 1.25)]
    refs = [eager_off(model, a) for a in sets]
    assert not torch.equal(refs[0], refs[1]) and not torch.equal(refs[1], refs[2])
    pipe = GraphedPipeline(model, args, depth=2)
    order = [0, 1, 2, 2, 1, 1, 0, 2]                                # consecutive replays differ, repeat, and revisit an instance's last table
    pending = []
    for k in order:
        it = pipe.replay(pipe.copy_inputs(*sets[k]))
        pending.append((it, k))
        if len(pending) >= 2:
            old, ko = pending[-2]
            old.wait()
            assert torch.equal(old.static_out, refs[ko]), ko
    pipe.wait()
    torch.cuda.synchronize()
    assert torch.equal(pending[-1][0].static_out, refs[order[-1]])


def test_the_switch_turns_the_memo_off(small, monkeypatch):
    """label_gcn_memo = False: the same call into the same launch with no memo buffers, the same logits bit for bit."""
    model, args = small
    seen = []
    real = ops.label_gcn

    def spy(*a, **kw):
        seen.append(kw.get("memo"))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "label_gcn", spy)
    with torch.no_grad():
        on = model(*args).clone()
    assert len(seen) == 2 and all(isinstance(m, dict) for m in seen)
    del seen[:]
    for k in [k for k in model._wt_cache if isinstance(k, tuple) and k[0] == "lgcn_memo"]:
        del model._wt_cache[k]
    off = eager_off(model, args)
    assert seen == [None, None] and not any(isinstance(k, tuple) and k[0] == "lgcn_memo" for k in model._wt_cache)
    assert torch.equal(on, off)
