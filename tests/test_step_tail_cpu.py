"""Host side of the training step's tail (mgnns_amd/optim.py, include/mgnns_step.h): how far the
specification (tests/step_tail_ref.py) is from torch's own Adam, the chunk-table builder, the binding, the interchange of state
with torch.optim.Adam and the refusals.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mgnns_amd import _lib, ops, optim
from tests import step_tail_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = optim.CHUNK


# ---- the specification against torch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", ["off", "engaged", "idle"])
def test_the_restatement_is_as_close_to_fp64_as_torch_is(clip):
    """Over the GPU test's case list, 5 steps: the restatement's worst |p - p64| (and m, v) against an fp64 run of the same formula
    must not exceed twice the worst error of torch.optim.Adam(foreach=False) in fp32 on this CPU against the same fp64 run.  Both
    are measured here, so the yardstick is torch.  The factor 2 allows for another association of about ten roundings.
    Measured ratios restatement / torch on an x86-64 CPU: without clipping and with an idle clip p 1.000, m 1.236, v 1.000 (worst
    |m - m64| 1.76e-6 against torch's 1.43e-6 at gradients of magnitude 1e2); with the clip engaged p 0.58, m 0.26, v 0.22 (torch
    rounds the scaled gradients to fp32 in memory and takes its norm in fp32)."""
    lay = R.layout(CHUNK)
    max_norm = {"off": None, "engaged": 0.25 * R.big_norm(lay), "idle": 1e6 * R.big_norm(lay)}[clip]
    start = R.initial(lay)
    spec = R.RefAdam(start, R.groups_of(lay), max_norm, np.float32)
    exact = R.RefAdam(start, R.groups_of(lay), max_norm, np.float64)
    tp = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in start.items()}
    topt = torch.optim.Adam([dict(params=[tp[k] for k in names], **hyper) for hyper, names in R.groups_of(lay)], betas=R.BETAS, eps=R.EPS,
                            foreach=False)
    for s in range(R.STEPS):
        g = R.gradients(lay, s)
        spec.step(g)
        exact.step(g)
        for k, p in tp.items():
            p.grad = None if g[k] is None else torch.from_numpy(g[k].copy())
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(tp.values()), max_norm)
        topt.step()
    worst = {}
    for what, ours, theirs in (("p", spec.p, {k: v.detach().numpy() for k, v in tp.items()}),
                               ("m", spec.m, {k: topt.state[tp[k]]["exp_avg"].numpy() for k in tp if topt.state[tp[k]]}),
                               ("v", spec.v, {k: topt.state[tp[k]]["exp_avg_sq"].numpy() for k in tp if topt.state[tp[k]]})):
        ref = getattr(exact, what)
        e_spec = max(float(np.max(np.abs(ours[k].astype(np.float64) - ref[k]))) for k in theirs if ref[k].size)
        e_torch = max(float(np.max(np.abs(theirs[k].astype(np.float64) - ref[k]))) for k in theirs if ref[k].size)
        worst[what] = (e_spec, e_torch)
        print("clip %s, %s: restatement %.3e, torch %.3e, ratio %.3f" % (clip, what, e_spec, e_torch, e_spec / e_torch if e_torch else 0.0))
    for what, (e_spec, e_torch) in worst.items():
        assert np.isfinite(e_spec) and e_spec <= 2 * e_torch, "%s: restatement %.3e vs torch %.3e" % (what, e_spec, e_torch)
    # the tensor without gradient did not move and took no step, on either side
    assert np.array_equal(spec.p["nograd"], start["nograd"]) and spec.step_of["nograd"] == 0 and not topt.state[tp["nograd"]]
    if clip == "engaged":
        assert spec.clip_coef < 1
    if clip == "idle":
        assert spec.clip_coef == 1


def test_the_reference_cross_entropy_is_torch_s():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((9, 7)) * 5
    t = rng.integers(0, 7, 9)
    t[2] = t[5] = R.IGNORE
    xt = torch.tensor(x, requires_grad=True)
    want = torch.nn.functional.cross_entropy(xt, torch.from_numpy(t))
    want.backward()
    loss, d = R.cross_entropy(x, t)
    assert abs(loss - want.item()) < 1e-13 and np.abs(d - xt.grad.numpy()).max() < 1e-15
    assert np.isnan(R.cross_entropy(x, np.full(9, R.IGNORE))[0])
    t[0] = 7
    loss, d = R.cross_entropy(x, t)
    assert np.isnan(loss) and np.isnan(d[0]).all() and np.isfinite(d[1:]).all()


# ---- the chunk table -------------------------------------------------------------------------------------------------------
def _unpack(table):
    return table[:, :4], table[:, 4] & 0xFFFFFFFF, table[:, 4] >> 32


def test_chunk_table_splits_tensors_at_chunk():
    sizes = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 0, 5]
    four = [tuple(torch.zeros(n) for _ in range(4)) for n in sizes]
    rows = [0, 1, 2, 0, 1, 2, 3]
    addr, n, row = _unpack(optim.chunk_table(four, rows))
    want_n, want_row, want_addr = [], [], []
    for ts, size, r in zip(four, sizes, rows):
        for off in range(0, size, CHUNK):
            want_n.append(min(CHUNK, size - off))
            want_row.append(r)
            want_addr.append([t.data_ptr() + 4 * off for t in ts])
    assert n.tolist() == want_n == [1, CHUNK - 1, CHUNK, CHUNK, 1, CHUNK, CHUNK, 3, 5]
    assert row.tolist() == want_row and addr.tolist() == want_addr
    assert optim.chunk_table(four, rows).dtype == np.int64 and optim.chunk_table(four, rows).shape[1] == ops.STEP_CHUNK_WORDS
    assert optim.chunk_table([], []).shape == (0, ops.STEP_CHUNK_WORDS)
    assert optim.chunk_table(four[:2], rows[:2], chunk=4)[:, 4].tolist()[:2] == [1, 4 | 1 << 32]
    assert CHUNK == ops.STEP_CHUNK == _lib.STEP_CONSTANTS["MGNNS_STEP_CHUNK"] == _lib.lib().mgnns_step_chunk_elems() and CHUNK % 4 == 0


def test_chunk_table_takes_a_view_s_address_as_base_plus_offset():
    base = torch.zeros(100)
    view = base[3:40]
    assert view.is_contiguous() and view.storage_offset() == 3
    other = torch.zeros(37)
    addr, n, row = _unpack(optim.chunk_table([(view, other, other, view)], [5], chunk=16))
    assert n.tolist() == [16, 16, 5] and row.tolist() == [5, 5, 5]
    assert addr[:, 0].tolist() == [base.data_ptr() + 4 * (3 + 16 * i) for i in range(3)] == addr[:, 3].tolist()
    assert addr[:, 1].tolist() == [other.data_ptr() + 64 * i for i in range(3)]
    with pytest.raises(ValueError, match="multiple of 4"):
        optim.chunk_table_from_addresses(np.array([[2, 4, 8, 12]], np.int64), np.array([1]), np.array([0]))
    assert (optim.chunk_table([(other, other, other, other)], [-1], chunk=16)[:, 4] >> 32).tolist() == [-1, -1, -1]      # norm only
    with pytest.raises(ValueError, match="row outside"):
        optim.chunk_table([(other, other, other, other)], [-2])
    with pytest.raises(ValueError, match="negative count"):
        optim.chunk_table_from_addresses(np.array([[4, 4, 8, 12]], np.int64), np.array([-1]), np.array([0]))


def test_step_without_gradients_does_nothing_and_asks_for_no_gpu():
    """With no gradient anywhere there is nothing to do: step() on CPU tensors returns before the device check, creates no state
    and advances no step; one live CPU parameter is then refused by name, and a refused step leaves no state behind."""
    nograd, live = (torch.nn.Parameter(torch.zeros(n)) for n in (7, 3))
    opt = optim.Adam([dict(params=[nograd]), dict(params=[live], lr=1e-2)], max_norm=1.0)
    assert opt.step() is None and not opt.state[nograd] and opt.total_norm is None
    live.grad = torch.ones(3)
    with pytest.raises(ValueError, match="parameters not on the GPU"):
        opt.step()
    assert not opt.state[live] and not opt.state[nograd]


def test_group_scalars_are_the_reference_s():
    for step in (1, 2, 5, 1000):
        got = np.asarray(optim.group_scalars(1e-3, 0.9, 0.999, 1e-8, 1e-4, step), np.float32)
        want = R.group_scalars(1e-3, 0.9, 0.999, 1e-8, 1e-4, step)
        assert got[:7].tolist() == [float(x) for x in want] and got[7] == 0 and len(got) == ops.STEP_GROUP_FLOATS


# ---- the binding -----------------------------------------------------------------------------------------------------------
def test_the_step_entry_points_are_derived_from_their_header():
    hdr = open(os.path.join(ROOT, "include", "mgnns_step.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = {n: (0 if p.strip() == "void" else len(p.split(","))) for n, p in re.findall(r"\b(mgnns_\w+)\s*\(([^()]*)\)\s*;", code)}
    assert declared == {"mgnns_step_chunk_elems": 0, "mgnns_step_chunk_record_bytes": 0, "mgnns_step_chunk_table_bytes": 1,
                        "mgnns_step_group_table_bytes": 1, "mgnns_step_partials_bytes": 1, "mgnns_ce_loss_fwd_bwd": 7,
                        "mgnns_grad_sumsq": 4, "mgnns_grad_clip_coef": 5, "mgnns_adam_step": 6}
    V, I32, F32, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert _lib.STEP_SIGNATURES == {"mgnns_ce_loss_fwd_bwd": [V, V, I32, I32, V, V, V], "mgnns_grad_sumsq": [V, I32, V, V],
                                    "mgnns_grad_clip_coef": [V, I32, F32, V, V], "mgnns_adam_step": [V, I32, V, I32, V, V]}
    assert _lib.STEP_SIZE_GETTERS == {"mgnns_step_chunk_elems": [], "mgnns_step_chunk_record_bytes": [], "mgnns_step_chunk_table_bytes": [I32],
                                      "mgnns_step_group_table_bytes": [I32], "mgnns_step_partials_bytes": [I32]}
    assert len(_lib.STEP_HEADERS) == 1 and _lib.ABI_VERSION == 26 and "MGNNS_STEP_CHUNK" not in _lib.CONSTANTS
    earlier = [_lib.SIGNATURES, _lib.SIZE_GETTERS, _lib.EXTENSION_SIGNATURES, _lib.EXTENSION_SIZE_GETTERS, _lib.SPLIT_SIGNATURES,
               _lib.SPLIT_SIZE_GETTERS, _lib.LAYOUT_SIGNATURES, _lib.LAYOUT_SIZE_GETTERS]
    for table in earlier:
        assert not set(table) & (set(_lib.STEP_SIGNATURES) | set(_lib.STEP_SIZE_GETTERS))
    lib = _lib.lib()
    for table, ret in ((_lib.STEP_SIGNATURES, ctypes.c_int), (_lib.STEP_SIZE_GETTERS, SZ)):
        for name, args in table.items():
            fn = getattr(lib, name)
            assert list(fn.argtypes) == args and fn.restype is ret
    with pytest.raises(_lib.MgnnsLibraryError, match="a second time"):
        _lib._read_extensions(_lib.STEP_HEADERS, {"mgnns_adam_step": None})


def test_the_size_getters_and_argument_checks_need_no_gpu():
    lib = _lib.lib()
    assert lib.mgnns_step_chunk_record_bytes() == 8 * ops.STEP_CHUNK_WORDS == 40
    assert lib.mgnns_step_chunk_table_bytes(3) == 120 and lib.mgnns_step_chunk_table_bytes(-1) == 0
    assert lib.mgnns_step_group_table_bytes(2) == 2 * 4 * ops.STEP_GROUP_FLOATS and lib.mgnns_step_group_table_bytes(-5) == 0
    assert lib.mgnns_step_partials_bytes(7) == 56 and lib.mgnns_step_partials_bytes(0) == 0
    E = {k: _lib.CONSTANTS[k] for k in ("MGNNS_ERR_ARG", "MGNNS_ERR_UNSUPP")}
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert lib.mgnns_ce_loss_fwd_bwd(None, a, 1, 3, a, a, None) == E["MGNNS_ERR_ARG"]
    for B, NL in ((1, 0), (1, 65), (0, 3), (-1, 3)):
        assert lib.mgnns_ce_loss_fwd_bwd(a, a, B, NL, a, a, None) == E["MGNNS_ERR_UNSUPP"]
        assert b"NL" in lib.mgnns_last_error()
    assert lib.mgnns_grad_sumsq(a, -1, a, None) == E["MGNNS_ERR_ARG"] and lib.mgnns_grad_sumsq(None, 1, a, None) == E["MGNNS_ERR_ARG"]
    assert lib.mgnns_grad_sumsq(None, 0, None, None) == 0 and lib.mgnns_adam_step(None, 0, None, 0, None, None) == 0
    assert lib.mgnns_grad_sumsq(a + 4, 1, a, None) == E["MGNNS_ERR_ARG"]
    assert lib.mgnns_grad_clip_coef(a, -1, 1.0, a, None) == E["MGNNS_ERR_ARG"] and lib.mgnns_grad_clip_coef(a, 1, 1.0, None, None) == E["MGNNS_ERR_ARG"]
    assert lib.mgnns_grad_clip_coef(a, 1, -1.0, a, None) == E["MGNNS_ERR_ARG"] and lib.mgnns_grad_clip_coef(a, 1, float("nan"), a, None) == E["MGNNS_ERR_ARG"]
    assert lib.mgnns_adam_step(a, 1, a, 0, a, None) == E["MGNNS_ERR_ARG"] and lib.mgnns_adam_step(a, -1, a, 1, a, None) == E["MGNNS_ERR_ARG"]
    assert lib.mgnns_adam_step(a, 1, None, 1, a, None) == E["MGNNS_ERR_ARG"] and lib.mgnns_adam_step(a, 1, a, 1, None, None) == E["MGNNS_ERR_ARG"]
    # the wrappers refuse CPU tensors as every operator does
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ce_loss(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.adam_step(torch.zeros(1, 5, dtype=torch.int64), 1, torch.zeros(1, 8), torch.ones(1))


# ---- state interchange and refusals ----------------------------------------------------------------------------------------
def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3), (5,), (2, 2, 2))]


def _torch_step(opt, params, k):
    g = torch.Generator().manual_seed(100 + k)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    opt.step()


def test_state_dict_round_trips_through_torch_adam():
    """torch.optim.Adam -> optim.Adam -> torch.optim.Adam: the state that comes back is the state that went in (torch's keys and
    types), and a torch optimizer that loaded it continues exactly like one that never stopped."""
    make = lambda ps: [dict(params=ps[:2], lr=1e-2), dict(params=ps[2:], lr=1e-3, weight_decay=1e-4)]
    pa, pb = _params(), _params()
    ta, tb = torch.optim.Adam(make(pa)), torch.optim.Adam(make(pb))
    for k in range(2):
        _torch_step(ta, pa, k)
        _torch_step(tb, pb, k)
    ours = optim.Adam(make(pb), max_norm=10)
    ours.load_state_dict(tb.state_dict())
    st = ours.state[pb[0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and torch.is_tensor(st["step"]) and st["step"].dtype == torch.float32
    assert st["step"].device.type == "cpu" and float(st["step"]) == 2 and st["exp_avg"].dtype == torch.float32
    back, sent = ours.state_dict(), tb.state_dict()
    assert back["param_groups"] == sent["param_groups"] and back["state"].keys() == sent["state"].keys()
    for i in sent["state"]:
        assert sent["state"][i].keys() == back["state"][i].keys()
        for k in sent["state"][i]:
            assert torch.equal(sent["state"][i][k], back["state"][i][k])
    tc = torch.optim.Adam(make(pb))
    tc.load_state_dict(back)
    for k in range(2, 4):
        _torch_step(ta, pa, k)
        _torch_step(tc, pb, k)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    # a fresh optim.Adam's groups carry every key torch.optim.Adam's have, so its own state_dict loads there too
    fresh = optim.Adam(make(_params()), lr=3e-4)
    t2 = torch.optim.Adam(make(_params()))
    t2.load_state_dict(fresh.state_dict())
    assert t2.param_groups[0].keys() == torch.optim.Adam(make(_params())).param_groups[0].keys()
    # the engine's adjust_learning_rate
    for group in ours.param_groups:
        group["lr"] *= 0.1
    assert ours.param_groups[0]["lr"] == pytest.approx(1e-3) and ours.state_dict()["param_groups"][1]["lr"] == pytest.approx(1e-4)
    ours.zero_grad()
    assert all(p.grad is None for p in pb)
    ours.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(2))], lr=0.5))
    assert len(ours.param_groups) == 3 and ours.param_groups[2]["betas"] == (0.9, 0.999)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "capturable", "differentiable"])
def test_unsupported_switches_are_refused_by_name(flag):
    with pytest.raises(ValueError, match=flag):
        optim.Adam(_params(), **{flag: True})
    opt = optim.Adam(_params())
    opt.param_groups[0][flag] = True              # e.g. arrived through load_state_dict
    with pytest.raises(ValueError, match=flag):
        opt.step()
    with pytest.raises(ValueError, match=flag):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(2))], **{flag: True}))


def test_unsupported_tensors_are_refused_by_name_without_a_gpu():
    def refused(p, grad, match):
        p = torch.nn.Parameter(p)
        opt = optim.Adam([p])
        p.grad = grad
        with pytest.raises(ValueError, match=match):
            opt.step()
        assert not opt.state[p]

    refused(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), "non-fp32")
    refused(torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.bfloat16), "non-fp32")
    refused(torch.zeros(4, 6).t(), torch.zeros(6, 4), "non-contiguous")
    refused(torch.zeros(4, 6), torch.zeros(6, 4).t(), "non-contiguous")
    refused(torch.zeros(4, 6), torch.zeros(4, 6).to_sparse(), "sparse gradients")
    refused(torch.zeros(4), torch.zeros(4), "parameters not on the GPU")
    with pytest.raises(ValueError, match="max_norm"):
        optim.Adam(_params(), max_norm=-1)
    with pytest.raises(ValueError, match="invalid lr"):
        optim.Adam(_params(), lr=-1e-3)
    with pytest.raises(ValueError, match="Python numbers"):
        optim.Adam(_params(), lr=torch.tensor(1e-3))
