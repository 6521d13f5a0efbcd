"""The fenced arena (tests/fenced_alloc.py) detects what it claims: run on the CPU against tests/fenced_standin.py, a module that
allocates through a module-global `torch` as mgnns_amd/ops.py does.  No project kernel runs here.  The last test holds the two fenced
GPU files to the list of launching wrappers of ops.py."""
import ast
import os
import re

import pytest
import torch

from tests import fenced_alloc, fenced_standin as S
from tests.fenced_alloc import FENCE, fenced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = "cpu"


def site(name):
    """Line of tests/fenced_standin.py that carries the marker `SITE <name>`."""
    with open(S.__file__) as f:
        for no, line in enumerate(f, 1):
            if line.rstrip().endswith("# SITE " + name):
                return "%s:%d" % (S.__file__, no)
    raise KeyError(name)


def arena_cpu():
    return fenced(S, fence_cpu=True)


# ---- passthrough and views ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize("shape", [(3, 5), (7,), (2, 3, 4), (0,), (4, 0, 3), (1,)])
def test_views_have_the_requested_shape_dtype_and_alignment(dtype, shape):
    with arena_cpu() as arena:
        forms = [S.out_shape(shape, dtype, CPU), S.out_shape(torch.Size(shape), dtype, torch.device(CPU)), S.out_shape(list(shape), dtype, CPU),
                 S.zeroed(shape, dtype, CPU), S.like(torch.ones(shape, dtype=dtype), device=CPU)]
        want = torch.empty(shape, dtype=dtype)
        for t in forms:
            assert t.shape == want.shape and t.dtype == dtype and t.stride() == want.stride() and t.is_contiguous()
            assert t.device.type == "cpu" and t.data_ptr() % 256 == 0
    arena.check()
    assert arena.counts() == {"empty": 4, "zeros": 1}
    for r in arena.records:
        assert r.region.numel() == 2 * FENCE + r.nbytes and r.nbytes == want.numel() * want.element_size()


def test_separate_ints_and_keywords_behave_as_torch_empty_does():
    with arena_cpu() as arena:
        t = S.out_f32(3, 5, CPU)
        u = S.torch.empty(2, 3, 4, dtype=torch.int64, device=torch.device(CPU), pin_memory=False, memory_format=torch.contiguous_format)
        v = S.torch.zeros((6,), device=CPU)                   # no dtype: torch's default
        assert (t.shape, t.dtype) == ((3, 5), torch.float32) and (u.shape, u.dtype) == ((2, 3, 4), torch.int64)
        assert (v.shape, v.dtype) == ((6,), torch.get_default_dtype())
    arena.check()
    assert [r.nbytes for r in arena.records] == [60, 192, 24]


def test_empty_like_follows_its_argument_and_its_keywords():
    src = torch.arange(12, dtype=torch.int32).view(3, 4)
    with arena_cpu() as arena:
        a = S.like(src, device=CPU)
        b = S.like(src, dtype=torch.float32, device=CPU)
        c = S.like(src)                                      # the argument's own device: a CPU tensor, fenced under fence_cpu
        assert (a.shape, a.dtype) == (src.shape, torch.int32) and (b.shape, b.dtype) == (src.shape, torch.float32)
        assert c.shape == src.shape and (a == -1).all() and torch.isnan(b).all() and (c == -1).all()
        with pytest.raises(NotImplementedError):
            S.like(src.t(), device=CPU)
    arena.check()
    assert len(arena.records) == 3


def test_host_and_pinned_requests_pass_through_untouched():
    with fenced(S) as arena:                                 # as the GPU tests use it: a CPU device is the host
        raw, z, e = S.host_staging(64)
        assert raw.dtype == torch.uint8 and raw.numel() == 64 and (z == 0).all() and e.numel() == 64
        assert S.zeros_bytes(5, CPU).numel() == 256          # the stand-in's own rounding: the real function ran
    assert arena.records == []
    with arena_cpu() as arena:                               # no device named at all: host, even when CPU devices are fenced
        raw, z, _ = S.host_staging(64)
        assert raw.numel() == 64 and (z == 0).all()
    assert [r.func for r in arena.records] == ["host_staging"] and arena.records[0].nbytes == 64 * 4
    if torch.cuda.is_available():
        with fenced(S) as arena:
            assert S.host_staging(64, pin=True)[0].is_pinned()
        assert arena.records == []


def test_everything_else_of_torch_is_forwarded():
    with arena_cpu():
        f32, ar, is_t = S.other_names()
        assert f32 is torch.float32 and torch.equal(ar, torch.arange(3)) and is_t is True
        assert S.torch.cuda is torch.cuda and S.torch is not torch
        with pytest.raises(NotImplementedError):
            S.torch.empty(3, device=CPU, requires_grad=True)


# ---- poison ---------------------------------------------------------------------------------------------------------------------
def test_untouched_allocations_read_as_poison_or_zero():
    with arena_cpu() as arena:
        assert torch.isnan(S.out_f32(5, 7, CPU)).all()
        assert torch.isnan(S.out_shape((33,), torch.bfloat16, CPU).float()).all()
        assert (S.out_shape((9,), torch.int32, CPU) == -1).all() and (S.out_shape((9,), torch.int64, CPU) == -1).all()
        assert (S.out_shape((9,), torch.uint8, CPU) == 255).all()
        assert (S.zeroed(11, torch.float32, CPU) == 0).all() and (S.zeroed((2, 3), torch.int32, CPU) == 0).all()
        zb = S.zeros_bytes(5, CPU)
        assert zb.dtype == torch.uint8 and zb.numel() == 5 and (zb == 0).all()        # exactly the bytes asked for: the fence is tight
        c = S.counter(3, CPU)
        assert c.dtype == torch.int32 and c.numel() == 3 and (c == 0).all()
    arena.check()
    assert arena.counts() == {"empty": 5, "zeros": 2, "counter": 2}


# ---- detection ------------------------------------------------------------------------------------------------------------------
def elems(t, offset_elems, n=1):
    """n elements of t's own buffer starting offset_elems from t's first element (as_strided: stays inside the arena's buffer)."""
    return t.as_strided((n,), (1,), t.storage_offset() + offset_elems)


def test_a_store_into_the_interior_alone_passes():
    with arena_cpu() as arena:
        t = S.out_f32(3, 5, CPU)
        t.fill_(1.0)
        elems(t, 14)[0] = 2.0                                # the last element
        S.counter(4, CPU).add_(1).sub_(1)
    arena.check()


@pytest.mark.parametrize("where,offset,reported", [
    ("before", -1, "first damaged byte offset -4 "),
    ("after", 15, "first damaged byte offset 0 "),
    ("after", 15 + (FENCE - 4) // 4, "first damaged byte offset %d " % (FENCE - 4)),
])
def test_a_store_outside_the_interior_is_reported_with_its_call_site(where, offset, reported):
    with arena_cpu() as arena:
        S.out_f32(2, 2, CPU).fill_(0.0)                      # a well-behaved neighbour stays out of the report
        t = S.out_f32(3, 5, CPU)
        elems(t, offset)[0] = 1.0
    with pytest.raises(AssertionError) as e:
        arena.check()
    msg = str(e.value)
    assert "1 finding" in msg and site("out_f32") in msg and "of 60 bytes" in msg
    assert "store %s the interior" % where in msg and reported in msg


def test_the_last_byte_of_the_fence_is_watched():
    with arena_cpu() as arena:
        t = S.out_shape((10,), torch.uint8, CPU)
        elems(t, 10 + FENCE - 1)[0] = 0                      # FENCE - 1 bytes after the interior
    with pytest.raises(AssertionError) as e:
        arena.check()
    assert site("out_shape") in str(e.value) and "first damaged byte offset %d " % (FENCE - 1) in str(e.value)


def test_a_store_outside_a_zero_size_allocation_is_reported():
    with arena_cpu() as arena:
        t = S.out_f32(0, 5, CPU)
        assert t.numel() == 0 and t.shape == (0, 5)
        elems(t, 0)[0] = 1.0
    with pytest.raises(AssertionError, match="store after the interior, first damaged byte offset 0 "):
        arena.check()


def test_a_counter_left_at_one_is_reported_with_its_call_site():
    with arena_cpu() as arena:
        c = S.counter(4, CPU)
        c[2] = 1
    with pytest.raises(AssertionError) as e:
        arena.check()
    msg = str(e.value)
    assert site("counter") in msg and "not zero again" in msg and "first byte offset 8" in msg
    arena.check(stateful=("counter",))                       # the documented exemption is by the allocating function's name


def test_zeros_need_not_be_zero_again_only_counters():
    with arena_cpu() as arena:
        S.zeroed(4, torch.float32, CPU).fill_(3.0)
    arena.check()


# ---- fence_input ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fence_input_copies_and_an_over_read_sees_nan(dtype):
    src = torch.randn(4, 6, generator=torch.Generator().manual_seed(3)).to(dtype)
    with arena_cpu() as arena:
        t = arena.fence_input(src.t())                       # a non-contiguous input comes back contiguous
        assert torch.equal(t, src.t()) and t.is_contiguous() and t.dtype == dtype and t.data_ptr() % 256 == 0
        assert torch.isnan(elems(t, 24).float()).all() and torch.isnan(elems(t, -1).float()).all()
        ints = arena.fence_input(torch.arange(5))
        assert torch.equal(ints, torch.arange(5)) and int(elems(ints, 5)[0]) == -1
        elems(t, 24)[0] = 0.0                                # a store past an input is a finding as well
    with pytest.raises(AssertionError, match="input allocation of %d bytes" % (24 * src.element_size())):
        arena.check()


# ---- restore --------------------------------------------------------------------------------------------------------------------
def test_everything_is_put_back_also_when_the_body_raises():
    real_zb = S.zeros_bytes
    with arena_cpu():
        assert S.torch is not torch and S.zeros_bytes is not real_zb
    assert S.torch is torch and S.zeros_bytes is real_zb
    with pytest.raises(KeyError):
        with arena_cpu():
            raise KeyError("body")
    assert S.torch is torch and S.zeros_bytes is real_zb
    assert fenced_alloc._torch is torch and torch.empty.__module__ != fenced_alloc.__name__          # torch itself is never patched


def test_views_outlive_the_block():
    with arena_cpu() as arena:
        t = S.out_f32(2, 3, CPU)
    t.fill_(4.0)
    arena.check()
    assert float(t.sum()) == 24.0 and S.out_f32(1, 1, CPU).data_ptr() != 0 and len(arena.records) == 1


# ---- coverage of the launching wrappers -----------------------------------------------------------------------------------------
# Launching wrappers of ops.py that the fenced GPU files leave out on purpose, each with its reason.
EXCLUDED = {}
for _n in ("stem_conv7", "maxpool3x3s2_nhwc", "conv_bf16_nhwc", "conv_transpose_pack", "conv_dgrad_bf16_nhwc", "conv_wgrad_bf16_nhwc",
           "conv_fold_bn", "conv_bn_unfold", "map_grad_relu_nhwc", "stem_wgrad", "maxpool3x3s2_bwd_nhwc"):
    EXCLUDED[_n] = "trunk convolution entry point: canary-fenced by test_matrix_pipe_edges_gpu.py / test_trunk_train_edges_gpu.py"
for _n in ("bn_stats_bf16_nhwc", "bn_apply_bf16_nhwc", "bn_backward_bf16_nhwc"):
    EXCLUDED[_n] = "BatchNorm entry point: canary-fenced by test_bn_train_gpu.py"
for _n in ("transpose_cast_bf16", "gemm_bf16_nt"):
    EXCLUDED[_n] = "the trunk's bf16 GEMM: canary-fenced by test_matrix_pipe_edges_gpu.py"
for _n in ("image_prep", "jpeg_decode", "jpeg_decode_progressive"):
    EXCLUDED[_n] = "input pipeline, not a wrapper family of the fenced sweep: its buffers are sized and owned by images.py's batch objects"
EXCLUDED["stamp"] = "profiling stamp of bench.py, off in every forward the suite runs"
EXCLUDED["gemm_bf16_set_form"] = "sets a switch of the trunk GEMM's launcher (an integer): launches nothing and allocates nothing"


def launching_wrappers():
    with open(os.path.join(ROOT, "mgnns_amd", "ops.py")) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and not node.name.startswith("_"):
            for c in ast.walk(node):
                if isinstance(c, ast.Call):
                    fn = c.func
                    if (isinstance(fn, ast.Name) and fn.id == "_launch") or (
                            isinstance(fn, ast.Attribute) and fn.attr == "call" and isinstance(fn.value, ast.Name) and fn.value.id == "_lib"):
                        names.add(node.name)
                        break
    return names


def test_every_launching_wrapper_is_reached_by_a_fenced_case():
    launching = launching_wrappers()
    assert len(launching) > 60 and {"linear", "bilstm", "adam_step", "label_gcn"} <= launching
    referenced = set()
    for name in ("test_fenced_kernels_gpu.py", "test_fenced_model_gpu.py"):
        with open(os.path.join(ROOT, "tests", name)) as f:
            referenced |= set(re.findall(r"\bops\.(\w+)", f.read()))
    stale = sorted(set(EXCLUDED) - launching)
    assert not stale, "excluded names that are no launching wrapper of ops.py (any more): %s" % stale
    both = sorted(set(EXCLUDED) & referenced)
    assert not both, "excluded and yet referenced: %s" % both
    missing = sorted(launching - referenced - set(EXCLUDED))
    assert not missing, "launching wrappers of ops.py that no fenced case reaches: %s" % missing
