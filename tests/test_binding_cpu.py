"""The ctypes binding is derived from include/mgnns_hip.h (mgnns_amd/_lib.py): the parser on small synthetic headers, the derived
tables against the real header and the built library, and the one call helper (_lib.call / ops._launch) against a stub."""
import ctypes
import os
import re

import pytest
import torch

from mgnns_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = {"mgnns_last_error", "mgnns_abi_version", "mgnns_source_fingerprint"}
PP = ctypes.POINTER(ctypes.c_void_p)


# ---- the parser ---------------------------------------------------------------------------------------------------------------
def test_parser_on_a_synthetic_header():
    decls, consts = _lib.parse_header("""
        #ifndef X_H
        #define X_H
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef void* mgnns_stream_t;
        typedef struct mgnns_comm_s* mgnns_comm_t;   /* int mgnns_fake(int x); */
        // int mgnns_fake(int x);
        /* a block comment over lines
           int mgnns_fake(int x);
        */
        #define MGNNS_ACT_RELU   1   /* F.relu */
        #define MGNNS_ERR_X (-3)
        #define MGNNS_ABI_VERSION 7
        int mgnns_spread(const float* x, int n /* rows */,
                         float eps, double m,
                         int64_t k, long long j, uint64_t seed,
                         size_t bytes, const unsigned char* mask,
                         mgnns_stream_t stream);
        int mgnns_ptrs(const float* const* w, void** out, mgnns_comm_t* comm, mgnns_comm_t c, const void * const * packed);
        int mgnns_none(void);
        size_t mgnns_bytes(int a, int b);
        const char* mgnns_text(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    c = ctypes
    assert consts == {"MGNNS_ACT_RELU": 1, "MGNNS_ERR_X": -3, "MGNNS_ABI_VERSION": 7}
    assert set(decls) == {"mgnns_spread", "mgnns_ptrs", "mgnns_none", "mgnns_bytes", "mgnns_text"}      # no mgnns_fake
    assert decls["mgnns_spread"] == (c.c_int, [c.c_void_p, c.c_int, c.c_float, c.c_double, c.c_int64, c.c_longlong, c.c_uint64,
                                               c.c_size_t, c.c_void_p, c.c_void_p])
    assert decls["mgnns_ptrs"] == (c.c_int, [PP, PP, PP, c.c_void_p, PP])
    assert decls["mgnns_none"] == (c.c_int, [])
    assert decls["mgnns_bytes"] == (c.c_size_t, [c.c_int, c.c_int])
    assert decls["mgnns_text"] == (c.c_char_p, [])


@pytest.mark.parametrize("decl,name", [("int mgnns_short_arg(const float* x, short n);", "mgnns_short_arg"),
                                       ("float mgnns_float_ret(int n);", "mgnns_float_ret"),
                                       ("int mgnns_deep(float*** x);", "mgnns_deep"),
                                       ("int mgnns_array(float x[4]);", "mgnns_array"),
                                       ("int mgnns_callback(void (*f)(int));", "mgnns_callback")])
def test_parser_refuses_a_type_outside_its_map(decl, name):
    with pytest.raises(_lib.MgnnsLibraryError, match=name):
        _lib.parse_header("typedef void* mgnns_stream_t;\nint mgnns_fine(int a);\n" + decl)


def test_a_missing_or_empty_header_is_refused_with_its_path(tmp_path):
    with pytest.raises(_lib.MgnnsLibraryError, match="no_such_header.h"):
        _lib._read_header(str(tmp_path / "no_such_header.h"))
    p = tmp_path / "empty.h"
    p.write_text("/* nothing declared */\n")
    with pytest.raises(_lib.MgnnsLibraryError, match="empty.h"):
        _lib._read_header(str(p))


# ---- the real header ------------------------------------------------------------------------------------------------------------
def _declared():
    """{name: (return type text, parameter count)} by this test's own reading of the header."""
    hdr = open(os.path.join(ROOT, "include", "mgnns_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([\w \*]+?)\s*\b(mgnns_\w+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M):
        out[name] = (ret.replace(" *", "*"), 0 if params.strip() == "void" else len(params.split(",")))
    return out


def test_tables_partition_the_declared_functions():
    declared = _declared()
    assert len(declared) == 148
    sig, size = set(_lib.SIGNATURES), set(_lib.SIZE_GETTERS)
    assert sig | size | SPECIAL == set(declared)
    assert not (sig & size) and not (sig & SPECIAL) and not (size & SPECIAL)
    for name, (ret, n) in declared.items():
        table = _lib.SIZE_GETTERS if ret == "size_t" else _lib.SIGNATURES
        if name in SPECIAL:
            continue
        assert ret in ("int", "size_t"), name
        assert name in table and len(table[name]) == n, name
    for name, args in _lib.SIZE_GETTERS.items():
        assert _lib._DECLS[name][0] is ctypes.c_size_t
    assert _lib._DECLS["mgnns_last_error"] == (ctypes.c_char_p, []) and _lib._DECLS["mgnns_source_fingerprint"] == (ctypes.c_char_p, [])
    assert _lib._DECLS["mgnns_abi_version"] == (ctypes.c_int, [])


def test_abi_number_and_constants_come_from_the_header():
    assert _lib.ABI_VERSION == 26
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU2) == (0, 1, 2)
    assert (ops.ELT_ADD, ops.ELT_RELU_BWD, ops.ELT_LRELU2_BWD) == (0, 1, 2)
    assert (ops.DROP_LABEL_ATTN, ops.DROP_HEAD, ops.DROP_LSTM, ops.DROP_TEXT_GCN) == (3, 4, 5, 6)
    assert (ops.DROP_ATTN, ops.DROP_FC, ops.DROP_FFN) == (0, 1, 2)
    C = _lib.CONSTANTS
    assert (C["MGNNS_ERR_ARG"], C["MGNNS_ERR_LAUNCH"], C["MGNNS_ERR_UNSUPP"]) == (-1, -2, -3)
    assert (C["MGNNS_STATUS_LABEL_GCN_TIMEOUT"], C["MGNNS_STATUS_CLUSTER_TIMEOUT"], C["MGNNS_STATUS_BAD_PLAN"]) == (1, 2, 3)


def test_the_loaded_library_is_bound_as_declared():
    L = _lib.lib()
    for name, args in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int, name
    for name, args in _lib.SIZE_GETTERS.items():
        fn = getattr(L, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_size_t, name
    assert L.mgnns_last_error.restype is ctypes.c_char_p and L.mgnns_source_fingerprint.restype is ctypes.c_char_p
    # the pointer-to-pointer arguments take what the callers pass: arrays of addresses and a byref(handle)
    assert _lib.SIGNATURES["mgnns_bilstm_bf16_prepack"][:2] == [PP, PP] and _lib.SIGNATURES["mgnns_comm_init_rank"][-1] is PP
    PP.from_param((ctypes.c_void_p * 2)(1, 2))
    PP.from_param(ctypes.byref(ctypes.c_void_p()))
    ctypes.c_void_p.from_param(ctypes.byref(ctypes.c_int()))           # mgnns_comm_info's int* arguments


# ---- the call helper ------------------------------------------------------------------------------------------------------------
class _Stub:
    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def __call__(self, *args):
        self.calls.append(args)
        return self.rc


class _AskedTimer(ops.KernelTimer):
    def __init__(self, yes):
        super().__init__()
        self.yes, self.asked = yes, []

    def wants(self, name):
        self.asked.append(name)
        return self.yes


def test_call_passes_a_zero_return_and_raises_on_any_other(monkeypatch):
    ok, bad = _Stub(0), _Stub(-1)
    monkeypatch.setitem(_lib._bound, "mgnns_stub_ok", ok)
    monkeypatch.setitem(_lib._bound, "mgnns_stub_bad", bad)
    assert _lib.call("mgnns_stub_ok", 1, None, 2.5) is None and ok.calls == [(1, None, 2.5)]
    with pytest.raises(RuntimeError, match=r"mgnns_stub_bad failed \(-1\)"):
        _lib.call("mgnns_stub_bad", 7)
    assert bad.calls == [(7,)]
    with pytest.raises(AttributeError):
        _lib.call("mgnns_no_such_entry_point")
    monkeypatch.setattr(ops, "_TIMER", None)
    ops._launch("mgnns_stub_ok", 3, key=(9,))
    with pytest.raises(RuntimeError, match="mgnns_stub_bad failed"):
        ops._launch("mgnns_stub_bad", 3, key=(9,))
    assert ok.calls[-1] == (3,) and bad.calls[-1] == (3,)


def test_a_bound_function_is_looked_up_once(monkeypatch):
    L = _lib.lib()
    monkeypatch.delitem(_lib._bound, "mgnns_take_status", raising=False)
    assert "mgnns_take_status" not in _lib._bound
    _lib.call("mgnns_take_status")                                      # host-only: reads and clears the status word, 0 = fine
    assert _lib._bound["mgnns_take_status"] is L.mgnns_take_status


def test_launch_without_a_wanting_timer_creates_no_event(monkeypatch):
    stub = _Stub(0)
    monkeypatch.setitem(_lib._bound, "mgnns_stub", stub)

    def no_event(*a, **k):
        raise AssertionError("an event was created for a launch the timer does not want")
    monkeypatch.setattr(torch.cuda, "Event", no_event)
    t = _AskedTimer(False)
    monkeypatch.setattr(ops, "_TIMER", t)
    ops._launch("mgnns_stub", 1, 2)
    ops._launch("mgnns_stub", 3, key=(5, True))
    ops._launch("mgnns_stub", 4, key=(5,), alias="mgnns_other")
    ops._launch("mgnns_stub", 5, key=(5,), wanted="mgnns_other_name")
    assert t.asked == ["mgnns_stub", "mgnns_stub", "mgnns_other", "mgnns_other_name"] and t.events == {}
    assert stub.calls == [(1, 2), (3,), (4,), (5,)]


def test_launch_files_events_under_the_name_and_the_key_fields(monkeypatch):
    """(with events that record nothing: the recording path itself runs in tests/test_model_gpu.py's timer tests)"""
    stub = _Stub(0)
    monkeypatch.setitem(_lib._bound, "mgnns_stub", stub)
    order = []

    class Ev:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            order.append(len(stub.calls))
    monkeypatch.setattr(torch.cuda, "Event", Ev)
    t = _AskedTimer(True)
    monkeypatch.setattr(ops, "_TIMER", t)
    ops._launch("mgnns_stub", 1)
    ops._launch("mgnns_stub", 2, key=(64, False))
    ops._launch("mgnns_stub", 3, key=(7,), alias="mgnns_other")
    ops._launch("mgnns_stub", 4, key=(7, 8), wanted="mgnns_other_name")
    assert t.asked == ["mgnns_stub", "mgnns_stub", "mgnns_other", "mgnns_other_name"]
    assert set(t.events) == {("mgnns_stub",), ("mgnns_stub", 64, False), ("mgnns_other", 7), ("mgnns_stub", 7, 8)}
    assert all(len(v) == 1 for v in t.events.values())
    assert order == [0, 1, 1, 2, 2, 3, 3, 4]                           # one event before and one after each call
