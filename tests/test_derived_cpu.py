"""The rules of mgnns_amd.derived.derived -- the one helper behind every weight-derived value the forward keeps between calls --
and of the two parks a superseded entry can go to, on plain CPU tensors ("Derived packs and launch scratch")."""
import gc
import types
import weakref

import torch

from mgnns_amd import ops
from mgnns_amd.derived import derived
from mgnns_amd.model import Multi_GCN_Multihead_Att


class Builder:
    """build() that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return ["value", self.calls]


def test_a_second_call_with_unchanged_sources_returns_the_same_object():
    store, build = {}, Builder()
    a, b = torch.randn(3, 4), torch.randn(4)
    first = derived(store, "slot", (a, b), build)
    assert derived(store, "slot", (a, b), build) is first
    assert derived(store, "slot", (a.detach(), b), build) is first          # another tensor object over the same weights
    assert build.calls == 1 and list(store) == ["slot"]


def test_a_version_bump_is_a_miss():
    store, build = {}, Builder()
    t = torch.randn(3, 4)
    first = derived(store, "slot", (t,), build)
    with torch.no_grad():
        t.mul_(1.0)
    second = derived(store, "slot", (t,), build)
    assert second is not first and build.calls == 2
    assert derived(store, "slot", (t,), build) is second and build.calls == 2


def test_a_replaced_source_is_a_miss():
    store, build = {}, Builder()
    a, b = torch.randn(3, 4), torch.randn(4)
    first = derived(store, "slot", (a, b), build)
    b2 = b.clone()
    second = derived(store, "slot", (a, b2), build)
    assert second is not first and build.calls == 2
    assert derived(store, "slot", (a, b2), build) is second and build.calls == 2


def test_a_changed_extra_is_a_miss():
    store, build = {}, Builder()
    t = torch.randn(3, 4)
    first = derived(store, "slot", (t,), build, extra=("bf16",))
    second = derived(store, "slot", (t,), build, extra=("split",))
    assert second is not first and build.calls == 2
    assert derived(store, "slot", (t,), build, extra=("split",)) is second and build.calls == 2


def test_a_view_of_another_shape_over_the_same_storage_is_a_miss():
    store, build = {}, Builder()
    t = torch.randn(3, 4)
    v = t.view(4, 3)
    assert v.data_ptr() == t.data_ptr() and v._version == t._version
    first = derived(store, "slot", (t,), build)
    second = derived(store, "slot", (v,), build)
    assert second is not first and build.calls == 2
    assert derived(store, "slot", (v,), build) is second and build.calls == 2


def test_an_in_place_reshape_of_the_pinned_tensor_itself_is_a_miss():
    store, build = {}, Builder()
    t = torch.randn(3, 4)
    first = derived(store, "slot", (t,), build)
    ptr = t.data_ptr()
    t.t_()                                                            # same object, same address: the version says so
    assert t.data_ptr() == ptr and tuple(t.shape) == (4, 3)
    assert derived(store, "slot", (t,), build) is not first and build.calls == 2


def test_replaced_data_is_a_miss_and_the_old_storage_stays_pinned():
    store, build = {}, Builder()
    p = torch.nn.Parameter(torch.randn(3, 4))
    first = derived(store, "slot", (p,), build)
    old_ptr = p.data_ptr()
    p.data = torch.randn(3, 4)                                        # no version bump; the entry still holds the old storage,
    fresh = [torch.randn(3, 4) for _ in range(8)]                     # so no new tensor can land on its address
    assert p.data_ptr() != old_ptr and all(f.data_ptr() != old_ptr for f in fresh)
    assert store["slot"][4][0].data_ptr() == old_ptr
    assert derived(store, "slot", (p,), build) is not first and build.calls == 2


def test_none_among_the_sources_is_ignored():
    store, build = {}, Builder()
    a, b = torch.randn(3), torch.randn(5)
    first = derived(store, "slot", (a, None, b), build)
    assert derived(store, "slot", (a, b), build) is first
    assert derived(store, "slot", (None, a, b, None), build) is first
    assert build.calls == 1


def test_park_gets_the_superseded_entry_after_build_and_not_on_the_first_build():
    store, events = {}, []

    def build():
        events.append("build")
        return object()

    def park(entry):
        events.append(("park", entry))

    t = torch.randn(3)
    first = derived(store, "slot", (t,), build, park=park)
    assert events == ["build"]                                        # nothing superseded yet
    old_entry = store["slot"]
    t2 = torch.randn(3)
    second = derived(store, "slot", (t2,), build, park=park)
    assert events[1] == "build" and events[2][0] == "park" and len(events) == 3
    parked = events[2][1]
    assert parked is old_entry and parked[2] is first and parked[0][0] is t          # the value AND its pinned sources
    assert store["slot"][2] is second
    derived(store, "slot", (t2,), build, park=park)                   # a hit parks nothing
    assert len(events) == 3


def test_an_entry_pins_its_sources_until_it_is_replaced_and_not_parked():
    store, build = {}, Builder()
    t = torch.randn(3, 4)
    ref = weakref.ref(t)
    derived(store, "slot", (t,), build)
    del t
    gc.collect()
    assert ref() is not None                                          # the entry holds the tensor: its address cannot be recycled
    derived(store, "slot", (torch.randn(3, 4),), build)              # replaced, no park
    gc.collect()
    assert ref() is None and build.calls == 2


def test_a_parked_entry_keeps_its_sources_pinned():
    store, build, parked = {}, Builder(), []
    t = torch.randn(3, 4)
    ref = weakref.ref(t)
    derived(store, "slot", (t,), build, park=parked.append)
    del t
    derived(store, "slot", (torch.randn(3, 4),), build, park=parked.append)
    gc.collect()
    assert ref() is not None and len(parked) == 1
    parked.clear()
    gc.collect()
    assert ref() is None


def test_model_level_park_keeps_superseded_entries_only_while_a_graph_lives():
    """Multi_GCN_Multihead_Att._park on a bare object with the three attributes it touches."""
    m = types.SimpleNamespace(_wt_cache={}, _live_graphs=0, _wt_retired=[])
    park = lambda entry: Multi_GCN_Multihead_Att._park(m, entry)
    build = Builder()
    derived(m._wt_cache, "head", (torch.randn(3),), build, park=park)
    derived(m._wt_cache, "head", (torch.randn(3),), build, park=park)
    assert m._wt_retired == [] and build.calls == 2                   # no graph alive: the old entry is simply dropped
    m._live_graphs = 1
    old = m._wt_cache["head"]
    derived(m._wt_cache, "head", (torch.randn(3),), build, park=park)
    assert len(m._wt_retired) == 1 and m._wt_retired[0] is old and m._wt_cache["head"] is not old


def test_layer_level_park_fills_while_a_capture_lives_and_empties_with_the_last_one():
    store, build = {}, Builder()
    saved = ops._LIVE_CAPTURES, list(ops._RETIRED)
    ops._LIVE_CAPTURES = 0                                            # whatever an earlier test left: this one starts with no capture
    del ops._RETIRED[:]
    try:
        derived(store, "slot", (torch.randn(3),), build, park=ops.retire)
        derived(store, "slot", (torch.randn(3),), build, park=ops.retire)
        assert ops._RETIRED == [] and build.calls == 2                # no capture alive: nothing is parked
        ops.capture_born()
        try:
            old = store["slot"]
            derived(store, "slot", (torch.randn(3),), build, park=ops.retire)
            assert len(ops._RETIRED) == 1 and ops._RETIRED[0] is old
        finally:
            ops.capture_gone()
        assert ops._LIVE_CAPTURES == 0 and ops._RETIRED == []
    finally:
        ops._LIVE_CAPTURES = saved[0]
        ops._RETIRED[:] = saved[1]
