"""Values derived from tensors and rebuilt when those tensors change: the one rule behind every weight pack, composed map,
concatenated LSTM weight, folded table and CSR pair that the forward keeps between calls ("Derived packs and
launch scratch").  Plain torch: imports without a GPU and without the library.
"""
from operator import is_


def _shapes(sources):
    return [(t.shape, t.get_device()) for t in sources if t is not None]


def derived(store, slot, sources, build, extra=(), park=None):
    """store[slot]'s value if it was built from exactly these `sources` (None members are skipped) and this `extra`, else
    build() -- stored in its place -- after handing the superseded entry to park(entry), if there is one and a park is given.

    An entry is the tuple (sources, stamp, value, shapes, pins).  The stamp holds (data_ptr, _version) per source, then `extra`:
    whatever hashable is part of the identity without being a tensor.  shapes holds (shape, device index) per source.  pins
    holds a detach() of every source: it shares the source's storage, so that storage cannot be freed and handed to another
    weight while the entry lives -- not even after `source.data = other` -- and an address in the stamp was never recycled.
    A hit is an equal stamp and equal shapes.  Shapes are not read again from a source that is the very tensor object the
    entry holds: every in-place operation, those that only change the shape included, bumps _version, so with its address
    and version unchanged such a tensor still has the shape and device it had (the one way round that is
    `t.data = <another view of t's own storage at the same address>`, which this package does not do).  The value is built
    BEFORE the old entry is parked or dropped, and a parked entry keeps its sources pinned along with its value."""
    stamp = ([(t.data_ptr(), t._version) for t in sources if t is not None], extra)
    entry = store.get(slot)
    if entry is not None and entry[1] == stamp and (
            len(entry[0]) == len(sources) and all(map(is_, sources, entry[0])) or _shapes(sources) == entry[3]):
        return entry[2]
    value = build()
    if entry is not None and park is not None:
        park(entry)
    store[slot] = (tuple(sources), stamp, value, _shapes(sources), [t.detach() for t in sources if t is not None])
    return value
