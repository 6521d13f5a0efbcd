"""Fenced, poisoned allocations for the wrappers of mgnns_amd: a test-side stand-in for the address sanitizer.

    with fenced(ops, metrics, optim, images) as arena:
        ...   # calls into mgnns_amd
    arena.check()

Inside the block the global `torch` of each named module is a proxy that forwards every attribute to the real torch except
`empty`, `empty_like` and `zeros`; a module-level `zeros_bytes` (ops.zeros_bytes, which ops.zeros_i32 reaches through the module
global) is replaced as well.  torch itself is never patched, and everything is put back on exit, also when the body raises.

Every DEVICE allocation made through those names is the interior of a fresh uint8 buffer of FENCE + nbytes + FENCE bytes:
  * both fences are 0xFF bytes; the post-fence starts at the first byte after nbytes (no rounding up: a kernel must not rely on the
    allocator's 512-byte granularity);
  * the interior of `empty` / `empty_like` is 0xFF bytes as well (NaN in fp32 and bf16, -1 in int32 and int64, 255 in uint8): a
    kernel that reads a slot nothing has written computes NaN, and an unwritten index lands in the fence, not gigabytes away;
  * the interior of `zeros` / `zeros_bytes` is zero;
  * the fill is issued on the current stream, which is synchronised before the tensor is handed out (the zero pool of ops.py makes
    the same assumption: reserve_zeros).
Host and pinned allocations (no `device`, a CPU device, or pin_memory=True) pass through untouched.

`arena.check()` synchronises and raises AssertionError naming every allocation (call site, size, first damaged byte, before or
after the interior) whose fences are no longer all 0xFF, and every `counter` allocation (zeros_bytes) whose interior is not all zero
again: counters "are left at zero by the kernels themselves" (ops.py).  `arena.fence_input(t)` gives a test's input the same fences,
so that an over-read that reaches a result turns it into NaN.  The arena keeps every buffer alive until it is dropped: views cached
in packs or scratch dicts stay valid.

EAGER ONLY: the fills synchronise the stream, so nothing inside the block may capture a hipGraph (torch.cuda.graph,
graph.GraphedForward); a capture under the arena is an error of the test, not a case.

Only tensor views are used (no raw pointer is dereferenced), so the arena works for any device; `fence_cpu=True` fences explicit
`device="cpu"` requests too, which is how tests/test_fenced_alloc_cpu.py exercises it without a GPU.
"""
import contextlib
import os
import sys

import torch as _torch

FENCE = 4096        # bytes on each side: a multiple of every alignment the wrappers check (16, 256), 4 x a wave's widest store (64 x 16 B)
ALIGN = 256
POISON = 0xFF
_HERE = os.path.abspath(__file__)
_SKIP_FUNCS = ("zeros_bytes", "zeros_i32")     # allocation helpers: the record names THEIR caller


def _call_site():
    f = sys._getframe(1)
    while f is not None and (os.path.abspath(f.f_code.co_filename) == _HERE or f.f_code.co_name in _SKIP_FUNCS):
        f = f.f_back
    if f is None:
        return "?", 0, "?", ()
    site = (f.f_code.co_filename, f.f_lineno, f.f_code.co_name)
    here, chain = os.path.dirname(site[0]), []           # the callers inside the same package: a lambda's owner, a helper's wrapper
    while f is not None and len(chain) < 8 and os.path.dirname(f.f_code.co_filename) == here:
        chain.append(f.f_code.co_name)
        f = f.f_back
    return site + (tuple(chain),)


class Allocation:
    __slots__ = ("region", "nbytes", "kind", "file", "line", "func", "callers")

    def __init__(self, region, nbytes, kind, site):
        self.region, self.nbytes, self.kind = region, nbytes, kind
        self.file, self.line, self.func, self.callers = site

    @property
    def interior(self):
        return self.region[FENCE:FENCE + self.nbytes]

    def where(self):
        return "%s:%d (%s)" % (self.file, self.line, self.func)


class Arena:
    def __init__(self, fence_cpu=False):
        self.fence_cpu = bool(fence_cpu)
        self.records = []

    # ---- allocation -----------------------------------------------------------------------------------------------------------
    def is_host(self, device, pin_memory=False):
        if pin_memory or device is None:
            return True
        return _torch.device(device).type == "cpu" and not self.fence_cpu

    def alloc(self, shape, dtype, device, kind, fill):
        device = _torch.device(device)
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _torch.empty((), dtype=dtype).element_size()
        raw = _torch.empty(FENCE + nbytes + FENCE + ALIGN - 1, dtype=_torch.uint8, device=device)
        skip = (-raw.data_ptr()) % ALIGN                 # the caching allocator aligns to 512 B on the GPU, the host one to 64 B
        region = raw[skip:skip + FENCE + nbytes + FENCE]
        region.fill_(POISON)
        if fill != POISON:
            region[FENCE:FENCE + nbytes].fill_(fill)
        if device.type == "cuda":
            _torch.cuda.current_stream(device).synchronize()
        rec = Allocation(region, nbytes, kind, _call_site())
        self.records.append(rec)
        return rec.interior.view(dtype).view(shape)

    def fence_input(self, t):
        """A contiguous copy of `t` (same device, dtype, shape) inside 0xFF fences."""
        out = self.alloc(t.shape, t.dtype, t.device, "input", POISON)
        out.copy_(t)
        if t.device.type == "cuda":
            _torch.cuda.current_stream(t.device).synchronize()
        return out

    def counts(self):
        c = {}
        for r in self.records:
            c[r.kind] = c.get(r.kind, 0) + 1
        return c

    # ---- verdict --------------------------------------------------------------------------------------------------------------
    def check(self, stateful=()):
        """stateful: names of the mgnns_amd functions whose zeros_bytes buffers hold more than counters by their stated contract
        (the caller checks the counter part itself); the interiors of what they allocate, directly or through a helper of their
        module, are not required to be zero again."""
        if _torch.cuda.is_available():
            _torch.cuda.synchronize()
        bad = []
        for r in self.records:
            pre, post = r.region[:FENCE], r.region[FENCE + r.nbytes:]
            if not bool(_torch.cat([pre, post]).eq(POISON).all()):                       # FENCE-CHECK
                for name, part in (("before", pre), ("after", post)):
                    hit = part.ne(POISON).nonzero()
                    if hit.numel():
                        off = int(hit[0]) - (FENCE if name == "before" else 0)           # relative to the interior's start / end
                        bad.append("%s allocation of %d bytes at %s: store %s the interior, first damaged byte offset %d "
                                   "(%d bytes damaged)" % (r.kind, r.nbytes, r.where(), name, off, int(hit.numel())))
            if r.kind == "counter" and r.nbytes and not set(r.callers) & set(stateful):
                live = r.interior.ne(0).nonzero()                                        # COUNTER-CHECK
                if live.numel():
                    bad.append("counter allocation of %d bytes at %s: not zero again after the launch, first byte offset %d" % (
                        r.nbytes, r.where(), int(live[0])))
        if bad:
            raise AssertionError("fenced arena: %d finding(s)\n  " % len(bad) + "\n  ".join(bad))


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
        return tuple(size[0])
    return tuple(size)


def _plain_kwargs(kw, name):
    """The remaining keywords must ask for what the arena gives: a strided, contiguous tensor without autograd."""
    if kw.pop("requires_grad", False):
        raise NotImplementedError("fenced %s: requires_grad" % name)
    if kw.pop("layout", _torch.strided) is not _torch.strided:
        raise NotImplementedError("fenced %s: layout" % name)
    if kw.pop("memory_format", _torch.contiguous_format) not in (_torch.contiguous_format, _torch.preserve_format):
        raise NotImplementedError("fenced %s: memory_format" % name)
    if kw:
        raise NotImplementedError("fenced %s: keyword(s) %s" % (name, sorted(kw)))


class TorchProxy:
    """Stands in for a module's global `torch`."""

    def __init__(self, arena):
        object.__setattr__(self, "_arena", arena)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    def _make(self, real, kind, fill, size, kw):
        a = self._arena
        if a.is_host(kw.get("device"), kw.get("pin_memory", False)):
            return real(*size, **kw)
        kw = dict(kw)
        device = kw.pop("device")
        dtype = kw.pop("dtype", None) or _torch.get_default_dtype()
        kw.pop("pin_memory", None)
        _plain_kwargs(kw, kind)
        return a.alloc(_shape_of(size), dtype, device, kind, fill)

    def empty(self, *size, **kw):
        return self._make(_torch.empty, "empty", POISON, size, kw)

    def zeros(self, *size, **kw):
        return self._make(_torch.zeros, "zeros", 0, size, kw)

    def empty_like(self, t, **kw):
        a = self._arena
        device = kw.get("device", None)
        device = t.device if device is None else device
        if a.is_host(device, kw.get("pin_memory", False)):
            return _torch.empty_like(t, **kw)
        kw = dict(kw)
        kw.pop("device", None)
        dtype = kw.pop("dtype", None) or t.dtype
        kw.pop("pin_memory", None)
        _plain_kwargs(kw, "empty_like")
        if not t.is_contiguous():
            raise NotImplementedError("fenced empty_like of a non-contiguous tensor")
        return a.alloc(t.shape, dtype, device, "empty", POISON)


@contextlib.contextmanager
def fenced(*modules, fence_cpu=False):
    """Fence and poison what `modules` allocate for the length of the block (see the module docstring).  Eager only: no hipGraph
    capture inside the block."""
    arena = Arena(fence_cpu=fence_cpu)
    proxy = TorchProxy(arena)
    saved = []
    try:
        for m in modules:
            d = vars(m)
            if d.get("torch") is not _torch:
                raise RuntimeError("%s has no module-global torch to fence" % m.__name__)
            saved.append((m, "torch", d["torch"]))
            m.torch = proxy
            real_zb = d.get("zeros_bytes")
            if real_zb is not None:
                saved.append((m, "zeros_bytes", real_zb))

                def zeros_bytes(nbytes, device, _real=real_zb):
                    if arena.is_host(device):
                        return _real(nbytes, device)
                    return arena.alloc((int(nbytes),), _torch.uint8, device, "counter", 0)
                m.zeros_bytes = zeros_bytes
        yield arena
    finally:
        for m, name, obj in reversed(saved):
            setattr(m, name, obj)
