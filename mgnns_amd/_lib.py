"""ctypes binding of libmgnns_hip.so, derived from include/mgnns_hip.h and its extension headers.

The header is the one place an entry point's signature is written down: the compiler checks every definition against it (each
.hip includes it), and this module parses it at import into the argtypes, restypes and integer constants of the binding.

The library is required: there is no CPU or PyTorch fallback for any operator.  `lib()`
raises if the shared object has not been built (python -m mgnns_amd.build).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGNNS_LIB") or os.path.join(_HERE, "libmgnns_hip.so")   # MGNNS_LIB: an instrumented build (tools/)
HEADER_PATH = os.path.join(_HERE, "..", "include", "mgnns_hip.h")
# Extension headers: entry points added without an ABI bump are declared beside mgnns_hip.h, which stays the surface of the ABI as it
# stood.  They are parsed by the same rules into tables of their own (EXTENSION_SIGNATURES / EXTENSION_SIZE_GETTERS).
EXTENSION_HEADERS = (os.path.join(_HERE, "..", "include", "mgnns_jpeg_progressive.h"),)
# ... and so are the headers added after those tables were pinned down: tables of their own again (SPLIT_SIGNATURES).
SPLIT_HEADERS = (os.path.join(_HERE, "..", "include", "mgnns_jpeg_split.h"),)
# ... and the JPEG files of other component layouts (LAYOUT_SIGNATURES)
LAYOUT_HEADERS = (os.path.join(_HERE, "..", "include", "mgnns_jpeg_layouts.h"),)
# ... and the tail of a training step: loss, gradient norm, Adam (STEP_SIGNATURES, STEP_SIZE_GETTERS, STEP_CONSTANTS)
STEP_HEADERS = (os.path.join(_HERE, "..", "include", "mgnns_step.h"),)


class MgnnsLibraryError(RuntimeError):
    pass


# The closed type map: a header type outside it raises, it never binds silently.  Any single pointer is an address (callers pass
# data_ptr() ints or None); a pointer to pointers takes a (c_void_p * n) array or a byref(handle).
_HANDLES = ("mgnns_stream_t", "mgnns_comm_t")
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64,
            "long long": ctypes.c_longlong, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "mgnns_stream_t": ctypes.c_void_p, "mgnns_comm_t": ctypes.c_void_p}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_PP = ctypes.POINTER(ctypes.c_void_p)


def _ctype(param, decl, where):
    """One (named) parameter of a declaration -> its ctypes class."""
    tok = [t for t in re.findall(r"\w+|\*|\S", param) if t != "const"]
    if len(tok) > 1 and tok[-1] != "*":
        tok.pop()                                        # the parameter's name
    depth = tok.count("*") + (1 if tok and tok[0] in _HANDLES else 0)
    base = " ".join(t for t in tok if t != "*")
    if not re.fullmatch(r"[A-Za-z_]\w*( [A-Za-z_]\w*)*", base) or depth > 2 or (depth == 0 and base not in _SCALARS):
        raise MgnnsLibraryError("%s: no ctypes mapping for the parameter '%s' of '%s'" % (where, param.strip(), decl))
    return _SCALARS[base] if "*" not in tok else ctypes.c_void_p if depth == 1 else _PP


def parse_header(text, where="the header"):
    """-> ({name: (restype, [argtypes])} for every `<ret> mgnns_<name>(<params>);`, {MGNNS_<NAME>: int} for every integer #define)."""
    text = re.sub(r"/\*.*?\*/", " ", text.replace("\\\n", " "), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    define = r"^[ \t]*#[ \t]*define[ \t]+(MGNNS_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$"
    constants = {n: int(v) for n, v in re.findall(define, text, flags=re.M)}
    decls = {}
    for stmt in re.split(r"[;{}]", re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)):
        if "(" not in stmt:
            continue                                     # typedefs, `extern "C"`
        decl = " ".join(stmt.split())
        m = re.fullmatch(r"(.+?)\s*\b(mgnns_\w+)\s*\(([^()]*)\)", decl)
        if m is None:
            raise MgnnsLibraryError("%s: cannot parse the declaration '%s'" % (where, decl))
        ret, name, params = re.sub(r"\s*\*", "*", m.group(1)), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise MgnnsLibraryError("%s: no ctypes mapping for the return type '%s' of '%s'" % (where, ret, decl))
        decls[name] = (_RETURNS[ret], [] if params == "void" else [_ctype(p, decl, where) for p in params.split(",")])
    return decls, constants


def _read_header(path):
    try:
        with open(path) as f:
            decls, constants = parse_header(f.read(), path)
    except OSError as e:
        raise MgnnsLibraryError("cannot read the C header %s (%s): the binding is derived from it" % (path, e))
    if not decls or "MGNNS_ABI_VERSION" not in constants:
        raise MgnnsLibraryError("%s declares no mgnns_* entry point or no MGNNS_ABI_VERSION" % path)
    return decls, constants


_DECLS, CONSTANTS = _read_header(HEADER_PATH)
ABI_VERSION = CONSTANTS["MGNNS_ABI_VERSION"]
_UNCHECKED = ("mgnns_last_error", "mgnns_abi_version", "mgnns_source_fingerprint")       # bound first: lib() needs them for its own checks
# name -> argtypes, in the order of include/mgnns_hip.h: the int-returning entry points and the size_t-returning helpers
# (buffer sizes the caller allocates)
SIGNATURES = {n: a for n, (r, a) in _DECLS.items() if r is ctypes.c_int and n not in _UNCHECKED}
SIZE_GETTERS = {n: a for n, (r, a) in _DECLS.items() if r is ctypes.c_size_t}


def _read_extensions(paths, base, constants=None):
    """{name: (restype, [argtypes])} of the extension headers; a name mgnns_hip.h or another extension declares is an error.
    The headers' integer #defines are added to `constants` if one is given."""
    out = {}
    for path in paths:
        try:
            with open(path) as f:
                decls, defines = parse_header(f.read(), path)
        except OSError as e:
            raise MgnnsLibraryError("cannot read the C header %s (%s): the binding is derived from it" % (path, e))
        if not decls:
            raise MgnnsLibraryError("%s declares no mgnns_* entry point" % path)
        for n in decls:
            if n in base or n in out:
                raise MgnnsLibraryError("%s declares %s a second time" % (path, n))
        out.update(decls)
        if constants is not None:
            constants.update(defines)
    return out


_EXT_DECLS = _read_extensions(EXTENSION_HEADERS, _DECLS)
EXTENSION_SIGNATURES = {n: a for n, (r, a) in _EXT_DECLS.items() if r is ctypes.c_int}
EXTENSION_SIZE_GETTERS = {n: a for n, (r, a) in _EXT_DECLS.items() if r is ctypes.c_size_t}
_SPLIT_DECLS = _read_extensions(SPLIT_HEADERS, {**_DECLS, **_EXT_DECLS})
SPLIT_SIGNATURES = {n: a for n, (r, a) in _SPLIT_DECLS.items() if r is ctypes.c_int}
SPLIT_SIZE_GETTERS = {n: a for n, (r, a) in _SPLIT_DECLS.items() if r is ctypes.c_size_t}
_LAYOUT_DECLS = _read_extensions(LAYOUT_HEADERS, {**_DECLS, **_EXT_DECLS, **_SPLIT_DECLS})
LAYOUT_SIGNATURES = {n: a for n, (r, a) in _LAYOUT_DECLS.items() if r is ctypes.c_int}
LAYOUT_SIZE_GETTERS = {n: a for n, (r, a) in _LAYOUT_DECLS.items() if r is ctypes.c_size_t}
STEP_CONSTANTS = {}          # the #defines of include/mgnns_step.h (CONSTANTS stays what mgnns_hip.h defines)
_STEP_DECLS = _read_extensions(STEP_HEADERS, {**_DECLS, **_EXT_DECLS, **_SPLIT_DECLS, **_LAYOUT_DECLS}, STEP_CONSTANTS)
STEP_SIGNATURES = {n: a for n, (r, a) in _STEP_DECLS.items() if r is ctypes.c_int}
STEP_SIZE_GETTERS = {n: a for n, (r, a) in _STEP_DECLS.items() if r is ctypes.c_size_t}

_lib = None
_bound = {}          # name -> bound function: call() does no getattr on the CDLL per launch


def _bind(L, name):
    fn = getattr(L, name)          # AttributeError if the symbol is missing
    for decls in (_DECLS, _EXT_DECLS, _SPLIT_DECLS, _LAYOUT_DECLS, _STEP_DECLS):
        if name in decls:
            fn.restype, fn.argtypes = decls[name]
            return
    raise MgnnsLibraryError("no header declares %s" % name)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MgnnsLibraryError(
            "%s is missing: the HIP extension is mandatory (no CPU/PyTorch fallback exists). "
            "Build it with `python -m mgnns_amd.build`." % LIB_PATH)
    import torch  # noqa: F401  -- loads libamdhip64 first so the kernels share PyTorch's HIP runtime
    L = ctypes.CDLL(LIB_PATH)
    for name in _UNCHECKED:
        _bind(L, name)
    if L.mgnns_abi_version() != ABI_VERSION:
        raise MgnnsLibraryError("libmgnns_hip.so ABI %d != binding ABI %d; rebuild" % (L.mgnns_abi_version(), ABI_VERSION))
    for name in list(_DECLS) + list(_EXT_DECLS) + list(_SPLIT_DECLS) + list(_LAYOUT_DECLS) + list(_STEP_DECLS):
        _bind(L, name)
    _lib = L
    _register_status_word(L)
    return L


def call(name, *args):
    """Call the int-returning entry point `name`; raise on a non-zero return."""
    fn = _bound.get(name)
    if fn is None:
        fn = _bound[name] = getattr(lib(), name)
    rc = fn(*args)
    if rc != 0:
        check(rc, name)


def source_state():
    """(fingerprint compiled into the loaded library, fingerprint of the sources next to it, equal?) -- mgnns_amd/build.py."""
    from . import build
    built, tree = lib().mgnns_source_fingerprint().decode(), build.source_fingerprint()
    return built, tree, built == tree


def check_sources(who="this measurement"):
    """Raise unless the loaded library was built from exactly the sources in the tree (an instrumented MGNNS_LIB build is named
    as such by the caller): a profile must not be filed under sources newer than the kernels that ran."""
    built, tree, same = source_state()
    if not same:
        raise MgnnsLibraryError("%s: %s was built from sources %s, the tree holds %s -- rebuild (python -m mgnns_amd.build) first"
                                % (who, LIB_PATH, built, tree))
    return built


_status_word = None


def _register_status_word(L):
    """Hand the library 4 bytes of host-pinned memory for the status of its persistent launches (include/mgnns_hip.h):
    a bounded wait that runs out is then REPORTED by the next such launch instead of being lost.  Needs a GPU."""
    global _status_word
    import torch
    if _status_word is not None or not torch.cuda.is_available():
        return
    try:
        w = torch.zeros(16, dtype=torch.int32).pin_memory()
    except RuntimeError:
        return
    L.mgnns_set_status_word(w.data_ptr())
    _status_word = w                     # keeps the allocation alive for the life of the process


def xcd_probe():
    """-> (ok, [XCC_ID seen for block indices b & 7 == k]): whether `blockIdx.x & 7` selects the XCD here (the placement several
    kernels use for SPEED; HIP promises nothing).  Synchronises the device: a set-up time measurement."""
    out = (ctypes.c_int32 * 9)()
    call("mgnns_xcd_probe", ctypes.addressof(out))
    return bool(out[0]), [int(out[1 + k]) for k in range(8)]


def take_status():
    """Read-and-clear the persistent launches' status word (0 = fine); raise if it is set.  Meaningful after a stream
    synchronise; the next persistent launch reports a raised word on its own."""
    code = lib().mgnns_take_status()
    if code:
        raise RuntimeError("a launch raised the library status word (status %d: %d / %d = a persistent launch gave up a bounded wait, "
                           "%d = a masked attention launch refused its plan): results since then are invalid"
                           % (code, CONSTANTS["MGNNS_STATUS_LABEL_GCN_TIMEOUT"], CONSTANTS["MGNNS_STATUS_CLUSTER_TIMEOUT"],
                              CONSTANTS["MGNNS_STATUS_BAD_PLAN"]))


def check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (name, rc, lib().mgnns_last_error().decode()))
