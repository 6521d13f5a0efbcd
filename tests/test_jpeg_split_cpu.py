"""Split scans without a GPU ("Split scans"): the chunk walks the GPU lanes run (csrc/jpeg_entropy.hpp, csrc/jpeg_split.hpp),
built for the CPU as tools/dev/jpeg_split_host_check.cpp, give the serial decoder's coefficient workspace and status word byte for
byte -- the program compares them itself on every input and exits non-zero on a difference -- for every baseline fixture, sound or
corrupt, at every chunk size and lane count, whatever the speculative start state; accepted files give Pillow's recorded pixels
(tests/golden/jpeg_decode.npz, tests/golden/jpeg_split.npz) and live Pillow's.  Then the binding of the new entry point and the
host side of ImagePrep(split=...)."""
import io
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mgnns_amd import images as I, ops
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = "8,16,24,64,256,1048576"
LANES = "4,1024"
LINE = re.compile(r"chunk (\d+), (\d+) lanes: reason (\d+), worst status (\d+), (\d+)x(\d+), (\d+) split, (\d+) chunks, (\d+) rounds, (\d+) grown, "
                  r"(\d+) in a pair(, pixels equal)?")


@pytest.fixture(autouse=True)
def rng_left_as_found():
    state = random.getstate(), torch.get_rng_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])


@pytest.fixture(scope="module")
def gold():
    g = dict(H.load_golden("jpeg_decode.npz"))
    s = H.load_golden("jpeg_split.npz")
    assert len(s["accepted"]) == 4 and str(s["versions"][0]).startswith("Pillow")
    for k in s:
        if k.startswith(("file_", "pix_")):
            g["split_" + k] = s[k]
    g["split_accepted"] = s["accepted"]
    return g


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("split") / "check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "dev", "jpeg_split_host_check.cpp"), "-o", out], check=True)
    return out


def inputs(gold):
    """(name, file bytes, golden pixels or None, recorded status) of every baseline fixture the parser accepts"""
    out = [(n, gold["file_" + n], gold["pix_" + n], 0) for n in gold["accepted"]]
    out += [(n, gold["file_" + n], None, int(s)) for n, s in zip(gold["corrupt"], gold["corrupt_status"])]
    out += [("split_" + n, gold["split_file_" + n], gold["split_pix_" + n], 0) for n in gold["split_accepted"]]
    return out


def run(exe, tmp_path, name, data, pixels, *args):
    """-> one dict per chunk size x lane count; the program has compared coefficients and status with the serial decoder's"""
    f = str(tmp_path / (name + ".jpg"))
    with open(f, "wb") as o:
        o.write(bytes(data))
    cmd = [exe, f]
    if pixels is not None:
        with open(f[:-4] + ".rgb", "wb") as o:
            o.write(pixels.tobytes())
        cmd.append(f[:-4] + ".rgb")
    r = subprocess.run(cmd + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, (name, r.stdout)
    keys = ("chunk", "lanes", "reason", "status", "w", "h", "split", "chunks", "rounds", "grown", "in_pair")
    rows = [dict(zip(keys, (int(v) for v in m.groups()[:-1])), pixels=m.group(12) is not None) for m in LINE.finditer(r.stdout)]
    assert rows and "inputs equal to the serial decoder" in r.stdout, r.stdout
    return rows


def check_rows(rows, name, pixels, status, combos=12):
    assert len(rows) == combos, name
    for row in rows:
        assert row["reason"] == 0 and row["status"] == status, (name, row)
        assert row["pixels"] == (pixels is not None), (name, row)
        assert row["rounds"] <= row["chunks"] and row["chunks"] <= row["lanes"], (name, row)        # bounded by the chunks; a lane per chunk


def test_equivalence_on_every_fixture(gold, exe, tmp_path):
    assert [int(s) for s in gold["corrupt_status"]] == [1, 1, 2]
    split_somewhere = set()
    for name, data, pixels, status in inputs(gold):
        rows = run(exe, tmp_path, name, data, pixels, "--chunks", CHUNKS, "--lanes", LANES)
        check_rows(rows, name, pixels, status)
        for row in rows:
            assert row["chunk"] < 1 << 20 or row["split"] == 0, (name, row)              # no fixture is two such chunks long: the serial route
            if row["split"]:
                split_somewhere.add(name)
    assert len(split_somewhere) >= 20 and "one_pixel" not in split_somewhere                # one_pixel's scan is below 16 bytes


def test_the_result_does_not_depend_on_the_guess(gold, exe, tmp_path):
    worst = 0
    for name, data, pixels, status in inputs(gold):
        for guess in (("1", "5"), ("2", "63")):
            rows = run(exe, tmp_path, name, data, pixels, "--chunks", CHUNKS, "--lanes", LANES, "--guess", *guess)
            check_rows(rows, name, pixels, status)
            worst = max(worst, max(r["rounds"] for r in rows))
    print("most rounds with a wrong guess: %d" % worst)
    assert worst >= 2                                                                        # (the guesses were wrong somewhere)


def pair_boundaries(data, chunk, lanes):
    """chunk boundaries of the file's one segment that fall on the 00 of a stuffed FF 00, by the geometry of csrc/jpeg_split.hpp:
    boundaries at multiples of the chunk size counted from the 8-byte boundary at or before the segment's first byte (files sit on
    16-byte boundaries), the chunk grown to a multiple of 8 if there would be more chunks than lanes -> (boundaries, chunks, chunk)"""
    p = I.parse_jpeg(bytes(data))
    assert p["reason"] == 0 and p["nseg"] == 1
    b, e = (int(v) for v in p["segments"][0])
    lead, n = b & 7, e - b
    if n < 2 * chunk:
        return [], 1, chunk
    if (lead + n + chunk - 1) // chunk > lanes:
        chunk = ((lead + n + lanes - 1) // lanes + 7) // 8 * 8
    chunks = (lead + n + chunk - 1) // chunk
    seg = bytes(data[b:e])
    at = [t * chunk - lead for t in range(1, chunks)]
    return [a for a in at if a < n and seg[a - 1] == 0xFF and seg[a] == 0], chunks, chunk


def test_chunk_growth_and_a_boundary_inside_a_stuffed_pair(gold, exe, tmp_path):
    noise = gold["split_file_noise_s0_q100"]
    found, chunks, chunk = pair_boundaries(noise, 8, 1024)
    assert chunks <= 1024 and chunk > 8                                  # above 8 KB: more 8-byte chunks than lanes, the chunk grew
    rows = run(exe, tmp_path, "noise", noise, gold["split_pix_noise_s0_q100"], "--chunks", "8", "--lanes", "1024")
    check_rows(rows, "noise", True, 0, combos=1)
    assert rows[0]["grown"] == 1 and rows[0]["chunks"] == chunks and rows[0]["in_pair"] == len(found)
    # a boundary between FF and its stuffed 00: search the restart-free fixtures and the chunk sizes
    hits = []
    for name, data, pixels, status in inputs(gold):
        if I.parse_jpeg(bytes(data))["nseg"] != 1:
            continue
        for c in (8, 16, 24, 64, 256):
            at, chunks, _ = pair_boundaries(data, c, 1024)
            if at:
                hits.append((name, c, len(at), chunks, data, pixels, status))
    assert hits, "no fixture has a chunk boundary inside a stuffed pair"
    for name, c, count, chunks, data, pixels, status in hits[:6]:
        rows = run(exe, tmp_path, name, data, pixels, "--chunks", str(c), "--lanes", "1024")
        check_rows(rows, name, pixels, status, combos=1)
        assert rows[0]["in_pair"] == count and rows[0]["chunks"] == chunks, (name, c, rows)


def test_live_pillow(exe, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(41)
    split = 0
    for k in range(24):
        w, h = (int(v) for v in rs.randint(8, 97, 2))
        if k % 2:
            a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            a = np.clip(np.linspace(0, 255, w)[None, :, None] + rs.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
        opts = dict(quality=int(rs.randint(30, 101)), optimize=bool(k % 3 == 0))
        if k % 4 == 3:
            a = a[:, :, 0]                                                   # grayscale
        else:
            opts["subsampling"] = k % 4
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", **opts)
        pixels = np.asarray(Image.open(buf).convert("RGB"))
        rows = run(exe, tmp_path, "live%d" % k, buf.getvalue(), pixels, "--chunks", "8,64", "--lanes", "1024")
        check_rows(rows, (w, h, opts), pixels, 0, combos=2)
        split += sum(r["split"] for r in rows)
    assert split >= 40


def test_the_new_entry_point_is_derived_from_its_header():
    import ctypes
    from mgnns_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mgnns_jpeg_split.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = {n: len(p.split(",")) for n, p in re.findall(r"\b(mgnns_\w+)\s*\(([^()]*)\)\s*;", code)}
    assert declared == {"mgnns_jpeg_decode_split_fwd": 27}
    V, I32, SZ, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong
    assert _lib.SPLIT_SIGNATURES == {"mgnns_jpeg_decode_split_fwd": _lib.EXTENSION_SIGNATURES["mgnns_jpeg_decode_progressive_fwd"] + [I32]}
    assert _lib.SPLIT_SIGNATURES["mgnns_jpeg_decode_split_fwd"] == [V, SZ, V, I32, V, I32, V, I32, V, V, I32, V, I32, V, I32, V, SZ, V, SZ, V, SZ, LL, LL,
                                                                   I32, V, V, I32]
    assert _lib.SPLIT_SIZE_GETTERS == {}
    # the pinned tables are as they were
    assert set(_lib.EXTENSION_SIGNATURES) == {"mgnns_jpeg_parse_progressive", "mgnns_jpeg_decode_progressive_fwd"}
    assert _lib.EXTENSION_SIZE_GETTERS == {"mgnns_jpeg_huff_bytes": []}
    assert "mgnns_jpeg_decode_split_fwd" not in _lib.SIGNATURES and _lib.ABI_VERSION == 26
    assert len(_lib.EXTENSION_HEADERS) == 1 and len(_lib.SPLIT_HEADERS) == 1
    L = _lib.lib()
    fn = L.mgnns_jpeg_decode_split_fwd
    assert list(fn.argtypes) == _lib.SPLIT_SIGNATURES["mgnns_jpeg_decode_split_fwd"] and fn.restype is ctypes.c_int
    with pytest.raises(_lib.MgnnsLibraryError, match="a second time"):                     # against everything declared before
        _lib._read_extensions(_lib.SPLIT_HEADERS, {"mgnns_jpeg_decode_split_fwd": None})
    # the entry point checks its own argument before anything else (no GPU call)
    with pytest.raises(RuntimeError, match="chunk_bytes=12 is no multiple of 8"):
        _lib.call("mgnns_jpeg_decode_split_fwd", None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, 1, 1,
                  7, None, None, 12)


def test_host_side_of_the_switch(gold):
    assert I.ImagePrep(size=16, device=None).split == 0 and I.ImagePrep(size=16, device=None, split=False).split == 0
    assert I.ImagePrep(size=16, device=None, split=True).split == ops.JPEG_SPLIT_CHUNK and ops.JPEG_SPLIT_CHUNK % 8 == 0
    assert I.ImagePrep(size=16, device=None, split=64).split == 64 and I.ImagePrep(size=16, device=None, split=65536).split == 65536
    for bad in (4, 12, -8, 65544, 8.0, "64"):
        with pytest.raises(ValueError, match="split must be"):
            I.ImagePrep(size=16, device=None, split=bad)
    for bad in (0, 4, 12, 65544, True, 8.0):
        with pytest.raises(ValueError, match="chunk_bytes must be"):
            ops.jpeg_decode_split(*([None] * 12), chunk_bytes=bad)
    prep = I.ImagePrep(size=16, device=None, split=True)
    files = [bytes(gold["file_s0_q90"]), bytes(gold["split_file_gray"])]
    with pytest.raises(RuntimeError, match="GPU only"):
        prep.decode_jpeg(files)
    with pytest.raises(I.UnsupportedJpeg) as e:                               # split alone does not accept progressive files
        prep.decode_jpeg(files + [bytes(gold["file_progressive"])])
    assert e.value.refused == [(2, 3)]
    import inspect
    from mgnns_amd import model
    sig = inspect.signature(model.Multi_GCN_Multihead_Att.image_prep)
    assert sig.parameters["split"].default == 0 and sig.parameters["progressive"].default is False
