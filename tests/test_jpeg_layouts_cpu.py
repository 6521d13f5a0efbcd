"""Other component layouts without a GPU ("Other component layouts"): the numpy restatement tests/jpeg_layouts_ref.py
equals Pillow's recorded pixels (tests/golden/jpeg_layouts.npz) and live Pillow's on seeded random files of every layout; the
library's parser (mgnns_jpeg_parse_layout behind images.parse_jpeg(..., layouts=True)) equals the restatement on every fixture and
on every truncation of two headers; with the switch off every fixture is refused exactly as before; the binding tables; the host
side of the switch; and the functions the GPU kernels run, built for the CPU as tools/dev/jpeg_layouts_host_check.cpp, give the
golden pixels and the recorded statuses."""
import inspect
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
from tests import jpeg_layouts_ref as L
from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S440, S411, S1X4 = [(1, 2), (1, 1), (1, 1)], [(4, 1), (1, 1), (1, 1)], [(1, 4), (1, 1), (1, 1)]


@pytest.fixture(autouse=True)
def rng_left_as_found():
    state = random.getstate(), torch.get_rng_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])


@pytest.fixture(scope="module")
def gold():
    g = H.load_golden("jpeg_layouts.npz")
    assert len(g["accepted"]) == 29 and len(g["refused"]) == 6 and len(g["corrupt"]) == 2
    assert str(g["versions"][0]).startswith("Pillow") and str(g["versions"][1]).startswith("libjpeg-turbo")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_layouts.npz")) < 100 * 1024
    return g


def every_file(gold):
    return [str(n) for n in list(gold["accepted"]) + list(gold["refused"]) + list(gold["corrupt"])]


def same_parse(got, want, name):
    """images.parse_jpeg's dictionary against the restatement's"""
    assert got["reason"] == want["reason"], (name, got, want.get("detail"))
    if want["reason"] != L.OK:
        if want["reason"] != L.MALFORMED:                  # (the detail of a malformed file is an offset: the two parsers' own business)
            assert got["detail"] == want.get("detail", 0), (name, got, want)
        return
    assert bool(got.get("layout")) == bool(want.get("layout")), name
    keys = ("width", "height", "ncomp", "hmax", "vmax", "h", "v", "tq", "td", "ta", "ri", "mcux", "mcuy", "colour", "sof", "mcu_blocks") \
        if want.get("layout") else ("width", "height", "ncomp", "hs", "vs", "tq", "td", "ta", "ri", "mcux", "mcuy")
    for k in keys:
        assert got[k] == want[k] or (k in ("tq", "td", "ta") and got[k][:want["ncomp"]] == want[k]), (name, k, got[k], want[k])
    assert got["ecs"] == (want["ecs_begin"], want["ecs_end"]) and got["restarts"] == want["restarts_found"], name
    assert got["segments"].tolist() == [list(s) for s in want["segments"]], name


def test_the_restatement_gives_the_golden_pixels(gold):
    seen = set()
    for name in gold["accepted"]:
        data = bytes(gold["file_" + name])
        assert L.routed(R.parse(data)["reason"], R.parse(data).get("detail", 0)), name         # the baseline parser refuses it
        p = L.parse(data)
        assert p["reason"] == L.OK, (name, p)
        got, status = L.decode(data)
        assert not any(status) and np.array_equal(got, gold["pix_" + name]), name
        seen.add((p["colour"], tuple(zip(p["h"], p["v"]))))
    assert {c for c, _ in seen} == {L.GRAY, L.YCC, L.RGB, L.CMYK, L.YCCK}
    assert {(L.YCC, tuple(S440)), (L.YCC, tuple(S411)), (L.YCC, tuple(S1X4)), (L.YCC, ((1, 1), (2, 1), (1, 1))),
            (L.YCC, ((2, 1), (1, 2), (2, 1))), (L.CMYK, ((2, 2), (1, 1), (1, 1), (1, 1)))} <= seen
    # a gray file labelled 2x2 is the file labelled 1x1
    g = bytearray(gold["file_gray_2x2"])
    at = _seg(g, 0xC0) + 11
    assert g[at] == 0x22
    g[at] = 0x11
    assert np.array_equal(R.decode(bytes(g))[0], gold["pix_gray_2x2"])
    # the corrupt files: their statuses, and the restart-per-row file's three segments
    assert [max(L.decode(bytes(gold["file_" + n]))[1]) for n in gold["corrupt"]] == gold["corrupt_status"].tolist() == [1, 2]
    assert len(L.parse(bytes(gold["file_s440_rst"]))["segments"]) == 3


def _seg(data, marker):
    """offset of the FF of the first segment with this marker, walking the segments"""
    pos = 2
    while data[pos + 1] != marker:
        assert data[pos] == 0xFF and data[pos + 1] != 0xDA, marker
        pos += 2 + (data[pos + 2] << 8 | data[pos + 3])
    return pos


def _relabel(data, w, h, samp):
    d = bytearray(data)
    pos = _seg(d, 0xC0)
    d[pos + 5:pos + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
    for i, (a, b) in enumerate(samp):
        d[pos + 11 + 3 * i] = a << 4 | b
    return bytes(d)


def _cut(data, marker):
    pos = _seg(data, marker)
    return data[:pos] + data[pos + 2 + (data[pos + 2] << 8 | data[pos + 3]):]


def live_files(count, seed):
    """seeded random files of every layout, made as tools/gen_jpeg_layouts_goldens.py makes the fixtures: (what, bytes)"""
    from PIL import Image
    rs = np.random.RandomState(seed)

    def save(a, mode=None, **o):
        buf = io.BytesIO()
        Image.fromarray(a, mode).save(buf, "JPEG", quality=int(rs.randint(30, 101)), **o)
        return buf.getvalue()

    def pic(w, h, ch=3):
        if rs.randint(2):
            return rs.randint(0, 256, (h, w, ch)).astype(np.uint8)
        return np.clip(np.linspace(0, 255, w)[None, :, None] + rs.normal(0, 20, (h, w, ch)), 0, 255).astype(np.uint8)

    out = []
    for k in range(count):
        kind = k % 10
        w, h = (int(v) for v in rs.randint(1, 71, 2))
        if k % 3 == 0:
            w = 1 + (k // 3) % 5                                               # widths 1..5
        rst = {} if k % 3 != 1 else dict(restart_marker_rows=1) if k % 2 else dict(restart_marker_blocks=int(rs.randint(1, 5)))
        if kind < 5:                                                           # relabelled: same MCU grid, same blocks per MCU
            # (Only layouts whose every block keeps the Huffman tables it was coded with: luma alone relabelled, or a CMYK file, whose
            # four components share one table pair.  A block read with another table is a corrupt stream, which libjpeg shrugs off
            # and this decoder reports; the goldens cb2x1 and y2x1_cb1x2_cr2x1 happen to decode cleanly.)
            samp, (sub, mw, mh) = [(S440, (1, 8, 16)), (S411, (2, 32, 8)), (S1X4, (2, 8, 32)), ([(2, 1), (1, 2), (2, 1), (1, 1)], (2, 16, 16)),
                                   ([(1, 1), (2, 2), (1, 1), (1, 1)], (2, 16, 16))][kind]
            mx, my = -(-w // mw), -(-h // mh)
            sw, sh = mx * (16 if sub else 8), my * (16 if sub == 2 else 8)
            if kind < 3:
                src = save(pic(sw, sh), subsampling=sub, optimize=bool(k % 4 == 1), **rst)
            else:
                src = save(pic(sw, sh, 4), "CMYK", subsampling=2, **rst)
                if k % 4 == 0:
                    src = _cut(src, 0xEE)
            out.append((("relabel", samp, w, h, rst), _relabel(src, w, h, samp)))
        elif kind < 8:                                                         # CMYK, YCCK, CMYK without the Adobe segment
            c = save(pic(w, h, 4), "CMYK", subsampling=(0, 2, 1)[kind - 5], **rst)
            if kind == 6:
                c = bytearray(c)
                c[_seg(c, 0xEE) + 15] = 2                                      # the transform byte: YCCK
                c = bytes(c)
            elif kind == 7:
                c = _cut(c, 0xEE)
            out.append((("cmyk", kind, w, h, rst), c))
        elif kind == 8:
            c = save(pic(w, h), keep_rgb=True, **rst)
            if k % 3 == 1:
                c = _cut(c, 0xEE)                                              # ids R G B alone
            elif k % 3 == 2:                                                   # ids 1 2 3 under the Adobe segment
                c = bytearray(c)
                sof, sos = _seg(c, 0xC0), _seg(c, 0xDA)
                for i in range(3):
                    c[sof + 10 + 3 * i] = c[sos + 5 + 2 * i] = i + 1
                c = bytes(c)
            out.append((("rgb", k % 3, w, h, rst), c))
        else:
            c = bytearray(save(pic(w, h), subsampling=k % 3, **rst))
            c[_seg(c, 0xC0) + 1] = 0xC1                                        # SOF1
            out.append((("sof1", k % 3, w, h, rst), bytes(c)))
    return out


def test_the_restatement_against_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    files = live_files(50, 1234)
    assert len(files) >= 40 and {f[0][0] for f in files} == {"relabel", "cmyk", "rgb", "sof1"}
    assert {f[0][2] for f in files if f[0][0] == "relabel"} >= {1, 2, 3, 4, 5}
    for what, data in files:
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        p = L.parse_routed(data)
        assert p["reason"] == L.OK and p.get("layout"), (what, p)
        got, status = L.decode(data)
        assert not any(status) and np.array_equal(got, want), what
    # Pillow decides where the rules are in doubt: every Adobe transform but 0 on four components is YCCK, and on three YCbCr
    cmyk = [d for w, d in files if w[0] == "cmyk" and w[1] == 5][0]
    rgb = [d for w, d in files if w[0] == "rgb" and w[1] == 0][0]
    for data, transform, colour in ((cmyk, 1, L.YCCK), (cmyk, 3, L.YCCK), (cmyk, 255, L.YCCK), (rgb, 1, L.YCC), (rgb, 2, L.YCC)):
        d = bytearray(data)
        d[_seg(d, 0xEE) + 15] = transform
        want = np.asarray(Image.open(io.BytesIO(bytes(d))).convert("RGB"))
        assert np.array_equal(L.decode(bytes(d))[0], want) and I.parse_jpeg(bytes(d), layouts=True)["colour"] == colour, (transform, colour)


def test_the_librarys_parser_equals_the_restatement(gold):
    for name in every_file(gold):
        data = bytes(gold["file_" + name])
        same_parse(I.parse_jpeg(data, layouts=True), L.parse_routed(data), name)
        same_parse(I._parse_layout(np.frombuffer(data, np.uint8), None), L.parse(data), name)
    # every truncation of two headers (and a little of their scans)
    for name in ("cmyk_s2", "s440_rst"):
        data = bytes(gold["file_" + name])
        stop = data.index(b"\xff\xda") + 40
        for n in range(stop):
            same_parse(I.parse_jpeg(data[:n], layouts=True), L.parse_routed(data[:n]), (name, n))
    # the baseline goldens keep the baseline parser's dictionary
    base = H.load_golden("jpeg_decode.npz")
    for name in base["accepted"]:
        data = bytes(base["file_" + name])
        on, off = I.parse_jpeg(data, layouts=True), I.parse_jpeg(data)
        assert "layout" not in on and set(on) == set(off) and all(np.array_equal(on[k], off[k]) for k in on), name


def test_reasons_17_and_18(gold):
    want = dict(zip((str(n) for n in gold["refused"]), gold["refused_reason"].tolist()))
    assert want == {"frac_3x1_2x1_1x1": 17, "factor_5x1": 18, "blocks_14": 18, "two_components": 6, "cmyk_progressive": 3, "two_scans": 10}
    details = {"frac_3x1_2x1_1x1": 0x21, "factor_5x1": 0x51, "blocks_14": 14, "two_components": 2, "cmyk_progressive": 0xC2, "two_scans": 2}
    for name, reason in want.items():
        p = I.parse_jpeg(bytes(gold["file_" + name]), layouts=True)
        assert (p["reason"], p["detail"]) == (reason, details[name]) and set(p) == {"reason", "detail"}, (name, p)
    assert set(I.JPEG_LAYOUT_REASONS) == {17, 18} and not set(I.JPEG_LAYOUT_REASONS) & (set(I.JPEG_REASONS) | set(I.JPEG_PROGRESSIVE_REASONS))
    # a factor of zero is outside 1..4 as well; ten blocks are accepted, with 4x2 luma
    data = bytes(gold["file_s440_16x32"])
    assert I.parse_jpeg(_relabel(data, 16, 32, [(0, 2), (1, 1), (1, 1)]), layouts=True)["reason"] == 18
    p = I.parse_jpeg(_relabel(data, 16, 32, [(4, 2), (1, 1), (1, 1)]), layouts=True)
    assert p["reason"] == 0 and p["mcu_blocks"] == 10 and (p["mcux"], p["mcuy"]) == (1, 2)
    e = I.UnsupportedJpeg([(0, 17), (3, 18)], [0x21, 14])
    assert "integral fraction" in str(e) and "10 blocks" in str(e) and "reason 17" in str(e)


def test_with_the_switch_off_everything_is_as_it_was(gold):
    assert I.JPEG_REASONS.keys() == set(range(14))
    want = {"s440": 9, "s411": 9, "s1x4": 9, "cb2x1": 9, "y2x1": 9, "cmyk": 6, "ycck": 6, "rgb_adobe": 8, "rgb_ids": 8, "rgb_123": 7, "sof1": 3,
            "gray_2x2": 9, "frac": 9, "factor": 9, "blocks": 9, "two_components": 6, "two_scans": 9, "cmyk_progressive": 3}
    for name in every_file(gold):
        data = bytes(gold["file_" + name])
        off = I.parse_jpeg(data)
        assert off == I.parse_jpeg(data, layouts=False) and set(off) == {"reason", "detail"}, name
        assert off["reason"] == R.parse(data)["reason"], name                   # (jpeg_ref keeps no detail for most reasons)
        key = [k for k in want if name.startswith(k)]
        assert off["reason"] == want[max(key, key=len)], (name, off)
    prep = I.ImagePrep(size=16, device=None)
    assert prep.layouts is False
    with pytest.raises(I.UnsupportedJpeg) as e:
        prep.decode_jpeg([bytes(gold["file_" + n]) for n in gold["accepted"]])
    assert [i for i, _ in e.value.refused] == list(range(29))
    assert list(inspect.signature(I.ImagePrep.__init__).parameters)[-1] == "layouts"
    from mgnns_amd import model
    sig = inspect.signature(model.Multi_GCN_Multihead_Att.image_prep)
    assert list(sig.parameters)[-1] == "layouts" and sig.parameters["layouts"].default is False


def test_the_new_entry_points_are_derived_from_their_header():
    import ctypes
    from mgnns_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mgnns_jpeg_layouts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = {n: len(p.split(",")) for n, p in re.findall(r"\b(mgnns_\w+)\s*\(([^()]*)\)\s*;", code)}
    assert declared == {"mgnns_jpeg_parse_layout": 8, "mgnns_jpeg_decode_layouts_fwd": 31}
    V, I32, SZ, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong
    split = _lib.SPLIT_SIGNATURES["mgnns_jpeg_decode_split_fwd"]
    assert _lib.LAYOUT_SIGNATURES == {"mgnns_jpeg_parse_layout": _lib.SIGNATURES["mgnns_jpeg_parse"],
                                      "mgnns_jpeg_decode_layouts_fwd": split[:15] + [V, I32] + split[15:23] + [LL, LL] + split[23:]}
    assert _lib.LAYOUT_SIZE_GETTERS == {} and len(_lib.LAYOUT_HEADERS) == 1
    # the pinned tables are as they were
    assert set(_lib.EXTENSION_SIGNATURES) == {"mgnns_jpeg_parse_progressive", "mgnns_jpeg_decode_progressive_fwd"}
    assert set(_lib.SPLIT_SIGNATURES) == {"mgnns_jpeg_decode_split_fwd"} and _lib.ABI_VERSION == 26
    assert not set(_lib.LAYOUT_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXTENSION_SIGNATURES) | set(_lib.SPLIT_SIGNATURES))
    lib = _lib.lib()
    for name, args in _lib.LAYOUT_SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int
    with pytest.raises(_lib.MgnnsLibraryError, match="a second time"):
        _lib._read_extensions(_lib.LAYOUT_HEADERS, {"mgnns_jpeg_parse_layout": None})
    # the entry points check their own arguments before anything else (no GPU call)
    with pytest.raises(RuntimeError, match="chunk_bytes=12 is neither 0 nor a multiple of 8"):
        _lib.call("mgnns_jpeg_decode_layouts_fwd", None, 0, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0,
                  None, 0, 1, 1, 1, 1, 7, None, None, 12)
    with pytest.raises(RuntimeError, match="max_extent=0"):
        _lib.call("mgnns_jpeg_parse_layout", None, 0, 0, 1, 1, None, 0, 1)


def test_host_side_of_the_switch(gold):
    prep = I.ImagePrep(size=16, device=None, layouts=True)
    assert prep.layouts is True and prep.progressive is False and prep.split == 0
    files = [bytes(gold["file_" + n]) for n in gold["accepted"]]
    with pytest.raises(RuntimeError, match="GPU only"):                       # every fixture is accepted: the next thing missing is a GPU
        prep.decode_jpeg(files)
    headers = prep._jpeg_headers(files, None)
    assert [(W, H) for W, H in headers[3]] == [gold["pix_" + n].shape[1::-1] for n in gold["accepted"]]
    # refusals are listed before any GPU work, all of them in one exception, with the codes they have
    refused = [bytes(gold["file_" + n]) for n in gold["refused"]]
    with pytest.raises(I.UnsupportedJpeg) as e:
        prep.decode_jpeg(files[:2] + refused + files[2:4])
    assert e.value.refused == [(2 + i, int(r)) for i, r in enumerate(gold["refused_reason"])]
    for text in ("reason 17", "reason 18", "reason 6", "reason 10", "found 194"):
        assert text in str(e.value)
    # ... or go to the fallback, the accepted ones never
    seen = []
    headers = prep._jpeg_headers(files[:1] + refused[:1], lambda f: seen.append(f) or np.zeros((3, 5, 3), np.uint8))
    assert seen == refused[:1] and headers[3] == [(21, 45), (5, 3)]
    for bad in (4, 12, True, 8.0):
        with pytest.raises(ValueError, match="chunk_bytes must be 0 or"):
            ops.jpeg_decode_layouts(*([None] * 14), chunk_bytes=bad)
    assert ops.JPEG_LAYOUT_KIND == 3 and I.JPEG_COLOUR_MODELS == {0: "gray", 1: "YCbCr", 2: "RGB", 3: "CMYK", 4: "YCCK"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = str(tmp_path_factory.mktemp("layouts") / "check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "dev", "jpeg_layouts_host_check.cpp"), "-o", out], check=True)
    return out


LINE = re.compile(r"reason (\d+), detail (\d+), baseline (\d), (\d+)x(\d+), (\d) components (\d)x(\d), colour (\d), (\d+) segments, "
                  r"statuses \[(\d*)\], worst status (\d)(, pixels equal)?")


def run(exe, tmp_path, name, data, pixels, *args):
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
    m = LINE.search(r.stdout)
    assert m, r.stdout
    keys = ("reason", "detail", "baseline", "w", "h", "ncomp", "hmax", "vmax", "colour", "nseg")
    return dict(zip(keys, (int(v) for v in m.groups()[:10])), statuses=[int(c) for c in m.group(11)], worst=int(m.group(12)),
                pixels=m.group(13) is not None, text=r.stdout)


def test_the_kernels_functions_on_the_cpu_give_the_golden_pixels_and_statuses(gold, exe, tmp_path):
    for name in gold["accepted"]:
        data, pix = gold["file_" + name], gold["pix_" + name]
        row = run(exe, tmp_path, name, data, pix)
        p = L.parse(bytes(data))
        assert row["pixels"] and row["reason"] == 0 and row["worst"] == 0 and not row["baseline"], (name, row)
        assert (row["w"], row["h"], row["ncomp"], row["hmax"], row["vmax"], row["colour"], row["nseg"]) == \
            (p["width"], p["height"], p["ncomp"], p["hmax"], p["vmax"], p["colour"], len(p["segments"])), (name, row)
    for name, reason in zip(gold["refused"], gold["refused_reason"]):
        assert run(exe, tmp_path, name, gold["file_" + name], None)["reason"] == reason, name
    for name, status in zip(gold["corrupt"], gold["corrupt_status"]):
        row = run(exe, tmp_path, name, gold["file_" + name], None)
        assert row["reason"] == 0 and row["statuses"] == L.decode(bytes(gold["file_" + name]))[1] and row["worst"] == status, (name, row)
    # every truncation and a few hundred mutations of the smallest file end with a documented reason and status
    row = run(exe, tmp_path, "cut", gold["file_gray_2x2"], gold["pix_gray_2x2"], "--truncate", "--mutations", "300")
    assert "%d inputs" % (1 + gold["file_gray_2x2"].size + 300) in row["text"]
    # a baseline file is the baseline decoder's
    base = H.load_golden("jpeg_decode.npz")
    assert run(exe, tmp_path, "base", base["file_s0_q90"], None)["baseline"] == 1


def test_the_kernels_functions_on_the_cpu_against_live_pillow(exe, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    for k, (what, data) in enumerate(live_files(40, 99)):
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        row = run(exe, tmp_path, "live%d" % k, data, want)
        assert row["pixels"] and not row["baseline"], what
