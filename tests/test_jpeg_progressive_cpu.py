"""The progressive JPEG decoder without a GPU: the numpy restatement tests/jpeg_progressive_ref.py equals Pillow's recorded pixels
(tests/golden/jpeg_progressive.npz, tools/gen_jpeg_progressive_goldens.py) and live Pillow bit for bit; the library's progressive
parser (mgnns_jpeg_parse_progressive through images.parse_jpeg(..., progressive=True) -- it makes no GPU call) agrees with the
restatement's on every fixture; with the switch off every entry point answers as before; the host side of
ImagePrep(progressive=True) refuses what it must; and the C++ decoder body the GPU lanes run (csrc/jpeg_progressive.hpp), built
for the CPU as tools/dev/jpeg_progressive_host_check.cpp, decodes every fixture to its golden pixels."""
import io
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mgnns_amd import images as I, ops
from tests import helpers as H
from tests import jpeg_progressive_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def rng_left_as_found():
    state = random.getstate(), torch.get_rng_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])


@pytest.fixture(scope="module")
def gold():
    return H.load_golden("jpeg_progressive.npz")


@pytest.fixture(scope="module")
def base():
    return H.load_golden("jpeg_decode.npz")


def test_restatement_equals_every_golden(gold):
    assert len(gold["accepted"]) == 20 and str(gold["versions"][0]).startswith("Pillow")
    parsed = {}
    for name in gold["accepted"]:
        data = bytes(gold["file_" + name])
        pix, status, stats = P.decode(data)
        assert {s for _, _, s in status} == {P.SEG_OK}, name
        assert pix.shape == gold["pix_" + name].shape and np.array_equal(pix, gold["pix_" + name]), name
        parsed[name] = (P.parse(data), stats)
    # the fixtures cover what they are meant to cover
    p = {n: q for n, (q, _) in parsed.items()}
    assert {(q["hs"], q["vs"]) for q in p.values() if q["ncomp"] == 3} == {(1, 1), (2, 1), (2, 2)}
    assert p["gray"]["ncomp"] == 1 and p["one_pixel"]["width"] == p["one_pixel"]["height"] == 1
    # Pillow's script: ten scans on four levels, up to five of them at a time
    sc = p["s2_q90"]["scans"]
    assert [(len(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in sc] == [
        (3, 0, 0, 0, 1), (1, 1, 5, 0, 2), (1, 1, 63, 0, 1), (1, 1, 63, 0, 1), (1, 6, 63, 0, 2), (1, 1, 63, 2, 1), (3, 0, 0, 1, 0), (1, 1, 63, 1, 0),
        (1, 1, 63, 1, 0), (1, 1, 63, 1, 0)]
    assert [s["level"] for s in sc] == [0, 1, 1, 1, 1, 2, 1, 2, 2, 3] and p["s2_q90"]["levels"] == 4
    assert [s["level"] for s in p["gray"]["scans"]] == [0, 1, 1, 2, 1, 3]
    # restart intervals count MCUs in the interleaved DC scans and blocks in the scans of one component
    assert {(len(s["comps"]), s["ri"], len(s["segments"])) for s in p["rst_blocks3"]["scans"]} == {(3, 3, 4), (1, 3, 16), (1, 3, 4)}
    assert sum(len(s["segments"]) for s in p["rst_rows1"]["scans"]) == 70
    # Y alone walks 5 x 3 blocks of a 6 x 4 grid
    assert [s["units"] for s in p["narrow_y"]["scans"] if s["comps"] == [0]] == [15] * 4 and p["narrow_y"]["mcux"] * p["narrow_y"]["hs"] == 6
    assert parsed["eob_long"][1]["eob_cat_max"] >= 13 and parsed["s2_q30"][1]["eob_cat_max"] >= 3
    # widths 2, 3, 4 at both subsamplings: a chroma plane of at most two samples a row, repeated and not filtered
    assert sorted((q["width"], q["hs"], q["vs"]) for n, q in p.items() if n[0] == "w") == [(2, 2, 1), (2, 2, 2), (3, 2, 1), (3, 2, 2), (4, 2, 1), (4, 2, 2)]
    for n in ("w3_s1", "w4_s1", "w2_s2", "w3_s2", "w4_s2"):               # ... and filtering them gives other pixels: the goldens tell the two apart
        coef, _, _ = P.entropy_decode(bytes(gold["file_" + n]), p[n])
        assert not np.array_equal(P.R.pixels_from(coef, p[n]), gold["pix_" + n]), n
    assert gold["pix_s1_q100_noise"].min() == 0 and gold["pix_s1_q100_noise"].max() == 255      # saturating samples


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(23)
    for k in range(40):
        w, h = (int(v) for v in rs.randint(1, 71, 2))
        if k % 2:
            a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            a = np.clip(np.linspace(0, 255, w)[None, :, None] + rs.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
        opts = dict(quality=int(rs.randint(20, 101)), progressive=True)
        if k % 4 == 3:
            a = a[:, :, 0]                                                   # grayscale
        else:
            opts["subsampling"] = k % 4
        if k % 5 == 4:
            opts["restart_marker_rows"] = 1
        elif k % 5 == 2:
            opts["restart_marker_blocks"] = int(rs.randint(1, 6))
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", **opts)
        pix, status, _ = P.decode(buf.getvalue())
        assert {s for _, _, s in status} == {P.SEG_OK}
        assert np.array_equal(pix, np.asarray(Image.open(buf).convert("RGB"))), (w, h, opts)


def huff_bytes(bits, vals):
    """MgJpegHuff (csrc/jpeg_entropy.hpp) from a DHT's counts and symbols, by the definition of its fields"""
    look, maxcode, valoffset = np.zeros(512, np.uint16), np.full(18, -1, np.int32), np.zeros(18, np.int32)
    huffval = np.zeros(256, np.uint8)
    huffval[:len(vals)] = vals
    code = k = 0
    for l in range(1, 17):
        if bits[l - 1]:
            valoffset[l] = k - code
            for _ in range(bits[l - 1]):
                if l <= 9:
                    look[code << (9 - l):(code + 1) << (9 - l)] = l << 8 | vals[k]
                k += 1
                code += 1
            maxcode[l] = code - 1
        code <<= 1
    return look.tobytes() + maxcode.tobytes() + valoffset.tobytes() + huffval.tobytes()


def same_parse(p, r, name):
    for k in ("width", "height", "ncomp", "hs", "vs", "mcux", "mcuy", "levels"):
        assert p[k] == r[k], (name, k)
    assert len(p["scans"]) == len(r["scans"]) and p["nseg"] == sum(len(s["segments"]) for s in r["scans"]) == len(p["segments"]), name
    assert all(len(t) == ops.jpeg_huff_bytes() == 1424 for t in p["pool"]) and len(set(p["pool"])) == len(p["pool"]), name
    used = set()
    for k, (a, b) in enumerate(zip(p["scans"], r["scans"])):
        for f in ("comps", "ss", "se", "ah", "al", "ri", "level", "units", "ecs", "restarts"):
            assert a[f] == b[f], (name, k, f)
        assert a["ns"] == len(b["comps"]) and a["nseg"] == len(b["segments"]), (name, k)
        assert p["segments"][a["seg0"]:a["seg0"] + a["nseg"]].tolist() == [list(s) for s in b["segments"]], (name, k)
        for c in range(3):                                                    # the tables by content, through the pool
            if c in b["dc_tables"]:
                assert p["pool"][a["dc"][c]] == huff_bytes(*b["dc_tables"][c]), (name, k, c)
                used.add(a["dc"][c])
            else:
                assert a["dc"][c] == -1, (name, k, c)
        if b["ac_table"] is not None:
            assert p["pool"][a["ac"]] == huff_bytes(*b["ac_table"]), (name, k)
            used.add(a["ac"])
        else:
            assert a["ac"] == -1, (name, k)
    assert used == set(range(len(p["pool"]))), name
    q = np.frombuffer(p["quant"], np.uint8).reshape(3, 64)
    for c in range(3):
        assert np.array_equal(q[c], r["qt"][c].astype(np.uint8) if c < r["ncomp"] else np.zeros(64, np.uint8)), (name, c)


def test_parser_equals_the_restatement_on_every_fixture(gold):
    assert (P.INCOMPLETE_PROGRESSION, P.ILLEGAL_PROGRESSION, P.TOO_MANY_SCANS) == (14, 15, 16)
    assert set(I.JPEG_PROGRESSIVE_REASONS) == {14, 15, 16} and not set(I.JPEG_PROGRESSIVE_REASONS) & set(I.JPEG_REASONS)
    names = [k[5:] for k in gold if k.startswith("file_")]
    assert len(names) == 26
    for name in names:
        data = bytes(gold["file_" + name])
        p, r = I.parse_jpeg(data, progressive=True), P.parse(data)
        assert p["reason"] == r["reason"] and p["detail"] == r.get("detail", p["detail"]), name
        if r["reason"] == P.OK:
            same_parse(p, r, name)
    for name, reason in zip(gold["refused"], gold["refused_reason"]):
        assert I.parse_jpeg(bytes(gold["file_" + name]), progressive=True)["reason"] == int(reason), name
    assert sorted(int(v) for v in gold["refused_reason"]) == [6, 14, 14, 15]
    for name in gold["corrupt"]:                                             # a sound header: the parser accepts them
        assert I.parse_jpeg(bytes(gold["file_" + name]), progressive=True)["reason"] == 0, name


def test_the_new_entry_points_are_derived_from_their_header():
    """include/mgnns_jpeg_progressive.h declares the three entry points; _lib parses it as it parses mgnns_hip.h, the library exports
    them with the derived signatures, and mgnns_hip.h's own tables do not change."""
    import ctypes
    import re
    from mgnns_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mgnns_jpeg_progressive.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = {n: len(p.split(",")) for n, p in re.findall(r"\b(mgnns_\w+)\s*\(([^()]*)\)\s*;", code)}
    assert declared == {"mgnns_jpeg_huff_bytes": 1, "mgnns_jpeg_parse_progressive": 9, "mgnns_jpeg_decode_progressive_fwd": 26}
    assert set(_lib.EXTENSION_SIGNATURES) == {"mgnns_jpeg_parse_progressive", "mgnns_jpeg_decode_progressive_fwd"}
    assert _lib.EXTENSION_SIZE_GETTERS == {"mgnns_jpeg_huff_bytes": []}
    assert not (set(_lib.EXTENSION_SIGNATURES) | set(_lib.EXTENSION_SIZE_GETTERS)) & (set(_lib.SIGNATURES) | set(_lib.SIZE_GETTERS))
    for name, args in _lib.EXTENSION_SIGNATURES.items():
        assert len(args) == declared[name], name
    V, I32 = ctypes.c_void_p, ctypes.c_int
    assert _lib.EXTENSION_SIGNATURES["mgnns_jpeg_parse_progressive"] == [V, ctypes.c_size_t, I32, V, V, V, ctypes.c_size_t, V, V]
    L = _lib.lib()
    for name in declared:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (0 if name == "mgnns_jpeg_huff_bytes" else declared[name]), name
    assert L.mgnns_jpeg_huff_bytes() == 1424 and L.mgnns_jpeg_huff_bytes.restype is ctypes.c_size_t
    with pytest.raises(_lib.MgnnsLibraryError, match="a second time"):
        _lib._read_extensions(_lib.EXTENSION_HEADERS, {"mgnns_jpeg_huff_bytes": None})
    with pytest.raises(_lib.MgnnsLibraryError, match="no_such.h"):
        _lib._read_extensions((os.path.join(ROOT, "include", "no_such.h"),), {})


def test_parser_on_rewritten_scripts(gold):
    """Scripts Pillow does not write, made by editing a fixture's scan headers (the parsers read no entropy-coded data): both parsers
    give the same answer, and the answer is the documented one."""
    data = bytes(gold["file_s2_q90"])
    p = P.parse(data)
    at = [s["ecs"][0] for s in p["scans"]]              # behind a scan header; Ss, Se and Ah/Al are its last three bytes
    cases = []
    for field, value in [(-3, 6), (-2, 64), (-1, 0x32), (-1, 0x0E), (-3, 0)]:
        d = bytearray(data)                              # scan 2 is Y 1-5 at Al 2: Ss > Se; Se = 64; a refinement with no first pass;
        d[at[1] + field] = value                         # Al = 14; a DC scan with Se = 5
        cases.append((bytes(d), 15, 1))
    d = bytearray(data)
    d[at[0] - 1] = 0x00                                  # the DC scan at Al = 0: the DC refinement's Ah = 1 contradicts it
    cases.append((bytes(d), 15, 6))
    cases.append((data[:at[0] - 14] + data[p["scans"][0]["ecs"][1]:], 15, 0))           # no DC scan: AC before DC
    cases.append((data[:p["scans"][9]["ecs"][1]] + data[at[9] - 10:], 15, 10))          # the last scan twice: Ah = 1 after Al = 0
    # gray, one coefficient per scan from 6 on: 32 scans are accepted as a script (and incomplete), the 33rd is one too many
    gray = bytes(gold["file_gray"])
    g = P.parse(gray)
    head = gray[:g["scans"][1]["ecs"][1]]                # ... DC, Y 1-5 and the AC table in force
    sos = gray[g["scans"][1]["ecs"][0] - 10:g["scans"][1]["ecs"][0] - 3]
    assert sos[:5] == b"\xff\xda\x00\x08\x01"
    more = [sos + bytes([k, k, 0]) + b"\x00" for k in range(6, 64)]
    cases.append((head + b"".join(more[:30]) + b"\xff\xd9", 14, 0))                     # (incomplete from DC on: it stands at Al = 1)
    cases.append((head + b"".join(more[:31]) + b"\xff\xd9", 16, 33))
    cases.append((head + b"".join(more) + b"\xff\xd9", 16, 33))
    for k, (d, reason, detail) in enumerate(cases):
        a, b = I.parse_jpeg(d, progressive=True), P.parse(d)
        assert a["reason"] == b["reason"] == reason and a["detail"] == b["detail"] == detail, (k, a, b)


def test_every_truncation_gives_a_reason_code(gold):
    data = bytes(gold["file_one_pixel"])
    p = P.parse(data)
    first, last = p["scans"][0]["ecs"][0], p["scans"][-1]["ecs"][1]
    seen = set()
    for n in range(0, len(data)):
        a, b = I.parse_jpeg(memoryview(data)[:n], progressive=True), P.parse(data[:n])
        assert a["reason"] == b["reason"] and a["reason"] in (1, 2, 14, 0), n
        assert a["reason"] == (1 if n < 2 else 2 if n < first else 14 if n < p["scans"][-1]["ecs"][0] else 0), n
        seen.add(a["reason"])
    assert seen == {0, 1, 2, 14} and last <= len(data)


def test_switch_off_parity(gold, base):
    """Without the keyword, and with progressive=False, parse_jpeg answers as it did: the same dictionary on every baseline
    fixture, reason 3 on every progressive one.  With the switch on a baseline file gets the same fields, and no scans."""
    for k in base:
        if not k.startswith("file_"):
            continue
        data = bytes(base[k])
        a, b, c = I.parse_jpeg(data), I.parse_jpeg(data, progressive=False), I.parse_jpeg(data, progressive=True)
        assert set(a) == set(b) and "scans" not in a
        for f in a:
            assert np.array_equal(a[f], b[f]), (k, f)
        if k == "file_progressive":
            assert a == dict(reason=3, detail=0xC2) and c["reason"] == 0 and len(c["scans"]) == 10
        else:
            assert c["reason"] == a["reason"] and (a["reason"] != 0 or (c["scans"] == [] and c["levels"] == 0)), k
            for f in a:
                assert np.array_equal(a[f], c[f]), (k, f)
    for k in gold:
        if k.startswith("file_") and k != "file_cmyk":
            assert I.parse_jpeg(bytes(gold[k])) == dict(reason=3, detail=0xC2) == I.parse_jpeg(bytes(gold[k]), progressive=False), k
    assert set(I.JPEG_REASONS) == set(range(14))


def test_host_side_refusals_and_crop_sampling(gold, base):
    prep = I.ImagePrep(size=16, device=None, progressive=True)
    assert prep.progressive and not I.ImagePrep(size=16, device=None).progressive
    good = [bytes(gold["file_" + n]) for n in ("s0_q90", "rst_rows1", "s2_q30", "gray")]
    pixels = [gold["pix_" + n] for n in ("s0_q90", "rst_rows1", "s2_q30", "gray")]
    bad = [good[0], bytes(gold["file_cut_before_scan7"]), bytes(base["file_s2_q90"]), bytes(gold["file_ah_patched"]), bytes(gold["file_cmyk"]),
           bytes(gold["file_cut_in_scan3"])]
    with pytest.raises(I.UnsupportedJpeg, match=r"image 1: incomplete progression.*image 3: illegal progression.*image 4: neither 1 nor 3") as e:
        prep.decode_jpeg(bad)
    assert e.value.refused == [(1, 14), (3, 15), (4, 6), (5, 14)]
    with pytest.raises(I.UnsupportedJpeg) as e:                               # the same prep with the switch off: reason 3 for all of them
        I.ImagePrep(size=16, device=None).decode_jpeg(good + [bytes(base["file_s2_q90"])])
    assert e.value.refused == [(0, 3), (1, 3), (2, 3), (3, 3)]
    with pytest.raises(RuntimeError, match="GPU only"):
        prep.decode_jpeg(good)
    # crops and flips from header sizes: the same draws in the same order as train() on the decoded arrays
    for seed in (3, 4):
        random.seed(seed)
        torch.manual_seed(seed)
        with pytest.raises(RuntimeError, match="GPU only"):
            prep.train(pixels)
        want = (prep.last_crops, prep.last_flips, random.getstate(), torch.get_rng_state())
        random.seed(seed)
        torch.manual_seed(seed)
        with pytest.raises(RuntimeError, match="GPU only"):
            prep.train_jpeg(good)
        assert (prep.last_crops, prep.last_flips) == want[:2] and random.getstate() == want[2] and torch.equal(torch.get_rng_state(), want[3])
    # a fallback sees only the files still refused
    seen = []

    def fallback(b):
        seen.append(bytes(b))
        return np.zeros((16, 16, 3), np.uint8)

    with pytest.raises(RuntimeError, match="GPU only"):
        prep.decode_jpeg(bad, fallback=fallback)
    assert seen == [bad[1], bad[3], bad[4], bad[5]]


def test_the_decoder_body_on_the_cpu(gold, tmp_path):
    """csrc/jpeg_parse.hpp + csrc/jpeg_progressive.hpp + csrc/jpeg_pixels.hpp -- the code the GPU lanes run -- compiled for the
    host: every accepted fixture decodes to its golden pixels, every corrupt one ends in its recorded status, every refused one in
    its reason."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "dev", "jpeg_progressive_host_check.cpp"), "-o", exe], check=True)

    def run(name, with_pixels):
        f = str(tmp_path / (name + ".jpg"))
        with open(f, "wb") as o:
            o.write(bytes(gold["file_" + name]))
        args = [exe, f]
        if with_pixels:
            with open(f[:-4] + ".rgb", "wb") as o:
                o.write(gold["pix_" + name].tobytes())
            args.append(f[:-4] + ".rgb")
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (name, r.stdout)
        return r.stdout

    for name in gold["accepted"]:
        out = run(name, True)
        assert "reason 0, worst status 0" in out and "pixels equal" in out, name
    for name, status in zip(gold["corrupt"], gold["corrupt_status"]):
        assert "reason 0, worst status %d," % status in run(name, False), name
    for name, reason in zip(gold["refused"], gold["refused_reason"]):
        assert "reason %d," % reason in run(name, False), name
