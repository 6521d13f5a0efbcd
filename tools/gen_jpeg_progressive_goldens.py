"""tests/golden/jpeg_progressive.npz: small progressive JPEG files encoded by Pillow (libjpeg-turbo) from seeded synthetic images,
with the pixels Pillow's own decoder gives for them (Image.open(...).convert('RGB')), the files the GPU decoder must refuse with
the switch on, and two files with a sound header and a corrupt scan.  Build container only (needs Pillow); rerunning reproduces
the committed file byte for byte with the same Pillow / libjpeg-turbo (their versions are recorded in the file; the zip members
carry a fixed date).  The conventions are tools/gen_jpeg_goldens.py's.

    python tools/gen_jpeg_progressive_goldens.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gen_jpeg_goldens import encode, noise, photo  # noqa: E402


def flat_with_corners(w, h, seed):
    """flat 128 with a random 8x8 block in the first and in the last corner: between them one end-of-band run per AC scan"""
    rs = np.random.RandomState(seed)
    a = np.full((h, w, 3), 128, np.uint8)
    a[:8, :8] = rs.randint(0, 256, (8, 8, 1))
    a[h - 8:, w - 8:] = rs.randint(0, 256, (8, 8, 1))
    return a


# name, (w, h), source, Pillow's save options (progressive=True is added to all)
ACCEPTED = [
    ("s0_q90", (37, 53), photo, dict(quality=90, subsampling=0)),
    ("s1_q90", (37, 53), photo, dict(quality=90, subsampling=1)),
    ("s2_q90", (37, 53), photo, dict(quality=90, subsampling=2)),
    ("s1_q100_noise", (17, 33), noise, dict(quality=100, subsampling=1)),       # large coefficients, ZRL, dense refinement
    ("s2_q100_noise", (9, 130), noise, dict(quality=100, subsampling=2)),
    ("s2_q30", (64, 48), photo, dict(quality=30, subsampling=2)),              # end-of-band runs across blocks
    ("one_pixel", (1, 1), photo, dict(quality=90, subsampling=2)),
    ("one_block", (8, 8), photo, dict(quality=90, subsampling=2)),
    ("one_mcu", (16, 16), photo, dict(quality=90, subsampling=2)),
    ("gray", (17, 33), photo, dict(quality=90)),
    ("rst_rows1", (37, 53), photo, dict(quality=90, subsampling=1, restart_marker_rows=1)),
    ("rst_blocks3", (64, 48), photo, dict(quality=90, subsampling=2, restart_marker_blocks=3)),  # MCUs in DC scans, blocks in AC scans
    ("narrow_y", (33, 17), photo, dict(quality=90, subsampling=2)),            # Y alone has fewer block columns than the MCU grid
    ("eob_long", (1024, 1024), flat_with_corners, dict(quality=90)),           # gray: an end-of-band run over 16 382 blocks
    # widths 2..4 with subsampled chroma: libjpeg repeats the samples of a chroma plane of at most two samples a row, it does not filter
    ("w2_s1", (2, 9), noise, dict(quality=90, subsampling=1)),
    ("w3_s1", (3, 17), noise, dict(quality=90, subsampling=1)),
    ("w4_s1", (4, 5), noise, dict(quality=90, subsampling=1)),
    ("w2_s2", (2, 19), noise, dict(quality=90, subsampling=2)),
    ("w3_s2", (3, 6), noise, dict(quality=90, subsampling=2)),
    ("w4_s2", (4, 33), noise, dict(quality=90, subsampling=2)),
]


def main():
    from PIL import Image, features
    from tests import jpeg_progressive_ref as P
    out = {}
    names = []
    for k, (name, (w, h), src, opts) in enumerate(ACCEPTED):
        arr = src(w, h, 200 + k)
        if name in ("gray", "eob_long"):
            arr = arr[:, :, 0]
        data = encode(arr, progressive=True, **opts)
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["pix_" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        names.append(name)
    out["accepted"] = np.asarray(names)
    pix, status, stats = P.decode(bytes(out["file_eob_long"]))
    assert np.array_equal(pix, out["pix_eob_long"]) and stats["eob_cat_max"] >= 13, stats     # an EOB-run symbol of category >= 13
    for name in ("w2_s1", "w3_s1", "w4_s1", "w2_s2", "w3_s2", "w4_s2"):     # the narrow files tell repeating from filtering
        p = P.parse(bytes(out["file_" + name]))
        coef, status, _ = P.entropy_decode(bytes(out["file_" + name]), p)
        assert np.array_equal(P.pixels_from(coef, p), out["pix_" + name]), name
        assert name == "w2_s1" or not np.array_equal(P.R.pixels_from(coef, p), out["pix_" + name]), name    # (one sample a row, h2v1: the same)
    p = P.parse(bytes(out["file_narrow_y"]))
    assert p["mcux"] * 2 == 6 and [s["units"] for s in p["scans"] if s["comps"] == [0] and s["ss"]][0] == 5 * 3
    p = P.parse(bytes(out["file_rst_blocks3"]))
    assert {(len(s["comps"]), s["ri"], len(s["segments"])) for s in p["scans"]} == {(3, 3, 4), (1, 3, 16), (1, 3, 4)}

    # ---- files the decoder refuses with the switch on, with the parser's reason ----
    whole = bytes(out["file_s2_q90"])
    p = P.parse(whole)
    assert len(p["scans"]) == 10
    cut7 = whole[:p["scans"][5]["ecs"][1]] + b"\xff\xd9"                 # in front of whatever precedes the 7th scan's SOS; Pillow smooths it
    b, e = p["scans"][2]["ecs"]
    cut3 = whole[:(b + e) // 2]                                          # in the middle of scan 3's data
    refine = [s for s in p["scans"] if s["ah"]][0]
    at = refine["ecs"][0] - 1                                            # the scan header's Ah / Al byte
    assert whole[at] == refine["ah"] << 4 | refine["al"]
    patched = bytearray(whole)
    patched[at] = (refine["ah"] + 1) << 4 | refine["al"]
    cmyk = io.BytesIO()
    Image.fromarray(noise(8, 8, 9)).convert("CMYK").save(cmyk, "JPEG", quality=90, progressive=True)
    refused = [("cut_before_scan7", cut7, P.INCOMPLETE_PROGRESSION), ("cut_in_scan3", cut3, P.INCOMPLETE_PROGRESSION),
               ("ah_patched", bytes(patched), P.ILLEGAL_PROGRESSION), ("cmyk", cmyk.getvalue(), P.COMPONENTS)]
    for name, data, reason in refused:
        assert P.parse(data)["reason"] == reason, (name, P.parse(data))
        out["file_" + name] = np.frombuffer(data, np.uint8)
    out["refused"] = np.asarray([r[0] for r in refused])
    out["refused_reason"] = np.asarray([r[2] for r in refused], np.int64)
    smoothed = np.asarray(Image.open(io.BytesIO(cut7)).convert("RGB")).astype(int)
    assert np.abs(smoothed - out["pix_s2_q90"].astype(int)).max() > 8     # Pillow decodes the cut file to other pixels: hence refused

    # ---- sound header, corrupt scan: the status the decoder reports, and the scan it reports it for ----
    b, e = p["scans"][-1]["ecs"]
    cut = whole[:(b + e) // 2]                                           # the last scan's data cut short
    b, e = p["scans"][8]["ecs"]                                          # (a chroma refinement: no later scan builds on it)
    n = e - b
    ones = whole[:b] + (b"\xff\x00" * n)[:n // 2 * 2] + whole[e:]         # one AC scan's data: FF 00 pairs, all-one bits
    corrupt = [("last_scan_cut", cut, P.SEG_OUT_OF_DATA, 9), ("ac_all_ones", ones, P.SEG_INVALID_CODE, 8)]
    for name, data, status, scan in corrupt:
        _, st, _ = P.decode(data)
        assert [(k, s) for k, _, s in st if s] == [(scan, status)], (name, st)
        out["file_" + name] = np.frombuffer(data, np.uint8)
    out["corrupt"] = np.asarray([c[0] for c in corrupt])
    out["corrupt_status"] = np.asarray([c[2] for c in corrupt], np.int64)
    out["corrupt_scan"] = np.asarray([c[3] for c in corrupt], np.int64)
    import PIL
    out["versions"] = np.asarray(["Pillow " + PIL.__version__, "libjpeg-turbo " + str(features.version("jpg"))])

    path = os.path.join(ROOT, "tests", "golden", "jpeg_progressive.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:          # (np.savez stamps the members with the current time)
        for key in sorted(out):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            z.writestr(info, buf.getvalue())
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == "__main__":
    main()
