"""tests/golden/jpeg_decode.npz: small baseline JPEG files encoded by Pillow (libjpeg-turbo) from seeded synthetic images, with the
pixels Pillow's own decoder gives for them (Image.open(...).convert('RGB')), the files the GPU decoder must refuse, and three files
with a sound header and a corrupt scan.  Build container only (needs Pillow); rerunning reproduces the committed file byte for byte
with the same Pillow / libjpeg-turbo (their versions are recorded in the file; the zip members carry a fixed date).

    python tools/gen_jpeg_goldens.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def photo(w, h, seed):
    """gradients plus noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin((x + 2 * y) / 5.0)], 2)
    return np.clip(base + rs.normal(0.0, 20.0, size=(h, w, 3)), 0, 255).astype(np.uint8)


def noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


# name, (w, h), source, Pillow's save options
ACCEPTED = [
    ("s0_q90", (37, 53), photo, dict(quality=90, subsampling=0)),
    ("s1_q90", (17, 33), photo, dict(quality=90, subsampling=1)),
    ("s2_q90", (37, 53), photo, dict(quality=90, subsampling=2)),
    ("s0_q100_noise", (16, 16), noise, dict(quality=100, subsampling=0)),
    ("s1_q100_noise", (9, 130), noise, dict(quality=100, subsampling=1)),
    ("s2_q100_noise", (17, 33), noise, dict(quality=100, subsampling=2)),
    ("opt_q30", (64, 48), photo, dict(quality=30, subsampling=2, optimize=True)),
    ("rst_blocks3", (64, 48), photo, dict(quality=90, subsampling=2, restart_marker_blocks=3)),
    ("rst_rows1", (37, 53), photo, dict(quality=90, subsampling=1, restart_marker_rows=1)),
    ("rst_rows2", (9, 130), photo, dict(quality=90, subsampling=2, restart_marker_rows=2)),
    ("one_pixel", (1, 1), photo, dict(quality=90, subsampling=2)),
    ("one_block", (8, 8), photo, dict(quality=90, subsampling=0)),
    ("one_mcu_s2", (16, 16), photo, dict(quality=90, subsampling=2)),
    ("gray", (17, 33), photo, dict(quality=90)),
]


def encode(arr, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **opts)
    return buf.getvalue()


def main():
    from PIL import Image, features
    from tests import jpeg_ref as R
    out = {}
    names = []
    for k, (name, (w, h), src, opts) in enumerate(ACCEPTED):
        arr = src(w, h, 100 + k)
        if name == "gray":
            arr = arr[:, :, 0]
        data = encode(arr, **opts)
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["pix_" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        names.append(name)
    out["accepted"] = np.asarray(names)

    # ---- files the decoder refuses, with the parser's reason ----
    base = encode(photo(16, 16, 7), quality=90, subsampling=0)
    p = R.parse(base)
    sof = base.index(b"\xff\xc0")
    patched = bytearray(base)
    assert patched[sof + 11] == 0x11
    patched[sof + 11] = 0x12                                         # Y sampled 1 x 2 (4:4:0)
    sos = base.rindex(b"\xff\xda", 0, p["ecs_begin"])
    two = base[:p["ecs_end"]] + base[sos:p["ecs_end"]] + base[p["ecs_end"]:]      # the scan (header and data) twice
    cmyk = io.BytesIO()
    Image.fromarray(noise(8, 8, 9)).convert("CMYK").save(cmyk, "JPEG", quality=90)
    refused = [("progressive", encode(photo(16, 16, 7), quality=90, progressive=True), R.UNSUPPORTED_SOF),
               ("cmyk", cmyk.getvalue(), R.COMPONENTS),
               ("sampling_1x2", bytes(patched), R.SAMPLING),
               ("two_scans", two, R.SCANS),
               ("not_jpeg", b"\x89PNG\r\n\x1a\n" + bytes(56), R.NOT_JPEG)]
    for name, data, reason in refused:
        out["file_" + name] = np.frombuffer(data, np.uint8)
    out["refused"] = np.asarray([r[0] for r in refused])
    out["refused_reason"] = np.asarray([r[2] for r in refused], np.int64)

    # ---- sound header, corrupt scan: the status the decoder reports for the file ----
    whole = bytes(out["file_s2_q90"])
    p = R.parse(whole)
    cut = whole[:(p["ecs_begin"] + p["ecs_end"]) // 2]
    rst = bytes(out["file_rst_rows1"])
    p = R.parse(rst)
    at = p["segments"][1][1]                                          # the second restart marker
    assert rst[at] == 0xFF and 0xD0 <= rst[at + 1] <= 0xD7
    removed = rst[:at] + rst[at + 2:]
    p = R.parse(whole)
    n = p["ecs_end"] - p["ecs_begin"]
    ones = whole[:p["ecs_begin"]] + (b"\xff\x00" * n)[:n // 2 * 2] + whole[p["ecs_end"]:]
    corrupt = [("cut", cut, R.SEG_OUT_OF_DATA), ("rst_removed", removed, R.SEG_OUT_OF_DATA), ("all_ones", ones, R.SEG_INVALID_CODE)]
    for name, data, status in corrupt:
        out["file_" + name] = np.frombuffer(data, np.uint8)
    out["corrupt"] = np.asarray([c[0] for c in corrupt])
    out["corrupt_status"] = np.asarray([c[2] for c in corrupt], np.int64)
    import PIL
    out["versions"] = np.asarray(["Pillow " + PIL.__version__, "libjpeg-turbo " + str(features.version("jpg"))])

    path = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
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
