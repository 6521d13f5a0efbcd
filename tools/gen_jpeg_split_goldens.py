"""tests/golden/jpeg_split.npz: restart-free baseline JPEG files whose one scan is long enough to be split over many lanes
("Split scans"), encoded by Pillow (libjpeg-turbo) from seeded synthetic images, with the pixels Pillow's own decoder
gives for them (Image.open(...).convert('RGB')).  Build container only (needs Pillow); rerunning reproduces the committed file byte
for byte with the same Pillow / libjpeg-turbo (their versions are recorded in the file; the zip members carry a fixed date).

    python tools/gen_jpeg_split_goldens.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def photo(w, h, seed):
    """photograph-like: posterised gradients, a disc, a wavy horizon, a little sensor noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255.0 * x / (w - 1), 255.0 * y / (h - 1), 127.5 + 127.5 * np.sin((x + 2 * y) / 19.0)], 2)
    base[(x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2 < (0.25 * h) ** 2] *= 0.35          # a dark disc
    base[y > 0.8 * h + 6 * np.sin(x / 7.0)] = (40.0, 160.0, 60.0)                     # a wavy horizon
    base = np.round(base / 32.0) * 32.0                                               # flat areas (they keep the golden file small)
    return np.clip(base + rs.normal(0.0, 0.3, size=(h, w, 3)), 0, 255).astype(np.uint8)


def noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


# name, (w, h), source, Pillow's save options
ACCEPTED = [
    ("noise_s0_q100", (64, 64), noise, dict(quality=100, subsampling=0)),       # a scan above 8 KB: at 8-byte chunks more chunks than lanes
    ("photo_s2_opt", (128, 96), photo, dict(quality=90, subsampling=2, optimize=True)),      # its own Huffman tables
    ("photo_s1_opt", (128, 96), photo, dict(quality=90, subsampling=1, optimize=True)),
    ("gray", (56, 40), photo, dict(quality=90)),
]


def encode(arr, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **opts)
    return buf.getvalue()


def main():
    import PIL
    from PIL import Image, features
    from tests import jpeg_ref as R
    out = {}
    for name, (w, h), src, opts in ACCEPTED:
        arr = src(w, h, 300 if name.startswith("photo") else 301 + len(out))
        if name == "gray":
            arr = arr[:, :, 0]
        data = encode(arr, **opts)
        p = R.parse(data)
        assert p["reason"] == R.OK and len(p["segments"]) == 1, name           # restart-free: one segment
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["pix_" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    p = R.parse(bytes(out["file_noise_s0_q100"]))
    assert p["ecs_end"] - p["ecs_begin"] > 8192
    out["accepted"] = np.asarray([a[0] for a in ACCEPTED])
    out["versions"] = np.asarray(["Pillow " + PIL.__version__, "libjpeg-turbo " + str(features.version("jpg"))])

    path = os.path.join(ROOT, "tests", "golden", "jpeg_split.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:          # (np.savez stamps the members with the current time)
        for key in sorted(out):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            z.writestr(info, buf.getvalue())
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 100 * 1024
    for name, _, _, _ in ACCEPTED:
        print("  %-14s %6d bytes" % (name, out["file_" + name].size))


if __name__ == "__main__":
    main()
