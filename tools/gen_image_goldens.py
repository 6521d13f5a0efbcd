"""tests/golden/image_prep.npz: what the REFERENCE's image transforms (utils/util.py:67-146 Warp, MultiScaleCrop, run unmodified on
Pillow) make of a handful of small images.  Build container only (needs the reference checkout and PIL); the file it writes is
data -- source pixels, output pixels, sampled crops -- and travels with the repository.

    python tools/gen_image_goldens.py

Keys: size (the output extent S); src_<i> [H,W,3] uint8; warp_<i> = Warp(S)(src_<i>) [S,S,3] uint8;
seeds, crop_images; for seed s and image i: crop_s<s>_i<i> = (crop_w, crop_h, off_w, off_h) as MultiScaleCrop(S, scales, 2) samples
them right after random.seed(s), cropout_s<s>_i<i> = its output [S,S,3]; flip = (seed, image) and flipout = that output mirrored
left-right (what RandomHorizontalFlip does when it flips)."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 32
SCALES = (1.0, 0.875, 0.75, 0.66, 0.5)          # ENGINE:276
SEEDS = (0, 1, 2, 3)
CROP_IMAGES = (0, 3)


def sources():
    rs = np.random.RandomState(20240607)
    a = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    b = rs.randint(0, 256, (64, 48, 3)).astype(np.uint8)
    b[..., 0] = 0                                # planes saturated at both ends: the clip and the rounding term show here
    b[..., 1] = 255
    c = rs.randint(0, 256, (24, 90, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:80, 0:60]
    d = np.stack([(3 * xx + yy) % 256, (255 - 2 * yy) % 256, (xx * yy) % 256], -1) + rs.randint(-3, 4, (80, 60, 3))
    d = np.clip(d, 0, 255).astype(np.uint8)
    e = np.where(rs.uniform(size=(41, 43, 3)) < 0.5, 0, 255).astype(np.uint8)    # only 0 and 255
    return [a, b, c, d, e]


def main():
    out_path = os.path.join(ROOT, "tests", "golden", "image_prep.npz")    # (resolved before the shims change directory)
    from PIL import Image
    from oracle import ref_shims
    U = ref_shims.install().UTIL
    warp = U.Warp(S)
    msc = U.MultiScaleCrop(S, scales=SCALES, max_distort=2)
    out = {"size": np.int64(S), "seeds": np.asarray(SEEDS), "crop_images": np.asarray(CROP_IMAGES)}
    srcs = sources()
    for i, a in enumerate(srcs):
        out["src_%d" % i] = a
        out["warp_%d" % i] = np.asarray(warp(Image.fromarray(a)))
    for s in SEEDS:
        for i in CROP_IMAGES:
            im = Image.fromarray(srcs[i])
            random.seed(s)
            crop = msc._sample_crop_size(im.size)
            random.seed(s)
            res = msc(im)
            out["crop_s%d_i%d" % (s, i)] = np.asarray(crop, dtype=np.int64)
            out["cropout_s%d_i%d" % (s, i)] = np.asarray(res)
    fs, fi = SEEDS[1], CROP_IMAGES[1]
    random.seed(fs)
    out["flip"] = np.asarray([fs, fi])
    out["flipout"] = np.asarray(msc(Image.fromarray(srcs[fi])).transpose(Image.FLIP_LEFT_RIGHT))
    np.savez_compressed(out_path, **out)
    print("%s: %d arrays, %d bytes" % (out_path, len(out), os.path.getsize(out_path)))
    assert os.path.getsize(out_path) <= 100 * 1024


if __name__ == "__main__":
    main()
