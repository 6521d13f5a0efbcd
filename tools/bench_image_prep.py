"""The image transforms' one launch per batch (csrc/image_prep.hip) at the sizes a user runs, B = 256 -> 448 x 448:

    warp_500x375     the eval transform of 500 x 375 photographs
    warp_1024x768    ... of 1024 x 768 photographs
    train_1024x768   the training transform (sampled crops and flips) of the same batch

Per case: microseconds per launch and images/s (HIP events over n launches -- 200 by default, about 0.1 s a round --, three
rounds alternating with a torch copy_ that moves the same bytes -- the crop's bytes read plus the fp32 output written --
best of each, and the ratio), the H2D copy of the
staged pixel buffer from pinned memory, and the launch's share of the two trunks' eval forward (ResNet-101 + ResNet-50 at 448)
for the same 256 images, timed in the same process over 10 forwards (about 0.5 s).  One JSON line.

    python tools/bench_image_prep.py [--batch 256] [--iters 200] [--no-trunks]
"""
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mgnns_amd import _lib, ops, synth, trunk          # noqa: E402
from mgnns_amd.images import ImagePrep                 # noqa: E402

DEV = "cuda:0"


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timeit(fn, n, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us per call


def case(prep, imgs, n, crops=None, flips=None):
    B, S = len(imgs), prep.size
    p = prep.pack(imgs, crops, flips)
    table, table_dev, data_dev = prep._plans_on_device()
    pix_dev = torch.empty(p.pixels.numel(), dtype=torch.uint8, device=DEV)
    desc, desc_dev = p.desc.clone(), p.desc.to(DEV)
    h2d = timeit(lambda: pix_dev.copy_(p.pixels, non_blocking=True), max(3, n // 10), warm=1)
    out = torch.empty(B, 3, S, S, device=DEV)
    fn = lambda: ops.image_prep(pix_dev, desc, desc_dev, table, table_dev, data_dev, prep.table_dev, S, S, out=out)
    read = int((desc[:, 5] * desc[:, 6] * 3).sum())
    moved = read + out.numel() * 4
    src = torch.empty(moved // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    tk, tc = [], []
    for _ in range(3):
        tk.append(timeit(fn, n))
        tc.append(timeit(lambda: dst.copy_(src), n))
    again = out.clone()
    fn()
    assert torch.equal(out, again)
    t = min(tk)
    return {"B": B, "us": round(t, 1), "images_per_s": round(B / t * 1e6), "copy_us": round(min(tc), 1), "ratio_to_copy": round(t / min(tc), 3),
            "moved_MB": round(moved / 1e6, 1), "read_MB": round(read / 1e6, 1), "TB/s": round(moved / t / 1e6, 2),
            "h2d_us": round(h2d, 1), "h2d_MB": round(p.pixels.numel() / 1e6, 1), "h2d_GB/s": round(p.pixels.numel() / h2d / 1e3, 1),
            "plans": int(table.shape[0]), "runs_us": [round(v, 1) for v in tk], "copy_runs_us": [round(v, 1) for v in tc]}, t


def main():
    B, n = arg("--batch", 256), arg("--iters", 200)
    built = _lib.check_sources("tools/bench_image_prep.py")
    res = {"bench": "image_prep", "device": torch.cuda.get_device_name(0), "sources": built, "size": 448, "iters": n}
    prep = ImagePrep(448, device=DEV)
    rng = np.random.default_rng(0)
    times = {}
    for name, (h, w) in (("500x375", (375, 500)), ("1024x768", (768, 1024))):
        base = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(8)]
        imgs = [base[i % 8] for i in range(B)]
        res["warp_" + name], times["warp_" + name] = case(prep, imgs, n)
        if name == "1024x768":
            random.seed(0)
            torch.manual_seed(0)
            crops = [prep.sample_crop(w, h) for _ in imgs]
            flips = [bool(torch.rand(1) < 0.5) for _ in imgs]
            res["train_" + name], times["train_" + name] = case(prep, imgs, n, crops, flips)
    if "--no-trunks" not in sys.argv:
        obj = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet101(), 1)).to(DEV).eval()
        place = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet50(365), 2)).to(DEV).eval()
        img = torch.randn(B, 3, 448, 448, device=DEV)
        with torch.no_grad():
            t = timeit(lambda: (obj(img), place(img)), 10, warm=2)
        res["trunks_eval_us"] = round(t, 1)
        res["trunks_images_per_s"] = round(B / t * 1e6)
        res["share_of_trunks"] = {k: round(v / t, 4) for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
