"""The JPEG decoder (csrc/jpeg_decode.hip) at the sizes a user runs: B = 256 files of 500 x 375 and of 1024 x 768, quality 90,
4:2:0, encoded here by Pillow from seeded synthetic photographs (gradients plus noise) -- or, without Pillow, read from a directory
of .jpg files given as the argument.

Per case: microseconds per batch for the whole decode (zeroing the workspace, Huffman decoding, IDCT, upsampling + colour) and per
stage (HIP events over n rounds -- 100 by default --, three rounds alternating between the whole and the stages, best of each),
images/s, the bytes that cross PCIe (files + tables + records) against the raw-pixel path's, the host's share (parsing and staging
a batch), Pillow's own decode time per image on this host, and the two trunks' eval forward (ResNet-101 + ResNet-50 at 448) for the
same 256 images in the same process: the yardstick a decode launched beside them should stay under.  One JSON line.

--progressive adds, per size, the same photographs saved as progressive files and decoded by ImagePrep(progressive=True): the whole
decode, the entropy stage as a whole and level by level (the entropy stage with the levels after l left out, minus the same with l
left out too), IDCT and colour, and Pillow's time for those files; the baseline leg runs in the same process as before.

--split [CHUNK] adds, per size, the same baseline files decoded by ImagePrep(split=CHUNK) (ops.jpeg_decode_split; without a number
the default chunk): the whole decode and the stages by the same method, the segments the split kernel took, and the pixel buffer
compared with the switch-off leg's.

--layouts adds, at 500 x 375, the baseline files decoded by ImagePrep(layouts=True) (ops.jpeg_decode_layouts: the baseline route with
the switch on, its pixel buffer compared with the switch-off leg's), the baseline files with a restart marker per MCU row, and the
same photographs as files of other component layouts, each without restart markers and with one per MCU row of its source: CMYK
(4:4:4), and 375 x 500 4:4:0 relabelled from the 500 x 375 4:2:2 files (47 x 32 MCUs either way).

    python tools/bench_jpeg.py [DIR] [--batch 256] [--iters 100] [--restart-rows N] [--no-trunks] [--progressive] [--split [CHUNK]] [--layouts]
"""
import glob
import io
import json
import os
import sys
import time

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


def photograph(w, h, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255.0 * x / (w - 1), 255.0 * y / (h - 1), 127.5 + 127.5 * np.sin((x + 2 * y) / 23.0)], 2)
    return np.clip(base + rs.normal(0.0, 12.0, size=(h, w, 3)), 0, 255).astype(np.uint8)


def encode(w, h, B, restart_rows, progressive=False):
    from PIL import Image
    distinct = []
    for k in range(8):
        buf = io.BytesIO()
        opts = dict(quality=90, subsampling=2, progressive=progressive)
        if restart_rows:
            opts["restart_marker_rows"] = restart_rows
        Image.fromarray(photograph(w, h, k)).save(buf, "JPEG", **opts)
        distinct.append(buf.getvalue())
    return [distinct[i % 8] for i in range(B)]


def case(prep, files, n):
    B = len(files)
    t0 = time.perf_counter()
    headers = prep._jpeg_headers(files, None)
    t1 = time.perf_counter()
    args, batch = prep._jpeg_run(headers, staged_only=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    whole = lambda: ops.jpeg_decode(*args, check=False)
    stage = {k: (lambda m=m: ops.jpeg_decode(*args, stages=m, check=False)) for k, m in (("entropy", 1), ("idct", 2), ("colour", 4))}
    assert not bool(whole().any())
    first = batch.pixels.clone()
    once = timeit(whole, 2, warm=0)
    if once * n > 4e6:                           # a round of more than 4 s: fewer iterations, and the result says how many
        n = max(10, int(4e6 / once))
    tw, ts = [], {k: [] for k in stage}
    for _ in range(3):
        tw.append(timeit(whole, n))
        for k, fn in stage.items():
            ts[k].append(timeit(fn, n))
    whole()
    assert torch.equal(batch.pixels, first)
    t = min(tw)
    h2d = int(args[0].numel()) + 8 * int(args[2].numel() + args[4].numel())
    res = {"B": B, "iters_used": n, "us": round(t, 1), "images_per_s": round(B / t * 1e6), "stage_us": {k: round(min(v), 1) for k, v in ts.items()},
           "segments": int(args[3].shape[0]), "table_sets": int(args[5].shape[0]), "file_MB": round(sum(len(f) for f in files) / 1e6, 2),
           "h2d_MB": round(h2d / 1e6, 2), "raw_pixel_MB": round(batch.pixels.numel() / 1e6, 1),
           "host_parse_ms": round((t1 - t0) * 1e3, 2), "host_stage_ms": round((t2 - t1) * 1e3, 2), "runs_us": [round(v, 1) for v in tw]}
    try:
        from PIL import Image
        t0 = time.perf_counter()
        for f in files[:64]:
            Image.open(io.BytesIO(f)).convert("RGB")
        res["pillow_ms_per_image"] = round((time.perf_counter() - t0) / min(64, B) * 1e3, 3)
        assert torch.equal(batch.image(0).cpu(), torch.from_numpy(np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB"))))
    except ImportError:
        pass
    return res, t


def case_progressive(prep, files, n):
    """the --progressive leg: the method of case(), on ops.jpeg_decode_progressive"""
    B = len(files)
    t0 = time.perf_counter()
    headers = prep._jpeg_headers(files, None)
    t1 = time.perf_counter()
    args, batch = prep._jpeg_run(headers, staged_only=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    data, img, img_dev, seg, seg_dev, tables, pseg, pseg_dev, counts, pool, qsets, pixels = args
    run = lambda stages=7: ops.jpeg_decode_progressive(*args, stages=stages, check=False)
    assert not bool(run().any())
    first = batch.pixels.clone()

    def upto(l):                                 # the entropy stage with the levels after l left out (l = -1: the zeroing alone)
        k = sum(counts[:l + 1])
        return lambda: ops.jpeg_decode_progressive(data, img, img_dev, seg, seg_dev, tables, pseg[:k], pseg_dev[:k], counts[:l + 1], pool, qsets,
                                                   pixels, stages=1, check=False)

    fns = {"whole": run, "entropy": lambda: run(1), "idct": lambda: run(2), "colour": lambda: run(4)}
    fns.update({"upto%d" % l: upto(l) for l in range(-1, len(counts))})
    once = timeit(run, 2, warm=0)
    if once * n > 4e6:
        n = max(10, int(4e6 / once))
    ts = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ts[k].append(timeit(fn, n))
    run()
    assert torch.equal(batch.pixels, first)
    best = {k: min(v) for k, v in ts.items()}
    t = best["whole"]
    res = {"B": B, "iters_used": n, "us": round(t, 1), "images_per_s": round(B / t * 1e6),
           "stage_us": {k: round(best[k], 1) for k in ("entropy", "idct", "colour")}, "zeroing_us": round(best["upto-1"], 1),
           "level_us": [round(best["upto%d" % l] - best["upto%d" % (l - 1)], 1) for l in range(len(counts))], "level_segments": list(counts),
           "tables_in_pool": int(pool.shape[0]), "file_MB": round(sum(len(f) for f in files) / 1e6, 2),
           "host_parse_ms": round((t1 - t0) * 1e3, 2), "host_stage_ms": round((t2 - t1) * 1e3, 2), "runs_us": [round(v, 1) for v in ts["whole"]]}
    try:
        from PIL import Image
        t0 = time.perf_counter()
        for f in files[:64]:
            Image.open(io.BytesIO(f)).convert("RGB")
        res["pillow_ms_per_image"] = round((time.perf_counter() - t0) / min(64, B) * 1e3, 3)
        assert torch.equal(batch.image(0).cpu(), torch.from_numpy(np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB"))))
    except ImportError:
        pass
    return res, t


def case_split(prep, files, n, want):
    """the --split leg: the method of case(), on ops.jpeg_decode_split; `want`: the switch-off leg's pixel buffer"""
    B = len(files)
    args, batch = prep._jpeg_run(prep._jpeg_headers(files, None), staged_only=True)
    torch.cuda.synchronize()
    run = lambda stages=7: ops.jpeg_decode_split(*args, chunk_bytes=prep.split, stages=stages, check=False)
    assert not bool(run().any())
    assert torch.equal(batch.pixels, want)
    fns = {"whole": run, "entropy": lambda: run(1), "idct": lambda: run(2), "colour": lambda: run(4)}
    once = timeit(run, 2, warm=0)
    if once * n > 4e6:
        n = max(10, int(4e6 / once))
    ts = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ts[k].append(timeit(fn, n))
    run()
    assert torch.equal(batch.pixels, want)
    best = {k: min(v) for k, v in ts.items()}
    seg = args[3]
    taken = int(((seg[:, 2] - seg[:, 1]) >= 2 * prep.split).sum())
    res = {"B": B, "chunk_bytes": prep.split, "iters_used": n, "us": round(best["whole"], 1), "images_per_s": round(B / best["whole"] * 1e6),
           "stage_us": {k: round(best[k], 1) for k in ("entropy", "idct", "colour")}, "segments": int(seg.shape[0]), "segments_split": taken,
           "runs_us": [round(v, 1) for v in ts["whole"]]}
    return res, best["whole"]


def layout_files(w, h, B):
    """{name: files}: the photographs as CMYK and as 4:4:0 relabelled from 4:2:2 (h x w), restart-free and with a marker per MCU row"""
    from PIL import Image
    out = {}
    for rows in (0, 1):
        cmyk, s440 = [], []
        for k in range(8):
            opts = dict(quality=90, restart_marker_rows=rows) if rows else dict(quality=90)
            rgb = photograph(w, h, k)
            buf = io.BytesIO()
            Image.fromarray(np.concatenate([rgb, rgb[:, ::-1, :1]], 2), "CMYK").save(buf, "JPEG", subsampling=0, **opts)
            cmyk.append(buf.getvalue())
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, "JPEG", subsampling=1, **opts)
            d = bytearray(buf.getvalue())
            pos = 2
            while d[pos + 1] != 0xC0:
                pos += 2 + (d[pos + 2] << 8 | d[pos + 3])
            assert d[pos + 11] == 0x21                   # (ceil(w / 16) x ceil(h / 8) MCUs become ceil(h / 8) x ceil(w / 16))
            d[pos + 5:pos + 9] = bytes([w >> 8, w & 255, h >> 8, h & 255])          # height = w, width = h
            d[pos + 11] = 0x12
            s440.append(bytes(d))
        tag = "_rst1" if rows else ""
        out["cmyk" + tag] = [cmyk[i % 8] for i in range(B)]
        out["s440" + tag] = [s440[i % 8] for i in range(B)]
    return out


def case_layouts(prep, files, n, want=None):
    """the --layouts leg: the method of case(), on ops.jpeg_decode_layouts; `want`: the switch-off leg's pixel buffer, if there is one"""
    B = len(files)
    args, batch = prep._jpeg_run(prep._jpeg_headers(files, None), staged_only=True)
    torch.cuda.synchronize()
    run = lambda stages=7: ops.jpeg_decode_layouts(*args, chunk_bytes=prep.split, stages=stages, check=False)
    assert not bool(run().any())
    first = batch.pixels.clone()
    assert want is None or torch.equal(first, want)
    fns = {"whole": run, "entropy": lambda: run(1), "idct": lambda: run(2), "colour": lambda: run(4)}
    once = timeit(run, 2, warm=0)
    if once * n > 4e6:
        n = max(10, int(4e6 / once))
    ts = {k: [] for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ts[k].append(timeit(fn, n))
    run()
    assert torch.equal(batch.pixels, first)
    best = {k: min(v) for k, v in ts.items()}
    res = {"B": B, "iters_used": n, "us": round(best["whole"], 1), "images_per_s": round(B / best["whole"] * 1e6),
           "stage_us": {k: round(best[k], 1) for k in ("entropy", "idct", "colour")}, "segments": int(args[3].shape[0]),
           "layout_segments": int(args[11].shape[0]), "file_MB": round(sum(len(f) for f in files) / 1e6, 2),
           "runs_us": [round(v, 1) for v in ts["whole"]]}
    try:
        from PIL import Image
        assert torch.equal(batch.image(0).cpu(), torch.from_numpy(np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB"))))
    except ImportError:
        pass
    return res, best["whole"]


def main():
    B, n, rr = arg("--batch", 256), arg("--iters", 100), arg("--restart-rows", 0)
    built = _lib.check_sources("tools/bench_jpeg.py")
    res = {"bench": "jpeg_decode", "device": torch.cuda.get_device_name(0), "sources": built, "iters": n, "restart_rows": rr}
    prep = ImagePrep(448, device=DEV)
    times = {}
    dirs = [a for a in sys.argv[1:] if os.path.isdir(a)]
    if dirs:
        paths = sorted(glob.glob(os.path.join(dirs[0], "*.jpg")))
        files = [open(paths[i % len(paths)], "rb").read() for i in range(B)]
        res["files"], times["files"] = case(prep, files, n)
    else:
        for name, (w, h) in (("500x375", (500, 375)), ("1024x768", (1024, 768))):
            files = encode(w, h, B, rr)
            res[name], times[name] = case(prep, files, n)
            if "--split" in sys.argv:
                at = sys.argv.index("--split") + 1
                chunk = int(sys.argv[at]) if at < len(sys.argv) and sys.argv[at].isdigit() else True
                want = prep.decode_jpeg(files).pixels
                key = name + "_split"
                res[key], times[key] = case_split(ImagePrep(448, device=DEV, split=chunk), files, n, want)
            if "--layouts" in sys.argv and name == "500x375":
                on = ImagePrep(448, device=DEV, layouts=True)
                res[name + "_layouts_on"], times[name + "_layouts_on"] = case_layouts(on, files, n, prep.decode_jpeg(files).pixels)
                res[name + "_rst1"], times[name + "_rst1"] = case(prep, encode(w, h, B, 1), n)
                for key, fs in layout_files(w, h, B).items():
                    res[name + "_" + key], times[name + "_" + key] = case_layouts(on, fs, n)
            if "--progressive" in sys.argv:
                key = name + "_progressive"
                res[key], times[key] = case_progressive(ImagePrep(448, device=DEV, progressive=True), encode(w, h, B, rr, True), n)
    if "--no-trunks" not in sys.argv:
        obj = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet101(), 1)).to(DEV).eval()
        place = trunk.ResNetFeatures(synth.fill_trunk_(trunk.resnet50(365), 2)).to(DEV).eval()
        img = torch.randn(B, 3, 448, 448, device=DEV)
        with torch.no_grad():
            t = timeit(lambda: (obj(img), place(img)), 10, warm=2)
        res["trunks_eval_us"] = round(t, 1)
        res["ratio_to_trunks"] = {k: round(v / t, 3) for k, v in times.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
