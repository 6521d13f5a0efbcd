"""Image batches in front of the trunks: the reference's transforms, from decoded uint8 pixels to the [B,3,S,S] fp32 tensor
the stem reads, in ONE HIP launch per batch (csrc/image_prep.hip).

    eval   (utils/Multi_GCN_Co_att_dataset.py:259-264):        Warp(S) -> ToTensor -> Normalize
    train  (engine/Multi_GCN_Multihead_Att_engine.py:273-299): MultiScaleCrop(S, scales, max_distort=2)
                                                               -> RandomHorizontalFlip -> ToTensor -> Normalize

Both resizes are PIL.Image.resize(..., BILINEAR) (utils/util.py:67-146).  On 8-bit channels that is integer arithmetic with
22-bit fixed-point taps; this module computes the taps on the host in float64 exactly as Pillow's precompute_coeffs /
normalize_coeffs_8bpc do (build_plan) and the kernel runs Pillow's two passes, horizontal first.  The result is Pillow's, bit
for bit, for extents 16..4096 with an aspect of at most 4:1 (tests/test_image_prep_cpu.py); far outside that domain Pillow may
run its passes in the other order (seen at 1000x7 -> 16 and 1000x8 -> 16) and the intermediate rounding then differs.

An image is a [H,W,3] uint8 array, or anything with __array_interface__ (a PIL image in mode RGB) -- or the bytes of a baseline JPEG
file, which decode_jpeg / warp_jpeg / train_jpeg decode on the GPU to exactly Pillow's pixels (csrc/jpeg_decode.hip):
the host only parses the markers.  ImagePrep(..., progressive=True) decodes progressive (SOF2) files as well (csrc/jpeg_progressive.hpp);
the switch is off by default, and a progressive file is then refused with reason 3 as before.  ImagePrep(..., split=True) decodes a
long baseline scan -- a file without restart markers is one -- on many lanes instead of one, to the same pixels (csrc/jpeg_split.hpp;
DESIGN.md 17, "Split scans"); off by default as well.  ImagePrep(..., layouts=True) also decodes the other component layouts of
SOF0 / SOF1 files -- CMYK and YCCK, RGB, 4:4:0, 4:1:1 and every other interleaved layout of 1, 3 or 4 components whose sampling
factors divide the largest -- to Pillow's convert('RGB') pixels (csrc/jpeg_layouts.hpp; DESIGN.md 17, "Other component layouts");
off by default, and such a file is then refused with reason 3, 6, 7, 8 or 9 as before.  This module does not import PIL."""
import math
import random

import numpy as np
import torch

from . import ops

SCALES = (1.0, 0.875, 0.75, 0.66, 0.5)        # ENGINE:276
MAX_DISTORT = 2
PRECISION_BITS = 22
ALIGN = 16                                     # every image starts on a 16-byte boundary; 16 bytes of slack end the buffer


def build_plan(n, S):
    """Pillow's bilinear coefficients for resizing an extent of n to S -> (bounds int32 [S,2] = (first source index, tap count),
    taps int32 [S,ksize] with 22 fractional bits, zero beyond the count).  float64 throughout, in Pillow's order of operations."""
    n, S = int(n), int(S)
    if n < 1 or S < 1:
        raise ValueError("build_plan: extents must be positive, got %d -> %d" % (n, S))
    scale = n / S
    fs = max(scale, 1.0)
    support = 1.0 * fs                          # the bilinear filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(S, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int) truncates towards zero, as astype does
    hi = np.minimum((center + support + 0.5).astype(np.int64), n)
    cnt = hi - lo
    j = np.arange(ksize, dtype=np.int64)
    x = np.abs(((j[None, :] + lo[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((x < 1.0) & (j[None, :] < cnt[:, None]), 1.0 - x, 0.0)
    ww = np.zeros(S, dtype=np.float64)
    for t in range(ksize):                      # the sequential sum Pillow normalises by
        ww += w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    taps = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)          # all weights are >= 0
    taps[j[None, :] >= cnt[:, None]] = 0
    return np.stack([lo, cnt], 1).astype(np.int32), taps


def normalize_table(mean, std):
    """[3,256] fp32: ToTensor + Normalize of every byte value, computed by torch's own ops and therefore exact by construction."""
    v = torch.arange(256, dtype=torch.uint8)
    return torch.stack([v.float().div(255).sub(float(m)).div(float(s)) for m, s in zip(mean, std)])


def sample_crop(width, height, size=448, scales=SCALES, max_distort=MAX_DISTORT):
    """MultiScaleCrop._sample_crop_size with fix_crop and more_fix_crop (utils/util.py:96-146) on Python's `random`: the same two
    random.choice calls over lists built in the same order, so random.seed(k) gives the reference's crops.
    -> (crop_w, crop_h, offset_w, offset_h)"""
    base = min(width, height)
    sizes = [int(base * x) for x in scales]
    crop_h = [size if abs(x - size) < 3 else x for x in sizes]
    crop_w = [size if abs(x - size) < 3 else x for x in sizes]
    pairs = []
    for i, h in enumerate(crop_h):
        for j, w in enumerate(crop_w):
            if abs(i - j) <= max_distort:
                pairs.append((w, h))
    cw, ch = random.choice(pairs)
    ws, hs = (width - cw) // 4, (height - ch) // 4
    offsets = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs),
               (0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0),
               (ws, hs), (3 * ws, hs), (ws, 3 * hs), (3 * ws, 3 * hs)]
    ow, oh = random.choice(offsets)
    return cw, ch, ow, oh


def as_rgb8(img, i=0):
    """-> a [H,W,3] uint8 numpy view of one decoded image, or a refusal that says what to do."""
    if not isinstance(img, np.ndarray):
        if not hasattr(img, "__array_interface__"):
            raise TypeError("image %d: expected a [H,W,3] uint8 numpy array or an object with __array_interface__ (a PIL image in "
                            "mode RGB), got %s" % (i, type(img).__name__))
        img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError("image %d: pixels must be uint8, got %s -- decode to 8-bit RGB first (PIL: .convert('RGB'))" % (i, img.dtype))
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("image %d: expected [H,W,3] RGB, got shape %s -- grayscale, palette and RGBA images must be converted "
                         "first (PIL: .convert('RGB'))" % (i, tuple(img.shape)))
    H, W = img.shape[:2]
    if not (1 <= H <= ops.IMAGE_MAX_EXTENT and 1 <= W <= ops.IMAGE_MAX_EXTENT):
        raise ValueError("image %d: %dx%d is outside the supported extents 1..%d" % (i, W, H, ops.IMAGE_MAX_EXTENT))
    return img


# ---- JPEG files ------------------------------------------------------------------------------------------------------------
# the parser's reason codes (csrc/jpeg_parse.hpp)
JPEG_REASONS = {
    0: "accepted", 1: "not a JPEG file (no SOI marker)", 2: "malformed or truncated header", 3: "progressive or another unsupported SOFn frame",
    4: "arithmetic coding", 5: "12-bit samples or 16-bit quantisation tables", 6: "neither 1 nor 3 components (CMYK / YCCK)",
    7: "Adobe APP14 segment with transform 0 (RGB)", 8: "component ids R, G, B", 9: "sampling factors other than 4:4:4, 4:2:2, 4:2:0",
    10: "more than one scan, or a non-interleaved scan", 11: "height given by a DNL segment", 12: "extent out of range",
    13: "the scan refers to a table that is not defined"}
# further codes of the progressive parser (parse_jpeg(..., progressive=True)); JPEG_REASONS stays the baseline parser's own set
JPEG_PROGRESSIVE_REASONS = {
    14: "incomplete progression: at the end of the file a coefficient has not had its last bit (libjpeg would smooth it)",
    15: "illegal progression: Ss / Se / Ah / Al contradict T.81 G.1.1.1.1 or the scans before", 16: "more than 32 scans"}
# further codes of the layout parser (parse_jpeg(..., layouts=True))
JPEG_LAYOUT_REASONS = {
    17: "a sampling factor that is no integral fraction of the largest (libjpeg refuses it too)",
    18: "a sampling factor outside 1..4, or more than 10 blocks per MCU"}
JPEG_COLOUR_MODELS = ops.JPEG_COLOUR_MODELS
_JL = dict(reason=0, detail=1, width=2, height=3, ncomp=4, hmax=5, vmax=6, h=7, v=11, tq=15, td=19, ta=23, ri=27, restarts=28, nseg=29, mcux=30,
           mcuy=31, colour=32, sof=33, mcu_blocks=34)
_JPEG_LAYOUT_INFO_INTS = 40
_JI = dict(reason=0, detail=1, width=2, height=3, ncomp=4, hs=5, vs=6, tq=7, td=10, ta=13, ri=16, restarts=17, nseg=18, mcux=19, mcuy=20)


class UnsupportedJpeg(ValueError):
    """A batch holds files the GPU decoder refuses and no fallback was given.  refused: [(index, reason code)]."""

    def __init__(self, refused, details):
        self.refused = refused
        ValueError.__init__(self, "%d JPEG file(s) cannot be decoded on the GPU (pass fallback= to decode them yourself): %s" % (
            len(refused), "; ".join("image %d: %s (reason %d, found %s)"
                                   % (i, JPEG_REASONS.get(r) or JPEG_PROGRESSIVE_REASONS.get(r) or JPEG_LAYOUT_REASONS.get(r, "?"), r, d)
                                   for (i, r), d in zip(refused, details))))


def _file_bytes(f, i=0):
    if not isinstance(f, (bytes, bytearray, memoryview)):
        raise TypeError("file %d: expected bytes, bytearray or memoryview, got %s" % (i, type(f).__name__))
    return np.frombuffer(f, dtype=np.uint8)


_JS = dict(ns=0, comps=1, ss=2, se=3, ah=4, al=5, ri=6, level=7, dc=8, ac=11, seg0=12, nseg=13, units=14, begin=15, end=16, restarts=17)
JPEG_MAX_SCANS, _JPEG_SCAN_INTS, _JPEG_POOL_TABLES = 32, 18, 96


def _parse_progressive(a, max_extent, bufs=None):
    """mgnns_jpeg_parse_progressive on one file's bytes (a uint8 array) -> parse_jpeg's dict for a progressive file."""
    from . import _lib
    HB = ops.jpeg_huff_bytes()
    if bufs is None:
        bufs = (np.zeros((JPEG_MAX_SCANS, _JPEG_SCAN_INTS), np.int64), np.zeros((256, 4), np.int64), np.zeros((_JPEG_POOL_TABLES, HB), np.uint8))
    scans, seg, pool = bufs
    info = np.zeros(24, np.int32)
    quant = np.zeros(ops.JPEG_QSET, np.uint8)
    ptr = a.ctypes.data if a.size else None
    for _ in range(2):
        _lib.call("mgnns_jpeg_parse_progressive", ptr, a.size, int(max_extent or ops.IMAGE_MAX_EXTENT), info.ctypes.data, scans.ctypes.data,
                  seg.ctypes.data, seg.shape[0], pool.ctypes.data, quant.ctypes.data)
        if info[0] != 0 or info[_JI["nseg"]] <= seg.shape[0]:
            break
        seg = np.zeros((int(info[_JI["nseg"]]), 4), np.int64)
    out = dict(reason=int(info[0]), detail=int(info[1]))
    if out["reason"] == 0:
        for k in ("width", "height", "ncomp", "hs", "vs", "nseg", "mcux", "mcuy"):
            out[k] = int(info[_JI[k]])
        out["scans"] = []
        for r in scans[:int(info[21])]:
            d = {k: int(r[_JS[k]]) for k in ("ns", "ss", "se", "ah", "al", "ri", "level", "ac", "seg0", "nseg", "units", "restarts")}
            d["comps"] = [c for c in range(3) if int(r[_JS["comps"]]) >> c & 1]
            d["dc"] = [int(v) for v in r[_JS["dc"]:_JS["dc"] + 3]]
            d["ecs"] = (int(r[_JS["begin"]]), int(r[_JS["end"]]))
            out["scans"].append(d)
        out["levels"] = int(info[23])
        out["segments"] = seg[:out["nseg"]].copy()
        out["pool"] = [pool[t].tobytes() for t in range(int(info[22]))]
        out["quant"] = quant.tobytes()
    return out


def _parse_layout(a, max_extent, seg=None):
    """mgnns_jpeg_parse_layout on one file's bytes (a uint8 array) -> parse_jpeg's dict for a file of another component layout."""
    from . import _lib
    info = np.zeros(_JPEG_LAYOUT_INFO_INTS, np.int32)
    rng = np.zeros(2, np.int64)
    tables = np.zeros(ops.jpeg_tableset_bytes(), np.uint8)
    seg = np.zeros((64, 2), np.int64) if seg is None else seg
    ptr = a.ctypes.data if a.size else None
    for _ in range(2):
        _lib.call("mgnns_jpeg_parse_layout", ptr, a.size, int(max_extent or ops.IMAGE_MAX_EXTENT), info.ctypes.data, rng.ctypes.data,
                  seg.ctypes.data, seg.shape[0], tables.ctypes.data)
        if info[0] != 0 or info[_JL["nseg"]] <= seg.shape[0]:
            break
        seg = np.zeros((int(info[_JL["nseg"]]), 2), np.int64)
    out = dict(reason=int(info[0]), detail=int(info[1]))
    if out["reason"] == 0:
        for k in ("width", "height", "ncomp", "hmax", "vmax", "ri", "restarts", "nseg", "mcux", "mcuy", "colour", "sof", "mcu_blocks"):
            out[k] = int(info[_JL[k]])
        for k in ("h", "v", "tq", "td", "ta"):
            out[k] = [int(x) for x in info[_JL[k]:_JL[k] + out["ncomp"]]]
        out["layout"] = True
        out["ecs"] = (int(rng[0]), int(rng[1]))
        out["segments"] = seg[:out["nseg"]].copy()
        out["tables"] = tables.tobytes()
    return out


def parse_jpeg(data, max_extent=None, _seg=None, progressive=False, _bufs=None, layouts=False):
    """The host parser (mgnns_jpeg_parse: no GPU call) on one file's bytes -> dict: reason (0 = accepted), detail, and for an accepted
    file width, height, ncomp, hs, vs (Y's sampling), tq / td / ta (table ids per component), ri, restarts (markers found), nseg, mcux,
    mcuy, ecs (begin, end), segments (int64 [nseg,2] byte ranges) and tables (the table set's bytes).

    progressive=True also accepts SOF2 files (mgnns_jpeg_parse_progressive, DESIGN.md 17, "Progressive files").  The dictionary then carries `scans`
    and `levels`: for a baseline file [] and 0 beside the fields above; for a progressive file the scans in file order -- each a dict
    of ns, comps (the frame's components in it), ss, se, ah, al, ri (in units: MCUs, or blocks of its one component), level, dc (pool
    index of the DC table per frame component, -1 = none read), ac, seg0 / nseg (its rows of `segments`), units, ecs, restarts -- with
    width, height, ncomp, hs, vs, mcux, mcuy, nseg (of all scans), segments (int64 [nseg,4]: begin, end, first unit, units), pool (the
    distinct Huffman tables' bytes) and quant (192 bytes: per component the quantisation table in force at its first scan).  Scans
    of one level touch different coefficients and decode at the same time; levels run in order.

    layouts=True hands a file the baseline parser has refused with reason 3 (detail 0xC1: SOF1), 6, 7, 8 or 9 to the layout parser
    (mgnns_jpeg_parse_layout, DESIGN.md 17, "Other component layouts").  An accepted one has layout=True, width, height, ncomp (1, 3 or
    4), hmax, vmax, h / v / tq / td / ta (per component), colour (JPEG_COLOUR_MODELS), sof, mcu_blocks, ri, restarts, nseg, mcux, mcuy
    (MCUs of 8 hmax x 8 vmax pixels), ecs, segments and tables; a refused one a reason of JPEG_REASONS or JPEG_LAYOUT_REASONS.  A file
    the baseline parser accepts is the baseline parser's, with the dictionary it always had."""
    from . import _lib
    a = _file_bytes(data)
    info = np.zeros(24, np.int32)
    rng = np.zeros(2, np.int64)
    tables = np.zeros(ops.jpeg_tableset_bytes(), np.uint8)
    seg = np.zeros((64, 2), np.int64) if _seg is None else _seg
    ptr = a.ctypes.data if a.size else None
    _lib.call("mgnns_jpeg_parse", ptr, a.size, int(max_extent or ops.IMAGE_MAX_EXTENT), info.ctypes.data, rng.ctypes.data, seg.ctypes.data,
              seg.shape[0], tables.ctypes.data)
    if info[0] == 0 and info[_JI["nseg"]] > seg.shape[0]:
        seg = np.zeros((int(info[_JI["nseg"]]), 2), np.int64)
        _lib.call("mgnns_jpeg_parse", ptr, a.size, int(max_extent or ops.IMAGE_MAX_EXTENT), info.ctypes.data, rng.ctypes.data,
                  seg.ctypes.data, seg.shape[0], tables.ctypes.data)
    out = dict(reason=int(info[0]), detail=int(info[1]))
    if out["reason"] == 0:
        for k in ("width", "height", "ncomp", "hs", "vs", "ri", "restarts", "nseg", "mcux", "mcuy"):
            out[k] = int(info[_JI[k]])
        for k in ("tq", "td", "ta"):
            out[k] = [int(v) for v in info[_JI[k]:_JI[k] + 3]]
        out["ecs"] = (int(rng[0]), int(rng[1]))
        out["segments"] = seg[:out["nseg"]].copy()
        out["tables"] = tables.tobytes()
        if progressive:
            out["scans"], out["levels"] = [], 0
    elif progressive and out["reason"] == 3 and out["detail"] == 0xC2:
        return _parse_progressive(a, max_extent, _bufs)
    elif layouts and (out["reason"] in (6, 7, 8, 9) or (out["reason"] == 3 and out["detail"] == 0xC1)):
        return _parse_layout(a, max_extent, _seg)
    return out


class DecodedBatch:
    """What decode_jpeg returns; unpacks as (pixels, sizes, offsets).  pixels: uint8 on the device, every image interleaved RGB8 at
    its 16-byte-aligned offset, padding and 16 bytes of slack zero -- pack()'s layout; sizes: host int64 [B,2] (H, W); offsets: host
    int64 [B]."""

    def __init__(self, pixels, sizes, offsets):
        self.pixels, self.sizes, self.offsets = pixels, sizes, offsets

    def __iter__(self):
        return iter((self.pixels, self.sizes, self.offsets))

    def __len__(self):
        return int(self.sizes.shape[0])

    def image(self, i):
        """Image i as a [H,W,3] uint8 device tensor (a view of pixels)."""
        H, W = (int(v) for v in self.sizes[i])
        o = int(self.offsets[i])
        return self.pixels[o:o + H * W * 3].view(H, W, 3)


class _Slot:
    """One batch's pinned staging: the packed pixels and the descriptors."""

    def __init__(self, pin):
        self.pin = pin
        self.pix = torch.empty(0, dtype=torch.uint8)
        self.desc = torch.empty(0, ops.IMAGE_DESC, dtype=torch.int64)
        self.done = torch.cuda.Event() if pin else None
        self.raw = torch.empty(0, dtype=torch.uint8)          # JPEG batches: the files' bytes, the table sets, fall-back pixels
        self.rec = torch.empty(0, dtype=torch.int64)          # ... and the image and segment records

    def reserve_jpeg(self, nbytes, nrec):
        if self.raw.numel() < nbytes:
            self.raw = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=self.pin)
        if self.rec.numel() < nrec:
            self.rec = torch.empty(nrec + nrec // 4, dtype=torch.int64, pin_memory=self.pin)

    def reserve(self, nbytes, B):
        if self.pix.numel() < nbytes:
            self.pix = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=self.pin)
        if self.desc.shape[0] < B:
            self.desc = torch.empty(B + B // 4, ops.IMAGE_DESC, dtype=torch.int64, pin_memory=self.pin)


class Packed:
    """What pack() staged: `pixels` (uint8 host tensor, every image 16-byte aligned, 16 bytes of slack at the end), `desc` ([B,10]
    int64 host tensor, ops.image_prep's layout) and the slot they live in."""

    def __init__(self, pixels, desc, slot):
        self.pixels, self.desc, self.slot = pixels, desc, slot


def split_chunk(split):
    """ImagePrep's `split` argument -> the chunk size in bytes: 0 / False is off, True the default chunk (ops.JPEG_SPLIT_CHUNK), an
    integer a chunk size -- a multiple of 8 in 8..65536."""
    if split is None or split is False or (not isinstance(split, bool) and isinstance(split, int) and split == 0):
        return 0
    if split is True:
        return ops.JPEG_SPLIT_CHUNK
    if not isinstance(split, int) or split < 8 or split > 65536 or split % 8:
        raise ValueError("split must be False / 0 (off), True (chunks of %d bytes) or a chunk size, a multiple of 8 in 8..65536; got %r"
                         % (ops.JPEG_SPLIT_CHUNK, split))
    return split


class ImagePrep:
    def __init__(self, size=448, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None, scales=SCALES,
                 max_distort=MAX_DISTORT, ring=2, progressive=False, split=0, layouts=False):
        size = int(size)
        if not 1 <= size <= ops.IMAGE_MAX_SIZE:
            raise ValueError("size must be in 1..%d, got %d" % (ops.IMAGE_MAX_SIZE, size))
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std must have one entry per RGB channel")
        if any(float(s) == 0.0 for s in std):
            raise ValueError("std must be non-zero")
        if int(ring) < 2:
            raise ValueError("the pinned ring needs at least two batches, got %d" % ring)
        self.size = size
        self.progressive = bool(progressive)         # decode_jpeg / warp_jpeg / train_jpeg also decode progressive (SOF2) files
        self.split = split_chunk(split)              # ... and decode long baseline scans on many lanes, in chunks of so many bytes (0: off)
        self.layouts = bool(layouts)                 # ... and CMYK, YCCK, RGB, 4:4:0, 4:1:1 and the other interleaved layouts
        self.scales, self.max_distort = tuple(scales), int(max_distort)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise ValueError("ImagePrep runs on the GPU only (no CPU path); device=%s" % (device,))
        self.table = normalize_table(mean, std)
        self.table_dev = None if self.device is None else self.table.to(self.device)
        pin = self.device is not None and torch.cuda.is_available()
        self._ring = [_Slot(pin) for _ in range(int(ring))]
        self._next = 0
        # plans, cached by (extent, size): index into plan_table; plan_data is the concatenation of (bounds, taps)
        self._plan_index = {}
        self._plan_rows = []
        self._plan_chunks = []
        self._plan_ints = 0
        self._host_table = self.plan_table()
        self._dev_table, self._dev_data, self._dev_plans, self._dev_ints, self._retired = None, None, 0, 0, []
        self.last_crops, self.last_flips = None, None

    # ---- plans -------------------------------------------------------------------------------------------------------------
    def plan(self, extent):
        """Index of the plan for (extent, size), built on first use."""
        key = (int(extent), self.size)
        idx = self._plan_index.get(key)
        if idx is None:
            bounds, taps = build_plan(*key)
            idx = len(self._plan_rows)
            self._plan_rows.append((self._plan_ints, taps.shape[1], key[0], key[1]))
            self._plan_chunks += [bounds.reshape(-1), taps.reshape(-1)]
            self._plan_ints += bounds.size + taps.size
            self._plan_index[key] = idx
        return idx

    def plan_table(self):
        return torch.tensor(self._plan_rows, dtype=torch.int32).reshape(len(self._plan_rows), 4)

    def plan_data(self):
        return torch.from_numpy(np.concatenate(self._plan_chunks)) if self._plan_chunks else torch.empty(0, dtype=torch.int32)

    def _plans_on_device(self):
        """(plan_table host [P,4], its device copy, plan_data on the device).  The device copies live in buffers with room to spare:
        a batch that brings new plans appends only those -- one pinned, asynchronous copy each for their data and their table
        rows, on the current stream -- and a full buffer is replaced by one of twice the size, its contents copied on the device
        (the old one is kept: a captured graph may hold its address).  The cache only grows: a plan is (2 + ksize) * size
        int32, about 16 KB at 448 for a photograph's extents, and there are at most 8192 extents."""
        P, n = len(self._plan_rows), self._plan_ints
        if self._dev_table is None or P > self._dev_table.shape[0] or n > self._dev_data.numel():
            table = torch.empty(max(64, 2 * P), 4, dtype=torch.int32, device=self.device)
            data = torch.empty(max(1 << 18, 2 * n), dtype=torch.int32, device=self.device)
            if self._dev_plans:
                table[:self._dev_plans].copy_(self._dev_table[:self._dev_plans])
                data[:self._dev_ints].copy_(self._dev_data[:self._dev_ints])
                self._retired.append((self._dev_table, self._dev_data))
            self._dev_table, self._dev_data = table, data
        if P > self._dev_plans:
            rows = torch.tensor(self._plan_rows[self._dev_plans:], dtype=torch.int32).pin_memory()
            tail = torch.from_numpy(np.concatenate(self._plan_chunks[2 * self._dev_plans:])).pin_memory()
            self._dev_table[self._dev_plans:P].copy_(rows, non_blocking=True)      # (torch frees a pinned tensor only after its copy ran)
            self._dev_data[self._dev_ints:n].copy_(tail, non_blocking=True)
            self._dev_plans, self._dev_ints = P, n
            self._host_table = self.plan_table()
        return self._host_table, self._dev_table[:P], self._dev_data[:n]

    # ---- host staging ------------------------------------------------------------------------------------------------------
    def pack(self, images, crops=None, flips=None):
        """Stage one batch into the next slot of the pinned ring: pixels packed at 16-byte starts, one descriptor per image,
        plans de-duplicated.  crops: (crop_w, crop_h, offset_w, offset_h) per image (None = the whole image); flips: bool per
        image.  -> Packed"""
        arrs = [as_rgb8(im, i) for i, im in enumerate(images)]
        B = len(arrs)
        if crops is not None and len(crops) != B or flips is not None and len(flips) != B:
            raise ValueError("crops / flips must have one entry per image")
        offs, total = [], 0
        for a in arrs:
            offs.append(total)
            total += (a.shape[0] * a.shape[1] * 3 + ALIGN - 1) // ALIGN * ALIGN
        total += ALIGN
        rows = []
        for i, a in enumerate(arrs):
            H, W = a.shape[:2]
            cw, ch, cx, cy = (W, H, 0, 0) if crops is None else (int(v) for v in crops[i])
            if cw < 1 or ch < 1 or cx < 0 or cy < 0 or cx + cw > W or cy + ch > H:
                raise ValueError("image %d: crop (w=%d, h=%d, x=%d, y=%d) is not inside the %dx%d image" % (i, cw, ch, cx, cy, W, H))
            rows.append((offs[i], H, W, cx, cy, cw, ch, 1 if (flips is not None and bool(flips[i])) else 0, self.plan(cw), self.plan(ch)))
        slot = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if slot.done is not None:
            slot.done.synchronize()              # the slot's previous H2D copies have left the pinned buffers
        slot.reserve(total, B)
        pix = slot.pix.numpy()
        for a, o, end in zip(arrs, offs, offs[1:] + [total]):
            nb = a.shape[0] * a.shape[1] * 3
            np.copyto(pix[o:o + nb].reshape(a.shape), a)
            pix[o + nb:end] = 0                  # the padding up to the next start; behind the last image, the 16 bytes of slack too
        if not arrs:
            pix[:total] = 0
        desc = slot.desc[:B]
        if B:
            desc.numpy()[:] = np.asarray(rows, dtype=np.int64)
        return Packed(slot.pix[:total], desc, slot)

    # ---- the transforms ----------------------------------------------------------------------------------------------------
    def _run(self, images, crops, flips):
        if self.device is None:
            raise RuntimeError("ImagePrep was built without a device: the transforms run on the GPU only (no CPU path)")
        p = self.pack(images, crops, flips)
        with torch.cuda.device(self.device):
            table, table_dev, data_dev = self._plans_on_device()
            pix_dev = torch.empty(p.pixels.numel(), dtype=torch.uint8, device=self.device)
            desc_dev = torch.empty(p.desc.shape, dtype=torch.int64, device=self.device)
            pix_dev.copy_(p.pixels, non_blocking=True)           # one H2D per buffer, on the current stream
            desc_dev.copy_(p.desc, non_blocking=True)
            p.slot.done.record()
            return ops.image_prep(pix_dev, p.desc, desc_dev, table, table_dev, data_dev, self.table_dev, self.size, self.size)

    def warp(self, images):
        """The eval transform: Warp(size) -> ToTensor -> Normalize.  images: a list of [H,W,3] uint8 arrays (or objects with
        __array_interface__) -> [B,3,size,size] fp32 on the device."""
        return self._run(list(images), None, None)

    def sample_crop(self, width, height):
        return sample_crop(width, height, self.size, self.scales, self.max_distort)

    def check_croppable(self, width, height, i=0):
        """MultiScaleCrop snaps a candidate crop within 3 pixels of `size` to `size` (utils/util.py:102-103).  On an image whose
        short side is size - 2 or size - 1 that candidate is larger than the image; the reference lets Pillow pad it with black
        when it is drawn.  There is no padding here: such an image is refused, whatever the draw would have been."""
        base = min(width, height)
        if any(abs(int(base * x) - self.size) < 3 and self.size > base for x in self.scales):
            raise ValueError("image %d: %dx%d has a short side of %d, which MultiScaleCrop(%d) may crop to %d pixels -- larger than "
                             "the image (the reference pads with black); resize or pad the image first, or pass crops="
                             % (i, width, height, base, self.size, self.size))

    def train(self, images, crops=None, flips=None):
        """The training transform: MultiScaleCrop -> RandomHorizontalFlip -> ToTensor -> Normalize.  crops ((crop_w, crop_h,
        offset_w, offset_h) per image) and flips (bool per image) are sampled as the reference samples them when not given:
        per image, the crop from Python's `random`, then the flip as torch.rand(1) < 0.5.  The samples of the last call are
        kept in last_crops / last_flips.  An image on which a sampled crop could be larger than the image (check_croppable: a
        short side of size - 2 or size - 1) raises ValueError before anything is drawn, so a run never depends on the draw."""
        images = list(images)
        if crops is None or flips is None:
            arrs = [as_rgb8(im, i) for i, im in enumerate(images)]
            if crops is None:
                for i, a in enumerate(arrs):
                    self.check_croppable(a.shape[1], a.shape[0], i)
            sc, sf = [], []
            for i, a in enumerate(arrs):
                sc.append(self.sample_crop(a.shape[1], a.shape[0]) if crops is None else tuple(crops[i]))
                sf.append(bool(torch.rand(1) < 0.5) if flips is None else bool(flips[i]))
            crops, flips = sc, sf
        self.last_crops, self.last_flips = [tuple(int(v) for v in c) for c in crops], [bool(f) for f in flips]
        return self._run(images, self.last_crops, self.last_flips)

    # ---- JPEG files --------------------------------------------------------------------------------------------------------
    def _jpeg_headers(self, files, fallback):
        """Parse every file on the host (no GPU work).  Refused files go to `fallback` -- or raise UnsupportedJpeg, all of them in
        one exception.  -> (files, parsed, {index: fall-back pixels}, [(W, H)])"""
        files = list(files)
        seg = np.zeros((1024, 2), np.int64)
        bufs = None
        if self.progressive:
            bufs = (np.zeros((JPEG_MAX_SCANS, _JPEG_SCAN_INTS), np.int64), np.zeros((1024, 4), np.int64),
                    np.zeros((_JPEG_POOL_TABLES, ops.jpeg_huff_bytes()), np.uint8))
        parsed, refused = [], []
        for i, f in enumerate(files):
            _file_bytes(f, i)
            parsed.append(parse_jpeg(f, _seg=seg, progressive=self.progressive, _bufs=bufs, layouts=self.layouts))
            if parsed[-1]["reason"]:
                refused.append((i, parsed[-1]["reason"]))
        if refused and fallback is None:
            raise UnsupportedJpeg(refused, [parsed[i]["detail"] for i, _ in refused])
        arrays = {i: as_rgb8(fallback(files[i]), i) for i, _ in refused}
        sizes = [(arrays[i].shape[1], arrays[i].shape[0]) if i in arrays else (p["width"], p["height"]) for i, p in enumerate(parsed)]
        return files, parsed, arrays, sizes

    def _jpeg_run(self, headers, crops=None, flips=None, prep=False, staged_only=False):
        """Stage one batch of parsed files into the next slot of the pinned ring -- the files' bytes, the distinct table sets, the
        image and segment records, the pixels of fall-back images -- copy them over and decode.  With prep=True the descriptors of
        (crops, flips) follow and image_prep runs on the decoded buffer.  -> DecodedBatch, or the [B,3,size,size] tensor.
        staged_only=True stops before the decode and returns (ops.jpeg_decode's arguments, DecodedBatch): tools/bench_jpeg.py
        (with progressive or split: ops.jpeg_decode_progressive's, which are ops.jpeg_decode_split's; with layouts:
        ops.jpeg_decode_layouts's)."""
        if self.device is None:
            raise RuntimeError("ImagePrep was built without a device: JPEG files are decoded on the GPU only (no CPU path)")
        files, parsed, arrays, sizes = headers
        B = len(files)
        if crops is not None and len(crops) != B or flips is not None and len(flips) != B:
            raise ValueError("crops / flips must have one entry per image")
        offs, total = [], 0
        for W, H in sizes:
            offs.append(total)
            total += (H * W * 3 + ALIGN - 1) // ALIGN * ALIGN
        total += ALIGN
        ends = offs[1:] + [total]
        desc_rows = []
        if prep:
            for i, (W, H) in enumerate(sizes):
                cw, ch, cx, cy = (W, H, 0, 0) if crops is None else (int(v) for v in crops[i])
                if cw < 1 or ch < 1 or cx < 0 or cy < 0 or cx + cw > W or cy + ch > H:
                    raise ValueError("image %d: crop (w=%d, h=%d, x=%d, y=%d) is not inside the %dx%d image" % (i, cw, ch, cx, cy, W, H))
                desc_rows.append((offs[i], H, W, cx, cy, cw, ch, 1 if (flips is not None and bool(flips[i])) else 0, self.plan(cw), self.plan(ch)))
        # layout of the raw buffer: the accepted files at 16-byte starts, the table sets, then the fall-back images' pixels
        TB = ops.jpeg_tableset_bytes()
        mixed = self.progressive or self.split > 0 or self.layouts     # the decode that takes the progressive arguments (maybe empty)
        HB = ops.jpeg_huff_bytes() if mixed else 0
        raw_off, n, sets, pool, qsets = {}, 0, {}, {}, {}
        for i, f in enumerate(files):
            if i not in arrays:
                raw_off[i] = n
                n += (_file_bytes(f).size + ALIGN - 1) // ALIGN * ALIGN
                if "pool" in parsed[i]:                                 # a progressive file: its tables go to the batch's pool
                    for t in parsed[i]["pool"]:
                        pool.setdefault(t, len(pool))
                    qsets.setdefault(parsed[i]["quant"], len(qsets))
                else:
                    sets.setdefault(parsed[i]["tables"], len(sets))
        tab_off = n
        n += len(sets) * TB
        pool_off = n
        n += len(pool) * HB
        q_off = n
        n += len(qsets) * ops.JPEG_QSET
        n_data = n
        fb_off = {}
        for i in arrays:
            fb_off[i] = n
            n += ends[i] - offs[i]
        img = np.zeros((B, ops.JPEG_IMG), np.int64)
        segs, psegs, lsegs, coef_off, plane_off = [], [], [], 0, 0
        for i, p in enumerate(parsed):
            W, H = sizes[i]
            if i in arrays:
                img[i] = (0, W, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, offs[i], ends[i])
                continue
            nmcu = p["mcux"] * p["mcuy"]
            if p.get("layout"):                  # another component layout: kind 3, segments of its own (never split)
                pack = lambda v, bits: sum(x << (bits * c) for c, x in enumerate(v))
                img[i] = (ops.JPEG_LAYOUT_KIND, W, H, p["ncomp"] | p["colour"] << 8, pack(p["h"], 4), pack(p["v"], 4), p["mcux"], p["mcuy"],
                          pack(p["tq"], 8), pack(p["td"], 8), pack(p["ta"], 8), sets[p["tables"]], coef_off, plane_off, offs[i], ends[i])
                coef_off += nmcu * p["mcu_blocks"] * 64
                plane_off += nmcu * p["mcu_blocks"] * 64
                s = np.empty((p["nseg"], ops.JPEG_SEG), np.int64)
                s[:, 0] = i
                s[:, 1:3] = p["segments"] + raw_off[i]
                s[:, 3] = np.arange(p["nseg"]) * p["ri"]
                s[:, 4] = np.minimum(p["ri"], nmcu - s[:, 3]) if p["ri"] else nmcu
                lsegs.append(s)
                continue
            blocks = nmcu if p["ncomp"] == 1 else nmcu * (p["hs"] * p["vs"] + 2)
            pack3 = lambda v: v[0] | v[1] << 8 | v[2] << 16
            if "pool" in p:                      # progressive: kind 2, the latched quantisation set, a record per segment of every scan
                img[i] = (2, W, H, p["ncomp"], p["hs"], p["vs"], p["mcux"], p["mcuy"], 0, 0, 0, qsets[p["quant"]], coef_off, plane_off,
                          offs[i], ends[i])
                coef_off += blocks * 64
                plane_off += blocks * 64
                at = [pool[t] for t in p["pool"]]
                s = np.empty((p["nseg"], ops.JPEG_PSEG + 1), np.int64)     # (the last column, the level, is the sort key)
                s[:, 0] = i
                s[:, 1:3] = p["segments"][:, :2] + raw_off[i]
                s[:, 3:5] = p["segments"][:, 2:]
                for k, sc in enumerate(p["scans"]):
                    rows = slice(sc["seg0"], sc["seg0"] + sc["nseg"])
                    tabs = 0
                    for j, t in enumerate(sc["dc"] + [sc["ac"]]):
                        tabs |= (0xFFFF if t < 0 else at[t]) << (16 * j)
                    s[rows, 5:] = (sum(1 << c for c in sc["comps"]), sc["ss"], sc["se"], sc["ah"], sc["al"],
                                   tabs - (1 << 64) if tabs >= 1 << 63 else tabs, k, sc["level"])
                psegs.append(s)
                continue
            img[i] = (1, W, H, p["ncomp"], p["hs"], p["vs"], p["mcux"], p["mcuy"], pack3(p["tq"]), pack3(p["td"]), pack3(p["ta"]),
                      sets[p["tables"]], coef_off, plane_off, offs[i], ends[i])
            coef_off += blocks * 64
            plane_off += blocks * 64
            s = np.empty((p["nseg"], ops.JPEG_SEG), np.int64)
            s[:, 0] = i
            s[:, 1:3] = p["segments"] + raw_off[i]
            s[:, 3] = np.arange(p["nseg"]) * p["ri"]
            s[:, 4] = np.minimum(p["ri"], nmcu - s[:, 3]) if p["ri"] else nmcu
            segs.append(s)
        seg = np.concatenate(segs) if segs else np.zeros((0, ops.JPEG_SEG), np.int64)
        S = seg.shape[0]
        pseg = np.concatenate(psegs) if psegs else np.zeros((0, ops.JPEG_PSEG + 1), np.int64)
        pseg = pseg[np.argsort(pseg[:, -1], kind="stable")]                # level by level; within a level image, scan, segment
        level_counts = np.bincount(pseg[:, -1]).tolist() if len(pseg) else []
        pseg = pseg[:, :ops.JPEG_PSEG]
        P = pseg.shape[0]
        lseg = np.concatenate(lsegs) if lsegs else np.zeros((0, ops.JPEG_SEG), np.int64)
        L = lseg.shape[0]
        lseg_at = B * ops.JPEG_IMG + S * ops.JPEG_SEG                       # the layout segments lie between seg and pseg
        nrec = lseg_at + L * ops.JPEG_SEG + P * ops.JPEG_PSEG

        slot = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if slot.done is not None:
            slot.done.synchronize()              # the slot's previous H2D copies have left the pinned buffers
        slot.reserve_jpeg(n, nrec)
        slot.reserve(0, B)
        raw = slot.raw.numpy()
        for i, f in enumerate(files):
            if i in arrays:
                a, o = arrays[i], fb_off[i]
                nb = a.shape[0] * a.shape[1] * 3
                np.copyto(raw[o:o + nb].reshape(a.shape), a)
                raw[o + nb:o + ends[i] - offs[i]] = 0
            else:
                o = raw_off[i]
                raw[o:o + _file_bytes(f).size] = _file_bytes(f)
        for t, k in sets.items():
            raw[tab_off + k * TB:tab_off + (k + 1) * TB] = np.frombuffer(t, np.uint8)
        for t, k in pool.items():
            raw[pool_off + k * HB:pool_off + (k + 1) * HB] = np.frombuffer(t, np.uint8)
        for t, k in qsets.items():
            raw[q_off + k * ops.JPEG_QSET:q_off + (k + 1) * ops.JPEG_QSET] = np.frombuffer(t, np.uint8)
        img_host = slot.rec[:B * ops.JPEG_IMG].view(B, ops.JPEG_IMG)
        seg_host = slot.rec[B * ops.JPEG_IMG:B * ops.JPEG_IMG + S * ops.JPEG_SEG].view(S, ops.JPEG_SEG)
        pseg_host = slot.rec[nrec - P * ops.JPEG_PSEG:nrec].view(P, ops.JPEG_PSEG)
        lseg_host = slot.rec[lseg_at:lseg_at + L * ops.JPEG_SEG].view(L, ops.JPEG_SEG)
        img_host.numpy()[:] = img
        seg_host.numpy()[:] = seg
        lseg_host.numpy()[:] = lseg
        pseg_host.numpy()[:] = pseg
        desc = slot.desc[:B]
        if prep and B:
            desc.numpy()[:] = np.asarray(desc_rows, dtype=np.int64)

        with torch.cuda.device(self.device):
            raw_dev = torch.empty(max(n_data, ALIGN), dtype=torch.uint8, device=self.device)
            rec_dev = torch.empty(max(nrec, 1), dtype=torch.int64, device=self.device)
            pix_dev = torch.empty(total, dtype=torch.uint8, device=self.device) if B else torch.zeros(total, dtype=torch.uint8, device=self.device)
            raw_dev[:n_data].copy_(slot.raw[:n_data], non_blocking=True)                # the files and the tables: one H2D
            rec_dev[:nrec].copy_(slot.rec[:nrec], non_blocking=True)
            for i in arrays:                                                             # fall-back images: their pixels, as pack stages them
                pix_dev[offs[i]:ends[i]].copy_(slot.raw[fb_off[i]:fb_off[i] + ends[i] - offs[i]], non_blocking=True)
            if prep:
                table, table_dev, data_dev = self._plans_on_device()
                desc_dev = torch.empty(desc.shape, dtype=torch.int64, device=self.device)
                desc_dev.copy_(desc, non_blocking=True)
            slot.done.record()
            img_dev = rec_dev[:B * ops.JPEG_IMG].view(B, ops.JPEG_IMG)
            seg_dev = rec_dev[B * ops.JPEG_IMG:B * ops.JPEG_IMG + S * ops.JPEG_SEG].view(S, ops.JPEG_SEG)
            tables_dev = raw_dev[tab_off:tab_off + len(sets) * TB].view(len(sets), TB)
            batch = DecodedBatch(pix_dev, torch.tensor([(H, W) for W, H in sizes], dtype=torch.int64).reshape(B, 2),
                                 torch.tensor(offs, dtype=torch.int64))
            if mixed:                            # the mixed decode: its further arguments
                pseg_dev = rec_dev[nrec - P * ops.JPEG_PSEG:nrec].view(P, ops.JPEG_PSEG)
                pool_dev = raw_dev[pool_off:pool_off + len(pool) * HB].view(len(pool), HB)
                qsets_dev = raw_dev[q_off:q_off + len(qsets) * ops.JPEG_QSET].view(len(qsets), ops.JPEG_QSET)
                lseg_dev = rec_dev[lseg_at:lseg_at + L * ops.JPEG_SEG].view(L, ops.JPEG_SEG)
            if staged_only:                      # (host records cloned: the slot is reused two batches later)
                if self.layouts:
                    return (raw_dev, img_host.clone(), img_dev, seg_host.clone(), seg_dev, tables_dev, pseg_host.clone(), pseg_dev, level_counts,
                            pool_dev, qsets_dev, lseg_host.clone(), lseg_dev, pix_dev), batch
                if mixed:
                    return (raw_dev, img_host.clone(), img_dev, seg_host.clone(), seg_dev, tables_dev, pseg_host.clone(), pseg_dev, level_counts,
                            pool_dev, qsets_dev, pix_dev), batch
                return (raw_dev, img_host.clone(), img_dev, seg_host.clone(), seg_dev, tables_dev, pix_dev), batch
            try:
                if self.layouts:
                    ops.jpeg_decode_layouts(raw_dev, img_host, img_dev, seg_host, seg_dev, tables_dev, pseg_host, pseg_dev, level_counts,
                                            pool_dev, qsets_dev, lseg_host, lseg_dev, pix_dev, chunk_bytes=self.split)
                elif self.split:
                    ops.jpeg_decode_split(raw_dev, img_host, img_dev, seg_host, seg_dev, tables_dev, pseg_host, pseg_dev, level_counts,
                                          pool_dev, qsets_dev, pix_dev, chunk_bytes=self.split)
                elif self.progressive:
                    ops.jpeg_decode_progressive(raw_dev, img_host, img_dev, seg_host, seg_dev, tables_dev, pseg_host, pseg_dev, level_counts,
                                                pool_dev, qsets_dev, pix_dev)
                else:
                    ops.jpeg_decode(raw_dev, img_host, img_dev, seg_host, seg_dev, tables_dev, pix_dev)
            except ops.JpegDecodeError as e:
                e.batch = batch                  # every image the error does not name is decoded in it
                raise
            if prep:
                return ops.image_prep(pix_dev, desc, desc_dev, table, table_dev, data_dev, self.table_dev, self.size, self.size)
        return batch

    def decode_jpeg(self, files, fallback=None):
        """Decode a batch of baseline JPEG files (bytes / bytearray / memoryview each) on the GPU to exactly the pixels Pillow's
        Image.open(...).convert('RGB') gives -> DecodedBatch (pixels on the device in pack()'s layout, host sizes [B,2] as (H, W),
        host offsets; .image(i) views one image).  The host parses the markers and copies the compressed bytes; raw pixels never
        cross PCIe.  A file outside the decoder's scope (progressive, CMYK, ...: JPEG_REASONS) raises UnsupportedJpeg before any GPU
        work -- or, with fallback=callable, is decoded by the caller: fallback(file bytes) -> a [H,W,3] uint8 array, staged into the
        same pixel buffer.  A file whose scan is corrupt raises ops.JpegDecodeError (a ValueError) after the decode, naming the
        image and the segment's status.  A prep built with progressive=True decodes progressive files as well, in any mix with
        baseline ones; the error then names the scan too, and files of its further reasons are in JPEG_PROGRESSIVE_REASONS.  A prep
        built with layouts=True decodes CMYK, YCCK, RGB, 4:4:0, 4:1:1 and the other interleaved layouts as well (JPEG_LAYOUT_REASONS)."""
        return self._jpeg_run(self._jpeg_headers(files, fallback))

    def warp_jpeg(self, files, fallback=None):
        """warp() of the decoded files: one decode launch sequence and one image_prep launch -> [B,3,size,size] fp32."""
        return self._jpeg_run(self._jpeg_headers(files, fallback), None, None, prep=True)

    def train_jpeg(self, files, crops=None, flips=None, fallback=None):
        """train() of the decoded files.  Crops and flips are sampled from the header sizes exactly as train samples them from the
        arrays' -- check_croppable on every image first, then per image the crop and the flip -- and kept in last_crops / last_flips."""
        headers = self._jpeg_headers(files, fallback)
        sizes = headers[3]
        if crops is None or flips is None:
            if crops is None:
                for i, (W, H) in enumerate(sizes):
                    self.check_croppable(W, H, i)
            sc, sf = [], []
            for i, (W, H) in enumerate(sizes):
                sc.append(self.sample_crop(W, H) if crops is None else tuple(crops[i]))
                sf.append(bool(torch.rand(1) < 0.5) if flips is None else bool(flips[i]))
            crops, flips = sc, sf
        self.last_crops, self.last_flips = [tuple(int(v) for v in c) for c in crops], [bool(f) for f in flips]
        return self._jpeg_run(headers, self.last_crops, self.last_flips, prep=True)
