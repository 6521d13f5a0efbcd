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

Decoding stays the caller's: an image is a [H,W,3] uint8 array, or anything with __array_interface__ (a PIL image in mode RGB).
This module does not import PIL."""
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


class _Slot:
    """One batch's pinned staging: the packed pixels and the descriptors."""

    def __init__(self, pin):
        self.pin = pin
        self.pix = torch.empty(0, dtype=torch.uint8)
        self.desc = torch.empty(0, ops.IMAGE_DESC, dtype=torch.int64)
        self.done = torch.cuda.Event() if pin else None

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


class ImagePrep:
    def __init__(self, size=448, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None, scales=SCALES,
                 max_distort=MAX_DISTORT, ring=2):
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
