"""numpy restatement of the image transforms (mgnns_amd/images.py, csrc/image_prep.hip): Pillow's 8-bit bilinear resize as
integer arithmetic, the crop as a sub-array, the flip, and ToTensor + Normalize as a table.  Shared by test_image_prep_cpu.py and
test_image_prep_gpu.py; written independently of mgnns_amd.images (scalar Python floats, which are C doubles) and without PIL.

Per axis, input extent n (the CROPPED extent), output extent S:
    scale = n / S; fs = max(scale, 1); support = fs
    center = (i + 0.5) * scale; lo = max(0, int(center - support + 0.5)); hi = min(n, int(center + support + 0.5))
    w_j = max(0, 1 - |(j + lo - center + 0.5) / fs|), divided by their sequential sum; k_j = int(w_j * 2^22 + 0.5)
A pass is clip(0, 255, (2^21 + sum_j k_j * pixel_j) >> 22) in int32, stored as uint8; the horizontal pass runs first, over every
source row, the vertical pass over its uint8 result."""
import numpy as np
import torch

BITS = 22


def plan(n, S):
    """-> (lo [S], cnt [S], taps: list of S int lists)"""
    scale = n / S
    fs = max(scale, 1.0)
    support = fs
    los, cnts, taps = [], [], []
    for i in range(S):
        center = (i + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(n, int(center + support + 0.5))
        w = [max(0.0, 1.0 - abs((j + lo - center + 0.5) / fs)) for j in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        los.append(lo)
        cnts.append(hi - lo)
        taps.append([int(v * (1 << BITS) + 0.5) for v in w])
    return los, cnts, taps


def resize_axis1(a, S, wrong=None):
    """One pass along axis 1 of a uint8 [R, n, C] array -> uint8 [R, S, C]."""
    los, cnts, taps = plan(a.shape[1], S)
    out = np.empty((a.shape[0], S, a.shape[2]), dtype=np.uint8)
    half = 0 if wrong == "no_half" else 1 << (BITS - 1)
    for i in range(S):
        k = np.asarray(taps[i], dtype=np.int64)
        acc = half + np.tensordot(a[:, los[i]:los[i] + cnts[i], :].astype(np.int64), k, axes=([1], [0]))
        assert acc.max() < 2 ** 31                       # the kernel and Pillow accumulate in int32
        out[:, i, :] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(img, S_h, S_w, wrong=None):
    """Pillow's img.resize((S_w, S_h), BILINEAR) of a [H,W,3] uint8 array.  wrong: a deliberately wrong variant, for the tests that
    show the goldens can tell -- "vertical_first" swaps the passes, "no_half" drops the rounding term."""
    if wrong == "vertical_first":
        v = resize_axis1(img.transpose(1, 0, 2), S_h).transpose(1, 0, 2)
        return resize_axis1(v, S_w)
    h = resize_axis1(img, S_w, wrong)
    return resize_axis1(h.transpose(1, 0, 2), S_h, wrong).transpose(1, 0, 2)


def table(mean, std):
    v = torch.arange(256)
    return torch.stack([v.float().div(255).sub(m).div(s) for m, s in zip(mean, std)])


def prep(img, S_h, S_w, tab, crop=None, flip=False, wrong=None):
    """One image through crop ((crop_w, crop_h, offset_w, offset_h) or None) -> resize -> flip -> table: fp32 [3,S_h,S_w] tensor."""
    if crop is not None:
        cw, ch, ox, oy = crop
        img = img[oy:oy + ch, ox:ox + cw]
    r = resize(np.ascontiguousarray(img), S_h, S_w, wrong)
    if flip:
        r = r[:, ::-1]
    idx = torch.from_numpy(r.transpose(2, 0, 1).copy()).long()
    return torch.stack([tab[c][idx[c]] for c in range(3)])


def prep_batch(images, S_h, S_w, tab, crops=None, flips=None):
    if not images:
        return torch.empty(0, 3, S_h, S_w)
    return torch.stack([prep(im, S_h, S_w, tab, None if crops is None else crops[i], bool(flips[i]) if flips is not None else False)
                        for i, im in enumerate(images)])
