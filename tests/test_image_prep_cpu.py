"""The image transforms without a GPU (mgnns_amd/images.py): the numpy restatement the GPU test compares the kernel with equals the
reference's recorded outputs (tests/golden/image_prep.npz, tools/gen_image_goldens.py) and live Pillow bit for bit; the host side
-- coefficient plans, crop sampling, the normalisation table, the packing of a batch, every refusal -- is checked directly."""
import random

import numpy as np
import pytest
import torch

from mgnns_amd import images as I
from mgnns_amd import ops
from tests import helpers as H
from tests import image_prep_ref as R

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.fixture(scope="module")
def gold():
    return H.load_golden("image_prep.npz")


def n_sources(g):
    return sum(1 for k in g.keys() if k.startswith("src_"))


def test_restatement_equals_every_golden(gold):
    S = int(gold["size"])
    assert n_sources(gold) >= 4
    for i in range(n_sources(gold)):
        assert np.array_equal(R.resize(gold["src_%d" % i], S, S), gold["warp_%d" % i]), "Warp, image %d" % i
    for s in gold["seeds"]:
        for i in gold["crop_images"]:
            cw, ch, ox, oy = (int(v) for v in gold["crop_s%d_i%d" % (s, i)])
            got = R.resize(np.ascontiguousarray(gold["src_%d" % i][oy:oy + ch, ox:ox + cw]), S, S)
            assert np.array_equal(got, gold["cropout_s%d_i%d" % (s, i)]), "MultiScaleCrop, seed %d image %d" % (s, i)
    s, i = (int(v) for v in gold["flip"])
    cw, ch, ox, oy = (int(v) for v in gold["crop_s%d_i%d" % (s, i)])
    got = R.resize(np.ascontiguousarray(gold["src_%d" % i][oy:oy + ch, ox:ox + cw]), S, S)[:, ::-1]
    assert np.array_equal(got, gold["flipout"])


@pytest.mark.parametrize("wrong", ["vertical_first", "no_half"])
def test_goldens_tell_a_wrong_resize(gold, wrong):
    """The goldens are sharp enough: running the vertical pass first, or dropping the rounding term 2^21, changes pixels of every
    recorded Warp output."""
    S = int(gold["size"])
    for i in range(n_sources(gold)):
        assert not np.array_equal(R.resize(gold["src_%d" % i], S, S, wrong), gold["warp_%d" % i]), i


def test_restatement_equals_live_pillow():
    """Fixed-seed sweep against PIL.Image.resize and crop().resize(): extents 16..1024, aspect at most 4:1, S in {16, 30, 32, 64},
    random crops, planes saturated at 0 and 255; then the sizes of real photographs at 448, up to 4000 x 3000, and the domain's
    largest extent, 4096, on either axis at its largest aspect."""
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(7)
    n = 0
    for case in range(110):
        w = int(rs.randint(16, 1025))
        h = int(np.clip(rs.randint(max(16, w // 4), min(1024, 4 * w) + 1), 16, 1024))
        S = int(rs.choice([16, 30, 32, 64]))
        a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        if case % 5 == 0:
            a[..., case % 3] = 0
            a[..., (case + 1) % 3] = 255
        if case % 2:
            cw, ch = int(rs.randint(16, w + 1)), int(rs.randint(16, h + 1))
            cw, ch = min(w, max(cw, (ch + 3) // 4)), min(h, max(ch, (cw + 3) // 4))    # the crop keeps to the aspect domain as well
            ox, oy = int(rs.randint(0, w - cw + 1)), int(rs.randint(0, h - ch + 1))
            want = np.asarray(Image.fromarray(a).crop((ox, oy, ox + cw, oy + ch)).resize((S, S), Image.BILINEAR))
            got = R.resize(np.ascontiguousarray(a[oy:oy + ch, ox:ox + cw]), S, S)
        else:
            want = np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR))
            got = R.resize(a, S, S)
        assert np.array_equal(got, want), (case, w, h, S)
        n += 1
    for (w, h), S in (((333, 500), 448), ((500, 375), 448), ((1600, 1200), 448), ((3000, 2000), 448), ((4000, 3000), 448),
                      ((4096, 1024), 448), ((1024, 4096), 64), ((1, 1), 8), ((2, 3), 32), ((40, 40), 40)):
        a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(R.resize(a, S, S), np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR))), (w, h, S)
        n += 1
    assert n >= 100


def test_plans_equal_the_restatement():
    """build_plan (vectorised float64) against the restatement's scalar loop: bounds, taps and the zero fill, over every extent a
    kernel path changes at and the extremes the entry point accepts."""
    for n in list(range(1, 130)) + [333, 375, 500, 768, 1000, 1024, 3000, 4096, 8191, 8192]:
        for S in (1, 7, 16, 30, 33, 64, 448, 1024):
            bounds, taps = I.build_plan(n, S)
            lo, cnt, ref = R.plan(n, S)
            assert bounds.dtype == np.int32 and taps.dtype == np.int32 and bounds.shape == (S, 2)
            assert bounds[:, 0].tolist() == lo and bounds[:, 1].tolist() == cnt, (n, S)
            assert taps.shape[1] >= max(cnt) and (bounds[:, 0] + bounds[:, 1] <= n).all() and (bounds[:, 1] >= 1).all()
            for i in range(S):
                assert taps[i, :cnt[i]].tolist() == ref[i] and not taps[i, cnt[i]:].any(), (n, S, i)
    b, t = I.build_plan(40, 40)                  # identity: one tap of exactly 1.0
    assert (t[:, 0] == 1 << 22).all() and not t[:, 1:].any() and b[:, 0].tolist() == list(range(40))
    with pytest.raises(ValueError):
        I.build_plan(0, 4)


def test_sample_crop_reproduces_the_recorded_crops(gold):
    S = int(gold["size"])
    prep = I.ImagePrep(size=S)
    for s in gold["seeds"]:
        for i in gold["crop_images"]:
            h, w = gold["src_%d" % i].shape[:2]
            random.seed(int(s))
            assert prep.sample_crop(w, h) == tuple(int(v) for v in gold["crop_s%d_i%d" % (s, i)]), (s, i)
    random.seed(5)                               # two choices per crop, nothing else drawn
    prep.sample_crop(500, 375)
    state = random.getstate()
    random.seed(5)
    random.choice(range(19))
    random.choice(range(13))
    assert random.getstate() == state


def test_table_equals_the_torch_formula():
    tab = I.normalize_table(MEAN, STD)
    assert tab.shape == (3, 256) and tab.dtype == torch.float32
    v = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1).contiguous()
    x = v.float().div(255)                                                      # ToTensor of a [3,256,1] uint8 image
    want = (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)        # Normalize
    assert torch.equal(tab, want.view(3, 256)) and torch.equal(tab, R.table(MEAN, STD))
    assert torch.equal(I.ImagePrep(size=8, mean=MEAN, std=STD).table, tab)


def test_packing_of_a_batch():
    rs = np.random.RandomState(3)
    shapes = [(5, 7), (16, 16), (9, 7), (5, 16), (3, 3)]                       # (H, W): byte sizes 105, 768, 189, 240, 27
    imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    prep = I.ImagePrep(size=8)
    p = prep.pack(imgs, flips=[False, True, False, False, True])
    d = p.desc.numpy()
    assert p.desc.dtype == torch.int64 and d.shape == (5, ops.IMAGE_DESC) and p.pixels.dtype == torch.uint8
    pix = p.pixels.numpy()
    end = 0
    for i, a in enumerate(imgs):
        off, h, w, cx, cy, cw, ch, flip, ix, iy = d[i].tolist()
        assert off % 16 == 0 and off >= end and (h, w) == a.shape[:2] and (cx, cy, cw, ch) == (0, 0, w, h)
        assert flip == [0, 1, 0, 0, 1][i]
        assert np.array_equal(pix[off:off + a.size].reshape(a.shape), a)
        end = off + a.size
    assert d[0, 0] == 0 and d[:, 0].tolist() == [0, 112, 880, 1072, 1312]
    assert pix.size == 1312 + 32 + 16 and pix.size >= end + 16 and not pix[end:].any()        # the tail: padding + 16 bytes of slack
    # plans: extents {7, 5, 16, 9, 3} -> five plans for ten references, shared between axes and between images
    table = prep.plan_table().numpy()
    assert table.shape == (5, 4) and sorted(table[:, 2].tolist()) == [3, 5, 7, 9, 16] and (table[:, 3] == 8).all()
    assert d[0, 8] == d[2, 8] and d[0, 9] == d[3, 9] and d[1, 8] == d[1, 9] == d[3, 8] and d[4, 8] == d[4, 9]
    data = prep.plan_data().numpy()
    for off, ks, n, S in table.tolist():
        bounds, taps = I.build_plan(n, S)
        assert taps.shape[1] == ks
        assert np.array_equal(data[off:off + 2 * S], bounds.reshape(-1))
        assert np.array_equal(data[off + 2 * S:off + (2 + ks) * S], taps.reshape(-1))
    assert data.size == sum(S * (2 + ks) for _, ks, _, S in table.tolist())
    # a second batch re-uses the cached plans, adds its new one, and goes to the other slot of the ring
    q = prep.pack([imgs[0], rs.randint(0, 256, (4, 11, 3)).astype(np.uint8)], crops=[(3, 2, 4, 1), (11, 4, 0, 0)])
    assert prep.plan_table().shape[0] == 8 and q.slot is not p.slot                  # new extents: 2, 11, 4
    assert q.desc[0].tolist() == [0, 5, 7, 4, 1, 3, 2, 0, prep.plan(3), prep.plan(2)]
    assert np.array_equal(p.pixels.numpy()[:105].reshape(5, 7, 3), imgs[0])            # the first slot is untouched
    r = prep.pack([])
    assert r.desc.shape == (0, ops.IMAGE_DESC) and r.pixels.numel() == 16 and r.slot is p.slot


def test_every_refusal_of_image_prep():
    rgb = np.zeros((4, 5, 3), np.uint8)
    prep = I.ImagePrep(size=8)
    for bad, exc in ((np.zeros((4, 5), np.uint8), ValueError),             # grayscale
                     (np.zeros((4, 5, 4), np.uint8), ValueError),          # RGBA
                     (np.zeros((4, 5, 1), np.uint8), ValueError),
                     (np.zeros((4, 5, 3), np.float32), TypeError),
                     (np.zeros((4, 5, 3), np.uint16), TypeError)):
        with pytest.raises(exc, match=r"\.convert\('RGB'\)"):
            prep.pack([rgb, bad])
    with pytest.raises(TypeError, match="__array_interface__"):
        prep.pack([[[0, 0, 0]]])
    with pytest.raises(ValueError, match="outside the supported extents"):
        prep.pack([np.zeros((1, 8193, 3), np.uint8)])
    with pytest.raises(ValueError, match="outside the supported extents"):
        prep.pack([np.zeros((0, 4, 3), np.uint8)])
    for crop in ((6, 2, 0, 0), (2, 2, 4, 0), (2, 2, 0, 3), (0, 2, 0, 0), (2, 2, -1, 0)):
        with pytest.raises(ValueError, match="not inside"):
            prep.pack([rgb], crops=[crop])
    with pytest.raises(ValueError, match="one entry per image"):
        prep.pack([rgb], crops=[(1, 1, 0, 0)] * 2)
    with pytest.raises(ValueError, match="one entry per image"):
        prep.pack([rgb], flips=[])
    for kw in (dict(size=0), dict(size=1025), dict(mean=(0.5, 0.5)), dict(std=(1.0, 0.0, 1.0)), dict(ring=1), dict(device="cpu")):
        with pytest.raises(ValueError):
            I.ImagePrep(**kw)
    with pytest.raises(RuntimeError, match="GPU only"):                    # no CPU path: the transforms need a device
        prep.warp([rgb])
    with pytest.raises(RuntimeError, match="GPU only"):
        prep.train([rgb])
    with pytest.raises(ValueError, match="not inside"):                    # a sampled crop larger than the image (447 px -> 448)
        random.seed(0)
        I.ImagePrep(size=448, device=None).pack([np.zeros((447, 447, 3), np.uint8)], crops=[(448, 448, 0, 0)])

    class Arr:                                                            # anything with __array_interface__ is accepted
        def __init__(self, a):
            self.__array_interface__ = a.__array_interface__
            self._keep = a
    a = np.arange(60, dtype=np.uint8).reshape(4, 5, 3)
    p = prep.pack([Arr(a)])
    assert np.array_equal(p.pixels.numpy()[:60].reshape(4, 5, 3), a)


def test_train_refuses_an_uncroppable_image_before_it_draws():
    """MultiScaleCrop snaps a candidate within 3 pixels of `size` to `size`; on a short side of size - 2 or size - 1 that is larger
    than the image (the reference pads with black).  Such an image is refused whatever the draw, and nothing is drawn."""
    prep = I.ImagePrep(size=448)
    for w, h in ((447, 600), (600, 446), (446, 446)):
        with pytest.raises(ValueError, match="larger than the image"):
            prep.check_croppable(w, h)
    for w, h in ((445, 600), (448, 448), (449, 700), (510, 510), (512, 600), (1024, 768), (300, 200)):      # 510 * 0.875 = 446 -> 448 <= 510
        prep.check_croppable(w, h)
    random.seed(9)
    torch.manual_seed(9)
    state, tstate = random.getstate(), torch.get_rng_state()
    with pytest.raises(ValueError, match="image 1: 447x500"):
        prep.train([np.zeros((600, 600, 3), np.uint8), np.zeros((500, 447, 3), np.uint8)])
    assert random.getstate() == state and torch.equal(torch.get_rng_state(), tstate)
    with pytest.raises(RuntimeError, match="GPU only"):                    # explicit crops skip the rule (and then need the device)
        prep.train([np.zeros((500, 447, 3), np.uint8)], crops=[(400, 400, 0, 0)])
