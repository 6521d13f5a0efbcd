"""Other component layouts on the GPU (the layout kernels of csrc/jpeg_decode.hip through ops.jpeg_decode_layouts and
ImagePrep(layouts=True)): CMYK, YCCK, RGB, 4:4:0, 4:1:1, odd mixtures of sampling factors, SOF1 and gray labelled 2x2 decode to
exactly the pixels Pillow gives (tests/golden/jpeg_layouts.npz), alone and mixed with baseline, progressive and fall-back images;
the baseline files keep their route, their pixels and their status words.  The arithmetic is integer: every comparison is
torch.equal.  The corrupt files fed here are the two fixed fixtures, which tools/dev/jpeg_layouts_host_check.py proves harmless on
the CPU along with every truncation and 10 000 mutations of every file."""
import random

import numpy as np
import pytest
import torch

from mgnns_amd import images as I, ops
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def rng_left_as_found():
    """Leave every generator exactly as it was found (tests/test_jpeg_decode_gpu.py says why)."""
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2], DEV)


@pytest.fixture(scope="module")
def gold():
    return H.load_golden("jpeg_layouts.npz")


@pytest.fixture(scope="module")
def base():
    return H.load_golden("jpeg_decode.npz")


@pytest.fixture(scope="module")
def prep():
    return I.ImagePrep(size=16, device=DEV, layouts=True)


@pytest.fixture(scope="module")
def prep_off():
    return I.ImagePrep(size=16, device=DEV)


def files_of(g, names):
    return [bytes(g["file_" + n]) for n in names]


def check_layout(batch, pixels):
    """every image equals its pixels; every byte between the images and the 16 bytes of slack are zero"""
    buf = batch.pixels.cpu().numpy()
    covered = np.zeros(buf.size, bool)
    assert len(batch) == len(pixels) and batch.sizes.tolist() == [list(p.shape[:2]) for p in pixels]
    for i, p in enumerate(pixels):
        o = int(batch.offsets[i])
        assert o % 16 == 0 and torch.equal(batch.image(i).cpu(), torch.from_numpy(p)), i
        covered[o:o + p.size] = True
    last = int(batch.offsets[-1]) + pixels[-1].size if pixels else 0
    assert buf.size == (last + 15) // 16 * 16 + 16
    assert not buf[~covered].any()


def test_every_fixture_decodes_to_pillows_pixels_alone(gold, prep):
    assert len(gold["accepted"]) == 29
    for name in gold["accepted"]:
        batch = prep.decode_jpeg(files_of(gold, [name]))
        assert batch.pixels.dtype == torch.uint8 and batch.pixels.is_cuda
        check_layout(batch, [gold["pix_" + name]])


def test_one_mixed_batch_with_every_other_kind_of_image_and_it_repeats(gold, base):
    prog = H.load_golden("jpeg_progressive.npz")
    prep = I.ImagePrep(size=16, device=DEV, progressive=True, layouts=True)
    assert len(base["accepted"]) == 14
    staged = np.random.RandomState(5).randint(0, 256, (9, 13, 3)).astype(np.uint8)
    refused = bytes(gold["file_two_scans"])
    files, pixels = [], []
    lay, bas, pro = list(gold["accepted"]), list(base["accepted"]), list(prog["accepted"])
    for k in range(max(len(lay), len(bas), len(pro))):                   # interleaved: no kind of image lies in one stretch of the buffers
        for g, names in ((gold, lay), (base, bas), (prog, pro)):
            if k < len(names):
                files.append(bytes(g["file_" + names[k]]))
                pixels.append(g["pix_" + names[k]])
        if k == 3:
            files.append(refused)
            pixels.append(staged)
    seen = []
    fallback = lambda f: seen.append(f) or staged
    first = prep.decode_jpeg(files, fallback=fallback)
    assert seen == [refused] and len(first) == 29 + 14 + len(pro) + 1
    check_layout(first, pixels)
    keep = first.pixels.clone()
    second = prep.decode_jpeg(files, fallback=fallback)
    assert torch.equal(second.pixels, keep) and torch.equal(first.pixels, keep)
    assert torch.equal(prep.warp_jpeg(files, fallback=fallback), prep.warp(pixels))          # one decode sequence, one image_prep launch


def test_baseline_files_keep_their_pixels_and_status_words(base, prep, prep_off):
    names = list(base["accepted"]) + list(base["corrupt"])
    files = files_of(base, names)
    on_args, on = prep._jpeg_run(prep._jpeg_headers(files, None), staged_only=True)
    off_args, off = prep_off._jpeg_run(prep_off._jpeg_headers(files, None), staged_only=True)
    assert len(on_args) == 14 and len(off_args) == 7 and on_args[11].shape == (0, ops.JPEG_SEG)          # no image of kind 3
    assert torch.equal(on_args[1], off_args[1]) and torch.equal(on_args[3], off_args[3])                 # the same records
    on.pixels.fill_(3), off.pixels.fill_(3)
    st_on = ops.jpeg_decode_layouts(*on_args, check=False)
    st_off = ops.jpeg_decode(*off_args, check=False)
    assert torch.equal(st_on, st_off) and sorted(set(st_on.tolist())) == [0, 1, 2]
    assert torch.equal(on.pixels, off.pixels)                              # the whole buffer: what a failed scan left behind as well
    ok = list(base["accepted"])
    a, b = prep.decode_jpeg(files_of(base, ok)), prep_off.decode_jpeg(files_of(base, ok))
    assert torch.equal(a.pixels, b.pixels) and torch.equal(a.offsets, b.offsets) and torch.equal(a.sizes, b.sizes)
    check_layout(a, [base["pix_" + n] for n in ok])


def test_warp_and_train_equal_the_array_path(gold, base, prep):
    names = ["s440_21x45", "cmyk_s2", "s411_61x13", "rgb_ids", "ycck_s0", "y2x1_cb1x2_cr2x1"]
    files = files_of(gold, names) + files_of(base, ["s2_q90"])
    pixels = [gold["pix_" + n] for n in names] + [base["pix_s2_q90"]]
    assert torch.equal(prep.warp_jpeg(files), prep.warp(pixels))
    crops = [(10, 30, 5, 7), (37, 29, 0, 0), (9, 9, 28, 4), (20, 13, 3, 5), (10, 16, 7, 1), (20, 20, 9, 7), (30, 20, 1, 2)]
    flips = [True, False, True, True, False, True, False]
    out = prep.train_jpeg(files, crops, flips)
    assert prep.last_crops == crops and prep.last_flips == flips
    assert torch.equal(out, prep.train(pixels, crops, flips))
    assert out.shape == (7, 3, 16, 16) and bool(torch.isfinite(out).all())


def test_layouts_compose_with_split_scans(gold, base):
    split = H.load_golden("jpeg_split.npz")
    prep = I.ImagePrep(size=16, device=DEV, split=8, layouts=True)
    names = ["cmyk_s0", "s440_rst", "s1x4_16x64", "gray_2x2", "sof1_s2"]
    files = files_of(gold, names[:2]) + [bytes(split["file_photo_s2_opt"])] + files_of(gold, names[2:]) + files_of(base, ["rst_rows1", "s0_q90"])
    pixels = [gold["pix_" + n] for n in names[:2]] + [split["pix_photo_s2_opt"]] + [gold["pix_" + n] for n in names[2:]] + \
        [base["pix_rst_rows1"], base["pix_s0_q90"]]
    check_layout(prep.decode_jpeg(files), pixels)
    assert torch.equal(prep.warp_jpeg(files), prep.warp(pixels))


def test_refusals_without_a_fallback(gold, prep):
    files = files_of(gold, ["cmyk_s0"]) + files_of(gold, gold["refused"]) + files_of(gold, ["s440_w1"])
    with pytest.raises(I.UnsupportedJpeg) as e:
        prep.decode_jpeg(files)
    assert e.value.refused == [(1 + i, int(r)) for i, r in enumerate(gold["refused_reason"])]
    assert sorted({r for _, r in e.value.refused}) == [3, 6, 10, 17, 18]


def test_corrupt_scans_name_their_image_and_the_rest_is_decoded(gold, base, prep):
    assert list(gold["corrupt"]) == ["s440_truncated", "cmyk_bad_code"] and gold["corrupt_status"].tolist() == [1, 2]
    names = ["cmyk_s2", "s440_21x45", "rgb_adobe"]
    files = files_of(gold, names[:1]) + files_of(gold, ["s440_truncated"]) + files_of(base, ["s1_q90"]) + files_of(gold, names[1:2]) + \
        files_of(gold, ["cmyk_bad_code"]) + files_of(gold, names[2:])
    with pytest.raises(ops.JpegDecodeError) as e:
        prep.decode_jpeg(files)
    err = e.value
    assert [(i, st) for i, _, st in err.failed] == [(1, 1), (4, 2)]
    assert "image 1: segment" in str(err) and "image 4: segment" in str(err) and "ran out of data" in str(err) and "invalid Huffman code" in str(err)
    assert err.pixels is err.batch.pixels
    for i, (g, n) in ((0, (gold, names[0])), (2, (base, "s1_q90")), (3, (gold, names[1])), (5, (gold, names[2]))):
        assert torch.equal(err.batch.image(i).cpu(), torch.from_numpy(g["pix_" + n])), n


def test_empty_batch(prep):
    batch = prep.decode_jpeg([])
    assert len(batch) == 0 and batch.pixels.numel() == 16 and not bool(batch.pixels.any()) and batch.sizes.shape == (0, 2)
    assert prep.warp_jpeg([]).shape == (0, 3, 16, 16)
    assert prep.train_jpeg([]).shape == (0, 3, 16, 16) and prep.last_crops == [] and prep.last_flips == []


def test_a_few_hundred_segments(gold, prep):
    """130 copies of the file with a restart marker per MCU row: 390 lanes, more than one wave's worth in a workgroup"""
    data = bytes(gold["file_s440_rst"])
    assert I.parse_jpeg(data, layouts=True)["nseg"] == 3
    batch = prep.decode_jpeg([data] * 130)
    check_layout(batch, [gold["pix_s440_rst"]] * 130)


def test_a_device_record_that_differs_from_the_hosts_is_status_4_and_writes_nothing(gold):
    name = "cmyk_s2"
    p = I.parse_jpeg(bytes(gold["file_" + name]), layouts=True)
    W, Hh = p["width"], p["height"]
    data = torch.from_numpy(gold["file_" + name].copy()).to(DEV)
    tables = torch.frombuffer(bytearray(p["tables"]), dtype=torch.uint8).to(DEV).view(1, -1)
    pack = lambda v, bits: sum(int(x) << (bits * c) for c, x in enumerate(v))
    npix = W * Hh * 3
    end = (npix + 15) // 16 * 16 + 16
    img = torch.tensor([[3, W, Hh, p["ncomp"] | p["colour"] << 8, pack(p["h"], 4), pack(p["v"], 4), p["mcux"], p["mcuy"], pack(p["tq"], 8),
                         pack(p["td"], 8), pack(p["ta"], 8), 0, 0, 0, 0, end]], dtype=torch.int64)
    b, e = (int(v) for v in p["segments"][0])
    lseg = torch.tensor([[0, b, e, 0, p["mcux"] * p["mcuy"]]], dtype=torch.int64)
    seg = torch.zeros(0, ops.JPEG_SEG, dtype=torch.int64)
    pseg = torch.zeros(0, ops.JPEG_PSEG, dtype=torch.int64)
    pool = torch.zeros(0, ops.jpeg_huff_bytes(), dtype=torch.uint8, device=DEV)
    qsets = torch.zeros(0, ops.JPEG_QSET, dtype=torch.uint8, device=DEV)
    pixels = torch.full((end,), 7, dtype=torch.uint8, device=DEV)

    def run(i_dev=img, l_dev=lseg, **kw):
        return ops.jpeg_decode_layouts(data, img, i_dev.to(DEV), seg, seg.to(DEV), tables, pseg, pseg.to(DEV), [], pool, qsets, lseg, l_dev.to(DEV),
                                       pixels, check=False, **kw)

    st = run()
    assert st.dtype == torch.int32 and st.is_cuda and st.tolist() == [0]
    assert torch.equal(pixels[:npix].cpu().view(Hh, W, 3), torch.from_numpy(gold["pix_" + name])) and not bool(pixels[npix:].any())
    # the host refuses what the kernels would refuse
    wrong = img.clone()
    wrong[0, 4] = 0x1115                                                     # a sampling factor of 5
    with pytest.raises(ValueError, match="sampling factors outside 1..4"):
        ops.jpeg_decode_layouts(data, wrong, wrong.to(DEV), seg, seg.to(DEV), tables, pseg, pseg.to(DEV), [], pool, qsets, lseg, lseg.to(DEV), pixels)
    # an image record the device refuses stops the IDCT and colour stages too; a segment record it refuses, the lane
    cases = ((0, 1, "img"), (3, 3 | 3 << 8, "img"), (4, 0x1113, "img"), (5, 0x1115, "img"), (6, p["mcux"] + 1, "img"), (11, 1, "img"),
             (12, 32, "img"), (15, 1 << 40, "img"), (4, 1 << 20, "seg"), (0, 1, "seg"), (2, 1 << 40, "seg"), (3, 1, "seg"))
    for col, val, rec in cases:
        pixels.fill_(7)
        wrong = (img if rec == "img" else lseg).clone()
        wrong[0, col] = val
        st = run(i_dev=wrong) if rec == "img" else run(l_dev=wrong, stages=1)
        assert st.tolist() == [4] and bool((pixels == 7).all()), (col, val, rec)
