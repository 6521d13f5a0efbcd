"""The JPEG decoder on the GPU (csrc/jpeg_decode.hip through ops.jpeg_decode and ImagePrep.decode_jpeg / warp_jpeg / train_jpeg)
against the pixels Pillow decoded for the same files (tests/golden/jpeg_decode.npz).  The arithmetic is integer: every comparison
is torch.equal, there is no tolerance.  All shapes are the fixtures' own (1x1 to 64x48; 4:4:4, 4:2:2, 4:2:0 and grayscale; the
library's and a file's own Huffman tables; restart intervals by blocks and by rows).  The corrupt files fed here are the three
fixed fixtures, which tools/dev/jpeg_host_check.py proves harmless on the CPU along with 10 000 mutations of every file."""
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
    """These tests seed Python's and torch's generators (crop and flip sampling).  Tests that run after them draw dropout seeds from
    torch's global generator without seeding it: leave every generator exactly as it was found."""
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2], DEV)


@pytest.fixture(scope="module")
def gold():
    return H.load_golden("jpeg_decode.npz")


@pytest.fixture(scope="module")
def prep():
    return I.ImagePrep(size=16, device=DEV)


def files_of(gold, names):
    return [bytes(gold["file_" + n]) for n in names]


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


def test_every_golden_decodes_to_pillows_pixels_alone(gold, prep):
    for name in gold["accepted"]:
        batch = prep.decode_jpeg(files_of(gold, [name]))
        assert batch.pixels.dtype == torch.uint8 and batch.pixels.is_cuda
        got, want = batch.image(0).cpu().numpy(), gold["pix_" + name]
        assert got.shape == want.shape and int(np.abs(got.astype(int) - want.astype(int)).max()) == 0, name
        check_layout(batch, [want])


def test_one_mixed_batch_equals_the_single_decodes_and_repeats(gold, prep):
    names = list(gold["accepted"])
    pixels = [gold["pix_" + n] for n in names]
    first = prep.decode_jpeg(files_of(gold, names))
    check_layout(first, pixels)                                         # (the single decodes equal the same goldens: the test above)
    second = prep.decode_jpeg([bytearray(f) for f in files_of(gold, names)])
    third = prep.decode_jpeg([memoryview(f) for f in files_of(gold, names)])
    assert torch.equal(first.pixels, second.pixels) and torch.equal(first.pixels, third.pixels)
    pix, sizes, offsets = first                                          # unpacks as the three things the caller needs
    assert pix is first.pixels and sizes.shape == (len(names), 2) and offsets.shape == (len(names),)


def test_warp_and_train_equal_the_array_path(gold, prep):
    names = ["s0_q90", "s2_q90", "rst_rows1", "opt_q30", "gray", "s1_q100_noise"]
    files, pixels = files_of(gold, names), [gold["pix_" + n] for n in names]
    assert torch.equal(prep.warp_jpeg(files), prep.warp(pixels))
    crops = [(20, 30, 5, 7), (37, 53, 0, 0), (9, 9, 28, 44), (64, 40, 0, 8), (10, 16, 7, 17), (8, 100, 1, 30)]
    flips = [True, False, True, True, False, True]
    out = prep.train_jpeg(files, crops, flips)
    assert prep.last_crops == crops and prep.last_flips == flips
    assert torch.equal(out, prep.train(pixels, crops, flips))
    assert out.shape == (6, 3, 16, 16) and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError, match="image 2: crop .* is not inside the 37x53 image"):
        prep.train_jpeg(files, [crops[0], crops[1], (30, 30, 10, 30)] + crops[3:], flips)


def test_sampled_crops_are_trains(gold, prep):
    names = ["s0_q90", "rst_blocks3", "s1_q90", "opt_q30"]
    files, pixels = files_of(gold, names), [gold["pix_" + n] for n in names]
    random.seed(21)
    torch.manual_seed(21)
    want = prep.train(pixels)
    crops, flips = prep.last_crops, prep.last_flips
    random.seed(21)
    torch.manual_seed(21)
    got = prep.train_jpeg(files)
    assert prep.last_crops == crops and prep.last_flips == flips and torch.equal(got, want)


def test_every_refusal_raises_with_reason_and_index(gold, prep):
    good = files_of(gold, ["one_block"])[0]
    for name, reason in zip(gold["refused"], gold["refused_reason"]):
        with pytest.raises(I.UnsupportedJpeg, match=r"image 1: .*\(reason %d," % int(reason)) as e:
            prep.decode_jpeg([good, bytes(gold["file_" + name]), good])
        assert e.value.refused == [(1, int(reason))], name
    with pytest.raises(I.UnsupportedJpeg) as e:                           # all of them in one exception
        prep.warp_jpeg([bytes(gold["file_" + n]) for n in gold["refused"]] + [good])
    assert e.value.refused == [(i, int(r)) for i, r in enumerate(gold["refused_reason"])]


def test_fallback_images_share_the_batch(gold, prep):
    names = ["s2_q90", "gray", "rst_rows2"]
    fb_pixels = {bytes(gold["file_progressive"]): np.full((16, 16, 3), 200, np.uint8), bytes(gold["file_cmyk"]): np.arange(192, dtype=np.uint8).reshape(8, 8, 3)}
    files = [bytes(gold["file_progressive"])] + files_of(gold, names[:2]) + [bytes(gold["file_cmyk"])] + files_of(gold, names[2:]) + [bytes(gold["file_cmyk"])]
    pixels = [fb_pixels[files[0]], gold["pix_s2_q90"], gold["pix_gray"], fb_pixels[files[3]], gold["pix_rst_rows2"], fb_pixels[files[3]]]
    seen = []

    def fallback(data):
        seen.append(bytes(data))
        return fb_pixels[bytes(data)]

    batch = prep.decode_jpeg(files, fallback=fallback)
    assert seen == [files[0], files[3], files[5]]                         # only the refused files, as their bytes
    check_layout(batch, pixels)                                           # (a fall-back image is last: its padding and the slack too)
    assert torch.equal(prep.warp_jpeg(files, fallback=fallback), prep.warp(pixels))
    only = prep.decode_jpeg([files[0]], fallback=fallback)                # a batch with nothing to decode
    check_layout(only, [pixels[0]])


def test_corrupt_scans_raise_after_the_rest_decoded(gold, prep):
    names = ["s0_q90", "rst_blocks3", "one_pixel"]
    nseg = {n: I.parse_jpeg(bytes(gold["file_" + n]))["nseg"] for n in list(names) + list(gold["corrupt"])}
    for bad, status in zip(gold["corrupt"], gold["corrupt_status"]):
        files = files_of(gold, names[:2]) + [bytes(gold["file_" + bad])] + files_of(gold, names[2:])
        with pytest.raises(ValueError, match=r"image 2: segment \d+: .*\(status %d\)" % int(status)) as e:
            prep.decode_jpeg(files)
        err = e.value
        assert isinstance(err, ops.JpegDecodeError) and {i for i, _, _ in err.failed} == {2}
        assert [st for _, _, st in err.failed] == [int(status)]
        if bad == "rst_removed":                                          # its last segment has no data left
            assert err.failed[0][1] == nseg["s0_q90"] + nseg["rst_blocks3"] + nseg[bad] - 1
        for i, n in ((0, names[0]), (1, names[1]), (3, names[2])):       # the others are decoded in the buffer the error carries
            assert torch.equal(err.batch.image(i).cpu(), torch.from_numpy(gold["pix_" + n])), (bad, n)
        assert err.pixels is err.batch.pixels
    with pytest.raises(ValueError, match="image 0: .*image 1: .*image 2: "):      # all three at once: every image is named
        prep.warp_jpeg([bytes(gold["file_" + n]) for n in gold["corrupt"]])


def test_empty_batch(prep):
    batch = prep.decode_jpeg([])
    assert len(batch) == 0 and batch.pixels.numel() == 16 and not bool(batch.pixels.any()) and batch.sizes.shape == (0, 2)
    assert prep.warp_jpeg([]).shape == (0, 3, 16, 16)
    assert prep.train_jpeg([]).shape == (0, 3, 16, 16) and prep.last_crops == [] and prep.last_flips == []


def test_segments_span_more_than_one_wave(gold, prep):
    """65 copies of a file with 7 restart segments: 455 lanes"""
    data = bytes(gold["file_rst_rows1"])
    batch = prep.decode_jpeg([data] * 65)
    want = torch.from_numpy(gold["pix_rst_rows1"])
    got = batch.pixels.cpu()
    for i in range(65):
        o = int(batch.offsets[i])
        assert torch.equal(got[o:o + want.numel()].view(want.shape), want), i
    check_layout(batch, [gold["pix_rst_rows1"]] * 65)


def test_ops_jpeg_decode_refuses_bad_records(gold):
    """ops.jpeg_decode validates the HOST records; the kernels re-check the device copy and answer a bad record with status 4,
    writing nothing (a record buffer can change under a captured graph)."""
    p = I.parse_jpeg(bytes(gold["file_one_block"]))
    data = torch.from_numpy(gold["file_one_block"].copy()).to(DEV)
    tables = torch.frombuffer(bytearray(p["tables"]), dtype=torch.uint8).to(DEV).view(1, -1)
    img = torch.tensor([[1, 8, 8, 3, 1, 1, 1, 1, 0x010100, 0x010100, 0x010100, 0, 0, 0, 0, 208]], dtype=torch.int64)
    seg = torch.tensor([[0, p["ecs"][0], p["ecs"][1], 0, 1]], dtype=torch.int64)
    pixels = torch.full((208,), 7, dtype=torch.uint8, device=DEV)
    st = ops.jpeg_decode(data, img, img.to(DEV), seg, seg.to(DEV), tables, pixels)
    assert st.tolist() == [0] and torch.equal(pixels[:192].cpu().view(8, 8, 3), torch.from_numpy(gold["pix_one_block"]))
    assert not bool(pixels[192:].any())

    def bad(col, val, what, rec="img"):
        i2, s2 = img.clone(), seg.clone()
        (i2 if rec == "img" else s2)[0, col] = val
        with pytest.raises(ValueError, match=what):
            ops.jpeg_decode(data, i2, i2.to(DEV), s2, s2.to(DEV), tables, pixels)

    bad(1, 9000, "extent")
    bad(4, 3, "sampling")
    bad(6, 2, "MCU counts")
    bad(11, 1, "table set")
    bad(12, 32, "multiples of 64")
    bad(14, 8, "multiple of 16")
    bad(15, 4096, "do not fit")
    bad(2, int(data.numel()) + 1, "byte range", "seg")
    bad(4, 2, "MCU range", "seg")
    bad(0, 1, "image index", "seg")
    # device records that differ from the validated host ones: status 4, the pixel buffer untouched
    pixels.fill_(7)
    wrong = img.clone()
    wrong[0, 15] = 1 << 40
    st = ops.jpeg_decode(data, img, wrong.to(DEV), seg, seg.to(DEV), tables, pixels, check=False)
    assert st.tolist() == [4] and bool((pixels == 7).all())
    wrong_seg = seg.clone()
    wrong_seg[0, 2] = 1 << 40
    with pytest.raises(ops.JpegDecodeError, match=r"status 4"):
        ops.jpeg_decode(data, img, img.to(DEV), seg, wrong_seg.to(DEV), tables, pixels)
