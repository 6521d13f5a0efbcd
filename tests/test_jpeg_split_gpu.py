"""Split scans on the GPU (jpeg_split_kernel of csrc/jpeg_decode.hip through ops.jpeg_decode_split and ImagePrep(split=...)): a long
baseline scan decoded by a workgroup, a lane per chunk, gives exactly the pixels of the one-lane decode, which are Pillow's
(tests/golden/jpeg_decode.npz, tests/golden/jpeg_split.npz, tests/golden/jpeg_progressive.npz).  The arithmetic is integer: every
comparison is torch.equal.  The corrupt files fed here are the three fixed fixtures, which tools/dev/jpeg_split_host_check.py proves
harmless and equal to the serial decoder on the CPU along with 10 000 mutations of every file."""
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
    """both baseline goldens under one roof: the split file's names carry the prefix split_"""
    g = dict(H.load_golden("jpeg_decode.npz"))
    s = H.load_golden("jpeg_split.npz")
    for n in s["accepted"]:
        g["file_split_" + n], g["pix_split_" + n] = s["file_" + n], s["pix_" + n]
    g["accepted"] = list(g["accepted"]) + ["split_" + n for n in s["accepted"]]
    return g


@pytest.fixture(scope="module")
def prep_off():
    return I.ImagePrep(size=16, device=DEV)


@pytest.fixture(scope="module")
def prep8():
    return I.ImagePrep(size=16, device=DEV, split=8)


@pytest.fixture(scope="module")
def prep64():
    return I.ImagePrep(size=16, device=DEV, split=64)


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


def test_every_golden_decodes_to_pillows_pixels_alone(gold, prep8, prep64):
    assert len(gold["accepted"]) == 18
    for name in gold["accepted"]:
        for prep in (prep8, prep64):
            batch = prep.decode_jpeg(files_of(gold, [name]))
            assert batch.pixels.dtype == torch.uint8 and batch.pixels.is_cuda
            check_layout(batch, [gold["pix_" + name]])


def test_one_mixed_batch_equals_the_switch_off_decode_and_repeats(gold, prep8, prep_off):
    names = list(gold["accepted"])                                       # the rst_* files among them: short segments, the one-lane route
    assert {"rst_blocks3", "rst_rows1", "rst_rows2", "one_pixel"} <= set(names)
    first = prep8.decode_jpeg(files_of(gold, names))
    check_layout(first, [gold["pix_" + n] for n in names])
    off = prep_off.decode_jpeg(files_of(gold, names))
    second = prep8.decode_jpeg(files_of(gold, names))
    assert torch.equal(first.pixels, off.pixels) and torch.equal(first.pixels, second.pixels)
    assert torch.equal(first.offsets, off.offsets) and torch.equal(first.sizes, off.sizes)


def test_corrupt_scans_fail_as_they_do_with_the_switch_off(gold, prep8, prep_off):
    names = ["s0_q90", "rst_blocks3", "split_photo_s2_opt", "one_pixel"]
    files = files_of(gold, names[:1]) + [bytes(gold["file_" + gold["corrupt"][0]])] + files_of(gold, names[1:3]) + \
        [bytes(gold["file_" + n]) for n in gold["corrupt"][1:]] + files_of(gold, names[3:])
    errs = []
    for prep in (prep8, prep_off):
        with pytest.raises(ops.JpegDecodeError) as e:
            prep.decode_jpeg(files)
        errs.append(e.value)
    on, off = errs
    assert on.failed == off.failed and [st for _, _, st in on.failed] == [int(s) for s in gold["corrupt_status"]] == [1, 1, 2]
    assert {i for i, _, _ in on.failed} == {1, 4, 5}
    assert torch.equal(on.pixels, off.pixels)                            # the whole buffer: what a failed scan left behind as well
    for i, n in ((0, names[0]), (2, names[1]), (3, names[2]), (6, names[3])):
        assert torch.equal(on.batch.image(i).cpu(), torch.from_numpy(gold["pix_" + n])), n


def test_warp_and_train_equal_the_array_path(gold, prep64):
    names = ["s0_q90", "split_photo_s2_opt", "rst_rows1", "split_noise_s0_q100", "split_gray", "split_photo_s1_opt"]
    files, pixels = files_of(gold, names), [gold["pix_" + n] for n in names]
    assert torch.equal(prep64.warp_jpeg(files), prep64.warp(pixels))
    crops = [(20, 30, 5, 7), (128, 96, 0, 0), (9, 9, 28, 44), (40, 33, 11, 31), (10, 16, 7, 17), (100, 40, 20, 50)]
    flips = [True, False, True, True, False, True]
    out = prep64.train_jpeg(files, crops, flips)
    assert prep64.last_crops == crops and prep64.last_flips == flips
    assert torch.equal(out, prep64.train(pixels, crops, flips))
    assert out.shape == (6, 3, 16, 16) and bool(torch.isfinite(out).all())


def test_split_composes_with_progressive(gold):
    prog = H.load_golden("jpeg_progressive.npz")
    prep = I.ImagePrep(size=16, device=DEV, progressive=True, split=8)
    pnames = ["s2_q90", "gray", "rst_rows1", "s0_q90"]
    bnames = ["split_photo_s2_opt", "s1_q90", "rst_blocks3", "split_gray"]
    files = [bytes(prog["file_" + pnames[0]])] + files_of(gold, bnames[:2]) + [bytes(prog["file_" + n]) for n in pnames[1:3]] + \
        files_of(gold, bnames[2:]) + [bytes(prog["file_" + pnames[3]])]
    pixels = [prog["pix_" + pnames[0]]] + [gold["pix_" + n] for n in bnames[:2]] + [prog["pix_" + n] for n in pnames[1:3]] + \
        [gold["pix_" + n] for n in bnames[2:]] + [prog["pix_" + pnames[3]]]
    check_layout(prep.decode_jpeg(files), pixels)
    assert torch.equal(prep.warp_jpeg(files), prep.warp(pixels))


def test_ops_jpeg_decode_split_status_and_bad_device_records(gold):
    """check=False returns the status tensor; the kernel re-checks the device records and answers a bad one with status 4, writing
    nothing -- the split kernel for the segment it takes as the one-lane kernel for its own."""
    name = "split_photo_s1_opt"
    p = I.parse_jpeg(bytes(gold["file_" + name]))
    W, Hh = p["width"], p["height"]
    data = torch.from_numpy(gold["file_" + name].copy()).to(DEV)
    tables = torch.frombuffer(bytearray(p["tables"]), dtype=torch.uint8).to(DEV).view(1, -1)
    pack3 = lambda v: int(v[0]) | int(v[1]) << 8 | int(v[2]) << 16
    npix = W * Hh * 3
    end = (npix + 15) // 16 * 16 + 16
    img = torch.tensor([[1, W, Hh, p["ncomp"], p["hs"], p["vs"], p["mcux"], p["mcuy"], pack3(p["tq"]), pack3(p["td"]), pack3(p["ta"]), 0, 0, 0, 0, end]],
                       dtype=torch.int64)
    b, e = (int(v) for v in p["segments"][0])
    seg = torch.tensor([[0, b, e, 0, p["mcux"] * p["mcuy"]]], dtype=torch.int64)
    assert e - b >= 2 * 64                                                # the split kernel's at chunk 64
    pseg = torch.zeros(0, ops.JPEG_PSEG, dtype=torch.int64)
    pool = torch.zeros(0, ops.jpeg_huff_bytes(), dtype=torch.uint8, device=DEV)
    qsets = torch.zeros(0, ops.JPEG_QSET, dtype=torch.uint8, device=DEV)
    pixels = torch.full((end,), 7, dtype=torch.uint8, device=DEV)

    def run(i_dev=img, s_dev=seg, chunk=64, **kw):
        return ops.jpeg_decode_split(data, img, i_dev.to(DEV), seg, s_dev.to(DEV), tables, pseg, pseg.to(DEV), [], pool, qsets, pixels,
                                     chunk_bytes=chunk, check=False, **kw)

    st = run()
    assert st.dtype == torch.int32 and st.is_cuda and st.tolist() == [0]
    assert torch.equal(pixels[:npix].cpu().view(Hh, W, 3), torch.from_numpy(gold["pix_" + name])) and not bool(pixels[npix:].any())
    with pytest.raises(ValueError, match="chunk_bytes must be"):
        run(chunk=12)
    # (a segment record with a range outside the buffer is the one-lane kernel's to refuse; an image record that is refused stops the
    # IDCT and colour stages too)
    for col, val, rec in ((15, 1 << 40, "img"), (12, 32, "img"), (4, 1 << 20, "seg"), (0, 1, "seg"), (2, 1 << 40, "seg")):
        pixels.fill_(7)
        wrong = (img if rec == "img" else seg).clone()
        wrong[0, col] = val
        st = run(i_dev=wrong) if rec == "img" else run(s_dev=wrong, stages=1)
        assert st.tolist() == [4] and bool((pixels == 7).all()), (col, rec)


def test_more_workgroups_than_xcds_and_more_chunks_than_lanes(gold, prep8):
    """65 copies of the noise file: its scan is above 8 KB, so 8-byte chunks outnumber the lanes and the chunk grows"""
    name = "split_noise_s0_q100"
    p = I.parse_jpeg(bytes(gold["file_" + name]))
    assert int(p["segments"][0][1] - p["segments"][0][0]) > 8192
    batch = prep8.decode_jpeg([bytes(gold["file_" + name])] * 65)
    want = torch.from_numpy(gold["pix_" + name])
    got = batch.pixels.cpu()
    for i in range(65):
        o = int(batch.offsets[i])
        assert torch.equal(got[o:o + want.numel()].view(want.shape), want), i
    check_layout(batch, [gold["pix_" + name]] * 65)
