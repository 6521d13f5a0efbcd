"""The progressive JPEG decoder on the GPU (jpeg_progressive_kernel of csrc/jpeg_decode.hip through ops.jpeg_decode_progressive
and ImagePrep(progressive=True).decode_jpeg / warp_jpeg / train_jpeg) against the pixels Pillow decoded for the same files
(tests/golden/jpeg_progressive.npz; baseline files from tests/golden/jpeg_decode.npz share the batches).  The arithmetic is integer:
every comparison is torch.equal, there is no tolerance.  All shapes are the fixtures' own (1x1 to 64x48, and one 1024x1024 file of
4.5 KB for an end-of-band run over 16 382 blocks).  The corrupt files fed here are the two fixed fixtures, which end in a status
word by construction: tests/test_jpeg_progressive_cpu.py runs the same decoder body on them on the CPU first."""
import numpy as np
import pytest
import torch

from mgnns_amd import images as I, ops
from tests import helpers as H
from tests import jpeg_progressive_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return H.load_golden("jpeg_progressive.npz")


@pytest.fixture(scope="module")
def base():
    return H.load_golden("jpeg_decode.npz")


@pytest.fixture(scope="module")
def prep():
    return I.ImagePrep(size=16, device=DEV, progressive=True)


@pytest.fixture(scope="module")
def prep_off():
    return I.ImagePrep(size=16, device=DEV)


SMALL = ["s0_q90", "s1_q90", "s2_q90", "s1_q100_noise", "s2_q100_noise", "s2_q30", "one_pixel", "one_block", "one_mcu", "gray", "rst_rows1",
         "rst_blocks3", "narrow_y", "w2_s1", "w3_s1", "w4_s1", "w2_s2", "w3_s2", "w4_s2"]


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
    assert sorted(SMALL + ["eob_long"]) == sorted(gold["accepted"])
    for name in SMALL:
        batch = prep.decode_jpeg(files_of(gold, [name]))
        assert batch.pixels.dtype == torch.uint8 and batch.pixels.is_cuda
        check_layout(batch, [gold["pix_" + name]])


def test_one_end_of_band_run_over_16382_blocks(gold, prep):
    batch = prep.decode_jpeg(files_of(gold, ["eob_long"]))
    assert torch.equal(batch.image(0).cpu(), torch.from_numpy(gold["pix_eob_long"]))


def test_one_mixed_batch_of_progressive_and_baseline_files_and_its_repeat(gold, base, prep, prep_off):
    names = list(base["accepted"])
    assert len(names) == 14
    files, pixels = [], []
    for k, n in enumerate(SMALL):                                         # interleaved: progressive, baseline, progressive, ...
        files.append(bytes(gold["file_" + n]))
        pixels.append(gold["pix_" + n])
        if k < len(names):
            files.append(bytes(base["file_" + names[k]]))
            pixels.append(base["pix_" + names[k]])
    assert len(files) == len(SMALL) + 14
    first = prep.decode_jpeg(files)
    check_layout(first, pixels)
    second = prep.decode_jpeg([bytearray(f) for f in files])              # lanes of one level do not race: the same buffer again
    assert torch.equal(first.pixels, second.pixels)
    # the baseline files alone: a prep with the switch off and one with it on give the same buffer
    only = [bytes(base["file_" + n]) for n in names]
    assert torch.equal(prep.decode_jpeg(only).pixels, prep_off.decode_jpeg(only).pixels)


def test_warp_and_train_equal_the_array_path(gold, base, prep):
    names = ["s0_q90", "s2_q90", "rst_rows1", "s2_q30", "gray", "s2_q100_noise"]
    files, pixels = files_of(gold, names) + [bytes(base["file_opt_q30"])], [gold["pix_" + n] for n in names] + [base["pix_opt_q30"]]
    assert torch.equal(prep.warp_jpeg(files), prep.warp(pixels))
    crops = [(20, 30, 5, 7), (37, 53, 0, 0), (9, 9, 28, 44), (64, 40, 0, 8), (10, 16, 7, 17), (8, 100, 1, 30), (30, 30, 30, 10)]
    flips = [True, False, True, True, False, True, False]
    out = prep.train_jpeg(files, crops, flips)
    assert prep.last_crops == crops and prep.last_flips == flips
    assert torch.equal(out, prep.train(pixels, crops, flips))
    assert out.shape == (7, 3, 16, 16) and bool(torch.isfinite(out).all())


def test_refusals_by_reason_and_index(gold, base, prep, prep_off):
    good = files_of(gold, ["one_block"])[0]
    for name, reason in zip(gold["refused"], gold["refused_reason"]):
        with pytest.raises(I.UnsupportedJpeg, match=r"image 1: .*\(reason %d," % int(reason)) as e:
            prep.decode_jpeg([good, bytes(gold["file_" + name]), good])
        assert e.value.refused == [(1, int(reason))], name
    with pytest.raises(I.UnsupportedJpeg) as e:                           # all of them in one exception, baseline refusals beside them
        prep.warp_jpeg([bytes(gold["file_" + n]) for n in gold["refused"]] + [good, bytes(base["file_two_scans"])])
    assert e.value.refused == [(i, int(r)) for i, r in enumerate(gold["refused_reason"])] + [(5, 10)]
    # the same prep built with the switch off: every progressive file is reason 3
    with pytest.raises(I.UnsupportedJpeg) as e:
        prep_off.decode_jpeg([good, bytes(base["file_one_block"]), bytes(gold["file_gray"])])
    assert e.value.refused == [(0, 3), (2, 3)]


def test_fallback_sees_only_the_files_still_refused(gold, base, prep):
    fb = np.arange(192, dtype=np.uint8).reshape(8, 8, 3)
    files = [bytes(gold["file_cmyk"])] + files_of(gold, ["s2_q90", "gray"]) + [bytes(gold["file_cut_before_scan7"]), bytes(base["file_s1_q90"]),
                                                                              bytes(base["file_progressive"])]
    seen = []

    def fallback(data):
        seen.append(bytes(data))
        return fb

    batch = prep.decode_jpeg(files, fallback=fallback)
    assert seen == [files[0], files[3]]                                   # the baseline fixture's progressive file is decoded now
    pixels = [fb, gold["pix_s2_q90"], gold["pix_gray"], fb, base["pix_s1_q90"], P.decode(files[5])[0]]     # (no golden pixels for that one)
    check_layout(batch, pixels)
    assert torch.equal(prep.warp_jpeg(files, fallback=fallback), prep.warp(pixels))


def test_corrupt_scans_raise_after_the_rest_decoded(gold, base, prep):
    names = ["s0_q90", "rst_blocks3", "one_pixel"]
    for bad, status, scan in zip(gold["corrupt"], gold["corrupt_status"], gold["corrupt_scan"]):
        files = files_of(gold, names[:2]) + [bytes(gold["file_" + bad]), bytes(base["file_rst_rows1"])] + files_of(gold, names[2:])
        with pytest.raises(ValueError, match=r"image 2: scan %d, segment \d+: .*\(status %d\)" % (int(scan), int(status))) as e:
            prep.decode_jpeg(files)
        err = e.value
        assert isinstance(err, ops.JpegDecodeError) and [(i, st) for i, _, st in err.failed] == [(2, int(status))]
        assert err.scans == {err.failed[0][1]: int(scan)}
        for i, pix in ((0, gold["pix_s0_q90"]), (1, gold["pix_rst_blocks3"]), (3, base["pix_rst_rows1"]), (4, gold["pix_one_pixel"])):
            assert torch.equal(err.batch.image(i).cpu(), torch.from_numpy(pix)), (bad, i)   # the others are decoded in the buffer the error carries
        assert err.pixels is err.batch.pixels
    with pytest.raises(ValueError, match="image 0: scan .*image 1: scan .*image 2: segment "):       # a baseline segment beside them
        prep.warp_jpeg([bytes(gold["file_" + n]) for n in gold["corrupt"]] + [bytes(base["file_cut"])])


def test_empty_batch(prep):
    batch = prep.decode_jpeg([])
    assert len(batch) == 0 and batch.pixels.numel() == 16 and not bool(batch.pixels.any()) and batch.sizes.shape == (0, 2)
    assert prep.warp_jpeg([]).shape == (0, 3, 16, 16)
    assert prep.train_jpeg([]).shape == (0, 3, 16, 16) and prep.last_crops == [] and prep.last_flips == []


@pytest.mark.parametrize("copies", [8, 48])
def test_many_segments_over_four_levels(gold, prep, copies):
    """the 64x48 file with a restart marker every 3 units: 88 segments a file on four levels.  48 copies are 4224 segments, 2112 of
    them on level 1: more than one lane per wave on a chip of 256 CUs"""
    data = bytes(gold["file_rst_blocks3"])
    p = I.parse_jpeg(data, progressive=True)
    assert p["nseg"] == 88 and p["levels"] == 4 and sum(s["nseg"] for s in p["scans"] if s["level"] == 1) == 44
    batch = prep.decode_jpeg([data] * copies)
    check_layout(batch, [gold["pix_rst_blocks3"]] * copies)


def test_ops_jpeg_decode_progressive_refuses_bad_records(gold):
    """ops.jpeg_decode_progressive validates the HOST records; the kernel re-checks the device copy and answers a bad record with
    status 4, writing nothing."""
    p = I.parse_jpeg(bytes(gold["file_one_block"]), progressive=True)
    data = torch.from_numpy(gold["file_one_block"].copy()).to(DEV)
    pool = torch.frombuffer(bytearray(b"".join(p["pool"])), dtype=torch.uint8).to(DEV).view(len(p["pool"]), -1)
    qsets = torch.frombuffer(bytearray(p["quant"]), dtype=torch.uint8).to(DEV).view(1, -1)
    tables = torch.zeros(0, ops.jpeg_tableset_bytes(), dtype=torch.uint8, device=DEV)
    img = torch.tensor([[2, 8, 8, 3, 2, 2, 1, 1, 0, 0, 0, 0, 0, 0, 0, 208]], dtype=torch.int64)
    seg = torch.zeros(0, ops.JPEG_SEG, dtype=torch.int64)
    rows, counts = [], [0] * p["levels"]
    for level in range(p["levels"]):
        for k, sc in enumerate(p["scans"]):
            if sc["level"] != level:
                continue
            tabs = 0
            for j, t in enumerate(sc["dc"] + [sc["ac"]]):
                tabs |= (0xFFFF if t < 0 else t) << (16 * j)
            b, e, u0, un = p["segments"][sc["seg0"]].tolist()
            rows.append([0, b, e, u0, un, sum(1 << c for c in sc["comps"]), sc["ss"], sc["se"], sc["ah"], sc["al"], tabs - (1 << 64) if tabs >= 1 << 63 else tabs, k])
            counts[level] += 1
    pseg = torch.tensor(rows, dtype=torch.int64)
    pixels = torch.full((208,), 7, dtype=torch.uint8, device=DEV)

    def run(i2=img, s2=pseg, i_dev=None, s_dev=None, check=True):
        return ops.jpeg_decode_progressive(data, i2, (i2 if i_dev is None else i_dev).to(DEV), seg, seg.to(DEV), tables, s2,
                                           (s2 if s_dev is None else s_dev).to(DEV), counts, pool, qsets, pixels, check=check)

    st = run()
    assert st.tolist() == [0] * 10 and torch.equal(pixels[:192].cpu().view(8, 8, 3), torch.from_numpy(gold["pix_one_block"]))
    assert not bool(pixels[192:].any())

    def bad(col, val, what, rec="img", row=0):
        i2, s2 = img.clone(), pseg.clone()
        (i2 if rec == "img" else s2)[row, col] = val
        with pytest.raises(ValueError, match=what):
            run(i2, s2)

    bad(0, 3, "kind must be")
    bad(4, 3, "sampling")
    bad(11, 1, "quantisation set")
    bad(12, 32, "multiples of 64")
    bad(2, int(data.numel()) + 1, "byte range", "seg")
    bad(0, 1, "image index", "seg")
    bad(4, 2, "unit range", "seg")
    bad(5, 8, "component mask", "seg")
    bad(7, 64, "Ss / Se", "seg", 1)
    bad(9, 14, "Ah / Al", "seg")
    bad(10, 0x7FFF, "outside the pool", "seg")
    bad(10, -1, "does not name", "seg")
    with pytest.raises(ValueError, match="level_counts"):
        ops.jpeg_decode_progressive(data, img, img.to(DEV), seg, seg.to(DEV), tables, pseg, pseg.to(DEV), counts[:-1], pool, qsets, pixels)
    # device records that differ from the validated host ones: status 4, the pixel buffer untouched
    pixels.fill_(7)
    wrong = img.clone()
    wrong[0, 15] = 1 << 40
    st = run(i_dev=wrong, check=False)
    assert st.tolist() == [4] * 10 and bool((pixels == 7).all())
    for col, val in ((2, 1 << 40), (3, 1), (7, 64), (9, 15), (10, 0x7FFF)):       # the last scan's record: no scan builds on it
        w = pseg.clone()
        w[9, col] = val
        st = run(s_dev=w, check=False)
        assert st.tolist() == [0] * 9 + [4], (col, st.tolist())
