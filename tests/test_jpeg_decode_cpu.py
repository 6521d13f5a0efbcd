"""The JPEG decoder without a GPU: the numpy restatement tests/jpeg_ref.py equals Pillow's recorded pixels
(tests/golden/jpeg_decode.npz, tools/gen_jpeg_goldens.py) and live Pillow bit for bit; the host parser of the library
(mgnns_jpeg_parse through images.parse_jpeg -- it makes no GPU call) agrees with the restatement's parser on every fixture; the
host side of ImagePrep's JPEG entry points refuses what it must and samples crops from header sizes as train() does from arrays."""
import io
import random

import numpy as np
import pytest
import torch

from mgnns_amd import images as I, ops
from tests import helpers as H
from tests import jpeg_ref as R


@pytest.fixture(autouse=True)
def rng_left_as_found():
    """The crop-sampling test seeds Python's and torch's generators: leave them as they were found for the tests that follow."""
    state = random.getstate(), torch.get_rng_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])


@pytest.fixture(scope="module")
def gold():
    return H.load_golden("jpeg_decode.npz")


def test_restatement_equals_every_golden(gold):
    assert len(gold["accepted"]) == 14 and str(gold["versions"][0]).startswith("Pillow")
    for name in gold["accepted"]:
        pix, status = R.decode(bytes(gold["file_" + name]))
        assert set(status) == {R.SEG_OK}, name
        assert pix.shape == gold["pix_" + name].shape and np.array_equal(pix, gold["pix_" + name]), name
    # the fixtures cover what they are meant to cover
    p = {n: R.parse(bytes(gold["file_" + n])) for n in gold["accepted"]}
    assert {(q["hs"], q["vs"]) for q in p.values() if q["ncomp"] == 3} == {(1, 1), (2, 1), (2, 2)}
    assert p["gray"]["ncomp"] == 1 and p["one_pixel"]["width"] == p["one_pixel"]["height"] == 1
    assert p["rst_blocks3"]["ri"] == 3 and len(p["rst_blocks3"]["segments"]) == 4 and len(p["rst_rows1"]["segments"]) == 7
    assert p["opt_q30"]["huff"] != p["s2_q90"]["huff"]                       # optimised tables are the file's own
    assert gold["pix_s0_q100_noise"].min() == 0 and gold["pix_s0_q100_noise"].max() == 255      # saturating samples


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(11)
    for k in range(15):
        w, h = (int(v) for v in rs.randint(1, 97, 2))
        if k % 2:
            a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        else:
            a = np.clip(np.linspace(0, 255, w)[None, :, None] + rs.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        opts = dict(quality=int(rs.randint(30, 101)), subsampling=k % 3)
        if k % 5 == 4:
            opts["restart_marker_rows"] = 1
        Image.fromarray(a).save(buf, "JPEG", **opts)
        pix, status = R.decode(buf.getvalue())
        assert set(status) == {R.SEG_OK}
        assert np.array_equal(pix, np.asarray(Image.open(buf).convert("RGB"))), (w, h, opts)


def test_parser_fields_and_reason_codes(gold):
    """The library's parser against the restatement's on every fixture: reason codes, header fields, table ids, restart layout, the
    entropy-coded range and every segment's byte range.  (The library loads without a device: the parser is host code.)"""
    assert (R.OK, R.NOT_JPEG, R.UNSUPPORTED_SOF, R.COMPONENTS, R.SAMPLING, R.SCANS, R.MISSING_TABLES) == (0, 1, 3, 6, 9, 10, 13)
    assert set(I.JPEG_REASONS) == set(range(14))
    names = [k[5:] for k in gold if k.startswith("file_")]
    assert len(names) == 22
    for name in names:
        data = bytes(gold["file_" + name])
        p, r = I.parse_jpeg(data), R.parse(data)
        assert p["reason"] == r["reason"], name
        if r["reason"] != R.OK:
            continue
        for k in ("width", "height", "ncomp", "hs", "vs", "ri", "mcux", "mcuy"):
            assert p[k] == r[k], (name, k)
        n = r["ncomp"]
        assert p["tq"][:n] == r["tq"] and p["td"][:n] == r["td"] and p["ta"][:n] == r["ta"], name
        assert p["restarts"] == r["restarts_found"] and p["ecs"] == (r["ecs_begin"], r["ecs_end"]), name
        assert p["nseg"] == len(r["segments"]) and p["segments"].tolist() == [list(s) for s in r["segments"]], name
        assert len(p["tables"]) == ops.jpeg_tableset_bytes()
        t = np.frombuffer(p["tables"], np.uint8)
        for c in range(n):
            assert np.array_equal(t[64 * r["tq"][c]:64 * r["tq"][c] + 64], r["qt"][r["tq"][c]].astype(np.uint8)), name
    for name, reason in zip(gold["refused"], gold["refused_reason"]):
        assert I.parse_jpeg(bytes(gold["file_" + name]))["reason"] == int(reason), name
    for name in gold["corrupt"]:                                         # a sound header: the parser accepts them
        assert I.parse_jpeg(bytes(gold["file_" + name]))["reason"] == 0, name
    # the restart-marked file with one marker removed: one marker short, the last segment empty
    p = I.parse_jpeg(bytes(gold["file_rst_removed"]))
    assert p["restarts"] == p["nseg"] - 2 and p["segments"][-1, 0] == p["segments"][-1, 1] == p["ecs"][1]
    # nearly every file carries the same tables: one set by content
    assert len({I.parse_jpeg(bytes(gold["file_" + n]))["tables"] for n in ("s0_q90", "s2_q90", "rst_blocks3", "rst_rows1", "one_mcu_s2")}) == 1
    assert I.parse_jpeg(bytes(gold["file_opt_q30"]))["tables"] != I.parse_jpeg(bytes(gold["file_s2_q90"]))["tables"]
    # other inputs the parser must turn into reason codes: extents, empty input, every truncation of a header
    big = I.parse_jpeg(bytes(gold["file_s0_q90"]), max_extent=36)
    assert big["reason"] == 12
    assert I.parse_jpeg(b"")["reason"] == 1 and I.parse_jpeg(bytearray(b"\xff\xd8"))["reason"] == 2
    data = bytes(gold["file_one_pixel"])
    begin = I.parse_jpeg(data)["ecs"][0]
    for n in range(2, begin):
        assert I.parse_jpeg(memoryview(data)[:n])["reason"] == R.parse(data[:n])["reason"] == 2, n


def test_corrupt_fixtures_have_their_status_in_the_restatement(gold):
    for name, status in zip(gold["corrupt"], gold["corrupt_status"]):
        _, st = R.decode(bytes(gold["file_" + name]))
        assert max(st) == int(status) and [s for s in st if s] == [int(status)], name


def test_host_side_refusals_and_crop_sampling(gold):
    prep = I.ImagePrep(size=16, device=None)
    files = [bytes(gold["file_" + n]) for n in ("s0_q90", "rst_rows1", "opt_q30", "gray")]
    pixels = [gold["pix_" + n] for n in ("s0_q90", "rst_rows1", "opt_q30", "gray")]
    # refused files: one exception that lists all of them, before any GPU work (there is no GPU here)
    bad = [files[0], bytes(gold["file_progressive"]), files[1], bytes(gold["file_cmyk"])]
    with pytest.raises(I.UnsupportedJpeg, match=r"image 1: progressive.*image 3: neither 1 nor 3") as e:
        prep.decode_jpeg(bad)
    assert e.value.refused == [(1, 3), (3, 6)] and isinstance(e.value, ValueError)
    with pytest.raises(TypeError, match="file 1: expected bytes"):
        prep.decode_jpeg([files[0], "a path"])
    with pytest.raises(RuntimeError, match="GPU only"):
        prep.decode_jpeg(files)
    # crops and flips from header sizes: the same draws in the same order as train() on the decoded arrays
    for seed in (3, 4):
        random.seed(seed)
        torch.manual_seed(seed)
        with pytest.raises(RuntimeError, match="GPU only"):
            prep.train(pixels)
        want = (prep.last_crops, prep.last_flips, random.getstate(), torch.get_rng_state())
        random.seed(seed)
        torch.manual_seed(seed)
        with pytest.raises(RuntimeError, match="GPU only"):
            prep.train_jpeg(files)
        assert (prep.last_crops, prep.last_flips) == want[:2] and random.getstate() == want[2] and torch.equal(torch.get_rng_state(), want[3])
    # check_croppable comes first, from the header size, and nothing is drawn
    prep = I.ImagePrep(size=38, device=None)                               # 37 x 53: a short side of size - 1
    random.seed(1)
    state = random.getstate()
    with pytest.raises(ValueError, match="image 1: 37x53"):
        prep.train_jpeg([files[2], files[0]])
    assert random.getstate() == state
    # a fallback's pixels give the sizes of refused files
    prep = I.ImagePrep(size=16, device=None)
    with pytest.raises(RuntimeError, match="GPU only"):
        prep.train_jpeg([bytes(gold["file_progressive"])], crops=[(8, 8, 1, 2)], flips=[True], fallback=lambda b: np.zeros((16, 16, 3), np.uint8))
    assert prep.last_crops == [(8, 8, 1, 2)] and prep.last_flips == [True]
