"""The image transforms on the GPU (csrc/image_prep.hip through ops.image_prep and mgnns_amd.images.ImagePrep) against the numpy
restatement tests/image_prep_ref.py, which test_image_prep_cpu.py ties to the reference's recorded outputs and to live Pillow.
The arithmetic is integer and the table look-up exact, so every comparison is torch.equal: there is no tolerance.

Shapes are the smallest at which the kernel takes each of its paths: a tile is 16 rows x 64 columns of output; horizontal plans of
up to 16 taps per output are staged in LDS (a reduction of up to 7x), longer ones are read from global memory; a source row
segment longer than 1344 pixels goes through LDS in several chunks; rows are stored 16 bytes per lane when S_w % 4 == 0."""
import numpy as np
import pytest
import torch

from mgnns_amd import harness, images as I, ops, synth, trunk
from tests import helpers as H
from tests import image_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TAB = R.table(MEAN, STD)


def rnd(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def stage(imgs, S_h, S_w, crops=None, flips=None):
    """Pack a batch for ops.image_prep by hand (any S_h x S_w; ImagePrep itself is square): host tensors + the lut."""
    plans, rows, chunks, desc, parts, off = {}, [], [], [], [], 0

    def plan(n, S):
        if (n, S) not in plans:
            bounds, taps = I.build_plan(n, S)
            plans[(n, S)] = len(rows)
            rows.append((sum(c.size for c in chunks), taps.shape[1], n, S))
            chunks.extend([bounds.reshape(-1), taps.reshape(-1)])
        return plans[(n, S)]

    for i, a in enumerate(imgs):
        h, w = a.shape[:2]
        cw, ch, cx, cy = (w, h, 0, 0) if crops is None or crops[i] is None else crops[i]
        desc.append((off, h, w, cx, cy, cw, ch, int(bool(flips[i])) if flips is not None else 0, plan(cw, S_w), plan(ch, S_h)))
        pad = -a.size % 16
        parts += [a.reshape(-1), np.full(pad, 0xAB, np.uint8)]           # padding that is NOT zero: nothing may read it into a result
        off += a.size + pad
    parts.append(np.full(16, 0xCD, np.uint8))
    return dict(pixels=torch.from_numpy(np.concatenate(parts)), desc=torch.tensor(desc, dtype=torch.int64).reshape(len(desc), ops.IMAGE_DESC),
                table=torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 4),
                data=torch.from_numpy(np.concatenate(chunks)) if chunks else torch.empty(0, dtype=torch.int32))


def launch(st, S_h, S_w, **over):
    a = dict(pixels=st["pixels"].to(DEV), desc=st["desc"], desc_dev=st["desc"].to(DEV), plan_table=st["table"],
             plan_table_dev=st["table"].to(DEV), plan_data=st["data"].to(DEV), lut=TAB.to(DEV))
    a.update(over)
    return ops.image_prep(a["pixels"], a["desc"], a["desc_dev"], a["plan_table"], a["plan_table_dev"], a["plan_data"], a["lut"], S_h, S_w)


def check(imgs, S_h, S_w, crops=None, flips=None):
    got = launch(stage(imgs, S_h, S_w, crops, flips), S_h, S_w)
    want = R.prep_batch(imgs, S_h, S_w, TAB, crops, flips)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(imgs), 3, S_h, S_w)
    assert torch.equal(got.cpu(), want), "%d of %d values differ" % (int((got.cpu() != want).sum()), want.numel())
    return got


def test_every_golden():
    """The reference's own outputs: Warp of every recorded image, MultiScaleCrop under every recorded seed, the flipped case."""
    g = H.load_golden("image_prep.npz")
    S = int(g["size"])
    prep = I.ImagePrep(size=S, mean=MEAN, std=STD, device=DEV)
    lut = lambda a: torch.stack([TAB[c][torch.from_numpy(np.ascontiguousarray(a[..., c])).long()] for c in range(3)])
    n = sum(1 for k in g.keys() if k.startswith("src_"))
    got = prep.warp([g["src_%d" % i] for i in range(n)]).cpu()
    for i in range(n):
        assert torch.equal(got[i], lut(g["warp_%d" % i])), "Warp, image %d" % i
    keys = [(int(s), int(i)) for s in g["seeds"] for i in g["crop_images"]]
    fs, fi = (int(v) for v in g["flip"])
    got = prep.train([g["src_%d" % i] for _, i in keys] + [g["src_%d" % fi]],
                     crops=[tuple(g["crop_s%d_i%d" % k]) for k in keys] + [tuple(g["crop_s%d_i%d" % (fs, fi)])],
                     flips=[False] * len(keys) + [True]).cpu()
    for j, k in enumerate(keys):
        assert torch.equal(got[j], lut(g["cropout_s%d_i%d" % k])), "MultiScaleCrop, seed %d image %d" % k
    assert torch.equal(got[-1], lut(g["flipout"]))
    assert prep.last_flips[-1] is True and prep.last_crops[0] == tuple(int(v) for v in g["crop_s%d_i%d" % keys[0]])


@pytest.mark.parametrize("S_h,S_w", [(1, 1), (8, 8), (30, 30), (33, 33), (64, 64), (30, 64), (8, 33),
                                     (17, 65)])       # 17 x 65: one row and one column past a tile boundary
def test_output_sizes(S_h, S_w):
    check([rnd(37, 53, 1), rnd(16, 16, 2), rnd(90, 24, 3)], S_h, S_w, flips=[False, True, False])


@pytest.mark.parametrize("name,shapes,S", [
    ("1x1", [(1, 1)], 8), ("2x3", [(3, 2)], 32),
    ("3W % 4 != 0", [(9, 7), (6, 53), (5, 10)], 16),       # 3W % 4 = 1, 3, 2
    ("identity", [(32, 32)], 32), ("upscale 7 -> 32", [(7, 7)], 32),
    ("1000x16 -> 16", [(16, 1000)], 16), ("16x1000 -> 16", [(1000, 16)], 16),        # 127 taps: taps from global memory
    ("300x40 -> 32", [(40, 300)], 32),
    ("7x and just above: the LDS-taps threshold", [(20, 224), (20, 225)], 32),       # 15 and 17 taps per output
    ("three chunks per row", [(4, 3000)], 8),                                        # a 3000-pixel segment, 1344 per chunk
    ("extent limits", [(2, 8192), (8192, 2)], 1),                                    # 16385 taps, seven chunks; 8192 rows
    ("500x375 -> 448", [(375, 500)], 448),
])
def test_sources(name, shapes, S):
    check([rnd(h, w, 10 + i) for i, (h, w) in enumerate(shapes)], S, S)


def test_crops_at_odd_offsets_and_at_the_edges_of_the_last_image():
    imgs = [rnd(37, 53, 20), rnd(41, 43, 21), rnd(24, 90, 22)]
    # (crop_w, crop_h, x, y): odd offsets and extents; the last image's crops end at its right and bottom edges, i.e. at the last
    # pixel of the buffer, where only the 16 bytes of slack follow
    check(imgs, 32, 32, crops=[(21, 17, 5, 3), (17, 29, 1, 7), (33, 11, 57, 13)])
    check(imgs, 30, 33, crops=[(1, 1, 52, 36), (43, 1, 0, 40), (90, 24, 0, 0)], flips=[True, False, True])
    check(imgs[:2] + [rnd(24, 90, 23)], 16, 16, crops=[None, (3, 5, 39, 35), (7, 9, 83, 15)])


@pytest.mark.parametrize("S", [32, 33, 130])
def test_flips_with_odd_and_even_sizes(S):
    """The mirror is exact for an even and an odd S, and across tiles (130 = two tiles and two columns)."""
    imgs = [rnd(37, 53, 30), rnd(64, 48, 31)]
    a = check(imgs, S, S, flips=[True, True])
    b = check(imgs, S, S, flips=[False, False])
    assert torch.equal(a, b.flip(3))


def test_empty_batch():
    assert tuple(check([], 8, 8).shape) == (0, 3, 8, 8)
    prep = I.ImagePrep(size=8, device=DEV)
    assert tuple(prep.warp([]).shape) == (0, 3, 8, 8) and tuple(prep.train([]).shape) == (0, 3, 8, 8)


def test_five_images_that_share_two_plans():
    imgs = [rnd(20, 30, 40), rnd(30, 20, 41), rnd(20, 20, 42), rnd(30, 30, 43), rnd(40, 50, 44)]
    crops = [None, None, None, None, (30, 20, 11, 7)]
    st = stage(imgs, 16, 16, crops)
    assert st["table"].shape[0] == 2 and st["desc"][:, 8:].unique().tolist() == [0, 1]
    assert torch.equal(launch(st, 16, 16).cpu(), R.prep_batch(imgs, 16, 16, TAB, crops))
    prep = I.ImagePrep(size=16, mean=MEAN, std=STD, device=DEV)
    got = prep.train(imgs, crops=[(30, 20, 0, 0), (20, 30, 0, 0), (20, 20, 0, 0), (30, 30, 0, 0), (30, 20, 11, 7)], flips=[False] * 5)
    assert prep.plan_table().shape[0] == 2 and torch.equal(got.cpu(), R.prep_batch(imgs, 16, 16, TAB, crops))


def test_the_same_call_twice_and_the_sampled_training_transform():
    imgs = [rnd(375, 500, 50), rnd(120, 90, 51), rnd(64, 64, 52)]
    prep = I.ImagePrep(size=64, mean=MEAN, std=STD, device=DEV)
    a, b = prep.warp(imgs), prep.warp(imgs)                   # the two calls go through different slots of the pinned ring
    assert torch.equal(a, b) and torch.equal(a.cpu(), R.prep_batch(imgs, 64, 64, TAB))
    import random
    random.seed(4)
    torch.manual_seed(4)
    t = prep.train(imgs)                                     # crops and flips sampled as the reference samples them
    assert len(prep.last_crops) == 3 and len(prep.last_flips) == 3
    assert torch.equal(t.cpu(), R.prep_batch(imgs, 64, 64, TAB, prep.last_crops, prep.last_flips))
    random.seed(4)
    torch.manual_seed(4)
    crops, flips = prep.last_crops, prep.last_flips
    assert torch.equal(prep.train(imgs), t) and prep.last_crops == crops and prep.last_flips == flips
    for _ in range(3):                                       # the ring wraps: a re-used slot is a finished one
        assert torch.equal(prep.warp(imgs), a)


def test_model_takes_the_prepared_images():
    """Images -> logits in eval mode: the model fed prep.warp(...) equals the model fed the restatement's tensor."""
    cfg = synth.CONFIGS["mvsa_single_b8"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=2, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV)
    model.object_features = trunk.ResNetFeatures(synth.fill_trunk_(trunk.ResNet([1, 1, 1, 1]), 1)).to(DEV)        # one block per stage
    model.place_features = trunk.ResNetFeatures(synth.fill_trunk_(trunk.ResNet([1, 1, 1, 1], 365), 2)).to(DEV)
    model.eval()
    args = list(harness.call_args(inp, DEV))
    prep = model.image_prep(448)
    assert isinstance(prep, I.ImagePrep) and prep.size == 448 and prep.device == torch.device(DEV)
    assert torch.equal(prep.table, R.table(model.image_normalization_mean, model.image_normalization_std))
    imgs = [rnd(60, 45, 60), rnd(50, 70, 61)]
    with torch.no_grad():
        out = model(*args[:3], prep.warp(imgs), prep.warp(imgs), *args[5:])
        ref_in = R.prep_batch(imgs, 448, 448, TAB).to(DEV)
        ref = model(*args[:3], ref_in, ref_in.clone(), *args[5:])
    assert torch.isfinite(out).all() and torch.equal(out, ref)


def test_ops_image_prep_refusals():
    imgs = [rnd(20, 30, 70), rnd(9, 7, 71)]
    st = stage(imgs, 8, 8)
    assert tuple(launch(st, 8, 8).shape) == (2, 3, 8, 8)

    def desc(i, col, v):
        d = st["desc"].clone()
        d[i, col] = v
        return d

    for d, what in ((desc(0, 5, 31), "crop outside"), (desc(1, 4, 2), "crop outside"), (desc(0, 3, -1), "crop outside"),
                    (desc(1, 0, st["desc"][1, 0] + 8), "multiple of 16"), (desc(1, 0, st["desc"][1, 0] + 16), "does not fit"),
                    (desc(0, 8, 4), "plan index"), (desc(1, 9, -1), "plan index"), (desc(0, 8, st["desc"][0, 9]), "horizontal plan"),
                    (desc(0, 1, 8193), "source extent"), (desc(0, 7, 2), "flip")):
        with pytest.raises(ValueError, match=what):
            launch(st, 8, 8, desc=d)
    with pytest.raises(ValueError, match="vertical plan"):
        launch(st, 9, 8)
    with pytest.raises(TypeError):
        launch(st, 8, 8, pixels=st["pixels"].to(DEV).float())
    with pytest.raises(TypeError):
        launch(st, 8, 8, desc=st["desc"].int())
    with pytest.raises(TypeError):
        launch(st, 8, 8, lut=TAB.to(DEV).double())
    with pytest.raises(TypeError):
        launch(st, 8, 8, plan_data=st["data"].to(DEV).long())
    with pytest.raises(ValueError, match="HOST copy"):
        launch(st, 8, 8, desc=st["desc"].to(DEV))
    with pytest.raises(RuntimeError, match="GPU only"):
        launch(st, 8, 8, pixels=st["pixels"])
    with pytest.raises(ValueError, match="shapes of their host copies"):
        launch(st, 8, 8, desc_dev=st["desc"][:1].to(DEV))
    with pytest.raises(ValueError, match="contiguous"):
        launch(st, 8, 8, desc_dev=st["desc"].to(DEV).t().contiguous().t())
    with pytest.raises(ValueError, match="lut must be"):
        launch(st, 8, 8, lut=TAB[:2].to(DEV).contiguous())
    with pytest.raises(ValueError, match="16-byte boundary"):
        launch(st, 8, 8, pixels=torch.cat([st["pixels"][:1], st["pixels"]]).to(DEV)[1:])
    t = st["table"].clone()
    t[1, 0] = st["data"].numel()
    with pytest.raises(ValueError, match="not a plan inside plan_data"):
        launch(st, 8, 8, plan_table=t)
    for S in ((0, 8), (8, 1025)):
        with pytest.raises(ValueError, match="unsupported"):
            launch(st, *S)


def test_a_bad_device_descriptor_gives_nan_not_a_read():
    """ops.image_prep validates the HOST descriptors; the kernel reads the device copy, which can change under a captured graph.
    A device descriptor the kernel's own check rejects fills that image with NaN and leaves the others as they are.  (The cases
    are ones that would stay inside the buffers even if the check let them through.)"""
    imgs = [rnd(20, 30, 80), rnd(9, 7, 81), rnd(12, 12, 82)]
    st = stage(imgs, 17, 65)
    want = R.prep_batch(imgs, 17, 65, TAB)
    for col, v in ((5, 8), (3, 1), (6, 10), (4, 1), (8, st["table"].shape[0]), (9, -1), (8, int(st["desc"][1, 9])), (0, int(st["desc"][1, 0]) + 8)):
        d = st["desc"].clone()
        d[1, col] = v                          # image 1 is 9 x 7: crop wider / taller than it or shifted out, bad plans, a bad offset
        got = launch(st, 17, 65, desc_dev=d.to(DEV)).cpu()
        assert torch.isnan(got[1]).all(), (col, v)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), (col, v)


def test_plans_are_appended_batch_after_batch():
    """The device plan buffers grow by appending: 35 images with 70 distinct extents outgrow the first plan table (64 rows), later
    batches use old and new plans together, and every result stays exact."""
    prep = I.ImagePrep(size=8, mean=MEAN, std=STD, device=DEV)
    first = [rnd(9, 11, 90), rnd(11, 9, 91)]
    a = prep.warp(first)
    assert prep.plan_table().shape[0] == 2
    many = [rnd(20 + i, 60 + i, 100 + i) for i in range(35)]
    assert torch.equal(prep.warp(many).cpu(), R.prep_batch(many, 8, 8, TAB)) and prep.plan_table().shape[0] == 72
    mixed = [first[1], many[34], rnd(13, 9, 92), many[0]]
    assert torch.equal(prep.warp(mixed).cpu(), R.prep_batch(mixed, 8, 8, TAB)) and prep.plan_table().shape[0] == 73
    assert torch.equal(prep.warp(first), a) and torch.equal(a.cpu(), R.prep_batch(first, 8, 8, TAB))
