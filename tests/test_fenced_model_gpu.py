"""The whole model once into fenced, poisoned buffers (tests/fenced_alloc.py): the smallest configuration, mvsa_single_b8, with a batch
whose last samples are empty.  Each case runs plainly; then a second model is built from the same seeds inside `fenced(...)`, so that
its derived packs, caches, plans and launch scratch come out of the arena, and runs there on fenced inputs and a fresh stream.  Equal
bits and a clean arena.check() are required: a read of unwritten memory anywhere on these paths reaches the logits or a gradient as
NaN, a store outside a buffer lands in a fence.  Eager only: nothing here captures a hipGraph (the arena's fills synchronise)."""
import numpy as np
import pytest
import torch

from mgnns_amd import optim, synth, train, trunk
from tests import model_util as MU
from tests import test_fenced_kernels_gpu as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = "mvsa_single_b8"
# the label GCN's scratch and memo state hold more than counters by their stated contract (the table of tests/test_fenced_kernels_gpu.py)
STATEFUL = ("label_gcn",)


def build(B=None, empty=2, with_trunks=False):
    """(model on the device in eval mode, the inputs as host arrays): the seeded harness; the last `empty` samples have no token."""
    cfg = synth.CONFIGS[CFG]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = MU.synthetic_adjacencies(cfg)
    inp = {k: np.array(v) for k, v in synth.make_inputs(cfg, B=B or cfg.B, seed=7, pmi=pmi).items()}
    if empty:
        inp["text"][-empty:] = 0
        inp["text_lens"][-empty:] = 0
        inp["text_mask"][-empty:] = 0
    model = MU.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV)
    if with_trunks:                                      # one block per stage, as tests/test_image_prep_gpu.py builds them
        model.object_features = trunk.ResNetFeatures(synth.fill_trunk_(trunk.ResNet([1, 1, 1, 1]), 1)).to(DEV)
        model.place_features = trunk.ResNetFeatures(synth.fill_trunk_(trunk.ResNet([1, 1, 1, 1], 365), 2)).to(DEV)
    return cfg, model, inp


def same_bits(case, family):
    """case(put) -> tensors, with put(host array) -> device tensor; plain, then fenced on a fresh stream; K.same_bits' criterion."""
    return K.same_bits(case, family, stateful=STATEFUL)


@pytest.mark.parametrize("attention", ["folded", "faithful"])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_eval_forward(precision, attention):
    def case(put):
        cfg, model, inp = build()
        model.set_precision(precision).set_attention(attention)
        args = [put(a) for a in MU.call_args(inp, "cpu")]
        with torch.no_grad():
            first = model(*args).float().clone()
            second = model(*args).float().clone()          # the cached packs, plans and memos of the first forward
        return first, second
    same_bits(case, "model eval")


def step_case(put, with_trunks):
    B = 2 if with_trunks else None
    cfg, model, inp = build(B=B, empty=1 if with_trunks else 2, with_trunks=with_trunks)
    args = [put(a) for a in MU.call_args(inp, "cpu")]
    if with_trunks:
        g = torch.Generator().manual_seed(3)
        args[3], args[4] = (put(torch.randn(args[0].shape[0], 3, 448, 448, generator=g)) for _ in range(2))
    target = put(np.random.default_rng(7).integers(0, cfg.NL, args[0].shape[0]))
    model.train().freeze_text_encoders()                 # the reference's dropout rates stay as built
    if with_trunks:
        model.unfreeze_trunks(batchnorm="batch")
    opt = optim.Adam(model.get_config_optim(1e-3, 0.1), lr=1e-3, max_norm=1e-2, norm_params=model.parameters())
    model.zero_grad(set_to_none=True)
    torch.manual_seed(99)
    logits = model(*args)
    loss = train.cross_entropy(logits, target)
    loss.backward()
    named = [(k, p) for k, p in model.named_parameters() if p.grad is not None]
    assert named and (not with_trunks or any("_features." in k for k, _ in named))
    grads = [p.grad.clone() for _, p in named]
    opt.step()
    assert float(opt.clip_coef) < 1.0, "the clip must be engaged"
    return logits.detach(), loss.detach(), grads, opt.total_norm.clone(), [p.detach().clone() for _, p in named]


def test_training_step_at_the_reference_dropout_rates():
    same_bits(lambda put: step_case(put, False), "model train")


def test_training_step_with_the_trunks_last_stage_unfrozen_under_batch_statistics():
    same_bits(lambda put: step_case(put, True), "model train")
