"""The trunk's per-layer derived packs on the GPU (trunk.layer_pack): a superseded pack is parked while a capture
lives -- checked on the host, no graph is replayed over a retired pack -- and the eval forward and fine-tuning, which share one folded
tensor per layer, both see an update."""
import pytest
import torch

from mgnns_amd import ops, synth, trunk
from tests.test_trunk_train_cpu import narrow_stage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def update_and_look_up(blk):
    """Look up, update conv2.weight as an optimizer does, look up again -> (the superseded entries, their wt and wT with the
    addresses they had, the new wt and wT)."""
    old = trunk.block_packs(blk)[1]
    store = blk.conv2._packs
    entries = [store["folded"], store["folded.T"]]
    assert entries[0][2][0] is old[0] and entries[1][2] is old[2]
    held = [(t, t.data_ptr()) for t in (old[0], old[2])]
    with torch.no_grad():
        blk.conv2.weight.add_(1)
    new = trunk.block_packs(blk)[1]
    assert store["folded"] is not entries[0] and store["folded.T"] is not entries[1]
    return entries, held, (new[0], new[2])


def test_a_superseded_pack_is_parked_while_a_capture_lives(monkeypatch):
    monkeypatch.setattr(ops, "_LIVE_CAPTURES", 0)
    monkeypatch.setattr(ops, "_RETIRED", [])
    blk = narrow_stage(128, 64, 2, 2, 3).to(DEV)[0]
    ops.capture_born()
    try:
        entries, held, new = update_and_look_up(blk)
        assert len(ops._RETIRED) == 2 and all(any(r is e for r in ops._RETIRED) for e in entries)
        for (t, ptr), n in zip(held, new):
            assert t.data_ptr() == ptr and t.untyped_storage().nbytes() > 0 and n.data_ptr() != ptr
        assert not torch.equal(held[0][0], new[0])
    finally:
        ops.capture_gone()
    assert not ops._RETIRED
    update_and_look_up(blk)                                             # no capture alive: nothing is parked
    assert not ops._RETIRED


def small_trunk(state=None):
    f = trunk.ResNetFeatures(synth.fill_trunk_(trunk.ResNet((1, 1, 1, 1)), 1) if state is None else trunk.ResNet((1, 1, 1, 1)))
    if state is not None:
        f.load_state_dict(state)
    return f.to(DEV).eval()


def image():
    return torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)


def test_the_eval_forward_sees_an_updated_weight_as_a_fresh_trunk_does():
    f, img = small_trunk(), image()
    with torch.no_grad():
        before = f(img)
        f[7][0].conv2.weight.mul_(1.5)
        f[4][0].bn1.running_var.mul_(2.0)
        after = f(img)
        assert not torch.equal(after, before)
        assert torch.equal(after, small_trunk(f.state_dict())(img))


@pytest.mark.parametrize("kw", [dict(stages=2), dict(stages=2, batchnorm="batch"), dict(stages=4, stem=True)], ids=["frozen", "batch", "stem"])
def test_eval_after_a_fine_tuning_step_equals_a_fresh_trunk(kw):
    f, img = small_trunk(), image()
    with torch.no_grad():
        before = f(img)                                                 # the eval plan holds the packs that training shares
    out = f.forward_train(img, **kw)
    assert kw.get("batchnorm") == "batch" or torch.equal(out.detach(), before)
    out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV))
    with torch.no_grad():
        for p in f.parameters():
            if p.grad is not None:
                p.sub_(1e-2 * p.grad / p.grad.abs().max().clamp_min(1e-30))
        after = f(img)
        again = f.forward_train(img, **kw).detach() if kw.get("batchnorm") != "batch" else None
        assert torch.isfinite(after).all() and not torch.equal(after, before)
        assert again is None or torch.equal(again, after)
        assert torch.equal(after, small_trunk(f.state_dict())(img))
