"""Training mode of the fusion layers (csrc/mha_train.hip, mgnns_amd/train.py) against torch autograd in fp64 on the CPU over
the reference's formulation of MyMultiHeadAttention (models/moudles.py:198-230, models/submodules.py:15-156): K and V projected,
dropout applied with the keep masks the kernels drew.  Gate: fp32-class error, 1e-4 of each gradient's largest magnitude."""
import math

import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import fusion, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, DK = 300, 128

PNAMES = ["slf_attn.w_qs.weight", "slf_attn.w_qs.bias", "slf_attn.w_ks.weight", "slf_attn.w_ks.bias", "slf_attn.w_vs.weight",
          "slf_attn.w_vs.bias", "slf_attn.fc.weight", "slf_attn.fc.bias", "slf_attn.layer_norm.gamma",
          "slf_attn.layer_norm.beta", "pos_ffn.w_1.weight", "pos_ffn.w_1.bias", "pos_ffn.w_2.weight", "pos_ffn.w_2.bias",
          "pos_ffn.layer_norm.gamma", "pos_ffn.layer_norm.beta"]


def make_layer(H, rate=0.0, attn_rate=0.0, seed=0):
    torch.manual_seed(seed)
    m = fusion.MyMultiHeadAttention(H, D, DK, dropout=rate)
    with torch.no_grad():                       # LayerNorm gamma / beta away from 1 / 0 so that their gradients are tested
        for ln in (m.slf_attn.layer_norm, m.pos_ffn.layer_norm):
            ln.gamma.add_(0.3 * torch.randn(D))
            ln.beta.add_(0.3 * torch.randn(D))
    m.slf_attn.attn_dropout.p = attn_rate
    return m.to(DEV).train()


def inputs(B, L, masked, seed=1):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, D, generator=g)
    bank = torch.randn(B, L, D, generator=g)
    mask = None
    if masked:
        lens = torch.randint(1, L + 1, (B,), generator=g)
        lens[0] = L
        mask = (torch.arange(L)[None, :] < lens[:, None]).float()
    G = torch.randn(B, D, generator=g)
    return q, bank, mask, G


def ln_ref(x, gamma, beta, eps=1e-6):
    return gamma * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + eps) + beta


def layer_ref(p, q, bank, mask, H, keeps=None, rates=(0.0, 0.0, 0.0)):
    """fp64 restatement of one layer in training mode; keeps = (attn [H*B,1,L], fc [B,D], ffn [B,D]) bool or None."""
    B, L, _ = bank.shape
    a = "slf_attn."
    f = "pos_ffn."
    qh = F.linear(q, p[a + "w_qs.weight"], p[a + "w_qs.bias"]).view(B, H, DK)
    kh = F.linear(bank, p[a + "w_ks.weight"], p[a + "w_ks.bias"]).view(B, L, H, DK)
    vh = F.linear(bank, p[a + "w_vs.weight"], p[a + "w_vs.bias"]).view(B, L, H, DK)
    s = torch.einsum("bhd,blhd->bhl", qh, kh) / math.sqrt(DK)
    if mask is not None:
        s = s.masked_fill(mask[:, None, :] == 0, float("-inf"))
    pa = torch.softmax(s, dim=2)

    def drop(x, k, r):
        return x if k is None else x * k.to(x.dtype) / (1.0 - r)

    ka, kf, kn = keeps if keeps is not None else (None, None, None)
    pd = drop(pa, None if ka is None else ka.view(H, B, L).permute(1, 0, 2), rates[0])
    o = torch.einsum("bhl,blhd->bhd", pd, vh).reshape(B, H * DK)
    y = ln_ref(drop(F.linear(o, p[a + "fc.weight"], p[a + "fc.bias"]), kf, rates[1]) + q, p[a + "layer_norm.gamma"],
               p[a + "layer_norm.beta"])
    z = F.linear(F.relu(F.linear(y, p[f + "w_1.weight"].squeeze(-1), p[f + "w_1.bias"])), p[f + "w_2.weight"].squeeze(-1),
                 p[f + "w_2.bias"])
    out = ln_ref(drop(z, kn, rates[2]) + y, p[f + "layer_norm.gamma"], p[f + "layer_norm.beta"])
    return out, pd.permute(1, 0, 2).reshape(H * B, 1, L)


def cpu_params(m):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()}


def masks_of(m, B, L, H):
    """The keep masks of the module's last training forward, redrawn through the ops from the seeds it kept."""
    a, f = m.slf_attn, m.pos_ffn
    z = torch.zeros(B, D, device=DEV)
    one, zero = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    qh = torch.zeros(B, H * DK, device=DEV)
    bank = torch.zeros(B, L, D, device=DEV)
    *_, ka = ops.mha_attn_train(qh, bank, None, H, DK, a.w_ks.weight.detach(), a.w_vs.weight.detach(), a.w_vs.bias.detach(),
                                a.last_dropout_seed, a.attn_dropout.p, return_masks=True)
    *_, kf = ops.dropout_residual_layernorm(z, z, one, zero, 1e-6, a.last_dropout_seed, ops.DROP_FC, a.dropout.p,
                                            return_masks=True)
    *_, kn = ops.dropout_residual_layernorm(z, z, one, zero, 1e-6, f.last_dropout_seed, ops.DROP_FFN, f.dropout.p,
                                            return_masks=True)
    return ka.cpu(), kf.cpu(), kn.cpu()


def run_and_compare(H, B, L, masked, rate=0.0, attn_rate=0.0):
    m = make_layer(H, rate, attn_rate, seed=H * 31 + B)
    q, bank, mask, G = inputs(B, L, masked, seed=B + L)
    qd = q.to(DEV).requires_grad_(True)
    bd = bank.to(DEV).requires_grad_(True)
    out, attn = m(qd, bd, bd, None if mask is None else mask.to(DEV))
    (out * G.to(DEV)).sum().backward()
    keeps = masks_of(m, B, L, H) if (rate or attn_rate) else None
    p = cpu_params(m)
    qc = q.double().requires_grad_(True)
    bc = bank.double().requires_grad_(True)
    ref, ref_attn = layer_ref(p, qc, bc, mask, H, keeps, (attn_rate, rate, rate))
    (ref * G.double()).sum().backward()
    assert_close(out, ref, "out")
    assert_close(attn, ref_attn, "attn")
    sd = dict(m.named_parameters())
    for k in PNAMES:
        assert_close(sd[k].grad, p[k].grad, k)
    assert_close(qd.grad, qc.grad, "q")
    assert_close(bd.grad, bc.grad, "bank")
    if mask is not None:
        assert (bd.grad.cpu()[mask == 0] == 0).all()           # masked rows get exactly zero
    return m, keeps


def assert_close(got, ref, name, tol=1e-4):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    assert err <= tol * scale + 1e-9, "%s: max err %.3g, max |ref| %.3g" % (name, err, scale)


@pytest.mark.parametrize("H,B,L,masked", [(1, 7, 100, True), (4, 256, 196, False), (8, 7, 196, False), (4, 1, 100, True),
                                          (8, 256, 100, True), (1, 1, 196, False)])
def test_layer_gradients_match_fp64_autograd(H, B, L, masked):
    run_and_compare(H, B, L, masked)


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("H,B,L,masked", [(4, 256, 196, False), (8, 7, 100, True)])
def test_layer_with_dropout_matches_under_returned_masks(H, B, L, masked, rate):
    m, keeps = run_and_compare(H, B, L, masked, rate=rate, attn_rate=rate)
    for k in keeps[1:]:                  # [B, D] masks: keep fraction within 6 sigma of the binomial
        n = k.numel()
        assert abs(k.float().mean().item() - (1 - rate)) <= 6 * math.sqrt(rate * (1 - rate) / n)
    ka = keeps[0]
    n = ka.numel()
    assert abs(ka.float().mean().item() - (1 - rate)) <= 6 * math.sqrt(rate * (1 - rate) / n)


def test_same_seed_is_bit_identical():
    B, L, H = 64, 100, 4
    q, bank, mask, G = inputs(B, L, True, seed=5)

    def once():
        m = make_layer(H, 0.3, 0.2, seed=9)
        qd = q.to(DEV).requires_grad_(True)
        bd = bank.to(DEV).requires_grad_(True)
        torch.manual_seed(1234)
        out, attn = m(qd, bd, bd, mask.to(DEV))
        (out * G.to(DEV)).sum().backward()
        return [out, attn, qd.grad, bd.grad] + [p.grad for p in m.parameters()]

    a, b = once(), once()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    m = make_layer(H, 0.3, 0.2, seed=9)
    torch.manual_seed(99)
    bd = bank.to(DEV)
    out, _ = m(q.to(DEV), bd, bd, mask.to(DEV))
    assert not torch.equal(out, a[0])                          # another seed, other masks


def test_stack_over_shared_bank_accumulates_the_bank_gradient():
    B, L, H = 32, 100, 4
    q, bank, mask, G = inputs(B, L, True, seed=11)
    layers = [make_layer(H, seed=40 + i) for i in range(3)]
    bd = bank.to(DEV).requires_grad_(True)
    mb = fusion.MemoryBank(f32=bd)
    x = q.to(DEV)
    for layer in layers:
        x, _ = layer(x, mb, mb, mask.to(DEV))
    (x * G.to(DEV)).sum().backward()
    bc = bank.double().requires_grad_(True)
    xr = q.double()
    ps = [cpu_params(layer) for layer in layers]
    for p in ps:
        xr, _ = layer_ref(p, xr, bc, mask, H)
    (xr * G.double()).sum().backward()
    assert_close(bd.grad, bc.grad, "bank")
    for layer, p in zip(layers, ps):
        assert_close(layer.slf_attn.w_ks.weight.grad, p["slf_attn.w_ks.weight"].grad, "w_ks")


def test_optimizer_steps_track_fp64_and_eval_uses_the_new_weights():
    B, L, H = 16, 100, 4
    q, bank, mask, G = inputs(B, L, True, seed=21)
    m = make_layer(H, seed=3)
    p = cpu_params(m)
    names = [k for k, _ in m.named_parameters()]
    opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
    opt_ref = torch.optim.SGD([p[k] for k in names], lr=1e-2, momentum=0.9)
    qd, bd, md = q.to(DEV), bank.to(DEV), mask.to(DEV)
    m.eval()
    out0 = m(qd, bd, bd, md)[0].detach().clone()
    y0 = fusion.run_stack([m], qd, bd, md).detach().clone()
    m.train()
    for _ in range(3):
        opt.zero_grad()
        (m(qd, bd, bd, md)[0] * G.to(DEV)).sum().backward()
        opt.step()
        opt_ref.zero_grad()
        (layer_ref(p, q.double(), bank.double(), mask, H)[0] * G.double()).sum().backward()
        opt_ref.step()
    sd = dict(m.named_parameters())
    for k in names:
        assert_close(sd[k], p[k], k, tol=1e-5)
    m.eval()
    with torch.no_grad():
        ref = layer_ref(p, q.double(), bank.double(), mask, H)[0]
    out1 = m(qd, bd, bd, md)[0]
    y1 = fusion.run_stack([m], qd, bd, md)
    assert_close(out1, ref, "eval after steps")
    assert_close(y1, ref, "run_stack after steps")
    assert (out1 - out0).abs().max() > 1e-4 and (y1 - y0).abs().max() > 1e-4


def test_training_refusals():
    B, L = 4, 20
    q, bank, mask, _ = inputs(B, L, True, seed=2)
    qd, bd, md = q.to(DEV), bank.to(DEV), mask.to(DEV)
    m = make_layer(4)
    for prec in ("bf16", "bf16x3"):
        m.slf_attn.precision = prec
        with pytest.raises(NotImplementedError, match="fp32"):
            m(qd, bd, bd, md)
    m.slf_attn.precision = 'fp32'
    m.slf_attn.attention = 'folded'
    m(qd, bd, bd, md)                                           # the maths is the same: folded trains too
    r = fusion.MyMultiHeadAttention(4, D, DK, is_regu=True).to(DEV).train()
    with pytest.raises(NotImplementedError, match="is_regu"):
        r(qd, bd, bd, md)
    with pytest.raises(RuntimeError, match="eval"):
        fusion.run_stack([m], qd, bd, md)
    big = make_layer(4)
    with pytest.raises(ValueError, match="L <= 208"):
        long_bank = torch.zeros(2, 209, D, device=DEV)
        big(torch.zeros(2, D, device=DEV), long_bank, long_bank)


def test_weight_gradient_kernel_is_exact_and_deterministic():
    g = torch.Generator().manual_seed(7)
    for M, N, K in [(1, 5, 3), (256, 300, 300), (300, 128, 300), (1000, 33, 65)]:
        dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
        dW, db = ops.wgrad(dy.to(DEV), x.to(DEV))
        assert_close(dW, dy.double().t() @ x.double(), "dW", tol=2e-6)
        assert_close(db, dy.double().sum(0), "db", tol=2e-6)
        dW2, _ = ops.wgrad(dy.to(DEV), x.to(DEV))
        assert torch.equal(dW, dW2)
