"""Gradients of the training step with respect to the two [B,2048,h,w] feature maps (csrc/map_grad.hip, train.ImgBankFunction):
dX[b,k,p] = sum_o W[o,k] dBank[b,p,o] + [p == first argmax_p X[b,k,:]] dPooled[b,k], against torch autograd in fp64 on the CPU.
Gate: the training gate, 1e-4 of the reference tensor's largest magnitude (tests/test_model_train_gpu.py::close).  The dense part
is gated on its own: the max-pool's sparse contributions are larger and would loosen a gate taken on the sum."""
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import harness, ops
from mgnns_amd import train as T
from tests import test_model_train_gpu as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
close = M.close


@pytest.fixture(autouse=True)
def _rng_state_as_found():
    """These tests seed and draw from torch's default generators (dropout seeds, model initialisation); the tests that run after
    them find the generators as they were."""
    with torch.random.fork_rng(devices=[0]):
        yield


# ---- the dense part alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,P,N", [
    (3, 200, 49, 37),            # K no multiple of any tile, P odd, N small
    (2, 2048, 196, 300),         # the product shape
    (1, 16, 1, 1),
    (2, 144, 208, 320),          # the limits of one position block and of N
    (5, 130, 17, 304),
    (2, 72, 250, 24),            # more than one position block: rows are no longer one contiguous range
    (9, 16, 5, 8),               # more samples than the 8 the block map interleaves
])
def test_dense_part_matches_fp64(B, K, P, N):
    g = torch.Generator().manual_seed(B * 1000 + P)
    dbank = torch.randn(B, P, N, generator=g)
    W = torch.randn(N, K, generator=g)
    ref = torch.einsum("ok,bpo->bkp", W.double(), dbank.double())
    out = torch.full((B, K, P), float("nan"), device=DEV)
    got = ops.imgbank_dgrad(dbank.to(DEV), W.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any(), "elements of dX left unwritten"
    close(out, ref, "dX")
    again = ops.imgbank_dgrad(dbank.to(DEV), W.to(DEV))
    assert again.shape == (B, K, P) and torch.equal(again, out)


def test_dgrad_refusals_and_empty_batch():
    W = torch.zeros(320, 16, device=DEV)
    assert ops.imgbank_dgrad(torch.zeros(0, 4, 320, device=DEV), W).shape == (0, 16, 4)
    with pytest.raises(RuntimeError, match="N <= 320"):
        ops.imgbank_dgrad(torch.zeros(2, 4, 321, device=DEV), torch.zeros(321, 16, device=DEV))
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(torch.zeros(2, 4, 300, device=DEV), W)                       # N mismatch
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(torch.zeros(2, 4, 320, device=DEV), W, dpooled=torch.zeros(2, 16, device=DEV))     # no arg
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(torch.zeros(2, 4, 320, device=DEV), W, torch.zeros(3, 16, device=DEV),
                          torch.zeros(3, 16, device=DEV, dtype=torch.int32))           # B mismatch
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(None, W)
    with pytest.raises(ValueError):
        ops.map_argmax(torch.zeros(2, 16, device=DEV))
    assert ops.map_argmax(torch.zeros(0, 16, 4, device=DEV)).shape == (0, 16)


# ---- argmax: the first maximum ----------------------------------------------------------------------------------------------
def tied_map(B, K, P, seed=0):
    """A ReLU'd random map [B, K, P] whose rows cover the tie cases: all-zero rows, a maximum planted at two and at three
    positions, a maximum at the last position, negative-only rows (one of them with its maximum twice)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, K, P, generator=g))
    rows = x.view(B * K, P)
    pos = sorted({P // 5, P // 2, P - 1})
    for r in range(0, B * K, 7):
        kind = (r // 7) % 6
        if kind == 0:
            rows[r] = 0.0
        elif kind == 1:
            rows[r, pos[:2]] = 9.0
        elif kind == 2:
            rows[r, pos] = 7.5
        elif kind == 3:
            rows[r, P - 1] = 11.0
        elif kind == 4:
            rows[r] = -1.0 - torch.rand(P, generator=g)
        else:
            rows[r] = -1.0 - torch.rand(P, generator=g)
            rows[r, pos[-2:]] = -0.5
    return x


def host_argmax(x):
    B, K, P = x.shape
    _, idx = F.max_pool2d(x.reshape(B, K, 1, P), (1, P), return_indices=True)
    return idx.view(B, K).to(torch.int32)


@pytest.mark.parametrize("P", [1, 49, 196, 208, 250, 260])      # 250: the unaligned path in 4 steps; 260: the aligned one in 2
def test_argmax_is_the_first_maximum(P):
    x = tied_map(3, 200, P, seed=P)
    ref = host_argmax(x)
    flat = x.view(-1, P)
    assert P == 1 or (flat == flat.max(dim=1, keepdim=True).values).sum(dim=1).max() >= 2, "no tie in the input"
    got = ops.map_argmax(x.to(DEV))
    assert got.dtype == torch.int32 and got.shape == (3, 200)
    assert torch.equal(got.cpu(), ref)
    if P > 1:
        assert int(got.view(-1)[0]) == 0                                # the all-zero row
        assert int(got.view(-1)[21]) == P - 1                           # the maximum at the last position


def test_argmax_row_counts_off_the_wave_group():
    x = tied_map(1, 13, 12, seed=5)                # 13 rows: the last group of 4 rows is partial
    assert torch.equal(ops.map_argmax(x.to(DEV)).cpu(), host_argmax(x))


# ---- the max-pool scatter in the epilogue -------------------------------------------------------------------------------------
def map_grad_ref(x, W, dbank, dpooled, hw):
    """fp64 autograd of F.linear + F.max_pool2d (which pins the tie rule) -> d x."""
    B, K, P = x.shape
    xd = x.double().requires_grad_(True)
    loss = 0.0
    if dbank is not None:
        loss = loss + (F.linear(xd.permute(0, 2, 1), W.double()) * dbank.double()).sum()
    if dpooled is not None:
        loss = loss + (F.max_pool2d(xd.view(B, K, *hw), hw).view(B, K) * dpooled.double()).sum()
    loss.backward()
    return xd.grad


@pytest.mark.parametrize("B,K,hw,N", [(3, 200, (7, 7), 37), (2, 144, (14, 14), 300), (2, 40, (25, 10), 24)])
def test_scatter_goes_to_the_first_maximum(B, K, hw, N):
    P = hw[0] * hw[1]
    g = torch.Generator().manual_seed(11)
    x = tied_map(B, K, P, seed=P + 1)
    W, dbank, dpooled = torch.randn(N, K, generator=g), torch.randn(B, P, N, generator=g), torch.randn(B, K, generator=g)
    xg, Wg, dbg, dpg = (t.to(DEV) for t in (x, W, dbank, dpooled))
    arg = ops.map_argmax(xg)
    both = ops.imgbank_dgrad(dbg, Wg, dpg, arg)
    close(both, map_grad_ref(x, W, dbank, dpooled, hw), "dX")
    dense = ops.imgbank_dgrad(dbg, Wg)
    close(dense, map_grad_ref(x, W, dbank, None, hw), "dX bank only")
    pooled = ops.imgbank_dgrad(None, Wg, dpg, arg, positions=P)
    ref_p = map_grad_ref(x, W, None, dpooled, hw)
    assert torch.equal(pooled.cpu(), ref_p.float())                      # one value per row, copied: exact
    # the sum is the dense part plus one addition per row
    assert torch.equal(both, dense + pooled)
    assert torch.equal(ops.imgbank_dgrad(dbg, Wg, dpg, arg), both)


# ---- ImgBankFunction ----------------------------------------------------------------------------------------------------------
def bank_inputs(B=3, K=144, hw=(6, 6), N=37, seed=2):      # (the forward kernel takes P % 4 == 0, K % 16 == 0)
    P = hw[0] * hw[1]
    g = torch.Generator().manual_seed(seed)
    x = tied_map(B, K, P, seed=seed)
    W, c = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    Gb, Gp = torch.randn(B, P, N, generator=g), torch.randn(B, K, generator=g)
    return x, W, c, Gb, Gp


def run_function(x, W, c, Gb, Gp, map_grad=True, weight_grad=True):
    f = x.to(DEV).requires_grad_(map_grad)
    w, b = W.to(DEV).requires_grad_(weight_grad), c.to(DEV).requires_grad_(weight_grad)
    bank, pooled = T.ImgBankFunction.apply(f, w, b, ops.transpose_pad(w.detach(), ops.IMGBANK_LDW))
    loss = 0.0
    if Gb is not None:
        loss = loss + (bank * Gb.to(DEV)).sum()
    if Gp is not None and pooled.requires_grad:
        loss = loss + (pooled * Gp.to(DEV)).sum()
    loss.backward()
    return f, w, b, bank, pooled


def test_function_gradients_to_map_weight_and_bias():
    x, W, c, Gb, Gp = bank_inputs()
    hw = (6, 6)
    f, w, b, bank, pooled = run_function(x, W, c, Gb, Gp)
    assert pooled.requires_grad and bank.requires_grad
    xd, Wd, cd = x.double().requires_grad_(True), W.double().requires_grad_(True), c.double().requires_grad_(True)
    rb = F.linear(xd.permute(0, 2, 1), Wd, cd)
    rp = F.max_pool2d(xd.view(*x.shape[:2], *hw), hw).view(x.shape[:2])
    ((rb * Gb.double()).sum() + (rp * Gp.double()).sum()).backward()
    close(bank.detach(), rb.detach(), "bank")
    assert torch.equal(pooled.detach().cpu(), rp.detach().float())
    assert f.grad.shape == f.shape and f.grad.dtype == torch.float32
    close(f.grad, xd.grad, "df")
    close(w.grad, Wd.grad, "dW")
    close(b.grad, cd.grad, "db")


def test_function_with_one_consumer_only():
    x, W, c, Gb, Gp = bank_inputs()
    hw = (6, 6)
    f, w, b, _, _ = run_function(x, W, c, None, Gp)                          # the bank is unused: no dbank arrives
    assert torch.equal(f.grad.cpu(), map_grad_ref(x, W, None, Gp, hw).float())
    assert w.grad is None and b.grad is None
    f, w, b, _, _ = run_function(x, W, c, Gb, None)                          # pooled is unused
    close(f.grad, map_grad_ref(x, W, Gb, None, hw), "df bank only")
    assert w.grad is not None and b.grad is not None
    f, w, b, _, _ = run_function(x, W, c, Gb, Gp, weight_grad=False)         # frozen bank, trainable map
    close(f.grad, map_grad_ref(x, W, Gb, Gp, hw), "df frozen bank")
    assert w.grad is None and b.grad is None


class count_calls:
    """Counts the calls of ops.<name> for the length of a with block."""

    def __init__(self, *names):
        self.names, self.calls = names, {n: 0 for n in names}

    def __enter__(self):
        self.real = {n: getattr(ops, n) for n in self.names}
        for n in self.names:
            setattr(ops, n, self._wrap(n))
        return self.calls

    def _wrap(self, n):
        def f(*a, **k):
            self.calls[n] += 1
            return self.real[n](*a, **k)
        return f

    def __exit__(self, *exc):
        for n, fn in self.real.items():
            setattr(ops, n, fn)


def test_function_without_map_gradient_launches_neither_kernel():
    x, W, c, Gb, Gp = bank_inputs()
    with count_calls("map_argmax", "imgbank_dgrad", "imgbank_wgrad") as calls:
        f, w, b, bank, pooled = run_function(x, W, c, Gb, Gp, map_grad=False)
    assert calls == {"map_argmax": 0, "imgbank_dgrad": 0, "imgbank_wgrad": 1}
    assert not pooled.requires_grad and f.grad is None and w.grad is not None
    with count_calls("map_argmax", "imgbank_dgrad", "imgbank_wgrad") as calls:
        run_function(x, W, c, Gb, Gp)
    assert calls == {"map_argmax": 1, "imgbank_dgrad": 1, "imgbank_wgrad": 1}


# ---- the whole model ----------------------------------------------------------------------------------------------------------
def grads_of(model):
    return {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}


def with_map_leaves(args):
    args = list(args)
    for i in (3, 4):
        args[i] = args[i].detach().clone().requires_grad_(True)
    return args


@pytest.mark.parametrize("cfg_name", ["mvsa_single_b8", "tumemo_b64"])
def test_whole_model_map_gradients_match_fp64(cfg_name):
    cfg, model, inp = M.make(cfg_name)
    plain = harness.call_args(inp, DEV)
    torch.manual_seed(1234)
    logits0 = M.train_step(model, plain)
    g0 = grads_of(model)
    args = with_map_leaves(plain)
    torch.manual_seed(1234)
    logits = M.train_step(model, args)
    g1 = grads_of(model)
    # asking for the maps' gradients changes nothing else, bit for bit
    assert torch.equal(logits, logits0) and g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    B, Tn = args[0].shape
    masks = M.collect_masks(model, B, Tn, args[3].shape[2] * args[3].shape[3])
    p = M.ref_params(model)
    ref_inp = dict(inp)
    for name in ("object_feature", "place_feature"):
        ref_inp[name] = torch.as_tensor(inp[name]).double().requires_grad_(True)
        flat = ref_inp[name].detach().reshape(B * 2048, -1)
        assert int((flat == flat.max(dim=1, keepdim=True).values).sum(dim=1).max()) == 1, "tied maxima in the synthetic maps"
    ref = M.model_ref(p, model, M.constants(model, plain), ref_inp, masks)
    ref.sum().backward()
    close(logits, ref.detach(), "logits")
    for i, name in ((3, "object_feature"), (4, "place_feature")):
        got = args[i].grad
        assert got is not None, "%s got no gradient" % name
        assert got.shape == args[i].shape and got.dtype == args[i].dtype
        close(got, ref_inp[name].grad, "d " + name)
    for k, v in model.named_parameters():
        if v.grad is not None:
            close(v.grad, p[k].grad, k)
    assert {k for k, v in p.items() if v.grad is None} == {k for k, v in model.named_parameters() if v.grad is None}


class ChannelTrunk(torch.nn.Module):
    """A stand-in for a CNN trunk's last stage: a per-channel affine map (a 1x1 depthwise convolution) and a ReLU."""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.weight = torch.nn.Parameter(1.0 + 0.1 * torch.randn(2048, generator=g))
        self.bias = torch.nn.Parameter(0.05 * torch.randn(2048, generator=g))

    def forward(self, x):
        return torch.relu(x * self.weight[None, :, None, None] + self.bias[None, :, None, None])


def test_a_trunk_in_front_of_the_model_trains():
    cfg, model, inp = M.make("mvsa_single_b8")
    args = list(harness.call_args(inp, DEV))
    raw = {3: args[3], 4: args[4]}
    trunks = {3: ChannelTrunk(1).to(DEV), 4: ChannelTrunk(2).to(DEV)}
    lr, lrp = 1e-3, 0.1
    opt = torch.optim.Adam(model.get_config_optim(lr, lrp) + [{"params": list(t.parameters()), "lr": lr * lrp} for t in trunks.values()],
                           lr=lr)
    opt.zero_grad(set_to_none=True)
    for i, t in trunks.items():
        args[i] = t(raw[i])
    logits = model(*args)
    logits.sum().backward()
    B, Tn = args[0].shape
    masks = M.collect_masks(model, B, Tn, 196)
    p = M.ref_params(model)
    ref_trunks = {i: ChannelTrunk(i - 2).double() for i in trunks}
    ref_inp = dict(inp)
    for i, name in ((3, "object_feature"), (4, "place_feature")):
        ref_inp[name] = ref_trunks[i](torch.as_tensor(inp[name]).double())
    consts = M.constants(model, harness.call_args(inp, DEV))
    ref = M.model_ref(p, model, consts, ref_inp, masks)
    ref.sum().backward()
    close(logits.detach(), ref.detach(), "logits")
    for i, t in trunks.items():
        assert t.weight.grad is not None, "the trunk got no gradient"
        close(t.weight.grad, ref_trunks[i].weight.grad, "trunk %d weight" % i)
        close(t.bias.grad, ref_trunks[i].bias.grad, "trunk %d bias" % i)
    before = {i: t.weight.detach().clone() for i, t in trunks.items()}
    opt.step()
    for i, t in trunks.items():
        assert not torch.equal(t.weight.detach(), before[i]) and torch.isfinite(t.weight).all()
    model.eval()
    with torch.no_grad():
        for i, t in trunks.items():
            args[i] = t(raw[i])
        out = model(*args)
    assert out.shape == logits.shape and torch.isfinite(out).all()


def test_frozen_banks_still_pass_the_gradient_to_the_maps():
    cfg, model, inp = M.make("mvsa_single_b8")
    args = with_map_leaves(harness.call_args(inp, DEV))
    torch.manual_seed(5)
    M.train_step(model, args)
    want = (args[3].grad.clone(), args[4].grad.clone())
    model.liner_img_object.requires_grad_(False)
    model.liner_img_place.requires_grad_(False)
    args = with_map_leaves(args)
    torch.manual_seed(5)
    with count_calls("imgbank_wgrad", "imgbank_dgrad", "map_argmax") as calls:
        M.train_step(model, args)
    assert calls == {"imgbank_wgrad": 0, "imgbank_dgrad": 2, "map_argmax": 2}
    assert model.liner_img_object.weight.grad is None and model.liner_img_place.bias.grad is None
    assert torch.equal(args[3].grad, want[0]) and torch.equal(args[4].grad, want[1])
