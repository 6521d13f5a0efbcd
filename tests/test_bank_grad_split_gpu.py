"""The image banks' training products on the bf16 matrix pipe (csrc/bank_grad_split.hip, set_train_bank_precision('bf16x3')):
split-bf16 weight and map gradients against fp64 on the CPU, at the training gate (1e-4 of the reference tensor's largest
magnitude, tests/test_model_train_gpu.py::close) -- a correct three-term kernel errs by ~5e-6, one that drops a term by ~3e-3."""
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import _lib, harness, ops
from mgnns_amd import train as T
from tests import test_map_grad_gpu as G
from tests import test_model_train_gpu as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
close = M.close


@pytest.fixture(autouse=True)
def _rng_state_as_found():
    with torch.random.fork_rng(devices=[0]):
        yield


# ---- the weight gradient -----------------------------------------------------------------------------------------------------
WGRAD_SHAPES = [
    (1, 16, 1, 1),
    (3, 200, 49, 37),
    (9, 16, 5, 8),
    (5, 130, 17, 304),
    (2, 144, 208, 320),
    (2, 72, 250, 24),
    (2, 2048, 196, 300),         # the product shape
    (40, 16, 196, 8),            # a long reduction over few channels: many slabs
]


def test_the_wgrad_shapes_cover_the_direct_write_and_the_combine():
    """One slab writes dW itself and needs no workspace (64 bytes); several write partials that one ordered launch adds."""
    sizes = [_lib.lib().mgnns_imgbank_wgrad_split_workspace_bytes(*s) for s in WGRAD_SHAPES]
    assert any(n == 64 for n in sizes), "no one-slab shape"
    assert any(n > 64 for n in sizes), "no shape that takes the combine launch"
    B, K, P, N = WGRAD_SHAPES[-1]
    assert sizes[-1] >= 4 * 8 * N * (K + 1), "the long reduction does not run as many slabs"


@pytest.mark.parametrize("B,K,P,N", WGRAD_SHAPES)
def test_wgrad_split_matches_fp64(B, K, P, N):
    g = torch.Generator().manual_seed(B * 1000 + P)
    X = torch.relu(torch.randn(B, K, P, generator=g))
    dbank = torch.randn(B, P, N, generator=g)
    Xg, dg = X.to(DEV), dbank.to(DEV)
    dW, db = ops.imgbank_wgrad(Xg, dg, split=True)
    assert dW.shape == (N, K) and db.shape == (N,)
    refW = torch.einsum("bpo,bkp->ok", dbank.double(), X.double())
    refb = dbank.double().sum(dim=(0, 1))
    print("wgrad split %s: dW err %.3e of %.3e, db err %.3e of %.3e"
          % ((B, K, P, N), float((dW.double().cpu() - refW).abs().max()), float(refW.abs().max()),
             float((db.double().cpu() - refb).abs().max()), float(refb.abs().max())))
    close(dW, refW, "dW")
    close(db, refb, "db")
    dW2, db2 = ops.imgbank_wgrad(Xg, dg, split=True)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


def test_wgrad_split_empty_batch_and_refusals():
    dW, db = ops.imgbank_wgrad(torch.zeros(0, 8, 4, device=DEV), torch.zeros(0, 4, 12, device=DEV), split=True)
    assert dW.shape == (12, 8) and db.shape == (12,)
    assert not dW.any() and not db.any()
    ops.imgbank_wgrad(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 4, 320, device=DEV), split=True)
    with pytest.raises(RuntimeError, match="N <= 320"):
        ops.imgbank_wgrad(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 4, 321, device=DEV), split=True)
    with pytest.raises(ValueError):
        ops.imgbank_wgrad(torch.zeros(2, 8, 4, device=DEV), torch.zeros(2, 5, 16, device=DEV), split=True)      # P mismatch
    with pytest.raises(ValueError):
        ops.imgbank_wgrad(torch.zeros(2, 8, 4, device=DEV), torch.zeros(3, 4, 16, device=DEV), split=True)      # B mismatch


# ---- the map gradient: the dense part ---------------------------------------------------------------------------------------
DGRAD_SHAPES = [(3, 200, 49, 37), (2, 2048, 196, 300), (1, 16, 1, 1), (2, 144, 208, 320), (5, 130, 17, 304), (2, 72, 250, 24),
                (9, 16, 5, 8)]          # (those of tests/test_map_grad_gpu.py::test_dense_part_matches_fp64)


@pytest.mark.parametrize("B,K,P,N", DGRAD_SHAPES)
def test_dgrad_split_dense_part_matches_fp64(B, K, P, N):
    g = torch.Generator().manual_seed(B * 1000 + P)
    dbank = torch.randn(B, P, N, generator=g)
    W = torch.randn(N, K, generator=g)
    ref = torch.einsum("ok,bpo->bkp", W.double(), dbank.double())
    out = torch.full((B, K, P), float("nan"), device=DEV)
    got = ops.imgbank_dgrad(dbank.to(DEV), W.to(DEV), out=out, split=True)
    assert got.data_ptr() == out.data_ptr()
    assert not torch.isnan(out).any(), "elements of dX left unwritten"
    print("dgrad split %s: dX err %.3e of %.3e" % ((B, K, P, N), float((out.double().cpu() - ref).abs().max()), float(ref.abs().max())))
    close(out, ref, "dX")
    again = ops.imgbank_dgrad(dbank.to(DEV), W.to(DEV), split=True)
    assert again.shape == (B, K, P) and torch.equal(again, out)


# ---- the map gradient: pooled term and scatter -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,hw,N", [(2, 64, (7, 7), 300), (3, 130, (14, 14), 37)])
def test_dgrad_split_scatter_goes_to_the_first_maximum(B, K, hw, N):
    P = hw[0] * hw[1]
    g = torch.Generator().manual_seed(11)
    x = G.tied_map(B, K, P, seed=P + 1)
    W, dbank, dpooled = torch.randn(N, K, generator=g), torch.randn(B, P, N, generator=g), torch.randn(B, K, generator=g)
    xg, Wg, dbg, dpg = (t.to(DEV) for t in (x, W, dbank, dpooled))
    arg = ops.map_argmax(xg)
    assert torch.equal(arg.cpu(), G.host_argmax(x))
    both = ops.imgbank_dgrad(dbg, Wg, dpg, arg, split=True)
    close(both, G.map_grad_ref(x, W, dbank, dpooled, hw), "dX")
    dense = ops.imgbank_dgrad(dbg, Wg, split=True)
    close(dense, G.map_grad_ref(x, W, dbank, None, hw), "dX bank only")
    # without dbank there is no product: today's kernel, bit for bit
    pooled = ops.imgbank_dgrad(None, Wg, dpg, arg, positions=P, split=True)
    assert torch.equal(pooled, ops.imgbank_dgrad(None, Wg, dpg, arg, positions=P, split=False))
    # the scattered element lands at host_argmax's position: the sum is the dense part plus one addition per row
    assert torch.equal(both, dense + pooled)
    where = (both != dense).cpu()
    hit = torch.zeros(B, K, P, dtype=torch.bool).scatter_(2, G.host_argmax(x).long().unsqueeze(2), True)
    assert not (where & ~hit).any(), "a pooled gradient landed off the first maximum"
    assert torch.equal(ops.imgbank_dgrad(dbg, Wg, dpg, arg, split=True), both)


def test_dgrad_split_refusals_and_empty_batch():
    W = torch.zeros(320, 16, device=DEV)
    assert ops.imgbank_dgrad(torch.zeros(0, 4, 320, device=DEV), W, split=True).shape == (0, 16, 4)
    with pytest.raises(RuntimeError, match="N <= 320"):
        ops.imgbank_dgrad(torch.zeros(2, 4, 321, device=DEV), torch.zeros(321, 16, device=DEV), split=True)
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(torch.zeros(2, 4, 300, device=DEV), W, split=True)                       # N mismatch
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(torch.zeros(2, 4, 320, device=DEV), W, dpooled=torch.zeros(2, 16, device=DEV), split=True)     # no arg
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(torch.zeros(2, 4, 320, device=DEV), W, torch.zeros(3, 16, device=DEV),
                          torch.zeros(3, 16, device=DEV, dtype=torch.int32), split=True)           # B mismatch
    with pytest.raises(ValueError):
        ops.imgbank_dgrad(None, W, split=True)


# ---- ImgBankFunction in split mode --------------------------------------------------------------------------------------------
def run_split_function(x, W, c, Gb, Gp, map_grad=True, weight_grad=True):
    f = x.to(DEV).requires_grad_(map_grad)
    w, b = W.to(DEV).requires_grad_(weight_grad), c.to(DEV).requires_grad_(weight_grad)
    fits = T.split_forward_fits(x.shape[1], x.shape[2], W.shape[0])
    bank, pooled = T.ImgBankFunction.apply(f, w, b, None if fits else ops.transpose_pad(w.detach(), ops.IMGBANK_LDW), 'bf16x3',
                                           ops.pack_weight_bf16_split(w.detach().contiguous()) if fits else None)
    loss = (bank * Gb.to(DEV)).sum()
    if pooled.requires_grad:
        loss = loss + (pooled * Gp.to(DEV)).sum()
    loss.backward()
    return f, w, b, bank, pooled


@pytest.mark.parametrize("K,hw,split_forward", [(128, (6, 6), True), (208, (7, 8), False)])
def test_function_in_split_mode(K, hw, split_forward):
    """Inside the split forward's limits, and outside them (the fp32 forward with the split backward).  The second case is
    K = 208, P = 56: the fp32 forward kernel itself takes only K % 16 == 0 and P % 4 == 0, so K = 200, P = 49 has no forward in
    either mode (mgnns_imgbank_pool_fwd refuses it); the split gradients at K = 200, P = 49 are tested above on their own."""
    N = 300
    assert T.split_forward_fits(K, hw[0] * hw[1], N) == split_forward
    x, W, c, Gb, Gp = G.bank_inputs(B=3, K=K, hw=hw, N=N)
    with G.count_calls("imgbank_pool_split", "imgbank_pool") as fwd:
        f, w, b, bank, pooled = run_split_function(x, W, c, Gb, Gp)
    assert fwd == {"imgbank_pool_split": int(split_forward), "imgbank_pool": int(not split_forward)}
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


def test_function_in_split_mode_without_map_gradient_launches_neither_kernel():
    x, W, c, Gb, Gp = G.bank_inputs(B=3, K=128, hw=(6, 6), N=300)
    with G.count_calls("map_argmax", "imgbank_dgrad", "imgbank_wgrad") as calls:
        f, w, b, bank, pooled = run_split_function(x, W, c, Gb, Gp, map_grad=False)
    assert calls == {"map_argmax": 0, "imgbank_dgrad": 0, "imgbank_wgrad": 1}
    assert not pooled.requires_grad and f.grad is None and w.grad is not None
    with G.count_calls("map_argmax", "imgbank_dgrad", "imgbank_wgrad") as calls:
        run_split_function(x, W, c, Gb, Gp)
    assert calls == {"map_argmax": 1, "imgbank_dgrad": 1, "imgbank_wgrad": 1}
    with G.count_calls("map_argmax", "imgbank_dgrad", "imgbank_wgrad") as calls:
        f, w, b, _, _ = run_split_function(x, W, c, Gb, Gp, weight_grad=False)                # frozen bank: no wgrad
    assert calls == {"map_argmax": 1, "imgbank_dgrad": 1, "imgbank_wgrad": 0}
    assert w.grad is None and b.grad is None and f.grad is not None


# ---- the whole model ----------------------------------------------------------------------------------------------------------
def step_with_map_leaves(model, plain, seed=1234):
    args = G.with_map_leaves(plain)
    torch.manual_seed(seed)
    logits = M.train_step(model, args)
    return args, logits, G.grads_of(model)


@pytest.mark.parametrize("cfg_name", ["mvsa_single_b8", "tumemo_b64"])
def test_whole_model_in_split_mode_matches_fp64(cfg_name):
    """The mode as the model runs it: both gradients of each bank split, the bank's forward fp32.  (With the forward split as
    well -- model.train_bank_split_forward -- the bank's ~5e-6 error is amplified by the fusion attention's backward: measured
    at mvsa_single_b8, text_img_place_multi_head_att.0.slf_attn.w_ks.weight errs by 1.4e-4 of its largest magnitude and
    liner_img_place.weight by 9e-5, against 1e-5 and 2e-6 with the fp32 forward: past this gate, so it is not the default.)"""
    cfg, model, inp = M.make(cfg_name)
    assert not model.train_bank_split_forward
    plain = harness.call_args(inp, DEV)
    args_f, logits_f, g_f = step_with_map_leaves(model, plain)         # never switched
    assert model.set_train_bank_precision('bf16x3') is model
    with G.count_calls("imgbank_wgrad", "imgbank_dgrad") as calls:
        args, logits, g1 = step_with_map_leaves(model, plain)
    assert calls == {"imgbank_wgrad": 2, "imgbank_dgrad": 2}
    B, Tn = args[0].shape
    masks = M.collect_masks(model, B, Tn, args[3].shape[2] * args[3].shape[3])
    p = M.ref_params(model)
    ref_inp = dict(inp)
    for name in ("object_feature", "place_feature"):
        ref_inp[name] = torch.as_tensor(inp[name]).double().requires_grad_(True)
    ref = M.model_ref(p, model, M.constants(model, plain), ref_inp, masks)
    ref.sum().backward()
    close(logits, ref.detach(), "logits")
    for i, name in ((3, "object_feature"), (4, "place_feature")):
        got = args[i].grad
        assert got is not None and got.shape == args[i].shape and got.dtype == args[i].dtype
        close(got, ref_inp[name].grad, "d " + name)
    for k, v in model.named_parameters():
        if v.grad is not None:
            close(v.grad, p[k].grad, k)
    assert {k for k, v in p.items() if v.grad is None} == {k for k, v in model.named_parameters() if v.grad is None}
    # two steps from one seed are bit-equal
    args2, logits2, g2 = step_with_map_leaves(model, plain)
    assert torch.equal(logits, logits2) and g1.keys() == g2.keys()
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for i in (3, 4):
        assert torch.equal(args[i].grad, args2[i].grad)
    # back in fp32 the step is the one of a model that was never switched
    model.set_train_bank_precision('fp32')
    args3, logits3, g3 = step_with_map_leaves(model, plain)
    assert torch.equal(logits3, logits_f) and g3.keys() == g_f.keys()
    for k in g3:
        assert torch.equal(g3[k], g_f[k]), k
    for i in (3, 4):
        assert torch.equal(args3[i].grad, args_f[i].grad)


def test_eval_is_untouched_by_the_training_switch():
    cfg, model, inp = M.make("mvsa_single_b8")
    args = harness.call_args(inp, DEV)
    model.eval()
    with torch.no_grad():
        before = model(*args).clone()
        model.set_train_bank_precision('bf16x3')
        after = model(*args)
    assert torch.equal(before, after)
