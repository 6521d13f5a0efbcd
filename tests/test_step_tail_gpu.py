"""The training step's tail on the GPU (csrc/step_tail.hip, mgnns_amd/optim.py, train.cross_entropy): the Adam
kernel bit for bit against the numpy restatement of its specification (tests/step_tail_ref.py), the norm and the cross-entropy
within one fp32 ulp of fp64 references, and three whole-model steps against torch's loss, clip and Adam -- where a parameter
version that did not rise would leave the next forward on stale derived packs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mgnns_amd import _lib, ops, optim, synth, train
from tests import model_util as MU
from tests import step_tail_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = optim.CHUNK


def same_bits(got, want):
    """Bit for bit, NaN equal to NaN."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    return got.shape == want.shape and bool(np.all((got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))))


# ---- Adam, bit for bit -------------------------------------------------------------------------------------------------------
def view_at(values, offset):
    """A contiguous fp32 view at storage offset `offset` of a larger device buffer (storage is 16-byte aligned), holding `values`."""
    buf = torch.zeros(len(values) + 8, device=DEV)
    v = buf[offset:offset + len(values)]
    v.copy_(torch.from_numpy(np.asarray(values, np.float32)))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * offset
    return v


class Case:
    """The case list of tests/step_tail_ref.layout as device tensors under an optim.Adam, next to the restatement."""

    def __init__(self, max_norm):
        self.lay = R.layout(CHUNK)
        start = R.initial(self.lay)
        self.ref = R.RefAdam(start, R.groups_of(self.lay), max_norm)
        self.offset = {"view1": 1, "view3": 3}
        self.p = {}
        for name, n, _, kind in self.lay:
            data = view_at(start[name], self.offset[kind]) if kind in self.offset else torch.from_numpy(start[name]).to(DEV)
            self.p[name] = torch.nn.Parameter(data)
            assert self.p[name].data_ptr() == data.data_ptr()
        self.opt = optim.Adam([dict(params=[self.p[k] for k in names], **hyper) for hyper, names in R.groups_of(self.lay)],
                              betas=R.BETAS, eps=R.EPS, max_norm=max_norm)
        # view1 with state that sits in its 16-byte lines as the parameter and its gradient do: the 16-byte path with a head and a
        # tail.  view3 gets the state step() makes, which is aligned: its four runs sit differently, the element-wise path.
        n1 = start["view1"].size
        self.opt.state[self.p["view1"]] = dict(step=torch.tensor(0.0), exp_avg=view_at(np.zeros(n1), 1), exp_avg_sq=view_at(np.zeros(n1), 1))

    def step(self, s, inf_at=None, use_kernel_coef=False):
        g = R.gradients(self.lay, s, inf_at=inf_at)
        for name, n, _, kind in self.lay:                        # fresh gradient tensors every step, as after zero_grad()
            if g[name] is None:
                self.p[name].grad = None
            else:
                self.p[name].grad = view_at(g[name], self.offset[kind]) if kind in self.offset else torch.from_numpy(g[name]).to(DEV)
        before = {k: v._version for k, v in self.p.items()}
        self.opt.step()
        self.ref.step(g, coef=float(self.opt.clip_coef) if use_kernel_coef else None)
        for name, n, _, kind in self.lay:
            moved = kind not in ("empty", "nograd")
            assert (self.p[name]._version > before[name]) == moved, name
            assert same_bits(self.p[name].grad.cpu().numpy(), g[name]) if g[name] is not None else self.p[name].grad is None

    def check(self, s):
        for name, n, _, kind in self.lay:
            p, st = self.p[name], self.opt.state[self.p[name]]
            assert same_bits(p.detach().cpu().numpy(), self.ref.p[name]), "step %d: p of %s" % (s, name)
            if kind in ("empty", "nograd"):
                assert not st, "%s must have no state (its step is unchanged)" % name
                continue
            assert float(st["step"]) == s + 1 == self.ref.step_of[name] and st["step"].device.type == "cpu"
            assert same_bits(st["exp_avg"].cpu().numpy(), self.ref.m[name]), "step %d: exp_avg of %s" % (s, name)
            assert same_bits(st["exp_avg_sq"].cpu().numpy(), self.ref.v[name]), "step %d: exp_avg_sq of %s" % (s, name)


def test_adam_equals_the_restatement_bit_for_bit_without_clipping():
    case = Case(None)
    for s in range(R.STEPS):
        case.step(s)
        case.check(s)
    assert case.opt.total_norm is None and case.opt._uploads >= R.STEPS
    # nothing was left behind in the buffers around the views
    assert R.initial(case.lay)["nograd"].tolist() == case.p["nograd"].detach().cpu().tolist()


def test_adam_with_the_clip_engaged():
    """max_norm below every step's norm: clip_coef < 1.  The norm is within one fp32 ulp of the fp64 reference, the coefficient is
    exactly the fp32 function of the kernel's own norm, and given that coefficient p, m and v are the restatement's bits."""
    max_norm = 0.25 * R.big_norm(R.layout(CHUNK))
    case = Case(max_norm)
    for s in range(R.STEPS):
        case.step(s, use_kernel_coef=True)
        norm, coef = np.float32(float(case.opt.total_norm)), np.float32(float(case.opt.clip_coef))
        assert R.ulps(norm, case.ref.total_norm).max() <= 1, "step %d: total_norm %r vs %r" % (s, norm, case.ref.total_norm)
        # (a norm one ulp off moves the quotient by at most two of its own ulps, and each side rounds it once)
        assert coef == R.coefficient(norm, max_norm) and coef < 1 and R.ulps(coef, case.ref.clip_coef).max() <= 3
        case.check(s)
    assert case.opt.total_norm.device.type == "cuda" and case.opt.total_norm.dim() == 0


def test_adam_with_an_idle_clip_equals_the_unclipped_run():
    max_norm = 1e6 * R.big_norm(R.layout(CHUNK))
    idle, off = Case(max_norm), Case(None)
    for s in range(R.STEPS):
        idle.step(s)
        off.step(s)
        assert float(idle.opt.clip_coef) == 1.0 and idle.ref.clip_coef == 1.0
        idle.check(s)
    for name in idle.p:
        assert same_bits(idle.p[name].detach().cpu().numpy(), off.p[name].detach().cpu().numpy()), name
        for key in ("exp_avg", "exp_avg_sq"):
            if idle.opt.state[idle.p[name]]:
                assert same_bits(idle.opt.state[idle.p[name]][key].cpu().numpy(), off.opt.state[off.p[name]][key].cpu().numpy()), name


def test_adam_with_one_infinite_gradient_entry():
    """Norm inf, coefficient 0: the infinite entry becomes inf * 0 = NaN, every other gradient 0; the pattern is the restatement's."""
    case = Case(10.0)
    for s in range(3):
        case.step(s, inf_at=("t5", 2) if s == 1 else None, use_kernel_coef=(s != 1))
        if s == 1:
            assert float(case.opt.total_norm) == float("inf") == case.ref.total_norm and float(case.opt.clip_coef) == 0.0 == case.ref.clip_coef
        case.check(s)
    got = case.p["t5"].detach().cpu().numpy()
    assert np.isnan(got[2]) and np.isfinite(np.delete(got, 2)).all()
    assert all(np.isfinite(p.detach().cpu().numpy()).all() for k, p in case.p.items() if k != "t5")


def test_parameters_of_one_group_at_different_step_counts():
    """A parameter whose gradient was None for a step has its own bias corrections afterwards (torch keeps `step` per parameter)."""
    a, b = (torch.nn.Parameter(torch.from_numpy(v).to(DEV)) for v in (np.linspace(-1, 1, 9, dtype=np.float32), np.ones(5, np.float32)))
    opt = optim.Adam([a, b], lr=1e-2)
    ref = R.RefAdam({"a": a.detach().cpu().numpy(), "b": b.detach().cpu().numpy()}, [(dict(lr=1e-2, weight_decay=0.0), ["a", "b"])])
    rng = np.random.default_rng(5)
    for s in range(4):
        g = {"a": rng.standard_normal(9).astype(np.float32), "b": None if s == 1 else rng.standard_normal(5).astype(np.float32)}
        a.grad, b.grad = torch.from_numpy(g["a"]).to(DEV), None if g["b"] is None else torch.from_numpy(g["b"]).to(DEV)
        opt.step()
        ref.step(g)
    assert float(opt.state[a]["step"]) == 4 and float(opt.state[b]["step"]) == 3 == ref.step_of["b"]
    assert same_bits(a.detach().cpu().numpy(), ref.p["a"]) and same_bits(b.detach().cpu().numpy(), ref.p["b"])


def test_the_chunk_table_is_uploaded_again_only_when_an_address_moves():
    p = torch.nn.Parameter(torch.zeros(CHUNK + 5, device=DEV))
    opt = optim.Adam([p], max_norm=1.0)
    g1, g2 = torch.ones_like(p), torch.full_like(p, 2.0)
    p.grad = g1
    opt.step()
    n = opt._uploads
    opt.step()
    assert opt._uploads == n + 1, "same addresses: only the scalar rows are uploaded"
    p.grad = g2
    opt.step()
    assert opt._uploads == n + 3, "the gradient moved: the table follows it"
    assert float(opt.total_norm) == pytest.approx(2.0 * (CHUNK + 5) ** 0.5, rel=1e-6)


def test_norm_params_count_in_the_norm_and_do_not_move():
    """What clip_grad_norm_(model.parameters()) does for a parameter outside the optimizer's groups: its gradient is in the norm
    and is multiplied by the coefficient."""
    inside, outside, twice = (torch.nn.Parameter(torch.full((n,), 1.0, device=DEV)) for n in (CHUNK + 3, 2 * CHUNK + 1, 5))
    inside.grad, outside.grad, twice.grad = torch.full_like(inside, 3.0), torch.full_like(outside, 4.0), torch.full_like(twice, 1.0)
    opt = optim.Adam([inside, twice], lr=1e-2, max_norm=1.0, norm_params=[outside, twice, inside])
    ref = R.RefAdam({"inside": np.ones(CHUNK + 3, np.float32), "twice": np.ones(5, np.float32)},
                    [(dict(lr=1e-2, weight_decay=0.0), ["inside", "twice"])], 1.0)
    want_norm, want_coef = R.clip([np.full(CHUNK + 3, 3.0, np.float32), np.full(2 * CHUNK + 1, 4.0, np.float32), np.ones(5, np.float32)], 1.0)
    v0 = outside._version
    opt.step()
    assert R.ulps(np.float32(float(opt.total_norm)), want_norm).max() <= 1 and float(opt.clip_coef) == R.coefficient(float(opt.total_norm), 1.0)
    ref.step({"inside": np.full(CHUNK + 3, 3.0, np.float32), "twice": np.ones(5, np.float32)}, coef=float(opt.clip_coef))
    assert same_bits(inside.detach().cpu().numpy(), ref.p["inside"]) and same_bits(twice.detach().cpu().numpy(), ref.p["twice"])
    scaled = np.float32(4.0) * np.float32(float(opt.clip_coef))          # ... and multiplied by the coefficient in place
    assert (outside == 1).all() and same_bits(outside.grad.cpu().numpy(), np.full(2 * CHUNK + 1, scaled)) and float(opt.clip_coef) < 1
    assert outside._version == v0 and not opt.state[outside] and (inside.grad == 3).all()
    # without max_norm they are not looked at
    optim.Adam([inside], norm_params=[torch.nn.Parameter(torch.zeros(2))]).step()


# ---- the norm ----------------------------------------------------------------------------------------------------------------
def test_total_norm_is_the_fp64_norm_within_one_ulp_and_repeatable():
    rng = np.random.default_rng(9)
    sizes = (1, 3, 5, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 2, 37, CHUNK + 6)
    grads = [R.draw_gradient(n, rng) for n in sizes]
    dev = [torch.from_numpy(g).to(DEV) for g in grads[:-2]] + [view_at(grads[-2], 1), view_at(grads[-1], 3)]
    table_host = optim.chunk_table([(g, g, g, g) for g in dev], [0] * len(dev))
    n = table_host.shape[0]
    assert n == sum(-(-s // CHUNK) for s in sizes)
    table = torch.from_numpy(table_host).to(DEV)
    outs = []
    for _ in range(2):
        partial = torch.full((n + 3,), -1.0, device=DEV, dtype=torch.float64)
        out = torch.full((4,), -1.0, device=DEV)
        ops.grad_sumsq(table, n, partial)
        ops.grad_clip_coef(partial, n, 3.0, out)
        outs.append((partial.cpu().numpy(), out.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    partial, out = outs[0]
    assert (partial[n:] == -1).all() and (out[2:] == -1).all()
    want_partial = [np.sum(g[o:o + CHUNK].astype(np.float64) ** 2) for g in grads for o in range(0, g.size, CHUNK)]
    assert np.allclose(partial[:n], want_partial, rtol=1e-12, atol=0)
    want_norm, want_coef = R.clip(grads, 3.0)
    assert R.ulps(out[0], want_norm).max() <= 1 and out[1] == R.coefficient(out[0], 3.0) and out[1] < 1
    # no chunk at all: norm 0, coefficient 1
    none = torch.full((2,), -1.0, device=DEV)
    ops.grad_clip_coef(torch.zeros(1, device=DEV, dtype=torch.float64), 0, 3.0, none)
    assert none.tolist() == [0.0, 1.0]


# ---- cross-entropy -----------------------------------------------------------------------------------------------------------
def check_ce(x, t, what):
    loss, d = ops.ce_loss(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
    want_loss, want_d = R.cross_entropy(x, t)
    with np.errstate(all="ignore"):
        want_loss, want_d = np.float32(want_loss), want_d.astype(np.float32)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and d.shape == x.shape
    ul, ud = R.ulps(loss.cpu().numpy(), want_loss).max(), R.ulps(d.cpu().numpy(), want_d).max()
    assert ul <= 1 and ud <= 1, "%s: loss %r vs %r (%d ulp), dlogits %d ulp" % (what, float(loss), want_loss, ul, ud)
    return loss, d


@pytest.mark.parametrize("NL", [1, 3, 7, 64])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257])
def test_cross_entropy_is_the_fp64_reference_within_one_ulp(B, NL):
    rng = np.random.default_rng(1000 * B + NL)
    x = rng.standard_normal((B, NL)).astype(np.float32) * 3
    t = rng.integers(0, NL, B)
    loss, d = check_ce(x, t, "plain")
    want = F.cross_entropy(torch.from_numpy(x), torch.from_numpy(t))
    assert float(loss) == pytest.approx(float(want), rel=1e-5, abs=1e-6)
    check_ce((x * (80 / np.abs(x).max())).astype(np.float32), t, "logits of magnitude 80")
    if B > 1:
        ti = t.copy()
        ti[rng.random(B) < 0.4] = R.IGNORE
        ti[0], ti[1] = R.IGNORE, t[1]
        loss, d = check_ce(x, ti, "some targets ignored")
        assert (d[torch.from_numpy(ti == R.IGNORE).to(DEV)] == 0).all() and torch.isfinite(loss)
    loss, d = check_ce(x, np.full(B, R.IGNORE), "every target ignored")
    assert torch.isnan(loss) and (d == 0).all()
    if NL > 1:
        xi = x.copy()
        xi[rng.random(x.shape) < 0.3] = -np.inf
        xi[np.arange(B), t] = x[np.arange(B), t]          # the target's logit stays finite: a finite loss
        loss, _ = check_ce(xi, t, "rows containing -inf")
        assert torch.isfinite(loss)
        xi[B // 2, t[B // 2]] = -np.inf                   # the target's own logit: an infinite loss
        loss, _ = check_ce(xi, t, "a target at -inf")
        assert float(loss) == float("inf")
        xi[0, :] = -np.inf                                # one row all -inf: NaN, as torch gives
        loss, _ = check_ce(xi, t, "a row of -inf")
        assert torch.isnan(loss)


@pytest.mark.parametrize("row", ["middle", "last"])
def test_cross_entropy_with_a_target_equal_to_NL_is_nan_and_writes_nothing_outside_its_row(row):
    B, NL = 6, 3
    rng = np.random.default_rng(4)
    x = rng.standard_normal((B, NL)).astype(np.float32)
    t = rng.integers(0, NL, B)
    bad = {"middle": 2, "last": B - 1}[row]
    t[bad] = NL
    guard = torch.full((B * NL + 16,), 7.0, device=DEV)
    loss = torch.full((3,), 7.0, device=DEV)
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    _lib.call("mgnns_ce_loss_fwd_bwd", xd.data_ptr(), td.data_ptr(), B, NL, loss.data_ptr() + 4, guard.data_ptr() + 32, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, l = guard.cpu().numpy(), loss.cpu().numpy()
    assert (got[:8] == 7).all() and (got[8 + B * NL:] == 7).all() and l[0] == 7 and l[2] == 7 and np.isnan(l[1])
    d = got[8:8 + B * NL].reshape(B, NL)
    _, want = R.cross_entropy(x, t)
    assert np.isnan(d[bad]).all() and R.ulps(np.delete(d, bad, 0), np.delete(want, bad, 0).astype(np.float32)).max() <= 1
    loss, d2 = check_ce(x, t, "target == NL")
    assert torch.isnan(loss)
    with pytest.raises(ValueError, match="NL"):
        ops.ce_loss(torch.zeros(2, 65, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))


def test_train_cross_entropy_backward_scales_dlogits_by_the_upstream_gradient():
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((8, 3)).astype(np.float32)).to(DEV)
    t = torch.from_numpy(rng.integers(0, 3, 8)).to(DEV)
    logits = x.clone().requires_grad_(True)
    loss = train.cross_entropy(logits, t)
    assert loss.dim() == 0 and loss.requires_grad
    (loss * 3.0).backward()
    want_loss, d = ops.ce_loss(x, t)
    assert torch.equal(loss.detach(), want_loss) and torch.equal(logits.grad, d * 3.0)
    ref = x.clone().requires_grad_(True)
    (F.cross_entropy(ref, t) * 3.0).backward()
    assert loss.item() == pytest.approx(F.cross_entropy(x, t).item(), rel=1e-6)
    assert (logits.grad - ref.grad).abs().max() <= 1e-6


# ---- the whole model, and the version trap -------------------------------------------------------------------------------------
STEPS = 3


def make_model(seed=7):
    """mvsa_single_b8 from the seeded harness, every dropout rate 0 -- the construction of tests/test_model_train_gpu.make."""
    cfg = synth.CONFIGS["mvsa_single_b8"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = MU.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=cfg.B, seed=seed, pmi=pmi)
    model = MU.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    args = MU.call_args(inp, DEV)
    target = torch.from_numpy(np.random.default_rng(seed).integers(0, cfg.NL, args[0].shape[0])).to(DEV)
    return model, args, target


def evaluate(model, args, precision="fp32"):
    model.eval()
    model.set_precision(precision)
    with torch.no_grad():
        out = model(*args).float().clone()
    model.set_precision("fp32")
    return out


def to_training(model):
    model.train()
    model.freeze_text_encoders()
    return model


def run(which, bf16_runs=0):
    """STEPS training steps of one model -> (training logits per step, fp32 eval logits before, after each step, bf16 eval logits
    after each step (bf16_runs of them), the model).  which = 'hip': train.cross_entropy and optim.Adam(max_norm=10); 'torch':
    F.cross_entropy, clip_grad_norm_(model.parameters(), 10) and torch.optim.Adam."""
    model, args, target = make_model()
    before = evaluate(model, args)
    groups = model.get_config_optim(1e-3, 0.1)
    # (norm_params: clip_grad_norm_ below counts and scales every parameter of the model, the head outside the groups included,
    # whose gradients opt.zero_grad() never clears)
    opt = optim.Adam(groups, max_norm=10, norm_params=model.parameters()) if which == "hip" else torch.optim.Adam(groups)
    train_logits, after, after_bf16 = [], [], []
    for s in range(STEPS):
        to_training(model)
        logits = model(*args)
        loss = train.cross_entropy(logits, target) if which == "hip" else F.cross_entropy(logits, target)
        opt.zero_grad()
        loss.backward()
        if which == "torch":
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10)
        opt.step()
        train_logits.append(logits.detach().clone())
        after.append(evaluate(model, args))
        after_bf16.append([evaluate(model, args, "bf16") for _ in range(bf16_runs)])
    return train_logits, before, after, after_bf16, model, opt


def gate(got, ref, what, tol=1e-4):
    """The project's logit gate: 1e-4 of the reference's largest magnitude."""
    err, scale = float((got.double() - ref.double()).abs().max()), float(ref.double().abs().max())
    assert np.isfinite(err) and err <= tol * scale + 1e-12, "%s: max err %.3e vs max |ref| %.3e" % (what, err, scale)


@pytest.fixture(scope="module")
def runs():
    torch.manual_seed(0)
    return run("hip", bf16_runs=1), run("torch", bf16_runs=2)


def test_three_steps_of_the_whole_model_match_torch_s_tail(runs):
    (a_train, a_before, a_after, _, model_a, opt), (b_train, b_before, b_after, _, model_b, _) = runs
    assert torch.equal(a_before, b_before)
    for s in range(STEPS):
        gate(a_train[s], b_train[s], "training logits of step %d" % s)
        gate(a_after[s], b_after[s], "eval logits after step %d" % s)
    # the optimizer moved the weights, and every forward since saw the moved weights: with a version that did not rise the derived
    # packs (mgnns_amd/derived.py) would be stale and the eval logits those of the initial weights
    shift = float((a_after[0] - a_before).abs().max())
    assert shift > 1e-3 * float(a_before.abs().max()), "eval logits did not move after a step (%.3e): stale derived packs?" % shift
    assert float((a_after[-1] - a_after[0]).abs().max()) > 0
    stepped = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    assert len(stepped) > 20 and all(p._version >= STEPS for p in stepped)
    start = make_model()[0].state_dict()
    names = [k for k, p in model_a.named_parameters() if any(p is q for q in stepped)]
    moved = [k for k in names if not torch.equal(model_a.state_dict()[k], start[k])]
    assert len(moved) >= 0.9 * len(names), "only %d of %d stepped parameters moved" % (len(moved), len(names))
    assert float(opt.total_norm) > 0 and 0 < float(opt.clip_coef) <= 1
    # three steps on one batch bring its loss down
    target = make_model()[2]
    assert float(F.cross_entropy(a_after[-1], target)) < float(F.cross_entropy(a_before, target))


def test_three_steps_in_bf16_precision_mode(runs):
    """The bf16 forward after every step, its packs rebuilt from the moved fp32 weights on both sides.  Bound: the largest |dlogit|
    that the two bf16 runs of the torch-tail model show against that model in fp32, measured here."""
    (_, _, a_after, a_bf16, _, _), (_, _, b_after, b_bf16, _, _) = runs
    bound = max(float((r - b_after[s]).abs().max()) for s in range(STEPS) for r in b_bf16[s])
    worst = max(float((a_bf16[s][0] - b_bf16[s][0]).abs().max()) for s in range(STEPS))
    print("bf16 mode: hip tail vs torch tail %.3e, bound (bf16 vs fp32 of the torch-tail model) %.3e" % (worst, bound))
    assert bound > 0 and worst <= bound
    for s in range(1, STEPS):
        assert not torch.equal(a_bf16[s][0], a_bf16[s - 1][0]), "the bf16 packs did not follow the weights of step %d" % s
