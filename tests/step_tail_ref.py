"""Not a test: the specification of the training step's tail (csrc/step_tail.hip, mgnns_amd/optim.py)
restated in numpy, and the cases the CPU and GPU tests share.

Adam: fp32 arrays, scalar constants cast to np.float32, one rounding per operation in exactly the order of the kernel's
adam_element.  The clip coefficient from an fp64 sum of squares.  The cross-entropy in fp64."""
import numpy as np

IGNORE = -100
BETAS, EPS = (0.9, 0.999), 1e-8
# three groups with different lr, one of them with weight decay
GROUPS = (dict(lr=1e-3, weight_decay=0.0), dict(lr=1e-2, weight_decay=1e-4), dict(lr=1e-4, weight_decay=0.0))
STEPS = 5


def group_scalars(lr, b1, b2, eps, wd, step, dtype=np.float32):
    """[-(lr / bc1), sqrt(bc2), 1 - b1, b2, 1 - b2, eps, wd] from Python doubles, as torch's _single_tensor_adam computes them."""
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    return [dtype(x) for x in (-(lr / bc1), bc2 ** 0.5, 1 - b1, b2, 1 - b2, eps, wd)]


def adam_update(p, g, m, v, scalars, coef):
    """-> (p, m, v) after one update; arrays and scalars of one dtype (np.float32: the specification; np.float64: the yardstick)."""
    neg_step, sqrt_bc2, omb1, b2, omb2, eps, wd = scalars
    with np.errstate(all="ignore"):
        g = g * coef
        if wd != 0:
            g = g + wd * p
        m = m + (g - m) * omb1
        v = v * b2 + (omb2 * g) * g
        denom = np.sqrt(v) / sqrt_bc2 + eps
        p = p + neg_step * (m / denom)
    return p, m, v


def sumsq64(grads):
    """The fp64 sum of the squares of fp32 gradients (each square is exact in fp64)."""
    return float(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in grads))


def coefficient(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in fp32, as clip_grad_norm_ computes it from its fp32 norm; NaN stays NaN (torch.clamp)."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > 1 else c


def clip(grads, max_norm):
    """-> (total_norm, clip_coef) as np.float32: the norm rounded once from the fp64 sum of squares."""
    with np.errstate(all="ignore"):
        norm = np.float32(np.sqrt(sumsq64(grads)))
    return norm, coefficient(norm, max_norm)


class RefAdam:
    """The optimizer over {name: array}: groups = [(hyperparameters, [names])].  dtype np.float32 is the specification, np.float64
    the same formula with nothing rounded to fp32 (the clip coefficient included)."""

    def __init__(self, params, groups, max_norm=None, dtype=np.float32):
        self.dtype, self.groups, self.max_norm = dtype, groups, max_norm
        self.p = {k: np.array(v, dtype) for k, v in params.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.step_of = {k: 0 for k in self.p}
        self.total_norm = self.clip_coef = None

    def step(self, grads, coef=None):
        """grads: {name: fp32 array}; a name that is missing or None has no gradient and does not move.  coef: the clip coefficient
        to use instead of this object's own (a kernel's, whose norm may differ from the reference's in its last fp32 bit)."""
        live = [k for _, names in self.groups for k in names if grads.get(k) is not None and self.p[k].size]
        if coef is not None:
            self.total_norm, self.clip_coef = clip([grads[k] for k in live], self.max_norm)
            coef = self.dtype(coef)
        elif self.max_norm is None:
            coef = self.dtype(1.0)
        else:
            if self.dtype is np.float32:
                self.total_norm, self.clip_coef = clip([grads[k] for k in live], self.max_norm)
                coef = self.clip_coef
            else:
                with np.errstate(all="ignore"):
                    norm = np.sqrt(sumsq64([grads[k] for k in live]))
                    coef = min(1.0, self.max_norm / (norm + 1e-6))
        for hyper, names in self.groups:
            for k in names:
                if k not in live:
                    continue
                self.step_of[k] += 1
                s = group_scalars(hyper["lr"], BETAS[0], BETAS[1], EPS, hyper["weight_decay"], self.step_of[k], self.dtype)
                self.p[k], self.m[k], self.v[k] = adam_update(self.p[k], np.asarray(grads[k], self.dtype), self.m[k], self.v[k], s, coef)


# ---- the case list ---------------------------------------------------------------------------------------------------------
def layout(chunk):
    """[(name, elements, group, kind)]: every size around the chunk in one step; an empty tensor and one without gradient, which
    must stay as they are; two contiguous views at storage offsets 1 and 3 of larger buffers (misaligned head and tail)."""
    sizes = (1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3)
    out = [("t%d" % n, n, i % 3, "plain") for i, n in enumerate(sizes)]
    return out + [("empty", 0, 0, "empty"), ("nograd", 7, 1, "nograd"), ("view1", 37, 2, "view1"), ("view3", chunk + 6, 0, "view3")]


def groups_of(lay):
    return [(GROUPS[g], [name for name, _, gg, _ in lay if gg == g]) for g in range(len(GROUPS))]


def initial(lay, seed=11):
    rng = np.random.default_rng(seed)
    return {name: rng.standard_normal(n).astype(np.float32) for name, n, _, _ in lay}


def draw_gradient(n, rng):
    """Magnitudes from 1e-20 to 1e2 (g * g goes denormal and to zero at the small end), random signs, about 5 % exact zeros."""
    g = (10.0 ** rng.uniform(-20, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0.0
    return g


def gradients(lay, step, seed=23, inf_at=None):
    """{name: gradient of this step}; None for the tensor without gradient.  inf_at = (name, index): one entry is +inf."""
    rng = np.random.default_rng(seed * 1000 + step)
    out = {name: (None if kind == "nograd" else draw_gradient(n, rng)) for name, n, _, kind in lay}
    if inf_at is not None:
        out[inf_at[0]][inf_at[1]] = np.inf
    return out


def big_norm(lay, steps=STEPS):
    """The largest total norm any step of the case list has (fp64): for choosing max_norm below or far above it."""
    worst = 0.0
    for s in range(steps):
        worst = max(worst, sumsq64([g for g in gradients(lay, s).values() if g is not None]) ** 0.5)
    return worst


# ---- cross-entropy ---------------------------------------------------------------------------------------------------------
def cross_entropy(logits, target):
    """-> (loss, dlogits [B, NL]) in fp64: mean over the rows whose target is not -100 of -log softmax(row)[target]; dlogits =
    (softmax - onehot) / n_live, a zero row for an ignored sample.  Any other target outside [0, NL): NaN loss, NaN row."""
    x = np.asarray(logits, np.float64)
    B, NL = x.shape
    t = np.asarray(target, np.int64)
    live = t != IGNORE
    bad = live & ((t < 0) | (t >= NL))
    n_live = float(live.sum())
    d = np.zeros_like(x)
    total = 0.0
    with np.errstate(all="ignore"):
        for b in range(B):
            if not live[b]:
                continue
            if bad[b]:
                d[b] = np.nan
                continue
            mx = np.max(x[b])
            e = np.exp(x[b] - mx)
            s = np.sum(e)
            total -= (x[b, t[b]] - mx) - np.log(s)
            onehot = np.zeros(NL)
            onehot[t[b]] = 1.0
            d[b] = (e / s - onehot) / n_live
        loss = np.nan if bad.any() else np.float64(total) / n_live
    return loss, d


def ulps(got, want):
    """Elementwise distance in fp32 ulps between two fp32 arrays; 0 where both are NaN or the same infinity, huge where one is."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)

    def key(a):
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(key(got) - key(want))
    both_nan = np.isnan(got) & np.isnan(want)
    one_nan = np.isnan(got) != np.isnan(want)
    return np.where(both_nan, 0, np.where(one_nan, 2 ** 40, d))
