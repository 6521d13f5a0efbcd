"""Adam with the gradient-norm clip in front of it, as three HIP launches over one table of chunks (csrc/step_tail.hip; DESIGN.md
section 18): what `torch.nn.utils.clip_grad_norm_(params, max_norm)` followed by `torch.optim.Adam(...).step()` do in the
reference's training loop.

The optimizer is a torch.optim.Optimizer: param_groups, zero_grad, state_dict, load_state_dict and add_param_group are torch's,
and the state uses torch's keys and types ('step' a 0-d tensor on the host, 'exp_avg', 'exp_avg_sq'), so a state_dict loads into
torch.optim.Adam and back.  It keeps no copy of the weights: the kernels write the parameters, which stay ordinary nn.Parameters,
in place, and step() then bumps their versions so that every derived pack (mgnns_amd/derived.py) is rebuilt from the moved weights.
"""
import numpy as np
import torch

from . import ops

CHUNK = ops.STEP_CHUNK
_REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable")
_PINNED_SLOTS = 4          # host buffers an upload is staged in, in turn; a slot is reused after its own upload has completed


def chunk_table(tensors, rows, chunk=CHUNK):
    """The chunk table of a step, on the host: int64 [n_chunks, ops.STEP_CHUNK_WORDS] with the addresses of each run in p, g, m and v
    and n | row << 32 (the record of include/mgnns_step.h).  tensors: a list of (p, g, m, v) tensors of equal element counts, fp32
    and contiguous; rows: the scalar row of each, or -1 for a tensor whose gradient only counts in the norm (the Adam kernel scales
    it in place and updates nothing).  A tensor of n elements is ceil(n / chunk) consecutive runs of at most `chunk` elements; an empty tensor gives none."""
    ptr = np.array([[t.data_ptr() for t in four] for four in tensors], dtype=np.int64).reshape(-1, 4)
    numel = np.array([four[0].numel() for four in tensors], dtype=np.int64)
    return chunk_table_from_addresses(ptr, numel, np.asarray(rows, dtype=np.int64), chunk)


def chunk_table_from_addresses(ptr, numel, rows, chunk=CHUNK):
    """chunk_table from ptr int64 [T, 4] (byte addresses, multiples of 4), numel int64 [T] and rows int64 [T]."""
    if ptr.shape != (len(numel), 4) or len(rows) != len(numel):
        raise ValueError("chunk table: %s addresses, %d counts, %d rows" % (ptr.shape, len(numel), len(rows)))
    if (ptr & 3).any() or (numel < 0).any() or (rows < -1).any() or (rows >= 2 ** 31).any():
        raise ValueError("chunk table: an address that is no multiple of 4, a negative count or a row outside -1 .. 2^31 - 1")
    per = (numel + chunk - 1) // chunk                                  # runs per tensor
    which = np.repeat(np.arange(len(numel)), per)                       # the tensor of each run
    first = np.repeat(np.cumsum(per) - per, per)
    off = (np.arange(which.size, dtype=np.int64) - first) * chunk       # the run's first element
    table = np.empty((which.size, ops.STEP_CHUNK_WORDS), dtype=np.int64)
    table[:, :4] = ptr[which] + 4 * off[:, None]
    table[:, 4] = np.minimum(chunk, numel[which] - off) | (rows[which] << 32)
    return table


def group_scalars(lr, beta1, beta2, eps, weight_decay, step):
    """One row of the scalar table, computed in Python doubles as torch's _single_tensor_adam computes them:
    [-(lr / bc1), sqrt(bc2), 1 - b1, b2, 1 - b2, eps, wd, 0] with bc = 1 - beta ** step; the kernel reads them as fp32."""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return [-(lr / bc1), bc2 ** 0.5, 1 - beta1, beta2, 1 - beta2, eps, weight_decay, 0.0]


def check_hyperparameters(group):
    """ValueError, by name, for a switch of torch.optim.Adam that this optimizer does not have, or a value outside torch's range."""
    for flag in _REFUSED_FLAGS:
        if group.get(flag):
            raise ValueError("mgnns_amd.optim.Adam does not support %s=True" % flag)
    if group.get("fused") or group.get("decoupled_weight_decay"):
        raise ValueError("mgnns_amd.optim.Adam does not support fused=True or decoupled_weight_decay=True")
    lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
    if torch.is_tensor(lr) or torch.is_tensor(b1) or torch.is_tensor(b2):
        raise ValueError("mgnns_amd.optim.Adam takes lr and betas as Python numbers, not tensors")
    if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0 or not 0.0 <= wd:
        raise ValueError("invalid lr=%r, betas=%r, eps=%r or weight_decay=%r" % (lr, (b1, b2), eps, wd))


def check_tensors(p, g, device=None):
    """ValueError, by name, for a parameter / gradient pair the kernels do not take.  Reads no data: works on CPU tensors too (where
    the last check, the device, is the one that fires)."""
    if g.is_sparse or g.layout != torch.strided:
        raise ValueError("mgnns_amd.optim.Adam does not support sparse gradients")
    if p.dtype != torch.float32 or g.dtype != torch.float32:
        raise ValueError("mgnns_amd.optim.Adam takes fp32 parameters and gradients (non-fp32: %s, %s)" % (p.dtype, g.dtype))
    if not p.is_contiguous() or not g.is_contiguous():
        raise ValueError("mgnns_amd.optim.Adam takes contiguous parameters and gradients (non-contiguous: shape %s, strides %s / %s)"
                         % (tuple(p.shape), p.stride(), g.stride()))
    if g.shape != p.shape:
        raise ValueError("gradient of shape %s for a parameter of shape %s" % (tuple(g.shape), tuple(p.shape)))
    if not p.is_cuda or g.device != p.device or (device is not None and p.device != device):
        raise ValueError("mgnns_amd.optim.Adam runs on the GPU: parameters not on the GPU, or not all on one device (%s, gradient on %s)"
                         % (p.device, g.device))


def _check_state(p, m, v):
    for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape or t.device != p.device:
            raise ValueError("optimizer state %s must be a contiguous fp32 tensor like its parameter (shape %s on %s)"
                             % (name, tuple(p.shape), p.device))


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's update (the plain path: no amsgrad, maximize, capturable, differentiable) as one fused HIP pass, with
    `clip_grad_norm_(params, max_norm)` over the optimizer's own parameters folded in front of it when max_norm is given.

    The update is specified operation by operation (tests/step_tail_ref.py restates it):
        g = g * clip_coef;  g += wd * p (wd != 0);  m += (g - m) * (1 - b1);  v = v * b2 + ((1 - b2) * g) * g;
        p += -(lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
    in fp32, one rounding per operation.  The .grad of a parameter this optimizer steps is read, never written: after a clipped
    step it is still unscaled (clip_grad_norm_ would have left it scaled; zero_grad() discards it either way).
    With max_norm, `total_norm` is a 0-d tensor on the device after each step -- the norm clip_grad_norm_ would have returned over
    the same parameters -- and `clip_coef` the coefficient the gradients were multiplied with; nothing synchronises.
    norm_params: further parameters whose gradients count in that norm although this optimizer does not step them, and are
    multiplied by clip_coef in place -- what clip_grad_norm_ does to them.  The reference's loop clips over model.parameters() but
    hands Adam only model.get_config_optim(), which leaves out the parameters outside its groups (the classifier head among them);
    optimizer.zero_grad() never clears those, so their scaled gradients accumulate from step to step and weigh on every later
    coefficient.  `Adam(model.get_config_optim(lr, lrp), max_norm=10, norm_params=model.parameters())` is that loop's coefficient,
    step after step.  Parameters that are in a group are not counted twice.
    step() runs on the current stream."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_norm=None, norm_params=None, *, amsgrad=False,
                 maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError("max_norm=%r must be None or a number >= 0" % (max_norm,))
        # every key torch.optim.Adam's groups have, at the values this optimizer implements: a state_dict loads there and steps
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        check_hyperparameters(defaults)
        super().__init__(params, defaults)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.norm_params = [] if norm_params is None else list(norm_params)
        self.total_norm = None
        self.clip_coef = None
        self._dev = None           # the buffers below live on this device
        self._key = None           # what the uploaded chunk table was built from
        self._n_chunks = 0
        self._uploads = 0

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        check_hyperparameters(self.param_groups[-1])

    # ---- device buffers ----------------------------------------------------------------------------------------------------
    def _buffers(self, device, n_chunks, n_rows):
        if self._dev != device:
            self._dev, self._key = device, None
            self._table = self._rows = self._partial = None
            self._pinned = [None] * _PINNED_SLOTS
            self._pinned_done = [None] * _PINNED_SLOTS
            self._slot = 0
            self._norm = torch.zeros(2, device=device, dtype=torch.float32)          # total_norm, clip_coef
            self._one = torch.ones(1, device=device, dtype=torch.float32)
        if self._table is None or self._table.shape[0] < n_chunks:
            self._key = None
            self._table = torch.empty(max(n_chunks, 1), ops.STEP_CHUNK_WORDS, device=device, dtype=torch.int64)
            self._partial = torch.empty(max(n_chunks, 1), device=device, dtype=torch.float64)
        if self._rows is None or self._rows.shape[0] < n_rows:
            self._rows = torch.empty(max(n_rows, 1), ops.STEP_GROUP_FLOATS, device=device, dtype=torch.float32)

    def _upload(self, dst, array):
        """dst[:len(array)] = array (numpy, the dtype and row width of dst) through a pinned host buffer, on the current stream.  The
        buffers take turns, and one is written again only after the copy that last read it has completed."""
        k = self._slot = (self._slot + 1) % _PINNED_SLOTS
        nbytes = array.nbytes
        if self._pinned_done[k] is not None:
            self._pinned_done[k].synchronize()
        if self._pinned[k] is None or self._pinned[k].numel() < nbytes:
            self._pinned[k] = torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory()
            self._pinned_done[k] = torch.cuda.Event()
        host = self._pinned[k][:nbytes]
        host.numpy()[:] = array.reshape(-1).view(np.uint8)
        dst.view(-1).view(torch.uint8)[:nbytes].copy_(host, non_blocking=True)
        self._pinned_done[k].record()
        self._uploads += 1

    # ---- the step ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # 1. what moves, checked before anything touches the GPU or any state is made; then state as torch creates it
        moving, device = [], None
        for gi, group in enumerate(self.param_groups):
            check_hyperparameters(group)
            for p in group["params"]:
                if p.grad is None:
                    continue
                check_tensors(p, p.grad, device)
                device = p.device
                if p.numel():                    # an empty tensor has nothing to update and is left as it is, state and all
                    moving.append((gi, p))
        norm_only = []
        if self.max_norm is not None and self.norm_params:
            ours = {id(p) for group in self.param_groups for p in group["params"]}
            for p in self.norm_params:
                if id(p) in ours or p.grad is None:
                    continue
                ours.add(id(p))
                check_tensors(p, p.grad, device)
                device = p.device
                if p.numel():
                    norm_only.append(p.grad)
        tensors, rows, row_of, steps = [], [], {}, []
        for gi, p in moving:
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = state["exp_avg"], state["exp_avg_sq"]
            _check_state(p, m, v)
            tensors.append((p, p.grad, m, v))
            steps.append(state["step"])
            rows.append((gi, float(state["step"]) + 1))
        if not tensors:
            return loss                          # (nothing to clip for either: no gradient is written)
        # 2. the scalar rows: one per (group, step count) in use -- parameters of one group whose gradients were None at different
        # times have different bias corrections
        scalars = []
        for i, key in enumerate(rows):
            r = row_of.get(key)
            if r is None:
                r = row_of[key] = len(scalars)
                group = self.param_groups[key[0]]
                scalars.append(group_scalars(group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], key[1]))
            rows[i] = r
        # 3. the chunk table follows the current addresses (.grad may have been reallocated); uploaded only when it changed
        ptr = np.array([[t.data_ptr() for t in four] for four in tensors] + [[g.data_ptr()] * 4 for g in norm_only], dtype=np.int64)
        numel = np.array([four[0].numel() for four in tensors] + [g.numel() for g in norm_only], dtype=np.int64)
        rows += [-1] * len(norm_only)            # counted by the norm and scaled in place, not updated
        key = (ptr.tobytes(), numel.tobytes(), tuple(rows))
        with torch.cuda.device(device):
            table = None
            if key != self._key or self._dev != device:
                table = chunk_table_from_addresses(ptr, numel, np.asarray(rows, dtype=np.int64))
                self._n_chunks = table.shape[0]
            self._buffers(device, self._n_chunks, len(scalars))
            if table is not None:
                self._upload(self._table, table)
                self._key = key
            self._upload(self._rows, np.asarray(scalars, dtype=np.float32))
            # 4. the launches
            n = self._n_chunks
            if self.max_norm is not None:
                ops.grad_sumsq(self._table, n, self._partial)
                ops.grad_clip_coef(self._partial, n, self.max_norm, self._norm)
                coef = self._norm[1:2]
                self.total_norm, self.clip_coef = self._norm[0], self._norm[1]
            else:
                coef = self._one
            ops.adam_step(self._table, n, self._rows, coef)
        # 5. the kernels wrote through addresses: tell torch, so that packs keyed on (data_ptr, _version) are rebuilt
        torch._foreach_add_(steps, 1)
        torch.autograd.graph.increment_version([four[0] for four in tensors] + norm_only)      # (and the gradients scaled in place)
        return loss
