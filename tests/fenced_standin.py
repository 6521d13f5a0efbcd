"""A tiny stand-in for mgnns_amd/ops.py: functions that allocate through a module-global `torch` and a module-level zeros_bytes, the
way the wrappers do.  tests/test_fenced_alloc_cpu.py runs the fenced arena against it on the CPU; it launches nothing."""
import torch


def zeros_bytes(nbytes, device):
    return torch.zeros((int(nbytes) + 255) // 256 * 256, dtype=torch.uint8, device=device)


def zeros_i32(n, device):
    return zeros_bytes(4 * n, device).view(torch.int32)[:n]


def out_f32(rows, cols, device):
    return torch.empty(rows, cols, device=device, dtype=torch.float32)          # SITE out_f32


def out_shape(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)                       # SITE out_shape


def like(t, **kw):
    return torch.empty_like(t, **kw)                                            # SITE like


def zeroed(n, dtype, device):
    return torch.zeros(n, device=device, dtype=dtype)                           # SITE zeroed


def counter(n, device):
    return zeros_i32(n, device)                                                 # SITE counter


def host_staging(n, pin=False):
    return torch.empty(n, dtype=torch.uint8, pin_memory=pin), torch.zeros(n), torch.empty(n, device="cpu")


def other_names():
    return torch.float32, torch.arange(3), torch.is_tensor(torch.ones(1))
