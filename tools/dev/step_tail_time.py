"""The tail of a training step alone, on the parameter set of the whole model -- unfreeze_trunks(4, stem=True) and
unfreeze_text_encoders(), every gradient filled once with synthetic values: torch's clip_grad_norm_(model.parameters(), 10) +
torch.optim.Adam(...).step() with its defaults (the loop as it was) against mgnns_amd.optim.Adam(..., max_norm=10).step()
(csrc/step_tail.hip).  Device events around each step, a warm-up, alternating rounds, the median; the host
synchronises only around a timed region.  Also the new step's effective bandwidth at 28 bytes per element for the Adam pass plus 4
for the norm pass, the host time a step takes to enqueue, and the new step's three launches alone (the host out of the way).

    python tools/dev/step_tail_time.py [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mgnns_amd import _lib, harness, ops, optim, synth

DEV = "cuda:0"


def timed(step, steps):
    """-> (device ms per step between events, host ms per step to enqueue); one synchronise before and one after the region."""
    marks = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a, b in marks:
        a.record()
        step()
        b.record()
    host = (time.perf_counter() - t0) / steps * 1e3
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in marks], host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_tail_time.py measures on the GPU: none found")
    _lib.check_sources("tools/dev/step_tail_time.py")
    cfg = synth.CONFIGS["mvsa_multiple_b256"]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    A_obj, A_place = harness.synthetic_adjacencies(cfg)
    inp = synth.make_inputs(cfg, B=2, seed=7, pmi=pmi)
    model = harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"], DEV, trunks=True).train()
    model.unfreeze_text_encoders()
    model.unfreeze_trunks(4, stem=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for p in model.parameters():
        if p.requires_grad:
            p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-4
    ours = optim.Adam(model.get_config_optim(1e-5, 0.1), max_norm=10, norm_params=model.parameters())
    theirs = torch.optim.Adam(model.get_config_optim(1e-5, 0.1))
    everything = list(model.parameters())
    stepped = [p for g in ours.param_groups for p in g["params"] if p.grad is not None]
    elements = sum(p.numel() for p in stepped)

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(everything, 10)
        theirs.step()

    for _ in range(a.warmup):
        torch_tail()
        ours.step()
    dev = {"torch": [], "hip": []}
    host = {"torch": [], "hip": []}
    for _ in range(a.rounds):
        for name, fn in (("torch", torch_tail), ("hip", ours.step)):
            d, h = timed(fn, a.steps)
            dev[name] += d
            host[name].append(h)
    t_torch, t_hip = statistics.median(dev["torch"]), statistics.median(dev["hip"])

    def launches():          # the new step's three launches alone, on the table of the last step: what the device does once the host is ahead
        ops.grad_sumsq(ours._table, ours._n_chunks, ours._partial)
        ops.grad_clip_coef(ours._partial, ours._n_chunks, 10.0, ours._norm)
        ops.adam_step(ours._table, ours._n_chunks, ours._rows, ours._norm[1:2])

    t_kernels = statistics.median(timed(launches, a.steps * a.rounds)[0])
    print(json.dumps({
        "tensors_stepped": len(stepped), "elements_stepped": elements, "tensors_with_grad": sum(p.grad is not None for p in everything),
        "chunks": ours._n_chunks, "steps_timed_each": a.steps * a.rounds,
        "torch_clip_adam_ms": round(t_torch, 4), "torch_min_ms": round(min(dev["torch"]), 4),
        "hip_clip_adam_ms": round(t_hip, 4), "hip_min_ms": round(min(dev["hip"]), 4),
        "ratio_torch_over_hip": round(t_torch / t_hip, 3),
        "hip_effective_GBps": round(32 * elements / (t_hip * 1e-3) / 1e9, 1),
        "hip_launches_alone_ms": round(t_kernels, 4), "hip_launches_alone_GBps": round(32 * elements / (t_kernels * 1e-3) / 1e9, 1),
        "host_enqueue_ms": {k: round(statistics.median(v), 4) for k, v in host.items()},
        "total_norm": float(ours.total_norm), "sources": _lib.source_state()[0]}))


if __name__ == "__main__":
    main()
