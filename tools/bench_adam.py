"""One optimizer step over the parameters of the full CVSR_V8 with resident random gradients: `cdfo_amd.optim.DeviceAdam.step()` against
``torch.optim.Adam.step()`` (torch's default ``foreach`` choice).

    python tools/bench_adam.py [--steps 50] [--rounds 5] [--max-grad-norm X]

The two forms alternate in one process; every figure is the median of --rounds passes of --steps steps.  Per form: ``wall_us``, the host's
time to issue a step (no synchronisation inside the pass); ``device_us``, the pass between two events on the stream, per step (the larger
of the host's and the device's pace); ``kernel_us`` and ``launches``, the device time and the number of the kernels of one step as
torch.profiler sees them.  ``bytes_per_s``: 28 B per element (p, g, m, v read, p, m, v written) over DeviceAdam's ``kernel_us``.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_pass(opt, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    wall = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return wall / steps * 1e6, a.elapsed_time(b) / steps * 1e3


def kernels_of_a_step(opt):
    """(launches, device microseconds) of one step's kernels by torch.profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    if not kernels:
        raise RuntimeError("torch.profiler recorded no device kernels")
    return len(kernels), sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in kernels)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-grad-norm", type=float)
    a = ap.parse_args()
    import torch
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.optim import DeviceAdam
    torch.manual_seed(0)
    forms = {}
    for name in ("device", "torch"):
        model = CVSR_V8().cuda()
        for p in model.parameters():
            p.grad = 1e-3 * torch.randn_like(p)
        forms[name] = (DeviceAdam(model.named_parameters(), lr=1e-4, weight_decay=1e-5, max_grad_norm=a.max_grad_norm) if name == "device"
                       else torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-5))
    elements = sum(p.numel() for p in model.parameters())
    for opt in forms.values():                                  # moments made, table uploaded, code loaded
        for _ in range(3):
            opt.step()
    passes = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, opt in forms.items():
            passes[name].append(one_pass(opt, a.steps))
    out = {"elements": elements, "tensors": len(list(model.parameters())), "steps": a.steps, "rounds": a.rounds}
    for name, opt in forms.items():
        launches, kernel_us = kernels_of_a_step(opt)
        out[name] = {"wall_us": round(statistics.median(w for w, _ in passes[name]), 2),
                     "device_us": round(statistics.median(d for _, d in passes[name]), 2),
                     "wall_us_passes": [round(w, 2) for w, _ in passes[name]], "device_us_passes": [round(d, 2) for _, d in passes[name]],
                     "launches": launches, "kernel_us": round(kernel_us, 2)}
    out["device"]["bytes_per_s"] = round(28.0 * elements / (out["device"]["kernel_us"] * 1e-6), 0)
    out["device_over_torch"] = {k: round(out["device"][k] / out["torch"][k], 4) for k in ("wall_us", "device_us", "kernel_us")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
