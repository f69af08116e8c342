"""Developer benchmark (GPU box only) of the training loop's data and loss side (cdfo_amd/train_data.py, cdfo_amd/loss.py):

    python tools/bench_train_data.py [--seqs S] [--batch B] [--crop C] [--coding RA] [--no-step]

All figures are medians of five in one process, the compared forms in alternating passes after one warm-up pass each.
  batch   `ClipSet.batch` at B = 20, crop 64 on S 32-frame clips of 270 x 480 (HR 1080 x 1920): device time from events and wall time with
          a synchronisation, against the same batch built on the host by the numpy statement (tests/train_batch_ref.py) plus
          ``torch.from_numpy`` and ``.to(device)`` -- the reference's path without its PNG decode and without its worker processes.
          With --coding RA the set also holds mvl1 (a block in five without a reference in each list) and the RA batch
          (`cdfo_train_batch_ra`) is timed against the LD batch of the same plan in alternating passes of their own.
  loss    `charbonnier` forward + backward against the torch expression of tools/bench_train.py at [B,1,4C,4C], from events.
  step    the training step with a device batch and the device loss against the step as tools/bench_train.py times it (resident random
          inputs, the torch expression), forward + backward from events."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _alternate(forms, reps=5, spread=None):
    """forms: {name: fn -> None}; one warm-up pass each, then `reps` alternating passes: {name: (median event ms, median wall ms)}.
    ``spread``: a dict that receives {name: (least, greatest event ms)} of the passes."""
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ev[k].append(e0.elapsed_time(e1))
    if spread is not None:
        spread.update({k: (min(ev[k]), max(ev[k])) for k in forms})
    return {k: (float(np.median(ev[k])), float(np.median(wall[k]))) for k in forms}


def main():
    import train_batch_ref as R
    from cdfo_amd.loss import charbonnier
    from cdfo_amd.train_data import ClipSet
    S, B, c = _arg("--seqs", 4), _arg("--batch", 20), _arg("--crop", 64)
    coding = sys.argv[sys.argv.index("--coding") + 1] if "--coding" in sys.argv else "LD"
    if coding not in ("LD", "RA"):
        sys.exit(f"--coding is LD or RA, got {coding}")
    T, H, W = 32, 270, 480
    rs = np.random.RandomState(0)
    u8 = lambda *s: rs.randint(0, 256, s, dtype=np.uint8)      # noqa: E731
    mv = rs.randint(-64, 64, (S, T, H, W, 3), dtype=np.int8)
    mv[..., 2] = np.array([-2, -1, 1], np.int8)[rs.randint(0, 3, (S, T, H, W), dtype=np.int8)]     # never 0: finite flows
    arrays = (u8(S, T, H, W), u8(S, T, H, W), rs.randint(-20, 20, (S, T, H, W), dtype=np.int8), u8(S, T, H + 2, W), mv,
              u8(S, T, 4 * H, 4 * W))
    cs = ClipSet.from_arrays(*arrays)
    plan = cs.draw(B, np.random.default_rng(0), c)

    def host():
        out = R.batch(*arrays, plan, c)
        return [torch.from_numpy(out[k]).to("cuda") for k in ("x", "mvs0", "mvs1", "pms", "rms", "ufs", "hr")]

    r = _alternate({"device": lambda: cs.batch(plan, c), "host": host})
    print(f"batch of {B} at crop {c} from {S} clips of {T}x{H}x{W}, median of 5: ClipSet.batch {r['device'][0]:.3f} ms on the device, "
          f"{r['device'][1]:.3f} ms wall; host statement + upload {r['host'][1]:.1f} ms wall", flush=True)
    if coding == "RA":                           # passes of their own: a form that follows the host form's 20 ms finds an idle device
        mv1 = rs.randint(-64, 64, (S, T, H, W, 3), dtype=np.int8)
        mv1[..., 2] = np.array([-99, -2, -1, 1, 2], np.int8)[rs.randint(0, 5, (S, T, H, W), dtype=np.int8)]
        mv0 = mv.copy()
        mv0[..., 2][rs.randint(0, 5, (S, T, H, W), dtype=np.int8) == 0] = -99
        cs_ra = ClipSet.from_arrays(*arrays[:4], mv0, arrays[5], mvl1=mv1, coding="RA")
        spread = {}
        r = _alternate({"ld": lambda: cs.batch(plan, c), "ra": lambda: cs_ra.batch(plan, c)}, spread=spread)
        print(f"RA batch against the LD batch of the same plan, median of 5: RA {r['ra'][0]:.3f} ms on the device, {r['ra'][1]:.3f} ms wall "
              f"(passes {spread['ra'][0]:.3f} .. {spread['ra'][1]:.3f} ms); LD {r['ld'][0]:.3f} ms on the device, {r['ld'][1]:.3f} ms wall "
              f"(passes {spread['ld'][0]:.3f} .. {spread['ld'][1]:.3f} ms)", flush=True)

    sr = torch.rand(B, 1, 4 * c, 4 * c, device="cuda", requires_grad=True)
    hr = torch.rand(B, 1, 4 * c, 4 * c, device="cuda")

    def loss_hip():
        sr.grad = None
        charbonnier(sr, hr).backward()

    def loss_torch():
        sr.grad = None
        torch.sum(torch.sqrt((sr - hr) ** 2 + 1e-4)).backward()

    r = _alternate({"hip": loss_hip, "torch": loss_torch})
    print(f"Charbonnier forward + backward at {tuple(sr.shape)}, median of 5: charbonnier {r['hip'][0]:.3f} ms, torch expression "
          f"{r['torch'][0]:.3f} ms (events); wall {r['hip'][1]:.3f} / {r['torch'][1]:.3f} ms", flush=True)
    if "--no-step" in sys.argv:
        return

    from arch.SIDECVSR_our import CVSR_V8
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _inputs import random_inputs
    m = CVSR_V8().cuda().train()
    d = {k: v for k, v in random_inputs(B, c, c, 7).items() if k != "gumbel_u"}
    hr_fixed = torch.rand(B, 1, 4 * c, 4 * c, device="cuda")

    def step_old():
        m.zero_grad(set_to_none=True)
        out, _ = m(d["x"], d["mvs0"], d["mvs1"], d["pms"], d["rms"], d["ufs"])
        torch.sum(torch.sqrt((out - hr_fixed) ** 2 + 1e-4)).backward()

    def step_new():
        m.zero_grad(set_to_none=True)
        x, mvs0, mvs1, pms, rms, ufs, hr_b = cs.batch(plan, c)
        out, _ = m(x, mvs0, mvs1, pms, rms, ufs)
        charbonnier(out, hr_b).backward()

    r = _alternate({"old": step_old, "new": step_new})
    print(f"training step {B}x{c}x{c} (forward + loss + backward), median of 5: resident inputs + torch loss {r['old'][0]:.1f} ms, "
          f"device batch + charbonnier {r['new'][0]:.1f} ms (events); wall {r['old'][1]:.1f} / {r['new'][1]:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
