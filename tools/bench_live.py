"""Developer benchmark (GPU box only): live sequence inference (cdfo_amd.live.LiveSR, frames pushed one at a time) against
StreamingSR.run_chunked on the same synthetic content, in one process.

    python tools/bench_live.py [--frames 64 256] [--chunks 4 8 16] [--passes 5] [--size 270 480] [--coding LD]

Per length, compensation mode and chunk size: after a warm-up pass of each, `passes` passes of run_chunked and of LiveSR ALTERNATE and
the frames/s of every pass is printed with the median (`seconds` of both covers what a chunk does on the device: input building,
extraction, forward; LiveSR's second figure is wall time over the whole loop, host staging and uploads included).  The two count as
separated when their ranges over the passes do not overlap.  Then, per chunk size, the time of the two launches that build a chunk's
inputs from the rings (cdfo_live_planes + cdfo_seq_flows_ring) beside the launches they replace (cdfo_gather_frames x 4 +
cdfo_seq_flows on the resident planes), and per length the peak allocated bytes of one pass of each with its outputs dropped chunk by
chunk.  --coding RA runs all of it on the random-access field (both motion lists pushed, some blocks marked) and adds, per chunk size, the
two random-access flow launches beside their LD twins: medians of `passes` timings each, the four forms alternating."""
import argparse
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from arch.SIDECVSR_our import CVSR_V8
from bench_streaming import _synthetic
from cdfo_amd import kernels as K
from cdfo_amd.live import LiveSR
from cdfo_amd.streaming import StreamingSR


CODING = "LD"             # --coding: every LiveSR and StreamingSR of the run


def live_pass(model, seq, chunk, share):
    """One stream through LiveSR, its frames dropped as they arrive -> (the object, wall seconds of the whole loop)."""
    lr, pms, rms, ufs, mv = seq
    s = LiveSR(model, lr.shape[1], lr.shape[2], chunk=chunk, share_compensation=share, coding=CODING)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(lr.shape[0]):
        s.push(lr[t], pms[t], rms[t], ufs[t], mv[1][t], mv[0][t] if CODING == "RA" else None)
    s.close()
    torch.cuda.synchronize()
    return s, time.perf_counter() - t0


def chunked_pass(s, chunk, share):
    for _ in s.iter_chunked(chunk, share):          # the outputs are dropped chunk by chunk, as in live_pass
        pass
    return s.fps


def throughput(model, seq, chunk, share, passes):
    T = seq[0].shape[0]
    s = StreamingSR(model, seq[0], seq[1], seq[2], seq[3], seq[4][0], seq[4][1], coding=CODING)
    chunked_pass(s, chunk, share)
    live_pass(model, seq, chunk, share)
    a, b, wall = [], [], []
    for _ in range(passes):
        a.append(chunked_pass(s, chunk, share))
        live, w = live_pass(model, seq, chunk, share)
        b.append(live.fps)
        wall.append(T / w)
    fmt = lambda v: " ".join("%.2f" % f for f in v)
    apart = min(a) > max(b) or min(b) > max(a)
    print(f"{T} frames, chunk {chunk}{', shared compensation' if share else ''}{', coding RA' if CODING == 'RA' else ''}: run_chunked frames/s per pass {fmt(a)} (median "
          f"{np.median(a):.2f}); LiveSR {fmt(b)} (median {np.median(b):.2f}; whole loop with staging and uploads {fmt(wall)}, median "
          f"{np.median(wall):.2f}); ratio of medians {np.median(b) / np.median(a):.4f}, ranges {'do not overlap' if apart else 'overlap'}",
          flush=True)


def peak_bytes(model, seq, chunk, share):
    def fresh():
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        return torch.cuda.memory_allocated()
    base = fresh()
    live_pass(model, seq, chunk, share)
    live = torch.cuda.max_memory_allocated() - base
    base = fresh()
    chunked_pass(StreamingSR(model, seq[0], seq[1], seq[2], seq[3], seq[4][0], seq[4][1], coding=CODING), chunk, share)
    return live, torch.cuda.max_memory_allocated() - base


def build_times(H, W, chunk, share, reps=50):
    """ms per chunk (steady state: `chunk` centres, `chunk` new frames): the ring launches, and the launches on resident planes."""
    Hp, Wp, cap, k = (H + 7) // 8 * 8, (W + 7) // 8 * 8, chunk + 6, chunk
    g = torch.Generator(device="cuda").manual_seed(0)
    u8 = lambda: torch.randint(0, 256, (cap, H, W), device="cuda", generator=g, dtype=torch.uint8)
    lr, uf, pm = u8(), u8(), u8()
    rm, mv = torch.randn((cap, H, W), device="cuda", generator=g), torch.randn((cap, H, W, 3), device="cuda", generator=g)
    mv0 = torch.randn((cap, H, W, 3), device="cuda", generator=g) if CODING == "RA" else None
    planes = [torch.rand((cap, Hp, Wp), device="cuda", generator=g) for _ in range(4)]
    win = [min(max(i + n - 3, 0), cap - 1) for i in range(3, 3 + k) for n in range(7)]
    new = list(range(6, 6 + k))
    dev = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    table, widx, nidx = dev(win + win + new + new), dev(win), dev(new)

    def ring():
        K.live_planes(lr, uf, pm, rm, table, k, k, Hp, Wp, 255, want_r=not share, want_r_new=share)
        K.seq_flows_ra_ring(mv0, mv, 3, k, 0, Hp, Wp) if CODING == "RA" else K.seq_flows_ring(mv, 3, k, 0, Hp, Wp)

    def resident():
        K.gather_frames(planes[0], widx), K.gather_frames(planes[3], widx), K.gather_frames(planes[1], nidx)
        K.gather_frames(planes[2], nidx if share else widx)
        K.seq_flows_ra(mv0, mv, 3, k, Hp, Wp) if CODING == "RA" else K.seq_flows(mv, 3, k, Hp, Wp)

    ms = []
    for fn in (ring, resident):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def flow_times(H, W, chunk, passes, reps=200):
    """us per launch of the four flow builders at `chunk` centres: `passes` timings of `reps` launches each, the forms alternating;
    -> {name: (median, min, max)}."""
    Hp, Wp, cap = (H + 7) // 8 * 8, (W + 7) // 8 * 8, chunk + 6
    g = torch.Generator(device="cuda").manual_seed(0)
    mv0, mv1 = (torch.randn((cap, H, W, 3), device="cuda", generator=g) for _ in range(2))
    forms = {"cdfo_seq_flows": lambda: K.seq_flows(mv1, 3, chunk, Hp, Wp),
             "cdfo_seq_flows_ra": lambda: K.seq_flows_ra(mv0, mv1, 3, chunk, Hp, Wp),
             "cdfo_seq_flows_ring": lambda: K.seq_flows_ring(mv1, 3, chunk, 0, Hp, Wp),
             "cdfo_seq_flows_ra_ring": lambda: K.seq_flows_ra_ring(mv0, mv1, 3, chunk, 0, Hp, Wp)}
    us = {name: [] for name in forms}
    for fn in forms.values():
        for _ in range(5):
            fn()
    for _ in range(passes):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / reps)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in us.items()}


def main():
    global CODING
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--chunks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=[270, 480], metavar=("H", "W"))
    ap.add_argument("--modes", nargs="+", default=["unshared", "shared"], choices=["unshared", "shared"])
    ap.add_argument("--coding", choices=("LD", "RA"), default="LD")
    a = ap.parse_args()
    H, W = a.size
    CODING = a.coding
    model = CVSR_V8().cuda().eval()
    shares = [m == "shared" for m in a.modes]
    peaks = {}
    for T in a.frames:
        seq = _synthetic(T, H, W, CODING == "RA")
        for share in shares:
            for c in a.chunks:
                throughput(model, seq, c, share, a.passes)
            peaks[T, share] = peak_bytes(model, seq, a.chunks[len(a.chunks) // 2], share)
    for share in shares:
        for c in a.chunks:
            ring, resident = build_times(H, W, c, share)
            ra = "_ra" if CODING == "RA" else ""
            print(f"input building per chunk of {c}{', shared compensation' if share else ''}: cdfo_live_planes + cdfo_seq_flows{ra}_ring "
                  f"{1e3 * ring:.1f} us; cdfo_gather_frames x 4 + cdfo_seq_flows{ra} on resident planes {1e3 * resident:.1f} us", flush=True)
    if CODING == "RA":
        for c in a.chunks:
            print(f"flow launches at {c} centres of {H}x{W}, us per launch, median of {a.passes} (min .. max): "
                  + "; ".join(f"{n} {m:.1f} ({lo:.1f} .. {hi:.1f})" for n, (m, lo, hi) in flow_times(H, W, c, a.passes).items()), flush=True)
    mib = lambda b: "%.1f MiB" % (b / 2 ** 20)
    for (T, share), (live, chunked) in peaks.items():
        print(f"peak allocated over one pass of {T} frames, chunk {a.chunks[len(a.chunks) // 2]}{', shared compensation' if share else ''}"
              f" (outputs dropped per chunk): LiveSR {mib(live)} ({live} bytes), run_chunked {mib(chunked)} ({chunked} bytes)", flush=True)


if __name__ == "__main__":
    main()
