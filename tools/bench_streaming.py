"""Developer benchmark (GPU box only): the reference's real evaluation scenario -- ONE sequence, one new frame per
forward, feature cache (test_LD_22_FPS.py:155-192) -- through cdfo_amd.streaming.StreamingSR on synthetic data."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from arch.SIDECVSR_our import CVSR_V8
from cdfo_amd.streaming import ChunkRunner, StreamingSR


def _coding():
    """--coding {LD,RA}: `StreamingSR`'s coding of every mode of this run (LD when absent)."""
    coding = sys.argv[sys.argv.index("--coding") + 1] if "--coding" in sys.argv else "LD"
    if coding not in ("LD", "RA"):
        sys.exit("--coding LD or --coding RA")
    return coding


def _synthetic(T, H, W, markers=False):
    """One synthetic sequence: 8-bit planes, a residual map, two decoder motion fields that are constant on 8x8 blocks.  markers: about
    three blocks in eight carry the random-access mark -99 in list 0, list 1 or both, drawn from a generator of their own."""
    rs = np.random.RandomState(0)
    u8 = lambda: rs.randint(0, 256, size=(T, H, W)).astype(np.uint8)
    lr, pms, ufs = u8(), u8(), u8()
    rms = np.clip(np.round(rs.randn(T, H, W) * 6), -128, 127).astype(np.float32)
    mv = rs.randint(-64, 64, size=(2, T, (H + 7) // 8, (W + 7) // 8, 3)).astype(np.float32)
    mv[..., 2] = rs.choice([-2.0, -1.0, 1.0], size=mv.shape[:-1])
    if markers:
        marks = np.random.RandomState(1).randint(0, 8, size=mv.shape[1:-1])      # 1: list 0 marked, 2: list 1, 3: both, else neither
        for l, bit in ((0, 1), (1, 2)):
            mv[l][(marks < 4) & ((marks & bit) != 0), 2] = -99.0
    mv = np.repeat(np.repeat(mv, 8, axis=2), 8, axis=3)[:, :, :H, :W]
    return lr, pms, rms, ufs, mv


def main():
    T, H, W = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 24, 270, 480
    coding = _coding()
    lr, pms, rms, ufs, mv = _synthetic(T, H, W, coding == "RA")
    model = CVSR_V8()
    model = model.cuda().eval()
    # (HIP graph, neighbour streams, frames per group, group of frames 0-2 beside the new frame's feature extraction, new frame alone)
    for use_graph, nstr, grp, ovl, alone in ((False, 2, 3, False, False), (True, 2, 3, False, False), (False, 2, 3, True, False),
                                             (True, 2, 3, True, False), (False, 2, 3, True, True), (True, 2, 3, True, True),
                                             (True, 1, 3, False, False)):
        model.neighbour_streams, model.neighbour_group, model.overlap_new_frame, model.new_frame_alone = nstr, grp, ovl, alone
        s = StreamingSR(model, lr, pms, rms, ufs, mv[0], mv[1], use_graph=use_graph, coding=coding)
        s.run()                               # warm-up (weight packing, first-touch allocations, graph capture)
        outs = s.run()
        print(f"streaming, 1 sequence of {T} frames {H}x{W} -> {tuple(outs[0].shape)}, HIP graph {use_graph}, neighbour streams {nstr}, frames per group {grp}, overlap {ovl}, new frame alone {alone}: "
              f"{s.fps:.2f} frames/s ({1e3 * s.seconds / T:.1f} ms per frame, forward only, B=1)", flush=True)


def pipelined():
    T, H, W = 48, 270, 480
    if "--size" in sys.argv:
        k = sys.argv.index("--size")
        T, H, W = int(sys.argv[k + 1]), int(sys.argv[k + 2]), int(sys.argv[k + 3])
    coding = _coding()
    lr, pms, rms, ufs, mv = _synthetic(T, H, W, coding == "RA")
    model = CVSR_V8().cuda().eval()
    s = StreamingSR(model, lr, pms, rms, ufs, mv[0], mv[1], coding=coding)
    s.run()
    s.run()
    print(f"streaming, sequential loop (per-frame timing), {T} frames {H}x{W}: {s.fps:.2f} frames/s", flush=True)
    for _ in range(3):
        s.run_pipelined()
        print(f"streaming, PIPELINED over two streams (whole-loop wall time), {T} frames: {s.fps:.2f} frames/s "
              f"({1e3 * s.seconds / T:.2f} ms per frame)", flush=True)


def chunked():
    """--chunk K [K ...] [--size T H W] [--repeats R]: run(), HIP-graph replay, run_pipelined() and run_chunked(K) on one synthetic
    sequence in one process; after a warm-up pass each mode runs R times and every repeat's frames/s is printed (the spread,
    not one number).  --only-chunk skips the three one-frame modes (for a kernel trace of the chunked path alone); --phases adds an event breakdown of
    one pass per chunk size; --share adds run_chunked(K, share_compensation=True) rows (and their --phases breakdown, with the
    per-frame compensation and the indexed warp as rows of their own); --coding RA runs every mode on the random-access field (both
    motion lists, some blocks marked) in place of the LD rule."""
    T, H, W = 64, 270, 480
    if "--size" in sys.argv:
        k = sys.argv.index("--size")
        T, H, W = int(sys.argv[k + 1]), int(sys.argv[k + 2]), int(sys.argv[k + 3])
    reps = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
    k = sys.argv.index("--chunk") + 1
    chunks = []
    while k < len(sys.argv) and sys.argv[k].isdigit():
        chunks.append(int(sys.argv[k]))
        k += 1
    coding = _coding()
    lr, pms, rms, ufs, mv = _synthetic(T, H, W, coding == "RA")
    model = CVSR_V8().cuda().eval()

    def report(name, make, loop):
        s = make()
        loop(s)                                # warm-up (weight packing, first-touch allocations, graph capture)
        fps = []
        for _ in range(reps):
            loop(s)
            fps.append(s.fps)
        print(f"{name}{', coding RA' if coding == 'RA' else ''}, {T} frames {H}x{W}: frames/s per repeat {' '.join('%.2f' % f for f in fps)}; median {np.median(fps):.2f}, "
              f"min {min(fps):.2f}, max {max(fps):.2f}" + (f"; frames extracted per pass {s.frames_extracted}" if "chunk" in name else "")
              + (f", compensated {s.frames_compensated}" if "share" in name else ""), flush=True)

    seq = lambda **kw: StreamingSR(model, lr, pms, rms, ufs, mv[0], mv[1], coding=coding, **kw)
    if "--only-chunk" not in sys.argv:
        report("run() (per-frame timing, B=1)", seq, lambda s: s.run())
        report("run() under HIP-graph replay", lambda: seq(use_graph=True), lambda s: s.run())
        report("run_pipelined() (whole-loop wall time)", seq, lambda s: s.run_pipelined())
    for c in chunks:
        report(f"run_chunked(chunk={c}) (extraction + input building + forward)", seq, lambda s: s.run_chunked(c))
        if "--share" in sys.argv:
            report(f"run_chunked(chunk={c}, share_compensation=True) (extraction + compensation + input building + forward)", seq,
                   lambda s: s.run_chunked(c, share_compensation=True))
    if "--phases" in sys.argv:
        for c in chunks:
            _phases(model, seq(), c)
            if "--share" in sys.argv:
                _phases(model, seq(), c, share=True)


def _phases(model, s, chunk, share=False):
    """Where a chunk's time goes: events around feature extraction, the neighbour pipelines + fusion, the trunk, and the whole
    chunk step (the rest = input building, the copy into the bank, the up-sampler), summed over one pass of the sequence.
    share: the shared-compensation mode -- compensation is a row of its own, "alignment + fusion" is what is left of the
    neighbour phase, and the indexed warp (one launch per neighbour group, timed on its side stream) is reported per chunk."""
    marks, keep_run = {}, ChunkRunner.run             # the whole chunk step of either mode

    def wrap(name, fn):
        def f(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            marks.setdefault(name, []).append((e0, e1))
            return r
        return f

    if share:
        from cdfo_amd import kernels as K
        s.run_chunked(chunk, share_compensation=True)
        keep_warp = K.flow_warp_frames
        model.extract_features, model.compensate_features = wrap("feature extraction", model.extract_features), wrap("compensation", model.compensate_features)
        model._fuse_windows_shared, model._trunk = wrap("alignment + fusion", model._fuse_windows_shared), wrap("trunk", model._trunk)
        ChunkRunner.run, K.flow_warp_frames = wrap("whole chunk step", keep_run), wrap("flow_warp_frames", keep_warp)
        try:
            s.run_chunked(chunk, share_compensation=True)
        finally:
            del model.extract_features, model.compensate_features, model._fuse_windows_shared, model._trunk
            ChunkRunner.run, K.flow_warp_frames = keep_run, keep_warp
        torch.cuda.synchronize()
        warp = marks.pop("flow_warp_frames")
        ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in marks.items()}
        rest = ms["whole chunk step"] - sum(v for k, v in ms.items() if k != "whole chunk step")
        nchunks = len(marks["whole chunk step"])
        print(f"phases of run_chunked(chunk={chunk}, share_compensation=True), ms per frame over {s.T} frames: "
              + ", ".join(f"{k} {v / s.T:.2f}" for k, v in ms.items()) + f", rest {rest / s.T:.2f}; flow_warp_frames "
              f"{sum(a.elapsed_time(b) for a, b in warp) / nchunks:.3f} ms per chunk ({len(warp) // nchunks} launches)", flush=True)
        return
    s.run_chunked(chunk)
    keep = model.extract_features, model._fuse_windows, model._trunk
    model.extract_features, model._fuse_windows = wrap("feature extraction", keep[0]), wrap("neighbour pipelines + fusion", keep[1])
    model._trunk, ChunkRunner.run = wrap("trunk", keep[2]), wrap("whole chunk step", keep_run)
    try:
        s.run_chunked(chunk)
    finally:
        del model.extract_features, model._fuse_windows, model._trunk
        ChunkRunner.run = keep_run
    torch.cuda.synchronize()
    ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in marks.items()}
    rest = ms["whole chunk step"] - sum(v for k, v in ms.items() if k != "whole chunk step")
    print(f"phases of run_chunked(chunk={chunk}), ms per frame over {s.T} frames: "
          + ", ".join(f"{k} {v / s.T:.2f}" for k, v in ms.items()) + f", rest {rest / s.T:.2f}", flush=True)


if __name__ == "__main__":
    if "--chunk" in sys.argv:
        chunked()
        sys.exit(0)
    if "--pipelined" in sys.argv:
        pipelined()
        sys.exit(0)
    main()
