"""Live sequence inference: frames and their coding priors are pushed as they decode, device memory does not grow with the stream.

`StreamingSR.run_chunked` needs the whole sequence before its first forward; a super-resolver behind a video decoder gets one frame
at a time and does not know how long the stream is.  `LiveSR` is the same chunked forward fed incrementally:

* `LivePlanner` emits `plan_chunks`' own plans as frames arrive.  A chunk of centres c0 .. c0+K-1 needs frames up to c0+K+2; once
  that frame has been pushed, T >= c0+K+3, so every centre of the chunk is at most T-4: no window of it is clipped at the far end,
  none of the three end rules of `modify_mv_for_end_frames` applies and T > 1 is known.  The chunk planned with only the pushed
  frames known is therefore the chunk `plan_chunks(T, K)` yields for the true T; `close()` plans the remaining centres (at most
  K + 2, hence at most three chunks) with T known.
* The inputs live in rings of chunk + 6 frames in the files' own sample types (frame t in slot t mod (chunk + 6), `bank_slot`);
  two launches build everything a chunk reads from them (libcdfo_hip.so: cdfo_live_planes, cdfo_seq_flows_ring), bit for bit what
  `StreamingSR` builds from the resident sequence.
* The chunk step is `streaming.ChunkRunner.run`, the one `run_chunked` makes, with the same model calls on the same shapes in the
  same order: the frames are bit-identical to ``StreamingSR(...).run_chunked(chunk)`` on the completed sequence.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from .streaming import (NFRAMES, ChunkPlan, ChunkRunner, bank_slot, check_coding, check_noise_format, check_peak, cropped, padded,
                        plan_chunks)


class LivePlanner:
    """`plan_chunks` for a sequence whose length is not known yet (host only): `push()` once per arriving frame returns the plan of
    the chunk that has just become runnable (the push of frame c0 + chunk + 2 releases the chunk that starts at centre c0) or
    None; `close()` returns the plans of the remaining centres, at most three.  What the two return, concatenated, is
    ``list(plan_chunks(T, chunk))`` for the T frames pushed."""

    def __init__(self, chunk: int):
        if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
            raise ValueError(f"LivePlanner: chunk >= 1 expected, got {chunk!r}")
        self.chunk = chunk
        self.pushed = 0            # frames 0 .. pushed-1 have arrived
        self.closed = False
        self._next = 0             # the first centre no emitted plan holds, a multiple of chunk
        self._extracted = 0        # frames 0 .. _extracted-1 are scheduled for extraction by the emitted plans

    def _emit(self, plan: ChunkPlan) -> ChunkPlan:
        self._next += self.chunk
        self._extracted = max(self._extracted, plan.windows[-1][-1] + 1)
        return plan

    def push(self) -> Optional[ChunkPlan]:
        if self.closed:
            raise RuntimeError("LivePlanner.push after close()")
        self.pushed += 1
        if self.pushed < self._next + self.chunk + NFRAMES // 2:
            return None
        # the far end is at least four frames beyond the chunk's last centre: the plan does not depend on it
        return self._emit(next(plan_chunks(self.pushed, self.chunk, self._next, self._extracted)))

    def close(self) -> List[ChunkPlan]:
        if self.closed:
            raise RuntimeError("LivePlanner.close called twice")
        self.closed = True
        if self.pushed == 0 or self._next >= self.pushed:
            return []
        return [self._emit(p) for p in plan_chunks(self.pushed, self.chunk, self._next, self._extracted)]


class _Indexed:
    """A callable of the index read like a sequence (the noise arguments of `LiveSR` are either)."""

    def __init__(self, fn):
        self.fn = fn

    def __getitem__(self, i):
        return self.fn(i)


def check_push_lists(coding: str, mvl0) -> None:
    """Which motion lists a push must carry: list 1 always, list 0 exactly when the stream builds the random-access field."""
    if coding == "RA" and mvl0 is None:
        raise ValueError("LiveSR.push: coding='RA' builds its flows from both lists: pass mvl0= with every frame")
    if coding != "RA" and mvl0 is not None:
        raise ValueError("LiveSR.push: mvl0 is read by coding='RA' only; this stream was opened with coding='LD', which would drop it")


_REAL = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64,
         torch.uint16)
STAGING_SETS = 2


class LiveSR:
    """One stream of frames of ``height`` x ``width``, super-resolved ``chunk`` centre frames per forward as they arrive.

        s = LiveSR(model, height, width, chunk=8)
        for every decoded frame:  done = s.push(lr, pm, rm, uf, mvl1)     # [(index, frame [1,1,4H,4W] fp32), ...], possibly empty
        done = s.close()                                                 # the tail; afterwards push raises RuntimeError

    lr, pm, rm, uf : [H,W]; mvl1 : [H,W,3] (list 1's field: the model reads mvs1 only).  Each is a numpy array, a CPU tensor or a
    tensor on the model's device.  lr / uf: uint8 at peak <= 255, uint16 above; pm: uint8; rm: any real dtype, converted with
    ``astype(float32)``; mvl1: any dtype `kernels.seq_flows` accepts, converted the same way (the first step of `mv2mvs`).  A wrong
    shape or dtype raises ValueError before anything is copied.  The reference reads the priors and the motion field of frame 0
    from entry 1 (``max(1, i)``): frame 0's pm, rm, uf and mvl1 are read only if the stream closes after one frame.

    The frames returned by all pushes and `close`, in order, are bit-identical to ``StreamingSR(model, <the whole sequence>,
    peak=peak, ...).run_chunked(chunk, share_compensation)``: the same planes and flows go through the same model calls.  Centre i
    of the chunk that starts at c0 comes out of the push of frame c0 + chunk + 2, or of `close`.

    Device state: rings of exactly chunk + 6 slots for the four sample planes and the motion field (in the files' sample types), the
    feature bank and, with share_compensation, the compensation ring -- nothing whose size depends on the number of frames pushed
    (`resident_bytes`).  Uploads: `push` copies host arrays into pinned staging and enqueues the host-to-device copies on a copy
    stream of its own, so the caller may overwrite its arrays as soon as `push` returns; a device tensor is copied into its ring
    slot on the current stream.  Ordering is by events: a chunk's two build kernels wait for the uploads of the frames they read,
    an upload into a ring slot waits for the build kernels of the last chunk that read the slot's previous frame, and the host
    rewrites a staging buffer only after that buffer's own upload has completed.

    coding="RA" (opt-in; "LD" is everything above, unchanged): the stream builds `StreamingSR`'s random-access field
    (`streaming.mv2mvs_ra`): ``push(lr, pm, rm, uf, mvl1, mvl0)`` takes list 0's field as well (same shape and dtype as mvl1), a second
    fp32 motion ring and a staging buffer of its own in each set hold it, and the chunk's flows come from cdfo_seq_flows_ra_ring.  The
    frames are then bit-identical to ``StreamingSR(..., coding="RA").run_chunked(chunk, share_compensation)``.

    Noise: gumbel_uniform (per centre frame: six draws [1,64,Hp,Wp]) and frame_noise (per frame, read by share_compensation only)
    are a sequence or a callable of the index, under `check_noise_format`'s rules.  Without them the unshared mode draws per forward
    call like `run_chunked`, and the shared mode takes one Philox key per stream before its first extraction, draw = frame index."""

    def __init__(self, model, height: int, width: int, chunk: int = 8, share_compensation: bool = False, peak: int = 255,
                 gumbel_uniform=None, frame_noise=None, coding: str = "LD"):
        self.coding = check_coding(coding)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise NotImplementedError("LiveSR needs the model on a GPU (HIP path, no CPU fallback)")
        self.peak = check_peak(peak)
        if min(int(height), int(width)) < 1:
            raise ValueError(f"LiveSR: a positive frame size expected, got {height} x {width}")
        self.shared = bool(share_compensation)
        self.model, self.dev = model, dev
        self.plan = LivePlanner(chunk)
        self.chunk, self.H, self.W = chunk, int(height), int(width)
        self.Hp, self.Wp = padded(self.H, self.W)
        seq = lambda n: None if n is None else _Indexed(n) if callable(n) else n
        self.noise, self.frame_noise = seq(gumbel_uniform), seq(frame_noise)
        self._check_noise(None)
        self.sample = torch.uint8 if peak <= 255 else torch.uint16
        cap, H, W = chunk + NFRAMES - 1, self.H, self.W
        # the feature bank, the compensation ring, the key and the counters of the stream; it waits for this stream only
        self._runner = ChunkRunner(model, dev, self.Hp, self.Wp, cap, self.shared, self.noise, self.frame_noise,
                                   lambda: torch.cuda.current_stream(dev).synchronize())
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        # frame t lives in slot t mod cap of every ring
        self._rings = {"lr": new((cap, H, W), self.sample), "uf": new((cap, H, W), self.sample), "pm": new((cap, H, W), torch.uint8),
                       "rm": new((cap, H, W), torch.float32), "mv": new((cap, H, W, 3), torch.float32)}
        if self.coding == "RA":           # list 0's fields beside list 1's, with a staging buffer of their own in each set
            self._rings["mv0"] = new((cap, H, W, 3), torch.float32)
        self._copy = torch.cuda.Stream(dev)
        for t in self._rings.values():
            t.record_stream(self._copy)
        pinned = lambda k: torch.empty(self._rings[k].shape[1:], dtype=self._rings[k].dtype).pin_memory()
        self._staging = [({k: pinned(k) for k in self._rings}, torch.cuda.Event()) for _ in range(STAGING_SETS)]
        self._staged = 0                  # host frames staged so far: set _staged mod STAGING_SETS is rewritten next
        self._last_upload = None          # the event behind the newest upload on the copy stream (which runs in order)
        self._slot_read = [None] * cap    # per ring slot: the event behind the build kernels of the last chunk that read it
        self.frames_out = 0

    # -- what the object reports --------------------------------------------------------------------------------------------------
    @property
    def frames_pushed(self) -> int:
        return self.plan.pushed

    @property
    def seconds(self) -> float:
        return self._runner.count.seconds

    @property
    def frames_extracted(self) -> int:
        """Frames sent through feature extraction since this object was made: the number pushed once `close` has returned."""
        return self._runner.count.frames_extracted

    @property
    def frames_compensated(self) -> int:
        """Frames sent through `compensate_features` (share_compensation only; a chunk the range guard repeats adds its windows')."""
        return self._runner.count.frames_compensated

    @property
    def ring_capacity(self) -> int:
        return self.chunk + NFRAMES - 1

    @property
    def resident_bytes(self) -> int:
        """The object's own persistent device buffers: the five input rings (six with coding="RA": list 0's motion ring), the feature
        bank and the compensation ring."""
        return sum(t.numel() * t.element_size() for t in self._rings.values()) + self._runner.resident_bytes

    @property
    def fps(self) -> float:
        return self.frames_out / self.seconds if self.seconds > 0 else float("nan")

    # -- input side -----------------------------------------------------------------------------------------------------------------
    def _check_noise(self, T: Optional[int]) -> None:
        """`check_noise_format`; the one-entry-per-frame rule can only be judged once the stream has closed (T known)."""
        fn = self.frame_noise
        if T is None or not hasattr(fn, "__len__"):       # a callable, or the stream is still open: the format rule alone
            fn, T = (None if fn is None else ()), 0
        check_noise_format(self.shared, self.noise, fn, T)

    def _checked(self, name: str, a, shape, dtypes) -> torch.Tensor:
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
        if tuple(t.shape) != shape:
            raise ValueError(f"LiveSR.push: {name} must be {list(shape)}, got {list(t.shape)}")
        if t.dtype not in dtypes:
            raise ValueError(f"LiveSR.push: {name} must be of {' / '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if t.device.type != "cpu" and t.device != self.dev:
            raise ValueError(f"LiveSR.push: {name} lives on {t.device}; a host array or a tensor on {self.dev} expected")
        return t

    def push(self, lr, pm, rm, uf, mvl1, mvl0=None) -> List[Tuple[int, torch.Tensor]]:
        """One frame and its priors.  Returns the frames of the chunk this push made runnable, complete, or [].  mvl0: list 0's field
        of the frame, required with coding="RA" and refused (ValueError) with coding="LD", which would never read it."""
        if self.plan.closed:
            raise RuntimeError("LiveSR.push after close()")
        check_push_lists(self.coding, mvl0)
        from . import kernels as K
        hw = (self.H, self.W)
        frame = {"lr": self._checked("lr", lr, hw, (self.sample,)), "pm": self._checked("pm", pm, hw, (torch.uint8,)),
                 "rm": self._checked("rm", rm, hw, _REAL), "uf": self._checked("uf", uf, hw, (self.sample,)),
                 "mv": self._checked("mvl1", mvl1, hw + (3,), tuple(K._MV_DTYPES))}
        if self.coding == "RA":
            frame["mv0"] = self._checked("mvl0", mvl0, hw + (3,), tuple(K._MV_DTYPES))
            if frame["mv0"].dtype != frame["mv"].dtype:      # one rule decides what marks a block: both lists in one type
                raise ValueError(f"LiveSR.push: mvl0 and mvl1 must be of one dtype, got {frame['mv0'].dtype} and {frame['mv'].dtype}")
        slot = bank_slot(self.plan.pushed, self.ring_capacity)
        host = {k: t for k, t in frame.items() if not t.is_cuda}
        with torch.cuda.device(self.dev):
            for k, t in frame.items():
                if t.is_cuda:             # ring to ring on the caller's stream, behind whatever produced the tensor there (and
                    self._rings[k][slot].copy_(t)     # behind the build kernels that read the slot, which ran on it as well)
            if host:
                stage, uploaded = self._staging[self._staged % STAGING_SETS]
                self._staged += 1
                uploaded.synchronize()                # this buffer's own previous upload (a no-op on a fresh event)
                for k, t in host.items():
                    stage[k].copy_(t)                 # converts rm and mvl1 like astype(float32)
                if self._slot_read[slot] is not None:
                    self._copy.wait_event(self._slot_read[slot])
                with torch.cuda.stream(self._copy):
                    for k in host:
                        self._rings[k][slot].copy_(stage[k], non_blocking=True)
                    uploaded.record(self._copy)
                self._last_upload = uploaded
        plan = self.plan.push()
        return [] if plan is None else self._run(plan, 0)

    def close(self) -> List[Tuple[int, torch.Tensor]]:
        """The end of the stream: the remaining centre frames (at most chunk + 2, in at most three forwards), with T known."""
        if self.plan.closed:
            raise RuntimeError("LiveSR.close called twice")
        self._check_noise(self.plan.pushed)
        T = self.plan.pushed
        return [f for plan in self.plan.close() for f in self._run(plan, T)]

    # -- one chunk --------------------------------------------------------------------------------------------------------------------
    def _run(self, plan: ChunkPlan, T_known: int) -> List[Tuple[int, torch.Tensor]]:
        from . import kernels as K
        k, E, cap = len(plan.centres), len(plan.extract), self.ring_capacity
        slot = lambda t: bank_slot(t, cap)
        live = [slot(t) for w in plan.windows for t in w] + [slot(e) for w in plan.priors for e in w] \
            + [slot(t) for t in plan.extract] + [slot(e) for e in plan.extract_priors]
        head, R, head_t = self._runner.head(plan), self._rings, None

        def build():          # the chunk's tables in one upload, then its inputs from the rings in two launches
            nonlocal head_t
            tables = torch.tensor(head + live, dtype=torch.int32).to(self.dev)
            head_t = tables[:len(head)]
            cur = torch.cuda.current_stream(self.dev)
            if self._last_upload is not None:
                cur.wait_event(self._last_upload)
            planes = K.live_planes(R["lr"], R["uf"], R["pm"], R["rm"], tables[len(head):], k, E, self.Hp, self.Wp, self.peak,
                                   want_r=not self.shared, want_r_new=self.shared)
            if self.coding == "RA":
                m1 = K.seq_flows_ra_ring(R["mv0"], R["mv"], plan.centres[0], k, T_known, self.Hp, self.Wp)
            else:
                m1 = K.seq_flows_ring(R["mv"], plan.centres[0], k, T_known, self.Hp, self.Wp)
            read = torch.cuda.Event()
            read.record(cur)
            for s in set(live):
                self._slot_read[s] = read
            return (*planes, m1)

        out = self._runner.run(plan, lambda: head_t, build, self._rms_planes)
        self.frames_out += k
        return list(zip(plan.centres, cropped(out, self.H, self.W)))

    def _rms_planes(self, entries: List[int]) -> torch.Tensor:
        """The residual planes [F,Hp,Wp] of a list of prior entries, from the ring (a chunk that the range guard repeats)."""
        from . import kernels as K
        R, n = self._rings, len(entries)
        slots = [bank_slot(e, self.ring_capacity) for e in entries]
        table = torch.tensor(slots[:1] * (2 * NFRAMES) + slots + slots, dtype=torch.int32).to(self.dev)
        return K.live_planes(R["lr"], R["uf"], R["pm"], R["rm"], table, 1, n, self.Hp, self.Wp, self.peak, want_r=False)[5]

