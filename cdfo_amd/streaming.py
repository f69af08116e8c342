"""Streaming evaluation of one sequence on the device: the caller side of ``CVSR_V8.forward(..., pre_L1_fea)``.

Mirrors the reference's evaluation loop (``test_LD_22_FPS.py:155-189``) with the sequence resident in HBM: the LR
frames and the coding priors are uploaded ONCE, each step gathers its seven-frame window by index on the device (the
reference re-reads and re-uploads six repeated frames per step), converts the decoder's motion field to the seven
per-slot flows (``mv2mvs``, ``:100-122``), applies the sequence-boundary fix-ups (``modify_mv_for_end_frames``,
``:200-225``) and calls the model with the feature cache returned by the previous step, so that only ONE new frame
goes through feature extraction (``arch/SIDECVSR_our.py:4420-4427``).  Quirks of the reference loop that are kept:
window indices are clipped to the sequence (``generate_input_index``, ``:14-17``); the priors and motion fields of
frame 0 are read from entry 1 (``ii = max(1, i)``, ``:36,53,66,168``); ``x / 0`` in ``mv2mvs`` stays ``inf`` (only NaN
becomes 0).

``run_chunked`` processes the same sequence several centre frames per forward against a per-frame feature bank (each frame
extracted once; `plan_chunks` is its schedule), with the windows, planes and flows built by the library's own kernels.
With ``share_compensation=True`` (opt-in) the per-frame half of the six neighbour pipelines (residual-map stem, RDAB compensation,
conv_expand_fea_r) is also computed once per frame, into a second ring beside the feature bank, with ONE Gumbel draw per frame;
the reference draws per (step, slot), so the windows of different output frames then see correlated noise -- see `run_chunked`.
"""
from __future__ import annotations

import time
from typing import Iterator, List, NamedTuple, Optional, Sequence, Tuple

import torch

NFRAMES = 7


def generate_input_index(center_index: int, frame_number: int, max_index: int) -> torch.Tensor:
    """test_LD_22_FPS.py:14-17."""
    return (torch.arange(frame_number) - (frame_number // 2) + center_index).clamp_(0, max_index)


def mv2mvs(mv: torch.Tensor) -> torch.Tensor:
    """test_LD_22_FPS.py:100-122.  mv: [H,W,3] (any float/int dtype, any device) -> flows [7,2,H,W] in pixels, ready for
    ``mvs.unsqueeze(0)`` (the reference's ``permute(0,1,4,2,3)`` is folded in)."""
    m = mv.to(torch.float32)
    d = m[..., 2] * -1.0
    fx, fy = m[..., 1] / d, m[..., 0] / d                       # components swapped (:103)
    f = torch.stack([torch.where(torch.isnan(fx), torch.zeros_like(fx), fx),
                     torch.where(torch.isnan(fy), torch.zeros_like(fy), fy)], 0)      # [2,H,W]
    scale = torch.tensor([3.0, 2.0, 1.0, 0.0, -1.0, -2.0, -3.0], device=m.device).view(7, 1, 1, 1)
    out = f.unsqueeze(0) * scale
    out[3] = 0.0                                                # slot 3 stays zero (0 * inf would be NaN)
    return out / (4.0 * 32.0)


CODINGS = ("LD", "RA")
RA_MARK = -99.0             # a block with no reference in a list carries this in its reference component (opt/data_RA_bi.py)


def check_coding(coding) -> str:
    if coding not in CODINGS:
        raise ValueError(f"coding must be one of {CODINGS}, got {coding!r}")
    return coding


def check_ra_lists(who: str, mv0: torch.Tensor, mv1: torch.Tensor) -> None:
    """The two lists of a random-access field are read together, element by element: one shape, one dtype, one device."""
    if mv0.shape != mv1.shape or mv0.dtype != mv1.dtype or mv0.device != mv1.device:
        raise ValueError(f"{who}: the two motion lists must agree in shape, dtype and device, got {mv0.dtype} {tuple(mv0.shape)} on "
                         f"{mv0.device} and {mv1.dtype} {tuple(mv1.shape)} on {mv1.device}")


def mv2mvs_ra(mv0: torch.Tensor, mv1: torch.Tensor) -> torch.Tensor:
    """The random-access field of one frame, opt/data_RA_bi.py's rule without the flips (tests/train_batch_ra_ref.py::flows):
    mv0, mv1: [H,W,3] of the two lists (one dtype, one device) -> flows [7,2,H,W] in pixels.  Slots 0-2 come from list 0
    (``/ (ref * -1)``), slots 4-6 from list 1 (``/ ref``), NaN -> 0 and x / 0 stays inf as in `mv2mvs`; a block with no reference in
    one list (``ref == -99`` after the conversion to fp32) takes the other list's vector, negated.  Nothing is clipped."""
    check_ra_lists("mv2mvs_ra", mv0, mv1)
    if mv0.dim() != 3 or mv0.shape[2] != 3:
        raise ValueError(f"mv2mvs_ra: fields [H,W,3] expected, got {tuple(mv0.shape)}")
    m0, m1 = mv0.to(torch.float32), mv1.to(torch.float32)

    def vector(m, d):                                          # components swapped, NaN -> +0
        fx, fy = m[..., 1] / d, m[..., 0] / d
        return torch.stack([torch.where(torch.isnan(fx), torch.zeros_like(fx), fx),
                            torch.where(torch.isnan(fy), torch.zeros_like(fy), fy)], 0)      # [2,H,W]

    p2, p4 = vector(m0, m0[..., 2] * -1.0), vector(m1, m1[..., 2])
    p2 = torch.where(m0[..., 2] == RA_MARK, -p4, p2)
    p4 = torch.where(m1[..., 2] == RA_MARK, -p2, p4)           # p2 after the line above: both marked leaves p4 as it was
    w = torch.tensor([3.0, 2.0, 1.0], device=m0.device).view(3, 1, 1, 1)
    out = torch.zeros((NFRAMES,) + tuple(p2.shape), dtype=torch.float32, device=m0.device)
    out[0:3] = p2.unsqueeze(0) * w
    out[4:7] = p4.unsqueeze(0) * w.flip(0)
    return out / (4.0 * 32.0)


def modify_mv_for_end_frames(i: int, mvs: torch.Tensor, max_idx: int) -> torch.Tensor:
    """test_LD_22_FPS.py:200-225 on mvs [B,7,2,H,W], in place; max_idx = number of frames in the sequence."""
    if i == 0:
        mvs[:, 0:3] = 0.0
    if i == 1:
        mvs[:, 0] = mvs[:, 2]
        mvs[:, 1] = mvs[:, 2]
    if i == 2:
        mvs[:, 0] = mvs[:, 1]
    if i == max_idx - 1:
        mvs[:, 4:7] = 0.0
    if i == max_idx - 2:
        mvs[:, 5] = mvs[:, 4]
        mvs[:, 6] = mvs[:, 4]
    if i == max_idx - 3:
        mvs[:, 6] = mvs[:, 5]
    return mvs


class ChunkPlan(NamedTuple):
    """One chunk of `plan_chunks`: plain Python integers, no device work."""
    centres: List[int]            # the centre frames of the chunk, consecutive
    windows: List[List[int]]      # per centre: the seven frame indices of its window (= generate_input_index)
    priors: List[List[int]]       # per centre: the entries its pms / rms / ufs planes are read from (max(1, .); 0 if T == 1)
    mv_entry: List[int]           # per centre: the entry its motion fields are read from (max(1, i); 0 if T == 1)
    extract: List[int]            # frames that go through feature extraction before this chunk's forward, consecutive
    extract_priors: List[int]     # per extracted frame: the entry its pms plane is read from
    oldest: int                   # the bank may drop every frame below this one before the chunk's forward
    # shared-compensation mode: a frame is compensated by the chunk that extracts it, into the same slot of a second ring
    compensate: List[int]                 # frames that go through compensate_features before this chunk's forward (= extract)
    compensate_priors: List[int]          # per compensated frame: the entry its rms plane is read from (max(1, .); 0 if T == 1)


def plan_chunks(T: int, chunk: int, first: int = 0, extracted: int = 0) -> Iterator[ChunkPlan]:
    """The schedule of `StreamingSR.run_chunked` for a sequence of T frames, `chunk` centre frames per forward (the last chunk
    may be shorter).  The features a window uses for frame t are always those of (lr[t], pms[max(1, t)]), whichever step or
    slot asks, so every frame is extracted once, by the first chunk whose windows reach it, and is kept until the last window
    that contains it has run: at most chunk + 6 frames are resident.  `first`, `extracted`: resume the schedule at centre `first` (a
    multiple of `chunk`) with frames 0 .. extracted-1 already scheduled by the chunks before it (`cdfo_amd.live.LivePlanner`)."""
    if T < 1 or chunk < 1:
        raise ValueError(f"plan_chunks: T >= 1 and chunk >= 1 expected, got T = {T}, chunk = {chunk}")
    if first < 0 or first % chunk or extracted < 0:
        raise ValueError(f"plan_chunks: first must be a non-negative multiple of chunk and extracted >= 0, got {first}, {extracted}")
    prior = (lambda t: max(1, t)) if T > 1 else (lambda t: 0)
    half = NFRAMES // 2
    for c0 in range(first, T, chunk):                              # frames 0 .. extracted-1 have been scheduled
        centres = list(range(c0, min(c0 + chunk, T)))
        windows = [[min(max(i + n - half, 0), T - 1) for n in range(NFRAMES)] for i in centres]
        reach = windows[-1][-1] + 1
        extract = list(range(extracted, reach))
        extracted = max(extracted, reach)
        yield ChunkPlan(centres, windows, [[prior(t) for t in w] for w in windows], [prior(i) for i in centres], extract,
                        [prior(t) for t in extract], windows[0][0], list(extract), [prior(t) for t in extract])


def bank_capacity(T: int, chunk: int) -> int:
    """Frames of features the bank of `run_chunked` holds: the chunk's centres and three neighbours on either side."""
    return min(chunk, T) + NFRAMES - 1


def bank_slot(t: int, capacity: int) -> int:
    """The bank is a ring: frame t lives in slot t mod capacity, and is overwritten by frame t + capacity."""
    return t % capacity


def bank_runs(first: int, count: int, capacity: int) -> List[tuple]:
    """Frames first .. first+count-1 as contiguous runs of ring slots: [(slot, offset into the run of frames, length)], at most two."""
    runs, done = [], 0
    while done < count:
        slot = bank_slot(first + done, capacity)
        n = min(count - done, capacity - slot)
        runs.append((slot, done, n))
        done += n
    return runs


NEIGHBOUR_SLOTS = (0, 1, 2, 4, 5, 6)


def comp_slot_table(plan: ChunkPlan, capacity: int) -> List[int]:
    """The [6,K] table of `CVSR_V8.forward_windows_shared` for one chunk, flat and slot-major over the neighbour slots 0, 1, 2, 4,
    5, 6: entry [n][k] = the ring slot of the frame that window k has at neighbour slot n."""
    return [bank_slot(w[n], capacity) for n in NEIGHBOUR_SLOTS for w in plan.windows]


def check_noise_format(share_compensation: bool, gumbel_uniform, frame_noise, T: int) -> None:
    """Injected noise comes per step (`gumbel_uniform`: T entries of six [1,64,H,W] draws, one per neighbour slot of that step's
    window) or per frame (`frame_noise`: T tensors [1,64,H,W]).  The shared mode draws once per FRAME and the unshared modes once
    per (step, slot): neither format converts into the other.  (The unshared modes never read `frame_noise`.)"""
    if share_compensation and frame_noise is None and gumbel_uniform is not None:
        raise ValueError("run_chunked(share_compensation=True) draws one noise tensor per frame: pass frame_noise= (T tensors "
                         "[1,64,H,W]); the per-step gumbel_uniform= format does not convert")
    if share_compensation and frame_noise is not None and len(frame_noise) != T:
        raise ValueError(f"frame_noise must hold one tensor per frame (T = {T}), got {len(frame_noise)}")


def store_frames(ring: torch.Tensor, first: int, frames: torch.Tensor) -> None:
    """frames[j] -> the ring slot of frame first + j (`bank_slot`), at most two contiguous copies."""
    for slot, off, n in bank_runs(first, int(frames.shape[0]), int(ring.shape[0])):
        ring[slot:slot + n].copy_(frames[off:off + n])


def compensate_frames(model, dev, fea, frames: List[int], rms_planes, key, frame_noise):
    """compensate_features of `frames` (their features `fea`, their rms planes [F,Hp,Wp]) with each frame's own noise: its
    injected tensor, or draw = frame index under the sequence's key."""
    noise = None if frame_noise is None else [frame_noise[t] for t in frames]
    if noise is None:
        model.resolve_noise_key(dev, key)
    return model.compensate_features(fea, rms_planes.unsqueeze(1), gumbel_uniform=noise, draws=frames)


def chunk_forward(model, plan: ChunkPlan, bank, lf_idx, lr_new, p_new, x, r, u, m1, noise) -> torch.Tensor:
    """The model calls of one chunk, whoever built its inputs (`StreamingSR` from the resident sequence, `cdfo_amd.live.LiveSR`
    from its rings): the frames the chunk is the first to reach (lr_new, p_new [E,Hp,Wp]: their LR planes and the partition maps of
    their prior entries) are extracted into the bank (frame t lives in slot t mod capacity; what it overwrites is below
    `plan.oldest`), the window stack is gathered from the bank, one forward at batch len(plan.centres) on x, r, u [K,7,1,Hp,Wp] and
    the flows m1.  Returns the padded output [len(plan.centres),1,4Hp,4Wp]."""
    from . import kernels as K
    k = len(plan.centres)
    if plan.extract:
        store_frames(bank, plan.extract[0], model.extract_features(lr_new.unsqueeze(1), p_new.unsqueeze(1)))
    Lf = K.gather_frames(bank, lf_idx).view(NFRAMES, k, *bank.shape[1:])
    # (the model reads mvs1 only, like the reference's forward: mvl0's flows are not built)
    return model.forward_windows(Lf, x, None, m1, r, u, gumbel_uniform=noise)


def chunk_forward_shared(model, plan: ChunkPlan, bank, comp_bank, comp_idx, centre_idx, lr_new, p_new, r_new, x, u, m1, compensate,
                         rms_planes_of) -> torch.Tensor:
    """The model calls of one chunk of the shared mode: the frames it is the first to reach are extracted AND compensated (r_new
    [E,Hp,Wp]: the residual maps of their prior entries) into the two rings, same slot in both, then one forward at batch
    len(plan.centres) whose alignment reads the compensation ring in place.  compensate(fea, frames, rms_planes) is
    `compensate_frames` with the sequence's key and noise; rms_planes_of(entries) builds the residual planes of a list of prior
    entries (a repeated chunk only)."""
    from . import kernels as K
    dev, cap = bank.device, int(bank.shape[0])
    if plan.extract:
        fea = model.extract_features(lr_new.unsqueeze(1), p_new.unsqueeze(1))
        comp = compensate(fea, plan.compensate, r_new)
        store_frames(bank, plan.extract[0], fea)
        store_frames(comp_bank, plan.extract[0], comp)
    Lc = K.gather_frames(bank, centre_idx)

    def recompensate():
        # a rejected chunk (rare; called in the bf16x3 mode): the frames its windows hold, from the feature ring, into a
        # scratch stack -- the compensation ring keeps what later chunks will read in the sequence's own arithmetic
        prior = {t: e for w, pw in zip(plan.windows, plan.priors) for t, e in zip(w, pw)}
        need = sorted(prior)
        at = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
        fea2 = K.gather_frames(bank, at([bank_slot(t, cap) for t in need]))
        comp2 = compensate(fea2, need, rms_planes_of([prior[t] for t in need]))
        return comp2, at([need.index(w[n]) for n in NEIGHBOUR_SLOTS for w in plan.windows])

    return model.forward_windows_shared(Lc, comp_bank, comp_idx, x, m1, u, recompensate=recompensate)


def check_peak(peak) -> int:
    if isinstance(peak, bool) or not isinstance(peak, int) or not 1 <= peak <= 65535:
        raise ValueError(f"peak must be an integer in 1 .. 65535, got {peak!r}")
    return peak


def padded(H: int, W: int) -> Tuple[int, int]:
    """H, W rounded up to multiples of 8 (window attention)."""
    return (H + 7) // 8 * 8, (W + 7) // 8 * 8


def cropped(out: torch.Tensor, H: int, W: int) -> List[torch.Tensor]:
    """A chunk's padded output [K,1,4Hp,4Wp] as K frames [1,1,4H,4W]."""
    return [out[j:j + 1, :, :4 * H, :4 * W] for j in range(int(out.shape[0]))]


class PassCounters:
    """Forward seconds, and what the model's counters of extracted / compensated frames have gained since this object was made."""

    def __init__(self, model):
        self.model, self.seconds = model, 0.0
        self._extracted0, self._compensated0 = (int(getattr(model, n, 0)) for n in ("frames_extracted", "frames_compensated"))

    @property
    def frames_extracted(self) -> int:
        return int(getattr(self.model, "frames_extracted", 0)) - self._extracted0

    @property
    def frames_compensated(self) -> int:
        return int(getattr(self.model, "frames_compensated", 0)) - self._compensated0


class ChunkRunner:
    """One pass of the chunked forward (one `StreamingSR.iter_chunked` call, one `cdfo_amd.live.LiveSR` stream): all of a chunk step
    that does not depend on where the chunk's inputs come from.  It owns the feature bank [capacity,Hp,Wp,64] and, in the shared
    mode, the compensation ring beside it; a chunk's bank-side index table (`head`, `split_head`); the noise (`noise` per step,
    `frame_noise` per frame; without it the shared mode takes ONE Philox key at the pass's first chunk and frame t draws with (key,
    t) whichever chunk compensates it); the timed chunk step (`run`, between two calls of the owner's `sync`) and the counters (`count`)."""

    def __init__(self, model, dev, Hp: int, Wp: int, capacity: int, shared: bool, noise, frame_noise, sync):
        need = ("extract_features", "compensate_features", "forward_windows_shared") if shared else ("extract_features", "forward_windows")
        if not all(hasattr(model, n) for n in need):
            raise NotImplementedError(f"chunked inference needs a model with {' / '.join(need)} (CVSR_V8)")
        self.model, self.count = model, PassCounters(model)
        self.dev, self.Hp, self.Wp, self.shared, self.sync = dev, Hp, Wp, shared, sync
        self.noise, self.frame_noise, self.key = noise, frame_noise, None
        self.bank = torch.empty((capacity, Hp, Wp, 64), dtype=torch.float32, device=dev)
        self.comp_bank = torch.empty_like(self.bank) if shared else None

    @property
    def resident_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.bank, self.comp_bank) if t is not None)

    def head(self, plan: ChunkPlan) -> List[int]:
        """The bank-side table of one chunk, 7 K entries.  Unshared: the bank slots of its window stack, slot-major.  Shared: the
        [6,K] ring slots of its neighbours (`comp_slot_table`), then the ring slots of its centres."""
        cap = int(self.bank.shape[0])
        if self.shared:
            return comp_slot_table(plan, cap) + [bank_slot(i, cap) for i in plan.centres]
        return [bank_slot(w[n], cap) for n in range(NFRAMES) for w in plan.windows]

    def split_head(self, head_t, k: int):
        """`head(plan)` on the device -> (comp_idx [6,K] flat, centre_idx) in the shared mode, (lf_idx,) in the unshared one."""
        return (head_t[:6 * k], head_t[6 * k:]) if self.shared else (head_t,)

    def run(self, plan: ChunkPlan, head_t, build, rms_planes_of) -> torch.Tensor:
        """One chunk, timed into `seconds`: build() -> (x, r, u, lr_new, p_new, r_new, m1), the owner's inputs (x, r, u [7K,Hp,Wp]
        centre-major; None where the mode reads none), then `chunk_forward` / `chunk_forward_shared`, whose output it returns.
        head_t: `head(plan)` on the device, or a callable that returns it once build() has run (an owner that uploads per chunk)."""
        k = len(plan.centres)
        noise = None
        if not self.shared and self.noise is not None:      # per-step format: noise[i] = the six [1,64,H,W] draws of centre i
            per_centre = [self.noise[i] for i in plan.centres]
            noise = [torch.cat([n[d] for n in per_centre], 0) for d in range(NFRAMES - 1)]
        self.sync()
        t0 = time.perf_counter()
        with torch.no_grad(), torch.cuda.device(self.dev):
            x, r, u, lr_new, p_new, r_new, m1 = build()
            idx = self.split_head(head_t() if callable(head_t) else head_t, k)
            x, r, u = (None if t is None else t.view(k, NFRAMES, 1, self.Hp, self.Wp) for t in (x, r, u))
            if not self.shared:
                out = chunk_forward(self.model, plan, self.bank, *idx, lr_new, p_new, x, r, u, m1, noise)
            else:
                if self.key is None and self.frame_noise is None:
                    self.key = self.model.resolve_noise_key(self.dev)       # one Philox key per pass, before its first extraction
                compensate = lambda fea, frames, rm: compensate_frames(self.model, self.dev, fea, frames, rm, self.key, self.frame_noise)
                out = chunk_forward_shared(self.model, plan, self.bank, self.comp_bank, *idx, lr_new, p_new, r_new, x, u, m1, compensate,
                                           rms_planes_of)
        self.sync()
        self.count.seconds += time.perf_counter() - t0
        return out


class StreamingSR:
    """One sequence, device resident.

    lr, pms, ufs : [T,H,W] pixel planes in file units (0..255), rms : [T,H,W] residual map in file units
    (``*_res.npy[:,:,0]``), mvl0 / mvl1 : [T,H,W,3] decoder motion fields (``*_mvl0.npy``); index t = file index t.
    H, W are padded with zero rows / columns to multiples of 8 (``test_LD_37.py:24-26`` pads 270 -> 272) and the
    output is cropped back to 4H x 4W.

    gumbel_uniform: injected noise per step (T entries of six draws); frame_noise: injected noise per frame (T tensors
    [1,64,Hp,Wp]), read by ``run_chunked(share_compensation=True)`` only.

    peak: the largest sample of lr, rms and ufs, 2**depth - 1 (255: 8-bit files).  The three are divided by it, and pms, a mask that is
    8-bit at every depth, by 255: true fp32 divisions, so a sequence and its samples times 257 at peak 65535 give the same planes.

    coding: "LD" (the default: the reference's evaluation loops, `mv2mvs` on list 1 alone, mvl0 unread) or "RA" (opt-in, the project's
    own definition for a model trained on the random-access loader's field): every path builds its flows from BOTH lists with
    `mv2mvs_ra` -- past slots from list 0, future slots from list 1, a block with no reference in one list borrowing the other's
    vector negated -- at the entry the LD rule reads, followed by the same end rules; `run_chunked` builds them with
    ``kernels.seq_flows_ra``.  The model reads mvs1 only; `step` passes the one field for both arguments, as the RA loader does.

    Deliberate deviations from the reference loop: the sequence is device resident and windows are gathered by index;
    `run_chunked` extracts each frame once (same arithmetic per output frame); ``run_chunked(share_compensation=True)`` -- opt-in
    -- also compensates each neighbour frame once, with one Gumbel draw per frame where the reference draws per (step, slot).
    """

    def __init__(self, model, lr, pms, rms, ufs, mvl0, mvl1, device: Optional[torch.device] = None,
                 gumbel_uniform: Optional[Sequence] = None, use_graph: bool = False, frame_noise: Optional[Sequence] = None,
                 peak: int = 255, coding: str = "LD"):
        self.coding = check_coding(coding)
        if coding == "RA":                   # the two lists are read pixel by pixel together: judged before anything is uploaded
            check_ra_lists("StreamingSR(coding='RA')", torch.as_tensor(mvl0), torch.as_tensor(mvl1))
        dev = torch.device(device) if device is not None else next(model.parameters()).device
        if dev.type != "cuda":
            raise NotImplementedError("StreamingSR needs the model on a GPU (HIP path, no CPU fallback)")
        self.model, self.dev = model, dev
        as_dev = lambda t: torch.as_tensor(t).to(dev)
        lr = as_dev(lr)
        self.T, self.H, self.W = int(lr.shape[0]), int(lr.shape[1]), int(lr.shape[2])
        self.Hp, self.Wp = padded(self.H, self.W)
        self.peak = check_peak(peak)
        # the divisors are device tensors: with a host scalar torch's device kernel multiplies by the rounded reciprocal, which is
        # not the correctly rounded quotient the reference's CPU `/ 255.0` (test_LD_37.py:27) and the oracle loop give
        mask_peak, sample_peak = (torch.tensor(p, dtype=torch.float32, device=dev) for p in (255.0, float(peak)))

        def plane(t, divisor):               # [T,H,W] file units -> float32 / divisor, zero padded
            out = torch.zeros((self.T, self.Hp, self.Wp), dtype=torch.float32, device=dev)
            out[:, :self.H, :self.W] = as_dev(t).to(torch.float32) / divisor
            return out

        self.lr, self.pms = plane(lr, sample_peak), plane(pms, mask_peak)
        self.rms, self.ufs = plane(rms, sample_peak), plane(ufs, sample_peak)
        self.mvl0, self.mvl1 = as_dev(mvl0), as_dev(mvl1)
        self.noise = gumbel_uniform
        self.frame_noise = frame_noise
        self.fea = None
        self._pass = PassCounters(model)     # seconds and the frame counters: the current `ChunkRunner`'s once run_chunked has begun
        # use_graph: the cached-path forward (frames >= 1: identical shapes every step, ~700 kernel launches of a few
        # microseconds each at one clip) is captured once into a HIP graph and replayed from static buffers
        self.use_graph = use_graph
        self._graph = None

    def _mvs(self, mvl: torch.Tensor, i: int) -> torch.Tensor:
        m = torch.zeros((NFRAMES, 2, self.Hp, self.Wp), dtype=torch.float32, device=self.dev)
        m[:, :, :self.H, :self.W] = mv2mvs(mvl[max(1, i) if self.T > 1 else 0])
        return modify_mv_for_end_frames(i, m.unsqueeze(0), self.T)

    def _mvs_ra(self, i: int) -> torch.Tensor:
        e = max(1, i) if self.T > 1 else 0
        m = torch.zeros((NFRAMES, 2, self.Hp, self.Wp), dtype=torch.float32, device=self.dev)
        m[:, :, :self.H, :self.W] = mv2mvs_ra(self.mvl0[e], self.mvl1[e])
        return modify_mv_for_end_frames(i, m.unsqueeze(0), self.T)

    def step(self, i: int) -> torch.Tensor:
        """Super-resolve frame i (frames must be visited in order: the feature cache slides by one frame per step)."""
        if (self.fea is None) != (i == 0):
            raise ValueError("StreamingSR.step: frames must be processed in order, starting at 0")
        x, m0, m1, p, r, u = self._inputs(i)
        noise = None if self.noise is None else self.noise[i]
        if self.use_graph and i >= 1:
            return self._graph_step(x, m0, m1, p, r, u, noise)
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        with torch.no_grad():
            out, self.fea = self.model(x, m0, m1, p, r, u, self.fea, gumbel_uniform=noise)
        torch.cuda.synchronize(self.dev)
        self._pass.seconds += time.perf_counter() - t0
        return out[..., :4 * self.H, :4 * self.W]

    def _graph_step(self, x, m0, m1, p, r, u, noise):
        """Frames >= 1 from a HIP graph of the cached-path forward (cdfo_amd.graph.CapturedForward: device-side Philox key
        refreshed per replay, no range guard inside the graph -- the eager first frame of the sequence ran with it)."""
        fea = self.fea.contiguous()
        if self._graph is None:
            from .graph import CapturedForward
            self._graph = CapturedForward(self.model, x, m0, m1, p, r, u, fea, noise, check_range=False)
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        out, new_fea = self._graph(x, m0, m1, p, r, u, fea, noise)
        torch.cuda.synchronize(self.dev)
        self._pass.seconds += time.perf_counter() - t0
        self.fea = new_fea.clone()                                   # the graph's output buffers are overwritten next step
        return out[..., :4 * self.H, :4 * self.W].clone()

    def _inputs(self, i: int):
        o = generate_input_index(i, NFRAMES, self.T - 1).to(self.dev)
        po = o.clamp_min(1) if self.T > 1 else o                 # priors of frame 0 come from entry 1 (:36,53,66)
        win = lambda t, idx: t.index_select(0, idx)[None, :, None]            # [1,7,1,H,W]
        x, p, r, u = win(self.lr, o), win(self.pms, po), win(self.rms, po), win(self.ufs, po)
        if self.coding == "RA":                                  # one field for both arguments, as the RA loader hands it out
            m = self._mvs_ra(i)
            return x, m, m, p, r, u
        return x, self._mvs(self.mvl0, i), self._mvs(self.mvl1, i), p, r, u

    def run_pipelined(self) -> List[torch.Tensor]:
        """All frames in order, software-pipelined over two streams: frame i + 1's front half (the new frame's feature
        extraction, the six neighbour pipelines, temporal fusion -- launches on one to three frames that leave much of the GPU
        idle at one clip) runs beside frame i's reconstruction trunk (matrix-core bound).  Frame i + 1 only needs frame i's
        feature cache, which its front half produced.  Same kernels, same arithmetic, same noise keys in the same order as
        `run()`: the outputs are identical.  `self.fps` afterwards = frames / wall time of the whole loop (a THROUGHPUT; the
        per-frame latency is that of `run()`).  The fp16 range guard of `forward` (one host readback per call) is not part
        of this schedule, as in the graph mode."""
        if not hasattr(self.model, "forward_front"):
            raise NotImplementedError("run_pipelined needs a model with forward_front / forward_back (CVSR_V8)")
        front, back = torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev)
        cur = torch.cuda.current_stream(self.dev)
        front.wait_stream(cur)
        back.wait_stream(cur)
        outs, fea = [], None
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(self.T):
                with torch.cuda.stream(front):
                    x, m0, m1, p, r, u = self._inputs(i)
                    noise = None if self.noise is None else self.noise[i]
                    state, fea = self.model.forward_front(x, m0, m1, p, r, u, fea, gumbel_uniform=noise)
                    ready = torch.cuda.Event()
                    ready.record(front)
                with torch.cuda.stream(back):
                    back.wait_event(ready)
                    for t in state:
                        t.record_stream(back)
                    out = self.model.forward_back(state)
                    outs.append(out[..., :4 * self.H, :4 * self.W])
        torch.cuda.synchronize(self.dev)
        self._pass.seconds = time.perf_counter() - t0
        self.fea = fea
        cur.wait_stream(back)
        return outs

    def run(self) -> List[torch.Tensor]:
        """All frames in order; ``self.fps`` afterwards = frames / summed forward time (test_LD_22_FPS.py:192)."""
        self.fea, self._pass.seconds = None, 0.0
        return [self.step(i) for i in range(self.T)]

    # -- chunked inference: `chunk` consecutive centre frames per forward against a per-frame feature bank ------------------------
    def run_chunked(self, chunk: int = 8, share_compensation: bool = False) -> List[torch.Tensor]:
        """All frames in order, `chunk` centre frames per forward (the last chunk may be shorter).  Each frame goes through
        feature extraction ONCE, into a bank of at most chunk + 6 frames of features; the windows of a chunk are gathered from the
        bank in one pass and the neighbour pipelines, the fusion, the trunk and the up-sampler run at batch `chunk`
        (CVSR_V8.forward_windows).  Per output frame the arithmetic is that of `run()`.  The windows, the flows and the planes are
        built by libcdfo_hip.so (cdfo_gather_frames, cdfo_seq_flows).  ``self.seconds`` / ``fps`` cover everything a chunk does
        on the device: extraction, input building, forward.

        share_compensation=True (opt-in; False is the path above, unchanged): everything a neighbour pipeline does before the
        alignment depends on the neighbour FRAME only (fea + conv_expand_rms(rms), RDAB, conv_expand_fea_r on frame t and
        rms[max(1, t)]), so it is computed once per frame, by the chunk that extracts the frame, into a second ring of the same
        capacity and slot rule as the feature bank (CVSR_V8.compensate_features); the alignment of all six slots reads that ring
        through a [6,K] slot table (CVSR_V8.forward_windows_shared, cdfo_flow_warp_frames).  6 K pipelines per chunk become at
        most K + 6.  NOISE: one Gumbel draw per frame -- `frame_noise[t]`, or the in-kernel Philox generator with one key per
        run_chunked call and draw = t, so the result does not depend on the chunk size.  Each window still sees six draws,
        independent whenever its six neighbour frames are distinct, so away from the ends of the sequence every output frame has
        the reference's distribution; but the reference draws afresh per step and per slot, while here a frame carries ONE draw
        into every window that holds it (and into every slot of a clipped window that repeats frame 0 or T - 1): across output
        frames the draws are correlated.  That is why the mode is opt-in.  A chunk that the fp16 range guard rejects is repeated
        in bf16x3 with the compensation of its frames recomputed (same noise) into a scratch stack; the ring is not rewritten."""
        outs = []
        for centres, out in self.iter_chunked(chunk, share_compensation):
            outs.extend(cropped(out, self.H, self.W))
        return outs

    def iter_chunked(self, chunk: int = 8, share_compensation: bool = False) -> Iterator[Tuple[List[int], torch.Tensor]]:
        """`run_chunked` one chunk at a time: yields ``(centres, out)`` with `centres` the chunk's frame indices and `out` its padded
        fp32 output [len(centres),1,4Hp,4Wp] (frame j's picture is ``out[j, :, :4H, :4W]``).  A consumer that is done with a chunk
        before it asks for the next one (cdfo_amd.evaluate) never holds more than one chunk of fp32 frames.  The schedule, the
        counters and ``self.seconds`` are those of `run_chunked`, which is a list-builder over this generator."""
        check_noise_format(bool(share_compensation), self.noise, self.frame_noise, getattr(self, "T", 0))
        chunk, shared = int(chunk), bool(share_compensation)
        plans = list(plan_chunks(self.T, chunk))
        runner = ChunkRunner(self.model, self.dev, self.Hp, self.Wp, bank_capacity(self.T, chunk), shared, self.noise, self.frame_noise,
                             lambda: torch.cuda.synchronize(self.dev))
        self.fea, self._pass = None, runner.count        # (not the runner: its rings live as long as this generator, no longer)
        # every index table of the sequence in one upload: per chunk the runner's bank-side table, the frames and the prior entries
        # of its windows (centre-major) and the prior entries of the frames it extracts
        flat = []
        for p in plans:
            flat += runner.head(p) + [t for w in p.windows for t in w] + [t for w in p.priors for t in w] + p.extract_priors
        tables = torch.tensor(flat, dtype=torch.int32).to(self.dev)
        from . import kernels as K
        rms_of = lambda entries: K.gather_frames(self.rms, torch.tensor(entries, dtype=torch.int32).to(self.dev))    # a repeated chunk
        at = 0
        for p in plans:
            n7 = NFRAMES * len(p.centres)
            idx = tables[at:at + 3 * n7 + len(p.extract)]
            at += 3 * n7 + len(p.extract)
            build = lambda: self._chunk_inputs(p, shared, idx[n7:2 * n7], idx[2 * n7:3 * n7], idx[3 * n7:])
            yield p.centres, runner.run(p, idx[:n7], build, rms_of)

    def _chunk_inputs(self, plan: ChunkPlan, shared: bool, frame_idx, prior_idx, new_prior_idx):
        """`ChunkRunner.run`'s build() from the resident planes (cdfo_gather_frames, cdfo_seq_flows): the LR, residual and unfiltered
        planes of its windows, the planes of the frames it is the first to reach, its flows; residual map per new frame if `shared`."""
        from . import kernels as K
        lr_new = p_new = r_new = None
        if plan.extract:
            lr_new, p_new = self.lr[plan.extract[0]:plan.extract[-1] + 1], K.gather_frames(self.pms, new_prior_idx)
            r_new = K.gather_frames(self.rms, new_prior_idx) if shared else None
        x = K.gather_frames(self.lr, frame_idx)
        r = None if shared else K.gather_frames(self.rms, prior_idx)
        u = K.gather_frames(self.ufs, prior_idx)
        if self.coding == "RA":
            m1 = K.seq_flows_ra(self.mvl0, self.mvl1, plan.centres[0], len(plan.centres), self.Hp, self.Wp)
        else:
            m1 = K.seq_flows(self.mvl1, plan.centres[0], len(plan.centres), self.Hp, self.Wp)
        return x, r, u, lr_new, p_new, r_new, m1

    @property
    def seconds(self) -> float:
        """Summed forward time of the current pass: `run()`, `run_pipelined()` and `run_chunked()` each start it from zero."""
        return self._pass.seconds

    @property
    def frames_compensated(self) -> int:
        """Frames the model has sent through `compensate_features` since this object was made or its last `run_chunked()`
        began: T for ``run_chunked(share_compensation=True)`` (a chunk that the range guard repeats adds the frames of its windows
        once more), 0 for every other mode."""
        return self._pass.frames_compensated

    @property
    def frames_extracted(self) -> int:
        """Frames the model has sent through feature extraction since this object was made or its last `run_chunked()` began
        (one `run()`: 7 + (T - 1); `run_chunked()`: T).  It is the model's counter of eager extraction calls: exact for `run()`,
        `run_pipelined()` and `run_chunked()`; a forward that the fp16 range guard of `forward` repeats is counted twice (a repeated
        chunk is not: it reuses the bank), and replays of a HIP graph (`use_graph=True`) are not counted, only the capture is."""
        return self._pass.frames_extracted

    @property
    def fps(self) -> float:
        return self.T / self.seconds if self.seconds > 0 else float("nan")
