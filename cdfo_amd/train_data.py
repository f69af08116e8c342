"""The training set resident on the device, and training batches built by one kernel (csrc/train_batch.hip).

The reference feeds its training step from the host: ``CDVL_sideInfo_Dataset.__getitem__`` in DataLoader workers
(opt/data_LD_bi.py:139-242, one 1080p PNG decode per sample for the ground truth), ``RandomCrop(64) -> Augment -> ToTensor`` in numpy
(:245-505), eight ``.to(device)`` copies and the permutes and ``/32`` of train_LD_37.py:365-374.  ``ClipSet`` keeps S sequences of T
frames (the reference: T = 32) in HBM in the loader's storage types and builds a whole batch in one launch, with the reference's
arithmetic bit for bit (tests/golden/train_batch_ref.npz holds the real reference's outputs):

    lr, pms   uint8 [S,T,H,W]
    rms       int8  [S,T,H,W]
    ufs       uint8 [S,T,Hu,W], Hu >= H   (the reference's unfiltered planes have 272 rows beside 270; rows are indexed from the top)
    mvl0      int8  [S,T,H,W,3]           components (a, b, ref)
    hr        uint8 [S,T,4H,4W]           66 MB per 32-frame 1080p sequence (32 x 1080 x 1920 bytes)

A set has a coding, the reference's two training configurations.  ``"LD"`` (low delay, opt/data_LD_bi.py; the default) stores no
``mvl1``: that loader's ``Augment`` returns an all-zero ``mvl1s_7`` (:473-489), so ``batch`` hands out one cached zero tensor for it.
``"RA"`` (random access, opt/data_RA_bi.py) also stores

    mvl1      int8  [S,T,H,W,3]           the second reference list's field

and builds the flow field from both lists (:495-533): list 0 feeds slots 0-2, list 1 slots 4-6, and each stands in for the other where
a block has no reference in it (a reference component of -99).  That loader sets ``mvl1s_7 = mvl0s_7``, so ``batch`` returns ONE tensor
as ``mvs0`` and ``mvs1``.  Everything else -- planes, plans, draw ranges -- is the same in both codings (tests/golden/
train_batch_ra_ref.npz holds the real RA loader's outputs).

A batch is described by a host plan, int32 [B,8], rows ``(seq, first, top, left, hflip, vflip, rot, 0)``: ``draw`` and ``epoch`` make
plans with the reference's distribution (not its RNG streams), ``batch`` validates a plan on the host, uploads it and launches."""
from __future__ import annotations

import os
from typing import Iterator, Sequence, Tuple

import numpy as np
import torch

from . import kernels as K
from .priors import load_sequence, read_gray_png

FRAMES = 7


def _clip_i8(a: np.ndarray) -> np.ndarray:
    """The loader's ``np.clip(., -128, 127).astype(np.int8)`` (opt/data_LD_bi.py:91, 102)."""
    return np.clip(a, -128, 127).astype(np.int8)


class ClipSet:
    def __init__(self, lr, pms, rms, ufs, mvl0, hr, mvl1=None):
        """Device tensors in the storage types of the module docstring (see `from_arrays` / `from_directories`); ``mvl1`` makes the
        set a random-access one."""
        self.lr, self.pms, self.rms, self.ufs, self.mvl0, self.hr, self.mvl1 = lr, pms, rms, ufs, mvl0, hr, mvl1
        self.coding = "LD" if mvl1 is None else "RA"
        self.S, self.T, self.H, self.W = (int(v) for v in lr.shape)
        self._zero_flows = {}

    def __len__(self) -> int:
        return self.S

    @classmethod
    def from_arrays(cls, lr, pms, rms, ufs, mvl0, hr, device="cuda", *, mvl1=None, coding="LD") -> "ClipSet":
        """numpy arrays [S,T,...] -> a resident set.  Residuals and motion fields are clipped to int8 as the reference loader clips
        them; the 8-bit planes must be uint8.  Shapes are checked against ``lr`` before anything is uploaded.  ``coding="RA"`` needs
        ``mvl1`` (clipped and shaped like ``mvl0``), ``coding="LD"`` takes none."""
        if coding not in ("LD", "RA"):
            raise ValueError(f"coding is 'LD' or 'RA', got {coding!r}")
        if (coding == "RA") != (mvl1 is not None):
            raise ValueError("coding='RA' needs mvl1" if coding == "RA" else "coding='LD' stores no mvl1: pass coding='RA' with it")
        lr, pms, ufs, hr = (np.asarray(a) for a in (lr, pms, ufs, hr))
        if lr.ndim != 4 or lr.shape[1] < FRAMES:
            raise ValueError(f"lr must be [S,T,H,W] with T >= {FRAMES}, got {lr.shape}")
        S, T, H, W = lr.shape
        rms, mvl0 = _clip_i8(np.asarray(rms)), _clip_i8(np.asarray(mvl0))
        lists = (("mvl0", mvl0),) if mvl1 is None else (("mvl0", mvl0), ("mvl1", _clip_i8(np.asarray(mvl1))))
        for name, a in (("lr", lr), ("pms", pms), ("ufs", ufs), ("hr", hr)):
            if a.dtype != np.uint8:
                raise ValueError(f"{name} must be uint8, got {a.dtype}")
        for name, a, shape in (("pms", pms, (S, T, H, W)), ("rms", rms, (S, T, H, W)), *((n, a, (S, T, H, W, 3)) for n, a in lists),
                               ("hr", hr, (S, T, 4 * H, 4 * W))):
            if a.shape != shape:
                raise ValueError(f"{name} is {a.shape}, the LR frames {lr.shape} need {shape}")
        if ufs.ndim != 4 or ufs.shape[:2] != (S, T) or ufs.shape[3] != W or ufs.shape[2] < H:
            raise ValueError(f"ufs is {ufs.shape}, the LR frames {lr.shape} need ({S}, {T}, >= {H}, {W})")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
        return cls(up(lr), up(pms), up(rms), up(ufs), up(mvl0), up(hr), *(up(a) for _, a in lists[1:]))

    @classmethod
    def from_directories(cls, sequences: Sequence[Tuple[str, str, str]], device="cuda", *, coding="LD") -> "ClipSet":
        """``[(lr_dir, side_dir, hr_dir), ...]``: the layout of cdfo_amd/priors.py, every frame with its OWN prior files (the training
        loader reads ``00000_*`` too; a missing one is an error naming it), plus ``<hr_dir>/%05d.png``, 8-bit grey, 4H x 4W.  All
        sequences must have one shape.  ``coding="RA"`` keeps the ``mvl1`` files' fields too."""
        if coding not in ("LD", "RA"):
            raise ValueError(f"coding is 'LD' or 'RA', got {coding!r}")
        cols = {k: [] for k in ("lr", "pms", "rms", "ufs", "mvl0", "hr") + (("mvl1",) if coding == "RA" else ())}
        for lr_dir, side_dir, hr_dir in sequences:
            seq = load_sequence(lr_dir, side_dir, own_frame0=True)
            seq["hr"] = np.stack([read_gray_png(os.path.join(hr_dir, "%05d.png" % t)) for t in range(len(seq["lr"]))])
            for k in cols:
                if cols[k] and cols[k][0].shape != seq[k].shape:
                    raise ValueError(f"{lr_dir}: {k} is {seq[k].shape}, the first sequence's is {cols[k][0].shape}")
                cols[k].append(seq[k])
        if not cols["lr"]:
            raise ValueError("no sequences given")
        return cls.from_arrays(*(np.stack(cols[k]) for k in ("lr", "pms", "rms", "ufs", "mvl0", "hr")), device=device,
                               mvl1=np.stack(cols["mvl1"]) if coding == "RA" else None, coding=coding)

    # ------------------------------------------------------------------------------------------------------------------ plans
    def draw(self, B: int, rng: np.random.Generator, crop: int = 64, seqs=None) -> np.ndarray:
        """A plan of B samples with the reference's draw ranges, quirks included: ``first`` uniform in 0 .. T-7 (``randint(0, 25)`` at
        T = 32, bounds inclusive), ``top`` in 0 .. H-crop-1 and ``left`` in 0 .. W-crop-1 (``np.random.randint``'s bound is exclusive, so
        the last position is never drawn), each flag with probability 1/2.  ``seqs``: the sequence of each sample (default: uniform)."""
        if crop >= self.H or crop >= self.W:
            raise ValueError(f"crop {crop} leaves no origin to draw in {self.H}x{self.W} frames (the reference draws from [0, size - crop))")
        plan = np.zeros((B, 8), np.int32)
        plan[:, 0] = rng.integers(0, self.S, B) if seqs is None else seqs
        plan[:, 1] = rng.integers(0, self.T - FRAMES + 1, B)
        plan[:, 2] = rng.integers(0, self.H - crop, B)
        plan[:, 3] = rng.integers(0, self.W - crop, B)
        plan[:, 4:7] = rng.random((B, 3)) < 0.5
        return plan

    def epoch(self, batch_size: int, rng: np.random.Generator, crop: int = 64) -> Iterator[np.ndarray]:
        """Plans that cover one permutation of the sequences, each once; the last may be short (``shuffle=True, drop_last=False``)."""
        order = rng.permutation(self.S)
        for i in range(0, self.S, batch_size):
            yield self.draw(len(order[i:i + batch_size]), rng, crop, seqs=order[i:i + batch_size])

    def check_plan(self, plan, crop: int) -> np.ndarray:
        """The plan as int32 [B,8], or ValueError: indices in range, ``top + crop <= H`` and ``left + crop <= W`` (the far corner is
        allowed in an explicit plan), flags 0 or 1, ``crop`` a positive multiple of 4."""
        p = np.asarray(plan)
        if p.ndim != 2 or p.shape[1] != 8 or p.shape[0] == 0 or not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f"a plan is an integer array [B,8] with B >= 1, got {p.dtype} {p.shape}")
        if crop <= 0 or crop % 4:
            raise ValueError(f"crop must be a positive multiple of 4, got {crop}")
        p = p.astype(np.int64)
        ok = ((p[:, 0] >= 0) & (p[:, 0] < self.S) & (p[:, 1] >= 0) & (p[:, 1] + FRAMES <= self.T) & (p[:, 2] >= 0) &
              (p[:, 2] + crop <= self.H) & (p[:, 3] >= 0) & (p[:, 3] + crop <= self.W) &
              ((p[:, 4:7] == 0) | (p[:, 4:7] == 1)).all(axis=1))
        if not ok.all():
            b = int(np.flatnonzero(~ok)[0])
            raise ValueError(f"plan row {b} = {p[b].tolist()} does not fit {self.S} sequences of {self.T} frames of {self.H}x{self.W} at "
                             f"crop {crop}")
        return np.ascontiguousarray(p.astype(np.int32))

    # ---------------------------------------------------------------------------------------------------------------- batches
    def batch(self, plan, crop: int = 64):
        """(x, mvs0, mvs1, pms, rms, ufs, hr), fp32 and dense, in the shapes train_LD_37.py:365-377 hands to the model and the loss:
        x, pms [B,7,1,c,c]; mvs0, mvs1 [B,7,2,c,c]; rms, ufs [B,1,7,c,c]; hr [B,1,4c,4c].  One launch.  In an LD set ``mvs1`` is a
        cached zero tensor shared by every batch of its shape; in an RA set ``mvs1`` IS ``mvs0`` (the reference's two fields are equal
        there, train_RA_37.py:383-386).  Callers must not write into either."""
        p = self.check_plan(plan, crop)
        B = p.shape[0]
        if self.coding == "RA":
            with K.on_device(self.lr):
                x, mvs, pms, rms, ufs, hr = K.train_batch_ra(self.lr, self.pms, self.rms, self.ufs, self.mvl0, self.mvl1, self.hr,
                                                             torch.from_numpy(p).to(self.lr.device), crop)
            return x, mvs, mvs, pms, rms, ufs, hr
        with K.on_device(self.lr):
            x, mvs0, pms, rms, ufs, hr = K.train_batch(self.lr, self.pms, self.rms, self.ufs, self.mvl0, self.hr,
                                                       torch.from_numpy(p).to(self.lr.device), crop)
            if (B, crop) not in self._zero_flows:
                self._zero_flows[(B, crop)] = torch.zeros((B, FRAMES, 2, crop, crop), dtype=torch.float32, device=self.lr.device)
        return x, mvs0, self._zero_flows[(B, crop)], pms, rms, ufs, hr


def synthetic_arrays(S: int, T: int, H: int, W: int, seed: int = 0, coding: str = "LD"):
    """Random content for tools and tests that have no data set at hand, as (lr, pms, rms, ufs, mvl0, hr) for `ClipSet.from_arrays`:
    a smooth scene per sequence that drifts by a whole HR pixel per frame, its x4 area mean plus noise as the LR frames, block-constant
    motion with a reference distance of -2, -1 or 1 (never 0: the flows stay finite), unfiltered planes of H + 2 rows.
    ``coding="RA"`` returns a seventh array, ``mvl1`` (for ``from_arrays(*six, mvl1=mvl1, coding="RA")``): block-constant like
    ``mvl0``, and a block in eight is marked -99 in list 0, one in list 1 and one in both; the other distances stay non-zero.  The
    first six arrays of a seed do not depend on the coding except for list 0's markers."""
    if coding not in ("LD", "RA"):
        raise ValueError(f"coding is 'LD' or 'RA', got {coding!r}")
    rs = np.random.RandomState(seed)
    lr, hr = np.zeros((S, T, H, W), np.uint8), np.zeros((S, T, 4 * H, 4 * W), np.uint8)
    for s in range(S):
        coarse = rs.rand((4 * H + T) // 8 + 2, (4 * W + T) // 8 + 2)
        scene = np.kron(coarse, np.ones((8, 8)))
        scene = (scene + np.roll(scene, 3, 0) + np.roll(scene, 3, 1) + np.roll(scene, (5, 5), (0, 1))) / 4.0
        for t in range(T):
            f = scene[t:t + 4 * H, t:t + 4 * W]
            hr[s, t] = np.round(f * 255.0)
            small = f.reshape(H, 4, W, 4).mean(axis=(1, 3)) * 255.0 + rs.randn(H, W) * 2.0
            lr[s, t] = np.clip(np.round(small), 0, 255)
    hb, wb = (H + 7) // 8, (W + 7) // 8
    mv = rs.randint(-64, 64, (S, T, hb, wb, 3))
    mv[..., 2] = rs.choice([-2, -1, 1], size=(S, T, hb, wb))
    mvl0 = np.repeat(np.repeat(mv, 8, axis=2), 8, axis=3)[:, :, :H, :W]
    six = (lr, rs.randint(0, 256, (S, T, H, W)).astype(np.uint8), np.round(rs.randn(S, T, H, W) * 6),
           rs.randint(0, 256, (S, T, H + 2, W)).astype(np.uint8), mvl0, hr)
    if coding == "LD":
        return six
    mv1 = rs.randint(-64, 64, (S, T, hb, wb, 3))                 # drawn after everything the LD call draws
    mv1[..., 2] = rs.choice([-2, -1, 1], size=(S, T, hb, wb))
    mark = rs.randint(0, 8, (S, T, hb, wb))                      # 1: list 0 has no reference, 2: list 1, 3: neither has
    mv[..., 2][(mark == 1) | (mark == 3)] = -99
    mv1[..., 2][(mark == 2) | (mark == 3)] = -99
    block = lambda a: np.repeat(np.repeat(a, 8, axis=2), 8, axis=3)[:, :, :H, :W]      # noqa: E731
    return six[:4] + (block(mv), hr, block(mv1))
