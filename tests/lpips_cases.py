"""The LPIPS tests' shared cases: the nets, the frame pairs and, measured once per process on the CPU from the statement alone
(tests/lpips_ref.py), the fp32 floor -- how far the statement with an fp32 trunk is from the fp64 one.  The device tests bound the
device's deviation from the fp64 statement by 16 x this floor; nothing here ever looks at a device result."""
import functools

import numpy as np
import torch

import lpips_ref as ref

NARROW = (16, 32, 48, 64, 64)
TRUE = (64, 128, 256, 512, 512)

# name: (widths, model seed, result size, ground-truth size, frames, frame seed)
CASES = {
    "narrow-16x16": (NARROW, 11, (16, 16), (16, 16), 3, 1),
    "narrow-37x53": (NARROW, 11, (37, 53), (37, 53), 3, 2),
    "true-32x32": (TRUE, 12, (32, 32), (32, 32), 1, 3),
    "narrow-40x64-vs-37x70": (NARROW, 11, (40, 64), (37, 70), 2, 4),
}


@functools.lru_cache(maxsize=None)
def model(widths, seed):
    from cdfo_amd import metrics as M
    return M.lpips_random_params(widths, seed)


def frames(sr_size, gt_size, n, seed):
    """(sr, gt) uint8 [n,h,w] stacks: the ground truth a blocky random field, the result the same content (over the larger of the two
    canvases) with noise of up to 24 levels, clipped."""
    rs = np.random.RandomState(seed)
    H, W = max(sr_size[0], gt_size[0]), max(sr_size[1], gt_size[1])
    coarse = rs.randint(0, 256, (n, (H + 3) // 4, (W + 3) // 4))
    canvas = np.repeat(np.repeat(coarse, 4, axis=1), 4, axis=2)[:, :H, :W] // 2 + rs.randint(0, 128, (n, H, W))
    gt = np.clip(canvas, 0, 255).astype(np.uint8)
    sr = np.clip(canvas + rs.randint(-24, 25, (n, H, W)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(sr[:, :sr_size[0], :sr_size[1]]), np.ascontiguousarray(gt[:, :gt_size[0], :gt_size[1]])


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, sr, gt, fp64 layers [n,5], fp32-trunk layers [n,5]) of a case; the arrays are shared and read-only."""
    widths, mseed, sr_size, gt_size, n, fseed = CASES[name]
    params = model(widths, mseed)
    sr, gt = frames(sr_size, gt_size, n, fseed)
    want = np.stack([ref.layers(sr[j], gt[j], params) for j in range(n)])
    floor = np.stack([ref.layers(sr[j], gt[j], params, trunk_dtype=torch.float32) for j in range(n)])
    for a in (sr, gt, want, floor):
        a.setflags(write=False)
    return params, sr, gt, want, floor


def rel(got, want) -> float:
    """The worst relative difference of two arrays of positive figures."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.abs(want)).max())


def totals(layers) -> np.ndarray:
    return np.array([ref.total(row) for row in np.atleast_2d(layers)])


@functools.lru_cache(maxsize=None)
def floors():
    """(worst per-layer relative fp32 floor, worst floor of the total) over every case."""
    per_layer = max(rel(case(n)[4], case(n)[3]) for n in CASES)
    tot = max(rel(totals(case(n)[4]), totals(case(n)[3])) for n in CASES)
    return per_layer, tot


@functools.lru_cache(maxsize=None)
def stem_case(name):
    """(params, sr frames, fp64 ReLU(conv1_1) [n,h,w,C0], the fp32 statement's worst distance from it as a fraction of the largest
    value) of a case's result frames."""
    params, sr, _, _, _ = case(name)
    want = np.stack([ref.stem(f, params).permute(1, 2, 0).numpy() for f in sr])
    f32 = np.stack([ref.stem(f, params, dtype=torch.float32).permute(1, 2, 0).numpy() for f in sr])
    return params, sr, want, float(np.abs(f32 - want).max() / np.abs(want).max())
