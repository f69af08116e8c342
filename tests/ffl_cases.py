"""The cases and the bound of the focal frequency loss tests (tests/test_ffl_cpu.py, test_gpu_ffl_kernels.py, test_gpu_ffl_loss.py).

Shapes: every transform length 16 .. 512 on each axis with the other at 16 -- below the width of a column tile, and at H = 512 the
narrower tile -- and four shapes with more than one tile, strip and row group each way.  Per shape four cases: "random-n1", "-n3"
and "-n5", N frames of uniform samples where frame 1 has its difference scaled by 0.01 (the maximum is per frame) and frame 2 has
sr == hr in bits; and "patterns", five frames whose difference is a single cosine, a constant, (-1)^x, (-1)^y and an impulse
(|F| flat: every w = 1), on a random hr.

The bound.  Nothing is taken on faith: the floor of a shape is the same statement on the same fp32 inputs run in float32 --
torch.fft in complex64 on the CPU -- against the float64 statement, measured when the test runs on the shape's random cases (the
largest figure over their nine frames and, for loss and gradient, over ALPHAS; the frames with sr == hr have nothing to measure and
are left out.  The loss of a frame is ONE number, so its fp32 error is one draw that can come out small by luck, and it does come
out differently on different hosts' torch builds; the largest of some twenty draws does not).  Every case of the shape is held to
16 x that floor, the margin the LPIPS tests have over the same kind of floor: a radix-2 schedule with fused multiply-adds may sit a
few times above a library's mixed-radix floor; a wrong stage, twiddle or index is wrong by O(1).  Spectrum: max |F - F64| over the frame's max |F64|.  Loss: |l - l64| / l64.  Gradient: max |g - g64| over the frame's
max |g64|, the upstream gradient included.  Where the reference is exactly zero the device must be, too."""
import functools

import numpy as np
import torch

import ffl_ref as ref

LENGTHS = (16, 32, 64, 128, 256, 512)
SHAPES = tuple([(16, w) for w in LENGTHS] + [(h, 16) for h in LENGTHS[1:]] + [(32, 128), (128, 32), (64, 64), (256, 256)])
COUNTS = (1, 3, 5)
ALPHAS = (1.0, 0.0, 0.5)
RANDOM = tuple("random-n%d" % n for n in COUNTS)
KINDS = RANDOM + ("patterns",)
MARGIN = 16.0
CASES = tuple((h, w, kind) for h, w in SHAPES for kind in KINDS)


def case_id(c) -> str:
    return "%dx%d-%s" % c


@functools.lru_cache(maxsize=None)
def case(h: int, w: int, kind: str):
    """(sr, hr) fp32 [N,H,W], read-only."""
    rs = np.random.RandomState(1000 * h + w + 7 * KINDS.index(kind))
    if kind in RANDOM:
        n = COUNTS[RANDOM.index(kind)]
        hr = rs.uniform(0, 1, (n, h, w)).astype(np.float32)
        sr = rs.uniform(0, 1, (n, h, w)).astype(np.float32)
        if n > 1:
            sr[1] = hr[1] + np.float32(0.01) * (sr[1] - hr[1])
        if n > 2:
            sr[2] = hr[2]
    else:
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        d = np.zeros((5, h, w))
        d[0] = 0.3 * np.cos(2 * np.pi * (3 * y / h + 5 * x / w))
        d[1] = 0.25
        d[2] = 0.2 * (-1.0) ** x
        d[3] = 0.15 * (-1.0) ** y
        d[4, h // 3, w // 5] = 0.5
        hr = rs.uniform(0, 1, (5, h, w)).astype(np.float32)
        sr = (hr + d).astype(np.float32)
    sr.setflags(write=False)
    hr.setflags(write=False)
    return sr, hr


def upstream(n: int) -> np.ndarray:
    """A non-unit upstream gradient per frame."""
    return (0.5 + 0.75 * np.arange(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(h: int, w: int, kind: str, alpha: float):
    """(F complex128 [N,H,W], loss fp64 [N], g fp64 [N,H,W] with `upstream` applied) of the fp64 statement, as numpy, read-only."""
    sr, hr = case(h, w, kind)
    d = ref.difference(sr, hr)
    F = ref.spectrum(d).numpy()
    loss = ref.statement(d, alpha).numpy()
    g = ref.gradient(d, alpha).numpy() * upstream(d.shape[0]).astype(np.float64)[:, None, None]
    for a in (F, loss, g):
        a.setflags(write=False)
    return F, loss, g


def spectrum_err(F, F64) -> np.ndarray:
    """Per frame: max |F - F64| / max |F64|; a frame whose F64 is all zero gives 0 if F is, else inf."""
    top = np.abs(F64).max(axis=(1, 2))
    e = np.abs(np.asarray(F).astype(np.complex128) - F64).max(axis=(1, 2))
    return _relative(e, top)


def loss_err(loss, loss64) -> np.ndarray:
    return _relative(np.abs(np.asarray(loss).astype(np.float64) - loss64), np.abs(loss64))


def grad_err(g, g64) -> np.ndarray:
    top = np.abs(g64).max(axis=(1, 2))
    return _relative(np.abs(np.asarray(g).astype(np.float64) - g64).max(axis=(1, 2)), top)


def _relative(e, top):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(top > 0, e / top, np.where(e == 0, 0.0, np.inf))


@functools.lru_cache(maxsize=None)
def floors(h: int, w: int):
    """(spectrum, loss, gradient): the float32 statement against the float64 one on the shape's random cases.  Never 0."""
    fs = fl = fg = 0.0
    for kind in RANDOM:
        d = ref.difference(*case(h, w, kind))
        live = np.array([bool(f.any()) for f in d.numpy()])
        up = upstream(d.shape[0])
        fs = max(fs, spectrum_err(ref.spectrum(d, torch.float32).numpy(), ref.spectrum(d).numpy())[live].max())
        for alpha in ALPHAS:
            _, l64, g64 = reference(h, w, kind, alpha)
            fl = max(fl, loss_err(ref.statement(d, alpha, torch.float32).numpy(), l64)[live].max())
            g32 = ref.gradient(d, alpha, torch.float32).numpy() * up[:, None, None]
            fg = max(fg, grad_err(g32, g64)[live].max())
    assert fs > 0 and fl > 0 and fg > 0, (fs, fl, fg)
    return float(fs), float(fl), float(fg)
