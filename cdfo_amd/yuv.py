"""Raw 8-bit YUV 4:2:0 sequences (planar I420, the format of the HEVC test material and of a decoder's output): per frame W*H luma
bytes, then (W/2)*(H/2) U bytes, then (W/2)*(H/2) V bytes; no header, so width and height come from the caller and must be even.

``YuvReader`` maps a file and hands out array VIEWS of its planes (nothing is read until a view is touched, never the whole file);
``YuvWriter`` appends frames in order.  ``load_sequence_yuv`` is ``priors.load_sequence`` with the LR luma (and chroma) taken from
such a file; the coding priors keep the reference's directory layout (cdfo_amd/priors.py).  Host side only: numpy, no torch.

``pix_fmt`` (ffmpeg's names, `parse_pix_fmt`) selects other planar layouts: 4:0:0 (luma only), 4:2:0 and 4:4:4 at 8, 10, 12 or 16 bits.
Above 8 bits a sample is two bytes, little-endian, the value in the low bits, and the planes are ``<u2`` views.  The default,
``yuv420p``, is the 8-bit I420 described above."""
from __future__ import annotations

import mmap
import os
import re
from typing import Dict, NamedTuple, Optional

import numpy as np

from .priors import load_priors


class PixFmt(NamedTuple):
    name: str
    depth: int                  # bits of a sample: 8, 10, 12, 16
    chroma: str                 # "400" (no chroma planes), "420", "444"
    sample_bytes: int           # 1, or 2 (little-endian, the value in the low bits)
    peak: int                   # 2**depth - 1

    @property
    def dtype(self) -> np.dtype:
        return np.dtype(np.uint8 if self.sample_bytes == 1 else "<u2")

    def chroma_shape(self, height: int, width: int):
        """(h, w) of a chroma plane of a height x width frame; None for 4:0:0."""
        return {"400": None, "420": (height // 2, width // 2), "444": (height, width)}[self.chroma]


_PIX_FMT = re.compile(r"(gray|yuv420p|yuv444p)(?:(10|12|16)le)?")


def parse_pix_fmt(name) -> PixFmt:
    """ffmpeg's name of a planar format -> its description.  ``gray``, ``yuv420p``, ``yuv444p`` (8 bits) and their ``10le``, ``12le``,
    ``16le`` forms; anything else (4:2:2, packed and semi-planar layouts, big-endian samples) is a ValueError."""
    if isinstance(name, PixFmt):
        return name
    m = _PIX_FMT.fullmatch(name) if isinstance(name, str) else None
    if m is None:
        raise ValueError(f"unsupported pixel format {name!r}: gray, yuv420p, yuv444p and their 10le / 12le / 16le forms are")
    depth = int(m.group(2) or 8)
    return PixFmt(name, depth, {"gray": "400", "yuv420p": "420", "yuv444p": "444"}[m.group(1)], 1 if depth == 8 else 2, 2 ** depth - 1)


def frame_bytes(width: int, height: int, pix_fmt="yuv420p") -> int:
    """Bytes of one frame (by default I420); ValueError unless width and height are positive and, for 4:2:0, even."""
    fmt = parse_pix_fmt(pix_fmt)
    if isinstance(width, bool) or isinstance(height, bool) or not isinstance(width, (int, np.integer)) \
            or not isinstance(height, (int, np.integer)) or width <= 0 or height <= 0 \
            or (fmt.chroma == "420" and (width % 2 or height % 2)):
        if fmt.chroma == "420":
            raise ValueError(f"4:2:0 frames need a positive even width and height, got {width!r} x {height!r}")
        raise ValueError(f"{fmt.name} frames need a positive width and height, got {width!r} x {height!r}")
    c = fmt.chroma_shape(int(height), int(width))
    return (int(width) * int(height) + (2 * c[0] * c[1] if c else 0)) * fmt.sample_bytes


class YuvReader:
    """A memory-mapped I420 file of ``frames`` frames of ``width`` x ``height``.  ``y(t)`` / ``u(t)`` / ``v(t)``: frame t's plane, a
    read-only uint8 view [H,W] / [H/2,W/2]; ``y(t0, t1)`` etc.: the planes of frames t0 .. t1-1, a view [t1-t0,H,W] whose frame stride
    is the file's.  ValueError for odd sizes, an empty file and a file that is not a whole number of frames.  ``pix_fmt``: the
    views are ``<u2`` above 8 bits, the chroma planes are [H,W] for 4:4:4, and ``u`` / ``v`` of a 4:0:0 file raise ValueError."""

    def __init__(self, path: str, width: int, height: int, pix_fmt="yuv420p"):
        self.pix_fmt = fmt = parse_pix_fmt(pix_fmt)
        fb = frame_bytes(width, height, fmt)
        size = os.path.getsize(path)
        if size == 0 or size % fb:
            raise ValueError(f"{path}: {size} bytes is not a whole number (>= 1) of {width}x{height} "
                             f"{'4:2:0' if fmt.name == 'yuv420p' else fmt.name} frames of {fb} bytes")
        self.path, self.width, self.height, self.frames = path, int(width), int(height), size // fb
        W, H, T, S = self.width, self.height, self.frames, fmt.sample_bytes
        with open(path, "rb") as f:
            self._map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        plane = lambda off, h, w: np.ndarray((T, h, w), dtype=fmt.dtype, buffer=self._map, offset=off * S, strides=(fb, w * S, S))
        self._planes = dict(y=plane(0, H, W))
        c = fmt.chroma_shape(H, W)
        if c is not None:
            self._planes.update(u=plane(W * H, *c), v=plane(W * H + c[0] * c[1], *c))

    def _view(self, name: str, t: int, stop: Optional[int]) -> np.ndarray:
        if name not in self._planes and self.pix_fmt.chroma == "400":
            raise ValueError(f"{self.path}: a {self.pix_fmt.name} file has no {name} plane")
        if stop is None:
            if not 0 <= t < self.frames:
                raise IndexError(f"frame {t} of {self.frames}")
            return self._planes[name][t]
        if not 0 <= t <= stop <= self.frames:
            raise IndexError(f"frames {t}:{stop} of {self.frames}")
        return self._planes[name][t:stop]

    def y(self, t: int, stop: Optional[int] = None) -> np.ndarray:
        return self._view("y", t, stop)

    def u(self, t: int, stop: Optional[int] = None) -> np.ndarray:
        return self._view("u", t, stop)

    def v(self, t: int, stop: Optional[int] = None) -> np.ndarray:
        return self._view("v", t, stop)

    def close(self) -> None:
        """Drop the views (arrays handed out earlier keep the mapping alive for as long as they live)."""
        self._planes = {}
        self._map = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class YuvWriter:
    """Appends I420 frames of ``width`` x ``height`` to a new file, in the order of the ``append(y, u, v)`` calls (uint8 arrays
    [H,W], [H/2,W/2], [H/2,W/2], any memory layout).  ``pix_fmt``: uint16 arrays above 8 bits (written little-endian), chroma planes
    [H,W] for 4:4:4, and ``append(y)`` alone for 4:0:0."""

    def __init__(self, path: str, width: int, height: int, pix_fmt="yuv420p"):
        self.pix_fmt = parse_pix_fmt(pix_fmt)
        frame_bytes(width, height, self.pix_fmt)
        self.path, self.width, self.height, self.frames = path, int(width), int(height), 0
        self._f = open(path, "wb", buffering=0)

    def append(self, y: np.ndarray, u: Optional[np.ndarray] = None, v: Optional[np.ndarray] = None) -> None:
        H, W, fmt = self.height, self.width, self.pix_fmt
        c = fmt.chroma_shape(H, W)
        if c is None:
            if u is not None or v is not None:
                raise ValueError(f"a {fmt.name} frame has no u and v planes")
            planes = (("y", y, (H, W)),)
        else:
            if u is None or v is None:
                raise ValueError(f"a {fmt.name} frame needs its u and v planes")
            planes = (("y", y, (H, W)), ("u", u, c), ("v", v, c))
        kind = np.uint8 if fmt.sample_bytes == 1 else np.uint16
        for name, a, shape in planes:
            if a.dtype != kind or a.shape != shape:
                raise ValueError(f"{name} plane must be {np.dtype(kind).name} {shape}, got {a.dtype} {a.shape}")
        for _, a, _ in planes:
            data = memoryview(np.ascontiguousarray(a, dtype=fmt.dtype)).cast("B")
            while len(data):                            # an unbuffered write may be partial
                data = data[self._f.write(data):]
        self.frames += 1

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load_sequence_yuv(lr_yuv: str, width: int, height: int, side_dir: str, pix_fmt="yuv420p") -> Dict[str, np.ndarray]:
    """``priors.load_sequence`` for an LR sequence in an I420 file: lr [T,H,W] from the file's luma, pms, rms, ufs, mvl0, mvl1 from
    ``side_dir`` (the reference's layout, read by `priors.load_priors`), plus the LR chroma u, v uint8 [T,H/2,W/2].  A raw file has
    no header: a wrong ``width`` / ``height`` shows as a frame count or a plane size the priors do not have, a ValueError.
    ``pix_fmt``: the planes in the format's dtype (uint8, or uint16 above 8 bits); a 4:0:0 file gives no u and v."""
    with YuvReader(lr_yuv, width, height, pix_fmt) as r:
        T = r.frames
        lr = np.array(r.y(0, T))
        chroma = dict(u=np.array(r.u(0, T)), v=np.array(r.v(0, T))) if r.pix_fmt.chroma != "400" else {}
    masks = [n for n in os.listdir(os.path.join(side_dir, "part_m")) if n.endswith("_M_mask.png")]
    if len(masks) != max(1, T - 1):          # the priors of frame 0 are frame 1's: files 00001 .. T-1
        raise ValueError(f"{lr_yuv} holds {T} frames of {width}x{height}, which need {max(1, T - 1)} partition maps; "
                         f"{os.path.join(side_dir, 'part_m')} holds {len(masks)}")
    seq = load_priors(side_dir, T, lr.shape, r.pix_fmt.depth)
    return dict(lr=lr, **seq, **chroma)
