"""File readers of the reference's evaluation loop: the 8-bit grey PNG frames and coding priors and
the NPY residual / motion-vector dumps that ``test_LD_22_FPS.py:20-97,155-176`` (= ``train_LD_37.py:56-126``) reads frame
by frame with ``cv2.imread(path, 0)`` and ``np.load``.  Here a sequence is read ONCE into uint8 / int arrays that
``cdfo_amd.streaming.StreamingSR`` uploads and keeps resident in HBM; the ``/255``, the 270 -> 272 zero padding
(``:24-26``) and the seven-frame window gathering happen on the device.

``cv2`` is not available in this image, so the PNG decoder is a small stdlib one (zlib + the five PNG row filters) for
the formats the data set uses: 8-bit greyscale (colour type 0; an alpha channel is dropped), non-interlaced; and 16-bit greyscale
of the same kinds (samples big-endian in the file, uint16 here), which a decoder at 10 or more bits writes its unfiltered planes as.

Directory layout and the reference's naming (``test_LD_22_FPS.py:143-170``):
    <lr_dir>/<any sorted file names>.png                      LR luma frames, index i = position in the sorted list
    <side_dir>/part_m/%05d_M_mask.png   partition maps        (index max(1, i): the priors of frame 0 are frame 1's)
    <side_dir>/res/%05d_res.npy         residual maps, [:,:,0]
    <side_dir>/unfiltered/%05d_unflt.png
    <side_dir>/mvl0/%05d_mvl0.npy, <side_dir>/mvl1/%05d_mvl1.npy     decoder motion fields [H,W,3]"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Dict

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"


def read_gray_png(path: str) -> np.ndarray:
    """8-bit greyscale PNG -> uint8 [H,W] (what ``cv2.imread(path, 0)`` returns for such a file); 16-bit greyscale -> uint16 [H,W]."""
    data = open(path, "rb").read()
    if data[:8] != _SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if hdr is None:
        raise ValueError(f"{path}: no IHDR chunk")
    W, H, depth, ctype, _, _, interlace = hdr
    if depth not in (8, 16) or ctype not in (0, 4) or interlace:
        raise NotImplementedError(f"{path}: only 8- and 16-bit non-interlaced greyscale PNGs are supported "
                                  f"(bit depth {depth}, colour type {ctype}, interlace {interlace})")
    bpp = (1 if ctype == 0 else 2) * (depth // 8)          # the filters run over bytes, a pixel apart
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    stride = W * bpp
    if raw.size != H * (stride + 1):
        raise ValueError(f"{path}: truncated image data")
    rows = raw.reshape(H, stride + 1)
    out = np.zeros((H, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    for y in range(H):
        f, line = int(rows[y, 0]), rows[y, 1:]
        if f == 0:
            cur = line.copy()
        elif f == 2:                                           # Up
            cur = line + prev
        elif f == 1:                                           # Sub: running sum along the row, per byte lane
            cur = line.copy()
            for c in range(bpp):
                cur[c::bpp] = np.cumsum(line[c::bpp], dtype=np.uint64).astype(np.uint8)
        elif f in (3, 4):                                      # Average / Paeth: sequential in x
            cur = np.empty(stride, dtype=np.uint8)
            ln, pv = line.tolist(), prev.tolist()
            res = [0] * stride
            for x in range(stride):
                a = res[x - bpp] if x >= bpp else 0
                b = pv[x]
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    c = pv[x - bpp] if x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                res[x] = (ln[x] + pred) & 255
            cur[:] = res
        else:
            raise ValueError(f"{path}: bad filter type {f} in row {y}")
        out[y] = cur
        prev = cur
    if depth == 16:                                        # big-endian samples; with alpha, every second one
        return out.view(">u2")[:, ::bpp // 2].astype(np.uint16)
    return out[:, ::bpp].copy() if bpp == 2 else out


def write_gray_png(path: str, img: np.ndarray, filter_type: int = 0, level: int = 6) -> None:
    """uint8 [H,W] -> 8-bit greyscale PNG with every row filtered by ``filter_type`` (0-4), deflated at zlib ``level``.  Filter 0
    (the default, what the evaluation loop writes) is one array operation; the other filters, for tests and tools, go row by row.
    uint16 [H,W] -> a 16-bit greyscale PNG: the same over the rows' big-endian bytes, a pixel two bytes apart."""
    depth = 16 if np.asarray(img).dtype == np.uint16 else 8
    if depth == 16:
        H, W = img.shape
        img = np.ascontiguousarray(img, dtype=">u2").view(np.uint8)      # [H, 2W] bytes
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        H, W = img.shape
    if filter_type == 0:
        packed = np.zeros((H, img.shape[1] + 1), dtype=np.uint8)    # each row: its filter byte (0), then the pixels
        packed[:, 1:] = img
        raw = packed.tobytes()
    else:
        raw = _filtered_rows(img, filter_type, depth // 8)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(_SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b""))


def _filtered_rows(img: np.ndarray, filter_type: int, bpp: int = 1) -> bytes:
    """The rows of `img` (bytes, a pixel ``bpp`` of them apart) under PNG filter 1-4 (Sub, Up, Average, Paeth), each behind its
    filter byte."""
    H, W = img.shape
    rows = bytearray()
    prev = np.zeros(W, dtype=np.int32)
    for y in range(H):
        cur = img[y].astype(np.int32)
        left = np.concatenate([[0] * bpp, cur[:-bpp]])
        ul = np.concatenate([[0] * bpp, prev[:-bpp]])
        if filter_type == 1:
            enc = cur - left
        elif filter_type == 2:
            enc = cur - prev
        elif filter_type == 3:
            enc = cur - ((left + prev) >> 1)
        else:
            p = left + prev - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
            enc = cur - pred
        rows.append(filter_type)
        rows += (enc & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(rows)


def load_priors(side_dir: str, T: int, shape=None, depth: int = 8, own_frame0: bool = False) -> Dict[str, np.ndarray]:
    """The coding priors of a sequence of T frames: pms uint8, ufs uint8 or (16-bit PNGs) uint16 [T,H,W]; rms [T,H,W] (dtype of the
    ``*_res.npy`` files); mvl0, mvl1 [T,H,W,3].  Entry 0 (which the reference never reads: ``ii = max(1, i)``) repeats entry 1.  ``shape``: the (T,H,W) of the
    LR frames the planes must have, else ValueError.  ``depth``: the bit depth of the sequence's samples; the unfiltered planes must
    be 8-bit PNGs at depth 8 and 16-bit PNGs above it, and the partition maps 8-bit at every depth, else ValueError (a plane of the
    wrong depth would be divided by the wrong peak without a sound).  ``own_frame0``: entry 0 is read from the ``00000_*`` files, as the
    reference's TRAINING loader reads them (opt/data_LD_bi.py:74-118: every frame its own files); a missing one is then a
    FileNotFoundError that names it.  The unfiltered planes of that layout may have more rows than the LR frames (272 beside 270)."""

    def per_frame(fn):
        if own_frame0:
            return np.stack([fn("%05d" % t) for t in range(T)])
        items = [fn("%05d" % max(1, t)) for t in range(T)] if T > 1 else [fn("%05d" % 1)]
        return np.stack(items)

    def png(part, suffix, want, what):                   # every file on its own: stacking would widen a stray 8-bit plane
        def read(i):
            img = read_gray_png(os.path.join(side_dir, part, i + suffix))
            if img.dtype != want:
                raise ValueError(f"{os.path.join(side_dir, part, i + suffix)}: a {8 * img.dtype.itemsize}-bit PNG; {what}")
            return img
        return per_frame(read)

    pms = png("part_m", "_M_mask.png", np.uint8, "partition maps are 8-bit masks at every depth")
    ufs = png("unfiltered", "_unflt.png", np.uint8 if depth == 8 else np.uint16,
              f"the unfiltered planes of a sequence of {depth}-bit samples are {'8' if depth == 8 else '16'}-bit PNGs")
    rms = per_frame(lambda i: np.load(os.path.join(side_dir, "res", i + "_res.npy"))[:, :, 0])
    mvl0 = per_frame(lambda i: np.load(os.path.join(side_dir, "mvl0", i + "_mvl0.npy")))
    mvl1 = per_frame(lambda i: np.load(os.path.join(side_dir, "mvl1", i + "_mvl1.npy")))
    if shape is not None:
        for name, arr in (("pms", pms), ("ufs", ufs), ("rms", rms)):
            taller = own_frame0 and name == "ufs" and arr.shape[1] > shape[1] and arr.shape[::2] == tuple(shape)[::2]
            if arr.shape != tuple(shape) and not taller:
                raise ValueError(f"{name} planes are {arr.shape[1:]} but the LR frames are {tuple(shape)[1:]}")
    return dict(pms=pms, rms=rms, ufs=ufs, mvl0=mvl0, mvl1=mvl1)


def load_sequence(lr_dir: str, side_dir: str, own_frame0: bool = False) -> Dict[str, np.ndarray]:
    """One sequence of the reference's test layout -> the arrays ``StreamingSR`` takes:
    lr, pms, ufs uint8 [T,H,W]; rms [T,H,W] (dtype of the ``*_res.npy`` files); mvl0, mvl1 [T,H,W,3].
    Index t = file index t; entry 0 of the priors (which the reference never reads: ``ii = max(1, i)``) repeats entry 1, unless
    ``own_frame0`` asks for the ``00000_*`` files (`load_priors`)."""
    names = sorted(n for n in os.listdir(lr_dir) if n.lower().endswith(".png"))
    if not names:
        raise FileNotFoundError(f"no PNG frames in {lr_dir}")
    lr = np.stack([read_gray_png(os.path.join(lr_dir, n)) for n in names])
    if lr.dtype != np.uint8:
        raise NotImplementedError(f"{lr_dir}: only 8-bit LR frames are supported in the PNG layout, these are {lr.dtype} "
                                  f"(high bit depth goes through raw files: cdfo_amd/yuv.py)")
    return dict(lr=lr, **load_priors(side_dir, len(names), lr.shape, own_frame0=own_frame0))
