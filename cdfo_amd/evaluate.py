"""Evaluation of one sequence end to end: the reference's ``eval_seq`` (test_LD_37.py:115-206) on the chunked path.

The reference, per frame: forward, ``torch.clamp(out,0,1).numpy() * 255.0`` with ``astype(np.uint8)`` (``:179-180``: an fp32 multiply,
then TRUNCATION), ``cv2.imwrite`` under the LR frame's file name; afterwards ``cal_psnr_ssim`` (psnr_ssim.py:446-484) reads the PNGs back
and logs the sequence's mean PSNR / SSIM against ``<gt>/%05d.png``, both cropped to (min_height, min_width), border 4.

Here one chunk loop, `_run_chunks`, serves ``evaluate_sequence`` (8-bit gray PNG directories, the reference's layout) and
``evaluate_yuv`` (raw planar files of cdfo_amd/yuv.py: 4:0:0, 4:2:0 and 4:4:4 at 8, 10, 12 or 16 bits, one format for the LR file, the
ground truth and the result).  The two are adapters: they check their arguments, build a frame SOURCE for the ground truth (frame
count, plane shapes, sample dtype and peak, and "stage frame t into these numpy views", which runs in the pool: `_PngSource` decodes a
file, `_YuvSource` copies out of a memory map) and a frame SINK for the result (`_PngSink`: one PNG per frame under the LR file's name,
in any order; `_YuvSink`: chunks appended to one file in frame order), call the loop and turn its integer sums into PSNR.

The loop, per chunk of ``StreamingSR.iter_chunked``, on the device: ``cdfo_finish_frames`` turns the padded fp32 output into cropped
8- or 16-bit frames and sums the squared differences against the ground truth in the same pass (exact integers), the SSIM kernel sums
the map of those frames, and the chroma planes, which never pass through the model, are upsampled x4 from the LR file's by
``cdfo_chroma_up4``, with their sums.  Above 8 bits the buffers are uint16, `StreamingSR` divides by the format's peak 2**depth - 1 and
the three kernels are their 16-bit forms with that peak.  Every buffer the loop owns exists TWICE
(`_Slots`) and chunk c works in slot c % 2.  Up: the pool stages chunk c + 1's ground truth into pinned buffers during chunk c's forward,
from where it is uploaded without blocking; a slot's pinned buffers are staged again only after the event behind that upload.  Down:
the frames go to the host on a copy stream into pinned buffers and the sink's pool tasks write them while the next forward runs; a
slot's device buffers are written again only after the event behind that copy, its pinned buffers only after the sink's tasks.  So
nothing relies on the allocator's stream bookkeeping, no fp32 output frame outlives its chunk, and the memory held does not depend
on the sequence's length.  ``msssim=True`` adds the luma's five-scale MS-SSIM (`metrics.msssim_components`)
on the frames SSIM runs on; its pyramid scratch exists once, the launch stream orders its use.  ``niqe=`` a pristine model adds the
reference's no-reference metric (metric/cal_VideoLQ.py scores every output frame with metric/niqe.py) on the chunk's 8-bit luma, with or
without ground truth (`metrics.niqe_features_u8`): seven launches behind ``cdfo_finish_frames`` on the main
stream, no wait for the device; the scores are formed on the host after the last chunk.  ``brisque=`` a support-vector model adds the
reference's other live no-reference figure (metric/brisque.py) the same way (`metrics.brisque_features_u8`, DESIGN.md section
5.00000000000000): seven launches of its own per chunk, 36 features per frame kept on the device until the last chunk.  ``tof=True``
adds the reference's temporal-consistency figure tOF (metric/psnr_ssim.py: calculate_tOF) with ground truth on 8-bit luma: the
Farneback flows of the chunk's ground-truth pairs and result pairs go through the same launches behind BRISQUE's
(`metrics.tof_frames_u8`), the frame in front of the chunk carried on the device.  ``lpips=`` a
model adds LPIPS, the learned perceptual distance to the ground truth, on 8-bit luma (`metrics.lpips_layers_u8`, DESIGN.md section
5.0000000000000000): a VGG-shaped trunk in fp32 behind tOF's launches, five layer values per frame kept on the device until the last chunk.
Above 8 bits those four are a ValueError unless ``evaluate_yuv(..., rescale_metrics=True)``: then the same launches run on the uint16
luma with the format's peak, a sample v read as 255 v / peak (LPIPS: v / peak), the ``metrics.*_u16`` forms (DESIGN.md section
5.000000000000000000).

Deliberate deviation: ``cal_psnr_ssim`` sends single-channel frames through ``to_y_channel``, an fp32 ``/255*255`` round
trip, and takes fp32 means.  The metric semantics here are the project's established ones, ``oracle/metrics_ref.py``: fp64 on the
integers."""
from __future__ import annotations

import concurrent.futures as cf
import os
import struct
import time
from types import SimpleNamespace
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kernels as K
from . import metrics as M
from .priors import load_sequence, read_gray_png, write_gray_png
from .streaming import StreamingSR, check_coding
from .yuv import YuvReader, YuvWriter, load_sequence_yuv, parse_pix_fmt

MAX_WORKERS = 16


_NO_FRAMES = np.zeros(0, np.float64)               # the default of the result tuples' trailing arrays: one object, so read-only
_NO_FRAMES.setflags(write=False)


class SequenceResult(NamedTuple):
    psnr: np.ndarray            # fp64 [T] (empty without ground truth)
    ssim: np.ndarray            # fp64 [T] (empty without ground truth)
    mean_psnr: float            # nan without ground truth
    mean_ssim: float
    frames: int
    seconds_forward: float      # StreamingSR.seconds: everything the chunks do on the device up to their fp32 output
    seconds_total: float        # the whole call: reading the files, the forwards, metrics, downloads, PNG encoding
    msssim: np.ndarray = _NO_FRAMES                 # fp64 [T] with ``msssim=True`` and ground truth, else empty
    mean_msssim: float = float("nan")
    niqe: np.ndarray = _NO_FRAMES                   # fp64 [T] with ``niqe=`` a model (ground truth or not), else empty
    mean_niqe: float = float("nan")
    brisque: np.ndarray = _NO_FRAMES                # fp64 [T] with ``brisque=`` a model (ground truth or not), else empty
    mean_brisque: float = float("nan")
    tof: np.ndarray = _NO_FRAMES                    # fp64 [T] with ``tof=True`` (needs ground truth), else empty
    mean_tof: float = float("nan")
    lpips: np.ndarray = _NO_FRAMES                  # fp64 [T] with ``lpips=`` a model (needs ground truth), else empty
    mean_lpips: float = float("nan")


def format_log(result: SequenceResult, name: str) -> str:
    """The reference's log line (psnr_ssim.py:481); with MS-SSIM figures, `` MS-SSIM: %.5f`` behind it, with NIQE figures
    `` NIQE: %.5f`` behind that, with BRISQUE figures `` BRISQUE: %.5f``, with tOF figures `` tOF: %.5f``, with LPIPS figures `` LPIPS: %.5f`` last."""
    return '%s Average PSNR/SSIM: %.3f/%.5f' % (name, result.mean_psnr, result.mean_ssim) + _msssim_suffix(result) + _niqe_suffix(result) + \
        _brisque_suffix(result) + _tof_suffix(result) + _lpips_suffix(result)


def _msssim_suffix(result) -> str:
    return ' MS-SSIM: %.5f' % result.mean_msssim if len(result.msssim) else ''


def _niqe_suffix(result) -> str:
    return ' NIQE: %.5f' % result.mean_niqe if len(result.niqe) else ''


def _brisque_suffix(result) -> str:
    return ' BRISQUE: %.5f' % result.mean_brisque if len(result.brisque) else ''


def _tof_suffix(result) -> str:
    return ' tOF: %.5f' % result.mean_tof if len(result.tof) else ''


def _lpips_suffix(result) -> str:
    return ' LPIPS: %.5f' % result.mean_lpips if len(result.lpips) else ''


def quantise_numpy(x: np.ndarray, mode: str = "trunc", peak: int = 255) -> np.ndarray:
    """The numpy statement of ``kernels.finish_frames``: clip to [0,1] (NaN -> 0), fp32 * 255, truncation or round-to-nearest-even.
    On finite values ``mode="trunc"`` is ``(np.clip(x, 0, 1) * 255.0).astype(np.uint8)``, the reference's writer.  ``peak``: the
    multiplier in place of 255 (1 .. 65535); uint16 comes back above 255."""
    if isinstance(peak, bool) or not isinstance(peak, (int, np.integer)) or not 1 <= peak <= 65535:
        raise ValueError(f"peak must be an integer in 1 .. 65535, got {peak!r}")
    v = np.asarray(x, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    v = np.clip(v, np.float32(0), np.float32(1)) * np.float32(peak)
    if mode == "nearest":
        v = np.rint(v)
    elif mode != "trunc":
        raise ValueError(f"quantise must be 'trunc' or 'nearest', got {mode!r}")
    return v.astype(np.uint8 if peak <= 255 else np.uint16)


def metric_region(h_out: int, w_out: int, h_gt: int, w_gt: int, crop: int):
    """(Hm, Wm, rows, columns): the common size of result and ground truth (psnr_ssim.py:462-468) and what is left of it inside
    the ``crop`` border, the pixels PSNR runs over (SSIM's map is 10 smaller each way)."""
    hm, wm = M.common_size(h_out, w_out, h_gt, w_gt)
    return hm, wm, hm - 2 * crop, wm - 2 * crop


def _check_args(workers, quantise, chunk) -> Tuple[int, int]:
    if not isinstance(workers, int) or not 1 <= workers <= MAX_WORKERS:
        raise ValueError(f"workers must be an integer between 1 and {MAX_WORKERS}, got {workers!r}")
    if quantise not in K.QUANT_MODES:
        raise ValueError(f"quantise must be one of {sorted(K.QUANT_MODES)}, got {quantise!r}")
    if int(chunk) < 1:
        raise ValueError(f"chunk >= 1 expected, got {chunk}")
    return workers, int(chunk)


def _inside(shape, gt_shape, crop: int) -> Tuple[int, int]:
    """(rows, columns) PSNR runs over: the x4 result of LR planes of ``shape`` against ground truth of ``gt_shape``, less the border."""
    return metric_region(4 * shape[0], 4 * shape[1], *gt_shape, crop)[2:]


def _check_regions(lr, gt, crop_border: int, ccrop: int) -> None:
    if min(_inside(lr.shape, gt.shape, crop_border)) <= 10:
        raise ValueError(f"crop_border {crop_border} leaves no SSIM window in the common {min(4 * lr.shape[0], gt.shape[0])} x "
                         f"{min(4 * lr.shape[1], gt.shape[1])} of result and ground truth")
    if lr.chroma_shape is not None and min(_inside(lr.chroma_shape, gt.chroma_shape, ccrop)) <= 0:
        raise ValueError(f"crop_border {crop_border} leaves nothing of the chroma planes")


def _check_msssim(lr, gt, crop_border: int) -> None:
    """MS-SSIM's five scales need `metrics.msssim_min_size` samples each way inside the border (ValueError, naming the size)."""
    M.msssim_region(4 * lr.shape[0], 4 * lr.shape[1], *gt.shape, crop_border)


def _check_niqe(lr, niqe, rescale_metrics: bool = False):
    """The pristine model of a ``niqe=`` argument (None: the metric is off), before any device work: `metrics.niqe_params`' checks;
    ValueError above 8 bits (the reference defines the metric on 0 .. 255 integers) and for x4 frames below one 96 x 96 block.
    ``rescale_metrics``: no error above 8 bits, where the loop then runs the metric's 16-bit form (`evaluate_yuv`)."""
    if niqe is None:
        return None
    params = niqe if isinstance(niqe, M.NiqeParams) else M.niqe_params(niqe)
    if lr.dtype != torch.uint8 and not rescale_metrics:
        raise ValueError(f"niqe: the metric is defined on 8-bit samples, the format's peak is {lr.peak}")
    M.niqe_region(4 * lr.shape[0], 4 * lr.shape[1])
    return params


def _niqe(features: np.ndarray, params) -> np.ndarray:
    """Per-frame NIQE from the loop's features; empty where it has none."""
    return np.atleast_1d(M.niqe_from_features(features, params)) if len(features) else np.zeros(0, np.float64)


def _check_brisque(lr, brisque, rescale_metrics: bool = False):
    """The model of a ``brisque=`` argument (None: the metric is off), before any device work: `metrics.brisque_params`' checks;
    ValueError above 8 bits (the reference defines the metric on 0 .. 255 integers) and for x4 frames below 16 x 16.
    ``rescale_metrics``: as `_check_niqe`'s."""
    if brisque is None:
        return None
    params = brisque if isinstance(brisque, M.BrisqueParams) else M.brisque_params(brisque)
    if lr.dtype != torch.uint8 and not rescale_metrics:
        raise ValueError(f"brisque: the metric is defined on 8-bit samples, the format's peak is {lr.peak}")
    M.brisque_size(4 * lr.shape[0], 4 * lr.shape[1])
    return params


def _brisque(features: np.ndarray, params) -> np.ndarray:
    """Per-frame BRISQUE from the loop's features; empty where it has none."""
    return np.atleast_1d(M.brisque_from_features(features, params)) if len(features) else np.zeros(0, np.float64)


def _check_tof(lr, gt, tof, rescale_metrics: bool = False) -> bool:
    """Whether tOF runs, before any device work: ValueError without ground truth, above 8 bits (the reference computes the flow of
    8-bit images) and for a common region below 32 x 32 (`metrics.tof_size`).  ``rescale_metrics``: as `_check_niqe`'s."""
    if not tof:
        return False
    if gt is None:
        raise ValueError("tof: the metric compares the result's flow with the ground truth's, and there is no ground truth")
    if lr.dtype != torch.uint8 and not rescale_metrics:
        raise ValueError(f"tof: the metric is defined on 8-bit samples, the format's peak is {lr.peak}")
    M.tof_size(min(4 * lr.shape[0], gt.shape[0]), min(4 * lr.shape[1], gt.shape[1]))
    return True


def _check_lpips(lr, gt, lpips, rescale_metrics: bool = False):
    """The model of an ``lpips=`` argument (None: the metric is off), before any device work: `metrics.lpips_params`' checks;
    ValueError without ground truth, above 8 bits and for a common region below 16 x 16 (`metrics.lpips_size`).
    ``rescale_metrics``: as `_check_niqe`'s."""
    if lpips is None:
        return None
    if gt is None:
        raise ValueError("lpips: the metric is a distance to the ground truth, and there is no ground truth")
    if lr.dtype != torch.uint8 and not rescale_metrics:
        raise ValueError(f"lpips: the metric is defined on 8-bit samples, the format's peak is {lr.peak}")
    M.lpips_size(min(4 * lr.shape[0], gt.shape[0]), min(4 * lr.shape[1], gt.shape[1]))
    return M.lpips_params(lpips)


def _lpips(layers: np.ndarray) -> np.ndarray:
    """Per-frame LPIPS from the loop's layer values; empty where it has none."""
    return np.atleast_1d(M.lpips_from_layers(layers)) if len(layers) else np.zeros(0, np.float64)


def _psnr(sse: np.ndarray, shape, gt_shape, crop: int, peak: int) -> np.ndarray:
    """Per-frame PSNR from the loop's integer sums; empty where it has none (no ground truth, no chroma)."""
    return M.psnr_from_sse(sse, int(np.prod(_inside(shape, gt_shape, crop))), peak) if len(sse) else np.zeros(0, np.float64)


def _mean(a: np.ndarray) -> float:
    return float(a.sum() / len(a)) if len(a) else float("nan")      # psnr / frames, as the reference accumulates


class _PngSource:
    """A frame source: a directory of 8-bit gray PNGs, frame t in the file ``names[t]`` (by default the directory's PNGs in
    `load_sequence`'s order).  The plane shape is that of frame 0, read from its header."""
    chroma_shape, dtype, peak = None, torch.uint8, 255

    def __init__(self, directory: str, names: Optional[List[str]] = None):
        self.directory = directory
        self.names = sorted(n for n in os.listdir(directory) if n.lower().endswith(".png")) if names is None else names
        if not self.names:
            raise FileNotFoundError(f"no PNG frames in {directory}")
        self.frames = len(self.names)
        with open(os.path.join(directory, self.names[0]), "rb") as f:
            header = f.read(24)
        if len(header) < 24 or header[12:16] != b"IHDR":
            raise ValueError(f"{os.path.join(directory, self.names[0])}: not a PNG file")
        W, H = struct.unpack(">II", header[16:24])
        self.shape = (H, W)

    def stage(self, t: int, y: np.ndarray) -> None:
        g = read_gray_png(os.path.join(self.directory, self.names[t]))
        if g.shape != self.shape:
            raise ValueError(f"ground-truth frame {t} is {g.shape}, frame 0 is {self.shape}")
        y[...] = g


class _YuvSource:
    """A frame source: the planes of an open `YuvReader`."""

    def __init__(self, reader: YuvReader):
        fmt = reader.pix_fmt
        self.reader, self.frames, self.shape = reader, reader.frames, (reader.height, reader.width)
        self.chroma_shape = fmt.chroma_shape(reader.height, reader.width)
        self.dtype, self.peak = torch.uint8 if fmt.sample_bytes == 1 else torch.uint16, fmt.peak

    def stage(self, t: int, y: np.ndarray, u: Optional[np.ndarray] = None, v: Optional[np.ndarray] = None) -> None:
        """Frame t of the mapped file into its places in a pinned buffer (the page faults of the map happen here, in the pool); u and
        v None: a 4:0:0 file."""
        np.copyto(y, self.reader.y(t))
        if u is not None:
            np.copyto(u, self.reader.u(t))
            np.copyto(v, self.reader.v(t))


class _PngSink:
    """A frame sink: frame t as an 8-bit PNG ``<save_dir>/<names[t]>``, one pool task per frame, in any order."""

    def __init__(self, save_dir: str, names: List[str], level: int):
        os.makedirs(save_dir, exist_ok=True)
        self.save_dir, self.names, self.level = save_dir, names, level

    def _write(self, copied, path: str, frame: np.ndarray) -> None:
        copied.synchronize()                    # the chunk's download into the pinned buffer `frame` is a view of
        write_gray_png(path, frame, 0, self.level)

    def __call__(self, pool, copied, centres, y: np.ndarray, c: Optional[np.ndarray]) -> List[cf.Future]:
        return [pool.submit(self._write, copied, os.path.join(self.save_dir, self.names[t]), y[j]) for j, t in enumerate(centres)]


class _YuvSink:
    """A frame sink: the chunks appended to a `YuvWriter` in the order they are handed in, one pool task per chunk."""

    def __init__(self, writer: YuvWriter):
        self.writer, self.last = writer, None

    def _append(self, before: Optional[cf.Future], copied, y: np.ndarray, c: Optional[np.ndarray]) -> None:
        """Append a chunk (y [k,Ho,Wo]; c [2k,Hc,Wc], its U planes then its V planes; None: 4:0:0) once the chunk before it is in the
        file and its own download into the pinned buffers `y` and `c` are views of has completed."""
        if before is not None:
            before.result()
        copied.synchronize()
        k = len(y)
        for j in range(k):
            if c is None:
                self.writer.append(y[j])
            else:
                self.writer.append(y[j], c[j], c[k + j])

    def __call__(self, pool, copied, centres, y: np.ndarray, c: Optional[np.ndarray]) -> List[cf.Future]:
        self.last = pool.submit(self._append, self.last, copied, y, c)
        return [self.last]


class _Slots:
    """Two alternating sets of buffers with an event each.  Chunk c works in slot c % 2 and records the slot's event behind the
    asynchronous copy that reads (uploads) or fills (downloads) the slot's buffers; chunk c + 2 may touch them once that event, and
    whatever the pool still does with them (`futures`), has completed."""

    def __init__(self):
        self._two = [SimpleNamespace(event=torch.cuda.Event(), futures=[]) for _ in range(2)]

    def __getitem__(self, c: int) -> SimpleNamespace:
        return self._two[c % 2]

    def add(self, make, **shapes) -> None:
        """name=(n, plane shape): a buffer ``make((n, *shape))`` of that name in each slot; None where the shape is None (planes this
        run does not have)."""
        for slot in self._two:
            for name, (n, shape) in shapes.items():
                setattr(slot, name, None if shape is None else make((n, *shape)))


def _run_chunks(lr, load, gt, sink, chunk: int, share_compensation: bool, crop: int, ccrop: int, quantise: str, workers: int,
                msssim: bool = False, niqe: bool = False, brisque: bool = False, tof: bool = False, lpips=None):
    """The chunk loop of both evaluators.  ``lr``: the LR sequence as a frame source (its counts, shapes, dtype and peak; its frames
    come from ``load``).  ``load()`` -> (`StreamingSR`, (u, v) LR chroma planes [T,h,w] or None); it runs after the first
    ground-truth reads have been handed to the pool.  ``gt``: a frame source or None.  ``sink``: a frame sink or None.
    ``msssim``: with ground truth, `metrics.msssim_components` on the frames SSIM runs on, on the main stream; its pyramid scratch
    exists once (every call that writes or reads it is on that stream, which orders them).  ``niqe``: `metrics.niqe_features_u8` on the
    chunk's 8-bit luma, with or without ground truth, on the main stream too, its scratch held the same way; like SSIM's sums the
    features stay on the device until the last chunk.  ``brisque``: `metrics.brisque_features_u8` likewise, behind NIQE's launches.
    ``tof``: with ground truth, `metrics.tof_frames_u8` behind those, its scratch held once as well; the last ground-truth frame and
    the last result frame of a chunk are copied into two one-frame buffers, the next chunk's first pair.  ``lpips``: an
    `metrics.LpipsParams` or None; with ground truth, `metrics.lpips_layers_u8` behind tOF's launches, its scratch held once too.
    -> (the `StreamingSR`, sse_y int64 [T], sse_uv int64 [2,T], ssim fp64 [T], MS-SSIM components fp64 [T,5,2], NIQE features fp64
    [T,nb,36], BRISQUE features fp64 [T,36], tOF fp64 [T], LPIPS layer values fp64 [T,5]); the arrays are empty without ground truth
    (sse_uv without chroma, the components without ``msssim``, tOF without ``tof``, the layer values without ``lpips``), the features
    without ``niqe`` / ``brisque``.  Above 8 bits (``lr.dtype`` uint16, which the callers' checks let through with
    ``rescale_metrics`` only) those four run their ``_u16`` forms with ``lr.peak`` on the same scratch; tOF's carried frames are
    uint16 then.  The module's docstring has the order of events."""
    T, kmax, kind, peak = lr.frames, min(chunk, lr.frames), lr.dtype, lr.peak
    has_c = lr.chroma_shape is not None
    out_y, out_c = (shape and (4 * shape[0], 4 * shape[1]) for shape in (lr.shape, lr.chroma_shape))      # None stays None
    gt_y, gt_c = (gt.shape, gt.chroma_shape) if gt is not None else (None, None)
    pinned = lambda shape: torch.empty(shape, dtype=kind).pin_memory()
    with cf.ThreadPoolExecutor(max_workers=workers) as pool:
        up, down = _Slots(), _Slots()
        up.add(pinned, gt_y=(kmax, gt_y), gt_c=(2 * kmax, gt_c))

        def stage(c: int) -> List[cf.Future]:
            """Hand chunk c's ground-truth reads to the pool: they fill the pinned buffers of slot c."""
            up[c].event.synchronize()                   # chunk c - 2 has left the pinned upload buffers of slot c
            t0, k = c * chunk, max(0, min(chunk, T - c * chunk))
            if gt is None or k == 0:
                return []
            y, uv = up[c].gt_y.numpy(), up[c].gt_c.numpy() if has_c else None
            return [pool.submit(gt.stage, t0 + j, y[j], *((uv[j], uv[k + j]) if has_c else ())) for j in range(k)]

        reads = stage(0)
        s, lr_c = load()
        dev = s.dev
        with torch.cuda.device(dev):
            main, copy = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
            on_dev = lambda shape: torch.empty(shape, dtype=kind, device=dev)
            up.add(pinned, lr_c=(2 * kmax, lr.chroma_shape))
            up.add(on_dev, lr_c_dev=(2 * kmax, lr.chroma_shape), gt_y_dev=(kmax, gt_y), gt_c_dev=(2 * kmax, gt_c))
            down.add(on_dev, y=(kmax, out_y), c=(2 * kmax, out_c))
            if sink is not None:
                down.add(pinned, host_y=(kmax, out_y), host_c=(2 * kmax, out_c))
            sse_y, sse_c, ssim, ms = [], [], [], []
            ms_scratch = None
            if msssim and gt is not None:
                ms_scratch = M.msssim_scratch(kmax, *M.msssim_region(*out_y, *gt_y, crop), dev)
            nq, nq_scratch = [], M.niqe_scratch(kmax, *M.niqe_region(*out_y), dev) if niqe else None
            bq, bq_scratch = [], M.brisque_scratch(kmax, *out_y, dev) if brisque else None
            tf, tf_scratch, tf_gt, tf_sr = [], None, None, None
            if tof and gt is not None:
                tf_scratch = M.tof_scratch(2 * kmax, min(out_y[0], gt_y[0]), min(out_y[1], gt_y[1]), dev)
                tf_carry = (on_dev(gt_y), on_dev(out_y))          # the frames in front of the next chunk: ground truth, result
            lp, lp_scratch = [], None
            if lpips is not None and gt is not None:
                lp_scratch = M.lpips_scratch(kmax, min(out_y[0], gt_y[0]), min(out_y[1], gt_y[1]), lpips, dev)
            chunks = s.iter_chunked(chunk, share_compensation)
            for c in range((T + chunk - 1) // chunk):
                u, d = up[c], down[c]
                mine, reads = reads, stage(c + 1)       # the next chunk's frames: decoded or copied during this chunk's forward
                centres, out = next(chunks)
                k = len(centres)
                for f in d.futures:                     # chunk c - 2 is out of the pinned result buffers (raises what a writer raised)
                    f.result()
                main.wait_event(d.event)                # ... and out of the device result buffers
                src_c = gy = gc = None
                if has_c:                               # (stage(c) has seen chunk c - 2 leave this pinned buffer too)
                    planes = u.lr_c.numpy()
                    planes[:k], planes[k:2 * k] = (p[centres[0]:centres[0] + k] for p in lr_c)
                    src_c = u.lr_c_dev[:2 * k]
                    src_c.copy_(u.lr_c[:2 * k], non_blocking=True)
                if gt is not None:
                    for f in mine:
                        f.result()
                    gy = u.gt_y_dev[:k]
                    gy.copy_(u.gt_y[:k], non_blocking=True)
                    if has_c:
                        gc = u.gt_c_dev[:2 * k]
                        gc.copy_(u.gt_c[:2 * k], non_blocking=True)
                u.event.record(main)                    # the launch stream orders the reuse of the device upload buffers
                y8, e = K.finish_frames(out, s.H, s.W, gt=gy, crop=crop, mode=quantise, dst=d.y[:k], peak=peak)
                del out                                 # the chunk's fp32 frames end here
                c8 = ec = None
                if has_c:
                    c8, ec = K.chroma_up4(src_c, gt=gc, crop=ccrop, dst=d.c[:2 * k], peak=peak)
                if gt is not None:
                    sse_y.append(e)
                    if has_c:
                        sse_c.append(ec.view(2, k))
                    ssim.append(M.ssim_u8(y8, gy, crop) if kind == torch.uint8 else M.ssim_u16(y8, gy, crop, peak))
                    if ms_scratch is not None:
                        ms.append(M.msssim_components(y8, gy, crop, None if kind == torch.uint8 else peak, ms_scratch))
                if nq_scratch is not None:
                    nq.append(M.niqe_features_u8(y8, nq_scratch) if kind == torch.uint8 else M.niqe_features_u16(y8, peak, nq_scratch))
                if bq_scratch is not None:
                    bq.append(M.brisque_features_u8(y8, bq_scratch) if kind == torch.uint8 else
                              M.brisque_features_u16(y8, peak, bq_scratch))
                if tf_scratch is not None:
                    tf.append(M.tof_frames_u8(gy, y8, tf_gt, tf_sr, tf_scratch) if kind == torch.uint8 else
                              M.tof_frames_u16(gy, y8, peak, tf_gt, tf_sr, tf_scratch))
                    tf_gt, tf_sr = tf_carry
                    tf_gt.copy_(gy[k - 1])
                    tf_sr.copy_(y8[k - 1])
                if lp_scratch is not None:
                    lp.append(M.lpips_layers_u8(y8, gy, lpips, lp_scratch) if kind == torch.uint8 else
                              M.lpips_layers_u16(y8, gy, peak, lpips, lp_scratch))
                if sink is not None:
                    ready = torch.cuda.Event()
                    ready.record(main)
                    copy.wait_event(ready)
                    with torch.cuda.stream(copy):
                        d.host_y[:k].copy_(y8, non_blocking=True)
                        if has_c:
                            d.host_c[:2 * k].copy_(c8, non_blocking=True)
                        d.event.record(copy)
                    d.futures = sink(pool, d.event, centres, d.host_y.numpy()[:k], d.host_c.numpy()[:2 * k] if has_c else None)
            for f in down[0].futures + down[1].futures:
                f.result()
            main.wait_stream(copy)
            host = lambda parts, dim, empty: torch.cat(parts, dim=dim).cpu().numpy() if parts else np.zeros(empty, np.int64)
            result = (s, host(sse_y, 0, 0), host(sse_c, 1, (2, 0)), host(ssim, 0, 0).astype(np.float64),
                      host(ms, 0, (0, 5, 2)).astype(np.float64), host(nq, 0, (0, 1, 36)).astype(np.float64),
                      host(bq, 0, (0, 36)).astype(np.float64), host(tf, 0, 0).astype(np.float64),
                      host(lp, 0, (0, 5)).astype(np.float64))
            torch.cuda.synchronize(dev)
    return result


def evaluate_sequence(model, lr_dir: str, side_dir: str, gt_dir: Optional[str] = None, save_dir: Optional[str] = None, chunk: int = 8,
                      share_compensation: bool = False, crop_border: int = 4, quantise: str = "trunc", workers: int = 8,
                      png_level: int = 6, gumbel_uniform: Optional[Sequence] = None,
                      frame_noise: Optional[Sequence] = None, msssim: bool = False, niqe=None, brisque=None,
                      tof: bool = False, lpips=None, coding: str = "LD", rescale_metrics: bool = False) -> SequenceResult:
    """Super-resolve the sequence in ``lr_dir`` / ``side_dir`` (the reference's test layout, see cdfo_amd/priors.py) with ``model`` (on a
    GPU), ``chunk`` centre frames per forward.  ``save_dir``: write every frame as an 8-bit PNG under its LR file name.  ``gt_dir``:
    per-frame PSNR / SSIM of the 8-bit frames against ``<gt_dir>/%05d.png`` over the common size less ``crop_border``.
    ``quantise``: "trunc" (the reference's writer) or "nearest".  ``workers``: threads that read ground truth and encode PNGs, at
    most 16.  ``gumbel_uniform`` / ``frame_noise``: injected noise, per step or per frame, as `StreamingSR` takes it; without it the
    default mode draws per forward call, so its frames depend on the chunk size (the shared mode's never do).  ``msssim``: with
    ground truth, per-frame five-scale MS-SSIM (`metrics.msssim_u8`) as well; the region inside the border must then be at least
    `metrics.msssim_min_size` each way.  ``niqe``: the pristine model of the no-reference metric NIQE, a path or arrays as
    `metrics.niqe_params` takes them (the project ships no model); every output frame is then scored (`metrics.niqe_u8`, lower is
    better), WITH OR WITHOUT ground truth; the x4 frames must hold one 96 x 96 block.  ``brisque``: the support-vector model of the
    no-reference metric BRISQUE, a path, the five arrays or a `metrics.BrisqueParams` (`metrics.brisque_params`; the project ships no
    model); every output frame is then scored as well (`metrics.brisque_u8`, lower is better), with or without ground truth; the x4
    frames must be at least 16 x 16.  ``tof``: with ground truth, per-frame tOF as well (`metrics.tof_u8`: the mean distance between
    the Farneback flow of consecutive ground-truth frames and that of consecutive result frames over the whole common region, no
    border dropped; lower is better); the region must be at least 32 x 32, and without ground truth it is a ValueError.
    ``lpips``: the model of the learned perceptual distance LPIPS, a path, the arrays or a `metrics.LpipsParams` (`metrics.lpips_params`;
    the project ships no model, and parity with the ``lpips`` package is unpinned); with ground truth every frame's distance to it is
    then reported as well (`metrics.lpips_u8`: VGG-shaped trunk on the luma over the whole common region, lower is better); the
    region must be at least 16 x 16, and without ground truth it is a ValueError.  ``coding``: `StreamingSR`'s ("LD": the reference's
    flows from list 1; "RA": the random-access field from both lists, for a model trained on it).  ``rescale_metrics``:
    `evaluate_yuv`'s, accepted for symmetry: the frames here are 8-bit, where it changes nothing."""
    workers, chunk = _check_args(workers, quantise, chunk)
    check_coding(coding)
    t_start = time.perf_counter()
    lr = _PngSource(lr_dir)
    nq_params = _check_niqe(lr, niqe, rescale_metrics)
    bq_params = _check_brisque(lr, brisque, rescale_metrics)
    gt = sink = None
    if gt_dir is not None:
        gt = _PngSource(gt_dir, ["%05d.png" % t for t in range(lr.frames)])
        _check_regions(lr, gt, crop_border, 0)
        if msssim:
            _check_msssim(lr, gt, crop_border)
    tof = _check_tof(lr, gt, tof, rescale_metrics)
    lp_params = _check_lpips(lr, gt, lpips, rescale_metrics)
    if save_dir is not None:
        sink = _PngSink(save_dir, lr.names, png_level)   # the result PNGs take the LR frames' names (test_LD_37.py:180)

    def load():
        seq = load_sequence(lr_dir, side_dir)
        return StreamingSR(model, seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"], gumbel_uniform=gumbel_uniform,
                           frame_noise=frame_noise, coding=coding), None

    s, sse, _, ssim, ms, nq, bq, tf, lp = _run_chunks(lr, load, gt, sink, chunk, share_compensation, crop_border, 0, quantise, workers,
                                                      msssim, nq_params is not None, bq_params is not None, tof, lp_params)
    psnr, ms, nq = _psnr(sse, lr.shape, gt and gt.shape, crop_border, 255), M.msssim_from_components(ms), _niqe(nq, nq_params)
    bq, lp = _brisque(bq, bq_params), _lpips(lp)
    return SequenceResult(psnr, ssim, _mean(psnr), _mean(ssim), lr.frames, s.seconds, time.perf_counter() - t_start, ms, _mean(ms),
                          nq, _mean(nq), bq, _mean(bq), tf, _mean(tf), lp, _mean(lp))


class YuvResult(NamedTuple):
    psnr_y: np.ndarray          # fp64 [T] each (empty without ground truth)
    psnr_u: np.ndarray
    psnr_v: np.ndarray
    ssim_y: np.ndarray
    psnr_yuv: np.ndarray        # (6 Y + U + V) / 8 per frame (4:0:0: Y)
    mean_psnr_y: float          # nan without ground truth
    mean_psnr_u: float
    mean_psnr_v: float
    mean_ssim_y: float
    mean_psnr_yuv: float
    frames: int
    seconds_forward: float      # StreamingSR.seconds
    seconds_total: float        # the whole call
    msssim: np.ndarray = _NO_FRAMES                 # of the luma; fp64 [T] with ``msssim=True`` and ground truth, else empty
    mean_msssim: float = float("nan")
    niqe: np.ndarray = _NO_FRAMES                   # of the luma; fp64 [T] with ``niqe=`` a model (ground truth or not), else empty
    mean_niqe: float = float("nan")
    brisque: np.ndarray = _NO_FRAMES                # of the luma; fp64 [T] with ``brisque=`` a model (ground truth or not), else empty
    mean_brisque: float = float("nan")
    tof: np.ndarray = _NO_FRAMES                    # of the luma; fp64 [T] with ``tof=True`` (needs ground truth), else empty
    mean_tof: float = float("nan")
    lpips: np.ndarray = _NO_FRAMES                  # of the luma; fp64 [T] with ``lpips=`` a model (needs ground truth), else empty
    mean_lpips: float = float("nan")


def format_log_yuv(result: YuvResult, name: str) -> str:
    """`format_log` for a 4:2:0 result: the luma figures in the reference's places, then the chroma and the combined PSNR."""
    return '%s Average PSNR/SSIM: %.3f/%.5f PSNR-U/V/YUV: %.3f/%.3f/%.3f' % (
        name, result.mean_psnr_y, result.mean_ssim_y, result.mean_psnr_u, result.mean_psnr_v, result.mean_psnr_yuv) + _msssim_suffix(result) + \
        _niqe_suffix(result) + _brisque_suffix(result) + _tof_suffix(result) + _lpips_suffix(result)


def chroma_crop(crop_border: int, chroma: str = "420") -> int:
    """The border dropped from a 4:2:0 chroma plane when ``crop_border`` is dropped from the luma: half of it, rounded down.
    ``chroma="444"``: the planes are the luma's size and so is the border."""
    return int(crop_border) // 2 if chroma == "420" else int(crop_border)


def psnr_yuv(psnr_y, psnr_u, psnr_v) -> np.ndarray:
    """The JCT-VC combined PSNR of 4:2:0 material, per frame: (6 Y + U + V) / 8.  The project's definition for 4:4:4 as well (the
    weights are the convention's, not the planes' share of the samples); a 4:0:0 sequence reports its luma PSNR in this place."""
    y, u, v = (np.asarray(a, dtype=np.float64) for a in (psnr_y, psnr_u, psnr_v))
    return (6.0 * y + u + v) / 8.0


def evaluate_yuv(model, lr_yuv: str, width: int, height: int, side_dir: str, gt_yuv: Optional[str] = None,
                 save_yuv: Optional[str] = None, chunk: int = 8, share_compensation: bool = False, crop_border: int = 4,
                 quantise: str = "trunc", workers: int = 8, gumbel_uniform: Optional[Sequence] = None,
                 frame_noise: Optional[Sequence] = None, gt_size: Optional[Tuple[int, int]] = None,
                 pix_fmt: str = "yuv420p", msssim: bool = False, niqe=None, brisque=None, tof: bool = False,
                 lpips=None, coding: str = "LD", rescale_metrics: bool = False) -> YuvResult:
    """`evaluate_sequence` on raw 8-bit I420 files (cdfo_amd/yuv.py).  ``lr_yuv``: the LR sequence, ``width`` x ``height`` (even);
    the coding priors stay in ``side_dir``.  The luma goes the way it goes there (`StreamingSR.iter_chunked`, ``finish_frames`` with the
    PSNR numerator, ``ssim_u8``).  The chroma never passes through the model: per chunk the U and V planes of its centre frames are
    uploaded as 8 bits and upsampled x4 by ``kernels.chroma_up4`` (from the unpadded planes), against the ground truth's chroma with
    the border ``crop_border // 2``.  ``gt_yuv``: ground truth, an I420 file of ``gt_size`` = (width, height), by default 4 x the
    LR size; the pool copies the next chunk out of the memory map into one of two pinned buffers during the current forward.
    ``save_yuv``: the result as an I420 file of 4 width x 4 height, appended in frame order by the pool from one of two sets of
    pinned buffers.  The other arguments are `evaluate_sequence`'s.

    ``pix_fmt`` (`yuv.parse_pix_fmt`): the one format of ``lr_yuv``, ``gt_yuv`` and ``save_yuv``.  Above 8 bits the buffers hold
    uint16 samples and every figure is on the 0 .. 2**depth - 1 scale; the unfiltered planes and residuals in ``side_dir`` are at that
    depth too (16-bit PNGs, wider NPYs), the partition maps stay 8-bit masks.  ``gray*``: no chroma work, ``psnr_u`` / ``psnr_v`` are
    empty and ``psnr_yuv`` is ``psnr_y``.  ``yuv444p*``: chroma planes of the luma's size, their border ``crop_border``.
    ``msssim``: as `evaluate_sequence`'s, on the luma (`metrics.msssim_u8` / `msssim_u16` with the format's peak).  ``niqe``: as
    `evaluate_sequence`'s, on the luma of 8-bit formats; above 8 bits it is a ValueError (the reference defines the metric on 0 .. 255
    integers).  ``brisque``: as `evaluate_sequence`'s, with the same restriction to 8-bit formats.  ``tof``: as `evaluate_sequence`'s, on
    the luma of 8-bit formats with ground truth.  ``lpips``: as `evaluate_sequence`'s, on the luma only, of 8-bit formats with ground
    truth.  ``coding``: as `evaluate_sequence`'s.  ``rescale_metrics``: True lifts that restriction of ``niqe``, ``brisque``, ``tof``
    and ``lpips``: above 8 bits they then run their 16-bit forms on the luma (`metrics.niqe_features_u16`, `brisque_features_u16`,
    `tof_frames_u16`, `lpips_layers_u16`) with the format's peak, a sample v read as 255 v / peak (LPIPS: v / peak) -- the project's
    own definition, the reference has none above 8 bits; the size limits, the order of the errors, the result's fields and
    the log are the 8-bit ones.  On an 8-bit format, and with False (the default) on any, nothing changes."""
    fmt = parse_pix_fmt(pix_fmt)
    check_coding(coding)
    workers, chunk = _check_args(workers, quantise, chunk)
    t_start = time.perf_counter()
    ccrop = chroma_crop(crop_border, fmt.chroma)
    with YuvReader(lr_yuv, width, height, fmt) as head:
        lr = _YuvSource(head)
    nq_params = _check_niqe(lr, niqe, rescale_metrics)
    bq_params = _check_brisque(lr, brisque, rescale_metrics)
    gt = reader = writer = None
    try:
        if gt_yuv is not None:
            Wgt, Hgt = gt_size if gt_size is not None else (4 * width, 4 * height)
            reader = YuvReader(gt_yuv, Wgt, Hgt, fmt)
            gt = _YuvSource(reader)
            if gt.frames != lr.frames:
                raise ValueError(f"{gt_yuv} holds {gt.frames} frames of {Wgt}x{Hgt}, {lr_yuv} holds {lr.frames}")
            _check_regions(lr, gt, crop_border, ccrop)
            if msssim:
                _check_msssim(lr, gt, crop_border)
        tof = _check_tof(lr, gt, tof, rescale_metrics)
        lp_params = _check_lpips(lr, gt, lpips, rescale_metrics)
        writer = YuvWriter(save_yuv, 4 * width, 4 * height, fmt) if save_yuv is not None else None

        def load():
            seq = load_sequence_yuv(lr_yuv, width, height, side_dir, fmt)
            lr_c = (seq["u"], seq["v"]) if "u" in seq else None
            return StreamingSR(model, seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"],
                               gumbel_uniform=gumbel_uniform, frame_noise=frame_noise, peak=fmt.peak, coding=coding), lr_c

        s, sse_y, sse_c, ssim, ms, nq, bq, tf, lp = _run_chunks(lr, load, gt, writer and _YuvSink(writer), chunk, share_compensation,
                                                                crop_border, ccrop, quantise, workers, msssim, nq_params is not None,
                                                                bq_params is not None, tof, lp_params)
    finally:
        if writer is not None:
            writer.close()
        if reader is not None:
            reader.close()
    py = _psnr(sse_y, lr.shape, gt and gt.shape, crop_border, fmt.peak)
    pu, pv = (_psnr(e, lr.chroma_shape, gt and gt.chroma_shape, ccrop, fmt.peak) for e in sse_c)
    pyuv = psnr_yuv(py, pu, pv) if lr.chroma_shape is not None else py
    ms, nq, bq, lp = M.msssim_from_components(ms), _niqe(nq, nq_params), _brisque(bq, bq_params), _lpips(lp)
    return YuvResult(py, pu, pv, ssim, pyuv, _mean(py), _mean(pu), _mean(pv), _mean(ssim), _mean(pyuv), lr.frames, s.seconds,
                     time.perf_counter() - t_start, ms, _mean(ms), nq, _mean(nq), bq, _mean(bq), tf, _mean(tf), lp, _mean(lp))


def _write_synthetic(root: str, T: int, H: int, W: int, seed: int, put_lr, put_gt, peak: int = 255, markers: bool = False) -> str:
    """The random content of the synthetic writers, drawn in one fixed order: per frame the LR luma to ``put_lr(t, frame)``, the
    4H x 4W ground-truth luma to ``put_gt(t, frame)`` (None: not drawn), then the frame's coding priors into ``<root>/side``, which
    is returned.  ``peak`` above 255: samples over 0 .. peak as uint16, the unfiltered planes as 16-bit PNGs, the residuals scaled to
    the depth as int16; the partition maps stay 8-bit.  ``markers``: about three motion blocks in eight of every frame carry the
    random-access streams' "no reference in this list" mark, -99 in the reference component, in list 0, in list 1 or in both; the marks
    come from a generator of their own, so every other byte is what it is without them."""
    rs = np.random.RandomState(seed)
    rm = np.random.RandomState((seed + 0x51ED270B) % (1 << 32)) if markers else None
    kind, gain = (np.uint8, 1) if peak == 255 else (np.uint16, (peak + 1) // 256)
    side = os.path.join(root, "side")
    for d in (os.path.join(side, n) for n in ("part_m", "res", "unfiltered", "mvl0", "mvl1")):
        os.makedirs(d, exist_ok=True)
    hb, wb = (H + 7) // 8, (W + 7) // 8
    for t in range(T):
        put_lr(t, rs.randint(0, peak + 1, (H, W)).astype(kind))
        if put_gt is not None:
            put_gt(t, rs.randint(0, peak + 1, (4 * H, 4 * W)).astype(kind))
        if t >= 1 or T == 1:                         # the reference's side-info files start at 00001
            i = "%05d" % max(1, t)
            write_gray_png(os.path.join(side, "part_m", i + "_M_mask.png"), rs.randint(0, 256, (H, W)).astype(np.uint8))
            write_gray_png(os.path.join(side, "unfiltered", i + "_unflt.png"), rs.randint(0, peak + 1, (H, W)).astype(kind))
            res = np.clip(np.round(rs.randn(H, W, 3) * (6 * gain)), -128 * gain, 128 * gain - 1).astype(np.int8 if gain == 1 else np.int16)
            np.save(os.path.join(side, "res", i + "_res.npy"), res)
            marks = rm.randint(0, 8, (hb, wb)) if markers else None      # 1: list 0 marked, 2: list 1, 3: both, else neither
            for bit, name in ((1, "mvl0"), (2, "mvl1")):                 # block-constant motion, a reference distance of -2, -1 or 1
                mv = rs.randint(-64, 64, (hb, wb, 3)).astype(np.int16)
                mv[..., 2] = rs.choice([-2, -1, 1], size=(hb, wb))
                if marks is not None:
                    mv[(marks < 4) & ((marks & bit) != 0), 2] = -99
                mv = np.repeat(np.repeat(mv, 8, axis=0), 8, axis=1)[:H, :W]
                np.save(os.path.join(side, name, i + "_" + name + ".npy"), mv)
    return side


def write_synthetic_sequence(root: str, T: int, H: int, W: int, seed: int = 0, gt: bool = True, markers: bool = False):
    """A random sequence of T frames of H x W in the reference's layout under ``root`` (lr/, side/..., and gt/ with 4H x 4W frames):
    (lr_dir, side_dir, gt_dir or None).  For tools and benchmarks that have no data set at hand.  ``markers``: some motion blocks
    carry the random-access mark -99 in list 0, list 1 or both (`_write_synthetic`); every other byte is unchanged."""
    lr_dir, gt_dir = os.path.join(root, "lr"), os.path.join(root, "gt")
    os.makedirs(lr_dir, exist_ok=True)
    if gt:
        os.makedirs(gt_dir, exist_ok=True)
    side = _write_synthetic(root, T, H, W, seed, lambda t, f: write_gray_png(os.path.join(lr_dir, "%05d.png" % t), f),
                            (lambda t, f: write_gray_png(os.path.join(gt_dir, "%05d.png" % t), f, level=1)) if gt else None,
                            markers=markers)
    return lr_dir, side, (gt_dir if gt else None)


def write_synthetic_sequence_yuv(root: str, T: int, H: int, W: int, seed: int = 0, gt: bool = True, pix_fmt: str = "yuv420p",
                                 markers: bool = False):
    """`write_synthetic_sequence` with the frames in raw I420 files: the same luma and the same coding priors for the same ``seed``,
    plus random chroma (a generator of its own, so the luma's draws are those of the PNG layout).  H and W even.
    (lr_yuv, side_dir, gt_yuv or None); the files are ``<root>/lr_WxH.yuv`` and ``<root>/gt_4Wx4H.yuv``.
    ``pix_fmt``: another format of cdfo_amd/yuv.py (H and W even for 4:2:0 only).  Above 8 bits every plane draws from the whole
    0 .. 2**depth - 1, the priors are at that depth, and each chroma plane holds both ends of the range.  ``markers``: as
    `write_synthetic_sequence`'s."""
    fmt = parse_pix_fmt(pix_fmt)
    rc = np.random.RandomState((seed + 0x9E3779B9) % (1 << 32))
    lr_yuv, gt_yuv = os.path.join(root, "lr_%dx%d.yuv" % (W, H)), os.path.join(root, "gt_%dx%d.yuv" % (4 * W, 4 * H))
    os.makedirs(root, exist_ok=True)

    def planes(h, w):                                    # the two chroma planes of an h x w frame, drawn U then V
        shape = fmt.chroma_shape(h, w)
        if shape is None:
            return ()
        if fmt.depth == 8:
            return tuple(rc.randint(0, 256, shape).astype(np.uint8) for _ in range(2))
        both = tuple(rc.randint(0, fmt.peak + 1, shape).astype(np.uint16) for _ in range(2))
        for p in both:
            p.flat[0], p.flat[-1] = 0, fmt.peak
        return both

    with YuvWriter(lr_yuv, W, H, fmt) as lw:
        gw = YuvWriter(gt_yuv, 4 * W, 4 * H, fmt) if gt else None
        try:
            side = _write_synthetic(root, T, H, W, seed, lambda t, f: lw.append(f, *planes(H, W)),
                                    (lambda t, f: gw.append(f, *planes(4 * H, 4 * W))) if gt else None, fmt.peak, markers)
        finally:
            if gw is not None:
                gw.close()
    return lr_yuv, side, (gt_yuv if gt else None)
