"""Host side of sequence evaluation (cdfo_amd/evaluate.py): the log line, the min-crop rule, the PNG writer's level / vectorised
filter-0 path, the numpy statement of the quantiser, the worker cap, and the chunk loop's frame sources and sinks.  No GPU."""
import struct
import zlib

import numpy as np
import pytest

from cdfo_amd import evaluate as E
from cdfo_amd.priors import read_gray_png, write_gray_png


def test_format_log_is_the_reference_line():
    r = E.SequenceResult(np.array([30.0, 32.4691]), np.array([0.9, 0.912346]), 31.23455, 0.906173, 2, 0.5, 0.75)
    assert E.format_log(r, "BasketballDrive_1920x1080_50_500F") == "BasketballDrive_1920x1080_50_500F Average PSNR/SSIM: 31.235/0.90617"
    nan = E.SequenceResult(np.zeros(0), np.zeros(0), float("nan"), float("nan"), 2, 0.5, 0.75)
    assert E.format_log(nan, "s") == "s Average PSNR/SSIM: nan/nan"


@pytest.mark.parametrize("gt,want", [((1080, 1920), (1080, 1920, 1072, 1912)),      # equal
                                     ((1088, 1920), (1080, 1920, 1072, 1912)),      # ground truth taller: its extra rows are dropped
                                     ((1080, 1916), (1080, 1916, 1072, 1908)),      # narrower: the result's extra columns are dropped
                                     ((1000, 2000), (1000, 1920, 992, 1912))])      # one of each
def test_metric_region_is_the_min_rule(gt, want):
    """psnr_ssim.py:462-468: both images are cropped to (min_height, min_width), then the border of 4 goes."""
    assert E.metric_region(1080, 1920, gt[0], gt[1], 4) == want
    assert E.metric_region(1080, 1920, gt[0], gt[1], 0) == (want[0], want[1], want[0], want[1])


def _old_filter0_file(img, level):
    """What write_gray_png wrote for filter 0 before its row loop became one array operation: byte for byte."""
    rows = bytearray()
    for y in range(img.shape[0]):
        rows.append(0)
        rows += img[y].tobytes()

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 8, 0, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(bytes(rows), level)) + chunk(b"IEND", b""))


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (84, 108)])
def test_png_writer_level_and_vectorised_filter0(tmp_path, shape):
    rs = np.random.RandomState(shape[0])
    img = (rs.randint(0, 256, size=shape) // 16 * 16).astype(np.uint8)       # compressible, so the levels differ
    p = str(tmp_path / "a.png")
    write_gray_png(p, img)
    assert open(p, "rb").read() == _old_filter0_file(img, 6)                 # default: the old bytes
    assert np.array_equal(read_gray_png(p), img)
    sizes = {}
    for level in (0, 1, 6, 9):
        for ft in (0, 2, 4):
            write_gray_png(p, img, ft, level=level)
            assert np.array_equal(read_gray_png(p), img), (level, ft)
        write_gray_png(p, img, level=level)
        assert open(p, "rb").read() == _old_filter0_file(img, level)
        sizes[level] = len(open(p, "rb").read())
    if img.size > 1000:
        assert sizes[0] > max(sizes[1], sizes[6], sizes[9])                  # level 0 stores; the others deflate 16-level data
    view = np.asfortranarray(img)                                            # any memory layout
    write_gray_png(p, view)
    assert open(p, "rb").read() == _old_filter0_file(img, 6)


def test_quantiser_statement_equals_the_reference_writer():
    """clip, ONE fp32 multiply by 255, truncation == (np.clip(x, 0, 1) * 255.0).astype(np.uint8) (test_LD_37.py:179-180), on every
    k / 255 (in fp32 and from fp64), their fp32 neighbours, and values beyond both ends."""
    k = np.arange(256)
    exact = (k / 255.0).astype(np.float32)
    x = np.concatenate([exact, (k.astype(np.float32) / np.float32(255.0)), np.nextafter(exact, np.float32(2)),
                        np.nextafter(exact, np.float32(-1)), np.linspace(-0.2, 1.2, 4001).astype(np.float32),
                        np.array([-0.0, 0.0, 1.0, -np.inf, np.inf], np.float32)])
    want = (np.clip(x, 0, 1) * 255.0).astype(np.uint8)
    assert (np.clip(x, 0, 1) * 255.0).dtype == np.float32
    got = E.quantise_numpy(x)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 255
    # truncation is not rounding: the two modes differ, by exactly one level and never downwards
    near = E.quantise_numpy(x, "nearest")
    assert np.array_equal(near, np.rint(np.clip(x, 0, 1) * np.float32(255.0)).astype(np.uint8))
    d = near.astype(int) - got.astype(int)
    assert set(np.unique(d)) == {0, 1}
    assert E.quantise_numpy(np.array([np.nan], np.float32))[0] == 0           # documented: NaN -> 0
    with pytest.raises(ValueError):
        E.quantise_numpy(x, "floor")


def test_worker_cap():
    """The pool is sized by the caller, never from the machine's CPU count; more than 16 is refused before anything is read."""
    for bad in (64, 17, 0, -1, 2.5):
        with pytest.raises(ValueError, match="workers"):
            E.evaluate_sequence(None, "/nonexistent/lr", "/nonexistent/side", workers=bad)
    with pytest.raises(ValueError, match="quantise"):
        E.evaluate_sequence(None, "/nonexistent/lr", "/nonexistent/side", quantise="floor")
    assert E.MAX_WORKERS == 16


def test_psnr_from_integer_sums_is_the_oracle_bit_for_bit():
    """mse = float64(sse) / n, then calculate_psnr's expression: on integer-valued frames np.mean of the squares is exact, so
    the two agree to the last bit."""
    from cdfo_amd.metrics import psnr_from_sse
    from oracle.metrics_ref import calculate_psnr
    rs = np.random.RandomState(3)
    for shape, crop in (((84, 108), 4), ((84, 108), 0), ((19, 19), 4), ((270, 480), 4)):
        a = rs.randint(0, 256, shape).astype(np.uint8)
        b = np.clip(a.astype(int) + rs.randint(-9, 10, shape), 0, 255).astype(np.uint8)
        c = slice(crop, shape[0] - crop), slice(crop, shape[1] - crop)
        sse = int(((a[c].astype(np.int64) - b[c].astype(np.int64)) ** 2).sum())
        assert psnr_from_sse([sse], a[c].size)[0] == calculate_psnr(a, b, crop)
    assert np.isinf(psnr_from_sse([0], 100)[0])


class _NoEvent:
    """Stands in for the copy's event: the download it guards is not what these tests are about."""

    def synchronize(self):
        pass


def test_sources_and_sinks_without_a_gpu(tmp_path):
    """The two kinds of frame source on the same content (T = 3, 6 x 8, one seed, once as PNGs and once as a gray raw file), and the
    two kinds of frame sink behind an event that does nothing."""
    import concurrent.futures as cf
    import os
    import threading
    from cdfo_amd.yuv import YuvReader, YuvWriter
    T, H, W = 3, 6, 8
    lr_dir, _, gt_dir = E.write_synthetic_sequence(str(tmp_path / "png"), T, H, W, seed=7)
    _, _, gt_yuv = E.write_synthetic_sequence_yuv(str(tmp_path / "raw"), T, H, W, seed=7, pix_fmt="gray")
    png = E._PngSource(gt_dir)
    with YuvReader(gt_yuv, 4 * W, 4 * H, "gray") as reader:
        raw = E._YuvSource(reader)
        assert png.frames == raw.frames == T and png.shape == raw.shape == (4 * H, 4 * W)
        assert png.chroma_shape is None and raw.chroma_shape is None
        assert (png.dtype, png.peak) == (raw.dtype, raw.peak)
        for t in range(T):
            a, b = np.full((4 * H, 4 * W), 7, np.uint8), np.full((4 * H, 4 * W), 9, np.uint8)
            png.stage(t, a)
            raw.stage(t, b)
            assert np.array_equal(a, b) and a.tobytes() == b.tobytes()
            # exactly the arrays the two readers hand out
            assert np.array_equal(a, read_gray_png(os.path.join(gt_dir, "%05d.png" % t))) and np.array_equal(b, reader.y(t))
    # a ground-truth directory whose frame 1 has another shape: refused when that frame is staged, by its number
    write_gray_png(os.path.join(gt_dir, "00001.png"), np.zeros((4 * H, 4 * W - 1), np.uint8))
    odd, view = E._PngSource(gt_dir), np.zeros((4 * H, 4 * W), np.uint8)
    odd.stage(0, view)
    with pytest.raises(ValueError, match="frame 1 "):
        odd.stage(1, view)
    frames = np.random.RandomState(1).randint(0, 256, (4, 4 * H, 4 * W)).astype(np.uint8)
    with cf.ThreadPoolExecutor(max_workers=2) as pool:
        # PNGs under the LR names, whichever slot of the chunk a frame sits in
        names = E._PngSource(lr_dir).names
        assert names == ["%05d.png" % t for t in range(T)]
        save = str(tmp_path / "out")
        for f in E._PngSink(save, names, 1)(pool, _NoEvent(), [1, 2], frames[:2], None):
            f.result()
        assert sorted(os.listdir(save)) == names[1:]
        assert all(np.array_equal(read_gray_png(os.path.join(save, names[1 + j])), frames[j]) for j in range(2))
        # the raw file in submission order: chunk 1 is handed in, and runs on the second worker, while chunk 0 still waits for its copy
        gate = threading.Event()
        held = _NoEvent()
        held.synchronize = gate.wait
        out = str(tmp_path / "out.yuv")
        with YuvWriter(out, 4 * W, 4 * H, "gray") as writer:
            sink = E._YuvSink(writer)
            first, = sink(pool, held, [0, 1], frames[:2], None)
            second, = sink(pool, _NoEvent(), [2, 3], frames[2:], None)
            assert not first.done() and not second.done()
            gate.set()
            second.result()
            assert first.done()
        with YuvReader(out, 4 * W, 4 * H, "gray") as r:
            assert r.frames == 4 and np.array_equal(r.y(0, 4), frames)
