"""Host side of sequence evaluation (cdfo_amd/evaluate.py): the log line, the min-crop rule, the PNG writer's level / vectorised
filter-0 path, the numpy statement of the quantiser and the worker cap.  No GPU."""
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
