"""Host side of YUV 4:2:0 evaluation: the I420 reader and writer (cdfo_amd/yuv.py), load_sequence_yuv against load_sequence, the numpy
statement of the x4 chroma filter (tests/chroma_ref.py) against its own definition, and the metric helpers.  No GPU."""
import os

import numpy as np
import pytest

from chroma_ref import COEF, catmull_rom_float, contents, up4, up4_sums


# --- reader and writer ------------------------------------------------------------------------------------------------------------
def _frames(T, W, H, seed):
    rs = np.random.RandomState(seed)
    return [(rs.randint(0, 256, (H, W)).astype(np.uint8), rs.randint(0, 256, (H // 2, W // 2)).astype(np.uint8),
             rs.randint(0, 256, (H // 2, W // 2)).astype(np.uint8)) for _ in range(T)]


@pytest.mark.parametrize("W,H", [(6, 4), (22, 18)])
def test_reader_writer_round_trip(tmp_path, W, H):
    from cdfo_amd.yuv import YuvReader, YuvWriter, frame_bytes
    p = str(tmp_path / "a.yuv")
    frames = _frames(3, W, H, W)
    with YuvWriter(p, W, H) as w:
        for y, u, v in frames:
            w.append(np.asfortranarray(y), u, v[::1])                       # any memory layout
        assert w.frames == 3
    assert os.path.getsize(p) == 3 * W * H * 3 // 2 == 3 * frame_bytes(W, H)
    raw = np.fromfile(p, dtype=np.uint8).reshape(3, -1)                      # the layout itself: Y, then U, then V, per frame
    for t, (y, u, v) in enumerate(frames):
        assert np.array_equal(raw[t], np.concatenate([y.ravel(), u.ravel(), v.ravel()]))
    with YuvReader(p, W, H) as r:
        assert r.frames == 3 and (r.width, r.height) == (W, H)
        for t, (y, u, v) in enumerate(frames):
            assert r.y(t).shape == (H, W) and r.u(t).shape == r.v(t).shape == (H // 2, W // 2) and r.y(t).dtype == np.uint8
            assert np.array_equal(r.y(t), y) and np.array_equal(r.u(t), u) and np.array_equal(r.v(t), v)
        ys, us, vs = r.y(1, 3), r.u(0, 3), r.v(1, 2)
        assert ys.shape == (2, H, W) and us.shape == (3, H // 2, W // 2) and vs.shape == (1, H // 2, W // 2)
        assert np.array_equal(ys, np.stack([f[0] for f in frames[1:]])) and np.array_equal(us, np.stack([f[1] for f in frames]))
        assert np.array_equal(vs[0], frames[1][2])
        assert not ys.flags["OWNDATA"] and not ys.flags["WRITEABLE"] and ys.strides[0] == frame_bytes(W, H)   # views of the map
        assert r.y(0, 0).shape == (0, H, W)
        with pytest.raises(IndexError):
            r.y(3)
        with pytest.raises(IndexError):
            r.u(2, 4)
    with YuvWriter(p, W, H) as w, pytest.raises(ValueError):
        w.append(frames[0][0], frames[0][1], frames[0][2][:, :-1])
    with YuvWriter(p, W, H) as w, pytest.raises(ValueError):
        w.append(frames[0][0].astype(np.int16), frames[0][1], frames[0][2])


def test_reader_refuses_odd_sizes_truncated_and_empty_files(tmp_path):
    from cdfo_amd.yuv import YuvReader, YuvWriter
    p = str(tmp_path / "a.yuv")
    with YuvWriter(p, 6, 4) as w:
        for y, u, v in _frames(3, 6, 4, 1):
            w.append(y, u, v)
    for (W, H) in ((5, 4), (6, 3), (0, 4), (6, -2)):
        with pytest.raises(ValueError):
            YuvReader(p, W, H)
        with pytest.raises(ValueError):
            YuvWriter(str(tmp_path / "b.yuv"), W, H)
    data = open(p, "rb").read()
    assert len(data) == 108
    open(p, "wb").write(data[:-1])                                           # truncated
    with pytest.raises(ValueError):
        YuvReader(p, 6, 4)
    open(p, "wb").write(data)
    with pytest.raises(ValueError):
        YuvReader(p, 8, 4)                                                   # 108 bytes are no whole number of 48-byte frames
    assert YuvReader(p, 6, 12).frames == 1                                   # ... but a raw file cannot tell 6x12 from three 6x4
    open(p, "wb").close()                                                    # zero frames
    with pytest.raises(ValueError):
        YuvReader(p, 6, 4)


# --- load_sequence_yuv ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 4])
def test_load_sequence_yuv_equals_load_sequence_on_the_same_content(tmp_path, T):
    from cdfo_amd.evaluate import write_synthetic_sequence, write_synthetic_sequence_yuv
    from cdfo_amd.priors import load_sequence, read_gray_png
    from cdfo_amd.yuv import YuvReader, load_sequence_yuv
    H, W = 10, 12
    lr_dir, side, gt_dir = write_synthetic_sequence(str(tmp_path / "png"), T, H, W, seed=7)
    lr_yuv, side_y, gt_yuv = write_synthetic_sequence_yuv(str(tmp_path / "yuv"), T, H, W, seed=7)
    a, b = load_sequence(lr_dir, side), load_sequence_yuv(lr_yuv, W, H, side_y)
    assert list(b)[:len(a)] == list(a) and set(b) - set(a) == {"u", "v"}
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert b["u"].shape == b["v"].shape == (T, H // 2, W // 2) and b["u"].dtype == b["v"].dtype == np.uint8
    assert b["lr"].flags["WRITEABLE"] and b["u"].flags["WRITEABLE"]          # copies: the map is closed again
    assert len(np.unique(b["u"])) > 16 and not np.array_equal(b["u"], b["v"])   # random chroma
    with YuvReader(lr_yuv, W, H) as r:
        assert r.frames == T and np.array_equal(r.u(0, T), b["u"]) and np.array_equal(r.v(0, T), b["v"])
    with YuvReader(gt_yuv, 4 * W, 4 * H) as g:                               # the ground truth's luma is the PNG layout's
        assert g.frames == T
        for t in range(T):
            assert np.array_equal(g.y(t), read_gray_png(os.path.join(gt_dir, "%05d.png" % t)))
        assert len(np.unique(g.u(0))) > 16
    assert write_synthetic_sequence_yuv(str(tmp_path / "nogt"), T, H, W, seed=7, gt=False)[2] is None
    assert not os.path.exists(str(tmp_path / "nogt" / ("gt_%dx%d.yuv" % (4 * W, 4 * H))))


def test_load_sequence_yuv_refuses_a_frame_count_the_priors_do_not_have(tmp_path):
    """load_sequence raises ValueError where the priors' planes do not fit the LR frames; so does a raw file whose frame count (or
    size, which for a raw file shows as one) disagrees with the priors present."""
    from cdfo_amd.evaluate import write_synthetic_sequence_yuv
    from cdfo_amd.yuv import YuvWriter, load_sequence_yuv
    lr_yuv, side, _ = write_synthetic_sequence_yuv(str(tmp_path / "s"), 4, 8, 12, gt=False)
    load_sequence_yuv(lr_yuv, 12, 8, side)
    with pytest.raises(ValueError, match="partition maps"):
        load_sequence_yuv(lr_yuv, 12, 16, side)                              # read as 2 frames of 12x16
    with pytest.raises(ValueError, match="planes are"):
        load_sequence_yuv(lr_yuv, 8, 12, side)                               # 4 frames, of the wrong shape
    longer = str(tmp_path / "longer.yuv")
    with YuvWriter(longer, 12, 8) as w:
        for _ in range(6):
            w.append(np.zeros((8, 12), np.uint8), np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint8))
    with pytest.raises(ValueError, match="partition maps"):
        load_sequence_yuv(longer, 12, 8, side)


# --- the filter ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 3), (5, 7), (9, 17), (33, 20)]


def test_coefficients_are_catmull_rom_out_of_128():
    """Fractions 5/8, 7/8, 1/8, 3/8; each row sums to 128 and is within 0.5 of 128 x the cubic's weight."""
    assert COEF.sum(axis=1).tolist() == [128] * 4
    for r, t in enumerate((5 / 8, 7 / 8, 1 / 8, 3 / 8)):
        w = np.array([(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2,
                      (t ** 3 - t ** 2) / 2])
        assert np.abs(COEF[r] - 128 * w).max() <= 0.5, (r, COEF[r], 128 * w)
    assert 255 * int(np.abs(COEF).sum(axis=1).max()) ** 2 < 2 ** 23             # the magnitudes the kernel's 32-bit sums hold


def test_filter_preserves_flat_planes():
    for shape in ((1, 1), (3, 5)):
        planes = np.arange(256, dtype=np.uint8)[:, None, None] * np.ones(shape, dtype=np.uint8)
        out = up4(planes)
        assert out.shape == (256, 4 * shape[0], 4 * shape[1])
        assert np.array_equal(out, np.arange(256, dtype=np.uint8)[:, None, None] * np.ones(out.shape[1:], dtype=np.uint8))


@pytest.mark.parametrize("shape", SHAPES)
def test_filter_order_of_axes_and_distance_to_float_catmull_rom(shape):
    """x then y == y then x (integers, no intermediate rounding); within 3 of the float64 cubic: coefficient rounding of at most
    1.0 per axis plus the final 0.5."""
    for name, p in contents(shape, shape[0] * 100 + shape[1]).items():
        a, b = up4(p), up4(p, x_first=False)
        assert a.dtype == np.uint8 and a.shape == (4 * shape[0], 4 * shape[1])
        assert np.array_equal(up4_sums(p), up4_sums(p, x_first=False)) and np.array_equal(a, b)
        assert np.abs(up4_sums(p)).max() < 2 ** 23
        d = np.abs(a.astype(np.float64) - catmull_rom_float(p)).max()
        print(f"{shape} {name}: max |integer filter - float64 Catmull-Rom| = {d}")
        assert d <= 3
        if name != "random" and min(shape) > 1:                              # both clamps are exercised
            s = (up4_sums(p) + 8192) >> 14
            assert s.min() < 0 and s.max() > 255


# --- metric helpers -----------------------------------------------------------------------------------------------------------------
def test_common_size_chroma_crop_and_psnr_yuv():
    from cdfo_amd import evaluate as E
    # 1080p luma, 540 x 960 chroma: crop 4 -> 2; ground truth taller / narrower: the min rule on the chroma planes
    assert [E.chroma_crop(c) for c in (0, 1, 2, 3, 4, 5, 8)] == [0, 0, 1, 1, 2, 2, 4]
    assert E.metric_region(540, 960, 540, 960, E.chroma_crop(4)) == (540, 960, 536, 956)
    assert E.metric_region(540, 960, 544, 958, E.chroma_crop(4)) == (540, 958, 536, 954)
    assert E.metric_region(36, 48, 36, 48, E.chroma_crop(4)) == (36, 48, 32, 44)
    got = E.psnr_yuv([40.0, 32.0], [48.0, 40.0], [32.0, 24.0])
    assert got.dtype == np.float64 and got.tolist() == [40.0, 32.0]          # (240 + 48 + 32) / 8, (192 + 40 + 24) / 8
    assert E.psnr_yuv([30.0], [38.0], [46.0]).tolist() == [33.0]             # (180 + 38 + 46) / 8
    assert E.psnr_yuv([], [], []).shape == (0,)
    assert np.isinf(E.psnr_yuv([np.inf], [30.0], [30.0])[0])
    r = E.YuvResult(*(np.zeros(0),) * 5, *(float("nan"),) * 5, 2, 0.5, 0.75)
    assert E.format_log_yuv(r, "s") == "s Average PSNR/SSIM: nan/nan PSNR-U/V/YUV: nan/nan/nan"
    r = E.YuvResult(*(np.zeros(2),) * 5, 31.23455, 40.0, 41.5, 0.906173, 33.6134, 2, 0.5, 0.75)
    assert E.format_log_yuv(r, "seq") == "seq Average PSNR/SSIM: 31.235/0.90617 PSNR-U/V/YUV: 40.000/41.500/33.613"


def test_evaluate_yuv_checks_its_arguments_before_it_reads_anything():
    from cdfo_amd import evaluate as E
    for bad in (64, 17, 0, -1, 2.5):
        with pytest.raises(ValueError, match="workers"):
            E.evaluate_yuv(None, "/nonexistent/lr.yuv", 8, 8, "/nonexistent/side", workers=bad)
    with pytest.raises(ValueError, match="quantise"):
        E.evaluate_yuv(None, "/nonexistent/lr.yuv", 8, 8, "/nonexistent/side", quantise="floor")
    with pytest.raises(ValueError, match="even"):
        E.evaluate_yuv(None, "/nonexistent/lr.yuv", 7, 8, "/nonexistent/side")
