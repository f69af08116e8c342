"""The six 16-bit sample kernels -- cdfo_niqe_mscn_u16, cdfo_niqe_half_u16, cdfo_brisque_mscn_u16, cdfo_brisque_half_u16,
cdfo_tof_level_u16, cdfo_lpips_stem_u16 -- and the ``_u16`` functions of cdfo_amd/metrics.py built on them.

Identity: a sample v of peak P is read as x = (255 v) / P in fp64 (LPIPS: (float)v / (float)P), and v = 257 k at P = 65535 gives the
8-bit form's value exactly (tests/test_metrics_u16_cpu.py), so an 8-bit frame times 257 must give the BITS of the 8-bit kernels at
every stage: maps, half images, level images, stem output, features, flows, scores.  Shapes: the smallest that take each path of a
kernel -- one block, ragged tiles, odd sizes with a rounded-up half image, every pyramid stage, the carried first frame.

In place: every kernel also reads its frames out of a wider buffer -- pitch above the width, a frame stride above the plane, the
region starting at an ODD column, so the pointer is 2-byte aligned only -- and must give the bits of the dense copy.

Statement: tests/*_ref.py fed 255 v / P as float64, at the peaks 1023, 4095 and 65535, on random frames that hold 0 and P.  The
bounds are the ones the 8-bit kernels' tests assert for the same stages (tests/test_gpu_{niqe,brisque,tof,lpips}_kernels.py): MSCN
maps 1e-12 absolute, half images 1e-10 absolute, features 1e-9 relative with equal table indices where the statement's two best
distances are at least 1e-9 apart, level images `LEVEL_ABS`, the stem 16 x the fp32 statement's own distance from the fp64 one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import brisque_ref
import lpips_cases
import lpips_ref
import niqe_ref
import tof_ref
from test_gpu_tof_kernels import LEVEL_ABS

pytestmark = pytest.mark.gpu
PEAKS = (1023, 4095, 65535)
MSCN_ABS, HALF_ABS, FEATURE_REL, GAP = 1e-12, 1e-10, 1e-9, 1e-9      # tests/test_gpu_niqe_kernels.py, test_gpu_brisque_kernels.py


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a, b))
    kind = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(kind), b.view(kind))


def u8_frames(n, H, W, seed):
    """uint8 [n,H,W]: a blocky field plus noise, so the maps have structure; holds 0 and 255."""
    rs = np.random.RandomState(seed)
    coarse = np.repeat(np.repeat(rs.randint(0, 256, (n, (H + 7) // 8, (W + 7) // 8)), 8, axis=1), 8, axis=2)[:, :H, :W]
    f = np.clip(coarse // 2 + rs.randint(0, 160, (n, H, W)), 0, 255).astype(np.uint8)
    f[:, 0, 0], f[:, -1, -1] = 0, 255
    return f


def x257(u8):
    return up(u8.astype(np.uint16) * np.uint16(257))


def random_u16(n, H, W, peak, seed):
    """uint16 [n,H,W] uniform on 0 .. peak that holds 0 and peak."""
    f = np.random.RandomState(seed).randint(0, peak + 1, (n, H, W)).astype(np.uint16)
    f[:, 0, 0], f[:, -1, -1] = 0, peak
    return f


def as_fp64(v, peak):
    return (255.0 * v.astype(np.float64)) / float(peak)


def in_place(frames):
    """The uint16 frames [n,H,W] (numpy) inside a device buffer [n+2,H+3,pitch] of other content, as a view that starts at column 1 of
    frame 1: its pitch and frame stride exceed the region and its first sample is 2-byte aligned only."""
    n, H, W = frames.shape
    pitch = W + 6 + (W & 1)                                                    # even, so frame 1 starts on an even sample
    buf = np.random.RandomState(11).randint(0, 65536, (n + 2, H + 3, pitch)).astype(np.uint16)
    buf[1:1 + n, :H, 1:1 + W] = frames
    view = up(buf)[1:1 + n, :H, 1:1 + W]
    assert not view.is_contiguous() and view.data_ptr() % 4 == 2 and view.stride() == ((H + 3) * pitch, pitch, 1)
    return view


# ---- NIQE ----
@pytest.mark.parametrize("H,W", [(96, 96), (100, 197)])
def test_niqe_identity_and_in_place(H, W):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    u = u8_frames(2, H, W, H + W)
    a8, a16, win = up(u), x257(u), M.niqe_window()
    R, Cc = M.niqe_region(H, W)
    m8, h8 = K.niqe_mscn(a8, R, Cc, win), K.niqe_half(a8, R, Cc)
    m16, h16 = K.niqe_mscn(a16, R, Cc, win, peak=65535), K.niqe_half(a16, R, Cc, peak=65535)
    assert same_bits(m16, m8) and same_bits(h16, h8)
    assert same_bits(K.niqe_mscn(h16, R // 2, Cc // 2, win), K.niqe_mscn(h8, R // 2, Cc // 2, win))
    F8, F16 = M.niqe_features_u8(a8), M.niqe_features_u16(a16, 65535)
    assert F16.shape == (2, (R // 96) * (Cc // 96), 36) and same_bits(F16, F8)
    mu, cov = niqe_ref.model()
    assert same_bits(M.niqe_u16(a16, 65535, (mu, cov)), M.niqe_u8(a8, (mu, cov)))
    # in place at another peak: the bits of the dense copy, and of a second call with a held scratch
    v = random_u16(2, H, W, 1023, H)
    view, dense = in_place(v), up(v)
    assert same_bits(K.niqe_mscn(view, R, Cc, win, peak=1023), K.niqe_mscn(dense, R, Cc, win, peak=1023))
    assert same_bits(K.niqe_half(view, R, Cc, peak=1023), K.niqe_half(dense, R, Cc, peak=1023))
    scratch = M.niqe_scratch(3, R, Cc, "cuda")
    assert same_bits(M.niqe_features_u16(view, 1023, scratch), M.niqe_features_u16(dense, 1023))


@functools.lru_cache(maxsize=None)
def niqe_case(peak):
    v = random_u16(1, 100, 197, peak, peak)[0]
    return v, niqe_ref.pieces(as_fp64(v, peak), niqe_ref.shared_table())


def _feature_columns(ok):
    """bool [..., 5] per (scale, map) -> bool [..., 36]: the feature columns of the maps that are set."""
    cols = np.zeros(ok.shape[:-2] + (36,), bool)
    for s in range(2):
        cols[..., 18 * s:18 * s + 2] = ok[..., s, 0:1]
        for k in range(1, 5):
            cols[..., 18 * s + 4 * k - 2:18 * s + 4 * k + 2] = ok[..., s, k:k + 1]
    return cols


@pytest.mark.parametrize("peak", PEAKS)
def test_niqe_against_the_statement(peak):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    v, want = niqe_case(peak)
    dev, win = up(v)[None], M.niqe_window()
    m1, hf = K.niqe_mscn(dev, 96, 192, win, peak=peak), K.niqe_half(dev, 96, 192, peak=peak)
    e1, eh = float(np.abs(m1[0].cpu().numpy() - want["mscn1"]).max()), float(np.abs(hf[0].cpu().numpy() - want["half"]).max())
    print(f"NIQE peak {peak}: MSCN scale 1 {e1:.2e}, half image {eh:.2e}")
    assert e1 <= MSCN_ABS and eh <= HALF_ABS
    F = M.niqe_features_u16(dev, peak)[0].cpu().numpy()                            # [nb,36]
    sure = (want["gap"] >= GAP).transpose(1, 0, 2)                                 # [nb,2,5]
    gam = niqe_ref.shared_table()[0]
    alphas = F[:, niqe_ref.ALPHAS].reshape(-1, 2, 5)
    assert np.array_equal(alphas[sure], gam[want["index"].transpose(1, 0, 2)][sure])
    cols = _feature_columns(sure) & ~np.isnan(want["features"])
    assert np.array_equal(np.isnan(F), np.isnan(want["features"])) and cols.sum() >= 30
    rel = np.abs(F[cols] - want["features"][cols]) / np.abs(want["features"][cols])
    print(f"NIQE peak {peak}: features worst {rel.max():.2e} relative over {int(cols.sum())} of {cols.size}")
    assert rel.max() <= FEATURE_REL


# ---- BRISQUE ----
@pytest.mark.parametrize("H,W", [(16, 16), (17, 23), (96, 160)])
def test_brisque_identity_and_in_place(H, W):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    u = u8_frames(2, H, W, H * W)
    a8, a16, win = up(u), x257(u), M.brisque_window()
    m8, h8 = K.brisque_mscn(a8, win), K.brisque_half(a8)
    m16, h16 = K.brisque_mscn(a16, win, peak=65535), K.brisque_half(a16, peak=65535)
    assert h16.shape == (2, (H + 1) // 2, (W + 1) // 2) and same_bits(m16, m8) and same_bits(h16, h8)
    assert same_bits(K.brisque_mscn(h16, win), K.brisque_mscn(h8, win))
    F8, F16 = M.brisque_features_u8(a8), M.brisque_features_u16(a16, 65535)
    assert F16.shape == (2, 36) and same_bits(F16, F8)
    model = brisque_ref.model()
    assert same_bits(M.brisque_u16(a16, 65535, model), M.brisque_u8(a8, model))
    v = random_u16(2, H, W, 4095, W)
    view, dense = in_place(v), up(v)
    assert same_bits(K.brisque_mscn(view, win, peak=4095), K.brisque_mscn(dense, win, peak=4095))
    assert same_bits(K.brisque_half(view, peak=4095), K.brisque_half(dense, peak=4095))
    scratch = M.brisque_scratch(3, H, W, "cuda")
    assert same_bits(M.brisque_features_u16(view, 4095, scratch), M.brisque_features_u16(dense, 4095))


@functools.lru_cache(maxsize=None)
def brisque_case(peak, H, W):
    v = random_u16(1, H, W, peak, peak + H)[0]
    return v, brisque_ref.pieces(as_fp64(v, peak), brisque_ref.shared_table())


@pytest.mark.parametrize("H,W", [(17, 23), (96, 160)])
@pytest.mark.parametrize("peak", PEAKS)
def test_brisque_against_the_statement(peak, H, W):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    v, want = brisque_case(peak, H, W)
    dev, win = up(v)[None], M.brisque_window()
    m1, hf = K.brisque_mscn(dev, win, peak=peak), K.brisque_half(dev, peak=peak)
    e1, eh = float(np.abs(m1[0].cpu().numpy() - want["mscn1"]).max()), float(np.abs(hf[0].cpu().numpy() - want["half"]).max())
    print(f"BRISQUE {H}x{W} peak {peak}: MSCN scale 1 {e1:.2e}, half image {eh:.2e}")
    assert e1 <= MSCN_ABS and eh <= HALF_ABS
    F, wantF = M.brisque_features_u16(dev, peak)[0].cpu().numpy(), want["features"]
    gam = brisque_ref.shared_table()[0]
    assert np.array_equal(np.isnan(F), np.isnan(wantF))
    assert np.array_equal(F[list(brisque_ref.ALPHAS)], gam[want["index"].reshape(10)])      # the fixture's rule: indices equal
    zero = wantF == 0
    assert np.array_equal(F[zero], wantF[zero])
    ok = ~np.isnan(wantF) & ~zero
    rel = np.abs(F[ok] - wantF[ok]) / np.abs(wantF[ok])
    print(f"BRISQUE {H}x{W} peak {peak}: features worst {rel.max():.2e} relative")
    assert rel.max() <= FEATURE_REL


# ---- tOF ----
def _tof_frames(H, W, seed):
    """uint8 [4,H,W]: one field moving by a pixel or two per frame, plus noise."""
    rs = np.random.RandomState(seed)
    canvas = u8_frames(1, H + 8, W + 8, seed)[0].astype(np.int64)
    out = [np.clip(canvas[4 + dy:4 + dy + H, 4 + dx:4 + dx + W] + rs.randint(-3, 4, (H, W)), 0, 255) for dy, dx in ((0, 0), (1, -1), (2, 1), (1, 2))]
    return np.stack(out).astype(np.uint8)


@pytest.mark.parametrize("H,W", [(32, 32), (37, 45), (69, 131)])
def test_tof_identity_and_in_place(H, W):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    u = _tof_frames(H, W, H)
    a8, a16 = up(u), x257(u)
    v = random_u16(4, H, W, 1023, H + W)
    view, dense = in_place(v), up(v)
    assert len(M.tof_size(H, W)) == (2 if H >= 64 else 1)
    for k, h, w in M.tof_size(H, W):
        taps = M.tof_taps(k)
        assert same_bits(K.tof_level(a16[:3], a16[1:], h, w, taps, peak=65535), K.tof_level(a8[:3], a8[1:], h, w, taps))
        # the chunk form: the carried frame in front, pair j's previous frame is frame j - 1 of the same stack
        assert same_bits(K.tof_level(a16[1:], a16[1:], h, w, taps, first=a16[0], peak=65535),
                         K.tof_level(a8[1:], a8[1:], h, w, taps, first=a8[0]))
        assert same_bits(K.tof_level(view[:3], view[1:], h, w, taps, peak=1023), K.tof_level(dense[:3], dense[1:], h, w, taps, peak=1023))
        assert same_bits(K.tof_level(view[1:], view[1:], h, w, taps, first=view[0], peak=1023),
                         K.tof_level(dense[1:], dense[1:], h, w, taps, first=dense[0].contiguous(), peak=1023))
    assert same_bits(M.farneback_u16(a16[:3], a16[1:], 65535), M.farneback_u8(a8[:3], a8[1:]))
    noisy = np.clip(u.astype(np.int64) + np.random.RandomState(2).randint(-6, 7, u.shape), 0, 255).astype(np.uint8)
    b8, b16 = up(noisy), x257(noisy)
    assert same_bits(M.tof_u16(a16, b16, 65535), M.tof_u8(a8, b8))
    carried = M.tof_frames_u16(a16[1:], b16[1:], 65535, a16[0], b16[0], M.tof_scratch(2, H, W, "cuda"))      # one frame per group
    assert same_bits(carried, M.tof_frames_u8(a8[1:], b8[1:], a8[0], b8[0])) and same_bits(carried.cpu().numpy(), M.tof_u8(a8, b8)[1:])


@pytest.mark.parametrize("H,W", [(37, 45), (69, 131)])
@pytest.mark.parametrize("peak", PEAKS)
def test_tof_levels_against_the_statement(peak, H, W):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    v = random_u16(3, H, W, peak, peak + W)
    x, dev, worst = as_fp64(v, peak), up(v), 0.0
    for k, h, w in tof_ref.levels(H, W):
        want = np.stack([np.stack([tof_ref.level_image(x[j], k, h, w), tof_ref.level_image(x[j + 1], k, h, w)]) for j in range(2)])
        got = K.tof_level(dev[:2], dev[1:], h, w, M.tof_taps(k), peak=peak).cpu().numpy()
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"tOF {H}x{W} peak {peak}: level images worst {worst:.3e} (bound {LEVEL_ABS:.3e})")
    assert worst <= LEVEL_ABS


# ---- LPIPS ----
def _stem(params, frames, normalize, peak=None):
    from cdfo_amd import kernels as K
    w0, b0 = torch.from_numpy(np.array(params.weights[0])).cuda(), torch.from_numpy(np.array(params.biases[0])).cuda()
    return K.lpips_stem(frames, w0, b0, normalize, peak=peak)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("H,W", [(16, 16), (18, 35)])
def test_lpips_identity_and_in_place(H, W, normalize):
    from cdfo_amd import metrics as M
    params = lpips_cases.model(lpips_cases.NARROW, 11)
    sr, gt = lpips_cases.frames((H, W), (H, W), 2, H)
    assert same_bits(_stem(params, x257(sr), normalize, 65535), _stem(params, up(sr), normalize))
    L8, L16 = M.lpips_layers_u8(up(sr), up(gt), params, normalize=normalize), M.lpips_layers_u16(x257(sr), x257(gt), 65535, params, normalize=normalize)
    assert L16.shape == (2, 5) and same_bits(L16, L8)
    assert same_bits(M.lpips_u16(x257(sr), x257(gt), 65535, params, normalize), M.lpips_u8(up(sr), up(gt), params, normalize))
    v = random_u16(2, H, W, 4095, H + W)
    view, dense = in_place(v), up(v)
    assert same_bits(_stem(params, view, normalize, 4095), _stem(params, dense, normalize, 4095))
    other = up(random_u16(2, H, W, 4095, 5))
    assert same_bits(M.lpips_layers_u16(view, other, 4095, params, normalize=normalize),
                     M.lpips_layers_u16(dense, other, 4095, params, normalize=normalize))
    assert not M.lpips_layers_u16(view, view, 4095, params).any()                  # equal stacks: exactly 0


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("peak", PEAKS)
def test_lpips_stem_against_the_statement(peak, normalize):
    params = lpips_cases.model(lpips_cases.NARROW, 11)
    v = random_u16(2, 18, 35, peak, peak)
    x = as_fp64(v, peak)
    want = np.stack([lpips_ref.stem(f, params, normalize).permute(1, 2, 0).numpy() for f in x])
    f32 = np.stack([lpips_ref.stem(f, params, normalize, dtype=torch.float32).permute(1, 2, 0).numpy() for f in x])
    floor = float(np.abs(f32 - want).max() / np.abs(want).max())
    got = _stem(params, up(v), normalize, peak)
    assert got.shape == want.shape and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
    print(f"LPIPS stem peak {peak} normalize {normalize}: {err:.2e} of the largest value; the fp32 statement's floor {floor:.2e}")
    assert floor > 0.0 and err <= 16 * floor


# ---- the entry points' own checks ----
def test_entry_points_refuse_bad_peaks_and_odd_pointers_before_any_launch():
    from cdfo_amd import _lib
    from cdfo_amd import metrics as M
    lib = _lib.lib()
    vp, ll = C.c_void_p, C.c_longlong
    st = vp(torch.cuda.current_stream().cuda_stream)
    u = torch.zeros((3, 96, 128), dtype=torch.uint16, device="cuda")          # K = 2 below: a frame of room behind the shifted pointers
    d = torch.zeros((2 * 2 * 96 * 128,), dtype=torch.float64, device="cuda")
    f = torch.zeros((2 * 96 * 128 * 16,), dtype=torch.float32, device="cuda")
    w0, b0 = torch.zeros((16, 3, 3, 3), device="cuda"), torch.zeros(16, device="cuda")
    win, taps = np.ascontiguousarray(M.niqe_window()), np.ascontiguousarray(M.tof_taps(0))
    p, hw, ht = u.data_ptr(), vp(win.ctypes.data), vp(taps.ctypes.data)
    calls = {
        "niqe_mscn": lambda src, peak: lib.cdfo_niqe_mscn_u16(vp(src), 128, ll(96 * 128), 2, 96, 96, hw, vp(d.data_ptr()), peak, st),
        "niqe_half": lambda src, peak: lib.cdfo_niqe_half_u16(vp(src), 128, ll(96 * 128), 2, 96, 96, vp(d.data_ptr()), peak, st),
        "brisque_mscn": lambda src, peak: lib.cdfo_brisque_mscn_u16(vp(src), 128, ll(96 * 128), 2, 96, 128, hw, vp(d.data_ptr()), peak, st),
        "brisque_half": lambda src, peak: lib.cdfo_brisque_half_u16(vp(src), 128, ll(96 * 128), 2, 96, 128, vp(d.data_ptr()), peak, st),
        "tof_level": lambda src, peak: lib.cdfo_tof_level_u16(vp(src), 128, ll(96 * 128), vp(src), 128, ll(96 * 128), None, 0, 2, 96, 128, 96,
                                                              128, ht, 3, vp(d.data_ptr()), peak, st),
        "lpips_stem": lambda src, peak: lib.cdfo_lpips_stem_u16(vp(src), 128, ll(96 * 128), 2, 96, 128, vp(w0.data_ptr()), vp(b0.data_ptr()),
                                                                16, 1, vp(f.data_ptr()), peak, st),
    }
    for name, call in calls.items():
        for peak in (0, -1, 65536, 1 << 20):
            assert call(p, peak) == -1, (name, peak)
        assert call(p + 1, 1023) == -2, name                                       # an odd address
        assert call(p + 2, 1023) == 0 and call(p, 1) == 0 and call(p, 65535) == 0, name      # 2-byte aligned is enough (the buffer has room)
    torch.cuda.synchronize()
