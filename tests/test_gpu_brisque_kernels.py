"""The four BRISQUE kernels (csrc/brisque.hip) on the GPU, each against the numpy statement of the definition (tests/brisque_ref.py) at
the fixture frames of tests/golden/brisque_ref.npz.  Every kernel is fed the STATEMENT's input, so each bound is that kernel's own.

Frames c, d and z (all zeros) go in one launch (K = 3) as a slice of a larger buffer, with a frame stride and a row stride larger than
the frame and other content behind each frame's edge (the window's padding is ZERO, so none of it may be read); a, b and e are
launched alone.  Bounds (the issue's, the scheme of tests/test_gpu_niqe_kernels.py): MSCN maps 1e-12 absolute on O(1) values; the half
image 1e-10 absolute on values up to 255; counts exact; each sum -- a strip's and a frame's -- within 10 N 2^-53 of the sum of its
terms' magnitudes, N = H W (every term is >= 0, so that is the sum itself); table indices equal (the fixture's smallest gap between
the two best distances is 2e-3 relative); features 1e-9 relative, exact where the statement's is 0."""
import ctypes as C

import numpy as np
import pytest
import torch

import brisque_ref as ref

pytestmark = pytest.mark.gpu
GROUPS = ["cdz", "a", "b", "e"]
ALPHAS = list(ref.ALPHAS)


def _frames(group):
    """(device uint8 [K,H,W] view, the names): one frame alone as it is; c, d, z inside a [5,80,144] buffer of other content."""
    z = ref.golden()
    if len(group) == 1:
        return torch.from_numpy(z["frame_" + group]).cuda()[None], group
    buf = np.random.RandomState(3).randint(1, 256, (5, 80, 144)).astype(np.uint8)
    for k, n in enumerate(group):
        buf[1 + k, :70, :130] = z["frame_" + n]
    view = torch.from_numpy(buf).cuda()[1:4, :70, :130]
    assert view.stride() == (80 * 144, 144, 1) and not view.is_contiguous()
    return view, group


def _stack(group, key):
    return np.stack([ref.golden_pieces(n)[key] for n in group])


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint64)


def _strips(m):
    """fp64 [G,5,6]: the statement's six sums of each map over each strip of 16 rows."""
    maps, H = ref.products(m), m.shape[0]
    out = np.zeros(((H + 15) // 16, 5, 6))
    for g in range(out.shape[0]):
        for k, full in enumerate(maps):
            v = full[16 * g:16 * g + 16]
            neg, pos = v < 0, v > 0
            out[g, k] = (neg.sum(), pos.sum(), (v[neg] ** 2).sum(), (v[pos] ** 2).sum(), np.abs(v).sum(), (v ** 2).sum())
    return out


def _check_features(F, names, what):
    want, index = _stack(names, "features"), _stack(names, "index")             # [K,36], [K,2,5]
    gam = ref.shared_table()[0]
    assert F.shape == want.shape and np.array_equal(np.isnan(F), np.isnan(want))
    got_index = np.searchsorted(gam, F[:, ALPHAS])
    assert np.array_equal(gam[got_index], F[:, ALPHAS]) and np.array_equal(got_index, index.reshape(len(names), 10))
    zero = want == 0
    assert np.array_equal(F[zero], want[zero])
    ok = ~np.isnan(want) & ~zero
    rel = np.abs(F[ok] - want[ok]) / np.abs(want[ok])
    print(f"{names} {what}: features worst {rel.max():.2e} relative, {int(np.isnan(want).sum())} NaN")
    assert rel.max() <= 1e-9


@pytest.mark.parametrize("group", GROUPS)
def test_mscn_and_half(group):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    frames, names = _frames(group)
    H, W = frames.shape[1:]
    Hh, Wh = (H + 1) // 2, (W + 1) // 2
    want1, wanth, want2 = _stack(names, "mscn1"), _stack(names, "half"), _stack(names, "mscn2")
    m1 = K.brisque_mscn(frames, M.brisque_window())
    hf = K.brisque_half(frames)
    m2 = K.brisque_mscn(_up(wanth), M.brisque_window())
    assert m1.shape == (len(names), H, W) and hf.shape == m2.shape == (len(names), Hh, Wh) and m1.dtype == hf.dtype == torch.float64
    e1, eh, e2 = (float(np.abs(g.cpu().numpy() - w).max()) for g, w in ((m1, want1), (hf, wanth), (m2, want2)))
    print(f"{group}: MSCN scale 1 {e1:.2e}, half image {eh:.2e}, MSCN scale 2 {e2:.2e}")
    assert e1 <= 1e-12 and e2 <= 1e-12 and eh <= 1e-10
    if "z" in names:                                                           # zeros in, zeros out: nothing behind the edge was read
        k = names.index("z")
        assert not m1[k].any() and not hf[k].any() and not m2[k].any()
    # the same bits from a second launch, and from a contiguous copy of the slice
    assert torch.equal(m1, K.brisque_mscn(frames, M.brisque_window())) and torch.equal(hf, K.brisque_half(frames))
    dense = frames.contiguous()
    assert torch.equal(m1, K.brisque_mscn(dense, M.brisque_window())) and torch.equal(hf, K.brisque_half(dense))
    # a strided fp64 source (the half image inside a wider buffer) as well
    wide = torch.full((len(names), Hh + 3, Wh + 5), 1e9, dtype=torch.float64, device="cuda")
    wide[:, :Hh, :Wh] = _up(wanth)
    assert torch.equal(m2, K.brisque_mscn(wide[:, :Hh, :Wh], M.brisque_window()))


@pytest.mark.parametrize("group", GROUPS)
def test_sums_and_features(group):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    names = group
    table = torch.from_numpy(M.brisque_table().copy()).cuda()
    from_statement = torch.full((len(names), 36), -1.0, dtype=torch.float64, device="cuda")
    from_device = from_statement.clone()
    for scale in (0, 1):
        maps = _stack(names, "mscn%d" % (scale + 1))
        N = maps.shape[1] * maps.shape[2]
        want = _stack(names, "sums%d" % (scale + 1))                           # [K,5,6]
        strips = np.stack([_strips(m) for m in maps])                          # [K,G,5,6]
        s = K.brisque_sums(_up(maps))
        assert torch.equal(s, K.brisque_sums(_up(maps)))
        got = s.cpu().numpy()
        assert got.shape == strips.shape == (len(names), (maps.shape[1] + 15) // 16, 5, 6)
        total, bound = got.sum(axis=1), 10.0 * N * 2.0 ** -53
        assert np.array_equal(got[..., :2], strips[..., :2]) and np.array_equal(total[..., :2], want[..., :2])       # the counts
        e_strip, e_total = np.abs(got[..., 2:] - strips[..., 2:]), np.abs(total[..., 2:] - want[..., 2:])
        print(f"{group} scale {scale + 1}: {got.shape[1]} strips, sums worst {np.max(e_total / np.maximum(want[..., 2:], 1e-300)):.2e} "
              f"of the sum (bound {bound:.2e})")
        assert (e_strip <= bound * strips[..., 2:]).all() and (e_total <= bound * want[..., 2:]).all()
        K.brisque_features(_up(want[:, None]), N, table, scale, from_statement)       # from the STATEMENT's sums, as one strip
        K.brisque_features(s, N, table, scale, from_device)                           # the strips added on the device
    _check_features(from_statement.cpu().numpy(), names, "from the statement's sums")
    _check_features(from_device.cpu().numpy(), names, "from the device's strips")


@pytest.mark.parametrize("group", GROUPS)
def test_features_of_frames(group):
    """The seven launches of `brisque_features_u8` on the frames themselves: the same indices and 1e-9 relative again, equal bits from a
    second call, from a scratch made for more frames, and from a dense copy."""
    from cdfo_amd import metrics as M
    frames, names = _frames(group)
    F = M.brisque_features_u8(frames)
    assert F.shape == (len(names), 36) and F.dtype == torch.float64 and F.is_cuda
    scratch = M.brisque_scratch(len(names) + 2, *frames.shape[1:], frames.device)
    again, held, dense = M.brisque_features_u8(frames), M.brisque_features_u8(frames, scratch), M.brisque_features_u8(frames.contiguous())
    for other in (again, held, dense):
        assert np.array_equal(_bits(F), _bits(other))
    _check_features(F.cpu().numpy(), names, "of the frames")


def test_zero_frame_leaves_its_neighbours_alone():
    """z's features are NaN where the statement's are (the reference asserts on such a frame); c and d, launched with it, have the bits
    they have when launched alone and when launched with another frame in z's place."""
    from cdfo_amd import metrics as M
    frames, names = _frames("cdz")
    F = M.brisque_features_u8(frames).cpu().numpy()
    want = ref.golden_pieces("z")["features"]
    assert np.isnan(F[2]).sum() == 24 and np.array_equal(np.isnan(F[2]), np.isnan(want))
    assert np.array_equal(F[2][~np.isnan(want)], want[~np.isnan(want)])
    assert np.isnan(M.brisque_from_features(F, ref.model())).tolist() == [False, False, True]
    for k in (0, 1):
        assert np.array_equal(_bits(F[k]), _bits(M.brisque_features_u8(frames[k].contiguous()))[0])
    other = frames.clone()
    other[2] = frames[0].flip(0)
    assert np.array_equal(_bits(F[:2]), _bits(M.brisque_features_u8(other))[:2])


def test_wrong_sizes_and_strides_raise_before_any_launch():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    w, table = M.brisque_window(), torch.from_numpy(M.brisque_table().copy()).cuda()
    u = torch.zeros((2, 40, 60), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, 32, 32), dtype=torch.float64, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    bad = [lambda: K.brisque_mscn(u.float(), w), lambda: K.brisque_mscn(u, w[:6]), lambda: K.brisque_mscn(u.transpose(1, 2), w),
           lambda: K.brisque_mscn(u.cpu(), w), lambda: K.brisque_mscn(u, w, out=f64(2, 40, 59)),
           lambda: K.brisque_mscn(u, w, out=f64(2, 40, 120)[:, :, ::2]), lambda: K.brisque_mscn(u, w, out=f64(2, 40, 60).float()),
           lambda: K.brisque_half(d), lambda: K.brisque_half(u[:, :7]), lambda: K.brisque_half(u[:, :, ::2]),
           lambda: K.brisque_half(u, out=f64(2, 20, 31)), lambda: K.brisque_sums(d.float()), lambda: K.brisque_sums(d[:, :, :16]),
           lambda: K.brisque_sums(d[:, :1].contiguous()), lambda: K.brisque_sums(d, out=f64(2, 3, 5, 6)),
           lambda: K.brisque_features(f64(2, 1, 5, 5), 1024, table, 0, None), lambda: K.brisque_features(f64(2, 1, 5, 6), 1024, table[:2], 0, None),
           lambda: K.brisque_features(f64(2, 1, 5, 6), 1024, table[:, :9800], 0, None),
           lambda: K.brisque_features(f64(2, 1, 5, 6), 1024, table, 2, None), lambda: K.brisque_features(f64(2, 1, 5, 6), 0, table, 0, None),
           lambda: K.brisque_features(f64(2, 1, 5, 6), 1024, table, 0, f64(2, 1, 36)),
           lambda: M.brisque_features_u8(u[:, :15, :16]), lambda: M.brisque_features_u8(u[:, :16, :15]),
           lambda: M.brisque_features_u8(u, M.brisque_scratch(1, 40, 60, "cuda")),
           lambda: M.brisque_features_u8(u, M.brisque_scratch(2, 40, 62, "cuda")), lambda: M.brisque_scratch(2, 15, 16, "cuda"),
           lambda: M.brisque_features_u8(u, M.niqe_scratch(2, 96, 96, "cuda")),
           lambda: M.brisque_u8(u, (np.zeros((3, 36)), np.zeros(3), np.zeros((36, 2)), 0.05, -1.0))]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")
    # the library's own checks, through the C ABI: statuses, nothing launched
    lib, p = _lib.lib(), d.data_ptr()
    vp, st = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    host_w = np.ascontiguousarray(w).ctypes.data
    assert lib.cdfo_brisque_mscn_u8(vp(u.data_ptr()), 59, C.c_longlong(2400), 2, 40, 60, vp(host_w), vp(p), st) == -1      # pitch < W
    assert lib.cdfo_brisque_mscn_u8(vp(u.data_ptr()), 60, C.c_longlong(-1), 2, 40, 60, vp(host_w), vp(p), st) == -1
    assert lib.cdfo_brisque_mscn_u8(vp(u.data_ptr()), 60, C.c_longlong(2400), 0, 40, 60, vp(host_w), vp(p), st) == -1
    assert lib.cdfo_brisque_mscn_u8(vp(u.data_ptr()), 60, C.c_longlong(2400), 2, 40, 60, vp(host_w), vp(p + 4), st) == -2   # alignment
    assert lib.cdfo_brisque_mscn_f64(vp(p + 4), 32, C.c_longlong(1024), 2, 32, 32, vp(host_w), vp(p), st) == -2
    assert lib.cdfo_brisque_mscn_u8(vp(u.data_ptr()), 60, C.c_longlong(2400), 2, 40, 60, None, vp(p), st) == -1
    assert lib.cdfo_brisque_half(vp(u.data_ptr()), 60, C.c_longlong(2400), 2, 7, 60, vp(p), st) == -1
    assert lib.cdfo_brisque_half(vp(u.data_ptr()), 59, C.c_longlong(2400), 2, 40, 60, vp(p), st) == -1
    assert lib.cdfo_brisque_half(vp(u.data_ptr()), 60, C.c_longlong(2400), 2, 40, 60, vp(p + 2), st) == -2
    assert lib.cdfo_brisque_sums(vp(p), 2, 1, 32, vp(p), st) == -1
    assert lib.cdfo_brisque_sums(vp(p), 70000, 32, 32, vp(p), st) == -1
    assert lib.cdfo_brisque_sums(vp(p), 2, 32, 32, vp(p + 4), st) == -2
    assert lib.cdfo_brisque_sums(vp(p), 2, 65536, 65536, vp(p), st) == -1                                                    # 32-bit offsets
    assert lib.cdfo_brisque_features(vp(p), 2, 1, 1024, vp(table.data_ptr()), 2, vp(p), st) == -1
    assert lib.cdfo_brisque_features(vp(p), 2, 0, 1024, vp(table.data_ptr()), 0, vp(p), st) == -1
    assert lib.cdfo_brisque_features(vp(p), 2, 1, 0, vp(table.data_ptr()), 0, vp(p), st) == -1
    assert lib.cdfo_brisque_features(vp(p), 2, 1, 1024, vp(table.data_ptr() + 4), 0, vp(p), st) == -2
    torch.cuda.synchronize()
