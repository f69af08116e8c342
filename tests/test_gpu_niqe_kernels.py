"""The four NIQE kernels (csrc/niqe.hip) on the GPU, each against the numpy statement of the definition (tests/niqe_ref.py) at the
fixture frames of tests/golden/niqe_ref.npz.  Every kernel is fed the STATEMENT's input, so each bound is that kernel's own.

Frames b, c and f go in one launch (K = 3) as a slice of a larger buffer, with a frame stride and a row stride larger than the region
and other content behind the region's edge; a, d and e are launched alone.  Bounds (the issue's): MSCN maps 1e-12 absolute on O(1)
values; the half image 1e-10 absolute on values up to 255; counts exact, each sum within 1e-11 of the sum of its terms' magnitudes
(9216 reordered terms cost at most 9216 * 2^-53 = 1e-12 of it, times ten); table indices equal unless the statement's two best
distances differ by less than 1e-9 relative (at most one such search per frame; the fixture has none); features 1e-9 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import niqe_ref as ref

pytestmark = pytest.mark.gpu
GROUPS = ["bcf", "a", "d", "e"]


def _frames(group):
    """(device uint8 [K,H,W] view, the names): one frame alone as it is; b, c, f inside a [5,210,320] buffer of other content."""
    z = ref.golden()
    if len(group) == 1:
        return torch.from_numpy(z["frame_" + group]).cuda()[None], group
    buf = np.random.RandomState(3).randint(0, 256, (5, 210, 320)).astype(np.uint8)
    for k, n in enumerate(group):
        f = z["frame_" + n]
        buf[1 + k, :f.shape[0], :f.shape[1]] = f
    view = torch.from_numpy(buf).cuda()[1:4, :200, :300]
    assert view.stride() == (210 * 320, 320, 1) and not view.is_contiguous()
    return view, group


def _stack(group, key):
    return np.stack([ref.golden_pieces(n)[key] for n in group])


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("group", GROUPS)
def test_mscn_and_half(group):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    frames, names = _frames(group)
    R, Cc = M.niqe_region(*frames.shape[1:])
    want1, wanth, want2 = _stack(names, "mscn1"), _stack(names, "half"), _stack(names, "mscn2")
    m1 = K.niqe_mscn(frames, R, Cc, M.niqe_window())
    hf = K.niqe_half(frames, R, Cc)
    m2 = K.niqe_mscn(_up(wanth), R // 2, Cc // 2, M.niqe_window())
    assert m1.shape == (len(names), R, Cc) and hf.shape == m2.shape == (len(names), R // 2, Cc // 2) and m1.dtype == torch.float64
    e1, eh, e2 = (float(np.abs(g.cpu().numpy() - w).max()) for g, w in ((m1, want1), (hf, wanth), (m2, want2)))
    print(f"{group}: MSCN scale 1 {e1:.2e}, half image {eh:.2e}, MSCN scale 2 {e2:.2e}")
    assert e1 <= 1e-12 and e2 <= 1e-12 and eh <= 1e-10
    # the same bits from a second launch, and from a contiguous copy of the slice
    assert torch.equal(m1, K.niqe_mscn(frames, R, Cc, M.niqe_window())) and torch.equal(hf, K.niqe_half(frames, R, Cc))
    dense = frames.contiguous()
    assert torch.equal(m1, K.niqe_mscn(dense, R, Cc, M.niqe_window())) and torch.equal(hf, K.niqe_half(dense, R, Cc))
    # a strided fp64 source (the half image inside a wider buffer) as well
    wide = torch.full((len(names), R // 2 + 3, Cc // 2 + 5), 1e9, dtype=torch.float64, device="cuda")
    wide[:, :R // 2, :Cc // 2] = _up(wanth)
    assert torch.equal(m2, K.niqe_mscn(wide, R // 2, Cc // 2, M.niqe_window()))


@pytest.mark.parametrize("group", GROUPS)
def test_block_sums_and_features(group):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    names = group
    table = torch.from_numpy(M.niqe_table().copy()).cuda()
    gam = M.niqe_table()[0]
    out = torch.full((len(names), _stack(names, "sums1").shape[1], 36), -1.0, dtype=torch.float64, device="cuda")
    for scale, B in ((0, 96), (1, 48)):
        want = _stack(names, "sums%d" % (scale + 1))                           # [K,nb,5,6]
        s = K.niqe_block_sums(_up(_stack(names, "mscn%d" % (scale + 1))), B)
        assert torch.equal(s, K.niqe_block_sums(_up(_stack(names, "mscn%d" % (scale + 1))), B))
        got = s.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got[..., :2], want[..., :2])             # the counts
        # every term of these sums is >= 0, so the sum of the terms' magnitudes is the sum itself
        err = np.abs(got[..., 2:] - want[..., 2:])
        print(f"{group} scale {scale + 1}: sums worst {np.max(err / np.maximum(want[..., 2:], 1e-300)):.2e} of the sum")
        assert (err <= 1e-11 * want[..., 2:]).all()
        K.niqe_features(_up(want), B * B, table, scale, out)                   # from the STATEMENT's sums
    F = out.cpu().numpy()
    want, index, gap = _stack(names, "features"), _stack(names, "index"), _stack(names, "gap")      # index, gap: [K,2,nb,5]
    assert np.array_equal(np.isnan(F), np.isnan(want))
    alphas = F[:, :, ref.ALPHAS].reshape(F.shape[0], F.shape[1], 2, 5).transpose(0, 2, 1, 3)
    got_index = np.searchsorted(gam, alphas)
    assert np.array_equal(gam[got_index], alphas)                              # every alpha is an entry of the table
    differ = got_index != index
    assert (gap[differ] < 1e-9).all() and (differ.reshape(len(names), -1).sum(axis=1) <= 1).all()
    assert not (gap < 1e-9).any()                                              # the fixture has no tie in the statement
    flat = want[:, :, ref.ALPHAS] == gam[0]
    assert np.array_equal(F[:, :, ref.ALPHAS] == gam[0], flat)
    ok = ~np.isnan(want)
    rel = np.abs(F[ok] - want[ok]) / np.abs(want[ok])
    print(f"{group}: features worst {rel.max():.2e} relative, {int(np.isnan(want).sum())} NaN, {int(flat.sum())} alphas at gam[0]")
    assert rel.max() <= 1e-9


@pytest.mark.parametrize("group", GROUPS)
def test_features_of_frames(group):
    """The seven launches of `niqe_features_u8` on the frames themselves: the same indices and 1e-9 relative again (the sums'
    1e-12 on the way is far inside it), equal bits from a second call, from a scratch made for more frames, and from a dense copy."""
    from cdfo_amd import metrics as M
    frames, names = _frames(group)
    F = M.niqe_features_u8(frames)
    want = _stack(names, "features")
    assert F.shape == want.shape and F.dtype == torch.float64 and F.is_cuda
    scratch = M.niqe_scratch(len(names) + 2, *M.niqe_region(*frames.shape[1:]), frames.device)
    again, held, dense = M.niqe_features_u8(frames), M.niqe_features_u8(frames, scratch), M.niqe_features_u8(frames.contiguous())
    for other in (again, held, dense):
        assert np.array_equal(F.cpu().numpy().view(np.uint64), other.cpu().numpy().view(np.uint64))
    F = F.cpu().numpy()
    assert np.array_equal(np.isnan(F), np.isnan(want)) and np.array_equal(F[:, :, ref.ALPHAS], want[:, :, ref.ALPHAS])
    ok = ~np.isnan(want)
    rel = np.abs(F[ok] - want[ok]) / np.abs(want[ok])
    print(f"{group}: features of the frames worst {rel.max():.2e} relative")
    assert rel.max() <= 1e-9


def test_wrong_sizes_and_strides_raise_before_any_launch():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    w, table = M.niqe_window(), torch.from_numpy(M.niqe_table().copy()).cuda()
    u = torch.zeros((2, 200, 300), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, 96, 96), dtype=torch.float64, device="cuda")
    bad = [lambda: K.niqe_mscn(u, 201, 288, w), lambda: K.niqe_mscn(u, 192, 301, w), lambda: K.niqe_mscn(u, 0, 288, w),
           lambda: K.niqe_mscn(u.float(), 192, 288, w), lambda: K.niqe_mscn(u, 192, 288, w[:6]),
           lambda: K.niqe_mscn(u.transpose(1, 2), 192, 192, w), lambda: K.niqe_mscn(u.cpu(), 192, 288, w),
           lambda: K.niqe_mscn(u, 192, 288, w, out=torch.zeros((2, 192, 287), dtype=torch.float64, device="cuda")),
           lambda: K.niqe_mscn(u, 192, 288, w, out=torch.zeros((2, 192, 576), dtype=torch.float64, device="cuda")[:, :, ::2]),
           lambda: K.niqe_half(u, 191, 288), lambda: K.niqe_half(u, 192, 302), lambda: K.niqe_half(u, 6, 288),
           lambda: K.niqe_half(d, 96, 96), lambda: K.niqe_block_sums(d, 95), lambda: K.niqe_block_sums(d, 1),
           lambda: K.niqe_block_sums(d[:, :, :48], 48), lambda: K.niqe_block_sums(d.float(), 96),
           lambda: K.niqe_features(torch.zeros((2, 1, 5, 5), dtype=torch.float64, device="cuda"), 9216, table, 0, None),
           lambda: K.niqe_features(torch.zeros((2, 1, 5, 6), dtype=torch.float64, device="cuda"), 9216, table[:, :9800], 0, None),
           lambda: K.niqe_features(torch.zeros((2, 1, 5, 6), dtype=torch.float64, device="cuda"), 9216, table, 2, None),
           lambda: K.niqe_features(torch.zeros((2, 1, 5, 6), dtype=torch.float64, device="cuda"), 0, table, 0, None),
           lambda: M.niqe_features_u8(u[:, :95]), lambda: M.niqe_features_u8(u, M.niqe_scratch(1, 192, 288, "cuda")),
           lambda: M.niqe_features_u8(u, M.niqe_scratch(2, 96, 288, "cuda")), lambda: M.niqe_scratch(2, 100, 288, "cuda")]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")
    # the library's own checks, through the C ABI: statuses, nothing launched
    lib, p = _lib.lib(), d.data_ptr()
    vp, st = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    host_w = np.ascontiguousarray(w).ctypes.data
    assert lib.cdfo_niqe_mscn_u8(vp(u.data_ptr()), 287, C.c_longlong(60000), 2, 192, 288, vp(host_w), vp(p), st) == -1     # pitch < C
    assert lib.cdfo_niqe_mscn_u8(vp(u.data_ptr()), 300, C.c_longlong(-1), 2, 192, 288, vp(host_w), vp(p), st) == -1
    assert lib.cdfo_niqe_mscn_u8(vp(u.data_ptr()), 300, C.c_longlong(60000), 2, 192, 288, vp(host_w), vp(p + 4), st) == -2  # alignment
    assert lib.cdfo_niqe_mscn_f64(vp(p + 4), 96, C.c_longlong(9216), 2, 96, 96, vp(host_w), vp(p), st) == -2
    assert lib.cdfo_niqe_mscn_u8(vp(u.data_ptr()), 300, C.c_longlong(60000), 2, 192, 288, None, vp(p), st) == -1
    assert lib.cdfo_niqe_half(vp(u.data_ptr()), 300, C.c_longlong(60000), 2, 191, 288, vp(p), st) == -1
    assert lib.cdfo_niqe_half(vp(u.data_ptr()), 300, C.c_longlong(60000), 2, 192, 288, vp(p + 2), st) == -2
    assert lib.cdfo_niqe_block_sums(vp(p), 2, 96, 96, 36, vp(p), st) == -1     # 36 does not divide 96
    assert lib.cdfo_niqe_block_sums(vp(p), 2, 96, 96, 48, vp(p + 4), st) == -2
    assert lib.cdfo_niqe_block_sums(vp(p), 70000, 96, 96, 48, vp(p), st) == -1
    assert lib.cdfo_niqe_features(vp(p), 2, 1, 9216, vp(table.data_ptr()), 2, vp(p), st) == -1
    assert lib.cdfo_niqe_features(vp(p), 2, 0, 9216, vp(table.data_ptr()), 0, vp(p), st) == -1
    assert lib.cdfo_niqe_features(vp(p), 2, 1, 9216, vp(table.data_ptr() + 4), 0, vp(p), st) == -2
    torch.cuda.synchronize()
