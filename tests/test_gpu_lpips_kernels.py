"""The four kernels of csrc/lpips.hip, each fed the statement's own inputs (tests/lpips_ref.py).

Stem: ReLU(conv1_1) of 8-bit frames against the fp64 statement; the bound is 16 x the distance of the statement's own fp32 form from
it, measured on the CPU for the same frames (tests/lpips_cases.py), as a fraction of the largest value.  Pool: bit-equal to
``torch.max_pool2d``.  Distance and fold: fed fp32 features, they are fp64 with another order of addition over at most a few thousand
terms, so 1e-12 relative against the statement; equal stacks give exactly 0, swapped stacks and repeated calls equal bits."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as cases
import lpips_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def region_case():
    """Three 40 x 64 frames whose top-left 33 x 50 is the region: (params, frames, fp64 stem of the region, its fp32 floor)."""
    params = cases.model(cases.NARROW, 11)
    frames = np.random.RandomState(7).randint(0, 256, (3, 40, 64)).astype(np.uint8)
    want = np.stack([ref.stem(f[:33, :50], params).permute(1, 2, 0).numpy() for f in frames])
    f32 = np.stack([ref.stem(f[:33, :50], params, dtype=torch.float32).permute(1, 2, 0).numpy() for f in frames])
    return params, frames, want, float(np.abs(f32 - want).max() / np.abs(want).max())


def _stem(params, frames, normalize=True):
    from cdfo_amd import kernels as K
    w0, b0 = torch.from_numpy(np.array(params.weights[0])).cuda(), torch.from_numpy(np.array(params.biases[0])).cuda()
    return K.lpips_stem(frames, w0, b0, normalize)


@pytest.mark.parametrize("name", ["narrow-16x16", "narrow-37x53", "true-32x32", "region-33x50-of-40x64"])
def test_stem_matches_the_statement(name):
    if name.startswith("region"):
        params, frames, want, floor = region_case()
        dev = torch.from_numpy(frames).cuda()[:, :33, :50]                 # read in place: pitch 64, frame stride 40 * 64
        assert not dev.is_contiguous()
    else:
        params, frames, want, floor = cases.stem_case(name)
        dev = torch.from_numpy(np.array(frames)).cuda()
    got = _stem(params, dev)
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
    print(f"{name}: stem against the fp64 statement {err:.2e} of the largest value; the fp32 statement's floor {floor:.2e}")
    assert floor > 0.0 and err <= 16 * floor
    assert torch.equal(got, _stem(params, dev))


def test_stem_without_normalize():
    params, frames, want_on, floor = cases.stem_case("narrow-37x53")
    want = np.stack([ref.stem(f, params, normalize=False).permute(1, 2, 0).numpy() for f in frames])
    f32 = np.stack([ref.stem(f, params, normalize=False, dtype=torch.float32).permute(1, 2, 0).numpy() for f in frames])
    floor = float(np.abs(f32 - want).max() / np.abs(want).max())
    got = _stem(params, torch.from_numpy(np.array(frames)).cuda(), normalize=False).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"normalize=False: {err:.2e} of the largest value, floor {floor:.2e}")
    assert err <= 16 * floor and np.abs(want - want_on).max() > 0.1


@pytest.mark.parametrize("C", [16, 512])
@pytest.mark.parametrize("H,W", [(37, 53), (2, 3), (2, 2), (3, 3)])
def test_pool_is_bit_equal(H, W, C):
    from cdfo_amd import kernels as K
    x = torch.from_numpy(np.random.RandomState(H * W + C).standard_normal((2, H, W, C)).astype(np.float32))
    if H > 3:
        x[1, 5, 7, 3] = float("nan")                                        # a NaN wins, as in ATen
        x[0, 36, 52, :] = 1e9                                               # the floored row and column are never read
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    got = K.lpips_pool2(x.cuda()).cpu()
    assert got.shape == want.shape == (2, H // 2, W // 2, C)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if H > 3:
        assert torch.isnan(got[1, 2, 3, 3]) and int(torch.isnan(got).sum()) == 1 and float(got[~torch.isnan(got)].max()) < 1e8


@functools.lru_cache(maxsize=None)
def stacks(C, h, w):
    """Two fp32 NHWC stacks [2,h,w,C] of ReLU outputs and lin [C]; frame 0 has a pixel whose features are all zero in the first stack
    only, frame 1 one where they are zero in both (with one pixel: frame 0 the first kind, frame 1 the second).  -> with the
    statement's sums [2]."""
    rs = np.random.RandomState(C + 7 * h + w)
    a = np.maximum(rs.standard_normal((2, h, w, C)), 0.0).astype(np.float32)
    b = np.maximum(a + 0.3 * rs.standard_normal((2, h, w, C)), 0.0).astype(np.float32)
    lin = rs.uniform(0.0, 1.0, C)
    a[0, 0, 0] = 0.0
    a[1, h - 1, w - 1] = 0.0
    b[1, h - 1, w - 1] = 0.0
    t = lambda x: torch.from_numpy(x).permute(2, 0, 1)
    want = np.array([ref.layer_distance(t(a[j]), t(b[j]), lin) for j in range(2)])
    return a, b, lin, want


def _distance(a, b, lin):
    from cdfo_amd import kernels as K
    N, h, w, _ = a.shape
    part = K.lpips_dist(a, b, lin)
    assert part.shape == (N, (h + K.LPIPS_STRIP - 1) // K.LPIPS_STRIP) and part.dtype == torch.float64
    return K.lpips_fold(part.view(-1), N, [part.shape[1]], [h * w]).cpu().numpy()[:, 0]


@pytest.mark.parametrize("C", [16, 64, 512])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (37, 53)])
def test_distance_and_fold_match_the_statement(h, w, C):
    a, b, lin, want = stacks(C, h, w)
    da, db, dl = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(lin).cuda()
    got = _distance(da, db, dl)
    err = np.abs(got - want)
    print(f"C = {C}, {h}x{w}: device {got}, statement {want}, worst relative difference {float((err / np.maximum(want, 1e-300)).max()):.2e}")
    assert np.all(np.isfinite(got)) and np.all(err <= 1e-12 * want)
    assert want[0] > 0.0 and (want[1] > 0.0 or h * w == 1)
    assert np.array_equal(_distance(da, da.clone(), dl), np.zeros(2))                       # equal stacks: exactly 0
    assert np.array_equal(_distance(db, da, dl).view(np.uint64), got.view(np.uint64))       # swapped: equal bits
    assert np.array_equal(_distance(da, db, dl).view(np.uint64), got.view(np.uint64))       # again: equal bits


def test_fold_takes_the_layers_in_one_launch():
    from cdfo_amd import kernels as K
    one, two = stacks(16, 37, 53), stacks(64, 2, 3)
    dev = lambda x: torch.from_numpy(x).cuda()
    p1, p2 = K.lpips_dist(dev(one[0]), dev(one[1]), dev(one[2])), K.lpips_dist(dev(two[0]), dev(two[1]), dev(two[2]))
    packed = torch.cat([p1.view(-1), p2.view(-1)])
    got = K.lpips_fold(packed, 2, [p1.shape[1], p2.shape[1]], [37 * 53, 6]).cpu().numpy()
    assert got.shape == (2, 2)
    assert np.all(np.abs(got[:, 0] - one[3]) <= 1e-12 * one[3]) and np.all(np.abs(got[:, 1] - two[3]) <= 1e-12 * two[3])
    out = torch.empty((2, 2), dtype=torch.float64, device="cuda")
    assert K.lpips_fold(packed, 2, [p1.shape[1], p2.shape[1]], [37 * 53, 6], out=out) is out and np.array_equal(out.cpu().numpy(), got)


def test_wrappers_refuse_before_any_launch():
    from cdfo_amd import kernels as K
    u = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    w0, b0 = torch.zeros((16, 3, 3, 3), device="cuda"), torch.zeros(16, device="cuda")
    x, lin = torch.zeros((2, 4, 4, 16), device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda")
    part = torch.zeros(4, dtype=torch.float64, device="cuda")
    bad = [lambda: K.lpips_stem(u.float(), w0, b0), lambda: K.lpips_stem(u, w0.double(), b0), lambda: K.lpips_stem(u, w0[:8], b0[:8]),
           lambda: K.lpips_stem(u, w0, b0.cpu()), lambda: K.lpips_stem(u.transpose(1, 2), w0, b0),
           lambda: K.lpips_stem(u, w0, b0, out=torch.zeros((2, 16, 16, 32), device="cuda")),
           lambda: K.lpips_pool2(x.double()), lambda: K.lpips_pool2(x[..., :6]), lambda: K.lpips_pool2(x[:, :1]),
           lambda: K.lpips_pool2(x.permute(0, 2, 1, 3)[:, :, ::2]), lambda: K.lpips_pool2(x, out=torch.zeros((2, 2, 2, 8), device="cuda")),
           lambda: K.lpips_dist(x, x[:1], lin), lambda: K.lpips_dist(x, x, lin.float()), lambda: K.lpips_dist(x, x, lin[:8]),
           lambda: K.lpips_dist(x, x.cpu(), lin), lambda: K.lpips_dist(x, x, lin, out=torch.zeros((2, 3), dtype=torch.float64, device="cuda")),
           lambda: K.lpips_fold(part, 2, [3], [16]), lambda: K.lpips_fold(part, 2, [2], [0]), lambda: K.lpips_fold(part.float(), 2, [2], [16]),
           lambda: K.lpips_fold(part, 2, [1] * 9, [1] * 9), lambda: K.lpips_fold(part, 2, [2], [16, 16])]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")
