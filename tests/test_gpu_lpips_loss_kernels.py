"""The four kernels csrc/lpips.hip adds for the training loss, run through their wrappers with every output prefilled with NaN (a
kernel that leaves an element unwritten shows), each against the statement's own autograd on the CPU (tests/lpips_loss_cases.py).

Float stem: the bits of the 8-bit stem.  Distance backward: fp64 arithmetic with one rounding, bounded by 16 x the gap measured
against the statement rounded to fp32.  Pool backward: a copy or +0, so bit-equal to ``torch.max_pool2d``'s CPU backward.  Stem
backward: 16 x the fp32 floor, the statement in fp32 against fp64 on the same inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import lpips_loss_cases as cases

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("C0", [16, 64])
@pytest.mark.parametrize("h,w", [(16, 16), (17, 19), (18, 35)])
@pytest.mark.parametrize("normalize", [True, False])
def test_float_stem_on_k_over_255_has_the_bits_of_the_8_bit_stem(h, w, C0, normalize):
    from cdfo_amd import kernels as K
    params = cases.model((C0, 16, 16, 16, 16), 23)
    w0, b0 = torch.from_numpy(np.array(params.weights[0])).cuda(), torch.from_numpy(np.array(params.biases[0])).cuda()
    k = np.random.RandomState(h * w + C0).randint(0, 256, (3, h + 3, w + 5)).astype(np.uint8)
    # the division on the host: IEEE, correctly rounded (a device-side `/ 255` of torch may multiply by a reciprocal)
    k, x = torch.from_numpy(k).cuda(), torch.from_numpy(k.astype(np.float32) / np.float32(255)).cuda()
    want = K.lpips_stem(k[:, :h, :w].contiguous(), w0, b0, normalize)
    got = K.lpips_stem_f32(x[:, :h, :w].contiguous(), w0, b0, normalize, out=_nan(3, h, w, C0))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool((want > 0).any())
    # a region read in place: pitch w + 5, frame stride (h + 3) (w + 5), an odd first column
    want = K.lpips_stem(k[:, 2:2 + h, 3:3 + w], w0, b0, normalize)
    got = K.lpips_stem_f32(x[:, 2:2 + h, 3:3 + w], w0, b0, normalize, out=_nan(3, h, w, C0))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got, K.lpips_stem_f32(x[:, 2:2 + h, 3:3 + w].contiguous(), w0, b0, normalize))


# The worst gap of cdfo_lpips_dist_bwd to the fp64 statement rounded to fp32, as a fraction of the largest |gradient|, over every case
# below as measured on the MI355X: 0 in all thirty -- the device's fp64 sums run in another order than torch's, which moves a value by
# a few 1e-16 of itself, and the one rounding to fp32 hides that unless the value lies that close to a rounding boundary (about one
# element in 1e8).  Asserted: 16 x the measured gap, which is bit equality with the rounded statement.
DIST_BWD_GAP = 0.0


@pytest.mark.parametrize("Cc", [16, 48, 64, 80, 512])
def test_distance_backward_matches_autograd_on_the_statement(Cc):
    """Measured on the MI355X: a worst gap of 0 (DIST_BWD_GAP above) over C of 16, 48, 64, 80, 512 on 1 x 1, 3 x 5 and 9 x 17, with
    and without gin: every element has the bits of the fp64 statement rounded to fp32."""
    from cdfo_amd import kernels as K
    dev = lambda a: torch.from_numpy(a).cuda()
    for h, w in ((1, 1), (3, 5), (9, 17)):
        pre, fa, fb, lin, gscale, gin = cases.dist_case(Cc, h, w)
        for arrives in (None, gin):
            want = cases.dist_bwd_autograd(pre, fb, lin, gscale, arrives)
            got = K.lpips_dist_bwd(dev(fa), dev(fb), dev(lin), dev(gscale), None if arrives is None else dev(arrives),
                                   out=_nan(*fa.shape)).cpu().numpy()
            assert np.isfinite(got).all() and np.isfinite(want).all()                       # the NaN under a non-positive fa is dropped
            assert not got[0, 0, 0].any() and not np.signbit(got[fa <= 0]).any()            # the all-zero pixel; +0 under the select
            assert np.abs(want[-1, -1, -1]).max() > 0                                       # the pixel all zero in fb has a gradient
            if arrives is None:
                assert not got[1].any()                                                      # the frame with gscale 0
            gap = np.abs(got - want.astype(np.float32)).max() / np.abs(want).max()
            print(f"C = {Cc}, {h}x{w}, gin {arrives is not None}: gap to the rounded statement {gap:.3g} of max |g|")
            assert gap <= 16 * DIST_BWD_GAP
            again = K.lpips_dist_bwd(dev(fa), dev(fb), dev(lin), dev(gscale), None if arrives is None else dev(arrives)).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("Cc", [4, 64])
@pytest.mark.parametrize("H,W", [(2, 2), (3, 3), (5, 8), (17, 19)])
def test_pool_backward_is_bit_equal(H, W, Cc):
    from cdfo_amd import kernels as K
    x, g = cases.pool_case(H, W, Cc)
    want = cases.torch_pool2_bwd(x, g)
    got = K.lpips_pool2_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), out=_nan(2, H, W, Cc)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[:, H // 2 * 2:].view(np.uint32).any() and not got[:, :, W // 2 * 2:].view(np.uint32).any()      # +0, bit for bit
    assert np.count_nonzero(got) == g.size - np.count_nonzero(g == 0)


@pytest.mark.parametrize("C0", [16, 64])
@pytest.mark.parametrize("h,w", [(16, 16), (17, 19), (18, 35)])
@pytest.mark.parametrize("normalize", [True, False])
def test_stem_backward_matches_the_statement(h, w, C0, normalize):
    from cdfo_amd import kernels as K, metrics as M
    w0, g, want, floor = cases.stem_bwd_case(h, w, C0, normalize)
    wf = torch.from_numpy(M.lpips_stem_adjoint(w0, normalize)).cuda()
    got = K.lpips_stem_bwd(torch.from_numpy(g).cuda(), wf, out=_nan(2, h, w)).cpu().numpy()
    err = cases.err(got, want)
    print(f"C0 = {C0}, {h}x{w}, normalize {normalize}: {err:.3g} of max |g|, fp32 floor {floor:.3g}")
    assert np.isfinite(got).all() and err <= 16 * floor


def test_every_einval_is_reached_without_a_launch():
    from cdfo_amd import _lib
    lib = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    x, out = torch.zeros(2 * 4 * 4 * 16, device="cuda"), _nan(2 * 4 * 4 * 16)
    lin, gs = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(2, device="cuda")
    X, O, L, G, Z, st = p(x), p(out), p(lin), p(gs), None, None
    s0 = C.c_longlong(16)
    calls = [
        lib.cdfo_lpips_stem_f32(Z, 4, s0, 2, 4, 4, X, X, 16, 1, O, st), lib.cdfo_lpips_stem_f32(X, 4, s0, 2, 4, 4, Z, X, 16, 1, O, st),
        lib.cdfo_lpips_stem_f32(X, 4, s0, 2, 4, 4, X, Z, 16, 1, O, st), lib.cdfo_lpips_stem_f32(X, 4, s0, 2, 4, 4, X, X, 16, 1, Z, st),
        lib.cdfo_lpips_stem_f32(X, 4, s0, 0, 4, 4, X, X, 16, 1, O, st), lib.cdfo_lpips_stem_f32(X, 4, s0, 2, 0, 4, X, X, 16, 1, O, st),
        lib.cdfo_lpips_stem_f32(X, 3, s0, 2, 4, 4, X, X, 16, 1, O, st), lib.cdfo_lpips_stem_f32(X, 4, C.c_longlong(-1), 2, 4, 4, X, X, 16, 1, O, st),
        lib.cdfo_lpips_stem_f32(X, 4, s0, 2, 4, 4, X, X, 8, 1, O, st), lib.cdfo_lpips_stem_f32(X, 4, s0, 2, 4, 4, X, X, 272, 1, O, st),
        lib.cdfo_lpips_stem_f32(X, 4, s0, 65536, 4, 4, X, X, 16, 1, O, st), lib.cdfo_lpips_stem_f32(X, 65536, s0, 2, 65536, 4, X, X, 16, 1, O, st),
        lib.cdfo_lpips_dist_bwd(Z, X, L, G, Z, 2, 4, 4, 16, O, st), lib.cdfo_lpips_dist_bwd(X, Z, L, G, Z, 2, 4, 4, 16, O, st),
        lib.cdfo_lpips_dist_bwd(X, X, Z, G, Z, 2, 4, 4, 16, O, st), lib.cdfo_lpips_dist_bwd(X, X, L, Z, Z, 2, 4, 4, 16, O, st),
        lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 2, 4, 4, 16, Z, st), lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 0, 4, 4, 16, O, st),
        lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 65536, 4, 4, 16, O, st), lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 2, 0, 4, 16, O, st),
        lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 2, 4, 0, 16, O, st), lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 2, 4, 4, 8, O, st),
        lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 2, 4, 4, 0, O, st), lib.cdfo_lpips_dist_bwd(X, X, L, G, Z, 2, 65536, 65536, 16, O, st),
        lib.cdfo_lpips_pool2_bwd(Z, X, 2, 4, 4, 16, O, st), lib.cdfo_lpips_pool2_bwd(X, Z, 2, 4, 4, 16, O, st),
        lib.cdfo_lpips_pool2_bwd(X, X, 2, 4, 4, 16, Z, st), lib.cdfo_lpips_pool2_bwd(X, X, 0, 4, 4, 16, O, st),
        lib.cdfo_lpips_pool2_bwd(X, X, 2, 1, 4, 16, O, st), lib.cdfo_lpips_pool2_bwd(X, X, 2, 4, 1, 16, O, st),
        lib.cdfo_lpips_pool2_bwd(X, X, 2, 4, 4, 6, O, st), lib.cdfo_lpips_pool2_bwd(X, X, 2, 4, 4, 0, O, st),
        lib.cdfo_lpips_pool2_bwd(X, X, 1 << 30, 64, 64, 16, O, st),
        lib.cdfo_lpips_stem_bwd(Z, X, 2, 4, 4, 16, O, st), lib.cdfo_lpips_stem_bwd(X, Z, 2, 4, 4, 16, O, st),
        lib.cdfo_lpips_stem_bwd(X, X, 2, 4, 4, 16, Z, st), lib.cdfo_lpips_stem_bwd(X, X, 0, 4, 4, 16, O, st),
        lib.cdfo_lpips_stem_bwd(X, X, 65536, 4, 4, 16, O, st), lib.cdfo_lpips_stem_bwd(X, X, 2, 0, 4, 16, O, st),
        lib.cdfo_lpips_stem_bwd(X, X, 2, 4, 0, 16, O, st), lib.cdfo_lpips_stem_bwd(X, X, 2, 4, 4, 8, O, st),
        lib.cdfo_lpips_stem_bwd(X, X, 2, 4, 4, 272, O, st), lib.cdfo_lpips_stem_bwd(X, X, 2, 65536, 65536, 16, O, st),
        lib.cdfo_lpips_stem_bwd(X, X, 2, 1048592, 4, 16, O, st),
    ]
    assert calls == [-1] * len(calls)                                                       # CDFO_EINVAL, each of them
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                                     # and nothing was launched on the output


def test_wrappers_refuse_before_any_launch():
    from cdfo_amd import kernels as K
    x, lin, gs = torch.zeros((2, 4, 4, 16), device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(2, device="cuda")
    f, w0, b0 = torch.zeros((2, 16, 16), device="cuda"), torch.zeros((16, 3, 3, 3), device="cuda"), torch.zeros(16, device="cuda")
    wf = torch.zeros((16, 3, 3), device="cuda")
    bad = [lambda: K.lpips_stem_f32(f.double(), w0, b0), lambda: K.lpips_stem_f32(f.to(torch.uint8), w0, b0),
           lambda: K.lpips_stem_f32(f.transpose(1, 2), w0, b0), lambda: K.lpips_stem_f32(f, w0[:8], b0[:8]),
           lambda: K.lpips_dist_bwd(x, x[:1], lin, gs), lambda: K.lpips_dist_bwd(x, x, lin.float(), gs), lambda: K.lpips_dist_bwd(x, x, lin, gs[:1]),
           lambda: K.lpips_dist_bwd(x, x, lin, gs.double()), lambda: K.lpips_dist_bwd(x, x, lin, gs, x[:, :2]),
           lambda: K.lpips_dist_bwd(x[..., :8].contiguous(), x[..., :8].contiguous(), lin[:8], gs), lambda: K.lpips_dist_bwd(x, x, lin, gs.cpu()),
           lambda: K.lpips_dist_bwd(x, x, lin, gs, out=x.double()),
           lambda: K.lpips_pool2_bwd(x, x), lambda: K.lpips_pool2_bwd(x[:, :1], x[:, :1, :2]), lambda: K.lpips_pool2_bwd(x.double(), x[:, :2, :2]),
           lambda: K.lpips_pool2_bwd(x, x[:, :2, :2, :8]), lambda: K.lpips_pool2_bwd(x, x[:, :2, :2].contiguous(), out=x[:, :2]),
           lambda: K.lpips_stem_bwd(x, wf.double()), lambda: K.lpips_stem_bwd(x, wf[:8]), lambda: K.lpips_stem_bwd(x[..., :8].contiguous(), wf[:8]),
           lambda: K.lpips_stem_bwd(x, wf.cpu()), lambda: K.lpips_stem_bwd(x, wf, out=torch.zeros((2, 4, 5), device="cuda"))]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")
