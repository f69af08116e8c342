"""The tOF kernels (csrc/tof.hip) on the GPU, each against its stage of the numpy statement (tests/tof_ref.py).  Every kernel is fed
the STATEMENT's inputs for that stage, so no difference upstream can move a bound.

Shapes: 32 x 32 (one stage), 33 x 47 (narrower than a tile of any kernel), 69 x 131 (two stages, 34 x 66 below) and 259 x 301 (all four
stages).  Three pairs are in flight with different content per pair; the frames are read in place out of a larger buffer with other
content behind their edges.

Bounds: measured on one MI355X over every case below, then 16 x the worst asserted.  The kernels follow the statement term by term
(every sum in the statement's order from 0.0, IEEE division and square root); what is left is the compiler fusing some multiply-adds
(the library's build flag disregards the file's contraction pragma), one rounding where numpy has two.  Measured worst absolute
differences: level images 1.14e-13 on samples of 0 .. 255 (equal bits at stage 0, where the taps are powers of two); coefficient
planes 5.6e-14 on values up to 34; normal equations 4.2e-16 of the largest value of their case (1.8e-12 on values up to 8044 with
the hand-made flow); solved flows 1.8e-15 px and resized flows 2.7e-15 px on flows up to 5 px.  The endpoint mean is compared with
`np.mean`, whose order of adding differs: its bound is derived in the test (measured: equal).  No pixel is left out of a comparison."""
import functools

import numpy as np
import pytest
import torch

import tof_ref as ref
from test_tof_cpu import pattern

pytestmark = pytest.mark.gpu
SHAPES = [(32, 32), (33, 47), (69, 131), (259, 301)]
PAIRS = 3
LEVEL_ABS = 16 * 1.14e-13                                # on samples of 0 .. 255
POLY_ABS = 16 * 5.6e-14                                  # on coefficients up to 34
MATRICES_REL = 16 * 4.2e-16                              # of the largest value of the case
FLOW_ABS = 16 * 2.7e-15                                  # px, on flows up to 5 px


@functools.lru_cache(maxsize=None)
def frames(shape):
    """uint8 [4,H,W]: four frames of one moving pattern plus noise; pair j is (frame j, frame j + 1)."""
    H, W = shape
    c = pattern(H + 16, W + 16, 7 + H)
    rs = np.random.RandomState(H * W)
    out = []
    for j, (oy, ox) in enumerate(((8, 8), (7, 10), (9, 11), (6, 9))):
        f = c[oy:oy + H, ox:ox + W].astype(np.int64) + rs.randint(-3, 4, (H, W)) + 4 * j
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    out = np.stack(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stages(shape):
    """Per stage of the statement on the three pairs: dict(k, h, w, img [3,2,h,w], R [3,2,5,h,w], flow_in [3,h,w,2] or None, Ms
    (the three M [3,5,h,w] the iterations see), flows (the three solved flows [3,h,w,2]))."""
    f = frames(shape)
    out, flow = [], None
    for k, h, w in ref.levels(*shape):
        img = np.stack([np.stack([ref.level_image(f[j], k, h, w), ref.level_image(f[j + 1], k, h, w)]) for j in range(PAIRS)])
        R = np.stack([np.stack([ref.polyexp(img[j, 0]), ref.polyexp(img[j, 1])]) for j in range(PAIRS)])
        prev_flow = flow
        flow_in = None if flow is None else np.stack([ref.flow_up(flow[j], h, w) for j in range(PAIRS)])
        cur = np.zeros((PAIRS, h, w, 2)) if flow_in is None else flow_in
        Ms, flows = [], []
        for i in range(ref.ITERATIONS):
            Ms.append(np.stack([ref.matrices(R[j, 0], R[j, 1], cur[j]) for j in range(PAIRS)]))
            cur = np.stack([ref.blur_solve(Ms[-1][j]) for j in range(PAIRS)])
            flows.append(cur)
        flow = cur
        out.append(dict(k=k, h=h, w=w, img=img, R=R, prev_flow=prev_flow, flow_in=flow_in, Ms=Ms, flows=flows))
    return out


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def report(what, got, want):
    """Prints and returns the worst absolute difference over EVERY element; shapes must agree."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all()
    worst = float(np.abs(got - want).max())
    print(f"{what}: worst |device - statement| {worst:.3e} on values up to {np.abs(want).max():.3e}; "
          f"{int((got.view(np.uint64) != want.view(np.uint64)).sum())} of {want.size} differ in bits")
    return worst


def framed(shape):
    """The four frames inside a [6,H+5,W+9] device buffer of other content: a view with a frame stride and a pitch of its own."""
    H, W = shape
    buf = np.random.RandomState(3).randint(0, 256, (6, H + 5, W + 9)).astype(np.uint8)
    buf[1:5, :H, :W] = frames(shape)
    view = up(buf)[1:5, :H, :W]
    assert not view.is_contiguous()
    return view


@pytest.mark.parametrize("shape", SHAPES)
def test_level_images(shape):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    v = framed(shape)
    carry = up(frames(shape)[0])
    worst = 0.0
    for st in stages(shape):
        taps = M.tof_taps(st["k"])
        got = K.tof_level(v[:3], v[1:], st["h"], st["w"], taps)
        worst = max(worst, report(f"{shape} stage {st['k']} level images", got, st["img"]))
        # the chunk form: pair 0's previous frame is the carried frame, pair j's is frame j - 1 of the same stack
        chunk = K.tof_level(v[1:], v[1:], st["h"], st["w"], taps, first=carry)
        assert torch.equal(chunk, got)
    assert worst <= LEVEL_ABS


@pytest.mark.parametrize("shape", SHAPES)
def test_polyexp(shape):
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    worst = 0.0
    for st in stages(shape):
        got = K.tof_polyexp(up(st["img"]), M.tof_poly_kernels())
        worst = max(worst, report(f"{shape} stage {st['k']} coefficient planes", got, st["R"]))
    assert worst <= POLY_ABS


def hand_made_flow(h, w):
    """fp64 [3,h,w,2]: samples leaving the frame on each side, exact integers, fx = w - 1 and fy = h - 1 exactly, negative
    fractions, and the positions just inside each edge; a different mixture per pair."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rs = np.random.RandomState(h * 1000 + w)
    out = []
    for j in range(PAIRS):
        dx, dy = rs.uniform(-3.0, 3.0, (h, w)), rs.uniform(-3.0, 3.0, (h, w))
        dx[:, :3] -= 2.5 + j                              # leaves on the left
        dx[:, -3:] += 2.5 + j                             # ... on the right
        dy[:3, 8:-8] -= 3.5                               # ... at the top
        dy[-3:, 8:-8] += 3.5                              # ... at the bottom
        dx[10:14], dy[10:14] = 2.0, -1.0                  # exact integers
        dx[15], dy[15] = (w - 1) - x[15], 0.0             # fx = w - 1 exactly: outside
        dx[16], dy[16] = (w - 2) - x[16], 0.25            # fx = w - 2: the last position inside
        dx[17], dy[17] = -0.25, -1.75                     # negative fractions
        dx[:, 20], dy[:, 20] = 0.5, (h - 1) - y[:, 20]    # fy = h - 1 exactly: outside
        dx[18], dy[18] = -x[18], -18.0                    # fx = 0, fy = 0 exactly: inside
        dx[19], dy[19] = -x[19] - 2.0 ** -40, 0.0         # just below 0: outside
        out.append(np.stack([dx, dy], axis=-1))
    return np.stack(out)


@pytest.mark.parametrize("shape", SHAPES)
def test_matrices(shape):
    from cdfo_amd import kernels as K
    worst = 0.0
    for st in stages(shape):
        R, h, w = st["R"], st["h"], st["w"]
        dR = up(R)
        cases = [("the flow the stage enters with", st["flow_in"], st["Ms"][0]),
                 ("the flow after the first iteration", st["flows"][0], st["Ms"][1])]
        hand = hand_made_flow(h, w)
        cases.append(("the hand-made flow", hand, np.stack([ref.matrices(R[j, 0], R[j, 1], hand[j]) for j in range(PAIRS)])))
        for what, flow, want in cases:
            got = K.tof_matrices(dR, None if flow is None else up(flow))
            worst = max(worst, report(f"{shape} stage {st['k']} normal equations, {what}", got, want) / np.abs(want).max())
    print(f"{shape} normal equations: worst difference relative to the largest value of its case {worst:.3e}")
    assert worst <= MATRICES_REL
    fx = np.arange(w)[None, None, :] + hand[..., 0]
    fy = np.arange(h)[None, :, None] + hand[..., 1]
    inside = (fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1)
    assert inside.any() and (fx < 0).any() and (fx >= w - 1).any() and (fy < 0).any() and (fy >= h - 1).any()
    assert (fx == w - 1).any() and (fy == h - 1).any() and ((fx == np.floor(fx)) & inside).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_solve(shape):
    from cdfo_amd import kernels as K
    worst = 0.0
    for st in stages(shape):
        for i in range(ref.ITERATIONS):
            got = K.tof_blur_solve(up(st["Ms"][i]))
            worst = max(worst, report(f"{shape} stage {st['k']} iteration {i} flow (px)", got, st["flows"][i]))
    assert worst <= FLOW_ABS


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_solve_of_a_constant(shape):
    """The box mean of a constant plane is that constant up to the rounding of 28 additions and one division (30 x 2^-53 relative
    per mean), and the solve then has a closed form; a different constant set per pair, the second with a zero matrix."""
    from cdfo_amd import kernels as K
    h, w = shape
    sets = np.array([[0.1, 0.03, 0.07, 0.013, -0.021], [0.0, 0.0, 0.0, 5.0, 7.0], [1e4, -2e3, 3e4, 1.5e3, -2.5e4]])
    M_ = np.broadcast_to(sets[:, :, None, None], (PAIRS, 5, h, w)).copy()
    got = K.tof_blur_solve(up(M_)).cpu().numpy()
    assert got.shape == (PAIRS, h, w, 2)
    for j, (g11, g12, g22, h1, h2) in enumerate(sets):
        idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
        want = np.array([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet])
        assert np.all(got[j] == got[j, 0, 0])                              # the same value at every pixel, edges included
        scale = (abs(g22 * h1) + abs(g12 * h2) + abs(g11 * h2) + abs(g12 * h1)) * abs(idet)
        # each flow component is a difference of two products of means times idet: 100 x 2^-53 of the terms' magnitudes covers
        # the three means and the roundings in each term; the determinant's own cancellation multiplies that by `cond`
        cond = (abs(g11 * g22) + abs(g12 * g12)) * abs(idet) + 1.0
        err = np.abs(got[j, 0, 0] - want).max()
        print(f"{shape} constant set {j}: flow {got[j, 0, 0]}, closed form {want}, |difference| {err:.2e}")
        assert err <= 100 * 2.0 ** -53 * scale * cond
    assert np.all(got[1] == 0.0)                                           # a zero matrix: the 1e-3 alone divides, the flow is 0


@pytest.mark.parametrize("shape", SHAPES[2:])
def test_flow_up(shape):
    from cdfo_amd import kernels as K
    worst = 0.0
    for st in stages(shape)[1:]:
        got = K.tof_flow_up(up(st["prev_flow"]), st["h"], st["w"])
        worst = max(worst, report(f"{shape} stage {st['k']} flow from the stage above", got, st["flow_in"]))
    assert worst <= FLOW_ABS


@pytest.mark.parametrize("shape", SHAPES)
def test_epe(shape):
    from cdfo_amd import kernels as K
    h, w = shape
    rs = np.random.RandomState(h + w)
    a, b = rs.uniform(-8.0, 8.0, (PAIRS, h, w, 2)), rs.uniform(-8.0, 8.0, (PAIRS, h, w, 2))
    b[1] = a[1]                                                             # equal flows: exactly 0
    b[2, :, :, 1] = a[2, :, :, 1]
    b[2, :, :, 0] = a[2, :, :, 0] + 0.5                                     # a constant distance: exactly 0.5
    got = K.tof_epe(up(a), up(b)).cpu().numpy()
    d = a - b
    want = np.array([np.mean(np.sqrt(d[j, ..., 0] * d[j, ..., 0] + d[j, ..., 1] * d[j, ..., 1])) for j in range(PAIRS)])
    rel = abs(got[0] - want[0]) / want[0]
    print(f"{shape} endpoint means: device {got}, np.mean {want}, relative difference {rel:.2e}")
    assert got.dtype == np.float64 and got.shape == (PAIRS,)
    bound = 2 * h * w * 2.0 ** -53                       # two orders of adding h w terms >= 0: each within (h w - 1) 2^-53 of the sum
    assert rel <= bound and got[1] == 0.0 and abs(got[2] - 0.5) <= 0.5 * bound
