"""BRISQUE on the CPU: the numpy statement of the definition (tests/brisque_ref.py) and the host pieces of cdfo_amd.metrics against
what the reference recorded in tests/golden/brisque_ref.npz (tools/gen_brisque_fixture.py: its 36 features and its score of five
frames, its model, and an all-zero frame it asserts on).

Measured on the committed fixture, fp64 statement against the reference's recorded fp32 values (the bounds below are 2 x these; both
sides are fixed data plus deterministic fp64 numpy, so the margin covers library last bits only):
    features   2.41e-05 relative  worst, frame c (a 2.24e-05, b 2.03e-05, d 6.87e-06, e 4.51e-06)          bound 4.82e-05
    scores     1.76e-03 absolute  worst, frame a (b 5.2e-04, c 8.3e-04, d 2.1e-04, e 1.4e-04), on 53 .. 96  bound 3.52e-03
    SVM step   1.74e-03 absolute  worst, frame a: `brisque_from_features` on the reference's OWN features    bound 3.48e-03
The SVM step alone accounts for the score's distance: the coefficients sum to 7.4e5 in magnitude, so the reference's fp32 kernel
sum is the floor.  The reference holds the ranges, gamma and rho in fp32 beside its float32 features, so its scores are compared
with the model rounded the same way (`brisque_ref.model(as_reference=True)`).  All ten table indices per frame are the reference's
(the generator asserts it, the first test repeats it); the statement's smallest relative gap between the two best distances is 2.1e-3."""
import os
import sys

import numpy as np
import pytest
import torch

import brisque_ref as ref

FEATURE_REL = 2 * 2.41e-05
SCORE_ABS = 2 * 1.76e-03
SVM_ABS = 2 * 1.74e-03


@pytest.mark.parametrize("name", ref.FRAMES)
def test_statement_matches_the_reference(name):
    z = ref.golden()
    p, G = ref.golden_pieces(name), z["features_" + name]
    F = p["features"]
    assert z["frame_" + name].shape == ref.SIZES[name] and F.shape == G.shape == (36,) and np.isfinite(F).all()
    assert np.array_equal(z["luma_" + name], z["frame_" + name])            # the luma the reference saw is the frame
    gam = ref.shared_table()[0]
    index = np.searchsorted(gam, G[list(ref.ALPHAS)])
    assert np.array_equal(gam[index], G[list(ref.ALPHAS)]) and np.array_equal(index, p["index"].reshape(-1))
    assert np.array_equal(F[list(ref.ALPHAS)], G[list(ref.ALPHAS)]) and p["gap"].min() > 1e-6
    rel = float(np.max(np.abs(F - G) / np.abs(G)))
    s = abs(ref.score(F, *ref.model(as_reference=True)) - float(z["score_" + name]))
    print(f"{name}: features {rel:.3e} relative, score {s:.3e} (fp64 model {abs(ref.score(F, *ref.model()) - float(z['score_' + name])):.3e})")
    assert rel <= FEATURE_REL < 1e-3
    assert s <= SCORE_ABS < 1e-2


@pytest.mark.parametrize("name", ref.FRAMES)
def test_from_features_reproduces_the_reference_scores(name):
    """The SVM step without the features in the way: the reference's own features in, its score out, to its fp32 sum's floor; and the
    project's function is the statement's, to the last bits of two fp64 sums of 774 terms of up to 2.4e3 (1e-9 leaves a margin)."""
    from cdfo_amd import metrics as M
    z = ref.golden()
    got = M.brisque_from_features(z["features_" + name], M.brisque_params(ref.model(as_reference=True)))
    print(f"{name}: SVM step {abs(got - z['score_' + name]):.3e}")
    assert got.shape == () and abs(got - z["score_" + name]) <= SVM_ABS
    assert abs(got - ref.score(z["features_" + name], *ref.model(as_reference=True))) <= 1e-9


def test_zero_frame_and_stacks():
    """The all-zero frame: every sample of every map is zero, so every search sees NaN (index 0, alpha gam[0]), the variances are 0,
    the other features and the score NaN -- where the reference asserts.  A stack scores frame by frame."""
    from cdfo_amd import metrics as M
    p, params = ref.golden_pieces("z"), M.brisque_params(ref.model())
    F = p["features"]
    gam0 = ref.shared_table()[0][0]
    assert (p["index"] == 0).all() and (F[list(ref.ALPHAS)] == gam0).all() and gam0 == np.float64(np.float32(0.2))
    assert F[1] == 0 and F[19] == 0 and np.isnan(np.delete(F, list(ref.ALPHAS) + [1, 19])).all()
    assert np.isnan(ref.score(F, *ref.model())) and np.isnan(M.brisque_from_features(F, params))
    both = M.brisque_from_features(torch.from_numpy(np.stack([ref.golden_pieces("c")["features"], F, ref.golden_pieces("d")["features"]])), params)
    assert both.dtype == np.float64 and both.shape == (3,) and np.isnan(both[1])
    assert both[0] == M.brisque_from_features(ref.golden_pieces("c")["features"], params)
    assert both[2] == M.brisque_from_features(ref.golden_pieces("d")["features"], params)
    with pytest.raises(ValueError):
        M.brisque_from_features(np.zeros((2, 35)), params)
    with pytest.raises(ValueError):
        ref.luma(np.zeros((15, 16), np.uint8))


def test_half_sizes_and_partners():
    """Odd sizes give ceil(n / 2) outputs; a constant image stays that constant (the taps sum to 1); the fourth partner is the
    sample BELOW and to the left, circular over the whole frame."""
    x = np.random.RandomState(1).rand(37, 83) * 255
    assert ref.half(x).shape == (19, 42) and ref.half(x[:16, :16]).shape == (8, 8)
    assert np.abs(ref.half(np.full((17, 21), 200.0)) - 200.0).max() < 1e-12
    # the last output of an odd size reads inputs n-4 .. n+3: the four beyond the edge mirror onto n-1 .. n-4
    n, col = 21, np.arange(21.0)[:, None] * np.ones((1, 16))
    want = sum(ref.HALF_TAPS[k] * [17, 18, 19, 20, 20, 19, 18, 17][k] for k in range(8))
    assert abs(ref.half(col)[(n - 1) // 2, 0] - want) < 1e-12
    m = np.arange(12.0).reshape(3, 4)
    assert ref.products(m)[4][0, 0] == m[0, 0] * m[1, 3] and ref.products(m)[4][2, 1] == m[2, 1] * m[0, 0]
    assert ref.products(m)[1][1, 0] == m[1, 0] * m[1, 3] and ref.products(m)[2][0, 2] == m[0, 2] * m[2, 2]
    assert ref.products(m)[3][0, 0] == m[0, 0] * m[2, 3]


def test_params_round_trip_and_refusals(tmp_path):
    from cdfo_amd import metrics as M
    sv, coef, ranges, gamma, rho = ref.model()
    np.savez(tmp_path / "m.npz", sv=sv, sv_coef=coef.reshape(-1, 1), feature_ranges=ranges, gamma=gamma, rho=rho)
    p = M.brisque_params(str(tmp_path / "m.npz"))
    assert isinstance(p, M.BrisqueParams) and p.sv.dtype == p.sv_coef.dtype == p.feature_ranges.dtype == np.float64
    assert np.array_equal(p.sv, sv) and np.array_equal(p.sv_coef, coef) and np.array_equal(p.feature_ranges, ranges)
    assert p.gamma == float(gamma) and p.rho == float(rho) and isinstance(p.gamma, float)
    q = M.brisque_params((sv.astype(np.float32), coef, ranges, gamma, rho))
    assert np.array_equal(q.sv, sv) and M.brisque_params(tuple(p)).rho == p.rho
    bad_range, nan_sv = ranges.copy(), sv.copy()
    bad_range[7, 1] = bad_range[7, 0]
    nan_sv[3, 3] = np.nan
    for args in ((sv[:, :35], coef, ranges, gamma, rho), (sv, coef[:-1], ranges, gamma, rho), (sv, coef, ranges[:35], gamma, rho),
                 (sv, coef, ranges.T, gamma, rho), (sv[:0], coef[:0], ranges, gamma, rho), (sv, coef, bad_range, gamma, rho),
                 (nan_sv, coef, ranges, gamma, rho), (sv, coef, ranges, np.inf, rho), (sv, coef, ranges, gamma, [1.0, 2.0]),
                 (sv, coef, ranges, gamma)):
        with pytest.raises(ValueError):
            M.brisque_params(args)
    np.savez(tmp_path / "k.npz", sv=sv, sv_coef=coef, feature_ranges=ranges, gamma=gamma)
    with pytest.raises(ValueError, match="rho"):
        M.brisque_params(str(tmp_path / "k.npz"))


def test_model_out_format(tmp_path):
    """What ``tools/gen_brisque_fixture.py --model-out`` writes is what `brisque_params` reads."""
    from cdfo_amd import metrics as M
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gen_brisque_fixture as gen
    finally:
        sys.path.remove(tools)
    z = ref.golden()
    gen.write_model(str(tmp_path / "user.npz"), z)
    p = M.brisque_params(str(tmp_path / "user.npz"))
    for got, want in zip(p, ref.model()):
        assert np.array_equal(got, want)
    with np.load(tmp_path / "user.npz") as f:
        assert sorted(f.files) == sorted(M.BrisqueParams._fields) and all(f[k].dtype == np.float64 for k in f.files)


def test_table_and_window():
    """The third row is the reference's expression evaluated with torch on the CPU, within the two lgamma implementations' last bits
    (1e-13 relative, as for NIQE's row); the first two rows are NIQE's table, the window NIQE's window."""
    from cdfo_amd import metrics as M
    t = M.brisque_table()
    gam = torch.arange(0.2, 10 + 0.001, 0.001).to(torch.float64)
    r = (torch.lgamma(1.0 / gam) + torch.lgamma(3.0 / gam) - 2 * torch.lgamma(2.0 / gam)).exp()
    assert t.shape == (3, M.BRISQUE_TABLE) == (3, 9801) and t.dtype == np.float64 and np.array_equal(t[:2], M.niqe_table())
    assert np.max(np.abs(t[2] - r.numpy()) / r.numpy()) <= 1e-13
    for k in range(3):
        assert np.array_equal(t[k], ref.shared_table()[k])
    assert (np.diff(t[2]) < 0).all()                                           # monotonic: one nearest entry but for exact ties
    assert np.array_equal(M.brisque_window(), ref.window())


def test_argument_validation_needs_no_gpu():
    """Every wrapper refuses host tensors and wrong sizes before it looks for the library or a device."""
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    w = M.brisque_window()
    u, d = torch.zeros((2, 32, 32), dtype=torch.uint8), torch.zeros((2, 32, 32), dtype=torch.float64)
    bad = [lambda: K.brisque_mscn(u, w), lambda: K.brisque_mscn(u.float(), w), lambda: K.brisque_half(u), lambda: K.brisque_half(d),
           lambda: K.brisque_sums(d), lambda: K.brisque_sums(d.float()), lambda: K.brisque_features(d.view(2, 1024), 1024, d, 0, None),
           lambda: M.brisque_features_u8(u), lambda: M.brisque_u8(u, ref.model()), lambda: M.brisque_scratch(0, 32, 32, "cpu"),
           lambda: M.brisque_scratch(2, 15, 16, "cpu"), lambda: M.brisque_size(16, 15),
           lambda: M.brisque_u8(u, (np.zeros((3, 35)), np.zeros(3), np.zeros((36, 2)), 0.05, 1.0))]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")
    assert M.brisque_size(16, 16) == (16, 16)


def test_result_fields_and_log_lines():
    from cdfo_amd import evaluate as E
    r = E.SequenceResult(np.array([30.0]), np.array([0.9]), 30.0, 0.9, 1, 0.5, 1.0)
    assert len(r.brisque) == 0 and np.isnan(r.mean_brisque) and E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000"
    r = r._replace(brisque=np.array([61.5]), mean_brisque=61.5)
    assert E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000 BRISQUE: 61.50000"
    r = r._replace(niqe=np.array([5.25]), mean_niqe=5.25, msssim=np.array([0.5]), mean_msssim=0.5)
    assert E.format_log(r, "s").endswith(" MS-SSIM: 0.50000 NIQE: 5.25000 BRISQUE: 61.50000")
    z = np.zeros(2)
    y = E.YuvResult(z, z, z, z, z, 31.0, 40.0, 41.0, 0.8, 33.375, 2, 0.5, 1.0)
    assert "BRISQUE" not in E.format_log_yuv(y, "s")
    assert E.format_log_yuv(y._replace(niqe=z, mean_niqe=4.0, brisque=z, mean_brisque=7.0), "s").endswith(" NIQE: 4.00000 BRISQUE: 7.00000")


def test_evaluators_refuse_before_any_device_work():
    """`evaluate._check_brisque`, the first thing both evaluators do with the option: above 8 bits and below 16 x 16 (after x4) it
    raises, as it does for a bad model; None is the option off."""
    from cdfo_amd import evaluate as E
    from cdfo_amd import metrics as M

    class Lr:
        dtype, peak, shape = torch.uint8, 255, (3, 4)

    class Lr10:
        dtype, peak, shape = torch.uint16, 1023, (48, 56)

    class LrFine:
        dtype, peak, shape = torch.uint8, 255, (4, 4)

    assert E._check_brisque(Lr, None) is None and isinstance(E._check_brisque(LrFine, ref.model()), M.BrisqueParams)
    with pytest.raises(ValueError, match="16 x 16"):
        E._check_brisque(Lr, ref.model())
    with pytest.raises(ValueError, match="8-bit"):
        E._check_brisque(Lr10, ref.model())
    with pytest.raises(ValueError, match="model"):
        E._check_brisque(LrFine, ref.model()[:4])
