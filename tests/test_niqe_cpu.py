"""NIQE on the CPU: the numpy statement of the definition (tests/niqe_ref.py) and the host pieces of cdfo_amd.metrics against what the
reference recorded in tests/golden/niqe_ref.npz (tools/gen_niqe_fixture.py: its per-block features and scores of six frames).

Measured on the committed fixture, statement against reference (the bounds below are 4 x these):
    scale-1 features   1.4e-14 relative   (both fp64, the summation order differs)             bound 1e-11, the issue's
    scale-2 features   4.02e-07 relative  (the reference resizes in fp32, the project in fp64)   bound 1.61e-06
    scores             8.09e-07 absolute  on scores of 13.5 .. 26.9                             bound 3.24e-06
The reference rounds the pristine model to fp32 (it moves it to the dtype of its float32 input), so its scores are compared with the
model rounded the same way (`niqe_ref.model(as_reference=True)`); with the fp64 model the scores differ by up to 6.6e-05, all of it
the model's rounding.  The flat block of frame c is flat with a margin of 16 samples: with only the 96 x 96 block flat, the windows at
its edge see the neighbouring blocks and none of its features is NaN."""
import numpy as np
import pytest
import torch

import niqe_ref as ref

SCALE1_REL = 1e-11
SCALE2_REL = 4 * 4.02e-07
SCORE_ABS = 4 * 8.09e-07


def _rel(F, G):
    return np.abs(F - G) / np.maximum(np.abs(G), 1e-3)


@pytest.mark.parametrize("name", ref.FRAMES)
def test_statement_matches_the_reference(name):
    z = ref.golden()
    F, G = ref.golden_pieces(name)["features"], z["features_" + name]
    assert F.shape == G.shape == ((z["frame_" + name].shape[0] // 96) * (z["frame_" + name].shape[1] // 96), 36)
    assert np.array_equal(np.isnan(F), np.isnan(G))
    assert np.array_equal(F[:, ref.ALPHAS], G[:, ref.ALPHAS])               # every alpha: the same table entry
    rel = _rel(F, G)
    s1, s2 = np.nanmax(rel[:, :18]), np.nanmax(rel[:, 18:])
    s = abs(ref.score(F, *ref.model(as_reference=True)) - float(z["score_" + name]))
    print(f"{name}: scale 1 {s1:.3e}, scale 2 {s2:.3e}, score {s:.3e} (fp64 model {abs(ref.score(F, *ref.model()) - float(z['score_' + name])):.3e})")
    assert s1 <= SCALE1_REL and s2 <= SCALE2_REL
    assert s <= SCORE_ABS < 1e-3


def test_flat_block_of_frame_c():
    """Block (1, 0), row 1: its MSCN samples are one constant of one sign, so every alpha is gam[0] (index 0 on NaN), the other
    features are NaN or the product of a tiny deviation, and the row leaves the covariance but not the means."""
    F, p = ref.golden_pieces("c")["features"], ref.golden_pieces("c")
    gam0 = ref.shared_table()[0][0]
    assert np.isnan(F).any(axis=1).tolist() == [False, True, False, False, False, False]
    assert (F[1, ref.ALPHAS] == gam0).all() and gam0 == np.float64(np.float32(0.2))
    assert (p["index"][:, 1] == 0).all()
    assert np.ptp(p["mscn1"][96:192, :96]) == 0 and np.ptp(p["mscn2"][48:96, :48]) == 0
    mu, cov = ref.model()
    full = ref.score(F, mu, cov)
    dropped = ref.score(np.delete(F, 1, axis=0), mu, cov)                      # the same covariance, other means
    assert np.isfinite(full) and abs(full - dropped) > 1e-3


@pytest.mark.parametrize("name", ref.FRAMES)
def test_from_features_reproduces_the_reference_scores(name):
    """nanmean, nancov and pinv without the resize in the way: the reference's own features in, its score out (1e-9 relative)."""
    from cdfo_amd import metrics as M
    z = ref.golden()
    got = M.niqe_from_features(z["features_" + name], M.niqe_params(ref.model(as_reference=True)))
    assert got.shape == () and abs(got - z["score_" + name]) <= 1e-9 * z["score_" + name]
    assert abs(got - ref.score(z["features_" + name], *ref.model(as_reference=True))) <= 1e-9 * z["score_" + name]


def test_from_features_stacks_and_edge_cases():
    from cdfo_amd import metrics as M
    z, p = ref.golden(), M.niqe_params(ref.model())
    both = M.niqe_from_features(torch.from_numpy(np.stack([z["features_b"], z["features_c"]])), p)
    assert both.dtype == np.float64 and both.shape == (2,)
    assert both[0] == M.niqe_from_features(z["features_b"], p) and both[1] == M.niqe_from_features(z["features_c"], p)
    one = z["features_e"]                                                      # one block: the zero covariance
    d = p.mu - one[0]
    assert M.niqe_from_features(one, p) == pytest.approx(np.sqrt(d @ np.linalg.pinv(p.cov / 2) @ d), rel=1e-12)
    assert np.isnan(M.niqe_from_features(z["features_c"][1:2], p))             # no complete block
    with pytest.raises(ValueError):
        M.niqe_from_features(np.zeros((2, 35)), p)


def test_params_round_trip_and_refusals(tmp_path):
    from cdfo_amd import metrics as M
    mu, cov = ref.model()
    np.savez(tmp_path / "m.npz", mu_prisparam=mu.reshape(1, 36), cov_prisparam=cov)
    p = M.niqe_params(str(tmp_path / "m.npz"))
    assert np.array_equal(p.mu, mu) and np.array_equal(p.cov, cov) and p.mu.dtype == p.cov.dtype == np.float64
    assert M.niqe_params(p) is not None and np.array_equal(M.niqe_params((mu, cov)).cov, cov)
    scipy_io = pytest.importorskip("scipy.io")
    scipy_io.savemat(str(tmp_path / "m.mat"), dict(mu_prisparam=mu.reshape(1, 36), cov_prisparam=cov))
    q = M.niqe_params(str(tmp_path / "m.mat"))
    assert np.array_equal(q.mu, mu) and np.array_equal(q.cov, cov)
    bad = cov.copy()
    bad[0, 1] += 1e-3
    for args in ((mu[:35], cov), (mu, cov[:35]), (mu, bad), (mu, np.where(np.eye(36) > 0, np.nan, cov))):
        with pytest.raises(ValueError):
            M.niqe_params(args)
    np.savez(tmp_path / "k.npz", mu_prisparam=mu)
    with pytest.raises(ValueError):
        M.niqe_params(str(tmp_path / "k.npz"))


def test_table_and_window():
    """The table is the reference's expression evaluated with torch on the CPU: gam the same numbers, r_gam within the two lgamma
    implementations' last bits (6 operations of at most 1 ulp each on values below 40: 1e-13 relative leaves a margin of ten)."""
    from cdfo_amd import metrics as M
    t = M.niqe_table()
    gam = torch.arange(0.2, 10 + 0.001, 0.001).to(torch.float64)
    r = (2 * torch.lgamma(2.0 / gam) - (torch.lgamma(1.0 / gam) + torch.lgamma(3.0 / gam))).exp()
    assert t.shape == (2, M.NIQE_TABLE) == (2, 9801) and t.dtype == np.float64
    assert np.array_equal(t[0], gam.numpy()) and np.array_equal(t[0], ref.shared_table()[0])
    assert np.max(np.abs(t[1] - r.numpy()) / r.numpy()) <= 1e-13 and np.array_equal(t[1], ref.shared_table()[1])
    assert (np.diff(t[0]) > 0).all() and (np.diff(t[1]) > 0).all()            # monotonic: one nearest entry but for exact ties
    w = M.niqe_window()
    assert np.array_equal(w, ref.window()) and np.array_equal(w, w.astype(np.float32)) and abs(w.sum() - 1) < 1e-7
    assert not np.allclose(w, np.outer(w.sum(1), w.sum(0)), rtol=0, atol=1e-12)   # not a separable product after the rounding


def test_region_and_result_fields():
    from cdfo_amd import evaluate as E
    from cdfo_amd import metrics as M
    assert M.niqe_region(200, 300) == (192, 288) and M.niqe_region(96, 96) == (96, 96)
    for h, w in ((95, 400), (400, 95), (80, 120)):
        with pytest.raises(ValueError):
            M.niqe_region(h, w)
    with pytest.raises(ValueError):
        ref.region(np.zeros((80, 120), np.uint8))
    r = E.SequenceResult(np.array([30.0]), np.array([0.9]), 30.0, 0.9, 1, 0.5, 1.0)
    assert len(r.niqe) == 0 and np.isnan(r.mean_niqe) and E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000"
    r = r._replace(niqe=np.array([5.25]), mean_niqe=5.25)
    assert E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000 NIQE: 5.25000"
    r = r._replace(msssim=np.array([0.5]), mean_msssim=0.5)
    assert E.format_log(r, "s").endswith(" MS-SSIM: 0.50000 NIQE: 5.25000")
    z = np.zeros(2)
    y = E.YuvResult(z, z, z, z, z, 31.0, 40.0, 41.0, 0.8, 33.375, 2, 0.5, 1.0)
    assert "NIQE" not in E.format_log_yuv(y, "s") and E.format_log_yuv(y._replace(niqe=z, mean_niqe=4.0), "s").endswith(" NIQE: 4.00000")
