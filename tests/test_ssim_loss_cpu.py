"""The SSIM / MS-SSIM losses without a GPU: the two fp64 statements of tests/ssim_loss_ref.py against each other, the statement's
identities, the numpy restatement of the kernels' tiling (tests/ssim_loss_model.py) against the derived bounds with and without its
defects, and the argument checks of the new entry points, of the public functions and of `train.fit`'s new keywords, none of which
may reach the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssim_loss_cases as cases
import ssim_loss_model as tiled
import ssim_loss_ref as ref


@pytest.mark.parametrize("c", cases.CASES + (cases.CLAMP,), ids=cases.case_id)
def test_the_two_statements_agree(c):
    levels, peak = c[0], c[5]
    l64, _, m64, _ = cases.reference(c)
    l2, m2 = ref.numpy_statement(*cases.case(c), peak, levels)
    print("%s: loss %.2g, means %.2g apart" % (cases.case_id(c), np.abs(l2 - l64).max(), np.abs(m2 - m64).max()))
    assert np.abs(l2 - l64).max() <= 1e-12 and np.abs(m2 - m64).max() <= 1e-12


def test_statement_identities():
    c = cases.SSIM_CASES[12]
    sr, hr = cases.case(c)
    # 1 - loss is the evaluators' SSIM; the pool is the defined rounding; identical frames; the clamp
    from oracle.metrics_ref import calculate_ssim
    l255 = ref.statement(sr * np.float32(255), hr * np.float32(255), 255.0)[0]
    for n in range(len(sr)):
        want = calculate_ssim((sr[n] * np.float32(255)).astype(np.float64), (hr[n] * np.float32(255)).astype(np.float64), 0)
        assert abs((1 - l255[n]) - want) <= 1e-12
    x = torch.from_numpy(cases.case(cases.MS_CASES[2])[0].astype(np.float64))
    assert np.array_equal(ref.pool(x).numpy(), np.stack([ref.pool_numpy(f.numpy().astype(np.float32)) for f in x]).astype(np.float64))
    loss, g, _, _ = ref.statement(hr, hr)
    assert np.abs(loss).max() <= 1e-12 and np.abs(g).max() <= 1e-12
    loss, g, means, coef = cases.reference(cases.CLAMP)
    assert (means[:, :4, 0] < 0).all() and (loss == 1.0).all() and not g.any() and not coef.any()


@pytest.mark.parametrize("c", cases.CASES + (cases.CLAMP,), ids=cases.case_id)
def test_tiled_model_meets_the_bounds(c):
    levels, _, _, n, _, peak = c
    sr, hr = cases.case(c)
    l64, g64, _, _ = cases.reference(c)
    loss, g = tiled.model(sr, hr, peak, levels, cases.upstream(n))
    rl, rg = cases.loss_ratio(loss, l64), cases.grad_ratio(g, g64)
    print("%s: tiled model measured / bound: loss %.3f, gradient %.3f" % (cases.case_id(c), rl, rg))
    assert rl <= 1 and rg <= 1
    if c == cases.CLAMP:
        assert (loss == 1.0).all() and not g.any()
    same_l, same_g = tiled.model(hr, hr, peak, levels)
    assert np.abs(same_l).max() <= 1e-9 and np.abs(same_g).max() <= 1e-9 / peak


_S = {(c[1], c[2], c[3], c[4], c[5]): c for c in cases.CASES}
# defect -> a case whose bound it misses, and whether the loss shows it (the gradient always does)
_SHOWS = {
    "halo-short": (_S[64, 64, 1, 0.5, 1.0], True),
    "centre-off": (_S[21, 21, 1, 0.5, 1.0], True),
    "adjoint-valid": (_S[11, 12, 1, 0.5, 1.0], False),
    "skip-partial": (_S[11, 11, 1, 0.05, 1.0], True),
    "pool-odd-row": (_S[177, 191, 2, 0.5, 1.0], False),
    "spread-one": (_S[176, 176, 2, 0.5, 1.0], False),
    "q-without-2": (_S[21, 21, 3, 0.05, 1.0], False),
    "c1-c2-swapped": (_S[43, 75, 3, 0.05, 255.0], True),
    "clamp-gradient": (cases.CLAMP, False),
    "level4-cs": (_S[200, 233, 2, 0.5, 1.0], True),
}
PROBE = np.arange(1.0, 12.0) / 66.0                                            # an asymmetric window of sum 1


@pytest.mark.parametrize("defect", tiled.DEFECTS)
def test_every_defect_of_the_tiled_model_misses_a_bound(defect):
    if defect == "adjoint-no-flip":
        # the Gaussian is symmetric: the defect is invisible there, so the model and the statement run with an asymmetric window
        c = _S[43, 75, 1, 0.5, 1.0]
        sr, hr = cases.case(c)
        l64, g64, _, _ = ref.statement(sr, hr, 1.0, 1, cases.upstream(1).astype(np.float64), g=PROBE)
        loss, g = tiled.model(sr, hr, 1.0, 1, cases.upstream(1), g=PROBE)
        assert cases.loss_ratio(loss, l64) <= 1 and cases.grad_ratio(g, g64) <= 1
        loss, g = tiled.model(sr, hr, 1.0, 1, cases.upstream(1), defects=(defect,), g=PROBE)
        assert cases.loss_ratio(loss, l64) <= 1 and cases.grad_ratio(g, g64) > 1
        loss, g = tiled.model(sr, hr, 1.0, 1, cases.upstream(1), defects=(defect,))
        assert cases.grad_ratio(g, cases.reference(c)[1]) <= 1
        return
    c, in_loss = _SHOWS[defect]
    levels, _, _, n, _, peak = c
    l64, g64, _, _ = cases.reference(c)
    loss, g = tiled.model(*cases.case(c), peak, levels, cases.upstream(n), defects=(defect,))
    rl, rg = cases.loss_ratio(loss, l64), cases.grad_ratio(g, g64)
    print("%s on %s: measured / bound: loss %.3g, gradient %.3g" % (defect, cases.case_id(c), rl, rg))
    assert rg > 1 and (rl > 1) == in_loss


def test_argument_validation_needs_no_gpu():
    """CDFO_EINVAL (-1) from every new entry point before any HIP call: the pointers below are never dereferenced."""
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    lib = _lib.lib()
    p, odd = C.c_void_p(4096), C.c_void_p(4100)                             # non-null, aligned / 4-byte aligned only; never touched
    big = 1 << 40
    for h, w, levels in ((11, 11, 1), (59, 91, 1), (64, 64, 1), (176, 176, 5), (177, 191, 5), (200, 233, 5)):
        assert lib.cdfo_ssim_loss_tiles(h, w, levels) == K.ssim_loss_tiles(h, w, levels) > 0
    assert lib.cdfo_ssim_loss_tiles(11, 11, 1) == 1 and lib.cdfo_ssim_loss_tiles(59, 91, 1) == 12 and lib.cdfo_ssim_loss_tiles(176, 176, 5) == 89

    def level(x=p, y=p, N=1, H=64, W=64, levels=1, lv=0, peak=1.0, partial=p, cap=big):
        return lib.cdfo_ssim_loss_level(x, y, N, H, W, levels, lv, peak, partial, cap, None)

    def pool(x=p, y=p, N=1, h=64, w=64, xn=p, yn=p):
        return lib.cdfo_ssim_loss_pool(x, y, N, h, w, xn, yn, None)

    def combine(partial=p, cap=big, N=1, H=64, W=64, levels=1, means=p, coef=p, loss=p):
        return lib.cdfo_ssim_loss_combine(partial, cap, N, H, W, levels, means, coef, loss, None)

    def pqr(x=p, y=p, N=1, H=64, W=64, levels=1, lv=0, peak=1.0, coef=p, out=p, cap=big):
        return lib.cdfo_ssim_loss_pqr(x, y, N, H, W, levels, lv, peak, coef, out, cap, None)

    def adjoint(maps=p, x=p, y=p, N=1, H=64, W=64, levels=1, lv=0, coarse=p, g64=p, g32=p):
        return lib.cdfo_ssim_loss_adjoint(maps, x, y, N, H, W, levels, lv, coarse, g64, g32, None)

    for f, names in ((level, ("x", "y", "partial")), (pool, ("x", "y", "xn", "yn")), (combine, ("partial", "means", "coef", "loss")),
                     (pqr, ("x", "y", "coef", "out")), (adjoint, ("maps", "x", "y", "g32"))):
        for name in names:                                                   # each pointer null in turn
            assert f(**{name: None}) == -1, (f.__name__, name)
        for n in (0, -1, 65536):
            assert f(N=n) == -1
    assert adjoint(H=200, W=200, levels=5, lv=2, g64=None) == -1 and adjoint(H=200, W=200, levels=5, lv=2, coarse=None) == -1
    for f in (level, combine, pqr, adjoint):
        for kw in (dict(H=10), dict(W=10), dict(H=16385), dict(W=16385), dict(levels=0), dict(levels=2), dict(levels=6),
                   dict(levels=5, H=175, W=300), dict(levels=5, H=300, W=175)):
            assert lib.cdfo_ssim_loss_tiles(kw.get("H", 64), kw.get("W", 64), kw.get("levels", 1)) == -1
            assert f(**kw) == -1, (f.__name__, kw)
    for f in (level, pqr, adjoint):
        assert f(lv=-1) == -1 and f(lv=1) == -1 and f(H=200, W=200, levels=5, lv=5) == -1
    for f in (level, pqr):
        for peak in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert f(peak=peak) == -1
    for kw in (dict(h=21), dict(w=21), dict(h=16385), dict(w=16385)):
        assert pool(**kw) == -1
    assert level(N=3, H=59, W=91, cap=2 * 3 * 12 - 1) == -1 and combine(N=3, H=59, W=91, cap=2 * 3 * 12 - 1) == -1
    assert level(N=2, H=176, W=176, levels=5, lv=4, cap=2 * 2 * 89 - 1) == -1
    assert pqr(N=3, H=59, W=91, cap=3 * 3 * 49 * 81 - 1) == -1
    assert pqr(N=1, H=200, W=200, levels=5, lv=1, cap=3 * 90 * 90 - 1) == -1
    # CDFO_EALIGN (-2): fp64 arrays are 8-byte aligned
    assert level(partial=odd) == -2 and combine(means=odd) == -2 and pqr(out=odd) == -2 and adjoint(maps=odd) == -2
    assert pool(x=C.c_void_p(4098)) == -2


def test_python_refuses_before_any_device_work(monkeypatch):
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    from cdfo_amd.loss import msssim_loss, ssim_loss
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    a = torch.zeros(2, 1, 200, 200)
    for f in (ssim_loss, msssim_loss):
        with pytest.raises(NotImplementedError):
            f(a, a)
    with pytest.raises(ValueError):
        K.ssim_loss(a, a)                                                    # the wrappers take device tensors only
    for peak in (0, -1.0, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError):
            K.ssim_loss_peak(peak, "test")
    assert K.ssim_loss_peak(255, "test") == 255.0 and K.ssim_loss_peak(0.5, "test") == 0.5


def test_fit_refuses_before_any_device_work(tmp_path, monkeypatch):
    from cdfo_amd import _lib
    from cdfo_amd.train import fit
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    for kw in (dict(ssim_weight=-0.5), dict(ssim_weight=float("inf")), dict(ssim_weight=float("nan")), dict(ssim_weight=True),
               dict(ssim_weight="1"), dict(ssim_scales=5), dict(ssim_weight=0.0, ssim_scales=5), dict(ssim_weight=1.0, ssim_scales=2),
               dict(ssim_weight=1.0, ssim_scales=0), dict(ssim_weight=1.0, ssim_scales=True), dict(ssim_weight=1.0, ssim_scales=None),
               dict(ssim_weight=1.0, crop=2), dict(ssim_weight=1.0, ssim_scales=5, crop=43), dict(ssim_weight=1.0, ssim_scales=5, crop=16)):
        with pytest.raises(ValueError, match="ssim"):
            fit(None, None, 1, str(tmp_path / "never"), **kw)
    # the smallest crops pass the checks: the call gets as far as reading the clip set, which is None here
    for kw in (dict(ssim_weight=1.0, crop=3), dict(ssim_weight=1.0, ssim_scales=5, crop=44)):
        with pytest.raises(AttributeError, match="coding"):
            fit(None, None, 1, str(tmp_path / "never"), **kw)
    assert not (tmp_path / "never").exists()


def test_run_arguments_with_and_without_the_new_names():
    from cdfo_amd.train import RUN_ARGUMENTS, check_run_arguments, run_arguments
    assert RUN_ARGUMENTS[-2:] == ("ssim_weight", "ssim_scales") and len(RUN_ARGUMENTS) == 12
    old = run_arguments(2, 16, 1e-4, 1e-5, 1, "LD", 0.0, 0.0, 1.0, None)       # ten positionals: the call of before
    assert list(old) == list(RUN_ARGUMENTS) and old["ssim_weight"] == 0.0 and old["ssim_scales"] == 1
    new = run_arguments(2, 16, 1e-4, 1e-5, 1, "LD", 0.0, 0.0, 1.0, None, ssim_weight=0.5, ssim_scales=5)
    assert new["ssim_weight"] == 0.5 and new["ssim_scales"] == 5
    check_run_arguments(old, old)
    check_run_arguments(new, new)
    before = {k: v for k, v in old.items() if not k.startswith("ssim")}        # a state file written before the names existed
    check_run_arguments(before, old)
    with pytest.raises(ValueError, match="ssim_weight = 0.0, this call has ssim_weight = 0.5"):
        check_run_arguments(before, new)
    with pytest.raises(ValueError, match="ssim_weight = 0.5, this call has ssim_weight = 0.0"):
        check_run_arguments(new, old)
    with pytest.raises(ValueError, match="ssim_scales = 5, this call has ssim_scales = 1"):
        check_run_arguments(new, dict(new, ssim_scales=1))
    with pytest.raises(ValueError, match="does not record crop"):
        check_run_arguments({k: v for k, v in old.items() if k != "crop"}, old)
