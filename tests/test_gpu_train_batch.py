"""Training batches built on the device (csrc/train_batch.hip: cdfo_train_batch; cdfo_amd/train_data.py::ClipSet.batch) against the REAL
reference's outputs (tests/golden/train_batch_ref.npz) and against the numpy statement (tests/train_batch_ref.py), which
tests/test_train_batch_cpu.py pins to that fixture.  Every comparison is exact (np.array_equal: infinities in place, sign included)."""
import numpy as np
import pytest
import torch

import train_batch_ref as R
from test_train_batch_cpu import OUTPUTS, fixture_arrays

pytestmark = pytest.mark.gpu
ORDER = ("lr", "pms", "rms", "ufs", "mvl0", "hr")
SHAPES = {"x": lambda B, c: (B, 7, 1, c, c), "mvs0": lambda B, c: (B, 7, 2, c, c), "mvs1": lambda B, c: (B, 7, 2, c, c),
          "pms": lambda B, c: (B, 7, 1, c, c), "rms": lambda B, c: (B, 1, 7, c, c), "ufs": lambda B, c: (B, 1, 7, c, c),
          "hr": lambda B, c: (B, 1, 4 * c, 4 * c)}


def random_arrays(S, T, H, W, seed):
    """Every value of the storage types, motion-field reference components in -2..2 (zeros under zero and non-zero vectors)."""
    rs = np.random.RandomState(seed)
    u8 = lambda *s: rs.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    mv = rs.randint(-128, 128, (S, T, H, W, 3)).astype(np.int8)
    mv[..., 2] = rs.randint(-2, 3, (S, T, H, W))
    mv[:, :, ::3, ::2, :2] = 0
    return dict(lr=u8(S, T, H, W), pms=u8(S, T, H, W), rms=rs.randint(-128, 128, (S, T, H, W)).astype(np.int8), ufs=u8(S, T, H + 2, W),
                mvl0=mv, hr=u8(S, T, 4 * H, 4 * W))


def check_batch(a, plan, crop):
    from cdfo_amd.train_data import ClipSet
    cs = ClipSet.from_arrays(*(a[k] for k in ORDER))
    got = dict(zip(OUTPUTS, cs.batch(plan, crop)))
    want = R.batch(*(a[k] for k in ORDER), plan, crop)
    B = len(plan)
    for k in OUTPUTS:
        t = got[k]
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == SHAPES[k](B, crop), k
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    assert not got["mvs1"].any()
    return cs, got, want


def test_fixture_cases_equal_the_reference_outputs():
    a, plans, crop, want = fixture_arrays()
    _, got, _ = check_batch(a, plans, crop)                    # all 16 cases as one batch of S = 1, T = 7
    assert np.isinf(want["mvs0"]).any()
    for k in OUTPUTS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


@pytest.mark.parametrize("crop", [8, 12])
def test_small_crops_equal_the_statement(crop):
    S, T, H, W = 3, 9, 22, 28
    a = random_arrays(S, T, H, W, 7 + crop)
    # all eight flag combinations over the two batches' rows; first in {0, T-7}; the four corners; sequence 1 twice in a batch
    rows = [(1, 0, 0, 0), (1, T - 7, H - crop, W - crop), (0, 0, H - crop, 0), (2, T - 7, 0, W - crop), (2, 1, 3, 5)]
    for base in (0, 3):
        plan = np.array([(s, f, t, l, (base + i) & 1, ((base + i) >> 1) & 1, ((base + i) >> 2) & 1, 0) for i, (s, f, t, l) in enumerate(rows)],
                        np.int32)
        _, _, want = check_batch(a, plan, crop)
        assert np.isinf(want["mvs0"]).any()
    assert {(base + i) & 7 for base in (0, 3) for i in range(5)} == set(range(8))


def test_crop_64_covers_several_tiles():
    S, T, H, W = 2, 7, 70, 72
    a = random_arrays(S, T, H, W, 11)
    plan = np.array([(1, 0, 6, 8, 1, 0, 1, 0), (0, 0, 1, 3, 0, 1, 0, 0)], np.int32)      # 2 x 2 tiles a plane, a 256 x 256 HR plane
    cs, got, _ = check_batch(a, plan, 64)
    plan2 = np.array([(0, 0, 0, 0, 1, 1, 1, 0), (1, 0, 5, 7, 0, 0, 1, 0)], np.int32)
    got2 = dict(zip(OUTPUTS, cs.batch(plan2, 64)))
    assert got2["mvs1"] is got["mvs1"]                                             # the cached zero tensor
    want2 = R.batch(*(a[k] for k in ORDER), plan2, 64)
    for k in OUTPUTS:
        assert np.array_equal(got2[k].cpu().numpy(), want2[k]), k


def test_invalid_plans_raise_before_any_launch(monkeypatch):
    from cdfo_amd import kernels as K
    from cdfo_amd.train_data import ClipSet
    cs = ClipSet.from_arrays(*(random_arrays(1, 7, 12, 16, 1)[k] for k in ORDER))
    launches = []
    monkeypatch.setattr(K, "train_batch", lambda *args: launches.append(args))
    good = (0, 0, 4, 8, 1, 0, 1, 0)
    for bad in ((1, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0), (0, 0, 5, 0, 0, 0, 0, 0), (0, 0, 0, 9, 0, 0, 0, 0),
                (0, 0, -1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 3, 0, 0)):
        with pytest.raises(ValueError):
            cs.batch(np.array([good, bad], np.int32), 8)
    for crop in (6, 10, 0):
        with pytest.raises(ValueError):
            cs.batch(np.array([(0, 0, 0, 0, 0, 0, 0, 0)], np.int32), crop)
    assert not launches
    monkeypatch.undo()
    # the wrapper's own checks, below ClipSet's: a crop that is no multiple of 4, a plan of the wrong type
    plan = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        K.train_batch(cs.lr, cs.pms, cs.rms, cs.ufs, cs.mvl0, cs.hr, plan, 6)
    with pytest.raises(ValueError):
        K.train_batch(cs.lr, cs.pms, cs.rms, cs.ufs, cs.mvl0, cs.hr, plan.long(), 8)


def test_a_device_batch_trains_the_model():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.loss import charbonnier
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    torch.manual_seed(0)
    cs = ClipSet.from_arrays(*synthetic_arrays(2, 7, 12, 16, seed=2))
    x, mvs0, mvs1, pms, rms, ufs, hr = cs.batch(cs.draw(2, np.random.default_rng(0), crop=8), 8)
    assert torch.isfinite(mvs0).all()
    m = CVSR_V8(SCGs=8).cuda().train()
    sr, _ = m(x, mvs0, mvs1, pms, rms, ufs)
    loss = charbonnier(sr, hr)
    loss.backward()
    assert loss.dim() == 0 and loss.is_cuda and bool(torch.isfinite(loss))
    grads = {k: p.grad for k, p in m.named_parameters()}
    none = sorted(k for k, g in grads.items() if g is None)
    assert all(k.startswith("MV_deform_align.fusion_in") for k in none), none       # never called by the reference forward either
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)
