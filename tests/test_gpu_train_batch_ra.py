"""Random-access training batches built on the device (csrc/train_batch_ra.hip: cdfo_train_batch_ra; ClipSet.batch with ``coding="RA"``)
against the REAL RA loader's outputs (tests/golden/train_batch_ra_ref.npz) and against the numpy statement
(tests/train_batch_ra_ref.py), which tests/test_train_batch_ra_cpu.py pins to that fixture.  Every comparison is exact and on bit
patterns (`RA.bits`): the arithmetic makes -0, the reference's output carries them, and ``np.array_equal`` on floats cannot see a
zero's sign."""
import numpy as np
import pytest
import torch

import train_batch_ra_ref as RA
from test_gpu_train_batch import SHAPES
from test_train_batch_cpu import OUTPUTS
from test_train_batch_ra_cpu import BOTH, ORDER, fixture_arrays

pytestmark = pytest.mark.gpu
PLANES = ("x", "pms", "rms", "ufs", "hr")
REFS = (-99, -99, 0, 1, 2, 3, -1, -2, 4, 8)       # the marker twice as likely as a value; zero; distances of both signs


def random_arrays(S, T, H, W, seed):
    """Every value of the storage types; both lists' reference components from REFS, over a lattice of zero vectors."""
    rs = np.random.RandomState(seed)
    u8 = lambda *s: rs.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    a = dict(lr=u8(S, T, H, W), pms=u8(S, T, H, W), rms=rs.randint(-128, 128, (S, T, H, W)).astype(np.int8), ufs=u8(S, T, H + 2, W),
             hr=u8(S, T, 4 * H, 4 * W))
    for k in ("mvl0", "mvl1"):
        mv = rs.randint(-128, 128, (S, T, H, W, 3)).astype(np.int8)
        mv[..., 2] = rs.choice(REFS, size=(S, T, H, W))
        mv[:, :, ::3, ::2, :2] = 0
        a[k] = mv
    return a


def ra_set(a):
    from cdfo_amd.train_data import ClipSet
    return ClipSet.from_arrays(*(a[k] for k in ORDER if k != "mvl1"), mvl1=a["mvl1"], coding="RA")


def covers_every_case(a, plan, crop, mvs):
    """The expected field has infinities, negative zeros and no NaN, and the plan's windows hold the four marker classes."""
    classes = set()
    for s, f, top, left, hf, vf, rot, _ in np.asarray(plan).tolist():
        classes |= RA.marker_classes(a["mvl0"][s, f + 3], a["mvl1"][s, f + 3], crop, top, left, hf, vf, rot)
    return bool(np.isinf(mvs).any() and not np.isnan(mvs).any() and ((mvs == 0) & np.signbit(mvs)).any() and classes == BOTH)


def check_batch(cs, a, plan, crop):
    got = dict(zip(OUTPUTS, cs.batch(plan, crop)))
    want = RA.batch(*(a[k] for k in ORDER), plan, crop)
    assert got["mvs1"] is got["mvs0"]
    for k in OUTPUTS:
        t = got[k]
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == SHAPES[k](len(plan), crop), k
        assert np.array_equal(RA.bits(t.cpu().numpy()), RA.bits(want[k])), k
    return got, want


def test_fixture_cases_equal_the_reference_outputs():
    from cdfo_amd.train_data import ClipSet
    a, plans, crop, want = fixture_arrays()
    got, _ = check_batch(ra_set(a), a, plans, crop)                  # all 16 cases as one batch of S = 1, T = 7
    assert covers_every_case(a, plans, crop, want["mvs0"])
    for k in OUTPUTS:
        assert np.array_equal(RA.bits(got[k].cpu().numpy()), RA.bits(want[k])), k
    ld = dict(zip(OUTPUTS, ClipSet.from_arrays(*(a[k] for k in ORDER if k != "mvl1")).batch(plans, crop)))
    for k in PLANES:                                                 # the planes do not depend on the coding
        assert torch.equal(got[k].view(torch.int32), ld[k].view(torch.int32)), k
    assert not torch.equal(got["mvs0"][:, 4:], ld["mvs0"][:, 4:])   # list 1 feeds slots 4-6


@pytest.mark.parametrize("crop", [8, 12])
def test_small_crops_equal_the_statement(crop):
    S, T, H, W = 3, 9, 22, 28
    a = random_arrays(S, T, H, W, 7 + crop)
    cs = ra_set(a)
    # all eight flag combinations over the two batches' rows; first in {0, T-7}; the four corners; sequence 1 twice in a batch
    rows = [(1, 0, 0, 0), (1, T - 7, H - crop, W - crop), (0, 0, H - crop, 0), (2, T - 7, 0, W - crop), (2, 1, 3, 5)]
    for base in (0, 3):
        plan = np.array([(s, f, t, l, (base + i) & 1, ((base + i) >> 1) & 1, ((base + i) >> 2) & 1, 0) for i, (s, f, t, l) in enumerate(rows)],
                        np.int32)
        _, want = check_batch(cs, a, plan, crop)
        assert covers_every_case(a, plan, crop, want["mvs0"])        # holds on the inputs: the seeds were picked on the CPU
    assert {(base + i) & 7 for base in (0, 3) for i in range(5)} == set(range(8))


def test_crop_64_covers_several_tiles():
    S, T, H, W = 2, 7, 70, 72
    a = random_arrays(S, T, H, W, 11)
    cs = ra_set(a)
    for plan in ([(1, 0, 6, 8, 1, 0, 1, 0), (0, 0, 1, 3, 0, 1, 0, 0)], [(0, 0, 0, 0, 1, 1, 1, 0), (1, 0, 5, 7, 0, 0, 1, 0)]):
        plan = np.array(plan, np.int32)                              # 2 x 2 tiles a plane, a 256 x 256 HR plane
        _, want = check_batch(cs, a, plan, 64)
        assert covers_every_case(a, plan, 64, want["mvs0"])


def test_a_set_without_coding_is_the_ld_set_it_was():
    from cdfo_amd import kernels as K
    from cdfo_amd.train_data import ClipSet
    a = random_arrays(1, 7, 12, 16, 1)
    cs = ClipSet.from_arrays(*(a[k] for k in ORDER if k != "mvl1"))
    assert cs.coding == "LD" and cs.mvl1 is None
    plan = np.array([(0, 0, 4, 8, 1, 0, 1, 0), (0, 0, 0, 3, 0, 1, 0, 0)], np.int32)
    x, mvs0, mvs1, *_ = cs.batch(plan, 8)
    assert mvs1 is not mvs0 and not mvs1.any() and cs.batch(plan, 8)[2] is mvs1          # the cached zero tensor
    direct = K.train_batch(cs.lr, cs.pms, cs.rms, cs.ufs, cs.mvl0, cs.hr, torch.from_numpy(plan).cuda(), 8)[1]
    assert torch.equal(mvs0.view(torch.int32), direct.view(torch.int32))
    ra = ra_set(a).batch(plan, 8)
    assert ra[2] is ra[1] and not torch.equal(ra[1].view(torch.int32), mvs0.view(torch.int32))


def test_invalid_plans_raise_before_any_launch(monkeypatch):
    from cdfo_amd import kernels as K
    a = random_arrays(1, 7, 12, 16, 1)
    cs = ra_set(a)
    launches = []
    monkeypatch.setattr(K, "train_batch_ra", lambda *args: launches.append(args))
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


def test_the_wrapper_refuses_a_wrong_mvl1():
    from cdfo_amd import kernels as K
    cs = ra_set(random_arrays(1, 7, 12, 16, 1))
    plan = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    args = lambda mvl1: (cs.lr, cs.pms, cs.rms, cs.ufs, cs.mvl0, mvl1, cs.hr, plan, 8)      # noqa: E731
    assert len(K.train_batch_ra(*args(cs.mvl1))) == 6
    for bad in (cs.mvl1.to(torch.uint8), cs.mvl1.short(), cs.mvl1[:, :, :, :-1].contiguous(), cs.mvl1[..., :2].contiguous(),
                cs.mvl1.transpose(2, 3), cs.mvl1.cpu(), None):
        with pytest.raises(ValueError):
            K.train_batch_ra(*args(bad))
    with pytest.raises(ValueError):
        K.train_batch_ra(cs.lr, cs.pms, cs.rms, cs.ufs, cs.mvl0, cs.mvl1, cs.hr, plan, 6)
    with pytest.raises(ValueError):
        K.train_batch_ra(cs.lr, cs.pms, cs.rms, cs.ufs, cs.mvl0, cs.mvl1, cs.hr, plan.long(), 8)


def test_an_ra_batch_trains_the_model():
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.loss import charbonnier
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    torch.manual_seed(0)
    *six, mvl1 = synthetic_arrays(2, 7, 12, 16, coding="RA")
    cs = ClipSet.from_arrays(*six, mvl1=mvl1, coding="RA")
    x, mvs0, mvs1, pms, rms, ufs, hr = cs.batch(cs.draw(2, np.random.default_rng(0), crop=8), 8)
    assert mvs1 is mvs0 and bool(mvs1.any()) and bool(torch.isfinite(mvs1).all())
    m = CVSR_V8(SCGs=8).cuda().train()
    sr, _ = m(x, mvs0, mvs1, pms, rms, ufs)
    loss = charbonnier(sr, hr)
    loss.backward()
    assert loss.dim() == 0 and loss.is_cuda and bool(torch.isfinite(loss))
    grads = {k: p.grad for k, p in m.named_parameters()}
    none = sorted(k for k, g in grads.items() if g is None)
    assert all(k.startswith("MV_deform_align.fusion_in") for k in none), none       # never called by the reference forward either
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)


def test_fit_trains_on_an_ra_set(tmp_path):
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.train import fit
    from cdfo_amd.train_data import ClipSet, synthetic_arrays
    torch.manual_seed(1)
    *six, mvl1 = synthetic_arrays(4, 8, 16, 16, seed=1, coding="RA")
    clips = ClipSet.from_arrays(*six, mvl1=mvl1, coding="RA")
    lines = []
    averages = fit(CVSR_V8(SCGs=8).cuda(), clips, 2, str(tmp_path), batch_size=2, crop=8, val_itv=1, log=lines.append)
    assert len(averages) == 2 and np.isfinite(averages).all() and all(v > 0 for v in averages)
    for n in (1, 2):
        sd = torch.load(str(tmp_path / "ckpt" / f"epoch-{n}.pth"), map_location="cpu")
        assert len(sd) == 261 and all(bool(torch.isfinite(v).all()) for v in sd.values())
