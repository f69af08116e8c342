"""Host side of random-access training batches (cdfo_amd/train_data.py with ``coding="RA"``): the numpy statement of an RA batch
(tests/train_batch_ra_ref.py) against the REAL reference's RandomCrop -> Augment -> ToTensor outputs of opt/data_RA_bi.py
(tests/golden/train_batch_ra_ref.npz, written by tools/gen_train_batch_ra_fixture.py), what the fixture covers, and the ``coding`` /
``mvl1`` arguments of the clip set.  Every comparison is on bit patterns: the reference's negations make -0 and its output carries
them.  No GPU: the clip sets here live on the CPU and nothing launches."""
import os

import numpy as np
import pytest
import torch

import train_batch_ra_ref as RA
from test_train_batch_cpu import OUTPUTS

GOLD = os.path.join(os.path.dirname(__file__), "golden", "train_batch_ra_ref.npz")
ORDER = ("lr", "pms", "rms", "ufs", "mvl0", "mvl1", "hr")
BOTH = {(a, b) for a in (False, True) for b in (False, True)}


def fixture_arrays():
    """(arrays [1,7,...] for `ClipSet.from_arrays` / `RA.batch`, plans [16,8], crop, expected outputs).  The fixture holds the centre
    frame's two motion fields and HR frame only; the other six entries get other content, so a wrong frame index shows."""
    g = np.load(GOLD)
    rs = np.random.RandomState(6)
    a = dict(lr=g["in_lr"][None], pms=g["in_pms"][None], rms=g["in_rms"][None], ufs=g["in_ufs"][None])
    for k, lo, hi, dt in (("mvl0", -128, 128, np.int8), ("mvl1", -128, 128, np.int8), ("hr", 0, 256, np.uint8)):
        a[k] = rs.randint(lo, hi, (1, 7) + g["in_" + k].shape[1:]).astype(dt)
        a[k][0, 3] = g["in_" + k][0]
    return a, g["plans"], int(g["crop"]), {k: g["out_" + k] for k in OUTPUTS}


def test_statement_equals_the_reference_outputs_bit_for_bit():
    a, plans, crop, want = fixture_arrays()
    assert len(plans) == 16 and {tuple(p[4:7]) for p in plans.tolist()} == {(h, v, r) for h in (0, 1) for v in (0, 1) for r in (0, 1)}
    got = RA.batch(*(a[k] for k in ORDER), plans, crop)
    for k in OUTPUTS:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, k
        assert np.array_equal(RA.bits(got[k]), RA.bits(want[k])), k
    assert np.array_equal(RA.bits(want["mvs1"]), RA.bits(want["mvs0"]))          # mvl1s_7 = mvl0s_7 in the RA loader
    assert np.array_equal(RA.bits(got["mvs1"]), RA.bits(got["mvs0"]))


def test_fixture_holds_every_case_the_arithmetic_has():
    a, plans, crop, want = fixture_arrays()
    mvs = want["mvs0"]
    assert np.isinf(mvs).any() and not np.isnan(mvs).any()
    assert ((mvs == 0) & np.signbit(mvs)).any() and ((mvs == 0) & ~np.signbit(mvs))[:, [0, 1, 2, 4, 5, 6]].any()
    assert not RA.bits(mvs[:, 3]).any()                                           # slot 3 is +0 everywhere
    for s, f, top, left, hf, vf, rot, _ in plans.tolist():                        # every window: neither, list 0, list 1, both
        assert RA.marker_classes(a["mvl0"][s, f + 3], a["mvl1"][s, f + 3], crop, top, left, hf, vf, rot) == BOTH
    # the statement is not the LD one: slots 4-6 are list 1's wherever neither list is marked
    import train_batch_ref as R
    ld = R.batch(*(a[k] for k in ORDER if k != "mvl1"), plans, crop)["mvs0"]
    assert not np.array_equal(RA.bits(ld[:, 4:]), RA.bits(mvs[:, 4:]))


def _args(S=1, T=7, H=8, W=8, seed=3):
    rs = np.random.RandomState(seed)
    u8 = lambda *s: rs.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    mv = lambda: rs.randint(-400, 400, (S, T, H, W, 3)).astype(np.int16)      # noqa: E731
    return [u8(S, T, H, W), u8(S, T, H, W), rs.randint(-400, 400, (S, T, H, W)).astype(np.int16), u8(S, T, H + 2, W), mv(),
            u8(S, T, 4 * H, 4 * W)], mv()


def test_an_ra_set_stores_mvl1_clipped_like_the_loader():
    from cdfo_amd.train_data import ClipSet
    six, mvl1 = _args()
    cs = ClipSet.from_arrays(*six, device="cpu", mvl1=mvl1, coding="RA")
    assert cs.coding == "RA" and cs.mvl1.dtype == torch.int8 and cs.mvl1.shape == cs.mvl0.shape
    assert np.array_equal(cs.mvl1.numpy(), np.clip(mvl1, -128, 127).astype(np.int8)) and (np.abs(mvl1) > 128).any()
    ld = ClipSet.from_arrays(*six, device="cpu")
    assert ld.coding == "LD" and ld.mvl1 is None
    assert ClipSet.from_arrays(*six, "cpu", coding="LD").coding == "LD"           # device stays the seventh positional argument


class _NoUpload:
    """A device argument that fails the test if anything is uploaded to it."""

    def __getattr__(self, name):
        raise AssertionError("an argument error must be raised before any upload")


@pytest.mark.parametrize("device", ["cpu", "none"])
def test_coding_and_mvl1_argument_errors(device):
    from cdfo_amd.train_data import ClipSet
    six, mvl1 = _args()
    dev = "cpu" if device == "cpu" else _NoUpload()
    with pytest.raises(ValueError, match="mvl1"):
        ClipSet.from_arrays(*six, device=dev, coding="RA")                        # RA without the second list
    with pytest.raises(ValueError, match="mvl1"):
        ClipSet.from_arrays(*six, device=dev, mvl1=mvl1)                          # LD with it
    with pytest.raises(ValueError, match="mvl1"):
        ClipSet.from_arrays(*six, device=dev, mvl1=mvl1, coding="LD")
    for coding in ("ra", "AI", "", None):
        with pytest.raises(ValueError, match="coding"):
            ClipSet.from_arrays(*six, device=dev, mvl1=mvl1, coding=coding)
    with pytest.raises(ValueError, match="mvl1"):
        ClipSet.from_arrays(*six, device=dev, mvl1=mvl1[:, :, :, :-1], coding="RA")      # shaped like mvl0, or refused
    with pytest.raises(ValueError, match="coding"):
        ClipSet.from_directories([], device=dev, coding="P")


def test_synthetic_ra_arrays_mark_blocks_in_either_list_and_stay_finite():
    from cdfo_amd.train_data import synthetic_arrays
    ld = synthetic_arrays(2, 7, 12, 16, seed=2)
    assert len(ld) == 6 and len(synthetic_arrays(2, 7, 12, 16, seed=2, coding="LD")) == 6
    ra = synthetic_arrays(2, 7, 12, 16, seed=2, coding="RA")
    assert len(ra) == 7
    for i in (0, 1, 2, 3, 5):                                                     # everything but list 0's markers is the LD call's
        assert np.array_equal(ra[i], ld[i]), i
    mv0, mv1 = ra[4], ra[6]
    assert mv1.shape == mv0.shape == (2, 7, 12, 16, 3)
    assert np.array_equal(mv0[..., :2], ld[4][..., :2]) and np.array_equal(mv0[..., 2][mv0[..., 2] != -99], ld[4][..., 2][mv0[..., 2] != -99])
    no0, no1 = mv0[..., 2] == -99, mv1[..., 2] == -99
    assert set(zip(no0.ravel().tolist(), no1.ravel().tolist())) == BOTH
    assert not (mv0[..., 2] == 0).any() and not (mv1[..., 2] == 0).any()          # no division by zero: the flows stay finite
    for mv in (mv0, mv1):                                                         # block-constant, 8 x 8
        assert np.array_equal(mv[:, :, :8, :8], np.broadcast_to(mv[:, :, :1, :1], mv[:, :, :8, :8].shape))
    out = RA.flows(mv0[0, 3], mv1[0, 3], 8, 2, 4, 0, 0, 0)
    assert np.isfinite(out).all() and out.any()
    with pytest.raises(ValueError, match="coding"):
        synthetic_arrays(1, 7, 8, 8, coding="B")


def test_from_directories_keeps_list_1_in_an_ra_set(tmp_path):
    from cdfo_amd.evaluate import write_synthetic_sequence
    from cdfo_amd.priors import write_gray_png
    from cdfo_amd.train_data import ClipSet
    T, H, W = 7, 8, 12
    rs = np.random.RandomState(8)
    lr_dir, side, hr_dir = write_synthetic_sequence(str(tmp_path), T, H, W, seed=1)
    write_gray_png(os.path.join(side, "part_m", "00000_M_mask.png"), rs.randint(0, 256, (H, W)).astype(np.uint8))
    for t in range(T):
        write_gray_png(os.path.join(side, "unfiltered", "%05d_unflt.png" % t), rs.randint(0, 256, (H + 2, W)).astype(np.uint8))
    np.save(os.path.join(side, "res", "00000_res.npy"), rs.randint(-300, 300, (H, W, 3)).astype(np.int16))
    for name in ("mvl0", "mvl1"):
        np.save(os.path.join(side, name, "00000_" + name + ".npy"), rs.randint(-300, 300, (H, W, 3)).astype(np.int16))
    cs = ClipSet.from_directories([(lr_dir, side, hr_dir)], device="cpu", coding="RA")
    assert cs.coding == "RA" and cs.mvl1.shape == (1, T, H, W, 3)
    for t in (0, 3):
        assert np.array_equal(cs.mvl1[0, t].numpy(), np.clip(np.load(os.path.join(side, "mvl1", "%05d_mvl1.npy" % t)), -128, 127))
    assert not np.array_equal(cs.mvl1.numpy(), cs.mvl0.numpy())
    assert ClipSet.from_directories([(lr_dir, side, hr_dir)], device="cpu").mvl1 is None
