"""Host side of device training batches (cdfo_amd/train_data.py): the numpy statement of a batch (tests/train_batch_ref.py) against
the REAL reference's RandomCrop -> Augment -> ToTensor outputs (tests/golden/train_batch_ref.npz, written by
tools/gen_train_batch_fixture.py), the plan draws, the epoch cover, the loader's clipping and plan validation.  No GPU: the clip
sets here live on the CPU and nothing launches."""
import os

import numpy as np
import pytest
import torch

import train_batch_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "train_batch_ref.npz")
OUTPUTS = ("x", "mvs0", "mvs1", "pms", "rms", "ufs", "hr")


def fixture_arrays():
    """(arrays [1,7,...] for `ClipSet.from_arrays` / `R.batch`, plans [16,8], crop, expected outputs).  The fixture holds the centre
    frame's motion field and HR frame only; the other six entries get other content, so a wrong frame index shows."""
    g = np.load(GOLD)
    rs = np.random.RandomState(5)
    mvl0 = rs.randint(-128, 128, (1, 7) + g["in_mvl0"].shape[1:]).astype(np.int8)
    hr = rs.randint(0, 256, (1, 7) + g["in_hr"].shape[1:]).astype(np.uint8)
    mvl0[0, 3], hr[0, 3] = g["in_mvl0"][0], g["in_hr"][0]
    arrays = dict(lr=g["in_lr"][None], pms=g["in_pms"][None], rms=g["in_rms"][None], ufs=g["in_ufs"][None], mvl0=mvl0, hr=hr)
    return arrays, g["plans"], int(g["crop"]), {k: g["out_" + k] for k in OUTPUTS}


def cpu_set(S=3, T=32, H=20, W=24):
    from cdfo_amd.train_data import ClipSet
    z = lambda *s, d=np.uint8: np.zeros(s, d)      # noqa: E731
    return ClipSet.from_arrays(z(S, T, H, W), z(S, T, H, W), z(S, T, H, W, d=np.int8), z(S, T, H + 2, W), z(S, T, H, W, 3, d=np.int8),
                               z(S, T, 4 * H, 4 * W), device="cpu")


def test_statement_equals_the_reference_outputs_exactly():
    a, plans, crop, want = fixture_arrays()
    assert len(plans) == 16 and {tuple(p[4:7]) for p in plans.tolist()} == {(h, v, r) for h in (0, 1) for v in (0, 1) for r in (0, 1)}
    got = R.batch(a["lr"], a["pms"], a["rms"], a["ufs"], a["mvl0"], a["hr"], plans, crop)
    assert np.isinf(want["mvs0"]).any() and not np.isnan(want["mvs0"]).any()
    for k in OUTPUTS:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k             # infinities compare equal to themselves, sign included


def test_draws_follow_the_reference_ranges():
    cs = cpu_set()
    plan = cs.draw(10000, np.random.default_rng(1), crop=8)
    assert plan.dtype == np.int32 and plan.shape == (10000, 8)
    for col, last in ((0, cs.S - 1), (1, cs.T - 7), (2, cs.H - 8 - 1), (3, cs.W - 8 - 1)):        # both ends hit, H - crop never
        assert plan[:, col].min() == 0 and plan[:, col].max() == last, col
    for col in (4, 5, 6):
        assert set(np.unique(plan[:, col])) == {0, 1} and 0.45 <= plan[:, col].mean() <= 0.55, col
    assert not plan[:, 7].any()
    cs.check_plan(plan, 8)
    with pytest.raises(ValueError):
        cs.draw(4, np.random.default_rng(1), crop=cs.H)


@pytest.mark.parametrize("S,batch", [(7, 3), (4, 2), (5, 8)])
def test_epoch_covers_each_sequence_once(S, batch):
    cs = cpu_set(S=S, T=8)
    plans = list(cs.epoch(batch, np.random.default_rng(2), crop=8))
    assert [len(p) for p in plans] == [batch] * (S // batch) + ([S % batch] if S % batch else [])     # drop_last=False
    assert sorted(np.concatenate(plans)[:, 0].tolist()) == list(range(S))


def test_from_arrays_clips_like_the_loader():
    from cdfo_amd.train_data import ClipSet
    S, T, H, W = 1, 7, 8, 8
    rs = np.random.RandomState(3)
    rms, mv = rs.randint(-400, 400, (S, T, H, W)).astype(np.int16), rs.randint(-400, 400, (S, T, H, W, 3)).astype(np.int16)
    u8 = lambda *s: rs.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    cs = ClipSet.from_arrays(u8(S, T, H, W), u8(S, T, H, W), rms, u8(S, T, H + 2, W), mv, u8(S, T, 4 * H, 4 * W), device="cpu")
    assert cs.rms.dtype == torch.int8 and cs.mvl0.dtype == torch.int8 and cs.ufs.shape == (S, T, H + 2, W)
    assert np.array_equal(cs.rms.numpy(), np.clip(rms, -128, 127).astype(np.int8)) and (np.abs(rms) > 128).any()
    assert np.array_equal(cs.mvl0.numpy(), np.clip(mv, -128, 127).astype(np.int8))
    with pytest.raises(ValueError):
        ClipSet.from_arrays(u8(S, T, H, W), u8(S, T, H, W + 1), rms, u8(S, T, H + 2, W), mv, u8(S, T, 4 * H, 4 * W), device="cpu")
    with pytest.raises(ValueError):
        ClipSet.from_arrays(u8(S, T, H, W), u8(S, T, H, W), rms, u8(S, T, H - 1, W), mv, u8(S, T, 4 * H, 4 * W), device="cpu")
    with pytest.raises(ValueError):
        ClipSet.from_arrays(u8(S, 6, H, W), u8(S, 6, H, W), rms[:, :6], u8(S, 6, H, W), mv[:, :6], u8(S, 6, 4 * H, 4 * W), device="cpu")


BAD_PLANS = {"sequence": (3, 0, 0, 0, 0, 0, 0, 0), "negative": (0, -1, 0, 0, 0, 0, 0, 0), "first": (0, 26, 0, 0, 0, 0, 0, 0),
             "top": (0, 0, 13, 0, 0, 0, 0, 0), "left": (0, 0, 0, 17, 0, 0, 0, 0), "flag": (0, 0, 0, 0, 2, 0, 0, 0),
             "rot": (0, 0, 0, 0, 0, 0, -1, 0)}


@pytest.mark.parametrize("name", sorted(BAD_PLANS))
def test_bad_plans_raise(name):
    cs = cpu_set()                                   # 3 x 32 frames of 20 x 24
    good = np.array([[2, 25, 12, 16, 1, 1, 1, 0]], np.int32)                # the far corner is allowed in an explicit plan
    assert np.array_equal(cs.check_plan(good, 8), good)
    with pytest.raises(ValueError):
        cs.check_plan(np.array([good[0], BAD_PLANS[name]], np.int32), 8)
    with pytest.raises(ValueError):
        cs.batch(np.array([BAD_PLANS[name]], np.int32), 8)                  # raises before anything touches a device


def test_bad_crops_and_shapes_raise():
    cs = cpu_set()
    good = np.array([[0, 0, 0, 0, 0, 0, 0, 0]], np.int32)
    for crop in (6, 0, -4):
        with pytest.raises(ValueError):
            cs.batch(good, crop)
    for plan in (good[0], good[:, :7], good[:0], good.astype(np.float32)):
        with pytest.raises(ValueError):
            cs.check_plan(plan, 8)


def test_priors_of_frame_0_are_its_own_files_on_request(tmp_path):
    from cdfo_amd.evaluate import write_synthetic_sequence
    from cdfo_amd.priors import load_sequence
    lr_dir, side, _ = write_synthetic_sequence(str(tmp_path), 3, 8, 8, gt=False)
    assert load_sequence(lr_dir, side)["pms"].shape == (3, 8, 8)             # the evaluation loop: frame 1's priors stand in
    with pytest.raises(FileNotFoundError, match="00000_"):
        load_sequence(lr_dir, side, own_frame0=True)


def test_from_directories_reads_every_frames_own_priors(tmp_path):
    """The training layout: 00000_* prior files exist, the unfiltered planes have two rows more than the LR frames, HR frames beside."""
    from cdfo_amd.evaluate import write_synthetic_sequence
    from cdfo_amd.priors import read_gray_png, write_gray_png
    from cdfo_amd.train_data import ClipSet
    T, H, W = 7, 8, 12
    rs = np.random.RandomState(6)
    seqs = []
    for s in range(2):
        lr_dir, side, hr_dir = write_synthetic_sequence(str(tmp_path / str(s)), T, H, W, seed=s)
        write_gray_png(os.path.join(side, "part_m", "00000_M_mask.png"), rs.randint(0, 256, (H, W)).astype(np.uint8))
        for t in range(T):
            write_gray_png(os.path.join(side, "unfiltered", "%05d_unflt.png" % t), rs.randint(0, 256, (H + 2, W)).astype(np.uint8))
        np.save(os.path.join(side, "res", "00000_res.npy"), rs.randint(-300, 300, (H, W, 3)).astype(np.int16))
        for name in ("mvl0", "mvl1"):
            np.save(os.path.join(side, name, "00000_" + name + ".npy"), rs.randint(-300, 300, (H, W, 3)).astype(np.int16))
        seqs.append((lr_dir, side, hr_dir))
    cs = ClipSet.from_directories(seqs, device="cpu")
    assert (cs.S, cs.T, cs.H, cs.W) == (2, T, H, W) and cs.ufs.shape == (2, T, H + 2, W) and cs.hr.shape == (2, T, 4 * H, 4 * W)
    side = seqs[1][1]
    assert np.array_equal(cs.pms[1, 0].numpy(), read_gray_png(os.path.join(side, "part_m", "00000_M_mask.png")))
    assert np.array_equal(cs.pms[1, 1].numpy(), read_gray_png(os.path.join(side, "part_m", "00001_M_mask.png")))
    assert np.array_equal(cs.rms[1, 0].numpy(), np.clip(np.load(os.path.join(side, "res", "00000_res.npy"))[:, :, 0], -128, 127))
    assert np.array_equal(cs.mvl0[1, 0].numpy(), np.clip(np.load(os.path.join(side, "mvl0", "00000_mvl0.npy")), -128, 127))
    assert np.array_equal(cs.hr[1, 3].numpy(), read_gray_png(os.path.join(seqs[1][2], "00003.png")))
    with pytest.raises(ValueError):                                                          # the evaluation loop takes no taller planes
        from cdfo_amd.priors import load_sequence
        load_sequence(seqs[0][0], seqs[0][1])
