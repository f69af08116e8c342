"""Host side of sequence inference with ``coding="RA"`` (cdfo_amd/streaming.py, live.py): the torch statement `mv2mvs_ra` against the
REAL random-access loader's recorded field (tests/golden/train_batch_ra_ref.npz) and against its numpy statement
(tests/train_batch_ra_ref.py), the identity with the LD rule when both lists are one field, the end rules, and the argument errors,
each of which is raised before anything launches.  Comparisons are on bit patterns unless said otherwise: the negations make -0.
No GPU: nothing here touches a device."""
import os

import numpy as np
import pytest
import torch

import train_batch_ra_ref as RA
from cdfo_amd.streaming import StreamingSR, check_coding, mv2mvs, mv2mvs_ra, modify_mv_for_end_frames

GOLD = os.path.join(os.path.dirname(__file__), "golden", "train_batch_ra_ref.npz")
BOTH = {(a, b) for a in (False, True) for b in (False, True)}


def bits(t):
    return RA.bits(t.numpy() if isinstance(t, torch.Tensor) else t)


def marked_fields(H, W, seed):
    """Two int8 fields [H,W,3] with all four marker classes, zero references (infinities and 0 / 0), zero vectors over a negative
    reference (-0) and plain blocks."""
    rs = np.random.RandomState(seed)
    mv0, mv1 = (rs.randint(-128, 128, (H, W, 3)).astype(np.int8) for _ in range(2))
    for mv in (mv0, mv1):
        mv[..., 2] = rs.choice([-3, -2, -1, 0, 1, 2, -99], size=(H, W))
        mv[rs.rand(H, W) < 0.2, :2] = 0
    mv0[0, :4, 2], mv1[0, :4, 2] = (-99, -99, 1, 2), (-99, 1, -99, -1)       # every class, whatever the draw
    mv0[1, :2], mv1[1, :2] = ((0, 0, 0), (5, 0, 0)), ((0, 7, 0), (0, 0, 0))   # 0 / 0 and x / 0 in both lists
    mv0[2, 0], mv1[2, 0] = (0, 0, 2), (0, 0, -2)                              # -0 out of the division itself
    return mv0, mv1


def test_statement_equals_the_loaders_unflipped_windows_bit_for_bit():
    g = np.load(GOLD)
    plans, crop, want = g["plans"], int(g["crop"]), g["out_mvs0"]
    mv0, mv1 = g["in_mvl0"][0], g["in_mvl1"][0]
    got = mv2mvs_ra(torch.from_numpy(mv0), torch.from_numpy(mv1))
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 2) + mv0.shape[:2]
    for row in (0, 8):
        s, f, top, left, hf, vf, rot, _ = plans[row].tolist()
        assert (hf, vf, rot) == (0, 0, 0)
        assert np.array_equal(bits(got[:, :, top:top + crop, left:left + crop]), bits(want[row])), row
        assert RA.marker_classes(mv0, mv1, crop, top, left, 0, 0, 0) == BOTH


@pytest.mark.parametrize("H,W,seed", [(16, 16, 0), (5, 7, 1), (9, 20, 2)])
def test_statement_equals_the_numpy_statement_on_marked_fields(H, W, seed):
    mv0, mv1 = marked_fields(H, W, seed)
    n = max(H, W)                                             # the numpy statement crops squares: pad, and compare the field's part
    pad = lambda mv: np.pad(mv, ((0, n - H), (0, n - W), (0, 0)))
    want = RA.flows(pad(mv0), pad(mv1), n, 0, 0, 0, 0, 0)[:, :, :H, :W]
    got = mv2mvs_ra(torch.from_numpy(mv0), torch.from_numpy(mv1))
    assert np.array_equal(bits(got), bits(want))
    assert RA.marker_classes(pad(mv0), pad(mv1), n, 0, 0, 0, 0, 0) >= BOTH
    assert np.isinf(want).any() and not np.isnan(want).any() and ((want == 0) & np.signbit(want)).any()
    assert not bits(got[3]).any()                             # slot 3 is +0


def test_one_field_for_both_lists_gives_the_ld_rule_under_equality():
    rs = np.random.RandomState(4)
    mv = rs.randint(-128, 128, (16, 16, 3)).astype(np.int8)
    mv[..., 2] = rs.choice([-2, -1, 0, 1, 2], size=(16, 16))
    mv[mv[..., 2] == 0, :2] |= 1                              # x / 0 with x != 0: infinities, no NaN
    t = torch.from_numpy(mv)
    ld, ra = mv2mvs(t), mv2mvs_ra(t, t)
    assert torch.isinf(ld).any() and not torch.isnan(ld).any()
    assert torch.equal(ra, ld)                                # == : +0 and -0 compare equal
    # The claim is made under ==, not on bit patterns, because of 0 / 0: NaN becomes +0 BEFORE the weights, so the LD rule's negative
    # weights turn it into -0 in slots 4-6 where list 1's own quotient stays +0.  (Without a NaN the two do agree bit for bit.)
    mv[0, 0], mv[3, 5] = (0, 0, 0), (0, 9, 0)
    t = torch.from_numpy(mv)
    ld, ra = mv2mvs(t), mv2mvs_ra(t, t)
    assert torch.equal(ra, ld)
    differ = torch.from_numpy((bits(ra) != bits(ld)).astype(np.uint8))
    assert differ[4:, :, 0, 0].all() and differ[4:, 1, 3, 5].all() and int(differ.sum()) == 9


def test_an_unsigned_field_never_marks():
    mv0, mv1 = marked_fields(8, 8, 5)
    u0, u1 = (torch.from_numpy(m.view(np.uint8)) for m in (mv0, mv1))          # -99 reads 157
    assert (u0[..., 2] == 157).any()
    plain = lambda m: torch.stack([m[..., 1] / m[..., 2], m[..., 0] / m[..., 2]]).nan_to_num(nan=0.0, posinf=float("inf"))
    got = mv2mvs_ra(u0, u1)
    assert torch.equal(got[6], plain(u1.float()) * 3.0 / 128.0) and torch.equal(got[2], -plain(u0.float()) / 128.0)


@pytest.mark.parametrize("T", range(1, 8))
def test_end_rules_on_the_ra_field(T):
    """`modify_mv_for_end_frames` on the RA field, against the six rules written out per slot (the slots are all distinct here)."""
    mv0, mv1 = marked_fields(8, 8, 10 + T)
    base = mv2mvs_ra(torch.from_numpy(mv0), torch.from_numpy(mv1))
    for i in range(T):
        src = list(range(7))                                  # slot k of the result holds slot src[k] of the field, or zeros (None)
        if i == 0:
            src[0:3] = [None] * 3
        if i == 1:
            src[0] = src[1] = src[2]
        if i == 2:
            src[0] = src[1]
        if i == T - 1:
            src[4:7] = [None] * 3
        if i == T - 2:
            src[5] = src[6] = src[4]
        if i == T - 3:
            src[6] = src[5]
        got = modify_mv_for_end_frames(i, base.clone().unsqueeze(0), T)[0]
        for k in range(7):
            want = torch.zeros_like(base[0]) if src[k] is None else base[src[k]]
            assert np.array_equal(bits(got[k]), bits(want)), (T, i, k)


def test_bad_coding_is_refused_before_any_device_work():
    from cdfo_amd.evaluate import evaluate_sequence, evaluate_yuv
    from cdfo_amd.live import LiveSR
    from cdfo_amd.train import fit
    assert check_coding("LD") == "LD" and check_coding("RA") == "RA"
    model = torch.nn.Linear(1, 1)                             # on the CPU: a valid coding would get as far as NotImplementedError
    z = np.zeros((2, 8, 8), np.uint8)
    mv = np.zeros((2, 8, 8, 3), np.int8)
    for bad in ("ra", "LDP", None, 0):
        with pytest.raises(ValueError, match="coding"):
            StreamingSR(model, z, z, z, z, mv, mv, coding=bad)
        with pytest.raises(ValueError, match="coding"):
            LiveSR(model, 8, 8, coding=bad)
        with pytest.raises(ValueError, match="coding"):
            evaluate_sequence(model, "/nonexistent/lr", "/nonexistent/side", coding=bad)
        with pytest.raises(ValueError, match="coding"):
            evaluate_yuv(model, "/nonexistent/lr.yuv", 8, 8, "/nonexistent/side", coding=bad)
        with pytest.raises(ValueError, match="coding"):
            fit(model, None, 0, "/nonexistent/out", val_coding=bad)
    for good in ("LD", "RA"):
        with pytest.raises(NotImplementedError):
            StreamingSR(model, z, z, z, z, mv, mv, coding=good)


def test_lists_of_different_shape_or_dtype_are_refused_before_any_launch(monkeypatch):
    from cdfo_amd import _lib, kernels as K
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was looked up"))
    a = torch.zeros((3, 8, 8, 3), dtype=torch.int8)
    for b in (a.to(torch.int16), a[:, :, :4], a[:2], a.float()):
        with pytest.raises(ValueError, match="agree"):
            K.seq_flows_ra(a, b, 0, 1, 8, 8)
        with pytest.raises(ValueError, match="agree"):
            K.seq_flows_ra_ring(a.float(), b.double() if b.dtype == torch.float32 else b, 0, 1, 0, 8, 8)
        if b[0].shape != a[0].shape or b.dtype != a.dtype:
            with pytest.raises(ValueError, match="agree"):
                mv2mvs_ra(a[0], b[0])
    with pytest.raises(ValueError):                           # equal, but no device tensors
        K.seq_flows_ra(a, a, 0, 1, 8, 8)
    with pytest.raises(ValueError):
        K.seq_flows_ra_ring(a.float(), a.float(), 0, 1, 0, 8, 8)
    z = np.zeros((3, 8, 8), np.uint8)
    with pytest.raises(ValueError, match="agree"):            # judged before the model's device is
        StreamingSR(torch.nn.Linear(1, 1), z, z, z, z, a.numpy(), a.numpy().astype(np.int16), coding="RA")
    with pytest.raises(NotImplementedError):                  # the LD rule never reads mvl0: it may be anything, as before
        StreamingSR(torch.nn.Linear(1, 1), z, z, z, z, a.numpy()[:1], a.numpy(), coding="LD")


def test_live_push_wants_list_0_exactly_when_the_coding_reads_it():
    from cdfo_amd.live import check_push_lists
    mv = np.zeros((8, 8, 3), np.int8)
    check_push_lists("LD", None)
    check_push_lists("RA", mv)
    with pytest.raises(ValueError, match="mvl0"):
        check_push_lists("RA", None)
    with pytest.raises(ValueError, match="mvl0"):
        check_push_lists("LD", mv)


def test_synthetic_markers_change_reference_components_only(tmp_path):
    from cdfo_amd.evaluate import write_synthetic_sequence
    plain = write_synthetic_sequence(str(tmp_path / "a"), 3, 32, 48, seed=5)
    marked = write_synthetic_sequence(str(tmp_path / "b"), 3, 32, 48, seed=5, markers=True)
    classes = set()
    for root_a, root_b in zip(plain, marked):
        for d, _, names in os.walk(root_a):
            for n in names:
                pa, pb = os.path.join(d, n), os.path.join(root_b, os.path.relpath(os.path.join(d, n), root_a))
                if "mvl" not in n:
                    assert open(pa, "rb").read() == open(pb, "rb").read(), n
    for t in (1, 2):
        a0, a1, b0, b1 = (np.load(os.path.join(r[1], l, "%05d_%s.npy" % (t, l))) for r in (plain, marked) for l in ("mvl0", "mvl1"))
        for a, b in ((a0, b0), (a1, b1)):
            assert a.dtype == b.dtype and np.array_equal(a[..., :2], b[..., :2]) and not (a[..., 2] == -99).any()
            assert np.array_equal(a[..., 2][b[..., 2] != -99], b[..., 2][b[..., 2] != -99])
        classes |= set(zip((b0[..., 2] == -99).ravel().tolist(), (b1[..., 2] == -99).ravel().tolist()))
    assert classes == BOTH
