"""The two kernels of csrc/live.hip on the GPU: cdfo_live_planes against its numpy statement (tests/live_ref.py) and
cdfo_seq_flows_ring against cdfo_seq_flows on the whole field.  Every comparison is exact, on bit patterns."""
import numpy as np
import pytest
import torch

import live_ref

pytestmark = pytest.mark.gpu

SHAPES = [(21, 27, 24, 32),      # rows of 27 samples: an unaligned start for every row but the first, guarded tails
          (8, 8, 8, 8),          # no padding
          (5, 3, 8, 8)]
KINDS = [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rings(rs, cap, H, W, kind, peak):
    lr, ufs = (rs.randint(0, peak + 1, (cap, H, W)).astype(kind) for _ in range(2))
    lr.flat[0], lr.flat[-1], ufs.flat[0], ufs.flat[-1] = peak, 0, 0, peak
    pms = rs.randint(0, 256, (cap, H, W)).astype(np.uint8)
    rms = (rs.randn(cap, H, W) * 6).astype(np.float32)          # what astype(float32) of any residual file may hold
    rms[:, ::2, ::2] = np.round(rms[:, ::2, ::2])
    rms[:, 0, 0] = -0.0
    rms[:, H - 1, W - 1] = -128.0
    return lr, ufs, pms, rms


def _tables(rs, cap, K, E):
    """Window slots with the repeats of the clipped windows of both ends of a sequence of `cap` frames; priors = max(1, .)."""
    centres = [0, cap - 1, 1, cap - 2][:K]
    win_frame = [[min(max(i + n - 3, 0), cap - 1) for n in range(7)] for i in centres]
    win_prior = [[max(1, t) for t in w] for w in win_frame]
    new_frame = [int(v) for v in rs.randint(0, cap, E)]
    return win_frame, win_prior, new_frame, [max(1, t) for t in new_frame]


def _launch(rings, tables, K, E, Hp, Wp, peak, **want):
    from cdfo_amd import kernels as Kn
    flat = [s for w in tables[0] for s in w] + [s for w in tables[1] for s in w] + tables[2] + tables[3]
    dev = lambda a: torch.from_numpy(a).cuda()
    lr, ufs, pms, rms = rings
    return Kn.live_planes(dev(lr), dev(ufs), dev(pms), dev(rms), torch.tensor(flat, dtype=torch.int32).cuda(), K, E, Hp, Wp, peak, **want)


def _same(got, ref, what):
    names = ("x", "r", "u", "lr_new", "p_new", "r_new")
    for name, g, w in zip(names, got, ref):
        if g is None:
            continue
        assert tuple(g.shape) == w.shape, (what, name)
        assert np.array_equal(_bits(g), _bits(w)), (what, name)


@pytest.mark.parametrize("kind,peak", KINDS)
@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_live_planes_equal_the_numpy_statement(H, W, Hp, Wp, kind, peak):
    """cap 7 and 10, K 1 and 4, E 0, 1 and K + 3, repeated slots, residuals with negative values and -0.0; r null and r_new null,
    each; a slot of -1 and of cap gives planes of zeros while the other planes are right."""
    rs = np.random.RandomState(H * 100 + W + peak)
    for cap in (7, 10):
        rings = _rings(rs, cap, H, W, kind, peak)
        for K in (1, 4):
            for E in (0, 1, K + 3):
                tables = _tables(rs, cap, K, E)
                ref = live_ref.live_planes(rings[0], rings[1], rings[2], rings[3], *tables, Hp, Wp, peak)
                what = (cap, K, E)
                got = _launch(rings, tables, K, E, Hp, Wp, peak)
                assert all(g is not None for g in got)
                _same(got, ref, what)
                assert np.signbit(ref[1][0, 3, 0, 0]) and ref[1][0, 3, 0, 0] == 0           # the -0.0 survives, padding is +0
                no_r = _launch(rings, tables, K, E, Hp, Wp, peak, want_r=False)
                assert no_r[1] is None and no_r[5] is not None
                _same(no_r, ref, what + ("r null",))
                no_rn = _launch(rings, tables, K, E, Hp, Wp, peak, want_r_new=False)
                assert no_rn[5] is None and no_rn[1] is not None
                _same(no_rn, ref, what + ("r_new null",))
                # bad slots: planes of zeros, everything else untouched
                bad = [[list(w) for w in tables[0]], [list(w) for w in tables[1]], list(tables[2]), list(tables[3])]
                bad[0][0][2], bad[1][K - 1][5] = -1, cap
                if E:
                    bad[2][0], bad[3][E - 1] = cap, -1
                ref_bad = live_ref.live_planes(rings[0], rings[1], rings[2], rings[3], *bad, Hp, Wp, peak)
                got_bad = _launch(rings, bad, K, E, Hp, Wp, peak)
                _same(got_bad, ref_bad, what + ("bad slots",))
                assert not got_bad[0][0, 2].any() and not got_bad[1][K - 1, 5].any() and not got_bad[2][K - 1, 5].any()
                if E:
                    assert not got_bad[3][0].any() and not got_bad[4][E - 1].any() and not got_bad[5][E - 1].any()


@pytest.mark.parametrize("H,W,Hp,Wp", SHAPES)
def test_live_planes_8_bit_and_16_bit_forms_of_the_same_samples_agree(H, W, Hp, Wp):
    """v / 255 and (257 v) / 65535 are the same rational: with ONE correctly rounded division each the planes are the same bits."""
    rs = np.random.RandomState(77)
    cap, K, E = 7, 4, 7
    lr, ufs, pms, rms = _rings(rs, cap, H, W, np.uint8, 255)
    tables = _tables(rs, cap, K, E)
    a = _launch((lr, ufs, pms, rms), tables, K, E, Hp, Wp, 255)
    b = _launch((lr.astype(np.uint16) * 257, ufs.astype(np.uint16) * 257, pms, rms), tables, K, E, Hp, Wp, 65535)
    for i in (0, 2, 3, 4):                       # x, u, lr_new, p_new (the residual planes are divided by another peak)
        assert np.array_equal(_bits(a[i]), _bits(b[i])), i


def test_live_planes_refuses_what_it_cannot_read():
    from cdfo_amd import kernels as Kn
    rs = np.random.RandomState(1)
    rings = _rings(rs, 7, 8, 8, np.uint8, 255)
    tables = _tables(rs, 7, 1, 1)
    with pytest.raises(ValueError):             # 16-bit rings at an 8-bit peak
        _launch((rings[0].astype(np.uint16), rings[1].astype(np.uint16), rings[2], rings[3]), tables, 1, 1, 8, 8, 255)
    with pytest.raises(ValueError):             # a table of another length
        _launch(rings, tables, 1, 2, 8, 8, 255)
    with pytest.raises(Kn.CdfoError):
        _launch(rings, tables, 1, 1, 8, 10, 255)


def _field(T, H, W):
    """The fp32 field of test_gpu_sequence.py::test_seq_flows_equals_the_host_functions: zeros in mv[..., 2], 0 / 0, an inf / NaN
    pixel, the 3e38 / -1e-39 pixel."""
    g = torch.Generator().manual_seed(100 + T)
    mv = torch.randint(-64, 64, (T, H, W, 3), generator=g)
    mv[..., 2] = torch.randint(-3, 4, (T, H, W), generator=g)
    mv[:, ::5, ::3, 0] = 0
    mv = mv.to(torch.float32)
    mv = mv + (torch.rand(mv.shape, generator=g, dtype=torch.float64) * (mv[..., 2:3] != 0)).to(torch.float32) * 0.37
    mv[0 if T == 1 else 1, 2, 3] = torch.tensor([float("inf"), float("nan"), 2.0])
    mv[T - 1, H - 1, W - 1] = torch.tensor([3e38, -1e-39, 1e-3])
    return mv


@pytest.mark.parametrize("cap", [7, 9])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 11])
def test_seq_flows_ring_equals_seq_flows_on_the_whole_field(T, cap):
    """The ring as LiveSR has it when each chunk runs (chunk = cap - 6: frame t in slot t mod cap, older frames overwritten, the
    rest garbage).  Every centre with T_known = T; every centre <= T - 4 also with T_known = 0 (the end not known yet)."""
    from cdfo_amd import kernels as Kn
    from cdfo_amd.live import LivePlanner
    H, W, Hp, Wp = 21, 27, 24, 32
    mv = _field(T, H, W)
    want = Kn.seq_flows(mv.cuda(), 0, T, Hp, Wp).cpu().view(torch.int32)
    assert torch.isinf(want.view(torch.float32)).any() or T == 1
    ring = torch.full((cap, H, W, 3), 7.25)
    planner, seen, open_checked = LivePlanner(cap - 6), [], 0

    def check(plan, closed):
        nonlocal open_checked
        dev = ring.cuda()
        c0, k = plan.centres[0], len(plan.centres)
        assert torch.equal(Kn.seq_flows_ring(dev, c0, k, T, Hp, Wp).cpu().view(torch.int32), want[c0:c0 + k]), (plan.centres, T)
        if not closed:
            assert torch.equal(Kn.seq_flows_ring(dev, c0, k, 0, Hp, Wp).cpu().view(torch.int32), want[c0:c0 + k]), (plan.centres, 0)
        for i in plan.centres:
            if i <= T - 4:
                one = Kn.seq_flows_ring(dev, i, 1, 0, Hp, Wp).cpu().view(torch.int32)
                assert torch.equal(one, want[i:i + 1]), (i, "end not known")
                open_checked += 1
        seen.extend(plan.centres)

    for t in range(T):
        ring[t % cap] = mv[t]
        plan = planner.push()
        if plan is not None:
            check(plan, False)
    for plan in planner.close():
        check(plan, True)
    assert seen == list(range(T)) and open_checked == max(0, T - 3)


def test_seq_flows_ring_refuses_bad_arguments():
    from cdfo_amd import kernels as Kn
    ring = torch.zeros((7, 8, 8, 3), device="cuda")
    for i0, k, tk, Hp, Wp in ((2, 2, 3, 8, 8), (0, 0, 0, 8, 8), (-1, 1, 0, 8, 8), (0, 1, 0, 4, 8), (0, 1, 0, 8, 10), (0, 1, -1, 8, 8)):
        with pytest.raises(Kn.CdfoError):
            Kn.seq_flows_ring(ring, i0, k, tk, Hp, Wp)
    with pytest.raises(ValueError):
        Kn.seq_flows_ring(ring.double(), 0, 1, 0, 8, 8)
