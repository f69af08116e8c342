"""The random-access flow builders on the GPU (csrc/seq_flows_ra.hip: cdfo_seq_flows_ra, cdfo_seq_flows_ra_ring) against the host
statement they restate, ``streaming.mv2mvs_ra`` + ``modify_mv_for_end_frames`` on the CPU (tests/test_seq_flows_ra_cpu.py pins that
statement to the real loader's recorded field), against each other, and against cdfo_train_batch_ra on un-flipped plans.  Every
comparison is exact and on bit patterns: the rule's negations make -0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = ((5, 7), (9, 20), (12, 16), (16, 24))          # 5 x 7: W no multiple of 4, padded to 8 x 8; 9 x 20: padding rows and columns
LENGTHS = (1, 2, 3, 4, 5, 6, 7, 11)
REFS = (-99, -99, 0, 1, 2, 3, -1, -2, 4, 8)            # the marker twice as likely as a value; zero; distances of both signs
DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)


def bits(t):
    return t.contiguous().view(torch.int32)


def fields(T, H, W, dtype, seed):
    """Both lists [T,H,W,3] with values exact in `dtype`: vectors in -64 .. 63 over a lattice of zero vectors, reference components
    from REFS (zero included: x / 0 and 0 / 0), the four marker classes at the head of every entry's first row; fp32 and fp64 get
    inexact quotients as well.  uint8 wraps: -99 reads 157 and marks nothing."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for cls in ((-99, -99, 1, 2), (-99, 1, -99, -1)):
        mv = torch.randint(-64, 64, (T, H, W, 3), generator=g)
        mv[..., 2] = torch.tensor(REFS)[torch.randint(0, len(REFS), (T, H, W), generator=g)]
        mv[:, ::3, ::2, :2] = 0
        mv[:, 0, :4, 2] = torch.tensor(cls)
        plain = (mv[..., 2:3] != 0) & (mv[..., 2:3] != -99)
        mv = mv.to(dtype)
        if dtype in (torch.float32, torch.float64):
            mv[..., :2] += (torch.rand((T, H, W, 2), generator=g, dtype=torch.float64) * plain).to(dtype) * 0.37
        out.append(mv)
    return out


def host_flows(mv0, mv1, i, T, Hp, Wp):
    """What `StreamingSR(coding="RA")` builds for centre i, on the CPU (IEEE arithmetic): [7,2,Hp,Wp]."""
    from cdfo_amd.streaming import modify_mv_for_end_frames, mv2mvs_ra
    H, W = mv0.shape[1:3]
    e = max(1, i) if T > 1 else 0
    m = torch.zeros((7, 2, Hp, Wp), dtype=torch.float32)
    m[:, :, :H, :W] = mv2mvs_ra(mv0[e], mv1[e])
    return modify_mv_for_end_frames(i, m.unsqueeze(0), T)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_seq_flows_ra_equals_the_host_statement(dtype):
    """Every size, every length (all six end rules and their overlaps), the centres split as K = T, 4 and 1."""
    from cdfo_amd import kernels as K
    from cdfo_amd.streaming import padded
    seen_inf = seen_neg0 = False
    for H, W in SIZES:
        Hp, Wp = padded(H, W)
        for T in LENGTHS:
            mv0, mv1 = fields(T, H, W, dtype, 1000 * H + 10 * T)
            want = torch.stack([host_flows(mv0, mv1, i, T, Hp, Wp) for i in range(T)])
            assert not torch.isnan(want).any()
            seen_inf |= bool(torch.isinf(want).any())
            seen_neg0 |= bool(((want == 0) & torch.signbit(want)).any())
            d0, d1 = mv0.cuda(), mv1.cuda()
            whole = K.seq_flows_ra(d0, d1, 0, T, Hp, Wp)
            assert whole.shape == (T, 7, 2, Hp, Wp) and whole.dtype == torch.float32
            fours = torch.cat([K.seq_flows_ra(d0, d1, c, min(4, T - c), Hp, Wp) for c in range(0, T, 4)])
            ones = torch.cat([K.seq_flows_ra(d0, d1, i, 1, Hp, Wp) for i in range(T)])
            for name, got in (("K = T", whole), ("K = 4", fours), ("K = 1", ones)):
                got = got.cpu()
                same = (bits(got) == bits(want)).flatten(1).all(1)
                assert bool(same.all()), f"{name}, {H}x{W}, T = {T}: centres {(~same).nonzero().flatten().tolist()} differ"
    assert seen_inf and seen_neg0                              # the inputs do what they are meant to


@pytest.mark.parametrize("dtype", [torch.float32, torch.int8], ids=["float32", "int8"])
def test_more_than_one_block_of_threads(dtype):
    """The sizes above fit one block of 256 threads; 37 x 50 padded to 40 x 56 takes three, the last one partly idle, and the fp32
    field's last pixels fall back from the 16-byte loads to the guarded ones in the middle of a block."""
    from cdfo_amd import kernels as K
    T, H, W, Hp, Wp = 4, 37, 50, 40, 56
    mv0, mv1 = fields(T, H, W, dtype, 41)
    want = torch.stack([host_flows(mv0, mv1, i, T, Hp, Wp) for i in range(T)])
    got = K.seq_flows_ra(mv0.cuda(), mv1.cuda(), 0, T, Hp, Wp).cpu()
    assert torch.equal(bits(got), bits(want))
    if dtype == torch.float32:
        ring = K.seq_flows_ra_ring(mv0.cuda(), mv1.cuda(), 0, T, T, Hp, Wp).cpu()         # cap = T: the field is its own ring
        assert torch.equal(bits(ring), bits(want))


def test_an_unsigned_field_marks_nothing_and_a_signed_one_does():
    from cdfo_amd import kernels as K
    m0, m1 = fields(4, 8, 8, torch.int8, 3)
    assert (m0[..., 2] == -99).any() and (m1[..., 2] == -99).any()
    signed = K.seq_flows_ra(m0.cuda(), m1.cuda(), 0, 4, 8, 8)
    wide = K.seq_flows_ra(m0.view(torch.uint8).to(torch.int16).cuda(), m1.view(torch.uint8).to(torch.int16).cuda(), 0, 4, 8, 8)
    unsigned = K.seq_flows_ra(m0.view(torch.uint8).cuda(), m1.view(torch.uint8).cuda(), 0, 4, 8, 8)
    assert torch.equal(bits(unsigned), bits(wide)) and not torch.equal(bits(unsigned), bits(signed))


def test_seq_flows_ra_ring_equals_seq_flows_ra_on_the_completed_field():
    """cap = 10 (chunk 4) and T = 23: every slot is rewritten twice.  The rings as LiveSR has them when each chunk runs (frame t in
    slot t mod cap, older frames overwritten, the rest garbage).  Every chunk with T_known = T; every chunk released by a push, and
    every centre <= T - 4 on its own, also with T_known = 0 (the end not known yet)."""
    from cdfo_amd import kernels as K
    from cdfo_amd.live import LivePlanner
    T, cap, H, W, Hp, Wp = 23, 10, 9, 20, 16, 24
    mv0, mv1 = fields(T, H, W, torch.float32, 77)
    want = bits(K.seq_flows_ra(mv0.cuda(), mv1.cuda(), 0, T, Hp, Wp))
    assert torch.equal(want.cpu(), bits(torch.stack([host_flows(mv0, mv1, i, T, Hp, Wp) for i in range(T)])))
    ring0, ring1 = torch.full((cap, H, W, 3), 7.25), torch.full((cap, H, W, 3), -99.0)
    planner, seen, open_checked = LivePlanner(cap - 6), [], 0

    def check(plan, closed):
        nonlocal open_checked
        r0, r1 = ring0.cuda(), ring1.cuda()
        c0, k = plan.centres[0], len(plan.centres)
        assert torch.equal(bits(K.seq_flows_ra_ring(r0, r1, c0, k, T, Hp, Wp)), want[c0:c0 + k]), (plan.centres, T)
        if not closed:
            assert torch.equal(bits(K.seq_flows_ra_ring(r0, r1, c0, k, 0, Hp, Wp)), want[c0:c0 + k]), (plan.centres, 0)
        for i in plan.centres:
            if i <= T - 4:
                assert torch.equal(bits(K.seq_flows_ra_ring(r0, r1, i, 1, 0, Hp, Wp)), want[i:i + 1]), (i, "end not known")
                open_checked += 1
        seen.extend(plan.centres)

    for t in range(T):
        ring0[t % cap], ring1[t % cap] = mv0[t], mv1[t]
        plan = planner.push()
        if plan is not None:
            check(plan, False)
    for plan in planner.close():
        check(plan, True)
    assert seen == list(range(T)) and open_checked == T - 3


def test_a_one_frame_stream_reads_entry_zero_of_both_rings():
    from cdfo_amd import kernels as K
    mv0, mv1 = fields(1, 5, 7, torch.float32, 5)
    ring0, ring1 = torch.full((7, 5, 7, 3), 3.5), torch.full((7, 5, 7, 3), 3.5)
    ring0[0], ring1[0] = mv0[0], mv1[0]
    got = K.seq_flows_ra_ring(ring0.cuda(), ring1.cuda(), 0, 1, 1, 8, 8)
    assert torch.equal(bits(got), bits(K.seq_flows_ra(mv0.cuda(), mv1.cuda(), 0, 1, 8, 8))) and not got.any()   # both end rules: zeros


def test_an_unflipped_ra_training_batch_holds_the_same_field():
    """cdfo_train_batch_ra and cdfo_seq_flows_ra state one rule: the windows of an RA `ClipSet.batch` with no flips are the same
    windows of the sequence field of the plan's centre frame f + 3 (3 <= f + 3 <= T - 4: no end rule applies)."""
    from cdfo_amd import kernels as K
    from test_gpu_train_batch_ra import ra_set, random_arrays
    S, T, H, W, crop = 2, 10, 22, 28, 8
    a = random_arrays(S, T, H, W, 15)
    cs = ra_set(a)
    plan = np.array([(0, 0, 0, 0, 0, 0, 0, 0), (1, 3, H - crop, W - crop, 0, 0, 0, 0), (1, 1, 3, 5, 0, 0, 0, 0), (0, 2, 14, 0, 0, 0, 0, 0)],
                    np.int32)
    mvs = cs.batch(plan, crop)[1]
    assert torch.isinf(mvs).any() and ((mvs == 0) & torch.signbit(mvs)).any()
    for b, (s, f, top, left, *_) in enumerate(plan.tolist()):
        m0, m1 = (torch.from_numpy(a[k][s]).cuda() for k in ("mvl0", "mvl1"))
        field = K.seq_flows_ra(m0, m1, f + 3, 1, 24, 28)[0]
        assert torch.equal(bits(field[:, :, top:top + crop, left:left + crop]), bits(mvs[b])), b


def test_repeated_calls_give_equal_bits():
    from cdfo_amd import kernels as K
    mv0, mv1 = (m.cuda() for m in fields(11, 16, 24, torch.float32, 9))
    first = bits(K.seq_flows_ra(mv0, mv1, 0, 11, 16, 24)).clone()
    ring = bits(K.seq_flows_ra_ring(mv0, mv1, 3, 4, 0, 16, 24)).clone()          # cap = T: the field is its own ring
    for _ in range(3):
        assert torch.equal(bits(K.seq_flows_ra(mv0, mv1, 0, 11, 16, 24)), first)
        assert torch.equal(bits(K.seq_flows_ra_ring(mv0, mv1, 3, 4, 0, 16, 24)), ring)
    assert torch.equal(ring, first[3:7])


def test_bad_arguments_are_refused():
    from cdfo_amd import kernels as K
    from cdfo_amd._lib import CdfoError
    mv = torch.zeros((3, 8, 8, 3), device="cuda")
    for i0, k, Hp, Wp in ((2, 2, 8, 8), (0, 0, 8, 8), (-1, 1, 8, 8), (0, 1, 4, 8), (0, 1, 8, 10)):
        with pytest.raises(CdfoError):
            K.seq_flows_ra(mv, mv, i0, k, Hp, Wp)
    for i0, k, tk, Hp, Wp in ((2, 2, 3, 8, 8), (0, 0, 0, 8, 8), (-1, 1, 0, 8, 8), (0, 1, 0, 4, 8), (0, 1, 0, 8, 10), (0, 1, -1, 8, 8)):
        with pytest.raises(CdfoError):
            K.seq_flows_ra_ring(mv, mv, i0, k, tk, Hp, Wp)
    with pytest.raises(ValueError):
        K.seq_flows_ra(mv, mv.double(), 0, 1, 8, 8)
    with pytest.raises(ValueError):
        K.seq_flows_ra(mv, mv[:2], 0, 1, 8, 8)
    with pytest.raises(ValueError):
        K.seq_flows_ra_ring(mv.double(), mv.double(), 0, 1, 0, 8, 8)
    with pytest.raises(ValueError):
        K.seq_flows_ra(mv[..., :2], mv[..., :2], 0, 1, 8, 8)
