"""Live sequence inference without a GPU: `LivePlanner` against `plan_chunks` (the plans, when each is emitted, what a ring of
chunk + 6 slots has to hold), and the argument checks of the two C entry points of csrc/live.hip, which refuse before any launch."""
import ctypes as C

import pytest

CHUNKS = (1, 2, 3, 4, 8, 16)
LENGTHS = range(1, 41)


def _emitted(T, chunk):
    """[(the push that released it, or None for close(), plan)] for a stream of T frames."""
    from cdfo_amd.live import LivePlanner
    p, got = LivePlanner(chunk), []
    for t in range(T):
        plan = p.push()
        if plan is not None:
            got.append((t, plan))
    tail = p.close()
    assert len(tail) <= 3
    return got + [(None, plan) for plan in tail]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_live_plans_are_plan_chunks_plans(chunk):
    """T = 1 .. 40: what push() and close() return, concatenated, is list(plan_chunks(T, chunk)) entry for entry; the chunk that
    starts at c0 is released by the push of frame c0 + chunk + 2 or by close(), which returns at most three plans."""
    from cdfo_amd.streaming import plan_chunks
    for T in LENGTHS:
        got = _emitted(T, chunk)
        assert [plan for _, plan in got] == list(plan_chunks(T, chunk)), (T, chunk)
        for t, plan in got:
            c0 = plan.centres[0]
            if t is None:
                assert c0 + chunk + 2 >= T, (T, chunk, c0)          # its last frame never arrived: only close() can release it
            else:
                assert t == c0 + chunk + 2 and len(plan.centres) == chunk, (T, chunk, c0)
        # the centre-0 rules: priors of frame 0 come from entry max(1, 0); entry 0 is used only when T == 1
        first = got[0][1]
        assert first.priors[0][0] == first.mv_entry[0] == first.extract_priors[0] == (0 if T == 1 else 1)
        entries = {e for _, plan in got for w in plan.priors for e in w} | {e for _, plan in got for e in plan.mv_entry + plan.extract_priors}
        assert (0 in entries) == (T == 1)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_ring_of_chunk_plus_six_holds_what_every_plan_names(chunk):
    """For every emitted plan the distinct frames (and prior entries) its windows and its extract list name occupy distinct slots
    of a ring of chunk + 6, all of them have been pushed when it is emitted, and the frame pushed next after a chunk overwrites no
    frame that any later plan names."""
    from cdfo_amd.streaming import bank_slot
    cap = chunk + 6
    named = lambda plan: ({t for w in plan.windows for t in w} | set(plan.extract) | {e for w in plan.priors for e in w}
                          | set(plan.mv_entry) | set(plan.extract_priors) | set(plan.compensate_priors))
    for T in LENGTHS:
        got = _emitted(T, chunk)
        for n, (t, plan) in enumerate(got):
            frames = named(plan)
            assert len({bank_slot(f, cap) for f in frames}) == len(frames), (T, chunk, plan.centres)
            pushed = T if t is None else t + 1
            assert max(frames) < pushed and max(frames) - min(frames) < cap
            if t is not None and t + 1 < T:
                # frame t + 1 takes the slot of frame t + 1 - cap (if there is one): nobody may name that frame any more
                gone = t + 1 - cap
                for _, later in got[n + 1:]:
                    assert gone not in named(later), (T, chunk, t, later.centres)
            # and what this plan names has not been overwritten by the pushes before it
            assert min(frames) > pushed - 1 - cap


def test_close_without_a_push_is_empty_and_the_planner_closes():
    from cdfo_amd.live import LivePlanner
    p = LivePlanner(4)
    assert p.close() == []
    with pytest.raises(RuntimeError):
        p.push()
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            LivePlanner(bad)


def test_plan_chunks_resumes_where_the_planner_left_it():
    from cdfo_amd.streaming import plan_chunks
    whole = list(plan_chunks(23, 4))
    assert list(plan_chunks(23, 4, first=8, extracted=whole[1].extract[-1] + 1)) == whole[2:]
    for first, extracted in ((2, 0), (-4, 0), (4, -1)):
        with pytest.raises(ValueError):
            list(plan_chunks(23, 4, first=first, extracted=extracted))


EINVAL, EALIGN = -1, -2


def test_live_entry_points_refuse_bad_arguments_without_a_device():
    """Null pointers, cap <= 0, Hp < H, Wp % 4, K <= 0, a negative i0, a misaligned output: CDFO_EINVAL / CDFO_EALIGN before any HIP
    call.  (Every call here is refused: none of the pointers is real.)"""
    from cdfo_amd import _lib
    lib = _lib.lib()
    P = lambda v: C.c_void_p(v)
    good = dict(lr=P(64), ufs=P(128), pms=P(192), rms=P(256), sample_bytes=1, cap=7, H=21, W=27, table=P(320), K=1, E=1, Hp=24, Wp=32,
                peak=255, x=P(1024), r=P(2048), u=P(4096), lr_new=P(8192), p_new=P(16384), r_new=P(32768))

    def planes(**change):
        a = dict(good, **change)
        return lib.cdfo_live_planes(*a.values(), None)

    for name in ("lr", "ufs", "pms", "rms", "table", "x", "u", "lr_new", "p_new"):
        assert planes(**{name: None}) == EINVAL, name
    for change in (dict(cap=0), dict(cap=-3), dict(H=0), dict(W=-1), dict(Hp=20), dict(Wp=24), dict(Wp=30), dict(K=0), dict(K=-1),
                   dict(E=-1), dict(K=3200), dict(sample_bytes=3), dict(sample_bytes=1, peak=1023), dict(peak=0), dict(peak=65536),
                   dict(H=1 << 15, W=1 << 15, Hp=1 << 15, Wp=1 << 15)):
        assert planes(**change) == EINVAL, change
    for change in (dict(x=P(1032)), dict(r=P(2052)), dict(u=P(4100)), dict(lr_new=P(8200)), dict(p_new=P(16388)), dict(r_new=P(32770)),
                   dict(rms=P(258)), dict(table=P(322)), dict(sample_bytes=2, peak=1023, lr=P(65)), dict(sample_bytes=2, peak=1023, ufs=P(129))):
        assert planes(**change) == EALIGN, change

    ring = dict(ring=P(64), cap=7, H=21, W=27, i0=0, K=1, T_known=0, Hp=24, Wp=32, out=P(1024))

    def flows(**change):
        a = dict(ring, **change)
        return lib.cdfo_seq_flows_ring(*a.values(), None)

    for change in (dict(ring=None), dict(out=None), dict(cap=0), dict(cap=-1), dict(H=0), dict(Hp=16), dict(Wp=24), dict(Wp=34),
                   dict(K=0), dict(K=-2), dict(i0=-1), dict(T_known=-1), dict(T_known=3, i0=2, K=2), dict(K=70000),
                   dict(i0=0x7ffffff0, K=64)):
        assert flows(**change) == EINVAL, change
    for change in (dict(out=P(1028)), dict(ring=P(66))):
        assert flows(**change) == EALIGN, change
