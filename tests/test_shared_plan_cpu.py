"""The schedule of chunked inference with shared compensation (run_chunked(share_compensation=True)): pure Python, no GPU.  For
every sequence length 1..20 and chunk size 1..9 every frame is compensated exactly once, by the chunk that extracts it; the [6,K]
slot table names the ring slot of each window's neighbour; no slot is overwritten while a window still reads it; and the fields
ChunkPlan had before the mode existed keep their values."""
import pytest

from cdfo_amd.streaming import (NEIGHBOUR_SLOTS, NFRAMES, StreamingSR, bank_capacity, bank_runs, bank_slot, check_noise_format,
                                comp_slot_table, generate_input_index, plan_chunks)

CASES = [(T, chunk) for T in range(1, 21) for chunk in range(1, 10)]


def _parent_plan(T, chunk):
    """The seven fields of ChunkPlan as the unshared schedule defines them, restated from the reference loop's index rules."""
    prior = (lambda t: max(1, t)) if T > 1 else (lambda t: 0)
    done = 0
    for c0 in range(0, T, chunk):
        centres = list(range(c0, min(c0 + chunk, T)))
        windows = [generate_input_index(i, NFRAMES, T - 1).tolist() for i in centres]
        reach = max(done, windows[-1][-1] + 1)
        extract = list(range(done, reach))
        done = reach
        yield (centres, windows, [[prior(t) for t in w] for w in windows], [prior(i) for i in centres], extract,
               [prior(t) for t in extract], windows[0][0])


@pytest.mark.parametrize("T,chunk", CASES)
def test_existing_fields_keep_their_values(T, chunk):
    plans = list(plan_chunks(T, chunk))
    want = list(_parent_plan(T, chunk))
    assert len(plans) == len(want)
    for p, w in zip(plans, want):
        assert p._fields[:7] == ("centres", "windows", "priors", "mv_entry", "extract", "extract_priors", "oldest")
        assert tuple(p[:7]) == w


@pytest.mark.parametrize("T,chunk", CASES)
def test_every_frame_is_compensated_once_by_the_chunk_that_extracts_it(T, chunk):
    prior = (lambda t: max(1, t)) if T > 1 else (lambda t: 0)
    seen = []
    for p in plan_chunks(T, chunk):
        assert p.compensate == p.extract
        assert p.compensate_priors == [prior(t) for t in p.compensate]          # rms[max(1, t)], entry 0 if T == 1
        seen += p.compensate
    assert seen == list(range(T))


@pytest.mark.parametrize("T,chunk", CASES)
def test_slot_table_names_ring_slots_that_still_hold_their_frame(T, chunk):
    """The compensation ring follows the feature bank's rule (bank_capacity / bank_slot / bank_runs): after a chunk's frames are
    written, every slot its [6,K] table names holds the frame the window has there, and nothing a chunk (or an earlier one) still
    reads was overwritten."""
    cap = bank_capacity(T, chunk)
    ring = [None] * cap
    for p in plan_chunks(T, chunk):
        k = len(p.centres)
        if p.compensate:
            for slot, off, n in bank_runs(p.compensate[0], len(p.compensate), cap):
                assert 0 <= slot and slot + n <= cap
                for j in range(n):
                    old = ring[slot + j]
                    assert old is None or old < p.oldest, f"T={T} chunk={chunk}: frame {old} overwritten while still needed"
                    ring[slot + j] = p.compensate[off + j]
        table = comp_slot_table(p, cap)
        assert len(table) == (NFRAMES - 1) * k
        for n, slot in enumerate(NEIGHBOUR_SLOTS):
            for w in range(k):
                entry = table[n * k + w]
                assert entry == bank_slot(p.windows[w][slot], cap)
                assert ring[entry] == p.windows[w][slot], f"T={T} chunk={chunk}: slot {entry} holds {ring[entry]}"
    assert NEIGHBOUR_SLOTS == (0, 1, 2, 4, 5, 6)


def test_shared_mode_refuses_per_step_noise_alone():
    """The per-step format (six draws per step) does not convert into the per-frame one: ValueError before any device work."""
    per_step = [[object()] * 6 for _ in range(5)]
    per_frame = [object()] * 5
    with pytest.raises(ValueError, match="frame_noise"):
        check_noise_format(True, per_step, None, 5)
    check_noise_format(True, None, None, 5)                 # default noise
    check_noise_format(True, None, per_frame, 5)
    check_noise_format(True, per_step, per_frame, 5)        # both given: the shared mode reads frame_noise
    check_noise_format(False, per_step, None, 5)
    with pytest.raises(ValueError):
        check_noise_format(True, None, per_frame[:4], 5)    # one tensor per frame
    # run_chunked validates before it touches the device: an object that has only its arguments gets the same answer
    s = object.__new__(StreamingSR)
    s.T, s.noise, s.frame_noise = 5, per_step, None
    with pytest.raises(ValueError, match="frame_noise"):
        s.run_chunked(4, share_compensation=True)
