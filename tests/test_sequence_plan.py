"""The schedule of chunked sequence inference (cdfo_amd.streaming.plan_chunks): pure Python, no GPU.  For every sequence length
1..20 and chunk size 1..9 it must restate the reference loop's index rules (generate_input_index, ii = max(1, i)), visit every
centre once and in order, extract every frame exactly once, and never ask the bank for a frame it has dropped."""
import pytest

from cdfo_amd.streaming import NFRAMES, bank_capacity, bank_runs, bank_slot, generate_input_index, plan_chunks


@pytest.mark.parametrize("chunk", range(1, 10))
@pytest.mark.parametrize("T", range(1, 21))
def test_plan_restates_the_reference_loop(T, chunk):
    plans = list(plan_chunks(T, chunk))
    prior = (lambda t: max(1, t)) if T > 1 else (lambda t: 0)
    centres, extracted, bank = [], [], set()
    for p in plans:
        assert 1 <= len(p.centres) <= chunk
        assert len(p.windows) == len(p.priors) == len(p.mv_entry) == len(p.centres)
        assert len(p.extract_priors) == len(p.extract)
        for i, win, pri, mv in zip(p.centres, p.windows, p.priors, p.mv_entry):
            want = generate_input_index(i, NFRAMES, T - 1).tolist()
            assert win == want
            assert pri == [prior(t) for t in want]
            assert mv == prior(i)
        assert p.extract == list(range(len(extracted), len(extracted) + len(p.extract)))      # consecutive, nothing twice
        assert p.extract_priors == [prior(t) for t in p.extract]
        # the bank: what this chunk extracts comes in, what lies below `oldest` may go; every window frame must be there
        bank |= set(p.extract)
        bank = {t for t in bank if t >= p.oldest}
        need = {t for w in p.windows for t in w}
        assert need <= bank, f"T={T} chunk={chunk}: centres {p.centres} need {sorted(need - bank)}, dropped or never extracted"
        assert len(bank) <= chunk + NFRAMES - 1
        centres += p.centres
        extracted += p.extract
    assert centres == list(range(T))                       # every centre once, in order
    assert sorted(extracted) == list(range(T)) == extracted    # every frame extracted exactly once
    assert all(len(p.centres) == chunk for p in plans[:-1])  # only the last chunk may be short


@pytest.mark.parametrize("chunk", range(1, 10))
@pytest.mark.parametrize("T", range(1, 21))
def test_bank_ring_holds_what_the_windows_read(T, chunk):
    """The slot mapping the device code uses (bank_capacity / bank_slot / bank_runs, the functions run_chunked itself calls):
    after a chunk's extraction is written into the ring, every slot its window stack gathers holds the frame the plan names,
    and what the extraction overwrote lies below the plan's `oldest`."""
    cap = bank_capacity(T, chunk)
    assert cap <= chunk + NFRAMES - 1
    ring = [None] * cap
    for p in plan_chunks(T, chunk):
        if p.extract:
            runs = bank_runs(p.extract[0], len(p.extract), cap)
            assert 1 <= len(runs) <= 2 and sum(n for _, _, n in runs) == len(p.extract)
            for slot, off, n in runs:
                assert 0 <= slot and slot + n <= cap
                for j in range(n):
                    old = ring[slot + j]
                    assert old is None or old < p.oldest, f"T={T} chunk={chunk}: frame {old} overwritten while still needed"
                    ring[slot + j] = p.extract[off + j]
        for win in p.windows:
            for t in win:
                assert ring[bank_slot(t, cap)] == t, f"T={T} chunk={chunk}: slot of frame {t} holds {ring[bank_slot(t, cap)]}"


def test_plan_refuses_empty_sequences_and_chunks():
    for T, chunk in ((0, 4), (5, 0), (-1, 1)):
        with pytest.raises(ValueError):
            list(plan_chunks(T, chunk))
