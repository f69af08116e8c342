"""The bank-side index table of a chunk (cdfo_amd/streaming.py::ChunkRunner.head / split_head): pure Python and host tensors, no GPU.
For every (T, chunk) of tests/test_sequence_plan.py, at the capacity of `run_chunked` and at that of `LiveSR`, the table is the
literal expression the two drivers used to write out, 7 K entries in either mode, and `split_head` cuts it where they cut it."""
from types import SimpleNamespace

import pytest
import torch

from cdfo_amd.streaming import NFRAMES, ChunkRunner, bank_capacity, bank_slot, comp_slot_table, plan_chunks

_MODEL = SimpleNamespace(extract_features=None, compensate_features=None, forward_windows=None, forward_windows_shared=None)


def _runner(capacity, shared, model=_MODEL):
    return ChunkRunner(model, torch.device("cpu"), 8, 8, capacity, shared, None, None, lambda: None)


@pytest.mark.parametrize("chunk", range(1, 10))
@pytest.mark.parametrize("T", range(1, 21))
def test_head_is_the_table_the_drivers_wrote_out(T, chunk):
    for cap in (bank_capacity(T, chunk), chunk + NFRAMES - 1):
        unshared, shared = _runner(cap, False), _runner(cap, True)
        assert tuple(shared.bank.shape) == tuple(shared.comp_bank.shape) == (cap, 8, 8, 64) and unshared.comp_bank is None
        for p in plan_chunks(T, chunk):
            k = len(p.centres)
            head = unshared.head(p)
            assert head == [bank_slot(p.windows[j][n], cap) for n in range(NFRAMES) for j in range(k)]       # slot-major window stack
            assert len(head) == 7 * k and all(type(v) is int for v in head)
            head_t = torch.tensor(head + [-1] * 5, dtype=torch.int32)[:len(head)]
            (lf_idx,) = unshared.split_head(head_t, k)
            assert lf_idx.tolist() == head
            head = shared.head(p)
            assert head == comp_slot_table(p, cap) + [bank_slot(i, cap) for i in p.centres]
            assert len(head) == 7 * k and all(type(v) is int for v in head)
            idx = torch.tensor(head + [-1] * 5, dtype=torch.int32)                   # followed by an owner's input-side tables
            comp_idx, centre_idx = shared.split_head(idx[:len(head)], k)
            assert torch.equal(comp_idx, idx[:6 * k]) and torch.equal(centre_idx, idx[6 * k:7 * k])
            assert comp_idx.tolist() == comp_slot_table(p, cap) and centre_idx.tolist() == [bank_slot(i, cap) for i in p.centres]


def test_resident_bytes_counts_the_rings_of_the_mode():
    assert _runner(10, False).resident_bytes == 10 * 8 * 8 * 64 * 4
    assert _runner(10, True).resident_bytes == 2 * 10 * 8 * 8 * 64 * 4


@pytest.mark.parametrize("shared,missing", [(False, "forward_windows"), (False, "extract_features"), (True, "compensate_features"),
                                            (True, "forward_windows_shared")])
def test_a_model_without_the_calls_is_refused_before_anything_is_allocated(shared, missing, monkeypatch):
    model = SimpleNamespace(**{n: None for n in vars(_MODEL) if n != missing})
    monkeypatch.setattr(torch, "empty", lambda *a, **k: pytest.fail("allocated before the capability check"))
    with pytest.raises(NotImplementedError, match="needs a model with"):
        _runner(10, shared, model)
