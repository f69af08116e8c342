"""The counters both drivers of the chunked forward read from their `ChunkRunner` (cdfo_amd/streaming.py): T = 9 frames of 24 x 40 at
chunk 4, the values the docstrings of `StreamingSR` and `LiveSR` state."""
import numpy as np
import pytest

from test_gpu_sequence import _model, _sequence

pytestmark = pytest.mark.gpu
T, H, W = 9, 24, 40


def test_run_chunked_keeps_no_ring_after_the_pass():
    """The rings belong to the pass: a `StreamingSR` that has run holds its counters, not the feature bank or the compensation ring
    (a condition, not a measurement: less than one ring of 10 frames stays allocated once the outputs are dropped)."""
    import torch
    from cdfo_amd.streaming import StreamingSR
    s = StreamingSR(_model(21)[1], *_sequence(T, H, W, 7))
    s.run_chunked(4, share_compensation=True)                                  # weight packing, first-touch allocations
    for shared in (False, True):
        before = torch.cuda.memory_allocated()
        s.run_chunked(4, share_compensation=shared)
        held = torch.cuda.memory_allocated() - before
        print(f"share_compensation={shared}: {held} bytes held after the pass")
        assert held < 10 * H * W * 64 * 4 and s.frames_extracted == T


def test_counters_of_both_drivers_per_pass():
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    model = _model(21)[1]
    seq = _sequence(T, H, W, 7)
    s = StreamingSR(model, *seq)
    assert (s.seconds, s.frames_extracted, s.frames_compensated) == (0.0, 0, 0)
    for shared, compensated in ((False, 0), (True, T), (False, 0)):            # every run_chunked starts from zero again
        before = model.frames_extracted
        outs = s.run_chunked(4, share_compensation=shared)
        print(f"run_chunked(4, share_compensation={shared}): seconds {s.seconds:.4f}, extracted {s.frames_extracted}, compensated "
              f"{s.frames_compensated}")
        assert len(outs) == T and model.frames_extracted - before == T
        assert s.frames_extracted == T and s.frames_compensated == compensated
        assert s.seconds > 0 and s.fps == T / s.seconds
    lr, pms, rms, ufs, _, mvl1 = seq
    for shared, compensated in ((False, 0), (True, T)):
        live = LiveSR(model, H, W, chunk=4, share_compensation=shared)
        assert (live.seconds, live.frames_extracted, live.frames_compensated) == (0.0, 0, 0)
        for t in range(T):
            live.push(lr[t].astype(np.uint8), pms[t].astype(np.uint8), rms[t], ufs[t].astype(np.uint8), mvl1[t])
        live.close()
        print(f"LiveSR(chunk=4, share_compensation={shared}): seconds {live.seconds:.4f}, extracted {live.frames_extracted}, "
              f"compensated {live.frames_compensated}")
        assert live.frames_extracted == T and live.frames_compensated == compensated and live.frames_out == T
        assert live.seconds > 0 and live.fps == T / live.seconds
        assert live.resident_bytes == 10 * (H * W * (1 + 1 + 1 + 4 + 12) + H * W * 256 * (2 if shared else 1)) and live.ring_capacity == 10
