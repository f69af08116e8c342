"""Live sequence inference on the GPU (cdfo_amd/live.py::LiveSR): frames pushed one at a time against
``StreamingSR.run_chunked`` on the completed sequence.  The inputs are bit-identical and the model calls are the same calls, so
every comparison is ``torch.equal``.  The model and the sequence are those of tests/test_gpu_sequence.py: frames of 16 x 24."""
import numpy as np
import pytest
import torch

from test_gpu_sequence import _model, _scaled_state, _sequence

pytestmark = pytest.mark.gpu
H, W = 16, 24


@pytest.fixture(scope="module")
def model():
    return _model(21)[1]


def _centre_noise(T, seed):
    from oracle.cvsr_v8_ref import make_inputs
    return [[u.cuda() for u in make_inputs(1, H, W, seed + i)["gumbel_u"]] for i in range(T)]


def _frame_noise(T, seed):
    from oracle.cvsr_v8_ref import make_inputs
    return [make_inputs(1, H, W, seed + t)["gumbel_u"][0].cuda() for t in range(T)]


def _push_all(s, seq, kind=np.uint8, device=None):
    """Push the sequence frame by frame, filling the caller's arrays with garbage as soon as each push returns.  Returns the frames
    in arrival order and {index: the push that returned it, or None for close()}."""
    lr, pms, rms, ufs, _, mvl1 = seq
    frames, arrival = [], {}
    for t in range(lr.shape[0]):
        args = [lr[t].astype(kind), pms[t].astype(np.uint8), rms[t].copy(), ufs[t].astype(kind), mvl1[t].copy()]
        if device is not None:
            args = [torch.from_numpy(a).to(device) for a in args]
        done = s.push(*args)
        for a in args:
            a.fill(77) if isinstance(a, np.ndarray) else a.fill_(77)
        for i, f in done:
            arrival[i] = t
            frames.append((i, f))
    for i, f in s.close():
        arrival[i] = None
        frames.append((i, f))
    return frames, arrival


def _assert_equal(frames, want, T):
    assert [i for i, _ in frames] == list(range(T)) and len(want) == T
    for (i, f), w in zip(frames, want):
        assert tuple(f.shape) == (1, 1, 4 * H, 4 * W) and f.dtype == torch.float32
        assert torch.equal(f, w), f"frame {i}: max-abs {(f - w).abs().max().item():.3e}"


def _assert_arrivals(arrival, T, chunk):
    for i in range(T):
        release = i // chunk * chunk + chunk + 2           # the push of frame c0 + chunk + 2, else close()
        assert arrival[i] == (release if release < T else None), (i, chunk)


@pytest.mark.parametrize("chunk", [1, 4, 8, 16])
def test_live_equals_run_chunked_with_injected_noise(chunk, model):
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    T = 11
    seq, noise = _sequence(T, H, W, 5), _centre_noise(T, 300)
    want = StreamingSR(model, *seq, gumbel_uniform=noise).run_chunked(chunk)
    s = LiveSR(model, H, W, chunk=chunk, gumbel_uniform=noise)
    frames, arrival = _push_all(s, seq)
    _assert_equal(frames, want, T)
    _assert_arrivals(arrival, T, chunk)
    assert s.frames_extracted == T and s.frames_pushed == T and s.frames_out == T and s.frames_compensated == 0
    assert s.ring_capacity == chunk + 6 and s.fps > 0


@pytest.mark.parametrize("chunk", [1, 4, 8])
def test_live_shared_compensation_equals_run_chunked(chunk, model):
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    T = 11
    seq, noise = _sequence(T, H, W, 5), _frame_noise(T, 700)
    want = StreamingSR(model, *seq, frame_noise=noise).run_chunked(chunk, share_compensation=True)
    s = LiveSR(model, H, W, chunk=chunk, share_compensation=True, frame_noise=lambda t: noise[t])       # the callable form
    frames, arrival = _push_all(s, seq)
    _assert_equal(frames, want, T)
    _assert_arrivals(arrival, T, chunk)
    assert s.frames_extracted == T and s.frames_compensated == T


@pytest.mark.parametrize("shared", [False, True])
def test_live_default_noise_follows_the_generator_like_run_chunked(shared, model):
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    T = 9
    seq = _sequence(T, H, W, 9)
    torch.manual_seed(1234)
    want = StreamingSR(model, *seq).run_chunked(4, share_compensation=shared)
    torch.manual_seed(1234)
    frames, _ = _push_all(LiveSR(model, H, W, chunk=4, share_compensation=shared), seq)
    _assert_equal(frames, want, T)


@pytest.mark.parametrize("shared", [False, True])
def test_live_ring_wrap(shared, model):
    """T = 23 at chunk 4: capacity 10, every slot is rewritten twice."""
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    T = 23
    seq = _sequence(T, H, W, 11)
    kw = dict(frame_noise=_frame_noise(T, 900)) if shared else dict(gumbel_uniform=_centre_noise(T, 900))
    want = StreamingSR(model, *seq, **kw).run_chunked(4, share_compensation=shared)
    s = LiveSR(model, H, W, chunk=4, share_compensation=shared, **kw)
    frames, arrival = _push_all(s, seq)
    _assert_equal(frames, want, T)
    _assert_arrivals(arrival, T, 4)
    assert s.frames_extracted == T and s.frames_compensated == (T if shared else 0)


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_live_short_streams_come_out_of_close(T, model):
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    seq, noise = _sequence(T, H, W, 13), _centre_noise(T, 100)
    want = StreamingSR(model, *seq, gumbel_uniform=noise).run_chunked(4)
    s = LiveSR(model, H, W, chunk=4, gumbel_uniform=noise)
    frames, arrival = _push_all(s, seq)
    _assert_equal(frames, want, T)
    assert all(a is None for a in arrival.values()) and s.frames_extracted == T


def test_live_high_bit_depth(model):
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    T, peak = 6, 1023
    lr, pms, rms, ufs, mvl0, mvl1 = _sequence(T, H, W, 15)
    seq = (np.round(lr * 4 + 1), pms, rms * 4, np.round(ufs * 4 + 3), mvl0, mvl1)          # samples over 0 .. 1023
    noise = _centre_noise(T, 200)
    want = StreamingSR(model, *seq, gumbel_uniform=noise, peak=peak).run_chunked(4)
    frames, _ = _push_all(LiveSR(model, H, W, chunk=4, peak=peak, gumbel_uniform=noise), seq, kind=np.uint16)
    _assert_equal(frames, want, T)


def test_live_takes_tensors_on_the_device(model):
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    T = 9
    seq, noise = _sequence(T, H, W, 17), _centre_noise(T, 400)
    want = StreamingSR(model, *seq, gumbel_uniform=noise).run_chunked(4)
    frames, _ = _push_all(LiveSR(model, H, W, chunk=4, gumbel_uniform=noise), seq, device="cuda")
    _assert_equal(frames, want, T)


def test_live_range_guard_recompensates_from_the_ring():
    """Trunk activations x 2^16 (test_run_chunked_range_guard_repairs_an_overflowing_chunk's model), shared mode: every chunk
    leaves fp16's range and is repeated in bf16x3 with the compensation of its frames recomputed from the residual ring."""
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.live import LiveSR
    from cdfo_amd.streaming import StreamingSR
    from oracle.cvsr_v8_ref import make_state_dict
    T = 5
    seq, noise = _sequence(T, H, W, 6), _frame_noise(T, 500)
    m16 = CVSR_V8()
    m16.load_state_dict(_scaled_state(make_state_dict(3), 2.0 ** 16), strict=True)
    m16 = m16.cuda().eval()
    s = LiveSR(m16, H, W, chunk=4, share_compensation=True, frame_noise=noise)
    with pytest.warns(UserWarning, match="fp16 range"):                  # (the model warns once: the live stream goes first)
        frames, _ = _push_all(s, seq)
    assert m16.last_range is not None and m16.last_range["fallback"] and m16._probe is None
    assert all(torch.isfinite(f).all() for _, f in frames)
    assert s.frames_extracted == T and s.frames_compensated > T          # the repeated chunks recompensated their windows
    _assert_equal(frames, StreamingSR(m16, *seq, frame_noise=noise).run_chunked(4, share_compensation=True), T)


def test_live_device_state_does_not_grow_with_the_stream(model):
    from cdfo_amd.live import LiveSR
    sizes = []
    for T in (12, 32):
        s = LiveSR(model, H, W, chunk=4)
        frames, _ = _push_all(s, _sequence(T, H, W, 19))
        assert len(frames) == T and s.frames_extracted == T
        sizes.append((s.resident_bytes, s.ring_capacity))
    assert sizes[0] == sizes[1] and sizes[0][1] == 4 + 6
    # two uint8 planes, one uint8 mask, the fp32 residual and the fp32 field per slot, and the bank's 64 fp32 channels
    assert sizes[0][0] == 10 * H * W * (1 + 1 + 1 + 4 + 12 + 256)


def test_live_misuse_raises_before_any_launch(model, monkeypatch):
    from cdfo_amd import kernels as K
    from cdfo_amd.live import LiveSR
    lr, pms, rms, ufs, _, mvl1 = _sequence(2, H, W, 3)
    u8 = lambda a: a.astype(np.uint8)
    good = [u8(lr[0]), u8(pms[0]), rms[0], u8(ufs[0]), mvl1[0]]
    s = LiveSR(model, H, W, chunk=4)
    launches = []
    monkeypatch.setattr(K, "live_planes", lambda *a, **k: launches.append(a))
    before = model.frames_extracted
    for at, bad in ((0, u8(lr[0])[:, :-1]), (1, u8(pms[0])[:-1]), (4, mvl1[0][..., :2]), (0, lr[0].astype(np.uint16)),
                    (3, ufs[0].astype(np.float32)), (1, pms[0].astype(np.float32)), (2, rms[0].astype(np.complex64))):
        args = list(good)
        args[at] = bad
        with pytest.raises(ValueError):
            s.push(*args)
    assert s.frames_pushed == 0
    with pytest.raises(ValueError):                                        # the per-step format does not convert (check_noise_format)
        LiveSR(model, H, W, share_compensation=True, gumbel_uniform=[])
    with pytest.raises(ValueError):
        LiveSR(model, H, W, peak=70000)
    assert s.close() == []
    with pytest.raises(RuntimeError):
        s.push(*good)
    with pytest.raises(RuntimeError):
        s.close()
    assert not launches and model.frames_extracted == before
