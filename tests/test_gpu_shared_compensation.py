"""Chunked inference with each neighbour frame's compensation computed once (StreamingSR.run_chunked(share_compensation=True)):
cdfo_flow_warp_frames against gather + flow_warp (exact), the shared mode against the oracle's restatement of the reference loop
fed the tied per-step noise, against the unshared mode fed the same, its counters, its default noise and its range guard.
Every figure is printed before it is asserted (run with -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_sequence import _model, _scaled_state, _sequence

pytestmark = pytest.mark.gpu
TOL = 1e-3            # the project's parity bound against the fp32 reference (README)
SAME_KERNELS = 2e-5   # the gate of test_run_chunked_matches_the_oracle_loop_and_run between run_chunked and run()
SLOTS = (0, 1, 2, 4, 5, 6)


# ------------------------------------------------------------------------------------------------------ cdfo_flow_warp_frames
def _flows(K, H, W, seed):
    """[K,7,2,H,W]: sub-pixel values, a block of zeros, values beyond every border, +-inf and NaN."""
    g = torch.Generator().manual_seed(seed)
    mv = torch.randn((K, 7, 2, H, W), generator=g) * 2.5
    mv[:, :, :, :2, :3] = 0.0
    mv[:, :, 0, 3, :] = 100.0          # right of the image
    mv[:, :, 0, 4, :] = -100.0         # left
    mv[:, :, 1, 5, :] = 100.0          # below
    mv[:, :, 1, 6, :] = -100.0         # above
    mv[:, :, 0, 7, 0] = float("inf")
    mv[:, :, 1, 7, 1] = float("-inf")
    mv[:, :, 0, 7, 2] = float("nan")
    mv[:, :, :, 7, 3] = float("nan")
    mv[:, :, 0, 2, 5] = 0.5            # exactly between two pixels
    mv[:, :, 1, 2, 5] = -1.0           # a whole pixel
    return mv.cuda()


@pytest.mark.parametrize("slot0", [0, 4])
@pytest.mark.parametrize("Kw", [1, 3])
@pytest.mark.parametrize("H,W,ld", [(8, 12, 64), (9, 13, 64), (9, 13, 128)])
def test_flow_warp_frames_equals_gather_plus_warp(H, W, ld, Kw, slot0):
    """Banks of 5 frames, C = 64 (pitch 64, and 128 on input and output), G = 3: indices that repeat, one at -1 and one at
    n_bank (frames of zeros).  Exact: max-abs 0.0 and the same bit patterns as gather_frames + flow_warp per slot."""
    from cdfo_amd import kernels as K
    n_bank, G, Cc = 5, 3, 64
    g = torch.Generator().manual_seed(11 * H + W + Kw)
    wide = (torch.randn((n_bank, H, W, ld), generator=g) * 3).cuda()
    bank = wide[..., :Cc]
    idx = torch.tensor([4, 4, 0, 2, -1, 3, n_bank, 1, 4][:G * Kw] if Kw == 3 else [2, -1, n_bank], dtype=torch.int32).cuda()
    if Kw == 1 and slot0 == 4:
        idx = torch.tensor([3, 3, 0], dtype=torch.int32).cuda()
    mv = _flows(Kw, H, W, 5 + slot0)
    stride = 14 * H * W
    gathered = K.gather_frames(bank.contiguous(), idx)
    want = torch.cat([K.flow_warp(gathered[s * Kw:(s + 1) * Kw], mv[:, slot0 + s], stride) for s in range(G)])
    wide_out = torch.full((G * Kw, H, W, ld), 7.0, device="cuda")
    out = wide_out[..., :Cc]
    assert K.flow_warp_frames(bank, idx, mv, stride, slot0, G, Kw, out=out) is out
    d = (out - want).abs().max().item()
    print(f"{H}x{W} ld {ld} K {Kw} slot0 {slot0}: max-abs vs gather + flow_warp {d}")
    assert d == 0.0 and torch.equal(out.contiguous().view(torch.int32), want.view(torch.int32))
    assert torch.isfinite(out).all() and want.abs().max().item() > 1.0            # the case samples something
    for j, s in enumerate(idx.tolist()):
        if s < 0 or s >= n_bank:
            assert not out[j].any()
    if ld > Cc:
        assert (wide_out[..., Cc:] == 7.0).all()                                   # nothing written beyond the C channels
    fresh = K.flow_warp_frames(bank, idx, mv, stride, slot0, G, Kw)
    assert torch.equal(fresh, out.contiguous())


def test_flow_warp_frames_refuses_bad_arguments():
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    H, W, Cc, n, G, Kw = 8, 8, 64, 3, 3, 2
    bank = torch.randn((n, H, W, Cc), device="cuda")
    idx = torch.zeros(G * Kw + 1, dtype=torch.int32, device="cuda")
    mv = torch.zeros((Kw, 7, 2, H, W), device="cuda")
    out = torch.full((G * Kw, H, W, Cc), 7.0, device="cuda")
    f = _lib.lib().cdfo_flow_warp_frames
    stream = K._stream()

    def call(bank_p=bank.data_ptr(), ldi=Cc, n_bank=n, idx_p=idx.data_ptr(), mv_p=mv.data_ptr(), ks=14 * H * W, slot0=0, g=G, k=Kw,
             h=H, w=W, c=Cc, out_p=out.data_ptr(), ldo=Cc):
        return f(C.c_void_p(bank_p), ldi, n_bank, C.c_void_p(idx_p), C.c_void_p(mv_p), C.c_longlong(ks), slot0, g, k, h, w, c,
                 C.c_void_p(out_p), ldo, stream)

    einval = [dict(g=0), dict(k=0), dict(n_bank=0), dict(c=6), dict(c=0), dict(ldi=66), dict(ldo=62), dict(ldi=32), dict(ldo=32),
              dict(h=0), dict(w=-1), dict(slot0=-1), dict(ks=-1), dict(g=256, k=256), dict(idx_p=None), dict(bank_p=None),
              dict(mv_p=None), dict(out_p=None)]
    for kw in einval:
        assert call(**kw) == -1, kw                                               # CDFO_EINVAL
    ealign = [dict(bank_p=bank.data_ptr() + 4), dict(out_p=out.data_ptr() + 8), dict(idx_p=idx.data_ptr() + 2),
              dict(mv_p=mv.data_ptr() + 2)]
    for kw in ealign:
        assert call(**kw) == -2, kw                                               # CDFO_EALIGN
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                     # nothing was launched
    assert call(idx_p=idx.data_ptr() + 4) == 0                                    # a 4-byte aligned table is enough
    torch.cuda.synchronize()
    assert torch.equal(out, K.flow_warp(bank[:1].repeat(G * Kw, 1, 1, 1), mv[:1, 0].repeat(G * Kw, 1, 1, 1), 2 * H * W))
    with pytest.raises(ValueError):
        K.flow_warp_frames(bank, idx[:5], mv, 14 * H * W, 0, G, Kw)
    with pytest.raises(ValueError):
        K.flow_warp_frames(bank, idx[:6].long(), mv, 14 * H * W, 0, G, Kw)


# ------------------------------------------------------------------------------------------------------------- the shared mode
def _frame_noise(T, H, W, seed):
    from oracle.cvsr_v8_ref import make_inputs
    return [make_inputs(1, H, W, seed + t)["gumbel_u"][0] for t in range(T)]


def _tied(u, T):
    """The per-step lists that give every (step, slot) the draw of the FRAME it holds: [u[w[i][n]] for n in 0, 1, 2, 4, 5, 6]."""
    from cdfo_amd.streaming import generate_input_index
    w = [generate_input_index(i, 7, T - 1).tolist() for i in range(T)]
    return [[u[w[i][n]] for n in SLOTS] for i in range(T)]


def _reference_loop(sd, seq, per_step):
    """oracle.streaming_ref.stream_sequence.  Its `max(1, i)` has no entry to read in a sequence of ONE frame; there the project's
    rule (entry 0 if T == 1) is restated around the oracle's forward: one step, seven copies of frame 0, every flow zeroed by the
    two end rules."""
    from oracle.cvsr_v8_ref import cvsr_v8_forward
    from oracle.streaming_ref import modify_mv_for_end_frames, mv2mvs, stream_sequence
    lr, pms, rms, ufs, mvl0, mvl1 = seq
    if lr.shape[0] > 1:
        return stream_sequence(sd, lr / 255.0, pms / 255.0, rms / 255.0, ufs / 255.0, mvl0, mvl1, per_step)
    win = lambda a: torch.from_numpy((a / 255.0)[[0] * 7])[None, :, None]
    m0, m1 = (torch.from_numpy(modify_mv_for_end_frames(0, np.transpose(mv2mvs(m[0]), (0, 3, 1, 2))[None].copy(), 1)) for m in (mvl0, mvl1))
    return [cvsr_v8_forward(sd, win(lr), m0, m1, win(pms), win(rms), win(ufs), None, per_step[0])[0]]


@pytest.fixture(scope="module")
def shared_case():
    """T = 11 frames of 16 x 24, the inputs of test_gpu_sequence.py::oracle_case, one noise tensor per frame; the oracle loop with
    the tied per-step noise, once for every test that needs it."""
    T, H, W = 11, 16, 24
    sd, model = _model(21)
    seq = _sequence(T, H, W, 5)
    u = _frame_noise(T, H, W, 300)
    ref = _reference_loop(sd, seq, _tied(u, T))
    return sd, model, seq, [t.cuda() for t in u], ref


@pytest.mark.parametrize("chunk", [1, 4, 8, 16])
def test_shared_mode_matches_the_reference_loop(chunk, shared_case):
    """Every frame within 1e-3 of the reference loop fed the noise of the frame each (step, slot) holds; each frame extracted and
    compensated once.  Measured on an MI355X: see DESIGN section 5.00000."""
    from cdfo_amd.streaming import StreamingSR
    T, H, W = 11, 16, 24
    sd, model, seq, u, ref = shared_case
    s = StreamingSR(model, *seq, frame_noise=u)
    outs = s.run_chunked(chunk, share_compensation=True)
    assert len(outs) == T and s.fps > 0
    assert s.frames_compensated == T and s.frames_extracted == T
    err = [(o.cpu() - r).abs().max().item() for o, r in zip(outs, ref)]
    print(f"shared, chunk {chunk}: vs the reference loop max {max(err):.2e}; per frame {['%.1e' % e for e in err]}")
    for i, o in enumerate(outs):
        assert tuple(o.shape) == (1, 1, 4 * H, 4 * W)
        assert err[i] <= TOL, f"frame {i}: max-abs {err[i]} against the reference loop"


@pytest.mark.parametrize("T", [1, 2, 5])
def test_shared_mode_on_sequences_whose_every_window_is_clipped(T):
    """8 x 8, chunk 4: every window repeats frame 0 or T - 1 in several slots, which then share that frame's one draw."""
    from cdfo_amd.streaming import StreamingSR
    H = W = 8
    sd, model = _model(23)
    seq = _sequence(T, H, W, 40 + T)
    u = _frame_noise(T, H, W, 700)
    ref = _reference_loop(sd, seq, _tied(u, T))
    s = StreamingSR(model, *seq, frame_noise=[t.cuda() for t in u])
    outs = s.run_chunked(4, share_compensation=True)
    assert s.frames_compensated == T and s.frames_extracted == T
    err = [(o.cpu() - r).abs().max().item() for o, r in zip(outs, ref)]
    print(f"shared, T = {T} at 8x8: vs the reference loop max {max(err):.2e}")
    assert len(outs) == T and max(err) <= TOL


@pytest.mark.parametrize("precision", ["fp16x2", "bf16x3"])
def test_shared_mode_matches_the_unshared_mode_under_tied_noise(precision, shared_case):
    """The unshared mode with dnoise[i][d] = u[w[i][slot d]] computes the same function: within 2e-5 at chunk 1, 4, 8, 16."""
    from cdfo_amd.streaming import StreamingSR
    T = 11
    sd, model, seq, u, ref = shared_case
    model.precision = precision
    try:
        worst = {}
        for chunk in (1, 4, 8, 16):
            a = StreamingSR(model, *seq, frame_noise=u).run_chunked(chunk, share_compensation=True)
            b = StreamingSR(model, *seq, gumbel_uniform=_tied(u, T)).run_chunked(chunk)
            worst[chunk] = max((x - y).abs().max().item() for x, y in zip(a, b))
    finally:
        model.precision = "fp16x2"
    print(f"shared vs unshared, {precision}: max-abs per chunk size {worst}")
    for chunk, d in worst.items():
        assert d <= SAME_KERNELS, f"chunk {chunk}: {d}"


def test_shared_mode_default_noise_is_seeded_fresh_and_independent_of_the_chunk_size():
    """Noise drawn in the mask kernel, one key per run and draw = frame index: the same generator state gives the same frames,
    another state other masks, and chunk 4 and chunk 8 draw the same uniforms for every frame."""
    from cdfo_amd.streaming import StreamingSR
    T, H, W = 10, 16, 24
    _, model = _model(22)
    seq = _sequence(T, H, W, 9)

    def run(seed, chunk):
        torch.manual_seed(seed)
        s = StreamingSR(model, *seq)
        outs = s.run_chunked(chunk, share_compensation=True)
        assert s.frames_compensated == T and s.frames_extracted == T
        return outs
    a, b, c, d = run(1234, 4), run(1234, 4), run(4321, 4), run(1234, 8)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
    dif = max((x - y).abs().max().item() for x, y in zip(a, d))
    other = max((x - y).abs().max().item() for x, y in zip(a, c))
    print(f"default noise: chunk 4 vs chunk 8 under one seed {dif:.2e}; another seed {other:.2e}")
    assert dif <= SAME_KERNELS
    assert SAME_KERNELS < other < 1e-2


def test_shared_mode_range_guard_repairs_an_overflowing_chunk():
    """The scenario of test_run_chunked_range_guard_repairs_an_overflowing_chunk in the shared mode: trunk activations x 2^16, every
    chunk leaves fp16's range and is repeated in bf16x3 from a recomputed scratch stack; the compensation ring keeps its bits."""
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.streaming import StreamingSR
    from oracle.cvsr_v8_ref import make_state_dict
    T, H, W = 5, 16, 24
    seq = _sequence(T, H, W, 6)
    u = [t.cuda() for t in _frame_noise(T, H, W, 500)]
    sd = make_state_dict(3)

    def load(state):
        m = CVSR_V8()
        m.load_state_dict(state, strict=True)
        return m.cuda().eval()
    shared = lambda m: StreamingSR(m, *seq, frame_noise=u)
    want = shared(load(sd)).run_chunked(4, share_compensation=True)                 # the same function, inside fp16's range
    m16 = load(_scaled_state(sd, 2.0 ** 16))
    m16.precision = "bf16x3"
    exact = shared(m16).run_chunked(4, share_compensation=True)
    m16.precision = "fp16x2"
    banks = []
    inner = m16.forward_windows_shared

    def watched(Lc, comp_bank, comp_idx, *a, **kw):
        before = comp_bank.clone()
        out = inner(Lc, comp_bank, comp_idx, *a, **kw)
        banks.append((before, comp_bank.clone(), m16.last_range["fallback"]))
        return out
    m16.forward_windows_shared = watched
    s = shared(m16)
    try:
        with pytest.warns(UserWarning, match="fp16 range"):
            got = s.run_chunked(4, share_compensation=True)
    finally:
        del m16.forward_windows_shared
    assert m16.last_range is not None and m16.last_range["fallback"] and m16._probe is None      # settled on return
    assert len(banks) == 2 and all(rejected for _, _, rejected in banks)
    for before, after, _ in banks:                                                  # the ring is not rewritten by the repair
        assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    assert s.frames_extracted == T
    for i in range(T):
        assert torch.isfinite(got[i]).all()
        d_exact, d_want = (got[i] - exact[i]).abs().max().item(), (got[i] - want[i]).abs().max().item()
        print(f"frame {i}: repaired vs bf16x3 {d_exact:.2e}, vs the unscaled model {d_want:.2e}")
        assert d_exact <= TOL and d_want <= TOL
