"""Chunked sequence inference on the GPU: the two kernels of sequence.hip against the host functions they restate (exact), and
StreamingSR.run_chunked against the oracle's restatement of the reference loop and against the per-frame loop `run()`.
Frames of 16x24 and 21x27; every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-3            # the project's parity bound against the fp32 reference (README)
SAME_KERNELS = 2e-5   # cached vs fresh path in tests/test_streaming.py: same kernels, another image count per launch


def _sequence(T, H, W, seed):
    """Inputs of tests/test_streaming.py::_sequence."""
    rs = np.random.RandomState(seed)
    lr = rs.randint(0, 256, size=(T, H, W)).astype(np.float32)
    pms = rs.randint(0, 256, size=(T, H, W)).astype(np.float32)
    ufs = rs.randint(0, 256, size=(T, H, W)).astype(np.float32)
    rms = np.clip(np.round(rs.randn(T, H, W) * 6), -128, 127).astype(np.float32)
    mv = rs.randint(-64, 64, size=(2, T, H // 8, W // 8, 3)).astype(np.float32)
    mv[..., 2] = rs.choice([-2.0, -1.0, 1.0], size=mv.shape[:-1])
    mv = np.repeat(np.repeat(mv, 8, axis=2), 8, axis=3)
    return lr, pms, rms, ufs, mv[0], mv[1]


def _model(seed):
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_state_dict
    sd = make_state_dict(seed, perturb=True)
    m = CVSR_V8()
    m.load_state_dict(sd, strict=True)
    return sd, m.cuda().eval()


def _scaled_state(sd, s):
    """The same function with the trunk's activations multiplied by s, a power of two (the re-parametrisation of
    tests/test_gpu_range_and_noise.py: the trunk between tsa_fusion and upconv1 is positively homogeneous)."""
    out = {k: v.clone() for k, v in sd.items()}
    out["tsa_fusion.weight"] *= s
    out["tsa_fusion.bias"] *= s
    for k in out:
        if k.startswith("recon_trunk.") and k.endswith(".bias"):
            out[k] *= s
    out["upconv1.weight"] /= s
    return out


def _host_flows(mvl, i, T, Hp, Wp):
    """What StreamingSR._mvs builds for centre i, on the CPU (IEEE arithmetic): [7,2,Hp,Wp]."""
    from cdfo_amd.streaming import modify_mv_for_end_frames, mv2mvs
    H, W = mvl.shape[1:3]
    m = torch.zeros((7, 2, Hp, Wp), dtype=torch.float32)
    m[:, :, :H, :W] = mv2mvs(mvl[max(1, i) if T > 1 else 0])
    return modify_mv_for_end_frames(i, m.unsqueeze(0), T)[0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.float64])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 11])
def test_seq_flows_equals_the_host_functions(T, dtype):
    """Every centre of sequences of 1, 2, 3, 4, 7 and 11 frames (all six boundary rules and their overlaps), a field with zeros
    (0 / 0 -> NaN -> 0, x / 0 -> inf kept) in mv[..., 2], H x W = 21 x 27 padded to 24 x 32; one launch per sequence and one per
    centre.  Exact: torch.equal and the same bit patterns."""
    from cdfo_amd import kernels as K
    H, W, Hp, Wp = 21, 27, 24, 32
    g = torch.Generator().manual_seed(100 + T)
    mv = torch.randint(-64, 64, (T, H, W, 3), generator=g)
    mv[..., 2] = torch.randint(-3, 4, (T, H, W), generator=g)            # about one pixel in seven divides by zero
    mv[:, ::5, ::3, 0] = 0                                                # and some of those are 0 / 0
    mv = mv.to(dtype)
    if dtype.is_floating_point:
        mv = mv + (torch.rand(mv.shape, generator=g, dtype=torch.float64) * (mv[..., 2:3] != 0)).to(dtype) * 0.37   # inexact quotients
        mv[0 if T == 1 else 1, 2, 3] = torch.tensor([float("inf"), float("nan"), 2.0], dtype=dtype)
        mv[T - 1, H - 1, W - 1] = torch.tensor([3e38, -1e-39, 1e-3], dtype=dtype)
    want = torch.stack([_host_flows(mv, i, T, Hp, Wp) for i in range(T)])
    # the inputs do what they are meant to: infinities survive (at T = 1 both end rules zero every slot), NaN never does
    assert (torch.isinf(want).any() if T > 1 else not want.any()) and not torch.isnan(want).any()
    dev = mv.cuda()
    got = K.seq_flows(dev, 0, T, Hp, Wp).cpu()
    assert got.shape == (T, 7, 2, Hp, Wp)
    assert torch.equal(got, want)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    for i in range(T):                                                    # any first centre, any count
        one = K.seq_flows(dev, i, 1, Hp, Wp).cpu()
        assert torch.equal(one.view(torch.int32), want[i:i + 1].view(torch.int32)), f"centre {i} of {T}"


def test_seq_flows_refuses_bad_arguments():
    from cdfo_amd import kernels as K
    from cdfo_amd._lib import CdfoError
    mv = torch.zeros((3, 8, 8, 3), device="cuda")
    for i0, k, Hp, Wp in ((2, 2, 8, 8), (0, 0, 8, 8), (0, 1, 4, 8), (0, 1, 8, 10)):
        with pytest.raises(CdfoError):
            K.seq_flows(mv, i0, k, Hp, Wp)
    with pytest.raises(ValueError):
        K.seq_flows(mv[..., :2], 0, 1, 8, 8)


@pytest.mark.parametrize("shape,dtype", [((24, 40), torch.float32), ((16, 24, 64), torch.float32), ((3, 5, 8), torch.int16)])
def test_gather_frames_equals_index_select(shape, dtype):
    """Frames of 1 and of 64 channels (and a 240-byte one); repeated indices, the clipped windows of both ends of a sequence."""
    from cdfo_amd import kernels as K
    from cdfo_amd.streaming import NFRAMES, generate_input_index
    n = 9
    g = torch.Generator().manual_seed(7)
    src = (torch.randn((n,) + shape, generator=g) * 100).to(dtype).cuda()
    idx = torch.cat([generate_input_index(i, NFRAMES, n - 1) for i in (0, 1, 4, n - 2, n - 1)] + [torch.tensor([3, 3, 3, 8, 0])])
    got = K.gather_frames(src, idx.to(torch.int32).cuda())
    assert torch.equal(got, src.index_select(0, idx.cuda()))
    out = torch.full((2,) + shape, 5, dtype=dtype, device="cuda")
    assert K.gather_frames(src, torch.tensor([8, 8], dtype=torch.int32, device="cuda"), out=out) is out
    assert torch.equal(out, src[[8, 8]])
    # an index outside the source reads nothing: a frame of zeros
    bad = K.gather_frames(src, torch.tensor([2, n, -1], dtype=torch.int32, device="cuda"))
    assert torch.equal(bad[0], src[2]) and not bad[1:].any()


@pytest.fixture(scope="module")
def oracle_case():
    """The oracle loop and `run()` on T = 11 frames of 16 x 24, once for the four chunk sizes."""
    from cdfo_amd.streaming import StreamingSR
    from oracle.cvsr_v8_ref import make_inputs
    from oracle.streaming_ref import stream_sequence
    T, H, W = 11, 16, 24
    sd, model = _model(21)
    seq = _sequence(T, H, W, 5)
    noise = [make_inputs(1, H, W, 300 + i)["gumbel_u"] for i in range(T)]
    lr, pms, rms, ufs, mvl0, mvl1 = seq
    ref = stream_sequence(sd, lr / 255.0, pms / 255.0, rms / 255.0, ufs / 255.0, mvl0, mvl1, noise)
    dnoise = [[u.cuda() for u in n] for n in noise]
    s = StreamingSR(model, *seq, gumbel_uniform=dnoise)
    per_frame = s.run()
    assert s.frames_extracted == 7 + (T - 1)
    return model, seq, dnoise, ref, per_frame


@pytest.mark.parametrize("chunk", [1, 4, 8, 16])
def test_run_chunked_matches_the_oracle_loop_and_run(chunk, oracle_case):
    """T = 11 frames of 16 x 24 with injected noise (the inputs of test_streaming_loop_matches_oracle_loop, longer): chunk 16 > T,
    chunks 4 and 8 end ragged, chunk 1 is the per-step schedule.  Every frame within 1e-3 of the oracle's restatement of the
    reference loop and within 2e-5 of `run()` (same kernels, another image count per launch); each frame extracted once."""
    from cdfo_amd.streaming import StreamingSR
    T, H, W = 11, 16, 24
    model, seq, dnoise, ref, per_frame = oracle_case
    s = StreamingSR(model, *seq, gumbel_uniform=dnoise)
    outs = s.run_chunked(chunk)
    assert len(outs) == T and s.fps > 0
    assert s.frames_extracted == T
    err = [(o.cpu() - r).abs().max().item() for o, r in zip(outs, ref)]
    dif = [(o - p).abs().max().item() for o, p in zip(outs, per_frame)]
    print(f"chunk {chunk}: vs oracle max {max(err):.2e}, vs run() max {max(dif):.2e}; per frame vs run(): {['%.1e' % d for d in dif]}")
    for i, o in enumerate(outs):
        assert tuple(o.shape) == (1, 1, 4 * H, 4 * W)
        assert err[i] <= TOL, f"frame {i}: max-abs {err[i]} against the oracle loop"
    for i in range(T):
        assert dif[i] <= SAME_KERNELS, f"frame {i}: max-abs {dif[i]} against run()"


def test_run_chunked_range_guard_repairs_an_overflowing_chunk():
    """Trunk activations x 2^16 (tests/test_gpu_range_and_noise.py::_scaled_state): every chunk leaves fp16's range.  The chunk
    forward must warn, come back finite and within the bound of what the bf16x3 mode computes, with the guard settled on return."""
    from arch.SIDECVSR_our import CVSR_V8
    from cdfo_amd.streaming import StreamingSR
    from oracle.cvsr_v8_ref import make_inputs, make_state_dict
    T, H, W = 5, 16, 24
    seq = _sequence(T, H, W, 6)
    noise = [[u.cuda() for u in make_inputs(1, H, W, 500 + i)["gumbel_u"]] for i in range(T)]
    sd = make_state_dict(3)

    def load(state):
        m = CVSR_V8()
        m.load_state_dict(state, strict=True)
        return m.cuda().eval()
    want = StreamingSR(load(sd), *seq, gumbel_uniform=noise).run_chunked(4)           # the same function, inside fp16's range
    m16 = load(_scaled_state(sd, 2.0 ** 16))
    m16.precision = "bf16x3"
    exact = StreamingSR(m16, *seq, gumbel_uniform=noise).run_chunked(4)
    m16.precision = "fp16x2"
    s = StreamingSR(m16, *seq, gumbel_uniform=noise)
    with pytest.warns(UserWarning, match="fp16 range"):
        got = s.run_chunked(4)
    assert m16.last_range is not None and m16.last_range["fallback"] and m16._probe is None      # settled on return
    assert s.frames_extracted == T                                                                 # recomputed from the same bank
    for i in range(T):
        assert torch.isfinite(got[i]).all()
        d_exact, d_want = (got[i] - exact[i]).abs().max().item(), (got[i] - want[i]).abs().max().item()
        print(f"frame {i}: repaired vs bf16x3 {d_exact:.2e}, vs the unscaled model {d_want:.2e}")
        assert d_exact <= TOL and d_want <= TOL
    m16.range_guard = False                       # unguarded, the same chunk is visibly wrong: the guard is what repaired it
    raw = StreamingSR(m16, *seq, gumbel_uniform=noise).run_chunked(4)
    assert not ((raw[0] - want[0]).abs().max().item() <= 1e-5)


def test_run_chunked_default_noise_is_seeded_and_fresh():
    """Noise drawn in the mask kernel: the same generator state gives the same frames, another state other masks."""
    from cdfo_amd.streaming import StreamingSR
    T, H, W = 6, 16, 24
    _, model = _model(22)
    seq = _sequence(T, H, W, 9)

    def run(seed):
        torch.manual_seed(seed)
        return StreamingSR(model, *seq).run_chunked(4)
    a, b, c = run(1234), run(1234), run(4321)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
    assert max((x - y).abs().max().item() for x, y in zip(a, c)) < 1e-2
