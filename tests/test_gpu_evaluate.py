"""Sequence evaluation end to end on the GPU (cdfo_amd/evaluate.py): a synthetic sequence of T = 11 frames of 21x27 in the reference's
directory layout, seeded weights, chunk 4 (three chunks: more than the evaluator's two staging buffers).  The written PNGs against
the numpy quantisation of what run_chunked returns, the metrics against oracle/metrics_ref.py on the PNGs read back."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T, H, W = 11, 21, 27
SEED = 1234
SSIM_TOL = 1e-9       # the bound of tests/test_metrics.py for the device SSIM against the oracle


def _write_sequence(root, T, H, W, seed):
    """The reference's layout (test_LD_22_FPS.py:143-170): LR frames under any sortable names, side information from 00001 on."""
    from cdfo_amd.priors import write_gray_png
    rs = np.random.RandomState(seed)
    lr_dir, side = os.path.join(root, "lr"), os.path.join(root, "side")
    for d in ("part_m", "res", "unfiltered", "mvl0", "mvl1"):
        os.makedirs(os.path.join(side, d))
    os.makedirs(lr_dir)
    names = []
    for t in range(T):
        names.append("frame_%03d.png" % (t + 1))
        write_gray_png(os.path.join(lr_dir, names[-1]), rs.randint(0, 256, (H, W)).astype(np.uint8), t % 5)
        if t >= 1 or T == 1:
            i = "%05d" % max(1, t)
            write_gray_png(os.path.join(side, "part_m", i + "_M_mask.png"), rs.randint(0, 256, (H, W)).astype(np.uint8))
            write_gray_png(os.path.join(side, "unfiltered", i + "_unflt.png"), rs.randint(0, 256, (H, W)).astype(np.uint8))
            np.save(os.path.join(side, "res", i + "_res.npy"), np.clip(np.round(rs.randn(H, W, 3) * 6), -128, 127).astype(np.int8))
            for name in ("mvl0", "mvl1"):
                mv = rs.randint(-64, 64, ((H + 7) // 8, (W + 7) // 8, 3)).astype(np.int16)
                mv[..., 2] = rs.choice([-2, -1, 1], size=mv.shape[:2])
                np.save(os.path.join(side, name, i + "_" + name + ".npy"), np.repeat(np.repeat(mv, 8, axis=0), 8, axis=1)[:H, :W])
    return lr_dir, side, names


def _write_gt(root, T, h, w, seed):
    from cdfo_amd.priors import write_gray_png
    os.makedirs(root)
    gt = np.random.RandomState(seed).randint(0, 256, (T, h, w)).astype(np.uint8)
    for t in range(T):
        write_gray_png(os.path.join(root, "%05d.png" % t), gt[t], t % 5)
    return gt


def _quantise(x):
    v = np.clip(x.astype(np.float32), np.float32(0), np.float32(1)) * np.float32(255.0)
    return v.astype(np.uint8)


def _chunked_frames(model, lr_dir, side, chunk, share=False):
    """The 8-bit frames of run_chunked(chunk) under the test's seed: numpy quantisation of what it returns."""
    from cdfo_amd.priors import load_sequence
    from cdfo_amd.streaming import StreamingSR
    seq = load_sequence(lr_dir, side)
    torch.manual_seed(SEED)
    s = StreamingSR(model, seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"])
    outs = s.run_chunked(chunk, share_compensation=share)
    assert all(tuple(o.shape) == (1, 1, 4 * H, 4 * W) for o in outs)
    return np.stack([_quantise(o[0, 0].cpu().numpy()) for o in outs])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Model, sequence on disk, ground truth of three sizes, and the reference frames of chunk 4: made once, never changed."""
    from arch.SIDECVSR_our import CVSR_V8
    from oracle.cvsr_v8_ref import make_state_dict
    root = str(tmp_path_factory.mktemp("seq"))
    m = CVSR_V8()
    m.load_state_dict(make_state_dict(21, perturb=True), strict=True)
    model = m.cuda().eval()
    lr_dir, side, names = _write_sequence(root, T, H, W, 5)
    gts = {(h, w): (os.path.join(root, "gt_%dx%d" % (h, w)), _write_gt(os.path.join(root, "gt_%dx%d" % (h, w)), T, h, w, h + w))
           for (h, w) in ((84, 108), (86, 108), (84, 104))}
    return dict(model=model, lr=lr_dir, side=side, names=names, gts=gts, root=root, frames4=_chunked_frames(model, lr_dir, side, 4))


def _evaluate(case, **kw):
    from cdfo_amd.evaluate import evaluate_sequence
    torch.manual_seed(SEED)
    return evaluate_sequence(case["model"], case["lr"], case["side"], **kw)


def _read_all(case, save):
    from cdfo_amd.priors import read_gray_png
    assert sorted(os.listdir(save)) == case["names"]                            # the LR file names (test_LD_37.py:180)
    return np.stack([read_gray_png(os.path.join(save, n)) for n in case["names"]])


def _check_metrics(result, frames, gt, crop=4):
    from oracle.metrics_ref import calculate_psnr, calculate_ssim
    hm, wm = min(frames.shape[1], gt.shape[1]), min(frames.shape[2], gt.shape[2])
    assert result.psnr.dtype == np.float64 and result.psnr.shape == (len(frames),) and result.ssim.shape == (len(frames),)
    for t in range(len(frames)):
        a, b = frames[t, :hm, :wm], gt[t, :hm, :wm]
        want_p, want_s = calculate_psnr(a, b, crop), calculate_ssim(a, b, crop)
        print(f"frame {t}: PSNR {result.psnr[t]!r} (oracle {want_p!r}), SSIM {result.ssim[t]!r}, error {abs(result.ssim[t] - want_s):.2e}")
        assert result.psnr[t] == want_p
        assert abs(result.ssim[t] - want_s) < SSIM_TOL
    assert abs(result.mean_psnr - result.psnr.mean()) < 1e-12 and abs(result.mean_ssim - result.ssim.mean()) < 1e-15


@pytest.mark.parametrize("gt_size", [(84, 108), (86, 108), (84, 104)])
def test_pngs_and_metrics(case, gt_size, tmp_path):
    """Ground truth of the output's size, 2 rows taller, 4 columns narrower (the min rule)."""
    from cdfo_amd.evaluate import format_log
    gt_dir, gt = case["gts"][gt_size]
    save = str(tmp_path / "out")
    before = torch.cuda.memory_allocated()
    r = _evaluate(case, gt_dir=gt_dir, save_dir=save, chunk=4, workers=3)
    held = torch.cuda.memory_allocated() - before
    frames = _read_all(case, save)
    assert np.array_equal(frames, case["frames4"])                              # bit for bit what run_chunked(4) gives, quantised
    _check_metrics(r, frames, gt)
    assert r.frames == T and 0 < r.seconds_forward < r.seconds_total
    line = format_log(r, "seq")
    assert line == "seq Average PSNR/SSIM: %.3f/%.5f" % (r.mean_psnr, r.mean_ssim)
    assert re.fullmatch(r"seq Average PSNR/SSIM: \d+\.\d{3}/-?\d\.\d{5}", line), line
    # a condition, not a measurement: the evaluator keeps no per-frame fp32 output (two chunk outputs of 4 padded frames each)
    assert held < 2 * 4 * (4 * 24) * (4 * 32) * 4, held


@pytest.mark.parametrize("chunk", [1, 16])
def test_other_chunk_sizes_follow_run_chunked(case, chunk, tmp_path):
    """Chunk 1 (eleven chunks, every staging buffer reused five times) and chunk 16 > T (one ragged chunk): the PNGs are the
    quantised frames of run_chunked at that chunk size, the metrics the oracle's on them."""
    gt_dir, gt = case["gts"][(86, 108)]
    save = str(tmp_path / "out")
    r = _evaluate(case, gt_dir=gt_dir, save_dir=save, chunk=chunk)
    frames = _read_all(case, save)
    assert np.array_equal(frames, _chunked_frames(case["model"], case["lr"], case["side"], chunk))
    _check_metrics(r, frames, gt)


def _step_noise(seed):
    """Injected noise in the per-step format: for every centre frame the six uniform draws of its window's neighbour slots."""
    from oracle.cvsr_v8_ref import make_inputs
    return [[u.cuda() for u in make_inputs(1, 24, 32, seed + t)["gumbel_u"]] for t in range(T)]


@pytest.mark.parametrize("share", [False, True])
def test_results_at_chunk_1_4_16_are_identical(case, share, tmp_path):
    """Frames and metrics at chunk 1, 4 and 16 under one source of noise.  The shared mode draws per frame, whichever chunk holds
    it, so one seed is enough.  The default mode draws per forward call, so WITHOUT injected noise its frames depend on the chunk
    size (test_other_chunk_sizes_follow_run_chunked pins those to run_chunked at the same size); here it gets per-step noise
    through evaluate_sequence(gumbel_uniform=), which belongs to the (step, slot) and not to the chunk."""
    gt_dir, gt = case["gts"][(84, 108)]
    kw = dict(share_compensation=True) if share else dict(gumbel_uniform=_step_noise(900))
    res = {}
    for chunk in (1, 4, 16):
        save = str(tmp_path / ("out%d" % chunk))
        r = _evaluate(case, gt_dir=gt_dir, save_dir=save, chunk=chunk, **kw)
        res[chunk] = (r, _read_all(case, save))
    for chunk in (1, 16):
        d = res[chunk][1].astype(int) - res[4][1].astype(int)
        print(f"chunk {chunk} vs chunk 4: {np.count_nonzero(d)} of {d.size} pixels differ, max {np.abs(d).max()} levels; "
              f"PSNR max |difference| {np.abs(res[chunk][0].psnr - res[4][0].psnr).max():.3e}, SSIM "
              f"{np.abs(res[chunk][0].ssim - res[4][0].ssim).max():.3e}")
    for chunk in (1, 16):
        assert np.array_equal(res[chunk][1], res[4][1])
        assert np.array_equal(res[chunk][0].psnr, res[4][0].psnr) and np.array_equal(res[chunk][0].ssim, res[4][0].ssim)
    _check_metrics(res[4][0], res[4][1], gt)


def test_no_fp32_frame_outlives_its_chunk(case, tmp_path):
    """Peak device memory DURING the call (the difference after it has returned is about 0 whatever it held meanwhile), against the
    peak of the same chunk loop with every output dropped at once.  What the evaluator owns on the device beyond that loop: two
    8-bit frame buffers [4,84,108], two 8-bit ground-truth buffers [4,86,108], and while a chunk is finished the partial sums of
    its two kernels ([4,1024] of 8 bytes each); 64 KiB more is allowed for the per-chunk result tensors and the allocator's
    rounding.  One fp32 chunk output kept alive ([4,1,96,128], 192 KiB) goes past that."""
    from cdfo_amd.priors import load_sequence
    from cdfo_amd.streaming import StreamingSR
    gt_dir, gt = case["gts"][(86, 108)]

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    def bare_loop():
        seq = load_sequence(case["lr"], case["side"])
        torch.manual_seed(SEED)
        s = StreamingSR(case["model"], seq["lr"], seq["pms"], seq["rms"], seq["ufs"], seq["mvl0"], seq["mvl1"])
        chunks = s.iter_chunked(4)
        for _ in range(3):
            next(chunks)                                                          # the output is dropped before the next forward

    base = peak(bare_loop)
    full = peak(lambda: _evaluate(case, gt_dir=gt_dir, save_dir=str(tmp_path / "out"), chunk=4))
    own = 2 * 4 * 84 * 108 + 2 * 4 * 86 * 108 + 2 * 4 * 1024 * 8 + 64 * 1024
    print(f"peak of the bare chunk loop {base} bytes, of evaluate_sequence {full} bytes: {full - base} more, {own} allowed; one fp32 "
          f"chunk output is {4 * 96 * 128 * 4} bytes")
    assert full - base < own


def test_shared_compensation_runs_and_writes_every_frame(case, tmp_path):
    """share_compensation=True with the in-kernel Philox noise (no frame_noise): T files, the frames of run_chunked in that mode."""
    gt_dir, gt = case["gts"][(84, 104)]
    save = str(tmp_path / "out")
    r = _evaluate(case, gt_dir=gt_dir, save_dir=save, chunk=4, share_compensation=True)
    frames = _read_all(case, save)
    assert len(frames) == T and r.frames == T
    assert np.array_equal(frames, _chunked_frames(case["model"], case["lr"], case["side"], 4, share=True))
    _check_metrics(r, frames, gt)


def test_without_ground_truth_and_without_saving(case, tmp_path):
    gt_dir, gt = case["gts"][(84, 108)]
    save = str(tmp_path / "out")
    r = _evaluate(case, save_dir=save, chunk=4)                                  # frames, no metrics
    assert r.psnr.shape == (0,) and r.ssim.shape == (0,) and np.isnan(r.mean_psnr) and np.isnan(r.mean_ssim) and r.frames == T
    assert np.array_equal(_read_all(case, save), case["frames4"])
    listing = sorted(os.listdir(case["root"]))
    r = _evaluate(case, gt_dir=gt_dir, chunk=4)                                  # metrics, nothing written
    assert sorted(os.listdir(case["root"])) == listing and sorted(os.listdir(str(tmp_path))) == ["out"]
    _check_metrics(r, case["frames4"], gt)
    r8 = _evaluate(case, gt_dir=gt_dir, chunk=4, quantise="nearest")             # the other quantiser changes the metrics
    assert not np.array_equal(r8.psnr, r.psnr)


def test_single_frame_sequence(case, tmp_path):
    lr_dir, side, names = _write_sequence(str(tmp_path / "one"), 1, H, W, 8)
    gt = _write_gt(str(tmp_path / "gt"), 1, 84, 108, 3)
    from cdfo_amd.evaluate import evaluate_sequence
    from cdfo_amd.priors import read_gray_png
    torch.manual_seed(SEED)
    r = evaluate_sequence(case["model"], lr_dir, side, gt_dir=str(tmp_path / "gt"), save_dir=str(tmp_path / "out"), chunk=4)
    assert r.frames == 1 and os.listdir(str(tmp_path / "out")) == names
    frame = read_gray_png(os.path.join(str(tmp_path / "out"), names[0]))[None]
    assert np.array_equal(frame, _chunked_frames(case["model"], lr_dir, side, 4))
    _check_metrics(r, frame, gt)
