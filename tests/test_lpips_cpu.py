"""LPIPS without a device: the torch statement of the definition (tests/lpips_ref.py) against what the definition must yield and
against a second, numpy-only statement written from DESIGN.md's text (explicit padded arrays, no torch.nn.functional); the model
reader's round trips and refusals; every refusal of the option; and the fp32 floor the device tests take their bounds from.

Neither the ``lpips`` package nor torchvision nor any published weights are available, so nothing here pins parity with them."""
import numpy as np
import pytest
import torch

import lpips_cases as cases
import lpips_ref as ref


# ---- the second statement: numpy alone ----
def np_conv_relu(x, w, b):
    """x [Cin,h,w], w [Cout,Cin,3,3], b [Cout] -> ReLU of the 3 x 3 convolution with a zero border, tap by tap."""
    cin, h, wd = x.shape
    pad = np.zeros((cin, h + 2, wd + 2))
    pad[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], h, wd)) + b[:, None, None]
    for ky in range(3):
        for kx in range(3):
            out += np.tensordot(w[:, :, ky, kx], pad[:, ky:ky + h, kx:kx + wd], axes=(1, 0))
    return np.maximum(out, 0.0)


def np_pool(x):
    c, h, w = x.shape
    x = x[:, :h // 2 * 2, :w // 2 * 2].reshape(c, h // 2, 2, w // 2, 2)
    return x.max(axis=(2, 4))


def np_layers(a, b, params, normalize=True):
    h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    taps = []
    for frame in (a[:h, :w], b[:h, :w]):
        v = frame.astype(np.float64) / 255.0
        if normalize:
            v = 2.0 * v - 1.0
        x = np.stack([(v - s) / q for s, q in zip((-.030, -.088, -.188), (.458, .448, .450))])
        i, mine = 0, []
        for k, convs in enumerate((2, 2, 3, 3, 3)):
            if k:
                x = np_pool(x)
            for _ in range(convs):
                x = np_conv_relu(x, params.weights[i].astype(np.float64), params.biases[i].astype(np.float64))
                i += 1
            mine.append(x)
        taps.append(mine)
    d = []
    for k in range(5):
        A, B = taps[0][k], taps[1][k]
        nA = A / (np.sqrt((A * A).sum(axis=0)) + 1e-10)
        nB = B / (np.sqrt((B * B).sum(axis=0)) + 1e-10)
        d.append(((params.lins[k][:, None, None] * (nA - nB) ** 2).sum(axis=0)).mean())
    return np.array(d)


@pytest.mark.parametrize("name", ["narrow-16x16", "narrow-37x53"])
def test_two_statements_agree(name):
    params, sr, gt, want, _ = cases.case(name)
    worst = 0.0
    for j in range(len(sr)):
        got = np_layers(sr[j], gt[j], params)
        worst = max(worst, cases.rel(got, want[j]), abs(ref.total(got) - ref.total(want[j])) / ref.total(want[j]))
    print(f"{name}: numpy statement against the torch statement, worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    off = np_layers(sr[0], gt[0], params, normalize=False)
    assert cases.rel(off, ref.layers(sr[0], gt[0], params, normalize=False)) <= 1e-12 and cases.rel(off, want[0]) > 1e-3


def test_equal_frames_give_exactly_zero_and_the_distance_is_symmetric():
    params, sr, gt, want, _ = cases.case("narrow-37x53")
    assert np.array_equal(ref.layers(gt[0], gt[0].copy(), params), np.zeros(5)) and ref.lpips(sr[1], sr[1], params) == 0.0
    back = ref.layers(gt[0], sr[0], params)
    assert np.array_equal(back, want[0]) and ref.lpips(gt[0], sr[0], params) == ref.lpips(sr[0], gt[0], params)
    assert np.all(want > 0.0) and np.all(np.isfinite(want))
    # the region is the common top-left rectangle
    assert np.array_equal(ref.layers(np.pad(sr[0], ((0, 3), (0, 5))), gt[0], params), want[0])
    # an all-zero feature vector normalises to zero, not to NaN
    z = torch.zeros(4, 2, 2)
    assert ref.layer_distance(z, z, np.ones(4)) == 0.0
    o = torch.ones(4, 2, 2)
    assert abs(ref.layer_distance(z, o, np.ones(4)) - 1.0) < 1e-9


def test_sizes_and_scratch_bytes():
    from cdfo_amd import metrics as M
    assert M.lpips_size(16, 16) == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert M.lpips_size(37, 53) == [(37, 53), (18, 26), (9, 13), (4, 6), (2, 3)]
    assert M.lpips_size(1080, 1920)[-1] == (67, 120)
    for h, w in ((15, 16), (16, 15), (12, 40)):
        with pytest.raises(ValueError, match="16 x 16"):
            M.lpips_size(h, w)
    # two fp32 buffers of one pair's largest activation (stage 1: 2 x 1080 x 1920 x 64) and the strips of eight frames
    strips = 540 + 270 + 135 + 68 + 34
    assert M.LpipsScratch.bytes_for(1, 1080, 1920) == 2 * 4 * 2 * 1080 * 1920 * 64 + 8 * 8 * strips == 2123366400 + 8 * 8 * strips
    assert M.LpipsScratch.bytes_for(2, 37, 53, cases.NARROW, 3) == 2 * 4 * 4 * 37 * 53 * 16 + 8 * 3 * (19 + 9 + 5 + 2 + 1)
    assert np.array_equal(M.lpips_from_layers(np.array([[1.0, 2.0, 3.0, 4.0, 5.0]])), [15.0])
    with pytest.raises(ValueError):
        M.lpips_from_layers(np.zeros((2, 4)))


def test_params_round_trip(tmp_path):
    from cdfo_amd import metrics as M
    p = cases.model(cases.NARROW, 11)
    assert p.widths == cases.NARROW and len(p.weights) == 13 and p.weights[0].shape == (16, 3, 3, 3) and p.lins[2].shape == (48,)
    assert all(w.dtype == np.float32 for w in p.weights + p.biases) and all(l.dtype == np.float64 for l in p.lins)
    assert M.lpips_params(p) is p

    def same(q):
        return all(np.array_equal(x, y) for x, y in zip(p.weights + p.biases + p.lins, q.weights + q.biases + q.lins))

    assert same(M.lpips_params(p.arrays()))
    np.savez(tmp_path / "model.npz", **p.arrays())
    assert same(M.lpips_params(str(tmp_path / "model.npz"))) and same(M.lpips_params(tmp_path / "model.npz"))
    trunk = {}
    for i, key in enumerate(M.LPIPS_TRUNK_KEYS):
        trunk[f"features.{key}.weight"], trunk[f"features.{key}.bias"] = torch.from_numpy(p.weights[i].copy()), torch.from_numpy(p.biases[i].copy())
    trunk["classifier.0.weight"] = torch.zeros(3, 3)                                   # a whole VGG16 checkpoint has more than the trunk
    head = {f"lin{k}.model.1.weight": torch.from_numpy(p.lins[k].astype(np.float32)).reshape(1, -1, 1, 1) for k in range(5)}
    assert same(M.lpips_params((trunk, head)))
    torch.save(trunk, tmp_path / "trunk.pth")
    torch.save(head, tmp_path / "head.pth")
    assert same(M.lpips_params((str(tmp_path / "trunk.pth"), str(tmp_path / "head.pth"))))


def test_params_refusals():
    from cdfo_amd import metrics as M
    good = cases.model(cases.NARROW, 11).arrays()

    def broken(**change):
        d = dict(good)
        d.update(change)
        return d

    rs = np.random.RandomState(0)
    wrong_topology = broken(w3=rs.standard_normal((32, 16, 3, 3)).astype(np.float32))          # stage 2's second conv must read 32
    bad = [
        wrong_topology,
        broken(w0=good["w0"][:, :1]),                                                           # one input channel
        broken(w4=good["w4"][:, :, :1, :1]),                                                    # a 1 x 1 convolution
        {k: v for k, v in good.items() if k != "b7"},                                           # a bias missing
        {"w0": good["w0"]},
        broken(lin1=good["lin1"][:-1]),                                                         # a lin of the wrong length
        broken(lin4=np.stack([good["lin4"], good["lin4"]])),
        broken(b5=np.where(np.arange(48) == 7, np.nan, good["b5"]).astype(np.float32)),         # a NaN
        broken(w12=np.where(np.arange(64)[:, None, None, None] == 3, np.inf, good["w12"]).astype(np.float32)),
        (good, good, good),                                                                     # neither a mapping nor a pair
        ({}, {}),
    ]
    for k, source in enumerate(bad):
        with pytest.raises(ValueError):
            M.lpips_params(source)
            pytest.fail(f"source {k} was accepted")
    # a width of 24: a well-formed net whose first stage is no multiple of 16
    with pytest.raises(ValueError, match="multiples of 16"):
        narrow = {}
        cin, i = 3, 0
        for k, convs in enumerate(M.LPIPS_STAGES):
            width = (24, 32, 48, 64, 64)[k]
            for _ in range(convs):
                narrow[f"w{i}"], narrow[f"b{i}"] = np.zeros((width, cin, 3, 3), np.float32), np.zeros(width, np.float32)
                cin, i = width, i + 1
            narrow[f"lin{k}"] = np.zeros(width)
        M.lpips_params(narrow)
    with pytest.raises(ValueError):
        M.lpips_random_params((16, 32, 48, 64))
    with pytest.raises(ValueError, match="multiples of 16"):
        M.lpips_random_params((16, 32, 40, 64, 64))


def test_result_fields_and_log_lines():
    from cdfo_amd import evaluate as E
    r = E.SequenceResult(np.array([30.0]), np.array([0.9]), 30.0, 0.9, 1, 0.5, 1.0)
    assert len(r.lpips) == 0 and np.isnan(r.mean_lpips) and E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000"
    r = r._replace(lpips=np.array([0.25]), mean_lpips=0.25)
    assert E.format_log(r, "s") == "s Average PSNR/SSIM: 30.000/0.90000 LPIPS: 0.25000"
    r = r._replace(tof=np.array([0.125]), mean_tof=0.125)
    assert E.format_log(r, "s").endswith(" tOF: 0.12500 LPIPS: 0.25000")
    z = np.zeros(2)
    y = E.YuvResult(z, z, z, z, z, 31.0, 40.0, 41.0, 0.8, 33.375, 2, 0.5, 1.0)
    assert "LPIPS" not in E.format_log_yuv(y, "s") and len(y.lpips) == 0 and np.isnan(y.mean_lpips)
    assert E.format_log_yuv(y._replace(tof=z, mean_tof=0.5, lpips=z, mean_lpips=0.75), "s").endswith(" tOF: 0.50000 LPIPS: 0.75000")


def test_every_refusal_needs_no_device(tmp_path):
    from cdfo_amd import evaluate as E
    from cdfo_amd import kernels as K
    from cdfo_amd import metrics as M
    params = cases.model(cases.NARROW, 11)

    class Lr:
        dtype, peak, shape = torch.uint8, 255, (16, 20)

    class Lr10:
        dtype, peak, shape = torch.uint16, 1023, (16, 20)

    class Gt:
        shape = (64, 80)

    class GtSmall:
        shape = (12, 40)

    assert E._check_lpips(Lr, None, None) is None and E._check_lpips(Lr, Gt, params) is params
    assert E._check_lpips(Lr, Gt, params.arrays()).widths == cases.NARROW
    with pytest.raises(ValueError, match="ground truth"):
        E._check_lpips(Lr, None, params)
    with pytest.raises(ValueError, match="8-bit"):
        E._check_lpips(Lr10, Gt, params)
    with pytest.raises(ValueError, match="16 x 16"):
        E._check_lpips(Lr, GtSmall, params)
    with pytest.raises(ValueError, match="LPIPS model"):
        E._check_lpips(Lr, Gt, {"w0": np.zeros(3)})
    # through the evaluators themselves: refused before the model is touched (None stands in for it)
    lr_dir, side, gt_dir = E.write_synthetic_sequence(str(tmp_path / "seq"), 2, 16, 20, seed=3)
    with pytest.raises(ValueError, match="ground truth"):
        E.evaluate_sequence(None, lr_dir, side, lpips=params)
    lr_small, side_small, gt_small = E.write_synthetic_sequence(str(tmp_path / "small"), 2, 3, 10, seed=3)     # a 12 x 40 region
    with pytest.raises(ValueError, match="16 x 16"):
        E.evaluate_sequence(None, lr_small, side_small, gt_dir=gt_small, crop_border=0, lpips=params)
    lr_yuv, side_yuv, gt_yuv = E.write_synthetic_sequence_yuv(str(tmp_path / "ten"), 2, 16, 20, seed=3, pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="8-bit"):                                                               # peak 1023
        E.evaluate_yuv(None, lr_yuv, 20, 16, side_yuv, gt_yuv=gt_yuv, pix_fmt="yuv420p10le", lpips=params)
    lr_yuv, side_yuv, _ = E.write_synthetic_sequence_yuv(str(tmp_path / "free"), 2, 16, 20, seed=3, gt=False)
    with pytest.raises(ValueError, match="ground truth"):
        E.evaluate_yuv(None, lr_yuv, 20, 16, side_yuv, lpips=params)
    # the host functions and the wrappers
    u = torch.zeros((2, 16, 16), dtype=torch.uint8)
    x, lin, part = torch.zeros((2, 4, 4, 16)), torch.zeros(16, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    w0, b0 = torch.zeros((16, 3, 3, 3)), torch.zeros(16)
    bad = [lambda: M.lpips_scratch(2, 15, 40, params, "cpu"), lambda: M.lpips_scratch(0, 16, 16, params, "cpu"),
           lambda: M.lpips_scratch(2, 16, 16, (16, 32, 48, 60, 64), "cpu"), lambda: M.lpips_scratch(2, 16, 16, params, "cpu", pairs=0),
           lambda: M.lpips_layers_u8(u, u, params), lambda: M.lpips_u8(u, u, params),
           lambda: K.lpips_stem(u, w0, b0), lambda: K.lpips_pool2(x), lambda: K.lpips_dist(x, x, lin),
           lambda: K.lpips_fold(part, 2, [4], [16])]
    for k, call in enumerate(bad):
        with pytest.raises((ValueError, NotImplementedError)):
            call()
            pytest.fail(f"call {k} did not raise")


def test_fp32_floor_of_the_device_tests_cases():
    """The statement with an fp32 trunk against the fp64 one on the device tests' own cases: the floor their bounds are 16 x of.  An
    fp32 trunk of 13 convolutions of up to 4608 terms each cannot be expected below ~1e-7 nor, rounding errors adding up like a
    random walk (sqrt(4608) * 2^-24 = 4e-6 per convolution), above ~5e-5."""
    for name in cases.CASES:
        _, _, _, want, f32 = cases.case(name)
        print(f"{name}: fp32-trunk statement against fp64: per layer {cases.rel(f32, want):.2e}, total "
              f"{cases.rel(cases.totals(f32), cases.totals(want)):.2e}; LPIPS {cases.totals(want).min():.4f} .. {cases.totals(want).max():.4f}")
        _, _, stem64, stem_floor = cases.stem_case(name)
        print(f"{name}: fp32 stem against fp64: {stem_floor:.2e} of the largest value {np.abs(stem64).max():.3f}")
        assert 0.0 < stem_floor <= 1e-6
    per_layer, total = cases.floors()
    print(f"worst fp32 floor: per layer {per_layer:.2e}, total {total:.2e}")
    assert 0.0 < total <= 5e-5 and 1e-8 <= per_layer <= 5e-5
