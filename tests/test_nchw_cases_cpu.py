"""Do the cases of the NCHW operator tests bite?  (No GPU.)

tests/test_gpu_nchw_ops.py compares the kernels of csrc/nchw_ops.hip and csrc/nchw_bwd.hip with the float64 references of
nchw_cases.py on the inputs of nchw_cases.py, within fold_cases.bound.  Here every kernel is restated in numpy fp32 as a MODEL
that follows the kernel's own structure (gathers, candidate ranges, 64-lane sums, tiles and slabs) and can be given one of the
mistakes such a kernel makes.  Asserted: the defect-free model lands inside the bound of EVERY case, and every defect lands
outside the bound of AT LEAST ONE case (a result of another shape, or one with elements left unwritten = NaN, is outside).
The models are independent of the references: the references are F.conv2d / F.max_pool2d / dense weight matrices / autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nchw_cases as NC

f32 = np.float32
F64, F32 = torch.float64, torch.float32


def _np(t):
    return None if t is None else t.numpy()


def _sigmoid(v):
    return (f32(1.0) / (f32(1.0) + np.exp(-v))).astype(f32)


def margin(got, ref, restated):
    """error / bound of a model result against the reference; inf for another shape or an unwritten (NaN) element"""
    got = (got if torch.is_tensor(got) else torch.from_numpy(np.array(got))).double()
    if got.shape != ref.shape:
        return float("inf")
    err = (got - ref).abs().max().item()
    return float("inf") if err != err else err / NC.bound(ref, restated)


# ------------------------------------------------------------------------------------------------------------ conv2d
CONV_DEFECTS = ("pad_off_by_one", "bias_grad_dropped", "stride_phase_ignored")


def conv_model(c, defect=None):
    """conv2d_nchw_kernel before its activation: out = bias + sum over (c, ky, kx) of in[oy s - pad + ky][ox s - pad + kx] w"""
    x, w, b, _ = (_np(t) for t in NC.conv_inputs(c))
    Ho, Wo = NC.conv_out_hw(c)
    sh = 1 if defect == "pad_off_by_one" else 0                    # iy = oy s - pad + ky + 1
    xp = np.pad(x, ((0, 0), (0, 0), (c.pad, c.pad + sh), (c.pad, c.pad + sh)))
    out = np.zeros((c.B, c.Co, Ho, Wo), f32)
    if b is not None:
        out += b[None, :, None, None]
    for ky in range(c.k):
        for kx in range(c.k):
            win = xp[:, :, ky + sh:ky + sh + (Ho - 1) * c.stride + 1:c.stride, kx + sh:kx + sh + (Wo - 1) * c.stride + 1:c.stride]
            out += np.einsum("bchw,oc->bohw", win, w[:, :, ky, kx])
    return out


def conv_bwd_model(c, defect=None):
    """the three gathers of nchw_bwd.hip: (gin, gw, gbias)"""
    x, w, _, g = (_np(t) for t in NC.conv_inputs(c))
    Ho, Wo = NC.conv_out_hw(c)
    s, pad = c.stride, c.pad
    gin = np.zeros_like(x)
    for iy in range(c.H):
        for ky in range(c.k):
            ty = iy + pad - ky
            if ty < 0 or (ty % s and defect != "stride_phase_ignored") or ty // s >= Ho:
                continue
            for ix in range(c.W):
                for kx in range(c.k):
                    tx = ix + pad - kx
                    if tx < 0 or (tx % s and defect != "stride_phase_ignored") or tx // s >= Wo:
                        continue
                    gin[:, :, iy, ix] += g[:, :, ty // s, tx // s] @ w[:, :, ky, kx]
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    gw = np.zeros_like(w)
    for ky in range(c.k):
        for kx in range(c.k):
            win = xp[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
            gw[:, :, ky, kx] = np.einsum("bohw,bchw->oc", g, win)
    gb = np.zeros(c.Co, f32) if defect == "bias_grad_dropped" else g.sum((0, 2, 3), dtype=f32)
    return gin, gw, gb


def _conv_margins(c, defect=None):
    pre = conv_model(c, defect)
    m = [margin(pre, NC.conv_ref(c), NC.conv_ref(c, dtype=F32)), margin(np.maximum(pre, 0), NC.conv_ref(c, "relu"), NC.conv_ref(c, "relu", F32)),
         margin(_sigmoid(pre), NC.conv_ref(c, "sigmoid"), NC.conv_ref(c, "sigmoid", F32))]
    ref, ref32 = NC.conv_grad_ref(c), NC.conv_grad_ref(c, dtype=F32)
    return m + [margin(got, r, r32) for got, r, r32 in zip(conv_bwd_model(c, defect), ref, ref32)]


@pytest.mark.parametrize("c", NC.CONV_CASES, ids=NC.case_id)
def test_conv_model_passes_every_case(c):
    m = _conv_margins(c)
    print(NC.case_id(c), ["%.3f" % v for v in m])
    assert max(m) <= 1.0, m
    assert NC.conv_ref(c).abs().max().item() < 8.0          # the sigmoid's argument


@pytest.mark.parametrize("defect", CONV_DEFECTS)
def test_a_defective_conv_is_caught(defect):
    m = {NC.case_id(c): max(_conv_margins(c, defect)) for c in NC.CONV_CASES}
    print(defect, {k: "%.3g" % v for k, v in m.items()})
    assert max(m.values()) > 1.0, m
    if defect == "stride_phase_ignored":       # only a stride above 1 has a phase
        assert all((v > 1.0) == (c.stride > 1 and c.k > 1) for c, v in zip(NC.CONV_CASES, m.values())), m


def test_conv_cases_have_the_shapes_they_are_named_for():
    c = next(c for c in NC.CONV_CASES if c.name == "unused_edge")
    Ho, Wo = NC.conv_out_hw(c)
    assert (Ho - 1) * c.stride + c.k - c.pad == c.H - 1 and (Wo - 1) * c.stride + c.k - c.pad == c.W - 1
    gin = NC.conv_grad_ref(c)[0]
    assert (gin[:, :, -1] == 0).all() and (gin[..., -1] == 0).all()
    c = next(c for c in NC.CONV_CASES if c.name == "below_kernel")
    assert c.H < c.k and c.W < c.k
    g = NC.CONV_GRID_CASE
    assert g.C == 1 and g.k == 1 and g.B * g.Co * g.H * g.W > NC.GRID_CAP
    assert {(c.k, c.stride, c.pad) for c in NC.CONV_CASES if c.name == "base"} == set(NC.GEOMETRIES)
    assert {c.bias for c in NC.CONV_CASES} == {False, True}


# ------------------------------------------------------------------------------------------------------------ max-pool
POOL_DEFECTS = ("last_maximum", "nan_dropped", "remainder_kept")


def pool_model(c, defect=None):
    """the scan of maxpool_nchw_kernel / maxpool_nchw_argmax_kernel and the routing of maxpool_nchw_bwd_kernel: (out, gin)"""
    x, g = (_np(t) for t in NC.pool_inputs(c))
    Ho, Wo = NC.pool_out_hw(c)
    if defect == "remainder_kept":             # a last, clipped window over the rows and columns the floor drops
        Ho, Wo = -(-(c.H - c.k) // c.stride) + 1, -(-(c.W - c.k) // c.stride) + 1
    out = np.zeros((c.B, c.C, Ho, Wo), f32)
    gin = np.zeros((c.B * c.C, c.H * c.W), f32)
    planes = np.arange(c.B * c.C)
    for oy in range(Ho):
        for ox in range(Wo):
            m = np.full((c.B, c.C), -np.inf, f32)
            am = np.full((c.B, c.C), oy * c.stride * c.W + ox * c.stride)
            for ky in range(c.k):
                for kx in range(c.k):
                    y, xx = oy * c.stride + ky, ox * c.stride + kx
                    if y >= c.H or xx >= c.W:
                        continue
                    v = x[:, :, y, xx]
                    with np.errstate(invalid="ignore"):
                        take = (v >= m) if defect == "last_maximum" else (v > m)
                    if defect != "nan_dropped":
                        take = take | np.isnan(v)
                    m = np.where(take, v, m)
                    am = np.where(take, y * c.W + xx, am)
            out[:, :, oy, ox] = m
            if oy < g.shape[2] and ox < g.shape[3]:
                np.add.at(gin, (planes, am.ravel()), g[:, :, oy, ox].ravel())
    return out, gin.reshape(x.shape)


@pytest.mark.parametrize("c", NC.POOL_CASES, ids=NC.case_id)
def test_pool_model_passes_every_case(c):
    out, gin = pool_model(c)
    ref, gref = NC.pool_ref(c)
    assert NC.same_with_nan(torch.from_numpy(out), ref) and torch.equal(torch.from_numpy(gin).double(), gref)


@pytest.mark.parametrize("defect", POOL_DEFECTS)
def test_a_defective_pool_is_caught(defect):
    caught = {}
    for c in NC.POOL_CASES:
        out, gin = pool_model(c, defect)
        ref, gref = NC.pool_ref(c)
        caught[NC.case_id(c)] = (not NC.same_with_nan(torch.from_numpy(out), ref), not torch.equal(torch.from_numpy(gin).double(), gref))
    print(defect, caught)
    fwd, bwd = any(f for f, _ in caught.values()), any(b for _, b in caught.values())
    # a tie moves the gradient and not the maximum; a dropped NaN changes the forward (and with it the tap)
    assert {"last_maximum": bwd and not fwd, "nan_dropped": fwd and bwd, "remainder_kept": fwd}[defect], caught
    if defect == "nan_dropped":
        assert all(f == (NC.POOL_CASES[i].data == "nan") for i, (f, _) in enumerate(caught.values())), caught


def test_pool_cases_have_the_data_they_are_named_for():
    geometries = {(c.H, c.W, c.k, c.stride) for c in NC.POOL_CASES}
    assert {(7, 7, 7, 3), (8, 9, 7, 3), (13, 16, 7, 3), (6, 6, 2, 2), (5, 5, 3, 1)} <= geometries
    for c in NC.POOL_CASES:
        x, g = NC.pool_inputs(c)
        Ho, Wo = NC.pool_out_hw(c)
        assert torch.equal(g, g.round()) and torch.equal(x.nan_to_num(nan=0.0, neginf=0.0), x.nan_to_num(nan=0.0, neginf=0.0).round())
        if c.data == "ties":                   # some window holds its maximum more than once
            win = x.unfold(2, c.k, c.stride).unfold(3, c.k, c.stride).reshape(c.B, c.C, Ho, Wo, -1)
            assert ((win == win.amax(-1, keepdim=True)).sum(-1) > 1).any()
        if c.data == "nan":
            assert [tuple(p.nonzero()[0].tolist()) for p in x[0].isnan()] == [(0, 0), (c.k - 1, c.k - 1), (c.k // 2, c.k // 2)]
        if c.data == "neginf":
            assert (x[0, 0] == float("-inf")).all() and NC.pool_ref(c)[0][0, 0].isinf().all()
        if (c.H, c.W) == (8, 9):               # rows and columns beyond the last window
            assert (Ho - 1) * c.stride + c.k < c.H and (Wo - 1) * c.stride + c.k < c.W


# ------------------------------------------------------------------------------------------------------------ bilinear resize
RESIZE_DEFECTS = ("float64_scale", "no_clamp_at_0", "far_tap_not_clamped", "bwd_range_narrowed")


def _positions(n_in, n_out, defect=None):
    """(i0, i1, l) of one axis as resize_bilinear_nchw_kernel computes them"""
    if defect == "float64_scale":
        s = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    else:
        s = ((np.arange(n_out, dtype=f32) + f32(0.5)).astype(np.float64) * np.float64(f32(n_in) / f32(n_out)) - 0.5).astype(f32)   # one fma
    if defect != "no_clamp_at_0":
        s = np.maximum(s, 0)
    i0 = np.trunc(s).astype(np.int64)          # (int)s
    i1 = i0 + 1 if defect == "far_tap_not_clamped" else i0 + (i0 < n_in - 1)
    return i0, i1, (s - i0).astype(f32)


def resize_model(c, defect=None):
    """one thread per output, four taps read from the flat buffer (a tap past a row or a plane reads what lies there)"""
    x = _np(NC.resize_inputs(c)[0])
    flat = np.concatenate([x.ravel(), np.full(c.W + 2, 1e3, f32)])
    y0, y1, ly = _positions(c.H, c.Ho, defect)
    x0, x1, lx = _positions(c.W, c.Wo, defect)
    base = (np.arange(c.B * c.C) * c.H * c.W)[:, None, None]
    tap = lambda yy, xx: flat[base + yy[None, :, None] * c.W + xx[None, None, :]]      # noqa: E731
    ly, lx, one = ly[None, :, None], lx[None, None, :], f32(1.0)
    v = (one - ly) * ((one - lx) * tap(y0, x0) + lx * tap(y0, x1)) + ly * ((one - lx) * tap(y1, x0) + lx * tap(y1, x1))
    return v.astype(f32).reshape(c.B, c.C, c.Ho, c.Wo)


def _bwd_axis(n_in, n_out, defect=None):
    """[n_in, n_out] weights as resize_bilinear_nchw_bwd_kernel gathers them: a candidate range per input row, the forward's
    tap arithmetic re-evaluated for every candidate"""
    sh = f32(n_in) / f32(n_out)
    i0, i1, l = _positions(n_in, n_out)
    M = np.zeros((n_in, n_out), f32)
    for y in range(n_in):
        lo = int(np.floor((f32(y) - f32(1.5)) / sh - f32(0.5))) - 1
        hi = int(np.ceil((f32(y) + f32(1.5)) / sh)) + 1
        lo = 0 if y == 0 else lo
        hi = n_out - 1 if y == n_in - 1 else hi
        lo, hi = max(lo, 0), min(hi, n_out - 1)
        if defect == "bwd_range_narrowed":
            lo, hi = lo + 1, hi - 1
        for o in range(lo, hi + 1):
            M[y, o] = (f32(1.0) - l[o] if i0[o] == y else f32(0.0)) + (l[o] if i1[o] == y else f32(0.0))
    return M


def resize_bwd_model(c, defect=None):
    g = _np(NC.resize_inputs(c)[1])
    return np.einsum("yo,bcop,xp->bcyx", _bwd_axis(c.H, c.Ho, defect), g, _bwd_axis(c.W, c.Wo, defect)).astype(f32)


def _resize_margins(c, defect=None):
    return (margin(resize_model(c, defect), NC.resize_ref(c), NC.resize_ref(c, F32)),
            margin(resize_bwd_model(c, defect), NC.resize_grad_ref(c), NC.resize_grad_ref(c, F32)))


@pytest.mark.parametrize("c", NC.RESIZE_CASES + (NC.RESIZE_GRID_CASE,), ids=NC.case_id)
def test_resize_model_passes_every_case(c):
    """... and F.interpolate in fp32, ATen's own statement of the same positions, is inside the bound too."""
    m = _resize_margins(c) + (margin(NC.resize_interpolate32(c), NC.resize_ref(c), NC.resize_ref(c, F32)),)
    print(NC.case_id(c), ["%.3f" % v for v in m])
    assert max(m) <= 1.0, m


def test_the_backward_candidate_range_misses_no_tap():
    """The dense matrices of the kernel's gather and of the forward's taps have the same non-zeros, at every case's two axes."""
    for c in NC.RESIZE_CASES + (NC.RESIZE_GRID_CASE,):
        for n_in, n_out in ((c.H, c.Ho), (c.W, c.Wo)):
            assert np.array_equal(_bwd_axis(n_in, n_out).T, NC.resize_matrix(n_in, n_out, F32).numpy())


@pytest.mark.parametrize("defect", RESIZE_DEFECTS)
def test_a_defective_resize_is_caught(defect):
    m = {NC.case_id(c): _resize_margins(c, defect) for c in NC.RESIZE_CASES}
    print(defect, {k: "%.3g %.3g" % v for k, v in m.items()})
    fwd, bwd = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    assert (bwd if defect == "bwd_range_narrowed" else fwd) > 1.0, m
    if defect in ("no_clamp_at_0", "far_tap_not_clamped"):
        # only an enlarged axis reaches beyond the edge centres (of one sample: both taps are 0 below it, the far tap 1 above it)
        low = 1 if defect == "no_clamp_at_0" else 0
        assert all((v[0] > 1.0) == (c.Ho > c.H > low or c.Wo > c.W > low) for c, v in zip(NC.RESIZE_CASES, m.values())), m


def test_resize_cases_cover_the_shapes_asked_for():
    assert {(c.H, c.W, c.Ho, c.Wo) for c in NC.RESIZE_CASES} == {(5, 7, 16, 23), (16, 23, 5, 7), (4, 6, 25, 37), (6, 6, 6, 6),
                                                                (1, 9, 4, 3), (3, 4, 1, 1)}
    c = NC.RESIZE_GRID_CASE
    assert c.B * c.C * c.Ho * c.Wo > NC.GRID_CAP
    assert torch.equal(NC.resize_ref(NC.RESIZE_CASES[3]).float(), NC.resize_inputs(NC.RESIZE_CASES[3])[0])      # 6x6 -> 6x6: the identity


# ------------------------------------------------------------------------------------------------------------ plane mean, element-wise modes, gate
def _wave_sum(terms):
    """[planes, P] -> [planes]: lane l adds the terms l, l + 64, ... in order, then the xor butterfly 32 .. 1 (lane 0)"""
    n, P = terms.shape
    pad = np.zeros((n, -(-P // 64) * 64), f32)
    pad[:, :P] = terms
    v = np.zeros((n, 64), f32)
    for row in range(pad.shape[1] // 64):
        v = v + pad[:, row * 64:(row + 1) * 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def ew_model(c, mode, defect=None):
    d = {k: _np(v) for k, v in NC.ew_inputs(c).items()}
    a = d["a"]
    out = a + d["b"] if mode == 0 else np.maximum(a, 0) if mode == 1 else _sigmoid(a) if mode == 2 else d["x"] * _sigmoid(a) * d["yv"]
    return _trips(out.astype(f32), defect)


def ew_bwd_model(c, mode, defect=None):
    d = {k: _np(v) for k, v in NC.ew_inputs(c).items()}
    if mode == 1:
        out = np.where(d["y_relu"] > 0, d["g"], f32(0))
    elif mode == 2:
        out = d["g"] * d["y_sigmoid"] * (f32(1) - d["y_sigmoid"])
    elif mode == 4:
        out = np.broadcast_to(d["gp"] / f32(c.H * c.W), d["a"].shape)
    else:
        s = _sigmoid(d["a"])
        out = d["g"] * d["x"] * d["yv"] * s * (f32(1) - s) if mode == 5 else d["g"] * s * d["yv"]
    return _trips(np.ascontiguousarray(out, f32), defect)


def _trips(out, defect):
    """a grid-stride loop that stops after its first trip leaves everything past 16384 x 256 elements unwritten"""
    if defect == "second_trip_skipped":
        out = out.copy()
        out.reshape(-1)[NC.GRID_CAP:] = np.nan
    return out


@pytest.mark.parametrize("c", NC.EW_CASES, ids=NC.case_id)
def test_ew_models_pass_every_case(c):
    d = {k: _np(v) for k, v in NC.ew_inputs(c).items()}
    P = c.H * c.W
    m = {f"ew {mode}": margin(ew_model(c, mode), NC.ew_ref(c, mode), NC.ew_ref(c, mode, F32)) for mode in NC.EW_MODES}
    m.update({f"ew_bwd {mode}": margin(ew_bwd_model(c, mode), NC.ew_bwd_ref(c, mode), NC.ew_bwd_ref(c, mode, F32)) for mode in NC.EW_BWD_MODES})
    mean = (_wave_sum(d["x"].reshape(-1, P)) / f32(P)).reshape(c.B, c.C, 1, 1)
    m["mean"] = margin(mean, NC.mean_ref(c), NC.mean_ref(c, F32))
    gy = _wave_sum((d["g"] * d["x"] * _sigmoid(d["a"])).reshape(-1, P)).reshape(c.B, c.C, 1, 1)
    m["gate_y"] = margin(gy, NC.gate_grads(c)[2], NC.gate_grads(c, F32)[2])
    print(NC.case_id(c), {k: "%.3f" % v for k, v in m.items()})
    assert max(m.values()) <= 1.0, m
    assert abs(d["a"]).max() <= 8.0


def test_a_skipped_second_trip_is_caught_by_the_grid_cases_alone():
    c = NC.EW_GRID_CASE
    assert c.B * c.C * c.H * c.W > NC.GRID_CAP
    for model, ref, ref32 in ((ew_model(c, 3, "second_trip_skipped"), NC.ew_ref(c, 3), NC.ew_ref(c, 3, F32)),
                              (ew_bwd_model(c, 5, "second_trip_skipped"), NC.ew_bwd_ref(c, 5), NC.ew_bwd_ref(c, 5, F32))):
        assert margin(model, ref, ref32) == float("inf") and np.isnan(model.reshape(-1)[-1])
    assert margin(ew_model(c, 3), NC.ew_ref(c, 3), NC.ew_ref(c, 3, F32)) <= 1.0
    assert margin(ew_bwd_model(c, 5), NC.ew_bwd_ref(c, 5), NC.ew_bwd_ref(c, 5, F32)) <= 1.0
    for small in NC.EW_CASES:
        assert margin(ew_model(small, 3, "second_trip_skipped"), NC.ew_ref(small, 3), NC.ew_ref(small, 3, F32)) <= 1.0
    # the resize and the 1x1 convolution of the same size: the reference's last element lies in the second trip
    r = NC.RESIZE_GRID_CASE
    out = _trips(resize_model(r), "second_trip_skipped")
    assert margin(out, NC.resize_ref(r), NC.resize_ref(r, F32)) == float("inf") and np.isnan(out.reshape(-1)[-1])
    g = NC.CONV_GRID_CASE
    out = _trips(conv_model(g), "second_trip_skipped")
    assert margin(out, NC.conv_ref(g), NC.conv_ref(g, dtype=F32)) == float("inf")
    assert margin(conv_model(g), NC.conv_ref(g), NC.conv_ref(g, dtype=F32)) <= 1.0


def test_ew_cases_cover_the_plane_sizes_asked_for():
    assert [c.H * c.W for c in NC.EW_CASES] == [1, 63, 64, 65, 4097]


# ------------------------------------------------------------------------------------------------------------ offset / mask assembly
OM_DEFECTS = ("flow_not_flipped", "slab_tail_skipped", "tile_tail_skipped", "pitch_as_3_third")


def _om_tails(full, c, defect):
    """[B,P,3 third]: what a skipped partial slab of 48 channels / a skipped partial tile of 64 pixels leaves unwritten"""
    n = 3 * c.third
    if defect == "slab_tail_skipped" and n % 48:
        full[..., n // 48 * 48:] = np.nan
    if defect == "tile_tail_skipped" and c.P % 64:
        full[:, c.P // 64 * 64:] = np.nan
    return full


def _om_heads(c, defect):
    o1, o2 = (_np(t) for t in NC.om_inputs(c)[:2])
    n = 3 * c.third
    if defect == "pitch_as_3_third":           # element (b, p, k) read at (b P + p) 3 third + k of the pitched buffer
        return tuple(o.reshape(-1)[:c.B * c.P * n].reshape(c.B, c.P, n) for o in (o1, o2))
    return o1[..., :n], o2[..., :n]


def om_model(c, defect=None):
    """mv_offset_mask_kernel: (offset [B,2 third,P], mask [B,third,P])"""
    a, b = _om_heads(c, defect)
    flow = _np(NC.om_inputs(c)[2])[:, :2 * c.P].reshape(c.B, 2, c.P)
    t2, mag = 2 * c.third, f32(NC.OM_MAG)
    k = np.arange(t2)
    plane = (k & 1) if defect == "flow_not_flipped" else 1 - (k & 1)
    off = mag * np.tanh(a[..., :t2]) + mag * np.tanh(b[..., :t2]) + flow[:, plane, :].transpose(0, 2, 1)
    full = _om_tails(np.concatenate([off, _sigmoid(a[..., t2:] + b[..., t2:])], -1).astype(f32), c, defect)
    return full[..., :t2].transpose(0, 2, 1), full[..., t2:].transpose(0, 2, 1)


def om_bwd_model(c, defect=None):
    """mv_offset_mask_bwd_kernel: (g1, g2) [B,P,3 third]"""
    a, b = _om_heads(c, defect)
    goff, gmask = (_np(t) for t in NC.om_inputs(c)[3:])
    t2, mag = 2 * c.third, f32(NC.OM_MAG)
    go, gm = goff.transpose(0, 2, 1), gmask.transpose(0, 2, 1)
    s = _sigmoid(a[..., t2:] + b[..., t2:])
    r = gm * s * (f32(1) - s)
    g1 = np.concatenate([go * mag * (f32(1) - np.tanh(a[..., :t2]) ** 2), r], -1).astype(f32)
    g2 = np.concatenate([go * mag * (f32(1) - np.tanh(b[..., :t2]) ** 2), r], -1).astype(f32)
    return _om_tails(g1, c, defect), _om_tails(g2, c, defect)


def _om_margins(c, defect=None):
    pairs = list(zip(om_model(c, defect), NC.om_ref(c), NC.om_ref(c, F32))) + list(zip(om_bwd_model(c, defect), NC.om_grad_ref(c), NC.om_grad_ref(c, F32)))
    return [margin(np.ascontiguousarray(got), r, r32) for got, r, r32 in pairs]


@pytest.mark.parametrize("c", NC.OM_CASES, ids=NC.case_id)
def test_assembly_model_passes_every_case(c):
    m = _om_margins(c)
    print(NC.case_id(c), ["%.3f" % v for v in m])
    assert max(m) <= 1.0, m
    o1, o2 = NC.om_inputs(c)[:2]
    n = 3 * c.third
    assert o1[..., :n].abs().max() <= 8.0 and (o1[..., 2 * c.third:n] + o2[..., 2 * c.third:n]).abs().max() <= 8.0


@pytest.mark.parametrize("defect", OM_DEFECTS)
def test_a_defective_assembly_is_caught(defect):
    m = {c: _om_margins(c, defect) for c in NC.OM_CASES}
    print(defect, {NC.case_id(c): ["%.3g" % v for v in vals] for c, vals in m.items()})
    hit = {c: max(v) > 1.0 for c, v in m.items()}
    assert any(hit.values())
    expect = {"flow_not_flipped": lambda c: True, "slab_tail_skipped": lambda c: 3 * c.third % 48 != 0,
              "tile_tail_skipped": lambda c: c.P % 64 != 0, "pitch_as_3_third": lambda c: c.pitched}[defect]
    assert all(hit[c] == expect(c) for c in NC.OM_CASES), hit
    if defect == "flow_not_flipped":           # the flow has no gradient: the forward's offsets alone show it
        assert all(v[0] > 1.0 and max(v[1:]) <= 1.0 for v in m.values())


def test_assembly_cases_cover_the_slabs_tiles_and_pitches_asked_for():
    assert {c.third for c in NC.OM_CASES} == {9, 18, 144} and {c.P for c in NC.OM_CASES} == {63, 64, 65, 130}
    assert sorted({3 * c.third % 48 for c in NC.OM_CASES}) == [0, 6, 27] and 3 * 144 == 9 * 48 and 3 * 18 > 48 > 3 * 9
    for c in NC.OM_CASES:
        ld, fb = NC.om_pitches(c)
        assert c.B == 2 and (ld > 3 * c.third and fb > 2 * c.P) == c.pitched


# ------------------------------------------------------------------------------------------------------------ the references themselves
def test_the_assembly_reference_is_the_modules_formula():
    """mag tanh(o1) + mag tanh(o2) + flow.flip(1) tiled over the pairs, sigmoid(o1 + o2) on the mask third, element by element."""
    c = NC.OM_CASES[2]
    o1, o2, flow, _, _ = NC.om_inputs(c)
    offset, mask = NC.om_ref(c)
    b, p = 1, 17
    fl = flow[b, :2 * c.P].double().view(2, c.P)
    for k in (0, 1, 6, 17):
        want = NC.OM_MAG * torch.tanh(o1[b, p, k].double()) + NC.OM_MAG * torch.tanh(o2[b, p, k].double()) + fl[1 - k % 2, p]
        assert abs(offset[b, k, p].item() - want.item()) < 1e-12
    k = 2 * c.third + 4
    assert abs(mask[b, 4, p].item() - torch.sigmoid(o1[b, p, k].double() + o2[b, p, k].double()).item()) < 1e-15


def test_the_resize_reference_has_atens_positions_and_a_float64_scale_does_not():
    c = NC.RESIZE_CASES[1]
    x = NC.resize_inputs(c)[0]
    ref = NC.resize_ref(c)
    near = (F.interpolate(x, size=(c.Ho, c.Wo), mode="bilinear", align_corners=False).double() - ref).abs().max().item()
    far = (F.interpolate(x.double(), size=(c.Ho, c.Wo), mode="bilinear", align_corners=False) - ref).abs().max().item()
    tol = NC.bound(ref, NC.resize_ref(c, F32))
    print(f"fp32 interpolate {near:.2e}, fp64 interpolate {far:.2e}, bound {tol:.2e}")
    assert near <= tol < far
