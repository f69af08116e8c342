"""Do the cases of the CVSR_V7 operator tests bite?  (No GPU.)

tests/test_gpu_v7_ops.py compares the kernels of csrc/v7_ops.hip and csrc/v7_train.hip with the float64 references of v7_cases.py
on the inputs of v7_cases.py, within fold_cases.bound or by equality.  Here every kernel is restated in numpy fp32 as a MODEL that
follows the kernel's own structure (16 lanes of 4 channels with the xor butterfly and its tie rule, the 64-pixel tiles and the
surplus wave, nested tap loops with bounds checks over the flat pooled buffer, e / sum + gate) and can be given one of the
mistakes such a kernel makes.  Asserted: the defect-free model lands inside the bound of EVERY case (equal, for the exact
families), and every defect lands outside the bound of AT LEAST ONE named case (an element left unwritten = NaN is outside, and
so is a write past the end of the output).  The models are independent of the references: the references are torch.max / mean /
F.conv2d / softmax / F.interpolate and autograd on NCHW tensors."""
import numpy as np
import pytest
import torch

import v7_cases as VC

f32 = np.float32
F64, F32 = torch.float64, torch.float32
INF = float("inf")
LANES = np.arange(16)


def _np(t):
    return t.numpy()


def _sigmoid(v):
    return (f32(1.0) / (f32(1.0) + np.exp(-v))).astype(f32)


def margin(got, ref, restated, exact=False):
    """error / bound of a model result against the reference; inf for another shape or an unwritten (NaN) element.  exact: 0 for
    equality, inf otherwise."""
    got = (got if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(got))).double()
    if got.shape != ref.shape:
        return INF
    if exact:
        return 0.0 if torch.equal(got, ref) else INF
    err = (got - ref).abs().max().item()
    return INF if err != err else err / VC.bound(ref, restated)


def _caught(m):
    return {k: v for k, v in m.items() if v > 1.0}


# ------------------------------------------------------------------------------------------------------------ per-pixel kernels
POOL_DEFECTS = ("mean_of_63", "max_seeded_with_0")
POOL_BWD_DEFECTS = ("last_tie_wins", "tie_gradient_split", "butterfly_one_step_short")


def _lanes(t):
    """[B,H,W,64] -> [npix,16,4]: lane l holds the channels 4 l .. 4 l + 3"""
    return _np(t).reshape(-1, 16, 4)


def pool_model(c, defect=None):
    """chan_pool_kernel: per-lane max and sum of four, xor butterfly 8 4 2 1, lane 0 writes (max, sum / 64)"""
    v = _lanes(VC.pix_inputs(c)["x"])
    mx = np.maximum(np.maximum(v[..., 0], v[..., 1]), np.maximum(v[..., 2], v[..., 3]))
    if defect == "max_seeded_with_0":
        mx = np.maximum(mx, f32(0))
    last = np.where(LANES == 15, f32(0), v[..., 3]) if defect == "mean_of_63" else v[..., 3]
    sm = (v[..., 0] + v[..., 1]) + (v[..., 2] + last)
    for o in (8, 4, 2, 1):
        mx, sm = np.maximum(mx, mx[:, LANES ^ o]), sm + sm[:, LANES ^ o]
    mean = sm[:, 0] * (f32(1) / f32(63 if defect == "mean_of_63" else 64))
    return np.stack([mx[:, 0], mean], -1).astype(f32).reshape(c.B, c.H, c.W, 2)


def pool_bwd_model(c, defect=None):
    """chan_pool_bwd_kernel: the first maximum of a lane's four, the butterfly carrying (max, arg) with `smaller channel wins a
    tie`, every lane writes dmean / 64 + [channel == arg] dmax"""
    d = VC.pix_inputs(c)
    v, cot = _lanes(d["x"]), _np(d["cot2"]).reshape(-1, 2)
    later = defect == "last_tie_wins"
    mx, am = v[..., 0].copy(), np.broadcast_to(LANES * 4, v.shape[:2]).copy()
    for k in (1, 2, 3):
        take = (v[..., k] >= mx) if later else (v[..., k] > mx)
        mx, am = np.where(take, v[..., k], mx), np.where(take, LANES * 4 + k, am)
    for o in ((4, 2, 1) if defect == "butterfly_one_step_short" else (8, 4, 2, 1)):
        om, oa = mx[:, LANES ^ o], am[:, LANES ^ o]
        take = (om > mx) | ((om == mx) & ((oa > am) if later else (oa < am)))
        mx, am = np.where(take, om, mx), np.where(take, oa, am)
    dmax, dmean = cot[:, 0, None, None], (cot[:, 1] * (f32(1) / f32(64)))[:, None, None]
    ch = (LANES * 4)[None, :, None] + np.arange(4)[None, None, :]
    if defect == "tie_gradient_split":
        tied = v == v.max((1, 2), keepdims=True)
        g = dmean + tied * (dmax / tied.sum((1, 2), keepdims=True).astype(f32))
    else:
        g = dmean + np.where(ch == am[:, :, None], dmax, f32(0))
    return g.astype(f32).reshape(c.B, c.H, c.W, 64)


def _dot16(a, b):
    """dot_plane_kernel / softmax64_bwd_kernel: [npix,16,4] twice -> [npix]; pairs of products, then the butterfly"""
    s = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + (a[..., 2] * b[..., 2] + a[..., 3] * b[..., 3])
    for o in (8, 4, 2, 1):
        s = s + s[:, LANES ^ o]
    return s[:, 0]


def mul_plane_model(c):
    """(x * plane, y * plane, sum_c y x): mul_plane_kernel on x and on the cotangent, dot_plane_kernel"""
    d = VC.pix_inputs(c)
    pl = _np(d["plane"])[..., None]
    return _np(d["x"]) * pl, _np(d["y"]) * pl, _dot16(_lanes(d["y"]), _lanes(d["x"])).reshape(c.B, c.H, c.W)


def softmax_rows_bwd_model(c):
    """softmax64_bwd_kernel on the fp32 rows r: r (dm - sum_c r dm), the sum by _dot16"""
    r, dm = _lanes(VC.softmax_rows_ref(c)[0].float()), _lanes(VC.pix_inputs(c)["y"])
    return (r * (dm - _dot16(r, dm)[:, None, None])).reshape(c.B, c.H, c.W, 64)


def _pool_margins(c, defect=None):
    exact = c.family in VC.EXACT_FAMILIES
    (ref, gref), (r32, g32) = VC.pool_ref(c), VC.pool_ref(c, F32)
    fwd = pool_model(c, defect if defect in POOL_DEFECTS else None)
    bwd = pool_bwd_model(c, defect if defect in POOL_BWD_DEFECTS else None)
    return margin(fwd, ref, r32, exact), margin(bwd, gref, g32, exact)


@pytest.mark.parametrize("c", VC.PIX_CASES, ids=VC.case_id)
def test_per_pixel_models_pass_every_case(c):
    exact = c.family in VC.EXACT_FAMILIES
    m = list(_pool_margins(c))
    m += [margin(got, r, r32, exact) for got, r, r32 in zip(mul_plane_model(c), VC.mul_plane_ref(c), VC.mul_plane_ref(c, F32))]
    if not exact:
        m.append(margin(softmax_rows_bwd_model(c), VC.softmax_rows_ref(c)[1], VC.softmax_rows_ref(c, F32)[1]))
    print(VC.case_id(c), ["%.3f" % v for v in m])
    assert max(m) <= 1.0, m


@pytest.mark.parametrize("defect", POOL_DEFECTS + POOL_BWD_DEFECTS)
def test_a_defective_channel_pool_is_caught(defect):
    m = {c: _pool_margins(c, defect) for c in VC.PIX_CASES}
    hit = {VC.case_id(c): v for c, v in m.items() if max(v) > 1.0}
    print(defect, hit)
    assert hit
    if defect == "max_seeded_with_0":          # only a pixel whose channels are all negative shows it: `negative` has them at every size
        assert all(m[c][0] > 1.0 for c in VC.PIX_CASES if c.family == "negative")
        assert all(m[c][0] <= 1.0 for c in VC.PIX_CASES if c.family == "plain" and c.B * c.H * c.W < 100)
    if defect in ("last_tie_wins", "tie_gradient_split"):      # a tie moves the gradient and not the maximum: `ties` alone, at every size
        assert all((max(m[c]) > 1.0) == (c.family == "ties") and m[c][0] <= 1.0 for c in VC.PIX_CASES), hit
    if defect == "butterfly_one_step_short":   # two groups of 8 lanes mark a channel each: any pixel shows it
        assert all(m[c][1] > 1.0 for c in VC.PIX_CASES), hit


def test_per_pixel_cases_have_the_data_they_are_named_for():
    assert [s[0] * s[1] * s[2] for s in VC.PIX_SHAPES] == [1, 6, 15, 16, 17, 126, 720]
    for c in VC.PIX_CASES:
        d = VC.pix_inputs(c)
        x = d["x"].view(-1, 64)
        if c.family == "negative":
            assert (x[0::2] < 0).all() and (x.max(1)[0] > 0).any() == (x.shape[0] > 1)
        if c.family == "ties":
            assert all(torch.equal(t, t.round()) for t in d.values()) and x.abs().max() <= 1
            top = x == x.max(1, keepdim=True)[0]
            for q in range(x.shape[0]):
                kind, where = VC.tie_kind(q), top[q].nonzero().flatten().tolist()
                if kind == "two_lanes":
                    assert where == list(VC.TIE_PAIR) and where[0] // 4 != where[1] // 4
                elif kind == "all_equal":
                    assert len(where) == 64
                elif kind != "random":
                    assert where == [0 if kind == "only_0" else 63]
            kinds = {VC.tie_kind(q) for q in range(x.shape[0])}
            assert kinds == set(VC.TIE_KINDS) or x.shape[0] < len(VC.TIE_KINDS)
            # the adjoint's expectation puts the whole of dmax on the FIRST maximum
            gref = VC.pool_ref(c)[1].view(-1, 64)
            first = top.int().argmax(1)
            want = d["cot2"].view(-1, 2).double()
            assert torch.equal(gref[torch.arange(x.shape[0]), first], want[:, 0] + want[:, 1] / 64)


# ------------------------------------------------------------------------------------------------------------ pooled_conv users
GATE_DEFECTS = ("radius_off_by_one", "planes_swapped", "no_column_bound", "no_image_bound")
CUM_DEFECTS = ("cum_on_centre_tap_only", "cum_dropped_from_product")


def pooled_conv_model(pooled, w, ks, defect=None, cum=None):
    """pooled_conv / gate_map_cum_kernel's loop: [B,H,W,2] -> the sum s [B,H,W].  One flat buffer of all images (zeros before and
    after it): a tap that is not stopped by its bounds check reads what lies at its address.  cum [B,H,W]: every tap's pooled
    pair is scaled by the plane at the tap."""
    B, H, W, _ = pooled.shape
    r = (ks - 1) // 2
    guard = (ks + 1) * (W + 1)
    flat = np.zeros((B * H * W + 2 * guard, 2), f32)
    flat[guard:guard + B * H * W] = pooled.reshape(-1, 2)
    cflat = np.ones(flat.shape[0], f32)
    if cum is not None:
        cflat[guard:guard + B * H * W] = cum.reshape(-1)
    b, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    w0, w1 = (w[0, 1], w[0, 0]) if defect == "planes_swapped" else (w[0, 0], w[0, 1])
    rr = r + 1 if defect == "radius_off_by_one" else r
    s = np.zeros((B, H, W), f32)
    for dy in range(ks):
        yy = y + dy - rr
        rows = np.ones_like(yy, bool) if defect == "no_image_bound" else (yy >= 0) & (yy < H)
        for dx in range(ks):
            xx = x + dx - rr
            ok = rows if defect == "no_column_bound" else rows & (xx >= 0) & (xx < W)
            at = guard + (b * H + yy) * W + xx
            pv = flat[np.where(ok, at, 0)]
            g = cflat[np.where(ok, at, 0)]
            if defect == "cum_on_centre_tap_only" and not (dy == r and dx == r):
                g = f32(1)
            term = w0[dy, dx] * (pv[..., 0] * g) + (w1[dy, dx] * (pv[..., 1] * g) + s)
            s = np.where(ok, term, s).astype(f32)
    return s


def gate_model(c, defect=None, inputs=VC.gate_inputs, ks=None):
    """chan_pool, gate_map_kernel, spatial_gate_kernel: x * sigmoid(s + bias)"""
    x, w, b = (_np(t) for t in inputs(c))
    pooled = np.stack([x.max(-1), x.mean(-1, dtype=f32)], -1)
    return x * _sigmoid(pooled_conv_model(pooled, w, ks or c.ks, defect) + b[0])[..., None]


def cum_model(c, defect=None):
    """gate_map_cum_kernel, CUM_ROUNDS times from pool(x_0): [x_0 G_1 .. x_0 G_4]"""
    x, w, b = (_np(t) for t in VC.gate_inputs(c))
    pooled = np.stack([x.max(-1), x.mean(-1, dtype=f32)], -1)
    G, outs = None, []
    for _ in range(VC.CUM_ROUNDS):
        g = _sigmoid(pooled_conv_model(pooled, w, c.ks, defect if defect in CUM_DEFECTS else None, G) + b[0])
        G = g if (G is None or defect == "cum_dropped_from_product") else G * g
        outs.append(x * G[..., None])
    return outs


def _gate_margin(c, defect=None):
    return margin(gate_model(c, defect), VC.gate_ref(c)[0], VC.gate_ref(c, F32)[0])


def _cum_margins(c, defect=None):
    return [margin(got, r, r32) for got, r, r32 in zip(cum_model(c, defect), VC.cum_ref(c), VC.cum_ref(c, F32))]


@pytest.mark.parametrize("c", VC.GATE_CASES, ids=VC.case_id)
def test_gate_model_passes_every_case(c):
    m = _gate_margin(c)
    arg = VC.gate_ref(c)[1].abs().max().item()
    print(VC.case_id(c), "%.3f" % m, "max|argument| %.2f" % arg)
    assert m <= 1.0 and arg <= 8.0


@pytest.mark.parametrize("c", [c for c in VC.PIX_CASES if c.family == "plain"], ids=VC.case_id)
def test_gate_model_passes_the_per_pixel_shapes(c):
    """spatial_gate at the pixel counts around its 16-pixel block"""
    (ref, arg), (r32, _) = VC.pix_gate_ref(c), VC.pix_gate_ref(c, F32)
    m = margin(gate_model(c, None, VC.pix_gate_inputs, 7), ref, r32)
    print(VC.case_id(c), "%.3f" % m, "max|argument| %.2f" % arg.abs().max().item())
    assert m <= 1.0 and arg.abs().max().item() <= 8.0


@pytest.mark.parametrize("c", VC.CUM_CASES, ids=VC.case_id)
def test_cumulative_gate_model_passes_every_round(c):
    m = _cum_margins(c)
    print(VC.case_id(c), ["%.3f" % v for v in m])
    assert max(m) <= 1.0, m


@pytest.mark.parametrize("defect", GATE_DEFECTS)
def test_a_defective_gate_is_caught(defect):
    m = {c: _gate_margin(c, defect) for c in VC.GATE_CASES}
    print(defect, {VC.case_id(c): "%.3g" % v for c, v in m.items()})
    hit = {c: v > 1.0 for c, v in m.items()}
    assert any(hit.values())
    # every case: a tap right of a row lands in the next row or, from the last row, in the next image; a tap below image 0 lands
    # in image 1 -- the 1x1 maps included
    assert all(hit.values()), hit


@pytest.mark.parametrize("defect", CUM_DEFECTS)
def test_a_defective_cumulative_gate_is_caught(defect):
    m = {c: _cum_margins(c, defect) for c in VC.CUM_CASES}
    print(defect, {VC.case_id(c): ["%.3g" % v for v in vals] for c, vals in m.items()})
    # round 1 has no plane yet: both defects are invisible there and show from round 2 on; a 1x1 map has the centre tap only
    assert all(vals[0] <= 1.0 for vals in m.values())
    for c, vals in m.items():
        if defect == "cum_dropped_from_product" or c.H * c.W > 1:
            assert min(vals[1:]) > 1.0, (c, vals)
        else:
            assert max(vals) <= 1.0, (c, vals)


def test_gate_cases_have_the_shapes_and_weights_they_are_named_for():
    assert {(c.B, c.H, c.W) for c in VC.GATE_CASES} == set(VC.GATE_SHAPES) and {c.ks for c in VC.GATE_CASES} == {7, 3}
    assert [(c.H, c.W) for c in VC.CUM_CASES] == [(1, 1), (3, 5), (9, 11)] and VC.CUM_ROUNDS == 4
    for c in VC.GATE_CASES + VC.CUM_CASES:
        x, w, b = VC.gate_inputs(c)
        assert c.B >= 2 and w.shape == (1, 2, c.ks, c.ks)
        pooled = VC.channel_pool(VC.nchw(x))
        assert (pooled[0] - pooled[1]).abs().amax((1, 2)).min() > 0.05       # the two images are unlike, in both planes
        assert not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3)) and not torch.equal(w, w.transpose(2, 3))
        assert not torch.equal(w[0, 0], w[0, 1])
    assert any(c.H < c.ks and c.W < c.ks for c in VC.GATE_CASES) and any(c.W == 1 and c.H > 1 for c in VC.GATE_CASES)


# ------------------------------------------------------------------------------------------------------------ rdab_mix, gumbel_softmax
MIX_DEFECTS = ("noise_as_nhwc", "partial_tile_unwritten", "surplus_wave_writes_past_the_end", "log_off_by_2^-21")
LOG_ERR = f32(2.0 ** -21)


def _noise(c, defect):
    """[B,P,64]: the 64 noise values of every pixel as the kernels gather them from the NCHW tensor"""
    u = _np(VC.mix_inputs(c)["u"])
    P = c.H * c.W
    if defect == "noise_as_nhwc":              # element (b, c, p) read at (b P + p) 64 + c
        return u.reshape(c.B, P, 64)
    return u.reshape(c.B, 64, P).transpose(0, 2, 1)


def _log(u, defect):
    lg = np.log(u).astype(f32)
    return lg - LOG_ERR if defect == "log_off_by_2^-21" else lg


def _tiles(full, c, defect):
    """[B,P,64]: what a skipped partial tile of 64 pixels leaves unwritten"""
    P = c.H * c.W
    if defect == "partial_tile_unwritten" and P % 64:
        full[:, P // 64 * 64:] = np.nan
    return full


def softmax_model(c, defect=None):
    """gumbel_softmax_kernel: z = v - log(-log u), the maximum, exp(z - m) and its sum in channel order, one tile = 64 pixels"""
    v = _np(VC.mix_inputs(c)["v"])[:, None, :]
    with np.errstate(all="ignore"):
        z = (v - np.log(-_log(_noise(c, defect), defect))).astype(f32)
        e = np.exp(z - z.max(-1, keepdims=True)).astype(f32)
    s = np.zeros(e.shape[:2], f32)
    for ch in range(64):
        s = s + e[..., ch]
    return _tiles(e * (f32(1) / s)[..., None], c, defect).reshape(c.B, c.H, c.W, 64)


def softmax_bwd_model(c, r):
    """softmax64_bwd_kernel and the column sum over the pixels of an image: dv [B,64] from the fp32 rows r"""
    cot = _lanes(VC.mix_inputs(c)["cot"])
    rl = r.reshape(-1, 16, 4)
    dz = rl * (cot - _dot16(rl, cot)[:, None, None])
    return dz.reshape(c.B, c.H * c.W, 64).sum(1, dtype=f32)


def mix_model(c, defect=None):
    """rdab_mix_kernel: blocks of two waves, wave -> tile min(2 block + wave, B tiles - 1), e = exp(v - vmax) / (-log u), the sum in
    channel order, x_f (e / sum + gate), the gate by the kernel's own pooled_conv(..., 3) (it takes the GATE_DEFECTS too).  Returns (out [B,H,W,64], rows written past the end of the output)."""
    d = {k: _np(t) for k, t in VC.mix_inputs(c).items()}
    P = c.H * c.W
    tiles, Bt = -(-P // 64), VC.mix_tiles(c)
    v = d["v"]
    with np.errstate(all="ignore"):
        e = (np.exp(v - v.max(-1, keepdims=True)).astype(f32)[:, None, :] / -_log(_noise(c, defect), defect)).astype(f32)
    s = np.zeros(e.shape[:2], f32)
    for ch in range(64):
        s = s + e[..., ch]
    xc = d["xc"]
    pooled = np.stack([xc.max(-1), xc.mean(-1, dtype=f32)], -1)
    gate = _sigmoid(pooled_conv_model(pooled, d["w3"], 3, defect if defect in GATE_DEFECTS else None) + d["b3"][0]).reshape(c.B, P)
    with np.errstate(all="ignore"):
        full = d["xf"].reshape(c.B, P, 64) * (e * (f32(1) / s)[..., None] + gate[..., None])
    full = _tiles(full.astype(f32), c, defect)
    out, past = np.full((c.B, P, 64), np.nan, f32), 0
    for block in range((Bt + 1) // 2):
        for wave in range(2):
            tile = 2 * block + wave
            if defect != "surplus_wave_writes_past_the_end":
                tile = min(tile, Bt - 1)
            b, p0 = tile // tiles, tile % tiles * 64
            if b >= c.B:
                past += min(64, P - p0)
                continue
            out[b, p0:p0 + 64] = full[b, p0:p0 + 64]
    return out.reshape(c.B, c.H, c.W, 64), past


def _mix_margins(c, defect=None):
    """(rdab_mix, gumbel_softmax, its gradient to v)"""
    out, past = mix_model(c, defect)
    r = softmax_model(c, defect)
    (rref, dvref), (r32, dv32) = VC.softmax_ref(c), VC.softmax_ref(c, F32)
    with np.errstate(all="ignore"):
        dv = softmax_bwd_model(c, r)
    return (INF if past else margin(out, VC.mix_ref(c), VC.mix_ref(c, F32)), margin(r, rref, r32), margin(dv, dvref, dv32))


@pytest.mark.parametrize("c", VC.MIX_CASES, ids=VC.case_id)
def test_mix_and_softmax_models_pass_every_case(c):
    m = _mix_margins(c)
    print(VC.case_id(c), ["%.3f" % v for v in m], "bounds %.2e %.2e" % (VC.bound(VC.mix_ref(c), VC.mix_ref(c, F32)),
                                                                        VC.bound(VC.softmax_ref(c)[0], VC.softmax_ref(c, F32)[0])))
    assert max(m) <= 1.0, m
    assert all(torch.isfinite(t).all() for dt in (F64, F32) for t in (VC.mix_ref(c, dt), *VC.softmax_ref(c, dt)))
    assert VC.mix_gate_arg(c).abs().max().item() <= 8.0


@pytest.mark.parametrize("defect", MIX_DEFECTS)
def test_a_defective_mix_or_softmax_is_caught(defect):
    m = {c: _mix_margins(c, defect) for c in VC.MIX_CASES}
    print(defect, {VC.case_id(c): ["%.3g" % v for v in vals] for c, vals in m.items()})
    hit = {c: (vals[0] > 1.0, vals[1] > 1.0) for c, vals in m.items()}
    assert any(h[0] for h in hit.values()) and (defect == "surplus_wave_writes_past_the_end" or any(h[1] for h in hit.values()))
    P = lambda c: c.H * c.W  # noqa: E731
    if defect == "noise_as_nhwc":              # one pixel per image: [64][1] and [1][64] are the same buffer
        assert all(h == ((P(c) > 1,) * 2) for c, h in hit.items()), hit
    if defect == "partial_tile_unwritten":
        assert all(h == ((P(c) % 64 != 0,) * 2) for c, h in hit.items()), hit
    if defect == "surplus_wave_writes_past_the_end":       # rdab_mix alone has waves in pairs
        assert all(h == (VC.mix_tiles(c) % 2 == 1, False) for c, h in hit.items()), hit
    if defect == "log_off_by_2^-21":
        # an absolute error of a logarithm is a relative error of -log u only where u is close to 1: the `extreme` family has a
        # tenth of its entries there and must catch it, in both kernels, at every size; `uniform` is not relied upon
        extreme = [h for c, h in hit.items() if c.noise == "extreme"]
        assert all(h == (True, True) for h in extreme), hit


@pytest.mark.parametrize("defect", GATE_DEFECTS)
def test_a_defective_gate_inside_the_mix_is_caught(defect):
    """rdab_mix has its own copy of the tap loop: the MIX cases themselves must show a mistake in it"""
    m = {c: _mix_margins(c, defect)[0] for c in VC.MIX_CASES}
    print(defect, {VC.case_id(c): "%.3g" % v for c, v in m.items()})
    hit = {c: v > 1.0 for c, v in m.items()}
    if defect == "no_image_bound":             # a tap past an image lands in its neighbour: the batches of 2 and 3, one pixel included
        assert all(h == (c.B > 1) for c, h in hit.items()), hit
    else:                                      # every one-image case has more than one row for a wrapped tap to land in
        assert all(hit.values()) and all(c.B > 1 or c.H > 1 for c in hit), hit


def test_mix_cases_have_the_tiles_and_the_noise_they_are_named_for():
    assert [s[1] * s[2] for s in VC.MIX_SHAPES] == [1, 63, 64, 65, 130, 65, 240]
    assert [VC.mix_tiles(VC.MixCase("uniform", "spread", *s)) for s in VC.MIX_SHAPES] == [3, 1, 1, 2, 3, 6, 8]
    assert f32(VC.U_TOP) == np.nextafter(f32(1), f32(0)) and 0 < f32(VC.U_LOW) == torch.tensor(1e-30).item()
    for c in VC.MIX_CASES:
        d = VC.mix_inputs(c)
        u, v = d["u"], d["v"]
        assert u.dtype == F32 and u.min().item() >= float(f32(VC.U_LOW)) and u.max().item() <= VC.U_TOP
        if c.noise == "extreme":
            n = u.numel()
            assert (u == VC.U_TOP).sum() > 0.04 * n and (u == float(f32(VC.U_LOW))).sum() > 0.04 * n
            assert ((u > 1 - 1.01e-4) & (u < VC.U_TOP)).sum() > 0.04 * n
        top2 = v.topk(2, dim=1)[0]
        assert ((top2[:, 0] - top2[:, 1] >= 17) if c.v == "peaked" else (top2[:, 0] <= 3)).all()


# ------------------------------------------------------------------------------------------------------------ shrink_planes
SHRINK_DEFECTS = ("level2_top_left_block", "level2_divided_by_2")


def shrink_model(c, defect=None):
    """shrink_planes_kernel: the mean of the central 2x2 of every 2^level block, times 2^-level"""
    s = _np(VC.shrink_input(c))[:, VC.SHRINK_FRAME]
    lv = c.level
    o = 1 if (lv == 2 and defect != "level2_top_left_block") else 0
    st = 1 << lv
    m = f32(0.25) * ((s[..., o::st, o::st] + s[..., o::st, o + 1::st]) + (s[..., o + 1::st, o::st] + s[..., o + 1::st, o + 1::st]))
    return (m * f32(0.5 if (lv == 1 or defect == "level2_divided_by_2") else 0.25)).astype(f32)


def _shrink_margin(c, defect=None):
    return margin(shrink_model(c, defect), VC.shrink_ref(c), VC.shrink_ref(c, F32), c.data == "integer")


@pytest.mark.parametrize("c", VC.SHRINK_CASES, ids=VC.case_id)
def test_shrink_model_passes_every_case(c):
    assert _shrink_margin(c) <= 1.0
    assert tuple(VC.shrink_ref(c).shape) == (c.B, c.planes, c.H >> c.level, c.W >> c.level)


@pytest.mark.parametrize("defect", SHRINK_DEFECTS)
def test_a_defective_shrink_is_caught(defect):
    hit = {c: _shrink_margin(c, defect) > 1.0 for c in VC.SHRINK_CASES}
    print(defect, {VC.case_id(c): h for c, h in hit.items()})
    assert all(h == (c.level == 2) for c, h in hit.items()), hit


def test_shrink_cases_cover_the_smallest_maps_and_a_one_plane_source():
    shapes = {(c.B, c.planes, c.H, c.W, c.level) for c in VC.SHRINK_CASES}
    assert shapes == set(VC.SHRINK_SHAPES) and (1, 1, 2, 2, 1) in shapes and (1, 1, 4, 4, 2) in shapes
    for c in VC.SHRINK_CASES:
        t = VC.shrink_input(c)
        assert t.shape[1] == 7 and (c.data != "integer" or torch.equal(t, t.round()))


# ------------------------------------------------------------------------------------------------------------ lincomb
LIN_DEFECTS = ("first_block_only", "cc_applied_to_b")


def lin_model(c, defect=None):
    """lincomb_kernel: ca a, then fma(cb, b, .), then fma(cc, c, .), one float4 per thread, 256 threads per block.  The output may
    be a or b itself: every thread reads its own four elements of all operands before it writes them."""
    a, b, cc_ = (_np(t) for t in VC.lin_inputs(c))
    ca, cb, cc = (f32(v) for v in VC.LIN_COEFFS[c.data])
    r = a * ca
    if c.has_b:
        r = (cc if defect == "cc_applied_to_b" else cb) * b + r
    if c.has_c:
        r = cc * cc_ + r
    out = {"new": np.full(c.n, np.nan, f32), "a": a.copy(), "b": b.copy()}[c.out]
    n = min(c.n, 1024) if defect == "first_block_only" else c.n
    out[:n] = r[:n]
    return out


def _lin_margin(c, defect=None):
    return margin(lin_model(c, defect), VC.lin_ref(c), VC.lin_ref(c, F32), c.data == "integer")


@pytest.mark.parametrize("c", VC.LIN_CASES, ids=VC.case_id)
def test_lincomb_model_passes_every_case(c):
    assert _lin_margin(c) <= 1.0


@pytest.mark.parametrize("defect", LIN_DEFECTS)
def test_a_defective_lincomb_is_caught(defect):
    hit = {c: _lin_margin(c, defect) > 1.0 for c in VC.LIN_CASES}
    print(defect, {VC.case_id(c): h for c, h in hit.items()})
    expect = (lambda c: c.n > 1024) if defect == "first_block_only" else (lambda c: c.has_b)
    assert all(h == expect(c) for c, h in hit.items()), hit


def test_lincomb_cases_cover_the_lengths_operands_and_aliases_asked_for():
    assert {c.n for c in VC.LIN_CASES} == {4, 1024, 1028}
    assert {(c.has_b, c.has_c) for c in VC.LIN_CASES if c.out == "new"} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c.out for c in VC.LIN_CASES} == {"new", "a", "b"}
    for v in VC.LIN_COEFFS["integer"]:
        assert np.log2(abs(v)) == round(np.log2(abs(v)))
