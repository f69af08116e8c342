"""Do the fold tests' references and inputs bite?  (No GPU.)

tests/test_gpu_folds.py compares mdta_fold / align_fold / vec_mlp with the float64 formulas of fold_cases.py on the inputs of
fold_cases.py.  Here (1) those formulas are held to the model's own definition -- the oracle's _channel_attention and the
lines of dual_att_alignment, which know nothing of partials or of a folded matrix -- in float64 from float64 partials;
(2) DEFECTIVE folds, the mistakes such kernels make, are put through the same inputs and must move the result by at least
100 x the bound the GPU test applies to that very case; (3) every input family is shown to have the property it is named
for.  Only the float64 reference stands on the passing side: no emulation of the kernels' fp32 arithmetic is asserted to
pass."""
import pytest
import torch

import fold_cases as FC

H, W = FC.FOLD_HW
P = H * W
GATE = FC.mlp_config("gate")
DU0, DU2 = (GATE[0], GATE[1]), (GATE[3], GATE[4])


def _apply(M, *xs):
    """the per-image matrix [B,64,Cin] on every pixel of cat(xs) [B,H,W,Cin], float64"""
    return torch.einsum("boc,bhwc->bhwo", M, torch.cat([x.double() for x in xs], -1))


# ------------------------------------------------------------------------------------------------------------ the fold identity
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("family", FC.FAMILIES)
@pytest.mark.parametrize("CH", [8, 16])
def test_mdta_matrix_is_the_models_attention(CH, family, n):
    """mdta_matrix applied to v == project_out(_channel_attention(q, k, v)), float64 from float64 partials, to 1e-12."""
    B, h, w = 2, 12, 30
    q, k, t = FC.gram_inputs(family, CH, B, h, w)
    v = FC.sum_inputs(family, "v", B, h, w)
    proj, _ = FC.matrices()
    part, _ = FC.split_partials(q, k, CH, n)
    got = _apply(FC.mdta_matrix(part, t, proj), v)
    want = FC.mdta_model(q, k, v, t, proj)
    err = (got - want).abs().max().item()
    print(f"mdta identity CH {CH} {family} n {n}: {err:.1e} (max|ref| {want.abs().max().item():.2f})")
    assert err <= 1e-12, err


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("family", FC.FAMILIES)
def test_align_matrix_is_the_models_alignment(family, n):
    """relu(align_matrix . cat[warped, pred, x]) == the oracle's lines of dual_att_alignment, float64, to 1e-12."""
    B, h, w = 2, 12, 30
    x, warped, pred, t = FC.align_inputs(family, B, h, w)
    proj, wf = FC.matrices()
    want, kf = FC.align_model(x, warped, pred, t, DU0, DU2, proj, wf)
    gpart, _ = FC.split_partials(x, kf, 16, n)
    sw, sp = FC.split_sums(warped, n)[0], FC.split_sums(pred, n)[0]
    got = torch.relu(_apply(FC.align_matrix(gpart, sw, sp, h * w, t, DU0, DU2, proj, wf), warped, pred, x))
    err = (got - want).abs().max().item()
    print(f"align identity {family} n {n}: {err:.1e} (max|ref| {want.abs().max().item():.2e})")
    assert err <= 1e-12, err


@pytest.mark.parametrize("n", FC.SLOT_COUNTS)
def test_slots_partition_the_pixels(n):
    """The slots add up to the whole image, a slot past the last pixel is zero, and slot c is its own pixel range."""
    q, k, _ = FC.gram_inputs("integer", 8, 2, H, W)
    part, part32 = FC.split_partials(q, k, 8, n)
    whole, _ = FC.split_partials(q, k, 8, 1)
    assert torch.equal(part.sum(1), whole[:, 0]) and torch.equal(part32.double(), part)       # integers: exact
    per = -(-P // n)
    first_empty = -(-P // per)
    assert (part[:, first_empty:] == 0).all() and (part[:, :first_empty].abs().amax(-1) > 0).all()
    c = first_empty - 1                                                                        # the ragged last slot
    lo = c * per
    qs, ks = q.double().reshape(2, P, 64)[:, lo:], k.double().reshape(2, P, 64)[:, lo:]
    slot = part[:, c].view(2, 64, 10)
    assert torch.equal(slot[:, 3, 8], qs[:, :, 3].pow(2).sum(1)) and torch.equal(slot[:, 3, 9], ks[:, :, 3].pow(2).sum(1))
    assert torch.equal(slot[:, 11, 2], (qs[:, :, 11] * ks[:, :, 10]).sum(1))                   # head 1 = channels 8..15, j = 2
    x = FC.sum_inputs("integer", "x", 2, H, W)
    sums, _ = FC.split_sums(x, n)
    assert torch.equal(sums.sum(1), x.double().sum((1, 2))) and torch.equal(sums[:, c], x.double().reshape(2, P, 64)[:, lo:].sum(1))


# ------------------------------------------------------------------------------------------------------------ defective folds
def _mdta_case(family, B=5, n=7):
    q, k, t = FC.gram_inputs(family, 8, B, H, W)
    return FC.split_partials(q, k, 8, n)[1], t


def _align_case(family, B=5, n=7):
    q, k, t = FC.gram_inputs(family, 16, B, H, W)
    sw = FC.split_sums(FC.sum_inputs("gate", "warped", B, H, W), n)[1]
    sp = FC.split_sums(FC.sum_inputs("gate", "pred", B, H, W), n)[1]
    return FC.split_partials(q, k, 16, n)[1], sw, sp, t


def _roll_images(*parts):
    return tuple(p.roll(1, 0) for p in parts)


def _drop_last(*parts):
    return tuple(p[:, :-1] for p in parts)


def _margins(defect, which):
    """{family: shift of the matrix under the defect / the GPU test's bound of that case}"""
    proj, wf = FC.matrices()
    out = {}
    for family in FC.FAMILIES:
        if which == "mdta":
            part, t = _mdta_case(family)
            fn = lambda parts, dtype=torch.float64, d=None: FC.mdta_matrix(parts[0], t, proj, dtype, d)      # noqa: E731
            parts = (part,)
        else:
            gp, sw, sp, t = _align_case(family)
            fn = lambda parts, dtype=torch.float64, d=None: FC.align_matrix(*parts, P, t, DU0, DU2, proj, wf, dtype, d)   # noqa: E731
            parts = (gp, sw, sp)
        ref = fn(parts)
        tol = FC.bound(ref, fn(parts, torch.float32))
        if defect == "images_shifted":
            bad = fn(_roll_images(*parts))
        elif defect == "last_slot_dropped":
            bad = fn(_drop_last(*parts))
        else:
            bad = fn(parts, torch.float64, defect)
        out[family] = (bad - ref).abs().max().item() / tol
    return out


@pytest.mark.parametrize("defect", FC.DEFECTS + ("images_shifted", "last_slot_dropped"))
@pytest.mark.parametrize("which", ["mdta", "align"])
def test_a_defective_fold_misses_the_bound_by_100x(which, defect):
    """A transposed softmax block, the temperatures rolled by one head, |q| and |k| exchanged, a clamp of 1e-6, image b's
    partials used for image b + 1, the last slot left out: each moves the folded matrix of at least one family by 100 x
    the bound of test_gpu_folds.py.  The clamp must show in `tiny` (its norms lie between 1e-12 and 1e-6); `hot` cannot be
    the family that catches a transposed block (one-hot rows are nearly symmetric), `plain` is."""
    m = _margins(defect, which)
    print(f"{which} {defect}: " + ", ".join(f"{f} {r:.3g}" for f, r in m.items()))
    assert max(m.values()) >= 100.0, m
    if defect == "clamp_1e-6":
        assert m["tiny"] >= 100.0 and max(r for f, r in m.items() if f != "tiny") == 0.0, m
    if defect in ("transpose", "roll_temperature"):
        assert m["plain"] >= 100.0, m


@pytest.mark.parametrize("defect", FC.ALIGN_DEFECTS)
def test_a_defective_alignment_fold_misses_the_bound_by_100x(defect):
    """g1 and g2 exchanged; the Wb block written from wf[:, :64]."""
    m = _margins(defect, "align")
    print(f"align {defect}: " + ", ".join(f"{f} {r:.3g}" for f, r in m.items()))
    assert max(m.values()) >= 100.0, m


@pytest.mark.parametrize("name", ["gate", "ca", "vmax", "vmax_nobias"])
def test_a_defective_mlp_misses_the_bound_by_100x(name):
    cfg = FC.mlp_config(name)
    part = FC.split_sums(FC.sum_inputs("gate", "x", 5, H, W), 7)[1]
    ref = FC.mlp(part, P, *cfg)
    tol = FC.bound(ref, FC.mlp(part, P, *cfg, dtype=torch.float32))
    for bad in (FC.mlp(part.roll(1, 0), P, *cfg), FC.mlp(part[:, :-1], P, *cfg)):
        assert (bad - ref).abs().max().item() >= 100.0 * tol


# ------------------------------------------------------------------------------------------------------------ the families
@pytest.mark.parametrize("CH", [8, 16])
def test_dead_channels_have_zero_norms_and_uniform_rows(CH):
    q, k, t = FC.gram_inputs("dead", CH, 5, H, W)
    part = FC.split_partials(q, k, CH, 9)[1]
    s = FC.sum_slots(part).view(5, 64, CH + 2)
    assert (s[:, [FC.DEAD_Q, FC.DEAD_BOTH], CH] == 0).all() and (s[:, [FC.DEAD_K, FC.DEAD_BOTH], CH + 1] == 0).all()
    assert (s[..., CH:] == 0).sum().item() == 5 * 4
    A = FC.attention(part, t, CH)
    for c in (FC.DEAD_Q, FC.DEAD_BOTH):
        hb = c // CH * CH
        assert (A[:, c, hb:hb + CH] == 1.0 / CH).all()


@pytest.mark.parametrize("CH", [8, 16])
def test_hot_rows_are_nearly_one_hot_and_tiny_norms_lie_between_the_clamps(CH):
    q, k, t = FC.gram_inputs("hot", CH, 5, H, W)
    A = FC.attention(FC.split_partials(q, k, CH, 7)[1], t, CH)
    assert A.amax(-1).min().item() > 0.99
    q, k, t = FC.gram_inputs("tiny", CH, 5, H, W)
    norms = FC.sum_slots(FC.split_partials(q, k, CH, 7)[1]).view(5, 64, CH + 2)[..., CH:].sqrt()
    assert norms.min().item() > 1e-9 and norms.min().item() < 1e-6 < norms.max().item() * 10, (norms.min(), norms.max())


@pytest.mark.parametrize("B,h,w", FC.PARTIAL_SHAPES)
def test_integer_sums_stay_exact_in_fp32(B, h, w):
    """sum |terms| < 2^24 for every entry of the whole-image sums: any summation order of any slots is exact in fp32."""
    for CH in (8, 16):
        q, k, _ = FC.gram_inputs("integer", CH, B, h, w)
        assert FC.split_partials(q.abs(), k.abs(), CH, 1)[0].max().item() < 2 ** 24
    assert FC.split_sums(FC.sum_inputs("integer", "x", B, h, w).abs(), 1)[0].max().item() < 2 ** 24


def test_gate_preactivations_reach_beyond_six():
    x = FC.sum_inputs("gate", "x", 5, H, W)
    part = FC.split_sums(x, 7)[1]
    for name in ("gate", "ca"):
        pre = FC.mlp_preact(part, P, *FC.mlp_config(name))
        assert pre.min().item() < -6.0 and pre.max().item() > 6.0, (name, pre.min(), pre.max())
