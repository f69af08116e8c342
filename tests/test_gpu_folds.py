"""The channel-attention chain on the GPU, piece by piece: gram_partial / chan_sum_partial (partials), mdta_fold / align_fold /
vec_mlp / fold_scale_inputs (partials -> a per-image packed 1x1 matrix or a gate vector), and the chain partials -> fold -> conv
against the model's own definition.  Inputs, float64 references and bounds live in fold_cases.py; test_fold_cases_cpu.py
shows that the references equal the model's attention and that the inputs catch defective folds.

Bounds.  Partials of integer data: exact, slot by slot.  Partials of fp32 data: (per/4 + 8) 2^-24 sum|terms| per entry (one
thread adds at most per/4 + 1 terms in order, then a fixed tree; per = pixels per slot).  Folds and chain:
max(4 x the error of the same formula in torch fp32 on the CPU, 2^-20 max|ref|), see fold_cases.bound.  The Wb third of
align_fold's matrix is a copy (bitwise), a dead channel's softmax row is exactly 1/CH, every fold is run twice (bitwise).

Measured on MI355X, max-abs error against float64 (smallest .. largest over the cases of a row), the bounds of those cases, and
the worst error / bound; each test prints its own figures:
    partials, integer data (14 shapes + slices)      exact in every slot
    partials, fp32 data 2x37x53 (n 1)       error / bound: gram CH 8 0.0218, CH 16 0.0216, chan_sum 0.0057
    partials, fp32 data 1x64x64 (n 4)       error / bound: gram CH 8 0.0239, CH 16 0.0240, chan_sum 0.0092
  folds from synthetic partials, 6 slot counts x B 1 and 5 (12 cases a row):
    mdta_fold plain                 err 1.45e-08 .. 2.19e-08   bound 1.43e-07 .. 1.45e-07   worst 0.151
    mdta_fold dead                  err 1.42e-08 .. 2.27e-08   bound 1.44e-07 .. 1.44e-07   worst 0.158
    mdta_fold aligned               err 2.69e-08 .. 4.19e-08   bound 1.77e-07 .. 1.77e-07   worst 0.237
    mdta_fold hot                   err 4.43e-08 .. 9.81e-08   bound 4.30e-07 .. 4.30e-07   worst 0.228
    mdta_fold negative              err 1.80e-08 .. 2.52e-08   bound 1.73e-07 .. 1.77e-07   worst 0.142
    mdta_fold tiny                  err 1.80e-08 .. 2.16e-08   bound 1.44e-07 .. 1.45e-07   worst 0.149
    mdta_fold identity-proj dead    err 1.60e-08 .. 2.15e-08   bound 1.30e-07 .. 1.30e-07   worst 0.166   dead rows exactly 1/8
    align_fold plain                err 1.57e-08 .. 2.80e-08   bound 3.41e-07 .. 3.41e-07   worst 0.082
    align_fold dead                 err 1.59e-08 .. 2.91e-08   bound 3.41e-07 .. 3.41e-07   worst 0.085
    align_fold aligned              err 1.98e-08 .. 3.11e-08   bound 3.41e-07 .. 3.41e-07   worst 0.091
    align_fold hot                  err 9.25e-08 .. 1.57e-07   bound 3.41e-07 .. 4.94e-07   worst 0.461
    align_fold negative             err 1.65e-08 .. 3.16e-08   bound 3.41e-07 .. 3.41e-07   worst 0.093
    align_fold tiny                 err 1.60e-08 .. 2.82e-08   bound 3.41e-07 .. 3.41e-07   worst 0.083   Wb third bitwise in all 72
    vec_mlp gate (64-4-64 sigmoid)  err 9.03e-08 .. 7.53e-07   bound 9.54e-07 .. 1.91e-06   worst 0.682
    vec_mlp ca (64-64-64 sigmoid)   err 2.46e-07 .. 5.01e-07   bound 9.54e-07 .. 1.42e-06   worst 0.508
    vec_mlp vmax (64-64 relu)       err 3.40e-07 .. 1.20e-06   bound 3.25e-06 .. 3.64e-06   worst 0.370
    vec_mlp vmax, no bias           err 2.83e-07 .. 9.59e-07   bound 2.21e-06 .. 3.34e-06   worst 0.287
  fold_scale_inputs: within 1 ulp of the packed M diag(gate) at B 1 and B 5
  chain against the model at 2x12x30, 1x37x53, 2x5x7 (3 cases a row):
    mdta chain plain                err 5.58e-07 .. 1.15e-06   bound 2.58e-06 .. 4.03e-06   worst 0.293
    mdta chain aligned              err 6.60e-07 .. 1.51e-06   bound 2.64e-06 .. 8.36e-06   worst 0.250
    mdta chain negative             err 7.98e-07 .. 1.09e-06   bound 3.59e-06 .. 4.82e-06   worst 0.257
    mdta chain with a folded gate   err 6.44e-07               bound 2.12e-06               worst 0.304   (2x12x30)
    alignment chain plain           err 9.66e-07 .. 1.03e-06   bound 4.02e-06 .. 4.17e-06   worst 0.246
    alignment chain aligned         err 9.25e-07 .. 1.71e-06   bound 2.75e-06 .. 6.77e-06   worst 0.336
    alignment chain negative        err 9.65e-07 .. 1.53e-06   bound 3.82e-06 .. 6.10e-06   worst 0.256
Both gates' exponentials (vec_mlp: __expf through act_apply, align_fold: expf) stay inside the bound; no kernel was changed.
"""
import functools

import pytest
import torch

import fold_cases as FC

pytestmark = pytest.mark.gpu
H, W = FC.FOLD_HW
P = H * W


def _acts():
    from cdfo_amd import kernels as K
    return {"relu": K.ACT_RELU, "sigmoid": K.ACT_SIGMOID, None: K.ACT_NONE}


def _pack(M):
    """[B,64,Cin] float64 -> the packed 1x1 layout [B, 64 Cin] in float64, by kernels.pack_conv itself: packing permutes, so the
    fp32 head and the fp32 remainder of M are packed one after the other and added."""
    from cdfo_amd import kernels as K
    cin = M.shape[2]
    hi = M.float()
    lo = (M - hi.double()).float()
    rows = [K.pack_conv(hi[b].view(64, cin, 1, 1).cuda(), None).w.double() + K.pack_conv(lo[b].view(64, cin, 1, 1).cuda(), None).w.double()
            for b in range(M.shape[0])]
    return torch.stack(rows).cpu()


def _report(what, got, ref, tol):
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"{what}: err {err:.2e} bound {tol:.2e} ({err / tol:.3f}) max|ref| {ref.abs().max().item():.2e}")
    return err


# ------------------------------------------------------------------------------------------------------------ partials
@pytest.mark.parametrize("B,h,w", FC.PARTIAL_SHAPES)
def test_partials_of_integer_data_are_exact_slot_by_slot(B, h, w):
    """Every slot equals the sum over its own pixel range (float64 holds these integers exactly; fp32 too, in any order)."""
    from cdfo_amd import kernels as K
    n = K.nchunks_for(h * w)
    assert n == {1: 1, 2047: 1, 2048: 2, 2049: 2, 3077: 3, 132355: 128}.get(h * w, 1)
    for CH in (8, 16):
        q, k, _ = FC.gram_inputs("integer", CH, B, h, w)
        part, got_n = K.gram_partial(q.cuda(), k.cuda(), CH)
        assert got_n == n and tuple(part.shape) == (B, n, 64 * (CH + 2))
        assert torch.equal(part.cpu().double(), FC.split_partials(q, k, CH, n)[0]), CH
    x = FC.sum_inputs("integer", "x", B, h, w)
    part, got_n = K.chan_sum_partial(x.cuda())
    assert got_n == n and tuple(part.shape) == (B, n, 64)
    assert torch.equal(part.cpu().double(), FC.split_sums(x, n)[0])


def test_partials_of_channel_slices():
    """q, k and x as 64-channel slices of wider tensors (pitch 192 and 128), as _mdta and _rdab hand them out; the other
    channels hold other integers."""
    from cdfo_amd import kernels as K
    B, h, w = 3, 17, 181
    g = torch.Generator().manual_seed(17181)
    wide = torch.randint(-4, 5, (B, h, w, 192), generator=g).float()
    mid = torch.randint(-4, 5, (B, h, w, 128), generator=g).float()
    wd, md = wide.cuda(), mid.cuda()
    n = K.nchunks_for(h * w)
    assert n == 3
    for CH in (8, 16):
        for (qd, q), (kd, k) in (((wd[..., 64:128], wide[..., 64:128]), (md[..., 64:128], mid[..., 64:128])),
                                 ((md[..., 0:64], mid[..., 0:64]), (wd[..., 128:192], wide[..., 128:192]))):
            part, _ = K.gram_partial(qd, kd, CH)
            assert torch.equal(part.cpu().double(), FC.split_partials(q, k, CH, n)[0])
    for xd, x in ((wd[..., 128:192], wide[..., 128:192]), (md[..., 0:64], mid[..., 0:64])):
        part, _ = K.chan_sum_partial(xd)
        assert torch.equal(part.cpu().double(), FC.split_sums(x, n)[0])


@pytest.mark.parametrize("B,h,w", [(2, 37, 53), (1, 64, 64)])
def test_partials_of_fp32_data(B, h, w):
    from cdfo_amd import kernels as K
    n = K.nchunks_for(h * w)
    per = -(-h * w // n)
    unit = (per / 4 + 8) * 2.0 ** -24
    worst = {}
    for CH in (8, 16):
        q, k, _ = FC.gram_inputs("plain", CH, B, h, w)
        part, _ = K.gram_partial(q.cuda(), k.cuda(), CH)
        err = (part.cpu().double() - FC.split_partials(q, k, CH, n)[0]).abs()
        worst[f"gram{CH}"] = (err / (unit * FC.split_partials(q.abs(), k.abs(), CH, n)[0])).max().item()
    x = FC.sum_inputs("plain", "x", B, h, w)
    part, _ = K.chan_sum_partial(x.cuda())
    err = (part.cpu().double() - FC.split_sums(x, n)[0]).abs()
    worst["chan_sum"] = (err / (unit * FC.split_sums(x.abs(), n)[0])).max().item()
    print(f"fp32 partials {B}x{h}x{w} (n {n}, per {per}): error / bound " + ", ".join(f"{a} {r:.4f}" for a, r in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------ folds from synthetic partials
@functools.lru_cache(maxsize=None)
def _mdta_case(family, B, n, identity=False):
    q, k, t = FC.gram_inputs(family, 8, B, H, W)
    part = FC.split_partials(q, k, 8, n)[1]
    proj = torch.eye(64) if identity else FC.matrices()[0]
    ref = FC.mdta_matrix(part, t, proj)
    return part, t, proj, ref, FC.bound(ref, FC.mdta_matrix(part, t, proj, torch.float32))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("family", FC.FAMILIES)
@pytest.mark.parametrize("n", FC.SLOT_COUNTS)
def test_mdta_fold(n, family, B):
    from cdfo_amd import kernels as K
    part, t, proj, ref, tol = _mdta_case(family, B, n)
    args = (part.cuda(), n, t.cuda(), proj.cuda())
    fold = K.mdta_fold(*args)
    assert (fold.Cout, fold.Cin, fold.ks, fold.CoutP, fold.w_bstride) == (64, 64, 1, 64, 4096) and tuple(fold.w.shape) == (B, 4096)
    assert torch.equal(fold.w, K.mdta_fold(*args).w)
    err = _report(f"mdta_fold {family} n {n} B {B}", fold.w, _pack(ref), tol)
    assert err <= tol


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", FC.SLOT_COUNTS)
def test_mdta_fold_identity_projection_dead_rows(n, B):
    """proj = I: the packed matrix is blockdiag(attention) itself, and the rows of the two dead q channels are exactly 1/8."""
    from cdfo_amd import kernels as K
    part, t, proj, ref, tol = _mdta_case("dead", B, n, True)
    fold = K.mdta_fold(part.cuda(), n, t.cuda(), proj.cuda())
    err = _report(f"mdta_fold identity-proj dead n {n} B {B}", fold.w, _pack(ref), tol)
    assert err <= tol
    rows = torch.zeros(1, 64, 64, dtype=torch.float64)
    for c in (FC.DEAD_Q, FC.DEAD_BOTH):
        rows[0, c, c // 8 * 8:c // 8 * 8 + 8] = 1.0
    sel = _pack(rows)[0] == 1.0
    assert sel.sum().item() == 16 and (fold.w.cpu()[:, sel] == 0.125).all()


@functools.lru_cache(maxsize=None)
def _align_case(family, B, n):
    q, k, t = FC.gram_inputs(family, 16, B, H, W)
    gp = FC.split_partials(q, k, 16, n)[1]
    sw = FC.split_sums(FC.sum_inputs("gate", "warped", B, H, W), n)[1]
    sp = FC.split_sums(FC.sum_inputs("gate", "pred", B, H, W), n)[1]
    gate = FC.mlp_config("gate")
    du0, du2 = (gate[0], gate[1]), (gate[3], gate[4])
    proj, wf = FC.matrices()
    ref = FC.align_matrix(gp, sw, sp, P, t, du0, du2, proj, wf)
    return gp, sw, sp, t, du0, du2, ref, FC.bound(ref, FC.align_matrix(gp, sw, sp, P, t, du0, du2, proj, wf, torch.float32))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("family", FC.FAMILIES)
@pytest.mark.parametrize("n", FC.SLOT_COUNTS)
def test_align_fold(n, family, B):
    from cdfo_amd import kernels as K
    gp, sw, sp, t, du0, du2, ref, tol = _align_case(family, B, n)
    proj, wf = FC.matrices()
    args = (gp.cuda(), n, sw.cuda(), sp.cuda(), n, P, t.cuda(), du0[0].cuda(), du0[1].cuda(), du2[0].cuda(), du2[1].cuda(),
            proj.cuda(), wf.cuda())
    fold = K.align_fold(*args)
    assert (fold.Cout, fold.Cin, fold.ks, fold.CoutP, fold.w_bstride) == (64, 192, 1, 64, 192 * 64) and tuple(fold.w.shape) == (B, 192 * 64)
    assert torch.equal(fold.w, K.align_fold(*args).w)
    want = _pack(ref)
    err = _report(f"align_fold {family} n {n} B {B}", fold.w, want, tol)
    assert err <= tol
    third = torch.zeros(1, 64, 192, dtype=torch.float64)
    third[..., 128:] = 1.0
    sel = _pack(third)[0] == 1.0
    assert sel.sum().item() == 4096 and torch.equal(fold.w.cpu().double()[:, sel], want[:, sel])         # Wb: a copy


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", FC.SLOT_COUNTS)
@pytest.mark.parametrize("name", ["gate", "ca", "vmax", "vmax_nobias"])
def test_vec_mlp(name, n, B):
    from cdfo_amd import kernels as K
    w1, b1, act1, w2, b2, act2 = FC.mlp_config(name)
    part = FC.split_sums(FC.sum_inputs("gate", "x", B, H, W), n)[1]
    ref = FC.mlp(part, P, w1, b1, act1, w2, b2, act2)
    tol = FC.bound(ref, FC.mlp(part, P, w1, b1, act1, w2, b2, act2, dtype=torch.float32))
    dev = lambda t: None if t is None else t.cuda()      # noqa: E731
    A = _acts()
    args = (part.cuda(), n, P, dev(w1), dev(b1), w1.shape[0], A[act1], dev(w2), dev(b2), 0 if w2 is None else w2.shape[0], A[act2])
    out = K.vec_mlp(*args)
    assert tuple(out.shape) == tuple(ref.shape)
    assert torch.equal(out, K.vec_mlp(*args))
    err = _report(f"vec_mlp {name} n {n} B {B}", out, ref, tol)
    assert err <= tol


# ------------------------------------------------------------------------------------------------------------ fold_scale_inputs
def _random_fold(B, g):
    from cdfo_amd import kernels as K
    M = torch.randn(B, 64, 64, generator=g) / 8.0
    w = torch.stack([K.pack_conv(M[b].view(64, 64, 1, 1).cuda(), None).w for b in range(B)]).view(B, 4096).contiguous()
    return M, K.PackedConv(w, None, 64, 64, 1, 64, False, 4096)


def test_fold_scale_inputs():
    """M diag(gate) in the packed layout, to 1 ulp, for B = 1 and then B = 5 with the index table the first call cached."""
    from cdfo_amd import kernels as K
    K._FOLD_CIN.clear()
    g = torch.Generator().manual_seed(64)
    for B in (1, 5):
        M, fold = _random_fold(B, g)
        gate = torch.rand(B, 64, generator=g) + 0.01
        got = K.fold_scale_inputs(fold, gate.cuda())
        assert (got.Cout, got.Cin, got.ks, got.CoutP, got.w_bstride) == (64, 64, 1, 64, 4096)
        want = _pack(M.double() * gate.double().unsqueeze(1))
        w32 = want.float().abs()
        ulp = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()
        excess = ((got.w.cpu().double() - want).abs() - ulp).max().item()
        print(f"fold_scale_inputs B {B}: max(|got - want| - ulp) {excess:.2e}")
        assert excess <= 0.0
        assert len(K._FOLD_CIN) == 1
    for bad in (torch.rand(5, 32), torch.rand(4, 64), torch.rand(64)):
        with pytest.raises(ValueError):
            K.fold_scale_inputs(fold, bad.cuda())


# ------------------------------------------------------------------------------------------------------------ the chain
CHAIN_SHAPES = [(2, 12, 30), (1, 37, 53), (2, 5, 7)]
CHAIN_FAMILIES = ["plain", "aligned", "negative"]


@pytest.mark.parametrize("family", CHAIN_FAMILIES)
@pytest.mark.parametrize("B,h,w", CHAIN_SHAPES)
def test_mdta_chain_against_the_model(B, h, w, family):
    """gram_partial -> mdta_fold -> conv(v, fold) against project_out(_channel_attention(q, k, v)) in float64."""
    from cdfo_amd import kernels as K
    q, k, t = FC.gram_inputs(family, 8, B, h, w)
    v = FC.sum_inputs(family, "v", B, h, w)
    proj, _ = FC.matrices()
    ref = FC.mdta_model(q, k, v, t, proj)
    tol = FC.bound(ref, FC.mdta_model(q, k, v, t, proj, torch.float32))
    part, n = K.gram_partial(q.cuda(), k.cuda(), 8)
    fold = K.mdta_fold(part, n, t.cuda(), proj.cuda())
    out = K.conv(v.cuda(), fold, prec=K.PREC_F32)
    err = _report(f"mdta chain {family} {B}x{h}x{w}", out, ref, tol)
    assert err <= tol


def test_mdta_chain_with_a_folded_gate():
    """... -> fold_scale_inputs(fold, gate) -> conv against project_out(attention(q, k, v * gate))."""
    from cdfo_amd import kernels as K
    B, h, w = 2, 12, 30
    q, k, t = FC.gram_inputs("plain", 8, B, h, w)
    v = FC.sum_inputs("plain", "v", B, h, w)
    gate = torch.rand(B, 64, generator=torch.Generator().manual_seed(12)) + 0.01
    proj, _ = FC.matrices()
    gated = v.double() * gate.double().view(B, 1, 1, 64)
    ref = FC.mdta_model(q, k, gated, t, proj)
    tol = FC.bound(ref, FC.mdta_model(q, k, gated, t, proj, torch.float32))
    part, n = K.gram_partial(q.cuda(), k.cuda(), 8)
    fold = K.fold_scale_inputs(K.mdta_fold(part, n, t.cuda(), proj.cuda()), gate.cuda())
    out = K.conv(v.cuda(), fold, prec=K.PREC_F32)
    err = _report(f"mdta chain with gate {B}x{h}x{w}", out, ref, tol)
    assert err <= tol


@pytest.mark.parametrize("family", CHAIN_FAMILIES)
@pytest.mark.parametrize("B,h,w", CHAIN_SHAPES)
def test_alignment_chain_against_the_model(B, h, w, family):
    """kf = relu(fusion_out.0([warped, pred])); gram_partial(x, kf) + two chan_sum_partial -> align_fold -> conv([warped, pred, x],
    fold, relu) against the oracle's lines of dual_att_alignment in float64."""
    from cdfo_amd import kernels as K
    x, warped, pred, t = FC.align_inputs(family, B, h, w)
    gate = FC.mlp_config("gate")
    du0, du2 = (gate[0], gate[1]), (gate[3], gate[4])
    proj, wf = FC.matrices()
    ref, _ = FC.align_model(x, warped, pred, t, du0, du2, proj, wf)
    tol = FC.bound(ref, FC.align_model(x, warped, pred, t, du0, du2, proj, wf, torch.float32)[0])
    xd, wd, pd, wfd = x.cuda(), warped.cuda(), pred.cuda(), wf.cuda()
    kf = K.conv([wd, pd], K.pack_conv(wfd.view(64, 128, 1, 1), None), act=K.ACT_RELU, prec=K.PREC_F32)
    gp, ng = K.gram_partial(xd, kf, 16)
    sw, ns = K.chan_sum_partial(wd)
    sp, _ = K.chan_sum_partial(pd)
    fold = K.align_fold(gp, ng, sw, sp, ns, h * w, t.cuda(), du0[0].cuda(), du0[1].cuda(), du2[0].cuda(), du2[1].cuda(),
                        proj.cuda(), wfd)
    out = K.conv([wd, pd, xd], fold, act=K.ACT_RELU, prec=K.PREC_F32)
    err = _report(f"alignment chain {family} {B}x{h}x{w}", out, ref, tol)
    assert err <= tol


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from cdfo_amd import kernels as K
    q, k, _ = FC.gram_inputs("plain", 8, 2, 12, 30)
    with pytest.raises(K.CdfoError):
        K.gram_partial(q.cuda(), k.cuda(), 12)
    part = FC.split_sums(FC.sum_inputs("gate", "x", 1, H, W), 1)[1].cuda()
    w1 = torch.zeros(65, 64).cuda()
    with pytest.raises(K.CdfoError):
        K.vec_mlp(part, 1, P, w1, None, 65, K.ACT_RELU)
    torch.cuda.synchronize()
