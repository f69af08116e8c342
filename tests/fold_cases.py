"""Inputs, float64 references and bounds of the channel-attention statistics and fold tests (gram_partial, chan_sum_partial,
mdta_fold, align_fold, vec_mlp, fold_scale_inputs).

A plain helper module: tests/test_gpu_folds.py runs the kernels on what is built here, tests/test_fold_cases_cpu.py checks,
without a GPU, that the fold identity behind the kernels holds and that these very inputs would catch a defective fold.
Everything is seeded and computed on the CPU; cached tensors must be left unchanged by their users.

Conventions.  Activations are pixel-major [B,H,W,64].  A Gram partial slot is [64][CH+2] (CH channels per head):
j < CH: sum_p q[p][c] k[p][head(c) CH + j], j == CH: sum q[p][c]^2, j == CH+1: sum k[p][c]^2; a channel-sum slot is [64].
Slot c of n covers the pixels [c per, min(P, (c+1) per)), per = ceil(P / n) -- the kernels' chunking; a slot past the last
pixel is all zeros."""
import functools
import zlib

import torch
import torch.nn.functional as F

HEADS = {8: 8, 16: 4}                                       # channels per head -> heads (MDTA: 8 x 8, DualAttAlignment: 4 x 16)
FAMILIES = ("plain", "dead", "aligned", "hot", "negative", "tiny")       # the fp32 families (`integer` stands apart)
TEMP_FACTOR = {"hot": 30.0, "negative": -10.0}
DEAD_K, DEAD_BOTH, DEAD_Q = 5, 9, 20                        # `dead`: k channel zero / q and k zero / q channel zero
SLOT_COUNTS = (1, 7, 8, 9, 128, 304)                        # around the reduction loop's unroll of 8, the cap of nchunks_for, beyond
FOLD_HW = (37, 53)                                          # P = 1961: no power of two, no multiple of any slot count above 1
# (B, H, W) of the exact partial tests: P below 4 and below 16, the ragged tails of the 4- and 32-pixel strides, P = 1024 n +- 1
# around the slot-count steps of nchunks_for, three slots, and the cap at 128 slots
PARTIAL_SHAPES = ((2, 1, 1), (2, 1, 3), (2, 3, 5), (2, 4, 4), (2, 1, 17), (2, 1, 31), (2, 3, 11), (2, 31, 33), (2, 32, 32),
                  (2, 23, 89), (2, 32, 64), (2, 3, 683), (2, 17, 181), (1, 257, 515))
DEFECTS = ("transpose", "roll_temperature", "swap_norms", "clamp_1e-6")      # of the attention itself (all folds)
ALIGN_DEFECTS = ("swap_gates", "wb_from_wa")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def gram_inputs(family, CH, B, H, W):
    """(q, k, temperature): fp32 [B,H,W,64] twice and [heads].  Channel scales run 0.5 .. 2 on q and 2 .. 0.5 on k, the
    temperatures 0.5 .. 1.5 over the heads: no two channels and no two heads are interchangeable."""
    g = _gen("gram", family, CH, B, H, W)
    shape = (B, H, W, 64)
    if family == "integer":        # every sum of products stays below 2^24: fp32 partials are exact in any summation order
        top = 4 if H * W <= 4096 else 2
        q = torch.randint(-top, top + 1, shape, generator=g).float()
        k = torch.randint(-top, top + 1, shape, generator=g).float()
    else:
        scale = torch.linspace(0.5, 2.0, 64)
        q = torch.randn(shape, generator=g) * scale
        if family in ("aligned", "hot"):
            k = q + 0.05 * torch.randn(shape, generator=g)
        else:
            k = torch.randn(shape, generator=g) * scale.flip(0)
        if family == "dead":
            k[..., DEAD_K] = 0.0
            q[..., DEAD_BOTH] = 0.0
            k[..., DEAD_BOTH] = 0.0
            q[..., DEAD_Q] = 0.0
        if family == "tiny":       # norms of 2e-7 .. 2e-6 |P = 1961|: above the 1e-12 clamp, around a clamp of 1e-6
            q, k = q * 1e-8, k * 1e-8
    t = torch.linspace(0.5, 1.5, HEADS[CH]) * TEMP_FACTOR.get(family, 1.0)
    return q, k, t


@functools.lru_cache(maxsize=None)
def sum_inputs(family, which, B, H, W):
    """x [B,H,W,64] for the channel sums: noise on a per-image, per-channel offset of order 1, so that the means differ
    between channels and between images (`which` tells the operands of one case apart)."""
    g = _gen("sum", family, which, B, H, W)
    if family == "integer":
        top = 4 if H * W <= 4096 else 2
        return torch.randint(-top, top + 1, (B, H, W, 64), generator=g).float()
    return torch.randn(B, H, W, 64, generator=g) * torch.linspace(0.5, 2.0, 64) + torch.randn(B, 1, 1, 64, generator=g)


@functools.lru_cache(maxsize=None)
def matrices():
    """(proj [64,64], wf [64,128]): random, non-symmetric, every row different."""
    g = _gen("matrices")
    return torch.randn(64, 64, generator=g) / 8.0, torch.randn(64, 128, generator=g) / 128 ** 0.5


@functools.lru_cache(maxsize=None)
def mlp_config(name):
    """(w1, b1, act1, w2, b2, act2) of the gate family: pre-sigmoid values span about +-8 on the means of sum_inputs.
    gate: DualAttAlignment / MVDualAttAlignment conv_du (64 -> 4 relu -> 64 sigmoid); ca: CALayer (64 -> 64 relu -> 64
    sigmoid); vmax / vmax_nobias: one layer 64 -> 64 relu (the prior-fusion attention's vmax)."""
    g = _gen("mlp", name)
    if name == "gate":
        return (torch.randn(4, 64, generator=g) / 8.0, torch.randn(4, generator=g) * 0.5, "relu",
                torch.randn(64, 4, generator=g) * 3.0, torch.randn(64, generator=g), "sigmoid")
    if name == "ca":
        return (torch.randn(64, 64, generator=g) / 8.0, torch.randn(64, generator=g) * 0.5, "relu",
                torch.randn(64, 64, generator=g) * 0.75, torch.randn(64, generator=g), "sigmoid")
    w1, b1 = torch.randn(64, 64, generator=g) / 8.0, torch.randn(64, generator=g) * 0.5
    return (w1, b1 if name == "vmax" else None, "relu", None, None, None)


# ------------------------------------------------------------------------------------------------------------ partials
def _slots(t, n):
    """[B,P,C] -> [B,n,per,C], zero padded: slot c holds the pixels [c per, min(P, (c+1) per))"""
    B, P, C = t.shape
    per = -(-P // n)
    pad = torch.zeros(B, n * per - P, C, dtype=t.dtype)
    return torch.cat([t, pad], 1).view(B, n, per, C)


def split_partials(q, k, CH, n):
    """(float64, fp32) Gram partials [B,n,64 (CH+2)] of q, k [B,H,W,64] in n slots.  The fp32 set is the float64 one
    rounded: the best fp32 partials there are, for a fold to consume."""
    B, heads = q.shape[0], 64 // CH
    qs, ks = _slots(q.double().reshape(B, -1, 64), n), _slots(k.double().reshape(B, -1, 64), n)
    per = qs.shape[2]
    G = torch.einsum("bnphc,bnphj->bnhcj", qs.view(B, n, per, heads, CH), ks.view(B, n, per, heads, CH))
    part = torch.cat([G.reshape(B, n, 64, CH), qs.pow(2).sum(2).unsqueeze(-1), ks.pow(2).sum(2).unsqueeze(-1)], -1)
    part = part.reshape(B, n, 64 * (CH + 2)).contiguous()
    return part, part.float()


def split_sums(x, n):
    """(float64, fp32) channel-sum partials [B,n,64] of x [B,H,W,64] in n slots."""
    part = _slots(x.double().reshape(x.shape[0], -1, 64), n).sum(2).contiguous()
    return part, part.float()


def sum_slots(part):
    """The folds' reduction: slots added in index order, in the partials' own precision."""
    s = part[:, 0].clone()
    for ch in range(1, part.shape[1]):
        s = s + part[:, ch]
    return s


# ------------------------------------------------------------------------------------------------------------ folds
def attention(part, temperature, CH, dtype=torch.float64, defect=None):
    """blockdiag(softmax_j(G[c][j] / (max(|q_c|, 1e-12) max(|k_j|, 1e-12)) t_head)) [B,64,64] from Gram partials, evaluated in
    `dtype` (float64: the reference; float32: the restatement that sets the scale of the bounds).  defect: one of DEFECTS,
    a mistake such a kernel makes -- for the sensitivity test only."""
    heads = 64 // CH
    s = sum_slots(part).to(dtype).view(-1, 64, CH + 2)
    B = s.shape[0]
    eps = 1e-6 if defect == "clamp_1e-6" else 1e-12
    nq, nk = s[..., CH].sqrt().clamp_min(eps), s[..., CH + 1].sqrt().clamp_min(eps)
    if defect == "swap_norms":
        nq, nk = nk, nq
    t = temperature.to(dtype).reshape(heads)
    if defect == "roll_temperature":
        t = t.roll(1)
    G = s[..., :CH].reshape(B, heads, CH, CH)
    A = (G / (nq.view(B, heads, CH, 1) * nk.view(B, heads, 1, CH)) * t.view(1, heads, 1, 1)).softmax(-1)
    if defect == "transpose":
        A = A.transpose(-1, -2)
    full = torch.zeros(B, 64, 64, dtype=dtype)
    for h in range(heads):
        full[:, h * CH:(h + 1) * CH, h * CH:(h + 1) * CH] = A[:, h]
    return full


def mdta_matrix(part, temperature, proj, dtype=torch.float64, defect=None):
    """M [B,64,64] = proj . blockdiag(attention): attn @ v followed by project_out as ONE matrix per image.  The channels
    per head follow from the partials' width."""
    CH = part.shape[-1] // 64 - 2
    return proj.to(dtype) @ attention(part, temperature, CH, dtype, defect)


def _act(x, name):
    return torch.relu(x) if name == "relu" else torch.sigmoid(x) if name == "sigmoid" else x


def mlp_preact(part, P, w1, b1, act1, w2=None, b2=None, act2=None, dtype=torch.float64):
    """The last layer's pre-activation of `mlp`, [B,c]."""
    a = (sum_slots(part).to(dtype) / P) @ w1.to(dtype).t()
    if b1 is not None:
        a = a + b1.to(dtype)
    if w2 is None:
        return a
    a = _act(a, act1) @ w2.to(dtype).t()
    return a if b2 is None else a + b2.to(dtype)


def mlp(part, P, w1, b1, act1, w2=None, b2=None, act2=None, dtype=torch.float64):
    """act2(W2 act1(W1 mean + b1) + b2) [B,c] from channel-sum partials (second layer optional)."""
    return _act(mlp_preact(part, P, w1, b1, act1, w2, b2, act2, dtype), act1 if w2 is None else act2)


def align_matrix(gpart, sw, sp, P, temperature, du0, du2, proj, wf, dtype=torch.float64, defect=None):
    """[B,64,192] = [Wa P A diag(g1) | Wa P A diag(g2) | Wb]: Wa = wf[:, :64], Wb = wf[:, 64:], A the 4 x 16 attention,
    g1 / g2 = sigmoid(du2(relu(du0(mean)))) of the warped / predicted frame's channel means; du0, du2: (weight, bias)."""
    A = attention(gpart, temperature, 16, dtype, defect if defect in DEFECTS else None)
    g1 = mlp(sw, P, du0[0], du0[1], "relu", du2[0], du2[1], "sigmoid", dtype)
    g2 = mlp(sp, P, du0[0], du0[1], "relu", du2[0], du2[1], "sigmoid", dtype)
    if defect == "swap_gates":
        g1, g2 = g2, g1
    wf = wf.to(dtype)
    R = wf[:, :64] @ proj.to(dtype) @ A
    Wb = wf[:, :64] if defect == "wb_from_wa" else wf[:, 64:]
    return torch.cat([R * g1.unsqueeze(1), R * g2.unsqueeze(1), Wb.expand(R.shape[0], 64, 64)], -1)


def bound(ref, restated):
    """The folds' and the chain's bound, absolute: max(4 x the error of the fp32 restatement, 2^-20 max|ref|).  4 x is this
    project's rule for the same products in another fp32 order and with other library functions (test_gpu_align_stats.py);
    the floor is a 16-term dot product of rounded terms, 16 x 2^-24."""
    return max(4.0 * (restated.double() - ref).abs().max().item(), 2.0 ** -20 * ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------ the model's own definition
def _nchw(t, dtype):
    return t.to(dtype).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def mdta_model(q, k, v, temperature, proj, dtype=torch.float64):
    """project_out(attention(q, k, v)) by the oracle's own _channel_attention, [B,H,W,64]: no partials, no folded matrix."""
    from oracle.cvsr_v8_ref import _channel_attention
    heads = temperature.numel()
    o = _channel_attention(_nchw(q, dtype), _nchw(k, dtype), _nchw(v, dtype), heads, temperature.to(dtype).view(heads, 1, 1))
    return _nhwc(F.conv2d(o, proj.to(dtype).view(64, 64, 1, 1)))


def align_model(x, warped, pred, temperature, du0, du2, proj, wf, dtype=torch.float64):
    """oracle.cvsr_v8_ref.dual_att_alignment from k = fusion_out(cat[warped, pred]) to out = fusion_out(cat[o1 + o2, x]),
    `warped` given (no flow_warp): returns (out, k), both [B,H,W,64]."""
    from oracle.cvsr_v8_ref import _channel_attention, _conv
    p = "MV_deform_align."
    sd = {p + "conv_du.0.weight": du0[0].view(4, 64, 1, 1), p + "conv_du.0.bias": du0[1],
          p + "conv_du.2.weight": du2[0].view(64, 4, 1, 1), p + "conv_du.2.bias": du2[1],
          p + "project_out.weight": proj.view(64, 64, 1, 1), p + "fusion_out.0.weight": wf.view(64, 128, 1, 1),
          p + "temperature": temperature.view(4, 1, 1)}
    sd = {key: val.to(dtype) for key, val in sd.items()}
    x, warped, pred = _nchw(x, dtype), _nchw(warped, dtype), _nchw(pred, dtype)

    def gate(z):  # conv_du(avg_pool(z))
        y = z.mean((2, 3), keepdim=True)
        y = F.relu(_conv(sd, p + "conv_du.0", y))
        return torch.sigmoid(_conv(sd, p + "conv_du.2", y))

    def fusion_out(z):
        return F.relu(_conv(sd, p + "fusion_out.0", z))

    k = fusion_out(torch.cat([warped, pred], 1))
    temp = sd[p + "temperature"]
    o1 = _conv(sd, p + "project_out", _channel_attention(x, k, warped * gate(warped), 4, temp))
    o2 = _conv(sd, p + "project_out", _channel_attention(x, k, pred * gate(pred), 4, temp))
    out = fusion_out(torch.cat([o1 + o2, x], 1))
    return _nhwc(out), _nhwc(k)


@functools.lru_cache(maxsize=None)
def align_inputs(family, B, H, W):
    """(x, warped, pred, temperature) of one alignment case, fp32.  The keys are kf = relu(wf [warped, pred]), so the family
    is made on the query side: `aligned` / `hot` take x = kf + 0.05 noise, `dead` zeroes two channels of x, `tiny` scales
    all three operands by 1e-8."""
    g = _gen("align", family, B, H, W)
    warped, pred = sum_inputs(family, "warped", B, H, W), sum_inputs(family, "pred", B, H, W)
    if family == "tiny":
        warped, pred = warped * 1e-8, pred * 1e-8
    if family in ("aligned", "hot"):
        kf = torch.relu(torch.cat([warped, pred], -1) @ matrices()[1].t())
        x = kf + 0.05 * torch.randn(B, H, W, 64, generator=g)
    else:
        x = torch.randn(B, H, W, 64, generator=g) * torch.linspace(0.5, 2.0, 64)
    if family == "dead":
        x[..., [DEAD_BOTH, DEAD_Q]] = 0.0
    if family == "tiny":
        x = x * 1e-8
    return x, warped, pred, torch.linspace(0.5, 1.5, 4) * TEMP_FACTOR.get(family, 1.0)
