"""Inputs, fp64 references and tolerances of the prior-fusion attention tests (rdab_prep, colconv9, seq_attn).

A plain helper module: tests/test_gpu_attention.py runs the kernels on what is built here, tests/test_attention_cases_cpu.py
checks, without a GPU, that these very inputs and tolerances would catch a defective kernel.  Everything is seeded and
computed on the CPU; references are cached and must be left unchanged by their users."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

# key counts of the row / column attention tests (the other spatial dimension is OTHER, B = 2)
SEQ_LENGTHS = (1, 8, 33, 36, 37, 136, 168, 272, 300, 400, 480, 490)
OTHER = 3
FAMILIES = {"spread": (0.15, 0.0), "peaked": (0.5, 0.0), "offset": (0.15, 0.5)}       # q = scale * randn + shift, v = randn
WINDOW_SHAPES = ((8, 8), (16, 40), (40, 136), (136, 72), (24, 8))


# ------------------------------------------------------------------------------------------------------------ seq_attn
def seq_shape(mode, L):
    """(H, W) that puts L keys on the sequence axis of `mode` (0 / 20 / 10: rows, 1 / 21 / 11: columns)."""
    return (OTHER, L) if mode % 10 == 0 else (L, OTHER)


def to_sequences(t, mode):
    """[B,H,W,C] -> [..., L, C] with one sequence per leading index (mode % 10 = 0: rows, 1: columns, 2: 8x8 windows)."""
    B, H, W, C = t.shape
    if mode % 10 == 0:
        return t
    if mode % 10 == 1:
        return t.transpose(1, 2)
    return t.reshape(B, H // 8, 8, W // 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 8, W // 8, 64, C)


def from_sequences(o, mode, shape):
    B, H, W, C = shape
    if mode % 10 == 0:
        return o
    if mode % 10 == 1:
        return o.transpose(1, 2)
    return o.reshape(B, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def seq_ref(q, v, mode):
    """softmax(Q Q^T) V in fp64 and, beside it, softmax(Q Q^T) |V| (the PV1 bound needs it); both [B,H,W,C]."""
    qs, vs = to_sequences(q.double(), mode), to_sequences(v.double(), mode)
    p = (qs @ qs.transpose(-1, -2)).softmax(-1)
    return (from_sequences(p @ vs, mode, q.shape).contiguous(), from_sequences(p @ vs.abs(), mode, q.shape).contiguous())


def seq_len(mode, H, W):
    return W if mode % 10 == 0 else (H if mode % 10 == 1 else 64)


@functools.lru_cache(maxsize=None)
def seq_case(family, mode10, B, H, W):
    """(q, v, ref, pav) of one seeded case; mode10 = mode % 10, so the MFMA, PV1 and VALU forms share inputs and reference."""
    scale, shift = FAMILIES[family]
    seed = (sorted(FAMILIES).index(family) * 3 + mode10) * 1000003 + (B * 1009 + H) * 1013 + W
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, W, 64, generator=g) * scale + shift
    v = torch.randn(B, H, W, 64, generator=g)
    ref, pav = seq_ref(q, v, mode10)
    return q, v, ref, pav


LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)     # the kernel's fp32 constant


def snap_to_fp16_ties(q):
    """Move every element of q (fp32) to a nearby value whose fp32 product with log2 e lies EXACTLY half way between two fp16
    numbers, where one exists within two fp32 steps (most do).  The MFMA kernel scales its queries by log2 e and splits the
    product into fp16 hi + fp16 lo; on a tie the rounding of hi is decided by the tie rule alone, and a kernel that derives hi
    twice (once from the exact product, once from the fp32 one) gets two different answers there."""
    x = q * LOG2E
    h = x.half().float()
    ulp = torch.exp2(torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -14))) - 10)
    mid = h + 0.5 * ulp * torch.sign(x)                     # 12 significant bits: exact in fp32
    best = (mid.double() / LOG2E.double()).float()
    out = best.clone()
    found = torch.zeros_like(q, dtype=torch.bool)
    for steps in (0, 1, -1, 2, -2):
        cand = best.clone()
        for _ in range(abs(steps)):
            cand = torch.nextafter(cand, torch.full_like(cand, math.copysign(math.inf, steps)))
        hit = (cand * LOG2E == mid) & ~found
        out[hit] = cand[hit]
        found |= hit
    return out, found


@functools.lru_cache(maxsize=None)
def tie_case(mode10, B, H, W):
    """The `offset` case of this shape (the larger the elements, the larger an fp16 ulp of theirs) with its queries snapped to
    fp16 ties: (q, v, ref, pav, share of tie elements)."""
    q, v, _, _ = seq_case("offset", mode10, B, H, W)
    q, found = snap_to_fp16_ties(q)
    ref, pav = seq_ref(q, v, mode10)
    return q, v, ref, pav, found.float().mean().item()


def tol_three_pass(ref):
    """The project's rule for fp32-grade results (split-fp16 x 3 passes, VALU fp32): max|out - ref| < 2e-5 max(1, max|ref|)."""
    return 2e-5 * max(1.0, ref.abs().max().item())


def bound_pv1(ref, pav, L, vmax):
    """Elementwise bound of modes 20 / 21 / 22 (PV1: the second product on single-fp16 operands):

        |out - ref|[i,c] <= 2^-10 (p @ |v|)[i,c] + L 2^-24 max|v| + tol_three_pass(ref)

    Derivation from the kernel's arithmetic.  The scores keep their three split-fp16 passes and the sums are fp32, which is
    what the three-pass tolerance (`base`) pays for.  PV1 adds: every probability p_j = exp2(s_j - m) in [0, 1] and every value
    v_j is rounded ONCE to fp16 before the product, 2^-11 relative each (10 stored mantissa bits, round to nearest), so a term
    p_j v_j is off by at most ((1 + 2^-11)^2 - 1) |p_j v_j| ~ 2^-10 |p_j v_j|; after the division by l = sum_j p_j the terms
    add up to 2^-10 sum_j softmax_j |v_j| = 2^-10 (p @ |v|).  The relative bound fails only below fp16's normal range:
    a probability under 2^-14 is rounded on the subnormal grid (step 2^-24) or lost altogether, an absolute error of at most
    2^-24 per key, times |v_j| <= max|v|, and l >= 1 (the key that holds the running maximum has p = 1): L 2^-24 max|v| for the
    L keys.  (A probability is rounded relative to the running maximum of its stage and scaled down afterwards in fp32, which
    only shrinks that absolute error.)  Nothing here was fitted to a GPU result."""
    return 2.0 ** -10 * pav + (L * 2.0 ** -24 * vmax + tol_three_pass(ref))


def seq_ratio(out, ref, pav, mode, L, vmax):
    """Largest error / tolerance of a seq_attn result (a pass is < 1): the three-pass rule, or the PV1 bound for modes 20-22."""
    err = (out.double() - ref).abs()
    if 20 <= mode <= 22:
        return (err / bound_pv1(ref, pav, L, vmax)).max().item()
    return err.max().item() / tol_three_pass(ref)


# ------------------------------------------------------------------------------------------------------------ rdab_prep
RDAB_SHAPES = ((3, 8, 40), (2, 16, 24), (5, 8, 8), (1, 8, 8))
RAISED = (0, 7, 63)     # channels whose vmax is lifted: the channel conv's zero padding meets masked values at both ends


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def rdab_inputs(B, H, W, seed=0):
    """xq [B,H,W,128] (q | v), vmax [B,64], u [B,64,H,W] on the kernel's grid (k + 0.5) 2^-24, the 9 taps and the bias."""
    g = torch.Generator().manual_seed(7919 * seed + (B * 131 + H) * 137 + W)
    xq = torch.randn(B, H, W, 128, generator=g)
    vmax = 3.0 * torch.rand(B, 64, generator=g)
    vmax[:, list(RAISED)] += 3.0 + 2.0 * torch.rand(B, len(RAISED), generator=g)
    # the fp32 sum k + 0.5 rounds to even from k = 2^23 on, exactly as the kernel's does; k = 2^24 - 1 would round to u = 1
    k = torch.randint(0, (1 << 24) - 1, (B, 64, H, W), generator=g)
    u = ((k.double() + 0.5) * 2.0 ** -24).float()
    wW = torch.randn(1, 1, 1, 9, generator=g) * 0.4
    bW = torch.randn(1, generator=g)
    return xq, vmax, u, wW, bW


def gumbel_softmax64(vmax, u):
    """softmax_c(vmax + G), G = -log(-log u), in fp64: the quantity gumbel_hard_mask thresholds.  [B,64,H,W]."""
    B = vmax.shape[0]
    return (vmax.double().view(B, 64, 1, 1) - (-u.double().log()).log()).softmax(1)


def chan_conv9(x, w, b):
    """Zero-padded 9-tap cross-correlation over the channel axis of an NHWC tensor (arch.py:2216-2219), in x's precision."""
    B, H, W, C = x.shape
    y = F.conv2d(x.reshape(B * H, 1, W, C), w.to(x.dtype), b.to(x.dtype), padding=(0, 4))
    return y.reshape(B, H, W, C)


def rdab_ref(xq, vmax, u, wW, bW, threshold=None, flip_taps=False):
    """fp64 reference of rdab_prep: {"mask", "qwin", "sq", "vrow"}, all [B,H,W,64].  threshold / flip_taps build DEFECTIVE
    variants for the sensitivity test (a threshold other than 0.5, the 9 taps reversed); the reference leaves both alone."""
    from oracle.cvsr_v8_ref import gumbel_hard_mask
    B, H, W, _ = xq.shape
    if threshold is None:
        mask = gumbel_hard_mask(vmax.double().view(B, 64, 1, 1).expand(B, 64, H, W), u.double())
    else:
        mask = (gumbel_softmax64(vmax, u) >= threshold).double()
    mask = nhwc(mask)
    q, v = xq[..., :64].double(), xq[..., 64:].double()
    w = wW.double().flip(-1) if flip_taps else wW.double()
    return {"mask": mask, "qwin": (1.0 - mask) * q, "sq": chan_conv9(mask * q, w, bW.double()),
            "vrow": chan_conv9(v, w, bW.double())}


def rdab_tie_distance(vmax, u):
    """min |softmax - 0.5| in fp64: the kernel decides w_c >= 0.5 sum w in fp32, so an exact mask may only be demanded of
    inputs that keep clear of the threshold (the tests assert > 1e-5 first)."""
    return (gumbel_softmax64(vmax, u) - 0.5).abs().min().item()


def tol_conv9(ref):
    """A 9-term fp32 sum: 1e-5 max(1, max|ref|), the depthwise-conv tolerance of test_gpu_attention.py."""
    return 1e-5 * max(1.0, ref.abs().max().item())


def rdab_check(sq, vrow, qwin, want):
    """The checks of an rdab_prep result against rdab_ref's dict.  The mask is recovered as qwin == 0 (the inputs have no
    zero q) and must match EXACTLY, no element excluded; sq and vrow within tol_conv9.  Returns
    {"mask_mismatches": count, "qwin": max abs error, "sq": err / tol, "vrow": err / tol}; rdab_assert asserts on them."""
    got_mask = (qwin == 0).double()
    return {"mask_mismatches": int((got_mask != want["mask"]).sum().item()),
            "qwin": (qwin.double() - want["qwin"]).abs().max().item(),
            "sq": (sq.double() - want["sq"]).abs().max().item() / tol_conv9(want["sq"]),
            "vrow": (vrow.double() - want["vrow"]).abs().max().item() / tol_conv9(want["vrow"])}


def rdab_assert(sq, vrow, qwin, want):
    r = rdab_check(sq, vrow, qwin, want)
    print(f"rdab_prep: mask mismatches {r['mask_mismatches']}, sq {r['sq']:.3f} vrow {r['vrow']:.3f} of the tolerance")
    assert r["mask_mismatches"] == 0, r
    assert r["qwin"] == 0.0, r            # (1 - mask) * q with mask in {0, 1}: q or 0, exactly
    assert r["sq"] < 1.0 and r["vrow"] < 1.0, r
    return r


# Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written from the paper:
# ten rounds of  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key bumped by the
# Weyl constants between rounds.  Counters / keys are arrays of uint32 values (any common shape).
_PH_M0, _PH_M1, _PH_W0, _PH_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) & _M32 for a in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_PH_M0) * c0, np.uint64(_PH_M1) * c2           # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(_PH_W0)) & _M32, (k1 + np.uint64(_PH_W1)) & _M32
    return c0, c1, c2, c3


# Random123's known-answer vectors for philox4x32-10 (kat_vectors): (counter, key, result)
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def rdab_noise(B, P, seed, draw):
    """The generator contract of numeric.h between inference and training: u[b,c,p] = ((word >> 8) + 0.5) 2^-24 with word
    c & 3 of Philox4x32-10(counter = (p, b, c >> 2, draw), key = (seed low 32, seed high 32)).  fp32 [B,64,P]."""
    b = np.arange(B, dtype=np.uint64).reshape(B, 1, 1)
    j = np.arange(16, dtype=np.uint64).reshape(1, 16, 1)
    p = np.arange(P, dtype=np.uint64).reshape(1, 1, P)
    words = philox4x32_10(p, b, j, np.uint64(draw), np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF))
    w = np.stack([np.broadcast_to(x, (B, 16, P)) for x in words], axis=2).reshape(B, 64, P)     # channel = 4 j + word
    u = ((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return torch.from_numpy(u.astype(np.float32))          # one rounding of k + 0.5 to fp32, as in the kernel's fp32 sum


# ------------------------------------------------------------------------------------------------------------ colconv9
COL_HEIGHTS = (1, 4, 5, 33, 34, 35, 68, 69, 100)      # both image edges' halo rows and the seams of the 34-row segments


@functools.lru_cache(maxsize=None)
def col_weights():
    g = torch.Generator().manual_seed(4)
    return torch.randn(1, 1, 9, 1, generator=g) * 0.4, torch.randn(1, generator=g)


def col_ref(x, w, b):
    """directH1_conv (arch.py:2225) on an NHWC tensor in fp64: [(b w), 1, h, c], the (9,1) kernel slides over h, zero padded."""
    B, H, W, C = x.shape
    z = x.double().permute(0, 2, 1, 3).reshape(B * W, 1, H, C)
    y = F.conv2d(z, w.double(), b.double(), padding=(4, 0))
    return y.reshape(B, W, H, C).permute(0, 2, 1, 3).contiguous()


def col_ref_taps(x, w, b):
    """The same as a sum of shifted rows, tap by tap: for tensors too large for the conv2d form (few rows, very many columns)."""
    B, H, W, C = x.shape
    xd, wd = x.double(), w.double().reshape(9)
    out = torch.full((B, H, W, C), b.double().item(), dtype=torch.float64)
    for t in range(9):                                   # out[y] += w[t] x[y + t - 4]
        lo, hi = max(0, 4 - t), min(H, H + 4 - t)
        if lo < hi:
            out[:, lo:hi] += wd[t] * xd[:, lo + t - 4:hi + t - 4]
    return out


# ---------------------------------------------------------------------------------- defective emulations (sensitivity test)
def seq_ref_unmasked_tail(q, v, mode):
    """Defect (i): the last 32-key sub-tile's masked keys left in.  The kernel loads them clamped, i.e. as copies of key
    L - 1, so the defective result is the fp64 attention over the sequence padded to a multiple of 32 with that key."""
    qs, vs = to_sequences(q.double(), mode), to_sequences(v.double(), mode)
    L = qs.shape[-2]
    pad = -L % 32
    kq = torch.cat([qs, qs[..., L - 1:L, :].expand(*qs.shape[:-2], pad, qs.shape[-1])], -2)
    kv = torch.cat([vs, vs[..., L - 1:L, :].expand(*vs.shape[:-2], pad, vs.shape[-1])], -2)
    o = (qs @ kq.transpose(-1, -2)).softmax(-1) @ kv
    return from_sequences(o, mode, q.shape).contiguous()


def seq_ref_swapped_values(q, v, mode, a=0, b=1):
    """Defect (ii): the values of keys a and b exchanged (a V slot-order error), otherwise the fp64 attention."""
    qs, vs = to_sequences(q.double(), mode), to_sequences(v.double(), mode).clone()
    vs[..., [a, b], :] = vs[..., [b, a], :]
    o = (qs @ qs.transpose(-1, -2)).softmax(-1) @ vs
    return from_sequences(o, mode, q.shape).contiguous()


def seq_ref_two_roundings_of_hi(q, v, mode):
    """Defect (iv), found by these tests in the MFMA kernel: the fp16 hi of the scaled query x = fp32(q log2 e) rounded from
    the EXACT product for the operand and from x for the remainder lo = x - hi, so that hi + lo misses x by an fp16 ulp
    wherever the two roundings part (on exact ties).  Keys are unaffected (they are not scaled)."""
    x = q * LOG2E
    hi_x = x.half().double()
    # fp16 rounding of the exact product: as hi_x, except where x sits on a tie and the exact product lies beyond it
    r, d = x.double() - hi_x, q.double() * LOG2E.double() - x.double()
    ulp = torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -14))) - 10)
    beyond = (r.abs() == 0.5 * ulp) & (torch.sign(d) == torch.sign(r))
    hi_exact = hi_x + torch.where(beyond, torch.sign(r) * ulp, torch.zeros_like(r))
    q_eff = (hi_exact + (x.double() - hi_x)) / LOG2E.double()
    qs, ks, vs = to_sequences(q_eff, mode), to_sequences(q.double(), mode), to_sequences(v.double(), mode)
    o = (qs @ ks.transpose(-1, -2)).softmax(-1) @ vs
    return from_sequences(o, mode, q.shape).contiguous()
