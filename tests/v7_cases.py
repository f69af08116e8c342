"""Inputs, float64 references and bounds of the tests of the operators only CVSR_V7 uses (csrc/v7_ops.hip: chan_pool, spatial_gate /
gate_map, gate_map_cumulative, rdab_mix, shrink_planes, lincomb; csrc/v7_train.hip: chan_pool_bwd, mul_plane, dot_plane,
gumbel_softmax, softmax64_bwd).

A plain helper module: tests/test_gpu_v7_ops.py runs the kernels on what is built here, tests/test_v7_cases_cpu.py shows, without
a GPU, that these inputs and references catch defective kernels.  Everything is seeded and computed on the CPU; cached tensors
must be left unchanged by their users.

References are written from the operators' definitions in arch/SIDECVSR_our.py (ChannelPool 1883-1885, SpatialAttention 2719-2730,
RDAB 2813-2847, the feature extractor's repeated gate 1350-1368, the prior pyramid 4296-4303, Block's sums 367-375) in plain torch
on NCHW tensors -- max / mean, F.conv2d, softmax, F.interpolate, autograd for the adjoints -- and take a `dtype`: float64 is the
reference, float32 the restatement that sets the scale of the bound (fold_cases.bound: max(4 x the restatement's error, 2^-20
max|ref|)).  Activations are handed over pixel-major [B,H,W,64] as the kernels take them; the noise stays NCHW like the module's.

The sigmoid's argument stays within +-8 (asserted in test_v7_cases_cpu.py).  The `ties` family of the per-pixel kernels, the
integer families of shrink_planes and lincomb give exact expectations."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

from fold_cases import bound  # noqa: F401  (the one bound of this family too)

F64, F32 = torch.float64, torch.float32


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def case_id(c):
    return "-".join(str(v) for v in c)


def nchw(t, dtype=F64):
    return t.to(dtype).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def channel_pool(x):
    """What ChannelPool computes (arch.py:1883-1885), on NCHW: plane 0 the maximum over the channels, plane 1 their mean.
    max(dim) and not amax: its gradient goes to the first maximum alone, as the module's does."""
    return torch.stack([x.max(dim=1).values, x.mean(dim=1)], dim=1)


def spatial_attention(x, w, b):
    """What SpatialAttention computes (arch.py:2719-2730), on NCHW: (the gated tensor, the sigmoid's argument); the convolution
    over the pooled pair is zero padded to keep the size"""
    arg = F.conv2d(channel_pool(x), w, b, padding=w.shape[-1] // 2)
    return torch.sigmoid(arg) * x, arg


# ------------------------------------------------------------------------------------------------------------ per-pixel kernels
PixCase = collections.namedtuple("PixCase", "family B H W")
PIX_SHAPES = ((1, 1, 1), (2, 1, 3), (1, 3, 5), (1, 4, 4), (1, 1, 17), (2, 7, 9), (3, 12, 20))       # npix 1, 6, 15, 16, 17, 126, 720
PIX_FAMILIES = ("plain", "negative", "ties")
PIX_CASES = tuple(PixCase(f, *s) for f in PIX_FAMILIES for s in PIX_SHAPES)
EXACT_FAMILIES = ("ties",)
TIE_KINDS = ("two_lanes", "all_equal", "only_0", "only_63", "random")
TIE_PAIR = (9, 42)                           # `two_lanes`: the maximum sits in channel 9 (lane 2) and in channel 42 (lane 10)
PITCH = 128                                  # the strided cases: rows of 128 channels read as [..., 64:128]


def tie_kind(q):
    """the kind of pixel q of a `ties` case (pixel 0 has the two-lane tie: the one-pixel case holds it)"""
    return TIE_KINDS[q % len(TIE_KINDS)]


@functools.lru_cache(maxsize=None)
def pix_inputs(c):
    """dict of fp32 tensors: x, y [B,H,W,64] (y: the second operand of dot_plane = the cotangent of mul_plane), plane [B,H,W],
    cot2 [B,H,W,2] (the cotangent of ChannelPool).  plain: randn with a per-channel scale of 0.5 .. 2; negative: every even pixel
    has all channels below -0.1; ties: integers in {-1, 0, 1}, the pixels cycling through TIE_KINDS, integer cotangents."""
    g = _gen("pix", *c)
    shape = (c.B, c.H, c.W, 64)
    npix = c.B * c.H * c.W
    if c.family == "ties":
        x = torch.randint(-1, 2, shape, generator=g).float().view(npix, 64)
        low = torch.randint(-1, 1, shape, generator=g).float().view(npix, 64)        # {-1, 0}: below a maximum of 1
        for q in range(npix):
            kind = tie_kind(q)
            if kind == "all_equal":
                x[q] = float(q % 3 - 1)
            elif kind != "random":
                x[q] = low[q]
                x[q, {"two_lanes": list(TIE_PAIR), "only_0": [0], "only_63": [63]}[kind]] = 1.0
        ints = lambda *s: torch.randint(-3, 4, s, generator=g).float()  # noqa: E731
        cot2 = ints(c.B, c.H, c.W, 2)
        cot2[..., 0] += (cot2[..., 0] == 0) * 2.0                # no pixel without a gradient to route
        return {"x": x.view(shape), "y": ints(*shape), "plane": ints(c.B, c.H, c.W), "cot2": cot2}
    x = torch.randn(shape, generator=g) * torch.linspace(0.5, 2.0, 64)
    if c.family == "negative":
        x = x.view(npix, 64)
        x[0::2] = -(x[0::2].abs() + 0.1)
        x = x.view(shape)
    return {"x": x, "y": torch.randn(shape, generator=g), "plane": torch.rand(c.B, c.H, c.W, generator=g) + 0.25,
            "cot2": torch.randn(c.B, c.H, c.W, 2, generator=g)}


def pool_ref(c, dtype=F64):
    """(pooled [B,H,W,2], dx [B,H,W,64]): ChannelPool and its adjoint on cot2 by autograd (torch.max(dim): the first maximum)"""
    d = pix_inputs(c)
    x = nchw(d["x"], dtype).clone().requires_grad_()
    y = channel_pool(x)
    (dx,) = torch.autograd.grad(y, x, nchw(d["cot2"], dtype))
    return nhwc(y.detach()), nhwc(dx)


def mul_plane_ref(c, dtype=F64):
    """(out [B,H,W,64], dx [B,H,W,64], dplane [B,H,W]): x * scale (arch.py:2730) and both gradients of <x * scale, y>"""
    d = pix_inputs(c)
    x = nchw(d["x"], dtype).clone().requires_grad_()
    scale = d["plane"].to(dtype).unsqueeze(1).clone().requires_grad_()
    out = x * scale
    dx, ds = torch.autograd.grad(out, (x, scale), nchw(d["y"], dtype))
    return nhwc(out.detach()), nhwc(dx), ds[:, 0].contiguous()


def softmax_rows_ref(c, dtype=F64):
    """(r [B,H,W,64], dz [B,H,W,64]): r = softmax over the channels of the case's x, and the gradient of <r, y> with respect
    to x by autograd.  softmax64_bwd is handed the fp32 rounding of the float64 r, as it is handed the forward's fp32 rows."""
    d = pix_inputs(c)
    z = nchw(d["x"], dtype).clone().requires_grad_()
    r = z.softmax(1)
    (dz,) = torch.autograd.grad(r, z, nchw(d["y"], dtype))
    return nhwc(r.detach()), nhwc(dz)


def pitched(t, fill=1e3):
    """[B,H,W,64] as the upper half of rows of PITCH channels (ld = 128); the lower half holds `fill`: used by mistake, it shows"""
    wide = torch.full((*t.shape[:-1], PITCH), fill, dtype=t.dtype, device=t.device)
    wide[..., 64:] = t
    return wide[..., 64:]


# ------------------------------------------------------------------------------------------------------------ pooled_conv users
GateCase = collections.namedtuple("GateCase", "ks B H W")
GATE_SHAPES = ((2, 1, 1), (2, 3, 5), (2, 7, 1), (2, 1, 9), (2, 7, 7), (2, 8, 9), (2, 12, 20))
GATE_CASES = tuple(GateCase(ks, *s) for ks in (7, 3) for s in GATE_SHAPES)
CUM_CASES = tuple(GateCase(7, *s) for s in ((2, 1, 1), (2, 3, 5), (2, 9, 11)))
CUM_ROUNDS = 4
GATE_ARG = 5.5                               # the convolution's share of the sigmoid's argument; the bias adds at most 0.5


def _unlike_images(g, B, H, W):
    """[B,H,W,64]: a per-pixel scale of 0.25 .. 1.5 moves the max map, image b has the channel offset 0.4 b and every second
    image the opposite sign of the scale ramp: no two images, rows or columns of the pooled maps are alike"""
    x = torch.randn(B, H, W, 64, generator=g) * (torch.rand(B, H, W, 1, generator=g) * 1.25 + 0.25)
    return x + 0.4 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def gate_inputs(c):
    """(x [B,H,W,64], w [1,2,ks,ks], b [1]): random = unsymmetric weights, scaled so that |conv(pool(x))| <= GATE_ARG"""
    g = _gen("gate", *c)
    x = _unlike_images(g, c.B, c.H, c.W)
    w = torch.randn(1, 2, c.ks, c.ks, generator=g)
    b = torch.rand(1, generator=g) - 0.5
    top = F.conv2d(channel_pool(nchw(x)), w.double(), None, padding=(c.ks - 1) // 2).abs().max().item()
    return x, (w * (GATE_ARG / top)).float(), b


def gate_ref(c, dtype=F64):
    """(SpatialAttention(x) [B,H,W,64], the sigmoid's argument [B,1,H,W])"""
    x, w, b = gate_inputs(c)
    out, arg = spatial_attention(nchw(x, dtype), w.to(dtype), b.to(dtype))
    return nhwc(out), arg


@functools.lru_cache(maxsize=None)
def pix_gate_inputs(c):
    """(x, w [1,2,7,7], b [1]): the 7x7 gate on a per-pixel case's own x (npix 1, 6, 15, 16, 17, ... of the 16-pixel blocks of
    spatial_gate_kernel), the weights scaled like gate_inputs'"""
    g = _gen("pix_gate", *c)
    x = pix_inputs(c)["x"]
    w = torch.randn(1, 2, 7, 7, generator=g)
    top = F.conv2d(channel_pool(nchw(x)), w.double(), None, padding=3).abs().max().item()
    return x, (w * (GATE_ARG / top)).float(), torch.rand(1, generator=g) - 0.5


def pix_gate_ref(c, dtype=F64):
    """(SpatialAttention(x) [B,H,W,64], the sigmoid's argument) of pix_gate_inputs"""
    x, w, b = pix_gate_inputs(c)
    out, arg = spatial_attention(nchw(x, dtype), w.to(dtype), b.to(dtype))
    return nhwc(out), arg


def cum_ref(c, dtype=F64):
    """[x_1 .. x_4], each [B,H,W,64]: SpatialAttention applied CUM_ROUNDS times to x itself (arch.py:1351-1366)"""
    x, w, b = gate_inputs(c)
    x2, outs = nchw(x, dtype), []
    for _ in range(CUM_ROUNDS):
        x2, _ = spatial_attention(x2, w.to(dtype), b.to(dtype))
        outs.append(nhwc(x2))
    return outs


# ------------------------------------------------------------------------------------------------------------ rdab_mix, gumbel_softmax
MixCase = collections.namedtuple("MixCase", "noise v B H W")
MIX_SHAPES = ((3, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (1, 10, 13), (3, 5, 13), (2, 12, 20))     # P 1 63 64 65 130 65 240
NOISES = ("uniform", "extreme")
V_FAMILIES = ("spread", "peaked")
MIX_CASES = tuple(MixCase(n, v, *s) for n in NOISES for v in V_FAMILIES for s in MIX_SHAPES)
U_TOP, U_LOW = 1.0 - 2.0 ** -24, 1e-30       # the ends of rand().clamp_min(1e-30) in fp32


def mix_tiles(c):
    """B * tiles of 64 pixels: the waves rdab_mix needs (an odd count leaves a surplus wave)"""
    return c.B * (-(-c.H * c.W // 64))


@functools.lru_cache(maxsize=None)
def mix_inputs(c):
    """dict of fp32 tensors: xf, xc, cot [B,H,W,64], w3 [1,2,3,3], b3 [1], v [B,64], u [B,64,H,W].
    noise  uniform: rand().clamp_min(1e-30); extreme: a tenth of the entries at 1 - 2^-24, a tenth at 1e-30, a tenth within 1e-4
           below 1, the rest uniform.
    v      spread: rand * 3; peaked: one channel of each image (7, 28, 49, ...) 20 above that."""
    g = _gen("mix", *c)
    shape = (c.B, c.H, c.W, 64)
    xc = _unlike_images(g, c.B, c.H, c.W)
    w3 = torch.randn(1, 2, 3, 3, generator=g)
    w3 = (w3 * (GATE_ARG / F.conv2d(channel_pool(nchw(xc)), w3.double(), None, padding=1).abs().max().item())).float()
    u = torch.rand(c.B, 64, c.H, c.W, generator=g).clamp_min(U_LOW)
    if c.noise == "extreme":
        pick = torch.rand(u.shape, generator=g)
        near = (1.0 - 1e-4 * torch.rand(u.shape, generator=g)).clamp_max(U_TOP)
        u = torch.where(pick < 0.1, torch.full_like(u, U_TOP), torch.where(pick < 0.2, torch.full_like(u, U_LOW),
                                                                         torch.where(pick < 0.3, near, u)))
    v = torch.rand(c.B, 64, generator=g) * 3
    if c.v == "peaked":
        v[torch.arange(c.B), (7 + 21 * torch.arange(c.B)) % 64] += 20.0
    return {"xf": torch.randn(shape, generator=g), "xc": xc, "cot": torch.randn(shape, generator=g), "w3": w3,
            "b3": torch.rand(1, generator=g) - 0.5, "v": v, "u": u}


def _gumbel_softmax(v, u):
    """What RDAB.gumbel_softmax computes (arch.py:2819-2828) at temperature 1 with the uniform draw u given: the softmax over
    the channels of v plus Gumbel noise, the noise being minus the logarithm of minus the logarithm of u"""
    return (v - torch.log(-torch.log(u))).softmax(dim=1)


def _v_map(v, H, W):
    """conv_du_re2's [B,64,1,1] output resized to the frame (arch.py:2835: bilinear from one sample = that sample everywhere)"""
    return F.interpolate(v.view(*v.shape, 1, 1), (H, W), mode="bilinear", align_corners=False)


def softmax_ref(c, dtype=F64):
    """(the residual mask [B,H,W,64], the gradient [B,64] of <mask, cot> with respect to v by autograd)"""
    d = mix_inputs(c)
    v = d["v"].to(dtype).clone().requires_grad_()
    r = _gumbel_softmax(_v_map(v, c.H, c.W), d["u"].to(dtype))
    (dv,) = torch.autograd.grad(r, v, nchw(d["cot"], dtype))
    return nhwc(r.detach()), dv


def mix_ref(c, dtype=F64):
    """The mixing step of RDAB.forward (arch.py:2836-2844) [B,H,W,64], its convolved operand xf given: xf times the sum of the
    residual mask (the Gumbel softmax of v) and the attention mask (the sigmoid of the 3x3 convolution of pool(xc))"""
    d = mix_inputs(c)
    soft = _gumbel_softmax(_v_map(d["v"].to(dtype), c.H, c.W), d["u"].to(dtype))
    gate = torch.sigmoid(mix_gate_arg(c, dtype))
    return nhwc((soft + gate) * nchw(d["xf"], dtype))


def mix_gate_arg(c, dtype=F64):
    """the argument of the attention mask's sigmoid [B,1,H,W]"""
    d = mix_inputs(c)
    return F.conv2d(channel_pool(nchw(d["xc"], dtype)), d["w3"].to(dtype), d["b3"].to(dtype), padding=1)


# ------------------------------------------------------------------------------------------------------------ shrink_planes
ShrinkCase = collections.namedtuple("ShrinkCase", "data B planes H W level")
SHRINK_SHAPES = ((1, 1, 2, 2, 1), (1, 1, 4, 4, 2), (2, 2, 6, 10, 1), (2, 2, 8, 12, 2), (2, 2, 16, 24, 1), (2, 1, 16, 24, 2))
SHRINK_CASES = tuple(ShrinkCase(d, *s) for d in ("integer", "random") for s in SHRINK_SHAPES)
SHRINK_FRAMES, SHRINK_FRAME = 7, 3           # the batch-strided source: t[:, 3] of [B,7,planes,H,W]


@functools.lru_cache(maxsize=None)
def shrink_input(c):
    """[B,7,planes,H,W]: the case's source is frame 3; integer: values in -8 .. 8 (sums of four, divided by 16: exact)"""
    g = _gen("shrink", *c)
    shape = (c.B, SHRINK_FRAMES, c.planes, c.H, c.W)
    return torch.randint(-8, 9, shape, generator=g).float() if c.data == "integer" else torch.randn(shape, generator=g)


def shrink_ref(c, dtype=F64):
    """F.interpolate(scale_factor 0.5 / 0.25, bilinear, align_corners=False) / 2 resp. / 4 (arch.py:4294-4300)"""
    src = shrink_input(c)[:, SHRINK_FRAME].to(dtype).clone()
    return F.interpolate(src, scale_factor=0.5 ** c.level, mode="bilinear", align_corners=False) / float(2 ** c.level)


# ------------------------------------------------------------------------------------------------------------ lincomb
LinCase = collections.namedtuple("LinCase", "data n has_b has_c out")
LIN_LENGTHS = (4, 1024, 1028)                # one vector; one full block of 256 x 4; a second block of one thread
LIN_CASES = tuple(LinCase(d, n, hb, hc, "new") for d in ("integer", "random") for n in LIN_LENGTHS
                  for hb in (False, True) for hc in (False, True)) + tuple(
    LinCase(d, n, True, True, o) for d in ("integer", "random") for n in LIN_LENGTHS for o in ("a", "b"))
LIN_COEFFS = {"integer": (2.0, -0.5, 4.0), "random": (1.0, -0.7, 3.1)}       # (ca, cb, cc); integer: powers of two


@functools.lru_cache(maxsize=None)
def lin_inputs(c):
    """(a, b, c) [n]; integer: values in -8 .. 8"""
    g = _gen("lincomb", c.data, c.n)
    if c.data == "integer":
        return tuple(torch.randint(-8, 9, (c.n,), generator=g).float() for _ in range(3))
    return tuple(torch.randn(c.n, generator=g) for _ in range(3))


def lin_ref(c, dtype=F64):
    """x + r + d + u with the callers' coefficients (arch.py:370-373): ca a + cb b + cc c over the operands present"""
    a, b, cc_ = (t.to(dtype) for t in lin_inputs(c))
    ca, cb, cc = LIN_COEFFS[c.data]
    out = ca * a
    if c.has_b:
        out = out + cb * b
    if c.has_c:
        out = out + cc * cc_
    return out
