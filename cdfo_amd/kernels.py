"""Thin host wrappers: torch tensors (device memory + stream plumbing only) -> libcdfo_hip.so C-ABI calls.

Activations are fp32 pixel-major tensors of logical shape [B, H, W, C] whose last dim is contiguous; the pixel
pitch ``ld = t.stride(2)`` may exceed C, so a channel slice ``t[..., a:b]`` of a wider buffer is a valid operand
(this is how ``torch.cat`` disappears from the path)."""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, switches
from ._lib import CdfoError, ConvArgs, _vp, check
from .streaming import check_ra_lists

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
PREC_F32, PREC_BF16X3, PREC_BF16, PREC_FP16X2, PREC_FP16, PREC_FP16X1 = 0, 1, 2, 3, 4, 5


def _stream() -> C.c_void_p:
    """The CURRENT device's current stream.  Every public entry point (module forwards, the DCN operator, the metrics)
    makes its operands' device current first (`on_device`), and `_chk_act` refuses operands of another device, so a
    launch never pairs one device's stream with another device's pointers."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(t: torch.Tensor):
    """Context manager: make `t`'s device the current one (stream lookup, per-device caches of libcdfo_hip.so)."""
    if not t.is_cuda:
        raise NotImplementedError("the HIP path needs device tensors (there is no CPU fallback)")
    return torch.cuda.device(t.device)


class ImageMap:
    """M images of a pixel-major fp32 operand [M,H,W,C >= 64] that are not one dense block: image m starts
    ``(m % Bi) * s_b + (m // Bi) * s_g`` floats behind the first one (csrc/image_map.h); inside an image nothing changes (pixel
    pitch ld, dense pixels).  Built and validated by `image_map`; the wrappers that name a mapped operand take it where they take
    the dense tensor [M,H,W,C] and give the same bits."""
    __slots__ = ("first", "M", "Bi", "s_b", "s_g")

    def __init__(self, first, M, Bi, s_b, s_g):
        self.first, self.M, self.Bi, self.s_b, self.s_g = first, M, Bi, s_b, s_g

    shape = property(lambda self: (self.M, *self.first.shape))
    dtype = property(lambda self: self.first.dtype)
    device = property(lambda self: self.first.device)
    is_cuda = property(lambda self: self.first.is_cuda)
    ld = property(lambda self: self.first.stride(1))

    def dim(self) -> int:
        return 4

    def data_ptr(self) -> int:
        return self.first.data_ptr()

    def offset(self, m: int) -> int:
        """Floats from the first image to image m."""
        return (m % self.Bi) * self.s_b + (m // self.Bi) * self.s_g

    def image(self, m: int) -> torch.Tensor:
        """Image m as a view [H,W,C] of the operand's storage."""
        f = self.first
        return f.as_strided(f.shape, f.stride(), f.storage_offset() + self.offset(m))

    def dense(self) -> torch.Tensor:
        """The materialised copy [M,H,W,C] (tests, and the paths that take no map)."""
        return torch.stack([self.image(m) for m in range(self.M)])

    def triple(self):
        return self.Bi, self.s_b, self.s_g

    def sub(self, start: int, count: int) -> "ImageMap":
        """Images start .. start + count - 1 as a map of their own (start must open a block of Bi images: the form stays affine)."""
        if start % self.Bi or start < 0 or count <= 0 or start + count > self.M:
            raise ValueError(f"ImageMap.sub({start}, {count}): the slice must start a block of {self.Bi} images inside the {self.M}")
        f = self.first
        return ImageMap(f.as_strided(f.shape, f.stride(), f.storage_offset() + (start // self.Bi) * self.s_g), count, self.Bi, self.s_b, self.s_g)


def image_map(first: torch.Tensor, M: int, Bi: int, s_b: int, s_g: int) -> ImageMap:
    """The one place an image map is built and validated.  first: the FIRST image as a view [H,W,C >= 64] (fp32, channels contiguous,
    rows dense at its pixel pitch); image m of the M lies (m % Bi) * s_b + (m // Bi) * s_g floats behind it, all inside first's
    storage.  Strides are non-negative multiples of 4 floats (every image stays 16-byte aligned).  The three shapes of the neighbour
    phase over a stack whose clips lie s_c and whose frames lie s_f floats apart:
      frames i0 .. i0 + G - 1 of every clip, neighbour major   first = frame i0 of clip 0, M = G B, Bi = B, s_b = s_c, s_g = s_f
      one frame of every clip                                   first = that frame of clip 0, M = Bi = B, s_b = s_c, s_g = 0
      one frame of every clip, once per neighbour of a group    the same with M = G B"""
    if first.dtype != torch.float32 or first.dim() != 3 or first.stride(2) != 1:
        raise ValueError(f"image_map: the first image must be an fp32 [H,W,C] view with contiguous channels, got {first.dtype} "
                         f"{tuple(first.shape)} strides {first.stride()}")
    H, W, Cc = first.shape
    ld = first.stride(1)
    if Cc < 64 or ld < Cc or ld % 4 or (H > 1 and first.stride(0) != W * ld):
        raise ValueError(f"image_map: rows must be densely packed at a pixel pitch ld >= C >= 64, ld % 4 == 0; strides {first.stride()}")
    M, Bi, s_b, s_g = int(M), int(Bi), int(s_b), int(s_g)
    if M <= 0 or Bi <= 0 or s_b < 0 or s_g < 0 or s_b % 4 or s_g % 4 or first.storage_offset() % 4:
        raise ValueError(f"image_map: M = {M}, Bi = {Bi}, s_b = {s_b}, s_g = {s_g}: positive counts and non-negative strides that are "
                         "multiples of 4 floats expected")
    last = max((m % Bi) * s_b + (m // Bi) * s_g for m in range(M))
    if (first.storage_offset() + last + (H * W - 1) * ld + Cc) * 4 > first.untyped_storage().nbytes():
        raise ValueError(f"image_map: the {M} images leave the tensor's storage")
    return ImageMap(first, M, Bi, s_b, s_g)


def _is_map(t) -> bool:
    return isinstance(t, ImageMap)


def _chk_act(t: torch.Tensor, name: str = "tensor", dtype=torch.float32):
    if _is_map(t):      # validated by image_map; what is left is the device
        if dtype != torch.float32:
            raise ValueError(f"{name}: an image map describes an fp32 operand")
        _chk_act(t.first.unsqueeze(0), name)
        return (*t.shape, t.ld)
    if not t.is_cuda:
        raise NotImplementedError(f"{name}: the HIP path needs device tensors (no CPU fallback)")
    if t.device.index != torch.cuda.current_device():
        raise CdfoError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                        "enter kernels.on_device(tensor) (the module forwards do) before calling the wrappers")
    if t.dtype != dtype or t.dim() != 4 or t.stride(3) != 1:
        raise ValueError(f"{name}: expected fp32 [B,H,W,C] with contiguous channels, got {t.dtype} {tuple(t.shape)} "
                         f"strides {t.stride()}")
    B, H, W, Cc = t.shape
    ld = t.stride(2)
    if (W > 1 and t.stride(1) != W * ld) or (B > 1 and t.stride(0) != H * W * ld):
        raise ValueError(f"{name}: rows/images must be densely packed at pitch ld={ld}, strides {t.stride()}")
    return B, H, W, Cc, ld


def empty_act(B: int, H: int, W: int, Cc: int, device) -> torch.Tensor:
    return torch.empty((B, H, W, Cc), dtype=torch.float32, device=device)


# ----------------------------------------------------------------------------------------------- layout
def nchw_to_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, Cc, H, W = x.shape
    x = x.contiguous()
    if out is None:
        out = empty_act(B, H, W, Cc, x.device)
    _, _, _, _, ldo = _chk_act(out, "out")
    check(_lib.lib().cdfo_nchw_to_nhwc(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), B, Cc, H, W, ldo,
                                       _stream()), "cdfo_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(x, "x")
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
    check(_lib.lib().cdfo_nhwc_to_nchw(C.c_void_p(x.data_ptr()), ld, C.c_void_p(out.data_ptr()), B, Cc, H, W,
                                       _stream()), "cdfo_nhwc_to_nchw")
    return out


def range_probe(x: torch.Tensor, slots: torch.Tensor) -> None:
    """slots (int32[2], zeroed by the caller): [0] = bits of max finite |x|, [1] = 1 if x holds a NaN / infinity."""
    if not x.is_contiguous() or x.dtype != torch.float32 or x.numel() % 4:
        raise ValueError("range_probe: dense fp32 tensor with a multiple of 4 elements expected")
    check(_lib.lib().cdfo_range_probe(C.c_void_p(x.data_ptr()), C.c_longlong(x.numel()), C.c_void_p(slots.data_ptr()),
                                      _stream()), "cdfo_range_probe")


# ----------------------------------------------------------------------------------------------- conv
@dataclass
class PackedConv:
    w: torch.Tensor            # packed [ks*ks][Cin/4][CoutP][4]  (optionally [B] of those)
    bias: Optional[torch.Tensor]
    Cout: int
    Cin: int
    ks: int
    CoutP: int
    shuffle2: bool = False
    w_bstride: int = 0
    wq: Optional[torch.Tensor] = None   # split-bf16 packing for cdfo_conv3x3_bf16 (3x3, Cout % 64 == 0)
    tap_mask: Optional[torch.Tensor] = None   # int32 [Cin/16]: bit t set = tap t of that chunk has weights
    wh: Optional[torch.Tensor] = None   # fp16 packing (single block) for PREC_FP16X2
    CoutP16: int = 0                    # padded output channels of the 16-bit packings (multiple of 64)
    wh_sparse: Optional[torch.Tensor] = None   # fp16 packing of the four active taps per chunk (conv_ring + tap_mask)
    ww: Optional[torch.Tensor] = None   # Winograd F(2,3) fp16 image for conv3x3_wino (3x3, Cin = 64, Cout % 128 == 0)


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], shuffle2: bool = False,
              transposed: bool = False) -> PackedConv:
    """weight: OIHW (or IOHW for a ConvTranspose2d) fp32 on the device."""
    w = weight.detach().contiguous().float()
    if transposed:
        Cin, Cout, ks, _ = w.shape
    else:
        Cout, Cin, ks, _ = w.shape
    CoutP = (Cout + 31) // 32 * 32
    packed = torch.empty(ks * ks * Cin * CoutP, dtype=torch.float32, device=w.device)
    check(_lib.lib().cdfo_pack_conv_weight(C.c_void_p(w.data_ptr()), C.c_void_p(packed.data_ptr()), Cout, Cin, ks,
                                           int(shuffle2), int(transposed), _stream()), "cdfo_pack_conv_weight")
    b = None
    if bias is not None:
        b = bias.detach().contiguous().float()
        if shuffle2:
            cq = Cout // 4
            b = b.view(cq, 4).t().contiguous().view(-1)
    pc = PackedConv(packed, b, Cout, Cin, ks, CoutP, shuffle2)
    if ks == 3 and not transposed and not shuffle2 and Cout % 4 == 0 and Cin % 16 == 0:
        cp16 = (Cout + 63) // 64 * 64          # thin outputs (UDSA 64->16) ride on a 64-wide tile, masked in the epilogue
        pc.CoutP16 = cp16
        wq = torch.empty(2 * (Cin // 16) * 18 * cp16 * 8, dtype=torch.bfloat16, device=w.device)
        check(_lib.lib().cdfo_pack_conv3x3_bf16(C.c_void_p(w.data_ptr()), C.c_void_p(wq.data_ptr()), Cout, Cin,
                                                _stream()), "cdfo_pack_conv3x3_bf16")
        pc.wq = wq
        wh = torch.empty((Cin // 16) * 18 * cp16 * 8, dtype=torch.float16, device=w.device)
        check(_lib.lib().cdfo_pack_conv3x3_f16(C.c_void_p(w.data_ptr()), C.c_void_p(wh.data_ptr()), Cout, Cin, _stream()),
              "cdfo_pack_conv3x3_f16")
        pc.wh = wh
        if Cin == 64 and Cout % 128 == 0:
            ww = torch.empty(Cout * 64 * 12, dtype=torch.float16, device=w.device)
            check(_lib.lib().cdfo_pack_conv3x3_wino(C.c_void_p(w.data_ptr()), C.c_void_p(ww.data_ptr()), Cout, _stream()),
                  "cdfo_pack_conv3x3_wino")
            pc.ww = ww
    return pc


def _chk_cp16(src: torch.Tensor, who: str, planes: Optional[int] = 4):
    """src: fp16 chunk-planar [B, planes, H, W, 16] on the device (planes=None: any count) -> (B, planes, H, W)."""
    if not src.is_cuda:
        raise NotImplementedError(f"{who}: the HIP path needs device tensors (no CPU fallback)")
    if (src.dtype != torch.float16 or src.dim() != 5 or src.shape[1] != (planes or src.shape[1]) or src.shape[4] != 16
            or not src.is_contiguous()):
        raise ValueError(f"{who}: expected a contiguous fp16 [B,{planes or 'C/16'},H,W,16] source, got {src.dtype} {tuple(src.shape)}")
    return tuple(src.shape[:4])


def _cp16_out(out: Optional[torch.Tensor], shape: tuple, device, who: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float16, device=device)
    if out.shape != shape or out.dtype != torch.float16 or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous fp16 tensor of shape {shape}")
    return out


def _batch_slices(B: int, H: int, W: int, who: str):
    """The weights-stationary kernels address their [nb,4,H,W,16] fp16 source with 32-bit buffer offsets (< 2 GiB per launch):
    the batch in slices that fit."""
    limit = (1 << 31)
    per_img = 4 * H * W * 32
    if per_img >= limit:
        raise ValueError(f"{who}: one {H}x{W} image exceeds the 2 GiB source limit of a launch")
    step = max(1, min(B, (limit - 1) // per_img))
    for b0 in range(0, B, step):
        yield slice(b0, min(B, b0 + step))


def _offmask_ok(offset: torch.Tensor, mask: torch.Tensor, flow: torch.Tensor, B: int, third: int, H: int, W: int) -> bool:
    """The DCN operator's inputs of conv_offset_mask[_ws]: contiguous fp32 offset [B,2 third,H,W], mask [B,third,H,W], flow [B,2,H,W]."""
    return (tuple(offset.shape) == (B, 2 * third, H, W) and tuple(mask.shape) == (B, third, H, W) and tuple(flow.shape) == (B, 2, H, W)
            and all(t.is_contiguous() and t.dtype == torch.float32 for t in (offset, mask, flow)))


def _bind_res(res1: Optional[torch.Tensor], res2: Optional[torch.Tensor], B: int, Ho: int, Wo: int, Cout: int,
              a: Optional[ConvArgs] = None):
    """res1 / res2: fp32 pixel-major [B,Ho,Wo,>= Cout] or None -> their pitches (0 for None), also bound in `a` if given."""
    lds = [0, 0]
    for i, (nm, r) in enumerate((("res1", res1), ("res2", res2))):
        if r is not None:
            rb, rh, rw, rc, lds[i] = _chk_act(r, nm)
            if (rb, rh, rw) != (B, Ho, Wo) or rc < Cout:
                raise ValueError(f"{nm} shape {tuple(r.shape)} does not match the conv output")
            if a is not None:
                setattr(a, nm, r.data_ptr())
                setattr(a, "ldr" + nm[-1], lds[i])
    return lds


def _bind_res2_scale(a: ConvArgs, res2: Optional[torch.Tensor], res2_scale: Optional[torch.Tensor]) -> None:
    if res2_scale is not None:
        if (res2 is None or tuple(res2_scale.shape) != (a.B, a.Ho, a.Wo) or not res2_scale.is_contiguous()
                or res2_scale.dtype != torch.float32):
            raise ValueError("conv: res2_scale must be a contiguous fp32 [B,H,W] plane next to res2")
        a.res2_pixscale = res2_scale.data_ptr()


def pack_plane_chunk(w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """A one-channel 3x3 stencil (w [Co,1,3,3], b [Co]; where it feeds a 1x1 product, composed with it by compose_stem_1x1) as the weight
    table of the stream kernels' plane chunk: fp32 [Co,16] = nine taps | bias | six zeros (csrc/plane_chunk.h)."""
    Co = w.shape[0]
    if tuple(w.shape) != (Co, 1, 3, 3) or tuple(b.shape) != (Co,):
        raise ValueError("pack_plane_chunk: a [Co,1,3,3] stencil and its [Co] bias expected")
    t = torch.zeros((Co, 16), dtype=torch.float32, device=w.device)
    t[:, :9] = w.detach().float().reshape(Co, 9)
    t[:, 9] = b.detach().float()
    return t


def plane_ok(H: int, W: int) -> bool:
    """The shapes the plane chunk's 32-bit tap indices cover."""
    return H > 0 and W > 0 and H * W + 2 * W + 64 < (1 << 29)


def _plane_args(plane, B: int, H: int, W: int, Co: int, who: str):
    """plane = (view, Bi, s_b, s_g, table[, table image stride]): image b's dense H x W fp32 plane at view.data_ptr() + 4 * ((b % Bi) * s_b +
    (b // Bi) * s_g), all B of them inside view's storage; table: pack_plane_chunk's [Co,16] (or [B,Co,16] with its stride Co * 16)."""
    view, Bi, s_b, s_g, table = plane[:5]
    tstride = plane[5] if len(plane) > 5 else 0
    if view.dtype != torch.float32 or table.dtype != torch.float32 or not table.is_contiguous() or view.device != table.device:
        raise ValueError(f"{who}: the plane and its weight table must be fp32 tensors on one device")
    if not plane_ok(H, W) or Bi <= 0 or s_b < 0 or s_g < 0:
        raise ValueError(f"{who}: plane shape / strides outside the plane chunk's contract")
    last = max((b % Bi) * s_b + (b // Bi) * s_g for b in range(B))
    first = (view.data_ptr() - view.untyped_storage().data_ptr()) // 4
    if (first + last + H * W) * 4 > view.untyped_storage().nbytes():
        raise ValueError(f"{who}: the planes of {B} images leave the plane tensor's storage")
    if tuple(table.shape[-2:]) != (Co, 16) or (tstride and (table.dim() != 3 or table.shape[0] != B or tstride != Co * 16)):
        raise ValueError(f"{who}: the plane's weight table must be [{Co},16] (per image: [{B},{Co},16])")
    return view, int(Bi), int(s_b), int(s_g), table, int(tstride)


def _conv_args(srcs, pc: PackedConv, *, stride: int = 1, pad: int = 0, act: int = ACT_NONE, src_dtype=torch.float32,
               cp16: bool = False, store_mode: int = 0, out: Optional[torch.Tensor] = None, out_f16: bool = False,
               ldo: Optional[int] = None):
    """The one place that fills cdfo_conv_args: sources, geometry, weight / bias / activation, output -> (args, out).
    srcs: pixel-major tensors of src_dtype (validated here), or with cp16 ONE fp16 chunk-planar tensor that passed _chk_cp16.
    out=None allocates the tensor that store_mode writes; ldo: the pitch of an `out` that is no pixel-major activation (the caller
    has checked it).  The weight is pc's fp32 packing; a caller on another packing overwrites w / CoutP, and sets every field
    beyond these itself (a zero field = feature off)."""
    a = ConvArgs()
    if cp16:
        B, _, H, W, _ = srcs.shape
        device = srcs.device
        a.src[0], a.ld[0], a.cs[0], a.nsrc = srcs.data_ptr(), 16, pc.Cin, 1
    else:
        B = H = W = None
        cin = 0
        for i, s in enumerate(srcs):
            b_, h_, w_, c_, ld_ = _chk_act(s, f"src{i}", src_dtype)
            if B is None:
                B, H, W = b_, h_, w_
            elif (B, H, W) != (b_, h_, w_):
                raise ValueError("conv sources disagree on B/H/W")
            a.src[i], a.ld[i], a.cs[i] = s.data_ptr(), ld_, c_
            cin += c_
        if cin != pc.Cin:
            raise ValueError(f"conv: sources have {cin} channels, weight expects {pc.Cin}")
        device = srcs[0].device
        a.nsrc = len(srcs)
    Ho = (H + 2 * pad - pc.ks) // stride + 1
    Wo = (W + 2 * pad - pc.ks) // stride + 1
    a.B, a.H, a.W, a.Ho, a.Wo = B, H, W, Ho, Wo
    a.ks, a.stride, a.pad = pc.ks, stride, pad
    a.Cin, a.Cout, a.CoutP = pc.Cin, pc.Cout, pc.CoutP
    a.w, a.w_bstride, a.bias, a.act = pc.w.data_ptr(), pc.w_bstride, _vp(pc.bias), act
    a.src_f16, a.out_f16, a.store_mode = int(cp16 or src_dtype == torch.float16), int(out_f16), store_mode
    if ldo is None:
        odt = torch.float16 if out_f16 else torch.float32
        if out is None:    # CDFO_STORE_PLAIN, _SHUFFLE2, _S2D, _TAPS9
            shape = ((B, Ho, Wo, pc.Cout), (B, 2 * Ho, 2 * Wo, pc.Cout // 4), (B, Ho // 2, Wo // 2, 4 * pc.Cout),
                     (B, 2 * Ho, 2 * Wo, 12))[store_mode]
            out = torch.empty(shape, dtype=odt, device=device)
        _, _, _, _, ldo = _chk_act(out, "out", odt)
    a.out, a.ldo = out.data_ptr(), ldo
    return a, out


def conv(srcs: Sequence[torch.Tensor], pc: PackedConv, *, stride: int = 1, pad: int = 0, act: int = ACT_NONE,
         res1: Optional[torch.Tensor] = None, res2: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, prec: int = PREC_F32,
         ln: Optional[tuple] = None, s2d: bool = False, out_f16: bool = False, ln_out: Optional[tuple] = None,
         res2_scale: Optional[torch.Tensor] = None, cp16_out: bool = False, chan_sum_out: bool = False, plane=None):
    """plane = (view, Bi, s_b, s_g, table) (streaming 1x1 kernel, 64-channel result; raises elsewhere): one more 64-channel operand of the
    product that is a 3x3 stencil of the one-channel planes `view` addresses (see _plane_args) and is never materialised; table:
    pack_plane_chunk of the product's weights for that operand composed with the stencil, [64,16] or per image [B,64,16] + stride.
    chan_sum_out (64-channel result): also the per-image channel sums of the result as partials; the call returns (out, part, n)
    as `chan_sum_partial(out)` would give them (the streaming 1x1 kernel sums in its epilogue, every other path runs that pass).
    cp16_out (1x1, Cout = 64, 16-bit modes): also the fp16 chunk-planar copy [B,4,H,W,16] of the result (to_cp16 of the returned
    tensor) from the same kernel; the call then returns the pair (out, copy).
    res2_scale [B,H,W]: res2 enters the sum as res2 * res2_scale[pixel] (streaming 1x1 kernel only; raises elsewhere).
    ln_out = (gamma, beta) (1x1, Cout = 64, 16-bit modes): also LayerNorm64 of the RESULT as fp16 hi | lo planes
    [B,8,H,W,16] (layernorm64_hl of the returned tensor); the call then returns the pair (out, planes)."""
    if isinstance(srcs, (torch.Tensor, ImageMap)):
        srcs = [srcs]
    if any(_is_map(t) for t in (*srcs, res1, res2)):
        if ln is not None or s2d or out_f16 or ln_out is not None or res2_scale is not None or cp16_out:
            raise ValueError("conv: a mapped operand needs a plain fp32 64-channel result (no LayerNorm, no second output)")
        return _conv_mapped(srcs, pc, stride=stride, pad=pad, act=act, res1=res1, res2=res2, out=out, prec=prec,
                            chan_sum_out=chan_sum_out, plane=plane)
    if chan_sum_out:
        if cp16_out or ln_out is not None or out_f16 or s2d or pc.shuffle2 or pc.Cout != 64:
            raise ValueError("conv: chan_sum_out needs a plain fp32 64-channel result")
        if not (prec != PREC_F32 and pc.ks == 1 and stride == 1 and pad == 0 and pc.CoutP == 64 and ln is None
                and all(s.dtype == torch.float32 and s.shape[3] % 64 == 0 for s in srcs)):
            if plane is not None:
                raise ValueError("conv: a plane operand needs the streaming 1x1 kernel")
            o = conv(srcs, pc, stride=stride, pad=pad, act=act, res1=res1, res2=res2, out=out, prec=prec, ln=ln, res2_scale=res2_scale)
            return (o, *chan_sum_partial(o))
    src_f16 = srcs[0].dtype == torch.float16       # Block_'s fp16 body intermediate (single source, 1-pass fp16 MFMA)
    if src_f16:
        prec = PREC_FP16
    elif prec == PREC_FP16:
        raise ValueError("PREC_FP16 needs an fp16 source tensor")
    a, out = _conv_args(srcs, pc, stride=stride, pad=pad, act=act, src_dtype=torch.float16 if src_f16 else torch.float32,
                        store_mode=1 if pc.shuffle2 else 2 if s2d else 0, out=out, out_f16=out_f16)
    B, Ho, Wo = a.B, a.Ho, a.Wo
    _bind_res(res1, res2, B, Ho, Wo, pc.Cout, a)
    _bind_res2_scale(a, res2, res2_scale)
    if plane is not None:
        if not (prec != PREC_F32 and pc.ks == 1 and stride == 1 and pad == 0 and pc.CoutP == 64 and ln is None and ln_out is None
                and not cp16_out and res2_scale is None and not src_f16 and not out_f16
                and all(s.shape[3] % 64 == 0 for s in srcs)):
            raise ValueError("conv: a plane operand needs the streaming 1x1 kernel (split-bf16, plain 64-channel result)")
        view, Bi, s_b, s_g, table, tstride = _plane_args(plane, B, a.H, a.W, 64, "conv")
        if chan_sum_out:
            n = align_stats_slots(B, Ho * Wo)
            part = torch.zeros((B, n, 64), dtype=torch.float32, device=out.device)
            a.chan_sum_out, a.chan_sum_slots = part.data_ptr(), n
        check(_lib.lib().cdfo_conv1x1_bf16x3_plane(C.byref(a), _vp(view), Bi, C.c_longlong(s_b), C.c_longlong(s_g), _vp(table),
                                                   C.c_longlong(tstride), _stream()), "cdfo_conv1x1_bf16x3_plane")
        return (out, part, n) if chan_sum_out else out
    if (prec != PREC_F32 and pc.wq is not None and stride == 1 and pad == 1 and pc.w_bstride == 0):
        a.prec = prec
        a.CoutP = pc.CoutP16
        a.w = (pc.wh if prec in (PREC_FP16X2, PREC_FP16, PREC_FP16X1) else pc.wq).data_ptr()
        a.tap_mask = _vp(pc.tap_mask)
        check(_lib.lib().cdfo_conv3x3_bf16(C.byref(a), _stream()), "cdfo_conv3x3_bf16")
        return out
    if src_f16 or out_f16:
        raise ValueError("fp16 tensors are only supported by the 16-bit MFMA 3x3 kernel")
    if ln is not None:
        a.ln_gamma, a.ln_beta = ln[0].data_ptr(), ln[1].data_ptr()
    if (prec != PREC_F32 and pc.ks == 1 and stride == 1 and pad == 0 and pc.CoutP % 64 == 0 and pc.CoutP <= 256
            and all(s.shape[3] % 64 == 0 for s in srcs)):
        if cp16_out:
            if ln_out is not None or ln is not None or pc.Cout != 64 or pc.CoutP != 64:
                raise ValueError("conv: cp16_out needs a plain 64-channel 1x1 convolution")
            copy = torch.empty((B, 4, Ho, Wo, 16), dtype=torch.float16, device=out.device)
            a.out2_cp16 = copy.data_ptr()
            check(_lib.lib().cdfo_conv1x1_bf16x3(C.byref(a), _stream()), "cdfo_conv1x1_bf16x3")
            return out, copy
        if chan_sum_out:
            n = align_stats_slots(B, Ho * Wo)
            part = torch.zeros((B, n, 64), dtype=torch.float32, device=out.device)
            a.chan_sum_out, a.chan_sum_slots = part.data_ptr(), n
            check(_lib.lib().cdfo_conv1x1_bf16x3(C.byref(a), _stream()), "cdfo_conv1x1_bf16x3")
            return out, part, n
        planes = None
        if ln_out is not None and pc.Cout == 64 and pc.CoutP == 64 and ln is None:
            planes = torch.empty((B, 8, Ho, Wo, 16), dtype=torch.float16, device=out.device)
            a.out2_cp16, a.ln_gamma, a.ln_beta = planes.data_ptr(), ln_out[0].data_ptr(), ln_out[1].data_ptr()
        check(_lib.lib().cdfo_conv1x1_bf16x3(C.byref(a), _stream()), "cdfo_conv1x1_bf16x3")
        if ln_out is not None:
            return out, (planes if planes is not None else layernorm64_hl(out, ln_out[0], ln_out[1]))
        return out
    check(_lib.lib().cdfo_conv_igemm(C.byref(a), _stream()), "cdfo_conv_igemm")
    if ln_out is not None:
        return out, layernorm64_hl(out, ln_out[0], ln_out[1])
    if cp16_out:
        return out, to_cp16(out)
    return out


def conv_map_ok(pc: PackedConv, prec: int, *, pad: int = 0, plane: bool = False, res: bool = False, chan_sum: bool = False,
                src0_only: bool = True) -> bool:
    """Whether conv() takes image maps for this convolution: a 1x1 with a 64-channel result on the split-bf16 kernels (plane: with a
    plane operand; res: a residual is mapped; chan_sum: with chan_sum_out -- those three need the streaming kernel, which holds up to
    192 input channels), or the tiled 3x3 kernel in split-bf16 / split-fp16 with only source 0 mapped."""
    if prec == PREC_F32 or pc.shuffle2:
        return False
    if pc.ks == 1 and pad == 0:
        return pc.CoutP == 64 and pc.Cout % 8 == 0 and conv1x1_map_ok(pc.Cin, plane=plane, res=res, chan_sum=chan_sum)
    return (pc.ks == 3 and pad == 1 and prec in (PREC_BF16X3, PREC_FP16X2) and pc.wq is not None and pc.w_bstride == 0 and pc.Cout > 32
            and src0_only and not (plane or res or chan_sum))


def conv1x1_map_ok(Cin: int, *, plane: bool = False, res: bool = False, chan_sum: bool = False) -> bool:
    """cdfo_conv1x1_map_ok: whether the mapped 1x1 entry point takes Cin input channels -> 64 with these features (host arithmetic)."""
    return Cin % 64 == 0 and bool(_lib.lib().cdfo_conv1x1_map_ok(Cin, int(plane), int(res), int(chan_sum)))


def _conv_mapped(srcs, pc: PackedConv, *, stride, pad, act, res1, res2, out, prec, chan_sum_out, plane):
    """conv() where a source or a residual is an ImageMap (see conv_map_ok)."""
    smap, rmap = [_is_map(s) for s in srcs], [_is_map(res1), _is_map(res2)]
    if stride != 1 or not conv_map_ok(pc, prec, pad=pad, plane=plane is not None, res=any(rmap), chan_sum=chan_sum_out,
                                      src0_only=not any(smap[1:])):
        raise ValueError("conv: no kernel of this convolution takes these operands through an image map (conv_map_ok)")
    a, out = _conv_args(srcs, pc, stride=1, pad=pad, act=act, out=out)
    B, Ho, Wo = a.B, a.Ho, a.Wo
    _bind_res(res1, res2, B, Ho, Wo, pc.Cout, a)
    if pc.ks == 3:
        a.prec = prec
        a.CoutP = pc.CoutP16
        a.w = (pc.wh if prec == PREC_FP16X2 else pc.wq).data_ptr()
        a.tap_mask = _vp(pc.tap_mask)
        Bi, s_b, s_g = srcs[0].triple()
        check(_lib.lib().cdfo_conv3x3_bf16_map(C.byref(a), Bi, C.c_longlong(s_b), C.c_longlong(s_g), _stream()), "cdfo_conv3x3_bf16_map")
        return out
    if any(s.shape[3] % 64 for s in srcs):
        raise ValueError("conv: the mapped 1x1 kernels need 64-channel sources")
    maps = (C.c_longlong * (3 * (len(a.src) + 2)))()
    for i, t in (*enumerate(srcs), (len(a.src), res1), (len(a.src) + 1, res2)):
        if _is_map(t):
            maps[3 * i:3 * i + 3] = t.triple()
    pl = (None, 0, 0, 0, None, 0)
    if plane is not None:
        pl = _plane_args(plane, B, a.H, a.W, 64, "conv")
    part = n = None
    if chan_sum_out:
        n = align_stats_slots(B, Ho * Wo)
        part = torch.zeros((B, n, 64), dtype=torch.float32, device=out.device)
        a.chan_sum_out, a.chan_sum_slots = part.data_ptr(), n
    check(_lib.lib().cdfo_conv1x1_bf16x3_map(C.byref(a), maps, _vp(pl[0]), pl[1], C.c_longlong(pl[2]), C.c_longlong(pl[3]), _vp(pl[4]),
                                             C.c_longlong(pl[5]), _stream()), "cdfo_conv1x1_bf16x3_map")
    return (out, part, n) if chan_sum_out else out


@contextlib.contextmanager
def cu_limit(n: int):
    """Persistent kernels launched by this thread inside the block fill at most n compute units (cdfo_set_cu_limit)."""
    prev = _lib.lib().cdfo_set_cu_limit(int(n))
    try:
        yield
    finally:
        _lib.lib().cdfo_set_cu_limit(prev)


def conv_offset_mask(src: torch.Tensor, pc: PackedConv, offset: torch.Tensor, mask: torch.Tensor, flow: torch.Tensor, mag: float,
                     accumulate: bool, prec: int) -> None:
    """MVDualAttAlignment's conv_offset[2] (3x3, 64 -> 27 dg) with the module's offset / mask assembly (arch.py:3336-3350) as its
    epilogue (CDFO_STORE_OFFMASK): src pixel-major [B,H,W,64]; offset [B,18 dg,H,W] / mask [B,9 dg,H,W] NCHW = the DCN operator's
    inputs; flow [B,2,H,W] contiguous.  accumulate=False: the first head (offset = mag tanh + flipped flow, mask = raw sums);
    accumulate=True: the second head in place (offset += mag tanh, mask = sigmoid(mask + sums)).  W % 4 == 0, 16-bit modes only."""
    a, _ = _conv_args([src], pc, pad=1, store_mode=4, out=offset, ldo=4)
    B, H, W = a.B, a.H, a.W
    if (pc.ks != 3 or pc.Cout % 3 or pc.wq is None or W % 4 or prec not in (PREC_BF16X3, PREC_FP16X2, PREC_FP16X1)
            or not _offmask_ok(offset, mask, flow, B, pc.Cout // 3, H, W)):
        raise ValueError("conv_offset_mask: unsupported configuration")
    a.CoutP, a.prec = pc.CoutP16, prec
    a.w = (pc.wh if prec in (PREC_FP16X2, PREC_FP16X1) else pc.wq).data_ptr()
    a.mask_out, a.flow, a.flow_bstride = mask.data_ptr(), flow.data_ptr(), 2 * H * W
    a.off_mag, a.off_accumulate = float(mag), int(accumulate)
    check(_lib.lib().cdfo_conv3x3_bf16(C.byref(a), _stream()), "cdfo_conv3x3_bf16 (offset / mask epilogue)")


def pack_conv_n16(weight: torch.Tensor) -> torch.Tensor:
    """[16, 64, 3, 3] fp32 -> the bf16 hi | lo image of cdfo_conv3x3_c64_n16: [18 K steps = tap*2 + half][hi|lo][lane = kg*16 + m][8]
    with element j = W[m][32 half + 8 kg + j][tap] (parameter-sized torch arithmetic, once per weight version)."""
    if tuple(weight.shape) != (16, 64, 3, 3):
        raise ValueError("pack_conv_n16: a [16, 64, 3, 3] weight expected")
    w = weight.detach().float().permute(2, 3, 1, 0).reshape(9, 2, 4, 8, 16).permute(0, 1, 2, 4, 3).reshape(18, 64, 8)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo], 1).contiguous()              # [18, 2, 64, 8] bf16 = 36,864 bytes


def conv3x3_n16(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], act: int = ACT_NONE) -> torch.Tensor:
    """3x3 / stride 1 / pad 1 convolution 64 -> 16 (split-bf16, fp32-grade): x [B,H,W,64] (channel slices allowed) -> [B,H,W,16]."""
    B, H, W, Cc, ld = _chk_act(x)
    if Cc != 64 or w_packed.dtype != torch.bfloat16 or w_packed.numel() != 18 * 2 * 64 * 8:
        raise ValueError("conv3x3_n16: 64 input channels and a pack_conv_n16 weight image expected")
    out = empty_act(B, H, W, 16, x.device)
    check(_lib.lib().cdfo_conv3x3_c64_n16(_vp(x), ld, B, H, W, _vp(w_packed), _vp(bias), act, _vp(out), 16, _stream()),
          "cdfo_conv3x3_c64_n16")
    return out


def to_cp16(x: torch.Tensor) -> torch.Tensor:
    """fp32 pixel-major [B,H,W,C] -> fp16 chunk-planar [B, C/16, H, W, 16] (the source layout of conv3x3_ws)."""
    B, H, W, Cc, ld = _chk_act(x)
    out = torch.empty((B, Cc // 16, H, W, 16), dtype=torch.float16, device=x.device)
    check(_lib.lib().cdfo_to_cp16(_vp(x), ld, B, C.c_longlong(H * W), Cc, _vp(out), _stream()), "cdfo_to_cp16")
    return out


def conv3x3_ws(src: torch.Tensor, pc: PackedConv, *, act: int = ACT_NONE, s2d: bool = False,
               out: Optional[torch.Tensor] = None, dbg: int = 0, clk: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Block_.body[0]-shaped convolution (3x3, 64 input channels, Cout % 64 == 0) on the weights-stationary kernel.
    src: fp16 chunk-planar [B,4,H,W,16]; result: fp16 chunk-planar [B,Cout/16,H,W,16], or with s2d its space-to-depth
    form [B,4*Cout/16,H/2,W/2,16] (chunk = phase*Cout/16 + channel/16, phase = (y&1)*2 + (x&1))."""
    B, _, H, W = _chk_cp16(src, "conv3x3_ws")
    if pc.wh is None or pc.Cin != 64 or pc.ks != 3 or pc.Cout % 64:
        raise ValueError("conv3x3_ws: needs a 3x3 weight with 64 input channels and Cout % 64 == 0")
    shape = (B, pc.Cout // 4, H // 2, W // 2, 16) if s2d else (B, pc.Cout // 16, H, W, 16)
    out = _cp16_out(out, shape, src.device, "conv3x3_ws")
    for sl in _batch_slices(B, H, W, "conv3x3_ws"):
        check(_lib.lib().cdfo_conv3x3_c64_ws(_vp(src[sl]), sl.stop - sl.start, H, W, _vp(pc.wh), pc.CoutP16, _vp(pc.bias), pc.Cout,
                                             act, _vp(out[sl]), 2 if s2d else 0, dbg, _vp(clk), _stream()),
              "cdfo_conv3x3_c64_ws")
    return out


def wino_enabled() -> bool:
    """CDFO_WINO=0 keeps Block_.body[0] on the direct weights-stationary kernel (developer A/B switch)."""
    return switches.get("CDFO_WINO")


def halfsplit_to_rows(t: torch.Tensor) -> torch.Tensor:
    """[B, planes, H, W, 16] stored with half-split rows ([H][2][W][8], CDFO_STORE_S2D_HS) -> the natural [B, planes, H, W, 16] (tests)."""
    B, P, H, W, _ = t.shape
    return t.reshape(B, P, H, 2, W, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, P, H, W, 16)


def conv3x3_wino(src: torch.Tensor, pc: PackedConv, *, act: int = ACT_NONE, s2d: bool = False,
                 out: Optional[torch.Tensor] = None, dbg: int = 0, halfsplit: bool = False, clk: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv3x3_ws's operands and result on the row-streaming Winograd F(2,3) kernel (cdfo_conv3x3_c64_wino): Cout % 128 == 0, W even."""
    B, _, H, W = _chk_cp16(src, "conv3x3_wino")
    if pc.ww is None:
        raise ValueError("conv3x3_wino: needs a 3x3 weight with 64 input channels and Cout % 128 == 0")
    shape = (B, pc.Cout // 4, H // 2, W // 2, 16) if s2d else (B, pc.Cout // 16, H, W, 16)
    out = _cp16_out(out, shape, src.device, "conv3x3_wino")
    if halfsplit and not s2d:
        raise ValueError("conv3x3_wino: half-split rows exist for the space-to-depth store only")
    mode = (5 if halfsplit else 2) if s2d else 0
    if dbg:      # developer ablations (tools/bench_wino.py): wrong results by construction
        check(_lib.lib().cdfo_conv3x3_c64_wino_dbg(_vp(src), B, H, W, _vp(pc.ww), _vp(pc.bias), pc.Cout, act, _vp(out), mode,
                                                   dbg, _vp(clk), _stream()), "cdfo_conv3x3_c64_wino_dbg")
        return out
    check(_lib.lib().cdfo_conv3x3_c64_wino(_vp(src), B, H, W, _vp(pc.ww), _vp(pc.bias), pc.Cout, act, _vp(out), mode,
                                           _stream()), "cdfo_conv3x3_c64_wino")
    return out


def wino_up2_enabled() -> bool:
    """CDFO_WINO_UP2=0 keeps Block_'s x2 branch on a materialised double-resolution source (developer A/B switch)."""
    return wino_enabled() and switches.get("CDFO_WINO_UP2")


def conv3x3_wino_up2(src_lr: torch.Tensor, pc: PackedConv, *, act: int = ACT_NONE, halfsplit: bool = False) -> torch.Tensor:
    """Block_.body[0] on the bilinear x2 of src_lr (fp16 chunk-planar [B,4,h,w,16], h and w even) without materialising it: the
    interpolation is folded into the Winograd kernel's input transform (cdfo_conv3x3_c64_wino_up2).  Result: the space-to-depth form
    [B, 4*Cout/16, h, w, 16] of the [B, Cout/16, 2h, 2w, 16] convolution output, as conv3x3_wino(..., s2d=True)."""
    B, _, h, w = _chk_cp16(src_lr, "conv3x3_wino_up2")
    if pc.ww is None or h % 2 or w % 2:
        raise ValueError("conv3x3_wino_up2: needs a Winograd weight image (Cout % 128 == 0) and even low-resolution sizes")
    out = torch.empty((B, pc.Cout // 4, h, w, 16), dtype=torch.float16, device=src_lr.device)
    check(_lib.lib().cdfo_conv3x3_c64_wino_up2(_vp(src_lr), B, 2 * h, 2 * w, _vp(pc.ww), _vp(pc.bias), pc.Cout, act, _vp(out),
                                               5 if halfsplit else 2, _stream()), "cdfo_conv3x3_c64_wino_up2")
    return out


def conv3x3_body0(src: torch.Tensor, pc: PackedConv, *, act: int = ACT_NONE, s2d: bool = False) -> torch.Tensor:
    """Block_.body[0]-shaped convolution (fp16 chunk-planar in and out): the Winograd F(2,3) kernel where it applies (Cout % 128 == 0,
    even width, one image of source / result below 2 GiB, CDFO_WINO != 0), the direct weights-stationary kernel otherwise."""
    _, _, H, W, _ = src.shape
    if pc.ww is not None and wino_enabled() and W % 2 == 0 and (not s2d or H % 2 == 0) and H * W * 2 * pc.Cout < (1 << 31):
        return conv3x3_wino(src, pc, act=act, s2d=s2d)
    return conv3x3_ws(src, pc, act=act, s2d=s2d)


def conv_offset_mask_ws_fits(B: int, H: int, W: int, third: int) -> bool:
    """The 32-bit addressing limits of cdfo_conv3x3_c64_ws_offmask: the whole fp16 source and one image's offset planes below 2 GiB."""
    return 4 * H * W * 32 * B < (1 << 31) and H * W * 2 * third * 4 < (1 << 31)


def conv_offset_mask_ws(src: torch.Tensor, pc: PackedConv, offset: torch.Tensor, mask: torch.Tensor, flow: torch.Tensor, mag: float,
                        accumulate: bool) -> None:
    """conv_offset_mask on the weights-stationary kernel (single-pass fp16 operands): src fp16 chunk-planar [B,4,H,W,16]; the rest as
    conv_offset_mask.  H even, 18 dg a multiple of 32 (dg = 16: 288)."""
    B, _, H, W = _chk_cp16(src, "conv_offset_mask_ws")
    third = pc.Cout // 3
    if (pc.wh is None or pc.Cin != 64 or pc.ks != 3 or pc.Cout % 3 or H % 2 or (2 * third) % 32 or pc.Cout % 8
            or not _offmask_ok(offset, mask, flow, B, third, H, W) or not conv_offset_mask_ws_fits(B, H, W, third)):
        raise ValueError("conv_offset_mask_ws: unsupported configuration")
    check(_lib.lib().cdfo_conv3x3_c64_ws_offmask(_vp(src), B, H, W, _vp(pc.wh), pc.CoutP16, _vp(pc.bias), pc.Cout, _vp(offset), _vp(mask),
                                                 _vp(flow), C.c_longlong(2 * H * W), float(mag), int(accumulate), _stream()),
          "cdfo_conv3x3_c64_ws_offmask")


def conv3x3_ws_res(src: torch.Tensor, pc: PackedConv, *, res1: torch.Tensor, res2: Optional[torch.Tensor] = None,
                   act: int = ACT_NONE, out: Optional[torch.Tensor] = None,
                   out2_cp16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Residual form of conv3x3_ws: fp32 pixel-major act(conv + bias) + res1 (+ res2); optionally also the fp16
    chunk-planar copy of the result (out2_cp16 [B,Cout/16,H,W,16]).  res2 may be an ImageMap (one launch: ws_res_map_ok)."""
    B, _, H, W = _chk_cp16(src, "conv3x3_ws_res")
    if pc.wh is None or pc.Cin != 64 or pc.ks != 3 or pc.Cout % 64:
        raise ValueError("conv3x3_ws_res: needs a 3x3 weight with 64 input channels and Cout % 64 == 0")
    if out is None:
        out = empty_act(B, H, W, pc.Cout, src.device)
    _, _, _, _, ldo = _chk_act(out, "out")
    lds = _bind_res(res1, res2, B, H, W, pc.Cout)
    if out2_cp16 is not None and (out2_cp16.dtype != torch.float16 or not out2_cp16.is_contiguous()
                                  or tuple(out2_cp16.shape) != (B, pc.Cout // 16, H, W, 16)):
        raise ValueError("conv3x3_ws_res: out2_cp16 must be a contiguous fp16 [B,Cout/16,H,W,16] tensor")
    if _is_map(res2):
        if not ws_res_map_ok(B, H, W):
            raise ValueError("conv3x3_ws_res: a mapped res2 needs a batch that one launch takes (ws_res_map_ok)")
        Bi, s_b, s_g = res2.triple()
        check(_lib.lib().cdfo_conv3x3_c64_ws_res_map(
            _vp(src), B, H, W, _vp(pc.wh), pc.CoutP16, _vp(pc.bias), pc.Cout, act, _vp(out), ldo, _vp(res1), lds[0], _vp(res2), lds[1],
            Bi, C.c_longlong(s_b), C.c_longlong(s_g), _vp(out2_cp16), _stream()), "cdfo_conv3x3_c64_ws_res_map")
        return out
    for sl in _batch_slices(B, H, W, "conv3x3_ws_res"):
        check(_lib.lib().cdfo_conv3x3_c64_ws_res(
            _vp(src[sl]), sl.stop - sl.start, H, W, _vp(pc.wh), pc.CoutP16, _vp(pc.bias), pc.Cout, act, _vp(out[sl]), ldo,
            _vp(res1[sl]), lds[0], _vp(None if res2 is None else res2[sl]), lds[1],
            _vp(None if out2_cp16 is None else out2_cp16[sl]), _stream()), "cdfo_conv3x3_c64_ws_res")
    return out


def ws_res_map_ok(B: int, H: int, W: int) -> bool:
    """conv3x3_ws_res takes a mapped res2 where the batch is one launch (the map counts images from the launch's first)."""
    return 4 * H * W * 32 < (1 << 31) and len(list(_batch_slices(B, H, W, "conv3x3_ws_res"))) == 1


def from_cp16(t: torch.Tensor) -> torch.Tensor:
    """chunk-planar [B,C/16,H,W,16] -> pixel-major [B,H,W,C] (torch ops; tests and tools only)."""
    B, nc, H, W, _ = t.shape
    return t.permute(0, 2, 3, 1, 4).reshape(B, H, W, nc * 16)


def sparse_taps_f16(pc: PackedConv) -> torch.Tensor:
    """fp16 packing [Cin/16][9][2][CoutP][8] + tap_mask -> [Cin/16][4][2][CoutP][8]: each chunk's four active taps in
    ascending order (the weight layout cdfo_conv3x3_ring reads when a tap mask is given)."""
    nc = pc.Cin // 16
    masks = pc.tap_mask.tolist()
    idx = []
    for m in masks:
        taps = [t for t in range(9) if (m >> t) & 1]
        if m not in (0x1B, 0x36, 0xD8, 0x1B0):
            raise ValueError("sparse_taps_f16: every chunk's active taps must be a 2x2 window of the 3x3 stencil")
        idx.append(taps)
    idx = torch.tensor(idx, dtype=torch.long, device=pc.wh.device)                  # [nc,4]
    w = pc.wh.view(nc, 9, 2 * pc.CoutP16 * 8)
    return torch.gather(w, 1, idx[:, :, None].expand(nc, 4, w.shape[2])).contiguous().view(-1)


def conv_ring(src: torch.Tensor, pc: PackedConv, *, act: int = ACT_NONE, res1: Optional[torch.Tensor] = None,
              res2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              out_f16: bool = False, out2_cp16: Optional[torch.Tensor] = None,
              res_up2: Optional[torch.Tensor] = None, plane_wrap: int = 0, dbg: int = 0,
              out2_hl: bool = False, src_halfsplit: bool = False) -> torch.Tensor:
    """3x3/s1/p1 convolution of an fp16 chunk-planar source [B,Cin/16,H,W,16] on the LDS-DMA ring kernel
    (Block_.body[2] and the composed stride-2 convolution).  Result: pixel-major fp32 (or fp16) [B,H,W,Cout]."""
    B, nc, H, W = _chk_cp16(src, "conv_ring", None)
    if pc.wh is None or pc.ks != 3 or (pc.Cin != nc * 16 and not (plane_wrap == nc and pc.Cin % 16 == 0 and pc.Cin > nc * 16)):
        raise ValueError("conv_ring: weight does not match the source")
    a, out = _conv_args(src, pc, pad=1, act=act, cp16=True, out=out, out_f16=out_f16)
    a.CoutP, a.prec = pc.CoutP16, PREC_FP16 | (dbg << 8)
    if pc.tap_mask is not None:
        if pc.wh_sparse is None:
            pc.wh_sparse = sparse_taps_f16(pc)
        a.w, a.tap_mask = pc.wh_sparse.data_ptr(), pc.tap_mask.data_ptr()
    else:
        a.w = pc.wh.data_ptr()
    a.src_plane_wrap = plane_wrap
    a.src_halfsplit = int(src_halfsplit)
    _bind_res(res1, None if dbg & 16 else res2, B, H, W, pc.Cout, a)
    if res_up2 is not None:         # half-resolution residual, added after bilinear x2
        rb, rh, rw, rc, rld = _chk_act(res_up2, "res_up2")
        if (rb, rh * 2, rw * 2) != (B, H, W) or rc < pc.Cout:
            raise ValueError(f"res_up2 shape {tuple(res_up2.shape)} is not the half-resolution of the conv output")
        a.res_up2, a.ldru = res_up2.data_ptr(), rld
    if dbg & 16:                    # developer timeline probe: res2 carries a u64 stamp buffer (see conv3x3_ring.hip)
        if res2 is None or res2.dtype != torch.int64:
            raise ValueError("conv_ring: dbg 16 expects res2 = int64 stamp buffer [workgroups, 8, 4, 10]")
        a.res2, a.ldr2 = res2.data_ptr(), 0
    if out2_cp16 is not None:       # second, fp16 chunk-planar copy of the result (the next Block_'s body[0] source)
        npl = (2 if out2_hl else 1) * (pc.Cout // 16)     # out2_hl: hi | lo planes (the source of a split-fp16 convolution)
        if (out2_cp16.dtype != torch.float16 or tuple(out2_cp16.shape) != (B, npl, H, W, 16)
                or not out2_cp16.is_contiguous()):
            raise ValueError("conv_ring: out2_cp16 must be a contiguous fp16 [B,Cout/16 (x2 with out2_hl),H,W,16] tensor")
        a.out2_cp16, a.out2_lo = out2_cp16.data_ptr(), int(out2_hl)
    check(_lib.lib().cdfo_conv3x3_ring(C.byref(a), _stream()), "cdfo_conv3x3_ring")
    return out


# ----------------------------------------------------------------------------------------------- pointwise


def swap_outer(x: torch.Tensor, B: int, N: int) -> torch.Tensor:
    """x: dense [B*N, ...] -> dense [N*B, ...] (out[n*B+b] = in[b*N+n])."""
    x = x if x.is_contiguous() else x.contiguous()
    out = torch.empty_like(x)
    block = x.numel() // (B * N)
    check(_lib.lib().cdfo_swap_outer(_vp(x), _vp(out), B, N, C.c_longlong(block), _stream()), "cdfo_swap_outer")
    return out


_MV_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.int8: 4, torch.uint8: 5,
              torch.int16: 6, torch.int32: 7, torch.int64: 8}        # CDFO_MV_* of include/cdfo_hip.h


def seq_flows(mv: torch.Tensor, i0: int, K: int, Hp: int, Wp: int) -> torch.Tensor:
    """mv: the decoder's motion field [T,H,W,3] of one sequence (device) -> the flows of centre frames i0 .. i0+K-1,
    [K,7,2,Hp,Wp] fp32: streaming.mv2mvs + modify_mv_for_end_frames of each centre, bit for bit, in one launch."""
    if not mv.is_cuda or mv.dim() != 4 or mv.shape[3] != 3 or mv.dtype not in _MV_DTYPES:
        raise ValueError(f"seq_flows: a device tensor [T,H,W,3] of a real dtype expected, got {mv.dtype} {tuple(mv.shape)}")
    mv = mv if mv.is_contiguous() else mv.contiguous()
    T, H, W, _ = mv.shape
    out = torch.empty((K, 7, 2, Hp, Wp), dtype=torch.float32, device=mv.device)
    check(_lib.lib().cdfo_seq_flows(_vp(mv), _MV_DTYPES[mv.dtype], T, H, W, i0, K, Hp, Wp, _vp(out), _stream()), "cdfo_seq_flows")
    return out


def gather_frames(src: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[j] = src[idx[j]] over the frames src[i] of a dense tensor; idx: int32 on the device.  Returns [len(idx), *src.shape[1:]]."""
    if not src.is_cuda or not src.is_contiguous() or idx.dtype != torch.int32 or idx.device != src.device or idx.dim() != 1 \
            or not idx.is_contiguous():
        raise ValueError("gather_frames: a dense device tensor and a dense int32 index vector on the same device expected")
    n = int(idx.shape[0])
    frame_bytes = src[0].numel() * src.element_size()
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    elif out.dtype != src.dtype or out.numel() != n * src[0].numel() or not out.is_contiguous() or out.device != src.device:
        raise ValueError("gather_frames: out must be a dense tensor of len(idx) frames of src's dtype")
    check(_lib.lib().cdfo_gather_frames(_vp(src), int(src.shape[0]), _vp(idx), n, C.c_longlong(frame_bytes), _vp(out), _stream()),
          "cdfo_gather_frames")
    return out


def live_planes(lr: torch.Tensor, ufs: torch.Tensor, pms: torch.Tensor, rms: torch.Tensor, table: torch.Tensor, K: int, E: int,
                Hp: int, Wp: int, peak: int, want_r: bool = True, want_r_new: bool = True):
    """Every plane a chunk reads from the sample rings of live inference, in one launch (cdfo_live_planes).  lr, ufs: rings
    [cap,H,W] uint8 (peak <= 255) or uint16; pms: [cap,H,W] uint8; rms: [cap,H,W] fp32; table: device int32 [14K + 2E] of ring slots
    (win_frame[K,7], win_prior[K,7], new_frame[E], new_prior[E]).  Returns (x, r, u, lr_new, p_new, r_new): x, r, u [K,7,Hp,Wp],
    the others [E,Hp,Wp], fp32 = sample / peak (pms / 255) zero padded; r / r_new are None when not wanted."""
    cap, H, W = (int(v) for v in lr.shape) if lr.dim() == 3 else (0, 0, 0)
    sample = torch.uint8 if peak <= 255 else torch.uint16
    for name, t, dt in (("lr", lr, sample), ("ufs", ufs, sample), ("pms", pms, torch.uint8), ("rms", rms, torch.float32)):
        if not t.is_cuda or t.device != lr.device or t.dtype != dt or tuple(t.shape) != (cap, H, W) or not t.is_contiguous():
            raise ValueError(f"live_planes: {name} must be a dense device ring [cap,H,W] of {dt}, got {t.dtype} {tuple(t.shape)}")
    if table.dtype != torch.int32 or table.device != lr.device or table.dim() != 1 or not table.is_contiguous() \
            or table.numel() != 14 * K + 2 * E:
        raise ValueError(f"live_planes: table must be a dense device int32 vector of 14 K + 2 E = {14 * K + 2 * E} slots")
    new = lambda n, want=True: torch.empty((n, Hp, Wp), dtype=torch.float32, device=lr.device) if want else None
    x, r, u = new(7 * K), new(7 * K, want_r), new(7 * K)
    lr_new, p_new, r_new = new(E), new(E), new(E, want_r_new)
    check(_lib.lib().cdfo_live_planes(_vp(lr), _vp(ufs), _vp(pms), _vp(rms), lr.element_size(), cap, H, W, _vp(table), K, E, Hp, Wp,
                                      int(peak), _vp(x), _vp(r), _vp(u), _vp(lr_new), _vp(p_new), _vp(r_new), _stream()),
          "cdfo_live_planes")
    win = lambda t: None if t is None else t.view(K, 7, Hp, Wp)
    return win(x), win(r), win(u), lr_new, p_new, r_new


def seq_flows_ring(ring: torch.Tensor, i0: int, K: int, T_known: int, Hp: int, Wp: int) -> torch.Tensor:
    """`seq_flows` reading the fp32 ring [cap,H,W,3] of live inference (entry e in slot e mod cap) for centres i0 .. i0+K-1.
    T_known: the sequence's length, or 0 while the stream is open (no end rule applies, T > 1).  -> [K,7,2,Hp,Wp] fp32."""
    if not ring.is_cuda or ring.dim() != 4 or ring.shape[3] != 3 or ring.dtype != torch.float32 or not ring.is_contiguous():
        raise ValueError(f"seq_flows_ring: a dense fp32 device ring [cap,H,W,3] expected, got {ring.dtype} {tuple(ring.shape)}")
    cap, H, W, _ = ring.shape
    out = torch.empty((K, 7, 2, Hp, Wp), dtype=torch.float32, device=ring.device)
    check(_lib.lib().cdfo_seq_flows_ring(_vp(ring), cap, H, W, i0, K, T_known, Hp, Wp, _vp(out), _stream()), "cdfo_seq_flows_ring")
    return out


def seq_flows_ra(mv0: torch.Tensor, mv1: torch.Tensor, i0: int, K: int, Hp: int, Wp: int) -> torch.Tensor:
    """`seq_flows` for the random-access field: mv0, mv1: both lists' motion fields [T,H,W,3] of one sequence (device, one dtype) ->
    the flows of centre frames i0 .. i0+K-1, [K,7,2,Hp,Wp] fp32: streaming.mv2mvs_ra + modify_mv_for_end_frames of each centre,
    bit for bit, in one launch (cdfo_seq_flows_ra)."""
    check_ra_lists("seq_flows_ra", mv0, mv1)
    if not mv0.is_cuda or mv0.dim() != 4 or mv0.shape[3] != 3 or mv0.dtype not in _MV_DTYPES:
        raise ValueError(f"seq_flows_ra: device tensors [T,H,W,3] of a real dtype expected, got {mv0.dtype} {tuple(mv0.shape)}")
    mv0, mv1 = (m if m.is_contiguous() else m.contiguous() for m in (mv0, mv1))
    T, H, W, _ = mv0.shape
    out = torch.empty((K, 7, 2, Hp, Wp), dtype=torch.float32, device=mv0.device)
    check(_lib.lib().cdfo_seq_flows_ra(_vp(mv0), _vp(mv1), _MV_DTYPES[mv0.dtype], T, H, W, i0, K, Hp, Wp, _vp(out), _stream()),
          "cdfo_seq_flows_ra")
    return out


def seq_flows_ra_ring(ring0: torch.Tensor, ring1: torch.Tensor, i0: int, K: int, T_known: int, Hp: int, Wp: int) -> torch.Tensor:
    """`seq_flows_ra` reading the two fp32 rings [cap,H,W,3] of live inference (entry e of both lists in slot e mod cap) for centres
    i0 .. i0+K-1.  T_known: the sequence's length, or 0 while the stream is open (no end rule applies, T > 1).  -> [K,7,2,Hp,Wp]."""
    check_ra_lists("seq_flows_ra_ring", ring0, ring1)
    if not ring0.is_cuda or ring0.dim() != 4 or ring0.shape[3] != 3 or ring0.dtype != torch.float32 or not ring0.is_contiguous() \
            or not ring1.is_contiguous():
        raise ValueError(f"seq_flows_ra_ring: dense fp32 device rings [cap,H,W,3] expected, got {ring0.dtype} {tuple(ring0.shape)}")
    cap, H, W, _ = ring0.shape
    out = torch.empty((K, 7, 2, Hp, Wp), dtype=torch.float32, device=ring0.device)
    check(_lib.lib().cdfo_seq_flows_ra_ring(_vp(ring0), _vp(ring1), cap, H, W, i0, K, T_known, Hp, Wp, _vp(out), _stream()),
          "cdfo_seq_flows_ra_ring")
    return out


QUANT_MODES = {"trunc": 0, "nearest": 1}        # CDFO_QUANT_* of include/cdfo_hip.h


def _sample_frames(t: torch.Tensor, name: str, dtype: torch.dtype):
    """A stack of uint8 or uint16 frames [N,H,W] (or [H,W]) with contiguous rows -> (tensor [N,H,W], N, H, W, pitch, frame stride),
    in samples; pitch and stride may exceed W and H * pitch (a view of larger frames is read in place)."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if not t.is_cuda or t.dtype != dtype or t.dim() != 3 or t.stride(2) != 1 or t.stride(1) < t.shape[2] or t.stride(0) < 0:
        kind = str(dtype).split(".")[-1]
        raise ValueError(f"{name}: a device {kind} tensor [N,H,W] with contiguous rows expected, got {t.dtype} {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return t, int(t.shape[0]), int(t.shape[1]), int(t.shape[2]), int(t.stride(1)), int(t.stride(0))


def sample_dtype(peak: Optional[int], given: Optional[torch.dtype], name: str):
    """(dtype, peak) of the samples of a kernel call: ``peak`` None or 255 with 8-bit tensors is the 8-bit kernel; a peak in
    1 .. 65535 beyond that (or any peak with uint16 tensors, which need one) is the 16-bit kernel."""
    if peak is not None and (isinstance(peak, bool) or not isinstance(peak, int) or not 1 <= peak <= 65535):
        raise ValueError(f"{name}: peak must be an integer in 1 .. 65535, got {peak!r}")
    if given is None:
        given = torch.uint8 if peak in (None, 255) else torch.uint16
    if given == torch.uint8:
        if peak not in (None, 255):
            raise ValueError(f"{name}: 8-bit samples have the peak 255, got {peak}")
        return torch.uint8, 255
    if given == torch.uint16:
        if peak is None:
            raise ValueError(f"{name}: uint16 samples need their peak (2**depth - 1)")
        return torch.uint16, peak
    raise ValueError(f"{name}: uint8 or uint16 samples expected, got {given}")


def _write_samples(name: str, src: torch.Tensor, planes: tuple, N: int, Ho: int, Wo: int, kind: torch.dtype, peak: int, mode: tuple,
                   gt: Optional[torch.Tensor], crop: int, dst: Optional[torch.Tensor], on: str, one_per: str):
    """The common end of `finish_frames` and `chroma_up4`, cdfo_<name> or its _u16 form by ``kind``: ``planes``, the entry point's
    arguments up to the source's sizes; a dense ``dst`` [N,Ho,Wo] of ``kind`` on ``src``'s device, validated or allocated; ``gt``
    bound as a stack of N frames; the [N,1024] int64 partial sums, added up per frame.  -> (dst, sse or None)."""
    if dst is None:
        dst = torch.empty((N, Ho, Wo), dtype=kind, device=src.device)
    elif dst.dtype != kind or tuple(dst.shape) != (N, Ho, Wo) or not dst.is_contiguous() or dst.device != src.device:
        raise ValueError(f"{name}: dst must be a dense {kind} [{N},{Ho},{Wo}] tensor on {on}'s device")
    part, nb = None, C.c_int(0)
    g = gp = gs = gh = gw = None
    if gt is not None:
        g, n, gh, gw, gp, gs = _sample_frames(gt, f"{name}: gt", kind)
        if n != N or g.device != src.device:
            raise ValueError(f"{name}: gt must hold {one_per} = {N}) on {on}'s device, got {n}")
        part = torch.empty((N, 1024), dtype=torch.int64, device=src.device)
    entry = f"cdfo_{name}_u16" if kind == torch.uint16 else f"cdfo_{name}"
    with on_device(src):
        check(getattr(_lib.lib(), entry)(*planes, _vp(dst), *((peak,) if kind == torch.uint16 else ()), *mode, _vp(g), gp or 0,
                                         C.c_longlong(gs or 0), gh or 0, gw or 0, int(crop), _vp(part),
                                         0 if part is None else part.numel(), C.byref(nb), _stream()), entry)
    if part is None:
        return dst, None
    # the kernel packs its partial sums as [N][nblocks]; integers, so the sum is exact in any order
    return dst, part.view(-1)[:N * nb.value].view(N, nb.value).sum(dim=1)


def finish_frames(out: torch.Tensor, H: int, W: int, gt: Optional[torch.Tensor] = None, crop: int = 4, mode: str = "trunc",
                  dst: Optional[torch.Tensor] = None, peak: int = 255):
    """out: the fp32 output of a chunk, [K,1,>=4H,>=4W] or [K,>=4H,>=4W] with contiguous rows (the padded tensor, read in place)
    -> (u8 [K,4H,4W], sse): clamp to [0,1] (NaN -> 0), fp32 * 255, truncation (``mode="trunc"``, the reference's writer) or
    round-to-nearest-even (``"nearest"``).  With ``gt`` (uint8 [K,Hgt,Wgt], device) sse is the int64 [K] sum of (u8 - gt)^2 over the
    common min(4H, Hgt) x min(4W, Wgt) less ``crop`` border pixels, exact; else None.  ``dst``: an optional dense uint8 [K,4H,4W]
    destination.  ``peak``: 255 with uint8 ``dst`` / ``gt`` (or neither) is the call above; any other peak in 1 .. 65535, or uint16
    ``dst`` / ``gt``, multiplies by the peak and gives uint16 frames (cdfo_finish_frames_u16)."""
    given = dst.dtype if dst is not None else gt.dtype if gt is not None else None
    kind, peak = sample_dtype(peak, given, "finish_frames")
    if mode not in QUANT_MODES:
        raise ValueError(f"finish_frames: mode must be one of {sorted(QUANT_MODES)}, got {mode!r}")
    if out.dim() == 4 and out.shape[1] == 1:
        out = out[:, 0]
    Ho, Wo = 4 * int(H), 4 * int(W)
    if not out.is_cuda or out.dtype != torch.float32 or out.dim() != 3 or out.stride(2) != 1 or out.shape[1] < Ho or out.shape[2] < Wo \
            or Ho <= 0 or Wo <= 0 or out.stride(1) < out.shape[2] or out.stride(0) < 0:
        raise ValueError(f"finish_frames: a device fp32 tensor [K,1,>={Ho},>={Wo}] with contiguous rows expected, got {out.dtype} "
                         f"{tuple(out.shape)} strides {out.stride()}")
    K = int(out.shape[0])
    planes = (_vp(out), int(out.stride(1)), C.c_longlong(out.stride(0)), K, Ho, Wo)
    return _write_samples("finish_frames", out, planes, K, Ho, Wo, kind, peak, (QUANT_MODES[mode],), gt, crop, dst, "out",
                          "one frame per output frame (K")


def chroma_up4(src: torch.Tensor, gt: Optional[torch.Tensor] = None, crop: int = 2, dst: Optional[torch.Tensor] = None,
               peak: Optional[int] = None):
    """src: 8-bit planes [N,h,w] (or [h,w]) on the device with contiguous rows, read in place (pitch and plane stride may exceed the
    plane) -> (u8 [N,4h,4w], sse): the centre-aligned x4 cubic of include/cdfo_hip.h, in integers, bit-exact against its numpy
    statement.  With ``gt`` (uint8 [N,Hgt,Wgt], device) sse is the int64 [N] sum of (u8 - gt)^2 over the common min(4h, Hgt) x
    min(4w, Wgt) less ``crop`` border pixels, exact; else None.  ``dst``: an optional dense uint8 [N,4h,4w] destination.
    uint16 planes (``src``, ``gt``, ``dst`` alike) need ``peak``, 2**depth - 1: the same filter clamped to [0, peak]
    (cdfo_chroma_up4_u16)."""
    kind, peak = sample_dtype(peak, src.dtype, "chroma_up4")
    s, N, h, w, sp, ss = _sample_frames(src, "chroma_up4: src", kind)
    if h <= 0 or w <= 0 or N <= 0:
        raise ValueError(f"chroma_up4: src holds no pixels: {tuple(s.shape)}")
    return _write_samples("chroma_up4", s, (_vp(s), sp, C.c_longlong(ss), N, h, w), N, 4 * h, 4 * w, kind, peak, (), gt, crop, dst,
                          "src", "one plane per source plane (N")


# ---- NIQE's block features (csrc/niqe.hip); cdfo_amd/metrics.py builds the window and the table and puts the launches together ----
def _f64_out(out: Optional[torch.Tensor], shape: tuple, like: torch.Tensor, name: str) -> torch.Tensor:
    """A dense fp64 destination of ``shape`` on ``like``'s device: ``out`` validated, or a new tensor."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=like.device)
    if out.dtype != torch.float64 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != like.device:
        raise ValueError(f"{name}: out must be a dense fp64 {list(shape)} tensor on the source's device, got {out.dtype} "
                         f"{tuple(out.shape)} strides {out.stride()} on {out.device}")
    return out


def _metric_peak(name: str, peak) -> int:
    """The peak of the 16-bit form of a metric's sample kernel, 2**depth - 1: an integer in 1 .. 65535 (`streaming.check_peak`'s rule)."""
    if isinstance(peak, bool) or not isinstance(peak, int) or not 1 <= peak <= 65535:
        raise ValueError(f"{name}: peak must be an integer in 1 .. 65535, got {peak!r}")
    return peak


def _niqe_region(name: str, H: int, W: int, rows: int, cols: int, N: int):
    rows, cols = int(rows), int(cols)
    if N <= 0 or not 0 < rows <= H or not 0 < cols <= W:
        raise ValueError(f"{name}: a region of {rows} x {cols} does not lie in {N} frames of {H} x {W}")
    return rows, cols


def niqe_mscn(src: torch.Tensor, rows: int, cols: int, window, out: Optional[torch.Tensor] = None,
              peak: Optional[int] = None) -> torch.Tensor:
    """src: uint8 or fp64 frames [K,H,W] (or [H,W]) on the device with contiguous rows, read in place (pitch and frame stride may
    exceed the frame) -> fp64 [K,rows,cols]: the MSCN map of the top-left ``rows`` x ``cols``, (x - mu) / (sigma + 1) under the 7 x 7
    ``window`` (49 fp64 values, a host array), the samples beyond the REGION's edge replaced by the edge sample.  ``peak``: the frames
    are uint16 samples of that peak, read as x = 255 v / peak (cdfo_niqe_mscn_u16)."""
    if peak is not None:
        peak, kind = _metric_peak("niqe_mscn", peak), torch.uint16
    elif src.dtype not in (torch.uint8, torch.float64):
        raise ValueError(f"niqe_mscn: uint8 or fp64 frames expected, got {src.dtype}")
    else:
        kind = src.dtype
    s, N, H, W, sp, ss = _sample_frames(src, "niqe_mscn: src", kind)
    rows, cols = _niqe_region("niqe_mscn", H, W, rows, cols, N)
    win = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    if win.size != 49:
        raise ValueError(f"niqe_mscn: a window of 7 x 7 values expected, got {win.size}")
    out = _f64_out(out, (N, rows, cols), s, "niqe_mscn")
    entry = "cdfo_niqe_mscn_u16" if peak is not None else "cdfo_niqe_mscn_u8" if src.dtype == torch.uint8 else "cdfo_niqe_mscn_f64"
    with on_device(s):
        check(getattr(_lib.lib(), entry)(_vp(s), sp, C.c_longlong(ss), N, rows, cols, C.c_void_p(win.ctypes.data), _vp(out),
                                         *(() if peak is None else (peak,)), _stream()), entry)
    return out


def niqe_half(src: torch.Tensor, rows: int, cols: int, out: Optional[torch.Tensor] = None, peak: Optional[int] = None) -> torch.Tensor:
    """src: uint8 frames as `niqe_mscn` takes them -> fp64 [K,rows/2,cols/2]: the top-left ``rows`` x ``cols`` (even) at half size,
    the fixed 8 taps of include/cdfo_hip.h on x / 255 down the columns, then along the rows, times 255; not rounded.  ``peak``: as
    `niqe_mscn`'s (cdfo_niqe_half_u16)."""
    if peak is not None:
        peak = _metric_peak("niqe_half", peak)
    s, N, H, W, sp, ss = _sample_frames(src, "niqe_half: src", torch.uint8 if peak is None else torch.uint16)
    rows, cols = _niqe_region("niqe_half", H, W, rows, cols, N)
    if rows % 2 or cols % 2 or min(rows, cols) < 8:
        raise ValueError(f"niqe_half: an even region of at least 8 x 8 expected, got {rows} x {cols}")
    out = _f64_out(out, (N, rows // 2, cols // 2), s, "niqe_half")
    with on_device(s):
        if peak is None:
            check(_lib.lib().cdfo_niqe_half(_vp(s), sp, C.c_longlong(ss), N, rows, cols, _vp(out), _stream()), "cdfo_niqe_half")
        else:
            check(_lib.lib().cdfo_niqe_half_u16(_vp(s), sp, C.c_longlong(ss), N, rows, cols, _vp(out), peak, _stream()), "cdfo_niqe_half_u16")
    return out


def niqe_block_sums(mscn: torch.Tensor, block: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mscn: dense fp64 [K,R,C], ``block`` divides R and C -> fp64 [K,nb,5,6]: per block (block (ih, iw) at iw * (R / block) + ih) and
    map -- x and its four products with a circular neighbour inside the block -- the counts of negative and of positive samples, the
    sums of squares over each, of magnitudes and of squares.  Fixed summation order: equal inputs give equal bits."""
    block = int(block)
    if not mscn.is_cuda or mscn.dtype != torch.float64 or mscn.dim() != 3 or not mscn.is_contiguous() or mscn.shape[0] == 0:
        raise ValueError(f"niqe_block_sums: a dense device fp64 tensor [K,R,C] expected, got {mscn.dtype} {tuple(mscn.shape)} strides "
                         f"{mscn.stride()}")
    N, R, Cc = (int(v) for v in mscn.shape)
    if not 2 <= block <= 96 or R < block or Cc < block or R % block or Cc % block:
        raise ValueError(f"niqe_block_sums: blocks of {block} (2 .. 96) do not tile {R} x {Cc}")
    out = _f64_out(out, (N, (R // block) * (Cc // block), 5, 6), mscn, "niqe_block_sums")
    with on_device(mscn):
        check(_lib.lib().cdfo_niqe_block_sums(_vp(mscn), N, R, Cc, block, _vp(out), _stream()), "cdfo_niqe_block_sums")
    return out


def niqe_features(sums: torch.Tensor, count: int, table: torch.Tensor, scale: int, out: torch.Tensor) -> torch.Tensor:
    """sums: dense fp64 [K,nb,5,6] of blocks of ``count`` samples; table: fp64 [2,9801] on the device (gam, r_gam) -> the 18 features of
    scale ``scale`` (0 or 1) of each block into its half of ``out``, dense fp64 [K,nb,36], which is returned."""
    if not sums.is_cuda or sums.dtype != torch.float64 or sums.dim() != 4 or tuple(sums.shape[2:]) != (5, 6) or not sums.is_contiguous() \
            or sums.shape[0] == 0 or sums.shape[1] == 0:
        raise ValueError(f"niqe_features: dense device fp64 sums [K,nb,5,6] expected, got {sums.dtype} {tuple(sums.shape)}")
    N, nb = int(sums.shape[0]), int(sums.shape[1])
    if table.dtype != torch.float64 or tuple(table.shape) != (2, 9801) or not table.is_contiguous() or table.device != sums.device:
        raise ValueError(f"niqe_features: the table must be a dense fp64 [2,9801] tensor on {sums.device}")
    if scale not in (0, 1) or int(count) <= 0:
        raise ValueError(f"niqe_features: scale 0 or 1 and a positive sample count expected, got {scale!r} and {count!r}")
    out = _f64_out(out, (N, nb, 36), sums, "niqe_features")
    with on_device(sums):
        check(_lib.lib().cdfo_niqe_features(_vp(sums), N, nb, int(count), _vp(table), int(scale), _vp(out), _stream()),
              "cdfo_niqe_features")
    return out


# ---- BRISQUE's features (csrc/brisque.hip); cdfo_amd/metrics.py builds the window and the table and puts the launches together ----
BRISQUE_STRIP = 16                                      # CDFO_BRISQUE_STRIP: rows per workgroup of `brisque_sums`


def brisque_mscn(src: torch.Tensor, window, out: Optional[torch.Tensor] = None, peak: Optional[int] = None) -> torch.Tensor:
    """src: uint8 or fp64 frames [K,H,W] (or [H,W]) on the device with contiguous rows, read in place (pitch and frame stride may
    exceed the frame) -> fp64 [K,H,W]: the MSCN map of the whole frame, (x - mu) / (sigma + 1) under the 7 x 7 ``window`` (49 fp64
    values, a host array) with the reference's epsilon 2^-23 under the root, the samples beyond the FRAME's edge zero.  ``peak``: the
    frames are uint16 samples of that peak, read as x = 255 v / peak (cdfo_brisque_mscn_u16)."""
    if peak is not None:
        peak, kind = _metric_peak("brisque_mscn", peak), torch.uint16
    elif src.dtype not in (torch.uint8, torch.float64):
        raise ValueError(f"brisque_mscn: uint8 or fp64 frames expected, got {src.dtype}")
    else:
        kind = src.dtype
    s, N, H, W, sp, ss = _sample_frames(src, "brisque_mscn: src", kind)
    if N <= 0 or H <= 0 or W <= 0:
        raise ValueError(f"brisque_mscn: no samples in {N} frames of {H} x {W}")
    win = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    if win.size != 49:
        raise ValueError(f"brisque_mscn: a window of 7 x 7 values expected, got {win.size}")
    out = _f64_out(out, (N, H, W), s, "brisque_mscn")
    entry = "cdfo_brisque_mscn_u16" if peak is not None else "cdfo_brisque_mscn_u8" if src.dtype == torch.uint8 else "cdfo_brisque_mscn_f64"
    with on_device(s):
        check(getattr(_lib.lib(), entry)(_vp(s), sp, C.c_longlong(ss), N, H, W, C.c_void_p(win.ctypes.data), _vp(out),
                                         *(() if peak is None else (peak,)), _stream()), entry)
    return out


def brisque_half(src: torch.Tensor, out: Optional[torch.Tensor] = None, peak: Optional[int] = None) -> torch.Tensor:
    """src: uint8 frames as `brisque_mscn` takes them, at least 8 x 8 -> fp64 [K,ceil(H/2),ceil(W/2)]: the frame at half size, the fixed
    8 taps of include/cdfo_hip.h on x itself down the columns, then along the rows, the edge sample repeated; odd sizes are legal;
    not rounded.  ``peak``: as `brisque_mscn`'s (cdfo_brisque_half_u16)."""
    if peak is not None:
        peak = _metric_peak("brisque_half", peak)
    s, N, H, W, sp, ss = _sample_frames(src, "brisque_half: src", torch.uint8 if peak is None else torch.uint16)
    if N <= 0 or min(H, W) < 8:
        raise ValueError(f"brisque_half: frames of at least 8 x 8 expected, got {N} of {H} x {W}")
    out = _f64_out(out, (N, (H + 1) // 2, (W + 1) // 2), s, "brisque_half")
    with on_device(s):
        if peak is None:
            check(_lib.lib().cdfo_brisque_half(_vp(s), sp, C.c_longlong(ss), N, H, W, _vp(out), _stream()), "cdfo_brisque_half")
        else:
            check(_lib.lib().cdfo_brisque_half_u16(_vp(s), sp, C.c_longlong(ss), N, H, W, _vp(out), peak, _stream()), "cdfo_brisque_half_u16")
    return out


def brisque_sums(mscn: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mscn: dense fp64 [K,H,W] -> fp64 [K,G,5,6], G = ceil(H / 16): per strip of 16 rows and map -- x and its four products with the
    partner at (r, c-1), (r-1, c), (r-1, c-1), (r+1, c-1), circular over the WHOLE frame -- the counts of negative and of positive
    samples, the sums of squares over each, of magnitudes and of squares.  G depends on the shape alone and the summation order is
    fixed: equal inputs give equal bits on any device."""
    if not mscn.is_cuda or mscn.dtype != torch.float64 or mscn.dim() != 3 or not mscn.is_contiguous() or mscn.shape[0] == 0 \
            or min(mscn.shape[1:]) < 2:
        raise ValueError(f"brisque_sums: a dense device fp64 tensor [K,H,W] of at least 2 x 2 expected, got {mscn.dtype} "
                         f"{tuple(mscn.shape)} strides {mscn.stride()}")
    N, H, W = (int(v) for v in mscn.shape)
    out = _f64_out(out, (N, (H + BRISQUE_STRIP - 1) // BRISQUE_STRIP, 5, 6), mscn, "brisque_sums")
    with on_device(mscn):
        check(_lib.lib().cdfo_brisque_sums(_vp(mscn), N, H, W, _vp(out), _stream()), "cdfo_brisque_sums")
    return out


def brisque_features(partials: torch.Tensor, count: int, table: torch.Tensor, scale: int, out: torch.Tensor) -> torch.Tensor:
    """partials: dense fp64 [K,G,5,6] of maps of ``count`` samples; table: fp64 [3,9801] on the device (gam, r_gam, r_ggd) -> the 18
    features of scale ``scale`` (0 or 1) of each frame into its half of ``out``, dense fp64 [K,36], which is returned."""
    if not partials.is_cuda or partials.dtype != torch.float64 or partials.dim() != 4 or tuple(partials.shape[2:]) != (5, 6) \
            or not partials.is_contiguous() or partials.shape[0] == 0 or partials.shape[1] == 0:
        raise ValueError(f"brisque_features: dense device fp64 partials [K,G,5,6] expected, got {partials.dtype} {tuple(partials.shape)}")
    N, G = int(partials.shape[0]), int(partials.shape[1])
    if table.dtype != torch.float64 or tuple(table.shape) != (3, 9801) or not table.is_contiguous() or table.device != partials.device:
        raise ValueError(f"brisque_features: the table must be a dense fp64 [3,9801] tensor on {partials.device}")
    if scale not in (0, 1) or int(count) <= 0:
        raise ValueError(f"brisque_features: scale 0 or 1 and a positive sample count expected, got {scale!r} and {count!r}")
    out = _f64_out(out, (N, 36), partials, "brisque_features")
    with on_device(partials):
        check(_lib.lib().cdfo_brisque_features(_vp(partials), N, G, int(count), _vp(table), int(scale), _vp(out), _stream()),
              "cdfo_brisque_features")
    return out


# ---- tOF's Farneback flow (csrc/tof.hip); cdfo_amd/metrics.py builds the taps and puts the stages together ----
TOF_MIN, TOF_MAX_TAPS, TOF_STRIP = 32, 19, 16           # CDFO_TOF_MIN, CDFO_TOF_MAX_TAPS, CDFO_TOF_STRIP


def _tof_f64(t: torch.Tensor, dims: int, name: str) -> tuple:
    """The shape of a dense device fp64 tensor of ``dims`` dimensions with no empty one."""
    if not t.is_cuda or t.dtype != torch.float64 or t.dim() != dims or not t.is_contiguous() or 0 in t.shape:
        raise ValueError(f"{name}: a dense device fp64 tensor of {dims} dimensions expected, got {t.dtype} {tuple(t.shape)} "
                         f"strides {t.stride()}")
    return tuple(int(v) for v in t.shape)


def tof_level(prev: torch.Tensor, cur: torch.Tensor, h: int, w: int, taps, first: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, peak: Optional[int] = None) -> torch.Tensor:
    """prev, cur: uint8 frames [K,H,W] (or [H,W]) on the device with contiguous rows, read in place -> fp64 [K,2,h,w]: per pair the
    level image of its previous frame and of its current one, smoothed with the odd number of ``taps`` (a host array, at most 19)
    down the columns and along the rows, reflect-101, then resized to h x w bilinearly.  Pair j is (prev[j], cur[j]); with ``first``
    (uint8 [H,W]) it is (first, cur[0]) for j = 0 and (prev[j - 1], cur[j]) beyond, so ``prev`` may then be ``cur`` itself.  ``peak``:
    all frames are uint16 samples of that peak, read as x = 255 v / peak (cdfo_tof_level_u16)."""
    kind = torch.uint8 if peak is None else torch.uint16
    if peak is not None:
        peak = _metric_peak("tof_level", peak)
    c, N, H, W, cp, cs = _sample_frames(cur, "tof_level: cur", kind)
    p, Np, Hp, Wp, pp, ps = _sample_frames(prev, "tof_level: prev", kind)
    f = fp = None
    if first is not None:
        f, Nf, Hf, Wf, fp, _ = _sample_frames(first, "tof_level: first", kind)
        if (Nf, Hf, Wf) != (1, H, W) or f.device != c.device:
            raise ValueError(f"tof_level: first must be one frame of {H} x {W} on cur's device, got {tuple(f.shape)}")
    if N <= 0 or (Hp, Wp) != (H, W) or Np < (N if first is None else N - 1) or p.device != c.device:
        raise ValueError(f"tof_level: prev {tuple(p.shape)} does not pair with cur {tuple(c.shape)}")
    h, w = int(h), int(w)
    if min(H, W) < TOF_MIN or not 0 < h <= H or not 0 < w <= W:
        raise ValueError(f"tof_level: frames of at least {TOF_MIN} x {TOF_MIN} and a level no larger expected, got {H} x {W} -> {h} x {w}")
    t = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
    if not 3 <= t.size <= TOF_MAX_TAPS or t.size % 2 == 0 or t.size // 2 >= min(H, W):
        raise ValueError(f"tof_level: an odd number of taps in 3 .. {TOF_MAX_TAPS} expected, got {t.size}")
    out = _f64_out(out, (N, 2, h, w), c, "tof_level")
    entry = "cdfo_tof_level_u8" if peak is None else "cdfo_tof_level_u16"
    with on_device(c):
        check(getattr(_lib.lib(), entry)(_vp(p), pp, C.c_longlong(ps), _vp(c), cp, C.c_longlong(cs), _vp(f), fp or 0, N, H, W, h, w,
                                         C.c_void_p(t.ctypes.data), int(t.size), _vp(out), *(() if peak is None else (peak,)), _stream()),
              entry)
    return out


def tof_polyexp(img: torch.Tensor, kernels, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """img: dense fp64 [...,h,w] -> fp64 [...,5,h,w] = (b_x, b_y, a_xx, a_yy, a_xy), the edge sample repeated.  ``kernels``: 37 fp64
    values on the host, the taps g, x g, x^2 g (11 each) and the inverse Gram matrix's entries [1][1], [0][3], [3][3], [5][5]."""
    shape = _tof_f64(img, img.dim(), "tof_polyexp: img")
    if len(shape) < 2:
        raise ValueError(f"tof_polyexp: images [...,h,w] expected, got {shape}")
    k = np.ascontiguousarray(kernels, dtype=np.float64).reshape(-1)
    if k.size != 37:
        raise ValueError(f"tof_polyexp: 37 kernel values expected, got {k.size}")
    h, w = shape[-2:]
    out = _f64_out(out, shape[:-2] + (5, h, w), img, "tof_polyexp")
    with on_device(img):
        check(_lib.lib().cdfo_tof_polyexp(_vp(img), int(np.prod(shape[:-2], dtype=np.int64)), h, w, C.c_void_p(k.ctypes.data), _vp(out),
                                          _stream()), "cdfo_tof_polyexp")
    return out


def tof_matrices(R: torch.Tensor, flow: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """R: dense fp64 [N,2,5,h,w] (per pair the previous frame's expansion, then the current one's); flow: dense fp64 [N,h,w,2] or
    None for zeros -> fp64 [N,5,h,w]: the planes of the normal equations, border factors applied."""
    N, two, five, h, w = _tof_f64(R, 5, "tof_matrices: R")
    if (two, five) != (2, 5) or min(h, w) < 2:
        raise ValueError(f"tof_matrices: R [N,2,5,h,w] of at least 2 x 2 expected, got {tuple(R.shape)}")
    if flow is not None and (_tof_f64(flow, 4, "tof_matrices: flow") != (N, h, w, 2) or flow.device != R.device):
        raise ValueError(f"tof_matrices: flow [{N},{h},{w},2] on R's device expected, got {tuple(flow.shape)}")
    out = _f64_out(out, (N, 5, h, w), R, "tof_matrices")
    with on_device(R):
        check(_lib.lib().cdfo_tof_matrices(_vp(R), _vp(flow), N, h, w, _vp(out), _stream()), "cdfo_tof_matrices")
    return out


def tof_blur_solve(M: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """M: dense fp64 [N,5,h,w] -> the flow fp64 [N,h,w,2]: the 15 x 15 box mean of each plane (direct sums in a fixed order, the edge
    sample repeated), then the 2 x 2 solve."""
    N, five, h, w = _tof_f64(M, 4, "tof_blur_solve: M")
    if five != 5:
        raise ValueError(f"tof_blur_solve: M [N,5,h,w] expected, got {tuple(M.shape)}")
    out = _f64_out(out, (N, h, w, 2), M, "tof_blur_solve")
    with on_device(M):
        check(_lib.lib().cdfo_tof_blur_solve(_vp(M), N, h, w, _vp(out), _stream()), "cdfo_tof_blur_solve")
    return out


def tof_flow_up(flow: torch.Tensor, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """flow: dense fp64 [N,hp,wp,2] -> fp64 [N,h,w,2]: the flow on the next stage's grid (bilinear, both taps clamped), times 2."""
    N, hp, wp, two = _tof_f64(flow, 4, "tof_flow_up: flow")
    h, w = int(h), int(w)
    if two != 2 or h <= 0 or w <= 0:
        raise ValueError(f"tof_flow_up: flow [N,hp,wp,2] and a size expected, got {tuple(flow.shape)} -> {h} x {w}")
    out = _f64_out(out, (N, h, w, 2), flow, "tof_flow_up")
    with on_device(flow):
        check(_lib.lib().cdfo_tof_flow_up(_vp(flow), N, hp, wp, h, w, _vp(out), _stream()), "cdfo_tof_flow_up")
    return out


def tof_epe(a: torch.Tensor, b: torch.Tensor, partials: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a, b: dense fp64 flows [K,h,w,2] -> fp64 [K]: the mean endpoint distance per frame.  Strips of 16 rows are summed by one
    workgroup each, then added in index order by one workgroup per frame: the order depends on the shape alone."""
    K_, h, w, two = _tof_f64(a, 4, "tof_epe: a")
    if two != 2 or _tof_f64(b, 4, "tof_epe: b") != (K_, h, w, 2) or b.device != a.device:
        raise ValueError(f"tof_epe: two flows [K,h,w,2] on one device expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    partials = _f64_out(partials, (K_, (h + TOF_STRIP - 1) // TOF_STRIP), a, "tof_epe: partials")
    out = _f64_out(out, (K_,), a, "tof_epe")
    with on_device(a):
        check(_lib.lib().cdfo_tof_epe(_vp(a), _vp(b), K_, h, w, _vp(partials), _vp(out), _stream()), "cdfo_tof_epe")
    return out


# ---- LPIPS' own kernels (csrc/lpips.hip); cdfo_amd/metrics.py packs the model and puts the trunk and the distances together ----
LPIPS_MIN, LPIPS_STRIP, LPIPS_STEM_MAXC, LPIPS_MAX_LAYERS = 16, 2, 256, 8       # CDFO_LPIPS_* of include/cdfo_hip.h


def _lpips_act(t: torch.Tensor, name: str) -> tuple:
    """The shape of a dense device NHWC fp32 stack [N,h,w,C] with no empty dimension and C a multiple of 4."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() \
            or 0 in t.shape or t.shape[3] % 4:
        raise ValueError(f"{name}: a dense device fp32 tensor [N,h,w,C] with C a multiple of 4 expected, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return tuple(int(v) for v in t.shape)


def _lpips_out(out: Optional[torch.Tensor], shape: tuple, like: torch.Tensor, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != like.device:
        raise ValueError(f"{name}: out must be a dense fp32 {list(shape)} tensor on the source's device, got {out.dtype} "
                         f"{tuple(out.shape)} strides {out.stride()} on {out.device}")
    return out


def lpips_stem(frames: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, normalize: bool = True,
               out: Optional[torch.Tensor] = None, peak: Optional[int] = None, _f32: bool = False) -> torch.Tensor:
    """frames: uint8 [N,h,w] (or [h,w]) on the device with contiguous rows, read in place (a view of larger frames is a region);
    weight fp32 [C0,3,3,3] and bias fp32 [C0] on the same device, C0 a multiple of 16, at most 256 -> fp32 [N,h,w,C0]: ReLU of the
    trunk's first convolution on the three scaled channels of the luma (``normalize``: samples to -1 .. 1 first), zeros round the
    SCALED tensor.  ``peak``: the frames are uint16 samples of that peak, v / peak where the 8-bit form has v / 255
    (cdfo_lpips_stem_u16).  ``_f32``: fp32 samples used as they are (`lpips_stem_f32`)."""
    if peak is not None:
        peak = _metric_peak("lpips_stem", peak)
    f, N, h, w, fp, fs = _sample_frames(frames, "lpips_stem: frames", torch.float32 if _f32 else torch.uint8 if peak is None else torch.uint16)
    if N <= 0 or h <= 0 or w <= 0:
        raise ValueError(f"lpips_stem: no samples in {N} frames of {h} x {w}")
    for name, t in (("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != f.device:
            raise ValueError(f"lpips_stem: {name} must be a dense fp32 tensor on the frames' device")
    C0 = int(weight.shape[0]) if weight.dim() else 0
    if tuple(weight.shape) != (C0, 3, 3, 3) or tuple(bias.shape) != (C0,) or C0 == 0 or C0 % 16 or C0 > LPIPS_STEM_MAXC:
        raise ValueError(f"lpips_stem: weight [C0,3,3,3] and bias [C0] with C0 a multiple of 16 up to {LPIPS_STEM_MAXC} expected, got "
                         f"{tuple(weight.shape)} and {tuple(bias.shape)}")
    out = _lpips_out(out, (N, h, w, C0), f, "lpips_stem")
    entry = "cdfo_lpips_stem_f32" if _f32 else "cdfo_lpips_stem_u8" if peak is None else "cdfo_lpips_stem_u16"
    with on_device(f):
        check(getattr(_lib.lib(), entry)(_vp(f), fp, C.c_longlong(fs), N, h, w, _vp(weight), _vp(bias), C0, int(bool(normalize)),
                                         _vp(out), *(() if peak is None else (peak,)), _stream()), entry)
    return out


def lpips_stem_f32(frames: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, normalize: bool = True,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`lpips_stem` of fp32 frames [N,h,w] (or [h,w]) with contiguous rows whose samples are used as they are, nominally in 0 .. 1:
    no division, no clamp, no quantisation (cdfo_lpips_stem_f32; the training loss).  Samples k / 255 give the bits of the 8-bit
    form on k."""
    return lpips_stem(frames, weight, bias, normalize, out, _f32=True)


def lpips_pool2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: dense fp32 [N,H,W,C] on the device, at least 2 x 2, C a multiple of 4 -> fp32 [N,H//2,W//2,C]: the 2 x 2 / stride 2
    maximum, odd sizes floored; bit-equal to ``torch.max_pool2d``."""
    N, H, W, Cc = _lpips_act(x, "lpips_pool2: x")
    if H < 2 or W < 2:
        raise ValueError(f"lpips_pool2: at least 2 x 2 expected, got {H} x {W}")
    out = _lpips_out(out, (N, H // 2, W // 2, Cc), x, "lpips_pool2")
    with on_device(x):
        check(_lib.lib().cdfo_lpips_pool2(_vp(x), N, H, W, Cc, _vp(out), _stream()), "cdfo_lpips_pool2")
    return out


def lpips_dist(fa: torch.Tensor, fb: torch.Tensor, lin: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fa, fb: dense fp32 [N,h,w,C] on one device; lin: dense fp64 [C] there -> fp64 [N,G], G = ceil(h / 2): per strip of two rows
    the sum over its pixels of sum_c lin[c] (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2, in fp64 and in a fixed order."""
    N, h, w, Cc = _lpips_act(fa, "lpips_dist: fa")
    if _lpips_act(fb, "lpips_dist: fb") != (N, h, w, Cc) or fb.device != fa.device:
        raise ValueError(f"lpips_dist: two stacks of one shape on one device expected, got {tuple(fa.shape)} and {tuple(fb.shape)}")
    if not isinstance(lin, torch.Tensor) or lin.dtype != torch.float64 or tuple(lin.shape) != (Cc,) or not lin.is_contiguous() \
            or lin.device != fa.device:
        raise ValueError(f"lpips_dist: lin must be a dense fp64 [{Cc}] tensor on the stacks' device")
    out = _f64_out(out, (N, (h + LPIPS_STRIP - 1) // LPIPS_STRIP), fa, "lpips_dist")
    with on_device(fa):
        check(_lib.lib().cdfo_lpips_dist(_vp(fa), _vp(fb), _vp(lin), N, h, w, Cc, _vp(out), _stream()), "cdfo_lpips_dist")
    return out


def lpips_dist_bwd(fa: torch.Tensor, fb: torch.Tensor, lin: torch.Tensor, gscale: torch.Tensor, gin: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fa, fb: dense fp32 [N,h,w,C] on one device, C a multiple of 16; lin: dense fp64 [C]; gscale: dense fp32 [N], the upstream
    gradient of each frame's layer distance; gin: dense fp32 [N,h,w,C] or None, the gradient that arrives at this tap from the deeper
    stage -> fp32 [N,h,w,C]: the gradient at the pre-activation of ``fa``, ``fa_c > 0 ? d(gscale_n d_n)/d fa_c + gin_c : +0``, the
    derivative in fp64 and rounded once (csrc/lpips.hip has the closed form).  The select drops what arrives where ``fa`` is not
    positive, a NaN included."""
    N, h, w, Cc = _lpips_act(fa, "lpips_dist_bwd: fa")
    if _lpips_act(fb, "lpips_dist_bwd: fb") != (N, h, w, Cc) or fb.device != fa.device:
        raise ValueError(f"lpips_dist_bwd: two stacks of one shape on one device expected, got {tuple(fa.shape)} and {tuple(fb.shape)}")
    if Cc % 16:
        raise ValueError(f"lpips_dist_bwd: C must be a multiple of 16, got {Cc}")
    if not isinstance(lin, torch.Tensor) or lin.dtype != torch.float64 or tuple(lin.shape) != (Cc,) or not lin.is_contiguous() \
            or lin.device != fa.device:
        raise ValueError(f"lpips_dist_bwd: lin must be a dense fp64 [{Cc}] tensor on the stacks' device")
    if not isinstance(gscale, torch.Tensor) or gscale.dtype != torch.float32 or tuple(gscale.shape) != (N,) or not gscale.is_contiguous() \
            or gscale.device != fa.device:
        raise ValueError(f"lpips_dist_bwd: gscale must be a dense fp32 [{N}] tensor on the stacks' device")
    if gin is not None and (_lpips_act(gin, "lpips_dist_bwd: gin") != (N, h, w, Cc) or gin.device != fa.device):
        raise ValueError(f"lpips_dist_bwd: gin must have the stacks' shape and device, got {tuple(gin.shape)}")
    out = _lpips_out(out, (N, h, w, Cc), fa, "lpips_dist_bwd")
    with on_device(fa):
        check(_lib.lib().cdfo_lpips_dist_bwd(_vp(fa), _vp(fb), _vp(lin), _vp(gscale), _vp(gin), N, h, w, Cc, _vp(out), _stream()),
              "cdfo_lpips_dist_bwd")
    return out


def lpips_pool2_bwd(x: torch.Tensor, g: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: dense fp32 [N,H,W,C], the pool's input; g: dense fp32 [N,H//2,W//2,C], the gradient at its output -> fp32 [N,H,W,C]: g at
    the element `lpips_pool2` took, +0 elsewhere and in the floored row and column; bit-equal to the CPU backward of
    ``torch.max_pool2d``."""
    N, H, W, Cc = _lpips_act(x, "lpips_pool2_bwd: x")
    if H < 2 or W < 2:
        raise ValueError(f"lpips_pool2_bwd: at least 2 x 2 expected, got {H} x {W}")
    if _lpips_act(g, "lpips_pool2_bwd: g") != (N, H // 2, W // 2, Cc) or g.device != x.device:
        raise ValueError(f"lpips_pool2_bwd: g [{N},{H // 2},{W // 2},{Cc}] on x's device expected, got {tuple(g.shape)}")
    out = _lpips_out(out, (N, H, W, Cc), x, "lpips_pool2_bwd")
    with on_device(x):
        check(_lib.lib().cdfo_lpips_pool2_bwd(_vp(x), _vp(g), N, H, W, Cc, _vp(out), _stream()), "cdfo_lpips_pool2_bwd")
    return out


def lpips_stem_bwd(g: torch.Tensor, wf: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g: dense fp32 [N,h,w,C0], the gradient at the stem's output already masked by it; wf: dense fp32 [C0,3,3] on the same device,
    the stem's weights folded over the three scaled channels (`cdfo_amd.metrics`: ``k sum_c w[o][c] / scale_c``) -> fp32 [N,h,w]:
    the gradient at the samples, the adjoint of the scaling and conv1_1 as one 3 x 3 C0 -> 1 convolution with flipped taps."""
    N, h, w, C0 = _lpips_act(g, "lpips_stem_bwd: g")
    if C0 % 16 or C0 > LPIPS_STEM_MAXC:
        raise ValueError(f"lpips_stem_bwd: C0 must be a multiple of 16 up to {LPIPS_STEM_MAXC}, got {C0}")
    if not isinstance(wf, torch.Tensor) or wf.dtype != torch.float32 or tuple(wf.shape) != (C0, 3, 3) or not wf.is_contiguous() \
            or wf.device != g.device:
        raise ValueError(f"lpips_stem_bwd: wf must be a dense fp32 [{C0},3,3] tensor on g's device")
    out = _lpips_out(out, (N, h, w), g, "lpips_stem_bwd")
    with on_device(g):
        check(_lib.lib().cdfo_lpips_stem_bwd(_vp(g), _vp(wf), N, h, w, C0, _vp(out), _stream()), "cdfo_lpips_stem_bwd")
    return out


def lpips_fold(partials: torch.Tensor, N: int, strips, counts, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """partials: dense fp64 [N * sum(strips)] on the device, layer k's [N,strips[k]] block behind layer k - 1's -> fp64 [N,layers]:
    the strips of each (frame, layer) added in index order and divided by counts[k] (the layer's pixels); one launch."""
    N = int(N)
    strips, counts = [int(v) for v in strips], [int(v) for v in counts]
    if N <= 0 or not 0 < len(strips) <= LPIPS_MAX_LAYERS or len(counts) != len(strips) or min(strips) <= 0 or min(counts) <= 0:
        raise ValueError(f"lpips_fold: frames and 1 .. {LPIPS_MAX_LAYERS} positive strip and pixel counts expected, got {N}, {strips}, "
                         f"{counts}")
    if not isinstance(partials, torch.Tensor) or not partials.is_cuda or partials.dtype != torch.float64 or partials.dim() != 1 \
            or not partials.is_contiguous() or partials.numel() != N * sum(strips):
        raise ValueError(f"lpips_fold: a dense device fp64 tensor of {N * sum(strips)} partial sums expected, got "
                         f"{getattr(partials, 'dtype', type(partials))} {tuple(getattr(partials, 'shape', ()))}")
    out = _f64_out(out, (N, len(strips)), partials, "lpips_fold")
    g, n = (C.c_int * len(strips))(*strips), (C.c_longlong * len(counts))(*counts)
    with on_device(partials):
        check(_lib.lib().cdfo_lpips_fold(_vp(partials), N, len(strips), g, n, _vp(out), _stream()), "cdfo_lpips_fold")
    return out


def stem_conv(img: torch.Tensor, img_bstride: int, B: int, H: int, W: int, w: torch.Tensor, bias: torch.Tensor,
              act: int = ACT_NONE, add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              out2: Optional[torch.Tensor] = None, write_out: bool = True):
    """img: any fp32 device tensor whose element [b][y][x] sits at data_ptr + (b*img_bstride + y*W + x)*4.
    out / out2: optional dense [B,H,W,64] destinations (slices of a larger batch).  write_out=False (with add): only
    out2 = conv + add is written and returned."""
    if not write_out:
        if add is None or out is not None:
            raise ValueError("stem_conv: write_out=False needs add and no out")
    elif out is None:
        out = empty_act(B, H, W, 64, img.device)
    elif tuple(out.shape) != (B, H, W, 64) or not out.is_contiguous():
        raise ValueError("stem_conv: out must be a dense [B,H,W,64] tensor")
    lda = ldo2 = 0
    if add is not None:
        _, _, _, _, lda = _chk_act(add, "add")
        if out2 is None:
            out2 = empty_act(B, H, W, 64, img.device)
        elif tuple(out2.shape) != (B, H, W, 64) or not out2.is_contiguous():
            raise ValueError("stem_conv: out2 must be a dense [B,H,W,64] tensor")
        ldo2 = 64
    else:
        out2 = None
    check(_lib.lib().cdfo_stem_conv(_vp(img), C.c_longlong(img_bstride), _vp(w), _vp(bias), B, H, W, act, _vp(out), 64,
                                    _vp(add), lda, _vp(out2), ldo2, _stream()), "cdfo_stem_conv")
    if not write_out:
        return out2
    return (out, out2) if add is not None else out


def stem_conv2(img: torch.Tensor, img_bstride: int, B: int, H: int, W: int, wA: torch.Tensor, bA: torch.Tensor,
               add: torch.Tensor, outA: torch.Tensor, wB: torch.Tensor, bB: torch.Tensor, actB: int, outB: torch.Tensor,
               s2dB: bool = False):
    """outA = conv3x3(img; wA, bA) + add, outB = actB(conv3x3(img; wB, bB)); img as in stem_conv, outA dense [B,H,W,64]; outB
    dense [B,H,W,64], or with s2dB a dense [B,H/2+1,W/2+1,256] space-to-depth tensor whose last row / column the caller zeroes."""
    _, _, _, _, lda = _chk_act(add, "add")
    shapeB = (B, H // 2 + 1, W // 2 + 1, 256) if s2dB else (B, H, W, 64)
    if tuple(outA.shape) != (B, H, W, 64) or not outA.is_contiguous() or tuple(outB.shape) != shapeB or not outB.is_contiguous():
        raise ValueError("stem_conv2: outputs must be dense tensors of the documented shapes")
    check(_lib.lib().cdfo_stem_conv2(_vp(img), C.c_longlong(img_bstride), _vp(wA), _vp(bA), _vp(add), lda, _vp(outA), 64,
                                     _vp(wB), _vp(bB), actB, _vp(outB), shapeB[3], int(s2dB), B, H, W, _stream()),
          "cdfo_stem_conv2")


def compose_stem_1x1(w_stem: torch.Tensor, b_stem: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor):
    """A 1x1 convolution (w1 [Co,64,1,1], b1) applied to a one-channel 3x3 stem (w_stem [64,1,3,3], b_stem) with nothing in between
    = one 1 -> Co stencil for the stem kernels (composed in float64): returns (weight [Co,1,3,3], bias [Co]).  Used for
    conv_du_re.0 o conv_expand_rms (arch.py:2200 / 2832, 4446-4449), so that `rms_prior` is never read back."""
    m = w1.detach().double()[:, :, 0, 0]
    return (torch.einsum("oc,ckyx->okyx", m, w_stem.detach().double()).float().contiguous(),
            (m @ b_stem.detach().double() + b1.detach().double()).float().contiguous())


def pack_conv_s2p2_s2d(w2: torch.Tensor, b2: torch.Tensor) -> PackedConv:
    """A 3x3 / stride 2 / pad 2 convolution (64 -> 64) over the space-to-depth form of its input [H/2+1, W/2+1, 4*64] (one zero row /
    column at the end): output (i, j) reads input rows 2i-2+dy = s2d row i-1 phase dy (dy = 0, 1) or s2d row i phase 0 (dy = 2) -- a
    stride-1 pad-1 convolution with weights on the taps (-1, 0) x (-1, 0) only, which the 16-bit MFMA kernel runs with a per-chunk
    tap mask (the exact-fp32 strided kernel it replaces: 0.91 ms per launch at 24 frames)."""
    w2 = w2.detach()
    ws2d = w2.new_zeros(64, 4, 64, 3, 3)
    masks = []
    for a_ in range(2):
        for b_ in range(2):
            m = 0
            for ty in range(2):
                for tx in range(2):
                    dy, dx = 2 * ty + a_, 2 * tx + b_
                    if dy <= 2 and dx <= 2:
                        ws2d[:, a_ * 2 + b_, :, ty, tx] = w2[:, :, dy, dx]
                        m |= 1 << (ty * 3 + tx)
            masks += [m] * 4
    pc2 = pack_conv(ws2d.view(64, 256, 3, 3).contiguous(), b2)
    pc2.tap_mask = torch.tensor(masks, dtype=torch.int32, device=w2.device)
    return pc2


def pack_udsa_head(w0: torch.Tensor, b0: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """Composition of conv_second (1 -> 64, 3x3, w2 / b2) and the prior U-net's body.0 (64 -> 16, 3x3, w0 / b0) for
    cdfo_udsa_head: (wc [9,9,16], bt [9,16], b0 [16]), summed over the 64 channels in float64."""
    W0 = w0.detach().double().reshape(16, 64, 9)
    W2 = w2.detach().double().reshape(64, 9)
    wc = torch.einsum("oct,cu->tuo", W0, W2).float().contiguous()
    bt = torch.einsum("oct,c->to", W0, b2.detach().double()).float().contiguous()
    return wc, bt, b0.detach().float().contiguous()


def udsa_head(img: torch.Tensor, img_bstride: int, B: int, H: int, W: int, packed) -> torch.Tensor:
    """lrelu(body.0(conv_second(img))) -> [B,H,W,16]; img as in stem_conv."""
    out = empty_act(B, H, W, 16, img.device)
    check(_lib.lib().cdfo_udsa_head(_vp(img), C.c_longlong(img_bstride), _vp(packed[0]), _vp(packed[1]), _vp(packed[2]), B, H, W,
                                    _vp(out), 16, _stream()), "cdfo_udsa_head")
    return out


def layernorm64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 64
    out = empty_act(B, H, W, 64, x.device)
    check(_lib.lib().cdfo_layernorm64(_vp(x), ld, _vp(gamma), _vp(beta), C.c_longlong(B * H * W), _vp(out), 64,
                                      _stream()), "cdfo_layernorm64")
    return out


def pack_block_prologue(w_up: torch.Tensor, b_up: torch.Tensor, w_dn: torch.Tensor, b_dn: torch.Tensor):
    """Split-bf16 packing [hi|lo][4][2][128][8] of Block_'s two 1x1 convs (rows 0-63 up.0, 64-127 down.0) + bias[128]."""
    w = torch.cat([w_up.detach().float().reshape(64, 64), w_dn.detach().float().reshape(64, 64)], 0)
    hi = w.bfloat16()
    lo = (w - hi.float()).bfloat16()
    pack = lambda t: t.view(128, 4, 2, 8).permute(1, 2, 0, 3).contiguous().view(-1)
    return torch.cat([pack(hi), pack(lo)]).contiguous(), torch.cat([b_up.detach().float(), b_dn.detach().float()]).contiguous()


def block_prologue(x: torch.Tensor, packed, want_x16: bool = False, lowres_up: bool = False):
    """(u16, d16): fp16 chunk-planar bilinear_x2(up.0(x)) [B,4,2H,2W,16] and down.0(mean2x2(x)) [B,4,H/2,W/2,16];
    want_x16: also (third) the fp16 chunk-planar copy [B,4,H,W,16] of x itself, from the same read of x.
    lowres_up: the first result is up.0(x) at the block's OWN resolution [B,4,H,W,16] (not resampled): the source of
    conv3x3_wino(..., up2=True), which interpolates it on the fly."""
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 64 and H % 2 == 0 and W % 2 == 0
    u16 = torch.empty((B, 4, H, W, 16) if lowres_up else (B, 4, 2 * H, 2 * W, 16), dtype=torch.float16, device=x.device)
    d16 = torch.empty((B, 4, H // 2, W // 2, 16), dtype=torch.float16, device=x.device)
    x16 = torch.empty((B, 4, H, W, 16), dtype=torch.float16, device=x.device) if want_x16 else None
    check(_lib.lib().cdfo_block_prologue2(_vp(x), ld, B, H, W, _vp(packed[0]), _vp(packed[1]), _vp(None if lowres_up else u16),
                                          _vp(u16 if lowres_up else None), _vp(d16), _vp(x16), _stream()), "cdfo_block_prologue2")
    return (u16, d16, x16) if want_x16 else (u16, d16)


def pack_qkv_dw(w_qkv: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """LayerNorm's affine folded into the 1x1 qkv weights: (split-bf16 packing [hi|lo][4][2][192][8], bias W @ beta)."""
    w = w_qkv.detach().float().reshape(192, 64)
    wg = w * gamma.detach().float()[None, :]
    hi = wg.bfloat16()
    lo = (wg - hi.float()).bfloat16()
    pack = lambda t: t.view(192, 4, 2, 8).permute(1, 2, 0, 3).contiguous().view(-1)
    return torch.cat([pack(hi), pack(lo)]).contiguous(), (w @ beta.detach().float()).contiguous()


def qkv_dw(x: torch.Tensor, packed, dw_w: torch.Tensor, eps: float = 1e-5, gram: bool = False):
    """depthwise3x3(conv1x1_64->192(LayerNorm64(x))) in one kernel; packed = pack_qkv_dw(...).
    gram=True: the attention's Gram pass is fused -- returns (v [B,H,W,64], partial [B,n,640], n) for mdta_fold(partial, n, ..)
    and q / k never reach HBM."""
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 64
    if gram:
        out = empty_act(B, H, W, 64, x.device)
        n = int(_lib.lib().cdfo_qkv_dw_gram_slots(B, H, W))
        if n < 1:
            raise CdfoError("cdfo_qkv_dw_gram_slots failed")
        part = torch.zeros((B, n, 640), dtype=torch.float32, device=x.device)
        check(_lib.lib().cdfo_qkv_dw(_vp(x), ld, B, H, W, _vp(packed[0]), _vp(packed[1]), _vp(dw_w), C.c_float(eps), _vp(out),
                                     64, _vp(part), n, _stream()), "cdfo_qkv_dw")
        return out, part, n
    out = empty_act(B, H, W, 192, x.device)
    check(_lib.lib().cdfo_qkv_dw(_vp(x), ld, B, H, W, _vp(packed[0]), _vp(packed[1]), _vp(dw_w), C.c_float(eps), _vp(out),
                                 192, None, 0, _stream()), "cdfo_qkv_dw")
    return out


def layernorm64_hl(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """LayerNorm64 written as fp16 hi | lo chunk-planar planes [B, 8, H, W, 16] (planes 0-3 hi, 4-7 lo)."""
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 64
    out = torch.empty((B, 8, H, W, 16), dtype=torch.float16, device=x.device)
    check(_lib.lib().cdfo_layernorm64_cp16hl(_vp(x), ld, _vp(gamma), _vp(beta), B, C.c_longlong(H * W), _vp(out), _stream()),
          "cdfo_layernorm64_cp16hl")
    return out


def pack_conv_hilo(weight: torch.Tensor, bias: Optional[torch.Tensor], weight_lo: bool = True) -> PackedConv:
    """3x3 weight for the split-fp16 product on the ring kernel: K-expanded (w_hi | w_hi | w_lo) along the input channels,
    to be used with a source of hi | lo planes and plane_wrap = 2 * Cin / 16: a_hi*w_hi + a_lo*w_hi + a_hi*w_lo.
    weight_lo=False drops the third term (weights rounded once to fp16, activations still hi + lo: the "fp16x2" arithmetic
    of the tiled kernel): (w_hi | w_hi), a third fewer K chunks."""
    w = weight.detach().float()
    wh = w.half().float()
    return pack_conv(torch.cat([wh, wh, w - wh] if weight_lo else [wh, wh], 1).contiguous(), bias)


def dwconv3x3(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(x)
    out = empty_act(B, H, W, Cc, x.device)
    check(_lib.lib().cdfo_dwconv3x3(_vp(x), ld, _vp(w), B, H, W, Cc, _vp(out), Cc, _stream()), "cdfo_dwconv3x3")
    return out


def flow_warp(x: torch.Tensor, mv: torch.Tensor, mv_bstride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(x)
    if out is None:
        out = empty_act(B, H, W, Cc, x.device)
    elif tuple(out.shape) != (B, H, W, Cc) or not out.is_contiguous():
        raise ValueError("flow_warp: out must be a dense tensor of the input's shape")
    check(_lib.lib().cdfo_flow_warp(_vp(x), ld, _vp(mv), C.c_longlong(mv_bstride), B, H, W, Cc, _vp(out), Cc,
                                    _stream()), "cdfo_flow_warp")
    return out


def flow_warp_frames(bank: torch.Tensor, idx: torch.Tensor, mv: torch.Tensor, mv_kstride: int, slot0: int, G: int, K: int,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """flow_warp with an indexed source: out[g*K + k] = flow_warp(bank[idx[g*K + k]], mv + k*mv_kstride + (slot0 + g)*2*H*W) for
    g < G, k < K.  bank [n,H,W,C] is read in place; idx: int32 [G*K] on the device, an index outside the bank gives zeros."""
    n_bank, H, W, Cc, ld = _chk_act(bank, "bank")
    if idx.dtype != torch.int32 or idx.device != bank.device or idx.dim() != 1 or not idx.is_contiguous() or idx.numel() != G * K:
        raise ValueError("flow_warp_frames: idx must be a dense int32 vector of G*K entries on the bank's device")
    if mv.dtype != torch.float32 or mv.device != bank.device:
        raise ValueError("flow_warp_frames: mv must be an fp32 tensor on the bank's device")
    if out is None:
        out = empty_act(G * K, H, W, Cc, bank.device)
    _, _, _, _, ldo = _chk_act(out, "out")
    if tuple(out.shape) != (G * K, H, W, Cc):
        raise ValueError("flow_warp_frames: out must hold G*K frames of the bank's shape")
    check(_lib.lib().cdfo_flow_warp_frames(_vp(bank), ld, n_bank, _vp(idx), _vp(mv), C.c_longlong(mv_kstride), slot0, G, K, H, W, Cc,
                                           _vp(out), ldo, _stream()), "cdfo_flow_warp_frames")
    return out


def resample2(x: torch.Tensor, up: bool, out: Optional[torch.Tensor] = None, accumulate: bool = False,
              out_f16: bool = False, cp16: bool = False) -> torch.Tensor:
    """cp16 (up only): the result is the fp16 chunk-planar tensor [B, C/16, 2H, 2W, 16] that conv3x3_ws reads."""
    B, H, W, Cc, ld = _chk_act(x)
    Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
    if cp16:
        assert up and out is None and not accumulate
        out = torch.empty((B, Cc // 16, Ho, Wo, 16), dtype=torch.float16, device=x.device)
        check(_lib.lib().cdfo_resample2(_vp(x), ld, B, H, W, Cc, _vp(out), 16, 1, 0, 2, _stream()), "cdfo_resample2")
        return out
    odt = torch.float16 if out_f16 else torch.float32
    if out is None:
        assert not accumulate
        out = torch.empty((B, Ho, Wo, Cc), dtype=odt, device=x.device)
    ob, oh, ow, oc, ldo = _chk_act(out, "out", odt)
    assert (ob, oh, ow, oc) == (B, Ho, Wo, Cc)
    check(_lib.lib().cdfo_resample2(_vp(x), ld, B, H, W, Cc, _vp(out), ldo, int(up), int(accumulate), int(out_f16),
                                    _stream()), "cdfo_resample2")
    return out


def scale_channels(x: torch.Tensor, gate: torch.Tensor, want_cp16: bool = False):
    """x * gate[b][c]; want_cp16: also the fp16 chunk-planar copy [B,C/16,H,W,16] of the result (returns a pair)."""
    B, H, W, Cc, ld = _chk_act(x)
    out = empty_act(B, H, W, Cc, x.device)
    o16 = torch.empty((B, Cc // 16, H, W, 16), dtype=torch.float16, device=x.device) if want_cp16 else None
    check(_lib.lib().cdfo_scale_channels(_vp(x), ld, _vp(gate), B, C.c_longlong(H * W), Cc, _vp(out), Cc, _vp(o16),
                                         _stream()), "cdfo_scale_channels")
    return (out, o16) if want_cp16 else out


def upconv_last(x: torch.Tensor, pc: PackedConv, w_last: torch.Tensor, b_last: torch.Tensor, xc: torch.Tensor,
                xc_bstride: int) -> torch.Tensor:
    """Upsampler tail (arch.py:4474-4480) without the HR feature map: lrelu(pixel_shuffle(upconv2(x))) -> conv_last ->
    + bilinear_x4(x_center).  x: [B,2H,2W,64]; pc: upconv2 packed with shuffle2=True; returns [B,1,4H,4W]."""
    if not pc.shuffle2 or pc.Cout != 256 or pc.ks != 1:
        raise ValueError("upconv_last: needs the pixel-shuffle packing of a 1x1 conv with 256 outputs")
    a, taps = _conv_args([x], pc, act=ACT_LRELU, store_mode=3)       # CDFO_STORE_TAPS9: taps [B,4H,4W,12]
    B, H2, W2 = a.B, a.H, a.W
    a.res2 = w_last.detach().contiguous().float().data_ptr()
    check(_lib.lib().cdfo_conv1x1_bf16x3(C.byref(a), _stream()), "cdfo_conv1x1_bf16x3 (tap sums)")
    out = torch.empty((B, 1, 2 * H2, 2 * W2), dtype=torch.float32, device=x.device)
    check(_lib.lib().cdfo_conv_last_taps(_vp(taps), 12, _vp(b_last), _vp(xc), C.c_longlong(xc_bstride), B, 2 * H2, 2 * W2,
                                         _vp(out), _stream()), "cdfo_conv_last_taps")
    return out


def conv_last(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, xc: torch.Tensor, xc_bstride: int) -> torch.Tensor:
    B, Hh, Wh, Cc, ld = _chk_act(x)
    assert Cc == 64
    out = torch.empty((B, 1, Hh, Wh), dtype=torch.float32, device=x.device)
    check(_lib.lib().cdfo_conv_last(_vp(x), ld, _vp(w), _vp(bias), _vp(xc), C.c_longlong(xc_bstride), B, Hh, Wh,
                                    _vp(out), _stream()), "cdfo_conv_last")
    return out


def small_conv16(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stride: int, pad: int, out_pad: int = 0,
                 transposed: bool = False, act: int = ACT_NONE, out_hl: bool = False) -> torch.Tensor:
    """out_hl: return the result as fp16 hi | lo chunk-planar planes [B, 2, Ho, Wo, 16] (source of conv_ring with plane_wrap=2)."""
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 16
    if transposed:
        Ho, Wo = (H - 1) * stride - 2 * pad + 3 + out_pad, (W - 1) * stride - 2 * pad + 3 + out_pad
    else:
        Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    if out_hl:
        hl = torch.empty((B, 2, Ho, Wo, 16), dtype=torch.float16, device=x.device)
        check(_lib.lib().cdfo_small_conv16_hl(_vp(x), ld, _vp(w), _vp(bias), B, H, W, stride, pad, out_pad, int(transposed), act,
                                              _vp(hl), _stream()), "cdfo_small_conv16_hl")
        return hl
    out = empty_act(B, Ho, Wo, 16, x.device)
    check(_lib.lib().cdfo_small_conv16(_vp(x), ld, _vp(w), _vp(bias), B, H, W, stride, pad, out_pad, int(transposed),
                                       act, _vp(out), 16, _stream()), "cdfo_small_conv16")
    return out


def spatial_gate16(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 16
    out = empty_act(B, H, W, 16, x.device)
    check(_lib.lib().cdfo_spatial_gate16(_vp(x), ld, _vp(w), _vp(bias), B, H, W, _vp(out), 16, _stream()),
          "cdfo_spatial_gate16")
    return out


# ----------------------------------------------------------------------------------------------- CVSR_V7 operators
def chan_pool(x: torch.Tensor) -> torch.Tensor:
    """[B,H,W,64] -> [B,H,W,2] = (max over channels, mean over channels)."""
    B, H, W, Cc, ld = _chk_act(x)
    out = torch.empty((B, H, W, 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().cdfo_chan_pool(_vp(x), ld, C.c_longlong(B * H * W), Cc, _vp(out), _stream()), "cdfo_chan_pool")
    return out


def gate_map_cumulative(pooled: torch.Tensor, cum: Optional[torch.Tensor], w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """G_k = G_{k-1} * sigmoid(conv(G_{k-1} * pooled_0) + bias): the running per-pixel product of a SpatialAttention applied repeatedly
    to the same tensor (x_k = x_0 * G_k); pooled = chan_pool(x_0) [B,H,W,2], cum = G_{k-1} [B,H,W] or None."""
    B, H, W, two = pooled.shape
    if two != 2 or not pooled.is_contiguous() or (cum is not None and (tuple(cum.shape) != (B, H, W) or not cum.is_contiguous())):
        raise ValueError("gate_map_cumulative: pooled [B,H,W,2] and cum [B,H,W] expected")
    out = torch.empty((B, H, W), dtype=torch.float32, device=pooled.device)
    check(_lib.lib().cdfo_gate_map_cumulative(_vp(pooled), _vp(cum), _vp(w), _vp(bias), B, H, W, int(w.shape[-1]), _vp(out), _stream()),
          "cdfo_gate_map_cumulative")
    return out


def spatial_gate(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """SpatialAttention: x * sigmoid(conv(pool(x))); w: the [1,2,ks,ks] weight."""
    B, H, W, Cc, ld = _chk_act(x)
    out = empty_act(B, H, W, Cc, x.device)
    gate = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    check(_lib.lib().cdfo_spatial_gate(_vp(x), ld, _vp(chan_pool(x)), _vp(w), _vp(bias), B, H, W, Cc, int(w.shape[-1]),
                                       _vp(gate), _vp(out), Cc, _stream()), "cdfo_spatial_gate")
    return out


def rdab_mix(xf: torch.Tensor, xc: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, vmax: torch.Tensor,
             noise: torch.Tensor) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(xf)
    if tuple(noise.shape) != (B, 64, H, W) or not noise.is_contiguous() or noise.dtype != torch.float32:
        raise ValueError(f"rdab_mix: noise must be a contiguous fp32 [B,64,H,W] tensor, got {tuple(noise.shape)}")
    if tuple(vmax.shape) != (B, 64) or tuple(w3.shape) != (1, 2, 3, 3):
        raise ValueError("rdab_mix: vmax must be [B,64] and the spatial weight [1,2,3,3]")
    out = empty_act(B, H, W, 64, xf.device)
    check(_lib.lib().cdfo_rdab_mix(_vp(xf), ld, _vp(chan_pool(xc)), _vp(w3), _vp(b3), _vp(vmax), _vp(noise), B, H, W,
                                   _vp(out), 64, _stream()), "cdfo_rdab_mix")
    return out


def shrink_planes(t: torch.Tensor, level: int) -> torch.Tensor:
    """t: fp32 [B,C,H,W] whose images are dense (any batch stride) -> contiguous [B,C,H>>level,W>>level]."""
    B, Cc, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W:
        t = t.contiguous()
    out = torch.empty((B, Cc, H >> level, W >> level), dtype=torch.float32, device=t.device)
    check(_lib.lib().cdfo_shrink_planes(_vp(t), C.c_longlong(t.stride(0)), Cc, B, H, W, level, _vp(out), _stream()),
          "cdfo_shrink_planes")
    return out


def lincomb(a: torch.Tensor, ca: float, b: Optional[torch.Tensor] = None, cb: float = 0.0,
            c: Optional[torch.Tensor] = None, cc: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    for t in (a, b, c, out):
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32 or t.shape != a.shape):
            raise ValueError("lincomb: contiguous fp32 tensors of one shape expected")
    if out is None:
        out = torch.empty_like(a)
    check(_lib.lib().cdfo_lincomb(_vp(out), _vp(a), float(ca), _vp(b), float(cb), _vp(c), float(cc),
                                  C.c_longlong(a.numel()), _stream()), "cdfo_lincomb")
    return out


# ----------------------------------------------------------------------------------------------- reductions / folds
def nchunks_for(P: int) -> int:
    return max(1, min(128, P // 1024))


def chan_sum_partial(x: torch.Tensor):
    B, H, W, Cc, ld = _chk_act(x)
    assert Cc == 64
    n = nchunks_for(H * W)
    part = torch.empty((B, n, 64), dtype=torch.float32, device=x.device)
    check(_lib.lib().cdfo_chan_sum_partial(_vp(x), ld, B, C.c_longlong(H * W), n, _vp(part), _stream()),
          "cdfo_chan_sum_partial")
    return part, n


def pack_rdab_stats(w2: torch.Tensor) -> torch.Tensor:
    """conv_du_re.2's weight [64,64,3,3] as rdab_stats reads it: bf16 hi | lo = bf16(w - hi), [2][9 taps][4 k-steps][2 k-halves][64 out][8].
    Element j of k-step c, half h is input channel 16 c + 8 (j >> 2) + 4 h + (j & 3): the order in which a lane of the 32x32 MFMA
    holds the accumulators of the product that forms du0, so that they become the next product's operand in place."""
    if tuple(w2.shape) != (64, 64, 3, 3):
        raise ValueError(f"pack_rdab_stats: a [64,64,3,3] weight expected, got {tuple(w2.shape)}")
    w = w2.detach().float().permute(2, 3, 1, 0).reshape(9, 4, 2, 2, 4, 64).permute(0, 1, 3, 5, 2, 4).reshape(9, 4, 2, 64, 8)
    hi = w.to(torch.bfloat16)
    return torch.stack([hi, (w - hi.float()).to(torch.bfloat16)]).contiguous()


def rdab_stats_ok(H: int, W: int) -> bool:
    """Inside the contract of rdab_stats: an even-sized map (conv_du_re.2's stride-2 output grid is then (H/2+1) x (W/2+1), as the
    space-to-depth path has it) whose pixel indices fit 32 bits."""
    return H > 0 and W > 0 and H % 2 == 0 and W % 2 == 0 and H * W < (1 << 30)


def rdab_stats(img: torch.Tensor, Bi: int, s_b: int, s_g: int, B: int, H: int, W: int, w0: torch.Tensor, b0: torch.Tensor,
               w2_packed: torch.Tensor, b2: torch.Tensor, out: Optional[torch.Tensor] = None):
    """LLongRangAttention's mask statistics from the residual maps themselves: returns (part [B,n,64], n, count) with part the
    channel sums, in chan_sum_partial's layout, of relu(conv_du_re.2(du0)) over its count = (H/2+1)(W/2+1) output pixels, du0 =
    relu(stencil(img; w0, b0)) on the H x W grid and zero outside it.  Neither du0 nor the convolution's result is allocated.
    img: an fp32 device tensor; image m's dense H x W plane starts (m % Bi) * s_b + (m // Bi) * s_g elements behind its first
    element (for maps[:, 0, i:i+G] of a [B,1,7,H,W] tensor: Bi = B, s_b = 7 H W, s_g = H W).  w0 / b0: compose_stem_1x1's stencil;
    w2_packed: pack_rdab_stats; out: optional dense [B,n,64] destination (a slice of a larger batch).  Fixed-order sums."""
    if not rdab_stats_ok(H, W):
        raise ValueError(f"rdab_stats: an even-sized map expected, got {H} x {W} (use stem_conv2 + conv + chan_sum_partial)")
    if img.dtype != torch.float32 or not img.is_cuda or B <= 0 or Bi <= 0 or s_b < 0 or s_g < 0:
        raise ValueError("rdab_stats: an fp32 device tensor, B, Bi > 0 and non-negative strides expected")
    last = (min(B, Bi) - 1) * s_b + ((B - 1) // Bi) * s_g + H * W
    if last > img.untyped_storage().nbytes() // 4 - img.storage_offset():
        raise ValueError("rdab_stats: the planes reach beyond the tensor's storage")
    if (w2_packed.dtype != torch.bfloat16 or tuple(w2_packed.shape) != (2, 9, 4, 2, 64, 8) or not w2_packed.is_contiguous()
            or tuple(w0.shape) != (64, 1, 3, 3) or not w0.is_contiguous() or w0.dtype != torch.float32
            or any(t.numel() != 64 or t.dtype != torch.float32 or not t.is_contiguous() for t in (b0, b2))
            or any(t.device != img.device for t in (w0, b0, w2_packed, b2))):
        raise ValueError("rdab_stats: w0 [64,1,3,3], b0 [64], b2 [64] fp32 and pack_rdab_stats' image expected on the maps' device")
    count = (H // 2 + 1) * (W // 2 + 1)
    n = nchunks_for(count)
    if out is None:
        out = torch.empty((B, n, 64), dtype=torch.float32, device=img.device)
    elif tuple(out.shape) != (B, n, 64) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != img.device:
        raise ValueError(f"rdab_stats: out must be a dense fp32 [{B},{n},64] tensor on the maps' device")
    with on_device(img):
        check(_lib.lib().cdfo_rdab_stats(_vp(img), Bi, C.c_longlong(s_b), C.c_longlong(s_g), _vp(w0), _vp(b0), _vp(w2_packed),
                                         _vp(b2), B, H, W, n, _vp(out), _stream()), "cdfo_rdab_stats")
    return out, n, count


def gram_partial(q: torch.Tensor, k: torch.Tensor, ch_per_head: int):
    B, H, W, Cc, ldq = _chk_act(q, "q")
    _, _, _, _, ldk = _chk_act(k, "k")
    n = nchunks_for(H * W)
    part = torch.empty((B, n, 64 * (ch_per_head + 2)), dtype=torch.float32, device=q.device)
    check(_lib.lib().cdfo_gram_partial(_vp(q), ldq, _vp(k), ldk, B, C.c_longlong(H * W), ch_per_head, n, _vp(part),
                                       _stream()), "cdfo_gram_partial")
    return part, n


def align_stats_slots(B: int, P: int) -> int:
    """Partial slots per image of the persistent streaming kernels' statistics outputs (align_stats, conv(chan_sum_out=True)) for the
    calling thread's CU share."""
    n = _lib.lib().cdfo_align_stats_slots(B, C.c_longlong(P))
    if n <= 0:
        raise CdfoError(f"cdfo_align_stats_slots({B}, {P}) failed: {n}")
    return n


def align_stats(x0: torch.Tensor, x1: Optional[torch.Tensor], q: torch.Tensor, pc: PackedConv, act: int, ch_per_head: int, plane=None):
    """The statistics of DualAttAlignment in one pass over x0, x1, q ([B,H,W,64] each, any pixel pitch): with
    kf = act(conv1x1([x0, x1], pc)) (128 -> 64, never written) returns (gram, sum0, sum1, n) = gram_partial(q, kf, ch_per_head)[0],
    chan_sum_partial(x0)[0], chan_sum_partial(x1)[0] with n partial slots each (fixed-order sums: run-to-run identical).
    plane = (view, Bi, s_b, s_g, table, stencil) with x1 = None: x1 is the 3x3 stencil `stencil` (pack_plane_chunk of it) of the
    one-channel planes `view` addresses (see _plane_args) and is never materialised; table: pack_plane_chunk of pc's second half
    composed with the stencil (compose_stem_1x1).  sum1 is then formed from the planes' tap sums.  q may be an ImageMap."""
    if (x1 is None) != (plane is not None):
        raise ValueError("align_stats: either x1 or the plane it is a stencil of")
    B, H, W, c0, ld0 = _chk_act(x0, "x0")
    b1, h1, w1, c1, ld1 = (B, H, W, 64, 0) if x1 is None else _chk_act(x1, "x1")
    bq, hq, wq, cq, ldq = _chk_act(q, "q")
    if (b1, h1, w1) != (B, H, W) or (bq, hq, wq) != (B, H, W) or (c0, c1, cq) != (64, 64, 64):
        raise ValueError("align_stats: three [B,H,W,64] operands expected")
    if pc.ks != 1 or pc.Cin != 128 or pc.Cout != 64 or pc.CoutP != 64 or pc.w_bstride != 0:
        raise ValueError("align_stats: a packed 128 -> 64 1x1 convolution expected")
    n = align_stats_slots(B, H * W)
    gs = 64 * (ch_per_head + 2)
    buf = torch.zeros((B * n * (gs + 128),), dtype=torch.float32, device=q.device)     # one fill for the three outputs
    gram = buf[:B * n * gs].view(B, n, gs)
    s0 = buf[B * n * gs:B * n * (gs + 64)].view(B, n, 64)
    s1 = buf[B * n * (gs + 64):].view(B, n, 64)
    view, Bi, s_b, s_g, table, stencil = None, 0, 0, 0, None, None
    if plane is not None:
        view, Bi, s_b, s_g, table, _ = _plane_args(plane[:5], B, H, W, 64, "align_stats")
        stencil = plane[5]
        if (tuple(stencil.shape) != (64, 16) or stencil.dtype != torch.float32 or not stencil.is_contiguous()
                or stencil.device != table.device or table.dim() != 2):
            raise ValueError("align_stats: the stencil's table and the composed table must be fp32 [64,16] (pack_plane_chunk)")
    if _is_map(q):
        qB, qsb, qsg = q.triple()
        check(_lib.lib().cdfo_align_stats_map(_vp(x0), ld0, _vp(x1), ld1, _vp(q), ldq, qB, C.c_longlong(qsb), C.c_longlong(qsg), _vp(pc.w),
                                              _vp(pc.bias), act, ch_per_head, B, C.c_longlong(H * W), n, _vp(gram), _vp(s0), _vp(s1),
                                              _vp(view), Bi, C.c_longlong(s_b), C.c_longlong(s_g), W, _vp(table), _vp(stencil), _stream()),
              "cdfo_align_stats_map")
        return gram, s0, s1, n
    if plane is not None:
        check(_lib.lib().cdfo_align_stats_plane(_vp(x0), ld0, _vp(q), ldq, _vp(pc.w), _vp(pc.bias), act, ch_per_head, B,
                                                C.c_longlong(H * W), n, _vp(gram), _vp(s0), _vp(s1), _vp(view), Bi, C.c_longlong(s_b),
                                                C.c_longlong(s_g), W, _vp(table), _vp(stencil), _stream()), "cdfo_align_stats_plane")
        return gram, s0, s1, n
    check(_lib.lib().cdfo_align_stats(_vp(x0), ld0, _vp(x1), ld1, _vp(q), ldq, _vp(pc.w), _vp(pc.bias), act, ch_per_head, B,
                                      C.c_longlong(H * W), n, _vp(gram), _vp(s0), _vp(s1), _stream()), "cdfo_align_stats")
    return gram, s0, s1, n


def mdta_fold(part: torch.Tensor, n: int, temperature: torch.Tensor, proj_w: torch.Tensor) -> PackedConv:
    B = part.shape[0]
    wout = torch.empty((B, 4096), dtype=torch.float32, device=part.device)
    check(_lib.lib().cdfo_mdta_fold(_vp(part), n, _vp(temperature), _vp(proj_w), B, _vp(wout), _stream()),
          "cdfo_mdta_fold")
    return PackedConv(wout, None, 64, 64, 1, 64, False, 4096)


_FOLD_CIN = {}


def fold_scale_inputs(fold: PackedConv, gate: torch.Tensor) -> PackedConv:
    """The per-image 64 x 64 matrices of mdta_fold with a per-image input-channel gate folded in: M'[b] = M[b] diag(gate[b]), so that
    conv(x * gate, M) == conv(x, M') and the gated copy of x is never written (parameter-sized torch arithmetic on [B, 4096])."""
    if fold.Cin != 64 or fold.Cout != 64 or fold.ks != 1 or fold.w_bstride != 4096 or tuple(gate.shape) != (fold.w.shape[0], 64):
        raise ValueError("fold_scale_inputs: a mdta_fold result and a [B, 64] gate expected")
    cin = _FOLD_CIN.get(gate.device)
    if cin is None:       # packed layout [Cin/16][4][CoutP = 64][4]: input channel of every element
        i = torch.arange(4096, device=gate.device)
        cin = (i // 1024) * 16 + ((i // 256) % 4) * 4 + i % 4
        # cached only outside stream capture: a table built while capturing lives in the graph's private pool and is merely RECORDED,
        # so a later eager call would read uninitialised indices
        if not (gate.is_cuda and torch.cuda.is_current_stream_capturing()):
            _FOLD_CIN[gate.device] = cin
    return PackedConv(fold.w * gate[:, cin], None, 64, 64, 1, 64, False, 4096)


def align_fold(gpart, ng, sw, sp, ns, P, temperature, du0_w, du0_b, du2_w, du2_b, proj_w, fusion_w) -> PackedConv:
    B = gpart.shape[0]
    wout = torch.empty((B, 192 * 64), dtype=torch.float32, device=gpart.device)
    check(_lib.lib().cdfo_align_fold(_vp(gpart), ng, _vp(sw), _vp(sp), ns, C.c_longlong(P), _vp(temperature),
                                     _vp(du0_w), _vp(du0_b), _vp(du2_w), _vp(du2_b), _vp(proj_w), _vp(fusion_w), B,
                                     _vp(wout), _stream()), "cdfo_align_fold")
    return PackedConv(wout, None, 64, 192, 1, 64, False, 192 * 64)


def align_fold_plane(gpart, ng, sw, sp, ns, P, temperature, du0_w, du0_b, du2_w, du2_b, proj_w, fusion_w, stencil):
    """align_fold where pred stays a one-channel plane (stencil: pack_plane_chunk of its 3x3 stem): returns (PackedConv 128 -> 64 over
    cat[warped, x] = align_fold's columns [M1 | Wb], bit for bit; tables [B,64,16] = M2 . [w_s | b_s], the per-image plane tables of
    conv(..., plane=(..., tables, 64 * 16)))."""
    B = gpart.shape[0]
    if tuple(stencil.shape) != (64, 16) or stencil.dtype != torch.float32 or not stencil.is_contiguous():
        raise ValueError("align_fold_plane: the stencil's table must be fp32 [64,16] (pack_plane_chunk)")
    wout = torch.empty((B, 128 * 64), dtype=torch.float32, device=gpart.device)
    tables = torch.empty((B, 64, 16), dtype=torch.float32, device=gpart.device)
    check(_lib.lib().cdfo_align_fold_plane(_vp(gpart), ng, _vp(sw), _vp(sp), ns, C.c_longlong(P), _vp(temperature),
                                           _vp(du0_w), _vp(du0_b), _vp(du2_w), _vp(du2_b), _vp(proj_w), _vp(fusion_w), _vp(stencil),
                                           B, _vp(wout), _vp(tables), _stream()), "cdfo_align_fold_plane")
    return PackedConv(wout, None, 64, 128, 1, 64, False, 128 * 64), tables


def vec_mlp(part: torch.Tensor, n: int, P: int, w1, b1, c1: int, act1: int, w2=None, b2=None, c2: int = 0,
            act2: int = ACT_NONE) -> torch.Tensor:
    B = part.shape[0]
    out = torch.empty((B, c2 if w2 is not None else c1), dtype=torch.float32, device=part.device)
    check(_lib.lib().cdfo_vec_mlp(_vp(part), n, C.c_longlong(P), _vp(w1), _vp(b1), c1, act1, _vp(w2), _vp(b2), c2, act2,
                                  B, _vp(out), _stream()), "cdfo_vec_mlp")
    return out


# ----------------------------------------------------------------------------------------------- prior-fusion attention
def _prep_outs(outs, B, H, W, device):
    if outs is None:
        return empty_act(B, H, W, 64, device), empty_act(B, H, W, 64, device), empty_act(B, H, W, 64, device)
    for t in outs:
        if tuple(t.shape) != (B, H, W, 64) or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError("rdab_prep: outs must be three dense fp32 [B,H,W,64] tensors")
    return outs


def rdab_prep(xq: torch.Tensor, vmax: torch.Tensor, noise: torch.Tensor, wW: torch.Tensor, bW: torch.Tensor, outs=None):
    B, H, W, Cc, ld = _chk_act(xq)
    assert Cc == 128 and noise.is_contiguous() and tuple(noise.shape) == (B, 64, H, W)
    sq, vrow, qwin = _prep_outs(outs, B, H, W, xq.device)
    check(_lib.lib().cdfo_rdab_prep(_vp(xq), ld, _vp(vmax), _vp(noise), _vp(wW), _vp(bW), B, C.c_longlong(H * W),
                                    _vp(sq), 64, _vp(vrow), 64, _vp(qwin), 64, _stream()), "cdfo_rdab_prep")
    return sq, vrow, qwin


def rdab_prep_rng(xq: torch.Tensor, vmax: torch.Tensor, seed: int, draw: int, wW: torch.Tensor, bW: torch.Tensor,
                  noise_out: Optional[torch.Tensor] = None, outs=None):
    """rdab_prep with the uniform draws of arch.py:2169 generated inside the kernel (Philox4x32-10, key = seed, `draw` =
    index of the call within the forward).  noise_out: optional fp32 [B,64,H,W] tensor that receives the drawn values."""
    B, H, W, Cc, ld = _chk_act(xq)
    assert Cc == 128
    if noise_out is not None and (tuple(noise_out.shape) != (B, 64, H, W) or not noise_out.is_contiguous()
                                  or noise_out.dtype != torch.float32):
        raise ValueError("rdab_prep_rng: noise_out must be a contiguous fp32 [B,64,H,W] tensor")
    sq, vrow, qwin = _prep_outs(outs, B, H, W, xq.device)
    if isinstance(seed, torch.Tensor):      # the key lives in device memory (int64[1]): graph replays re-read it
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != xq.device:
            raise ValueError("rdab_prep_rng: a device-side key must be an int64[1] tensor on the operands' device")
        check(_lib.lib().cdfo_rdab_prep_rng_dev(_vp(xq), ld, _vp(vmax), _vp(seed), draw, _vp(noise_out), _vp(wW), _vp(bW), B,
                                                C.c_longlong(H * W), _vp(sq), 64, _vp(vrow), 64, _vp(qwin), 64, _stream()),
              "cdfo_rdab_prep_rng_dev")
        return sq, vrow, qwin
    check(_lib.lib().cdfo_rdab_prep_rng(_vp(xq), ld, _vp(vmax), C.c_longlong(seed & 0x7FFFFFFFFFFFFFFF), draw, _vp(noise_out),
                                        _vp(wW), _vp(bW), B, C.c_longlong(H * W), _vp(sq), 64, _vp(vrow), 64, _vp(qwin), 64,
                                        _stream()), "cdfo_rdab_prep_rng")
    return sq, vrow, qwin


def rdab_prep_fused_ok(x: torch.Tensor, pc: PackedConv) -> bool:
    """Inside the contract of rdab_prep_fused: a 64 -> 128 1x1 convolution with shared weights over whole 64-pixel blocks."""
    return (x.dim() == 4 and x.shape[3] == 64 and (x.shape[1] * x.shape[2]) % 64 == 0 and pc.ks == 1 and pc.Cin == 64
            and pc.Cout == 128 and pc.CoutP == 128 and pc.w_bstride == 0 and not pc.shuffle2)


def rdab_prep_fused_map_ok(plane: bool) -> bool:
    """rdab_prep_fused takes a mapped x in its plane form only (the form of the default path)."""
    return bool(plane)


def rdab_prep_fused(x: torch.Tensor, pc: PackedConv, vmax: torch.Tensor, noise, wW: torch.Tensor, bW: torch.Tensor,
                    v_f16: bool = False, outs=None, plane=None):
    """plane = (view, Bi, s_b, s_g, table): the convolution runs on x + stencil9(plane) with only x in memory (see conv's `plane`;
    table = pack_plane_chunk(*compose_stem_1x1(stencil, input_conv without its bias)), [128,16]).
    conv(x, pc) (RDAB.input_conv, 64 -> 128 = q | v) followed by rdab_prep / rdab_prep_rng in ONE launch: the 128-channel product
    is never written.  noise: the injected fp32 [B,64,H,W] draws, or ("rng", seed, draw, noise_out) as rdab_prep_rng takes them.
    Returns (sq, vrow, qwin, vwin) -- vwin = the v half of the product, which the two-kernel path reads from xq[..., 64:].
    v_f16 (a bool for both, or a pair (vrow, vwin)): that output as fp16, each value rounded once (what seq_attn's modes 20-22 do
    to an fp32 V while staging).  outs: the four [B,H,W,64] result tensors, dense, of those dtypes.  x may be an ImageMap
    (beside a plane: rdab_prep_fused_map_ok)."""
    B, H, W, Cc, ld = _chk_act(x, "x")
    if not rdab_prep_fused_ok(x, pc):
        raise ValueError("rdab_prep_fused: a 64 -> 128 1x1 convolution over H*W % 64 == 0 pixels expected (use conv + rdab_prep)")
    row16, win16 = (v_f16, v_f16) if isinstance(v_f16, bool) else v_f16
    dts = (torch.float32, torch.float16 if row16 else torch.float32, torch.float32, torch.float16 if win16 else torch.float32)
    if outs is None:
        outs = tuple(torch.empty((B, H, W, 64), dtype=dt, device=x.device) for dt in dts)
    sq, vrow, qwin, vwin = outs
    for t, dt in zip(outs, dts):
        if tuple(t.shape) != (B, H, W, 64) or not t.is_contiguous() or t.dtype != dt:
            raise ValueError("rdab_prep_fused: outs must be dense [B,H,W,64] tensors: sq, qwin fp32; vrow, vwin fp32 or, as v_f16 says, fp16")
    seed, seed_dev, draw, noise_in, noise_out = 0, None, 0, None, None
    if isinstance(noise, tuple):
        _, seed, draw, noise_out = noise
        if noise_out is not None and (tuple(noise_out.shape) != (B, 64, H, W) or not noise_out.is_contiguous()
                                      or noise_out.dtype != torch.float32):
            raise ValueError("rdab_prep_fused: noise_out must be a contiguous fp32 [B,64,H,W] tensor")
        if isinstance(seed, torch.Tensor):      # the key lives in device memory (int64[1]): graph replays re-read it
            if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != x.device:
                raise ValueError("rdab_prep_fused: a device-side key must be an int64[1] tensor on the operands' device")
            seed, seed_dev = 0, seed
        else:
            seed &= 0x7FFFFFFFFFFFFFFF
    else:
        noise_in = noise
        if tuple(noise.shape) != (B, 64, H, W) or not noise.is_contiguous() or noise.dtype != torch.float32:
            raise ValueError("rdab_prep_fused: noise must be a contiguous fp32 [B,64,H,W] tensor")
    args = (_vp(x), ld, _vp(pc.w), _vp(pc.bias), _vp(vmax), _vp(noise_in), C.c_longlong(seed), _vp(seed_dev), draw, _vp(noise_out),
            _vp(wW), _vp(bW), B, C.c_longlong(H * W), _vp(sq), 64, _vp(vrow), 64, _vp(qwin), 64, _vp(vwin), 64,
            int(row16) + 2 * int(win16))
    if _is_map(x):
        if plane is None:
            raise ValueError("rdab_prep_fused: a mapped x needs the plane form (rdab_prep_fused_map_ok)")
        view, Bi, s_b, s_g, table, _ = _plane_args(plane[:5], B, H, W, 128, "rdab_prep_fused")
        xB, xsb, xsg = x.triple()
        check(_lib.lib().cdfo_rdab_prep_fused_plane_map(args[0], ld, xB, C.c_longlong(xsb), C.c_longlong(xsg), *args[2:], _vp(view), Bi,
                                                        C.c_longlong(s_b), C.c_longlong(s_g), W, _vp(table), _stream()),
              "cdfo_rdab_prep_fused_plane_map")
    elif plane is not None:
        view, Bi, s_b, s_g, table, _ = _plane_args(plane[:5], B, H, W, 128, "rdab_prep_fused")
        check(_lib.lib().cdfo_rdab_prep_fused_plane(*args, _vp(view), Bi, C.c_longlong(s_b), C.c_longlong(s_g), W, _vp(table), _stream()),
              "cdfo_rdab_prep_fused_plane")
    else:
        check(_lib.lib().cdfo_rdab_prep_fused(*args, _stream()), "cdfo_rdab_prep_fused")
    return sq, vrow, qwin, vwin


_seed_counter = 0


def next_noise_seed(device) -> int:
    """A fresh 63-bit Philox key per forward, reproducible under torch.manual_seed: taken from (and advancing) the state
    of torch's default generator of `device` -- plumbing only, no random numbers are drawn by torch."""
    global _seed_counter
    if torch.cuda.is_current_stream_capturing():
        # the generator refuses state changes during a graph capture; a captured forward reads its key from device memory
        # anyway (CVSR_V8.refresh_noise_key rewrites it before every replay), so this value only seeds the capture run
        base, off = int(torch.initial_seed()), 4 * _seed_counter
        _seed_counter += 1
    else:
        g = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        base, off = int(g.initial_seed()), int(g.get_offset())
        g.set_offset(off + 4)
    return (base * 0x9E3779B97F4A7C15 + off * 0xD1B54A32D192ED03 + 0x632BE59BD9B4E019) & 0x7FFFFFFFFFFFFFFF


def colconv9(x: torch.Tensor, wH: torch.Tensor, bH: torch.Tensor) -> torch.Tensor:
    B, H, W, Cc, ld = _chk_act(x)
    out = empty_act(B, H, W, 64, x.device)
    check(_lib.lib().cdfo_colconv9(_vp(x), ld, _vp(wH), _vp(bH), B, H, W, _vp(out), 64, _stream()), "cdfo_colconv9")
    return out


def seq_attn(q: torch.Tensor, v: torch.Tensor, mode: int, out: Optional[torch.Tensor] = None,
             out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Modes 20-22 (single-fp16 second product) also take v as fp16 -- (fp16)v, the rounding they apply to an fp32 v while staging:
    the same result at half the bytes --, and mode 20 can leave its result as fp16 (`out` of that dtype, or out_dtype), the form in
    which mode 21 would round it as ITS v.  16-bit operands with any other mode raise."""
    if out is not None:
        out_dtype = out.dtype
    v_f16, out_f16 = v.dtype == torch.float16, out_dtype == torch.float16
    if (v_f16 and mode not in (20, 21, 22)) or (out_f16 and mode != 20):
        raise ValueError(f"seq_attn: an fp16 v needs mode 20, 21 or 22 and an fp16 out mode 20, got mode {mode}")
    B, H, W, Cc, ldq = _chk_act(q, "q")
    _, _, _, _, ldv = _chk_act(v, "v", v.dtype if v_f16 else torch.float32)
    if out is None:
        out = torch.empty((B, H, W, 64), dtype=out_dtype, device=q.device)
    _, _, _, _, ldo = _chk_act(out, "out", out_dtype if out_f16 else torch.float32)
    if v_f16 or out_f16:
        check(_lib.lib().cdfo_seq_attn_f16(_vp(q), ldq, _vp(v), ldv, _vp(out), ldo, B, H, W, mode, int(v_f16), int(out_f16),
                                           _stream()), "cdfo_seq_attn_f16")
        return out
    check(_lib.lib().cdfo_seq_attn(_vp(q), ldq, _vp(v), ldv, _vp(out), ldo, B, H, W, mode, _stream()), "cdfo_seq_attn")
    return out


# ------------------------------------------------------------------------------------- training batches and the training loss
def _train_batch(who, lr, pms, rms, ufs, mvl0, mvl1, hr, plan, crop):
    """Both forms of a training batch: ``mvl1`` None is the LD form (cdfo_train_batch), a tensor the RA form (cdfo_train_batch_ra)."""
    S, T, H, W = lr.shape
    want = [(lr, torch.uint8, (S, T, H, W)), (pms, torch.uint8, (S, T, H, W)), (rms, torch.int8, (S, T, H, W)),
            (ufs, torch.uint8, (S, T, ufs.shape[2] if ufs.dim() == 4 else -1, W)), (mvl0, torch.int8, (S, T, H, W, 3)),
            (hr, torch.uint8, (S, T, 4 * H, 4 * W))]
    if mvl1 is not None:
        want.append((mvl1, torch.int8, (S, T, H, W, 3)))
    for t, dtype, shape in want:
        if not t.is_cuda or t.device != lr.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: a dense {dtype} device tensor {shape} expected, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if plan.dtype != torch.int32 or plan.dim() != 2 or plan.shape[1] != 8 or not plan.is_contiguous() or plan.device != lr.device \
            or plan.shape[0] == 0:
        raise ValueError(f"{who}: the plan is a dense int32 [B,8] tensor on the clip set's device, B >= 1")
    B, c, dev = int(plan.shape[0]), int(crop), lr.device
    if c <= 0 or c % 4 or c > min(H, W):
        raise ValueError(f"{who}: crop must be a positive multiple of 4 that fits the {H}x{W} frames, got {crop}")
    f32 = dict(dtype=torch.float32, device=dev)
    x, pm = torch.empty((B, 7, 1, c, c), **f32), torch.empty((B, 7, 1, c, c), **f32)
    rm, uf = torch.empty((B, 1, 7, c, c), **f32), torch.empty((B, 1, 7, c, c), **f32)
    mvs0, hro = torch.empty((B, 7, 2, c, c), **f32), torch.empty((B, 1, 4 * c, 4 * c), **f32)
    tail = (S, T, H, W, int(ufs.shape[2]), _vp(plan), B, c, _vp(x), _vp(pm), _vp(rm), _vp(uf), _vp(mvs0), _vp(hro), _stream())
    if mvl1 is None:
        check(_lib.lib().cdfo_train_batch(_vp(lr), _vp(pms), _vp(rms), _vp(ufs), _vp(mvl0), _vp(hr), *tail), "cdfo_train_batch")
    else:
        check(_lib.lib().cdfo_train_batch_ra(_vp(lr), _vp(pms), _vp(rms), _vp(ufs), _vp(mvl0), _vp(mvl1), _vp(hr), *tail),
              "cdfo_train_batch_ra")
    return x, mvs0, pm, rm, uf, hro


def train_batch(lr: torch.Tensor, pms: torch.Tensor, rms: torch.Tensor, ufs: torch.Tensor, mvl0: torch.Tensor, hr: torch.Tensor,
                plan: torch.Tensor, crop: int):
    """The resident clip set (cdfo_amd/train_data.py::ClipSet's tensors) and a device plan int32 [B,8] -> (x, mvs0, pms, rms, ufs, hr)
    of B samples in one launch.  The plan's rows are the caller's to validate (ClipSet.batch does); shapes and dtypes are checked here."""
    return _train_batch("train_batch", lr, pms, rms, ufs, mvl0, None, hr, plan, crop)


def train_batch_ra(lr: torch.Tensor, pms: torch.Tensor, rms: torch.Tensor, ufs: torch.Tensor, mvl0: torch.Tensor, mvl1: torch.Tensor,
                   hr: torch.Tensor, plan: torch.Tensor, crop: int):
    """`train_batch` for a random-access clip set: ``mvl1`` is the second list's field, int8 and dense in ``mvl0``'s shape, and the
    returned flow field (x, mvs, pms, rms, ufs, hr) is built from both lists (opt/data_RA_bi.py:495-533); it serves as mvs0 and mvs1."""
    if mvl1 is None:
        raise ValueError("train_batch_ra: mvl1 is required")
    return _train_batch("train_batch_ra", lr, pms, rms, ufs, mvl0, mvl1, hr, plan, crop)


CHARBONNIER_MAX_BLOCKS = 1024        # CDFO_CHARBONNIER_MAX_BLOCKS of include/cdfo_hip.h


def charbonnier(sr: torch.Tensor, hr: torch.Tensor, eps: float):
    """(loss fp32 scalar, g fp32 like sr): the sum of sqrt((sr - hr)^2 + eps) and its derivative by sr, one pass; no host sync."""
    for name, t in (("sr", sr), ("hr", hr)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"charbonnier: {name} must be a dense fp32 device tensor, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    if sr.shape != hr.shape or sr.device != hr.device or sr.numel() == 0:
        raise ValueError(f"charbonnier: sr and hr must have one non-empty shape on one device, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    n = sr.numel()
    g = torch.empty_like(sr)
    partial = torch.empty(CHARBONNIER_MAX_BLOCKS, dtype=torch.float64, device=sr.device)
    loss = torch.empty((), dtype=torch.float32, device=sr.device)
    check(_lib.lib().cdfo_charbonnier(_vp(sr), _vp(hr), C.c_longlong(n), C.c_float(eps), _vp(g), _vp(partial), CHARBONNIER_MAX_BLOCKS,
                                      _vp(loss), _stream()), "cdfo_charbonnier")
    return loss, g


FFL_MIN, FFL_MAX = 16, 512           # CDFO_FFL_MIN, CDFO_FFL_MAX of include/cdfo_hip.h
_ffl_tables = {}                     # (device, n) -> the twiddle table of length n there: uploaded once per process and device


def ffl_size(n) -> bool:
    """Whether ``n`` is a transform length of the focal frequency loss: a power of two from 16 to 512."""
    return isinstance(n, int) and FFL_MIN <= n <= FFL_MAX and n & (n - 1) == 0


def ffl_twiddles(n: int) -> np.ndarray:
    """fp32 [n/2, 2]: (cos, sin)(2 pi k / n) for k < n / 2, computed in fp64 and rounded once."""
    if not ffl_size(n):
        raise ValueError(f"ffl_twiddles: a power of two from {FFL_MIN} to {FFL_MAX} expected, got {n!r}")
    a = 2.0 * np.pi * np.arange(n // 2, dtype=np.float64) / n
    return np.stack((np.cos(a), np.sin(a)), axis=1).astype(np.float32)


def _ffl_table_on(device, n: int) -> torch.Tensor:
    if (device, n) not in _ffl_tables:
        _ffl_tables[device, n] = torch.from_numpy(ffl_twiddles(n)).to(device)
    return _ffl_tables[device, n]


def _ffl_frames(sr: torch.Tensor, hr: torch.Tensor, who: str):
    """(N, H, W) of two dense fp32 device tensors [N,1,H,W] or [N,H,W] of one shape on one device; anything else is a ValueError."""
    for name, t in (("sr", sr), ("hr", hr)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[1] != 1):
            raise ValueError(f"{who}: {name} must be a dense fp32 device tensor [N,1,H,W] or [N,H,W], got {t.dtype} {tuple(t.shape)} "
                             f"strides {t.stride()}")
    if sr.shape != hr.shape or sr.device != hr.device or sr.shape[0] == 0:
        raise ValueError(f"{who}: sr and hr must have one shape with N >= 1 on one device, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    N, H, W = int(sr.shape[0]), int(sr.shape[-2]), int(sr.shape[-1])
    if not ffl_size(H) or not ffl_size(W) or N > 65535:
        raise ValueError(f"{who}: H and W must be powers of two from {FFL_MIN} to {FFL_MAX} and N at most 65535, got N = {N}, {H} x {W}")
    return N, H, W


def ffl_alpha(alpha, who: str) -> float:
    """``alpha`` as the float the kernels take, or a ValueError: a finite real number >= 0 (it crosses the C ABI as fp32)."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not np.isfinite(alpha) or alpha < 0 or alpha > 3.4e38:
        raise ValueError(f"{who}: alpha must be a finite number >= 0, got {alpha!r}")
    return float(alpha)


def _ffl_spectrum(sr, hr, N, H, W):
    """(F fp32 [N,H,W,2], pmax fp64 [N,P]) of cdfo_ffl_spectrum."""
    dev = sr.device
    P = W // (8 if H > 256 else 16)                                          # cdfo_ffl_tiles
    F = torch.empty((N, H, W, 2), dtype=torch.float32, device=dev)
    pmax = torch.empty((N, P), dtype=torch.float64, device=dev)
    check(_lib.lib().cdfo_ffl_spectrum(_vp(sr), _vp(hr), N, H, W, _vp(_ffl_table_on(dev, H)), _vp(_ffl_table_on(dev, W)), _vp(F), _vp(pmax),
                                       N * P, _stream()), "cdfo_ffl_spectrum")
    return F, pmax


def ffl_spectrum(sr: torch.Tensor, hr: torch.Tensor) -> torch.Tensor:
    """complex64 [N,H,W]: fft2(sr - hr, norm="ortho"), the full spectrum.  A test surface of the loss's transform, not a general FFT."""
    N, H, W = _ffl_frames(sr, hr, "ffl_spectrum")
    return torch.view_as_complex(_ffl_spectrum(sr, hr, N, H, W)[0])


def ffl_loss(sr: torch.Tensor, hr: torch.Tensor, alpha: float = 1.0, want_grad: bool = True):
    """(loss fp32 [N], g fp32 like sr or None): the focal frequency loss of each frame and, with ``want_grad``, its derivative by sr
    (the two inverse passes; skipped otherwise).  Scratch: the spectrum, 8 N H W bytes, and two small fp64 arrays; no host sync."""
    N, H, W = _ffl_frames(sr, hr, "ffl_loss")
    alpha = ffl_alpha(alpha, "ffl_loss")
    dev = sr.device
    F, pmax = _ffl_spectrum(sr, hr, N, H, W)
    S = max(1, H * W // 4096)                                                # cdfo_ffl_strips
    partial = torch.empty((N, S), dtype=torch.float64, device=dev)
    loss = torch.empty(N, dtype=torch.float32, device=dev)
    check(_lib.lib().cdfo_ffl_weight(_vp(F), _vp(pmax), pmax.shape[1], N, H, W, C.c_float(alpha), int(bool(want_grad)), _vp(partial), N * S,
                                     _vp(loss), _stream()), "cdfo_ffl_weight")
    if not want_grad:
        return loss, None
    g = torch.empty_like(sr)
    check(_lib.lib().cdfo_ffl_inverse(_vp(F), N, H, W, _vp(_ffl_table_on(dev, H)), _vp(_ffl_table_on(dev, W)), _vp(g), _stream()),
          "cdfo_ffl_inverse")
    return loss, g


SSIM_LOSS_MIN, SSIM_LOSS_MS_MIN, SSIM_LOSS_MAX = 11, 176, 16384      # one window; CDFO_MSSSIM_MIN; the entry points' largest side
SSIM_LOSS_TILE = (16, 32)                                             # rows x columns of valid positions a workgroup takes


def ssim_loss_peak(peak, who: str) -> float:
    """``peak`` as the double the kernels take, or a ValueError: a finite real number > 0."""
    if isinstance(peak, bool) or not isinstance(peak, (int, float)) or not np.isfinite(peak) or peak <= 0:
        raise ValueError(f"{who}: peak must be a finite number > 0, got {peak!r}")
    return float(peak)


def ssim_loss_tiles(H: int, W: int, levels: int) -> int:
    """cdfo_ssim_loss_tiles: the tiles of all levels of an H x W frame."""
    th, tw = SSIM_LOSS_TILE
    return sum(-(-((H >> j) - 10) // th) * -(-((W >> j) - 10) // tw) for j in range(levels))


def _ssim_loss_frames(sr: torch.Tensor, hr: torch.Tensor, levels: int, who: str):
    """(N, H, W) of two dense fp32 device tensors [N,1,H,W] or [N,H,W] of one shape on one device; anything else is a ValueError."""
    if levels not in (1, 5):
        raise ValueError(f"{who}: 1 or 5 levels expected, got {levels!r}")
    for name, t in (("sr", sr), ("hr", hr)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[1] != 1):
            raise ValueError(f"{who}: {name} must be a dense fp32 device tensor [N,1,H,W] or [N,H,W], got {t.dtype} {tuple(t.shape)} "
                             f"strides {t.stride()}")
    if sr.shape != hr.shape or sr.device != hr.device or sr.shape[0] == 0:
        raise ValueError(f"{who}: sr and hr must have one shape with N >= 1 on one device, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    N, H, W = int(sr.shape[0]), int(sr.shape[-2]), int(sr.shape[-1])
    lo = SSIM_LOSS_MS_MIN if levels == 5 else SSIM_LOSS_MIN
    if min(H, W) < lo or max(H, W) > SSIM_LOSS_MAX or N > 65535:
        raise ValueError(f"{who}: H and W must be from {lo} to {SSIM_LOSS_MAX} and N at most 65535, got N = {N}, {H} x {W}")
    return N, H, W


def ssim_loss(sr: torch.Tensor, hr: torch.Tensor, peak: float = 1.0, levels: int = 1, want_grad: bool = True):
    """(loss fp32 [N], g fp32 like sr or None): ``1 - SSIM`` (``levels`` 1) or ``1 - MS-SSIM`` (5) of each frame and, with
    ``want_grad``, its derivative by sr (the P/Q/R and adjoint passes, coarsest level first; skipped otherwise).  Launches: ``levels``
    sums, ``levels - 1`` pools, one combine, and ``2 levels`` for the gradient.  Scratch until it returns: the pyramid of both frames
    (8 N h_j w_j bytes per level j >= 1), the tile sums, means and coefficients, and for the gradient the three fp64 maps of the
    largest level (24 N (H - 10)(W - 10) bytes) and the fp64 gradients of levels >= 1.  No host synchronisation."""
    N, H, W = _ssim_loss_frames(sr, hr, levels, "ssim_loss")
    peak = ssim_loss_peak(peak, "ssim_loss")
    dev, lib = sr.device, _lib.lib()
    T = ssim_loss_tiles(H, W, levels)                                        # cdfo_ssim_loss_tiles
    partial = torch.empty((N, T, 2), dtype=torch.float64, device=dev)
    xs, ys = [sr], [hr]
    for j in range(levels):
        if j:
            h, w = H >> (j - 1), W >> (j - 1)
            xs.append(torch.empty((N, h >> 1, w >> 1), dtype=torch.float32, device=dev))
            ys.append(torch.empty((N, h >> 1, w >> 1), dtype=torch.float32, device=dev))
            check(lib.cdfo_ssim_loss_pool(_vp(xs[j - 1]), _vp(ys[j - 1]), N, h, w, _vp(xs[j]), _vp(ys[j]), _stream()), "cdfo_ssim_loss_pool")
        check(lib.cdfo_ssim_loss_level(_vp(xs[j]), _vp(ys[j]), N, H, W, levels, j, peak, _vp(partial), partial.numel(), _stream()),
              "cdfo_ssim_loss_level")
    means = torch.empty((N, levels, 2), dtype=torch.float64, device=dev)
    coef = torch.empty((N, levels, 2), dtype=torch.float64, device=dev)
    loss = torch.empty(N, dtype=torch.float32, device=dev)
    check(lib.cdfo_ssim_loss_combine(_vp(partial), partial.numel(), N, H, W, levels, _vp(means), _vp(coef), _vp(loss), _stream()),
          "cdfo_ssim_loss_combine")
    if not want_grad:
        return loss, None
    pqr = torch.empty(3 * N * (H - 10) * (W - 10), dtype=torch.float64, device=dev)
    g, coarse = torch.empty_like(sr), None
    for j in range(levels - 1, -1, -1):
        check(lib.cdfo_ssim_loss_pqr(_vp(xs[j]), _vp(ys[j]), N, H, W, levels, j, peak, _vp(coef), _vp(pqr), pqr.numel(), _stream()),
              "cdfo_ssim_loss_pqr")
        g64 = torch.empty((N, H >> j, W >> j), dtype=torch.float64, device=dev) if j else None
        check(lib.cdfo_ssim_loss_adjoint(_vp(pqr), _vp(xs[j]), _vp(ys[j]), N, H, W, levels, j, _vp(coarse), _vp(g64), _vp(None if j else g),
                                         _stream()), "cdfo_ssim_loss_adjoint")
        coarse = g64
    return loss, g
