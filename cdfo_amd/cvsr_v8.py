"""``CVSR_V8`` -- the reference's seven-frame x4 VSR model (arch/SIDECVSR_our.py:4371-4481) with the forward pass
running entirely in hand-written gfx950 kernels (libcdfo_hip.so, C-ABI in include/cdfo_hip.h).

Drop-in boundary B1: same class name, constructor signature, ``forward(x, mvs0, mvs1, pms, rms,
ufs, pre_L1_fea=None) -> (out, L1_fea)`` and the same 261 ``state_dict`` entries (names + shapes), so a published
``.pth`` loads with ``load_state_dict(strict=True)``.

Differences, all deliberate:
  * forward needs CUDA (ROCm) tensors: there is NO CPU fallback -- it raises ``NotImplementedError`` like the reference's
    own CUDA-only operator does (ops/dcn/deform_conv.py:136).  Under ``torch.no_grad()`` the fused inference schedule of
    this file runs; with gradients enabled (``train_LD_37.py:376-381``) the call goes to ``cvsr_v8_train.forward_train``:
    the plain operator graph under torch autograd, HIP kernels forward and backward (convolutions as split-bf16 3-pass MFMA
    products by default, exact fp32 with ``CDFO_TRAIN_EXACT=1``; everything else exact fp32: ``cdfo_amd/autograd.py``).
  * ``gumbel_uniform=`` (kwarg or attribute): the six uniform draws of ``LLongRangAttention.gumbel_softmax``
    (arch.py:2169) may be injected as six ``[B,64,H,W]`` tensors; by default they are drawn like the reference does
    (fresh uniforms per call, never 0), by a Philox4x32-10 generator inside the mask kernel, keyed per forward from
    torch's default generator (``torch.manual_seed`` reproduces a run); ``capture_noise = []`` collects the values drawn.
  * ``range_guard`` (default True; any truthy value, the older ``"sync"`` included, turns it on): in the default ``fp16x2``
    mode a forward whose activations leave fp16's range is detected (max |trunk input| outside [2^-6, 2^11], or a non-finite
    trunk input / result) and repeated in ``bf16x3``.  Both checks are settled before the call returns (one host sync per
    forward), so what it returns is final; ``last_range`` holds what the guard saw.
  * ``precision`` attribute: "f32" | "bf16x3" | "fp16x2" (default) | "bf16" selects the matrix-core arithmetic of the
    wide 3x3 convolutions; "f32", "bf16x3" and "fp16x2" meet the 1e-3 max-abs parity bound against the fp32 reference
    (1e-6, 1e-5 and 3-5e-4 respectively), "bf16" does not (6e-3).
  * the debug side effects of the reference forward (``featuremap_visual`` PNG dumps, arch.py:4450-4475) are absent.
  * ``L1_fea`` is returned as a ``[B*7,64,H,W]`` tensor in channels-last memory format (a view of the kernels'
    pixel-major buffer); feeding it back as ``pre_L1_fea`` needs no conversion.  Plain NCHW tensors are accepted too.
  * ``extract_features`` / ``forward_windows`` serve one sequence K centre frames per call (StreamingSR.run_chunked): same
    arithmetic per output frame.  ``compensate_features`` / ``forward_windows_shared`` (opt-in,
    ``run_chunked(share_compensation=True)``) also run the per-frame half of the neighbour pipelines once per FRAME, with one
    Gumbel draw per frame where the reference draws per (forward, slot): every window still sees six draws (independent when its
    neighbour frames are distinct), but windows that hold the same frame share its draw.
"""
from __future__ import annotations

import threading

import contextlib
import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import kernels as K
from . import switches

NF, NFRAMES = 64, 7


# ------------------------------------------------------------------------------------------------ parameters
def _param_spec():
    """(key, shape, fan_in, init) of the reference's state_dict (arch.py:4379-4398 and the sub-modules it builds)."""
    sp = []

    def conv(key, co, ci, kh, kw=None, bias=True, init="default"):
        kw = kw or kh
        sp.append((key + ".weight", (co, ci, kh, kw), ci * kh * kw, init))
        if bias:
            sp.append((key + ".bias", (co,), ci * kh * kw, "zero" if init == "kaiming0.1" else "bias"))

    conv("conv_first", 64, 1, 3)
    conv("conv_second", 64, 1, 3)
    p = "transformer_feature_extraction.path1."
    for n in ("norm1", "norm2"):
        sp.append((p + n + ".body.weight", (64,), None, "ones"))
        sp.append((p + n + ".body.bias", (64,), None, "zero"))
    sp.append((p + "attn.temperature", (8, 1, 1), None, "ones"))
    conv(p + "attn.qkv", 192, 64, 1, bias=False)
    conv(p + "attn.qkv_dwconv", 192, 1, 3, bias=False)
    conv(p + "attn.project_out", 64, 64, 1, bias=False)
    conv(p + "conv", 64, 64, 3)
    u = p + "side_to_feaoneUDSA.body."
    conv(u + "0", 16, 64, 3)
    conv(u + "2", 16, 16, 3)
    conv(u + "4", 16, 16, 3)
    conv(u + "6.spatial", 1, 2, 7)
    conv(u + "7", 16, 16, 3)
    conv(u + "9", 16, 16, 3)
    conv(u + "11", 64, 16, 3)
    conv("conv_expand_fea_r", 64, 128, 3)
    conv("conv_expand_ufs", 64, 1, 3)
    conv("conv_expand_rms", 64, 1, 3)
    conv("tsa_fusion", 64, 448, 1)
    for g in range(7):
        gp = f"recon_trunk.body.{g}."
        conv(gp + "conv", 64, 64, 3)
        for b in range(3):
            bp = gp + f"body.{b}."
            conv(bp + "body.0", 256, 64, 3, init="kaiming0.1")
            conv(bp + "body.2", 64, 256, 3, init="kaiming0.1")
            conv(bp + "down.0", 64, 64, 1, init="kaiming0.1")
            conv(bp + "up.0", 64, 64, 1, init="kaiming0.1")
    conv("upconv1", 256, 64, 1)
    conv("upconv2", 256, 64, 1)
    conv("conv_last", 1, 64, 3)
    a = "MV_deform_align."
    sp.append((a + "temperature", (4, 1, 1), None, "ones"))
    conv(a + "conv_du.0", 4, 64, 1)
    conv(a + "conv_du.2", 64, 4, 1)
    conv(a + "project_out", 64, 64, 1, bias=False)
    conv(a + "fusion_in.0", 64, 128, 1)          # has parameters, never called (arch.py:3441-3444)
    conv(a + "fusion_in.2", 64, 64, 1)
    conv(a + "fusion_out.0", 64, 128, 1, bias=False)
    conv(a + "CALayer.conv_du.0", 64, 64, 1)
    conv(a + "CALayer.conv_du.2", 64, 64, 1)
    for rb in ("ResidualBlock.", "ResidualBlock1."):
        conv(a + rb + "conv1", 64, 64, 3, init="kaiming0.1")
        conv(a + rb + "conv2", 64, 64, 3, init="kaiming0.1")
    r = "RDAB."
    conv(r + "input_conv", 128, 64, 1)
    conv(r + "conv_du_re.0", 64, 64, 1)
    conv(r + "conv_du_re.2", 64, 64, 3)
    conv(r + "conv_du_re2.0", 64, 64, 1)
    conv(r + "fuse", 64, 128, 1)
    conv(r + "directW1_conv", 1, 1, 1, 9)
    conv(r + "directH1_conv", 1, 1, 9, 1)
    return sp


class _Holder(nn.Module):
    """Parameter container: reproduces the reference's module tree names without its Python forward code."""


def _register(root: nn.Module, key: str, param: nn.Parameter):
    parts = key.split(".")
    m = root
    for name in parts[:-1]:
        if name not in m._modules:
            m.add_module(name, _Holder())
        m = m._modules[name]
    m.register_parameter(parts[-1], param)


# ------------------------------------------------------------------------------------------------ the module
class _FeatureStack:
    """The frames' features of B clips where they lie: frame i of clip b starts i * s_f + b * s_c floats behind T's first element
    (clip-major L1 [B*7,H,W,64]: s_f = P 64, s_c = 7 P 64; a frame-major window stack [7,B,H,W,64]: s_f = B P 64, s_c = P 64).  The
    neighbour phase takes its operands from it as image maps (K.image_map): nothing is copied."""

    def __init__(self, T, B, H, W, s_f, s_c):
        self.T, self.B, self.H, self.W, self.s_f, self.s_c = T, B, H, W, s_f, s_c

    def _first(self, i):
        return self.T.as_strided((self.H, self.W, NF), (self.W * NF, NF, 1), self.T.storage_offset() + i * self.s_f)

    def group(self, i0, G):
        """Frames i0 .. i0 + G - 1 of every clip, neighbour major: [G*B,H,W,64]."""
        return K.image_map(self._first(i0), G * self.B, self.B, self.s_c, self.s_f)

    def frame(self, i, times=1):
        """Frame i of every clip, addressed `times` times over: [times*B,H,W,64]."""
        return K.image_map(self._first(i), times * self.B, self.B, self.s_c, 0)


class CVSR_V8(nn.Module):
    def __init__(self, nf=64, nframes=7, fea_ext_RBs=7, SCGs=4, istraining=False):
        super().__init__()
        if nf != 64 or nframes != 7:
            raise ValueError("the HIP path is specialised for nf=64, nframes=7 (the only configuration the reference runs)")
        self.nf, self.center, self.istraining, self.stride = nf, nframes // 2, istraining, 4
        self.gumbel_uniform: Optional[Sequence[torch.Tensor]] = None
        # arithmetic of the wide 3x3 convolutions (89 % of the FLOPs):
        #   "f32"    exact fp32 MFMA (1e-6 max-abs on the forward vs the fp32 reference);
        #   "bf16x3" split-bf16 3-pass MFMA (fp32-grade: ~1e-5);
        #   "fp16x2" fp16 weights; fp16 hi+lo activations (2 MFMA passes), single fp16 rounding (1 pass) inside Block_, whose
        #            256-channel intermediates also live in HBM as fp16; the returned feature cache stays split-bf16
        #            (2-4e-4 max-abs: inside the 1e-3 parity bound; default);
        #   "bf16"   plain bf16 MFMA with fp32 accumulation (BASELINE's bf16 configuration, ~6e-3: outside the bound).
        self._precision = "fp16x2"      # read through the `precision` property (a per-thread override serves the range guard's retry)
        # HIP side streams for the two independent neighbour groups (frames 0-2 and 4-6): 1 = everything on the caller's
        # stream, 0 = auto = 2 (one side stream per group)
        self.neighbour_streams = 0
        self.udsa_n16 = switches.get("CDFO_UDSA_N16")       # developer A/B: the prior U-net's first layer, see _udsa
        self.udsa_side_stream = switches.get("CDFO_UDSA_STREAM")   # developer A/B, see _feature_extraction
        self.attn_pv_single = not switches.get("CDFO_ATTN_PV3")    # see _rdab (developer A/B: CDFO_ATTN_PV3=1 -> three passes)
        # see _rdab (developer A/B: CDFO_RDAB_FUSED=0 -> input_conv and the mask kernel as two launches, every V operand fp32)
        self.rdab_fused = switches.get("CDFO_RDAB_FUSED")
        # the one-channel prior planes stay one-channel inside their consumers (see _compensate: the mask statistics straight from
        # the residual maps; developer A/B: CDFO_PRIOR_STEMS=0 -> du0 written by the stem kernel and read back by a convolution)
        self.prior_stems = switches.get("CDFO_PRIOR_STEMS")
        # ... and fea_com = fea + conv_expand_rms(rms) is never written: its two readers (the mask kernel's input_conv, RDAB.fuse's
        # residual) read fea and take the stencil's part as one more k-step built from the residual map (see _compensate, _rdab;
        # developer A/B: CDFO_INLINE_RMS=0 -> the stem kernel writes fea_com).  Needs prior_stems: without it the stem launch that
        # writes du0 writes fea_com anyway
        self.inline_rms = switches.get("CDFO_INLINE_RMS")
        # ... and ufs_prior = conv_expand_ufs(ufs) is never written either: its two readers (the alignment's statistics pass and the
        # folded 192 -> 64 convolution) take it as the plane chunk of their products from the partition map (see _align_group, _align;
        # developer A/B: CDFO_INLINE_UFS=0 -> one stem launch per neighbour writes ufs_prior).  Needs align_stats
        self.inline_ufs = switches.get("CDFO_INLINE_UFS")
        # ... and the neighbour phase reads the feature stack where the extractor wrote it: no frame-major copy, no centre features
        # repeated per neighbour -- its seven readers take an image map (see _stack_inplace; developer A/B: CDFO_STACK_INPLACE=0 ->
        # K.swap_outer and the repeat of the rounds before)
        self.stack_inplace = switches.get("CDFO_STACK_INPLACE")
        self.neighbour_group = 0      # frames per neighbour group: 0 = auto = 3
        # cached-feature call on one sequence (B = 1): the group of frames 0-2 (cached features only) starts beside the new
        # frame's feature extraction instead of behind it (see _forward)
        self.overlap_new_frame = switches.get("CDFO_OVERLAP_NEW")
        # ... and the new frame's own neighbour pipeline follows the extraction as a group of one, frames 4-5 on the second side
        # stream (tools/bench_streaming.py, 24 frames 270x480, eager / HIP graph: 65.4 / 67.1 frames/s without the overlap,
        # 66.7 / 67.6 with it, 66.9 / 68.0 with the new frame alone)
        self.new_frame_alone = switches.get("CDFO_NEW_ALONE")
        # Block_: the half-resolution branch on a side stream beside the other two (see _block)
        self.trunk_side_stream = switches.get("CDFO_TRUNK_SIDE")
        # (the x2 branch's 256-channel intermediate in half-split rows: the Winograd kernel's lanes then store contiguous runs;
        # measured: no gain in the forward (105.2 vs 105.3 ms), off by default)
        self.wino_halfsplit = switches.get("CDFO_WINO_HS")
        # DualAttAlignment's statistics in one pass that never writes kf, CALayer's pool from the producing epilogue (see _align;
        # developer A/B: CDFO_ALIGN_STATS=0 -> the five launches of round 5)
        self.align_stats = switches.get("CDFO_ALIGN_STATS")
        # fp16x2 mode, the feature extractor's two 3x3 convolutions on the ring kernel: True = activations fp16 hi + lo x
        # weights fp16 hi + lo (three terms, fp32-grade: L1_fea 1.3e-5 max-abs); False = weights rounded once to fp16 (two
        # terms): measured 1.7e-3 on the RETURNED feature cache (|L1_fea| up to 7), outside the 1e-3 bound, for 1.3 ms per
        # step -- so the three-term product stays.  Set before the first forward (it selects the weight packing).
        self.fe_weight_lo = True
        # fp16x2 mode, conv_expand_fea_r (arch.py:4454; 128 -> 64, 3x3, twice per forward on 3*B images): False = fp16 hi + lo
        # activations (two MFMA passes), True = activations rounded once to fp16 like the convolutions inside Block_ (one pass)
        self.fea_r_single_pass = switches.get("CDFO_FEA_R_1PASS")
        for key, shape, fan_in, init in _param_spec():
            t = torch.empty(shape)
            if init == "default":
                nn.init.kaiming_uniform_(t, a=math.sqrt(5))
            elif init == "kaiming0.1":
                nn.init.kaiming_normal_(t, a=0, mode="fan_in")
                t.mul_(0.1)
            elif init == "bias":
                bound = 1.0 / math.sqrt(fan_in)
                nn.init.uniform_(t, -bound, bound)
            elif init == "ones":
                t.fill_(1.0)
            else:
                t.zero_()
            _register(self, key, nn.Parameter(t))
        self.debug_taps: Optional[dict] = None      # set to {} to collect stage outputs (tests only)
        self.capture_noise: Optional[list] = None   # set to [] to receive the six uniform tensors the default path drew
        self._noise_seed = 0
        self._noise_key: Optional[torch.Tensor] = None   # device-side Philox key of captured forwards (refresh_noise_key)
        # fp16 range guard of the fp16x2 mode (see forward; a truthy flag); costs one 16-byte device->host readback and host
        # sync per forward.  Callers that capture the forward into a HIP graph by hand set it to False (model.capture() carries
        # it).  last_range: what it saw in the most recent guarded forward
        self.range_guard = True
        self.last_range: Optional[dict] = None
        self._probe = None
        self._warned_range = False
        # frames sent through feature extraction since construction (every inference route counts here; StreamingSR reports it)
        self.frames_extracted = 0
        # frames sent through compensate_features (the per-frame half of the neighbour pipeline, shared-compensation mode)
        self.frames_compensated = 0
        self._packed: Optional[dict] = None
        self._packed_sig = None

    # -- packed / device-resident weights, rebuilt whenever a parameter changed ----------------------------------
    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _weights(self) -> dict:
        sig = self._signature()
        if self._packed is not None and sig == self._packed_sig:
            return self._packed
        sd = {k: v.detach() for k, v in self.named_parameters()}
        for k, v in sd.items():
            if not v.is_cuda:
                raise NotImplementedError("CVSR_V8 (HIP): parameters must live on the GPU; call .cuda() / .to(device)")
            if v.dtype != torch.float32:
                raise NotImplementedError("CVSR_V8 (HIP): fp32 parameters expected")
        w: Dict[str, object] = {}

        def pc(key, **kw):
            w[key] = K.pack_conv(sd[key + ".weight"], sd.get(key + ".bias"), **kw)

        p = "transformer_feature_extraction.path1."
        for key in (p + "attn.qkv", p + "conv", p + "side_to_feaoneUDSA.body.0", p + "side_to_feaoneUDSA.body.11",
                    "conv_expand_fea_r", "tsa_fusion", "MV_deform_align.fusion_out.0",
                    "MV_deform_align.ResidualBlock.conv1", "MV_deform_align.ResidualBlock.conv2",
                    "MV_deform_align.ResidualBlock1.conv1", "MV_deform_align.ResidualBlock1.conv2",
                    "RDAB.input_conv", "RDAB.conv_du_re.0", "RDAB.conv_du_re.2", "RDAB.fuse"):
            pc(key)
        for g in range(7):
            pc(f"recon_trunk.body.{g}.conv")
            # the same convolution for the ring kernel: fp16 hi + lo activations (planes written by the group's last block) x
            # weights rounded once to fp16 = the tiled kernel's "fp16x2" arithmetic as a K-expanded (w | w) product
            w[f"recon_trunk.body.{g}.conv_hl2"] = K.pack_conv_hilo(sd[f"recon_trunk.body.{g}.conv.weight"],
                                                                   sd[f"recon_trunk.body.{g}.conv.bias"], weight_lo=False)
            for b in range(3):
                for leaf in ("body.0", "body.2", "down.0", "up.0"):
                    pc(f"recon_trunk.body.{g}.body.{b}.{leaf}")
        # Block_'s double-resolution branch ends in  down(body.2(.)) = 1x1(mean2x2(conv3x3(.))).  All three are linear, so
        # they compose into ONE 4x4 stride-2 convolution (16 taps instead of 4*9 per low-res output: 2.25x fewer FLOPs),
        # expressed here as a 3x3 convolution over the space-to-depth image [H,W,4*256] in which each input phase has
        # weights on 4 of the 9 taps only (tap_mask), with down.0 folded in.
        masks = []
        for ph in range(4):
            pa, pb = ph >> 1, ph & 1
            m = 0
            for dy in range(3):
                for dx in range(3):
                    if 0 <= 2 * dy + pa - 1 <= 3 and 0 <= 2 * dx + pb - 1 <= 3:
                        m |= 1 << (dy * 3 + dx)
            masks += [m] * 16
        tap_mask = torch.tensor(masks, dtype=torch.int32, device=sd["conv_first.weight"].device)
        for g in range(7):
            for b in range(3):
                bp = f"recon_trunk.body.{g}.body.{b}."
                w3, b2 = sd[bp + "body.2.weight"], sd[bp + "body.2.bias"]
                wdn, bdn = sd[bp + "down.0.weight"][:, :, 0, 0], sd[bp + "down.0.bias"]
                w4 = w3.new_zeros(64, 256, 4, 4)
                for pa in range(2):
                    for pb in range(2):
                        w4[:, :, pa:pa + 3, pb:pb + 3] += 0.25 * w3
                wp = w3.new_zeros(64, 4, 256, 3, 3)
                for ph in range(4):
                    pa, pb = ph >> 1, ph & 1
                    for dy in range(3):
                        for dx in range(3):
                            u, v = 2 * dy + pa - 1, 2 * dx + pb - 1
                            if 0 <= u <= 3 and 0 <= v <= 3:
                                wp[:, ph, :, dy, dx] = w4[:, :, u, v]
                wf = torch.einsum("po,ocyx->pcyx", wdn, wp.view(64, 1024, 3, 3)).contiguous()
                fused = K.pack_conv(wf, wdn @ b2 + bdn)
                fused.tap_mask = tap_mask
                w[bp + "down_fused"] = fused
                # the half-resolution branch ends in up.0(body.2(.)) before its bilinear x2: a 1x1 after a 3x3 convolution,
                # both linear -> one 3x3 convolution (one launch and one round trip of the 64-channel tensor less per block)
                wup, bup = sd[bp + "up.0.weight"][:, :, 0, 0], sd[bp + "up.0.bias"]
                w[bp + "body.2_up"] = K.pack_conv(torch.einsum("po,ocyx->pcyx", wup, w3).contiguous(), wup @ b2 + bup)
                w[bp + "pro"] = K.pack_block_prologue(sd[bp + "up.0.weight"], sd[bp + "up.0.bias"],
                                                      sd[bp + "down.0.weight"], sd[bp + "down.0.bias"])
        fe = "transformer_feature_extraction.path1."
        wlo = bool(getattr(self, "fe_weight_lo", True))
        w[fe + "conv_hl"] = K.pack_conv_hilo(sd[fe + "conv.weight"], sd[fe + "conv.bias"], wlo)
        w[fe + "side_to_feaoneUDSA.body.11_hl"] = K.pack_conv_hilo(sd[fe + "side_to_feaoneUDSA.body.11.weight"],
                                                                   sd[fe + "side_to_feaoneUDSA.body.11.bias"], wlo)
        w[fe + "qkv_dw"] = K.pack_qkv_dw(sd[fe + "attn.qkv.weight"], sd[fe + "norm1.body.weight"], sd[fe + "norm1.body.bias"])
        # conv_du_re.0 (1x1) of the compensation module composed with conv_expand_rms (3x3 on the one-channel residual map): a
        # second 1 -> 64 stencil for the stem kernel, so that `rms_prior` is never materialised (arch.py:2200, 4446-4449)
        w["rms_du0"] = K.compose_stem_1x1(sd["conv_expand_rms.weight"], sd["conv_expand_rms.bias"], sd["RDAB.conv_du_re.0.weight"],
                                          sd["RDAB.conv_du_re.0.bias"])
        # conv_du_re.2 (3x3, stride 2, pad 2) over the space-to-depth form of its input [H/2+1, W/2+1, 4*64] (written that way by
        # the stem kernel): a stride-1 pad-1 convolution with a per-chunk tap mask (K.pack_conv_s2p2_s2d)
        w["RDAB.conv_du_re.2_s2d"] = K.pack_conv_s2p2_s2d(sd["RDAB.conv_du_re.2.weight"], sd["RDAB.conv_du_re.2.bias"])
        # ... and the same weights as bf16 hi | lo for K.rdab_stats, which forms du0 in registers and leaves only the channel sums
        w["RDAB.conv_du_re.2_stats"] = K.pack_rdab_stats(sd["RDAB.conv_du_re.2.weight"])
        # conv_expand_rms as the plane chunk of the stream kernels (K.pack_plane_chunk): by itself where fea_com is a residual
        # (RDAB.fuse), composed with input_conv (whose own bias stays in the kernel's bias table) where it is the convolution's input
        w["rms_chunk"] = K.pack_plane_chunk(sd["conv_expand_rms.weight"], sd["conv_expand_rms.bias"])
        w["rms_chunk_input_conv"] = K.pack_plane_chunk(*K.compose_stem_1x1(
            sd["conv_expand_rms.weight"], sd["conv_expand_rms.bias"], sd["RDAB.input_conv.weight"],
            torch.zeros_like(sd["RDAB.input_conv.bias"])))
        # conv_expand_ufs likewise: by itself (the statistics kernel's channel sums of ufs_prior from the map's tap sums, and what
        # align_fold_plane composes with the per-image M2), and composed with the second half of fusion_out.0 for that kernel's kf
        w["ufs_chunk"] = K.pack_plane_chunk(sd["conv_expand_ufs.weight"], sd["conv_expand_ufs.bias"])
        fo = sd["MV_deform_align.fusion_out.0.weight"]
        w["ufs_chunk_fusion_out"] = K.pack_plane_chunk(*K.compose_stem_1x1(
            sd["conv_expand_ufs.weight"], sd["conv_expand_ufs.bias"], fo[:, 64:], fo.new_zeros(fo.shape[0])))
        w[fe + "side_to_feaoneUDSA.body.0_n16"] = K.pack_conv_n16(sd[fe + "side_to_feaoneUDSA.body.0.weight"])
        w["udsa_head"] = K.pack_udsa_head(sd[fe + "side_to_feaoneUDSA.body.0.weight"], sd[fe + "side_to_feaoneUDSA.body.0.bias"],
                                          sd["conv_second.weight"], sd["conv_second.bias"])
        pc("upconv1", shuffle2=True)
        pc("upconv2", shuffle2=True)
        w["raw"] = {k: v.contiguous() for k, v in sd.items()}
        self._packed, self._packed_sig = w, sig
        return w

    # -- arithmetic of the 3x3 convolutions ---------------------------------------------------------------------
    PRECISIONS = {"f32": K.PREC_F32, "bf16x3": K.PREC_BF16X3, "bf16": K.PREC_BF16, "fp16x2": K.PREC_FP16X2}

    def _conv(self, *args, exact=False, inner=False, **kw):
        """``exact``: convolutions whose result is RETURNED to the caller (the L1_fea feature cache) never drop below
        split-bf16 accuracy, so both outputs of forward() stay inside the 1e-3 bound in every parity-grade mode."""
        prec = self.PRECISIONS[self.precision]
        if exact and prec == K.PREC_FP16X2:
            prec = K.PREC_BF16X3
        elif inner and prec == K.PREC_FP16X2:
            # convolutions inside Block_: a single fp16 rounding of their input leaves the forward's error where the
            # fp16 weight rounding puts it (2.76e-4 -> 2.78e-4 in the oracle emulation): one MFMA pass
            prec = K.PREC_FP16X1
        return K.conv(*args, prec=prec, **kw)

    # -- building blocks ------------------------------------------------------------------------------------------
    def _udsa(self, w, x2, res, head=None):
        """head: body.0's activated output when it was computed elsewhere (round 0: straight from the prior image)."""
        raw = w["raw"]
        u = "transformer_feature_extraction.path1.side_to_feaoneUDSA.body."
        if head is not None:
            t = head
        elif self.precision != "f32" and self.udsa_n16:
            # 64 -> 16 on its own streaming kernel (16 x 16 x 32 MFMA, every lane useful) instead of a quarter-filled 64-wide tile
            t = K.conv3x3_n16(x2, w[u + "0_n16"], raw[u + "0.bias"], K.ACT_LRELU)
        else:
            t = self._conv(x2, w[u + "0"], pad=1, act=K.ACT_LRELU, exact=True)
        t = K.small_conv16(t, raw[u + "2.weight"], raw[u + "2.bias"], 2, 2, act=K.ACT_LRELU)
        t = K.small_conv16(t, raw[u + "4.weight"], raw[u + "4.bias"], 2, 2, act=K.ACT_LRELU)
        t = K.spatial_gate16(t, raw[u + "6.spatial.weight"], raw[u + "6.spatial.bias"])
        t = K.small_conv16(t, raw[u + "7.weight"], raw[u + "7.bias"], 2, 2, 0, True, K.ACT_LRELU)
        if self.precision == "fp16x2":
            # the last transposed conv writes fp16 hi | lo planes; the 16 -> 64 conv (+ LeakyReLU + residual) then runs as a
            # split-fp16, fp32-grade product (a_hi*w_hi + a_lo*w_hi + a_hi*w_lo) on the LDS-DMA ring kernel, like the
            # feature extractor's 64 -> 64 conv: 3 K chunks per tile instead of the tiled kernel's restaging (1.57 -> ~0.6 ms)
            t = K.small_conv16(t, raw[u + "9.weight"], raw[u + "9.bias"], 2, 2, 1, True, K.ACT_LRELU, out_hl=True)
            return K.conv_ring(t, w[u + "11_hl"], act=K.ACT_LRELU, res1=res, plane_wrap=2)
        t = K.small_conv16(t, raw[u + "9.weight"], raw[u + "9.bias"], 2, 2, 1, True, K.ACT_LRELU)
        return self._conv(t, w[u + "11"], pad=1, act=K.ACT_LRELU, res1=res, exact=True)

    def _feature_extraction(self, w, x1, prior, P, Bn):
        """x1: conv_first features [Bn,H,W,64]; prior: the one-channel prior images (element [b][y][x] at b*P + y*W + x).
        conv_second(prior) feeds only the prior U-net's first layer of round 0 and has no activation (arch.py:4420,
        1463-1468): the two convolutions are composed (K.udsa_head), the 64-channel tensor between them never exists."""
        raw = w["raw"]
        p = "transformer_feature_extraction.path1."
        x2 = None
        main = torch.cuda.current_stream(x1.device)
        side = self._trunk_side(x1.device) if self.udsa_side_stream else None
        for rnd in range(3):
            # The prior U-net of a round is independent of its MDTA chain (they meet in the round's last convolution).  Round 1
            # tried it on a side stream: 18 % slower with that round's kernels; measured again in round 4 (udsa_side_stream).
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                if side is not None and rnd == 0:
                    side.wait_stream(main)
                if rnd == 0:
                    x2 = self._udsa(w, None, x1, head=K.udsa_head(prior, P, Bn, self.H, self.W, w["udsa_head"]))
                else:
                    x2 = self._udsa(w, x2, x2)
                if side is not None:
                    x2.record_stream(main)
            if self.precision == "f32":
                qkv = self._conv(x1, w[p + "attn.qkv"], ln=(raw[p + "norm1.body.weight"], raw[p + "norm1.body.bias"]))
                qkv = K.dwconv3x3(qkv, raw[p + "attn.qkv_dwconv.weight"])
            else:   # LayerNorm + qkv + depthwise 3x3 + the attention's Gram sums in one pass (split-bf16 MFMA, fp32-grade):
                # q and k never reach HBM, only v and 640 sums per frame
                v, part, n = K.qkv_dw(x1, w[p + "qkv_dw"], raw[p + "attn.qkv_dwconv.weight"], gram=True)
                fold = K.mdta_fold(part, n, raw[p + "attn.temperature"], raw[p + "attn.project_out.weight"])
                if self.precision == "fp16x2":      # norm2 of the result leaves the same kernel as fp16 hi | lo planes
                    x1, ln = self._conv(v, fold, res1=x1, ln_out=(raw[p + "norm2.body.weight"], raw[p + "norm2.body.bias"]))
                else:
                    x1 = self._conv(v, fold, res1=x1)
            if self.precision == "f32":
                part, n = K.gram_partial(qkv[..., 0:64], qkv[..., 64:128], 8)
                fold = K.mdta_fold(part, n, raw[p + "attn.temperature"], raw[p + "attn.project_out.weight"])
                x1 = self._conv(qkv[..., 128:192], fold, res1=x1)
            if side is not None:
                main.wait_stream(side)
            if self.precision == "fp16x2":
                # LayerNorm written as fp16 hi | lo planes; the 3x3 conv as a split-fp16 product (a_hi*w_hi + a_lo*w_hi +
                # a_hi*w_lo, 22-bit operands: fp32-grade like the split-bf16 path it replaces) on the ring kernel
                x1 = K.conv_ring(ln, w[p + "conv_hl"], res1=x1, res2=x2, plane_wrap=8)
            else:
                ln = K.layernorm64(x1, raw[p + "norm2.body.weight"], raw[p + "norm2.body.bias"])
                x1 = self._conv(ln, w[p + "conv"], pad=1, res1=x1, res2=x2, exact=True)
        return x1

    def _rdab(self, w, du0, x, noises, stats=None, rms_planes=None):
        """rms_planes = (view, Bi, s_b, s_g) (K.conv's plane addressing over the GB images; the images of one noise lie inside one
        block of Bi): the module's input is x + conv_expand_rms(plane) and only x is in memory -- the mask kernel and RDAB.fuse
        build the stencil's part from the residual maps (needs the fused mask kernel).
        LLongRangAttention (arch.py:2179-2249) on a GROUP of neighbour frames at once: du0 / x are [G*B,H,W,64] (neighbour
        major; du0 = relu(conv_du_re.0(res)) of the module's residual-map input in space-to-depth form, computed by the stem
        kernel -- or None with `stats`, the mask statistics that K.rdab_stats formed from the residual maps), `noises` one
        entry per neighbour -- the module's weights are shared by all neighbours, only the noise draw (and with it the mask
        kernel's launch) is per neighbour."""
        raw = w["raw"]
        GB, H, W, _ = x.shape
        G = len(noises)
        B = GB // G
        if stats is not None:      # (partials, slots, pixel count) of K.rdab_stats: du0 and t were never written
            part, n, count = stats
        else:
            t = self._conv(du0, w["RDAB.conv_du_re.2_s2d"], pad=1, act=K.ACT_RELU, exact=True)     # [GB, H/2+1, W/2+1, 64]
            part, n = K.chan_sum_partial(t)
            count = t.shape[1] * t.shape[2]
        vmax = K.vec_mlp(part, n, count, raw["RDAB.conv_du_re2.0.weight"],
                         raw["RDAB.conv_du_re2.0.bias"], 64, K.ACT_RELU)
        # fp16x2 (default): the probabilities-times-values product of the three attentions on single-fp16 operands (modes 20-22:
        # error <= 2^-11 max|v|, measured ~1e-5 |v|; the scores keep their three split-fp16 passes); fp32-grade modes: all three passes
        am = 20 if self.precision == "fp16x2" and self.attn_pv_single else 0
        wW, bW = raw["RDAB.directW1_conv.weight"], raw["RDAB.directW1_conv.bias"]
        fused_prep = self.rdab_fused and self.precision != "f32" and K.rdab_prep_fused_ok(x, w["RDAB.input_conv"])
        if rms_planes is not None and not (fused_prep and rms_planes[1] % B == 0):
            raise ValueError("_rdab: rms_planes needs the fused mask kernel and each noise's images inside one block of planes")
        if fused_prep:
            # input_conv inside the mask kernel: its 128-channel result is never written.  Modes 20-22 round every V once to fp16
            # while staging, so the V operands of the column and window attentions (the row attention's output, the window V) are
            # stored that way: same bits.  vrow stays fp32: the row form measured slower on an fp16 V
            vdt = torch.float16 if am == 20 else torch.float32
            sq, vrow, qwin = (K.empty_act(GB, H, W, 64, x.device) for _ in range(3))
            vwin = torch.empty((GB, H, W, 64), dtype=vdt, device=x.device)
            for g, noise in enumerate(noises):
                sl = slice(g * B, (g + 1) * B)
                plane = None
                if rms_planes is not None:      # this noise's planes: images g B .. g B + B - 1 of the addressing, inside one block
                    view, Bi, s_b, s_g = rms_planes
                    off = (g * B % Bi) * s_b + (g * B // Bi) * s_g
                    first = view.as_strided((1,), (1,), view.storage_offset() + off)      # (no copy: an address in the storage)
                    plane = (first, B, s_b, 0, w["rms_chunk_input_conv"])
                xs = x.sub(sl.start, B) if isinstance(x, K.ImageMap) else x[sl]      # (a mapped stack: this noise's images as a map of their own)
                K.rdab_prep_fused(xs, w["RDAB.input_conv"], vmax[sl], noise, wW, bW, v_f16=(False, am == 20),
                                  outs=(sq[sl], vrow[sl], qwin[sl], vwin[sl]), plane=plane)
        else:
            if isinstance(x, K.ImageMap):
                raise ValueError("_rdab: a mapped x needs the fused mask kernel (_stack_inplace decides before the first launch)")
            vdt = torch.float32
            xq = self._conv(x, w["RDAB.input_conv"])
            vwin = xq[..., 64:128]
            sq, vrow, qwin = (K.empty_act(GB, H, W, 64, x.device) for _ in range(3))
            for g, noise in enumerate(noises):
                sl = slice(g * B, (g + 1) * B)
                outs = (sq[sl], vrow[sl], qwin[sl])
                if isinstance(noise, tuple):  # ("rng", seed, draw, capture): draw the uniforms inside the kernel (default path)
                    _, seed, draw, capture = noise
                    K.rdab_prep_rng(xq[sl], vmax[sl], seed, draw, wW, bW, noise_out=capture, outs=outs)
                else:
                    K.rdab_prep(xq[sl], vmax[sl], noise, wW, bW, outs=outs)
        cat = K.empty_act(GB, H, W, 128, x.device)
        rowo = K.seq_attn(sq, vrow, am, out_dtype=vdt)
        qc = K.colconv9(sq, raw["RDAB.directH1_conv.weight"], raw["RDAB.directH1_conv.bias"])
        K.seq_attn(qc, rowo, am + 1, out=cat[..., 0:64])
        K.seq_attn(qwin, vwin, am + 2, out=cat[..., 64:128])
        if rms_planes is not None:      # the residual is x + conv_expand_rms(plane): the stencil's part goes through the product
            return self._conv(cat, w["RDAB.fuse"], res1=x, plane=(*rms_planes, w["rms_chunk"]))
        return self._conv(cat, w["RDAB.fuse"], res1=x)

    def _align(self, w, xc, extra, pred, mvs, mv_bstride, out, frames=None, ufs_planes=None):
        """DualAttAlignment (arch.py:3455-3496) on a group of neighbours: xc / extra / pred / out are [G*B,H,W,64] (xc = the
        centre frame's features repeated per neighbour), mvs one motion field view per neighbour.  frames (shared compensation):
        (bank, idx, mvs1, slot0) -- `extra` is None and image g*B + b is bank[idx[g*B + b]], warped in place by one launch with
        the flow of window b at slot slot0 + g of mvs1 [B,7,2,H,W].  ufs_planes (model.inline_ufs, with pred = None): the plane
        addressing (view, Bi, s_b, s_g) of the partition maps whose conv_expand_ufs stencil pred is; it stays inside the products."""
        raw = w["raw"]
        a = "MV_deform_align."
        GB, H, W, _ = xc.shape
        B = GB // len(mvs)
        warped = K.empty_act(GB, H, W, NF, xc.device)
        if frames is not None:
            bank, idx, mvs1, slot0 = frames
            K.flow_warp_frames(bank, idx, mvs1, mv_bstride, slot0, len(mvs), B, out=warped)
        for g, mv in enumerate(mvs if frames is None else ()):
            K.flow_warp(extra[g * B:(g + 1) * B], mv, mv_bstride, out=warped[g * B:(g + 1) * B])
        fused = self.precision != "f32" and self.align_stats
        fold_args = (raw[a + "temperature"], raw[a + "conv_du.0.weight"], raw[a + "conv_du.0.bias"], raw[a + "conv_du.2.weight"],
                     raw[a + "conv_du.2.bias"], raw[a + "project_out.weight"], raw[a + "fusion_out.0.weight"])
        if ufs_planes is not None:
            # pred has two readers, both products over the pixel's channels: each takes it as one more k-step of ten numbers per pixel
            # built from the partition map (the statistics pass with fusion_out.0's second half composed in, the folded convolution
            # with the per-image M2), and the channel sums of pred come from the map's tap sums
            gp, sw, sp, ng = K.align_stats(warped, None, xc, w[a + "fusion_out.0"], K.ACT_RELU, 16,
                                           plane=(*ufs_planes, w["ufs_chunk_fusion_out"], w["ufs_chunk"]))
            fold128, tables = K.align_fold_plane(gp, ng, sw, sp, ng, H * W, *fold_args, w["ufs_chunk"])
            o, part, n = self._conv([warped, xc], fold128, act=K.ACT_RELU, chan_sum_out=True, plane=(*ufs_planes, tables, 64 * 16))
        elif fused:
            # kf = relu(fusion_out.0([warped, pred])) has one consumer, the Gram: one pass over warped, pred, xc forms it tile by tile
            # and leaves the Gram and the two channel sums; kf never reaches memory
            gp, sw, sp, ng = K.align_stats(warped, pred, xc, w[a + "fusion_out.0"], K.ACT_RELU, 16)
            fold = K.align_fold(gp, ng, sw, sp, ng, H * W, *fold_args)
            o, part, n = self._conv([warped, pred, xc], fold, act=K.ACT_RELU, chan_sum_out=True)     # CALayer's pool from the epilogue
        else:
            kf = self._conv([warped, pred], w[a + "fusion_out.0"], act=K.ACT_RELU)
            gp, ng = K.gram_partial(xc, kf, 16)
            sw, ns = K.chan_sum_partial(warped)
            sp, _ = K.chan_sum_partial(pred)
            fold = K.align_fold(gp, ng, sw, sp, ns, H * W, *fold_args)
            o = self._conv([warped, pred, xc], fold, act=K.ACT_RELU)
            part, n = K.chan_sum_partial(o)
        gate = K.vec_mlp(part, n, H * W, raw[a + "CALayer.conv_du.0.weight"], raw[a + "CALayer.conv_du.0.bias"], 64,
                         K.ACT_RELU, raw[a + "CALayer.conv_du.2.weight"], raw[a + "CALayer.conv_du.2.bias"], 64,
                         K.ACT_SIGMOID)
        rb = [w[a + n] for n in ("ResidualBlock.conv1", "ResidualBlock.conv2", "ResidualBlock1.conv1", "ResidualBlock1.conv2")]
        fast16 = self.precision == "fp16x2" and H % 2 == 0 and all(c.wh is not None for c in rb)
        if fast16:
            o, o16 = K.scale_channels(o, gate, want_cp16=True)
        else:
            o = K.scale_channels(o, gate)
        if fast16:
            # the two ResidualBlock_noBN (arch.py:261-262) on the Block_ kernels: conv1 + ReLU weights-stationary (fp16
            # chunk-planar in and out), conv2 + residual on its residual form (fp32 pixel-major out); single-pass fp16 MFMA like the
            # convolutions inside Block_ (no measurable change of the forward's error: 2.80e-4 with and without)
            n16 = torch.empty_like(o16)
            o = K.conv3x3_ws_res(K.conv3x3_ws(o16, rb[0], act=K.ACT_RELU), rb[1], res1=o, out2_cp16=n16)
            return K.conv3x3_ws_res(K.conv3x3_ws(n16, rb[2], act=K.ACT_RELU), rb[3], res1=o, res2=xc, out=out)
        r = self._conv(o, rb[0], pad=1, act=K.ACT_RELU)
        o = self._conv(r, rb[1], pad=1, res1=o)
        r = self._conv(o, rb[2], pad=1, act=K.ACT_RELU)
        return self._conv(r, rb[3], pad=1, res1=o, res2=xc, out=out)

    def _block(self, w, p, x, x16=None, want16=False, want_hl=False):
        """Block_ (arch.py:378-406): x + body(x) + up(body(down(x))) + down(body(up(x))).
        The 1x1 convs commute with the (linear) resampling, so they run on the smaller side of it.
        x16: optional fp16 chunk-planar copy of x; want16: also return such a copy of the result (fp16x2 mode)."""
        b0, b2, dn, up = w[p + "body.0"], w[p + "body.2"], w[p + "down.0"], w[p + "up.0"]
        # fp16x2 mode: the 256-channel body intermediate is stored as fp16 (rounding it does not move the forward's
        # error: 2.76e-4 with and without, oracle emulation) -> half the HBM bytes between the two convs, body.2 becomes
        # a single-pass fp16 MFMA whose staging is a plain copy
        t16 = self.precision == "fp16x2"
        if t16 and x.shape[1] % 4 == 0 and b0.wh is not None:
            # body[0] on the weights-stationary kernel, body[2] / the composed stride-2 convolution on the LDS-DMA ring
            # kernel; the 64- and 256-channel tensors between them are fp16 chunk-planar [B,C/16,H,W,16].  Same
            # arithmetic as the single-pass fp16 mode of the tiled kernel: fp16 operands, fp32 accumulation
            # body[0]: the row-streaming Winograd F(2,3) kernel (2/3 of the direct product's MFMAs) unless CDFO_WINO=0
            c1 = lambda src, **kw: K.conv3x3_body0(src, b0, act=K.ACT_LRELU, **kw)
            # sources of the x2 and x1/2 branches (and, for a group's first block, of the 1x branch), one read of x.  up2: the x2 branch's
            # source stays at the block's resolution (up.0(x), a quarter of the bytes) and the Winograd kernel interpolates it on the fly
            up2 = (b0.ww is not None and K.wino_up2_enabled() and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0
                   and x.shape[1] * x.shape[2] * 8 * b0.Cout < (1 << 31))
            if x16 is None:
                u16, d16, x16 = K.block_prologue(x, w[p + "pro"], want_x16=True, lowres_up=up2)
            else:
                u16, d16 = K.block_prologue(x, w[p + "pro"], lowres_up=up2)
            hs = up2 and self.wino_halfsplit
            c2 = (lambda src: K.conv3x3_wino_up2(src, b0, act=K.ACT_LRELU, halfsplit=hs)) if up2 else (lambda src: c1(src, s2d=True))
            # The x1/2 branch (two launches on a quarter of the pixels: 72 tiles per clip at 272x480, a fraction of the GPU for one
            # or two clips and a ragged last round for eight) runs on a side stream beside the x1 and x2 branches; the last
            # convolution joins the three.
            side = self._trunk_side(x.device) if self.trunk_side_stream else None
            if side is not None:
                main = torch.cuda.current_stream(x.device)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    d = K.conv_ring(c1(d16), w[p + "body.2_up"])      # = up.0(body.2(.)) of the x1/2 branch
                out = K.conv_ring(c1(x16), b2, res1=x)
                t = c2(u16)
                main.wait_stream(side)
                d.record_stream(main)
            else:
                out = K.conv_ring(c1(x16), b2, res1=x)
                d = K.conv_ring(c1(d16), w[p + "body.2_up"])      # = up.0(body.2(.)) of the x1/2 branch
                t = c2(u16)
            # want16: the next block's fp16 source; want_hl (a group's last block): fp16 hi | lo planes for the group convolution
            y16 = torch.empty_like(x16) if want16 else None
            if want_hl:
                y16 = torch.empty((x16.shape[0], 8) + tuple(x16.shape[2:]), dtype=torch.float16, device=x16.device)
            # the x1/2 branch (bilinear x2 of d) is added by the last convolution's epilogue
            y = K.conv_ring(t, w[p + "down_fused"], res1=out, res_up2=d, out2_cp16=y16, out2_hl=want_hl, src_halfsplit=hs)
            return (y, y16) if (want16 or want_hl) else y
        out = self._conv(self._conv(x, b0, pad=1, act=K.ACT_LRELU, out_f16=t16, inner=True), b2, pad=1, res1=x)
        # half-resolution branch
        d = self._conv(K.resample2(x, up=False), dn)
        d = self._conv(self._conv(d, b0, pad=1, act=K.ACT_LRELU, out_f16=t16, inner=True), b2, pad=1)
        K.resample2(self._conv(d, up), up=True, out=out, accumulate=True)
        # double-resolution branch: conv1 writes its 256 channels space-to-depth; conv2 + 2x2 mean + down.0 are one
        # composed sparse-tap convolution at the block's own resolution (see _weights)
        u = K.resample2(self._conv(x, up), up=True, out_f16=t16)     # fp16 in fp16x2 mode: conv1 stages it by plain copy
        t = self._conv(u, b0, pad=1, act=K.ACT_LRELU, s2d=True, out_f16=t16, inner=True)
        y = self._conv(t, w[p + "down_fused"], pad=1, res1=out)
        return (y, None) if want16 else y

    def _side(self, device, count):
        """`count` side streams of `device`, created once per (device, count): the neighbour groups ask for two or more, the
        trunk and the feature extractor for one of their own."""
        cache = self.__dict__.setdefault("_side_streams", {})
        if (device, count) not in cache:
            cache[(device, count)] = [torch.cuda.Stream(device) for _ in range(count)]
        return cache[(device, count)]

    def _trunk_side(self, device):
        return self._side(device, 1)[0]

    def _trunk(self, w, fused):
        y = fused
        for g in range(7):
            r, r16 = y, None
            fast = self.precision == "fp16x2" and y.shape[1] % 4 == 0 and w[f"recon_trunk.body.{g}.body.0.body.0"].wh is not None
            for b in range(3):      # blocks 0 and 1 hand their successor an fp16 chunk-planar copy of the result, block 2 hands
                if b < 2:           # the group convolution fp16 hi | lo planes of it
                    r, r16 = self._block(w, f"recon_trunk.body.{g}.body.{b}.", r, r16, want16=True)
                elif fast:
                    r, r16 = self._block(w, f"recon_trunk.body.{g}.body.{b}.", r, r16, want_hl=True)
                else:
                    r, r16 = self._block(w, f"recon_trunk.body.{g}.body.{b}.", r, r16), None
            if fast:    # SCGroup_.conv (arch.py:435) on the ring kernel: 8 K chunks (hi | lo) against the tiled kernel's restaging
                y = K.conv_ring(r16, w[f"recon_trunk.body.{g}.conv_hl2"], res1=y, res2=fused if g == 6 else None)
            else:
                y = self._conv(r, w[f"recon_trunk.body.{g}.conv"], pad=1, res1=y, res2=fused if g == 6 else None)
        return y

    # -- arithmetic mode ---------------------------------------------------------------------------------------------
    _tls = threading.local()

    @property
    def precision(self) -> str:
        ov = getattr(CVSR_V8._tls, "override", None)
        if ov is not None and ov[0] is self:
            return ov[1]
        return self._precision

    @precision.setter
    def precision(self, value: str):
        if value not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}, got {value!r}")
        self._precision = value

    def _resolve_noise(self, x, gumbel_uniform):
        """The noise source of one inference forward and, if it is the in-kernel generator, its Philox key: an integer launch
        argument for an eager forward; the DEVICE word of refresh_noise_key() for a forward that is being captured into a HIP
        graph (a launch argument would freeze into the graph and every replay would draw the same uniforms; the reference draws
        per call, arch.py:2169).  Shared by forward() and forward_front()."""
        noise = gumbel_uniform if gumbel_uniform is not None else self.gumbel_uniform
        if noise is None:
            if torch.cuda.is_current_stream_capturing():
                if self._noise_key is None or self._noise_key.device != x.device:
                    raise RuntimeError("CVSR_V8 (HIP): call model.refresh_noise_key(device) before capturing a forward "
                                       "that draws its own Gumbel noise")
                self._noise_seed = self._noise_key
            else:
                self._noise_seed = K.next_noise_seed(x.device)
        return noise

    # -- forward ---------------------------------------------------------------------------------------------------
    def forward(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea=None, gumbel_uniform=None):
        self._check("forward", x, grad_ok=True, capture_ok=True)
        with K.on_device(x):     # the operands' device becomes the current one: streams, per-device caches of the library
            training = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            if training and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("CVSR_V8 (HIP): the autograd path cannot be captured into a HIP graph (its mask kernel takes the "
                                   "Philox key as a launch argument); capture inference forwards under torch.no_grad()")
            noise = self._resolve_noise(x, gumbel_uniform)
            if training:
                # training call (train_LD_37.py:376-381): the operator graph under autograd, HIP kernels in both directions
                # (cdfo_amd/cvsr_v8_train.py; convolution arithmetic = autograd.CONV_PREC); the fused schedule below is forward-only
                if pre_L1_fea is not None:
                    raise NotImplementedError("CVSR_V8 (HIP): the cached-feature path is an inference path; training uses fresh clips")
                for prm in self.parameters():
                    if not prm.is_cuda or prm.dtype != torch.float32:
                        raise NotImplementedError("CVSR_V8 (HIP): fp32 parameters on the GPU expected")
                from .cvsr_v8_train import forward_train
                return forward_train(self, x, mvs0, mvs1, pms, rms, ufs, noise)
            return self._guarded(x.device, lambda: self._forward(x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea, noise))

    def _guarded(self, device, run, rerun=None):
        """``run()`` -- one inference forward of any route -- under the fp16 range guard.  The fp16x2 mode keeps the trunk's
        tensors (and the alignment's residual blocks) in fp16.  Outside fp16's comfortable range -- max |trunk input| not in
        [2^-6, 2^11], or a NaN / infinity in the trunk's input or output (what an overflowed fp16 store turns into) -- the forward
        is repeated in the split-bf16 mode (fp32 exponent range, fp32-grade products), through ``rerun()`` if the route has to
        rebuild operands first, with the Philox key of the rejected forward.  Two probe kernels fill a zeroed 4-int probe (trunk
        input: slots 0-1, trunk output: 2-3) that `_fuse` and `_back` find in ``self._probe``; it is copied to pinned host memory
        behind the last kernel and settled before the call returns: what an eager forward returns is final."""
        if not (self.precision == "fp16x2" and self.range_guard):
            return run()
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            # model.capture() (graph.py): the probe is a graph node -- zeroed, filled by the two probe kernels, copied to pinned
            # host memory behind the last kernel; CapturedForward.replay() reads it and repeats a rejected forward eagerly in bf16x3
            # (through _range_fallback)
            probe = self.__dict__.get("_graph_probe")
            if probe is None:
                raise RuntimeError("CVSR_V8 (HIP): the fp16 range guard reads probes back and cannot be captured by hand; use "
                                   "model.capture(), whose graph carries the two probes and whose replay() reads them back")
            probe.zero_()
        else:
            probe = torch.zeros(4, dtype=torch.int32, device=device)
        self._probe = probe
        try:
            res = run()
        finally:
            self._probe = None
        if capturing or not self._settle_range(probe):
            return res
        return self._recompute_bf16x3(rerun or run, self._noise_seed)

    def _settle_range(self, probe) -> bool:
        """Read a guarded forward's probe words back behind its last kernel (one host sync), set ``last_range``; True = the
        forward has to be repeated in bf16x3."""
        pinned = self.__dict__.setdefault("_guard_pinned", {})
        if probe.device not in pinned:
            pinned[probe.device] = torch.zeros(4, dtype=torch.int32).pin_memory()
        host = pinned[probe.device]
        host.copy_(probe, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        self.last_range = self._range_verdict(host)
        return self.last_range["fallback"]

    FP16_WINDOW = (2.0 ** -6, 2.0 ** 11)

    def _range_verdict(self, host4) -> dict:
        """The fp16 range guard's decision from its four probe words (host int32; eager forward and CapturedForward alike):
        [0] bits of max |trunk input|, [1] non-finite trunk input, [3] non-finite trunk output.  ``FP16_WINDOW`` is read from the
        instance, so a per-model override takes effect."""
        amax = host4[0:1].view(torch.float32).item()
        nonfinite = bool(host4[1].item()) or bool(host4[3].item())
        lo, hi = self.FP16_WINDOW
        return {"trunk_input_amax": amax, "nonfinite": nonfinite, "fallback": nonfinite or not (amax == 0.0 or lo <= amax <= hi)}

    def _range_fallback(self, args, out_ref, l1_ref):
        """Recompute a forward whose activations left fp16's range in the split-bf16 mode; with out_ref / l1_ref (a captured
        forward's output buffers) the results are written into those tensors."""
        x, mvs0, mvs1, pms, rms, ufs, pre, noise, seed = args
        res = self._recompute_bf16x3(lambda: self._forward(x, mvs0, mvs1, pms, rms, ufs, pre, noise), seed)
        if out_ref is not None:
            out_ref.copy_(res[0])
        if l1_ref is not None:
            l1_ref.copy_(res[1])
        return res

    def _recompute_bf16x3(self, run, seed):
        """``run()`` once more in the split-bf16 mode with the Philox key `seed` of the rejected forward; warns once per model."""
        lr = self.last_range
        if not self._warned_range:
            import warnings
            warnings.warn(f"CVSR_V8 (HIP): activations leave the fp16 range (max |trunk input| = {lr['trunk_input_amax']:.3g}, non-finite "
                          f"result: {lr['nonfinite']}); this forward and others like it are recomputed with "
                          "precision='bf16x3'.  Set model.precision = 'bf16x3' to avoid the repeated work.")
            self._warned_range = True
        # the retry's mode is an override visible to THIS thread only: another thread / stream sharing the module keeps
        # reading the attribute the user set
        CVSR_V8._tls.override = (self, "bf16x3")
        keep_seed, self._noise_seed = self._noise_seed, seed
        try:
            with torch.no_grad():
                return run()
        finally:
            CVSR_V8._tls.override = None
            self._noise_seed = keep_seed

    # -- the forward in two halves (inference only, no range guard: the caller owns the schedule) -------------------
    def forward_front(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea=None, gumbel_uniform=None):
        """Feature extraction + neighbour pipelines + temporal fusion on the CURRENT stream.  Returns (state, L1_fea):
        `state` goes to `forward_back`, `L1_fea` is what `forward` returns as its second output (the next call's
        `pre_L1_fea`).  A caller may run `forward_back(state)` on another stream (after making it wait for this one) while the
        next frame's `forward_front` is already running here: cdfo_amd.streaming.StreamingSR.run_pipelined does."""
        self._check("forward_front", x, capture_ok=True)
        with K.on_device(x):
            noise = self._resolve_noise(x, gumbel_uniform)
            fused, L1, xf = self._front(x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea, noise)
        return (fused, xf), L1.permute(0, 3, 1, 2)

    def forward_back(self, state):
        """Reconstruction trunk + upsampling + skip of a `forward_front` state, on the CURRENT stream."""
        fused, xf = state
        with K.on_device(fused):
            return self._back(fused, xf)

    # -- one sequence, K centre frames per call, features supplied by the caller (inference only) ----------------------
    def _check(self, what: str, t: torch.Tensor, size=None, clip=False, grad_ok=False, capture_ok=False):
        """The refusals the entry points share.  t: an operand of `what`, which has to live on the GPU; grad_ok / capture_ok: the
        call also serves autograd / may be captured into a HIP graph; clip: t is the input clip x [B,7,1,H,W]; size: (H, W) of
        the frames (read from the clip if t is one)."""
        if not t.is_cuda:
            raise NotImplementedError("CVSR_V8 (HIP): CPU tensors are not supported; there is no CPU fallback")
        if not grad_ok and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(f"CVSR_V8 (HIP): {what} is an inference call -- wrap it in torch.no_grad()")
        if not capture_ok and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError(f"CVSR_V8 (HIP): {what} is not captured into HIP graphs")
        if clip:
            if t.dim() != 5 or t.shape[1] != NFRAMES or t.shape[2] != 1:
                raise ValueError(f"expected x of shape [B,7,1,H,W], got {tuple(t.shape)}")
            size = t.shape[3:]
        if size is not None:
            H, W = size
            if H % 8 or W % 8:
                raise ValueError(f"H and W must be multiples of 8 (window attention, arch.py:2147,2235); got {H}x{W}")

    def extract_features(self, frames, pms):
        """Step 1 of the forward per frame (arch.py:4416-4427 is per image): frames, pms [F,1,H,W] -> features [F,H,W,64],
        pixel-major.  What any window of a sequence uses for frame t is extract_features(lr[t], pms[max(1, t)])."""
        self._check("extract_features", frames, size=frames.shape[2:])
        F, C, H, W = frames.shape
        if C != 1 or tuple(pms.shape) != (F, 1, H, W):
            raise ValueError(f"expected frames and pms of shape [F,1,H,W], got {tuple(frames.shape)} and {tuple(pms.shape)}")
        with K.on_device(frames):
            w = self._weights()
            raw = w["raw"]
            self.H, self.W = H, W
            self.frames_extracted += F
            f = K.stem_conv(frames.contiguous().float(), H * W, F, H, W, raw["conv_first.weight"], raw["conv_first.bias"], K.ACT_LRELU)
            return self._feature_extraction(w, f, pms.contiguous().float(), H * W, F)

    def forward_windows(self, Lf, x, mvs0, mvs1, rms, ufs, gumbel_uniform=None):
        """K windows of one sequence from extracted features: Lf [7,K,H,W,64] the frame-major window stack (slot n of window k
        = the features of the frame that window has there), x [K,7,1,H,W] (only the centre frames are read: the skip
        connection), mvs0 / mvs1 / rms / ufs / gumbel_uniform as for ``forward`` at B = K (mvs0 is unused there too).  Returns
        out [K,1,4H,4W].  Steps 2-5 of ``forward`` on the same kernels; the clip-major feature tensor, its shift copy and its
        transpose never exist.  The fp16 range guard is that of ``forward``: settled before the call returns, a rejected call
        is repeated in bf16x3 from the same Lf."""
        self._check("forward_windows", x, clip=True)
        Kw, N, C, H, W = x.shape
        if tuple(Lf.shape) != (N, Kw, H, W, NF):
            raise ValueError(f"expected x [K,7,1,H,W] and Lf [7,K,H,W,64], got {tuple(x.shape)} and {tuple(Lf.shape)}")
        if Lf.dtype != torch.float32 or not Lf.is_contiguous():
            raise ValueError("Lf must be a dense fp32 tensor")
        with K.on_device(x):
            noise = self._resolve_noise(x, gumbel_uniform)
            x = x.contiguous().float()
            mvs1 = mvs1.contiguous().float()
            self.H, self.W = H, W

            def run():
                fused = self._fuse_windows(self._weights(), Lf, x, mvs1, rms, ufs, noise)
                return self._back(fused, x)

            return self._guarded(x.device, run)

    def resolve_noise_key(self, device, key: Optional[int] = None) -> int:
        """The Philox key that compensate_features draws with: `key`, or a fresh one taken from torch's default generator of
        `device` as a forward does (``torch.manual_seed`` reproduces it).  A caller that shares one key over several calls (one
        sequence) passes the returned value back in before each of them."""
        self._noise_seed = K.next_noise_seed(torch.device(device)) if key is None else int(key)
        return self._noise_seed

    def compensate_features(self, fea, rms, gumbel_uniform=None, draws=None):
        """The per-frame half of a neighbour pipeline (arch.py:4443-4454), once per FRAME instead of once per (window, slot):
        fea [F,H,W,64] pixel-major fp32 (extract_features), rms [F,1,H,W] in [0,1] -> comp [F,H,W,64] =
        conv_expand_fea_r([fea, RDAB(fea + conv_expand_rms(rms))]), the `fea_i` that `_neighbour_group` hands to the alignment,
        on the same kernels.  What any window of a sequence uses for frame t is compensate_features(fea[t], rms[max(1, t)]).
        Noise: gumbel_uniform = F tensors [1,64,H,W] (one draw per FRAME), else the in-kernel Philox generator, one mask launch
        per frame with image index 0, draw = draws[f] (default f) and the key of resolve_noise_key(): a frame's uniforms depend on
        (key, draws[f]) only, not on which other frames share the call.  Deviation from the reference, which draws per (forward,
        slot): see StreamingSR.run_chunked(share_compensation=True)."""
        self._check("compensate_features", fea, size=fea.shape[1:3])
        if fea.dim() != 4 or fea.shape[3] != NF or fea.dtype != torch.float32 or not fea.is_contiguous():
            raise ValueError(f"compensate_features: fea must be a dense fp32 [F,H,W,64] tensor, got {fea.dtype} {tuple(fea.shape)}")
        F, H, W, _ = fea.shape
        if tuple(rms.shape) != (F, 1, H, W):
            raise ValueError(f"compensate_features: rms must be [F,1,H,W] = {(F, 1, H, W)}, got {tuple(rms.shape)}")
        noise = gumbel_uniform if gumbel_uniform is not None else self.gumbel_uniform
        draws = list(range(F)) if draws is None else [int(d) for d in draws]
        if len(draws) != F or (noise is not None and len(noise) != F):
            raise ValueError(f"compensate_features: one noise tensor / one draw index per frame expected (F = {F})")
        for f, u in enumerate(noise or ()):
            if tuple(u.shape) != (1, NF, H, W):
                raise ValueError(f"compensate_features: noise of frame {f} must be [1,64,{H},{W}], got {tuple(u.shape)}")
        with K.on_device(fea):
            w = self._weights()
            self.H, self.W = H, W
            self.frames_compensated += F
            # one stem launch for all frames; one image per "neighbour": the mask kernel runs per frame
            return self._compensate(w, fea, [(rms.contiguous().float(), H * W, slice(0, F))], draws, noise)[0]

    def forward_windows_shared(self, Lc, comp_bank, comp_idx, x, mvs1, ufs, recompensate=None):
        """K windows of one sequence whose neighbours' compensation is banked per frame: Lc [K,H,W,64] the centres' features,
        comp_bank [cap,H,W,64] the output of compensate_features per bank slot, comp_idx a device int32 [6,K] (slot-major over
        the neighbour slots 0, 1, 2, 4, 5, 6): the bank slot of each window's neighbour; x [K,7,1,H,W] (centre frames: the skip
        connection), mvs1 [K,7,2,H,W], ufs [K,7,1,H,W].  Returns out [K,1,4H,4W].  Steps 2b-5 of ``forward``: the partition-map
        stem per slot, the alignment of two groups of three slots on the two side streams (each reads the bank in place through
        cdfo_flow_warp_frames), temporal fusion, trunk, up-sampler.  The fp16 range guard is that of ``forward_windows``, settled
        before the call returns; a rejected call is repeated in bf16x3 -- from `recompensate()` -> (comp_bank, comp_idx) if given
        (called in the bf16x3 mode: the caller recomputes the compensation its windows use), else from the same bank."""
        self._check("forward_windows_shared", x, clip=True)
        Kw, N, C, H, W = x.shape
        if tuple(Lc.shape) != (Kw, H, W, NF) or comp_bank.dim() != 4 or tuple(comp_bank.shape[1:]) != (H, W, NF):
            raise ValueError(f"expected x [K,7,1,H,W], Lc [K,H,W,64] and comp_bank [cap,H,W,64], got {tuple(x.shape)}, {tuple(Lc.shape)} "
                             f"and {tuple(comp_bank.shape)}")
        for name, t in (("Lc", Lc), ("comp_bank", comp_bank)):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name} must be a dense fp32 tensor")
        if comp_idx.dtype != torch.int32 or comp_idx.device != x.device or comp_idx.numel() != (N - 1) * Kw or not comp_idx.is_contiguous():
            raise ValueError("comp_idx must be a dense int32 [6,K] tensor on the operands' device")
        if tuple(mvs1.shape) != (Kw, N, 2, H, W) or ufs.numel() != Kw * N * H * W:
            raise ValueError(f"expected mvs1 [K,7,2,H,W] and ufs [K,7,1,H,W], got {tuple(mvs1.shape)} and {tuple(ufs.shape)}")
        with K.on_device(x):
            x = x.contiguous().float()
            mvs1 = mvs1.contiguous().float()
            ufs = ufs.contiguous().float().view(Kw, 1, N, H, W)
            self.H, self.W = H, W
            state = [comp_bank, comp_idx.view(-1)]

            def run():
                fused = self._fuse_windows_shared(self._weights(), Lc, state[0], state[1], x, mvs1, ufs)
                return self._back(fused, x)

            def rerun():
                if recompensate is not None:
                    bank2, idx2 = recompensate()
                    state[0], state[1] = bank2, idx2.view(-1)
                return run()

            return self._guarded(x.device, run, rerun)

    def capture(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea=None, gumbel_uniform=None, check_range: bool = True):
        """Capture one inference forward at these operands' shapes into a HIP graph (opt-in; fixed shapes).  Returns a
        ``cdfo_amd.graph.CapturedForward``: ``cap(x, mvs0, ...)`` copies the operands into the graph's input buffers, refreshes
        the device-side Philox key (fresh Gumbel noise per replay, arch.py:2169) and replays; it returns graph-owned
        ``(out, L1_fea)`` buffers that the next replay overwrites.  Same launches as the eager path: bit-identical outputs.  In the
        fp16x2 mode with the range guard on, the graph carries the guard's two probes and ``replay()`` reads them back (a rejected
        forward is repeated eagerly in bf16x3 into the graph's output buffers), see graph.py."""
        from .graph import CapturedForward
        return CapturedForward(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea, gumbel_uniform, check_range)

    def capture_pipelined(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea=None, gumbel_uniform=None, check_range: bool = True):
        """Two alternating captured forwards (``cdfo_amd.graph.PipelinedForward``): ``submit(...)`` launches a forward and reads the
        PREVIOUS forward's range-guard probes afterwards, so the GPU never waits for a graph launch between forwards of a stream of
        batches.  Results of a ``submit`` are final once the next ``submit`` / ``drain()`` has returned."""
        from .graph import PipelinedForward
        return PipelinedForward(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea, gumbel_uniform, check_range)

    def refresh_noise_key(self, device=None) -> int:
        """Write a fresh Philox key (advancing torch's default generator like an eager forward does) into the device word that
        CAPTURED forwards read: call before capturing and before every replay of a HIP graph of this model, so that each
        replayed forward draws its own Gumbel noise like the reference does per call (arch.py:2169)."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        seed = K.next_noise_seed(dev)
        if self._noise_key is None or self._noise_key.device != dev:
            self._noise_key = torch.empty(1, dtype=torch.int64, device=dev)
        self._noise_key.fill_(seed)
        return seed

    def _forward(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea=None, gumbel_uniform=None):
        fused, L1, xf = self._front(x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea, gumbel_uniform)
        return self._back(fused, xf, L1), L1.permute(0, 3, 1, 2)

    def _front(self, x, mvs0, mvs1, pms, rms, ufs, pre_L1_fea=None, gumbel_uniform=None):
        """Steps 1-3 of the forward: feature extraction, the six neighbour pipelines, temporal fusion.  Returns (fused
        [B,H,W,64], L1 [B*7,H,W,64] clip-major, x as the contiguous fp32 tensor the skip connection reads).  `_back` is the
        rest; the split exists for callers that run the two halves of consecutive frames beside each other
        (StreamingSR.run_pipelined)."""
        self._check("forward", x, clip=True, grad_ok=True, capture_ok=True)
        B, N, C, H, W = x.shape
        w = self._weights()
        raw = w["raw"]
        self.H, self.W = H, W
        ctr = self.center
        x = x.contiguous().float()
        pms = pms.contiguous().float()
        mvs1 = mvs1.contiguous().float()
        P = H * W

        nstr = int(getattr(self, "neighbour_streams", 0)) or 2       # see step 2
        gsz = int(getattr(self, "neighbour_group", 0)) or ctr
        deferred_new = None

        # 1. feature extraction (arch.py:4416-4427)
        self.frames_extracted += B * N if pre_L1_fea is None else B
        if pre_L1_fea is None:
            f = K.stem_conv(x, P, B * N, H, W, raw["conv_first.weight"], raw["conv_first.bias"], K.ACT_LRELU)
            L1 = self._feature_extraction(w, f, pms, P, B * N)           # [B*7,H,W,64], clip-major
        else:
            last_x, last_p = x[:, -1].contiguous(), pms[:, -1].contiguous()
            pre = self._as_pixel_major(pre_L1_fea, B * N, H, W)
            L1 = torch.empty_like(pre)
            L1v, prev = L1.view(B, N, H, W, NF), pre.view(B, N, H, W, NF)
            L1v[:, :-1].copy_(prev[:, 1:])                               # device-side shift of the feature cache

            def new_frame_features():
                f = K.stem_conv(last_x, P, B, H, W, raw["conv_first.weight"], raw["conv_first.bias"], K.ACT_LRELU)
                L1v[:, -1].copy_(self._feature_extraction(w, f, last_p, P, B))       # [B,H,W,64]

            # One streamed sequence (B = 1, test_LD_22_FPS.py:155-192): L1 is already frame-major, and the neighbour group of
            # frames 0-2 reads cached features only.  It is forked onto its side stream BEFORE the new frame's feature
            # extraction is enqueued -- ~35 launches on ONE frame, which leave most of the GPU idle -- and runs beside it;
            # the group that holds the new frame follows the extraction on the caller's stream.
            if B == 1 and nstr > 1 and gsz == ctr and self.overlap_new_frame:
                deferred_new = new_frame_features
            else:
                new_frame_features()
        if self._stack_inplace(w, B, H, W):
            Lf = _FeatureStack(L1, B, H, W, P * NF, N * P * NF)                # the stack as it lies: clip-major
        else:
            Lf = (K.swap_outer(L1, B, N) if B > 1 else L1).view(N, B, H, W, NF)   # frame-major views for the loop
        return self._fuse_windows(w, Lf, x, mvs1, rms, ufs, gumbel_uniform, deferred_new), L1, x

    def _stack_inplace(self, w, B, H, W) -> bool:
        """The one predicate of the in-place neighbour phase, evaluated before its first launch; it decides for the whole forward.  True:
        the seven readers of the feature stack -- the mask kernel's x, RDAB.fuse's residual, source 0 of conv_expand_fea_r, the
        alignment's statistics (q), its folded convolution (second source), the last ResidualBlock's res2, tsa_fusion's centre --
        all take an image map at this shape in the form this forward runs them in.  Else the forward is launch for launch the one
        without the switch.  Both give the same bits, so the choice may depend on shape and mode."""
        if not self.stack_inplace or self.precision == "f32" or self.istraining:
            return False
        prec = self.PRECISIONS[self.precision]
        a = "MV_deform_align."
        G = int(getattr(self, "neighbour_group", 0)) or self.center
        # the forms of the default path: the mask statistics from the residual maps and fea_com inside the products (_compensate,
        # _inline_rms_planes), the alignment on its one-pass statistics (_align), the ResidualBlocks on the Block_ kernels (fast16)
        rms_inline = (self.prior_stems and K.rdab_stats_ok(H, W) and self.inline_rms and "rms_chunk" in w and self.rdab_fused
                      and K.plane_ok(H, W) and (H * W) % 64 == 0)
        ufs_inline = self.inline_ufs and "ufs_chunk" in w and K.plane_ok(H, W)
        fast16 = (self.precision == "fp16x2" and H % 2 == 0
                  and all(w[a + n].wh is not None for n in ("ResidualBlock.conv1", "ResidualBlock.conv2", "ResidualBlock1.conv1", "ResidualBlock1.conv2")))
        fea_r_prec = K.PREC_FP16X1 if self.fea_r_single_pass and prec == K.PREC_FP16X2 else prec
        return bool(rms_inline and self.align_stats and fast16
                    and K.rdab_prep_fused_map_ok(plane=True)
                    and K.conv_map_ok(w["RDAB.fuse"], prec, plane=True, res=True)
                    and K.conv_map_ok(w["conv_expand_fea_r"], fea_r_prec, pad=1)
                    and (not ufs_inline or K.conv1x1_map_ok(128, plane=True, chan_sum=True))      # the folded convolution: with the
                    and K.conv1x1_map_ok(192, chan_sum=True)                                    # partition map inside, or with pred
                    and K.ws_res_map_ok(G * B, H, W)
                    and K.conv_map_ok(w["tsa_fusion"], prec))

    def _fuse_windows(self, w, Lf, x, mvs1, rms, ufs, gumbel_uniform, deferred_new=None):
        """Steps 2-3 of the forward from the frame-major feature stack Lf [7,B,H,W,64], or from a _FeatureStack (the stack as it lies
        in memory, read in place; a frame-major tensor is read that way too where _stack_inplace allows): the six neighbour pipelines
        and the temporal fusion.  x: only its device is read here.  gumbel_uniform: resolved by forward() -- injected tensors, or None =
        draw inside the mask kernel.  deferred_new: `_front`'s cached path at B = 1 -- the new frame's feature extraction,
        enqueued behind the fork of the side streams.  Returns fused [B,H,W,64]."""
        N, ctr = NFRAMES, self.center
        nstr = int(getattr(self, "neighbour_streams", 0)) or 2
        gsz = int(getattr(self, "neighbour_group", 0)) or ctr
        # 2. per-neighbour compensation + alignment (arch.py:4443-4460)
        if ufs.shape[1] != 1:
            ufs, rms = ufs.transpose(1, 2), rms.transpose(1, 2)
        ufs = ufs.contiguous().float()
        rms = rms.contiguous().float()
        # The six neighbours share every weight of the compensation + alignment modules, so they are processed as two GROUPS of
        # three frames (frames 0-2 and 4-6 are contiguous in the frame-major feature stack): each operator runs once on 3*B
        # images instead of three times on B.  Only what reads a per-neighbour input plane (prior stems, noise draw, motion
        # field) is launched per neighbour, into slices of the group's tensors.  The two groups are independent: with
        # `neighbour_streams` > 1 they are issued on two side streams (joined before the temporal fusion).
        # group size: three frames per group (one launch per operator and group, two groups on two streams) at every batch size.
        # Round 2 kept one frame per group on six streams for one or two clips; measured again in round 3 on the streamed B = 1
        # sequence (tools/bench_streaming.py, 270x480): 66.7 frames/s grouped on two streams against 62.5 (68.1 / 65.6 under
        # HIP-graph replay)
        groups = [list(range(s, min(s + gsz, e))) for (s0, e) in ((0, ctr), (ctr + 1, N)) for s in range(s0, e, gsz)]
        if deferred_new is not None and self.new_frame_alone:
            groups = [list(range(0, ctr)), list(range(ctr + 1, N - 1)), [N - 1]]     # the new frame is a group of its own
        if not isinstance(Lf, _FeatureStack) and self._stack_inplace(w, Lf.shape[1], Lf.shape[2], Lf.shape[3]):
            _, B, H, W, _ = Lf.shape
            Lf = _FeatureStack(Lf, B, H, W, B * H * W * NF, H * W * NF)         # frame-major: the same path with its own strides
        if isinstance(Lf, _FeatureStack):
            xcG, centre = Lf.frame(ctr, times=gsz), Lf.frame(ctr)               # the centre of every clip, addressed once per neighbour
        else:
            xcG = Lf[ctr].repeat(gsz, 1, 1, 1) if gsz > 1 else Lf[ctr]      # the centre features once per neighbour of a group
            centre = Lf[ctr]
        keep = []
        aligned = self._fork_join(x.device, nstr, groups, deferred_new, lambda gi, idxs: self._neighbour_group(
            w, Lf, idxs, xcG, ufs, rms, mvs1, gumbel_uniform, keep))
        return self._fuse(w, centre, aligned)

    def _fuse_windows_shared(self, w, Lc, comp_bank, comp_idx, x, mvs1, ufs):
        """Steps 2b-3 of the forward with banked compensations: the two neighbour groups (slots 0-2 and 4-6) on the two side
        streams as in `_fuse_windows`, each aligning comp_bank[comp_idx[...]] to the centres; then the temporal fusion.  ufs:
        [K,1,7,H,W] dense.  Returns fused [K,H,W,64]."""
        B, N, ctr = x.shape[0], NFRAMES, self.center
        if self._stack_inplace(w, B, Lc.shape[1], Lc.shape[2]):
            xcG = K.image_map(Lc[0], ctr * B, B, Lc.stride(0), 0)             # the centres, addressed once per neighbour
        else:
            xcG = Lc.repeat(ctr, 1, 1, 1)
        keep = []
        aligned = self._fork_join(x.device, 2, [list(range(0, ctr)), list(range(ctr + 1, N))], None, lambda gi, idxs: self._align_group(
            w, idxs, xcG, ufs, mvs1, keep, frames=(comp_bank, comp_idx[gi * ctr * B:(gi + 1) * ctr * B])))
        return self._fuse(w, Lc, aligned)

    def _fork_join(self, device, nstr, groups, deferred_new, body):
        """The neighbour groups `groups` (lists of frame indices) beside each other: ``body(gi, idxs)`` -> the group's aligned
        features [len(idxs)*B,H,W,64], neighbour major, issued under one of `nstr` side streams (on the caller's stream with
        nstr = 1).  Returns {frame index: its [B,H,W,64] slice}, complete on the caller's stream.
        The groups' common inputs -- the feature stack, and xcG, the centre features per neighbour -- are complete on the caller's
        stream BEFORE this call: the side streams read them (Gram pass and last residual of _align) behind their wait.  Read in place
        (_stack_inplace) xcG is an image map of the stack and nothing is enqueued for it; else it is a copy on the caller's stream,
        ordered ahead of the wait like the stack.  deferred_new (`_front`: the new frame's feature extraction) is enqueued on the caller's stream behind the
        fork, so the side streams do not wait for it; the group that reads the new frame then follows it on the caller's stream."""
        main = torch.cuda.current_stream(device)
        side = self._side(device, nstr) if nstr > 1 else []
        for st in side:
            st.wait_stream(main)
        if deferred_new is not None:
            deferred_new()
        by_frame = {}
        for gi, idxs in enumerate(groups):
            on_side = bool(side) and not (deferred_new is not None and NFRAMES - 1 in idxs)
            with torch.cuda.stream(side[gi % len(side)]) if on_side else contextlib.nullcontext():
                al = body(gi, idxs)
            if on_side:
                al.record_stream(main)               # produced on a side stream, consumed on the caller's
            B = al.shape[0] // len(idxs)
            for n, i in enumerate(idxs):
                by_frame[i] = al[n * B:(n + 1) * B]
        for st in side:
            main.wait_stream(st)
        return by_frame

    def _fuse(self, w, centre, aligned):
        """Step 3, temporal fusion (arch.py:4463) of the aligned neighbours {frame index: [B,H,W,64]} and the centre features;
        the range guard's first probe reads its result, the trunk's input."""
        fused = self._conv([centre if i == self.center else aligned[i] for i in range(NFRAMES)], w["tsa_fusion"], act=K.ACT_LRELU)
        if self._probe is not None:
            K.range_probe(fused, self._probe[0:2])
        return fused

    def _back(self, fused, x, L1=None):
        """Steps 4-5: reconstruction trunk, upsampling + skip (arch.py:4464-4481).  x: the fp32 input clip of `_front`."""
        B, N, C, H, W = x.shape
        w = self._weights()
        raw = w["raw"]
        ctr, P = self.center, H * W
        t = self._trunk(w, fused)
        if self._probe is not None:
            # the second probe of the fp16 range guard sits on the trunk's OUTPUT (round 5; rounds 2-4 probed the final image): the
            # up-sampler's fused tail turns a non-finite trunk result into finite garbage (its block scale comes from an integer maximum of
            # bit patterns), so the image itself can look healthy when a Block_'s fp16 intermediate has overflowed
            K.range_probe(t, self._probe[2:4])
        if self.debug_taps is not None:
            self.debug_taps.update(L1_fea=L1, fused=fused, trunk=t)
        t = self._conv(t, w["upconv1"], act=K.ACT_LRELU)
        if self.precision == "f32":
            t = self._conv(t, w["upconv2"], act=K.ACT_LRELU)
            out = K.conv_last(t, raw["conv_last.weight"], raw["conv_last.bias"], x[:, ctr], N * P)
        else:   # upconv2 writes conv_last's nine per-tap channel sums instead of the 64-channel HR map
            out = K.upconv_last(t, w["upconv2"], raw["conv_last.weight"], raw["conv_last.bias"], x[:, ctr], N * P)
        return out

    def _neighbour_group(self, w, Lf, idxs, xcG, ufs, rms, mvs1, noise, keep):
        """Neighbour frames `idxs` (consecutive) of the frame-major stack Lf [7,B,H,W,64] together: RDAB compensation,
        conv_expand_fea_r, prior stems, MV alignment (arch.py:4443-4460) on [len(idxs)*B, H, W, 64] tensors, neighbour major.
        rms / ufs: [B,1,7,H,W] dense."""
        if isinstance(Lf, _FeatureStack):
            N, B, H, W = NFRAMES, Lf.B, Lf.H, Lf.W
        else:
            N, B, H, W, _ = Lf.shape
        G = len(idxs)
        fea = Lf.group(idxs[0], G) if isinstance(Lf, _FeatureStack) else Lf[idxs[0]:idxs[0] + G].view(G * B, H, W, NF)
        # fea_com = fea_i + rms_prior and du0 = relu(conv_du_re.0(rms_prior)) from the residual map itself, per neighbour; a
        # neighbour's noise draw is its rank among the six
        stems = [(rms[:, 0, i], N * H * W, slice(n * B, (n + 1) * B)) for n, i in enumerate(idxs)]
        draws = [i - (i > self.center) for i in idxs]
        fea_i, x_n = self._compensate(w, fea, stems, draws,
                                      None if noise is None else [noise[d] for d in draws], keep)
        if self.debug_taps is not None:
            for n, i in enumerate(idxs):
                self.debug_taps[f"rdab_{i}"] = x_n[n * B:(n + 1) * B]
        return self._align_group(w, idxs, xcG, ufs, mvs1, keep, extra=fea_i)

    def _compensate(self, w, fea, stems, draws, noise, keep=None):
        """The per-frame half of a neighbour pipeline (arch.py:4443-4454) on a stack of images fea [M,H,W,64]:
        fea_i = conv_expand_fea_r([fea, RDAB(fea + conv_expand_rms(rms))]).  stems: (rms view, batch stride, slice) -- one
        stem launch per entry, on the residual maps of the images fea[slice] (image b of the view at b * batch stride); draws:
        the Philox draw index of each mask launch (M / len(draws) consecutive images each); noise: the injected uniforms of each
        mask launch instead, or None.  Returns (fea_i, x_n = the RDAB output); keep: receives the intermediates."""
        raw = w["raw"]
        M, H, W, _ = fea.shape
        dev = fea.device
        du0 = stats = planes = None
        if self.prior_stems and self.precision != "f32" and not self.istraining and K.rdab_stats_ok(H, W):
            # du0 has one consumer, a convolution whose result has one consumer, the global average pool: K.rdab_stats goes from the
            # residual maps to the pool's partial sums, and the stem only adds conv_expand_rms(rms) to the features
            stats = self._mask_stats(w, stems, M, H, W)
            planes = self._inline_rms_planes(w, fea, stems, len(draws))
        if planes is None and isinstance(fea, K.ImageMap):
            raise ValueError("_compensate: a mapped stack needs the inline residual planes (_stack_inplace decides before the first launch)")
        if planes is not None:
            # ... and that sum has two consumers, both matrix products over the pixel's channels: they read fea and the residual map
            fea_com = None
        elif stats is not None:
            fea_com = K.empty_act(M, H, W, NF, dev)
            for rms, bstride, sl in stems:
                K.stem_conv(rms, bstride, sl.stop - sl.start, H, W, raw["conv_expand_rms.weight"], raw["conv_expand_rms.bias"],
                            add=fea[sl], out2=fea_com[sl], write_out=False)
        else:
            fea_com = K.empty_act(M, H, W, NF, dev)
            du0 = K.empty_act(M, H // 2 + 1, W // 2 + 1, 4 * NF, dev)       # space-to-depth, + one zero row / column
            du0[:, H // 2].zero_()
            du0[:, :, W // 2].zero_()
            for rms, bstride, sl in stems:
                K.stem_conv2(rms, bstride, sl.stop - sl.start, H, W, raw["conv_expand_rms.weight"], raw["conv_expand_rms.bias"],
                             fea[sl], fea_com[sl], w["rms_du0"][0], w["rms_du0"][1], K.ACT_RELU, du0[sl], s2dB=True)
        noises = []
        for k, draw in enumerate(draws):
            if noise is None:
                # the reference's default (torch.rand_like per call, arch.py:2169): the draws are generated INSIDE rdab_prep
                # (Philox4x32-10), the [B,64,H,W] noise tensor never exists; `capture_noise` (tests) asks for a copy
                cap = None
                if self.capture_noise is not None:
                    cap = torch.empty((M // len(draws), NF, H, W), device=dev, dtype=torch.float32)
                    self.capture_noise.append(cap)
                noises.append(("rng", self._noise_seed, draw, cap))
            else:
                noises.append(noise[k].to(device=dev, dtype=torch.float32).contiguous())
        if planes is not None:
            x_n = self._rdab(w, du0, fea, noises, stats, rms_planes=planes)
        else:
            x_n = self._rdab(w, du0, fea_com, noises, stats)
        fea_i = self._conv([fea, x_n], w["conv_expand_fea_r"], pad=1, inner=self.fea_r_single_pass)
        if keep is not None:
            keep.extend([du0, stats, fea_com, noises, x_n, fea_i])
        return fea_i, x_n

    @staticmethod
    def _affine_stems(stems):
        """(view, Bi, s_b, s_g) where the stems' planes lie at one stride behind each other (consecutive slots of one [B,1,7,H,W]
        tensor) and their slices tile the image stack in order: image m's plane at view + (m % Bi) s_b + (m // Bi) s_g.  Else None."""
        v0, s_b, sl0 = stems[0]
        Bi = sl0.stop - sl0.start
        step = (stems[1][0].data_ptr() - v0.data_ptr()) // 4 if len(stems) > 1 else 0
        if step >= 0 and all(v.untyped_storage().data_ptr() == v0.untyped_storage().data_ptr() and bs == s_b
                             and (sl.start, sl.stop) == (k * Bi, (k + 1) * Bi) and v.data_ptr() == v0.data_ptr() + 4 * k * step
                             for k, (v, bs, sl) in enumerate(stems)):
            return v0, Bi, s_b, step
        return None

    def _inline_rms_planes(self, w, fea, stems, nnoise):
        """The plane addressing for _rdab where fea_com need not be written (model.inline_rms): the composed tables are packed, the
        mask kernel is the fused one, the planes are affine and inside the plane chunk's contract, and the images of one noise
        (M / nnoise consecutive ones) lie inside one stem -- a neighbour group's one noise per stem, compensate_features' one
        stem for all frames with a noise each: which path a frame takes must not depend on how many frames share the call.  Else
        None: the stem kernel writes fea_com (stems without a common stride stay on that path)."""
        M, H, W, _ = fea.shape
        if not (self.inline_rms and "rms_chunk" in w and self.rdab_fused and K.plane_ok(H, W) and M % nnoise == 0
                and K.rdab_prep_fused_ok(fea, w["RDAB.input_conv"])):
            return None
        aff = self._affine_stems(stems)
        if aff is None or aff[1] % (M // nnoise) or any(v.dtype != torch.float32 for v, _, _ in stems):
            return None
        return aff

    @staticmethod
    def _mask_stats(w, stems, M, H, W):
        """K.rdab_stats over the stems of `_compensate` (M images in all): one launch where the stems' planes lie at one stride
        behind each other (consecutive slots of one [B,1,7,H,W] tensor), else one launch per stem.  Returns (partials, slots,
        pixel count)."""
        args = (*w["rms_du0"], w["RDAB.conv_du_re.2_stats"], w["raw"]["RDAB.conv_du_re.2.bias"])
        aff = CVSR_V8._affine_stems(stems)
        if aff is not None:
            v0, Bi, s_b, step = aff
            return K.rdab_stats(v0, Bi, s_b, step, M, H, W, *args)
        count = (H // 2 + 1) * (W // 2 + 1)
        n = K.nchunks_for(count)
        part = torch.empty((M, n, 64), dtype=torch.float32, device=stems[0][0].device)
        for v, bs, sl in stems:
            K.rdab_stats(v, sl.stop - sl.start, bs, 0, sl.stop - sl.start, H, W, *args, out=part[sl])
        return part, n, count

    def _align_group(self, w, idxs, xcG, ufs, mvs1, keep, extra=None, frames=None):
        """The alignment half of a neighbour pipeline for the slots `idxs` (consecutive): the partition-map stem per slot and the
        MV alignment (arch.py:4455-4460) of the slots' compensated features to the centres xcG.  Those features are `extra`
        [len(idxs)*B,H,W,64], neighbour major, or with frames = (comp_bank, idx) the bank of compensate_features, read in place:
        image n*B + b is comp_bank[idx[n*B + b]].  ufs: [B,1,7,H,W] dense, mvs1: [B,7,2,H,W] dense."""
        raw = w["raw"]
        B, N, _, H, W = mvs1.shape
        GB, P = len(idxs) * B, H * W
        # model.inline_ufs: ufs_prior has two readers, both matrix products over the pixel's channels -- they read the partition map
        # itself.  The slots of a group are consecutive, so image n*B + b's plane lies at ufs[b, 0, idxs[0] + n]: always affine.  The
        # same conditions for both callers: which path a frame takes must not depend on how many frames share the call
        planes = ufs_prior = None
        if (self.inline_ufs and "ufs_chunk" in w and self.precision != "f32" and not self.istraining and self.align_stats
                and K.plane_ok(H, W) and ufs.dtype == torch.float32 and ufs.is_contiguous()):
            planes = (ufs[:, 0, idxs[0]], B, N * P, P)
        else:
            ufs_prior = K.empty_act(GB, H, W, NF, xcG.device)
            for n, i in enumerate(idxs):
                K.stem_conv(ufs[:, 0, i], N * P, B, H, W, raw["conv_expand_ufs.weight"], raw["conv_expand_ufs.bias"],
                            out=ufs_prior[n * B:(n + 1) * B])
        al = K.empty_act(GB, H, W, NF, xcG.device)
        xc = xcG if xcG.shape[0] == GB else (xcG.sub(0, GB) if isinstance(xcG, K.ImageMap) else xcG[:GB])
        self._align(w, xc, extra, ufs_prior, [mvs1[:, i] for i in idxs], N * 2 * P, al,
                    frames=None if frames is None else (*frames, mvs1, idxs[0]), ufs_planes=planes)
        if self.debug_taps is not None:
            for n, i in enumerate(idxs):
                self.debug_taps[f"align_{i}"] = al[n * B:(n + 1) * B]
        keep.extend([xc] if ufs_prior is None else [ufs_prior, xc])
        return al

    @staticmethod
    def _as_pixel_major(t: torch.Tensor, F: int, H: int, W: int) -> torch.Tensor:
        """[F,64,H,W] in either memory format -> dense pixel-major [F,H,W,64]."""
        if tuple(t.shape) != (F, NF, H, W):
            raise ValueError(f"pre_L1_fea must be [{F},{NF},{H},{W}], got {tuple(t.shape)}")
        t = t.float()
        v = t.permute(0, 2, 3, 1)
        if v.is_contiguous():
            return v
        return K.nchw_to_nhwc(t.contiguous())
