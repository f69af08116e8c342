"""The developer switches of cdfo_amd: ONE table of every CDFO_* environment variable, and the one reader of the Python layer.

A switch never changes what is computed beyond the documented precision modes -- it selects a kernel form or a schedule, for
same-box A/B measurements.  Rules, the same for every name:

  * unset -> the row's default; on/off switches: "0" -> off, "1" -> on; int switches: one of the row's values (any integer
    where the row lists none); any other value, the empty string included, raises ValueError naming the variable;
  * a name that is not a row of TABLE is refused (KeyError);
  * the environment is read once per process per name: set a switch before the first use, not between forwards.

Rows of layer "python" are read through get() below and nowhere else; rows of layer "hip" are read inside libcdfo_hip.so by
csrc/common.h's cdfo_switch(name, default) (atoi of the same values) and are validated here when the library is loaded
(check_hip_environment).  INTEGRATION.md section 1 carries the same table; tests/test_switches_cpu.py keeps the three in step.

Read by the harness files themselves, not rows: CDFO_BENCH_BACKEND, CDFO_BENCH_PG_TIMEOUT_S (bench.py), CDFO_FORKSERVER
(tests/conftest.py).
"""
from __future__ import annotations

import functools
import os
from typing import NamedTuple, Optional, Tuple, Union

ONOFF, INT, PATH = "on/off", "int", "path"


class Switch(NamedTuple):
    name: str
    default: Union[int, None]          # on/off: 0 | 1; int: the integer; path: None
    kind: str                          # ONOFF | INT | PATH
    layer: str                         # "python" | "hip": who reads it
    meaning: str
    values: Optional[Tuple[int, ...]] = None     # int switches: the allowed values (None = any integer)


TABLE = (
    # --- Python layer -------------------------------------------------------------------------------------------------------
    Switch("CDFO_LIB_PATH", None, PATH, "python", "another build of libcdfo_hip.so (A/B builds, the developer library cdfo_amd/lib/dev/)"),
    Switch("CDFO_DCN_EXACT", 0, ONOFF, "python", "1: the DCN forward always on its exact-fp32 kernel (cdfo_amd.dcn.EXACT_FP32)"),
    Switch("CDFO_TRAIN_EXACT", 0, ONOFF, "python", "1: the training path's convolutions on exact-fp32 MFMA (cdfo_amd.autograd.CONV_PREC = PREC_F32)"),
    Switch("CDFO_WINO", 1, ONOFF, "python", "0: Block_.body[0] stays on the direct weights-stationary kernel instead of the Winograd F(2,3) one"),
    Switch("CDFO_WINO_UP2", 1, ONOFF, "python", "0: Block_'s x2 branch on a materialised double-resolution source instead of the interpolating Winograd form"),
    Switch("CDFO_WINO_HS", 0, ONOFF, "python", "1: the x2 branch's 256-channel intermediate in half-split rows (model.wino_halfsplit; measured: no gain in the forward, 105.2 vs 105.3 ms)"),
    Switch("CDFO_UDSA_N16", 1, ONOFF, "python", "0: the prior U-net's first layer off the 16-channel kernel (model.udsa_n16)"),
    Switch("CDFO_UDSA_STREAM", 1, ONOFF, "python", "0: the prior U-net on the caller's stream instead of a side stream (model.udsa_side_stream)"),
    Switch("CDFO_ATTN_PV3", 0, ONOFF, "python", "1: all three fp16 passes in the attentions' second product instead of one (model.attn_pv_single = False)"),
    Switch("CDFO_OVERLAP_NEW", 1, ONOFF, "python", "0: streaming, frames 0-2 start behind the new frame's feature extraction, not beside it (model.overlap_new_frame)"),
    Switch("CDFO_NEW_ALONE", 1, ONOFF, "python", "0: streaming, the new frame's neighbour pipeline is not a group of its own (model.new_frame_alone)"),
    Switch("CDFO_TRUNK_SIDE", 1, ONOFF, "python", "0: Block_'s half-resolution branch on the caller's stream instead of a side stream (model.trunk_side_stream)"),
    Switch("CDFO_FEA_R_1PASS", 0, ONOFF, "python", "1: conv_expand_fea_r with activations rounded once to fp16 (model.fea_r_single_pass)"),
    Switch("CDFO_V7_FEAR_1PASS", 1, ONOFF, "python", "0: CVSR_V7's conv_expand_fea_r on fp16 hi + lo activations, two passes (model.fea_r_single_pass)"),
    Switch("CDFO_V7_FUSE_ASSEMBLY", 1, ONOFF, "python", "0: MVDualAttAlignment assembles offsets / masks in a kernel of its own (fuse_assembly)"),
    Switch("CDFO_V7_HEAD_1PASS", 1, ONOFF, "python", "0: MVDualAttAlignment's offset head on two-pass activations (head_one_pass)"),
    Switch("CDFO_V7_OFF0_1PASS", 1, ONOFF, "python", "0: MVDualAttAlignment's conv_offset[0] on two-pass activations (off0_one_pass)"),
    Switch("CDFO_V7_WS_HEAD", 1, ONOFF, "python", "0: MVDualAttAlignment's offset head off the weights-stationary kernel (ws_head)"),
    Switch("CDFO_ALIGN_STATS", 1, ONOFF, "python", "0: DualAttAlignment's statistics on the five launches of round 5: kf written, Gram and channel sums in passes of their own (model.align_stats)"),
    Switch("CDFO_RDAB_FUSED", 1, ONOFF, "python", "0: LLongRangAttention's input_conv and mask kernel as two launches with the 128-channel product written, every V operand of its attentions fp32 (model.rdab_fused)"),
    Switch("CDFO_PRIOR_STEMS", 1, ONOFF, "python", "0: LLongRangAttention's mask statistics through memory: du0 written by the stem kernel, read back by conv_du_re.2, its result summed by a third launch (model.prior_stems)"),
    Switch("CDFO_INLINE_RMS", 1, ONOFF, "python", "0: fea_com = fea + conv_expand_rms(rms) written by the stem kernel and read by the mask kernel and RDAB.fuse, instead of built inside their products from the residual map; needs CDFO_PRIOR_STEMS (model.inline_rms)"),
    Switch("CDFO_INLINE_UFS", 1, ONOFF, "python", "0: ufs_prior = conv_expand_ufs(ufs) written by one stem launch per neighbour and read by DualAttAlignment's statistics pass and its folded 192 -> 64 convolution, instead of built inside their products from the partition map; needs CDFO_ALIGN_STATS (model.inline_ufs)"),
    Switch("CDFO_STACK_INPLACE", 1, ONOFF, "python", "0: the neighbour phase reads a frame-major copy of the feature stack (K.swap_outer) and the centre features repeated per neighbour, instead of the stack where the extractor wrote it through image maps in its seven readers (model.stack_inplace)"),
    # --- HIP layer (csrc/) --------------------------------------------------------------------------------------------------
    Switch("CDFO_WS_RING", 1, ONOFF, "hip", "0: Block_.body[0] on the private-halo kernel of rounds 1-2 instead of the ring-fed wave-specialised one"),
    Switch("CDFO_WS_WAVES", 12, INT, "hip", "8: two instead of three waves per SIMD in the private-halo weights-stationary kernel", (8, 12)),
    Switch("CDFO_RING_SPLIT", 1, ONOFF, "hip", "0: the four-tap ring convolution on the eight-identical-waves kernel"),
    Switch("CDFO_RING_TOUCH", 0, ONOFF, "hip", "1: producer-side touches of the tile's residual lines ahead of the epilogue (measured useless, off)"),
    Switch("CDFO_CONV1X1_STREAM", 1, ONOFF, "hip", "0: 1x1 convolutions on the one-tile-per-workgroup kernel instead of the persistent streaming one"),
    Switch("CDFO_TAPS_STREAM", 1, ONOFF, "hip", "0: the CDFO_STORE_TAPS9 1x1 convolution off the persistent streaming kernel"),
    Switch("CDFO_ATTN_NW", 0, INT, "hip", "4 | 8: force the attention workgroup width (0: chosen per shape)", (0, 4, 8)),
    Switch("CDFO_ATTN_XCD", 1, INT, "hip", "0: attention workgroups of one sequence spread over the XCDs as in round 2"),
    Switch("CDFO_DCN_WIN", 1, INT, "hip", "0: the DCN forward on the round-2 gather kernel instead of the window-sampled one"),
    Switch("CDFO_DCN_DBG", 0, INT, "hip", "developer library only (-DCDFO_DEV_ABLATIONS): ablation code of the window-sampled DCN kernel, wrong results"),
)
_ROWS = {s.name: s for s in TABLE}


def _parse(sw: Switch, raw: Optional[str]):
    if sw.kind == PATH:
        return raw or None
    if raw is None:
        return bool(sw.default) if sw.kind == ONOFF else sw.default
    if sw.kind == ONOFF and raw in ("0", "1"):
        return raw == "1"
    if sw.kind == INT and raw.lstrip("-").isdigit() and (sw.values is None or int(raw) in sw.values):
        return int(raw)
    allowed = "0 or 1" if sw.kind == ONOFF else ("one of %s" % (sw.values,) if sw.values else "an integer")
    raise ValueError(f"{sw.name}={raw!r}: expected {allowed} (cdfo_amd/switches.py)")


@functools.lru_cache(maxsize=None)
def get(name: str):
    """The value of a python-layer switch: bool (on/off), int, or a path / None.  Read once per process."""
    sw = _ROWS[name]
    if sw.layer != "python":
        raise KeyError(f"{name} is read by the HIP library, not by Python")
    return _parse(sw, os.environ.get(name))


def check_hip_environment() -> None:
    """Apply the table's rules to the hip-layer variables that are set (called once, when the library is loaded)."""
    for sw in TABLE:
        if sw.layer == "hip":
            _parse(sw, os.environ.get(sw.name))
