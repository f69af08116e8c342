"""Host side of `model.inline_ufs` (CDFO_INLINE_UFS): the path `CVSR_V8._align_group` selects, the two entry points' prototypes and the
composed table of the statistics kernel.  No GPU: the kernels are replaced by recorders."""
import ctypes as C

import pytest
import torch

from cdfo_amd import _lib
from cdfo_amd import kernels as K


def test_header_declares_the_entry_points():
    protos = _lib.header_prototypes()
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    restype, argtypes = protos["cdfo_align_stats_plane"]
    # x0, ld0, q, ldq, w_packed, bias, act, ch_per_head, B, P, nslots, gram, sum0, sum1 | plane, Bi, s_b, s_g, W, plane_w, stencil_w | stream
    assert restype is C.c_int and argtypes == [vp, i, vp, i, vp, vp, i, i, i, ll, i, vp, vp, vp, vp, i, ll, ll, i, vp, vp, vp]
    base = protos["cdfo_align_stats"][1]
    assert argtypes[:2] + argtypes[2:14] == base[:2] + base[4:-1]          # cdfo_align_stats without x1 / ld1, then the plane
    restype, argtypes = protos["cdfo_align_fold_plane"]
    base = protos["cdfo_align_fold"][1]
    # cdfo_align_fold's inputs, the stencil's table, B, wout | tables, stream
    assert restype is C.c_int and argtypes == base[:13] + [vp] + base[13:15] + [vp, vp]
    assert _lib.lib().cdfo_abi_version() == 1


def test_composed_table_is_the_second_half_of_fusion_out_times_the_stencil_in_float64():
    g = torch.Generator().manual_seed(11)
    w_u, b_u = torch.randn(64, 1, 3, 3, generator=g), torch.randn(64, generator=g)
    wf = torch.randn(64, 128, 1, 1, generator=g)
    t = K.pack_plane_chunk(*K.compose_stem_1x1(w_u, b_u, wf[:, 64:], torch.zeros(64)))
    want = wf.double().view(64, 128)[:, 64:] @ torch.cat([w_u.double().view(64, 9), b_u.double().view(64, 1)], 1)
    assert tuple(t.shape) == (64, 16) and torch.equal(t[:, :10], want.float()) and not t[:, 10:].any()
    # ... and the un-composed one is the stencil itself
    s = K.pack_plane_chunk(w_u, b_u)
    assert torch.equal(s[:, :9], w_u.view(64, 9)) and torch.equal(s[:, 9], b_u) and not s[:, 10:].any()


def _model(monkeypatch, inline, precision="fp16x2", training=False, align_stats=True):
    from arch.SIDECVSR_our import CVSR_V8
    m = CVSR_V8()
    m.inline_ufs, m._precision, m.istraining, m.align_stats = inline, precision, training, align_stats
    calls = []
    monkeypatch.setattr(K, "empty_act", lambda B, Hh, Ww, Cc, dev: torch.zeros(B, Hh, Ww, Cc))
    monkeypatch.setattr(K, "stem_conv", lambda *a, **kw: calls.append(("stem_conv",)))
    monkeypatch.setattr(m, "_align", lambda w, xc, extra, pred, mvs, mv_bstride, out, frames=None, ufs_planes=None: calls.append(
        ("align", pred is None, None if ufs_planes is None else (ufs_planes[0].data_ptr(), *ufs_planes[1:]), frames is not None)))
    z = torch.zeros(1)
    w = {"raw": {"conv_expand_ufs.weight": z, "conv_expand_ufs.bias": z}, "ufs_chunk": z, "ufs_chunk_fusion_out": z}
    return m, w, calls


@pytest.mark.parametrize("inline,precision,training,align_stats,frames,expect", [
    (True, "fp16x2", False, True, False, True), (True, "bf16x3", False, True, False, True),
    (False, "fp16x2", False, True, False, False),      # the switch
    (True, "f32", False, True, False, False), (True, "fp16x2", True, True, False, False),
    (True, "fp16x2", False, False, False, False),      # without align_stats ufs_prior has other readers
    (True, "fp16x2", False, True, True, True), (False, "fp16x2", False, True, True, False),      # the frames= form: the same conditions
])
def test_align_group_selects_the_path(monkeypatch, inline, precision, training, align_stats, frames, expect):
    m, w, calls = _model(monkeypatch, inline, precision, training, align_stats)
    H, W, B, idxs = 8, 8, 2, [4, 5, 6]
    ufs, mvs1 = torch.zeros(B, 1, 7, H, W), torch.zeros(B, 7, 2, H, W)
    xcG = torch.zeros(3 * B, H, W, 64)
    keep = []
    fr = (torch.zeros(5, H, W, 64), torch.zeros(3 * B, dtype=torch.int64)) if frames else None
    m._align_group(w, idxs, xcG, ufs, mvs1, keep, extra=None if frames else torch.zeros(3 * B, H, W, 64), frames=fr)
    stems = [c for c in calls if c[0] == "stem_conv"]
    if expect:      # no stem launch, no ufs_prior: _align gets pred = None and the group's plane addressing, nothing kept for ufs_prior
        assert stems == [] and calls[-1] == ("align", True, (ufs[:, 0, 4].data_ptr(), B, 7 * H * W, H * W), frames)
        assert len(keep) == 1 and keep[0].shape == xcG.shape
    else:
        assert len(stems) == 3 and calls[-1] == ("align", False, None, frames)
        assert len(keep) == 2 and tuple(keep[0].shape) == (3 * B, H, W, 64)


def test_path_does_not_depend_on_the_frames_sharing_the_call(monkeypatch):
    """one window or four: the same path (the chunked evaluators rely on it); a half-precision partition map stays materialised"""
    for B in (1, 4):
        m, w, calls = _model(monkeypatch, True)
        H, W = 8, 8
        m._align_group(w, [0, 1, 2], torch.zeros(3 * B, H, W, 64), torch.zeros(B, 1, 7, H, W), torch.zeros(B, 7, 2, H, W), [],
                       frames=(torch.zeros(9, H, W, 64), torch.zeros(3 * B, dtype=torch.int64)))
        assert calls == [("align", True, calls[0][2], True)] and calls[0][2][1:] == (B, 7 * H * W, H * W)
    m, w, calls = _model(monkeypatch, True)
    m._align_group(w, [0, 1, 2], torch.zeros(3, 8, 8, 64), torch.zeros(1, 1, 7, 8, 8, dtype=torch.float16), torch.zeros(1, 7, 2, 8, 8), [],
                   extra=torch.zeros(3, 8, 8, 64))
    assert [c[0] for c in calls] == ["stem_conv"] * 3 + ["align"] and calls[-1][1:3] == (False, None)


def test_wrappers_refuse_what_the_kernels_do_not_take():
    x = torch.zeros(1, 4, 4, 64)
    pc = K.PackedConv(torch.zeros(128 * 64), None, 64, 128, 1, 64)
    with pytest.raises(ValueError, match="either x1 or the plane"):
        K.align_stats(x, None, x, pc, K.ACT_RELU, 16)
    with pytest.raises(ValueError, match="either x1 or the plane"):
        K.align_stats(x, x, x, pc, K.ACT_RELU, 16, plane=(x, 1, 0, 0, torch.zeros(64, 16), torch.zeros(64, 16)))
    with pytest.raises(ValueError, match="stencil"):
        K.align_fold_plane(torch.zeros(1, 1, 64 * 18), 1, None, None, 1, 16, *([None] * 7), torch.zeros(64, 9))
