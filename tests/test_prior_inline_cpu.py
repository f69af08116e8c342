"""Host side of the plane chunk (`kernels.pack_plane_chunk`, the `plane` keyword of `kernels.conv` / `kernels.rdab_prep_fused`) and
the path `CVSR_V8._compensate` selects with `model.inline_rms`.  No GPU: the kernels are replaced by recorders."""
import ctypes as C

import pytest
import torch

from cdfo_amd import _lib
from cdfo_amd import kernels as K


def test_table_layout_and_composition_against_float64():
    g = torch.Generator().manual_seed(3)
    ws, bs = torch.randn(64, 1, 3, 3, generator=g), torch.randn(64, generator=g)
    w1, b1 = torch.randn(128, 64, 1, 1, generator=g), torch.randn(128, generator=g)
    t = K.pack_plane_chunk(ws, bs)
    assert t.dtype == torch.float32 and tuple(t.shape) == (64, 16) and t.is_contiguous()
    assert torch.equal(t[:, :9], ws.view(64, 9)) and torch.equal(t[:, 9], bs) and not t[:, 10:].any()
    # composed with a 1x1 product (its own bias stays with the product): W . [w_s | b_s] in float64, rounded once
    tc = K.pack_plane_chunk(*K.compose_stem_1x1(ws, bs, w1, torch.zeros(128)))
    want = w1.double().view(128, 64) @ torch.cat([ws.double().view(64, 9), bs.double().view(64, 1)], 1)
    assert tuple(tc.shape) == (128, 16) and torch.equal(tc[:, :10], want.float()) and not tc[:, 10:].any()
    # the stencil of one pixel through the table = the 1x1 product of the stencil
    nb = torch.randn(9, generator=g).double()
    direct = w1.double().view(128, 64) @ (ws.double().view(64, 9) @ nb + bs.double())
    assert (tc[:, :10].double() @ torch.cat([nb, torch.ones(1, dtype=torch.float64)]) - direct).abs().max() < 1e-5
    with pytest.raises(ValueError):
        K.pack_plane_chunk(ws[:, :, :2], bs)


def test_plane_addressing_is_checked_against_the_storage():
    H, W, B = 4, 6, 2
    stack = torch.zeros(B, 1, 7, H, W)
    table = torch.zeros(64, 16)
    v, Bi, s_b, s_g, t, ts = K._plane_args((stack[:, 0, 4], B, 7 * H * W, H * W, table), 3 * B, H, W, 64, "t")
    assert (Bi, s_b, s_g, ts) == (B, 7 * H * W, H * W, 0) and v.data_ptr() == stack[:, 0, 4].data_ptr()
    with pytest.raises(ValueError, match="storage"):      # slots 5, 6, 7: the last one does not exist
        K._plane_args((stack[:, 0, 5], B, 7 * H * W, H * W, table), 3 * B, H, W, 64, "t")
    with pytest.raises(ValueError, match="table"):
        K._plane_args((stack[:, 0, 4], B, 7 * H * W, H * W, torch.zeros(128, 16)), B, H, W, 64, "t")
    with pytest.raises(ValueError):
        K._plane_args((stack[:, 0, 4], B, -1, 0, table), B, H, W, 64, "t")
    assert K.plane_ok(272, 480) and not K.plane_ok(0, 8) and not K.plane_ok(1 << 15, 1 << 15)


def test_header_declares_the_entry_points():
    protos = _lib.header_prototypes()
    restype, argtypes = protos["cdfo_conv1x1_bf16x3_plane"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]
    restype, argtypes = protos["cdfo_rdab_prep_fused_plane"]
    base = protos["cdfo_rdab_prep_fused"][1]
    assert argtypes == base[:-1] + [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    assert _lib.lib().cdfo_abi_version() == 1


def _model(monkeypatch, inline, prior_stems=True, precision="fp16x2", training=False):
    from arch.SIDECVSR_our import CVSR_V8
    m = CVSR_V8()
    m.inline_rms, m.prior_stems, m._precision, m.istraining = inline, prior_stems, precision, training
    calls = []
    monkeypatch.setattr(K, "empty_act", lambda B, Hh, Ww, Cc, dev: torch.zeros(B, Hh, Ww, Cc))
    monkeypatch.setattr(K, "stem_conv", lambda *a, **kw: calls.append(("stem_conv", kw.get("write_out"))))
    monkeypatch.setattr(K, "stem_conv2", lambda *a, **kw: calls.append(("stem_conv2", kw.get("s2dB"))))
    monkeypatch.setattr(K, "rdab_stats", lambda img, Bi, s_b, s_g, B, *a, **kw: calls.append(("rdab_stats", Bi, s_b, s_g, B)) or ("part", 1, 25))
    monkeypatch.setattr(m, "_rdab", lambda w, du0, x, noises, stats=None, rms_planes=None:
                        calls.append(("rdab", None if rms_planes is None else rms_planes[1:])) or x)
    monkeypatch.setattr(m, "_conv", lambda srcs, *a, **kw: srcs[0])
    z = torch.zeros(1)
    ic = K.PackedConv(z, z, 128, 64, 1, 128)
    w = {"raw": {"conv_expand_rms.weight": z, "conv_expand_rms.bias": z, "RDAB.conv_du_re.2.bias": z}, "rms_du0": (z, z),
         "RDAB.conv_du_re.2_stats": z, "conv_expand_fea_r": None, "rms_chunk": z, "rms_chunk_input_conv": z, "RDAB.input_conv": ic}
    return m, w, calls


@pytest.mark.parametrize("inline,prior_stems,precision,training,slots,expect", [
    (True, True, "fp16x2", False, (4, 5, 6), True), (True, True, "bf16x3", False, (0, 1, 2), True),
    (False, True, "fp16x2", False, (4, 5, 6), False),      # the switch
    (True, False, "fp16x2", False, (4, 5, 6), False),      # without prior_stems the stem launch writes fea_com anyway
    (True, True, "f32", False, (4, 5, 6), False), (True, True, "fp16x2", True, (4, 5, 6), False),
    (True, True, "fp16x2", False, (1, 3, 6), False),       # non-affine stems: the materialised path
])
def test_compensate_selects_the_path(monkeypatch, inline, prior_stems, precision, training, slots, expect):
    m, w, calls = _model(monkeypatch, inline, prior_stems, precision, training)
    H, W, B = 8, 8, 2
    rms = torch.zeros(B, 1, 7, H, W)
    stems = [(rms[:, 0, i], 7 * H * W, slice(n * B, (n + 1) * B)) for n, i in enumerate(slots)]
    m._compensate(w, torch.zeros(3 * B, H, W, 64), stems, [3, 4, 5], [torch.zeros(B, 64, H, W)] * 3)
    stem_writes = [c for c in calls if c[0] in ("stem_conv", "stem_conv2")]
    if expect:      # no stem launch at all; _rdab gets the features themselves and the group's plane addressing
        assert stem_writes == [] and calls[-1] == ("rdab", (B, 7 * H * W, H * W))
    else:
        assert len(stem_writes) == 3 and calls[-1] == ("rdab", None)


def test_one_noise_for_several_stems_stays_materialised(monkeypatch):
    m, w, calls = _model(monkeypatch, True)
    H, W, B = 8, 8, 2
    rms = torch.zeros(B, 1, 7, H, W)
    stems = [(rms[:, 0, i], 7 * H * W, slice(n * B, (n + 1) * B)) for n, i in enumerate((4, 5, 6))]
    assert m._inline_rms_planes(w, torch.zeros(3 * B, H, W, 64), stems, 1) is None
    assert m._inline_rms_planes(w, torch.zeros(3 * B, H, W, 64), stems, 3)[1:] == (B, 7 * H * W, H * W)
    assert m._inline_rms_planes(w, torch.zeros(3 * B, 7, 9, 64), stems, 3) is None       # P % 64 != 0: outside the mask kernel's contract
    # compensate_features: ONE stem for F frames with a noise each -- inline whatever F is (results must not depend on the chunking)
    for F in (1, 4):
        one = [(torch.zeros(F, H, W), H * W, slice(0, F))]
        assert m._inline_rms_planes(w, torch.zeros(F, H, W, 64), one, F)[1:] == (F, H * W, 0)
