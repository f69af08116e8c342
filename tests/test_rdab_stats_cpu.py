"""Host side of the mask statistics kernel (`kernels.rdab_stats`): the predicate, the weight image, the header's prototype and
the path `CVSR_V8._compensate` selects.  No GPU: the kernels are replaced by recorders."""
import ctypes as C

import pytest
import torch

from cdfo_amd import _lib
from cdfo_amd import kernels as K


def test_predicate():
    assert K.rdab_stats_ok(272, 480) and K.rdab_stats_ok(2, 2)
    for H, W in ((271, 480), (272, 479), (0, 8), (8, 0), (1 << 15, 1 << 15)):
        assert not K.rdab_stats_ok(H, W), (H, W)


def test_odd_size_is_refused_before_the_library_is_touched():
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="even-sized"):
        K.rdab_stats(z, 1, 0, 0, 1, 9, 14, z, z, z, z)


def test_weight_image_layout():
    """[2][tap][k-step][k-half][out][8]: element j of a 16-byte group is input channel 16 c + 8 (j >> 2) + 4 h + (j & 3), the order of
    a 32x32 MFMA lane's accumulators; hi + lo reproduces the weight to bf16-squared precision"""
    g = torch.Generator().manual_seed(1)
    w2 = torch.randn(64, 64, 3, 3, generator=g)
    img = K.pack_rdab_stats(w2)
    assert img.dtype == torch.bfloat16 and tuple(img.shape) == (2, 9, 4, 2, 64, 8) and img.is_contiguous()
    assert img.numel() * 2 == 147456
    for (t, c, h, n, j) in ((0, 0, 0, 0, 0), (4, 2, 1, 37, 5), (8, 3, 1, 63, 7), (5, 1, 0, 9, 3)):
        v = w2[n, 16 * c + 8 * (j >> 2) + 4 * h + (j & 3), t // 3, t % 3]
        assert img[0, t, c, h, n, j] == v.to(torch.bfloat16)
        assert abs(float(img[0, t, c, h, n, j]) + float(img[1, t, c, h, n, j]) - float(v)) <= abs(float(v)) * 2.0 ** -15
    with pytest.raises(ValueError):
        K.pack_rdab_stats(w2[:, :32])


def test_header_declares_the_entry_point_and_the_conv_args_mirror_still_matches():
    protos = _lib.header_prototypes()
    restype, argtypes = protos["cdfo_rdab_stats"]
    assert restype is C.c_int and len(argtypes) == 14
    assert argtypes[:4] == [C.c_void_p, C.c_int, C.c_longlong, C.c_longlong] and argtypes[-1] is C.c_void_p
    names = [n for n, _ in _lib.header_conv_args_fields()]
    assert names == [n for n, _ in _lib.ConvArgs._fields_] and names[-2:] == ["chan_sum_out", "chan_sum_slots"]
    assert _lib.lib().cdfo_sizeof_conv_args() == C.sizeof(_lib.ConvArgs)


@pytest.mark.parametrize("on,precision,training,H,expect_new", [(True, "fp16x2", False, 8, True), (True, "bf16x3", False, 8, True),
                                                               (False, "fp16x2", False, 8, False), (True, "f32", False, 8, False),
                                                               (True, "fp16x2", True, 8, False), (True, "fp16x2", False, 7, False)])
def test_compensate_selects_the_path(monkeypatch, on, precision, training, H, expect_new):
    from arch.SIDECVSR_our import CVSR_V8
    m = CVSR_V8()
    m.prior_stems, m._precision, m.istraining = on, precision, training
    calls = []
    monkeypatch.setattr(K, "empty_act", lambda B, Hh, Ww, Cc, dev: torch.zeros(B, Hh, Ww, Cc))
    monkeypatch.setattr(K, "stem_conv", lambda *a, **kw: calls.append(("stem_conv", kw.get("write_out"))))
    monkeypatch.setattr(K, "stem_conv2", lambda *a, **kw: calls.append(("stem_conv2", kw.get("s2dB"))))
    monkeypatch.setattr(K, "rdab_stats", lambda img, Bi, s_b, s_g, B, *a, **kw: calls.append(("rdab_stats", Bi, s_b, s_g, B)) or ("part", 1, 25))
    monkeypatch.setattr(m, "_rdab", lambda w, du0, x, noises, stats=None: calls.append(("rdab", du0 is None, stats)) or x)
    monkeypatch.setattr(m, "_conv", lambda srcs, *a, **kw: srcs[0])
    W, B = 8, 2
    rms = torch.zeros(B, 1, 7, H, W)
    stems = [(rms[:, 0, i], 7 * H * W, slice(n * B, (n + 1) * B)) for n, i in enumerate((4, 5, 6))]
    z = torch.zeros(1)
    w = {"raw": {"conv_expand_rms.weight": z, "conv_expand_rms.bias": z, "RDAB.conv_du_re.2.bias": z}, "rms_du0": (z, z),
         "RDAB.conv_du_re.2_stats": z, "conv_expand_fea_r": None}
    m._compensate(w, torch.zeros(3 * B, H, W, 64), stems, [3, 4, 5], [torch.zeros(B, 64, H, W)] * 3)
    if expect_new:      # one statistics launch for the three slots through the plane strides; the stem writes fea_com only
        assert calls == [("rdab_stats", B, 7 * H * W, H * W, 3 * B)] + [("stem_conv", False)] * 3 + [("rdab", True, ("part", 1, 25))]
    else:
        assert calls == [("stem_conv2", True)] * 3 + [("rdab", False, None)]
