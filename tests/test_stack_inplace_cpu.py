"""Host side of `model.stack_inplace` (CDFO_STACK_INPLACE): the image map helper's addresses, the predicate that selects the in-place
neighbour phase, the entry points' prototypes and the size of cdfo_conv_args (which did not grow).  No GPU."""
import ctypes as C

import pytest
import torch

from cdfo_amd import _lib
from cdfo_amd import kernels as K


def _stack(B, H, W, ld=64):
    """a clip-major stack [B,7,H,W,ld] whose every float is its own index"""
    return torch.arange(B * 7 * H * W * ld, dtype=torch.float32).view(B, 7, H, W, ld)


@pytest.mark.parametrize("B,G,ld", [(1, 1, 64), (2, 3, 64), (3, 3, 80), (8, 3, 64)])
def test_map_addresses_agree_with_torch_indexing(B, G, ld):
    """the three shapes of the map over a clip-major stack (clips 7 P ld apart, frames P ld apart)"""
    H, W, i0 = 4, 6, 4
    st = _stack(B, H, W, ld)
    P = H * W
    first = st[0, i0, :, :, :64]
    # a group's frames i0 .. i0 + G - 1, neighbour major
    m = K.image_map(first, G * B, B, 7 * P * ld, P * ld)
    assert m.shape == (G * B, H, W, 64) and m.ld == ld and m.data_ptr() == first.data_ptr() and m.triple() == (B, 7 * P * ld, P * ld)
    for g in range(G):
        for b in range(B):
            k = g * B + b
            assert first.storage_offset() + m.offset(k) == st[b, i0 + g].storage_offset()
            assert torch.equal(m.image(k), st[b, i0 + g, :, :, :64])
    assert torch.equal(m.dense(), torch.stack([st[b, i0 + g, :, :, :64] for g in range(G) for b in range(B)]))
    # one frame of every clip
    m1 = K.image_map(first, B, B, 7 * P * ld, 0)
    assert torch.equal(m1.dense(), st[:, i0, :, :, :64])
    # ... once per neighbour of a group (what `repeat` wrote)
    mr = K.image_map(first, G * B, B, 7 * P * ld, 0)
    assert torch.equal(mr.dense(), st[:, i0, :, :, :64].repeat(G, 1, 1, 1))
    # a neighbour's images of the group as a map of their own
    for g in range(G):
        assert torch.equal(m.sub(g * B, B).dense(), st[:, i0 + g, :, :, :64])
    if B > 1:
        with pytest.raises(ValueError):
            m.sub(1, 1)


def test_frame_major_stack_uses_the_same_form_with_its_own_strides():
    from cdfo_amd.cvsr_v8 import _FeatureStack
    Kw, H, W = 3, 4, 6
    Lf = torch.arange(7 * Kw * H * W * 64, dtype=torch.float32).view(7, Kw, H, W, 64)
    fs = _FeatureStack(Lf, Kw, H, W, Kw * H * W * 64, H * W * 64)
    assert torch.equal(fs.group(4, 3).dense(), Lf[4:7].reshape(3 * Kw, H, W, 64))
    assert torch.equal(fs.frame(3).dense(), Lf[3])
    assert torch.equal(fs.frame(3, times=3).dense(), Lf[3].repeat(3, 1, 1, 1))
    L1 = torch.arange(Kw * 7 * H * W * 64, dtype=torch.float32).view(Kw * 7, H, W, 64)         # clip-major, as the extractor writes
    fs = _FeatureStack(L1, Kw, H, W, H * W * 64, 7 * H * W * 64)
    v = L1.view(Kw, 7, H, W, 64)
    assert torch.equal(fs.group(0, 3).dense(), v[:, 0:3].transpose(0, 1).reshape(3 * Kw, H, W, 64))
    assert torch.equal(fs.frame(3, times=2).dense(), v[:, 3].repeat(2, 1, 1, 1))


def test_map_helper_refuses_what_no_kernel_can_read():
    st = _stack(2, 4, 6)
    first = st[0, 3]
    P = 24
    with pytest.raises(ValueError, match="storage"):
        K.image_map(first, 3, 3, 7 * P * 64, 0)                 # a third clip
    with pytest.raises(ValueError, match="storage"):
        K.image_map(st[0, 5], 6, 2, 7 * P * 64, P * 64)         # frames 5, 6, 7
    with pytest.raises(ValueError, match="multiples of 4"):
        K.image_map(first, 2, 2, 7 * P * 64 + 1, 0)
    with pytest.raises(ValueError, match="multiples of 4"):
        K.image_map(first, 2, 0, 7 * P * 64, 0)
    with pytest.raises(ValueError, match="multiples of 4"):
        K.image_map(first, 2, 2, -4, 0)
    with pytest.raises(ValueError):
        K.image_map(first[:, :, :32], 2, 2, 7 * P * 64, 0)      # fewer than 64 channels
    with pytest.raises(ValueError):
        K.image_map(first.double(), 2, 2, 7 * P * 64, 0)
    with pytest.raises(ValueError):
        K.image_map(first[::2], 2, 2, 7 * P * 64, 0)            # rows not dense at the pixel pitch


def test_header_declares_the_entry_points_and_the_argument_block_did_not_grow():
    protos = _lib.header_prototypes()
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    assert protos["cdfo_conv3x3_bf16_map"] == (C.c_int, [vp, i, ll, ll, vp])
    assert protos["cdfo_conv1x1_bf16x3_map"] == (C.c_int, [vp, vp] + protos["cdfo_conv1x1_bf16x3_plane"][1][1:])
    assert protos["cdfo_conv1x1_map_ok"] == (C.c_int, [i, i, i, i])
    base = protos["cdfo_conv3x3_c64_ws_res"][1]
    assert protos["cdfo_conv3x3_c64_ws_res_map"][1] == base[:15] + [i, ll, ll] + base[15:]
    base = protos["cdfo_rdab_prep_fused_plane"][1]
    assert protos["cdfo_rdab_prep_fused_plane_map"][1] == base[:2] + [i, ll, ll] + base[2:]
    a, p = protos["cdfo_align_stats"][1], protos["cdfo_align_stats_plane"][1]
    assert protos["cdfo_align_stats_map"][1] == a[:6] + [i, ll, ll] + a[6:-1] + p[14:]
    lib = _lib.lib()
    assert lib.cdfo_sizeof_conv_args() == C.sizeof(_lib.ConvArgs) == 392      # what it was before the maps: they travel beside it
    assert [n for n, _ in _lib.ConvArgs._fields_][-2:] == ["chan_sum_out", "chan_sum_slots"]


def test_one_by_one_map_contract_is_host_arithmetic():
    # the streaming kernel holds up to 192 input channels beside its rings; beyond it only plain products of mapped sources
    assert K.conv1x1_map_ok(128, plane=True, res=True) and K.conv1x1_map_ok(128, plane=True, chan_sum=True)
    assert K.conv1x1_map_ok(192, chan_sum=True) and K.conv1x1_map_ok(448)
    assert not K.conv1x1_map_ok(448, res=True) and not K.conv1x1_map_ok(448, chan_sum=True) and not K.conv1x1_map_ok(448, plane=True)
    assert not K.conv1x1_map_ok(96)


def _model(precision="fp16x2", training=False, **switches):
    from arch.SIDECVSR_our import CVSR_V8
    m = CVSR_V8()
    m._precision, m.istraining = precision, training
    for k, v in switches.items():
        assert hasattr(m, k)
        setattr(m, k, v)
    z = torch.zeros(1)
    one = lambda cin, ks=1, **kw: K.PackedConv(z, None, 64, cin, ks, 64, **kw)
    w = {"rms_chunk": z, "ufs_chunk": z, "RDAB.fuse": one(128), "tsa_fusion": one(448),
         "conv_expand_fea_r": one(128, 3, wq=z, wh=z, CoutP16=64)}
    for n in ("ResidualBlock.conv1", "ResidualBlock.conv2", "ResidualBlock1.conv1", "ResidualBlock1.conv2"):
        w["MV_deform_align." + n] = one(64, 3, wq=z, wh=z, CoutP16=64)
    return m, w


def test_predicate_selects_the_in_place_path():
    m, w = _model()
    assert m.stack_inplace                                     # the row's default
    for B, H, W in ((1, 8, 8), (2, 24, 40), (8, 272, 480)):
        assert m._stack_inplace(w, B, H, W)
    # the switch, exact-fp32 arithmetic, training
    assert not _model(stack_inplace=False)[0]._stack_inplace(w, 2, 24, 40)
    assert not _model(precision="f32")[0]._stack_inplace(w, 2, 24, 40)
    assert not _model(training=True)[0]._stack_inplace(w, 2, 24, 40)
    # a reader that takes no map in the form this forward runs it in
    assert not _model(precision="bf16x3")[0]._stack_inplace(w, 2, 24, 40)          # the last residual on the tiled 3x3 kernel's epilogue
    assert not _model(rdab_fused=False)[0]._stack_inplace(w, 2, 24, 40)            # the mask kernel's two-launch form
    assert not _model(inline_rms=False)[0]._stack_inplace(w, 2, 24, 40)            # the mask kernel without its plane
    assert not _model(prior_stems=False)[0]._stack_inplace(w, 2, 24, 40)
    assert not _model(align_stats=False)[0]._stack_inplace(w, 2, 24, 40)           # gram_partial reads xc
    assert not _model(fea_r_single_pass=True)[0]._stack_inplace(w, 2, 24, 40)      # conv_expand_fea_r on the single-pass form
    assert _model(inline_ufs=False)[0]._stack_inplace(w, 2, 24, 40)                # pred in memory: the 192 -> 64 form takes the map too
    assert not m._stack_inplace(w, 2, 23, 40)                                      # odd height: the ResidualBlocks leave the Block_ kernels
    assert not m._stack_inplace(w, 2, 6, 10)                                       # P % 64 != 0: the mask kernel's two-launch form
    w2 = dict(w)
    w2["MV_deform_align.ResidualBlock1.conv2"] = K.PackedConv(torch.zeros(1), None, 64, 64, 3, 64)
    assert not m._stack_inplace(w2, 2, 24, 40)


def test_predicate_refuses_when_a_consumer_refuses(monkeypatch):
    m, w = _model()
    for name in ("rdab_prep_fused_map_ok", "conv_map_ok", "conv1x1_map_ok", "ws_res_map_ok"):
        with monkeypatch.context() as mp:
            mp.setattr(K, name, lambda *a, **kw: False)
            assert not m._stack_inplace(w, 2, 24, 40)
    assert m._stack_inplace(w, 2, 24, 40)


def test_front_takes_the_parents_path_without_the_predicate(monkeypatch):
    """_fuse_windows with the predicate false: swap_outer's frame-major tensor is sliced and the centre repeated, as before"""
    m, w = _model(stack_inplace=False)
    B, H, W = 2, 8, 8
    Lf = torch.arange(7 * B * H * W * 64, dtype=torch.float32).view(7, B, H, W, 64)
    seen = {}

    def fork_join(device, nstr, groups, deferred_new, body):
        seen["groups"] = groups
        return {}

    def neighbour_group(w_, Lf_, idxs, xcG, *a):
        raise AssertionError("not reached: _fork_join is a recorder")
    monkeypatch.setattr(m, "_fork_join", fork_join)
    monkeypatch.setattr(m, "_neighbour_group", neighbour_group)
    monkeypatch.setattr(m, "_fuse", lambda w_, centre, aligned: seen.setdefault("centre", centre))
    z = torch.zeros(B, 1, 7, H, W)
    m._fuse_windows(w, Lf, torch.zeros(B, 7, 1, H, W), torch.zeros(B, 7, 2, H, W), z, z, None)
    assert isinstance(seen["centre"], torch.Tensor) and torch.equal(seen["centre"], Lf[3])
    m.stack_inplace = True
    seen.clear()
    m._fuse_windows(w, Lf, torch.zeros(B, 7, 1, H, W), torch.zeros(B, 7, 2, H, W), z, z, None)
    assert isinstance(seen["centre"], K.ImageMap) and torch.equal(seen["centre"].dense(), Lf[3])


def test_isa_diff_by_kernel_ignores_label_numbers_and_added_instantiations():
    """tools/isa_diff.py --by-kernel: the check behind "every existing instantiation keeps its instructions" when a file gains kernels"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from isa_diff import missing_kernels
    old = "k1:    ; @k1\n\ts_nop 0\n.LBB0_1:    ; in Loop: Header=BB0_1\n\ts_branch .LBB0_1\n.Lfunc_end0:\n"
    new = ("k0:    ; @k0\n\ts_endpgm\n.Lfunc_end0:\n"
           "k1_renamed:    ; @k1_renamed\n\ts_nop 0\n.LBB1_1:    ; in Loop: Header=BB1_1\n\ts_branch .LBB1_1\n.Lfunc_end1:\n")
    assert missing_kernels(old, new) == ([], 1, 1)
    assert missing_kernels(old, new.replace("s_nop 0", "s_nop 1")) == (["k1"], 1, 2)
