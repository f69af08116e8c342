"""Every persistent trunk kernel under a limited CU share (`kernels.cu_limit`), at the (shape, limit) pairs of
tests/schedule_cases.py -- whose walks (two and three units per workgroup, empty workgroups, image and output-block changes inside a
walk, ragged last tiles) tests/test_schedule_cases_cpu.py pins down without a GPU.

Inputs, references and bounds are those of the per-kernel parity tests: a case CALLS the existing test function with the table's shape
inside `with K.cu_limit(L)`, so every assertion of that test holds under the limit, at its own bound.  The wrappers' results are
recorded on the way and compared bit for bit (`torch.equal`) with the results of the same call without a limit, wherever the limit
does not change which kernel form runs.  From the code, per kernel:

  conv_ring (dense, four-tap, split)  equal: a unit's result is a function of (image, tile, block) alone -- one workgroup computes the
                      whole K loop of a tile in chunk order; the limit only changes which workgroup gets the unit.
  conv3x3_ws, _ws_res, conv_offset_mask_ws   equal while the form is the same (ring-fed / private halo: the accumulation order of a
                      pixel is chunk-major in both, but the MFMA shapes differ: 16x16 against 32x32).  Cout = 128 at L = 8 flips to
                      the private-halo form (2 blocks > 8 / 8): reference only.
  conv3x3_wino, _wino_up2   equal although the segment height follows the share: an output row's accumulator is opened by input row
                      y - 1 (dy = 0), continued by row y and closed by row y + 1, K halves in order, at every position of the row
                      inside a batch or a segment, in the guarded and in the straight-line code (conv3x3_wino.hip: `row`, and the
                      guarded loop behind it).
  conv3x3_n16, block_prologue, qkv_dw (192-channel form), conv on the streaming 1x1 path   equal: one workgroup per tile, fixed order.
  qkv_dw(gram=True)   v equal; the Gram partials are regrouped: their slot sums against float64 at the existing bound, n = the
                      restated slot count, slots beyond those the restated walk uses exactly zero.
  conv(chan_sum_out=True)   the result equal; the channel-sum partials as the Gram partials.
  align_stats         every output is a partial sum: slot sums against float64 at the existing bound (4 x the replaced path), n and
                      the unused slots as above."""
import pytest
import torch

import schedule_cases as S

gpu = pytest.mark.gpu
_UNLIMITED = {}        # (kernel, form, shape) -> (recorded results, largest error / bound) of the call without a limit


class _Recorder:
    """wraps attributes of cdfo_amd.kernels: every call's tensor results (and named in-place operands) are cloned into .calls"""

    def __init__(self, monkeypatch, names, inplace=()):
        from cdfo_amd import kernels as K
        self.calls = []
        for name in names:
            monkeypatch.setattr(K, name, self._wrap(getattr(K, name), inplace))

    def _wrap(self, fn, inplace):
        def wrapped(*a, **kw):
            r = fn(*a, **kw)
            outs = list(r) if isinstance(r, tuple) else [r]
            outs += [a[i] for i in inplace]
            outs += [kw[k] for k in ("out2_cp16",) if kw.get(k) is not None]
            self.calls.append([o.clone() if isinstance(o, torch.Tensor) else o for o in outs])
            return r
        return wrapped


def _ratio_hooks(monkeypatch, sink):
    """error / bound of every assertion that the re-run tests make through their modules' bound helpers (test_gpu_conv._le and _cmp,
    which calls it; test_gpu_attention._lt; test_gpu_align_stats._le; test_gpu_dcn_modules._lt) is appended to `sink`"""
    import test_gpu_align_stats as TS
    import test_gpu_attention as TA
    import test_gpu_conv as TC
    import test_gpu_dcn_modules as TD
    for mod, name in ((TC, "_le"), (TA, "_lt"), (TS, "_le"), (TD, "_lt")):
        def hook(err, bound, what, real=getattr(mod, name)):
            sink.append(err / bound)
            real(err, bound, what)
        monkeypatch.setattr(mod, name, hook)


def _forms(kernel, shape):
    """{form: (callable, wrapper names to record, positions of in-place result operands)} of one table kernel"""
    import test_gpu_align_stats as TS
    import test_gpu_attention as TA
    import test_gpu_conv as TC
    import test_gpu_dcn_modules as TD
    from cdfo_amd import kernels as K
    if kernel == "ring":
        B, H, W, Cout = shape
        forms = {"dense": (lambda: TC.test_conv3x3_ring_dense(64, Cout, H, W, B, True, False), ["conv_ring"], ())}
        if Cout == 64:
            forms.update({
                "four_tap_residuals": (lambda: TC.test_conv3x3_ring_sparse_taps_with_residuals(B, H, W), ["conv_ring"], ()),
                "half_resolution_residual": (lambda: TC.test_conv3x3_ring_half_resolution_residual(B, H, W), ["conv_ring"], ()),
                "out2_chunk_planar": (lambda: TC.test_conv3x3_ring_second_output_chunk_planar(B, H, W), ["conv_ring"], ()),
                "halfsplit_source": (lambda: TC.test_conv3x3_ring_sparse_taps_halfsplit_source(B, H, W), ["conv_ring"], ())})
        return forms
    if kernel == "ws_plain":
        B, H, W, Cout = shape
        return {"plain": (lambda: TC.test_conv3x3_c64_ws(Cout, H, W, B, False, 1), ["conv3x3_ws"], ()),
                "s2d": (lambda: TC.test_conv3x3_c64_ws(Cout, H, W, B, True, 1), ["conv3x3_ws"], ())}
    if kernel == "ws_res":
        return {"res": (lambda: TC.test_conv3x3_ws_residual_form(*shape, True), ["conv3x3_ws_res"], ())}
    if kernel == "offmask":
        return {"offmask": (lambda: TD.test_offset_head_with_the_assembly_as_its_epilogue(shape, "fp16x2"), ["conv_offset_mask_ws"], (2, 3))}
    if kernel == "wino":
        B, H, W, Cout = shape
        return {"wino": (lambda: TC.test_conv3x3_c64_wino(Cout, H, W, B, False, 1), ["conv3x3_wino"], ())}
    if kernel == "wino_up2":
        B, h, w, Cout = shape
        return {"up2": (lambda: TC.test_conv3x3_c64_wino_up2(Cout, h, w, B, 1), ["conv3x3_wino_up2"], ())}
    B, H, W = shape
    if kernel == "n16":
        return {"n16": (lambda: TC.test_conv3x3_n16_matches_fp64_conv(B, H, W, 1), ["conv3x3_n16"], ())}
    if kernel == "block_pro":
        return {"prologue": (lambda: TC.test_block_prologue(B, H, W), ["block_prologue"], ())}
    if kernel in ("qkv_tiled", "qkv_gram"):
        return {"qkv": (lambda: TA.test_qkv_dw_fused(B, H, W), ["qkv_dw"], ())}
    if kernel == "align_stats":
        return {"stats": (lambda: TS.test_align_stats_against_float64(B, H, W, False), ["align_stats"], ())}
    if kernel == "stream":
        many = TC.test_conv1x1_stream_many_tiles_across_images
        return {"one_source_per_image_weights_two_residuals": (lambda: many([64], 64, 2, True, shape), ["conv"], ()),
                "two_sources_one_residual": (lambda: many([64, 64], 64, 1, False, shape), ["conv"], ()),
                "two_output_blocks": (lambda: many([64], 128, 0, False, shape), ["conv"], ()),
                "fp16x2": (lambda: many([64, 64], 64, 1, False, shape, K.PREC_FP16X2), ["conv"], ()),
                "ln_out": (lambda: TC.test_conv1x1_with_layernorm_planes_of_the_result(B, H, W), ["conv"], ()),
                "chan_sum_out": (lambda: TS.test_stream_kernel_channel_sums(B, H, W, 1), ["conv"], ())}
    raise KeyError(kernel)


def _device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _same_form(kernel, shape, limit, dev):
    if kernel == "ws_plain":
        import os
        ring = os.environ.get("CDFO_WS_RING", "1") != "0"   # 0 (tests/test_gpu_kernel_variants.py): the private-halo form at every share
        return S.ws_form(shape[3], min(limit, dev), ring) == S.ws_form(shape[3], dev, ring)
    return True


def _used_slots(kernel, shape, cus):
    """{image: slots the restated walk writes}, restated slot count"""
    B, H, W = shape
    walks, _ = S.walks_of(kernel, shape, cus)
    if kernel == "qkv_gram":
        n, slot_of = S.qkv_gram_slots(B, H, W, cus), lambda wg, b: S.qkv_gram_slot_of(B, H, W, cus, wg, b)  # noqa: E731
    else:
        n, slot_of = S.stream_slots(B, H * W, cus), lambda wg, b: S.stream_slot_of(B, H * W, cus, wg, b)  # noqa: E731
    used = {b: set() for b in range(B)}
    for wg, w in enumerate(walks):
        for b in {u[0] for u in w}:
            used[b].add(slot_of(wg, b))
    return used, n


def _check_partials(kernel, shape, cus, part, n):
    """n is the restated count; slots the restated walk does not write are exactly zero, the written ones are not all zero"""
    used, want_n = _used_slots(kernel, shape, cus)
    assert n == want_n and part.shape[1] == n, (kernel, shape, cus, n, want_n)
    for b, slots in used.items():
        for s in range(n):
            if s in slots:
                assert bool((part[b, s] != 0).any()), (kernel, shape, cus, b, s)
            else:
                assert bool((part[b, s] == 0).all()), (kernel, shape, cus, b, s)


@gpu
@pytest.mark.parametrize("kernel,shape,limit", S.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_under_a_cu_limit(kernel, shape, limit, monkeypatch):
    from cdfo_amd import kernels as K
    dev = _device_cus()
    cus = min(limit, dev)
    if kernel == "offmask" and dev < 56:
        pytest.skip("conv_offset_mask_ws takes no share below 56 CUs (7 output blocks): this device has fewer")
    assert S.walks_of(kernel, shape, cus)[0] is not None, "the table holds no launch that the wrapper refuses"
    for form, (call, names, inplace) in _forms(kernel, shape).items():
        key = (kernel, form, shape)
        if key not in _UNLIMITED:
            rec, ratios = _Recorder(monkeypatch, names, inplace), []
            _ratio_hooks(monkeypatch, ratios)
            call()
            torch.cuda.synchronize()
            _UNLIMITED[key] = (rec.calls, max(ratios, default=None))
            monkeypatch.undo()
        rec, ratios = _Recorder(monkeypatch, names, inplace), []
        _ratio_hooks(monkeypatch, ratios)
        with K.cu_limit(limit):
            call()                                   # the per-kernel test's own references and bounds, under the limit
            torch.cuda.synchronize()
        monkeypatch.undo()
        free, free_ratio = _UNLIMITED[key]
        assert len(rec.calls) == len(free) and rec.calls
        assert (free_ratio is None) == (not ratios)
        if ratios:                                   # (forms whose test asserts equalities only have none)
            print(f"schedule ratio {kernel} {form} {'x'.join(map(str, shape))} L={limit}: error / bound {max(ratios):.3f} (no limit: {free_ratio:.3f})")
        stats_kernel = kernel in ("qkv_gram", "qkv_tiled", "align_stats") or form == "chan_sum_out"
        for got, want in zip(rec.calls, free):
            if kernel == "align_stats":              # (gram, s0, s1, n): partial sums only
                for part in got[:3]:
                    _check_partials(kernel, shape, cus, part, got[3])
                continue
            if stats_kernel and len(got) == 3 and isinstance(got[2], int):      # (result, partials, n)
                assert torch.equal(got[0], want[0]), f"{kernel} {form}: result differs from the unlimited launch"
                _check_partials("qkv_gram" if kernel.startswith("qkv") else "stream", shape, cus, got[1], got[2])
                continue
            if not _same_form(kernel, shape, limit, dev):
                continue                             # another kernel form under the limit: reference only
            for g, w in zip(got, want):
                if isinstance(g, torch.Tensor):
                    assert torch.equal(g, w), f"{kernel} {form} {shape} L={limit}: differs from the unlimited launch"


@gpu
def test_a_share_below_the_minimum_is_refused_before_the_launch():
    """cus < 8 in the ws, ring and Winograd wrappers (and fewer than 8 CUs per output block in conv_offset_mask_ws and the Winograd
    kernel) return CDFO_EINVAL; the limit is back after the block, also when the body raises."""
    from cdfo_amd import _lib
    from cdfo_amd import kernels as K
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 8, 16, 64, generator=g).cuda()
    pc = K.pack_conv((torch.randn(128, 64, 3, 3, generator=g) / 24).cuda(), torch.randn(128, generator=g).cuda())
    src = K.to_cp16(x)
    res = torch.zeros(1, 8, 16, 128, device="cuda")
    before = _lib.lib().cdfo_set_cu_limit(0)
    _lib.lib().cdfo_set_cu_limit(before)
    calls = [lambda: K.conv_ring(src, pc), lambda: K.conv3x3_ws(src, pc), lambda: K.conv3x3_ws_res(src, pc, res1=res),
             lambda: K.conv3x3_wino(src, pc)]
    for call in calls:
        with pytest.raises(_lib.CdfoError):
            with K.cu_limit(4):
                call()
        assert _lib.lib().cdfo_set_cu_limit(before) == before          # restored although the body raised
    with pytest.raises(_lib.CdfoError):
        with K.cu_limit(8):                                            # each 128-channel half needs 8 CUs: 256 channels need 16
            K.conv3x3_wino(src, K.pack_conv((torch.randn(256, 64, 3, 3, generator=g) / 24).cuda(), None))
    # conv_offset[2]: 27 x 16 = 432 -> 448 padded channels = 7 blocks of the ring-fed kernel, 8 CUs each
    pc_om = K.pack_conv((torch.randn(432, 64, 3, 3, generator=g) / 24).cuda(), torch.zeros(432, device="cuda"))
    off, msk, flow = (torch.zeros(1, c, 8, 16, device="cuda") for c in (288, 144, 2))
    for share in (4, 48):
        with pytest.raises(_lib.CdfoError):
            with K.cu_limit(share):
                K.conv_offset_mask_ws(src, pc_om, off, msk, flow, 10.0, False)
        assert _lib.lib().cdfo_set_cu_limit(before) == before
    with K.cu_limit(8):
        inside = _lib.lib().cdfo_set_cu_limit(8)
        out = K.conv_ring(src, pc)
    assert inside == 8 and _lib.lib().cdfo_set_cu_limit(before) == before
    torch.cuda.synchronize()
    assert torch.equal(out, K.conv_ring(src, pc))
    with K.cu_limit(3):                                                # kernels without a minimum take any share
        y = K.conv3x3_n16(x, K.pack_conv_n16(torch.randn(16, 64, 3, 3, generator=g).cuda()), None)
    assert tuple(y.shape) == (1, 8, 16, 16)
