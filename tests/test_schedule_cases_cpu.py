"""The case table of tests/schedule_cases.py really produces the walks it was written for -- checked without a GPU, for device CU
counts 256, 304, 64 and 32 (the effective share of a case is min(limit, device CUs)):
  (a) every unit of a launch is walked exactly once;
  (b) per kernel, the table reaches walk lengths 0, 1, 2, 3 and >= 5, a walk that crosses an image boundary, one that changes
      output block, and one that ends on the image's ragged corner tile -- except what schedule_cases.UNREACHABLE names, with the
      reason, as impossible for that kernel's scheme;
  (c) the restated slot counts bound the partial slots that the restated walks use, every (image, slot) has one writer, and the
      restatement agrees with the library's own host arithmetic (cdfo_stream_slots_for_grid / cdfo_stream_slot_of).
A (shape, limit) pair of the GPU test that does not give its intended walk fails here."""
import ctypes as C

import pytest

import schedule_cases as S

KERNELS = sorted({S.kernel_key(k, s, min(L, d)) for k, s, L in S.CASES for d in S.DEVICE_CUS})
PROPS = ("len0", "len1", "len2", "len3", "len5", "image", "block", "ragged")


def _props(kernel, shape, cus, walks):
    got = set()
    for w in walks:
        n = len(w)
        got.add({0: "len0", 1: "len1", 2: "len2", 3: "len3"}.get(n, "len5" if n >= 5 else "len4"))
        if any(a[0] != b[0] for a, b in zip(w, w[1:])):
            got.add("image")
        if any(a[2] != b[2] for a, b in zip(w, w[1:])):
            got.add("block")
        if w and S.ragged_last(kernel, shape, cus, w[-1]):
            got.add("ragged")
    return got


@pytest.mark.parametrize("dev", S.DEVICE_CUS)
@pytest.mark.parametrize("kernel,shape,limit", S.CASES + [(k, s, None) for k, s, _ in S.CASES[::3]])
def test_every_unit_is_walked_exactly_once(kernel, shape, limit, dev):
    cus = dev if limit is None else min(limit, dev)
    walks, units = S.walks_of(kernel, shape, cus)
    if walks is None:                     # the wrapper refuses this share: only conv_offset[2]'s 7 blocks on fewer than 56 CUs
        assert kernel == "offmask" and cus < 56
        return
    flat = [u for w in walks for u in w]
    assert len(flat) == units and len(set(flat)) == units
    B = shape[0]
    assert {u[0] for u in flat} == set(range(B))
    per_image = {}
    for b, t, nb in flat:
        per_image.setdefault((b, nb), []).append(t)
    first = sorted(per_image[(0, 0)])
    assert first == list(range(len(first)))                       # tile indices 0 .. n - 1, the same for every image and block
    assert all(sorted(v) == first for v in per_image.values())


@pytest.mark.parametrize("dev", S.DEVICE_CUS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_table_reaches_every_targeted_walk(kernel, dev):
    reached = set()
    for k, shape, limit in S.CASES:
        cus = min(limit, dev)
        if S.kernel_key(k, shape, cus) != kernel:
            continue
        walks, _ = S.walks_of(k, shape, cus)
        if walks is not None:
            reached |= _props(k, shape, cus, walks)
    if kernel == "offmask" and dev < 56:
        assert not reached                                         # every launch refused (S.UNREACHABLE)
        return
    want = set(PROPS) - S.UNREACHABLE[kernel]
    print(f"{kernel} on {dev} CUs reaches {sorted(reached & set(PROPS))}")
    assert want <= reached, f"{kernel} on {dev} CUs: not reached: {sorted(want - reached)}"
    if "block" in S.UNREACHABLE[kernel]:
        assert "block" not in reached                              # the comment in schedule_cases.py is checked, too


def test_the_issue_s_hand_derived_walks():
    """3 x 40 x 70 on the banded kernels: 4 / 3 / 0 at 8 CUs, 2 (2 + 1 on XCD 6) at 16, 2 / 1 / 1 at 24; 2 x 48 x 100 x 128 at 8: 6, alternating."""
    lens = lambda ws: [len(w) for w in ws]  # noqa: E731
    assert lens(S.ring_walks(3, 40, 70, 64, 8)) == [4, 4, 4, 4, 4, 4, 3, 0]
    assert lens(S.ring_walks(3, 40, 70, 64, 16)) == [2] * 6 + [2, 0] + [2] * 6 + [1, 0]
    assert lens(S.ring_walks(3, 40, 70, 64, 24)) == [2] * 6 + [1, 0] + [1] * 7 + [0] + [1] * 7 + [0]
    assert lens(S.wsq_walks(3, 40, 70, 64, 8)) == [4, 4, 4, 4, 4, 4, 3, 0]
    assert lens(S.wsq_walks(3, 48, 100, 64, 8)) == [5] * 7 + [1]                                    # ring-fed ws kernel: 36 tiles, band 5
    off = S.walks_of("offmask", (4, 40, 72), 56)[0]                                                # 7 blocks x 8 XCDs, one workgroup each
    assert lens(off) == ([5] * 7 + [1]) * 7 and S.walks_of("offmask", (4, 40, 72), 48)[0] is None
    w = S.ring_walks(2, 48, 100, 128, 8)
    assert lens(w) == [6] * 8 and [u[2] for u in w[3]] == [0, 1, 0, 1, 0, 1]
    assert S.ring_walks(3, 40, 70, 64, 8)[2] == [(0, 8, 0), (1, 0, 0), (1, 1, 0), (1, 2, 0)]      # band 2 crosses into image 1
    assert S.ring_walks(3, 40, 70, 64, 4) is None and S.ws_walks(3, 40, 70, 64, 7) is None          # cus < 8: refused
    assert S.ws_form(128, 8) == "ws" and S.ws_form(128, 16) == "wsq" and S.ws_form(64, 8) == "wsq"


SLOT_CASES = [(k, s, L) for k, s, L in S.CASES if k in ("stream", "align_stats", "qkv_gram")]


@pytest.mark.parametrize("dev", S.DEVICE_CUS)
@pytest.mark.parametrize("kernel,shape,limit", SLOT_CASES)
def test_slot_counts_bound_the_slots_a_schedule_uses(kernel, shape, limit, dev):
    cus = min(limit, dev)
    B, H, W = shape
    walks, _ = S.walks_of(kernel, shape, cus)
    if kernel == "qkv_gram":
        n, slot_of = S.qkv_gram_slots(B, H, W, cus), lambda wg, b: S.qkv_gram_slot_of(B, H, W, cus, wg, b)  # noqa: E731
    else:
        n, slot_of = S.stream_slots(B, H * W, cus), lambda wg, b: S.stream_slot_of(B, H * W, cus, wg, b)  # noqa: E731
    writers = {}
    for wg, w in enumerate(walks):
        for b in sorted({u[0] for u in w}):
            s = slot_of(wg, b)
            assert 0 <= s < n, (kernel, shape, cus, wg, b, s, n)
            assert (b, s) not in writers
            writers[(b, s)] = wg
    for b in range(B):                                            # used from 0 upwards: the folds add n slots in index order
        used = sorted(s for (bb, s) in writers if bb == b)
        assert used and used == list(range(len(used)))
    if kernel != "qkv_gram":
        assert max(s for _, s in writers) == n - 1                # the stream kernels' count is tight (qkv_dw's has one to spare)


@pytest.fixture(scope="module")
def lib():
    from cdfo_amd import _lib
    from cdfo_amd.build import build
    build()
    return _lib.lib()


@pytest.mark.parametrize("dev", S.DEVICE_CUS)
def test_restated_stream_slots_are_the_library_s(lib, dev):
    for kernel, (B, H, W), limit in SLOT_CASES:
        if kernel == "qkv_gram":
            continue
        cus, P = min(limit, dev), H * W
        assert lib.cdfo_stream_slots_for_grid(B, C.c_longlong(P), cus) == S.stream_slots(B, P, cus)
        for wg, w in enumerate(S.stream_walks(B, P, cus)):
            for b in range(B):
                want = S.stream_slot_of(B, P, cus, wg, b) if any(u[0] == b for u in w) else -1
                assert lib.cdfo_stream_slot_of(B, C.c_longlong(P), cus, wg, b) == want
