"""Host arithmetic of the partial slots of the persistent streaming kernels (cdfo_align_stats, the channel-sum output of the
1x1 streaming kernel): the tile stream of B images x ceil(P / 128) tiles is cut into `grid` contiguous ranges; a workgroup stores
its sums over its tiles of image b into slot (wg - first workgroup of b).  Checked here without a GPU, against a plain Python
restatement of the cut: the slot count covers every slot that is written, every (image, slot) has at most one writer, every
workgroup that holds tiles of an image has a slot, and bad arguments are refused before any HIP call."""
import ctypes as C

import pytest

SHAPES = [(1, 64 * 64), (3, 272 * 480), (24, 272 * 480), (5, 72 * 120), (24, 40 * 56), (2, 37 * 53), (520, 96), (1, 1), (7, 129),
          (256, 128), (257, 128), (300, 1000)]
GRIDS = [1, 2, 7, 64, 128, 255, 256, 304]


@pytest.fixture(scope="module")
def lib():
    from cdfo_amd import _lib
    from cdfo_amd.build import build
    build()
    return _lib.lib()


def _cut(B, P, grid):
    """{wg: set of images it holds tiles of} of the kernels' cut [tiles*w/grid, tiles*(w+1)/grid)"""
    tpi = (P + 127) // 128
    tiles = B * tpi
    g = min(tiles, grid)
    held = {}
    for w in range(g):
        t_lo, t_hi = tiles * w // g, tiles * (w + 1) // g
        if t_lo < t_hi:
            held[w] = list(range(t_lo // tpi, (t_hi - 1) // tpi + 1))
    return g, held


@pytest.mark.parametrize("B,P", SHAPES)
def test_every_image_slot_has_one_writer(lib, B, P):
    for grid in GRIDS:
        n = lib.cdfo_stream_slots_for_grid(B, C.c_longlong(P), grid)
        g, held = _cut(B, P, grid)
        assert 1 <= n <= (P + 127) // 128
        owners = {}
        for w in range(g):
            for b in held.get(w, []):
                s = lib.cdfo_stream_slot_of(B, C.c_longlong(P), grid, w, b)
                assert 0 <= s < n, (B, P, grid, w, b, s, n)
                assert (b, s) not in owners, (B, P, grid, w, b, s, owners[(b, s)])
                owners[(b, s)] = w
        # nobody else writes: a workgroup without a tile of image b has no slot there
        for w in range(0, g, max(1, g // 16)):
            for b in range(0, B, max(1, B // 16)):
                if b not in held.get(w, []):
                    assert lib.cdfo_stream_slot_of(B, C.c_longlong(P), grid, w, b) == -1
        # slots of an image are used from 0 upwards (the fold kernels sum nslots zero-initialised slots in index order)
        for b in range(B):
            used = sorted(s for (bb, s) in owners if bb == b)
            assert used == list(range(len(used))) and used
        assert max(s for (_, s) in owners) == n - 1              # the count is tight


def test_slot_count_at_the_benchmark_shape(lib):
    # 24 images of 272 x 480 on 256 workgroups: 1020 tiles per image, 95.6 tiles per workgroup -> 11 or 12 workgroups touch an image
    assert lib.cdfo_stream_slots_for_grid(24, C.c_longlong(272 * 480), 256) == 12
    assert lib.cdfo_stream_slots_for_grid(1, C.c_longlong(64 * 64), 256) == 32       # one tile per workgroup
    assert lib.cdfo_stream_slots_for_grid(520, C.c_longlong(96), 256) == 1           # whole images per workgroup


def test_bad_arguments_are_refused_without_a_gpu(lib):
    assert lib.cdfo_stream_slots_for_grid(0, C.c_longlong(128), 4) == -1
    assert lib.cdfo_stream_slots_for_grid(1, C.c_longlong(0), 4) == -1
    assert lib.cdfo_stream_slots_for_grid(1, C.c_longlong(128), 0) == -1
    assert lib.cdfo_stream_slot_of(2, C.c_longlong(128), 4, 0, 2) == -1
    p = C.c_void_p(256)
    args = lambda **kw: [kw.get("x0", p), kw.get("ld0", 64), p, 64, p, kw.get("ldq", 64), p, None, kw.get("act", 2), kw.get("ch", 16),
                         kw.get("B", 1), C.c_longlong(128), kw.get("n", 1), p, p, p, None]
    assert lib.cdfo_align_stats(*args(B=0)) == -1
    assert lib.cdfo_align_stats(*args(n=0)) == -1
    assert lib.cdfo_align_stats(*args(ch=12)) == -1
    assert lib.cdfo_align_stats(*args(act=3)) == -1                      # sigmoid is not an epilogue of the product
    assert lib.cdfo_align_stats(*args(ld0=62)) == -1
    assert lib.cdfo_align_stats(*args(ldq=32)) == -1
    assert lib.cdfo_align_stats(*args(x0=C.c_void_p(260))) == -2          # CDFO_EALIGN
