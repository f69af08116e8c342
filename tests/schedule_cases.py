"""The tile walks of the persistent trunk kernels, restated in plain Python from the kernels' own index arithmetic, and the table of
(kernel, shape, CU limit) cases that tests/test_gpu_schedules.py runs.

Every hot-path kernel launches a grid sized from cdfo_num_cus() (= min(device CUs, cdfo_set_cu_limit)) and each workgroup walks a
list of units.  A function here takes the kernel's shape arguments and `cus` and returns `walks`: one list per workgroup, in
blockIdx order, of the units it computes, in the order it computes them; a unit is (image, tile index inside the image, output
block).  A launch the host wrapper refuses for that CU share is `None`.  Four schemes:

  banded      the units are cut into 8 contiguous bands (one per XCD = blockIdx & 7); the grid / 8 workgroups of an XCD stride through
              its band.  conv3x3_ring.hip (both kernels, :119-126 / :571-577, unit = block fastest), conv3x3_c64_wsq_kernel
              (conv3x3_ws.hip:478-484, a workgroup keeps ONE output block and the band is over tiles).
  interleaved conv3x3_c64_ws_kernel (private halo, conv3x3_ws.hip:104-107, :157-169: groups of 8 consecutive 2 x 32 tiles dealt
              round-robin over the partitions) and the Winograd kernel (conv3x3_wino.hip:89-95: unit pair * 8 + xcd + k * npairs * 8).
  contiguous  [units * w / grid, units * (w + 1) / grid): the two stream kernels (conv1x1_stream.hip:97, :479), conv3x3_n16.hip:85;
              [w * per, (w + 1) * per) with per = ceil(units / grid): qkv_dw.hip:91 (tiled) and :330 (row streaming).
  strided     w, w + grid, ...: block_pro.hip:76-78, grid = min(tiles, 2 * cus).

No GPU, no torch: tests/test_schedule_cases_cpu.py holds this table to the walks it is meant to produce."""


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------- banded (ring, wsq)
def _band_walk(n, xcd, slot, nslots):
    """ordinals band0 + slot + k * nslots inside XCD xcd's band of n units (band_n may be <= 0: an empty walk)"""
    band = (n + 7) >> 3
    band0 = xcd * band
    band_n = min(band, n - band0)
    mine = (band_n - slot + nslots - 1) // nslots if band_n > slot else 0
    return [band0 + slot + k * nslots for k in range(mine)]


def ring_walks(B, H, W, Cout, cus):
    """conv3x3_ring_kernel / conv3x3_ring_split_kernel: tile 16 x 32, unit = (image, tile, 64-channel block), block fastest;
    grid = cus / 8 * 8 (cdfo_conv3x3_ring); cus < 8 is refused."""
    if cus < 8:
        return None
    grid = cus // 8 * 8
    tiles = cdiv(W, 32) * cdiv(H, 16)
    nco = cdiv(Cout, 64)
    units = B * tiles * nco
    walks = []
    for wg in range(grid):
        us = _band_walk(units, wg & 7, wg >> 3, grid >> 3)
        walks.append([((u // nco) // tiles, (u // nco) % tiles, u % nco) for u in us])
    return walks


def ws_form(Cout, cus, ring_switch=True):
    """cdfo_conv3x3_c64_ws's choice (ws_launch): 'wsq' (ring-fed) while (Cout >> 6) <= cus / 8, else the private-halo kernel 'ws';
    the residual entry point always takes 'ws'."""
    return "wsq" if ring_switch and (Cout >> 6) <= cus // 8 else "ws"


def wsq_walks(B, H, W, Cout, cus):
    """conv3x3_c64_wsq_kernel: tile 16 x 32; slot -> (block nb = slot % nco, q = slot / nco); the nq = nslots / nco workgroups of a
    block stride through the XCD's band of tiles; q >= nq idles.  grid = cus / 8 * 8."""
    if cus < 8:
        return None
    grid = cus // 8 * 8
    nco = Cout >> 6
    nslots = grid >> 3
    nq = nslots // nco
    if nq < 1:
        return None                                     # ws_launch never sends such a launch here (ws_form)
    tiles = cdiv(W, 32) * cdiv(H, 16)
    walks = []
    for wg in range(grid):
        slot = wg >> 3
        nb, q = slot % nco, slot // nco
        ts = _band_walk(B * tiles, wg & 7, q, nq) if q < nq else []
        walks.append([(t // tiles, t % tiles, nb) for t in ts])
    return walks


# ------------------------------------------------------------------------------------------------------ interleaved (ws, wino)
def ws_walks(B, H, W, Cout, cus):
    """conv3x3_c64_ws_kernel (private halo): tiles of 2 rows x 32 columns, total = B * H/2 * tiles_x; grid = 8 * qn * nco with
    qn = max(1, cus / 8 / nco); the workgroup's i-th tile is ((i >> 3) * nparts + part) * 8 + (i & 7) while that is < total.  Its
    waves draw i from an LDS counter, so the ORDER inside a workgroup is not fixed; the set is."""
    if cus < 8:
        return None
    nco = Cout >> 6
    qn = max(1, cus // 8 // nco)
    grid = 8 * qn * nco
    nparts = ((grid >> 3) // nco) * 8
    tiles_x, hp = cdiv(W, 32), H >> 1
    total = B * hp * tiles_x
    walks = []
    for wg in range(grid):
        slot = wg >> 3
        nb, part = slot % nco, (slot // nco) * 8 + (wg & 7)
        walk, i = [], 0
        while ((i >> 3) * nparts + part) * 8 + (i & 7) < total:
            u = ((i >> 3) * nparts + part) * 8 + (i & 7)
            walk.append((u // (hp * tiles_x), u % (hp * tiles_x), nb))
            i += 1
        walks.append(walk)
    return walks


def wino_geometry(B, H, W, Cout, cus):
    """cdfo_conv3x3_c64_wino_dbg's segment search: (seg_h, nseg, nstrips) -- the segment height depends on the CU share"""
    nhalf = Cout // 128
    lanes = (cus // 8 // nhalf) * 8
    nstrips = cdiv(W, 32)
    best_seg, best_cost = H, 1e30
    for nseg in range(1, cdiv(H, 8) + 1):
        seg_h = cdiv(H, nseg)
        if seg_h * (nseg - 1) >= H:
            continue
        rounds = cdiv(B * nstrips * nseg, lanes)
        cost = float(rounds) * (3.0 * ((seg_h + 2 + 2) // 3) + 1.0)
        if cost < best_cost - 1e-9:
            best_cost, best_seg = cost, seg_h
    return best_seg, cdiv(H, best_seg), nstrips


def wino_walks(B, H, W, Cout, cus):
    """conv3x3_c64_wino_kernel (H, W of the convolution: twice the source's in the up2 form): unit = (image, segment, 32-column
    strip), strip fastest; slot -> (128-channel half = slot % nhalf, pair = slot / nhalf), pair >= npairs idles; units
    pair * 8 + xcd + k * npairs * 8.  cus / 8 < nhalf is refused."""
    nhalf = Cout // 128
    if cus < 8 or cus // 8 < nhalf:
        return None
    nslots = cus // 8
    npairs = nslots // nhalf
    _, nseg, nstrips = wino_geometry(B, H, W, Cout, cus)
    upi = nstrips * nseg
    walks = []
    for wg in range(nslots * 8):
        slot = wg >> 3
        half, pair = slot % nhalf, slot // nhalf
        us = range(pair * 8 + (wg & 7), B * upi, npairs * 8) if pair < npairs else []
        walks.append([(u // upi, u % upi, half) for u in us])
    return walks


# ---------------------------------------------------------------------------------------------------------------- contiguous
def _ranges(units, grid):
    return [list(range(units * w // grid, units * (w + 1) // grid)) for w in range(grid)]


def stream_walks(B, P, cus):
    """conv1x1_stream_kernel and align_gram_partial_kernel: 128-pixel tiles, grid = min(tiles, cus) (st_tiling); every output block of
    a tile is computed by the tile's workgroup in one pass (block = 0)."""
    tpi = cdiv(P, 128)
    grid = min(B * tpi, cus)
    return [[(t // tpi, t % tpi, 0) for t in r] for r in _ranges(B * tpi, grid)]


def st_owner(t, tiles, grid):
    return ((t + 1) * grid + tiles - 1) // tiles - 1


def stream_slots(B, P, cus):
    """cdfo_align_stats_slots = cdfo_stream_slots_for_grid(B, P, cus) (st_slots)"""
    tpi = cdiv(P, 128)
    tiles = B * tpi
    grid = min(tiles, cus)
    return max(1, max(st_owner((b + 1) * tpi - 1, tiles, grid) - st_owner(b * tpi, tiles, grid) + 1 for b in range(B)))


def stream_slot_of(B, P, cus, wg, b):
    """the slot of image b that workgroup wg writes (conv1x1_stream.hip:426, :642)"""
    tpi = cdiv(P, 128)
    tiles = B * tpi
    return wg - st_owner(b * tpi, tiles, min(tiles, cus))


def n16_walks(B, H, W, cus):
    """conv3x3_c64_n16_kernel: tile 8 x 32, t = (b * tiles_x + tx) * tiles_y + ty (down a column); grid = min(tiles, cus)."""
    tx_n, ty_n = cdiv(W, 32), cdiv(H, 8)
    ntiles = B * tx_n * ty_n
    walks = []
    for r in _ranges(ntiles, min(ntiles, cus)):
        walks.append([(t // ty_n // tx_n, (t % ty_n) * tx_n + (t // ty_n) % tx_n, 0) for t in r])     # tile index row-major
    return walks


def _per_ranges(units, grid):
    per = cdiv(units, grid)
    return per, [list(range(w * per, min((w + 1) * per, units))) for w in range(grid)]


def qkv_tiled_walks(B, H, W, cus):
    """qkv_dw_kernel (192-channel form): tile 6 x 30, t = (b * tiles_y + ty) * tiles_x + tx; grid = min(tiles, cus)."""
    tpi = cdiv(H, 6) * cdiv(W, 30)
    _, rs = _per_ranges(B * tpi, min(B * tpi, cus))
    return [[(t // tpi, t % tpi, 0) for t in r] for r in rs]


def qkv_gram_geometry(H, W):
    """q2_geometry: (strips, nseg, rows per segment, units per image)"""
    strips = cdiv(W, 30)
    nseg = (H + 55) // 56 if H > 80 else 1
    return strips, nseg, cdiv(H, nseg), strips * nseg


def qkv_gram_walks(B, H, W, cus):
    """qkv_dw2_kernel (row streaming, fused Gram pass): unit = (image, segment, 30-column strip), strip fastest; grid = min(units, cus)."""
    upi = qkv_gram_geometry(H, W)[3]
    _, rs = _per_ranges(B * upi, min(B * upi, cus))
    return [[(u // upi, u % upi, 0) for u in r] for r in rs]


def qkv_gram_slots(B, H, W, cus):
    """cdfo_qkv_dw_gram_slots"""
    upi = qkv_gram_geometry(H, W)[3]
    units = B * upi
    per = cdiv(units, min(units, cus))
    return cdiv(upi, per) + 1


def qkv_gram_slot_of(B, H, W, cus, wg, b):
    """qkv_dw.hip:383-384: slot = blockIdx - (b * upi) / per"""
    upi = qkv_gram_geometry(H, W)[3]
    units = B * upi
    per = cdiv(units, min(units, cus))
    return wg - (b * upi) // per


# -------------------------------------------------------------------------------------------------------------------- strided
def block_pro_walks(B, H, W, cus):
    """block_pro_kernel: tile 6 x 30, t = (b * tiles_y + ty) * tiles_x + tx; grid = min(tiles, 2 * cus), t = w, w + grid, ..."""
    tpi = cdiv(H, 6) * cdiv(W, 30)
    ntiles = B * tpi
    grid = min(ntiles, 2 * cus)
    return [[(t // tpi, t % tpi, 0) for t in range(w, ntiles, grid)] for w in range(grid)]


# ------------------------------------------------------------------------------------------------------- walks of a table entry
TILE = {"ring": (16, 32), "wsq": (16, 32), "ws": (2, 32), "n16": (8, 32), "qkv_tiled": (6, 30), "block_pro": (6, 30)}


def walks_of(kernel, shape, cus):
    """(walks or None, number of units) of `kernel` at `shape` on `cus` compute units.  Kernels: ring (B, H, W, Cout), ws_plain
    (B, H, W, Cout; the form follows ws_form), ws_res (B, H, W), offmask (B, H, W; 432 -> 448 padded channels, refused unless 7 <=
    cus / 8), wino (B, H, W, Cout), wino_up2 (B, h, w, Cout: source size), n16, block_pro, qkv_tiled, qkv_gram (B, H, W), stream,
    align_stats (B, H, W)."""
    if kernel == "ring":
        B, H, W, Cout = shape
        return ring_walks(B, H, W, Cout, cus), B * cdiv(W, 32) * cdiv(H, 16) * cdiv(Cout, 64)
    if kernel == "ws_plain":
        B, H, W, Cout = shape
        if ws_form(Cout, cus) == "wsq":
            return wsq_walks(B, H, W, Cout, cus), B * cdiv(W, 32) * cdiv(H, 16) * (Cout >> 6)
        return ws_walks(B, H, W, Cout, cus), B * (H >> 1) * cdiv(W, 32) * (Cout >> 6)
    if kernel == "ws_res":
        B, H, W = shape
        return ws_walks(B, H, W, 64, cus), B * (H >> 1) * cdiv(W, 32)
    if kernel == "offmask":
        B, H, W = shape
        return (wsq_walks(B, H, W, 448, cus) if cus >= 8 and 7 <= cus // 8 else None), B * cdiv(W, 32) * cdiv(H, 16) * 7
    if kernel in ("wino", "wino_up2"):
        B, H, W, Cout = shape
        if kernel == "wino_up2":
            H, W = 2 * H, 2 * W
        walks = wino_walks(B, H, W, Cout, cus)
        if walks is None:
            return None, 0
        _, nseg, nstrips = wino_geometry(B, H, W, Cout, cus)
        return walks, B * nseg * nstrips * (Cout // 128)
    B, H, W = shape
    if kernel == "n16":
        return n16_walks(B, H, W, cus), B * cdiv(W, 32) * cdiv(H, 8)
    if kernel == "block_pro":
        return block_pro_walks(B, H, W, cus), B * cdiv(H, 6) * cdiv(W, 30)
    if kernel == "qkv_tiled":
        return qkv_tiled_walks(B, H, W, cus), B * cdiv(H, 6) * cdiv(W, 30)
    if kernel == "qkv_gram":
        return qkv_gram_walks(B, H, W, cus), B * qkv_gram_geometry(H, W)[3]
    if kernel in ("stream", "align_stats"):
        return stream_walks(B, H * W, cus), B * cdiv(H * W, 128)
    raise KeyError(kernel)


def ragged_last(kernel, shape, cus, unit):
    """True when `unit` is the image's last tile and that tile is cut by the image in x and in y (2-D tiled kernels); for the
    1-D tile streams (stream, align_stats): the image's last, partial 128-pixel tile."""
    b, t, _ = unit
    if kernel in ("stream", "align_stats"):
        B, H, W = shape
        return (H * W) % 128 != 0 and t == cdiv(H * W, 128) - 1
    if kernel in ("wino", "wino_up2"):
        B, H, W, Cout = shape
        if kernel == "wino_up2":
            H, W = 2 * H, 2 * W
        seg_h, nseg, nstrips = wino_geometry(B, H, W, Cout, cus)
        return W % 32 != 0 and H % seg_h != 0 and t == nseg * nstrips - 1
    if kernel == "qkv_gram":
        B, H, W = shape
        strips, nseg, rs, upi = qkv_gram_geometry(H, W)
        return W % 30 != 0 and t == upi - 1              # (one segment per image below 81 rows: nothing ragged in y)
    B, H, W = shape[:3]
    key = {"ws_res": "ws", "offmask": "wsq"}.get(kernel, kernel)
    if kernel == "ws_plain":
        key = ws_form(shape[3], cus)
    th, tw = TILE[key]
    if key == "ws":
        return W % tw != 0 and t == cdiv(H, th) * cdiv(W, tw) - 1
    return H % th != 0 and W % tw != 0 and t == cdiv(H, th) * cdiv(W, tw) - 1


# ------------------------------------------------------------------------------------------------------------------ the table
# Banded kernels (tile 16 x 32).  3 x 40 x 70: 9 tiles per image (both edges ragged), 27 units per output block, band 4: XCDs 0-5
# hold 4, XCD 6 holds 3, XCD 7's band_n is -1; image boundaries (units 9, 18) fall inside bands 2 and 4.
#   L = 8 (one slot per XCD): walks 4 / 3 / 0;  L = 16: 2 (and 2 + 1 on XCD 6);  L = 24: 2 / 1 / 1 (and 1 / 1 / 1 on XCD 6).
# 2 x 48 x 100 with Cout = 128: 12 tiles, 48 units with the block fastest, band 6: at L = 8 walks of 6 that alternate the block.
S_BAND = (3, 40, 70)
S_BLOCKS = (2, 48, 100)
BAND_LIMITS = (8, 16, 24)
# Contiguous and strided kernels.  3 x 16 x 136 = 51 stream tiles of 128 pixels (17 per image), as tests/test_gpu_rdab_fused.py uses;
# one small ragged shape per kernel from its own tile size.
S_STREAM = (3, 16, 136)
SMALL_LIMITS = (1, 3, 7)

CASES = []          # (kernel, shape, limit)
for _L in BAND_LIMITS:
    CASES.append(("ring", S_BAND + (64,), _L))
    CASES.append(("ws_plain", S_BAND + (64,), _L))          # ring-fed form at every limit (1 block <= L / 8)
    CASES.append(("ws_res", S_BAND, _L))                    # always the private-halo form
    CASES.append(("wino", S_BAND + (128,), _L))
    CASES.append(("wino_up2", (3, 20, 35 + 1, 128), _L))    # source 20 x 36 -> a 40 x 72 convolution (even source sizes)
CASES.append(("wino", (3, 24, 70, 128), 8))                 # 12-row segments, 18 units on 8 lanes: walks of 2 and 3
CASES.append(("wino_up2", (3, 12, 36, 128), 8))             # the same walks on a 24 x 72 convolution
for _s in ((1, 2, 8), (1, 2, 40), (1, 6, 8)):               # 1, 2, 3 tiles of 2 x 32: the first partition's waves take one each
    CASES.append(("ws_res", _s, 8))
CASES.append(("ring", S_BLOCKS + (128,), 8))                # six units per workgroup, output block alternating
CASES.append(("ws_plain", S_BLOCKS + (128,), 8))            # 2 blocks > 8 / 8: the limit flips the call to the private-halo form
CASES.append(("ws_plain", S_BLOCKS + (128,), 16))           # 2 blocks <= 16 / 8: ring-fed, one workgroup per block and XCD
CASES.append(("ws_plain", (3, 48, 100, 64), 8))             # ring-fed: 36 tiles, band 5: walks 5 (crossing images inside bands 2 and 4) and 1
for _s in ((1, 2, 8), (1, 2, 40), (1, 6, 8)):               # private-halo form (2 blocks at L = 8) with 1, 2, 3 tiles of 2 x 32
    CASES.append(("ws_plain", _s + (128,), 8))
CASES.append(("wino", S_BLOCKS + (256,), 16))               # two 128-channel halves, one pair: every workgroup walks 8 / 1 = all units of its lane
# conv_offset[2] on the ring-fed kernel: 448 padded channels = 7 blocks, so the wrapper takes no share below 56 CUs
for _L in (56, 64, 112):
    CASES.append(("offmask", (3, 40, 72), _L))              # (the tiled kernel beside it in the existing test needs W % 4 == 0)
CASES.append(("offmask", (1, 40, 72), 56))                  # 9 tiles, band 2: walks 2 / 1 / 0 with one workgroup per block
CASES.append(("offmask", (4, 40, 72), 56))                  # 36 tiles, band 5, one workgroup per block and XCD: walks 5 and 1
for _L in SMALL_LIMITS:
    CASES.append(("stream", (3, 13, 21), _L))               # 273 pixels: three tiles per image, the last one partial
    CASES.append(("align_stats", (3, 13, 21), _L))
    for _k in ("stream", "align_stats", "n16", "block_pro", "qkv_tiled", "qkv_gram"):
        CASES.append((_k, S_STREAM, _L))
    CASES.append(("n16", (2, 20, 40), _L))                  # 8 x 32 tiles: 3 x 2 per image, ragged in x and y
    CASES.append(("block_pro", (2, 16, 40), _L))            # 6 x 30 tiles: 3 x 2 per image, ragged in x and y
    CASES.append(("qkv_tiled", (2, 16, 40), _L))
    CASES.append(("qkv_gram", (3, 10, 70), _L))             # 3 strips per image (ragged in x), 9 units
CASES.append(("qkv_gram", (3, 10, 70), 4))                  # per = 3: the fourth workgroup's range is empty
CASES.append(("qkv_tiled", (1, 18, 90), 4))                 # 9 tiles, per = 3: an empty fourth range
CASES.append(("stream", (3, 16, 136), 17))                  # 51 tiles on 17 workgroups: walks of exactly 3
CASES.append(("stream", (3, 16, 136), 26))                  # walks of 1 and 2
CASES.append(("align_stats", (3, 16, 136), 17))
CASES.append(("align_stats", (3, 16, 136), 26))
CASES.append(("n16", (2, 20, 40), 4))                       # 12 tiles: walks of 3
CASES.append(("n16", (2, 20, 40), 6))                       # walks of 2
CASES.append(("n16", (2, 20, 40), 12))                      # walks of 1
CASES.append(("block_pro", (2, 16, 40), 2))                 # 12 tiles on 4 workgroups: walks of 3
CASES.append(("block_pro", (2, 16, 40), 6))                 # 12 workgroups: walks of 1
CASES.append(("qkv_tiled", (2, 16, 40), 4))                 # walks of 3
CASES.append(("qkv_tiled", (2, 16, 40), 12))                # walks of 1
CASES.append(("qkv_gram", (3, 10, 70), 9))                  # walks of 1
CASES.append(("qkv_gram", (3, 10, 70), 5))                  # per = 2: walks of 2 and one of 1

DEVICE_CUS = (256, 304, 64, 32)

# What a scheme cannot reach (tests/test_schedule_cases_cpu.py asserts everything else, per kernel):
#   empty     stream, align_stats, n16: grid = min(units, cus) and the ranges units * w / grid are never empty; block_pro: grid <=
#             tiles, every workgroup has its first tile.
#   block     only the ring kernels carry the output block inside the unit index; every other kernel keeps one block per workgroup
#             (ws, wsq, wino) or computes all blocks of a tile in one pass (stream, n16, block_pro, qkv_dw).
#   ragged_xy qkv_gram is ragged in x only at these sizes (one segment per image up to 80 rows), the private-halo ws kernel always
#             (2-row tiles, H even); the stream kernels' tiles are 1-D: "ragged" there is the image's partial last tile.
#   offmask   on a 32-CU device every launch is refused (7 blocks need 56 CUs); nothing else is out of its reach.
# ws_plain is two kernels: the ring-fed conv3x3_c64_wsq_kernel and, where the share has fewer than 8 CUs per output block, the
# private-halo conv3x3_c64_ws_kernel.  kernel_key() names the one that runs, and each has to reach its own walks.
UNREACHABLE = {
    "stream": {"len0", "block"}, "align_stats": {"len0", "block"}, "n16": {"len0", "block"}, "block_pro": {"len0", "block"},
    "qkv_tiled": {"block"}, "qkv_gram": {"block"}, "ws_plain/wsq": {"block"}, "ws_plain/ws": {"block"}, "ws_res": {"block"},
    "wino": {"block"}, "wino_up2": {"block"}, "offmask": {"block"}, "ring": set(),
}


def kernel_key(kernel, shape, cus):
    """the table kernel, with ws_plain split by the form that runs on `cus` compute units"""
    return f"ws_plain/{ws_form(shape[3], cus)}" if kernel == "ws_plain" else kernel
