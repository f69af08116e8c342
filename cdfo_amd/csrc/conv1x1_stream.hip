// 1x1 convolution as a persistent HBM stream: LDS-DMA rings, no workgroup barrier in the steady state.
//
// conv1x1_bf16x3.hip (one 128-pixel tile per workgroup: load -> split -> LDS -> barrier -> MFMA -> LDS transpose -> store)
// reaches 2.2-3.4 TB/s of algorithmic traffic: its phases are separated by barriers, only two workgroups fit a CU, and
// HBM is idle whenever both are computing or storing.  The 1x1 convolutions of the CVSR_V8 forward (arch.py: attention
// apply of MDTA :1573-1575 and DualAttAlignment :3459-3491 as per-image folded weights, RDAB.input_conv / fuse
// :2196,2246, conv_du_re.0 :2148, fusion_out :3441, Block_.up.0 :381) move 4*(Cin+Cout) bytes per pixel for 2*Cin*Cout
// FLOP: pure streams.  Here
//   * one 256-thread workgroup per CU is persistent over a contiguous range of 128-pixel tiles; each of its four waves owns
//     32 pixels of the tile and a PRIVATE ring of 8 KB LDS stages that it fills itself by LDS-DMA
//     (buffer_load_dwordx4 ... lds): the fp32 pixel-major activations of one 64-channel K block (32 pixels x 256 B), and
//     after the last K block the tile's residual operands, arrive as 8 pieces of 1 KiB with NS-1 stages in flight behind a
//     counted s_waitcnt -- no staging registers, no barrier, the waves drift freely;
//   * the LDS image is [pixel][16-byte part ^ (pixel & 15)] (the swizzle is applied on the DMA's per-lane source
//     address), so the fragment reads -- a lane's 8 consecutive input channels of its pixel, two ds_read_b128 -- are
//     conflict-free; the lane splits them to bf16 hi / lo in registers and feeds the MFMA directly (no LDS write pass);
//   * same arithmetic as conv1x1_bf16x3: split-bf16, a_lo*w_hi + a_hi*w_lo + a_hi*w_hi, fp32 accumulation (fp32-grade);
//     the weights (also the per-image folded attention weights) are split once per image into LDS, rows permuted so that
//     a lane's accumulators are 8 consecutive output channels of its pixel (transposed product, as conv3x3_ws.hip): the
//     epilogue (bias, activation, up to two residuals read from their LDS stages) stores 32 contiguous bytes per lane
//     straight from registers.
// Contract: cdfo_conv_args as cdfo_conv1x1_bf16x3 with plain store, Cin % 64 == 0 per source, Cout % 8 == 0,
// CoutP in {64, 128}, weights + ring within the CU's LDS (Cin * CoutP <= 192 * 64); everything else stays on that kernel.
#include "plane_chunk.h"
#include "image_map.h"
#include <type_traits>

namespace {

struct st_item { const float* base; int ld; int ch0; };     // one 64-channel slice of a pixel-major operand

struct st_args {
  st_item act[CDFO_MAXSRC * 4];    // K blocks in order (<= 12 used: Cin <= 768 guarded by the LDS test anyway)
  int nkb;
  st_item res[2];                  // residual operands (ch0 = 0), res[i].base == nullptr: absent
  const float* res_scale;          // optional per-pixel factor [B][P] of the LAST residual operand (a spatial gate folded into the add)
  const float* w; long long w_bstride; const float* bias;
  int Cin, Cout, CoutP, act_fn;
  float* out; int ldo;
  int B; long long P;              // pixels per image
  int tiles_per_image; long long tiles;
  int ns;                          // ring stages per wave
  // optional second output (Cout == 64): LayerNorm64(result) as fp16 hi | lo chunk-planar planes [B][8][P][16] -- the source of
  // the split-fp16 3x3 convolution that follows the attention in the feature extractor (arch.py:1470-1474): the values are in
  // the epilogue's registers, a separate LayerNorm pass would read the 64-channel result back from HBM
  _Float16* ln_hl; const float* ln_g; const float* ln_b;
  // TAPS form (upconv2 of arch.py:4474-4476, Cout = 256 = 4 sub-pixels x 64): instead of the pixel-shuffled 64-channel HR map, out
  // receives for every HR pixel the nine per-tap channel sums of the 3x3 conv_last that follows (see conv1x1_bf16x3.hip, TAPS):
  // out[HR pixel][ldo], HR pixel = (b, 2 y + (cb >> 1), 2 x + (cb & 1)) of the W-pixel-wide input row (y, x)
  const float* w_last;             // conv_last.weight as [64][9]
  int W;                           // input image width (pixels per row) for the pixel shuffle
  // optional third output (CSUM form, Cout == 64): per-image channel sums of the RESULT as fixed-order partials [B][csum_slots][64]
  // (cdfo_chan_sum_partial's layout; the buffer is zeroed by the caller).  The values are in the epilogue's registers: the global
  // average pool that follows (CALayer, arch.py:3493) needs no pass of its own over the tensor
  float* csum; int csum_slots;
  // PLANE form: one more 64-channel operand of the product, stencil9 of a one-channel plane, as the plane chunk of plane_chunk.h
  // (plane.w: [CoutP][16] per image, the product's weights for that operand composed with the stencil); plane.base == nullptr: absent
  pc_plane plane;
};
// MAP form: where the images of every item lie (image_map.h); act_map[k] belongs to act[k], res_map[i] to res[i].  A block of its own
// that only the MAP instantiations take: the other forms' kernel arguments, and with them their instructions, stay what they were
struct st_args_map : st_args {
  im_map act_map[CDFO_MAXSRC * 4], res_map[2];
};

// The persistent kernels here cut the stream of `tiles` 128-pixel tiles into `grid` contiguous ranges [tiles w / grid, tiles (w + 1) /
// grid).  st_owner: the workgroup whose range holds tile t.  A workgroup's partial sums over its tiles of image b go to slot
// (w - st_owner(first tile of b)) of that image: a static function of the shape and the grid, one writer per (image, slot).
__host__ __device__ inline long long st_owner(long long t, long long tiles, int grid) { return ((t + 1) * grid + tiles - 1) / tiles - 1; }
// slots per image that such a launch may write
inline int st_slots(int B, int tiles_per_image, int grid) {
  const long long tiles = (long long)B * tiles_per_image;
  int n = 1;
  for (int b = 0; b < B; ++b) {
    const int m = (int)(st_owner((long long)(b + 1) * tiles_per_image - 1, tiles, grid) - st_owner((long long)b * tiles_per_image, tiles, grid)) + 1;
    n = m > n ? m : n;
  }
  return n;
}

// NCB: 64-wide output-channel blocks (1, 2; 4 in the TAPS form)
// CSUM (NCB == 1): also the channel sums of the result, see st_args.csum
// PLANE: the plane chunk of st_args.plane joins the product (a template parameter: the other forms' instructions stay what they were)
// MAP: the items' images lie where st_args.act_map / res_map say (a template parameter for the same reason)
template <int NCB, bool TAPS = false, bool CSUM = false, bool PLANE = false, bool MAP = false>
__global__ __launch_bounds__(ST_THREADS) void conv1x1_stream_kernel(std::conditional_t<MAP, st_args_map, st_args> a) {
  static_assert(!(PLANE && TAPS), "the TAPS form takes no plane chunk");
  static_assert(!(MAP && TAPS), "the TAPS form takes no image map");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkb = a.nkb, NS = a.ns;
  // LDS map: weights hi [nkb*4 chunks][2 k-halves][NCB*64 rows][8 bf16] | weights lo (same) | bias [NCB*64 floats] |
  //          4 waves x NS stages (st_weight_bytes on the host)
  const int w_half = nkb * 4 * 2 * NCB * 64 * 16;
  const int ring_off = 2 * w_half + NCB * 64 * 4;
  unsigned char* sWh = smem;
  unsigned char* sWl = smem + w_half;
  float* sBias = reinterpret_cast<float*>(smem + 2 * w_half);
  unsigned char* ring = smem + ring_off + wave * NS * ST_STAGE;
  const unsigned ring_lds = (unsigned)(unsigned long long)(smem) + ring_off + wave * NS * ST_STAGE;
  // res_scale: two 256-byte slots per wave (tile parity) behind the rings
  const unsigned char* scale_slots = smem + ring_off + 4 * NS * ST_STAGE + wave * 512;
  const unsigned scale_lds = (unsigned)(unsigned long long)(smem) + ring_off + 4 * NS * ST_STAGE + wave * 512;
  // PLANE (never together with res_scale): behind the rings the chunk's weight image hi | lo, then NS tap slots per wave
  unsigned char* sPh = smem + ring_off + 4 * NS * ST_STAGE;
  unsigned char* sPl = sPh + pc_weight_bytes(NCB) / 2;
  const unsigned char* tap_slots = sPh + pc_weight_bytes(NCB) + wave * NS * PC_SLOT;
  const unsigned tap_lds = (unsigned)(unsigned long long)(smem) + ring_off + 4 * NS * ST_STAGE + pc_weight_bytes(NCB) + wave * NS * PC_SLOT;

  // this workgroup's contiguous tile range
  const long long t_lo = a.tiles * blockIdx.x / gridDim.x, t_hi = a.tiles * (blockIdx.x + 1) / gridDim.x;
  if (t_lo >= t_hi) return;
  const int nres = (a.res[0].base ? 1 : 0) + (a.res[1].base ? 1 : 0);
  const int items_per_tile = nkb + nres * NCB;
  const float slope = a.act_fn == CDFO_ACT_NONE ? 1.f : (a.act_fn == CDFO_ACT_LRELU ? 0.1f : 0.f);

  // per-lane DMA slot geometry: piece k, lane l -> slot s = 64 k + l -> pixel p = s >> 4 (0..31), part (s & 15) ^ (p & 15)
  int d_px[8], d_part[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int s = 64 * k + lane, p = s >> 4;
    d_px[k] = p;
    d_part[k] = (s & 15) ^ (p & 15);
  }
  // fragment read offsets of this lane's pixel r: 16-byte part q lives at r*256 + ((q ^ (r & 15)) << 4)
  auto part_off = [&](int q) { return r * 256 + ((q ^ (r & 15)) << 4); };

  // TAPS: A operand of the second product = w_last^T (row = tap, rows 9..31 zero), fp16 hi | lo, in registers for the whole launch:
  // lane (r = tap, h) holds channels 16 s4 + 8 h .. + 7
  f16x8_t twh[TAPS ? 4 : 1], twl[TAPS ? 4 : 1];
  if (TAPS) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float wv = r < 9 ? a.w_last[(16 * s4 + 8 * h + j) * 9 + r] : 0.f;
        twh[s4][j] = (_Float16)wv;
        twl[s4][j] = (_Float16)(wv - (float)twh[s4][j]);
      }
  }

  for (long long img_t0 = t_lo; img_t0 < t_hi;) {
    const int b = (int)(img_t0 / a.tiles_per_image);
    const long long img_end = (long long)(b + 1) * a.tiles_per_image;
    const long long seg_hi = img_end < t_hi ? img_end : t_hi;           // tiles [img_t0, seg_hi) belong to image b
    // ---- this image's weights -> LDS (split bf16 hi | lo, rows permuted).  No DMA is in flight here.
    __syncthreads();                                                     // previous image's MFMAs are done with sW
    {
      const float* wb = a.w + (long long)b * a.w_bstride;
      const int ngrp = (a.Cin >> 2) * NCB * 64;                          // (group of 4 input channels, row position)
      for (int i = tid; i < ngrp; i += ST_THREADS) {
        const int rowpos = i % (NCB * 64), kg = i / (NCB * 64);
        const int n = mfma_row_channel(rowpos);
        f32x4 wv = {0.f, 0.f, 0.f, 0.f};
        if (n < a.CoutP) wv = *reinterpret_cast<const f32x4*>(wb + ((long long)kg * a.CoutP + n) * 4);
        const int c = kg >> 2, hh = (kg >> 1) & 1, j0 = (kg & 1) * 4;
        u32x2 hi, lo;
        split4_bf16(wv, hi, lo);
        const int off = ((c * 2 + hh) * (NCB * 64) + rowpos) * 16 + j0 * 2;
        *reinterpret_cast<u32x2*>(sWh + off) = hi;
        *reinterpret_cast<u32x2*>(sWl + off) = lo;
      }
      for (int i = tid; i < NCB * 64; i += ST_THREADS) sBias[i] = (a.bias && i < a.Cout) ? a.bias[i] : 0.f;   // by channel
      if (PLANE) pc_load_weights<NCB>(a.plane.w + (long long)b * a.plane.w_bstride, a.CoutP, sPh, sPl, tid);
    }
    __syncthreads();

    // ---- the item stream of this wave for tiles [img_t0, seg_hi): per tile nkb K blocks, then the residual stages
    const long long n_items = (seg_hi - img_t0) * items_per_tile;
    long long issued = 0;
    auto issue = [&](long long it) {
      const long long tile = img_t0 + it / items_per_tile;
      const int k = (int)(it % items_per_tile);
      const long long p0 = (tile - (long long)b * a.tiles_per_image) * 128 + wave * 32;      // first pixel (inside image b)
      if (a.res_scale && k == 0) {
        // the tile's per-pixel residual factors: one more LDS-DMA piece (lane l -> dword l of the tile-parity slot), requested AHEAD
        // of the tile's first item.  An ordinary load would be waited for with vmcnt(0) at its use and drain the ring; memory
        // operations retire in order, so the slot is valid once any item of this tile has landed (the hand-counted waits below,
        // which one more older piece only makes more conservative).
        const long long rows = a.P - p0;
        const i32x4 rs = lds_dma_rsrc_uniform(a.res_scale + (long long)b * a.P + (rows > 0 ? p0 : 0),
                                              (unsigned)(rows > 0 ? (rows < 32 ? rows : 32) * 4 : 0));      // beyond the image: zeros
        lds_dma0_dword((unsigned)r * 4, rs, __builtin_amdgcn_readfirstlane(scale_lds + (unsigned)(tile & 1) * 256));
      }
      if (PLANE && k == 0)       // the tile's taps, ahead of its first item like the factors above (plane_chunk.h)
        pc_issue(pc_image(a.plane, b), (int)a.P, a.plane.W, (int)p0, lane, tap_lds + (unsigned)((it / items_per_tile) % NS) * PC_SLOT);
      st_item src;
      int chan0;
      long long img = 0;         // MAP: floats from the item's first image to image b -- the one place an item's image is located
      if (k < nkb) { src = a.act[k]; chan0 = src.ch0; if constexpr (MAP) img = im_offset(a.act_map[k], b); }
      else {                     // residual operands are packed from slot 0 by the host wrapper
        const int j = k - nkb;
        src = a.res[j / NCB];
        chan0 = (j % NCB) * 64;
        if constexpr (MAP) img = im_offset(a.res_map[j / NCB], b);
      }
      // descriptor based at the wave's first pixel: offsets stay small whatever the tensor's size
      const long long rows_left = a.P - p0;                               // may be <= 0: everything out of range
      // (MAP: the descriptor below still ends with this image's last pixel, so no lane reads a neighbouring slot of a stack)
      const float* base = MAP ? src.base + img + (rows_left > 0 ? p0 : 0) * src.ld + chan0
                              : src.base + ((long long)b * a.P + (rows_left > 0 ? p0 : 0)) * src.ld + chan0;
      i32x4 rsrc = lds_dma_rsrc_uniform(base, 0u);
      const long long bytes = rows_left > 0 ? (rows_left < 32 ? rows_left : 32) * (long long)src.ld * 4 : 0;
      lds_dma_rsrc_resize_uniform(rsrc, (unsigned)bytes);                 // lanes beyond the image read zeros
      unsigned voff[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) voff[q] = (unsigned)(d_px[q] * src.ld * 4 + d_part[q] * 16);
      lds_dma0(voff, rsrc, __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)(it % NS) * ST_STAGE));
    };
    for (; issued < NS - 1 && issued < n_items; ++issued) issue(issued);

    f32x16 acc[NCB][2];
    float cs[CSUM ? 32 : 1];       // CSUM: this lane's running sums of its 32 channels over its pixels of image b
#pragma unroll
    for (int e = 0; e < (CSUM ? 32 : 1); ++e) cs[e] = 0.f;
    for (long long it = 0; it < n_items; ++it) {
      const int k = (int)(it % items_per_tile);
      // item `it` has landed when at most the 8 * (younger items in flight) youngest DMA pieces are outstanding
      // (pieces retire in order among themselves; stores in flight only make the wait more conservative)
      st_wait_landed(TAPS ? 0 : issued - it - 1);      // TAPS: nothing younger is in flight, its next request goes out just below
      const unsigned char* st = ring + (it % NS) * ST_STAGE;
      if (TAPS) {
        // two-stage ring (the 64 KB weight image leaves room for no more): the stage of item it - 1 was consumed in the previous
        // trip, so item it + 1 is requested NOW and lands behind this tile's products and tap epilogue
        if (issued < n_items) { wait_lgkm<0>(); issue(issued); ++issued; }
      }
      if (k == 0) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[cb][ni][e] = 0.f;
        if (PLANE) {
          // the plane chunk's k-step opens the tile's product: its slot landed before this item (requested ahead of it) and is
          // read here, before the request below can reuse any slot (plane_chunk.h)
          const int p = (int)((img_t0 + it / items_per_tile - (long long)b * a.tiles_per_image) * 128) + wave * 32 + r;
          unsigned thi[4], tlo[4];
          pc_operand(tap_slots + ((it / items_per_tile) % NS) * PC_SLOT, r, h, p, (int)a.P, a.plane.W, thi, tlo);
          pc_mfma<NCB>(sPh, sPl, r, h, thi, tlo, acc);
        }
      }
      if (k < nkb) {
        // ---- one K block: 4 chunks of 16 channels; this lane's operand = channels c*16 + h*8 .. +7 of pixel r
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(st + part_off(c * 4 + h * 2));
          const f32x4 v1 = *reinterpret_cast<const f32x4*>(st + part_off(c * 4 + h * 2 + 1));
          union { unsigned u[4]; bf16x8_t v; } ph, pl;
          split8_bf16(v0, v1, ph.u, pl.u);
          const int wrow = ((k * 4 + c) * 2 + h) * (NCB * 64) + r;
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
              const bf16x8_t wh = *reinterpret_cast<const bf16x8_t*>(sWh + (wrow + cb * 64 + ni * 32) * 16);
              const bf16x8_t wl = *reinterpret_cast<const bf16x8_t*>(sWl + (wrow + cb * 64 + ni * 32) * 16);
              acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, pl.v, acc[cb][ni], 0, 0, 0);
              acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ph.v, acc[cb][ni], 0, 0, 0);
              acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ph.v, acc[cb][ni], 0, 0, 0);
            }
        }
        if (k == nkb - 1) {      // bias + activation, in place: acc[cb][ni][8 jj + q] = channel cb*64 + ni*32 + jj*16 + h*8 + q
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
              for (int e = 0; e < 16; ++e) {
                const float t = acc[cb][ni][e] + sBias[cb * 64 + ni * 32 + (e >> 3) * 16 + h * 8 + (e & 7)];
                acc[cb][ni][e] = fmaxf(t, 0.f) + slope * fminf(t, 0.f);
              }
        }
      } else {
        // ---- a residual stage: 64 channels of block cb of the tile's residual operand
        const int cb = (k - nkb) % NCB;
        float sc = 1.f;
        if (a.res_scale && (k - nkb) / NCB == nres - 1)
          sc = *reinterpret_cast<const float*>(scale_slots + ((img_t0 + it / items_per_tile) & 1) * 256 + lane * 4);
#pragma unroll
        for (int cc = 0; cc < NCB; ++cc) {
          if (cc != cb) continue;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
              const int q = (ni * 32 + jj * 16 + h * 8) >> 2;
              const f32x4 r0 = *reinterpret_cast<const f32x4*>(st + part_off(q));
              const f32x4 r1 = *reinterpret_cast<const f32x4*>(st + part_off(q + 1));
#pragma unroll
              for (int e = 0; e < 4; ++e) { acc[cc][ni][8 * jj + e] = fmaf(sc, r0[e], acc[cc][ni][8 * jj + e]); acc[cc][ni][8 * jj + 4 + e] = fmaf(sc, r1[e], acc[cc][ni][8 * jj + 4 + e]); }
            }
        }
      }
      // the stage may be overwritten once its reads have returned: the next DMA below targets the stage of item it-1... wait
      // for this item's own LDS reads too (they were consumed by the MFMAs / adds above, so they have returned)
      if (!TAPS && issued < n_items) { wait_lgkm<0>(); issue(issued); ++issued; }
      if (k == items_per_tile - 1) {
        // ---- store: 32 contiguous bytes per lane and 16-channel group
        const long long tile = img_t0 + it / items_per_tile;
        const long long pin = (tile - (long long)b * a.tiles_per_image) * 128 + wave * 32 + r;
        if (NCB == 1 && a.ln_hl && !a.ln_g) {
          // plain fp16 chunk-planar copy [B][4][P][16] of the result (the source layout of the weights-stationary 3x3 kernel)
          typedef _Float16 st_f16x8 __attribute__((ext_vector_type(8)));
          if (pin < a.P) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
              for (int jj = 0; jj < 2; ++jj) {
                const int n = ni * 32 + jj * 16 + h * 8;
                st_f16x8 hv;
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = (_Float16)acc[0][ni][8 * jj + e];
                *reinterpret_cast<st_f16x8*>(a.ln_hl + (((long long)b * 4 + (n >> 4)) * a.P + pin) * 16 + h * 8) = hv;
              }
          }
        } else if (NCB == 1 && a.ln_hl) {
          // per-pixel LayerNorm over the 64 channels this lane (32 of them) and lane ^ 32 hold; biased variance, eps 1e-5
          typedef _Float16 st_f16x8 __attribute__((ext_vector_type(8)));
          float sm = 0.f;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) sm += acc[0][ni][e];
          sm += __shfl_xor(sm, 32, 64);
          const float mu = sm * (1.f / 64.f);
          float sq = 0.f;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) { const float d = acc[0][ni][e] - mu; sq = fmaf(d, d, sq); }
          sq += __shfl_xor(sq, 32, 64);
          const float rstd = 1.f / sqrtf(sq * (1.f / 64.f) + 1e-5f);
          if (pin < a.P) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
              for (int jj = 0; jj < 2; ++jj) {
                const int n = ni * 32 + jj * 16 + h * 8;               // 8 consecutive channels = half of chunk n >> 4
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.ln_g + n), g1 = *reinterpret_cast<const f32x4*>(a.ln_g + n + 4);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.ln_b + n), b1 = *reinterpret_cast<const f32x4*>(a.ln_b + n + 4);
                st_f16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const float y = (acc[0][ni][8 * jj + e] - mu) * rstd * (e < 4 ? g0[e & 3] : g1[e & 3]) + (e < 4 ? b0[e & 3] : b1[e & 3]);
                  hi[e] = (_Float16)y;
                  lo[e] = (_Float16)(y - (float)hi[e]);
                }
                _Float16* o16 = a.ln_hl + (((long long)b * 8 + (n >> 4)) * a.P + pin) * 16 + h * 8;
                *reinterpret_cast<st_f16x8*>(o16) = hi;
                *reinterpret_cast<st_f16x8*>(o16 + 4 * a.P * 16) = lo;
              }
          }
        }
        if (TAPS) {
          // Block cb = sub-pixel (cb >> 1, cb & 1) of the pixel-shuffled map.  acc[cb][ni][8 jj + q] = act(y)[channel 16 (2 ni + jj) +
          // 8 h + q] of this lane's pixel: exactly the B fragment (k = 8 h + q of chunk 2 ni + jj) of taps[k][pixel] = sum_c
          // w_last[c][k] act(y)[pixel][c] -- the accumulators feed the second product straight from registers.  Scaled per PIXEL by a
          // power of two into fp16's range (a column of the product may carry its own scale), split hi | lo: hi*hi + lo*hi + hi*lo.
          const int oy = (int)(pin / a.W), ox = (int)(pin - (long long)oy * a.W);
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) {
            float amax = 0.f;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
              for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(acc[cb][ni][e]));
            amax = fmaxf(amax, __shfl_xor(amax, 32, 64));              // the pixel's other 32 channels sit in lane ^ 32
            int ex = 0;
            if (amax > 0.f && amax < INFINITY) frexpf(amax, &ex);
            ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
            const float sc = ldexpf(1.f, 14 - ex), inv = ldexpf(1.f, ex - 14);
            f32x16 tacc;
#pragma unroll
            for (int e = 0; e < 16; ++e) tacc[e] = 0.f;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
              unsigned hh[4], ll[4];
#pragma unroll
              for (int j = 0; j < 4; ++j)
                split_pair_f16(acc[cb][s4 >> 1][8 * (s4 & 1) + 2 * j] * sc, acc[cb][s4 >> 1][8 * (s4 & 1) + 2 * j + 1] * sc, hh[j], ll[j]);
              const u32x4 hu = {hh[0], hh[1], hh[2], hh[3]}, lu = {ll[0], ll[1], ll[2], ll[3]};
              const f16x8_t yh = __builtin_bit_cast(f16x8_t, hu), yl = __builtin_bit_cast(f16x8_t, lu);
              tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(twl[s4], yh, tacc, 0, 0, 0);
              tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(twh[s4], yl, tacc, 0, 0, 0);
              tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(twh[s4], yh, tacc, 0, 0, 0);
            }
            // lane (pixel r, h): registers 0..3 = taps 4 h .. 4 h + 3, register 4 = tap 8 (h = 0)
            if (pin < a.P) {
              const long long opix = ((long long)b * 2 * (a.P / a.W) + 2 * oy + (cb >> 1)) * (2 * a.W) + 2 * ox + (cb & 1);
              float* op = a.out + opix * a.ldo;
              const f32x4 t4 = {tacc[0] * inv, tacc[1] * inv, tacc[2] * inv, tacc[3] * inv};
              *reinterpret_cast<f32x4*>(op + 4 * h) = t4;
              if (h == 0) op[8] = tacc[4] * inv;
            }
          }
        } else if (pin < a.P) {
          if (CSUM) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
              for (int e = 0; e < 16; ++e) cs[ni * 16 + e] += acc[0][ni][e];
          }
          float* op = a.out + ((long long)b * a.P + pin) * a.ldo;
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
              for (int jj = 0; jj < 2; ++jj) {
                const int n = cb * 64 + ni * 32 + jj * 16 + h * 8;
                if (n < a.Cout) {
                  f32x4 v0, v1;
#pragma unroll
                  for (int e = 0; e < 4; ++e) { v0[e] = acc[cb][ni][8 * jj + e]; v1[e] = acc[cb][ni][8 * jj + 4 + e]; }
                  *reinterpret_cast<f32x4*>(op + n) = v0;
                  *reinterpret_cast<f32x4*>(op + n + 4) = v1;
                }
              }
        }
      }
    }
    if (CSUM) {
      // ---- leaving image b: the workgroup's channel sums -> its slot.  Every item of the segment has been consumed, so the wave's
      // ring is idle: stage 0 takes the lanes' sums as [pixel lane r][64 channels]; summed in a fixed order (r ascending, then waves)
      float* red = reinterpret_cast<float*>(ring);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int n = ni * 32 + jj * 16 + h * 8;
          const f32x4 v0 = {cs[ni * 16 + 8 * jj], cs[ni * 16 + 8 * jj + 1], cs[ni * 16 + 8 * jj + 2], cs[ni * 16 + 8 * jj + 3]};
          const f32x4 v1 = {cs[ni * 16 + 8 * jj + 4], cs[ni * 16 + 8 * jj + 5], cs[ni * 16 + 8 * jj + 6], cs[ni * 16 + 8 * jj + 7]};
          *reinterpret_cast<f32x4*>(red + r * 64 + n) = v0;
          *reinterpret_cast<f32x4*>(red + r * 64 + n + 4) = v1;
        }
      __syncthreads();
      const int slot = (int)(blockIdx.x - st_owner((long long)b * a.tiles_per_image, a.tiles, gridDim.x));
      if (tid < 64 && slot >= 0 && slot < a.csum_slots) {
        float sw[4];
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
          const float* rw = reinterpret_cast<const float*>(smem + ring_off + wv * NS * ST_STAGE);
          float t = 0.f;
          for (int rr = 0; rr < 32; ++rr) t += rw[rr * 64 + tid];
          sw[wv] = t;
        }
        a.csum[((long long)b * a.csum_slots + slot) * 64 + tid] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
      }
      // (the barriers at the top of the next image's trip keep its DMAs behind these reads)
    }
    img_t0 = seg_hi;
  }
}

// ---- Statistics form: the alignment module's kf = act(W . [x0; x1]) (128 -> 64) is formed tile by tile like above and never
// stored.  What leaves the kernel per (image, workgroup segment) is what the fold kernels of stats.hip read:
//   gram[b][slot][c*(CH+2) + j]   j < CH: sum_p q[p][c] kf[p][head(c)*CH + j];  j == CH: sum q[p][c]^2;  j == CH+1: sum kf[p][c]^2
//   sum0 / sum1[b][slot][c]       channel sums of x0 / x1
// (cdfo_gram_partial's and cdfo_chan_sum_partial's layouts with "chunk" = slot, see st_owner; buffers zeroed by the caller).
// Per tile a wave streams three items through its ring: x0, x1 (the two K blocks) and q.  When q is consumed, the stage of the item
// before it (x1, already in the accumulators) is free until the next request is issued: the wave writes its 32 x 64 kf values there
// in the ring's own swizzled layout, and lane c forms row c of the Gram from the two stages in fp32 (one dword of q and of kf,
// CH/4 broadcast reads of the head's kf channels per pixel).  Sums are kept per tile and then added to the segment's running
// values, so no chain is longer than 32 + tiles-per-segment terms; waves and slots are summed in index order: deterministic.
struct sg_args {
  st_item src[3];                  // x0, x1, q
  const float* w; const float* bias; int act_fn;      // packed [128/4][64][4] weights, optional bias
  long long P; int tiles_per_image; long long tiles;
  float* gram; float* sum0; float* sum1; int slots;
  // PLANE form: x1 = stencil9 of a one-channel plane and never in memory.  src = {x0, q}; plane.w: the image-independent chunk table
  // W1 . [w_s | b_s] of the product's second half; stencil: the un-composed table [w_s | b_s] ([64][16]) that turns the ten tap sums
  // of a segment into sum1
  pc_plane plane; const float* stencil;
};
// MAP form: where the images of q lie (image_map.h); x0 and x1 stay dense.  A block of its own, as st_args_map
struct sg_args_map : sg_args {
  im_map q_map;
};

constexpr int SG_NS = 3;

template <int CH, bool PLANE = false, bool MAP = false>
__global__ __launch_bounds__(ST_THREADS) void align_gram_partial_kernel(std::conditional_t<MAP, sg_args_map, sg_args> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NS = SG_NS, NKB = PLANE ? 1 : 2, IPT = NKB + 1, GS = CH + 2;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // LDS map as conv1x1_stream_kernel<1>: weights hi | lo (8 KB per K block each) | bias | 4 waves x NS stages
  constexpr int w_half = NKB * 4 * 2 * 64 * 16;
  constexpr int ring_off = 2 * w_half + 64 * 4;
  unsigned char* sWh = smem;
  unsigned char* sWl = smem + w_half;
  float* sBias = reinterpret_cast<float*>(smem + 2 * w_half);
  unsigned char* ring = smem + ring_off + wave * NS * ST_STAGE;
  const unsigned ring_lds = (unsigned)(unsigned long long)(smem) + ring_off + wave * NS * ST_STAGE;
  // PLANE: behind the rings the chunk's weight image hi | lo, then NS tap slots per wave (as conv1x1_stream_kernel)
  unsigned char* sPh = smem + ring_off + 4 * NS * ST_STAGE;
  unsigned char* sPl = sPh + pc_weight_bytes(1) / 2;
  const unsigned char* tap_slots = sPh + pc_weight_bytes(1) + wave * NS * PC_SLOT;
  const unsigned tap_lds = (unsigned)(unsigned long long)(smem) + ring_off + 4 * NS * ST_STAGE + pc_weight_bytes(1) + wave * NS * PC_SLOT;

  const long long t_lo = a.tiles * blockIdx.x / gridDim.x, t_hi = a.tiles * (blockIdx.x + 1) / gridDim.x;
  if (t_lo >= t_hi) return;
  const float slope = a.act_fn == CDFO_ACT_NONE ? 1.f : (a.act_fn == CDFO_ACT_LRELU ? 0.1f : 0.f);

  int d_px[8], d_part[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int s = 64 * k + lane, p = s >> 4;
    d_px[k] = p;
    d_part[k] = (s & 15) ^ (p & 15);
  }
  auto part_off = [&](int q) { return r * 256 + ((q ^ (r & 15)) << 4); };

  // ---- the weights (the same for every image) -> LDS, split bf16 hi | lo, rows permuted
  for (int i = tid; i < (NKB * 64 >> 2) * 64; i += ST_THREADS) {      // PLANE: the first 64 input channels of the 128 -> 64 packing
    const int rowpos = i % 64, kg = i / 64;
    const int n = mfma_row_channel(rowpos);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(a.w + ((long long)kg * 64 + n) * 4);
    const int c = kg >> 2, hh = (kg >> 1) & 1, j0 = (kg & 1) * 4;
    u32x2 hi, lo;
    split4_bf16(wv, hi, lo);
    const int off = ((c * 2 + hh) * 64 + rowpos) * 16 + j0 * 2;
    *reinterpret_cast<u32x2*>(sWh + off) = hi;
    *reinterpret_cast<u32x2*>(sWl + off) = lo;
  }
  for (int i = tid; i < 64; i += ST_THREADS) sBias[i] = a.bias ? a.bias[i] : 0.f;
  if (PLANE) pc_load_weights<1>(a.plane.w, 64, sPh, sPl, tid);      // (the barrier of the first image's trip publishes them)

  // lane c of the statistics phases: channel c of q / kf / x0 / x1 of pixel p sits at p*256 + (((c >> 2) ^ (p & 15)) << 4) + (c & 3)*4
  const int c_part = lane >> 2, c_sub = (lane & 3) * 4, h_part = (lane / CH) * CH / 4;

  for (long long img_t0 = t_lo; img_t0 < t_hi;) {
    const int b = (int)(img_t0 / a.tiles_per_image);
    const long long img_end = (long long)(b + 1) * a.tiles_per_image;
    const long long seg_hi = img_end < t_hi ? img_end : t_hi;
    __syncthreads();       // weights are in LDS / the previous segment's reduction has read the rings; no DMA is in flight here

    const long long n_items = (seg_hi - img_t0) * IPT;
    long long issued = 0;
    auto issue = [&](long long it) {
      const long long tile = img_t0 + it / IPT;
      const st_item src = a.src[(int)(it % IPT)];
      const long long p0 = (tile - (long long)b * a.tiles_per_image) * 128 + wave * 32;
      if (PLANE && it % IPT == 0)      // the tile's taps, ahead of its first item (plane_chunk.h; the slot rules with ipt = 2)
        pc_issue(pc_image(a.plane, b), (int)a.P, a.plane.W, (int)p0, lane, tap_lds + (unsigned)((it / IPT) % NS) * PC_SLOT);
      const long long rows_left = a.P - p0;                               // may be <= 0: everything out of range
      // (MAP: q, the tile's last item, lies where q_map says; the descriptor still ends with this image's last pixel)
      const float* base = src.base + ((long long)b * a.P + (rows_left > 0 ? p0 : 0)) * src.ld + src.ch0;
      if constexpr (MAP) {
        if (it % IPT == IPT - 1) base = src.base + im_offset(a.q_map, b) + (rows_left > 0 ? p0 : 0) * src.ld + src.ch0;
      }
      i32x4 rsrc = lds_dma_rsrc_uniform(base, 0u);
      const long long bytes = rows_left > 0 ? (rows_left < 32 ? rows_left : 32) * (long long)src.ld * 4 : 0;
      lds_dma_rsrc_resize_uniform(rsrc, (unsigned)bytes);                 // lanes beyond the image read zeros
      unsigned voff[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) voff[q] = (unsigned)(d_px[q] * src.ld * 4 + d_part[q] * 16);
      lds_dma0(voff, rsrc, __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)(it % NS) * ST_STAGE));
    };
    for (; issued < NS - 1 && issued < n_items; ++issued) issue(issued);

    f32x16 acc[2];
    float g[CH], sq = 0.f, sk = 0.f, sx[2] = {0.f, 0.f};     // the segment's running sums of lane c
    // PLANE: this lane's running sums of the nine taps of its pixels as they enter the product, and the count of pixels inside
    float ts[PLANE ? 10 : 1];
#pragma unroll
    for (int j = 0; j < (PLANE ? 10 : 1); ++j) ts[j] = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j) g[j] = 0.f;
    for (long long it = 0; it < n_items; ++it) {
      const int k = (int)(it % IPT);
      if (!PLANE) st_wait_landed(issued - it - 1);
      else {
        // IPT = 2, NS = 3: the requests run NS - 1 = 2 items ahead, so at most ONE item younger than `it` is in flight.  The order of
        // the wave's pieces is ... [x0(t): 8] [q(t): 8] [taps(t + 1): 3] [x0(t + 1): 8] [q(t + 1): 8] ...
        if (issued - it - 1 == 0) wait_vm<0>();      // the segment's last item: nothing younger, 0
        else if (k == 0) wait_vm<8>();               // x0(t): q(t) is younger, 8 pieces; taps(t) are older than x0(t): landed with it
        else wait_vm<11>();                          // q(t): taps(t + 1) and x0(t + 1) are younger, 3 + 8 = 11 pieces
      }
      const unsigned char* st = ring + (it % NS) * ST_STAGE;
      if (k == 0) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
      }
      if (k < NKB) {
        // ---- one K block of the product, as conv1x1_stream_kernel
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(st + part_off(c * 4 + h * 2));
          const f32x4 v1 = *reinterpret_cast<const f32x4*>(st + part_off(c * 4 + h * 2 + 1));
          union { unsigned u[4]; bf16x8_t v; } ph, pl;
          split8_bf16(v0, v1, ph.u, pl.u);
          const int wrow = ((k * 4 + c) * 2 + h) * 64 + r;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const bf16x8_t wh = *reinterpret_cast<const bf16x8_t*>(sWh + (wrow + ni * 32) * 16);
            const bf16x8_t wl = *reinterpret_cast<const bf16x8_t*>(sWl + (wrow + ni * 32) * 16);
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, pl.v, acc[ni], 0, 0, 0);
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ph.v, acc[ni], 0, 0, 0);
            acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ph.v, acc[ni], 0, 0, 0);
          }
        }
        // ---- channel sum of this operand over the wave's 32 pixels (rows beyond the image arrived as zeros)
        float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 32; ++p)
          t4[p & 3] += *reinterpret_cast<const float*>(st + p * 256 + ((c_part ^ (p & 15)) << 4) + c_sub);
        sx[k] += (t4[0] + t4[1]) + (t4[2] + t4[3]);
        if (PLANE) {
          // the plane chunk's k-step closes the tile's product (x1 = stencil9 of the plane): the tile's slot landed before x0 (requested
          // ahead of it) and is read here, with the tile's first item, before the request below can reuse any slot (plane_chunk.h)
          const int p = (int)((img_t0 + it / IPT - (long long)b * a.tiles_per_image) * 128) + wave * 32 + r;
          unsigned thi[4], tlo[4];
          float t9[9];
          pc_operand<true>(tap_slots + ((it / IPT) % NS) * PC_SLOT, r, h, p, (int)a.P, a.plane.W, thi, tlo, t9);
          f32x16 pacc[1][2] = {{acc[0], acc[1]}};
          pc_mfma<1>(sPh, sPl, r, h, thi, tlo, pacc);
          acc[0] = pacc[0][0];
          acc[1] = pacc[0][1];
#pragma unroll
          for (int j = 0; j < 9; ++j) ts[j] += t9[j];
          ts[PLANE ? 9 : 0] += p < (int)a.P ? 1.f : 0.f;
        }
        if (k == NKB - 1) {      // bias + activation: acc[ni][8 jj + q] = kf channel ni*32 + jj*16 + h*8 + q of pixel r; zero beyond the image
          const long long pin = (img_t0 + it / IPT - (long long)b * a.tiles_per_image) * 128 + wave * 32 + r;
          const bool inside = pin < a.P;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const float t = acc[ni][e] + sBias[ni * 32 + (e >> 3) * 16 + h * 8 + (e & 7)];
              acc[ni][e] = inside ? fmaxf(t, 0.f) + slope * fminf(t, 0.f) : 0.f;
            }
        }
      } else {
        // ---- q has landed: kf -> the stage of the item before (x1's; PLANE: x0's -- already in the accumulators and in sx[0], free
        // until the request below), then row c of the Gram
        unsigned char* kst = ring + ((it - 1) % NS) * ST_STAGE;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int q0 = (ni * 32 + jj * 16 + h * 8) >> 2;
            const f32x4 v0 = {acc[ni][8 * jj], acc[ni][8 * jj + 1], acc[ni][8 * jj + 2], acc[ni][8 * jj + 3]};
            const f32x4 v1 = {acc[ni][8 * jj + 4], acc[ni][8 * jj + 5], acc[ni][8 * jj + 6], acc[ni][8 * jj + 7]};
            *reinterpret_cast<f32x4*>(kst + part_off(q0)) = v0;
            *reinterpret_cast<f32x4*>(kst + part_off(q0 + 1)) = v1;
          }
        float gt[CH], tq = 0.f, tk = 0.f;
#pragma unroll
        for (int j = 0; j < CH; ++j) gt[j] = 0.f;
#pragma unroll
        for (int p = 0; p < 32; ++p) {
          const int own = p * 256 + ((c_part ^ (p & 15)) << 4) + c_sub;
          const float qv = *reinterpret_cast<const float*>(st + own);
          const float kc = *reinterpret_cast<const float*>(kst + own);
          tq = fmaf(qv, qv, tq);
          tk = fmaf(kc, kc, tk);
#pragma unroll
          for (int j4 = 0; j4 < CH / 4; ++j4) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kst + p * 256 + (((h_part + j4) ^ (p & 15)) << 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) gt[j4 * 4 + e] = fmaf(qv, kv[e], gt[j4 * 4 + e]);
          }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) g[j] += gt[j];
        sq += tq;
        sk += tk;
      }
      // this item's (and the kf stage's) LDS reads have returned before the next request overwrites the stage of item it - 1
      if (issued < n_items) { wait_lgkm<0>(); issue(issued); ++issued; }
    }

    // ---- leaving image b: the four waves' sums (each in stage 0 of its idle ring) -> this workgroup's slot, waves in index order
    {
      float* red = reinterpret_cast<float*>(ring);
#pragma unroll
      for (int j = 0; j < CH; ++j) red[lane * GS + j] = g[j];
      red[lane * GS + CH] = sq;
      red[lane * GS + CH + 1] = sk;
      red[64 * GS + lane] = sx[0];
      if (!PLANE) red[64 * GS + 64 + lane] = sx[1];
      else {
        // the ten tap sums over the wave's 32 pixels, a fixed tree (both k-halves hold the same taps): ten numbers per wave
#pragma unroll
        for (int j = 0; j < 10; ++j) {
          float v = ts[j];
#pragma unroll
          for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m, 64);
          if (lane == 0) red[64 * GS + 64 + j] = v;
        }
      }
      __syncthreads();
      const int slot = (int)(blockIdx.x - st_owner((long long)b * a.tiles_per_image, a.tiles, gridDim.x));
      if (slot >= 0 && slot < a.slots) {
        const float* r0 = reinterpret_cast<const float*>(smem + ring_off);
        const float* r1 = reinterpret_cast<const float*>(smem + ring_off + 1 * NS * ST_STAGE);
        const float* r2 = reinterpret_cast<const float*>(smem + ring_off + 2 * NS * ST_STAGE);
        const float* r3 = reinterpret_cast<const float*>(smem + ring_off + 3 * NS * ST_STAGE);
        const long long bs = (long long)b * a.slots + slot;
        for (int i = tid; i < 64 * GS + 128; i += ST_THREADS) {
          const float v = (r0[i] + r1[i]) + (r2[i] + r3[i]);
          if (i < 64 * GS) a.gram[bs * (64 * GS) + i] = v;
          else if (i < 64 * GS + 64) a.sum0[bs * 64 + (i - 64 * GS)] = v;
          else if (!PLANE) a.sum1[bs * 64 + (i - 64 * GS - 64)] = v;
          else {
            // sum1[c] = sum_t w_s[c][t] S_t + b_s[c] count: the channel sum of stencil9 over the segment from its ten tap sums
            // (waves in index order like every other sum here, then t ascending)
            const int c = i - 64 * GS - 64;
            float s1 = 0.f;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
              const int o = 64 * GS + 64 + j;
              s1 = fmaf(a.stencil[c * 16 + j], (r0[o] + r1[o]) + (r2[o] + r3[o]), s1);
            }
            a.sum1[bs * 64 + c] = s1;
          }
        }
      }
    }
    img_t0 = seg_hi;
  }
}

}  // namespace

// Pure host arithmetic of the partial slots (no device needed): slots per image written by a launch of `grid` workgroups, and the
// slot that workgroup `wg` writes for image b (-1: it holds no tile of b).
extern "C" int cdfo_stream_slots_for_grid(int B, long long P, int grid) {
  if (B <= 0 || P <= 0 || grid <= 0 || (P + 127) / 128 > 0x7fffffff / 2) return CDFO_EINVAL;
  const int tpi = (int)((P + 127) / 128);
  const long long tiles = (long long)B * tpi;
  return st_slots(B, tpi, (int)(tiles < grid ? tiles : grid));
}
extern "C" int cdfo_stream_slot_of(int B, long long P, int grid, int wg, int b) {
  if (B <= 0 || P <= 0 || grid <= 0 || wg < 0 || b < 0 || b >= B) return CDFO_EINVAL;
  const int tpi = (int)((P + 127) / 128);
  const long long tiles = (long long)B * tpi;
  const int g = (int)(tiles < grid ? tiles : grid);
  if (wg >= g) return -1;
  const long long t_lo = tiles * wg / g, t_hi = tiles * (wg + 1) / g;
  const long long lo = t_lo > (long long)b * tpi ? t_lo : (long long)b * tpi, hi = t_hi < (long long)(b + 1) * tpi ? t_hi : (long long)(b + 1) * tpi;
  if (lo >= hi) return -1;
  return (int)(wg - st_owner((long long)b * tpi, tiles, g));
}
// slots per image of the launches the CALLING THREAD would make now (its CU share): cdfo_align_stats and the channel-sum output of
// cdfo_conv1x1_bf16x3 use the same cut of the tile stream
extern "C" int cdfo_align_stats_slots(int B, long long P) {
  const int cus = cdfo_num_cus();
  if (cus <= 0) return CDFO_EINVAL;
  return cdfo_stream_slots_for_grid(B, P, cus);
}

// pl != null: cdfo_align_stats_plane (x1 is the plane's stencil: x1 == null, ld1 unused)
static int align_stats(const float* x0, int ld0, const float* x1, int ld1, const float* q, int ldq, const float* w_packed, const float* bias,
                       int act, int ch_per_head, int B, long long P, int nslots, float* gram_partial, float* sum0_partial,
                       float* sum1_partial, const pc_plane* pl, const float* stencil, const im_map* qm, void* stream) {
  if (qm && !im_map_ok(*qm)) return CDFO_EINVAL;
  if (B <= 0 || P <= 0 || nslots <= 0 || !x0 || (!x1 && !pl) || !q || !w_packed || !gram_partial || !sum0_partial || !sum1_partial) return CDFO_EINVAL;
  if (act != CDFO_ACT_NONE && act != CDFO_ACT_LRELU && act != CDFO_ACT_RELU) return CDFO_EINVAL;
  if (ch_per_head != 8 && ch_per_head != 16) return CDFO_EINVAL;
  const int lds_[3] = {ld0, pl ? 64 : ld1, ldq};
  for (int i = 0; i < 3; ++i)
    if (lds_[i] < 64 || lds_[i] % 4 || (long long)lds_[i] * 4 * 32 >= (1ll << 31)) return CDFO_EINVAL;
  if (!aligned16(x0) || !aligned16(x1) || !aligned16(q) || !aligned16(w_packed) || !aligned16(gram_partial) || !aligned16(sum0_partial) ||
      !aligned16(sum1_partial))
    return CDFO_EALIGN;
  if ((P + 127) / 128 > 0x7fffffff / 2) return CDFO_EINVAL;
  if (pl) {
    // a plane outside the chunk's contract is an error: there is no other kernel for this form
    if (!pl->base || !pl->w || !stencil || pl->Bi <= 0 || pl->s_b < 0 || pl->s_g < 0 || !pc_shape_ok(P, pl->W)) return CDFO_EINVAL;
    if ((unsigned long long)pl->base % 4 || !aligned16(pl->w) || !aligned16(stencil)) return CDFO_EALIGN;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  sg_args_map sm{};
  sg_args& s = sm;
  s.src[0] = {x0, ld0, 0};
  if (pl) { s.src[1] = {q, ldq, 0}; s.plane = *pl; s.stencil = stencil; }
  else { s.src[1] = {x1, ld1, 0}; s.src[2] = {q, ldq, 0}; }
  s.w = w_packed; s.bias = bias; s.act_fn = act;
  s.P = P;
  s.gram = gram_partial; s.sum0 = sum0_partial; s.sum1 = sum1_partial; s.slots = nslots;
  if (qm) sm.q_map = *qm;
  int grid;
  if (!st_tiling(B, P, s.tiles_per_image, s.tiles, grid)) return CDFO_EINVAL;
  if (nslots < st_slots(B, s.tiles_per_image, grid)) return CDFO_EINVAL;
  const double px = (double)B * P;
  if (pl) {
    const int lds = st_lds_bytes(1, 1, SG_NS) + pc_lds_bytes(1, SG_NS);
    static_assert(st_lds_bytes(1, 1, SG_NS) + pc_lds_bytes(1, SG_NS) <= ST_MAX_LDS, "the PLANE form's LDS (128256 bytes)");
    // (the plane chunk: one k-step of 16 instead of a K block of 64, 4 bytes per pixel instead of 256)
    CdfoProfScope prof(st, KID_GRAM, px * (2.0 * 80 * 64 + 2.0 * 64 * 18), 4.0 * 129 * px);
    static CdfoAttrOnce once8p, once16p, once8pm, once16pm;
    if (qm)
      return ch_per_head == 16 ? st_launch(align_gram_partial_kernel<16, true, true>, once16pm, grid, lds, st, sm)
                               : st_launch(align_gram_partial_kernel<8, true, true>, once8pm, grid, lds, st, sm);
    return ch_per_head == 16 ? st_launch(align_gram_partial_kernel<16, true>, once16p, grid, lds, st, s)
                             : st_launch(align_gram_partial_kernel<8, true>, once8p, grid, lds, st, s);
  }
  const int lds = st_lds_bytes(2, 1, SG_NS);
  CdfoProfScope prof(st, KID_GRAM, px * (2.0 * 128 * 64 + 2.0 * 64 * 18), 4.0 * 192 * px);
  static CdfoAttrOnce once8, once16, once8m, once16m;
  if (qm)
    return ch_per_head == 16 ? st_launch(align_gram_partial_kernel<16, false, true>, once16m, grid, lds, st, sm)
                             : st_launch(align_gram_partial_kernel<8, false, true>, once8m, grid, lds, st, sm);
  return ch_per_head == 16 ? st_launch(align_gram_partial_kernel<16>, once16, grid, lds, st, s)
                           : st_launch(align_gram_partial_kernel<8>, once8, grid, lds, st, s);
}

extern "C" int cdfo_align_stats(const float* x0, int ld0, const float* x1, int ld1, const float* q, int ldq, const float* w_packed,
                                const float* bias, int act, int ch_per_head, int B, long long P, int nslots, float* gram_partial,
                                float* sum0_partial, float* sum1_partial, void* stream) {
  if (!x1) return CDFO_EINVAL;
  return align_stats(x0, ld0, x1, ld1, q, ldq, w_packed, bias, act, ch_per_head, B, P, nslots, gram_partial, sum0_partial, sum1_partial,
                     nullptr, nullptr, nullptr, stream);
}

extern "C" int cdfo_align_stats_plane(const float* x0, int ld0, const float* q, int ldq, const float* w_packed, const float* bias, int act,
                                      int ch_per_head, int B, long long P, int nslots, float* gram_partial, float* sum0_partial,
                                      float* sum1_partial, const float* plane, int plane_Bi, long long plane_sb, long long plane_sg,
                                      int W, const float* plane_w, const float* stencil_w, void* stream) {
  const pc_plane pl = {plane, plane_Bi, plane_sb, plane_sg, W, plane_w, 0};
  return align_stats(x0, ld0, nullptr, 0, q, ldq, w_packed, bias, act, ch_per_head, B, P, nslots, gram_partial, sum0_partial, sum1_partial,
                     &pl, stencil_w, nullptr, stream);
}

// cdfo_align_stats (plane == null: x1 in memory) / cdfo_align_stats_plane with q read through an image map: image b of q starts at
// q + (b % q_Bi) q_sb + (b / q_Bi) q_sg floats (image_map.h).  Same results bit for bit as on the dense copy of those images.
extern "C" int cdfo_align_stats_map(const float* x0, int ld0, const float* x1, int ld1, const float* q, int ldq, int q_Bi, long long q_sb,
                                    long long q_sg, const float* w_packed, const float* bias, int act, int ch_per_head, int B, long long P,
                                    int nslots, float* gram_partial, float* sum0_partial, float* sum1_partial, const float* plane,
                                    int plane_Bi, long long plane_sb, long long plane_sg, int W, const float* plane_w,
                                    const float* stencil_w, void* stream) {
  const im_map qm = {q_Bi, q_sb, q_sg};
  if (!plane) {
    if (!x1) return CDFO_EINVAL;
    return align_stats(x0, ld0, x1, ld1, q, ldq, w_packed, bias, act, ch_per_head, B, P, nslots, gram_partial, sum0_partial, sum1_partial,
                       nullptr, nullptr, &qm, stream);
  }
  const pc_plane pl = {plane, plane_Bi, plane_sb, plane_sg, W, plane_w, 0};
  return align_stats(x0, ld0, nullptr, 0, q, ldq, w_packed, bias, act, ch_per_head, B, P, nslots, gram_partial, sum0_partial, sum1_partial,
                     &pl, stencil_w, &qm, stream);
}

// Returns 1 when the streaming kernel took the launch, 0 when the shapes are outside its contract (the caller falls back to
// cdfo_conv1x1_bf16x3), < 0 / hipError_t on errors.  Same argument block as cdfo_conv1x1_bf16x3.
// plane != null: the PLANE form, or 0
// maps != null: the MAP form -- maps[i] locates the images of source i (i < nsrc), maps[CDFO_MAXSRC] / [CDFO_MAXSRC + 1] those of res1 /
// res2; Bi == 0: that operand is dense.  64 output channels, no second output, no scaled residual; or 0
int cdfo_conv1x1_stream_try(const cdfo_conv_args& a, hipStream_t st, const pc_plane* pl, const im_map* maps) {
  const bool ln_out = a.out2_cp16 != nullptr;      // post-LayerNorm hi | lo second output (checked by the caller: Cout == 64)
  const bool taps = a.store_mode == CDFO_STORE_TAPS9;
  if (taps && (pl || maps)) return 0;
  if (taps) {
    // upconv2 + conv_last's tap sums (checked by the caller: Cout = CoutP = 256, res2 = conv_last.weight [64][9], no res1)
    if (a.Cin != 64 || a.nsrc != 1 || a.ldo % 4 || a.ldo < 12 || a.ln_gamma || ln_out || (long long)a.ld[0] * 4 * 32 >= (1ll << 31)) return 0;
    st_args s{};
    s.act[0].base = a.src[0]; s.act[0].ld = a.ld[0]; s.act[0].ch0 = 0;
    s.nkb = 1;
    s.w = a.w; s.w_bstride = a.w_bstride; s.bias = a.bias;
    s.Cin = 64; s.Cout = 256; s.CoutP = 256; s.act_fn = a.act;
    s.out = a.out; s.ldo = a.ldo; s.B = a.B; s.P = (long long)a.H * a.W;
    s.w_last = a.res2; s.W = a.W;
    s.ns = 2;
    int grid;
    if (!st_tiling(a.B, s.P, s.tiles_per_image, s.tiles, grid)) return CDFO_EINVAL;
    const double px = (double)a.B * s.P;
    CdfoProfScope prof(st, KID_CONV1, 2.0 * px * 256 * 64 + 2.0 * px * 4 * 9 * 64, 4.0 * (px * 64 + px * 4 * a.ldo + 64.0 * 256));
    static CdfoAttrOnce once;
    const int e = st_launch(conv1x1_stream_kernel<4, true>, once, grid, st_lds_bytes(1, 4, s.ns), st, s);
    return e == 0 ? 1 : e;
  }
  if (a.store_mode != CDFO_STORE_PLAIN || (a.ln_gamma && !ln_out) || a.CoutP % 64 || a.CoutP > 128 || a.Cout % 8) return 0;      // (ln_out without ln_gamma: plain fp16 copy)
  const bool plane = pl != nullptr;
  // the plane chunk: 64 output channels, no second output, no scaled residual (its LDS lies where the factors' slots would)
  if (plane && (a.CoutP != 64 || ln_out || a.res2_pixscale || !pc_shape_ok((long long)a.H * a.W, a.W))) return 0;
  if (ln_out && (a.CoutP != 64 || a.Cout != 64)) return 0;
  if (maps && (a.CoutP != 64 || ln_out || a.res2_pixscale)) return 0;
  if (a.chan_sum_out && (a.CoutP != 64 || a.Cout != 64 || ln_out || a.chan_sum_slots <= 0)) return 0;   // the caller sums in a pass of its own
  const int ncb = a.CoutP / 64, nkb = a.Cin / 64;
  if (nkb < 1 || nkb > CDFO_MAXSRC * 4) return 0;
  const int w_bytes = st_weight_bytes(nkb, ncb);
  const int scale_bytes = (a.res2 && a.res2_pixscale) ? 4 * 512 : 0;      // two tile-parity slots per wave
  int ns = plane ? (ST_MAX_LDS - w_bytes - pc_weight_bytes(ncb)) / (4 * (ST_STAGE + PC_SLOT)) : (ST_MAX_LDS - scale_bytes - w_bytes) / (4 * ST_STAGE);
  if (ns > ST_MAXNS) ns = ST_MAXNS;
  if (scale_bytes) {
    // the per-pixel factors of tile t + 2 are requested with item (t + 2, 0), NS - 1 items ahead of consumption, into the slot tile t
    // used (two tile-parity slots): safe only while NS <= items_per_tile + 2, or tile t's residual stage would read tile t + 2's factors
    const int items_per_tile = nkb + ((a.res1 ? 1 : 0) + 1) * ncb;      // as the kernel counts them: K blocks + residual stages
    if (ns > items_per_tile + 2) ns = items_per_tile + 2;
  }
  if (ns < 3) return 0;
  const long long P = (long long)a.H * a.W;
  st_args_map sm{};
  st_args& s = sm;
  int k = 0;
  for (int i = 0; i < a.nsrc; ++i) {
    if ((long long)a.ld[i] * 4 * 32 >= (1ll << 31)) return 0;
    for (int c = 0; c < a.cs[i]; c += 64) {
      s.act[k].base = a.src[i]; s.act[k].ld = a.ld[i]; s.act[k].ch0 = c;
      if (maps) sm.act_map[k] = maps[i].Bi ? maps[i] : im_dense(a.B, P, a.ld[i]);
      ++k;
    }
  }
  if (k != nkb) return 0;
  s.nkb = nkb;
  // residual operands are staged 64 channels at a time: they must be at least NCB*64 channels wide in memory terms only
  // where Cout needs it (a narrower tensor would be read past its pitch): require ld >= CoutP
  int nr = 0;
  if (a.res1) {
    if (a.ldr1 < a.CoutP) return 0;
    s.res[nr].base = a.res1; s.res[nr].ld = a.ldr1;
    if (maps) sm.res_map[nr] = maps[CDFO_MAXSRC].Bi ? maps[CDFO_MAXSRC] : im_dense(a.B, P, a.ldr1);
    ++nr;
  }
  if (a.res2) {
    if (a.ldr2 < a.CoutP) return 0;
    s.res[nr].base = a.res2; s.res[nr].ld = a.ldr2;
    if (maps) sm.res_map[nr] = maps[CDFO_MAXSRC + 1].Bi ? maps[CDFO_MAXSRC + 1] : im_dense(a.B, P, a.ldr2);
    ++nr;
  }
  s.res_scale = a.res2 ? a.res2_pixscale : nullptr;
  s.w = a.w; s.w_bstride = a.w_bstride; s.bias = a.bias;
  s.Cin = a.Cin; s.Cout = a.Cout; s.CoutP = a.CoutP; s.act_fn = a.act;
  s.out = a.out; s.ldo = a.ldo; s.B = a.B; s.P = P;
  s.ln_hl = ln_out ? static_cast<_Float16*>(a.out2_cp16) : nullptr; s.ln_g = a.ln_gamma; s.ln_b = a.ln_beta;
  s.ns = ns;
  int grid;
  if (!st_tiling(a.B, P, s.tiles_per_image, s.tiles, grid)) return CDFO_EINVAL;
  const int lds = st_lds_bytes(nkb, ncb, ns) + scale_bytes + (plane ? pc_lds_bytes(ncb, ns) : 0);
  const double px = (double)a.B * P;
  if (plane) { s.plane = *pl; s.plane.W = a.W; }
  // (the plane chunk: one k-step of 16 and 4 bytes per pixel more)
  CdfoProfScope prof(st, KID_CONV1, 2.0 * px * a.Cout * (a.Cin + (plane ? 16 : 0)),
                     4.0 * (px * a.Cout * (1 + nr) + px * a.Cin + (plane ? px : 0.0) + (double)a.Cin * a.Cout));
  if (a.chan_sum_out) {
    // (checked above: ncb == 1, Cout == 64) the result's channel sums from the epilogue's registers, one slot per (image, workgroup segment)
    if (a.chan_sum_slots < st_slots(a.B, s.tiles_per_image, grid)) return 0;
    s.csum = a.chan_sum_out; s.csum_slots = a.chan_sum_slots;
  }
  static CdfoAttrOnce once_csum, once1, once2, once_pl, once_pl_csum, once_map[4];
  if (maps) {
    const int e = plane ? (a.chan_sum_out ? st_launch(conv1x1_stream_kernel<1, false, true, true, true>, once_map[3], grid, lds, st, sm)
                                          : st_launch(conv1x1_stream_kernel<1, false, false, true, true>, once_map[2], grid, lds, st, sm))
                        : (a.chan_sum_out ? st_launch(conv1x1_stream_kernel<1, false, true, false, true>, once_map[1], grid, lds, st, sm)
                                          : st_launch(conv1x1_stream_kernel<1, false, false, false, true>, once_map[0], grid, lds, st, sm));
    return e == 0 ? 1 : e;
  }
  if (plane) {
    const int e = a.chan_sum_out ? st_launch(conv1x1_stream_kernel<1, false, true, true>, once_pl_csum, grid, lds, st, s)
                                 : st_launch(conv1x1_stream_kernel<1, false, false, true>, once_pl, grid, lds, st, s);
    return e == 0 ? 1 : e;
  }
  const int e = a.chan_sum_out ? st_launch(conv1x1_stream_kernel<1, false, true>, once_csum, grid, lds, st, s)
                : ncb == 1     ? st_launch(conv1x1_stream_kernel<1>, once1, grid, lds, st, s)
                               : st_launch(conv1x1_stream_kernel<2>, once2, grid, lds, st, s);
  return e == 0 ? 1 : e;
}
