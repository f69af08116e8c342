// The "plane chunk" of the persistent stream kernels (conv1x1_stream.hip, attention.hip's rdab_prep_kernel_fused): a 64-channel
// operand that is a 3x3 stencil of a ONE-channel plane, stencil9(plane; w_s, b_s), enters a 1x1 product W . [...] without existing in
// memory.  W . stencil9 is a 1x1 convolution of ten numbers per pixel -- the nine neighbours and a constant 1 -- with the weights
// W . [w_s | b_s] (composed on the host in float64), i.e. ONE more 16-wide k-step of the split-bf16 product: 6 MFMAs per 64 output
// channels and tile.  The pixel operand of lane (pixel r, k-half h) is built in registers as rdab_stats.hip builds its stem block:
// half 0 = taps 0..7, half 1 = tap 8, 1.0, six zeros; tap t = plane(y + t / 3 - 1, x + t % 3 - 1), zero outside the image.
//
// Fetching the taps.  An ordinary load would be waited for with vmcnt(0) at its use and drain the wave's ring (see res_scale in
// conv1x1_stream.hip); as there, the taps arrive by LDS-DMA: per (tile, wave) three dword pieces, requested AHEAD of the tile's first
// item.  Lane l < 34 of piece dy fetches flattened plane element p0 + (dy - 1) W - 1 + l (p0 = the wave's first pixel), the 34
// elements under the three-wide windows of its 32 pixels in image row offset dy - 1; the descriptor covers THAT image's plane only
// (P * 4 bytes) and a lane whose element lies outside [0, P) asks for an out-of-range offset, so rows above and below the image read
// zero and nothing of a neighbouring plane is touched.  Consumer lane r takes slot[dy][r + dx] and zeroes the tap when x + dx - 1
// leaves [0, W): a wave's 32 pixels may span several image rows, and the flattened neighbour of a row's first / last pixel belongs to
// another row.  Memory operations retire in order, so a tile's slot is valid once any of its items has landed; the hand-counted
// st_wait_landed arguments of the kernels stay valid, older pieces in flight only make them more conservative.
//
// Slots.  A wave owns NS slots (NS = its ring's stage count), indexed by the tile's rank in the segment modulo NS, and consumes a
// tile's slot with the tile's FIRST item.  The request of tile t + NS (the first that reuses the slot of tile t) goes out with that
// tile's first item, NS - 1 items ahead of its consumption: after item NS (ipt - 1) + 1 >= 1 past tile t's first item has been
// consumed, ipt >= 1 items per tile -- always behind the read of slot t.
#pragma once
#include "stream_ring.h"

struct pc_plane {
  const float* base; int Bi; long long s_b, s_g;   // image m's plane (H x W fp32, dense) at base + (m % Bi) s_b + (m / Bi) s_g
  int W;
  const float* w; long long w_bstride;             // the chunk's weights [CoutP][16] fp32: taps 0..8, the bias column, zeros
};

namespace {

constexpr int PC_SLOT = 3 * 256;                 // three pieces of 64 lanes x 4 bytes
constexpr unsigned PC_OUTSIDE = 0x80000000u;     // an offset beyond every descriptor: the lane's LDS bytes receive zero

// ---- host side: LDS behind the rings -- the chunk's weight image (hi | lo, [2 k-halves][ncb * 64 rows][8 bf16] each), then the slots
__host__ __device__ constexpr int pc_weight_bytes(int ncb) { return 2 * (2 * ncb * 64 * 16); }
__host__ __device__ constexpr int pc_lds_bytes(int ncb, int ns) { return pc_weight_bytes(ncb) + 4 * ns * PC_SLOT; }
// what the 32-bit tap indices and byte offsets need
inline bool pc_shape_ok(long long P, int W) { return W > 0 && P > 0 && P % W == 0 && P + 2ll * W + 64 < (1ll << 29); }

__device__ __forceinline__ const float* pc_image(const pc_plane& pl, int m) {
  return pl.base + (long long)(m % pl.Bi) * pl.s_b + (long long)(m / pl.Bi) * pl.s_g;
}

// the chunk's weights of one image -> LDS, split bf16 hi | lo, rows permuted like the kernels' own weight images (all threads)
template <int NCB>
__device__ __forceinline__ void pc_load_weights(const float* w16, int CoutP, unsigned char* sPh, unsigned char* sPl, int tid) {
  for (int i = tid; i < 2 * NCB * 64; i += ST_THREADS) {
    const int rowpos = i % (NCB * 64), hh = i / (NCB * 64);
    const int n = mfma_row_channel(rowpos);
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if (n < CoutP) {
      v0 = *reinterpret_cast<const f32x4*>(w16 + n * 16 + hh * 8);
      v1 = *reinterpret_cast<const f32x4*>(w16 + n * 16 + hh * 8 + 4);
    }
    unsigned hi[4], lo[4];
    split8_bf16(v0, v1, hi, lo);
    const u32x4 h4 = {hi[0], hi[1], hi[2], hi[3]}, l4 = {lo[0], lo[1], lo[2], lo[3]};
    *reinterpret_cast<u32x4*>(sPh + (hh * (NCB * 64) + rowpos) * 16) = h4;
    *reinterpret_cast<u32x4*>(sPl + (hh * (NCB * 64) + rowpos) * 16) = l4;
  }
}

// the three pieces of the wave whose first pixel is p0 (inside image `img`, P pixels, rows of W) -> the slot at LDS address slot_lds
__device__ __forceinline__ void pc_issue(const float* img, int P, int W, int p0, int lane, unsigned slot_lds) {
  const i32x4 rs = lds_dma_rsrc_uniform(img, (unsigned)P * 4u);
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int idx = p0 + (dy - 1) * W - 1 + lane;
    const unsigned voff = (lane < 34 && idx >= 0 && idx < P) ? (unsigned)idx * 4u : PC_OUTSIDE;
    lds_dma0_dword(voff, rs, __builtin_amdgcn_readfirstlane(slot_lds + (unsigned)dy * 256u));
  }
}

// the pixel operand of lane (r, h): pixel p = p0 + r of the image, in column x = p % W; `slot` has landed.  TAPS_OUT: taps[0..8] also
// receive the nine taps as they enter the product (zero outside the image and beyond its last pixel), for a caller that sums them
template <bool TAPS_OUT = false>
__device__ __forceinline__ void pc_operand(const unsigned char* slot, int r, int h, int p, int P, int W, unsigned (&hi)[4],
                                           unsigned (&lo)[4], float* taps = nullptr) {
  const int x = p % W;
  const bool inside = p < P, lok = inside && x > 0, rok = inside && x + 1 < W;
  float t[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const float* row = reinterpret_cast<const float*>(slot + dy * 256) + r;
    t[3 * dy] = lok ? row[0] : 0.f;
    t[3 * dy + 1] = inside ? row[1] : 0.f;
    t[3 * dy + 2] = rok ? row[2] : 0.f;
  }
  f32x4 v0, v1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v0[j] = h ? (j == 0 ? t[8] : (j == 1 && inside ? 1.f : 0.f)) : t[j];
    v1[j] = h ? 0.f : t[4 + j];
  }
  split8_bf16(v0, v1, hi, lo);
  if constexpr (TAPS_OUT) {
#pragma unroll
    for (int j = 0; j < 9; ++j) taps[j] = t[j];
  }
}

// the chunk's k-step for NCB blocks of 64 output channels: acc[cb][ni] += W_chunk . operand (hi*lo + lo*hi + hi*hi)
template <int NCB>
__device__ __forceinline__ void pc_mfma(const unsigned char* sPh, const unsigned char* sPl, int r, int h, const unsigned (&hi)[4],
                                        const unsigned (&lo)[4], f32x16 (&acc)[NCB][2]) {
  union { unsigned u[4]; bf16x8_t v; } ph, pl;
#pragma unroll
  for (int i = 0; i < 4; ++i) { ph.u[i] = hi[i]; pl.u[i] = lo[i]; }
  const int wrow = h * (NCB * 64) + r;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const bf16x8_t wh = *reinterpret_cast<const bf16x8_t*>(sPh + (wrow + cb * 64 + ni * 32) * 16);
      const bf16x8_t wl = *reinterpret_cast<const bf16x8_t*>(sPl + (wrow + cb * 64 + ni * 32) * 16);
      acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, pl.v, acc[cb][ni], 0, 0, 0);
      acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ph.v, acc[cb][ni], 0, 0, 0);
      acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ph.v, acc[cb][ni], 0, 0, 0);
    }
}

}  // namespace
