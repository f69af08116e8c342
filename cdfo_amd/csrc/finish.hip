// The output side of sequence evaluation (cdfo_amd/evaluate.py): what the reference does on the host after every forward
// (test_LD_37.py:179-180: clamp, * 255.0, astype(uint8), cv2.imwrite; then cal_psnr_ssim on the PNGs read back), here on the
// device and on 8-bit frames.
//
//   cdfo_finish_frames       K fp32 chunk outputs, read in place through a row pitch and a frame stride, -> K cropped 8-bit frames
//                            [K][Ho][Wo]; optionally the PSNR numerator sum (u8 - gt)^2 against 8-bit ground truth in the same pass,
//                            as exact integers.
//   cdfo_metric_partials_u8  cdfo_metric_partials on two stacks of 8-bit frames with their own pitches, over their common size.
//   cdfo_finish_frames_u16   cdfo_finish_frames to 16-bit samples of a peak of 1 .. 65535 (10-, 12-, 16-bit material).
//   cdfo_ssim_partials_u16   the SSIM form of cdfo_metric_partials_u8 on 16-bit samples of such a peak.
//   cdfo_msssim_partials_u8 / _u16   five-scale MS-SSIM of two such stacks: the sums of cs and of l * cs per level (at the end of this file).
//
// The kernels are templates on the sample type; the 16-bit forms take the peak as an argument where the 8-bit forms have 255 compiled in.
//
// The first is a streaming kernel (16-byte fp32 loads, 4-, 8- or 16-byte stores of 8-bit pixels, no LDS beyond the block sum).  The
// SSIM form of the second is separable: a tile of byte pairs and its 10-pixel halo is staged in LDS once, a horizontal 11-tap pass
// writes the five moments (a, b, a^2, b^2, ab) in fp64 to LDS, a vertical pass forms the SSIM term.  22 taps per output instead of
// the 121 of ssim_kernel (metrics.hip); fp64 throughout, as there.  No atomics: per-block partials, summed by the caller in order.
#include "common.h"
#include "numeric.h"

namespace {

// ------------------------------------------------------------------------------------------------------ cdfo_finish_frames
// x -> 8-bit: clamp to [0,1] (NaN -> 0), one correctly rounded fp32 multiply by 255, then truncation (the reference's
// astype(np.uint8)) or round-to-nearest-even.  The clamped product lies in [0,255]: the conversions cannot overflow.
// (16-bit samples: by the peak, 1 .. 65535, exact in fp32; the product lies in [0,peak].)
__device__ __forceinline__ unsigned quantise(float x, int mode, float peak) {
  float v = (x != x) ? 0.f : x;
  v = fminf(fmaxf(v, 0.f), 1.f);
  v = __fmul_rn(v, peak);
  if (mode == CDFO_QUANT_NEAREST) v = rintf(v);
  return (unsigned)(int)v;
}

template <int P> struct store_t;
template <> struct store_t<4> { typedef unsigned type; };
template <> struct store_t<8> { typedef unsigned long long type; };
template <> struct store_t<16> { typedef unsigned type __attribute__((ext_vector_type(4))); };

// One thread and trip: P consecutive pixels of one row, P * sizeof(T) = 4, 8 or 16 bytes: the widest store every row of Wo pixels is
// aligned for (8-bit: P = 4, 8, 16; 16-bit: P = 4, 8).
// grid (x: workgroups striding over the frame's Ho * Wo / P threads; y: frame).  Offsets inside a frame are 32-bit (host guard).
// gt_words: the ground truth can be read in aligned 32-bit words (1: pointer, pitch and frame stride multiples of 4 bytes) or, 16-bit
// samples, in aligned 64-bit words (2: multiples of 8 bytes); 0: per element.  peak: read by the 16-bit form only.
template <int P, typename T>
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ src, int src_pitch, long long src_fstride, int Ho, int Wo,
                                                     T* __restrict__ dst, int mode, const T* __restrict__ gt,
                                                     int gt_pitch, long long gt_fstride, int gt_words, int Hm, int Wm, int crop,
                                                     long long* __restrict__ partial, float peak) {
  constexpr int BITS = 8 * sizeof(T), PW = 4 / sizeof(T), NW = P / PW;   // bits of a pixel, pixels of a 32-bit word, words of a trip
  __shared__ long long sh[4];
  const int k = blockIdx.y;
  const float scale = sizeof(T) == 1 ? 255.f : peak;
  const float* s = src + (long long)k * src_fstride;
  T* d = dst + (long long)k * Ho * Wo;
  const T* g = gt ? gt + (long long)k * gt_fstride : nullptr;
  const int wp = Wo / P, total = Ho * wp;
  long long sse = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int y = i / wp, x = (i - y * wp) * P;
    unsigned q[P];
#pragma unroll
    for (int v = 0; v < P / 4; ++v) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(s + y * src_pitch + x + 4 * v);
#pragma unroll
      for (int e = 0; e < 4; ++e) q[4 * v + e] = quantise(f[e], mode, scale);
    }
    unsigned w[NW];
#pragma unroll
    for (int v = 0; v < NW; ++v) {
      w[v] = q[PW * v];
#pragma unroll
      for (int e = 1; e < PW; ++e) w[v] |= q[PW * v + e] << (BITS * e);
    }
    typename store_t<4 * NW>::type* o = reinterpret_cast<typename store_t<4 * NW>::type*>(d + y * Wo + x);
    if constexpr (NW == 1) *o = w[0];
    else if constexpr (NW == 2) *o = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    else *o = typename store_t<16>::type{w[0], w[1], w[2], w[3]};
    if (g && y >= crop && y < Hm - crop) {
      const T* row = g + y * gt_pitch;
#pragma unroll
      for (int v = 0; v < P / 4; ++v) {
        const int x0 = x + 4 * v;
        if (x0 + 3 < crop || x0 >= Wm - crop) continue;
        // a word starts inside the row (x0 < Wm <= Wgt <= pitch, both multiples of the word's pixels => its last pixel < pitch);
        // the second 32-bit word of 16-bit samples is read only where a wanted pixel lies in it (x0 + 2 < Wm - crop <= pitch)
        const typename gt_word<T>::type word = load_gt_word(row + x0, gt_words, x0 + 2 < Wm - crop);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int xe = x0 + e;
          if (xe >= crop && xe < Wm - crop) {
            const unsigned r = gt_words ? (unsigned)((word >> (BITS * e)) & ((1u << BITS) - 1u)) : (unsigned)row[xe];
            sse += sqdiff<T>(q[4 * v + e], r);
          }
        }
      }
    }
  }
  if (partial) {
    sse = block_sum_i64(sse, sh);
    if (threadIdx.x == 0) partial[(long long)k * gridDim.x + blockIdx.x] = sse;
  }
}

// ------------------------------------------------------------------------------------------------- cdfo_metric_partials_u8
__global__ __launch_bounds__(256) void sqdiff_u8_kernel(const unsigned char* __restrict__ a, int a_pitch, long long a_fstride,
                                                        const unsigned char* __restrict__ b, int b_pitch, long long b_fstride,
                                                        int Hm, int Wm, int crop, double* __restrict__ partial) {
  __shared__ long long sh[4];
  const int n = blockIdx.y, Hc = Hm - 2 * crop, Wc = Wm - 2 * crop, total = Hc * Wc;
  const unsigned char* pa = a + (long long)n * a_fstride;
  const unsigned char* pb = b + (long long)n * b_fstride;
  long long s = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int y = i / Wc + crop, x = i - (i / Wc) * Wc + crop;
    const int df = (int)pa[y * a_pitch + x] - (int)pb[y * b_pitch + x];
    s += df * df;
  }
  s = block_sum_i64(s, sh);
  if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = (double)s;   // < 2^53: exact
}

// A product rounded on its own.  The build's -ffp-contract=fast fuses a multiply into a later add across statements and ignores
// fp-contract pragmas, and the __dmul_rn family is a plain `*` here; an empty asm on the product's registers is what keeps it apart.
__device__ __forceinline__ double mul_rounded(double a, double b) {
  double p = a * b;
  asm("" : "+v"(p));
  return p;
}

// The SSIM term of the 16-bit form with its three products of means rounded on their own: with equal frames (m1 == m2,
// s11 == s22 == s12, bit for bit: the passes above treat both frames alike) 2 p12 + C1 and p11 + p22 + C1 are then the same number
// (2 p is exact), as are 2 cv + C2 and v1 + v2 + C2, and the term is exactly 1.  A fused fma(2 m1, m2, C1) beside a fused
// fma(m1, m1, m2 m2) + C1 differs from it by an ulp in about a sixth of the pixels.  (The 8-bit form keeps the expression, and the
// contraction, it was released with.)
__device__ __forceinline__ double ssim_term_strict(double m1, double m2, double s11, double s22, double s12, double C1, double C2) {
  const double p11 = mul_rounded(m1, m1), p22 = mul_rounded(m2, m2), p12 = mul_rounded(m1, m2);
  const double v1 = s11 - p11, v2 = s22 - p22, cv = s12 - p12;
  return ((2 * p12 + C1) * (2 * cv + C2)) / ((p11 + p22 + C1) * (v1 + v2 + C2));
}

constexpr int SS_TW = 32, SS_TH = 16;                    // outputs of one tile
constexpr int SS_IW = SS_TW + 10, SS_IH = SS_TH + 10;    // its input pixels

// grid (x: workgroups striding over the tiles of the SSIM map; y: frame pair).  peak: read by the 16-bit form only.
template <typename T>
__global__ __launch_bounds__(256) void ssim_kernel_t(const T* __restrict__ a, int a_pitch, long long a_fstride,
                                                     const T* __restrict__ b, int b_pitch, long long b_fstride,
                                                     int Hm, int Wm, int crop, double* __restrict__ partial, double peak) {
  __shared__ double sh[4];
  __shared__ double g[11];
  __shared__ T ta[SS_IH][SS_IW + 2], tb[SS_IH][SS_IW + 2];
  __shared__ double hm[5][SS_IH][SS_TW];                 // horizontal pass: 5 x 26 x 32 x 8 = 33280 bytes
  if (threadIdx.x < 11) {
    double s = 0.0;
    for (int i = 0; i < 11; ++i) s += exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    g[threadIdx.x] = exp(-((int)(threadIdx.x - 5) * (int)(threadIdx.x - 5)) / (2.0 * 1.5 * 1.5)) / s;   // cv2.getGaussianKernel(11, 1.5)
  }
  const int n = blockIdx.y;
  const T* pa = a + (long long)n * a_fstride;
  const T* pb = b + (long long)n * b_fstride;
  const int Ho = Hm - 2 * crop - 10, Wo = Wm - 2 * crop - 10;               // the SSIM map
  const int tx_n = (Wo + SS_TW - 1) / SS_TW, ty_n = (Ho + SS_TH - 1) / SS_TH;
  const double C1 = sizeof(T) == 1 ? (0.01 * 255) * (0.01 * 255) : (0.01 * peak) * (0.01 * peak);
  const double C2 = sizeof(T) == 1 ? (0.03 * 255) * (0.03 * 255) : (0.03 * peak) * (0.03 * peak);
  double acc = 0.0;
  for (int tile = blockIdx.x; tile < tx_n * ty_n; tile += gridDim.x) {
    const int oy0 = (tile / tx_n) * SS_TH, ox0 = (tile % tx_n) * SS_TW;     // map coordinates of the tile
    __syncthreads();                                                          // g ready / the previous tile's passes done
    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {
      const int r = i / SS_IW, c = i - r * SS_IW;
      const int y = oy0 + crop + r, x = ox0 + crop + c;
      const bool in = y < Hm && x < Wm;                                       // beyond the frames: zeros, feeding masked outputs only
      ta[r][c] = in ? pa[y * a_pitch + x] : (T)0;
      tb[r][c] = in ? pb[y * b_pitch + x] : (T)0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_IH * SS_TW; i += 256) {
      const int r = i / SS_TW, c = i - r * SS_TW;
      double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const double w = g[t], p = (double)ta[r][c + t], q = (double)tb[r][c + t];
        m1 += w * p; m2 += w * q; s11 += w * (p * p); s22 += w * (q * q); s12 += w * (p * q);
      }
      hm[0][r][c] = m1; hm[1][r][c] = m2; hm[2][r][c] = s11; hm[3][r][c] = s22; hm[4][r][c] = s12;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_TH * SS_TW; i += 256) {
      const int r = i / SS_TW, c = i - r * SS_TW;
      if (oy0 + r >= Ho || ox0 + c >= Wo) continue;
      double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const double w = g[t];
        m1 += w * hm[0][r + t][c]; m2 += w * hm[1][r + t][c]; s11 += w * hm[2][r + t][c]; s22 += w * hm[3][r + t][c];
        s12 += w * hm[4][r + t][c];
      }
      if constexpr (sizeof(T) == 1) {
        const double v1 = s11 - m1 * m1, v2 = s22 - m2 * m2, cv = s12 - m1 * m2;
        acc += ((2 * m1 * m2 + C1) * (2 * cv + C2)) / ((m1 * m1 + m2 * m2 + C1) * (v1 + v2 + C2));
      } else {
        acc += ssim_term_strict(m1, m2, s11, s22, s12, C1, C2);
      }
    }
  }
  acc = block_sum_f64(acc, sh);
  if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = acc;
}

inline bool fits32(long long rows, long long pitch) { return rows * pitch <= 0x7fffffffLL; }

// cdfo_finish_frames (T = unsigned char, peak 255) and cdfo_finish_frames_u16 (T = unsigned short)
template <typename T>
int finish_frames(const float* src, int src_pitch, long long src_fstride, int K, int Ho, int Wo, T* dst, int peak, int mode, const T* gt,
                  int gt_pitch, long long gt_fstride, int Hgt, int Wgt, int crop, long long* partial, int partial_cap, int* nblocks_out,
                  void* stream) {
  constexpr int S = sizeof(T);
  if (!src || !dst || K <= 0 || K > 65535 || Ho <= 0 || Wo <= 0 || Wo % 4 || src_pitch < Wo || src_fstride < 0 ||
      (mode != CDFO_QUANT_TRUNC && mode != CDFO_QUANT_NEAREST) || peak < 1 || peak > (1 << (8 * S)) - 1)
    return CDFO_EINVAL;
  if (!fits32(Ho, src_pitch) || !fits32(Ho, Wo) || (long long)Ho * (Wo / 4) + 1024LL * 256 > 0x7fffffffLL) return CDFO_EINVAL;   // 32-bit offsets inside a frame
  int Hm = 0, Wm = 0;
  if (gt) {
    if (!partial || !nblocks_out || Hgt <= 0 || Wgt <= 0 || gt_pitch < Wgt || gt_fstride < 0 || crop < 0 || !fits32(Hgt, gt_pitch))
      return CDFO_EINVAL;
    Hm = Ho < Hgt ? Ho : Hgt;                                  // psnr_ssim.py:462-468: min_height / min_width
    Wm = Wo < Wgt ? Wo : Wgt;
    if (Hm - 2 * crop <= 0 || Wm - 2 * crop <= 0) return CDFO_EINVAL;
  }
  if (!aligned16(src) || src_pitch % 4 || src_fstride % 4 || !aligned16(dst) || (gt && (reinterpret_cast<uintptr_t>(partial) & 7u)) ||
      (gt && (reinterpret_cast<uintptr_t>(gt) & (S - 1))))
    return CDFO_EALIGN;
  // the widest store every row start is aligned for: frames and rows are packed, so Wo decides (Ho * Wo keeps the next frame aligned)
  const int wb = Wo * S;                                       // bytes of a row: a multiple of 4 (8-bit) or 8 (16-bit)
  const int P = ((wb % 16 == 0) ? 16 : (wb % 8 == 0 && ((long long)Ho * wb) % 8 == 0) ? 8 : 4) / S;
  long long blocks = ((long long)Ho * (Wo / P) + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if (gt) {
    if ((long long)K * blocks > partial_cap) return CDFO_EINVAL;
    *nblocks_out = (int)blocks;
  }
  // in units of the word: pointer, pitch and frame stride (a multiple of 4 / S or 8 / S samples)
  auto words_of = [&](int bytes) {
    return gt && (reinterpret_cast<uintptr_t>(gt) & (bytes - 1)) == 0 && gt_pitch % (bytes / S) == 0 && gt_fstride % (bytes / S) == 0;
  };
  const int gt_words = (S == 2 && words_of(8)) ? 2 : words_of(4) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 0, (double)K * Ho * Wo * (4.0 + S + (gt ? S : 0)));
  const dim3 grid((unsigned)blocks, (unsigned)K);
  long long* part = gt ? partial : nullptr;
#define CDFO_FINISH(PX)                                                                                                              \
  hipLaunchKernelGGL((finish_kernel<PX, T>), grid, dim3(256), 0, st, src, src_pitch, src_fstride, Ho, Wo, dst, mode, gt, gt_pitch,    \
                     gt_fstride, gt_words, Hm, Wm, crop, part, (float)peak)
  if constexpr (S == 1) {
    if (P == 16) CDFO_FINISH(16);
    else if (P == 8) CDFO_FINISH(8);
    else CDFO_FINISH(4);
  } else {
    if (P == 8) CDFO_FINISH(8);
    else CDFO_FINISH(4);
  }
#undef CDFO_FINISH
  CDFO_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------ cdfo_msssim_partials_*
// Five-scale MS-SSIM of the luma (DESIGN.md has the definition): level 0 is the cropped common region of the two stacks, level j + 1
// the 2x2 mean of level j from its top-left sample, a trailing odd row or column dropped.  Three launches per call, whatever the
// number of frames (the frame is on grid.y everywhere):
//   1. msssim_pyramid_kernel writes levels 1..4 of both stacks in ONE pass over level 0: a workgroup owns a 64 x 64 tile, a thread
//      its 4 x 4 block (levels 1 and 2 in registers), levels 3 and 4 go through two small LDS stages.  The sums are integers
//      (at most 65535 * 256 < 2^24) and leave as sum / 4^j in fp32: every level is exact.
//   2. msssim_level_kernel<T> on level 0, read in place through pitch, frame stride and crop like ssim_kernel_t;
//   3. msssim_level_kernel<float> on levels 1..4 in one grid: a level owns a range of blockIdx.x, its blocks stride over its tiles.
// The level pass is ssim_kernel_t's (tiles, the two separable 11-tap passes through LDS in fp64) with two sums per block, cs and
// l * cs, and with the products of means rounded on their own at every depth, so that equal frames give exactly 1 in both.  The
// pyramid is a pass of its own, not fused into the level pass: a level-j tile with its halo would need (32 + 10) * 2^j columns of
// level 0 again for every tile, the 10-sample halo re-reducing what the neighbour tile reduces.
struct MsLevels {
  int n;                     // levels of this launch: 1 (level 0) or 4 (the pyramid)
  int H[4], W[4];            // the planes
  int a_pitch[4], b_pitch[4];
  long long off[4];          // a plane's first sample inside its frame
  int blk[5];                // level i owns the workgroups blk[i] <= blockIdx.x < blk[i + 1], that many stride over its tiles
};

template <typename T>
__global__ __launch_bounds__(256) void msssim_pyramid_kernel(const T* __restrict__ a, int a_pitch, long long a_fstride,
                                                             const T* __restrict__ b, int b_pitch, long long b_fstride, int Hc, int Wc,
                                                             float* __restrict__ pyr, long long plane, MsLevels L) {
  __shared__ unsigned s2[16][16], s3[8][8];
  const int n = blockIdx.y, which = blockIdx.z;                                // which: 0 the stack a, 1 the stack b
  const T* src = which ? b + (long long)n * b_fstride : a + (long long)n * a_fstride;
  const int pitch = which ? b_pitch : a_pitch;
  float* dst = pyr + ((long long)n * 2 + which) * plane;
  const int tx_n = (Wc + 63) / 64;
  const int y0 = (blockIdx.x / tx_n) * 64, x0 = (blockIdx.x % tx_n) * 64;      // level-0 origin of the tile
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  unsigned q[2][2];                                                            // the thread's 2 x 2 of level 1, as sums of four
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned s = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int y = y0 + 4 * ty + 2 * i + (e >> 1), x = x0 + 4 * tx + 2 * j + (e & 1);
        s += (y < Hc && x < Wc) ? (unsigned)src[y * pitch + x] : 0u;           // beyond the region: feeds samples that are not written
      }
      q[i][j] = s;
      const int y1 = (y0 >> 1) + 2 * ty + i, x1 = (x0 >> 1) + 2 * tx + j;
      if (y1 < L.H[0] && x1 < L.W[0]) dst[L.off[0] + y1 * L.W[0] + x1] = (float)s * 0.25f;
    }
  const unsigned t2 = q[0][0] + q[0][1] + q[1][0] + q[1][1];
  {
    const int y2 = (y0 >> 2) + ty, x2 = (x0 >> 2) + tx;
    if (y2 < L.H[1] && x2 < L.W[1]) dst[L.off[1] + y2 * L.W[1] + x2] = (float)t2 * (1.f / 16.f);
  }
  s2[ty][tx] = t2;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
    const unsigned t3 = s2[2 * r][2 * c] + s2[2 * r][2 * c + 1] + s2[2 * r + 1][2 * c] + s2[2 * r + 1][2 * c + 1];
    const int y3 = (y0 >> 3) + r, x3 = (x0 >> 3) + c;
    if (y3 < L.H[2] && x3 < L.W[2]) dst[L.off[2] + y3 * L.W[2] + x3] = (float)t3 * (1.f / 64.f);
    s3[r][c] = t3;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
    const unsigned t4 = s3[2 * r][2 * c] + s3[2 * r][2 * c + 1] + s3[2 * r + 1][2 * c] + s3[2 * r + 1][2 * c + 1];
    const int y4 = (y0 >> 4) + r, x4 = (x0 >> 4) + c;
    if (y4 < L.H[3] && x4 < L.W[3]) dst[L.off[3] + y4 * L.W[3] + x4] = (float)t4 * (1.f / 256.f);   // t4 < 2^24: exact
  }
}

// grid (x: the levels' workgroups, see MsLevels; y: frame pair).  A workgroup writes its two sums, cs then l * cs, at
// partial[n * row + 2 * (base + blockIdx.x)].
template <typename T>
__global__ __launch_bounds__(256) void msssim_level_kernel(const T* __restrict__ a, long long a_fstride, const T* __restrict__ b,
                                                           long long b_fstride, MsLevels L, double* __restrict__ partial, int row,
                                                           int base, double peak) {
  __shared__ double sh[4];
  __shared__ double g[11];
  __shared__ T ta[SS_IH][SS_IW + 2], tb[SS_IH][SS_IW + 2];
  __shared__ double hm[5][SS_IH][SS_TW];
  if (threadIdx.x < 11) {
    double s = 0.0;
    for (int i = 0; i < 11; ++i) s += exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    g[threadIdx.x] = exp(-((int)(threadIdx.x - 5) * (int)(threadIdx.x - 5)) / (2.0 * 1.5 * 1.5)) / s;   // as ssim_kernel_t
  }
  int H = L.H[0], W = L.W[0], a_pitch = L.a_pitch[0], b_pitch = L.b_pitch[0], first = L.blk[0], end = L.blk[1];
  long long off = L.off[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (i < L.n && (int)blockIdx.x >= L.blk[i]) {
      H = L.H[i]; W = L.W[i]; a_pitch = L.a_pitch[i]; b_pitch = L.b_pitch[i]; off = L.off[i]; first = L.blk[i]; end = L.blk[i + 1];
    }
  const int n = blockIdx.y;
  const T* pa = a + (long long)n * a_fstride + off;
  const T* pb = b + (long long)n * b_fstride + off;
  const int Ho = H - 10, Wo = W - 10;                                         // the level's map
  const int tx_n = (Wo + SS_TW - 1) / SS_TW, ty_n = (Ho + SS_TH - 1) / SS_TH;
  const double C1 = (0.01 * peak) * (0.01 * peak), C2 = (0.03 * peak) * (0.03 * peak);
  double acc_cs = 0.0, acc_s = 0.0;
  for (int tile = blockIdx.x - first; tile < tx_n * ty_n; tile += end - first) {
    const int oy0 = (tile / tx_n) * SS_TH, ox0 = (tile % tx_n) * SS_TW;
    __syncthreads();                                                          // g ready / the previous tile's passes done
    for (int i = threadIdx.x; i < SS_IH * SS_IW; i += 256) {
      const int r = i / SS_IW, c = i - r * SS_IW;
      const int y = oy0 + r, x = ox0 + c;
      const bool in = y < H && x < W;                                         // beyond the plane: zeros, feeding masked outputs only
      ta[r][c] = in ? pa[y * a_pitch + x] : (T)0;
      tb[r][c] = in ? pb[y * b_pitch + x] : (T)0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_IH * SS_TW; i += 256) {
      const int r = i / SS_TW, c = i - r * SS_TW;
      double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const double w = g[t], p = (double)ta[r][c + t], q = (double)tb[r][c + t];
        m1 += w * p; m2 += w * q; s11 += w * (p * p); s22 += w * (q * q); s12 += w * (p * q);
      }
      hm[0][r][c] = m1; hm[1][r][c] = m2; hm[2][r][c] = s11; hm[3][r][c] = s22; hm[4][r][c] = s12;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SS_TH * SS_TW; i += 256) {
      const int r = i / SS_TW, c = i - r * SS_TW;
      if (oy0 + r >= Ho || ox0 + c >= Wo) continue;
      double m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const double w = g[t];
        m1 += w * hm[0][r + t][c]; m2 += w * hm[1][r + t][c]; s11 += w * hm[2][r + t][c]; s22 += w * hm[3][r + t][c];
        s12 += w * hm[4][r + t][c];
      }
      // ssim_term_strict's products; with equal frames numerator and denominator of each factor are the same number, cs == l == 1
      const double p11 = mul_rounded(m1, m1), p22 = mul_rounded(m2, m2), p12 = mul_rounded(m1, m2);
      const double v1 = s11 - p11, v2 = s22 - p22, cv = s12 - p12;
      const double cs = (2 * cv + C2) / (v1 + v2 + C2), l = (2 * p12 + C1) / (p11 + p22 + C1);
      acc_cs += cs;
      acc_s += l * cs;
    }
  }
  acc_cs = block_sum_f64(acc_cs, sh);
  acc_s = block_sum_f64(acc_s, sh);
  if (threadIdx.x == 0) {
    double* out = partial + (long long)n * row + 2 * (long long)(base + blockIdx.x);
    out[0] = acc_cs;
    out[1] = acc_s;
  }
}

// the pyramid of an Hc x Wc region: levels 1..4 packed one after the other; -> the samples of one plane's pyramid
long long msssim_layout(int Hc, int Wc, MsLevels& L) {
  long long at = 0;
  for (int j = 0; j < 4; ++j) {
    L.H[j] = Hc >> (j + 1);
    L.W[j] = Wc >> (j + 1);
    L.a_pitch[j] = L.b_pitch[j] = L.W[j];
    L.off[j] = at;
    at += (long long)L.H[j] * L.W[j];
  }
  return at;
}

int msssim_blocks(int H, int W) {
  const long long tiles = (long long)cdiv(W - 10, SS_TW) * cdiv(H - 10, SS_TH);
  return tiles > 1024 ? 1024 : (int)tiles;
}

// cdfo_msssim_partials_u8 (T = unsigned char, peak 255) and cdfo_msssim_partials_u16 (T = unsigned short)
template <typename T>
int msssim_partials(const T* a, int a_pitch, long long a_fstride, int Ha, int Wa, const T* b, int b_pitch, long long b_fstride, int Hb,
                    int Wb, int N, int crop, int peak, float* pyramid, long long pyramid_bytes, double* partial, int partial_cap,
                    int* nblocks_out, void* stream) {
  if (!a || !b || !pyramid || !partial || !nblocks_out || N <= 0 || N > 65535 || Ha <= 0 || Wa <= 0 || Hb <= 0 || Wb <= 0 || crop < 0 ||
      a_pitch < Wa || b_pitch < Wb || a_fstride < 0 || b_fstride < 0 || peak < 1 || peak > (1 << (8 * sizeof(T))) - 1)
    return CDFO_EINVAL;
  if (!fits32(Ha, a_pitch) || !fits32(Hb, b_pitch)) return CDFO_EINVAL;                       // 32-bit offsets inside a frame
  const int Hm = Ha < Hb ? Ha : Hb, Wm = Wa < Wb ? Wa : Wb;
  if (crop > (Hm < Wm ? Hm : Wm) / 2) return CDFO_EINVAL;
  const int Hc = Hm - 2 * crop, Wc = Wm - 2 * crop;
  if (Hc < CDFO_MSSSIM_MIN_SIZE || Wc < CDFO_MSSSIM_MIN_SIZE) return CDFO_EINVAL;             // level 4 holds one 11 x 11 window
  MsLevels P;
  const long long plane = msssim_layout(Hc, Wc, P);
  if (pyramid_bytes < 2LL * N * plane * (long long)sizeof(float)) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partial) & 7u) || (reinterpret_cast<uintptr_t>(pyramid) & 3u) ||
      ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & (sizeof(T) - 1)))
    return CDFO_EALIGN;
  MsLevels Z = {};
  Z.n = 1;
  Z.H[0] = Hc; Z.W[0] = Wc; Z.a_pitch[0] = a_pitch; Z.b_pitch[0] = b_pitch;
  Z.blk[1] = msssim_blocks(Hc, Wc);
  P.n = 4;
  P.blk[0] = 0;
  for (int j = 0; j < 4; ++j) P.blk[j + 1] = P.blk[j] + msssim_blocks(P.H[j], P.W[j]);
  const int row = 2 * (Z.blk[1] + P.blk[4]);
  if ((long long)N * row > partial_cap) return CDFO_EINVAL;
  nblocks_out[0] = Z.blk[1];
  for (int j = 0; j < 4; ++j) nblocks_out[j + 1] = P.blk[j + 1] - P.blk[j];
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the level passes: ssim's 2 x 11 taps of five moments per output, over 1 + 1/4 + ... of the pixels
  CdfoProfScope prof(st, KID_LAYOUT, 220.0 * N * ((double)(Hc - 10) * (Wc - 10) + (double)plane), 2.0 * N * (sizeof(T) * 2.0 * Hc * Wc + 8.0 * plane));
  const T* a0 = a + (long long)crop * a_pitch + crop;
  const T* b0 = b + (long long)crop * b_pitch + crop;
  hipLaunchKernelGGL(msssim_pyramid_kernel<T>, dim3((unsigned)(cdiv(Wc, 64) * cdiv(Hc, 64)), (unsigned)N, 2u), dim3(256), 0, st, a0, a_pitch,
                     a_fstride, b0, b_pitch, b_fstride, Hc, Wc, pyramid, plane, P);
  hipLaunchKernelGGL(msssim_level_kernel<T>, dim3((unsigned)Z.blk[1], (unsigned)N), dim3(256), 0, st, a0, a_fstride, b0, b_fstride, Z,
                     partial, row, 0, (double)peak);
  hipLaunchKernelGGL(msssim_level_kernel<float>, dim3((unsigned)P.blk[4], (unsigned)N), dim3(256), 0, st,
                     static_cast<const float*>(pyramid), 2 * plane, static_cast<const float*>(pyramid) + plane, 2 * plane, P, partial, row,
                     Z.blk[1], (double)peak);
  CDFO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cdfo_finish_frames(const float* src, int src_pitch, long long src_fstride, int K, int Ho, int Wo, unsigned char* dst,
                                  int mode, const unsigned char* gt, int gt_pitch, long long gt_fstride, int Hgt, int Wgt, int crop,
                                  long long* partial, int partial_cap, int* nblocks_out, void* stream) {
  return finish_frames<unsigned char>(src, src_pitch, src_fstride, K, Ho, Wo, dst, 255, mode, gt, gt_pitch, gt_fstride, Hgt, Wgt, crop,
                                      partial, partial_cap, nblocks_out, stream);
}

extern "C" int cdfo_finish_frames_u16(const float* src, int src_pitch, long long src_fstride, int K, int Ho, int Wo, unsigned short* dst,
                                      int peak, int mode, const unsigned short* gt, int gt_pitch, long long gt_fstride, int Hgt, int Wgt,
                                      int crop, long long* partial, int partial_cap, int* nblocks_out, void* stream) {
  return finish_frames<unsigned short>(src, src_pitch, src_fstride, K, Ho, Wo, dst, peak, mode, gt, gt_pitch, gt_fstride, Hgt, Wgt, crop,
                                       partial, partial_cap, nblocks_out, stream);
}

extern "C" int cdfo_metric_partials_u8(const unsigned char* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned char* b,
                                       int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, int metric, double* partial,
                                       int partial_cap, int* nblocks_out, void* stream) {
  if (!a || !b || !partial || !nblocks_out || N <= 0 || N > 65535 || Ha <= 0 || Wa <= 0 || Hb <= 0 || Wb <= 0 || crop < 0 ||
      a_pitch < Wa || b_pitch < Wb || a_fstride < 0 || b_fstride < 0 || (metric != 0 && metric != 1))
    return CDFO_EINVAL;
  if (!fits32(Ha, a_pitch) || !fits32(Hb, b_pitch)) return CDFO_EINVAL;                       // 32-bit offsets inside a frame
  const int Hm = Ha < Hb ? Ha : Hb, Wm = Wa < Wb ? Wa : Wb;
  const int Ho = Hm - 2 * crop - (metric == 1 ? 10 : 0), Wo = Wm - 2 * crop - (metric == 1 ? 10 : 0);
  if (Ho <= 0 || Wo <= 0) return CDFO_EINVAL;
  if ((long long)Ho * Wo + 1024LL * 256 > 0x7fffffffLL) return CDFO_EINVAL;                   // the grid-stride index stays 32-bit
  if (reinterpret_cast<uintptr_t>(partial) & 7u) return CDFO_EALIGN;
  long long blocks = metric == 1 ? (long long)cdiv(Wo, SS_TW) * cdiv(Ho, SS_TH) : ((long long)Ho * Wo + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  if ((long long)N * blocks > partial_cap) return CDFO_EINVAL;
  *nblocks_out = (int)blocks;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks, (unsigned)N);
  // SSIM: 2 x 11 taps of five moments per output, one multiply-add each (the halo's share of the horizontal pass not counted)
  CdfoProfScope prof(st, KID_LAYOUT, metric == 1 ? 220.0 * N * Ho * Wo : 0.0, 2.0 * N * Hm * Wm);
  if (metric == 0)
    hipLaunchKernelGGL(sqdiff_u8_kernel, grid, dim3(256), 0, st, a, a_pitch, a_fstride, b, b_pitch, b_fstride, Hm, Wm, crop, partial);
  else
    hipLaunchKernelGGL(ssim_kernel_t<unsigned char>, grid, dim3(256), 0, st, a, a_pitch, a_fstride, b, b_pitch, b_fstride, Hm, Wm, crop,
                       partial, 255.0);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ssim_partials_u16(const unsigned short* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned short* b,
                                      int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, int peak, double* partial,
                                      int partial_cap, int* nblocks_out, void* stream) {
  if (!a || !b || !partial || !nblocks_out || N <= 0 || N > 65535 || Ha <= 0 || Wa <= 0 || Hb <= 0 || Wb <= 0 || crop < 0 ||
      a_pitch < Wa || b_pitch < Wb || a_fstride < 0 || b_fstride < 0 || peak < 1 || peak > 65535)
    return CDFO_EINVAL;
  if (!fits32(Ha, a_pitch) || !fits32(Hb, b_pitch)) return CDFO_EINVAL;                       // 32-bit offsets inside a frame
  const int Hm = Ha < Hb ? Ha : Hb, Wm = Wa < Wb ? Wa : Wb;
  const int Ho = Hm - 2 * crop - 10, Wo = Wm - 2 * crop - 10;
  if (Ho <= 0 || Wo <= 0) return CDFO_EINVAL;
  if ((long long)Ho * Wo + 1024LL * 256 > 0x7fffffffLL) return CDFO_EINVAL;                   // as cdfo_metric_partials_u8
  if ((reinterpret_cast<uintptr_t>(partial) & 7u) || ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 1u)) return CDFO_EALIGN;
  long long blocks = (long long)cdiv(Wo, SS_TW) * cdiv(Ho, SS_TH);
  if (blocks > 1024) blocks = 1024;
  if ((long long)N * blocks > partial_cap) return CDFO_EINVAL;
  *nblocks_out = (int)blocks;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 220.0 * N * Ho * Wo, 4.0 * N * Hm * Wm);
  hipLaunchKernelGGL(ssim_kernel_t<unsigned short>, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, st, a, a_pitch, a_fstride, b,
                     b_pitch, b_fstride, Hm, Wm, crop, partial, (double)peak);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" long long cdfo_msssim_pyramid_bytes(int Hc, int Wc, int N) {
  if (Hc < CDFO_MSSSIM_MIN_SIZE || Wc < CDFO_MSSSIM_MIN_SIZE || N <= 0) return 0;
  MsLevels L;
  return 2LL * N * msssim_layout(Hc, Wc, L) * (long long)sizeof(float);
}

extern "C" int cdfo_msssim_partials_u8(const unsigned char* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned char* b,
                                       int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, float* pyramid,
                                       long long pyramid_bytes, double* partial, int partial_cap, int* nblocks_out, void* stream) {
  return msssim_partials<unsigned char>(a, a_pitch, a_fstride, Ha, Wa, b, b_pitch, b_fstride, Hb, Wb, N, crop, 255, pyramid, pyramid_bytes,
                                        partial, partial_cap, nblocks_out, stream);
}

extern "C" int cdfo_msssim_partials_u16(const unsigned short* a, int a_pitch, long long a_fstride, int Ha, int Wa, const unsigned short* b,
                                        int b_pitch, long long b_fstride, int Hb, int Wb, int N, int crop, int peak, float* pyramid,
                                        long long pyramid_bytes, double* partial, int partial_cap, int* nblocks_out, void* stream) {
  return msssim_partials<unsigned short>(a, a_pitch, a_fstride, Ha, Wa, b, b_pitch, b_fstride, Hb, Wb, N, crop, peak, pyramid,
                                         pyramid_bytes, partial, partial_cap, nblocks_out, stream);
}
