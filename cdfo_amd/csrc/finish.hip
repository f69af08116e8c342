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
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
  __syncthreads();
  return t;   // valid in thread 0
}

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
