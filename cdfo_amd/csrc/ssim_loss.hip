// SSIM and MS-SSIM as training losses on the device (cdfo_amd/loss.py: ssim_loss, msssim_loss; DESIGN.md "SSIM and MS-SSIM as
// losses"): the forward sums of a level, the 2 x 2 pool, the per-frame combine, and the exact gradient by sr.
// A frame is dense fp32 [H][W]; level j of the pyramid is (H >> j) x (W >> j), held in fp32.  Per valid position of a level, with the
// 11-tap Gaussian G of csrc/metrics.hip (cv2.getGaussianKernel(11, 1.5)), everything behind the fp32 loads in fp64:
//     m1 = G*x   m2 = G*y   e11 = G*x^2   e22 = G*y^2   e12 = G*xy
//     cs = (2 (e12 - m1 m2) + C2) / B2,  B2 = (e11 - m1^2) + (e22 - m2^2) + C2        l = (2 m1 m2 + C1) / B1,  B1 = m1^2 + m2^2 + C1
//     M_cs = mean(cs)   M_ssim = mean(l cs)
//
//   cdfo_ssim_loss_level    one launch.  A workgroup of 256 threads takes a tile of 16 x 32 valid positions: it stages the 26 x 42
//                           samples of both frames in LDS (zeros beyond the frame), runs the window along x over the 26 rows (five
//                           fp64 planes in LDS), then along y, and adds cs and l cs of its positions: per thread in index order, the
//                           wave's xor tree, the four waves in order.  The two sums go to partial[n][tile].
//   cdfo_ssim_loss_pool     one launch, both frames: a sample of the next level is fp32(((a + b) + c) + d in fp64, times 0.25).
//   cdfo_ssim_loss_combine  one thread per frame: the tiles of every level in index order, the means, the loss rounded once, and per
//                           level the coefficients a_cs = d loss / d M_cs, a_s = d loss / d M_ssim in fp64.
//   cdfo_ssim_loss_pqr      the level kernel's staging and passes again; per valid position P = d/d m1, Q = d/d e11, R = d/d e12 of
//                           (a_cs sum cs + a_s sum l cs) / n, fp64, to three valid-size maps.
//   cdfo_ssim_loss_adjoint  a workgroup takes 16 x 32 SAMPLES of the level: it stages the 26 x 42 map values that reach them (zeros
//                           beyond the maps), runs the window as the full correlation along x, then y, and forms
//                           (Gt*P + 2x Gt*Q) + y Gt*R, plus a quarter of the coarser level's gradient at (y / 2, x / 2) where the pool
//                           read this sample.  Levels above 0 keep their gradient in fp64; level 0's is rounded to fp32, once.
//
// Every window sum runs k = 0 .. 10 in order; no atomics; every grid is a function of (N, H, W) alone: equal inputs give equal bits.
#include "common.h"
#include <math.h>

namespace {

constexpr int SL_THREADS = 256;
constexpr int SL_TH = 16, SL_TW = 32;                      // the tile: rows x columns
constexpr int SL_TAPS = 11, SL_HALO = SL_TAPS - 1;
constexpr int SL_SH = SL_TH + SL_HALO, SL_SW = SL_TW + SL_HALO;
constexpr int SL_MAX_SIZE = 16384;
constexpr int SL_MS_MIN = CDFO_MSSSIM_MIN;                 // metrics.msssim_min_size: level 4 still holds one window

__device__ const double SL_WEIGHTS[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};      // metrics.MSSSIM_WEIGHTS

inline bool sl_frame_ok(int H, int W, int levels) {
  if (levels != 1 && levels != 5) return false;
  const int lo = levels == 5 ? SL_MS_MIN : SL_TAPS;
  return H >= lo && W >= lo && H <= SL_MAX_SIZE && W <= SL_MAX_SIZE;
}
__host__ __device__ inline int sl_tiles(int h, int w) {
  return ((h - SL_HALO + SL_TH - 1) / SL_TH) * ((w - SL_HALO + SL_TW - 1) / SL_TW);
}
__host__ __device__ inline int sl_tile_offset(int H, int W, int level) {
  int off = 0;
  for (int j = 0; j < level; ++j) off += sl_tiles(H >> j, W >> j);
  return off;
}
inline bool sl_peak_ok(double peak) { return peak > 0.0 && peak <= 1.7976931348623157e308; }      // a NaN fails the first
inline bool sl_misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

__device__ __forceinline__ void sl_window(double* g) {
  if (threadIdx.x < SL_TAPS) {
    double s = 0.0;
    for (int i = 0; i < SL_TAPS; ++i) s += exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    g[threadIdx.x] = exp(-((int)(threadIdx.x - 5) * (int)(threadIdx.x - 5)) / (2.0 * 1.5 * 1.5)) / s;   // cv2.getGaussianKernel(11, 1.5)
  }
}

// The five window sums at the tile's valid positions: f(oy, ox, m1, m2, e11, e22, e12) for each of this thread's positions that
// lies inside ho x wo, in index order.  sx, sy, hp, g: the workgroup's LDS.
template <class F>
__device__ __forceinline__ void sl_stats(const float* __restrict__ x, const float* __restrict__ y, int h, int w, int ho, int wo,
                                         float (*sx)[SL_SW], float (*sy)[SL_SW], double (*hp)[SL_SH][SL_TW], double* g, F&& f) {
  const int oy0 = blockIdx.y * SL_TH, ox0 = blockIdx.x * SL_TW;
  sl_window(g);
  for (int e = threadIdx.x; e < SL_SH * SL_SW; e += SL_THREADS) {
    const int r = e / SL_SW, c = e - r * SL_SW, gy = oy0 + r, gx = ox0 + c;
    const bool in = gy < h && gx < w;
    const size_t o = (size_t)gy * w + gx;
    sx[r][c] = in ? x[o] : 0.f;
    sy[r][c] = in ? y[o] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SL_SH * SL_TW; e += SL_THREADS) {
    const int r = e / SL_TW, c = e - r * SL_TW;
    double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
    for (int k = 0; k < SL_TAPS; ++k) {
      const double a = sx[r][c + k], b = sy[r][c + k], wk = g[k];
      m1 += wk * a; m2 += wk * b; e11 += wk * (a * a); e22 += wk * (b * b); e12 += wk * (a * b);
    }
    hp[0][r][c] = m1; hp[1][r][c] = m2; hp[2][r][c] = e11; hp[3][r][c] = e22; hp[4][r][c] = e12;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SL_TH * SL_TW; e += SL_THREADS) {
    const int r = e / SL_TW, c = e - r * SL_TW, oy = oy0 + r, ox = ox0 + c;
    if (oy >= ho || ox >= wo) continue;
    double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
    for (int k = 0; k < SL_TAPS; ++k) {
      const double wk = g[k];
      m1 += wk * hp[0][r + k][c]; m2 += wk * hp[1][r + k][c]; e11 += wk * hp[2][r + k][c]; e22 += wk * hp[3][r + k][c];
      e12 += wk * hp[4][r + k][c];
    }
    f(oy, ox, m1, m2, e11, e22, e12);
  }
}

// grid (tiles along x, tiles along y, N)
__global__ __launch_bounds__(SL_THREADS) void sl_level_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w,
                                                              double C1, double C2, double* __restrict__ partial, int tile_off,
                                                              int tile_stride) {
  __shared__ float sx[SL_SH][SL_SW], sy[SL_SH][SL_SW];
  __shared__ double hp[5][SL_SH][SL_TW];
  __shared__ double g[SL_TAPS];
  __shared__ double sh[2][SL_THREADS / 64];
  const size_t frame = (size_t)blockIdx.z * h * w;
  double acc_cs = 0.0, acc_s = 0.0;
  sl_stats(x + frame, y + frame, h, w, h - SL_HALO, w - SL_HALO, sx, sy, hp, g,
           [&](int, int, double m1, double m2, double e11, double e22, double e12) {
             const double cs = (2.0 * (e12 - m1 * m2) + C2) / ((e11 - m1 * m1) + (e22 - m2 * m2) + C2);
             const double l = (2.0 * m1 * m2 + C1) / (m1 * m1 + m2 * m2 + C1);
             acc_cs += cs;
             acc_s += l * cs;
           });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc_cs += __shfl_xor(acc_cs, off, 64);
    acc_s += __shfl_xor(acc_s, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = acc_cs;
    sh[1][threadIdx.x >> 6] = acc_s;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const size_t t = (size_t)blockIdx.z * tile_stride + tile_off + blockIdx.y * gridDim.x + blockIdx.x;
    partial[2 * t + threadIdx.x] = ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
  }
}

// grid (blocks over hn wn, 2 frames, N)
__global__ __launch_bounds__(SL_THREADS) void sl_pool_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w,
                                                             float* __restrict__ xn, float* __restrict__ yn) {
  const int hn = h >> 1, wn = w >> 1;
  const int i = blockIdx.x * SL_THREADS + threadIdx.x;
  if (i >= hn * wn) return;
  const int r = i / wn, c = i - r * wn;
  const float* src = (blockIdx.y ? y : x) + (size_t)blockIdx.z * h * w + (size_t)(2 * r) * w + 2 * c;
  float* dst = (blockIdx.y ? yn : xn) + (size_t)blockIdx.z * hn * wn;
  const double s = (((double)src[0] + (double)src[1]) + (double)src[w]) + (double)src[w + 1];
  dst[i] = (float)(s * 0.25);
}

// one thread per frame.  means, coef: [N][levels][2] = (M_cs, M_ssim), (a_cs, a_s)
__global__ __launch_bounds__(64) void sl_combine_kernel(const double* __restrict__ partial, int N, int H, int W, int levels,
                                                        int tile_stride, double* __restrict__ means, double* __restrict__ coef,
                                                        float* __restrict__ loss) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  const double* p = partial + (size_t)n * tile_stride * 2;
  double* mn = means + (size_t)n * levels * 2;
  double* cf = coef + (size_t)n * levels * 2;
  double used[5];
  for (int j = 0; j < levels; ++j) {
    const int h = H >> j, w = W >> j, t = sl_tiles(h, w);
    double s0 = 0.0, s1 = 0.0;
    for (int i = 0; i < t; ++i) {
      s0 += p[2 * i];
      s1 += p[2 * i + 1];
    }
    p += 2 * t;
    const double cnt = (double)(h - SL_HALO) * (double)(w - SL_HALO);
    mn[2 * j] = s0 / cnt;
    mn[2 * j + 1] = s1 / cnt;
    used[j] = j == levels - 1 ? mn[2 * j + 1] : mn[2 * j];
  }
  if (levels == 1) {
    loss[n] = (float)(1.0 - used[0]);
    cf[0] = 0.0;
    cf[1] = -1.0;
    return;
  }
  bool clamped = false;
  for (int j = 0; j < 5; ++j) clamped = clamped || used[j] <= 0.0;
  double prod = 1.0;
  if (!clamped)
    for (int j = 0; j < 5; ++j) prod *= pow(used[j], SL_WEIGHTS[j]);
  loss[n] = clamped ? 1.f : (float)(1.0 - prod);
  for (int j = 0; j < 5; ++j) {
    const double d = clamped ? 0.0 : -SL_WEIGHTS[j] * prod / used[j];
    cf[2 * j] = j < 4 ? d : 0.0;
    cf[2 * j + 1] = j < 4 ? 0.0 : d;
  }
}

// grid as sl_level_kernel.  pqr: [N][3][ho][wo]
__global__ __launch_bounds__(SL_THREADS) void sl_pqr_kernel(const float* __restrict__ x, const float* __restrict__ y, int h, int w,
                                                            double C1, double C2, const double* __restrict__ coef, int levels, int level,
                                                            double* __restrict__ pqr) {
  __shared__ float sx[SL_SH][SL_SW], sy[SL_SH][SL_SW];
  __shared__ double hp[5][SL_SH][SL_TW];
  __shared__ double g[SL_TAPS];
  const int ho = h - SL_HALO, wo = w - SL_HALO;
  const size_t frame = (size_t)blockIdx.z * h * w, plane = (size_t)ho * wo;
  const double* cf = coef + ((size_t)blockIdx.z * levels + level) * 2;
  const double cnt = (double)ho * (double)wo, a_cs = cf[0], a_s = cf[1];
  double* out = pqr + (size_t)blockIdx.z * 3 * plane;
  sl_stats(x + frame, y + frame, h, w, ho, wo, sx, sy, hp, g,
           [&](int oy, int ox, double m1, double m2, double e11, double e22, double e12) {
             const double B2 = (e11 - m1 * m1) + (e22 - m2 * m2) + C2, B1 = m1 * m1 + m2 * m2 + C1;
             const double cs = (2.0 * (e12 - m1 * m2) + C2) / B2, l = (2.0 * m1 * m2 + C1) / B1;
             const double alpha = (a_cs + a_s * l) / cnt, beta = a_s * cs / cnt;      // d / d cs, d / d l
             const double q = -(alpha * cs / B2);
             const size_t o = (size_t)oy * wo + ox;
             out[o] = alpha * ((2.0 * m1 * cs - 2.0 * m2) / B2) + beta * ((2.0 * m2 - 2.0 * m1 * l) / B1);
             out[plane + o] = q;
             out[2 * plane + o] = 2.0 * (alpha / B2);
           });
}

// grid (tiles of w, tiles of h, N) over the level's SAMPLES.  coarse: the next level's gradient [N][h / 2][w / 2] or null.
template <typename T>
__global__ __launch_bounds__(SL_THREADS) void sl_adjoint_kernel(const double* __restrict__ pqr, const float* __restrict__ x,
                                                                const float* __restrict__ y, int h, int w,
                                                                const double* __restrict__ coarse, T* __restrict__ gout) {
  __shared__ double sp[3][SL_SH][SL_SW];
  __shared__ double hq[3][SL_SH][SL_TW];
  __shared__ double g[SL_TAPS];
  const int ho = h - SL_HALO, wo = w - SL_HALO, y0 = blockIdx.y * SL_TH, x0 = blockIdx.x * SL_TW;
  const size_t plane = (size_t)ho * wo;
  const double* in = pqr + (size_t)blockIdx.z * 3 * plane;
  sl_window(g);
  for (int e = threadIdx.x; e < SL_SH * SL_SW; e += SL_THREADS) {
    const int r = e / SL_SW, c = e - r * SL_SW, py = y0 - SL_HALO + r, px = x0 - SL_HALO + c;
    const bool ok = py >= 0 && py < ho && px >= 0 && px < wo;
    const size_t o = ok ? (size_t)py * wo + px : 0;
    sp[0][r][c] = ok ? in[o] : 0.0;
    sp[1][r][c] = ok ? in[plane + o] : 0.0;
    sp[2][r][c] = ok ? in[2 * plane + o] : 0.0;
  }
  __syncthreads();
  // sample column x0 + c takes map columns x0 + c - k: staged column c + 10 - k
  for (int e = threadIdx.x; e < SL_SH * SL_TW; e += SL_THREADS) {
    const int r = e / SL_TW, c = e - r * SL_TW;
    double a = 0, b = 0, d = 0;
#pragma unroll
    for (int k = 0; k < SL_TAPS; ++k) {
      const double wk = g[k];
      a += wk * sp[0][r][c + SL_HALO - k]; b += wk * sp[1][r][c + SL_HALO - k]; d += wk * sp[2][r][c + SL_HALO - k];
    }
    hq[0][r][c] = a; hq[1][r][c] = b; hq[2][r][c] = d;
  }
  __syncthreads();
  const size_t frame = (size_t)blockIdx.z * h * w;
  const int hc = h >> 1, wc = w >> 1;
  for (int e = threadIdx.x; e < SL_TH * SL_TW; e += SL_THREADS) {
    const int r = e / SL_TW, c = e - r * SL_TW, yy = y0 + r, xx = x0 + c;
    if (yy >= h || xx >= w) continue;
    double a = 0, b = 0, d = 0;
#pragma unroll
    for (int k = 0; k < SL_TAPS; ++k) {
      const double wk = g[k];
      a += wk * hq[0][r + SL_HALO - k][c]; b += wk * hq[1][r + SL_HALO - k][c]; d += wk * hq[2][r + SL_HALO - k][c];
    }
    const size_t o = frame + (size_t)yy * w + xx;
    double v = (a + 2.0 * (double)x[o] * b) + (double)y[o] * d;
    if (coarse && (yy >> 1) < hc && (xx >> 1) < wc)       // a dropped odd row or column gets none
      v += 0.25 * coarse[(size_t)blockIdx.z * hc * wc + (size_t)(yy >> 1) * wc + (xx >> 1)];
    gout[o] = (T)v;
  }
}

inline dim3 sl_grid_valid(int h, int w, int N) { return dim3(cdiv(w - SL_HALO, SL_TW), cdiv(h - SL_HALO, SL_TH), N); }

}  // namespace

extern "C" int cdfo_ssim_loss_tiles(int H, int W, int levels) {
  if (!sl_frame_ok(H, W, levels)) return CDFO_EINVAL;
  return sl_tile_offset(H, W, levels);
}

extern "C" int cdfo_ssim_loss_level(const float* x, const float* y, int N, int H, int W, int levels, int level, double peak,
                                    double* partial, long long partial_cap, void* stream) {
  if (!x || !y || !partial || N <= 0 || N > 65535 || !sl_frame_ok(H, W, levels) || level < 0 || level >= levels || !sl_peak_ok(peak))
    return CDFO_EINVAL;
  const int stride = sl_tile_offset(H, W, levels);
  if (partial_cap < 2LL * N * stride) return CDFO_EINVAL;
  if (sl_misaligned(x, 3u) || sl_misaligned(y, 3u) || sl_misaligned(partial, 7u)) return CDFO_EALIGN;
  const int h = H >> level, w = W >> level;
  const double C1 = (0.01 * peak) * (0.01 * peak), C2 = (0.03 * peak) * (0.03 * peak);
  hipLaunchKernelGGL(sl_level_kernel, sl_grid_valid(h, w, N), dim3(SL_THREADS), 0, static_cast<hipStream_t>(stream), x, y, h, w, C1, C2,
                     partial, sl_tile_offset(H, W, level), stride);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ssim_loss_pool(const float* x, const float* y, int N, int h, int w, float* xn, float* yn, void* stream) {
  if (!x || !y || !xn || !yn || N <= 0 || N > 65535 || h < 2 * SL_TAPS || w < 2 * SL_TAPS || h > SL_MAX_SIZE || w > SL_MAX_SIZE)
    return CDFO_EINVAL;
  if (sl_misaligned(x, 3u) || sl_misaligned(y, 3u) || sl_misaligned(xn, 3u) || sl_misaligned(yn, 3u)) return CDFO_EALIGN;
  hipLaunchKernelGGL(sl_pool_kernel, dim3(cdiv((h >> 1) * (w >> 1), SL_THREADS), 2, N), dim3(SL_THREADS), 0,
                     static_cast<hipStream_t>(stream), x, y, h, w, xn, yn);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ssim_loss_combine(const double* partial, long long partial_cap, int N, int H, int W, int levels, double* means,
                                      double* coef, float* loss, void* stream) {
  if (!partial || !means || !coef || !loss || N <= 0 || N > 65535 || !sl_frame_ok(H, W, levels)) return CDFO_EINVAL;
  const int stride = sl_tile_offset(H, W, levels);
  if (partial_cap < 2LL * N * stride) return CDFO_EINVAL;
  if (sl_misaligned(partial, 7u) || sl_misaligned(means, 7u) || sl_misaligned(coef, 7u) || sl_misaligned(loss, 3u)) return CDFO_EALIGN;
  hipLaunchKernelGGL(sl_combine_kernel, dim3(cdiv(N, 64)), dim3(64), 0, static_cast<hipStream_t>(stream), partial, N, H, W, levels, stride,
                     means, coef, loss);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ssim_loss_pqr(const float* x, const float* y, int N, int H, int W, int levels, int level, double peak,
                                  const double* coef, double* pqr, long long pqr_cap, void* stream) {
  if (!x || !y || !coef || !pqr || N <= 0 || N > 65535 || !sl_frame_ok(H, W, levels) || level < 0 || level >= levels || !sl_peak_ok(peak))
    return CDFO_EINVAL;
  const int h = H >> level, w = W >> level;
  if (pqr_cap < 3LL * N * (h - SL_HALO) * (w - SL_HALO)) return CDFO_EINVAL;
  if (sl_misaligned(x, 3u) || sl_misaligned(y, 3u) || sl_misaligned(coef, 7u) || sl_misaligned(pqr, 7u)) return CDFO_EALIGN;
  const double C1 = (0.01 * peak) * (0.01 * peak), C2 = (0.03 * peak) * (0.03 * peak);
  hipLaunchKernelGGL(sl_pqr_kernel, sl_grid_valid(h, w, N), dim3(SL_THREADS), 0, static_cast<hipStream_t>(stream), x, y, h, w, C1, C2, coef,
                     levels, level, pqr);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ssim_loss_adjoint(const double* pqr, const float* x, const float* y, int N, int H, int W, int levels, int level,
                                      const double* coarse, double* g64, float* g32, void* stream) {
  if (!pqr || !x || !y || N <= 0 || N > 65535 || !sl_frame_ok(H, W, levels) || level < 0 || level >= levels) return CDFO_EINVAL;
  if ((level == 0 && !g32) || (level > 0 && !g64) || (level < levels - 1 && !coarse)) return CDFO_EINVAL;
  if (sl_misaligned(pqr, 7u) || sl_misaligned(x, 3u) || sl_misaligned(y, 3u) || sl_misaligned(coarse, 7u) || sl_misaligned(g64, 7u) ||
      sl_misaligned(g32, 3u))
    return CDFO_EALIGN;
  const int h = H >> level, w = W >> level;
  const dim3 grid(cdiv(w, SL_TW), cdiv(h, SL_TH), N);
  const double* up = level < levels - 1 ? coarse : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (level == 0)
    hipLaunchKernelGGL(sl_adjoint_kernel<float>, grid, dim3(SL_THREADS), 0, st, pqr, x, y, h, w, up, g32);
  else
    hipLaunchKernelGGL(sl_adjoint_kernel<double>, grid, dim3(SL_THREADS), 0, st, pqr, x, y, h, w, up, g64);
  CDFO_LAUNCH_CHECK();
  return 0;
}
