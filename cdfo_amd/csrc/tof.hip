// tOF's dense Farneback flow of 8-bit luma pairs on the device (DESIGN.md has the definition, tests/tof_ref.py its numpy statement;
// cdfo_amd/metrics.py: farneback_u8 / tof_frames_u8 make the launches of a chunk, stage by stage).  Pairs are the batch dimension:
//   cdfo_tof_level_u8    u8 frames -> the fp64 level images of every pair (prev, cur): stage smoothing and bilinear resize fused
//   cdfo_tof_level_u16   the same of 16-bit frames of a peak of 1 .. 65535: x = 255 v / peak (metric_sample.h)
//   cdfo_tof_polyexp     level images -> the five coefficient planes (b_x, b_y, a_xx, a_yy, a_xy): both 11-tap passes through LDS
//   cdfo_tof_matrices    both expansions and the flow -> the five planes of the normal equations (the gather, the border factors)
//   cdfo_tof_blur_solve  15 x 15 box mean through LDS, plane by plane, then the 2 x 2 solve: the new flow
//   cdfo_tof_flow_up     a stage's flow on the next stage's grid, times 2
//   cdfo_tof_epe         per strip of rows the sum of endpoint distances of two flows; one workgroup per frame adds them in order
// Everything is fp64 and written the way the statement is: the taps in the statement's order from an accumulator of 0.0.  The
// pragma below is niqe.hip's and brisque.hip's convention; the library is built with -ffp-contract=fast, under which clang
// disregards it, so some multiply-adds are still fused (one rounding instead of two): against the statement that is a few units in
// the last place per stage and 2e-15 px in a solved flow (DESIGN.md has the measurements).  Grids depend on the shapes alone, all
// stores are vector stores and there are no atomics: equal frames give equal bits.
#include "common.h"
#include "metric_sample.h"

#pragma clang fp contract(off)

namespace {

inline bool fits32(long long rows, long long pitch) { return rows * pitch <= 0x7fffffffLL; }
inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

struct TofTaps { double t[CDFO_TOF_MAX_TAPS]; };
struct TofPoly { double g[11], xg[11], xxg[11], ig11, ig03, ig33, ig55; };

__device__ __forceinline__ int tof_reflect101(int i, int n) {          // dcb|abcd|cba; one reflection (radius < n), then clamped
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}
__device__ __forceinline__ int tof_clamp(int i, int n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// the smoothed sample at (yc, xc): down the columns first, then along the row.  T, peak: as tof_level_kernel's.
template <typename T, typename... P>
__device__ __forceinline__ double tof_smooth(const T* __restrict__ p, int pitch, int H, int W, int yc, int xc, const TofTaps& taps, int n,
                                             P... peak) {
  const int r = (n - 1) >> 1;
  double s = 0.0;
  for (int j = 0; j < n; ++j) {
    const int x = tof_reflect101(xc + j - r, W);
    double col = 0.0;
    for (int i = 0; i < n; ++i) col = col + taps.t[i] * metric_sample(p[tof_reflect101(yc + i - r, H) * pitch + x], peak...);
    s = s + taps.t[j] * col;
  }
  return s;
}

// the resize's source position of output i: (i0, i1) clamped into [0, N), the weight from the unclamped floor
__device__ __forceinline__ void tof_resize_at(int i, int N, int n, int& i0, int& i1, double& wgt) {
  const double f = ((double)i + 0.5) * ((double)N / (double)n) - 0.5;
  const double fl = floor(f);
  wgt = f - fl;
  const int k = (int)fl;                                               // -1 .. N - 1
  i0 = tof_clamp(k, N);
  i1 = tof_clamp(k + 1, N);
}

// grid (tiles of 64 across, tiles of 4 down, 2 K): z = 2 pair + slot, slot 0 the pair's previous frame, 1 its current one.
// dst [K][2][h][w].  A weight of exactly 0 (always at h == H, w == W) drops its second sample: (1 - 0) a + 0 b == a.
// T: unsigned char, or unsigned short with the samples' peak behind dst (metric_sample.h).
template <typename T, typename... P>
__global__ __launch_bounds__(256) void tof_level_kernel(const T* __restrict__ prev, int ppitch, long long pstride,
                                                        const T* __restrict__ cur, int cpitch, long long cstride,
                                                        const T* __restrict__ first, int fpitch, int H, int W, int h,
                                                        int w, TofTaps taps, int n, double* __restrict__ dst, P... peak) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int pair = blockIdx.z >> 1, slot = blockIdx.z & 1;
  const T* p;
  int pitch;
  if (slot) {
    p = cur + (long long)pair * cstride;
    pitch = cpitch;
  } else if (first) {
    p = pair ? prev + (long long)(pair - 1) * pstride : first;
    pitch = pair ? ppitch : fpitch;
  } else {
    p = prev + (long long)pair * pstride;
    pitch = ppitch;
  }
  int y0, y1, x0, x1;
  double wy, wx;
  tof_resize_at(y, H, h, y0, y1, wy);
  tof_resize_at(x, W, w, x0, x1, wx);
  const bool one_x = wx == 0.0 || x1 == x0;
  const double s00 = tof_smooth(p, pitch, H, W, y0, x0, taps, n, peak...);
  const double s01 = one_x ? s00 : tof_smooth(p, pitch, H, W, y0, x1, taps, n, peak...);
  const double top = (1.0 - wx) * s00 + wx * s01;
  double bot = top;
  if (!(wy == 0.0 || y1 == y0)) {
    const double s10 = tof_smooth(p, pitch, H, W, y1, x0, taps, n, peak...);
    const double s11 = one_x ? s10 : tof_smooth(p, pitch, H, W, y1, x1, taps, n, peak...);
    bot = (1.0 - wx) * s10 + wx * s11;
  }
  dst[(long long)blockIdx.z * h * w + y * w + x] = (1.0 - wy) * top + wy * bot;
}

constexpr int PX_TW = 32, PX_TH = 16, PX_A = 5;          // the expansion's tile and its apron

// grid (tiles across, tiles down, images).  img [N][h][w] -> R [N][5][h][w]; the edge sample repeated beyond the border.
__global__ __launch_bounds__(256) void tof_polyexp_kernel(const double* __restrict__ img, int h, int w, TofPoly k, double* __restrict__ R) {
  constexpr int IW = PX_TW + 2 * PX_A, IH = PX_TH + 2 * PX_A;
  __shared__ double tin[IH][IW], mid[3][PX_TH][IW];
  const int y0 = blockIdx.y * PX_TH, x0 = blockIdx.x * PX_TW;
  const double* p = img + (long long)blockIdx.z * h * w;
  for (int i = threadIdx.x; i < IH * IW; i += 256) {
    const int r = i / IW, c = i - r * IW;
    tin[r][c] = p[tof_clamp(y0 + r - PX_A, h) * w + tof_clamp(x0 + c - PX_A, w)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PX_TH * IW; i += 256) {   // down the columns: g, x g, x^2 g
    const int r = i / IW, c = i - r * IW;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int j = 0; j < 11; ++j) {
      const double v = tin[r + j][c];
      a0 = a0 + k.g[j] * v;
      a1 = a1 + k.xg[j] * v;
      a2 = a2 + k.xxg[j] * v;
    }
    mid[0][r][c] = a0;
    mid[1][r][c] = a1;
    mid[2][r][c] = a2;
  }
  __syncthreads();
  double* out = R + (long long)blockIdx.z * 5 * h * w;
  const int hw = h * w;
  for (int i = threadIdx.x; i < PX_TH * PX_TW; i += 256) {
    const int r = i / PX_TW, c = i - r * PX_TW;
    if (y0 + r >= h || x0 + c >= w) continue;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0;
#pragma unroll
    for (int j = 0; j < 11; ++j) {
      const double v0 = mid[0][r][c + j], v1 = mid[1][r][c + j], v2 = mid[2][r][c + j];
      m0 = m0 + k.g[j] * v0;
      m1 = m1 + k.xg[j] * v0;
      m3 = m3 + k.xxg[j] * v0;
      m2 = m2 + k.g[j] * v1;
      m5 = m5 + k.xg[j] * v1;
      m4 = m4 + k.g[j] * v2;
    }
    const int at = (y0 + r) * w + x0 + c;
    out[at] = m1 * k.ig11;
    out[hw + at] = m2 * k.ig11;
    out[2 * hw + at] = m0 * k.ig03 + m3 * k.ig33;
    out[3 * hw + at] = m0 * k.ig03 + m4 * k.ig33;
    out[4 * hw + at] = m5 * k.ig55;
  }
}

__device__ __forceinline__ double tof_border(int x, int y, int w, int h) {      // left, right, top, bottom, from 1.0
  const double b[5] = {0.14, 0.14, 0.4472, 0.4472, 0.4472};
  double s = 1.0;
  if (x < 5) s = s * b[x];
  if (x >= w - 5) s = s * b[w - 1 - x];
  if (y < 5) s = s * b[y];
  if (y >= h - 5) s = s * b[h - 1 - y];
  return s;
}

// grid (blocks of 256 pixels, pair).  R [N][2][5][h][w] (the pair's previous, then current expansion), flow [N][h][w][2] or NULL
// (zeros) -> M [N][5][h][w].  "Inside" is decided on the doubles, so no sample position is ever formed from an out-of-range value.
__global__ __launch_bounds__(256) void tof_matrices_kernel(const double* __restrict__ R, const double* __restrict__ flow, int h, int w,
                                                           double* __restrict__ M) {
  const int hw = h * w, at = blockIdx.x * 256 + threadIdx.x;
  if (at >= hw) return;
  const int y = at / w, x = at - y * w;
  const double* R0 = R + (long long)blockIdx.y * 10 * hw;
  const double* R1 = R0 + 5LL * hw;
  double dx = 0.0, dy = 0.0;
  if (flow) {
    const double2 f = reinterpret_cast<const double2*>(flow + (long long)blockIdx.y * 2 * hw)[at];
    dx = f.x;
    dy = f.y;
  }
  const double fx = (double)x + dx, fy = (double)y + dy;
  const bool inside = fx >= 0.0 && fx < (double)(w - 1) && fy >= 0.0 && fy < (double)(h - 1);
  double axx = R0[2 * hw + at], ayy = R0[3 * hw + at], axy = R0[4 * hw + at], b1x = 0.0, b1y = 0.0;
  if (inside) {
    const int x1 = (int)floor(fx), y1 = (int)floor(fy);                          // 0 .. w - 2, 0 .. h - 2
    const double a0 = fx - (double)x1, a1 = fy - (double)y1;
    const double w00 = (1.0 - a1) * (1.0 - a0), w01 = (1.0 - a1) * a0, w10 = a1 * (1.0 - a0), w11 = a1 * a0;
    const int q = y1 * w + x1;
    double S[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const double* r = R1 + (long long)c * hw + q;
      S[c] = ((w00 * r[0] + w01 * r[1]) + w10 * r[w]) + w11 * r[w + 1];
    }
    axx = (axx + S[2]) * 0.5;
    ayy = (ayy + S[3]) * 0.5;
    axy = (axy + S[4]) * 0.25;
    b1x = S[0];
    b1y = S[1];
  } else {
    axy = axy * 0.5;
  }
  double bx = ((R0[at] - b1x) * 0.5 + axx * dx) + axy * dy;
  double by = ((R0[hw + at] - b1y) * 0.5 + axy * dx) + ayy * dy;
  const double s = tof_border(x, y, w, h);
  axx = axx * s;
  ayy = ayy * s;
  axy = axy * s;
  bx = bx * s;
  by = by * s;
  double* out = M + (long long)blockIdx.y * 5 * hw + at;
  out[0] = axx * axx + axy * axy;
  out[hw] = (axx + ayy) * axy;
  out[2 * hw] = ayy * ayy + axy * axy;
  out[3 * hw] = axx * bx + axy * by;
  out[4 * hw] = axy * bx + ayy * by;
}

constexpr int BS_TW = 32, BS_TH = 16, BS_A = 7;          // the box's tile and its apron

// grid (tiles across, tiles down, pair).  M [N][5][h][w] -> flow [N][h][w][2].  Per plane: 15 rows added top to bottom, 15 of those
// sums added left to right, / 225; direct sums, the edge sample repeated.
__global__ __launch_bounds__(256) void tof_blur_solve_kernel(const double* __restrict__ M, int h, int w, double* __restrict__ flow) {
  constexpr int IW = BS_TW + 2 * BS_A, IH = BS_TH + 2 * BS_A;
  __shared__ double tin[IH][IW], mid[BS_TH][IW], mean[5][BS_TH * BS_TW];
  const int y0 = blockIdx.y * BS_TH, x0 = blockIdx.x * BS_TW, hw = h * w;
#pragma unroll 1
  for (int pl = 0; pl < 5; ++pl) {
    const double* p = M + ((long long)blockIdx.z * 5 + pl) * hw;
    for (int i = threadIdx.x; i < IH * IW; i += 256) {
      const int r = i / IW, c = i - r * IW;
      tin[r][c] = p[tof_clamp(y0 + r - BS_A, h) * w + tof_clamp(x0 + c - BS_A, w)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BS_TH * IW; i += 256) {
      const int r = i / IW, c = i - r * IW;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 15; ++j) s = s + tin[r + j][c];
      mid[r][c] = s;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = threadIdx.x + 256 * e, r = i / BS_TW, c = i - r * BS_TW;
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 15; ++j) s = s + mid[r][c + j];
      mean[pl][i] = s / 225.0;                            // read back by the thread that wrote it
    }
    __syncthreads();                                      // the next plane overwrites both tiles
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = threadIdx.x + 256 * e, r = i / BS_TW, c = i - r * BS_TW;
    if (y0 + r >= h || x0 + c >= w) continue;
    const double g11 = mean[0][i], g12 = mean[1][i], g22 = mean[2][i], h1 = mean[3][i], h2 = mean[4][i];
    const double idet = 1.0 / ((g11 * g22 - g12 * g12) + 1e-3);
    double2 f;
    f.x = (g22 * h1 - g12 * h2) * idet;
    f.y = (g11 * h2 - g12 * h1) * idet;
    reinterpret_cast<double2*>(flow + (long long)blockIdx.z * 2 * hw)[(y0 + r) * w + x0 + c] = f;
  }
}

// grid (blocks of 256 pixels, pair).  src [N][hp][wp][2] -> dst [N][h][w][2] = 2 * bilinear resize (x on both rows, then y)
__global__ __launch_bounds__(256) void tof_flow_up_kernel(const double* __restrict__ src, int hp, int wp, int h, int w,
                                                          double* __restrict__ dst) {
  const int at = blockIdx.x * 256 + threadIdx.x;
  if (at >= h * w) return;
  const int y = at / w, x = at - y * w;
  int y0, y1, x0, x1;
  double wy, wx;
  tof_resize_at(y, hp, h, y0, y1, wy);
  tof_resize_at(x, wp, w, x0, x1, wx);
  const double2* p = reinterpret_cast<const double2*>(src + (long long)blockIdx.y * 2 * hp * wp);
  const double2 a = p[y0 * wp + x0], b = p[y0 * wp + x1], c = p[y1 * wp + x0], d = p[y1 * wp + x1];
  double2 o;
  o.x = 2.0 * ((1.0 - wy) * ((1.0 - wx) * a.x + wx * b.x) + wy * ((1.0 - wx) * c.x + wx * d.x));
  o.y = 2.0 * ((1.0 - wy) * ((1.0 - wx) * a.y + wx * b.y) + wy * ((1.0 - wx) * c.y + wx * d.y));
  reinterpret_cast<double2*>(dst + (long long)blockIdx.y * 2 * h * w)[at] = o;
}

// grid (strip, frame); strip g is the rows 16 g .. 16 g + 15.  A thread's partial, the wave's butterfly, the four waves in order.
__global__ __launch_bounds__(256) void tof_epe_strips_kernel(const double* __restrict__ a, const double* __restrict__ b, int h, int w,
                                                             double* __restrict__ partials) {
  __shared__ double sh[4];
  const int n = blockIdx.y, r0 = blockIdx.x * CDFO_TOF_STRIP;
  const int rows = h - r0 < CDFO_TOF_STRIP ? h - r0 : CDFO_TOF_STRIP;
  const double2* pa = reinterpret_cast<const double2*>(a + (long long)n * 2 * h * w) + r0 * w;
  const double2* pb = reinterpret_cast<const double2*>(b + (long long)n * 2 * h * w) + r0 * w;
  double acc = 0.0;
  for (int i = threadIdx.x; i < rows * w; i += 256) {
    const double2 u = pa[i], v = pb[i];
    const double ex = u.x - v.x, ey = u.y - v.y;
    acc = acc + sqrt(ex * ex + ey * ey);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[(long long)n * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// grid (frame), one wave: the G strips added in index order, divided by the pixel count
__global__ __launch_bounds__(64) void tof_epe_mean_kernel(const double* __restrict__ partials, int G, double count, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const double* q = partials + (long long)blockIdx.x * G;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s = s + q[g];
  out[blockIdx.x] = s / count;
}

// peak: empty, or the peak of 16-bit samples, checked by the entry point
template <typename T, typename... P>
int tof_level(const T* prev, int ppitch, long long pstride, const T* cur, int cpitch, long long cstride, const T* first, int fpitch, int K,
              int H, int W, int h, int w, const double* taps, int ntaps, double* dst, void* stream, P... peak) {
  if (!prev || !cur || !taps || !dst || K <= 0 || 2 * (long long)K > 65535 || H < CDFO_TOF_MIN || W < CDFO_TOF_MIN) return CDFO_EINVAL;
  if (h <= 0 || w <= 0 || h > H || w > W || ppitch < W || cpitch < W || (first && fpitch < W) || pstride < 0 || cstride < 0) return CDFO_EINVAL;
  if (ntaps < 3 || ntaps > CDFO_TOF_MAX_TAPS || !(ntaps & 1) || ntaps / 2 >= (H < W ? H : W)) return CDFO_EINVAL;   // one reflection
  if (!fits32(H, ppitch) || !fits32(H, cpitch) || (first && !fits32(H, fpitch)) || !fits32(h, w) || cdiv(h, 4) > 65535) return CDFO_EINVAL;
  if (misaligned8(dst)) return CDFO_EALIGN;
  if ((reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(first)) & (sizeof(T) - 1))
    return CDFO_EALIGN;
  TofTaps t;
  for (int i = 0; i < CDFO_TOF_MAX_TAPS; ++i) t.t[i] = i < ntaps ? taps[i] : 0.0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 8.0 * ntaps * ntaps * K * (double)h * w, 2.0 * K * (sizeof(T) * (double)H * W + 8.0 * h * w));
  hipLaunchKernelGGL((tof_level_kernel<T, P...>), dim3((unsigned)cdiv(w, 64), (unsigned)cdiv(h, 4), (unsigned)(2 * K)), dim3(256), 0, st, prev,
                     ppitch, pstride, cur, cpitch, cstride, first, fpitch, H, W, h, w, t, ntaps, dst, peak...);
  CDFO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cdfo_tof_level_u8(const unsigned char* prev, int ppitch, long long pstride, const unsigned char* cur, int cpitch,
                                 long long cstride, const unsigned char* first, int fpitch, int K, int H, int W, int h, int w,
                                 const double* taps, int ntaps, double* dst, void* stream) {
  return tof_level<unsigned char>(prev, ppitch, pstride, cur, cpitch, cstride, first, fpitch, K, H, W, h, w, taps, ntaps, dst, stream);
}

extern "C" int cdfo_tof_level_u16(const unsigned short* prev, int ppitch, long long pstride, const unsigned short* cur, int cpitch,
                                  long long cstride, const unsigned short* first, int fpitch, int K, int H, int W, int h, int w,
                                  const double* taps, int ntaps, double* dst, int peak, void* stream) {
  if (peak < 1 || peak > 65535) return CDFO_EINVAL;
  return tof_level<unsigned short>(prev, ppitch, pstride, cur, cpitch, cstride, first, fpitch, K, H, W, h, w, taps, ntaps, dst, stream,
                                   (double)peak);
}

extern "C" int cdfo_tof_polyexp(const double* img, int N, int h, int w, const double* kernels, double* R, void* stream) {
  if (!img || !kernels || !R || N <= 0 || N > 65535 || h <= 0 || w <= 0) return CDFO_EINVAL;
  if (!fits32(5LL * h, w) || cdiv(h, PX_TH) > 65535) return CDFO_EINVAL;                        // 32-bit offsets inside an image's planes
  if (misaligned8(img) || misaligned8(R)) return CDFO_EALIGN;
  TofPoly k;
  for (int i = 0; i < 11; ++i) {
    k.g[i] = kernels[i];
    k.xg[i] = kernels[11 + i];
    k.xxg[i] = kernels[22 + i];
  }
  k.ig11 = kernels[33];
  k.ig03 = kernels[34];
  k.ig33 = kernels[35];
  k.ig55 = kernels[36];
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 99 * N * (double)h * w, 48.0 * N * (double)h * w);
  hipLaunchKernelGGL(tof_polyexp_kernel, dim3((unsigned)cdiv(w, PX_TW), (unsigned)cdiv(h, PX_TH), (unsigned)N), dim3(256), 0, st, img, h, w, k, R);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_tof_matrices(const double* R, const double* flow, int N, int h, int w, double* M, void* stream) {
  if (!R || !M || N <= 0 || N > 65535 || h < 2 || w < 2) return CDFO_EINVAL;
  if (!fits32(5LL * h, w)) return CDFO_EINVAL;
  if (misaligned8(R) || misaligned8(M) || (reinterpret_cast<uintptr_t>(flow) & 15u)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 90.0 * N * (double)h * w, 8.0 * 27 * N * (double)h * w);
  hipLaunchKernelGGL(tof_matrices_kernel, dim3((unsigned)cdiv(h * w, 256), (unsigned)N), dim3(256), 0, st, R, flow, h, w, M);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_tof_blur_solve(const double* M, int N, int h, int w, double* flow, void* stream) {
  if (!M || !flow || N <= 0 || N > 65535 || h <= 0 || w <= 0) return CDFO_EINVAL;
  if (!fits32(5LL * h, w) || cdiv(h, BS_TH) > 65535) return CDFO_EINVAL;
  if (misaligned8(M) || (reinterpret_cast<uintptr_t>(flow) & 15u)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 5.0 * 30 * N * (double)h * w, 8.0 * 7 * N * (double)h * w);
  hipLaunchKernelGGL(tof_blur_solve_kernel, dim3((unsigned)cdiv(w, BS_TW), (unsigned)cdiv(h, BS_TH), (unsigned)N), dim3(256), 0, st, M, h, w, flow);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_tof_flow_up(const double* src, int N, int hp, int wp, int h, int w, double* dst, void* stream) {
  if (!src || !dst || N <= 0 || N > 65535 || hp <= 0 || wp <= 0 || h <= 0 || w <= 0) return CDFO_EINVAL;
  if (!fits32(2LL * hp, wp) || !fits32(2LL * h, w)) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 16.0 * N * (double)h * w, 16.0 * N * ((double)h * w + (double)hp * wp));
  hipLaunchKernelGGL(tof_flow_up_kernel, dim3((unsigned)cdiv(h * w, 256), (unsigned)N), dim3(256), 0, st, src, hp, wp, h, w, dst);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_tof_epe(const double* a, const double* b, int K, int h, int w, double* partials, double* out, void* stream) {
  if (!a || !b || !partials || !out || K <= 0 || K > 65535 || h <= 0 || w <= 0) return CDFO_EINVAL;
  if (!fits32(2LL * h, w)) return CDFO_EINVAL;
  if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) || misaligned8(partials) || misaligned8(out)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = cdiv(h, CDFO_TOF_STRIP);
  CdfoProfScope prof(st, KID_LAYOUT, 8.0 * K * (double)h * w, 32.0 * K * (double)h * w);
  hipLaunchKernelGGL(tof_epe_strips_kernel, dim3((unsigned)G, (unsigned)K), dim3(256), 0, st, a, b, h, w, partials);
  CDFO_LAUNCH_CHECK();
  hipLaunchKernelGGL(tof_epe_mean_kernel, dim3((unsigned)K), dim3(64), 0, st, partials, G, (double)h * (double)w, out);
  CDFO_LAUNCH_CHECK();
  return 0;
}
