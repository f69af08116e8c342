// BRISQUE's 36 features of 8-bit luma frames on the device (DESIGN.md has the definition, tests/brisque_ref.py its numpy statement;
// cdfo_amd/metrics.py: brisque_features_u8 makes the seven launches of a chunk and the score from the features on the host).
//   cdfo_brisque_mscn_u8 / _f64  (x - mu) / (sigma + 1) with the 7 x 7 window over the WHOLE frame, zeros beyond its edge, fp64 out
//   cdfo_brisque_half            the fixed 8-tap half-size filter on x, rows then columns, the edge sample repeated, ceil(n / 2) outputs
//   cdfo_brisque_mscn_u16 / cdfo_brisque_half_u16   the two on 16-bit samples of a peak of 1 .. 65535: x = 255 v / peak (metric_sample.h)
//   cdfo_brisque_sums            per (strip of rows, frame) the thirty moment sums of the five maps, partners circular over the frame
//   cdfo_brisque_features        the strips added in order, the table searches (one wave each) and the 18 features of one scale
// The sibling of niqe.hip, which stays as it is: the extent, the padding, the epsilon, the fourth partner and the symmetric fit all
// differ, so the few shared lines (the mirror, the taps, the butterfly) are repeated here.  Everything is fp64 and written the way
// the statement is: the taps in the statement's order, and no contraction of a multiply with the add behind it (the pragma below).
// All stores are vector stores; there are no atomics.
#include "common.h"
#include "metric_sample.h"
#include "numeric.h"

#pragma clang fp contract(off)

namespace {

inline bool fits32(long long rows, long long pitch) { return rows * pitch <= 0x7fffffffLL; }

struct BrisqueWindow { double h[49]; };

constexpr int BQ_TW = 64, BQ_TH = 16;                 // the MSCN tile; its apron is 3 samples each way

// grid (tiles across, tiles down, frame).  T: unsigned char or unsigned short (a frame, read in place; the latter with its peak
// behind dst) or double (the half image).
template <typename T, typename... P>
__global__ __launch_bounds__(256) void brisque_mscn_kernel(const T* __restrict__ src, int pitch, long long fstride, int H, int W,
                                                           BrisqueWindow win, double* __restrict__ dst, P... peak) {
  __shared__ double t[BQ_TH + 6][BQ_TW + 6];
  const int n = blockIdx.z, y0 = blockIdx.y * BQ_TH, x0 = blockIdx.x * BQ_TW;
  const T* p = src + (long long)n * fstride;
  for (int i = threadIdx.x; i < (BQ_TH + 6) * (BQ_TW + 6); i += 256) {
    const int r = i / (BQ_TW + 6), c = i - r * (BQ_TW + 6);
    const int y = y0 + r - 3, x = x0 + c - 3;
    t[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? metric_sample(p[y * pitch + x], peak...) : 0.0;      // zeros beyond the FRAME
  }
  __syncthreads();
  double* out = dst + (long long)n * H * W;
  for (int i = threadIdx.x; i < BQ_TH * BQ_TW; i += 256) {
    const int r = i / BQ_TW, c = i - r * BQ_TW;
    if (y0 + r >= H || x0 + c >= W) continue;
    double mu = 0.0, sq = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int b = 0; b < 7; ++b) {
        const double v = t[r + a][c + b], h = win.h[a * 7 + b];
        mu = mu + h * v;
        sq = sq + h * (v * v);
      }
    const double sigma = sqrt(fabs(sq - mu * mu) + 0x1p-23);          // the reference's fp32 epsilon
    out[(y0 + r) * W + x0 + c] = (t[r + 3][c + 3] - mu) / (sigma + 1.0);
  }
}

constexpr int BQ_HT = 16;                               // the half image's tile, 16 x 16 outputs of 38 x 38 inputs

__device__ __forceinline__ int brisque_mirror(int i, int n) {   // [a,b,c] -> [c,b,a,a,b,c,c,b,a]; clamped beyond that (never read there)
  i = i < 0 ? -1 - i : i >= n ? 2 * n - 1 - i : i;
  return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

// grid (tiles across, tiles down, frame) over the ceil(H/2) x ceil(W/2) outputs.  T, peak: as brisque_mscn_kernel's.
template <typename T, typename... P>
__global__ __launch_bounds__(256) void brisque_half_kernel(const T* __restrict__ src, int pitch, long long fstride, int H, int W,
                                                           double* __restrict__ dst, P... peak) {
  constexpr int IN = 2 * BQ_HT + 6;
  __shared__ double tin[IN][IN], mid[BQ_HT][IN];
  const double w[8] = {-3.0 / 256, -9.0 / 256, 29.0 / 256, 111.0 / 256, 111.0 / 256, 29.0 / 256, -9.0 / 256, -3.0 / 256};
  const int n = blockIdx.z, oy0 = blockIdx.y * BQ_HT, ox0 = blockIdx.x * BQ_HT;
  const T* p = src + (long long)n * fstride;
  for (int i = threadIdx.x; i < IN * IN; i += 256) {
    const int r = i / IN, c = i - r * IN;
    const int y = brisque_mirror(2 * oy0 - 3 + r, H), x = brisque_mirror(2 * ox0 - 3 + c, W);
    tin[r][c] = metric_sample(p[y * pitch + x], peak...);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BQ_HT * IN; i += 256) {   // rows first: output row r of inputs 2r-3 .. 2r+4
    const int r = i / IN, c = i - r * IN;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = s + w[k] * tin[2 * r + k][c];
    mid[r][c] = s;
  }
  __syncthreads();
  const int r = threadIdx.x / BQ_HT, c = threadIdx.x - r * BQ_HT;
  const int Hh = (H + 1) / 2, Wh = (W + 1) / 2;
  if (oy0 + r < Hh && ox0 + c < Wh) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = s + w[k] * mid[r][2 * c + k];
    dst[(long long)n * Hh * Wh + (oy0 + r) * Wh + ox0 + c] = s;
  }
}

// grid (strip, frame); strip g is the rows 16 g .. 16 g + 15 of the map, so the strip count is a function of the shape alone.
// partials [K][G][5][6]: per map (count < 0, count > 0, sum v^2 over < 0, over > 0, sum |v|, sum v^2).  The partners m[r][c-1],
// m[r-1][c], m[r-1][c-1], m[r+1][c-1] are read from the map with the indices modulo H and W, so they cross strips and wrap round
// the frame.  A thread's partials, the wave's butterfly, then the four waves in order through LDS: equal inputs give equal bits.
__global__ __launch_bounds__(256) void brisque_sums_kernel(const double* __restrict__ m, int H, int W, double* __restrict__ partials) {
  __shared__ double sh[4][30];
  const int n = blockIdx.y, r0 = blockIdx.x * CDFO_BRISQUE_STRIP;
  const int rows = H - r0 < CDFO_BRISQUE_STRIP ? H - r0 : CDFO_BRISQUE_STRIP;
  const double* p = m + (long long)n * H * W;
  double acc[30];
#pragma unroll
  for (int j = 0; j < 30; ++j) acc[j] = 0.0;
  for (int i = threadIdx.x; i < rows * W; i += 256) {
    const int q = i / W, c = i - q * W, r = r0 + q;
    const int ru = r ? r - 1 : H - 1, rd = r + 1 < H ? r + 1 : 0, cl = c ? c - 1 : W - 1;        // circular over the frame
    const double x = p[r * W + c];
    const double v[5] = {x, x * p[r * W + cl], x * p[ru * W + c], x * p[ru * W + cl], x * p[rd * W + cl]};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double q2 = v[k] * v[k];
      const bool neg = v[k] < 0.0, pos = v[k] > 0.0;
      acc[6 * k + 0] += neg ? 1.0 : 0.0;
      acc[6 * k + 1] += pos ? 1.0 : 0.0;
      acc[6 * k + 2] += neg ? q2 : 0.0;
      acc[6 * k + 3] += pos ? q2 : 0.0;
      acc[6 * k + 4] += fabs(v[k]);
      acc[6 * k + 5] += q2;
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 30; ++j) {
    double s = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sh[wave][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < 30)
    partials[((long long)n * gridDim.x + blockIdx.x) * 30 + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// grid (frame), 320 threads: the G strips are added in index order, then wave k searches the table for map k and its lane 0 writes
// the map's features into features[n * 36 + 18 scale ...].  table: gam [9801], r_gam [9801], r_ggd [9801]; the map itself is fitted
// symmetrically against r_ggd, its four products asymmetrically against r_gam.
__global__ __launch_bounds__(320) void brisque_features_kernel(const double* __restrict__ partials, int G, double count,
                                                               const double* __restrict__ table, int scale, double* __restrict__ features) {
  __shared__ double sh[30];
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x < 30) {
    const double* q = partials + (long long)blockIdx.x * G * 30 + threadIdx.x;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += q[(long long)g * 30];
    sh[threadIdx.x] = s;
  }
  __syncthreads();
  const double* s = sh + 6 * k;
  const double ls = sqrt(s[2] / s[0]), rs = sqrt(s[3] / s[1]), g = ls / rs;
  const double ma = s[4] / count, ms = s[5] / count;
  const double g2 = g * g + 1.0;
  const double x = k == 0 ? ms / (ma * ma) : (ma * ma / ms) * (g * g * g + 1.0) * (g + 1.0) / (g2 * g2);
  const double* row = table + (k == 0 ? 2 : 1) * CDFO_BRISQUE_TABLE;
  double best = __builtin_inf();
  int at = 0x7fffffff;                                   // stays with a NaN x (no distance compares below): index 0
  for (int i = lane; i < CDFO_BRISQUE_TABLE; i += 64) {
    const double d = fabs(row[i] - x);
    if (d < best) { best = d; at = i; }                  // strict: the first minimum of the lane's stride
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(at, o, 64);
    if (od < best || (od == best && oi < at)) { best = od; at = oi; }      // the lower index on equal distance
  }
  if (lane != 0) return;
  const double alpha = table[at == 0x7fffffff ? 0 : at];
  double* f = features + (long long)blockIdx.x * 36 + 18 * scale;
  if (k == 0) {
    f[0] = alpha;
    f[1] = ms;
  } else {
    f += 4 * k - 2;
    f[0] = alpha;
    f[1] = (rs - ls) * exp(lgamma(2.0 / alpha) - (lgamma(1.0 / alpha) + lgamma(3.0 / alpha)) / 2.0);
    f[2] = ls * ls;
    f[3] = rs * rs;
  }
}

// peak: empty, or the peak of 16-bit samples, checked by the entry point
template <typename T, typename... P>
int brisque_mscn(const T* src, int pitch, long long fstride, int K, int H, int W, const double* window, double* dst, void* stream, P... peak) {
  if (!src || !window || !dst || K <= 0 || K > 65535 || H <= 0 || W <= 0 || pitch < W || fstride < 0) return CDFO_EINVAL;
  if (!fits32(H, pitch) || !fits32(H, W) || cdiv(H, BQ_TH) > 65535) return CDFO_EINVAL;        // 32-bit offsets inside a frame
  if ((reinterpret_cast<uintptr_t>(dst) & 7u) || (reinterpret_cast<uintptr_t>(src) & (sizeof(T) - 1))) return CDFO_EALIGN;
  BrisqueWindow win;
  for (int i = 0; i < 49; ++i) win.h[i] = window[i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 5.0 * 49 * K * (double)H * W, (sizeof(T) + 8.0) * K * (double)H * W);
  hipLaunchKernelGGL((brisque_mscn_kernel<T, P...>), dim3((unsigned)cdiv(W, BQ_TW), (unsigned)cdiv(H, BQ_TH), (unsigned)K), dim3(256), 0, st, src,
                     pitch, fstride, H, W, win, dst, peak...);
  CDFO_LAUNCH_CHECK();
  return 0;
}

template <typename T, typename... P>
int brisque_half(const T* src, int pitch, long long fstride, int K, int H, int W, double* dst, void* stream, P... peak) {
  if (!src || !dst || K <= 0 || K > 65535 || H < 8 || W < 8 || pitch < W || fstride < 0) return CDFO_EINVAL;
  if (!fits32(H, pitch) || cdiv((H + 1) / 2, BQ_HT) > 65535) return CDFO_EINVAL;               // 32-bit offsets inside a frame
  if ((reinterpret_cast<uintptr_t>(dst) & 7u) || (reinterpret_cast<uintptr_t>(src) & (sizeof(T) - 1))) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 8 * K * 0.75 * H * W, K * (double)H * W * (2.0 + sizeof(T)));
  hipLaunchKernelGGL((brisque_half_kernel<T, P...>), dim3((unsigned)cdiv((W + 1) / 2, BQ_HT), (unsigned)cdiv((H + 1) / 2, BQ_HT), (unsigned)K),
                     dim3(256), 0, st, src, pitch, fstride, H, W, dst, peak...);
  CDFO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cdfo_brisque_mscn_u8(const unsigned char* src, int pitch, long long fstride, int K, int H, int W, const double* window,
                                    double* dst, void* stream) {
  return brisque_mscn<unsigned char>(src, pitch, fstride, K, H, W, window, dst, stream);
}

extern "C" int cdfo_brisque_mscn_f64(const double* src, int pitch, long long fstride, int K, int H, int W, const double* window,
                                     double* dst, void* stream) {
  return brisque_mscn<double>(src, pitch, fstride, K, H, W, window, dst, stream);
}

extern "C" int cdfo_brisque_mscn_u16(const unsigned short* src, int pitch, long long fstride, int K, int H, int W, const double* window,
                                     double* dst, int peak, void* stream) {
  if (peak < 1 || peak > 65535) return CDFO_EINVAL;
  return brisque_mscn<unsigned short>(src, pitch, fstride, K, H, W, window, dst, stream, (double)peak);
}

extern "C" int cdfo_brisque_half(const unsigned char* src, int pitch, long long fstride, int K, int H, int W, double* dst, void* stream) {
  return brisque_half<unsigned char>(src, pitch, fstride, K, H, W, dst, stream);
}

extern "C" int cdfo_brisque_half_u16(const unsigned short* src, int pitch, long long fstride, int K, int H, int W, double* dst, int peak,
                                     void* stream) {
  if (peak < 1 || peak > 65535) return CDFO_EINVAL;
  return brisque_half<unsigned short>(src, pitch, fstride, K, H, W, dst, stream, (double)peak);
}

extern "C" int cdfo_brisque_sums(const double* mscn, int K, int H, int W, double* partials, void* stream) {
  if (!mscn || !partials || K <= 0 || K > 65535 || H < 2 || W < 2) return CDFO_EINVAL;
  if (!fits32(H, W)) return CDFO_EINVAL;                                                        // 32-bit offsets inside a frame
  if ((reinterpret_cast<uintptr_t>(mscn) | reinterpret_cast<uintptr_t>(partials)) & 7u) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 40.0 * K * (double)H * W, 8.0 * K * (double)H * W);
  hipLaunchKernelGGL(brisque_sums_kernel, dim3((unsigned)cdiv(H, CDFO_BRISQUE_STRIP), (unsigned)K), dim3(256), 0, st, mscn, H, W, partials);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_brisque_features(const double* partials, int K, int G, int count, const double* table, int scale, double* features,
                                     void* stream) {
  if (!partials || !table || !features || K <= 0 || G <= 0 || count <= 0 || (scale != 0 && scale != 1)) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(features)) & 7u)
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 5 * CDFO_BRISQUE_TABLE * (double)K, 8.0 * 5 * CDFO_BRISQUE_TABLE * (double)K);
  hipLaunchKernelGGL(brisque_features_kernel, dim3((unsigned)K), dim3(320), 0, st, partials, G, (double)count, table, scale, features);
  CDFO_LAUNCH_CHECK();
  return 0;
}
