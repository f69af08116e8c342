// NIQE's per-block features of 8-bit luma frames on the device (DESIGN.md has the definition, tests/niqe_ref.py its numpy statement;
// cdfo_amd/metrics.py: niqe_features_u8 makes the seven launches of a chunk and the score from the features on the host).
//   cdfo_niqe_mscn_u8 / _f64   (x - mu) / (sigma + 1) with the 7 x 7 window, replicate padding at the edge of the region, fp64 out
//   cdfo_niqe_half             the fixed 8-tap half-size filter on x / 255, rows then columns, the edge sample repeated, * 255
//   cdfo_niqe_mscn_u16 / cdfo_niqe_half_u16   the two on 16-bit samples of a peak of 1 .. 65535: x = 255 v / peak (metric_sample.h)
//   cdfo_niqe_block_sums       per (frame, block) the thirty moment sums of the five maps, in a fixed order
//   cdfo_niqe_features         the table search (one wave each) and the 18 features of one scale
// Everything is fp64 and written the way the statement is: the taps in the statement's order, and no contraction of a multiply with
// the add behind it (the pragma below), so the maps differ from numpy's by the library functions' last bits only.  All stores are
// vector stores.
#include "common.h"
#include "metric_sample.h"
#include "numeric.h"

#pragma clang fp contract(off)

namespace {

inline bool fits32(long long rows, long long pitch) { return rows * pitch <= 0x7fffffffLL; }

struct NiqeWindow { double h[49]; };

constexpr int NQ_TW = 64, NQ_TH = 16;                 // the MSCN tile; its apron is 3 samples each way

// grid (tiles across, tiles down, frame).  T: unsigned char or unsigned short (a frame, read in place; the latter with its peak
// behind dst) or double (the half image).
template <typename T, typename... P>
__global__ __launch_bounds__(256) void niqe_mscn_kernel(const T* __restrict__ src, int pitch, long long fstride, int R, int C,
                                                        NiqeWindow win, double* __restrict__ dst, P... peak) {
  __shared__ double t[NQ_TH + 6][NQ_TW + 6];
  const int n = blockIdx.z, y0 = blockIdx.y * NQ_TH, x0 = blockIdx.x * NQ_TW;
  const T* p = src + (long long)n * fstride;
  for (int i = threadIdx.x; i < (NQ_TH + 6) * (NQ_TW + 6); i += 256) {
    const int r = i / (NQ_TW + 6), c = i - r * (NQ_TW + 6);
    int y = y0 + r - 3, x = x0 + c - 3;
    y = y < 0 ? 0 : y > R - 1 ? R - 1 : y;               // the edge of the REGION, not of the frame
    x = x < 0 ? 0 : x > C - 1 ? C - 1 : x;
    t[r][c] = metric_sample(p[y * pitch + x], peak...);
  }
  __syncthreads();
  double* out = dst + (long long)n * R * C;
  for (int i = threadIdx.x; i < NQ_TH * NQ_TW; i += 256) {
    const int r = i / NQ_TW, c = i - r * NQ_TW;
    if (y0 + r >= R || x0 + c >= C) continue;
    double mu = 0.0, sq = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int b = 0; b < 7; ++b) {
        const double v = t[r + a][c + b], h = win.h[a * 7 + b];
        mu = mu + h * v;
        sq = sq + h * (v * v);
      }
    const double sigma = sqrt(fabs(sq - mu * mu) + 0x1p-52);
    out[(y0 + r) * C + x0 + c] = (t[r + 3][c + 3] - mu) / (sigma + 1.0);
  }
}

constexpr int NQ_HT = 16;                               // the half image's tile, 16 x 16 outputs of 38 x 38 inputs

__device__ __forceinline__ int niqe_mirror(int i, int n) {   // [a,b,c] -> [c,b,a,a,b,c,c,b,a]; clamped beyond that (never read there)
  i = i < 0 ? -1 - i : i >= n ? 2 * n - 1 - i : i;
  return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}

// grid (tiles across, tiles down, frame) over the R/2 x C/2 outputs.  T, peak: as niqe_mscn_kernel's.
template <typename T, typename... P>
__global__ __launch_bounds__(256) void niqe_half_kernel(const T* __restrict__ src, int pitch, long long fstride, int R, int C,
                                                        double* __restrict__ dst, P... peak) {
  constexpr int IN = 2 * NQ_HT + 6;
  __shared__ double tin[IN][IN], mid[NQ_HT][IN];
  const double w[8] = {-3.0 / 256, -9.0 / 256, 29.0 / 256, 111.0 / 256, 111.0 / 256, 29.0 / 256, -9.0 / 256, -3.0 / 256};
  const int n = blockIdx.z, oy0 = blockIdx.y * NQ_HT, ox0 = blockIdx.x * NQ_HT;
  const T* p = src + (long long)n * fstride;
  for (int i = threadIdx.x; i < IN * IN; i += 256) {
    const int r = i / IN, c = i - r * IN;
    const int y = niqe_mirror(2 * oy0 - 3 + r, R), x = niqe_mirror(2 * ox0 - 3 + c, C);
    tin[r][c] = metric_sample(p[y * pitch + x], peak...) / 255.0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NQ_HT * IN; i += 256) {   // rows first: output row r of inputs 2r-3 .. 2r+4
    const int r = i / IN, c = i - r * IN;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = s + w[k] * tin[2 * r + k][c];
    mid[r][c] = s;
  }
  __syncthreads();
  const int r = threadIdx.x / NQ_HT, c = threadIdx.x - r * NQ_HT;
  const int Rh = R / 2, Ch = C / 2;
  if (oy0 + r < Rh && ox0 + c < Ch) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = s + w[k] * mid[r][2 * c + k];
    dst[(long long)n * Rh * Ch + (oy0 + r) * Ch + ox0 + c] = s * 255.0;
  }
}

// grid (block, frame); block b is (ih, iw) = (b % nh, b / nh), the order of the reference's blockproc.  sums [K][nb][5][6]: per map
// (count < 0, count > 0, sum v^2 over < 0, over > 0, sum |v|, sum v^2).  A thread's partials, the wave's butterfly, then the four
// waves in order through LDS: equal inputs give equal bits.  The block is read from memory, not staged: its five reads per sample
// hit L1 / L2, and 72 KiB of LDS would halve the workgroups a CU holds.
__global__ __launch_bounds__(256) void niqe_block_sums_kernel(const double* __restrict__ m, int R, int C, int B,
                                                              double* __restrict__ sums) {
  __shared__ double sh[4][30];
  const int n = blockIdx.y, nh = R / B, ih = blockIdx.x % nh, iw = blockIdx.x / nh;
  const double* p = m + (long long)n * R * C + (long long)ih * B * C + iw * B;
  double acc[30];
#pragma unroll
  for (int j = 0; j < 30; ++j) acc[j] = 0.0;
  for (int i = threadIdx.x; i < B * B; i += 256) {
    const int r = i / B, c = i - r * B;
    const int ru = r ? r - 1 : B - 1, cl = c ? c - 1 : B - 1, cr = c + 1 < B ? c + 1 : 0;      // circular inside the block
    const double x = p[r * C + c];
    const double v[5] = {x, x * p[r * C + cl], x * p[ru * C + c], x * p[ru * C + cl], x * p[ru * C + cr]};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double q = v[k] * v[k];
      const bool neg = v[k] < 0.0, pos = v[k] > 0.0;
      acc[6 * k + 0] += neg ? 1.0 : 0.0;
      acc[6 * k + 1] += pos ? 1.0 : 0.0;
      acc[6 * k + 2] += neg ? q : 0.0;
      acc[6 * k + 3] += pos ? q : 0.0;
      acc[6 * k + 4] += fabs(v[k]);
      acc[6 * k + 5] += q;
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
    sums[((long long)n * gridDim.x + blockIdx.x) * 30 + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// grid (block, frame), 320 threads: wave k searches the table for map k and its lane 0 writes the map's features into
// features[(n nb + b) * 36 + 18 scale ...].  table: gam [9801], then r_gam [9801].
__global__ __launch_bounds__(320) void niqe_features_kernel(const double* __restrict__ sums, double count, const double* __restrict__ table,
                                                            int scale, double* __restrict__ features) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  const double* s = sums + blk * 30 + 6 * k;
  const double ls = sqrt(s[2] / s[0]), rs = sqrt(s[3] / s[1]), g = ls / rs;
  const double ma = s[4] / count, rhat = ma * ma / (s[5] / count);
  const double g2 = g * g + 1.0, rn = rhat * (g * g * g + 1.0) * (g + 1.0) / (g2 * g2);
  double best = __builtin_inf();
  int at = 0x7fffffff;                                   // stays with a NaN rn (no distance compares below): index 0
  for (int i = lane; i < CDFO_NIQE_TABLE; i += 64) {
    const double d = fabs(table[CDFO_NIQE_TABLE + i] - rn);
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
  const double c = sqrt(exp(lgamma(1.0 / alpha) - lgamma(3.0 / alpha)));
  const double bl = ls * c, br = rs * c;
  double* f = features + blk * 36 + 18 * scale;
  if (k == 0) {
    f[0] = alpha;
    f[1] = (bl + br) / 2.0;
  } else {
    f += 4 * k - 2;
    f[0] = alpha;
    f[1] = (br - bl) * exp(lgamma(2.0 / alpha) - lgamma(1.0 / alpha));
    f[2] = bl;
    f[3] = br;
  }
}

// peak: empty, or the peak of 16-bit samples, checked by the entry point
template <typename T, typename... P>
int niqe_mscn(const T* src, int pitch, long long fstride, int K, int R, int C, const double* window, double* dst, void* stream, P... peak) {
  if (!src || !window || !dst || K <= 0 || K > 65535 || R <= 0 || C <= 0 || pitch < C || fstride < 0) return CDFO_EINVAL;
  if (!fits32(R, pitch) || !fits32(R, C) || cdiv(R, NQ_TH) > 65535) return CDFO_EINVAL;        // 32-bit offsets inside a frame
  if ((reinterpret_cast<uintptr_t>(dst) & 7u) || (reinterpret_cast<uintptr_t>(src) & (sizeof(T) - 1))) return CDFO_EALIGN;
  NiqeWindow win;
  for (int i = 0; i < 49; ++i) win.h[i] = window[i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 5.0 * 49 * K * (double)R * C, (sizeof(T) + 8.0) * K * (double)R * C);
  hipLaunchKernelGGL((niqe_mscn_kernel<T, P...>), dim3((unsigned)cdiv(C, NQ_TW), (unsigned)cdiv(R, NQ_TH), (unsigned)K), dim3(256), 0, st, src, pitch,
                     fstride, R, C, win, dst, peak...);
  CDFO_LAUNCH_CHECK();
  return 0;
}

template <typename T, typename... P>
int niqe_half(const T* src, int pitch, long long fstride, int K, int R, int C, double* dst, void* stream, P... peak) {
  if (!src || !dst || K <= 0 || K > 65535 || R < 8 || C < 8 || (R & 1) || (C & 1) || pitch < C || fstride < 0) return CDFO_EINVAL;
  if (!fits32(R, pitch) || cdiv(R / 2, NQ_HT) > 65535) return CDFO_EINVAL;                     // 32-bit offsets inside a frame
  if ((reinterpret_cast<uintptr_t>(dst) & 7u) || (reinterpret_cast<uintptr_t>(src) & (sizeof(T) - 1))) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 8 * K * 0.75 * R * C, K * (double)R * C * (2.0 + sizeof(T)));
  hipLaunchKernelGGL((niqe_half_kernel<T, P...>), dim3((unsigned)cdiv(C / 2, NQ_HT), (unsigned)cdiv(R / 2, NQ_HT), (unsigned)K), dim3(256), 0, st,
                     src, pitch, fstride, R, C, dst, peak...);
  CDFO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cdfo_niqe_mscn_u8(const unsigned char* src, int pitch, long long fstride, int K, int R, int C, const double* window,
                                 double* dst, void* stream) {
  return niqe_mscn<unsigned char>(src, pitch, fstride, K, R, C, window, dst, stream);
}

extern "C" int cdfo_niqe_mscn_f64(const double* src, int pitch, long long fstride, int K, int R, int C, const double* window,
                                  double* dst, void* stream) {
  return niqe_mscn<double>(src, pitch, fstride, K, R, C, window, dst, stream);
}

extern "C" int cdfo_niqe_mscn_u16(const unsigned short* src, int pitch, long long fstride, int K, int R, int C, const double* window,
                                  double* dst, int peak, void* stream) {
  if (peak < 1 || peak > 65535) return CDFO_EINVAL;
  return niqe_mscn<unsigned short>(src, pitch, fstride, K, R, C, window, dst, stream, (double)peak);
}

extern "C" int cdfo_niqe_half(const unsigned char* src, int pitch, long long fstride, int K, int R, int C, double* dst, void* stream) {
  return niqe_half<unsigned char>(src, pitch, fstride, K, R, C, dst, stream);
}

extern "C" int cdfo_niqe_half_u16(const unsigned short* src, int pitch, long long fstride, int K, int R, int C, double* dst, int peak,
                                  void* stream) {
  if (peak < 1 || peak > 65535) return CDFO_EINVAL;
  return niqe_half<unsigned short>(src, pitch, fstride, K, R, C, dst, stream, (double)peak);
}

extern "C" int cdfo_niqe_block_sums(const double* mscn, int K, int R, int C, int B, double* sums, void* stream) {
  if (!mscn || !sums || K <= 0 || K > 65535 || B < 2 || B > 96 || R < B || C < B || R % B || C % B) return CDFO_EINVAL;
  if (!fits32(R, C)) return CDFO_EINVAL;                                                        // 32-bit offsets inside a frame
  if ((reinterpret_cast<uintptr_t>(mscn) | reinterpret_cast<uintptr_t>(sums)) & 7u) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 40.0 * K * (double)R * C, 8.0 * K * (double)R * C);
  hipLaunchKernelGGL(niqe_block_sums_kernel, dim3((unsigned)((R / B) * (C / B)), (unsigned)K), dim3(256), 0, st, mscn, R, C, B, sums);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_niqe_features(const double* sums, int K, int nb, int count, const double* table, int scale, double* features,
                                  void* stream) {
  if (!sums || !table || !features || K <= 0 || K > 65535 || nb <= 0 || count <= 0 || (scale != 0 && scale != 1)) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(features)) & 7u)
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 5 * CDFO_NIQE_TABLE * (double)K * nb, 8.0 * 5 * CDFO_NIQE_TABLE * (double)K * nb);
  hipLaunchKernelGGL(niqe_features_kernel, dim3((unsigned)nb, (unsigned)K), dim3(320), 0, st, sums, (double)count, table, scale, features);
  CDFO_LAUNCH_CHECK();
  return 0;
}
