// The focal frequency loss on the device (cdfo_amd/loss.py: focal_frequency_loss; DESIGN.md "Focal frequency loss"): a 2-D FFT pair
// in HIP and the loss between them.  Per frame of H x W samples, H and W powers of two from CDFO_FFL_MIN to CDFO_FFL_MAX:
//     d = sr - hr (fp32)      F = fft2(d) / sqrt(H W)      D = Re(F)^2 + Im(F)^2      M = sqrt(D)^alpha
//     w = M / max M, NaN -> 0, clamped to [0, 1], a constant for the gradient        loss = sum(w D) / (H W)
//     d loss / d sr = 2 / (H W) Re(sum_k w F exp(+2 pi i ...)) / sqrt(H W)            (the transform is unitary)
//
//   cdfo_ffl_spectrum   two launches.  Rows: a workgroup forms d for R = min(H, 1024 / W) rows and transforms them along x in LDS.
//                       Columns: a workgroup takes a tile of CT = cdfo_ffl_tiles' width (16 columns, 8 at H = 512) by H through LDS,
//                       transposed so that a column is contiguous, transforms it, scales by 1 / sqrt(H W) in fp64 (one rounding),
//                       writes F in place and the tile's maximum of D (fp64) to pmax[n][tile].
//   cdfo_ffl_weight     two launches.  A workgroup per strip of 4096 bins takes the frame's maximum from pmax in index order, forms w
//                       in fp64, sums w D in fp64 (per thread in index order, then the wave's xor tree, then the four waves in order),
//                       and with `apply` overwrites F with w F (product in fp64, one rounding).  One thread per frame then adds the
//                       strips in index order and rounds loss[n] once.
//   cdfo_ffl_inverse    two launches: columns (unscaled, in place), then rows, whose real part times 2 / (H W)^(3/2) (fp64, one
//                       rounding) is g.  The imaginary part is dropped: w F keeps the Hermitian symmetry of a real frame's spectrum.
//
// The transform: radix 2, decimation in time, in place in LDS; a sequence enters in bit-reversed order (the index is reversed where
// the tile is written, __brev) and leaves in natural order.  Stage s pairs elements 2^s apart; butterfly j of a sequence takes the
// twiddle W_n^(pos 2^(log n - 1 - s)) from a table of cos / sin (2 pi k / n), k < n / 2, that the caller computed in fp64 and rounded
// once (kernels.ffl_twiddles); the table is copied to LDS first.  The inverse conjugates the table's sine.  A sequence sits at a pitch
// of n + 1 complex values: the columns pass writes and reads its tile transposed, 16 lanes a row of the tile, and the odd pitch
// spreads those over the banks.  No atomics; every grid is a function of (N, H, W) alone; equal inputs give equal bits.
#include "common.h"

namespace {

constexpr int FFL_THREADS = 256;
constexpr int FFL_ROW_ELEMS = 1024;                        // complex samples of a rows-pass workgroup
constexpr int FFL_STRIP = 4096;                            // bins of a weight-pass workgroup

inline bool ffl_size(int v) { return v >= CDFO_FFL_MIN && v <= CDFO_FFL_MAX && (v & (v - 1)) == 0; }
inline int ffl_col_tile(int H) { return H > 256 ? 8 : 16; }
inline int ffl_rows(int H, int W) { const int r = FFL_ROW_ELEMS / W; return r < H ? r : H; }
inline int ffl_strips(int H, int W) { const int s = H * W / FFL_STRIP; return s > 0 ? s : 1; }

// `seqs` sequences of 2^logn complex values each, sequence q at buf + q pitch, bit-reversed on entry, natural on return
template <bool INV>
__device__ __forceinline__ void fft_lds(float2* buf, int pitch, int seqs, int logn, const float2* tw) {
  const int lh = logn - 1, total = seqs << lh;
  for (int s = 0; s < logn; ++s) {
    const int half = 1 << s;
    for (int t = threadIdx.x; t < total; t += FFL_THREADS) {
      const int q = t >> lh, j = t & ((1 << lh) - 1), pos = j & (half - 1);
      float2* p = buf + q * pitch + (((j >> s) << (s + 1)) + pos);
      const float2 w = tw[pos << (lh - s)], a = p[0], b = p[half];
      const float si = INV ? w.y : -w.y;
      const float tr = b.x * w.x - b.y * si, ti = b.x * si + b.y * w.x;
      p[0] = make_float2(a.x + tr, a.y + ti);
      p[half] = make_float2(a.x - tr, a.y - ti);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// grid (H / R, N).  Forward: sr, hr -> F rows.  Inverse: F rows -> g = Re * gscale.
template <bool INV>
__global__ __launch_bounds__(FFL_THREADS) void ffl_rows_kernel(const float* __restrict__ sr, const float* __restrict__ hr,
                                                               float2* __restrict__ F, float* __restrict__ g, int H, int W, int logW,
                                                               int R, const float2* __restrict__ twg, double gscale) {
  extern __shared__ float2 ffl_lds[];
  float2* tw = ffl_lds;
  float2* buf = ffl_lds + W / 2;
  const int pitch = W + 1, elems = R * W;
  const size_t base = ((size_t)blockIdx.y * H + (size_t)blockIdx.x * R) * W;
  for (int k = threadIdx.x; k < W / 2; k += FFL_THREADS) tw[k] = twg[k];
  for (int e = threadIdx.x; e < elems; e += FFL_THREADS) {
    const int r = e >> logW, x = e & (W - 1);
    float2 v;
    if (INV) v = F[base + e];
    else v = make_float2(sr[base + e] - hr[base + e], 0.f);
    buf[r * pitch + bitrev(x, logW)] = v;
  }
  __syncthreads();
  fft_lds<INV>(buf, pitch, R, logW, tw);
  for (int e = threadIdx.x; e < elems; e += FFL_THREADS) {
    const float2 v = buf[(e >> logW) * pitch + (e & (W - 1))];
    if (INV) g[base + e] = (float)((double)v.x * gscale);
    else F[base + e] = v;
  }
}

// grid (W / CT, N), in place on F.  Forward: scaled, and the tile's maximum of D to pmax[n][tile].  Inverse: unscaled.
template <bool INV>
__global__ __launch_bounds__(FFL_THREADS) void ffl_cols_kernel(float2* __restrict__ F, int H, int W, int logH, int logCT,
                                                               const float2* __restrict__ twg, double scale, double* __restrict__ pmax) {
  extern __shared__ float2 ffl_lds[];
  __shared__ double shmax[FFL_THREADS / 64];
  float2* tw = ffl_lds;
  float2* buf = ffl_lds + H / 2;
  const int CT = 1 << logCT, pitch = H + 1, elems = H << logCT;
  float2* frame = F + (size_t)blockIdx.y * H * W + (size_t)blockIdx.x * CT;
  for (int k = threadIdx.x; k < H / 2; k += FFL_THREADS) tw[k] = twg[k];
  for (int e = threadIdx.x; e < elems; e += FFL_THREADS) {
    const int c = e & (CT - 1), y = e >> logCT;
    buf[c * pitch + bitrev(y, logH)] = frame[(size_t)y * W + c];
  }
  __syncthreads();
  fft_lds<INV>(buf, pitch, CT, logH, tw);
  double m = 0.0;
  for (int e = threadIdx.x; e < elems; e += FFL_THREADS) {
    const int c = e & (CT - 1), y = e >> logCT;
    float2 v = buf[c * pitch + y];
    if (!INV) {
      v = make_float2((float)((double)v.x * scale), (float)((double)v.y * scale));
      const double re = v.x, im = v.y;
      m = fmax(m, __fma_rn(re, re, im * im));              // both squares are exact in fp64: one rounding
    }
    frame[(size_t)y * W + c] = v;
  }
  if (!INV) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) shmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
      pmax[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = fmax(fmax(shmax[0], shmax[1]), fmax(shmax[2], shmax[3]));
  }
}

// grid (S, N): strip s of frame n is `bins` consecutive bins
__global__ __launch_bounds__(FFL_THREADS) void ffl_weight_kernel(float2* __restrict__ F, const double* __restrict__ pmax, int P, int hw,
                                                                 int bins, double alpha, int apply, double* __restrict__ partial) {
  __shared__ double sh[FFL_THREADS / 64];
  const double* pm = pmax + (size_t)blockIdx.y * P;
  double mx = pm[0];
  for (int p = 1; p < P; ++p) mx = fmax(mx, pm[p]);
  double top = sqrt(mx);
  if (alpha != 1.0) top = pow(top, alpha);
  float2* f = F + (size_t)blockIdx.y * hw + (size_t)blockIdx.x * bins;
  double acc = 0.0;
  for (int i = threadIdx.x; i < bins; i += FFL_THREADS) {
    const float2 v = f[i];
    const double re = v.x, im = v.y, D = __fma_rn(re, re, im * im);
    double M = sqrt(D);
    if (alpha != 1.0) M = pow(M, alpha);
    double w = M / top;
    if (w != w) w = 0.0;
    w = fmin(fmax(w, 0.0), 1.0);
    acc += w * D;
    if (apply) f[i] = make_float2((float)(w * re), (float)(w * im));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one thread per frame: the strips in index order, one rounding
__global__ __launch_bounds__(64) void ffl_fold_kernel(const double* __restrict__ partial, int N, int S, double inv_hw, float* __restrict__ loss) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += partial[(size_t)n * S + s];
  loss[n] = (float)(acc * inv_hw);
}

inline int ilog2(int v) { return __builtin_ctz((unsigned)v); }
inline bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

}  // namespace

extern "C" int cdfo_ffl_tiles(int H, int W) {
  if (!ffl_size(H) || !ffl_size(W)) return CDFO_EINVAL;
  const int ct = ffl_col_tile(H);
  return W / ct;
}

extern "C" int cdfo_ffl_strips(int H, int W) {
  if (!ffl_size(H) || !ffl_size(W)) return CDFO_EINVAL;
  return ffl_strips(H, W);
}

extern "C" int cdfo_ffl_spectrum(const float* sr, const float* hr, int N, int H, int W, const float* tw_h, const float* tw_w, float* F,
                                 double* pmax, int pmax_cap, void* stream) {
  if (!sr || !hr || !tw_h || !tw_w || !F || !pmax || N <= 0 || N > 65535 || !ffl_size(H) || !ffl_size(W)) return CDFO_EINVAL;
  const int ct = ffl_col_tile(H), P = W / ct;
  if ((long long)pmax_cap < (long long)N * P) return CDFO_EINVAL;
  if (misaligned(sr, 3u) || misaligned(hr, 3u) || misaligned(tw_h, 7u) || misaligned(tw_w, 7u) || misaligned(F, 7u) || misaligned(pmax, 7u))
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int R = ffl_rows(H, W);
  float2* Fc = reinterpret_cast<float2*>(F);
  hipLaunchKernelGGL(ffl_rows_kernel<false>, dim3(H / R, N), dim3(FFL_THREADS), (size_t)(W / 2 + R * (W + 1)) * sizeof(float2), st, sr, hr,
                     Fc, static_cast<float*>(nullptr), H, W, ilog2(W), R, reinterpret_cast<const float2*>(tw_w), 0.0);
  CDFO_LAUNCH_CHECK();
  hipLaunchKernelGGL(ffl_cols_kernel<false>, dim3(P, N), dim3(FFL_THREADS), (size_t)(H / 2 + ct * (H + 1)) * sizeof(float2), st, Fc, H, W,
                     ilog2(H), ilog2(ct), reinterpret_cast<const float2*>(tw_h), 1.0 / sqrt((double)H * (double)W), pmax);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ffl_weight(float* F, const double* pmax, int P, int N, int H, int W, float alpha, int apply, double* partial,
                               int partial_cap, float* loss, void* stream) {
  if (!F || !pmax || !partial || !loss || P <= 0 || N <= 0 || N > 65535 || !ffl_size(H) || !ffl_size(W) || !(alpha >= 0.f) ||
      !(alpha <= 3.402823466e38f))
    return CDFO_EINVAL;
  const int S = ffl_strips(H, W);
  if ((long long)partial_cap < (long long)N * S) return CDFO_EINVAL;
  if (misaligned(F, 7u) || misaligned(pmax, 7u) || misaligned(partial, 7u) || misaligned(loss, 3u)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int hw = H * W;
  hipLaunchKernelGGL(ffl_weight_kernel, dim3(S, N), dim3(FFL_THREADS), 0, st, reinterpret_cast<float2*>(F), pmax, P, hw, hw / S,
                     (double)alpha, apply ? 1 : 0, partial);
  CDFO_LAUNCH_CHECK();
  hipLaunchKernelGGL(ffl_fold_kernel, dim3((N + 63) / 64), dim3(64), 0, st, partial, N, S, 1.0 / (double)hw, loss);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_ffl_inverse(float* F, int N, int H, int W, const float* tw_h, const float* tw_w, float* g, void* stream) {
  if (!F || !tw_h || !tw_w || !g || N <= 0 || N > 65535 || !ffl_size(H) || !ffl_size(W)) return CDFO_EINVAL;
  if (misaligned(F, 7u) || misaligned(tw_h, 7u) || misaligned(tw_w, 7u) || misaligned(g, 3u)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int ct = ffl_col_tile(H), R = ffl_rows(H, W);
  const double hw = (double)H * (double)W;
  float2* Fc = reinterpret_cast<float2*>(F);
  hipLaunchKernelGGL(ffl_cols_kernel<true>, dim3(W / ct, N), dim3(FFL_THREADS), (size_t)(H / 2 + ct * (H + 1)) * sizeof(float2), st, Fc, H, W,
                     ilog2(H), ilog2(ct), reinterpret_cast<const float2*>(tw_h), 1.0, static_cast<double*>(nullptr));
  CDFO_LAUNCH_CHECK();
  hipLaunchKernelGGL(ffl_rows_kernel<true>, dim3(H / R, N), dim3(FFL_THREADS), (size_t)(W / 2 + R * (W + 1)) * sizeof(float2), st,
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr), Fc, g, H, W, ilog2(W), R,
                     reinterpret_cast<const float2*>(tw_w), 2.0 / (hw * sqrt(hw)));
  CDFO_LAUNCH_CHECK();
  return 0;
}
