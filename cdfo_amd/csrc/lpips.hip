// LPIPS' own kernels: what a VGG-shaped trunk needs beside the 3x3 convolutions of conv_igemm.hip, and the distance of two feature
// stacks (DESIGN.md has the definition, tests/lpips_ref.py its torch statement; cdfo_amd/metrics.py: lpips_layers_u8 puts a chunk's
// launches together).
//   cdfo_lpips_stem_u8   8-bit luma read in place -> ReLU(conv1_1) as NHWC fp32: the scaling to three channels, the zero padding of
//                        the SCALED tensor and the 27-tap convolution in one pass, halo tile and weights through LDS
//   cdfo_lpips_stem_u16  the same of 16-bit luma of a peak of 1 .. 65535: v / peak where the 8-bit form has v / 255
//   cdfo_lpips_stem_f32  the same of fp32 samples used as they are (the training loss, cdfo_amd/loss.py: lpips_loss)
//   cdfo_lpips_pool2     NHWC fp32 2 x 2 / 2 maximum with floor, 16 bytes per lane, bit-exact
//   cdfo_lpips_dist      two NHWC fp32 stacks and lin [C] -> fp64 partial sums per (frame, strip of rows): lanes over a pixel's
//                        channels, the two norms and the weighted squared differences reduced by a butterfly of fixed order
//   cdfo_lpips_fold      the strips of every layer added in index order and divided by the layer's pixel count, one launch
// The adjoint of the above for the training loss (gradient to the result's samples only, the weights are frozen):
//   cdfo_lpips_dist_bwd  the gradient of a frame's layer distance with respect to the result's tap, plus the gradient that arrives from
//                        the deeper stage, through the tap's ReLU (a select): the forward's lanes and butterflies
//   cdfo_lpips_pool2_bwd the pooled gradient to the element ATen's kernel picks, +0 elsewhere and in the floored row and column
//   cdfo_lpips_stem_bwd  the adjoint of the scaling and conv1_1 folded to one 3 x 3 C0 -> 1 convolution, halo tile through LDS
// The trunk is fp32 up to and including the ReLU outputs; everything behind the features is fp64.  Grids and summation orders
// depend on the shapes alone and nothing is atomic: equal inputs give equal bits, d(a, a) is exactly 0 and d(a, b) has the bits of
// d(b, a) (both norms are formed the same way and (x - y)^2 = (y - x)^2 exactly).  All stores are vector stores.
#include "common.h"
#include "metric_sample.h"

namespace {

inline bool fits32(long long rows, long long pitch) { return rows * pitch <= 0x7fffffffLL; }

constexpr int LP_T = 16;                                // the stem's tile, 16 x 16 pixels of an 18 x 18 halo
constexpr int LP_HALO = LP_T + 2;

// grid (tiles across, tiles down, frame), dynamic LDS: 3 halo planes, 27 C0 weights as [tap][channel], C0 biases.
// A sample v becomes x = v / 255 (normalize: 2 x - 1), then channel c = (x - shift_c) / scale_c; beyond the region the SCALED tensor
// is zero.  Item i of a tile is (pixel i / (C0 / 4), channel quad i % (C0 / 4)): neighbouring lanes hold neighbouring quads of one
// pixel, so a wave's stores are contiguous runs of a pixel's channels and its halo reads are broadcasts.
// T: unsigned char, or unsigned short with the samples' peak behind dst: x = v / peak, or float: x = v (metric_sample.h).
template <typename T, typename... P>
__global__ __launch_bounds__(256) void lpips_stem_kernel(const T* __restrict__ src, int pitch, long long fstride, int h, int w,
                                                         const float* __restrict__ weight, const float* __restrict__ bias, int C0,
                                                         int normalize, float* __restrict__ dst, P... peak) {
  extern __shared__ __attribute__((aligned(16))) float lp_smem[];
  float* sIn = lp_smem;                                 // [3][LP_HALO][LP_HALO], padded to a multiple of 4 floats
  float* sW = lp_smem + 3 * LP_HALO * LP_HALO;          // [27][C0]  (3 * 18 * 18 = 972 floats: 16-byte aligned)
  float* sB = sW + 27 * C0;
  const int n = blockIdx.z, y0 = blockIdx.y * LP_T, x0 = blockIdx.x * LP_T;
  const T* p = src + (long long)n * fstride;
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
  for (int i = threadIdx.x; i < LP_HALO * LP_HALO; i += 256) {
    const int r = i / LP_HALO, c = i - r * LP_HALO;
    const int y = y0 + r - 1, x = x0 + c - 1;
    const bool inside = y >= 0 && y < h && x >= 0 && x < w;
    float v = inside ? unit_sample(p[y * pitch + x], peak...) : 0.f;
    if (normalize) v = 2.f * v - 1.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) sIn[ch * LP_HALO * LP_HALO + i] = inside ? (v - shift[ch]) / scale[ch] : 0.f;
  }
  for (int i = threadIdx.x; i < 27 * C0; i += 256) {    // OIHW [C0][3][3][3] -> [tap = ci * 9 + ky * 3 + kx][C0]
    const int t = i / C0, co = i - t * C0;
    sW[i] = weight[co * 27 + t];
  }
  for (int i = threadIdx.x; i < C0; i += 256) sB[i] = bias[i];
  __syncthreads();
  const int CQ = C0 >> 2;
  float* out = dst + (long long)n * h * w * C0;
  for (int i = threadIdx.x; i < LP_T * LP_T * CQ; i += 256) {
    const int px = i / CQ, q = i - px * CQ;
    const int r = px / LP_T, c = px - r * LP_T;
    if (y0 + r >= h || x0 + c >= w) continue;
    f32x4 acc = *reinterpret_cast<const f32x4*>(sB + 4 * q);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float v = sIn[ch * LP_HALO * LP_HALO + (r + ky) * LP_HALO + c + kx];
          acc += v * *reinterpret_cast<const f32x4*>(sW + (ch * 9 + ky * 3 + kx) * C0 + 4 * q);
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] > 0.f ? acc[e] : 0.f;
    *reinterpret_cast<f32x4*>(out + ((long long)(y0 + r) * w + x0 + c) * C0 + 4 * q) = acc;
  }
}

// ATen's rule, in its order: a later sample replaces the maximum if it is larger or a NaN
__device__ __forceinline__ f32x4 lpips_max4(f32x4 m, f32x4 v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];
  return m;
}

// one thread per output channel quad: total = N * (H / 2) * (W / 2) * (C / 4)
__global__ __launch_bounds__(256) void lpips_pool2_kernel(const float* __restrict__ src, int H, int W, int C, long long total,
                                                          float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int CQ = C >> 2, Ho = H >> 1, Wo = W >> 1;
  const int q = (int)(i % CQ);
  long long rest = i / CQ;
  const int x = (int)(rest % Wo);
  rest /= Wo;
  const int y = (int)(rest % Ho);
  const long long n = rest / Ho;
  const float* p = src + (((n * H + 2 * y) * W + 2 * x) * (long long)C) + 4 * q;
  f32x4 m = *reinterpret_cast<const f32x4*>(p);
  m = lpips_max4(m, *reinterpret_cast<const f32x4*>(p + C));
  m = lpips_max4(m, *reinterpret_cast<const f32x4*>(p + (long long)W * C));
  m = lpips_max4(m, *reinterpret_cast<const f32x4*>(p + (long long)W * C + C));
  *reinterpret_cast<f32x4*>(dst + 4 * i) = m;
}

// grid (strip, frame), LP_DT threads: sixteen waves per strip keep enough loads in flight for a kernel that only streams.  L lanes
// (a power of two, 4 .. 64, at least C / 4 below 64) share a pixel: lane s of a group takes the channel quads s, s + L, ...; a
// workgroup holds LP_DT / L pixels at a time, group j the strip's pixels j, j + LP_DT / L, ...  A lane keeps its first LP_KEEP quads
// of both stacks in registers between the two passes (all of them up to C = 512), and reads any beyond again.
// Per pixel: the two sums of squares (each lane its quads in order, then the group's butterfly, after which every lane of the group
// holds the same bits), the roots, then the weighted squared differences the same way.  Lane 0 of a group adds its pixels' values
// in order; thread 0 adds the groups in index order.
constexpr int LP_DT = 1024, LP_KEEP = 2;

__global__ __launch_bounds__(LP_DT) void lpips_dist_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                         const double* __restrict__ lin, int h, int w, int C, int L,
                                                         double* __restrict__ partials) {
  __shared__ double sh[LP_DT / 4];
  const int n = blockIdx.y, r0 = blockIdx.x * CDFO_LPIPS_STRIP;
  const int rows = h - r0 < CDFO_LPIPS_STRIP ? h - r0 : CDFO_LPIPS_STRIP;
  const int CQ = C >> 2, groups = LP_DT / L, grp = threadIdx.x / L, s = threadIdx.x - grp * L;
  const long long base = ((long long)n * h + r0) * w * C;
  const float* pa = fa + base;
  const float* pb = fb + base;
  double acc = 0.0;
  for (int px = grp; px < rows * w; px += groups) {     // the lanes of a group leave together: the butterflies stay inside a group
    const float* a = pa + (long long)px * C;
    const float* b = pb + (long long)px * C;
    double na = 0.0, nb = 0.0;
    f32x4 ka[LP_KEEP], kb[LP_KEEP];
#pragma unroll
    for (int j = 0; j < LP_KEEP; ++j)
      if (s + j * L < CQ) {
        ka[j] = *reinterpret_cast<const f32x4*>(a + 4 * (s + j * L));
        kb[j] = *reinterpret_cast<const f32x4*>(b + 4 * (s + j * L));
      }
#pragma unroll
    for (int j = 0; j < LP_KEEP; ++j)
      if (s + j * L < CQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          na += (double)ka[j][e] * (double)ka[j][e];
          nb += (double)kb[j][e] * (double)kb[j][e];
        }
      }
    for (int q = s + LP_KEEP * L; q < CQ; q += L) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(a + 4 * q), vb = *reinterpret_cast<const f32x4*>(b + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        na += (double)va[e] * (double)va[e];
        nb += (double)vb[e] * (double)vb[e];
      }
    }
    for (int o = L >> 1; o > 0; o >>= 1) {
      na += __shfl_xor(na, o, 64);
      nb += __shfl_xor(nb, o, 64);
    }
    const double da = sqrt(na) + 1e-10, db = sqrt(nb) + 1e-10;
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < LP_KEEP; ++j)
      if (s + j * L < CQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double t = (double)ka[j][e] / da - (double)kb[j][e] / db;
          d += lin[4 * (s + j * L) + e] * (t * t);
        }
      }
    for (int q = s + LP_KEEP * L; q < CQ; q += L) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(a + 4 * q), vb = *reinterpret_cast<const f32x4*>(b + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double t = (double)va[e] / da - (double)vb[e] / db;
        d += lin[4 * q + e] * (t * t);
      }
    }
    for (int o = L >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    acc += d;
  }
  if (s == 0) sh[grp] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int j = 0; j < groups; ++j) t += sh[j];
    partials[(long long)n * gridDim.x + blockIdx.x] = t;
  }
}

struct LpipsFold {
  int strips[CDFO_LPIPS_MAX_LAYERS];
  long long first[CDFO_LPIPS_MAX_LAYERS];               // where layer k's [N][strips[k]] block begins
  double count[CDFO_LPIPS_MAX_LAYERS];
};

// one thread per (frame, layer)
__global__ __launch_bounds__(64) void lpips_fold_kernel(const double* __restrict__ partials, int N, int layers, LpipsFold f,
                                                        double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= N * layers) return;
  const int n = i / layers, k = i - n * layers;
  const double* p = partials + f.first[k] + (long long)n * f.strips[k];
  double t = 0.0;
  for (int g = 0; g < f.strips[k]; ++g) t += p[g];
  out[i] = t / f.count[k];
}

// ---- the adjoint ----
// grid (groups of pixels, frame), LP_BT threads.  L lanes share a pixel exactly as in lpips_dist_kernel (lane s the channel quads s,
// s + L, ..., the first LP_KEEP of both stacks kept in registers); a workgroup holds LP_BT / L pixels, one per group.  Per pixel, in
// fp64: na = sum A^2, nb = sum B^2 (each lane its quads in order, then the group's butterfly), r = 1 / (sqrt(na) + 1e-10),
// u_c = A_c / (sqrt(na) + 1e-10) - B_c / (sqrt(nb) + 1e-10) -- the forward's two quotients, not products with reciprocals, which
// the compiler may contract into one fused operation that leaves a rounding residue where A equals B: equal stacks give u = 0, and
// with it an all-zero gradient, exactly -- q = sum lin_c u_c A_c (the same way), and
//   t_c = gscale / (h w) * 2 r * (lin_c u_c - (r q / sqrt(na)) A_c),   gout_c = A_c > 0 ? (float)(t_c + gin_c) : +0.
// The select drops whatever arrives under a ReLU output that is not positive: the 0 / 0 of a pixel whose tap is all zero included.
constexpr int LP_BT = 256;

__global__ __launch_bounds__(LP_BT) void lpips_dist_bwd_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                               const double* __restrict__ lin, const float* __restrict__ gscale,
                                                               const float* __restrict__ gin, int hw, int C, int L,
                                                               float* __restrict__ gout) {
  const int n = blockIdx.y, grp = threadIdx.x / L, s = threadIdx.x - grp * L, CQ = C >> 2;
  const long long px = (long long)blockIdx.x * (LP_BT / L) + grp;
  if (px >= hw) return;                                 // the lanes of a group leave together: the butterflies stay inside a group
  const long long base = ((long long)n * hw + px) * C;
  const float* a = fa + base;
  const float* b = fb + base;
  f32x4 ka[LP_KEEP], kb[LP_KEEP];
#pragma unroll
  for (int j = 0; j < LP_KEEP; ++j)
    if (s + j * L < CQ) {
      ka[j] = *reinterpret_cast<const f32x4*>(a + 4 * (s + j * L));
      kb[j] = *reinterpret_cast<const f32x4*>(b + 4 * (s + j * L));
    }
  auto quads = [&](auto&& f) {                          // f(quad, A, B) for each of this lane's quads, in order
#pragma unroll
    for (int j = 0; j < LP_KEEP; ++j)
      if (s + j * L < CQ) f(s + j * L, ka[j], kb[j]);
    for (int q = s + LP_KEEP * L; q < CQ; q += L)
      f(q, *reinterpret_cast<const f32x4*>(a + 4 * q), *reinterpret_cast<const f32x4*>(b + 4 * q));
  };
  double na = 0.0, nb = 0.0;
  quads([&](int, const f32x4 va, const f32x4 vb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      na += (double)va[e] * (double)va[e];
      nb += (double)vb[e] * (double)vb[e];
    }
  });
  for (int o = L >> 1; o > 0; o >>= 1) {
    na += __shfl_xor(na, o, 64);
    nb += __shfl_xor(nb, o, 64);
  }
  const double sa = sqrt(na), da = sa + 1e-10, db = sqrt(nb) + 1e-10, r = 1.0 / da;
  double q = 0.0;
  quads([&](int c4, const f32x4 va, const f32x4 vb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double u = (double)va[e] / da - (double)vb[e] / db;
      q += lin[4 * c4 + e] * u * (double)va[e];
    }
  });
  for (int o = L >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const double k1 = (double)gscale[n] / (double)hw * 2.0 * r, k2 = r * q / sa;
  quads([&](int c4, const f32x4 va, const f32x4 vb) {
    f32x4 gi = {0.f, 0.f, 0.f, 0.f}, out;
    if (gin) gi = *reinterpret_cast<const f32x4*>(gin + base + 4 * c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double u = (double)va[e] / da - (double)vb[e] / db;
      const double t = k1 * (lin[4 * c4 + e] * u - k2 * (double)va[e]);
      out[e] = va[e] > 0.f ? (float)(t + (double)gi[e]) : 0.f;
    }
    *reinterpret_cast<f32x4*>(gout + base + 4 * c4) = out;
  });
}

// one thread per channel quad of a 2 x 2 cell of gx, the cells of the floored row and column included:
// total = N * ceil(H / 2) * ceil(W / 2) * (C / 4).  A whole cell routes its pooled gradient to the element lpips_max4 took (ATen's
// order (0,0), (0,1), (1,0), (1,1): a later sample replaces the maximum if it is larger or a NaN); every other element is +0.
__global__ __launch_bounds__(256) void lpips_pool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int H, int W, int C,
                                                              long long total, float* __restrict__ gx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int CQ = C >> 2, Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
  const int q = (int)(i % CQ);
  long long rest = i / CQ;
  const int xo = (int)(rest % Wc);
  rest /= Wc;
  const int yo = (int)(rest % Hc);
  const long long n = rest / Hc;
  const long long at = (((n * H + 2 * yo) * W + 2 * xo) * (long long)C) + 4 * q, down = (long long)W * C;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (yo >= Ho || xo >= Wo) {                           // a cell the floor drops: what of it lies inside is +0
    *reinterpret_cast<f32x4*>(gx + at) = zero;
    if (2 * xo + 1 < W) *reinterpret_cast<f32x4*>(gx + at + C) = zero;
    if (2 * yo + 1 < H) *reinterpret_cast<f32x4*>(gx + at + down) = zero;
    return;
  }
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + at), v1 = *reinterpret_cast<const f32x4*>(x + at + C);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(x + at + down), v3 = *reinterpret_cast<const f32x4*>(x + at + down + C);
  const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (((n * Ho + yo) * Wo + xo) * (long long)C) + 4 * q);
  f32x4 o0, o1, o2, o3;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float m = v0[e];
    int k = 0;
    if (v1[e] > m || v1[e] != v1[e]) { m = v1[e]; k = 1; }
    if (v2[e] > m || v2[e] != v2[e]) { m = v2[e]; k = 2; }
    if (v3[e] > m || v3[e] != v3[e]) { m = v3[e]; k = 3; }
    o0[e] = k == 0 ? gv[e] : 0.f;
    o1[e] = k == 1 ? gv[e] : 0.f;
    o2[e] = k == 2 ? gv[e] : 0.f;
    o3[e] = k == 3 ? gv[e] : 0.f;
  }
  *reinterpret_cast<f32x4*>(gx + at) = o0;
  *reinterpret_cast<f32x4*>(gx + at + C) = o1;
  *reinterpret_cast<f32x4*>(gx + at + down) = o2;
  *reinterpret_cast<f32x4*>(gx + at + down + C) = o3;
}

// grid (tiles across, tiles down, frame), 256 threads, one per pixel of a 16 x 16 tile; dynamic LDS: a halo tile of LP_BC channels of
// g as [18 * 18][LP_BP] (a pixel's 16 channels padded to 20 floats: the 16 lanes of a 16-byte LDS read then hit different banks) and
// wf as [tap][C0].  The padding of the scaled tensor is constant, so the adjoint of the scaling and of conv1_1 is
//   gx[y][x] = sum_o sum_ky sum_kx wf[o][ky][kx] g[y + 1 - ky][x + 1 - kx][o],   g zero outside,
// taken LP_BC channels at a time in the order (chunk, ky, kx) into four fp32 sums per pixel, added as (s0 + s1) + (s2 + s3).
constexpr int LP_BC = 16, LP_BP = 20;

__global__ __launch_bounds__(256) void lpips_stem_bwd_kernel(const float* __restrict__ g, const float* __restrict__ wf, int h, int w, int C0,
                                                             float* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) float lp_smem[];
  float* sG = lp_smem;                                  // [LP_HALO * LP_HALO][LP_BP]
  float* sW = lp_smem + LP_HALO * LP_HALO * LP_BP;      // [9][C0]
  const int n = blockIdx.z, y0 = blockIdx.y * LP_T, x0 = blockIdx.x * LP_T;
  const int r = threadIdx.x / LP_T, c = threadIdx.x - r * LP_T;
  for (int i = threadIdx.x; i < 9 * C0; i += 256) {     // [C0][3][3] -> [tap][C0]
    const int t = i / C0, o = i - t * C0;
    sW[i] = wf[o * 9 + t];
  }
  const float* src = g + (long long)n * h * w * C0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < C0; c0 += LP_BC) {
    __syncthreads();                                    // the chunk before is read (the first time: nothing to wait for)
    for (int i = threadIdx.x; i < LP_HALO * LP_HALO * (LP_BC / 4); i += 256) {
      const int p = i / (LP_BC / 4), qd = i - p * (LP_BC / 4);
      const int rr = p / LP_HALO, cc = p - rr * LP_HALO;
      const int y = y0 + rr - 1, x = x0 + cc - 1;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (y >= 0 && y < h && x >= 0 && x < w) v = *reinterpret_cast<const f32x4*>(src + ((long long)y * w + x) * C0 + c0 + 4 * qd);
      *reinterpret_cast<f32x4*>(sG + p * LP_BP + 4 * qd) = v;
    }
    __syncthreads();
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float* pg = sG + ((r + 2 - ky) * LP_HALO + c + 2 - kx) * LP_BP;
        const float* pw = sW + (ky * 3 + kx) * C0 + c0;
#pragma unroll
        for (int qd = 0; qd < LP_BC / 4; ++qd)
          acc += *reinterpret_cast<const f32x4*>(pg + 4 * qd) * *reinterpret_cast<const f32x4*>(pw + 4 * qd);
      }
  }
  if (y0 + r < h && x0 + c < w) gx[((long long)n * h + y0 + r) * w + x0 + c] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// peak: empty, or the peak of 16-bit samples, checked by the entry point
template <typename T, typename... P>
int lpips_stem(const T* src, int pitch, long long fstride, int N, int h, int w, const float* weight, const float* bias, int C0, int normalize,
               float* dst, void* stream, P... peak) {
  if (!src || !weight || !bias || !dst || N <= 0 || N > 65535 || h <= 0 || w <= 0 || pitch < w || fstride < 0) return CDFO_EINVAL;
  if (C0 <= 0 || C0 % 16 || C0 > CDFO_LPIPS_STEM_MAXC) return CDFO_EINVAL;
  if (!fits32(h, pitch) || cdiv(h, LP_T) > 65535) return CDFO_EINVAL;                          // 32-bit offsets inside a frame
  if (!aligned16(dst) || (reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) & 3u) return CDFO_EALIGN;
  if (reinterpret_cast<uintptr_t>(src) & (sizeof(T) - 1)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double px = (double)N * h * w;
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 27 * C0 * px, (sizeof(T) + 4.0 * C0) * px);
  const int lds = (3 * LP_HALO * LP_HALO + 28 * C0) * (int)sizeof(float);
  hipLaunchKernelGGL((lpips_stem_kernel<T, P...>), dim3((unsigned)cdiv(w, LP_T), (unsigned)cdiv(h, LP_T), (unsigned)N), dim3(256), lds, st, src,
                     pitch, fstride, h, w, weight, bias, C0, normalize ? 1 : 0, dst, peak...);
  CDFO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cdfo_lpips_stem_u8(const unsigned char* src, int pitch, long long fstride, int N, int h, int w, const float* weight,
                                  const float* bias, int C0, int normalize, float* dst, void* stream) {
  return lpips_stem<unsigned char>(src, pitch, fstride, N, h, w, weight, bias, C0, normalize, dst, stream);
}

extern "C" int cdfo_lpips_stem_u16(const unsigned short* src, int pitch, long long fstride, int N, int h, int w, const float* weight,
                                   const float* bias, int C0, int normalize, float* dst, int peak, void* stream) {
  if (peak < 1 || peak > 65535) return CDFO_EINVAL;
  return lpips_stem<unsigned short>(src, pitch, fstride, N, h, w, weight, bias, C0, normalize, dst, stream, (float)peak);
}

extern "C" int cdfo_lpips_stem_f32(const float* src, int pitch, long long fstride, int N, int h, int w, const float* weight,
                                   const float* bias, int C0, int normalize, float* dst, void* stream) {
  return lpips_stem<float>(src, pitch, fstride, N, h, w, weight, bias, C0, normalize, dst, stream);
}

extern "C" int cdfo_lpips_pool2(const float* src, int N, int H, int W, int C, float* dst, void* stream) {
  if (!src || !dst || N <= 0 || H < 2 || W < 2 || C <= 0 || C % 4) return CDFO_EINVAL;
  if (!aligned16(src) || !aligned16(dst)) return CDFO_EALIGN;
  const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return CDFO_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 12.0 * total, 80.0 * total);
  hipLaunchKernelGGL(lpips_pool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, H, W, C, total, dst);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_lpips_dist(const float* fa, const float* fb, const double* lin, int N, int h, int w, int C, double* partials,
                               void* stream) {
  if (!fa || !fb || !lin || !partials || N <= 0 || N > 65535 || h <= 0 || w <= 0 || C <= 0 || C % 4) return CDFO_EINVAL;
  if (!fits32(CDFO_LPIPS_STRIP, w)) return CDFO_EINVAL;                                         // a strip's pixel index is an int
  if (!aligned16(fa) || !aligned16(fb) || (reinterpret_cast<uintptr_t>(lin) | reinterpret_cast<uintptr_t>(partials)) & 7u)
    return CDFO_EALIGN;
  int L = 4;
  while (L < C / 4 && L < 64) L *= 2;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double el = (double)N * h * w * C;
  CdfoProfScope prof(st, KID_LAYOUT, 12.0 * el, 8.0 * el);
  hipLaunchKernelGGL(lpips_dist_kernel, dim3((unsigned)cdiv(h, CDFO_LPIPS_STRIP), (unsigned)N), dim3(LP_DT), 0, st, fa, fb, lin, h, w, C, L,
                     partials);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_lpips_fold(const double* partials, int N, int layers, const int* strips, const long long* counts, double* out,
                               void* stream) {
  if (!partials || !strips || !counts || !out || N <= 0 || layers <= 0 || layers > CDFO_LPIPS_MAX_LAYERS) return CDFO_EINVAL;
  if ((long long)N * layers > 0x7fffffffLL) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(out)) & 7u) return CDFO_EALIGN;
  LpipsFold f;
  long long at = 0;
  for (int k = 0; k < layers; ++k) {
    if (strips[k] <= 0 || counts[k] <= 0) return CDFO_EINVAL;
    f.strips[k] = strips[k];
    f.first[k] = at;
    f.count[k] = (double)counts[k];
    at += (long long)N * strips[k];
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, (double)at, 8.0 * at);
  hipLaunchKernelGGL(lpips_fold_kernel, dim3((unsigned)cdiv(N * layers, 64)), dim3(64), 0, st, partials, N, layers, f, out);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_lpips_dist_bwd(const float* fa, const float* fb, const double* lin, const float* gscale, const float* gin, int N, int h,
                                   int w, int C, float* gout, void* stream) {
  if (!fa || !fb || !lin || !gscale || !gout || N <= 0 || N > 65535 || h <= 0 || w <= 0 || C <= 0 || C % 16) return CDFO_EINVAL;
  if (!fits32(h, w)) return CDFO_EINVAL;                                                        // a frame's pixel count is an int
  if (!aligned16(fa) || !aligned16(fb) || !aligned16(gout) || (gin && !aligned16(gin)) || reinterpret_cast<uintptr_t>(lin) & 7u ||
      reinterpret_cast<uintptr_t>(gscale) & 3u)
    return CDFO_EALIGN;
  int L = 4;
  while (L < C / 4 && L < 64) L *= 2;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double el = (double)N * h * w * C;
  CdfoProfScope prof(st, KID_LAYOUT, 16.0 * el, (gin ? 16.0 : 12.0) * el);
  hipLaunchKernelGGL(lpips_dist_bwd_kernel, dim3((unsigned)cdiv(h * w, LP_BT / L), (unsigned)N), dim3(LP_BT), 0, st, fa, fb, lin, gscale, gin,
                     h * w, C, L, gout);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_lpips_pool2_bwd(const float* x, const float* g, int N, int H, int W, int C, float* gx, void* stream) {
  if (!x || !g || !gx || N <= 0 || H < 2 || W < 2 || C <= 0 || C % 4) return CDFO_EINVAL;
  if (!aligned16(x) || !aligned16(g) || !aligned16(gx)) return CDFO_EALIGN;
  const long long total = (long long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return CDFO_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 12.0 * total, 144.0 * total);
  hipLaunchKernelGGL(lpips_pool2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, g, H, W, C, total, gx);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_lpips_stem_bwd(const float* g, const float* wf, int N, int h, int w, int C0, float* gx, void* stream) {
  if (!g || !wf || !gx || N <= 0 || N > 65535 || h <= 0 || w <= 0) return CDFO_EINVAL;
  if (C0 <= 0 || C0 % 16 || C0 > CDFO_LPIPS_STEM_MAXC) return CDFO_EINVAL;
  if (!fits32(h, w) || cdiv(h, LP_T) > 65535) return CDFO_EINVAL;
  if (!aligned16(g) || (reinterpret_cast<uintptr_t>(wf) | reinterpret_cast<uintptr_t>(gx)) & 3u) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double px = (double)N * h * w;
  CdfoProfScope prof(st, KID_LAYOUT, 2.0 * 9 * C0 * px, (4.0 * C0 + 4.0) * px);
  const int lds = (LP_HALO * LP_HALO * LP_BP + 9 * C0) * (int)sizeof(float);
  hipLaunchKernelGGL(lpips_stem_bwd_kernel, dim3((unsigned)cdiv(w, LP_T), (unsigned)cdiv(h, LP_T), (unsigned)N), dim3(256), lds, st, g, wf, h, w,
                     C0, gx);
  CDFO_LAUNCH_CHECK();
  return 0;
}
