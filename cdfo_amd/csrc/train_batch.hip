// Training batches and the training loss on the device (cdfo_amd/train_data.py, cdfo_amd/loss.py): what the reference does on the
// host per step -- RandomCrop -> Augment -> ToTensor in DataLoader workers (opt/data_LD_bi.py:245-505), eight .to(device) copies,
// the permutes and /32 of train_LD_37.py:365-374, and a six-operator Charbonnier expression (opt/loss.py:20-31) -- as two entry points.
//
//   cdfo_train_batch   the clip set is resident ([S][T] 8-bit planes); one launch cuts, flips, transposes and converts B samples.
//                      Plan row b = (seq, first, top, left, hflip, vflip, rot, 0).  For an n x n output plane (n = crop; the HR
//                      plane: n = 4 crop, origin (4 top, 4 left)):
//                          out[y][x] = P[top + i'][left + j'] / 255,  (i, j) = rot ? (x, y) : (y, x),  i' = vflip ? n-1-i : i,
//                          j' = hflip ? n-1-j : j,
//                      the division correctly rounded (a product with a rounded reciprocal differs by an ulp).  The motion field
//                      of frame first + 3, components (a, b, ref), goes through the same index map: m0 = b, m1 = a; hflip
//                      negates m0, vflip m1, rot swaps them; p = m / (ref * -1), NaN -> 0.  AN INFINITY STAYS: the reference
//                      keeps x / 0, and so does cdfo_seq_flows.  Slot k of the seven holds fl(p * w_k) / 128,
//                      w = 3, 2, 1, 0, -1, -2, -3 (the reference's / 4 and / 32 are exact); slot 3 is +0 whatever p.
//   cdfo_charbonnier   one pass over sr and hr: g = d / sqrt(d^2 + eps) and fp64 partial sums of sqrt(d^2 + eps) per workgroup; a
//                      one-wave kernel adds the partials in a fixed order.  No atomics: equal inputs give equal bits.
//
// Shape of cdfo_train_batch.  Grid (tile work list, sample): per sample 28 LR-sized planes, the HR plane and the motion field, cut
// into 32 x 32 output tiles.  The plan row is read through wave-uniform loads (its address depends on blockIdx alone).  Every tile
// goes through an LDS tile padded to 33 floats a row: the SOURCE tile is read along source rows (byte loads, no alignment assumed:
// `left` and W are arbitrary), converted once, and written in source order; the OUTPUT tile is read back through the index map --
// along LDS rows, or down LDS columns when rot transposes, both conflict-free at pitch 33 -- and leaves as 16-byte stores along
// output rows (crop % 4 == 0 makes every output row 16-byte aligned).  A plan row that does not fit the clip set writes nothing:
// the host validates plans (ClipSet.batch), the check in the kernel is the net under a wrong one.
#include "common.h"

namespace {

constexpr int TILE = 32, LDP = TILE + 1;

struct BatchArgs {
  const unsigned char *lr, *pms, *ufs, *hr;
  const signed char *rms, *mvl0;
  const int* plan;
  float *x, *pms_o, *rms_o, *ufs_o, *mvs0, *hr_o;
  int S, T, H, W, Hu, c;
};

// one 32 x 32 output tile of an n x n plane, and the source tile (origin (si0, sj0) inside the crop, ni x nj) that feeds it
struct TileMap {
  int n, oy0, ox0, si0, sj0, ni, nj, hf, vf, rot;
  __device__ TileMap(int n_, int tile, int hf_, int vf_, int rot_) : n(n_), hf(hf_), vf(vf_), rot(rot_) {
    const int per_row = (n + TILE - 1) / TILE;
    oy0 = (tile / per_row) * TILE;
    ox0 = (tile % per_row) * TILE;
    const int th = min(TILE, n - oy0), tw = min(TILE, n - ox0);
    const int i0 = rot ? ox0 : oy0, j0 = rot ? oy0 : ox0;
    ni = rot ? tw : th;
    nj = rot ? th : tw;
    si0 = vf ? n - i0 - ni : i0;      // i' = n-1-i over [i0, i0+ni) starts at n - i0 - ni
    sj0 = hf ? n - j0 - nj : j0;
  }
  // LDS offset of the source of output position (y, x)
  __device__ __forceinline__ int lds_of(int y, int x) const {
    const int i = rot ? x : y, j = rot ? y : x;
    return ((vf ? n - 1 - i : i) - si0) * LDP + (hf ? n - 1 - j : j) - sj0;
  }
};

// src: the plane's sample at the crop's origin; pitch in samples
template <typename T>
__device__ __forceinline__ void plane_tile(const T* __restrict__ src, int pitch, const TileMap& m, float* __restrict__ out, float* lds) {
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
  if (r < m.ni) {
    const T* row = src + (long long)(m.si0 + r) * pitch + m.sj0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < m.nj) lds[r * LDP + c0 + q] = __fdiv_rn((float)row[c0 + q], 255.0f);
  }
  __syncthreads();
  const int y = m.oy0 + r, x = m.ox0 + c0;
  if (y < m.n && x < m.n) {             // n % 4 == 0: four outputs are inside together
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = lds[m.lds_of(y, x + q)];
    *reinterpret_cast<f32x4*>(out + (long long)y * m.n + x) = v;
  }
}

// src: the field's (a, b, ref) at the crop's origin; pitch in pixels; out: the sample's [7][2][n][n]
__device__ __forceinline__ void motion_tile(const signed char* __restrict__ src, int pitch, const TileMap& m, float* __restrict__ out,
                                            float* lds) {
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
  float* lds1 = lds + TILE * LDP;
  if (r < m.ni) {
    const signed char* row = src + ((long long)(m.si0 + r) * pitch + m.sj0) * 3;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < m.nj) {
        const signed char* e = row + (c0 + q) * 3;
        float m0 = (float)e[1], m1 = (float)e[0];             // the reference swaps the first two components first
        if (m.hf) m0 = -m0;
        if (m.vf) m1 = -m1;
        if (m.rot) { const float t = m0; m0 = m1; m1 = t; }
        const float den = (float)e[2] * -1.0f;
        float p0 = __fdiv_rn(m0, den), p1 = __fdiv_rn(m1, den);
        if (p0 != p0) p0 = 0.f;                               // NaN -> 0; x / 0 stays infinite
        if (p1 != p1) p1 = 0.f;
        lds[r * LDP + c0 + q] = p0;
        lds1[r * LDP + c0 + q] = p1;
      }
  }
  __syncthreads();
  const int y = m.oy0 + r, x = m.ox0 + c0;
  if (y < m.n && x < m.n) {
    float p[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = m.lds_of(y, x + q);
      p[0][q] = lds[o];
      p[1][q] = lds1[o];
    }
    const long long plane = (long long)m.n * m.n;
    float* o = out + (long long)y * m.n + x;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int comp = 0; comp < 2; ++comp) {
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = k == 3 ? 0.f : __fmul_rn(p[comp][q], (float)(3 - k)) * 0.0078125f;   // the product is rounded first; / 128 is exact
        *reinterpret_cast<f32x4*>(o + (k * 2 + comp) * plane) = v;
      }
  }
}

__global__ __launch_bounds__(256) void train_batch_kernel(BatchArgs a) {
  __shared__ float lds[2 * TILE * LDP];
  const int b = blockIdx.y;
  const int* __restrict__ row = a.plan + b * 8;               // wave-uniform: scalar loads
  const int s = row[0], f = row[1], top = row[2], left = row[3], hf = row[4], vf = row[5], rot = row[6];
  const int c = a.c;
  if (s < 0 || s >= a.S || f < 0 || f + 7 > a.T || top < 0 || top + c > a.H || left < 0 || left + c > a.W || (hf | vf | rot) & ~1) return;
  const int per = (c + TILE - 1) / TILE, tl = per * per;
  const int per_hr = (4 * c + TILE - 1) / TILE, thr = per_hr * per_hr;
  int w = blockIdx.x;
  const long long frame0 = (long long)s * a.T + f;            // the first of the sample's seven frames, in frames of the set
  if (w < 28 * tl) {
    const int p = w / tl, arr = p / 7, k = p % 7;
    const TileMap m(c, w % tl, hf, vf, rot);
    const long long o = ((long long)b * 7 + k) * c * c;       // x, pms: [B][7][1][c][c]; rms, ufs: [B][1][7][c][c] -- the same memory
    const long long in = ((frame0 + k) * a.H + top) * a.W + left;
    if (arr == 0) plane_tile(a.lr + in, a.W, m, a.x + o, lds);
    else if (arr == 1) plane_tile(a.pms + in, a.W, m, a.pms_o + o, lds);
    else if (arr == 2) plane_tile(a.rms + in, a.W, m, a.rms_o + o, lds);
    else plane_tile(a.ufs + ((frame0 + k) * a.Hu + top) * a.W + left, a.W, m, a.ufs_o + o, lds);   // Hu >= H rows, indexed from the top
    return;
  }
  w -= 28 * tl;
  if (w < thr) {
    const TileMap m(4 * c, w, hf, vf, rot);
    const long long in = ((frame0 + 3) * 4 * a.H + 4 * top) * 4 * a.W + 4 * left;
    plane_tile(a.hr + in, 4 * a.W, m, a.hr_o + (long long)b * 16 * c * c, lds);
    return;
  }
  w -= thr;
  const TileMap m(c, w, hf, vf, rot);
  motion_tile(a.mvl0 + (((frame0 + 3) * a.H + top) * a.W + left) * 3, a.W, m, a.mvs0 + (long long)b * 14 * c * c, lds);
}

// ---------------------------------------------------------------------------------------------------------- cdfo_charbonnier
__global__ __launch_bounds__(256) void charbonnier_kernel(const float* __restrict__ sr, const float* __restrict__ hr, long long n,
                                                          float eps, int vec, float* __restrict__ g, double* __restrict__ partial) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * 1024) {
    const int cnt = n - i < 4 ? (int)(n - i) : 4;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (vec && cnt == 4) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(sr + i), vb = *reinterpret_cast<const f32x4*>(hr + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) { a[q] = va[q]; b[q] = vb[q]; }
    } else {
      for (int q = 0; q < cnt; ++q) { a[q] = sr[i + q]; b[q] = hr[i + q]; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = a[q] - b[q];
      const float t = __fsqrt_rn(d * d + eps);                // correctly rounded: no fast reciprocal square root
      o[q] = __fdiv_rn(d, t);
      if (q < cnt) acc += (double)t;
    }
    if (vec && cnt == 4) {
      const f32x4 vo = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(g + i) = vo;
    } else {
      for (int q = 0; q < cnt; ++q) g[i + q] = o[q];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one wave: lane l adds partials l, l + 64, ... in order, then the xor tree: a fixed order
__global__ __launch_bounds__(64) void charbonnier_sum_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) acc += partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (threadIdx.x == 0) *loss = (float)acc;
}

}  // namespace

extern "C" int cdfo_train_batch(const unsigned char* lr, const unsigned char* pms, const signed char* rms, const unsigned char* ufs,
                                const signed char* mvl0, const unsigned char* hr, int S, int T, int H, int W, int Hu, const int* plan,
                                int B, int crop, float* x, float* pms_out, float* rms_out, float* ufs_out, float* mvs0, float* hr_out,
                                void* stream) {
  if (!lr || !pms || !rms || !ufs || !mvl0 || !hr || !plan || !x || !pms_out || !rms_out || !ufs_out || !mvs0 || !hr_out) return CDFO_EINVAL;
  if (S <= 0 || T < 7 || H <= 0 || W <= 0 || Hu < H || B <= 0 || B > 65535) return CDFO_EINVAL;
  if (crop <= 0 || crop % 4 || crop > H || crop > W || crop > 4096) return CDFO_EINVAL;
  if (!aligned16(x) || !aligned16(pms_out) || !aligned16(rms_out) || !aligned16(ufs_out) || !aligned16(mvs0) || !aligned16(hr_out) ||
      (reinterpret_cast<uintptr_t>(plan) & 3u) != 0)
    return CDFO_EALIGN;
  BatchArgs a;
  a.lr = lr; a.pms = pms; a.ufs = ufs; a.hr = hr; a.rms = rms; a.mvl0 = mvl0; a.plan = plan;
  a.x = x; a.pms_o = pms_out; a.rms_o = rms_out; a.ufs_o = ufs_out; a.mvs0 = mvs0; a.hr_o = hr_out;
  a.S = S; a.T = T; a.H = H; a.W = W; a.Hu = Hu; a.c = crop;
  const int per = cdiv(crop, TILE), per_hr = cdiv(4 * crop, TILE);
  const long long work = 29LL * per * per + (long long)per_hr * per_hr;
  if (work > 0x7fffffffLL) return CDFO_EINVAL;
  hipLaunchKernelGGL(train_batch_kernel, dim3((unsigned)work, B), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  CDFO_LAUNCH_CHECK();
  return 0;
}

// a fixed function of n: the grid, and with it the order of the sum, never depends on the device
static int charbonnier_blocks(long long n) {
  const long long blocks = (n + 1023) / 1024;
  return (int)(blocks < CDFO_CHARBONNIER_MAX_BLOCKS ? blocks : CDFO_CHARBONNIER_MAX_BLOCKS);
}

extern "C" int cdfo_charbonnier(const float* sr, const float* hr, long long n, float eps, float* grad, double* partial, int partial_cap,
                                float* loss, void* stream) {
  if (!sr || !hr || !grad || !partial || !loss || n <= 0 || !(eps >= 0.f)) return CDFO_EINVAL;
  const int blocks = charbonnier_blocks(n);
  if (partial_cap < blocks) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(sr) | reinterpret_cast<uintptr_t>(hr) | reinterpret_cast<uintptr_t>(grad) |
       reinterpret_cast<uintptr_t>(loss)) & 3u || (reinterpret_cast<uintptr_t>(partial) & 7u))
    return CDFO_EALIGN;
  const int vec = aligned16(sr) && aligned16(hr) && aligned16(grad);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(charbonnier_kernel, dim3(blocks), dim3(256), 0, st, sr, hr, n, eps, vec, grad, partial);
  CDFO_LAUNCH_CHECK();
  hipLaunchKernelGGL(charbonnier_sum_kernel, dim3(1), dim3(64), 0, st, partial, blocks, loss);
  CDFO_LAUNCH_CHECK();
  return 0;
}
