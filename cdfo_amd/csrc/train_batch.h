// The device pieces and the host checks that cdfo_train_batch (train_batch.hip) and cdfo_train_batch_ra (train_batch_ra.hip) share: the
// tile map, the plane and motion tiles and the kernel template with its work list.  Each file instantiates one form: with both in one
// module the compiler emits other LDS address arithmetic for the LD form, whose code is to stay what it was before the RA form came.
#pragma once
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

// the RA form: src0, src1: both lists' fields at the crop's origin.  The complement needs the pixel's own two fields only, so it is done
// before staging; lds holds p2.x, p2.y, p4.x, p4.y
__device__ __forceinline__ void motion_tile_ra(const signed char* __restrict__ src0, const signed char* __restrict__ src1, int pitch,
                                               const TileMap& m, float* __restrict__ out, float* lds) {
  const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
  constexpr int PL = TILE * LDP;
  if (r < m.ni) {
    const long long off = ((long long)(m.si0 + r) * pitch + m.sj0) * 3;
    const signed char *row0 = src0 + off, *row1 = src1 + off;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + q < m.nj) {
        const signed char *e0 = row0 + (c0 + q) * 3, *e1 = row1 + (c0 + q) * 3;
        float p[2][2];                                          // [list][component]
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          const signed char* e = l ? e1 : e0;
          float m0 = (float)e[1], m1 = (float)e[0];
          if (m.hf) m0 = -m0;
          if (m.vf) m1 = -m1;
          if (m.rot) { const float t = m0; m0 = m1; m1 = t; }
          const float den = l ? (float)e[2] : (float)e[2] * -1.0f;   // list 0 points back: / (ref * -1); list 1 forward: / ref
          p[l][0] = __fdiv_rn(m0, den);
          p[l][1] = __fdiv_rn(m1, den);
          if (p[l][0] != p[l][0]) p[l][0] = 0.f;
          if (p[l][1] != p[l][1]) p[l][1] = 0.f;
        }
        if (e0[2] == -99) { p[0][0] = -p[1][0]; p[0][1] = -p[1][1]; }
        if (e1[2] == -99) { p[1][0] = -p[0][0]; p[1][1] = -p[0][1]; }   // after the line above: both marked leaves p4 as it was
        const int o = r * LDP + c0 + q;
        lds[o] = p[0][0];
        lds[PL + o] = p[0][1];
        lds[2 * PL + o] = p[1][0];
        lds[3 * PL + o] = p[1][1];
      }
  }
  __syncthreads();
  const int y = m.oy0 + r, x = m.ox0 + c0;
  if (y < m.n && x < m.n) {
    float p[4][4];                                              // [list * 2 + component][q]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = m.lds_of(y, x + q);
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j][q] = lds[j * PL + o];
    }
    const long long plane = (long long)m.n * m.n;
    float* o = out + (long long)y * m.n + x;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int comp = 0; comp < 2; ++comp) {
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          v[q] = k == 3 ? 0.f : __fmul_rn(p[(k > 3) * 2 + comp][q], (float)(k < 3 ? 3 - k : k - 3)) * 0.0078125f;
        *reinterpret_cast<f32x4*>(o + (k * 2 + comp) * plane) = v;
      }
  }
}

// both kernels: train_batch.hip instantiates the LD form, train_batch_ra.hip the RA form; mvl1 is the RA form's second list
template <bool RA>
__global__ __launch_bounds__(256) void train_batch_kernel(BatchArgs a, const signed char* __restrict__ mvl1) {
  __shared__ float lds[(RA ? 4 : 2) * TILE * LDP];
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
  if constexpr (RA) {
    const long long in = (((frame0 + 3) * a.H + top) * a.W + left) * 3;
    motion_tile_ra(a.mvl0 + in, mvl1 + in, a.W, m, a.mvs0 + (long long)b * 14 * c * c, lds);
  } else {
    motion_tile(a.mvl0 + (((frame0 + 3) * a.H + top) * a.W + left) * 3, a.W, m, a.mvs0 + (long long)b * 14 * c * c, lds);
  }
}

// the argument checks of both entry points; fills the kernel's arguments and the grid's first dimension
static inline int train_batch_args(const unsigned char* lr, const unsigned char* pms, const signed char* rms, const unsigned char* ufs,
                                   const signed char* mvl0, const unsigned char* hr, int S, int T, int H, int W, int Hu, const int* plan,
                                   int B, int crop, float* x, float* pms_out, float* rms_out, float* ufs_out, float* mvs0, float* hr_out,
                                   BatchArgs& a, unsigned& work_out) {
  if (!lr || !pms || !rms || !ufs || !mvl0 || !hr || !plan || !x || !pms_out || !rms_out || !ufs_out || !mvs0 || !hr_out) return CDFO_EINVAL;
  if (S <= 0 || T < 7 || H <= 0 || W <= 0 || Hu < H || B <= 0 || B > 65535) return CDFO_EINVAL;
  if (crop <= 0 || crop % 4 || crop > H || crop > W || crop > 4096) return CDFO_EINVAL;
  if (!aligned16(x) || !aligned16(pms_out) || !aligned16(rms_out) || !aligned16(ufs_out) || !aligned16(mvs0) || !aligned16(hr_out) ||
      (reinterpret_cast<uintptr_t>(plan) & 3u) != 0)
    return CDFO_EALIGN;
  a.lr = lr; a.pms = pms; a.ufs = ufs; a.hr = hr; a.rms = rms; a.mvl0 = mvl0; a.plan = plan;
  a.x = x; a.pms_o = pms_out; a.rms_o = rms_out; a.ufs_o = ufs_out; a.mvs0 = mvs0; a.hr_o = hr_out;
  a.S = S; a.T = T; a.H = H; a.W = W; a.Hu = Hu; a.c = crop;
  const int per = cdiv(crop, TILE), per_hr = cdiv(4 * crop, TILE);
  const long long work = 29LL * per * per + (long long)per_hr * per_hr;
  if (work > 0x7fffffffLL) return CDFO_EINVAL;
  work_out = (unsigned)work;
  return 0;
}

}  // namespace
