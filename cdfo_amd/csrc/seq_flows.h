// Device pieces shared by the kernels that build a chunk's inputs: sequence.hip (whole sequence resident) and live.hip (rings of
// chunk + 6 frames).  A frame descriptor whose range check returns zero outside the frame, the loads of a motion field's twelve
// values, and the per-pixel body of cdfo_seq_flows / cdfo_seq_flows_ring: test_LD_22_FPS.py's mv2mvs (:100-122) and
// modify_mv_for_end_frames (:200-225), bit for bit.
// seq_flows_ra_pixels is the same body for the random-access field (both lists, seq_flows_ra.hip).
#pragma once
#include "lds_dma.h"

namespace {


__device__ __forceinline__ __amdgpu_buffer_rsrc_t frame_rsrc(const unsigned char* base, int bytes) {
  // wave-uniform by construction (kernel arguments and blockIdx only); readfirstlane makes that provable, so the loads are not
  // wrapped in waterfall loops
  const unsigned long long p = reinterpret_cast<unsigned long long>(base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
  void* q = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane(bytes), BUFFER_RSRC_WORD3);
}

template <typename T> __device__ __forceinline__ float mv_to_float(T v) { return (float)v; }

struct bf16_t { unsigned short bits; };
template <> __device__ __forceinline__ float mv_to_float<bf16_t>(bf16_t v) { return __uint_as_float((unsigned)v.bits << 16); }

// the twelve values (four pixels x three components) at element offset e0 of a field of n elements; outside -> 0
template <typename T>
__device__ __forceinline__ void load_mv12(const T* __restrict__ f, int e0, int n, float (&m)[12]) {
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = (e0 + k < n) ? mv_to_float<T>(f[e0 + k]) : 0.f;
}
// fp32: three 16-byte buffer loads (dword-aligned: a row of W pixels is 12 W bytes).  The last pixels of a field, whose twelve
// values would run past its end, and the padding rows take the guarded element loads; the descriptor's range check stays
// behind them as the net under a wrong offset
template <>
__device__ __forceinline__ void load_mv12<float>(const float* __restrict__ f, int e0, int n, float (&m)[12]) {
  if (e0 + 12 > n) {
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = (e0 + k < n) ? f[e0 + k] : 0.f;
    return;
  }
  const __amdgpu_buffer_rsrc_t r = frame_rsrc(reinterpret_cast<const unsigned char*>(f), n * 4);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (e0 + 4 * q) * 4, 0, 0));
#pragma unroll
    for (int k = 0; k < 4; ++k) m[4 * q + k] = v[k];
  }
}

// One thread: four consecutive pixels (x .. x+3 of row y) of centre frame i, all seven slots and both components, from `field`
// [H][W][3] (the entry the centre reads) into `o` [7][2][Hp][Wp]: 14 16-byte stores.  Tn: the length the three end rules are
// judged against; a caller that does not know the end yet passes a value no centre can reach, so that none of them applies.
template <typename T>
__device__ __forceinline__ void seq_flows_pixels(const T* __restrict__ field, int H, int W, int i, int Tn, int Hp, int Wp, int y, int x,
                                                 float* __restrict__ o) {
  const int n = H * W * 3;
  float m[12];
  // padding rows start beyond the field: every element is out of range
  load_mv12<T>(field, y < H ? (y * W + x) * 3 : n, n, m);
  float v[7][2][4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const bool inside = y < H && x + p < W;
    // mv2mvs: components swapped, divided by -mv[2], NaN -> 0 (x / 0 stays inf), x 3, 2, 1, 0, -1, -2, -3, slot 3 forced to 0, / 128.
    // Each step is one correctly rounded fp32 operation, in the order of the host function.
    const float d = m[3 * p + 2] * -1.0f;
    float f[2] = {__fdiv_rn(m[3 * p + 1], d), __fdiv_rn(m[3 * p + 0], d)};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (f[c] != f[c]) f[c] = 0.f;
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const float sc = (float)(3 - s);
        const float r = s == 3 ? 0.f : __fdiv_rn(f[c] * sc, 128.0f);
        v[s][c][p] = inside ? r : 0.f;                       // zero padding to Hp x Wp
      }
    }
  }
  // modify_mv_for_end_frames, the six rules in the reference's order (they overlap in sequences shorter than six frames)
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      auto& a = v;
      if (i == 0) a[0][c][p] = a[1][c][p] = a[2][c][p] = 0.f;
      if (i == 1) { a[0][c][p] = a[2][c][p]; a[1][c][p] = a[2][c][p]; }
      if (i == 2) a[0][c][p] = a[1][c][p];
      if (i == Tn - 1) a[4][c][p] = a[5][c][p] = a[6][c][p] = 0.f;
      if (i == Tn - 2) { a[5][c][p] = a[4][c][p]; a[6][c][p] = a[4][c][p]; }
      if (i == Tn - 3) a[6][c][p] = a[5][c][p];
    }
  const long long plane = (long long)Hp * Wp;
  o += (long long)y * Wp + x;
#pragma unroll
  for (int s = 0; s < 7; ++s)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      f32x4 q = {v[s][c][0], v[s][c][1], v[s][c][2], v[s][c][3]};
      *reinterpret_cast<f32x4*>(o + (s * 2 + c) * plane) = q;
    }
}

// The random-access form (cdfo_seq_flows_ra / cdfo_seq_flows_ra_ring, seq_flows_ra.hip): the same four pixels, stores and end rules,
// from BOTH lists' fields of the entry the centre reads.  Slots 0-2 come from list 0 (p2 = m / (ref * -1)), slots 4-6 from list 1
// (p4 = m / ref); a pixel with no reference in one list (ref == -99 after the conversion to fp32) takes the other list's vector,
// negated: opt/data_RA_bi.py's field as cdfo_train_batch_ra builds it, without the flips.
template <typename T>
__device__ __forceinline__ void seq_flows_ra_pixels(const T* __restrict__ field0, const T* __restrict__ field1, int H, int W, int i, int Tn,
                                                    int Hp, int Wp, int y, int x, float* __restrict__ o) {
  const int n = H * W * 3;
  float m0[12], m1[12];
  // padding rows start beyond the field: every element is out of range
  const int e0 = y < H ? (y * W + x) * 3 : n;
  load_mv12<T>(field0, e0, n, m0);
  load_mv12<T>(field1, e0, n, m1);
  float v[7][2][4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const bool inside = y < H && x + p < W;
    // Each step is one correctly rounded fp32 operation, in the order of streaming.mv2mvs_ra.
    const float d0 = m0[3 * p + 2] * -1.0f, d1 = m1[3 * p + 2];
    float p2[2] = {__fdiv_rn(m0[3 * p + 1], d0), __fdiv_rn(m0[3 * p + 0], d0)};
    float p4[2] = {__fdiv_rn(m1[3 * p + 1], d1), __fdiv_rn(m1[3 * p + 0], d1)};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (p2[c] != p2[c]) p2[c] = 0.f;
      if (p4[c] != p4[c]) p4[c] = 0.f;
    }
    if (m0[3 * p + 2] == -99.0f) { p2[0] = -p4[0]; p2[1] = -p4[1]; }
    if (m1[3 * p + 2] == -99.0f) { p4[0] = -p2[0]; p4[1] = -p2[1]; }   // after the line above: both marked leaves p4 as it was
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const float sc = (float)(s < 3 ? 3 - s : s - 3);
        const float r = s == 3 ? 0.f : __fdiv_rn(__fmul_rn(s < 3 ? p2[c] : p4[c], sc), 128.0f);
        v[s][c][p] = inside ? r : 0.f;                         // zero padding to Hp x Wp
      }
  }
  // modify_mv_for_end_frames, as in seq_flows_pixels
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      auto& a = v;
      if (i == 0) a[0][c][p] = a[1][c][p] = a[2][c][p] = 0.f;
      if (i == 1) { a[0][c][p] = a[2][c][p]; a[1][c][p] = a[2][c][p]; }
      if (i == 2) a[0][c][p] = a[1][c][p];
      if (i == Tn - 1) a[4][c][p] = a[5][c][p] = a[6][c][p] = 0.f;
      if (i == Tn - 2) { a[5][c][p] = a[4][c][p]; a[6][c][p] = a[4][c][p]; }
      if (i == Tn - 3) a[6][c][p] = a[5][c][p];
    }
  const long long plane = (long long)Hp * Wp;
  o += (long long)y * Wp + x;
#pragma unroll
  for (int s = 0; s < 7; ++s)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      f32x4 q = {v[s][c][0], v[s][c][1], v[s][c][2], v[s][c][3]};
      *reinterpret_cast<f32x4*>(o + (s * 2 + c) * plane) = q;
    }
}

}  // namespace
