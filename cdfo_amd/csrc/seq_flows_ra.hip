// The random-access forms of cdfo_seq_flows (sequence.hip) and cdfo_seq_flows_ring (live.hip): the flows of K centre frames from BOTH
// lists' motion fields, for a model trained on opt/data_RA_bi.py's field (cdfo_amd/streaming.py with coding="RA").
//
//   cdfo_seq_flows_ra       mv0, mv1 [T,H,W,3] of one element type -> [K,7,2,Hp,Wp]: slots 0-2 from list 0, slots 4-6 from list 1, a
//                           pixel without a reference in one list (-99) takes the other list's vector negated; then
//                           modify_mv_for_end_frames.  Both lists are read at the entry the LD form reads, max(1, i).
//   cdfo_seq_flows_ra_ring  the same from two fp32 rings [cap,H,W,3], the sequence's end possibly not known yet.
//
// A translation unit of its own so that sequence.hip and live.hip compile to the code they had without these beside them.  The
// per-pixel body is seq_flows.h's seq_flows_ra_pixels; grids, loads and stores are the LD twins': one thread per four pixels of a row,
// guarded loads outside the field, 14 16-byte stores, no LDS, no atomics.  24 bytes per pixel are read for the 56 written.
#include "common.h"
#include "seq_flows.h"

namespace {

// grid (x: Hp * Wp / 4 threads; y: centre frame)
template <typename T>
__global__ __launch_bounds__(256) void seq_flows_ra_kernel(const T* __restrict__ mv0, const T* __restrict__ mv1, int Tn, int H, int W, int i0,
                                                           int Hp, int Wp, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w4 = Wp >> 2;
  if (t >= Hp * w4) return;
  const int y = t / w4, x = (t - y * w4) << 2;
  const int i = i0 + (int)blockIdx.y;
  const int entry = Tn > 1 ? (i > 1 ? i : 1) : 0;            // both lists at the entry the LD form reads
  const long long at = (long long)entry * (H * W * 3);
  seq_flows_ra_pixels<T>(mv0 + at, mv1 + at, H, W, i, Tn, Hp, Wp, y, x, out + (long long)blockIdx.y * 14 * Hp * Wp);
}

template <typename T>
void launch_seq_flows_ra(const void* mv0, const void* mv1, int Tn, int H, int W, int i0, int K, int Hp, int Wp, float* out, hipStream_t st) {
  hipLaunchKernelGGL(seq_flows_ra_kernel<T>, dim3(cdiv(Hp * (Wp / 4), 256), K), dim3(256), 0, st, static_cast<const T*>(mv0),
                     static_cast<const T*>(mv1), Tn, H, W, i0, Hp, Wp, out);
}

// the centre's entry lives in slot entry mod cap of both rings
__global__ __launch_bounds__(256) void seq_flows_ra_ring_kernel(const float* __restrict__ ring0, const float* __restrict__ ring1, int cap,
                                                                int T_known, int H, int W, int i0, int Hp, int Wp, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w4 = Wp >> 2;
  if (t >= Hp * w4) return;
  const int y = t / w4, x = (t - y * w4) << 2;
  const int i = i0 + (int)blockIdx.y;
  const int entry = T_known == 1 ? 0 : (i > 1 ? i : 1);
  // an open stream has no end yet: the end rules are judged against a length that no centre reaches
  const int Tn = T_known > 0 ? T_known : 0x7fffffff;
  const long long at = (long long)(entry % cap) * (H * W * 3);
  seq_flows_ra_pixels<float>(ring0 + at, ring1 + at, H, W, i, Tn, Hp, Wp, y, x, out + (long long)blockIdx.y * 14 * Hp * Wp);
}

}  // namespace

extern "C" int cdfo_seq_flows_ra(const void* mv0, const void* mv1, int dtype, int T, int H, int W, int i0, int K, int Hp, int Wp, float* out,
                                 void* stream) {
  if (!mv0 || !mv1 || !out || T <= 0 || H <= 0 || W <= 0 || K <= 0 || K > 65535 || i0 < 0 || (long long)i0 + K > T || Hp < H || Wp < W ||
      Wp % 4)
    return CDFO_EINVAL;
  if ((long long)H * W * 3 * 8 > 0x7fffffffLL || (long long)Hp * Wp > 0x7fffffffLL) return CDFO_EINVAL;   // 32-bit offsets inside a field
  if (dtype < CDFO_MV_F32 || dtype > CDFO_MV_I64) return CDFO_EINVAL;
  if (!aligned16(out) ||
      (dtype == CDFO_MV_F32 && ((reinterpret_cast<uintptr_t>(mv0) | reinterpret_cast<uintptr_t>(mv1)) & 3u) != 0))
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 0, (double)K * (56.0 * Hp * Wp + 24.0 * H * W));
  switch (dtype) {
    case CDFO_MV_F32: launch_seq_flows_ra<float>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_F64: launch_seq_flows_ra<double>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_F16: launch_seq_flows_ra<_Float16>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_BF16: launch_seq_flows_ra<bf16_t>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I8: launch_seq_flows_ra<signed char>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_U8: launch_seq_flows_ra<unsigned char>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I16: launch_seq_flows_ra<short>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I32: launch_seq_flows_ra<int>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I64: launch_seq_flows_ra<long long>(mv0, mv1, T, H, W, i0, K, Hp, Wp, out, st); break;
    default: return CDFO_EINVAL;
  }
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_seq_flows_ra_ring(const float* ring0, const float* ring1, int cap, int H, int W, int i0, int K, int T_known, int Hp,
                                      int Wp, float* out, void* stream) {
  if (!ring0 || !ring1 || !out || cap <= 0 || H <= 0 || W <= 0 || K <= 0 || K > 65535 || i0 < 0 || T_known < 0 || Hp < H || Wp < W ||
      Wp % 4)
    return CDFO_EINVAL;
  if (T_known > 0 && (long long)i0 + K > T_known) return CDFO_EINVAL;
  if ((long long)i0 + K > 0x7ffffff0LL) return CDFO_EINVAL;
  if ((long long)H * W * 3 * 8 > 0x7fffffffLL || (long long)Hp * Wp > 0x7fffffffLL) return CDFO_EINVAL;   // 32-bit offsets inside a field
  if (!aligned16(out) || ((reinterpret_cast<uintptr_t>(ring0) | reinterpret_cast<uintptr_t>(ring1)) & 3u) != 0) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 0, (double)K * (56.0 * Hp * Wp + 24.0 * H * W));
  hipLaunchKernelGGL(seq_flows_ra_ring_kernel, dim3(cdiv(Hp * (Wp / 4), 256), K), dim3(256), 0, st, ring0, ring1, cap, T_known, H, W, i0,
                     Hp, Wp, out);
  CDFO_LAUNCH_CHECK();
  return 0;
}
