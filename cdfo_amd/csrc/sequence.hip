// Sequence-level input building for chunked inference (cdfo_amd/streaming.py::StreamingSR.run_chunked): K consecutive centre
// frames of ONE sequence per forward, against a per-frame feature bank.
//
//   cdfo_seq_flows      the decoder's motion field [T,H,W,3] -> the seven per-slot flows of K centre frames [K,7,2,Hp,Wp] in one
//                       launch: test_LD_22_FPS.py's mv2mvs (:100-122) and modify_mv_for_end_frames (:200-225) per pixel, bit for bit.
//   cdfo_gather_frames  dst[j] = src[idx[j]] over whole frames, index table on the device: the frame-major window stack out of
//                       the feature bank (clipped / repeated indices at the sequence's ends included) and the [K,7] windows of
//                       the one-channel planes, one pass each.
//   cdfo_flow_warp_frames  flow_warp with an indexed source: each output image samples the bank frame its index names, in place,
//                       with the flow of its (window, neighbour slot): one launch per neighbour group of the shared-compensation
//                       mode, no gathered copy of the bank.  Per pixel it is flow_warp_kernel's arithmetic (flow_sample.h).
//
// The first two are streaming kernels: 16-byte stores, 16-byte reads through a buffer descriptor whose range check returns zero for
// everything outside the frame (a bad index), no atomics, no LDS.  cdfo_seq_flows reads 12 bytes per pixel for the 56 it writes;
// only the fp32 field (what the evaluation loop holds) is read in 16-byte loads, every other element type in guarded element loads.
#include "common.h"
#include "flow_sample.h"
#include "seq_flows.h"

namespace {

// ---------------------------------------------------------------------------------------------------- cdfo_gather_frames
// grid (x: 16-byte vectors of a frame, four per thread and trip; y: destination frame)
__global__ __launch_bounds__(256) void gather_frames_kernel(const unsigned char* __restrict__ src, u32x4* __restrict__ dst,
                                                            const int* __restrict__ idx, int n_src, int frame_bytes) {
  const int j = blockIdx.y;
  const int s = idx[j];
  // an index outside [0, n_src) gets a descriptor of zero bytes: every load through it returns zero
  const bool ok = s >= 0 && s < n_src;
  const __amdgpu_buffer_rsrc_t r = frame_rsrc(src + (long long)(ok ? s : 0) * frame_bytes, ok ? frame_bytes : 0);
  const int n16 = frame_bytes >> 4;
  u32x4* d = dst + (long long)j * n16;
  const int stride = gridDim.x * 256;
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (i + u * stride) << 4, 0, 0));
#pragma unroll
    for (int u = 0; u < 4; ++u) d[i + u * stride] = v[u];
  }
  for (; i < n16; i += stride) d[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, i << 4, 0, 0));
}

// ------------------------------------------------------------------------------------------------- cdfo_flow_warp_frames
// thread = (pixel, 4-channel group) of ONE output image, 16-byte loads and stores as in flow_warp_kernel.
// grid (x: workgroups striding over the image's H * W * C / 4 threads; y: output image j = g * K + k): the image's bank index and
// the base of its motion field depend on blockIdx.y alone, so they are wave-uniform (one scalar load of idx[j] per wave)
__global__ __launch_bounds__(256) void flow_warp_frames_kernel(const float* __restrict__ bank, int ldi, int n_bank,
                                                               const int* __restrict__ idx, const float* __restrict__ mv,
                                                               long long mv_kstride, int slot0, int K, int H, int W, int C,
                                                               float* __restrict__ out, int ldo) {
  const int j = blockIdx.y;
  const int s = idx[j];
  const int g = j / K, k = j - g * K;
  const int cgs = C >> 2;
  const int total = H * W * cgs;
  float* o = out + (long long)j * H * W * ldo;
  if (s < 0 || s >= n_bank) {     // cdfo_gather_frames' contract: an index outside the bank names a frame of zeros
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
      const int cg = i % cgs, p = i / cgs;
      *reinterpret_cast<f32x4*>(o + (long long)p * ldo + cg * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const float* img = bank + (long long)s * H * W * ldi;
  const float* m = mv + (long long)k * mv_kstride + (long long)(slot0 + g) * 2 * H * W;
  const float wm = (float)(W - 1 > 1 ? W - 1 : 1), hm = (float)(H - 1 > 1 ? H - 1 : 1);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int cg = i % cgs, p = i / cgs;
    const int x = p % W, y = p / W;
    *reinterpret_cast<f32x4*>(o + (long long)p * ldo + cg * 4) = flow_warp_sample(img + cg * 4, ldi, m, x, y, H, W, wm, hm);
  }
}

// -------------------------------------------------------------------------------------------------------- cdfo_seq_flows
// One thread: four consecutive pixels of one row of one centre frame, all seven slots and both components: 14 16-byte stores.
// grid (x: Hp * Wp / 4 threads; y: centre frame)
template <typename T>
__global__ __launch_bounds__(256) void seq_flows_kernel(const T* __restrict__ mv, int Tn, int H, int W, int i0, int Hp, int Wp,
                                                        float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w4 = Wp >> 2;
  if (t >= Hp * w4) return;
  const int y = t / w4, x = (t - y * w4) << 2;
  const int i = i0 + (int)blockIdx.y;
  const int entry = Tn > 1 ? (i > 1 ? i : 1) : 0;            // the field of frame 0 is read from entry 1 (test_LD_22_FPS.py:168)
  // the per-pixel body is shared with cdfo_seq_flows_ring (seq_flows.h)
  seq_flows_pixels<T>(mv + (long long)entry * (H * W * 3), H, W, i, Tn, Hp, Wp, y, x, out + (long long)blockIdx.y * 14 * Hp * Wp);
}

template <typename T>
void launch_seq_flows(const void* mv, int Tn, int H, int W, int i0, int K, int Hp, int Wp, float* out, hipStream_t st) {
  hipLaunchKernelGGL(seq_flows_kernel<T>, dim3(cdiv(Hp * (Wp / 4), 256), K), dim3(256), 0, st, static_cast<const T*>(mv), Tn, H, W,
                     i0, Hp, Wp, out);
}

}  // namespace

extern "C" int cdfo_seq_flows(const void* mv, int dtype, int T, int H, int W, int i0, int K, int Hp, int Wp, float* out, void* stream) {
  if (!mv || !out || T <= 0 || H <= 0 || W <= 0 || K <= 0 || i0 < 0 || i0 + K > T || Hp < H || Wp < W || Wp % 4) return CDFO_EINVAL;
  if ((long long)H * W * 3 * 8 > 0x7fffffffLL || (long long)Hp * Wp > 0x7fffffffLL) return CDFO_EINVAL;   // 32-bit offsets inside a field
  if (!aligned16(out) || (dtype == CDFO_MV_F32 && (reinterpret_cast<uintptr_t>(mv) & 3u) != 0)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 0, (double)K * (56.0 * Hp * Wp + 12.0 * H * W));
  switch (dtype) {
    case CDFO_MV_F32: launch_seq_flows<float>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_F64: launch_seq_flows<double>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_F16: launch_seq_flows<_Float16>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_BF16: launch_seq_flows<bf16_t>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I8: launch_seq_flows<signed char>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_U8: launch_seq_flows<unsigned char>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I16: launch_seq_flows<short>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I32: launch_seq_flows<int>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    case CDFO_MV_I64: launch_seq_flows<long long>(mv, T, H, W, i0, K, Hp, Wp, out, st); break;
    default: return CDFO_EINVAL;
  }
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_gather_frames(const void* src, int n_src, const int* idx, int n_dst, long long frame_bytes, void* dst, void* stream) {
  if (!src || !dst || !idx || n_src <= 0 || n_dst <= 0 || n_dst > 65535 || frame_bytes <= 0 || frame_bytes % 16 ||
      frame_bytes > 0x7ffffff0LL)
    return CDFO_EINVAL;
  if (!aligned16(src) || !aligned16(dst) || (reinterpret_cast<uintptr_t>(idx) & 3u)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long n16 = frame_bytes / 16;
  // enough workgroups over all frames to fill the chip a few times, at most one thread per 16-byte vector
  long long bx = (n16 + 1023) / 1024;
  const long long want = cdiv(8 * (cdfo_num_cus() > 0 ? cdfo_num_cus() : 256), n_dst);
  if (bx > want) bx = want;
  if (bx < 1) bx = 1;
  CdfoProfScope prof(st, KID_LAYOUT, 0, 2.0 * (double)n_dst * (double)frame_bytes);
  hipLaunchKernelGGL(gather_frames_kernel, dim3((unsigned)bx, (unsigned)n_dst), dim3(256), 0, st,
                     static_cast<const unsigned char*>(src), static_cast<u32x4*>(dst), idx, n_src, (int)frame_bytes);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_flow_warp_frames(const float* bank, int ldi, int n_bank, const int* idx, const float* mv, long long mv_kstride,
                                     int slot0, int G, int K, int H, int W, int C, float* out, int ldo, void* stream) {
  if (!bank || !idx || !mv || !out || n_bank <= 0 || G <= 0 || K <= 0 || (long long)G * K > 65535 || slot0 < 0 || mv_kstride < 0 ||
      H <= 0 || W <= 0 || C <= 0 || C % 4 || ldi % 4 || ldo % 4 || ldi < C || ldo < C)
    return CDFO_EINVAL;
  if ((long long)H * W * (C / 4) + 8192LL * 256 > 0x7fffffffLL) return CDFO_EINVAL;          // 32-bit thread index inside an image
  if (!aligned16(bank) || !aligned16(out) || (reinterpret_cast<uintptr_t>(idx) & 3u) || (reinterpret_cast<uintptr_t>(mv) & 3u))
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n = G * K;
  // flow_warp's grid: at most 8192 workgroups in all, at most one thread per 16-byte vector of an image
  int bx = cdiv(8192, n);
  const int need = cdiv(H * W * (C / 4), 256);
  if (bx > need) bx = need;
  CdfoProfScope prof(st, KID_FLOW_WARP, 0, 4.0 * (2 * C + 2) * (double)n * H * W);
  hipLaunchKernelGGL(flow_warp_frames_kernel, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, st, bank, ldi, n_bank, idx, mv, mv_kstride,
                     slot0, K, H, W, C, out, ldo);
  CDFO_LAUNCH_CHECK();
  return 0;
}
