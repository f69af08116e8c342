// Input building for live sequence inference (cdfo_amd/live.py::LiveSR): frames and their coding priors are pushed one at a time
// into rings of cap = chunk + 6 frames (frame t in slot t mod cap) that keep the files' own sample types; a chunk's inputs are
// built out of the rings by two launches.
//
//   cdfo_live_planes    every fp32 plane a chunk reads from the sample rings, in one launch: the [K,7] windows of the LR frames, the
//                       residual maps and the unfiltered frames, and the LR / partition / residual planes of the E frames the chunk
//                       extracts: sample / peak (partition maps / 255) as ONE correctly rounded fp32 division, zero padded from
//                       H x W to Hp x Wp.  Bit for bit what StreamingSR's whole-sequence planes followed by cdfo_gather_frames give.
//   cdfo_seq_flows_ring cdfo_seq_flows reading the fp32 ring of motion fields, with the sequence's end possibly not known yet
//                       (T_known = 0: no end rule applies and T > 1).  The per-pixel body is seq_flows.h's, shared with sequence.hip.
//
// Both are streaming kernels in sequence.hip's form: grid y over output planes / centre frames with the source slot wave-uniform,
// 16-byte stores, no LDS, no atomics.  A frame's rows are not 16-byte aligned (27 samples per row is a legal frame), so the samples
// are read in element loads through a buffer descriptor bounded to the frame: an offset outside the frame returns zero, and a slot
// outside [0, cap) gets a descriptor of zero bytes (cdfo_gather_frames' contract: a plane of zeros), never an out-of-range read.
#include "common.h"
#include "seq_flows.h"

namespace {

struct LivePlanesArgs {
  const unsigned char* lr;       // [cap][H][W] samples of `sb` bytes
  const unsigned char* ufs;      // the same
  const unsigned char* pms;      // [cap][H][W] uint8
  const unsigned char* rms;      // [cap][H][W] fp32
  const int* table;              // win_frame[7K], win_prior[7K], new_frame[E], new_prior[E]
  float *x, *r, *u, *lr_new, *p_new, *r_new;
  int sb, cap, H, W, K, E, Hp, Wp;
  float peak;
};

// element `e` of a frame of `ES`-byte elements as fp32; outside the descriptor's range the load returns zero
template <int ES> __device__ __forceinline__ float load_sample(__amdgpu_buffer_rsrc_t r, int e);
template <> __device__ __forceinline__ float load_sample<1>(__amdgpu_buffer_rsrc_t r, int e) {
  return (float)__builtin_amdgcn_raw_buffer_load_b8(r, e, 0, 0);
}
template <> __device__ __forceinline__ float load_sample<2>(__amdgpu_buffer_rsrc_t r, int e) {
  return (float)__builtin_amdgcn_raw_buffer_load_b16(r, e * 2, 0, 0);
}
template <> __device__ __forceinline__ float load_sample<4>(__amdgpu_buffer_rsrc_t r, int e) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, e * 4, 0, 0));
}

// one output plane [Hp][Wp] = frame / div, zero padded; a thread writes four consecutive pixels of a row with one 16-byte store
template <int ES>
__device__ __forceinline__ void plane_from_frame(const unsigned char* __restrict__ ring, int slot, int cap, int H, int W, int Hp, int Wp,
                                                 float div, float* __restrict__ dst) {
  const bool ok = slot >= 0 && slot < cap;
  const int frame_bytes = H * W * ES;
  const __amdgpu_buffer_rsrc_t rs = frame_rsrc(ring + (long long)(ok ? slot : 0) * frame_bytes, ok ? frame_bytes : 0);
  const int w4 = Wp >> 2;
  const int total = Hp * w4;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
    const int y = t / w4, x = (t - y * w4) << 2;
    f32x4 q;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // a pixel of the padding is not loaded at all: its offset may lie inside the frame (the next row) or beyond its end
      const bool inside = y < H && x + p < W;
      q[p] = inside ? __fdiv_rn(load_sample<ES>(rs, y * W + x + p), div) : 0.f;
    }
    *reinterpret_cast<f32x4*>(dst + (long long)y * Wp + x) = q;
  }
}

// grid (x: workgroups striding over a plane's Hp * Wp / 4 threads; y: output plane).  Planes in the order x, r, u (7K each),
// lr_new, p_new, r_new (E each); which group, which table entry and which ring depend on blockIdx.y alone: wave-uniform
__global__ __launch_bounds__(256) void live_planes_kernel(LivePlanesArgs a) {
  const int n7 = 7 * a.K;
  int j = blockIdx.y;
  const long long plane = (long long)a.Hp * a.Wp;
  const unsigned char* ring;
  float* dst;
  int entry, es;
  float div = a.peak;
  if (j < 3 * n7) {
    const int g = j / n7;
    j -= g * n7;
    ring = g == 0 ? a.lr : g == 1 ? a.rms : a.ufs;
    dst = g == 0 ? a.x : g == 1 ? a.r : a.u;
    es = g == 1 ? 4 : a.sb;
    entry = (g == 0 ? 0 : n7) + j;
  } else {
    j -= 3 * n7;
    const int g = j / a.E;
    j -= g * a.E;
    ring = g == 0 ? a.lr : g == 1 ? a.pms : a.rms;
    dst = g == 0 ? a.lr_new : g == 1 ? a.p_new : a.r_new;
    es = g == 0 ? a.sb : g == 1 ? 1 : 4;
    if (g == 1) div = 255.0f;
    entry = 2 * n7 + (g == 0 ? 0 : a.E) + j;
  }
  if (!dst) return;                                          // an output the caller did not ask for
  const int slot = a.table[entry];
  dst += (long long)j * plane;
  if (es == 1) plane_from_frame<1>(ring, slot, a.cap, a.H, a.W, a.Hp, a.Wp, div, dst);
  else if (es == 2) plane_from_frame<2>(ring, slot, a.cap, a.H, a.W, a.Hp, a.Wp, div, dst);
  else plane_from_frame<4>(ring, slot, a.cap, a.H, a.W, a.Hp, a.Wp, div, dst);
}

// cdfo_seq_flows' grid (x: Hp * Wp / 4 threads; y: centre frame); the centre's entry lives in slot entry mod cap of the ring
__global__ __launch_bounds__(256) void seq_flows_ring_kernel(const float* __restrict__ ring, int cap, int T_known, int H, int W, int i0,
                                                             int Hp, int Wp, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int w4 = Wp >> 2;
  if (t >= Hp * w4) return;
  const int y = t / w4, x = (t - y * w4) << 2;
  const int i = i0 + (int)blockIdx.y;
  const int entry = T_known == 1 ? 0 : (i > 1 ? i : 1);      // the field of frame 0 is read from entry 1 (test_LD_22_FPS.py:168)
  // an open stream has no end yet: the end rules are judged against a length that no centre reaches
  const int Tn = T_known > 0 ? T_known : 0x7fffffff;
  seq_flows_pixels<float>(ring + (long long)(entry % cap) * (H * W * 3), H, W, i, Tn, Hp, Wp, y, x,
                          out + (long long)blockIdx.y * 14 * Hp * Wp);
}

}  // namespace

extern "C" int cdfo_live_planes(const void* lr, const void* ufs, const unsigned char* pms, const float* rms, int sample_bytes, int cap,
                                int H, int W, const int* table, int K, int E, int Hp, int Wp, int peak, float* x, float* r, float* u,
                                float* lr_new, float* p_new, float* r_new, void* stream) {
  if (!lr || !ufs || !pms || !rms || !table || !x || !u || (sample_bytes != 1 && sample_bytes != 2) || cap <= 0 || H <= 0 || W <= 0 ||
      K <= 0 || E < 0 || Hp < H || Wp < W || Wp % 4 || peak < 1 || peak > 65535 || (sample_bytes == 1 && peak > 255))
    return CDFO_EINVAL;
  if (E > 0 && (!lr_new || !p_new)) return CDFO_EINVAL;
  if (21LL * K + 3LL * E > 65535) return CDFO_EINVAL;                                        // grid y
  // 32-bit offsets inside a frame (its fp32 form is the widest) and inside a plane; the grid-stride index stays below 2^31
  if ((long long)H * W * 4 > 0x7fffffffLL || (long long)Hp * Wp + 4096LL * 256 * 4 > 0x7fffffffLL) return CDFO_EINVAL;
  const float* outs[6] = {x, r, u, lr_new, p_new, r_new};
  for (const float* o : outs)
    if (!aligned16(o)) return CDFO_EALIGN;
  if ((reinterpret_cast<uintptr_t>(lr) | reinterpret_cast<uintptr_t>(ufs)) & (uintptr_t)(sample_bytes - 1)) return CDFO_EALIGN;
  if ((reinterpret_cast<uintptr_t>(rms) | reinterpret_cast<uintptr_t>(table)) & 3u) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  LivePlanesArgs a;
  a.lr = static_cast<const unsigned char*>(lr);
  a.ufs = static_cast<const unsigned char*>(ufs);
  a.pms = pms;
  a.rms = reinterpret_cast<const unsigned char*>(rms);
  a.table = table;
  a.x = x, a.r = r, a.u = u, a.lr_new = lr_new, a.p_new = p_new, a.r_new = r_new;
  a.sb = sample_bytes, a.cap = cap, a.H = H, a.W = W, a.K = K, a.E = E, a.Hp = Hp, a.Wp = Wp;
  a.peak = (float)peak;
  const int planes = 21 * K + 3 * E;
  // enough workgroups over all planes to fill the chip a few times, at most one thread per 16-byte vector of a plane
  int bx = cdiv(Hp * (Wp / 4), 256);
  const int want = cdiv(8 * (cdfo_num_cus() > 0 ? cdfo_num_cus() : 256), planes);
  if (bx > want) bx = want;
  if (bx > 4096) bx = 4096;
  if (bx < 1) bx = 1;
  const double px = (double)H * W, out_planes = (r ? 21.0 : 14.0) * K + (r_new ? 3.0 : 2.0) * E;
  CdfoProfScope prof(st, KID_LAYOUT, 0, 4.0 * out_planes * Hp * Wp + out_planes * px * sample_bytes);
  hipLaunchKernelGGL(live_planes_kernel, dim3((unsigned)bx, (unsigned)planes), dim3(256), 0, st, a);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_seq_flows_ring(const float* ring, int cap, int H, int W, int i0, int K, int T_known, int Hp, int Wp, float* out,
                                   void* stream) {
  if (!ring || !out || cap <= 0 || H <= 0 || W <= 0 || K <= 0 || K > 65535 || i0 < 0 || T_known < 0 || Hp < H || Wp < W || Wp % 4)
    return CDFO_EINVAL;
  if (T_known > 0 && (long long)i0 + K > T_known) return CDFO_EINVAL;
  if ((long long)i0 + K > 0x7ffffff0LL) return CDFO_EINVAL;
  if ((long long)H * W * 3 * 8 > 0x7fffffffLL || (long long)Hp * Wp > 0x7fffffffLL) return CDFO_EINVAL;   // 32-bit offsets inside a field
  if (!aligned16(out) || (reinterpret_cast<uintptr_t>(ring) & 3u) != 0) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 0, (double)K * (56.0 * Hp * Wp + 12.0 * H * W));
  hipLaunchKernelGGL(seq_flows_ring_kernel, dim3(cdiv(Hp * (Wp / 4), 256), K), dim3(256), 0, st, ring, cap, T_known, H, W, i0, Hp, Wp, out);
  CDFO_LAUNCH_CHECK();
  return 0;
}
