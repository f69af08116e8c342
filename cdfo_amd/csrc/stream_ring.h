// Device and host pieces of the persistent LDS-DMA stream kernels (conv1x1_stream.hip: the 1x1 convolution and the alignment
// statistics; attention.hip: the prior-fusion attention's input_conv + mask kernel): a 256-thread workgroup per CU walks a contiguous
// range of 128-pixel tiles, each wave owns 32 pixels of a tile and a private ring of 8 KB LDS stages that it fills itself.
#pragma once
#include "numeric.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_STAGE = 8192;                 // 32 pixels x 64 channels x 4 B
constexpr int ST_MAXNS = 4;
constexpr int ST_MAX_LDS = 160 * 1024 - 256;   // dynamic LDS a workgroup of these kernels may ask for

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// eight 1 KiB pieces of one stage: lane l of piece k writes LDS bytes lds + 1024 k + 16 l from (buffer base + voff[k])
__device__ __forceinline__ void st_dma8(const unsigned (&voff)[8], i32x4 rsrc, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %10\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %1, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %2, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %3, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %4, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %5, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %6, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %7, %9, 0 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %8, %9, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "v"(voff[4]), "v"(voff[5]), "v"(voff[6]), "v"(voff[7]),
        "s"(rsrc), "s"(lds)
      : "memory", "scc");
}

// one dword per lane: lane l writes LDS bytes lds + 4 l from (buffer base + voff)
__device__ __forceinline__ void st_dma1(unsigned voff, i32x4 rsrc, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_nop 4\n\t"
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "buffer_load_dword %1, %2, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(rsrc), "s"(lds)
      : "memory", "scc");
}

// An item has landed when at most the 8 * (younger items in flight) youngest DMA pieces are outstanding (pieces retire in order
// among themselves; stores and older requests in flight only make the wait more conservative)
__device__ __forceinline__ void st_wait_landed(long long younger) {
  if (younger >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (younger == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// MFMA row m of a 32-channel block holds channel (m>>4)*16 + ((m>>2)&1)*8 + ((m>>3)&1)*4 + (m&3) (see conv3x3_ws.hip):
// a lane's accumulator registers then are 8 consecutive channels of each 16-channel group
__device__ __forceinline__ int st_chan_of_row(int n) {
  const int m = n & 31;
  return (n & ~31) + ((m >> 4) & 1) * 16 + ((m >> 2) & 1) * 8 + ((m >> 3) & 1) * 4 + (m & 3);
}

// ---- host side
// the stream of B images of P pixels as 128-pixel tiles, and the persistent grid over the calling thread's CUs; false: no device
inline bool st_tiling(int B, long long P, int& tiles_per_image, long long& tiles, int& grid) {
  tiles_per_image = (int)((P + 127) / 128);
  tiles = (long long)B * tiles_per_image;
  const int cus = cdfo_num_cus();
  grid = (int)(tiles < cus ? tiles : cus);
  return cus > 0;
}
// the kernels' LDS map: split weights hi | lo and the bias in front of the rings
inline int st_weight_bytes(int nkb, int ncb) { return 2 * (nkb * 4 * 2 * ncb * 64 * 16) + ncb * 64 * 4; }
inline int st_lds_bytes(int nkb, int ncb, int ns) { return st_weight_bytes(nkb, ncb) + 4 * ns * ST_STAGE; }

// `once`: the call site's static table, one per kernel instantiation.  Returns 0 or the hipError_t.
template <class KernelPtr, class Args>
int st_launch(KernelPtr kernel, CdfoAttrOnce& once, int grid, int lds, hipStream_t st, const Args& s) {
  const hipError_t e = cdfo_set_max_lds(once, reinterpret_cast<const void*>(kernel), ST_MAX_LDS);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(ST_THREADS), lds, st, s);
  return (int)hipGetLastError();
}

}  // namespace
