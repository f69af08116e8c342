// Device and host pieces of the persistent LDS-DMA stream kernels (conv1x1_stream.hip: the 1x1 convolution and the alignment
// statistics; attention.hip: the prior-fusion attention's input_conv + mask kernel): a 256-thread workgroup per CU walks a contiguous
// range of 128-pixel tiles, each wave owns 32 pixels of a tile and a private ring of 8 KB LDS stages that it fills itself.
#pragma once
#include "lds_dma.h"
#include "numeric.h"

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_STAGE = 8192;                 // 32 pixels x 64 channels x 4 B
constexpr int ST_MAXNS = 4;
constexpr int ST_MAX_LDS = 160 * 1024 - 256;   // dynamic LDS a workgroup of these kernels may ask for

// An item has landed when at most the 8 * (younger items in flight) youngest DMA pieces are outstanding (pieces retire in order
// among themselves; stores and older requests in flight only make the wait more conservative)
__device__ __forceinline__ void st_wait_landed(long long younger) {
  if (younger >= 2) wait_vm<16>();
  else if (younger == 1) wait_vm<8>();
  else wait_vm<0>();
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
constexpr int st_weight_bytes(int nkb, int ncb) { return 2 * (nkb * 4 * 2 * ncb * 64 * 16) + ncb * 64 * 4; }
constexpr int st_lds_bytes(int nkb, int ncb, int ns) { return st_weight_bytes(nkb, ncb) + 4 * ns * ST_STAGE; }

// `once`: the call site's static table, one per kernel instantiation.  Returns 0 or the hipError_t.
template <class KernelPtr, class Args>
int st_launch(KernelPtr kernel, CdfoAttrOnce& once, int grid, int lds, hipStream_t st, const Args& s) {
  const hipError_t e = cdfo_set_max_lds(once, reinterpret_cast<const void*>(kernel), ST_MAX_LDS);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(ST_THREADS), lds, st, s);
  return (int)hipGetLastError();
}

}  // namespace
