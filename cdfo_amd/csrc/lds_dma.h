// The hand-written pieces of the LDS-DMA kernels that hipcc cannot check: the `buffer_load ... lds` issue blocks, the buffer
// descriptor they read through, the counted waits behind them and the MFMA row permutation that the weight packers and the
// epilogues agree on.  Each is a contract between kernels (or with the hardware), so each has exactly one definition here.
#pragma once
#include "common.h"

// ---- buffer descriptors
// word 3 of a raw buffer descriptor on gfx950: DATA_FORMAT (bits 15-18) = 4 = one 32-bit element, everything else zero -- raw
// byte addressing, no swizzle, range-checked against word 2 (NUM_RECORDS = bytes).  The value of every descriptor in the library,
// hand-filled or made by __builtin_amdgcn_make_buffer_rsrc.
constexpr int BUFFER_RSRC_WORD3 = 0x00020000;

// descriptor of `bytes` bytes at `base`; an access at or beyond `bytes` loads zero / stores nothing
__device__ __forceinline__ i32x4 lds_dma_rsrc(const void* base, unsigned bytes) {
  const unsigned long long p = reinterpret_cast<unsigned long long>(base);
  i32x4 r;
  r[0] = (int)(unsigned)p;
  r[1] = (int)(unsigned)(p >> 32);
  r[2] = (int)bytes;
  r[3] = BUFFER_RSRC_WORD3;
  return r;
}
// the same where the compiler cannot prove base / bytes wave-uniform (they are: the caller says so): words read from lane 0
__device__ __forceinline__ i32x4 lds_dma_rsrc_uniform(const void* base, unsigned bytes) {
  const unsigned long long p = reinterpret_cast<unsigned long long>(base);
  i32x4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)p);
  r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32));
  r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
  r[3] = BUFFER_RSRC_WORD3;
  return r;
}
// word 2 alone.  (conv1x1_stream.hip builds its descriptors with size 0 and sizes them here: where the size is computed, between
// the readfirstlanes of the base and its own, decides the kernels' instruction order)
__device__ __forceinline__ void lds_dma_rsrc_resize_uniform(i32x4& r, unsigned bytes) { r[2] = __builtin_amdgcn_readfirstlane((int)bytes); }

// ---- LDS-DMA issue: N pieces of 64 lanes x 16 bytes (1 KiB) into consecutive kilobytes of LDS.  Lane l of piece k writes LDS
// bytes lds + 1024 k + 16 l from (descriptor base + voff[k] + soff).  The rules, for every member of the family:
//  * rsrc, soff and lds must be wave-uniform values that the compiler can keep in SGPRs ("s" operands): kernel arguments,
//    blockIdx expressions or readfirstlane results.
//  * All pieces of a call are ONE asm statement: m0 (the LDS destination base) is live from the first piece to the last, the
//    compiler neither preserves it around a statement nor accepts it as a clobber, so it is saved in `keep` and restored.
//  * `s_nop 4` opening the block: an SGPR operand fresh from v_readfirstlane needs five wait states before a buffer instruction
//    reads it as descriptor or soffset, and hipcc pads nothing inside (or for) an asm string.
//  * `s_nop 0` behind every write of m0: one wait state between a scalar write of m0 and the LDS-DMA instruction that reads it.
//  * A lane whose voff (+ soff) is at or beyond the descriptor's size writes ZEROS to its LDS bytes: callers give lanes outside the
//    image 0x80000000 (the convolutions' zero padding) or shrink the descriptor's size (tiles beyond the stream's end).
//  * hipcc does not count these loads: the caller waits with wait_vm<N>() below before anyone reads the LDS bytes.
// What differs between the callers stays visible in the call: the piece count, an SGPR soffset (lds_dma) against the literal 0
// (lds_dma0), and 16 bytes per lane against 4 (lds_dma0_dword).
#define LDS_DMA_OPEN "s_nop 4\n\ts_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[lds]\n\ts_nop 0\n\t"
#define LDS_DMA_PIECE(LOAD, K, SOFF) LOAD " %[v" #K "], %[rsrc], " SOFF " offen lds\n\t"
#define LDS_DMA_NEXT "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
#define LDS_DMA_CLOSE "s_mov_b32 m0, %[keep]"
#define LDS_DMA_PIECES1(LOAD, S) LDS_DMA_PIECE(LOAD, 0, S)
#define LDS_DMA_PIECES5(LOAD, S) \
  LDS_DMA_PIECES1(LOAD, S) LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 1, S) LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 2, S) LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 3, S) \
  LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 4, S)
#define LDS_DMA_PIECES6(LOAD, S) LDS_DMA_PIECES5(LOAD, S) LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 5, S)
#define LDS_DMA_PIECES8(LOAD, S) LDS_DMA_PIECES6(LOAD, S) LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 6, S) LDS_DMA_NEXT LDS_DMA_PIECE(LOAD, 7, S)
#define LDS_DMA_VOFF1 [v0] "v"(voff[0])
#define LDS_DMA_VOFF5 LDS_DMA_VOFF1, [v1] "v"(voff[1]), [v2] "v"(voff[2]), [v3] "v"(voff[3]), [v4] "v"(voff[4])
#define LDS_DMA_VOFF6 LDS_DMA_VOFF5, [v5] "v"(voff[5])
#define LDS_DMA_VOFF8 LDS_DMA_VOFF6, [v6] "v"(voff[6]), [v7] "v"(voff[7])
#define LDS_DMA_SOFF_SGPR , [soff] "s"(soff)
#define LDS_DMA_SOFF_NONE
// one statement: N pieces of instruction LOAD with soffset text SOFF (SOFF_OPERAND: its operand, or nothing), then the clobbers
#define LDS_DMA_ASM(N, LOAD, SOFF, SOFF_OPERAND, ...)                           \
  asm volatile(LDS_DMA_OPEN LDS_DMA_PIECES##N(LOAD, SOFF) LDS_DMA_CLOSE         \
               : [keep] "=&s"(keep)                                             \
               : LDS_DMA_VOFF##N, [rsrc] "s"(rsrc), [lds] "s"(lds) SOFF_OPERAND \
               : __VA_ARGS__)

// SGPR soffset, the first N entries of voff (the five-piece producer waves of conv3x3_c64_wsq_kernel hold six).  s_add_u32 writes
// scc: clobbered by every form of more than one piece.
template <int N, int M>
__device__ __forceinline__ void lds_dma(const unsigned (&voff)[M], i32x4 rsrc, unsigned soff, unsigned lds) {
  static_assert(N <= M && (N == 1 || N == 5 || N == 6), "piece counts in use");
  unsigned keep;
  if constexpr (N == 1) LDS_DMA_ASM(1, "buffer_load_dwordx4", "%[soff]", LDS_DMA_SOFF_SGPR, "memory");
  else if constexpr (N == 5) LDS_DMA_ASM(5, "buffer_load_dwordx4", "%[soff]", LDS_DMA_SOFF_SGPR, "memory", "scc");
  else LDS_DMA_ASM(6, "buffer_load_dwordx4", "%[soff]", LDS_DMA_SOFF_SGPR, "memory", "scc");
}
__device__ __forceinline__ void lds_dma1(unsigned voff1, i32x4 rsrc, unsigned soff, unsigned lds) {
  const unsigned voff[1] = {voff1};
  lds_dma<1>(voff, rsrc, soff, lds);
}
// soffset 0 (the descriptor is based at the wave's own data), eight pieces
__device__ __forceinline__ void lds_dma0(const unsigned (&voff)[8], i32x4 rsrc, unsigned lds) {
  unsigned keep;
  LDS_DMA_ASM(8, "buffer_load_dwordx4", "0", LDS_DMA_SOFF_NONE, "memory", "scc");
}
// soffset 0, ONE DWORD per lane: lane l writes LDS bytes lds + 4 l
__device__ __forceinline__ void lds_dma0_dword(unsigned voff1, i32x4 rsrc, unsigned lds) {
  const unsigned voff[1] = {voff1};
  unsigned keep;
  LDS_DMA_ASM(1, "buffer_load_dword", "0", LDS_DMA_SOFF_NONE, "memory");
}

// ---- counted waits.  N = how many of the wave's youngest vector-memory (vm) or LDS / scalar-memory (lgkm) operations may
// still be outstanding; the call site says what is being counted.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_vm_lgkm0() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }

// ---- the MFMA row -> output channel permutation of the 32x32 kernels' weight images (packers, bias tables and epilogues agree on it).
// MFMA row m = 8j + 4h + k of a 32-channel block holds channel (j>>1)*16 + h*8 + (j&1)*4 + k, so that a lane's accumulators
// (fixed h; j, k = register index) are 8 consecutive channels of each 16-channel chunk.  n = row position over any number of
// 32-channel blocks, which keep their order: n & ~31 (where n < 64, as in the 64-channel kernels that wrote n & 32, the same number).
// The formula is a macro only for conv3x3_ring.hip, which expands it in place: inlined from the function, hipcc swaps two operands
// of one v_or3_b32 there, and a refactor changes no instruction.  Everyone else calls the function.
#define MFMA_ROW_CHANNEL(n) \
  (((n) & ~31) + ((((n) & 31) >> 4) & 1) * 16 + ((((n) & 31) >> 2) & 1) * 8 + ((((n) & 31) >> 3) & 1) * 4 + ((n) & 3))
__device__ __forceinline__ int mfma_row_channel(int n) { return MFMA_ROW_CHANNEL(n); }
