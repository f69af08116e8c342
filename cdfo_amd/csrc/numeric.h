// Device numerics that more than one translation unit needs: the split-precision conversions, the Philox generator, the
// DPP row sum, the DCN power-of-two scale and the workgroup's 64-bit integer and fp64 sums.  Two of them are contracts BETWEEN kernels
// (philox4x32_10: inference and training draw the same noise for one seed; pow2_scale: both DCN paths scale alike), so each
// has exactly one definition here.
#pragma once
#include "common.h"

// two fp32 -> one register of two bf16 (round to nearest even), a in the low half
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  const __bf16 ha = (__bf16)a, hb = (__bf16)b;
  return (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
}
__device__ __forceinline__ float bf16_round(float a) { return (float)(__bf16)a; }
// four fp32 -> packed bf16 hi and packed bf16 lo = bf16(v - hi): the two operands of the split-bf16 (3-pass) products
__device__ __forceinline__ void split4_bf16(const f32x4 v, u32x2& hi, u32x2& lo) {
  hi[0] = pack_bf16(v[0], v[1]);
  hi[1] = pack_bf16(v[2], v[3]);
  lo[0] = pack_bf16(v[0] - bf16_round(v[0]), v[1] - bf16_round(v[1]));
  lo[1] = pack_bf16(v[2] - bf16_round(v[2]), v[3] - bf16_round(v[3]));
}

// eight fp32 -> the MFMA operand registers of their bf16 hi and lo parts
__device__ __forceinline__ void split8_bf16(const f32x4 v0, const f32x4 v1, unsigned (&hi)[4], unsigned (&lo)[4]) {
  hi[0] = pack_bf16(v0[0], v0[1]); hi[1] = pack_bf16(v0[2], v0[3]);
  hi[2] = pack_bf16(v1[0], v1[1]); hi[3] = pack_bf16(v1[2], v1[3]);
  lo[0] = pack_bf16(v0[0] - bf16_round(v0[0]), v0[1] - bf16_round(v0[1]));
  lo[1] = pack_bf16(v0[2] - bf16_round(v0[2]), v0[3] - bf16_round(v0[3]));
  lo[2] = pack_bf16(v1[0] - bf16_round(v1[0]), v1[1] - bf16_round(v1[1]));
  lo[3] = pack_bf16(v1[2] - bf16_round(v1[2]), v1[3] - bf16_round(v1[3]));
}

// Two fp32 values -> packed fp16 hi (round to nearest) and packed fp16 lo = fp16(v - hi), four instructions per pair:
// v_cvt_pk_f16_f32, two v_fma_mix_f32 (f32 * 1.0 - f16 -> f32: the exact remainder, the fp16 operand read straight from its
// half of the packed register), v_cvt_pk_f16_f32.  hipcc emits cvt_f32_f16 + sub per element for the plain C expression (six
// per pair) and folds a source-level fma back into it; the attention kernel is bound by its vector instructions (DESIGN section
// 5.2), so the form is spelled out.  Full-register results only: the three-instruction form through v_fma_mixlo_f16 /
// v_fma_mixhi_f16 writes half registers, and gfx950 needs a wait state between such a write and the next vector read of the
// register, which hipcc cannot insert around inline assembly (measured: wrong window-attention results where the consumer
// followed directly).
__device__ __forceinline__ void split_pair_f16(float a, float b, unsigned& hi, unsigned& lo) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const h2 hv = {(_Float16)a, (_Float16)b};
  hi = __builtin_bit_cast(unsigned, hv);
  float ra, rb;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(ra) : "v"(a), "v"(hi));
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(rb) : "v"(b), "v"(hi));
  const h2 lv = {(_Float16)ra, (_Float16)rb};
  lo = __builtin_bit_cast(unsigned, lv);
}

// Philox4x32-10 (Salmon et al., SC'11): counter-based generator, 4 x 32 random bits per (counter, key).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__device__ __forceinline__ float row16_sum(float v) {     // sum over the 16 lanes of a DPP row, result in every lane
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));  // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));  // row_ror:8
  return v;
}

// the DCN kernels' power-of-two scale from the bit pattern of a maximum m >= 0: m * s in (8, 16]; the exponent is clamped so that
// neither s nor 1 / s leaves the fp32 range
__device__ __forceinline__ float pow2_scale(unsigned max_bits) {
  const float m = __uint_as_float(max_bits);
  return m > 0.f ? exp2f(fminf(fmaxf(4.f - ceilf(log2f(m)), -100.f), 100.f)) : 1.f;
}

// exact 64-bit integer sum over a workgroup of whole waves (sh: one slot per wave); the total is valid in thread 0
__device__ __forceinline__ long long block_sum_i64(long long v, long long* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), o, 64);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  long long t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
  return t;   // valid in thread 0
}

// the fp64 sum over a workgroup of whole waves (sh: one slot per wave, free again on return); the total is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
  __syncthreads();
  return t;   // valid in thread 0
}

// Ground truth of the evaluation kernels (finish.hip, chroma.hip): the samples x0 .. x0+3 of a row (x0 a multiple of 4) as one word,
// sample e in bits [8 sizeof(T) e, 8 sizeof(T) (e + 1)).  words = 0: nothing is read here (the caller reads per element); 1: aligned
// 32-bit words (for 16-bit samples two of them, the second, samples x0+2 and x0+3, only where the caller wants it: it may lie beyond
// the row's pitch); 2, 16-bit samples only: one aligned 64-bit word.
template <typename T> struct gt_word;
template <> struct gt_word<unsigned char> { typedef unsigned type; };
template <> struct gt_word<unsigned short> { typedef unsigned long long type; };

__device__ __forceinline__ unsigned load_gt_word(const unsigned char* p, int words, bool) {
  return words ? *reinterpret_cast<const unsigned*>(p) : 0u;
}
__device__ __forceinline__ unsigned long long load_gt_word(const unsigned short* p, int words, bool second) {
  if (words == 2) return *reinterpret_cast<const unsigned long long*>(p);
  if (words == 0) return 0ull;
  const unsigned* q = reinterpret_cast<const unsigned*>(p);
  return (unsigned long long)q[0] | (second ? (unsigned long long)q[1] << 32 : 0ull);
}

// (q - r)^2 of two samples as a 64-bit addend.  8-bit: the signed 32-bit product.  16-bit: 65535^2 = 4294836225 does not fit a signed
// 32-bit product; the unsigned one holds it (the square of a wrapped negative difference is the same number modulo 2^32).
template <typename T> __device__ __forceinline__ long long sqdiff(unsigned q, unsigned r) {
  if constexpr (sizeof(T) == 1) {
    const int df = (int)q - (int)r;
    return df * df;
  } else {
    const unsigned df = q - r;
    return (long long)(unsigned long long)(df * df);
  }
}
