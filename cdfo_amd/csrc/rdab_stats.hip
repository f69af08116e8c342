// The mask statistics of LLongRangAttention (arch/SIDECVSR_our.py:2148-2152, 2200-2203) straight from the one-channel residual
// map: per image the channel sums over all output pixels of
//     relu(conv_du_re.2(du0)),   du0 = relu(stencil9(rms; w0, b0)) on the H x W grid and ZERO outside it,
// conv_du_re.2 the 3x3 / stride 2 / pad 2 convolution 64 -> 64 and (w0, b0) = conv_du_re.0 o conv_expand_rms (K.compose_stem_1x1).
// Neither du0 (64 channels per pixel, 64 x the bytes of the map) nor the convolution's result, whose only reader is the global
// average pool, reaches memory.  Per output pixel and tap of conv_du_re.2 the 64 du0 values are themselves a matrix product, the
// "stem K block": one 16-wide k-step whose pixel operand is built in registers from the 5x5 window of the map around the output
// pixel -- the tap's nine neighbours, a constant 1 (the bias column) and zeros, all zero where the tap's centre lies outside the
// map -- against the 64 x 10 matrix [w0 | b0].  Its accumulators hold, per lane, 8 channels of each 16-channel k-step of the
// convolution that follows (in the accumulator's own channel order, which the weight image's k order matches), so ReLU and the bf16
// hi | lo split turn them into that product's operand without leaving the lane.  Both products run as three bf16 MFMA passes
// (hi*lo + lo*hi + hi*hi, fp32 accumulation) like the exact-mode convolution this replaces: the mean feeds a hard 0.5 threshold.
//
// A 512-thread workgroup holds the convolution's whole weight image (hi | lo, 144 KB) in LDS and walks (image, chunk) items; a
// wave owns 32 output pixels at a time (MFMA columns; rows = channels).  Sums are kept per lane over the item, reduced over lanes
// and waves in a fixed order and stored in cdfo_chan_sum_partial's layout [B][nchunk][64]: every slot is written, no atomics, equal
// inputs give equal bits.
#include "numeric.h"

namespace {

constexpr int RS_THREADS = 512;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_KSTEPS = 36;                               // 9 taps x 4 k-steps of 16 input channels
constexpr int RS_W2_HALF = RS_KSTEPS * 2 * 64 * 16;         // bytes of the weight image's hi (or lo) part
constexpr int RS_B2_OFF = 2 * RS_W2_HALF;                   // conv_du_re.2's bias, 64 floats
constexpr int RS_RED_OFF = RS_B2_OFF + 64 * 4;              // the waves' sums [RS_WAVES][64]
constexpr int RS_LDS = RS_RED_OFF + RS_WAVES * 64 * 4;

struct rs_args {
  const float* img; int Bi; long long s_b, s_g;             // image m's plane at img + (m % Bi) s_b + (m / Bi) s_g
  const float* w0; const float* b0;                         // the composed stencil [64][9], [64]
  const void* w2; const float* b2;                          // pack_rdab_stats' image, [64]
  int B, H, W, Ho, Wo, nchunk;
  float* partial;
};

union rs_frag { unsigned u[4]; bf16x8_t v; };

// split8_bf16 with the two conversions of a pair in one v_cvt_pk_bf16_f32 and the remainder taken from the packed register's halves
// (six instructions per pair; the kernel is bound by its vector instructions)
__device__ __forceinline__ void rs_split8(const f32x4 v0, const f32x4 v1, unsigned (&hi)[4], unsigned (&lo)[4]) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 v = i < 2 ? f32x2{v0[2 * i], v0[2 * i + 1]} : f32x2{v1[2 * i - 4], v1[2 * i - 3]};
    hi[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
    const f32x2 rem = {v[0] - __uint_as_float(hi[i] << 16), v[1] - __uint_as_float(hi[i] & 0xffff0000u)};
    lo[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(rem, bf16x2_t));
  }
}

__global__ __launch_bounds__(RS_THREADS) void rdab_stats_kernel(rs_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned char* sWh = smem;
  const unsigned char* sWl = smem + RS_W2_HALF;
  float* sB2 = reinterpret_cast<float*>(smem + RS_B2_OFF);
  float* sRed = reinterpret_cast<float*>(smem + RS_RED_OFF);

  // ---- the static weights, once per workgroup: the convolution's image -> LDS; the stem block's matrix -> registers, row = channel
  // 32 ni + r, this lane's 8 k-values: taps 0..7 in half 0; tap 8, the bias and zeros in half 1
  for (int i = tid; i < 2 * RS_W2_HALF / 16; i += RS_THREADS)
    reinterpret_cast<u32x4*>(smem)[i] = reinterpret_cast<const u32x4*>(a.w2)[i];
  if (tid < 64) sB2[tid] = a.b2[tid];
  rs_frag s0h[2], s0l[2];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int ch = 32 * ni + r;
    f32x4 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v0[j] = h ? (j == 0 ? a.w0[ch * 9 + 8] : (j == 1 ? a.b0[ch] : 0.f)) : a.w0[ch * 9 + j];
      v1[j] = h ? 0.f : a.w0[ch * 9 + 4 + j];
    }
    split8_bf16(v0, v1, s0h[ni].u, s0l[ni].u);
  }
  __syncthreads();

  const int H = a.H, W = a.W, Wo = a.Wo;
  const int Pout = a.Ho * Wo;
  const int per = (Pout + a.nchunk - 1) / a.nchunk;
  for (int item = blockIdx.x; item < a.B * a.nchunk; item += gridDim.x) {
    const int b = item / a.nchunk, chunk = item - b * a.nchunk;
    const int p0 = chunk * per, p1 = p0 + per < Pout ? p0 + per : Pout;
    const float* ip = a.img + (long long)(b % a.Bi) * a.s_b + (long long)(b / a.Bi) * a.s_g;
    // the 5x5 window of the map around output pixel p: rows 2 oy - 3 .. 2 oy + 1, zero beyond the map (a pixel beyond the image
    // has rows beyond it too)
    auto load_win = [&](int p, float (&win)[5][5]) {
      const int oy = p / Wo, ox = p - oy * Wo;
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const int yy = 2 * oy - 3 + i, xx = 2 * ox - 3 + j;
          // every lane loads from a clamped, valid address and selects afterwards: 25 loads in flight, no branches
          const int yc = yy < 0 ? 0 : (yy < H ? yy : H - 1), xc = xx < 0 ? 0 : (xx < W ? xx : W - 1);
          const float v = ip[yc * W + xc];
          win[i][j] = (yy == yc && xx == xc) ? v : 0.f;
        }
    };
    float cs[32];        // acc layout: cs[16 no + e] = channel 32 no + 8 (e >> 2) + 4 h + (e & 3), summed over this lane's pixels
#pragma unroll
    for (int e = 0; e < 32; ++e) cs[e] = 0.f;
    float win[5][5];
    int t0 = p0 + wave * 32;
    if (t0 < p1) load_win(t0 + r, win);
    for (; t0 < p1; t0 += RS_WAVES * 32) {
      const int p = t0 + r, tn = t0 + RS_WAVES * 32;
      const int oy = p / Wo, ox = p - oy * Wo;
      f32x16 acc[2];
#pragma unroll
      for (int no = 0; no < 2; ++no)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[no][e] = 0.f;
      // the stem block of tap t: du0 before its ReLU, 64 channels x 32 pixels
      auto stem = [&](int t, f32x16 (&du)[2]) {
        const int yy = 2 * oy - 2 + t / 3, xx = 2 * ox - 2 + t % 3;
        const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;       // else du0 = 0: every k-value zero, the constant included
        f32x4 x0, x1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo_half = win[t / 3 + j / 3][t % 3 + j % 3];
          const float hi_half = j == 0 ? win[t / 3 + 2][t % 3 + 2] : (j == 1 ? 1.f : 0.f);
          x0[j] = inside ? (h ? hi_half : lo_half) : 0.f;
          x1[j] = (inside && !h) ? win[t / 3 + (4 + j) / 3][t % 3 + (4 + j) % 3] : 0.f;
        }
        rs_frag xh, xl;
        rs_split8(x0, x1, xh.u, xl.u);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
          for (int e = 0; e < 16; ++e) du[ni][e] = 0.f;
          du[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s0h[ni].v, xl.v, du[ni], 0, 0, 0);
          du[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s0l[ni].v, xh.v, du[ni], 0, 0, 0);
          du[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s0h[ni].v, xh.v, du[ni], 0, 0, 0);
        }
      };
      f32x16 du[2][2];       // two taps in flight: the next tap's stem block runs in the matrix pipe under this tap's conversions
      stem(0, du[0]);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        if (t < 8) stem(t + 1, du[(t + 1) & 1]);
        // ---- conv_du_re.2's four k-steps of this tap: k-step (ni, half) = du[ni][8 half .. + 7], i.e. this lane's channels
        // 32 ni + 16 half + 8 (q >> 2) + 4 h + (q & 3), q = 0..7 (pack_rdab_stats orders the weights' k the same way)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            f32x4 v0, v1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              v0[q] = fmaxf(du[t & 1][ni][8 * half + q], 0.f);
              v1[q] = fmaxf(du[t & 1][ni][8 * half + 4 + q], 0.f);
            }
            rs_frag ph, pl;
            rs_split8(v0, v1, ph.u, pl.u);
            const int wrow = (((t * 2 + ni) * 2 + half) * 2 + h) * 64 + r;
#pragma unroll
            for (int no = 0; no < 2; ++no) {
              const bf16x8_t wh = *reinterpret_cast<const bf16x8_t*>(sWh + (wrow + no * 32) * 16);
              const bf16x8_t wl = *reinterpret_cast<const bf16x8_t*>(sWl + (wrow + no * 32) * 16);
              acc[no] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, pl.v, acc[no], 0, 0, 0);
              acc[no] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ph.v, acc[no], 0, 0, 0);
              acc[no] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ph.v, acc[no], 0, 0, 0);
            }
          }
        __builtin_amdgcn_sched_barrier(0);      // keeps the scheduler from starting every tap's stem block at once (96 registers each)
      }
      // the next tile's window is requested now: its loads return behind the epilogue and the other waves' products
      if (tn < p1) load_win(tn + r, win);
      // bias, ReLU, and the pixel joins its lane's sums unless it lies beyond the chunk
      const bool valid = p < p1;
#pragma unroll
      for (int no = 0; no < 2; ++no)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const f32x4 bb = *reinterpret_cast<const f32x4*>(sB2 + no * 32 + 8 * jj + 4 * h);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float t = fmaxf(acc[no][4 * jj + k] + bb[k], 0.f);
            cs[16 * no + 4 * jj + k] += valid ? t : 0.f;
          }
        }
    }
    // ---- the item's sums: over the 32 pixel lanes of each half, then over the waves, both in a fixed order
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      float v = cs[e];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (r == 0) sRed[wave * 64 + (e >> 4) * 32 + 8 * ((e & 15) >> 2) + 4 * h + (e & 3)] = v;
    }
    __syncthreads();
    if (tid < 64) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < RS_WAVES; ++w) s += sRed[w * 64 + tid];
      a.partial[((long long)b * a.nchunk + chunk) * 64 + tid] = s;
    }
    __syncthreads();      // sRed is free for the next item
  }
}

}  // namespace

extern "C" int cdfo_rdab_stats(const float* img, int Bi, long long s_b, long long s_g, const float* w0, const float* b0,
                               const void* w2_packed, const float* b2, int B, int H, int W, int nchunk, float* partial,
                               void* stream) {
  if (B <= 0 || Bi <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || nchunk <= 0 || s_b < 0 || s_g < 0) return CDFO_EINVAL;
  if ((long long)H * W >= (1ll << 30) || (long long)B * nchunk >= (1ll << 31)) return CDFO_EINVAL;   // 32-bit pixel indices
  if (!aligned16(w2_packed)) return CDFO_EALIGN;
  const int cus = cdfo_num_cus();
  if (cus <= 0) return (int)hipErrorInvalidDevice;
  rs_args a;
  a.img = img; a.Bi = Bi; a.s_b = s_b; a.s_g = s_g;
  a.w0 = w0; a.b0 = b0; a.w2 = w2_packed; a.b2 = b2;
  a.B = B; a.H = H; a.W = W; a.Ho = H / 2 + 1; a.Wo = W / 2 + 1; a.nchunk = nchunk;
  a.partial = partial;
  static CdfoAttrOnce once;
  const hipError_t e = cdfo_set_max_lds(once, reinterpret_cast<const void*>(rdab_stats_kernel), RS_LDS);
  if (e != hipSuccess) return (int)e;
  const long long items = (long long)B * nchunk;
  const double px = (double)B * a.Ho * a.Wo;
  CdfoProfScope prof(static_cast<hipStream_t>(stream), KID_CHAN_SUM, 2.0 * (576 + 9 * 16) * 64 * px, 4.0 * (double)B * H * W);
  hipLaunchKernelGGL(rdab_stats_kernel, dim3((unsigned)(items < cus ? items : cus)), dim3(RS_THREADS), RS_LDS,
                     static_cast<hipStream_t>(stream), a);
  CDFO_LAUNCH_CHECK();
  return 0;
}
