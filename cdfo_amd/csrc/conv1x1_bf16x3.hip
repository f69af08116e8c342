// 1x1 convolution as a streaming GEMM on the bf16 matrix cores in split-bf16 (3-pass, fp32-grade) arithmetic.
//
// The exact-fp32 MFMA kernel (conv_igemm.hip) spends as long in v_mfma_f32_32x32x2_f32 as in HBM traffic once the
// output is 128-256 channels wide (64->192 qkv: 2.4 TB/s algorithmic); a 1x1 convolution moves 4*(Cin+Cout) bytes per
// pixel for 2*Cin*Cout FLOP, so it should be a pure HBM stream.  Here one workgroup owns 128 consecutive pixels of one
// image: the 64-channel input block is read ONCE (fp32 -> bf16 hi/lo while staging, optional fused per-pixel LayerNorm)
// and kept in LDS for every 64-wide output-channel block; weights come straight from the fp32 packing
// [Cin/4][CoutP][4] of cdfo_pack_conv_weight (also the per-image folded attention weights) and are split on the fly.
// Three bf16 MFMA passes (a_hi*w_hi + a_lo*w_hi + a_hi*w_lo) cost ~1/5 of the exact-fp32 MFMA time.
//
// Same argument block / epilogue contract as cdfo_conv_igemm (bias, LeakyReLU/ReLU, two residuals, plain or 2x
// pixel-shuffle store); every source must be a multiple of 64 channels wide.  Replaces the 1x1 convolutions of the
// CVSR_V8 path (qkv, project_out folded, input_conv, fuse, fusion_out, down.0 / up.0, tsa_fusion, upconv1/2).
#include "numeric.h"
#include "plane_chunk.h"      // pc_plane: the optional plane operand, streaming form only
#include "image_map.h"
#include <type_traits>

namespace {

constexpr int PXT = 128;                        // pixels per workgroup (4 waves x one 32-pixel MFMA M tile)
constexpr int PIXB = 80;                        // LDS bytes per staged pixel and 16-channel chunk: 32 hi | 32 lo | 16 pad
constexpr int A_CHUNK = PXT * PIXB;             // 10,240
constexpr int A_BYTES = 4 * A_CHUNK;            // 40,960: one 64-channel K block
constexpr int W_HALF = 4 * 2 * 64 * 16;         // 8,192: [chunk][k-half][64 cout][8 bf16]
constexpr int W_BYTES = 2 * W_HALF;             // hi | lo
constexpr int EPI_RS = 68;                      // floats per pixel row in the epilogue transpose (64 + 4)
constexpr int EPI_BYTES = 4 * 32 * EPI_RS * 4;  // 34,816
constexpr int MAXCB = 4;                        // up to 256 output channels


__device__ __forceinline__ void split_store(unsigned char* dst_hi, int lo_delta, const f32x4 v) {
  u32x2 hi, lo;
  split4_bf16(v, hi, lo);
  *reinterpret_cast<u32x2*>(dst_hi) = hi;
  *reinterpret_cast<u32x2*>(dst_hi + lo_delta) = lo;
}

// MAP form: where the images of every source lie (image_map.h).  A block of its own that only the MAP instantiation takes: the other
// forms' kernel arguments, and with them their instructions, stay what they were
struct c1_args_map : cdfo_conv_args {
  im_map src_map[CDFO_MAXSRC];
};

// NCB: number of 64-wide output-channel blocks (1..4).
// TAPS (CDFO_STORE_TAPS9, upconv2 of arch.py:4474-4476 only): instead of the pixel-shuffled 64-channel HR feature map,
// store for every HR pixel the nine per-tap channel sums t_k = sum_c w_last[c][k] * act(y)[c] of the 3x3 conv_last that
// follows: 36 bytes per HR pixel instead of 256 (the 4.3 GB HR map is never written nor read back).  The sums are a second
// matrix product in the epilogue (round 2; as sixteen-lane DPP reductions they were 1 150 vector instructions per lane and
// output block and made the launch 2.06 ms long).
// MAP: the sources' images lie where c1_args_map.src_map says (residuals and the result stay dense)
template <int NCB, bool TAPS = false, bool MAP = false>
__global__ __launch_bounds__(256, 2) void conv1x1_bf16x3_kernel(std::conditional_t<MAP, c1_args_map, cdfo_conv_args> a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[A_BYTES + W_BYTES];
  static_assert(EPI_BYTES <= A_BYTES + W_BYTES, "the epilogue transpose reuses the staging buffers");
  unsigned char* sA = smem;
  unsigned char* sW = smem + A_BYTES;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, r = lane & 31;
  const int b = blockIdx.y;
  const long long P = (long long)a.H * a.W;
  const long long p0 = (long long)blockIdx.x * PXT;          // first pixel of this tile inside image b
  const long long gp0 = (long long)b * P + p0;               // global pixel index
  const float* wbase = a.w + (long long)b * a.w_bstride;

  f32x16 acc[NCB][2];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[cb][ni][e] = 0.f;

  const int a_off = (wave * 32 + r) * PIXB + h * 16;   // this lane's pixel record inside a chunk
  const int b_off = (h * 64 + r) * 16;
  const bool do_ln = a.ln_gamma != nullptr;

  const int nkb = a.Cin >> 6;
  int s_idx = 0, s_base = 0;
  for (int kb = 0; kb < nkb; ++kb) {
    const int ch0 = kb * 64;
    while (ch0 >= s_base + a.cs[s_idx]) { s_base += a.cs[s_idx]; ++s_idx; }
    const float* src = a.src[s_idx] + (ch0 - s_base);
    const int ld = a.ld[s_idx];
    // MAP: image b of this source starts im_offset floats behind its first image, not b P ld -- the loads below index from there,
    // and stay inside the image (pixels beyond it are clamped to its first)
    if constexpr (MAP) src += im_offset(a.src_map[s_idx], b) - (long long)b * P * ld;
    __syncthreads();   // previous K block's MFMAs are done with sA / sW
    // ---- stage 128 pixels x 64 channels: 8 float4 per thread, all loads first
    f32x4 v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int idx = tid + 256 * s, px = idx >> 4, q = idx & 15;
      const long long pp = p0 + px < P ? gp0 + px : gp0;          // clamped: always loaded, zeroed below
      v[s] = *reinterpret_cast<const f32x4*>(src + pp * ld + q * 4);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int idx = tid + 256 * s, px = idx >> 4, q = idx & 15;
      f32x4 t = v[s];
      if (do_ln) {   // per-pixel LayerNorm over the 64 channels held by 16 consecutive lanes (arch.py:1169-1185)
        float sm = (t[0] + t[1]) + (t[2] + t[3]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sm += __shfl_xor(sm, o, 64);
        const f32x4 d = t - sm * (1.f / 64.f);
        float sq = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        const float rstd = 1.f / sqrtf(sq * (1.f / 64.f) + 1e-5f);
        t = d * rstd * *reinterpret_cast<const f32x4*>(a.ln_gamma + q * 4) + *reinterpret_cast<const f32x4*>(a.ln_beta + q * 4);
      }
      if (p0 + px >= P) t = f32x4{0.f, 0.f, 0.f, 0.f};
      split_store(sA + (q >> 2) * A_CHUNK + px * PIXB + (q & 3) * 8, 32, t);
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      if (cb > 0) __syncthreads();   // the previous output block's MFMAs are done with sW
      // ---- weights of (K block kb, output block cb) from the fp32 packing, split to bf16 hi/lo: 4 float4 per thread
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int idx = tid + 256 * s, kg = idx >> 6, n = idx & 63;   // kg: group of 4 input channels inside the block
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wbase + ((long long)(kb * 16 + kg) * a.CoutP + cb * 64 + n) * 4);
        const int c = kg >> 2, hh = (kg >> 1) & 1, j0 = (kg & 1) * 4;
        split_store(sW + ((c * 2 + hh) * 64 + n) * 16 + j0 * 2, W_HALF, wv);
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8_t ah = *reinterpret_cast<const bf16x8_t*>(sA + c * A_CHUNK + a_off);
        const bf16x8_t al = *reinterpret_cast<const bf16x8_t*>(sA + c * A_CHUNK + a_off + 32);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(sW + (c * 2 * 64 + ni * 32) * 16 + b_off);
          const bf16x8_t bl = *reinterpret_cast<const bf16x8_t*>(sW + W_HALF + (c * 2 * 64 + ni * 32) * 16 + b_off);
          acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[cb][ni], 0, 0, 0);
          acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[cb][ni], 0, 0, 0);
          acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[cb][ni], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: wave-private LDS transpose, then 16-byte rows: +bias -> act -> +res1 -> +res2 -> store
  __syncthreads();
  float* wl = reinterpret_cast<float*>(smem) + wave * 32 * EPI_RS;
  const float slope = a.act == CDFO_ACT_NONE ? 1.f : (a.act == CDFO_ACT_LRELU ? 0.1f : 0.f);
  const int c4 = lane & 15, pr = lane >> 4;                  // 16 float4 columns, 4 pixel rows per wave-instruction
  const bool plain = a.store_mode == CDFO_STORE_PLAIN;
  const int cq = a.Cout >> 2;
  // TAPS: the nine tap sums are a second matrix product, taps[k][pixel] = sum_c w_last[c][k] * act(y)[pixel][c] -- A = w_last^T
  // (row = tap, zero rows 9..31), split fp16 hi | lo once per lane: lane (r = tap, h) holds channels 16 s + 8 h .. + 7
  typedef _Float16 c1_f16x8 __attribute__((ext_vector_type(8)));
  c1_f16x8 twh[TAPS ? 4 : 1], twl[TAPS ? 4 : 1];
  if (TAPS) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float wv = r < 9 ? a.res2[(16 * s4 + 8 * h + j) * 9 + r] : 0.f;      // a.res2 = conv_last.weight as [64][9]
        twh[s4][j] = (_Float16)wv;
        twl[s4][j] = (_Float16)(wv - (float)twh[s4][j]);
      }
  }
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) wl[((e & 3) + 8 * (e >> 2) + 4 * h) * EPI_RS + ni * 32 + r] = acc[cb][ni][e];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (TAPS) {
      // block cb = sub-pixel (dy, dx) = (cb >> 1, cb & 1) of the pixel-shuffled map.  B = act(y + bias) of this wave's 32
      // pixels (lane (r = pixel, h): channels 16 s + 8 h .. + 7 from the transposed tile), scaled per PIXEL by a power of two
      // into fp16's range (a column of the product may carry its own scale) and split hi | lo: hi*hi + lo*hi + hi*lo.
      f32x4 y[4][2];
      float amax = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int ch = 16 * s4 + 8 * h + 4 * q;
          f32x4 t = *reinterpret_cast<const f32x4*>(wl + r * EPI_RS + ch);
          if (a.bias) t += *reinterpret_cast<const f32x4*>(a.bias + cb * 64 + ch);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            t[k] = fmaxf(t[k], 0.f) + slope * fminf(t[k], 0.f);
            amax = fmaxf(amax, fabsf(t[k]));
          }
          y[s4][q] = t;
        }
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));            // the pixel's other 32 channels sit in lane ^ 32
      int ex = 0;
      if (amax > 0.f && amax < INFINITY) frexpf(amax, &ex);
      ex = ex < -100 ? -100 : (ex > 100 ? 100 : ex);
      const float sc = ldexpf(1.f, 14 - ex), inv = ldexpf(1.f, ex - 14);
      f32x16 tacc;
#pragma unroll
      for (int e = 0; e < 16; ++e) tacc[e] = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        c1_f16x8 yh, yl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = y[s4][j >> 2][j & 3] * sc;
          yh[j] = (_Float16)v;
          yl[j] = (_Float16)(v - (float)yh[j]);
        }
        tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(twl[s4], yh, tacc, 0, 0, 0);
        tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(twh[s4], yl, tacc, 0, 0, 0);
        tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(twh[s4], yh, tacc, 0, 0, 0);
      }
      // lane (pixel r, h): registers 0..3 = taps 4 h .. 4 h + 3, register 4 = tap 8 (h = 0)
      const long long pin = p0 + wave * 32 + r;
      if (pin < P) {
        const int oy = (int)(pin / a.W), ox = (int)(pin - (long long)oy * a.W);
        const long long opix = ((long long)b * 2 * a.H + 2 * oy + (cb >> 1)) * (2 * a.W) + 2 * ox + (cb & 1);
        float* op = a.out + opix * a.ldo;
        const f32x4 t4 = {tacc[0] * inv, tacc[1] * inv, tacc[2] * inv, tacc[3] * inv};
        if ((a.ldo & 3) == 0) *reinterpret_cast<f32x4*>(op + 4 * h) = t4;
        else { op[4 * h] = t4[0]; op[4 * h + 1] = t4[1]; op[4 * h + 2] = t4[2]; op[4 * h + 3] = t4[3]; }
        if (h == 0) op[8] = tacc[4] * inv;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    const int n = cb * 64 + c4 * 4;
    const bool nok = n < a.Cout;
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && nok) bias = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int i = it * 4 + pr;                              // pixel inside this wave's M tile
      f32x4 t = *reinterpret_cast<const f32x4*>(wl + i * EPI_RS + c4 * 4) + bias;
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = fmaxf(t[k], 0.f) + slope * fminf(t[k], 0.f);
      const long long pin = p0 + wave * 32 + i;               // pixel inside the image
      if (!nok || pin >= P) continue;
      const long long pix = (long long)b * P + pin;
      if (plain) {
        if (a.res1) t += *reinterpret_cast<const f32x4*>(a.res1 + pix * a.ldr1 + n);
        if (a.res2) t += *reinterpret_cast<const f32x4*>(a.res2 + pix * a.ldr2 + n);
        *reinterpret_cast<f32x4*>(a.out + pix * a.ldo + n) = t;
      } else {  // 2x pixel shuffle; packed channel order is (dy,dx,c)
        const int sub = n / cq, cc = n - sub * cq;
        const int oy = (int)(pin / a.W), ox = (int)(pin - (long long)oy * a.W);
        const long long opix = ((long long)b * 2 * a.H + 2 * oy + (sub >> 1)) * (2 * a.W) + 2 * ox + (sub & 1);
        *reinterpret_cast<f32x4*>(a.out + opix * a.ldo + cc) = t;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

// conv1x1_stream.hip: the persistent LDS-DMA streaming form (plain store, CoutP <= 128, weights + rings within LDS)
int cdfo_conv1x1_stream_try(const cdfo_conv_args& a, hipStream_t st, const pc_plane* plane = nullptr, const im_map* maps = nullptr);
extern "C" int cdfo_layernorm64_cp16hl(const float* in, int ldi, const float* gamma, const float* beta, int B, long long P,
                                       void* out, void* stream);

// pl != null: cdfo_conv1x1_bf16x3_plane; maps != null: cdfo_conv1x1_bf16x3_map
static int conv1x1_bf16x3(const cdfo_conv_args* pa, const pc_plane* pl, void* stream, const im_map* maps = nullptr) {
  const cdfo_conv_args& a = *pa;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.nsrc < 1 || a.nsrc > CDFO_MAXSRC || a.B <= 0 || a.ks != 1 || a.stride != 1 || a.pad != 0) return CDFO_EINVAL;
  if (a.act == CDFO_ACT_SIGMOID || a.tap_mask || a.src_f16 || a.out_f16 || a.res_up2 || a.src_plane_wrap) return CDFO_EINVAL;
  // out2_cp16 here = a second output: with ln_gamma / ln_beta LayerNorm64 of the RESULT as fp16 hi | lo planes [B][8][P][16]; without
  // them the result itself as one fp16 chunk-planar tensor [B][4][P][16] (what cdfo_to_cp16 would make of `out`)
  const bool ln_out = a.out2_cp16 != nullptr;
  const bool copy_out = ln_out && !a.ln_gamma && !a.ln_beta;
  if (ln_out && (a.Cout != 64 || a.CoutP != 64 || a.store_mode != CDFO_STORE_PLAIN || a.ldo < 64 || !aligned16(a.out2_cp16))) return CDFO_EINVAL;
  if (ln_out && !copy_out && (!a.ln_gamma || !a.ln_beta || !aligned16(a.ln_gamma) || !aligned16(a.ln_beta))) return CDFO_EINVAL;
  int csum = 0;
  for (int s = 0; s < a.nsrc; ++s) {
    if (a.cs[s] <= 0 || a.cs[s] % 64 || a.ld[s] % 4 || a.ld[s] < a.cs[s]) return CDFO_EINVAL;
    if (!aligned16(a.src[s])) return CDFO_EALIGN;
    csum += a.cs[s];
  }
  if (csum != a.Cin || a.CoutP % 64 || a.CoutP > 64 * MAXCB || a.CoutP < a.Cout || a.Cout <= 0 || a.Cout % 4) return CDFO_EINVAL;
  if (a.Ho != a.H || a.Wo != a.W) return CDFO_EINVAL;
  if (a.store_mode == CDFO_STORE_S2D || (a.store_mode == CDFO_STORE_SHUFFLE2 && (a.Cout % 16 || a.res1 || a.res2))) return CDFO_EINVAL;
  if (a.store_mode == CDFO_STORE_TAPS9 && (a.Cout != 256 || a.CoutP != 256 || a.res1 || !a.res2 || a.ldo < 9 || a.w_bstride)) return CDFO_EINVAL;
  const bool taps = a.store_mode == CDFO_STORE_TAPS9;
  if (!aligned16(a.w) || a.w_bstride % 4 || (!taps && a.ldo % 4) || !aligned16(a.out) || (a.bias && !aligned16(a.bias))) return CDFO_EALIGN;
  if ((a.res1 && (a.ldr1 % 4 || !aligned16(a.res1))) || (!taps && a.res2 && (a.ldr2 % 4 || !aligned16(a.res2)))) return CDFO_EALIGN;
  if (!ln_out && a.ln_gamma && !(a.nsrc == 1 && a.cs[0] == 64 && a.ln_beta && aligned16(a.ln_gamma) && aligned16(a.ln_beta))) return CDFO_EINVAL;
  const long long P = (long long)a.H * a.W;
  if (a.res2_pixscale && (!a.res2 || taps)) return CDFO_EINVAL;
  if (pl) {
    // one more operand, stencil9 of a one-channel plane, inside the product: only the streaming kernel has that form, and a launch
    // outside its contract is an error (the caller materialises the operand instead)
    if (!pl->base || !pl->w || pl->Bi <= 0 || pl->s_b < 0 || pl->s_g < 0 || taps) return CDFO_EINVAL;
    if (!aligned16(pl->w) || pl->w_bstride % 4 || (a.chan_sum_out && !aligned16(a.chan_sum_out))) return CDFO_EALIGN;
    const int r = cdfo_conv1x1_stream_try(a, st, pl, maps);
    return r == 1 ? 0 : (r == 0 ? CDFO_EINVAL : r);
  }
  if (maps) {
    // mapped operands: the streaming kernel where the launch is inside its contract (there also for the residuals), else the
    // one-tile-per-workgroup kernel below for a plain 64-channel product of mapped sources.  Anything else is an error: the caller
    // materialises the operand instead (cdfo_conv1x1_map_ok says which, without a launch)
    if (taps || ln_out || a.ln_gamma || a.res2_pixscale || a.store_mode != CDFO_STORE_PLAIN || a.CoutP != 64) return CDFO_EINVAL;
    if (a.chan_sum_out && (a.Cout != 64 || a.chan_sum_slots <= 0 || !aligned16(a.chan_sum_out))) return CDFO_EINVAL;
    // (with the streaming kernel switched off the dense launch would run on another kernel: no mapped form then)
    static const bool use_stream = cdfo_switch("CDFO_CONV1X1_STREAM", 1) != 0;
    if (!use_stream) return CDFO_EINVAL;
    const int r = cdfo_conv1x1_stream_try(a, st, nullptr, maps);
    if (r == 1) return 0;
    if (r != 0) return r;
    if (a.chan_sum_out || maps[CDFO_MAXSRC].Bi || maps[CDFO_MAXSRC + 1].Bi) return CDFO_EINVAL;
    c1_args_map am{};
    static_cast<cdfo_conv_args&>(am) = a;
    for (int i = 0; i < a.nsrc; ++i) am.src_map[i] = maps[i].Bi ? maps[i] : im_dense(a.B, P, a.ld[i]);
    dim3 grid((unsigned)((P + PXT - 1) / PXT), a.B);
    const double px = (double)a.B * P;
    CdfoProfScope prof(st, KID_CONV1, 2.0 * px * a.Cout * a.Cin, 4.0 * (px * a.Cout + px * a.Cin + (double)a.Cin * a.Cout));
    hipLaunchKernelGGL((conv1x1_bf16x3_kernel<1, false, true>), grid, dim3(256), 0, st, am);
    CDFO_LAUNCH_CHECK();
    return 0;
  }
  if (a.chan_sum_out) {
    // channel sums of the result: from the streaming kernel's epilogue, else (outside its contract / switched off) a pass of their own
    if (a.Cout != 64 || a.CoutP != 64 || a.store_mode != CDFO_STORE_PLAIN || a.chan_sum_slots <= 0 || !aligned16(a.chan_sum_out)) return CDFO_EINVAL;
    static const bool use_stream = cdfo_switch("CDFO_CONV1X1_STREAM", 1) != 0;
    if (use_stream && !ln_out) {
      const int r = cdfo_conv1x1_stream_try(a, st);
      if (r == 1) return 0;
      if (r != 0) return r;
    }
    cdfo_conv_args plain = a;
    plain.chan_sum_out = nullptr; plain.chan_sum_slots = 0;
    const int rc = cdfo_conv1x1_bf16x3(&plain, stream);
    if (rc) return rc;
    return cdfo_chan_sum_partial(a.out, a.ldo, a.B, P, a.chan_sum_slots, a.chan_sum_out, stream);
  }
  if (ln_out) {
    // the streaming kernel normalises in its epilogue; outside its contract: the convolution, then a LayerNorm pass
    const int r = cdfo_conv1x1_stream_try(a, st);
    if (r == 1) return 0;
    if (r != 0) return r;
    if (a.res2_pixscale) return CDFO_EINVAL;      // only the streaming form scales its residual
    cdfo_conv_args plain = a;
    plain.out2_cp16 = nullptr; plain.ln_gamma = nullptr; plain.ln_beta = nullptr;
    const int rc = cdfo_conv1x1_bf16x3(&plain, stream);
    if (rc) return rc;
    if (copy_out) return cdfo_to_cp16(a.out, a.ldo, a.B, P, 64, a.out2_cp16, stream);
    return cdfo_layernorm64_cp16hl(a.out, a.ldo, a.ln_gamma, a.ln_beta, a.B, P, a.out2_cp16, stream);
  }
  {
    static const bool use_stream = cdfo_switch("CDFO_CONV1X1_STREAM", 1) != 0;   // developer A/B switch
    static const bool taps_stream = cdfo_switch("CDFO_TAPS_STREAM", 1) != 0;   // developer A/B switch
    if (use_stream && (!taps || taps_stream)) {
      const int r = cdfo_conv1x1_stream_try(a, st);
      if (r == 1) return 0;
      if (r != 0) return r;
    }
  }
  if (a.res2_pixscale) return CDFO_EINVAL;        // only the streaming form scales its residual
  dim3 grid((unsigned)((P + PXT - 1) / PXT), a.B);
  const double px = (double)a.B * P;
  CdfoProfScope prof(st, KID_CONV1, 2.0 * px * a.Cout * a.Cin, 4.0 * (px * a.Cout + px * a.Cin + (double)a.Cin * a.Cout));
  if (taps) {
    hipLaunchKernelGGL((conv1x1_bf16x3_kernel<4, true>), grid, dim3(256), 0, st, a);
    CDFO_LAUNCH_CHECK();
    return 0;
  }
  switch (a.CoutP / 64) {
    case 1: hipLaunchKernelGGL(conv1x1_bf16x3_kernel<1>, grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(conv1x1_bf16x3_kernel<2>, grid, dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(conv1x1_bf16x3_kernel<3>, grid, dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(conv1x1_bf16x3_kernel<4>, grid, dim3(256), 0, st, a); break;
  }
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_conv1x1_bf16x3(const cdfo_conv_args* pa, void* stream) { return conv1x1_bf16x3(pa, nullptr, stream); }

extern "C" int cdfo_conv1x1_bf16x3_plane(const cdfo_conv_args* pa, const float* plane, int plane_Bi, long long plane_sb,
                                         long long plane_sg, const float* plane_w, long long plane_w_bstride, void* stream) {
  const pc_plane pl = {plane, plane_Bi, plane_sb, plane_sg, 0, plane_w, plane_w_bstride};      // (W: the argument block's)
  return conv1x1_bf16x3(pa, &pl, stream);
}

// cdfo_conv1x1_bf16x3 (plane == null) / cdfo_conv1x1_bf16x3_plane on operands read through image maps (image_map.h).  maps: CDFO_MAXSRC + 2
// triples (Bi, s_b, s_g) -- entry i for source i, entries CDFO_MAXSRC and CDFO_MAXSRC + 1 for res1 and res2; Bi == 0: that operand is dense.  Image b of
// a mapped operand starts at its pointer + (b % Bi) s_b + (b / Bi) s_g floats.  64-channel plain results only; same bits as on the
// dense copies of those images.
extern "C" int cdfo_conv1x1_bf16x3_map(const cdfo_conv_args* pa, const long long* maps, const float* plane, int plane_Bi,
                                       long long plane_sb, long long plane_sg, const float* plane_w, long long plane_w_bstride,
                                       void* stream) {
  if (!pa || !maps) return CDFO_EINVAL;
  im_map m[CDFO_MAXSRC + 2];
  for (int i = 0; i < CDFO_MAXSRC + 2; ++i) {
    m[i] = im_map{(int)maps[3 * i], maps[3 * i + 1], maps[3 * i + 2]};
    if (maps[3 * i] < 0 || maps[3 * i] > 0x7fffffff || (m[i].Bi && !im_map_ok(m[i]))) return CDFO_EINVAL;
  }
  if (!plane) return conv1x1_bf16x3(pa, nullptr, stream, m);
  const pc_plane pl = {plane, plane_Bi, plane_sb, plane_sg, 0, plane_w, plane_w_bstride};
  return conv1x1_bf16x3(pa, &pl, stream, m);
}

// Whether cdfo_conv1x1_bf16x3_map takes a launch of this form (pure host arithmetic): Cin input channels in 64-channel sources, 64 output
// channels; with_plane / with_res / with_csum: a plane operand, a mapped residual or the channel sums, which only the streaming kernel has
extern "C" int cdfo_conv1x1_map_ok(int Cin, int with_plane, int with_res, int with_csum) {
  if (Cin <= 0 || Cin % 64 || Cin / 64 > CDFO_MAXSRC * 4) return 0;
  if (!with_plane && cdfo_switch("CDFO_CONV1X1_STREAM", 1) == 0) return 0;
  const int w_bytes = st_weight_bytes(Cin / 64, 1);      // the ring stages left beside the weights, as cdfo_conv1x1_stream_try counts them
  const int ns = with_plane ? (ST_MAX_LDS - w_bytes - pc_weight_bytes(1)) / (4 * (ST_STAGE + PC_SLOT)) : (ST_MAX_LDS - w_bytes) / (4 * ST_STAGE);
  const bool stream_fits = ns >= 3;
  return stream_fits || !(with_plane || with_res || with_csum) ? 1 : 0;
}
