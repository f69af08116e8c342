// Prior-fusion attention `LLongRangAttention` (arch/SIDECVSR_our.py:2179-2249): residual-driven hard mask, row /
// column long-range attention and 8x8 window attention -- without ever writing a WxW / HxH / 64x64 score map to HBM.
//
//   rdab_prep   : Gumbel-softmax hard mask (arch.py:2168-2195) from the injected uniform noise; q,v split of the
//                 128-channel input_conv output; sparse_q = conv1x9_over_channels(mask*q), v' = conv1x9(v)
//                 (directW1_conv, arch.py:2216-2219); window query (1-mask)*q (arch.py:2235-2238).
//   colconv9    : directH1_conv, the 9-tap conv along H on sparse_q (arch.py:2225).
//   seq_attn    : softmax(Q Q^T) V over a row, a column or an 8x8 window, one query per lane, keys streamed through
//                 wave-uniform (scalar) loads, online softmax in registers.
#include "plane_chunk.h"
#include "image_map.h"
#include <type_traits>

namespace {

typedef _Float16 attn_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 attn_f16x4 __attribute__((ext_vector_type(4)));

constexpr int ZS = 65;  // LDS pitch for the [pixel][channel] logits (conflict-free both ways)
constexpr int QS = 72;  // 4 zero floats on both sides of the 64 channels for the 9-tap channel conv

// RNG: the uniform draws of gumbel_softmax (arch.py:2169, torch.rand_like + "redraw while any == 0") are generated here
// instead of being read: u = (24 random bits + 0.5) * 2^-24 lies strictly inside (0, 1), element (image b, channel c,
// pixel p) takes word c & 3 of Philox(counter = (p, b, c >> 2, draw), key = seed).  noise_out (optional): the drawn
// values, [B][64][P], for callers that replay the forward elsewhere (parity tests).
template <bool RNG>
__global__ __launch_bounds__(256) void rdab_prep_kernel(const float* __restrict__ xq, int ldx,  // [.,128]: q | v
                                                        const float* __restrict__ vmax,         // [B][64]
                                                        const float* __restrict__ noise,        // [B][64][P] (NCHW)
                                                        const float* __restrict__ wW, const float* __restrict__ bW,
                                                        long long P, float* __restrict__ sq, int lds_,
                                                        float* __restrict__ vrow, int ldv, float* __restrict__ qwin,
                                                        int ldw, unsigned long long seed, unsigned draw,
                                                        float* __restrict__ noise_out,
                                                        const unsigned long long* __restrict__ seed_dev) {
  __shared__ float z[64 * ZS];
  __shared__ float mq[64 * QS];
  __shared__ float vv[64 * QS];
  __shared__ float ev[64];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * 64;  // P % 64 == 0, so the 64 pixels share one image
  const long long b = p0 / P, pin = p0 - b * P;
  // softmax_c(v_c + g_c) with g = -log(-log u)  ==  (E_c / L_c) / sum_j (E_j / L_j),  E_c = exp(v_c - max v), L_c = -log u_c > 0:
  // ONE logarithm per element instead of two logarithms and an exponential (the kernel is bound by exactly this arithmetic and by
  // the Philox rounds), E is 64 values per image.  Same quantity as arch.py:2168-2177 up to fp32 rounding.  (The v_log_f32 /
  // v_rcp_f32 forms of the logarithm and the quotient were measured too: no change, 0.3835 ms per launch either way -- the kernel
  // moves 1.34 GB in that time, 3.5 TB/s stand-alone.)
  if (tid < 64) {
    float vm = vmax[b * 64];
    for (int c = 1; c < 64; ++c) vm = fmaxf(vm, vmax[b * 64 + c]);
    ev[tid] = expf(vmax[b * 64 + tid] - vm);
  }
  __syncthreads();
  // phase 1: weights w[i][c] = E_c / (-log u)   (coalesced along pixels)
  if (RNG) {
    if (seed_dev) seed = *seed_dev;                // key in device memory (graph replays: rewritten between replays)
    const int i = tid & 63;
    for (int j = tid >> 6; j < 16; j += 4) {       // channel group j = channels 4j .. 4j+3 of pixel i
      unsigned o[4];
      philox4x32_10((unsigned)(pin + i), (unsigned)b, (unsigned)j, draw, (unsigned)seed, (unsigned)(seed >> 32), o);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = 4 * j + k;
        const float u = ((float)(o[k] >> 8) + 0.5f) * (1.f / 16777216.f);
        if (noise_out) noise_out[(b * 64 + c) * P + pin + i] = u;
        z[i * ZS + c] = ev[c] / (-logf(u));
      }
    }
  } else {
    const int i = tid & 63;
    for (int c = tid >> 6; c < 64; c += 4) {
      const float u = noise[(b * 64 + c) * P + pin + i];
      z[i * ZS + c] = ev[c] / (-logf(u));
    }
  }
  for (int i = tid; i < 64 * QS; i += 256) { mq[i] = 0.f; vv[i] = 0.f; }
  __syncthreads();
  // phase 2: hard mask = softmax_c >= 0.5  <=>  w_c >= 0.5 * sum_j w_j ; 4 lanes per pixel, 16 channels each
  const int i = tid >> 2, part = tid & 3;
  {
    float e[16], s = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) { e[c] = z[i * ZS + part * 16 + c]; s += e[c]; }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    const float* px = xq + (p0 + i) * ldx + part * 16;
    float* pw = qwin + (p0 + i) * ldw + part * 16;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(px + c4 * 4);
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(px + 64 + c4 * 4);
      f32x4 w4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float mk = (e[c4 * 4 + k] >= 0.5f * s) ? 1.f : 0.f;
        mq[i * QS + 4 + part * 16 + c4 * 4 + k] = mk * q4[k];
        vv[i * QS + 4 + part * 16 + c4 * 4 + k] = v4[k];
        w4[k] = (1.f - mk) * q4[k];
      }
      *reinterpret_cast<f32x4*>(pw + c4 * 4) = w4;
    }
  }
  __syncthreads();
  // phase 3: 9-tap cross-correlation along the channel axis (zero padded), + bias
  {
    float w9[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w9[t] = wW[t];
    const float bb = bW[0];
    float* ps = sq + (p0 + i) * lds_ + part * 16;
    float* pv = vrow + (p0 + i) * ldv + part * 16;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      f32x4 a, bq;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = part * 16 + c4 * 4 + k;
        float s1 = bb, s2 = bb;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          s1 += w9[t] * mq[i * QS + c + t];
          s2 += w9[t] * vv[i * QS + c + t];
        }
        a[k] = s1;
        bq[k] = s2;
      }
      *reinterpret_cast<f32x4*>(ps + c4 * 4) = a;
      *reinterpret_cast<f32x4*>(pv + c4 * 4) = bq;
    }
  }
}

// ---- RDAB.input_conv (1x1, 64 -> 128: q | v) and rdab_prep in ONE pass: the 128-channel product never reaches HBM.
// The persistent LDS-DMA stream of conv1x1_stream.hip (NCB = 2, one K block): a wave's 32 pixels x 128 channels are in its
// accumulators after the split-bf16 product -- the same instructions in the same order as conv1x1_stream_kernel<2>, so q and v carry
// the bits that kernel would have stored.  Lane (pixel r, half h) holds channels 16 s + 8 h .. + 7 (s = 0..3) of q and of v, and
// everything rdab_prep does is local to the pixel:
//   * the weights E_c / (-log u_c) of the lane's 32 channels (noise read or drawn for exactly those channels);
//   * their sum in rdab_prep's order: 16 sequential terms per quarter -- lane h = 0 adds its 8, hands the partial sum to lane h = 1,
//     which adds its 8 and hands the total back --, then (q0 + q1) + (q2 + q3), which is what the xor-shuffles 1 and 2 form in every lane;
//   * qwin = (1 - mask) q and the window V straight from registers;
//   * the 9-tap channel convolutions need 4 channels on either side of a lane's 8: mask * q, then v, go through the stage the K
//     block has just been read from (free until the request after next), in the ring's own swizzled layout, wave-privately.
// V outputs (vrow: VT, window V: WT) as fp32 or, _Float16, rounded once -- the rounding the single-pass attentions apply while staging.
struct rf_args {
  const float* x; int ldx;                       // [B][P][>= 64]
  const float* w; const float* bias;             // input_conv: packed [64/4][128][4], bias [128] or null
  const float* vmax; const float* noise; const float* wW; const float* bW;
  long long P; int tiles_per_image; long long tiles; int ns;
  float* sq; int lds_; float* qwin; int ldw;
  void* vrow; int ldv; void* vwin; int ldvw;     // fp32 or fp16, pitches in elements
  unsigned long long seed; unsigned draw; float* noise_out; const unsigned long long* seed_dev;
  // PLANE form: the convolution's input is x + stencil9(plane) (fea + conv_expand_rms(rms), arch.py:4446-4449) and only x is in
  // memory; the stencil's part joins the product as the plane chunk of plane_chunk.h, plane.w = input_conv . [w_s | b_s], [128][16]
  pc_plane plane;
};
// MAP form: where the images of x lie (image_map.h).  A block of its own that only the MAP instantiations take: the other forms'
// kernel arguments, and with them their instructions, stay what they were
struct rf_args_map : rf_args {
  im_map x_map;
};

// PLANE is a template parameter: the other form's instructions stay what they were; so is MAP
template <bool RNG, typename VT, typename WT, bool PLANE = false, bool MAP = false>      // VT: vrow, WT: window V
__global__ __launch_bounds__(ST_THREADS) void rdab_prep_kernel_fused(std::conditional_t<MAP, rf_args_map, rf_args> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_smem[];
  constexpr int NCB = 2;
  constexpr bool VH = sizeof(VT) == 2, WH = sizeof(WT) == 2;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NS = a.ns;
  // LDS map: weights hi [4 chunks][2 k-halves][128 rows][8 bf16] | lo (same) | bias [128] | E [64] | 4 waves x NS stages
  constexpr int w_half = 4 * 2 * NCB * 64 * 16;
  constexpr int ring_off = 2 * w_half + NCB * 64 * 4 + 64 * 4;
  unsigned char* sWh = rf_smem;
  unsigned char* sWl = rf_smem + w_half;
  float* sBias = reinterpret_cast<float*>(rf_smem + 2 * w_half);
  float* ev = sBias + NCB * 64;
  unsigned char* ring = rf_smem + ring_off + wave * NS * ST_STAGE;
  const unsigned ring_lds = (unsigned)(unsigned long long)(rf_smem) + ring_off + wave * NS * ST_STAGE;
  // PLANE: behind the rings the chunk's weight image hi | lo, then NS tap slots per wave, indexed like the ring (one item per tile)
  unsigned char* sPh = rf_smem + ring_off + 4 * NS * ST_STAGE;
  unsigned char* sPl = sPh + pc_weight_bytes(NCB) / 2;
  const unsigned char* tap_slots = sPh + pc_weight_bytes(NCB) + wave * NS * PC_SLOT;
  const unsigned tap_lds = (unsigned)(unsigned long long)(rf_smem) + ring_off + 4 * NS * ST_STAGE + pc_weight_bytes(NCB) + wave * NS * PC_SLOT;

  const long long t_lo = a.tiles * blockIdx.x / gridDim.x, t_hi = a.tiles * (blockIdx.x + 1) / gridDim.x;
  if (t_lo >= t_hi) return;

  int d_px[8], d_part[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int s = 64 * k + lane, p = s >> 4;
    d_px[k] = p;
    d_part[k] = (s & 15) ^ (p & 15);
  }
  auto part_off = [&](int q) { return r * 256 + ((q ^ (r & 15)) << 4); };

  if (PLANE) pc_load_weights<NCB>(a.plane.w, NCB * 64, sPh, sPl, tid);      // (the barriers of the first image's trip publish them)
  // ---- the weights (the same for every image) -> LDS, split bf16 hi | lo, rows permuted (as conv1x1_stream_kernel)
  for (int i = tid; i < 16 * NCB * 64; i += ST_THREADS) {
    const int rowpos = i % (NCB * 64), kg = i / (NCB * 64);
    const int n = mfma_row_channel(rowpos);
    const f32x4 wv = *reinterpret_cast<const f32x4*>(a.w + ((long long)kg * (NCB * 64) + n) * 4);
    const int c = kg >> 2, hh = (kg >> 1) & 1, j0 = (kg & 1) * 4;
    u32x2 hi, lo;
    split4_bf16(wv, hi, lo);
    const int off = ((c * 2 + hh) * (NCB * 64) + rowpos) * 16 + j0 * 2;
    *reinterpret_cast<u32x2*>(sWh + off) = hi;
    *reinterpret_cast<u32x2*>(sWl + off) = lo;
  }
  for (int i = tid; i < NCB * 64; i += ST_THREADS) sBias[i] = a.bias ? a.bias[i] : 0.f;

  float w9[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w9[t] = a.wW[t];
  const float bb = a.bW[0];
  unsigned long long seed = a.seed;
  if (RNG && a.seed_dev) seed = *a.seed_dev;       // key in device memory (graph replays: rewritten between replays)

  for (long long img_t0 = t_lo; img_t0 < t_hi;) {
    const int b = (int)(img_t0 / a.tiles_per_image);
    const long long img_end = (long long)(b + 1) * a.tiles_per_image;
    const long long seg_hi = img_end < t_hi ? img_end : t_hi;           // tiles [img_t0, seg_hi) belong to image b
    __syncthreads();                                                     // the previous image's E has been read; no DMA is in flight here
    if (tid < 64) {                                                      // E_c = exp(v_c - max v), as rdab_prep_kernel
      float vm = a.vmax[(long long)b * 64];
      for (int c = 1; c < 64; ++c) vm = fmaxf(vm, a.vmax[(long long)b * 64 + c]);
      ev[tid] = expf(a.vmax[(long long)b * 64 + tid] - vm);
    }
    __syncthreads();

    const long long n_items = seg_hi - img_t0;                           // one item = one tile (a single K block)
    long long issued = 0;
    auto issue = [&](long long it) {
      const long long p0 = (img_t0 + it - (long long)b * a.tiles_per_image) * 128 + wave * 32;      // first pixel (inside image b)
      const long long rows_left = a.P - p0;                              // may be <= 0: everything out of range
      // (MAP: image b lies where x_map says; the descriptor still ends with this image's last pixel)
      long long img = 0;
      if constexpr (MAP) img = im_offset(a.x_map, b);
      const float* base = MAP ? a.x + img + (rows_left > 0 ? p0 : 0) * a.ldx
                              : a.x + ((long long)b * a.P + (rows_left > 0 ? p0 : 0)) * a.ldx;
      const long long bytes = rows_left > 0 ? (rows_left < 32 ? rows_left : 32) * (long long)a.ldx * 4 : 0;
      const i32x4 rsrc = lds_dma_rsrc_uniform(base, (unsigned)bytes);      // lanes beyond the image read zeros
      if (PLANE)                 // the tile's taps, ahead of its item: in order behind it, so landed when it has (plane_chunk.h)
        pc_issue(pc_image(a.plane, b), (int)a.P, a.plane.W, (int)p0, lane, tap_lds + (unsigned)(it % NS) * PC_SLOT);
      unsigned voff[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) voff[q] = (unsigned)(d_px[q] * a.ldx * 4 + d_part[q] * 16);
      lds_dma0(voff, rsrc, __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)(it % NS) * ST_STAGE));
    };
    for (; issued < NS - 1 && issued < n_items; ++issued) issue(issued);

    for (long long it = 0; it < n_items; ++it) {
      st_wait_landed(issued - it - 1);
      unsigned char* st = ring + (it % NS) * ST_STAGE;
      f32x16 acc[NCB][2];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[cb][ni][e] = 0.f;
      if (PLANE) {
        // the plane chunk's k-step opens the product; its slot is read here, before the request below can reuse any slot.  The
        // hand-counted wait above stays valid: the three older pieces of every tile only make it more conservative
        const int p = (int)((img_t0 + it - (long long)b * a.tiles_per_image) * 128) + wave * 32 + r;
        unsigned thi[4], tlo[4];
        pc_operand(tap_slots + (it % NS) * PC_SLOT, r, h, p, (int)a.P, a.plane.W, thi, tlo);
        pc_mfma<NCB>(sPh, sPl, r, h, thi, tlo, acc);
      }
      // ---- the K block, as conv1x1_stream_kernel: this lane's operand = channels c*16 + h*8 .. +7 of pixel r
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(st + part_off(c * 4 + h * 2));
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(st + part_off(c * 4 + h * 2 + 1));
        union { unsigned u[4]; bf16x8_t v; } ph, pl;
        split8_bf16(v0, v1, ph.u, pl.u);
        const int wrow = (c * 2 + h) * (NCB * 64) + r;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const bf16x8_t wh = *reinterpret_cast<const bf16x8_t*>(sWh + (wrow + cb * 64 + ni * 32) * 16);
            const bf16x8_t wl = *reinterpret_cast<const bf16x8_t*>(sWl + (wrow + cb * 64 + ni * 32) * 16);
            acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, pl.v, acc[cb][ni], 0, 0, 0);
            acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, ph.v, acc[cb][ni], 0, 0, 0);
            acc[cb][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, ph.v, acc[cb][ni], 0, 0, 0);
          }
      }
      // the next request overwrites the stage of item it - 1; this item's fragment reads have returned (the MFMAs consumed them)
      if (issued < n_items) { wait_lgkm<0>(); issue(issued); ++issued; }

      const long long pin = (img_t0 + it - (long long)b * a.tiles_per_image) * 128 + wave * 32 + r;
      if (pin - r >= a.P) continue;                  // P % 32 == 0: a wave's 32 pixels lie inside the image or all beyond it
      const long long gp = (long long)b * a.P + pin;
      // acc[cb][s >> 1][8 (s & 1) + k] = channel 16 s + 8 h + k of q (cb = 0) / v (cb = 1), + bias
      float ez[4][8];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int c0 = 16 * s + 8 * h;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          acc[0][s >> 1][8 * (s & 1) + k] += sBias[c0 + k];
          acc[1][s >> 1][8 * (s & 1) + k] += sBias[64 + c0 + k];
        }
        // ---- weights E_c / (-log u_c)
        if (RNG) {
#pragma unroll
          for (int j2 = 0; j2 < 2; ++j2) {
            unsigned o[4];
            philox4x32_10((unsigned)pin, (unsigned)b, (unsigned)((c0 >> 2) + j2), a.draw, (unsigned)seed, (unsigned)(seed >> 32), o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int c = c0 + 4 * j2 + k;
              const float u = ((float)(o[k] >> 8) + 0.5f) * (1.f / 16777216.f);
              if (a.noise_out) a.noise_out[((long long)b * 64 + c) * a.P + pin] = u;
              ez[s][4 * j2 + k] = ev[c] / (-logf(u));
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float u = a.noise[((long long)b * 64 + c0 + k) * a.P + pin];
            ez[s][k] = ev[c0 + k] / (-logf(u));
          }
        }
      }
      // ---- the pixel's sum in rdab_prep's order
      float qs[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float p = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) p += ez[s][k];                     // h = 0: terms 0..7 of the quarter
        float f = __shfl_xor(p, 32, 64);
#pragma unroll
        for (int k = 0; k < 8; ++k) f += ez[s][k];                     // h = 1: ... + terms 8..15
        const float fo = __shfl_xor(f, 32, 64);
        qs[s] = h ? f : fo;
      }
      const float half_s = 0.5f * ((qs[0] + qs[1]) + (qs[2] + qs[3]));
      // ---- mask; qwin and the window V from registers; mask * q replaces q in the accumulators
      {
        float* pw = a.qwin + gp * a.ldw;
        WT* pvw = static_cast<WT*>(a.vwin) + gp * a.ldvw;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int c0 = 16 * s + 8 * h;
          float wq[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float mk = (ez[s][k] >= half_s) ? 1.f : 0.f;
            const float qv = acc[0][s >> 1][8 * (s & 1) + k];
            acc[0][s >> 1][8 * (s & 1) + k] = mk * qv;
            wq[k] = (1.f - mk) * qv;
          }
          const f32x4 w0 = {wq[0], wq[1], wq[2], wq[3]}, w1 = {wq[4], wq[5], wq[6], wq[7]};
          *reinterpret_cast<f32x4*>(pw + c0) = w0;
          *reinterpret_cast<f32x4*>(pw + c0 + 4) = w1;
          if (WH) {
            attn_f16x8 hv;
#pragma unroll
            for (int k = 0; k < 8; ++k) hv[k] = (_Float16)acc[1][s >> 1][8 * (s & 1) + k];
            *reinterpret_cast<attn_f16x8*>(pvw + c0) = hv;
          } else {
            const f32x4 x0 = {acc[1][s >> 1][8 * (s & 1)], acc[1][s >> 1][8 * (s & 1) + 1], acc[1][s >> 1][8 * (s & 1) + 2], acc[1][s >> 1][8 * (s & 1) + 3]};
            const f32x4 x1 = {acc[1][s >> 1][8 * (s & 1) + 4], acc[1][s >> 1][8 * (s & 1) + 5], acc[1][s >> 1][8 * (s & 1) + 6], acc[1][s >> 1][8 * (s & 1) + 7]};
            *reinterpret_cast<f32x4*>(pvw + c0) = x0;
            *reinterpret_cast<f32x4*>(pvw + c0 + 4) = x1;
          }
        }
      }
      // ---- 9-tap cross-correlation along the channel axis (zero padded) + bias: mask * q -> sq, then v -> vrow
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");           // the other lanes' reads of the previous contents come first
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int q0 = 4 * s + 2 * h;
          const f32x4 x0 = {acc[cb][s >> 1][8 * (s & 1)], acc[cb][s >> 1][8 * (s & 1) + 1], acc[cb][s >> 1][8 * (s & 1) + 2], acc[cb][s >> 1][8 * (s & 1) + 3]};
          const f32x4 x1 = {acc[cb][s >> 1][8 * (s & 1) + 4], acc[cb][s >> 1][8 * (s & 1) + 5], acc[cb][s >> 1][8 * (s & 1) + 6], acc[cb][s >> 1][8 * (s & 1) + 7]};
          *reinterpret_cast<f32x4*>(st + part_off(q0)) = x0;
          *reinterpret_cast<f32x4*>(st + part_off(q0 + 1)) = x1;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");           // a wave's LDS operations execute in order: lane ^ 32's values are there
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int c0 = 16 * s + 8 * h, q0 = 4 * s + 2 * h;
          const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
          f32x4 lf = *reinterpret_cast<const f32x4*>(st + part_off(q0 > 0 ? q0 - 1 : 0));
          f32x4 rt = *reinterpret_cast<const f32x4*>(st + part_off(q0 + 2 < 16 ? q0 + 2 : 15));
          lf = q0 > 0 ? lf : z4;
          rt = q0 + 2 < 16 ? rt : z4;
          float win[16];                                                  // channels c0 - 4 .. c0 + 11
#pragma unroll
          for (int k = 0; k < 4; ++k) { win[k] = lf[k]; win[12 + k] = rt[k]; }
#pragma unroll
          for (int k = 0; k < 8; ++k) win[4 + k] = acc[cb][s >> 1][8 * (s & 1) + k];
          float o8[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float s1 = bb;
#pragma unroll
            for (int t = 0; t < 9; ++t) s1 = fmaf(w9[t], win[k + t], s1);
            o8[k] = s1;
          }
          if (cb == 1 && VH) {
            attn_f16x8 hv;
#pragma unroll
            for (int k = 0; k < 8; ++k) hv[k] = (_Float16)o8[k];
            *reinterpret_cast<attn_f16x8*>(static_cast<VT*>(a.vrow) + gp * a.ldv + c0) = hv;
          } else {
            float* po = cb == 0 ? a.sq + gp * a.lds_ : static_cast<float*>(a.vrow) + gp * a.ldv;
            const f32x4 y0 = {o8[0], o8[1], o8[2], o8[3]}, y1 = {o8[4], o8[5], o8[6], o8[7]};
            *reinterpret_cast<f32x4*>(po + c0) = y0;
            *reinterpret_cast<f32x4*>(po + c0 + 4) = y1;
          }
        }
      }
    }
    img_t0 = seg_hi;
  }
}

// directH1_conv (arch.py:2162, 2225): 9 taps along the image rows.  A thread owns one (image, row segment, column, 4-channel
// group) and slides down its segment with the nine input rows of the current output in registers: every input element is
// read once per segment (the rows of a segment's 4 + 4 halo twice), coalesced across columns / channel groups.
constexpr int CC9_SEG = 34;     // output rows per thread
__global__ __launch_bounds__(256) void colconv9_kernel(const float* __restrict__ in, int ldi,
                                                       const float* __restrict__ wH, const float* __restrict__ bH,
                                                       int B, int H, int W, int nseg, float* __restrict__ out, int ldo) {
  float w9[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w9[t] = wH[t];
  const float bb = bH[0];
  const long long total = (long long)B * nseg * W * 16;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int cg = idx & 15;
    long long r = idx >> 4;
    const int x = (int)(r % W); r /= W;
    const int seg = (int)(r % nseg);
    const long long b = r / nseg;
    const int y0 = seg * CC9_SEG, y1 = min(H, y0 + CC9_SEG);
    const float* col = in + (b * H * W + x) * ldi + cg * 4;
    float* ocol = out + (b * H * W + x) * ldo + cg * 4;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 win[9];                                        // win[t] = in[y + t - 4]
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int yy = y0 + t - 4;
      win[t + 1] = (yy >= 0 && yy < H) ? *reinterpret_cast<const f32x4*>(col + (long long)yy * W * ldi) : z;
    }
    for (int y = y0; y < y1; ++y) {
#pragma unroll
      for (int t = 0; t < 8; ++t) win[t] = win[t + 1];
      const int yy = y + 4;
      win[8] = yy < H ? *reinterpret_cast<const f32x4*>(col + (long long)yy * W * ldi) : z;
      f32x4 acc = {bb, bb, bb, bb};
#pragma unroll
      for (int t = 0; t < 9; ++t) acc += w9[t] * win[t];
      *reinterpret_cast<f32x4*>(ocol + (long long)y * W * ldo) = acc;
    }
  }
}

// MODE 0: sequence = image row (keys along W); 1: image column (keys along H); 2: 8x8 window.
template <int MODE>
__global__ __launch_bounds__(64) void seq_attn_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ v,
                                                      int ldv, float* __restrict__ out, int ldo, int B, int H, int W) {
  const int lane = threadIdx.x;
  long long kbase;      // pixel index of key 0
  long long kstep;      // pixel stride between consecutive keys (MODE 0/1)
  int L;                // number of keys
  long long qpix;       // this lane's query pixel
  bool active = true;
  if (MODE == 0) {
    const int nb = (W + 63) / 64;
    const int blk = blockIdx.x % nb;
    const long long row = blockIdx.x / nb;  // b*H + h
    kbase = row * W; kstep = 1; L = W;
    int x = blk * 64 + lane;
    if (x >= W) { x = W - 1; active = false; }
    qpix = kbase + x;
  } else if (MODE == 1) {
    const int nb = (H + 63) / 64;
    const int blk = blockIdx.x % nb;
    const long long col = blockIdx.x / nb;  // b*W + w
    const long long b = col / W, w = col - b * W;
    kbase = b * H * W + w; kstep = W; L = H;
    int y = blk * 64 + lane;
    if (y >= H) { y = H - 1; active = false; }
    qpix = kbase + (long long)y * W;
  } else {
    const int nwx = W >> 3, nwy = H >> 3;
    const int wx = blockIdx.x % nwx, wy = (blockIdx.x / nwx) % nwy;
    const long long b = blockIdx.x / (nwx * nwy);
    kbase = (b * H + wy * 8) * W + wx * 8; kstep = 0; L = 64;
    qpix = kbase + (long long)(lane >> 3) * W + (lane & 7);
  }
  float qr[64], o[64];
#pragma unroll
  for (int c4 = 0; c4 < 16; ++c4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(q + qpix * ldq + c4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { qr[c4 * 4 + e] = t[e]; o[c4 * 4 + e] = 0.f; }
  }
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j < L; ++j) {
    const long long kp = (MODE == 2) ? kbase + (long long)(j >> 3) * W + (j & 7) : kbase + (long long)j * kstep;
    const float* __restrict__ kr = q + kp * ldq;  // wave-uniform address -> scalar loads
    const float* __restrict__ vr = v + kp * ldv;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
      s0 = fmaf(qr[c], kr[c], s0);
      s1 = fmaf(qr[c + 1], kr[c + 1], s1);
      s2 = fmaf(qr[c + 2], kr[c + 2], s2);
      s3 = fmaf(qr[c + 3], kr[c + 3], s3);
    }
    const float s = (s0 + s1) + (s2 + s3);
    if (s > m) {  // new running max: rescale what has been accumulated so far
      const float alpha = expf(m - s);
      l *= alpha;
#pragma unroll
      for (int c = 0; c < 64; ++c) o[c] *= alpha;
      m = s;
    }
    const float pj = expf(s - m);
    l += pj;
#pragma unroll
    for (int c = 0; c < 64; ++c) o[c] = fmaf(pj, vr[c], o[c]);
  }
  if (active) {
    const float inv = 1.f / l;
    float* po = out + qpix * ldo;
#pragma unroll
    for (int c4 = 0; c4 < 16; ++c4) {
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = o[c4 * 4 + e] * inv;
      *reinterpret_cast<f32x4*>(po + c4 * 4) = t;
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------
// Row / column attention on the matrix cores, flash style.
// One wave owns 32 queries; 4 waves (128 queries of ONE sequence) share the key/value tiles staged in LDS.
//   S^T[key][query] = K Q^T : A = K (rows = keys), B = Q^T, on the fp16 matrix cores with BOTH operands split into
//                     fp16 hi + fp16 lo (22 significant bits; hi*hi + lo*hi + hi*lo, the 2^-22 lo*lo term dropped):
//                     12 v_mfma_f32_32x32x16_f16 (384 cycles) per 32x32 tile instead of 32 v_mfma_f32_32x32x2_f32
//                     (2048 cycles), scores exact to ~1e-6 relative.  Lane (r, h) keeps Q[r][16s + 8h .. +7] (s = 0..3)
//                     in registers and reads the same channels of K[r] from LDS (hi | lo halves of a 272-byte row).
//   softmax          : the accumulator holds, per lane, 16 keys of ITS query (column) -> the running max needs one
//                     cross-half shuffle, the exponentials are lane-local.
//   O^T[ch][query]  += V^T P^T, also fp16 hi/lo x 3 passes: the probabilities are already the B operand -- register
//                     8u + j of half h is key 16u + 4h + 8(j>>2) + (j&3) of query r, and the key order inside a dot
//                     product is free, so V is staged TRANSPOSED ([channel][key slot], slot = 16u + 8h + j) in that
//                     same order: a staging thread loads 4 keys x 4 channels, transposes 4x4 in registers and writes
//                     8-byte runs of 4 keys; no data movement between the two products.
typedef unsigned attn_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned attn_u32x4 __attribute__((ext_vector_type(4)));

// NW waves per workgroup = 32*NW queries of one sequence at most; a stage is 8*NW keys (NW/4 sub-tiles of 32), staged by
// all NW*64 threads with one 4-key x 4-channel unit each -- the larger the workgroup, the less staging work (loads,
// fp32 -> fp16 hi/lo splits, LDS writes) per query.  The query tiles of a sequence are spread evenly over its workgroups
// (tpb tiles each; waves >= tpb only stage).  The kernel is VALU-bound (softmax + splits), not MFMA-bound, hence:
// scores in the log2 domain (Q is scaled by log2 e once, p = v_exp_f32(s - m) -- one instruction instead of expf's ten),
// key masking only in a sequence's last sub-tile, and the accumulator rescale skipped while no lane's running maximum moves.
// PV1 (the default fp16x2 arithmetic of the forward): the SECOND product with single-fp16 operands -- probabilities p in [0, 1]
// (sum 1) and values rounded once to fp16: |error of an output| <= 2^-11 * sum_j p_j |v_j| <= 4.9e-4 * max|v| in the worst case,
// ~1e-5 * |v| measured (random signs average); the scores, whose error the exponential amplifies, keep all three passes.  8 of the
// 24 MFMAs per 32 x 32 tile, the lo halves of V's staging and of P's conversion, and half of V's fragment reads go away.
// VT = _Float16 (PV1 only): V arrives already rounded -- its producer stored (_Float16)v, the same single rounding the staging
// thread applies to an fp32 V -- and goes to sV unconverted, ldv counted in halves.  OT = _Float16: the output leaves as
// (_Float16)(o / l), the form in which the next attention's staging would round it (row attention -> V of the column attention).
template <int MODE, int NW, bool PV1 = false, typename VT = float, typename OT = float>   // MODE 0: sequence = image row, 1: image column, 2: 8x8 window (row-major inside the window)
__global__ __launch_bounds__(NW * 64, NW == 4 ? 3 : 2) void seq_attn_mfma_kernel(const float* __restrict__ q, int ldq,
                                                                const VT* __restrict__ v, int ldv,
                                                                OT* __restrict__ out, int ldo, int B, int H, int W,
                                                                int nb, int tpb, int xcd_map) {
  constexpr bool VH = sizeof(VT) == 2, OH = sizeof(OT) == 2;
  static_assert(PV1 || !VH, "an fp16 V is the single-pass second product's operand");
  constexpr int KROW = 272;                                 // bytes per staged key row: 128 B hi | 128 B lo | 16 B pad
  constexpr int NT = NW * 64, SUB = NW / 4, KT = 32 * SUB, KQ = KT / 4;
  constexpr int K_BYTES = KT * KROW, V_BYTES = SUB * 64 * 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  unsigned char* const sK = attn_smem;                      // [2][KT][KROW]
  // V^T per sub-tile: row = channel (128 B: four 16-byte hi slots 2u+h, four lo slots 4+2u+h), slot index XORed with
  // (ch>>1)&7 so that the 16 channels of a ds_read_b128 lane group hit 16 distinct 16-byte slots
  unsigned char* const sV = attn_smem + 2 * K_BYTES;        // [2][SUB][64][128]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, r = lane & 31;
  const int L = MODE == 0 ? W : (MODE == 1 ? H : 64);
  // The nb workgroups of a sequence each stage ALL of its keys / values: give them consecutive slots of ONE XCD (workgroup i
  // runs on XCD i % 8), so that they run at about the same time behind the same L2 and the sequence leaves HBM once
  unsigned bid = blockIdx.x;
  if (xcd_map) {
    const unsigned q8 = gridDim.x >> 3, r8 = gridDim.x & 7, xcd = bid & 7, idx = bid >> 3;
    bid = xcd * q8 + (xcd < r8 ? xcd : r8) + idx;
  }
  const int blk = bid % nb;
  const long long seq = bid / nb;
  long long kbase;
  if (MODE == 0) kbase = seq * W;                           // seq = b*H + y
  else if (MODE == 1) { const long long b = seq / W, x = seq - b * W; kbase = b * H * W + x; }
  else {                                                    // seq = (b*(H/8) + wy)*(W/8) + wx
    const int wpr = W >> 3;
    const long long t = seq / wpr;
    const int wx = (int)(seq - t * wpr);
    kbase = (t * 8) * W + wx * 8;                           // t*8 = b*H + wy*8
  }
  auto pix_of = [&](int i) -> long long {                   // pixel of element i of the sequence
    return MODE == 0 ? kbase + i : (MODE == 1 ? kbase + (long long)i * W : kbase + (long long)(i >> 3) * W + (i & 7));
  };
  const int q0 = (blk * tpb + wave) * 32;                   // this wave's first query
  const bool wave_active = wave < tpb && q0 < L;
  int qi = q0 + r;
  const bool q_ok = qi < L;
  if (qi >= L) qi = L - 1;
  const long long qpix = pix_of(qi);

  attn_f16x8 qh[4], ql[4];                                  // log2(e) * Q[r][16s + 8h + j], fp16 hi / lo
  constexpr float LOG2E = 1.4426950408889634f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(q + qpix * ldq + 16 * s + 8 * h) * LOG2E;
    const f32x4 t1 = *reinterpret_cast<const f32x4*>(q + qpix * ldq + 16 * s + 8 * h + 4) * LOG2E;
    // split_pair_f16, not "lo = fp16(x - (float)hi)" written out: under -ffp-contract=fast the compiler fused the multiplication
    // into ONE of hi's two uses (v_fma_mixlo_f16 rounds the exact product q * log2 e, v_cvt_pk_f16_f32 the fp32 product).  Where
    // the fp32 product is an exact fp16 tie (1 element in 8192) the two can round apart, and hi + lo was then off by a whole fp16
    // ulp of that element, 2^-10 relative, in every score of its query.  The helper's remainder reads the hi register it returns.
    unsigned hu[4], lu[4];
    split_pair_f16(t0[0], t0[1], hu[0], lu[0]);
    split_pair_f16(t0[2], t0[3], hu[1], lu[1]);
    split_pair_f16(t1[0], t1[1], hu[2], lu[2]);
    split_pair_f16(t1[2], t1[3], hu[3], lu[3]);
    const attn_u32x4 qhu = {hu[0], hu[1], hu[2], hu[3]}, qlu = {lu[0], lu[1], lu[2], lu[3]};
    qh[s] = __builtin_bit_cast(attn_f16x8, qhu);
    ql[s] = __builtin_bit_cast(attn_f16x8, qlu);
  }
  f32x16 o0, o1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
  float m = -INFINITY, l = 0.f;                             // running maximum (log2 domain) and sum of this half-wave's keys

  // staging (4 float4 loads per thread and stage): the first NT/2 threads take V -- keys 4sm..4sm+3 x channels 4c..4c+3
  // each --, the others K -- keys sm + KQ*s (s = 0..3) x channels 4c..4c+3.
  // fp16 V: a 16-byte load is 8 channels of a key, so the first NT/4 threads cover the stage's V (keys 4sm..4sm+3 x channels
  // 8c..8c+7); the next NT/4 repeat their loads and write nothing -- one instruction stream for every thread, no branch around the
  // loads (a branch there made hipcc wait for them where the paths meet instead of behind the stage's products; sharing the writes
  // between the two quarters, four channels each, measured no better)
  const bool st_v = tid < NT / 2, vh_t = VH && st_v;
  const int sj = st_v ? tid : tid - NT / 2, sjv = sj & (NT / 4 - 1);
  const int sm = vh_t ? sjv >> 3 : sj >> 4, sc4 = vh_t ? 2 * (sjv & 7) : sj & 15;        // sc4: the first 4-channel group
  const float* const sbase = (st_v ? reinterpret_cast<const float*>(v) : q) + (vh_t ? sc4 * 2 : sc4 * 4);
  const int sld = vh_t ? ldv >> 1 : (st_v ? ldv : ldq);                                  // in floats
  f32x4 rs[4];
  auto load_tile = [&](int t0) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int key = t0 + (st_v ? 4 * sm + s : sm + KQ * s);
      key = key < L ? key : L - 1;                          // clamped (masked below), always loaded
      rs[s] = *reinterpret_cast<const f32x4*>(sbase + pix_of(key) * sld);
    }
  };
  auto write_tile = [&](int buf) {
    if (st_v) {
      // keys 4m..4m+3 of sub-tile sm>>3 = slots 16u + 8hh + 4g + (0..3) with m = sm&7, u = m>>2, hh = m&1, g = (m&3)>>1
      const int mm = sm & 7, c = 2 * (mm >> 2) + (mm & 1), g = (mm & 3) >> 1;
      unsigned char* const vb = sV + buf * V_BYTES + (sm >> 3) * 8192 + g * 8;
      if (VH) {                                             // rounded by the producer: 8 channels x keys 4m .. 4m+3, as they are
        if (sj < NT / 4) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ch = 4 * sc4 + e, swz = (ch >> 1) & 7;
            unsigned k[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) k[s] = __float_as_uint(rs[s][e >> 1]);
            const attn_u32x2 vh = {(e & 1) ? (k[0] >> 16) | (k[1] & 0xffff0000u) : (k[0] & 0xffffu) | (k[1] << 16),
                                   (e & 1) ? (k[2] >> 16) | (k[3] & 0xffff0000u) : (k[2] & 0xffffu) | (k[3] << 16)};
            *reinterpret_cast<attn_u32x2*>(vb + ch * 128 + ((c ^ swz) * 16)) = vh;
          }
        }
      } else
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = 4 * sc4 + e, swz = (ch >> 1) & 7;
        if (PV1) {                                          // keys 4m .. 4m+3 of channel ch, rounded once
          const attn_f16x4 vh = {(_Float16)rs[0][e], (_Float16)rs[1][e], (_Float16)rs[2][e], (_Float16)rs[3][e]};
          *reinterpret_cast<attn_f16x4*>(vb + ch * 128 + ((c ^ swz) * 16)) = vh;
        } else {
          unsigned h0, l0, h1, l1;
          split_pair_f16(rs[0][e], rs[1][e], h0, l0);
          split_pair_f16(rs[2][e], rs[3][e], h1, l1);
          const attn_u32x2 vh = {h0, h1}, vl = {l0, l1};
          *reinterpret_cast<attn_u32x2*>(vb + ch * 128 + ((c ^ swz) * 16)) = vh;
          *reinterpret_cast<attn_u32x2*>(vb + ch * 128 + (((4 + c) ^ swz) * 16)) = vl;
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        unsigned h0, l0, h1, l1;
        split_pair_f16(rs[s][0], rs[s][1], h0, l0);
        split_pair_f16(rs[s][2], rs[s][3], h1, l1);
        const attn_u32x2 kh = {h0, h1}, kl = {l0, l1};
        unsigned char* row = sK + buf * K_BYTES + (sm + KQ * s) * KROW + sc4 * 8;
        *reinterpret_cast<attn_u32x2*>(row) = kh;
        *reinterpret_cast<attn_u32x2*>(row + 128) = kl;
      }
    }
  };

  const int nstages = (L + KT - 1) / KT;
  load_tile(0);
  write_tile(0);
  __syncthreads();
  for (int t = 0; t < nstages; ++t) {
    const int buf = t & 1;
    if (t + 1 < nstages) load_tile((t + 1) * KT);
    if (wave_active) {
      // The stage's SUB sub-tiles of 32 keys share ONE softmax update: all their score products first (independent
      // accumulators, back to back on the matrix pipe), one running-maximum step for the 64 keys, then all the V^T P^T products
      // -- half the rescale tests and longer MFMA runs for the vector work of the SIMD's other wave to hide behind
      const int kv_stage = L - t * KT;                      // keys of this stage that exist (> 0)
      const int nsub = kv_stage >= KT ? SUB : (kv_stage + 31) >> 5;
      f32x16 sacc[SUB];
#pragma unroll
      for (int sub = 0; sub < SUB; ++sub) {
        if (sub >= nsub) break;
        // ---- S^T = K Q^T (log2 domain)
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[sub][e] = 0.f;
        const unsigned char* const kb = sK + buf * K_BYTES + (sub * 32 + r) * KROW + 16 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const attn_f16x8 kh = *reinterpret_cast<const attn_f16x8*>(kb + 32 * s);
          const attn_f16x8 kl = *reinterpret_cast<const attn_f16x8*>(kb + 32 * s + 128);
          sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[s], sacc[sub], 0, 0, 0);
          sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[s], sacc[sub], 0, 0, 0);
          sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[s], sacc[sub], 0, 0, 0);
        }
      }
      // ---- online softmax over the stage's keys (per sub-tile 16 here, 16 in the partner half-wave)
      float tmax = -INFINITY;
#pragma unroll
      for (int sub = 0; sub < SUB; ++sub) {
        if (sub >= nsub) break;
        const int kv_left = kv_stage - sub * 32;
        if (kv_left < 32) {                                 // only a sequence's last sub-tile has keys to mask
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if ((e & 3) + 8 * (e >> 2) + 4 * h >= kv_left) sacc[sub][e] = -INFINITY;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) tmax = fmaxf(tmax, sacc[sub][e]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m, tmax);
      if (__any(mn > m)) {                                  // some lane's running maximum moved: rescale
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        l *= alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
        m = mn;
      }
      float psum = 0.f;
#pragma unroll
      for (int sub = 0; sub < SUB; ++sub) {
        if (sub >= nsub) break;
#pragma unroll
        for (int e = 0; e < 16; ++e) { sacc[sub][e] = __builtin_amdgcn_exp2f(sacc[sub][e] - m); psum += sacc[sub][e]; }
      }
      l += psum;
      // ---- O^T += V^T P^T
#pragma unroll
      for (int sub = 0; sub < SUB; ++sub) {
        if (sub >= nsub) break;
        const unsigned char* const vb = sV + buf * V_BYTES + sub * 8192;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          attn_f16x8 ph, pl;
          if (PV1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ph[j] = (_Float16)sacc[sub][8 * u + j];
          } else {
            unsigned hh[4], ll[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) split_pair_f16(sacc[sub][8 * u + 2 * j], sacc[sub][8 * u + 2 * j + 1], hh[j], ll[j]);
            const attn_u32x4 phu = {hh[0], hh[1], hh[2], hh[3]}, plu = {ll[0], ll[1], ll[2], ll[3]};
            ph = __builtin_bit_cast(attn_f16x8, phu);
            pl = __builtin_bit_cast(attn_f16x8, plu);
          }
#pragma unroll
          for (int half = 0; half < 2; ++half) {            // channels 0-31 -> o0, 32-63 -> o1
            const int ch = 32 * half + r, swz = (ch >> 1) & 7, c = 2 * u + h;
            const attn_f16x8 vh = *reinterpret_cast<const attn_f16x8*>(vb + ch * 128 + ((c ^ swz) * 16));
            f32x16& o = half ? o1 : o0;
            if (!PV1) {
              const attn_f16x8 vl = *reinterpret_cast<const attn_f16x8*>(vb + ch * 128 + (((4 + c) ^ swz) * 16));
              o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o, 0, 0, 0);
              o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o, 0, 0, 0);
            }
            o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o, 0, 0, 0);
          }
        }
      }
    }
    if (t + 1 < nstages) write_tile(buf ^ 1);
    __syncthreads();
  }
  if (wave_active) {
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.f / l;
    if (q_ok) {
      OT* po = out + qpix * ldo;
#pragma unroll
      for (int g = 0; g < 4; ++g) {                          // rows 8g+4h .. +3 of each 32-channel tile
        f32x4 a0, a1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a0[e] = o0[4 * g + e] * inv; a1[e] = o1[4 * g + e] * inv; }
        if (OH) {
          // The fp32 products are pinned in their registers first: hipcc otherwise merges product and conversion into ONE
          // v_fma_mixlo_f16, which rounds the exact product -- not the fp32 value that the fp32 form stores and the next
          // attention's staging rounds (an empty statement, no instruction)
#pragma unroll
          for (int e = 0; e < 4; ++e) { asm("" : "+v"(a0[e])); asm("" : "+v"(a1[e])); }
          const attn_f16x4 h0 = {(_Float16)a0[0], (_Float16)a0[1], (_Float16)a0[2], (_Float16)a0[3]};
          const attn_f16x4 h1 = {(_Float16)a1[0], (_Float16)a1[1], (_Float16)a1[2], (_Float16)a1[3]};
          *reinterpret_cast<attn_f16x4*>(po + 8 * g + 4 * h) = h0;
          *reinterpret_cast<attn_f16x4*>(po + 32 + 8 * g + 4 * h) = h1;
        } else {
          *reinterpret_cast<f32x4*>(po + 8 * g + 4 * h) = a0;
          *reinterpret_cast<f32x4*>(po + 32 + 8 * g + 4 * h) = a1;
        }
      }
    }
  }
}

template <int MODE, int NW, bool PV1 = false, typename VT = float, typename OT = float>
int seq_attn_launch(const float* q, int ldq, const VT* v, int ldv, OT* out, int ldo, int B, int H, int W, hipStream_t st) {
  static CdfoAttrOnce once;
  constexpr int SUB = NW / 4, LDSB = 2 * (32 * SUB * 272 + SUB * 64 * 128);
  const hipError_t e = cdfo_set_max_lds(once, reinterpret_cast<const void*>(&seq_attn_mfma_kernel<MODE, NW, PV1, VT, OT>), LDSB);
  if (e != hipSuccess) return (int)e;
  const int L = MODE == 0 ? W : (MODE == 1 ? H : 64);
  const int ntq = cdiv(L, 32), nb = cdiv(ntq, NW), tpb = cdiv(ntq, nb);
  const long long nseq = MODE == 0 ? (long long)B * H : (MODE == 1 ? (long long)B * W : (long long)B * (H / 8) * (W / 8));
  if (nseq * nb >= (1ll << 31)) return CDFO_EINVAL;
  static const int xcd_map = cdfo_switch("CDFO_ATTN_XCD", 1);   // developer A/B switch
  hipLaunchKernelGGL((seq_attn_mfma_kernel<MODE, NW, PV1, VT, OT>), dim3((unsigned)(nseq * nb)), dim3(NW * 64), LDSB, st, q, ldq, v, ldv,
                     out, ldo, B, H, W, nb, tpb, (nb > 1 && xcd_map) ? 1 : 0);
  return 0;
}

// 8-wave workgroups amortise the staging over twice the queries, but only if the sequence's 32-query tiles fill them:
// 272 keys = 9 tiles = 2 x 8 waves at 56 % or 3 x 4 waves at 75 % (column attention at 24 x 272 x 480: 1.61 vs 1.35 ms;
// row attention, 480 keys: 1.67 ms with 8 waves, 1.86 with 4).  The strided key rows of the column form are NOT what
// it waits for: the same products over transposed tensors (contiguous rows of 272 keys) took 1.50 ms.
bool seq_attn_wide(int L) {
  const int ntq = cdiv(L, 32);
  static const int force_nw = cdfo_switch("CDFO_ATTN_NW", 0);     // developer switch (4 / 8)
  return force_nw ? force_nw == 8 : L > 128 && (double)ntq / (cdiv(ntq, 8) * 8) >= (double)ntq / (cdiv(ntq, 4) * 4) - 0.1;
}

// the single-pass forms (modes 20 / 21 / 22) over the operand types
template <int MODE, typename VT, typename OT>
int seq_attn_pv1(const float* q, int ldq, const VT* v, int ldv, OT* out, int ldo, int B, int H, int W, hipStream_t st) {
  if constexpr (MODE != 2) {
    if (seq_attn_wide(MODE == 0 ? W : H)) return seq_attn_launch<MODE, 8, true, VT, OT>(q, ldq, v, ldv, out, ldo, B, H, W, st);
  }
  return seq_attn_launch<MODE, 4, true, VT, OT>(q, ldq, v, ldv, out, ldo, B, H, W, st);
}

}  // namespace

extern "C" int cdfo_rdab_prep(const float* xq, int ldx, const float* vmax, const float* noise, const float* wW,
                              const float* bW, int B, long long P, float* sq, int lds_, float* vrow, int ldv, float* qwin,
                              int ldw, void* stream) {
  if (B <= 0 || P <= 0 || P % 64 || ldx % 4 || lds_ % 4 || ldv % 4 || ldw % 4) return CDFO_EINVAL;
  if (!aligned16(xq) || !aligned16(sq) || !aligned16(vrow) || !aligned16(qwin)) return CDFO_EALIGN;
  CdfoProfScope prof(static_cast<hipStream_t>(stream), KID_RDAB_PREP, 0, 4.0*(128+64+192)*(double)B*P);
  hipLaunchKernelGGL(rdab_prep_kernel<false>, dim3((unsigned)(B * P / 64)), dim3(256), 0, static_cast<hipStream_t>(stream), xq,
                     ldx, vmax, noise, wW, bW, P, sq, lds_, vrow, ldv, qwin, ldw, 0ull, 0u, nullptr, nullptr);
  CDFO_LAUNCH_CHECK();
  return 0;
}

// The same with the uniform noise drawn inside the kernel (Philox4x32-10 keyed by `seed`; `draw` numbers the call, so the
// draws of one forward are independent).  noise_out: optional [B][64][P] copy of the drawn values.
extern "C" int cdfo_rdab_prep_rng(const float* xq, int ldx, const float* vmax, long long seed, int draw, float* noise_out,
                                  const float* wW, const float* bW, int B, long long P, float* sq, int lds_, float* vrow,
                                  int ldv, float* qwin, int ldw, void* stream) {
  if (B <= 0 || P <= 0 || P % 64 || P >= (1ll << 32) || ldx % 4 || lds_ % 4 || ldv % 4 || ldw % 4) return CDFO_EINVAL;
  if (!aligned16(xq) || !aligned16(sq) || !aligned16(vrow) || !aligned16(qwin)) return CDFO_EALIGN;
  CdfoProfScope prof(static_cast<hipStream_t>(stream), KID_RDAB_PREP, 0, 4.0*(128+192)*(double)B*P);
  hipLaunchKernelGGL(rdab_prep_kernel<true>, dim3((unsigned)(B * P / 64)), dim3(256), 0, static_cast<hipStream_t>(stream), xq,
                     ldx, vmax, nullptr, wW, bW, P, sq, lds_, vrow, ldv, qwin, ldw, (unsigned long long)seed, (unsigned)draw,
                     noise_out, nullptr);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_rdab_prep_rng_dev(const float* xq, int ldx, const float* vmax, const void* seed_dev, int draw, float* noise_out,
                                      const float* wW, const float* bW, int B, long long P, float* sq, int lds_, float* vrow,
                                      int ldv, float* qwin, int ldw, void* stream) {
  if (B <= 0 || P <= 0 || P % 64 || P >= (1ll << 32) || ldx % 4 || lds_ % 4 || ldv % 4 || ldw % 4 || !seed_dev) return CDFO_EINVAL;
  if (!aligned16(xq) || !aligned16(sq) || !aligned16(vrow) || !aligned16(qwin) || (reinterpret_cast<uintptr_t>(seed_dev) & 7u)) return CDFO_EALIGN;
  CdfoProfScope prof(static_cast<hipStream_t>(stream), KID_RDAB_PREP, 0, 4.0*(128+192)*(double)B*P);
  hipLaunchKernelGGL(rdab_prep_kernel<true>, dim3((unsigned)(B * P / 64)), dim3(256), 0, static_cast<hipStream_t>(stream), xq,
                     ldx, vmax, nullptr, wW, bW, P, sq, lds_, vrow, ldv, qwin, ldw, 0ull, (unsigned)draw, noise_out,
                     static_cast<const unsigned long long*>(seed_dev));
  CDFO_LAUNCH_CHECK();
  return 0;
}

// RDAB.input_conv + rdab_prep in one launch (rdab_prep_kernel_fused): x [B][P][ldx >= 64] fp32, w_packed / bias the convolution's
// packed [16][128][4] weights and [128] bias (null: none).  noise != null: the injected [B][64][P] draws (cdfo_rdab_prep); else Philox
// with (seed_dev ? *seed_dev : seed, draw) and the optional noise_out (cdfo_rdab_prep_rng / _rng_dev).  v_f16 bit 0: vrow, bit 1: vwin
// (the v half of the product, which the two-kernel path reads from xq) is fp16 with its pitch in halves.  Results equal those of
// cdfo_conv1x1_bf16x3's streaming kernel followed by cdfo_rdab_prep* bit for bit (fp16: rounded once).
// plane != null: the PLANE form (cdfo_rdab_prep_fused_plane)
static int rdab_prep_fused_launch(const float* x, int ldx, const float* w_packed, const float* bias, const float* vmax,
                                  const float* noise, long long seed, const void* seed_dev, int draw, float* noise_out,
                                  const float* wW, const float* bW, int B, long long P, float* sq, int lds_, void* vrow, int ldv,
                                  float* qwin, int ldw, void* vwin, int ldvw, int v_f16, const pc_plane* plane, void* stream,
                                  const im_map* xm = nullptr) {
  if (xm && (!plane || !im_map_ok(*xm))) return CDFO_EINVAL;      // the mapped form exists beside the plane chunk only
  if (B <= 0 || P <= 0 || P % 64 || P >= (1ll << 32) || ldx < 64 || ldx % 4 || (long long)ldx * 4 * 32 >= (1ll << 31) || lds_ % 4 ||
      ldw % 4 || ldv % 8 || ldvw % 8 || !x || !w_packed || !vmax || !wW || !bW)
    return CDFO_EINVAL;
  if ((P + 127) / 128 > 0x7fffffff / 2) return CDFO_EINVAL;
  if (!aligned16(x) || !aligned16(w_packed) || !aligned16(sq) || !aligned16(vrow) || !aligned16(qwin) || !aligned16(vwin) ||
      (reinterpret_cast<uintptr_t>(seed_dev) & 7u))
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rf_args_map sm{};
  rf_args& s = sm;
  s.x = x; s.ldx = ldx; s.w = w_packed; s.bias = bias; s.vmax = vmax; s.noise = noise; s.wW = wW; s.bW = bW;
  s.P = P; s.ns = 3;
  s.sq = sq; s.lds_ = lds_; s.qwin = qwin; s.ldw = ldw; s.vrow = vrow; s.ldv = ldv; s.vwin = vwin; s.ldvw = ldvw;
  s.seed = (unsigned long long)seed; s.draw = (unsigned)draw; s.noise_out = noise ? nullptr : noise_out;
  s.seed_dev = static_cast<const unsigned long long*>(seed_dev);
  int grid;
  if (!st_tiling(B, P, s.tiles_per_image, s.tiles, grid)) return CDFO_EINVAL;
  const int lds = st_lds_bytes(1, 2, s.ns) + 64 * 4 + (plane ? pc_lds_bytes(2, s.ns) : 0);
  const double px = (double)B * P;
  if (v_f16 < 0 || v_f16 > 3) return CDFO_EINVAL;
  // (the plane chunk: one k-step of 16 and 4 bytes per pixel more)
  CdfoProfScope prof(st, KID_RDAB_PREP, 2.0 * px * 128 * (plane ? 80 : 64),
                     px * (4.0 * (64 + 128 + (noise ? 64 : 0) + (plane ? 1 : 0)) + ((v_f16 & 1) ? 2.0 : 4.0) * 64 + ((v_f16 & 2) ? 2.0 : 4.0) * 64));
  static CdfoAttrOnce once[8], once_pl[8], once_map[8];
  typedef _Float16 h;
  if (xm) {
    s.plane = *plane;
    sm.x_map = *xm;
    switch ((noise ? 0 : 4) + v_f16) {
      case 0: return st_launch(rdab_prep_kernel_fused<false, float, float, true, true>, once_map[0], grid, lds, st, sm);
      case 1: return st_launch(rdab_prep_kernel_fused<false, h, float, true, true>, once_map[1], grid, lds, st, sm);
      case 2: return st_launch(rdab_prep_kernel_fused<false, float, h, true, true>, once_map[2], grid, lds, st, sm);
      case 3: return st_launch(rdab_prep_kernel_fused<false, h, h, true, true>, once_map[3], grid, lds, st, sm);
      case 4: return st_launch(rdab_prep_kernel_fused<true, float, float, true, true>, once_map[4], grid, lds, st, sm);
      case 5: return st_launch(rdab_prep_kernel_fused<true, h, float, true, true>, once_map[5], grid, lds, st, sm);
      case 6: return st_launch(rdab_prep_kernel_fused<true, float, h, true, true>, once_map[6], grid, lds, st, sm);
      default: return st_launch(rdab_prep_kernel_fused<true, h, h, true, true>, once_map[7], grid, lds, st, sm);
    }
  }
  if (plane) {
    s.plane = *plane;
    switch ((noise ? 0 : 4) + v_f16) {
      case 0: return st_launch(rdab_prep_kernel_fused<false, float, float, true>, once_pl[0], grid, lds, st, s);
      case 1: return st_launch(rdab_prep_kernel_fused<false, h, float, true>, once_pl[1], grid, lds, st, s);
      case 2: return st_launch(rdab_prep_kernel_fused<false, float, h, true>, once_pl[2], grid, lds, st, s);
      case 3: return st_launch(rdab_prep_kernel_fused<false, h, h, true>, once_pl[3], grid, lds, st, s);
      case 4: return st_launch(rdab_prep_kernel_fused<true, float, float, true>, once_pl[4], grid, lds, st, s);
      case 5: return st_launch(rdab_prep_kernel_fused<true, h, float, true>, once_pl[5], grid, lds, st, s);
      case 6: return st_launch(rdab_prep_kernel_fused<true, float, h, true>, once_pl[6], grid, lds, st, s);
      default: return st_launch(rdab_prep_kernel_fused<true, h, h, true>, once_pl[7], grid, lds, st, s);
    }
  }
  switch ((noise ? 0 : 4) + v_f16) {
    case 0: return st_launch(rdab_prep_kernel_fused<false, float, float>, once[0], grid, lds, st, s);
    case 1: return st_launch(rdab_prep_kernel_fused<false, h, float>, once[1], grid, lds, st, s);
    case 2: return st_launch(rdab_prep_kernel_fused<false, float, h>, once[2], grid, lds, st, s);
    case 3: return st_launch(rdab_prep_kernel_fused<false, h, h>, once[3], grid, lds, st, s);
    case 4: return st_launch(rdab_prep_kernel_fused<true, float, float>, once[4], grid, lds, st, s);
    case 5: return st_launch(rdab_prep_kernel_fused<true, h, float>, once[5], grid, lds, st, s);
    case 6: return st_launch(rdab_prep_kernel_fused<true, float, h>, once[6], grid, lds, st, s);
    default: return st_launch(rdab_prep_kernel_fused<true, h, h>, once[7], grid, lds, st, s);
  }
}

extern "C" int cdfo_colconv9(const float* in, int ldi, const float* wH, const float* bH, int B, int H, int W, float* out,
                             int ldo, void* stream) {
  if (B <= 0 || ldi % 4 || ldo % 4) return CDFO_EINVAL;
  if (!aligned16(in) || !aligned16(out)) return CDFO_EALIGN;
  const int nseg = cdiv(H, CC9_SEG);
  long long blocks = ((long long)B * nseg * W * 16 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  CdfoProfScope prof(static_cast<hipStream_t>(stream), KID_COLCONV9, 0, 4.0*128*(double)B*H*W);
  hipLaunchKernelGGL(colconv9_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), in, ldi, wH,
                     bH, B, H, W, nseg, out, ldo);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_seq_attn(const float* q, int ldq, const float* v, int ldv, float* out, int ldo, int B, int H, int W,
                             int mode, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || ldq % 4 || ldv % 4 || ldo % 4) return CDFO_EINVAL;
  if (!aligned16(q) || !aligned16(v) || !aligned16(out)) return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(static_cast<hipStream_t>(stream), (mode%10)==0?KID_ATTN_ROW:((mode%10)==1?KID_ATTN_COL:KID_ATTN_WIN), 4.0*64*(double)B*H*W*((mode%10)==0?W:((mode%10)==1?H:64)), 4.0*192*(double)B*H*W);
  const bool pv1 = mode >= 20 && mode <= 22;           // modes 20 / 21 / 22: modes 0 / 1 / 2 with the single-fp16 second product (PV1)
  if (pv1) mode -= 20;
  if (mode == 0 || mode == 1) {
    const bool wide = seq_attn_wide(mode == 0 ? W : H);
    int rc;
    if (pv1) rc = mode == 0 ? seq_attn_pv1<0>(q, ldq, v, ldv, out, ldo, B, H, W, st) : seq_attn_pv1<1>(q, ldq, v, ldv, out, ldo, B, H, W, st);
    else if (mode == 0) rc = !wide ? seq_attn_launch<0, 4>(q, ldq, v, ldv, out, ldo, B, H, W, st)
                                     : seq_attn_launch<0, 8>(q, ldq, v, ldv, out, ldo, B, H, W, st);
    else rc = !wide ? seq_attn_launch<1, 4>(q, ldq, v, ldv, out, ldo, B, H, W, st)
                    : seq_attn_launch<1, 8>(q, ldq, v, ldv, out, ldo, B, H, W, st);
    if (rc) return rc;
  } else if (mode == 10) {   // VALU reference forms of modes 0 / 1 (kept for A/B tests)
    hipLaunchKernelGGL(seq_attn_kernel<0>, dim3((unsigned)((long long)B * H * cdiv(W, 64))), dim3(64), 0, st, q, ldq, v,
                       ldv, out, ldo, B, H, W);
  } else if (mode == 11) {
    hipLaunchKernelGGL(seq_attn_kernel<1>, dim3((unsigned)((long long)B * W * cdiv(H, 64))), dim3(64), 0, st, q, ldq, v,
                       ldv, out, ldo, B, H, W);
  } else if (mode == 2) {
    if ((H & 7) || (W & 7)) return CDFO_EINVAL;
    const int rc = pv1 ? seq_attn_pv1<2>(q, ldq, v, ldv, out, ldo, B, H, W, st)
                       : seq_attn_launch<2, 4>(q, ldq, v, ldv, out, ldo, B, H, W, st);
    if (rc) return rc;
  } else if (mode == 12) {   // VALU reference form of mode 2
    if ((H & 7) || (W & 7)) return CDFO_EINVAL;
    hipLaunchKernelGGL(seq_attn_kernel<2>, dim3((unsigned)((long long)B * (H / 8) * (W / 8))), dim3(64), 0, st, q, ldq, v,
                       ldv, out, ldo, B, H, W);
  } else {
    return CDFO_EINVAL;
  }
  CDFO_LAUNCH_CHECK();
  return 0;
}

// Modes 20 / 21 / 22 with 16-bit operands: v_f16: V is fp16 [.,ldv] (ldv in halves) holding (_Float16)v -- the rounding the fp32
// form applies while staging, so the result is the same bit for bit; out_f16 (mode 20 only): the output as (_Float16)result, the V
// operand of the column attention that follows.  With neither flag this is cdfo_seq_attn.
extern "C" int cdfo_seq_attn_f16(const float* q, int ldq, const void* v, int ldv, void* out, int ldo, int B, int H, int W, int mode,
                                 int v_f16, int out_f16, void* stream) {
  if (!v_f16 && !out_f16)
    return cdfo_seq_attn(q, ldq, static_cast<const float*>(v), ldv, static_cast<float*>(out), ldo, B, H, W, mode, stream);
  if (mode < 20 || mode > 22 || (out_f16 && mode != 20)) return CDFO_EINVAL;
  if (B <= 0 || H <= 0 || W <= 0 || ldq % 4 || ldv % (v_f16 ? 8 : 4) || ldo % 4) return CDFO_EINVAL;
  if (mode == 22 && ((H & 7) || (W & 7))) return CDFO_EINVAL;
  if (!aligned16(q) || !aligned16(v) || (reinterpret_cast<uintptr_t>(out) & (out_f16 ? 7u : 15u)))
    return CDFO_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int L = mode == 20 ? W : (mode == 21 ? H : 64);
  CdfoProfScope prof(st, mode == 20 ? KID_ATTN_ROW : (mode == 21 ? KID_ATTN_COL : KID_ATTN_WIN), 4.0 * 64 * (double)B * H * W * L,
                     (4.0 * 64 + (v_f16 ? 2.0 : 4.0) * 64 + (out_f16 ? 2.0 : 4.0) * 64) * (double)B * H * W);
  const _Float16* vh = static_cast<const _Float16*>(v);
  const float* vf = static_cast<const float*>(v);
  int rc;
  if (mode == 20) {
    if (v_f16) rc = out_f16 ? seq_attn_pv1<0>(q, ldq, vh, ldv, static_cast<_Float16*>(out), ldo, B, H, W, st)
                            : seq_attn_pv1<0>(q, ldq, vh, ldv, static_cast<float*>(out), ldo, B, H, W, st);
    else rc = seq_attn_pv1<0>(q, ldq, vf, ldv, static_cast<_Float16*>(out), ldo, B, H, W, st);
  } else if (mode == 21) rc = seq_attn_pv1<1>(q, ldq, vh, ldv, static_cast<float*>(out), ldo, B, H, W, st);
  else rc = seq_attn_pv1<2>(q, ldq, vh, ldv, static_cast<float*>(out), ldo, B, H, W, st);
  if (rc) return rc;
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_rdab_prep_fused(const float* x, int ldx, const float* w_packed, const float* bias, const float* vmax,
                                    const float* noise, long long seed, const void* seed_dev, int draw, float* noise_out,
                                    const float* wW, const float* bW, int B, long long P, float* sq, int lds_, void* vrow, int ldv,
                                    float* qwin, int ldw, void* vwin, int ldvw, int v_f16, void* stream) {
  return rdab_prep_fused_launch(x, ldx, w_packed, bias, vmax, noise, seed, seed_dev, draw, noise_out, wW, bW, B, P, sq, lds_, vrow, ldv,
                                qwin, ldw, vwin, ldvw, v_f16, nullptr, stream);
}

// cdfo_rdab_prep_fused on x + stencil9(plane; w_s, b_s) with only x in memory: image b's plane (W pixels per row, P / W rows, dense
// fp32) at plane + (b % plane_Bi) plane_sb + (b / plane_Bi) plane_sg floats; plane_w [128][16] = input_conv . [w_s | b_s] | zeros
extern "C" int cdfo_rdab_prep_fused_plane(const float* x, int ldx, const float* w_packed, const float* bias, const float* vmax,
                                          const float* noise, long long seed, const void* seed_dev, int draw, float* noise_out,
                                          const float* wW, const float* bW, int B, long long P, float* sq, int lds_, void* vrow,
                                          int ldv, float* qwin, int ldw, void* vwin, int ldvw, int v_f16, const float* plane,
                                          int plane_Bi, long long plane_sb, long long plane_sg, int W, const float* plane_w,
                                          void* stream) {
  if (!plane || !plane_w || plane_Bi <= 0 || plane_sb < 0 || plane_sg < 0 || !pc_shape_ok(P, W)) return CDFO_EINVAL;
  if (!aligned16(plane_w)) return CDFO_EALIGN;
  const pc_plane pl = {plane, plane_Bi, plane_sb, plane_sg, W, plane_w, 0};
  return rdab_prep_fused_launch(x, ldx, w_packed, bias, vmax, noise, seed, seed_dev, draw, noise_out, wW, bW, B, P, sq, lds_, vrow, ldv,
                                qwin, ldw, vwin, ldvw, v_f16, &pl, stream);
}

// cdfo_rdab_prep_fused_plane with x read through an image map: image b of x starts at x + (b % x_Bi) x_sb + (b / x_Bi) x_sg floats
// (image_map.h).  Same results bit for bit as on the dense copy of those images.
extern "C" int cdfo_rdab_prep_fused_plane_map(const float* x, int ldx, int x_Bi, long long x_sb, long long x_sg, const float* w_packed,
                                              const float* bias, const float* vmax, const float* noise, long long seed,
                                              const void* seed_dev, int draw, float* noise_out, const float* wW, const float* bW, int B,
                                              long long P, float* sq, int lds_, void* vrow, int ldv, float* qwin, int ldw, void* vwin,
                                              int ldvw, int v_f16, const float* plane, int plane_Bi, long long plane_sb,
                                              long long plane_sg, int W, const float* plane_w, void* stream) {
  if (!plane || !plane_w || plane_Bi <= 0 || plane_sb < 0 || plane_sg < 0 || !pc_shape_ok(P, W)) return CDFO_EINVAL;
  if (!aligned16(plane_w)) return CDFO_EALIGN;
  const pc_plane pl = {plane, plane_Bi, plane_sb, plane_sg, W, plane_w, 0};
  const im_map xm = {x_Bi, x_sb, x_sg};
  return rdab_prep_fused_launch(x, ldx, w_packed, bias, vmax, noise, seed, seed_dev, draw, noise_out, wW, bW, B, P, sq, lds_, vrow, ldv,
                                qwin, ldw, vwin, ldvw, v_f16, &pl, stream, &xm);
}
