// Training batches and the training loss on the device (cdfo_amd/train_data.py, cdfo_amd/loss.py): what the reference does on the
// host per step -- RandomCrop -> Augment -> ToTensor in DataLoader workers (opt/data_LD_bi.py:245-505), eight .to(device) copies,
// the permutes and /32 of train_LD_37.py:365-374, and a six-operator Charbonnier expression (opt/loss.py:20-31) -- as three entry points.
//
//   cdfo_train_batch   the clip set is resident ([S][T] 8-bit planes); one launch cuts, flips, transposes and converts B samples.
//                      Plan row b = (seq, first, top, left, hflip, vflip, rot, 0).  For an n x n output plane (n = crop; the HR
//                      plane: n = 4 crop, origin (4 top, 4 left)):
//                          out[y][x] = P[top + i'][left + j'] / 255,  (i, j) = rot ? (x, y) : (y, x),  i' = vflip ? n-1-i : i,
//                          j' = hflip ? n-1-j : j,
//                      the division correctly rounded (a product with a rounded reciprocal differs by an ulp).  The motion field
//                      of frame first + 3, components (a, b, ref), goes through the same index map: m0 = b, m1 = a; hflip
//                      negates m0, vflip m1, rot swaps them; p = m / (ref * -1), NaN -> 0.  AN INFINITY STAYS: the reference
//                      keeps x / 0, and so does cdfo_seq_flows.  Slot k of the seven holds fl(p * w_k) / 128,
//                      w = 3, 2, 1, 0, -1, -2, -3 (the reference's / 4 and / 32 are exact); slot 3 is +0 whatever p.
//   cdfo_train_batch_ra  the random-access form (opt/data_RA_bi.py:495-533, train_RA_37.py:383-386): the set also holds mvl1, and the
//                      field is built from both lists.  Planes, grid and work list are cdfo_train_batch's; the motion tile reads both
//                      fields of frame first + 3 through the same index map and the same m0 / m1 rules, then per pixel
//                          p2 = m(list 0) / (ref0 * -1),  p4 = m(list 1) / ref1        NaN -> +0, an infinity stays
//                          ref0 == -99: p2 = -p4;   then ref1 == -99: p4 = -p2         (both marked: p4 stays, p2 = -p4)
//                      (a list stands in for the other where a block has no reference in it; the negations make -0 and the
//                      reference's output carries them).  Slots 0, 1, 2 hold fl(p2 * w) / 128, w = 3, 2, 1; slot 3 is +0; slots 4, 5,
//                      6 hold fl(p4 * w) / 128, w = 1, 2, 3.  The reference's second field is the same array (mvl1s_7 = mvl0s_7): one
//                      output serves both.
//   cdfo_charbonnier   one pass over sr and hr: g = d / sqrt(d^2 + eps) and fp64 partial sums of sqrt(d^2 + eps) per workgroup; a
//                      one-wave kernel adds the partials in a fixed order.  No atomics: equal inputs give equal bits.
//
// Shape of cdfo_train_batch.  Grid (tile work list, sample): per sample 28 LR-sized planes, the HR plane and the motion field, cut
// into 32 x 32 output tiles.  The plan row is read through wave-uniform loads (its address depends on blockIdx alone).  Every tile
// goes through an LDS tile padded to 33 floats a row: the SOURCE tile is read along source rows (byte loads, no alignment assumed:
// `left` and W are arbitrary), converted once, and written in source order; the OUTPUT tile is read back through the index map --
// along LDS rows, or down LDS columns when rot transposes, both conflict-free at pitch 33 -- and leaves as 16-byte stores along
// output rows (crop % 4 == 0 makes every output row 16-byte aligned).  A plan row that does not fit the clip set writes nothing:
// the host validates plans (ClipSet.batch), the check in the kernel is the net under a wrong one.  Both forms are one kernel
// template (train_batch.h) that differs in the motion tile alone; the RA form stages four planes (p2 and p4, two components each:
// 16.9 KB) instead of two.  This file instantiates the LD form only and train_batch_ra.hip the RA form: with both in one module the
// compiler addresses the LD form's LDS tile with other instructions, and that kernel's code is to stay what it was.
#include "train_batch.h"

namespace {

// ---------------------------------------------------------------------------------------------------------- cdfo_charbonnier
__global__ __launch_bounds__(256) void charbonnier_kernel(const float* __restrict__ sr, const float* __restrict__ hr, long long n,
                                                          float eps, int vec, float* __restrict__ g, double* __restrict__ partial) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * 1024) {
    const int cnt = n - i < 4 ? (int)(n - i) : 4;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (vec && cnt == 4) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(sr + i), vb = *reinterpret_cast<const f32x4*>(hr + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) { a[q] = va[q]; b[q] = vb[q]; }
    } else {
      for (int q = 0; q < cnt; ++q) { a[q] = sr[i + q]; b[q] = hr[i + q]; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = a[q] - b[q];
      const float t = __fsqrt_rn(d * d + eps);                // correctly rounded: no fast reciprocal square root
      o[q] = __fdiv_rn(d, t);
      if (q < cnt) acc += (double)t;
    }
    if (vec && cnt == 4) {
      const f32x4 vo = {o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(g + i) = vo;
    } else {
      for (int q = 0; q < cnt; ++q) g[i + q] = o[q];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one wave: lane l adds partials l, l + 64, ... in order, then the xor tree: a fixed order
__global__ __launch_bounds__(64) void charbonnier_sum_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 64) acc += partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (threadIdx.x == 0) *loss = (float)acc;
}

}  // namespace

extern "C" int cdfo_train_batch(const unsigned char* lr, const unsigned char* pms, const signed char* rms, const unsigned char* ufs,
                                const signed char* mvl0, const unsigned char* hr, int S, int T, int H, int W, int Hu, const int* plan,
                                int B, int crop, float* x, float* pms_out, float* rms_out, float* ufs_out, float* mvs0, float* hr_out,
                                void* stream) {
  BatchArgs a;
  unsigned work;
  if (const int st = train_batch_args(lr, pms, rms, ufs, mvl0, hr, S, T, H, W, Hu, plan, B, crop, x, pms_out, rms_out, ufs_out, mvs0, hr_out,
                                      a, work))
    return st;
  hipLaunchKernelGGL(train_batch_kernel<false>, dim3(work, B), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     static_cast<const signed char*>(nullptr));
  CDFO_LAUNCH_CHECK();
  return 0;
}

// a fixed function of n: the grid, and with it the order of the sum, never depends on the device
static int charbonnier_blocks(long long n) {
  const long long blocks = (n + 1023) / 1024;
  return (int)(blocks < CDFO_CHARBONNIER_MAX_BLOCKS ? blocks : CDFO_CHARBONNIER_MAX_BLOCKS);
}

extern "C" int cdfo_charbonnier(const float* sr, const float* hr, long long n, float eps, float* grad, double* partial, int partial_cap,
                                float* loss, void* stream) {
  if (!sr || !hr || !grad || !partial || !loss || n <= 0 || !(eps >= 0.f)) return CDFO_EINVAL;
  const int blocks = charbonnier_blocks(n);
  if (partial_cap < blocks) return CDFO_EINVAL;
  if ((reinterpret_cast<uintptr_t>(sr) | reinterpret_cast<uintptr_t>(hr) | reinterpret_cast<uintptr_t>(grad) |
       reinterpret_cast<uintptr_t>(loss)) & 3u || (reinterpret_cast<uintptr_t>(partial) & 7u))
    return CDFO_EALIGN;
  const int vec = aligned16(sr) && aligned16(hr) && aligned16(grad);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(charbonnier_kernel, dim3(blocks), dim3(256), 0, st, sr, hr, n, eps, vec, grad, partial);
  CDFO_LAUNCH_CHECK();
  hipLaunchKernelGGL(charbonnier_sum_kernel, dim3(1), dim3(64), 0, st, partial, blocks, loss);
  CDFO_LAUNCH_CHECK();
  return 0;
}
