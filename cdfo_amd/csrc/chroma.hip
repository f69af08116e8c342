// The chroma side of YUV 4:2:0 evaluation (cdfo_amd/evaluate.py: evaluate_yuv): the two chroma planes of a frame never pass through the
// model; they are upsampled x4 here, on 8-bit planes, by a filter defined in integers so that its numpy statement is bit-exact.
//
//   cdfo_chroma_up4   N 8-bit planes [h][w], read in place through a row pitch and a plane stride, -> N dense 8-bit planes [4h][4w];
//                     optionally the PSNR numerator sum (out - gt)^2 against 8-bit ground truth in the same pass, as exact integers.
//
// The filter: centre-aligned x4 Catmull-Rom.  Output index j = 4q + r samples the source at q + (2r - 3) / 8, i.e. at fraction 5/8,
// 7/8 (between q-1 and q) for r = 0, 1 and 1/8, 3/8 (between q and q+1) for r = 2, 3; four taps from q-2 (r = 0, 1) or q-1 (r = 2, 3),
// indices clamped to the plane, coefficients out of 128 (each row sums to 128):
//     r = 0: (-6, 50, 93, -9)    r = 1: (-1, 12, 123, -6)    r = 2: (-6, 123, 12, -1)    r = 3: (-9, 93, 50, -6)
// x and y passes in 32-bit integers without intermediate rounding (|horizontal| <= 255 * 158, |both| <= 255 * 158^2 < 2^23), then
// clamp((v + 8192) >> 14, 0, 255) with an arithmetic shift.
//
// Bandwidth-bound (1 byte in, 16 out, 16 more with ground truth, per source pixel).  A workgroup takes a tile of 32 x 16 source
// pixels: the tile and its 2-pixel halo go to LDS once (clamped coordinates: a ragged tile reads nothing outside the plane), the
// horizontal pass writes 20 rows of 128 ints to LDS, the vertical pass reads five 16-byte rows of them per thread and stores the
// 4 x 4 outputs of one source pixel as four aligned words (4w is a multiple of 4, the planes are packed).  No atomics: per-block partials.
//
//   cdfo_chroma_up4_u16   the same filter on 16-bit samples of a peak of 1 .. 65535 (10-, 12-, 16-bit material): the kernel is a template
//                         on the sample type, the clamp is to [0, peak], a word of four outputs is 64 bits.  The 32-bit sums still hold:
//                         |both passes| <= 65535 * 158^2 = 1 636 015 740 < 2^31 - 8192.
#include "common.h"
#include "numeric.h"

namespace {

constexpr int CU_TW = 32, CU_TH = 16;                   // source pixels of one tile
constexpr int CU_IW = CU_TW + 4, CU_IH = CU_TH + 4;     // with the halo: source q-2 .. q+2 feeds outputs 4q .. 4q+3


// the four outputs 4q .. 4q+3 from the five sources q-2 .. q+2, scaled by 128
__device__ __forceinline__ i32x4 up4_taps(int a, int b, int c, int d, int e) {
  return i32x4{-6 * a + 50 * b + 93 * c - 9 * d, -1 * a + 12 * b + 123 * c - 6 * d, -6 * b + 123 * c + 12 * d - 1 * e,
               -9 * b + 93 * c + 50 * d - 6 * e};
}

// grid (x: workgroups striding over the plane's tiles; y: plane).  Offsets inside a plane are 32-bit (host guard).
// gt_words: the ground truth can be read in aligned 32-bit words (1: pointer, pitch and plane stride multiples of 4 bytes) or, 16-bit
// samples, in aligned 64-bit words (2: multiples of 8 bytes); 0: per element.  peak: read by the 16-bit form only.
template <typename T>
__global__ __launch_bounds__(256) void chroma_up4_kernel(const T* __restrict__ src, int src_pitch, long long src_pstride,
                                                         int h, int w, T* __restrict__ dst,
                                                         const T* __restrict__ gt, int gt_pitch, long long gt_pstride,
                                                         int gt_words, int Hm, int Wm, int crop, long long* __restrict__ partial, int peak) {
  typedef typename gt_word<T>::type word_t;              // four outputs: 32 bits of 8-bit samples, 64 bits of 16-bit samples
  constexpr int BITS = 8 * sizeof(T);
  __shared__ long long sh[4];
  __shared__ T tile[CU_IH][CU_IW];
  __shared__ i32x4 hp[CU_IH][CU_TW];                     // horizontal pass: 20 x 32 x 16 = 10240 bytes
  const int n = blockIdx.y;
  const int top = sizeof(T) == 1 ? 255 : peak;
  const T* s = src + (long long)n * src_pstride;
  word_t* d = reinterpret_cast<word_t*>(dst + (long long)n * 16 * h * w);   // a row of 4w pixels is w words
  const T* g = gt ? gt + (long long)n * gt_pstride : nullptr;
  const int tx_n = (w + CU_TW - 1) / CU_TW, ty_n = (h + CU_TH - 1) / CU_TH;
  long long sse = 0;
  for (int t = blockIdx.x; t < tx_n * ty_n; t += gridDim.x) {
    const int y0 = (t / tx_n) * CU_TH, x0 = (t % tx_n) * CU_TW;                // source coordinates of the tile
    __syncthreads();                                                            // the previous tile's passes are done
    for (int i = threadIdx.x; i < CU_IH * CU_IW; i += 256) {
      const int r = i / CU_IW, c = i - r * CU_IW;
      const int y = min(max(y0 - 2 + r, 0), h - 1), x = min(max(x0 - 2 + c, 0), w - 1);   // edge replication
      tile[r][c] = s[y * src_pitch + x];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CU_IH * CU_TW; i += 256) {
      const int r = i / CU_TW, c = i - r * CU_TW;
      hp[r][c] = up4_taps(tile[r][c], tile[r][c + 1], tile[r][c + 2], tile[r][c + 3], tile[r][c + 4]);
    }
    __syncthreads();
    // one trip: the four output rows of source row r at word column c (outputs 4(x0+c) .. +3 of rows 4(y0+r) .. +3)
    for (int i = threadIdx.x; i < CU_TH * CU_TW; i += 256) {
      const int r = i / CU_TW, c = i - r * CU_TW;
      const int q = x0 + c;
      if (y0 + r >= h || q >= w) continue;
      const i32x4 a = hp[r][c], b = hp[r + 1][c], m = hp[r + 2][c], e = hp[r + 3][c], f = hp[r + 4][c];
      word_t word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const i32x4 v = up4_taps(a[k], b[k], m[k], e[k], f[k]);                // the four rows of output column 4q + k
#pragma unroll
        for (int j = 0; j < 4; ++j) word[j] |= (word_t)(unsigned)min(max((v[j] + 8192) >> 14, 0), top) << (BITS * k);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int oy = 4 * (y0 + r) + j;
        d[oy * w + q] = word[j];
        if (g && oy >= crop && oy < Hm - crop) {
          const int ox = 4 * q;
          if (ox + 3 < crop || ox >= Wm - crop) continue;
          const T* row = g + oy * gt_pitch;
          // a word starts inside the row (ox < Wm <= Wgt <= pitch, both multiples of the word's pixels => its last pixel < pitch);
          // the second 32-bit word of 16-bit samples is read only where a wanted pixel lies in it (ox + 2 < Wm - crop <= pitch)
          const word_t gw = load_gt_word(row + ox, gt_words, ox + 2 < Wm - crop);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int xe = ox + k;
            if (xe >= crop && xe < Wm - crop) {
              const unsigned ref = gt_words ? (unsigned)((gw >> (BITS * k)) & ((1u << BITS) - 1u)) : (unsigned)row[xe];
              sse += sqdiff<T>((unsigned)((word[j] >> (BITS * k)) & ((1u << BITS) - 1u)), ref);
            }
          }
        }
      }
    }
  }
  if (partial) {
    sse = block_sum_i64(sse, sh);
    if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = sse;
  }
}

inline bool fits32(long long rows, long long pitch) { return rows * pitch <= 0x7fffffffLL; }

// cdfo_chroma_up4 (T = unsigned char, peak 255) and cdfo_chroma_up4_u16 (T = unsigned short)
template <typename T>
int chroma_up4(const T* src, int src_pitch, long long src_pstride, int N, int h, int w, T* dst, int peak, const T* gt, int gt_pitch,
               long long gt_pstride, int Hgt, int Wgt, int crop, long long* partial, int partial_cap, int* nblocks_out, void* stream) {
  constexpr int S = sizeof(T);
  if (!src || !dst || N <= 0 || N > 65535 || h <= 0 || w <= 0 || src_pitch < w || src_pstride < 0 || peak < 1 ||
      peak > (1 << (8 * S)) - 1)
    return CDFO_EINVAL;
  if (!fits32(h, src_pitch) || !fits32(4LL * h, 4LL * w)) return CDFO_EINVAL;                 // 32-bit offsets inside a plane
  int Hm = 0, Wm = 0;
  if (gt) {
    if (!partial || !nblocks_out || Hgt <= 0 || Wgt <= 0 || gt_pitch < Wgt || gt_pstride < 0 || crop < 0 || !fits32(Hgt, gt_pitch))
      return CDFO_EINVAL;
    Hm = 4 * h < Hgt ? 4 * h : Hgt;                            // psnr_ssim.py:462-468: min_height / min_width
    Wm = 4 * w < Wgt ? 4 * w : Wgt;
    if (Hm - 2 * crop <= 0 || Wm - 2 * crop <= 0) return CDFO_EINVAL;
  }
  // dst: a word of four outputs (8-bit), 16 bytes (16-bit, as cdfo_finish_frames_u16's); 16-bit sources and ground truth: 2 bytes
  if ((reinterpret_cast<uintptr_t>(dst) & (S == 1 ? 3u : 15u)) || (gt && (reinterpret_cast<uintptr_t>(partial) & 7u)) ||
      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(gt)) & (S - 1)))
    return CDFO_EALIGN;
  long long blocks = (long long)cdiv(w, CU_TW) * cdiv(h, CU_TH);
  if (blocks > 1024) blocks = 1024;
  if (gt) {
    if ((long long)N * blocks > partial_cap) return CDFO_EINVAL;
    *nblocks_out = (int)blocks;
  }
  // in units of the word: pointer, pitch and plane stride (a multiple of 4 / S or 8 / S samples)
  auto words_of = [&](int bytes) {
    return gt && (reinterpret_cast<uintptr_t>(gt) & (bytes - 1)) == 0 && gt_pitch % (bytes / S) == 0 && gt_pstride % (bytes / S) == 0;
  };
  const int gt_words = (S == 2 && words_of(8)) ? 2 : words_of(4) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  CdfoProfScope prof(st, KID_LAYOUT, 0, (double)N * h * w * S * (gt ? 33.0 : 17.0));
  hipLaunchKernelGGL(chroma_up4_kernel<T>, dim3((unsigned)blocks, (unsigned)N), dim3(256), 0, st, src, src_pitch, src_pstride, h, w, dst,
                     gt, gt_pitch, gt_pstride, gt_words, Hm, Wm, crop, gt ? partial : nullptr, peak);
  CDFO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int cdfo_chroma_up4(const unsigned char* src, int src_pitch, long long src_pstride, int N, int h, int w, unsigned char* dst,
                               const unsigned char* gt, int gt_pitch, long long gt_pstride, int Hgt, int Wgt, int crop,
                               long long* partial, int partial_cap, int* nblocks_out, void* stream) {
  return chroma_up4<unsigned char>(src, src_pitch, src_pstride, N, h, w, dst, 255, gt, gt_pitch, gt_pstride, Hgt, Wgt, crop, partial,
                                   partial_cap, nblocks_out, stream);
}

extern "C" int cdfo_chroma_up4_u16(const unsigned short* src, int src_pitch, long long src_pstride, int N, int h, int w,
                                   unsigned short* dst, int peak, const unsigned short* gt, int gt_pitch, long long gt_pstride, int Hgt,
                                   int Wgt, int crop, long long* partial, int partial_cap, int* nblocks_out, void* stream) {
  return chroma_up4<unsigned short>(src, src_pitch, src_pstride, N, h, w, dst, peak, gt, gt_pitch, gt_pstride, Hgt, Wgt, crop, partial,
                                    partial_cap, nblocks_out, stream);
}
