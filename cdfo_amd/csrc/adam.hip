// Adam on the device (cdfo_amd/optim.py: DeviceAdam; DESIGN.md "Adam on the device"): the gradient norm, the step's scalars and the
// update, three launches and no host read.  The moments of all parameters live in one fp32 buffer m and one fp32 buffer v; parameter
// t owns [offset_t, offset_t + n_t) of both, offset_t a multiple of 4.  Parameters and gradients stay the caller's tensors:
//     table   [T][4] int64: (p, g, offset, n) of every tensor, on the device; the caller also hands the host copy it uploaded, which is
//             what the entry points validate (a device table cannot be checked without a read)
//     chunks  [C][2] int32: (tensor, first element) of every run of at most CDFO_ADAM_CHUNK elements, first a multiple of the chunk
// A workgroup of 256 threads takes one chunk; thread i owns the float4 groups i, i + 256, i + 512, i + 768 of it and, for i < n mod 4,
// element i of the chunk's tail.  That assignment is the same in the 16-byte path and in the scalar path of an unaligned view.
//
//   cdfo_grad_norm_partials  partials[c] = sum of g^2 over chunk c in fp64: the thread's elements in index order (the product of two
//                            fp32 values is exact in fp64, so each step is one rounding), the wave's xor tree, the four waves in order.
//   cdfo_adam_scalars        one workgroup: thread i adds the partials [i k, (i + 1) k), k = ceil(C / 256), in index order; xor tree;
//                            waves in order.  Thread 0 then writes the scalar block and advances `step` or `skipped`:
//                              scalars[0] norm = sqrt(sum)          [1] coef, rounded to fp32       [2] step_size = lr / (1 - b1^step)
//                              [3] 1 / sqrt(1 - b2^step)            [4] skip = !isfinite(sum)       [5] sum of norm over unskipped steps
//                            On a skip [1..3] keep their values.
//   cdfo_adam_step           returns at once when scalars[4] is set; else the single-tensor statement of torch.optim.Adam per element
//                            in fp32 (L2 weight decay, no amsgrad).  g is not written.
// No atomics; every grid is a function of the sizes alone; equal inputs give equal bits.
#include "common.h"
#include <limits.h>

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = CDFO_ADAM_CHUNK;
constexpr int ADAM_VECS = ADAM_CHUNK / 4 / ADAM_THREADS;               // float4 groups of a thread
static_assert(ADAM_VECS * 4 * ADAM_THREADS == ADAM_CHUNK, "a chunk is a whole number of float4 groups per thread");

struct AdamTensor { float* p; const float* g; long long offset; long long n; };
static_assert(sizeof(AdamTensor) == 32, "a table row is four 64-bit words");

__device__ __forceinline__ bool dev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// chunk c of the table -> its tensor and its length; 0 for a row that does not lie inside its tensor (nothing is then touched)
__device__ __forceinline__ int chunk_of(const AdamTensor* __restrict__ table, int ntensors, const int2 c, AdamTensor& t) {
  if (c.x < 0 || c.x >= ntensors || c.y < 0) return 0;
  t = table[c.x];
  const long long left = t.n - (long long)c.y;
  if (left <= 0) return 0;
  return left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
}

__device__ __forceinline__ float4 load4(const float* __restrict__ base, int i, bool vec) {
  if (vec) return reinterpret_cast<const float4*>(base)[i];
  const float* q = base + 4 * i;
  return make_float4(q[0], q[1], q[2], q[3]);
}

__device__ __forceinline__ double sq_add(double acc, float g) {
  const double d = (double)g;
  return acc + d * d;
}

// the four waves' sums in wave order, valid in thread 0
__device__ __forceinline__ double block_sum(double acc, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(ADAM_THREADS) void grad_norm_kernel(const AdamTensor* __restrict__ table, int ntensors,
                                                                const int2* __restrict__ chunks, double* __restrict__ partials) {
  __shared__ double sh[ADAM_THREADS / 64];
  AdamTensor t;
  const int2 c = chunks[blockIdx.x];
  const int cnt = chunk_of(table, ntensors, c, t);
  double acc = 0.0;
  if (cnt > 0) {
    const float* g = t.g + c.y;
    const int nvec = cnt >> 2;
    const bool vec = dev_aligned16(g);
    float4 q[ADAM_VECS];
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
      const int i = (int)threadIdx.x + j * ADAM_THREADS;
      q[j] = i < nvec ? load4(g, i, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
      if ((int)threadIdx.x + j * ADAM_THREADS < nvec) acc = sq_add(sq_add(sq_add(sq_add(acc, q[j].x), q[j].y), q[j].z), q[j].w);
    }
    if ((int)threadIdx.x < (cnt & 3)) acc = sq_add(acc, g[4 * nvec + (int)threadIdx.x]);
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_scalars_kernel(const double* __restrict__ partials, int nchunks, double lr, double b1,
                                                                   double b2, double max_norm, long long* __restrict__ counters,
                                                                   double* __restrict__ scal) {
  __shared__ double sh[ADAM_THREADS / 64];
  const int per = (nchunks + ADAM_THREADS - 1) / ADAM_THREADS;
  const int lo = (int)threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
  double acc = 0.0;
  for (int i = lo; i < hi; ++i) acc += partials[i];
  const double sum = block_sum(acc, sh);
  if (threadIdx.x != 0) return;
  const bool skip = !isfinite(sum);
  const double norm = sqrt(sum);
  scal[0] = norm;
  scal[4] = skip ? 1.0 : 0.0;
  if (skip) {
    counters[1] += 1;
    return;
  }
  const long long step = counters[0] + 1;
  counters[0] = step;
  double coef = 1.0;
  if (max_norm > 0.0 && !(norm <= max_norm)) coef = max_norm / (norm + 1e-6);
  scal[1] = (double)(float)coef;
  scal[2] = lr / (1.0 - pow(b1, (double)step));
  scal[3] = 1.0 / sqrt(1.0 - pow(b2, (double)step));
  scal[5] += norm;
}

struct AdamConst { float coef, step_size, inv_bc2_sqrt, b1c, b2, b2c, eps, wd; };      // b1c = 1 - b1, b2c = 1 - b2

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamConst& k) {
  g = k.coef * g;
  g = g + k.wd * p;
  m = m + k.b1c * (g - m);
  v = k.b2 * v + k.b2c * g * g;
  p = p - k.step_size * (m / (sqrtf(v) * k.inv_bc2_sqrt + k.eps));
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamTensor* __restrict__ table, int ntensors,
                                                                const int2* __restrict__ chunks, float* __restrict__ m,
                                                                float* __restrict__ v, long long total, const double* __restrict__ scal,
                                                                float b1c, float b2, float b2c, float eps, float wd) {
  if (scal[4] != 0.0) return;
  const AdamConst k = {(float)scal[1], (float)scal[2], (float)scal[3], b1c, b2, b2c, eps, wd};
  AdamTensor t;
  const int2 c = chunks[blockIdx.x];
  const int cnt = chunk_of(table, ntensors, c, t);
  if (cnt <= 0 || t.offset < 0 || (t.offset & 3) || t.offset + c.y + cnt > total) return;
  float* p = t.p + c.y;
  const float* g = t.g + c.y;
  float* mm = m + t.offset + c.y;                             // 16-byte aligned: m is, offset and the chunk's start are multiples of 4
  float* vv = v + t.offset + c.y;
  const int nvec = cnt >> 2;
  const bool pvec = dev_aligned16(p), gvec = dev_aligned16(g);
  float4 P[ADAM_VECS], G[ADAM_VECS], M[ADAM_VECS], V[ADAM_VECS];
#pragma unroll
  for (int j = 0; j < ADAM_VECS; ++j) {
    const int i = (int)threadIdx.x + j * ADAM_THREADS;
    if (i < nvec) {
      P[j] = load4(p, i, pvec);
      G[j] = load4(g, i, gvec);
      M[j] = reinterpret_cast<const float4*>(mm)[i];
      V[j] = reinterpret_cast<const float4*>(vv)[i];
    }
  }
#pragma unroll
  for (int j = 0; j < ADAM_VECS; ++j) {
    const int i = (int)threadIdx.x + j * ADAM_THREADS;
    if (i < nvec) {
      adam_one(P[j].x, G[j].x, M[j].x, V[j].x, k);
      adam_one(P[j].y, G[j].y, M[j].y, V[j].y, k);
      adam_one(P[j].z, G[j].z, M[j].z, V[j].z, k);
      adam_one(P[j].w, G[j].w, M[j].w, V[j].w, k);
      reinterpret_cast<float4*>(mm)[i] = M[j];
      reinterpret_cast<float4*>(vv)[i] = V[j];
      if (pvec) {
        reinterpret_cast<float4*>(p)[i] = P[j];
      } else {
        float* q = p + 4 * i;
        q[0] = P[j].x, q[1] = P[j].y, q[2] = P[j].z, q[3] = P[j].w;
      }
    }
  }
  if ((int)threadIdx.x < (cnt & 3)) {
    const int e = 4 * nvec + (int)threadIdx.x;
    float pe = p[e], me = mm[e], ve = vv[e];
    adam_one(pe, g[e], me, ve, k);
    p[e] = pe, mm[e] = me, vv[e] = ve;
  }
}

inline bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// the host copy of the table: every row names two fp32 tensors, a size an int holds and a slot of m and v that starts a float4
int check_table(const long long* host, int ntensors) {
  int status = 0;
  for (int t = 0; t < ntensors; ++t) {
    const long long p = host[4 * t], g = host[4 * t + 1], offset = host[4 * t + 2], n = host[4 * t + 3];
    if (!p || !g || offset < 0 || (offset & 3) || n < 0 || n > INT_MAX) return CDFO_EINVAL;
    if ((p & 3) || (g & 3)) status = CDFO_EALIGN;
  }
  return status;
}

}  // namespace

extern "C" int cdfo_grad_norm_partials(const long long* table_host, const long long* table, int ntensors, const int* chunks, int nchunks,
                                       double* partials, void* stream) {
  if (!table_host || !table || !chunks || !partials || ntensors <= 0 || nchunks <= 0) return CDFO_EINVAL;
  const int bad = check_table(table_host, ntensors);
  if (bad) return bad;
  if (misaligned(table, 7u) || misaligned(chunks, 7u) || misaligned(partials, 7u)) return CDFO_EALIGN;
  hipLaunchKernelGGL(grad_norm_kernel, dim3(nchunks), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const AdamTensor*>(table), ntensors, reinterpret_cast<const int2*>(chunks), partials);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_adam_scalars(const double* partials, int nchunks, double lr, double beta1, double beta2, double max_norm,
                                 long long* counters, double* scalars, void* stream) {
  if (!partials || !counters || !scalars || nchunks <= 0) return CDFO_EINVAL;
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || max_norm != max_norm) return CDFO_EINVAL;
  if (misaligned(partials, 7u) || misaligned(counters, 7u) || misaligned(scalars, 7u)) return CDFO_EALIGN;
  hipLaunchKernelGGL(adam_scalars_kernel, dim3(1), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream), partials, nchunks, lr, beta1,
                     beta2, max_norm, counters, scalars);
  CDFO_LAUNCH_CHECK();
  return 0;
}

extern "C" int cdfo_adam_step(const long long* table_host, const long long* table, int ntensors, const int* chunks, int nchunks, float* m,
                              float* v, long long total, const double* scalars, double beta1, double beta2, double eps,
                              double weight_decay, void* stream) {
  if (!table_host || !table || !chunks || !m || !v || !scalars || ntensors <= 0 || nchunks <= 0 || total <= 0 || (total & 3))
    return CDFO_EINVAL;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return CDFO_EINVAL;
  const int bad = check_table(table_host, ntensors);
  if (bad) return bad;
  for (int t = 0; t < ntensors; ++t)
    if (table_host[4 * t + 2] + table_host[4 * t + 3] > total) return CDFO_EINVAL;
  if (misaligned(table, 7u) || misaligned(chunks, 7u) || misaligned(m, 15u) || misaligned(v, 15u) || misaligned(scalars, 7u))
    return CDFO_EALIGN;
  hipLaunchKernelGGL(adam_step_kernel, dim3(nchunks), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const AdamTensor*>(table), ntensors, reinterpret_cast<const int2*>(chunks), m, v, total, scalars,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay);
  CDFO_LAUNCH_CHECK();
  return 0;
}
