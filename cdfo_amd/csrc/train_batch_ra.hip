// cdfo_train_batch_ra: the random-access form of a training batch (see train_batch.hip for the whole story, train_batch.h for the shared
// pieces).  A translation unit of its own so that the LD form's kernel compiles to the code it had without this one beside it.
#include "train_batch.h"

extern "C" int cdfo_train_batch_ra(const unsigned char* lr, const unsigned char* pms, const signed char* rms, const unsigned char* ufs,
                                   const signed char* mvl0, const signed char* mvl1, const unsigned char* hr, int S, int T, int H, int W,
                                   int Hu, const int* plan, int B, int crop, float* x, float* pms_out, float* rms_out, float* ufs_out,
                                   float* mvs, float* hr_out, void* stream) {
  if (!mvl1) return CDFO_EINVAL;
  BatchArgs a;
  unsigned work;
  if (const int st = train_batch_args(lr, pms, rms, ufs, mvl0, hr, S, T, H, W, Hu, plan, B, crop, x, pms_out, rms_out, ufs_out, mvs, hr_out,
                                      a, work))
    return st;
  hipLaunchKernelGGL(train_batch_kernel<true>, dim3(work, B), dim3(256), 0, static_cast<hipStream_t>(stream), a, mvl1);
  CDFO_LAUNCH_CHECK();
  return 0;
}
