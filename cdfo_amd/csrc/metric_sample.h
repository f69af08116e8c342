// The one place where the sample kernels of NIQE, BRISQUE, tOF and LPIPS turn a stored sample into the value their arithmetic runs
// on (DESIGN.md has the definition).  The kernels are templates on the sample type and on a parameter pack that is empty for 8-bit
// and fp64 sources and holds the format's peak, 2^depth - 1, for 16-bit ones; they call metric_sample(v, peak...) or
// unit_sample(v, peak...) and share every other statement, so an 8-bit instantiation has the arguments and the instructions it had
// before the 16-bit forms existed.
//   fp64 metrics: x = (255 v) / peak.  The product is exact, the division is the one rounding: no reciprocal.  v = 257 k at the peak
//                 65535 gives k exactly.
//   LPIPS' stem:  x01 = (float)v / (float)peak, one fp32 division, where the 8-bit form has (float)v / 255.f.  A float sample (the
//                 training loss, cdfo_lpips_stem_f32) is x01 itself: no division, no clamp, no quantisation.
#pragma once

__device__ __forceinline__ double metric_sample(unsigned char v) { return (double)v; }
__device__ __forceinline__ double metric_sample(double v) { return v; }
__device__ __forceinline__ double metric_sample(unsigned short v, double peak) { return (255.0 * (double)v) / peak; }

__device__ __forceinline__ float unit_sample(unsigned char v) { return (float)v / 255.f; }
__device__ __forceinline__ float unit_sample(unsigned short v, float peak) { return (float)v / peak; }
__device__ __forceinline__ float unit_sample(float v) { return v; }
