// Reductions over the 64 lanes of a wavefront by butterfly: xor distances 32, 16, ... 1, after which every lane holds the
// result.  The order of the distances is part of the fixed summation order of the kernels that use them (me_mbar.hip,
// me_mbar_cov.hip, me_statistics.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace me {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d));
  return v;
}

}  // namespace me
