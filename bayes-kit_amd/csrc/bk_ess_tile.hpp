// Device helpers shared by the LDS-staged ESS kernels (bk_diag.hip: per-chain ESS and autocorrelation; bk_ess_multi.hip:
// cross-chain lag sums).
#pragma once
#include "bk_common.hpp"

namespace bke {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < BK_WAVE; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}

// (register tiles of 64 lag accumulators per lane: bk_diag.hip, k_ess_tile)
template <int HALF>
__device__ __forceinline__ void ess_fold(double (&v)[64], int lane) {
  // lanes whose bit HALF is set keep the upper half of the first 2*HALF entries, the others the lower half
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const bool up = (lane & HALF) != 0;
    const double send = up ? v[i] : v[i + HALF];
    const double mine = up ? v[i + HALF] : v[i];
    v[i] = mine + __shfl_xor(send, HALF);
  }
}

}  // namespace bke
