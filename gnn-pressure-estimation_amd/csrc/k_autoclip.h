// AutoClip (include/gatres.h: gatres_autoclip_t), device pieces shared by the norm launches -- the stand-alone one
// (k_autoclip.hip) and the sum-of-squares variant of the fused path's slab reduction (k_fused_host.hip) -- and the update.
#pragma once
#include "gatres_common.h"

// gatres_autoclip_t.ctl words
constexpr int AC_COUNT = 0;      // entries in the history
constexpr int AC_SNAP_COUNT = 1; // what the norm launch found: the count, ...
constexpr int AC_SNAP_STEP = 2;  // ... the optimizer step count, ...
constexpr int AC_SNAP_DROP = 3;  // ... and whether this step is dropped (stable words for every workgroup of the update)
constexpr int AC_OVERFLOW = 4;   // sticky: an update found the history full and skipped its step

namespace {

// Sum over a 256-thread workgroup in a fixed order (wave butterflies, then the four waves in order); every thread gets the
// same bits.  lds4: __shared__ double[4].
__device__ __forceinline__ double ac_block_sum(double s, double* lds4) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  __syncthreads();                                   // (lds4 may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// Block 0, thread 0 of a norm launch: the words the update launch reads instead of the live ones it changes
__device__ __forceinline__ void ac_snapshot(unsigned long long* ctl, const unsigned long long* step_counter, bool drop) {
  ctl[AC_SNAP_COUNT] = ctl[AC_COUNT];
  ctl[AC_SNAP_STEP] = step_counter[0];
  ctl[AC_SNAP_DROP] = drop ? 1ULL : 0ULL;
}

}  // namespace
