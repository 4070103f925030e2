// Shared helpers for the gfx950 kernels of libegnn_hip.so.  CDNA4 only: wave64, no portability shims.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/egnn_hip.h"

#define EGNN_WAVE 64

#define EGNN_CHECK_ARG(cond) \
  do {                       \
    if (!(cond)) return EGNN_EINVAL; \
  } while (0)

static inline int egnn_launch_status() { return hipGetLastError() == hipSuccess ? EGNN_OK : EGNN_ELAUNCH; }

static inline bool egnn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ int egnn_lane() { return threadIdx.x & 63; }
// wave index inside the workgroup as a provably wave-uniform (SGPR) value
__device__ __forceinline__ int egnn_wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

#include "block_reduce.h"

// the float butterflies under their historical names
__device__ __forceinline__ float egnn_wave_sum(float v) { return egnn_reduce::group_sum<EGNN_WAVE>(v); }
// sum over the aligned group of G consecutive lanes (G a power of two <= 64) the calling lane sits in; every lane of the group gets it
template <int G>
__device__ __forceinline__ float egnn_group_sum(float v) { return egnn_reduce::group_sum<G>(v); }
__device__ __forceinline__ float egnn_wave_max(float v) { return egnn_reduce::group_max<EGNN_WAVE>(v); }
