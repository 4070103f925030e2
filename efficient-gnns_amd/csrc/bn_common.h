// Pieces of the fused BatchNorm1d (+ ReLU + dropout) kernels shared by fused_bn.hip and the skinny GEMM that applies them in its
// operand load (gemm_skinny.hip): the parameter block, the counter-based dropout uniform and the per-element forward.
#pragma once
#include "common.h"

namespace egnn_bn {

struct BnParams {
  const float* x; int64_t ldx;
  int64_t n, C;
  const float* mean; const float* var; float eps;
  const float* gamma; const float* beta;
  int relu; float p; unsigned long long seed;
  const unsigned long long* seed_dev;   // nullable: added to `seed` (a per-step value kept on the device: hipGraph replays)
  const int64_t* pick;                  // nullable: the kernel works on the n rows x[pick[i]] (unique ids); y / dy rows are i
  int wide;                             // element indices may pass 2^32 (rows of x * C > 2^32): the hash takes the 64-bit index
};
__device__ __forceinline__ int64_t bn_row(const BnParams& q, int64_t i) { return q.pick ? q.pick[i] : i; }

// counter-based uniform in [0,1) of (seed, element index): two rounds of a 32-bit multiply-xorshift mixer (constants of C. Wellons'
// "lowbias32"), the halves of the seed injected before each round.  32-bit integer VALU only: the mask is RECOMPUTED in every
// backward pass and inside GEMM epilogues, where a 64-bit splitmix (three 64 x 64 multiplies) cost more issue slots than the arithmetic
// around it.  Forward and backward only have to agree with each other (no other RNG is reproduced).
__device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned hash32(unsigned long long seed, unsigned long long idx) {
  unsigned h = mix32((unsigned)idx ^ (unsigned)seed);
  return mix32(h + (unsigned)(seed >> 32) + (unsigned)(idx >> 32) * 0x9E3779B9U);
}
__device__ __forceinline__ float uniform01(unsigned long long seed, unsigned long long idx) {
  return (float)(hash32(seed, idx) >> 8) * (1.0f / 16777216.0f);
}

// What a kernel forms ONCE about the dropout gate: seed + *seed_dev and the scale of a kept element.  The ReLU / dropout gate is exactly
// 0 or 1 before the scale, so  gate * inv_keep  is the same float as  gate / (1 - p).
struct BnGate { unsigned long long seed; float inv_keep; };
__device__ __forceinline__ BnGate bn_gate(const BnParams& q) {
  BnGate gt{0ull, 1.f};
  if (q.p > 0.f) {
    gt.seed = q.seed + (q.seed_dev ? *q.seed_dev : 0ull);
    gt.inv_keep = 1.f / (1.f - q.p);
  }
  return gt;
}

// keep bits of the four neighbouring elements (row, c .. c + 3) from the hash: bit k set = element c + k is kept (u >= p); p == 0: all
// kept.  Below 2^32 elements (!q.wide, the host's choice) the index is formed in 32 bits from one product per call and the term of its
// upper half, which is zero, is left out: the same bits as hash32 gives.
__device__ __forceinline__ unsigned bn_keep4_hash(const BnParams& q, const BnGate& gt, int64_t row, int64_t c) {
  if (!(q.p > 0.f)) return 0xFu;
  unsigned keep = 0u;
  if (q.wide) {
#pragma unroll
    for (int k = 0; k < 4; ++k) keep |= (uniform01(gt.seed, (unsigned long long)(row * q.C + c + k)) >= q.p ? 1u : 0u) << k;   // (as before)
  } else {
    const unsigned i0 = (unsigned)row * (unsigned)q.C + (unsigned)c, s_lo = (unsigned)gt.seed, s_hi = (unsigned)(gt.seed >> 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned h = mix32(mix32((i0 + k) ^ s_lo) + s_hi);
      keep |= ((float)(h >> 8) * (1.0f / 16777216.0f) >= q.p ? 1u : 0u) << k;
    }
  }
  return keep;
}
// per-element forward pieces shared by forward and backward; `keep`: this element's dropout decision (one bit of bn_keep4_hash)
__device__ __forceinline__ void bn_elem(const BnParams& q, const BnGate& gt, bool keep, float x, float mean, float rstd, float g, float b,
                                        float& xhat, float& gate) {
  xhat = (x - mean) * rstd;
  const float pre = g * xhat + b;
  gate = (q.relu && !(pre > 0.f)) ? 0.f : 1.f;
  if (q.p > 0.f) gate = keep ? gate * gt.inv_keep : 0.f;
}

}  // namespace egnn_bn
