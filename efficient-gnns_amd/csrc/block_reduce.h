// The fixed-order reduction every scalar or per-column result of the library goes through, defined here and nowhere else (DESIGN.md
// section 3): a butterfly over the lanes of a group, the workgroup's waves (or threads) combined in a fixed order, one partial per
// workgroup in a workspace, and a last small launch that adds the partials in a fixed order.  No floating-point atomic anywhere, so two
// runs agree bit for bit; the order of the additions is part of each helper's contract and a site keeps the one it was written with.
//
// common.h includes this header at its end and builds egnn_wave_sum / egnn_wave_max / egnn_group_sum on it, so every kernel file has
// it; the files whose reductions live here name it as well.  The kernels below are `static` templates: the library links without
// relocatable device code, so each translation unit instantiates (and registers) the ones it launches, and no other carries them.
#pragma once
#ifndef EGNN_WAVE
#error "block_reduce.h is included through common.h"
#endif

namespace egnn_reduce {

__device__ __forceinline__ float larger(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double larger(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ int larger(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ long long larger(long long a, long long b) { return a > b ? a : b; }

// ---- lane groups: sum / max over the aligned group of G consecutive lanes (G a power of two <= 64) the calling lane sits in, xor
// offsets G/2 ... 1; every lane of the group gets the result (the same tree with commuted operands, hence the same bits)
template <int G, class T>
__device__ __forceinline__ T group_sum(T v) {
  static_assert(G >= 1 && G <= EGNN_WAVE && (G & (G - 1)) == 0, "a lane group is a power of two within the wave");
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int G, class T>
__device__ __forceinline__ T group_max(T v) {
  static_assert(G >= 1 && G <= EGNN_WAVE && (G & (G - 1)) == 0, "a lane group is a power of two within the wave");
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = larger(v, __shfl_xor(v, o));
  return v;
}

// ---- the four waves of a 256-thread workgroup: v[q] of each wave's lane 0 summed over the waves, result on every thread.  `sh` holds
// 4 * K elements and is free again when the call returns (the barrier pair).  PAIRWISE is (w0 + w1) + (w2 + w3), SERIAL is
// ((w0 + w1) + w2) + w3: floating-point sites differ in this and each keeps its own.
enum Assoc { PAIRWISE, SERIAL };
template <Assoc A, int K, class T>
__device__ __forceinline__ void waves4_sum(T (&v)[K], T* sh) {
  const int wave = egnn_wave_id();
  if (egnn_lane() == 0) {
#pragma unroll
    for (int q = 0; q < K; ++q) sh[wave * K + q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; ++q)
    v[q] = A == PAIRWISE ? (sh[q] + sh[K + q]) + (sh[2 * K + q] + sh[3 * K + q]) : ((sh[q] + sh[K + q]) + sh[2 * K + q]) + sh[3 * K + q];
  __syncthreads();
}
template <Assoc A, class T>
__device__ __forceinline__ T waves4_sum(T v, T* sh) {
  T a[1] = {v};
  waves4_sum<A>(a, sh);
  return a[0];
}

// ---- the LDS halving tree over the THREADS threads of a workgroup, K quantities at a time: red[q][t] += red[q][t + o] for
// o = THREADS/2 ... 1, one barrier per step; the totals are red[q][0], valid for every thread that reads them after the call (no
// broadcast, no barrier beyond the tree's own).  The caller owns `red`, which may have more than K rows (at_finish_kernel folds two,
// then three quantities through one array).  block_tree_fold expects the values stored and a barrier passed; block_tree_sum stores
// them first.
template <int THREADS, int K, class T>
__device__ __forceinline__ void block_tree_fold(T (*red)[THREADS]) {
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < K; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    }
    __syncthreads();
  }
}
template <int THREADS, int K, class T>
__device__ __forceinline__ void block_tree_sum(const T (&v)[K], T (*red)[THREADS]) {
#pragma unroll
  for (int q = 0; q < K; ++q) red[q][threadIdx.x] = v[q];
  __syncthreads();
  block_tree_fold<THREADS, K>(red);
}

// ---- the finalize launches
// workgroup q: out[q] = scale * sum of partials[q * stride .. + nb), thread t adding partials t, t + THREADS, ... and the tree above
template <int THREADS, class T>
static __global__ __launch_bounds__(THREADS) void sum_partials_kernel(const T* __restrict__ partials, int64_t stride, int64_t nb, T scale,
                                                                      T* __restrict__ out) {
  __shared__ T red[1][THREADS];
  const T* p = partials + (int64_t)blockIdx.x * stride;
  T v[1] = {0};
  for (int64_t i = threadIdx.x; i < nb; i += THREADS) v[0] += p[i];
  block_tree_sum<THREADS>(v, red);
  if (threadIdx.x == 0) out[blockIdx.x] = red[0][0] * scale;
}

// out[k] = sum over the nb partial rows of column k (partials is [nb, K]): one wave per column, lane l adding rows l, l + 64, ...,
// then the wave butterfly
template <class T>
static __global__ __launch_bounds__(256) void colsum_partials_kernel(const T* __restrict__ partials, int nb, int64_t K, T* __restrict__ out) {
  const int lane = egnn_lane();
  const int64_t k = (int64_t)blockIdx.x * 4 + egnn_wave_id();
  if (k >= K) return;
  T t = 0;
  for (int b = lane; b < nb; b += 64) t += partials[(int64_t)b * K + k];
  t = group_sum<EGNN_WAVE>(t);
  if (lane == 0) out[k] = t;
}
template <class T>
inline void colsum_partials(const T* partials, int nb, int64_t K, T* out, hipStream_t st) {
  hipLaunchKernelGGL(colsum_partials_kernel<T>, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st, partials, nb, K, out);
}

// ---- the grid rule: one workgroup per `per` items, at least one, at most `cap`
__host__ __device__ __forceinline__ int64_t capped_blocks(int64_t n, int64_t per, int64_t cap) {
  const int64_t want = (n + per - 1) / per;
  return want < 1 ? 1 : (want < cap ? want : cap);
}

}  // namespace egnn_reduce
