// Aggregation of E message rows into N node rows by an UNSORTED index (what torch_scatter.scatter computes for dim 0), and its
// backward, for user-defined message-passing layers (nn.MessagePassing).  No float atomics in either direction.
//
// Forward (egnn_scatter_runs_f32) walks the sorted (row, position) keys of egnn_rows_plan_build_i64 (rows_keys.h, rows_sum.hip): a
// row's positions form one run, in ascending position.
//   sum / mean: the run-sum itself -- egnn_rows_add_runs_f32(accumulate = 0) is called on the same keys, so the bits and the order of
//               the additions are that entry point's by construction; one more launch takes a row's run length off the keys (two
//               binary searches), stores it in `count` and, for mean, divides the row by it.
//   max / min:  the cut, the partial slots and the two passes of rows_runs.h with another fold.  The lane group at a chunk's first
//               sorted position folds the chunk's rows in ascending position, keeping per column the pair (value, position) and
//               replacing it only by a STRICTLY better value, so the smallest position attaining the extreme wins; the second launch
//               merges a long run's pairs in ascending chunk order under the same strict rule.  Rows without a run get value 0 and
//               arg = S.
// Backward (egnn_scatter_bwd_f32) is a gather: one lane group per position p reads g[index[p]] (and count / arg) and writes dsrc[p]
// with plain stores; every element of dsrc is written.
#include "rows_runs.h"

namespace {

using namespace egnn_rows;

enum { SUM = 0, MEAN = 1, MAX = 2, MIN = 3 };

template <bool IS_MAX> __device__ __forceinline__ bool better(float x, float best) { return IS_MAX ? x > best : x < best; }

// the pair (v, p) joins (best, bp): a pair without a position (p == S: nothing was read) never wins, one always loses to any other
template <bool IS_MAX>
__device__ __forceinline__ void merge_pair(float& best, int64_t& bp, float v, int64_t p, int64_t S) {
  if (p != S && (bp == S || better<IS_MAX>(v, best))) {
    best = v;
    bp = p;
  }
}

// the W positions that go with the W values at column c of a row of pitch C
template <int W> __device__ __forceinline__ void store_pos(int64_t* p, const int64_t (&v)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) p[i] = v[i];
}

// rows that no key names: value 0, arg = S (one lane group per row)
template <int W>
__global__ __launch_bounds__(THREADS) void scatter_ext_absent_kernel(float* __restrict__ out, int64_t ldo, int64_t* __restrict__ arg,
                                                                     int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S,
                                                                     int shift, int64_t C, int lg) {
  int sub;
  const int64_t row = group_item(lg, sub);
  if (row >= n_rows || row_has_run(sorted, S, shift, row)) return;
  const float zero[W] = {};
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    store_w<W>(out + row * ldo + c, zero);
    if (arg != nullptr)
#pragma unroll
      for (int i = 0; i < W; ++i) arg[row * C + c + i] = S;
  }
}

// pass 1: the lane group at sorted position j folds the chunk that starts there (if one does)
template <int W, bool IS_MAX>
__global__ __launch_bounds__(THREADS) void scatter_ext_runs_kernel(float* __restrict__ out, int64_t ldo, int64_t* __restrict__ arg,
                                                                   int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S,
                                                                   int shift, const float* __restrict__ src, int64_t lds_, int64_t C,
                                                                   float* __restrict__ part_v, int64_t* __restrict__ part_p, int64_t ldp,
                                                                   int lg) {
  int sub;
  const int64_t j = group_item(lg, sub);
  chunk_start(sorted, S, shift, n_rows, j, [&](bool head, uint64_t r) {
    const bool long_run = chunk_is_long(sorted, S, shift, j, head, r);
    if (long_run && part_v == nullptr) return;                         // (the entry point refuses this: S > CHUNK without a workspace)
    for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
      float best[W];
      int64_t bp[W];
#pragma unroll
      for (int i = 0; i < W; ++i) best[i] = 0.f, bp[i] = S;
      fold_chunk4<W>(sorted, j, chunk_limit(j, S), r, shift, S, src, lds_, c, [&best, &bp, S](const float (&x)[W], int64_t p) {
#pragma unroll
        for (int i = 0; i < W; ++i) merge_pair<IS_MAX>(best[i], bp[i], x[i], p, S);
      });
      if (long_run) {
        const int64_t slot = part_slot(j, head);
        store_w<W>(part_v + slot * ldp + c, best);
        store_pos<W>(part_p + slot * ldp + c, bp);
      } else {
        store_w<W>(out + (int64_t)r * ldo + c, best);
        if (arg != nullptr) store_pos<W>(arg + (int64_t)r * C + c, bp);
      }
    }
  });
}

// pass 2: one lane group per window of CHUNK sorted positions; the (at most one) head of a run longer than CHUNK in the window merges
// the run's partial pairs in ascending chunk order
template <int W, bool IS_MAX>
__global__ __launch_bounds__(THREADS) void scatter_ext_parts_kernel(float* __restrict__ out, int64_t ldo, int64_t* __restrict__ arg,
                                                                    int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S,
                                                                    int shift, int64_t C, const float* __restrict__ part_v,
                                                                    const int64_t* __restrict__ part_p, int64_t ldp, int lg) {
  int sub;
  const int64_t found = long_run_head(sorted, S, shift, n_rows, group_item(lg, sub) * CHUNK, sub, lg);
  if (found < 0) return;
  uint64_t r;
  const int64_t chunks = run_chunks(sorted, S, shift, found, r);
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    float best[W];
    int64_t bp[W];
    const int64_t s0 = part_slot(found, true);
    load_w<W>(part_v + s0 * ldp + c, best);
#pragma unroll
    for (int i = 0; i < W; ++i) bp[i] = part_p[s0 * ldp + c + i];
    for (int64_t k = 1; k < chunks; ++k) {
      const int64_t s = part_slot(found + k * CHUNK, false);
      float v[W];
      load_w<W>(part_v + s * ldp + c, v);
#pragma unroll
      for (int i = 0; i < W; ++i) merge_pair<IS_MAX>(best[i], bp[i], v[i], part_p[s * ldp + c + i], S);
    }
#pragma unroll
    for (int i = 0; i < W; ++i)
      if (bp[i] == S) best[i] = 0.f;
    store_w<W>(out + (int64_t)r * ldo + c, best);
    if (arg != nullptr) store_pos<W>(arg + (int64_t)r * C + c, bp);
  }
}

// count[row] = the length of row's run; mean: out[row, :] /= float(count) (rows without a run were zeroed by the run-sum)
template <int W>
__global__ __launch_bounds__(THREADS) void scatter_count_kernel(float* __restrict__ out, int64_t ldo, int32_t* __restrict__ count,
                                                                int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S, int shift,
                                                                int64_t C, int divide, int lg) {
  int sub;
  const int64_t row = group_item(lg, sub);
  if (row >= n_rows) return;
  const int64_t q0 = lower_bound(sorted, 0, S, (uint64_t)row << shift);
  const int64_t q1 = lower_bound(sorted, q0, S, ((uint64_t)row + 1) << shift);
  const int32_t n = (int32_t)(q1 - q0);
  if (sub == 0) count[row] = n;
  if (!divide || n <= 1) return;
  const float d = (float)n;
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    float v[W];
    load_w<W>(out + row * ldo + c, v);
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = v[i] / d;
    store_w<W>(out + row * ldo + c, v);
  }
}

// one lane group per position p: dsrc[p, :] from g[index[p], :]
template <int W>
__global__ __launch_bounds__(THREADS) void scatter_bwd_kernel(float* __restrict__ dsrc, int64_t ldd, int64_t S,
                                                              const int64_t* __restrict__ index, int64_t n_rows,
                                                              const float* __restrict__ g, int64_t ldg, int64_t C, int reduce,
                                                              const int32_t* __restrict__ count, const int64_t* __restrict__ arg, int lg) {
  int sub;
  const int64_t p = group_item(lg, sub);
  if (p >= S) return;
  const int64_t r = index[p];
  const bool live = r >= 0 && r < n_rows;
  float d = 1.f;
  if (live && reduce == MEAN) d = (float)count[r];
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    float v[W] = {};
    if (live) {
      load_w<W>(g + r * ldg + c, v);
      if (reduce == MEAN) {
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = v[i] / d;
      } else if (reduce >= MAX) {
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (arg[r * C + c + i] != p) v[i] = 0.f;
      }
    }
    store_w<W>(dsrc + p * ldd + c, v);
  }
}

// wrapped[p] = index[p] (+ n_rows when negative), or -1 when the id is outside [-n_rows, n_rows)
__global__ __launch_bounds__(THREADS) void rows_wrap_kernel(const int64_t* __restrict__ idx, int64_t S, int64_t n_rows,
                                                            int64_t* __restrict__ wrapped) {
  const int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (p >= S) return;
  int64_t r = idx[p];
  if (r < 0) r += n_rows;
  wrapped[p] = r >= 0 && r < n_rows ? r : -1;
}

// absent rows, pass 1 and (S > CHUNK) pass 2 of one max / min reduction
template <int W, bool IS_MAX>
void launch_ext(float* out, int64_t ldo, int64_t* arg, int64_t n_rows, const uint64_t* sorted, int64_t S, int shift, const float* src,
                int64_t lds_, int64_t C, void* ws, hipStream_t st) {
  const int lg = lanes_lg(C / W);
  const int64_t ldp = part_pitch(C);
  float* part_v = S > CHUNK ? (float*)ws : nullptr;
  int64_t* part_p = S > CHUNK ? (int64_t*)((char*)ws + (size_t)part_slots(S) * (size_t)ldp * sizeof(float)) : nullptr;
  hipLaunchKernelGGL((scatter_ext_absent_kernel<W>), dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, out, ldo, arg, n_rows, sorted,
                     S, shift, C, lg);
  if (S == 0) return;
  hipLaunchKernelGGL((scatter_ext_runs_kernel<W, IS_MAX>), dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, st, out, ldo, arg, n_rows,
                     sorted, S, shift, src, lds_, C, part_v, part_p, ldp, lg);
  if (S > CHUNK)
    hipLaunchKernelGGL((scatter_ext_parts_kernel<W, IS_MAX>), dim3((unsigned)blocks_for(part_slots(S) / 2, lg)), dim3(THREADS), 0, st, out, ldo,
                       arg, n_rows, sorted, S, shift, C, (const float*)part_v, (const int64_t*)part_p, ldp, lg);
}

}  // namespace

extern "C" int egnn_rows_wrap_i64(const int64_t* idx, int64_t S, int64_t n_rows, int64_t* wrapped, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows));
  if (S == 0) return EGNN_OK;
  EGNN_CHECK_ARG(idx && wrapped);
  if (((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(wrapped)) & 7u) != 0) return EGNN_EALIGN;
  hipLaunchKernelGGL(rows_wrap_kernel, dim3((unsigned)blocks_for(S, 0)), dim3(THREADS), 0, (hipStream_t)stream, idx, S, n_rows, wrapped);
  return egnn_launch_status();
}

extern "C" size_t egnn_scatter_runs_ws_bytes(int64_t S, int64_t C, int reduce) {
  if (reduce == SUM || reduce == MEAN) return egnn_rows_add_runs_ws_bytes(S, C);
  if ((reduce != MAX && reduce != MIN) || S <= CHUNK || S >= 0x7fffffffLL || C <= 0) return 0;
  return (size_t)part_slots(S) * (size_t)part_pitch(C) * (sizeof(float) + sizeof(int64_t));   // the values, then the positions
}

extern "C" int egnn_scatter_runs_f32(float* out, int64_t ld_out, int64_t n_rows, int32_t* count, int64_t* arg, const uint64_t* keys_sorted,
                                     int64_t S, int shift, const float* src, int64_t ld_src, int64_t C, int reduce, void* ws,
                                     size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows) && C > 0 && ld_out >= C && ld_src >= C && reduce >= SUM && reduce <= MIN);
  if (S == 0 && (n_rows == 0 || out == nullptr)) return EGNN_OK;
  EGNN_CHECK_ARG(out && n_rows > 0);
  EGNN_CHECK_ARG(reduce != MEAN || count != nullptr);
  EGNN_CHECK_ARG(reduce >= MAX || arg == nullptr);
  if (S > 0) EGNN_CHECK_ARG(keys_sorted && src && shift == bits_for((uint64_t)S - 1));
  if (S == 0) shift = 0;
  const size_t need = egnn_scatter_runs_ws_bytes(S, C, reduce);
  if (need > 0 && (!ws || ws_bytes < need)) return EGNN_EWORKSPACE;
  if ((need > 0 && !egnn_aligned16(ws)) || (reinterpret_cast<uintptr_t>(keys_sorted) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(count) & 3u) != 0 || (reinterpret_cast<uintptr_t>(arg) & 7u) != 0)
    return EGNN_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = C % 4 == 0 && ld_out % 4 == 0 && ld_src % 4 == 0 && egnn_aligned16(out) && egnn_aligned16(src);
  if (reduce <= MEAN) {
    const int rc = egnn_rows_add_runs_f32(out, ld_out, n_rows, keys_sorted, S, shift, src, ld_src, C, 0, ws, ws_bytes, stream);
    if (rc != EGNN_OK) return rc;
  }
  dispatch_w(vec4, [&](auto w) {
    constexpr int W = decltype(w)::value;
    if (reduce == MAX) launch_ext<W, true>(out, ld_out, arg, n_rows, keys_sorted, S, shift, src, ld_src, C, ws, st);
    else if (reduce == MIN) launch_ext<W, false>(out, ld_out, arg, n_rows, keys_sorted, S, shift, src, ld_src, C, ws, st);
    if (count != nullptr)
      hipLaunchKernelGGL((scatter_count_kernel<W>), dim3((unsigned)blocks_for(n_rows, lanes_lg(C / W))), dim3(THREADS), 0, st, out, ld_out, count,
                         n_rows, keys_sorted, S, shift, C, (int)(reduce == MEAN), lanes_lg(C / W));
  });
  return egnn_launch_status();
}

extern "C" int egnn_scatter_bwd_f32(float* dsrc, int64_t ld_dsrc, int64_t S, const int64_t* index, int64_t n_rows, const float* g,
                                    int64_t ld_g, int64_t C, int reduce, const int32_t* count, const int64_t* arg, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows) && C > 0 && ld_dsrc >= C && ld_g >= C && reduce >= SUM && reduce <= MIN);
  if (S == 0) return EGNN_OK;
  EGNN_CHECK_ARG(dsrc && index && (g || n_rows == 0));
  EGNN_CHECK_ARG(reduce != MEAN || count != nullptr);
  EGNN_CHECK_ARG(reduce < MAX || arg != nullptr);
  if ((reinterpret_cast<uintptr_t>(index) & 7u) != 0 || (reinterpret_cast<uintptr_t>(count) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(arg) & 7u) != 0)
    return EGNN_EALIGN;
  const bool vec4 = C % 4 == 0 && ld_dsrc % 4 == 0 && ld_g % 4 == 0 && egnn_aligned16(dsrc) && egnn_aligned16(g);
  dispatch_w(vec4, [&](auto w) {
    constexpr int W = decltype(w)::value;
    const int lg = lanes_lg(C / W);
    hipLaunchKernelGGL((scatter_bwd_kernel<W>), dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, (hipStream_t)stream, dsrc, ld_dsrc, S, index,
                       n_rows, g, ld_g, C, reduce, count, arg, lg);
  });
  return egnn_launch_status();
}
