// Aggregation of E message rows into N node rows by an UNSORTED index (what torch_scatter.scatter computes for dim 0), and its
// backward, for user-defined message-passing layers (nn.MessagePassing).  No float atomics in either direction.
//
// Forward (egnn_scatter_runs_f32) walks the sorted (row, position) keys of egnn_rows_plan_build_i64 (rows_keys.h, rows_sum.hip): a
// row's positions form one run, in ascending position.
//   sum / mean: the run-sum itself -- egnn_rows_add_runs_f32(accumulate = 0) is called on the same keys, so the bits and the order of
//               the additions are that entry point's by construction; one more launch takes a row's run length off the keys (two
//               binary searches), stores it in `count` and, for mean, divides the row by it.
//   max / min:  the run-sum's cut with another fold.  A run is cut from its head into chunks of EGNN_ROWS_SUM_CHUNK positions; the lane
//               group at a chunk's first sorted position folds the chunk's rows in ascending position, keeping per column the pair
//               (value, position) and replacing it only by a STRICTLY better value, so the smallest position attaining the extreme
//               wins.  A run of one chunk goes straight to out / arg; the chunks of a longer run leave their pairs in the workspace
//               and a second launch merges them in ascending chunk order under the same strict rule.  Whether a position starts a
//               chunk is read off the keys, so nothing depends on the launch geometry.  Rows without a run get value 0 and arg = S.
// Backward (egnn_scatter_bwd_f32) is a gather: one lane group per position p reads g[index[p]] (and count / arg) and writes dsrc[p]
// with plain stores; every element of dsrc is written.
#include "rows_keys.h"

namespace {

using namespace egnn_rows;

constexpr int THREADS = 256;
constexpr int64_t CHUNK = EGNN_ROWS_SUM_CHUNK;
enum { SUM = 0, MEAN = 1, MAX = 2, MIN = 3 };

template <int W> struct Vec;
template <> struct Vec<1> { using type = float; };
template <> struct Vec<4> { using type = float4; };

template <int W> __device__ __forceinline__ void load_w(const float* p, float (&v)[W]) {
  const typename Vec<W>::type t = *reinterpret_cast<const typename Vec<W>::type*>(p);
  __builtin_memcpy(v, &t, sizeof(t));
}
template <int W> __device__ __forceinline__ void store_w(float* p, const float (&v)[W]) {
  typename Vec<W>::type t;
  __builtin_memcpy(&t, v, sizeof(t));
  *reinterpret_cast<typename Vec<W>::type*>(p) = t;
}

// first position in [lo, hi) whose key is >= key (hi when there is none)
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ sorted, int64_t lo, int64_t hi, uint64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <bool IS_MAX> __device__ __forceinline__ bool better(float x, float best) { return IS_MAX ? x > best : x < best; }

// the pair (v, p) joins (best, bp): a pair without a position (p == S: nothing was read) never wins, one always loses to any other
template <bool IS_MAX>
__device__ __forceinline__ void merge_pair(float& best, int64_t& bp, float v, int64_t p, int64_t S) {
  if (p != S && (bp == S || better<IS_MAX>(v, best))) {
    best = v;
    bp = p;
  }
}

__device__ __forceinline__ int64_t part_slot(int64_t q, bool is_head) { return 2 * (q / CHUNK) + (is_head ? 0 : 1); }

// rows that no key names: value 0, arg = S (one lane group per row)
template <int W>
__global__ __launch_bounds__(THREADS) void scatter_ext_absent_kernel(float* __restrict__ out, int64_t ldo, int64_t* __restrict__ arg,
                                                                     int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S,
                                                                     int shift, int64_t C, int lg) {
  const int64_t row = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
  if (row >= n_rows) return;
  const int64_t q = lower_bound(sorted, 0, S, (uint64_t)row << shift);
  if (q < S && (sorted[q] >> shift) == (uint64_t)row) return;
  const float zero[W] = {};
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    store_w<W>(out + row * ldo + c, zero);
    if (arg != nullptr)
#pragma unroll
      for (int i = 0; i < W; ++i) arg[row * C + c + i] = S;
  }
}

// pass 1: the lane group at sorted position j folds the chunk that starts there (if one does); the cut is rows_sum.hip's
template <int W, bool IS_MAX>
__global__ __launch_bounds__(THREADS) void scatter_ext_runs_kernel(float* __restrict__ out, int64_t ldo, int64_t* __restrict__ arg,
                                                                   int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S,
                                                                   int shift, const float* __restrict__ src, int64_t lds_, int64_t C,
                                                                   float* __restrict__ part_v, int64_t* __restrict__ part_p, int64_t ldp,
                                                                   int lg) {
  const int64_t j = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
  if (j >= S) return;
  const uint64_t key = sorted[j];
  const uint64_t r = key >> shift;
  if (key == NO_KEY || r >= (uint64_t)n_rows) return;
  const bool head = j == 0 || (sorted[j - 1] >> shift) != r;
  if (!head) {
    if (j < CHUNK || (sorted[j - CHUNK] >> shift) != r) return;       // inside its run's first chunk
    const int64_t h = lower_bound(sorted, 0, j - CHUNK + 1, r << shift);  // the run's head
    if ((j - h) % CHUNK != 0) return;
  }
  const bool long_run = !head || (j + CHUNK < S && (sorted[j + CHUNK] >> shift) == r);
  if (long_run && part_v == nullptr) return;                           // (the entry point refuses this: S > CHUNK without a workspace)
  const int64_t limit = j + CHUNK < S ? j + CHUNK : S;
  const uint64_t mask = (uint64_t(1) << shift) - 1;
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    float best[W];
    int64_t bp[W];
#pragma unroll
    for (int i = 0; i < W; ++i) best[i] = 0.f, bp[i] = S;
    // four keys and rows in flight at a time; the comparisons stay in ascending position
    for (int64_t q = j; q < limit; q += 4) {
      uint64_t k[4];
      float x[4][W];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) k[u] = q + u < limit ? sorted[q + u] : NO_KEY;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = (k[u] >> shift) == r && (k[u] & mask) < (uint64_t)S;   // a position outside [0, S) is never used as an address
        if (ok[u]) load_w<W>(src + (int64_t)(k[u] & mask) * lds_ + c, x[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u])
#pragma unroll
          for (int i = 0; i < W; ++i) merge_pair<IS_MAX>(best[i], bp[i], x[u][i], (int64_t)(k[u] & mask), S);
      if ((k[3] >> shift) != r) break;
    }
    if (long_run) {
      const int64_t slot = part_slot(j, head);
      store_w<W>(part_v + slot * ldp + c, best);
#pragma unroll
      for (int i = 0; i < W; ++i) part_p[slot * ldp + c + i] = bp[i];
    } else {
      store_w<W>(out + (int64_t)r * ldo + c, best);
      if (arg != nullptr)
#pragma unroll
        for (int i = 0; i < W; ++i) arg[(int64_t)r * C + c + i] = bp[i];
    }
  }
}

// pass 2: one lane group per window of CHUNK sorted positions; the (at most one) head of a run longer than CHUNK in the window merges
// the run's partial pairs in ascending chunk order
template <int W, bool IS_MAX>
__global__ __launch_bounds__(THREADS) void scatter_ext_parts_kernel(float* __restrict__ out, int64_t ldo, int64_t* __restrict__ arg,
                                                                    int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S,
                                                                    int shift, int64_t C, const float* __restrict__ part_v,
                                                                    const int64_t* __restrict__ part_p, int64_t ldp, int lg) {
  const int64_t m = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
  const int64_t base = m * CHUNK;                                     // (base >= S: the loop below is empty, found stays -1)
  int64_t found = -1;
  for (int64_t j = base + sub; j < base + CHUNK && j + CHUNK < S; j += (int64_t)1 << lg) {
    const uint64_t key = sorted[j];
    const uint64_t r = key >> shift;
    if (key != NO_KEY && r < (uint64_t)n_rows && (j == 0 || (sorted[j - 1] >> shift) != r) && (sorted[j + CHUNK] >> shift) == r) found = j;
  }
  for (int o = (1 << lg) >> 1; o > 0; o >>= 1) {
    const int64_t other = __shfl_xor(found, o, 1 << lg);
    found = other > found ? other : found;
  }
  if (found < 0) return;
  const uint64_t r = sorted[found] >> shift;
  const int64_t end = lower_bound(sorted, found + CHUNK + 1, S, (r + 1) << shift);
  const int64_t chunks = (end - found + CHUNK - 1) / CHUNK;
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
    if (arg != nullptr)
#pragma unroll
      for (int i = 0; i < W; ++i) arg[(int64_t)r * C + c + i] = bp[i];
  }
}

// count[row] = the length of row's run; mean: out[row, :] /= float(count) (rows without a run were zeroed by the run-sum)
template <int W>
__global__ __launch_bounds__(THREADS) void scatter_count_kernel(float* __restrict__ out, int64_t ldo, int32_t* __restrict__ count,
                                                                int64_t n_rows, const uint64_t* __restrict__ sorted, int64_t S, int shift,
                                                                int64_t C, int divide, int lg) {
  const int64_t row = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
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
  const int64_t p = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
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

int64_t blocks_for(int64_t n, int lg) {
  const int64_t per_block = THREADS >> lg;
  return (n + per_block - 1) / per_block;
}

int64_t part_pitch(int64_t C) { return (C + 3) / 4 * 4; }
int64_t part_slots(int64_t S) { return 2 * ((S + CHUNK - 1) / CHUNK); }

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
    hipLaunchKernelGGL((scatter_ext_parts_kernel<W, IS_MAX>), dim3((unsigned)blocks_for((S + CHUNK - 1) / CHUNK, lg)), dim3(THREADS), 0, st, out,
                       ldo, arg, n_rows, sorted, S, shift, C, (const float*)part_v, (const int64_t*)part_p, ldp, lg);
}

template <int W>
void launch_count(float* out, int64_t ldo, int32_t* count, int64_t n_rows, const uint64_t* sorted, int64_t S, int shift, int64_t C, int divide,
                  hipStream_t st) {
  const int lg = lanes_lg(C / W);
  hipLaunchKernelGGL((scatter_count_kernel<W>), dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, out, ldo, count, n_rows, sorted, S,
                     shift, C, divide, lg);
}

bool sizes_ok(int64_t S, int64_t n_rows) { return S >= 0 && S < 0x7fffffffLL && n_rows >= 0 && n_rows < 0x7fffffffLL; }

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
    if (count != nullptr) {
      if (vec4) launch_count<4>(out, ld_out, count, n_rows, keys_sorted, S, shift, C, reduce == MEAN, st);
      else launch_count<1>(out, ld_out, count, n_rows, keys_sorted, S, shift, C, reduce == MEAN, st);
    }
    return egnn_launch_status();
  }
  if (vec4 && reduce == MAX) launch_ext<4, true>(out, ld_out, arg, n_rows, keys_sorted, S, shift, src, ld_src, C, ws, st);
  else if (vec4) launch_ext<4, false>(out, ld_out, arg, n_rows, keys_sorted, S, shift, src, ld_src, C, ws, st);
  else if (reduce == MAX) launch_ext<1, true>(out, ld_out, arg, n_rows, keys_sorted, S, shift, src, ld_src, C, ws, st);
  else launch_ext<1, false>(out, ld_out, arg, n_rows, keys_sorted, S, shift, src, ld_src, C, ws, st);
  if (count != nullptr) {
    if (vec4) launch_count<4>(out, ld_out, count, n_rows, keys_sorted, S, shift, C, 0, st);
    else launch_count<1>(out, ld_out, count, n_rows, keys_sorted, S, shift, C, 0, st);
  }
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
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = C % 4 == 0 && ld_dsrc % 4 == 0 && ld_g % 4 == 0 && egnn_aligned16(dsrc) && egnn_aligned16(g);
  if (vec4) {
    const int lg = lanes_lg(C / 4);
    hipLaunchKernelGGL((scatter_bwd_kernel<4>), dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, st, dsrc, ld_dsrc, S, index, n_rows, g, ld_g,
                       C, reduce, count, arg, lg);
  } else {
    const int lg = lanes_lg(C);
    hipLaunchKernelGGL((scatter_bwd_kernel<1>), dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, st, dsrc, ld_dsrc, S, index, n_rows, g, ld_g,
                       C, reduce, count, arg, lg);
  }
  return egnn_launch_status();
}
