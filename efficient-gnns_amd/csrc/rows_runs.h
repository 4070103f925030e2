// The run cut over the sorted (row << shift) | position keys of rows_keys.h, defined here and nowhere else: what the run-sum
// (rows_sum.hip), the max / min scatter (scatter.hip) and the segment softmax (scatter_softmax.hip) share, and the head-of-run test the
// summing Adam step (adam_rows.hip, which steps a row from its head and cuts nothing) takes from here too.
//
// THE CUT.  A row's positions form one run of the sorted list, in ascending position.  A run is cut, from its head, into chunks of
// CHUNK = EGNN_ROWS_SUM_CHUNK positions.  Whether sorted position j starts a chunk is read off the keys alone (chunk_start: the run's
// head is found by a binary search, and only for positions whose key CHUNK places earlier names the same row), never off the launch
// geometry.  A run of one chunk goes straight to its row; the chunks of a longer run (chunk_is_long) are folded by different lane
// groups at the same time and leave partial rows in a workspace, and a second launch -- one lane group per window of CHUNK positions --
// lets the head of a long run (long_run_head) merge the run's run_chunks partials in ascending chunk order.
// PARTIAL SLOTS.  The chunk that starts at sorted position q takes slot part_slot = 2 (q / CHUNK) + (q is not its run's head).  A window
// of CHUNK consecutive positions holds at most one head of a run longer than CHUNK and at most one later chunk start, so the
// part_slots(S) = 2 ceil(S / CHUNK) slots of part_pitch(C) elements never collide; workspace sizes and kernels read this one rule.
// USABLE KEYS.  key_usable is the one test that lets a key's position become an address: the key names the chunk's row and its position
// is inside [0, S) (a key list built for other operands is skipped, never dereferenced).
//
// A kernel is on a shared piece only where its code object kept its LDS and occupancy and stayed without scratch, and where its
// timing stayed (profiles/rows_runs_resources.txt, profiles/rows_runs_refactor.jsonl).  Two forms here follow from that.  chunk_start
// hands the chunk to a continuation instead of returning a bool: the pass-1 launches have one lane group per sorted position and
// most groups leave at once, and a bool merged over five exits cost the run-sum 3 % (the continuation compiles to the plain exits of
// a kernel written out by hand).  An accumulator that a fold captures is a local array of the caller, never an out-parameter (12
// more registers in the run-sum otherwise, another 3 %).  fold_chunk4 is the four-in-flight walk of the lane groups that run along COLUMNS (run-sum,
// max / min); the softmax's groups run along POSITIONS with STEPS loads per lane: its walk_chunk keeps its own body and takes key_usable.
#pragma once
#include <type_traits>

#include "rows_keys.h"

namespace egnn_rows {

constexpr int THREADS = 256;
constexpr int64_t CHUNK = EGNN_ROWS_SUM_CHUNK;

template <int W> struct Vec;
template <> struct Vec<1> { using type = float; };
template <> struct Vec<4> { using type = float4; };

// W floats (4 or 16 bytes in one access) at p
template <int W> __device__ __forceinline__ void load_w(const float* p, float (&v)[W]) {
  const typename Vec<W>::type t = *reinterpret_cast<const typename Vec<W>::type*>(p);
  __builtin_memcpy(v, &t, sizeof(t));
}
template <int W> __device__ __forceinline__ void store_w(float* p, const float (&v)[W]) {
  typename Vec<W>::type t;
  __builtin_memcpy(&t, v, sizeof(t));
  *reinterpret_cast<typename Vec<W>::type*>(p) = t;
}

// lane group g of 2^lg neighbouring lanes -> the item it serves; sub: the lane's place in its group
__device__ __forceinline__ int64_t group_item(int lg, int& sub) {
  sub = threadIdx.x & ((1 << lg) - 1);
  return (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
}

// first position in [lo, hi) whose key is >= key (hi when there is none); the sorted list is ascending as 64-bit values
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ sorted, int64_t lo, int64_t hi, uint64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// does any key name `row`?
__device__ __forceinline__ bool row_has_run(const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t row) {
  const int64_t q = lower_bound(sorted, 0, S, (uint64_t)row << shift);
  return q < S && (sorted[q] >> shift) == (uint64_t)row;
}

// is sorted position j, whose key names row r, the first of r's run?
__device__ __forceinline__ bool is_run_head(const uint64_t* __restrict__ sorted, int shift, int64_t j, uint64_t r) {
  return j == 0 || (sorted[j - 1] >> shift) != r;
}

// body(head, r) runs iff sorted position j carries a usable key (of row r < n_rows) and starts a chunk of its run; head: it is the
// run's first.  (A continuation, not a bool: every other position leaves through a plain exit, as in a kernel written out by hand.)
template <class Body>
__device__ __forceinline__ void chunk_start(const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t n_rows, int64_t j,
                                            Body body) {
  if (j >= S) return;
  const uint64_t key = sorted[j];
  const uint64_t r = key >> shift;
  if (key == NO_KEY || r >= (uint64_t)n_rows) return;
  const bool head = is_run_head(sorted, shift, j, r);
  if (!head) {
    if (j < CHUNK || (sorted[j - CHUNK] >> shift) != r) return;             // inside its run's first chunk
    const int64_t h = lower_bound(sorted, 0, j - CHUNK + 1, r << shift);      // the run's head
    if ((j - h) % CHUNK != 0) return;
  }
  body(head, r);
}

// the chunk that starts at j belongs to a run of more than one chunk: its result is a partial
__device__ __forceinline__ bool chunk_is_long(const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t j, bool head, uint64_t r) {
  return !head || (j + CHUNK < S && (sorted[j + CHUNK] >> shift) == r);
}
__device__ __forceinline__ int64_t chunk_limit(int64_t j, int64_t S) { return j + CHUNK < S ? j + CHUNK : S; }

__device__ __forceinline__ uint64_t key_pos(uint64_t key, int shift) { return key & ((uint64_t(1) << shift) - 1); }
__device__ __forceinline__ bool key_usable(uint64_t key, uint64_t r, int shift, int64_t S) {
  return (key >> shift) == r && key_pos(key, shift) < (uint64_t)S;
}

// The chunk's sorted positions q = first .. limit - 1 of row r, columns c .. c + W - 1: four keys and rows are in flight at a time, and
// fold(x, position) is called in ascending position for every usable key.
template <int W, class Fold>
__device__ __forceinline__ void fold_chunk4(const uint64_t* __restrict__ sorted, int64_t first, int64_t limit, uint64_t r, int shift,
                                            int64_t S, const float* __restrict__ src, int64_t lds_, int64_t c, Fold fold) {
  for (int64_t q = first; q < limit; q += 4) {
    uint64_t k[4];
    float x[4][W];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) k[u] = q + u < limit ? sorted[q + u] : NO_KEY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ok[u] = key_usable(k[u], r, shift, S);
#pragma unroll
      for (int i = 0; i < W; ++i) x[u][i] = 0.f;                             // (a defined value: fewer registers than a row left unset)
      if (ok[u]) load_w<W>(src + (int64_t)key_pos(k[u], shift) * lds_ + c, x[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (ok[u]) fold(x[u], (int64_t)key_pos(k[u], shift));
    if ((k[3] >> shift) != r) break;
  }
}

// pass 2, for the lane group (lane `sub` of 2^lg) that owns the window of CHUNK positions at `base`: the window's one head of a
// run longer than CHUNK, or -1 (base >= S: the loop is empty); every lane of the group gets the result
__device__ __forceinline__ int64_t long_run_head(const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t n_rows, int64_t base,
                                                 int sub, int lg) {
  int64_t found = -1;
  for (int64_t j = base + sub; j < base + CHUNK && j + CHUNK < S; j += (int64_t)1 << lg) {
    const uint64_t key = sorted[j];
    const uint64_t r = key >> shift;
    if (key != NO_KEY && r < (uint64_t)n_rows && is_run_head(sorted, shift, j, r) && (sorted[j + CHUNK] >> shift) == r) found = j;
  }
  for (int o = (1 << lg) >> 1; o > 0; o >>= 1) {
    const int64_t other = __shfl_xor(found, o, 1 << lg);
    found = other > found ? other : found;
  }
  return found;
}

// the row r and the number of chunks of the long run whose head is `found`; chunk k > 0 starts at found + k * CHUNK
__device__ __forceinline__ int64_t run_chunks(const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t found, uint64_t& r) {
  r = sorted[found] >> shift;
  const int64_t end = lower_bound(sorted, found + CHUNK + 1, S, (r + 1) << shift);
  return (end - found + CHUNK - 1) / CHUNK;
}

__host__ __device__ __forceinline__ int64_t part_slot(int64_t q, bool is_head) { return 2 * (q / CHUNK) + (is_head ? 0 : 1); }
__host__ __device__ __forceinline__ int64_t part_slots(int64_t S) { return 2 * ((S + CHUNK - 1) / CHUNK); }
__host__ __device__ __forceinline__ int64_t part_pitch(int64_t C) { return (C + 3) / 4 * 4; }

// hipCUB item counts are int; row and position share one 64-bit key
inline bool sizes_ok(int64_t S, int64_t n_rows) { return S >= 0 && S < 0x7fffffffLL && n_rows >= 0 && n_rows < 0x7fffffffLL; }

// workgroups of THREADS for n items served by 2^lg lanes each
inline int64_t blocks_for(int64_t n, int lg) {
  const int64_t per_block = THREADS >> lg;
  return (n + per_block - 1) / per_block;
}

// launch(std::integral_constant<int, W>): a launch list names its arguments once for the 16-byte (W = 4) and the scalar (W = 1) path
template <class L>
inline void dispatch_w(bool vec4, L&& launch) {
  if (vec4) launch(std::integral_constant<int, 4>{});
  else launch(std::integral_constant<int, 1>{});
}

}  // namespace egnn_rows
