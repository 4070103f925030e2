// Backward of a row gather x[idx] whose ids may repeat: dst[r] = (dst[r] +) the sum of src[p] over the positions p with idx[p] == r,
// as torch's index backward defines it -- without float atomics and in an order that is a function of (idx, C) alone.
//
// The plan (egnn_rows_plan_build_i64, once per index tensor): position p naming row r gets the key (r << shift) | p (rows_keys.h; an
// id in [-n_rows, 0) is wrapped first, an id outside [-n_rows, n_rows) gets no key and is counted), the keys are radix-sorted, and
// four counters are taken from the sorted list (entries out of range, entries that are not the head of their run, entries that
// were negative, the longest run).  A row's positions then form one run of the sorted list, in ascending position.
//
// The sum (egnn_rows_add_runs_f32): one lane group of G = min(64, pow2ceil(C / 4)) lanes per sorted position (float4 per lane; a
// scalar path with G = min(64, pow2ceil(C)) when C, a pitch or a pointer does not allow it).  Only the groups at chunk starts work:
// a run is cut, from its head, into chunks of EGNN_ROWS_SUM_CHUNK entries, and the group at a chunk's first position adds that
// chunk's src rows in registers in ascending position.  A run of one chunk goes straight to dst.  The chunks of a longer run (a hub:
// edge endpoints repeat a node as often as it has edges) are summed by different groups at the same time and leave their partial
// rows in the workspace; a second launch adds a run's partials in ascending chunk order.  Whether a position starts a chunk is
// read off the sorted keys (its run's head is found by a binary search, and only for positions whose key CHUNK places earlier
// names the same row), so the cut never depends on the launch geometry.  Partial slots: the chunk that starts at sorted position q
// takes slot 2 (q / CHUNK) + (q is not its run's head); a window of CHUNK consecutive positions holds at most one head of a run
// longer than CHUNK and at most one later chunk start, so 2 ceil(S / CHUNK) slots never collide.
#include "rows_keys.h"

namespace {

using namespace egnn_rows;

constexpr int THREADS = 256;
constexpr int64_t CHUNK = EGNN_ROWS_SUM_CHUNK;

__device__ __forceinline__ float4 zero_of(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float zero_of(float) { return 0.f; }
__device__ __forceinline__ void add_to(float4& s, const float4 x) { s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w; }
__device__ __forceinline__ void add_to(float& s, const float x) { s += x; }
template <class T> __device__ __forceinline__ T load_at(const float* p) { return *reinterpret_cast<const T*>(p); }
template <class T> __device__ __forceinline__ void store_at(float* p, const T v) { *reinterpret_cast<T*>(p) = v; }

// first position in [lo, hi) whose key is >= key (hi when there is none); the sorted list is ascending as 64-bit values
__device__ __forceinline__ int64_t lower_bound(const uint64_t* __restrict__ sorted, int64_t lo, int64_t hi, uint64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void rows_counters_zero_kernel(int32_t* __restrict__ counters) {
  if (threadIdx.x < 4) counters[threadIdx.x] = 0;
}

__device__ __forceinline__ void count_flags(bool flag, int32_t* counter) {
  const unsigned long long b = __ballot(flag);
  if (b != 0 && egnn_lane() == (int)(__ffsll((long long)b) - 1)) atomicAdd(counter, (int)__popcll(b));
}

// keys[i] = (wrapped idx[i] << shift) | i; counters[0] += ids outside [-n_rows, n_rows) (NO_KEY), counters[2] += wrapped ids
__global__ __launch_bounds__(THREADS) void rows_keys_kernel(const int64_t* __restrict__ idx, int64_t S, int64_t n_rows, int shift,
                                                            uint64_t* __restrict__ keys, int32_t* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const bool live = i < S;
  int64_t r = live ? idx[i] : 0;
  const bool neg = live && r < 0 && r >= -n_rows;
  if (neg) r += n_rows;
  const bool out = live && (r < 0 || r >= n_rows);
  if (live) keys[i] = out ? NO_KEY : make_key(r, shift, i);
  count_flags(out, counters + 0);
  count_flags(neg, counters + 2);
}

// counters[1] += keyed entries that are not the head of their run; counters[3] = max run length
__global__ __launch_bounds__(THREADS) void rows_run_stats_kernel(const uint64_t* __restrict__ sorted, int64_t S, int shift,
                                                                 int32_t* __restrict__ counters) {
  const int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const uint64_t key = j < S ? sorted[j] : NO_KEY;
  const bool keyed = key != NO_KEY;
  const uint64_t r = key >> shift;
  const bool head = keyed && (j == 0 || (sorted[j - 1] >> shift) != r);
  count_flags(keyed && !head, counters + 1);
  int len = 0;
  if (head) len = (int)(lower_bound(sorted, j + 1, S, (r + 1) << shift) - j);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o));
  if (egnn_lane() == 0 && len > 0) atomicMax(counters + 3, len);
}

// accumulate == 0: a row that no key names is zeroed (one lane group per row; the rows that have a run are written by its head)
template <class T>
__global__ __launch_bounds__(THREADS) void rows_zero_absent_kernel(float* __restrict__ dst, int64_t ldd, int64_t n_rows,
                                                                   const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C,
                                                                   int lg) {
  constexpr int W = sizeof(T) / 4;
  const int64_t row = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
  if (row >= n_rows) return;
  const int64_t q = lower_bound(sorted, 0, S, (uint64_t)row << shift);
  if (q < S && (sorted[q] >> shift) == (uint64_t)row) return;
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) store_at<T>(dst + row * ldd + c, zero_of(T{}));
}

// ((src[p1] + src[p2]) + ...) over the sorted positions q = j, j + 1, ... < limit whose key names row r, columns c .. c + W - 1.
// Four keys and rows are in flight at a time; the additions stay in ascending position.  A position outside [0, S) (a key list
// that was not built for this src) is never used as an address.
template <class T>
__device__ __forceinline__ T run_sum(const uint64_t* __restrict__ sorted, int64_t j, int64_t limit, uint64_t r, int shift, int64_t S,
                                     const float* __restrict__ src, int64_t lds_, int64_t c) {
  const uint64_t mask = (uint64_t(1) << shift) - 1;
  const uint64_t p0 = sorted[j] & mask;
  T s = p0 < (uint64_t)S ? load_at<T>(src + (int64_t)p0 * lds_ + c) : zero_of(T{});
  for (int64_t q = j + 1; q < limit; q += 4) {
    uint64_t k[4];
    T x[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = q + i < limit ? sorted[q + i] : NO_KEY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ok[i] = (k[i] >> shift) == r && (k[i] & mask) < (uint64_t)S;
      x[i] = ok[i] ? load_at<T>(src + (int64_t)(k[i] & mask) * lds_ + c) : zero_of(T{});
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ok[i]) add_to(s, x[i]);
    if ((k[3] >> shift) != r) break;
  }
  return s;
}

__device__ __forceinline__ int64_t part_slot(int64_t q, bool is_head) { return 2 * (q / CHUNK) + (is_head ? 0 : 1); }

// pass 1: the lane group at sorted position j sums the chunk that starts there (if one does)
template <class T>
__global__ __launch_bounds__(THREADS) void rows_add_runs_kernel(float* __restrict__ dst, int64_t ldd, int64_t n_rows,
                                                                const uint64_t* __restrict__ sorted, int64_t S, int shift,
                                                                const float* __restrict__ src, int64_t lds_, int64_t C, int accumulate,
                                                                float* __restrict__ part, int64_t ldp, int lg) {
  constexpr int W = sizeof(T) / 4;
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
  if (long_run && part == nullptr) return;                             // (the entry point refuses this: S > CHUNK without a workspace)
  const int64_t limit = j + CHUNK < S ? j + CHUNK : S;
  float* out = long_run ? part + part_slot(j, head) * ldp : dst + (int64_t)r * ldd;
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    T s = run_sum<T>(sorted, j, limit, r, shift, S, src, lds_, c);
    if (!long_run && accumulate) {
      T d = load_at<T>(out + c);
      add_to(d, s);
      s = d;
    }
    store_at<T>(out + c, s);
  }
}

// pass 2: one lane group per window of CHUNK sorted positions; the (at most one) head of a run longer than CHUNK in the window adds
// the run's partial rows in ascending chunk order: dst[r] = (dst[r] +) ((P0 + P1) + ...)
template <class T>
__global__ __launch_bounds__(THREADS) void rows_add_parts_kernel(float* __restrict__ dst, int64_t ldd, int64_t n_rows,
                                                                 const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C,
                                                                 int accumulate, const float* __restrict__ part, int64_t ldp, int lg) {
  constexpr int W = sizeof(T) / 4;
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
  float* out = dst + (int64_t)r * ldd;
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    T s = load_at<T>(part + part_slot(found, true) * ldp + c);
    for (int64_t k = 1; k < chunks; ++k) add_to(s, load_at<T>(part + part_slot(found + k * CHUNK, false) * ldp + c));
    if (accumulate) {
      T d = load_at<T>(out + c);
      add_to(d, s);
      s = d;
    }
    store_at<T>(out + c, s);
  }
}

int64_t blocks_for(int64_t n, int lg) {
  const int64_t per_block = THREADS >> lg;
  return (n + per_block - 1) / per_block;
}

int64_t part_pitch(int64_t C) { return (C + 3) / 4 * 4; }

template <class T>
void launch_add_runs(float* dst, int64_t ld_dst, int64_t n_rows, const uint64_t* sorted, int64_t S, int shift, const float* src,
                     int64_t ld_src, int64_t C, int accumulate, float* part, hipStream_t st) {
  const int lg = lanes_lg(C / (int64_t)(sizeof(T) / 4));
  const int64_t ldp = part_pitch(C);
  if (!accumulate)
    hipLaunchKernelGGL(rows_zero_absent_kernel<T>, dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, dst, ld_dst, n_rows, sorted,
                       S, shift, C, lg);
  if (S == 0) return;
  hipLaunchKernelGGL(rows_add_runs_kernel<T>, dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, st, dst, ld_dst, n_rows, sorted, S, shift,
                     src, ld_src, C, accumulate, part, ldp, lg);
  if (S > CHUNK)
    hipLaunchKernelGGL(rows_add_parts_kernel<T>, dim3((unsigned)blocks_for((S + CHUNK - 1) / CHUNK, lg)), dim3(THREADS), 0, st, dst, ld_dst,
                       n_rows, sorted, S, shift, C, accumulate, (const float*)part, ldp, lg);
}

bool sizes_ok(int64_t S, int64_t n_rows) { return S >= 0 && S < 0x7fffffffLL && n_rows >= 0 && n_rows < 0x7fffffffLL; }

}  // namespace

extern "C" size_t egnn_rows_plan_ws_bytes(int64_t S, int64_t n_rows) {
  if (S <= 0 || !sizes_ok(S, n_rows) || n_rows == 0) return kAlign;
  size_t temp = 0;
  if (!sort_keys_temp(S, bits_for((uint64_t)S - 1) + bits_for((uint64_t)n_rows), &temp)) temp = 0;   // no device to ask (the build then refuses)
  return align_up((size_t)S * 8) + align_up(temp) + kAlign;
}

extern "C" int egnn_rows_plan_build_i64(const int64_t* idx, int64_t S, int64_t n_rows, uint64_t* keys_sorted, int32_t* counters, void* ws,
                                        size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows));                                 // hipCUB item counts are int; row and position share one 64-bit key
  if (S == 0) return EGNN_OK;
  EGNN_CHECK_ARG(idx && keys_sorted && counters);
  if (!ws || ws_bytes < egnn_rows_plan_ws_bytes(S, n_rows)) return EGNN_EWORKSPACE;
  if (!egnn_aligned16(ws) || (reinterpret_cast<uintptr_t>(keys_sorted) & 7u) != 0 || (reinterpret_cast<uintptr_t>(counters) & 3u) != 0)
    return EGNN_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int shift = bits_for((uint64_t)S - 1), end_bit = shift + bits_for((uint64_t)n_rows);
  size_t temp = 0;
  if (n_rows > 0 && !sort_keys_temp(S, end_bit, &temp)) return EGNN_ELAUNCH;
  const unsigned blocks = (unsigned)((S + THREADS - 1) / THREADS);
  hipLaunchKernelGGL(rows_counters_zero_kernel, dim3(1), dim3(64), 0, st, counters);
  // an empty table: every entry is out of range; the keys (all NO_KEY) need no sort
  uint64_t* keys = n_rows > 0 ? (uint64_t*)ws : keys_sorted;
  hipLaunchKernelGGL(rows_keys_kernel, dim3(blocks), dim3(THREADS), 0, st, idx, S, n_rows, shift, keys, counters);
  if (n_rows == 0) return egnn_launch_status();
  char* p = (char*)ws + align_up((size_t)S * 8);
  if (!sort_keys(p, ws_bytes - align_up((size_t)S * 8), keys, keys_sorted, S, end_bit, st)) return EGNN_ELAUNCH;
  hipLaunchKernelGGL(rows_run_stats_kernel, dim3(blocks), dim3(THREADS), 0, st, (const uint64_t*)keys_sorted, S, shift, counters);
  return egnn_launch_status();
}

extern "C" size_t egnn_rows_add_runs_ws_bytes(int64_t S, int64_t C) {
  if (S <= CHUNK || S >= 0x7fffffffLL || C <= 0) return 0;
  return (size_t)(2 * ((S + CHUNK - 1) / CHUNK)) * (size_t)part_pitch(C) * sizeof(float);
}

extern "C" int egnn_rows_add_runs_f32(float* dst, int64_t ld_dst, int64_t n_rows, const uint64_t* keys_sorted, int64_t S, int shift,
                                      const float* src, int64_t ld_src, int64_t C, int accumulate, void* ws, size_t ws_bytes,
                                      void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows) && C > 0 && ld_dst >= C && ld_src >= C && (accumulate == 0 || accumulate == 1));
  if (S == 0 && (accumulate == 1 || n_rows == 0 || dst == nullptr)) return EGNN_OK;
  EGNN_CHECK_ARG(dst && n_rows > 0);
  if (S > 0) EGNN_CHECK_ARG(keys_sorted && src && shift == bits_for((uint64_t)S - 1));
  if (S == 0) shift = 0;
  const size_t need = egnn_rows_add_runs_ws_bytes(S, C);
  if (need > 0 && (!ws || ws_bytes < need)) return EGNN_EWORKSPACE;
  if ((need > 0 && !egnn_aligned16(ws)) || (reinterpret_cast<uintptr_t>(keys_sorted) & 7u) != 0) return EGNN_EALIGN;
  const bool vec4 = C % 4 == 0 && ld_dst % 4 == 0 && ld_src % 4 == 0 && egnn_aligned16(dst) && egnn_aligned16(src);
  float* part = need > 0 ? (float*)ws : nullptr;
  if (vec4) launch_add_runs<float4>(dst, ld_dst, n_rows, keys_sorted, S, shift, src, ld_src, C, accumulate, part, (hipStream_t)stream);
  else launch_add_runs<float>(dst, ld_dst, n_rows, keys_sorted, S, shift, src, ld_src, C, accumulate, part, (hipStream_t)stream);
  return egnn_launch_status();
}
