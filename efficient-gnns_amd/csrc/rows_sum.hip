// Backward of a row gather x[idx] whose ids may repeat: dst[r] = (dst[r] +) the sum of src[p] over the positions p with idx[p] == r,
// as torch's index backward defines it -- without float atomics and in an order that is a function of (idx, C) alone.
//
// The plan (egnn_rows_plan_build_i64, once per index tensor): position p naming row r gets the key (r << shift) | p (rows_keys.h; an
// id in [-n_rows, 0) is wrapped first, an id outside [-n_rows, n_rows) gets no key and is counted), the keys are radix-sorted, and
// four counters are taken from the sorted list (entries out of range, entries that are not the head of their run, entries that
// were negative, the longest run).  A row's positions then form one run of the sorted list, in ascending position.
//
// The sum (egnn_rows_add_runs_f32): one lane group of G = min(64, pow2ceil(C / 4)) lanes per sorted position (float4 per lane; a
// scalar path with G = min(64, pow2ceil(C)) when C, a pitch or a pointer does not allow it).  Only the groups at chunk starts work
// (the cut, the partial slots and the second pass: rows_runs.h): the group at a chunk's first position adds that chunk's src rows in
// registers in ascending position; a second launch adds a long run's partial rows in ascending chunk order.
#include "rows_runs.h"
#include "block_reduce.h"

namespace {

using namespace egnn_rows;

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
  const bool head = keyed && is_run_head(sorted, shift, j, r);
  count_flags(keyed && !head, counters + 1);
  int len = 0;
  if (head) len = (int)(lower_bound(sorted, j + 1, S, (r + 1) << shift) - j);
  len = egnn_reduce::group_max<EGNN_WAVE>(len);
  if (egnn_lane() == 0 && len > 0) atomicMax(counters + 3, len);
}

// accumulate == 0: a row that no key names is zeroed (one lane group per row; the rows that have a run are written by its head)
template <int W>
__global__ __launch_bounds__(THREADS) void rows_zero_absent_kernel(float* __restrict__ dst, int64_t ldd, int64_t n_rows,
                                                                   const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C,
                                                                   int lg) {
  int sub;
  const int64_t row = group_item(lg, sub);
  if (row >= n_rows || row_has_run(sorted, S, shift, row)) return;
  const float zero[W] = {};
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) store_w<W>(dst + row * ldd + c, zero);
}

template <int W> __device__ __forceinline__ void add_w(float (&s)[W], const float (&x)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) s[i] += x[i];
}

// s = ((src[p1] + src[p2]) + ...) over the sorted positions q = j, j + 1, ... < limit whose key names row r, columns c .. c + W - 1:
// the first row, then the additions in ascending position (0.f + -0.f is not -0.f)
template <int W>
__device__ __forceinline__ void run_sum(const uint64_t* __restrict__ sorted, int64_t j, int64_t limit, uint64_t r, int shift, int64_t S,
                                        const float* __restrict__ src, int64_t lds_, int64_t c, float (&s)[W]) {
  const uint64_t p0 = key_pos(sorted[j], shift);
  float acc[W] = {};
  if (p0 < (uint64_t)S) load_w<W>(src + (int64_t)p0 * lds_ + c, acc);
  fold_chunk4<W>(sorted, j + 1, limit, r, shift, S, src, lds_, c, [&acc](const float (&x)[W], int64_t) { add_w<W>(acc, x); });
#pragma unroll
  for (int i = 0; i < W; ++i) s[i] = acc[i];
}

// out[c ..] = (out[c ..] +) s
template <int W> __device__ __forceinline__ void put_row(float* out, int accumulate, float (&s)[W]) {
  if (accumulate) {
    float d[W];
    load_w<W>(out, d);
    add_w<W>(d, s);
#pragma unroll
    for (int i = 0; i < W; ++i) s[i] = d[i];
  }
  store_w<W>(out, s);
}

// pass 1: the lane group at sorted position j sums the chunk that starts there (if one does)
template <int W>
__global__ __launch_bounds__(THREADS) void rows_add_runs_kernel(float* __restrict__ dst, int64_t ldd, int64_t n_rows,
                                                                const uint64_t* __restrict__ sorted, int64_t S, int shift,
                                                                const float* __restrict__ src, int64_t lds_, int64_t C, int accumulate,
                                                                float* __restrict__ part, int64_t ldp, int lg) {
  int sub;
  const int64_t j = group_item(lg, sub);
  chunk_start(sorted, S, shift, n_rows, j, [&](bool head, uint64_t r) {
    const bool long_run = chunk_is_long(sorted, S, shift, j, head, r);
    if (long_run && part == nullptr) return;                           // (the entry point refuses this: S > CHUNK without a workspace)
    float* out = long_run ? part + part_slot(j, head) * ldp : dst + (int64_t)r * ldd;
    for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
      float s[W];
      run_sum<W>(sorted, j, chunk_limit(j, S), r, shift, S, src, lds_, c, s);
      put_row<W>(out + c, !long_run && accumulate, s);
    }
  });
}

// pass 2: one lane group per window of CHUNK sorted positions; the (at most one) head of a run longer than CHUNK in the window adds
// the run's partial rows in ascending chunk order: dst[r] = (dst[r] +) ((P0 + P1) + ...)
template <int W>
__global__ __launch_bounds__(THREADS) void rows_add_parts_kernel(float* __restrict__ dst, int64_t ldd, int64_t n_rows,
                                                                 const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C,
                                                                 int accumulate, const float* __restrict__ part, int64_t ldp, int lg) {
  int sub;
  const int64_t found = long_run_head(sorted, S, shift, n_rows, group_item(lg, sub) * CHUNK, sub, lg);
  if (found < 0) return;
  uint64_t r;
  const int64_t chunks = run_chunks(sorted, S, shift, found, r);
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    float s[W], x[W];
    load_w<W>(part + part_slot(found, true) * ldp + c, s);
    for (int64_t k = 1; k < chunks; ++k) {
      load_w<W>(part + part_slot(found + k * CHUNK, false) * ldp + c, x);
      add_w<W>(s, x);
    }
    put_row<W>(dst + (int64_t)r * ldd + c, accumulate, s);
  }
}

void launch_add_runs(bool vec4, float* dst, int64_t ld_dst, int64_t n_rows, const uint64_t* sorted, int64_t S, int shift, const float* src,
                     int64_t ld_src, int64_t C, int accumulate, float* part, hipStream_t st) {
  dispatch_w(vec4, [&](auto w) {
    constexpr int W = decltype(w)::value;
    const int lg = lanes_lg(C / W);
    const int64_t ldp = part_pitch(C);
    if (!accumulate)
      hipLaunchKernelGGL(rows_zero_absent_kernel<W>, dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, dst, ld_dst, n_rows, sorted,
                         S, shift, C, lg);
    if (S == 0) return;
    hipLaunchKernelGGL(rows_add_runs_kernel<W>, dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, st, dst, ld_dst, n_rows, sorted, S, shift,
                       src, ld_src, C, accumulate, part, ldp, lg);
    if (S > CHUNK)
      hipLaunchKernelGGL(rows_add_parts_kernel<W>, dim3((unsigned)blocks_for(part_slots(S) / 2, lg)), dim3(THREADS), 0, st, dst, ld_dst, n_rows,
                         sorted, S, shift, C, accumulate, (const float*)part, ldp, lg);
  });
}

}  // namespace

extern "C" size_t egnn_rows_plan_ws_bytes(int64_t S, int64_t n_rows) {
  if (S <= 0 || !sizes_ok(S, n_rows) || n_rows == 0) return kAlign;
  size_t temp = 0;
  if (!sort_keys_temp(S, bits_for((uint64_t)S - 1) + bits_for((uint64_t)n_rows), &temp)) temp = 0;   // no device to ask (the build then refuses)
  return align_up((size_t)S * 8) + align_up(temp) + kAlign;
}

extern "C" int egnn_rows_plan_build_i64(const int64_t* idx, int64_t S, int64_t n_rows, uint64_t* keys_sorted, int32_t* counters, void* ws,
                                        size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows));
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
  return (size_t)part_slots(S) * (size_t)part_pitch(C) * sizeof(float);
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
  launch_add_runs(vec4, dst, ld_dst, n_rows, keys_sorted, S, shift, src, ld_src, C, accumulate, part, (hipStream_t)stream);
  return egnn_launch_status();
}
