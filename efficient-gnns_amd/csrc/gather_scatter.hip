// Gather, weight and aggregate in ONE walk over the sorted (row, position) keys of egnn_rows_plan_build_i64: what
// ops.scatter(ops.take_rows(x, src) * w, dst) computes, without the [E, C] message tensor in either direction -- and the per-edge dot
// that is the weights' gradient.  No float or integer atomics.
//
// egnn_gather_scatter_runs_f32: the cut, the partial slots and the two passes of rows_runs.h, with the fold reading
// x[from[p]] (/ from_count[from[p]]) * w[p, head] instead of src[p].  The chain key -> position -> from[position] -> row is three
// dependent loads; gather_chunk4 keeps four of each stage in flight (keys, then ids and weights, then rows), as fold_chunk4 does for
// its two.  It is a fold of its own: the shared one takes the row address from the key alone, and a second id load inside its fold
// callback would serialise the stages.  The product is rounded to fp32 before it is added (-ffp-contract=off), the first product of a
// chunk is taken as it is and the others are added in ascending position, long runs meet in ws in ascending chunk order: the order of
// egnn_rows_add_runs_f32, so the result is bit-equal to that run-sum over materialised messages.  The backward of x is the same entry
// point over the source side's keys with the roles swapped (from = the target rows, from_count = the mean's counts).
//
// egnn_edge_dot_f32: one lane group per (position, head); see the order of the additions at the kernel.
#include "rows_runs.h"

namespace {

using namespace egnn_rows;

enum { SUM = 0, MEAN = 1 };

// rows that no key names: 0 (one lane group per row)
template <int W>
__global__ __launch_bounds__(THREADS) void gs_zero_absent_kernel(float* __restrict__ out, int64_t ldo, int64_t n_rows,
                                                                 const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C, int lg) {
  int sub;
  const int64_t row = group_item(lg, sub);
  if (row >= n_rows || row_has_run(sorted, S, shift, row)) return;
  const float zero[W] = {};
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) store_w<W>(out + row * ldo + c, zero);
}

// what one walk reads besides the keys
struct Gather {
  const int64_t* from;      // [S]: the row of x that position p reads; outside [0, n_x): a zero row, nothing is read
  const float* x;           // [n_x, ldx]
  int64_t ldx, n_x;
  const int32_t* from_count;  // nullable, [n_x]: the gathered row is divided by (float)from_count[from[p]] first
  const float* w;           // nullable, [S, ldw]: the weight of (position, head)
  int64_t ldw;
};

// The chunk's sorted positions q = first .. limit - 1 of row r, columns c .. c + W - 1 (all of head h): fold(m) is called in ascending
// position for every usable key with m = (x[from[p]] / count) * w[p, h], each step rounded to fp32.  Four keys, then four ids and
// weights, then four rows are in flight.
template <int W, class Fold>
__device__ __forceinline__ void gather_chunk4(const uint64_t* __restrict__ sorted, int64_t first, int64_t limit, uint64_t r, int shift,
                                              int64_t S, const Gather& g, int64_t h, int64_t c, Fold fold) {
  for (int64_t q = first; q < limit; q += 4) {
    uint64_t k[4];
    int64_t f[4];
    float wt[4], d[4], x[4][W];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) k[u] = q + u < limit ? sorted[q + u] : NO_KEY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ok[u] = key_usable(k[u], r, shift, S);
      const int64_t p = (int64_t)key_pos(k[u], shift);
      f[u] = ok[u] ? g.from[p] : -1;
      wt[u] = ok[u] && g.w != nullptr ? g.w[p * g.ldw + h] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool live = f[u] >= 0 && f[u] < g.n_x;
#pragma unroll
      for (int i = 0; i < W; ++i) x[u][i] = 0.f;
      d[u] = 1.f;
      if (live) {
        load_w<W>(g.x + f[u] * g.ldx + c, x[u]);
        if (g.from_count != nullptr) d[u] = (float)g.from_count[f[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!ok[u]) continue;
      if (g.from_count != nullptr)
#pragma unroll
        for (int i = 0; i < W; ++i) x[u][i] = x[u][i] / d[u];
      if (g.w != nullptr)
#pragma unroll
        for (int i = 0; i < W; ++i) x[u][i] = x[u][i] * wt[u];
      fold(x[u]);
    }
    if ((k[3] >> shift) != r) break;
  }
}

// pass 1: the lane group at sorted position j sums the chunk that starts there (if one does); the first message is taken as it is
template <int W>
__global__ __launch_bounds__(THREADS) void gs_runs_kernel(float* __restrict__ out, int64_t ldo, int64_t n_rows,
                                                          const uint64_t* __restrict__ sorted, int64_t S, int shift, Gather g, int64_t C,
                                                          int64_t D, float* __restrict__ part, int64_t ldp, int lg) {
  int sub;
  const int64_t j = group_item(lg, sub);
  chunk_start(sorted, S, shift, n_rows, j, [&](bool head, uint64_t r) {
    const bool long_run = chunk_is_long(sorted, S, shift, j, head, r);
    if (long_run && part == nullptr) return;                           // (the entry point refuses this: S > CHUNK without a workspace)
    float* dst = long_run ? part + part_slot(j, head) * ldp : out + (int64_t)r * ldo;
    for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
      const int64_t h = D == C ? 0 : (int64_t)((uint32_t)c / (uint32_t)D);
      float acc[W] = {};
      bool any = false;
      gather_chunk4<W>(sorted, j, chunk_limit(j, S), r, shift, S, g, h, c, [&acc, &any](const float (&m)[W]) {
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = any ? acc[i] + m[i] : m[i];
        any = true;
      });
      store_w<W>(dst + c, acc);
    }
  });
}

// pass 2: one lane group per window of CHUNK sorted positions; the (at most one) head of a run longer than CHUNK in the window adds
// the run's partial rows in ascending chunk order (rows_add_parts_kernel's arithmetic)
template <int W>
__global__ __launch_bounds__(THREADS) void gs_parts_kernel(float* __restrict__ out, int64_t ldo, int64_t n_rows,
                                                           const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C,
                                                           const float* __restrict__ part, int64_t ldp, int lg) {
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
#pragma unroll
      for (int i = 0; i < W; ++i) s[i] += x[i];
    }
    store_w<W>(out + (int64_t)r * ldo + c, s);
  }
}

// count[row] = the length of row's run; mean: out[row, :] /= float(count) (scatter.hip's scatter_count_kernel, the same division)
template <int W>
__global__ __launch_bounds__(THREADS) void gs_count_kernel(float* __restrict__ out, int64_t ldo, int32_t* __restrict__ count, int64_t n_rows,
                                                           const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C, int divide,
                                                           int lg) {
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

// dw[p, h] = sum over the D columns of head h of A[a_rows[p], c] * B[b_rows[p], c] (/ (float)a_count[a_rows[p]]).
// ORDER OF THE ADDITIONS, a function of (C, H) only: with D = C / H and G = min(64, pow2ceil(ceil(D / 4))) lanes, lane l starts from
// 0.f and adds the products (each rounded to fp32) of the head's columns 4 (l + G t) + i, t = 0, 1, ..., i = 0 .. 3, below D, in
// ascending column order; the G lane sums meet in egnn_group_sum<G> (xor offsets G / 2 .. 1).  VEC only changes how the same
// columns are loaded (16 bytes when D % 4 == 0 and pitches and bases allow it).
template <int G, bool VEC>
__global__ __launch_bounds__(THREADS) void edge_dot_kernel(float* __restrict__ dw, int64_t ldd, int64_t S, int64_t H, int64_t D,
                                                           const int64_t* __restrict__ a_rows, const float* __restrict__ A, int64_t lda,
                                                           int64_t n_a, const int64_t* __restrict__ b_rows, const float* __restrict__ B,
                                                           int64_t ldb, int64_t n_b, const int32_t* __restrict__ a_count) {
  const int l = threadIdx.x & (G - 1);
  const int64_t item = (int64_t)blockIdx.x * (THREADS / G) + threadIdx.x / G;
  if (item >= S * H) return;                                           // (whole lane groups leave: the butterfly below stays within a group)
  const int64_t p = H == 1 ? item : (int64_t)((uint64_t)item / (uint64_t)H);
  const int64_t h = item - p * H;
  const int64_t ra = a_rows[p], rb = b_rows[p];
  const bool live = ra >= 0 && ra < n_a && rb >= 0 && rb < n_b;
  float s = 0.f;
  if (live) {
    const float* a = A + ra * lda + h * D;
    const float* b = B + rb * ldb + h * D;
    for (int64_t c = 4 * (int64_t)l; c < D; c += 4 * G) {
      float av[4] = {}, bv[4] = {};
      if (VEC) {
        load_w<4>(a + c, av);
        load_w<4>(b + c, bv);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c + i < D) av[i] = a[c + i], bv[i] = b[c + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (VEC || c + i < D) s += av[i] * bv[i];
    }
  }
  s = egnn_group_sum<G>(s);
  if (l != 0) return;
  if (live && a_count != nullptr) s = s / (float)a_count[ra];
  dw[p * ldd + h] = s;
}

template <int G>
void launch_edge_dot(bool vec, unsigned blocks, hipStream_t st, float* dw, int64_t ldd, int64_t S, int64_t H, int64_t D, const int64_t* a_rows,
                     const float* A, int64_t lda, int64_t n_a, const int64_t* b_rows, const float* B, int64_t ldb, int64_t n_b,
                     const int32_t* a_count) {
  if (vec)
    hipLaunchKernelGGL((edge_dot_kernel<G, true>), dim3(blocks), dim3(THREADS), 0, st, dw, ldd, S, H, D, a_rows, A, lda, n_a, b_rows, B, ldb, n_b,
                       a_count);
  else
    hipLaunchKernelGGL((edge_dot_kernel<G, false>), dim3(blocks), dim3(THREADS), 0, st, dw, ldd, S, H, D, a_rows, A, lda, n_a, b_rows, B, ldb, n_b,
                       a_count);
}

}  // namespace

extern "C" size_t egnn_gather_scatter_ws_bytes(int64_t S, int64_t C) { return egnn_rows_add_runs_ws_bytes(S, C); }

extern "C" int egnn_gather_scatter_runs_f32(float* out, int64_t ld_out, int64_t n_rows, int32_t* count, const uint64_t* keys_sorted, int64_t S,
                                            int shift, const int64_t* from, const float* x, int64_t ld_x, int64_t n_x,
                                            const int32_t* from_count, const float* w, int64_t ld_w, int64_t H, int64_t C, int reduce,
                                            void* ws, size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows) && C > 0 && C < 0x7fffffffLL && H >= 1 && C % H == 0 && ld_out >= C && ld_x >= C && n_x >= 0 &&
                 (reduce == SUM || reduce == MEAN));
  EGNN_CHECK_ARG(w == nullptr ? (H == 1 || S == 0) : ld_w >= H);
  if (S == 0 && (n_rows == 0 || out == nullptr)) return EGNN_OK;
  EGNN_CHECK_ARG(out && n_rows > 0);
  EGNN_CHECK_ARG(reduce != MEAN || count != nullptr);
  if (S > 0) EGNN_CHECK_ARG(keys_sorted && from && (x || n_x == 0) && shift == bits_for((uint64_t)S - 1));
  if (S == 0) shift = 0;
  const size_t need = egnn_gather_scatter_ws_bytes(S, C);
  if (need > 0 && (!ws || ws_bytes < need)) return EGNN_EWORKSPACE;
  if ((need > 0 && !egnn_aligned16(ws)) || ((reinterpret_cast<uintptr_t>(keys_sorted) | reinterpret_cast<uintptr_t>(from)) & 7u) != 0 ||
      ((reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(from_count) | reinterpret_cast<uintptr_t>(w) |
        reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3u) != 0)
    return EGNN_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int64_t D = C / H;
  const bool vec4 = D % 4 == 0 && ld_out % 4 == 0 && ld_x % 4 == 0 && egnn_aligned16(out) && egnn_aligned16(x);
  const Gather g{from, x, ld_x, n_x, from_count, w, ld_w};
  float* part = need > 0 ? (float*)ws : nullptr;
  dispatch_w(vec4, [&](auto wd) {
    constexpr int W = decltype(wd)::value;
    const int lg = lanes_lg(C / W);
    const int64_t ldp = part_pitch(C);
    hipLaunchKernelGGL(gs_zero_absent_kernel<W>, dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, out, ld_out, n_rows, keys_sorted, S,
                       shift, C, lg);
    if (S > 0)
      hipLaunchKernelGGL(gs_runs_kernel<W>, dim3((unsigned)blocks_for(S, lg)), dim3(THREADS), 0, st, out, ld_out, n_rows, keys_sorted, S, shift, g,
                         C, D, part, ldp, lg);
    if (S > CHUNK)
      hipLaunchKernelGGL(gs_parts_kernel<W>, dim3((unsigned)blocks_for(part_slots(S) / 2, lg)), dim3(THREADS), 0, st, out, ld_out, n_rows,
                         keys_sorted, S, shift, C, (const float*)part, ldp, lg);
    if (count != nullptr)
      hipLaunchKernelGGL(gs_count_kernel<W>, dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, out, ld_out, count, n_rows, keys_sorted,
                         S, shift, C, (int)(reduce == MEAN), lg);
  });
  return egnn_launch_status();
}

extern "C" int egnn_edge_dot_f32(float* dw, int64_t ld_dw, int64_t S, int64_t H, int64_t C, const int64_t* a_rows, const float* A,
                                 int64_t ld_a, int64_t n_a, const int64_t* b_rows, const float* B, int64_t ld_b, int64_t n_b,
                                 const int32_t* a_count, void* stream) {
  EGNN_CHECK_ARG(S >= 0 && S < 0x7fffffffLL && C > 0 && C < 0x7fffffffLL && H >= 1 && C % H == 0 && ld_dw >= H && ld_a >= C && ld_b >= C &&
                 n_a >= 0 && n_b >= 0);
  if (S == 0) return EGNN_OK;
  EGNN_CHECK_ARG(dw && a_rows && b_rows && (A || n_a == 0) && (B || n_b == 0));
  if (((reinterpret_cast<uintptr_t>(a_rows) | reinterpret_cast<uintptr_t>(b_rows)) & 7u) != 0 ||
      ((reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) |
        reinterpret_cast<uintptr_t>(a_count)) & 3u) != 0)
    return EGNN_EALIGN;
  const int64_t D = C / H;
  const int lg = lanes_lg((D + 3) / 4);
  const int64_t blocks = blocks_for(S * H, lg);
  EGNN_CHECK_ARG(blocks < 0x7fffffffLL);
  const bool vec = D % 4 == 0 && ld_a % 4 == 0 && ld_b % 4 == 0 && egnn_aligned16(A) && egnn_aligned16(B);
  hipStream_t st = (hipStream_t)stream;
#define EGNN_EDGE_DOT(G) \
  launch_edge_dot<G>(vec, (unsigned)blocks, st, dw, ld_dw, S, H, D, a_rows, A, ld_a, n_a, b_rows, B, ld_b, n_b, a_count)
  switch (lg) {
    case 0: EGNN_EDGE_DOT(1); break;
    case 1: EGNN_EDGE_DOT(2); break;
    case 2: EGNN_EDGE_DOT(4); break;
    case 3: EGNN_EDGE_DOT(8); break;
    case 4: EGNN_EDGE_DOT(16); break;
    case 5: EGNN_EDGE_DOT(32); break;
    default: EGNN_EDGE_DOT(64); break;
  }
#undef EGNN_EDGE_DOT
  return egnn_launch_status();
}
