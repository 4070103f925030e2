// Gather, add the edge's own row, activate and aggregate in ONE walk over the sorted (row, position) keys of egnn_rows_plan_build_i64:
// what ops.scatter(relu(ops.take_rows(x, src) + edge), dst) computes -- the message of every conv that reads edge features (GINE, the
// bond-aware GCN) -- without the two [E, C] tensors of the unfused spelling, in either direction.  No float or integer atomics.
//
// egnn_gather_edge_scatter_runs_f32: gather_scatter.hip's walk (the cut, the partial slots and the two passes of rows_runs.h) with the
// per-edge WEIGHT replaced by a per-edge ROW.  The chain key -> position -> from[position] -> row is three dependent loads and
// edge_chunk4 keeps four of each stage in flight, as gather_chunk4 does; e's address depends on the position only, so e[p] is loaded in
// the ids' stage and is in flight together with from[p].  Three messages (MODE):
//   ADD       m = v + e[p]                          v = x[from[p]] (/ (float)from_count[from[p]]); a from outside [0, n_x): a row of zeros
//   ADD_RELU  m = v + e[p] > 0 ? v + e[p] : +0      the sum rounded to fp32 first (-ffp-contract=off)
//   GATE      m = own[r] + e[p] > 0 ? v : +0        the backward of ADD_RELU for the gathered-from side: x is the upstream gradient, own
//                                                   the forward's x at the run's own row r (one load per column trip, outside the walk)
// Registers: four rows of e next to four rows of x are 16 more than gather_chunk4 holds.  The checked row id is kept in 32 bits, the
// division by counts is a template switch (CNT; the forward has none), and GATE turns its rows of e into four mask words BEFORE the rows
// of x are asked for -- the ids arrive together with e, so nothing waits longer, and the empty asm pins that order -- which keeps the
// 16-byte walks that ops launches for the relu at gs_runs_kernel's occupancy (profiles/gather_edge_scatter_resources.txt).
// The first message of a chunk is taken as it is, the others are added in ascending position, long runs meet in ws in ascending chunk
// order: egnn_rows_add_runs_f32's order, so the result is bit-equal to that run-sum over materialised messages.  The launches around
// pass 1 (rows no key names, the merge of the partials, the counts and mean's division) repeat gather_scatter.hip's arithmetic over
// the same shared pieces; they are kernels of this file because each file's launches live in its own unnamed namespace.
//
// egnn_edge_gate_f32: the gradient of the edge rows, elementwise, one lane group per position.
#include "rows_runs.h"

namespace {

using namespace egnn_rows;

enum { SUM = 0, MEAN = 1 };
enum { ADD = 0, ADD_RELU = 1, GATE = 2 };

// rows that no key names: 0 (one lane group per row)
template <int W>
__global__ __launch_bounds__(THREADS) void ges_zero_absent_kernel(float* __restrict__ out, int64_t ldo, int64_t n_rows,
                                                                  const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C, int lg) {
  int sub;
  const int64_t row = group_item(lg, sub);
  if (row >= n_rows || row_has_run(sorted, S, shift, row)) return;
  const float zero[W] = {};
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) store_w<W>(out + row * ldo + c, zero);
}

// what one walk reads besides the keys
struct EdgeGather {
  const int64_t* from;        // [S]: the row of x that position p reads; outside [0, n_x): a zero row, nothing is read
  const float* x;             // [n_x, ldx]
  int64_t ldx, n_x;
  const int32_t* from_count;  // nullable, [n_x]: the gathered row is divided by (float)from_count[from[p]] first
  const float* e;             // [S, lde]: the edge's own row (nullable for ADD only: nothing is added)
  int64_t lde;
  const float* own;           // GATE: [n_rows, ldown], the forward's x at the run's own row
  int64_t ldown;
};

// The chunk's sorted positions q = first .. limit - 1 of row r, columns c .. c + W - 1: fold(m) is called in ascending position for
// every usable key with the message of MODE (`own`: the GATE's own-row values of these columns; CNT: from_count is given), each step
// rounded to fp32.  Four
// keys, then four ids and four rows of e, then four rows of x are in flight.
template <int W, int MODE, bool CNT, class Fold>
__device__ __forceinline__ void edge_chunk4(const uint64_t* __restrict__ sorted, int64_t first, int64_t limit, uint64_t r, int shift,
                                            int64_t S, const EdgeGather& g, const float (&own)[W], int64_t c, Fold fold) {
  for (int64_t q = first; q < limit; q += 4) {
    uint64_t k[4];
    int f[4];                                                          // (n_x < 2^31 - 1: the checked id fits 32 bits, -1 = no row)
    float d[4], ev[4][W], x[4][W];
    unsigned open[4] = {};                                             // GATE: bit i = column c + i of position u lets the gradient through
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) k[u] = q + u < limit ? sorted[q + u] : NO_KEY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ok[u] = key_usable(k[u], r, shift, S);
      const int64_t p = (int64_t)key_pos(k[u], shift);
      const int64_t id = ok[u] ? g.from[p] : -1;
      f[u] = id >= 0 && id < g.n_x ? (int)id : -1;
#pragma unroll
      for (int i = 0; i < W; ++i) ev[u][i] = 0.f;
      if (ok[u] && (MODE != ADD || g.e != nullptr)) load_w<W>(g.e + p * g.lde + c, ev[u]);
    }
    if (MODE == GATE)                                                  // e arrives with the ids: its rows end here, before x's are asked for
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < W; ++i) open[u] |= (own[i] + ev[u][i] > 0.f ? 1u : 0u) << i;
    if (MODE == GATE) asm volatile("" : "+v"(open[0]), "+v"(open[1]), "+v"(open[2]), "+v"(open[3]) : : "memory");
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < W; ++i) x[u][i] = 0.f;
      d[u] = 1.f;
      if (f[u] >= 0) {
        load_w<W>(g.x + (int64_t)f[u] * g.ldx + c, x[u]);
        if (CNT) d[u] = (float)g.from_count[f[u]];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!ok[u]) continue;
      if (CNT)
#pragma unroll
        for (int i = 0; i < W; ++i) x[u][i] = x[u][i] / d[u];
      if (MODE == GATE) {
#pragma unroll
        for (int i = 0; i < W; ++i) x[u][i] = (open[u] >> i & 1u) != 0 ? x[u][i] : 0.f;
      } else if (MODE == ADD_RELU || g.e != nullptr) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const float s = x[u][i] + ev[u][i];
          x[u][i] = MODE == ADD || s > 0.f ? s : 0.f;
        }
      }
      fold(x[u]);
    }
    if ((k[3] >> shift) != r) break;
  }
}

// pass 1: the lane group at sorted position j sums the chunk that starts there (if one does); the first message is taken as it is
template <int W, int MODE, bool CNT>
__global__ __launch_bounds__(THREADS) void ges_runs_kernel(float* __restrict__ out, int64_t ldo, int64_t n_rows,
                                                           const uint64_t* __restrict__ sorted, int64_t S, int shift, EdgeGather g, int64_t C,
                                                           float* __restrict__ part, int64_t ldp, int lg) {
  int sub;
  const int64_t j = group_item(lg, sub);
  chunk_start(sorted, S, shift, n_rows, j, [&](bool head, uint64_t r) {
    const bool long_run = chunk_is_long(sorted, S, shift, j, head, r);
    if (long_run && part == nullptr) return;                           // (the entry point refuses this: S > CHUNK without a workspace)
    float* dst = long_run ? part + part_slot(j, head) * ldp : out + (int64_t)r * ldo;
    for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
      float own[W] = {};
      if (MODE == GATE) load_w<W>(g.own + (int64_t)r * g.ldown + c, own);
      float acc[W] = {};
      bool any = false;
      edge_chunk4<W, MODE, CNT>(sorted, j, chunk_limit(j, S), r, shift, S, g, own, c, [&acc, &any](const float (&m)[W]) {
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
__global__ __launch_bounds__(THREADS) void ges_parts_kernel(float* __restrict__ out, int64_t ldo, int64_t n_rows,
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

// count[row] = the length of row's run; mean: out[row, :] /= float(count) (gs_count_kernel's division)
template <int W>
__global__ __launch_bounds__(THREADS) void ges_count_kernel(float* __restrict__ out, int64_t ldo, int32_t* __restrict__ count, int64_t n_rows,
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

// de[p, c] = gate ? g[b_rows[p], c] / (float)b_count[b_rows[p]] : 0, gate = !RELU || x[a_rows[p], c] + e[p, c] > 0 (one lane group per p)
template <int W, bool RELU>
__global__ __launch_bounds__(THREADS) void edge_gate_kernel(float* __restrict__ de, int64_t ldd, int64_t S, int64_t C,
                                                            const int64_t* __restrict__ a_rows, const float* __restrict__ x, int64_t ldx,
                                                            int64_t n_x, const float* __restrict__ e, int64_t lde,
                                                            const int64_t* __restrict__ b_rows, const float* __restrict__ g, int64_t ldg,
                                                            int64_t n_g, const int32_t* __restrict__ b_count, int lg) {
  int sub;
  const int64_t p = group_item(lg, sub);
  if (p >= S) return;
  const int64_t rb = b_rows[p];
  const bool live = rb >= 0 && rb < n_g;
  int64_t ra = -1;
  if (RELU && live) ra = a_rows[p];
  const bool have_x = ra >= 0 && ra < n_x;                             // (an id outside x: a row of zeros, as the forward reads it)
  const float d = live && b_count != nullptr ? (float)b_count[rb] : 1.f;
  for (int64_t c = (int64_t)sub * W; c < C; c += (int64_t)W << lg) {
    float v[W] = {};
    if (live) {
      load_w<W>(g + rb * ldg + c, v);
      if (b_count != nullptr)
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = v[i] / d;
      if (RELU) {
        float xv[W] = {}, ev[W];
        if (have_x) load_w<W>(x + ra * ldx + c, xv);
        load_w<W>(e + p * lde + c, ev);
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = xv[i] + ev[i] > 0.f ? v[i] : 0.f;
      }
    }
    store_w<W>(de + p * ldd + c, v);
  }
}

}  // namespace

extern "C" size_t egnn_gather_edge_scatter_ws_bytes(int64_t S, int64_t C) { return egnn_rows_add_runs_ws_bytes(S, C); }

extern "C" int egnn_gather_edge_scatter_runs_f32(float* out, int64_t ld_out, int64_t n_rows, int32_t* count, const uint64_t* keys_sorted,
                                                 int64_t S, int shift, const int64_t* from, const float* x, int64_t ld_x, int64_t n_x,
                                                 const int32_t* from_count, const float* e, int64_t ld_e, const float* own, int64_t ld_own,
                                                 int mode, int64_t C, int reduce, void* ws, size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows) && C > 0 && C < 0x7fffffffLL && ld_out >= C && ld_x >= C && n_x >= 0 && n_x < 0x7fffffffLL &&
                 (reduce == SUM || reduce == MEAN) && (mode == ADD || mode == ADD_RELU || mode == GATE));
  EGNN_CHECK_ARG(e == nullptr ? (mode == ADD || S == 0) : ld_e >= C);
  EGNN_CHECK_ARG(mode != GATE || S == 0 || (own != nullptr && ld_own >= C));
  if (S == 0 && (n_rows == 0 || out == nullptr)) return EGNN_OK;
  EGNN_CHECK_ARG(out && n_rows > 0);
  EGNN_CHECK_ARG(reduce != MEAN || count != nullptr);
  if (S > 0) EGNN_CHECK_ARG(keys_sorted && from && (x || n_x == 0) && shift == bits_for((uint64_t)S - 1));
  if (S == 0) shift = 0;
  if (mode != GATE) own = nullptr;
  const size_t need = egnn_gather_edge_scatter_ws_bytes(S, C);
  if (need > 0 && (!ws || ws_bytes < need)) return EGNN_EWORKSPACE;
  if ((need > 0 && !egnn_aligned16(ws)) || ((reinterpret_cast<uintptr_t>(keys_sorted) | reinterpret_cast<uintptr_t>(from)) & 7u) != 0 ||
      ((reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(from_count) | reinterpret_cast<uintptr_t>(e) |
        reinterpret_cast<uintptr_t>(own) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 3u) != 0)
    return EGNN_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = C % 4 == 0 && ld_out % 4 == 0 && ld_x % 4 == 0 && egnn_aligned16(out) && egnn_aligned16(x) &&
                    (e == nullptr || (ld_e % 4 == 0 && egnn_aligned16(e))) && (own == nullptr || (ld_own % 4 == 0 && egnn_aligned16(own)));
  const EdgeGather g{from, x, ld_x, n_x, from_count, e, ld_e, own, ld_own};
  float* part = need > 0 ? (float*)ws : nullptr;
  dispatch_w(vec4, [&](auto wd) {
    constexpr int W = decltype(wd)::value;
    const int lg = lanes_lg(C / W);
    const int64_t ldp = part_pitch(C);
    hipLaunchKernelGGL(ges_zero_absent_kernel<W>, dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, out, ld_out, n_rows, keys_sorted, S,
                       shift, C, lg);
    if (S > 0) {
      const dim3 grid((unsigned)blocks_for(S, lg));
#define EGNN_GES_RUNS(MODE, CNT) \
  hipLaunchKernelGGL((ges_runs_kernel<W, MODE, CNT>), grid, dim3(THREADS), 0, st, out, ld_out, n_rows, keys_sorted, S, shift, g, C, part, ldp, lg)
      if (from_count != nullptr) {
        if (mode == ADD) EGNN_GES_RUNS(ADD, true);
        else if (mode == ADD_RELU) EGNN_GES_RUNS(ADD_RELU, true);
        else EGNN_GES_RUNS(GATE, true);
      } else {
        if (mode == ADD) EGNN_GES_RUNS(ADD, false);
        else if (mode == ADD_RELU) EGNN_GES_RUNS(ADD_RELU, false);
        else EGNN_GES_RUNS(GATE, false);
      }
#undef EGNN_GES_RUNS
    }
    if (S > CHUNK)
      hipLaunchKernelGGL(ges_parts_kernel<W>, dim3((unsigned)blocks_for(part_slots(S) / 2, lg)), dim3(THREADS), 0, st, out, ld_out, n_rows,
                         keys_sorted, S, shift, C, (const float*)part, ldp, lg);
    if (count != nullptr)
      hipLaunchKernelGGL(ges_count_kernel<W>, dim3((unsigned)blocks_for(n_rows, lg)), dim3(THREADS), 0, st, out, ld_out, count, n_rows, keys_sorted,
                         S, shift, C, (int)(reduce == MEAN), lg);
  });
  return egnn_launch_status();
}

extern "C" int egnn_edge_gate_f32(float* de, int64_t ld_de, int64_t S, int64_t C, const int64_t* a_rows, const float* x, int64_t ld_x,
                                  int64_t n_x, const float* e, int64_t ld_e, const int64_t* b_rows, const float* g, int64_t ld_g, int64_t n_g,
                                  const int32_t* b_count, int mode, void* stream) {
  EGNN_CHECK_ARG(S >= 0 && S < 0x7fffffffLL && C > 0 && C < 0x7fffffffLL && ld_de >= C && ld_g >= C && n_g >= 0 && n_x >= 0 &&
                 (mode == ADD || mode == ADD_RELU));
  EGNN_CHECK_ARG(mode == ADD || (ld_x >= C && ld_e >= C));
  if (S == 0) return EGNN_OK;
  EGNN_CHECK_ARG(de && b_rows && (g || n_g == 0));
  EGNN_CHECK_ARG(mode == ADD || (a_rows && e && (x || n_x == 0)));
  if (mode == ADD) a_rows = nullptr, x = nullptr, e = nullptr;
  if (((reinterpret_cast<uintptr_t>(a_rows) | reinterpret_cast<uintptr_t>(b_rows)) & 7u) != 0 ||
      ((reinterpret_cast<uintptr_t>(de) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(g) |
        reinterpret_cast<uintptr_t>(b_count)) & 3u) != 0)
    return EGNN_EALIGN;
  const bool vec4 = C % 4 == 0 && ld_de % 4 == 0 && ld_g % 4 == 0 && egnn_aligned16(de) && egnn_aligned16(g) &&
                    (mode == ADD || (ld_x % 4 == 0 && ld_e % 4 == 0 && egnn_aligned16(x) && egnn_aligned16(e)));
  hipStream_t st = (hipStream_t)stream;
  dispatch_w(vec4, [&](auto wd) {
    constexpr int W = decltype(wd)::value;
    const int lg = lanes_lg(C / W);
    const dim3 grid((unsigned)blocks_for(S, lg));
    if (mode == ADD)
      hipLaunchKernelGGL((edge_gate_kernel<W, false>), grid, dim3(THREADS), 0, st, de, ld_de, S, C, a_rows, x, ld_x, n_x, e, ld_e, b_rows, g, ld_g,
                         n_g, b_count, lg);
    else
      hipLaunchKernelGGL((edge_gate_kernel<W, true>), grid, dim3(THREADS), 0, st, de, ld_de, S, C, a_rows, x, ld_x, n_x, e, ld_e, b_rows, g, ld_g,
                         n_g, b_count, lg);
  });
  return egnn_launch_status();
}
