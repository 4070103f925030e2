// Softmax (and log-softmax) of E score rows over the groups of an UNSORTED index -- torch_scatter.scatter_softmax along dim 0, the step
// between the lift and the aggregation of an attention conv written in PyG's idiom (`alpha = softmax(alpha, index, ptr, size_i)` on
// [E, heads] scores) -- and its backward.  No float and no integer read-modify-write operations in either direction.
//
// Both directions are a RUN WALK over the sorted (row, position) keys of egnn_rows_plan_build_i64 (rows_keys.h, rows_sum.hip), which
// leaves per-row statistics in [n_rows, C] buffers, followed by a GATHER over the [S, C] elements that reads them back by rows[p].
//   forward walk:   row_max[r, c] = M = max_q x[q, c],  row_den[r, c] = Z = sum_q exp(x[q, c] - M)   over the positions q of row r's run
//   forward gather: out[p, c] = exp(x[p, c] - M) / (Z + eps)        (softmax: ONE true division per element, no reciprocal)
//                   out[p, c] = (x[p, c] - M) - log(Z + eps)        (log form)
//   backward walk:  row_dot[r, c] = sum_q out[q, c] * g[q, c]  (softmax; the products are formed in registers)  |  sum_q g[q, c]  (log form)
//   backward gather: dsrc[p, c] = out * (g - row_dot)  (softmax)  |  g - exp(out) * row_dot  (log form)
// A position with rows[p] outside [0, n_rows) (-1: an id the plan dropped) gets 0 from either gather; every element of out / dsrc and
// every row of the statistics is written with a plain store (a row that no key names gets 0), so no buffer needs a memset.
//
// LANE MAPPING.  C is the head count (1 - 16), so the lanes run along POSITIONS, not along columns.  One wave takes a window of 64
// consecutive sorted positions; lane i decides whether position (window + i) starts a chunk, the wave ballots those flags, and its
// four 16-lane groups take the window's chunk starts four at a time, in ascending position.  The cut of a run into chunks of
// EGNN_ROWS_SUM_CHUNK = 128 positions is the one of rows_runs.h (chunk_start), and no lane group walks more than one chunk: lane l of
// the group reads the chunk's offsets l, l + 16, ..., l + 112 (eight loads in flight per column), so a hub of degree 13 000 is ~100
// groups of 8 steps each, and a run of the common degrees is one group's single step.
// Columns are an outer loop of the group (four at a time, 16 bytes per lane, when C % 4 == 0 and every pitch and pointer allows it;
// one at a time otherwise): each column's arithmetic is the same scalar sequence on either path.
//
// ORDER OF THE ADDITIONS, a fixed function of a position's offset o in its chunk (0 <= o < 128), per column: with e_o the term of
// offset o (exp(x - m_j), out * g or g), lane l = o % 16 adds its terms in ascending offset,
//     s_l = ((e_l + e_(l+16)) + e_(l+32)) + ... + e_(l+112)                       (offsets past the chunk's end are left out),
// and the 16 lane sums meet in the xor butterfly of egnn_group_sum<16> (an empty lane adds 0):
//     t = (((s_0 + s_8) + (s_4 + s_12)) + ((s_2 + s_10) + (s_6 + s_14))) + (((s_1 + s_9) + (s_5 + s_13)) + ((s_3 + s_11) + (s_7 + s_15)))
// (every lane forms the same tree with commuted operands, hence the same bits).  The chunk maximum m_j is exact.  A run of one chunk
// goes straight to the row buffers.  The chunks of a longer run park their pairs (m_j, z_j) -- or their sums -- in the workspace (the
// slot rule of rows_runs.h), and a second launch merges them in ascending chunk order:
//     M = max_j m_j,  Z = ((z_0 e^(m_0 - M) + z_1 e^(m_1 - M)) + ...)  |  T = ((t_0 + t_1) + ...).
// Nothing above depends on the launch geometry, a pitch or the addressing path: the bits of out are a function of
// (index, C, values, eps, form) only, and column c of a [S, C] call equals the [S, 1] call on that column.
//
// A key whose position or row does not fit S / n_rows (keys built for other operands) is skipped and never used as an address.
// UNSPECIFIED inputs: NaN, +inf, and a run whose values are all -inf.
#include "rows_runs.h"
#include "block_reduce.h"

namespace {

using namespace egnn_rows;

constexpr int WAVES = THREADS / EGNN_WAVE;
constexpr int LG_ONE = 0, LG_WAVE = 6;        // log2 of the lanes per item: one thread, one wave
constexpr int GL = 16;                       // lanes of the group that walks one chunk
constexpr int STEPS = (int)(CHUNK / GL);      // positions per lane
static_assert(CHUNK % GL == 0 && EGNN_WAVE % GL == 0, "a chunk is a whole number of group steps");
enum { SOFTMAX = 0, LOG_SOFTMAX = 1 };
enum { STATS = 0, DOT = 1, SUM = 2 };        // what the walk folds: (max, sum of exp) of a | sum of a * b | sum of a

// rows that no key names: 0 in every statistic (one thread per row)
__global__ __launch_bounds__(THREADS) void ssm_absent_kernel(float* __restrict__ row_a, float* __restrict__ row_b, int64_t n_rows,
                                                             const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C) {
  const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (row >= n_rows || row_has_run(sorted, S, shift, row)) return;
  for (int64_t c = 0; c < C; ++c) {
    row_a[row * C + c] = 0.f;
    if (row_b != nullptr) row_b[row * C + c] = 0.f;
  }
}

// one 16-lane group folds the chunk that starts at sorted position j0 (sub: the lane's place in its group)
template <int W, int MODE>
__device__ __forceinline__ void walk_chunk(int64_t j0, bool head, int sub, float* __restrict__ row_a, float* __restrict__ row_b,
                                           const uint64_t* __restrict__ sorted, int64_t S, int shift, const float* __restrict__ xa,
                                           int64_t lda, const float* __restrict__ xb, int64_t ldb, int64_t C, float* __restrict__ part_a,
                                           float* __restrict__ part_b, int64_t ldp) {
  const uint64_t r = sorted[j0] >> shift;
  const bool long_run = chunk_is_long(sorted, S, shift, j0, head, r);
  if (long_run && part_a == nullptr) return;                           // (the entry points refuse this: S > CHUNK without a workspace)
  const int64_t limit = chunk_limit(j0, S);
  int64_t p[STEPS];
  bool ok[STEPS];
#pragma unroll
  for (int u = 0; u < STEPS; ++u) {
    const int64_t q = j0 + sub + GL * u;
    const uint64_t k = q < limit ? sorted[q] : NO_KEY;
    ok[u] = key_usable(k, r, shift, S);
    p[u] = (int64_t)key_pos(k, shift);
  }
  float* out_a = long_run ? part_a + part_slot(j0, head) * ldp : row_a + (int64_t)r * C;
  float* out_b = nullptr;
  if (MODE == STATS) out_b = long_run ? part_b + part_slot(j0, head) * ldp : row_b + (int64_t)r * C;
  for (int64_t c = 0; c < C; c += W) {
    float x[STEPS][W];
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
#pragma unroll
      for (int i = 0; i < W; ++i) x[u][i] = 0.f;
      if (ok[u]) load_w<W>(xa + p[u] * lda + c, x[u]);
    }
    if (MODE == DOT) {
#pragma unroll
      for (int u = 0; u < STEPS; ++u) {
        float b[W] = {};
        if (ok[u]) load_w<W>(xb + p[u] * ldb + c, b);
#pragma unroll
        for (int i = 0; i < W; ++i) x[u][i] = x[u][i] * b[i];
      }
    }
    float first[W], second[W];
    if (MODE == STATS) {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        float m = -INFINITY;
#pragma unroll
        for (int u = 0; u < STEPS; ++u)
          if (ok[u]) m = fmaxf(m, x[u][i]);
        m = egnn_reduce::group_max<GL>(m);
        float z = 0.f;
#pragma unroll
        for (int u = 0; u < STEPS; ++u)
          if (ok[u]) z += expf(x[u][i] - m);
        z = egnn_group_sum<GL>(z);
        // (a chunk without a usable position keeps m = -inf in the workspace, where the merge gives it weight 0; as a row's result it is 0)
        first[i] = (!long_run && m == -INFINITY) ? 0.f : m;
        second[i] = z;
      }
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < STEPS; ++u)
          if (ok[u]) s += x[u][i];
        first[i] = egnn_group_sum<GL>(s);
      }
    }
    if (sub == 0) {
      store_w<W>(out_a + c, first);
      if (MODE == STATS) store_w<W>(out_b + c, second);
    }
  }
}

// pass 1: one wave per window of 64 sorted positions; its four lane groups take the window's chunk starts, four at a time
template <int W, int MODE>
__global__ __launch_bounds__(THREADS) void ssm_walk_kernel(float* __restrict__ row_a, float* __restrict__ row_b, int64_t n_rows,
                                                           const uint64_t* __restrict__ sorted, int64_t S, int shift,
                                                           const float* __restrict__ xa, int64_t lda, const float* __restrict__ xb,
                                                           int64_t ldb, int64_t C, float* __restrict__ part_a, float* __restrict__ part_b,
                                                           int64_t ldp) {
  const int lane = egnn_lane();
  const int64_t base = ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * EGNN_WAVE;
  int flags = 0;                                                       // 1: starts a chunk, 2: and is its run's head
  chunk_start(sorted, S, shift, n_rows, base + lane, [&flags](bool head, uint64_t) { flags = head ? 3 : 1; });
  unsigned long long starts = __ballot(flags & 1);
  const unsigned long long heads = __ballot(flags & 2);
  const int grp = lane / GL, sub = lane % GL;
  while (starts != 0) {
    int mine = -1;
#pragma unroll
    for (int u = 0; u < EGNN_WAVE / GL; ++u) {
      if (starts != 0) {
        if (u == grp) mine = __ffsll((long long)starts) - 1;
        starts &= starts - 1;
      }
    }
    if (mine >= 0)
      walk_chunk<W, MODE>(base + mine, ((heads >> mine) & 1) != 0, sub, row_a, row_b, sorted, S, shift, xa, lda, xb, ldb, C, part_a, part_b, ldp);
  }
}

// pass 2: one wave per window of CHUNK sorted positions; the (at most one) head of a run longer than CHUNK in the window merges the
// run's partial results in ascending chunk order (one lane per column: a handful of columns, at most ~100 chunks for the largest hub)
template <int MODE>
__global__ __launch_bounds__(THREADS) void ssm_parts_kernel(float* __restrict__ row_a, float* __restrict__ row_b, int64_t n_rows,
                                                            const uint64_t* __restrict__ sorted, int64_t S, int shift, int64_t C,
                                                            const float* __restrict__ part_a, const float* __restrict__ part_b,
                                                            int64_t ldp) {
  const int lane = egnn_lane();
  const int64_t found = long_run_head(sorted, S, shift, n_rows, ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * CHUNK, lane, LG_WAVE);
  if (found < 0) return;
  uint64_t r;
  const int64_t chunks = run_chunks(sorted, S, shift, found, r);
  const int64_t s0 = part_slot(found, true);
  for (int64_t c = lane; c < C; c += EGNN_WAVE) {
    if (MODE == STATS) {
      float M = part_a[s0 * ldp + c];
      for (int64_t k = 1; k < chunks; ++k) M = fmaxf(M, part_a[part_slot(found + k * CHUNK, false) * ldp + c]);
      float Z = 0.f;
      for (int64_t k = 0; k < chunks; ++k) {
        const int64_t s = k == 0 ? s0 : part_slot(found + k * CHUNK, false);
        const float m = part_a[s * ldp + c];
        const float w = m == -INFINITY ? 0.f : expf(m - M);
        const float t = part_b[s * ldp + c] * w;
        Z = k == 0 ? t : Z + t;
      }
      row_a[(int64_t)r * C + c] = M == -INFINITY ? 0.f : M;
      row_b[(int64_t)r * C + c] = Z;
    } else {
      float T = part_a[s0 * ldp + c];
      for (int64_t k = 1; k < chunks; ++k) T += part_a[part_slot(found + k * CHUNK, false) * ldp + c];
      row_a[(int64_t)r * C + c] = T;
    }
  }
}

// element t of the [S, C / W] grid of column vectors -> (position, first column)
template <int W>
__device__ __forceinline__ bool gather_place(int64_t S, int64_t C, int64_t& p, int64_t& c) {
  const int64_t cv = C / W;
  const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= S * cv) return false;
  if (cv == 1) p = t;
  else if (S * cv <= 0xffffffffLL) p = (int64_t)((uint32_t)t / (uint32_t)cv);
  else p = t / cv;
  c = (t - p * cv) * W;
  return true;
}

template <int W, int FORM>
__global__ __launch_bounds__(THREADS) void ssm_fwd_gather_kernel(float* __restrict__ out, int64_t ldo, const float* __restrict__ src,
                                                                 int64_t lds_, const int64_t* __restrict__ rows, int64_t S, int64_t n_rows,
                                                                 int64_t C, const float* __restrict__ row_max,
                                                                 const float* __restrict__ row_den, float eps) {
  int64_t p, c;
  if (!gather_place<W>(S, C, p, c)) return;
  const int64_t r = rows[p];
  float v[W] = {};
  if (r >= 0 && r < n_rows) {
    float x[W], m[W], z[W];
    load_w<W>(src + p * lds_ + c, x);
    load_w<W>(row_max + r * C + c, m);
    load_w<W>(row_den + r * C + c, z);
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = FORM == SOFTMAX ? expf(x[i] - m[i]) / (z[i] + eps) : (x[i] - m[i]) - logf(z[i] + eps);
  }
  store_w<W>(out + p * ldo + c, v);
}

template <int W, int FORM>
__global__ __launch_bounds__(THREADS) void ssm_bwd_gather_kernel(float* __restrict__ dsrc, int64_t ldd, const float* __restrict__ out,
                                                                 int64_t ldo, const float* __restrict__ g, int64_t ldg,
                                                                 const int64_t* __restrict__ rows, int64_t S, int64_t n_rows, int64_t C,
                                                                 const float* __restrict__ row_dot) {
  int64_t p, c;
  if (!gather_place<W>(S, C, p, c)) return;
  const int64_t r = rows[p];
  float v[W] = {};
  if (r >= 0 && r < n_rows) {
    float y[W], gy[W], d[W];
    load_w<W>(out + p * ldo + c, y);
    load_w<W>(g + p * ldg + c, gy);
    load_w<W>(row_dot + r * C + c, d);
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = FORM == SOFTMAX ? y[i] * (gy[i] - d[i]) : gy[i] - expf(y[i]) * d[i];
  }
  store_w<W>(dsrc + p * ldd + c, v);
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// absent rows, pass 1 and (S > CHUNK) pass 2 of one walk
template <int W, int MODE>
void launch_walk(float* row_a, float* row_b, int64_t n_rows, const uint64_t* sorted, int64_t S, int shift, const float* xa, int64_t lda,
                 const float* xb, int64_t ldb, int64_t C, void* ws, hipStream_t st) {
  const int64_t ldp = part_pitch(C);
  float* part_a = S > CHUNK ? (float*)ws : nullptr;
  float* part_b = S > CHUNK && MODE == STATS ? part_a + part_slots(S) * ldp : nullptr;
  hipLaunchKernelGGL(ssm_absent_kernel, dim3((unsigned)blocks_for(n_rows, LG_ONE)), dim3(THREADS), 0, st, row_a, row_b, n_rows, sorted, S, shift,
                     C);
  if (S == 0) return;
  hipLaunchKernelGGL((ssm_walk_kernel<W, MODE>), dim3((unsigned)blocks_for(S, LG_ONE)), dim3(THREADS), 0, st, row_a, row_b, n_rows, sorted, S,
                     shift, xa, lda, xb, ldb, C, part_a, part_b, ldp);
  if (S > CHUNK)
    hipLaunchKernelGGL((ssm_parts_kernel<MODE>), dim3((unsigned)blocks_for(part_slots(S) / 2, LG_WAVE)), dim3(THREADS), 0, st, row_a, row_b,
                       n_rows, sorted, S, shift, C, (const float*)part_a, (const float*)part_b, ldp);
}

// launch(W, FORM), both integral constants: a launch list names its arguments once for 16-byte / scalar x softmax / log-softmax
template <class L>
void dispatch_w_form(bool vec4, int form, L&& launch) {
  dispatch_w(vec4, [&](auto w) {
    if (form == SOFTMAX) launch(w, std::integral_constant<int, SOFTMAX>{});
    else launch(w, std::integral_constant<int, LOG_SOFTMAX>{});
  });
}

// the checks both directions share, in the order the header documents; OK_EMPTY: S == 0 and nothing more to check
enum { OK_EMPTY = 1 };
int check_common(int64_t S, int64_t n_rows, int64_t C, int form, int shift, const uint64_t* keys_sorted, const int64_t* rows, void* ws,
                 size_t ws_bytes) {
  EGNN_CHECK_ARG(sizes_ok(S, n_rows) && C >= 1 && (form == SOFTMAX || form == LOG_SOFTMAX));
  if (S == 0) return OK_EMPTY;
  EGNN_CHECK_ARG(keys_sorted && rows && n_rows > 0 && shift == bits_for((uint64_t)S - 1));
  const size_t need = egnn_scatter_softmax_ws_bytes(S, C);
  if (need > 0 && (!ws || ws_bytes < need)) return EGNN_EWORKSPACE;
  if ((need > 0 && !egnn_aligned16(ws)) || !aligned(keys_sorted, 8) || !aligned(rows, 8)) return EGNN_EALIGN;
  return EGNN_OK;
}

}  // namespace

extern "C" size_t egnn_scatter_softmax_ws_bytes(int64_t S, int64_t C) {
  if (S <= CHUNK || S >= 0x7fffffffLL || C <= 0) return 0;
  return (size_t)part_slots(S) * (size_t)part_pitch(C) * 2 * sizeof(float);   // the chunk maxima, then the chunk sums
}

extern "C" int egnn_scatter_softmax_fwd_f32(float* out, int64_t ld_out, float* row_max, float* row_den, int64_t n_rows,
                                            const uint64_t* keys_sorted, int64_t S, int shift, const int64_t* rows, const float* src,
                                            int64_t ld_src, int64_t C, float eps, int form, void* ws, size_t ws_bytes, void* stream) {
  const int rc = check_common(S, n_rows, C, form, shift, keys_sorted, rows, ws, ws_bytes);
  if (rc < 0) return rc;
  EGNN_CHECK_ARG(ld_out >= C && ld_src >= C);
  if (!aligned(row_max, 4) || !aligned(row_den, 4)) return EGNN_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (rc == OK_EMPTY) {
    if (row_max == nullptr || row_den == nullptr || n_rows == 0) return EGNN_OK;
    launch_walk<1, STATS>(row_max, row_den, n_rows, nullptr, 0, 0, nullptr, 0, nullptr, 0, C, nullptr, st);
    return egnn_launch_status();
  }
  EGNN_CHECK_ARG(out && row_max && row_den && src);
  if (!aligned(out, 4) || !aligned(src, 4)) return EGNN_EALIGN;
  const bool vec4 = C % 4 == 0 && ld_out % 4 == 0 && ld_src % 4 == 0 && egnn_aligned16(out) && egnn_aligned16(src) &&
                    egnn_aligned16(row_max) && egnn_aligned16(row_den);
  const int64_t blocks = blocks_for(S * (C / (vec4 ? 4 : 1)), LG_ONE);
  EGNN_CHECK_ARG(blocks < 0x7fffffffLL);
  dispatch_w_form(vec4, form, [&](auto w, auto f) {
    constexpr int W = decltype(w)::value, FORM = decltype(f)::value;
    launch_walk<W, STATS>(row_max, row_den, n_rows, keys_sorted, S, shift, src, ld_src, nullptr, 0, C, ws, st);
    hipLaunchKernelGGL((ssm_fwd_gather_kernel<W, FORM>), dim3((unsigned)blocks), dim3(THREADS), 0, st, out, ld_out, src, ld_src, rows, S, n_rows, C,
                       (const float*)row_max, (const float*)row_den, eps);
  });
  return egnn_launch_status();
}

extern "C" int egnn_scatter_softmax_bwd_f32(float* dsrc, int64_t ld_dsrc, float* row_dot, int64_t n_rows, const uint64_t* keys_sorted,
                                            int64_t S, int shift, const int64_t* rows, const float* out, int64_t ld_out, const float* g,
                                            int64_t ld_g, int64_t C, int form, void* ws, size_t ws_bytes, void* stream) {
  const int rc = check_common(S, n_rows, C, form, shift, keys_sorted, rows, ws, ws_bytes);
  if (rc < 0) return rc;
  EGNN_CHECK_ARG(ld_dsrc >= C && ld_out >= C && ld_g >= C);
  if (!aligned(row_dot, 4)) return EGNN_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (rc == OK_EMPTY) {
    if (row_dot == nullptr || n_rows == 0) return EGNN_OK;
    launch_walk<1, SUM>(row_dot, nullptr, n_rows, nullptr, 0, 0, nullptr, 0, nullptr, 0, C, nullptr, st);
    return egnn_launch_status();
  }
  EGNN_CHECK_ARG(dsrc && row_dot && out && g);
  if (!aligned(dsrc, 4) || !aligned(out, 4) || !aligned(g, 4)) return EGNN_EALIGN;
  const bool vec4 = C % 4 == 0 && ld_dsrc % 4 == 0 && ld_out % 4 == 0 && ld_g % 4 == 0 && egnn_aligned16(dsrc) && egnn_aligned16(out) &&
                    egnn_aligned16(g) && egnn_aligned16(row_dot);
  const int64_t blocks = blocks_for(S * (C / (vec4 ? 4 : 1)), LG_ONE);
  EGNN_CHECK_ARG(blocks < 0x7fffffffLL);
  dispatch_w_form(vec4, form, [&](auto w, auto f) {
    constexpr int W = decltype(w)::value, FORM = decltype(f)::value;
    if (FORM == SOFTMAX) launch_walk<W, DOT>(row_dot, nullptr, n_rows, keys_sorted, S, shift, out, ld_out, g, ld_g, C, ws, st);
    else launch_walk<W, SUM>(row_dot, nullptr, n_rows, keys_sorted, S, shift, g, ld_g, nullptr, 0, C, ws, st);
    hipLaunchKernelGGL((ssm_bwd_gather_kernel<W, FORM>), dim3((unsigned)blocks), dim3(THREADS), 0, st, dsrc, ld_dsrc, out, ld_out, g, ld_g, rows, S,
                       n_rows, C, (const float*)row_dot);
  });
  return egnn_launch_status();
}
