// Row-lazy Adam for the MAG embedding tables (mag_pyg/gnn.py:100-108 emb_dict, :424 torch.optim.Adam) and the one-launch
// group_input gather (:117-127).  A GraphSAINT batch touches ~55 k of the 1.2 M table rows; dense Adam nevertheless moves every row every
// step, because a row whose gradient is zero still decays m and v and goes on moving p while m != 0.  Here every table row records the
// last step it is current for (`last`, -1 = never had a gradient: m = v = 0, dense Adam leaves such a row where it is).  Before a row is
// read or stepped, the zero-gradient steps it missed are replayed in registers (catch-up); the step itself then runs over the batch rows
// only.  The replay IS the step with g = 0 (one device function, adam_elem): "lazy" and "touched every step with a zero gradient" give
// the same bits.  The per-step scalars lr_tau / (1 - beta1^tau) and sqrt(1 - beta2^tau) are formed on the host in double and travel in
// two rings of EGNN_ADAM_MAX_LAG entries inside the descriptor (staged to LDS once per workgroup): the device never forms a power.
//
// Work layout, shared by all kernels: a row is served by G = min(64, pow2ceil(D / 4)) neighbouring lanes, 16 bytes (float4) per lane and
// column chunk, 64 / G rows per wave (two at D = 128) and 256 / G rows per workgroup.  Sub-lane 0 of a row reads / claims `last[r]` and
// hands the verdict to its G - 1 neighbours through a width-G shuffle, so the replay trip count is uniform per row.  A row is claimed
// with a compare-and-swap on `last[r]`, so a table row named twice in one batch is served once (catch-up) or counted (step) and never
// read while another group writes it.  All stores are ordinary vector stores; no float atomics: results are bit-stable.
//
// The summing step (egnn_adam_rows_step_sum_f32) takes a list that may name a table row several times (several batches of one optimiser
// step, or the batches of several ranks).  The selected entries get 64-bit keys (row << shift) | entry, the keys are radix-sorted over
// the bits they use, and the lane group at the first key of a row's run walks the run forward: the row's gradient rows are added in
// registers in ascending entry order, scaled once, and the row takes ONE step through the same device functions.  Only the head's
// group touches the row, so runs that cross a workgroup boundary need no hand-over.
#include "rows_runs.h"

namespace {

using egnn_rows::NO_KEY;               // an entry of another type or outside the table: sorts behind every row
using egnn_rows::THREADS;
using egnn_rows::align_up;
using egnn_rows::bits_for;
using egnn_rows::blocks_for;
using egnn_rows::is_run_head;
using egnn_rows::kAlign;
using egnn_rows::make_key;
using egnn_rows::sort_keys;
using egnn_rows::sort_keys_temp;

constexpr int MAX_TABLES = 8;
constexpr int RING = EGNN_ADAM_MAX_LAG;
static_assert((RING & (RING - 1)) == 0 && 2 * RING <= THREADS, "the ring is indexed with tau & (RING - 1) and staged by one workgroup pass");

static int lanes_lg(int64_t D) { return egnn_rows::lanes_lg(D / 4); }

// ONE Adam step of one element, in torch.optim.Adam's single-tensor order (no fused multiply-add: the library is built with
// -ffp-contract=off).  g = 0 is the replayed step of a row outside the batch.
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, float b1, float b2, float omb1, float omb2, float eps,
                                          float step_size, float bc2_sqrt) {
  m = b1 * m + omb1 * g;
  v = b2 * v + omb2 * g * g;
  p -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
}

// the four gradient columns c .. c + 3 of one gradient row (nullptr: zero)
struct RowGrad {
  const float* __restrict__ g_row;
  __device__ __forceinline__ float4 operator()(int64_t c) const {
    return g_row ? *reinterpret_cast<const float4*>(g_row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
};

// steps tau = from .. to of table row r with the gradient columns grad(c) over the columns of sub-lane `sub`
template <class GradAt>
__device__ __forceinline__ void row_steps(const egnn_adam_rows_t& a, const float* s_ss, const float* s_bc, int64_t r, int sub, int G,
                                          int from, int to, GradAt grad) {
  for (int64_t c = (int64_t)sub * 4; c < a.D; c += (int64_t)G * 4) {
    const int64_t o = r * a.ld + c;
    float4 p4 = *reinterpret_cast<const float4*>(a.p + o);
    float4 m4 = *reinterpret_cast<const float4*>(a.m + o);
    float4 v4 = *reinterpret_cast<const float4*>(a.v + o);
    const float4 g4 = grad(c);
    float p[4] = {p4.x, p4.y, p4.z, p4.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
    const float g[4] = {g4.x, g4.y, g4.z, g4.w};
    for (int tau = from; tau <= to; ++tau) {
      const float ss = s_ss[tau & (RING - 1)], bc = s_bc[tau & (RING - 1)];
#pragma unroll
      for (int k = 0; k < 4; ++k) adam_elem(p[k], m[k], v[k], g[k], a.beta1, a.beta2, a.one_minus_beta1, a.one_minus_beta2, a.eps, ss, bc);
    }
    *reinterpret_cast<float4*>(a.p + o) = make_float4(p[0], p[1], p[2], p[3]);
    *reinterpret_cast<float4*>(a.m + o) = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(a.v + o) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__device__ __forceinline__ void stage_ring(const egnn_adam_rows_t& a, float* s_ss, float* s_bc) {
  const int t = threadIdx.x;
  if (t < RING) s_ss[t] = a.step_size[t];
  else if (t < 2 * RING) s_bc[t - RING] = a.bc2_sqrt[t - RING];
  __syncthreads();
}

// batch row i of this thread's group -> table row r; false: nothing to do (past the end, another node type, id out of range)
__device__ __forceinline__ bool pick_row(const egnn_adam_rows_t& a, int type_id, const int64_t* __restrict__ node_type,
                                         const int64_t* __restrict__ local_idx, int64_t n, int lg, int64_t& i, int64_t& r, int& sub) {
  i = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  sub = threadIdx.x & ((1 << lg) - 1);
  if (i >= n) return false;
  if (node_type && node_type[i] != (int64_t)type_id) return false;
  r = local_idx ? local_idx[i] : i;
  return r >= 0 && r < a.n_rows;
}

// catch-up (and, with node_type == local_idx == nullptr and n == n_rows, the flush): last[r] + 1 .. step with a zero gradient
__global__ __launch_bounds__(THREADS) void adam_rows_catchup_kernel(egnn_adam_rows_t a, int type_id, const int64_t* __restrict__ node_type,
                                                                    const int64_t* __restrict__ local_idx, int64_t n, int lg) {
  __shared__ float s_ss[RING], s_bc[RING];
  stage_ring(a, s_ss, s_bc);
  int64_t i, r;
  int sub;
  if (!pick_row(a, type_id, node_type, local_idx, n, lg, i, r, sub)) return;
  int from = a.step + 1;                       // empty replay unless sub-lane 0 claims the row
  if (sub == 0) {
    const int l = a.last[r];
    if (l != -1 && l < a.step && atomicCAS(a.last + r, l, a.step) == l) from = l + 1;
  }
  from = __shfl(from, 0, 1 << lg);
  if (from <= a.step) row_steps(a, s_ss, s_bc, r, sub, 1 << lg, from, a.step, RowGrad{nullptr});
}

// the step: claim step - 1 -> step (or -1 -> step for a row's first gradient); a loser is counted in dup_count and writes nothing
__global__ __launch_bounds__(THREADS) void adam_rows_step_kernel(egnn_adam_rows_t a, int type_id, const int64_t* __restrict__ node_type,
                                                                 const int64_t* __restrict__ local_idx, int64_t n,
                                                                 const float* __restrict__ g, int64_t ldg, int lg) {
  __shared__ float s_ss[RING], s_bc[RING];
  stage_ring(a, s_ss, s_bc);
  int64_t i, r = -1;
  int sub;
  const bool mine = pick_row(a, type_id, node_type, local_idx, n, lg, i, r, sub);
  if (!mine) {
    // a selected batch row whose table row does not exist is an update that was not applied: counted, like a duplicate
    if (i < n && sub == 0 && (!node_type || node_type[i] == (int64_t)type_id)) atomicAdd(a.dup_count, 1);
    return;
  }
  int win = 0;
  if (sub == 0) {
    int old = atomicCAS(a.last + r, a.step - 1, a.step);
    win = old == a.step - 1;
    if (!win && old == -1) win = atomicCAS(a.last + r, -1, a.step) == -1;
    if (!win) atomicAdd(a.dup_count, 1);
  }
  win = __shfl(win, 0, 1 << lg);
  if (win) row_steps(a, s_ss, s_bc, r, sub, 1 << lg, a.step, a.step, RowGrad{g + i * ldg});
}

// ---- the summing step --------------------------------------------------------------------------------------------------------------
// keys[i] = (local_idx[i] << shift) | i for a selected entry inside the table; a selected entry outside it is counted here (keys ==
// nullptr: an empty table, count only)
__global__ __launch_bounds__(THREADS) void adam_rows_keys_kernel(int64_t n_rows, int32_t* __restrict__ dup_count, int type_id,
                                                                 const int64_t* __restrict__ node_type,
                                                                 const int64_t* __restrict__ local_idx, int64_t n, int shift,
                                                                 uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  uint64_t key = NO_KEY;
  if (!node_type || node_type[i] == (int64_t)type_id) {
    const int64_t r = local_idx[i];
    if (r >= 0 && r < n_rows) key = make_key(r, shift, i);
    else atomicAdd(dup_count, 1);
  }
  if (keys) keys[i] = key;
}

// scale * (((g[i1] + g[i2]) + ...) + g[ik]) over the run of sorted keys that starts at j (all of table row r, ascending entry)
struct RunGrad {
  const uint64_t* __restrict__ sorted;
  int64_t j, n;
  uint64_t r;
  int shift;
  const float* __restrict__ g;
  int64_t ldg;
  float scale;
  __device__ __forceinline__ float4 operator()(int64_t c) const {
    const uint64_t entry_mask = (uint64_t(1) << shift) - 1;
    float4 s = *reinterpret_cast<const float4*>(g + (int64_t)(sorted[j] & entry_mask) * ldg + c);
    for (int64_t q = j + 1; q < n; ++q) {
      const uint64_t k = sorted[q];
      if ((k >> shift) != r) break;
      const float4 x = *reinterpret_cast<const float4*>(g + (int64_t)(k & entry_mask) * ldg + c);
      s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
    }
    return make_float4(scale * s.x, scale * s.y, scale * s.z, scale * s.w);
  }
};

// one lane group per sorted key; the group at the head of a row's run claims the row like adam_rows_step_kernel and steps it once
__global__ __launch_bounds__(THREADS) void adam_rows_step_sum_kernel(egnn_adam_rows_t a, const uint64_t* __restrict__ sorted, int64_t n,
                                                                     int shift, const float* __restrict__ g, int64_t ldg, float scale,
                                                                     int lg) {
  __shared__ float s_ss[RING], s_bc[RING];
  stage_ring(a, s_ss, s_bc);
  const int64_t j = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
  if (j >= n) return;
  const uint64_t key = sorted[j];
  if (key == NO_KEY) return;
  const uint64_t r = key >> shift;
  if (!is_run_head(sorted, shift, j, r)) return;
  int win = 0;
  if (sub == 0) {
    int old = atomicCAS(a.last + r, a.step - 1, a.step);
    win = old == a.step - 1;
    if (!win && old == -1) win = atomicCAS(a.last + r, -1, a.step) == -1;
    if (!win) atomicAdd(a.dup_count, 1);
  }
  win = __shfl(win, 0, 1 << lg);
  if (win) row_steps(a, s_ss, s_bc, (int64_t)r, sub, 1 << lg, a.step, a.step, RunGrad{sorted, j, n, r, shift, g, ldg, scale});
}

struct Tables {
  const float* ptr[MAX_TABLES];
  int64_t rows[MAX_TABLES];
};

// h[i] = tables[node_type[i]][local_idx[i]]; a type without a table writes zeros, a type or an index out of range writes zeros and is
// counted in *oob
__global__ __launch_bounds__(THREADS) void group_input_kernel(Tables t, int n_types, const int64_t* __restrict__ node_type,
                                                              const int64_t* __restrict__ local_idx, int64_t n, int64_t D,
                                                              float* __restrict__ h, int64_t ldh, int32_t* __restrict__ oob, int lg) {
  const int64_t i = (int64_t)blockIdx.x * (THREADS >> lg) + (threadIdx.x >> lg);
  const int sub = threadIdx.x & ((1 << lg) - 1);
  if (i >= n) return;
  const int64_t ty = node_type[i], li = local_idx[i];
  const float* src = nullptr;
  int64_t rows = 0;
#pragma unroll
  for (int k = 0; k < MAX_TABLES; ++k)
    if (ty == k) { src = t.ptr[k]; rows = t.rows[k]; }
  bool bad = ty < 0 || ty >= n_types;
  if (bad) src = nullptr;
  if (src && (li < 0 || li >= rows)) { bad = true; src = nullptr; }
  if (bad && sub == 0) atomicAdd(oob, 1);
  for (int64_t c = (int64_t)sub * 4; c < D; c += (int64_t)4 << lg) {
    const float4 v = src ? *reinterpret_cast<const float4*>(src + li * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(h + i * ldh + c) = v;
  }
}

static int check_rows(const egnn_adam_rows_t* a, int min_step) {
  EGNN_CHECK_ARG(a && a->p && a->m && a->v && a->last && a->dup_count);
  EGNN_CHECK_ARG(a->n_rows >= 0 && a->D > 0 && a->D % 4 == 0 && a->ld >= a->D);
  EGNN_CHECK_ARG(a->step >= min_step && a->flushed >= 0 && a->flushed <= a->step);
  EGNN_CHECK_ARG(a->step - a->flushed <= EGNN_ADAM_MAX_LAG);      // older steps have left the ring
  if (a->ld % 4 != 0 || !egnn_aligned16(a->p) || !egnn_aligned16(a->m) || !egnn_aligned16(a->v)) return EGNN_EALIGN;
  return EGNN_OK;
}

}  // namespace

extern "C" int egnn_group_input_f32(const float* const* tables, const int64_t* table_rows, int n_types, const int64_t* node_type,
                                    const int64_t* local_idx, int64_t n, int64_t D, float* h, int64_t ldh, int32_t* oob, void* stream) {
  EGNN_CHECK_ARG(tables && table_rows && n_types >= 1 && n_types <= MAX_TABLES);
  EGNN_CHECK_ARG(node_type && local_idx && h && oob && n >= 0 && D > 0 && D % 4 == 0 && ldh >= D);
  Tables t{};
  for (int k = 0; k < n_types; ++k) {
    EGNN_CHECK_ARG(table_rows[k] >= 0);
    if (!egnn_aligned16(tables[k])) return EGNN_EALIGN;
    t.ptr[k] = tables[k];
    t.rows[k] = tables[k] ? table_rows[k] : 0;
  }
  if (ldh % 4 != 0 || !egnn_aligned16(h)) return EGNN_EALIGN;
  if (n == 0) return EGNN_OK;
  const int lg = lanes_lg(D);
  hipLaunchKernelGGL(group_input_kernel, dim3((unsigned)blocks_for(n, lg)), dim3(THREADS), 0, (hipStream_t)stream, t, n_types, node_type,
                     local_idx, n, D, h, ldh, oob, lg);
  return egnn_launch_status();
}

extern "C" int egnn_adam_rows_catchup_f32(const egnn_adam_rows_t* a, int type_id, const int64_t* node_type, const int64_t* local_idx,
                                          int64_t n, void* stream) {
  const int rc = check_rows(a, 0);
  if (rc != EGNN_OK) return rc;
  EGNN_CHECK_ARG(local_idx && n >= 0);
  if (n == 0 || a->n_rows == 0) return EGNN_OK;
  const int lg = lanes_lg(a->D);
  hipLaunchKernelGGL(adam_rows_catchup_kernel, dim3((unsigned)blocks_for(n, lg)), dim3(THREADS), 0, (hipStream_t)stream, *a, type_id,
                     node_type, local_idx, n, lg);
  return egnn_launch_status();
}

extern "C" int egnn_adam_rows_flush_f32(const egnn_adam_rows_t* a, void* stream) {
  const int rc = check_rows(a, 0);
  if (rc != EGNN_OK) return rc;
  if (a->n_rows == 0) return EGNN_OK;
  const int lg = lanes_lg(a->D);
  hipLaunchKernelGGL(adam_rows_catchup_kernel, dim3((unsigned)blocks_for(a->n_rows, lg)), dim3(THREADS), 0, (hipStream_t)stream, *a, 0,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, a->n_rows, lg);
  return egnn_launch_status();
}

extern "C" int egnn_adam_rows_step_f32(const egnn_adam_rows_t* a, int type_id, const int64_t* node_type, const int64_t* local_idx,
                                       int64_t n, const float* g, int64_t ldg, void* stream) {
  const int rc = check_rows(a, 1);
  if (rc != EGNN_OK) return rc;
  EGNN_CHECK_ARG(local_idx && g && n >= 0 && ldg >= a->D);
  if (ldg % 4 != 0 || !egnn_aligned16(g)) return EGNN_EALIGN;
  if (n == 0) return EGNN_OK;
  const int lg = lanes_lg(a->D);
  hipLaunchKernelGGL(adam_rows_step_kernel, dim3((unsigned)blocks_for(n, lg)), dim3(THREADS), 0, (hipStream_t)stream, *a, type_id, node_type,
                     local_idx, n, g, ldg, lg);
  return egnn_launch_status();
}

extern "C" size_t egnn_adam_rows_step_sum_ws_bytes(int64_t n, int64_t n_rows) {
  if (n <= 0 || n >= 0x7fffffffLL || n_rows <= 0 || n_rows >= 0x7fffffffLL) return kAlign;
  const int end_bit = bits_for((uint64_t)n - 1) + bits_for((uint64_t)n_rows);
  size_t temp = 0;
  if (!sort_keys_temp(n, end_bit, &temp)) temp = 0;      // no device to ask: the key arrays alone (the step itself then refuses)
  return 2 * align_up((size_t)n * 8) + align_up(temp) + kAlign;
}

extern "C" int egnn_adam_rows_step_sum_f32(const egnn_adam_rows_t* a, int type_id, const int64_t* node_type, const int64_t* local_idx,
                                           int64_t n, const float* g, int64_t ldg, float scale, void* ws, size_t ws_bytes,
                                           void* stream) {
  const int rc = check_rows(a, 1);
  if (rc != EGNN_OK) return rc;
  EGNN_CHECK_ARG(local_idx && g && n >= 0 && ldg >= a->D);
  EGNN_CHECK_ARG(n < 0x7fffffffLL && a->n_rows < 0x7fffffffLL);     // hipCUB item counts are int; row and entry share one 64-bit key
  if (ldg % 4 != 0 || !egnn_aligned16(g)) return EGNN_EALIGN;
  if (n == 0) return EGNN_OK;
  if (!ws || ws_bytes < egnn_adam_rows_step_sum_ws_bytes(n, a->n_rows)) return EGNN_EWORKSPACE;
  if (!egnn_aligned16(ws)) return EGNN_EALIGN;
  size_t temp = 0;
  if (a->n_rows > 0 && !sort_keys_temp(n, bits_for((uint64_t)n - 1) + bits_for((uint64_t)a->n_rows), &temp)) return EGNN_ELAUNCH;
  if (a->n_rows == 0) {                                              // every selected entry is outside the table: counted, nothing sorted
    hipLaunchKernelGGL(adam_rows_keys_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       a->n_rows, a->dup_count, type_id, node_type, local_idx, n, 1, (uint64_t*)nullptr);
    return egnn_launch_status();
  }
  hipStream_t st = (hipStream_t)stream;
  const int shift = bits_for((uint64_t)n - 1), end_bit = shift + bits_for((uint64_t)a->n_rows);
  char* p = (char*)ws;
  uint64_t* keys = (uint64_t*)p;   p += align_up((size_t)n * 8);
  uint64_t* sorted = (uint64_t*)p; p += align_up((size_t)n * 8);
  size_t tb = ws_bytes - (size_t)(p - (char*)ws);
  hipLaunchKernelGGL(adam_rows_keys_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, a->n_rows, a->dup_count,
                     type_id, node_type, local_idx, n, shift, keys);
  if (!sort_keys(p, tb, keys, sorted, n, end_bit, st)) return EGNN_ELAUNCH;
  const int lg = lanes_lg(a->D);
  hipLaunchKernelGGL(adam_rows_step_sum_kernel, dim3((unsigned)blocks_for(n, lg)), dim3(THREADS), 0, st, *a, sorted, n, shift, g, ldg, scale,
                     lg);
  return egnn_launch_status();
}
