// GraphSAINT random-walk mini-batches formed on the device (/root/reference/mag_pyg/gnn.py:361-366: PyG's
// GraphSAINTRandomWalkSampler = torch_sparse::random_walk + SparseTensor.saint_subgraph, CPU C++ in DataLoader workers there):
//   egnn_saint_random_walk_i64     B walks of L steps over a CSR; every visited node is flagged
//   egnn_saint_select_i64          flag -> relabel (exclusive scan) and the ascending list of flagged nodes (= walks.unique())
//   egnn_saint_induced_count_i64   per listed parent row, the number of entries whose column is flagged (+ the scan of those counts)
//   egnn_saint_induced_fill_i64    the kept entries, relabelled, IN THE PARENT'S ORDER within each row (= saint_subgraph)
//   egnn_saint_gather_i64          node / edge attributes of the batch
// Integer work only, no atomics: flags are plain byte stores of the same value, the compaction inside a row is a wave ballot
// plus a popcount prefix, and a running offset is carried across the passes of a row, so the output order never depends on
// launch order.  The flag table is one byte per node (1.9 MB at MAG size: L2-resident under the random column lookups).
#include <hipcub/hipcub.hpp>

#include "bn_common.h"
#include "block_reduce.h"

namespace {

constexpr int kThreads = 256;                 // 4 waves per workgroup
constexpr int kWavesPerBlock = kThreads / EGNN_WAVE;
constexpr int64_t kWavePass = EGNN_WAVE;      // entries one wave compacts per pass
constexpr int64_t kBlockPass = kThreads;      // entries one workgroup compacts per pass
constexpr int64_t kLongRow = 512;             // rows with more entries take the workgroup-per-row kernels
constexpr size_t kAlign = 256;

unsigned grid_for(int64_t n, int64_t per_block) {
  const int64_t b = (n + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// One thread per walk (latency-bound pointer chasing; B ~ 20 000).  Injected draws: start / rand; own draws: counter hash of
// (seed + *seed_dev, b * (L + 1) + j), j = 0 the start (multiply-shift of the 32-bit hash), j = 1 .. L the steps (uniform01).
__global__ void saint_walk_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col, int64_t N, int64_t B, int64_t L,
                                  const int64_t* __restrict__ start, const float* __restrict__ rnd, unsigned long long seed,
                                  const unsigned long long* __restrict__ seed_dev, int64_t* __restrict__ walks,
                                  uint8_t* __restrict__ flag) {
  const int64_t b = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (b >= B) return;
  const unsigned long long key = seed + (seed_dev ? *seed_dev : 0ull);
  const unsigned long long c0 = (unsigned long long)b * (unsigned long long)(L + 1);
  int64_t cur;
  if (start) {
    cur = start[b];
    cur = cur < 0 ? 0 : (cur >= N ? N - 1 : cur);     // an id outside the graph must not become an address
  } else {
    cur = (int64_t)(((unsigned long long)egnn_bn::hash32(key, c0) * (unsigned long long)N) >> 32);
  }
  if (walks) walks[b * (L + 1)] = cur;
  flag[cur] = 1;
  for (int64_t s = 0; s < L; ++s) {
    const int64_t r0 = rowptr[cur], d = rowptr[cur + 1] - r0;
    if (d > 0) {
      const float u = rnd ? rnd[b * L + s] : egnn_bn::uniform01(key, c0 + 1 + (unsigned long long)s);
      int64_t k = (int64_t)(u * (float)d);             // fp32 product, as torch_sparse::random_walk forms it
      k = k > d - 1 ? d - 1 : (k < 0 ? 0 : k);
      cur = col[r0 + k];
    }
    if (walks) walks[b * (L + 1) + s + 1] = cur;
    flag[cur] = 1;
  }
}

struct FlagAt {   // flag[i] for i < n, 0 for the one extra item that turns the exclusive scan into a row pointer with its total
  const uint8_t* f; int64_t n;
  __host__ __device__ int64_t operator()(int64_t i) const { return i < n ? (int64_t)f[i] : 0; }
};
struct CountAt {
  const int64_t* c; int64_t n;
  __host__ __device__ int64_t operator()(int64_t i) const { return i < n ? c[i] : 0; }
};
template <class Op>
using ScanIn = hipcub::TransformInputIterator<int64_t, Op, hipcub::CountingInputIterator<int64_t>>;

template <class Op>
hipError_t exclusive_scan(void* ws, size_t& bytes, Op op, int64_t* out, int64_t items, hipStream_t st) {
  ScanIn<Op> in(hipcub::CountingInputIterator<int64_t>(0), op);
  return hipcub::DeviceScan::ExclusiveSum(ws, bytes, in, out, (int)items, st);
}

__global__ void saint_compact_kernel(const uint8_t* __restrict__ flag, const int64_t* __restrict__ relabel, int64_t N,
                                     int64_t* __restrict__ node_idx, int64_t cap) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
    if (flag[i]) {
      const int64_t p = relabel[i];
      if (p < cap) node_idx[p] = i;
    }
  }
}

// Output row r = g * n_map + i stands for parent row g * group_stride + row_map[i]; rows with i >= the device-side count are empty
struct RowView {
  const int64_t* rowptr; const int64_t* row_map; int64_t n_map; const int64_t* n_map_dev; int64_t group_stride;
};
__device__ __forceinline__ bool parent_range(const RowView& v, int64_t r, int64_t n_valid, int64_t& b, int64_t& e) {
  const int64_t g = r / v.n_map, i = r - g * v.n_map;
  if (i >= n_valid) { b = e = 0; return false; }
  const int64_t prow = g * v.group_stride + v.row_map[i];
  b = v.rowptr[prow];
  e = v.rowptr[prow + 1];
  return true;
}
__device__ __forceinline__ int64_t valid_rows(const RowView& v) {
  if (!v.n_map_dev) return v.n_map;
  const int64_t n = *v.n_map_dev;
  return n < v.n_map ? n : v.n_map;
}

// rows of at most kLongRow entries: one wave per output row
__global__ void __launch_bounds__(kThreads) induced_count_wave_kernel(RowView v, const int64_t* __restrict__ col, int64_t R,
                                                                     const uint8_t* __restrict__ flag, int64_t* __restrict__ counts) {
  const int lane = egnn_lane();
  const int64_t n_valid = valid_rows(v);
  const int64_t w0 = blockIdx.x * (int64_t)kWavesPerBlock + egnn_wave_id(), nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t r = w0; r < R; r += nw) {
    int64_t b, e;
    parent_range(v, r, n_valid, b, e);
    if (e - b > kLongRow) continue;                     // the workgroup kernel writes this row
    int cnt = 0;
    for (int64_t p = b + lane; p < e; p += kWavePass) cnt += flag[col[p]] ? 1 : 0;
    cnt = egnn_reduce::group_sum<EGNN_WAVE>(cnt);
    if (lane == 0) counts[r] = cnt;
  }
}

// rows of more than kLongRow entries: one workgroup per output row
__global__ void __launch_bounds__(kThreads) induced_count_block_kernel(RowView v, const int64_t* __restrict__ col, int64_t R,
                                                                      const uint8_t* __restrict__ flag, int64_t* __restrict__ counts) {
  __shared__ int wave_cnt[kWavesPerBlock];
  const int lane = egnn_lane(), w = egnn_wave_id();
  const int64_t n_valid = valid_rows(v);
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    int64_t b, e;
    parent_range(v, r, n_valid, b, e);
    if (e - b <= kLongRow) continue;                    // uniform over the workgroup
    int cnt = 0;
    for (int64_t p = b + threadIdx.x; p < e; p += kBlockPass) cnt += flag[col[p]] ? 1 : 0;
    cnt = egnn_reduce::group_sum<EGNN_WAVE>(cnt);
    if (lane == 0) wave_cnt[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t t = 0;
      for (int k = 0; k < kWavesPerBlock; ++k) t += wave_cnt[k];
      counts[r] = t;
    }
    __syncthreads();
  }
}

struct FillOut {
  const int64_t* val; const int64_t* relabel; const int64_t* out_ptr; int64_t out_cap;
  int64_t* out_row; int64_t* out_col; int64_t* out_val;
};
__device__ __forceinline__ void emit(const FillOut& o, int64_t pos, int64_t i, int64_t c, int64_t p) {
  if (pos >= o.out_cap) return;                         // the caller sized the outputs from the counts of the same flags
  if (o.out_row) o.out_row[pos] = i;
  o.out_col[pos] = o.relabel[c];
  if (o.out_val) o.out_val[pos] = o.val ? o.val[p] : p;
}

__global__ void __launch_bounds__(kThreads) induced_fill_wave_kernel(RowView v, const int64_t* __restrict__ col, int64_t R,
                                                                    const uint8_t* __restrict__ flag, FillOut o) {
  const int lane = egnn_lane();
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t n_valid = valid_rows(v);
  const int64_t w0 = blockIdx.x * (int64_t)kWavesPerBlock + egnn_wave_id(), nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t r = w0; r < R; r += nw) {
    int64_t b, e;
    if (!parent_range(v, r, n_valid, b, e) || e - b > kLongRow) continue;
    const int64_t i = r % v.n_map;
    int64_t off = o.out_ptr[r];                         // running offset, carried across the passes of this row
    for (int64_t base = b; base < e; base += kWavePass) {
      const int64_t p = base + lane;
      int64_t c = 0;
      bool keep = false;
      if (p < e) { c = col[p]; keep = flag[c] != 0; }
      const unsigned long long m = __ballot(keep);
      if (keep) emit(o, off + __popcll(m & below), i, c, p);
      off += __popcll(m);
    }
  }
}

__global__ void __launch_bounds__(kThreads) induced_fill_block_kernel(RowView v, const int64_t* __restrict__ col, int64_t R,
                                                                     const uint8_t* __restrict__ flag, FillOut o) {
  __shared__ int wave_cnt[kWavesPerBlock];
  const int lane = egnn_lane(), w = egnn_wave_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t n_valid = valid_rows(v);
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    int64_t b, e;
    if (!parent_range(v, r, n_valid, b, e) || e - b <= kLongRow) continue;   // uniform over the workgroup
    const int64_t i = r % v.n_map;
    int64_t off = o.out_ptr[r];                         // running offset, carried across the workgroup passes of this row
    for (int64_t base = b; base < e; base += kBlockPass) {
      const int64_t p = base + threadIdx.x;
      int64_t c = 0;
      bool keep = false;
      if (p < e) { c = col[p]; keep = flag[c] != 0; }
      const unsigned long long m = __ballot(keep);
      if (lane == 0) wave_cnt[w] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int k = 0; k < kWavesPerBlock; ++k) {
        const int ck = wave_cnt[k];
        before += k < w ? ck : 0;
        total += ck;
      }
      if (keep) emit(o, off + before + __popcll(m & below), i, c, p);
      off += total;
      __syncthreads();                                  // wave_cnt is rewritten by the next pass
    }
  }
}

__global__ void saint_gather_kernel(const int64_t* __restrict__ node_idx, int64_t n_sub, const int64_t* __restrict__ node_type,
                                    const int64_t* __restrict__ local_idx, const int64_t* __restrict__ y,
                                    const uint8_t* __restrict__ train_mask, int64_t* __restrict__ o_node_type,
                                    int64_t* __restrict__ o_local_idx, int64_t* __restrict__ o_y, uint8_t* __restrict__ o_train_mask,
                                    const int64_t* __restrict__ edge_idx, int64_t e_sub, const int64_t* __restrict__ edge_attr,
                                    int64_t* __restrict__ o_edge_attr) {
  const int64_t n = n_sub > e_sub ? n_sub : e_sub;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    if (i < n_sub) {
      const int64_t g = node_idx[i];
      if (node_type) o_node_type[i] = node_type[g];
      if (local_idx) o_local_idx[i] = local_idx[g];
      if (y) o_y[i] = y[g];
      if (train_mask) o_train_mask[i] = train_mask[g];
    }
    if (i < e_sub && edge_attr) o_edge_attr[i] = edge_attr[edge_idx[i]];
  }
}

constexpr int64_t kMaxItems = 0x7fffffffLL;   // hipCUB item counts are int; node ids below 2^31

bool view_ok(const int64_t* rowptr, const int64_t* col, const int64_t* row_map, int64_t n_map, int64_t groups, int64_t group_stride,
             int64_t N, const uint8_t* flag) {
  if (!rowptr || !col || !row_map || !flag) return false;
  if (n_map < 1 || groups < 1 || group_stride < 0 || N < 1 || N >= kMaxItems) return false;
  if (groups > kMaxItems / n_map || groups * n_map + 1 >= kMaxItems) return false;
  return true;
}

}  // namespace

extern "C" int64_t egnn_saint_induced_geometry(int which) {
  switch (which) {
    case 0: return kWavePass;
    case 1: return kBlockPass;
    case 2: return kLongRow;
    default: return EGNN_EINVAL;
  }
}

extern "C" int egnn_saint_random_walk_i64(const int64_t* rowptr, const int64_t* col, int64_t N, int64_t nnz, int64_t B, int64_t L,
                                          const int64_t* start, const float* rnd, uint64_t seed, const uint64_t* seed_dev,
                                          int64_t* walks, uint8_t* flag, void* stream) {
  EGNN_CHECK_ARG(rowptr && flag && N >= 1 && N < kMaxItems && nnz >= 0 && (nnz == 0 || col));
  EGNN_CHECK_ARG(B >= 0 && L >= 1 && B < kMaxItems && L < 65536);
  EGNN_CHECK_ARG((start == nullptr) == (rnd == nullptr));   // both injected, or both drawn here
  if (B == 0) return EGNN_OK;
  hipLaunchKernelGGL(saint_walk_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, rowptr,
                     col, N, B, L, start, rnd, (unsigned long long)seed, (const unsigned long long*)seed_dev, walks, flag);
  return egnn_launch_status();
}

extern "C" size_t egnn_saint_scan_ws_bytes(int64_t items) {
  if (items <= 0 || items >= kMaxItems) return kAlign;
  size_t bytes = 0;
  (void)exclusive_scan(nullptr, bytes, CountAt{nullptr, 0}, (int64_t*)nullptr, items + 1, (hipStream_t)0);
  return (bytes + kAlign - 1) / kAlign * kAlign + kAlign;
}

extern "C" int egnn_saint_select_i64(const uint8_t* flag, int64_t N, int64_t* relabel, int64_t* node_idx, int64_t node_cap, void* ws,
                                     size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(flag && relabel && node_idx && N >= 1 && N < kMaxItems && node_cap >= 1);
  if (!ws || ws_bytes < egnn_saint_scan_ws_bytes(N)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  size_t tb = ws_bytes;
  if (exclusive_scan(ws, tb, FlagAt{flag, N}, relabel, N + 1, st) != hipSuccess) return EGNN_ELAUNCH;
  hipLaunchKernelGGL(saint_compact_kernel, dim3(grid_for(N, kThreads)), dim3(kThreads), 0, st, flag, relabel, N, node_idx, node_cap);
  return egnn_launch_status();
}

extern "C" int egnn_saint_induced_count_i64(const int64_t* rowptr, const int64_t* col, const int64_t* row_map, int64_t n_map,
                                            const int64_t* n_map_dev, int64_t groups, int64_t group_stride, int64_t N,
                                            const uint8_t* flag, int64_t* counts, int64_t* out_ptr, void* ws, size_t ws_bytes,
                                            void* stream) {
  EGNN_CHECK_ARG(view_ok(rowptr, col, row_map, n_map, groups, group_stride, N, flag) && counts && out_ptr);
  const int64_t R = groups * n_map;
  if (!ws || ws_bytes < egnn_saint_scan_ws_bytes(R)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const RowView v{rowptr, row_map, n_map, n_map_dev, group_stride};
  hipLaunchKernelGGL(induced_count_wave_kernel, dim3(grid_for(R, kWavesPerBlock)), dim3(kThreads), 0, st, v, col, R, flag, counts);
  hipLaunchKernelGGL(induced_count_block_kernel, dim3(grid_for(R, 64)), dim3(kThreads), 0, st, v, col, R, flag, counts);
  size_t tb = ws_bytes;
  if (exclusive_scan(ws, tb, CountAt{counts, R}, out_ptr, R + 1, st) != hipSuccess) return EGNN_ELAUNCH;
  return egnn_launch_status();
}

extern "C" int egnn_saint_induced_fill_i64(const int64_t* rowptr, const int64_t* col, const int64_t* val, const int64_t* row_map,
                                           int64_t n_map, const int64_t* n_map_dev, int64_t groups, int64_t group_stride, int64_t N,
                                           const uint8_t* flag, const int64_t* relabel, const int64_t* out_ptr, int64_t out_cap,
                                           int64_t* out_row, int64_t* out_col, int64_t* out_val, void* stream) {
  EGNN_CHECK_ARG(view_ok(rowptr, col, row_map, n_map, groups, group_stride, N, flag) && relabel && out_ptr && out_cap >= 0);
  EGNN_CHECK_ARG(out_cap == 0 || out_col);
  if (out_cap == 0) return EGNN_OK;
  const int64_t R = groups * n_map;
  hipStream_t st = (hipStream_t)stream;
  const RowView v{rowptr, row_map, n_map, n_map_dev, group_stride};
  const FillOut o{val, relabel, out_ptr, out_cap, out_row, out_col, out_val};
  hipLaunchKernelGGL(induced_fill_wave_kernel, dim3(grid_for(R, kWavesPerBlock)), dim3(kThreads), 0, st, v, col, R, flag, o);
  hipLaunchKernelGGL(induced_fill_block_kernel, dim3(grid_for(R, 64)), dim3(kThreads), 0, st, v, col, R, flag, o);
  return egnn_launch_status();
}

extern "C" int egnn_saint_gather_i64(const int64_t* node_idx, int64_t n_sub, const int64_t* node_type, const int64_t* local_idx,
                                     const int64_t* y, const uint8_t* train_mask, int64_t* o_node_type, int64_t* o_local_idx,
                                     int64_t* o_y, uint8_t* o_train_mask, const int64_t* edge_idx, int64_t e_sub,
                                     const int64_t* edge_attr, int64_t* o_edge_attr, void* stream) {
  EGNN_CHECK_ARG(n_sub >= 0 && e_sub >= 0 && (n_sub == 0 || node_idx));
  EGNN_CHECK_ARG((!node_type || o_node_type) && (!local_idx || o_local_idx) && (!y || o_y) && (!train_mask || o_train_mask));
  EGNN_CHECK_ARG(!edge_attr || e_sub == 0 || (edge_idx && o_edge_attr));
  const int64_t n = n_sub > e_sub ? n_sub : e_sub;
  if (n == 0) return EGNN_OK;
  hipLaunchKernelGGL(saint_gather_kernel, dim3(grid_for(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, node_idx, n_sub, node_type,
                     local_idx, y, train_mask, o_node_type, o_local_idx, o_y, o_train_mask, edge_idx, e_sub, edge_attr, o_edge_attr);
  return egnn_launch_status();
}
