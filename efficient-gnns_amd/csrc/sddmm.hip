// Sampled dense-dense product over a CSR pattern (SDDMM): the gradient of a neighbour aggregation with respect to its entry values,
//   dval[e] = row_scale[r] * sum_k m(e,k) * G[r,k] * X[col[e],k],   r = row of entry e
// (torch-sparse `spmm` value backward).  G = dY of the aggregation, X its dense operand; m = 1 for sum / mean and
// (argmax[r,k] == e) for max.
//
// Work is cut over ENTRIES, not rows: a wavefront owns a fixed chunk of kChunk consecutive entries, finds the row of the chunk's first
// entry with one wave-uniform binary search in rowptr and walks forward from there, so a hub row of thousands of entries is spread over
// as many wavefronts as any other stretch of the entry array.  Inside the chunk a group of G lanes owns one entry (G = the power of
// two at or above ceil(K / 4), at most 64): float4 lanes along the row, the group looping when K > 256, and 64 / G entries per
// wave-instruction.  No atomics; every entry is written exactly once with a summation order fixed by (K, G): bit-stable.
// HBM/L2-bound gather work: no MFMA.
#include "common.h"

namespace {

constexpr int kChunk = 256;   // entries per wavefront pass

// VEC4: K % 4 == 0 and 16-byte aligned rows of G and X; otherwise the lanes of a group walk the row one float at a time
template <int G, bool VEC4, typename I>
__global__ __launch_bounds__(256) void sddmm_kernel(const float* __restrict__ Gm, int64_t ldg, const float* __restrict__ X, int64_t ldx,
                                                    int64_t K, const I* __restrict__ rowptr, const I* __restrict__ col, int64_t n_rows,
                                                    int64_t nnz, const float* __restrict__ row_scale,
                                                    const int64_t* __restrict__ argmax, float* __restrict__ dval) {
  constexpr int EPW = 64 / G;                       // entries per wave-instruction
  const int lane = egnn_lane();
  const int grp = lane / G, sl = lane % G;
  const bool one_pass = VEC4 && K <= 4 * G;         // a lane holds its whole share of the G row: kept across the entries of one row
  const int64_t n_chunks = (nnz + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x * 4LL + egnn_wave_id(); c < n_chunks; c += (int64_t)gridDim.x * 4) {
    const int64_t e0 = c * kChunk;
    const int64_t e1 = e0 + kChunk < nnz ? e0 + kChunk : nnz;
    // row of entry e0: the first r with rowptr[r + 1] > e0 (wave-uniform: every lane searches the same value)
    int64_t lo = 0, hi = n_rows - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)rowptr[mid + 1] <= e0) lo = mid + 1; else hi = mid;
    }
    int64_t r = lo, r_held = -1;
    float4 gh = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t eb = e0; eb < e1; eb += EPW) {
      const int64_t e = eb + grp;
      const bool on = e < e1;
      float acc = 0.f;
      if (on) {
        while (r + 1 < n_rows && (int64_t)rowptr[r + 1] <= e) ++r;   // forward walk; empty rows are stepped over
        const float* g = Gm + r * ldg;
        const float* x = X + (int64_t)col[e] * ldx;
        const int64_t* am = argmax ? argmax + r * K : nullptr;
        if constexpr (VEC4) {
          if (one_pass) {
            const int64_t d = 4 * sl;
            if (d < K) {
              if (r != r_held) { gh = *reinterpret_cast<const float4*>(g + d); r_held = r; }
              const float4 xv = *reinterpret_cast<const float4*>(x + d);
              if (am) acc = (am[d] == e ? gh.x * xv.x : 0.f) + (am[d + 1] == e ? gh.y * xv.y : 0.f) + (am[d + 2] == e ? gh.z * xv.z : 0.f) +
                            (am[d + 3] == e ? gh.w * xv.w : 0.f);
              else acc = gh.x * xv.x + gh.y * xv.y + gh.z * xv.z + gh.w * xv.w;
            }
          } else {
            for (int64_t d = 4 * sl; d < K; d += 4 * G) {
              const float4 gv = *reinterpret_cast<const float4*>(g + d);
              const float4 xv = *reinterpret_cast<const float4*>(x + d);
              if (am) acc += (am[d] == e ? gv.x * xv.x : 0.f) + (am[d + 1] == e ? gv.y * xv.y : 0.f) + (am[d + 2] == e ? gv.z * xv.z : 0.f) +
                             (am[d + 3] == e ? gv.w * xv.w : 0.f);
              else acc += gv.x * xv.x + gv.y * xv.y + gv.z * xv.z + gv.w * xv.w;
            }
          }
        } else {
          for (int64_t d = sl; d < K; d += G) {
            if (!am || am[d] == e) acc += g[d] * x[d];
          }
        }
      }
      acc = egnn_group_sum<G>(acc);
      if (on && sl == 0) dval[e] = row_scale ? row_scale[r] * acc : acc;
    }
  }
}

template <int G, typename I>
void launch_g(bool vec4, unsigned grid, hipStream_t st, const float* Gm, int64_t ldg, const float* X, int64_t ldx, int64_t K, const void* rowptr,
              const void* col, int64_t n_rows, int64_t nnz, const float* row_scale, const int64_t* argmax, float* dval) {
  const I* rp = static_cast<const I*>(rowptr);
  const I* ci = static_cast<const I*>(col);
  if (vec4) hipLaunchKernelGGL((sddmm_kernel<G, true, I>), dim3(grid), dim3(256), 0, st, Gm, ldg, X, ldx, K, rp, ci, n_rows, nnz, row_scale, argmax, dval);
  else hipLaunchKernelGGL((sddmm_kernel<G, false, I>), dim3(grid), dim3(256), 0, st, Gm, ldg, X, ldx, K, rp, ci, n_rows, nnz, row_scale, argmax, dval);
}

template <typename I>
void launch_i(int G, bool vec4, unsigned grid, hipStream_t st, const float* Gm, int64_t ldg, const float* X, int64_t ldx, int64_t K,
              const void* rowptr, const void* col, int64_t n_rows, int64_t nnz, const float* row_scale, const int64_t* argmax, float* dval) {
#define EGNN_SDDMM_CASE(g) \
  case g: launch_g<g, I>(vec4, grid, st, Gm, ldg, X, ldx, K, rowptr, col, n_rows, nnz, row_scale, argmax, dval); break;
  switch (G) {
    EGNN_SDDMM_CASE(1) EGNN_SDDMM_CASE(2) EGNN_SDDMM_CASE(4) EGNN_SDDMM_CASE(8) EGNN_SDDMM_CASE(16) EGNN_SDDMM_CASE(32)
    default: launch_g<64, I>(vec4, grid, st, Gm, ldg, X, ldx, K, rowptr, col, n_rows, nnz, row_scale, argmax, dval); break;
  }
#undef EGNN_SDDMM_CASE
}

}  // namespace

extern "C" int egnn_sddmm_csr_f32(int64_t n_rows, int64_t n_src, int64_t K, const void* rowptr, const void* col, int index_bits, int64_t nnz,
                                  const float* G, int64_t ldg, const float* X, int64_t ldx, const float* row_scale, const int64_t* argmax,
                                  float* dval, void* stream) {
  EGNN_CHECK_ARG(n_rows >= 0 && n_src >= 0 && K >= 0 && nnz >= 0 && ldg >= K && ldx >= K);
  EGNN_CHECK_ARG(index_bits == 32 || index_bits == 64);
  if (nnz == 0) return EGNN_OK;
  EGNN_CHECK_ARG(n_rows > 0 && n_src > 0 && rowptr && col && dval && (K == 0 || (G && X)));
  EGNN_CHECK_ARG(index_bits == 64 || (nnz <= 0x7fffffffLL && n_src <= 0x7fffffffLL));
  int lanes = 1;                                   // the power of two at or above ceil(K / 4), at most 64
  while (lanes < 64 && 4LL * lanes < K) lanes <<= 1;
  const bool vec4 = K > 0 && K % 4 == 0 && ldg % 4 == 0 && ldx % 4 == 0 && egnn_aligned16(G) && egnn_aligned16(X);
  const int64_t blocks = ((nnz + kChunk - 1) / kChunk + 3) / 4;
  const unsigned grid = (unsigned)(blocks < (1LL << 20) ? blocks : (1LL << 20));
  hipStream_t st = (hipStream_t)stream;
  if (index_bits == 32) launch_i<int32_t>(lanes, vec4, grid, st, G, ldg, X, ldx, K, rowptr, col, n_rows, nnz, row_scale, argmax, dval);
  else launch_i<int64_t>(lanes, vec4, grid, st, G, ldg, X, ldx, K, rowptr, col, n_rows, nnz, row_scale, argmax, dval);
  return egnn_launch_status();
}
