// What the all-pairs kernels of pairwise.hip (GSP) and similarity.hip (Mantel moments, median of the distances, RBF CKA) share: one
// workgroup of 256 threads owns one 128 x 128 tile of an N x N pair matrix, runs the fp32-MFMA mainloop twice (student Gram tile,
// teacher Gram tile) and consumes both accumulator sets in registers.  The pair predicate, the walk over a lane's accumulator
// entries, the upper-triangle tile map are defined here and nowhere else; the fixed-order float64 block sum is block_reduce.h's.
#pragma once
#include <type_traits>

#include "gemm_core.h"
#include "block_reduce.h"

namespace egnn_pair {

using namespace egnn_gemm;

constexpr int GB = 128;
using TS = TileShape<GB, GB>;

// first block index of tile row ti in the row-major walk of the upper triangle (row ti holds the T - ti tiles tj = ti .. T-1)
__host__ __device__ __forceinline__ int64_t tri_row_start(int64_t ti, int64_t T) { return ti * T - ti * (ti - 1) / 2; }

// block index -> (ti, tj), tj >= ti: a float64 estimate of the inverse of tri_row_start, then an exact integer correction
__device__ __forceinline__ void tri_tile(int64_t b, int64_t T, int64_t& ti_out, int64_t& tj_out) {
  const double tt = 2.0 * (double)T + 1.0;
  int64_t ti = (int64_t)((tt - sqrt(fmax(tt * tt - 8.0 * (double)b, 0.0))) * 0.5);
  ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
  while (ti > 0 && tri_row_start(ti, T) > b) --ti;
  while (ti + 1 < T && tri_row_start(ti + 1, T) <= b) ++ti;
  ti_out = ti;
  tj_out = ti + (b - tri_row_start(ti, T));
}

inline int64_t pair_tiles(int64_t N) {
  const int64_t T = (N + GB - 1) / GB;
  return T * (T + 1) / 2;
}

// sum over the 256 threads of K values each, in a fixed order (wave butterfly, then the 4 waves in order); every thread gets the
// totals.  `red` holds 4 * K doubles and is free again when the call returns.
template <int K>
__device__ __forceinline__ void block_sum_f64(double (&m)[K], double* red) {
#pragma unroll
  for (int q = 0; q < K; ++q) m[q] = egnn_reduce::group_sum<EGNN_WAVE>(m[q]);
  egnn_reduce::waves4_sum<egnn_reduce::SERIAL>(m, red);
}

// Which entries of the tile at (i0, j0) are pairs, in tile-local 32-bit form: entry (lr, lc) is row i0 + lr, column j0 + lc, and
// row - i0 < col - i0 = lc + dj.  row < col keeps the strict upper triangle of a diagonal tile (always true in a tile off the
// diagonal of the upper triangle); col < N cuts the ragged edge, and with row <= col it bounds the row as well.
struct PairGeom {
  int dj, ncols;
  __device__ __forceinline__ PairGeom(int64_t i0, int64_t j0, int64_t N) : dj((int)(j0 - i0)), ncols((int)(N - j0 < GB ? N - j0 : GB)) {}
  __device__ __forceinline__ bool in_cols(int lc) const { return lc < ncols; }
  __device__ __forceinline__ bool diag(int lr, int lc) const { return lr == lc + dj; }
  __device__ __forceinline__ bool above(int lr, int lc) const { return lr < lc + dj && lc < ncols; }
  __device__ __forceinline__ bool on_or_above(int lr, int lc) const { return lr <= lc + dj && lc < ncols; }
};

// as = Xs[i0.., :] Xs[j0.., :]^T, at = Xt[i0.., :] Xt[j0.., :]^T over the N rows; when it returns the mainloop's last barrier has
// passed and `smem` (TS::SMEM_FLOATS floats) is free
template <bool VEC4>
__device__ __forceinline__ void gram_pair(f32x16 (&as)[TS::TM][TS::TN], f32x16 (&at)[TS::TM][TS::TN], const float* xs, int64_t ld_s,
                                          int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt, int64_t i0, int64_t j0, int64_t N,
                                          float* smem) {
  IdentityXf id;
  zero_acc(as);
  zero_acc(at);
  mainloop<GB, GB, KMAJOR, KMAJOR, VEC4>(as, xs, ld_s, i0, N, xs, ld_s, j0, N, 0, Ps, id, id, smem);
  mainloop<GB, GB, KMAJOR, KMAJOR, VEC4>(at, xt, ld_t, i0, N, xt, ld_t, j0, N, 0, Pt, id, id, smem);
}

// f(tm, tn, r, lr, lc, col(lc)) for this lane's 64 accumulator entries acc[tm][tn][r] at tile-local (lr, lc), columns outermost and
// col(lc) formed once per column; the second form has no column value.  No branch: every lane makes every call (ballots rely on it).
template <class C, class F>
__device__ __forceinline__ void for_each_entry(C&& col, F&& f) {
  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
  const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int tn = 0; tn < TS::TN; ++tn) {
    const int lc = acc_col<GB, GB>(wn, tn, lane);
    const auto cv = col(lc);
#pragma unroll
    for (int tm = 0; tm < TS::TM; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) f(tm, tn, r, acc_row<GB, GB>(wm, tm, r, lane), lc, cv);
    }
  }
}
template <class F>
__device__ __forceinline__ void for_each_entry(F&& f) {
  for_each_entry([](int) { return 0; }, [&](int tm, int tn, int r, int lr, int lc, int) { f(tm, tn, r, lr, lc); });
}

// out[row] = |x_row|^2 in fp32, one wave per row
static __global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ x, int64_t ld, int64_t P, int64_t N,
                                                                float* __restrict__ out) {
  const int lane = egnn_lane();
  const int64_t row = (int64_t)blockIdx.x * 4 + egnn_wave_id();
  if (row >= N) return;
  const float* xr = x + row * ld;
  float s = 0.f;
  for (int64_t k = lane; k < P; k += 64) s = fmaf(xr[k], xr[k], s);
  s = egnn_wave_sum(s);
  if (lane == 0) out[row] = s;
}

inline void row_sqnorm(const float* x, int64_t ld, int64_t P, int64_t N, float* out, hipStream_t st) {
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, x, ld, P, N, out);
}

// launch(std::bool_constant<vec4>): a kernel template on VEC4 is launched by one expression, `kernel<v.value>`, for both paths
template <class L>
inline void dispatch_vec4(bool vec4, L&& launch) {
  if (vec4) launch(std::true_type{});
  else launch(std::false_type{});
}

}  // namespace egnn_pair
