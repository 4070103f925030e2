// Structure-preservation metrics of the reference's analysis script (arxiv_pyg/correlation.py) for gfx950: the sufficient
// statistics of a Pearson correlation, over all unordered row pairs (Mantel / global structural correlation, :178-181, 205-208, 212)
// and over two plain vectors (local structural correlation, :182, 209, 213).
//
// The reference forms 1 - X X^T for teacher and student (two N x N fp32 matrices), moves them to the host, condenses them with
// squareform and calls scipy.stats.pearsonr.  Pearson r is invariant under a -> 1 - a applied to both variables (the sign flips
// twice), so the SIMILARITIES a = <xs_i, xs_j>, b = <xt_i, xt_j> are accumulated instead of the distances, and r needs only
//      out6 = (n, sum a, sum b, sum a^2, sum b^2, sum ab)      over the pairs i < j.
// No N x N object exists: one workgroup per 128 x 128 tile of the upper triangle (tj >= ti; T(T+1)/2 of the T^2 tiles) runs the
// fp32-MFMA mainloop twice (student Gram tile, teacher Gram tile -- as gsp_fwd_kernel of pairwise.hip does) and reduces both
// accumulator sets in registers.
// Precision split: a lane sums its <= 64 accumulator entries in fp32; from the wave reduction onwards everything is float64 and in
// a fixed order (wave butterfly, 4 waves in order, per-tile partials in the workspace, one finalising launch).  No atomics: two calls
// give bit-equal results.
// Conditioning: r is formed from n sum a^2 - (sum a)^2, which loses mean^2 / variance of the digits its inputs carry -- 1e4 and more
// when a teacher's cosines all sit in a narrow band -- so the fp32 lane sums are taken about the TILE'S OWN MEAN: a first pass over
// the registers gives the tile means (c_a, c_b), a second one sums (a - c_a), (b - c_b) and their products (small numbers, no
// cancellation left for fp32 to lose), and the tile's raw moments are restored in float64,
//      sum a = S_a + n c_a,   sum a^2 = S_aa + 2 c_a S_a + n c_a^2,   sum ab = S_ab + c_a S_b + c_b S_a + n c_a c_b,
// so that the float64 cancellation downstream sees inputs good to fp32 RELATIVE TO THE SPREAD, not to the mean.
#include "gemm_core.h"

using namespace egnn_gemm;

namespace {

constexpr int GB = 128;
constexpr int kMoments = 6;         // n, sum a, sum b, sum a^2, sum b^2, sum ab
constexpr int kVecBlocks = 1024;    // upper bound of the vector kernel's grid

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// first block index of tile row ti in the row-major walk of the upper triangle (row ti holds the T - ti tiles tj = ti .. T-1)
__host__ __device__ __forceinline__ int64_t tri_row_start(int64_t ti, int64_t T) { return ti * T - ti * (ti - 1) / 2; }

// sum over the 256 threads of K values each, in a fixed order (wave butterfly, then the 4 waves in order); every thread gets the
// totals.  `red` holds 4 * K doubles and is free again when the call returns.
template <int K>
__device__ __forceinline__ void block_sum_f64(double (&m)[K], double* red) {
  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
#pragma unroll
  for (int q = 0; q < K; ++q) m[q] = wave_sum_f64(m[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < K; ++q) red[wave * K + q] = m[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; ++q) m[q] = ((red[q] + red[K + q]) + red[2 * K + q]) + red[3 * K + q];
  __syncthreads();
}

template <bool VEC4>
__global__ __launch_bounds__(256) void pair_moments_kernel(const float* __restrict__ xs, int64_t lds_, int64_t Ps,
                                                           const float* __restrict__ xt, int64_t ldt, int64_t Pt, int64_t N,
                                                           int64_t T, double* __restrict__ partials) {
  using TS = TileShape<GB, GB>;
  __shared__ __attribute__((aligned(16))) float smem[TS::SMEM_FLOATS];
  // block index -> (ti, tj), tj >= ti: a float64 estimate of the inverse of tri_row_start, then an exact integer correction
  const int64_t b = blockIdx.x;
  const double tt = 2.0 * (double)T + 1.0;
  int64_t ti = (int64_t)((tt - sqrt(fmax(tt * tt - 8.0 * (double)b, 0.0))) * 0.5);
  ti = ti < 0 ? 0 : (ti > T - 1 ? T - 1 : ti);
  while (ti > 0 && tri_row_start(ti, T) > b) --ti;
  while (ti + 1 < T && tri_row_start(ti + 1, T) <= b) ++ti;
  const int64_t tj = ti + (b - tri_row_start(ti, T));
  const int64_t i0 = ti * GB, j0 = tj * GB;

  IdentityXf id;
  f32x16 as[TS::TM][TS::TN], at[TS::TM][TS::TN];
  zero_acc(as);
  zero_acc(at);
  mainloop<GB, GB, KMAJOR, KMAJOR, VEC4>(as, xs, lds_, i0, N, xs, lds_, j0, N, 0, Ps, id, id, smem);
  mainloop<GB, GB, KMAJOR, KMAJOR, VEC4>(at, xt, ldt, i0, N, xt, ldt, j0, N, 0, Pt, id, id, smem);
  // the mainloop's last barrier has passed: its LDS is free
  double* red = reinterpret_cast<double*>(smem);

  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  // pass 1: pairs of this tile and their means.  row < col keeps the strict upper triangle of a diagonal tile (always true off the
  // diagonal); col < N cuts the ragged edge.  Tile-local 32-bit form: row - i0 < col - i0 = lc + dj, lc < ncols
  const int dj = (int)(j0 - i0);
  const int ncols = (int)(N - j0 < GB ? N - j0 : GB);
  float cnt = 0.f, sa = 0.f, sb = 0.f;
#pragma unroll
  for (int tn = 0; tn < TS::TN; ++tn) {
    const int lc = acc_col<GB, GB>(wn, tn, lane);
#pragma unroll
    for (int tm = 0; tm < TS::TM; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = acc_row<GB, GB>(wm, tm, r, lane);
        if (lr < lc + dj && lc < ncols) {
          cnt += 1.f;
          sa += as[tm][tn][r];
          sb += at[tm][tn][r];
        }
      }
    }
  }
  double m1[3] = {(double)cnt, (double)sa, (double)sb};
  block_sum_f64(m1, red);
  const double n = m1[0];
  const float ca = n > 0.0 ? (float)(m1[1] / n) : 0.f;
  const float cb = n > 0.0 ? (float)(m1[2] / n) : 0.f;
  // pass 2: moments about (ca, cb)
  float da = 0.f, db = 0.f, daa = 0.f, dbb = 0.f, dab = 0.f;
#pragma unroll
  for (int tn = 0; tn < TS::TN; ++tn) {
    const int lc = acc_col<GB, GB>(wn, tn, lane);
#pragma unroll
    for (int tm = 0; tm < TS::TM; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = acc_row<GB, GB>(wm, tm, r, lane);
        if (lr < lc + dj && lc < ncols) {
          const float a = as[tm][tn][r] - ca, bb = at[tm][tn][r] - cb;
          da += a;
          db += bb;
          daa = fmaf(a, a, daa);
          dbb = fmaf(bb, bb, dbb);
          dab = fmaf(a, bb, dab);
        }
      }
    }
  }
  double m2[5] = {(double)da, (double)db, (double)daa, (double)dbb, (double)dab};
  block_sum_f64(m2, red);
  if (threadIdx.x == 0) {
    const double A = (double)ca, B = (double)cb;
    double* out = partials + b * kMoments;
    out[0] = n;
    out[1] = m2[0] + n * A;
    out[2] = m2[1] + n * B;
    out[3] = (m2[2] + 2.0 * A * m2[0]) + n * A * A;
    out[4] = (m2[3] + 2.0 * B * m2[1]) + n * B * B;
    out[5] = ((m2[4] + A * m2[1]) + B * m2[0]) + n * A * B;
  }
}

__global__ __launch_bounds__(256) void vec_moments_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                          double* __restrict__ partials) {
  __shared__ double red[4 * kMoments];
  double m[kMoments] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double x = (double)a[i], y = (double)b[i];
    m[0] += 1.0;
    m[1] += x;
    m[2] += y;
    m[3] = fma(x, x, m[3]);
    m[4] = fma(y, y, m[4]);
    m[5] = fma(x, y, m[5]);
  }
  block_sum_f64(m, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kMoments; ++q) partials[(int64_t)blockIdx.x * kMoments + q] = m[q];
  }
}

// out6[q] = sum over the `count` partial sextets, fixed order: thread t takes partials t, t + 1024, ..., then a tree over the threads
__global__ __launch_bounds__(1024) void moments_finalize_kernel(const double* __restrict__ partials, int64_t count,
                                                                double* __restrict__ out6) {
  __shared__ double red[kMoments][1024];
  double m[kMoments] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < count; i += 1024) {
#pragma unroll
    for (int q = 0; q < kMoments; ++q) m[q] += partials[i * kMoments + q];
  }
#pragma unroll
  for (int q = 0; q < kMoments; ++q) red[q][threadIdx.x] = m[q];
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < kMoments; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < kMoments) out6[threadIdx.x] = red[threadIdx.x][0];
}

inline int64_t pair_tiles(int64_t N) {
  const int64_t T = (N + GB - 1) / GB;
  return T * (T + 1) / 2;
}

inline int64_t vec_blocks(int64_t n) {
  const int64_t want = (n + 255) / 256;
  return want < kVecBlocks ? want : kVecBlocks;
}

}  // namespace

extern "C" size_t egnn_pair_moments_ws_bytes(int64_t N) {
  if (N < 1) return 0;
  return (size_t)pair_tiles(N) * kMoments * sizeof(double);
}

extern "C" int egnn_pair_moments_f32(const float* xs, int64_t ld_s, int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt,
                                     int64_t N, double* out6, void* ws, size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(N >= 2 && Ps > 0 && Pt > 0 && ld_s >= Ps && ld_t >= Pt);
  EGNN_CHECK_ARG(xs && xt && out6);
  if (ws_bytes < egnn_pair_moments_ws_bytes(N)) return EGNN_EWORKSPACE;
  EGNN_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out6) & 7u) == 0);
  const int64_t T = (N + GB - 1) / GB;
  const int64_t nblocks = pair_tiles(N);
  if (nblocks > 0x7fffffffLL) return EGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* partials = static_cast<double*>(ws);
  const bool vec4 = (ld_s % 4 == 0) && (ld_t % 4 == 0) && egnn_aligned16(xs) && egnn_aligned16(xt);
  if (vec4) hipLaunchKernelGGL(pair_moments_kernel<true>, dim3((unsigned)nblocks), dim3(256), 0, st, xs, ld_s, Ps, xt, ld_t, Pt, N, T, partials);
  else hipLaunchKernelGGL(pair_moments_kernel<false>, dim3((unsigned)nblocks), dim3(256), 0, st, xs, ld_s, Ps, xt, ld_t, Pt, N, T, partials);
  hipLaunchKernelGGL(moments_finalize_kernel, dim3(1), dim3(1024), 0, st, partials, nblocks, out6);
  return egnn_launch_status();
}

extern "C" size_t egnn_pearson_moments_ws_bytes(int64_t n) {
  if (n < 1) return 0;
  return (size_t)vec_blocks(n) * kMoments * sizeof(double);
}

extern "C" int egnn_pearson_moments_f32(const float* a, const float* b, int64_t n, double* out6, void* ws, size_t ws_bytes,
                                        void* stream) {
  EGNN_CHECK_ARG(n >= 1 && a && b && out6);
  if (ws_bytes < egnn_pearson_moments_ws_bytes(n)) return EGNN_EWORKSPACE;
  EGNN_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out6) & 7u) == 0);
  hipStream_t st = (hipStream_t)stream;
  double* partials = static_cast<double*>(ws);
  const int64_t nb = vec_blocks(n);
  hipLaunchKernelGGL(vec_moments_kernel, dim3((unsigned)nb), dim3(256), 0, st, a, b, n, partials);
  hipLaunchKernelGGL(moments_finalize_kernel, dim3(1), dim3(1024), 0, st, partials, nb, out6);
  return egnn_launch_status();
}
