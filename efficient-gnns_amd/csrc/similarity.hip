// Structure-preservation metrics of the reference's analysis script (arxiv_pyg/correlation.py) for gfx950: the sufficient
// statistics of a Pearson correlation, over all unordered row pairs (Mantel / global structural correlation, :178-181, 205-208, 212)
// and over two plain vectors (local structural correlation, :182, 209, 213); further down, kernel (RBF) CKA with its median
// bandwidth (:41-53, 70-75), which has its own comment.
//
// The reference forms 1 - X X^T for teacher and student (two N x N fp32 matrices), moves them to the host, condenses them with
// squareform and calls scipy.stats.pearsonr.  Pearson r is invariant under a -> 1 - a applied to both variables (the sign flips
// twice), so the SIMILARITIES a = <xs_i, xs_j>, b = <xt_i, xt_j> are accumulated instead of the distances, and r needs only
//      out6 = (n, sum a, sum b, sum a^2, sum b^2, sum ab)      over the pairs i < j.
// No N x N object exists: one workgroup per 128 x 128 tile of the upper triangle (tj >= ti; T(T+1)/2 of the T^2 tiles) runs the
// fp32-MFMA mainloop twice (student Gram tile, teacher Gram tile -- gram_pair of pair_tile.h, which also holds the pair predicate
// and the walk over the accumulators) and reduces both accumulator sets in registers.
// Precision split: a lane sums its <= 64 accumulator entries in fp32; from the wave reduction onwards everything is float64 and in
// a fixed order (wave butterfly, 4 waves in order, per-tile partials in the workspace, one finalising launch).  No atomics: two calls
// give bit-equal results.
// Conditioning: r is formed from n sum a^2 - (sum a)^2, which loses mean^2 / variance of the digits its inputs carry -- 1e4 and more
// when a teacher's cosines all sit in a narrow band -- so the fp32 lane sums are taken about the TILE'S OWN MEAN: a first pass over
// the registers gives the tile means (c_a, c_b), a second one sums (a - c_a), (b - c_b) and their products (small numbers, no
// cancellation left for fp32 to lose), and the tile's raw moments are restored in float64,
//      sum a = S_a + n c_a,   sum a^2 = S_aa + 2 c_a S_a + n c_a^2,   sum ab = S_ab + c_a S_b + c_b S_a + n c_a c_b,
// so that the float64 cancellation downstream sees inputs good to fp32 RELATIVE TO THE SPREAD, not to the mean.
#include "pair_tile.h"
#include "block_reduce.h"

using namespace egnn_pair;
using namespace egnn_reduce;

namespace {

constexpr int kMoments = 6;         // n, sum a, sum b, sum a^2, sum b^2, sum ab
constexpr int kVecBlocks = 1024;    // upper bound of the vector kernel's grid

template <bool VEC4>
__global__ __launch_bounds__(256) void pair_moments_kernel(const float* __restrict__ xs, int64_t lds_, int64_t Ps,
                                                           const float* __restrict__ xt, int64_t ldt, int64_t Pt, int64_t N,
                                                           int64_t T, double* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float smem[TS::SMEM_FLOATS];
  const int64_t b = blockIdx.x;
  int64_t ti, tj;
  tri_tile(b, T, ti, tj);
  const int64_t i0 = ti * GB, j0 = tj * GB;

  f32x16 as[TS::TM][TS::TN], at[TS::TM][TS::TN];
  gram_pair<VEC4>(as, at, xs, lds_, Ps, xt, ldt, Pt, i0, j0, N, smem);
  double* red = reinterpret_cast<double*>(smem);

  // pass 1: pairs of this tile and their means
  const PairGeom g(i0, j0, N);
  float cnt = 0.f, sa = 0.f, sb = 0.f;
  for_each_entry([&](int tm, int tn, int r, int lr, int lc) {
    if (g.above(lr, lc)) {
      cnt += 1.f;
      sa += as[tm][tn][r];
      sb += at[tm][tn][r];
    }
  });
  double m1[3] = {(double)cnt, (double)sa, (double)sb};
  block_sum_f64(m1, red);
  const double n = m1[0];
  const float ca = n > 0.0 ? (float)(m1[1] / n) : 0.f;
  const float cb = n > 0.0 ? (float)(m1[2] / n) : 0.f;
  // pass 2: moments about (ca, cb)
  float da = 0.f, db = 0.f, daa = 0.f, dbb = 0.f, dab = 0.f;
  for_each_entry([&](int tm, int tn, int r, int lr, int lc) {
    if (g.above(lr, lc)) {
      const float a = as[tm][tn][r] - ca, bb = at[tm][tn][r] - cb;
      da += a;
      db += bb;
      daa = fmaf(a, a, daa);
      dbb = fmaf(bb, bb, dbb);
      dab = fmaf(a, bb, dab);
    }
  });
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

// out[q] = sum over the `count` partial K-tuples, fixed order: thread t takes partials t, t + 1024, ..., then a tree over the threads
template <int K>
__global__ __launch_bounds__(1024) void moments_finalize_kernel(const double* __restrict__ partials, int64_t count,
                                                                double* __restrict__ out) {
  __shared__ double red[K][1024];
  double m[K];
#pragma unroll
  for (int q = 0; q < K; ++q) m[q] = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 1024) {
#pragma unroll
    for (int q = 0; q < K; ++q) m[q] += partials[i * K + q];
  }
  block_tree_sum<1024>(m, red);
  if (threadIdx.x < K) out[threadIdx.x] = red[threadIdx.x][0];
}

inline int64_t vec_blocks(int64_t n) { return capped_blocks(n, 256, kVecBlocks); }


// ------------------------------------------------------------------------------------------------ kernel (RBF) CKA
// correlation.py:41-53, 70-75: K_ij = exp(-d_ij / (2 sigma^2)), d_ij = |x_i|^2 + |x_j|^2 - 2 <x_i, x_j>, sigma^2 = median of d (here: over
// the pairs i < j), CKA = HSIC(K, L) / sqrt(HSIC(K, K) HSIC(L, L)), HSIC = sum(HKH o HLH).  No N x N object and no list of the
// N (N-1) / 2 distances exists: every pass recomputes the Gram tiles on the fp32 MFMA.
//   median   exact radix select over the 31 value bits of d >= +0 (non-negative floats order like their bit patterns): three
//            histogram passes (11 + 11 + 9 bits) over the upper-triangle tiles, a one-workgroup scan between them that picks the bin and
//            the residual rank ON THE DEVICE.  An even pair count needs two order statistics, which may part ways in any pass: two
//            (prefix, rank) selections are carried, and two histograms once their prefixes differ.  Counts are 64-bit integers (integer
//            adds commute: the result does not depend on the order of arrival).
//   row sums one workgroup per (tile row, column chunk) over the FULL row (twice the Gram work of a triangle walk, but the workspace
//            is [chunks][2][N] doubles, not a 128-vector per tile); a row's 64 entries per wave are summed in fp32 by a butterfly, all
//            further sums are float64 in a fixed order.
//   HSIC     upper-triangle tiles again; each entry is centred BEFORE the products, Kc_ij = K_ij - a_i - a_j with
//            a_i = rowmean_i - mean / 2 (the raw form sum KL - (2/n) sum k_i l_i + k l / n^2 cancels); weight 2 above the diagonal, weight
//            1 and K_ii = 1 exactly on it; reduced like pair_moments_kernel.
// One definition of the device distance serves the median and the kernel passes.
constexpr int kHistBins = 2048;        // 11 bits; the last pass uses 512 of them
constexpr int kSelPasses = 3;
constexpr int kRowChunks = 16;         // upper bound of the column chunks of the row-sum pass
constexpr int kAggRounds = 4;

struct SelState {                      // the two order statistics in flight: value bits found so far, rank among the entries that share them
  unsigned long long rank[2];
  unsigned prefix[2];
};

__device__ __forceinline__ float sqdist(float ni, float nj, float g) {
  const float v = fmaf(-2.f, g, ni + nj);
  return v > 0.f ? v : 0.f;            // max(v, +0): -0 and NaN become +0, so the bit pattern is a valid bin index
}

// ++h[bin] for the active lanes.  Unit rows put almost every d into a dozen bins of the first pass, and tied distances put a whole
// wave on one bin in any pass: the lanes that share the first active lane's bin are counted with a ballot and added once, for up to
// kAggRounds distinct bins; what is left goes through one LDS atomic per lane.  Called by all 64 lanes together.
__device__ __forceinline__ void wave_hist_add(unsigned* h, unsigned bin, bool active, int lane) {
  unsigned long long todo = __ballot(active);
#pragma unroll 1
  for (int round = 0; round < kAggRounds && todo != 0ull; ++round) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned b = (unsigned)__shfl((int)bin, leader);
    const bool mine = active && bin == b;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(&h[b], (unsigned)__popcll(same));
    if (mine) active = false;
    todo &= ~same;
  }
  if (active) atomicAdd(&h[bin], 1u);
}

// One histogram pass of the radix select over d_ij, i < j.  PASS 0: bits 30..20 of every entry; PASS 1: bits 19..9 of the entries whose
// bits 30..20 equal a selection's prefix; PASS 2: bits 8..0 under a 22-bit prefix.  ghist: [2][kHistBins] of this pass, zeroed.
template <int PASS, bool VEC4>
__global__ __launch_bounds__(256) void sqdist_hist_kernel(const float* __restrict__ x, int64_t ld, int64_t P, int64_t N, int64_t T,
                                                          const float* __restrict__ norms, const SelState* __restrict__ st,
                                                          unsigned long long* __restrict__ ghist) {
  static_assert(TS::SMEM_FLOATS >= 2 * kHistBins + 2 * GB, "the histograms and the norms live in the mainloop's LDS");
  __shared__ __attribute__((aligned(16))) float smem[TS::SMEM_FLOATS];
  const int64_t b = blockIdx.x;
  int64_t ti, tj;
  tri_tile(b, T, ti, tj);
  const int64_t i0 = ti * GB, j0 = tj * GB;

  IdentityXf id;
  f32x16 acc[TS::TM][TS::TN];
  zero_acc(acc);
  mainloop<GB, GB, KMAJOR, KMAJOR, VEC4>(acc, x, ld, i0, N, x, ld, j0, N, 0, P, id, id, smem);
  // the mainloop's last barrier has passed: its LDS is free
  unsigned* lh = reinterpret_cast<unsigned*>(smem);
  float* nrow = smem + 2 * kHistBins;
  float* ncol = nrow + GB;
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < 2 * kHistBins; i += 256) lh[i] = 0u;
  if (tid < GB) nrow[tid] = i0 + tid < N ? norms[i0 + tid] : 0.f;
  else ncol[tid - GB] = j0 + (tid - GB) < N ? norms[j0 + (tid - GB)] : 0.f;
  __syncthreads();

  unsigned p0 = 0u, p1 = 0u;
  if (PASS > 0) {
    p0 = st->prefix[0];
    p1 = st->prefix[1];
  }
  const bool two = p1 != p0;
  constexpr int kBinShift = PASS == 0 ? 20 : (PASS == 1 ? 9 : 0);
  constexpr unsigned kBinMask = PASS == 2 ? 0x1ffu : 0x7ffu;
  constexpr int kTopShift = PASS == 1 ? 20 : 9;

  const int lane = egnn_lane();
  const PairGeom g(i0, j0, N);
  for_each_entry([&](int lc) { return ncol[lc]; }, [&](int tm, int tn, int r, int lr, int lc, float nj) {
    const bool valid = g.above(lr, lc);
    const unsigned bits = __float_as_uint(sqdist(nrow[lr], nj, acc[tm][tn][r]));
    const unsigned bin = (bits >> kBinShift) & kBinMask;
    if (PASS == 0) {
      wave_hist_add(lh, bin, valid, lane);
    } else {
      const unsigned top = bits >> kTopShift;
      wave_hist_add(lh, bin, valid && top == p0, lane);
      if (two) wave_hist_add(lh + kHistBins, bin, valid && top == p1, lane);
    }
  });
  __syncthreads();
  for (int i = tid; i < 2 * kHistBins; i += 256) {
    const unsigned c = lh[i];
    if (c != 0u) atomicAdd(&ghist[i], (unsigned long long)c);
  }
}

// Between two passes: the bin that holds each selection's rank, by an inclusive scan of the pass's histogram (one workgroup, 1024
// threads, two bins each).  PASS 0 starts the two selections from the pair count m (0-based ranks (m-1)/2 and m/2: equal when m is
// odd); PASS 2 has all 31 bits and writes out2 = (0.5 (d_lo + d_hi), m).
template <int PASS>
__global__ __launch_bounds__(1024) void select_scan_kernel(const unsigned long long* __restrict__ hist, SelState* __restrict__ st,
                                                           unsigned long long m, double* __restrict__ out2) {
  __shared__ unsigned long long cum[kHistBins];
  __shared__ unsigned found[2];
  constexpr int kBits = PASS == 2 ? 9 : 11;
  const int t = (int)threadIdx.x;
  unsigned prefix[2] = {0u, 0u};
  unsigned long long rank[2] = {(m - 1ull) / 2ull, m / 2ull};
  if (PASS > 0) {
    prefix[0] = st->prefix[0];
    prefix[1] = st->prefix[1];
    rank[0] = st->rank[0];
    rank[1] = st->rank[1];
  }
  const bool two = prefix[1] != prefix[0];
  if (t < 2) found[t] = 0u;
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {
    const unsigned long long* h = hist + ((two && s == 1) ? kHistBins : 0);
    cum[t] = h[t];
    cum[t + 1024] = h[t + 1024];
    __syncthreads();
    for (int off = 1; off < kHistBins; off <<= 1) {
      const unsigned long long a = t >= off ? cum[t - off] : 0ull;
      const unsigned long long c = cum[t + 1024 - off];
      __syncthreads();
      cum[t] += a;
      cum[t + 1024] += c;
      __syncthreads();
    }
#pragma unroll
    for (int e = t; e < kHistBins; e += 1024) {
      const unsigned long long incl = cum[e], excl = e > 0 ? cum[e - 1] : 0ull;
      if (excl <= rank[s] && rank[s] < incl) {
        const unsigned np = (prefix[s] << kBits) | (unsigned)e;
        st->prefix[s] = np;
        st->rank[s] = rank[s] - excl;
        found[s] = np;
      }
    }
    __syncthreads();
  }
  if (PASS == 2 && t == 0) {
    out2[0] = 0.5 * ((double)__uint_as_float(found[0]) + (double)__uint_as_float(found[1]));
    out2[1] = (double)m;
  }
}

// -log2(e) / (2 sigma^2): K = exp2(d * that).  A bandwidth that is not positive (all rows equal, or more than half of the pairs
// coincide) makes every K, and with it the result, NaN.
__device__ __forceinline__ double rbf_scale(double sigma2) {
  return sigma2 > 0.0 ? -1.4426950408889634 / (2.0 * sigma2) : __longlong_as_double(0x7ff8000000000000ll);
}

__device__ __forceinline__ float rbf_value(float d, double scale) { return __builtin_amdgcn_exp2f((float)((double)d * scale)); }

// Row sums of K (student) and L (teacher) over the full matrix.  Block (ti, c) walks the column tiles tj = c, c + C, ... of tile row
// ti and writes rowpart[c][q][i0 .. i0 + 127], q = 0 student, 1 teacher.  norms: [2][N].
template <bool VEC4>
__global__ __launch_bounds__(256) void rbf_rowsum_kernel(const float* __restrict__ xs, int64_t lds_, int64_t Ps,
                                                         const float* __restrict__ xt, int64_t ldt, int64_t Pt, int64_t N, int64_t T,
                                                         int C, const float* __restrict__ norms, const double* __restrict__ sigma2,
                                                         double* __restrict__ rowpart) {
  __shared__ __attribute__((aligned(16))) float smem[TS::SMEM_FLOATS];
  __shared__ double racc[2][2][GB];      // [wn][q][row]: each entry is owned by one lane of one wave
  __shared__ float nrow[2][GB], ncol[2][GB];
  const int64_t ti = blockIdx.x / C;
  const int c = (int)(blockIdx.x % C);
  const int64_t i0 = ti * GB;
  const int tid = (int)threadIdx.x;
  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  {
    const int q = tid >> 7, lr = tid & (GB - 1);
    nrow[q][lr] = i0 + lr < N ? norms[q * N + i0 + lr] : 0.f;
    racc[0][q][lr] = 0.0;
    racc[1][q][lr] = 0.0;
  }
  const double scale_s = rbf_scale(sigma2[0]), scale_t = rbf_scale(sigma2[1]);
#pragma unroll 1
  for (int64_t tj = c; tj < T; tj += C) {
    const int64_t j0 = tj * GB;
    {
      const int q = tid >> 7, lc = tid & (GB - 1);
      ncol[q][lc] = j0 + lc < N ? norms[q * N + j0 + lc] : 0.f;
    }
    f32x16 as[TS::TM][TS::TN], at[TS::TM][TS::TN];
    gram_pair<VEC4>(as, at, xs, lds_, Ps, xt, ldt, Pt, i0, j0, N, smem);
    const PairGeom g(i0, j0, N);           // any tile of the row: the diagonal entry of row lr is column lr - dj of this tile
#pragma unroll
    for (int tm = 0; tm < TS::TM; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = acc_row<GB, GB>(wm, tm, r, lane);
        float ss = 0.f, st = 0.f;
#pragma unroll
        for (int tn = 0; tn < TS::TN; ++tn) {
          const int lc = acc_col<GB, GB>(wn, tn, lane);
          if (g.in_cols(lc)) {
            const bool diag = g.diag(lr, lc);
            ss += diag ? 1.f : rbf_value(sqdist(nrow[0][lr], ncol[0][lc], as[tm][tn][r]), scale_s);
            st += diag ? 1.f : rbf_value(sqdist(nrow[1][lr], ncol[1][lc], at[tm][tn][r]), scale_t);
          }
        }
        // the 32 lanes of a half-wave hold the same row: 64 entries per sum
        ss = group_sum<32>(ss);
        st = group_sum<32>(st);
        if ((lane & 31) == 0) {
          racc[wn][0][lr] += (double)ss;
          racc[wn][1][lr] += (double)st;
        }
      }
    }
    __syncthreads();   // ncol is rewritten at the top of the next round
  }
  __syncthreads();
  {
    const int q = tid >> 7, lr = tid & (GB - 1);
    if (i0 + lr < N) rowpart[((int64_t)c * 2 + q) * N + i0 + lr] = racc[0][q][lr] + racc[1][q][lr];
  }
}

// mean[q][i] = (sum over the chunks, in order) / N, and per block the sum of its 256 means
__global__ __launch_bounds__(256) void rbf_rowmean_kernel(const double* __restrict__ rowpart, int C, int64_t N, double* __restrict__ mean,
                                                          double* __restrict__ blockpart) {
  __shared__ double red[4 * 2];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double m[2] = {0.0, 0.0};
  if (i < N) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += rowpart[((int64_t)c * 2 + q) * N + i];
      m[q] = s / (double)N;
      mean[q * N + i] = m[q];
    }
  }
  block_sum_f64(m, red);
  if (threadIdx.x == 0) {
    blockpart[(int64_t)blockIdx.x * 2] = m[0];
    blockpart[(int64_t)blockIdx.x * 2 + 1] = m[1];
  }
}

// partials[b] = (sum Kc Lc, sum Kc^2, sum Lc^2) of upper-triangle tile b, the strict upper part counted twice.  msum: the sums of
// the row means (their mean is the grand mean).
template <bool VEC4>
__global__ __launch_bounds__(256) void rbf_hsic_kernel(const float* __restrict__ xs, int64_t lds_, int64_t Ps,
                                                       const float* __restrict__ xt, int64_t ldt, int64_t Pt, int64_t N, int64_t T,
                                                       const float* __restrict__ norms, const double* __restrict__ sigma2,
                                                       const double* __restrict__ mean, const double* __restrict__ msum,
                                                       double* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float smem[TS::SMEM_FLOATS];
  __shared__ float nrow[2][GB], ncol[2][GB], arow[2][GB], acol[2][GB];
  const int64_t b = blockIdx.x;
  int64_t ti, tj;
  tri_tile(b, T, ti, tj);
  const int64_t i0 = ti * GB, j0 = tj * GB;
  const int tid = (int)threadIdx.x;
  {
    const int q = tid >> 7, l = tid & (GB - 1);
    const double half = 0.5 * msum[q] / (double)N;
    const bool rin = i0 + l < N, cin = j0 + l < N;
    nrow[q][l] = rin ? norms[q * N + i0 + l] : 0.f;
    ncol[q][l] = cin ? norms[q * N + j0 + l] : 0.f;
    arow[q][l] = rin ? (float)(mean[q * N + i0 + l] - half) : 0.f;
    acol[q][l] = cin ? (float)(mean[q * N + j0 + l] - half) : 0.f;
  }
  const double scale_s = rbf_scale(sigma2[0]), scale_t = rbf_scale(sigma2[1]);

  f32x16 as[TS::TM][TS::TN], at[TS::TM][TS::TN];
  gram_pair<VEC4>(as, at, xs, lds_, Ps, xt, ldt, Pt, i0, j0, N, smem);
  double* red = reinterpret_cast<double*>(smem);

  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const PairGeom g(i0, j0, N);
  float ukl = 0.f, ukk = 0.f, ull_ = 0.f, dkl = 0.f, dkk = 0.f, dll = 0.f;   // strictly above the diagonal / on it
#pragma unroll
  for (int tn = 0; tn < TS::TN; ++tn) {
    const int lc = acc_col<GB, GB>(wn, tn, lane);
    const float njs = ncol[0][lc], njt = ncol[1][lc], ajs = acol[0][lc], ajt = acol[1][lc];
#pragma unroll
    for (int tm = 0; tm < TS::TM; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = acc_row<GB, GB>(wm, tm, r, lane);
        if (g.on_or_above(lr, lc)) {
          const bool diag = g.diag(lr, lc);
          const float k = diag ? 1.f : rbf_value(sqdist(nrow[0][lr], njs, as[tm][tn][r]), scale_s);
          const float l = diag ? 1.f : rbf_value(sqdist(nrow[1][lr], njt, at[tm][tn][r]), scale_t);
          const float kc = (k - arow[0][lr]) - ajs, lcn = (l - arow[1][lr]) - ajt;
          if (diag) {
            dkl = fmaf(kc, lcn, dkl);
            dkk = fmaf(kc, kc, dkk);
            dll = fmaf(lcn, lcn, dll);
          } else {
            ukl = fmaf(kc, lcn, ukl);
            ukk = fmaf(kc, kc, ukk);
            ull_ = fmaf(lcn, lcn, ull_);
          }
        }
      }
    }
  }
  double m3[3] = {2.0 * (double)ukl + (double)dkl, 2.0 * (double)ukk + (double)dkk, 2.0 * (double)ull_ + (double)dll};
  block_sum_f64(m3, red);
  if (threadIdx.x == 0) {
    partials[b * 3] = m3[0];
    partials[b * 3 + 1] = m3[1];
    partials[b * 3 + 2] = m3[2];
  }
}

inline int row_chunks(int64_t N) {
  const int64_t T = (N + GB - 1) / GB;
  return (int)(T < kRowChunks ? T : kRowChunks);
}

inline size_t hist_bytes() { return (size_t)kSelPasses * 2 * kHistBins * sizeof(unsigned long long); }
inline size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

// doubles of the kernel-CKA workspace ahead of the fp32 norms: row-sum slabs, row means, their two sums, block and tile partials
struct CkaLayout {
  int64_t rowpart, mean, msum, blockpart, tilepart, norms, end_bytes;
  explicit CkaLayout(int64_t N) {
    const int64_t nb = (N + 255) / 256;
    rowpart = 0;
    mean = rowpart + (int64_t)row_chunks(N) * 2 * N;
    msum = mean + 2 * N;
    blockpart = msum + 2;
    tilepart = blockpart + 2 * nb;
    norms = tilepart + 3 * pair_tiles(N);
    end_bytes = norms * 8 + (int64_t)round8((size_t)(2 * N) * sizeof(float));
  }
};

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
  dispatch_vec4(vec4, [&](auto v4) {
    hipLaunchKernelGGL(pair_moments_kernel<v4.value>, dim3((unsigned)nblocks), dim3(256), 0, st, xs, ld_s, Ps, xt, ld_t, Pt, N, T, partials);
  });
  hipLaunchKernelGGL(moments_finalize_kernel<kMoments>, dim3(1), dim3(1024), 0, st, partials, nblocks, out6);
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
  hipLaunchKernelGGL(moments_finalize_kernel<kMoments>, dim3(1), dim3(1024), 0, st, partials, nb, out6);
  return egnn_launch_status();
}

extern "C" size_t egnn_sqdist_median_ws_bytes(int64_t N) {
  if (N < 1) return 0;
  return hist_bytes() + round8(sizeof(SelState)) + round8((size_t)N * sizeof(float));
}

extern "C" int egnn_sqdist_median_f32(const float* x, int64_t ld, int64_t P, int64_t N, double* out2, void* ws, size_t ws_bytes,
                                      void* stream) {
  EGNN_CHECK_ARG(N >= 2 && P > 0 && ld >= P);
  EGNN_CHECK_ARG(x && out2);
  if (ws_bytes < egnn_sqdist_median_ws_bytes(N)) return EGNN_EWORKSPACE;
  EGNN_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out2) & 7u) == 0);
  const int64_t T = (N + GB - 1) / GB;
  const int64_t nblocks = pair_tiles(N);
  if (nblocks > 0x7fffffffLL) return EGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* hist = static_cast<unsigned long long*>(ws);
  SelState* sel = reinterpret_cast<SelState*>(static_cast<char*>(ws) + hist_bytes());
  float* norms = reinterpret_cast<float*>(static_cast<char*>(ws) + hist_bytes() + round8(sizeof(SelState)));
  const unsigned long long m = (unsigned long long)N * (unsigned long long)(N - 1) / 2ull;
  if (hipMemsetAsync(ws, 0, hist_bytes() + round8(sizeof(SelState)), st) != hipSuccess) return egnn_launch_status();
  row_sqnorm(x, ld, P, N, norms, st);
  const bool vec4 = (ld % 4 == 0) && egnn_aligned16(x);
  dispatch_vec4(vec4, [&](auto v4) {
    auto pass = [&](auto p, unsigned long long* h) {   // h: this pass's [2][kHistBins]
      hipLaunchKernelGGL((sqdist_hist_kernel<p.value, decltype(v4)::value>), dim3((unsigned)nblocks), dim3(256), 0, st, x, ld, P, N, T, norms, sel, h);
      hipLaunchKernelGGL(select_scan_kernel<p.value>, dim3(1), dim3(1024), 0, st, h, sel, m, out2);
    };
    pass(std::integral_constant<int, 0>{}, hist);
    pass(std::integral_constant<int, 1>{}, hist + 2 * kHistBins);
    pass(std::integral_constant<int, 2>{}, hist + 4 * kHistBins);
  });
  return egnn_launch_status();
}

extern "C" size_t egnn_rbf_cka_ws_bytes(int64_t N) {
  if (N < 1) return 0;
  return (size_t)CkaLayout(N).end_bytes;
}

extern "C" int egnn_rbf_cka_f32(const float* xs, int64_t ld_s, int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt, int64_t N,
                                const double* sigma2_dev, double* out3, void* ws, size_t ws_bytes, void* stream) {
  EGNN_CHECK_ARG(N >= 2 && Ps > 0 && Pt > 0 && ld_s >= Ps && ld_t >= Pt);
  EGNN_CHECK_ARG(xs && xt && sigma2_dev && out3);
  if (ws_bytes < egnn_rbf_cka_ws_bytes(N)) return EGNN_EWORKSPACE;
  EGNN_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out3) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(sigma2_dev) & 7u) == 0);
  const int64_t T = (N + GB - 1) / GB;
  const int64_t nblocks = pair_tiles(N);
  if (nblocks > 0x7fffffffLL) return EGNN_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const CkaLayout lay(N);
  double* w = static_cast<double*>(ws);
  float* norms = reinterpret_cast<float*>(w + lay.norms);
  const int C = row_chunks(N);
  const int64_t nb = (N + 255) / 256;
  row_sqnorm(xs, ld_s, Ps, N, norms, st);
  row_sqnorm(xt, ld_t, Pt, N, norms + N, st);
  const bool vec4 = (ld_s % 4 == 0) && (ld_t % 4 == 0) && egnn_aligned16(xs) && egnn_aligned16(xt);
  const dim3 rgrid((unsigned)(T * C)), hgrid((unsigned)nblocks), block(256);
  dispatch_vec4(vec4, [&](auto v4) {
    hipLaunchKernelGGL(rbf_rowsum_kernel<v4.value>, rgrid, block, 0, st, xs, ld_s, Ps, xt, ld_t, Pt, N, T, C, norms, sigma2_dev, w + lay.rowpart);
    hipLaunchKernelGGL(rbf_rowmean_kernel, dim3((unsigned)nb), dim3(256), 0, st, w + lay.rowpart, C, N, w + lay.mean, w + lay.blockpart);
    hipLaunchKernelGGL(moments_finalize_kernel<2>, dim3(1), dim3(1024), 0, st, w + lay.blockpart, nb, w + lay.msum);
    hipLaunchKernelGGL(rbf_hsic_kernel<v4.value>, hgrid, block, 0, st, xs, ld_s, Ps, xt, ld_t, Pt, N, T, norms, sigma2_dev, w + lay.mean, w + lay.msum, w + lay.tilepart);
  });
  hipLaunchKernelGGL(moments_finalize_kernel<3>, dim3(1), dim3(1024), 0, st, w + lay.tilepart, nblocks, out3);
  return egnn_launch_status();
}
