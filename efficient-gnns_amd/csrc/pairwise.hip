// GSP all-pairs similarity loss (/root/reference/arxiv_pyg/criterion.py:57-92) and the PPI BCE pair
// (/root/reference/ppi_pyg/criterion.py:8-18) for gfx950.
//
// GSP:  loss = mean_ij (k(xs_i, xs_j) - k(xt_i, xt_j))^2 over S sampled rows.
//   cosine / poly : rows are unit vectors (the caller normalises), k = <a,b> or <a,b>^2
//   l2 / rbf      : k = ||a-b|| or exp(-||a-b||^2 / 2), through ||a||^2 + ||b||^2 - 2<a,b> -- the
//                   reference materialises the [S,S,D] difference tensor (criterion.py:80-84), here no
//                   S x S x D object exists and the diagonal distance is exactly 0.
// Forward: one workgroup per 128 x 128 tile runs the fp32-MFMA mainloop twice (student Gram, teacher
// Gram), then an in-register epilogue forms D = k_s - k_t, accumulates sum D^2 and writes the two
// gradient weight matrices Ws, Wt so that the backward is
//      dXs = g * (Ws Xs - rowsum(Ws) o Xs) ,  dXt = g * (Wt Xt - rowsum(Wt) o Xt)
// (the rowsum term only for the distance kernels): one MFMA GEMM each (egnn_gemm_f32) plus the
// row kernels below.  All reductions have a fixed order.
#include "pair_tile.h"
#include "block_reduce.h"

using namespace egnn_pair;
using namespace egnn_reduce;

namespace {

enum { K_COSINE = 0, K_POLY = 1, K_L2 = 2, K_RBF = 3 };

// similarity value and d(sim)/d(gram-like argument) pieces for one pair
struct PairK {
  float k;   // kernel value
  float w;   // W_ij = c * D_ij * w :  cosine 1 | poly 2<a,b> | l2 -1/||a-b|| | rbf k
};

__device__ __forceinline__ PairK pair_kernel(int kernel, float dot, float ni, float nj, bool diag) {
  PairK r;
  if (kernel == K_COSINE) { r.k = dot; r.w = 1.f; }
  else if (kernel == K_POLY) { r.k = dot * dot; r.w = 2.f * dot; }
  else {
    float d2 = diag ? 0.f : fmaxf(ni + nj - 2.f * dot, 0.f);
    if (kernel == K_L2) { r.k = sqrtf(d2); r.w = r.k > 0.f ? -1.f / r.k : 0.f; }
    else { r.k = expf(-0.5f * d2); r.w = r.k; }
  }
  return r;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void gsp_fwd_kernel(const float* __restrict__ xs, int64_t lds_, int64_t Ps,
                                                      const float* __restrict__ xt, int64_t ldt, int64_t Pt, int64_t S,
                                                      int kernel, const float* __restrict__ ns, const float* __restrict__ nt,
                                                      float coef, float* __restrict__ Ws, float* __restrict__ Wt,
                                                      float* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float smem[TS::SMEM_FLOATS];
  const int64_t tiles = (S + GB - 1) / GB;
  const int64_t i0 = (blockIdx.x / tiles) * GB;
  const int64_t j0 = (blockIdx.x % tiles) * GB;
  f32x16 as[TS::TM][TS::TN], at[TS::TM][TS::TN];
  gram_pair<VEC4>(as, at, xs, lds_, Ps, xt, ldt, Pt, i0, j0, S, smem);
  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
  const int wm = wave >> 1, wn = wave & 1;
  const bool dist = kernel >= K_L2;
  float local[1] = {0.f};
#pragma unroll
  for (int tn = 0; tn < TS::TN; ++tn) {
    const int64_t c = j0 + acc_col<GB, GB>(wn, tn, lane);
    const float nsj = (dist && c < S) ? ns[c] : 0.f;
    const float ntj = (dist && c < S) ? nt[c] : 0.f;
#pragma unroll
    for (int tm = 0; tm < TS::TM; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = i0 + acc_row<GB, GB>(wm, tm, r, lane);
        if (row < S && c < S) {
          const float nsi = dist ? ns[row] : 0.f;
          const float nti = dist ? nt[row] : 0.f;
          const PairK ks = pair_kernel(kernel, as[tm][tn][r], nsi, nsj, row == c);
          const PairK kt = pair_kernel(kernel, at[tm][tn][r], nti, ntj, row == c);
          const float d = ks.k - kt.k;
          local[0] = fmaf(d, d, local[0]);
          // dXs = Ws Xs (- rowsum(Ws) o Xs for l2/rbf), dXt likewise: Ws = c D w_s, Wt = -c D w_t
          Ws[row * S + c] = coef * d * ks.w;
          Wt[row * S + c] = -coef * d * kt.w;
        }
      }
    }
  }
  // block reduction in a fixed order
  float (*red)[256] = reinterpret_cast<float (*)[256]>(smem);
  block_tree_sum<256>(local, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0][0];
}

__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ W, int64_t ld, int64_t n, int64_t m,
                                                     float* __restrict__ out) {
  const int lane = egnn_lane();
  const int64_t row = blockIdx.x * 4LL + egnn_wave_id();
  if (row >= n) return;
  float s = 0.f;
  for (int64_t j = lane; j < m; j += 64) s += W[row * ld + j];
  s = egnn_wave_sum(s);
  if (lane == 0) out[row] = s;
}

// out[i,:] = g * (WX[i,:] - r[i] * X[i,:])
__global__ __launch_bounds__(256) void scale_rowcorr_kernel(const float* __restrict__ WX, int64_t ldw, const float* __restrict__ X,
                                                            int64_t ldx, const float* __restrict__ r, const float* __restrict__ g,
                                                            int64_t n, int64_t P, float* __restrict__ out, int64_t ldo) {
  const float gs = g ? g[0] : 1.f;
  const int64_t total = n * P;
  for (int64_t t = blockIdx.x * 256LL + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t i = t / P, p = t % P;
    float v = WX[i * ldw + p];
    if (r) v -= r[i] * X[i * ldx + p];
    out[i * ldo + p] = gs * v;
  }
}

// ---- BCE-with-logits pair (PPI logit KD) ----------------------------------------------------------
constexpr int kBceBlocks = 1024;

__device__ __forceinline__ float bce_logits(float x, float y) {
  return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(256) void bce_pair_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ t, int64_t total,
                                                           float* __restrict__ partials) {
  __shared__ float red[2][256];
  float ab[2] = {0.f, 0.f};
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    ab[0] += bce_logits(x[i], y[i]);
    ab[1] += bce_logits(x[i], sigmoidf_(t[i]));
  }
  block_tree_sum<256>(ab, red);
  if (threadIdx.x == 0) { partials[blockIdx.x] = red[0][0]; partials[kBceBlocks + blockIdx.x] = red[1][0]; }
}

__global__ __launch_bounds__(256) void bce_pair_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ t, int64_t total,
                                                           const float* __restrict__ g_cls, const float* __restrict__ g_kd,
                                                           float* __restrict__ dx) {
  const float gc = g_cls ? g_cls[0] / (float)total : 0.f;
  const float gk = g_kd ? g_kd[0] / (float)total : 0.f;
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float s = sigmoidf_(x[i]);
    dx[i] = gc * (s - y[i]) + gk * (s - sigmoidf_(t[i]));
  }
}

}  // namespace

extern "C" size_t egnn_gsp_ws_floats(int64_t S) {
  const int64_t tiles = (S + GB - 1) / GB;
  return (size_t)(2 * S + tiles * tiles);
}

extern "C" int egnn_gsp_fwd_f32(const float* xs, int64_t ld_s, int64_t Ps, const float* xt, int64_t ld_t, int64_t Pt,
                                int64_t S, int kernel, float* Ws, float* Wt, float* loss, float* ws, size_t ws_floats,
                                void* stream) {
  EGNN_CHECK_ARG(S > 0 && Ps > 0 && Pt > 0 && ld_s >= Ps && ld_t >= Pt && kernel >= 0 && kernel <= 3);
  EGNN_CHECK_ARG(xs && xt && Ws && Wt && loss && ws);
  if (ws_floats < egnn_gsp_ws_floats(S)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* ns = ws;
  float* nt = ws + S;
  float* partials = ws + 2 * S;
  if (kernel >= K_L2) {
    row_sqnorm(xs, ld_s, Ps, S, ns, st);
    row_sqnorm(xt, ld_t, Pt, S, nt, st);
  }
  const int64_t tiles = (S + GB - 1) / GB;
  const int64_t nblocks = tiles * tiles;
  if (nblocks > 0x7fffffffLL) return EGNN_EINVAL;
  // dL/dk = 2 D / S^2; each unordered pair enters twice (k_ij and k_ji) => 4 / S^2
  const float coef = 4.f / ((float)S * (float)S);
  const bool vec4 = (ld_s % 4 == 0) && (ld_t % 4 == 0) && egnn_aligned16(xs) && egnn_aligned16(xt);
  dispatch_vec4(vec4, [&](auto v4) {
    hipLaunchKernelGGL(gsp_fwd_kernel<v4.value>, dim3((unsigned)nblocks), dim3(256), 0, st, xs, ld_s, Ps, xt, ld_t, Pt, S, kernel, ns, nt, coef, Ws, Wt, partials);
  });
  hipLaunchKernelGGL((sum_partials_kernel<1024, float>), dim3(1), dim3(1024), 0, st, partials, 0, nblocks, 1.f / ((float)S * (float)S), loss);
  return egnn_launch_status();
}

extern "C" int egnn_rowsum_f32(const float* W, int64_t ld, int64_t n, int64_t m, float* out, void* stream) {
  EGNN_CHECK_ARG(n >= 0 && m >= 0 && ld >= m);
  if (n == 0) return EGNN_OK;
  EGNN_CHECK_ARG(W && out);
  hipLaunchKernelGGL(rowsum_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, W, ld, n, m, out);
  return egnn_launch_status();
}

extern "C" int egnn_scale_rowcorr_f32(const float* WX, int64_t ldw, const float* X, int64_t ldx, const float* r,
                                      const float* g, int64_t n, int64_t P, float* out, int64_t ldo, void* stream) {
  EGNN_CHECK_ARG(n >= 0 && P >= 0 && ldw >= P && ldo >= P && (r == nullptr || (X != nullptr && ldx >= P)));
  if (n == 0 || P == 0) return EGNN_OK;
  EGNN_CHECK_ARG(WX && out);
  const int64_t blocks = (n * P + 255) / 256;
  hipLaunchKernelGGL(scale_rowcorr_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     WX, ldw, X, ldx, r, g, n, P, out, ldo);
  return egnn_launch_status();
}

extern "C" size_t egnn_bce_pair_ws_floats(void) { return 2 * (size_t)kBceBlocks; }

extern "C" int egnn_bce_pair_fwd_f32(const float* logits, const float* labels, const float* teacher, int64_t total,
                                     float* out2, float* ws, void* stream) {
  EGNN_CHECK_ARG(total > 0 && logits && labels && teacher && out2 && ws);
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)capped_blocks(total, 256, kBceBlocks);
  hipLaunchKernelGGL(bce_pair_fwd_kernel, dim3(nb), dim3(256), 0, st, logits, labels, teacher, total, ws);
  hipLaunchKernelGGL((sum_partials_kernel<1024, float>), dim3(1), dim3(1024), 0, st, ws, 0, nb, 1.f / (float)total, out2);
  hipLaunchKernelGGL((sum_partials_kernel<1024, float>), dim3(1), dim3(1024), 0, st, ws + kBceBlocks, 0, nb, 1.f / (float)total, out2 + 1);
  return egnn_launch_status();
}

extern "C" int egnn_bce_pair_bwd_f32(const float* logits, const float* labels, const float* teacher, int64_t total,
                                     const float* g_cls, const float* g_kd, float* dlogits, void* stream) {
  EGNN_CHECK_ARG(total > 0 && logits && labels && teacher && dlogits);
  hipLaunchKernelGGL(bce_pair_bwd_kernel, dim3((unsigned)capped_blocks(total, 256, 4096)), dim3(256), 0, (hipStream_t)stream, logits,
                     labels, teacher, total, g_cls, g_kd, dlogits);
  return egnn_launch_status();
}
