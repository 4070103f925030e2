// FitNet and attention-transfer losses as row kernels (wave64 per row, fixed-order reductions; HBM / latency-bound).
//   fitnet : /root/reference/arxiv_pyg/criterion.py:24-36   loss = mse(F.normalize(f), F.normalize(t))      (mean over n * D)
//   at     : /root/reference/arxiv_pyg/criterion.py:39-54   e_s[i] = sum_d f_id^2, e_t likewise;
//                                                           loss = mse(F.normalize(e_s), F.normalize(e_t))  (norm ACROSS nodes)
// F.normalize(x) = x / max(||x||_2, eps), eps = 1e-12: where the clamp is active the denominator is a constant.
#include "common.h"
#include "block_reduce.h"

namespace {

using namespace egnn_reduce;

constexpr int kFlBlocks = 1024;   // partial sums per launch (fixed => deterministic finalize)

// ---- FitNet --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fitnet_fwd_kernel(const float* __restrict__ f, int64_t ldf, const float* __restrict__ t, int64_t ldt,
                                                         int64_t n, int64_t D, float eps, float* __restrict__ partials) {
  __shared__ float sh[4];
  const int lane = egnn_lane(), wave = egnn_wave_id();
  float acc = 0.f;
  for (int64_t row = blockIdx.x * 4LL + wave; row < n; row += (int64_t)gridDim.x * 4) {
    const float* fp = f + row * ldf;
    const float* tp = t + row * ldt;
    float ff = 0.f, tt = 0.f;
    for (int64_t d = lane; d < D; d += 64) { ff = fmaf(fp[d], fp[d], ff); tt = fmaf(tp[d], tp[d], tt); }
    ff = egnn_wave_sum(ff); tt = egnn_wave_sum(tt);
    const float inf_ = 1.f / fmaxf(sqrtf(ff), eps), int_ = 1.f / fmaxf(sqrtf(tt), eps);
    float s = 0.f;
    for (int64_t d = lane; d < D; d += 64) { const float u = fp[d] * inf_ - tp[d] * int_; s = fmaf(u, u, s); }
    acc += egnn_wave_sum(s);
  }
  const float tot = waves4_sum<PAIRWISE>(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// df = c / |f| (d - f^ (f^ . d)),  dt = -c / |t| (d - t^ (t^ . d)),  d = f^ - t^,  c = 2 g / (n D); the projection term is
// dropped where the norm clamp is active
__global__ __launch_bounds__(256) void fitnet_bwd_kernel(const float* __restrict__ f, int64_t ldf, const float* __restrict__ t, int64_t ldt,
                                                         int64_t n, int64_t D, float eps, const float* __restrict__ g, float* __restrict__ df,
                                                         int64_t lddf, float* __restrict__ dt, int64_t lddt) {
  const int lane = egnn_lane();
  const int64_t row = blockIdx.x * 4LL + egnn_wave_id();
  if (row >= n) return;
  const float* fp = f + row * ldf;
  const float* tp = t + row * ldt;
  float ff = 0.f, tt = 0.f;
  for (int64_t d = lane; d < D; d += 64) { ff = fmaf(fp[d], fp[d], ff); tt = fmaf(tp[d], tp[d], tt); }
  ff = egnn_wave_sum(ff); tt = egnn_wave_sum(tt);
  const float nf = sqrtf(ff), nt = sqrtf(tt);
  const float inf_ = 1.f / fmaxf(nf, eps), int_ = 1.f / fmaxf(nt, eps);
  float fd = 0.f, td = 0.f;   // f^ . d and t^ . d
  for (int64_t d = lane; d < D; d += 64) {
    const float a = fp[d] * inf_, b = tp[d] * int_, u = a - b;
    fd = fmaf(a, u, fd); td = fmaf(b, u, td);
  }
  fd = egnn_wave_sum(fd); td = egnn_wave_sum(td);
  if (nf <= eps) fd = 0.f;
  if (nt <= eps) td = 0.f;
  const float c = 2.f * g[0] / ((float)n * (float)D);
  for (int64_t d = lane; d < D; d += 64) {
    const float a = fp[d] * inf_, b = tp[d] * int_, u = a - b;
    if (df) df[row * lddf + d] = c * inf_ * (u - a * fd);
    if (dt) dt[row * lddt + d] = -c * int_ * (u - b * td);
  }
}

// ---- attention transfer ------------------------------------------------------------------------------------------
// pass 1: row energies of both sides + per-block partials of sum e^2
__global__ __launch_bounds__(256) void at_energy_kernel(const float* __restrict__ f, int64_t ldf, int64_t Df, const float* __restrict__ t, int64_t ldt,
                                                        int64_t Dt, int64_t n, float* __restrict__ es, float* __restrict__ et,
                                                        float* __restrict__ partials) {
  __shared__ float sh[4];
  const int lane = egnn_lane(), wave = egnn_wave_id();
  float a2 = 0.f, b2 = 0.f;
  for (int64_t row = blockIdx.x * 4LL + wave; row < n; row += (int64_t)gridDim.x * 4) {
    const float* fp = f + row * ldf;
    const float* tp = t + row * ldt;
    float a = 0.f, b = 0.f;
    for (int64_t d = lane; d < Df; d += 64) a = fmaf(fp[d], fp[d], a);
    for (int64_t d = lane; d < Dt; d += 64) b = fmaf(tp[d], tp[d], b);
    a = egnn_wave_sum(a); b = egnn_wave_sum(b);
    if (lane == 0) { es[row] = a; et[row] = b; }
    a2 = fmaf(a, a, a2); b2 = fmaf(b, b, b2);
  }
  const float ta = waves4_sum<PAIRWISE>(a2, sh), tb = waves4_sum<PAIRWISE>(b2, sh);
  if (threadIdx.x == 0) { partials[blockIdx.x] = ta; partials[kFlBlocks + blockIdx.x] = tb; }
}

// pass 2 (one block): norms; then sum d^2, sum d e_s, sum d e_t with d = e_s / ns - e_t / nt.  scal = {ns, nt, sum d e_s, sum d e_t, raw |e_s|, raw |e_t|}
__global__ __launch_bounds__(1024) void at_finish_kernel(const float* __restrict__ es, const float* __restrict__ et, int64_t n, int nb,
                                                         const float* __restrict__ partials, float eps, float* __restrict__ scal,
                                                         float* __restrict__ loss) {
  __shared__ float red[3][1024];
  float ab[2] = {0.f, 0.f};
  for (int i = threadIdx.x; i < nb; i += 1024) { ab[0] += partials[i]; ab[1] += partials[kFlBlocks + i]; }
  block_tree_sum<1024>(ab, red);
  const float raw_s = sqrtf(red[0][0]), raw_t = sqrtf(red[1][0]);
  const float ns = fmaxf(raw_s, eps), nt = fmaxf(raw_t, eps);
  __syncthreads();
  float m[3] = {0.f, 0.f, 0.f};   // sum d^2, sum d e_s, sum d e_t
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    const float d = es[i] / ns - et[i] / nt;
    m[0] = fmaf(d, d, m[0]); m[1] = fmaf(d, es[i], m[1]); m[2] = fmaf(d, et[i], m[2]);
  }
  block_tree_sum<1024>(m, red);
  if (threadIdx.x == 0) {
    loss[0] = red[0][0] / (float)n;
    scal[0] = ns; scal[1] = nt; scal[2] = red[1][0]; scal[3] = red[2][0]; scal[4] = raw_s; scal[5] = raw_t;
  }
}

// dL/de_s[i] = 2/n (d_i / ns - [|e_s| > eps] e_s[i] (sum_j d_j e_s[j]) / ns^3), dL/de_t[i] = -2/n (d_i / nt - ...);  df_i = g dL/de_s[i] 2 f_i
__global__ __launch_bounds__(256) void at_bwd_kernel(const float* __restrict__ f, int64_t ldf, int64_t Df, const float* __restrict__ t, int64_t ldt,
                                                     int64_t Dt, int64_t n, const float* __restrict__ es, const float* __restrict__ et,
                                                     const float* __restrict__ scal, float eps, const float* __restrict__ g,
                                                     float* __restrict__ df, int64_t lddf, float* __restrict__ dt, int64_t lddt) {
  const int lane = egnn_lane();
  const int64_t row = blockIdx.x * 4LL + egnn_wave_id();
  if (row >= n) return;
  const float ns = scal[0], nt = scal[1];
  const float d = es[row] / ns - et[row] / nt;
  const float ps = scal[4] > eps ? es[row] * scal[2] / (ns * ns * ns) : 0.f;
  const float pt = scal[5] > eps ? et[row] * scal[3] / (nt * nt * nt) : 0.f;
  const float c = 2.f * g[0] / (float)n;
  const float ges = c * (d / ns - ps), get = -c * (d / nt - pt);
  if (df) for (int64_t k = lane; k < Df; k += 64) df[row * lddf + k] = 2.f * ges * f[row * ldf + k];
  if (dt) for (int64_t k = lane; k < Dt; k += 64) dt[row * lddt + k] = 2.f * get * t[row * ldt + k];
}

// ---- attention transfer on node-range shards: the same three steps cut where the ranks' sums meet ---------------------------------
// The host all-reduces sumsq (2 floats) between energy and partial and sums (3 floats) between partial and the backward; nothing else
// crosses ranks.  d_i stays in the direct form e_s[i]/ns - e_t[i]/nt: one all-reduce of the moments {sum e_s^2, sum e_t^2, sum e_s e_t}
// would do, but that closed form cancels (tens of per cent off at e_s ~ k e_t in fp32, the direct form below 1e-5).
constexpr int kAtPartBlocks = 512;   // 3 partial arrays of the second step fit the 2 kFlBlocks floats the first one uses

// this rank's partials of sum d^2, sum d e_s, sum d e_t under the GLOBAL norms; scal = {ns, nt, raw |e_s|, raw |e_t|}
__global__ __launch_bounds__(256) void at_partial_kernel(const float* __restrict__ es, const float* __restrict__ et, int64_t n,
                                                         const float* __restrict__ sumsq_global, float eps, float* __restrict__ scal,
                                                         float* __restrict__ partials) {
  __shared__ float red[3][256];
  const float raw_s = sqrtf(sumsq_global[0]), raw_t = sqrtf(sumsq_global[1]);
  const float ns = fmaxf(raw_s, eps), nt = fmaxf(raw_t, eps);
  float m[3] = {0.f, 0.f, 0.f};   // sum d^2, sum d e_s, sum d e_t
  for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = es[i] / ns - et[i] / nt;
    m[0] = fmaf(d, d, m[0]); m[1] = fmaf(d, es[i], m[1]); m[2] = fmaf(d, et[i], m[2]);
  }
  block_tree_sum<256>(m, red);
  if (threadIdx.x == 0) {
    for (int q = 0; q < 3; ++q) partials[q * kAtPartBlocks + blockIdx.x] = red[q][0];
    if (blockIdx.x == 0) { scal[0] = ns; scal[1] = nt; scal[2] = raw_s; scal[3] = raw_t; }
  }
}

// at_bwd_kernel for a row block of a larger problem: c = 2 g / n_global, the dot products sums = {sum d^2, sum d e_s, sum d e_t} over ALL
// ranks' rows, the projection term dropped where the GLOBAL raw norm is <= eps
__global__ __launch_bounds__(256) void at_bwd_rows_kernel(const float* __restrict__ f, int64_t ldf, int64_t Df, const float* __restrict__ t,
                                                          int64_t ldt, int64_t Dt, int64_t n, int64_t n_global, const float* __restrict__ es,
                                                          const float* __restrict__ et, const float* __restrict__ scal,
                                                          const float* __restrict__ sums, float eps, const float* __restrict__ g,
                                                          float* __restrict__ df, int64_t lddf, float* __restrict__ dt, int64_t lddt) {
  const int lane = egnn_lane();
  const int64_t row = blockIdx.x * 4LL + egnn_wave_id();
  if (row >= n) return;
  const float ns = scal[0], nt = scal[1];
  const float d = es[row] / ns - et[row] / nt;
  const float ps = scal[2] > eps ? es[row] * sums[1] / (ns * ns * ns) : 0.f;
  const float pt = scal[3] > eps ? et[row] * sums[2] / (nt * nt * nt) : 0.f;
  const float c = 2.f * g[0] / (float)n_global;
  const float ges = c * (d / ns - ps), get = -c * (d / nt - pt);
  if (df) for (int64_t k = lane; k < Df; k += 64) df[row * lddf + k] = 2.f * ges * f[row * ldf + k];
  if (dt) for (int64_t k = lane; k < Dt; k += 64) dt[row * lddt + k] = 2.f * get * t[row * ldt + k];
}

}  // namespace

extern "C" size_t egnn_feature_loss_ws_floats(int64_t n) { return 2 * (size_t)kFlBlocks + 2 * (size_t)(n > 0 ? n : 0) + 8; }

extern "C" int egnn_fitnet_fwd_f32(const float* f, int64_t ldf, const float* t, int64_t ldt, int64_t n, int64_t D, float eps, float* loss,
                                   float* ws, size_t ws_floats, void* stream) {
  EGNN_CHECK_ARG(n > 0 && D > 0 && f && t && loss && ws && ldf >= D && ldt >= D && eps > 0.f);
  if (ws_floats < egnn_feature_loss_ws_floats(n)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)capped_blocks(n, 4, kFlBlocks);
  hipLaunchKernelGGL(fitnet_fwd_kernel, dim3(nb), dim3(256), 0, st, f, ldf, t, ldt, n, D, eps, ws);
  hipLaunchKernelGGL((sum_partials_kernel<256, float>), dim3(1), dim3(256), 0, st, ws, 0, nb, 1.f / ((float)n * (float)D), loss);
  return egnn_launch_status();
}

extern "C" int egnn_fitnet_bwd_f32(const float* f, int64_t ldf, const float* t, int64_t ldt, int64_t n, int64_t D, float eps, const float* g,
                                   float* df, int64_t lddf, float* dt, int64_t lddt, void* stream) {
  EGNN_CHECK_ARG(n > 0 && D > 0 && f && t && g && ldf >= D && ldt >= D && (df == nullptr || lddf >= D) && (dt == nullptr || lddt >= D));
  hipLaunchKernelGGL(fitnet_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, f, ldf, t, ldt, n, D, eps, g, df, lddf,
                     dt, lddt);
  return egnn_launch_status();
}

// ws layout: [2 kFlBlocks partials][e_s n][e_t n][scal 8]; e_s / e_t / scal are what the backward reads (keep ws alive until then)
extern "C" int egnn_at_fwd_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, float eps,
                               float* loss, float* ws, size_t ws_floats, void* stream) {
  EGNN_CHECK_ARG(n > 0 && Df > 0 && Dt > 0 && f && t && loss && ws && ldf >= Df && ldt >= Dt && eps > 0.f);
  if (ws_floats < egnn_feature_loss_ws_floats(n)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* es = ws + 2 * kFlBlocks;
  float* et = es + n;
  float* scal = et + n;
  const int nb = (int)capped_blocks(n, 4, kFlBlocks);
  hipLaunchKernelGGL(at_energy_kernel, dim3(nb), dim3(256), 0, st, f, ldf, Df, t, ldt, Dt, n, es, et, ws);
  hipLaunchKernelGGL(at_finish_kernel, dim3(1), dim3(1024), 0, st, es, et, n, nb, ws, eps, scal, loss);
  return egnn_launch_status();
}

extern "C" int egnn_at_bwd_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, float eps,
                               const float* ws, const float* g, float* df, int64_t lddf, float* dt, int64_t lddt, void* stream) {
  EGNN_CHECK_ARG(n > 0 && Df > 0 && Dt > 0 && f && t && ws && g && (df == nullptr || lddf >= Df) && (dt == nullptr || lddt >= Dt));
  const float* es = ws + 2 * kFlBlocks;
  const float* et = es + n;
  const float* scal = et + n;
  hipLaunchKernelGGL(at_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, f, ldf, Df, t, ldt, Dt, n, es, et, scal, eps, g,
                     df, lddf, dt, lddt);
  return egnn_launch_status();
}

// ---- the split form (node-range shards).  ws of the two forward steps: egnn_feature_loss_ws_floats(n) floats, partials only (free after the call)
extern "C" int egnn_at_energy_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, float* es,
                                  float* et, float* sumsq, float* ws, size_t ws_floats, void* stream) {
  EGNN_CHECK_ARG(n > 0 && Df > 0 && Dt > 0 && f && t && es && et && sumsq && ws && ldf >= Df && ldt >= Dt);
  if (ws_floats < egnn_feature_loss_ws_floats(n)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)capped_blocks(n, 4, kFlBlocks);
  hipLaunchKernelGGL(at_energy_kernel, dim3(nb), dim3(256), 0, st, f, ldf, Df, t, ldt, Dt, n, es, et, ws);
  hipLaunchKernelGGL((sum_partials_kernel<256, float>), dim3(2), dim3(256), 0, st, ws, kFlBlocks, nb, 1.f, sumsq);
  return egnn_launch_status();
}

extern "C" int egnn_at_partial_f32(const float* es, const float* et, int64_t n, const float* sumsq_global, float eps, float* scal, float* sums,
                                   float* ws, size_t ws_floats, void* stream) {
  EGNN_CHECK_ARG(n > 0 && es && et && sumsq_global && scal && sums && ws && eps > 0.f);
  static_assert(3 * kAtPartBlocks <= 2 * kFlBlocks, "the partials of at_partial_kernel must fit egnn_feature_loss_ws_floats");
  if (ws_floats < egnn_feature_loss_ws_floats(n)) return EGNN_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)capped_blocks(n, 256, kAtPartBlocks);
  hipLaunchKernelGGL(at_partial_kernel, dim3(nb), dim3(256), 0, st, es, et, n, sumsq_global, eps, scal, ws);
  hipLaunchKernelGGL((sum_partials_kernel<256, float>), dim3(3), dim3(256), 0, st, ws, kAtPartBlocks, nb, 1.f, sums);
  return egnn_launch_status();
}

extern "C" int egnn_at_bwd_rows_f32(const float* f, int64_t ldf, int64_t Df, const float* t, int64_t ldt, int64_t Dt, int64_t n, int64_t n_global,
                                    const float* es, const float* et, const float* scal, const float* sums_global, float eps, const float* g,
                                    float* df, int64_t lddf, float* dt, int64_t lddt, void* stream) {
  EGNN_CHECK_ARG(n > 0 && n_global >= n && Df > 0 && Dt > 0 && f && t && es && et && scal && sums_global && g && ldf >= Df && ldt >= Dt &&
                 (df == nullptr || lddf >= Df) && (dt == nullptr || lddt >= Dt));
  hipLaunchKernelGGL(at_bwd_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, f, ldf, Df, t, ldt, Dt, n, n_global,
                     es, et, scal, sums_global, eps, g, df, lddf, dt, lddt);
  return egnn_launch_status();
}
