// Backward of the GAT attention + aggregation of one PyG <=1.7 GATConv (/root/reference/ppi_pyg/gnn.py:50-83,23-47: the PPI
// student and teacher train through it) for gfx950.  Forward (edge_softmax.hip / spmm.hip), per head h, CSR by target i:
//   s_e = leaky_relu(a_src[col e, h] + a_dst[i, h]);  att[h,e] = softmax_row(s);  out[i,h,:] = sum_e att[h,e] m[h,e] xl[col e,h,:]
// with m the optional attention-dropout multiplier (mask / (1 - p)).  With go = d out (per head; g_out / H for averaged heads):
//   g_e       = m_e <go[i,h,:], xl[col e,h,:]>                 (SDDMM over the gathered source rows)
//   d_raw_e   = att_e (g_e - sum_row att g) * (s_e > 0 ? 1 : slope)
//   d_a_dst   = sum_row d_raw;     d_a_src[j] = sum_{e: col e = j} d_raw_e
//   dxl[j,h,:] = sum_{e: col e = j} att_e m_e go[row e,h,:] + d_a_src[j,h] att_l[h,:] + d_a_dst[j,h] att_r[h,:]
//   d_att_l[h,:] = sum_j xl[j,h,:] d_a_src[j,h];   d_att_r likewise with d_a_dst
// Three launches for all heads: the target-side kernel (one wavefront per target row), the source-side kernel over the transposed
// structure (one wavefront per source row, no H permuted value copies, per-block partials of d_att_l / d_att_r in LDS) and a
// fixed-order finalize.  No atomics: every sum has a fixed order, so two backward passes are bit-equal.
#include "common.h"

namespace {

constexpr int kGatBwdBlocks = 1024;   // grid cap of the source-side kernel = row count of the d_att partials
constexpr int64_t kGatMaxHC = 2048;   // 4 waves x 2 H*C floats of LDS accumulators (64 KiB)

// <go_row[0:C], xr[0:C]> reduced over the wave (every lane holds the sum)
template <bool VEC4>
__device__ __forceinline__ float wave_dot(const float* __restrict__ a, const float* __restrict__ b, int C, int lane) {
  float s = 0.f;
  if constexpr (VEC4) {
    for (int c = lane * 4; c < C; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(a + c);
      const float4 y = *reinterpret_cast<const float4*>(b + c);
      s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
    }
  } else {
    for (int c = lane; c < C; c += 64) s = fmaf(a[c], b[c], s);
  }
  return egnn_wave_sum(s);
}

template <bool VEC4>
__global__ __launch_bounds__(256) void gat_attention_bwd_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                                const float* __restrict__ asrc, const float* __restrict__ adst,
                                                                const float* __restrict__ att, const float* __restrict__ mult,
                                                                const float* __restrict__ xl, int64_t ld_xl, const float* __restrict__ go,
                                                                int64_t ld_go, int64_t go_hs, float go_scale, int64_t n_rows, int64_t nnz,
                                                                int H, int C, float slope, float* __restrict__ d_raw,
                                                                float* __restrict__ d_adst) {
  const int lane = egnn_lane();
  const int64_t row = (int64_t)blockIdx.x * 4 + egnn_wave_id();
  if (row >= n_rows) return;
  const int64_t start = rowptr[row], end = rowptr[row + 1];
  for (int h = 0; h < H; ++h) {
    const float* gor = go + row * ld_go + h * go_hs;
    const float* a_h = att + (int64_t)h * nnz;
    float* dr_h = d_raw + (int64_t)h * nnz;
    // pass 1: g_e for 64 entries at a time (one wave-wide dot each; lane k keeps entry base + k), sum_row att g.  g is parked in
    // d_raw by the lane that owns the entry and read back by that same lane in pass 2 (same walk start, same stride).
    float acc = 0.f;
    for (int64_t base = start; base < end; base += 64) {
      const int cnt = (int)(end - base < 64 ? end - base : 64);
      float mine = 0.f;
      for (int k = 0; k < cnt; ++k) {
        const float g = wave_dot<VEC4>(gor, xl + col[base + k] * ld_xl + (int64_t)h * C, C, lane);
        mine = lane == k ? g : mine;
      }
      if (lane < cnt) {
        const int64_t e = base + lane;
        float g = mine * go_scale;
        if (mult != nullptr) g *= mult[(int64_t)h * nnz + e];
        acc = fmaf(a_h[e], g, acc);
        dr_h[e] = g;
      }
    }
    const float tot = egnn_wave_sum(acc);
    // pass 2: softmax and LeakyReLU backward (s recomputed exactly as the forward formed it), row sum -> d_a_dst
    const float ad = adst[row * H + h];
    float dsum = 0.f;
    for (int64_t e = start + lane; e < end; e += 64) {
      const float ds = a_h[e] * (dr_h[e] - tot);
      const float s = asrc[col[e] * H + h] + ad;
      const float d = s > 0.f ? ds : ds * slope;
      dr_h[e] = d;
      dsum += d;
    }
    dsum = egnn_wave_sum(dsum);
    if (lane == 0) d_adst[row * H + h] = dsum;
  }
}

// One wavefront per source row j of the transposed structure (colptr / t_col / perm: entry q of column j is entry perm[q] of the
// target-major CSR, whose row is t_col[q]).  Columns of a head in tiles of 256; per lane one float4 (VEC4) or four strided floats.
template <bool VEC4>
__global__ __launch_bounds__(256) void gat_aggregate_bwd_kernel(const int64_t* __restrict__ colptr, const int64_t* __restrict__ t_col,
                                                                const int64_t* __restrict__ perm, const float* __restrict__ att,
                                                                const float* __restrict__ mult, const float* __restrict__ d_raw,
                                                                const float* __restrict__ go, int64_t ld_go, int64_t go_hs, float go_scale,
                                                                const float* __restrict__ xl, int64_t ld_xl, const float* __restrict__ att_l,
                                                                const float* __restrict__ att_r, const float* __restrict__ d_adst,
                                                                int64_t n_src, int64_t nnz, int H, int C, float* __restrict__ dxl,
                                                                int64_t ld_dxl, float* __restrict__ partials) {
  extern __shared__ float s_acc[];   // [4 waves][2 H C] when partials != nullptr
  const int lane = egnn_lane();
  const int wave = egnn_wave_id();
  const int64_t HC = (int64_t)H * C;
  float* my = s_acc + (int64_t)wave * 2 * HC;
  if (partials != nullptr)
    for (int64_t k = lane; k < 2 * HC; k += 64) my[k] = 0.f;   // the wave's own region; lanes then update only their own columns
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * 4 + wave; j < n_src; j += (int64_t)gridDim.x * 4) {
    const int64_t b = colptr[j], e_end = colptr[j + 1];
    for (int h = 0; h < H; ++h) {
      const int64_t hoff = (int64_t)h * nnz;
      float das = 0.f;
      const float dad = att_r != nullptr ? d_adst[j * H + h] : 0.f;
      for (int c0 = 0; c0 < C; c0 += 256) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float das_part = 0.f;
        for (int64_t base = b; base < e_end; base += 64) {
          const int cnt = (int)(e_end - base < 64 ? e_end - base : 64);
          int64_t t = 0;
          float coef = 0.f;
          if (lane < cnt) {
            const int64_t p = perm[base + lane];
            t = t_col[base + lane];
            coef = att[hoff + p];
            if (mult != nullptr) coef *= mult[hoff + p];
            if (c0 == 0) das_part += d_raw[hoff + p];
          }
          for (int k = 0; k < cnt; ++k) {
            const int64_t tk = __shfl(t, k);
            const float ck = __shfl(coef, k);
            const float* gr = go + tk * ld_go + (int64_t)h * go_hs + c0;
            if constexpr (VEC4) {
              const int c = lane * 4;
              if (c0 + c < C) {
                const float4 v = *reinterpret_cast<const float4*>(gr + c);
                acc[0] = fmaf(ck, v.x, acc[0]); acc[1] = fmaf(ck, v.y, acc[1]);
                acc[2] = fmaf(ck, v.z, acc[2]); acc[3] = fmaf(ck, v.w, acc[3]);
              }
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (c0 + lane + 64 * r < C) acc[r] = fmaf(ck, gr[lane + 64 * r], acc[r]);
            }
          }
        }
        if (c0 == 0) das = egnn_wave_sum(das_part);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = VEC4 ? c0 + lane * 4 + r : c0 + lane + 64 * r;
          if (c >= C) continue;
          const int64_t hc = (int64_t)h * C + c;
          float v = fmaf(das, att_l[hc], acc[r] * go_scale);
          if (att_r != nullptr) v = fmaf(dad, att_r[hc], v);
          dxl[j * ld_dxl + hc] = v;
          if (partials != nullptr) {
            const float x = xl[j * ld_xl + hc];
            my[hc] = fmaf(x, das, my[hc]);
            my[HC + hc] = fmaf(x, dad, my[HC + hc]);
          }
        }
      }
    }
  }
  if (partials == nullptr) return;
  __syncthreads();
  for (int64_t k = threadIdx.x; k < 2 * HC; k += 256)
    partials[(int64_t)blockIdx.x * 2 * HC + k] = (s_acc[k] + s_acc[2 * HC + k]) + (s_acc[4 * HC + k] + s_acc[6 * HC + k]);
}

// out[k] = sum over the nb block partials of column k, one wave per column, fixed order
__global__ __launch_bounds__(256) void gat_partials_final_kernel(const float* __restrict__ partials, int nb, int64_t K,
                                                                 float* __restrict__ out) {
  const int lane = egnn_lane();
  const int64_t k = (int64_t)blockIdx.x * 4 + egnn_wave_id();
  if (k >= K) return;
  float t = 0.f;
  for (int b = lane; b < nb; b += 64) t += partials[(int64_t)b * K + k];
  t = egnn_wave_sum(t);
  if (lane == 0) out[k] = t;
}

inline int gat_bwd_blocks(int64_t n_src) {
  const int64_t want = (n_src + 3) / 4;
  return (int)(want < 1 ? 1 : (want < kGatBwdBlocks ? want : kGatBwdBlocks));
}

}  // namespace

extern "C" int egnn_gat_attention_bwd_f32(const int64_t* rowptr, const int64_t* col, const float* alpha_src, const float* alpha_dst,
                                          const float* att, const float* mult, const float* xl, int64_t ld_xl, const float* go,
                                          int64_t ld_go, int64_t go_head_stride, float go_scale, int64_t n_rows, int64_t nnz, int H,
                                          int C, float negative_slope, float* d_raw, float* d_alpha_dst, void* stream) {
  EGNN_CHECK_ARG(n_rows >= 0 && nnz >= 0 && H > 0 && H <= 64 && C > 0);
  EGNN_CHECK_ARG(ld_xl >= (int64_t)H * C && go_head_stride >= 0 && ld_go >= (H - 1) * go_head_stride + C);
  if (n_rows == 0) return EGNN_OK;
  EGNN_CHECK_ARG(rowptr && d_alpha_dst);
  EGNN_CHECK_ARG(nnz == 0 || (col && alpha_src && alpha_dst && att && xl && go && d_raw));
  const int64_t blocks = (n_rows + 3) / 4;
  if (blocks > 0x7fffffffLL) return EGNN_EINVAL;
  const bool vec4 = C % 4 == 0 && ld_xl % 4 == 0 && ld_go % 4 == 0 && go_head_stride % 4 == 0 && egnn_aligned16(xl) && egnn_aligned16(go);
  hipStream_t st = (hipStream_t)stream;
  if (vec4)
    hipLaunchKernelGGL(gat_attention_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, rowptr, col, alpha_src, alpha_dst, att,
                       mult, xl, ld_xl, go, ld_go, go_head_stride, go_scale, n_rows, nnz, H, C, negative_slope, d_raw, d_alpha_dst);
  else
    hipLaunchKernelGGL(gat_attention_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, rowptr, col, alpha_src, alpha_dst, att,
                       mult, xl, ld_xl, go, ld_go, go_head_stride, go_scale, n_rows, nnz, H, C, negative_slope, d_raw, d_alpha_dst);
  return egnn_launch_status();
}

extern "C" size_t egnn_gat_aggregate_bwd_ws_floats(int64_t n_src, int H, int C) {
  if (n_src < 0 || H <= 0 || C <= 0) return 0;
  return (size_t)gat_bwd_blocks(n_src) * 2 * (size_t)H * (size_t)C;
}

extern "C" int egnn_gat_aggregate_bwd_f32(const int64_t* colptr, const int64_t* t_col, const int64_t* perm, const float* att,
                                          const float* mult, const float* d_raw, const float* go, int64_t ld_go, int64_t go_head_stride,
                                          float go_scale, const float* xl, int64_t ld_xl, const float* att_l, const float* att_r,
                                          const float* d_alpha_dst, int64_t n_src, int64_t nnz, int H, int C, float* dxl, int64_t ld_dxl,
                                          float* d_att, float* ws, size_t ws_floats, void* stream) {
  EGNN_CHECK_ARG(n_src >= 0 && nnz >= 0 && H > 0 && H <= 64 && C > 0);
  const int64_t HC = (int64_t)H * C;
  EGNN_CHECK_ARG(ld_dxl >= HC && ld_xl >= HC && go_head_stride >= 0 && ld_go >= (H - 1) * go_head_stride + C);
  EGNN_CHECK_ARG((att_r == nullptr) == (d_alpha_dst == nullptr));
  if (d_att != nullptr) EGNN_CHECK_ARG(HC <= kGatMaxHC && ws && xl && ws_floats >= egnn_gat_aggregate_bwd_ws_floats(n_src, H, C));
  if (n_src == 0) return EGNN_OK;
  EGNN_CHECK_ARG(colptr && att_l && dxl);
  EGNN_CHECK_ARG(nnz == 0 || (t_col && perm && att && d_raw && go));
  const int nb = gat_bwd_blocks(n_src);
  const bool vec4 = C % 4 == 0 && ld_go % 4 == 0 && go_head_stride % 4 == 0 && egnn_aligned16(go);
  const size_t lds = d_att != nullptr ? (size_t)4 * 2 * HC * sizeof(float) : 0;
  float* partials = d_att != nullptr ? ws : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (vec4)
    hipLaunchKernelGGL(gat_aggregate_bwd_kernel<true>, dim3(nb), dim3(256), lds, st, colptr, t_col, perm, att, mult, d_raw, go, ld_go,
                       go_head_stride, go_scale, xl, ld_xl, att_l, att_r, d_alpha_dst, n_src, nnz, H, C, dxl, ld_dxl, partials);
  else
    hipLaunchKernelGGL(gat_aggregate_bwd_kernel<false>, dim3(nb), dim3(256), lds, st, colptr, t_col, perm, att, mult, d_raw, go, ld_go,
                       go_head_stride, go_scale, xl, ld_xl, att_l, att_r, d_alpha_dst, n_src, nnz, H, C, dxl, ld_dxl, partials);
  if (d_att != nullptr)
    hipLaunchKernelGGL(gat_partials_final_kernel, dim3((unsigned)((2 * HC + 3) / 4)), dim3(256), 0, st, ws, nb, 2 * HC, d_att);
  return egnn_launch_status();
}
