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
//
// The arxiv GAT teacher's layer (/root/reference/arxiv_dgl/models.py:95-236, trained by arxiv_dgl/gat.py:116-148) adds an edge subset
// `keep` (edge_drop: the softmax runs over the kept entries, att = 0 elsewhere), a source scale r (out-degree^-1/2) and a target
// scale q (in-degree^1/2), and has no a_dst term without attn_r:
//   out[i,h,:] = q_i sum_e att[h,e] m[h,e] r_{col e} xl[col e,h,:]
// gat_layer_fwd_kernel forms att and out for all heads in one launch (one wavefront per target row, xl read in place with row stride
// H*C -- float2 loads for C = 250 --, r folded into the coefficient).  The two backward kernels take r and q as nullable arguments:
// with go' = q_i go_i,  g_e = m_e r_{col e} <go'_i, xl[col e]>,  dxl[j] = r_j (sum att m go' + d_a_src[j] att_l) + d_a_dst[j] att_r,
// d_att_l = sum_j r_j xl_j d_a_src[j]  (a_src comes from the scaled source features, a_dst from the unscaled ones).
#include "common.h"
#include "block_reduce.h"

namespace {

using namespace egnn_reduce;

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
                                                                int H, int C, float slope, const float* __restrict__ r,
                                                                const float* __restrict__ q, float* __restrict__ d_raw,
                                                                float* __restrict__ d_adst) {
  const int lane = egnn_lane();
  const int64_t row = (int64_t)blockIdx.x * 4 + egnn_wave_id();
  if (row >= n_rows) return;
  const int64_t start = rowptr[row], end = rowptr[row + 1];
  const float qi = q != nullptr ? q[row] : 1.f;
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
        if (q != nullptr) g *= qi;
        if (mult != nullptr) g *= mult[(int64_t)h * nnz + e];
        if (r != nullptr) g *= r[col[e]];
        acc = fmaf(a_h[e], g, acc);
        dr_h[e] = g;
      }
    }
    const float tot = egnn_wave_sum(acc);
    // pass 2: softmax and LeakyReLU backward (s recomputed exactly as the forward formed it), row sum -> d_a_dst
    const float ad = adst != nullptr ? adst[row * H + h] : 0.f;
    float dsum = 0.f;
    for (int64_t e = start + lane; e < end; e += 64) {
      const float ds = a_h[e] * (dr_h[e] - tot);
      const float s = asrc[col[e] * H + h] + ad;
      const float d = s > 0.f ? ds : ds * slope;
      dr_h[e] = d;
      dsum += d;
    }
    if (d_adst == nullptr) continue;
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
                                                                int64_t n_src, int64_t nnz, int H, int C, const float* __restrict__ r_src,
                                                                const float* __restrict__ q_dst, float* __restrict__ dxl, int64_t ld_dxl,
                                                                float* __restrict__ partials) {
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
    const float rj = r_src != nullptr ? r_src[j] : 1.f;
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
            if (q_dst != nullptr) coef *= q_dst[t];
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
          if (r_src != nullptr) v *= rj;
          if (att_r != nullptr) v = fmaf(dad, att_r[hc], v);
          dxl[j * ld_dxl + hc] = v;
          if (partials != nullptr) {
            const float x = xl[j * ld_xl + hc];
            my[hc] = fmaf(x, r_src != nullptr ? das * rj : das, my[hc]);
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

inline int gat_bwd_blocks(int64_t n_src) { return (int)capped_blocks(n_src, 4, kGatBwdBlocks); }

// VEC floats of one load / store: float4 (16-byte aligned head blocks), float2 (8-byte: C = 250) or float
template <int VEC> struct GatVec;
template <> struct GatVec<4> { using T = float4; };
template <> struct GatVec<2> { using T = float2; };
template <> struct GatVec<1> { using T = float; };

template <int VEC>
__device__ __forceinline__ void gat_vec_fma(float ck, const typename GatVec<VEC>::T& v, float* acc) {
  if constexpr (VEC == 4) {
    acc[0] = fmaf(ck, v.x, acc[0]); acc[1] = fmaf(ck, v.y, acc[1]); acc[2] = fmaf(ck, v.z, acc[2]); acc[3] = fmaf(ck, v.w, acc[3]);
  } else if constexpr (VEC == 2) {
    acc[0] = fmaf(ck, v.x, acc[0]); acc[1] = fmaf(ck, v.y, acc[1]);
  } else {
    acc[0] = fmaf(ck, v, acc[0]);
  }
}

// The whole forward of one DGL-style GAT layer, one wavefront per target row, all heads in one launch: scores + LeakyReLU + softmax
// over the KEPT entries of the row (att [H, nnz], exactly 0 at dropped entries; a row without a kept entry: zeros), then
//   out[i,h,:] = q_i sum_e (att[h,e] mult[h,e] r_{col e}) xl[col e,h,:]
// with xl gathered in place (row stride ld_xl, head block h*C: no padded or scaled copy).  Columns of a head in tiles of 256: a lane
// owns R = 4 / VEC vectors of VEC floats.  Entries go 64 at a time (lane k forms the coefficient of entry base + k), the gathers of
// four entries are issued together; an entry whose coefficient is 0 (dropped edge, dropped attention) is not gathered.
template <int VEC>
__global__ __launch_bounds__(256) void gat_layer_fwd_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                            const float* __restrict__ el, const float* __restrict__ er,
                                                            const uint8_t* __restrict__ keep, const float* __restrict__ mult,
                                                            const float* __restrict__ r_src, const float* __restrict__ q_dst,
                                                            const float* __restrict__ xl, int64_t ld_xl, int64_t n_rows, int64_t nnz, int H,
                                                            int C, float slope, float* __restrict__ att, float* __restrict__ out,
                                                            int64_t ld_out) {
  using V = typename GatVec<VEC>::T;
  constexpr int R = 4 / VEC;
  const int lane = egnn_lane();
  const int64_t row = (int64_t)blockIdx.x * 4 + egnn_wave_id();
  if (row >= n_rows) return;
  const int64_t start = rowptr[row], end = rowptr[row + 1];
  const float qi = q_dst != nullptr ? q_dst[row] : 1.f;
  for (int h = 0; h < H; ++h) {
    const float ad = er != nullptr ? er[row * H + h] : 0.f;
    const int64_t hoff = (int64_t)h * nnz;
    float m = -INFINITY;
    for (int64_t e = start + lane; e < end; e += 64) {
      if (keep != nullptr && keep[e] == 0) continue;
      float s = el[col[e] * H + h] + ad;
      s = s > 0.f ? s : s * slope;
      m = fmaxf(m, s);
    }
    m = egnn_wave_max(m);
    float z = 0.f;
    for (int64_t e = start + lane; e < end; e += 64) {
      if (keep != nullptr && keep[e] == 0) continue;
      float s = el[col[e] * H + h] + ad;
      s = s > 0.f ? s : s * slope;
      z += expf(s - m);
    }
    z = egnn_wave_sum(z);   // >= 1 when the row has a kept entry (the maximum contributes exp(0)), 0 otherwise
    for (int c0 = 0; c0 < C; c0 += 256) {
      float acc[R][VEC];
#pragma unroll
      for (int t = 0; t < R; ++t)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[t][v] = 0.f;
      for (int64_t base = start; base < end; base += 64) {
        const int cnt = (int)(end - base < 64 ? end - base : 64);
        int64_t cj = 0;
        float coef = 0.f;
        if (lane < cnt) {
          const int64_t e = base + lane;
          cj = col[e];
          float a = 0.f;
          if (keep == nullptr || keep[e] != 0) {
            float s = el[cj * H + h] + ad;
            s = s > 0.f ? s : s * slope;
            a = expf(s - m) / z;
          }
          if (c0 == 0) att[hoff + e] = a;
          coef = a;
          if (mult != nullptr) coef *= mult[hoff + e];
          if (r_src != nullptr) coef *= r_src[cj];
        }
        for (int k = 0; k < cnt; k += 4) {   // cnt <= 64: lanes k .. k + 3 exist; those at or past cnt hold coef = 0
          float ck[4];
          const float* xr[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            ck[u] = __shfl(coef, k + u);
            xr[u] = xl + __shfl(cj, k + u) * ld_xl + (int64_t)h * C + c0;
          }
          V v[4][R];
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < R; ++t) {
              const int c = (lane + 64 * t) * VEC;
              v[u][t] = V{};
              if (ck[u] != 0.f && c0 + c < C) v[u][t] = *reinterpret_cast<const V*>(xr[u] + c);
            }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int t = 0; t < R; ++t) gat_vec_fma<VEC>(ck[u], v[u][t], acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const int c = c0 + (lane + 64 * t) * VEC;
        if (c >= C) continue;
        float* o = out + row * ld_out + (int64_t)h * C + c;
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(qi * acc[t][0], qi * acc[t][1], qi * acc[t][2], qi * acc[t][3]);
        else if constexpr (VEC == 2) *reinterpret_cast<float2*>(o) = make_float2(qi * acc[t][0], qi * acc[t][1]);
        else *o = qi * acc[t][0];
      }
    }
  }
}

inline bool gat_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

int gat_launch_attention_bwd(const int64_t* rowptr, const int64_t* col, const float* alpha_src, const float* alpha_dst, const float* att,
                             const float* mult, const float* xl, int64_t ld_xl, const float* go, int64_t ld_go, int64_t go_head_stride,
                             float go_scale, int64_t n_rows, int64_t nnz, int H, int C, float negative_slope, const float* r, const float* q,
                             float* d_raw, float* d_alpha_dst, hipStream_t st) {
  const int64_t blocks = (n_rows + 3) / 4;
  if (blocks > 0x7fffffffLL) return EGNN_EINVAL;
  const bool vec4 = C % 4 == 0 && ld_xl % 4 == 0 && ld_go % 4 == 0 && go_head_stride % 4 == 0 && egnn_aligned16(xl) && egnn_aligned16(go);
  if (vec4)
    hipLaunchKernelGGL(gat_attention_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, rowptr, col, alpha_src, alpha_dst, att,
                       mult, xl, ld_xl, go, ld_go, go_head_stride, go_scale, n_rows, nnz, H, C, negative_slope, r, q, d_raw, d_alpha_dst);
  else
    hipLaunchKernelGGL(gat_attention_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, rowptr, col, alpha_src, alpha_dst, att,
                       mult, xl, ld_xl, go, ld_go, go_head_stride, go_scale, n_rows, nnz, H, C, negative_slope, r, q, d_raw, d_alpha_dst);
  return egnn_launch_status();
}

int gat_launch_aggregate_bwd(const int64_t* colptr, const int64_t* t_col, const int64_t* perm, const float* att, const float* mult,
                             const float* d_raw, const float* go, int64_t ld_go, int64_t go_head_stride, float go_scale, const float* xl,
                             int64_t ld_xl, const float* att_l, const float* att_r, const float* d_alpha_dst, int64_t n_src, int64_t nnz,
                             int H, int C, const float* r, const float* q, float* dxl, int64_t ld_dxl, float* d_att, float* ws,
                             hipStream_t st) {
  const int64_t HC = (int64_t)H * C;
  const int nb = gat_bwd_blocks(n_src);
  const bool vec4 = C % 4 == 0 && ld_go % 4 == 0 && go_head_stride % 4 == 0 && egnn_aligned16(go);
  const size_t lds = d_att != nullptr ? (size_t)4 * 2 * HC * sizeof(float) : 0;
  float* partials = d_att != nullptr ? ws : nullptr;
  if (vec4)
    hipLaunchKernelGGL(gat_aggregate_bwd_kernel<true>, dim3(nb), dim3(256), lds, st, colptr, t_col, perm, att, mult, d_raw, go, ld_go,
                       go_head_stride, go_scale, xl, ld_xl, att_l, att_r, d_alpha_dst, n_src, nnz, H, C, r, q, dxl, ld_dxl, partials);
  else
    hipLaunchKernelGGL(gat_aggregate_bwd_kernel<false>, dim3(nb), dim3(256), lds, st, colptr, t_col, perm, att, mult, d_raw, go, ld_go,
                       go_head_stride, go_scale, xl, ld_xl, att_l, att_r, d_alpha_dst, n_src, nnz, H, C, r, q, dxl, ld_dxl, partials);
  if (d_att != nullptr)
    colsum_partials(ws, nb, 2 * HC, d_att, st);   // out[k] = the nb block partials of column k in block order
  return egnn_launch_status();
}

}  // namespace

// ---- one GAT layer (PyG GATConv or the DGL-style one) as a descriptor (include/egnn_hip.h: egnn_gat_layer_t) ----
static int gat_layer_check(const egnn_gat_layer_t* L) {
  EGNN_CHECK_ARG(L != nullptr);
  EGNN_CHECK_ARG(L->n >= 0 && L->nnz >= 0 && L->H > 0 && L->H <= 64 && L->C > 0 && L->ld_xl >= (int64_t)L->H * L->C);
  if (L->n == 0) return EGNN_OK;
  EGNN_CHECK_ARG(L->rowptr && L->xl && L->el);
  EGNN_CHECK_ARG(L->nnz == 0 || L->col);
  return EGNN_OK;
}

extern "C" int egnn_gat_layer_fwd_f32(const egnn_gat_layer_t* L, float* att, float* out, int64_t ld_out, void* stream) {
  const int rc = gat_layer_check(L);
  if (rc != EGNN_OK) return rc;
  EGNN_CHECK_ARG(ld_out >= (int64_t)L->H * L->C);
  if (L->n == 0) return EGNN_OK;
  EGNN_CHECK_ARG(out && (L->nnz == 0 || att));
  const int64_t blocks = (L->n + 3) / 4;
  if (blocks > 0x7fffffffLL) return EGNN_EINVAL;
  const int C = L->C;
  const auto fits = [&](int v) {
    return C % v == 0 && L->ld_xl % v == 0 && ld_out % v == 0 && gat_aligned(L->xl, 4u * v) && gat_aligned(out, 4u * v);
  };
  hipStream_t st = (hipStream_t)stream;
#define EGNN_GAT_LAYER_FWD(V)                                                                                                        \
  hipLaunchKernelGGL(gat_layer_fwd_kernel<V>, dim3((unsigned)blocks), dim3(256), 0, st, L->rowptr, L->col, L->el, L->er, L->keep,    \
                     L->mult, L->src_scale, L->dst_scale, L->xl, L->ld_xl, L->n, L->nnz, L->H, L->C, L->negative_slope, att, out, ld_out)
  if (fits(4)) EGNN_GAT_LAYER_FWD(4);
  else if (fits(2)) EGNN_GAT_LAYER_FWD(2);
  else EGNN_GAT_LAYER_FWD(1);
#undef EGNN_GAT_LAYER_FWD
  return egnn_launch_status();
}

extern "C" size_t egnn_gat_layer_bwd_ws_floats(int64_t n, int H, int C) {
  if (n < 0 || H <= 0 || C <= 0) return 0;
  return (size_t)gat_bwd_blocks(n) * 2 * (size_t)H * (size_t)C;
}

extern "C" int egnn_gat_layer_bwd_f32(const egnn_gat_layer_t* L, const float* att, const float* go, int64_t ld_go, int mean_heads,
                                      float* d_raw, float* d_er, float* dxl, int64_t ld_dxl, float* d_attn, float* ws, size_t ws_floats,
                                      void* stream) {
  const int rc = gat_layer_check(L);
  if (rc != EGNN_OK) return rc;
  const int64_t HC = (int64_t)L->H * L->C;
  EGNN_CHECK_ARG(ld_go >= (mean_heads ? (int64_t)L->C : HC) && ld_dxl >= HC);
  EGNN_CHECK_ARG((L->attn_r == nullptr) == (L->er == nullptr) && (L->er == nullptr) == (d_er == nullptr));
  if (d_attn != nullptr) EGNN_CHECK_ARG(HC <= kGatMaxHC && ws && ws_floats >= egnn_gat_layer_bwd_ws_floats(L->n, L->H, L->C));
  if (L->n == 0) return EGNN_OK;
  EGNN_CHECK_ARG(L->colptr && L->attn_l && dxl);
  EGNN_CHECK_ARG(L->nnz == 0 || (L->t_col && L->perm && att && go && d_raw));
  // go[i,h,:] = go_scale * go[i * ld_go + h * go_hs + :]: the gradient of the head average reaches every head, scaled by 1/H
  const int64_t go_hs = mean_heads ? 0 : L->C;
  const float go_scale = mean_heads ? (float)(1.0 / L->H) : 1.f;
  hipStream_t st = (hipStream_t)stream;
  const int rc2 = gat_launch_attention_bwd(L->rowptr, L->col, L->el, L->er, att, L->mult, L->xl, L->ld_xl, go, ld_go, go_hs, go_scale, L->n,
                                           L->nnz, L->H, L->C, L->negative_slope, L->src_scale, L->dst_scale, d_raw, d_er, st);
  if (rc2 != EGNN_OK) return rc2;
  return gat_launch_aggregate_bwd(L->colptr, L->t_col, L->perm, att, L->mult, d_raw, go, ld_go, go_hs, go_scale, L->xl, L->ld_xl,
                                  L->attn_l, L->attn_r, d_er, L->n, L->nnz, L->H, L->C, L->src_scale, L->dst_scale, dxl, ld_dxl, d_attn,
                                  ws, st);
}
