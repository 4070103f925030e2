// SIGN's element-wise operator family (/root/reference/arxiv_dgl/sign.py:128-133,150-157): Linear -> PReLU -> dropout with a learnable
// scalar slope, replicated over the hops and concatenated.  Three bandwidth kernels, each ONE launch for all hops:
//   gather + input dropout of the hop features into the concatenated batch matrix,
//   y = drop(prelu(z, a_h)) per column segment,
//   its backward: dz, the slope gradients and the column sums of dz (the bias gradient of the Linear that formed z) in one pass.
// "Segment" h = columns [h*Cs, (h+1)*Cs) of a row-major [B, H*Cs] matrix; every segment has its own slope pointer / source matrix and
// its own dropout seed.  The per-segment operands travel BY VALUE in the kernel arguments (SegTable, at most 16 segments): no device
// allocation, no copy.  The dropout uniform is bn_common.h's: uniform01(seed_h [+ *seed_dev], r * Cs + (c - h*Cs)), keep where u >= p.
//
// Work layout, shared by the three kernels: blockIdx.x = (segment, column chunk), blockIdx.y = row stripe.  Inside the workgroup the
// low TX lanes of the thread id run along the columns (VEC floats each: float4 on the aligned path, one float otherwise) and the rest
// along the rows, so that no index is ever divided and a thread keeps ONE column group for all its rows -- the column sums of the
// backward accumulate in registers.  Reductions: registers -> LDS tree per workgroup -> one partial per (stripe, column) in the
// workspace -> a finalize launch that folds the stripes in index order.  Every order is fixed: results are bit-equal from run to run.
#include "bn_common.h"
#include "block_reduce.h"

namespace {

using egnn_bn::uniform01;

constexpr int MAX_SEG = 16;
constexpr int THREADS = 256;
constexpr int MAX_STRIPES = 256;

struct SegTable {
  const float* ptr[MAX_SEG];            // prelu: the slope of segment h (device scalar); gather: the source matrix of hop h
  int64_t ld[MAX_SEG];                  // gather: its leading dimension
  unsigned long long seed[MAX_SEG];
};

struct Geo {
  int64_t B, Cs;
  int H, lg_tx, chunks, stripes;        // TX = 1 << lg_tx column lanes; `chunks` column chunks of TX * VEC per segment
  int64_t rows_per_stripe;
  float p;
  const unsigned long long* seed_dev;
};

static Geo make_geo(int64_t B, int64_t Cs, int H, int vec, float p, const unsigned long long* seed_dev) {
  Geo g{};
  g.B = B; g.Cs = Cs; g.H = H; g.p = p; g.seed_dev = seed_dev;
  const int64_t groups = (Cs + vec - 1) / vec;
  int lg = 0;
  while (lg < 6 && (int64_t(1) << lg) < groups) ++lg;
  g.lg_tx = lg;
  g.chunks = (int)((groups + (int64_t(1) << lg) - 1) >> lg);
  const int64_t ty = THREADS >> lg;
  int64_t s = (B + ty - 1) / ty;
  if (s > MAX_STRIPES) s = MAX_STRIPES;
  if (s < 1) s = 1;
  g.rows_per_stripe = (B + s - 1) / s;
  g.stripes = (int)((B + g.rows_per_stripe - 1) / g.rows_per_stripe);
  return g;
}

template <int VEC>
__device__ __forceinline__ void load_v(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void store_v(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// where this thread works: segment h, first column c (inside the segment), rows r0, r0 + TY, .. < r1
struct Where { int h; int64_t c; int64_t r0, r1; int ty_step; bool active; };
template <int VEC>
__device__ __forceinline__ Where where(const Geo& g) {
  Where w;
  const int h = (int)blockIdx.x / g.chunks;
  const int chunk = (int)blockIdx.x - h * g.chunks;
  const int tx = threadIdx.x & ((1 << g.lg_tx) - 1), ty = threadIdx.x >> g.lg_tx;
  w.h = h;
  w.c = ((int64_t)chunk << g.lg_tx | tx) * VEC;
  w.active = w.c < g.Cs;
  w.r0 = (int64_t)blockIdx.y * g.rows_per_stripe + ty;
  const int64_t end = ((int64_t)blockIdx.y + 1) * g.rows_per_stripe;
  w.r1 = end < g.B ? end : g.B;
  w.ty_step = THREADS >> g.lg_tx;
  return w;
}

// the multiplicative mask of VEC neighbouring elements: 1 / (1 - p) where u >= p, else 0 (bn_common.h bn_elem)
template <int VEC>
__device__ __forceinline__ void masks(unsigned long long seed, unsigned long long idx, float p, float inv, float (&m)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) m[v] = uniform01(seed, idx + v) >= p ? inv : 0.f;
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void gather_drop_kernel(SegTable t, Geo g, const int64_t* __restrict__ batch,
                                                              float* __restrict__ out, int64_t ld_out) {
  const Where w = where<VEC>(g);
  if (!w.active) return;
  const float* __restrict__ x = t.ptr[w.h];
  const int64_t ldx = t.ld[w.h];
  const unsigned long long seed = t.seed[w.h] + (g.seed_dev ? *g.seed_dev : 0ull);
  const float inv = 1.f / (1.f - g.p);
  const int64_t co = (int64_t)w.h * g.Cs + w.c;
#pragma unroll 2
  for (int64_t r = w.r0; r < w.r1; r += w.ty_step) {
    float v[VEC];
    load_v<VEC>(x + batch[r] * ldx + w.c, v);
    if (g.p > 0.f) {
      float m[VEC];
      masks<VEC>(seed, (unsigned long long)(r * g.Cs + w.c), g.p, inv, m);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] *= m[k];
    }
    store_v<VEC>(out + r * ld_out + co, v);
  }
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void prelu_drop_fwd_kernel(SegTable t, Geo g, const float* __restrict__ z, int64_t ld_z,
                                                                 float* __restrict__ y, int64_t ld_y) {
  const Where w = where<VEC>(g);
  if (!w.active) return;
  const float a = *t.ptr[w.h];
  const unsigned long long seed = t.seed[w.h] + (g.seed_dev ? *g.seed_dev : 0ull);
  const float inv = 1.f / (1.f - g.p);
  const int64_t co = (int64_t)w.h * g.Cs + w.c;
#pragma unroll 2
  for (int64_t r = w.r0; r < w.r1; r += w.ty_step) {
    float v[VEC];
    load_v<VEC>(z + r * ld_z + co, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = v[k] > 0.f ? v[k] : a * v[k];
    if (g.p > 0.f) {
      float m[VEC];
      masks<VEC>(seed, (unsigned long long)(r * g.Cs + w.c), g.p, inv, m);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] *= m[k];
    }
    store_v<VEC>(y + r * ld_y + co, v);
  }
}

// ws layout: [stripes][H * Cs] column partials, then [stripes][H * chunks] slope partials
template <int VEC>
__global__ __launch_bounds__(THREADS) void prelu_drop_bwd_kernel(SegTable t, Geo g, const float* __restrict__ z, int64_t ld_z,
                                                                 const float* __restrict__ dy, int64_t ld_dy, float* __restrict__ dz,
                                                                 int64_t ld_dz, float* __restrict__ ws) {
  __shared__ float s_col[THREADS * VEC];
  __shared__ float s_da[1][THREADS];
  const Where w = where<VEC>(g);
  float cs[VEC], da = 0.f;
#pragma unroll
  for (int k = 0; k < VEC; ++k) cs[k] = 0.f;
  if (w.active) {
    const float a = *t.ptr[w.h];
    const unsigned long long seed = t.seed[w.h] + (g.seed_dev ? *g.seed_dev : 0ull);
    const float inv = 1.f / (1.f - g.p);
    const int64_t co = (int64_t)w.h * g.Cs + w.c;
#pragma unroll 2
    for (int64_t r = w.r0; r < w.r1; r += w.ty_step) {
      float zv[VEC], gv[VEC];
      load_v<VEC>(z + r * ld_z + co, zv);
      load_v<VEC>(dy + r * ld_dy + co, gv);
      if (g.p > 0.f) {
        float m[VEC];
        masks<VEC>(seed, (unsigned long long)(r * g.Cs + w.c), g.p, inv, m);
#pragma unroll
        for (int k = 0; k < VEC; ++k) gv[k] *= m[k];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool pos = zv[k] > 0.f;
        da += pos ? 0.f : gv[k] * zv[k];
        gv[k] = pos ? gv[k] : gv[k] * a;
        cs[k] += gv[k];
      }
      store_v<VEC>(dz + r * ld_dz + co, gv);
    }
  }
  // workgroup fold: the column lanes keep their column, the row lanes fold as a tree (fixed order)
  const int TX = 1 << g.lg_tx, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.lg_tx;
#pragma unroll
  for (int k = 0; k < VEC; ++k) s_col[threadIdx.x * VEC + k] = cs[k];
  s_da[0][threadIdx.x] = da;
  __syncthreads();
  for (int s = (THREADS >> g.lg_tx) >> 1; s > 0; s >>= 1) {
    if (ty < s) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) s_col[threadIdx.x * VEC + k] += s_col[(threadIdx.x + (s << g.lg_tx)) * VEC + k];
    }
    __syncthreads();
  }
  egnn_reduce::block_tree_fold<THREADS, 1>(s_da);
  const int64_t HC = (int64_t)g.H * g.Cs;
  if (ty == 0 && w.active) {
    float* o = ws + (int64_t)blockIdx.y * HC + (int64_t)w.h * g.Cs + w.c;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = s_col[tx * VEC + k];
  }
  if (threadIdx.x == 0) ws[(int64_t)g.stripes * HC + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s_da[0][0];
}

// blocks [0, col_blocks): dbias[c] = the stripes' partials of column c in stripe order; block col_blocks + h: da[h]
__global__ __launch_bounds__(THREADS) void prelu_drop_finalize_kernel(Geo g, const float* __restrict__ ws, int col_blocks,
                                                                      float* __restrict__ da, float* __restrict__ dbias) {
  __shared__ float s[1][THREADS];
  const int64_t HC = (int64_t)g.H * g.Cs;
  if ((int)blockIdx.x < col_blocks) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= HC) return;
    float acc = 0.f;
    for (int st = 0; st < g.stripes; ++st) acc += ws[(int64_t)st * HC + c];
    dbias[c] = acc;
    return;
  }
  const int h = (int)blockIdx.x - col_blocks;
  const float* part = ws + (int64_t)g.stripes * HC;
  const int per_stripe = g.H * g.chunks, items = g.stripes * g.chunks;
  float acc[1] = {0.f};
  for (int i = threadIdx.x; i < items; i += THREADS) {
    const int st = i / g.chunks, k = i - st * g.chunks;
    acc[0] += part[(int64_t)st * per_stripe + h * g.chunks + k];
  }
  egnn_reduce::block_tree_sum<THREADS>(acc, s);
  if (threadIdx.x == 0) da[h] = s[0][0];
}

bool mult4(int64_t v) { return (v & 3) == 0; }

// the checks every entry point shares; the seeds are read (host memory) only when a mask is drawn
int common_args(const egnn_sign_seg_t* seg) {
  EGNN_CHECK_ARG(seg != nullptr);
  EGNN_CHECK_ARG(seg->H >= 1 && seg->H <= MAX_SEG && seg->B >= 0 && seg->Cs >= 1);
  EGNN_CHECK_ARG(seg->p >= 0.f && seg->p < 1.f);
  EGNN_CHECK_ARG(seg->p == 0.f || seg->seed != nullptr);
  EGNN_CHECK_ARG(seg->Cs <= (int64_t(1) << 31) && seg->B <= (int64_t(1) << 40));
  return EGNN_OK;
}

void fill_seeds(const egnn_sign_seg_t* seg, SegTable& t) {
  for (int h = 0; h < seg->H; ++h) t.seed[h] = seg->p > 0.f ? seg->seed[h] : 0ull;
}

}  // namespace

extern "C" int egnn_sign_gather_drop_f32(const egnn_sign_seg_t* seg, float* out, int64_t ld_out, void* stream) {
  const int rc = common_args(seg);
  if (rc != EGNN_OK) return rc;
  EGNN_CHECK_ARG(seg->src && seg->ld_src && seg->batch && out && seg->n_src >= 1 && ld_out >= seg->H * seg->Cs);
  SegTable t{};
  bool vec = mult4(seg->Cs) && mult4(ld_out) && egnn_aligned16(out);
  for (int h = 0; h < seg->H; ++h) {
    EGNN_CHECK_ARG(seg->src[h] != nullptr && seg->ld_src[h] >= seg->Cs);
    t.ptr[h] = seg->src[h];
    t.ld[h] = seg->ld_src[h];
    vec = vec && mult4(seg->ld_src[h]) && egnn_aligned16(seg->src[h]);
  }
  fill_seeds(seg, t);
  if (seg->B == 0) return EGNN_OK;
  const Geo g = make_geo(seg->B, seg->Cs, seg->H, vec ? 4 : 1, seg->p, (const unsigned long long*)seg->seed_dev);
  const dim3 grid((unsigned)(g.H * g.chunks), (unsigned)g.stripes);
  if (vec) hipLaunchKernelGGL(gather_drop_kernel<4>, grid, dim3(THREADS), 0, (hipStream_t)stream, t, g, seg->batch, out, ld_out);
  else hipLaunchKernelGGL(gather_drop_kernel<1>, grid, dim3(THREADS), 0, (hipStream_t)stream, t, g, seg->batch, out, ld_out);
  return egnn_launch_status();
}

static int prelu_table(const egnn_sign_seg_t* seg, SegTable& t) {
  EGNN_CHECK_ARG(seg->slope != nullptr);
  for (int h = 0; h < seg->H; ++h) {
    EGNN_CHECK_ARG(seg->slope[h] != nullptr);
    t.ptr[h] = seg->slope[h];
  }
  fill_seeds(seg, t);
  return EGNN_OK;
}

extern "C" int egnn_prelu_drop_fwd_f32(const egnn_sign_seg_t* seg, const float* z, int64_t ld_z, float* y, int64_t ld_y, void* stream) {
  int rc = common_args(seg);
  if (rc != EGNN_OK) return rc;
  const int64_t HC = seg->H * seg->Cs;
  EGNN_CHECK_ARG(z && y && ld_z >= HC && ld_y >= HC);
  SegTable t{};
  rc = prelu_table(seg, t);
  if (rc != EGNN_OK) return rc;
  if (seg->B == 0) return EGNN_OK;
  const bool vec = mult4(seg->Cs) && mult4(ld_z) && mult4(ld_y) && egnn_aligned16(z) && egnn_aligned16(y);
  const Geo g = make_geo(seg->B, seg->Cs, seg->H, vec ? 4 : 1, seg->p, (const unsigned long long*)seg->seed_dev);
  const dim3 grid((unsigned)(g.H * g.chunks), (unsigned)g.stripes);
  if (vec) hipLaunchKernelGGL(prelu_drop_fwd_kernel<4>, grid, dim3(THREADS), 0, (hipStream_t)stream, t, g, z, ld_z, y, ld_y);
  else hipLaunchKernelGGL(prelu_drop_fwd_kernel<1>, grid, dim3(THREADS), 0, (hipStream_t)stream, t, g, z, ld_z, y, ld_y);
  return egnn_launch_status();
}

// the scalar path has the most column chunks: its size covers both paths
extern "C" size_t egnn_prelu_drop_ws_floats(int64_t B, int64_t Cs, int H) {
  if (B < 1 || Cs < 1 || H < 1 || H > MAX_SEG) return 0;
  const Geo g = make_geo(B, Cs, H, 1, 0.f, nullptr);
  return (size_t)g.stripes * ((size_t)H * (size_t)Cs + (size_t)H * (size_t)g.chunks);
}

extern "C" int egnn_prelu_drop_bwd_f32(const egnn_sign_seg_t* seg, const float* z, int64_t ld_z, const float* dy, int64_t ld_dy,
                                       float* dz, int64_t ld_dz, float* da, float* dbias, float* ws, size_t ws_floats, void* stream) {
  int rc = common_args(seg);
  if (rc != EGNN_OK) return rc;
  const int64_t HC = seg->H * seg->Cs;
  EGNN_CHECK_ARG(z && dy && dz && da && dbias && ld_z >= HC && ld_dy >= HC && ld_dz >= HC);
  SegTable t{};
  rc = prelu_table(seg, t);
  if (rc != EGNN_OK) return rc;
  EGNN_CHECK_ARG(seg->B >= 1);
  if (!ws || ws_floats < egnn_prelu_drop_ws_floats(seg->B, seg->Cs, seg->H)) return EGNN_EWORKSPACE;
  const bool vec = mult4(seg->Cs) && mult4(ld_z) && mult4(ld_dy) && mult4(ld_dz) && egnn_aligned16(z) && egnn_aligned16(dy) &&
                   egnn_aligned16(dz);
  const Geo g = make_geo(seg->B, seg->Cs, seg->H, vec ? 4 : 1, seg->p, (const unsigned long long*)seg->seed_dev);
  const dim3 grid((unsigned)(g.H * g.chunks), (unsigned)g.stripes);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(prelu_drop_bwd_kernel<4>, grid, dim3(THREADS), 0, st, t, g, z, ld_z, dy, ld_dy, dz, ld_dz, ws);
  else hipLaunchKernelGGL(prelu_drop_bwd_kernel<1>, grid, dim3(THREADS), 0, st, t, g, z, ld_z, dy, ld_dy, dz, ld_dz, ws);
  const int col_blocks = (int)((HC + THREADS - 1) / THREADS);
  hipLaunchKernelGGL(prelu_drop_finalize_kernel, dim3((unsigned)(col_blocks + g.H)), dim3(THREADS), 0, st, g, ws, col_blocks, da, dbias);
  return egnn_launch_status();
}
