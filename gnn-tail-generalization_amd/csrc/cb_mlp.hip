// Row stage and losses of the Cold Brew STUDENT MLPs (MLP_model/__init__.py:1-156, utils.py:885-908 getMLP,
// trainer_node_classification.py:66-210).  All fp32, HBM-bound:
//   k_ln_gelu_drop_fwd / _bwd   [LayerNorm, GELU, Dropout] of a getMLP group in one pass over the Linear's output z
//   k_mse_rows                  nn.MSELoss()(pred, target[row_index]) and its gradient, the gather never materialised
//   k_part2_assemble / _bwd     torch.cat([x_b, alpha1 * replaced, alpha0 * part1_out], -1) and d(alpha0), d(alpha1)
// Row kernels: one wavefront per row, a lane owns 4 consecutive columns of every 256-column slab (dwordx4 accesses when the rows are
// 16-byte aligned), row reductions by cross-lane butterflies — no LDS, no block barrier.  Column sums (d gamma, d beta, the bias gradient
// of the Linear in front) leave as one partial row per wavefront and are summed in a fixed order: no float atomics, bit-reproducible.
#include "cb_common.h"
#include "cb_philox.h"

namespace cb {
namespace mlp {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kSlab = 4 * kWave;             // columns one wavefront covers per slab
constexpr int kMaxSlabs = 2;                 // d <= 512: a row lives in registers (a third slab makes the backward spill SGPRs)
constexpr int kMaxFwdBlocks = 256 * 8;
constexpr int kMaxBwdWaves = 256 * 8;        // partial rows of the backward's column sums
constexpr int kMaxBlocks = 256 * 8;          // flat kernels; == cb_reduce_workspace_bytes() / 4

// keep-mask factors of the 4 elements at flat indices f0 .. f0+3 (f0 need not be a multiple of 4): what cb_dropout_f32 draws there
__device__ __forceinline__ void keep4_flat(uint64_t seed, int64_t f0, int sub, uint32_t thresh, float scale, float (&m)[4]) {
  // sub = f0 & 3 is wave-uniform and the same in every slab of a row: every lane's f0 is row * d + a multiple of 4
  keep4(seed, f0 >> 2, thresh, scale, m);
  if (sub) {
    float m2[4];
    keep4(seed, (f0 >> 2) + 1, thresh, scale, m2);
    const float e[8] = {m[0], m[1], m[2], m[3], m2[0], m2[1], m2[2], m2[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = sub == 1 ? e[i + 1] : (sub == 2 ? e[i + 2] : e[i + 3]);   // (selects: no dynamically indexed registers)
  }
}

// v[s][i] = p[s * 256 + 4 * lane + i], 0 past column d.  EXACT: d == 256 and 16-byte aligned rows (no masks); vec: d % 4 == 0 and aligned.
template <int NS, bool EXACT>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, int d, int lane, bool vec, float (&v)[NS][4]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = s * kSlab + 4 * lane;
    if (EXACT || (vec && c < d)) {
      const float4 t = *reinterpret_cast<const float4*>(p + c);
      v[s][0] = t.x; v[s][1] = t.y; v[s][2] = t.z; v[s][3] = t.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[s][i] = (c + i < d) ? p[c + i] : 0.f;
    }
  }
}

template <int NS, bool EXACT>
__device__ __forceinline__ void store_cols(float* __restrict__ p, int d, int lane, bool vec, const float (&v)[NS][4]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int c = s * kSlab + 4 * lane;
    if (EXACT || (vec && c < d)) {
      *reinterpret_cast<float4*>(p + c) = make_float4(v[s][0], v[s][1], v[s][2], v[s][3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c + i < d) p[c + i] = v[s][i];
    }
  }
}

// out = dropout(gelu(gamma * (z - mean) * rstd + beta));  stats[r] = {mean, rstd}
template <int NS, bool EXACT, bool DROP>
__global__ void __launch_bounds__(kBlock) k_ln_gelu_drop_fwd(const float* __restrict__ z, int64_t rows, int d, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, uint32_t thresh, float scale, uint64_t seed,
                                                             const uint64_t* __restrict__ seed_dev, float* __restrict__ out,
                                                             float* __restrict__ stats, int vec_i) {
  if (DROP && seed_dev) seed += *seed_dev;
  const bool vec = vec_i != 0;
  const int lane = lane_id();
  const float inv_d = 1.f / (float)d;
  float g[NS][4], b[NS][4];
  load_cols<NS, EXACT>(gamma, d, lane, vec, g);
  load_cols<NS, EXACT>(beta, d, lane, vec, b);
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); r < rows; r += nw) {
    float v[NS][4];
    const int sub = EXACT ? 0 : bcast_first((int)((r * d) & 3));
    load_cols<NS, EXACT>(z + r * d, d, lane, vec, v);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) s += v[k][i];            // columns past d hold 0
    const float mean = wave_sum(s) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = (EXACT || k * kSlab + 4 * lane + i < d) ? v[k][i] - mean : 0.f;
        v[k][i] = t;
        q += t * t;
      }
    const float rstd = 1.f / sqrtf(wave_sum(q) * inv_d + eps);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int c = k * kSlab + 4 * lane;
      float m[4] = {1.f, 1.f, 1.f, 1.f};
      if (DROP && (EXACT || c < d)) keep4_flat(seed, r * d + c, sub, thresh, scale, m);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float u = __fmaf_rn(g[k][i], v[k][i] * rstd, b[k][i]);
        const float y = 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
        v[k][i] = DROP ? y * m[i] : y;
      }
    }
    store_cols<NS, EXACT>(out + r * d, d, lane, vec, v);
    if (stats && lane == 0) *reinterpret_cast<float2*>(stats + 2 * r) = make_float2(mean, rstd);
  }
}

// dz of the stage above from dy, z and the row statistics; per-wavefront partial rows of d gamma, d beta and colsum(dz) -> part[wave][3][d]
template <int NS, bool EXACT, bool DROP>
__global__ void __launch_bounds__(kBlock) k_ln_gelu_drop_bwd(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ stats,
                                                             int64_t rows, int d, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             uint32_t thresh, float scale, uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                                             float* __restrict__ dz, float* __restrict__ part, int vec_i) {
  if (DROP && seed_dev) seed += *seed_dev;
  const bool vec = vec_i != 0;
  const int lane = lane_id();
  const float inv_d = 1.f / (float)d;
  float g[NS][4], b[NS][4], ag[NS][4], ab[NS][4], az[NS][4];
  load_cols<NS, EXACT>(gamma, d, lane, vec, g);
  load_cols<NS, EXACT>(beta, d, lane, vec, b);
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) ag[k][i] = ab[k][i] = az[k][i] = 0.f;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t r = wave; r < rows; r += nw) {
    float xh[NS][4], du[NS][4];
    const int sub = EXACT ? 0 : bcast_first((int)((r * d) & 3));
    load_cols<NS, EXACT>(z + r * d, d, lane, vec, xh);
    load_cols<NS, EXACT>(dy + r * d, d, lane, vec, du);
    const float2 st = *reinterpret_cast<const float2*>(stats + 2 * r);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int c = k * kSlab + 4 * lane;
      float m[4] = {1.f, 1.f, 1.f, 1.f};
      if (DROP && (EXACT || c < d)) keep4_flat(seed, r * d + c, sub, thresh, scale, m);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = EXACT || c + i < d;
        const float x = ok ? (xh[k][i] - st.x) * st.y : 0.f;
        const float u = __fmaf_rn(g[k][i], x, b[k][i]);
        const float cdf = 0.5f * (1.f + erff(u * 0.70710678118654752f));
        const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
        float t = du[k][i] * (cdf + u * pdf);              // dy is 0 past column d
        if (DROP) t *= m[i];
        xh[k][i] = x;
        ag[k][i] += t * x;
        ab[k][i] += t;
        t *= g[k][i];                                      // d x_hat
        du[k][i] = t;
        s1 += t;
        s2 += t * x;
      }
    }
    const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = EXACT || k * kSlab + 4 * lane + i < d;
        const float t = ok ? st.y * (du[k][i] - m1 - xh[k][i] * m2) : 0.f;
        du[k][i] = t;
        az[k][i] += t;
      }
    store_cols<NS, EXACT>(dz + r * d, d, lane, vec, du);
  }
  float* p = part + wave * 3 * (int64_t)d;                  // (3 d floats: 16-byte aligned rows iff d % 4 == 0)
  store_cols<NS, EXACT>(p, d, lane, vec, ag);
  store_cols<NS, EXACT>(p + d, d, lane, vec, ab);
  store_cols<NS, EXACT>(p + 2 * (int64_t)d, d, lane, vec, az);
}

// out_k[c] = sum_w part[w][k][c]: one block per (k, c), strided sums per thread, then a fixed-order tree
__global__ void __launch_bounds__(kBlock) k_colsum3_finish(const float* __restrict__ part, int nparts, int d, float* __restrict__ o0,
                                                           float* __restrict__ o1, float* __restrict__ o2) {
  __shared__ float s_t[kBlock];
  const int k = blockIdx.x / d, c = blockIdx.x - k * d;
  float s = 0.f;
  for (int p = threadIdx.x; p < nparts; p += kBlock) s += part[((int64_t)p * 3 + k) * d + c];
  s_t[threadIdx.x] = s;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_t[threadIdx.x] += s_t[threadIdx.x + off];
    __syncthreads();
  }
  float* o = k == 0 ? o0 : (k == 1 ? o1 : o2);
  if (threadIdx.x == 0 && o) o[c] = s_t[0];
}

// block sum of NV per-thread values in a fixed order -> partial[blockIdx.x * NV + j]
template <int NV>
__device__ __forceinline__ void block_partials(float (&local)[NV], float* __restrict__ partial) {
  __shared__ float s_w[kWavesPerBlock][NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) local[j] = wave_sum(local[j]);
  if (lane_id() == 0)
#pragma unroll
    for (int j = 0; j < NV; ++j) s_w[threadIdx.x >> 6][j] = local[j];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      float t = 0.f;
      for (int w = 0; w < kWavesPerBlock; ++w) t += s_w[w][j];
      partial[blockIdx.x * NV + j] = t;
    }
}

// one wavefront: out[j] = scale * sum_p partial[p * NV + j] (double accumulation, fixed order)
template <int NV>
__global__ void k_partials_finish(const float* __restrict__ partial, int nparts, double scale, float* __restrict__ out) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    double t = 0.0;
    for (int p = threadIdx.x; p < nparts; p += kWave) t += (double)partial[p * NV + j];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    if (threadIdx.x == 0) out[j] = (float)(t * scale);
  }
}

// loss partials of mean((pred - target[row_index])^2) and grad = 2 (pred - target[row_index]) / (B D).  A row index outside [0, n_t) is
// never dereferenced: its elements count as NaN.
template <bool VEC4>
__global__ void __launch_bounds__(kBlock) k_mse_rows(const float* __restrict__ pred, int64_t B, int D, const float* __restrict__ target, int64_t ld_t,
                                                     int64_t n_t, const int64_t* __restrict__ row_index, float gscale, float* __restrict__ grad,
                                                     float* __restrict__ partial) {
  constexpr int W = VEC4 ? 4 : 1;
  const int64_t per_row = D / W, n = B * per_row;
  float local[1] = {0.f};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row) * W;
    const int64_t tr = row_index ? row_index[r] : r;
    const bool ok = tr >= 0 && tr < n_t;
    float pv[W], tv[W] = {};
    if constexpr (VEC4) {
      const float4 a = *reinterpret_cast<const float4*>(pred + r * D + c);
      pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
      if (ok) {
        const float4 t = *reinterpret_cast<const float4*>(target + tr * ld_t + c);
        tv[0] = t.x; tv[1] = t.y; tv[2] = t.z; tv[3] = t.w;
      }
    } else {
      pv[0] = pred[r * D + c];
      if (ok) tv[0] = target[tr * ld_t + c];
    }
    float gv[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float df = ok ? pv[k] - tv[k] : __builtin_nanf("");
      local[0] += df * df;
      gv[k] = df * gscale;
    }
    if (grad) {
      if constexpr (VEC4) *reinterpret_cast<float4*>(grad + r * D + c) = make_float4(gv[0], gv[1], gv[2], gv[3]);
      else grad[r * D + c] = gv[0];
    }
  }
  block_partials<1>(local, partial);
}

// out[b] = [ x[b] (F) | alpha[1] * rep[b] (D) | alpha[0] * p1[b] (D) ]; a block whose source is null is left as it is
__global__ void __launch_bounds__(kBlock) k_part2_assemble(const float* __restrict__ x, int F, const float* __restrict__ rep, const float* __restrict__ p1,
                                                           int D, const float* __restrict__ alphas, int64_t B, float* __restrict__ out) {
  const float a0 = alphas[0], a1 = alphas[1];
  const int W = F + 2 * D;
  const int64_t n = B * W;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t b = i / W;
    const int c = (int)(i - b * W);
    if (c < F) {
      if (x) out[i] = x[b * F + c];
    } else if (c < F + D) {
      if (rep) out[i] = a1 * rep[b * D + (c - F)];
    } else if (p1) {
      out[i] = a0 * p1[b * D + (c - F - D)];
    }
  }
}

// partial[block] = { <g[:, F+D:], p1>, <g[:, F:F+D], rep> }
__global__ void __launch_bounds__(kBlock) k_part2_assemble_bwd(const float* __restrict__ g, int F, const float* __restrict__ rep,
                                                               const float* __restrict__ p1, int D, int64_t B, float* __restrict__ partial) {
  const int W = F + 2 * D;
  const int64_t n = B * 2 * D;
  float local[2] = {0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t b = i / (2 * D);
    const int j = (int)(i - b * 2 * D);
    const float gv = g[b * W + F + j];
    if (j < D) local[1] += gv * rep[b * D + j];
    else local[0] += gv * p1[b * D + (j - D)];
  }
  block_partials<2>(local, partial);
}

static inline int flat_grid(int64_t items) {
  int64_t b = (items + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

static inline int64_t bwd_waves(int64_t rows) {
  int64_t w = (rows + kWavesPerBlock - 1) / kWavesPerBlock * kWavesPerBlock;
  return w > kMaxBwdWaves ? kMaxBwdWaves : w;
}

}  // namespace mlp
}  // namespace cb

using namespace cb;
using namespace cb::mlp;

extern "C" int cb_ln_gelu_drop_fwd_f32(const float* z, int64_t rows, int64_t d, const float* gamma, const float* beta, float eps, float p,
                                       uint64_t seed, const uint64_t* seed_dev, float* out, float* stats, void* stream) {
  CB_CHECK_ARG(rows >= 0 && d >= 1 && d <= kMaxSlabs * kSlab && p >= 0.f && p < 1.f && eps >= 0.f, CB_E_INVALID,
               "cb_ln_gelu_drop_fwd_f32: bad argument (rows=%lld, d=%lld: 1 <= d <= %d, p=%f)", (long long)rows, (long long)d, kMaxSlabs * kSlab, p);
  if (rows == 0) return CB_OK;
  CB_CHECK_ARG(z && gamma && beta && out, CB_E_INVALID, "cb_ln_gelu_drop_fwd_f32: null pointer");
  CB_CHECK_ARG(!stats || (uintptr_t)stats % 8 == 0, CB_E_INVALID, "cb_ln_gelu_drop_fwd_f32: stats must be 8-byte aligned");
  const int vec = d % 4 == 0 && aligned16(z) && aligned16(out) && aligned16(gamma) && aligned16(beta);
  const uint32_t thresh = dropout_threshold(p);
  const float scale = 1.f / (1.f - p);
  int64_t nb = (rows + kWavesPerBlock - 1) / kWavesPerBlock;
  if (nb > kMaxFwdBlocks) nb = kMaxFwdBlocks;
  hipStream_t st = (hipStream_t)stream;
#define CB_LN_FWD(NS_, EX_, DR_)                                                                                                            \
  hipLaunchKernelGGL((k_ln_gelu_drop_fwd<NS_, EX_, DR_>), dim3((unsigned)nb), dim3(kBlock), 0, st, z, rows, (int)d, gamma, beta, eps, thresh, \
                     scale, seed, seed_dev, out, stats, vec)
#define CB_LN_FWD_D(NS_, EX_) \
  do { if (p > 0.f) CB_LN_FWD(NS_, EX_, true); else CB_LN_FWD(NS_, EX_, false); } while (0)
  if (d == kSlab && vec) CB_LN_FWD_D(1, true);
  else if (d <= kSlab) CB_LN_FWD_D(1, false);
  else CB_LN_FWD_D(2, false);
#undef CB_LN_FWD_D
#undef CB_LN_FWD
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_ln_gelu_drop_bwd_workspace_bytes(int64_t rows, int64_t d) {
  if (rows <= 0 || d <= 0) return 0;
  return (size_t)bwd_waves(rows) * 3 * (size_t)d * sizeof(float);
}

extern "C" int cb_ln_gelu_drop_bwd_f32(const float* dy, const float* z, const float* stats, int64_t rows, int64_t d, const float* gamma,
                                       const float* beta, float p, uint64_t seed, const uint64_t* seed_dev, float* dz, float* dgamma,
                                       float* dbeta, float* dbias, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(rows >= 0 && d >= 1 && d <= kMaxSlabs * kSlab && p >= 0.f && p < 1.f, CB_E_INVALID,
               "cb_ln_gelu_drop_bwd_f32: bad argument (rows=%lld, d=%lld: 1 <= d <= %d, p=%f)", (long long)rows, (long long)d, kMaxSlabs * kSlab, p);
  hipStream_t st = (hipStream_t)stream;
  if (rows == 0) {
    if (dgamma) CB_HIP(hipMemsetAsync(dgamma, 0, d * sizeof(float), st));
    if (dbeta) CB_HIP(hipMemsetAsync(dbeta, 0, d * sizeof(float), st));
    if (dbias) CB_HIP(hipMemsetAsync(dbias, 0, d * sizeof(float), st));
    return CB_OK;
  }
  CB_CHECK_ARG(dy && z && stats && gamma && beta && dz, CB_E_INVALID, "cb_ln_gelu_drop_bwd_f32: null pointer");
  CB_CHECK_ARG((uintptr_t)stats % 8 == 0, CB_E_INVALID, "cb_ln_gelu_drop_bwd_f32: stats must be 8-byte aligned");
  CB_CHECK_ARG(ws && ws_bytes >= cb_ln_gelu_drop_bwd_workspace_bytes(rows, d), CB_E_WORKSPACE,
               "cb_ln_gelu_drop_bwd_f32: workspace too small (%zu < %zu)", ws_bytes, cb_ln_gelu_drop_bwd_workspace_bytes(rows, d));
  const int vec = d % 4 == 0 && aligned16(z) && aligned16(dy) && aligned16(dz) && aligned16(gamma) && aligned16(beta) && aligned16(ws);
  const uint32_t thresh = dropout_threshold(p);
  const float scale = 1.f / (1.f - p);
  const int64_t nwaves = bwd_waves(rows);
  const unsigned nb = (unsigned)(nwaves / kWavesPerBlock);
  float* part = (float*)ws;
#define CB_LN_BWD(NS_, EX_, DR_)                                                                                                       \
  hipLaunchKernelGGL((k_ln_gelu_drop_bwd<NS_, EX_, DR_>), dim3(nb), dim3(kBlock), 0, st, dy, z, stats, rows, (int)d, gamma, beta, thresh, \
                     scale, seed, seed_dev, dz, part, vec)
#define CB_LN_BWD_D(NS_, EX_) \
  do { if (p > 0.f) CB_LN_BWD(NS_, EX_, true); else CB_LN_BWD(NS_, EX_, false); } while (0)
  if (d == kSlab && vec) CB_LN_BWD_D(1, true);
  else if (d <= kSlab) CB_LN_BWD_D(1, false);
  else CB_LN_BWD_D(2, false);
#undef CB_LN_BWD_D
#undef CB_LN_BWD
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_colsum3_finish, dim3((unsigned)(3 * d)), dim3(kBlock), 0, st, (const float*)part, (int)nwaves, (int)d, dgamma, dbeta, dbias);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_mse_rows_f32(const float* pred, int64_t B, int64_t D, const float* target, int64_t ld_t, int64_t n_target_rows,
                               const int64_t* row_index, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(B >= 0 && D >= 1 && D < (1 << 20) && ld_t >= D && n_target_rows >= 0 && loss && (B == 0 || (pred && target)), CB_E_INVALID,
               "cb_mse_rows_f32: bad argument");
  CB_CHECK_ARG(ws && ws_bytes >= cb_reduce_workspace_bytes(), CB_E_WORKSPACE, "cb_mse_rows_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const double n = (double)B * (double)D;
  int nb = 0;
  if (B > 0) {
    const bool v4 = D % 4 == 0 && ld_t % 4 == 0 && aligned16(pred) && aligned16(target) && (!grad || aligned16(grad));
    nb = flat_grid(v4 ? B * (D / 4) : B * D);
    const float gscale = (float)(2.0 / n);
    if (v4) hipLaunchKernelGGL((k_mse_rows<true>), dim3(nb), dim3(kBlock), 0, st, pred, B, (int)D, target, ld_t, n_target_rows, row_index, gscale, grad, (float*)ws);
    else hipLaunchKernelGGL((k_mse_rows<false>), dim3(nb), dim3(kBlock), 0, st, pred, B, (int)D, target, ld_t, n_target_rows, row_index, gscale, grad, (float*)ws);
    CB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((k_partials_finish<1>), dim3(1), dim3(kWave), 0, st, (const float*)ws, nb, B > 0 ? 1.0 / n : 0.0, loss);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_part2_assemble_f32(const float* x, int64_t F, const float* replaced, const float* part1_out, int64_t D, const float* alphas,
                                     int64_t B, float* out, void* stream) {
  CB_CHECK_ARG(B >= 0 && F >= 0 && D >= 1 && F + 2 * D < (1 << 24), CB_E_INVALID, "cb_part2_assemble_f32: bad size");
  if (B == 0) return CB_OK;
  CB_CHECK_ARG((x || replaced || part1_out) && alphas && out, CB_E_INVALID, "cb_part2_assemble_f32: null pointer");
  hipLaunchKernelGGL(k_part2_assemble, dim3(flat_grid(B * (F + 2 * D))), dim3(kBlock), 0, (hipStream_t)stream, x, (int)F, replaced, part1_out, (int)D,
                     alphas, B, out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_part2_assemble_bwd_f32(const float* g, int64_t F, const float* replaced, const float* part1_out, int64_t D, int64_t B,
                                         float* dalphas, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(B >= 0 && F >= 0 && D >= 1 && F + 2 * D < (1 << 24) && dalphas, CB_E_INVALID, "cb_part2_assemble_bwd_f32: bad argument");
  CB_CHECK_ARG(ws && ws_bytes >= 2 * cb_reduce_workspace_bytes(), CB_E_WORKSPACE, "cb_part2_assemble_bwd_f32: workspace too small");
  CB_CHECK_ARG(B == 0 || (g && replaced && part1_out), CB_E_INVALID, "cb_part2_assemble_bwd_f32: null pointer");
  hipStream_t st = (hipStream_t)stream;
  int nb = 0;
  if (B > 0) {
    nb = flat_grid(B * 2 * D);
    hipLaunchKernelGGL(k_part2_assemble_bwd, dim3(nb), dim3(kBlock), 0, st, g, (int)F, replaced, part1_out, (int)D, B, (float*)ws);
    CB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((k_partials_finish<2>), dim3(1), dim3(kWave), 0, st, (const float*)ws, nb, 1.0, dalphas);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
