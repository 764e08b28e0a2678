// Reductions to a scalar or a vector in a fixed two-stage order, and what is fused with them: the second stage of every column sum, the Frobenius
// norm, the fused log-softmax + NLL loss, Adam (which leaves the updated tensors' norms).  Partials live in cb_reduce_workspace_bytes() /
// cb_colsum_workspace_bytes() of caller workspace; no float atomics -> bit-reproducible.
#include "cb_reduce.h"

namespace cb {

// out[c] = sum_p partial[p][c]: one block per column, strided partial sums per thread then a fixed-order
// LDS tree — the result does not depend on scheduling.
__global__ void __launch_bounds__(kBlock) k_colsum_finish(const float* __restrict__ partial, int nparts, int d, float* __restrict__ out) {
  __shared__ float s_t[kBlock];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int p = threadIdx.x; p < nparts; p += kBlock) s += partial[(int64_t)p * d + c];
  s_t[threadIdx.x] = s;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_t[threadIdx.x] += s_t[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = s_t[0];
}

int colsum_finish(const float* partial, int nb, int d, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_colsum_finish, dim3((unsigned)d), dim3(kBlock), 0, st, partial, nb, d, out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// sum of squares -> partial[block] (double accumulation across the partials in the finish kernel)
__global__ void __launch_bounds__(kBlock) k_sumsq(const float* __restrict__ x, int64_t n, float* __restrict__ partial, int vec_ok) {
  __shared__ float s_w[kBlock / kWave];
  float s = 0.f;
  const int64_t nq = (n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = q * 4;
    if (vec_ok && i + 4 <= n) {
      float4 v = *reinterpret_cast<const float4*>(x + i);
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    } else {
      for (int k = 0; k < 4; ++k)
        if (i + k < n) s += x[i + k] * x[i + k];
    }
  }
  s = wave_sum(s);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kBlock / kWave; ++w) t += s_w[w];
    partial[blockIdx.x] = t;
  }
}

// one wavefront: lane l sums partials l, l+64, ... in double, then a fixed-order butterfly (deterministic)
__device__ __forceinline__ double wave_sum_partials(const float* __restrict__ partial, int nparts) {
  double t = 0.0;
  for (int p = threadIdx.x; p < nparts; p += kWave) t += (double)partial[p];
  for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
  return t;
}

// out[0] = sqrt(sum partial) (Frobenius norm, th.norm(self.le) GCN.py:232); out[1] = sum
__global__ void k_norm_finish(const float* __restrict__ partial, int nparts, float* __restrict__ out) {
  const double t = wave_sum_partials(partial, nparts);
  if (threadIdx.x == 0) {
    out[0] = (float)sqrt(t);
    out[1] = (float)t;
  }
}

// Fused log_softmax + nll_loss(mean over masked rows) forward AND its gradient
// (trainer_node_classification.py:390-391).  One lane per row; C is small (<= 256).
//   loss_partial[block] = sum_{r in block, mask[r]} (logsumexp(z_r) - z_r[y_r])
//   grad[r, c] = mask[r] ? (softmax(z_r)[c] - [c == y_r]) * inv_count : 0
// (A sub-wave-group-per-row variant with consecutive addresses inside a row measured slower at C = 40: 1.91 vs 1.59 ms on
// 10^7 rows — the 160-byte rows of neighbouring lanes already share cache lines.)
__global__ void __launch_bounds__(kBlock) k_nll_fused(const float* __restrict__ z, int64_t ld, const int64_t* __restrict__ y,
                                                      const uint8_t* __restrict__ mask, int64_t rows, int C, float inv_count,
                                                      float* __restrict__ grad, float* __restrict__ loss_partial) {
  __shared__ float s_w[kBlock / kWave];
  float local = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    const float* zr = z + r * ld;
    float* gr = grad ? grad + r * (int64_t)C : nullptr;
    if (mask && !mask[r]) {
      if (gr)
        for (int c = 0; c < C; ++c) gr[c] = 0.f;
      continue;
    }
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, zr[c]);
    // se in partial sums of 64 columns, then their sum: one chain of C additions loses about sqrt(C) roundings (at C = 4096 the gradient was nine
    // times further from float64 than a pairwise float32 sum).  C <= 64 is a single chain, 0 + it: the bits of before and of the vector kernels.
    float se = 0.f;
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int c1 = c0 + 64 < C ? c0 + 64 : C;
      float part = 0.f;
      for (int c = c0; c < c1; ++c) part += expf(zr[c] - mx);
      se += part;
    }
    const float lse = mx + logf(se);
    const int64_t t = y[r];
    const bool ok = t >= 0 && t < C;      // a label outside [0, C) is never an index: the row's loss term and gradient row are NaN
    const float zt = zr[ok ? t : 0];
    local += ok ? lse - zt : NAN;
    if (gr) {
      const float inv = 1.f / se;
      const float ic = ok ? inv_count : NAN;      // x * NaN is NaN for every x: the whole row
      for (int c = 0; c < C; ++c) gr[c] = (expf(zr[c] - mx) * inv - (c == t ? 1.f : 0.f)) * ic;
    }
  }
  local = wave_sum(local);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kBlock / kWave; ++w) t += s_w[w];
    loss_partial[blockIdx.x] = t;
  }
}

// The same arithmetic, expression for expression, with a row of C = 4 NV floats (NV <= 16, 16-byte aligned rows) held in registers: ten
// float4 loads and ten float4 stores per row at C = 40 instead of 120 + 40 scalar ones, every exp() evaluated once (1.64 -> 0.82 ms on 10^7 rows; same loss bits).
template <int NV>
__global__ void __launch_bounds__(kBlock) k_nll_fused_v4(const float* __restrict__ z, int64_t ld, const int64_t* __restrict__ y,
                                                         const uint8_t* __restrict__ mask, int64_t rows, float inv_count,
                                                         float* __restrict__ grad, float* __restrict__ loss_partial) {
  constexpr int C = 4 * NV;
  __shared__ float s_w[kBlock / kWave];
  float local = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    float4* gr = grad ? reinterpret_cast<float4*>(grad + r * (int64_t)C) : nullptr;
    if (mask && !mask[r]) {
      if (gr) {
#pragma unroll
        for (int q = 0; q < NV; ++q) gr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      continue;
    }
    const float4* zr = reinterpret_cast<const float4*>(z + r * ld);
    float v[C];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const float4 t4 = zr[q];
      v[4 * q] = t4.x; v[4 * q + 1] = t4.y; v[4 * q + 2] = t4.z; v[4 * q + 3] = t4.w;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, v[c]);
    const int64_t t64 = y[r];
    const bool ok = t64 >= 0 && t64 < C;      // checked as int64, before the narrowing: out of range -> NaN row, as in k_nll_fused
    const int t = ok ? (int)t64 : -1;
    float se = 0.f, zt = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      zt = c == t ? v[c] : zt;
      v[c] = expf(v[c] - mx);
      se += v[c];
    }
    const float lse = mx + logf(se);
    local += ok ? lse - zt : NAN;
    if (gr) {
      const float inv = 1.f / se;
      const float ic = ok ? inv_count : NAN;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (v[4 * q + k] * inv - (4 * q + k == t ? 1.f : 0.f)) * ic;
        gr[q] = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
  }
  local = wave_sum(local);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kBlock / kWave; ++w) t += s_w[w];
    loss_partial[blockIdx.x] = t;
  }
}

__global__ void k_loss_finish(const float* __restrict__ partial, int nparts, float inv_count, float* __restrict__ out) {
  const double t = wave_sum_partials(partial, nparts);
  if (threadIdx.x == 0) out[0] = (float)(t * (double)inv_count);
}

// torch.optim.Adam semantics (trainer_node_classification.py:310): g += wd*p; m,v EMA; bias-corrected step
__global__ void __launch_bounds__(kBlock) k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                 float wd, float bc1, float bc2_sqrt, const int64_t* __restrict__ step_dev, int vec_ok) {
  const int64_t nq = (n + 3) / 4;
  if (step_dev) {   // hipGraph mode: the step count lives in device memory, bias corrections are derived here
    const double t = (double)*step_dev;
    bc1 = (float)(1.0 - pow((double)b1, t));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
  }
  const float step = lr / bc1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = q * 4;
    float pv[4], gv[4], mv[4], vv[4];
    const bool full = vec_ok && i + 4 <= n;
    if (full) {
      float4 a = *reinterpret_cast<const float4*>(p + i), b = *reinterpret_cast<const float4*>(g + i);
      float4 c = *reinterpret_cast<const float4*>(m + i), d = *reinterpret_cast<const float4*>(v + i);
      pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
      gv[0] = b.x; gv[1] = b.y; gv[2] = b.z; gv[3] = b.w;
      mv[0] = c.x; mv[1] = c.y; mv[2] = c.z; mv[3] = c.w;
      vv[0] = d.x; vv[1] = d.y; vv[2] = d.z; vv[3] = d.w;
    } else {
      for (int k = 0; k < 4; ++k) {
        const bool in = i + k < n;
        pv[k] = in ? p[i + k] : 0.f; gv[k] = in ? g[i + k] : 0.f; mv[k] = in ? m[i + k] : 0.f; vv[k] = in ? v[i + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gg = gv[k] + wd * pv[k];
      mv[k] = b1 * mv[k] + (1.f - b1) * gg;
      vv[k] = b2 * vv[k] + (1.f - b2) * gg * gg;
      const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
      pv[k] = pv[k] - step * (mv[k] / denom);
    }
    if (full) {
      *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      *reinterpret_cast<float4*>(m + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (i + k < n) { p[i + k] = pv[k]; m[i + k] = mv[k]; v[i + k] = vv[k]; }
    }
  }
}

// All parameter tensors of the model in ONE launch: blockIdx.y selects the tensor, blockIdx.x strides over its elements.
// The table travels by value in the kernel arguments (no device-side table to keep alive, capturable in a hipGraph).
constexpr int kAdamMax = 24;
struct AdamTable {
  float* p[kAdamMax];
  const float* g[kAdamMax];
  float* m[kAdamMax];
  float* v[kAdamMax];
  int64_t n[kAdamMax];
  const float* c[kAdamMax];   // per-tensor extra L2 coefficient read from device memory (null: none), added to weight_decay
  float* sq[kAdamMax];        // per-tensor partial sums of squares of the UPDATED parameter, one float per block of the launch (null: not wanted)
};

__global__ void __launch_bounds__(kBlock) k_adam_multi(AdamTable t, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                       float bc2_sqrt, const int64_t* __restrict__ step_dev, const int32_t* __restrict__ guard) {
  // a gradient check of this step failed (cb_rows_zero_outside_mask_f32 set the word): parameters and moments stay as they are, and a
  // tensor whose norm is wanted gets the partials of its UNCHANGED values (the workspace holds whatever it held before)
  const bool skip = guard && *guard != 0;
  const int ti = blockIdx.y;
  if (skip && !t.sq[ti]) return;
  float* __restrict__ p = t.p[ti];
  const float* __restrict__ g = t.g[ti];
  float* __restrict__ m = t.m[ti];
  float* __restrict__ v = t.v[ti];
  const int64_t n = t.n[ti];
  if (step_dev) {
    const double s = (double)*step_dev;
    bc1 = (float)(1.0 - pow((double)b1, s));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, s));
  }
  const float step = lr / bc1;
  if (t.c[ti]) {
    const float c = *t.c[ti];
    if (isfinite(c)) wd += c;    // se_reg / ||le|| with ||le|| == 0: no regulariser gradient (torch.norm's subgradient at 0)
  }
  const bool vec_ok = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) == 0;
  const int64_t nq = (n + 3) / 4;
  float ssq = 0.f;      // sum of squares of the updated values this thread wrote: k_sumsq's thread-to-element map and summation order
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = q * 4;
    if (skip) {      // (uniform over the launch) read p only, store nothing
      if (vec_ok && i + 4 <= n) {
        const float4 a = *reinterpret_cast<const float4*>(p + i);
        ssq += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
      } else {
        for (int k = 0; k < 4; ++k)
          if (i + k < n) ssq += p[i + k] * p[i + k];
      }
      continue;
    }
    float pv[4], gv[4], mv[4], vv[4];
    const bool full = vec_ok && i + 4 <= n;
    if (full) {
      const float4 a = *reinterpret_cast<const float4*>(p + i), b = *reinterpret_cast<const float4*>(g + i);
      const float4 c = *reinterpret_cast<const float4*>(m + i), d = *reinterpret_cast<const float4*>(v + i);
      pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
      gv[0] = b.x; gv[1] = b.y; gv[2] = b.z; gv[3] = b.w;
      mv[0] = c.x; mv[1] = c.y; mv[2] = c.z; mv[3] = c.w;
      vv[0] = d.x; vv[1] = d.y; vv[2] = d.z; vv[3] = d.w;
    } else {
      for (int k = 0; k < 4; ++k) {
        const bool in = i + k < n;
        pv[k] = in ? p[i + k] : 0.f; gv[k] = in ? g[i + k] : 0.f; mv[k] = in ? m[i + k] : 0.f; vv[k] = in ? v[i + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // same arithmetic as k_adam
      const float gg = gv[k] + wd * pv[k];
      mv[k] = b1 * mv[k] + (1.f - b1) * gg;
      vv[k] = b2 * vv[k] + (1.f - b2) * gg * gg;
      const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
      pv[k] = pv[k] - step * (mv[k] / denom);
    }
    if (full) {
      *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      *reinterpret_cast<float4*>(m + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      ssq += pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2] + pv[3] * pv[3];
    } else {
      for (int k = 0; k < 4; ++k)
        if (i + k < n) { p[i + k] = pv[k]; m[i + k] = mv[k]; v[i + k] = vv[k]; ssq += pv[k] * pv[k]; }
    }
  }
  if (t.sq[ti]) {      // (uniform over the block) ||p||_F^2 of the updated tensor as k_sumsq would leave it: the next forward's th.norm(le) for free
    __shared__ float s_w[kBlock / kWave];
    ssq = wave_sum(ssq);
    if (lane_id() == 0) s_w[threadIdx.x >> 6] = ssq;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tt = 0.f;
      for (int w = 0; w < kBlock / kWave; ++w) tt += s_w[w];
      t.sq[ti][blockIdx.x] = tt;
    }
  }
}

}  // namespace cb

using namespace cb;

extern "C" size_t cb_colsum_workspace_bytes(int64_t rows, int64_t d) {
  if (rows <= 0 || d <= 0) return 0;
  return (size_t)colsum_blocks(rows) * (size_t)d * sizeof(float);
}

extern "C" size_t cb_reduce_workspace_bytes(void) { return (size_t)kMaxBlocks * sizeof(float); }

extern "C" int cb_frobenius_norm_f32(const float* x, int64_t n, float* out2, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(n >= 0 && out2 && (n == 0 || x), CB_E_INVALID, "cb_frobenius_norm_f32: bad argument");
  CB_CHECK_ARG(ws && ws_bytes >= cb_reduce_workspace_bytes(), CB_E_WORKSPACE, "cb_frobenius_norm_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nb = n ? grid_for((n + 3) / 4) : 0;
  if (nb) {
    hipLaunchKernelGGL(k_sumsq, dim3(nb), dim3(kBlock), 0, st, x, n, (float*)ws, aligned16(x));
    CB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(64), 0, st, (const float*)ws, nb, out2);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_nll_logsoftmax_f32(const float* logits, int64_t ld, const int64_t* y, const uint8_t* mask, int64_t rows,
                                     int64_t C, int64_t count, float* loss, float* grad, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(rows >= 0 && C > 0 && C <= 4096 && ld >= C && loss && (rows == 0 || (logits && y)), CB_E_INVALID,
               "cb_nll_logsoftmax_f32: bad argument");
  CB_CHECK_ARG(ws && ws_bytes >= cb_reduce_workspace_bytes(), CB_E_WORKSPACE, "cb_nll_logsoftmax_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const float inv = count > 0 ? 1.f / (float)count : 0.f;
  const int nb = rows ? grid_for(rows) : 0;
  if (nb) {
    const bool v4 = C % 4 == 0 && C <= 64 && ld % 4 == 0 && aligned16(logits) && (!grad || aligned16(grad));
#define CB_NLL_V4(NV_) hipLaunchKernelGGL((k_nll_fused_v4<NV_>), dim3(nb), dim3(kBlock), 0, st, logits, ld, y, mask, rows, inv, grad, (float*)ws)
    if (v4 && C == 40) CB_NLL_V4(10);
    else if (v4 && C == 48) CB_NLL_V4(12);
    else if (v4 && C == 8) CB_NLL_V4(2);
    else if (v4 && C == 4) CB_NLL_V4(1);
    else if (v4 && C == 64) CB_NLL_V4(16);
    else hipLaunchKernelGGL(k_nll_fused, dim3(nb), dim3(kBlock), 0, st, logits, ld, y, mask, rows, (int)C, inv, grad, (float*)ws);
#undef CB_NLL_V4
    CB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(64), 0, st, (const float*)ws, nb, inv, loss);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                                float eps, float weight_decay, int64_t step, const int64_t* step_dev, void* stream) {
  CB_CHECK_ARG(n >= 0 && (step >= 1 || step_dev) && (n == 0 || (p && g && m && v)), CB_E_INVALID, "cb_adam_step_f32: bad argument");
  if (step < 1) step = 1;
  if (n == 0) return CB_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int vec_ok = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);
  hipLaunchKernelGGL(k_adam, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2,
                     eps, weight_decay, (float)bc1, (float)sqrt(bc2), step_dev, vec_ok);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_adam_norm_workspace_bytes(int32_t n_norms) { return (size_t)(n_norms > 0 ? n_norms : 0) * cb_reduce_workspace_bytes(); }

extern "C" int cb_adam_multi_norm_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                      const int64_t* numel, const float* const* extra_decay, float* const* norm_out, float lr, float beta1,
                                      float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev, const int32_t* guard,
                                      void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(n_tensors >= 0 && (step >= 1 || step_dev) && (n_tensors == 0 || (p && g && m && v && numel)), CB_E_INVALID,
               "cb_adam_multi_f32: bad argument");
  int n_norms = 0;
  if (norm_out)
    for (int i = 0; i < n_tensors; ++i) n_norms += norm_out[i] != nullptr;
  CB_CHECK_ARG(n_norms == 0 || (ws && ws_bytes >= cb_adam_norm_workspace_bytes(n_norms)), CB_E_WORKSPACE,
               "cb_adam_multi_norm_f32: workspace too small for %d norms", n_norms);
  int norm_slot = 0;
  if (step < 1) step = 1;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  for (int base = 0; base < n_tensors; base += kAdamMax) {
    AdamTable t{};
    const int cnt = n_tensors - base < kAdamMax ? n_tensors - base : kAdamMax;
    int64_t nmax = 0;
    for (int i = 0; i < cnt; ++i) {
      CB_CHECK_ARG(numel[base + i] >= 0 && (numel[base + i] == 0 || (p[base + i] && g[base + i] && m[base + i] && v[base + i])), CB_E_INVALID,
                   "cb_adam_multi_f32: null tensor %d", base + i);
      t.p[i] = p[base + i]; t.g[i] = g[base + i]; t.m[i] = m[base + i]; t.v[i] = v[base + i]; t.n[i] = numel[base + i];
      t.c[i] = extra_decay ? extra_decay[base + i] : nullptr;
      if (norm_out && norm_out[base + i]) t.sq[i] = (float*)ws + (size_t)(norm_slot++) * kMaxBlocks;
      if (t.n[i] > nmax) nmax = t.n[i];
    }
    const int nb = nmax ? grid_for((nmax + 3) / 4) : 0;
    if (nb) {
      hipLaunchKernelGGL(k_adam_multi, dim3((unsigned)nb, (unsigned)cnt), dim3(kBlock), 0, (hipStream_t)stream, t, lr,
                         beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), step_dev, guard);
      CB_LAUNCH_CHECK();
    }
    for (int i = 0; i < cnt; ++i)      // out[0] = ||p||_F, out[1] = ||p||_F^2 (cb_frobenius_norm_f32's pair) of every tensor that asked
      if (t.sq[i]) {
        hipLaunchKernelGGL(k_norm_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)t.sq[i], nb, norm_out[base + i]);
        CB_LAUNCH_CHECK();
      }
  }
  return CB_OK;
}

extern "C" int cb_adam_multi_f32(int32_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                                 const int64_t* numel, const float* const* extra_decay, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int64_t step, const int64_t* step_dev, const int32_t* guard, void* stream) {
  return cb_adam_multi_norm_f32(n_tensors, p, g, m, v, numel, extra_decay, nullptr, lr, beta1, beta2, eps, weight_decay, step, step_dev, guard, nullptr,
                                0, stream);
}
