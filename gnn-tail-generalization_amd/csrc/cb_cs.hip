// Row passes of Correct & Smooth (Label_propagation_model/outcome_correlation.py:95-126,158-213) for gfx950: everything of
// double_correlation_autoscale / double_correlation_fixed / only_outcome_correlation that is not a propagation step (those are
// cb_spmm_csr_prop_f32 launches).  Each kernel is one pass over [N, C]; both are bound by HBM (4 C bytes read or written per row and matrix).
//
// Mapping: a row of C floats is owned by LPR = min(64, next power of two >= Cp) neighbouring lanes of a wavefront (lane = column, so the loads of a
// wavefront's 64 / LPR rows are one contiguous stretch), a block of 256 threads walks its rows in a grid-stride loop.  Row sums are xor-butterflies
// inside the LPR lanes; the one global sum (sum |E0| over the label rows) is taken in two stages through the caller's workspace — per-thread running
// sum over the block's rows, butterfly, LDS across the four wavefronts -> one partial per block, then one block adds the partials in index order.
// The grid depends on N and Cp only: no atomics, bit-identical from run to run.
//
// Label rows are given as a byte mask [N] (non-zero = label row): the same array serves as fix_rows of cb_spmm_csr_prop_f32.
#include <math.h>

#include "cb_common.h"

namespace cb {

constexpr int kCsBlock = 256;
constexpr int kCsMaxBlocks = 1024;

static inline int cs_lpr(int64_t Cp) {
  int l = 1;
  while (l < Cp && l < kWave) l <<= 1;
  return l;
}
static inline int cs_blocks(int64_t N, int64_t Cp) {
  const int64_t rows_per_block = (int64_t)(kCsBlock / cs_lpr(Cp));
  const int64_t b = (N + rows_per_block - 1) / rows_per_block;
  return (int)(b < 1 ? 1 : (b > kCsMaxBlocks ? kCsMaxBlocks : b));
}

__device__ __forceinline__ float group_sum(float v, int lpr) {      // sum over the lpr lanes of a row group (lpr a power of two <= 64): every lane gets it
  for (int o = lpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// E0 = onehot(y) - P on the label rows, 0 elsewhere (pre_residual_correlation :95-110), written Cp wide (padding columns 0); state = state_scale (.) E0;
// partial[block] = the block's share of sum |E0|
__global__ void __launch_bounds__(kCsBlock) k_cs_residual_init(const float* __restrict__ P, int64_t ld_p, const int64_t* __restrict__ labels,
                                                               const uint8_t* __restrict__ label_rows, int N, int C, int Cp, int lpr,
                                                               const float* __restrict__ state_scale, float* __restrict__ E0, float* __restrict__ state,
                                                               float* __restrict__ partial) {
  __shared__ float s_w[kCsBlock / kWave];
  const int sub = threadIdx.x & (lpr - 1);
  const int rows_per_block = kCsBlock / lpr;
  float run = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / lpr; row < N; row += (int64_t)gridDim.x * rows_per_block) {
    const bool lab = label_rows[row] != 0;
    const int y = lab ? (int)labels[row] : -1;
    const float s = state_scale ? state_scale[row] : 1.f;
    for (int c = sub; c < Cp; c += lpr) {
      float e = 0.f;
      if (lab && c < C) e = (c == y ? 1.f : 0.f) - P[row * ld_p + c];
      run += fabsf(e);
      __builtin_nontemporal_store(e, E0 + row * Cp + c);
      if (state) __builtin_nontemporal_store(e * s, state + row * Cp + c);
    }
  }
  run = group_sum(run, kWave);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = run;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// out[0] = sum of partial[0 .. n) in a fixed order: one wavefront, strided running sums, butterfly
__global__ void __launch_bounds__(kWave) k_cs_sum_partials(const float* __restrict__ partial, int n, float* __restrict__ out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kWave) s += partial[i];
  s = group_sum(s, kWave);
  if (threadIdx.x == 0) out[0] = s;
}

// mode 0 (autoscale, :170-176), 1 (fixed scale, :200), 2 (only, :209): res = P (+ scale * resid); y2 = res with the label rows snapped to one-hot
// (pre_outcome_correlation :112-126); state = state_scale (.) y2
__global__ void __launch_bounds__(kCsBlock) k_cs_correct_snap(int mode, const float* __restrict__ P, int64_t ld_p, const float* __restrict__ resid,
                                                              int64_t ld_r, const int64_t* __restrict__ labels, const uint8_t* __restrict__ label_rows,
                                                              int N, int C, int Cp, int lpr, const float* __restrict__ abs_sum, float n_label,
                                                              float scale_fixed, const float* __restrict__ state_scale, float* __restrict__ res,
                                                              int64_t ld_res, float* __restrict__ y2, float* __restrict__ state) {
  const int sub = threadIdx.x & (lpr - 1);
  const int rows_per_block = kCsBlock / lpr;
  const float orig_diff = mode == 0 ? abs_sum[0] / n_label : 0.f;
  // (the trip count is the same for the lpr lanes of a row group, and lpr divides 64: the butterfly below never meets an exited lane of its group;
  //  groups of one wavefront may leave the loop at different times, so the shuffle width is the group's)
  for (int64_t row = (int64_t)blockIdx.x * rows_per_block + threadIdx.x / lpr; row < N; row += (int64_t)gridDim.x * rows_per_block) {
    float scale = scale_fixed;
    if (mode == 0) {
      float l1 = 0.f;
      for (int c = sub; c < C; c += lpr) l1 += fabsf(resid[row * ld_r + c]);
      for (int o = lpr >> 1; o > 0; o >>= 1) l1 += __shfl_xor(l1, o, lpr);
      scale = orig_diff / l1;
      if (isinf(scale)) scale = 1.f;
      if (scale > 1000.f) scale = 1.f;
    }
    const bool lab = label_rows[row] != 0;
    const int y = lab ? (int)labels[row] : -1;
    const float s = state_scale ? state_scale[row] : 1.f;
    for (int c = sub; c < Cp; c += lpr) {
      float v = 0.f;
      if (c < C) {
        const float p = P[row * ld_p + c];
        v = p;
        if (mode != 2) {
          v = __fadd_rn(p, __fmul_rn(scale, resid[row * ld_r + c]));      // (product and sum rounded separately, as the reference's two operators)
          if (mode == 0 && v != v) v = p;                                  // the 0 / 0 rows
        }
        __builtin_nontemporal_store(v, res + row * ld_res + c);
        if (lab) v = c == y ? 1.f : 0.f;
      }
      __builtin_nontemporal_store(v, y2 + row * Cp + c);
      if (state) __builtin_nontemporal_store(v * s, state + row * Cp + c);
    }
  }
}

}  // namespace cb

using namespace cb;

extern "C" size_t cb_cs_workspace_bytes(int64_t N, int64_t Cp) {
  if (N <= 0 || Cp <= 0) return 0;
  return (size_t)cs_blocks(N, Cp) * sizeof(float);
}

static int cs_check_shape(const char* who, int64_t N, int64_t C, int64_t Cp) {
  CB_CHECK_ARG(N >= 0 && C >= 0 && Cp >= 0, CB_E_INVALID, "%s: negative size", who);
  CB_CHECK_ARG(N < INT32_MAX && Cp < (1 << 20), CB_E_RANGE, "%s: size exceeds the int32 contract", who);
  CB_CHECK_ARG(Cp >= C, CB_E_INVALID, "%s: padded width Cp smaller than C", who);
  return CB_OK;
}

extern "C" int cb_cs_residual_init_f32(const float* P, int64_t ld_p, const int64_t* labels, const uint8_t* label_rows, int64_t N, int64_t C, int64_t Cp,
                                       const float* state_scale, float* E0, float* state, float* abs_sum, void* ws, size_t ws_bytes, void* stream) {
  const int rc = cs_check_shape("cb_cs_residual_init_f32", N, C, Cp);
  if (rc != CB_OK) return rc;
  CB_CHECK_ARG(abs_sum != nullptr, CB_E_INVALID, "cb_cs_residual_init_f32: abs_sum is null");
  CB_CHECK_ARG(N == 0 || C == 0 || (P && labels && label_rows && E0), CB_E_INVALID, "cb_cs_residual_init_f32: null pointer");
  CB_CHECK_ARG(ld_p >= C, CB_E_INVALID, "cb_cs_residual_init_f32: leading dimension smaller than C");
  CB_CHECK_ARG(N == 0 || C == 0 || (ws && ws_bytes >= cb_cs_workspace_bytes(N, Cp)), CB_E_WORKSPACE,
               "cb_cs_residual_init_f32: workspace missing/too small (%zu < %zu)", ws_bytes, cb_cs_workspace_bytes(N, Cp));
  hipStream_t st = (hipStream_t)stream;
  if (N == 0 || C == 0) {
    hipLaunchKernelGGL(k_cs_sum_partials, dim3(1), dim3(kWave), 0, st, (const float*)nullptr, 0, abs_sum);
    CB_LAUNCH_CHECK();
    return CB_OK;
  }
  const int nb = cs_blocks(N, Cp);
  hipLaunchKernelGGL(k_cs_residual_init, dim3(nb), dim3(kCsBlock), 0, st, P, ld_p, labels, label_rows, (int)N, (int)C, (int)Cp, cs_lpr(Cp), state_scale, E0,
                     state, (float*)ws);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cs_sum_partials, dim3(1), dim3(kWave), 0, st, (const float*)ws, nb, abs_sum);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_cs_correct_snap_f32(int32_t mode, const float* P, int64_t ld_p, const float* resid, int64_t ld_r, const int64_t* labels,
                                      const uint8_t* label_rows, int64_t N, int64_t C, int64_t Cp, const float* abs_sum, int64_t n_label, float scale,
                                      const float* state_scale, float* res_result, int64_t ld_res, float* y2, float* state, void* stream) {
  const int rc = cs_check_shape("cb_cs_correct_snap_f32", N, C, Cp);
  if (rc != CB_OK) return rc;
  CB_CHECK_ARG(mode >= 0 && mode <= 2, CB_E_INVALID, "cb_cs_correct_snap_f32: mode must be 0 (autoscale), 1 (fixed) or 2 (only), got %d", (int)mode);
  if (N == 0 || C == 0) return CB_OK;
  CB_CHECK_ARG(P && labels && label_rows && res_result && y2, CB_E_INVALID, "cb_cs_correct_snap_f32: null pointer");
  CB_CHECK_ARG(mode == 2 || resid, CB_E_INVALID, "cb_cs_correct_snap_f32: modes 0 and 1 need the propagated residual");
  CB_CHECK_ARG(mode != 0 || (abs_sum && n_label > 0), CB_E_INVALID, "cb_cs_correct_snap_f32: autoscale needs sum |E0| and a positive label-row count");
  CB_CHECK_ARG(ld_p >= C && ld_res >= C && (mode == 2 || ld_r >= C), CB_E_INVALID, "cb_cs_correct_snap_f32: leading dimension smaller than C");
  hipLaunchKernelGGL(k_cs_correct_snap, dim3(cs_blocks(N, Cp)), dim3(kCsBlock), 0, (hipStream_t)stream, (int)mode, P, ld_p, resid, ld_r, labels, label_rows,
                     (int)N, (int)C, (int)Cp, cs_lpr(Cp), abs_sum, (float)n_label, scale, state_scale, res_result, ld_res, y2, state);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
