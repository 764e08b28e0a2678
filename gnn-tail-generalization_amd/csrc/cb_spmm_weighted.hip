// Edge-weighted sum-aggregation — the `edge_weight` form of GCNConv.forward (GNN_model/GCN.py:199-202):
//     graph.edata['_edge_weight'] = edge_weight;  update_all(fn.u_mul_e('h', '_edge_weight', 'm'), fn.sum('m', 'h'))
//     rst[v, :] = sum_{e: (u -> v)} w_e * h[u, :]
// TricksComb never passes edge_weight (GCN.py:115), so this is the boundary's cold corner: a plain, exact, deterministic kernel — one
// wavefront per destination row, 64 (column id, weight) pairs per coalesced index load, wave-uniform broadcast, lanes own columns
// lane + 64 j — not the tuned edge-stream kernel of cb_spmm.hip.  Same epilogue (row scale, bias, ReLU) as cb_spmm_csr_f32.
// Backward pieces: the same kernel on the reverse CSR with the weights in that order (d h), and cb_spmm_edge_dot_f32 (d w_e =
// <h[u], g[v]>, one wavefront per row, wave reduction).  Bound: HBM, E (4 d + 8) + N (4 d + 4) bytes.
#include "cb_common.h"

namespace cb {

constexpr int kWJ = 8;     // column groups of 64 a wavefront keeps in registers per sweep over the row's edges (d <= 512 in one sweep)

__global__ void __launch_bounds__(256) k_spmm_weighted(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
                                                       const float* __restrict__ h, int64_t ld_h, float* __restrict__ out, int64_t ld_out,
                                                       int n_rows, int d, const float* __restrict__ row_scale, const float* __restrict__ bias,
                                                       int relu) {
  const int lane = lane_id();
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= n_rows) return;
  const int e0 = rowptr[row], e1 = rowptr[row + 1];
  const float rs = row_scale ? row_scale[row] : 1.f;
  for (int c0 = 0; c0 < d; c0 += 64 * kWJ) {
    float acc[kWJ];
#pragma unroll
    for (int j = 0; j < kWJ; ++j) acc[j] = 0.f;
    for (int base = e0; base < e1; base += kWave) {
      const int cnt = min(kWave, e1 - base);
      int my_col = 0;
      float my_w = 0.f;
      if (lane < cnt) {
        my_col = col[base + lane];
        my_w = w[base + lane];
      }
      for (int k = 0; k < cnt; ++k) {
        const int c = bcast_lane(my_col, k);
        const float wk = __int_as_float(bcast_lane(__float_as_int(my_w), k));
        const float* hr = h + (int64_t)c * ld_h + c0 + lane;
#pragma unroll
        for (int j = 0; j < kWJ; ++j)
          if (c0 + lane + 64 * j < d) acc[j] += wk * hr[64 * j];
      }
    }
#pragma unroll
    for (int j = 0; j < kWJ; ++j) {
      const int c = c0 + lane + 64 * j;
      if (c < d) {
        float v = scale_add(acc[j], rs, bias ? bias[c] : 0.f);      // rst * norm + bias (GCN.py:250,253), as cb_spmm_csr_f32
        out[(int64_t)row * ld_out + c] = relu ? relu_nan(v) : v;
      }
    }
  }
}

// dw[j] = <h[col[j], :], g[row of j, :]>
__global__ void __launch_bounds__(256) k_spmm_edge_dot(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ h,
                                                       int64_t ld_h, const float* __restrict__ g, int64_t ld_g, int n_rows, int d,
                                                       float* __restrict__ dw) {
  const int lane = lane_id();
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= n_rows) return;
  const int e0 = rowptr[row], e1 = rowptr[row + 1];
  const float* gr = g + (int64_t)row * ld_g;
  for (int e = e0; e < e1; ++e) {
    const float* hr = h + (int64_t)col[e] * ld_h;
    float s = 0.f;
    for (int c = lane; c < d; c += kWave) s += hr[c] * gr[c];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) dw[e] = s;
  }
}

}  // namespace cb

using namespace cb;

extern "C" int cb_spmm_csr_weighted_f32(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, int64_t E, const float* h,
                                        int64_t ld_h, int64_t d, const float* row_scale, const float* bias, int relu, float* out,
                                        int64_t ld_out, void* stream) {
  CB_CHECK_ARG(N >= 0 && E >= 0 && d >= 0, CB_E_INVALID, "cb_spmm_csr_weighted_f32: negative size");
  CB_CHECK_ARG(N < INT32_MAX && E < INT32_MAX && d < (1 << 20), CB_E_RANGE, "cb_spmm_csr_weighted_f32: size exceeds the int32 contract");
  if (N == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(rowptr && h && out && (E == 0 || (col && w)), CB_E_INVALID, "cb_spmm_csr_weighted_f32: null pointer");
  CB_CHECK_ARG(ld_h >= d && ld_out >= d, CB_E_INVALID, "cb_spmm_csr_weighted_f32: leading dimension smaller than d");
  hipLaunchKernelGGL(k_spmm_weighted, dim3((unsigned)((N * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, w, h, ld_h, out, ld_out,
                     (int)N, (int)d, row_scale, bias, relu);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_spmm_edge_dot_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E, const float* h, int64_t ld_h, const float* g,
                                    int64_t ld_g, int64_t d, float* dw, void* stream) {
  CB_CHECK_ARG(N >= 0 && E >= 0 && d >= 0, CB_E_INVALID, "cb_spmm_edge_dot_f32: negative size");
  CB_CHECK_ARG(N < INT32_MAX && E < INT32_MAX && d < (1 << 20), CB_E_RANGE, "cb_spmm_edge_dot_f32: size exceeds the int32 contract");
  if (N == 0 || E == 0) return CB_OK;
  CB_CHECK_ARG(rowptr && col && h && g && dw && ld_h >= d && ld_g >= d, CB_E_INVALID, "cb_spmm_edge_dot_f32: null pointer or bad ld");
  hipLaunchKernelGGL(k_spmm_edge_dot, dim3((unsigned)((N * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, h, ld_h, g, ld_g, (int)N,
                     (int)d, dw);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
