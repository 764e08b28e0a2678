// The two adjacency normalisations of the link-prediction experiment (Link_prediction_model/utils.py:93-106, applied by trainer_link_prediction.py:333-338)
// on an adjacency with one fp32 value per stored edge, in CSR order:
//     adj_normalization:  deg = row sums,  f = 1 / deg (inf -> 0),       w'[j] = f[row of j] * w[j]                         (D^-1 A)
//     gcn_normalization:  deg = row sums,  f = deg^-1/2 (inf -> 0),      w'[j] = (f[row of j] * w[j]) * f[col[j]]           (D^-1/2 A D^-1/2)
// (gcn's set_diag — stored self loops dropped, one (v, v) of value 1 per node — is a change of STRUCTURE and is made before these kernels, ops.adj_normalize.)
// Arithmetic, stated: deg is a float64 sum rounded once to fp32; the factor is computed in float64 from that fp32 value — 1.0 / d, 1.0 / sqrt(d), IEEE
// division and square root, no reciprocal-square-root instruction — and rounded once to fp32; an infinite fp32 result becomes 0.  The product takes two
// fp32 roundings in the order written.
// These run once per graph: plain and deterministic, not tuned.  One wavefront per row; lane l adds the row's values l, l + 64, ... in order, the 64 lane
// sums are combined by a fixed butterfly — the same bits run to run, no atomics on a float.  A negative row sum under the square root is counted in an
// integer status word (the error path only), which the caller reads once.
#include <math.h>

#include "cb_common.h"
#include "cb_spmm_core.h"

namespace cb {

__global__ void __launch_bounds__(256) k_adjnorm_rowsum(const int* __restrict__ rowptr, const float* __restrict__ w, int n_rows, int inv_sqrt,
                                                        float* __restrict__ deg, float* __restrict__ fac, int* __restrict__ status) {
  const int lane = lane_id();
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= n_rows) return;
  const int e0 = rowptr[row], e1 = rowptr[row + 1];
  double s = 0.0;
  for (int e = e0 + lane; e < e1; e += kWave) s += (double)w[e];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) {
    const float d = (float)s;
    const double r = inv_sqrt ? 1.0 / sqrt((double)d) : 1.0 / (double)d;
    float f = (float)r;
    if (isinf(f)) f = 0.f;
    if (inv_sqrt && d < 0.f) atomicAdd(status, 1);      // (f is NaN: the caller raises)
    deg[row] = d;
    fac[row] = f;
  }
}

__global__ void __launch_bounds__(256) k_adjnorm_scale(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w, int n_rows,
                                                       const float* __restrict__ f, const float* __restrict__ g, float* __restrict__ w_out) {
  const int lane = lane_id();
  const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (row >= n_rows) return;
  const int e0 = rowptr[row], e1 = rowptr[row + 1];
  const float fr = f[row];
  for (int e = e0 + lane; e < e1; e += kWave) {
    float t = fr * w[e];
    if (g) t = t * g[col[e] & kColMask];      // (the column ids may carry the hot-source flag)
    w_out[e] = t;
  }
}

}  // namespace cb

using namespace cb;

// deg[v] = fp32(float64 sum of row v's values), fac[v] = fp32(1 / deg) (inv_sqrt = 0) or fp32(1 / sqrt(deg)) (inv_sqrt = 1), inf -> 0.
// status (one int32, zeroed by the caller): the number of rows with a negative sum under inv_sqrt.
extern "C" int cb_adjnorm_rowsum_f64(const int32_t* rowptr, const float* w_csr, int64_t N, int64_t E, int32_t inv_sqrt, float* deg, float* fac,
                                     int32_t* status, void* stream) {
  CB_CHECK_ARG(N >= 0 && E >= 0, CB_E_INVALID, "cb_adjnorm_rowsum_f64: negative size");
  CB_CHECK_ARG(N < INT32_MAX && E < INT32_MAX, CB_E_RANGE, "cb_adjnorm_rowsum_f64: size exceeds the int32 contract");
  if (N == 0) return CB_OK;
  CB_CHECK_ARG(rowptr && deg && fac && status && (E == 0 || w_csr), CB_E_INVALID, "cb_adjnorm_rowsum_f64: null pointer");
  hipLaunchKernelGGL(k_adjnorm_rowsum, dim3((unsigned)((N * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, w_csr, (int)N, (int)inv_sqrt, deg, fac,
                     status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// w_out[j] = (f[row of j] * w_csr[j]) * g[col[j]]; g null: f[row of j] * w_csr[j].  w_out is a buffer of its own.
extern "C" int cb_adjnorm_scale_f32(const int32_t* rowptr, const int32_t* col, const float* w_csr, int64_t N, int64_t E, const float* f, const float* g,
                                    float* w_out, void* stream) {
  CB_CHECK_ARG(N >= 0 && E >= 0, CB_E_INVALID, "cb_adjnorm_scale_f32: negative size");
  CB_CHECK_ARG(N < INT32_MAX && E < INT32_MAX, CB_E_RANGE, "cb_adjnorm_scale_f32: size exceeds the int32 contract");
  if (N == 0 || E == 0) return CB_OK;
  CB_CHECK_ARG(rowptr && col && w_csr && f && w_out, CB_E_INVALID, "cb_adjnorm_scale_f32: null pointer");
  hipLaunchKernelGGL(k_adjnorm_scale, dim3((unsigned)((N * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, w_csr, (int)N, f, g, w_out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
