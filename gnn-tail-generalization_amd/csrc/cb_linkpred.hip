// The decoder of the link-prediction experiment (Link_prediction_model/layer.py:85-106, 182-191 `MLPPredictor`, `DotPredictor`; loss.py:4-30;
// model.py:108-119, 152-158) on index pairs instead of gathered rows.
//
//   pair GEMM   C = act((h[u] * h[v]) @ B + bias): the first Linear of MLPPredictor.  The gathered-operand GEMM of cb_gather_gemm.h with
//               PairRowOperand (cb_limb_core.h) as its A operand: a thin entry here.  The two gathered [S, K] matrices and their product are never
//               written; every product is rounded to fp32 once before the limb split, so the result has the bits of cb_gemm_nn_f32 /
//               cb_gemm_nn_drop2_f32 on the materialised product.
//   pair dot    s_e = <h[u_e], h[v_e]>: k_pair_dot (cb_pair_core.h), the kernel behind the edge-wise loss's scores, with the status count.
//   scatter     dH[n] = sum of c_e * h[v_e] into row u_e and c_e * h[u_e] into row v_e, c_e a scalar (dot predictor) or a row (the MLP predictor's
//               dX) per pair: pair_scatter (cb_pair_core.h), the sorted inverted index that cb_linkp_loss_bwd_f32 runs with its BCE coefficient.
//   rank loss   auc_loss / adaptive_auc_loss / log_rank_loss / ce_loss / info_nce_loss over pos [P] and neg [P, k]: every term in float64 from the
//               fp32 scores by the reference's formula as written (its + 1e-15 included), thread-strided float64 partial sums, a halving tree per
//               block and one over the blocks: one fixed order, rounded once.  The backward writes dpos [P] and dneg [P, k] from a
//               device-resident upstream scalar, each element a float64 sum rounded once.
// A pair with an endpoint outside [0, N) (the -1 of a failed sampler slot) is never used as an index: its score / row of C is NaN, it contributes
// nothing to the scatter, and it counts in an int32 status word (one integer atomic per such pair, on that path only).
// No float atomics, no host synchronisation inside an entry, two calls with the same inputs give the same bits.
#include "cb_common.h"
#include "cb_gather_gemm.h"
#include "cb_pair_core.h"

namespace cb {

// ---- ranking losses -------------------------------------------------------------------------------------------------------------------
constexpr int RL_MAX_BLOCKS = 256;
constexpr double RL_EPS = 1e-15;

__device__ __forceinline__ double rl_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// the terms of positive i: a (every kind) and b (ce_loss: the sum over its negatives, which has its own mean)
__device__ __forceinline__ void rl_row_terms(int kind, const float* __restrict__ pos, const float* __restrict__ neg, const float* __restrict__ weight,
                                             int64_t i, int64_t k, double& a, double& b) {
  const double p = (double)pos[i];
  const float* nr = neg + i * k;
  a = 0.0;
  b = 0.0;
  if (kind == CB_RANK_AUC || kind == CB_RANK_ADAPTIVE_AUC) {
    const double wt = kind == CB_RANK_ADAPTIVE_AUC ? (double)weight[i] : 1.0;      // (weight * square(...) per element, then the sum, as written)
    for (int64_t j = 0; j < k; ++j) {
      const double t = 1.0 - (p - (double)nr[j]);
      a += wt * (t * t);
    }
  } else if (kind == CB_RANK_LOG_RANK) {
    for (int64_t j = 0; j < k; ++j) a += -log(rl_sigmoid(p - (double)nr[j]) + RL_EPS);
  } else if (kind == CB_RANK_CE) {
    a = -log(rl_sigmoid(p) + RL_EPS);
    for (int64_t j = 0; j < k; ++j) b += -log(1.0 - rl_sigmoid((double)nr[j]) + RL_EPS);
  } else {      // CB_RANK_INFO_NCE
    const double pe = exp(p);
    double z = 0.0;
    for (int64_t j = 0; j < k; ++j) z += exp((double)nr[j]);
    a = -log(pe / (pe + z) + RL_EPS);
  }
}

// block b, thread t: rows b * 256 + t, + gridDim.x * 256, ...; part [2][RL_MAX_BLOCKS]
__global__ void __launch_bounds__(256) k_rank_loss_partial(int kind, const float* __restrict__ pos, int64_t P, const float* __restrict__ neg, int64_t k,
                                                           const float* __restrict__ weight, double* __restrict__ part) {
  __shared__ double s[2][256];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < P; i += (int64_t)gridDim.x * 256) {
    double ra, rb;
    rl_row_terms(kind, pos, neg, weight, i, k, ra, rb);
    a += ra;
    b += rb;
  }
  s[0][t] = a;
  s[1][t] = b;
  block_tree_f64(s, t);
  if (t == 0) {
    part[blockIdx.x] = s[0][0];
    part[RL_MAX_BLOCKS + blockIdx.x] = s[1][0];
  }
}

__global__ void __launch_bounds__(256) k_rank_loss_finish(int kind, int64_t P, int64_t k, const double* __restrict__ part, int nb, float* __restrict__ loss) {
  __shared__ double s[2][256];
  const int t = threadIdx.x;
  s[0][t] = t < nb ? part[t] : 0.0;
  s[1][t] = t < nb ? part[RL_MAX_BLOCKS + t] : 0.0;
  block_tree_f64(s, t);
  if (t == 0) {
    const double dP = (double)P, dS = (double)P * (double)k, sa = s[0][0], sb = s[1][0];
    double r;
    if (kind == CB_RANK_AUC || kind == CB_RANK_ADAPTIVE_AUC) r = sa;
    else if (kind == CB_RANK_LOG_RANK) r = sa / dS;
    else if (kind == CB_RANK_CE) r = sa / dP + sb / dS;
    else r = sa / dP;
    loss[0] = (float)r;
  }
}

// One thread per positive: dpos[i] and its k elements of dneg (autograd of the formulas above; sigmoid' = (1 - y) y as autograd forms it).
__global__ void __launch_bounds__(256) k_rank_loss_bwd(int kind, const float* __restrict__ pos, int64_t P, const float* __restrict__ neg, int64_t k,
                                                       const float* __restrict__ weight, const float* __restrict__ gp, float* __restrict__ dpos,
                                                       float* __restrict__ dneg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const double g = (double)gp[0], p = (double)pos[i];
  const double dP = (double)P, dS = (double)P * (double)k;
  const float* nr = neg + i * k;
  float* dn = dneg + i * k;
  double dp = 0.0;
  if (kind == CB_RANK_AUC || kind == CB_RANK_ADAPTIVE_AUC) {
    const double c = kind == CB_RANK_ADAPTIVE_AUC ? g * (double)weight[i] : g;
    for (int64_t j = 0; j < k; ++j) {
      const double q = c * 2.0 * (1.0 - (p - (double)nr[j]));
      dn[j] = (float)q;
      dp -= q;
    }
  } else if (kind == CB_RANK_LOG_RANK) {
    for (int64_t j = 0; j < k; ++j) {
      const double y = rl_sigmoid(p - (double)nr[j]);
      const double q = (g / dS) * ((1.0 - y) * y) / (y + RL_EPS);
      dn[j] = (float)q;
      dp -= q;
    }
  } else if (kind == CB_RANK_CE) {
    const double y = rl_sigmoid(p);
    dp = -(g / dP) * ((1.0 - y) * y) / (y + RL_EPS);
    for (int64_t j = 0; j < k; ++j) {
      const double yn = rl_sigmoid((double)nr[j]);
      dn[j] = (float)((g / dS) * ((1.0 - yn) * yn) / ((1.0 - yn) + RL_EPS));
    }
  } else {      // CB_RANK_INFO_NCE
    const double pe = exp(p);
    double z = 0.0;
    for (int64_t j = 0; j < k; ++j) z += exp((double)nr[j]);
    const double s = pe + z, c = -(g / dP) / (pe / s + RL_EPS);      // dL / dr, r = pe / s
    dp = c * (pe * z) / (s * s);
    for (int64_t j = 0; j < k; ++j) dn[j] = (float)(-c * (pe * exp((double)nr[j])) / (s * s));
  }
  dpos[i] = (float)dp;
}

}  // namespace cb

using namespace cb;

extern "C" int cb_pair_gemm_nn_supported(const float* h, int64_t ld, const float* B, int64_t ldb, int64_t Nout, int64_t K) {
  return gather_gemm_supported<PairProductForm>(h, ld, K, B, ldb, Nout);
}

extern "C" int cb_pair_gemm_nn_f32(const float* h, int64_t ld, int64_t N, const int32_t* pairs, int64_t S, const float* B, int64_t ldb, float* C, int64_t ldc,
                                   float* C2, int64_t ldc2, int64_t Nout, int64_t K, const float* bias, int relu, float drop_p, uint64_t seed,
                                   const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream) {
  return gather_gemm_entry<PairProductForm>("cb_pair_gemm_nn_f32", h, ld, N, K, pairs, S, B, ldb, C, ldc, C2, ldc2, Nout, bias, relu, drop_p, seed, seed_dev, row0,
                                            status, stream);
}

extern "C" int cb_pair_dot_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, float* scores, int32_t* status,
                               void* stream) {
  CB_PAIR_CHECK_SIZES("cb_pair_dot_f32", S, S >= 0, "S >= 0");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_pair_dot_f32: null pointer (status)");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (S == 0) return CB_OK;
  CB_CHECK_ARG(h && pairs && scores, CB_E_INVALID, "cb_pair_dot_f32: null pointer");
  return launch_pair_dot(h, ld, N, D, PairSource<false>{pairs, S, nullptr, 0}, scores, status, st);
}

extern "C" size_t cb_pair_scatter_workspace_bytes(int64_t S) {
  if (S <= 0 || S >= INT32_MAX / 2) return 0;
  return pair_scatter_ws_bytes(S);
}

extern "C" int cb_pair_scatter_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* coef, int64_t ldcoef,
                                   float* dh, int64_t ldd, void* ws, size_t ws_bytes, void* stream) {
  CB_PAIR_CHECK_SIZES("cb_pair_scatter_f32", S, S >= 0, "S >= 0");
  CB_CHECK_ARG(ldd >= D && (ldcoef == 0 || ldcoef >= D), CB_E_INVALID, "cb_pair_scatter_f32: ldd >= D and ldcoef == 0 (a scalar per pair) or >= D required");
  CB_CHECK_ARG(h && dh && (S == 0 || (pairs && coef)), CB_E_INVALID, "cb_pair_scatter_f32: null pointer");
  CB_CHECK_ARG(S == 0 || (ws && ws_bytes >= cb_pair_scatter_workspace_bytes(S)), CB_E_WORKSPACE, "cb_pair_scatter_f32: workspace too small");
  const PairSource<false> src{pairs, S, nullptr, 0};
  if (ldcoef) return pair_scatter(h, ld, N, D, src, CoefRows{coef, ldcoef}, dh, ldd, ws, ws_bytes, (hipStream_t)stream);
  return pair_scatter(h, ld, N, D, src, CoefScalar{coef}, dh, ldd, ws, ws_bytes, (hipStream_t)stream);
}

#define RL_CHECK(name)                                                                                                                      \
  CB_CHECK_ARG(kind >= CB_RANK_AUC && kind <= CB_RANK_INFO_NCE, CB_E_INVALID, name ": unknown kind");                                      \
  CB_CHECK_ARG(P >= 1 && k >= 1, CB_E_INVALID, name ": P >= 1 positives and k >= 1 negatives per positive required");                      \
  CB_CHECK_ARG(P < INT32_MAX / 2 && k < INT32_MAX / 2 && P * k < INT32_MAX / 2, CB_E_RANGE, name ": size out of range");                   \
  CB_CHECK_ARG(pos && neg && (weight || kind != CB_RANK_ADAPTIVE_AUC), CB_E_INVALID, name ": null pointer")

extern "C" size_t cb_rank_loss_workspace_bytes(void) { return 2 * RL_MAX_BLOCKS * sizeof(double); }

extern "C" int cb_rank_loss_fwd_f32(int32_t kind, const float* pos, int64_t P, const float* neg, int64_t k, const float* weight, float* loss, void* ws,
                                    size_t ws_bytes, void* stream) {
  RL_CHECK("cb_rank_loss_fwd_f32");
  CB_CHECK_ARG(loss, CB_E_INVALID, "cb_rank_loss_fwd_f32: null pointer (loss)");
  CB_CHECK_ARG(ws && (uintptr_t)ws % 8 == 0 && ws_bytes >= cb_rank_loss_workspace_bytes(), CB_E_WORKSPACE, "cb_rank_loss_fwd_f32: workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)((P + 255) / 256 < RL_MAX_BLOCKS ? (P + 255) / 256 : RL_MAX_BLOCKS);
  hipLaunchKernelGGL(k_rank_loss_partial, dim3((unsigned)nb), dim3(256), 0, st, (int)kind, pos, P, neg, k, weight, (double*)ws);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rank_loss_finish, dim3(1), dim3(256), 0, st, (int)kind, P, k, (const double*)ws, nb, loss);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_rank_loss_bwd_f32(int32_t kind, const float* pos, int64_t P, const float* neg, int64_t k, const float* weight, const float* g,
                                    float* dpos, float* dneg, void* stream) {
  RL_CHECK("cb_rank_loss_bwd_f32");
  CB_CHECK_ARG(g && dpos && dneg, CB_E_INVALID, "cb_rank_loss_bwd_f32: null pointer");
  hipLaunchKernelGGL(k_rank_loss_bwd, dim3((unsigned)blocks_for(P, 256)), dim3(256), 0, (hipStream_t)stream, (int)kind, pos, P, neg, k, weight, g, dpos, dneg);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
