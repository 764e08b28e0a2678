// The decoder of the link-prediction experiment (Link_prediction_model/layer.py:85-106, 182-191 `MLPPredictor`, `DotPredictor`; loss.py:4-30;
// model.py:108-119, 152-158) on index pairs instead of gathered rows.
//
//   pair GEMM   C = act((h[u] * h[v]) @ B + bias): the first Linear of MLPPredictor with its A operand formed while it is staged
//               (PairRowOperand, cb_limb_core.h).  The two gathered [S, K] matrices and their product are never written.  K loop, epilogue and
//               tile order are those of k_gemm_nn_l3 (cb_gemm_limb.hip), and every product is rounded to fp32 once before the limb split, so the
//               result has the bits of cb_gemm_nn_f32 / cb_gemm_nn_drop2_f32 on the materialised product.
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
#include <stdlib.h>

#include "cb_common.h"
#include "cb_gemm_core.h"
#include "cb_gemm_limb.h"
#include "cb_limb_core.h"
#include "cb_pair_core.h"

namespace cb {

// ---- pair GEMM ------------------------------------------------------------------------------------------------------------------------
// k_gemm_nn_l3 with PairRowOperand as its A operand; register prefetch depth 1 (the operand holds the second row's quads).
template <int WM, int WN, int WTN, int EPI>
__global__ void __launch_bounds__(256, (WM == 2 && WTN == 2 ? 3 : 2)) k_pair_gemm_nn_l3(const float* __restrict__ h, int64_t ld, int64_t n_nodes,
                                                                                       const int32_t* __restrict__ pairs, int64_t S,
                                                                                       const float* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                                                       int64_t ldc, int N, int K, GemmEpilogue ep, int n_row_blocks,
                                                                                       int n_col_blocks, int c_vec_ok, int32_t* __restrict__ status) {
  constexpr int BM = 64 * WM, BN = 32 * WTN * WN;
  using OA = PairRowOperand<BM>;
  using OB = ColOperand<BN, false>;
  constexpr int SMEM = 2 * (OA::BYTES + OB::BYTES);
  static_assert(32 * (BN + 4) * 4 <= SMEM, "epilogue staging must fit");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  const int per_group = 8 * n_col_blocks;   // XCD-aware order, see k_gemm_nn
  const int grp = blockIdx.x / per_group, r = blockIdx.x % per_group;
  const int row_blk = grp * 8 + (r & 7), col_blk = r >> 3;
  if (row_blk >= n_row_blocks) return;
  const int64_t m0 = (int64_t)row_blk * BM;
  const int n0 = col_blk * BN;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w / WN, wc = w % WN;

  f32x16 acc[2][WTN];
  zero_acc_n<WTN>(acc);
  OA oa;
  OB ob;
  oa.init(pairs + m0, S, S - m0, n_nodes, t);
  ob.init(ldb, N - n0, t);
  const uint32_t aaddr[2] = {OA::frag_addr(wr * 64, lane), OA::frag_addr(wr * 64 + 32, lane)};
  uint32_t baddr[WTN];
#pragma unroll
  for (int j = 0; j < WTN; ++j) baddr[j] = OB::frag_addr(wc * (32 * WTN) + 32 * j, lane);
  limb_k_loop<WTN, 1, OA, OB>(oa, ob, smem, h, KS, ld, B + n0, (int64_t)KS * ldb, ldb, nullptr, K, aaddr, baddr, acc, t);
  nn_epilogue<WM, WN, WTN, false, EPI>(acc, reinterpret_cast<float*>(smem), C, ldc, m0, n0, S, N, ep, c_vec_ok, t);
  // rows of unusable pairs (the epilogue ended with a block barrier: its stores to these rows are ordered before these)
  const float qnan = __int_as_float(0x7FC00000);
  const int n_end = N < n0 + BN ? N : n0 + BN;
#pragma unroll
  for (int j = 0; j < OA::NV; ++j) {
    int u, v;
    bool in;
    if (OA::pair_of(pairs + m0, S, S - m0, n_nodes, (t >> 2) + 64 * j, u, v, in) || !in) continue;
    const int64_t m = m0 + (t >> 2) + 64 * j;      // (< S)
    for (int n = n0 + (t & 3); n < n_end; n += 4) {
      C[m * ldc + n] = qnan;
      if constexpr (EPI == 1) ep.out2[m * ep.ld_out2 + n] = qnan;
    }
    if (col_blk == 0 && (t & 3) == 0) atomicAdd(status, 1);
  }
}

template <int WM, int WN, int WTN>
static int launch_pair_nn(const float* h, int64_t ld, int64_t n_nodes, const int32_t* pairs, int64_t S, const float* B, int64_t ldb, float* C, int64_t ldc,
                          int64_t N, int64_t K, const GemmEpilogue& ep, int32_t* status, hipStream_t st) {
  constexpr int BM = 64 * WM, BN = 32 * WTN * WN;
  const int nrb = (int)((S + BM - 1) / BM), ncb = (int)((N + BN - 1) / BN);
  const int64_t groups = (nrb + 7) / 8;
  const int c_vec_ok = aligned16(C) && ldc % 4 == 0;
  const dim3 grid((unsigned)(groups * 8 * ncb));
  if constexpr (WM == 2) {
    if (ep.out2) {      // dual-output epilogue (dropped copy): see pair_dual_eligible
      hipLaunchKernelGGL((k_pair_gemm_nn_l3<WM, WN, WTN, 1>), grid, dim3(256), 0, st, h, ld, n_nodes, pairs, S, B, ldb, C, ldc, (int)N, (int)K, ep, nrb, ncb,
                         c_vec_ok, status);
      CB_LAUNCH_CHECK();
      return CB_OK;
    }
  }
  hipLaunchKernelGGL((k_pair_gemm_nn_l3<WM, WN, WTN, 0>), grid, dim3(256), 0, st, h, ld, n_nodes, pairs, S, B, ldb, C, ldc, (int)N, (int)K, ep, nrb, ncb, c_vec_ok,
                     status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// 256 x 64 tiles for narrow outputs, 128 x 128 otherwise.  The 128 x 256 tile of launch_nn_limb3 is not used here: it sits at the 256-register cap
// with the plain row operand, and the second stream of loads (8 registers per lane) would spill.  An output element's K order, and with it its bits, does
// not depend on the tile.
static int launch_pair_nn_limb3(const float* h, int64_t ld, int64_t n_nodes, const int32_t* pairs, int64_t S, const float* B, int64_t ldb, float* C,
                                int64_t ldc, int64_t N, int64_t K, const GemmEpilogue& ep, int32_t* status, hipStream_t st) {
  if (N <= 64) return launch_pair_nn<4, 1, 2>(h, ld, n_nodes, pairs, S, B, ldb, C, ldc, N, K, ep, status, st);
  return launch_pair_nn<2, 2, 2>(h, ld, n_nodes, pairs, S, B, ldb, C, ldc, N, K, ep, status, st);
}

// the dropped copy leaves in the same epilogue (vector stores on both outputs) on the 128 x 128 tile
static inline bool pair_dual_eligible(const float* C, int64_t ldc, const float* C2, int64_t ldc2, int64_t N) {
  return N > 64 && aligned16(C) && aligned16(C2) && ldc % 4 == 0 && ldc2 % 4 == 0;
}

// the two-kernel form of the dropped copy: cb_dropout_f32 turns the dropped elements of a NaN row into zeros; the rows of unusable pairs are NaN in C2 too
__global__ void __launch_bounds__(256) k_pair_nan_rows(const int32_t* __restrict__ pairs, int64_t S, int64_t N, float* __restrict__ C2, int64_t ldc2, int Nout) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= S) return;
  int u, v;
  if (PairSource<false>{pairs, S, nullptr, 0}.get(m, N, u, v)) return;
  for (int n = 0; n < Nout; ++n) C2[m * ldc2 + n] = __int_as_float(0x7FC00000);
}

static inline bool pair_limb3_on() { return getenv("CB_GEMM_PLAIN_F32") == nullptr; }      // (the switch of cb_gemm.hip)

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
  return pair_limb3_on() && h && B && Nout > 0 && ld >= K && ldb >= Nout && limb3_nn_eligible(h, ld, B, ldb, Nout, K) ? 1 : 0;
}

extern "C" int cb_pair_gemm_nn_f32(const float* h, int64_t ld, int64_t N, const int32_t* pairs, int64_t S, const float* B, int64_t ldb, float* C, int64_t ldc,
                                   float* C2, int64_t ldc2, int64_t Nout, int64_t K, const float* bias, int relu, float drop_p, uint64_t seed,
                                   const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream) {
  CB_CHECK_ARG(N > 0 && S >= 0 && Nout > 0 && K > 0 && drop_p >= 0.f && drop_p < 1.f && row0 >= 0, CB_E_INVALID, "cb_pair_gemm_nn_f32: bad size or p");
  CB_CHECK_ARG(N < INT32_MAX && S < INT32_MAX / 2 && Nout < (1 << 24) && K < (1 << 24), CB_E_RANGE, "cb_pair_gemm_nn_f32: size out of range");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_pair_gemm_nn_f32: null pointer (status)");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (S == 0) return CB_OK;
  CB_CHECK_ARG(h && pairs && B && C && (C2 || drop_p == 0.f) && ld >= K && ldb >= Nout && ldc >= Nout && (!C2 || ldc2 >= Nout), CB_E_INVALID,
               "cb_pair_gemm_nn_f32: null pointer or leading dimension too small");
  CB_CHECK_ARG(cb_pair_gemm_nn_supported(h, ld, B, ldb, Nout, K), CB_E_INVALID,
               "cb_pair_gemm_nn_f32: shape / alignment outside the fused form (cb_pair_gemm_nn_supported)");
  GemmEpilogue ep{nullptr, nullptr, 0, bias, relu, nullptr, 0, 0u, 1.f, 0ull, nullptr, 0, S * Nout * 4 > ((int64_t)256 << 20) ? 1 : 0};
  if (drop_p > 0.f && pair_dual_eligible(C, ldc, C2, ldc2, Nout)) {
    ep.out2 = C2; ep.ld_out2 = ldc2; ep.thresh = dropout_threshold(drop_p); ep.keep_scale = 1.f / (1.f - drop_p);
    ep.seed = seed; ep.seed_dev = seed_dev; ep.row0 = row0;
    return launch_pair_nn_limb3(h, ld, N, pairs, S, B, ldb, C, ldc, Nout, K, ep, status, st);
  }
  CB_CHECK_ARG(drop_p == 0.f || (ldc == Nout && ldc2 == Nout), CB_E_INVALID,
               "cb_pair_gemm_nn_f32: the two-kernel form of the dropped copy (Nout <= 64 or outputs without float4 alignment) needs contiguous outputs");
  int rc = launch_pair_nn_limb3(h, ld, N, pairs, S, B, ldb, C, ldc, Nout, K, ep, status, st);
  if (rc != CB_OK || drop_p == 0.f) return rc;
  rc = cb_dropout_f32(C, C2, S * Nout, drop_p, seed, seed_dev, row0 * Nout, stream);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_pair_nan_rows, dim3((unsigned)blocks_for(S, 256)), dim3(256), 0, st, pairs, S, N, C2, ldc2, (int)Nout);
  CB_LAUNCH_CHECK();
  return CB_OK;
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
