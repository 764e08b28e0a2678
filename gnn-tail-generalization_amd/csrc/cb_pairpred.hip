// The device pieces of the link predictors that take their endpoint rows one at a time (Link_prediction_model/layer.py:108-180, 193-203
// `MLPCatPredictor`, `MLPDotPredictor`, `MLPBilPredictor`, `BilinearPredictor`) on indices instead of gathered rows.
//
//   rows GEMM   C = act(A @ B + bias) with A[r, s D + k] = h[idx[s][r], k], s < nseg: the gather h[idx] (nseg == 1: the first Linear of the MLP-dot /
//               MLP-bilinear predictors over the 2 S endpoint rows, and bilin(x_i)) or the concatenation [h[idx0] | h[idx1]] (nseg == 2: the first
//               Linear of the concatenating predictor).  A is formed while it is staged (IndexedRowOperand, cb_limb_core.h) and never written.  K loop,
//               epilogue and tile order are those of k_gemm_nn_l3 (cb_gemm_limb.hip) and the values are staged as they stand, so the result has the bits
//               of cb_gemm_nn_f32 / cb_gemm_nn_drop2_f32 on the materialised A.
//   bilinear    s_e = sum_j (sum_k W[j, k] h[u_e, k]) h[v_e, j]: the rows GEMM over u with the dot against row v_e taken in its epilogue.  No [S, D]
//               matrix is written: a tile leaves one partial sum per row, and a finishing pass adds a row's partials in ascending column-block order.
//   scatter     dH[n] = sum_e ([u_e == n] G0[e, :] + [v_e == n] G1[e, :]): the backward of both gathers; pair_scatter (cb_pair_core.h) with a functor
//               that contributes a row as it stands (CoefAsIs) — sorted keys, float64 sums in ascending contribution order, rounded once.
// An index outside [0, N) is never used as an index: its row of C / its score is NaN, its pair contributes nothing to the scatter, and it counts in an
// int32 status word (one integer atomic per such row, on that path only).
// No float atomics, no host synchronisation inside an entry, two calls with the same inputs give the same bits.
#include <stdlib.h>

#include "cb_common.h"
#include "cb_gemm_core.h"
#include "cb_gemm_limb.h"
#include "cb_limb_core.h"
#include "cb_pair_core.h"

namespace cb {

// ---- rows GEMM ------------------------------------------------------------------------------------------------------------------------
// k_gemm_nn_l3 with IndexedRowOperand as its A operand (the K loop's A base stays &h[0][0]: the operand finds the K step's columns itself).
template <int WM, int WN, int WTN, int EPI, int NSEG>
__global__ void __launch_bounds__(256, (WM == 2 && WTN == 2 ? 3 : 2)) k_rows_gemm_nn_l3(const float* __restrict__ h, int64_t ld, int64_t n_nodes, int D,
                                                                                       const int32_t* __restrict__ idx, int64_t R,
                                                                                       const float* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                                                       int64_t ldc, int N, GemmEpilogue ep, int n_row_blocks,
                                                                                       int n_col_blocks, int c_vec_ok, int32_t* __restrict__ status) {
  constexpr int BM = 64 * WM, BN = 32 * WTN * WN;
  using OA = IndexedRowOperand<BM, NSEG>;
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
  oa.init(idx + m0, R, R - m0, n_nodes, D, t);
  ob.init(ldb, N - n0, t);
  const uint32_t aaddr[2] = {OA::frag_addr(wr * 64, lane), OA::frag_addr(wr * 64 + 32, lane)};
  uint32_t baddr[WTN];
#pragma unroll
  for (int j = 0; j < WTN; ++j) baddr[j] = OB::frag_addr(wc * (32 * WTN) + 32 * j, lane);
  limb_k_loop<WTN, 1, OA, OB>(oa, ob, smem, h, 0, ld, B + n0, (int64_t)KS * ldb, ldb, nullptr, NSEG * D, aaddr, baddr, acc, t);
  nn_epilogue<WM, WN, WTN, false, EPI>(acc, reinterpret_cast<float*>(smem), C, ldc, m0, n0, R, N, ep, c_vec_ok, t);
  // rows of unusable indices (the epilogue ended with a block barrier: its stores to these rows are ordered before these)
  const float qnan = __int_as_float(0x7FC00000);
  const int n_end = N < n0 + BN ? N : n0 + BN;
#pragma unroll
  for (int j = 0; j < OA::NV; ++j) {
    int nd[NSEG];
    bool in;
    if (OA::row_of(idx + m0, R, R - m0, n_nodes, (t >> 2) + 64 * j, nd, in) || !in) continue;
    const int64_t m = m0 + (t >> 2) + 64 * j;      // (< R)
    for (int n = n0 + (t & 3); n < n_end; n += 4) {
      C[m * ldc + n] = qnan;
      if constexpr (EPI == 1) ep.out2[m * ep.ld_out2 + n] = qnan;
    }
    if (col_blk == 0 && (t & 3) == 0) atomicAdd(status, 1);
  }
}

template <int WM, int WN, int WTN, int NSEG>
static int launch_rows_nn(const float* h, int64_t ld, int64_t n_nodes, int64_t D, const int32_t* idx, int64_t R, const float* B, int64_t ldb, float* C,
                          int64_t ldc, int64_t N, const GemmEpilogue& ep, int32_t* status, hipStream_t st) {
  constexpr int BM = 64 * WM, BN = 32 * WTN * WN;
  const int nrb = (int)((R + BM - 1) / BM), ncb = (int)((N + BN - 1) / BN);
  const int64_t groups = (nrb + 7) / 8;
  const int c_vec_ok = aligned16(C) && ldc % 4 == 0;
  const dim3 grid((unsigned)(groups * 8 * ncb));
  if constexpr (WM == 2) {
    if (ep.out2) {      // dual-output epilogue (dropped copy): see rows_dual_eligible
      hipLaunchKernelGGL((k_rows_gemm_nn_l3<WM, WN, WTN, 1, NSEG>), grid, dim3(256), 0, st, h, ld, n_nodes, (int)D, idx, R, B, ldb, C, ldc, (int)N, ep, nrb, ncb,
                         c_vec_ok, status);
      CB_LAUNCH_CHECK();
      return CB_OK;
    }
  }
  hipLaunchKernelGGL((k_rows_gemm_nn_l3<WM, WN, WTN, 0, NSEG>), grid, dim3(256), 0, st, h, ld, n_nodes, (int)D, idx, R, B, ldb, C, ldc, (int)N, ep, nrb, ncb,
                     c_vec_ok, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// The tiles of launch_nn_limb3 by its own rule: 256 x 64 for narrow outputs, 128 x 256 where it fills the chip (one wide tile per CU), 128 x 128
// otherwise.  The pair GEMM of cb_linkpred.hip leaves the wide tile out because its second stream of loads would spill; here both segments come
// through ONE stream of loads (a K step lies in one segment), the operand holds only the indices, and the compiler's resource report
// (-Rpass-analysis=kernel-resource-usage) gives 246 VGPRs for one segment and 250 for two on the wide tile, no scratch, no spill, two wavefronts per
// SIMD as the launch bound asks — so it is used for both.  An output element's K order, and with it its bits, does not depend on the tile.
template <int NSEG>
static int launch_rows_nn_limb3(const float* h, int64_t ld, int64_t n_nodes, int64_t D, const int32_t* idx, int64_t R, const float* B, int64_t ldb, float* C,
                                int64_t ldc, int64_t N, const GemmEpilogue& ep, int32_t* status, hipStream_t st) {
  if (N <= 64) return launch_rows_nn<4, 1, 2, NSEG>(h, ld, n_nodes, D, idx, R, B, ldb, C, ldc, N, ep, status, st);
  if (N > 128 && ((R + 127) / 128) * ((N + 255) / 256) >= 256) return launch_rows_nn<2, 2, 4, NSEG>(h, ld, n_nodes, D, idx, R, B, ldb, C, ldc, N, ep, status, st);
  return launch_rows_nn<2, 2, 2, NSEG>(h, ld, n_nodes, D, idx, R, B, ldb, C, ldc, N, ep, status, st);
}

// the dropped copy leaves in the same epilogue (vector stores on both outputs) on the 128-row tiles
static inline bool rows_dual_eligible(const float* C, int64_t ldc, const float* C2, int64_t ldc2, int64_t N) {
  return N > 64 && aligned16(C) && aligned16(C2) && ldc % 4 == 0 && ldc2 % 4 == 0;
}

// the two-kernel form of the dropped copy: cb_dropout_f32 turns the dropped elements of a NaN row into zeros; the rows of unusable indices are NaN in C2 too
__global__ void __launch_bounds__(256) k_rows_nan_rows(const int32_t* __restrict__ idx, int nseg, int64_t R, int64_t N, float* __restrict__ C2, int64_t ldc2,
                                                       int Nout) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= R) return;
  bool ok = true;
  for (int s = 0; s < nseg; ++s) {
    const int n = idx[s * R + m];
    ok = ok && n >= 0 && n < N;
  }
  if (ok) return;
  for (int n = 0; n < Nout; ++n) C2[m * ldc2 + n] = __int_as_float(0x7FC00000);
}

static inline bool rows_limb3_on() { return getenv("CB_GEMM_PLAIN_F32") == nullptr; }      // (the switch of cb_gemm.hip)

// ---- bilinear pair score --------------------------------------------------------------------------------------------------------------
// The rows GEMM over u_e (B = W^T, so tile row m holds z_e = W h[u_e]) whose epilogue multiplies by h[v_e] and reduces instead of storing.  The
// accumulators pass through LDS 32 rows at a time as in nn_epilogue; a row's BN columns then sit four per lane in BN / 4 neighbouring lanes of one
// wavefront.  A lane adds its four products in ascending column order (fmaf chain), the lanes are added by an xor butterfly (one fixed shape), and
// the row's partial goes to part[m][col_blk].  The lane group of a row is the same wherever the row sits in the tile or the batch, and an
// accumulator's K order does not depend on its row, so a pair's partials depend on the pair alone.
template <int WM, int WN, int WTN>
__global__ void __launch_bounds__(256, (WM == 2 && WTN == 2 ? 3 : 2)) k_pair_bilinear_l3(const float* __restrict__ h, int64_t ld, int64_t n_nodes, int D,
                                                                                        const int32_t* __restrict__ pairs, int64_t S,
                                                                                        const float* __restrict__ B, int64_t ldb, float* __restrict__ part,
                                                                                        int n_row_blocks, int n_col_blocks) {
  constexpr int BM = 64 * WM, BN = 32 * WTN * WN, LDB = BN + 4;
  using OA = IndexedRowOperand<BM, 1>;
  using OB = ColOperand<BN, false>;
  constexpr int SMEM = 2 * (OA::BYTES + OB::BYTES);
  static_assert(32 * LDB * 4 <= SMEM, "epilogue staging must fit");
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
  oa.init(pairs + m0, S, S - m0, n_nodes, D, t);      // (row 0 of pairs: u)
  ob.init(ldb, D - n0, t);
  const uint32_t aaddr[2] = {OA::frag_addr(wr * 64, lane), OA::frag_addr(wr * 64 + 32, lane)};
  uint32_t baddr[WTN];
#pragma unroll
  for (int j = 0; j < WTN; ++j) baddr[j] = OB::frag_addr(wc * (32 * WTN) + 32 * j, lane);
  limb_k_loop<WTN, 1, OA, OB>(oa, ob, smem, h, 0, ld, B + n0, (int64_t)KS * ldb, ldb, nullptr, D, aaddr, baddr, acc, t);

  float* Cs = reinterpret_cast<float*>(smem);      // (every wavefront has passed the K loop's last barrier)
  const int l31 = lane & 31, lh = lane >> 5;
  constexpr int TPR = BN / 4, NV = 32 * TPR / 256;      // lanes per staged row; rows per thread per pass
  static_assert(TPR <= 64 && 64 % TPR == 0, "a row's lanes are neighbours inside one wavefront");
#pragma unroll
  for (int pass = 0; pass < 2 * WM; ++pass) {
    const int g = pass >> 1, ti = pass & 1;
    if (wr == g) {
#pragma unroll
      for (int tj = 0; tj < WTN; ++tj)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) Cs[((reg & 3) + 8 * (reg >> 2) + 4 * lh) * LDB + wc * (32 * WTN) + tj * 32 + l31] = acc[ti][tj][reg];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int id = t + 256 * i;
      const int row = id / TPR, c4 = (id % TPR) * 4;
      const int64_t m = m0 + g * 64 + ti * 32 + row;
      const int n = n0 + c4;
      float p = 0.f;
      if (m < S && n < D) {      // (D % 4 == 0: the lane's four columns lie inside together)
        const int u = pairs[m], v = pairs[S + m];
        if (u >= 0 && u < n_nodes && v >= 0 && v < n_nodes) {
          const float4 z = *reinterpret_cast<const float4*>(Cs + row * LDB + c4);
          const float4 y = *reinterpret_cast<const float4*>(h + (int64_t)v * ld + n);
          p = z.x * y.x;
          p = fmaf(z.y, y.y, p);
          p = fmaf(z.z, y.z, p);
          p = fmaf(z.w, y.w, p);
        }
      }
#pragma unroll
      for (int off = TPR / 2; off > 0; off >>= 1) p += __shfl_xor(p, off);
      if (c4 == 0 && m < S) part[m * n_col_blocks + col_blk] = p;
    }
    __syncthreads();
  }
}

// score of pair e = its partials in ascending column-block order; NaN and one count for an unusable pair
__global__ void __launch_bounds__(256) k_pair_bilinear_finish(const int32_t* __restrict__ pairs, int64_t S, int64_t N, const float* __restrict__ part, int ncb,
                                                              float* __restrict__ scores, int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= S) return;
  int u, v;
  if (!PairSource<false>{pairs, S, nullptr, 0}.get(e, N, u, v)) {
    scores[e] = __int_as_float(0x7FC00000);
    atomicAdd(status, 1);
    return;
  }
  float s = part[e * ncb];
  for (int c = 1; c < ncb; ++c) s += part[e * ncb + c];
  scores[e] = s;
}

static inline int bilinear_col_blocks(int64_t D) { return D <= 64 ? 1 : (int)((D + 127) / 128); }      // (the tile choice of launch_rows_nn_limb3)

template <int WM, int WN, int WTN>
static int launch_pair_bilinear(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* B, int64_t ldb, float* part,
                                hipStream_t st) {
  constexpr int BM = 64 * WM, BN = 32 * WTN * WN;
  const int nrb = (int)((S + BM - 1) / BM), ncb = (int)((D + BN - 1) / BN);
  const int64_t groups = (nrb + 7) / 8;
  hipLaunchKernelGGL((k_pair_bilinear_l3<WM, WN, WTN>), dim3((unsigned)(groups * 8 * ncb)), dim3(256), 0, st, h, ld, N, (int)D, pairs, S, B, ldb, part, nrb, ncb);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb

using namespace cb;

extern "C" int cb_rows_gemm_nn_supported(const float* h, int64_t ld, int64_t D, int32_t nseg, const float* B, int64_t ldb, int64_t Nout) {
  return rows_limb3_on() && h && B && Nout > 0 && D > 0 && (nseg == 1 || nseg == 2) && D % (nseg == 2 ? KS : 4) == 0 && ld >= D && ldb >= Nout &&
                 limb3_nn_eligible(h, ld, B, ldb, Nout, nseg * D)
             ? 1
             : 0;
}

extern "C" int cb_rows_gemm_nn_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* idx, int32_t nseg, int64_t R, const float* B, int64_t ldb,
                                   float* C, int64_t ldc, float* C2, int64_t ldc2, int64_t Nout, const float* bias, int relu, float drop_p, uint64_t seed,
                                   const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream) {
  CB_CHECK_ARG(N > 0 && D > 0 && R >= 0 && Nout > 0 && (nseg == 1 || nseg == 2) && drop_p >= 0.f && drop_p < 1.f && row0 >= 0, CB_E_INVALID,
               "cb_rows_gemm_nn_f32: bad size, nseg (1 or 2) or p");
  CB_CHECK_ARG(N < INT32_MAX && R < INT32_MAX / 2 && Nout < (1 << 24) && D < (1 << 23), CB_E_RANGE, "cb_rows_gemm_nn_f32: size out of range");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_rows_gemm_nn_f32: null pointer (status)");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (R == 0) return CB_OK;
  CB_CHECK_ARG(h && idx && B && C && (C2 || drop_p == 0.f) && ld >= D && ldb >= Nout && ldc >= Nout && (!C2 || ldc2 >= Nout), CB_E_INVALID,
               "cb_rows_gemm_nn_f32: null pointer or leading dimension too small");
  CB_CHECK_ARG(cb_rows_gemm_nn_supported(h, ld, D, nseg, B, ldb, Nout), CB_E_INVALID,
               "cb_rows_gemm_nn_f32: shape / alignment outside the fused form (cb_rows_gemm_nn_supported)");
  GemmEpilogue ep{nullptr, nullptr, 0, bias, relu, nullptr, 0, 0u, 1.f, 0ull, nullptr, 0, R * Nout * 4 > ((int64_t)256 << 20) ? 1 : 0};
  auto launch = [&]() {
    return nseg == 2 ? launch_rows_nn_limb3<2>(h, ld, N, D, idx, R, B, ldb, C, ldc, Nout, ep, status, st)
                     : launch_rows_nn_limb3<1>(h, ld, N, D, idx, R, B, ldb, C, ldc, Nout, ep, status, st);
  };
  if (drop_p > 0.f && rows_dual_eligible(C, ldc, C2, ldc2, Nout)) {
    ep.out2 = C2; ep.ld_out2 = ldc2; ep.thresh = dropout_threshold(drop_p); ep.keep_scale = 1.f / (1.f - drop_p);
    ep.seed = seed; ep.seed_dev = seed_dev; ep.row0 = row0;
    return launch();
  }
  CB_CHECK_ARG(drop_p == 0.f || (ldc == Nout && ldc2 == Nout), CB_E_INVALID,
               "cb_rows_gemm_nn_f32: the two-kernel form of the dropped copy (Nout <= 64 or outputs without float4 alignment) needs contiguous outputs");
  int rc = launch();
  if (rc != CB_OK || drop_p == 0.f) return rc;
  rc = cb_dropout_f32(C, C2, R * Nout, drop_p, seed, seed_dev, row0 * Nout, stream);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_rows_nan_rows, dim3((unsigned)blocks_for(R, 256)), dim3(256), 0, st, idx, (int)nseg, R, N, C2, ldc2, (int)Nout);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_rows_bilinear_supported(const float* h, int64_t ld, int64_t D, const float* Wt, int64_t ldw) {
  return cb_rows_gemm_nn_supported(h, ld, D, 1, Wt, ldw, D);
}

extern "C" size_t cb_rows_bilinear_workspace_bytes(int64_t S, int64_t D) {
  if (S <= 0 || D <= 0 || S >= INT32_MAX / 2 || D >= (1 << 23)) return 0;
  return (size_t)S * (size_t)bilinear_col_blocks(D) * sizeof(float);
}

extern "C" int cb_rows_bilinear_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* Wt, int64_t ldw,
                                    float* scores, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(N > 0 && D > 0 && ld >= D && ldw >= D && S >= 0, CB_E_INVALID, "cb_rows_bilinear_f32: bad size (N > 0, D > 0, ld >= D, ldw >= D, S >= 0 required)");
  CB_CHECK_ARG(N < INT32_MAX && D < (1 << 23) && S < INT32_MAX / 2, CB_E_RANGE, "cb_rows_bilinear_f32: size out of range");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_rows_bilinear_f32: null pointer (status)");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (S == 0) return CB_OK;
  CB_CHECK_ARG(h && pairs && Wt && scores, CB_E_INVALID, "cb_rows_bilinear_f32: null pointer");
  CB_CHECK_ARG(cb_rows_bilinear_supported(h, ld, D, Wt, ldw), CB_E_INVALID,
               "cb_rows_bilinear_f32: shape / alignment outside the fused form (cb_rows_bilinear_supported)");
  CB_CHECK_ARG(ws && aligned16(ws) && ws_bytes >= cb_rows_bilinear_workspace_bytes(S, D), CB_E_WORKSPACE, "cb_rows_bilinear_f32: workspace too small or misaligned");
  float* part = (float*)ws;
  const int rc = D <= 64 ? launch_pair_bilinear<4, 1, 2>(h, ld, N, D, pairs, S, Wt, ldw, part, st)
                         : launch_pair_bilinear<2, 2, 2>(h, ld, N, D, pairs, S, Wt, ldw, part, st);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_pair_bilinear_finish, dim3((unsigned)blocks_for(S, 256)), dim3(256), 0, st, pairs, S, N, (const float*)part, bilinear_col_blocks(D), scores,
                     status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_rows_scatter_f32(int64_t N, int64_t D, const int32_t* pairs, int64_t S, const float* G0, int64_t ld0, const float* G1, int64_t ld1,
                                        float* dh, int64_t ldd, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(N > 0 && D > 0 && S >= 0 && ldd >= D && ld0 >= D && ld1 >= D, CB_E_INVALID,
               "cb_rows_scatter_f32: bad size (N > 0, D > 0, S >= 0, ldd >= D, ld0 >= D, ld1 >= D required)");
  CB_CHECK_ARG(N < INT32_MAX && D < (1 << 24) && S < INT32_MAX / 2, CB_E_RANGE, "cb_rows_scatter_f32: size out of range");
  CB_CHECK_ARG(dh && (S == 0 || (pairs && G0 && G1)), CB_E_INVALID, "cb_rows_scatter_f32: null pointer");
  CB_CHECK_ARG(S == 0 || (ws && ws_bytes >= cb_pair_scatter_workspace_bytes(S)), CB_E_WORKSPACE, "cb_rows_scatter_f32: workspace too small");
  return pair_scatter((const float*)nullptr, 0, N, D, PairSource<false>{pairs, S, nullptr, 0}, CoefAsIs{G0, ld0, G1, ld1}, dh, ldd, ws, ws_bytes,
                      (hipStream_t)stream);
}
