// The device pieces of the link predictors that take their endpoint rows one at a time (Link_prediction_model/layer.py:108-180, 193-203
// `MLPCatPredictor`, `MLPDotPredictor`, `MLPBilPredictor`, `BilinearPredictor`) on indices instead of gathered rows.
//
//   rows GEMM   C = act(A @ B + bias) with A[r, s D + k] = h[idx[s][r], k], s < nseg: the gather h[idx] (nseg == 1: the first Linear of the MLP-dot /
//               MLP-bilinear predictors over the 2 S endpoint rows, and bilin(x_i)) or the concatenation [h[idx0] | h[idx1]] (nseg == 2: the first
//               Linear of the concatenating predictor).  The gathered-operand GEMM of cb_gather_gemm.h with IndexedRowOperand (cb_limb_core.h) as
//               its A operand: a thin entry here.
//   bilinear    s_e = sum_j (sum_k W[j, k] h[u_e, k]) h[v_e, j]: the main loop of that GEMM over u with the dot against row v_e taken in an epilogue
//               of its own.  No [S, D] matrix is written: a tile leaves one partial sum per row, and a finishing pass adds a row's partials in
//               ascending column-block order.
//   scatter     dH[n] = sum_e ([u_e == n] G0[e, :] + [v_e == n] G1[e, :]): the backward of both gathers; pair_scatter (cb_pair_core.h) with a functor
//               that contributes a row as it stands (CoefAsIs) — sorted keys, float64 sums in ascending contribution order, rounded once.
// An index outside [0, N) is never used as an index: its row of C / its score is NaN, its pair contributes nothing to the scatter, and it counts in an
// int32 status word (one integer atomic per such row, on that path only).
// No float atomics, no host synchronisation inside an entry, two calls with the same inputs give the same bits.
#include "cb_common.h"
#include "cb_gather_gemm.h"
#include "cb_pair_core.h"

namespace cb {

// ---- bilinear pair score --------------------------------------------------------------------------------------------------------------
// The gathered-operand GEMM over u_e (row 0 of pairs; B = W^T, so tile row m holds z_e = W h[u_e]) whose epilogue multiplies by h[v_e] and reduces
// instead of storing.  The accumulators pass through LDS 32 rows at a time as in nn_epilogue; a row's BN columns then sit four per lane in BN / 4
// neighbouring lanes of one wavefront.  A lane adds its four products in ascending column order (fmaf chain), the lanes are added by an xor butterfly (one fixed shape), and
// the row's partial goes to part[m][col_blk].  The lane group of a row is the same wherever the row sits in the tile or the batch, and an
// accumulator's K order does not depend on its row, so a pair's partials depend on the pair alone.
template <int WM, int WN, int WTN>
__global__ void __launch_bounds__(256, (WM == 2 && WTN == 2 ? 3 : 2)) k_pair_bilinear_l3(const float* __restrict__ h, int64_t ld, int64_t n_nodes, int D,
                                                                                        const int32_t* __restrict__ pairs, int64_t S,
                                                                                        const float* __restrict__ B, int64_t ldb, float* __restrict__ part,
                                                                                        int n_row_blocks, int n_col_blocks) {
  using OA = IndexedRowOperand<64 * WM, 1>;
  CB_GATHER_TILE_MAINLOOP(OA, h, ld, n_nodes, D, pairs, S, B, ldb, D, n_row_blocks, n_col_blocks);      // (row 0 of pairs: u)
  constexpr int BN = T::BN, LDB = BN + 4;

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

static inline int bilinear_col_blocks(int64_t D) { return D <= 64 ? 1 : (int)((D + 127) / 128); }      // (the tile choice of launch_gather_nn_limb3)

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
  return nseg == 2 ? gather_gemm_supported<IndexedRowsForm<2>>(h, ld, D, B, ldb, Nout) : nseg == 1 && gather_gemm_supported<IndexedRowsForm<1>>(h, ld, D, B, ldb, Nout);
}

extern "C" int cb_rows_gemm_nn_f32(const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* idx, int32_t nseg, int64_t R, const float* B, int64_t ldb,
                                   float* C, int64_t ldc, float* C2, int64_t ldc2, int64_t Nout, const float* bias, int relu, float drop_p, uint64_t seed,
                                   const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream) {
  CB_CHECK_ARG(nseg == 1 || nseg == 2, CB_E_INVALID, "cb_rows_gemm_nn_f32: %s", IndexedRowsForm<1>::BAD_SIZE);
  return nseg == 2 ? gather_gemm_entry<IndexedRowsForm<2>>("cb_rows_gemm_nn_f32", h, ld, N, D, idx, R, B, ldb, C, ldc, C2, ldc2, Nout, bias, relu, drop_p, seed, seed_dev,
                                                           row0, status, stream)
                   : gather_gemm_entry<IndexedRowsForm<1>>("cb_rows_gemm_nn_f32", h, ld, N, D, idx, R, B, ldb, C, ldc, C2, ldc2, Nout, bias, relu, drop_p, seed, seed_dev,
                                                           row0, status, stream);
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
