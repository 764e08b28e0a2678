// The three-limb NN GEMM whose A operand is gathered through an index array while it is staged: C = act(A @ B + bias) with a tile row of A formed from
// the rows h[idx[s][r]], s < NIDX, by one of the gathered operands of cb_limb_core.h — PairRowOperand (h[u] * h[v]: cb_pair_gemm_nn_f32,
// cb_linkpred.hip) or IndexedRowOperand (h[i] or [h[i] | h[j]]: cb_rows_gemm_nn_f32 and the bilinear score, cb_pairpred.hip).  A is never written.
// K loop, epilogue and tile order are those of k_gemm_nn_l3 (cb_gemm_limb.hip), and the operands stage the fp32 values of the materialised A, so the
// result has the bits of cb_gemm_nn_f32 / cb_gemm_nn_drop2_f32 on it.  An output element's K order, and with it its bits, does not depend on the tile.
// A row with an index outside [0, N) is never used as an index: its row of C is NaN and it counts in an int32 status word (one integer atomic per
// such row, on that path only).
#pragma once
#include <string.h>

#include "cb_common.h"
#include "cb_gemm_core.h"
#include "cb_gemm_limb.h"
#include "cb_limb_core.h"

namespace cb {

// What an entry fixes: its A operand by tile rows, its limits on the row length D of h, and the text of its first argument check.
struct PairProductForm {
  template <int R> using Operand = PairRowOperand<R>;
  static constexpr int D_MULT = 4;
  static constexpr int64_t D_LIMIT = 1 << 24;
  static constexpr const char* BAD_SIZE = "bad size or p";
};
template <int NSEG>
struct IndexedRowsForm {
  template <int R> using Operand = IndexedRowOperand<R, NSEG>;
  static constexpr int D_MULT = NSEG == 2 ? KS : 4;      // (two segments: no K step straddles the seam)
  static constexpr int64_t D_LIMIT = 1 << 23;
  static constexpr const char* BAD_SIZE = "bad size, nseg (1 or 2) or p";
};

template <int WM, int WN, int WTN, class OA>
struct GatherTile {
  static constexpr int BM = 64 * WM, BN = 32 * WTN * WN;
  static_assert(OA::NV == WM, "the operand's tile rows");
  using OB = ColOperand<BN, false>;
  static constexpr int SMEM = 2 * (OA::BYTES + OB::BYTES);
  static_assert(32 * (BN + 4) * 4 <= SMEM, "epilogue staging must fit");
};

// The main loop of a kernel with template parameters WM, WN, WTN: block -> tile in the XCD-aware order of k_gemm_nn, the early return of the grid's
// surplus blocks, operand set-up, fragment addresses and the K loop (register prefetch depth 1: PairRowOperand holds its second row's quads; the A
// base is &h[0][0] plus OA::A_STEP per K step).  idx [OA::NIDX][Rn], D = row length of h, N = columns of B.  Leaves in the kernel's scope: the tile
// T, smem, the thread's t / lane / wr / wc, the tile origin m0 / n0 / col_blk and the accumulators acc.
// A macro and not a __forceinline__ function on purpose: every function form tried hands the register allocator the same values in another order,
// and the 128 x 256 instantiations then spill (profiles/gather_gemm.md); this form compiles to the instructions of a body written in the kernel.
#define CB_GATHER_TILE_MAINLOOP(OA, h, ld, n_nodes, D, idx, Rn, B, ldb, N, n_row_blocks, n_col_blocks)                                        \
  using T = GatherTile<WM, WN, WTN, OA>;                                                                                                      \
  using OB = typename T::OB;                                                                                                                  \
  __shared__ __attribute__((aligned(16))) char smem[T::SMEM];                                                                                 \
  const int per_group = 8 * (n_col_blocks);                                                                                                   \
  const int grp = blockIdx.x / per_group, r = blockIdx.x % per_group;                                                                         \
  const int row_blk = grp * 8 + (r & 7), col_blk = r >> 3;                                                                                    \
  if (row_blk >= (n_row_blocks)) return;                                                                                                      \
  const int64_t m0 = (int64_t)row_blk * T::BM;                                                                                                \
  const int n0 = col_blk * T::BN;                                                                                                             \
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w / WN, wc = w % WN;                                                             \
  f32x16 acc[2][WTN];                                                                                                                         \
  zero_acc_n<WTN>(acc);                                                                                                                       \
  OA oa;                                                                                                                                      \
  OB ob;                                                                                                                                      \
  oa.init((idx) + m0, Rn, (Rn) - m0, n_nodes, D, t);                                                                                          \
  ob.init(ldb, (N) - n0, t);                                                                                                                  \
  const uint32_t aaddr[2] = {OA::frag_addr(wr * 64, lane), OA::frag_addr(wr * 64 + 32, lane)};                                                \
  uint32_t baddr[WTN];                                                                                                                        \
  _Pragma("unroll") for (int j = 0; j < WTN; ++j) baddr[j] = OB::frag_addr(wc * (32 * WTN) + 32 * j, lane);                                   \
  limb_k_loop<WTN, 1, OA, OB>(oa, ob, smem, h, OA::A_STEP, ld, (B) + n0, (int64_t)KS * (ldb), ldb, nullptr, OA::ktot(D), aaddr, baddr, acc, t)

template <int WM, int WN, int WTN, int EPI, class OA>
__global__ void __launch_bounds__(256, (WM == 2 && WTN == 2 ? 3 : 2)) k_gather_gemm_nn_l3(const float* __restrict__ h, int64_t ld, int64_t n_nodes, int D,
                                                                                         const int32_t* __restrict__ idx, int64_t R,
                                                                                         const float* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                                                         int64_t ldc, int N, GemmEpilogue ep, int n_row_blocks,
                                                                                         int n_col_blocks, int c_vec_ok, int32_t* __restrict__ status) {
  CB_GATHER_TILE_MAINLOOP(OA, h, ld, n_nodes, D, idx, R, B, ldb, N, n_row_blocks, n_col_blocks);
  nn_epilogue<WM, WN, WTN, false, EPI>(acc, reinterpret_cast<float*>(smem), C, ldc, m0, n0, R, N, ep, c_vec_ok, t);
  // rows of unusable indices (the epilogue ended with a block barrier: its stores to these rows are ordered before these)
  const float qnan = __int_as_float(0x7FC00000);
  const int n_end = N < n0 + T::BN ? N : n0 + T::BN;
#pragma unroll
  for (int j = 0; j < OA::NV; ++j) {
    int nd[OA::NIDX];
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

template <int WM, int WN, int WTN, class Form>
static int launch_gather_nn(const float* h, int64_t ld, int64_t n_nodes, int64_t D, const int32_t* idx, int64_t R, const float* B, int64_t ldb, float* C,
                            int64_t ldc, int64_t N, const GemmEpilogue& ep, int32_t* status, hipStream_t st) {
  using OA = typename Form::template Operand<64 * WM>;
  using T = GatherTile<WM, WN, WTN, OA>;
  const int nrb = (int)((R + T::BM - 1) / T::BM), ncb = (int)((N + T::BN - 1) / T::BN);
  const int64_t groups = (nrb + 7) / 8;
  const int c_vec_ok = aligned16(C) && ldc % 4 == 0;
  const dim3 grid((unsigned)(groups * 8 * ncb));
  if constexpr (WM == 2) {
    if (ep.out2) {      // dual-output epilogue (dropped copy): see gather_dual_eligible
      hipLaunchKernelGGL((k_gather_gemm_nn_l3<WM, WN, WTN, 1, OA>), grid, dim3(256), 0, st, h, ld, n_nodes, (int)D, idx, R, B, ldb, C, ldc, (int)N, ep, nrb, ncb,
                         c_vec_ok, status);
      CB_LAUNCH_CHECK();
      return CB_OK;
    }
  }
  hipLaunchKernelGGL((k_gather_gemm_nn_l3<WM, WN, WTN, 0, OA>), grid, dim3(256), 0, st, h, ld, n_nodes, (int)D, idx, R, B, ldb, C, ldc, (int)N, ep, nrb, ncb,
                     c_vec_ok, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// The tiles of launch_nn_limb3 by its own rule: 256 x 64 for narrow outputs, 128 x 256 where the operand allows it (OA::WIDE_TILE) and it fills the
// chip (one wide tile per CU), 128 x 128 otherwise.
template <class Form>
static int launch_gather_nn_limb3(const float* h, int64_t ld, int64_t n_nodes, int64_t D, const int32_t* idx, int64_t R, const float* B, int64_t ldb, float* C,
                                  int64_t ldc, int64_t N, const GemmEpilogue& ep, int32_t* status, hipStream_t st) {
  if (N <= 64) return launch_gather_nn<4, 1, 2, Form>(h, ld, n_nodes, D, idx, R, B, ldb, C, ldc, N, ep, status, st);
  if constexpr (Form::template Operand<128>::WIDE_TILE) {
    if (N > 128 && ((R + 127) / 128) * ((N + 255) / 256) >= 256) return launch_gather_nn<2, 2, 4, Form>(h, ld, n_nodes, D, idx, R, B, ldb, C, ldc, N, ep, status, st);
  }
  return launch_gather_nn<2, 2, 2, Form>(h, ld, n_nodes, D, idx, R, B, ldb, C, ldc, N, ep, status, st);
}

// the dropped copy leaves in the same epilogue (vector stores on both outputs) on the 128-row tiles
static inline bool gather_dual_eligible(const float* C, int64_t ldc, const float* C2, int64_t ldc2, int64_t N) {
  return N > 64 && aligned16(C) && aligned16(C2) && ldc % 4 == 0 && ldc2 % 4 == 0;
}

// the two-kernel form of the dropped copy: cb_dropout_f32 turns the dropped elements of a NaN row into zeros; the rows of unusable indices are NaN in C2 too
static __global__ void __launch_bounds__(256) k_gather_nan_rows(const int32_t* __restrict__ idx, int nidx, int64_t R, int64_t N, float* __restrict__ C2,
                                                                int64_t ldc2, int Nout) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= R) return;
  bool ok = true;
  for (int s = 0; s < nidx; ++s) {
    const int n = idx[s * R + m];
    ok = ok && n >= 0 && n < N;
  }
  if (ok) return;
  for (int n = 0; n < Nout; ++n) C2[m * ldc2 + n] = __int_as_float(0x7FC00000);
}

template <class Form>
static int gather_gemm_supported(const float* h, int64_t ld, int64_t D, const float* B, int64_t ldb, int64_t Nout) {
  return limb3_on() && h && B && Nout > 0 && D > 0 && D % Form::D_MULT == 0 && ld >= D && ldb >= Nout &&
                 limb3_nn_eligible(h, ld, B, ldb, Nout, Form::template Operand<64>::ktot(D))
             ? 1
             : 0;
}

// The body of an extern "C" entry (`who`: its name, for the messages).  idx [NIDX][R]; C2 receives dropout_p(C) when drop_p > 0.
template <class Form>
static int gather_gemm_entry(const char* who, const float* h, int64_t ld, int64_t N, int64_t D, const int32_t* idx, int64_t R, const float* B, int64_t ldb,
                             float* C, int64_t ldc, float* C2, int64_t ldc2, int64_t Nout, const float* bias, int relu, float drop_p, uint64_t seed,
                             const uint64_t* seed_dev, int64_t row0, int32_t* status, void* stream) {
  CB_CHECK_ARG(N > 0 && D > 0 && R >= 0 && Nout > 0 && drop_p >= 0.f && drop_p < 1.f && row0 >= 0, CB_E_INVALID, "%s: %s", who, Form::BAD_SIZE);
  CB_CHECK_ARG(N < INT32_MAX && R < INT32_MAX / 2 && Nout < (1 << 24) && D < Form::D_LIMIT, CB_E_RANGE, "%s: size out of range", who);
  CB_CHECK_ARG(status, CB_E_INVALID, "%s: null pointer (status)", who);
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (R == 0) return CB_OK;
  CB_CHECK_ARG(h && idx && B && C && (C2 || drop_p == 0.f) && ld >= D && ldb >= Nout && ldc >= Nout && (!C2 || ldc2 >= Nout), CB_E_INVALID,
               "%s: null pointer or leading dimension too small", who);
  CB_CHECK_ARG(gather_gemm_supported<Form>(h, ld, D, B, ldb, Nout), CB_E_INVALID, "%s: shape / alignment outside the fused form (%.*s_supported)", who,
               (int)strlen(who) - 4, who);      // (the predicate's name: the entry's with _supported for _f32)
  GemmEpilogue ep = epilogue(nullptr, nullptr, 0, bias, relu, gemm_nt_store(R, Nout));
  if (drop_p > 0.f && gather_dual_eligible(C, ldc, C2, ldc2, Nout)) {
    set_dropped_copy(ep, C2, ldc2, drop_p, seed, seed_dev, row0);
    return launch_gather_nn_limb3<Form>(h, ld, N, D, idx, R, B, ldb, C, ldc, Nout, ep, status, st);
  }
  CB_CHECK_ARG(drop_p == 0.f || (ldc == Nout && ldc2 == Nout), CB_E_INVALID,
               "%s: the two-kernel form of the dropped copy (Nout <= 64 or outputs without float4 alignment) needs contiguous outputs", who);
  int rc = launch_gather_nn_limb3<Form>(h, ld, N, D, idx, R, B, ldb, C, ldc, Nout, ep, status, st);
  if (rc != CB_OK || drop_p == 0.f) return rc;
  rc = cb_dropout_f32(C, C2, R * Nout, drop_p, seed, seed_dev, row0 * Nout, stream);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_gather_nan_rows, dim3((unsigned)blocks_for(R, 256)), dim3(256), 0, st, idx, Form::template Operand<64>::NIDX, R, N, C2, ldc2, (int)Nout);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb
