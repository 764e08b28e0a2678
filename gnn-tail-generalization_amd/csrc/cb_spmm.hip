// CSR sum-aggregation for gfx950 — replaces DGL's gspmm behind
// `graph.update_all(fn.copy_src('h','m'), fn.sum('m','h'))` (GNN_model/GCN.py:198,238)
// with the `* norm` and `+ bias` of GCN.py:242-253 and the following ReLU (GCN.py:127-128)
// fused into the store.
//
// Bound: HBM.  Algorithmic bytes per launch = E*(d*4 + 4) + N*(d*4 + 4) [+ 4N row scale].
//
// Mapping (d = 256 fp32 is the tuned case):
//   * one 64-lane wavefront owns RPW consecutive destination rows; lane l owns columns
//     [VEC*l, VEC*l + VEC) of the 64*VEC-wide column tile, so one neighbour row is ONE
//     fully coalesced 1 KiB global_load_dwordx4 per wavefront (d = 256, VEC = 4);
//   * the rows' edges are contiguous in CSR, so the wavefront walks them as ONE edge
//     stream: 64 column ids per coalesced index load, wave-uniform broadcast
//     (v_readlane -> SGPR base address), U independent gathers in flight before the first
//     add, row boundaries handled while consuming (wave-uniform scalar compares).  Short
//     rows therefore do not serialise on the rowptr -> col -> gather latency chain;
//   * rows longer than the hub threshold (power-law hubs) are skipped here and reduced by
//     k_spmm_hub_chunks (one wavefront per chunk of T edges -> partial row in the
//     workspace) + k_spmm_hub_finish (sums a hub's partials in chunk order + epilogue).
//   * no atomics anywhere: every output element is produced by one lane in a fixed order,
//     so results are bit-reproducible run to run.
//   * streaming data (indices, output rows) uses non-temporal accesses so the 4 MiB L2s and
//     the 256 MiB Infinity Cache keep the re-used neighbour rows (hub sources).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "cb_common.h"
#include "cb_philox.h"
#include "cb_spmm_small.h"

#include "cb_spmm_core.h"

namespace cb {

template <int VEC, bool FUSED, int RPW, int U, typename HT>
static int launch_spmm_cfg(const cb_csr_view& g, const HT* h, int64_t ld_h, int64_t d, Epilogue ep, float* out, int64_t ld_out, hipStream_t st,
                           FusedEpi fe) {
  const int tile = kWave * VEC, wpb = 4;
  const int64_t n_waves = (g.n_rows + RPW - 1) / RPW;
  const dim3 grid((unsigned)((n_waves + wpb - 1) / wpb), (unsigned)((d + tile - 1) / tile));
  // Which k_spmm_rows exist: gather policy 2 (flagged column ids: hot source rows keep the default cache policy, every other gather streams; all-streaming
  // measured slower, profiles/r02_spmm_gather_policy.md) in the d % 256 == 0 kernels, fp32 and bf16-stored rows; the source-row factor in the plain fp32
  // ones of those, without running sums
  constexpr bool kGP = VEC == 4 && RPW == 16 && U == 8;
  constexpr bool kCS = kGP && !FUSED && sizeof(HT) == 4;
  const bool tiled = d % tile == 0, full = FUSED || tiled, acc = ep.acc_init != nullptr, cs = kCS && ep.col_scale;      // (the fused entries take d % 256 == 0 only)
  const int gp = kGP && tiled && ep.col_flags ? 2 : 0;
  CB_CHECK_ARG(!ep.col_flags || gp == 2, CB_E_INVALID, "flagged column ids are only understood by the d %% 256 == 0 kernels");
  CB_CHECK_ARG(!cs || (!acc && tiled), CB_E_INVALID, "a source-row factor needs d %% 256 == 0 and no running sums");
  auto rows = [&](auto FULL, auto ACC, auto GP, auto CS) {
    hipLaunchKernelGGL((k_spmm_rows<VEC, RPW, U, decltype(FULL)::value, FUSED, HT, decltype(ACC)::value, decltype(GP)::value, decltype(CS)::value>), grid,
                       dim3(kWave * wpb), 0, st, g.rowptr, g.col, h, ld_h, out, ld_out, (int)g.n_rows, (int)d, ep, g.hub_threshold, fe);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (full) {
    if (acc) dispatch_gp_cs<kGP, false>(gp, false, [&](auto GP, auto CS) { rows(yes, yes, GP, CS); });
    else dispatch_gp_cs<kGP, kCS>(gp, cs, [&](auto GP, auto CS) { rows(yes, no, GP, CS); });
  } else if constexpr (!FUSED) {      // ragged last column tile: default gathers, no factor
    dispatch_bool(acc, [&](auto ACC) { rows(no, ACC, std::integral_constant<int, 0>{}, no); });
  }
  CB_LAUNCH_CHECK();
  return launch_hub_rows<VEC, HT, FUSED>(g, h, ld_h, d, out, ld_out, ep, fe, st);
}

template <int VEC, bool FUSED = false, typename HT = float>
static int launch_spmm(const cb_csr_view& g, const HT* h, int64_t ld_h, int64_t d, Epilogue ep, float* out, int64_t ld_out, hipStream_t st,
                       FusedEpi fe = FusedEpi{}) {
  // 16 rows per wavefront, 8 gathers in flight: the sweep of row-block / unroll shapes is in profiles/r01_* (all within +-1 %)
  return launch_spmm_cfg<VEC, FUSED, 16, 8, HT>(g, h, ld_h, d, ep, out, ld_out, st, fe);
}

}  // namespace cb

using namespace cb;

extern "C" size_t cb_spmm_workspace_bytes(int64_t n_chunks, int64_t d) {
  if (n_chunks <= 0 || d <= 0) return 0;
  return (size_t)n_chunks * (size_t)partial_ld(d) * sizeof(float);
}

// out = act(row_scale * (acc_init + sum_u col_scale[u] * h[u]) + bias) over fp32 or bf16-stored source rows (include/coldbrew_hip.h).
//   col_scale: a factor per SOURCE row applied as the row is gathered (d % 256 == 0).  The row-sparse backward takes A (a * X_l) on the loss rows with it
//     — the weight gradient of the level contracted over the loss rows (trunk.py; autograd of GCN.py:213,238 re-associated) — without a scaled copy of X_l.
//   acc_init: the later (halo-column) passes of the node-sharded aggregation; it holds the raw sums of the earlier passes (dist.py) and may alias out.
//   h_bf16: build extension BASELINE config 2, and the halo pass when the halo rows crossed the links as bf16 (the wire buffer is read as it arrived).
extern "C" int cb_spmm_csr_f32(const cb_csr_view* g, const void* h, int32_t h_bf16, int64_t ld_h, int64_t d, const float* col_scale,
                               const float* row_scale, const float* bias, int relu, const float* acc_init, int64_t ld_init, float* out,
                               int64_t ld_out, void* stream) {
  const char* who = "cb_spmm_csr_f32";
  cb_csr_view v;
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0 || d == 0) return rc;
  CB_CHECK_ARG(h && out, CB_E_INVALID, "%s: null pointer", who);
  CB_CHECK_ARG(ld_h >= d && ld_out >= d && (!acc_init || ld_init >= d), CB_E_INVALID, "%s: leading dimension smaller than d", who);
  CB_CHECK_ARG(!col_scale || (!h_bf16 && !acc_init && !bias && !relu), CB_E_INVALID,
               "%s: a source-row factor needs fp32 rows, no bias / ReLU / running sums", who);
  Epilogue ep{row_scale, bias, relu, acc_init, ld_init, v.col_flags};
  ep.col_scale = col_scale;
  ep.acc_skip_empty = acc_init && acc_init == out && ld_init == ld_out && !row_scale && !bias && !relu;      // raw in-place pass: rows without edges stay untouched
  hipStream_t st = (hipStream_t)stream;
  const bool ini16 = !acc_init || (aligned16(acc_init) && ld_init % 4 == 0);
  const bool ini8 = !acc_init || (((uintptr_t)acc_init % 8 == 0) && ld_init % 2 == 0);
  if (!h_bf16) {
    const float* hf = (const float*)h;
    const bool al16 = aligned16(h) && aligned16(out) && (ld_h % 4 == 0) && (ld_out % 4 == 0) && (d % 4 == 0) && ini16;
    const bool al8 = ((uintptr_t)h % 8 == 0) && ((uintptr_t)out % 8 == 0) && (ld_h % 2 == 0) && (ld_out % 2 == 0) && (d % 2 == 0) && ini8;
    CB_CHECK_ARG(!v.col_flags || (al16 && d % 256 == 0), CB_E_INVALID, "%s: flagged column ids need d %% 256 == 0 and 16-byte aligned rows", who);
    if (col_scale) {
      CB_CHECK_ARG(al16 && d % 256 == 0, CB_E_INVALID, "%s: a source-row factor needs 16-byte aligned rows with d %% 256 == 0", who);
      return launch_spmm<4>(v, hf, ld_h, d, ep, out, ld_out, st);
    }
    if (!acc_init && spmm_small_eligible(d, al16))
      return launch_spmm_small(v, hf, ld_h, d, row_scale, bias, relu, out, ld_out, partial_ld(d), al16, st);
    if (al16 && d >= 256) return launch_spmm<4>(v, hf, ld_h, d, ep, out, ld_out, st);
    if (al8 && d >= 128) return launch_spmm<2>(v, hf, ld_h, d, ep, out, ld_out, st);
    return launch_spmm<1>(v, hf, ld_h, d, ep, out, ld_out, st);
  }
  const bf16_t* hb = (const bf16_t*)h;
  const bool al8 = ((uintptr_t)h % 8 == 0) && aligned16(out) && (ld_h % 4 == 0) && (ld_out % 4 == 0) && (d % 4 == 0) && ini16;
  const bool al4 = ((uintptr_t)h % 4 == 0) && ((uintptr_t)out % 8 == 0) && (ld_h % 2 == 0) && (ld_out % 2 == 0) && (d % 2 == 0) && ini8;
  CB_CHECK_ARG(!v.col_flags || (al8 && d % 256 == 0), CB_E_INVALID, "%s: flagged column ids need d %% 256 == 0 and 8-byte aligned rows", who);
  if (al8 && d >= 256) return launch_spmm<4, false, bf16_t>(v, hb, ld_h, d, ep, out, ld_out, st);
  if (al4 && d >= 128) return launch_spmm<2, false, bf16_t>(v, hb, ld_h, d, ep, out, ld_out, st);
  return launch_spmm<1, false, bf16_t>(v, hb, ld_h, d, ep, out, ld_out, st);
}

// out[v] = sum_j w_csr[j] * h[col[j]] over fp32 rows with d % 256 == 0: the adjacency with one value per stored edge (w_csr in the order of the view's
// col array), on the kernels of cb_spmm_csr_f32 — the same walk, hub plan and gather policy; acc += w * x edge by edge, a hub row's chunk partials summed
// in chunk order.  No scale / bias / ReLU: the layers that take values (GraphConv, GCNConv(normalize=False)) have none before their GEMM.
extern "C" int cb_spmm_csr_ew_f32(const cb_csr_view* g, const float* w_csr, const float* h, int64_t ld_h, int64_t d, float* out, int64_t ld_out,
                                  void* stream) {
  const char* who = "cb_spmm_csr_ew_f32";
  cb_csr_view v;
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0 || d == 0) return rc;
  CB_CHECK_ARG(h && out && (v.n_edges == 0 || w_csr), CB_E_INVALID, "%s: null pointer", who);
  CB_CHECK_ARG(ld_h >= d && ld_out >= d, CB_E_INVALID, "%s: leading dimension smaller than d", who);
  CB_CHECK_ARG(d % 256 == 0 && aligned16(h) && aligned16(out) && ld_h % 4 == 0 && ld_out % 4 == 0, CB_E_INVALID,
               "%s: 16-byte aligned fp32 rows with d %% 256 == 0 required (other widths: cb_spmm_csr_weighted_f32)", who);
  Epilogue ep{};
  ep.col_flags = v.col_flags;
  ep.edge_w = w_csr;
  hipStream_t st = (hipStream_t)stream;
  constexpr int RPW = 16, wpb = 4;      // (launch_spmm's shape)
  const int64_t n_waves = (v.n_rows + RPW - 1) / RPW;
  const dim3 grid((unsigned)((n_waves + wpb - 1) / wpb), (unsigned)(d / 256));
  dispatch_gp_cs<true, false>(v.col_flags ? 2 : 0, false, [&](auto GP, auto) {
    hipLaunchKernelGGL((k_spmm_rows<4, RPW, 8, true, false, float, false, decltype(GP)::value, false, false, true>), grid, dim3(kWave * wpb), 0, st, v.rowptr,
                       v.col, h, ld_h, out, ld_out, (int)v.n_rows, (int)d, ep, v.hub_threshold, FusedEpi{});
  });
  CB_LAUNCH_CHECK();
  return launch_hub_rows<4, float, false, false, true>(v, h, ld_h, d, out, ld_out, ep, FusedEpi{}, st);
}

// One propagation step with its elementwise passes folded into the store (Label_propagation_model/outcome_correlation.py:128-145):
//     out[v, :] = post_scale[v] * fix_v(clamp(row_scale[v] * sum_{u in row v} h[u, :] + c_mix * mix[v, :], lo, hi))
// Narrow rows (d = number of classes): one lane per column (the VEC = 1 instantiation of k_spmm_rows + hub kernels).
static int spmm_prop_impl(const char* who, const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* mix,
                          int64_t ld_mix, float c_mix, int clamp, float lo, float hi, const uint8_t* fix_rows, const float* post_scale, float* out,
                          int64_t ld_out, void* stream) {
  CB_CHECK_ARG(lo <= hi, CB_E_INVALID, "%s: clamp bounds must satisfy lo <= hi (and neither may be NaN)", who);
  cb_csr_view v;
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0 || d == 0) return rc;
  CB_CHECK_ARG(h && out && mix, CB_E_INVALID, "%s: null pointer", who);
  CB_CHECK_ARG(ld_h >= d && ld_out >= d && ld_mix >= d, CB_E_INVALID, "%s: leading dimension smaller than d", who);
  CB_CHECK_ARG(!v.col_flags, CB_E_INVALID, "%s: flagged column ids are not understood by the narrow-row kernels", who);
  Epilogue ep{row_scale, nullptr, 0, nullptr, 0, 0};
  ep.lp_mix = mix; ep.ld_lp = ld_mix; ep.lp_c_mix = c_mix; ep.lp_post = post_scale;
  ep.lp_clamp = clamp; ep.lp_lo = lo; ep.lp_hi = hi; ep.lp_fix = fix_rows;
  return launch_spmm<1>(v, h, ld_h, d, ep, out, ld_out, (hipStream_t)stream);
}

// One label-propagation step (outcome_correlation.py:137-143, alpha_term = True, post_step = clamp(0, 1); trainer :33-63):
//     out[v, :] = post_scale[v] * clamp(row_scale[v] * sum_{u in row v} h[u, :] + c_mix * mix[v, :], 0, 1)
// With h = D^-1/2 result_t, row_scale = alpha D^-1/2, mix = y0, c_mix = 1 - alpha and post_scale = D^-1/2 the output IS the next step's
// gather operand D^-1/2 result_{t+1}; post_scale = NULL on the last step returns result itself.
extern "C" int cb_spmm_csr_lp_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* mix,
                                  int64_t ld_mix, float c_mix, const float* post_scale, float* out, int64_t ld_out, void* stream) {
  return spmm_prop_impl("cb_spmm_csr_lp_f32", g, h, ld_h, d, row_scale, mix, ld_mix, c_mix, 1, 0.f, 1.f, nullptr, post_scale, out, ld_out, stream);
}

// The propagation step of general_outcome_correlation for every normalisation and post-step the reference uses.
// A_norm = diag(R) A diag(S) (DAD: R = S = D^-1/2; DA: R = D^-1, S = 1; AD: R = 1, S = D^-1) needs no per-edge factor when the state carried from step
// to step is s_t = S (.) result_t: row_scale = alpha R, post_scale = S (NULL on the last step), c_mix = 1 - alpha (alpha_term) or 1.  lo = -inf and
// hi = +inf: no clamp (a NaN then stays a NaN).  fix_rows ([N] bytes or NULL): a row with a non-zero byte becomes mix[v, :] (fix_inputs, :194-199).
// The kernel, the hub plan and every expression are those of cb_spmm_csr_lp_f32: lo = 0, hi = 1, fix_rows = NULL gives its results bit for bit.
extern "C" int cb_spmm_csr_prop_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* mix,
                                    int64_t ld_mix, float c_mix, float lo, float hi, const uint8_t* fix_rows, const float* post_scale, float* out,
                                    int64_t ld_out, void* stream) {
  const int clamp = !(lo == -INFINITY && hi == INFINITY);
  return spmm_prop_impl("cb_spmm_csr_prop_f32", g, h, ld_h, d, row_scale, mix, ld_mix, c_mix, clamp, lo, hi, fix_rows, post_scale, out, ld_out, stream);
}

// The fused trunk store (include/coldbrew_hip.h).  acc_init: on top of the interior-column partial sums (the last pass of the node-sharded aggregation,
// bf16 rows when the halo rows crossed the links as bf16).  row_ids: over a CSR whose rows are a SUBSET of the node rows (rows-only forward, trunk.py) —
// row r of the CSR / of row_scale / of out_act / out_next is node row row_ids[r] (ascending); mix_src, relu_bits and the dropout mask are taken at the node row.
extern "C" int cb_spmm_csr_fused_f32(const cb_csr_view* g, const int32_t* row_ids, const void* h, int32_t h_bf16, int64_t ld_h, int64_t d,
                                     const float* row_scale, const float* bias, const float* acc_init, int64_t ld_init, const cb_trunk_store* store,
                                     float* out_next, int64_t ld_next, void* stream) {
  const char* who = "cb_spmm_csr_fused_f32";
  CB_CHECK_ARG(d > 0 && d % 256 == 0, CB_E_INVALID, "%s: d must be a positive multiple of 256", who);
  cb_csr_view v;
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG(h && out_next, CB_E_INVALID, "%s: null pointer", who);
  const int rcs = check_trunk_store(who, store, d);
  if (rcs != CB_OK) return rcs;
  CB_CHECK_ARG(!store->mix_index, CB_E_INVALID, "%s: the mix is taken at the node row (no mix_index)", who);
  CB_CHECK_ARG(!row_ids || (!acc_init && !h_bf16), CB_E_INVALID, "%s: a row subset needs fp32 rows and no running sums", who);
  const bool al = ((uintptr_t)h % (h_bf16 ? 8 : 16) == 0) && aligned16(out_next) && ld_h % 4 == 0 && ld_next % 4 == 0;
  CB_CHECK_ARG(al && ld_h >= d && ld_next >= d, CB_E_INVALID, "%s: 16-byte aligned rows required", who);
  CB_CHECK_ARG(!acc_init || (aligned16(acc_init) && ld_init % 4 == 0 && ld_init >= d), CB_E_INVALID,
               "%s: acc_init must be 16-byte aligned rows of at least d floats", who);
  Epilogue ep{row_scale, bias, 1, acc_init, ld_init, v.col_flags};
  FusedEpi fe{};
  fe.st = make_trunk_store(*store);
  fe.out_next = out_next; fe.ld_next = ld_next; fe.d = (int)d; fe.row_ids = row_ids;
  if (h_bf16) return launch_spmm<4, true, bf16_t>(v, (const bf16_t*)h, ld_h, d, ep, out_next, ld_next, (hipStream_t)stream, fe);
  return launch_spmm<4, true, float>(v, (const float*)h, ld_h, d, ep, out_next, ld_next, (hipStream_t)stream, fe);
}

// A (reverse) aggregation whose epilogue is the BACKWARD of the trunk's store of the rows it writes (the row-sparse backward's dense level, trunk.py):
//   g = row_scale * sum  -> out_g (the gradient w.r.t. the stored, dropped activation: kept for the input stage's mix gather)
//   out_gr = bwd_rowscale * c_act * dropout_bwd_seed(g) where relu_bits (READ: written by the forward's store) has the element's bit, else 0
// = cb_spmm_csr_f32 followed by cb_trunk_layer_bwd_f32 without the pass's read of g (bit-identical values); the bias gradient of that pass (column sums of
// the masked gradient) is taken by cb_trunk_input_bwd_multi_cs_f32, which reads g anyway.  d % 256 == 0, fp32 rows.
extern "C" int cb_spmm_csr_store_bwd_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const uint64_t* relu_bits,
                                         const float* bwd_rowscale, float c_act, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0,
                                         float* out_g, int64_t ld_g, float* out_gr, int64_t ld_gr, void* stream) {
  const char* who = "cb_spmm_csr_store_bwd_f32";
  CB_CHECK_ARG(d > 0 && d % 256 == 0, CB_E_INVALID, "%s: d must be a positive multiple of 256", who);
  cb_csr_view v;
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG(h && out_gr && relu_bits, CB_E_INVALID, "%s: null pointer", who);
  CB_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && row0 >= 0, CB_E_INVALID, "%s: dropout p / row offset out of range", who);
  CB_CHECK_ARG(aligned16(h) && aligned16(out_gr) && ld_h % 4 == 0 && ld_gr % 4 == 0 && ld_h >= d && ld_gr >= d &&
                   (!out_g || (aligned16(out_g) && ld_g % 4 == 0 && ld_g >= d)) && ((uintptr_t)relu_bits % 8 == 0),
               CB_E_INVALID, "%s: 16-byte aligned rows required", who);
  Epilogue ep{row_scale, nullptr, 0, nullptr, 0, v.col_flags};
  FusedEpi fe{};
  fe.bwd = 1; fe.bwd_rowscale = bwd_rowscale; fe.st.c_act = c_act;
  set_store_dropout(fe.st, drop_p);
  fe.st.seed = seed; fe.st.seed_dev = seed_dev; fe.st.row0 = row0; fe.st.bits = (unsigned long long*)relu_bits;
  fe.st.out_act = out_g; fe.st.ld_act = ld_g; fe.out_next = out_gr; fe.ld_next = ld_gr; fe.d = (int)d;
  return launch_spmm<4, true, float>(v, h, ld_h, d, ep, out_gr, ld_gr, (hipStream_t)stream, fe);
}

namespace cb {
// partial[p][c], p < nparts, summed in groups of `per` consecutive rows: thread = column (coalesced), fixed order -> folded[g][c]
__global__ void __launch_bounds__(256) k_colsum_fold(const float* __restrict__ partial, int nparts, int d, int per, float* __restrict__ folded) {
  const int g = blockIdx.x;
  const int p0 = g * per, p1 = min(nparts, p0 + per);
  for (int c = threadIdx.x; c < d; c += blockDim.x) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int p = p0;
    for (; p + 4 <= p1; p += 4) {
      s0 += partial[(int64_t)p * d + c]; s1 += partial[(int64_t)(p + 1) * d + c];
      s2 += partial[(int64_t)(p + 2) * d + c]; s3 += partial[(int64_t)(p + 3) * d + c];
    }
    for (; p < p1; ++p) s0 += partial[(int64_t)p * d + c];
    folded[(int64_t)g * d + c] = (s0 + s1) + (s2 + s3);
  }
}
// out[c] = sum_g folded[g][c]: 32 columns x 8 strided group lanes per block, fixed order
__global__ void __launch_bounds__(256) k_colsum_last(const float* __restrict__ folded, int ngroups, int d, float* __restrict__ out) {
  __shared__ float s_t[8][32];
  const int cl = threadIdx.x & 31, gl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < d) {
#pragma unroll 4
    for (int g = gl; g < ngroups; g += 8) s += folded[(int64_t)g * d + c];
  }
  s_t[gl][cl] = s;
  __syncthreads();
  if (gl == 0 && c < d)
    out[c] = ((s_t[0][cl] + s_t[1][cl]) + (s_t[2][cl] + s_t[3][cl])) + ((s_t[4][cl] + s_t[5][cl]) + (s_t[6][cl] + s_t[7][cl]));
}
constexpr int kFoldGroups = 1024;
static inline int64_t mix_row_blocks(int64_t N) { return ((N + 15) / 16 + 3) / 4; }
static inline int64_t mix_hub_blocks(int64_t n_hubs) { return (n_hubs + 3) / 4; }
}  // namespace cb

extern "C" size_t cb_spmm_store_bwd_mix_workspace_bytes(int64_t N, int64_t n_hubs, int64_t d) {
  if (N <= 0 || d <= 0) return 0;
  return (size_t)(mix_row_blocks(N) + mix_hub_blocks(n_hubs > 0 ? n_hubs : 0) + kFoldGroups) * (size_t)d * sizeof(float);
}

// cb_spmm_csr_store_bwd_f32 on ALL node rows whose first output is not the raw gradient g but the FOLDED mix gradient
//   out_m = c_mix * ( dropout_bwd_seed(g) + sum_q dropout_bwd_{mix_seeds[q]}(mix_g[q][mix_pos[q][row]]) )        (n_mix <= 2 compact operands; pos < 0: absent)
// — everything the layers above and this store send to X0 through their residual mixes (res_tricks.py:23, under each store's own dropout GCN.py:110,133),
// so that the input stage (cb_gemm_tn_instage_f32) reads ONE [N, d] matrix beside dL/d dropout(X0) — and colsum (may be null) = the column sums of
// out_gr / bwd_rowscale: the bias gradient of the store whose backward this is (autograd of GCN.py:253).  ws2: cb_spmm_store_bwd_mix_workspace_bytes.
extern "C" int cb_spmm_csr_store_bwd_mix_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale,
                                             const uint64_t* relu_bits, const float* bwd_rowscale, float c_act, float drop_p, uint64_t seed,
                                             const uint64_t* seed_dev, int64_t row0, float* out_m, int64_t ld_m, float* out_gr, int64_t ld_gr, int32_t n_mix,
                                             const float* const* mix_g, const int32_t* const* mix_pos, const uint64_t* mix_seeds, float c_mix, float* colsum,
                                             void* ws2, size_t ws2_bytes, void* stream) {
  const char* who = "cb_spmm_csr_store_bwd_mix_f32";
  CB_CHECK_ARG(d > 0 && d % 256 == 0, CB_E_INVALID, "%s: d must be a positive multiple of 256", who);
  cb_csr_view v;
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  const int64_t N = v.n_rows;
  CB_CHECK_ARG(h && out_gr && out_m && relu_bits, CB_E_INVALID, "%s: null pointer", who);
  CB_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && row0 >= 0, CB_E_INVALID, "%s: dropout p / row offset out of range", who);
  CB_CHECK_ARG(aligned16(h) && aligned16(out_gr) && aligned16(out_m) && ld_h % 4 == 0 && ld_gr % 4 == 0 && ld_m % 4 == 0 &&
                   ld_h >= d && ld_gr >= d && ld_m >= d && ((uintptr_t)relu_bits % 8 == 0),
               CB_E_INVALID, "%s: 16-byte aligned rows required", who);
  CB_CHECK_ARG(n_mix >= 0 && n_mix <= 2 && (n_mix == 0 || (mix_g && mix_pos && mix_seeds)), CB_E_INVALID, "%s: 0..2 compact mix operands", who);
  CB_CHECK_ARG(!colsum || (ws2 && ws2_bytes >= cb_spmm_store_bwd_mix_workspace_bytes(N, v.n_hubs, d)), CB_E_WORKSPACE,
               "%s: column-sum workspace missing/too small", who);
  Epilogue ep{row_scale, nullptr, 0, nullptr, 0, v.col_flags};
  FusedEpi fe{};
  fe.bwd = 1; fe.bwd_rowscale = bwd_rowscale; fe.st.c_act = c_act;
  set_store_dropout(fe.st, drop_p);
  fe.st.seed = seed; fe.st.seed_dev = seed_dev; fe.st.row0 = row0; fe.st.bits = (unsigned long long*)relu_bits;
  fe.st.out_act = out_m; fe.st.ld_act = ld_m; fe.out_next = out_gr; fe.ld_next = ld_gr; fe.d = (int)d;
  fe.mx_n = n_mix; fe.mx_c = c_mix;
  for (int q = 0; q < n_mix; ++q) {
    CB_CHECK_ARG(mix_g[q] && mix_pos[q] && aligned16(mix_g[q]), CB_E_INVALID, "%s: null or misaligned mix operand %d", who, q);
    fe.mx_g[q] = mix_g[q]; fe.mx_pos[q] = mix_pos[q]; fe.mx_seed[q] = mix_seeds[q];
  }
  fe.cs_partial = colsum ? (float*)ws2 : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb_rows = mix_row_blocks(N), nb_hub = v.n_hubs > 0 ? mix_hub_blocks(v.n_hubs) : 0;
  fe.cs_block0 = 0;
  dispatch_gp_cs<true, false>(v.col_flags ? 2 : 0, false, [&](auto GP, auto) {
    hipLaunchKernelGGL((k_spmm_rows<4, 16, 8, true, true, float, false, decltype(GP)::value, false, true>), dim3((unsigned)nb_rows, (unsigned)(d / 256)), dim3(256), 0,
                       st, v.rowptr, v.col, h, ld_h, out_gr, ld_gr, (int)N, (int)d, ep, v.hub_threshold, fe);
  });
  CB_LAUNCH_CHECK();
  fe.cs_block0 = (int)nb_rows;      // (the hub-finish blocks' partial column sums follow the row kernel's)
  const int rch = launch_hub_rows<4, float, true, true>(v, h, ld_h, d, out_gr, ld_gr, ep, fe, st);
  if (rch != CB_OK) return rch;
  if (colsum) {
    const int nparts = (int)(nb_rows + nb_hub);
    const int per = (nparts + kFoldGroups - 1) / kFoldGroups;
    const int ngroups = (nparts + per - 1) / per;
    float* folded = (float*)ws2 + (size_t)nparts * d;
    hipLaunchKernelGGL(k_colsum_fold, dim3((unsigned)ngroups), dim3(256), 0, st, (const float*)ws2, nparts, (int)d, per, folded);
    CB_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_colsum_last, dim3((unsigned)((d + 31) / 32)), dim3(256), 0, st, (const float*)folded, ngroups, (int)d, colsum);
    CB_LAUNCH_CHECK();
  }
  return CB_OK;
}
