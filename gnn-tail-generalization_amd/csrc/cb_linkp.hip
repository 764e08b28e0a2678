// The edge-wise (link-prediction) term of the teacher's training step (trainer_node_classification.py:417-438, 507-563 `gen_pn_edges` /
// `my_negative_sampling`; utils.py:754-791 `calc_score` / `linkp_loss_eva` / `cal_MRR`) on the device CSR.
//
//   samplers   The by-dst CSR keeps ascending columns inside a row, so "is (u, v) an edge" is a binary search in row v: a negative draw costs
//              O(log deg) and a positive draw O(log N + deg / 64), independent of E.  The reference (PyG `negative_sampling`) linearises, sorts and
//              isin-tests the whole edge list per call.  Every draw is Philox4x32-10 keyed by the 64-bit seed with the 64-bit counter
//              slot * CB_LINKP_MAX_TRIES + try; an integer in [0, n) is the high 64 bits of (r0 << 32 | r1) * n (r2, r3: the draw's second integer).
//   positives  uniform with replacement over the edges whose two endpoints are both inside (train) / both outside (test) the train mask, multiplicity
//              and self loops as the edge list has them.  prefix [N + 1] (built off the step from k_linkp_valid_counts and a scan) gives the row of the
//              k-th valid edge; one wavefront then walks that row 64 columns at a time (ballot + popcount) to the (k - prefix[row])-th valid column.
//   negatives  slot s writes (u, v) to column 2 s and (v, u) to column 2 s + 1.  train: u, v from the ascending list of train nodes; test: from all
//              nodes, rejected if both are train nodes.  Rejected too: u == v, u in row v, v in row u.  A slot without a pair after
//              CB_LINKP_MAX_TRIES tries writes -1 to its four cells and adds one to an int32 counter (integer atomic: order-independent).
//   loss       score_e = <emb[h_e], emb[t_e]> over pos | neg: k_pair_dot (cb_pair_core.h); one block finishes
//              loss = mean max(s, 0) - s y + log1p(exp(-|s|)) and mrr = mean 1 / (1 + #{negatives of i's group above pos_i}) in float64, rounded once.
//   backward   ds_e = g (sigmoid(s_e) - y_e) / (P + Nn); dEmb[h_e] += ds_e emb[t_e], dEmb[t_e] += ds_e emb[h_e] without atomics: the sorted
//              inverted-index scatter of cb_pair_core.h (pair_scatter) with the BCE coefficient, formed in float64 where it is used.
// No float atomics, no host synchronisation inside an entry, two calls with the same inputs give the same bits.
#include "cb_common.h"
#include "cb_pair_core.h"
#include "cb_draw.h"      // lp_draw2, lp_row_has: shared with cb_lpx.hip

namespace cb {

__device__ __forceinline__ bool lp_node_ok(const uint8_t* __restrict__ mask, int v, int mode) { return (mask[v] != 0) == (mode == 0); }

// ---- positives ------------------------------------------------------------------------------------------------------------------------
// counts[v] = number of entries of row v whose column is valid, 0 for a row that is not valid itself.  One wavefront per row.
__global__ void __launch_bounds__(256) k_linkp_valid_counts(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                            const uint8_t* __restrict__ mask, int mode, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t v = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (v >= N) return;
  int c = 0;
  if (lp_node_ok(mask, (int)v, mode)) {
    const int beg = rowptr[v], end = rowptr[v + 1];
    for (int e = beg + lane; e < end; e += 64) {
      const int u = col[e];
      c += (u >= 0 && u < N && lp_node_ok(mask, u, mode)) ? 1 : 0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (lane == 0) counts[v] = c;
}

// One wavefront per draw.  prefix[N] == V > 0.  A prefix array that does not belong to (graph, mask, mode) cannot make the walk leave its row:
// the slot then writes (-1, -1).
__global__ void __launch_bounds__(256) k_linkp_positives(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                         const uint8_t* __restrict__ mask, int mode, const int32_t* __restrict__ prefix, int64_t V,
                                                         int64_t P, uint64_t seed, const uint64_t* __restrict__ seed_dev, int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t slot = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (slot >= P) return;
  if (seed_dev) seed += *seed_dev;
  uint64_t k64, unused;
  lp_draw2(seed, (uint64_t)slot * CB_LINKP_MAX_TRIES, (uint64_t)V, k64, unused);
  const int k = (int)k64;
  int lo = 0, hi = (int)N - 1;      // the row r with prefix[r] <= k < prefix[r + 1]  (wave-uniform)
  while (lo < hi) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    if (prefix[mid + 1] <= k) lo = mid + 1;
    else hi = mid;
  }
  const int row = lo;
  int rank = k - prefix[row];
  int src = -1;
  const int beg = rowptr[row], end = rowptr[row + 1];
  for (int e0 = beg; e0 < end && rank >= 0; e0 += 64) {
    const int e = e0 + lane;
    const int u = e < end ? col[e] : -1;
    const bool ok = u >= 0 && u < N && lp_node_ok(mask, u, mode);
    const unsigned long long m = __ballot(ok);
    const int cnt = __popcll(m);
    if (rank < cnt) {
      const int before = __popcll(m & ((1ull << lane) - 1ull));
      const unsigned long long hit = __ballot(ok && before == rank);
      src = __shfl(u, __ffsll((long long)hit) - 1);
      break;
    }
    rank -= cnt;
  }
  if (lane == 0) {
    out[slot] = src;
    out[P + slot] = src >= 0 ? row : -1;
  }
}

// ---- negatives ------------------------------------------------------------------------------------------------------------------------
// One thread per slot: the tries of a slot are a chain of dependent searches, and the slots are independent.
__global__ void __launch_bounds__(256) k_linkp_negatives(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                         const uint8_t* __restrict__ mask, int mode, const int32_t* __restrict__ train_nodes,
                                                         int64_t n_train, int64_t n_slots, uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                                         int32_t* __restrict__ out, int32_t* __restrict__ n_failed) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= n_slots) return;
  if (seed_dev) seed += *seed_dev;
  const int64_t Nn = 2 * n_slots;
  const uint64_t n = mode == 0 ? (uint64_t)n_train : (uint64_t)N;
  int u = -1, v = -1;
  for (int t = 0; t < CB_LINKP_MAX_TRIES; ++t) {
    uint64_t a, b;
    lp_draw2(seed, (uint64_t)slot * CB_LINKP_MAX_TRIES + t, n, a, b);
    int cu = (int)a, cv = (int)b;
    if (mode == 0) {
      cu = train_nodes[cu];
      cv = train_nodes[cv];
      if (cu < 0 || cu >= N || cv < 0 || cv >= N) continue;      // (a list that does not belong to this graph)
    } else if (mask[cu] != 0 && mask[cv] != 0) {
      continue;      // test: at least one endpoint outside the train split
    }
    if (cu == cv) continue;
    if (lp_row_has(rowptr, col, cv, cu) || lp_row_has(rowptr, col, cu, cv)) continue;
    u = cu;
    v = cv;
    break;
  }
  out[2 * slot] = u;
  out[2 * slot + 1] = v;
  out[Nn + 2 * slot] = v;
  out[Nn + 2 * slot + 1] = u;
  if (u < 0) atomicAdd(n_failed, 1);
}

// ---- loss ------------------------------------------------------------------------------------------------------------------------------
// One block.  loss (may be NULL) = mean over P + Nn of the stable BCE-with-logits term, labels 1 for the P positives; mrr with k = Nn / P negatives
// per positive (the last Nn - k P are dropped), ties counting for the positive; status (may be NULL) = number of pairs of src with an endpoint
// outside [0, N) (a count below 2^31 is exact in float64).  Thread-strided float64 partial sums, then block_tree_f64: one fixed order.
__global__ void __launch_bounds__(256) k_linkp_finish(const float* __restrict__ ps, int64_t P, const float* __restrict__ ns, int64_t Nn, PairSource<true> src,
                                                      int64_t N, float* __restrict__ loss, float* __restrict__ mrr, int32_t* __restrict__ status) {
  __shared__ double sm[3][256];     // loss, reciprocal ranks, unusable pairs
  const int t = threadIdx.x;
  const int64_t S = P + Nn, k = Nn / P;
  double sl = 0.0, sr = 0.0;
  int bad = 0;
  if (loss)
    for (int64_t e = t; e < S; e += 256) {
      const double s = (double)(e < P ? ps[e] : ns[e - P]);
      sl += fmax(s, 0.0) - (e < P ? s : 0.0) + log1p(exp(-fabs(s)));
    }
  if (status)
    for (int64_t e = t; e < S; e += 256) {
      int u, v;
      bad += src.get(e, N, u, v) ? 0 : 1;
    }
  for (int64_t i = t; i < P; i += 256) {
    const float p = ps[i];
    int64_t rank = 1;
    for (int64_t j = i * k; j < (i + 1) * k; ++j) rank += ns[j] > p ? 1 : 0;
    sr += 1.0 / (double)rank;
  }
  sm[0][t] = sl;
  sm[1][t] = sr;
  sm[2][t] = (double)bad;
  block_tree_f64(sm, t);
  if (t == 0) {
    if (loss) loss[0] = (float)(sm[0][0] / (double)S);
    mrr[0] = (float)(sm[1][0] / (double)P);
    if (status) status[0] = (int32_t)sm[2][0];
  }
}

}  // namespace cb

using namespace cb;

#define LP_CHECK_GRAPH(name)                                                                                                     \
  CB_CHECK_ARG(g && g->rowptr && g->col && g->col_flags == 0, CB_E_INVALID, name ": null graph, or a column array with cache-policy flags"); \
  CB_CHECK_ARG(g->n_rows > 0 && g->n_edges >= 0, CB_E_INVALID, name ": bad graph size");                                         \
  CB_CHECK_ARG(g->n_rows < INT32_MAX && g->n_edges < INT32_MAX, CB_E_RANGE, name ": graph out of the int32 index range");          \
  CB_CHECK_ARG(mode == 0 || mode == 1, CB_E_INVALID, name ": mode must be 0 (train) or 1 (test)")

extern "C" int cb_linkp_max_tries(void) { return CB_LINKP_MAX_TRIES; }

extern "C" int cb_linkp_valid_counts_i32(const cb_csr_view* g, const uint8_t* mask, int32_t mode, int32_t* counts, void* stream) {
  LP_CHECK_GRAPH("cb_linkp_valid_counts_i32");
  CB_CHECK_ARG(mask && counts, CB_E_INVALID, "cb_linkp_valid_counts_i32: null pointer");
  hipLaunchKernelGGL(k_linkp_valid_counts, dim3((unsigned)blocks_for(g->n_rows, 4)), dim3(256), 0, (hipStream_t)stream, g->rowptr, g->col, g->n_rows, mask,
                     (int)mode, counts);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_linkp_positives_i32(const cb_csr_view* g, const uint8_t* mask, int32_t mode, const int32_t* prefix, int64_t n_valid, int64_t P,
                                      uint64_t seed, const uint64_t* seed_dev, int32_t* out, void* stream) {
  LP_CHECK_GRAPH("cb_linkp_positives_i32");
  CB_CHECK_ARG(P >= 0 && n_valid > 0 && n_valid <= g->n_edges, CB_E_INVALID, "cb_linkp_positives_i32: P >= 0 and 0 < n_valid <= n_edges required");
  CB_CHECK_ARG(P < INT32_MAX / 2, CB_E_RANGE, "cb_linkp_positives_i32: P out of range");
  if (P == 0) return CB_OK;
  CB_CHECK_ARG(mask && prefix && out, CB_E_INVALID, "cb_linkp_positives_i32: null pointer");
  hipLaunchKernelGGL(k_linkp_positives, dim3((unsigned)blocks_for(P, 4)), dim3(256), 0, (hipStream_t)stream, g->rowptr, g->col, g->n_rows, mask, (int)mode,
                     prefix, n_valid, P, seed, seed_dev, out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_linkp_negatives_i32(const cb_csr_view* g, const uint8_t* mask, int32_t mode, const int32_t* train_nodes, int64_t n_train, int64_t Nn,
                                      uint64_t seed, const uint64_t* seed_dev, int32_t* out, int32_t* n_failed, void* stream) {
  LP_CHECK_GRAPH("cb_linkp_negatives_i32");
  CB_CHECK_ARG(Nn >= 0 && Nn % 2 == 0, CB_E_INVALID, "cb_linkp_negatives_i32: Nn must be even and >= 0 (slot s fills columns 2 s and 2 s + 1)");
  CB_CHECK_ARG(Nn < INT32_MAX / 2, CB_E_RANGE, "cb_linkp_negatives_i32: Nn out of range");
  CB_CHECK_ARG(mode == 1 || (n_train > 0 && n_train <= g->n_rows), CB_E_INVALID, "cb_linkp_negatives_i32: train mode needs 0 < n_train <= N");
  if (Nn == 0) return CB_OK;
  CB_CHECK_ARG(mask && out && n_failed && (mode == 1 || train_nodes), CB_E_INVALID, "cb_linkp_negatives_i32: null pointer");
  hipLaunchKernelGGL(k_linkp_negatives, dim3((unsigned)blocks_for(Nn / 2, 256)), dim3(256), 0, (hipStream_t)stream, g->rowptr, g->col, g->n_rows, mask,
                     (int)mode, train_nodes, n_train, Nn / 2, seed, seed_dev, out, n_failed);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_linkp_mrr_f32(const float* pos_score, int64_t P, const float* neg_score, int64_t Nn, float* mrr, void* stream) {
  CB_CHECK_ARG(P >= 1 && Nn >= 0, CB_E_INVALID, "cb_linkp_mrr_f32: P >= 1 and Nn >= 0 required");
  CB_CHECK_ARG(P + Nn < INT32_MAX / 2, CB_E_RANGE, "cb_linkp_mrr_f32: size out of range");
  CB_CHECK_ARG(pos_score && (neg_score || Nn == 0) && mrr, CB_E_INVALID, "cb_linkp_mrr_f32: null pointer");
  hipLaunchKernelGGL(k_linkp_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, pos_score, P, neg_score, Nn, PairSource<true>{nullptr, 0, nullptr, 0},
                     (int64_t)0, (float*)nullptr, mrr, (int32_t*)nullptr);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// the scores over pos | neg are k_pair_dot's; the unusable pairs are counted by the finisher, which reads every pair anyway (no atomic)
extern "C" int cb_linkp_loss_fwd_f32(const float* emb, int64_t ld, int64_t N, int64_t D, const int32_t* pos, int64_t P, const int32_t* neg, int64_t Nn,
                                     float* scores, float* loss, float* mrr, int32_t* status, void* stream) {
  CB_PAIR_CHECK_SIZES("cb_linkp_loss_fwd_f32", P + Nn, P >= 1 && Nn >= 0, "P >= 1, Nn >= 0");
  CB_CHECK_ARG(emb && pos && (neg || Nn == 0) && scores && loss && mrr && status, CB_E_INVALID, "cb_linkp_loss_fwd_f32: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const PairSource<true> src{pos, P, neg, Nn};
  const int rc = launch_pair_dot(emb, ld, N, D, src, scores, nullptr, st);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_linkp_finish, dim3(1), dim3(256), 0, st, (const float*)scores, P, (const float*)(scores + P), Nn, src, N, loss, mrr, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_linkp_bwd_workspace_bytes(int64_t P, int64_t Nn) {
  if (P < 0 || Nn < 0 || P + Nn <= 0) return 0;
  return pair_scatter_ws_bytes(P + Nn);
}

extern "C" int cb_linkp_loss_bwd_f32(const float* emb, int64_t ld, int64_t N, int64_t D, const int32_t* pos, int64_t P, const int32_t* neg, int64_t Nn,
                                     const float* scores, const float* g, float* demb, int64_t ldd, void* ws, size_t ws_bytes, void* stream) {
  CB_PAIR_CHECK_SIZES("cb_linkp_loss_bwd_f32", P + Nn, P >= 1 && Nn >= 0, "P >= 1, Nn >= 0");
  CB_CHECK_ARG(ldd >= D, CB_E_INVALID, "cb_linkp_loss_bwd_f32: ldd >= D required");
  CB_CHECK_ARG(emb && pos && (neg || Nn == 0) && scores && g && demb, CB_E_INVALID, "cb_linkp_loss_bwd_f32: null pointer");
  CB_CHECK_ARG(ws && ws_bytes >= cb_linkp_bwd_workspace_bytes(P, Nn), CB_E_WORKSPACE, "cb_linkp_loss_bwd_f32: workspace too small");
  return pair_scatter(emb, ld, N, D, PairSource<true>{pos, P, neg, Nn}, CoefBce{scores, g, P, P + Nn}, demb, ldd, ws, ws_bytes, (hipStream_t)stream);
}
