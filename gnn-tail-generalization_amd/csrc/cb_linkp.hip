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
//   loss       score_e = <emb[h_e], emb[t_e]> (fp32, one wavefront per edge, fixed-shape reduction); one block finishes
//              loss = mean max(s, 0) - s y + log1p(exp(-|s|)) and mrr = mean 1 / (1 + #{negatives of i's group above pos_i}) in float64, rounded once.
//   backward   ds_e = g (sigmoid(s_e) - y_e) / (P + Nn); dEmb[h_e] += ds_e emb[t_e], dEmb[t_e] += ds_e emb[h_e] without atomics: the 2 (P + Nn)
//              contributions are sorted by destination (cb::sort_u64, stable: ascending contribution number inside a node), the wavefront at the
//              head of a node's run adds the run in that order (float64, rounded once) and writes the row; all other rows are zero-filled before.
// No float atomics, no host synchronisation inside an entry, two calls with the same inputs give the same bits.
#include "cb_common.h"
#include "cb_philox.h"
#include "cb_sort.h"

namespace cb {

__device__ __forceinline__ bool lp_node_ok(const uint8_t* __restrict__ mask, int v, int mode) { return (mask[v] != 0) == (mode == 0); }

// the two integers of draw `ctr` in [0, n): multiply-high of 64 random bits (a 32-bit multiply-high is biased by up to n / 2^32)
__device__ __forceinline__ void lp_draw2(uint64_t seed, uint64_t ctr, uint64_t n, uint64_t& a, uint64_t& b) {
  uint32_t r[4];
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  a = __umul64hi(((uint64_t)r[0] << 32) | r[1], n);
  b = __umul64hi(((uint64_t)r[2] << 32) | r[3], n);
}

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
__device__ __forceinline__ bool lp_row_has(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int row, int x) {
  int lo = rowptr[row], hi = rowptr[row + 1];
  while (lo < hi) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    const int c = col[mid];
    if (c == x) return true;
    if (c < x) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

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

// ---- scores ---------------------------------------------------------------------------------------------------------------------------
// edge e < P: (pos[e], pos[P + e]); e >= P: (neg[e - P], neg[Nn + e - P]).  false for an endpoint outside [0, N) (never used as an index).
__device__ __forceinline__ bool lp_edge(const int32_t* __restrict__ pos, int64_t P, const int32_t* __restrict__ neg, int64_t Nn, int64_t N, int64_t e,
                                        int& h, int& t) {
  if (e < P) {
    h = pos[e];
    t = pos[P + e];
  } else {
    h = neg[e - P];
    t = neg[Nn + e - P];
  }
  return h >= 0 && h < N && t >= 0 && t < N;
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_linkp_scores(const float* __restrict__ emb, int64_t ld, int64_t N, int D, const int32_t* __restrict__ pos,
                                                      int64_t P, const int32_t* __restrict__ neg, int64_t Nn, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (e >= P + Nn) return;
  int h, t;
  if (!lp_edge(pos, P, neg, Nn, N, e, h, t)) {      // (wave-uniform)
    if (lane == 0) scores[e] = __int_as_float(0x7FC00000);
    return;
  }
  const float* a = emb + (int64_t)h * ld;
  const float* b = emb + (int64_t)t * ld;
  float s = 0.f;
  if (VEC) {
    for (int c = 4 * lane; c < D; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(a + c), y = *reinterpret_cast<const float4*>(b + c);
      s = fmaf(x.x, y.x, s);
      s = fmaf(x.y, y.y, s);
      s = fmaf(x.z, y.z, s);
      s = fmaf(x.w, y.w, s);
    }
  } else {
    for (int c = lane; c < D; c += 64) s = fmaf(a[c], b[c], s);
  }
  s = wave_sum(s);
  if (lane == 0) scores[e] = s;
}

// One block.  loss (may be NULL) = mean over P + Nn of the stable BCE-with-logits term, labels 1 for the P positives; mrr with k = Nn / P negatives
// per positive (the last Nn - k P are dropped), ties counting for the positive; status (may be NULL) = number of edges with an endpoint outside
// [0, N).  Thread-strided float64 partial sums, then a halving tree over the 256 threads: one fixed order.
__global__ void __launch_bounds__(256) k_linkp_finish(const float* __restrict__ ps, int64_t P, const float* __restrict__ ns, int64_t Nn,
                                                      const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int64_t N,
                                                      float* __restrict__ loss, float* __restrict__ mrr, int32_t* __restrict__ status) {
  __shared__ double s_loss[256], s_rr[256];
  __shared__ int s_bad[256];
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
      int h, tt;
      bad += lp_edge(pos, P, neg, Nn, N, e, h, tt) ? 0 : 1;
    }
  for (int64_t i = t; i < P; i += 256) {
    const float p = ps[i];
    int64_t rank = 1;
    for (int64_t j = i * k; j < (i + 1) * k; ++j) rank += ns[j] > p ? 1 : 0;
    sr += 1.0 / (double)rank;
  }
  s_loss[t] = sl;
  s_rr[t] = sr;
  s_bad[t] = bad;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
      s_loss[t] += s_loss[t + off];
      s_rr[t] += s_rr[t + off];
      s_bad[t] += s_bad[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (loss) loss[0] = (float)(s_loss[0] / (double)S);
    mrr[0] = (float)(s_rr[0] / (double)P);
    if (status) status[0] = s_bad[0];
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
// contribution c = 2 e + side goes to node (side ? t_e : h_e); key = c << 32 | node, node = N for an edge that is not usable (sorted last, skipped)
__global__ void __launch_bounds__(256) k_linkp_keys(const int32_t* __restrict__ pos, int64_t P, const int32_t* __restrict__ neg, int64_t Nn, int64_t N,
                                                    uint64_t* __restrict__ keys) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * (P + Nn)) return;
  int h, t;
  const bool ok = lp_edge(pos, P, neg, Nn, N, c >> 1, h, t);
  const uint64_t node = ok ? (uint64_t)((c & 1) ? t : h) : (uint64_t)N;
  keys[c] = ((uint64_t)c << 32) | node;
}

// One wavefront per sorted position; the one at the head of a node's run owns the node's row of dEmb.  Columns in chunks of 256 (four per lane);
// wider rows walk the run once per chunk.
__global__ void __launch_bounds__(256) k_linkp_bwd_rows(const float* __restrict__ emb, int64_t ld, int64_t N, int D, const int32_t* __restrict__ pos,
                                                        int64_t P, const int32_t* __restrict__ neg, int64_t Nn, const float* __restrict__ scores,
                                                        const float* __restrict__ g, const uint64_t* __restrict__ keys, float* __restrict__ demb,
                                                        int64_t ldd) {
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_keys = 2 * (P + Nn);
  if (i >= n_keys) return;
  const uint32_t node = (uint32_t)keys[i];
  if (node >= (uint32_t)N) return;
  if (i > 0 && (uint32_t)keys[i - 1] == node) return;      // not the head of its run
  const double scale = (double)g[0] / (double)(P + Nn);
  for (int c0 = 0; c0 < D; c0 += 256) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j = i; j < n_keys; ++j) {
      const uint64_t key = keys[j];      // (wave-uniform)
      if ((uint32_t)key != node) break;
      const int64_t c = (int64_t)(key >> 32), e = c >> 1;
      int h, t;
      lp_edge(pos, P, neg, Nn, N, e, h, t);      // (usable: its node is < N)
      const float* other = emb + (int64_t)((c & 1) ? h : t) * ld;
      const double s = (double)scores[e];
      const double ds = scale * (1.0 / (1.0 + exp(-s)) - (e < P ? 1.0 : 0.0));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cc = c0 + lane + 64 * q;
        if (cc < D) acc[q] = fma(ds, (double)other[cc], acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cc = c0 + lane + 64 * q;
      if (cc < D) demb[(int64_t)node * ldd + cc] = (float)acc[q];
    }
  }
}

static inline int lp_bits(int64_t n) {
  int b = 0;
  while (((int64_t)1 << b) < n) ++b;
  return b;
}

static inline size_t lp_keys_bytes(int64_t S) { return align_up((size_t)(2 * S) * sizeof(uint64_t), 256); }

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

#define LP_CHECK_SIZES(name)                                                                                                           \
  CB_CHECK_ARG(N > 0 && D > 0 && ld >= D && P >= 1 && Nn >= 0, CB_E_INVALID, name ": bad size (N > 0, D > 0, ld >= D, P >= 1, Nn >= 0 required)"); \
  CB_CHECK_ARG(N < INT32_MAX && D < (1 << 24) && P + Nn < INT32_MAX / 2, CB_E_RANGE, name ": size out of range")

extern "C" int cb_linkp_mrr_f32(const float* pos_score, int64_t P, const float* neg_score, int64_t Nn, float* mrr, void* stream) {
  CB_CHECK_ARG(P >= 1 && Nn >= 0, CB_E_INVALID, "cb_linkp_mrr_f32: P >= 1 and Nn >= 0 required");
  CB_CHECK_ARG(P + Nn < INT32_MAX / 2, CB_E_RANGE, "cb_linkp_mrr_f32: size out of range");
  CB_CHECK_ARG(pos_score && (neg_score || Nn == 0) && mrr, CB_E_INVALID, "cb_linkp_mrr_f32: null pointer");
  hipLaunchKernelGGL(k_linkp_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, pos_score, P, neg_score, Nn, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, (int64_t)0, (float*)nullptr, mrr, (int32_t*)nullptr);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_linkp_loss_fwd_f32(const float* emb, int64_t ld, int64_t N, int64_t D, const int32_t* pos, int64_t P, const int32_t* neg, int64_t Nn,
                                     float* scores, float* loss, float* mrr, int32_t* status, void* stream) {
  LP_CHECK_SIZES("cb_linkp_loss_fwd_f32");
  CB_CHECK_ARG(emb && pos && (neg || Nn == 0) && scores && loss && mrr && status, CB_E_INVALID, "cb_linkp_loss_fwd_f32: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)blocks_for(P + Nn, 4);
  if (D % 4 == 0 && ld % 4 == 0 && aligned16(emb))
    hipLaunchKernelGGL(k_linkp_scores<true>, dim3(nb), dim3(256), 0, st, emb, ld, N, (int)D, pos, P, neg, Nn, scores);
  else
    hipLaunchKernelGGL(k_linkp_scores<false>, dim3(nb), dim3(256), 0, st, emb, ld, N, (int)D, pos, P, neg, Nn, scores);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_linkp_finish, dim3(1), dim3(256), 0, st, (const float*)scores, P, (const float*)(scores + P), Nn, pos, neg, N, loss, mrr, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_linkp_bwd_workspace_bytes(int64_t P, int64_t Nn) {
  if (P < 0 || Nn < 0 || P + Nn <= 0) return 0;
  const int64_t S = P + Nn;
  return 2 * lp_keys_bytes(S) + align_up(sort_u64_temp_bytes(2 * S), 256);
}

extern "C" int cb_linkp_loss_bwd_f32(const float* emb, int64_t ld, int64_t N, int64_t D, const int32_t* pos, int64_t P, const int32_t* neg, int64_t Nn,
                                     const float* scores, const float* g, float* demb, int64_t ldd, void* ws, size_t ws_bytes, void* stream) {
  LP_CHECK_SIZES("cb_linkp_loss_bwd_f32");
  CB_CHECK_ARG(ldd >= D, CB_E_INVALID, "cb_linkp_loss_bwd_f32: ldd >= D required");
  CB_CHECK_ARG(emb && pos && (neg || Nn == 0) && scores && g && demb, CB_E_INVALID, "cb_linkp_loss_bwd_f32: null pointer");
  CB_CHECK_ARG(ws && ws_bytes >= cb_linkp_bwd_workspace_bytes(P, Nn), CB_E_WORKSPACE, "cb_linkp_loss_bwd_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = P + Nn;
  char* base = (char*)ws;
  uint64_t* keys_in = (uint64_t*)base;
  uint64_t* keys_out = (uint64_t*)(base + lp_keys_bytes(S));
  void* temp = base + 2 * lp_keys_bytes(S);
  if (ldd == D) {
    CB_HIP(hipMemsetAsync(demb, 0, (size_t)N * (size_t)D * sizeof(float), st));
  } else {
    CB_HIP(hipMemset2DAsync(demb, (size_t)ldd * sizeof(float), 0, (size_t)D * sizeof(float), (size_t)N, st));
  }
  hipLaunchKernelGGL(k_linkp_keys, dim3((unsigned)blocks_for(2 * S, 256)), dim3(256), 0, st, pos, P, neg, Nn, N, keys_in);
  CB_LAUNCH_CHECK();
  const int rc = sort_u64(temp, ws_bytes - 2 * lp_keys_bytes(S), keys_in, keys_out, 2 * S, lp_bits(N + 1), st);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_linkp_bwd_rows, dim3((unsigned)blocks_for(2 * S, 4)), dim3(256), 0, st, emb, ld, N, (int)D, pos, P, neg, Nn, scores, g,
                     (const uint64_t*)keys_out, demb, ldd);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
