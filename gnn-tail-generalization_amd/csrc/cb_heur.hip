// The link-prediction baselines CN / AA (Link_prediction_baseline/heuristics.py:107-129; Link_prediction_model/layer.py:6-17 `Heuristics.get_score`;
// base_options.py:112 `--encoder CN | AA | PPR`) and the counts behind Hits@K / AUC (Link_prediction_model/utils.py:43-59;
// Link_prediction_baseline/heuristics.py:51-62) on the device CSR.
//
//   semantics  A = csr_matrix((1, (ei[0], ei[1]))) sums duplicates: A[s, k] is the multiplicity of the edge s -> k, row s of A the OUT-row of s — the
//              by-src CSR, whose rows keep ascending columns with duplicates stored.  CN(s, d) = sum_k A[s, k] A[d, k]; AA(s, d) = sum_k A[s, k]
//              A[d, k] w[k], w[k] = 1 / log(c_k), c_k = the column sum of A = the in-degree of k with multiplicity, w[k] = 0 where c_k <= 1 (the
//              reference zeroes the inf of c_k = 1; a c_k = 0 column is never hit).  No special case for s == d, self loops or (s, d) being an edge.
//   pairs      a group of G lanes (16: four pairs per wavefront, or 64) owns a pair and walks the SHORTER of the two rows one entry per lane in
//              strides of G; a 16-lane group hands a pair whose shorter row has more than 64 entries to its whole wavefront.  An entry with
//              column k finds the run of k in the longer row (lower bound, then the upper bound only where the run is longer than one) and
//              contributes its length (times w[k]): a column stored m_s times in the short row and m_d times in the long one contributes
//              m_s * m_d, with no run-head detection.  The searches are dependent loads: occupancy hides them, so the kernel holds few
//              registers and no LDS.  CN accumulates in int64, the weighted form in float64; a fixed butterfly over the group (the wavefront
//              for a handed-over pair) reduces; one lane converts to fp32 once and stores.  A pair with an endpoint outside [0, N) is never
//              used as an index: its score is NaN and it adds one to `status` (an integer atomic on one word, executed on that error path
//              only and order-independent: the float results involve no atomic, two calls give the same bits).
//   ranks      gt[i] = #{j : neg[j] > pos[i]}, eq[i] = #{j : neg[j] == pos[i]} over all negatives: an order-preserving float -> uint32 key (-0.0
//              and +0.0 share one key, -inf lowest, +inf highest), cb::sort_u64 on 32 bits, two binary searches per positive.  A NaN on either
//              side counts in status (the same error-path atomic) and every gt / eq is then -1.
#include <math.h>

#include "cb_common.h"
#include "cb_sort.h"

namespace cb {

// ---- AA weights -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_heur_aa_weights(const int32_t* __restrict__ rowptr, int64_t N, double* __restrict__ w) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  const int c = rowptr[k + 1] - rowptr[k];
  w[k] = c <= 1 ? 0.0 : 1.0 / log((double)c);
}

// ---- pair scores ----------------------------------------------------------------------------------------------------------------------
// first position in [lo, lo + n) whose column is not below k.  The trip count depends on n alone: the lanes of a group (one long row) stay together.
__device__ __forceinline__ int heur_lower(const int32_t* __restrict__ col, int lo, int n, int k) {
  while (n > 0) {
    const int half = n >> 1;
    const bool below = col[lo + half] < k;
    lo = below ? lo + half + 1 : lo;
    n = below ? n - half - 1 : half;
  }
  return lo;
}

__device__ __forceinline__ int heur_upper(const int32_t* __restrict__ col, int lo, int n, int k) {
  while (n > 0) {
    const int half = n >> 1;
    const bool not_above = col[lo + half] <= k;
    lo = not_above ? lo + half + 1 : lo;
    n = not_above ? n - half - 1 : half;
  }
  return lo;
}

template <typename T, int G>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The entries [ab, ae) of the short row, `start` + a multiple of `stride`, against the long row [bb, be): adds to cn / aa.
template <bool WEIGHTED>
__device__ __forceinline__ void heur_walk(const int32_t* __restrict__ col, const double* __restrict__ w, int64_t N, int ab, int ae, int bb, int be, int start,
                                          int stride, long long& cn, double& aa) {
  for (int64_t e = (int64_t)ab + start; e < ae; e += stride) {
    const int k = col[e];
    const int lo = heur_lower(col, bb, be - bb, k);
    if (lo < be && col[lo] == k) {
      int hi = lo + 1;
      if (hi < be && col[hi] == k) hi = heur_upper(col, hi, be - hi, k);      // a multi-edge in the long row
      if (WEIGHTED) {
        if (k >= 0 && k < N) aa += (double)(hi - lo) * w[k];
      } else {
        cn += hi - lo;
      }
    }
  }
}

// G = 16: a pair whose shorter row has more than kHeurHeavy entries is not walked by its group: the wavefront takes such pairs one after the other
// with all 64 lanes, so one hub pair does not leave the other 48 lanes of its wavefront idle.  G = 64: one pair per wavefront throughout.
constexpr int kHeurHeavy = 64;

template <int G, bool WEIGHTED>
__global__ void __launch_bounds__(256) k_heur_pairs(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int64_t E,
                                                    const double* __restrict__ w, const int32_t* __restrict__ pairs, int64_t P,
                                                    float* __restrict__ score, int32_t* __restrict__ status) {
  const int sub = threadIdx.x & (G - 1);
  const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  const bool live = p < P;      // (group-uniform; a dead group still takes part in the shuffles of its wavefront)
  int s = -1, d = -1;
  if (live) {
    s = pairs[p];
    d = pairs[P + p];
  }
  const bool ok = live && s >= 0 && s < N && d >= 0 && d < N;
  int ab = 0, ae = 0, bb = 0, be = 0;      // a: the shorter row, b: the longer one; both clamped into [0, E]
  if (ok) {
    const int e_max = (int)E;
    int sb = min(max(rowptr[s], 0), e_max), se = min(max(rowptr[s + 1], sb), e_max);
    int db = min(max(rowptr[d], 0), e_max), de = min(max(rowptr[d + 1], db), e_max);
    const bool s_short = se - sb <= de - db;
    ab = s_short ? sb : db;
    ae = s_short ? se : de;
    bb = s_short ? db : sb;
    be = s_short ? de : se;
  }
  long long cn = 0;
  double aa = 0.0;
  const bool heavy = G < 64 && ae - ab > kHeurHeavy;      // (group-uniform)
  if (!heavy) heur_walk<WEIGHTED>(col, w, N, ab, ae, bb, be, sub, G, cn, aa);
  if (WEIGHTED) aa = group_sum<double, G>(aa);
  else cn = group_sum<long long, G>(cn);
  if (G < 64) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(heavy && sub == 0);      // the leaders of the heavy groups of this wavefront (wave-uniform)
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      long long hcn = 0;
      double haa = 0.0;
      heur_walk<WEIGHTED>(col, w, N, __shfl(ab, leader), __shfl(ae, leader), __shfl(bb, leader), __shfl(be, leader), lane, 64, hcn, haa);
      if (WEIGHTED) {
        haa = group_sum<double, 64>(haa);
        if (lane == leader) aa = haa;
      } else {
        hcn = group_sum<long long, 64>(hcn);
        if (lane == leader) cn = hcn;
      }
    }
  }
  if (live && sub == 0) {
    score[p] = ok ? (WEIGHTED ? (float)aa : (float)cn) : __int_as_float(0x7FC00000);
    if (!ok) atomicAdd(status, 1);
  }
}

// ---- rank counts ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rk_is_nan(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

// ascending keys for ascending floats; -0.0 and +0.0 give the same key
__device__ __forceinline__ uint32_t rk_key(uint32_t u) {
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// keys[j] of the negatives, and the NaNs of both sides counted into status
__global__ void __launch_bounds__(256) k_rank_keys(const float* __restrict__ pos, int64_t P, const float* __restrict__ neg, int64_t Nn,
                                                   uint64_t* __restrict__ keys, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < Nn) {
    const uint32_t u = __float_as_uint(neg[i]);
    keys[i] = (uint64_t)rk_key(u);
    if (rk_is_nan(u)) atomicAdd(status, 1);
  } else if (i < Nn + P) {
    if (rk_is_nan(__float_as_uint(pos[i - Nn]))) atomicAdd(status, 1);
  }
}

__global__ void __launch_bounds__(256) k_rank_search(const float* __restrict__ pos, int64_t P, const uint64_t* __restrict__ keys, int64_t Nn,
                                                     const int32_t* __restrict__ status, int32_t* __restrict__ gt, int32_t* __restrict__ eq) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  if (status[0] != 0) {
    gt[i] = -1;
    eq[i] = -1;
    return;
  }
  const uint64_t k = (uint64_t)rk_key(__float_as_uint(pos[i]));
  int64_t lo = 0, n = Nn;      // first key >= k
  while (n > 0) {
    const int64_t half = n >> 1;
    const bool below = keys[lo + half] < k;
    lo = below ? lo + half + 1 : lo;
    n = below ? n - half - 1 : half;
  }
  int64_t hi = lo;             // first key > k
  n = Nn - lo;
  while (n > 0) {
    const int64_t half = n >> 1;
    const bool not_above = keys[hi + half] <= k;
    hi = not_above ? hi + half + 1 : hi;
    n = not_above ? n - half - 1 : half;
  }
  gt[i] = (int32_t)(Nn - hi);
  eq[i] = (int32_t)(hi - lo);
}

static inline size_t rk_keys_bytes(int64_t Nn) { return align_up((size_t)Nn * sizeof(uint64_t), 256); }

template <int G>
static int heur_launch(const cb_csr_view* g, const double* w, const int32_t* pairs, int64_t P, float* score, int32_t* status, hipStream_t st) {
  const unsigned nb = (unsigned)((P * G + 255) / 256);
  if (w)
    hipLaunchKernelGGL((k_heur_pairs<G, true>), dim3(nb), dim3(256), 0, st, g->rowptr, g->col, g->n_rows, g->n_edges, w, pairs, P, score, status);
  else
    hipLaunchKernelGGL((k_heur_pairs<G, false>), dim3(nb), dim3(256), 0, st, g->rowptr, g->col, g->n_rows, g->n_edges, w, pairs, P, score, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb

using namespace cb;

#define HEUR_CHECK_GRAPH(g, name)                                                                                                          \
  CB_CHECK_ARG((g) && (g)->rowptr, CB_E_INVALID, name ": null graph");                                                                     \
  CB_CHECK_ARG((g)->n_rows > 0 && (g)->n_edges >= 0, CB_E_INVALID, name ": bad graph size");                                               \
  CB_CHECK_ARG((g)->n_rows < INT32_MAX && (g)->n_edges < INT32_MAX, CB_E_RANGE, name ": graph out of the int32 index range")

extern "C" int cb_heur_aa_weights_f64(const cb_csr_view* g_in, double* w, void* stream) {
  HEUR_CHECK_GRAPH(g_in, "cb_heur_aa_weights_f64");
  CB_CHECK_ARG(w, CB_E_INVALID, "cb_heur_aa_weights_f64: null pointer");
  hipLaunchKernelGGL(k_heur_aa_weights, dim3((unsigned)blocks_for(g_in->n_rows, 256)), dim3(256), 0, (hipStream_t)stream, g_in->rowptr, g_in->n_rows, w);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_heur_pair_scores_width_f32(const cb_csr_view* g_out, const double* w, const int32_t* pairs, int64_t P, int32_t group, float* score,
                                             int32_t* status, void* stream) {
  HEUR_CHECK_GRAPH(g_out, "cb_heur_pair_scores_f32");
  CB_CHECK_ARG(g_out->col && g_out->col_flags == 0, CB_E_INVALID, "cb_heur_pair_scores_f32: null column array, or one with cache-policy flags");
  CB_CHECK_ARG(group == 16 || group == 64, CB_E_INVALID, "cb_heur_pair_scores_f32: the group width is 16 or 64 lanes");
  CB_CHECK_ARG(P >= 0, CB_E_INVALID, "cb_heur_pair_scores_f32: P >= 0 required");
  CB_CHECK_ARG(P < INT32_MAX / 2, CB_E_RANGE, "cb_heur_pair_scores_f32: P out of range");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_heur_pair_scores_f32: null pointer (status)");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (P == 0) return CB_OK;
  CB_CHECK_ARG(pairs && score, CB_E_INVALID, "cb_heur_pair_scores_f32: null pointer");
  return group == 16 ? heur_launch<16>(g_out, w, pairs, P, score, status, st) : heur_launch<64>(g_out, w, pairs, P, score, status, st);
}

extern "C" int cb_heur_pair_scores_f32(const cb_csr_view* g_out, const double* w, const int32_t* pairs, int64_t P, float* score, int32_t* status,
                                       void* stream) {
  return cb_heur_pair_scores_width_f32(g_out, w, pairs, P, CB_HEUR_GROUP, score, status, stream);
}

extern "C" size_t cb_rank_counts_workspace_bytes(int64_t P, int64_t Nn) {
  if (P < 0 || Nn <= 0) return 0;
  return 2 * rk_keys_bytes(Nn) + align_up(sort_u64_temp_bytes(Nn), 256);
}

extern "C" int cb_rank_counts_f32(const float* pos, int64_t P, const float* neg, int64_t Nn, int32_t* gt, int32_t* eq, int32_t* status, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  CB_CHECK_ARG(P >= 0 && Nn >= 0, CB_E_INVALID, "cb_rank_counts_f32: P >= 0 and Nn >= 0 required");
  CB_CHECK_ARG(P < INT32_MAX && Nn < INT32_MAX, CB_E_RANGE, "cb_rank_counts_f32: P and Nn must stay below 2^31 (the counts are int32)");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_rank_counts_f32: null pointer (status)");
  CB_CHECK_ARG((pos && gt && eq) || P == 0, CB_E_INVALID, "cb_rank_counts_f32: null pointer");
  CB_CHECK_ARG(neg || Nn == 0, CB_E_INVALID, "cb_rank_counts_f32: null pointer (neg)");
  CB_CHECK_ARG(Nn == 0 || (workspace && workspace_bytes >= cb_rank_counts_workspace_bytes(P, Nn)), CB_E_WORKSPACE, "cb_rank_counts_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (P + Nn == 0) return CB_OK;
  char* base = (char*)workspace;
  uint64_t* keys_in = (uint64_t*)base;
  uint64_t* keys_out = Nn ? (uint64_t*)(base + rk_keys_bytes(Nn)) : nullptr;
  hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)blocks_for(P + Nn, 256)), dim3(256), 0, st, pos, P, neg, Nn, keys_in, status);
  CB_LAUNCH_CHECK();
  if (Nn) {
    const int rc = sort_u64(base + 2 * rk_keys_bytes(Nn), workspace_bytes - 2 * rk_keys_bytes(Nn), keys_in, keys_out, Nn, 32, st);
    if (rc != CB_OK) return rc;
  }
  if (P == 0) return CB_OK;
  hipLaunchKernelGGL(k_rank_search, dim3((unsigned)blocks_for(P, 256)), dim3(256), 0, st, pos, P, (const uint64_t*)keys_out, Nn, (const int32_t*)status, gt, eq);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
