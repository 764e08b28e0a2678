// The link-prediction experiment's samplers, epoch shuffle and ranking metrics (Link_prediction_model/negative_sample.py:5-57; model.py:121-266;
// utils.py:568-586 `cal_recall`; the OGB evaluator's MRR) on the device.
//
//   neg_global   `global_neg_sample` (:5-19).  The reference (PyG `negative_sampling` after `add_self_loops`) linearises, sorts and isin-tests the whole edge
//                list for every call; here "is (u, v) an edge" is a binary search for u in row v of the by-dst CSR (ascending columns, duplicates kept):
//                O(log deg) per try, independent of E.  One thread per slot: a slot's tries are a chain of dependent searches, the slots are independent.
//                Only the directed pair is tested.  A slot without an accepted try in CB_LPX_MAX_TRIES holds -1 and counts in an int32 word (integer atomic).
//   neg_local    `local_neg_sample`, random_src=False (:28-40): the positive's source and a uniform node, no rejection.
//   permutation  perm = the low words of the sorted keys (r0(draw i) << 32) | i: distinct keys, so a pure function of (n, seed).  cb::sort_u64 on 64 bits.
//   row_ranks    per row i of neg [P, K]: the entries above pos[i] and equal to it (cb_rank_counts_f32's contract per row).  A group of 16 or 64 lanes
//                per row; a scalar head up to the row's first 16-byte boundary, float4 loads from there, a scalar tail.  Bound: HBM, 4 P K bytes read once.
//   recall_topk  the numerator of `cal_recall`: the positives above 0 and all negatives, ordered by descending score with a positive before a negative
//                among equals: keys (descending-order bits << 1) | is_negative, one sort_u64 on 34 bits (a positive at or below 0 takes the key 2^33 and
//                sorts behind every member), one counting pass over the first min(k, P + Nn) keys.
// Draws are those of cb_linkp.hip (cb_draw.h).  No float atomics; no host synchronisation inside an entry; two calls with the same inputs give the same bits.
#include "cb_common.h"
#include "cb_draw.h"
#include "cb_sort.h"

namespace cb {

// ---- samplers -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lpx_neg_global(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int64_t S,
                                                        uint64_t seed, int32_t* __restrict__ out, int32_t* __restrict__ n_failed) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= S) return;
  int u = -1, v = -1;
  for (int t = 0; t < CB_LPX_MAX_TRIES; ++t) {
    uint64_t a, b;
    lp_draw2(seed, (uint64_t)slot * CB_LPX_MAX_TRIES + t, (uint64_t)N, a, b);
    const int cu = (int)a, cv = (int)b;      // both below N by construction: rowptr[cv], rowptr[cv + 1] are inside the array
    if (cu == cv) continue;
    if (lp_row_has(rowptr, col, cv, cu)) continue;
    u = cu;
    v = cv;
    break;
  }
  out[slot] = u;
  out[S + slot] = v;
  if (u < 0) atomicAdd(n_failed, 1);
}

__global__ void __launch_bounds__(256) k_lpx_neg_local(const int32_t* __restrict__ pos_src, int64_t k, int64_t N, int64_t S, uint64_t seed,
                                                       int32_t* __restrict__ out) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= S) return;
  uint64_t a, unused;
  lp_draw2(seed, (uint64_t)slot * CB_LPX_MAX_TRIES, (uint64_t)N, a, unused);
  out[slot] = pos_src[slot / k];
  out[S + slot] = (int32_t)a;
}

// ---- permutation ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lpx_perm_keys(int64_t n, uint64_t seed, uint64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t r[4];
  lp_words(seed, (uint64_t)i, r);
  keys[i] = ((uint64_t)r[0] << 32) | (uint64_t)i;
}

__global__ void __launch_bounds__(256) k_lpx_perm_low(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ perm) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) perm[j] = (int32_t)(uint32_t)keys[j];
}

static inline size_t lpx_keys_bytes(int64_t n) { return align_up((size_t)n * sizeof(uint64_t), 256); }

// ---- row ranks ------------------------------------------------------------------------------------------------------------------------
// G lanes per row (G divides 64; the lanes of a group leave together, so the butterflies below stay inside a group of live lanes).
template <int G>
__global__ void __launch_bounds__(256) k_lpx_row_ranks(const float* __restrict__ pos, int64_t P, const float* __restrict__ neg, int64_t ld, int64_t K,
                                                       int32_t* __restrict__ gt, int32_t* __restrict__ eq, int32_t* __restrict__ status) {
  const int lane = threadIdx.x % G;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (i >= P) return;
  const float p = pos[i];
  const float* __restrict__ row = neg + i * ld;
  int g = 0, e = 0, nan = (lane == 0 && p != p) ? 1 : 0;
  auto take = [&](float x) {
    g += x > p ? 1 : 0;      // IEEE compares: -0.0 == +0.0, the infinities are numbers, a NaN is neither above nor equal
    e += x == p ? 1 : 0;
    nan += x != x ? 1 : 0;
  };
  int64_t head = (int64_t)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);      // scalar elements up to the first 16-byte boundary of the row (0..3)
  if (head > K) head = K;
  if (lane < head) take(row[lane]);
  const int64_t nv = (K - head) >> 2;
  const float4* __restrict__ v4 = (const float4*)(row + head);
  for (int64_t j = lane; j < nv; j += G) {
    const float4 q = v4[j];
    take(q.x);
    take(q.y);
    take(q.z);
    take(q.w);
  }
  const int64_t t0 = head + 4 * nv;      // at most 3 elements are left
  if (t0 + lane < K) take(row[t0 + lane]);
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    g += __shfl_xor(g, off);
    e += __shfl_xor(e, off);
    nan += __shfl_xor(nan, off);
  }
  if (lane == 0) {
    gt[i] = nan ? -1 : g;
    eq[i] = nan ? -1 : e;
    if (nan) atomicAdd(status, nan);
  }
}

// ---- recall -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lpx_is_nan(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

// ascending keys for DESCENDING floats; -0.0 and +0.0 give the same key
__device__ __forceinline__ uint32_t lpx_desc_key(uint32_t u) {
  if ((u << 1) == 0u) u = 0u;
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

constexpr uint64_t kLpxOutside = 1ull << 33;      // a positive at or below 0: behind every member of M (their keys stay below 2^33)

__global__ void __launch_bounds__(256) k_lpx_recall_keys(const float* __restrict__ pos, int64_t P, const float* __restrict__ neg, int64_t Nn,
                                                         uint64_t* __restrict__ keys, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P + Nn) return;
  const bool is_neg = i >= P;
  const float x = is_neg ? neg[i - P] : pos[i];
  const uint32_t u = __float_as_uint(x);
  if (lpx_is_nan(u)) atomicAdd(status, 1);
  keys[i] = (is_neg || x > 0.f) ? (((uint64_t)lpx_desc_key(u) << 1) | (is_neg ? 1ull : 0ull)) : kLpxOutside;
}

// result += the positives among the first `top` sorted keys (top <= P + Nn; the keys outside M are not positives of M).  Integer adds only.
__global__ void __launch_bounds__(256) k_lpx_recall_count(const uint64_t* __restrict__ keys, int64_t top, const int32_t* __restrict__ status,
                                                          long long* __restrict__ result) {
  if (status[0] != 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) result[0] = -1;
    return;
  }
  int c = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < top; j += (int64_t)gridDim.x * 256) {
    const uint64_t k = keys[j];
    c += (k < kLpxOutside && (k & 1ull) == 0ull) ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)result, (unsigned long long)c);
}

}  // namespace cb

using namespace cb;

#define LPX_CHECK_GRAPH(name)                                                                                                                \
  CB_CHECK_ARG(g && g->rowptr && g->col && g->col_flags == 0, CB_E_INVALID, name ": null graph, or a column array with cache-policy flags"); \
  CB_CHECK_ARG(g->n_rows >= 2 && g->n_edges >= 0, CB_E_INVALID, name ": N >= 2 required (a negative pair has two distinct nodes)");          \
  CB_CHECK_ARG(g->n_rows < INT32_MAX && g->n_edges < INT32_MAX, CB_E_RANGE, name ": graph out of the int32 index range")

extern "C" int cb_lpx_max_tries(void) { return CB_LPX_MAX_TRIES; }

extern "C" int cb_lpx_neg_global_i32(const cb_csr_view* g, int64_t S, uint64_t seed, int32_t* out, int32_t* n_failed, void* stream) {
  LPX_CHECK_GRAPH("cb_lpx_neg_global_i32");
  CB_CHECK_ARG(S >= 0, CB_E_INVALID, "cb_lpx_neg_global_i32: S >= 0 required");
  CB_CHECK_ARG(S < INT32_MAX / 2, CB_E_RANGE, "cb_lpx_neg_global_i32: S out of range");
  if (S == 0) return CB_OK;
  CB_CHECK_ARG(out && n_failed, CB_E_INVALID, "cb_lpx_neg_global_i32: null pointer");
  hipLaunchKernelGGL(k_lpx_neg_global, dim3((unsigned)blocks_for(S, 256)), dim3(256), 0, (hipStream_t)stream, g->rowptr, g->col, g->n_rows, S, seed, out,
                     n_failed);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_lpx_neg_local_i32(const int32_t* pos_src, int64_t P, int64_t k, int64_t N, uint64_t seed, int32_t* out, void* stream) {
  CB_CHECK_ARG(P >= 0 && k >= 0, CB_E_INVALID, "cb_lpx_neg_local_i32: P >= 0 and k >= 0 required");
  CB_CHECK_ARG(N >= 2, CB_E_INVALID, "cb_lpx_neg_local_i32: N >= 2 required");
  CB_CHECK_ARG(N < INT32_MAX && P < INT32_MAX / 2 && k < INT32_MAX / 2 && P * k < INT32_MAX / 2, CB_E_RANGE, "cb_lpx_neg_local_i32: size out of range");
  if (P * k == 0) return CB_OK;
  CB_CHECK_ARG(pos_src && out, CB_E_INVALID, "cb_lpx_neg_local_i32: null pointer");
  hipLaunchKernelGGL(k_lpx_neg_local, dim3((unsigned)blocks_for(P * k, 256)), dim3(256), 0, (hipStream_t)stream, pos_src, k, N, P * k, seed, out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_lpx_permutation_workspace_bytes(int64_t n) {
  if (n <= 0 || n >= INT32_MAX) return 0;
  return 2 * lpx_keys_bytes(n) + align_up(sort_u64_temp_bytes(n), 256);
}

extern "C" int cb_lpx_permutation_i32(int64_t n, uint64_t seed, int32_t* perm, void* workspace, size_t workspace_bytes, void* stream) {
  CB_CHECK_ARG(n >= 0, CB_E_INVALID, "cb_lpx_permutation_i32: n >= 0 required");
  CB_CHECK_ARG(n < INT32_MAX, CB_E_RANGE, "cb_lpx_permutation_i32: n must stay below 2^31 (the permutation is int32)");
  if (n == 0) return CB_OK;
  CB_CHECK_ARG(perm, CB_E_INVALID, "cb_lpx_permutation_i32: null pointer");
  CB_CHECK_ARG(workspace && workspace_bytes >= cb_lpx_permutation_workspace_bytes(n), CB_E_WORKSPACE, "cb_lpx_permutation_i32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  uint64_t* keys_in = (uint64_t*)base;
  uint64_t* keys_out = (uint64_t*)(base + lpx_keys_bytes(n));
  const unsigned nb = (unsigned)blocks_for(n, 256);
  hipLaunchKernelGGL(k_lpx_perm_keys, dim3(nb), dim3(256), 0, st, n, seed, keys_in);
  CB_LAUNCH_CHECK();
  const int rc = sort_u64(base + 2 * lpx_keys_bytes(n), workspace_bytes - 2 * lpx_keys_bytes(n), keys_in, keys_out, n, 64, st);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL(k_lpx_perm_low, dim3(nb), dim3(256), 0, st, (const uint64_t*)keys_out, n, perm);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_lpx_row_ranks_f32(const float* pos, int64_t P, const float* neg, int64_t ld, int64_t K, int32_t* gt, int32_t* eq, int32_t* status,
                                    void* stream) {
  CB_CHECK_ARG(P >= 0 && K >= 0, CB_E_INVALID, "cb_lpx_row_ranks_f32: P >= 0 and K >= 0 required");
  CB_CHECK_ARG(ld >= K, CB_E_INVALID, "cb_lpx_row_ranks_f32: row stride >= K required");
  CB_CHECK_ARG(P < INT32_MAX / 2 && K < INT32_MAX, CB_E_RANGE, "cb_lpx_row_ranks_f32: P and K must stay below 2^30 and 2^31 (the counts are int32)");
  CB_CHECK_ARG(status, CB_E_INVALID, "cb_lpx_row_ranks_f32: null pointer (status)");
  CB_CHECK_ARG(P == 0 || (pos && gt && eq && (neg || K == 0)), CB_E_INVALID, "cb_lpx_row_ranks_f32: null pointer");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  if (P == 0) return CB_OK;
  if (K <= 64)
    hipLaunchKernelGGL(k_lpx_row_ranks<16>, dim3((unsigned)blocks_for(P, 16)), dim3(256), 0, st, pos, P, neg, ld, K, gt, eq, status);
  else
    hipLaunchKernelGGL(k_lpx_row_ranks<64>, dim3((unsigned)blocks_for(P, 4)), dim3(256), 0, st, pos, P, neg, ld, K, gt, eq, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_lpx_recall_topk_workspace_bytes(int64_t P, int64_t Nn) {
  if (P < 0 || Nn < 0 || P + Nn <= 0 || P + Nn >= ((int64_t)1 << 32)) return 0;
  return 2 * lpx_keys_bytes(P + Nn) + align_up(sort_u64_temp_bytes(P + Nn), 256);
}

extern "C" int cb_lpx_recall_topk_f32(const float* pos, int64_t P, const float* neg, int64_t Nn, int64_t k, int64_t* result, int32_t* status,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  CB_CHECK_ARG(P >= 0 && Nn >= 0 && k >= 0, CB_E_INVALID, "cb_lpx_recall_topk_f32: P >= 0, Nn >= 0 and k >= 0 required");
  CB_CHECK_ARG(P < ((int64_t)1 << 32) && Nn < ((int64_t)1 << 32) && P + Nn < ((int64_t)1 << 32), CB_E_RANGE,
               "cb_lpx_recall_topk_f32: P + Nn must stay below 2^32 (one sort)");
  CB_CHECK_ARG(result && status, CB_E_INVALID, "cb_lpx_recall_topk_f32: null pointer (result / status)");
  CB_CHECK_ARG((pos || P == 0) && (neg || Nn == 0), CB_E_INVALID, "cb_lpx_recall_topk_f32: null pointer");
  const int64_t n = P + Nn;
  CB_CHECK_ARG(n == 0 || (workspace && workspace_bytes >= cb_lpx_recall_topk_workspace_bytes(P, Nn)), CB_E_WORKSPACE,
               "cb_lpx_recall_topk_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
  CB_HIP(hipMemsetAsync(result, 0, sizeof(int64_t), st));
  if (n == 0) return CB_OK;
  char* base = (char*)workspace;
  uint64_t* keys_in = (uint64_t*)base;
  uint64_t* keys_out = (uint64_t*)(base + lpx_keys_bytes(n));
  hipLaunchKernelGGL(k_lpx_recall_keys, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, st, pos, P, neg, Nn, keys_in, status);
  CB_LAUNCH_CHECK();
  const int rc = sort_u64(base + 2 * lpx_keys_bytes(n), workspace_bytes - 2 * lpx_keys_bytes(n), keys_in, keys_out, n, 34, st);
  if (rc != CB_OK) return rc;
  const int64_t top = k < n ? k : n;
  int64_t nb = blocks_for(top > 0 ? top : 1, 256);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_lpx_recall_count, dim3((unsigned)nb), dim3(256), 0, st, (const uint64_t*)keys_out, top, (const int32_t*)status, (long long*)result);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
