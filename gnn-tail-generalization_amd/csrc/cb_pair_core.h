// The device core of everything that works on index pairs over an embedding matrix, written once: the edge-wise BCE loss (cb_linkp.hip) and the
// link predictors (cb_linkpred.hip) call it, so their scores and their scatter are bit-identical because they are one piece of code.
//
//   source    PairSource: up to two [2, n] segments read as one run of pairs (pos | neg of the loss, or one `pairs` array).  get() is the only
//             read of an endpoint: an endpoint outside [0, N) (the -1 of a failed sampler slot) makes the pair unusable and never becomes an index.
//             Whether there is a second segment is a compile-time flag: the one-segment form pays no branch per pair, which the scatter's serial
//             walk of a hub node's run would feel (about 2 % of its time when measured).
//   pair dot  k_pair_dot: s_e = <h[u_e], h[v_e]> in fp32, one wavefront per pair, a fixed-shape reduction; NaN for an unusable pair.
//   scatter   dH[n] = sum of coef_e * h[v_e] into row u_e and coef_e * h[u_e] into row v_e without atomics: contribution c = 2 e + side gets the
//             key c << 32 | node (k_pair_keys), the keys are sorted by node (cb::sort_u64, stable: ascending contribution number inside a node),
//             and the wavefront at the head of a node's run adds the run in that order in float64, rounds once and writes the row
//             (k_pair_scatter_rows); all other rows are zero-filled before.  The coefficient is a functor: a scalar per pair, a row per pair, or
//             the BCE-with-logits derivative formed in float64 from the score; CoefAsIs contributes a row as it stands instead of a multiple of the
//             other endpoint's row (cb_pairpred.hip).
//   tree      block_tree_f64: the 256-thread float64 halving tree of the loss finishers.
// No float atomics, no host synchronisation, two calls with the same inputs give the same bits.
#pragma once
#include "cb_common.h"
#include "cb_sort.h"

namespace cb {

// pair e < na: (a[e], a[na + e]); else (b[e - na], b[nb + e - na]).  TWO == false: one segment, b and nb are not read.
template <bool TWO>
struct PairSource {
  const int32_t* a;
  int64_t na;
  const int32_t* b;
  int64_t nb;

  __host__ __device__ int64_t size() const { return TWO ? na + nb : na; }

  // false for an endpoint outside [0, N) (never used as an index)
  __device__ __forceinline__ bool get(int64_t e, int64_t N, int& u, int& v) const {
    if (!TWO || e < na) {
      u = a[e];
      v = a[na + e];
    } else {
      u = b[e - na];
      v = b[nb + e - na];
    }
    return u >= 0 && u < N && v >= 0 && v < N;
  }
};

// ---- pair dot -------------------------------------------------------------------------------------------------------------------------
// status (may be NULL: the caller counts elsewhere) += 1 per unusable pair (integer atomic: order-independent)
template <bool VEC, bool TWO>
__global__ void __launch_bounds__(256) k_pair_dot(const float* __restrict__ h, int64_t ld, int64_t N, int D, PairSource<TWO> src,
                                                  float* __restrict__ scores, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (e >= src.size()) return;
  int u, v;
  if (!src.get(e, N, u, v)) {      // (wave-uniform)
    if (lane == 0) {
      scores[e] = __int_as_float(0x7FC00000);
      if (status) atomicAdd(status, 1);
    }
    return;
  }
  const float* a = h + (int64_t)u * ld;
  const float* b = h + (int64_t)v * ld;
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

template <bool TWO>
static int launch_pair_dot(const float* h, int64_t ld, int64_t N, int64_t D, const PairSource<TWO>& src, float* scores, int32_t* status, hipStream_t st) {
  const unsigned nb = (unsigned)blocks_for(src.size(), 4);
  if (D % 4 == 0 && ld % 4 == 0 && aligned16(h))
    hipLaunchKernelGGL((k_pair_dot<true, TWO>), dim3(nb), dim3(256), 0, st, h, ld, N, (int)D, src, scores, status);
  else
    hipLaunchKernelGGL((k_pair_dot<false, TWO>), dim3(nb), dim3(256), 0, st, h, ld, N, (int)D, src, scores, status);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// ---- scatter --------------------------------------------------------------------------------------------------------------------------
// The coefficient of contribution (pair e, column cc) in float64, in three steps so that each form does its work where it always did:
// wave() once per wavefront, pair(e, w) once per contribution, col(e, cc, p) per column.
struct CoefScalar {      // c [S]: a scalar per pair
  static constexpr bool AS_IS = false;
  const float* c;
  __device__ __forceinline__ double wave() const { return 0.0; }
  __device__ __forceinline__ double pair(int64_t e, double) const { return (double)c[e]; }
  __device__ __forceinline__ double col(int64_t, int, double p) const { return p; }
};

struct CoefRows {      // c [S, ld]: a row per pair
  static constexpr bool AS_IS = false;
  const float* c;
  int64_t ld;
  __device__ __forceinline__ double wave() const { return 0.0; }
  __device__ __forceinline__ double pair(int64_t, double) const { return 0.0; }
  __device__ __forceinline__ double col(int64_t e, int cc, double) const { return (double)c[e * ld + cc]; }
};

struct CoefBce {      // g (sigmoid(s_e) - y_e) / S from the scores; y_e = 1 for the P first pairs
  static constexpr bool AS_IS = false;
  const float* scores;
  const float* g;
  int64_t P, S;
  __device__ __forceinline__ double wave() const { return (double)g[0] / (double)S; }
  __device__ __forceinline__ double pair(int64_t e, double scale) const {
    const double s = (double)scores[e];
    return scale * (1.0 / (1.0 + exp(-s)) - (e < P ? 1.0 : 0.0));
  }
  __device__ __forceinline__ double col(int64_t, int, double p) const { return p; }
};

// AS_IS: the contribution is a row as it stands, g0[e] into row u_e and g1[e] into row v_e (the backward of the two gathers of an indexed-row GEMM):
// no row of h is read (the scatter is run with h == nullptr), and term() replaces coefficient times other row.
struct CoefAsIs {
  static constexpr bool AS_IS = true;
  const float* g0;
  int64_t ld0;
  const float* g1;
  int64_t ld1;
  __device__ __forceinline__ double wave() const { return 0.0; }
  __device__ __forceinline__ double pair(int64_t, double) const { return 0.0; }
  __device__ __forceinline__ double term(int64_t e, int side, int cc) const { return (double)(side ? g1[e * ld1 + cc] : g0[e * ld0 + cc]); }
};

// contribution c = 2 e + side goes to node (side ? v_e : u_e); key = c << 32 | node, node = N for an unusable pair (sorted last, skipped)
template <bool TWO>
__global__ void __launch_bounds__(256) k_pair_keys(PairSource<TWO> src, int64_t N, uint64_t* __restrict__ keys) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * src.size()) return;
  int u, v;
  const bool ok = src.get(c >> 1, N, u, v);
  const uint64_t node = ok ? (uint64_t)((c & 1) ? v : u) : (uint64_t)N;
  keys[c] = ((uint64_t)c << 32) | node;
}

// One wavefront per sorted position; the one at the head of a node's run owns the node's row of dH.  Columns in chunks of 256 (four per lane); wider
// rows walk the run once per chunk.
template <bool TWO, typename Coef>
__global__ void __launch_bounds__(256) k_pair_scatter_rows(const float* __restrict__ h, int64_t ld, int64_t N, int D, PairSource<TWO> src, Coef coef,
                                                           const uint64_t* __restrict__ keys, float* __restrict__ dh, int64_t ldd) {
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_keys = 2 * src.size();
  if (i >= n_keys) return;
  const uint32_t node = (uint32_t)keys[i];
  if (node >= (uint32_t)N) return;
  if (i > 0 && (uint32_t)keys[i - 1] == node) return;      // not the head of its run
  const double cw = coef.wave();
  for (int c0 = 0; c0 < D; c0 += 256) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j = i; j < n_keys; ++j) {
      const uint64_t key = keys[j];      // (wave-uniform)
      if ((uint32_t)key != node) break;
      const int64_t c = (int64_t)(key >> 32), e = c >> 1;      // (e < S: the keys are a permutation of those k_pair_keys wrote)
      int u, v;
      src.get(e, N, u, v);      // (usable: its node is < N)
      if constexpr (Coef::AS_IS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cc = c0 + lane + 64 * q;
          if (cc < D) acc[q] += coef.term(e, (int)(c & 1), cc);
        }
      } else {
        const float* other = h + (int64_t)((c & 1) ? u : v) * ld;
        const double cp = coef.pair(e, cw);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cc = c0 + lane + 64 * q;
          if (cc < D) acc[q] = fma(coef.col(e, cc, cp), (double)other[cc], acc[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cc = c0 + lane + 64 * q;
      if (cc < D) dh[(int64_t)node * ldd + cc] = (float)acc[q];
    }
  }
}

static inline int pair_bits(int64_t n) {
  int b = 0;
  while (((int64_t)1 << b) < n) ++b;
  return b;
}

static inline size_t pair_keys_bytes(int64_t S) { return align_up((size_t)(2 * S) * sizeof(uint64_t), 256); }

// workspace of pair_scatter for S > 0 pairs: the keys, their sorted copy, the sort's scratch
static inline size_t pair_scatter_ws_bytes(int64_t S) { return 2 * pair_keys_bytes(S) + align_up(sort_u64_temp_bytes(2 * S), 256); }

// dh [N, D] (ldd >= D) = the scatter of src with coef: zero fill, keys, sort by node, rows.  ws: pair_scatter_ws_bytes(src.size()), unused for no pairs.
template <bool TWO, typename Coef>
static int pair_scatter(const float* h, int64_t ld, int64_t N, int64_t D, const PairSource<TWO>& src, const Coef& coef, float* dh, int64_t ldd, void* ws,
                        size_t ws_bytes, hipStream_t st) {
  const int64_t S = src.size();
  if (ldd == D) {
    CB_HIP(hipMemsetAsync(dh, 0, (size_t)N * (size_t)D * sizeof(float), st));
  } else {
    CB_HIP(hipMemset2DAsync(dh, (size_t)ldd * sizeof(float), 0, (size_t)D * sizeof(float), (size_t)N, st));
  }
  if (S == 0) return CB_OK;
  char* base = (char*)ws;
  uint64_t* keys_in = (uint64_t*)base;
  uint64_t* keys_out = (uint64_t*)(base + pair_keys_bytes(S));
  void* temp = base + 2 * pair_keys_bytes(S);
  hipLaunchKernelGGL(k_pair_keys<TWO>, dim3((unsigned)blocks_for(2 * S, 256)), dim3(256), 0, st, src, N, keys_in);
  CB_LAUNCH_CHECK();
  const int rc = sort_u64(temp, ws_bytes - 2 * pair_keys_bytes(S), keys_in, keys_out, 2 * S, pair_bits(N + 1), st);
  if (rc != CB_OK) return rc;
  hipLaunchKernelGGL((k_pair_scatter_rows<TWO, Coef>), dim3((unsigned)blocks_for(2 * S, 4)), dim3(256), 0, st, h, ld, N, (int)D, src, coef,
                     (const uint64_t*)keys_out, dh, ldd);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// the size checks of an entry over h [N, D] (ld) and S pairs; count_ok / count_txt: what the entry asks of its pair counts
#define CB_PAIR_CHECK_SIZES(name, S, count_ok, count_txt)                                                                               \
  CB_CHECK_ARG(N > 0 && D > 0 && ld >= D && (count_ok), CB_E_INVALID, name ": bad size (N > 0, D > 0, ld >= D, " count_txt " required)"); \
  CB_CHECK_ARG(N < INT32_MAX && D < (1 << 24) && (S) < INT32_MAX / 2, CB_E_RANGE, name ": size out of range")

// ---- float64 block tree ---------------------------------------------------------------------------------------------------------------
// s[v][0] = the sum of s[v][0 .. 255] for each of the NV rows: a halving tree over the 256 threads of the block, one fixed order.  Begins with a
// barrier (the caller has just written s[.][t]); thread 0 reads the sums after it returns.
template <int NV>
__device__ __forceinline__ void block_tree_f64(double (&s)[NV][256], int t) {
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int v = 0; v < NV; ++v) s[v][t] += s[v][t + off];
    }
    __syncthreads();
  }
}

}  // namespace cb
