// Attention over the rows of a CSR: the one primitive of PyG TransformerConv(heads = 1, no edge features, no beta) that is not a GEMM
// (Link_prediction_model/layer.py:77-83, the `Transformer` encoder).  With Q, K, V, S = the four projections of the node rows (fp32, D wide):
//     s_j    = <Q[v], K[u_j]> / sqrt(D)                          for every in-edge j = (u_j -> v), multiplicity and self loops as the CSR lists them
//     a_j    = exp(s_j - max_j s) / sum_j exp(s_j - max_j s)
//     out[v] = act(sum_j a_j V[u_j] + S[v]),   lse[v] = max_j s + log(sum_j exp(s_j - max_j s))         (a row without in-edges: out = act(S[v]), lse = -inf)
// and, with dO the gradient of the sum (the ReLU mask applied by the caller) and a_j recomputed as exp(s_j - lse[v]):
//     delta[v] = sum_j a_j <dO[v], V[u_j]>
//     dQ[v]    = 1/sqrt(D) sum_j a_j (<dO[v], V[u_j]> - delta[v]) K[u_j]                                 (by-dst CSR)
//     dK[u]    = 1/sqrt(D) sum_{j: u -> v} a_j (<dO[v], V[u]> - delta[v]) Q[v],   dV[u] = sum_{j: u -> v} a_j dO[v]      (by-src CSR: the scatter as a gather)
// Nothing of length E is written, there are no atomics, every sum is taken in CSR order: a call is bit-reproducible.
//
// Shape of a wavefront: FOUR groups of 16 lanes, one CSR row per group.  A lane owns the float4s at columns 4 * (gl + 16 i), i < NCH = ceil(D / 64), of
// every row it touches (16 lanes x 16 B = 256 contiguous bytes per load instruction), so
//   - a dot product is NCH x 4 FMAs per lane and FOUR cross-lane steps (xor 1, 2, 4, 8 inside the group) instead of the six of a 64-lane row — and the
//     four groups' reductions run in the same instructions;
//   - the softmax state (max, sum) is one scalar per group and the D-wide accumulator NCH float4s per lane: no merge at the end of a row;
//   - a wavefront keeps 4 groups x U edges in flight, each a K row and a V row (U = 2 up to D = 256: 8 edges = 16 KiB per wavefront at D = 256; U = 1 above).
// The price: the groups of a wavefront walk rows of different lengths (the loop runs to the longest of the four), and a row longer than the view's
// hub_threshold would hold a wavefront long after its neighbours have finished.  Those rows are cut into chunks of hub_threshold edges, ONE WAVEFRONT per
// chunk (its four groups take a quarter of the chunk each and merge in group order), the chunk's partial goes to the view's workspace and one group per hub
// row combines the partials in chunk order: (max, sum, acc[D]) with the usual rescaling in the forward, plain sums in the two backward kernels.
//
// The by-dst backward walks a row TWICE: first for delta[v], then for dQ[v] with (t_j - delta) formed per edge, the expression of the closed form.  The
// one-walk form (two accumulators sum a t K and sum a K, dQ = the first minus delta times the second) cancels where the t_j are close to each other;
// the second walk gathers rows the first one has just brought into the cache.  Hub rows take the two walks as two rounds of chunk + combine launches.
//
// K / V (by-dst) and Q / dO (by-src) rows follow the hot-column flags of the view (col_flags = 1: bit 31 of a column id marks a re-used source row, default
// cache policy; every other gather streams).  The flags choose a cache policy only: results do not depend on them.
#include <type_traits>

#include "cb_common.h"
#include "cb_spmm_core.h"

namespace cb {

constexpr int kAG = 16;            // lanes of a row group
constexpr int kAttnMaxD = 512;     // NCH <= 8
enum { A_FWD = 0, A_DELTA = 1, A_DQ = 2, A_SRC = 3, A_DST = 4 };      // A_DST: the row kernel's A_DELTA walk followed by its A_DQ walk

struct AttnArgs {
  const int* rowptr;
  const int* col;
  int n_rows, hub_T, d, relu;
  float scale;
  const float *q, *k, *v, *skip, *dout;
  int64_t ld_q, ld_k, ld_v, ld_s, ld_do;
  const float* lse_in;        // backward
  const float* delta_in;      // A_DQ (hub rounds), A_SRC
  float* out;                 // A_FWD: out, A_DQ / A_DST: dQ, A_SRC: dK
  int64_t ld_out;
  float* out2;                // A_SRC: dV
  int64_t ld_out2;
  float* lse_out;             // A_FWD, or null
  float* delta_out;           // A_DELTA / A_DST
  int n_hubs, n_chunks;
  const int* hub_rows;
  const int* hub_chunk_ptr;
  float* ws;                  // hub partials: ld_p floats per chunk, [0] = max / delta, [1] = sum, [4 ..] = the accumulators
  int64_t ld_p;
};

// What a group holds of its own row and what it accumulates (members a mode does not touch never exist)
template <int NCH>
struct AttnCtx {
  float r0[NCH][4];      // Q[v]   (A_SRC: K[u])
  float r1[NCH][4];      // dO[v]  (A_SRC: V[u])
  float lse, delta;      // of row v (by-dst backward)
  float m, l;            // A_FWD: running max and sum; A_DELTA: l = the running delta
  float acc[NCH][4];     // A_FWD: sum p V; A_DQ: sum c K; A_SRC: sum c Q
  float acc2[NCH][4];    // A_SRC: sum a dO
};

// Every product, sum and difference below is written with its rounding (__fmaf_rn / __fmul_rn / __fadd_rn / __fsub_rn): left to the compiler's contraction
// choice, the instantiations for the two gather policies gave different bits at D = 256 (a multiply fused into the following sum in one and not the other).
__device__ __forceinline__ float group_sum(float x) {      // over the 16 lanes of a group, every lane gets the same bits
#pragma unroll
  for (int off = 1; off < kAG; off <<= 1) x = __fadd_rn(x, __shfl_xor(x, off));
  return x;
}

template <int NCH>
__device__ __forceinline__ void load_frag(float (&f)[NCH][4], const float* __restrict__ row, int cl, int d, bool nt) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = cl + 64 * i;
    if (c < d) {
      if (nt) gather_nt4(f[i], row + c);
      else gather<4>(f[i], row + c);
    } else {
      zero<4>(f[i]);
    }
  }
}

template <int NCH>
__device__ __forceinline__ void zero_frag(float (&f)[NCH][4]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) zero<4>(f[i]);
}

template <int NCH>
__device__ __forceinline__ float dot_frag(const float (&a)[NCH][4], const float (&b)[NCH][4]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __fmaf_rn(a[i][e], b[i][e], s);
  return group_sum(s);
}

template <int NCH>
__device__ __forceinline__ void axpy_frag(float (&y)[NCH][4], float c, const float (&x)[NCH][4]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) y[i][e] = __fmaf_rn(c, x[i][e], y[i][e]);
}

template <int NCH>
__device__ __forceinline__ void store_frag(float* __restrict__ row, int cl, int d, const float (&f)[NCH][4]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = cl + 64 * i;
    if (c < d) *reinterpret_cast<float4*>(row + c) = make_float4(f[i][0], f[i][1], f[i][2], f[i][3]);
  }
}

// softmax states (m, l, acc) <- (m, l, acc) merged with (mo, lo, acco); an empty state is (-inf, 0, 0)
template <int NCH>
__device__ __forceinline__ void merge_state(float& m, float& l, float (&acc)[NCH][4], float mo, float lo, const float (&acco)[NCH][4]) {
  const float mn = fmaxf(m, mo);
  const float ca = m == -INFINITY ? 0.f : expf(__fsub_rn(m, mn)), cb = mo == -INFINITY ? 0.f : expf(__fsub_rn(mo, mn));
  l = __fmaf_rn(l, ca, __fmul_rn(lo, cb));
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = __fmaf_rn(acc[i][e], ca, __fmul_rn(acco[i][e], cb));
  m = mn;
}

template <int MODE, int NCH>
__device__ __forceinline__ void init_ctx(const AttnArgs& a, AttnCtx<NCH>& c, int row, int cl) {
  c.m = -INFINITY;
  c.l = 0.f;
  c.lse = 0.f;
  c.delta = 0.f;
  zero_frag<NCH>(c.acc);
  if constexpr (MODE == A_SRC) {
    zero_frag<NCH>(c.acc2);
    load_frag<NCH>(c.r0, a.k + (int64_t)row * a.ld_k, cl, a.d, false);
    load_frag<NCH>(c.r1, a.v + (int64_t)row * a.ld_v, cl, a.d, false);
  } else {
    load_frag<NCH>(c.r0, a.q + (int64_t)row * a.ld_q, cl, a.d, false);
    if constexpr (MODE != A_FWD) {
      load_frag<NCH>(c.r1, a.dout + (int64_t)row * a.ld_do, cl, a.d, false);
      c.lse = a.lse_in[row];
      if constexpr (MODE == A_DQ) c.delta = a.delta_in[row];
    }
  }
}

// U consecutive edges e .. e + U - 1 of the group's row: all gathers first, then the arithmetic, edge by edge in CSR order
template <int MODE, int NCH, bool GP, int U>
__device__ __forceinline__ void attn_step(const AttnArgs& a, AttnCtx<NCH>& c, int e, int cl) {
  float g0[U][NCH][4], g1[U][NCH][4];      // K, V of the source (A_SRC: Q, dO of the destination)
  float sl[U], sd[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int craw = a.col[e + u];
    const int64_t j = GP ? (craw & kColMask) : craw;
    const bool nt = GP && craw >= 0;
    if constexpr (MODE == A_SRC) {
      load_frag<NCH>(g0[u], a.q + j * a.ld_q, cl, a.d, nt);
      load_frag<NCH>(g1[u], a.dout + j * a.ld_do, cl, a.d, nt);
      sl[u] = a.lse_in[j];
      sd[u] = a.delta_in[j];
    } else {
      load_frag<NCH>(g0[u], a.k + j * a.ld_k, cl, a.d, nt);
      load_frag<NCH>(g1[u], a.v + j * a.ld_v, cl, a.d, nt);
      sl[u] = c.lse;
      sd[u] = c.delta;
    }
  }
  float s[U];
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = __fmul_rn(dot_frag<NCH>(c.r0, g0[u]), a.scale);
  if constexpr (MODE == A_FWD) {
    float mn = c.m;
#pragma unroll
    for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
    const float c0 = expf(__fsub_rn(c.m, mn));      // (first edges of a row: exp(-inf) = 0 on a zero state)
    c.l = __fmul_rn(c.l, c0);
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) c.acc[i][k] = __fmul_rn(c.acc[i][k], c0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = expf(__fsub_rn(s[u], mn));
      c.l = __fadd_rn(c.l, p);
      axpy_frag<NCH>(c.acc, p, g1[u]);
    }
    c.m = mn;
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float t = dot_frag<NCH>(c.r1, g1[u]);
      const float w = expf(__fsub_rn(s[u], sl[u]));
      if constexpr (MODE == A_DELTA) {
        c.l = __fmaf_rn(w, t, c.l);
      } else {
        axpy_frag<NCH>(c.acc, __fmul_rn(w, __fsub_rn(t, sd[u])), g0[u]);
        if constexpr (MODE == A_SRC) axpy_frag<NCH>(c.acc2, w, g1[u]);
      }
    }
  }
}

template <int MODE, int NCH, bool GP>
__device__ __forceinline__ void attn_walk(const AttnArgs& a, AttnCtx<NCH>& c, int e0, int e1, int cl) {
  constexpr int U = NCH <= 4 ? 2 : 1;
  int e = e0;
  if constexpr (U > 1) {
    for (; e + U <= e1; e += U) attn_step<MODE, NCH, GP, U>(a, c, e, cl);
  }
  for (; e < e1; ++e) attn_step<MODE, NCH, GP, 1>(a, c, e, cl);
}

// The finished row (all lanes of the group; scalars by its lane 0).  A row is empty where l == 0 (a row with edges has l >= 1: its largest score
// contributes exp(0)); an l that is not a number — a NaN or +Inf score — is NOT empty: the row and its lse come out NaN, never act(skip) and -inf
template <int MODE, int NCH>
__device__ __forceinline__ void attn_store(const AttnArgs& a, AttnCtx<NCH>& c, int row, int cl, int gl) {
  if constexpr (MODE == A_FWD) {
    float sk[NCH][4];
    load_frag<NCH>(sk, a.skip + (int64_t)row * a.ld_s, cl, a.d, true);
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float o = __fadd_rn(c.l == 0.f ? 0.f : __fdiv_rn(c.acc[i][e], c.l), sk[i][e]);
        c.acc[i][e] = a.relu ? relu_nan(o) : o;
      }
    store_frag<NCH>(a.out + (int64_t)row * a.ld_out, cl, a.d, c.acc);
    if (a.lse_out && gl == 0) a.lse_out[row] = c.l == 0.f ? -INFINITY : __fadd_rn(c.m, logf(c.l));
  } else if constexpr (MODE == A_DELTA) {
    if (gl == 0) a.delta_out[row] = c.l;
  } else {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) c.acc[i][e] = __fmul_rn(c.acc[i][e], a.scale);
    store_frag<NCH>(a.out + (int64_t)row * a.ld_out, cl, a.d, c.acc);
    if constexpr (MODE == A_SRC) store_frag<NCH>(a.out2 + (int64_t)row * a.ld_out2, cl, a.d, c.acc2);
  }
}

// One group per row; rows longer than hub_T are left to the hub kernels
template <int KMODE, int NCH, bool GP>
__global__ void __launch_bounds__(256) k_attn_rows(AttnArgs a) {
  const int gl = threadIdx.x & (kAG - 1), cl = gl * 4;
  const int64_t row64 = (int64_t)blockIdx.x * (256 / kAG) + (threadIdx.x / kAG);
  if (row64 >= a.n_rows) return;
  const int row = (int)row64;
  const int e0 = a.rowptr[row], e1 = a.rowptr[row + 1];
  if (e1 - e0 > a.hub_T) return;
  AttnCtx<NCH> c;
  if constexpr (KMODE == A_DST) {
    init_ctx<A_DELTA, NCH>(a, c, row, cl);
    attn_walk<A_DELTA, NCH, GP>(a, c, e0, e1, cl);
    attn_store<A_DELTA, NCH>(a, c, row, cl, gl);
    c.delta = c.l;
    attn_walk<A_DQ, NCH, GP>(a, c, e0, e1, cl);
    attn_store<A_DQ, NCH>(a, c, row, cl, gl);
  } else {
    init_ctx<KMODE, NCH>(a, c, row, cl);
    attn_walk<KMODE, NCH, GP>(a, c, e0, e1, cl);
    attn_store<KMODE, NCH>(a, c, row, cl, gl);
  }
}

// One wavefront per chunk of hub_T edges of a hub row: its four groups take a quarter of the chunk each, merge, and group 0 writes the partial
template <int MODE, int NCH, bool GP>
__global__ void __launch_bounds__(256) k_attn_hub_chunks(AttnArgs a) {
  const int lane = lane_id(), gl = lane & (kAG - 1), cl = gl * 4, grp = lane / kAG;
  const int chunk = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (chunk >= a.n_chunks) return;
  int lo = 0, hi = a.n_hubs;      // hub index: last i with hub_chunk_ptr[i] <= chunk (wave-uniform binary search)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.hub_chunk_ptr[mid] <= chunk) lo = mid; else hi = mid;
  }
  const int row = a.hub_rows[lo];
  const int cb0 = a.rowptr[row] + (chunk - a.hub_chunk_ptr[lo]) * a.hub_T;
  const int cb1 = min(cb0 + a.hub_T, a.rowptr[row + 1]);
  const int quarter = (cb1 - cb0 + 3) / 4;
  const int e0 = min(cb0 + grp * quarter, cb1), e1 = min(e0 + quarter, cb1);
  AttnCtx<NCH> c;
  init_ctx<MODE, NCH>(a, c, row, cl);
  attn_walk<MODE, NCH, GP>(a, c, e0, e1, cl);
#pragma unroll
  for (int off = kAG; off < kWave; off <<= 1) {      // groups (0 + 1) + (2 + 3): every lane is active here
    if constexpr (MODE == A_FWD) {
      float acco[NCH][4];
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acco[i][e] = __shfl_xor(c.acc[i][e], off);
      const float mo = __shfl_xor(c.m, off), lo_ = __shfl_xor(c.l, off);
      // (own, other) in every lane: what groups 0 and 2 hold after the first step, and group 0 after the second, is the merge in group order — the
      // upper group of a pair holds the operands the other way round, and nothing reads it)
      merge_state<NCH>(c.m, c.l, c.acc, mo, lo_, acco);
    } else if constexpr (MODE == A_DELTA) {
      c.l = __fadd_rn(c.l, __shfl_xor(c.l, off));
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c.acc[i][e] = __fadd_rn(c.acc[i][e], __shfl_xor(c.acc[i][e], off));
          if constexpr (MODE == A_SRC) c.acc2[i][e] = __fadd_rn(c.acc2[i][e], __shfl_xor(c.acc2[i][e], off));
        }
    }
  }
  if (grp != 0) return;
  float* p = a.ws + (int64_t)chunk * a.ld_p;
  if (gl == 0) {
    p[0] = MODE == A_FWD ? c.m : c.l;
    p[1] = c.l;
  }
  if constexpr (MODE != A_DELTA) store_frag<NCH>(p + 4, cl, a.d, c.acc);
  if constexpr (MODE == A_SRC) store_frag<NCH>(p + 4 + a.d, cl, a.d, c.acc2);
}

// One group per hub row: the partials combined in chunk order, then the row's store
template <int MODE, int NCH>
__global__ void __launch_bounds__(256) k_attn_hub_finish(AttnArgs a) {
  const int gl = threadIdx.x & (kAG - 1), cl = gl * 4;
  const int i = (int)blockIdx.x * (256 / kAG) + (int)(threadIdx.x / kAG);
  if (i >= a.n_hubs) return;
  const int row = a.hub_rows[i];
  AttnCtx<NCH> c;
  c.m = -INFINITY;
  c.l = 0.f;
  zero_frag<NCH>(c.acc);
  if constexpr (MODE == A_SRC) zero_frag<NCH>(c.acc2);
  for (int ch = a.hub_chunk_ptr[i]; ch < a.hub_chunk_ptr[i + 1]; ++ch) {
    const float* p = a.ws + (int64_t)ch * a.ld_p;
    if constexpr (MODE == A_FWD) {
      float acco[NCH][4];
      load_frag<NCH>(acco, p + 4, cl, a.d, false);
      merge_state<NCH>(c.m, c.l, c.acc, p[0], p[1], acco);
    } else if constexpr (MODE == A_DELTA) {
      c.l = __fadd_rn(c.l, p[0]);
    } else {
      float t[NCH][4];
      load_frag<NCH>(t, p + 4, cl, a.d, false);
      axpy_frag<NCH>(c.acc, 1.f, t);
      if constexpr (MODE == A_SRC) {
        load_frag<NCH>(t, p + 4 + a.d, cl, a.d, false);
        axpy_frag<NCH>(c.acc2, 1.f, t);
      }
    }
  }
  attn_store<MODE, NCH>(a, c, row, cl, gl);
}

static inline bool attn_rows_ok(int64_t d, const void* p, int64_t ld) {
  return d > 0 && d % 4 == 0 && d <= kAttnMaxD && p != nullptr && aligned16(p) && ld % 4 == 0 && ld >= d;
}

template <class F>
static inline void dispatch_nch(int64_t d, F&& f) {
  if (d <= 64) f(std::integral_constant<int, 1>{});
  else if (d <= 128) f(std::integral_constant<int, 2>{});
  else if (d <= 256) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// The graph side of an entry: the view checked for partials of 2 d + 4 floats per chunk (cb_attn_workspace_bytes), the launch arguments' graph part filled
static int attn_graph(const char* who, const cb_csr_view* g, int64_t d, AttnArgs& a, cb_csr_view& v) {
  CB_CHECK_ARG(g != nullptr, CB_E_INVALID, "%s: the graph view is null", who);
  CB_CHECK_ARG(d > 0 && d % 4 == 0 && d <= kAttnMaxD, CB_E_INVALID, "%s: D = %lld is not built (D %% 4 == 0, D <= %d); ask cb_attn_supported first", who,
               (long long)d, kAttnMaxD);
  const int rc = check_csr_view(who, g, 2 * d + 4, v);
  if (rc != CB_OK) return rc;
  CB_CHECK_ARG(v.n_hubs == 0 || aligned16(v.ws), CB_E_WORKSPACE, "%s: misaligned workspace", who);
  a.rowptr = v.rowptr; a.col = v.col; a.n_rows = (int)v.n_rows; a.hub_T = v.hub_threshold; a.d = (int)d;
  a.scale = 1.0f / sqrtf((float)d);
  a.n_hubs = v.n_hubs; a.n_chunks = v.n_chunks; a.hub_rows = v.hub_rows; a.hub_chunk_ptr = v.hub_chunk_ptr;
  a.ws = (float*)v.ws; a.ld_p = 2 * d + 4;
  return CB_OK;
}

template <int KMODE>
static int launch_rows(const AttnArgs& a, bool gp, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)a.n_rows + 256 / kAG - 1) / (256 / kAG)));
  dispatch_nch(a.d, [&](auto NCH) {
    dispatch_bool(gp, [&](auto GP) { hipLaunchKernelGGL((k_attn_rows<KMODE, decltype(NCH)::value, decltype(GP)::value>), grid, dim3(256), 0, st, a); });
  });
  CB_LAUNCH_CHECK();
  return CB_OK;
}

template <int MODE>
static int launch_hubs(const AttnArgs& a, bool gp, hipStream_t st) {
  if (a.n_hubs <= 0) return CB_OK;
  const dim3 gridc((unsigned)((a.n_chunks + 3) / 4)), gridf((unsigned)((a.n_hubs + 256 / kAG - 1) / (256 / kAG)));
  dispatch_nch(a.d, [&](auto NCH) {
    dispatch_bool(gp, [&](auto GP) { hipLaunchKernelGGL((k_attn_hub_chunks<MODE, decltype(NCH)::value, decltype(GP)::value>), gridc, dim3(256), 0, st, a); });
  });
  CB_LAUNCH_CHECK();
  dispatch_nch(a.d, [&](auto NCH) { hipLaunchKernelGGL((k_attn_hub_finish<MODE, decltype(NCH)::value>), gridf, dim3(256), 0, st, a); });
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb

using namespace cb;

extern "C" int cb_attn_supported(int64_t d, const void* rows, int64_t ld) { return attn_rows_ok(d, rows, ld) ? 1 : 0; }

extern "C" size_t cb_attn_workspace_bytes(int64_t n_chunks, int64_t d) {
  if (n_chunks <= 0 || d <= 0) return 0;
  return (size_t)n_chunks * (size_t)(2 * d + 4) * sizeof(float);
}

#define CB_ATTN_ROWS(p, ld, what) \
  CB_CHECK_ARG(attn_rows_ok(d, p, ld), CB_E_INVALID, "%s: " what ": 16-byte aligned fp32 rows with ld %% 4 == 0 and ld >= D required; ask cb_attn_supported first", who)

extern "C" int cb_attn_fwd_f32(const cb_csr_view* g, int64_t d, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                               const float* skip, int64_t ld_s, int relu, float* out, int64_t ld_out, float* lse, void* stream) {
  const char* who = "cb_attn_fwd_f32";
  AttnArgs a{};
  cb_csr_view vw;
  const int rc = attn_graph(who, g, d, a, vw);
  if (rc != CB_OK || vw.n_rows == 0) return rc;
  CB_ATTN_ROWS(q, ld_q, "q");
  CB_ATTN_ROWS(k, ld_k, "k");
  CB_ATTN_ROWS(v, ld_v, "v");
  CB_ATTN_ROWS(skip, ld_s, "skip");
  CB_ATTN_ROWS(out, ld_out, "out");
  a.q = q; a.ld_q = ld_q; a.k = k; a.ld_k = ld_k; a.v = v; a.ld_v = ld_v; a.skip = skip; a.ld_s = ld_s;
  a.relu = relu; a.out = out; a.ld_out = ld_out; a.lse_out = lse;
  hipStream_t st = (hipStream_t)stream;
  const bool gp = vw.col_flags != 0;
  const int rh = launch_hubs<A_FWD>(a, gp, st);
  if (rh != CB_OK) return rh;
  return launch_rows<A_FWD>(a, gp, st);
}

extern "C" int cb_attn_bwd_dst_f32(const cb_csr_view* g, int64_t d, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                                   const float* dout, int64_t ld_do, const float* lse, float* dq, int64_t ld_dq, float* delta, void* stream) {
  const char* who = "cb_attn_bwd_dst_f32";
  AttnArgs a{};
  cb_csr_view vw;
  const int rc = attn_graph(who, g, d, a, vw);
  if (rc != CB_OK || vw.n_rows == 0) return rc;
  CB_ATTN_ROWS(q, ld_q, "q");
  CB_ATTN_ROWS(k, ld_k, "k");
  CB_ATTN_ROWS(v, ld_v, "v");
  CB_ATTN_ROWS(dout, ld_do, "dout");
  CB_ATTN_ROWS(dq, ld_dq, "dq");
  CB_CHECK_ARG(lse && delta, CB_E_INVALID, "%s: null lse / delta", who);
  a.q = q; a.ld_q = ld_q; a.k = k; a.ld_k = ld_k; a.v = v; a.ld_v = ld_v; a.dout = dout; a.ld_do = ld_do;
  a.lse_in = lse; a.delta_in = delta; a.delta_out = delta; a.out = dq; a.ld_out = ld_dq;
  hipStream_t st = (hipStream_t)stream;
  const bool gp = vw.col_flags != 0;
  int rh = launch_hubs<A_DELTA>(a, gp, st);      // delta of the hub rows, then their dQ (the workspace serves both rounds in turn)
  if (rh == CB_OK) rh = launch_hubs<A_DQ>(a, gp, st);
  if (rh != CB_OK) return rh;
  return launch_rows<A_DST>(a, gp, st);
}

extern "C" int cb_attn_bwd_src_f32(const cb_csr_view* g_src, int64_t d, const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v,
                                   const float* dout, int64_t ld_do, const float* lse, const float* delta, float* dk, int64_t ld_dk, float* dv, int64_t ld_dv,
                                   void* stream) {
  const char* who = "cb_attn_bwd_src_f32";
  AttnArgs a{};
  cb_csr_view vw;
  const int rc = attn_graph(who, g_src, d, a, vw);
  if (rc != CB_OK || vw.n_rows == 0) return rc;
  CB_ATTN_ROWS(q, ld_q, "q");
  CB_ATTN_ROWS(k, ld_k, "k");
  CB_ATTN_ROWS(v, ld_v, "v");
  CB_ATTN_ROWS(dout, ld_do, "dout");
  CB_ATTN_ROWS(dk, ld_dk, "dk");
  CB_ATTN_ROWS(dv, ld_dv, "dv");
  CB_CHECK_ARG(lse && delta, CB_E_INVALID, "%s: null lse / delta", who);
  a.q = q; a.ld_q = ld_q; a.k = k; a.ld_k = ld_k; a.v = v; a.ld_v = ld_v; a.dout = dout; a.ld_do = ld_do;
  a.lse_in = lse; a.delta_in = delta; a.out = dk; a.ld_out = ld_dk; a.out2 = dv; a.ld_out2 = ld_dv;
  hipStream_t st = (hipStream_t)stream;
  const bool gp = vw.col_flags != 0;
  const int rh = launch_hubs<A_SRC>(a, gp, st);
  if (rh != CB_OK) return rh;
  return launch_rows<A_SRC>(a, gp, st);
}
