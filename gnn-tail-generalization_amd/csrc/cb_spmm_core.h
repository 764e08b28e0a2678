// The core of the CSR sum-aggregation (design notes: cb_spmm.hip), shared by cb_spmm.hip (the aggregation entry points), cb_agg_gemm.hip (aggregation +
// next dense transform in one kernel), cb_sage_core.h (the encoder layer: cb_sage.hip, cb_ewlayer.hip) and, for the row block's head, cb_spmm_small.hip.
// EW (stream_rows, k_spmm_rows, k_spmm_hub_chunks, launch_hub_rows; default off): one factor per stored EDGE, Epilogue::edge_w — the adjacency with values.
//   device: vector helpers and the epilogues; RowBlock + load_row_block (the head of a wavefront's row block), tile_row_cut / zero_tile_rows (a 64-row
//           tile among the gathering wavefronts), stream_rows (the edge-stream walk), the row / hub kernels;
//   host:   check_csr_view, partial_ld, dispatch_bool / dispatch_gp_cs (run-time flags as compile-time constants) and launch_hub_rows.
// What is still written out per kernel, on purpose (profiles/agg_core.md: each of these, shared, changes the registers or the schedule of a kernel):
// stream_rows' positional operands, its three accumulation forks and k_spmm_hub_chunks' two, the loop over the runs between hub rows, and
// k_spmm_rows' own copy of the head.
#pragma once
#include <type_traits>

#include "cb_common.h"
#include "cb_philox.h"
#include "cb_trunk_store.h"

namespace cb {

template <int VEC>
struct Vec;
template <>
struct Vec<1> {
  using T = float;
};
template <>
struct Vec<2> {
  using T = float2;
};
template <>
struct Vec<4> {
  using T = float4;
};

template <int VEC>
__device__ __forceinline__ void zero(float (&a)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) a[i] = 0.f;
}

template <int VEC>
__device__ __forceinline__ void gather(float (&v)[VEC], const float* __restrict__ p) {
  using T = typename Vec<VEC>::T;
  T t = *reinterpret_cast<const T*>(p);
  if constexpr (VEC == 1) {
    v[0] = t;
  } else if constexpr (VEC == 2) {
    v[0] = t.x;
    v[1] = t.y;
  } else {
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  }
}

// Row that is read exactly once (the mixed-in X0 row of the fused store): keep it out of L2 / Infinity Cache, which hold the
// re-used hub source rows
template <int VEC>
__device__ __forceinline__ void gather_stream(float (&v)[VEC], const float* __restrict__ p) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) v[i] = __builtin_nontemporal_load(p + i);
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// fp32 x4 source row chunk with the streaming (nt) cache policy: one global_load_dwordx4 ... nt
__device__ __forceinline__ void gather_nt4(float (&v)[4], const float* __restrict__ p) {
  const f32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}

// bf16 x4 source row chunk (8 bytes), streaming policy
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void gather_nt4_bf16(float (&v)[4], const void* __restrict__ p) {
  const u32x2_t t = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
  v[0] = __uint_as_float(t[0] << 16);
  v[1] = __uint_as_float(t[0] & 0xFFFF0000u);
  v[2] = __uint_as_float(t[1] << 16);
  v[3] = __uint_as_float(t[1] & 0xFFFF0000u);
}

// Gather policy of the source-row loads (GP): 0 = default cache policy for every row; 1 = every row streaming (nt);
// 2 = the CSR's column ids carry a "hot source" flag in bit 31 (set at graph build for the most-referenced source rows):
// hot rows default policy, all others streaming, so that the rows that ARE re-used keep L2 / Infinity Cache to themselves.
constexpr int kColMask = 0x7fffffff;

// Source-row load of the aggregation: fp32 rows, or bf16-stored rows widened to fp32 (accumulation stays fp32)
template <int VEC, typename HT>
__device__ __forceinline__ void gather_in(float (&v)[VEC], const HT* __restrict__ p) {
  if constexpr (sizeof(HT) == 4) {
    gather<VEC>(v, reinterpret_cast<const float*>(p));
  } else if constexpr (VEC == 4) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16);
    v[1] = __uint_as_float(t.x & 0xFFFF0000u);
    v[2] = __uint_as_float(t.y << 16);
    v[3] = __uint_as_float(t.y & 0xFFFF0000u);
  } else if constexpr (VEC == 2) {
    const uint32_t t = *reinterpret_cast<const uint32_t*>(p);
    v[0] = __uint_as_float(t << 16);
    v[1] = __uint_as_float(t & 0xFFFF0000u);
  } else {
    v[0] = bf16_to_f32(*reinterpret_cast<const bf16_t*>(p));
  }
}

template <int VEC>
__device__ __forceinline__ void store_stream(float* __restrict__ p, const float (&v)[VEC]) {
  // written once, read by a later kernel: keep it out of the caches
#pragma unroll
  for (int i = 0; i < VEC; ++i) __builtin_nontemporal_store(v[i], p + i);
}

struct Epilogue {
  const float* row_scale;  // [N] or null
  const float* bias;       // [d] or null
  int relu;
  // ACC kernels only: partial sums [N, ld_init] the reduction starts from (the interior-column pass of the node-sharded
  // path, dist.py: out = act(row_scale * (acc_init + sum over THIS CSR's columns) + bias))
  const float* acc_init;
  int64_t ld_init;
  int col_flags;           // 1: bit 31 of every column id marks a hot source row (gather policy 2, see gather_pol)
  // label-propagation step (outcome_correlation.py:137-143 with alpha_term, post_step = clamp(0, 1)), narrow rows (VEC < 4 kernels) only:
  //   out[v] = lp_post[v] * clamp(row_scale[v] * acc + lp_c_mix * lp_mix[v], 0, 1)        (lp_post = null: 1)
  // i.e. alpha * D^-1/2 A (.) + (1 - alpha) * y0, clamped, and already scaled by D^-1/2 for the next step's gather
  const float* lp_mix;      // [N, ld_lp] or null (null: plain epilogue)
  int64_t ld_lp;
  float lp_c_mix;
  const float* lp_post;     // [N] or null
  // ACC kernels, raw in-place accumulation only (out == acc_init, no scale / bias / ReLU: the intermediate halo passes of the node-sharded
  // aggregation): a row without edges in THIS CSR keeps its running sums as they are — neither read nor written (a halo slice touches only a
  // fraction of the rows; the passes are otherwise bound by reading and re-writing all of them)
  int acc_skip_empty;
  // CS kernels (d % 256 == 0, fp32 rows, plain store): out[v] = row_scale[v] * sum_u col_scale[u] * h[u] — the factor of a SOURCE row applied
  // as the row is gathered (the row-sparse backward's A (a * X) on the loss rows: no scaled copy of X, trunk.py)
  const float* col_scale;   // [n_cols] or null
  // generalised propagation step (cb_spmm_csr_prop_f32; the label-propagation entry sets lp_clamp = 1, lp_lo = 0, lp_hi = 1, lp_fix = null):
  //   out[v] = lp_post[v] * fix_v(clamp(row_scale[v] * acc + lp_c_mix * lp_mix[v], lp_lo, lp_hi))
  // lp_clamp = 0: no clamp (the identity post-step); lp_fix ([N] bytes or null): a row with a non-zero byte is replaced by lp_mix[v] itself
  // (fix_inputs, outcome_correlation.py:194-199)
  int lp_clamp;
  float lp_lo, lp_hi;
  const uint8_t* lp_fix;
  // EW kernels (d % 256 == 0, fp32 rows, plain store): out[v] = row_scale[v] * sum_j edge_w[j] * h[col[j]] — one factor per stored EDGE, in the order of
  // this CSR's col array (an adjacency with values: cb_spmm_csr_ew_f32, cb_ewlayer_f32); read by the lane that reads col[j], at the same absolute index
  const float* edge_w;      // [n_edges] or null
};

template <int VEC>
__device__ __forceinline__ void write_row_lp(float* __restrict__ out_row, const float (&acc)[VEC], float scale, const Epilogue& ep, int64_t row,
                                             int c0, bool (&on)[VEC]) {
  const float post = ep.lp_post ? ep.lp_post[row] : 1.f;
  const bool fix = ep.lp_fix && ep.lp_fix[row];      // (wave-uniform)
  float r[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if (!on[i]) continue;
    const float m = ep.lp_mix[row * ep.ld_lp + c0 + i];
    float t = acc[i] * scale;
    t = t + ep.lp_c_mix * m;
    if (ep.lp_clamp) t = fminf(fmaxf(t, ep.lp_lo), ep.lp_hi);
    if (fix) t = m;
    r[i] = t * post;
    __builtin_nontemporal_store(r[i], out_row + i);
  }
}

// Extended epilogue of the fused residual trunk (GCN.py:127-133 folded into the aggregation's store): the trunk's store (cb_trunk_store.h) applied to
//   y = row_scale * acc + bias,   x_next -> out_next (the next stage's input)
// Only for VEC = 4 full tiles (d % 256 == 0): lane l owns columns 4l..4l+3 of its 256-wide tile, the mask
// word k of a (row, tile) holds the ballot of component k over the 64 lanes.
struct FusedEpi {
  TrunkStore st;          // (no mix_index: the mix is taken at the node row)
  float* out_next;        // [N, ld_next]
  int64_t ld_next;
  int d;
  int skip_next;          // cb_agg_gemm.hip, forwards without a backward: the finished row only goes to the on-chip tile, not to out_next
  int bwd;                // BACKWARD of a store applied to the row this (reverse) aggregation just summed (cb_spmm_csr_store_bwd_f32): g = scale * acc goes to
                          // out_act (the raw gradient w.r.t. the stored activation: the input stage's mix operand), and
                          // out_next = bwd_rowscale[row] * c_act * keep(seed, row) * g where the mask word `bits` (READ here) has the element's bit set, else 0 —
                          // cb_trunk_layer_bwd_f32's pass without its read of g
  const float* bwd_rowscale;
  const int32_t* row_ids; // or null.  The CSR's rows are a SUBSET of the node rows (row r = node row_ids[r]; rows-only forward, trunk.py): mix_src, the mask
                          // words and the dropout mask are taken at the node row, out_act / out_next (and row_scale, rowptr) at the compact row
  // MIXB kernels (cb_spmm_csr_store_bwd_mix_f32: bwd, all node rows): the gradients that reach X0 through the residual mixes are FOLDED into one stream —
  //   out_act = mx_c * ( keep(seed, row) * g  +  sum_q keep(mx_seed[q], row) * mx_g[q][mx_pos[q][row]] )        (a row with mx_pos < 0 is absent: zero)
  // instead of the raw g: what the input stage adds to the gradient of dropout(X0) (the compact operands mx_g are the mix gradients of the layers above,
  // each under its own store's dropout mask), so that the input stage reads ONE matrix instead of n + 1 — and cs_partial ([blocks][d]) receives the
  // column sums of out_next / bwd_rowscale per block: the bias gradient of the store whose backward this epilogue applies
  int mx_n;
  const float* mx_g[2];
  const int* mx_pos[2];
  uint64_t mx_seed[2];
  float mx_c;
  float* cs_partial;
  int cs_block0;          // (hub-finish launch: its blocks' partial rows follow the row kernel's)
};

// The MIXB form of fused_store's bwd branch (see FusedEpi).  xm[q] / xp[q]: operand q's row of this node row and its position (< 0: absent), fetched one
// row ahead by the caller; cs: the wavefront's running column sums of c_act * keep * g under the mask word.
__device__ __forceinline__ void fused_store_bwd_mix(const FusedEpi& fe, int64_t row, int c0, const float (&acc)[4], float scale, float (&x)[4],
                                                    const float (&xm)[2][4], const int (&xp)[2], float (&cs)[4]) {
  const TrunkStore& st = fe.st;
  const uint64_t sd = st.seed_dev ? *st.seed_dev : 0ull;
  const int64_t quad = ((st.row0 + row) * fe.d + c0) >> 2;
  float m[4] = {1.f, 1.f, 1.f, 1.f}, mm[4] = {0.f, 0.f, 0.f, 0.f};
  if (st.thresh) keep4(st.seed + sd, quad, st.thresh, st.keep_scale, m);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (q < fe.mx_n && xp[q] >= 0) {      // (wave-uniform)
      float mq[4] = {1.f, 1.f, 1.f, 1.f};
      if (st.thresh) keep4(fe.mx_seed[q] + sd, quad, st.thresh, st.keep_scale, mq);
#pragma unroll
      for (int i = 0; i < 4; ++i) mm[i] += fe.mx_c * (xm[q][i] * mq[i]);
    }
  }
  const unsigned long long* bw = st.bits + (row * (fe.d >> 8) + (c0 >> 8)) * 4;
  const float rs = fe.bwd_rowscale ? fe.bwd_rowscale[row] : 1.f;
  const int lane = lane_id();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float gm = scale_add(acc[i], scale, 0.f) * m[i];
    mm[i] += fe.mx_c * gm;
    const float t = ((bw[i] >> lane) & 1ull) ? st.c_act * gm : 0.f;
    cs[i] += t;
    x[i] = t * rs;                       // (cb_trunk_layer_bwd_f32's expressions, in its order)
  }
  store_stream<4>(st.out_act + row * st.ld_act + c0, mm);
  store_stream<4>(fe.out_next + row * fe.ld_next + c0, x);
}

// x: the values stored to out_next (also handed to the caller: cb_agg_gemm.hip keeps the finished row on chip)
// grow: the node row of `row` (== row unless fe.row_ids)
__device__ __forceinline__ void fused_store(const FusedEpi& fe, int64_t row, int c0, const float (&acc)[4], float scale,
                                            const float (&b)[4], const float (&rmix)[4], float (&x)[4], int64_t grow) {
  const TrunkStore& st = fe.st;
  float a[4], m[4] = {1.f, 1.f, 1.f, 1.f};
  if (fe.bwd) {
    float g4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) g4[i] = scale_add(acc[i], scale, b[i]);      // (b = 0: what the plain store writes)
    if (st.out_act) store_stream<4>(st.out_act + row * st.ld_act + c0, g4);
    store_keep4(st, grow, fe.d, c0, m);
    const unsigned long long* bw = st.bits + (grow * (fe.d >> 8) + (c0 >> 8)) * 4;
    const float rs = fe.bwd_rowscale ? fe.bwd_rowscale[grow] : 1.f;
    const int lane = lane_id();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float gm = g4[i] * m[i];
      x[i] = ((bw[i] >> lane) & 1ull) ? (st.c_act * gm) * rs : 0.f;      // (cb_trunk_layer_bwd_f32's expressions, in its order)
    }
    store_stream<4>(fe.out_next + row * fe.ld_next + c0, x);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = relu_nan(scale_add(acc[i], scale, b[i]));
  store_keep4(st, grow, fe.d, c0, m);
  if (st.bits) store_mask_words(st, st.bits + (grow * (fe.d >> 8) + (c0 >> 8)) * 4, lane_id(), a, m);
  if (st.out_act) store_stream<4>(st.out_act + row * st.ld_act + c0, a);
  store_value(st, a, rmix, m, x);
  if (!fe.skip_next) store_stream<4>(fe.out_next + row * fe.ld_next + c0, x);
}

template <int VEC>
__device__ __forceinline__ void write_row(float* __restrict__ out_row, const float (&acc)[VEC], float scale,
                                          const float (&b)[VEC], int relu, float (&r)[VEC]) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    const float t = scale_add(acc[i], scale, b[i]);   // rst * norm + bias   (GCN.py:250,253)
    r[i] = relu ? relu_nan(t) : t;
  }
  store_stream<VEC>(out_row, r);
}

// What a wavefront knows about the consecutive rows r0 .. r0 + nr - 1 it walks: lane i holds my_ptr = rowptr[r0 + min(i, nr)] and my_scale =
// row_scale[r0 + i] (1 without row_scale; broadcast at flush time: no load on the flush path), bit i of hubmask marks a row with more than hub_T
// edges (left to the hub kernels).  BLOCK64: the block may have 64 rows (the tile kernels), so rowptr[r0 + nr] has no lane of its own and is kept
// in ptr_hi — the successor of lane 63's pointer, stream_rows' P65.  Blocks of fewer than 64 rows keep their end pointer in lane nr; ptr_hi is 0.
template <bool BLOCK64>
struct RowBlock {
  int my_ptr, ptr_hi;
  float my_scale;
  unsigned long long hubmask;
};

template <bool BLOCK64>
__device__ __forceinline__ RowBlock<BLOCK64> load_row_block(const int* __restrict__ rowptr, const float* __restrict__ row_scale, int hub_T, int r0, int nr) {
  const int lane = lane_id();
  RowBlock<BLOCK64> b;
  b.my_ptr = __builtin_nontemporal_load(rowptr + r0 + min(lane, nr));
  b.ptr_hi = 0;
  if constexpr (BLOCK64) b.ptr_hi = rowptr[r0 + nr];      // (uniform address: scalar load)
  b.my_scale = 1.f;
  if (row_scale && lane < nr) b.my_scale = __builtin_nontemporal_load(row_scale + r0 + lane);
  int nxt = __shfl_down(b.my_ptr, 1);
  if constexpr (BLOCK64) {
    if (lane == kWave - 1) nxt = b.ptr_hi;
  }
  b.hubmask = __ballot(lane < nr && (nxt - b.my_ptr) > hub_T);
  return b;
}

// A 64-row tile cut among NW gathering wavefronts at equal EDGE counts: wavefront w takes the rows [ra, rb) whose first edge falls into its
// share of the tile's edge range (row boundaries from the tile's rowptr values, two ballots), so that the wavefronts finish together.
struct RowCut {
  int ra, rb;
};
template <int NW>
__device__ __forceinline__ RowCut tile_row_cut(const RowBlock<true>& blk, int nrt, int w) {
  const int lane = lane_id();
  const int e0 = bcast_lane(blk.my_ptr, 0), e1 = blk.ptr_hi;
  const int64_t span = (int64_t)e1 - e0;
  const int ta = e0 + (int)(span * w / NW), tb = e0 + (int)(span * (w + 1) / NW);
  RowCut c;
  c.ra = w == 0 ? 0 : (int)__popcll(__ballot(lane < nrt && blk.my_ptr < ta));
  c.rb = w == NW - 1 ? nrt : (int)__popcll(__ballot(lane < nrt && blk.my_ptr < tb));
  return c;
}

// Tile rows [from, to) (past the matrix's last row) as zeros: one wavefront, this lane's 4 columns
template <int TLD>
__device__ __forceinline__ void zero_tile_rows(float* tile_lane, int from, int to) {
  for (int i = from; i < to; ++i) *reinterpret_cast<float4*>(tile_lane + i * TLD) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// One source row under gather policy GP.  wave-uniform `craw` = column id as stored (GP == 2: bit 31 = hot flag)
template <int VEC, typename HT, int GP>
__device__ __forceinline__ void gather_pol(float (&v)[VEC], const HT* __restrict__ h_lane, int64_t ld_h, int craw) {
  if constexpr (GP == 0 || VEC != 4) {
    gather_in<VEC, HT>(v, h_lane + (int64_t)craw * ld_h);
  } else if constexpr (GP == 1) {
    if constexpr (sizeof(HT) == 4) gather_nt4(v, reinterpret_cast<const float*>(h_lane) + (int64_t)craw * ld_h);
    else gather_nt4_bf16(v, h_lane + (int64_t)craw * ld_h);
  } else {
    const HT* p = h_lane + (int64_t)(craw & kColMask) * ld_h;
    if (craw < 0) gather_in<VEC, HT>(v, p);
    else if constexpr (sizeof(HT) == 4) gather_nt4(v, reinterpret_cast<const float*>(p));
    else gather_nt4_bf16(v, p);
  }
}

// Walks the contiguous edge range of local rows [rlo, rhi) of this wavefront's row block (no hub row inside).
// my_ptr_v / my_scale / ptr_hi: the RowBlock's.  All control flow is wave-uniform.
// TLD > 0 (cb_agg_gemm.hip): every finished row is also written to an LDS tile — tile_lane = this lane's 4 columns of the
// wavefront's local row 0, TLD floats per tile row.
// P65 (64-row blocks, cb_agg_gemm.hip): lane i holds rowptr[r0 + i] for i < 64 and ptr_hi = rowptr[r0 + 64].
// TILE_ONLY (cb_sage.hip, TLD > 0): the finished row goes to the LDS tile alone — nothing is written through out_lane (may be null).
template <int VEC, int U, bool FULL, bool FUSED, bool ACC, typename HT, int GP = 0, int TLD = 0, bool P65 = false, bool CS = false, bool MIXB = false,
          bool TILE_ONLY = false, bool EW = false>
__device__ __forceinline__ void stream_rows(int rlo, int rhi, int nr, int my_ptr_v, float my_scale, int r0, const int* __restrict__ col,
                                            const HT* __restrict__ h_lane, int64_t ld_h, float* __restrict__ out_lane,
                                            int64_t ld_out, bool active_in, int relu, const float (&bvec)[VEC], const FusedEpi& fe,
                                            int c0, const float* __restrict__ init_lane, int64_t ld_init, const Epilogue& ep,
                                            float* tile_lane = nullptr, int ptr_hi = 0, int my_gid_v = 0, int my_xp0 = 0, int my_xp1 = 0,
                                            float* cs_acc = nullptr) {
  // my_gid_v (FUSED with fe.row_ids): lane i holds the node row of local row i
  // MIXB (FusedEpi): my_xp0 / my_xp1: lane i holds the position of local row i in the compact operands; cs_acc: the wavefront's 4 running column sums
  static_assert(!MIXB || (FUSED && VEC == 4 && FULL && !ACC && TLD == 0 && !P65), "folded mix gradients: the fused d % 256 == 0 kernel on all node rows");
  static_assert(TLD == 0 || (VEC == 4 && FULL), "on-chip row tile: d == 256, float4 lanes");
  static_assert(!TILE_ONLY || (TLD > 0 && !FUSED && !ACC), "tile-only rows: the plain aggregation into an on-chip tile");
  static_assert(!CS || (!FUSED && !ACC && sizeof(HT) == 4), "source-row factor: plain fp32 aggregation only");
  static_assert(!EW || (!CS && !FUSED && !ACC && sizeof(HT) == 4), "per-edge factor: plain fp32 aggregation only, no source-row factor beside it");
  struct PtrAt {      // rowptr of local row i (wave-uniform i)
    int v, hi;
    __device__ __forceinline__ int operator()(int i) const {
      if constexpr (P65) return i >= kWave ? hi : bcast_lane(v, i);
      else return bcast_lane(v, i);
    }
  };
  const PtrAt my_ptr_at{my_ptr_v, ptr_hi};
  const bool active = FULL ? true : active_in;
  float ainit[VEC];                          // ACC: partial sums of local row `cur`, fetched one row ahead (read once: streaming)
  zero<VEC>(ainit);
  const bool skip_empty = ACC && !FUSED && ep.acc_skip_empty;
  if constexpr (ACC) {
    if (active && !(skip_empty && my_ptr_at(rlo) == my_ptr_at(rlo + 1))) gather_stream<VEC>(ainit, init_lane + (int64_t)(r0 + rlo) * ld_init);
  }
  float rmix[4] = {0.f, 0.f, 0.f, 0.f};   // FUSED: mix_src row of local row `cur`, fetched one row ahead
  auto gid_of = [&](int i) -> int64_t { return fe.row_ids ? (int64_t)bcast_lane(my_gid_v, i) : (int64_t)(r0 + i); };
  if constexpr (FUSED) {
    if (fe.st.mix_src) {
      float t[VEC];
      gather_stream<VEC>(t, fe.st.mix_src + gid_of(rlo) * fe.st.ld_mix + c0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) rmix[i] = t[i];
    }
  }
  float xm[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};      // MIXB: the compact operands' rows of local row `cur`, fetched one row ahead
  int xp[2] = {-1, -1};
  auto fetch_mix = [&](int i) {
    if constexpr (MIXB) {
      xp[0] = fe.mx_n > 0 ? bcast_lane(my_xp0, i) : -1;
      xp[1] = fe.mx_n > 1 ? bcast_lane(my_xp1, i) : -1;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (xp[q] >= 0) gather_stream<4>(xm[q], fe.mx_g[q] + (int64_t)xp[q] * fe.d + c0);
    }
  };
  if constexpr (MIXB) fetch_mix(rlo);
  const int lane = lane_id();
  const int e_begin = my_ptr_at(rlo);
  const int e_end = my_ptr_at(rhi);
  int cur = rlo;
  int cur_end = my_ptr_at(rlo + 1);
  float acc[VEC];
  zero<VEC>(acc);

  int cur_begin = e_begin;                   // first edge of local row `cur`
  auto flush = [&]() {
    const float s = __int_as_float(bcast_lane(__float_as_int(my_scale), cur));  // row scale of local row `cur`
    if constexpr (ACC) {
      const int nxt_end = my_ptr_at(cur + 2);      // (clamped beyond the block's last row: lanes past nr hold the block's end pointer)
      const bool fetch_next = active && cur + 1 < rhi && !(skip_empty && cur_end == nxt_end);
      if (skip_empty && cur_begin == cur_end) {      // raw in-place pass, row without edges here: its running sums stay untouched
        if (fetch_next) gather_stream<VEC>(ainit, init_lane + (int64_t)(r0 + cur + 1) * ld_init);
        ++cur;
        cur_begin = cur_end;
        cur_end = nxt_end;
        return;
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += ainit[i];
      if (fetch_next) gather_stream<VEC>(ainit, init_lane + (int64_t)(r0 + cur + 1) * ld_init);
    }
    if constexpr (FUSED) {
      float a4[4], b4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a4[i] = acc[i % VEC]; b4[i] = bvec[i % VEC]; }
      float x4[4];
      if constexpr (MIXB) {
        float (&csr)[4] = *reinterpret_cast<float (*)[4]>(cs_acc);
        fused_store_bwd_mix(fe, (int64_t)(r0 + cur), c0, a4, s, x4, xm, xp, csr);
        if (cur + 1 < rhi) fetch_mix(cur + 1);
      } else {
        fused_store(fe, (int64_t)(r0 + cur), c0, a4, s, b4, rmix, x4, gid_of(cur));
      }
      if constexpr (TLD > 0) *reinterpret_cast<float4*>(tile_lane + cur * TLD) = make_float4(x4[0], x4[1], x4[2], x4[3]);
      if (fe.st.mix_src && cur + 1 < nr) {
        float t[VEC];
        gather_stream<VEC>(t, fe.st.mix_src + gid_of(cur + 1) * fe.st.ld_mix + c0);
#pragma unroll
        for (int i = 0; i < VEC; ++i) rmix[i] = t[i];
      }
    } else if (active) {
      bool lp_done = false;
      if constexpr (VEC < 4 && !ACC && TLD == 0) {
        if (ep.lp_mix) {
          bool on[VEC];
#pragma unroll
          for (int i = 0; i < VEC; ++i) on[i] = true;
          write_row_lp<VEC>(out_lane + (int64_t)(r0 + cur) * ld_out, acc, s, ep, (int64_t)(r0 + cur), c0, on);
          lp_done = true;
        }
      }
      if (!lp_done) {
        float rv[VEC];
        if constexpr (TILE_ONLY) {      // write_row's value, not stored
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const float t = scale_add(acc[i], s, bvec[i]);
            rv[i] = relu ? relu_nan(t) : t;
          }
        } else {
          write_row<VEC>(out_lane + (int64_t)(r0 + cur) * ld_out, acc, s, bvec, relu, rv);
        }
        if constexpr (TLD > 0) *reinterpret_cast<float4*>(tile_lane + cur * TLD) = make_float4(rv[0], rv[1], rv[2], rv[3]);
      }
    }
    zero<VEC>(acc);
    ++cur;
    cur_begin = cur_end;
    cur_end = my_ptr_at(cur + 1);
  };

  // P65 kernels run ONE wavefront per SIMD (cb_agg_gemm.hip): no neighbour hides a dependent load, so the next window's column ids are
  // requested before this window's gathers and the remainder of a window goes out as one predicated batch instead of one load at a time
  int col_next = 0;
  float ew_next = 0.f;                         // EW: the factors of the next window's edges, requested with their column ids
  if constexpr (P65) {
    if (e_begin + lane < e_end) {
      col_next = __builtin_nontemporal_load(col + e_begin + lane);
      if constexpr (EW) ew_next = __builtin_nontemporal_load(ep.edge_w + e_begin + lane);
    }
  }
  for (int base = e_begin; base < e_end; base += kWave) {
    const int cnt = min(kWave, e_end - base);
    int my_col = 0;
    if constexpr (P65) {
      my_col = col_next;
      if (base + kWave + lane < e_end) col_next = __builtin_nontemporal_load(col + base + kWave + lane);
    } else {
      if (lane < cnt) my_col = __builtin_nontemporal_load(col + base + lane);
    }
    float my_cs = 0.f;                         // CS: lane i holds the factor of the window's i-th source row; EW: of the window's i-th edge
    if constexpr (CS) {
      if (lane < cnt) my_cs = ep.col_scale[my_col & kColMask];
    }
    if constexpr (EW) {
      if constexpr (P65) {
        my_cs = ew_next;
        if (base + kWave + lane < e_end) ew_next = __builtin_nontemporal_load(ep.edge_w + base + kWave + lane);
      } else {
        if (lane < cnt) my_cs = __builtin_nontemporal_load(ep.edge_w + base + lane);
      }
    }
    int k = 0;
    for (; k + U <= cnt; k += U) {
      float v[U][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = bcast_lane(my_col, k + u);
        if (active) gather_pol<VEC, HT, GP>(v[u], h_lane, ld_h, c);
        else zero<VEC>(v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = base + k + u;
        while (e == cur_end) flush();
        if constexpr (CS || EW) {
          const float cs = __int_as_float(bcast_lane(__float_as_int(my_cs), k + u));
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += cs * v[u][i];
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += v[u][i];
        }
      }
    }
    if constexpr (P65) {
      if (k < cnt) {
        const int nb = cnt - k;      // 1 .. U-1 edges left in this window
        float v[U][VEC];
#pragma unroll
        for (int u = 0; u < U - 1; ++u) {
          if (u < nb) gather_pol<VEC, HT, GP>(v[u], h_lane, ld_h, bcast_lane(my_col, k + u));
        }
#pragma unroll
        for (int u = 0; u < U - 1; ++u) {
          if (u < nb) {
            const int e = base + k + u;
            while (e == cur_end) flush();
            if constexpr (CS || EW) {
              const float cs = __int_as_float(bcast_lane(__float_as_int(my_cs), k + u));
#pragma unroll
              for (int i = 0; i < VEC; ++i) acc[i] += cs * v[u][i];
            } else {
#pragma unroll
              for (int i = 0; i < VEC; ++i) acc[i] += v[u][i];
            }
          }
        }
        k = cnt;
      }
    }
    for (; k < cnt; ++k) {
      const int c = bcast_lane(my_col, k);
      float v[VEC];
      if (active) gather_pol<VEC, HT, GP>(v, h_lane, ld_h, c);
      else zero<VEC>(v);
      const int e = base + k;
      while (e == cur_end) flush();
      if constexpr (CS || EW) {
        const float cs = __int_as_float(bcast_lane(__float_as_int(my_cs), k));
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += cs * v[i];
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += v[i];
      }
    }
  }
  while (cur < rhi) flush();  // last row + trailing empty rows
}

// The wavefronts' running column sums (MIXB: FusedEpi::cs_partial) -> one partial row per block: fixed order, no atomics.  All threads of the block call it.
__device__ __forceinline__ void block_colsum_store(const float (&cs)[4], float* __restrict__ partial_row, int c0, bool live) {
  __shared__ float s_cs[4][256 + 4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < 4; ++i) s_cs[w][lane * 4 + i] = live ? cs[i] : 0.f;
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      partial_row[c0 + i] = ((s_cs[0][lane * 4 + i] + s_cs[1][lane * 4 + i]) + s_cs[2][lane * 4 + i]) + s_cs[3][lane * 4 + i];
  }
}

template <int VEC, int RPW, int U, bool FULL, bool FUSED, typename HT, bool ACC = false, int GP = 0, bool CS = false, bool MIXB = false,
          bool EW = false>
__global__ void __launch_bounds__(256) k_spmm_rows(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                   const HT* __restrict__ h, int64_t ld_h, float* __restrict__ out,
                                                   int64_t ld_out, int n_rows, int d, Epilogue ep, int hub_T, FusedEpi fe) {
  static_assert(!FUSED || (VEC == 4 && FULL), "fused epilogue: d % 256 == 0, float4 lanes");
  static_assert(RPW < kWave, "row block must fit the lanes of one wavefront (+1 end pointer)");
  const int lane = lane_id();
  const int wave = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int r0 = wave * RPW;
  float cs_acc[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (MIXB) {      // (no early exit: every wavefront of the block takes part in the column sums' hand-over)
    if (r0 >= n_rows) {
      if (fe.cs_partial) block_colsum_store(cs_acc, fe.cs_partial + (int64_t)(fe.cs_block0 + blockIdx.x) * d + blockIdx.y * 256, lane * 4, false);
      return;
    }
  } else {
    if (r0 >= n_rows) return;
  }
  const int nr = min(RPW, n_rows - r0);
  const int c0 = (blockIdx.y * kWave + lane) * VEC;  // this lane's first column
  const bool active = c0 < d;

  int my_ptr = __builtin_nontemporal_load(rowptr + r0 + min(lane, nr));      // (load_row_block<false>, written out: as a call it moves the fused kernels' schedules)
  float my_scale = 1.f;  // lane i: row_scale[r0 + i], broadcast at flush time (no load on the flush path)
  if (ep.row_scale && lane < nr) my_scale = __builtin_nontemporal_load(ep.row_scale + r0 + lane);
  const int nxt = __shfl_down(my_ptr, 1);
  const unsigned long long hubmask = __ballot(lane < nr && (nxt - my_ptr) > hub_T);
  int my_gid = 0;
  if constexpr (FUSED) {
    if (fe.row_ids && lane < nr) my_gid = fe.row_ids[r0 + lane];
  }
  int my_xp0 = -1, my_xp1 = -1;      // MIXB: lane i holds the position of local row i in the compact operands
  if constexpr (MIXB) {
    if (fe.mx_n > 0 && lane < nr) my_xp0 = __builtin_nontemporal_load(fe.mx_pos[0] + r0 + lane);
    if (fe.mx_n > 1 && lane < nr) my_xp1 = __builtin_nontemporal_load(fe.mx_pos[1] + r0 + lane);
  }

  float bvec[VEC];
  zero<VEC>(bvec);
  if (ep.bias && active) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) bvec[i] = ep.bias[c0 + i];
  }
  const HT* h_lane = h + c0;
  float* out_lane = out + c0;
  const float* init_lane = ACC ? ep.acc_init + c0 : nullptr;

  if (hubmask == 0) {
    stream_rows<VEC, U, FULL, FUSED, ACC, HT, GP, 0, false, CS, MIXB, false, EW>(0, nr, nr, my_ptr, my_scale, r0, col, h_lane, ld_h, out_lane, ld_out, active, ep.relu, bvec, fe, c0,
                                                    init_lane, ep.ld_init, ep, nullptr, 0, my_gid, my_xp0, my_xp1, cs_acc);
  } else {
    int r = 0;
    while (r < nr) {  // maximal hub-free runs; hub rows are written by the hub kernels
      unsigned long long m = hubmask >> r;
      int nh = m ? r + (__ffsll((long long)m) - 1) : nr;
      if (nh > r)
        stream_rows<VEC, U, FULL, FUSED, ACC, HT, GP, 0, false, CS, MIXB, false, EW>(r, nh, nr, my_ptr, my_scale, r0, col, h_lane, ld_h, out_lane, ld_out, active, ep.relu, bvec, fe,
                                                        c0, init_lane, ep.ld_init, ep, nullptr, 0, my_gid, my_xp0, my_xp1, cs_acc);
      r = nh + 1;
    }
  }
  if constexpr (MIXB) {
    if (fe.cs_partial) block_colsum_store(cs_acc, fe.cs_partial + (int64_t)(fe.cs_block0 + blockIdx.x) * d + blockIdx.y * 256, lane * 4, true);
  }
}

// One wavefront per chunk of T edges of a hub row -> one partial row in `partial`.
template <int VEC, int U, typename HT, int GP = 0, bool CS = false, bool EW = false>
__global__ void __launch_bounds__(256) k_spmm_hub_chunks(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const HT* __restrict__ h, int64_t ld_h, int d, int hub_T,
                                                         int n_hubs, int n_chunks, const int* __restrict__ hub_rows,
                                                         const int* __restrict__ hub_chunk_ptr, float* __restrict__ partial,
                                                         int64_t ld_p, Epilogue ep) {
  static_assert(!EW || (!CS && sizeof(HT) == 4), "per-edge factor: fp32 rows, no source-row factor beside it");
  const int lane = lane_id();
  const int chunk = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (chunk >= n_chunks) return;
  const int c0 = (blockIdx.y * kWave + lane) * VEC;
  const bool active = c0 < d;
  // hub index: last i with hub_chunk_ptr[i] <= chunk (wave-uniform binary search)
  int lo = 0, hi = n_hubs;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (hub_chunk_ptr[mid] <= chunk) lo = mid; else hi = mid;
  }
  const int row = hub_rows[lo];
  const int j = chunk - hub_chunk_ptr[lo];
  const int e_begin = rowptr[row] + j * hub_T;
  const int e_end = min(e_begin + hub_T, rowptr[row + 1]);
  const HT* h_lane = h + c0;
  float acc[VEC];
  zero<VEC>(acc);
  for (int base = e_begin; base < e_end; base += kWave) {
    const int cnt = min(kWave, e_end - base);
    int my_col = 0;
    if (lane < cnt) my_col = __builtin_nontemporal_load(col + base + lane);
    float my_cs = 0.f;
    if constexpr (CS) {
      if (lane < cnt) my_cs = ep.col_scale[my_col & kColMask];
    }
    if constexpr (EW) {      // (base is an absolute edge index, rowptr[row] + j * hub_T + a multiple of 64: the index col is read at)
      if (lane < cnt) my_cs = __builtin_nontemporal_load(ep.edge_w + base + lane);
    }
    int k = 0;
    for (; k + U <= cnt; k += U) {
      float v[U][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = bcast_lane(my_col, k + u);
        if (active) gather_pol<VEC, HT, GP>(v[u], h_lane, ld_h, c);
        else zero<VEC>(v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (CS || EW) {
          const float cs = __int_as_float(bcast_lane(__float_as_int(my_cs), k + u));
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += cs * v[u][i];
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += v[u][i];
        }
      }
    }
    for (; k < cnt; ++k) {
      const int c = bcast_lane(my_col, k);
      float v[VEC];
      if (active) gather_pol<VEC, HT, GP>(v, h_lane, ld_h, c);
      else zero<VEC>(v);
      if constexpr (CS || EW) {
        const float cs = __int_as_float(bcast_lane(__float_as_int(my_cs), k));
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += cs * v[i];
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += v[i];
      }
    }
  }
  if (active) {
    float* p = partial + (int64_t)chunk * ld_p + c0;
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = acc[i];
  }
}

// One wavefront per hub row: partials summed in chunk order, then the epilogue.
template <int VEC, bool FUSED, bool MIXB = false>
__global__ void __launch_bounds__(256) k_spmm_hub_finish(int d, int n_hubs, const int* __restrict__ hub_rows,
                                                         const int* __restrict__ hub_chunk_ptr,
                                                         const float* __restrict__ partial, int64_t ld_p,
                                                         float* __restrict__ out, int64_t ld_out, Epilogue ep, FusedEpi fe) {
  const int lane = lane_id();
  const int i = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  float cs_acc[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (MIXB) {      // (d % 256 == 0: every lane has columns; every wavefront of the block hands its column sums over)
    if (i >= n_hubs) {
      if (fe.cs_partial) block_colsum_store(cs_acc, fe.cs_partial + (int64_t)(fe.cs_block0 + blockIdx.x) * d + blockIdx.y * 256, lane * 4, false);
      return;
    }
  } else {
    if (i >= n_hubs) return;
  }
  const int c0 = (blockIdx.y * kWave + lane) * VEC;
  if (c0 >= d) return;
  const int row = hub_rows[i];
  float acc[VEC];
  zero<VEC>(acc);
  for (int c = hub_chunk_ptr[i]; c < hub_chunk_ptr[i + 1]; ++c) {
    float v[VEC];
    gather<VEC>(v, partial + (int64_t)c * ld_p + c0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] += v[k];
  }
  if (ep.acc_init) {   // node-sharded path: partial sums of the interior-column pass
    float v[VEC];
    gather<VEC>(v, ep.acc_init + (int64_t)row * ep.ld_init + c0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] += v[k];
  }
  float bvec[VEC];
  zero<VEC>(bvec);
  if (ep.bias) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) bvec[k] = ep.bias[c0 + k];
  }
  const float s = ep.row_scale ? ep.row_scale[row] : 1.f;
  if constexpr (FUSED) {
    float a4[4], b4[4], rmix[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) { a4[k] = acc[k % VEC]; b4[k] = bvec[k % VEC]; }
    const int64_t grow = fe.row_ids ? (int64_t)fe.row_ids[row] : (int64_t)row;
    if (fe.st.mix_src) {
      float t[VEC];
      gather_stream<VEC>(t, fe.st.mix_src + grow * fe.st.ld_mix + c0);
#pragma unroll
      for (int k = 0; k < VEC; ++k) rmix[k] = t[k];
    }
    float x4[4];
    if constexpr (MIXB) {
      float xm[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      int xp[2] = {-1, -1};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q < fe.mx_n) xp[q] = fe.mx_pos[q][row];
        if (xp[q] >= 0) gather_stream<4>(xm[q], fe.mx_g[q] + (int64_t)xp[q] * fe.d + c0);
      }
      fused_store_bwd_mix(fe, (int64_t)row, c0, a4, s, x4, xm, xp, cs_acc);
      if (fe.cs_partial) block_colsum_store(cs_acc, fe.cs_partial + (int64_t)(fe.cs_block0 + blockIdx.x) * d + blockIdx.y * 256, lane * 4, true);
    } else {
      fused_store(fe, (int64_t)row, c0, a4, s, b4, rmix, x4, grow);
    }
  } else {
    {
      if (ep.lp_mix) {      // label-propagation store (narrow rows only ever set it)
        bool on[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) on[k] = true;
        write_row_lp<VEC>(out + (int64_t)row * ld_out + c0, acc, s, ep, (int64_t)row, c0, on);
        return;
      }
    }
    float rv[VEC];
    write_row<VEC>(out + (int64_t)row * ld_out + c0, acc, s, bvec, ep.relu, rv);
  }
}

// The graph side of every aggregation entry (include/coldbrew_hip.h, cb_csr_view), checked once for a call on rows of d elements: sizes, the
// int32 index contract, null pointers, the hub plan and the workspace for its partial sums.  v = the view the launches take: a copy with
// hub_threshold = INT32_MAX when there are no hub rows (no plan given: every row is reduced whole by one wavefront).  An empty call
// (n_rows == 0 or d == 0) passes without a look at the pointers: the entry returns before it launches anything.
static inline int check_csr_view(const char* who, const cb_csr_view* g, int64_t d, cb_csr_view& v) {
  CB_CHECK_ARG(g != nullptr, CB_E_INVALID, "%s: the graph view is null", who);
  v = *g;
  CB_CHECK_ARG(v.n_rows >= 0 && v.n_edges >= 0 && d >= 0, CB_E_INVALID, "%s: negative size", who);
  CB_CHECK_ARG(v.n_rows < INT32_MAX && v.n_edges < INT32_MAX && d < (1 << 20), CB_E_RANGE, "%s: size exceeds the int32 contract", who);
  if (v.n_rows == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(v.rowptr && (v.n_edges == 0 || v.col), CB_E_INVALID, "%s: null pointer in the graph view", who);
  CB_CHECK_ARG(v.hub_threshold > 0 && v.n_hubs >= 0 && v.n_chunks >= 0, CB_E_INVALID, "%s: bad hub plan", who);
  const size_t need = cb_spmm_workspace_bytes(v.n_chunks, d);
  CB_CHECK_ARG(v.n_hubs == 0 || (v.hub_rows && v.hub_chunk_ptr && v.ws && v.ws_bytes >= need), CB_E_WORKSPACE,
               "%s: hub plan given but workspace missing/too small (%zu < %zu)", who, v.ws_bytes, need);
  if (v.n_hubs == 0) v.hub_threshold = INT32_MAX;
  return CB_OK;
}

// row pitch of the hub partial sums in a view's workspace (cb_spmm_workspace_bytes)
static inline int64_t partial_ld(int64_t d) { return (d + 3) / 4 * 4; }

// A run-time flag as a compile-time constant: f(std::true_type / std::false_type)
template <class F>
static inline void dispatch_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// The run-time pair (gather policy 0 / 2, source-row factor or not) as compile-time constants: f(std::integral_constant<int, GP>, std::bool_constant<CS>).
// GP2 / CSF: whether the caller's kernels are compiled for gp == 2 / for a source-row factor at all — what is not compiled is not instantiated
// here either (the narrow-row kernels have neither, the fused and bf16 ones no factor), and the caller never asks for it.
template <bool GP2, bool CSF, class F>
static inline void dispatch_gp_cs(int gp, bool cs, F&& f) {
  auto with_gp = [&](auto CS) {
    if constexpr (GP2) {
      if (gp == 2) return f(std::integral_constant<int, 2>{}, CS);
    }
    f(std::integral_constant<int, 0>{}, CS);
  };
  if constexpr (CSF) {
    if (cs) return with_gp(std::true_type{});
  }
  with_gp(std::false_type{});
}

// The hub rows of a view: one wavefront per chunk of hub_threshold edges -> a partial row in the view's workspace, then one wavefront per hub row sums
// its partials in chunk order and applies the epilogue (k_spmm_hub_chunks, k_spmm_hub_finish).  ep.col_flags chooses the gather policy (float4 lanes);
// ep.col_scale the source-row factor (float4 lanes, fp32 rows, plain epilogue: a fused epilogue never takes one).  EW: ep.edge_w, the per-edge factor.
template <int VEC, typename HT, bool FUSED, bool MIXB = false, bool EW = false>
static int launch_hub_rows(const cb_csr_view& g, const HT* h, int64_t ld_h, int64_t d, float* out, int64_t ld_out, const Epilogue& ep, const FusedEpi& fe,
                           hipStream_t st) {
  if (g.n_hubs <= 0) return CB_OK;
  const int wpb = 4, ny = (int)((d + kWave * VEC - 1) / (kWave * VEC));
  const int64_t ld_p = partial_ld(d);
  float* partial = (float*)g.ws;
  const dim3 blk(kWave * wpb), gridc((unsigned)((g.n_chunks + wpb - 1) / wpb), ny), gridf((unsigned)((g.n_hubs + wpb - 1) / wpb), ny);
  static_assert(!EW || (VEC == 4 && !FUSED && sizeof(HT) == 4), "per-edge factor: the d % 256 == 0 fp32 kernels with the plain epilogue");
  dispatch_gp_cs<VEC == 4, VEC == 4 && !FUSED && !EW && sizeof(HT) == 4>(ep.col_flags ? 2 : 0, !EW && ep.col_scale != nullptr, [&](auto GP, auto CS) {
    hipLaunchKernelGGL((k_spmm_hub_chunks<VEC, 8, HT, decltype(GP)::value, decltype(CS)::value, EW>), gridc, blk, 0, st, g.rowptr, g.col, h, ld_h, (int)d,
                       g.hub_threshold, g.n_hubs, g.n_chunks, g.hub_rows, g.hub_chunk_ptr, partial, ld_p, ep);
  });
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_spmm_hub_finish<VEC, FUSED, MIXB>), gridf, blk, 0, st, (int)d, g.n_hubs, g.hub_rows, g.hub_chunk_ptr, partial, ld_p, out, ld_out, ep, fe);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb
