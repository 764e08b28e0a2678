// Backward of the residual trunk's fused stores and of its input stage, and the store itself on a row subset (trunk.py).  Wave-per-row passes over
// [rows, d], d % 256 == 0 (cb_rowpass.h); column sums in the fixed two-stage order.
#include "cb_philox.h"
#include "cb_reduce.h"
#include "cb_rowpass.h"
#include "cb_trunk_store.h"

namespace cb {

static_assert(kBlock / kWave == kRowWaves, "the wave-per-row kernels run four wavefronts per block");

// ---------------------------------------------------------------------------------------------
// Backward of the fused aggregation epilogue of the residual trunk, one pass over [rows, d], d % 256 == 0:
//   gm = g * keep(seed, row0 + r, c) / (1 - p)            dropout backward (thresh == 0: gm = g)
//   gx0 = (accumulate ? gx0 : 0) + c_mix * gm             gradient flowing to the mixed-in tensor (X0)
//   gy  = c_act * gm * relu_bit(r, c)                      mix + ReLU backward (mask bits written by the forward)
//   colsum(gy) -> dbias partials;  out = gy * row_scale[r] (input of the reverse-graph aggregation)
// One wavefront per row per iteration, lane l owns columns 4l..4l+3 of each 256-wide tile (cb_rowpass.h).
// MODE 0: the layer kernel above.  MODE 1: trunk input stage  gy = (add + gm) * (act > 0); out = gy; colsum(gy).
template <int MODE, bool OUT_BF16, bool STORE = true, bool RIDX = false>      // STORE = false: column sums only (no output row is written); RIDX: compact rows (ridx)
__global__ void __launch_bounds__(kBlock) k_trunk_bwd(const float* __restrict__ g, const unsigned long long* __restrict__ bits,
                                                      const float* __restrict__ act, const float* __restrict__ row_scale,
                                                      void* __restrict__ outv, float* __restrict__ gx0, int accumulate,
                                                      int64_t rows, int d, uint32_t thresh, float keep_scale, uint64_t seed,
                                                      const uint64_t* __restrict__ seed_dev, int64_t row0, float c_act, float c_mix,
                                                      float* __restrict__ partial, const int64_t* __restrict__ ridx,
                                                      const float* __restrict__ g2, uint64_t seed2, float c2, const int* __restrict__ g2_pos) {
  // g2 (MODE 0; may be null): the 'Residual' connection (res_tricks.py:7-14) — this layer's ReLU output A_l is also the mix source
  // of layer l+1, so dL/dA_l = c_act * dropout_bwd_seed(g) + c2 * dropout_bwd_seed2(g2), g2 = the gradient w.r.t. layer l+1's stored (dropped)
  // output; `bits` must then be the ReLU mask alone (bits_relu_only of the forward store).  g2_pos (may be null): g2 is a compact operand over the rows
  // of the FULL matrix (a row-sparse backward: g2 lives on the previous level's support); with ridx it is required
  // ridx (MODE 0, gx0 == NULL): g / out hold only the rows ridx[0 .. rows) of the matrix (the loss rows of a row-sparse backward); mask words,
  // row scale and the dropout mask are those of row ridx[r]
  extern __shared__ float s_red[];  // [4 waves][256 cols] per tile pass
  if (seed_dev) { seed += *seed_dev; seed2 += *seed_dev; }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tiles = d >> 8;
  const RowSlab slab = row_slab(rows);
  for (int tile = 0; tile < tiles; ++tile) {
    const int c = tile * 256 + lane * 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t rr_next = 0;      // RIDX: the index of the NEXT row is requested one iteration ahead (mask words and row scale hang on it)
    if constexpr (RIDX) {
      if (slab.begin + w < slab.end) rr_next = ridx[slab.begin + w];
    }
    // g is read once (streaming); the NEXT row's 1 KiB is requested before this row is worked on: at full occupancy (8 wavefronts per SIMD) one
    // row in flight per wavefront keeps only 32 KB per CU outstanding — 4 TB/s at the ~2 us these loads take; two rows double that
    float gn[4] = {0.f, 0.f, 0.f, 0.f};
    if (slab.begin + w < slab.end) load_quad_nt(g + (slab.begin + w) * d + c, gn);
    for (int64_t r = slab.begin + w; r < slab.end; r += kRowWaves) {
      const int64_t off = r * d + c;
      int64_t rr = r;      // the row of the full matrix this row is
      if constexpr (RIDX) {
        rr = rr_next;
        if (r + kRowWaves < slab.end) rr_next = ridx[r + kRowWaves];
      }
      float gm[4] = {gn[0], gn[1], gn[2], gn[3]};
      // (this row's mask words and scale are requested BEFORE the next row's gradient: loads return in order, so waiting for them must not
      // mean waiting for the prefetch)
      unsigned long long bwr[4] = {0ull, 0ull, 0ull, 0ull};
      float sc_r = 1.f;
      if (MODE == 0) {
        const unsigned long long* bwp = mask_words(bits, rr, tiles, tile);
#pragma unroll
        for (int k = 0; k < 4; ++k) bwr[k] = bwp[k];
        sc_r = row_scale ? row_scale[rr] : 1.f;
      }
      if (r + kRowWaves < slab.end) load_quad_nt(g + off + (int64_t)kRowWaves * d, gn);
      if (thresh) {
        float m[4];
        keep4(seed, ((row0 + rr) * d + c) >> 2, thresh, keep_scale, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) gm[k] *= m[k];
      }
      float gy[4];
      if (MODE == 0) {
        if (gx0) {
          float4 a = accumulate ? *reinterpret_cast<const float4*>(gx0 + off) : make_float4(0.f, 0.f, 0.f, 0.f);
          a.x += c_mix * gm[0]; a.y += c_mix * gm[1]; a.z += c_mix * gm[2]; a.w += c_mix * gm[3];
          *reinterpret_cast<float4*>(gx0 + off) = a;
        }
        const unsigned long long* bw = bwr;
        if (g2) {      // (uniform) second gradient through the same ReLU, under the next layer's dropout mask
          const int p2 = operand_row(g2_pos, rr);
          float g2m[4];
          load_operand_quad(g2, g2_pos, p2, off, d, c, g2m);
          zero_absent(p2, g2m);
          if (thresh) {
            float m2[4];
            keep4(seed2, ((row0 + rr) * d + c) >> 2, thresh, keep_scale, m2);
#pragma unroll
            for (int k = 0; k < 4; ++k) g2m[k] *= m2[k];
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) gy[k] = word_bit(bw[k], lane) ? c_act * gm[k] + c2 * g2m[k] : 0.f;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) gy[k] = word_bit(bw[k], lane) ? c_act * gm[k] : 0.f;
        }
      } else {
        const float4 a = *reinterpret_cast<const float4*>(gx0 + off);
        const float4 x = *reinterpret_cast<const float4*>(act + off);
        gy[0] = x.x > 0.f ? a.x + gm[0] : 0.f;
        gy[1] = x.y > 0.f ? a.y + gm[1] : 0.f;
        gy[2] = x.z > 0.f ? a.z + gm[2] : 0.f;
        gy[3] = x.w > 0.f ? a.w + gm[3] : 0.f;
      }
      const float sc = MODE == 0 ? sc_r : (row_scale ? row_scale[rr] : 1.f);
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += gy[k];
      if constexpr (!STORE) continue;
      else if constexpr (OUT_BF16)
        *reinterpret_cast<uint2*>((bf16_t*)outv + off) = pack4_bf16(gy[0] * sc, gy[1] * sc, gy[2] * sc, gy[3] * sc);
      else      // written once, gathered by the next kernel: streaming store
        store_quad_nt((float*)outv + off, gy[0] * sc, gy[1] * sc, gy[2] * sc, gy[3] * sc);
    }
    if (partial) block_colsum(s_red, s, partial, d, c, lane, w);
  }
}

// The layer kernel above (MODE 0, all rows, fp32 out) for LAYER 0 of the 'Initial' trunk, which also FOLDS the gradients that reach X0 through the mixes
// (the elementwise form of cb_spmm_csr_store_bwd_mix_f32's epilogue):
//   out_m = c_mix * ( keep(seed) * g  +  sum_q keep(seed_q) * g_q[pos_q[r] | r] )        (pos_q null: a dense operand; pos < 0: the row is absent)
// g is read here anyway; the input stage (cb_gemm_tn_instage_f32) then reads out_m instead of g and every g_q.
struct FoldOps {
  int n;
  const float* g[2];
  const int* pos[2];
  uint64_t seed[2];
  float* out_m;
  SecondColsum cs;      // (optional) which cb_trunk_input_bwd_multi_cs_f32 took while the input stage was a pass
};
__global__ void __launch_bounds__(kBlock) k_trunk_bwd_fold(const float* __restrict__ g, const unsigned long long* __restrict__ bits, const float* __restrict__ row_scale,
                                                           float* __restrict__ out, FoldOps fo, int64_t rows, int d, uint32_t thresh, float keep_scale, uint64_t seed,
                                                           const uint64_t* __restrict__ seed_dev, int64_t row0, float c_act, float c_mix, float* __restrict__ partial) {
  extern __shared__ float s_red[];
  const uint64_t sd = seed_dev ? *seed_dev : 0ull;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tiles = d >> 8;
  const RowSlab slab = row_slab(rows);
  for (int tile = 0; tile < tiles; ++tile) {
    const int c = tile * 256 + lane * 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    float gn[4] = {0.f, 0.f, 0.f, 0.f};
    if (slab.begin + w < slab.end) load_quad_nt(g + (slab.begin + w) * d + c, gn);
    for (int64_t r = slab.begin + w; r < slab.end; r += kRowWaves) {
      const int64_t off = r * d + c;
      float gm[4] = {gn[0], gn[1], gn[2], gn[3]};
      const unsigned long long* bwp = mask_words(bits, r, tiles, tile);
      unsigned long long bw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) bw[k] = bwp[k];
      const float sc = row_scale ? row_scale[r] : 1.f;
      int pq[2] = {-1, -1};      // (wave-uniform) position of row r in operand q (0: dense), or < 0
      float u[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q < fo.n) {
          pq[q] = operand_row(fo.pos[q], r);
          if (pq[q] >= 0) load_operand_quad(fo.g[q], fo.pos[q], pq[q], off, d, c, u[q]);      // (two operands at most: an absent row is not read at all)
        }
      }
      if (r + kRowWaves < slab.end) load_quad_nt(g + off + (int64_t)kRowWaves * d, gn);
      const int64_t quad = ((row0 + r) * d + c) >> 2;
      if (thresh) {
        float m[4];
        keep4(seed + sd, quad, thresh, keep_scale, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) gm[k] *= m[k];
      }
      float mm[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (q < fo.n && pq[q] >= 0) {
          float mq[4] = {1.f, 1.f, 1.f, 1.f};
          if (thresh) keep4(fo.seed[q] + sd, quad, thresh, keep_scale, mq);
          float um[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            um[k] = u[q][k] * mq[k];
            mm[k] += c_mix * um[k];
          }
          if (fo.cs.partial && q == fo.cs.src) second_colsum_add(fo.cs, r, tiles, tile, lane, um, s2);      // (wave-uniform)
        }
      }
      float gy[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mm[k] += c_mix * gm[k];
        gy[k] = word_bit(bw[k], lane) ? c_act * gm[k] : 0.f;
        s[k] += gy[k];
      }
      store_quad_nt(out + off, gy[0] * sc, gy[1] * sc, gy[2] * sc, gy[3] * sc);
      store_quad_nt(fo.out_m + off, mm[0], mm[1], mm[2], mm[3]);
    }
    if (partial) block_colsum(s_red, s, partial, d, c, lane, w);
    if (fo.cs.partial) block_colsum(s_red, s2, fo.cs.partial, d, c, lane, w);
  }
}

// Input stage of the trunk backward with the X0-gradient gathered in ONE pass instead of accumulated layer by layer:
//   gy = ( keep(seed, r, c) * g  +  c_mix * sum_l keep(seed_l, r, c) * g_l ) / (1 - p)  *  (act > 0)
// g = gradient w.r.t. the dropped X0 that feeds layer 0; g_l = gradient w.r.t. the output of layer l's fused store (the mix
// (1-a) relu(Y_l) + a X0 sits under that store's dropout).  Replaces n_mix read-modify-write passes over a [rows, d]
// accumulator (20 B/element each) by n_mix streaming reads (4 B/element each); masks are regenerated, never stored.
constexpr int kMixMax = 7;
struct MixTable {
  const float* g[kMixMax];
  uint64_t seed[kMixMax];
  int n;
  const int* pos[kMixMax];      // null, or [rows]: g[l] is a compact operand (a row-sparse backward's support rows)
  SecondColsum cs[2];           // up to two per launch
};

template <int NMIX>   // number of mixed-in gradients, compile-time so that all row loads are issued before the first Philox round
__global__ void __launch_bounds__(kBlock) k_trunk_input_bwd_multi(const float* __restrict__ g, MixTable mt, const float* __restrict__ act,
                                                                  const unsigned long long* __restrict__ act_bits,
                                                                  float* __restrict__ out, int64_t rows, int d, uint32_t thresh,
                                                                  float keep_scale, uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                                                  int64_t row0, float c_mix, float* __restrict__ partial) {
  extern __shared__ float s_red[];
  const uint64_t sd = seed_dev ? *seed_dev : 0ull;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tiles = d >> 8;
  const RowSlab slab = row_slab(rows);
  for (int tile = 0; tile < tiles; ++tile) {
    const int c = tile * 256 + lane * 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, s2[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int64_t r = slab.begin + w; r < slab.end; r += kRowWaves) {
      const int64_t off = r * d + c;
      const int64_t quad = ((row0 + r) * d + c) >> 2;
      float t[4];
      load_quad_nt(g + off, t);
      float u[NMIX > 0 ? NMIX : 1][4];
      int pl[NMIX > 0 ? NMIX : 1];      // (wave-uniform) position of row r in operand l (0: dense), or < 0
#pragma unroll
      for (int l = 0; l < NMIX; ++l) pl[l] = operand_row(mt.pos[l], r);
#pragma unroll
      for (int l = 0; l < NMIX; ++l) load_operand_quad(mt.g[l], mt.pos[l], pl[l], off, d, c, u[l]);
#pragma unroll
      for (int l = 0; l < NMIX; ++l) zero_absent(pl[l], u[l]);
      if (thresh) {
        float m[4];
        keep4(seed + sd, quad, thresh, keep_scale, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] *= m[k];
      }
#pragma unroll
      for (int l = 0; l < NMIX; ++l) {
        if (thresh && pl[l] >= 0) {      // (an absent row of a compact operand is zero whatever its mask)
          float m[4];
          keep4(mt.seed[l] + sd, quad, thresh, keep_scale, m);
#pragma unroll
          for (int k = 0; k < 4; ++k) u[l][k] *= m[k];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
          if (mt.cs[q].partial && l == mt.cs[q].src) second_colsum_add(mt.cs[q], r, tiles, tile, lane, u[l], s2[q]);      // (wave-uniform)
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] += c_mix * u[l][k];
      }
      float gy[4];
      if (act_bits) {      // mask words of (act > 0) instead of act itself
        const unsigned long long* bw = mask_words(act_bits, r, tiles, tile);
#pragma unroll
        for (int k = 0; k < 4; ++k) gy[k] = word_bit(bw[k], lane) ? t[k] : 0.f;
      } else {
        const float4 x = *reinterpret_cast<const float4*>(act + off);
        gy[0] = x.x > 0.f ? t[0] : 0.f; gy[1] = x.y > 0.f ? t[1] : 0.f; gy[2] = x.z > 0.f ? t[2] : 0.f; gy[3] = x.w > 0.f ? t[3] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] += gy[k];
      store_quad_nt(out + off, gy[0], gy[1], gy[2], gy[3]);      // written once, streamed by the weight-gradient GEMM that follows
    }
    if (partial) block_colsum(s_red, s, partial, d, c, lane, w);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (mt.cs[q].partial) block_colsum(s_red, s2[q], mt.cs[q].partial, d, c, lane, w);
  }
}

// The trunk's fused store (cb_spmm_core.h FusedEpi: ReLU, mask words, mix, dropout) on a SUBSET of the rows, after a dense transform instead of
// inside an aggregation — the rows-only forward of trunk.py (the last layer on the loss rows):
//   act = relu(y[r]);  out[r] = dropout_seed((c_act * act + c_mix * mix_src[mix_index[r]]));  mask words at the GLOBAL row row_index[r].
// y / out: compact [n_rows, d]; relu_bits: the full array; mix_src (may be null): its row mix_index[r] (mix_index null: row_index[r], i.e. the full
// array).  One wavefront per row, lane l = columns 4l .. 4l+3 of each tile.
__global__ void __launch_bounds__(kBlock) k_trunk_store_rows(const float* __restrict__ y, const int64_t* __restrict__ ridx, int64_t n_rows, int d, TrunkStore st,
                                                             float* __restrict__ out) {
  const uint64_t seed = store_seed(st);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tiles = d >> 8;
  for (int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + w; r < n_rows; r += (int64_t)gridDim.x * (kBlock / kWave)) {
    const int64_t rr = ridx[r], mr = store_mix_row(st, r, rr);
    for (int tile = 0; tile < tiles; ++tile) {
      const int c = tile * 256 + lane * 4;
      const float4 y4 = *reinterpret_cast<const float4*>(y + r * d + c);
      const float a[4] = {relu_nan(y4.x), relu_nan(y4.y), relu_nan(y4.z), relu_nan(y4.w)};
      float m[4] = {1.f, 1.f, 1.f, 1.f}, q[4] = {0.f, 0.f, 0.f, 0.f}, x[4];
      store_keep4(st, seed, rr, d, c, m);
      if (st.bits) store_mask_words(st, st.bits + (rr * tiles + tile) * 4, lane, a, m);
      if (st.out_act) *reinterpret_cast<float4*>(st.out_act + r * st.ld_act + c) = make_float4(a[0], a[1], a[2], a[3]);
      if (st.mix_src) {
        const float4 q4 = *reinterpret_cast<const float4*>(st.mix_src + mr * st.ld_mix + c);
        q[0] = q4.x; q[1] = q4.y; q[2] = q4.z; q[3] = q4.w;
      }
      store_value(st, a, q, m, x);
      *reinterpret_cast<float4*>(out + r * d + c) = make_float4(x[0], x[1], x[2], x[3]);
    }
  }
}

}  // namespace cb

using namespace cb;

struct DropParams {
  uint32_t thresh;      // 0: no dropout (the kernels then skip the mask)
  float keep_scale;
};
static inline DropParams drop_params(float p) { return {p > 0.f ? dropout_threshold(p) : 0u, 1.f / (1.f - p)}; }

// The argument check the trunk-backward entries share, in the order they all make it: the width; nothing to do without rows; what the entry itself found
// wrong with its pointers and operands (`bad`, null if nothing); the dropout rate; the column-sum workspace.
static int check_trunk_args(const char* who, int64_t rows, int64_t d, const char* bad, float drop_p, const float* colsum, const void* ws, size_t ws_bytes) {
  CB_CHECK_ARG(rows >= 0 && d > 0 && d % 256 == 0 && d < (1 << 20), CB_E_INVALID, "%s: d must be a multiple of 256", who);
  if (rows == 0) return CB_OK;
  CB_CHECK_ARG(!bad, CB_E_INVALID, "%s: %s", who, bad);
  CB_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, CB_E_INVALID, "%s: dropout p out of range", who);
  CB_CHECK_ARG(!colsum || (ws && ws_bytes >= cb_colsum_workspace_bytes(rows, d)), CB_E_WORKSPACE, "%s: workspace too small", who);
  return CB_OK;
}
static const char* const kBadPointer = "null or misaligned pointer";

static int launch_trunk_bwd(int mode, int out_bf16, const float* g, const uint64_t* bits, const float* act, const float* row_scale,
                            void* out, float* gx0, int accumulate, int64_t rows, int64_t d, float drop_p, uint64_t seed,
                            const uint64_t* seed_dev, int64_t row0, float c_act, float c_mix, float* colsum, void* ws, hipStream_t st,
                            const int64_t* ridx = nullptr, const float* g2 = nullptr, uint64_t seed2 = 0, float c2 = 0.f,
                            const int32_t* g2_pos = nullptr) {
  const int nb = colsum_blocks(rows);
  const DropParams dp = drop_params(drop_p);
  float* partial = colsum ? (float*)ws : nullptr;
#define CB_TB_ARGS g, (const unsigned long long*)bits, act, row_scale, out, gx0, accumulate, rows, (int)d, dp.thresh, dp.keep_scale, seed, seed_dev, row0, c_act, c_mix, partial, ridx, g2, seed2, c2, g2_pos
  const dim3 grid((unsigned)nb), blk(kBlock);
  const size_t sh = kBlock * 4 * sizeof(float);
  if (mode == 0 && ridx) hipLaunchKernelGGL((k_trunk_bwd<0, false, true, true>), grid, blk, sh, st, CB_TB_ARGS);
  else if (mode == 0 && !out) hipLaunchKernelGGL((k_trunk_bwd<0, false, false>), grid, blk, sh, st, CB_TB_ARGS);
  else if (mode == 0 && out_bf16) hipLaunchKernelGGL((k_trunk_bwd<0, true>), grid, blk, sh, st, CB_TB_ARGS);
  else if (mode == 0) hipLaunchKernelGGL((k_trunk_bwd<0, false>), grid, blk, sh, st, CB_TB_ARGS);
  else hipLaunchKernelGGL((k_trunk_bwd<1, false>), grid, blk, sh, st, CB_TB_ARGS);
#undef CB_TB_ARGS
  CB_LAUNCH_CHECK();
  return colsum ? colsum_finish(partial, nb, (int)d, colsum, st) : CB_OK;
}

extern "C" int cb_trunk_layer_bwd_f32(const float* g, const uint64_t* relu_bits, const float* row_scale, void* out, int out_bf16,
                                      float* gx0, int accumulate, int64_t rows, int64_t d, float drop_p, uint64_t seed,
                                      const uint64_t* seed_dev, int64_t row0, float c_act, float c_mix, const float* g2, uint64_t seed2, float c2,
                                      const int32_t* g2_pos, float* colsum, void* ws, size_t ws_bytes, void* stream) {
  const char* bad = g2 && !aligned16(g2) ? "misaligned second gradient" : nullptr;
  if (!bad && !(g && relu_bits && (out || colsum) && aligned16(g) && ((uintptr_t)out % (out_bf16 ? 8 : 16) == 0) && (!gx0 || aligned16(gx0)))) bad = kBadPointer;
  const int rc = check_trunk_args("cb_trunk_layer_bwd_f32", rows, d, bad, drop_p, colsum, ws, ws_bytes);
  if (rc != CB_OK || rows == 0) return rc;
  return launch_trunk_bwd(0, out_bf16, g, relu_bits, nullptr, row_scale, out, gx0, accumulate, rows, d, drop_p, seed, seed_dev, row0, c_act, c_mix,
                          colsum, ws, (hipStream_t)stream, nullptr, g2, seed2, c2, g2_pos);
}

// cb_trunk_layer_bwd_f32 for layer 0 of the 'Initial' trunk (all rows, fp32, no in-place accumulator) which also FOLDS the mix gradients:
//   out_m = c_mix * ( dropout_bwd_seed(g) + sum_q dropout_bwd_{mix_seeds[q]}(mix_g[q][mix_pos[q][r] | r]) ),  n_mix <= 2 operands (host arrays; mix_pos[q] NULL: a
// dense [rows, d] operand; else int32 [rows] positions in a compact one, < 0: absent) — what cb_gemm_tn_instage_f32 reads beside dL/d dropout(X0).  out and
// colsum exactly as cb_trunk_layer_bwd_f32 (bit-identical).  The elementwise form of cb_spmm_csr_store_bwd_mix_f32's epilogue, for the levels whose reverse
// aggregation does not carry the store backward (dense levels, mid-size graphs, row shards).
extern "C" int cb_trunk_layer_bwd_fold_f32(const float* g, const uint64_t* relu_bits, const float* row_scale, float* out, int64_t rows, int64_t d, float drop_p,
                                           uint64_t seed, const uint64_t* seed_dev, int64_t row0, float c_act, float c_mix, int32_t n_mix, const float* const* mix_g,
                                           const int32_t* const* mix_pos, const uint64_t* mix_seeds, float* out_m, float* colsum, void* ws, size_t ws_bytes,
                                           int32_t cs_src, const uint64_t* cs_bits, float cs_c, float* colsum2, void* ws2, size_t ws2_bytes, void* stream) {
  const char* bad = !(g && relu_bits && out && out_m && aligned16(g) && aligned16(out) && aligned16(out_m)) ? kBadPointer : nullptr;
  if (!bad && !(n_mix >= 0 && n_mix <= 2 && (n_mix == 0 || (mix_g && mix_seeds)))) bad = "0..2 mix operands";
  const int rc = check_trunk_args("cb_trunk_layer_bwd_fold_f32", rows, d, bad, drop_p, colsum, ws, ws_bytes);
  if (rc != CB_OK || rows == 0) return rc;
  CB_CHECK_ARG(!colsum2 || (cs_src >= 0 && cs_src < n_mix && cs_bits && (uintptr_t)cs_bits % 8 == 0 && ws2 && ws2_bytes >= cb_colsum_workspace_bytes(rows, d)),
               CB_E_INVALID, "cb_trunk_layer_bwd_fold_f32: the second column sum needs an operand index, its mask words and a workspace");
  FoldOps fo{};
  fo.n = n_mix; fo.out_m = out_m;
  fo.cs = {cs_src, (const unsigned long long*)cs_bits, cs_c, colsum2 ? (float*)ws2 : nullptr};
  for (int q = 0; q < n_mix; ++q) {
    CB_CHECK_ARG(mix_g[q] && aligned16(mix_g[q]), CB_E_INVALID, "cb_trunk_layer_bwd_fold_f32: null or misaligned mix operand %d", q);
    fo.g[q] = mix_g[q]; fo.pos[q] = mix_pos ? mix_pos[q] : nullptr; fo.seed[q] = mix_seeds[q];
  }
  const int nb = colsum_blocks(rows);
  const DropParams dp = drop_params(drop_p);
  hipStream_t st = (hipStream_t)stream;
  float* partial = colsum ? (float*)ws : nullptr;
  hipLaunchKernelGGL(k_trunk_bwd_fold, dim3((unsigned)nb), dim3(kBlock), kBlock * 4 * sizeof(float), st, g, (const unsigned long long*)relu_bits, row_scale, out, fo, rows,
                     (int)d, dp.thresh, dp.keep_scale, seed, seed_dev, row0, c_act, c_mix, partial);
  CB_LAUNCH_CHECK();
  int rc2 = colsum ? colsum_finish(partial, nb, (int)d, colsum, st) : CB_OK;
  if (rc2 == CB_OK && colsum2) rc2 = colsum_finish(fo.cs.partial, nb, (int)d, colsum2, st);
  return rc2;
}

// cb_trunk_layer_bwd_f32 over a SUBSET of the rows: g and out are compact [n_rows, d] matrices holding rows row_index[0 .. n_rows) of the full
// ones (ascending global row ids); relu_bits / row_scale are the full arrays, the dropout mask is drawn at the global row.  colsum = the
// column sums over the subset (all other rows of a row-sparse backward are zero).
extern "C" int cb_trunk_layer_bwd_rows_f32(const float* g, const int64_t* row_index, int64_t n_rows, const uint64_t* relu_bits, const float* row_scale,
                                           float* out, int64_t d, float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0, float c_act,
                                           const float* g2, uint64_t seed2, float c2, const int32_t* g2_pos, float* colsum, void* ws, size_t ws_bytes,
                                           void* stream) {
  const char* bad = !(g && row_index && relu_bits && out && aligned16(g) && aligned16(out)) ? kBadPointer : nullptr;
  const int rc = check_trunk_args("cb_trunk_layer_bwd_rows_f32", n_rows, d, bad, drop_p, colsum, ws, ws_bytes);
  if (rc != CB_OK) return rc;
  if (n_rows == 0) {
    if (colsum) CB_HIP(hipMemsetAsync(colsum, 0, (size_t)d * sizeof(float), (hipStream_t)stream));
    return CB_OK;
  }
  CB_CHECK_ARG(!g2 || (aligned16(g2) && g2_pos), CB_E_INVALID, "cb_trunk_layer_bwd_rows_f32: the second gradient needs 16-byte aligned rows and its position map");
  return launch_trunk_bwd(0, 0, g, relu_bits, nullptr, row_scale, out, nullptr, 0, n_rows, d, drop_p, seed, seed_dev, row0, c_act, 0.f, colsum, ws,
                          (hipStream_t)stream, row_index, g2, seed2, c2, g2_pos);
}

extern "C" int cb_trunk_input_bwd_f32(const float* g, const float* add, const float* act, float* out, int64_t rows, int64_t d,
                                      float drop_p, uint64_t seed, const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws,
                                      size_t ws_bytes, void* stream) {
  const char* bad = !(g && add && act && out && aligned16(g) && aligned16(add) && aligned16(act) && aligned16(out)) ? kBadPointer : nullptr;
  const int rc = check_trunk_args("cb_trunk_input_bwd_f32", rows, d, bad, drop_p, colsum, ws, ws_bytes);
  if (rc != CB_OK || rows == 0) return rc;
  return launch_trunk_bwd(1, 0, g, nullptr, act, nullptr, out, const_cast<float*>(add), 1, rows, d, drop_p, seed, seed_dev, row0, 0.f, 0.f, colsum,
                          ws, (hipStream_t)stream);
}

static int trunk_input_bwd_multi_impl(const float* g, uint64_t seed, int32_t n_mix, const float* const* g_mix, const uint64_t* seeds_mix,
                                      float c_mix, const float* act, float* out, int64_t rows, int64_t d, float drop_p,
                                      const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws, size_t ws_bytes,
                                      const uint64_t* act_bits, const int32_t* const* g_mix_pos, void* stream, int32_t n_cs, const int32_t* cs_src,
                                      const uint64_t* const* cs_bits, const float* cs_c, float* const* colsum2, void* ws2, size_t ws2_bytes) {
  CB_CHECK_ARG(n_mix >= 0 && n_mix <= kMixMax && (n_mix == 0 || (g_mix && seeds_mix)), CB_E_INVALID,
               "cb_trunk_input_bwd_multi_f32: 0..%d mixed-in gradients", kMixMax);
  const char* bad = !(g && (act || act_bits) && out && aligned16(g) && (!act || aligned16(act)) && aligned16(out) && ((uintptr_t)act_bits % 8 == 0)) ? kBadPointer : nullptr;
  const int rc = check_trunk_args("cb_trunk_input_bwd_multi_f32", rows, d, bad, drop_p, colsum, ws, ws_bytes);
  if (rc != CB_OK || rows == 0) return rc;
  MixTable mt{};
  mt.n = n_mix;
  for (int i = 0; i < n_mix; ++i) mt.pos[i] = g_mix_pos ? g_mix_pos[i] : nullptr;
  CB_CHECK_ARG(n_cs >= 0 && n_cs <= 2 && (n_cs == 0 || (cs_src && cs_bits && cs_c && colsum2)), CB_E_INVALID, "cb_trunk_input_bwd_multi_cs_f32: 0..2 extra column sums");
  const size_t plane = cb_colsum_workspace_bytes(rows, d);
  CB_CHECK_ARG(n_cs == 0 || (ws2 && ws2_bytes >= (size_t)n_cs * plane), CB_E_WORKSPACE, "cb_trunk_input_bwd_multi_cs_f32: second workspace too small");
  for (int q = 0; q < n_cs; ++q) {
    CB_CHECK_ARG(cs_src[q] >= 0 && cs_src[q] < n_mix && cs_bits[q] && (uintptr_t)cs_bits[q] % 8 == 0 && colsum2[q], CB_E_INVALID,
                 "cb_trunk_input_bwd_multi_cs_f32: extra column sum %d needs an operand index, its mask words and a result vector", q);
    mt.cs[q] = {cs_src[q], (const unsigned long long*)cs_bits[q], cs_c[q], (float*)((char*)ws2 + (size_t)q * plane)};
  }
  for (int i = 0; i < n_mix; ++i) {
    CB_CHECK_ARG(g_mix[i] && aligned16(g_mix[i]), CB_E_INVALID, "cb_trunk_input_bwd_multi_f32: null or misaligned mixed-in gradient %d", i);
    mt.g[i] = g_mix[i];
    mt.seed[i] = seeds_mix[i];
  }
  const int nb = colsum_blocks(rows);
  const DropParams dp = drop_params(drop_p);
  hipStream_t st = (hipStream_t)stream;
  float* partial = colsum ? (float*)ws : nullptr;
#define CB_MIX_LAUNCH(N_)                                                                                                        \
  hipLaunchKernelGGL((k_trunk_input_bwd_multi<N_>), dim3((unsigned)nb), dim3(kBlock), kBlock * 4 * sizeof(float), st, g, mt, act, (const unsigned long long*)act_bits, out, rows, \
                     (int)d, dp.thresh, dp.keep_scale, seed, seed_dev, row0, c_mix, partial)
  switch (n_mix) {
    case 0: CB_MIX_LAUNCH(0); break;
    case 1: CB_MIX_LAUNCH(1); break;
    case 2: CB_MIX_LAUNCH(2); break;
    case 3: CB_MIX_LAUNCH(3); break;
    case 4: CB_MIX_LAUNCH(4); break;
    case 5: CB_MIX_LAUNCH(5); break;
    case 6: CB_MIX_LAUNCH(6); break;
    default: CB_MIX_LAUNCH(7); break;
  }
#undef CB_MIX_LAUNCH
  CB_LAUNCH_CHECK();
  int rc2 = colsum ? colsum_finish(partial, nb, (int)d, colsum, st) : CB_OK;
  for (int q = 0; q < n_cs && rc2 == CB_OK; ++q) rc2 = colsum_finish(mt.cs[q].partial, nb, (int)d, colsum2[q], st);
  return rc2;
}

extern "C" int cb_trunk_input_bwd_multi_f32(const float* g, uint64_t seed, int32_t n_mix, const float* const* g_mix, const uint64_t* seeds_mix,
                                            float c_mix, const float* act, float* out, int64_t rows, int64_t d, float drop_p,
                                            const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws, size_t ws_bytes,
                                            const uint64_t* act_bits, const int32_t* const* g_mix_pos, void* stream) {
  return trunk_input_bwd_multi_impl(g, seed, n_mix, g_mix, seeds_mix, c_mix, act, out, rows, d, drop_p, seed_dev, row0, colsum, ws, ws_bytes, act_bits, g_mix_pos,
                                    stream, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
}

// The same, which also returns n_cs (<= 2) extra column sums: colsum2[q] = the column sums of cs_c[q] * dropout_bwd_{seeds_mix[cs_src[q]]}(g_mix[cs_src[q]])
// through the mask words cs_bits[q] (indexed by the node row, also for a compact operand) — the bias gradients of the stores whose backward was applied by
// cb_spmm_csr_store_bwd_f32.  Dense operand: the partial-sum order of cb_trunk_layer_bwd_f32's column sums (bit-identical).  ws2: n_cs planes of
// cb_colsum_workspace_bytes(rows, d).
extern "C" int cb_trunk_input_bwd_multi_cs_f32(const float* g, uint64_t seed, int32_t n_mix, const float* const* g_mix, const uint64_t* seeds_mix,
                                               float c_mix, const float* act, float* out, int64_t rows, int64_t d, float drop_p,
                                               const uint64_t* seed_dev, int64_t row0, float* colsum, void* ws, size_t ws_bytes,
                                               const uint64_t* act_bits, const int32_t* const* g_mix_pos, int32_t n_cs, const int32_t* cs_src,
                                               const uint64_t* const* cs_bits, const float* cs_c, float* const* colsum2, void* ws2, size_t ws2_bytes,
                                               void* stream) {
  return trunk_input_bwd_multi_impl(g, seed, n_mix, g_mix, seeds_mix, c_mix, act, out, rows, d, drop_p, seed_dev, row0, colsum, ws, ws_bytes, act_bits, g_mix_pos,
                                    stream, n_cs, cs_src, cs_bits, cs_c, colsum2, ws2, ws2_bytes);
}

extern "C" int cb_trunk_store_rows_f32(const float* y, const int64_t* row_index, int64_t n_rows, int64_t d, const cb_trunk_store* store, float* out, void* stream) {
  const char* who = "cb_trunk_store_rows_f32";
  CB_CHECK_ARG(n_rows >= 0 && d > 0 && d % 256 == 0 && d < (1 << 20), CB_E_INVALID, "%s: d must be a multiple of 256", who);
  if (n_rows == 0) return CB_OK;
  CB_CHECK_ARG(y && row_index && out && aligned16(y) && aligned16(out), CB_E_INVALID, "%s: null or misaligned pointer", who);
  const int rcs = check_trunk_store(who, store, d);
  if (rcs != CB_OK) return rcs;
  const int nb = grid_for(n_rows * kWave);      // one wavefront per row
  hipLaunchKernelGGL(k_trunk_store_rows, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)stream, y, row_index, n_rows, (int)d, make_trunk_store(*store), out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
