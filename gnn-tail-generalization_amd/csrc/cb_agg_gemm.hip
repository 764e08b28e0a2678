// Aggregation + the NEXT dense transform in one kernel ("the matrix cores run under the gathers").
//
// Replaces, per layer of the residual trunk, the pair
//     forward :  X_{l+1} = store( A^T Z_l )                     GNN_model/GCN.py:238-253,127-133   (cb_spmm_csr_fused_f32)
//                Z_{l+1} = a . (X_{l+1} W_{l+1}) + E_{l+1}      GNN_model/GCN.py:213,225,230-235    (cb_gemm_nn_f32)
//     backward:  dZ_l    = A (b . dY'_l)                        autograd of :238                    (cb_spmm_csr_f32, reverse CSR)
//                dX_l    = a . (dZ_l W_l^T)                     autograd of :213,225                (cb_gemm_nn_f32)
// by ONE launch each: one persistent block of 12 wavefronts per CU.  Wavefronts 0-7 aggregate 64-row tiles exactly as k_spmm_rows does
// (same edge-stream walk, same stores: X_{l+1} / dZ_l still go to memory, the weight-gradient GEMM needs them) and leave every finished row
// in one of two fp32 LDS tiles (64 x 256, 65 KB each); wavefronts 8-11 multiply the other tile by the 256 x 256 weight and store.  The tile
// buffers change hands through two LDS counters per buffer (no block barrier).  What disappears: the second kernel's 10 GB read of the
// matrix just written, and the matrix cores' time as a term of its own (profiles/r03_fused_agg_gemm.md).
//
// Arithmetic of the dense part = cb_gemm_limb.hip's, product by product: fp32 operands as three exact bf16 limbs, the six leading
// limb products per K step in the same order into fp32 MFMA accumulators, `rowscale * acc + addend` on the way out — results are
// bit-identical to cb_gemm_nn_f32 on the same inputs (tests/test_gpu_agg_gemm.py, tests/test_gpu_fullsize.py at 10^7 rows).
//   A operand: the LDS tile; a fragment (8 consecutive k of one row) = two ds_read_b128, split into limbs in registers
//              (1040-byte tile rows: the 16 lanes of a b128 group hit 16 distinct 16-byte bank columns);
//   B operand: the weight, split ONCE per launch by k_weight_image into MFMA fragment order (384 KB, L2 resident): a fragment is
//              one coalesced global_load_dwordx4 per limb, no LDS, no conversion in the K loop;
//   C: accumulators -> wave-private LDS strips -> row-major float4 -> epilogue -> 256-byte streaming row segments.
// Hub rows (more edges than the hub threshold) are reduced by the hub kernels, which run BEFORE this kernel (launch_hub_rows); their finished
// rows are read back from memory into the tile.  The row block's head (load_row_block), its cut among the gathering wavefronts (tile_row_cut)
// and the walk itself (stream_rows) are cb_spmm_core.h's, shared with k_spmm_rows and cb_sage.hip.
// ACC forms (node-sharded path, dist.py): the reduction of a row starts from the partial sums of the earlier passes (interior columns,
// earlier halo slices) — the LAST halo pass of a rank's aggregation then also produces the next layer's Z / this layer's dX.
#include <stdlib.h>
#include <string.h>

#include "cb_common.h"
#include "cb_limb_core.h"
#include "cb_spmm_core.h"
#include "cb_tile_gemm.h"

namespace cb {

struct GemmTail {
  const uint4* image;      // weight limbs in fragment order (k_weight_image)
  const float* rowscale;   // [rows] or null
  const float* addend;     // [rows, ld_add] or null
  int64_t ld_add;
  float* out;              // [rows, ld_out]
  int64_t ld_out;
  TrunkStore st;
  int* err;                // device-visible error word (cb_error.hip): a tile hand-over that timed out is recorded here, never silent
  // NARROW kernels only (the output Linear as the tail of the last layer's aggregation, GCN.py:133-138): out[m][n] = acc + bias[n], n < n_out <= 64
  const float* bias;       // [n_out] or null (SR kernels: [256] or null)
  int n_out;
  // SR kernels only (rows-only forward, trunk.py _layer_on_rows: the trunk's store on a SUBSET of the node rows as the tail — the expression of
  // cb_gemm_nn_store_rows_f32, cb_gemm_core.h nn_epilogue EPI == 2): with gm = row_ids[m],
  //   act = relu(rowscale[m] * acc + bias) (-> st.out_act);  out = the store's value at node row gm, mask words st.bits[gm][4]
  const int64_t* row_ids;
};

// (declared in cb_tile_gemm.h)
__global__ void __launch_bounds__(256) k_weight_image(const float* __restrict__ W, int64_t sk, int64_t sn, uint4* __restrict__ image, int n_steps) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int lane = idx & 63, sj = idx >> 6, j = sj % kNT, s = sj / kNT;
  if (s >= n_steps) return;
  const int k0 = 16 * s + 8 * (lane >> 5), n = 32 * j + (lane & 31);
  uint32_t h[4], m[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    split3x2(W[(int64_t)(k0 + 2 * e) * sk + (int64_t)n * sn], W[(int64_t)(k0 + 2 * e + 1) * sk + (int64_t)n * sn], h[e], m[e], l[e]);
  uint4* o = image + ((int64_t)(s * kNT + j) * 3) * 64 + lane;
  o[0] = make_uint4(h[0], h[1], h[2], h[3]);
  o[64] = make_uint4(m[0], m[1], m[2], m[3]);
  o[128] = make_uint4(l[0], l[1], l[2], l[3]);
}

// B[k][n] = W[k * sk + n * sn] for n < n_cols, zero beyond: the narrow image (kNTn = 2 column blocks) of a 256 x C weight, C <= 64
__global__ void __launch_bounds__(256) k_weight_image_narrow(const float* __restrict__ W, int64_t sk, int64_t sn, uint4* __restrict__ image, int n_steps,
                                                             int n_cols) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int lane = idx & 63, sj = idx >> 6, j = sj % kNTn, s = sj / kNTn;
  if (s >= n_steps) return;
  const int k0 = 16 * s + 8 * (lane >> 5), n = 32 * j + (lane & 31);
  uint32_t h[4], m[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float w0 = n < n_cols ? W[(int64_t)(k0 + 2 * e) * sk + (int64_t)n * sn] : 0.f;
    const float w1 = n < n_cols ? W[(int64_t)(k0 + 2 * e + 1) * sk + (int64_t)n * sn] : 0.f;
    split3x2(w0, w1, h[e], m[e], l[e]);
  }
  uint4* o = image + ((int64_t)(s * kNTn + j) * 3) * 64 + lane;
  o[0] = make_uint4(h[0], h[1], h[2], h[3]);
  o[64] = make_uint4(m[0], m[1], m[2], m[3]);
  o[128] = make_uint4(l[0], l[1], l[2], l[3]);
}

// Hand-over of the LDS tile buffers WITHOUT a block barrier: two counters per buffer in LDS.
//   ready[b]: +1 by every gathering wavefront that has written its rows of the tile in buffer b   (tile complete at kNG * (use + 1))
//   freed[b]: +1 by every multiplying wavefront that has read the tile in buffer b for the last time (buffer reusable at 4 * use)
// A wavefront's LDS instructions are executed in order, so a counter increment issued after the tile writes (or reads) is seen after them;
// the asm statements only keep the COMPILER from moving LDS accesses across the hand-over.  No wait on outstanding global loads / stores
// (a block barrier drains them): a gathering wavefront that has finished its rows moves on to the next tile while its row stores are still
// in flight and while the other wavefronts finish theirs, so the eight gathering wavefronts of a CU drift apart and cover each other's
// start-of-tile latencies (rowptr -> column ids -> first gathers), which a barrier lines up.
// Spins are bounded so that a lost hand-over can never hang the GPU — and it is never silent: the wavefront that gives up records
// CB_DEVERR_HANDOVER (+ block and counter target) in the device error word; every later cb_spmm_gemm_* call and cb_device_status()
// then return CB_E_DEVICE (the results of the launch that timed out are invalid).
constexpr int kSpinLimit = 1 << 26;      // ~7 s of s_sleep
__device__ __forceinline__ void ag_wait(int* flag, int target, int* err, int spin_limit = kSpinLimit) {
  int spins = 0;
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > spin_limit) {
      if (err && lane_id() == 0) {
        __hip_atomic_store(err + 1, (int)blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(err + 2, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(err, CB_DEVERR_HANDOVER, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      break;
    }
  }
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void ag_signal(int* flag, int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- one persistent 12-wavefront block per CU, wavefront-specialised ------------------------------------------------------------
// Two co-resident blocks that each alternate gather / MFMA phases fall into lock step (both gather, then both multiply: measured,
// profiles/r03_fused_agg_gemm.md), so nothing overlaps.  Here the roles are fixed instead: wavefronts 0-7 only gather (tile t+1
// into one LDS buffer), wavefronts 8-11 only multiply (tile t from the other buffer) and store.  The 64 rows of a tile are cut among the
// gathering wavefronts at equal EDGE counts (row boundaries from the tile's rowptr values, ballots), so that they finish together —
// a fixed 8 rows each leaves the tile waiting for the wavefront with the heaviest rows.
constexpr int kNG = 8;       // gathering wavefronts (3 wavefronts per SIMD at <= 168 registers; 12 gathers in flight each)
constexpr int kU = 12;       // gathers in flight per gathering wavefront (16: spills; 8: slower — profiles/r03_fused_agg_gemm.md)

// One gathering wavefront's share of tile t (tile_row_cut of cb_spmm_core.h) into the LDS tile and, as k_spmm_rows does, to memory
template <bool FUSED, int GP, bool ACC, bool CS = false>
__device__ __forceinline__ void ag2_gather_tile(int t, float* __restrict__ tile, int w, int lane, const int* __restrict__ rowptr,
                                                const int* __restrict__ col, const float* __restrict__ h, int64_t ld_h, float* __restrict__ out,
                                                int64_t ld_out, int n_rows, const Epilogue& ep, int hub_T, const FusedEpi& fe) {
  const int r0 = t * kTM;
  const int nrt = min(kTM, n_rows - r0);
  const int c0 = lane * 4;
  const auto blk = load_row_block<true>(rowptr, ep.row_scale, hub_T, r0, nrt);
  const RowCut cut = tile_row_cut<kNG>(blk, nrt, w);
  const int rb = cut.rb;
  float bvec[4] = {0.f, 0.f, 0.f, 0.f};
  if (ep.bias) {
#pragma unroll
    for (int i = 0; i < 4; ++i) bvec[i] = ep.bias[c0 + i];
  }
  const float* h_lane = h + c0;
  float* out_lane = out + c0;
  float* tile_lane = tile + c0;
  const float* init_lane = ACC ? ep.acc_init + c0 : nullptr;
  int r = cut.ra;
  while (r < rb) {      // maximal hub-free runs of [ra, rb)
    const unsigned long long m = (blk.hubmask >> r) & (rb - r >= 64 ? ~0ull : ((1ull << (rb - r)) - 1ull));
    const int nh = m ? r + (__ffsll((long long)m) - 1) : rb;
    if (nh > r)
      stream_rows<4, kU, true, FUSED, ACC, float, GP, kTLD, true, CS>(r, nh, nrt, blk.my_ptr, blk.my_scale, r0, col, h_lane, ld_h, out_lane, ld_out, true,
                                                                         ep.relu, bvec, fe, c0, init_lane, ep.ld_init, ep, tile_lane, blk.ptr_hi);
    if (nh < rb) {      // hub row nh: finished by the hub kernels, which ran before this launch
      const float* src = FUSED ? fe.out_next + (int64_t)(r0 + nh) * fe.ld_next + c0 : out + (int64_t)(r0 + nh) * ld_out + c0;
      *reinterpret_cast<float4*>(tile_lane + nh * kTLD) = *reinterpret_cast<const float4*>(src);
    }
    r = nh + 1;
  }
  if (w == kNG - 1) zero_tile_rows<kTLD>(tile_lane, nrt, kTM);
}

// One K step of B fragments in flight per multiplying wavefront (two register buffers, K loop unrolled by two): next to wavefronts that
// keep dozens of gathers outstanding, a load of this CU — L2 hit or not — comes back after microseconds.  For the same reason the tails below
// put NO load between their stores (profiles/tail_loads.md): what an epilogue reads per row (row scale, row id, mixed-in row index) is loaded
// once per tile BEFORE the K loop, one row per lane (lane l: tile row l; lanes past the tile's last row read nothing), and reaches the epilogue
// by a lane exchange; what it reads per column (bias) is loaded once per wavefront, outside the tile loop.  On gfx9 vmcnt counts stores as
// well as loads, so a load between two stores makes its wait cover the earlier store: sixteen serial round trips per tile before.
__device__ __forceinline__ float tile_lane_scale(const float* __restrict__ rowscale, int r0, int lane, int n_rows) {
  return (rowscale && r0 + lane < n_rows) ? rowscale[(int64_t)r0 + lane] : 1.f;
}

// The lane id as a value the compiler must take as new in every tile.  What a tail derives from it (the sixteen source lanes of a tile's lane
// exchanges, the addresses of the per-lane row loads) would otherwise be invariants of the persistent tile loop, hoisted out of it and kept in
// registers across the K loop: spills.
__device__ __forceinline__ int tile_variant(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

__device__ __forceinline__ void ag2_mfma_tile(int t, const float* __restrict__ tile, float* __restrict__ cs, int w, int lane, int n_rows,
                                              const GemmTail& gt, int* freed) {
  const int l31 = lane & 31, lh = lane >> 5;
  const int r0 = t * kTM;
  const int lane_v = tile_variant(lane), lrow = lane_v >> 4;
  const float rs_lane = tile_lane_scale(gt.rowscale, r0, lane_v, n_rows);      // (in flight under the K loop)
  f32x16 acc[2][2];
  tile_times_image<kNS, kTLD>(tile, gt.image, w, lane, acc);
  ag_signal(freed, lane);      // the tile has been read for the last time
  // epilogue through a WAVE-PRIVATE staging strip (the tile itself is still being read by the other three multiplying wavefronts
  // and there is no barrier among four of twelve wavefronts): 8 rows x 64 columns per pass, transposed so that a lane applies
  // `rowscale * acc + addend` on a float4 and the strip leaves as 256-byte row segments.  Two copies, with and without an addend: without
  // one (the training step) the sixteen stores of a tile follow each other with no wait on memory in between; with one, a pass's two addend
  // vectors are fetched before the pass's transposition.
  const float zero_bias = 0.f;      // (keeps the epilogue expression of cb_gemm_core.h's nn_epilogue: o * rs + addend + bias)
  auto epilogue = [&](auto HAS_ADD) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int mt0 = 32 * i + 8 * q + lrow;      // tile row of half 0; half 1: + 4
        float ad[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if constexpr (decltype(HAS_ADD)::value) {
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int64_t m = (int64_t)r0 + mt0 + 4 * half;      // (rows past the end re-read the last row, unused: unpredicated loads keep the waits counted)
            gather<4>(ad[half], gt.addend + (m < n_rows ? m : (int64_t)n_rows - 1) * gt.ld_add + 64 * w + (lane & 15) * 4);
          }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
          for (int j = 0; j < 2; ++j) cs[(r4 + 4 * lh) * kCLD + 32 * j + l31] = acc[i][j][4 * q + r4];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int idx = lane + 64 * half, row = idx >> 4, c4 = (idx & 15) * 4;
          const int64_t m = r0 + 32 * i + 8 * q + row;
          const float4 v = *reinterpret_cast<const float4*>(cs + row * kCLD + c4);
          const float rs = __shfl(rs_lane, mt0 + 4 * half);      // (every lane takes part: the source lane may hold a row past the end)
          if (m < n_rows) {
            const int n = 64 * w + c4;
            float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = o[e] * rs + ad[half][e] + zero_bias;
            store_stream<4>(gt.out + m * gt.ld_out + n, o);
          }
        }
      }
  };
  if (gt.addend) epilogue(std::true_type{});
  else epilogue(std::false_type{});
}

// NARROW tail: multiplying wavefront w takes the 32 x 32 block (rows 32 (w & 1), columns 32 (w >> 1)) of the tile's 64 x 64 output = the
// logits of 64 rows (C <= 64 classes): out = acc + bias, the epilogue expression of cb_gemm_nn_f32 with a bias and neither row scale nor addend.
// hb = the bias of this lane's four columns (head_lane_bias: loaded once per wavefront, zero beyond n_out or without a bias)
__device__ __forceinline__ void head_lane_bias(const GemmTail& gt, int w, int lane, float (&hb)[4]) {
  const int n = 32 * (w >> 1) + (lane & 7) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) hb[e] = (gt.bias && n + e < gt.n_out) ? gt.bias[n + e] : 0.f;
}

__device__ __forceinline__ void ag2_mfma_tile_head(int t, const float* __restrict__ tile, float* __restrict__ cs, int w, int lane, int n_rows,
                                                   const GemmTail& gt, int* freed, const float (&hb)[4]) {
  const int l31 = lane & 31, lh = lane >> 5, bi = w & 1, bj = w >> 1;
  f32x16 acc;
  tile_times_image_block<kNS, kTLD>(tile, gt.image, bi, bj, lane, acc);
  ag_signal(freed, lane);      // the tile has been read for the last time
  const int r0 = t * kTM + 32 * bi;
#pragma unroll
  for (int q = 0; q < 4; ++q) {      // 8 rows x 32 columns per pass through the wave-private strip
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) cs[(r4 + 4 * lh) * kCLD + l31] = acc[4 * q + r4];
    const int row = lane >> 3, c4 = (lane & 7) * 4;
    const float4 v = *reinterpret_cast<const float4*>(cs + row * kCLD + c4);
    const int64_t m = r0 + 8 * q + row;
    const int n = 32 * bj + c4;
    if (m < n_rows && n < gt.n_out) {
      const float zero_add = 0.f;
      float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] * 1.f + zero_add + hb[e];
      float* dst = gt.out + m * gt.ld_out + n;
      if (n + 4 <= gt.n_out && (gt.ld_out & 3) == 0) {
        store_stream<4>(dst, o);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < gt.n_out) dst[e] = o[e];
      }
    }
  }
}

// SR tail (the trunk's store on a subset of the node rows): multiplying wavefront w owns columns 64 w .. 64 w + 63 of each row, i.e. 16 bits of
// each of the row's four mask words (word e, bit L <-> column 4 L + e).  Its pieces go to the tile's 2 KB of LDS words (ushort w of word e of
// tile row mt); the LAST of the four wavefronts to finish the tile (LDS counter mw_cnt, no barrier) writes the assembled words, one 16-byte
// vector store per two words, and releases the buffer (mw_done: the pieces of buffer b's next tile wait for it).
// Per row the tail needs the node row id (Philox counter, mask-word address), the row scale and the mixed-in row's index: loaded one row per
// lane before the K loop.  The mixed-in rows themselves are gathered one pass ahead of their use (two register sets), so that a wait for
// them never covers a load issued in the same pass.  bias_lds = the 256 bias values (zeros without a bias), put into LDS once per block: four
// registers held across the K loop are four too many here (the kernel sits at its register limit).
__device__ __forceinline__ void ag2_mfma_tile_rows(int t, const float* __restrict__ tile, float* __restrict__ cs, int w, int lane, int n_rows,
                                                   const GemmTail& gt, uint64_t seed_eff, int* freed, unsigned short* __restrict__ words,
                                                   int* mw_cnt, int* mw_done, int use, const float* __restrict__ bias_lds) {
  const int l31 = lane & 31, lh = lane >> 5;
  const int r0 = t * kTM;
  const int n = 64 * w + (lane & 15) * 4;
  // lane l: tile row l
  const int lane_v = tile_variant(lane), lrow = lane_v >> 4;
  const int64_t m_lane = (int64_t)r0 + lane_v;
  const bool live_lane = m_lane < n_rows;
  const long long gm_lane = live_lane ? (long long)gt.row_ids[m_lane] : 0ll;
  const float rs_lane = tile_lane_scale(gt.rowscale, r0, lane_v, n_rows);
  // (store_mix_row: mix_index[m] where the store has a mix_index, the node row otherwise — chosen after the exchange, so that nothing here waits for gm_lane)
  const long long mixi_lane = (live_lane && gt.st.mix_src && gt.st.mix_index) ? (long long)gt.st.mix_index[m_lane] : 0ll;
  f32x16 acc[2][2];
  int64_t image_off = 0;
  asm volatile("" : "+s"(image_off));      // (tile-variant as well: the K loop's start addresses are not kept as invariants beside its running ones)
  tile_times_image<kNS, kTLD>(tile, gt.image + image_off, w, lane, acc);
  ag_signal(freed, lane);      // the tile has been read for the last time
  if (gt.st.bits && use > 0) ag_wait(mw_done, use, gt.err);      // the words of this buffer's previous tile have left
  const float4 b4 = *reinterpret_cast<const float4*>(bias_lds + n);
  const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
  auto epilogue = [&](auto MIX) {
    constexpr bool kMix = decltype(MIX)::value;
    float qn[2][2][4];      // the mixed-in rows of two passes: [pass parity][half]
    auto fetch_mix = [&](int pass, float (&dst)[2][4]) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int mt = 8 * pass + 4 * half + lrow;
        const long long mr = __shfl(gt.st.mix_index ? mixi_lane : gm_lane, mt);
        gather<4>(dst[half], gt.st.mix_src + mr * gt.st.ld_mix + n);      // (rows past the end: mr == 0, row 0 of mix_src, unused — unpredicated, so that the waits stay counted)
      }
    };
    if constexpr (kMix) fetch_mix(0, qn[0]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int pass = 4 * i + q;
        if constexpr (kMix) {
          if (pass + 1 < 8) fetch_mix(pass + 1, qn[(pass + 1) & 1]);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
          for (int j = 0; j < 2; ++j) cs[(r4 + 4 * lh) * kCLD + 32 * j + l31] = acc[i][j][4 * q + r4];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int idx = lane + 64 * half, row = idx >> 4, c4 = (idx & 15) * 4;
          const int mt = 32 * i + 8 * q + row, mts = 32 * i + 8 * q + 4 * half + lrow;      // (mts == mt, tile-variant for the compiler)
          const int64_t m = r0 + mt;
          const float4 v = *reinterpret_cast<const float4*>(cs + row * kCLD + c4);
          const bool live = m < n_rows;
          const int64_t gm = __shfl(gm_lane, mts);      // (every lane takes part: the source lane may hold a row past the end)
          const float rs = __shfl(rs_lane, mts);
          float o[4] = {v.x, v.y, v.z, v.w}, mk[4] = {1.f, 1.f, 1.f, 1.f};
          if (live) {      // nn_epilogue's expression (cb_gemm_core.h), then the store's steps (cb_trunk_store.h)
            const float ad[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              o[e] = o[e] * rs + ad[e] + bv[e];
              o[e] = relu_nan(o[e]);
            }
            store_keep4(gt.st, seed_eff, gm, kND, n, mk);
          }
          if (gt.st.bits) {
            // ballot e: bits 16 k .. 16 k + 15 = row (lane >> 4 == k) of this pass, columns 64 w .. 64 w + 63 -> bits 16 w .. of word e
            unsigned long long bal[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) bal[e] = __ballot(live && store_passes_grad(gt.st, o[e], mk[e]));
            if (lane < 16) {
              const int k = lane >> 2, e = lane & 3;
              unsigned long long be = bal[0];
#pragma unroll
              for (int f = 1; f < 4; ++f) if (e == f) be = bal[f];
              const int mtk = 32 * i + 8 * q + 4 * half + k;
              words[(mtk * 4 + e) * 4 + w] = (unsigned short)(be >> (16 * k));
            }
          }
          if (live) {
            if (gt.st.out_act) store_stream<4>(gt.st.out_act + m * gt.st.ld_act + n, o);
            float qv[4] = {0.f, 0.f, 0.f, 0.f}, x[4];
            if constexpr (kMix) {
#pragma unroll
              for (int e = 0; e < 4; ++e) qv[e] = qn[pass & 1][half][e];
            }
            store_value(gt.st, o, qv, mk, x);
            store_stream<4>(gt.out + m * gt.ld_out + n, x);
          }
        }
      }
  };
  if (gt.st.mix_src) epilogue(std::true_type{});
  else epilogue(std::false_type{});
  if (gt.st.bits) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wavefront's pieces are in LDS
    int prev = 0;
    if (lane == 0) prev = __hip_atomic_fetch_add(mw_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    prev = __shfl(prev, 0);
    asm volatile("" ::: "memory");
    if (prev == 4 * use + 3) {      // the last of the four: every piece of the tile is in place
      if (live_lane) {
        const uint4* src = reinterpret_cast<const uint4*>(words + lane * 16);
        const uint4 w01 = src[0], w23 = src[1];
        uint4* dst = reinterpret_cast<uint4*>(gt.st.bits + gm_lane * 4);
        dst[0] = w01;
        dst[1] = w23;
      }
      ag_signal(mw_done, lane);
    }
  }
}

template <bool FUSED, int GP, bool ACC, bool NARROW = false, bool SR = false>
__global__ void __launch_bounds__(64 * (kNG + 4), (kNG + 4) / 4) k_agg_gemm2(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                            const float* __restrict__ h, int64_t ld_h, float* __restrict__ out,
                                                                            int64_t ld_out, int n_rows, Epilogue ep, int hub_T, FusedEpi fe,
                                                                            GemmTail gt, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float tiles[2][kTM * kTLD];
  __shared__ __attribute__((aligned(16))) float cstrip[4][8 * kCLD];
  __shared__ int ready[2], freed[2];
  __shared__ __attribute__((aligned(16))) unsigned short mwords[SR ? 2 : 1][SR ? kTM * 16 : 8];      // SR: the tile's mask words, in pieces
  __shared__ int mw_cnt[2], mw_done[2];
  __shared__ __attribute__((aligned(16))) float sr_bias[SR ? kND : 4];      // SR: the tail's bias (zeros without one)
  const int lane = lane_id(), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (wave-uniform by construction: tell the compiler, so that what derives from it stays in SGPRs)
  const bool gathers = wv < kNG;
  const int w = gathers ? wv : wv - kNG;
  const int n_it = ((int)blockIdx.x < n_tiles) ? (n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  const uint64_t seed_eff = SR ? store_seed(gt.st) : 0ull;
  if (threadIdx.x < 2) ready[threadIdx.x] = freed[threadIdx.x] = mw_cnt[threadIdx.x] = mw_done[threadIdx.x] = 0;
  if constexpr (SR) {
    if (threadIdx.x < kND) sr_bias[threadIdx.x] = gt.bias ? gt.bias[threadIdx.x] : 0.f;
  }
  __syncthreads();
  if (gathers) {
    for (int it = 0; it < n_it; ++it) {
      const int b = it & 1, use = it >> 1;
      if (use > 0) ag_wait(&freed[b], 4 * use, gt.err);
      ag2_gather_tile<FUSED, GP, ACC, SR>(blockIdx.x + it * gridDim.x, tiles[b], w, lane, rowptr, col, h, ld_h, out, ld_out, n_rows, ep, hub_T, fe);
      ag_signal(&ready[b], lane);
    }
  } else {
    float head_bias[4] = {0.f, 0.f, 0.f, 0.f};      // NARROW: the bias of this lane's columns, once per wavefront
    if constexpr (NARROW) head_lane_bias(gt, w, lane, head_bias);
    for (int it = 0; it < n_it; ++it) {
      const int b = it & 1, use = it >> 1;
      ag_wait(&ready[b], kNG * (use + 1), gt.err);
      if constexpr (NARROW) ag2_mfma_tile_head(blockIdx.x + it * gridDim.x, tiles[b], cstrip[w], w, lane, n_rows, gt, &freed[b], head_bias);
      else if constexpr (SR)
        ag2_mfma_tile_rows(blockIdx.x + it * gridDim.x, tiles[b], cstrip[w], w, lane, n_rows, gt, seed_eff, &freed[b], mwords[b], &mw_cnt[b], &mw_done[b], use,
                           sr_bias);
      else ag2_mfma_tile(blockIdx.x + it * gridDim.x, tiles[b], cstrip[w], w, lane, n_rows, gt, &freed[b]);
    }
  }
}

// Fault injection for the hand-over's failure path (tests only reach it through cb_agg_gemm_handover_selftest): one wavefront waits, with a
// short spin bound, for a counter nobody increments.
__global__ void __launch_bounds__(64) k_agg_handover_selftest(int* err) {
  __shared__ int never;
  if (threadIdx.x == 0) never = 0;
  __syncthreads();
  ag_wait(&never, 1, err, 1 << 10);
}

constexpr int kMaxBlocks = 1024;      // cap of the persistent grid

// blocks of the persistent kernel: one per CU of the current device (139 KB of LDS each)
static int ag_n_blocks(int n_tiles) {
  int dev = 0, n_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) n_cu = 256;
  if (n_cu > kMaxBlocks) n_cu = kMaxBlocks;
  return n_tiles < n_cu ? n_tiles : n_cu;
}

template <bool FUSED, bool ACC>
static int launch_agg_gemm(const cb_csr_view& g, const float* h, int64_t ld_h, Epilogue ep, float* out, int64_t ld_out, hipStream_t st, FusedEpi fe,
                           GemmTail gt) {
  int* err = device_error_word();
  CB_CHECK_ARG(err != nullptr, CB_E_HIP, "cb_spmm_gemm: the device error word could not be allocated (%s)", cb_last_error());
  CB_CHECK_ARG(*(volatile int*)err == 0, CB_E_DEVICE, "cb_spmm_gemm: an earlier launch recorded a device-side error (%s); results since then are invalid",
               device_error_text());
  gt.err = err;
  FusedEpi fe_hub = fe;      // hub rows first: the main kernel reads their finished rows back
  fe_hub.skip_next = 0;      // (they always go through memory)
  const int rch = launch_hub_rows<4, float, FUSED>(g, h, ld_h, kKD, out, ld_out, ep, fe_hub, st);
  if (rch != CB_OK) return rch;
  const int n_tiles = (int)((g.n_rows + kTM - 1) / kTM);
  const dim3 grid((unsigned)ag_n_blocks(n_tiles)), block(64 * (kNG + 4));
  // the tail: the trunk's store on a subset of the node rows (gt.row_ids; source-row factor in the gathers), the output Linear of <= 64 classes
  // (gt.n_out > 0), or the plain 256 x 256 product
  dispatch_gp_cs<true, false>(ep.col_flags ? 2 : 0, false, [&](auto GP, auto) {
    auto go = [&](auto NARROW, auto SR) {
      hipLaunchKernelGGL((k_agg_gemm2<FUSED, decltype(GP)::value, ACC, decltype(NARROW)::value, decltype(SR)::value>), grid, block, 0, st, g.rowptr, g.col, h, ld_h, out,
                         ld_out, (int)g.n_rows, ep, g.hub_threshold, fe, gt, n_tiles);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if constexpr (!FUSED && !ACC) {
      if (gt.row_ids) return go(no, yes);
    }
    if constexpr (FUSED) {
      if (gt.n_out > 0) return go(yes, no);
    }
    go(no, no);
  });
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb

using namespace cb;

extern "C" int cb_agg_gemm_handover_selftest(void* stream) {
  int* err = device_error_word();
  CB_CHECK_ARG(err != nullptr, CB_E_HIP, "cb_agg_gemm_handover_selftest: the device error word could not be allocated");
  hipLaunchKernelGGL(k_agg_handover_selftest, dim3(1), dim3(64), 0, (hipStream_t)stream, err);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_agg_gemm_image_bytes(int64_t K, int64_t N) {
  if (K != kKD || N != kND) return 0;
  return (size_t)kNS * kNT * 3 * 64 * sizeof(uint4);
}

extern "C" int cb_agg_gemm_image_f32(const float* W, int64_t ld, int64_t K, int64_t N, int transpose, void* image, size_t image_bytes,
                                     void* stream) {
  CB_CHECK_ARG(K == kKD && N == kND, CB_E_INVALID, "cb_agg_gemm_image_f32: the fused dense part is built for 256 x 256 weights (got %lld x %lld)",
               (long long)K, (long long)N);
  CB_CHECK_ARG(W && image && ld >= (transpose ? K : N), CB_E_INVALID, "cb_agg_gemm_image_f32: null pointer / bad leading dimension");
  CB_CHECK_ARG(image_bytes >= cb_agg_gemm_image_bytes(K, N) && aligned16(image), CB_E_WORKSPACE, "cb_agg_gemm_image_f32: image buffer too small or misaligned");
  // B[k][n] = W[k][n] (transpose = 0) or W[n][k] (transpose = 1: the dX contraction multiplies by W^T)
  const int64_t sk = transpose ? 1 : ld, sn = transpose ? ld : 1;
  hipLaunchKernelGGL(k_weight_image, dim3(kNS * kNT * 64 / 256), dim3(256), 0, (hipStream_t)stream, W, sk, sn, (uint4*)image, kNS);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// What every entry of this file asks beyond the graph view (check_csr_view): d == 256, room for the ragged last tile in the int32 row index, the
// weight image and 16-byte aligned rows.  v = the checked view; an empty graph (n_rows == 0) passes and the entry returns.
static int agg_gemm_common_checks(const char* who, const cb_csr_view* g, cb_csr_view& v, int64_t d, const void* h, int64_t ld_h, const void* image,
                                  const float* g_addend, int64_t ld_add, const float* g_out, int64_t ld_gout, const float* acc_init, int64_t ld_init) {
  CB_CHECK_ARG(d == kKD, CB_E_INVALID, "%s: the fused dense part needs d == 256", who);
  const int rc = check_csr_view(who, g, d, v);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG(v.n_rows < INT32_MAX - kTM, CB_E_RANGE, "%s: size exceeds the int32 contract", who);
  CB_CHECK_ARG(h && image && g_out, CB_E_INVALID, "%s: null pointer", who);
  CB_CHECK_ARG(aligned16(h) && ld_h % 4 == 0 && ld_h >= d && aligned16(image) && aligned16(g_out) && ld_gout % 4 == 0 && ld_gout >= kND &&
                   (!g_addend || (aligned16(g_addend) && ld_add % 4 == 0 && ld_add >= kND)) &&
                   (!acc_init || (aligned16(acc_init) && ld_init % 4 == 0 && ld_init >= d)),
               CB_E_INVALID, "%s: 16-byte aligned rows of at least 256 floats required", who);
  return CB_OK;
}

// Plain aggregation (out = act(row_scale * (acc_init + sum) + bias), as cb_spmm_csr_f32) + g_out = g_rowscale * (out @ B) + g_addend, B = the
// 256 x 256 matrix whose fragment image cb_agg_gemm_image_f32 wrote.  acc_init (may be NULL): the partial sums of the earlier passes of a
// node-sharded aggregation ([N, ld_init]); `out` may alias it (a row's partial sums are read before the row is stored, by the same wavefront).
extern "C" int cb_spmm_gemm_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* row_scale, const float* bias, int relu,
                                const float* acc_init, int64_t ld_init, float* out, int64_t ld_out, const void* image, const float* g_rowscale,
                                const float* g_addend, int64_t ld_add, float* g_out, int64_t ld_gout, void* stream) {
  cb_csr_view v;
  const int rc = agg_gemm_common_checks("cb_spmm_gemm_f32", g, v, d, h, ld_h, image, g_addend, ld_add, g_out, ld_gout, acc_init, ld_init);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG(out && aligned16(out) && ld_out % 4 == 0 && ld_out >= d, CB_E_INVALID, "cb_spmm_gemm_f32: 16-byte aligned output rows required");
  Epilogue ep{row_scale, bias, relu, acc_init, ld_init, v.col_flags};
  GemmTail gt{(const uint4*)image, g_rowscale, g_addend, ld_add, g_out, ld_gout};
  if (acc_init) return launch_agg_gemm<false, true>(v, h, ld_h, ep, out, ld_out, (hipStream_t)stream, FusedEpi{}, gt);
  return launch_agg_gemm<false, false>(v, h, ld_h, ep, out, ld_out, (hipStream_t)stream, FusedEpi{}, gt);
}

// The sum-first layer of the rows-only forward (trunk.py _layer_on_rows) in one kernel: out = H = sum_u col_scale[u] * h[u] over each row's edges
// (cb_spmm_csr_f32 with col_scale, stored: the backward's source-side level reads it) and, from the dense tail, the trunk's store on the node rows row_ids
// of H's rows — g_out = dropout(c_act * relu(g_rowscale * (H @ B) + bias) + c_mix * mix_src[mix_index[m] | row_ids[m]]), out_act = the ReLU output,
// relu_bits[row_ids[m]] = its mask words (cb_gemm_nn_store_rows_f32: the same values bit for bit).
extern "C" int cb_spmm_gemm_store_rows_f32(const cb_csr_view* g, const float* h, int64_t ld_h, int64_t d, const float* col_scale, float* out, int64_t ld_out,
                                           const void* image, const float* g_rowscale, const float* bias, const int64_t* row_ids, const cb_trunk_store* store,
                                           float* g_out, int64_t ld_gout, void* stream) {
  const char* who = "cb_spmm_gemm_store_rows_f32";
  cb_csr_view v;
  const int rc = agg_gemm_common_checks(who, g, v, d, h, ld_h, image, nullptr, 0, g_out, ld_gout, nullptr, 0);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG(out && aligned16(out) && ld_out % 4 == 0 && ld_out >= d && col_scale && row_ids, CB_E_INVALID, "%s: null pointer or misaligned rows", who);
  const int rcs = check_trunk_store(who, store, kND);
  if (rcs != CB_OK) return rcs;
  CB_CHECK_ARG(aligned16(store->relu_bits), CB_E_INVALID, "%s: relu_bits must be 16-byte aligned (the mask words leave as 16-byte vectors)", who);
  Epilogue ep{nullptr, nullptr, 0, nullptr, 0, v.col_flags};
  ep.col_scale = col_scale;
  GemmTail gt{(const uint4*)image, g_rowscale, nullptr, 0, g_out, ld_gout};
  gt.bias = bias; gt.row_ids = row_ids; gt.st = make_trunk_store(*store);
  return launch_agg_gemm<false, false>(v, h, ld_h, ep, out, ld_out, (hipStream_t)stream, FusedEpi{}, gt);
}

// Fused trunk store (cb_spmm_csr_fused_f32: ReLU / mix / dropout, mask words, out_next) + g_out = g_rowscale * (out_next @ B) + g_addend.
// skip_next: a forward that no backward follows (evaluation / metrics passes) — the stored activations X_{l+1} have no reader, the next layer's Z
// leaves this kernel, so the rows the persistent kernel finishes stay on chip (out_next: still the hub rows' way into the tile, contents otherwise
// undefined; may be NULL when the plan has no hub rows).  10 GB less written per launch at the headline size.
// n_out > 0: the narrow tail — g_out = logits [N, ld_gout >= n_out]; the common checks see a stand-in leading dimension.
static int spmm_gemm_fused_impl(const char* who, const cb_csr_view* g, const float* acc_init, int64_t ld_init, const float* h, int64_t ld_h, int64_t d,
                                const float* row_scale, const float* bias, const cb_trunk_store* store, float* out_next, int64_t ld_next, int32_t skip_next,
                                const void* image, const float* g_rowscale, const float* g_addend, int64_t ld_add, float* g_out, int64_t ld_gout, void* stream,
                                const float* head_bias = nullptr, int n_out = 0) {
  cb_csr_view v;
  const int rc = agg_gemm_common_checks(who, g, v, d, h, ld_h, image, g_addend, ld_add, g_out, n_out > 0 ? kND : ld_gout, acc_init, ld_init);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG((out_next || (skip_next && v.n_hubs == 0)) && aligned16(out_next) && ld_next % 4 == 0 && ld_next >= d, CB_E_INVALID,
               "%s: 16-byte aligned rows required", who);
  const int rcs = check_trunk_store(who, store, d);
  if (rcs != CB_OK) return rcs;
  CB_CHECK_ARG(!store->mix_index, CB_E_INVALID, "%s: the mix is taken at the node row (no mix_index)", who);
  Epilogue ep{row_scale, bias, 1, acc_init, ld_init, v.col_flags};
  FusedEpi fe{};
  fe.st = make_trunk_store(*store);
  fe.out_next = out_next; fe.ld_next = ld_next; fe.d = (int)d;
  fe.skip_next = skip_next != 0;
  GemmTail gt{(const uint4*)image, g_rowscale, g_addend, ld_add, g_out, ld_gout};
  gt.bias = head_bias; gt.n_out = n_out;
  if (acc_init) return launch_agg_gemm<true, true>(v, h, ld_h, ep, out_next, ld_next, (hipStream_t)stream, fe, gt);
  return launch_agg_gemm<true, false>(v, h, ld_h, ep, out_next, ld_next, (hipStream_t)stream, fe, gt);
}

extern "C" int cb_spmm_gemm_fused_f32(const cb_csr_view* g, const float* acc_init, int64_t ld_init, const float* h, int64_t ld_h, int64_t d,
                                      const float* row_scale, const float* bias, const cb_trunk_store* store, float* out_next, int64_t ld_next,
                                      int32_t skip_next, const void* image, const float* g_rowscale, const float* g_addend, int64_t ld_add, float* g_out,
                                      int64_t ld_gout, void* stream) {
  return spmm_gemm_fused_impl("cb_spmm_gemm_fused_f32", g, acc_init, ld_init, h, ld_h, d, row_scale, bias, store, out_next, ld_next, skip_next, image, g_rowscale,
                              g_addend, ld_add, g_out, ld_gout, stream);
}

// ---- the output Linear as the tail of the LAST layer's aggregation (round 5; GCN.py:133-138: Linear(dropout(X_L)) on the rows the store just made) ----
extern "C" size_t cb_agg_gemm_head_image_bytes(int64_t K, int64_t C) {
  if (K != kKD || C < 1 || C > 32 * kNTn) return 0;
  return (size_t)kNS * kNTn * 3 * 64 * sizeof(uint4);
}

// image of B = W^T for an nn.Linear weight W [C, 256] (transpose = 1) or of B = W [256, C] (transpose = 0); columns C .. 63 are zero
extern "C" int cb_agg_gemm_head_image_f32(const float* W, int64_t ld, int64_t K, int64_t C, int transpose, void* image, size_t image_bytes, void* stream) {
  CB_CHECK_ARG(cb_agg_gemm_head_image_bytes(K, C) > 0, CB_E_INVALID, "cb_agg_gemm_head_image_f32: K must be 256 and 1 <= C <= 64 (got %lld x %lld)", (long long)K,
               (long long)C);
  CB_CHECK_ARG(W && image && ld >= (transpose ? K : C), CB_E_INVALID, "cb_agg_gemm_head_image_f32: null pointer / bad leading dimension");
  CB_CHECK_ARG(image_bytes >= cb_agg_gemm_head_image_bytes(K, C) && aligned16(image), CB_E_WORKSPACE, "cb_agg_gemm_head_image_f32: image buffer too small or misaligned");
  const int64_t sk = transpose ? 1 : ld, sn = transpose ? ld : 1;
  hipLaunchKernelGGL(k_weight_image_narrow, dim3(kNS * kNTn * 64 / 256), dim3(256), 0, (hipStream_t)stream, W, sk, sn, (uint4*)image, kNS, (int)C);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// Fused trunk store of the LAST layer (as cb_spmm_gemm_fused_f32) + logits = out_next @ B + head_bias, B = the 256 x C matrix behind head_image.
// skip_next: the last layer's activations are not written at all (hub rows excepted), only the logits leave.
extern "C" int cb_spmm_gemm_fused_head_f32(const cb_csr_view* g, const float* acc_init, int64_t ld_init, const float* h, int64_t ld_h, int64_t d,
                                           const float* row_scale, const float* bias, const cb_trunk_store* store, float* out_next, int64_t ld_next,
                                           int32_t skip_next, const void* head_image, const float* head_bias, int64_t C, float* logits, int64_t ld_logits,
                                           void* stream) {
  const char* who = "cb_spmm_gemm_fused_head_f32";
  const bool empty = g && g->n_rows == 0;
  CB_CHECK_ARG(C >= 1 && C <= 32 * kNTn && (empty || (logits && ld_logits >= C)), CB_E_INVALID, "%s: 1 <= C <= 64 logits per row expected", who);
  // (the common checks want a 256-wide 16-byte aligned tail output: the narrow tail has its own rule — any ld >= C, float4 stores where ld % 4 == 0)
  CB_CHECK_ARG(empty || aligned16(logits), CB_E_INVALID, "%s: logits must be 16-byte aligned", who);
  return spmm_gemm_fused_impl(who, g, acc_init, ld_init, h, ld_h, d, row_scale, bias, store, out_next, ld_next, skip_next, head_image, nullptr, nullptr, 0, logits,
                              ld_logits, stream, head_bias, (int)C);
}
