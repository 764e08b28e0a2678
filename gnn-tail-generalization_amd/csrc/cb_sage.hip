// One layer of the link-prediction encoders (Link_prediction_model/layer.py:8-35: SAGEConv / GraphConv / GCNConv(normalize=False)) in one kernel:
//     agg[v] = row_scale[v] * sum_{j in row v} col_scale[col[j]] * h[col[j]]                      (the aggregation, rows of 256 fp32)
//     out[v] = epi( [agg[v] | self[v]] @ B + bias )                                               (B: 512 x 256, or 256 x 256 without `self`)
// Forward (by-dst CSR, h = self = X, B = [W_n^T ; W_s^T]) and backward (by-src CSR, h = self = G, B = [W_n ; W_s], agg also stored: the weight
// gradient reads it) are the same launch.  What it spares against aggregation -> GEMM: the write and the read of the aggregated matrix and the
// second read of X, i.e. the `[agg | x]` operand never exists in memory.
//
// Shape of a block: 8 wavefronts, one 64-row tile, three phases kept apart by ONE block barrier (no hand-over through counters, no persistent
// loop, no spin, no atomics, nothing to report in the device error word):
//   1. all eight wavefronts copy their 8 rows of `self` into columns 256..511 of the LDS tile and reduce their share of the tile's rows into columns
//      0..255 — stream_rows of cb_spmm_core.h, the walk and the sums of cb_spmm_csr_f32 (rows cut among the wavefronts at equal edge counts by its
//      tile_row_cut, as in cb_agg_gemm.hip; hub rows are reduced by launch_hub_rows BEFORE this launch and read back from `agg_out`);
//   2. __syncthreads();
//   3. wavefronts 0..3 multiply the 64 x 512 tile by the image (tile_times_image of cb_tile_gemm.h: three bf16 limbs, the six limb products of
//      cb_gemm_nn_f32 in its order, K steps 0..31 in order into the same accumulators) and store through their private C strips.
// The arithmetic is therefore cb_spmm_csr_f32's followed by cb_gemm_nn_f32's on the materialised [agg | self], bit for bit.
//
// LDS: ONE 64 x 516-float tile (132 096 B) + four C strips (8 704 B) = 140 800 B of the CU's 160 KiB, one block per CU.  The alternative — a 64 x 260
// tile re-filled with the self rows after K step 15, 75 KB, two blocks per CU — was not taken: it puts a global-load latency and two more barriers in
// the middle of the K loop of every tile and needs tile_times_image to resume on live accumulators from an image offset (a change to a header three
// other kernels share).  Occupancy of the gather phase comes from the block instead: eight wavefronts (two per SIMD, twelve gathers in flight each)
// reduce the tile, the figure the aggregation + GEMM kernel settled on; the four that multiply afterwards have 256 registers each, which the K
// loop's two-step prefetch ring needs anyway.  Without `self` (GCN) the tile is 64 x 260 and two blocks share a CU.  The choice between the two tile
// forms was made from the guides' LDS / occupancy arithmetic, not from a measurement of both; the layer against the two-kernel form is measured
// (tools/bench_sage.py, profiles/sage.md).
// The kernel and its launch live in cb_sage_core.h, shared with cb_ewlayer.hip (the same layer with a factor per stored edge); this file instantiates the
// sixteen kernels without that factor.
#include "cb_sage_core.h"

using namespace cb;

extern "C" size_t cb_sage_image_bytes(int has_self) { return (size_t)(has_self ? 2 : 1) * kNS * kNT * 3 * 64 * sizeof(uint4); }

extern "C" int cb_sage_image_f32(const float* W_n, int64_t ld_n, const float* W_s, int64_t ld_s, int transpose, void* image, size_t image_bytes, void* stream) {
  CB_CHECK_ARG(W_n && image && ld_n >= kKD && (!W_s || ld_s >= kKD), CB_E_INVALID, "cb_sage_image_f32: null pointer / bad leading dimension (256 x 256 blocks)");
  CB_CHECK_ARG(image_bytes >= cb_sage_image_bytes(W_s != nullptr) && aligned16(image), CB_E_WORKSPACE, "cb_sage_image_f32: image buffer too small or misaligned");
  // B[k][n] = W[k][n] (transpose = 0) or W[n][k] (transpose = 1), W_n's block on top of W_s's: K steps 0..15 and 16..31 of the image
  const float* W[2] = {W_n, W_s};
  const int64_t ld[2] = {ld_n, ld_s};
  for (int b = 0; b < (W_s ? 2 : 1); ++b) {
    const int64_t sk = transpose ? 1 : ld[b], sn = transpose ? ld[b] : 1;
    hipLaunchKernelGGL(k_weight_image, dim3(kNS * kNT * 64 / 256), dim3(256), 0, (hipStream_t)stream, W[b], sk, sn, (uint4*)image + (size_t)b * kNS * kNT * 3 * 64, kNS);
    CB_LAUNCH_CHECK();
  }
  return CB_OK;
}

extern "C" int cb_sage_layer_supported(int64_t d_in, int64_t d_out, int32_t h_bf16, const void* h, int64_t ld_h, const float* self, int64_t ld_self,
                                       const float* agg_out, int64_t ld_agg, const float* out, int64_t ld_out) {
  if (d_in != kKD || d_out != kND || h_bf16 || !h || !out) return 0;
  if (!sage_rows_ok((const float*)h, ld_h) || !sage_rows_ok(out, ld_out)) return 0;
  if (self && !sage_rows_ok(self, ld_self)) return 0;
  if (agg_out && !sage_rows_ok(agg_out, ld_agg)) return 0;
  return 1;
}

extern "C" int cb_sage_layer_f32(const cb_csr_view* g, const float* h, int64_t ld_h, const float* self, int64_t ld_self, const float* col_scale,
                                 const float* row_scale, const void* image, const float* bias, int relu, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                                 int64_t row0, float* agg_out, int64_t ld_agg, int32_t agg_hubs_only, float* out, int64_t ld_out, void* stream) {
  return sage_layer_launch<false>("cb_sage_layer_f32", g, h, ld_h, self, ld_self, col_scale, row_scale, nullptr, image, bias, relu, drop_p, seed, seed_dev, row0,
                                  agg_out, ld_agg, agg_hubs_only, out, ld_out, stream);
}
