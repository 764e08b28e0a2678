// The one-kernel encoder layer (design notes: cb_sage.hip), shared by its two entries: cb_sage.hip (cb_sage_layer_f32: a factor per row and / or per source
// row) and cb_ewlayer.hip (cb_ewlayer_f32: a factor per stored edge — the adjacency with values).  k_sage_layer and the launch that chooses its
// instantiation; each file instantiates only the kernels of its own entry (EW = false / true).
#pragma once
#include "cb_common.h"
#include "cb_limb_core.h"
#include "cb_philox.h"
#include "cb_spmm_core.h"
#include "cb_tile_gemm.h"

namespace cb {

constexpr int kSG = 8;                 // wavefronts of a block (all gather; 0..3 multiply)
constexpr int kSU = 12;                // gathers in flight per wavefront
constexpr int kTLD2 = 2 * kKD + 4;     // floats per row of the [agg | self] tile (516 * 4 = 16 mod 256 bytes, as kTLD)

struct SageArgs {
  const int* rowptr;
  const int* col;
  int n_rows, hub_T;
  const float* h;
  int64_t ld_h;
  const float* self;
  int64_t ld_self;
  const float* col_scale;
  const float* row_scale;
  const float* edge_w;   // EW kernels: one factor per stored edge, in the order of col
  const uint4* image;
  const float* bias;
  int relu;
  uint32_t thresh;       // 0: no dropout
  float keep_scale;
  uint64_t seed;
  const uint64_t* seed_dev;
  int64_t row0;
  float* agg;            // hub rows' way into the tile; WAGG: receives every aggregated row
  int64_t ld_agg;
  float* out;
  int64_t ld_out;
};

template <bool HAS_SELF, bool CS, bool WAGG, int GP, bool EW = false>
__global__ void __launch_bounds__(64 * kSG) k_sage_layer(SageArgs a) {
  constexpr int TLD = HAS_SELF ? kTLD2 : kTLD;
  constexpr int NSTEPS = HAS_SELF ? 2 * kNS : kNS;
  __shared__ __attribute__((aligned(16))) float tile[kTM * TLD];
  __shared__ __attribute__((aligned(16))) float cstrip[4][8 * kCLD];
  const int lane = lane_id(), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r0 = (int)blockIdx.x * kTM;
  const int nrt = min(kTM, a.n_rows - r0);
  const int c0 = lane * 4;
  float* tile_lane = tile + c0;

  // ---- phase 1a: the self rows (8 per wavefront; rows past the matrix are zero) ----
  if constexpr (HAS_SELF) {
    float4 sv[kTM / kSG];
#pragma unroll
    for (int i = 0; i < kTM / kSG; ++i) {
      const int row = wv * (kTM / kSG) + i;
      sv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < nrt) sv[i] = *reinterpret_cast<const float4*>(a.self + (int64_t)(r0 + row) * a.ld_self + c0);
    }
#pragma unroll
    for (int i = 0; i < kTM / kSG; ++i) *reinterpret_cast<float4*>(tile_lane + (wv * (kTM / kSG) + i) * TLD + kKD) = sv[i];
  }

  // ---- phase 1b: the aggregation of this wavefront's rows (tile_row_cut of cb_spmm_core.h: the tile cut at equal edge counts) ----
  {
    const auto blk = load_row_block<true>(a.rowptr, a.row_scale, a.hub_T, r0, nrt);
    const RowCut cut = tile_row_cut<kSG>(blk, nrt, wv);
    const int rb = cut.rb;
    const float bvec[4] = {0.f, 0.f, 0.f, 0.f};
    Epilogue ep{};
    ep.row_scale = a.row_scale;
    ep.col_scale = a.col_scale;
    if constexpr (EW) ep.edge_w = a.edge_w;
    const FusedEpi fe{};
    const float* h_lane = a.h + c0;
    float* out_lane = WAGG ? a.agg + c0 : nullptr;
    int r = cut.ra;
    while (r < rb) {      // maximal hub-free runs of [ra, rb)
      const unsigned long long m = (blk.hubmask >> r) & (rb - r >= 64 ? ~0ull : ((1ull << (rb - r)) - 1ull));
      const int nh = m ? r + (__ffsll((long long)m) - 1) : rb;
      if (nh > r)
        stream_rows<4, kSU, true, false, false, float, GP, TLD, true, CS, false, !WAGG, EW>(r, nh, nrt, blk.my_ptr, blk.my_scale, r0, a.col, h_lane, a.ld_h,
                                                                                             out_lane, a.ld_agg, true, 0, bvec, fe, c0, nullptr, 0, ep, tile_lane,
                                                                                             blk.ptr_hi);
      if (nh < rb)        // hub row nh: finished by the hub kernels, which ran before this launch
        *reinterpret_cast<float4*>(tile_lane + nh * TLD) = *reinterpret_cast<const float4*>(a.agg + (int64_t)(r0 + nh) * a.ld_agg + c0);
      r = nh + 1;
    }
    if (wv == kSG - 1) zero_tile_rows<TLD>(tile_lane, nrt, kTM);
  }
  __syncthreads();

  // ---- phase 2: [agg | self] @ B on the matrix cores, epilogue, store ----
  if (wv < 4) {
    f32x16 acc[2][2];
    tile_times_image<NSTEPS, TLD, 2>(tile, a.image, wv, lane, acc);
    const int nl = 64 * wv + (lane & 15) * 4;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) {
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = a.bias[nl + e];
    }
    const uint64_t seed_eff = a.seed_dev ? a.seed + *a.seed_dev : a.seed;
    acc_rows_through_strip(acc, cstrip[wv], wv, lane, [&](int mt, int n, const float4& v) {
      if (mt >= nrt) return;
      const int64_t m = r0 + mt;
      float o[4] = {v.x, v.y, v.z, v.w};
      const float rs = 1.f, ad = 0.f;      // (cb_gemm_core.h nn_epilogue's expression: o * rowscale + addend + bias, then the ReLU)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = o[e] * rs + ad + bv[e];
        if (a.relu) o[e] = relu_nan(o[e]);
      }
      if (a.thresh) {                      // cb_dropout_f32's keep-mask for (seed, flat index (row0 + m) * 256 + n)
        float mk[4];
        keep4(seed_eff, ((a.row0 + m) * kND + n) >> 2, a.thresh, a.keep_scale, mk);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] * mk[e];
      }
      store_stream<4>(a.out + m * a.ld_out + n, o);
    });
  }
}

static inline bool sage_rows_ok(const float* p, int64_t ld) { return aligned16(p) && ld % 4 == 0 && ld >= kKD; }

// The checks and the two launches of a layer entry: the hub rows (launch_hub_rows, before the layer kernel reads them back), then k_sage_layer.
// EW = false: col_scale / row_scale (either may be null), edge_w unused.  EW = true: edge_w alone.
template <bool EW>
static int sage_layer_launch(const char* who, const cb_csr_view* g, const float* h, int64_t ld_h, const float* self, int64_t ld_self, const float* col_scale,
                             const float* row_scale, const float* edge_w, const void* image, const float* bias, int relu, float drop_p, uint64_t seed,
                             const uint64_t* seed_dev, int64_t row0, float* agg_out, int64_t ld_agg, int32_t agg_hubs_only, float* out, int64_t ld_out,
                             void* stream) {
  cb_csr_view v;
  const int rc = check_csr_view(who, g, kKD, v);
  if (rc != CB_OK || v.n_rows == 0) return rc;
  CB_CHECK_ARG(v.n_rows < INT32_MAX - kTM, CB_E_RANGE, "%s: size exceeds the int32 contract", who);
  CB_CHECK_ARG(h && image && out && aligned16(image), CB_E_INVALID, "%s: null pointer or misaligned image", who);
  CB_CHECK_ARG(!EW || edge_w || v.n_edges == 0, CB_E_INVALID, "%s: the edge values are null", who);
  CB_CHECK_ARG(cb_sage_layer_supported(kKD, kND, 0, h, ld_h, self, ld_self, agg_out, ld_agg, out, ld_out), CB_E_INVALID,
               "%s: 16-byte aligned fp32 rows of at least 256 floats (ld %% 4 == 0) required; ask cb_sage_layer_supported first", who);
  CB_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && row0 >= 0 && (drop_p == 0.f || relu), CB_E_INVALID, "%s: dropout follows the ReLU, 0 <= p < 1", who);
  CB_CHECK_ARG(agg_out || (v.n_hubs == 0 && !agg_hubs_only), CB_E_INVALID, "%s: a plan with hub rows needs agg_out (the hub rows' way into the tile)", who);
  hipStream_t st = (hipStream_t)stream;
  const bool cs = !EW && col_scale != nullptr, wagg = agg_out && !agg_hubs_only;
  {      // hub rows first: the layer kernel reads their finished rows back (cb_spmm_csr_f32's hub kernels, its sums)
    Epilogue ep{};
    ep.row_scale = row_scale;
    ep.col_scale = col_scale;
    ep.col_flags = v.col_flags;
    ep.edge_w = edge_w;
    const int rch = launch_hub_rows<4, float, false, false, EW>(v, h, ld_h, kKD, agg_out, ld_agg, ep, FusedEpi{}, st);
    if (rch != CB_OK) return rch;
  }
  SageArgs a{};
  a.rowptr = v.rowptr; a.col = v.col; a.n_rows = (int)v.n_rows; a.hub_T = v.hub_threshold;
  a.h = h; a.ld_h = ld_h; a.self = self; a.ld_self = ld_self; a.col_scale = col_scale; a.row_scale = row_scale; a.edge_w = edge_w;
  a.image = (const uint4*)image; a.bias = bias; a.relu = relu;
  a.thresh = drop_p > 0.f ? dropout_threshold(drop_p) : 0u; a.keep_scale = 1.f / (1.f - drop_p);
  a.seed = seed; a.seed_dev = seed_dev; a.row0 = row0;
  a.agg = agg_out; a.ld_agg = ld_agg; a.out = out; a.ld_out = ld_out;
  const dim3 grid((unsigned)((v.n_rows + kTM - 1) / kTM));
  dispatch_gp_cs<true, !EW>(v.col_flags ? 2 : 0, cs, [&](auto GP, auto CS) {
    dispatch_bool(self != nullptr, [&](auto HAS_SELF) {
      dispatch_bool(wagg, [&](auto WAGG) {
        hipLaunchKernelGGL((k_sage_layer<decltype(HAS_SELF)::value, decltype(CS)::value, decltype(WAGG)::value, decltype(GP)::value, EW>), grid, dim3(64 * kSG), 0,
                           st, a);
      });
    });
  });
  CB_LAUNCH_CHECK();
  return CB_OK;
}

}  // namespace cb
