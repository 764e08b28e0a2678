// The trunk's fused store (include/coldbrew_hip.h, cb_trunk_store: ReLU, mask words, residual mix, dropout, optional activation output), written once:
// the device-side parameter block every kernel that applies the store embeds, the steps of the store as device functions, and the one host-side check
// and conversion of the ABI struct.  The forms of the store — inside the aggregation (cb_spmm_core.h fused_store), as the epilogue of a dense transform
// (cb_gemm_core.h nn_epilogue EPI == 2), as the tail of the aggregation + GEMM kernel (cb_agg_gemm.hip) and as a row pass (cb_trunk_bwd.hip) — are
// bit-identical because they call these functions, not because they repeat them.
#pragma once
#include "cb_common.h"
#include "cb_philox.h"

namespace cb {

struct TrunkStore {
  const float* mix_src;        // [., ld_mix] or null (no mix)
  int64_t ld_mix;
  const int64_t* mix_index;
  float c_act, c_mix;          // (1 - alpha), alpha
  uint32_t thresh;             // dropout threshold (0 = keep everything)
  float keep_scale;            // 1 / (1 - p)
  uint64_t seed;
  const uint64_t* seed_dev;    // hipGraph mode: per-step seed part in device memory (added to `seed`), or null
  int64_t row0;                // global index of node row 0 (node-sharded runs draw the unsharded mask)
  unsigned long long* bits;    // [node rows][d/256][4] or null
  int bits_relu_only;          // mask words hold (act > 0) alone, not (act > 0 AND kept by this store's dropout): the 'Residual' trunk, whose backward
                               // also sends the NEXT layer's mix gradient through this ReLU (under another dropout mask)
  float* out_act;              // [., ld_act] or null
  int64_t ld_act;
};

__device__ __forceinline__ uint64_t store_seed(const TrunkStore& s) { return s.seed_dev ? s.seed + *s.seed_dev : s.seed; }

// The keep factors (1 / (1 - p) or 0; left as they are without dropout) of columns c .. c + 3 of node row `grow` of a d-wide matrix.
// seed = store_seed(s), for the kernels that load it once; the second form loads it where the mask is drawn.
__device__ __forceinline__ void store_keep4(const TrunkStore& s, uint64_t seed, int64_t grow, int d, int c, float (&m)[4]) {
  if (s.thresh) keep4(seed, ((s.row0 + grow) * d + c) >> 2, s.thresh, s.keep_scale, m);
}
__device__ __forceinline__ void store_keep4(const TrunkStore& s, int64_t grow, int d, int c, float (&m)[4]) {
  if (s.thresh) keep4(store_seed(s), ((s.row0 + grow) * d + c) >> 2, s.thresh, s.keep_scale, m);
}

// The element passes gradient to the pre-activation: ReLU positive AND kept by the dropout.  The backward kernels that also regenerate the keep-mask are
// unaffected (masking twice is masking once).
__device__ __forceinline__ bool store_passes_grad(const TrunkStore& s, float a, float m) { return a > 0.f && (s.bits_relu_only || m != 0.f); }

// Mask words of one 256-column tile row held by ONE wavefront (lane l: columns 4 l .. 4 l + 3): word k, bit l = pass[k] of lane l, i.e. column 4 l + k.
// Every lane of the wavefront calls it; lanes 0 .. 3 write words[0 .. 3].
__device__ __forceinline__ void write_row_mask_words(unsigned long long* __restrict__ words, int lane, const bool (&pass)[4]) {
  unsigned long long mine = 0ull;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long w = __ballot(pass[k]);
    if (lane == k) mine = w;
  }
  if (lane < 4) words[lane] = mine;
}
__device__ __forceinline__ void store_mask_words(const TrunkStore& s, unsigned long long* __restrict__ words, int lane, const float (&a)[4], const float (&m)[4]) {
  const bool pass[4] = {store_passes_grad(s, a[0], m[0]), store_passes_grad(s, a[1], m[1]), store_passes_grad(s, a[2], m[2]), store_passes_grad(s, a[3], m[3])};
  write_row_mask_words(words, lane, pass);
}

// The row of mix_src that stored row r (node row grow) mixes in
__device__ __forceinline__ int64_t store_mix_row(const TrunkStore& s, int64_t r, int64_t grow) { return s.mix_index ? s.mix_index[r] : grow; }

// x = dropout(c_act * a + c_mix * q)  (q: the mix_src row; unread without one).  The keep factor is a multiply of its own: the rounding sequence of
// cb_axpby_f32 followed by cb_dropout_f32.
__device__ __forceinline__ void store_value(const TrunkStore& s, const float (&a)[4], const float (&q)[4], const float (&m)[4], float (&x)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = s.mix_src ? mix2(s.c_act, a[i], s.c_mix, q[i]) : a[i];
  if (s.thresh) {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] *= m[i];
  }
}

static_assert(sizeof(cb_trunk_store) == 96, "cb_trunk_store: the field order of include/coldbrew_hip.h is part of the ABI");

static inline void set_store_dropout(TrunkStore& s, float drop_p) {
  s.thresh = drop_p > 0.f ? dropout_threshold(drop_p) : 0u;
  s.keep_scale = 1.f / (1.f - drop_p);
}

// The store argument of an entry (include/coldbrew_hip.h, cb_trunk_store), checked once for rows of d elements — what every kernel that applies the store
// relies on.  An entry whose kernel asks more (or has no kernel for an option) adds its own condition.
static inline int check_trunk_store(const char* who, const cb_trunk_store* s, int64_t d) {
  CB_CHECK_ARG(s != nullptr, CB_E_INVALID, "%s: the trunk store is null", who);
  CB_CHECK_ARG(s->drop_p >= 0.f && s->drop_p < 1.f && s->row0 >= 0, CB_E_INVALID, "%s: dropout p / row offset of the trunk store out of range", who);
  CB_CHECK_ARG(!s->mix_src || (aligned16(s->mix_src) && s->ld_mix % 4 == 0 && s->ld_mix >= d), CB_E_INVALID,
               "%s: mix_src must be 16-byte aligned rows of at least d floats", who);
  CB_CHECK_ARG(!s->out_act || (aligned16(s->out_act) && s->ld_act % 4 == 0 && s->ld_act >= d), CB_E_INVALID,
               "%s: out_act must be 16-byte aligned rows of at least d floats", who);
  CB_CHECK_ARG((uintptr_t)s->relu_bits % 8 == 0, CB_E_INVALID, "%s: relu_bits must be 8-byte aligned", who);
  return CB_OK;
}

static inline TrunkStore make_trunk_store(const cb_trunk_store& s) {
  TrunkStore t{s.mix_src, s.ld_mix, s.mix_index, s.c_act, s.c_mix, 0u, 1.f, s.seed, s.seed_dev, s.row0, (unsigned long long*)s.relu_bits, s.bits_relu_only, s.out_act, s.ld_act};
  set_store_dropout(t, s.drop_p);
  return t;
}

}  // namespace cb
