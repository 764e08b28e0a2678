// Launch geometry and the second reduction stage shared by the HBM-bound kernel files (cb_elementwise.hip, cb_trunk_bwd.hip, cb_norms.hip,
// cb_reduce.hip): 256-thread blocks, grid-stride loops capped at 256 CUs x 8 blocks, reductions in a fixed two-stage order (no float atomics ->
// bit-reproducible).
#pragma once
#include "cb_common.h"

namespace cb {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 8;

static inline int grid_for(int64_t work_items) {
  int64_t b = (work_items + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

// Blocks (= partial rows) of a column sum over `rows` rows, one per 64 rows: the size of cb_colsum_workspace_bytes and the grid of every kernel
// that fills it, which have to agree.
static inline int colsum_blocks(int64_t rows) {
  const int64_t nb = (rows + 63) / 64;
  return (int)(nb > kMaxBlocks ? kMaxBlocks : nb);
}

// out[c] = sum_p partial[p][c], p < nb (k_colsum_finish, cb_reduce.hip); CB_OK or CB_E_HIP.  Not part of the library's exported symbols.
__attribute__((visibility("hidden"))) int colsum_finish(const float* partial, int nb, int d, float* out, hipStream_t st);

}  // namespace cb
