// The integer draws and the row search shared by the edge samplers (cb_linkp.hip, cb_lpx.hip): draw number `ctr` gives the four Philox4x32-10 words
// under the 64-bit seed; an integer in [0, n) is the high 64 bits of (r0 << 32 | r1) * n, the draw's second integer comes from (r2, r3).
#pragma once
#include "cb_common.h"
#include "cb_philox.h"

namespace cb {

// the four words of draw `ctr`
__device__ __forceinline__ void lp_words(uint64_t seed, uint64_t ctr, uint32_t (&r)[4]) {
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
}

// the two integers of draw `ctr` in [0, n): multiply-high of 64 random bits (a 32-bit multiply-high is biased by up to n / 2^32)
__device__ __forceinline__ void lp_draw2(uint64_t seed, uint64_t ctr, uint64_t n, uint64_t& a, uint64_t& b) {
  uint32_t r[4];
  lp_words(seed, ctr, r);
  a = __umul64hi(((uint64_t)r[0] << 32) | r[1], n);
  b = __umul64hi(((uint64_t)r[2] << 32) | r[3], n);
}

// is x a column of row `row` of a CSR with ascending columns (duplicates allowed)
__device__ __forceinline__ bool lp_row_has(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int row, int x) {
  int lo = rowptr[row], hi = rowptr[row + 1];
  while (lo < hi) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    const int c = col[mid];
    if (c == x) return true;
    if (c < x) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

}  // namespace cb
