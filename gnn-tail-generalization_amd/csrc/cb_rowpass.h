// The row pass shared by the kernels that stream a [rows, d] matrix once and leave fixed-order column sums (cb_trunk_bwd.hip; the slab alone
// also in k_act_bwd and k_colstats): a block owns a slab of consecutive rows; in the wave-per-row kernels (256 threads, d % 256 == 0) wavefront w
// takes the slab's rows w, w + 4, ... and lane l the columns 4l .. 4l+3 of each 256-wide tile — the map of the forward's fused store, so word k of
// a (row, tile)'s four mask words is tested at bit l.  block_colsum below IS the block-level order of every column sum these kernels return;
// k_colsum_finish (cb_reduce.hip) is the second stage, oracle/coldbrew_oracle.py colsum_two_stage the host restatement of both.
#pragma once
#include "cb_common.h"

namespace cb {

constexpr int kRowWaves = 4;      // wavefronts (= rows in flight) of a wave-per-row block

struct RowSlab {
  int64_t begin, end;
};
// rows [begin, end) of this block: ceil(rows / gridDim.x) each, the last blocks ragged or empty
__device__ __forceinline__ RowSlab row_slab(int64_t rows) {
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t begin = (int64_t)blockIdx.x * per;
  return {begin, min(rows, begin + per)};
}

// a lane's four floats of a row that is read once / written once and read by the next kernel: non-temporal
__device__ __forceinline__ void load_quad_nt(const float* __restrict__ p, float (&v)[4]) {
  v[0] = __builtin_nontemporal_load(p); v[1] = __builtin_nontemporal_load(p + 1);
  v[2] = __builtin_nontemporal_load(p + 2); v[3] = __builtin_nontemporal_load(p + 3);
}
__device__ __forceinline__ void store_quad_nt(float* __restrict__ p, float a, float b, float c, float d) {
  typedef float f4_t __attribute__((ext_vector_type(4)));
  const f4_t q = {a, b, c, d};
  __builtin_nontemporal_store(q, reinterpret_cast<f4_t*>(p));
}

// the four mask words of (row, tile); the element of word k this lane owns
__device__ __forceinline__ const unsigned long long* mask_words(const unsigned long long* __restrict__ bits, int64_t row, int tiles, int tile) {
  return bits + (row * tiles + tile) * 4;
}
__device__ __forceinline__ bool word_bit(unsigned long long word, int lane) { return (word >> lane) & 1ull; }

// An operand that may be COMPACT (pos non-null, int32 per node row): node row r sits at row pos[r] of it, absent (zero) where that is negative; a dense
// operand (pos null) holds it at row r.  operand_row: that (wave-uniform) position, 0 for a dense operand.  load_operand_quad: this lane's quad of
// the row — off = r * d + c, where a dense operand is read; an absent row is read at row 0 (a valid address) and zeroed by zero_absent afterwards, so
// the loads of several operands can all be issued before the first of them is waited for.
// A DENSE operand shares g's row indexing: its row for the kernel's row r is r itself, also where g is a row subset (k_trunk_bwd's RIDX form, whose
// entry therefore takes a second gradient only with its position map).
__device__ __forceinline__ int operand_row(const int* __restrict__ pos, int64_t r) { return pos ? __builtin_amdgcn_readfirstlane(pos[r]) : 0; }
__device__ __forceinline__ void load_operand_quad(const float* __restrict__ g, const int* pos, int p, int64_t off, int d, int c, float (&v)[4]) {
  load_quad_nt(g + (pos ? (int64_t)max(p, 0) * d + c : off), v);
}
__device__ __forceinline__ void zero_absent(int p, float (&v)[4]) {
  if (p < 0) v[0] = v[1] = v[2] = v[3] = 0.f;
}

// Column sums of a block over its slab, columns c .. c+3 of this lane: wavefront w's running sums s meet in LDS (s_red: [4 waves][64 lanes][4]) and
// wavefront 0 adds them as (((0 + s_0) + s_1) + s_2) + s_3 into partial[blockIdx.x][c ..].  The closing barrier frees s_red for the next tile pass or
// the next sum.
__device__ __forceinline__ void block_colsum(float* s_red, const float (&s)[4], float* __restrict__ partial, int d, int c, int lane, int w) {
#pragma unroll
  for (int k = 0; k < 4; ++k) s_red[(w * 64 + lane) * 4 + k] = s[k];
  __syncthreads();
  if (w == 0) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < kRowWaves; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] += s_red[(j * 64 + lane) * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) partial[(int64_t)blockIdx.x * d + c + k] = t[k];
  }
  __syncthreads();
}

// A second column sum taken through ANOTHER store's mask words (partial non-null): over the rows, c * dropout_bwd(operand src) where bits (indexed by the
// node row, also for a compact operand) has the element's bit — the bias gradient of the store whose backward left a reverse aggregation's epilogue
// (cb_spmm_csr_store_bwd_f32).
struct SecondColsum {
  int src;
  const unsigned long long* bits;
  float c;
  float* partial;
};
// u: the operand's masked gradient at (r, tile), this lane's four columns
__device__ __forceinline__ void second_colsum_add(const SecondColsum& cs, int64_t r, int tiles, int tile, int lane, const float (&u)[4], float (&s2)[4]) {
  const unsigned long long* bw = mask_words(cs.bits, r, tiles, tile);
#pragma unroll
  for (int k = 0; k < 4; ++k) s2[k] += word_bit(bw[k], lane) ? cs.c * u[k] : 0.f;
}

}  // namespace cb
