// GraphMLP's neighbour-contrastive loss (MLP_model/__init__.py:190-208 `get_neighbor_contrastive_loss` + `cosine_sim`, with
// utils.py:1250-1276 `crop_adj_to_subgraph` for the batch) without any B x B matrix in the forward.  The reference builds, per step,
//     simz = (1 - I) * exp(cos(z) / tau)                    [B, B]   (:191-192)
//     adjb = crop(adj_pow, batch_idx).to_dense()            [B, B]   (:193)
//     num  = (adjb * simz).sum(1);  den = simz.sum(1)                (:194-195)
//     loss = -mean(log(num / den)[num != 0])                         (:196-197)
// Here: den is the Gram sweep of cb_topk.hip (128 x 128 MFMA score tiles, never written) with a row-sum epilogue; num walks the rows of
// the sparse power and evaluates only the pairs that exist; one block finishes the loss in a fixed order.  The backward
//     dzh_i = sum_{j != i} s_ij (w_i + w_j) zh_j - sum_j a_ij s_ij u_i zh_j - sum_j a_ji s_ji u_j zh_j,   zh = z / |z|, s = exp(cos / tau)
//     dz_i  = g (dzh_i - <dzh_i, zh_i> zh_i) / |z_i|
// takes its dense term from the same sweep with a store epilogue (P = s (w_i + w_j) for a slab of rows; the caller multiplies the slab by
// ZH on the GEMM) and its two sparse terms from the CSR and the CSC of the power, one wavefront per batch row, rows written by their owner.
// Batches drawn with replacement: the LAST position of a node represents it (what `n_idx[subset] = arange(B)`, utils.py:1261, leaves on the
// CPU); the other positions have an empty adjacency row and column, so num = 0 there.
// cos_ij = <z_i, z_j> * (rinv_i * rinv_j) everywhere in this file: the product of the two scales is symmetric, so s_ij == s_ji bit for bit within the
// sweep (fp32) and within the sparse walks (float64 per pair, see nc_sim_pair).
// Bound: MFMA (2 B^2 D flop per sweep, x6 bf16 passes on the limb core).  No float atomics: two calls give the same bits.
#include <stdlib.h>

#include "cb_common.h"
#include "cb_gemm_core.h"
#include "cb_limb_core.h"

namespace cb {

// ---- positions ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nc_fill_i32(int32_t* __restrict__ p, int64_t n, int32_t v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void __launch_bounds__(256) k_nc_pos_max(const int64_t* __restrict__ batch_idx, int64_t B, int64_t n, int32_t* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const int64_t id = batch_idx[i];
  if (id >= 0 && id < n) atomicMax(&pos[id], (int)i);      // integer max: the result does not depend on the order of arrival
}

__global__ void __launch_bounds__(256) k_nc_rep(const int64_t* __restrict__ batch_idx, int64_t B, int64_t n, const int32_t* __restrict__ pos,
                                                int32_t* __restrict__ rep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const int64_t id = batch_idx[i];
  rep[i] = (id >= 0 && id < n && pos[id] == (int)i) ? 1 : 0;
}

// ---- row kernels: one wavefront per row -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nc_row_norms(const float* __restrict__ x, int64_t ldx, int64_t rows, int D, float* __restrict__ nrm,
                                                      float* __restrict__ rinv) {
  const int lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (r >= rows) return;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float v = x[r * ldx + c];
    s = fmaf(v, v, s);
  }
  s = wave_sum(s);
  if (lane == 0) {
    const float nr = sqrtf(s);
    if (nrm) nrm[r] = nr;
    if (rinv) rinv[r] = 1.f / nr;      // a zero row: inf, NaN downstream — as the reference's x_sum ** (-1) (:207)
  }
}

__global__ void __launch_bounds__(256) k_nc_normalize(const float* __restrict__ z, int64_t ldz, int64_t B, int D, const float* __restrict__ rinv,
                                                      float* __restrict__ zhat) {
  const int lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (r >= B) return;
  const float ri = rinv[r];
  for (int c = lane; c < D; c += 64) zhat[r * D + c] = z[r * ldz + c] * ri;
}

__global__ void __launch_bounds__(256) k_nc_cosine_scale(float* __restrict__ s, int64_t lds_, int64_t N, const float* __restrict__ nrm) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= N) return;
  s[i * lds_ + j] = s[i * lds_ + j] * (1.f / (nrm[i] * nrm[j]));      // x_dis * (x_sum ** (-1)), x_sum = |x_i| |x_j|  (:204-207)
}

__device__ __forceinline__ float nc_sim(float dot, float ri, float rj, float tau) { return expf(dot * (ri * rj) / tau); }

// ---- the sweep's epilogues ------------------------------------------------------------------------------------------------------------
// accumulator layout of both cores (cb_topk.hip fold_filtered): acc[ti][tj][4 q4 + r4] = tile row wr*64 + ti*32 + 8 q4 + 4 (lane >> 5) + r4,
// tile column wc*64 + tj*32 + (lane & 31).
enum { NC_ROWSUM = 0, NC_STORE = 1 };

struct NcSweep {
  const float* rinv;      // [B]
  const float* w;         // [B]   (NC_STORE)
  float tau;
  float* partial;         // [n_splits][B]   (NC_ROWSUM)
  float* P;               // [row_end - row0][ldp]   (NC_STORE)
  int64_t ldp, row0, row_end;
};

// One 128 x 128 tile, NC_ROWSUM: the tile's row sums are reduced over the 32 lanes that share a row and added to s_rs[wc][row] by the one lane
// that owns that cell (no atomics; tiles arrive in ascending order).  Running sums kept in registers instead would stay live across the K loop,
// which has none to spare.
__device__ __forceinline__ void nc_tile_rowsum(const f32x16 (&acc)[2][2], float (*s_rs)[128], const float* __restrict__ s_ri, const NcSweep& a, int64_t m0,
                                               int n0, int64_t B, int t) {
  const int lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1, l31 = lane & 31, lh = lane >> 5;
  const int64_t col0 = (int64_t)n0 + wc * 64 + l31, col1 = col0 + 32;
  const bool cin0 = col0 < B, cin1 = col1 < B;
  const float rj0 = cin0 ? a.rinv[col0] : 0.f, rj1 = cin1 ? a.rinv[col1] : 0.f;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int reg = 4 * q4 + r4;
        const int rl = wr * 64 + ti * 32 + 8 * q4 + 4 * lh + r4;
        const int64_t row = m0 + rl;
        const float ri = s_ri[rl];
        const float s0 = nc_sim(acc[ti][0][reg], ri, rj0, a.tau), s1 = nc_sim(acc[ti][1][reg], ri, rj1, a.tau);
        float v = ((cin0 && col0 != row) ? s0 : 0.f) + ((cin1 && col1 != row) ? s1 : 0.f);
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (l31 == 0) s_rs[wc][rl] += v;
      }
      __builtin_amdgcn_sched_barrier(0);      // (keeps the 64 exponentials of a tile from being scheduled all at once: registers)
    }
  }
}

// One 128 x 128 tile, NC_STORE: 32 tile rows at a time are staged in LDS (cb_topk.hip fold_tile's staging; Cs is the K loop's memory, free after
// its last barrier), then every wavefront writes 8 of them, 64 consecutive columns per store.
__device__ __forceinline__ void nc_tile_store(const f32x16 (&acc)[2][2], float* __restrict__ Cs, const float* __restrict__ s_ri, const float* __restrict__ s_wi,
                                              const NcSweep& a, int64_t m0, int n0, int64_t B, int t) {
  constexpr int LDC = 128 + 4;
  const int lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1, l31 = lane & 31, lh = lane >> 5;
  const int64_t col0 = (int64_t)n0 + lane, col1 = col0 + 64;
  const bool cin0 = col0 < B, cin1 = col1 < B;
  const float rj0 = cin0 ? a.rinv[col0] : 0.f, rj1 = cin1 ? a.rinv[col1] : 0.f;
  const float wj0 = cin0 ? a.w[col0] : 0.f, wj1 = cin1 ? a.w[col1] : 0.f;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll 1
  for (int wr_sel = 0; wr_sel < 2; ++wr_sel) {
    if (wr == wr_sel) {
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
          Cs[((reg & 3) + 8 * (reg >> 2) + 4 * lh) * LDC + wc * 64 + tj * 32 + l31] = acc[ti][tj][reg];
    }
    __syncthreads();
#pragma unroll 1
    for (int rr = 0; rr < 8; ++rr) {
      const int r32 = w * 8 + rr, rl = wr_sel * 64 + ti * 32 + r32;
      const int64_t row = m0 + rl;
      if (row < a.row_end) {      // (wave-uniform)
        const float ri = s_ri[rl], wi = s_wi[rl];
        float* pr = a.P + (row - a.row0) * a.ldp;
        if (cin0) pr[col0] = (col0 != row) ? nc_sim(Cs[r32 * LDC + lane], ri, rj0, a.tau) * (wi + wj0) : 0.f;
        if (cin1) pr[col1] = (col1 != row) ? nc_sim(Cs[r32 * LDC + 64 + lane], ri, rj1, a.tau) * (wi + wj1) : 0.f;
      }
    }
    __syncthreads();
  }
}

template <int MODE>
__device__ __forceinline__ void nc_tile(const f32x16 (&acc)[2][2], float* __restrict__ Cs, float (*s_rs)[128], const float* __restrict__ s_ri,
                                        const float* __restrict__ s_wi, const NcSweep& a, int64_t m0, int n0, int64_t B, int t) {
  if (MODE == NC_ROWSUM) nc_tile_rowsum(acc, s_rs, s_ri, a, m0, n0, B, t);
  else nc_tile_store(acc, Cs, s_ri, s_wi, a, m0, n0, B, t);
}

// the block's row sums -> partial[split][row]: the two wavefronts of a row in a fixed order
__device__ __forceinline__ void nc_rowsum_out(float (*s_rs)[128], const NcSweep& a, int64_t m0, int64_t B, int split, int t) {
  __syncthreads();
  if (t < 128 && m0 + t < B) a.partial[(int64_t)split * B + m0 + t] = s_rs[0][t] + s_rs[1][t];
}

// Z x Z^T on the three-limb core (k_topk_scores_l3's sweep): both operands are k-contiguous "row" operands.
template <int MODE>
__global__ void __launch_bounds__(256, 2) k_nc_sweep_l3(const float* __restrict__ Z, int64_t ldz, int64_t B, int D, int tiles_per_split,
                                                        int n_col_tiles, NcSweep a) {
  using OA = RowOperand<128>;
  using OB = RowOperand<128>;
  constexpr int BM = 128, BN = 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * (OA::BYTES + OB::BYTES)];
  static_assert(32 * (BN + 4) * 4 <= 2 * (OA::BYTES + OB::BYTES), "store staging must fit");
  __shared__ float s_ri[BM], s_wi[BM];
  __shared__ float s_rs[2][128];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int64_t m0 = a.row0 + (int64_t)blockIdx.x * BM;
  const int split = blockIdx.y;
  if (t < BM) {
    const bool in = m0 + t < B;
    s_ri[t] = in ? a.rinv[m0 + t] : 0.f;
    s_wi[t] = (MODE == NC_STORE && in) ? a.w[m0 + t] : 0.f;
    s_rs[0][t] = s_rs[1][t] = 0.f;
  }
  __syncthreads();
  OA oa;
  oa.init(ldz, B - m0, t);
  const uint32_t aaddr[2] = {OA::frag_addr(wr * 64, lane), OA::frag_addr(wr * 64 + 32, lane)};
  const uint32_t baddr[2] = {OB::frag_addr(wc * 64, lane), OB::frag_addr(wc * 64 + 32, lane)};
  const int ct_begin = split * tiles_per_split, ct_end = min(n_col_tiles, ct_begin + tiles_per_split);
  for (int ct = ct_begin; ct < ct_end; ++ct) {
    const int n0 = ct * BN;
    OB ob;
    ob.init(ldz, B - n0, t);
    f32x16 acc[2][2];
    zero_acc_n<2>(acc);
    limb_k_loop<2, 1, OA, OB>(oa, ob, smem, Z + m0 * ldz, KS, ldz, Z + (int64_t)n0 * ldz, KS, ldz, nullptr, D, aaddr, baddr, acc, t);
    nc_tile<MODE>(acc, reinterpret_cast<float*>(smem), s_rs, s_ri, s_wi, a, m0, n0, B, t);
  }
  if (MODE == NC_ROWSUM) nc_rowsum_out(s_rs, a, m0, B, split, t);
}

// ... and on the fp32-input MFMA core (k_topk_scores' sweep) for operands without float4 access
template <int MODE>
__global__ void __launch_bounds__(256) k_nc_sweep_f32(const float* __restrict__ Z, int64_t ldz, int64_t B, int D, int tiles_per_split,
                                                      int n_col_tiles, NcSweep a, int aligned) {
  using TL = Tile<2, 2, BK, 2>;
  constexpr int BM = TL::BM, BN = TL::BN;
  static_assert(BM == 128 && BN == 128 && 32 * (BN + 4) <= TL::SMEM_FLOATS, "epilogue layout; store staging must fit");
  __shared__ __attribute__((aligned(16))) float smem[TL::SMEM_FLOATS];
  __shared__ float s_ri[BM], s_wi[BM];
  __shared__ float s_rs[2][128];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int64_t m0 = a.row0 + (int64_t)blockIdx.x * BM;
  const int split = blockIdx.y;
  if (t < BM) {
    const bool in = m0 + t < B;
    s_ri[t] = in ? a.rinv[m0 + t] : 0.f;
    s_wi[t] = (MODE == NC_STORE && in) ? a.w[m0 + t] : 0.f;
    s_rs[0][t] = s_rs[1][t] = 0.f;
  }
  __syncthreads();
  const int ct_begin = split * tiles_per_split, ct_end = min(n_col_tiles, ct_begin + tiles_per_split);
  const int N = (int)B;
  for (int ct = ct_begin; ct < ct_end; ++ct) {
    const int n0 = ct * BN;
    f32x16 acc[2][2];
    zero_acc<2>(acc);
    rowrow_tile_k_loop<TL>(Z, ldz, m0, B, Z, ldz, n0, N, D, aligned, smem, wr, wc, lane, t, acc);
    nc_tile<MODE>(acc, reinterpret_cast<float*>(smem), s_rs, s_ri, s_wi, a, m0, n0, B, t);
  }
  if (MODE == NC_ROWSUM) nc_rowsum_out(s_rs, a, m0, B, split, t);
}

// ---- sparse walks: one wavefront per batch row ----------------------------------------------------------------------------------------
// The pairs of the sparse walks are few next to the sweep's B^2, but a row of the power can hold hundreds of batch nodes, and the walk adds them one
// after the other: in fp32 that chain alone put num rows 5e-7 off in relative terms (measured at 257 distinct batch nodes; torch's tree-shaped row sum:
// 1.5e-7), whether a pair was evaluated in fp32 or not.  So the walks work in float64 — dot product, scaling, exponential, running sums — and round
// to fp32 once per output element; a numerator of one or two terms is then exact to half an ulp too.
__device__ __forceinline__ double nc_dot(const float* __restrict__ zi, const float* __restrict__ zj, int D, int lane) {
  double s = 0.0;
  for (int c = lane; c < D; c += 64) s = fma((double)zi[c], (double)zj[c], s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);      // fixed-order butterfly, every lane gets the sum
  return s;
}
__device__ __forceinline__ double nc_sim_pair(double dot, float ri, float rj, float tau) {
  return exp(dot * ((double)ri * (double)rj) / (double)tau);
}

// Entries e of [beg, end) whose column is a batch node (p = pos[col[e]] >= 0, p != i), in the order of the row: 4 x 64 entries are looked up at a
// time (the four col / val loads are issued before the four dependent pos loads: a hub row of the power is a chain of such round trips, and one
// at a time left the wavefront of the longest row waiting on latency alone), the hits are then taken one after the other by the whole wavefront.
// f(p, a) is wave-uniform.
template <class F>
__device__ __forceinline__ void nc_walk(const int32_t* __restrict__ col, const float* __restrict__ val, int beg, int end,
                                        const int32_t* __restrict__ pos, int64_t n, int i, int lane, F f) {
  constexpr int U = 4;
  for (int e0 = beg; e0 < end; e0 += 64 * U) {
    int v[U], p[U];
    float av[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int e = e0 + 64 * k + lane;
      const bool in = e < end;
      v[k] = in ? col[e] : -1;
      av[k] = in ? val[e] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      p[k] = (v[k] >= 0 && v[k] < n) ? pos[v[k]] : -1;
      if (p[k] == i) p[k] = -1;      // the diagonal of simz is masked (:191-192)
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      unsigned long long m = __ballot(p[k] >= 0);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        f(__shfl(p[k], l), __shfl(av[k], l));
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_nc_num(const float* __restrict__ z, int64_t ldz, int64_t B, int D, float tau, const float* __restrict__ rinv,
                                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ val,
                                                int64_t n, const int64_t* __restrict__ batch_idx, const int32_t* __restrict__ pos,
                                                const int32_t* __restrict__ rep, float* __restrict__ num) {
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (i >= B) return;
  double acc = 0.0;
  if (rep[i]) {      // (rep implies 0 <= batch_idx[i] < n)
    const int64_t node = batch_idx[i];
    const float ri = rinv[i];
    const float* zi = z + i * ldz;
    nc_walk(col, val, rowptr[node], rowptr[node + 1], pos, n, (int)i, lane, [&](int p, float av) {
      acc = fma((double)av, nc_sim_pair(nc_dot(zi, z + (int64_t)p * ldz, D, lane), ri, rinv[p], tau), acc);
    });
  }
  if (lane == 0) num[i] = (float)acc;
}

// den = the splits' partial sums in ascending order; M = #{num != 0}; loss = -(1 / M) sum log(num / den) over those rows; the backward's row weights.
// One block: every sum in a fixed order (thread-strided partial sums, then a binary tree over the 256 threads).
__global__ void __launch_bounds__(256) k_nc_finish(const float* __restrict__ partial, int n_splits, int64_t B, float tau, const float* __restrict__ num,
                                                   float* __restrict__ den, float* __restrict__ w, float* __restrict__ u, float* __restrict__ loss,
                                                   int32_t* __restrict__ m_count) {
  __shared__ float s_sum[256];
  __shared__ int s_cnt[256];
  const int t = threadIdx.x;
  float sum = 0.f;
  int cnt = 0;
  for (int64_t i = t; i < B; i += 256) {
    float d = 0.f;
    for (int s = 0; s < n_splits; ++s) d += partial[(int64_t)s * B + i];
    den[i] = d;
    const float nu = num[i];
    if (nu != 0.f) {      // (true for NaN, as torch.where(numerator != 0) is: a NaN row makes the loss NaN)
      cnt += 1;
      sum += logf(nu / d);
    }
  }
  s_sum[t] = sum;
  s_cnt[t] = cnt;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) {
      s_sum[t] += s_sum[t + off];
      s_cnt[t] += s_cnt[t + off];
    }
    __syncthreads();
  }
  const int M = s_cnt[0];
  if (t == 0) {
    loss[0] = -(s_sum[0] / (float)M);      // M == 0: 0 / 0 = NaN, the reference's mean of an empty tensor
    m_count[0] = M;
  }
  const float mt = (float)M * tau;
  for (int64_t i = t; i < B; i += 256) {      // (den[i] was written by this very thread)
    const float nu = num[i];
    const bool nz = nu != 0.f;
    w[i] = nz ? 1.f / (mt * den[i]) : 0.f;
    u[i] = nz ? 1.f / (mt * nu) : 0.f;
  }
}

// dzh (in: the dense term P @ ZH; out: the whole dzh) and dz for row i.  Columns in chunks of 256 (four per lane); widths above 256 walk the
// sparse rows once per chunk.
__global__ void __launch_bounds__(256) k_nc_bwd_finish(const float* __restrict__ z, int64_t ldz, const float* __restrict__ zhat, int64_t B, int D, float tau,
                                                       const float* __restrict__ rinv, const float* __restrict__ u, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col, const float* __restrict__ val, const int32_t* __restrict__ rowptr_t,
                                                       const int32_t* __restrict__ col_t, const float* __restrict__ val_t, int64_t n,
                                                       const int64_t* __restrict__ batch_idx, const int32_t* __restrict__ pos, const int32_t* __restrict__ rep,
                                                       const float* __restrict__ g, float* __restrict__ dzh, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (i >= B) return;
  const float ri = rinv[i];
  const float* zi = z + i * ldz;
  const float* zhi = zhat + i * D;
  float* di = dzh + i * D;
  const bool is_rep = rep[i] != 0;
  const int64_t node = is_rep ? batch_idx[i] : 0;
  const float ui = u[i];
  float proj = 0.f;
  for (int c0 = 0; c0 < D; c0 += 256) {
    double acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + lane + 64 * k;
      acc[k] = c < D ? (double)di[c] : 0.0;
    }
    if (is_rep) {
      auto take = [&](int p, double coef) {
        const float* zhp = zhat + (int64_t)p * D;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + lane + 64 * k;
          if (c < D) acc[k] = fma(-coef, (double)zhp[c], acc[k]);
        }
      };
      nc_walk(col, val, rowptr[node], rowptr[node + 1], pos, n, (int)i, lane, [&](int p, float av) {          // - a_ij s_ij u_i zh_j
        take(p, av * nc_sim_pair(nc_dot(zi, z + (int64_t)p * ldz, D, lane), ri, rinv[p], tau) * ui);
      });
      nc_walk(col_t, val_t, rowptr_t[node], rowptr_t[node + 1], pos, n, (int)i, lane, [&](int p, float av) {  // - a_ji s_ji u_j zh_j
        take(p, av * nc_sim_pair(nc_dot(zi, z + (int64_t)p * ldz, D, lane), ri, rinv[p], tau) * u[p]);
      });
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + lane + 64 * k;
      if (c < D) {
        const float d = (float)acc[k];
        di[c] = d;
        proj = fmaf(d, zhi[c], proj);
      }
    }
  }
  proj = wave_sum(proj);
  const float gv = g[0];
  for (int c = lane; c < D; c += 64) dz[i * D + c] = gv * (di[c] - proj * zhi[c]) * ri;      // (di[c] was written by this very lane)
}

// column splits of the sweep: cb_topk.hip's rule (about four blocks per CU), capped by the caller
static void nc_geometry(int64_t rows, int64_t B, int max_splits, int& n_row_blocks, int& n_col_tiles, int& n_splits, int& tiles_per_split) {
  n_row_blocks = (int)((rows + 127) / 128);
  n_col_tiles = (int)((B + 127) / 128);
  int want = (1024 + n_row_blocks - 1) / n_row_blocks;
  if (want < 1) want = 1;
  if (want > n_col_tiles) want = n_col_tiles;
  if (want > 256) want = 256;
  if (max_splits > 0 && want > max_splits) want = max_splits;
  tiles_per_split = (n_col_tiles + want - 1) / want;
  n_splits = (n_col_tiles + tiles_per_split - 1) / tiles_per_split;
}

static bool nc_limb(const float* z, int64_t ldz, int64_t D) {
  static const bool plain = getenv("CB_GEMM_PLAIN_F32") != nullptr;
  return aligned16(z) && ldz % 4 == 0 && !plain && D % 4 == 0 && ldz < (1 << 22);
}

template <int MODE>
static void nc_launch_sweep(const float* z, int64_t ldz, int64_t B, int64_t D, int rb, int ns, int tps, int ctl, const NcSweep& a, hipStream_t st) {
  if (nc_limb(z, ldz, D))
    hipLaunchKernelGGL(k_nc_sweep_l3<MODE>, dim3((unsigned)rb, (unsigned)ns), dim3(256), 0, st, z, ldz, B, (int)D, tps, ctl, a);
  else
    hipLaunchKernelGGL(k_nc_sweep_f32<MODE>, dim3((unsigned)rb, (unsigned)ns), dim3(256), 0, st, z, ldz, B, (int)D, tps, ctl, a,
                       (int)(aligned16(z) && ldz % 4 == 0));
}

}  // namespace cb

using namespace cb;

#define NC_CHECK_SIZES(name)                                                                                           \
  CB_CHECK_ARG(B >= 0 && D > 0 && ldz >= D, CB_E_INVALID, name ": bad size (B >= 0, D > 0, ldz >= D required)");       \
  CB_CHECK_ARG(B < INT32_MAX - 128 && D < (1 << 24), CB_E_RANGE, name ": size out of range")

extern "C" int cb_ncloss_uses_limb_core(const float* z, int64_t ldz, int64_t D) { return nc_limb(z, ldz, D) ? 1 : 0; }

extern "C" int cb_ncloss_positions_i64(const int64_t* batch_idx, int64_t B, int64_t n, int32_t* pos, int32_t* rep, void* stream) {
  CB_CHECK_ARG(B >= 0 && n > 0, CB_E_INVALID, "cb_ncloss_positions_i64: bad size (B >= 0, n > 0 required)");
  CB_CHECK_ARG(B < INT32_MAX - 128 && n < INT32_MAX, CB_E_RANGE, "cb_ncloss_positions_i64: size out of range");
  CB_CHECK_ARG(pos && (B == 0 || (batch_idx && rep)), CB_E_INVALID, "cb_ncloss_positions_i64: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_nc_fill_i32, dim3((unsigned)blocks_for(n, 256)), dim3(256), 0, st, pos, n, -1);
  CB_LAUNCH_CHECK();
  if (B == 0) return CB_OK;
  hipLaunchKernelGGL(k_nc_pos_max, dim3((unsigned)blocks_for(B, 256)), dim3(256), 0, st, batch_idx, B, n, pos);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nc_rep, dim3((unsigned)blocks_for(B, 256)), dim3(256), 0, st, batch_idx, B, n, (const int32_t*)pos, rep);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_ncloss_row_norms_f32(const float* x, int64_t ldx, int64_t rows, int64_t D, float* nrm, float* rinv, void* stream) {
  CB_CHECK_ARG(rows >= 0 && D > 0 && ldx >= D, CB_E_INVALID, "cb_ncloss_row_norms_f32: bad size (rows >= 0, D > 0, ldx >= D required)");
  CB_CHECK_ARG(rows < INT32_MAX && D < (1 << 24), CB_E_RANGE, "cb_ncloss_row_norms_f32: size out of range");
  if (rows == 0) return CB_OK;
  CB_CHECK_ARG(x && (nrm || rinv), CB_E_INVALID, "cb_ncloss_row_norms_f32: null pointer");
  hipLaunchKernelGGL(k_nc_row_norms, dim3((unsigned)blocks_for(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, rows, (int)D, nrm, rinv);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_cosine_scale_f32(float* s, int64_t ld, int64_t N, const float* nrm, void* stream) {
  CB_CHECK_ARG(N >= 0 && ld >= N, CB_E_INVALID, "cb_cosine_scale_f32: bad size (N >= 0, ld >= N required)");
  CB_CHECK_ARG(N < 65536, CB_E_RANGE, "cb_cosine_scale_f32: N < 65536 required (one grid row per matrix row)");
  if (N == 0) return CB_OK;
  CB_CHECK_ARG(s && nrm, CB_E_INVALID, "cb_cosine_scale_f32: null pointer");
  hipLaunchKernelGGL(k_nc_cosine_scale, dim3((unsigned)blocks_for(N, 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream, s, ld, N, nrm);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_ncloss_workspace_bytes(int64_t B, int32_t max_splits) {
  if (B <= 0) return 0;
  int rb, ctl, ns, tps;
  nc_geometry(B, B, max_splits, rb, ctl, ns, tps);
  return (size_t)ns * (size_t)B * sizeof(float);
}

extern "C" int cb_ncloss_fwd_f32(const float* z, int64_t ldz, int64_t B, int64_t D, float tau, const int32_t* rowptr, const int32_t* col,
                                 const float* val, int64_t n, const int64_t* batch_idx, const int32_t* pos, const int32_t* rep, int32_t max_splits,
                                 float* rinv, float* num, float* den, float* w, float* u, float* loss, int32_t* m_count, void* ws, size_t ws_bytes,
                                 void* stream) {
  NC_CHECK_SIZES("cb_ncloss_fwd_f32");
  CB_CHECK_ARG(B >= 1 && n > 0 && n < INT32_MAX && tau > 0.f, CB_E_INVALID, "cb_ncloss_fwd_f32: B >= 1, 0 < n < 2^31 and tau > 0 required");
  CB_CHECK_ARG(z && rowptr && col && val && batch_idx && pos && rep && rinv && num && den && w && u && loss && m_count, CB_E_INVALID,
               "cb_ncloss_fwd_f32: null pointer");
  CB_CHECK_ARG(ws && ws_bytes >= cb_ncloss_workspace_bytes(B, max_splits), CB_E_WORKSPACE, "cb_ncloss_fwd_f32: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  int rb, ctl, ns, tps;
  nc_geometry(B, B, max_splits, rb, ctl, ns, tps);
  hipLaunchKernelGGL(k_nc_row_norms, dim3((unsigned)blocks_for(B, 4)), dim3(256), 0, st, z, ldz, B, (int)D, (float*)nullptr, rinv);
  CB_LAUNCH_CHECK();
  NcSweep a{rinv, nullptr, tau, (float*)ws, nullptr, 0, 0, B};
  nc_launch_sweep<NC_ROWSUM>(z, ldz, B, D, rb, ns, tps, ctl, a, st);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nc_num, dim3((unsigned)blocks_for(B, 4)), dim3(256), 0, st, z, ldz, B, (int)D, tau, (const float*)rinv, rowptr, col, val, n,
                     batch_idx, pos, rep, num);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nc_finish, dim3(1), dim3(256), 0, st, (const float*)ws, ns, B, tau, (const float*)num, den, w, u, loss, m_count);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_ncloss_normalize_rows_f32(const float* z, int64_t ldz, int64_t B, int64_t D, const float* rinv, float* zhat, void* stream) {
  NC_CHECK_SIZES("cb_ncloss_normalize_rows_f32");
  if (B == 0) return CB_OK;
  CB_CHECK_ARG(z && rinv && zhat, CB_E_INVALID, "cb_ncloss_normalize_rows_f32: null pointer");
  hipLaunchKernelGGL(k_nc_normalize, dim3((unsigned)blocks_for(B, 4)), dim3(256), 0, (hipStream_t)stream, z, ldz, B, (int)D, rinv, zhat);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_ncloss_bwd_slab_f32(const float* z, int64_t ldz, int64_t B, int64_t D, float tau, const float* rinv, const float* w, int64_t row0,
                                      int64_t rows, int32_t max_splits, float* P, int64_t ldp, void* stream) {
  NC_CHECK_SIZES("cb_ncloss_bwd_slab_f32");
  CB_CHECK_ARG(B >= 1 && tau > 0.f && row0 >= 0 && row0 % 128 == 0 && rows >= 1 && row0 + rows <= B && ldp >= B, CB_E_INVALID,
               "cb_ncloss_bwd_slab_f32: B >= 1, tau > 0, row0 a multiple of 128, 1 <= rows, row0 + rows <= B and ldp >= B required");
  CB_CHECK_ARG(z && rinv && w && P, CB_E_INVALID, "cb_ncloss_bwd_slab_f32: null pointer");
  int rb, ctl, ns, tps;
  nc_geometry(rows, B, max_splits, rb, ctl, ns, tps);
  NcSweep a{rinv, w, tau, nullptr, P, ldp, row0, row0 + rows};
  nc_launch_sweep<NC_STORE>(z, ldz, B, D, rb, ns, tps, ctl, a, (hipStream_t)stream);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_ncloss_bwd_finish_f32(const float* z, int64_t ldz, const float* zhat, int64_t B, int64_t D, float tau, const float* rinv, const float* u,
                                        const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* rowptr_t, const int32_t* col_t,
                                        const float* val_t, int64_t n, const int64_t* batch_idx, const int32_t* pos, const int32_t* rep, const float* g,
                                        float* dzh, float* dz, void* stream) {
  NC_CHECK_SIZES("cb_ncloss_bwd_finish_f32");
  CB_CHECK_ARG(B >= 1 && n > 0 && n < INT32_MAX && tau > 0.f, CB_E_INVALID, "cb_ncloss_bwd_finish_f32: B >= 1, 0 < n < 2^31 and tau > 0 required");
  CB_CHECK_ARG(z && zhat && rinv && u && rowptr && col && val && rowptr_t && col_t && val_t && batch_idx && pos && rep && g && dzh && dz, CB_E_INVALID,
               "cb_ncloss_bwd_finish_f32: null pointer");
  hipLaunchKernelGGL(k_nc_bwd_finish, dim3((unsigned)blocks_for(B, 4)), dim3(256), 0, (hipStream_t)stream, z, ldz, zhat, B, (int)D, tau, rinv, u, rowptr, col,
                     val, rowptr_t, col_t, val_t, n, batch_idx, pos, rep, g, dzh, dz);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
