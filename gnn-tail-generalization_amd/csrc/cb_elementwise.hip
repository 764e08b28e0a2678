// HBM-bound elementwise kernels around the GEMM/SpMM pairs of the TeacherGNN step (TricksComb.forward GNN_model/GCN.py:103-138;
// run_trainSet trainer_node_classification.py:386-430): dropout, the residual mix, the plain activation backward, the row pack / unpack of
// the halo exchange and the row-sparse backward, and the zero-rows check.  All fp32, 16-byte vector accesses when the data allows it.
#include "cb_philox.h"
#include "cb_reduce.h"
#include "cb_rowpass.h"

namespace cb {

// out[i] = x[i] * keep(offset + i) / (1 - p).  `offset` is the flat index of x[0] in the logical
// (unsharded) tensor, so a row shard draws the same mask as the full tensor would.
__global__ void __launch_bounds__(kBlock) k_dropout(const float* __restrict__ x, float* __restrict__ out, int64_t n,
                                                    uint32_t thresh, float scale, uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                                    int64_t offset, int vec_ok) {
  if (seed_dev) seed += *seed_dev;   // hipGraph mode: the per-step part of the seed lives in device memory
  const int64_t nq = (n + 3) / 4;
  const int sub = (int)(offset & 3);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    float m[4];
    const int64_t gq = (offset >> 2) + q;
    keep4(seed, gq, thresh, scale, m);
    if (sub) {  // local quad straddles two global quads (compile-time shifts: no dynamically indexed register arrays)
      float m2[4];
      keep4(seed, gq + 1, thresh, scale, m2);
      const float e[8] = {m[0], m[1], m[2], m[3], m2[0], m2[1], m2[2], m2[3]};
      if (sub == 1) { m[0] = e[1]; m[1] = e[2]; m[2] = e[3]; m[3] = e[4]; }
      else if (sub == 2) { m[0] = e[2]; m[1] = e[3]; m[2] = e[4]; m[3] = e[5]; }
      else { m[0] = e[3]; m[1] = e[4]; m[2] = e[5]; m[3] = e[6]; }
    }
    const int64_t i = q * 4;
    if (vec_ok && i + 4 <= n) {
      float4 v = *reinterpret_cast<const float4*>(x + i);
      float4 o = make_float4(v.x * m[0], v.y * m[1], v.z * m[2], v.w * m[3]);
      *reinterpret_cast<float4*>(out + i) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < n) out[i + k] = x[i + k] * m[k];
    }
  }
}

// out = a*x + b*y   (res_tricks.py:14,23: (1-alpha)*Xs[-1] + alpha*Xs[k])
__global__ void __launch_bounds__(kBlock) k_axpby(float a, const float* __restrict__ x, float b, const float* __restrict__ y,
                                                  float* __restrict__ out, int64_t n, int vec_ok) {
  const int64_t nq = (n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = q * 4;
    if (vec_ok && i + 4 <= n) {
      float4 u = *reinterpret_cast<const float4*>(x + i);
      float4 w = *reinterpret_cast<const float4*>(y + i);
      *reinterpret_cast<float4*>(out + i) = make_float4(mix2(a, u.x, b, w.x), mix2(a, u.y, b, w.y), mix2(a, u.z, b, w.z), mix2(a, u.w, b, w.w));
    } else {
      for (int k = 0; k < 4; ++k)
        if (i + k < n) out[i + k] = mix2(a, x[i + k], b, y[i + k]);
    }
  }
}

// Backward of  Y = act(b * R + bias):  gm = g * (act > 0);  colsum(gm) -> dbias partials;  out = gm * row_scale.
// Block = 256 threads laid out as (rows_per_iter = 256 / tx) x (tx column groups of 4); each thread owns 4
// fixed columns per column pass so the column sums stay in registers; partial[blockIdx][d] is reduced by colsum_finish.
__global__ void __launch_bounds__(kBlock) k_act_bwd(const float* __restrict__ g, const float* __restrict__ act,
                                                    const float* __restrict__ row_scale, float* __restrict__ out,
                                                    int64_t rows, int d, float* __restrict__ partial) {
  extern __shared__ float s_red[];  // [kBlock][4]
  const int tx = min(64, (d + 3) / 4);       // threads along columns per pass
  const int ty = kBlock / tx;                // rows per iteration
  const int cx = threadIdx.x % tx, ry = threadIdx.x / tx;
  const bool live = ry < ty;
  const RowSlab slab = row_slab(rows);
  const bool vec_ok = (d % 4 == 0);
  for (int c_base = 0; c_base < d; c_base += tx * 4) {
    const int c = c_base + cx * 4;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (live && c < d) {
      for (int64_t r = slab.begin + ry; r < slab.end; r += ty) {
        const int64_t off = r * d + c;
        const float sc = row_scale ? row_scale[r] : 1.f;
        float gv[4], av[4];
        if (vec_ok) {
          float4 t = *reinterpret_cast<const float4*>(g + off);
          gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
          if (act) {
            float4 u = *reinterpret_cast<const float4*>(act + off);
            av[0] = u.x; av[1] = u.y; av[2] = u.z; av[3] = u.w;
          }
        } else {
          for (int k = 0; k < 4; ++k) {
            gv[k] = (c + k < d) ? g[off + k] : 0.f;
            av[k] = (act && c + k < d) ? act[off + k] : 1.f;
          }
        }
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float gm = (!act || av[k] > 0.f) ? gv[k] : 0.f;
          s[k] += gm;
          o[k] = gm * sc;
        }
        if (out) {
          if (vec_ok) *reinterpret_cast<float4*>(out + off) = make_float4(o[0], o[1], o[2], o[3]);
          else
            for (int k = 0; k < 4; ++k)
              if (c + k < d) out[off + k] = o[k];
        }
      }
    }
    if (partial) {  // reduce over ry in a fixed order
#pragma unroll
      for (int k = 0; k < 4; ++k) s_red[threadIdx.x * 4 + k] = s[k];
      __syncthreads();
      if (ry == 0 && c < d) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < ty; ++j)
#pragma unroll
          for (int k = 0; k < 4; ++k) t[k] += s_red[(j * tx + cx) * 4 + k];
        for (int k = 0; k < 4; ++k)
          if (c + k < d) partial[(int64_t)blockIdx.x * d + c + k] = t[k];
      }
      __syncthreads();
    }
  }
}

// out[i, :] = src[idx[i], :]  — packs the rows a peer rank asked for (halo exchange of the node-sharded path)
__global__ void __launch_bounds__(kBlock) k_gather_rows(const float* __restrict__ src, int64_t ld, const int64_t* __restrict__ idx,
                                                        int64_t n_idx, int d, float* __restrict__ out, int vec_ok) {
  if (vec_ok) {
    const int q = d >> 2;
    const int64_t total = n_idx * q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t r = i / q;
      const int c = (int)(i - r * q) * 4;
      *reinterpret_cast<float4*>(out + r * d + c) = *reinterpret_cast<const float4*>(src + idx[r] * ld + c);
    }
  } else {
    const int64_t total = n_idx * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t r = i / d;
      out[i] = src[idx[r] * ld + (i - r * d)];
    }
  }
}

// out[r, :] = pos[r] >= 0 ? src[pos[r], :] : fill — the inverse of the row pack: a compact [n, d] matrix over a row subset written back to all
// N rows in one pass (fill = 0: the table gradient dL/dZ_l of a compact level of the row-sparse backward; fill = NaN: the logits of a rows-only
// training forward, whose other rows nobody may read; trunk.py).  float4 rows.
__global__ void __launch_bounds__(kBlock) k_expand_rows(const float* __restrict__ src, const int* __restrict__ pos, int64_t n_rows, int d,
                                                        float fill, float* __restrict__ out) {
  const int q = d >> 2;
  const int64_t total = n_rows * q;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / q;
    const int c = (int)(i - r * q) * 4;
    const int p = pos[r];
    float4 v = make_float4(fill, fill, fill, fill);
    if (p >= 0) v = *reinterpret_cast<const float4*>(src + (int64_t)p * d + c);
    __builtin_nontemporal_store(v.x, out + r * d + c);
    __builtin_nontemporal_store(v.y, out + r * d + c + 1);
    __builtin_nontemporal_store(v.z, out + r * d + c + 2);
    __builtin_nontemporal_store(v.w, out + r * d + c + 3);
  }
}

// The same row pack with the rows narrowed to bf16 (round-to-nearest-even) on their way out: the bf16 halo wire of the node-sharded
// exchange leaves the pack kernel ready to send (no separate conversion pass over the packed rows).
__global__ void __launch_bounds__(kBlock) k_gather_rows_bf16(const float* __restrict__ src, int64_t ld, const int64_t* __restrict__ idx,
                                                             int64_t n_idx, int d, bf16_t* __restrict__ out, int vec_ok) {
  if (vec_ok) {
    const int q = d >> 2;
    const int64_t total = n_idx * q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t r = i / q;
      const int c = (int)(i - r * q) * 4;
      const float4 v = *reinterpret_cast<const float4*>(src + idx[r] * ld + c);
      *reinterpret_cast<uint2*>(out + r * d + c) = pack4_bf16(v.x, v.y, v.z, v.w);
    }
  } else {
    const int64_t total = n_idx * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t r = i / d;
      out[i] = f32_to_bf16(src[idx[r] * ld + (i - r * d)]);
    }
  }
}

}  // namespace cb

using namespace cb;

extern "C" int cb_dropout_f32(const float* x, float* out, int64_t n, float p, uint64_t seed, const uint64_t* seed_dev, int64_t offset,
                              void* stream) {
  CB_CHECK_ARG(n >= 0 && offset >= 0 && (n == 0 || (x && out)) && p >= 0.f && p < 1.f, CB_E_INVALID,
               "cb_dropout_f32: bad argument (p=%f)", p);
  if (n == 0) return CB_OK;
  const uint32_t thresh = dropout_threshold(p);
  const int vec_ok = aligned16(x) && aligned16(out);
  hipLaunchKernelGGL(k_dropout, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, (hipStream_t)stream, x, out, n, thresh,
                     1.f / (1.f - p), seed, seed_dev, offset, vec_ok);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_axpby_f32(float a, const float* x, float b, const float* y, float* out, int64_t n, void* stream) {
  CB_CHECK_ARG(n >= 0 && (n == 0 || (x && y && out)), CB_E_INVALID, "cb_axpby_f32: bad argument");
  if (n == 0) return CB_OK;
  const int vec_ok = aligned16(x) && aligned16(y) && aligned16(out);
  hipLaunchKernelGGL(k_axpby, dim3(grid_for((n + 3) / 4)), dim3(kBlock), 0, (hipStream_t)stream, a, x, b, y, out, n, vec_ok);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_act_bwd_f32(const float* g, const float* act, const float* row_scale, float* out, int64_t rows, int64_t d,
                              float* colsum, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(rows >= 0 && d >= 0 && d < (1 << 20), CB_E_INVALID, "cb_act_bwd_f32: bad size");
  if (rows == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(g && (out || colsum), CB_E_INVALID, "cb_act_bwd_f32: null pointer");
  CB_CHECK_ARG(!colsum || (ws && ws_bytes >= cb_colsum_workspace_bytes(rows, d)), CB_E_WORKSPACE,
               "cb_act_bwd_f32: workspace too small (%zu < %zu)", ws_bytes, cb_colsum_workspace_bytes(rows, d));
  CB_CHECK_ARG(d % 4 != 0 || (aligned16(g) && (!act || aligned16(act)) && (!out || aligned16(out))), CB_E_INVALID,
               "cb_act_bwd_f32: 16-byte alignment required when d %% 4 == 0");
  const int nb = colsum_blocks(rows);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_act_bwd, dim3((unsigned)nb), dim3(kBlock), kBlock * 4 * sizeof(float), st, g, act, row_scale, out, rows,
                     (int)d, colsum ? (float*)ws : nullptr);
  CB_LAUNCH_CHECK();
  return colsum ? colsum_finish((const float*)ws, nb, (int)d, colsum, st) : CB_OK;
}

// Rows of g outside `mask` must be exactly zero (the promise a row-sparse backward rests on: the loss_rows argument of the forward, ops.py / trunk.py).  A streaming pass
// over the matrix (contiguous rows: float4 per thread, the row of an element by one division); a violation is recorded in the device error
// word (never silent: cb_device_status reports it) and, if given, in the caller's `guard` word in device memory: an optimiser launch that
// follows on the same stream and is handed the same word leaves parameters and moments untouched (the truncated gradients never reach them).
template <bool VEC4>
__global__ void __launch_bounds__(kBlock) k_rows_zero_check(const float* __restrict__ g, int64_t ld, int64_t rows, int d, const uint8_t* __restrict__ mask,
                                                            int* __restrict__ err, int32_t* __restrict__ guard) {
  const int64_t per_row = VEC4 ? d / 4 : d;
  const int64_t n = rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t r = i / per_row, c = (i - r * per_row) * (VEC4 ? 4 : 1);
    bool bad;
    if constexpr (VEC4) {
      const float4 v = *reinterpret_cast<const float4*>(g + r * ld + c);
      bad = v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f;
    } else {
      bad = g[r * ld + c] != 0.f;
    }
    if (bad && !mask[r]) {
      __hip_atomic_store(err + 1, (int)(r & 0x7fffffff), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(err + 2, (int)(r >> 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(err, CB_DEVERR_GRADROWS, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      if (guard) *guard = 1;      // device memory: read by the Adam launch that follows on the stream (cb_adam_multi_norm_f32, `guard`)
    }
  }
}

extern "C" int cb_rows_zero_outside_mask_f32(const float* g, int64_t ld, int64_t rows, int64_t d, const uint8_t* mask, int32_t* guard, void* stream) {
  CB_CHECK_ARG(rows >= 0 && d >= 0 && d < (1 << 20) && ld >= d, CB_E_INVALID, "cb_rows_zero_outside_mask_f32: bad size");
  if (rows == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(g && mask, CB_E_INVALID, "cb_rows_zero_outside_mask_f32: null pointer");
  int* err = device_error_word();
  CB_CHECK_ARG(err != nullptr, CB_E_HIP, "cb_rows_zero_outside_mask_f32: the device error word could not be allocated (%s)", cb_last_error());
  if (d % 4 == 0 && ld % 4 == 0 && aligned16(g))
    hipLaunchKernelGGL((k_rows_zero_check<true>), dim3((unsigned)grid_for(rows * (d / 4))), dim3(kBlock), 0, (hipStream_t)stream, g, ld, rows, (int)d, mask, err, guard);
  else
    hipLaunchKernelGGL((k_rows_zero_check<false>), dim3((unsigned)grid_for(rows * d)), dim3(kBlock), 0, (hipStream_t)stream, g, ld, rows, (int)d, mask, err, guard);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_gather_rows_f32(const float* src, int64_t ld, const int64_t* idx, int64_t n_idx, int64_t d, float* out,
                                  void* stream) {
  CB_CHECK_ARG(n_idx >= 0 && d >= 0 && d < (1 << 24) && ld >= d, CB_E_INVALID, "cb_gather_rows_f32: bad size");
  if (n_idx == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(src && idx && out, CB_E_INVALID, "cb_gather_rows_f32: null pointer");
  const int vec_ok = aligned16(src) && aligned16(out) && d % 4 == 0 && ld % 4 == 0;
  const int64_t work = vec_ok ? n_idx * (d / 4) : n_idx * d;
  hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(work)), dim3(kBlock), 0, (hipStream_t)stream, src, ld, idx, n_idx, (int)d, out, vec_ok);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_expand_rows_f32(const float* src, const int32_t* pos, int64_t n_rows, int64_t d, float fill, float* out, void* stream) {
  CB_CHECK_ARG(n_rows >= 0 && d >= 0 && d < (1 << 24), CB_E_INVALID, "cb_expand_rows_f32: bad size");
  if (n_rows == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(pos && out, CB_E_INVALID, "cb_expand_rows_f32: null pointer");
  CB_CHECK_ARG(d % 4 == 0 && aligned16(out) && (!src || aligned16(src)), CB_E_INVALID, "cb_expand_rows_f32: 16-byte aligned rows with d %% 4 == 0 expected");
  hipLaunchKernelGGL(k_expand_rows, dim3(grid_for(n_rows * (d / 4))), dim3(kBlock), 0, (hipStream_t)stream, src, pos, n_rows, (int)d, fill, out);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" int cb_gather_rows_bf16_f32(const float* src, int64_t ld, const int64_t* idx, int64_t n_idx, int64_t d, uint16_t* out,
                                       void* stream) {
  CB_CHECK_ARG(n_idx >= 0 && d >= 0 && d < (1 << 24) && ld >= d, CB_E_INVALID, "cb_gather_rows_bf16_f32: bad size");
  if (n_idx == 0 || d == 0) return CB_OK;
  CB_CHECK_ARG(src && idx && out, CB_E_INVALID, "cb_gather_rows_bf16_f32: null pointer");
  const int vec_ok = aligned16(src) && ((uintptr_t)out % 8 == 0) && d % 4 == 0 && ld % 4 == 0;
  const int64_t work = vec_ok ? n_idx * (d / 4) : n_idx * d;
  hipLaunchKernelGGL(k_gather_rows_bf16, dim3(grid_for(work)), dim3(kBlock), 0, (hipStream_t)stream, src, ld, idx, n_idx, (int)d, out, vec_ok);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
