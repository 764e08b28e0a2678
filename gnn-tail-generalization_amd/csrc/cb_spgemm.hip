// fp32 sparse x sparse product C = A B of two int32 CSR matrices and the exact transpose of one (GraphMLP's adjacency power A~^r,
// utils.py:1242-1248: `torch.sparse.mm` on the host until now).  Expand - sort - compress, one chunk of consecutive rows at a time so that
// the workspace follows a product budget and not the graph:
//
//   cb_spgemm_entry_offsets_i64  ent_off[e] = sum over A's entries e' < e of deg_B(col_a[e'])  (int64; row product counts and chunk
//                                boundaries are differences of it)
//   cb_spgemm_chunk_count_f32    k_spgemm_expand: one thread per product p of the chunk; a binary search of ent_off gives A's entry and the
//                                offset into B's row; val[p] = a * b (rounded on its own: the sum happens in another kernel) and
//                                key[p] = p << (rb + cb) | row_local << cb | col.  cb::sort_u64 on the low rb + cb bits: stable, so equal
//                                (row, col) keep the expansion order, which is the order of A's entries in the row.  Head flags -> scan ->
//                                start[u] = first sorted position of output entry u; the number of entries goes to *count
//   cb_spgemm_chunk_emit_f32     k_spgemm_compress: one thread per output entry walks its run from start[u] and adds val[key >> (rb + cb)]
//                                one by one (the first addend is the first product); k_spgemm_rowptr: one thread per row of the chunk
//   cb_csr_transpose_f32         key = e << cb | col sorted on the cb column bits (stable: rows ascend inside a column); the entry number in
//                                the high bits fetches the value, so the transpose's values are a permutation of the matrix's
//
// Deterministic: no float atomics, every sum in one fixed order that does not depend on the chunking.  Streaming kernels (8-byte key traffic,
// int32 gathers), HBM-bound: about 24 B of workspace per product, (rb + cb) / 8 sort passes of 24 B per product each.
#include "cb_sort.h"

#include "cb_common.h"

namespace cb {

constexpr int kPB = 256;                    // threads per block
constexpr int kPItems = 4;                  // consecutive elements per thread of the scans
constexpr int kPTile = kPB * kPItems;
constexpr int64_t kMaxGrid = 1 << 20;       // grid-stride kernels

// number of bits that hold every value of [0, n)
static inline int bits_for(int64_t n) {
  int b = 0;
  while (((int64_t)1 << b) < n) ++b;
  return b;
}

static inline int64_t n_tiles(int64_t n) { return (n + kPTile - 1) / kPTile; }

static inline unsigned grid_for(int64_t n) {
  const int64_t nb = (n + kPB - 1) / kPB;
  return (unsigned)(nb < 1 ? 1 : (nb > kMaxGrid ? kMaxGrid : nb));
}

// ---- exclusive scan of f(i), i < n, in int64: tile sums -> one block scans the tiles -> every tile scans itself and hands
//      (i, exclusive prefix, f(i)) to the writer.  Integer only: exact whatever the tiling -----------------------------------------------
template <class F>
__global__ void __launch_bounds__(kPB) k_tile_sums(F f, int64_t n, long long* __restrict__ tile_sums) {
  __shared__ long long s_w[kPB / kWave];
  const int64_t base = (int64_t)blockIdx.x * kPTile + (int64_t)threadIdx.x * kPItems;
  long long c = 0;
#pragma unroll
  for (int k = 0; k < kPItems; ++k)
    if (base + k < n) c += f(base + k);
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(1024) k_scan_tiles(const long long* __restrict__ tile_sums, int64_t nb, long long* __restrict__ tile_off,
                                                     long long* __restrict__ total) {
  __shared__ long long s_wave[16];
  __shared__ long long s_carry;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < nb; base += 1024) {
    const int64_t i = base + t;
    const long long v = i < nb ? tile_sums[i] : 0;
    long long x = v;      // inclusive scan inside the wavefront
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    long long wave_off = 0;
    for (int j = 0; j < w; ++j) wave_off += s_wave[j];
    const long long carry = s_carry;
    if (i < nb) tile_off[i] = carry + wave_off + x - v;
    __syncthreads();
    if (t == 1023) s_carry = carry + wave_off + x;
    __syncthreads();
  }
  if (t == 0) *total = s_carry;
}

template <class F, class W>
__global__ void __launch_bounds__(kPB) k_tile_apply(F f, W write, int64_t n, const long long* __restrict__ tile_off) {
  __shared__ long long s_w[kPB / kWave];
  const int64_t base = (int64_t)blockIdx.x * kPTile + (int64_t)threadIdx.x * kPItems;
  long long v[kPItems], c = 0;
#pragma unroll
  for (int k = 0; k < kPItems; ++k) {
    v[k] = base + k < n ? f(base + k) : 0;
    c += v[k];
  }
  long long incl = c;      // exclusive prefix of c over the block's threads (thread order = element order)
  for (int off = 1; off < kWave; off <<= 1) {
    const long long y = __shfl_up(incl, off);
    if (lane_id() >= off) incl += y;
  }
  if (lane_id() == kWave - 1) s_w[threadIdx.x >> 6] = incl;
  __syncthreads();
  long long pos = tile_off[blockIdx.x] + incl - c;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) pos += s_w[w];
#pragma unroll
  for (int k = 0; k < kPItems; ++k)
    if (base + k < n) {
      write(base + k, pos, v[k]);
      pos += v[k];
    }
}

static size_t scan_ws_bytes(int64_t n) { return 2 * align_up((size_t)n_tiles(n < 1 ? 1 : n) * sizeof(long long), 256); }

// n > 0; *total (device) = sum of f
template <class F, class W>
static int run_scan(F f, W write, int64_t n, long long* total, void* ws, hipStream_t st) {
  const int64_t nb = n_tiles(n);
  CB_CHECK_ARG(nb < INT32_MAX, CB_E_RANGE, "spgemm scan: too many tiles");
  long long* sums = (long long*)ws;
  long long* offs = (long long*)((char*)ws + align_up((size_t)nb * sizeof(long long), 256));
  hipLaunchKernelGGL((k_tile_sums<F>), dim3((unsigned)nb), dim3(kPB), 0, st, f, n, sums);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, st, (const long long*)sums, nb, offs, total);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_tile_apply<F, W>), dim3((unsigned)nb), dim3(kPB), 0, st, f, write, n, (const long long*)offs);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

// ---- ent_off ------------------------------------------------------------------------------------------------------------------------
struct EntryDegree {      // products of A's entry e = length of B's row col_a[e]; 0 for a column outside B (reported by OffsetWriter)
  const int32_t* col_a;
  const int32_t* rowptr_b;
  int64_t k;
  __device__ __forceinline__ long long operator()(int64_t e) const {
    const int64_t c = col_a[e];
    if (c < 0 || c >= k) return 0;
    const long long d = (long long)rowptr_b[c + 1] - rowptr_b[c];
    return d > 0 ? d : 0;
  }
};

struct OffsetWriter {
  const int32_t* col_a;
  const int32_t* rowptr_b;
  int64_t k;
  long long* ent_off;
  int32_t* bad;
  __device__ __forceinline__ void operator()(int64_t e, long long pos, long long) const {
    ent_off[e] = pos;
    const int64_t c = col_a[e];
    if (c < 0 || c >= k || rowptr_b[c + 1] < rowptr_b[c]) atomicAdd(bad, 1);
  }
};

// ---- one chunk: rows [row0, row1) of A, P products ------------------------------------------------------------------------------------
// key[p] = p << eb | (row - row0) << cb | col,  val[p] = a * b.  Every lookup stays inside its array whatever the inputs hold: an entry or
// offset that does not belong to the chunk (P not the chunk's product count) yields the product 0.0 at (row0, column 0).
__global__ void __launch_bounds__(kPB) k_spgemm_expand(const int32_t* __restrict__ rowptr_a, const int32_t* __restrict__ col_a,
                                                       const float* __restrict__ val_a, const int32_t* __restrict__ rowptr_b,
                                                       const int32_t* __restrict__ col_b, const float* __restrict__ val_b,
                                                       const long long* __restrict__ ent_off, int64_t row0, int64_t row1, int64_t k, int64_t P,
                                                       int eb, int cb, uint64_t* __restrict__ keys, float* __restrict__ val) {
  const int64_t e_lo = rowptr_a[row0], e_hi = rowptr_a[row1];
  const long long g0 = ent_off[e_lo];
  const uint64_t cmask = (1ull << cb) - 1ull;
  for (int64_t p = (int64_t)blockIdx.x * kPB + threadIdx.x; p < P; p += (int64_t)gridDim.x * kPB) {
    const long long g = g0 + p;
    int64_t lo = e_lo, hi = e_hi;      // the last entry with ent_off[e] <= g: ent_off[lo] <= g < ent_off[hi]
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (ent_off[mid] <= g) lo = mid;
      else hi = mid;
    }
    const int64_t e = lo;
    int64_t rlo = row0, rhi = row1;    // the last row with rowptr_a[row] <= e (empty rows share a start with the row after them)
    while (rhi - rlo > 1) {
      const int64_t mid = rlo + (rhi - rlo) / 2;
      if (rowptr_a[mid] <= e) rlo = mid;
      else rhi = mid;
    }
    const int64_t c = e < e_hi ? col_a[e] : -1;
    uint64_t key = (uint64_t)p << eb;
    float v = 0.0f;
    if (c >= 0 && c < k) {
      const int64_t j = (int64_t)rowptr_b[c] + (g - ent_off[e]);
      if (j < rowptr_b[c + 1]) {
        v = val_a[e] * val_b[j];
        key |= ((uint64_t)(rlo - row0) << cb) | ((uint64_t)(uint32_t)col_b[j] & cmask);
      }
    }
    keys[p] = key;
    val[p] = v;
  }
}

struct HeadFlag {         // sorted position i opens a run: its (row, col) differs from its predecessor's
  const uint64_t* keys;
  uint64_t mask;
  __device__ __forceinline__ long long operator()(int64_t i) const { return (i == 0 || ((keys[i] ^ keys[i - 1]) & mask) != 0ull) ? 1 : 0; }
};

struct StartWriter {
  int32_t* start;
  __device__ __forceinline__ void operator()(int64_t i, long long pos, long long head) const {
    if (head) start[pos] = (int32_t)i;
  }
};

// C's entry u = the sequential fp32 sum of the products of its run, in sorted (= expansion) order
__global__ void __launch_bounds__(kPB) k_spgemm_compress(const uint64_t* __restrict__ keys, const float* __restrict__ val,
                                                         const int32_t* __restrict__ start, int64_t P, int64_t count, int eb, int cb,
                                                         int32_t* __restrict__ col_out, float* __restrict__ val_out) {
  const uint64_t cmask = (1ull << cb) - 1ull;
  for (int64_t u = (int64_t)blockIdx.x * kPB + threadIdx.x; u < count; u += (int64_t)gridDim.x * kPB) {
    const int64_t s0 = start[u], s1 = u + 1 < count ? (int64_t)start[u + 1] : P;
    const uint64_t k0 = keys[s0];
    float acc = val[k0 >> eb];
    for (int64_t s = s0 + 1; s < s1; ++s) acc += val[keys[s] >> eb];
    col_out[u] = (int32_t)(k0 & cmask);
    val_out[u] = acc;
  }
}

// rowptr[row0 + r] = nnz_base + (number of the chunk's entries in rows before r)
__global__ void __launch_bounds__(kPB) k_spgemm_rowptr(const uint64_t* __restrict__ keys, const int32_t* __restrict__ start, int64_t count,
                                                       int cb, int rb, int64_t rows, int64_t nnz_base, int32_t* __restrict__ rowptr) {
  const uint64_t rmask = (1ull << rb) - 1ull;
  for (int64_t r = (int64_t)blockIdx.x * kPB + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kPB) {
    int64_t lo = 0, hi = count;        // the first entry whose row is >= r
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)((keys[start[mid]] >> cb) & rmask) < r) lo = mid + 1;
      else hi = mid;
    }
    rowptr[r] = (int32_t)(nnz_base + lo);
  }
}

struct ChunkLayout {      // workspace of one chunk of P products
  size_t keys_a, keys_b, val, start, sort, scan, total, bytes;
  size_t sort_bytes;
  explicit ChunkLayout(int64_t P) {
    const size_t n = (size_t)(P < 1 ? 1 : P);
    size_t o = 0;
    keys_a = o, o += align_up(n * sizeof(uint64_t), 256);
    keys_b = o, o += align_up(n * sizeof(uint64_t), 256);
    val = o, o += align_up(n * sizeof(float), 256);
    start = o, o += align_up(n * sizeof(int32_t), 256);
    sort_bytes = align_up(sort_u64_temp_bytes((int64_t)n), 256);
    sort = o, o += sort_bytes;
    scan = o, o += scan_ws_bytes((int64_t)n);
    total = o, o += 256;
    bytes = o;
  }
};

// ---- transpose ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPB) k_transpose_keys(const int32_t* __restrict__ col, int64_t nnz, int cb, uint64_t* __restrict__ keys) {
  const uint64_t cmask = (1ull << cb) - 1ull;
  for (int64_t e = (int64_t)blockIdx.x * kPB + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kPB)
    keys[e] = ((uint64_t)e << cb) | ((uint64_t)(uint32_t)col[e] & cmask);
}

// transposed entry j: its row of the matrix becomes the column, its value is fetched by its entry number
__global__ void __launch_bounds__(kPB) k_transpose_emit(const uint64_t* __restrict__ keys, const int32_t* __restrict__ rowptr, int64_t m,
                                                        const float* __restrict__ val, int64_t nnz, int cb, int32_t* __restrict__ col_t,
                                                        float* __restrict__ val_t) {
  for (int64_t j = (int64_t)blockIdx.x * kPB + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * kPB) {
    const int64_t e = (int64_t)(keys[j] >> cb);
    int64_t lo = 0, hi = m;            // the last row with rowptr[row] <= e
    while (hi - lo > 1) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (rowptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    col_t[j] = (int32_t)lo;
    val_t[j] = val[e];
  }
}

__global__ void __launch_bounds__(kPB) k_transpose_rowptr(const uint64_t* __restrict__ keys, int64_t nnz, int64_t n, int cb,
                                                          int32_t* __restrict__ rowptr_t) {
  const uint64_t cmask = (1ull << cb) - 1ull;
  for (int64_t c = (int64_t)blockIdx.x * kPB + threadIdx.x; c <= n; c += (int64_t)gridDim.x * kPB) {
    int64_t lo = 0, hi = nnz;          // the first sorted entry whose column is >= c
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)(keys[mid] & cmask) < c) lo = mid + 1;
      else hi = mid;
    }
    rowptr_t[c] = (int32_t)lo;
  }
}

}  // namespace cb

using namespace cb;

extern "C" size_t cb_spgemm_offsets_workspace_bytes(int64_t nnz_a) { return scan_ws_bytes(nnz_a); }

extern "C" int cb_spgemm_entry_offsets_i64(const int32_t* col_a, int64_t nnz_a, const int32_t* rowptr_b, int64_t k, int64_t* ent_off,
                                           int32_t* n_bad, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(nnz_a >= 0 && k >= 0 && ent_off && n_bad && rowptr_b && (nnz_a == 0 || col_a), CB_E_INVALID,
               "cb_spgemm_entry_offsets_i64: bad argument");
  CB_CHECK_ARG(nnz_a < INT32_MAX && k < INT32_MAX, CB_E_RANGE, "cb_spgemm_entry_offsets_i64: size exceeds the int32 index contract");
  CB_CHECK_ARG(ws && ws_bytes >= cb_spgemm_offsets_workspace_bytes(nnz_a), CB_E_WORKSPACE, "cb_spgemm_entry_offsets_i64: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  CB_HIP(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
  if (nnz_a == 0) {
    CB_HIP(hipMemsetAsync(ent_off, 0, sizeof(int64_t), st));
    return CB_OK;
  }
  long long* off = (long long*)ent_off;
  return run_scan(EntryDegree{col_a, rowptr_b, k}, OffsetWriter{col_a, rowptr_b, k, off, n_bad}, nnz_a, off + nnz_a, ws, st);
}

extern "C" size_t cb_spgemm_chunk_workspace_bytes(int64_t n_products) { return n_products < 0 ? 0 : ChunkLayout(n_products).bytes; }

// the bit split of a chunk's keys; CB_E_RANGE where it does not fit
static int chunk_bits(int64_t rows, int64_t n_cols, int64_t P, int* rb, int* cb, const char* who) {
  CB_CHECK_ARG(P < INT32_MAX && n_cols < INT32_MAX, CB_E_RANGE, "%s: a chunk's products / the columns exceed the int32 index contract", who);
  *cb = bits_for(n_cols < 2 ? 2 : n_cols);
  *rb = bits_for(rows);
  CB_CHECK_ARG(bits_for(P) + *rb + *cb <= 64, CB_E_RANGE, "%s: product, row and column bits of the chunk exceed 64 (fewer rows per chunk)", who);
  return CB_OK;
}

extern "C" int cb_spgemm_chunk_count_f32(const int32_t* rowptr_a, const int32_t* col_a, const float* val_a, const int32_t* rowptr_b,
                                         const int32_t* col_b, const float* val_b, const int64_t* ent_off, int64_t row0, int64_t row1, int64_t k,
                                         int64_t n_cols, int64_t n_products, int64_t* count, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(row0 >= 0 && row1 > row0 && k >= 0 && n_cols >= 0 && n_products >= 0 && count && rowptr_a && rowptr_b && ent_off, CB_E_INVALID,
               "cb_spgemm_chunk_count_f32: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (n_products == 0) {
    CB_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), st));
    return CB_OK;
  }
  CB_CHECK_ARG(col_a && val_a && col_b && val_b, CB_E_INVALID, "cb_spgemm_chunk_count_f32: null matrix");
  int rb, cb;
  {
    const int rc = chunk_bits(row1 - row0, n_cols, n_products, &rb, &cb, "cb_spgemm_chunk_count_f32");
    if (rc != CB_OK) return rc;
  }
  const ChunkLayout L(n_products);
  CB_CHECK_ARG(ws && ws_bytes >= L.bytes, CB_E_WORKSPACE, "cb_spgemm_chunk_count_f32: workspace too small");
  char* w = (char*)ws;
  uint64_t* keys_a = (uint64_t*)(w + L.keys_a);
  uint64_t* keys_b = (uint64_t*)(w + L.keys_b);
  const int eb = rb + cb;
  hipLaunchKernelGGL(k_spgemm_expand, dim3(grid_for(n_products)), dim3(kPB), 0, st, rowptr_a, col_a, val_a, rowptr_b, col_b, val_b,
                     (const long long*)ent_off, row0, row1, k, n_products, eb, cb, keys_a, (float*)(w + L.val));
  CB_LAUNCH_CHECK();
  {
    const int rc = sort_u64(w + L.sort, L.sort_bytes, keys_a, keys_b, n_products, eb, st);
    if (rc != CB_OK) return rc;
  }
  return run_scan(HeadFlag{keys_b, (1ull << eb) - 1ull}, StartWriter{(int32_t*)(w + L.start)}, n_products, (long long*)count, w + L.scan, st);
}

extern "C" int cb_spgemm_chunk_emit_f32(const void* ws, size_t ws_bytes, int64_t row0, int64_t row1, int64_t n_cols, int64_t n_products,
                                        int64_t count, int64_t nnz_base, int32_t* rowptr, int32_t* col_out, float* val_out, void* stream) {
  CB_CHECK_ARG(row0 >= 0 && row1 > row0 && n_cols >= 0 && n_products >= 0 && count >= 0 && count <= n_products && nnz_base >= 0 && rowptr,
               CB_E_INVALID, "cb_spgemm_chunk_emit_f32: bad argument");
  CB_CHECK_ARG(nnz_base + count < INT32_MAX, CB_E_RANGE, "cb_spgemm_chunk_emit_f32: the product holds 2^31 entries or more (int32 index contract)");
  int rb, cb;
  {
    const int rc = chunk_bits(row1 - row0, n_cols, n_products, &rb, &cb, "cb_spgemm_chunk_emit_f32");
    if (rc != CB_OK) return rc;
  }
  const ChunkLayout L(n_products);
  CB_CHECK_ARG(count == 0 || (ws && ws_bytes >= L.bytes && col_out && val_out), CB_E_WORKSPACE,
               "cb_spgemm_chunk_emit_f32: workspace too small / null output");
  hipStream_t st = (hipStream_t)stream;
  const char* w = (const char*)ws;
  const uint64_t* keys = (const uint64_t*)(w + L.keys_b);
  const int32_t* start = (const int32_t*)(w + L.start);
  if (count > 0) {
    hipLaunchKernelGGL(k_spgemm_compress, dim3(grid_for(count)), dim3(kPB), 0, st, keys, (const float*)(w + L.val), start, n_products, count,
                       rb + cb, cb, col_out, val_out);
    CB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_spgemm_rowptr, dim3(grid_for(row1 - row0)), dim3(kPB), 0, st, keys, start, count, cb, rb, row1 - row0, nnz_base,
                     rowptr + row0);
  CB_LAUNCH_CHECK();
  return CB_OK;
}

extern "C" size_t cb_csr_transpose_workspace_bytes(int64_t nnz) {
  if (nnz < 0) return 0;
  const size_t n = (size_t)(nnz < 1 ? 1 : nnz);
  return 2 * align_up(n * sizeof(uint64_t), 256) + align_up(sort_u64_temp_bytes((int64_t)n), 256);
}

extern "C" int cb_csr_transpose_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t m, int64_t n, int64_t nnz,
                                    int32_t* rowptr_t, int32_t* col_t, float* val_t, void* ws, size_t ws_bytes, void* stream) {
  CB_CHECK_ARG(m >= 0 && n >= 0 && nnz >= 0 && rowptr && rowptr_t && (nnz == 0 || (col && val && col_t && val_t && m > 0)), CB_E_INVALID,
               "cb_csr_transpose_f32: bad argument");
  CB_CHECK_ARG(m < INT32_MAX && n < INT32_MAX && nnz < INT32_MAX, CB_E_RANGE, "cb_csr_transpose_f32: size exceeds the int32 index contract");
  hipStream_t st = (hipStream_t)stream;
  if (nnz == 0) {
    CB_HIP(hipMemsetAsync(rowptr_t, 0, (size_t)(n + 1) * sizeof(int32_t), st));
    return CB_OK;
  }
  CB_CHECK_ARG(ws && ws_bytes >= cb_csr_transpose_workspace_bytes(nnz), CB_E_WORKSPACE, "cb_csr_transpose_f32: workspace too small");
  const int cb = bits_for(n < 2 ? 2 : n);      // entry number (< 2^31) above the column bits (<= 31): always inside 64
  const size_t kb = align_up((size_t)nnz * sizeof(uint64_t), 256);
  char* w = (char*)ws;
  uint64_t* keys_a = (uint64_t*)w;
  uint64_t* keys_b = (uint64_t*)(w + kb);
  hipLaunchKernelGGL(k_transpose_keys, dim3(grid_for(nnz)), dim3(kPB), 0, st, col, nnz, cb, keys_a);
  CB_LAUNCH_CHECK();
  {
    const int rc = sort_u64(w + 2 * kb, ws_bytes - 2 * kb, keys_a, keys_b, nnz, cb, st);
    if (rc != CB_OK) return rc;
  }
  hipLaunchKernelGGL(k_transpose_emit, dim3(grid_for(nnz)), dim3(kPB), 0, st, (const uint64_t*)keys_b, rowptr, m, val, nnz, cb, col_t, val_t);
  CB_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_transpose_rowptr, dim3(grid_for(n + 1)), dim3(kPB), 0, st, (const uint64_t*)keys_b, nnz, n, cb, rowptr_t);
  CB_LAUNCH_CHECK();
  return CB_OK;
}
