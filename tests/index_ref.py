"""Plain numpy restatements of the integer kernels in front of the path — the radix sort (csrc/cb_sort.hip), the CSR ingest and the hub plan
(csrc/cb_graph.hip), the ordered compaction, crafting and symmetrisation (csrc/cb_ingest.hip), the tile scans of csrc/cb_spgemm.hip — and the
deterministic builders of the cases tests/test_index_host.py (no GPU) and tests/test_gpu_index.py (GPU) share.

Every single-block scan of those files walks its input in tiles of SCAN_TILE = 1024 items with a running carry:

    scan                       item                                    second tile from
    k_sort_scan                a sort block of 8192 keys               8192 * 1024 keys     (one scan per digit value)
    k_scan_counts   (ingest)   a compaction block of 1024 elements     1024 * 1024 elements
    k_hub_block_scan           a block of 256 rows                     256 * 1024 rows
    k_hub_scan                 a hub row                               1024 hubs
    k_scan_tiles    (spgemm)   a tile of 1024 entries                  1024 * 1024 entries

The large cases below put work behind that line; tiled_exclusive_scan(..., carry=False) is what a scan that lost its carry would produce, and
tests/test_index_host.py shows on the CPU that it differs from the restatement on exactly these inputs — so the GPU tests can fail.

Everything here is integer work (the one float product of the spgemm case is a single IEEE fp32 multiplication): the tests compare exactly."""
import functools
from types import SimpleNamespace

import numpy as np

SCAN_TILE = 1024            # items per iteration of every single-block scan
SORT_WAVE_KEYS = 2048       # keys of one wavefront of k_sort_hist / k_sort_scatter
SORT_BLOCK_KEYS = 8192      # ... of one block: the item of k_sort_scan
COMPACT_BLOCK = 1024        # elements per block of k_compact_count: the item of k_scan_counts
SPGEMM_TILE = 1024          # entries per block of k_tile_sums: the item of k_scan_tiles
HUB_ROW_BLOCK = 256         # rows per block of k_hub_block_count: the item of k_hub_block_scan

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def _ro(*arrays):
    """The builders are cached and their arrays shared between tests: nobody writes to them."""
    for a in arrays:
        a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


# ---- restatements ------------------------------------------------------------------------------------------------------------------------
def bit_mask(end_bit):
    return U64_MAX if end_bit >= 64 else np.uint64((1 << end_bit) - 1)


def sort_ref(keys, end_bit):
    """Ascending by bits [0, end_bit), stable; the bits above ride along."""
    keys = np.asarray(keys, dtype=np.uint64)
    return keys[np.argsort(keys & bit_mask(end_bit), kind='stable')]


def sort_passes(end_bit):
    return (end_bit + 7) // 8


def _align_up(x, a):
    return (x + a - 1) // a * a


def sort_workspace_bytes_ref(n):
    """The scratch layout documented in cb_sort.hip (sort_u64): hist[256][blocks] and scan[256][blocks] of uint32, each rounded up to 256 bytes,
    256 uint64 digit totals, 256 uint64 digit bases, and 256 bytes of slack; at least one block."""
    blocks = (max(n, 1) + SORT_BLOCK_KEYS - 1) // SORT_BLOCK_KEYS
    return 2 * _align_up(blocks * 256 * 4, 256) + 2 * 256 * 8 + 256


def key_bits(N):
    """Bits of a node id in the packed (major, minor) key of the ingest: the smallest b >= 1 with 2^b >= max(N, 2)."""
    b = 1
    while (1 << b) < max(N, 2):
        b += 1
    return b


def _csr_one(major, minor, N):
    bits = key_bits(N)
    key = np.sort((major.astype(np.uint64) << np.uint64(bits)) | minor.astype(np.uint64))      # (equal keys are the same edge: no order among them)
    col = (key & np.uint64((1 << bits) - 1)).astype(np.int32)
    rowptr = np.searchsorted(key >> np.uint64(bits), np.arange(N + 1, dtype=np.uint64), side='left').astype(np.int64)
    return rowptr, col


def csr_ref(src, dst, N):
    """Both orientations of edge_index = (src, dst) by sorting packed (major, minor) pairs: by dst (rows = dst, cols = src) and by src; plus what
    the ingest reports next to them."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    rowptr, col = _csr_one(dst, src, N)
    rowptr_t, col_t = _csr_one(src, dst, N)
    in_deg, out_deg = np.bincount(dst, minlength=N).astype(np.int64), np.bincount(src, minlength=N).astype(np.int64)
    return SimpleNamespace(N=N, E=int(src.size), rowptr=rowptr, col=col, rowptr_t=rowptr_t, col_t=col_t, in_deg=in_deg, out_deg=out_deg,
                           n_zero_in_degree=int((in_deg == 0).sum()), max_in_degree=int(in_deg.max()) if N else 0,
                           symmetric=bool(np.array_equal(rowptr, rowptr_t) and np.array_equal(col, col_t)))


def hub_plan_ref(rowptr, T):
    """(n_hubs, n_chunks, hub_rows ascending, hub_chunk_ptr): rows of more than T entries, cut into ceil(deg / T) chunks each."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    hub_rows = np.nonzero(deg > T)[0]
    chunks = (deg[hub_rows] + T - 1) // T
    ptr = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(chunks)])
    return int(hub_rows.size), int(ptr[-1]), hub_rows.astype(np.int32), ptr.astype(np.int32)


def select_range_ref(vals, lo, hi):
    """(ascending indices, mask, count) of lo <= vals[i] <= hi."""
    mask = (vals >= lo) & (vals <= hi)
    idx = np.nonzero(mask)[0].astype(np.int64)
    return idx, mask, int(idx.size)


def craft_ref(src, dst, flag):
    """The edges in order without those that join two different nodes of which one is flagged."""
    keep = ~((src != dst) & (flag[src] | flag[dst]))
    return src[keep], dst[keep], keep


def symmetrize_ref(src, dst, N):
    """Union with the transpose, duplicates removed, sorted by (row, col)."""
    key = np.unique(np.concatenate([src * N + dst, dst * N + src]))
    return key // N, key % N


def permuted_product_ref(rowptr_a, col_a, val_a, perm, bval):
    """A B for B = the permutation matrix with B[c, perm[c]] = bval[c]: entry (i, c) of A becomes (i, perm[c]) with the single fp32 product
    val_a * bval[c]; no two entries of a row meet, so nothing is summed.  Columns re-sorted inside each row; the row pointers are A's."""
    rows = np.repeat(np.arange(rowptr_a.size - 1), np.diff(rowptr_a))
    ccol, cval = perm[col_a], val_a * bval[col_a]
    assert cval.dtype == np.float32
    order = np.lexsort((ccol, rows))
    return rowptr_a.astype(np.int32), ccol[order].astype(np.int32), cval[order]


def csr_transpose_ref(rowptr, col, val, n_cols):
    """Stable sort of the entries by column: rows ascend inside a column, the values move with their entries."""
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    order = np.argsort(col, kind='stable')
    rowptr_t = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.bincount(col, minlength=n_cols))])
    return rowptr_t.astype(np.int32), rows[order].astype(np.int32), val[order]


def tiled_exclusive_scan(counts, tile=SCAN_TILE, carry=True):
    """What the single-block scans compute: an exclusive prefix sum, `tile` items per iteration, the total of the iterations so far carried into
    the next.  carry=False is the defect the large cases must expose: every iteration starts from zero again."""
    counts = np.asarray(counts, dtype=np.int64)
    out, run = np.empty_like(counts), 0
    for s in range(0, counts.size, tile):
        c = counts[s:s + tile]
        incl = np.cumsum(c)
        out[s:s + tile] = run + incl - c
        if carry:
            run += int(incl[-1])
    return out


def exclusive_scan(counts):
    counts = np.asarray(counts, dtype=np.int64)
    return np.cumsum(counts) - counts


def block_counts(flags, block):
    """Per-block sums of a 0/1 (or count) array, the last block ragged."""
    flags = np.asarray(flags, dtype=np.int64)
    pad = (-flags.size) % block
    return np.concatenate([flags, np.zeros(pad, dtype=np.int64)]).reshape(-1, block).sum(1)


# ---- the sort's cases --------------------------------------------------------------------------------------------------------------------
SORT_SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 77)
SORT_END_BITS = (1, 7, 8, 9, 16, 18, 34, 47, 64)
SORT_PATTERNS = ('all_equal', 'two_values_top_byte', 'sorted', 'reverse_sorted', 'all_ones_and_zero')
SORT_TURNOVER = ('full_tile_e20', 'one_key_over_e64', 'tail_blocks_perm_e24')


def random_keys(n, seed):
    """Random 64-bit keys: whatever end_bit a test sorts on, the bits above it are a random payload."""
    return _ro(np.random.default_rng(seed).integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True))


def pattern_keys(pattern, n=8193, seed=5):
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)
    if pattern == 'all_equal':
        k = np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    elif pattern == 'two_values_top_byte':      # equal in the seven passes below the last one
        k = np.where(rng.random(n) < 0.5, np.uint64(0x01AA55AA55AA55AA), np.uint64(0xFEAA55AA55AA55AA))
    elif pattern == 'sorted':
        k = np.sort(rnd)
    elif pattern == 'reverse_sorted':
        k = np.sort(rnd)[::-1].copy()
    elif pattern == 'all_ones_and_zero':        # valid keys equal to the value the kernels fill their ragged lanes with
        k = np.where(rng.random(n) < 0.5, U64_MAX, np.uint64(0))
    else:
        raise KeyError(pattern)
    return _ro(k.astype(np.uint64))


def sort_turnover_case(name):
    """The three sorts around the second tile of k_sort_scan (1024 sort blocks = 8192 * 1024 keys):
      full_tile_e20          exactly 1024 blocks, end_bit 20 under a random payload: the scan must stop after one full tile
      one_key_over_e64       one key more: block 1024 holds a single key, whose position in each of the 8 passes needs the carry of its digit
      tail_blocks_perm_e24   3 * 8192 + 77 keys behind the line; the low 24 bits are a permutation of [0, n), so in the passes over bits 0-7
                             and 8-15 every digit value occurs behind the line — and the reference is a scatter, not a sort
    Returns keys, end_bit and ref(): the expected output, computed on demand (the two argsorts take a second or two each)."""
    rng = np.random.default_rng({'full_tile_e20': 101, 'one_key_over_e64': 102, 'tail_blocks_perm_e24': 103}[name])
    line = SORT_BLOCK_KEYS * SCAN_TILE
    if name == 'tail_blocks_perm_e24':
        n, end_bit = line + 3 * SORT_BLOCK_KEYS + 77, 24
        low = rng.permutation(n).astype(np.uint64)
        keys = (rng.integers(0, 1 << 40, size=n, dtype=np.uint64) << np.uint64(24)) | low

        def ref():
            out = np.empty(n, dtype=np.uint64)
            out[low.astype(np.int64)] = keys      # distinct sort keys: the key whose low bits are j lands at j
            return out
    else:
        n, end_bit = (line, 20) if name == 'full_tile_e20' else (line + 1, 64)
        keys = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)

        def ref():
            return sort_ref(keys, end_bit)
    return SimpleNamespace(name=name, n=n, end_bit=end_bit, keys=_ro(keys), ref=ref, blocks=(n + SORT_BLOCK_KEYS - 1) // SORT_BLOCK_KEYS)


def sort_pass_hist(keys, p, end_bit):
    """hist[digit][block] of pass p as k_sort_hist writes it: the counts k_sort_scan scans, one row per digit value."""
    bits = min(8, end_bit - 8 * p)
    digit = ((keys >> np.uint64(8 * p)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    block = np.arange(keys.size, dtype=np.int64) // SORT_BLOCK_KEYS
    blocks = (keys.size + SORT_BLOCK_KEYS - 1) // SORT_BLOCK_KEYS
    return np.bincount(digit * blocks + block, minlength=256 * blocks).reshape(256, blocks)


# ---- the ingest's cases ------------------------------------------------------------------------------------------------------------------
CSR_NODES = (1, 2, 3, 255, 256, 257, 65536, 65537, 2 ** 20 + 1)      # key_bits changes between 256 / 257 and 65536 / 65537: 2 * bits = 16 -> 18, 32 -> 34
CSR_EDGES = (0, 1, 8191, 8192, 8193)
CSR_INT64_CASES = ((257, 8193), (65537, 8192), (2 ** 20 + 1, 8191))


@functools.lru_cache(maxsize=None)
def csr_case(N, E):
    """A random multigraph on N nodes: ids 0 and N - 1 present (E >= 1), an eighth of the edges repeated, an eighth self-loops (E >= 8)."""
    rng = np.random.default_rng(1000 * (N % 9973) + E)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    if E >= 1:
        src[0], dst[0] = 0, N - 1
    if E >= 2:
        src[1], dst[1] = N - 1, 0
    k = E // 8
    if k:
        src[-k:], dst[-k:] = src[2:2 + k], dst[2:2 + k]      # duplicates, far from their originals in the input
        dst[2 + k:2 + 2 * k] = src[2 + k:2 + 2 * k]          # self-loops
    return SimpleNamespace(N=N, E=E, src=_ro(src.astype(np.int64)), dst=_ro(dst.astype(np.int64)), n_dup_or_loop=2 * k)


@functools.lru_cache(maxsize=None)
def csr_one_row_case(N=257, E=8193, row=129):
    """Every edge enters `row`: one in-degree of E (a single run of the by-dst sort), sources random with repeats."""
    rng = np.random.default_rng(77)
    src = rng.integers(0, N, E)
    src[0], src[1] = 0, N - 1
    return SimpleNamespace(N=N, E=E, row=row, src=_ro(src.astype(np.int64)), dst=_ro(np.full(E, row, dtype=np.int64)))


# ---- the hub plan's cases ----------------------------------------------------------------------------------------------------------------
HUB_T = 4
HUB_N = HUB_ROW_BLOCK * SCAN_TILE + 300      # 1026 row blocks: two of them in the second tile of k_hub_block_scan
HUB_COUNTS = (0, 1, 1023, 1024, 1025, 2049)
HUB_LINE = HUB_ROW_BLOCK * SCAN_TILE         # first row behind the line: 262 144


@functools.lru_cache(maxsize=None)
def hub_case(H):
    """A CSR crafted from degrees: background rows of 0..T entries, H hub rows of T + 1..13.  As far as H allows, the hubs include the first
    row behind the line of k_hub_block_scan, the last row, row 0 and the last row before the line; the first hub has exactly T + 1 entries
    (two chunks), the second 13 (four); rows 1 and HUB_LINE + 1 have exactly T entries: not hubs."""
    T, N = HUB_T, HUB_N
    rng = np.random.default_rng(4000 + H)
    deg = rng.integers(0, T + 1, N)
    must = [HUB_LINE, N - 1, 0, HUB_LINE - 1][:min(H, 4)]
    not_hub = [1, HUB_LINE + 1]
    pool = np.setdiff1d(np.arange(N), np.array(must + not_hub + [HUB_LINE, N - 1, 0, HUB_LINE - 1]))
    hubs = np.array(must + list(rng.choice(pool, size=max(H - 4, 0), replace=False)), dtype=np.int64)
    deg[hubs] = rng.integers(T + 1, 14, hubs.size)
    deg[not_hub] = T
    if H >= 1:
        deg[hubs[0]] = T + 1
    if H >= 2:
        deg[hubs[1]] = 13
    rowptr = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(deg)])
    col = rng.integers(0, N, int(rowptr[-1])).astype(np.int32)
    return SimpleNamespace(H=H, T=T, N=N, deg=_ro(deg.astype(np.int64)), rowptr=_ro(rowptr), col=_ro(col), hubs=_ro(np.sort(hubs)))


# ---- the compaction's cases --------------------------------------------------------------------------------------------------------------
COMPACT_LINE = COMPACT_BLOCK * SCAN_TILE      # first element of block 1024: 1 048 576
COMPACT_SIZES = (1023, 1024, 1025, COMPACT_LINE, COMPACT_LINE + 1, COMPACT_LINE + 4099)
COMPACT_PATTERNS = ('all', 'none', 'every_other', 'only_first', 'only_last', 'only_first_of_block_1024', 'random_1pct', 'random_99pct')
# the patterns that keep elements on both sides of the line: with them a lost carry shows
COMPACT_CARRY_PATTERNS = ('all', 'every_other', 'random_1pct', 'random_99pct')


def compact_cases():
    """(n, pattern) of the grid; 'only_first_of_block_1024' exists where that element does."""
    return [(n, p) for n in COMPACT_SIZES for p in COMPACT_PATTERNS if p != 'only_first_of_block_1024' or n > COMPACT_LINE]


@functools.lru_cache(maxsize=None)
def keep_pattern(n, pattern):
    keep = np.zeros(n, dtype=bool)
    if pattern == 'all':
        keep[:] = True
    elif pattern == 'every_other':
        keep[::2] = True
    elif pattern == 'only_first':
        keep[0] = True
    elif pattern == 'only_last':
        keep[n - 1] = True
    elif pattern == 'only_first_of_block_1024':
        keep[COMPACT_LINE] = True
    elif pattern in ('random_1pct', 'random_99pct'):
        keep = np.random.default_rng(n % 65521 + len(pattern)).random(n) < (0.01 if pattern == 'random_1pct' else 0.99)
        if n > COMPACT_LINE:
            keep[COMPACT_LINE] = True      # (at n = COMPACT_LINE + 1 this is the one element behind the line)
    elif pattern != 'none':
        raise KeyError(pattern)
    return _ro(keep)


def select_case(n, pattern):
    """int32 values of which cb_select_range_i32(lo = 3, hi = 5) keeps exactly the pattern: kept values lie in [3, 5], the others just outside."""
    keep = keep_pattern(n, pattern)
    i = np.arange(n)
    vals = np.where(keep, 3 + i % 3, np.where(i % 2 == 0, 2, 6)).astype(np.int32)
    return _ro(vals), 3, 5, keep


@functools.lru_cache(maxsize=None)
def craft_case(E=1_200_000, N=50_000):
    """Edges with a twentieth self-loops and a tenth of the nodes flagged: about a fifth of the edges go, all along the list."""
    rng = np.random.default_rng(31)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    loops = rng.random(E) < 0.05
    dst[loops] = src[loops]
    flag = rng.random(N) < 0.1
    return SimpleNamespace(E=E, N=N, src=_ro(src.astype(np.int64)), dst=_ro(dst.astype(np.int64)), flag=_ro(flag))


@functools.lru_cache(maxsize=None)
def symmetrize_case(E=600_000, N=5000):
    """Random pairs on few nodes: 2 E = 1.2 M packed keys of which several percent repeat, spread over the whole sorted list."""
    rng = np.random.default_rng(32)
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    src[0], dst[0] = 0, N - 1
    src[1], dst[1] = N - 1, N - 1
    return SimpleNamespace(E=E, N=N, src=_ro(src.astype(np.int64)), dst=_ro(dst.astype(np.int64)))


# ---- the sparse product's cases ----------------------------------------------------------------------------------------------------------
SPGEMM_LINE = SPGEMM_TILE * SCAN_TILE      # 1 048 576 entries
# rows of A; row i holds i % 3 entries.  1 048 577 rows hold exactly SPGEMM_LINE entries (the scans stop after one full tile); 4099 rows more
# put 4099 entries — of A for the offsets' scan, products for the head-flag scan — behind the line
SPGEMM_ROWS = (SPGEMM_LINE + 1, SPGEMM_LINE + 1 + 4099)
SPGEMM_K = 4099


@functools.lru_cache(maxsize=None)
def spgemm_case(m):
    """A [m, K] with i % 3 distinct ascending columns in row i (every third row empty), B [K, K] a permutation matrix with random values."""
    K = SPGEMM_K
    rng = np.random.default_rng(m % 1000003)
    k = np.arange(m) % 3
    rowptr = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(k)])
    c0 = rng.integers(0, K, m)
    c1 = (c0 + 1 + rng.integers(0, K - 1, m)) % K      # != c0
    col = np.empty(int(rowptr[-1]), dtype=np.int64)
    one, two = np.nonzero(k == 1)[0], np.nonzero(k == 2)[0]
    col[rowptr[one]] = c0[one]
    col[rowptr[two]], col[rowptr[two] + 1] = np.minimum(c0[two], c1[two]), np.maximum(c0[two], c1[two])
    val = rng.uniform(0.5, 2.0, col.size).astype(np.float32)
    perm = rng.permutation(K)
    bval = rng.uniform(0.5, 2.0, K).astype(np.float32)
    return SimpleNamespace(m=m, K=K, nnz=int(col.size), rowptr=_ro(rowptr), col=_ro(col), val=_ro(val), perm=_ro(perm), bval=_ro(bval))
