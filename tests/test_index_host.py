"""Host-side checks (no GPU) behind tests/test_gpu_index.py:
  - the contract of the sort's C-ABI entry: every refusal with its code and the entry's name in cb_last_error(), the empty problem without
    pointers, the workspace size against the layout documented in csrc/cb_sort.hip;
  - the inputs of the large GPU cases are what those cases need: work lies behind the first 1024 items of every single-block scan, and a numpy
    emulation of the tiled scan WITHOUT its carry (index_ref.tiled_exclusive_scan(carry=False)) gives another answer than the restatement on
    them.  These are conditions on the inputs, not on the code under test: they make the GPU tests able to fail;
  - the numpy restatements of tests/index_ref.py agree with the committed reference fixtures where one exists."""
import ctypes
import os

import numpy as np
import pytest
import torch

import index_ref as ir
from conftest import GOLDEN, load_golden

CB_OK, CB_E_RANGE, CB_E_WORKSPACE = 0, -2, -3


# ---- cb_sort_u64: contract -----------------------------------------------------------------------------------------------------------------
def _host_buffers():
    """Three non-null addresses: every refusal comes before anything is read through them or launched."""
    bufs = [ctypes.create_string_buffer(64) for _ in range(3)]
    return bufs, [ctypes.c_void_p(ctypes.addressof(b)) for b in bufs]


@pytest.mark.parametrize('n, end_bit', [(-1, 8), (1 << 32, 8), ((1 << 32) + 5, 64), (8, 0), (8, -3), (8, 65), (0, 0), (0, 65)])
def test_sort_entry_refuses_sizes_and_bit_ranges(n, end_bit):
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    _keep, (a, b, w) = _host_buffers()
    assert lib.cb_sort_u64(a, b, n, end_bit, w, 1 << 40, None) == CB_E_RANGE
    assert b'cb_sort_u64' in lib.cb_last_error()


def test_sort_entry_refuses_null_buffers_and_short_scratch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    _keep, (a, b, w) = _host_buffers()
    need = lib.cb_sort_u64_workspace_bytes(100)
    for args in [(None, b, 100, 8, w, need), (a, None, 100, 8, w, need), (a, b, 100, 8, None, need), (a, b, 100, 8, w, need - 1), (a, b, 100, 8, w, 0),
                 (a, b, 8193, 64, w, lib.cb_sort_u64_workspace_bytes(8192))]:
        assert lib.cb_sort_u64(*args, None) == CB_E_WORKSPACE, args
        assert b'cb_sort_u64' in lib.cb_last_error()


@pytest.mark.parametrize('end_bit', [1, 20, 64])
def test_sort_entry_empty_problem_needs_no_pointers(end_bit):
    from gnn_tail_generalization_amd import _lib
    assert _lib.load().cb_sort_u64(None, None, 0, end_bit, None, 0, None) == CB_OK


@pytest.mark.parametrize('n', [0, 1, 8192, 8193, 8192 * 1024, 8192 * 1024 + 1])
def test_sort_workspace_bytes_follow_the_documented_layout(n):
    from gnn_tail_generalization_amd import _lib
    blocks = max(1, -(-n // 8192))
    table = -(-(blocks * 256 * 4) // 256) * 256                     # uint32 [256][blocks], rounded up to 256 bytes
    want = 2 * table + 2 * 256 * 8 + 256                            # hist + scan, 256 digit totals + 256 digit bases (uint64), slack
    assert ir.sort_workspace_bytes_ref(n) == want
    assert _lib.load().cb_sort_u64_workspace_bytes(n) == want


def test_sort_pass_counts_of_the_end_bit_grid():
    """Odd pass counts leave the result in keys_out directly, even ones in keys_in (copied back): the grid of the GPU test holds both."""
    assert [ir.sort_passes(e) for e in ir.SORT_END_BITS] == [1, 1, 1, 2, 2, 3, 5, 6, 8]
    assert all(ir.sort_passes(e) % 2 == 1 for e in list(range(1, 9)) + list(range(17, 25))) and all(ir.sort_passes(e) % 2 == 0 for e in range(9, 17))


# ---- key_bits at powers of two -------------------------------------------------------------------------------------------------------------
def test_key_bits_at_powers_of_two():
    assert [ir.key_bits(n) for n in ir.CSR_NODES] == [1, 1, 2, 8, 8, 9, 16, 17, 21]
    # 2 * bits is the sort's end_bit: a multiple of 8 (no masked pass) at 256 and 65536, a masked last pass of 2 bits one node later
    assert [2 * ir.key_bits(n) % 8 for n in (256, 257, 65536, 65537)] == [0, 2, 0, 2]


# ---- the tiled-scan emulation itself ---------------------------------------------------------------------------------------------------------
def test_tiled_scan_emulation_with_carry_is_the_exclusive_scan():
    rng = np.random.default_rng(0)
    for n in (0, 1, 1023, 1024, 1025, 2048, 2049, 5000):
        c = rng.integers(0, 9, n)
        assert np.array_equal(ir.tiled_exclusive_scan(c), ir.exclusive_scan(c))
        same = np.array_equal(ir.tiled_exclusive_scan(c, carry=False), ir.exclusive_scan(c))
        assert same == (n <= 1024 or c[:1024 * ((n - 1) // 1024)].sum() == 0)


def _carry_matters(counts):
    """True where the scan of `counts` needs its carry: the restatement and the emulation without it differ."""
    want = ir.exclusive_scan(counts)
    assert np.array_equal(ir.tiled_exclusive_scan(counts), want)
    return not np.array_equal(ir.tiled_exclusive_scan(counts, carry=False), want)


# ---- k_sort_scan ---------------------------------------------------------------------------------------------------------------------------
def test_sort_turnover_inputs_reach_the_second_tile():
    full = ir.sort_turnover_case('full_tile_e20')
    assert full.blocks == ir.SCAN_TILE and full.n == 8192 * 1024 and full.end_bit == 20      # the scan's loop must end after exactly one full tile
    one = ir.sort_turnover_case('one_key_over_e64')
    assert one.blocks == ir.SCAN_TILE + 1 and one.n == 8192 * 1024 + 1 and one.end_bit == 64
    for p in range(ir.sort_passes(one.end_bit)):      # (the histograms of pass p > 0 do not depend on the order the earlier passes left)
        d = int((one.keys[-1] >> np.uint64(8 * p)) & np.uint64(0xff))
        h = ir.sort_pass_hist(one.keys, p, one.end_bit)[d]
        assert h[ir.SCAN_TILE] == 1 and h[:ir.SCAN_TILE].sum() > 0 and _carry_matters(h), p
    tail = ir.sort_turnover_case('tail_blocks_perm_e24')
    assert tail.blocks == ir.SCAN_TILE + 4 and tail.end_bit == 24
    for p in (0, 1):      # pass p scans the keys in the order pass p - 1 left them; for p = 0 that is the input order
        keys = tail.keys if p == 0 else ir.sort_ref(tail.keys, 8 * p)
        hist = ir.sort_pass_hist(keys, p, tail.end_bit)
        assert (hist[:, ir.SCAN_TILE:].sum(1) > 0).all(), 'every one of the 256 digit values occurs in a sort block >= 1024'
        assert all(_carry_matters(hist[d]) for d in range(256))
    # the scatter that stands in for this case's argsort is the same restatement
    small = ir.sort_ref(tail.keys[:50000], 24)
    assert np.array_equal(small & np.uint64(0xffffff), np.sort(tail.keys[:50000] & np.uint64(0xffffff)))
    assert np.unique(tail.keys & np.uint64(0xffffff)).size == tail.n


# ---- k_scan_counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [s for s in ir.COMPACT_SIZES if s > ir.COMPACT_LINE])
def test_compaction_inputs_reach_the_second_tile(n):
    for pattern in ir.COMPACT_CARRY_PATTERNS:
        vals, lo, hi, keep = ir.select_case(n, pattern)
        idx, mask, count = ir.select_range_ref(vals, lo, hi)
        assert np.array_equal(mask, keep) and count == int(keep.sum())
        assert keep[ir.COMPACT_LINE:].any() and keep[:ir.COMPACT_LINE].any(), 'kept elements on both sides of block 1024'
        assert _carry_matters(ir.block_counts(keep, ir.COMPACT_BLOCK)), pattern
    # the other patterns of the grid need no carry (nothing kept, or nothing kept in front of the line): they pin the loop's bounds
    for pattern in ('none', 'only_last', 'only_first_of_block_1024'):
        assert not _carry_matters(ir.block_counts(ir.keep_pattern(n, pattern), ir.COMPACT_BLOCK)), pattern
    # ('only_first' keeps nothing behind the line, but the count is the carry out of the LAST tile: without it the count would be 0)
    assert _carry_matters(ir.block_counts(ir.keep_pattern(n, 'only_first'), ir.COMPACT_BLOCK))


def test_compaction_grid_is_complete():
    cases = ir.compact_cases()
    assert len(cases) == 6 * 7 + 2 and all(ir.select_case(n, p)[3].size == n for n, p in cases if n < 2000)
    assert ir.block_counts(ir.keep_pattern(ir.COMPACT_LINE, 'all'), ir.COMPACT_BLOCK).size == ir.SCAN_TILE      # exactly one full tile


def test_craft_and_symmetrize_inputs_reach_the_second_tile():
    c = ir.craft_case()
    assert c.E == 1_200_000
    s, d, keep = ir.craft_ref(c.src, c.dst, c.flag)
    assert 0.1 < 1 - keep.mean() < 0.3 and keep[ir.COMPACT_LINE:].any() and (c.src == c.dst).sum() > 1000
    assert _carry_matters(ir.block_counts(keep, ir.COMPACT_BLOCK))
    y = ir.symmetrize_case()
    assert (y.E, y.N) == (600_000, 5000)
    keys = np.sort(np.concatenate([y.src * y.N + y.dst, y.dst * y.N + y.src]))      # (same order as the kernel's shifted keys)
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    assert first.size == 2 * y.E > ir.COMPACT_LINE and 1000 < (~first).sum() and (~first)[ir.COMPACT_LINE:].any()
    assert _carry_matters(ir.block_counts(first, ir.COMPACT_BLOCK))
    row, col = ir.symmetrize_ref(y.src, y.dst, y.N)
    assert row.size == int(first.sum())


# ---- k_hub_block_scan, k_hub_scan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', ir.HUB_COUNTS)
def test_hub_inputs_reach_the_second_tiles(H):
    c = ir.hub_case(H)
    T, N = c.T, c.N
    assert N == 262_144 + 300 and T == 4 and c.rowptr.size == N + 1 and c.col.size == c.rowptr[-1]
    n_hubs, n_chunks, rows, ptr = ir.hub_plan_ref(c.rowptr, T)
    assert n_hubs == H and np.array_equal(rows, c.hubs) and ptr.size == H + 1 and ptr[-1] == n_chunks
    bg = np.delete(c.deg, c.hubs)
    assert bg.min() == 0 and bg.max() == T and c.deg[1] == T and c.deg[ir.HUB_LINE + 1] == T      # degree exactly T: not a hub
    if H:
        assert c.deg[c.hubs].min() == T + 1 and c.deg[c.hubs].max() == (13 if H >= 2 else T + 1)
        assert c.deg[ir.HUB_LINE] == T + 1 and ir.HUB_LINE in c.hubs                              # degree T + 1: two chunks
    if H >= 4:
        assert all(r in c.hubs for r in (0, N - 1, ir.HUB_LINE - 1, ir.HUB_LINE))
    per_block = ir.block_counts(c.deg > T, ir.HUB_ROW_BLOCK)
    assert per_block.size == ir.SCAN_TILE + 2
    if H >= 1:
        assert per_block[ir.SCAN_TILE:].sum() > 0, 'hubs in a row block >= 1024'
    if H >= 4:
        assert _carry_matters(per_block)                                                          # k_hub_block_scan
    chunks = (c.deg[rows] + T - 1) // T
    assert _carry_matters(chunks) == (H > ir.SCAN_TILE)                                           # k_hub_scan: 1025 and 2049 hubs
    assert np.array_equal(ptr[:-1], ir.exclusive_scan(chunks))


# ---- k_scan_tiles --------------------------------------------------------------------------------------------------------------------------
def test_spgemm_inputs_reach_the_second_tile():
    from gnn_tail_generalization_amd import tuning
    exact, over = (ir.spgemm_case(m) for m in ir.SPGEMM_ROWS)
    for c in (exact, over):
        k = np.diff(c.rowptr)
        assert np.array_equal(k, np.arange(c.m) % 3) and (k == 0).sum() > c.m // 3 - 1                      # empty rows
        two = np.nonzero(k == 2)[0]
        assert (c.col[c.rowptr[two]] < c.col[c.rowptr[two] + 1]).all() and c.col.min() == 0 and c.col.max() == c.K - 1
        assert np.array_equal(np.sort(c.perm), np.arange(c.K))
        assert tuning.Tuning().spgemm_chunk_products >= c.nnz      # one chunk: the head-flag scan sees every product at once
    # 1 048 577 rows of i % 3 entries hold exactly 1024 tiles of entries: both scans must stop after one full tile ...
    assert exact.m == 1_048_577 and exact.nnz == ir.SPGEMM_LINE
    # ... and the longer matrix puts entries (one product each, one distinct output entry each) behind the line of both
    assert over.nnz > ir.SPGEMM_LINE
    ones = np.ones(over.nnz, dtype=np.int64)      # B's rows hold one entry: one product per entry of A; no two products share (row, col): all heads
    assert _carry_matters(ir.block_counts(ones, ir.SPGEMM_TILE))
    assert not _carry_matters(ir.block_counts(np.ones(exact.nnz, dtype=np.int64), ir.SPGEMM_TILE))
    rp, col, val = ir.permuted_product_ref(over.rowptr, over.col, over.val, over.perm, over.bval)
    rows = np.repeat(np.arange(over.m), np.diff(over.rowptr))
    assert np.unique(rows * over.K + col).size == over.nnz and val.dtype == np.float32


# ---- the restatements against the committed fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['case_nr_se000_L2', 'case_r_initialbn_se111_L3_powerlaw'])
def test_csr_ref_matches_the_oracle_on_golden_graphs(name):
    import coldbrew_oracle as orc
    g = load_golden(name)
    ei, n = g['edge_index'].numpy(), int(g['cfg']['N_nodes'])
    want, got = orc.build_csr(g['edge_index'], n), ir.csr_ref(ei[0], ei[1], n)
    for k in ('rowptr', 'col', 'rowptr_t', 'col_t', 'in_deg', 'out_deg'):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert got.n_zero_in_degree == int((want.in_deg == 0).sum()) and got.max_in_degree == int(want.in_deg.max())
    assert got.symmetric == (np.array_equal(want.rowptr, want.rowptr_t) and np.array_equal(want.col, want.col_t))


@pytest.mark.parametrize('N, E', [(1, 1), (2, 1), (3, 8191), (257, 8193), (65537, 8192)])
def test_csr_ref_matches_the_oracle_on_the_ingest_cases(N, E):
    import coldbrew_oracle as orc
    c = ir.csr_case(N, E)
    assert c.src.min() == 0 and max(c.src.max(), c.dst.max()) == N - 1
    want, got = orc.build_csr(np.stack([c.src, c.dst]), N), ir.csr_ref(c.src, c.dst, N)
    for k in ('rowptr', 'col', 'rowptr_t', 'col_t'):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    if E >= 8:
        pairs = c.src * N + c.dst
        assert np.unique(pairs).size < E and (c.src == c.dst).sum() >= E // 8      # duplicates and self-loops


def test_symmetrize_ref_matches_the_reference_fixture():
    fx = torch.load(os.path.join(GOLDEN, 'utils_fixture.pt'), weights_only=False)
    ei = fx['asym_edge_index'].numpy()
    row, col = ir.symmetrize_ref(ei[0], ei[1], int(ei.max()) + 1)
    assert np.array_equal(np.stack([row, col]), fx['ensure_symmetric'].numpy())


def test_small_restatements_on_a_worked_example():
    vals = np.array([5, 1, 3, 3, 9, 4], dtype=np.int32)
    idx, mask, count = ir.select_range_ref(vals, 3, 5)
    assert idx.tolist() == [0, 2, 3, 5] and count == 4 and mask.tolist() == [True, False, True, True, False, True]
    src, dst, flag = np.array([0, 1, 2, 3, 3, 4]), np.array([1, 1, 2, 4, 3, 0]), np.array([False, False, False, True, False])
    s, d, _ = ir.craft_ref(src, dst, flag)
    assert s.tolist() == [0, 1, 2, 3, 4] and d.tolist() == [1, 1, 2, 3, 0]      # (3, 4) goes, the loop (3, 3) stays
    n_hubs, n_chunks, rows, ptr = ir.hub_plan_ref(np.array([0, 4, 9, 9, 22]), 4)
    assert (n_hubs, n_chunks, rows.tolist(), ptr.tolist()) == (2, 6, [1, 3], [0, 2, 6])
    keys = np.array([0x300, 0x201, 0x100, 0x001, 0x200], dtype=np.uint64)
    assert ir.sort_ref(keys, 8).tolist() == [0x300, 0x100, 0x200, 0x201, 0x001]      # stable on the low byte, the rest rides along
    rowptr, col, val = np.array([0, 2, 2, 3]), np.array([0, 2, 2]), np.array([1., 2., 3.], dtype=np.float32)
    rp_t, col_t, val_t = ir.csr_transpose_ref(rowptr, col, val, 3)
    assert rp_t.tolist() == [0, 1, 1, 3] and col_t.tolist() == [0, 0, 2] and val_t.tolist() == [1., 2., 3.]
