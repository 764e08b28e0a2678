"""GPU: the integer kernels every graph goes through before any floating-point work — the stable LSD radix sort (cb_sort_u64), the CSR ingest
(CSRGraph / SegmentedCSRGraph), the hub plan, the ordered compactions of csrc/cb_ingest.hip and the tile scans of csrc/cb_spgemm.hip — against
the plain numpy restatements of tests/index_ref.py, exactly (torch.equal / np.array_equal; the one float comparison is the aggregation tied to
the hub plan).  The cases sit where those kernels change path: the wavefront (2048 keys) and block (8192 keys) boundaries of the sort, its
masked last digit, key_bits(N) around powers of two, and the second tile of every single-block scan (index_ref's table;
tests/test_index_host.py shows on the CPU that the large inputs reach it and that a scan without its carry would answer differently)."""
import numpy as np
import pytest
import torch

import index_ref as ir

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = 0x5A5A5A5A5A5A5A5A      # fills every output buffer before the call: a slot the kernel skipped shows


def _lib_():
    from gnn_tail_generalization_amd import _lib
    return _lib, _lib.load()


def to_dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # (a copy: the builders' arrays are shared and read-only)


def u64_to_dev(keys):
    """Device keys are int64 tensors that hold the uint64 bit pattern."""
    return to_dev(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))


def u64_to_host(t):
    return t.cpu().numpy().view(np.uint64)


def gpu_sort(keys, end_bit):
    """cb_sort_u64 of a host uint64 array -> host uint64 array."""
    _lib, lib = _lib_()
    n = int(keys.size)
    kin = u64_to_dev(keys)
    kout = torch.full((n,), POISON, dtype=torch.int64, device=DEV)
    wsb = lib.cb_sort_u64_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_sort_u64(_lib.ptr(kin), _lib.ptr(kout), n, end_bit, _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_sort_u64')
    return u64_to_host(kout)


# ---- the sort ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('end_bit', ir.SORT_END_BITS)
@pytest.mark.parametrize('n', ir.SORT_SIZES)
def test_sort_random_keys(n, end_bit):
    """Random 64-bit keys: the bits above end_bit are a random payload, so equality with the stable argsort of the masked keys holds the order of
    equal keys (stability) and the payload that rides along at once."""
    keys = ir.random_keys(n, seed=n)
    assert np.array_equal(gpu_sort(keys, end_bit), ir.sort_ref(keys, end_bit))


@pytest.mark.parametrize('pattern', ir.SORT_PATTERNS)
def test_sort_key_patterns(pattern):
    keys = ir.pattern_keys(pattern)
    assert keys.size == 8193
    assert np.array_equal(gpu_sort(keys, 64), ir.sort_ref(keys, 64))


@pytest.mark.parametrize('name', ir.SORT_TURNOVER)
def test_sort_turnover_of_the_block_scan(name):
    """1024 sort blocks exactly, one key more, and three blocks and a bit more: the second tile of k_sort_scan."""
    c = ir.sort_turnover_case(name)
    got = gpu_sort(c.keys, c.end_bit)
    assert np.array_equal(got, c.ref())


@pytest.mark.parametrize('end_bit', [3, 8, 9, 12, 16, 17, 21, 24])
def test_sort_output_buffer_after_odd_and_even_pass_counts(end_bit):
    """An odd number of passes (end_bit 1-8, 17-24) ends in keys_out, an even one (9-16) in keys_in and is copied over."""
    assert ir.sort_passes(end_bit) % 2 == (0 if 9 <= end_bit <= 16 else 1)
    keys = ir.random_keys(8193, seed=end_bit)
    assert np.array_equal(gpu_sort(keys, end_bit), ir.sort_ref(keys, end_bit))


def test_sort_is_idempotent_and_reproducible():
    keys = ir.random_keys(3 * 8192 + 77, seed=9)
    for end_bit in (20, 64):
        once = gpu_sort(keys, end_bit)
        assert np.array_equal(gpu_sort(keys, end_bit), once), 'two calls give the same bits'
        assert np.array_equal(gpu_sort(once, end_bit), once), 'sorting a sorted array leaves it unchanged'


# ---- the CSR ingest --------------------------------------------------------------------------------------------------------------------------
def _check_graph(G, want, rowptr_dtype):
    E = want.E
    assert G.rowptr.dtype == rowptr_dtype and G.col.dtype == torch.int32
    assert np.array_equal(G.rowptr.cpu().numpy(), want.rowptr.astype(G.rowptr.cpu().numpy().dtype)), 'rowptr'
    assert np.array_equal(G.col[:E].cpu().numpy(), want.col), 'col'
    assert np.array_equal(G.rowptr_t.cpu().numpy(), want.rowptr_t.astype(G.rowptr_t.cpu().numpy().dtype)), 'rowptr_t'
    assert np.array_equal(G.col_t[:E].cpu().numpy(), want.col_t), 'col_t'
    assert (G.n_zero_in_degree, G.max_in_degree, G.symmetric) == (want.n_zero_in_degree, want.max_in_degree, want.symmetric)
    assert np.array_equal(G.in_degrees().cpu().numpy(), want.in_deg) and np.array_equal(G.out_degrees().cpu().numpy(), want.out_deg)


def _edge_index(c):
    return to_dev(np.stack([c.src, c.dst]))


@pytest.mark.parametrize('E', ir.CSR_EDGES)
@pytest.mark.parametrize('N', ir.CSR_NODES)
def test_csr_ingest_vs_numpy(N, E):
    from gnn_tail_generalization_amd.graph import CSRGraph
    c = ir.csr_case(N, E)
    _check_graph(CSRGraph(_edge_index(c), N), ir.csr_ref(c.src, c.dst, N), torch.int32)


def test_csr_ingest_all_edges_enter_one_row():
    from gnn_tail_generalization_amd.graph import CSRGraph
    c = ir.csr_one_row_case()
    want = ir.csr_ref(c.src, c.dst, c.N)
    assert want.max_in_degree == c.E and want.n_zero_in_degree == c.N - 1 and not want.symmetric
    _check_graph(CSRGraph(_edge_index(c), c.N), want, torch.int32)


@pytest.mark.parametrize('N, E', ir.CSR_INT64_CASES)
def test_csr_ingest_int64_row_pointers_equal_the_int32_form(N, E):
    from gnn_tail_generalization_amd.graph import CSRGraph, SegmentedCSRGraph
    c = ir.csr_case(N, E)
    ei = _edge_index(c)
    G, S = CSRGraph(ei, N), SegmentedCSRGraph(ei, N)
    _check_graph(S, ir.csr_ref(c.src, c.dst, N), torch.int64)
    assert torch.equal(S.rowptr, G.rowptr.long()) and torch.equal(S.rowptr_t, G.rowptr_t.long())
    assert torch.equal(S.col[:E], G.col[:E]) and torch.equal(S.col_t[:E], G.col_t[:E])
    assert (S.n_zero_in_degree, S.max_in_degree, S.symmetric) == (G.n_zero_in_degree, G.max_in_degree, G.symmetric)


# ---- the hub plan ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', ir.HUB_COUNTS)
def test_hub_plan_vs_numpy_and_the_sums_it_drives(H):
    """cb_spmm_hub_count / cb_spmm_hub_fill on a CSR crafted from degrees (index_ref.hub_case): 1026 row blocks for k_hub_block_scan, up to 2049
    hubs for k_hub_scan; then the aggregation that reduces the hub rows chunk by chunk."""
    import oracle_c
    from gnn_tail_generalization_amd.graph import CSRGraph
    c = ir.hub_case(H)
    G = CSRGraph.from_csr(to_dev(c.rowptr.astype(np.int32)), to_dev(c.col), c.N, hub_threshold=c.T)
    n_hubs, n_chunks, rows, ptr = ir.hub_plan_ref(c.rowptr, c.T)
    p = G._plan
    assert (p.n_hubs, p.n_chunks) == (n_hubs, n_chunks) == (H, int(ptr[-1]))
    assert np.array_equal(p.hub_rows[:n_hubs].cpu().numpy(), rows), 'hub_rows ascending'
    assert np.array_equal(p.hub_chunk_ptr.cpu().numpy(), ptr), 'hub_chunk_ptr'
    ones = G.spmm(torch.ones(c.N, 4, device=DEV))
    assert torch.equal(ones.cpu(), torch.from_numpy(np.array(c.deg)).float()[:, None].expand(c.N, 4)), 'sums of ones are the in-degrees'
    gen = torch.Generator(device=DEV).manual_seed(H)
    for d in (4, 64):
        h = torch.randn(c.N, d, device=DEV, generator=gen)
        ref = oracle_c.spmm(c.rowptr, c.col, h.cpu().numpy())
        torch.testing.assert_close(G.spmm(h).cpu(), torch.from_numpy(ref), atol=2e-5, rtol=1e-5)      # (test_spmm_narrow_large_graph_vs_c_oracle's)


# ---- the compactions ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, pattern', ir.compact_cases())
def test_select_range_vs_numpy(n, pattern):
    _lib, lib = _lib_()
    vals, lo, hi, _keep = ir.select_case(n, pattern)
    want_idx, want_mask, want_count = ir.select_range_ref(vals, lo, hi)
    v = to_dev(vals)
    idx = torch.full((n,), POISON, dtype=torch.int64, device=DEV)
    mask = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    cnt = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    wsb = lib.cb_compact_workspace_bytes(n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_select_range_i32(_lib.ptr(v), n, lo, hi, _lib.ptr(idx), _lib.ptr(mask), _lib.ptr(cnt), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                   'cb_select_range_i32')
    assert int(cnt.item()) == want_count
    assert np.array_equal(idx[:want_count].cpu().numpy(), want_idx), 'indices, ascending'
    assert bool((idx[want_count:] == POISON).all()), 'nothing written behind the count'
    assert np.array_equal(mask.cpu().numpy(), want_mask.astype(np.uint8)), 'mask'


def test_craft_isolation_vs_numpy():
    _lib, lib = _lib_()
    c = ir.craft_case()
    want_src, want_dst, _keep = ir.craft_ref(c.src, c.dst, c.flag)
    src, dst, flag = to_dev(c.src), to_dev(c.dst), to_dev(c.flag.astype(np.uint8))
    out = torch.full((2, c.E), POISON, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    wsb = lib.cb_compact_workspace_bytes(c.E)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_craft_isolation_i64(_lib.ptr(src), _lib.ptr(dst), c.E, _lib.ptr(flag), c.N, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(cnt),
                                              _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_craft_isolation_i64')
    k = int(cnt.item())
    assert k == want_src.size
    assert np.array_equal(out[0, :k].cpu().numpy(), want_src) and np.array_equal(out[1, :k].cpu().numpy(), want_dst)
    assert bool((out[:, k:] == POISON).all())


def test_symmetrize_vs_numpy():
    _lib, lib = _lib_()
    c = ir.symmetrize_case()
    want_row, want_col = ir.symmetrize_ref(c.src, c.dst, c.N)
    src, dst = to_dev(c.src), to_dev(c.dst)
    out = torch.full((2, 2 * c.E), POISON, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    bad = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    wsb = lib.cb_symmetrize_workspace_bytes(c.E, c.N)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_symmetrize_i64(_lib.ptr(src), _lib.ptr(dst), c.E, c.N, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(cnt), _lib.ptr(bad),
                                         _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_symmetrize_i64')
    k = int(cnt.item())
    assert int(bad.item()) == 0 and k == want_row.size
    assert np.array_equal(out[0, :k].cpu().numpy(), want_row) and np.array_equal(out[1, :k].cpu().numpy(), want_col)
    assert bool((out[:, k:] == POISON).all())


# ---- the sparse product's scans and the transpose ------------------------------------------------------------------------------------------------
def _device_csr(c):
    return to_dev(c.rowptr.astype(np.int32)), to_dev(c.col.astype(np.int32)), to_dev(c.val)


@pytest.mark.parametrize('m', ir.SPGEMM_ROWS)
def test_spgemm_with_a_permutation_matrix_vs_closed_form(m):
    """A (i % 3 entries in row i) times a permutation matrix: no sums, so C is exact — the permuted columns re-sorted inside each row with the
    single fp32 products.  1 048 577 rows hold exactly 1024 tiles of entries and products; the longer matrix puts both scans into their second tile."""
    from gnn_tail_generalization_amd import ops
    c = ir.spgemm_case(m)
    rp_b, col_b, val_b = to_dev(np.arange(c.K + 1, dtype=np.int32)), to_dev(c.perm.astype(np.int32)), to_dev(c.bval)
    rowptr, col, val = ops.spgemm_csr(*_device_csr(c), rp_b, col_b, val_b, c.K)
    want_rp, want_col, want_val = ir.permuted_product_ref(c.rowptr, c.col, c.val, c.perm, c.bval)
    assert np.array_equal(rowptr.cpu().numpy(), want_rp), 'rowptr'
    assert np.array_equal(col.cpu().numpy(), want_col), 'col'
    assert np.array_equal(val.cpu().numpy().view(np.uint32), want_val.view(np.uint32)), 'val, bit for bit'


@pytest.mark.parametrize('m', ir.SPGEMM_ROWS)
def test_csr_transpose_vs_stable_sort_by_column(m):
    from gnn_tail_generalization_amd import ops
    c = ir.spgemm_case(m)
    rowptr_t, col_t, val_t = ops.csr_transpose(*_device_csr(c), c.K)
    want_rp, want_col, want_val = ir.csr_transpose_ref(c.rowptr, c.col, c.val, c.K)
    assert np.array_equal(rowptr_t.cpu().numpy(), want_rp), 'rowptr_t'
    assert np.array_equal(col_t.cpu().numpy(), want_col), 'col_t: rows ascending inside a column'
    assert np.array_equal(val_t.cpu().numpy().view(np.uint32), want_val.view(np.uint32)), 'val_t: a bit-exact permutation'
