"""The top-K replacement kernel (csrc/cb_topk.hip, cb_topk_replace_f32 through ops.se_topk_replace) where one block folds MANY score
tiles: the running list carried from tile to tile, the threshold filter with its 1024-entry queue, the overflow fall-back once a
threshold exists, and the merge of the splits' lists — against a float64 host reference with the documented tie order (larger score,
then larger index: tests/topk_ref.py).  Every multi-tile case first proves from the ABI that its blocks get more than one tile.

Row i of a large query matrix repeats base query i mod P, so the host ranks P queries, not B."""
import functools

import numpy as np
import pytest
import torch

import topk_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
QCAP = 1024            # the filter queue of cb_topk.hip
WGT_TOL = dict(atol=1e-5, rtol=1e-4)        # the tolerances of test_se_topk_replace_matches_reference_and_oracle
OUT_TOL = dict(atol=1e-4, rtol=1e-4)

# (B, N): tiles per block / splits under the present topk_geometry — 2/16, 3/14 (last split short), 3/6 (last tile 5 columns),
# 6/1 (the production form: one split, no merge; last tile 3 columns).  The fifth is the third with a ragged last row block.
GEOMETRIES = [(8192, 4096), (8192, 5120), (16384, 2053), (131072, 643), (16300, 2053)]
RAGGED = [(8155, 5120), (16300, 2053), (130972, 643)]         # the same column geometries, B no multiple of 128


def _lib():
    from gnn_tail_generalization_amd import _lib as L
    return L, L.load()


def _assert_multi_tile(B, N, K):
    """From the ABI alone: n_splits = workspace / (B*K*8); fewer splits than column tiles <=> some block folds more than one tile."""
    _, lib = _lib()
    per_split = B * K * 8
    ws = lib.cb_topk_replace_workspace_bytes(B, N, K)
    assert ws > 0 and ws % per_split == 0, (B, N, K, ws)
    n_splits, n_col_tiles = ws // per_split, -(-N // 128)
    assert n_splits < n_col_tiles, f'(B={B}, N={N}): {n_splits} splits over {n_col_tiles} column tiles — one tile per block, not the case meant'
    return n_splits


def _place(x, layout):
    """Host [R, D] float32 -> device tensor of the same values in a named memory layout (which score kernel runs depends on it):
    'contig'  rows D apart, 16-byte aligned: the three-limb kernel when D % 4 == 0, else the fp32-input kernel with scalar loads;
    'offset'  a column-offset view, leading dimension D + 1, start 4 bytes off: the fp32-input kernel, scalar loads;
    'padded'  a view of a 16-byte aligned buffer whose leading dimension is a multiple of 4: with D % 4 != 0 the fp32-input kernel
              with float4 loads and a ragged last group.
    The cells outside the view hold 1e6, so a read past a row's D elements shows in the scores."""
    x = torch.as_tensor(x, dtype=torch.float32).to(DEV)
    R, D = x.shape
    if layout == 'contig':
        return x.contiguous()
    if layout == 'offset':
        buf = torch.full((R, D + 1), 1e6, dtype=torch.float32, device=DEV)
        v = buf[:, 1:]
    else:
        assert layout == 'padded'
        buf = torch.full((R, (D + 3) // 4 * 4 + 4), 1e6, dtype=torch.float32, device=DEV)
        v = buf[:, :D]
    v.copy_(x)
    assert v.stride(1) == 1 and not (layout != 'contig' and v.is_contiguous())
    return v


def _run(qbase, t, B, K, layout='contig'):
    """ops.se_topk_replace on B rows that repeat the base queries; returns (out, idx, wgt, rows) with rows[i] = i mod P on the device."""
    from gnn_tail_generalization_amd import ops
    rows = torch.arange(B, device=DEV) % qbase.shape[0]
    q = _place(torch.as_tensor(qbase, dtype=torch.float32)[rows.cpu()], layout)
    out, idx, wgt = ops.se_topk_replace(q, _place(t, layout), K, return_selection=True)
    torch.cuda.synchronize()
    return out, idx, wgt, rows


def _assert_idx_equal(idx, want, what):
    """idx [B,K] int32 device vs want [B,K] int64 device, with a message that names the first rows that differ."""
    bad = (idx.long() != want).any(dim=1)
    if bool(bad.any()):
        r = bad.nonzero().flatten()[:5].tolist()
        detail = '; '.join(f'row {i}: got {idx[i].tolist()} want {want[i].tolist()}' for i in r)
        raise AssertionError(f'{what}: selection differs in {int(bad.sum())} of {idx.shape[0]} rows — {detail}')


def _assert_matches(res, ref, what):
    """Kernel result on B rows vs the host reference on the P base queries: idx equal everywhere, weights and out to float64."""
    out, idx, wgt, rows = res
    ref_out, ref_idx, ref_wgt = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in ref)
    _assert_idx_equal(idx, ref_idx[rows], what)
    torch.testing.assert_close(wgt.double(), ref_wgt[rows], **WGT_TOL, msg=lambda m: f'{what}: weights: {m}')
    torch.testing.assert_close(out.double(), ref_out[rows], **OUT_TOL, msg=lambda m: f'{what}: out: {m}')


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. exact small-integer inputs: every score is an integer of magnitude <= 9 * D, exact in fp32 on either score kernel, so the
#    reference selection is unambiguous and idx must EQUAL it for every query — while about half of the queries tie exactly at the
#    K-th / (K+1)-th place (asserted below), so the index rule decides across tiles and splits.
# ------------------------------------------------------------------------------------------------------------------------------------
SCORE_PATHS = {'limb': (16, 'contig'), 'f32_d18': (18, 'contig'), 'f32_offset_view': (16, 'offset'), 'f32_padded_view': (18, 'padded')}


@functools.lru_cache(maxsize=None)
def _integer_case(N, D):
    rng = np.random.default_rng(1000 * D + N)
    q = rng.integers(-3, 4, size=(512, D)).astype(np.float32)
    t = rng.integers(-3, 4, size=(N, D)).astype(np.float32)
    return q, t, topk_ref.Ranking(q, t)


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('path', list(SCORE_PATHS))
@pytest.mark.parametrize('B,N', GEOMETRIES)
def test_exact_integer_scores_select_exactly(B, N, path, K):
    D, layout = SCORE_PATHS[path]
    _assert_multi_tile(B, N, K)
    q, t, rk = _integer_case(N, D)
    if N >= 4096 and K == 8:
        assert rk.boundary_ties(K).mean() > 0.3          # the index rule decides a large share of these selections
    _assert_matches(_run(q, t, B, K, layout), rk.select(K), f'B={B} N={N} D={D} K={K} {path}')


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. all teacher rows identical: every score of a query ties, the index rule alone selects N-K .. N-1, every weight is exactly 1/K.
#    From its second tile on, a block sees 16 384 scores equal to its threshold: the queue floods with a FINITE threshold in place.
#    (8192, 4096) is here because its LAST split ends in a full tile, so the winners themselves come through a flooded queue; the ragged
#    geometries end in a narrow tile (or a one-tile split) whose few columns fit the queue.
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 8])
@pytest.mark.parametrize('layout', ['contig', 'offset'])
@pytest.mark.parametrize('B,N', RAGGED + [(8192, 4096)])
def test_identical_teacher_rows_tie_to_the_largest_indices(B, N, layout, K):
    from gnn_tail_generalization_amd import ops
    D = 16
    _assert_multi_tile(B, N, K)
    gen = torch.Generator().manual_seed(N + K)
    row = torch.randn(D, generator=gen)
    q = torch.randn(B, D, generator=gen)
    out, idx, wgt = ops.se_topk_replace(_place(q, layout), _place(row.expand(N, D), layout), K, return_selection=True)
    want = torch.arange(N - K, N, device=DEV).expand(B, K)
    _assert_idx_equal(idx, want, f'B={B} N={N} K={K} {layout}')
    assert torch.equal(wgt, torch.full_like(wgt, 1.0) / K)         # exp(0) = 1, K ones sum to K, one correctly rounded division
    torch.testing.assert_close(out.double(), row.double().to(DEV).expand(B, D), **OUT_TOL)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. monotone score orders: coordinate 0 of teacher row j is j, a query is (a, 0, ..., 0), so its score is a * j exactly (< 2^24).
#    a > 0: every later tile supersedes the whole list.  a < 0: nothing after a block's first tile passes the filter.
#    Three kinds of row block (row i repeats base query i mod 384):
#      block 0  even rows a > 0, odd rows a < 0: 64 x 128 candidates per tile flood the queue; the unfiltered fold then runs over lists
#               of which half must not move;
#      block 1  all rows a < 0: after the first tile no score passes — the empty-queue path, which leaves the threshold untouched;
#      block 2  four rows a > 0 (4 x 128 = 512 candidates <= QCAP), the rest a < 0: the filtered path replaces whole lists, tile after tile.
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _monotone_case(N):
    D = 8
    rng = np.random.default_rng(N)
    t = rng.integers(-3, 4, size=(N, D)).astype(np.float32)
    t[:, 0] = np.arange(N)
    a = 1.0 + np.arange(384) % 3
    sign = -np.ones(384)
    sign[0:128:2] = 1
    sign[[256 + 5, 256 + 40, 256 + 77, 256 + 127]] = 1
    q = np.zeros((384, D), dtype=np.float32)
    q[:, 0] = a * sign
    assert 3 * N < 2 ** 24
    return q, t, topk_ref.Ranking(q, t)


@pytest.mark.parametrize('B,N,K,layout', [(8155, 5120, 8, 'contig'), (16300, 2053, 3, 'offset'), (130972, 643, 8, 'contig'),
                                          (130972, 643, 1, 'offset')])
def test_monotone_scores_supersede_or_never_pass(B, N, K, layout):
    _assert_multi_tile(B, N, K)
    q, t, rk = _monotone_case(N)
    ref = rk.select(K)
    up = q[:, 0] > 0
    assert (ref[1][up] == np.arange(N - K, N)).all() and (ref[1][~up] == np.arange(K - 1, -1, -1)).all()
    _assert_matches(_run(q, t, B, K, layout), ref, f'B={B} N={N} K={K} {layout}')


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. queue boundary.  B = 8192, N = 4096, D = 128 gives every block two tiles.  Teacher rows repeat with period 256: 128 zero rows, then
#    the 128 unit vectors.  A block's first tile scores 0 everywhere and leaves threshold 0; its second tile's score matrix is the block's
#    own 128 x 128 query matrix, filled with -1 except exactly c entries of +1.  Exactly c candidates pass the filter; c runs over
#    1019 .. 1030 across the row blocks (row block b: c = 1019 + b mod 12), on either side of the queue's 1024 entries, in one launch.
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _queue_case():
    rng = np.random.default_rng(4)
    counts = list(range(QCAP - 5, QCAP + 7))
    q = -np.ones((len(counts), 128 * 128), dtype=np.float32)
    for p, c in enumerate(counts):
        q[p, rng.choice(128 * 128, size=c, replace=False)] = 1.0
    q = q.reshape(len(counts) * 128, 128)
    t = np.zeros((4096, 128), dtype=np.float32)
    for s in range(16):
        t[256 * s + 128 + np.arange(128), np.arange(128)] = 1.0
    assert [int((blk > 0).sum()) for blk in q.reshape(len(counts), -1)] == counts and counts[5] == QCAP
    return q, t, topk_ref.Ranking(q, t)


@pytest.mark.parametrize('K', [2, 8])
@pytest.mark.parametrize('layout', ['contig', 'offset'])
def test_candidate_counts_around_the_queue_capacity(layout, K):
    B, N = 8192, 4096
    assert _assert_multi_tile(B, N, K) * 2 == N // 128         # two tiles per block, as the construction assumes
    q, t, rk = _queue_case()
    _assert_matches(_run(q, t, B, K, layout), rk.select(K), f'K={K} {layout}')


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. continuous inputs at multi-tile geometries.  fp32 scores may reorder two teacher rows whose float64 scores are closer than the
#    score kernels' error, so idx must equal the reference for every query whose smallest gap among its top K+1 float64 scores is at
#    least tau = 2 * (2e-5 * max(1, sqrt(D)) + 2e-5 * |top score|), twice what test_gemm_nn_epilogues grants the GEMM.  The share of
#    queries left out is a condition of the test (<= 5 %), computed from the reference alone.  With numpy default_rng(seed)
#    .standard_normal (float64 draws rounded to float32), q drawn before T, it is 3.03 % / 0 % / 0.20 % for the three cases below.
#    For EVERY query, kept or not: the selected scores are within tau of the reference's rank by rank, and weights and out agree with a
#    float64 recombination of the rows the kernel selected.
# ------------------------------------------------------------------------------------------------------------------------------------
CONTINUOUS = {'n5120_d64_k8': (8155, 1024, 5120, 64, 8, 0), 'n2053_d36_k3': (16300, 1024, 2053, 36, 3, 1), 'n643_d8_k2': (130972, 512, 643, 8, 2, 2)}


@functools.lru_cache(maxsize=None)
def _continuous_case(name):
    B, P, N, D, K, seed = CONTINUOUS[name]
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((P, D)).astype(np.float32)
    t = rng.standard_normal((N, D)).astype(np.float32)
    return q, t, topk_ref.Ranking(q, t)


@pytest.mark.parametrize('layout', ['contig', 'offset'])
@pytest.mark.parametrize('name', list(CONTINUOUS))
def test_continuous_scores_at_multi_tile_geometries(name, layout):
    B, P, N, D, K, seed = CONTINUOUS[name]
    _assert_multi_tile(B, N, K)
    q, t, rk = _continuous_case(name)
    tau = 2 * (2e-5 * max(1.0, D ** 0.5) + 2e-5 * np.abs(rk.top_values(1)[:, 0]))
    kept = rk.min_gap(K) >= tau
    left_out = 1.0 - kept.mean()
    print(f'{name}: left out {100 * left_out:.2f} % of {P} base queries')
    assert left_out <= 0.05
    out, idx, wgt, rows = _run(q, t, B, K, layout)
    ref_out, ref_idx, ref_wgt = (torch.from_numpy(a).to(DEV) for a in rk.select(K))
    kept_rows = torch.from_numpy(kept).to(DEV)[rows]
    _assert_idx_equal(idx[kept_rows], ref_idx[rows][kept_rows], f'{name} {layout} (queries with gap >= tau)')
    torch.testing.assert_close(out[kept_rows].double(), ref_out[rows][kept_rows], **OUT_TOL)
    torch.testing.assert_close(wgt[kept_rows].double(), ref_wgt[rows][kept_rows], **WGT_TOL)
    # every query: a valid selection (in range — checked before anything gathers with it —, distinct), as good as the reference's within tau
    assert bool(((idx >= 0) & (idx < N)).all())
    srt = idx.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    q64, t64 = torch.from_numpy(q).to(DEV).double()[rows], torch.from_numpy(t).to(DEV).double()
    tsel = t64[idx.long()]                                            # [B, K, D]
    ssel = torch.einsum('bd,bkd->bk', q64, tsel)
    want_s = torch.from_numpy(np.ascontiguousarray(rk.top_values(K))).to(DEV)[rows]
    assert bool(((ssel - want_s).abs() <= torch.from_numpy(tau).to(DEV)[rows].unsqueeze(1)).all())
    w64 = torch.softmax(ssel, dim=1)
    torch.testing.assert_close(wgt.double(), w64, **WGT_TOL)
    torch.testing.assert_close(out.double(), torch.einsum('bk,bkd->bd', w64, tsel), **OUT_TOL)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. edges of the contract
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,D,K', [(130, 8, 12, 8), (3, 1, 4, 1), (257, 5, 7, 5), (8155, 5120, 16, 8)])
def test_k_equal_to_n_and_k_equal_to_8(B, N, D, K):
    rng = np.random.default_rng(B + N)
    q = rng.integers(-3, 4, size=(min(B, 512), D)).astype(np.float32)
    t = rng.integers(-3, 4, size=(N, D)).astype(np.float32)
    res = _run(q, t, B, K)
    _assert_matches(res, topk_ref.replacement(q, t, K), f'B={B} N={N} K={K}')
    if K == N:
        assert torch.equal(res[1].sort(dim=1).values, torch.arange(N, device=DEV, dtype=torch.int32).expand(B, N))


def test_no_query_rows_is_no_launch():
    from gnn_tail_generalization_amd import ops
    t = torch.randn(300, 16, device=DEV)
    out, idx, wgt = ops.se_topk_replace(torch.empty(0, 16, device=DEV), t, 2, return_selection=True)
    torch.cuda.synchronize()
    assert out.shape == (0, 16) and idx.shape == (0, 2) and wgt.shape == (0, 2)


def test_bad_sizes_and_short_workspace_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import ops
    L, lib = _lib()
    B, N, D = 200, 300, 16
    q, t = torch.randn(B, D, device=DEV), torch.randn(N, D, device=DEV)
    need = lib.cb_topk_replace_workspace_bytes(B, N, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((B, D), 7.0, device=DEV)
    idx = torch.full((B, 8), 7, dtype=torch.int32, device=DEV)
    wgt = torch.full((B, 8), 7.0, device=DEV)

    def call(n, k, ws_bytes):
        return lib.cb_topk_replace_f32(L.ptr(q), D, L.ptr(t), D, B, n, D, k, L.ptr(out), L.ptr(idx), L.ptr(wgt), L.ptr(ws), ws_bytes, L.stream_ptr())

    assert call(N, 0, need) == -1 and call(N, 9, need) == -1 and call(N, -1, need) == -1          # CB_E_INVALID
    assert call(3, 5, need) == -1                                                                  # K > N
    short = lib.cb_topk_replace_workspace_bytes(B, N, 2) - 1
    assert call(N, 2, short) == -3 and b'workspace' in lib.cb_last_error()                         # CB_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((idx == 7).all()) and bool((wgt == 7).all()) and bool((ws == 0).all())      # nothing ran
    for n, k in [(N, 0), (N, 9), (3, 5)]:
        with pytest.raises(L.HipExtensionError, match=r'rc=-1'):
            ops.se_topk_replace(q, t[:n], k, return_selection=True)
    assert call(N, 2, short + 1) == 0                                                              # the same call with enough workspace runs
    torch.cuda.synchronize()
    got = idx.flatten()[:B * 2].view(B, 2)                                                          # K = 2: the launch wrote a [B, 2] selection
    assert bool(((got >= 0) & (got < N)).all()) and bool((got[:, 0] != got[:, 1]).all()) and not bool((out == 7).any())


def test_two_identical_calls_are_bit_identical():
    from gnn_tail_generalization_amd import ops
    B, P, N, D, K, seed = CONTINUOUS['n5120_d64_k8']
    n_splits = _assert_multi_tile(B, N, K)
    assert n_splits > 1                                     # the merge of the splits' lists is part of what must not vary
    q, t, _ = _continuous_case('n5120_d64_k8')
    qd, td = torch.from_numpy(q).to(DEV)[torch.arange(B, device=DEV) % P], torch.from_numpy(t).to(DEV)
    a = ops.se_topk_replace(qd, td, K, return_selection=True)
    b = ops.se_topk_replace(qd, td, K, return_selection=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------------------------
# NaN in a query row: every score of that row is NaN, no comparison accepts one, the row has no winner.  The reference's softmax of NaN
# scores gives a NaN row; so must the kernel (out row and weights NaN, idx -1) — not a row of zeros.  The other rows do not notice.
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,layout', [(8155, 5120, 'contig'), (8155, 5120, 'offset'), (130972, 643, 'contig'), (300, 200, 'contig')])
def test_nan_query_row_yields_nan_not_zeros(B, N, layout):
    from gnn_tail_generalization_amd import ops
    D, K = 16, 3
    if N > 256:
        _assert_multi_tile(B, N, K)
    gen = torch.Generator().manual_seed(B + N)
    q, t = torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen)
    clean = ops.se_topk_replace(_place(q, layout), _place(t, layout), K, return_selection=True)
    bad = [5, 129, B - 1]                                    # first row block, another one, and the last (ragged) one
    qn = q.clone()
    qn[bad[0], 3] = float('nan')
    qn[bad[1], :] = float('nan')
    qn[bad[2], D - 1] = float('nan')
    out, idx, wgt = ops.se_topk_replace(_place(qn, layout), _place(t, layout), K, return_selection=True)
    assert bool(torch.isnan(out[bad]).all()) and bool(torch.isnan(wgt[bad]).all()) and bool((idx[bad] == -1).all())
    good = torch.ones(B, dtype=torch.bool, device=DEV)
    good[bad] = False
    for x, y in zip((out, idx, wgt), clean):
        assert torch.equal(x[good], y[good])
    assert not bool(torch.isnan(out[good]).any())
