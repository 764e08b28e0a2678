"""Host-side checks (no GPU) of the CN / AA pair scores and the Hits@K / AUC counts: the C ABI of csrc/cb_heur.hip is declared, exported and bound
with matching argument counts and refuses bad arguments before any launch; so do the operators and the reference's surface; the dense float64
restatement (tests/heur_ref.py) equals the fixtures recorded from the unmodified reference `CN` / `AA` (CN exactly, AA within
2^-24 r (1 + 2^-16): one fp32 rounding, and n 2^-53 for the float64 summation order, log and division) and, where scipy imports, the reference's
`A[s].multiply(A_[d])`; the Hits@K and AUC formulas on counts equal brute-force pair counting."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import heur_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_heur_aa_weights_f64', 'cb_heur_pair_scores_f32', 'cb_heur_pair_scores_width_f32', 'cb_rank_counts_workspace_bytes',
               'cb_rank_counts_f32']
P8 = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: the checks below answer before any launch


def test_c_abi_of_the_heuristic_kernels():
    from gnn_tail_generalization_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'coldbrew_hip.h')).read()
    for cite in ('Link_prediction_baseline/heuristics.py:107-129', 'Link_prediction_model/layer.py:6-17', 'base_options.py:112',
                 'Link_prediction_model/utils.py:43-59'):
        assert cite in hdr, cite
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(cb_[a-z0-9_]+)\s*\(', hdr))
    assert os.path.isfile(_lib.LIB_PATH), 'build the extension first: python __graft_entry__.py'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        n_args = len([a for a in re.search(name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',') if a.strip() and a.strip() != 'void'])
        assert n_args == len(_lib.SIGNATURES[name][1]), (name, n_args, len(_lib.SIGNATURES[name][1]))
    assert {n for n in declared if 'heur' in n or 'rank_counts' in n} == set(NEW_ENTRIES)
    assert int(re.search(r'#define CB_HEUR_GROUP (\d+)', hdr).group(1)) in (16, 64)


def test_the_abi_refuses_bad_arguments_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()

    def view(**over):
        f = dict(rowptr=P8, col=P8, col_flags=0, n_rows=4, n_edges=4, hub_threshold=1, n_hubs=0, n_chunks=0, hub_rows=None, hub_chunk_ptr=None, ws=None,
                 ws_bytes=0)
        f.update(over)
        return ctypes.byref(_lib.CsrView(**f))
    assert lib.cb_heur_aa_weights_f64(None, P8, None) == -1
    assert lib.cb_heur_aa_weights_f64(view(), None, None) == -1 and b'null' in lib.cb_last_error()
    assert lib.cb_heur_aa_weights_f64(view(n_rows=0), P8, None) == -1
    assert lib.cb_heur_aa_weights_f64(view(n_rows=2 ** 31), P8, None) == -2
    assert lib.cb_heur_pair_scores_f32(None, None, P8, 3, P8, P8, None) == -1
    assert lib.cb_heur_pair_scores_f32(view(col_flags=1), None, P8, 3, P8, P8, None) == -1 and b'flags' in lib.cb_last_error()
    assert lib.cb_heur_pair_scores_f32(view(col=None), None, P8, 3, P8, P8, None) == -1
    assert lib.cb_heur_pair_scores_f32(view(n_edges=2 ** 31), None, P8, 3, P8, P8, None) == -2
    assert lib.cb_heur_pair_scores_f32(view(), None, P8, -1, P8, P8, None) == -1
    assert lib.cb_heur_pair_scores_f32(view(), None, P8, 2 ** 30, P8, P8, None) == -2
    assert lib.cb_heur_pair_scores_f32(view(), None, P8, 3, P8, None, None) == -1 and b'status' in lib.cb_last_error()
    for group in (0, 8, 32, 128):
        assert lib.cb_heur_pair_scores_width_f32(view(), None, P8, 3, group, P8, P8, None) == -1 and b'group' in lib.cb_last_error()
    assert lib.cb_rank_counts_workspace_bytes(5, 0) == 0 and lib.cb_rank_counts_workspace_bytes(-1, 4) == 0
    need = lib.cb_rank_counts_workspace_bytes(3, 1000)
    assert need >= 2 * 1000 * 8
    assert lib.cb_rank_counts_f32(P8, -1, P8, 4, P8, P8, P8, P8, need, None) == -1
    assert lib.cb_rank_counts_f32(P8, 3, P8, 2 ** 31, P8, P8, P8, P8, need, None) == -2
    assert lib.cb_rank_counts_f32(P8, 3, P8, 1000, P8, P8, None, P8, need, None) == -1 and b'status' in lib.cb_last_error()
    assert lib.cb_rank_counts_f32(None, 3, P8, 1000, P8, P8, P8, P8, need, None) == -1
    assert lib.cb_rank_counts_f32(P8, 3, None, 1000, P8, P8, P8, P8, need, None) == -1
    assert lib.cb_rank_counts_f32(P8, 3, P8, 1000, P8, P8, P8, P8, need - 1, None) == -3 and b'workspace' in lib.cb_last_error()
    assert lib.cb_rank_counts_f32(P8, 3, P8, 1000, P8, P8, P8, None, 0, None) == -3


def _fake_graph(n=8, **over):
    """A CSRGraph shell that never touched a device: enough for the checks that answer before any launch."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    g = CSRGraph.__new__(CSRGraph)
    g.N = g.n_cols = n
    g.E, g.row_offset, g.device = 4, 0, torch.device('cpu')
    g.rowptr = g.rowptr_t = torch.zeros(n + 1, dtype=torch.int32)
    g.col = g.col_t = torch.zeros(4, dtype=torch.int32)
    for k, v in over.items():
        setattr(g, k, v)
    return g


def test_the_operators_refuse_what_they_document():
    from gnn_tail_generalization_amd import _lib, ops
    from gnn_tail_generalization_amd.graph import SegmentedCSRGraph
    pairs = torch.zeros((2, 3), dtype=torch.int64)
    g = _fake_graph()
    with pytest.raises(_lib.HipExtensionError):                                              # CPU tensors: no fallback
        ops.pair_scores(g, pairs, 'CN')
    with pytest.raises(_lib.HipExtensionError):
        ops.pair_scores(g, pairs, 'AA')
    with pytest.raises(_lib.HipExtensionError):
        ops.rank_counts(torch.zeros(3), torch.zeros(6))
    with pytest.raises(_lib.HipExtensionError):
        ops.hits_at_k(torch.zeros(3), torch.zeros(6), (20,))
    with pytest.raises(_lib.HipExtensionError):
        ops.auc(torch.zeros(3), torch.zeros(6))
    for bad in (pairs.float(), pairs[0], torch.zeros((3, 2), dtype=torch.int64), pairs.to(torch.int16), pairs.numpy()):      # dtype, shape, type
        with pytest.raises(ValueError, match=r'int32 / int64 \[2, P\]'):
            ops.pair_scores(g, bad, 'CN')
    for seg in (object(), SegmentedCSRGraph.__new__(SegmentedCSRGraph), _fake_graph(n_cols=9), _fake_graph(row_offset=4)):
        with pytest.raises(ValueError, match='whole square'):                                # the wording of LinkSampler
            ops.pair_scores(seg, pairs, 'CN')
    with pytest.raises(ValueError, match='whole square'):
        ops.LinkSampler(object(), torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match='weight'):
        ops.pair_scores(g, pairs, 'CN', weight=torch.ones(8, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='fast_pagerank'):
        ops.pair_scores(g, pairs, 'PPR')
    with pytest.raises(ValueError, match='kind'):
        ops.pair_scores(g, pairs, 'Jaccard')
    with pytest.raises(ValueError, match='group'):
        ops.pair_scores(g, pairs, 'CN', group=32)
    with pytest.raises(ValueError):
        ops.auc(torch.zeros(0), torch.zeros(4))
    with pytest.raises(ValueError):
        ops.auc(torch.zeros(3), torch.zeros(0))
    with pytest.raises(ValueError):
        ops.auc_from_counts(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        ops.hits_from_counts(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), (20,))
    ops.pair_scores_check()                                                                  # nothing pending: no device is touched


def test_the_reference_surface_refuses_what_is_not_built():
    from gnn_tail_generalization_amd import _lib
    from gnn_tail_generalization_amd.Link_prediction_baseline import heuristics as H
    import gnn_tail_generalization_amd.Link_prediction_baseline as pkg
    assert pkg.CN is H.CN and pkg.AA is H.AA and pkg.eva_heuristics_v2_dec25 is H.eva_heuristics_v2_dec25 and pkg.tonp is H.tonp
    assert not hasattr(H, 'eva_heuristics') and not hasattr(H, 'get_pos_neg_edges')
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    data = types.SimpleNamespace(edge_index=ei, num_nodes=3, x=torch.zeros(3, 2))
    with pytest.raises(NotImplementedError, match='fast_pagerank'):
        H.eva_heuristics_v2_dec25('PPR', data, ei)
    with pytest.raises(NotImplementedError, match='fast_pagerank'):
        H.PPR(None, ei)
    with pytest.raises(ValueError):
        H.eva_heuristics_v2_dec25('Jaccard', data, ei)
    for name in ('edge_weight', 'edge_attr'):
        weighted = types.SimpleNamespace(edge_index=ei, num_nodes=3, x=torch.zeros(3, 2), **{name: torch.ones(3)})
        with pytest.raises(NotImplementedError, match=name):
            H.eva_heuristics_v2_dec25('CN', weighted, ei)
        assert not hasattr(weighted, 'A')
    with pytest.raises(_lib.HipExtensionError):                                              # a CPU edge list: the device graph cannot be built
        H.eva_heuristics_v2_dec25('CN', data, ei)
    with pytest.raises(ValueError, match='whole square'):
        H.CN(object(), ei)
    a = np.arange(3)
    assert H.tonp(a) is not None and np.array_equal(H.tonp(torch.arange(3)), a) and np.array_equal(H.tonp([0, 1, 2]), a)


def test_fixtures_are_the_graphs_the_issue_names():
    assert hr.golden_cases() == ['heur_asym_multi', 'heur_rows']
    a = hr.load_case('heur_asym_multi')
    g = torch.load(os.path.join(ROOT, 'tests', 'golden', 'case_graph_asym_multi.pt'), weights_only=False)
    assert torch.equal(a['edge_index'], g['edge_index']) and a['N'] == g['x'].shape[0]
    assert a['pairs'].shape == (2, 200) and int((a['pairs'][0] == a['pairs'][1]).sum()) >= 10
    assert not np.array_equal(a['A'], a['A'].T) and a['A'].max() >= 2 and np.trace(a['A']) > 0      # asymmetric, multi-edges, self loops
    r = hr.load_case('heur_rows')
    ei, n = hr.heur_rows_graph()
    assert np.array_equal(r['edge_index'].numpy(), ei) and r['N'] == n == 260
    A = r['A']
    assert tuple(int(v) for v in A.sum(axis=1)[:7]) == hr.ROW_LENGTHS
    both = (A[5] > 0) & (A[6] > 0)
    assert both.sum() >= 40
    combos = {(int(a_), int(b_)) for a_, b_ in zip(A[5][both], A[6][both])}
    assert combos >= {(i, j) for i in (1, 2, 3) for j in (1, 2, 3)}                            # multiplicities 1..3 on either side and on both
    c = A.sum(axis=0)
    assert (c == 1).any() and (c == 0).any() and A[3, 3] == 1 and A[5, 5] == 1
    assert sorted(map(tuple, r['pairs'].t().tolist())) == [(s, d) for s in range(7) for d in range(7)]
    for f in os.listdir(os.path.join(ROOT, 'tests', 'golden')):
        if f.startswith('heur_'):
            assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f)) < 64 * 1024


@pytest.mark.parametrize('name', hr.golden_cases())
def test_restatement_equals_the_reference_fixtures(name):
    c = hr.load_case(name)
    assert c['cn'].dtype == torch.float32 and c['aa'].dtype == torch.float32
    assert np.array_equal(c['cn'].numpy().astype(np.float64), c['cn64'])                     # CN: exact
    assert c['cn64'].max() < 2 ** 24
    err = np.abs(c['aa'].numpy().astype(np.float64) - c['aa64'])
    print(f'{name}: AA error / bound max {float((err / np.maximum(hr.AA_REL_BOUND * c["aa64"], 1e-300)).max()):.3f}, AA max {c["aa64"].max():.4f}')
    assert hr.within_aa_bound(c['aa'].numpy(), c['aa64']).all()
    assert (c['aa64'] > 0).sum() >= 10 and (c['cn64'] == 0).any()
    # the (s, d) and (d, s) scores agree: both are sums of the same products
    look = {(int(s), int(d)): i for i, (s, d) in enumerate(c['pairs'].t().tolist())}
    for (s, d), i in look.items():
        if (d, s) in look:
            assert c['cn64'][i] == c['cn64'][look[(d, s)]]


@pytest.mark.parametrize('name', hr.golden_cases())
def test_restatement_equals_scipy_where_it_imports(name):
    ssp = pytest.importorskip('scipy.sparse')
    c = hr.load_case(name)
    ei, n, pairs = c['edge_index'].numpy(), int(c['N']), c['pairs'].numpy()
    A = ssp.csr_matrix((np.ones(ei.shape[1], dtype=int), (ei[0], ei[1])), shape=(n, n))
    assert np.array_equal(np.asarray(A.todense(), dtype=np.float64), c['A'])
    cn = np.asarray(A[pairs[0]].multiply(A[pairs[1]]).sum(axis=1)).reshape(-1)
    assert np.array_equal(cn.astype(np.float64), c['cn64'])
    with np.errstate(divide='ignore'):
        mult = 1 / np.log(np.asarray(A.sum(axis=0), dtype=np.float64))
    mult[np.isinf(mult)] = 0
    assert np.allclose(np.asarray(mult).reshape(-1), hr.aa_weights(c['A']), rtol=0, atol=0)
    aa = np.asarray(A[pairs[0]].multiply(A.multiply(mult).tocsr()[pairs[1]]).sum(axis=1)).reshape(-1)
    assert (np.abs(aa - c['aa64']) <= 2.0 ** -40 * c['aa64']).all()                          # two float64 sums of < 2^8 terms each


def _tie_heavy(seed, P, Nn, levels):
    rng = np.random.default_rng(seed)
    return rng.integers(0, levels, P).astype(np.float32), rng.integers(0, levels, Nn).astype(np.float32)


@pytest.mark.parametrize('P,Nn,levels', [(1, 1, 1), (40, 300, 4), (65, 257, 9), (30, 19, 3), (50, 120, 1)])
def test_hits_and_auc_formulas_against_brute_force(P, Nn, levels):
    from gnn_tail_generalization_amd import ops
    pos, neg = _tie_heavy(1000 + P + Nn, P, Nn, levels)
    gt, eq = hr.rank_counts_brute(pos, neg)
    tg, te = torch.from_numpy(gt).to(torch.int32), torch.from_numpy(eq).to(torch.int32)
    ks = (1, 2, 20, 50, 100, Nn, Nn + 1)
    hits = ops.hits_from_counts(tg, te, ks)
    for k in ks:
        assert hits[f'Hits@{k}'] == hr.hits_brute(pos, neg, k), k                            # means of 0 / 1 over P in float64: the same sum
        if Nn < k:
            assert hits[f'Hits@{k}'] == 1.0
    auc = ops.auc_from_counts(tg, te, Nn)
    # every (positive, negative) pair counted one by one: above 1, tie 1/2
    wins2 = sum(2 * int(p > q) + int(p == q) for p in pos.tolist() for q in neg.tolist())
    assert auc == wins2 / (2 * P * Nn) == hr.auc_brute(pos, neg)
    per_pos = float(np.sum((Nn - gt - eq + eq / 2.0) / (P * Nn)))                            # the formula as the issue states it, in float64
    assert abs(auc - per_pos) <= 4 * P * 2.0 ** -53
    if levels == 1:
        assert auc == 0.5 and hits[f'Hits@{Nn + 1}'] == 1.0 and hits['Hits@1'] == 0.0      # a constant scorer: what MRR with ties-for-the-positive calls 1


def test_hits_is_one_with_fewer_negatives_than_k():
    from gnn_tail_generalization_amd import ops
    pos, neg = _tie_heavy(7, 12, 19, 3)
    gt, eq = hr.rank_counts_brute(pos, neg)
    hits = ops.hits_from_counts(torch.from_numpy(gt), torch.from_numpy(eq), (19, 20, 50, 100))
    assert hits['Hits@20'] == hits['Hits@50'] == hits['Hits@100'] == 1.0 and hits['Hits@19'] < 1.0
    none = ops.hits_from_counts(torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), (1, 20))
    assert none == {'Hits@1': 1.0, 'Hits@20': 1.0}                                           # Nn = 0
