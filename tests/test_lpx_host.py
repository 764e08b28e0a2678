"""Host-side checks (no GPU) of the link-prediction experiment's pieces: the C ABI of csrc/cb_lpx.hip is declared, exported and bound with matching
argument counts, its set of names is closed, and bad arguments are refused before any launch; the host restatements (tests/lpx_ref.py) equal the
fixtures recorded from the unmodified reference (tests/golden/lpx_reference.pt; `cal_recall` exactly, as integer / integer) and have the properties
the device output is then compared against bit for bit; Logger, get_pos_neg_edges and the documented refusals run on CPU tensors; the new operators
reject CPU tensors."""
import ctypes
import io
import os
import re
import types

import numpy as np
import pytest
import torch

import lpx_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_lpx_max_tries', 'cb_lpx_neg_global_i32', 'cb_lpx_neg_local_i32', 'cb_lpx_permutation_workspace_bytes', 'cb_lpx_permutation_i32',
               'cb_lpx_row_ranks_f32', 'cb_lpx_recall_topk_workspace_bytes', 'cb_lpx_recall_topk_f32']
P8 = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: the checks below answer before any launch


def test_c_abi_of_the_lpx_kernels():
    from gnn_tail_generalization_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'coldbrew_hip.h')).read()
    for cite in ('negative_sample.py:5-19', 'negative_sample.py:28-40', 'utils.py:568-586'):
        assert cite in hdr, cite
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(cb_[a-z0-9_]+)\s*\(', hdr))
    assert os.path.isfile(_lib.LIB_PATH), 'build the extension first: python __graft_entry__.py'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        n_args = len([a for a in re.search(name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',') if a.strip() and a.strip() != 'void'])
        assert n_args == len(_lib.SIGNATURES[name][1]), (name, n_args, len(_lib.SIGNATURES[name][1]))
    assert {n for n in declared if n.startswith('cb_lpx_')} == set(NEW_ENTRIES) == {n for n in _lib.SIGNATURES if 'lpx' in n}
    # no new name falls into a set that another host test closes
    for name in NEW_ENTRIES:
        assert not any(w in name for w in ('linkp', 'heur', 'rank_counts', 'ncloss', 'cosine')), name
        assert not name.startswith(('cb_pair_', 'cb_rank_loss', 'cb_sage_', 'cb_attn_')), name
    assert _lib.load().cb_lpx_max_tries() == xr.MAX_TRIES == int(re.search(r'#define CB_LPX_MAX_TRIES (\d+)', hdr).group(1))
    # the draws are shared with cb_linkp.hip through one header, not copied
    src = os.path.join(ROOT, 'gnn-tail-generalization_amd', 'csrc')
    for f in ('cb_linkp.hip', 'cb_lpx.hip'):
        text = open(os.path.join(src, f)).read()
        assert '#include "cb_draw.h"' in text and '__umul64hi' not in text, f


def test_bad_arguments_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()

    def view(**over):
        f = dict(rowptr=P8, col=P8, col_flags=0, n_rows=4, n_edges=4, hub_threshold=1, n_hubs=0, n_chunks=0, hub_rows=None, hub_chunk_ptr=None, ws=None,
                 ws_bytes=0)
        f.update(over)
        return ctypes.byref(_lib.CsrView(**f))
    # global negatives
    assert lib.cb_lpx_neg_global_i32(None, 3, 1, P8, P8, None) == -1
    assert lib.cb_lpx_neg_global_i32(view(col_flags=1), 3, 1, P8, P8, None) == -1 and b'flags' in lib.cb_last_error()
    assert lib.cb_lpx_neg_global_i32(view(col=None), 3, 1, P8, P8, None) == -1
    for n in (0, 1):
        assert lib.cb_lpx_neg_global_i32(view(n_rows=n), 3, 1, P8, P8, None) == -1 and b'N >= 2' in lib.cb_last_error()
    assert lib.cb_lpx_neg_global_i32(view(n_rows=2 ** 31), 3, 1, P8, P8, None) == -2
    assert lib.cb_lpx_neg_global_i32(view(), -1, 1, P8, P8, None) == -1
    assert lib.cb_lpx_neg_global_i32(view(), 2 ** 30, 1, P8, P8, None) == -2
    assert lib.cb_lpx_neg_global_i32(view(), 3, 1, None, P8, None) == -1 and b'null' in lib.cb_last_error()
    assert lib.cb_lpx_neg_global_i32(view(), 3, 1, P8, None, None) == -1
    assert lib.cb_lpx_neg_global_i32(view(), 0, 1, None, None, None) == 0                     # nothing to draw
    # local negatives
    assert lib.cb_lpx_neg_local_i32(P8, -1, 3, 10, 1, P8, None) == -1
    assert lib.cb_lpx_neg_local_i32(P8, 4, -3, 10, 1, P8, None) == -1
    assert lib.cb_lpx_neg_local_i32(P8, 4, 3, 1, 1, P8, None) == -1 and b'N >= 2' in lib.cb_last_error()
    assert lib.cb_lpx_neg_local_i32(P8, 4, 3, 2 ** 31, 1, P8, None) == -2
    assert lib.cb_lpx_neg_local_i32(P8, 2 ** 20, 2 ** 20, 10, 1, P8, None) == -2
    assert lib.cb_lpx_neg_local_i32(None, 4, 3, 10, 1, P8, None) == -1
    assert lib.cb_lpx_neg_local_i32(P8, 4, 3, 10, 1, None, None) == -1
    assert lib.cb_lpx_neg_local_i32(None, 0, 3, 10, 1, None, None) == 0
    # permutation
    assert lib.cb_lpx_permutation_workspace_bytes(0) == 0 and lib.cb_lpx_permutation_workspace_bytes(-3) == 0
    need = lib.cb_lpx_permutation_workspace_bytes(1000)
    assert need >= 2 * 1000 * 8
    assert lib.cb_lpx_permutation_i32(-1, 1, P8, P8, need, None) == -1
    assert lib.cb_lpx_permutation_i32(2 ** 31, 1, P8, P8, 2 ** 40, None) == -2 and b'2^31' in lib.cb_last_error()
    assert lib.cb_lpx_permutation_i32(2 ** 31 - 1, 1, P8, P8, 2 ** 40, None) == -2
    assert lib.cb_lpx_permutation_i32(1000, 1, None, P8, need, None) == -1
    assert lib.cb_lpx_permutation_i32(1000, 1, P8, None, need, None) == -3
    assert lib.cb_lpx_permutation_i32(1000, 1, P8, P8, need - 1, None) == -3 and b'workspace' in lib.cb_last_error()
    assert lib.cb_lpx_permutation_i32(0, 1, None, None, 0, None) == 0                          # a no-op
    # row ranks
    ok = [P8, 5, P8, 8, 8, P8, P8, P8, None]
    for at, val in ((1, -1), (4, -1), (3, 7), (7, None), (0, None), (2, None), (5, None), (6, None)):      # P, K, ld < K, status, pos, neg, gt, eq
        bad = list(ok)
        bad[at] = val
        assert lib.cb_lpx_row_ranks_f32(*bad) == -1, (at, val)
    for at, val in ((1, 2 ** 30), (4, 2 ** 31)):
        bad = list(ok)
        bad[at] = val
        bad[3] = max(bad[3], bad[4])
        assert lib.cb_lpx_row_ranks_f32(*bad) == -2, (at, val)
    # recall
    assert lib.cb_lpx_recall_topk_workspace_bytes(0, 0) == 0 and lib.cb_lpx_recall_topk_workspace_bytes(-1, 4) == 0
    assert lib.cb_lpx_recall_topk_workspace_bytes(2 ** 31, 2 ** 31) == 0
    need = lib.cb_lpx_recall_topk_workspace_bytes(300, 700)
    assert need >= 2 * 1000 * 8
    ok = [P8, 300, P8, 700, 5, P8, P8, P8, need, None]
    for at, val in ((1, -1), (3, -1), (4, -1), (0, None), (2, None), (5, None), (6, None)):
        bad = list(ok)
        bad[at] = val
        assert lib.cb_lpx_recall_topk_f32(*bad) == -1, (at, val)
    bad = list(ok)
    bad[1], bad[3] = 2 ** 31, 2 ** 31
    assert lib.cb_lpx_recall_topk_f32(*bad) == -2 and b'2^32' in lib.cb_last_error()
    bad = list(ok)
    bad[8] = need - 1
    assert lib.cb_lpx_recall_topk_f32(*bad) == -3 and b'workspace' in lib.cb_last_error()
    bad = list(ok)
    bad[7], bad[8] = None, 0
    assert lib.cb_lpx_recall_topk_f32(*bad) == -3


# ---- restatements against the reference's fixtures ------------------------------------------------------------------------------------------
def test_recall_restatement_equals_the_reference_exactly():
    cases = xr.load_golden()['recall']
    assert len(cases) == len(xr.RECALL_TOPKS) * (len(xr.RECALL_SIZES) + 1)
    sizes = sorted({(c['pos'].numel(), c['neg'].numel()) for c in cases})
    assert sizes == sorted(xr.RECALL_SIZES + [(6, 9)])
    assert {c['topk'] for c in cases} == set(xr.RECALL_TOPKS)
    tied_at_cut = 0
    for c in cases:
        pos, neg = c['pos'].numpy(), c['neg'].numpy()
        assert set(np.unique(2 * pos)) <= set(range(-2, 5)) and set(np.unique(2 * neg)) <= set(range(-2, 4))      # integers and half-integers
        num, P = xr.recall_parts(pos, neg, c['topk'])
        assert isinstance(num, int) and num / P == c['value'], (c['topk'], num, P, c['value'])
        if c['topk'] is not None and float(c['topk']) != 0:
            k = int(c['topk']) if float(c['topk']) > 5 else int(float(c['topk']) * P)
            assert xr.recall_threshold_form(pos, neg, k) == num
            kept = pos[pos > 0]
            M = np.sort(np.concatenate([kept, neg]))[::-1]
            if 0 < k < len(M) and M[k - 1] == M[k] and (kept == M[k]).any() and (neg == M[k]).any():
                tied_at_cut += 1
    assert tied_at_cut >= 3                                                                     # ties across the two sets at the cut
    nopos = [c for c in cases if c['pos'].numel() == 6]
    assert all(float(c['pos'].max()) <= 0 and c['value'] == 0.0 for c in nopos)


def test_threshold_form_equals_the_sort_on_random_tied_cases():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        P, Nn = int(rng.integers(1, 12)), int(rng.integers(0, 15))
        pos, neg = xr.half_integer_scores(rng, P, -1, 2), xr.half_integer_scores(rng, Nn, -1, 1.5)
        if Nn == 0 and not (pos > 0).any():
            continue
        k = int(rng.integers(0, P + Nn + 2))
        assert xr.recall_parts(pos, neg, str(k + 6))[0] == xr.recall_threshold_form(pos, neg, k + 6)
        kept = pos[pos > 0]
        order = np.argsort(-np.concatenate([kept, neg]).astype(np.float64), kind='stable')
        want = int(np.concatenate([np.ones(len(kept), dtype=np.int64), np.zeros(Nn, dtype=np.int64)])[order][:k].sum())
        assert want == xr.recall_threshold_form(pos, neg, k)


def test_shape_fixtures_and_their_properties():
    s = xr.load_golden()['shapes']
    loc = s['local']
    assert tuple(loc['out'].shape) == (11, 3, 2) and bool((loc['out'][:, :, 0] == loc['pos'][:, :1]).all())
    mine = xr.neg_local(loc['pos'].t().numpy(), loc['num_nodes'], loc['num_neg'], seed=3)
    view = torch.from_numpy(mine).t().reshape(11, 3, 2)                                     # column i k + j = entry [i, j]
    assert view.shape == loc['out'].shape and bool((view[:, :, 0] == loc['pos'][:, :1]).all())
    assert int(view[:, :, 1].min()) >= 0 and int(view[:, :, 1].max()) < loc['num_nodes']
    pc = s['perm_copy']
    n, k = pc['target_num_sample'], pc['num_perm_copy']
    assert tuple(pc['out'].shape) == (n, k, 2)
    chunks = pc['out'].reshape(k, n, 2)                                                       # the reference concatenates its copies before the reshape
    assert torch.equal(chunks[0], pc['edge_index'].t())
    for j in range(1, k):
        assert sorted(map(tuple, chunks[j].tolist())) == sorted(map(tuple, chunks[0].tolist()))
    ei = np.stack([np.arange(n), np.arange(n) + 100])
    cols = np.stack([np.arange(n)] + [xr.permutation(n, 9 + j).astype(np.int64) for j in range(1, k)], axis=1).reshape(-1)
    mine = ei[:, cols].T.reshape(n, k, 2)
    for j in range(k):
        assert sorted(map(tuple, mine[:, j].tolist())) == sorted(map(tuple, ei.T.tolist()))


@pytest.mark.parametrize('n', [0, 1, 2, 255, 256, 257, 5000])
def test_restated_permutation_is_one(n):
    a, b = xr.permutation(n, 0), xr.permutation(n, 2 ** 32 + 5)
    assert a.dtype == np.int32 and np.array_equal(np.sort(a), np.arange(n)) and np.array_equal(np.sort(b), np.arange(n))
    if n > 2:
        assert not np.array_equal(a, b)


@pytest.mark.parametrize('name', xr.GRAPHS)
def test_restated_global_negatives_are_no_edges_and_no_self_pairs(name):
    ei, n = xr.golden_graph(name)
    ei = ei.numpy()
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    accepted_reverse = 0
    for seed in (0, 2 ** 32 + 5):
        out, failed = xr.neg_global(ei, n, 900, seed)
        assert failed == 0 and out.min() >= 0 and out.max() < n
        for u, v in out.T.tolist():
            assert u != v and (u, v) not in edges
            accepted_reverse += (v, u) in edges
    if name == 'case_graph_asym_multi':
        assert accepted_reverse > 0                                                            # only the directed pair is tested
    perm, _ = xr.neg_global_perm(ei, n, 50, 3, 7)
    base, _ = xr.neg_global(ei, n, 50, 7)
    v = perm.T.reshape(50, 3, 2)
    assert np.array_equal(v[:, 0], base.T)
    for j in (1, 2):
        assert sorted(map(tuple, v[:, j].tolist())) == sorted(map(tuple, base.T.tolist())) and not np.array_equal(v[:, j], v[:, 0])
    # the complete directed graph on 3 nodes: every slot fails; two nodes and one edge: only 1 -> 0 is left
    full = np.array([[0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]])
    out, failed = xr.neg_global(full, 3, 10, 1)
    assert failed == 10 and (out == -1).all()
    out, failed = xr.neg_global(np.array([[0], [1]]), 2, 200, 0)
    assert failed == 0 and (out[0] == 1).all() and (out[1] == 0).all()


def test_brute_ranks_and_the_ogb_rule():
    pos = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0], dtype=np.float32)
    row = np.array([-0.0, 0.0, np.inf, -np.inf, 1.0], dtype=np.float32)
    neg = np.tile(row, (6, 1))
    neg[5, 2] = np.nan
    gt, eq, status = xr.row_ranks_brute(pos, neg)
    assert gt.tolist() == [2, 2, 0, 4, -1, -1] and eq.tolist() == [2, 2, 1, 1, -1, -1] and status == 2
    m = xr.mrr_ogb([0, 1, 0, 10], [0, 0, 2, 0])
    assert abs(m['MRR'] - (1 / 1 + 1 / 2 + 1 / 2 + 1 / 11) / 4) <= 4 * 2.0 ** -53 and m['hits@1'] == 0.25 and m['hits@3'] == 0.75 and m['hits@10'] == 0.75
    from gnn_tail_generalization_amd import ops
    got = ops.mrr_from_counts(torch.tensor([0, 1, 0, 10], dtype=torch.int32), torch.tensor([0, 0, 2, 0], dtype=torch.int32))
    assert abs(got['MRR'] - m['MRR']) <= 4 * 2.0 ** -53 and all(got[k] == m[k] for k in ('hits@1', 'hits@3', 'hits@10'))
    with pytest.raises(ValueError, match='NaN'):
        ops.mrr_from_counts(torch.tensor([0, -1], dtype=torch.int32), torch.tensor([0, -1], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.mrr_from_counts(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    assert [ops.recall_k(t, 8) for t in xr.RECALL_TOPKS] == [None, None, 6, 8, 10, 7, 200]


# ---- the reference's surface on CPU tensors -------------------------------------------------------------------------------------------------
def test_logger_prints_the_reference_text():
    from gnn_tail_generalization_amd.Link_prediction_model.logger import Logger
    g = xr.load_golden()['logger']
    lg = Logger(2)
    for run, rows in enumerate(g['record']):
        for r in rows:
            lg.add_result(run, r)
    assert len(g['record']) == 2 and all(len(r) == 3 for r in g['record'])
    for (run, last_best), want in g['text'].items():
        f = io.StringIO()
        lg.print_statistics(run, f=f, last_best=last_best)
        assert f.getvalue() == want, (run, last_best)
    assert g['text'][(0, False)] != g['text'][(0, True)] and g['text'][(None, False)] != g['text'][(None, True)]
    with pytest.raises(AssertionError):
        lg.add_result(2, (0.1, 0.2))


def test_get_pos_neg_edges_equals_the_reference_on_both_split_forms():
    from gnn_tail_generalization_amd.Link_prediction_model.utils import get_pos_neg_edges
    g = xr.load_golden()['edges']
    assert set(g) == {'edge', 'source_node'}
    for form, c in g.items():
        for split in ('valid', 'test'):
            pos, neg = get_pos_neg_edges(split, c['split_edge'])
            want_pos, want_neg = c['result'][split]
            assert torch.equal(pos, want_pos) and torch.equal(neg, want_neg), (form, split)
            assert pos.shape[1] == 2 and neg.shape[1] == 2
    with pytest.raises(KeyError):
        get_pos_neg_edges('valid', {'train': {}, 'valid': {}})


def test_the_surface_refuses_what_is_not_built():
    from gnn_tail_generalization_amd import _lib
    from gnn_tail_generalization_amd.Link_prediction_model import experiment, negative_sample as nsamp, utils as lpu
    pos = torch.zeros((4, 2), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='random_src'):
        nsamp.local_neg_sample(pos, 10, 3, random_src=True)
    with pytest.raises(_lib.HipExtensionError):
        nsamp.local_neg_sample(pos, 10, 3)
    with pytest.raises(ValueError, match='whole square'):                                      # an edge_index is not a graph
        nsamp.global_neg_sample(torch.zeros((2, 5), dtype=torch.int64), 10, 4, 3)
    with pytest.raises(ValueError, match='whole square'):
        lpu.get_pos_neg_edges('train', {'train': {'edge': pos}}, graph=object(), num_nodes=10, neg_sampler_name='global', num_neg=3)
    with pytest.raises(ValueError, match='rows of 3'):
        lpu.evaluate_mrr(None, torch.zeros(3), torch.zeros(7), torch.zeros(3), torch.zeros(6))
    for mode in ('logit', 'emb', 'xmc'):
        with pytest.raises(NotImplementedError, match=r'edge_LP\.py.*mutual_intermix'):
            experiment.refuse_edge_lp(types.SimpleNamespace(edge_lp_mode=mode))
    experiment.refuse_edge_lp(types.SimpleNamespace(edge_lp_mode=''))
    m = experiment.LinkPredictionModel.__new__(experiment.LinkPredictionModel)
    m.args, m.encoder_name = types.SimpleNamespace(edge_lp_mode='logit', num_neg=3), 'SAGE'
    with pytest.raises(NotImplementedError, match=r'edge_LP\.py'):
        m.test(None, {}, 10, None, 'hits')
    m.encoder_name = 'CN'
    assert m.train(None, {}, 10, 'global', 3) == -1.0
    m.encoder_name = 'SAGE'
    with pytest.raises(NotImplementedError, match='weight'):
        m.train(None, {'train': {'edge': pos, 'weight': torch.ones(4)}}, 10, 'global', 3)
    from gnn_tail_generalization_amd.trainer_link_prediction import result_keys
    assert result_keys('hits') == ['Hits@20', 'Hits@50', 'Hits@100'] and result_keys('mrr') == ['MRR'] and result_keys('recall_my@1.25') == ['recall@100%']
    with pytest.raises(ValueError):
        result_keys('auc')


def test_the_new_operators_reject_cpu_tensors():
    from gnn_tail_generalization_amd import _lib, ops
    from test_heur_host import _fake_graph
    with pytest.raises(_lib.HipExtensionError):
        ops.NegativeSampler(_fake_graph())
    with pytest.raises(ValueError, match='whole square'):
        ops.NegativeSampler(_fake_graph(n_cols=9))
    with pytest.raises(_lib.HipExtensionError):
        ops.seeded_permutation(10, 0, device='cpu')
    with pytest.raises(_lib.HipExtensionError):
        ops.local_negatives(torch.zeros((2, 3), dtype=torch.int64), 10, 2)
    with pytest.raises(_lib.HipExtensionError):
        ops.perm_copies(torch.zeros((2, 3), dtype=torch.int32), 2, 0)
    with pytest.raises(_lib.HipExtensionError):
        ops.row_rank_counts(torch.zeros(3), torch.zeros((3, 4)))
    with pytest.raises(_lib.HipExtensionError):
        ops.recall_at_topk(torch.zeros(3), torch.zeros(6), '1.25')
    with pytest.raises(_lib.HipExtensionError):
        ops.recall_numerator(torch.zeros(3), torch.zeros(6), 2)
    with pytest.raises(ValueError):
        ops.seeded_permutation(-1, 0, device='cpu')
    with pytest.raises(ValueError):
        ops.recall_at_topk(torch.zeros(0), torch.zeros(6), None)
