"""GPU: the CN / AA pair scores and the rank counts behind Hits@K / AUC (csrc/cb_heur.hip; ops.pair_scores / rank_counts / hits_at_k / auc;
Link_prediction_baseline.heuristics; trainer.evaluate_linkp_heuristic; tools/eval_linkp_baselines.py).

Contract (nothing here is a measured tolerance):
  CN      exact: the integer sum_k A[s, k] A[d, k] as fp32 (all fixture scores are far below 2^24)
  AA      and any weighted score: a sum of non-negative terms in float64 rounded once; against the float64 restatement r,
          |score - r| <= 2^-24 r (1 + 2^-16) — one fp32 rounding, and n 2^-53 (n far below 2^37) for the summation order and the device's log / division
  gt, eq  exact integers; Hits@K and AUC equal the float64 value of their formulas on brute-force counts
The restatement and the fixtures of the unmodified reference are loaded once (tests/heur_ref.py) and shared."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

import heur_ref as hr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_GRAPHS = {}


def _graph(name):
    from gnn_tail_generalization_amd.graph import CSRGraph
    if name not in _GRAPHS:
        c = hr.load_case(name)
        _GRAPHS[name] = CSRGraph(c['edge_index'].to(DEV), int(c['N']))
    return _GRAPHS[name]


def _check_scores(name, cn, aa, idx=None):
    c = hr.load_case(name)
    sel = slice(None) if idx is None else idx
    assert cn.dtype == torch.float32 and aa.dtype == torch.float32
    assert np.array_equal(cn.cpu().numpy().astype(np.float64), c['cn64'][sel])
    assert torch.equal(cn.cpu(), c['cn'][sel])                                               # the reference's own CN
    got, r = aa.cpu().numpy().astype(np.float64), c['aa64'][sel]
    ratio = np.abs(got - r) / np.maximum(hr.AA_REL_BOUND * r, 1e-300)
    print(f'{name}: AA error / bound max {float(ratio.max()):.3f} over {len(r)} pairs')
    assert hr.within_aa_bound(got, r).all()


@pytest.mark.parametrize('name', hr.golden_cases())
def test_pair_scores_against_the_restatement_and_the_reference(name):
    from gnn_tail_generalization_amd import ops
    c, g = hr.load_case(name), _graph(name)
    assert (not g.symmetric) or name != 'heur_asym_multi'
    pairs = c['pairs'].to(DEV)
    cn, aa = ops.pair_scores(g, pairs, 'CN'), ops.pair_scores(g, pairs, 'AA')
    assert cn.shape == aa.shape == (pairs.shape[1],)
    _check_scores(name, cn, aa)
    # the reference's own AA lies within the same bound of r, so the two lie within twice the bound of each other
    assert (np.abs(aa.cpu().numpy().astype(np.float64) - c['aa'].numpy().astype(np.float64)) <= 2 * hr.AA_REL_BOUND * c['aa64']).all()
    # int32 and int64 pairs, two calls: the same bits
    assert torch.equal(ops.pair_scores(g, pairs.int(), 'CN'), cn) and torch.equal(ops.pair_scores(g, pairs.int(), 'AA'), aa)
    assert torch.equal(ops.pair_scores(g, pairs, 'AA'), aa) and torch.equal(ops.pair_scores(g, pairs, 'CN'), cn)
    # the group width is not part of the result: CN exactly, AA within the bound
    for group in (16, 64):
        _check_scores(name, ops.pair_scores(g, pairs, 'CN', group=group), ops.pair_scores(g, pairs, 'AA', group=group))
    # P = 1, 5 and 257 (more than one block of 16 pairs; the last block partly filled)
    n_pairs = pairs.shape[1]
    for P in (1, 5, 257):
        idx = (np.arange(P) * 7 + 3) % n_pairs
        sub = pairs[:, torch.from_numpy(idx).to(DEV)]
        _check_scores(name, ops.pair_scores(g, sub, 'CN'), ops.pair_scores(g, sub, 'AA'), idx)
    empty = ops.pair_scores(g, pairs[:, :0], 'AA')
    assert empty.shape == (0,) and empty.dtype == torch.float32
    # the AA weights are built once and kept on the graph
    w = ops.aa_weights(g)
    assert w is ops.aa_weights(g) and w.dtype == torch.float64
    want_w = hr.aa_weights(c['A'])
    assert (np.abs(w.cpu().numpy() - want_w) <= 4 * 2.0 ** -53 * want_w).all() and ((w.cpu().numpy() == 0) == (want_w == 0)).all()
    # resource allocation: weight = 1 / c (0 where the column is empty), held to the restatement with that weight
    col_sum = c['A'].sum(axis=0)
    ra_w = np.where(col_sum > 0, 1.0 / np.maximum(col_sum, 1.0), 0.0)
    ra = ops.pair_scores(g, pairs, 'AA', weight=torch.from_numpy(ra_w).to(DEV))
    assert hr.within_aa_bound(ra.cpu().numpy(), hr.weighted64(c['A'], c['pairs'].numpy(), ra_w)).all()
    ones = ops.pair_scores(g, pairs, 'AA', weight=torch.ones(int(c['N']), dtype=torch.float64, device=DEV))
    assert torch.equal(ones, cn)                                                             # unit weights: the float64 sum of integers is CN
    with pytest.raises(ValueError, match='float64'):
        ops.pair_scores(g, pairs, 'AA', weight=torch.ones(int(c['N']), device=DEV))
    ops.pair_scores_check()


def test_out_of_range_endpoints_are_never_an_index():
    from gnn_tail_generalization_amd import ops
    c, g = hr.load_case('heur_rows'), _graph('heur_rows')
    ops.pair_scores_check()
    pairs = c['pairs'].clone()
    bad_at = 17
    pairs[1, bad_at] = int(c['N'])
    for kind, want in (('CN', c['cn']), ('AA', None)):
        score, status = ops.pair_scores(g, pairs.to(DEV), kind, return_status=True)
        assert int(status) == 1 and bool(torch.isnan(score[bad_at]))
        keep = torch.arange(pairs.shape[1]) != bad_at
        assert bool(torch.isfinite(score.cpu()[keep]).all())
        if want is not None:
            assert torch.equal(score.cpu()[keep], want[keep])
    with pytest.raises(RuntimeError, match='2 pair'):
        ops.pair_scores_check()
    ops.pair_scores_check()                                                                  # cleared
    pairs[0, 3], pairs[0, 4] = -1, 2 ** 31 - 1
    _, status = ops.pair_scores(g, pairs.to(DEV).int(), 'CN', return_status=True)
    assert int(status) == 3
    with pytest.raises(RuntimeError, match='3 pair'):
        ops.pair_scores_check()
    from gnn_tail_generalization_amd.Link_prediction_baseline import heuristics as H
    with pytest.raises(RuntimeError, match='outside'):
        H.CN(g, pairs)
    ops.pair_scores_check()


# ---- rank counts ----------------------------------------------------------------------------------------------------------------------
def _rank_inputs(P, Nn, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'ties':
        pos, neg = rng.integers(-3, 4, P).astype(np.float32), rng.integers(-3, 4, Nn).astype(np.float32)
    elif kind == 'equal':
        pos, neg = np.full(P, 2.5, np.float32), np.full(Nn, 2.5, np.float32)
    elif kind == 'real':
        pos, neg = rng.standard_normal(P).astype(np.float32), rng.standard_normal(Nn).astype(np.float32)
        if Nn:
            pos[::3] = neg[rng.integers(0, Nn, len(pos[::3]))]                               # exact ties among real values
    else:                                                                                    # 'special': +-inf, +-0, denormals, extremes
        pool = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1.0, -1.0], dtype=np.float32)
        pos, neg = pool[rng.integers(0, len(pool), P)], pool[rng.integers(0, len(pool), Nn)]
    return pos, neg


@pytest.mark.parametrize('P,Nn', [(1, 1), (1, 0), (65, 257), (300, 5000)])
@pytest.mark.parametrize('kind', ['ties', 'equal', 'real', 'special'])
def test_rank_counts_are_exact(P, Nn, kind):
    from gnn_tail_generalization_amd import ops
    pos, neg = _rank_inputs(P, Nn, kind, seed=P + 3 * Nn)
    want_gt, want_eq = hr.rank_counts_brute(pos, neg)
    tp, tn = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV)
    gt, eq, status = ops.rank_counts(tp, tn, return_status=True)
    assert gt.dtype == torch.int32 and eq.dtype == torch.int32 and gt.shape == eq.shape == (P,) and int(status) == 0
    assert np.array_equal(gt.cpu().numpy(), want_gt) and np.array_equal(eq.cpu().numpy(), want_eq)
    gt2, eq2 = ops.rank_counts(tp, tn)
    assert torch.equal(gt2, gt) and torch.equal(eq2, eq)
    ks = (1, 20, 50, 100)
    hits = ops.hits_at_k(tp, tn, ks)
    for k in ks:
        assert hits[f'Hits@{k}'] == hr.hits_brute(pos, neg, k)
        if Nn < k:
            assert hits[f'Hits@{k}'] == 1.0
    if Nn:
        assert ops.auc(tp, tn) == hr.auc_brute(pos, neg)
    else:
        assert not bool(gt.any()) and not bool(eq.any())
        with pytest.raises(ValueError):
            ops.auc(tp, tn)


def test_signed_zeros_infinities_and_nans():
    from gnn_tail_generalization_amd import ops
    f = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)      # noqa: E731
    gt, eq = ops.rank_counts(f(-0.0, 0.0), f(0.0, -0.0, 0.0, 1e-45, -1e-45))
    assert gt.tolist() == [1, 1] and eq.tolist() == [3, 3]
    inf = float('inf')
    gt, eq = ops.rank_counts(f(inf, -inf, 3.0e38), f(inf, -inf, -inf, 0.0, 3.4e38))
    assert gt.tolist() == [0, 3, 2] and eq.tolist() == [1, 2, 0]
    nan = float('nan')
    for pos, neg, n in ((f(1.0, nan), f(0.0, 2.0, 3.0), 1), (f(1.0, 2.0), f(nan, 2.0, -nan), 2), (f(nan), f(nan), 2)):
        gt, eq, status = ops.rank_counts(pos, neg, return_status=True)
        assert int(status) == n and bool((gt == -1).all()) and bool((eq == -1).all())
        with pytest.raises(ValueError, match='NaN'):
            ops.hits_at_k(pos, neg, (20,))
        with pytest.raises(ValueError, match='NaN'):
            ops.auc(pos, neg)
    gt, eq, status = ops.rank_counts(f(nan, 1.0), f(), return_status=True)                   # a NaN with no negative to sort
    assert int(status) == 1 and gt.tolist() == [-1, -1]
    # a constant scorer: MRR with ties for the positive says 1, these say chance
    z = torch.zeros(40, device=DEV)
    assert float(ops.cal_MRR(z[:10], z)) == 1.0 and ops.auc(z[:10], z) == 0.5 and ops.hits_at_k(z[:10], z, (20,))['Hits@20'] == 0.0


# ---- both surfaces --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', hr.golden_cases())
def test_the_reference_surface_returns_the_fixture_values(name):
    import types
    from gnn_tail_generalization_amd.Link_prediction_baseline import heuristics as H
    c, g = hr.load_case(name), _graph(name)
    for edge_index in (c['pairs'], c['pairs'].to(DEV), c['pairs'].numpy()):                  # host tensor, device tensor, numpy
        cn, back = H.CN(g, edge_index)
        assert back is edge_index and cn.dtype == torch.float32 and cn.device.type == 'cpu' and torch.equal(cn, c['cn'])
        aa, _ = H.AA(g, edge_index, batch_size=7)                                            # accepted and ignored
        assert aa.device.type == 'cpu' and hr.within_aa_bound(aa.numpy(), c['aa64']).all()
    data = types.SimpleNamespace(edge_index=c['edge_index'].to(DEV), num_nodes=int(c['N']))
    got = H.eva_heuristics_v2_dec25('CN', data, c['pairs'])
    assert isinstance(got, np.ndarray) and np.array_equal(got, c['cn'].numpy())
    cached = data.A
    got = H.eva_heuristics_v2_dec25('AA', data, c['pairs'].to(DEV))
    assert data.A is cached and hr.within_aa_bound(got, c['aa64']).all()
    with pytest.raises(NotImplementedError, match='fast_pagerank'):
        H.eva_heuristics_v2_dec25('PPR', data, c['pairs'])


def _trainer(seed=0):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(['--dataset=S-tiny', '--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0',
                                            '--epochs=1'])
        args.random_seed = seed
        args.has_loss_component_edgewise, args.has_loss_component_nodewise = True, True
        torch.manual_seed(seed)
        np.random.seed(seed)
        t = trainer(args, seed)
    ops.set_graph_seed(None)
    return t


def test_trainer_baseline_evaluation_is_finite_and_repeats(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    t = _trainer()
    with contextlib.redirect_stdout(io.StringIO()):
        t.setup_teacherGNN()
    for kind in ('CN', 'AA'):
        for mode in ('train', 'test'):
            torch.manual_seed(11)
            a = t.evaluate_linkp_heuristic(kind, mode)
            torch.manual_seed(11)
            b = t.evaluate_linkp_heuristic(kind, mode)
            assert set(a) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and a == b
            assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in a.values()), a
            assert a['Hits@20'] <= a['Hits@50'] <= a['Hits@100']
            print(kind, mode, a)
    with pytest.raises(NotImplementedError):
        t.evaluate_linkp_heuristic('CN', 'all')
    with pytest.raises(NotImplementedError):
        t.evaluate_linkp_heuristic('PPR', 'test')
    # the refused entry points of the link-prediction path stay refused
    with pytest.raises(NotImplementedError, match='only the train rows'):
        t.training_loss()
    with pytest.raises(NotImplementedError, match='I2_GTL'):
        t.run_trainSet()


def test_tool_end_to_end(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import eval_linkp_baselines
    rows = eval_linkp_baselines.main(['--dataset=S-tiny', '--kinds', 'CN', 'AA', '--samp_size_p=64', '--neg_per_pos=4', '--use_special_split=0',
                                      '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0'])
    out = capsys.readouterr().out
    assert [r[0] for r in rows] == ['CN', 'AA']
    for kind, res in rows:
        assert set(res) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and all(0.0 <= v <= 1.0 for v in res.values())
        assert any(line.startswith(kind) and 'Hits@20' in line and 'AUC' in line for line in out.splitlines())
    with pytest.raises(SystemExit):
        eval_linkp_baselines.main(['--dataset=S-tiny', '--kinds', 'PPR'])
