"""GPU: the samplers, the seeded permutation and the ranking metrics of the link-prediction experiment (csrc/cb_lpx.hip; ops.NegativeSampler,
seeded_permutation, row_rank_counts, mrr_from_counts, recall_at_topk).

Everything integer is compared bit for bit with the host restatement (tests/lpx_ref.py): the samplers and the permutation are pure functions of
(graph, seed, slot, try); the rank counts and the recall numerator are counts.  The MRR is a float64 mean of P terms 1 / rank, each of them the
correctly rounded quotient on both sides, so the two means differ by the summation order alone: |d| <= P 2^-53 value."""
import numpy as np
import pytest
import torch

import lpx_ref as xr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEEDS = (0, 2 ** 32 + 5)


def _graph(ei, n):
    from gnn_tail_generalization_amd.graph import CSRGraph
    return CSRGraph(torch.as_tensor(ei).to(DEV), n)


def _sampler(ei, n):
    from gnn_tail_generalization_amd import ops
    return ops.NegativeSampler(_graph(ei, n))


# ---- samplers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', xr.GRAPHS)
def test_samplers_equal_the_host_restatement_bit_for_bit(name):
    ei, n = xr.golden_graph(name)
    s = _sampler(ei, n)
    pos = torch.stack([torch.randint(0, n, (300,), generator=torch.Generator().manual_seed(3)), torch.arange(300) % n])
    for seed in SEEDS:
        for num_samples in (1, 7, 300):
            for k in (1, 3):
                want, failed = xr.neg_global(ei.numpy(), n, num_samples * k, seed)
                got = s.global_(num_samples, k, seed=seed)
                assert got.dtype == torch.int32 and got.shape == (2, num_samples * k) and failed == 0
                assert np.array_equal(got.cpu().numpy(), want), (name, seed, num_samples, k)
                assert torch.equal(s.global_(num_samples, k, seed=seed), got)                       # two calls, the same bits
                p = pos[:, :num_samples]
                got_l = s.local(p.to(DEV), k, seed=seed)
                assert np.array_equal(got_l.cpu().numpy(), xr.neg_local(p.numpy(), n, k, seed)), (name, seed, num_samples, k)
                want_p, _ = xr.neg_global_perm(ei.numpy(), n, num_samples, k, seed)
                got_p = s.global_perm(num_samples, k, seed=seed)
                assert np.array_equal(got_p.cpu().numpy(), want_p), (name, seed, num_samples, k)
                # every copy is a permutation of copy 0
                v = got_p.t().reshape(num_samples, k, 2).cpu()
                key0 = sorted(map(tuple, v[:, 0].tolist()))
                for j in range(1, k):
                    assert sorted(map(tuple, v[:, j].tolist())) == key0
    s.check()
    assert s.global_(0, 3).shape == (2, 0) and s.global_(5, 0).shape == (2, 0) and s.global_perm(4, 0).shape == (2, 0)


def test_a_complete_graph_fails_every_slot_and_check_reports_it():
    ei = torch.tensor([[0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]])
    s = _sampler(ei, 3)
    out = s.global_(5, 2, seed=1)
    assert bool((out == -1).all()) and int(s.failed.item()) == 10
    assert xr.neg_global(ei.numpy(), 3, 10, 1)[1] == 10
    with pytest.raises(RuntimeError, match='10 negative slot'):
        s.check()
    assert int(s.failed.item()) == 0
    s.check()


def test_two_nodes_one_edge_exercise_the_try_loop():
    ei = torch.tensor([[0], [1]])                       # the only non-edge with two distinct nodes is 1 -> 0: a quarter of the tries
    s = _sampler(ei, 2)
    for seed in SEEDS:
        want, failed = xr.neg_global(ei.numpy(), 2, 200, seed)
        got = s.global_(200, 1, seed=seed).cpu().numpy()
        assert np.array_equal(got, want) and failed == 0
        assert (got[0] == 1).all() and (got[1] == 0).all()
    s.check()


def test_local_keeps_the_source_and_reaches_the_last_node():
    ei, n = xr.golden_graph(xr.GRAPHS[0])
    s = _sampler(ei, n)
    pos = torch.tensor([[n - 1, 4, 4, n - 1, 0], [0, 1, 2, 3, n - 1]])
    got = s.local(pos.to(DEV), 3, seed=11).cpu()
    assert np.array_equal(got.numpy(), xr.neg_local(pos.numpy(), n, 3, 11))
    v = got.t().reshape(5, 3, 2)
    assert bool((v[:, :, 0] == pos[0].reshape(5, 1)).all())
    assert int(v[:, :, 1].min()) >= 0 and int(v[:, :, 1].max()) < n
    many = s.local(pos.to(DEV).to(torch.int32), 2000, seed=12)
    assert int(many[1].max()) == n - 1 and int(many[1].min()) == 0      # 10 000 draws over n nodes
    assert s.local(pos[:, :0].to(DEV), 3).shape == (2, 0)


# ---- permutation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [0, 1, 2, 255, 256, 257, 65537])
def test_permutation_equals_the_restatement_and_is_a_permutation(n):
    from gnn_tail_generalization_amd import ops
    seen = []
    for seed in SEEDS:
        got = ops.seeded_permutation(n, seed, device=DEV)
        assert got.dtype == torch.int32 and got.shape == (n,)
        g = got.cpu().numpy()
        assert np.array_equal(g, xr.permutation(n, seed)), (n, seed)
        assert np.array_equal(np.sort(g), np.arange(n))
        assert torch.equal(ops.seeded_permutation(n, seed, device=DEV), got)
        seen.append(g)
    if n > 2:
        assert not np.array_equal(seen[0], seen[1])


# ---- row ranks --------------------------------------------------------------------------------------------------------------------------
GRID = np.array([-1.5, -0.0, 0.0, 0.5, 2.0], dtype=np.float32)


def _grid_scores(rng, shape):
    x = GRID[rng.integers(0, len(GRID), shape)]
    flat = x.reshape(-1)
    if flat.size >= 8:
        flat[rng.integers(0, flat.size, 2)] = np.float32(np.inf), np.float32(-np.inf)
    return x


@pytest.mark.parametrize('P', [1, 5, 261])
@pytest.mark.parametrize('K', [1, 3, 63, 64, 65, 257, 1000])
def test_row_rank_counts_against_brute_force(P, K):
    from gnn_tail_generalization_amd import ops
    rng = np.random.default_rng(100 * P + K)
    pos = _grid_scores(rng, (P,))
    if P >= 5:
        pos[1], pos[2], pos[3] = np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0)
    wide = _grid_scores(rng, (P, K + 6))
    for off in (0, 1, 3):                                # a column slice: row stride K + 6 > K, rows off the 16-byte grid
        neg = wide[:, off:off + K]
        gt, eq, st = ops.row_rank_counts(torch.from_numpy(pos).to(DEV), torch.from_numpy(wide).to(DEV)[:, off:off + K], return_status=True)
        wg, we, ws = xr.row_ranks_brute(pos, neg)
        assert gt.dtype == torch.int32 and int(st.item()) == ws == 0
        assert np.array_equal(gt.cpu().numpy(), wg) and np.array_equal(eq.cpu().numpy(), we), (P, K, off)
    # contiguous rows, and NaNs: one in pos, one in a row
    neg = np.ascontiguousarray(wide[:, :K])
    posn, negn = pos.copy(), neg.copy()
    posn[0] = np.nan
    negn[P - 1, K // 2] = np.nan
    gt, eq, st = ops.row_rank_counts(torch.from_numpy(posn).to(DEV), torch.from_numpy(negn).to(DEV), return_status=True)
    wg, we, ws = xr.row_ranks_brute(posn, negn)
    assert int(st.item()) == ws == 2
    assert np.array_equal(gt.cpu().numpy(), wg) and np.array_equal(eq.cpu().numpy(), we)
    assert int(gt[0]) == int(eq[0]) == -1 and int(gt[P - 1]) == -1
    with pytest.raises(ValueError, match='NaN'):
        ops.mrr_from_counts(gt, eq)


def test_the_two_zeros_are_equal_and_the_infinities_are_numbers():
    from gnn_tail_generalization_amd import ops
    pos = torch.tensor([0.0, -0.0, float('inf'), float('-inf')], device=DEV)
    row = torch.tensor([-0.0, 0.0, float('inf'), float('-inf'), 1.0], device=DEV)
    gt, eq = ops.row_rank_counts(pos, row.repeat(4, 1))
    assert gt.tolist() == [2, 2, 0, 4] and eq.tolist() == [2, 2, 1, 1]


@pytest.mark.parametrize('P,K', [(1, 1), (261, 3), (500, 65)])
def test_mrr_from_counts_against_float64(P, K):
    from gnn_tail_generalization_amd import ops
    rng = np.random.default_rng(P + K)
    pos, neg = _grid_scores(rng, (P,)), _grid_scores(rng, (P, K))
    gt, eq = ops.row_rank_counts(torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV))
    got = ops.mrr_from_counts(gt, eq)
    wg, we, _ = xr.row_ranks_brute(pos, neg)
    want = xr.mrr_ogb(wg, we)
    err, bound = abs(got['MRR'] - want['MRR']), P * 2.0 ** -53 * want['MRR']
    print(f'P={P} K={K}: MRR {got["MRR"]:.6f}, error {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    for k in (1, 3, 10):
        assert got[f'hits@{k}'] == want[f'hits@{k}']
    assert 0.0 <= got['MRR'] <= 1.0


# ---- recall -----------------------------------------------------------------------------------------------------------------------------
def test_recall_equals_the_reference_fixtures_exactly():
    from gnn_tail_generalization_amd import ops
    cases = xr.load_golden()['recall']
    assert len(cases) == 7 * (len(xr.RECALL_SIZES) + 1)
    for c in cases:
        got = ops.recall_at_topk(c['pos'].to(DEV), c['neg'].to(DEV), c['topk'])
        assert isinstance(got, float) and got == c['value'], (c['topk'], got, c['value'])


@pytest.mark.parametrize('total', [255, 256, 257, 4097])
def test_recall_numerator_against_the_restatement(total):
    from gnn_tail_generalization_amd import ops
    rng = np.random.default_rng(total)
    P = total // 3
    pos, neg = xr.half_integer_scores(rng, P, -1, 2), xr.half_integer_scores(rng, total - P, -1, 1.5)
    pos[0], neg[0] = np.float32(-0.0), np.float32(-0.0)
    tp, tn = torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV)
    kept = pos[pos > 0]
    m = len(kept) + len(neg)
    M = np.sort(np.concatenate([kept, neg]))[::-1]
    # a cut inside a run of equal scores that both sets take part in
    ties = [k for k in range(1, m) if M[k - 1] == M[k] and (kept == M[k]).any() and (neg == M[k]).any()]
    assert ties
    for k in (0, 1, ties[0], ties[len(ties) // 2], m, m + 1):
        num, st = ops.recall_numerator(tp, tn, k)
        order = np.argsort(-np.concatenate([kept, neg]).astype(np.float64), kind='stable')
        want = int(np.concatenate([np.ones(len(kept), dtype=np.int64), np.zeros(len(neg), dtype=np.int64)])[order][:k].sum())
        assert int(num.item()) == want == xr.recall_threshold_form(pos, neg, k), (total, k)
        assert int(st.item()) == 0
    for topk in xr.RECALL_TOPKS:
        num, P_ = xr.recall_parts(pos, neg, topk)
        assert ops.recall_at_topk(tp, tn, topk) == num / P_
    bad = tn.clone()
    bad[3] = float('nan')
    num, st = ops.recall_numerator(tp, bad, 5)
    assert int(num.item()) == -1 and int(st.item()) == 1
    with pytest.raises(ValueError, match='NaN'):
        ops.recall_at_topk(tp, bad, '1.25')
    with pytest.raises(ValueError, match='nothing to rank'):
        ops.recall_at_topk(torch.tensor([-1.0, 0.0], device=DEV), torch.zeros(0, device=DEV), '1')


# ---- end to end on S-tiny ---------------------------------------------------------------------------------------------------------------
PLUMBING = ['--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1']
MODEL = ['--dataset=S-tiny', '--encoder=SAGE', '--predictor=MLP', '--loss_func=log_rank_loss', '--num_neg=3']


def _tool(argv, split_edge=None):
    import contextlib
    import io
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import run_linkpred
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        t = run_linkpred.main(list(argv) + PLUMBING, split_edge=split_edge)
    return t, out.getvalue()


def _model(seed=0):
    """(trainer, split_edge, model) on S-tiny at --dropout=0, parameters initialised under `seed`."""
    import contextlib
    import io
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import main as cb_main
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.Link_prediction_model.experiment import LinkPredictionModel
    from gnn_tail_generalization_amd.trainer_link_prediction import trainer
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(MODEL + PLUMBING)
        args.edge_lp_mode, args.random_seed = '', seed
        args.dropout = 0.0      # (the dataset's preset overrides --dropout: set where bits are compared against a second forward)
        cb_main.set_seed(args)
        t = trainer(args, 0)
        split = t.make_split_edge()
        model = LinkPredictionModel(args, t.data, t.device)
        model.param_init()
    return t, split, model


def _state(model):
    import copy
    return [copy.deepcopy(m.state_dict()) for m in (model.encoder, model.predictor, model.emb)]


def test_split_edges_parts_and_negatives(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    t, split, model = _model()
    ei = t.data.edge_index
    edges = set(map(tuple, ei.t().tolist()))
    target = ~t.data.train_mask
    where, total = {}, 0
    for s in ('train', 'valid', 'test'):
        pos, neg = split[s]['edge'], split[s]['edge_neg']
        assert pos.dtype == torch.int64 and pos.shape[1] == 2 and neg.shape[1] == 2 and pos.is_cuda
        total += pos.shape[0]
        for u, v in pos.tolist():
            assert (u, v) in edges and u != v
            assert where.setdefault((min(u, v), max(u, v)), s) == s            # both orientations of a pair land in one part
            if s != 'train':
                assert bool(target[u]) or bool(target[v])                        # an edge between two source nodes is train
        for u, v in neg.tolist():
            assert (u, v) not in edges and u != v                                # real negatives, never the positive itself
    assert total == int((ei[0] != ei[1]).sum()) and all(split[s]['edge'].shape[0] > 0 for s in split)
    assert sum(split[s]['edge_neg'].shape[0] for s in split) == ei.shape[1]
    from gnn_tail_generalization_amd.utils import split_edges
    again = split_edges(ei, t.data.x.shape[0], target_node_mask=target, seed=0)
    assert all(torch.equal(again[s][k], split[s][k]) for s in split for k in ('edge', 'edge_neg'))


def test_a_single_batch_epoch_reports_the_loss_of_its_pairs_bit_for_bit(tmp_path, monkeypatch):
    from gnn_tail_generalization_amd.Link_prediction_model import calculate_loss
    monkeypatch.chdir(tmp_path)
    t, split, model = _model()
    before = _state(model)
    P = int(split['train']['edge'].shape[0])
    loss = model.train(t.data, split, batch_size=P + 5, neg_sampler_name='global', num_neg=3)
    le = model.last_epoch
    assert model.steps == 1 and le['batch_sizes'] == [P] and isinstance(loss, float)
    perm = le['perm']
    assert torch.equal(torch.sort(perm).values, torch.arange(P, device=DEV)) and tuple(le['neg'].shape) == (P, 3, 2)
    edges = set(map(tuple, t.data.edge_index.t().tolist()))
    assert all((u, v) not in edges and u != v for u, v in le['neg'].reshape(-1, 2).tolist())
    for m, sd in zip((model.encoder, model.predictor, model.emb), before):      # back to the initial parameters
        m.load_state_dict(sd)
    model.encoder.train()
    model.predictor.train()
    h = model.embeddings(t.data)
    pos_out = model.predictor.score_pairs(h, le['pos'][perm].t())
    neg_out = model.predictor.score_pairs(h, le['neg'][perm].reshape(-1, 2).t())
    want = calculate_loss('log_rank_loss', pos_out, neg_out, 3)
    print(f'single batch: P = {P}, loss {loss!r}, recomputed {float(want.detach())!r}')
    assert loss == float(want.detach().double().item())


def test_three_batches_take_three_steps_and_report_their_weighted_mean(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    t, split, model = _model()
    P = int(split['train']['edge'].shape[0])
    bs = -(-P // 3) + 1
    for sampler in ('global', 'local', 'global_perm'):
        model.param_init()
        loss = model.train(t.data, split, batch_size=bs, neg_sampler_name=sampler, num_neg=3)
        le = model.last_epoch
        assert model.steps == 3 and le['batch_sizes'] == [bs, bs, P - 2 * bs] and sum(le['batch_sizes']) == P
        host = sum(float(v.item()) * n for v, n in zip(le['batch_losses'], le['batch_sizes'])) / P
        print(f'{sampler}: loss {loss!r}, host {host!r}')
        assert abs(loss - host) <= 1e-12 * abs(host) and np.isfinite(loss)
    # a state reset: the same seed gives the same first epoch
    torch.manual_seed(5)
    model.param_init()
    a = model.train(t.data, split, batch_size=bs, neg_sampler_name='global', num_neg=3)
    torch.manual_seed(5)
    model.param_init()
    assert model.steps == 0
    assert model.train(t.data, split, batch_size=bs, neg_sampler_name='global', num_neg=3) == a


def _source_node_form(split, n_nodes, k=5):
    g = torch.Generator().manual_seed(77)
    out = {'train': {'source_node': split['train']['edge'][:, 0].clone(), 'target_node': split['train']['edge'][:, 1].clone()}}
    for s in ('valid', 'test'):
        e = split[s]['edge']
        out[s] = {'source_node': e[:, 0].clone(), 'target_node': e[:, 1].clone(),
                  'target_node_neg': torch.randint(0, n_nodes, (e.shape[0], k), generator=g).to(e.device)}
    return out


@pytest.mark.parametrize('metric', ['hits', 'mrr', 'recall_my@1.25'])
def test_two_invocations_of_the_tool_agree(metric, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    argv = MODEL + [f'--eval_metric={metric}', '--neg_sampler=global', '--epochs=4', '--eval_steps=2', '--runs=2', '--batch_size=300', '--random_seed=3']
    split = None
    if metric == 'mrr':
        t0, sp, _ = _model()
        split = _source_node_form(sp, int(t0.data.x.shape[0]))
    runs = [_tool(argv, split_edge=split) for _ in range(2)]
    (a, text_a), (b, text_b) = runs
    assert a.losses == b.losses and a.results == b.results
    assert len(a.losses) == 2 and all(len(r) == 4 and np.isfinite(r).all() for r in a.losses)
    keys = {'hits': ['Hits@20', 'Hits@50', 'Hits@100'], 'mrr': ['MRR'], 'recall_my@1.25': ['recall@100%']}[metric]
    for run in a.results:
        assert len(run) == 2
        for res in run:
            assert list(res) == keys
            for value in res.values():
                assert len(value) == (3 if 'recall' in metric else 2) and all(0.0 <= float(v) <= 1.0 for v in value)
    assert a.model.steps > 0 and a.losses[0] != a.losses[1]                                   # param_init gave the second run new parameters
    strip = lambda s: '\n'.join(line for line in s.splitlines() if 'Training Time' not in line and not line.startswith('[data]'))      # noqa: E731
    assert strip(text_a) == strip(text_b)
    assert 'All runs:' in text_a and 'Run 02:' in text_a and 'Highest Eval Point' in text_a and f'Run: 02, Epoch: 04, Loss: {a.losses[1][3]:.4f}' in text_a


def test_the_cn_encoder_trains_nothing_and_scores_with_pair_scores(tmp_path, monkeypatch):
    from gnn_tail_generalization_amd import ops
    monkeypatch.chdir(tmp_path)
    t, _ = _tool(['--dataset=S-tiny', '--encoder=CN', '--eval_metric=hits', '--epochs=2', '--eval_steps=1', '--runs=1'])
    assert t.losses == [[-1.0, -1.0]] and t.model.encoder is None and t.model.optimizer is None
    sp, g = t.split_edge, t.model.graph
    score = {(s, k): ops.pair_scores(g, sp[s][k].t(), 'CN') for s in ('valid', 'test') for k in ('edge', 'edge_neg')}
    valid = ops.hits_at_k(score[('valid', 'edge')], score[('valid', 'edge_neg')], (20, 50, 100))
    test = ops.hits_at_k(score[('test', 'edge')], score[('test', 'edge_neg')], (20, 50, 100))
    for res in t.results[0]:
        assert res == {k: (valid[k], test[k]) for k in valid}
    assert float(score[('valid', 'edge')].max()) > 0
    t, _ = _tool(['--dataset=S-tiny', '--encoder=AA', '--eval_metric=recall_my@1.25', '--epochs=1', '--eval_steps=1', '--runs=1'])
    want = tuple(ops.recall_at_topk(ops.pair_scores(g2, sp2[s]['edge'].t(), 'AA'), ops.pair_scores(g2, sp2[s]['edge_neg'].t(), 'AA'), '1.25')
                 for g2, sp2 in [(t.model.graph, t.split_edge)] for s in ('valid', 'test'))
    assert t.results[0][0]['recall@100%'][1:] == want


def test_what_is_not_built_raises(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match=r'edge_LP\.py'):
        _tool(MODEL + ['--edge_lp_mode=logit', '--epochs=1', '--runs=1'])
    with pytest.raises(NotImplementedError, match='fast_pagerank'):
        _tool(['--dataset=S-tiny', '--encoder=PPR', '--epochs=1', '--runs=1'])
