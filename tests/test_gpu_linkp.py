"""GPU: the edge-wise (link-prediction) term of the teacher's step (csrc/cb_linkp.hip, ops.LinkSampler / linkp_loss_eva / cal_MRR,
trainer.training_loss_linkp and friends).

Samplers: bit for bit against the NumPy restatement on the host Philox (tests/linkp_ref.py).
Loss: against float64 (tests/linkp_ref.py) and the fixtures of the reference's utils.linkp_loss_eva (tests/golden/linkp_*.pt), with bounds derived
from the operands — u = 2^-24, gamma_n = n u / (1 - n u):
  score   the kernel adds D products in float32 in a fixed tree; every product passes through at most D roundings (its own, the lane's chain, the
          butterfly levels that add a non-zero partner), so |s - s64| <= gamma_D * sum_i |h_i t_i|                          =: ds_e
  loss    each term max(s, 0) - s y + log1p(exp(-|s|)) has derivative sigmoid(s) - y, of magnitude < 1; the terms are evaluated and summed in
          float64 from the float32 score and the mean is rounded once: |loss - loss64| <= mean_e ds_e + 2 u |loss64|
  dEmb    ds_e' = g (sigmoid(s_e) - y_e) / S has derivative <= g / (4 S) in s_e; a row is the float64 sum of ds_e' * other row, rounded once:
          |dEmb[r, c] - dEmb64[r, c]| <= sum_{contributions of r} ds_e / (4 S) * |other_c| + u * (|dEmb64[r, c]| + that sum)
  mrr     ranks are integers (the fixtures keep every negative four summation bounds away from its positive), the mean of 1 / rank is taken in
          float64 and rounded once: |mrr - mrr64| <= u * mrr64 + P * 2^-52
Every measured maximum is printed beside its bound (run with -s)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import linkp_ref as lr
import ncloss_ref as nr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = lr.EPS24


# ---- samplers -------------------------------------------------------------------------------------------------------------------------
def _sampler(ei, n, mask):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.graph import CSRGraph
    return ops.LinkSampler(CSRGraph(ei.to(DEV), n), mask.to(DEV))


def _half_mask(n, seed=0):
    m = torch.zeros(n, dtype=torch.bool)
    m[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:n // 2]] = True
    return m


def _sampler_graphs():
    out = {}
    ei, n = nr.graph('powerlaw')                                   # N = 300, half the nodes in train
    out['powerlaw300'] = (ei, n, _half_mask(n))
    for name in ('case_graph_powerlaw_d7_d64', 'case_graph_asym_multi'):
        out[name] = lr.golden_graph(name)
    return out


GRAPHS = _sampler_graphs()


@pytest.mark.parametrize('name', sorted(GRAPHS))
@pytest.mark.parametrize('mode', lr.MODES)
def test_samplers_equal_the_host_restatement_bit_for_bit(name, mode):
    ei, n, mask = GRAPHS[name]
    s = _sampler(ei, n, mask)
    for seed in (7, 2 ** 32 + 5, 2 ** 61 + 2 ** 33 + 1):           # seeds above 2^32: both key words in use
        want, k = lr.positives(ei.numpy(), n, mask.numpy(), mode, 333, seed)
        got = s.positives(mode, 333, seed=seed)
        assert got.dtype == torch.int32 and got.shape == (2, 333)
        assert np.array_equal(got.cpu().numpy(), want), (name, mode, seed)
        assert torch.equal(s.positives(mode, 333, seed=seed), got)                 # two calls, the same bits
        want_n, failed = lr.negatives(ei.numpy(), n, mask.numpy(), mode, 400, seed)
        got_n = s.negatives(mode, 399, seed=seed)                                  # rounded up to even
        assert got_n.shape == (2, 400) and failed == 0
        assert np.array_equal(got_n.cpu().numpy(), want_n), (name, mode, seed)
        assert torch.equal(s.negatives(mode, 400, seed=seed), got_n)
    s.check()
    assert s.positives(mode, 0).shape == (2, 0) and s.negatives(mode, 0).shape == (2, 0)
    # the device seed word of a captured step is added to the host seed, as the dropout kernels take it
    from gnn_tail_generalization_amd import ops
    word = 2 ** 40 + 17
    ops.set_graph_seed(torch.tensor([word], dtype=torch.int64, device=DEV))
    try:
        got, got_n = s.positives(mode, 64, seed=5), s.negatives(mode, 64, seed=5)
    finally:
        ops.set_graph_seed(None)
    assert np.array_equal(got.cpu().numpy(), lr.positives(ei.numpy(), n, mask.numpy(), mode, 64, 5 + word)[0])
    assert np.array_equal(got_n.cpu().numpy(), lr.negatives(ei.numpy(), n, mask.numpy(), mode, 64, 5 + word)[0])


@pytest.mark.parametrize('every', [1, 3])
def test_positive_walk_across_the_64_column_chunks_of_a_hub_row(every):
    """A star: the centre's row holds 200 columns.  every = 1: all neighbours are train nodes, valid position p is column p of the row (63 is the last
    lane of the first ballot, 64 the first lane of the second, 127 / 128 the same one chunk on).  every = 3: two neighbours in three are train nodes,
    so the same valid positions lie at other lanes and one chunk later.  Enough draws that each of those positions is drawn."""
    n = 201
    leaves = torch.arange(1, n)
    ei = torch.cat([torch.stack([leaves, torch.zeros_like(leaves)]), torch.stack([torch.zeros_like(leaves), leaves])], dim=1)
    mask = torch.ones(n, dtype=torch.bool)
    if every == 3:
        mask[leaves[leaves % 3 == 0]] = False
    T = int(mask[1:].sum())
    assert T > 129
    draws, seed = 6000, 2 ** 34 + 9
    want, k = lr.positives(ei.numpy(), n, mask.numpy(), 'train', draws, seed)
    src, dst = lr.valid_edges(ei.numpy(), n, mask.numpy(), 'train')
    assert (dst[:T] == 0).all() and len(src) == 2 * T                               # the centre's row comes first: k < T is a position in it
    assert {63, 64, 65, 127, 128} <= set(k[k < T].tolist())
    got = _sampler(ei, n, mask).positives('train', draws, seed=seed)
    assert np.array_equal(got.cpu().numpy(), want)


def test_exhausted_negative_slots_and_empty_modes():
    """A train set of two nodes joined by an edge: every train-mode negative slot exhausts its tries — the columns hold -1, the counter equals the slot
    count, check() raises and clears it; such columns are an error status of the loss, never an index.  A mode without a valid edge raises ValueError."""
    from gnn_tail_generalization_amd import ops
    ei, n = nr.graph('powerlaw')
    a, b = [(int(u), int(v)) for u, v in ei.t().tolist() if u != v][0]
    mask = torch.zeros(n, dtype=torch.bool)
    mask[[a, b]] = True
    s = _sampler(ei, n, mask)
    neg = s.negatives('train', 10, seed=3)
    want, failed = lr.negatives(ei.numpy(), n, mask.numpy(), 'train', 10, 3)
    assert failed == 5 and np.array_equal(neg.cpu().numpy(), want) and bool((neg == -1).all())
    assert int(s.failed.item()) == 5
    with pytest.raises(RuntimeError, match='5 negative slot'):
        s.check()
    s.check()                                                                       # cleared
    pos = s.positives('train', 50, seed=4)                                          # the two nodes' own edges and self loops
    assert np.array_equal(pos.cpu().numpy(), lr.positives(ei.numpy(), n, mask.numpy(), 'train', 50, 4)[0])
    emb = torch.randn(n, 8, device=DEV, requires_grad=True)
    loss, mrr, scores, status = ops.linkp_loss_eva(emb, pos, neg, return_parts=True)
    assert int(status) == 10 and bool(torch.isnan(loss)) and bool(torch.isnan(scores[50:]).all()) and bool(torch.isfinite(scores[:50]).all())
    loss.backward()
    touched = torch.zeros(n, dtype=torch.bool)
    touched[[a, b]] = True
    assert bool((emb.grad[~touched.to(DEV)] == 0).all())
    torch.cuda.synchronize()
    # no valid edge: a single train node without a self loop (train), every node a train node (test)
    ei2, n2, _ = lr.golden_graph('case_graph_asym_multi')
    loops = set(ei2[0][ei2[0] == ei2[1]].tolist())
    lonely = torch.zeros(n2, dtype=torch.bool)
    lonely[[v for v in range(n2) if v not in loops][0]] = True
    with pytest.raises(ValueError, match='no edge'):
        _sampler(ei2, n2, lonely).positives('train', 4)
    with pytest.raises(ValueError, match='no edge'):
        _sampler(ei2, n2, torch.ones(n2, dtype=torch.bool)).positives('test', 4)
    with pytest.raises(NotImplementedError):
        s.positives('all', 4)


# ---- loss, forward and backward -------------------------------------------------------------------------------------------------------
def _synthetic(N, D, P, Nn, seed, ld=None):
    g = torch.Generator().manual_seed(9000 + seed)
    emb = torch.randn(N, ld or D, generator=g) * 0.4
    pos = torch.randint(0, N, (2, P), generator=g)
    neg = torch.randint(0, N, (2, Nn), generator=g)
    return emb, pos, neg


def _loss_cases():
    cases = {name: None for name in lr.golden_cases()}
    for D in (4, 7, 64, 256, 300):
        cases[f'D{D}'] = dict(N=70, D=D, P=33, Nn=130, seed=D)
    cases['strided_ld80_D64'] = dict(N=70, D=64, P=33, Nn=130, seed=1, ld=80)
    cases['strided_ld9_D7'] = dict(N=70, D=7, P=33, Nn=130, seed=2, ld=9)
    cases['P1'] = dict(N=40, D=16, P=1, Nn=9, seed=3)
    cases['Nn0'] = dict(N=40, D=16, P=12, Nn=0, seed=4)
    return cases


LOSS_CASES = _loss_cases()


@pytest.mark.parametrize('name', sorted(LOSS_CASES))
def test_loss_mrr_and_gradient_against_float64(name):
    from gnn_tail_generalization_amd import ops
    spec = LOSS_CASES[name]
    golden = lr.load_case(name) if spec is None else None
    if golden is not None:
        full, pos, neg = golden['emb'], golden['pos'], golden['neg']
        D = full.shape[1]
    else:
        full, pos, neg = _synthetic(**spec)
        D = spec['D']
    emb = full[:, :D]                                             # a strided view where ld > D
    N, P, Nn, S = emb.shape[0], pos.shape[1], neg.shape[1], pos.shape[1] + neg.shape[1]
    loss64, mrr64, grad64, s64 = lr.loss_mrr_grad64(emb, pos, neg)
    dev_emb = full.to(DEV)[:, :D].requires_grad_(True)
    assert dev_emb.stride(0) == full.shape[1]
    idx_pos, idx_neg = (pos.to(DEV), neg.to(DEV)) if golden is not None else (pos.to(DEV).int(), neg.to(DEV).int())      # int64 and int32 both taken
    loss, mrr, scores, status = ops.linkp_loss_eva(dev_emb, idx_pos, idx_neg, return_parts=True)
    assert loss.dim() == 0 and mrr.dim() == 0 and loss.requires_grad and not mrr.requires_grad and int(status) == 0
    (grad,) = torch.autograd.grad(loss, dev_emb, retain_graph=True)
    (grad2,) = torch.autograd.grad(loss, dev_emb)
    assert torch.equal(grad, grad2)                                                  # bit-identical over two calls
    loss_b, mrr_b, scores_b, _ = ops.linkp_loss_eva(dev_emb, idx_pos, idx_neg, return_parts=True)
    assert torch.equal(loss_b, loss) and torch.equal(mrr_b, mrr) and torch.equal(scores_b, scores)
    # scores
    ad = torch.cat([lr.abs_dot(emb, pos), lr.abs_dot(emb, neg)])
    ds = lr.gamma(D) * ad
    err_s = (scores.cpu().double() - s64).abs()
    print(f'{name}: score error / bound max {float((err_s / ds.clamp(min=1e-300)).max()):.3f}')
    assert bool((err_s <= ds).all())
    # loss
    b_loss = float(ds.mean()) + 2 * U * abs(loss64)
    print(f'{name}: loss {float(loss.detach()):.8f} float64 {loss64:.8f} error {abs(float(loss.detach()) - loss64):.3e} bound {b_loss:.3e}')
    assert abs(float(loss.detach()) - loss64) <= b_loss
    # mrr: the ranks the fixture records (the reference's), or those of the device's own float32 scores
    if golden is not None:
        assert mrr64 == pytest.approx(golden['mrr'], abs=1e-12)
        want_mrr = golden['mrr']
        # the reference's own float32 evaluation: the same score bound, and a float32 mean of S terms in whatever order (gamma_{S + 8}: the sum and
        # at most eight roundings inside a term)
        b_ref_loss = float(ds.mean()) + lr.gamma(S + 8) * abs(loss64)
        print(f'{name}: reference loss {float(golden["loss"]):.8f} bound {b_ref_loss:.3e}')
        assert abs(float(golden['loss']) - float(loss.detach())) <= b_loss + b_ref_loss
    else:
        want_mrr, _ = lr.mrr_exact(scores[:P].cpu().double(), scores[P:].cpu().double())
    print(f'{name}: mrr {float(mrr):.8f} exact {want_mrr:.8f}')
    assert abs(float(mrr) - want_mrr) <= U * want_mrr + P * 2.0 ** -52
    if Nn < P:
        assert float(mrr) == 1.0
    # gradient
    other = torch.cat([torch.cat([pos[1], neg[1]]), torch.cat([pos[0], neg[0]])]).long()      # contribution to h_e reads t_e and the reverse
    dest = torch.cat([torch.cat([pos[0], neg[0]]), torch.cat([pos[1], neg[1]])]).long()
    first = torch.zeros(N, D, dtype=torch.float64).index_add_(0, dest, (torch.cat([ds, ds]) / (4 * S)).reshape(-1, 1) * emb.double()[other].abs())
    b_grad = first + U * (grad64.abs() + first)
    err_g = (grad.cpu().double() - grad64).abs()
    touched = torch.zeros(N, dtype=torch.bool)
    touched[dest] = True
    ratio = (err_g[touched] / b_grad[touched].clamp(min=1e-300)).max()
    print(f'{name}: dEmb error max {float(err_g.max()):.3e}, error / bound max {float(ratio):.3f}')
    assert bool((err_g <= b_grad).all())
    assert bool((grad.cpu()[~touched] == 0).all()) and grad.shape == (N, D)
    if golden is not None:
        # the reference's float32 gradient: the same propagated score error, then a float32 sum of the row's n_r terms in whatever order, each term
        # carrying at most eight roundings of its own (sigmoid, the label, 1 / S, the product): gamma_{n_r + 8} * sum |ds_e' other_c|
        y = torch.cat([torch.ones(P, dtype=torch.float64), torch.zeros(Nn, dtype=torch.float64)])
        dsp = ((torch.sigmoid(s64) - y) / S).abs()
        mag = torch.zeros(N, D, dtype=torch.float64).index_add_(0, dest, torch.cat([dsp, dsp]).reshape(-1, 1) * emb.double()[other].abs())
        n_r = torch.bincount(dest, minlength=N).double().reshape(-1, 1)
        b_ref = first + (n_r + 8) * U / (1 - (n_r + 8) * U) * mag
        err_ref = (grad.cpu().double() - golden['grad'].double()).abs()
        print(f'{name}: dEmb against the reference: error max {float(err_ref.max()):.3e}, error / bound max {float((err_ref / (b_grad + b_ref).clamp(min=1e-300)).max()):.3f}')
        assert bool((err_ref <= b_grad + b_ref).all())


@pytest.mark.parametrize('D', [4, 7, 300, 'slice8'])
def test_the_loss_scores_are_the_pair_dot_kernel(D):
    """One kernel behind both (cb_pair_core.h): the scores of the loss over pos | neg equal pair_dot over the concatenated pairs bit for bit — the
    float4 path (D = 4), the scalar path (7), more than one 256-column pass (300), and a column slice of a wider matrix — and both count the same
    unusable pairs, whose scores are NaN on both sides."""
    from gnn_tail_generalization_amd import ops
    N, P, Nn = 40, 5, 12
    if D == 'slice8':
        emb, pos, neg = _synthetic(N, 8, P, Nn, seed=12, ld=12)
        emb = emb.to(DEV)[:, :8]
        assert emb.stride(0) == 12
    else:
        emb, pos, neg = _synthetic(N, D, P, Nn, seed=D)
        emb = emb.to(DEV)
    neg[:, 3] = -1
    pos[1, 2] = N
    pos, neg = pos.to(DEV), neg.to(DEV)
    scores, status = ops.linkp_loss_eva(emb, pos, neg, return_parts=True)[2:]
    dot, dot_status = ops.pair_dot(emb, torch.cat([pos, neg], 1), return_status=True)
    nan = torch.zeros(P + Nn, dtype=torch.bool, device=DEV)
    nan[[2, P + 3]] = True
    assert torch.equal(torch.isnan(scores), nan) and torch.equal(torch.isnan(dot), nan)
    assert torch.equal(scores[~nan], dot[~nan]) and bool(torch.isfinite(dot[~nan]).all())
    assert int(status) == int(dot_status) == 2
    with pytest.raises(RuntimeError, match='2 pair'):
        ops.pair_check()


@pytest.mark.parametrize('D', [8, 300])
def test_the_loss_gradient_is_the_pair_scatter_with_the_bce_coefficient(D):
    """One scatter behind both: on inputs whose BCE coefficient is exact in fp32 the loss's gradient equals the scalar-coefficient scatter bit for
    bit.  Nodes 0..11 live in the first D / 2 columns and nodes 12..23 in the last, every pair joins the halves, so every score is exactly 0,
    sigmoid exactly 0.5, and with S = 64 and an upstream gradient of 1 the coefficient is -0.5 / 64 (positives) or +0.5 / 64 (negatives).  Node 0
    sits in 20 pairs (a long run of the sorted index); nodes 11 and 23 in none."""
    from gnn_tail_generalization_amd import ops
    N, P, Nn = 24, 16, 48
    S = P + Nn
    g = torch.Generator().manual_seed(300 + D)
    emb = torch.randn(N, D, generator=g)
    emb[:12, D // 2:] = 0
    emb[12:, :D // 2] = 0
    left, right = torch.randint(1, 11, (S,), generator=g), torch.randint(12, 23, (S,), generator=g)
    left[::3][:20] = 0
    pairs = torch.stack([left, right])
    pairs[:, 1::2] = pairs[:, 1::2].flip(0)      # both orientations
    assert int((pairs == 0).sum()) == 20 and not bool(((pairs == 11) | (pairs == 23)).any())
    pairs = pairs.to(DEV)
    pos, neg = pairs[:, :P].contiguous(), pairs[:, P:].contiguous()
    dev_emb = emb.to(DEV).requires_grad_(True)
    loss, _, scores, status = ops.linkp_loss_eva(dev_emb, pos, neg, return_parts=True)
    assert bool((scores == 0.0).all()) and int(status) == 0      # the premise: sigmoid is exactly 0.5 everywhere
    (grad,) = torch.autograd.grad(loss, dev_emb)
    coef = torch.cat([torch.full((P,), -0.5 / S), torch.full((Nn,), 0.5 / S)]).to(DEV)
    assert coef.dtype == torch.float32
    want = ops._pair_scatter_raw(dev_emb.detach(), pairs.to(torch.int32).contiguous(), coef)
    assert torch.equal(grad, want)
    assert bool((grad[[11, 23]] == 0).all()) and bool((grad[0] != 0).any()) and bool((grad[0, :D // 2] == 0).all())


def test_mrr_of_held_scores_ties_and_the_thin_forms_of_utils():
    from gnn_tail_generalization_amd import ops, utils
    f = lambda *v: torch.tensor(v, dtype=torch.float32, device=DEV)      # noqa: E731
    assert float(ops.cal_MRR(f(1.0), f(1.0, 2.0))) == 0.5                # the tie counts for the positive: rank 2, not 3
    assert float(ops.cal_MRR(f(1.0, 5.0), f(3.0, 0.0, 9.0, 9.0, 7.0))) == pytest.approx((1 / 2 + 1 / 3) / 2, abs=1e-7)      # k = 2, the last one dropped
    assert float(ops.cal_MRR(f(1.0, 5.0), f(3.0))) == 1.0                # k = 0
    c = lr.load_case('linkp_n50_d10_p7_n30')
    emb = c['emb'].to(DEV).requires_grad_(True)
    pos, neg = c['pos'].to(DEV), c['neg'].to(DEV)
    loss, mrr = utils.linkp_loss_eva(emb[pos[0]], emb[pos[1]], emb[neg[0]], emb[neg[1]])
    want, want_mrr = ops.linkp_loss_eva(emb, pos, neg)
    assert torch.equal(loss, want) and torch.equal(mrr, want_mrr)
    loss.backward()
    (g,) = torch.autograd.grad(want, emb)
    torch.testing.assert_close(emb.grad, g, atol=1e-7, rtol=1e-5)       # (torch's index backward adds in another order)
    sc = utils.calc_score(emb[pos[0]], emb[pos[1]])
    assert torch.equal(sc, ops.linkp_loss_eva(emb, pos, neg, return_parts=True)[2][:7])
    assert float(utils.cal_MRR(sc, utils.calc_score(emb[neg[0]], emb[neg[1]]))) == pytest.approx(c['mrr'], abs=1e-7)


# ---- trainer --------------------------------------------------------------------------------------------------------------------------
def _trainer(nodewise, epochs=5, seed=0, extra=()):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(['--dataset=S-tiny', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=111', '--se_reg=0.5',
                                            '--manual_assign_GPU=0', '--do_deg_analyze=0', f'--epochs={epochs}'] + list(extra))
        args.random_seed = seed
        args.has_loss_component_edgewise, args.has_loss_component_nodewise = True, bool(nodewise)
        torch.manual_seed(seed)
        np.random.seed(seed)
        t = trainer(args, seed)
    ops.set_graph_seed(None)
    return t


@pytest.mark.parametrize('nodewise', [0, 1])
def test_one_step_gradients_match_the_oracle_on_the_same_sampled_edges(nodewise, tmp_path, monkeypatch):
    """training_loss_linkp() against the CPU oracle's teacher carried through the reference formula (trainer…:386-394, 417-426; utils.py:754-774) on
    the edges this very step sampled; tolerances: those of the step-parity tests of this model (tests/test_gpu_trainer.py, tests/test_gpu_model.py)."""
    import coldbrew_oracle as orc
    import torch.nn.functional as F
    monkeypatch.chdir(tmp_path)
    t = _trainer(nodewise)
    t.args.dropout = 0.0
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(0)
        t.setup_teacherGNN()
    a, m = t.args, t.teacherGNN
    assert not a.has_proj2class
    m.train()
    samples = {}
    real = t.gen_pn_edge_index
    monkeypatch.setattr(t, 'gen_pn_edge_index', lambda mode: samples.setdefault(mode, real(mode)))
    loss, mrr_train, mrr_test = t.training_loss_linkp()
    t.optimizer.zero_grad()
    loss.backward()
    t.link_sampler().check()
    pos, neg = (v.cpu().long() for v in samples['train'])
    assert pos.shape == (2, a.samp_size_p) and neg.shape == (2, a.samp_size_n_train) and samples['test'][1].shape[1] == a.samp_size_p * a.samp_size_n_test_times_p
    n = t.data.x.shape[0]
    cfg = orc.make_cfg(type_trick=a.type_trick, num_layers=a.num_layers, num_feats=a.num_feats, dim_hidden=a.dim_hidden, num_classes=a.num_classes,
                       res_alpha=a.res_alpha, layer_agg=a.layer_agg, whetherHasSE=tuple(int(c) for c in a.whetherHasSE), se_reg=a.se_reg)
    sd = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in m.state_dict().items()}
    csr = orc.build_csr(t.data.edge_index.cpu(), n)
    o, reg = orc.teacher_forward(cfg, sd, t.data.x.cpu(), csr, training=True)
    ref = None
    if nodewise:
        ref = orc.training_loss(cfg, o, reg, t.data.y.cpu(), t.data.train_mask.cpu()) * a.TeacherGNN.lossa_semantic      # (lossa_semantic == 1)
        assert a.TeacherGNN.lossa_semantic == 1
    score = torch.cat([(o[pos[0]] * o[pos[1]]).sum(-1), (o[neg[0]] * o[neg[1]]).sum(-1)]).view(-1, 1)
    label = torch.cat([torch.ones(pos.shape[1], 1), torch.zeros(neg.shape[1], 1)])
    structure = F.binary_cross_entropy_with_logits(score, label) * a.TeacherGNN.lossa_structure
    ref = structure if ref is None else ref + structure
    ref.backward()
    print(f'nodewise {nodewise}: loss {float(loss.detach()):.7f} oracle {float(ref):.7f}; MRR train {float(mrr_train):.4f} test {float(mrr_test):.4f}')
    torch.testing.assert_close(loss.detach().cpu(), ref.detach(), atol=1e-5, rtol=1e-5)
    k = neg.shape[1] // pos.shape[1]
    assert 1 / (1 + k) <= float(mrr_train) <= 1 and 0 < float(mrr_test) <= 1
    checked = 0
    for k, p_ in m.named_parameters():
        want = sd[k].grad
        if p_.grad is None:
            assert want is None or not bool(want.abs().sum()), k
            continue
        assert want is not None, k
        torch.testing.assert_close(p_.grad.cpu(), want, atol=2e-5, rtol=2e-4, msg=lambda s_, k=k: f'{k}: {s_}')
        checked += 1
    assert checked >= 4


def test_training_records_are_finite_and_repeat_bit_for_bit(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    recs = []
    for _ in range(2):
        t = _trainer(1, epochs=5, seed=3)
        with contextlib.redirect_stdout(io.StringIO()):
            torch.manual_seed(3)
            recs.append(t.train_teacherGNN_linkp())
    assert recs[0].shape == (5, 5) and np.isfinite(recs[0]).all()
    assert (recs[0][3] >= 0.5).all() and (recs[0][3] <= 1).all() and (recs[0][4] > 0).all() and (recs[0][4] <= 1).all()
    assert np.array_equal(recs[0], recs[1])


def test_train_mrr_rises_when_only_the_edge_loss_is_trained(tmp_path, monkeypatch):
    """The direction is what is tested: 30 epochs on the edge-wise term alone leave the train MRR above its value at epoch 0."""
    monkeypatch.chdir(tmp_path)
    t = _trainer(0, epochs=30, seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(1)
        rec = t.train_teacherGNN_linkp()
    print('train MRR by epoch', np.round(rec[3], 3).tolist())
    assert rec.shape == (5, 30) and np.isfinite(rec).all()
    assert rec[3][-1] > rec[3][0]
    assert 0 < t.evaluate_linkp(t.teacherGNN, 'test') <= 1


def test_the_refused_paths_are_still_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    t = _trainer(1)
    with contextlib.redirect_stdout(io.StringIO()):
        t.setup_teacherGNN()
    with pytest.raises(NotImplementedError, match='only the train rows'):
        t.training_loss()
    with pytest.raises(NotImplementedError, match='I2_GTL'):
        t.run_trainSet()
    t.args.has_loss_component_edgewise = False
    with pytest.raises(ValueError, match='has_loss_component_edgewise'):
        t.training_loss_linkp()


def test_tool_end_to_end(tmp_path, monkeypatch):
    import os
    import sys
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkp
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkp.main(['--dataset=S-tiny', '--epochs=3', '--nodewise=1', '--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0',
                                 '--do_deg_analyze=0', '--N_exp=1'])
    assert len(recs) == 1 and recs[0].shape == (5, 3) and np.isfinite(recs[0]).all()
    with pytest.raises(SystemExit):
        train_linkp.main(['--nodewise=2'])
