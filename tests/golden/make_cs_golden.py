"""Generates the Correct & Smooth fixtures tests/golden/cs_*.pt from the *unmodified* reference on the CPU (build container only).

    python tests/golden/make_cs_golden.py

The reference's Label_propagation_model.outcome_correlation functions are driven the way LPStep drives them (LP_Adj.py:126-157: train_only=True,
display=False) with device='cpu' passed explicitly; LP_Adj itself does not import here (its diffusion features need packages that are absent), so
LPStep's three lines of glue are restated by the call below.  Every file stores the inputs, the reference's res_result / result, the accuracies
before and after (trainer_node_classification.evaluate) and ref_err64 = max |reference - fp64 restatement (tests/cs_ref.py)|.

A seed is rejected when a row's top-two gap in the model's probabilities or in the reference's result is below 1e-4 (an argmax a float32 rounding
could flip: the tests compare accuracies exactly).  One kind of row cannot meet that and is judged by the value BEFORE the last clamp instead: with
AD as the smoothing matrix the hub rows of a power-law graph sum hundreds of neighbours and saturate at the clamp's upper bound in several classes on
every seed (the hub of make_graph('powerlaw', 400, .) neighbours most of the graph), so their top two are both exactly 1.0.  Such a tie is decided by
torch.max's first-index rule, not by rounding, provided no entry of the row is near the bound before the clamp: a row whose two largest entries are
both exactly 1.0 passes iff every entry of its unclamped fp64 value is more than 1e-4 away from 1.0.  The branch case (cs_branch_autoscale) additionally requires, of the per-row fp64 ratio
orig_diff / sum |resid|: at least one row on the `inf` branch, at least one finite row above 1000, and NO finite row within 5 % of 1000 — so the
tests exclude no row: the margin is a property of the input.

cs_options.pt: args.lpStep / preStep / midStep as the reference's option pipeline leaves them (base_options.py:352-402).
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402
import cs_ref  # noqa: E402

ALPHA1, ALPHA2 = 0.9791632871592579, 0.7564990804200602
PAIRS = [('DA', 'AD'), ('DAD', 'DAD'), ('AD', 'DA')]
GAP = 1e-4


class Rejected(Exception):
    pass


def make_inputs(n, c, seed, pendant=0):
    """Power-law graph (make_golden.make_graph) of n nodes, optionally with an unlabelled path of `pendant` nodes hanging off node 0; labels, masks and
    class probabilities that follow the labels loosely."""
    ei, _ = mg.make_graph('powerlaw', n, seed)
    g = torch.Generator().manual_seed(7000 + seed)
    N = n + pendant
    if pendant:
        a = torch.cat([torch.tensor([0]), torch.arange(n, N - 1)])
        b = torch.arange(n, N)
        ei = torch.cat([ei, torch.stack([a, b]), torch.stack([b, a])], dim=1)
    y = torch.randint(0, c, (N,), generator=g)
    y[0] = c - 1                                            # labels.max() + 1 == c
    r = torch.rand(N, generator=g)
    train_mask, valid_mask = r < 0.4, (r >= 0.4) & (r < 0.55)
    train_mask[0] = True
    if pendant:
        train_mask[n:] = False
        valid_mask[n:] = False
    test_mask = ~(train_mask | valid_mask)
    logits = 1.5 * F.one_hot(y, c).float() * (torch.rand(N, 1, generator=g) < 0.7) + torch.randn(N, c, generator=g)
    return dict(edge_index=ei, y=y, train_mask=train_mask, valid_mask=valid_mask, test_mask=test_mask, model_out=torch.softmax(logits, 1))


def top2_gap(t):
    v = t.double().topk(2, dim=1)[0]
    return float((v[:, 0] - v[:, 1]).min())


def ref_adjs(oc, inp):
    Data = sys.modules['torch_geometric.data.data'].Data
    n = inp['y'].shape[0]
    data = Data(x=torch.zeros(n, 2), y=inp['y'].clone(), edge_index=inp['edge_index'].clone())
    adj, d_isqrt = oc.process_adj(data)
    return data, dict(zip(('DAD', 'DA', 'AD'), oc.gen_normalized_adjs(adj, d_isqrt))), d_isqrt


def accs(ns, inp, before, after):
    ev = ns.trainer.evaluate
    return torch.tensor([ev(before, inp['y'], inp['train_mask']), ev(before, inp['y'], inp['test_mask']),
                         ev(after, inp['y'], inp['train_mask']), ev(after, inp['y'], inp['test_mask'])], dtype=torch.float64)


def run_cs_case(ns, oc, name, fn, A1, A2, n, c, seed, pendant=0, branch=False, T=50, scale=1.0):
    inp = make_inputs(n, c, seed, pendant)
    data, adjs, d_isqrt = ref_adjs(oc, inp)
    split_idx = {k: torch.where(inp[k + '_mask'])[0] for k in ('train', 'valid', 'test')}
    kw = dict(train_only=True, display=False, device='cpu')
    if fn == 'only_outcome_correlation':
        res, result = oc.only_outcome_correlation(data, inp['model_out'].clone(), split_idx, adjs[A2], ALPHA2, T, ['train'], display=False, device='cpu')
    else:
        res, result = getattr(oc, fn)(data, inp['model_out'].clone(), split_idx, adjs[A1], ALPHA1, T, adjs[A2], ALPHA2, T, scale=scale, **kw)
    if top2_gap(inp['model_out']) < GAP:
        raise Rejected('top-two gap of the probabilities below 1e-4')
    g = dict(inp)
    g.update(name=name, kind='cs', fn=fn, A1=A1, A2=A2, alpha1=ALPHA1, alpha2=ALPHA2, num_propagations1=T, num_propagations2=T, scale=scale, seed=seed,
             label_idx=split_idx['train'], deg_inv_sqrt=d_isqrt, res_result=res, result=result, acc=accs(ns, inp, inp['model_out'], result))
    N = inp['y'].shape[0]
    ei_u = cs_ref.to_undirected(inp['edge_index'], N)
    assert torch.equal(ei_u, data.edge_index)
    res64, result64, parts = cs_ref.correct_and_smooth64(fn, ei_u, N, inp['y'], inp['model_out'], split_idx['train'], A1, ALPHA1, T, A2, ALPHA2, T,
                                                         scale=scale, want_parts=True)
    g['ref_err64'] = float(max((res.double() - res64).abs().max(), (result.double() - result64).abs().max()))
    v = result.double().topk(2, dim=1)[0]
    close = torch.where(v[:, 0] - v[:, 1] < GAP)[0]
    if len(close):
        saturated = bool(((v[close, 0] == 1.0) & (v[close, 1] == 1.0)).all())
        if not saturated or float((parts['pre_last'][close] - 1.0).abs().min()) <= GAP:
            raise Rejected('top-two gap of the result below 1e-4 in a row that is not safely saturated at the clamp bound')
    g['n_saturated_ties'] = int(len(close))
    if branch:
        ratio = parts['ratio'].reshape(-1)
        fin = ratio[torch.isfinite(ratio)]
        n_inf, n_big = int(ratio.isinf().sum()), int((fin > 1000).sum())
        closest = float(((fin - 1000).abs() / 1000).min())
        if not (n_inf >= 1 and n_big >= 1 and closest > 0.05):
            raise Rejected(f'branch case: {n_inf} inf rows, {n_big} rows above 1000, closest row {closest * 100:.1f} % from the threshold')
        g.update(n_inf=n_inf, n_big=n_big, closest_to_threshold=closest)
    return g


def run_general_case(ns, oc, name, A, alpha, T, alpha_term, clamp, n, c, seed):
    inp = make_inputs(n, c, seed)
    data, adjs, d_isqrt = ref_adjs(oc, inp)
    idx = torch.where(inp['train_mask'])[0]
    if alpha_term:
        y0 = oc.pre_outcome_correlation(labels=inp['y'], model_out=inp['model_out'].clone(), label_idx=idx)
    else:
        y0 = oc.pre_residual_correlation(labels=inp['y'].clone(), model_out=inp['model_out'].clone(), label_idx=idx)
    post = (lambda t: t) if clamp is None else (lambda t: torch.clamp(t, clamp[0], clamp[1]))
    result = oc.general_outcome_correlation(adjs[A], y0.clone(), alpha, T, post_step=post, alpha_term=alpha_term, device='cpu', display=False)
    g = dict(inp)
    g.update(name=name, kind='general', A=A, alpha=alpha, num_propagations=T, alpha_term=alpha_term, clamp=clamp, y0=y0, label_idx=idx, seed=seed,
             deg_inv_sqrt=d_isqrt, result=result)
    g['ref_err64'] = float((result.double() - cs_ref.case_outputs64(g)['result']).abs().max())
    return g


def options_fixture(ns):
    out = {}
    for key, argv in {'default': [], 'overrides': ['--LP__alpha=0.8', '--LP__num_propagations=20', '--LP__which_corr_and_DAD=DA']}.items():
        args = mg.ref_args(ns, 'Cora', argv)
        out[key] = dict(argv=argv, lp_has_prep=args.lp_has_prep, lpStep=dict(vars(args.lpStep)), preStep=dict(vars(args.preStep)),
                        midStep=dict(vars(args.midStep)))
    return out


def main():
    ns = ref_import.load_reference()
    torch.set_num_threads(1)
    with ref_import.in_scratch():
        from Label_propagation_model import outcome_correlation as oc
    jobs = []
    short = {'double_correlation_autoscale': 'autoscale', 'double_correlation_fixed': 'fixed', 'only_outcome_correlation': 'only'}
    for fn in cs_ref.FUNCTIONS:
        for A1, A2 in PAIRS:
            for c in (3, 7):
                name = f'cs_{short[fn]}_{A1}_{A2}_c{c}'
                jobs.append((name, lambda seed, fn=fn, A1=A1, A2=A2, c=c, name=name: run_cs_case(ns, oc, name, fn, A1, A2, 400, c, seed)))
    jobs.append(('cs_autoscale_DA_AD_c47', lambda seed: run_cs_case(ns, oc, 'cs_autoscale_DA_AD_c47', 'double_correlation_autoscale', 'DA', 'AD', 400, 47, seed)))
    jobs.append(('cs_branch_autoscale', lambda seed: run_cs_case(ns, oc, 'cs_branch_autoscale', 'double_correlation_autoscale', 'DA', 'AD', 300, 7, seed,
                                                                 pendant=70, branch=True)))
    jobs.append(('cs_general_noalpha_identity', lambda seed: run_general_case(ns, oc, 'cs_general_noalpha_identity', 'AD', 0.8, 50, False, None, 400, 7, seed)))
    jobs.append(('cs_general_clamp_1e-6', lambda seed: run_general_case(ns, oc, 'cs_general_clamp_1e-6', 'DAD', 0.9, 50, True, (1e-6, 1.0), 400, 7, seed)))
    for name, job in jobs:
        for seed in range(42, 90):
            try:
                g = job(seed)
            except Rejected as e:
                print(name, 'seed', seed, 'rejected:', e)
                continue
            path = os.path.join(HERE, name + '.pt')
            torch.save(g, path)
            print('wrote', name, 'seed', seed, os.path.getsize(path), 'bytes, ref_err64', g['ref_err64'],
                  'acc', g['acc'].tolist() if 'acc' in g else None, {k: g[k] for k in ('n_inf', 'n_big', 'closest_to_threshold') if k in g})
            break
        else:
            raise SystemExit(f'{name}: no seed passes the checks')
    torch.save(options_fixture(ns), os.path.join(HERE, 'cs_options.pt'))
    print('wrote cs_options')


if __name__ == '__main__':
    main()
