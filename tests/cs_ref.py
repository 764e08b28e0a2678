"""Plain fp64 restatement of the reference's Correct & Smooth (Label_propagation_model/outcome_correlation.py:39-55,95-213) — test code: torch on the
CPU, products with the adjacency as index_add over the undirected edge list.  tests/test_cs_host.py pins it to the fixtures the unmodified reference
wrote (tests/golden/cs_*.pt); the GPU tests measure the HIP path against it.  Inputs are taken as given (float32 values widened); every operation after
that is fp64, the degree normalisation included."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FORMS = ('DAD', 'DA', 'AD')
FUNCTIONS = ('double_correlation_autoscale', 'double_correlation_fixed', 'only_outcome_correlation')
TOL = dict(atol=1e-5, rtol=1e-5)


def cs_cases(prefix='cs_'):
    return sorted(f[:-3] for f in os.listdir(GOLDEN) if f.startswith(prefix) and f.endswith('.pt') and f != 'cs_options.pt')


def load_case(name):
    return torch.load(os.path.join(GOLDEN, name + '.pt'), weights_only=False)


def to_undirected(edge_index, n):
    key = torch.unique(torch.cat([edge_index[0] * n + edge_index[1], edge_index[1] * n + edge_index[0]]))
    return torch.stack([key // n, key % n])


def deg_inv_sqrt64(ei, n):
    deg = torch.bincount(ei[0], minlength=n).double()
    dis = deg.pow(-0.5)
    dis[dis == float('inf')] = 0
    return dis


def scales(dis, form):
    one = torch.ones_like(dis)
    return {'DAD': (dis, dis), 'DA': (dis * dis, one), 'AD': (one, dis * dis)}[form]


def adj_matmul(ei, n, dis, form, x):
    """(diag(R) A diag(S)) @ x for the undirected edge list ei ([2, E]: row, col)."""
    R, S = scales(dis, form)
    out = torch.zeros_like(x)
    out.index_add_(0, ei[0], (S[:, None] * x)[ei[1]])
    return R[:, None] * out


def propagate64(ei, n, dis, form, y, alpha, T, post=None, alpha_term=True, want_pre=False):
    """want_pre: also the last step's value BEFORE its post-step."""
    y = y.double()
    result = pre = y.clone()
    for _ in range(int(T)):
        result = pre = alpha * adj_matmul(ei, n, dis, form, result) + ((1 - alpha) * y if alpha_term else y)
        if post is not None:
            result = post(pre.clone())
    return (result, pre) if want_pre else result


def residual_init64(labels, model_out, idx):
    p = model_out.double()
    y = torch.zeros_like(p)
    y[idx] = torch.nn.functional.one_hot(labels[idx], p.shape[1]).double() - p[idx]
    return y


def snap64(labels, res, idx):
    y = res.clone()
    y[idx] = torch.nn.functional.one_hot(labels[idx], res.shape[1]).double()
    return y


def autoscale_ratio64(e0, resid, idx):
    """orig_diff / sum_j |resid[v, j]| per row, before the two replacements (inf where the row sum is 0, nan for 0 / 0)."""
    orig_diff = e0[idx].abs().sum() / idx.shape[0]
    return orig_diff / resid.abs().sum(dim=1, keepdim=True)


def correct_and_smooth64(fn, ei, n, labels, model_out, idx, A1, alpha1, T1, A2, alpha2, T2, scale=1.0, want_parts=False):
    """(res_result, result) of `fn` in fp64; ei: the undirected edge list; idx: the label rows (residual_idx == label_idx)."""
    dis = deg_inv_sqrt64(ei, n)
    p = model_out.double()
    e0 = resid = ratio = None
    if fn == 'only_outcome_correlation':
        res = p.clone()
    else:
        e0 = residual_init64(labels, model_out, idx)
        if fn == 'double_correlation_autoscale':
            resid = propagate64(ei, n, dis, A1, e0, alpha1, T1, post=lambda t: t.clamp(-1.0, 1.0))
            ratio = autoscale_ratio64(e0, resid, idx)
            s = ratio.clone()
            s[s.isinf()] = 1.0
            s[s > 1000] = 1.0
            res = p + s * resid
            res[res.isnan()] = p[res.isnan()]
        else:
            fix = e0[idx].clone()

            def fix_inputs(t):
                t[idx] = fix
                return t
            resid = propagate64(ei, n, dis, A1, e0, alpha1, T1, post=fix_inputs)
            res = p + scale * resid
    result, pre = propagate64(ei, n, dis, A2, snap64(labels, res, idx), alpha2, T2, post=lambda t: t.clamp(0, 1), want_pre=True)
    if want_parts:
        return res, result, dict(e0=e0, resid=resid, ratio=ratio, dis=dis, pre_last=pre)
    return res, result


def case_outputs64(g):
    """The fp64 restatement of whatever fixture g records -> dict of the tensors it stores."""
    n = int(g['y'].shape[0])
    ei = to_undirected(g['edge_index'], n)
    if g['kind'] == 'general':
        dis = deg_inv_sqrt64(ei, n)
        post = None if g['clamp'] is None else (lambda t: t.clamp(g['clamp'][0], g['clamp'][1]))
        return dict(result=propagate64(ei, n, dis, g['A'], g['y0'], g['alpha'], g['num_propagations'], post=post, alpha_term=g['alpha_term']))
    res, result = correct_and_smooth64(g['fn'], ei, n, g['y'], g['model_out'], g['label_idx'], g['A1'], g['alpha1'], g['num_propagations1'],
                                       g['A2'], g['alpha2'], g['num_propagations2'], scale=g['scale'])
    return dict(res_result=res, result=result)


def accuracy(out, labels, mask):
    """trainer_node_classification.evaluate (:672-681)."""
    idx = torch.max(out, dim=1)[1]
    return torch.sum(idx[mask] == labels[mask]).item() * 1.0 / mask.sum().item()


def powerlaw_graph(n, seed, exponent=0.9, edges_per_node=4):
    """Symmetric power-law graph with self-loops (the construction of tests/golden/make_golden.make_graph('powerlaw'))."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.arange(n, dtype=torch.float64) + 1.0) ** -exponent
    s = torch.multinomial(w, edges_per_node * n, replacement=True, generator=g)
    d = torch.multinomial(w, edges_per_node * n, replacement=True, generator=g)
    keep = s != d
    perm = torch.randperm(n, generator=g)
    s, d = perm[s[keep]], perm[d[keep]]
    key = torch.unique(torch.cat([s * n + d, d * n + s]))
    loops = torch.arange(n)
    return torch.cat([torch.stack([key // n, key % n]), torch.stack([loops, loops])], dim=1)
