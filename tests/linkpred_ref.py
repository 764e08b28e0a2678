"""Float64 restatements of the link predictors and ranking losses (Link_prediction_model/layer.py:85-106, 182-191; loss.py:4-30) for shapes without a
recorded fixture.  tests/test_linkpred_host.py pins every function here to the recordings of the unmodified reference (tests/golden/linkpred_*.pt,
tools/gen_linkpred_golden.py).  torch only, CPU."""
import torch

KINDS = ('auc_loss', 'adaptive_auc_loss', 'log_rank_loss', 'ce_loss', 'info_nce_loss')
EPS23 = 2.0 ** -23


def rank_loss64(kind, pos, neg, num_neg, weight=None):
    """The loss in float64 by the reference's formula as written, from scores of any float dtype."""
    p = pos.detach().double().reshape(-1, 1)
    n = neg.detach().double().reshape(-1, num_neg)
    if kind == 'auc_loss':
        return torch.square(1 - (p - n)).sum()
    if kind == 'adaptive_auc_loss':
        return (weight.detach().double().reshape(-1, 1) * torch.square(1 - (p - n))).sum()
    if kind == 'log_rank_loss':
        return -torch.log(torch.sigmoid(p - n) + 1e-15).mean()
    if kind == 'ce_loss':
        return -torch.log(torch.sigmoid(p) + 1e-15).mean() + -torch.log(1 - torch.sigmoid(n) + 1e-15).mean()
    if kind == 'info_nce_loss':
        pe = torch.exp(p)
        return -torch.log(pe / (pe + torch.sum(torch.exp(n), 1, keepdim=True)) + 1e-15).mean()
    raise ValueError(kind)


def rank_loss_grads64(kind, pos, neg, num_neg, weight=None, g=1.0):
    """(loss, dpos [P], dneg [P * k]) in float64 through autograd of the restatement, upstream gradient g."""
    p = pos.detach().double().clone().requires_grad_(True)
    n = neg.detach().double().clone().requires_grad_(True)
    pp, nn = p.reshape(-1, 1), n.reshape(-1, num_neg)
    w = weight.detach().double().reshape(-1, 1) if weight is not None else None
    if kind == 'auc_loss':
        loss = torch.square(1 - (pp - nn)).sum()
    elif kind == 'adaptive_auc_loss':
        loss = (w * torch.square(1 - (pp - nn))).sum()
    elif kind == 'log_rank_loss':
        loss = -torch.log(torch.sigmoid(pp - nn) + 1e-15).mean()
    elif kind == 'ce_loss':
        loss = -torch.log(torch.sigmoid(pp) + 1e-15).mean() + -torch.log(1 - torch.sigmoid(nn) + 1e-15).mean()
    elif kind == 'info_nce_loss':
        pe = torch.exp(pp)
        loss = -torch.log(pe / (pe + torch.sum(torch.exp(nn), 1, keepdim=True)) + 1e-15).mean()
    else:
        raise ValueError(kind)
    (loss * g).backward()
    return loss.detach(), p.grad, n.grad


def usable(pairs, n_nodes):
    return ((pairs >= 0) & (pairs < n_nodes)).all(0)


def pair_product64(h, pairs):
    """h[u] * h[v] with each product rounded to fp32 first (what the device stages), as float64; rows of unusable pairs are zero."""
    ok = usable(pairs, h.shape[0])
    u, v = pairs[0].long().clamp(0, h.shape[0] - 1), pairs[1].long().clamp(0, h.shape[0] - 1)
    x = (h[u] * h[v]).double()
    x[~ok] = 0
    return x


def pair_dot64(h, pairs):
    ok = usable(pairs, h.shape[0])
    u, v = pairs[0].long().clamp(0, h.shape[0] - 1), pairs[1].long().clamp(0, h.shape[0] - 1)
    s = (h[u].double() * h[v].double()).sum(-1)
    s[~ok] = float('nan')
    return s


def pair_scatter64(h, pairs, coef):
    """(dH [N, D], sum of |terms| [N, D]) in float64: edge e contributes coef_e * h[v_e] into row u_e and coef_e * h[u_e] into row v_e; coef [S]
    or [S, D]; unusable pairs contribute nothing."""
    N, D = h.shape
    ok = usable(pairs, N)
    u, v = pairs[0].long()[ok], pairs[1].long()[ok]
    c = coef.double()[ok]
    if c.dim() == 1:
        c = c[:, None]
    h64 = h.double()
    tu, tv = c * h64[v], c * h64[u]
    dh = torch.zeros((N, D), dtype=torch.float64)
    sa = torch.zeros((N, D), dtype=torch.float64)
    dh.index_add_(0, u, tu)
    dh.index_add_(0, v, tv)
    sa.index_add_(0, u, tu.abs())
    sa.index_add_(0, v, tv.abs())
    return dh, sa


def mlp_predictor64(sd, x_i, x_j):
    """MLPPredictor.forward in eval mode (or dropout 0) from a state_dict, in float64."""
    n = len([k for k in sd if k.endswith('.weight')])
    x = x_i.double() * x_j.double()
    for i in range(n):
        x = x @ sd[f'lins.{i}.weight'].double().t() + sd[f'lins.{i}.bias'].double()
        if i < n - 1:
            x = torch.relu(x)
    return x
