"""Float64 restatements of the BIL / MLPDOT / MLPBIL / MLPCAT predictors (Link_prediction_model/layer.py:108-180, 193-203) in eval mode, their
gradients, the magnitude sums the GPU tests' error bounds are formed from, and the row scatter.  tests/test_pairpred_host.py pins the outputs to
the recordings of the unmodified reference (tests/golden/pairpred_predictors.pt, tools/gen_pairpred_golden.py).  torch only, CPU."""
import torch

KINDS = ('bil', 'mlpdot', 'mlpbil', 'mlpcat')
U = 2.0 ** -24


def n_lins(sd):
    return len([k for k in sd if k.startswith('lins.') and k.endswith('.weight')])


def stack64(sd, x, last_relu=True, keep=None):
    """lins.* on x in float64, ReLU after every layer (the last one only with last_relu); keep: optional list of boolean keep-masks, one per layer
    that is followed by dropout, applied as x * keep / (1 - p) with keep = (mask, p)."""
    n = n_lins(sd)
    for i in range(n):
        x = x @ sd[f'lins.{i}.weight'].double().t() + sd[f'lins.{i}.bias'].double()
        if i < n - 1 or last_relu:
            x = torch.relu(x)
            if keep is not None:
                mask, p = keep[i]
                x = torch.where(mask, x / (1.0 - p), torch.zeros_like(x))
    return x


def predictor64(kind, sd, x_i, x_j, keep=None):
    """forward(x_i, x_j) of the reference module `kind` from a state_dict, in float64.  keep: per-layer (mask [2 S, width], p) over the matrix whose
    rows e < S are the x_i side (x1) and rows S + e the x_j side (x2)."""
    x_i, x_j = x_i.double(), x_j.double()
    S = x_i.shape[0]
    if kind == 'bil':
        return ((x_i @ sd['bilin.weight'].double().t()) * x_j).sum(-1)
    if kind == 'mlpcat':
        x = stack64(sd, torch.cat([torch.cat([x_i, x_j], -1), torch.cat([x_j, x_i], -1)], 0), last_relu=False, keep=keep)
        return (x[:S] + x[S:]) / 2
    x = stack64(sd, torch.cat([x_i, x_j], 0), keep=keep)
    if kind == 'mlpdot':
        return (x[:S] * x[S:]).sum(-1)
    if kind == 'mlpbil':
        return ((x[:S] @ sd['bilin.weight'].double().t()) * x[S:]).sum(-1)
    raise ValueError(kind)


def predictor_grads64(kind, sd, h, pairs, gout, keep=None):
    """(out, dh, {name: grad}) in float64 through autograd of the restatement; the scalar is sum(out.reshape(S, -1) * gout)."""
    sd64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    h64 = h.detach().double().clone().requires_grad_(True)
    out = predictor64(kind, sd64, h64[pairs[0].long()], h64[pairs[1].long()], keep=keep)
    (out.reshape(pairs.shape[1], -1) * gout.double()).sum().backward()
    return out.detach(), h64.grad, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd64.items()}


def predictor_abs64(kind, sd, h, pairs, gout):
    """The same network on absolute values — |h|, |W|, |b|, |gout| — through the same autograd: every entry of (out, dh, grads) is then the sum of the
    absolute values of the terms whose signed sum the real network's entry is (ReLU lets everything through: an upper bound of the masked sum)."""
    return predictor_grads64(kind, {k: v.detach().abs() for k, v in sd.items()}, h.abs(), pairs, gout.abs())


def usable(pairs, n_nodes):
    return ((pairs >= 0) & (pairs < n_nodes)).all(0)


def bilinear64(h, pairs, W):
    """(s [S], scale [S]) in float64: s_e = sum_j (W h[u_e])_j h[v_e, j], NaN for an unusable pair; scale_e = sum_jk |W_jk h[u_e, k] h[v_e, j]|."""
    N = h.shape[0]
    ok = usable(pairs, N)
    u, v = pairs[0].long().clamp(0, N - 1), pairs[1].long().clamp(0, N - 1)
    h64, W64 = h.double(), W.double()
    s = ((h64[u] @ W64.t()) * h64[v]).sum(-1)
    scale = ((h64[u].abs() @ W64.abs().t()) * h64[v].abs()).sum(-1)
    s[~ok] = float('nan')
    return s, scale


def scatter_rows64(pairs, g0, g1, n_rows):
    """(dH [n_rows, D], sum of |terms|) in float64: g0[e] into row u_e, g1[e] into row v_e; unusable pairs contribute nothing."""
    ok = usable(pairs, n_rows)
    u, v = pairs[0].long()[ok], pairs[1].long()[ok]
    a, b = g0.double()[ok], g1.double()[ok]
    dh = torch.zeros((n_rows, g0.shape[1]), dtype=torch.float64)
    sa = torch.zeros_like(dh)
    dh.index_add_(0, u, a)
    dh.index_add_(0, v, b)
    sa.index_add_(0, u, a.abs())
    sa.index_add_(0, v, b.abs())
    return dh, sa
