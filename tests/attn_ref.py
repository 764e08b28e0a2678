"""Restatement of one PyG TransformerConv(in, out) layer with every default (heads = 1, concat, no beta, no edge features, no dropout, bias, root weight)
from the EDGE LIST — index_add / scatter_reduce over edge_index, no CSR walk, so it shares no algorithm with the kernels of csrc/cb_attn.hip.  Every
function computes in the dtype of its inputs: float64 is the reference, the same code in float32 on the CPU is the yardstick of the GPU tests.

    Q, K, V, S = x W^T + b of lin_query, lin_key, lin_value, lin_skip                  D = out_channels
    s_j    = <Q[v], K[u_j]> / sqrt(D)                over the in-edges j = (u_j -> v): edge_index[0] = source, edge_index[1] = destination;
                                                     multiplicity and self loops as given, each copy of a duplicate edge its own softmax term
    a_j    = exp(s_j - max_j s) / sum_j exp(s_j - max_j s)            (PyG's + 1e-16 in the denominator is not reproduced: the denominator is >= 1)
    out[v] = act(sum_j a_j V[u_j] + S[v]),    lse[v] = max_j s + log sum_j exp(s_j - max_j s);     a row without in-edges: act(S[v]), lse = -inf
Closed-form gradients for dO = dY * 1[out > 0] (dY without the ReLU), a_j = exp(s_j - lse[v]):
    delta[v] = sum_j a_j <dO[v], V[u_j]>
    dQ[v] = 1/sqrt(D) sum_j a_j (<dO[v], V[u_j]> - delta[v]) K[u_j]
    dK[u] = 1/sqrt(D) sum_{j: u -> v} a_j (<dO[v], V[u]> - delta[v]) Q[v],     dV[u] = sum_{j: u -> v} a_j dO[v],     dS = dO
    dX = sum_i dP_i W_i,  dW_i = dP_i^T X,  db_i = colsum(dP_i)                 over the four projections i
params: a dict {'lin_key.weight', 'lin_key.bias', 'lin_query.weight', ...} of [out, in] weights and [out] biases (NAMES, PyG's order)."""
import math

import torch

from sage_ref import make_graph  # noqa: F401  (the graphs of the tests)

LINS = ('lin_key', 'lin_query', 'lin_value', 'lin_skip')
NAMES = tuple(f'{lin}.{w}' for lin in LINS for w in ('weight', 'bias'))


def make_params(in_ch, out_ch, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for lin in LINS:
        p[f'{lin}.weight'] = (torch.randn(out_ch, in_ch, generator=g) / math.sqrt(in_ch)).to(dtype)
        p[f'{lin}.bias'] = (torch.randn(out_ch, generator=g) / 4).to(dtype)
    return p


def cast(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


def project(x, params):
    """(Q, K, V, S)"""
    return tuple(x @ params[f'{lin}.weight'].t() + params[f'{lin}.bias'] for lin in ('lin_query', 'lin_key', 'lin_value', 'lin_skip'))


def attention(ei, n, Q, K, V):
    """(sum_j a_j V[u_j] [n, D], lse [n], a [E], s [E]); autograd flows through everything but the subtracted maximum (whose derivative is zero)."""
    src, dst = ei[0], ei[1]
    s = (Q[dst] * K[src]).sum(-1) / math.sqrt(Q.shape[1])
    m = torch.full((n,), float('-inf'), dtype=s.dtype).scatter_reduce(0, dst, s.detach(), 'amax', include_self=True)
    p = torch.exp(s - m[dst])
    l = torch.zeros(n, dtype=s.dtype).index_add(0, dst, p)
    a = p / l[dst]
    agg = torch.zeros((n, V.shape[1]), dtype=s.dtype).index_add(0, dst, a[:, None] * V[src])
    return agg, m + torch.log(l.detach()), a, s


def layer(ei, n, x, params, relu=False):
    """(out, lse) in the dtype of x."""
    Q, K, V, S = project(x, params)
    agg, lse, _, _ = attention(ei, n, Q, K, V)
    out = agg + S
    return (torch.relu(out) if relu else out), lse


def grads(ei, n, x, params, dY, relu=False):
    """The closed form: {'x': dX, 'lin_key.weight': ..., ...} for the loss sum(out * dY), plus 'out', 'lse', 'delta'.  No autograd."""
    src, dst = ei[0], ei[1]
    x = x.detach()
    params = {k: v.detach() for k, v in params.items()}
    Q, K, V, S = project(x, params)
    agg, lse, _, s = attention(ei, n, Q, K, V)
    out = agg + S
    dO = dY
    if relu:
        dO = dY * (out > 0).to(dY.dtype)
        out = torch.relu(out)
    scale = 1.0 / math.sqrt(Q.shape[1])
    a = torch.exp(s - lse[dst])
    t = (dO[dst] * V[src]).sum(-1)
    delta = torch.zeros(n, dtype=x.dtype).index_add(0, dst, a * t)
    c = a * (t - delta[dst])
    dQ = scale * torch.zeros_like(Q).index_add(0, dst, c[:, None] * K[src])
    dK = scale * torch.zeros_like(K).index_add(0, src, c[:, None] * Q[dst])
    dV = torch.zeros_like(V).index_add(0, src, a[:, None] * dO[dst])
    res = {'out': out, 'lse': lse, 'delta': delta, 'x': torch.zeros_like(x)}
    for lin, dP in (('lin_query', dQ), ('lin_key', dK), ('lin_value', dV), ('lin_skip', dO)):
        res['x'] = res['x'] + dP @ params[f'{lin}.weight']
        res[f'{lin}.weight'] = dP.t() @ x
        res[f'{lin}.bias'] = dP.sum(0)
    return res


def max_err(got, ref):
    """max |got - ref| in float64 where equal infinities (lse of a row without in-edges) count as zero and any other non-finite difference as inf."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    same_inf = torch.isinf(ref) & (got == ref)
    diff = torch.where(same_inf, torch.zeros_like(ref), (got - ref).abs())
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float('inf')), diff)
    return float(diff.max()) if diff.numel() else 0.0


def bound(ref64, cpu32):
    """4 * e32(T) + 2^-22 * max |T_64|: four times the error of the same formulas in float32 on the CPU (both are fp32 evaluations that differ in the
    order of the sums and in exp), plus one rounding of the result itself."""
    finite = ref64[torch.isfinite(ref64)]
    top = float(finite.abs().max()) if finite.numel() else 0.0
    return 4.0 * max_err(cpu32, ref64) + 2.0 ** -22 * top
