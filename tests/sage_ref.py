"""float64 restatement of the three encoder layers (Link_prediction_model/layer.py:8-35: PyG SAGEConv with mean aggregation and a root weight, GraphConv
with add, GCNConv(normalize=False)) from the EDGE LIST — index_add_ over edge_index, no CSR walk, so it shares no algorithm with the kernels — and the
error bounds the GPU tests hold the device results to.  Gradients come from torch autograd on this restatement.

    Y = act((s * (A X)) W_n^T + X W_s^T + b)      SAGE: s = 1 / indeg (0 where indeg = 0);  WSAGE: s = 1;  GCN: s = 1, no W_s
A X = the sum over the in-neighbours (edge_index[0] = source, edge_index[1] = destination), multiplicity and self loops as given.

Bound of a compared quantity (one contraction), elementwise:
    (length of the contraction + longest reduced row + 8) * 2^-24 * (the same contraction on absolute values, in float64)
fp32 products and sums each round by at most 2^-24 relative (the three-limb GEMM is exact to fp32 products, fp32 accumulation); a result of n such
operations is within n * 2^-24 of the sum of absolute values to first order; + 8 covers the epilogue's few operations (scale, bias, dropout factor)."""
import torch

EPS = 2.0 ** -24
MODES = ('SAGE', 'WSAGE', 'GCN')


def make_graph(n, n_edges, seed, no_in=(), hub_in=None, hub_out=None, n_self=12, n_dup=40):
    """int64 edge_index [2, E] of a directed, non-symmetric multigraph on n nodes: n_edges random edges, n_self self loops, n_dup repeated edges; the nodes
    `no_in` have no in-edge; hub_in = (node, degree) / hub_out = (node, degree) add a row of that in- / out-degree."""
    g = torch.Generator().manual_seed(seed)
    allowed = torch.tensor([v for v in range(n) if v not in set(no_in)])
    src = torch.randint(0, n, (n_edges,), generator=g)
    dst = allowed[torch.randint(0, len(allowed), (n_edges,), generator=g)]
    loops = allowed[torch.randperm(len(allowed), generator=g)[:n_self]]
    parts = [torch.stack([src, dst]), torch.stack([loops, loops]), torch.stack([src[:n_dup], dst[:n_dup]])]
    if hub_in is not None:
        v, k = hub_in
        parts.append(torch.stack([torch.randperm(n, generator=g)[:k], torch.full((k,), v)]))
    if hub_out is not None:
        v, k = hub_out
        parts.append(torch.stack([torch.full((k,), v), allowed[torch.randperm(len(allowed), generator=g)[:k]]]))
    ei = torch.cat(parts, 1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()


def degrees(ei, n):
    return torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)


def row_factor(ei, n, mode):
    """float64 [n]: s of the mode."""
    indeg = degrees(ei, n)[0].double()
    if mode == 'SAGE':
        return torch.where(indeg > 0, 1.0 / indeg.clamp(min=1.0), torch.zeros_like(indeg))
    return torch.ones(n, dtype=torch.float64)


def agg_sum(ei, n, x):
    """A x in the dtype of x: out[dst] += x[src] over the edge list."""
    return torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add(0, ei[1], x[ei[0]])


def agg_sum_t(ei, n, g):
    """A^T g: out[src] += g[dst]."""
    return torch.zeros((n, g.shape[1]), dtype=g.dtype).index_add(0, ei[0], g[ei[1]])


def layer(ei, n, x, W_n, W_s, b, mode, relu=False, mask=None):
    """float64 Y (autograd flows to x, W_n, W_s, b).  mask (float64 [n, out] or None) multiplies after the ReLU: the keep-mask over (1 - p)."""
    s = row_factor(ei, n, mode)
    agg = agg_sum(ei, n, x) * s[:, None]
    y = agg @ W_n.t()
    if W_s is not None:
        y = y + x @ W_s.t()
    if b is not None:
        y = y + b
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = y * mask
    return y, agg


def _bound(length, longest, absval):
    return (length + longest + 8) * EPS * absval


def bound_forward(ei, n, x, W_n, W_s, b, mode, factor=1.0):
    """Bound of Y: length 512 (256 without W_s) over [s * A|X|, |X|] and [|W_n| ; |W_s|], plus |b|; times the dropout factor 1 / (1 - p)."""
    s = row_factor(ei, n, mode)
    a = (agg_sum(ei, n, x.abs()) * s[:, None]) @ W_n.abs().t()
    k = x.shape[1]
    if W_s is not None:
        a = a + x.abs() @ W_s.abs().t()
        k *= 2
    if b is not None:
        a = a + b.abs()
    return _bound(k, int(degrees(ei, n)[0].max()), a * factor)


def bound_dx(ei, n, G, W_n, W_s, mode):
    """Bound of dX = (A^T (s * G)) W_n + G W_s."""
    s = row_factor(ei, n, mode)
    a = agg_sum_t(ei, n, G.abs() * s[:, None]) @ W_n.abs()
    k = G.shape[1]
    if W_s is not None:
        a = a + G.abs() @ W_s.abs()
        k *= 2
    return _bound(k, int(degrees(ei, n)[1].max()), a)


def bound_dw(ei, n, G, x, mode):
    """Bounds of dW_n = R^T X (R = A^T (s * G)) and dW_s = G^T X: contractions of length n."""
    s = row_factor(ei, n, mode)
    longest = int(degrees(ei, n)[1].max())
    return _bound(n, longest, agg_sum_t(ei, n, G.abs() * s[:, None]).t() @ x.abs()), _bound(n, longest, G.abs().t() @ x.abs())


def bound_db(n, G):
    return _bound(n, 0, G.abs().sum(0))


def within(got, ref, bound):
    """(ok, worst ratio |got - ref| / bound) with got fp32 from the device, ref / bound float64.  A zero bound asks for exact equality."""
    err = (got.double().cpu() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return worst <= 1.0, worst
