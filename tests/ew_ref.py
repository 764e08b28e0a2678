"""float64 restatement of the edge-weighted encoder layers (GraphConv / GCNConv(normalize=False) on an adj_t with values) and of the reference's two
adjacency normalisations (Link_prediction_model/utils.py:93-106), from the EDGE LIST: index_add_ of w[:, None] * x[src] — no CSR walk, so it shares no
algorithm with the kernels.  An adjacency with values has one value w_e per stored edge e = (u -> v); repeated edges stay separate entries.

    agg[v] = sum over the in-edges e of v of w_e * x[u_e]
    WSAGE:  Y = act(agg lin_rel^T + lin_rel.bias + X lin_root^T)          GCN:  Y = act(agg lin^T + bias)
    adj_normalization:  deg[v] = sum of row v's values, f = 1 / deg (inf -> 0), w'_e = f[v_e] * w_e
    gcn_normalization:  set_diag (every stored (v, v) dropped, one (v, v) of value 1 per node), deg = row sums, dis = deg^-1/2 (inf -> 0),
                        w'_e = (dis[v_e] * w_e) * dis[u_e]
Arithmetic of the normalisations in fp32 (`normalize`): deg is a float64 sum rounded once to fp32; f / dis are computed in float64 from that fp32 value
(1.0 / d, 1.0 / sqrt(d)) and rounded once; the products round in the order written.

Bound of a compared contraction (sage_ref's, with the reduced row counted twice: each edge adds one rounding for the product and one for the sum):
    (K + 2 * longest + 8) * 2^-24 * (the same contraction on absolute values, |w| included, in float64)"""
import torch

import sage_ref as sr

EPS = sr.EPS


def agg(ei, n, w, x):
    """A_w x in the dtype of x: out[dst] += w * x[src] over the edge list."""
    return torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add(0, ei[1], w.to(x.dtype)[:, None] * x[ei[0]])


def agg_t(ei, n, w, g):
    """A_w^T g: out[src] += w * g[dst]."""
    return torch.zeros((n, g.shape[1]), dtype=g.dtype).index_add(0, ei[0], w.to(g.dtype)[:, None] * g[ei[1]])


def layer(ei, n, w, x, W_n, W_s, b, relu=False, mask=None):
    """float64 (Y, agg); autograd flows to x, W_n, W_s, b (not to w: the values are data).  W_s None: GCN."""
    a = agg(ei, n, w.detach(), x)
    y = a @ W_n.t()
    if W_s is not None:
        y = y + x @ W_s.t()
    if b is not None:
        y = y + b
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = y * mask
    return y, a


def _bound(length, longest, absval):
    return (length + 2 * longest + 8) * EPS * absval


def longest_rows(ei, n):
    indeg, outdeg = sr.degrees(ei, n)
    return int(indeg.max()), int(outdeg.max())


def bound_agg(ei, n, w, x, transpose=False):
    """Bound of A_w x (or A_w^T x) alone: a contraction of length 0 over the reduced row."""
    f = agg_t if transpose else agg
    return _bound(0, longest_rows(ei, n)[1 if transpose else 0], f(ei, n, w.abs(), x.abs()))


def bound_forward(ei, n, w, x, W_n, W_s, b, factor=1.0):
    a = agg(ei, n, w.abs(), x.abs()) @ W_n.abs().t()
    k = x.shape[1]
    if W_s is not None:
        a = a + x.abs() @ W_s.abs().t()
        k *= 2
    if b is not None:
        a = a + b.abs()
    return _bound(k, longest_rows(ei, n)[0], a * factor)


def bound_dx(ei, n, w, G, W_n, W_s):
    a = agg_t(ei, n, w.abs(), G.abs()) @ W_n.abs()
    k = G.shape[1]
    if W_s is not None:
        a = a + G.abs() @ W_s.abs()
        k *= 2
    return _bound(k, longest_rows(ei, n)[1], a)


def bound_dw(ei, n, w, G, x):
    longest = longest_rows(ei, n)[1]
    return _bound(n, longest, agg_t(ei, n, w.abs(), G.abs()).t() @ x.abs()), _bound(n, longest, G.abs().t() @ x.abs())


def bound_db(n, G):
    return _bound(n, 0, G.abs().sum(0))


# ---- the normalisations ----------------------------------------------------------------------------------------------------------------
def set_diag(ei, n, w):
    """torch_sparse set_diag on the edge list: (edge_index, values) without any stored (v, v), followed by one (v, v) of value 1 per node."""
    keep = ei[0] != ei[1]
    d = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[:, keep], torch.stack([d, d])], 1), torch.cat([w[keep], torch.ones(n, dtype=w.dtype)])


def row_sums(ei, n, w):
    """fp32 [n]: the float64 sum of each destination row's values, rounded once."""
    return torch.zeros(n, dtype=torch.float64).index_add(0, ei[1], w.double()).float()


def inv_factor(deg, kind):
    """fp32 [n] from the fp32 row sums: 1 / deg ('adj') or deg^-1/2 ('gcn') in float64, rounded once, inf -> 0."""
    d = deg.double()
    f = (1.0 / d if kind == 'adj' else 1.0 / torch.sqrt(d)).float()
    return torch.where(torch.isinf(f), torch.zeros_like(f), f)


def normalize(ei, n, w, kind):
    """(edge_index', w' fp32, deg fp32, factor fp32) of the stated arithmetic; w fp32 [E].  'gcn' changes the structure (set_diag)."""
    w = w.float()
    if kind == 'gcn':
        ei, w = set_diag(ei, n, w)
    deg = row_sums(ei, n, w)
    f = inv_factor(deg, kind)
    out = f[ei[1]] * w
    if kind == 'gcn':
        out = out * f[ei[0]]
    return ei, out, deg, f


def by_edge_key(ei, n, w):
    """The values sorted by (dst, src, value): an order in which two statements of the same multiset of entries can be compared."""
    key = (ei[1] * n + ei[0]).double()
    order = torch.argsort(w.double(), stable=True)
    order = order[torch.argsort(key[order], stable=True)]
    return (ei[1] * n + ei[0])[order], w[order]


def ulp_distance(a, b):
    """int64: how many fp32 values lie between a and b (0: the same bits, up to the sign of zero)."""
    def ordered(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (ordered(a.float()) - ordered(b.float())).abs()
