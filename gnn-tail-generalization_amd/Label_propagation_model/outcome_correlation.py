"""The reference's Label_propagation_model/outcome_correlation.py (:39-55,83-213) on the device: same function names and signatures, every product
with a normalised adjacency is the aggregation kernel with the step's elementwise work in its store (ops.propagate, cb_spmm_csr_prop_f32), the
passes between the two propagations of Correct & Smooth are two row kernels (csrc/cb_cs.hip).

Documented deviations:
  * everything stays on the device the inputs live on: `device=` / `lp_force_on_cpu` are accepted and ignored (the reference pins C&S to the CPU);
  * `gen_normalized_adjs` returns three light handles (NormalizedAdj) over ONE CSRGraph in place of three torch_sparse matrices;
  * `post_step` takes the descriptors Clamp(lo, hi), Identity() and FixRows(idx), which run inside the aggregation's store; any other callable
    is applied to the matrix after an unclamped step (one launch + the callable per step: slower, same result);
  * `double_correlation_fixed` does not require `split_idx` to hold exactly three keys (the reference unpacks it into three names it never uses);
  * label rows given by index are taken as distinct.
"""
import torch
import torch.nn.functional as F

from .. import ops
from ..graph import CSRGraph
from ..utils import to_undirected

ADJ_FORMS = ops.ADJ_FORMS


class Clamp:
    """post_step = lambda x: torch.clamp(x, lo, hi), run in the store of the propagation step."""

    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def __call__(self, x):
        return torch.clamp(x, self.lo, self.hi)


class Identity:
    """post_step = lambda x: x."""

    def __call__(self, x):
        return x


class FixRows:
    """post_step = fix_inputs (:194-199): after every step the rows `idx` are reset to their rows of y (index tensor or mask)."""

    def __init__(self, idx):
        self.idx = idx

    def __call__(self, x):
        raise TypeError('FixRows is resolved inside general_outcome_correlation (it needs y)')


class NormalizedAdj:
    """One of DAD / DA / AD (:51-55) over a shared CSRGraph: the normalisation is applied through the operands of the propagation step."""

    def __init__(self, graph, deg_inv_sqrt, form):
        if form not in ADJ_FORMS:
            raise ValueError(f"normalised adjacency '{form}': one of {ADJ_FORMS}")
        self.graph, self.deg_inv_sqrt, self.form = graph, deg_inv_sqrt, form

    def to(self, device):
        return self

    def __matmul__(self, x):
        """A_norm @ x (one unclamped step with alpha = 1 and no mix term)."""
        R, S = ops.adj_scales(self.deg_inv_sqrt, self.form)
        h = x.float().contiguous() if S is None else ops._scaled_rows(x.float().contiguous(), S)
        return self.graph.spmm(h, row_scale=R)

    def __repr__(self):
        return f'NormalizedAdj({self.form}, N={self.graph.N}, E={self.graph.E})'


class _Adj:
    """What process_adj returns for the adjacency: the device graph of the undirected edge list."""

    def __init__(self, graph):
        self.graph = graph


def process_adj(data):
    N = data.num_nodes if getattr(data, 'num_nodes', None) is not None else int(data.x.shape[0])
    data.edge_index = to_undirected(data.edge_index, N)
    graph = CSRGraph(data.edge_index, N)
    deg_inv_sqrt = graph.in_degrees().to(torch.float).pow(-0.5)
    deg_inv_sqrt[deg_inv_sqrt == float('inf')] = 0
    return _Adj(graph), deg_inv_sqrt


def gen_normalized_adjs(adj, D_isqrt):
    graph = adj.graph if isinstance(adj, _Adj) else adj
    return tuple(NormalizedAdj(graph, D_isqrt, form) for form in ('DAD', 'DA', 'AD'))


def get_labels_from_name(labels, split_idx, **trash):
    if isinstance(labels, list):
        labels = list(labels)
        if len(labels) == 0:
            return torch.tensor([])
        for idx, i in enumerate(list(labels)):
            labels[idx] = split_idx[i]
        residual_idx = torch.cat(labels)
    else:
        residual_idx = split_idx[labels]
    return residual_idx


def _labels(labels):
    labels = labels.reshape(-1)
    if labels.dtype.is_floating_point:
        labels = torch.where(labels.isnan(), torch.zeros_like(labels), labels)
    return labels.long()


def pre_residual_correlation(labels, model_out, label_idx, **trash):
    """Generates the initial labels used for residual correlation: onehot(labels) - model_out on label_idx, 0 elsewhere."""
    rows = ops.rows_mask(label_idx, model_out.shape[0], model_out.device)
    e0, _, _ = ops.cs_residual_init(model_out, _labels(labels), rows)
    c = model_out.shape[1]
    return e0[:, :c].contiguous() if e0.shape[1] != c else e0


def pre_outcome_correlation(labels, model_out, label_idx, **trash):
    """Generates the initial labels used for outcome correlation: model_out with the rows label_idx snapped to one-hot."""
    rows = ops.rows_mask(label_idx, model_out.shape[0], model_out.device)
    _, y2, _ = ops.cs_correct_snap('only_outcome_correlation', model_out, None, _labels(labels), rows)
    c = model_out.shape[1]
    return y2[:, :c].contiguous() if y2.shape[1] != c else y2


def general_outcome_correlation(adj, y, alpha, num_propagations, post_step, alpha_term, device='cuda', display=True, **trash):
    """general outcome correlation. alpha_term = True for outcome correlation, alpha_term = False for residual correlation"""
    if not isinstance(adj, NormalizedAdj):
        raise TypeError('general_outcome_correlation: adj is one of the handles of gen_normalized_adjs')
    kw = dict(adj=adj.form, alpha_term=bool(alpha_term))
    if isinstance(post_step, Clamp):
        return ops.propagate(adj.graph, y, adj.deg_inv_sqrt, alpha, num_propagations, clamp=(post_step.lo, post_step.hi), **kw)
    if isinstance(post_step, Identity):
        return ops.propagate(adj.graph, y, adj.deg_inv_sqrt, alpha, num_propagations, clamp=None, **kw)
    if isinstance(post_step, FixRows):
        return ops.propagate(adj.graph, y, adj.deg_inv_sqrt, alpha, num_propagations, clamp=None, fixed_rows=post_step.idx, **kw)
    result = y.float().clone()
    for _ in range(int(num_propagations)):
        result = post_step(_one_step(adj, result, y, alpha, kw))
    return result


def _one_step(adj, result, y, alpha, kw):
    """alpha * A_norm result + (1 - alpha | 1) * y, unclamped: the step an arbitrary post_step callable is applied to."""
    R, S = ops.adj_scales(adj.deg_inv_sqrt, adj.form)
    y = y.float().contiguous()
    h = ops._scaled_rows(result.contiguous(), S)
    a_r = R * float(alpha) if R is not None else torch.full((y.shape[0],), float(alpha), dtype=torch.float32, device=y.device)
    return adj.graph.spmm_prop(h, a_r.contiguous(), y, 1.0 - float(alpha) if kw['alpha_term'] else 1.0)


def label_propagation(data, split_idx, A, alpha, num_propagations, idxs, **trash):
    labels = data.y.data.reshape(-1)
    c = int(labels.max()) + 1
    n = labels.shape[0]
    y = torch.zeros((n, c), device=data.y.device)
    label_idx = get_labels_from_name(idxs, split_idx)
    y[label_idx] = F.one_hot(labels[label_idx], c).float()
    return general_outcome_correlation(A, y, alpha, num_propagations, post_step=Clamp(0, 1), alpha_term=True)


def _label_rows(split_idx, train_only):
    if train_only:
        return torch.cat([split_idx['train']])
    return torch.cat([split_idx['train'], split_idx['valid']])


def _same_graph(A1, A2):
    if A1.graph is not A2.graph:
        raise ValueError('A1 and A2 must be handles over the same graph (one gen_normalized_adjs call)')


def double_correlation_autoscale(data, model_out, split_idx, A1, alpha1, num_propagations1, A2, alpha2, num_propagations2, scale=1.0, train_only=False,
                                 device='cuda', display=True, **trash):
    _same_graph(A1, A2)
    return ops.correct_and_smooth(A1.graph, model_out, _labels(data.y.data), _label_rows(split_idx, train_only), 'double_correlation_autoscale', A1.form,
                                  alpha1, num_propagations1, A2.form, alpha2, num_propagations2, scale=scale, deg_inv_sqrt=A1.deg_inv_sqrt)


def double_correlation_fixed(data, model_out, split_idx, A1, alpha1, num_propagations1, A2, alpha2, num_propagations2, scale=1.0, train_only=False,
                             device='cuda', display=True, **trash):
    _same_graph(A1, A2)
    return ops.correct_and_smooth(A1.graph, model_out, _labels(data.y.data), _label_rows(split_idx, train_only), 'double_correlation_fixed', A1.form,
                                  alpha1, num_propagations1, A2.form, alpha2, num_propagations2, scale=scale, deg_inv_sqrt=A1.deg_inv_sqrt)


def only_outcome_correlation(data, model_out, split_idx, A, alpha, num_propagations, labels, device='cuda', display=True, **trash):
    label_idxs = get_labels_from_name(labels, split_idx)
    return ops.correct_and_smooth(A.graph, model_out, _labels(data.y.data), label_idxs, 'only_outcome_correlation', A.form, alpha, num_propagations,
                                  A.form, alpha, num_propagations, deg_inv_sqrt=A.deg_inv_sqrt)
