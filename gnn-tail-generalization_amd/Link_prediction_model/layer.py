"""`DotPredictor`, `MLPPredictor` and `Heuristics` of the reference's Link_prediction_model/layer.py with its constructor arguments, parameter names
(`lins.{i}.weight` / `.bias`), reset_parameters and same-seed initialisation.  forward(x_i, x_j) is the reference's surface on gathered rows;
score_pairs(h, pairs) is the fused path on the full embedding matrix and an index tensor [2, S]: the gathered rows and their product are never
written (ops.pair_dot / ops.pair_linear, csrc/cb_linkpred.hip).  The other predictors' names are not built here and say what they need; they are
built under names of their own in pair_predictor.py (BilinearPairPredictor, MLPDotPairPredictor, MLPBilPairPredictor, MLPCatPairPredictor).  The encoders' names
(`MLP`, `SAGE`, `GCN`, `WSAGE`, `Transformer`) stand for the torch_geometric modules and raise likewise; all five are built on the HIP path under their
own names in encoder.py (SAGEEncoder, WSAGEEncoder, GCNEncoder, MLPEncoder, TransformerEncoder)."""
import torch

from .. import _lib, gemm, ops, tuning
from ..Link_prediction_baseline.heuristics import eva_heuristics_v2_dec25


class Heuristics(torch.nn.Module):
    """layer.py:6-17: the CN / AA scorer behind `--encoder CN | AA`; it has no parameters and passes features through."""

    def __init__(self, name, data):
        super().__init__()
        self.name, self.data = name, data

    def reset_parameters(self):
        pass

    def forward(self, x, e):
        return x

    def get_score(self, edge_index):
        return eva_heuristics_v2_dec25(self.name, self.data, edge_index)


def _gathered(predictor, h, pairs):
    """predictor.forward on the gathered rows: what score_pairs computes when tuning.T.score_pairs_fused is off."""
    return predictor(h[pairs[0].long()], h[pairs[1].long()])


class DotPredictor(torch.nn.Module):
    """layer.py:182-191: the inner product of the two endpoint rows; no parameters."""

    def __init__(self):
        super().__init__()

    def reset_parameters(self):
        pass

    def forward(self, x_i, x_j):
        _lib.require_device(x_i, x_j)
        return (x_i * x_j).sum(dim=-1)

    def score_pairs(self, h, pairs):
        """[S]: forward(h[pairs[0]], h[pairs[1]]) without the gathers."""
        _lib.require_device(h, pairs)
        return ops.pair_dot(h, pairs) if tuning.T.score_pairs_fused else _gathered(self, h, pairs)


class MLPPredictor(torch.nn.Module):
    """layer.py:85-106: num_layers Linear layers `lins.{i}` of widths in -> hidden -> ... -> out over x_i * x_j, ReLU and dropout between them.  The
    layers are created in order, so a seed gives the reference's initial weights."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.dropout = dropout

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()

    def _tail(self, x, first):
        """lins[first:] on x, the activations of lins[first - 1] (or the product, first == 0)."""
        for lin in self.lins[first:-1]:
            x = gemm.linear(x, lin.weight, lin.bias, relu=True)
            x = ops.dropout(x, self.dropout, training=self.training)
        return gemm.linear(x, self.lins[-1].weight, self.lins[-1].bias) if first < len(self.lins) else x

    def forward(self, x_i, x_j):
        _lib.require_device(x_i, x_j)
        return self._tail(x_i * x_j, 0)

    def score_pairs(self, h, pairs):
        """[S, out_channels]: forward(h[pairs[0]], h[pairs[1]]) with layer 0 through ops.pair_linear (Linear, ReLU and dropout in one kernel where
        the shape allows) and the rest through gemm.linear."""
        _lib.require_device(h, pairs)
        if not tuning.T.score_pairs_fused:
            return _gathered(self, h, pairs)
        l0 = self.lins[0]
        if len(self.lins) == 1:
            return ops.pair_linear(h, pairs, l0.weight, l0.bias)
        x = ops.pair_linear(h, pairs, l0.weight, l0.bias, relu=True, p=self.dropout if self.training else 0.0)
        return self._tail(x, 1)


def _not_built(name, needs):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f'{name} is not built on the HIP path: it needs {needs}')
    return type(name, (torch.nn.Module,), {'__init__': __init__, '__doc__': f'layer.py `{name}`: not built (needs {needs}).'})


MLP = _not_built('MLP', 'a Linear-stack encoder trained through gemm.linear (the teacher GNN is the encoder here)')
SAGE = _not_built('SAGE', "torch_geometric's SAGEConv (mean aggregation with a root weight)")
GCN = _not_built('GCN', "torch_geometric's GCNConv(normalize=False) over data.adj_t")
WSAGE = _not_built('WSAGE', "torch_geometric's GraphConv (edge-weighted sum aggregation with a root weight)")
Transformer = _not_built('Transformer', "torch_geometric's TransformerConv (attention over the edges)")
MLPCatPredictor = _not_built('MLPCatPredictor', 'a concatenating pair operand [h[u] | h[v]] in the first Linear')
MLPDotPredictor = _not_built('MLPDotPredictor', 'a per-node MLP before the pair dot product')
MLPBilPredictor = _not_built('MLPBilPredictor', 'a per-node MLP and a bilinear form before the pair dot product')
BilinearPredictor = _not_built('BilinearPredictor', 'a bilinear form W h[u] before the pair dot product')
