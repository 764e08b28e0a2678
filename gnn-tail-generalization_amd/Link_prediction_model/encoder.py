"""The encoders of the reference's Link_prediction_model/layer.py:19-75 (`SAGE`, `WSAGE`, `GCN`, `MLP` over `BaseGNN`) on the HIP path, under new names
next to the refusing `layer.SAGE` / `GCN` / `WSAGE` / `MLP` (which keep raising: they stand for the torch_geometric modules):

    SAGEEncoder    convs.{i} = PyG SAGEConv(mean, root weight):   (A X / indeg) lin_l^T + lin_l.bias + X lin_r^T       (rows without in-edges: mean 0)
    WSAGEEncoder   convs.{i} = PyG GraphConv(add), no edge weight: (A X) lin_rel^T + lin_rel.bias + X lin_root^T
    GCNEncoder     convs.{i} = PyG GCNConv(normalize=False):       (A X) lin^T + bias
    MLPEncoder     convs.{i} = torch.nn.Linear, through gemm.linear
    TransformerEncoder  convs.{i} = PyG TransformerConv(first, second) with every default (layer.py:77-83): heads = 1, concat, no beta, no edge
                   features, no attention dropout, bias, root weight.  With Q, K, V, S = lin_query / lin_key / lin_value / lin_skip of X (all with bias):
                       out[v] = sum_j softmax_j(<Q[v], K[u_j]> / sqrt(out)) V[u_j] + S[v]      over the in-edges (u_j -> v), duplicates each their own term;
                   a row without in-edges gives S[v].  One stacked GEMM and one attention kernel per layer (ops.transformer_conv, csrc/cb_attn.hip);
                   out_channels % 4 == 0 and <= 512.  PyG's 1e-16 in the softmax's denominator is dropped (invisible in fp32 once the maximum is
                   subtracted); heads > 1, edge_dim and beta are not built.

ReLU then dropout after every layer but the last (layer.py:29-35).  forward(x, graph) takes a graph.CSRGraph where the reference takes PyG's adj_t; every
SAGE / WSAGE / GCN layer is one ops.sage_layer call (csrc/cb_sage.hip where the widths are 256 -> 256, the composed kernels elsewhere).  `graph` may also
be a graph.WeightedAdj — an adj_t with values (real edge weights, gcn_normalization / adj_normalization of Link_prediction_model/utils.py): GraphConv and
GCNConv then multiply each gathered row by its edge's value, agg[v] = sum_e w_e x[u_e] (csrc/cb_ewlayer.hip); SAGEConv, TransformerConv and the MLP read
the structure alone and give the same bits with or without values.

Constructor arguments, parameter names and shapes ([out, in]) are PyG's, created layer by layer in PyG's order.  Initial values: every weight and bias
is drawn by torch.nn.Linear's reset_parameters (kaiming_uniform with a = sqrt(5); GCN's bias likewise from its Linear).  torch_geometric is not
available to compare against, so equality of same-seed initial values with PyG is NOT claimed (PyG's Linear uses its own glorot / zeros defaults for
some of these)."""
import torch

from .. import _lib, gemm, ops


def structure(graph):
    """The CSRGraph of what an encoder was handed: a graph.WeightedAdj's .graph, anything else as it is.  The layers that do not read edge values
    (SAGEConv: PyG drops them; TransformerConv: the reference strips them, trainer_link_prediction.py:340-342) see the structure alone."""
    return getattr(graph, 'graph', graph)


class _Conv(torch.nn.Module):
    """The parameters of one graph layer under PyG's names.  names = (neighbour Linear, self Linear or None); the neighbour Linear carries the bias."""
    mode, names = None, None

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        n, s = self.names
        setattr(self, n, torch.nn.Linear(in_channels, out_channels, bias=True))
        if s is not None:
            setattr(self, s, torch.nn.Linear(in_channels, out_channels, bias=False))

    def reset_parameters(self):
        for name in self.names:
            if name is not None:
                getattr(self, name).reset_parameters()

    def params(self):
        """(W_n, W_s or None, bias)"""
        n, s = self.names
        return getattr(self, n).weight, (getattr(self, s).weight if s is not None else None), getattr(self, n).bias

    def forward(self, x, graph, relu=False, p=0.0):
        W_n, W_s, b = self.params()
        return ops.sage_layer(graph, x, W_n, W_s, b, mode=self.mode, relu=relu, p=p)


class SAGEConv(_Conv):
    mode, names = 'SAGE', ('lin_l', 'lin_r')

    def forward(self, x, graph, relu=False, p=0.0):
        return super().forward(x, structure(graph), relu=relu, p=p)


class GraphConv(_Conv):
    mode, names = 'WSAGE', ('lin_rel', 'lin_root')


class GCNConv(torch.nn.Module):
    """PyG GCNConv(normalize=False): `lin.weight` without a bias of its own and a separate `bias` parameter."""
    mode = 'GCN'

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        tmp = torch.nn.Linear(self.in_channels, self.out_channels, bias=True)      # (torch.nn.Linear's reset, weight then bias)
        with torch.no_grad():
            self.lin.weight.copy_(tmp.weight)
            self.bias.copy_(tmp.bias)

    def params(self):
        return self.lin.weight, None, self.bias

    def forward(self, x, graph, relu=False, p=0.0):
        return ops.sage_layer(graph, x, self.lin.weight, None, self.bias, mode='GCN', relu=relu, p=p)


class TransformerConv(torch.nn.Module):
    """PyG TransformerConv(in_channels, out_channels) with every default: four Linears with bias, created in PyG's order (key, query, value, skip)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        for name in ('lin_key', 'lin_query', 'lin_value', 'lin_skip'):
            setattr(self, name, torch.nn.Linear(in_channels, out_channels, bias=True))

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
            lin.reset_parameters()

    def forward(self, x, graph, relu=False, p=0.0):
        y = ops.transformer_conv(structure(graph), x, self.lin_key.weight, self.lin_key.bias, self.lin_query.weight, self.lin_query.bias, self.lin_value.weight,
                                 self.lin_value.bias, self.lin_skip.weight, self.lin_skip.bias, relu=relu)
        return ops.dropout(y, p, training=True) if p else y


class _Encoder(torch.nn.Module):
    conv = None

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        self.convs = torch.nn.ModuleList()
        self.dropout = dropout
        for i in range(num_layers):
            first = in_channels if i == 0 else hidden_channels
            second = out_channels if i == num_layers - 1 else hidden_channels
            self.convs.append(self.conv(first, second))

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, x, graph):
        _lib.require_device(x)
        p = self.dropout if self.training else 0.0
        for conv in self.convs[:-1]:
            x = conv(x, graph, relu=True, p=p)
        return self.convs[-1](x, graph)


class SAGEEncoder(_Encoder):
    """layer.py:53-59 `SAGE`."""
    conv = SAGEConv


class WSAGEEncoder(_Encoder):
    """layer.py:69-75 `WSAGE` (edge values where the graph is a WeightedAdj)."""
    conv = GraphConv


class GCNEncoder(_Encoder):
    """layer.py:61-67 `GCN`."""
    conv = GCNConv


class TransformerEncoder(_Encoder):
    """layer.py:77-83 `Transformer`."""
    conv = TransformerConv


class MLPEncoder(_Encoder):
    """layer.py:37-51 `MLP`: Linear layers `convs.{i}`; the graph argument is not read."""
    conv = torch.nn.Linear

    def forward(self, x, graph=None):
        _lib.require_device(x)
        for lin in self.convs[:-1]:
            x = gemm.linear(x, lin.weight, lin.bias, relu=True)
            x = ops.dropout(x, self.dropout, training=self.training)
        return gemm.linear(x, self.convs[-1].weight, self.convs[-1].bias)
