"""`BilinearPredictor`, `MLPDotPredictor`, `MLPBilPredictor` and `MLPCatPredictor` of the reference's Link_prediction_model/layer.py:108-180, 193-203
on the HIP path, under names of their own (layer.py's names stand for what is not built there and keep raising): BilinearPairPredictor,
MLPDotPairPredictor, MLPBilPairPredictor, MLPCatPairPredictor, with the reference's constructor arguments, parameter names (`lins.{i}.weight` /
`.bias`, `bilin.weight`), creation order, reset_parameters and same-seed initialisation.  forward(x_i, x_j) is the reference's surface on gathered
rows, on gemm.linear / ops.dropout / torch elementwise; score_pairs(h, pairs) is the fused route on the full embedding matrix and an index tensor
[2, S] (ops.rows_linear / ops.pair_bilinear / ops.pair_dot, csrc/cb_pairpred.hip): the gathered rows, their concatenation and bilin(x_i) are never
written in the forward.

The 2 S endpoint rows are kept as ONE matrix, rows e < S the x_i side and rows S + e the x_j side (x1 / x2 of the concatenating predictor), in
forward and in score_pairs alike.  Dropout: every layer draws one seed (ops.next_seed) for that [2 S, width] matrix, offset 0 — the keep-mask of
ops.dropout_keep_mask((2 S, width), p, seed) — so the two sides of a pair never share a mask, a self pair included.

Per-node route (MLPDOT, MLPBIL, BIL): with no dropout active the Linear stack is a function of the node alone, so it is applied to the N rows of h
once (gemm.linear) and the pairs are scored on the result, where 2 S >= N — a row count, not a measurement; tuning.T.pair_predictor_per_node forces
either route.  A GEMM row's bits depend on its own K order only, so both routes give the same bits.  BIL has no stack: its two routes are the same
call.  MLPCAT has no such route (splitting its first Linear per node would change the K order).  `routes` records the route of each score_pairs."""
import collections

import torch

from .. import _lib, gemm, ops, tuning
from .layer import DotPredictor, MLPPredictor, _gathered

routes = collections.deque(maxlen=256)      # 'per_node' | 'per_pair' | 'gathered' per score_pairs call, newest last (tests, tools/bench_pairpred.py)


def _per_node(module, h, pairs):
    """The per-node route applies: no dropout is active and the stack over N rows is no more work than over the 2 S endpoint rows."""
    if module.training and module.dropout > 0.0:
        return False
    want = tuning.T.pair_predictor_per_node
    return 2 * pairs.shape[1] >= h.shape[0] if want is None else bool(want)


def _halves(S, device):
    """int32 [2, S]: pair e = rows (e, S + e) of the endpoint matrix."""
    return torch.arange(2 * S, dtype=torch.int32, device=device).reshape(2, S)


class _EndpointStack(torch.nn.Module):
    """The Linear stack of MLPDOT / MLPBIL: Linear(in, hidden) + (num_layers - 1) x Linear(hidden, hidden), EVERY layer followed by ReLU and dropout."""

    def __init__(self, in_channels, hidden_channels, num_layers, dropout):
        super().__init__()
        widths = [in_channels] + [hidden_channels] * num_layers
        self.lins = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.dropout = dropout

    def _p(self):
        return self.dropout if self.training else 0.0

    def _stack(self, x, first=0):
        """lins[first:] with ReLU and dropout on x, a matrix of endpoint (or node) rows."""
        for lin in self.lins[first:]:
            x = ops.dropout(gemm.linear(x, lin.weight, lin.bias, relu=True), self.dropout, training=self.training)
        return x

    def endpoint_rows(self, h, pairs):
        """[2 S, hidden]: the stack on rows (u | v), layer 0 one ops.rows_linear over `pairs` read as [1, 2 S] with ReLU and dropout in the launch."""
        l0 = self.lins[0]
        x = ops.rows_linear(h, pairs.reshape(1, -1), l0.weight, l0.bias, relu=True, p=self._p())
        return self._stack(x, 1)

    def _rows_and_pairs(self, h, pairs):
        """(z, index pairs into z): the stack per node or per endpoint row."""
        if _per_node(self, h, pairs):
            routes.append('per_node')
            return self._stack(h), pairs
        routes.append('per_pair')
        return self.endpoint_rows(h, pairs), _halves(pairs.shape[1], h.device)


class MLPDotPairPredictor(_EndpointStack):
    """layer.py:136-156: the stack on x_i and on x_j (the last layer's ReLU and dropout included), then sum(x_i * x_j, -1), shape [S]."""

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()

    def forward(self, x_i, x_j):
        _lib.require_device(x_i, x_j)
        x = self._stack(torch.cat([x_i, x_j], dim=0))
        S = x_i.shape[0]
        return (x[:S] * x[S:]).sum(dim=-1)

    def score_pairs(self, h, pairs):
        """[S]: forward(h[pairs[0]], h[pairs[1]]) without the gathers; the score is ops.pair_dot on the stack's rows."""
        _lib.require_device(h, pairs)
        if not tuning.T.score_pairs_fused:
            routes.append('gathered')
            return _gathered(self, h, pairs)
        z, zp = self._rows_and_pairs(h, pairs)
        return ops.pair_dot(z, zp)


class MLPBilPairPredictor(_EndpointStack):
    """layer.py:158-180: the same stack, then sum(bilin(x_i) * x_j, -1) with bilin = Linear(hidden, hidden, bias=False) created after the lins."""

    def __init__(self, in_channels, hidden_channels, num_layers, dropout):
        super().__init__(in_channels, hidden_channels, num_layers, dropout)
        self.bilin = torch.nn.Linear(hidden_channels, hidden_channels, bias=False)

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()
        self.bilin.reset_parameters()

    def forward(self, x_i, x_j):
        _lib.require_device(x_i, x_j)
        x = self._stack(torch.cat([x_i, x_j], dim=0))
        S = x_i.shape[0]
        return (gemm.linear(x[:S], self.bilin.weight) * x[S:]).sum(dim=-1)

    def score_pairs(self, h, pairs):
        """[S]: forward(h[pairs[0]], h[pairs[1]]) without the gathers; the score is ops.pair_bilinear on the stack's rows."""
        _lib.require_device(h, pairs)
        if not tuning.T.score_pairs_fused:
            routes.append('gathered')
            return _gathered(self, h, pairs)
        z, zp = self._rows_and_pairs(h, pairs)
        return ops.pair_bilinear(z, zp, self.bilin.weight)


class BilinearPairPredictor(torch.nn.Module):
    """layer.py:193-203: sum(bilin(x_i) * x_j, -1) with bilin = Linear(hidden, hidden, bias=False), shape [S]."""

    def __init__(self, hidden_channels):
        super().__init__()
        self.bilin = torch.nn.Linear(hidden_channels, hidden_channels, bias=False)
        self.dropout = 0.0

    def reset_parameters(self):
        self.bilin.reset_parameters()

    def forward(self, x_i, x_j):
        _lib.require_device(x_i, x_j)
        return (gemm.linear(x_i, self.bilin.weight) * x_j).sum(dim=-1)

    def score_pairs(self, h, pairs):
        """[S]: forward(h[pairs[0]], h[pairs[1]]) as one ops.pair_bilinear: no gather and no bilin(x_i) matrix.  There is no stack in front of the
        bilinear form, so the per-node route is this same call on h."""
        _lib.require_device(h, pairs)
        if not tuning.T.score_pairs_fused:
            routes.append('gathered')
            return _gathered(self, h, pairs)
        routes.append('per_node' if _per_node(self, h, pairs) else 'per_pair')
        return ops.pair_bilinear(h, pairs, self.bilin.weight)


class MLPCatPairPredictor(torch.nn.Module):
    """layer.py:108-134: num_layers Linear layers of widths 2 in -> hidden -> ... -> out on x1 = [x_i | x_j] and on x2 = [x_j | x_i], ReLU and
    dropout after every layer but the last, output (x1 + x2) / 2, shape [S, out]."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout):
        super().__init__()
        widths = [2 * in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = torch.nn.ModuleList(torch.nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.dropout = dropout

    def reset_parameters(self):
        for lin in self.lins:
            lin.reset_parameters()

    def _tail(self, x, first):
        """lins[first:] on x [2 S, width] (rows e: x1, rows S + e: x2), then the mean of the two halves."""
        for lin in self.lins[first:-1]:
            x = ops.dropout(gemm.linear(x, lin.weight, lin.bias, relu=True), self.dropout, training=self.training)
        if first < len(self.lins):
            x = gemm.linear(x, self.lins[-1].weight, self.lins[-1].bias)
        S = x.shape[0] // 2
        return (x[:S] + x[S:]) / 2

    def forward(self, x_i, x_j):
        _lib.require_device(x_i, x_j)
        return self._tail(torch.cat([torch.cat([x_i, x_j], dim=-1), torch.cat([x_j, x_i], dim=-1)], dim=0), 0)

    def score_pairs(self, h, pairs):
        """[S, out_channels]: forward(h[pairs[0]], h[pairs[1]]) with layer 0 as ONE ops.rows_linear of 2 S concatenated rows — index rows
        (u | v) and (v | u) — and the rest through gemm.linear."""
        _lib.require_device(h, pairs)
        if not tuning.T.score_pairs_fused:
            routes.append('gathered')
            return _gathered(self, h, pairs)
        routes.append('per_pair')
        idx = torch.cat([pairs, pairs.flip(0)], dim=1)
        l0 = self.lins[0]
        if len(self.lins) == 1:
            return self._tail(ops.rows_linear(h, idx, l0.weight, l0.bias), 1)
        x = ops.rows_linear(h, idx, l0.weight, l0.bias, relu=True, p=self.dropout if self.training else 0.0)
        return self._tail(x, 1)


# predictor name (upper case) -> constructor from (hidden_channels, num_layers, dropout): model.py:306-319, its argument mapping as written — the 1 of
# MLPDOT / MLPBIL lands in hidden_channels, so through this factory those two have hidden width one
_PAIR_PREDICTORS = {
    'DOT': lambda c, n, p: DotPredictor(),
    'BIL': lambda c, n, p: BilinearPairPredictor(c),
    'MLP': lambda c, n, p: MLPPredictor(c, c, 1, n, p),
    'MLPDOT': lambda c, n, p: MLPDotPairPredictor(c, 1, n, p),
    'MLPBIL': lambda c, n, p: MLPBilPairPredictor(c, 1, n, p),
    'MLPCAT': lambda c, n, p: MLPCatPairPredictor(c, c, 1, n, p),
}


def create_pair_predictor_layer(hidden_channels, num_layers, dropout=0, predictor_name='MLP'):
    """`create_predictor_layer` (model.py:306-319) over all six `--predictor` names, case-insensitive: DOT and MLP are layer.py's classes, the other
    four the classes above; an unknown name raises (the reference returns None)."""
    make = _PAIR_PREDICTORS.get(str(predictor_name).upper())
    if make is None:
        raise NotImplementedError(f'predictor_name {str(predictor_name).upper()} not implemented')
    return make(hidden_channels, num_layers, dropout)
