"""`CN`, `AA`, `eva_heuristics_v2_dec25` and `tonp` of the reference's Link_prediction_baseline/heuristics.py (:10-29, 107-129, 165-169) with the
adjacency held as a device `graph.CSRGraph` instead of a scipy matrix: the scores come from ops.pair_scores (csrc/cb_heur.hip), a sorted-row
intersection per pair instead of `A[src].multiply(A_[dst])` on the host.  Multi-edges count with their multiplicity, as scipy's summed duplicates
do.  Not built: `eva_heuristics` / `get_pos_neg_edges` (they need PyG's split objects), real-valued edge weights, and `PPR` (it needs the
fast_pagerank package)."""
import numpy as np
import torch

from .. import ops
from ..graph import CSRGraph


def tonp(arr):
    if type(arr) is torch.Tensor:
        return arr.detach().cpu().data.numpy()
    return np.asarray(arr)


def _scores(kind, A, edge_index):
    if type(A) is not CSRGraph:
        raise ValueError(f'{kind}: A must be a whole square graph.CSRGraph (segmented and node-sharded graphs are out of scope)')
    pairs = torch.as_tensor(tonp(edge_index) if not torch.is_tensor(edge_index) else edge_index)
    if pairs.dtype not in (torch.int32, torch.int64):
        pairs = pairs.to(torch.int64)
    scores = ops.pair_scores(A, pairs.to(A.device), kind).cpu()      # the host read of the reference's FloatTensor: the status is read here too
    ops.pair_scores_check()
    return scores, edge_index


def CN(A, edge_index, batch_size=100000):
    """The common-neighbour score of every column of edge_index [2, P]: (FloatTensor [P] on the host, edge_index).  batch_size is accepted and
    ignored: nothing is batched."""
    return _scores('CN', A, edge_index)


def AA(A, edge_index, batch_size=100000):
    """The Adamic-Adar score of every column of edge_index [2, P]: (FloatTensor [P] on the host, edge_index)."""
    return _scores('AA', A, edge_index)


def PPR(A, edge_index):
    raise NotImplementedError("'PPR' is not built: the reference's personalised PageRank needs the fast_pagerank package, which is absent here")


_HEURISTICS = {'CN': CN, 'AA': AA, 'PPR': PPR}


def eva_heuristics_v2_dec25(which_heuristic, data, edge_index):
    """The scores of `edge_index` under 'CN' or 'AA' as a numpy array (:10-29).  The device graph of data.edge_index is cached on `data.A` if absent.
    The graph is scored as given: holding the evaluated edges out of it is the caller's job."""
    if which_heuristic not in _HEURISTICS:
        raise ValueError(f"which_heuristic must be 'CN', 'AA' or 'PPR', got {which_heuristic!r}")
    if which_heuristic == 'PPR':
        PPR(None, edge_index)
    for name in ('edge_attr', 'edge_weight'):
        if getattr(data, name, None) is not None:
            raise NotImplementedError(f'data.{name}: real-valued edge weights are not built (an edge counts with its multiplicity in edge_index)')
    if getattr(data, 'A', None) is None:
        n = getattr(data, 'num_nodes', None)
        data.A = CSRGraph(data.edge_index, int(data.x.shape[0]) if n is None else int(n))
    pred_scores, _ = _HEURISTICS[which_heuristic](data.A, edge_index)
    return tonp(pred_scores)
