"""The reference's Link_prediction_model/utils.py:7-91 — `get_pos_neg_edges` and the three `evaluate_*` — over the device samplers and the tie-safe
counts of csrc/cb_heur.hip / cb_lpx.hip.  Result keys are the reference's ('Hits@20' | 'Hits@50' | 'Hits@100', 'MRR', 'recall@100%').  Where the
reference takes an OGB `evaluator`, the argument is kept (None) and ignored: Hits@K is ops.hits_at_k (the OGB rule on counts), the MRR is the current
OGB evaluator's rule rank = 1 + #above + #equal / 2 (ops.mrr_from_counts).  `gcn_normalization` / `adj_normalization` (utils.py:93-106) take and return
a graph.WeightedAdj where the reference takes a torch_sparse adj_t (ops.adj_normalize, csrc/cb_adjnorm.hip).  `generate_neg_dist_table` is not built."""
import torch

from .. import ops
from .negative_sample import global_neg_sample, global_perm_neg_sample, local_neg_sample


def get_pos_neg_edges(split, split_edge, graph=None, num_nodes=None, neg_sampler_name=None, num_neg=None):
    """(pos_edge [P, 2], neg_edge) of `split` (utils.py:7-41), for the 'edge' / 'edge_neg' form of split_edge and for the 'source_node' /
    'target_node' / 'target_node_neg' form.  'train': the negatives are drawn with the named sampler ('local', 'global', anything else: the
    permuted global copies) as [P, num_neg, 2] — `graph` (a graph.CSRGraph) stands where the reference passes edge_index; other splits: the
    stored negatives, [*, 2]."""
    train = split_edge['train']
    if 'edge' in train:
        pos_edge = split_edge[split]['edge']
    elif 'source_node' in train:
        source, target = split_edge[split]['source_node'], split_edge[split]['target_node']
        pos_edge = torch.stack([source, target]).t()
    else:
        raise KeyError("split_edge['train'] holds neither 'edge' nor 'source_node'")
    if split == 'train':
        if neg_sampler_name == 'local':
            neg_edge = local_neg_sample(pos_edge, num_nodes=num_nodes, num_neg=num_neg)
        elif neg_sampler_name == 'global':
            neg_edge = global_neg_sample(graph, num_nodes=num_nodes, num_samples=pos_edge.size(0), num_neg=num_neg)
        else:
            neg_edge = global_perm_neg_sample(graph, num_nodes=num_nodes, num_samples=pos_edge.size(0), num_neg=num_neg)
    elif 'edge' in train:
        neg_edge = split_edge[split]['edge_neg']
    else:
        target_neg = split_edge[split]['target_node_neg']
        neg_edge = torch.stack([source.repeat_interleave(target_neg.size(1)), target_neg.reshape(-1)]).t()
    return pos_edge, neg_edge


def gcn_normalization(adj_t):
    """utils.py:93-99: D^-1/2 (A with its diagonal set to 1) D^-1/2 of a graph.WeightedAdj, as a new one (ops.adj_normalize 'gcn')."""
    return ops.adj_normalize(adj_t, 'gcn')


def adj_normalization(adj_t):
    """utils.py:101-106: D^-1 A of a graph.WeightedAdj, as a new one (ops.adj_normalize 'adj')."""
    return ops.adj_normalize(adj_t, 'adj')


def _f32(t):
    return t.detach().reshape(-1).to(torch.float32)


def evaluate_hits(evaluator, pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred):
    """{'Hits@K': (valid, test)} for K = 20, 50, 100 (utils.py:43-59): every positive against all negatives of its split."""
    valid = ops.hits_at_k(_f32(pos_val_pred), _f32(neg_val_pred), (20, 50, 100))
    test = ops.hits_at_k(_f32(pos_test_pred), _f32(neg_test_pred), (20, 50, 100))
    return {key: (valid[key], test[key]) for key in valid}


def _mrr(pos, neg):
    pos, neg = _f32(pos), _f32(neg)
    P = pos.numel()
    if P == 0 or neg.numel() % P:
        raise ValueError(f'evaluate_mrr: {neg.numel()} negative scores do not split into rows of {P} positives')
    gt, eq, status = ops.row_rank_counts(pos, neg.view(P, -1), return_status=True)
    return ops.mrr_from_counts(gt, eq, status)['MRR']


def evaluate_mrr(evaluator, pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred):
    """{'MRR': (valid, test)} (utils.py:61-80): positive i is ranked among ITS negatives, row i of the negatives read as [P, Nn / P].  (The
    reference's `neg.view(neg.shape[0], -1)` makes rows of one negative each; the commented line above it is what the OGB evaluator needs.)"""
    return {'MRR': (_mrr(pos_val_pred, neg_val_pred), _mrr(pos_test_pred, neg_test_pred))}


def evaluate_recall_my(pos_train_pred, neg_train_pred, pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred, topk=None):
    """{'recall@100%': (train, valid, test)} (utils.py:82-91): `cal_recall` of each split, ops.recall_at_topk."""
    return {'recall@100%': tuple(ops.recall_at_topk(_f32(p), _f32(n), topk) for p, n in
                                 ((pos_train_pred, neg_train_pred), (pos_val_pred, neg_val_pred), (pos_test_pred, neg_test_pred)))}
