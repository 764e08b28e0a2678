"""`LinkPredictionModel`: the counterpart of the reference's `BaseModel` (Link_prediction_model/model.py:7-266) on the HIP path — the epoch and
test protocol of the link-prediction experiment over the parts that exist: create_input_layer's embedding, create_encoder_layer's encoders (or the
TransformerEncoder), the trainer's predictor mapping, calculate_loss, the fused Adam, the device samplers and shuffle of csrc/cb_lpx.hip and the
tie-safe metrics.

train()   model.py:121-169.  One draw of negatives for ALL train positives per epoch with the named sampler; one seeded permutation per epoch, cut
          into batches of batch_size (the last one shorter) where the reference iterates a shuffling DataLoader; per batch an encoder forward over the
          whole graph, predictor.score_pairs on the batch's positives and on its num_neg negatives each, calculate_loss, backward, the two separate
          clip_grad_norm_ calls, a step.  Returns sum(loss_b n_b) / sum(n_b), accumulated on the device in float64 and read ONCE per epoch; the
          sampler's, the pair operators' and the device status words are read there too, never per batch.
test()    model.py:187-266.  Eval-mode embeddings once; train negatives always 'global'; six batch_predict calls; 'hits' | 'mrr' | 'recall_my@...'.
The message graph is a graph.CSRGraph of data.edge_index.  data.edge_weight (a float tensor, one value per column of edge_index) makes it an adjacency
with values (graph.WeightedAdj), which the GCN / WSAGE layers multiply by and SAGE / Transformer / MLP ignore.  args.normalize_adj (default 0) applies
the reference's gcn_normalization for GCN and adj_normalization for WSAGE (trainer_link_prediction.py:333-338) once, in the constructor; the
reference normalises unconditionally — here it is a switch, so that the default stays the adjacency as given.  The samplers and the CN / AA scores
read the structure.  split_edge['train']['weight'] (the per-edge margins) stays refused.  edge_LP.py (`--edge_lp_mode`) is not built."""
import types

import torch

from .. import _lib, ops
from .. import optim as cb_optim
from ..graph import INT32_EDGE_LIMIT, CSRGraph, WeightedAdj, build_graph
from . import negative_sample
from .model import calculate_loss, create_encoder_layer, create_input_feat, create_input_layer, reset_input_layer
from .utils import adj_normalization, evaluate_hits, evaluate_mrr, evaluate_recall_my, gcn_normalization, get_pos_neg_edges

HEURISTICS = ('CN', 'AA', 'PPR')


def refuse_edge_lp(args):
    mode = getattr(args, 'edge_lp_mode', '')
    if mode != '':
        raise NotImplementedError(
            f"--edge_lp_mode={mode} is not built: the reference's edge_LP.py builds its edge graph from positions inside a node's edge set, not from edge "
            'ids (mutual_intermix), and its size does not match the score vector it propagates, so there is no defined result to reproduce; '
            "pass --edge_lp_mode=''")


def message_adjacency(args, data, num_nodes, device):
    """(graph, adj): the CSRGraph of data.edge_index (samplers, heuristics) and what the encoder is handed in place of the reference's data.adj_t — the
    graph itself, or a graph.WeightedAdj: data.edge_weight as given, or, under args.normalize_adj, gcn_normalization of it for `GCN` and
    adj_normalization for `WSAGE` (trainer_link_prediction.py:333-338; unit values where the data carries none), applied once, here."""
    encoder_name = str(args.encoder)
    if getattr(data, 'edge_attr', None) is not None:
        raise NotImplementedError('data.edge_attr: edge features are not built for the link-prediction experiment (one real value per edge: data.edge_weight)')
    edge_weight = getattr(data, 'edge_weight', None)
    if edge_weight is not None and encoder_name in HEURISTICS:
        raise NotImplementedError('data.edge_weight: the CN / AA / PPR scores count neighbours and read no edge values')
    normalize = int(getattr(args, 'normalize_adj', 0) or 0) and encoder_name.upper() in ('GCN', 'WSAGE')
    valued = edge_weight is not None or normalize
    if valued and int(data.edge_index.shape[1]) < INT32_EDGE_LIMIT:      # (edge values are looked up through the kept edge order)
        graph = CSRGraph(data.edge_index, num_nodes, keep_edge_order=True)
    else:
        graph = build_graph(data.edge_index, num_nodes)
    if not isinstance(graph, CSRGraph):
        raise NotImplementedError('the experiment needs the whole int32-indexed graph on this device; segmented and node-sharded graphs are not built for it')
    if not valued:
        return graph, graph
    if edge_weight is not None and (not torch.is_tensor(edge_weight) or not edge_weight.is_floating_point() or edge_weight.numel() != graph.E):
        raise ValueError(f'data.edge_weight: a float tensor of {graph.E} elements (one per column of edge_index) expected')
    w = edge_weight.to(device) if edge_weight is not None else torch.ones(graph.E, dtype=torch.float32, device=device)
    adj = WeightedAdj(graph, w)
    if normalize:
        adj = (gcn_normalization if encoder_name.upper() == 'GCN' else adj_normalization)(adj)
    return graph, adj


class LinkPredictionModel(object):
    def __init__(self, args, data, device=None):
        a = self.args = args
        self.device = torch.device(device if device is not None else data.x.device)
        self.encoder_name = str(a.encoder)
        self.loss_func_name = a.loss_func
        self.clip_norm = a.grad_clip_norm
        self.use_node_feats = a.use_node_feats
        self.num_nodes = int(data.x.shape[0]) if getattr(data, 'x', None) is not None else int(data.num_nodes)
        if str(a.optimizer) != 'Adam':
            raise NotImplementedError(f'--optimizer {a.optimizer} is not built on the HIP path: optim.py has the fused Adam only')
        if getattr(a, 'linkpred_baseline', '') in ('EGI', 'DGI'):
            raise NotImplementedError(f'--linkpred_baseline {a.linkpred_baseline} is not built')
        self.graph, self.adj = message_adjacency(a, data, self.num_nodes, self.device)
        self.sampler = negative_sample.sampler_of(self.graph)
        self.emb = self.encoder = self.predictor = self.optimizer = None
        self.para_list = []
        self.steps = 0                       # optimizer steps taken since param_init()
        self.last_epoch = None               # what the last train() drew: dict(pos, neg, perm, batch_losses, batch_sizes), device tensors
        if self.encoder_name in HEURISTICS:
            if self.encoder_name == 'PPR':
                ops.pair_scores(self.graph, torch.zeros((2, 0), dtype=torch.int32, device=self.device), 'PPR')      # raises: says what PPR needs
            return
        num_feats = int(data.x.shape[1]) if getattr(data, 'x', None) is not None else 0
        input_dim, self.emb = create_input_layer(self.num_nodes, num_feats, a.emb_hidden_channels, a.use_node_feats, a.train_node_emb, a.pretrain_emb)
        if self.emb is not None:
            self.emb = self.emb.to(self.device)
        if self.encoder_name.upper() == 'TRANSFORMER':      # (create_encoder_layer's name stands for the torch_geometric module and raises)
            from .encoder import TransformerEncoder
            self.encoder = TransformerEncoder(input_dim, a.gnn_hidden_channels, a.gnn_hidden_channels, a.gnn_num_layers, a.dropout).to(self.device)
        else:
            self.encoder = create_encoder_layer(input_dim, a.gnn_hidden_channels, a.gnn_num_layers, a.dropout, self.encoder_name).to(self.device)
        from ..trainer_node_classification import trainer as nc_trainer
        self.predictor = nc_trainer._linkpred_predictor(types.SimpleNamespace(args=a, device=self.device), a.gnn_hidden_channels)
        self.para_list = list(self.encoder.parameters()) + list(self.predictor.parameters()) + (list(self.emb.parameters()) if self.emb is not None else [])
        self._new_optimizer()

    def _new_optimizer(self):
        self.optimizer = cb_optim.Adam(self.para_list, lr=self.args.lr) if self.para_list else None
        self.steps = 0

    def param_init(self):
        """New parameters and a new optimizer state for a run (model.py:90-94)."""
        if self.encoder is None:
            return
        self.encoder.reset_parameters()
        self.predictor.reset_parameters()
        reset_input_layer(self.emb)
        self._new_optimizer()

    def create_input_feat(self, data):
        return create_input_feat(self.emb, data.x, self.use_node_feats)

    def embeddings(self, data):
        return self.encoder(self.create_input_feat(data), self.adj)

    def train(self, data, split_edge, batch_size, neg_sampler_name, num_neg):
        if self.encoder_name in HEURISTICS:
            return -1.
        if 'weight' in split_edge['train']:
            raise NotImplementedError("split_edge['train']['weight']: the per-edge margins of adaptive_auc_loss (real-valued edge weights) are not built")
        batch_size, num_neg = int(batch_size), int(num_neg)
        if batch_size < 1 or num_neg < 1:
            raise ValueError('train: batch_size >= 1 and num_neg >= 1 required')
        self.encoder.train()
        self.predictor.train()
        pos_train_edge, neg_train_edge = get_pos_neg_edges('train', split_edge, graph=self.graph, num_nodes=self.num_nodes,
                                                           neg_sampler_name=neg_sampler_name, num_neg=num_neg)
        pos_train_edge = pos_train_edge.to(self.device)
        P = int(pos_train_edge.size(0))
        if P == 0:
            raise ValueError('train: the train split holds no positive edge')
        perm = ops.seeded_permutation(P, device=self.device).long()
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        batch_losses, batch_sizes = [], []
        for at in range(0, P, batch_size):
            idx = perm[at:at + batch_size]
            self.optimizer.zero_grad()
            h = self.embeddings(data)
            pos_edge = pos_train_edge[idx].t()
            neg_edge = neg_train_edge[idx].reshape(-1, 2).t()
            pos_out = self.predictor.score_pairs(h, pos_edge)
            neg_out = self.predictor.score_pairs(h, neg_edge)
            loss = calculate_loss(self.loss_func_name, pos_out, neg_out, num_neg)
            loss.backward()
            if self.clip_norm >= 0:
                for module in (self.encoder, self.predictor):
                    if list(module.parameters()):
                        torch.nn.utils.clip_grad_norm_(module.parameters(), self.clip_norm)
            self.optimizer.step()
            self.steps += 1
            n_b = int(pos_out.size(0))
            value = loss.detach().reshape(())
            total += value.to(torch.float64) * n_b
            batch_losses.append(value)
            batch_sizes.append(n_b)
        self.last_epoch = dict(pos=pos_train_edge, neg=neg_train_edge, perm=perm, batch_losses=batch_losses, batch_sizes=batch_sizes)
        result = float(total.item()) / P      # the one host read of the epoch; the status words follow it
        self._checks()
        return result

    def _checks(self):
        self.sampler.check()
        ops.pair_check()
        ops.pair_scores_check()
        _lib.device_status()

    @torch.no_grad()
    def batch_predict(self, h, edges, batch_size):
        """float32 [n] scores of edges [n, 2], on the device: predictor.score_pairs in chunks of batch_size; CN / AA: ops.pair_scores on the message graph."""
        edges = edges.to(self.device)
        if self.encoder_name in HEURISTICS:
            return ops.pair_scores(self.graph, edges.t(), self.encoder_name)
        preds = [self.predictor.score_pairs(h, edges[at:at + int(batch_size)].t()).reshape(-1) for at in range(0, int(edges.size(0)), int(batch_size))]
        return torch.cat(preds, dim=0) if preds else torch.zeros(0, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def test(self, data, split_edge, batch_size, evaluator=None, eval_metric='hits'):
        refuse_edge_lp(self.args)
        h = None
        if self.encoder is not None:
            self.encoder.eval()
            self.predictor.eval()
            h = self.embeddings(data)
        pos_train_edge, neg_train_edge = get_pos_neg_edges('train', split_edge, graph=self.graph, num_nodes=self.num_nodes, neg_sampler_name='global',
                                                           num_neg=self.args.num_neg)
        neg_train_edge = neg_train_edge.reshape(-1, 2)
        pos_valid_edge, neg_valid_edge = get_pos_neg_edges('valid', split_edge)
        pos_test_edge, neg_test_edge = get_pos_neg_edges('test', split_edge)
        pos_train_pred = self.batch_predict(h, pos_train_edge, batch_size)
        neg_train_pred = self.batch_predict(h, neg_train_edge, batch_size)
        pos_valid_pred = self.batch_predict(h, pos_valid_edge, batch_size)
        neg_valid_pred = self.batch_predict(h, neg_valid_edge, batch_size)
        pos_test_pred = self.batch_predict(h, pos_test_edge, batch_size)
        neg_test_pred = self.batch_predict(h, neg_test_edge, batch_size)
        self._checks()
        if eval_metric == 'hits':
            return evaluate_hits(evaluator, pos_valid_pred, neg_valid_pred, pos_test_pred, neg_test_pred)
        if eval_metric == 'mrr':
            return evaluate_mrr(evaluator, pos_valid_pred, neg_valid_pred, pos_test_pred, neg_test_pred)
        if 'recall_my' in eval_metric:
            return evaluate_recall_my(pos_train_pred, neg_train_pred, pos_valid_pred, neg_valid_pred, pos_test_pred, neg_test_pred,
                                      topk=eval_metric.split('@')[1])
        raise ValueError(f"eval_metric must be 'hits', 'mrr' or 'recall_my@<k>', got {eval_metric!r}")
