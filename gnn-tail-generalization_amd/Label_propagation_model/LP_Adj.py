"""LPStep of the reference's Label_propagation_model/LP_Adj.py (:109-160): Correct & Smooth (or plain label propagation when `no_prep`) applied to a
model's class probabilities.  Same constructor and forward(model_out, data); `fn` / `A` / `A1` / `A2` are resolved through tables (the reference
evaluates the option strings), the graph is built on the device at the first forward (or in the constructor when `data` already lives there), and
`lp_force_on_cpu` is ignored: everything runs where model_out lives."""
import torch
import torch.nn as nn

from . import outcome_correlation as oc

FUNCTIONS = {name: getattr(oc, name) for name in ('double_correlation_fixed', 'double_correlation_autoscale', 'only_outcome_correlation')}
ADJ_INDEX = {'DAD': 0, 'DA': 1, 'AD': 2}      # position in gen_normalized_adjs' result


def _resolve(table, name, what):
    if name not in table:
        raise ValueError(f"lpStep.{what} = '{name}': one of {sorted(table)}")
    return table[name]


class LPStep(nn.Module):
    """two papers:
    http://mlg.eng.cam.ac.uk/zoubin/papers/CMU-CALD-02-107.pdf
    https://github.com/CUAI/CorrectAndSmooth
    """

    def __init__(self, args, data, split_masks):
        super().__init__()
        self.train_cnt = 0
        self.args = args
        dev = data.edge_index.device
        self.train_idx = torch.where(split_masks['train'])[0].to(dev)
        self.split_idx = {'train': self.train_idx}
        for k in ('valid', 'test'):
            if split_masks.get(k) is not None:
                self.split_idx[k] = torch.where(split_masks[k])[0].to(dev)
        lp = args.lpStep
        self.no_prep = lp.no_prep
        self.fn_name, self.adj_names = lp.fn, {'A': lp.A, 'A1': lp.A1, 'A2': lp.A2}
        self.fn = _resolve(FUNCTIONS, lp.fn, 'fn')
        for k, v in self.adj_names.items():
            _resolve(ADJ_INDEX, v, k)
        self.lp_dict = {
            'train_only': True,
            'alpha1': lp.alpha1,
            'alpha2': lp.alpha2,
            'num_propagations1': lp.num_propagations1,
            'num_propagations2': lp.num_propagations2,
            'display': False,
            'device': getattr(args, 'device', dev),
            # below: lp only
            'idxs': ['train'],
            'alpha': lp.alpha,
            'num_propagations': lp.num_propagations,
        }
        self.adjs = None
        if data.edge_index.is_cuda:
            self._build(data)

    def _build(self, data):
        adj, D_isqrt = oc.process_adj(data)
        self.adjs = oc.gen_normalized_adjs(adj, D_isqrt)
        for k, v in self.adj_names.items():
            self.lp_dict[k] = self.adjs[ADJ_INDEX[v]]

    def forward(self, model_out, data):
        # need to pass 'data.y' through 'data'
        self.train_cnt += 1
        if self.adjs is None:
            self._build(data)
        dev = self.adjs[0].graph.device
        split_idx = {k: v.to(dev) for k, v in self.split_idx.items()}
        model_out = model_out.to(dev)
        if self.no_prep:
            return oc.label_propagation(data, split_idx, **self.lp_dict)
        if self.fn is oc.only_outcome_correlation:
            _, out = self.fn(data, model_out, split_idx, labels=self.lp_dict['idxs'], **self.lp_dict)
        else:
            _, out = self.fn(data, model_out, split_idx, **self.lp_dict)
        return out
