"""The link-prediction experiment of the reference's trainer_link_prediction.py (:215-431) on the HIP path: `trainer(args, which_run).main()` runs
`--runs` runs of `--epochs` epochs of Link_prediction_model.experiment.LinkPredictionModel.train, evaluates with `.test` every `--eval_steps` epochs
under `--eval_metric` ('hits' | 'mrr' | 'recall_my@<k>'), keeps one Logger per result key, prints the reference's per-evaluation lines and, at the
end, the per-run and all-runs statistics with `--eval_last_best`.

Data: the package's datasets (data.load_data) stand where the reference reads ogbl-citation2 / ogbl-collab.  The target nodes (the reference's
`is_unique_in_targetG_mask`) are the nodes outside data.train_mask; with `--exp_on_cold_edge` the target edges are those with
out-degree(src) + in-degree(dst) <= 3 (:150-154).  utils.split_edges makes the train / valid / test edge split from them under --random_seed; a
split assigned to `self.split_edge` before main() is used as it is.  The message graph is all of data.edge_index, as in the reference
(`data.adj_t = edge_index_to_A(data.edge_index)` after the split, :158)."""
import sys
import time

from . import trainer_node_classification as nc
from .Link_prediction_model.experiment import LinkPredictionModel, refuse_edge_lp
from .Link_prediction_model.logger import Logger
from .utils import _degrees_device, split_edges


def result_keys(eval_metric):
    if eval_metric == 'hits':
        return ['Hits@20', 'Hits@50', 'Hits@100']
    if eval_metric == 'mrr':
        return ['MRR']
    if 'recall_my' in eval_metric:
        return ['recall@100%']
    raise ValueError(f"--eval_metric must be 'hits', 'mrr' or 'recall_my@<k>', got {eval_metric!r}")


class trainer:
    def __init__(self, args, which_run):
        self.args, self.which_run = args, which_run
        base = nc.trainer(args, which_run)      # loads the data onto the device, as the node-classification trainer does
        self.data, self.device = base.data, base.device
        self.split_edge = None
        self.model = None

    def make_split_edge(self):
        data, a = self.data, self.args
        n = int(data.x.shape[0])
        if a.exp_on_cold_edge:
            deg_out, deg_in = _degrees_device(n, data.edge_index)
            ei = data.edge_index.long()
            cold = (deg_out[ei[0]].long() + deg_in[ei[1]].long()) <= 3
            return split_edges(data.edge_index, n, target_edge_mask=cold, seed=int(a.random_seed))
        return split_edges(data.edge_index, n, target_node_mask=~data.train_mask, seed=int(a.random_seed))

    def main(self):
        a, data = self.args, self.data
        keys = result_keys(a.eval_metric)
        refuse_edge_lp(a)
        if self.split_edge is None:
            self.split_edge = self.make_split_edge()
        split_edge = self.split_edge
        model = self.model = LinkPredictionModel(a, data, self.device)
        print(f'Total number of model parameters is {sum(p.numel() for p in model.para_list)}')
        loggers = {key: Logger(a.runs, a) for key in keys}
        losses, results_log = [], []
        loss = None
        for run in range(a.runs):
            model.param_init()
            losses.append([])
            results_log.append([])
            start_time = time.time()
            for epoch in range(1, 1 + a.epochs):
                loss = model.train(data, split_edge, batch_size=a.batch_size, neg_sampler_name=a.neg_sampler, num_neg=a.num_neg)
                losses[-1].append(loss)
                if epoch % a.eval_steps == 0:
                    results = model.test(data, split_edge, batch_size=a.batch_size, evaluator=None, eval_metric=a.eval_metric)
                    results_log[-1].append(results)
                    for key, result in results.items():
                        loggers[key].add_result(run, result)
                    if epoch % a.log_steps == 0:
                        spent_time = time.time() - start_time
                        for key, result in results.items():
                            print(key)
                            if 'recall_my' not in a.eval_metric:
                                print(f'Run: {run + 1:02d}, Epoch: {epoch:02d}, Loss: {loss:.4f}, Valid: {100 * result[0]:.2f}%, Test: {100 * result[1]:.2f}%')
                            else:
                                print(f'Run: {run + 1:02d}, Epoch: {epoch:02d}, Loss: {loss:.4f}, \nresult = {result}')
                        print('---')
                        print(f'Training Time Per Epoch: {spent_time / a.eval_steps: .4f} s')
                        print('---')
                        start_time = time.time()
            for key in keys:
                if loggers[key].results[run]:
                    print(key)
                    loggers[key].print_statistics(run, f=sys.stdout, last_best=a.eval_last_best)      # (the stream of now, not of import time)
        for key in keys:
            if a.runs and all(loggers[key].results):
                print(key)
                loggers[key].print_statistics(f=sys.stdout, last_best=a.eval_last_best)
        self.loggers, self.losses, self.results = loggers, losses, results_log
        return loss
