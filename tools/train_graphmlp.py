"""Trains GraphMLP (MLP_model.GraphMLP: the MLP with the neighbour-contrastive loss, https://arxiv.org/abs/2106.04051) on the HIP path with the
package's options — what the reference runs for --train_which=GraphMLP (trainer.train_graphMLP; main.py does not route there yet):
    python tools/train_graphmlp.py --dataset=Cora --epochs=100 --batch_size=2048 --graphMLP_reg=10 --graphMLP_tau=2.0 --graphMLP_r=3
Loops over --N_exp seeds like main.py and returns / prints the per-seed record arrays [record_type, epochs]; weights -> saved_models/.../seMLP.
--power_on_device=1 (this tool's own flag, taken off the command line before the package's options are parsed) builds the adjacency power with
the device product: it sets tuning.T.power_on_device for the run."""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import main as cb_main  # noqa: E402
from gnn_tail_generalization_amd.base_options import BaseOptions  # noqa: E402


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    own = [a for a in argv if a.startswith('--power_on_device')]
    argv = [a for a in argv if a not in own]
    for a in own:
        if a not in ('--power_on_device=0', '--power_on_device=1'):
            raise SystemExit('tools/train_graphmlp.py: --power_on_device=0 or --power_on_device=1')
    if not any(a.startswith('--train_which') for a in argv):
        argv.append('--train_which=GraphMLP')
    args = BaseOptions().get_arguments(argv)
    if args.train_which != 'GraphMLP':
        raise SystemExit('tools/train_graphmlp.py trains GraphMLP: use main.py for --train_which=' + str(args.train_which))
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    from gnn_tail_generalization_amd.utils import save_graph_analyze
    if own:
        from gnn_tail_generalization_amd import tuning
        tuning.T.power_on_device = own[-1].endswith('=1')
    recs = []
    for seed in range(args.N_exp):
        print(f'seed (which_run) = <{seed}>')
        args.random_seed = seed
        cb_main.set_seed(args)
        trnr = trainer(args, seed)
        if args.do_deg_analyze:                      # as trainer.main() does: the head / tail (/ isolated) node sets of --want_headtail
            save_graph_analyze(args.N_nodes, trnr.data, args.use_special_split)
        rows = trnr.train_graphMLP()
        print(f'GraphMLP (reg {args.graphMLP_reg}, tau {args.graphMLP_tau}, r {args.graphMLP_r}): test accuracy of the last epoch {rows[0][-1]:.2f}, '
              f'last training loss {trnr.bag["graphMLP_loss_train"][-1]:.4f}')
        recs.append(rows)
        del trnr
        torch.cuda.empty_cache()
        gc.collect()
    return recs


if __name__ == '__main__':
    main()
