"""Trains the teacher GNN as the encoder of the reference's link-prediction experiment (Link_prediction_model/: `--predictor DOT | MLP | BIL | MLPDOT | MLPBIL | MLPCAT`,
`--loss_func AUC | ce_loss | log_rank_loss | info_nce_loss`, `--num_neg`, `--batch_size`, `--grad_clip_norm`) on the HIP path
(trainer.train_teacherGNN_linkpred; main.py does not route there):
    python tools/train_linkpred.py --dataset=S-tiny --predictor=MLP --loss_func=log_rank_loss --num_neg=3 --epochs=20
Every step scores --batch_size sampled positives and --num_neg negatives each through predictor.score_pairs on the teacher's embeddings.  Loops over
--N_exp seeds like main.py; returns / prints per seed (losses [epochs], {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} of a test-mode sample)."""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import main as cb_main  # noqa: E402
from gnn_tail_generalization_amd.base_options import BaseOptions  # noqa: E402


def main(argv=None):
    args = BaseOptions().get_arguments(list(sys.argv[1:] if argv is None else argv))
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    recs = []
    for seed in range(args.N_exp):
        print(f'seed (which_run) = <{seed}>')
        args.random_seed = seed
        cb_main.set_seed(args)
        trnr = trainer(args, seed)
        losses, metrics = trnr.train_teacherGNN_linkpred()
        print(f'link prediction ({args.predictor}, {args.loss_func}, num_neg {args.num_neg}): loss first / last epoch {losses[0]:.5f} / {losses[-1]:.5f}; '
              + ', '.join(f'{k} {v:.4f}' for k, v in metrics.items()))
        recs.append((losses, metrics))
        del trnr
        torch.cuda.empty_cache()
        gc.collect()
    return recs


if __name__ == '__main__':
    main()
