"""Trains the reference's link-prediction model (Link_prediction_model/model.py:37-169: a trainable node embedding, `--encoder SAGE | MLP` of
`--gnn_num_layers` layers and `--gnn_hidden_channels` width, `--predictor DOT | MLP | BIL | MLPDOT | MLPBIL | MLPCAT`, `--loss_func AUC | ce_loss | log_rank_loss | info_nce_loss`,
`--num_neg`, `--batch_size`, `--grad_clip_norm`) on the HIP path (trainer.train_linkpred_encoder; main.py does not route there):
    python tools/train_linkpred_encoder.py --dataset=S-tiny --encoder=SAGE --predictor=MLP --loss_func=log_rank_loss --num_neg=3 --epochs=20
Every step runs the encoder over the whole graph (one fused aggregation + GEMM kernel per 256 -> 256 layer where tuning.T.sage_fused is on, the
composed kernels otherwise) and scores --batch_size sampled positives and --num_neg negatives each through predictor.score_pairs.  WSAGE / GCN encoders
are reachable from Python (Link_prediction_model.create_encoder_layer).  --encoder=TRANSFORMER trains the TransformerEncoder (one stacked GEMM and one
attention kernel over the CSR rows per layer, ops.transformer_conv); the package's --encoder choices are the reference's, so this tool takes that value
off the command line before the package's options are parsed and sets args.encoder afterwards.  Loops over --N_exp seeds like main.py; returns / prints
per seed (losses [epochs], {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} of a test-mode sample); the trainer of the last seed is kept as main.last_trainer."""
import argparse
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import main as cb_main  # noqa: E402
from gnn_tail_generalization_amd.base_options import BaseOptions  # noqa: E402


def main(argv=None):
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument('--encoder', type=str, default=None)
    mine, rest = own.parse_known_args(list(sys.argv[1:] if argv is None else argv))
    transformer = mine.encoder is not None and mine.encoder.upper() == 'TRANSFORMER'
    if mine.encoder is not None and not transformer:
        rest = rest + [f'--encoder={mine.encoder}']
    args = BaseOptions().get_arguments(rest)
    if transformer:
        args.encoder = 'TRANSFORMER'
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    recs = []
    main.last_trainer = None
    for seed in range(args.N_exp):
        print(f'seed (which_run) = <{seed}>')
        args.random_seed = seed
        cb_main.set_seed(args)
        trnr = trainer(args, seed)
        losses, metrics = trnr.train_linkpred_encoder()
        print(f'link prediction ({args.encoder} encoder, {args.predictor}, {args.loss_func}, num_neg {args.num_neg}): loss first / last epoch '
              f'{losses[0]:.5f} / {losses[-1]:.5f}; ' + ', '.join(f'{k} {v:.4f}' for k, v in metrics.items()))
        recs.append((losses, metrics))
        main.last_trainer = trnr
        del trnr
        torch.cuda.empty_cache()
        gc.collect()
    return recs


if __name__ == '__main__':
    main()
