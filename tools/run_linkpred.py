"""Runs the reference's link-prediction experiment (trainer_link_prediction.py driving Link_prediction_model/model.py's BaseModel.train / test) on
the HIP path (gnn_tail_generalization_amd.trainer_link_prediction; main.py does not route there):
    python tools/run_linkpred.py --dataset=S-tiny --encoder=SAGE --predictor=MLP --loss_func=log_rank_loss --neg_sampler=global --num_neg=3 \
        --eval_metric=recall_my@1.25 --epochs=10 --eval_steps=5 --runs=2 --batch_size=4096
An epoch draws `--num_neg` negatives for every train positive with `--neg_sampler global | local | <anything else: permuted global copies>`, shuffles
the positives with a seeded device permutation and takes `--batch_size` of them per optimizer step; every `--eval_steps` epochs the train / valid /
test edges are scored and `--eval_metric hits | mrr | recall_my@<k>` is reported; `--runs` runs, per-run and all-runs statistics at the end
(`--eval_last_best`).  The edge split comes from utils.split_edges under --random_seed: target nodes are those outside the train mask, or, with
--exp_on_cold_edge, target edges those between low-degree endpoints.
Three values are taken off the command line before the package's options are parsed, because base_options pins the reference's choices:
`--encoder=TRANSFORMER | GCN | WSAGE` (encoders that are built but not among base_options' choices); `--edge_lp_mode`, whose default here is '' — base_options' default 'logit' names edge_LP.py,
which is not built; any other value raises NotImplementedError; and `--normalize_adj` (default 0): 1 applies the reference's gcn_normalization for
`--encoder GCN` and adj_normalization for `--encoder WSAGE` (trainer_link_prediction.py:333-338; the reference does so unconditionally, here the
default stays the adjacency as given), other encoders are unaffected.  `--encoder CN | AA` score with the common-neighbour heuristics and train
nothing (loss -1.0); `PPR` raises.
Real-valued edge weights: a dataset that carries `data.edge_weight` (one float per column of edge_index) has the GCN / WSAGE layers multiply by them —
as given, or normalised under `--normalize_adj=1`; SAGE, TRANSFORMER and MLP ignore them.  The per-edge margins split_edge['train']['weight'] stay refused.
main(argv, split_edge=None) returns the trainer (losses [runs][epochs], results [runs][evaluations], loggers) — a given split_edge (either form of
Link_prediction_model.utils.get_pos_neg_edges) is used instead of utils.split_edges."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import main as cb_main  # noqa: E402
from gnn_tail_generalization_amd.base_options import BaseOptions  # noqa: E402

BEYOND_BASE_OPTIONS = ('TRANSFORMER', 'GCN', 'WSAGE')      # encoders that are built but that base_options' --encoder choices do not name


def parse_args(argv=None):
    """The package's options with this tool's own three on top (--encoder beyond base_options' choices, --edge_lp_mode, --normalize_adj)."""
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument('--encoder', type=str, default=None)
    own.add_argument('--edge_lp_mode', type=str, default='')
    own.add_argument('--normalize_adj', type=int, default=0)
    mine, rest = own.parse_known_args(list(sys.argv[1:] if argv is None else argv))
    beyond = mine.encoder is not None and mine.encoder.upper() in BEYOND_BASE_OPTIONS
    if mine.encoder is not None and not beyond:
        rest = rest + [f'--encoder={mine.encoder}']
    args = BaseOptions().get_arguments(rest)
    if beyond:
        args.encoder = mine.encoder.upper()
    args.edge_lp_mode = mine.edge_lp_mode
    args.normalize_adj = mine.normalize_adj
    return args


def main(argv=None, split_edge=None):
    args = parse_args(argv)
    from gnn_tail_generalization_amd.trainer_link_prediction import trainer
    cb_main.set_seed(args)
    trnr = trainer(args, 0)
    trnr.split_edge = split_edge
    trnr.main()
    return trnr


if __name__ == '__main__':
    main()
