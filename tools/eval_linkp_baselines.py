"""Prints the link-prediction baselines a learned scorer's MRR / Hits@K is held against: one line per heuristic (CN = common neighbours,
AA = Adamic-Adar; Link_prediction_baseline/heuristics.py:107-129) with Hits@20 / Hits@50 / Hits@100 and the AUC on a fresh test-mode sample of
--samp_size_p positive edges and --samp_size_p * --neg_per_pos negative pairs (ops.LinkSampler), every positive ranked against all negatives:
    python tools/eval_linkp_baselines.py --dataset=S-tiny [--kinds CN AA] [--samp_size_p 200] [--neg_per_pos 20]
The graph is scored AS GIVEN: the sampled positives are edges of the very graph whose neighbourhoods are intersected, so the numbers are those of
a graph that contains its test edges.  Holding edges out of the graph before scoring — what an OGB-style split does — is the caller's job
(ops.pair_scores takes any whole square graph.CSRGraph).  --kinds and --neg_per_pos are this tool's own flags, taken off the command line
before the package's options are parsed; 'PPR' is not built (it needs the fast_pagerank package).  Returns [(kind, {metric: value})]."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import main as cb_main  # noqa: E402
from gnn_tail_generalization_amd.base_options import BaseOptions  # noqa: E402


def main(argv=None):
    own = argparse.ArgumentParser(add_help=False)
    own.add_argument('--kinds', nargs='+', default=['CN', 'AA'])
    own.add_argument('--neg_per_pos', type=int, default=None)
    mine, rest = own.parse_known_args(list(sys.argv[1:] if argv is None else argv))
    for kind in mine.kinds:
        if kind not in ('CN', 'AA'):
            raise SystemExit(f"tools/eval_linkp_baselines.py: --kinds takes CN and AA, got {kind!r} ('PPR' is not built: it needs fast_pagerank)")
    args = BaseOptions().get_arguments(rest)
    if mine.neg_per_pos is not None:
        args.samp_size_n_test_times_p = mine.neg_per_pos
    args.has_loss_component_edgewise = True
    args.random_seed = 0
    cb_main.set_seed(args)
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    trnr = trainer(args, 0)
    rows = []
    n_pos, n_neg = args.samp_size_p, args.samp_size_p * args.samp_size_n_test_times_p
    print(f'{args.dataset}: test-mode sample of {n_pos} positive edges and {n_neg + (n_neg & 1)} negative pairs; the graph is scored as given')
    for kind in mine.kinds:
        res = trnr.evaluate_linkp_heuristic(kind, 'test')
        print(f'{kind}  ' + '  '.join(f'{k} {res[k]:.4f}' for k in ('Hits@20', 'Hits@50', 'Hits@100', 'AUC')))
        rows.append((kind, res))
    return rows


if __name__ == '__main__':
    main()
