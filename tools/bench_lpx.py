"""Times the link-prediction experiment's device pieces (csrc/cb_lpx.hip) on one MI355X against their compositions from torch's own device operators.
Medians of alternating repeats (HIP, torch, HIP, torch, ...) after two warm-up runs of each; every timing ends in a synchronise (device events, or a
host clock around work that ends in a host read).  No speed threshold is fixed in advance: the table records what was measured, also where the HIP
form loses.
  (a) ops.NegativeSampler.global_ for 3 E pairs against ONE round of PyG's `negative_sampling` algorithm over the same number of draws:
      randint, linearise (v N + u), searchsorted in the sorted key list of the edges, compare.  PyG linearises and sorts the edge list on every call;
      both forms are timed, with the per-call sort and with the sorted list prebuilt.  The torch form keeps its rejected draws as holes (PyG then
      draws again); the HIP form retries inside the kernel and fills every slot.  "search bytes": counted by this tool from the output — per slot the
      two row pointers (8 B) and ceil(log2(deg(v) + 1)) column probes of 4 B in the accepted row, plus the 8 B written; rejected tries (rare: a
      uniform pair is almost never an edge) are not counted.
  (b) ops.row_rank_counts at P x K and ops.recall_at_topk's numerator over P positives and P K negatives (k = 1.25 P) against torch: broadcast compare +
      sum, and concatenate + stable descending sort + gather + sum.
  (c) one LinkPredictionModel.train epoch and one .test of SAGE + MLP at batch_size 65 536 (host clock; the epoch ends in its one host read), and the
      share of the epoch spent drawing the negatives and the shuffle (timed on their own with device events).  Datasets of (c): --epoch_datasets
      (an S-products epoch is ~1900 full-graph steps and is left out by default).
    usage: python tools/bench_lpx.py [--datasets S-arxiv S-products] [--epoch_datasets S-arxiv] [--repeats 7] [--out profiles/lpx.md]"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import CSRGraph  # noqa: E402

HBM_BYTES_PER_S = 8e12
PLUMBING = ['--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1']


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, repeats):
    """Median (min .. max) ms of each fn: two warm-up runs of each, then `repeats` rounds that run them one after the other."""
    for fn in fns:
        fn()
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def fmt(t):
    return f'{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--epoch_datasets', nargs='*', default=['S-arxiv'])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--rank_p', type=int, default=100000)
    ap.add_argument('--rank_k', type=int, default=1000)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev = 'cuda:0'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    say('# Negative samplers, shuffle and ranking metrics of the link-prediction experiment (`tools/bench_lpx.py`)\n')
    say(f'One MI355X, one process.  Medians (min .. max) of {a.repeats} alternating repeats after two warm-up runs of each form; device events around the '
        'operator calls (launches and the operator\'s allocations included), a host clock around the epoch and the test.  HIP / torch below 1: the HIP form is faster.\n')

    # ---- (a) global negatives ----
    say('## (a) `NegativeSampler.global_`, S = 3 E slots\n')
    say('| graph | HIP, ms | torch one round, sort per call (PyG), ms | torch one round, sorted list prebuilt, ms | HIP / torch (PyG) | HIP / torch (prebuilt) | '
        'slots / s (HIP) | search bytes (tool count) | share of 8 TB/s | failed slots | holes left by the torch round |')
    say('|---|---|---|---|---|---|---|---|---|---|---|')
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n, ei = int(data.x.shape[0]), data.edge_index.long()
        E = int(ei.shape[1])
        graph = CSRGraph(ei, n)
        sampler = ops.NegativeSampler(graph)
        S = 3 * E
        gen = torch.Generator(device=dev).manual_seed(1)
        prebuilt = torch.sort(ei[1] * n + ei[0]).values
        holes = [0]

        def torch_round(idx=None):
            idx = torch.sort(ei[1] * n + ei[0]).values if idx is None else idx
            u = torch.randint(0, n, (S,), device=dev, generator=gen)
            v = torch.randint(0, n, (S,), device=dev, generator=gen)
            key = v * n + u
            at = torch.searchsorted(idx, key).clamp_(max=E - 1)
            ok = (idx[at] != key) & (u != v)
            holes[0] = ok
            return u, v, ok
        th, tp, tb = alternate([lambda: sampler.global_(E, 3, seed=7), torch_round, lambda: torch_round(prebuilt)], a.repeats)
        out = sampler.global_(E, 3, seed=7)
        failed = int(sampler.failed.item())
        sampler.failed.zero_()
        deg = (graph.rowptr[1:] - graph.rowptr[:-1]).to(torch.float64)
        probes = torch.ceil(torch.log2(deg + 1))[out[1].long().clamp_(min=0)]
        search_bytes = int((8 + 4 * probes).sum().item()) + 8 * S
        n_holes = S - int(holes[0].sum().item())
        say(f'| {name}: N = {n}, E = {E} | {fmt(th)} | {fmt(tp)} | {fmt(tb)} | {th[0] / tp[0]:.2f} | {th[0] / tb[0]:.2f} | {S / (th[0] * 1e-3):.3g} | '
            f'{search_bytes / 1e9:.2f} GB | {search_bytes / (th[0] * 1e-3) / HBM_BYTES_PER_S * 100:.1f} % | {failed} | {n_holes} of {S} |')
        # the shuffle, for scale
        tperm, trand = alternate([lambda: ops.seeded_permutation(E, 3, device=dev), lambda: torch.randperm(E, device=dev)], a.repeats)
        say(f'| {name}: `seeded_permutation(E)` against `torch.randperm(E)` on the device | {fmt(tperm)} | {fmt(trand)} | | {tperm[0] / trand[0]:.2f} | | {E / (tperm[0] * 1e-3):.3g} | | | | |')
        del data, graph, sampler, ei, prebuilt, out, probes, deg
        holes[0] = None
        torch.cuda.empty_cache()

    # ---- (b) ranks and recall ----
    P, K = a.rank_p, a.rank_k
    say(f'\n## (b) `row_rank_counts` and `recall_at_topk`, P = {P}, K = {K} (P K = {P * K} negatives), k = 1.25 P\n')
    say('| operator | scores | HIP, ms | torch, ms | HIP / torch | algorithmic bytes over HIP time, share of 8 TB/s | results equal |')
    say('|---|---|---|---|---|---|---|')
    g = torch.Generator(device=dev).manual_seed(3)
    for label, pos, neg in (('real-valued', torch.randn(P, device=dev, generator=g), torch.randn((P, K), device=dev, generator=g)),
                            ('integers 0..15 (heavy ties)', torch.randint(0, 16, (P,), device=dev, generator=g).float(),
                             torch.randint(0, 16, (P, K), device=dev, generator=g).float())):
        def torch_rows():
            p = pos.reshape(-1, 1)
            return (neg > p).sum(1, dtype=torch.int32), (neg == p).sum(1, dtype=torch.int32)
        th, tt = alternate([lambda: ops.row_rank_counts(pos, neg), torch_rows], a.repeats)
        same = all(torch.equal(x, y) for x, y in zip(ops.row_rank_counts(pos, neg), torch_rows()))
        by = 4 * P * K + 12 * P
        say(f'| row_rank_counts | {label} | {fmt(th)} | {fmt(tt)} | {th[0] / tt[0]:.2f} | {by / (th[0] * 1e-3) / HBM_BYTES_PER_S * 100:.1f} % ({by / 1e6:.0f} MB) | {same} |')
        k = int(1.25 * P)
        flat = neg.reshape(-1)

        def torch_recall():
            kept = pos[pos > 0]
            scores = torch.cat([kept, flat])
            order = torch.sort(scores, descending=True, stable=True).indices[:k]
            return (order < kept.numel()).sum()
        th, tt = alternate([lambda: ops.recall_numerator(pos, flat, k), torch_recall], a.repeats)
        same = int(ops.recall_numerator(pos, flat, k)[0].item()) == int(torch_recall().item())
        by = 4 * (P + P * K) + 5 * 3 * 8 * (P + P * K)      # the scores once, then five radix passes of two reads and a write of 8 B keys
        say(f'| recall numerator | {label} | {fmt(th)} | {fmt(tt)} | {th[0] / tt[0]:.2f} | {by / (th[0] * 1e-3) / HBM_BYTES_PER_S * 100:.1f} % ({by / 1e6:.0f} MB) | {same} |')
    del pos, neg, flat
    torch.cuda.empty_cache()

    # ---- (c) an epoch and a test ----
    if a.epoch_datasets:
        import main as cb_main
        from gnn_tail_generalization_amd.base_options import BaseOptions
        from gnn_tail_generalization_amd.Link_prediction_model.experiment import LinkPredictionModel
        from gnn_tail_generalization_amd.trainer_link_prediction import trainer
        say('\n## (c) one `train` epoch and one `test`, SAGE (2 x 256) + MLP, log_rank_loss, num_neg 3, batch_size 65 536\n')
        say('| graph | train positives | steps | epoch, s: median (min .. max) | negatives for the epoch (`global`), ms | shuffle, ms | sampler + shuffle share of the epoch | test (recall_my@1.25), s |')
        say('|---|---|---|---|---|---|---|---|')
        for name in a.epoch_datasets:
            with contextlib.redirect_stdout(io.StringIO()):
                args = BaseOptions().get_arguments([f'--dataset={name}', '--encoder=SAGE', '--predictor=MLP', '--loss_func=log_rank_loss', '--num_neg=3',
                                                    '--batch_size=65536', '--random_seed=0'] + PLUMBING)
                args.edge_lp_mode = ''
                cb_main.set_seed(args)
                t = trainer(args, 0)
                split = t.make_split_edge()
                model = LinkPredictionModel(args, t.data, t.device)
                model.param_init()
            Ptr = int(split['train']['edge'].shape[0])

            def clock(fn, reps):
                fn()
                out = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    out.append(time.perf_counter() - t0)
                return statistics.median(out), min(out), max(out)
            ep = clock(lambda: model.train(t.data, split, args.batch_size, 'global', 3), 3)
            steps = model.steps // 4
            te = clock(lambda: model.test(t.data, split, args.batch_size, None, 'recall_my@1.25'), 3)
            ts, tp = alternate([lambda: model.sampler.global_(Ptr, 3), lambda: ops.seeded_permutation(Ptr, device=dev)], a.repeats)
            model.sampler.check()
            say(f'| {name} | {Ptr} | {steps} | {fmt(ep)} | {fmt(ts)} | {fmt(tp)} | {(ts[0] + tp[0]) * 1e-3 / ep[0] * 100:.2f} % | {fmt(te)} |')
            del t, split, model
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
