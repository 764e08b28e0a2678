"""Times forward + backward of the link predictors' fused path (predictor.score_pairs: ops.pair_linear / ops.pair_dot, csrc/cb_linkpred.hip) against
the composed path — torch gathers h[u], h[v], their product, the existing GEMM operators, and torch's index backward for the scatter
(predictor.forward(h[u], h[v])) — at S = 262 144 pairs (--batch_size 65536 positives + --num_neg 3 negatives each) and D = 256 on the node counts
of S-arxiv and S-products, for uniform pairs and for pairs skewed towards few nodes (long runs in the scatter).  Then the five ranking losses
(ops.rank_loss, float64 inside) against the reference's formulas composed from torch operators in fp32, at P = 65 536, k = 3.
  time     warm-up twice, then the median of --repeats runs (default five) of forward + backward timed with device events, launches and the
           operators' Python included; one process on the device
  memory   torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it
No speed threshold is fixed in advance: the table records what was measured, also where the fused path loses.
    usage: python tools/bench_linkpred.py [--nodes S-arxiv S-products] [--pairs 262144] [--dim 256] [--repeats 5] [--out profiles/linkpred_times.md]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops, tuning  # noqa: E402
from gnn_tail_generalization_amd.Link_prediction_model import DotPredictor, MLPPredictor  # noqa: E402

NODES = {'S-arxiv': 169343, 'S-products': 2449029}
KINDS = ('auc_loss', 'adaptive_auc_loss', 'log_rank_loss', 'ce_loss', 'info_nce_loss')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, repeats):
    fn()
    fn()
    torch.cuda.synchronize()
    t = [timed(fn) for _ in range(repeats)]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return statistics.median(t), min(t), max(t), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def torch_loss(kind, pos, neg, k, w):
    """loss.py as written, on the device in fp32."""
    p, n = pos.reshape(-1, 1), neg.reshape(-1, k)
    if kind == 'auc_loss':
        return torch.square(1 - (p - n)).sum()
    if kind == 'adaptive_auc_loss':
        return (w.reshape(-1, 1) * torch.square(1 - (p - n))).sum()
    if kind == 'log_rank_loss':
        return -torch.log(torch.sigmoid(p - n) + 1e-15).mean()
    if kind == 'ce_loss':
        return -torch.log(torch.sigmoid(pos) + 1e-15).mean() + -torch.log(1 - torch.sigmoid(neg) + 1e-15).mean()
    pe = torch.exp(p)
    return -torch.log(pe / (pe + torch.sum(torch.exp(n), 1, keepdim=True)) + 1e-15).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', nargs='+', default=list(NODES))
    ap.add_argument('--pairs', type=int, default=262144)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev = 'cuda:0'
    tuning.T.score_pairs_fused = True      # (score_pairs below is the fused path whatever the default)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    S, D = a.pairs, a.dim
    say(f'One MI355X, one process; forward + backward, medians of {a.repeats} runs after two warm-up runs, device events, launches and Python included; '
        f'S = {S} pairs, D = {D}.  Peak: extra device memory over one forward + backward.\n')
    say('| nodes | pairs | predictor | fused, ms: median (min .. max) | composed, ms | fused / composed | fused peak, MiB | composed peak, MiB | max abs difference of the scores | of dH |')
    say('|---|---|---|---|---|---|---|---|---|---|')
    gen = torch.Generator(device=dev).manual_seed(1)
    for name in a.nodes:
        N = NODES[name]
        h = (torch.randn(N, D, device=dev, generator=gen) * 0.1).requires_grad_(True)
        uniform = torch.randint(0, N, (2, S), device=dev, generator=gen)
        skewed = (torch.rand(2, S, device=dev, generator=gen) ** 6 * N).long().clamp_(0, N - 1)
        for pop, pairs in (('uniform', uniform), ('skewed', skewed)):
            torch.manual_seed(0)
            for pname, pred in (('MLP, 2 layers, dropout 0', MLPPredictor(D, D, 1, 2, 0.0).to(dev).train()), ('DOT', DotPredictor().to(dev))):
                def fused():
                    h.grad = None
                    pred.score_pairs(h, pairs).sum().backward()

                def composed():
                    h.grad = None
                    pred(h[pairs[0]], h[pairs[1]]).sum().backward()
                tf, tc = measure(fused, a.repeats), measure(composed, a.repeats)
                fused()
                gf = h.grad.clone()
                composed()
                gc = h.grad.clone()
                with torch.no_grad():
                    ds = float((pred.score_pairs(h, pairs) - pred(h[pairs[0]], h[pairs[1]])).abs().max())
                ops.pair_check()
                say(f'| {name} ({N}) | {pop} | {pname} | {tf[0]:.3f} ({tf[1]:.3f} .. {tf[2]:.3f}) | {tc[0]:.3f} ({tc[1]:.3f} .. {tc[2]:.3f}) | {tf[0] / tc[0]:.2f} | '
                    f'{tf[3]:.0f} | {tc[3]:.0f} | {ds:.3g} | {float((gf - gc).abs().max()):.3g} |')
                del gf, gc
        del h, uniform, skewed
        torch.cuda.empty_cache()
    P, k = 65536, 3
    say(f'\nRanking losses, P = {P}, k = {k}, scores uniform in [-3, 3], forward + backward:\n')
    say('| loss | ops.rank_loss (float64 inside), ms: median (min .. max) | torch composition in fp32, ms | HIP / torch | relative difference of the values |')
    say('|---|---|---|---|---|')
    pos = (torch.rand(P, device=dev, generator=gen) * 6 - 3).requires_grad_(True)
    neg = (torch.rand(P * k, device=dev, generator=gen) * 6 - 3).requires_grad_(True)
    w = torch.rand(P, device=dev, generator=gen) + 0.5
    for kind in KINDS:
        def hip():
            pos.grad = neg.grad = None
            ops.rank_loss(kind, pos, neg, k, w if kind == 'adaptive_auc_loss' else None).backward()

        def composed():
            pos.grad = neg.grad = None
            torch_loss(kind, pos, neg, k, w).backward()
        th, tt = measure(hip, a.repeats), measure(composed, a.repeats)
        with torch.no_grad():
            lv, tv = float(ops.rank_loss(kind, pos, neg, k, w if kind == 'adaptive_auc_loss' else None)), float(torch_loss(kind, pos, neg, k, w))
        say(f'| {kind} | {th[0]:.3f} ({th[1]:.3f} .. {th[2]:.3f}) | {tt[0]:.3f} ({tt[1]:.3f} .. {tt[2]:.3f}) | {th[0] / tt[0]:.2f} | {abs(lv - tv) / abs(tv):.2e} |')


if __name__ == '__main__':
    main()
