"""Times the BIL / MLPDOT / MLPBIL / MLPCAT link predictors (Link_prediction_model/pair_predictor.py): predictor.score_pairs(h, pairs) — the fused
route through ops.rows_linear / ops.pair_bilinear / ops.pair_dot / ops.pair_scatter_rows, csrc/cb_pairpred.hip — against
predictor.forward(h[u], h[v]) on rows torch gathers, which runs only the operators that existed before these kernels (gemm.linear, ops.dropout,
torch elementwise, torch's index backward).  Layout of tools/bench_linkpred.py: S = 262 144 pairs (65 536 positives + 3 negatives each),
D = hidden = 256, two layers, dropout 0, N of S-arxiv; uniform pairs and the hub batch (pairs skewed towards few nodes: long runs in the scatter).
  train    forward alone (under torch.no_grad()) and forward + backward, training mode, per-pair route
  eval     the per-node route against the per-pair route at S = 4 N, forward under torch.no_grad()
  time     warm-up twice, then the median of --repeats runs (default five) timed with device events, launches and the operators' Python included;
           one process on the device
  memory   torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it
  work     next to each predictor, the GEMM flops (2 M N K per product, one pass; the three-limb kernel issues six bf16 passes for it) and the
           algorithmic bytes (operands and results read or written once) of the fused forward
No speed threshold is fixed in advance: the table records what was measured, also where the fused route loses.
    usage: python tools/bench_pairpred.py [--nodes 169343] [--pairs 262144] [--dim 256] [--repeats 5] [--out profiles/pairpred_times.md]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_linkpred import measure  # noqa: E402
from gnn_tail_generalization_amd import ops, tuning  # noqa: E402
from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp  # noqa: E402


def work(kind, S, D, L):
    """(GEMM flops, algorithmic bytes) of the fused forward at hidden = D: rows read once from h, activations written and read once between layers,
    weights left out."""
    f4 = 4
    if kind == 'BIL':
        return 2 * S * D * D, 2 * S * D * f4 + S * f4
    if kind == 'MLPCAT':      # 2 S rows of width 2 D into D, L - 2 layers D -> D, the last D -> 1
        flops = 2 * (2 * S) * (2 * D) * D + (L - 2) * 2 * (2 * S) * D * D + 2 * (2 * S) * D
        return flops, (2 * S) * (2 * D) * f4 + (L - 1) * 2 * (2 * S) * D * f4 + 2 * S * f4
    flops = L * 2 * (2 * S) * D * D + (2 * S * D * D if kind == 'MLPBIL' else 0)
    return flops, (2 * S) * D * f4 + (2 * L - 1) * (2 * S) * D * f4 + 2 * S * D * f4 + S * f4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=169343)
    ap.add_argument('--pairs', type=int, default=262144)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--layers', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
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
    N, S, D, L = a.nodes, a.pairs, a.dim, a.layers
    say(f'One MI355X, one process; medians of {a.repeats} runs after two warm-up runs, device events, launches and Python included; N = {N} nodes, '
        f'S = {S} pairs, D = hidden = {D}, {L} layers, dropout 0.  fused: predictor.score_pairs on the per-pair route; composed: predictor.forward on '
        f'gathered rows.  Peak: extra device memory over one forward + backward.\n')
    say('| pairs | predictor | GEMM GFLOP, fused forward | algorithmic MB, fused forward | forward fused, ms: median (min .. max) | forward composed, ms | fused / composed | '
        'forward + backward fused, ms | forward + backward composed, ms | fused / composed | fused peak, MiB | composed peak, MiB | max abs difference of the scores | of dH |')
    say('|---|---|---|---|---|---|---|---|---|---|---|---|---|---|')
    gen = torch.Generator(device=dev).manual_seed(1)
    h = (torch.randn(N, D, device=dev, generator=gen) * 0.1).requires_grad_(True)
    uniform = torch.randint(0, N, (2, S), device=dev, generator=gen)
    skewed = (torch.rand(2, S, device=dev, generator=gen) ** 6 * N).long().clamp_(0, N - 1)

    def make(kind):
        torch.manual_seed(0)
        return {'BIL': lambda: pp.BilinearPairPredictor(D), 'MLPDOT': lambda: pp.MLPDotPairPredictor(D, D, L, 0.0),
                'MLPBIL': lambda: pp.MLPBilPairPredictor(D, D, L, 0.0), 'MLPCAT': lambda: pp.MLPCatPairPredictor(D, D, 1, L, 0.0)}[kind]().to(dev)
    tuning.T.score_pairs_fused, tuning.T.pair_predictor_per_node = True, False
    for pop, pairs in (('uniform', uniform), ('hub batch', skewed)):
        for kind in ('BIL', 'MLPDOT', 'MLPBIL', 'MLPCAT'):
            pred = make(kind).train()

            def fwd_fused():
                with torch.no_grad():
                    pred.score_pairs(h, pairs)

            def fwd_composed():
                with torch.no_grad():
                    pred(h[pairs[0]], h[pairs[1]])

            def fused():
                h.grad = None
                pred.score_pairs(h, pairs).sum().backward()

            def composed():
                h.grad = None
                pred(h[pairs[0]], h[pairs[1]]).sum().backward()
            ff, fc = measure(fwd_fused, a.repeats), measure(fwd_composed, a.repeats)
            tf, tc = measure(fused, a.repeats), measure(composed, a.repeats)
            fused()
            gf = h.grad.clone()
            composed()
            gc = h.grad.clone()
            with torch.no_grad():
                ds = float((pred.score_pairs(h, pairs) - pred(h[pairs[0]], h[pairs[1]])).abs().max())
            ops.pair_check()
            fl, by = work(kind, S, D, L)
            say(f'| {pop} | {kind} | {fl / 1e9:.1f} | {by / 1e6:.0f} | {ff[0]:.3f} ({ff[1]:.3f} .. {ff[2]:.3f}) | {fc[0]:.3f} ({fc[1]:.3f} .. {fc[2]:.3f}) | {ff[0] / fc[0]:.2f} | '
                f'{tf[0]:.3f} ({tf[1]:.3f} .. {tf[2]:.3f}) | {tc[0]:.3f} ({tc[1]:.3f} .. {tc[2]:.3f}) | {tf[0] / tc[0]:.2f} | {tf[3]:.0f} | {tc[3]:.0f} | {ds:.3g} | '
                f'{float((gf - gc).abs().max()):.3g} |')
            del gf, gc, pred
    S4 = 4 * N
    say(f'\nEval mode, forward under torch.no_grad(), S = 4 N = {S4} uniform pairs: the per-node route (the stack on the N rows of h once) against the per-pair '
        f'route (on the 2 S endpoint rows); BIL has no stack and is left out.\n')
    say('| predictor | per-node, ms: median (min .. max) | per-pair, ms | per-node / per-pair | same bits |')
    say('|---|---|---|---|---|')
    pairs4 = torch.randint(0, N, (2, S4), device=dev, generator=gen)
    for kind in ('MLPDOT', 'MLPBIL'):
        pred = make(kind).eval()
        res = {}
        for route in (True, False):
            tuning.T.pair_predictor_per_node = route

            def run():
                with torch.no_grad():
                    return pred.score_pairs(h, pairs4)
            res[route] = (measure(run, a.repeats), run())
        ops.pair_check()
        tn, tp = res[True][0], res[False][0]
        say(f'| {kind} | {tn[0]:.3f} ({tn[1]:.3f} .. {tn[2]:.3f}) | {tp[0]:.3f} ({tp[1]:.3f} .. {tp[2]:.3f}) | {tn[0] / tp[0]:.2f} | {torch.equal(res[True][1], res[False][1])} |')
    tuning.T.pair_predictor_per_node = None


if __name__ == '__main__':
    main()
