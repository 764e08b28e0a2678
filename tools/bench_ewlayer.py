"""Times one 256 -> 256 WSAGE / GCN layer over an adjacency WITH VALUES (graph.WeightedAdj; ops.sage_layer_raw, csrc/cb_ewlayer.hip) as ONE kernel,
on the synthetic S-arxiv and S-products graphs at D = 256, per direction, against
  before      how the same layer was computed before the weighted kernels existed: graph.spmm_weighted (one wavefront per row, no hub handling) into the
              materialised [agg | x], gemm.mm_nn with K = 512 (256 for GCN), ops.dropout's kernel;
  composed    the composed path of today: WeightedAdj.spmm_ew (the tuned aggregation with per-edge values) + the same GEMM + dropout;
  unweighted  the one-kernel layer WITHOUT values on the same graph (cb_sage_layer_f32, no scale): the algorithmic difference is 4 bytes per edge next to a
              1 KiB gathered row;
  noise       the unweighted layer against itself, timed the same way: the run-to-run spread a difference has to exceed.
  time     warm-up twice, then the median (min - max) of --repeats runs timed with device events on the launching stream, launches, weight images and the
           operators' Python included; one process on the device; the two sides of a pair alternate, so drift hits both alike
  forward  sage_layer_raw(relu, dropout 0.5);  backward  sage_layer_raw(backward=True, want_agg=True): G -> (dX, R)
Before anything is timed the fused result is checked equal (torch.equal) to the composed one and close to `before` (whose hub rows are summed in another
order).  No ratio is promised: the table records what was measured.
    usage: python tools/bench_ewlayer.py [--datasets S-arxiv S-products] [--modes WSAGE GCN] [--repeats 7] [--out profiles/ewlayer_times.md]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_sage import fmt, measure_pair  # noqa: E402
from gnn_tail_generalization_amd import gemm, ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import WeightedAdj  # noqa: E402


def before(adj, h, W_n, W_s, bias, relu, p, seed, backward):
    """(out, agg): the layer as graph.spmm_weighted + the materialised [agg | h] + gemm.mm_nn + ops.dropout."""
    G = adj.graph
    agg = G.spmm_weighted(h, adj.val_t if backward else adj.val, transpose=backward)
    if W_s is not None:
        cat = torch.cat([agg, h], dim=1)
        B = torch.cat([W_n, W_s]) if backward else torch.cat([W_n.t(), W_s.t()])
    else:
        cat, B = agg, (W_n if backward else W_n.t())
    y = gemm.mm_nn(cat, B.contiguous(), bias=bias, relu=relu)
    return (ops.dropout(y, p, seed=seed) if p else y), agg


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--modes', nargs='+', default=['WSAGE', 'GCN'])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev = 'cuda:0'
    lines = ['| graph | nodes | edges | hubs fwd / bwd | mode | what | fused ms | before ms | composed ms | unweighted fused ms | unweighted again ms '
             '| fused / before | fused / unweighted | unweighted / again |', '|' + '---|' * 14]
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n = int(data.x.shape[0])
        g = torch.Generator(device=dev).manual_seed(1)
        adj = WeightedAdj.from_edges(data.edge_index, torch.rand(data.edge_index.shape[1], device=dev, generator=g) + 0.5, n)
        G = adj.graph
        del data
        x = torch.randn(n, 256, device=dev, generator=g)
        dy = torch.randn(n, 256, device=dev, generator=g)
        W_n, W_s = torch.randn(256, 256, device=dev, generator=g) / 16, torch.randn(256, 256, device=dev, generator=g) / 16
        b = torch.randn(256, device=dev, generator=g)
        head = f'| {name} | {n} | {G.E} | {G._plan.n_hubs} / {G._plan_t.n_hubs} '
        for mode in a.modes:
            Ws = None if mode == 'GCN' else W_s
            fwd = lambda graph, fused: ops.sage_layer_raw(graph, x, W_n, Ws, b, None, relu=True, p=0.5, seed=7, fused=fused)                    # noqa: E731
            bwd = lambda graph, fused: ops.sage_layer_raw(graph, dy, W_n, Ws, None, None, backward=True, want_agg=True, fused=fused)            # noqa: E731
            old_fwd = lambda: before(adj, x, W_n, Ws, b, True, 0.5, 7, False)                                                                   # noqa: E731
            old_bwd = lambda: before(adj, dy, W_n, Ws, None, False, 0.0, 0, True)                                                               # noqa: E731
            for what, fn, old in (('forward', fwd, old_fwd), ('backward', bwd, old_bwd)):
                rf, rc, ro = fn(adj, True), fn(adj, False), old()
                assert (rf[2], rc[2]) == ('fused', 'composed') and torch.equal(rf[0], rc[0]) and (rf[1] is None or torch.equal(rf[1], rc[1])), (name, mode, what)
                if what == 'backward':      # (the forward's dropout makes a last-bit difference at the ReLU's edge a whole element)
                    for got, ref in ((rf[0], ro[0]), (rf[1], ro[1])):      # another summation order on hub rows: last bits of long fp32 sums
                        assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), (name, mode, what)
                del rf, rc, ro
                tf, to = measure_pair(lambda: fn(adj, True), old, a.repeats)
                tf2, tc = measure_pair(lambda: fn(adj, True), lambda: fn(adj, False), a.repeats)
                tf3, tu = measure_pair(lambda: fn(adj, True), lambda: fn(G, True), a.repeats)
                tu1, tu2 = measure_pair(lambda: fn(G, True), lambda: fn(G, True), a.repeats)
                lines.append(head + f'| {mode} | layer {what} | {fmt(tf)} | {fmt(to)} | {fmt(tc)} | {fmt(tu)} | {fmt(tu2)} | {tf[0] / to[0]:.3f} | '
                             f'{tf3[0] / tu[0]:.3f} | {tu1[0] / tu2[0]:.3f} |')
                print(lines[-1], flush=True)
        del adj, G, x, dy
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    return text


if __name__ == '__main__':
    main()
