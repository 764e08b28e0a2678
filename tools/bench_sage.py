"""Times one 256 -> 256 layer of the SAGE / WSAGE / GCN encoders (ops.sage_layer, csrc/cb_sage.hip) as ONE kernel against the composed path —
graph.spmm, the materialised [agg | x], one cb_gemm_nn_f32 with K = 512, ops.dropout's kernel: kernels unchanged by this feature, the yardstick — per
direction, and one whole training step of a two-layer SAGEEncoder (embedding -> encoder -> squared-norm loss -> backward), on the synthetic
S-arxiv and S-products graphs.
  time     warm-up twice, then the median (min - max) of --repeats runs timed with device events on the launching stream, launches, weight images and
           the operators' Python included; one process on the device; fused and composed alternate, so drift hits both alike
  forward  sage_layer_raw(relu, dropout 0.5);  backward  sage_layer_raw(backward=True, want_agg=True): G -> (dX, R);  step  forward + backward of the
           encoder with tuning.T.sage_fused on / off
Results are checked equal (torch.equal) between the two paths before anything is timed.  No ratio is promised: the table records what was measured.
    usage: python tools/bench_sage.py [--datasets S-arxiv S-products] [--modes SAGE GCN] [--repeats 7] [--out profiles/sage_times.md]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops, tuning  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import CSRGraph  # noqa: E402
from gnn_tail_generalization_amd.Link_prediction_model import SAGEEncoder  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure_pair(fa, fb, repeats):
    """Medians (min, max) of two functions timed alternately."""
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def fmt(t):
    return f'{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--modes', nargs='+', default=['SAGE', 'GCN'])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev = 'cuda:0'
    lines = ['| graph | nodes | edges | hubs fwd / bwd | mode | what | fused ms | composed ms | fused / composed |', '|---|---|---|---|---|---|---|---|---|']
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n = int(data.x.shape[0])
        G = CSRGraph(data.edge_index, n)
        del data
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(n, 256, device=dev, generator=g)
        dy = torch.randn(n, 256, device=dev, generator=g)
        W_n, W_s = torch.randn(256, 256, device=dev, generator=g) / 16, torch.randn(256, 256, device=dev, generator=g) / 16
        b = torch.randn(256, device=dev, generator=g)
        head = f'| {name} | {n} | {G.E} | {G._plan.n_hubs} / {G._plan_t.n_hubs} '
        for mode in a.modes:
            Ws = None if mode == 'GCN' else W_s
            s = ops.inv_indeg(G) if mode == 'SAGE' else None
            fwd = lambda fused: ops.sage_layer_raw(G, x, W_n, Ws, b, s, relu=True, p=0.5, seed=7, fused=fused)
            bwd = lambda fused: ops.sage_layer_raw(G, dy, W_n, Ws, None, s, backward=True, want_agg=True, fused=fused)
            for what, fn in (('forward', fwd), ('backward', bwd)):
                rf, rc = fn(True), fn(False)
                assert (rf[2], rc[2]) == ('fused', 'composed') and torch.equal(rf[0], rc[0]) and (rf[1] is None or torch.equal(rf[1], rc[1])), (name, mode, what)
                del rf, rc
                tf, tc = measure_pair(lambda: fn(True), lambda: fn(False), a.repeats)
                lines.append(head + f'| {mode} | layer {what} | {fmt(tf)} | {fmt(tc)} | {tf[0] / tc[0]:.3f} |')
                print(lines[-1], flush=True)
        torch.manual_seed(0)
        enc = SAGEEncoder(256, 256, 256, 2, 0.5).to(dev)
        emb = torch.nn.Parameter(torch.randn(n, 256, device=dev, generator=g) / 16)

        def step(fused):
            keep, tuning.T.sage_fused = tuning.T.sage_fused, fused
            try:
                enc.zero_grad()
                emb.grad = None
                h = enc(emb, G)
                (h * dy).sum().backward()
            finally:
                tuning.T.sage_fused = keep
        tf, tc = measure_pair(lambda: step(True), lambda: step(False), a.repeats)
        lines.append(head + f'| SAGE | 2-layer step | {fmt(tf)} | {fmt(tc)} | {tf[0] / tc[0]:.3f} |')
        print(lines[-1], flush=True)
        del G, x, dy, enc, emb
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    return text


if __name__ == '__main__':
    main()
