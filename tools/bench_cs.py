"""Times Correct & Smooth on the arxiv- and products-shaped synthetic graphs (ops.correct_and_smooth, the reference's default lpStep:
double_correlation_autoscale, A1 = DA, A2 = AD, 50 + 50 propagations):
  * one propagation step of each normalised adjacency (cb_spmm_csr_prop_f32: DAD / DA / AD) ALTERNATED in the same process with the
    label-propagation step cb_spmm_csr_lp_f32 on the same operands, `--repeats` rounds of `--steps` launches each -> median and spread;
  * the whole 50 + 50 call (2 row kernels + 100 launches), `--repeats` times.
Per-launch algorithmic bytes: G.algorithmic_bytes(Cp, bias=False) (edges: 4 Cp + 4, rows: 4 Cp + 4, row scale 4) plus the mix rows (4 Cp N) and the
state factor (4 N).       usage: python tools/bench_cs.py [--datasets S-arxiv S-products] [--repeats 7] [--steps 20] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import CSRGraph  # noqa: E402


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def spread(v):
    return f'{statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev = 'cuda:0'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n = int(data.x.shape[0])
        G = CSRGraph(data.edge_index, n)
        c = int(data.y.max()) + 1
        cp = ops.padded_classes(c)
        del data.x
        gen = torch.Generator(device=dev).manual_seed(1)
        p = torch.softmax(2 * torch.randn(n, c, device=dev, generator=gen), 1)
        dis = G.in_degrees().float().pow(-0.5)
        dis[dis == float('inf')] = 0
        y = torch.nn.functional.pad(p, (0, cp - c)).contiguous()
        out = torch.empty_like(y)
        alpha = 0.9791632871592579
        nbytes = G.algorithmic_bytes(cp, bias=False) + 4 * cp * n + 4 * n
        say(f'## {name}: N = {n}, E = {G.E}, C = {c} (rows of {cp} floats), {nbytes / 1e9:.3f} GB algorithmic bytes per step')
        a_dis = (dis * alpha).contiguous()
        h_dad = (dis[:, None] * y).contiguous()

        def lp_step():
            G.spmm_lp(h_dad, a_dis, y, 1 - alpha, dis, out=out)
        steps = {}
        for form in ops.ADJ_FORMS:
            R, S = ops.adj_scales(dis, form)
            a_r = (R * alpha).contiguous() if R is not None else torch.full((n,), alpha, device=dev)
            h = y if S is None else (S[:, None] * y).contiguous()
            steps[form] = (lambda h=h, a_r=a_r, S=S: G.spmm_prop(h, a_r, y, 1 - alpha, clamp=(-1.0, 1.0), post_scale=S, out=out))
        for fn in [lp_step] + list(steps.values()):
            timed(fn, 3)                                         # warm-up
        t = {k: [] for k in ['lp'] + list(steps)}
        for _ in range(a.repeats):                               # alternated: every round times the parent's step and the three forms back to back
            t['lp'].append(timed(lp_step, a.steps))
            for form, fn in steps.items():
                t[form].append(timed(fn, a.steps))
        for k, v in t.items():
            med = statistics.median(v)
            say(f'- {"cb_spmm_csr_lp_f32 (DAD, clamp 0..1)" if k == "lp" else "cb_spmm_csr_prop_f32 " + k}: {spread(v)} per step, '
                f'{nbytes / med / 1e6:.0f} GB/s; ratio to the LP step {med / statistics.median(t["lp"]):.3f}')
        idx = torch.where(data.train_mask)[0]

        def whole():
            return ops.correct_and_smooth(G, p, data.y, idx, 'double_correlation_autoscale', 'DA', alpha, 50, 'AD', 0.7564990804200602, 50, deg_inv_sqrt=dis)
        whole()
        torch.cuda.synchronize()
        tw = [timed(whole, 1) for _ in range(a.repeats)]
        say(f'- whole call, 50 + 50 propagations + 2 row kernels: {spread(tw)}; the 100 steps alone at the DA / AD medians: '
            f'{50 * statistics.median(t["DA"]) + 50 * statistics.median(t["AD"]):.1f} ms')
        del G, data, p, y, out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
