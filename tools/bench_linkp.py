"""Times the three pieces of the teacher's edge-wise term (csrc/cb_linkp.hip; ops.LinkSampler / ops.linkp_loss_eva) at the S-arxiv and S-products
shapes, with the default sample sizes (--samp_size_p 200, --samp_size_n_train 200) and with 64 times them, each next to a composition of torch
operators on the same device:
  (a) one negative draw          against a torch restatement of the method of PyG's `negative_sampling`: linearise the whole edge list, draw
                                 candidates, `isin`-test them against it, keep the survivors (a boolean index: one host synchronisation)
  (b) one positive draw          against the reference's mask of the whole edge list, compaction and indexed draw (trainer…:512-524)
  (c) loss forward + backward    against index_select x 4 / sum / binary_cross_entropy_with_logits / sort + nonzero (utils.py:754-791), D = the
                                 dataset's class count (the default dim_commonEmb) and D = 128 (--has_proj2class=1)
Warm-up, then the median over --repeats runs timed with device events (one process on the device).  What to look for: (a) and (b) of the HIP
path do not grow with E.
    usage: python tools/bench_linkp.py [--datasets S-arxiv S-products] [--repeats 9] [--out profiles/linkp.md]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import CSRGraph  # noqa: E402


def torch_negatives(edge_index, n, num):
    """`negative_sampling(edge_index, num_neg_samples=num, force_undirected=True)` restated: num / 2 undirected non-edges, both directions."""
    idx = edge_index[0] * n + edge_index[1]
    k = num // 2
    rnd = torch.randint(0, n * n, (int(1.1 * k) + 8,), device=edge_index.device)
    rnd = rnd[~torch.isin(rnd, idx)][:k]
    u, v = rnd // n, rnd % n
    return torch.stack([torch.cat([u, v]), torch.cat([v, u])])


def torch_positives(edge_index, mask, num):
    valid = edge_index[:, mask[edge_index[0]] & mask[edge_index[1]]]
    return valid[:, torch.randint(0, valid.shape[1], (num,), device=edge_index.device)]


def torch_loss(emb, pos, neg):
    ps = (emb.index_select(0, pos[0]) * emb.index_select(0, pos[1])).sum(-1)
    ns = (emb.index_select(0, neg[0]) * emb.index_select(0, neg[1])).sum(-1)
    score = torch.cat([ps, ns])
    label = torch.cat([torch.ones_like(ps), torch.zeros_like(ns)])
    k = len(ns) // len(ps)
    both = torch.cat([ps.detach().reshape(-1, 1), ns.detach()[:k * len(ps)].reshape(len(ps), k)], dim=1)
    rank = torch.nonzero(torch.sort(both, dim=1, descending=True)[1] == 0)[:, 1] + 1
    return F.binary_cross_entropy_with_logits(score, label), (1.0 / rank).mean()


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
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev = 'cuda:0'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(what, hip, ref):
        say(f'| {what} | {hip[0] * 1e3:.0f} ({hip[1] * 1e3:.0f} .. {hip[2] * 1e3:.0f}) | {ref[0] * 1e3:.0f} ({ref[1] * 1e3:.0f} .. {ref[2] * 1e3:.0f}) | {hip[0] / ref[0]:.3f} |')
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n, ei = int(data.x.shape[0]), data.edge_index
        C = int(data.y.max()) + 1
        graph = CSRGraph(ei, n)
        sampler = ops.LinkSampler(graph, data.train_mask)
        sampler.positives('train', 8)                                              # the prefix arrays: once, off the step
        say(f'\n## {name}: N = {n}, E = {int(ei.shape[1])}, {sampler.n_train} train nodes\n')
        say('| piece | HIP path, us: median (min .. max) | torch composition, us | HIP / torch |')
        say('|---|---|---|---|')
        for mult in (1, 64):
            P = Nn = 200 * mult
            row(f'(a) negatives, train mode, Nn = {Nn}', measure(lambda: sampler.negatives('train', Nn), a.repeats),
                measure(lambda: torch_negatives(ei, n, Nn), a.repeats))
            row(f'(b) positives, train mode, P = {P}', measure(lambda: sampler.positives('train', P), a.repeats),
                measure(lambda: torch_positives(ei, data.train_mask, P), a.repeats))
            sampler.check()
            pos, neg = sampler.positives('train', P, seed=1), sampler.negatives('train', Nn, seed=2)
            pos64, neg64 = pos.long(), neg.long()
            for D in (C, 128):
                emb = (torch.randn(n, D, device=dev) * 0.3).requires_grad_(True)

                def hip():
                    emb.grad = None
                    ops.linkp_loss_eva(emb, pos, neg)[0].backward()

                def ref():
                    emb.grad = None
                    torch_loss(emb, pos64, neg64)[0].backward()
                row(f'(c) loss forward + backward, P = Nn = {P}, D = {D}', measure(hip, a.repeats), measure(ref, a.repeats))
                with torch.no_grad():
                    l_h, m_h = ops.linkp_loss_eva(emb, pos, neg)
                    l_t, m_t = torch_loss(emb, pos64, neg64)
                say(f'| &nbsp;&nbsp; loss {float(l_h):.6f} vs {float(l_t):.6f}, MRR {float(m_h):.4f} vs {float(m_t):.4f} | | | |')
                del emb
        del data, graph, sampler, ei
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
