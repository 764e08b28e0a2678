"""Times forward + backward of the fused neighbour-contrastive loss (ops.neighbor_contrastive_loss, csrc/cb_ncloss.hip) at B in {4096, 16384,
65536}, D = 256, against the r = 2 power of a synthetic power-law graph of the S-arxiv shape, next to the same loss composed from torch's
operators on the same device — the reference's dense [B, B] form (MLP_model/__init__.py:190-208) — wherever that form fits in memory.
Also times the operator with a power that yields no pair: the difference is the share of the sparse walks (float64 per pair).
Warm-up, then the median over `--repeats` timed runs (device events, one process on the device); peak memory of each form.
    usage: python tools/bench_ncloss.py [--batches 4096 16384 65536] [--repeats 7] [--tau 2.0] [--out FILE.md]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.utils import graphUtils  # noqa: E402


def dense_loss(z, adj_b, tau):
    """The reference's composition (:190-208) with the cropped adjacency already dense on the device."""
    n = torch.norm(z, p=2, dim=1, keepdim=True)
    cos = (z @ z.T) * ((n @ n.T) ** (-1))
    simz = (1 - torch.eye(len(z), device=z.device)) * torch.exp(cos / tau)
    num, den = (adj_b * simz).sum(1), simz.sum(1)
    nz = torch.where(num != 0)[0]
    return -torch.mean(torch.log(num[nz] / den[nz]))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, repeats):
    fn()
    fn()                                             # warm-up (allocator, code objects)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = [timed(fn) for _ in range(repeats)]
    return statistics.median(t), min(t), max(t), (torch.cuda.max_memory_allocated() - base) / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[4096, 16384, 65536])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--tau', type=float, default=2.0)
    ap.add_argument('--dense_max_gib', type=float, default=96.0, help='the dense form keeps about 10 B x B fp32 matrices alive; skipped above this')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev, D = 'cuda:0', 256
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    data = synthetic_data('S-arxiv', seed=0, device='cpu')
    n = int(data.x.shape[0])
    adj_pow = graphUtils.sparse_power(graphUtils.normalize_adj(data.edge_index, n), 2)
    power = ops.SparsePower(adj_pow, dev)
    empty = ops.SparsePower(torch.sparse_coo_tensor(torch.zeros((2, 1), dtype=torch.long), torch.ones(1), (n, n)), dev)      # one diagonal entry, which the mask removes: no pair, the sweeps and the GEMM alone
    say(f'S-arxiv shape: N = {n}, E = {int(data.edge_index.shape[1])}, power r = 2: nnz = {power.nnz}; D = {D}, tau = {a.tau}')
    gen = torch.Generator().manual_seed(1)
    for B in a.batches:
        idx = torch.randint(0, n, (B,), generator=gen)
        z = torch.randn(B, D, generator=gen).to(dev).requires_grad_(True)
        slab = ops._ncloss_slab_rows(B)

        def fused():
            z.grad = None
            ops.neighbor_contrastive_loss(z, power, idx, a.tau).backward()
        med, lo, hi, mem = measure(fused, a.repeats)

        def dense_part():
            z.grad = None
            ops.neighbor_contrastive_loss(z, empty, idx, a.tau).backward()
        med_e = measure(dense_part, a.repeats)[0]
        say(f'- B = {B}: fused {med:.2f} ms (min {lo:.2f}, max {hi:.2f}), peak {mem:.2f} GiB over the inputs; core {ops.ncloss_core(z.detach())}, '
            f'slab {min(slab, B)} rows ({min(slab, B) * B * 4 / 2 ** 30:.2f} GiB), {6 * B * B * D / med / 1e9:.1f} TFLOP/s of 3 sweep-sized products; '
            f'with a power without pairs (sweeps + GEMM only) {med_e:.2f} ms, so the float64 sparse walks take {med - med_e:.2f} ms = {100 * (med - med_e) / med:.0f} %')
        if 10 * B * B * 4 / 2 ** 30 > a.dense_max_gib:
            say(f'  torch composition: skipped, about {10 * B * B * 4 / 2 ** 30:.0f} GiB of [B, B] fp32 matrices do not fit')
            continue
        adj_b = graphUtils.crop_adj_to_subgraph(adj_pow, idx).to(dev).to_dense()

        def dense():
            z.grad = None
            dense_loss(z, adj_b, a.tau).backward()
        with torch.no_grad():
            l_f, l_d = float(ops.neighbor_contrastive_loss(z.detach(), power, idx, a.tau)), float(dense_loss(z.detach(), adj_b, a.tau))
        med_d, lo_d, hi_d, mem_d = measure(dense, a.repeats)
        say(f'  torch composition {med_d:.2f} ms (min {lo_d:.2f}, max {hi_d:.2f}), peak {mem_d:.2f} GiB over the inputs (+ the dense cropped adjacency, '
            f'{B * B * 4 / 2 ** 30:.2f} GiB, built outside the timing); fused / torch = {med / med_d:.2f}; loss {l_f:.6f} vs {l_d:.6f}')
        del adj_b
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
