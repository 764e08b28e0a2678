"""Times the build of GraphMLP's adjacency power A~^r on the graph and r of tools/bench_ncloss.py (a synthetic power-law graph of the S-arxiv
shape, r = 2), A~ from graphUtils.normalize_adj on the host either way:
  host build    graphUtils.sparse_power (torch.sparse.mm on the CPU) + ops.SparsePower (two argsorts over all entries, then the upload); once
  device build  ops.SparsePower.from_adjacency (csrc/cb_spgemm.hip: expand - sort - compress per chunk, then the exact transpose), synchronised;
                two warm-up builds, then the median of `--repeats` builds (wall clock around a synchronised call), its stages from device
                events at the stage boundaries of ops.py (the gaps in which the host reads a count are part of the stage that ends there),
                and the peak device memory over what was allocated before the build.
The host build measured in the same run is the yardstick; no time is fixed in advance.
    usage: python tools/bench_power.py [--r 2] [--repeats 5] [--skip_host 0] [--out profiles/power.md]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops, tuning  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.utils import graphUtils  # noqa: E402

FIELDS = ('rowptr', 'col', 'val', 'rowptr_t', 'col_t', 'val_t')


def device_build(adj, r, dev, stages=None):
    """One synchronised build; wall seconds.  stages: dict name -> ms, filled from events recorded where ops.py enters a stage."""
    marks = []

    def hook(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    ops._stage_hook = hook if stages is not None else None
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp = ops.SparsePower.from_adjacency(adj, r, dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        ops._stage_hook = None
    for (name, e0), (_n, e1) in zip(marks, marks[1:]):
        stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1)
    return sp, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--r', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--skip_host', type=int, default=0, help='1: do not time the host build (then nothing is compared)')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev = 'cuda:0'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    data = synthetic_data('S-arxiv', seed=0, device='cpu')
    n = int(data.x.shape[0])
    t0 = time.perf_counter()
    adj = graphUtils.normalize_adj(data.edge_index, n)
    t_norm = time.perf_counter() - t0
    deg = torch.bincount(adj.indices()[0], minlength=n)
    products = int((deg[adj.indices()[1]]).sum())
    say(f'S-arxiv shape: N = {n}, nnz(A~) = {adj._nnz()}, r = {a.r}; {products} scalar products per multiplication by A~ at r = 2, largest degree {int(deg.max())}; '
        f'normalize_adj (host, both builds) {t_norm:.2f} s; {torch.get_num_threads()} host threads; chunk budget {tuning.T.spgemm_chunk_products} products')
    host = None
    if not a.skip_host:
        t0 = time.perf_counter()
        pw = graphUtils.sparse_power(adj, a.r)
        t_pow = time.perf_counter() - t0
        t0 = time.perf_counter()
        host = ops.SparsePower(pw, dev)
        torch.cuda.synchronize()
        t_form = time.perf_counter() - t0
        del pw
        say(f'- host build: {t_pow + t_form:.2f} s = sparse_power {t_pow:.2f} s + ops.SparsePower (argsorts + upload) {t_form:.2f} s; nnz = {host.nnz}')
    for _ in range(2):                                   # warm-up (allocator, code objects)
        sp, _dt = device_build(adj, a.r, dev)
        del sp
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times, stages, sp = [], {}, None
    for _ in range(a.repeats):
        del sp
        sp, dt = device_build(adj, a.r, dev)
        times.append(dt)
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    sp, _dt = device_build(adj, a.r, dev, stages)         # one more build with the stage events (not among the timed ones)
    med = statistics.median(times)
    say(f'- device build: median {med * 1e3:.1f} ms of {a.repeats} (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}), nnz = {sp.nnz}, '
        f'peak {peak:.2f} GiB of device memory over the inputs (the result itself: {sp.nnz * 16 / 2 ** 30:.2f} GiB in both orientations)')
    total = sum(stages.values())
    say(f'  stages of one build (device events, {total:.1f} ms): ' + ', '.join(f'{k} {v:.1f} ms' for k, v in stages.items()))
    if host is not None:
        same = all(torch.equal(getattr(sp, f), getattr(host, f)) for f in FIELDS)
        pattern = all(torch.equal(getattr(sp, f), getattr(host, f)) for f in ('rowptr', 'col', 'rowptr_t', 'col_t'))
        rel = float(((sp.val - host.val).abs() / host.val.abs().clamp_min(1e-30)).max()) if pattern else float('nan')
        say(f'- device / host = {med / (t_pow + t_form):.5f} ({(t_pow + t_form) / med:.0f} x); all six arrays bit-identical to the host build: {same}'
            f' (pattern identical: {pattern}, largest relative difference of a value {rel:.2e})')
        if med >= t_pow + t_form:
            say('  THE DEVICE BUILD IS NOT FASTER THAN THE HOST BUILD on this run.')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
