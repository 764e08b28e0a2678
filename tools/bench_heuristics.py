"""Times the CN / AA pair scores (csrc/cb_heur.hip; ops.pair_scores) at the S-arxiv and S-products shapes for P = 1e5 and 1e6 pairs of two
populations — uniform random node pairs, and ops.LinkSampler positives, which are hub-heavy (an endpoint of a uniformly drawn edge is a node
drawn in proportion to its degree): the hard case — and the rank counts (ops.rank_counts) at P = 1e5, Nn = 1e7 against torch.sort +
searchsorted on the device.
  device      ops.pair_scores with 16 and with 64 lanes per pair, launches and the operator's status bookkeeping included; warm-up, then the
              median over --repeats runs timed with device events (one process on the device)
  host        the reference's method (Link_prediction_baseline/heuristics.py:107-129): scipy `A[src].multiply(A_[dst])` summed per row, in
              batches of 100 000 pairs, on this machine's CPU threads; timed once per row over its first --host_pairs pairs (default: all).  If scipy
              does not import the column reads "not measured"; nothing else is put in its place
  bound       the bytes a merge of the two rows would have to read, 4 (len_s + len_d) per pair, over the measured time as a share of 8 TB/s: a
              bound the search-based kernel is not expected to reach (it reads the long row by dependent probes, not as a stream)
No speed threshold is fixed in advance: the table records what was measured, also where the device path loses.
    usage: python tools/bench_heuristics.py [--datasets S-arxiv S-products] [--pairs 100000 1000000] [--repeats 9] [--host_pairs 1000000] [--out profiles/heuristics.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import CSRGraph  # noqa: E402

HBM_BYTES_PER_S = 8e12
HOST_BATCH = 100000


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


def host_matrices(edge_index, n):
    """(A, A_) as the reference builds them (:19-24, 119-121), or None where scipy does not import."""
    try:
        import scipy.sparse as ssp
    except ImportError:
        return None
    ei = edge_index.cpu().numpy()
    A = ssp.csr_matrix((np.ones(ei.shape[1], dtype=int), (ei[0], ei[1])), shape=(n, n))
    with np.errstate(divide='ignore'):
        mult = 1 / np.log(A.sum(axis=0))
    mult[np.isinf(mult)] = 0
    return A, A.multiply(mult).tocsr()


def host_scores(A, B, pairs):
    out = []
    for i in range(0, pairs.shape[1], HOST_BATCH):
        src, dst = pairs[0, i:i + HOST_BATCH], pairs[1, i:i + HOST_BATCH]
        out.append(np.array(np.sum(A[src].multiply(B[dst]), 1)).flatten())
    return np.concatenate(out, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--pairs', nargs='+', type=int, default=[100000, 1000000])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--host_pairs', type=int, default=1000000, help='pairs the host method is timed over (0: skip the host)')
    ap.add_argument('--rank_p', type=int, default=100000)
    ap.add_argument('--rank_n', type=int, default=10000000)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    dev = 'cuda:0'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    say('# CN / AA pair scores and rank counts (`tools/bench_heuristics.py`)\n')
    say(f'One MI355X, one process; device times are medians of {a.repeats} runs after two warm-up runs, device events, launches and the operator\'s status '
        f'bookkeeping included.  Host: scipy `A[src].multiply(A_[dst])` in batches of {HOST_BATCH} on {os.cpu_count()} visible CPUs '
        f'({os.environ.get("OMP_NUM_THREADS", "unset")} threads allowed), timed once per row over its first {a.host_pairs} pairs.  "merge bound": 4 (len_s + len_d) bytes per pair over the '
        'measured time as a share of 8 TB/s — a bound the search-based kernel is not expected to reach.')
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n, ei = int(data.x.shape[0]), data.edge_index
        graph = CSRGraph(ei, n)
        sampler = ops.LinkSampler(graph, data.train_mask)
        deg = (graph.rowptr_t[1:] - graph.rowptr_t[:-1]).to(torch.int64)
        say(f'\n## {name}: N = {n}, E = {int(ei.shape[1])}, largest out-row {int(deg.max())}\n')
        host = None
        if a.host_pairs:
            t0 = time.perf_counter()
            host = host_matrices(ei, n)
            say(f'host matrices (scipy CSR + the AA-weighted copy): {"not measured (scipy does not import)" if host is None else f"{time.perf_counter() - t0:.1f} s, once"}\n')
        say('| pairs | kind | 16 lanes / pair, ms: median (min .. max) | 64 lanes / pair, ms | pairs / s (16) | merge bound, share of 8 TB/s (16) | host scipy, pairs / s | device (16) / host |')
        say('|---|---|---|---|---|---|---|---|')
        for P in a.pairs:
            pops = {'uniform': torch.randint(0, n, (2, P), device=dev, generator=torch.Generator(device=dev).manual_seed(P)).to(torch.int32),
                    'positives': sampler.positives('train', P, seed=P)}
            for pop, pairs in pops.items():
                merge_bytes = 4 * int((deg[pairs[0].long()] + deg[pairs[1].long()]).sum())
                for kind in ('CN', 'AA'):
                    t16 = measure(lambda: ops.pair_scores(graph, pairs, kind, group=16), a.repeats)
                    t64 = measure(lambda: ops.pair_scores(graph, pairs, kind, group=64), a.repeats)
                    same = torch.equal(ops.pair_scores(graph, pairs, 'CN', group=16), ops.pair_scores(graph, pairs, 'CN', group=64))
                    ops.pair_scores_check()
                    host_txt, ratio_txt = 'not measured', 'not measured'
                    if host is not None:
                        hp = pairs[:, :a.host_pairs].cpu().numpy().astype(np.int64)
                        t0 = time.perf_counter()
                        hs = host_scores(host[0], host[0] if kind == 'CN' else host[1], hp)
                        dt = time.perf_counter() - t0
                        got = ops.pair_scores(graph, pairs[:, :a.host_pairs], kind).cpu().numpy().astype(np.float64)
                        agree = bool((np.abs(got - hs) <= 2.0 ** -23 * np.abs(hs)).all())
                        host_txt = f'{hp.shape[1] / dt:.3g} ({dt:.2f} s for {hp.shape[1]}; scores agree: {agree})'
                        ratio_txt = f'{(P / (t16[0] * 1e-3)) / (hp.shape[1] / dt):.1f} x'
                    say(f'| {P} {pop} | {kind} | {t16[0]:.3f} ({t16[1]:.3f} .. {t16[2]:.3f}) | {t64[0]:.3f} ({t64[1]:.3f} .. {t64[2]:.3f}) | {P / (t16[0] * 1e-3):.3g} | '
                        f'{merge_bytes / (t16[0] * 1e-3) / HBM_BYTES_PER_S * 100:.2f} % ({merge_bytes / 1e6:.1f} MB) | {host_txt} | {ratio_txt} |'
                        + ('' if same else ' CN DIFFERS BETWEEN THE WIDTHS |'))
                    flush_out()
        del data, graph, sampler, ei, host, deg
        torch.cuda.empty_cache()
    # rank counts (--rank_p 0: skipped)
    P, Nn = a.rank_p, a.rank_n
    if P == 0:
        flush_out()
        return
    g = torch.Generator(device=dev).manual_seed(3)
    for label, pos, neg in (('real-valued scores', torch.randn(P, device=dev, generator=g), torch.randn(Nn, device=dev, generator=g)),
                            ('integer scores 0..15 (CN-like, heavy ties)', torch.randint(0, 16, (P,), device=dev, generator=g).float(),
                             torch.randint(0, 16, (Nn,), device=dev, generator=g).float())):
        def torch_counts():
            s = torch.sort(neg).values
            hi = torch.searchsorted(s, pos, right=True)
            lo = torch.searchsorted(s, pos, right=False)
            return (Nn - hi).to(torch.int32), (hi - lo).to(torch.int32)
        th = measure(lambda: ops.rank_counts(pos, neg), a.repeats)
        tt = measure(torch_counts, a.repeats)
        gt, eq = ops.rank_counts(pos, neg)
        gt_t, eq_t = torch_counts()
        if label.startswith('real'):
            say(f'\n## rank counts, P = {P}, Nn = {Nn}\n')
            say('| scores | ops.rank_counts, ms: median (min .. max) | torch.sort + 2 searchsorted, ms | HIP / torch | counts equal |')
            say('|---|---|---|---|---|')
        say(f'| {label} | {th[0]:.2f} ({th[1]:.2f} .. {th[2]:.2f}) | {tt[0]:.2f} ({tt[1]:.2f} .. {tt[2]:.2f}) | {th[0] / tt[0]:.2f} | '
            f'{bool(torch.equal(gt, gt_t) and torch.equal(eq, eq_t))} |')
        flush_out()


if __name__ == '__main__':
    main()
