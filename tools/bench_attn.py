"""Times the attention layer of the Transformer link-prediction encoder (ops.transformer_conv: one stacked GEMM + csrc/cb_attn.hip) against its
restatement in torch's own device operators — the stacked Linear through torch.nn.functional.linear, index_select, scatter_reduce(amax), index_add_ and
autograd — on the synthetic S-arxiv and S-products graphs:
  layer     one 256 -> 256 layer, forward (no_grad) and forward + backward
  step      a two-layer TransformerEncoder training step (embedding -> encoder -> sum(h * dY) -> backward), dropout 0
  kernels   the three attention entries alone (ops.attn_raw, ops.attn_bwd_raw one part at a time): time, algorithmic bytes (rows gathered plus rows
            read and written once: see attn_bytes) and those bytes over time as a fraction of 8 TB/s
  time      two warm-up runs, then the median (min - max) of --repeats runs timed with device events on the launching stream, the operators' Python
            included; fused and torch alternate, so drift hits both alike; one process on the device
The torch path needs E x D temporaries (1.2 GB each at S-arxiv, 63 GB at S-products).  Above --chunk_edges edges it walks the edge list in chunks (the
scores, the maxima and the sums over all edges first, then the weighted rows chunk by chunk) and recomputes each chunk in the backward
(torch.utils.checkpoint), which is what lets it finish at S-products; the table says where that form ran.  Results of the two paths are compared
(a layer without the ReLU, relative to the largest reference value) before anything is timed.  No ratio is promised: the table records what was measured.
    usage: python tools/bench_attn.py [--datasets S-arxiv S-products] [--repeats 7] [--out profiles/attn_times.md]"""
import argparse
import math
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_tail_generalization_amd import ops  # noqa: E402
from gnn_tail_generalization_amd.data import synthetic_data  # noqa: E402
from gnn_tail_generalization_amd.graph import CSRGraph  # noqa: E402
from gnn_tail_generalization_amd.Link_prediction_model import TransformerEncoder  # noqa: E402

NAMES = ('lin_key', 'lin_query', 'lin_value', 'lin_skip')
PEAK = 8.0e12      # bytes / s


def attn_bytes(n, e, d):
    """Algorithmic bytes per kernel: each edge gathers two rows of d floats once (K | V by destination, Q | dO by source; the by-dst backward walks a
    row twice and is charged once), each node row is read / written once per operand, scalars (column ids, lse, delta) counted."""
    row = 4 * d
    return {'fwd': e * (2 * row + 4) + n * (3 * row + 8), 'bwd_dst': e * (2 * row + 4) + n * (3 * row + 12), 'bwd_src': e * (2 * row + 12) + n * (4 * row + 4)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(fns, repeats):
    """Medians (min, max) in ms of functions timed alternately."""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return f'{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})'


def torch_layer(x, p, src, dst, relu, chunk_edges):
    """The layer in torch's operators with autograd.  p: (W [4 D, in], b [4 D]) stacked as [Q | K | V | S]."""
    n, d = x.shape[0], p[0].shape[0] // 4
    Q, K, V, S = F.linear(x, p[0], p[1]).split(d, 1)
    scale = 1.0 / math.sqrt(d)
    E = src.numel()
    cuts = list(range(0, E, chunk_edges)) + [E]
    whole = len(cuts) == 2

    def scores(Q, K, a, b):
        return (Q.index_select(0, dst[a:b]) * K.index_select(0, src[a:b])).sum(-1) * scale

    def weighted(Q, K, V, m, l, a, b):
        w = torch.exp(scores(Q, K, a, b) - m.index_select(0, dst[a:b])) / l.index_select(0, dst[a:b])
        return torch.zeros((n, d), dtype=x.dtype, device=x.device).index_add_(0, dst[a:b], w[:, None] * V.index_select(0, src[a:b]))

    with torch.no_grad():      # (the derivative with respect to the subtracted maximum is zero)
        m = torch.full((n,), float('-inf'), dtype=x.dtype, device=x.device)
        for a, b in zip(cuts[:-1], cuts[1:]):
            m = m.scatter_reduce(0, dst[a:b], scores(Q, K, a, b), 'amax', include_self=True)
    if whole:
        s = scores(Q, K, 0, E)
        pr = torch.exp(s - m.index_select(0, dst))
        l = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, dst, pr)
        w = pr / l.index_select(0, dst)
        out = torch.zeros((n, d), dtype=x.dtype, device=x.device).index_add_(0, dst, w[:, None] * V.index_select(0, src)) + S
    else:
        l = torch.zeros(n, dtype=x.dtype, device=x.device)
        for a, b in zip(cuts[:-1], cuts[1:]):
            l = l + checkpoint(lambda Q, K, a=a, b=b: torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(
                0, dst[a:b], torch.exp(scores(Q, K, a, b) - m.index_select(0, dst[a:b]))), Q, K, use_reentrant=False)
        out = S
        for a, b in zip(cuts[:-1], cuts[1:]):
            out = out + checkpoint(lambda Q, K, V, l, a=a, b=b: weighted(Q, K, V, m, l, a, b), Q, K, V, l, use_reentrant=False)
    return torch.relu(out) if relu else out


def stacked(conv):
    order = ('lin_query', 'lin_key', 'lin_value', 'lin_skip')
    return torch.cat([getattr(conv, l).weight for l in order]), torch.cat([getattr(conv, l).bias for l in order])


def clocks():
    """What the device reports for its clocks (read only); 'not read' where the tool is absent."""
    for cmd in (['rocm-smi', '--showclocks'], ['amd-smi', 'metric', '--clock']):
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=30)
        except (OSError, subprocess.TimeoutExpired):
            continue
        if r.returncode == 0 and r.stdout.strip():
            keep = [ln.strip() for ln in r.stdout.splitlines() if 'GPU[0]' in ln and ('sclk' in ln or 'mclk' in ln or 'fclk' in ln)]
            return '; '.join(keep) if keep else 'reported, no sclk / mclk line for GPU 0'
    return 'not read'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', nargs='+', default=['S-arxiv', 'S-products'])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--chunk_edges', type=int, default=8 << 20)
    ap.add_argument('--d', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev, d = 'cuda:0', a.d
    lines = [f'clocks before the runs: {clocks()}', '',
             '| graph | nodes | edges | hubs fwd / bwd | what | fused ms | torch ms | fused / torch | torch form |', '|---|---|---|---|---|---|---|---|---|']
    klines = ['| graph | kernel | ms | algorithmic GB | fraction of 8 TB/s |', '|---|---|---|---|---|']
    for name in a.datasets:
        data = synthetic_data(name, seed=0, device=dev)
        n = int(data.x.shape[0])
        G = CSRGraph(data.edge_index, n)
        src, dst = data.edge_index[0].contiguous(), data.edge_index[1].contiguous()
        del data
        form = 'whole edge list' if G.E <= a.chunk_edges else f'chunks of {a.chunk_edges} edges, recomputed in the backward'
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(n, d, device=dev, generator=g)
        dy = torch.randn(n, d, device=dev, generator=g)
        torch.manual_seed(0)
        enc = TransformerEncoder(d, d, d, 2, 0.0).to(dev)
        conv = enc.convs[0]
        args8 = [t for l in NAMES for t in (getattr(conv, l).weight, getattr(conv, l).bias)]
        head = f'| {name} | {n} | {G.E} | {G._plan.n_hubs} / {G._plan_t.n_hubs} '

        def fused_fwd(relu=True):
            with torch.no_grad():
                return ops.transformer_conv(G, x, *args8, relu=relu)

        def torch_fwd(relu=True):
            with torch.no_grad():
                return torch_layer(x, stacked(conv), src, dst, relu, a.chunk_edges)

        def fused_fb(relu=True):
            enc.zero_grad()
            xr = x.detach().requires_grad_(True)
            ops.transformer_conv(G, xr, *args8, relu=relu).backward(dy)
            return xr.grad

        def torch_fb(relu=True):
            enc.zero_grad()
            xr = x.detach().requires_grad_(True)
            torch_layer(xr, stacked(conv), src, dst, relu, a.chunk_edges).backward(dy)
            return xr.grad

        for what, ff, ft in (('layer forward', fused_fwd, torch_fwd), ('layer forward + backward', fused_fb, torch_fb)):
            rf, rt = ff(relu=False), ft(relu=False)      # (without the ReLU: an output within rounding of 0 flips its mask between two fp32 evaluations)
            rel = float((rf - rt).abs().max() / rt.abs().max())
            assert rel < 1e-3, (name, what, rel)
            del rf, rt
            tf, tt = measure([ff, ft], a.repeats)
            lines.append(head + f'| {what} | {fmt(tf)} | {fmt(tt)} | {tf[0] / tt[0]:.3f} | {form} |')
            print(lines[-1], flush=True)

        emb = torch.nn.Parameter(torch.randn(n, d, device=dev, generator=g) / 16)

        def fused_step():
            enc.zero_grad()
            emb.grad = None
            (enc(emb, G) * dy).sum().backward()

        def torch_step():
            enc.zero_grad()
            emb.grad = None
            h = torch_layer(emb, stacked(enc.convs[0]), src, dst, True, a.chunk_edges)
            (torch_layer(h, stacked(enc.convs[1]), src, dst, False, a.chunk_edges) * dy).sum().backward()

        tf, tt = measure([fused_step, torch_step], a.repeats)
        lines.append(head + f'| 2-layer step | {fmt(tf)} | {fmt(tt)} | {tf[0] / tt[0]:.3f} | {form} |')
        print(lines[-1], flush=True)

        # the three kernels alone
        with torch.no_grad():
            W, b = stacked(conv)
            P = F.linear(x, W, b)
        q, k, v, s = [P[:, i * d:(i + 1) * d] for i in range(4)]
        dP = torch.empty_like(P)
        dq, dk, dv = [dP[:, i * d:(i + 1) * d] for i in range(3)]
        out, lse = ops.attn_raw(G, q, k, v, s)
        delta = ops.attn_bwd_raw(G, q, k, v, dy, lse, dq, dk, dv)
        nb = attn_bytes(n, G.E, d)
        ts = measure([lambda: ops.attn_raw(G, q, k, v, s), lambda: ops.attn_bwd_raw(G, q, k, v, dy, lse, dq, dk, dv, parts=('dst',)),
                      lambda: ops.attn_bwd_raw(G, q, k, v, dy, lse, dq, dk, dv, parts=('src',), delta_in=delta)], a.repeats)
        for kname, t in zip(('fwd', 'bwd_dst', 'bwd_src'), ts):
            klines.append(f'| {name} | cb_attn_{kname}_f32 | {fmt(t)} | {nb[kname] / 1e9:.3f} | {nb[kname] / (t[0] * 1e-3) / PEAK:.3f} |')
            print(klines[-1], flush=True)
        del G, x, dy, enc, emb, P, dP, out, lse, delta, src, dst
        torch.cuda.empty_cache()
    lines += ['', f'clocks after the runs: {clocks()}', ''] + klines
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    return text


if __name__ == '__main__':
    main()
