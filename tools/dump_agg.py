#!/usr/bin/env python3
"""Bit comparison of two builds of the aggregation kernels (profiles/agg_core.md).

  python tools/dump_agg.py dump OUT_DIR [--root REPO_ROOT]    outputs of every aggregation entry point of the build under REPO_ROOT (default: this tree)
  python tools/dump_agg.py compare DIR_A DIR_B                torch.equal on every tensor, NaN positions as masks; exit status 1 on a difference

Every output is taken on two graphs: a small one with hub threshold 4 and a power-law graph of 70 000 rows; both also with flagged column ids (gather
policy 2; the d % 256 == 0 entries and the model steps), which graphs of this size get only under a reduced tuning.T.hot_bytes."""
import argparse
import os
import sys

import torch

DEV = 'cuda:0'


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _hot_bytes(n):
    """tuning.T.hot_bytes under which a graph of n rows gets flagged column ids (graph.py _hot_cols: n >= 2 * hot_bytes / 1024)"""
    return (64 if n < 1000 else 16384) * 1024


def _graphs():
    from gnn_tail_generalization_amd import tuning
    from gnn_tail_generalization_amd.data import powerlaw_pairs
    from gnn_tail_generalization_amd.graph import CSRGraph
    g = torch.Generator().manual_seed(1)
    n = 331      # five full 64-row tiles and one of 11; a row of 150 in-edges, a source of 150 out-edges, rows without in-edges
    src, dst = torch.randint(0, n, (2200,), generator=g), torch.randint(0, n, (2200,), generator=g)
    keep = (dst != 7) & (dst != 64) & (dst != 330)
    hub = torch.stack([torch.randint(0, n, (150,), generator=g), torch.full((150,), 63)])
    fan = torch.stack([torch.full((150,), 5), torch.randint(8, 60, (150,), generator=g)])
    ei_small = torch.cat([torch.stack([src[keep], dst[keep]]), hub, fan], 1).to(DEV)
    big = 70000
    pairs = powerlaw_pairs(big, 12 * big, 2.2, torch.Generator().manual_seed(2), 'cpu')
    ei_big = torch.cat([pairs, pairs[:, : pairs.shape[1] // 2].flip(0)], 1).to(DEV)      # (directed: the two orientations differ)
    out = {}
    keep_hot = tuning.T.hot_bytes
    for name, ei, nn, thr in (('small', ei_small, n, 4), ('big', ei_big, big, None)):
        out[name] = CSRGraph(ei, nn, hub_threshold=thr)
        tuning.T.hot_bytes = _hot_bytes(nn)      # flagged column ids on a graph of this size
        try:
            out[name + '_flags'] = CSRGraph(ei, nn, hub_threshold=thr)
        finally:
            tuning.T.hot_bytes = keep_hot
        assert out[name + '_flags'].col_k is not None and out[name]._plan.n_hubs > 0
    return out


def _entries(G, res, tag, flags_only):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.graph import weight_image
    N = G.N
    g = torch.Generator().manual_seed(3)
    h, rs, cs, b = _rand(g, N, 256), torch.rand(N, generator=g).to(DEV) + 0.5, torch.rand(N, generator=g).to(DEV) + 0.5, _rand(g, 256)
    put = lambda k, *ts: res.update({f'{tag}/{k}/{i}': t.detach().cpu() for i, t in enumerate(ts) if t is not None})
    for tr in (False, True):
        put(f'plain_t{int(tr)}', G.spmm(h, transpose=tr), G.spmm(h, transpose=tr, row_scale=rs, bias=b, relu=True))
        put(f'col_scale_t{int(tr)}', G.spmm(h, transpose=tr, row_scale=rs, col_scale=cs))
    for d in () if flags_only else (512, 300, 130, 128, 40):      # two column tiles; ragged float4, float2 and scalar lanes
        hd = _rand(g, N, d)
        put(f'plain_d{d}', G.spmm(hd, row_scale=rs, bias=_rand(g, d), relu=True), G.spmm(hd.to(torch.bfloat16), row_scale=rs))
    acc = _rand(g, N, 256)
    put('acc_init', G.spmm(h, row_scale=rs, bias=b, acc_init=acc), G.spmm(h.to(torch.bfloat16), acc_init=acc))
    raw = acc.clone()
    put('acc_skip_empty', G.spmm(h, out=raw, acc_init=raw))
    if not flags_only:
        put('acc_init_d300', G.spmm(_rand(g, N, 300), acc_init=_rand(g, N, 300), row_scale=rs))
    put('bf16', G.spmm(h.to(torch.bfloat16), row_scale=rs, bias=b, relu=True))
    # the store's backward, raw and with the folded mix gradients + column sums
    bits = torch.randint(-2 ** 62, 2 ** 62, (N, 4), generator=g, dtype=torch.int64).to(DEV)
    put('store_bwd', *G.spmm_store_bwd(h, rs, bits, cs, 0.9, 0.5, 1234, 0))
    nq = N // 3
    pos = [torch.full((N,), -1, dtype=torch.int32), torch.full((N,), -1, dtype=torch.int32)]
    for q in range(2):
        idx = torch.randperm(N, generator=g)[:nq]
        pos[q][idx] = torch.arange(nq, dtype=torch.int32)
    mix = ([_rand(g, nq, 256), _rand(g, nq, 256)], [p.to(DEV) for p in pos], [11, 12], 0.1, True)
    put('store_bwd_mix', *G.spmm_store_bwd(h, rs, bits, cs, 0.9, 0.5, 1234, 0, mix=mix))
    put('store_bwd_mix1', *G.spmm_store_bwd(h, rs, bits, cs, 0.9, 0.0, 1234, 0, mix=(mix[0][:1], mix[1][:1], [11], 0.1, False)))
    # aggregation + GEMM, plain forms
    img = weight_image(_rand(g, 256, 256, scale=1 / 16))
    put('spmm_gemm', *G.spmm_gemm(h, img, row_scale=rs, bias=b, relu=True, g_rowscale=cs, g_addend=acc))
    put('spmm_gemm_t', *G.spmm_gemm(h, img, transpose=True, row_scale=rs))
    put('spmm_gemm_acc', *G.spmm_gemm(h, img, row_scale=rs, acc_init=acc.clone()))
    # the SAGE layer, forward and backward, every mode
    Wn, Ws, bd = _rand(g, 256, 256, scale=1 / 16), _rand(g, 256, 256, scale=1 / 16), _rand(g, 256)
    for mode, s, ws in (('SAGE', ops.inv_indeg(G), Ws), ('WSAGE', None, Ws), ('GCN', None, None)):
        put(f'sage_fwd_{mode}', *ops.sage_layer_raw(G, h, Wn, ws, bd, s, relu=True, p=0.3, seed=77, want_agg=True, fused=True)[:2])
        put(f'sage_fwd_noagg_{mode}', ops.sage_layer_raw(G, h, Wn, ws, bd, s, fused=True)[0])
        put(f'sage_bwd_{mode}', *ops.sage_layer_raw(G, h, Wn, ws, None, s, backward=True, want_agg=True, fused=True)[:2])
        put(f'sage_bwd_noagg_{mode}', ops.sage_layer_raw(G, h, Wn, ws, None, s, backward=True, fused=True)[0])
    if flags_only:      # (the entries below take no flagged column ids; the model's graph gets its flags as this one did)
        from gnn_tail_generalization_amd import tuning
        keep_hot, tuning.T.hot_bytes = tuning.T.hot_bytes, _hot_bytes(N)
        try:
            _model_step(G, res, tag, flagged=True)
        finally:
            tuning.T.hot_bytes = keep_hot
        return
    # label propagation / the general propagation step, and the narrow-width kernel
    y0, hl = torch.rand(N, 40, generator=g).to(DEV), torch.rand(N, 40, generator=g).to(DEV)
    put('lp', G.spmm_lp(hl, rs, y0, 0.2, post_scale=cs), G.spmm_lp(hl, rs, y0, 0.2))
    fix = (torch.rand(N, generator=g) < 0.2).to(torch.uint8).to(DEV)
    put('prop', G.spmm_prop(hl, rs, y0, 1.0, clamp=None, fix_rows=fix, post_scale=cs), G.spmm_prop(hl, rs, y0, 0.2, clamp=(-0.5, 0.7)))
    for d in (3, 7, 12, 16):
        hn = _rand(g, N, d)
        put(f'narrow_d{d}', G.spmm(hn, row_scale=rs, bias=_rand(g, d), relu=True), G.spmm(hn))
    _model_step(G, res, tag)


def _model_step(G, res, tag, flagged=False):
    """The fused trunk on this graph: fused store forward and `bwd`, spmm_gemm fused / head / row-subset forms, the store backward with its mix — through the
    model, dense step, rows-only step and an evaluation forward; logits and every gradient."""
    import contextlib
    import io

    from gnn_tail_generalization_amd import ops, tuning
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.GNN_model import TeacherGNN
    from gnn_tail_generalization_amd.utils import set_arch_configs
    N = G.N
    with contextlib.redirect_stdout(io.StringIO()):
        a = BaseOptions().get_arguments(['--dataset=S-pl1M', '--num_layers=3', '--use_special_split=0', '--manual_assign_GPU=0'])
    a.N_nodes, a.dropout, a.device = N, 0.5, torch.device(DEV)
    set_arch_configs(a)
    g = torch.Generator().manual_seed(5)
    x = _rand(g, N, a.num_feats)
    y = torch.randint(0, a.num_classes, (N,), generator=g).to(DEV)
    mask = (torch.rand(N, generator=g) < 0.1).to(DEV)
    rp, col = G.rowptr.long(), G.col.long()[:G.E]
    loops = torch.arange(N, device=DEV)      # (the model refuses rows without in-edges: self-loops, as the reference advises)
    ei = torch.cat([torch.stack([col, torch.repeat_interleave(loops, rp[1:] - rp[:-1])]), torch.stack([loops, loops])], 1)
    torch.manual_seed(0)
    m = TeacherGNN(a).to(DEV)
    keep_min, tuning.T.rows_only_min_nodes = tuning.T.rows_only_min_nodes, 0
    try:
        for kind in ('dense', 'rows_only'):
            m.train()
            m.zero_grad(set_to_none=True)
            torch.manual_seed(99)      # (ops.next_seed draws the dropout seeds from torch's CPU generator)
            if kind == 'dense':
                out = m(x, ei)
                loss = ops.nll_logsoftmax(out, y, mask)
                logits = out
            else:
                m.model.model._graph(ei).rowsparse_small_ok = True      # (the row-sparse plan at this size too)
                r = m.get_3_embs(x, ei, mask, loss_rows=(mask, int(mask.sum())), rows_only=True)
                loss = ops.nll_logsoftmax(r.emb4classi, y[mask].contiguous(), None, int(mask.sum()))
                logits = r.emb4classi
            loss.backward()
            assert (m.model.model._graph(ei).col_k is not None) == flagged
            res[f'{tag}/model_{kind}/loss'] = loss.detach().cpu()
            res[f'{tag}/model_{kind}/logits'] = logits.detach().cpu()
            for k, p in m.named_parameters():
                if p.grad is not None:
                    res[f'{tag}/model_{kind}/grad/{k}'] = p.grad.detach().cpu()
        m.eval()
        with torch.no_grad():
            res[f'{tag}/model_eval/logits'] = m(x, ei).detach().cpu()
    finally:
        tuning.T.rows_only_min_nodes = keep_min


def dump(path, root):
    sys.path.insert(0, root)
    from gnn_tail_generalization_amd import _lib
    _lib.load()
    os.makedirs(path, exist_ok=True)
    for tag, G in _graphs().items():
        res = {}
        _entries(G, res, tag, tag.endswith('_flags'))
        torch.cuda.synchronize()
        _lib.device_status()
        print(f'{tag}: N = {G.N}, E = {G.E}, hubs = {G._plan.n_hubs} / {G._plan_t.n_hubs}, {len(res)} tensors', flush=True)
        torch.save(res, os.path.join(path, tag + '.pt'))      # (one file per graph: the 70 000-row outputs are gigabytes)


def compare(pa, pb):
    bad, groups = sorted(set(os.listdir(pa)) ^ set(os.listdir(pb))), {}
    for f in sorted(set(os.listdir(pa)) & set(os.listdir(pb))):
        bad += _compare_one(torch.load(os.path.join(pa, f)), torch.load(os.path.join(pb, f)), groups)
    print('| group | tensors | outcome |\n|---|---|---|')
    for grp, (n, ok) in groups.items():
        print(f'| `{grp}` | {n} | {"all equal" if ok else "DIFFERENT"} |')
    print(f'\n{sum(n for n, _ in groups.values())} tensors compared: ' + ('all equal' if not bad else f'{len(bad)} differ or are missing: {bad[:20]}'))
    return 1 if bad else 0


def _compare_one(a, b, groups):
    bad = sorted(set(a) ^ set(b))
    for k in sorted(set(a) & set(b)):
        x, y = a[k], b[k]
        nan = torch.isnan(x) if x.is_floating_point() else torch.zeros_like(x, dtype=torch.bool)
        nan_y = torch.isnan(y) if y.is_floating_point() else nan
        same = x.shape == y.shape and torch.equal(nan, nan_y) and torch.equal(torch.where(nan, torch.zeros_like(x), x), torch.where(nan, torch.zeros_like(y), y))
        grp = k.rsplit('/', 1)[0] if '/grad/' not in k else k.split('/grad/')[0] + '/grad'
        n, ok = groups.get(grp, (0, True))
        groups[grp] = (n + 1, ok and same)
        if not same:
            bad.append(k)
    return bad


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('cmd', choices=('dump', 'compare'))
    ap.add_argument('paths', nargs='+')
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    args = ap.parse_args()
    if args.cmd == 'dump':
        dump(args.paths[0], os.path.abspath(args.root))
    else:
        sys.exit(compare(*args.paths))
