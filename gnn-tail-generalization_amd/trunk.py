"""Fused residual trunk of TricksComb.forward for the 'Initial' and 'Residual' connections without a bare norm — the
configurations the reference's best-config table selects for Pubmed / ogbn-arxiv / chameleon / squirrel ('Initial…') and WISCONSIN /
CORNELL / TEXAS ('Residual…', base_options.py:416-421) and the benchmark graphs.  One autograd node for

    X0   = relu(Linear_0(dropout(x)))                                   GCN.py:103-107
    for l: X  = dropout(X);  Y = GCNConv_l(X);  A_l = relu(Y);  X = (1-a) A_l + a M_l      GCN.py:109-131
           M_l = X0 ('Initial', res_tricks.py:16-23)  |  M_0 = X0, M_l = A_{l-1} ('Residual', res_tricks.py:7-14: x_list holds the ReLU outputs)
    out  = Linear_1(dropout(X))                                          GCN.py:133-138

with the hand-written backward (kernels per stage: DESIGN.md section 3, "Fused nodes").  ReLU masks are kept as bits, dropout masks are regenerated, the
gradient w.r.t. X0 is gathered in one pass by the input stage.  Other widths, bf16-stored rows and node-sharded pull plans take the same node with one
kernel per stage.  Same arithmetic and the same sequence of dropout seeds as the modular path (ops.py), which stays the general fallback; every fused form
is bit-identical to the kernels it replaces (tests/test_gpu_agg_gemm.py, test_gpu_kernels.py, test_gpu_fullsize.py).  Under the caller's `loss_rows`
promise the backward (_Backward) runs on the rows that carry gradient, under `rows_only` as well a training forward (_Forward) evaluates its last layers on
the rows the loss reads (_rows_only_decision; DESIGN.md section 1, "Row-sparse backward" / "Rows-only training forward").

Environment switches, each read on every call through _switch (nothing is cached at import) — name = default:
    CB_AGG_GEMM = 1                 0: aggregation, then the next layer's GEMM, as two kernels (agg_gemm_eligible)
    CB_TRUNK_GATHER = unset         0 / 1: force the accumulate / gather mode of the gradients that reach X0 (_gather_fits)
    COLDBREW_CHUNKED_PRODUCERS = 1  0: no row-chunked producers in front of a sliced node-sharded exchange (_chunked)
    CB_ROWS_ONLY_FWD = 1            0: a training forward evaluates every row whatever the caller reads (rows_only_enabled)
    CB_ROWS_ONLY_BELOW = 2          the layer under a rows-only last layer: 0 all rows, 1 Z-first on S_1, 2 sum-first on S_1 (_rows_only_decision)
    CB_TRUNK_INDROP = 1             0: the dropout of the input features as a pass of its own (_Forward._front)
    CB_TRUNK_FRONT = 1              0: no forward-front kernel (_Forward._front)
    CB_TRUNK_X0_COPY = 1            0: the dropped copy of X0 is never stored, its mask is regenerated (_Forward._front)
    CB_INSTAGE_FOLD = 1             0: the input stage of the backward keeps a pass of its own (_Backward.__init__)
"""
import ctypes
import os
from typing import NamedTuple

import torch

from . import _lib, gemm, ops
from .graph import head_image, prof_rec, weight_image
from .tuning import T


def _switch(name, default):
    """The environment switch `name` (module docstring), read now: tests flip them between steps."""
    return os.environ.get(name, default)


TrunkCfg = NamedTuple('TrunkCfg', [('L', int), ('alpha', float), ('p', float), ('seeds', tuple), ('agg_bf16', bool), ('track', bool), ('loss_rows', object),
                                   ('residual', bool), ('rows_only', bool)])
TrunkCfg.__doc__ = """What one call of the trunk was asked for (second argument of _TrunkFn.apply).  L: number of GCNConv layers; alpha: weight of the mix
source in a layer's output (res_tricks.py); p: the one dropout rate (0 in evaluation); seeds: L + 2 dropout seeds (features, X0, one per layer); agg_bf16:
the gathered rows Z_l are stored as bf16; track: autograd was recording when the trunk was called (inside a Function's forward it never is, and
needs_input_grad does not know about no_grad); loss_rows: None or (bool mask [N], count), the caller's promise that the output receives gradient in those
rows only (ops.py); residual: the 'Residual' connection (mix source of layer l > 0 = the previous layer's ReLU output) instead of 'Initial' (X0);
rows_only: the second promise — the caller READS the output in the rows of loss_rows only (the others: ops.unread_rows_fill)."""


class RowsOnly(NamedTuple):
    """What a rows-only training forward evaluates on fewer rows (_rows_only_decision); None / False where not taken.
      plan    one GPU: the backward's row-support plan (the SAME decision, _support_plan) — the last layer, its store and the output Linear run on the loss
              rows S_0 (_last_layer_on_loss_rows), the backward's level 0 through the source rows' side on the saved aggregate (not with a table on it);
      below   graph.RowsOnlyFwd: ... and the layer below it on the rows the last layer reads, S_1, while the plan keeps that support compact ('Residual':
              its ReLU output, the last layer's mix source, lives there too).  CB_ROWS_ONLY_BELOW=0: that layer on all rows;
      sharded (space, orientation): row shards — the last layer on the rank's loss rows; the exchange ships only their in-neighbours;
      sum_first_below   the layer below takes its sum FIRST as well (L >= 3, no table on it, tuning.T.sum_first_below_min_edges): level 1 contracts the
              saved aggregate too, the layer under it loses its dense tail.  CB_ROWS_ONLY_BELOW=1: Z-first on S_1."""
    plan: object = None
    below: object = None
    sharded: object = None
    sum_first_below: bool = False


class SavedRows(NamedTuple):
    """ctx.saved_rows: where the forward left the last two inputs the backward keeps.  x_last = saved_in[L], the head's input: 'all' | 'S0' (the loss rows).
    x_below = saved_in[L - 1], the last layer's input: 'all' | 'S1' (the rows the last layer reads: level 0's destination) | 'absent' (not kept: that
    layer's weight gradient contracts the saved aggregate h_last instead)."""
    x_last: str = 'all'
    x_below: str = 'all'


def _layers(layer_params):
    """[(W_l, bias_l, le_l | None)] of the flat (W_0, bias_0, le_0 | None, W_1, ...) that the autograd nodes take (needs_input_grad indexes it)."""
    return [tuple(layer_params[i:i + 3]) for i in range(0, len(layer_params), 3)]


def _save(ctx, **named):
    """Keeps tensors for the backward under names (a tensor, a list of tensors, None in either place): ONE ctx.save_for_backward with those that are there, in
    the order given; ctx.saved_layout records which.  The trunk's order: xd, x0, w_in, w_out, saved_in, saved_bits, layer_params, h_last, h_below, x0_bits."""
    many = {k: isinstance(v, (list, tuple)) for k, v in named.items()}
    ctx.save_for_backward(*[t for k, v in named.items() for t in (v if many[k] else [v]) if t is not None])
    ctx.saved_layout = [(k, [t is not None for t in v] if many[k] else v is not None) for k, v in named.items()]


def _saved(ctx):
    """{name: what _save was given}: the kept tensors by name, None where there was none."""
    it = iter(ctx.saved_tensors)
    return {name: [next(it) if q else None for q in here] if isinstance(here, list) else (next(it) if here else None)
            for name, here in ctx.saved_layout}


def _dw_regen(x, gz, p, seed, row0, rowscale):
    """X^T (rowscale * dZ) with X = dropout(x): the mask of `seed` is regenerated from the undropped x while the GEMM stages it (cb_gemm_tn_adrop_f32),
    else by a dropout pass in front of the plain GEMM."""
    dw = gemm.mm_tn_adrop(x, gz, p, seed, row0, rowscale=rowscale)
    return dw if dw is not None else gemm.mm_tn(ops._dropout_raw(x, p, seed, row0 * x.shape[1]), gz, rowscale=rowscale)


def _collect_layer_params(tc, graph):
    """(flat layer_params, se_reg_all) of TricksComb's GCNConv layers; sets each table's se_norm (row shards: the norm is over all ranks' rows)."""
    params, se_reg_all = [], None
    for conv in tc.layers_GCN:
        le = conv.le if conv.whetherHasSE else None
        params += [conv.weight, conv.bias, le]
        if le is not None:
            reg = ops.frobenius_norm(le)
            if hasattr(graph, 'part'):
                from .dist import allreduce_sum
                reg = allreduce_sum(reg * reg, graph.group).sqrt()
            conv.se_norm = reg.detach()
            se_reg_all = reg if se_reg_all is None else se_reg_all + reg
    if not all(c._allow_zero_in_degree for c in tc.layers_GCN):      # GCN.py:187-197; set_allow_zero_in_degree(True) lifts it
        graph.check_zero_in_degree()
    return params, se_reg_all


def connection(tc):
    """'residual' | 'initial' | None: which mix TricksComb builds for this type_trick (GCN.py:57-60: 'Residual' is tested first)."""
    t = tc.type_trick
    return 'residual' if 'Residual' in t else 'initial' if 'Initial' in t else None


def eligible(tc, x, want_les):
    t = tc.type_trick
    return (tc.has_residual_MLP and connection(tc) is not None and 'Jumping' not in t and not want_les
            and tc.args.type_trick not in ('BatchNorm', 'PairNorm', 'NodeNorm', 'MeanNorm', 'GroupNorm', 'CombNorm')
            and tc.dim_hidden % 256 == 0 and x.is_cuda and x.dtype == torch.float32 and len(tc.layers_GCN) == tc.num_layers
            and len(tc.layers_MLP) == 2
            # one dropout rate everywhere (else the modular path, which takes the rates one by one)
            and tc.embedding_dropout == tc.dropout and tc.args.dropout == tc.dropout)


def _exchanged(graph, n_rows, d=256):
    """An [n_rows, d] fp32 matrix the next aggregation of `graph` will exchange: node-sharded, with room behind it for the first halo slice
    (dist.alloc_exchanged: the interior pass and the first halo pass then are one); otherwise a plain matrix."""
    if hasattr(graph, 'part'):
        from .dist import alloc_exchanged
        return alloc_exchanged(graph, n_rows, d)
    return torch.empty((n_rows, d), dtype=torch.float32, device=graph.norm_in.device)


def _fused_spmm(graph, z, bias, x0, c_act, c_mix, p, seed, want_act=False, produce=None, want_bits=True, relu_only=False):
    """(bits, out_next[, act]) of cb_spmm_csr_fused_f32 on the (possibly node-sharded) graph.  Node-sharded + overlapped: the exchange runs as the sliced
    pipeline of dist.ShardedGraph (produce(k, r0, r1), if given, fills rows [r0, r1) of z — the row-chunked layer GEMM — right before slice k is packed and
    sent); the interior-column pass (plain kernel, raw sums) and the halo passes of the earlier slices run while the later slices travel, the fused store is
    the last slice's pass (cb_spmm_csr_fused_f32 with acc_init; over bf16 rows when the halo rows crossed the links as bf16)."""
    lib = _lib.load()
    sh = graph if hasattr(graph, 'part') else None
    if sh is not None and sh.overlap and z.dtype == torch.float32:
        flights = sh.start_halo(z, False, produce)
        return sh.finish_halo(flights, sh.f, None, lambda g, recv, a_: _fused_launch(
            lib, graph, g, recv, a_, bias, x0, c_act, c_mix, p, seed, want_act, want_bits, relu_only), x_local=z)
    if produce is not None:
        produce(0, 0, z.shape[0])
    if sh is None:
        return _fused_launch(lib, graph, graph, z, None, bias, x0, c_act, c_mix, p, seed, want_act, want_bits, relu_only)
    return _fused_launch(lib, graph, sh.f.whole, sh.exchange(z, False), None, bias, x0, c_act, c_mix, p, seed, want_act, want_bits, relu_only)


def _fused_gemm_launch(graph, z, bias, x0, c_act, c_mix, p, seed, image, g_rowscale, g_addend, want_bits=True, g=None, acc=None, want_act=False,
                       relu_only=False, head=None):
    """(bits, out_next, z_next[, act]) of cb_spmm_gemm_fused_f32: the fused trunk store of layer l and Z_{l+1} = g_rowscale * (out_next @ W_{l+1}) + g_addend
    from one kernel (d = 256, fp32 rows).  g: the CSR to run on (default: the graph itself; node-sharded: the last halo slice, z = its receive buffer) with
    acc = the running sums of the earlier passes.  want_bits=False (a forward that no backward follows): the entry's skip_next — no mask words, and out_next
    is not written either (it has no reader: returned as None).  want_act: a fourth result, the ReLU output A_l itself (the next 'Residual' layer's mix
    source); relu_only: mask words of A_l > 0 alone.  head = (b_out, C) (the LAST layer; image = graph.head_image(w_out)): the tail is the output Linear — the
    third result is the logits [N, C] (cb_spmm_gemm_fused_head_f32, GCN.py:133-138), g_rowscale / g_addend are ignored."""
    lib = _lib.load()
    g = graph if g is None else g
    fn = lib.cb_spmm_gemm_fused_head_f32 if head is not None else lib.cb_spmm_gemm_fused_f32
    n, d = g.N, z.shape[1]
    dev = z.device
    bits = torch.empty((n, d // 256, 4), dtype=torch.int64, device=dev) if want_bits else None
    # (the evaluation form keeps the finished rows on chip: X_{l+1} goes to memory only as the hub rows' way into the tile)
    out_next = torch.empty((n, d), dtype=torch.float32, device=dev) if (want_bits or g._plan.n_hubs > 0) else None
    # (Z_{l+1}: the next aggregation exchanges it | the logits)
    z_next = _exchanged(graph, n) if head is None else torch.empty((n, int(head[1])), dtype=torch.float32, device=dev)
    act = torch.empty((n, d), dtype=torch.float32, device=dev) if want_act else None
    prof = getattr(graph, 'profile', None)
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    if g_addend is not None and g_addend.stride(1) != 1:
        g_addend = g_addend.contiguous()
    with torch.cuda.device(dev):
        _lib.check(fn(g._view(d, use_flags=True), _lib.ptr(acc), acc.stride(0) if acc is not None else 0,
                      _lib.ptr(z), z.stride(0), d, _lib.ptr(graph.norm_in), _lib.ptr(bias),
                      ops.store_args(x0, None, c_act, c_mix, p, seed, getattr(graph, 'row_offset', 0), bits, relu_only, act),
                      _lib.ptr(out_next), d, int(not want_bits), _lib.ptr(image),
                      *((_lib.ptr(head[0]), int(head[1])) if head is not None
                        else (_lib.ptr(g_rowscale), _lib.ptr(g_addend), g_addend.stride(0) if g_addend is not None else 0)),
                      _lib.ptr(z_next), z_next.stride(0), _lib.stream_ptr()),
                   'cb_spmm_gemm_fused_f32')
    if prof is not None:
        ev1.record()
        # (the evaluation form writes neither the mask words nor X_{l+1}: 8(d)'s output stream is not there, its rows stay on chip)
        prof.append(prof_rec(ev0, ev1, g, ('agg_gemm_head' if head is not None else 'agg_gemm_fused') + ('' if want_bits else '_eval'),
                             g.algorithmic_bytes(d) - (0 if want_bits else n * d * 4), n * d * 4 + (n * d // 8 if want_bits else 0),
                             (n * int(head[1]) * 4) if head is not None
                             else n * 256 * 4 * (2 if g_addend is not None else 1) + (4 * n if g_rowscale is not None else 0)))
    res = (bits, out_next if want_bits else None, z_next)
    return res + (act,) if want_act else res


def _fused_gemm(graph, z, bias, x0, c_act, c_mix, p, seed, image, g_rowscale, g_addend, want_bits=True, want_act=False, relu_only=False, head=None):
    """_fused_gemm_launch on the (possibly node-sharded) graph: sharded, the exchange of z runs as the sliced pipeline of dist.ShardedGraph (pack / push-sum,
    all-to-all, interior pass, halo passes of the earlier slices) and the LAST halo pass is the fused kernel on top of the running sums — the rank's last pass
    over its rows also yields the next layer's Z, so no GEMM stands between this aggregation and the next layer's first send."""
    if not hasattr(graph, 'part'):
        return _fused_gemm_launch(graph, z, bias, x0, c_act, c_mix, p, seed, image, g_rowscale, g_addend, want_bits, want_act=want_act,
                                  relu_only=relu_only, head=head)
    sh = graph
    flights = sh.start_halo(z, False)
    return sh.finish_halo(flights, sh.f, None, lambda g, recv, a_: _fused_gemm_launch(
        graph, recv, bias, x0, c_act, c_mix, p, seed, image, g_rowscale, g_addend, want_bits, g=g, acc=a_, want_act=want_act, relu_only=relu_only,
        head=head), x_local=z)


def head_tail_enabled(bwd):
    """The output Linear as the tail of the last layer's aggregation (cb_spmm_gemm_fused_head_f32): in forwards that no backward follows, where the last
    layer's activations are then not written at all.  A training forward must store them anyway and keeps two kernels (HISTORY.md)."""
    return not bwd


def agg_gemm_eligible(graph, hidden, agg_bf16):
    """The aggregation + next-dense-transform kernels (cb_agg_gemm.hip): hidden = 256, fp32 rows; one GPU, or node-sharded with the overlapped halo exchange
    on the fp32 wire under a push / pull cover plan or an unsliced pull plan (the last halo pass is then the fused kernel on top of the running sums).
    CB_AGG_GEMM=0 keeps the two-kernel form (aggregation, then GEMM)."""
    if _switch('CB_AGG_GEMM', '1') == '0' or hidden != 256 or agg_bf16:
        return False
    if hasattr(graph, 'part'):
        # (with the pull plan cut by owner row chunks the row-chunked producers win instead: profiles/r04_shard_probe_S-products.txt)
        plan = graph.f.plan
        return bool(graph.overlap) and graph.wire == 'f32' and plan is not None and (plan.cover or plan.n_slices == 1)
    return hasattr(graph, 'spmm_gemm')


def _fused_launch(lib, graph, g, z, acc, bias, x0, c_act, c_mix, p, seed, want_act, want_bits=True, relu_only=False, row_ids=None, row_scale=None):
    """One fused-store launch over CSR g (the whole graph, a rank's single-pass block, or the last halo slice on top of acc).
    want_bits=False (forward without a backward: eval / metrics forwards): the backward's mask words are not written.
    row_ids (int32 [g.N], with row_scale = norm_in on those rows): g's rows are a subset of the node rows (the entry's row_ids) — out_next is
    compact, x0 / the mask words / the dropout mask are taken at the node row (the mask words of the other rows are not written)."""
    n, d = g.N, z.shape[1]
    dev = z.device
    bits = torch.empty((n if row_ids is None else graph.N, d // 256, 4), dtype=torch.int64, device=dev) if want_bits else None
    out_next = torch.empty((n, d), dtype=torch.float32, device=dev)
    act = torch.empty((n, d), dtype=torch.float32, device=dev) if want_act else None
    prof = getattr(graph, 'profile', None)
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    bf16 = z.dtype == torch.bfloat16
    with torch.cuda.device(dev):
        _lib.check(lib.cb_spmm_csr_fused_f32(g._view(d, use_flags=True, elem=z.element_size()), _lib.ptr(row_ids), _lib.ptr(z), int(bf16), z.stride(0), d,
                                             _lib.ptr(graph.norm_in if row_scale is None else row_scale), _lib.ptr(bias), _lib.ptr(acc),
                                             d if acc is not None else 0,
                                             ops.store_args(x0, None, c_act, c_mix, p, seed, getattr(graph, 'row_offset', 0), bits, relu_only, act),
                                             _lib.ptr(out_next), d, _lib.stream_ptr()), 'cb_spmm_csr_fused_f32')
    if prof is not None:
        ev1.record()
        # SURVEY §8(d) bytes of the aggregation; the fused store's own streams (mixed-in row read + mask bits) are kept apart
        prof.append(prof_rec(ev0, ev1, g, 'fused_store', g.algorithmic_bytes(d, src_elem=2 if bf16 else 4), n * d * 4 + (n * d // 8 if want_bits else 0)))
    return bits, out_next, act


def _spmm_t(graph, gr):
    if hasattr(graph, 'part'):
        return graph.aggregate(gr, True)
    return graph.spmm(gr, transpose=True)


def _colsum_ws(lib, rows, d, device, want=True):
    """(colsum [d], its workspace, the workspace's size in bytes) for the column sums of a [rows, d] pass; (None, a 16-byte buffer, 0) if not wanted."""
    colsum = torch.empty(d, dtype=torch.float32, device=device) if want else None
    wsb = lib.cb_colsum_workspace_bytes(rows, d) if want else 0
    return colsum, torch.empty(max(wsb, 16), dtype=torch.uint8, device=device), wsb


def _layer_bwd_fold(g, bits, row_scale, p, seed, row0, c_act, c_mix, want_colsum, mix_g, mix_pos, mix_seeds, out=None, cs=None):
    """cb_trunk_layer_bwd_fold_f32: layer 0's store backward on all rows that also folds the mix gradients — (b * dY', dbias, m) with
    m = c_mix * (dropout_bwd(g) + sum_q dropout_bwd_q(mix_g[q])); mix_pos[q]: None for a dense operand, else its int32 position map.
    cs = (index into mix_g, mask words, factor): a fourth result — the column sums of factor * dropout_bwd(mix_g[index]) through those mask words (the bias
    gradient of a store whose backward left a reverse aggregation's epilogue)."""
    lib = _lib.load()
    rows, d = g.shape
    if out is None:
        out = torch.empty_like(g)
    m = torch.empty_like(g)
    colsum, ws, wsb = _colsum_ws(lib, rows, d, g.device, want_colsum)
    k = len(mix_g)
    colsum2, ws2, ws2b = _colsum_ws(lib, rows, d, g.device) if cs is not None else (None, None, 0)
    with torch.cuda.device(g.device):
        _lib.check(lib.cb_trunk_layer_bwd_fold_f32(_lib.ptr(g), _lib.ptr(bits), _lib.ptr(row_scale), _lib.ptr(out), rows, d, float(p), ctypes.c_uint64(seed),
                                                   ops.seed_dev_ptr(), int(row0), float(c_act), float(c_mix), k,
                                                   (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in mix_g]),
                                                   (ctypes.c_void_p * max(k, 1))(*[(q.data_ptr() if q is not None else None) for q in mix_pos]),
                                                   (ctypes.c_uint64 * max(k, 1))(*[int(s_) for s_ in mix_seeds]), _lib.ptr(m), _lib.ptr(colsum),
                                                   _lib.ptr(ws), wsb,
                                                   int(cs[0]) if cs is not None else -1, _lib.ptr(cs[1]) if cs is not None else None,
                                                   float(cs[2]) if cs is not None else 0.0, _lib.ptr(colsum2), _lib.ptr(ws2), ws2b,
                                                   _lib.stream_ptr()), 'cb_trunk_layer_bwd_fold_f32')
    if cs is not None:
        return out, colsum, m, colsum2
    return out, colsum, m


def _layer_bwd(g, bits, row_scale, gx0, accumulate, p, seed, row0, c_act, c_mix, want_colsum, out_bf16=False, out=None, g2=None, seed2=0, c2=0.0, g2_pos=None):
    """cb_trunk_layer_bwd_f32: (b * dY' of the layer's store, dbias).  g2 ('Residual'): the gradient w.r.t. the NEXT layer's stored output, which
    reaches this layer's ReLU output through that layer's mix (c2 = alpha) under that layer's dropout mask (seed2); g2_pos (int32 [rows]): g2 is
    a compact matrix of a row-sparse backward, row r at g2_pos[r] (absent where negative)."""
    lib = _lib.load()
    rows, d = g.shape
    if out is None:
        out = torch.empty(g.shape, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=g.device)
    colsum, ws, wsb = _colsum_ws(lib, rows, d, g.device, want_colsum)
    with torch.cuda.device(g.device):
        _lib.check(lib.cb_trunk_layer_bwd_f32(_lib.ptr(g), _lib.ptr(bits), _lib.ptr(row_scale), _lib.ptr(out), int(out_bf16),
                                              _lib.ptr(gx0), int(accumulate), rows, d, float(p), ctypes.c_uint64(seed), ops.seed_dev_ptr(),
                                              int(row0), float(c_act), float(c_mix), _lib.ptr(g2), ctypes.c_uint64(seed2), float(c2), _lib.ptr(g2_pos),
                                              _lib.ptr(colsum), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                   'cb_trunk_layer_bwd_f32')
    return out, colsum


def _layer_bwd_rows(g_c, rows_idx, bits, row_scale, p, seed, row0, c_act, want_colsum, out=None, g2=None, seed2=0, c2=0.0, g2_pos=None):
    """_layer_bwd over the compact rows rows_idx of a row-sparse backward (cb_trunk_layer_bwd_rows_f32): (b * dY' of those rows, dbias)."""
    lib = _lib.load()
    n_c, d = g_c.shape
    out = torch.empty_like(g_c) if out is None else out
    colsum, ws, wsb = _colsum_ws(lib, n_c, d, g_c.device, want_colsum)
    with torch.cuda.device(g_c.device):
        _lib.check(lib.cb_trunk_layer_bwd_rows_f32(_lib.ptr(g_c), _lib.ptr(rows_idx), n_c, _lib.ptr(bits), _lib.ptr(row_scale), _lib.ptr(out), d, float(p),
                                                   ctypes.c_uint64(seed), ops.seed_dev_ptr(), int(row0), float(c_act), _lib.ptr(g2), ctypes.c_uint64(seed2),
                                                   float(c2), _lib.ptr(g2_pos), _lib.ptr(colsum), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                   'cb_trunk_layer_bwd_rows_f32')
    return out, colsum


def _input_bwd(g, add, act, p, seed, row0):
    lib = _lib.load()
    rows, d = g.shape
    out = torch.empty_like(g)
    colsum, ws, wsb = _colsum_ws(lib, rows, d, g.device)
    with torch.cuda.device(g.device):
        _lib.check(lib.cb_trunk_input_bwd_f32(_lib.ptr(g), _lib.ptr(add), _lib.ptr(act), _lib.ptr(out), rows, d, float(p),
                                              ctypes.c_uint64(seed), ops.seed_dev_ptr(), int(row0), _lib.ptr(colsum), _lib.ptr(ws), wsb,
                                              _lib.stream_ptr()), 'cb_trunk_input_bwd_f32')
    return out, colsum


def _input_bwd_multi(g, seed, g_mix, seeds_mix, c_mix, act, p, row0, act_bits=None, mix_pos=None, cs=None):
    """cb_trunk_input_bwd_multi_f32: (dropout_bwd(g) + c_mix * sum_l dropout_bwd_l(g_mix[l])) * (act > 0) and its column sums.
    act_bits: int64 [rows, d/256, 4] mask words of (act > 0), read instead of act.  mix_pos (list, entries None or int32 [rows]): where set,
    g_mix[l] is a compact matrix of the rows with mix_pos[l] >= 0 (support rows of a row-sparse backward); its other rows are zero.
    cs = list of up to two (index into g_mix, mask words, factor): a third result — per entry the column sums of factor * dropout_bwd(g_mix[index]) through
    those mask words, the bias gradient of a store whose backward left the reverse aggregation's epilogue (cb_trunk_input_bwd_multi_cs_f32)."""
    lib = _lib.load()
    rows, d = g.shape
    out = torch.empty_like(g)
    colsum, ws, wsb = _colsum_ws(lib, rows, d, g.device)
    n = len(g_mix)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in g_mix])
    seeds = (ctypes.c_uint64 * max(n, 1))(*[int(s) for s in seeds_mix])
    pos = None
    if mix_pos is not None and any(q is not None for q in mix_pos):
        pos = (ctypes.c_void_p * max(n, 1))(*[(q.data_ptr() if q is not None else None) for q in mix_pos])
    with torch.cuda.device(g.device):
        if cs:
            k = len(cs)
            colsum2 = [torch.empty(d, dtype=torch.float32, device=g.device) for _ in range(k)]
            ws2 = torch.empty(max(k * wsb, 16), dtype=torch.uint8, device=g.device)
            _lib.check(lib.cb_trunk_input_bwd_multi_cs_f32(_lib.ptr(g), ctypes.c_uint64(seed), n, ptrs, seeds, float(c_mix),
                                                           _lib.ptr(None if act_bits is not None else act), _lib.ptr(out), rows, d, float(p),
                                                           ops.seed_dev_ptr(), int(row0), _lib.ptr(colsum), _lib.ptr(ws), wsb,
                                                           _lib.ptr(act_bits), pos, k, (ctypes.c_int32 * k)(*[int(c[0]) for c in cs]),
                                                           (ctypes.c_void_p * k)(*[c[1].data_ptr() for c in cs]),
                                                           (ctypes.c_float * k)(*[float(c[2]) for c in cs]),
                                                           (ctypes.c_void_p * k)(*[t.data_ptr() for t in colsum2]), _lib.ptr(ws2), k * wsb, _lib.stream_ptr()),
                       'cb_trunk_input_bwd_multi_cs_f32')
            return out, colsum, colsum2
        _lib.check(lib.cb_trunk_input_bwd_multi_f32(_lib.ptr(g), ctypes.c_uint64(seed), n, ptrs, seeds, float(c_mix),
                                                    _lib.ptr(None if act_bits is not None else act), _lib.ptr(out), rows, d, float(p),
                                                    ops.seed_dev_ptr(), int(row0), _lib.ptr(colsum), _lib.ptr(ws), wsb,
                                                    _lib.ptr(act_bits), pos, _lib.stream_ptr()), 'cb_trunk_input_bwd_multi_f32')
    return out, colsum


_GATHER_OK = {}


def _gather_fits(L, x0, graph=None):
    """Gather mode keeps every layer's [N, d] gradient alive until the input stage: (L - 1) * N * d * 4 bytes more than accumulating layer by layer.  Allowed
    while that stays below a quarter of the device memory free at the first backward of this shape (decided once per shape: no driver query per step).
    Node-sharded: ONE decision for the group (all-reduce MIN), so that every rank runs the same backward.  CB_TRUNK_GATHER=0/1 forces it."""
    key = (L, tuple(x0.shape), x0.device.index)
    ok = _GATHER_OK.get(key)
    if ok is None:
        env = _switch('CB_TRUNK_GATHER', None)
        if env in ('0', '1'):
            ok = env == '1'
        else:
            free, _total = torch.cuda.mem_get_info(x0.device)
            ok = (L - 1) * x0.numel() * 4 <= T.gather_mem_frac * free
        if graph is not None and hasattr(graph, 'part') and graph.part.world > 1:
            from .dist import _all_reduce
            import torch.distributed as dist
            flag = torch.tensor([int(ok)], dtype=torch.int64, device=x0.device)
            _all_reduce(flag, op=dist.ReduceOp.MIN, group=graph.group)
            ok = bool(int(flag.item()))
        _GATHER_OK[key] = ok
    return ok


def _chunked(graph, agg_bf16):
    """Row-chunk the producers of the exchanged matrices (layer GEMM forward; dX GEMM + trunk layer backward) so that chunk k
    ships while chunk k+1 is computed: node-sharded overlapped graphs whose plans are cut by owner row chunk into more than one slice
    (the pull-only plan, COLDBREW_HALO_COVER=0, without the aggregation + GEMM kernels)."""
    return (hasattr(graph, 'part') and graph.overlap and not agg_bf16 and graph.f.plan is not None and graph.f.plan.n_slices > 1
            and not graph.f.plan.cover and _switch('COLDBREW_CHUNKED_PRODUCERS', '1') != '0')


def _gather(graph, L, residual, x0):
    """Gather mode of a backward's gradients that reach X0 through the mixes."""
    return residual or (L <= T.mix_max and _gather_fits(L, x0, graph))


def _support_plan(graph, loss_rows, n_rows, L, residual, h, x0, committed=False):
    """The row-support plan of a backward — and of a rows-only forward — under the caller's loss_rows promise: ONE decision for both, so that a forward that
    evaluated its last layer on the loss rows finds the same plan in its backward.  plan: CSRGraph.grad_support_plan or None (dense).  committed (the backward
    of a rows-only forward): the plan's build / hit bookkeeping (support_plan_pays) is not asked again — the forward's own build may just have tipped it."""
    gather = _gather(graph, L, residual, x0)
    hint = loss_rows if (not hasattr(graph, 'part') and hasattr(graph, 'grad_support_plan') and graph.rowptr_t is not None) else None
    if hint is not None and (not ops.loss_rows_enabled() or hint[0].shape[0] != n_rows):
        hint = None
    if not (hint is not None and 1 <= hint[1] <= T.rowsparse_s0_limit * n_rows
            and (n_rows >= T.rowsparse_min_nodes or getattr(graph, 'rowsparse_small_ok', False)) and gather
            and agg_gemm_eligible(graph, h, False) and (committed or graph.support_plan_pays())):
        return None
    return hint


def rows_only_enabled():
    """CB_ROWS_ONLY_FWD=0: the training forward evaluates every row of every layer even when the caller reads the loss rows only."""
    return _switch('CB_ROWS_ONLY_FWD', '1') != '0'


def _rows_only_decision(graph, cfg, x, x0, h, ag, bwd, layer_params):
    """RowsOnly: what a training forward under both promises of the caller (gradient AND reads in the loss rows only) evaluates on fewer rows."""
    L, agg_bf16, loss_rows, residual = cfg.L, cfg.agg_bf16, cfg.loss_rows, cfg.residual
    none = RowsOnly()
    sharded = hasattr(graph, 'part')
    # (bf16-stored rows, one GPU: the last layer alone — its sum is taken over the fp32 activations, the layers below keep their bf16-stored Z)
    bf16_last_only = bool(agg_bf16) and not sharded and agg_gemm_eligible(graph, h, False)
    if not (cfg.rows_only and bwd and loss_rows is not None and L >= 2 and (ag or bf16_last_only) and rows_only_enabled()
            and (sharded or x.shape[0] >= T.rows_only_min_nodes)):
        return none
    if sharded:
        if not (hasattr(graph, 'loss_rows_forward') and ops.loss_rows_enabled() and loss_rows[0].shape[0] == x.shape[0]):
            return none
        gather = _gather(graph, L, residual, x0)
        levels = graph.support_levels(loss_rows[0], L, compact=ag and gather, cumulative=residual)
        if not (levels and levels[0].src is not None):
            return none
        return RowsOnly(sharded=(levels[0].src, graph.loss_rows_forward(levels)))
    if not T.rowsparse_loss_side:
        return none
    hint = _support_plan(graph, loss_rows, x.shape[0], L, residual, h, x0)
    if hint is None:
        return none
    plan = graph.grad_support_plan(hint[0], L, max_frac=T.rowsparse_max_frac, cumulative=residual)
    mode = '0' if bf16_last_only else _switch('CB_ROWS_ONLY_BELOW', '2')
    below = graph.rows_only_fwd(plan) if mode != '0' else None
    sum_first = (below is not None and mode == '2' and L >= 3 and _layers(layer_params)[L - 2][2] is None and len(plan.levels) >= 2
                 and below.fwd1.E >= T.sum_first_below_min_edges)
    return RowsOnly(plan, below, None, sum_first)


def _store_rows(y, idx, mix, c_act, c_mix, p, seed, row0, bits, relu_only, mix_index=None, want_act=False):
    """cb_trunk_store_rows_f32: the trunk's fused store (ReLU, mask words, mix, dropout) on the compact rows idx of a dense transform's output.
    mix_index: the rows of `mix` to read when that is a compact matrix itself (default: the node rows idx).  Returns (stored rows, ReLU output | None)."""
    lib = _lib.load()
    out = torch.empty_like(y)
    act = torch.empty_like(y) if want_act else None
    with torch.cuda.device(y.device):
        _lib.check(lib.cb_trunk_store_rows_f32(_lib.ptr(y), _lib.ptr(idx), y.shape[0], y.shape[1],
                                               ops.store_args(mix, mix_index, c_act, c_mix, p, seed, row0, bits, relu_only, act), _lib.ptr(out),
                                               _lib.stream_ptr()), 'cb_trunk_store_rows_f32')
    return out, act


def _layer_on_rows(graph, space, fwd, col_scale, cur, w, b, mix, mix_index, alpha, p, seed, row0, residual, want_act=False, le=None, fwd_le=None):
    """One GCNConv + store on the rows of `space` with the sum taken FIRST: H = (A (a * X))[space] over the forward orientation `fwd` restricted to
    those rows (col_scale = a on fwd's source space), Y = b * (H W) + bias on |space| rows, then the store on those rows.  le (a structural-embedding
    table on all node rows, GCN.py:230-232: Z = a * (X W) + le): its rows are summed the same way, Y = b * (H W + (A le)[space]) + bias, over fwd_le —
    the same orientation with node-row sources.  Returns (mask words [N, d/256, 4] with the rows of `space` written, stored rows, ReLU output | None, H)."""
    fwd.profile = getattr(graph, 'profile', None)
    b_rows = space.norm_in_of(graph)
    bits = torch.empty((graph.N, w.shape[1] // 256, 4), dtype=torch.int64, device=cur.device)
    if (le is None and tuple(w.shape) == (256, 256) and hasattr(fwd, 'spmm_gemm_store_rows') and fwd.E >= T.agg_gemm_store_rows_min_edges
            and agg_gemm_eligible(graph, 256, False)):
        # the three in one kernel (cb_spmm_gemm_store_rows_f32): the transform and the store run on the matrix cores under the gathers, H is not re-read
        h_agg, x_next, act = fwd.spmm_gemm_store_rows(cur, col_scale, weight_image(w), b_rows, b, space.idx, mix, mix_index, 1 - alpha, alpha, p, seed,
                                                      row0, bits, residual, want_act)
        return bits, x_next, act, h_agg
    h_agg = fwd.spmm(cur, col_scale=col_scale)
    le_sum = None
    if le is not None:
        fwd_le.profile = fwd.profile
        le_sum = fwd_le.spmm(le, row_scale=b_rows)
    # the store as the epilogue of the transform where that form exists (hidden 256), else the transform and then the elementwise pass: same values
    fused = gemm.mm_nn_store_rows(h_agg, w, b_rows, le_sum, b, space.idx, mix, mix_index, 1 - alpha, alpha, p, seed, row0, bits, residual, want_act)
    if fused is not None:
        return bits, fused[0], fused[1], h_agg
    y = gemm.mm_nn(h_agg, w, rowscale=b_rows, addend=le_sum, bias=b)
    del le_sum
    x_next, act = _store_rows(y, space.idx, mix, 1 - alpha, alpha, p, seed, row0, bits, residual, mix_index, want_act)
    return bits, x_next, act, h_agg


def _last_layer_on_loss_rows(graph, plan, cur, w, b, mix, alpha, p, seed, row0, residual, w_out, b_out, below=None, le=None):
    """The LAST GCNConv, its store and the output Linear on the loss rows S_0 only (rows-only forward): aggregation and transform commute,
        Y[S_0] = b * ((A (a * X))[S_0] W) + bias        (GCN.py:213-256 with the sum taken first)
    so the layer is one aggregation over the edges that ENTER the loss rows into a compact [|S_0|, H] matrix, a GEMM, the store and the head on |S_0| rows;
    Z_{L-1} — the previous layer's dense tail — is never formed.  Returns (mask words [N, H/256, 4] (rows of S_0 written), dropped X_L on S_0, logits [N, C]
    with ops.unread_rows_fill() (NaN) outside S_0, H = (A (a * X))[S_0]: the operand of the level's weight gradient in the backward's source-side form).
    below (CSRGraph.rows_only_fwd): `cur` holds the rows of S_1 only."""
    sp = plan.space0
    fwd0 = graph.loss_rows_fwd(plan) if below is None else below.fwd0c
    mix_index = None
    if below is not None and residual:      # the mix source (the layer below's ReLU output) lives on S_1 too: the loss rows' positions in it
        mix_index = getattr(plan, '_pos0_in_1', None)
        if mix_index is None:
            mix_index = plan._pos0_in_1 = below.s1.pos[sp.idx].long().contiguous()
    bits, x_l, _act, h_agg = _layer_on_rows(graph, sp, fwd0, graph.norm_out if below is None else below.s1.a, cur, w, b, mix, mix_index, alpha, p, seed, row0,
                                           residual, le=le, fwd_le=graph.loss_rows_fwd(plan) if le is not None else None)
    n = graph.N
    logits_c = gemm.mm_nn(x_l, w_out.t().contiguous(), bias=b_out)
    out = ops.expand_unread(logits_c, sp, n)      # the rows nobody may read: NaN (ops.unread_rows_fill)
    graph.rows_only_forwards = getattr(graph, 'rows_only_forwards', 0) + 1
    return bits, x_l, (out, logits_c), h_agg


def _last_layer_on_loss_rows_sharded(graph, s0, orient, cur, w, b, mix, alpha, p, seed, row0, residual, w_out, b_out, le=None):
    """_last_layer_on_loss_rows on a rank's row block: the aggregation of a * X over the edges that enter the rank's loss rows is a level orientation
    of the forward exchange (dist.ShardedGraph.loss_rows_forward: the peers ship only the in-neighbours of those rows).  Returns (mask words, dropped
    X_L on the rank's loss rows, logits [n_local, C] with ops.unread_rows_fill() (NaN) elsewhere)."""
    lib = _lib.load()
    xs = _exchanged(graph, cur.shape[0], cur.shape[1])
    with torch.cuda.device(cur.device):      # xs = a * X (the source rows' factor, applied before the rows travel)
        _lib.check(lib.cb_act_bwd_f32(_lib.ptr(cur), None, _lib.ptr(graph.norm_out), _lib.ptr(xs), cur.shape[0], cur.shape[1], None, None, 0,
                                      _lib.stream_ptr()), 'cb_act_bwd_f32')
    h_agg = graph.aggregate_finish(graph.aggregate_start(xs, False, orient=orient), False)
    del xs
    b0 = s0.norm_in_of(graph)
    # (a structural-embedding table on the layer: its rows are summed over the same level orientation — a second, equally small exchange)
    le_sum = graph.aggregate_finish(graph.aggregate_start(le, False, orient=orient), False, row_scale=b0) if le is not None else None
    y = gemm.mm_nn(h_agg, w, rowscale=b0, addend=le_sum, bias=b)
    del h_agg, le_sum
    n, d = graph.N, w.shape[1]
    bits = torch.empty((n, d // 256, 4), dtype=torch.int64, device=cur.device)
    x_l, _act = _store_rows(y, s0.idx, mix, 1 - alpha, alpha, p, seed, row0, bits, residual)
    del y
    logits_c = gemm.mm_nn(x_l, w_out.t().contiguous(), bias=b_out)
    out = ops.expand_unread(logits_c, s0, n)
    graph.rows_only_forwards += 1
    return bits, x_l, out


class _Forward:
    """The trunk's forward, one object per call: run() = _front, then per layer "_form picks the form, call it, book-keep", then the output Linear.
    Carried between the stages: cur (the dropped input of the next layer; None while no copy of it exists), mix (the layer's mix source: X0, 'Residual'
    above layer 0: the previous ReLU output), z_ready (Z_l already left by layer l-1's kernel), saved_in / saved_bits (kept for the backward), out_head /
    out_rows (the logits where the last layer's form produced them), h_last / h_below (the aggregates of the layers that took their sum first)."""

    def __init__(self, ctx, graph, cfg, x, w_in, b_in, w_out, b_out, layer_params):
        self.graph, self.cfg, self.x = graph, cfg, x.contiguous()
        self.w_in, self.b_in, self.w_out, self.b_out = w_in, b_in, w_out, b_out
        self.layer_params, self.layers = layer_params, _layers(layer_params)
        self.row0, self.a = int(getattr(graph, 'row_offset', 0)), graph.norm_out
        self.bwd = bool(cfg.track) and any(ctx.needs_input_grad)          # eval / metrics forwards (no_grad): no mask words, nothing kept
        self.z_ready = self.out_head = self.out_rows = self.h_last = self.h_below = None

    def run(self):
        cfg, graph = self.cfg, self.graph
        (self.xd, self.x0, self.x0_bits, self.cur, self.z_front), self.indrop = self._front()
        h = self.x0.shape[1]
        self.saved_in, self.saved_bits = [self.cur], []
        self.ag = agg_gemm_eligible(graph, h, cfg.agg_bf16)
        self.ro = _rows_only_decision(graph, cfg, self.x, self.x0, h, self.ag, self.bwd, self.layer_params)
        self.mix, self.kw = self.x0, dict(want_bits=self.bwd, relu_only=cfg.residual)
        for l in range(cfg.L):
            # (bias, mix source, c_act, c_mix, p, seed) of layer l's store; keep_act ('Residual'): its ReLU output is the next mix source (mask words: ReLU on
            self.st = (self.layers[l][1], self.mix, 1 - cfg.alpha, cfg.alpha, cfg.p, cfg.seeds[l + 2] if cfg.p > 0 else 0)
            self.keep_act = cfg.residual and l + 1 < cfg.L
            z0 = self._z0() if l == 0 else None
            bits, self.cur, act = self._form(l, z0 is not None)(l, z0)
            del z0
            if cfg.residual:
                self.mix = act
            if self.bwd:
                self.saved_bits.append(bits)
                self.saved_in.append(self.cur)
        self.mix = None
        return self.out_head if self.out_head is not None else gemm.mm_nn(self.cur, self.w_out.t().contiguous(), bias=self.b_out)

    def _front(self):
        """X0 = relu(Linear_0(dropout(x))): ((xd, x0, x0_bits, cur, z_front), fused) — xd = the features as the backward keeps them, x0_bits = mask words of
        (X0 > 0), cur = dropout(X0) | None, z_front = Z_0 | None; fused: a GEMM applied the features' dropout while it staged x (xd is the UNdropped x, the
        weight gradient regenerates the mask).  In order: the front kernel (cb_trunk_front_f32: also dropout(X0), stored for a backward unless
        CB_TRUNK_X0_COPY=0, and layer 0's transform), the in-drop GEMMs, the plain dropout pass + GEMM (CB_TRUNK_INDROP=0, or no such form)."""
        c, x, w_in, b_in, row0, bwd, p, seeds = self.cfg, self.x, self.w_in, self.b_in, self.row0, self.bwd, self.cfg.p, self.cfg.seeds
        indrop = p > 0 and _switch('CB_TRUNK_INDROP', '1') != '0'
        copy = _switch('CB_TRUNK_X0_COPY', '1') == '1'
        if (indrop or p == 0) and not c.agg_bf16 and c.L >= 1 and w_in.shape[0] == 256 and _switch('CB_TRUNK_FRONT', '1') != '0':
            w0, _b0, le0 = self.layers[0]
            fr = gemm.trunk_front(x, w_in, b_in, w0, self.a, le0, p, seeds[0], seeds[1], row0, want_bits=bwd, want_drop=bwd and p > 0 and copy,
                                  z_out=_exchanged(self.graph, x.shape[0]) if hasattr(self.graph, 'part') else None)
            if fr is not None:
                x0, x0_bits, cur, z_front = fr
                return (x, x0, x0_bits, x0 if p == 0 else cur, z_front), True
        if indrop:
            wb = bwd and w_in.shape[0] == 256
            r = None if copy else gemm.mm_nn_indrop(x, w_in.t().contiguous(), p, seeds[0], row0, bias=b_in, relu=True, want_bits=wb)
            if r is not None:
                return (x, *(r if wb else (r, None)), None, None), True
            r = gemm.mm_nn_indrop_drop2(x, w_in.t().contiguous(), p, seeds[0], seeds[1], row0, bias=b_in, relu=True, want_bits=wb)
            if r is not None:
                return (x, r[0], r[2] if len(r) > 2 else None, r[1], None), True
        xd = ops._dropout_raw(x, p, seeds[0], row0 * x.shape[1]) if p > 0 else x
        if p > 0:
            x0, cur = gemm.mm_nn_drop2(xd, w_in.t().contiguous(), p, seeds[1], row0, bias=b_in, relu=True)
        else:
            x0 = cur = gemm.mm_nn(xd, w_in.t().contiguous(), bias=b_in, relu=True)
        return (xd, x0, None, cur, None), False

    def dropped_x0(self):
        return ops._dropout_raw(self.x0, self.cfg.p, self.cfg.seeds[1], self.row0 * self.x0.shape[1])

    def _z0(self):
        """Z_0 where the front kernel left it or layer 0's GEMM draws the mask in front of it (GCN.py:110) while it stages X0; else None, and the dropped
        copy of X0 (cur) exists from here on."""
        z0, self.z_front = self.z_front, None
        if z0 is not None or self.cur is not None:
            return z0
        c, (w, _b, le) = self.cfg, self.layers[0]
        if not (c.agg_bf16 or (not self.ag and _chunked(self.graph, c.agg_bf16))):
            z0 = gemm.mm_nn_indrop(self.x0, w, c.p, c.seeds[1], self.row0, rowscale=self.a, addend=le, out=_exchanged(self.graph, self.x0.shape[0], w.shape[1]))
        if z0 is None:
            self.cur = self.saved_in[0] = self.dropped_x0()
        return z0

    def _form(self, l, have_z0):
        """The form layer l takes (a _form_* method), in this order of precedence; nothing is launched here."""
        L, ro = self.cfg.L, self.ro
        if self.ag and ro.sum_first_below and l == L - 2:
            return self._form_sum_first_below
        if self.ag and ro.sharded is not None and l == L - 1:
            return self._form_last_on_loss_rows_sharded
        if ro.plan is not None and l == L - 1:
            return self._form_last_on_loss_rows
        if self.ag:      # aggregation + GEMM kernels: what follows the store of this layer
            if ro.sum_first_below and l + 3 == L:      # the layer under the sum-first one
                return self._form_store
            if ro.plan is not None and l + 2 == L and ro.below is not None:
                return self._form_store_on_s1
            if (ro.plan is not None or ro.sharded is not None) and l + 2 == L:      # the layer above aggregates X_{l+1} itself: no dense tail
                return self._form_store
            return self._form_store_gemm if l + 1 < L else self._form_store_head
        if not have_z0 and _chunked(self.graph, self.cfg.agg_bf16):
            return self._form_chunked
        return self._form_store      # plain: the transform unless the front left it, then aggregation + store

    # -- the forms: each returns (mask words, the dropped stored output = the next `cur`, ReLU output | None) -------------------------------------
    def _z(self, l, z0):
        """Z_l: left by layer l-1's aggregation + GEMM kernel, by the front (z0), else a * (X W) + le now."""
        z, self.z_ready = self.z_ready, None
        if z is None and z0 is None:
            (w, _b, le), bf = self.layers[l], self.cfg.agg_bf16
            return gemm.mm_nn(self.cur, w, rowscale=self.a, addend=le, out_bf16=bf, out=None if bf else _exchanged(self.graph, self.cur.shape[0], w.shape[1]))
        return z if z is not None else z0

    def _form_sum_first_below(self, l, z0):
        """Layer L-2 on S_1 with its sum taken first (_layer_on_rows); X_{L-2} is read by that aggregation only, the backward contracts h_below."""
        c, below, (w, b, _le) = self.cfg, self.ro.below, self.layers[l]
        bits, cur, act, self.h_below = _layer_on_rows(self.graph, below.s1, below.fwd1, self.a, self.cur, w, b, self.mix, None, c.alpha, c.p,
                                                      self.st[5], self.row0, c.residual, want_act=self.keep_act)
        self.saved_in[l] = None
        return bits, cur, act

    def _form_last_on_loss_rows_sharded(self, l, z0):
        c, (s0, orient), (w, b, le) = self.cfg, self.ro.sharded, self.layers[l]
        bits, cur, self.out_head = _last_layer_on_loss_rows_sharded(self.graph, s0, orient, self.cur, w, b, self.mix, c.alpha, c.p, self.st[5],
                                                                    self.row0, c.residual, self.w_out, self.b_out, le=le)
        return bits, cur, None

    def _form_last_on_loss_rows(self, l, z0):
        c, (w, b, le) = self.cfg, self.layers[l]
        bits, cur, (self.out_head, self.out_rows), self.h_last = _last_layer_on_loss_rows(
            self.graph, self.ro.plan, self.cur, w, b, self.mix, c.alpha, c.p, self.st[5], self.row0, c.residual, self.w_out, self.b_out,
            below=self.ro.below, le=le)
        if le is None:
            self.saved_in[l] = None      # X_{L-1}: read by the aggregation above only (the level's weight gradient contracts h_last)
        else:
            self.h_last = None           # the table's gradient is dL/dZ itself: level 0 stays on the compact form, which reads X_{L-1} on S_1
        return bits, cur, None

    def _form_store(self, l, z0):
        return _fused_spmm(self.graph, self._z(l, z0), *self.st, want_act=self.keep_act, **self.kw)

    def _form_store_on_s1(self, l, z0):
        """... on S_1 only (the in-neighbours of the loss rows, all that reads this layer's outputs): compact."""
        below, z = self.ro.below, self._z(l, z0)
        below.fwd1.profile = getattr(self.graph, 'profile', None)
        return _fused_launch(_lib.load(), self.graph, below.fwd1, z, None, *self.st, self.keep_act, row_ids=below.ids1, row_scale=below.b1, **self.kw)

    def _form_store_gemm(self, l, z0):
        """This layer's store + the next layer's transform in one kernel (leaves z_ready)."""
        w1, _, le1 = self.layers[l + 1]
        res = _fused_gemm(self.graph, self._z(l, z0), *self.st, weight_image(w1), self.a, le1, want_act=self.keep_act, **self.kw)
        self.z_ready = res[2]
        return res[0], res[1], res[3] if self.keep_act else None

    def _form_store_head(self, l, z0):
        """The last layer: the output Linear (GCN.py:133-138) is the tail of its aggregation where that form exists (<= 64 classes; head_tail_enabled)."""
        z = self._z(l, z0)
        himg = head_image(self.w_out) if head_tail_enabled(self.bwd) else None
        if himg is None:
            return _fused_spmm(self.graph, z, *self.st, **self.kw)
        bits, cur, self.out_head = _fused_gemm(self.graph, z, *self.st, himg, None, None, head=(self.b_out, self.w_out.shape[0]), **self.kw)[:3]
        return bits, cur, None

    def _form_chunked(self, l, z0):
        """Node-sharded pipeline: row chunk k of Z leaves the GEMM, is packed and put on the links while chunk k+1 multiplies."""
        (w, _b, le), cur, a = self.layers[l], self.cur, self.a
        z = _exchanged(self.graph, cur.shape[0], w.shape[1])

        def produce(k, r0, r1):
            if r1 > r0:
                gemm.mm_nn(cur[r0:r1], w, rowscale=a[r0:r1], addend=le[r0:r1] if le is not None else None, out=z[r0:r1])
        return _fused_spmm(self.graph, z, *self.st, want_act=self.keep_act, produce=produce, **self.kw)


class _TrunkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, graph, cfg, x, w_in, b_in, w_out, b_out, *layer_params):
        """layer_params = (W_0, bias_0, le_0 | None, W_1, ...), cfg: TrunkCfg.  Returns (logits [N, C], the logits of the loss rows as the compact [|S_0|, C]
        matrix a rows-only forward on one GPU computed, else None): a loss built on the second hands its gradient back compact."""
        f = _Forward(ctx, graph, cfg, x, w_in, b_in, w_out, b_out, layer_params)
        out = f.run()
        ctx.graph, ctx.cfg, ctx.row0, ctx.indrop, ctx.n_layer_params = graph, cfg, f.row0, f.indrop, len(layer_params)
        if f.bwd:
            _save(ctx, xd=f.xd, x0=f.x0, w_in=w_in, w_out=w_out, saved_in=f.saved_in, saved_bits=f.saved_bits, layer_params=layer_params,
                  h_last=f.h_last, h_below=f.h_below, x0_bits=f.x0_bits)
            ro = f.ro      # (row shards / a table on the last layer: saved_in[L] alone is compact)
            ctx.saved_rows = SavedRows('S0' if (ro.plan is not None or ro.sharded is not None) else 'all',
                                       'absent' if f.h_last is not None else 'S1' if (ro.plan is not None and ro.below is not None) else 'all')
        ctx.set_materialize_grads(False)
        return out, f.out_rows

    @staticmethod
    def backward(ctx, gout, gout_rows=None):
        if gout is None and gout_rows is None:
            return (None,) * (7 + ctx.n_layer_params)
        return _Backward(ctx, gout, gout_rows).run()


class _Carry:
    """What a layer of the backward hands the one below: g = dL/d(its stored output), gr = its store backward (b * dY'), dbias, handle = gr's exchange
    where already in flight, space = the RowSpace of g / gr (None: all rows), g_above ('Residual'), deferred = a weight gradient (layer, X_l, dZ_l, dst)."""
    __slots__ = ('g', 'gr', 'dbias', 'handle', 'space', 'g_above', 'deferred')

    def __init__(self, g, gr, dbias, handle, space):
        self.g, self.gr, self.dbias, self.handle, self.space, self.g_above, self.deferred = g, gr, dbias, handle, space, None, None


class _Backward:
    """The hand-written backward of the trunk, one object per call.  run() = _resolve_plan, _head, then per layer from the last to the first _layer (reverse
    aggregation, dX, weight gradient) and _store_bwd_below (the layer below's store backward), then _input_stage.  _layer's forms, by where the operands live:
      * _layer_source_side / _layer_compact: a level of the row-sparse PLAN (one GPU): compact [|S_j|, .] matrices, the level's own orientation;
      * _layer_fused: the reverse aggregation + dX contraction in one kernel (cb_spmm_gemm_f32) on all rows — one GPU, or as the last halo pass
        of a node-sharded exchange (whose level orientations restrict the exchange to the support's rows: dist.ShardedGraph.support_orients);
      * _layer_plain: aggregation, then the dX GEMM (+ row-chunked producers of the node-sharded pull pipeline; bf16-stored rows).
    fold_ok: the input stage without a pass of its own — only with the row-sparse plan (plan_taken): the dense backward keeps the
    passes whose sums are the bit-for-bit witness of the fused forms."""

    def __init__(self, ctx, gout, gout_rows=None):
        self.gout_rows = gemm._rowmajor(gout_rows) if gout_rows is not None else None      # gradient of the compact loss-row logits (forward's second output)
        self.ctx, graph, c = ctx, ctx.graph, ctx.cfg
        self.graph, self.row0, self.L, self.alpha, self.p, self.seeds = graph, ctx.row0, c.L, c.alpha, c.p, c.seeds
        self.agg_bf16, self.residual = c.agg_bf16, c.residual
        sv = _saved(ctx)
        self.xd, self.x0, self.w_in, self.w_out = sv['xd'], sv['x0'], sv['w_in'], sv['w_out']
        self.saved_in, self.saved_bits, self.x0_bits = sv['saved_in'], sv['saved_bits'], sv['x0_bits']
        self.h_last, self.h_below = sv['h_last'], sv['h_below']      # (A (a * X_{L-1}))[S_0], (A (a * X_{L-2}))[S_1] of the sum-first layers
        self.lp, self.where = _layers(sv['layer_params']), ctx.saved_rows      # (SavedRows: where saved_in[L] and saved_in[L - 1] live)
        self.a, self.bnorm = graph.norm_out, graph.norm_in
        self.need = ctx.needs_input_grad       # (graph, cfg, x, w_in, b_in, w_out, b_out, *layer_params)
        self.gout = gemm._rowmajor(gout) if gout is not None else None
        self.n_rows, self.h = self.x0.shape
        self.sharded, loss_rows = hasattr(graph, 'part'), c.loss_rows
        if loss_rows is not None and self.where.x_last != 'S0' and (not ops.loss_rows_enabled() or loss_rows[0].shape[0] != self.x0.shape[0]):
            loss_rows = None
        self.loss_rows = loss_rows
        # the gradients that reach X0 through the mixes: gathered in one pass by the input stage (_gather), else accumulated in place layer by layer (gx0)
        self.gather = _gather(graph, c.L, c.residual, self.x0)
        self.gx0 = None if self.gather else torch.empty_like(self.x0)
        self.g_mix, self.seeds_mix, self.mix_pos = [], [], []
        self.cs = []      # (index into g_mix, mask words, factor, layer): bias gradients left to the input stage as extra column sums (_store_bwd_below)
        self.grads_layers = [None] * (3 * c.L)
        self.ag = agg_gemm_eligible(graph, self.h, c.agg_bf16)
        self.chunked = (self.gather and _chunked(graph, c.agg_bf16) and graph.b.plan.n_slices > 1 and not self.ag)
        self.fold_ok = (_switch('CB_INSTAGE_FOLD', '1') != '0' and self.gather and not c.residual and not c.agg_bf16 and c.p > 0
                        and ctx.indrop and self.need[3] and not self.need[2] and self.x0_bits is not None and self.h == 256
                        and gemm.mm_tn_instage_supported(self.x0, self.xd, self.x0.shape[0]))
        self.mfold, self.plan_taken = None, False      # (the folded mix gradients, once a level produced them)

    def seed(self, i):
        return self.seeds[i] if self.p > 0 else 0

    def need_w(self, l):
        return self.need[7 + 3 * l]

    def need_b(self, l):
        return self.need[7 + 3 * l + 1]

    def need_le(self, l):
        return self.lp[l][2] is not None and self.need[7 + 3 * l + 2]

    def _dw(self, l, x_in, gz):
        """X_l^T (a * dZ_l).  Layer 0 without a dropped copy of X0 (x_in is None): the mask of the dropout in front of layer 0 is
        regenerated from X0 (_dw_regen)."""
        if x_in is not None:
            return gemm.mm_tn(x_in, gz, rowscale=self.a)
        return _dw_regen(self.x0, gz, self.p, self.seed(1), self.row0, self.a)

    def _second(self, below, g_above, pos_above=None):
        """'Residual': keyword arguments of the second gradient that reaches layer `below`'s ReLU output — through the mix of layer below + 1,
        under that layer's dropout mask.  pos_above: the position map of g_above's row space when it is a compact matrix (row-sparse plan)."""
        if not self.residual or g_above is None:
            return {}
        return dict(g2=g_above, seed2=self.seed(below + 3), c2=self.alpha, **({'g2_pos': pos_above} if pos_above is not None else {}))

    def _dx_and_store_bwd(self, src, wt, rowscale, below, g_ready=None, g_above=None, orient=None, pos_above=None):
        """dL/dx of the stage above layer `below` and that layer's store backward: (g, gr, dbias, handle); handle = the already started
        exchange of gr (row-chunked producers of the node-sharded pull pipeline), else None.  g_ready: dL/dx left the reverse aggregation's kernel."""
        p, alpha, row0, bnorm = self.p, self.alpha, self.row0, self.bnorm
        sd, want_b, bits = self.seed(below + 2), self.need_b(below), self.saved_bits[below]
        if self.chunked:
            g_ = torch.empty((src.shape[0], wt.shape[1]), dtype=torch.float32, device=src.device)
            gr_ = _exchanged(self.graph, g_.shape[0], g_.shape[1])
            colsums = []
            sec = self._second(below, g_above, pos_above)

            def produce(k, r0, r1):
                if r1 <= r0:
                    return
                gemm.mm_nn(src[r0:r1], wt, rowscale=rowscale[r0:r1] if rowscale is not None else None, out=g_[r0:r1])
                sec_k = dict(sec, g2=sec['g2'][r0:r1]) if sec else {}
                _, cs = _layer_bwd(g_[r0:r1], bits[r0:r1], bnorm[r0:r1], None, False, p, sd, row0 + r0, 1 - alpha, alpha, want_b, out=gr_[r0:r1], **sec_k)
                if want_b:
                    colsums.append(cs)
            h_ = self.graph.aggregate_start(gr_, True, produce=produce, orient=orient)
            db_ = None
            if want_b:      # (a rank that owns no rows produces no chunk: its share of the bias gradient is zero)
                db_ = (torch.zeros(wt.shape[1], dtype=torch.float32, device=src.device) if not colsums
                       else colsums[0] if len(colsums) == 1 else torch.stack(colsums).sum(0))
            return g_, gr_, db_, h_
        g_ = g_ready if g_ready is not None else gemm.mm_nn(src, wt, rowscale=rowscale)
        cs_ = self.cs
        if (below == 0 and self.fold_ok and self.mfold is None and self.plan_taken and len(self.g_mix) <= 2 and len(cs_) <= 1
                and all(t.is_contiguous() for t in self.g_mix) and g_.is_contiguous()):
            # layer 0's store backward as a pass of its own (no reverse aggregation carries it): it also folds the mix gradients (cb_trunk_layer_bwd_fold_f32)
            res = _layer_bwd_fold(g_, bits, bnorm, p, sd, row0, 1 - alpha, alpha, want_b, self.g_mix, self.mix_pos, self.seeds_mix,
                                  out=_exchanged(self.graph, g_.shape[0], g_.shape[1]) if self.sharded else None, cs=cs_[0][:3] if cs_ else None)
            gr_, db_, self.mfold = res[:3]
            if cs_:      # (the bias gradient the input-stage pass would have taken for a store whose backward left a reverse aggregation's epilogue)
                self.grads_layers[3 * cs_[0][3] + 1] = res[3]
                self.cs = []
            self.g_mix, self.mix_pos, self.seeds_mix = [], [], []
            return None, gr_, db_, None
        gr_, db_ = _layer_bwd(g_, bits, bnorm, self.gx0, below != self.L - 1, p, sd, row0, 1 - alpha, alpha, want_b, out_bf16=self.agg_bf16,
                              out=_exchanged(self.graph, g_.shape[0], g_.shape[1]) if (self.sharded and not self.agg_bf16) else None,
                              **self._second(below, g_above, pos_above))
        return g_, gr_, db_, None

    def _head(self, space):
        """Output Linear (GCN.py:133-138) and the store backward of the last layer: sets d_w_out, d_b_out and returns the _Carry for layer L - 1.
        space: the compact row space of the loss rows (a plan's space0 / a rank's share of it), or None = all rows."""
        L, need, gout, xl = self.L, self.need, self.gout, self.saved_in[self.L]
        if space is not None:      # loss rows only
            gout = ops.gather_rows_by_index(gout, space.idx) if gout is not None else None
            if self.gout_rows is not None:      # (the compact output's gradient arrives on those rows already)
                gout = self.gout_rows if gout is None else gout + self.gout_rows
            xl = xl if self.where.x_last == 'S0' else ops.gather_rows_by_index(xl, space.idx)
        self.d_w_out = gemm.mm_tn(gout, xl) if need[5] else None
        self.d_b_out = ops.act_bwd(gout, None, None, want_out=False, want_colsum=True)[1] if need[6] else None
        if space is None:
            return _Carry(*self._dx_and_store_bwd(gout, self.w_out, None, L - 1, orient=self._orient_of(L - 1)), None)
        g = gemm.mm_nn(gout, self.w_out)                                        # dL/d(dropped X_L), loss rows only
        gr, dbias = _layer_bwd_rows(g, space.idx, self.saved_bits[L - 1], self.bnorm, self.p, self.seed(L + 1), self.row0, 1 - self.alpha,
                                    self.need_b(L - 1), out=_exchanged(self.graph, g.shape[0], g.shape[1]) if self.sharded else None)
        return _Carry(g, gr, dbias, None, space)

    def _sh_level(self, layer):
        """Node-sharded: the dist.SupportLevel of the reverse aggregation of `layer` (orientation + row spaces), or None."""
        j = self.L - 1 - layer
        return self.sh_levels[j] if 0 <= j < len(self.sh_levels) else None

    def _orient_of(self, layer):
        return getattr(self._sh_level(layer), 'orient', None)

    def _dw_rows(self, l, x_in, gz, dst):
        """The layer's weight gradient with dL/dZ_l on the rows of `dst` (None: all rows — _dw)."""
        if dst is None:
            return self._dw(l, x_in, gz)
        return gemm.mm_tn(ops.gather_rows_by_index(x_in, dst.idx), gz, rowscale=dst.a)

    def _layer_source_side(self, l, gr, level, fwd_j):
        """A plan level through its SOURCE rows' side (CSRGraph._support_fwd; level 0: the loss rows): a * (A^T dY) W^T = a * A^T (dY W^T) and
        X^T (a * A^T dY) = ((A (a * X))[S_j])^T dY[S_j] — the GEMM and the weight gradient contract over |S_j| rows instead of |S_{j+1}|,
        dL/dZ_l itself is never formed (so not with a table gradient, which IS dL/dZ_l).  Same sums, associated differently.
        Returns (None, g_new, fused): fused = (gr of the layer below, that layer) when the level's kernel also ran that layer's store backward, else None."""
        w = self.lp[l][0]
        dst = level[1]
        level[0].profile = getattr(self.graph, 'profile', None)
        if fwd_j is not None:
            fwd_j.profile = level[0].profile
        t = gemm.mm_nn(gr, w.t().contiguous())
        fused = None
        if (l > 0 and not self.residual and self.gather and len(self.cs) < 2 and dst is None
                and hasattr(level[0], 'spmm_store_bwd') and t.shape[1] % 256 == 0):
            # a level that writes all rows: the store backward of the layer below leaves this kernel's epilogue; its bias gradient: the input stage's (self.cs)
            fold = self.fold_ok and l == 1 and len(self.g_mix) <= 2 and all(q is not None for q in self.mix_pos) and not self.cs
            if fold:      # (g_mix holds the mix gradients of the layers above, compact on their supports; layer 0's own is this aggregation's sum)
                self.mfold, gr_below, db0 = level[0].spmm_store_bwd(t, self.a, self.saved_bits[0], self.bnorm, 1 - self.alpha, self.p, self.seed(2), self.row0,
                                                                    mix=(self.g_mix, self.mix_pos, self.seeds_mix, self.alpha, self.need_b(0)))
                self.grads_layers[1] = db0
                self.g_mix, self.mix_pos, self.seeds_mix = [], [], []      # folded: the input stage reads self.mfold instead
                g_new = None
            else:
                g_new, gr_below = level[0].spmm_store_bwd(t, self.a, self.saved_bits[l - 1], self.bnorm, 1 - self.alpha, self.p, self.seed(l + 1), self.row0)
            fused = (gr_below, l - 1)
        else:
            g_new = level[0].spmm(t, row_scale=dst.a if dst is not None else self.a)
        del t
        if self.need_w(l):
            # (the aggregate the rows-only forward saved, else taken now)
            x_agg = (self.h_last if (self.where.x_below == 'absent' and l == self.L - 1) else self.h_below if (self.h_below is not None and l == self.L - 2)
                     else fwd_j.spmm(self.saved_in[l], col_scale=self.a))
            self.grads_layers[3 * l] = gemm.mm_tn(x_agg, gr)
        return None, g_new, fused

    def _layer_compact(self, l, gr, level):
        """A plan level on compact matrices: dL/dZ_l = A (b * dY') over the level's own orientation (rows / columns renumbered to positions in
        S_{j+1} / S_j) and a * (dL/dZ_l @ W_l^T) from the same kernel; the weight gradient over the rows of S_{j+1}."""
        w = self.lp[l][0]
        dst = level[1]
        level[0].profile = getattr(self.graph, 'profile', None)
        gz, g_new = level[0].spmm_gemm(gr, weight_image(w, transpose=True), transpose=False, g_rowscale=dst.a if dst is not None else self.a)
        if self.need_w(l):
            if dst is not None:      # dL/dZ_l lives on S_{j+1}: X_l^T (a * dZ_l) over those rows (all others contribute zeros)
                on_s1 = self.where.x_below == 'S1' and l == self.L - 1      # (the rows-only forward left X_{L-1} on those rows already)
                x_rows = self.saved_in[l] if on_s1 else ops.gather_rows_by_index(self.saved_in[l], dst.idx)
                self.grads_layers[3 * l] = gemm.mm_tn(x_rows, gz, rowscale=dst.a)
            else:
                self.grads_layers[3 * l] = self._dw(l, self.saved_in[l], gz)
        return gz, g_new

    def _layer_fused(self, l, gr, handle, dst=None):
        """dL/dZ_l = A (b * dY') and a * (dL/dZ_l @ W_l^T) from one kernel (cb_spmm_gemm_f32) on all rows.  Node-sharded: the kernel is the LAST
        halo pass of the reverse aggregation, on top of the running sums of the earlier passes; dst (a compact level of the rank, dist.SupportLevel):
        its rows are the positions of the level's destination support.  Returns (gz, g_new)."""
        graph = self.graph
        a = dst.a if dst is not None else self.a
        img = weight_image(self.lp[l][0], transpose=True)

        def tail(csr, src, acc, tr):
            csr.profile = getattr(graph, 'profile', None)
            return csr.spmm_gemm(src, img, transpose=tr, g_rowscale=a, acc_init=acc)
        return (graph.aggregate_finish(handle, True, last_pass=lambda csr, recv, acc: tail(csr, recv, acc, False)) if self.sharded
                else tail(graph, gr, None, True))

    def _layer_plain(self, gr, handle):
        """dL/dZ_l = A (b * dY') by the plain aggregation (the dX GEMM is a kernel of its own)."""
        return self.graph.aggregate_finish(handle, True) if self.sharded else _spmm_t(self.graph, gr)

    def _resolve_plan(self):
        """(plan, space0): where this backward runs on fewer rows than all ("Row-sparse backward").  One GPU: level j lives on the
        support S_j of CSRGraph.grad_support_plan ('Residual': cumulative supports), compact while small; the caller's promise is checked on the device.
        Node-sharded (self.sh_levels): the same as level orientations of the reverse exchange."""
        graph, L, gout, xl_compact = self.graph, self.L, self.gout, self.where.x_last == 'S0'
        self.sh_levels = []
        if self.gout_rows is not None and not xl_compact:
            raise RuntimeError('gradient for the compact loss-row logits, but the forward did not run rows-only')
        if self.sharded and hasattr(graph, 'support_levels') and self.loss_rows is not None:
            ops.check_rows_zero(gout, self.loss_rows[0])
            self.sh_levels = graph.support_levels(self.loss_rows[0], L, compact=self.ag and self.gather, cumulative=self.residual)
        plan = None
        hint = None if self.sharded else _support_plan(graph, self.loss_rows, self.n_rows, L, self.residual, self.h, self.x0, committed=xl_compact)
        if hint is not None:
            if gout is not None:      # (no gradient for the [N, C] output at all: the loss was built on the compact output — nothing to check)
                ops.check_rows_zero(gout, hint[0])
            # (count: one use per step — the forward of a rows-only step has looked the plan up already)
            plan = graph.grad_support_plan(hint[0], L, max_frac=T.rowsparse_max_frac, cumulative=self.residual, count=not xl_compact)
        self.plan_taken = plan is not None or bool(self.sh_levels)
        if self.where.x_below == 'absent' and plan is None:
            raise RuntimeError('the forward evaluated its last layer on the loss rows (rows_only), but its backward finds no row-support plan: '
                               'CB_LOSS_ROWS / tuning.T / the mask changed between the forward and the backward')
        space0 = plan.space0 if plan is not None else (self.sh_levels[0].src if self.sh_levels else None)
        if xl_compact and space0 is None:
            raise RuntimeError('the forward evaluated its last layer on the loss rows (rows_only), but its backward has no compact level 0')
        return plan, space0

    def _layer(self, l, c, plan):
        """Layer l's reverse aggregation, dX and weight gradient: (gz = dL/dZ_l | None, g_new = dL/d(dropped X_l) | None, dst = their RowSpace | None,
        fused = _layer_source_side's third result).  Row shards: starts c.gr's exchange and computes the deferred weight gradient under it."""
        L, graph, sharded = self.L, self.graph, self.sharded
        j = L - 1 - l
        level = plan.levels[j] if (plan is not None and j < len(plan.levels)) else None
        lv = self._sh_level(l)
        dst = level[1] if level is not None else lv.dst if lv is not None else None
        if sharded and c.handle is None:
            c.handle = graph.aggregate_start(c.gr, True, orient=self._orient_of(l))   # node-sharded: the exchange is in flight from here
        if c.deferred is not None:
            self.grads_layers[3 * c.deferred[0]] = self._dw_rows(*c.deferred)
            c.deferred = None
        fwd_j = plan.fwd[j] if (level is not None and j < len(plan.fwd)) else None
        source_side = ((self.where.x_below == 'absent' and l == L - 1) or (self.h_below is not None and l == L - 2)
                       or (T.rowsparse_loss_side and fwd_j is not None and not self.need_le(l)
                           and not (self.need_w(l) and self.saved_in[l] is None)      # (layer 0 without a stored dropped copy of X0)
                           and not (self.where.x_below == 'S1' and l == L - 1)))
        if source_side:
            _gz, g_new, fused = self._layer_source_side(l, c.gr, level, fwd_j)
            return None, g_new, dst, fused
        if level is not None:
            return (*self._layer_compact(l, c.gr, level), dst, None)
        gz, g_new = self._layer_fused(l, c.gr, c.handle, dst) if self.ag else (self._layer_plain(c.gr, c.handle), None)
        if self.need_w(l):
            if sharded:
                c.deferred = (l, self.saved_in[l], gz, dst if self.ag else None)
            else:
                self.grads_layers[3 * l] = self._dw(l, self.saved_in[l], gz)
        return gz, g_new, dst, None

    def _store_bwd_below(self, l, c, gz, g_new, dst, fused, pos_above):
        """Into c what layer l - 1 starts from: g = dL/d(dropped X_l), gr = its store backward, dbias, handle (l = 0: g alone, for the input stage)."""
        w = self.lp[l][0]
        if l > 0 and fused is not None:      # the level's own kernel ran it
            c.g, (c.gr, _below), c.dbias = g_new, fused, None      # (dbias of layer l - 1: an extra column sum of the input stage)
            if self.mfold is not None:      # (folded: the epilogue took that bias gradient itself)
                c.dbias = self.grads_layers[3 * (l - 1) + 1]
            elif self.need_b(l - 1):
                self.cs = self.cs + [(len(self.g_mix), self.saved_bits[l - 1], 1 - self.alpha, l - 1)]
        elif l > 0 and dst is not None:      # the store backward of layer l-1 on the rows of S_{j+1}
            c.g = g_new
            c.gr, c.dbias = _layer_bwd_rows(g_new, dst.idx, self.saved_bits[l - 1], self.bnorm, self.p, self.seed(l + 1), self.row0, 1 - self.alpha,
                                            self.need_b(l - 1), out=_exchanged(self.graph, g_new.shape[0], g_new.shape[1]) if self.sharded else None,
                                            **self._second(l - 1, c.g_above, pos_above))
        elif l > 0:      # dL/d(dropped X_l) and the backward of layer l-1's store
            c.g, c.gr, c.dbias, c.handle = self._dx_and_store_bwd(gz, w.t().contiguous(), self.a, l - 1, g_new, c.g_above, orient=self._orient_of(l - 1),
                                                                  pos_above=pos_above)
        else:            # dL/d(dropped X_0): consumed by the input stage
            c.g = g_new if g_new is not None else gemm.mm_nn(gz, w.t().contiguous(), rowscale=self.a)

    def run(self):
        plan, space0 = self._resolve_plan()
        c = self._head(space0)
        for l in range(self.L - 1, -1, -1):
            if self.gather and (not self.residual or l == 0) and self.mfold is None:      # this layer's mix reads X0: the input stage gathers its gradient
                self.g_mix.append(c.g)
                self.mix_pos.append(c.space.pos if c.space is not None else None)
                self.seeds_mix.append(self.seed(l + 2))
            gz, g_new, dst, fused = self._layer(l, c, plan)
            c.g_above = c.g if self.residual else None         # 'Residual': dL/d(stored output) of the layer above the one whose store backward comes next
            pos_above = c.space.pos if (self.residual and c.space is not None) else None      # (g lives on the space of this level's source rows)
            c.g = c.gr = c.handle = None
            self.grads_layers[3 * l + 1] = c.dbias
            c.space = dst
            self._store_bwd_below(l, c, gz, g_new, dst, fused, pos_above)
            c.g_above = None
            if self.need_le(l):
                if dst is not None:      # the table's gradient is dL/dZ_l on ALL rows: the support's rows, zeros elsewhere
                    gz = ops.expand_rows(gz, dst.pos)
                self.grads_layers[3 * l + 2] = gz
            del gz, g_new      # (what the layer below needs of them is in c: nothing else keeps them alive through its reverse aggregation)
        if c.deferred is not None:
            self.grads_layers[3 * c.deferred[0]] = self._dw_rows(*c.deferred)
        return self._input_stage(c)

    def _input_stage(self, c):
        """X0 feeds layer 0 and the mixes: the gradients of the input Linear and the features; folded (inside the weight gradient), gathered or accumulated."""
        graph, p, need, xd, row0 = self.graph, self.p, self.need, self.xd, self.row0
        g, c.g = c.g, None
        if self.mfold is not None:
            d_w_in, d_b_in = gemm.mm_tn_instage(g, self.mfold, self.x0_bits, xd, p, self.seed(1), p, self.seeds[0], row0)
            del g
            self.gx0 = self.g_mix = self.mfold = None
            graph.instage_folds = getattr(graph, 'instage_folds', 0) + 1      # (tests, bench)
            return (None, None, None, d_w_in, d_b_in if need[4] else None, self.d_w_out, self.d_b_out, *self.grads_layers)
        if self.gather:
            res = _input_bwd_multi(g, self.seed(1), self.g_mix, self.seeds_mix, self.alpha, self.x0, p, row0, act_bits=self.x0_bits,
                                   mix_pos=self.mix_pos, cs=[q[:3] for q in self.cs])
            gpre, d_b_in = res[0], res[1]
            for q, db in zip(self.cs, res[2] if self.cs else []):
                self.grads_layers[3 * q[3] + 1] = db
        else:
            gpre, d_b_in = _input_bwd(g, self.gx0, self.x0, p, self.seed(1), row0)
        del g
        self.gx0 = self.g_mix = None
        d_w_in = None
        if need[3]:
            if self.ctx.indrop and p > 0:      # xd holds the undropped features: the mask is regenerated while the GEMM stages them
                d_w_in = gemm.mm_tn_gdrop(gpre, xd, p, self.seeds[0], row0)
                if d_w_in is None:
                    d_w_in = gemm.mm_tn(gpre, ops._dropout_raw(xd, p, self.seeds[0], row0 * xd.shape[1]))
            else:
                d_w_in = gemm.mm_tn(gpre, xd)
        d_x = None
        if need[2]:
            d_x = gemm.mm_nn(gpre, self.w_in)
            if p > 0:
                d_x = ops._dropout_raw(d_x, p, self.seeds[0], row0 * d_x.shape[1])
        return (None, None, d_x, d_w_in, d_b_in if need[4] else None, self.d_w_out, self.d_b_out, *self.grads_layers)


def forward(tc, x, graph, loss_rows=None, rows_only=False):
    """TricksComb.forward on the fused trunk; returns (logits, se_reg_all).  loss_rows: None, (bool mask [N], count) or the mask alone — the caller's promise
    that the logits receive gradient in the rows of the mask only (the masked loss, trainer_node_classification.py:390-391).  rows_only (with loss_rows): it
    also READS the logits in those rows only — a training forward may then evaluate its last layer on them; the others are NaN (ops.unread_rows_fill)."""
    L = tc.num_layers
    p = float(tc.dropout) if tc.training else 0.0
    seeds = tuple(ops.next_seed() for _ in range(L + 2)) if p > 0 else (0,) * (L + 2)
    params, se_reg_all = _collect_layer_params(tc, graph)
    agg_bf16 = getattr(tc.args, 'agg_dtype', 'f32') == 'bf16'
    if loss_rows is not None:
        mask, count = loss_rows if isinstance(loss_rows, (tuple, list)) else (loss_rows, None)
        if count is None:      # (a host sync: the trainers hand the count, computed once per run)
            count = int(mask.sum().item())
        if mask.dtype != torch.bool or mask.dim() != 1 or mask.shape[0] != x.shape[0]:
            raise ValueError(f'loss_rows: a bool mask over the {x.shape[0]} rows expected, got {tuple(mask.shape)} {mask.dtype}')
        loss_rows = (mask, int(count))
    cfg = TrunkCfg(L, float(tc.alpha), p, seeds, agg_bf16, torch.is_grad_enabled(), loss_rows, connection(tc) == 'residual',
                   bool(rows_only) and loss_rows is not None)
    out, out_rows = _TrunkFn.apply(graph, cfg, x, tc.layers_MLP[0].weight, tc.layers_MLP[0].bias, tc.layers_MLP[1].weight, tc.layers_MLP[1].bias, *params)
    if out_rows is not None:      # (rows-only forward: the logits of the loss rows as they were computed, == out[mask]; TeacherGNN.get_3_embs hands them on)
        out._cb_rows = (out_rows, loss_rows[0])
    return out, se_reg_all
