"""GPU: a NaN or an infinity in an operand comes out of every fused ReLU epilogue, and of the attention kernel, where the float64 restatement says it
must — the device's ReLU (csrc/cb_common.h relu_nan) keeps a NaN as torch.relu does — and nowhere else.  The cases, their restatements and their
structural dependency sets are tests/nonfinite_cases.py (checked on the CPU by tests/test_nonfinite_host.py).  Each case runs the product twice, on the
clean and on the poisoned operands, through the Python entry points, and asserts

    a. NaN poison: isnan(got) == isnan(ref), element for element;
    b. +-Inf poison: got is not finite wherever ref is NaN or +Inf — nothing more there (a three-limb split of an infinity legitimately gives NaN where
       fp32 gives Inf: profiles/bf16_rounding.md);
    c. every output element outside the dependency set — whole rows for a poisoned input, whole columns for a poisoned bias — equals the clean run's
       (torch.equal: the kernels are fixed-order, nothing may leak through shared staging);
    d. cb_device_status() == 0 after synchronising.

Elements the case's own dropout drops are left out of a and b (whether a dropped NaN is NaN or 0 is not decided here); the poison sits on an element
that an operand-side dropout keeps; the sign of a zero is never asserted.  The path each shape takes is named in nonfinite_cases (`path`, class
docstrings) and asserted wherever the API reports it."""
import functools
import math

import numpy as np
import pytest
import torch

import nonfinite_cases as nc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from gnn_tail_generalization_amd import _lib
    return _lib


def _status_ok():
    torch.cuda.synchronize()
    assert _lib().load().cb_device_status() == 0


def _dev_mask(shape, p, seed, offset=0):
    from gnn_tail_generalization_amd import ops
    return ops.dropout_keep_mask(tuple(shape), p, seed, DEV, offset).cpu()


def _to_dev(o):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in o.items()}


class _Rows:
    def __init__(self, idx):
        self.idx, self.n = idx, int(idx.numel())


@functools.lru_cache(maxsize=None)
def _graph(which, T, keep_edge_order=False):
    from gnn_tail_generalization_amd.graph import CSRGraph
    ei, n, _ = nc.graph_edges(which)
    return CSRGraph(ei.to(DEV), n, hub_threshold=T, keep_edge_order=keep_edge_order)


# ---- one runner per operation: the product's outputs under the names of the restatement's ---------------------------------------------------------
def _run_dense(op, o):
    """gemm.mm_nn / gemm.linear; the tile family is op.path.  Split-K is the one the library reports (cb_gemm_nn_splitk_workspace_bytes)."""
    from gnn_tail_generalization_amd import gemm
    assert (_lib().load().cb_gemm_nn_splitk_workspace_bytes(op.M, op.N, op.K) > 0) == ('split-K' in op.path)
    if op.entry == 'linear':
        return {'y': gemm.linear(o['a'], o['b'].t().contiguous(), o['bias'], relu=True)}
    return {'y': gemm.mm_nn(o['a'], o['b'], rowscale=o.get('rowscale'), addend=o.get('addend'), bias=o.get('bias'), relu=True)}


def _run_drop2(op, o):
    """The dual-output epilogue of the wide three-limb tile (cb_gemm_nn_indrop_supported is its predicate for both entries)."""
    from gnn_tail_generalization_amd import gemm
    if op.indrop:
        res = gemm.mm_nn_indrop_drop2(o['a'], o['b'], op.p, nc.SEED_A, nc.SEED_Y, bias=o['bias'], relu=True)
        assert res is not None
    else:
        y = torch.empty((op.M, op.N), device=DEV)
        P = _lib().ptr
        assert _lib().load().cb_gemm_nn_indrop_supported(P(o['a']), op.K, P(o['b']), op.N, P(y), op.N, P(y), op.N, op.M, op.N, op.K)
        res = gemm.mm_nn_drop2(o['a'], o['b'], op.p, nc.SEED_Y, bias=o['bias'], relu=True)
    return {'y': res[0], 'yd': res[1]}


def _run_front(op, o):
    """cb_trunk_front_f32 (None where the kernel does not exist for the shape)."""
    from gnn_tail_generalization_amd import gemm
    fr = gemm.trunk_front(o['x'], o['w_in'], o['b_in'], o['w0'], o['rowscale'], o['addend'], op.p, nc.SEED_A, nc.SEED_Y)
    assert fr is not None
    return {'x0': fr[0], 'z0': fr[3]}


def _bits(n):
    return torch.zeros((n, 1, 4), dtype=torch.int64, device=DEV)


def _run_store_rows_gemm(op, o):
    """cb_gemm_nn_store_rows_f32 (None where the fused form does not exist)."""
    from gnn_tail_generalization_amd import gemm
    res = gemm.mm_nn_store_rows(o['a'], o['b'], o['rowscale'], None, o['bias'], o['idx'], o['mix'], None, op.C_ACT, op.C_MIX, op.p, nc.SEED_Y, 0, _bits(op.n),
                                False, want_act=True)
    assert res is not None
    return {'out': res[0], 'act': res[1]}


def _run_store_rows(op, o):
    """cb_trunk_store_rows_f32."""
    from gnn_tail_generalization_amd import trunk
    out, act = trunk._store_rows(o['y'], o['idx'], o['mix'], op.C_ACT, op.C_MIX, op.p, nc.SEED_Y, 0, _bits(op.n), False, want_act=True)
    return {'out': out, 'act': act}


def _run_gather(op, o):
    """cb_pair_gemm_nn_f32 / cb_rows_gemm_nn_f32: fused=True raises where the gathered-operand form does not exist."""
    from gnn_tail_generalization_amd import ops
    fn = ops.pair_linear if op.form == 'pair' else ops.rows_linear
    return {'y': fn(o['h'], o['idx'], o['weight'], o['bias'], relu=True, fused=True)}


def _run_spmm(op, o):
    """cb_spmm_csr_f32 (hub rows: partial sums + cb_spmm_small.hip's finish) / cb_spmm_csr_weighted_f32."""
    G = _graph(op.which, op.T, op.weighted)
    assert (G._plan.n_hubs > 0) == (op.T == 4)
    if op.weighted:
        return {'y': G.spmm_weighted(o['h'], o['w'][G.edge_perm()].contiguous(), row_scale=o['row_scale'], bias=o['bias'], relu=True)}
    return {'y': G.spmm(o['h'], row_scale=o['row_scale'], bias=o['bias'], relu=True)}


def _run_spmm_gemm(op, o):
    """cb_spmm_gemm_f32."""
    from gnn_tail_generalization_amd.graph import weight_image
    G = _graph(op.which, op.T)
    assert (G._plan.n_hubs > 0) == (op.T == 16)
    out, g = G.spmm_gemm(o['h'], weight_image(o['w']), row_scale=o['row_scale'], bias=o['bias'], relu=True, g_rowscale=o['g_rowscale'], g_addend=o['g_addend'])
    return {'out': out, 'g_out': g}


def _run_spmm_gemm_store_rows(op, o):
    """cb_spmm_gemm_store_rows_f32 on the forward orientation restricted to the rows idx."""
    from gnn_tail_generalization_amd.graph import weight_image
    G = _graph(op.which, op.T)
    fwd = G._support_fwd(_Rows(o['idx']), G.N, force=True)
    assert (fwd._plan.n_hubs > 0) == (op.T == 16)
    H, out, act = fwd.spmm_gemm_store_rows(o['h'], o['col_scale'], weight_image(o['w']), o['rowscale'], o['bias'], o['idx'], o['mix'], None, op.C_ACT, op.C_MIX,
                                           op.p, nc.SEED_Y, 0, _bits(G.N), False, want_act=True)
    return {'out': out, 'act': act, 'H': H}


@functools.lru_cache(maxsize=None)
def _adj(which, T):
    from gnn_tail_generalization_amd.graph import WeightedAdj
    ei, n, _ = nc.graph_edges(which)
    w = nc.operands_of(nc.Sage(which, 'weighted', True))['w']
    return WeightedAdj.from_edges(ei.to(DEV), w.to(DEV), n, hub_threshold=T)


def _run_sage(op, o):
    """ops.sage_layer_raw: 'fused' = cb_sage_layer_f32 (CSRGraph) / cb_ewlayer_f32 (WeightedAdj), 'composed' = aggregation + cb_gemm_nn_f32, K = 512."""
    from gnn_tail_generalization_amd import ops
    T = 16 if op.which == 'hub' else 256
    G = _graph(op.which, T, True)
    assert (G._plan.n_hubs > 0) == (op.which == 'hub')
    if op.adj == 'weighted':
        adj = _adj(op.which, T)
        assert torch.equal(adj.edge_weight, o['w'])
        out, _, path = ops.sage_layer_raw(adj, o['x'], o['W_n'], o['W_s'], o['b'], None, relu=True, fused=op.fused)
    else:
        out, _, path = ops.sage_layer_raw(G, o['x'], o['W_n'], o['W_s'], o['b'], ops.inv_indeg(G), relu=True, fused=op.fused)
    assert path == ('fused' if op.fused else 'composed') and ops.sage_paths[-1] == ('fwd', path)
    return {'out': out}


def _run_attn(op, o):
    """cb_attn_fwd_f32; hub_threshold 64 makes the heavy row a hub row (chunk states merged), 4096 leaves every row to one group."""
    from gnn_tail_generalization_amd import ops
    G = _graph(op.which, op.T)
    assert (G._plan.n_hubs > 0) == (op.T == 64)
    out, lse = ops.attn_raw(G, o['q'], o['k'], o['v'], o['skip'], relu=op.relu)
    return {'out': out, 'lse': lse}


RUN = {nc.Dense: _run_dense, nc.Drop2: _run_drop2, nc.Front: _run_front, nc.StoreRowsGemm: _run_store_rows_gemm, nc.StoreRows: _run_store_rows,
       nc.GatherLinear: _run_gather, nc.Spmm: _run_spmm, nc.SpmmGemm: _run_spmm_gemm, nc.SpmmGemmStoreRows: _run_spmm_gemm_store_rows, nc.Sage: _run_sage,
       nc.Attn: _run_attn}


@functools.lru_cache(maxsize=2)
def _clean(op):
    """(device operands, keep-masks, the clean run's outputs on the CPU): once per operation, shared by its cases and left unchanged."""
    od = _to_dev(nc.operands_of(op))
    keep = op.keep(nc.operands_of(op), _dev_mask)
    out = {k: v.cpu() for k, v in RUN[type(op)](op, od).items()}
    _status_ok()
    return od, keep, out


@pytest.mark.parametrize('case', nc.CASES, ids=nc.case_id)
def test_poison_comes_out_where_it_must_and_nowhere_else(case):
    op, kind, where = case
    o = nc.operands_of(op)
    od, keep, clean = _clean(op)
    name, idx = op.position(o, where, keep)
    ref = op.ref(nc.poisoned(o, name, idx, kind), keep)
    dep, und = op.dep(o, where, idx), op.undecided(o, keep, where, idx)
    pd = dict(od)
    pd[name] = od[name].clone()
    pd[name][idx] = nc.KINDS[kind]
    got = {k: v.cpu() for k, v in RUN[type(op)](op, pd).items()}
    _status_ok()                                                                  # d
    assert set(got) == set(ref)
    for out, r in ref.items():
        g, decided = got[out], ~und.get(out, torch.zeros(r.shape, dtype=torch.bool))
        assert g.shape == r.shape
        outside = ~dep[out]
        leaked = int((g[outside] != clean[out][outside]).sum())
        if kind == 'nan':                                                         # a
            gn, rn = torch.isnan(g), torch.isnan(r)
            lost, extra = int((rn & ~gn & decided).sum()), int((gn & ~rn & decided).sum())
            print(f'{nc.case_id(case)} {out}: NaN expected {int((rn & decided).sum())}, lost {lost}, spurious {extra}, leaked {leaked}')
            assert lost == 0 and extra == 0, (out, lost, extra)
        else:                                                                     # b
            must = (torch.isnan(r) | (r == float('inf'))) & decided
            finite = int(torch.isfinite(g[must]).sum())
            print(f'{nc.case_id(case)} {out}: non-finite expected {int(must.sum())}, finite there {finite}, leaked {leaked}')
            assert finite == 0, (out, finite)
        assert leaked == 0 and torch.equal(g[outside], clean[out][outside]), out  # c


@pytest.mark.parametrize('relu', [True, False])
def test_attention_rows_without_in_edges(relu):
    """A row without in-edges gives act(skip) and lse = -inf, also while another row's scores are NaN; a NaN score gives a NaN row and a NaN lse — not the
    empty row's act(skip) and -inf, which is what `l > 0 ? ... : ...` made of a NaN l."""
    from gnn_tail_generalization_amd import ops
    op = nc.Attn('hub', 64, 64, relu, 'k')
    o = nc.operands_of(op)
    ei, n, _ = nc.graph_edges('hub')
    no_in = torch.bincount(ei[1], minlength=n) == 0
    assert int(no_in.sum()) >= 3
    name, idx = op.position(o, 'input', {})
    pd = _to_dev(nc.poisoned(o, name, idx, 'nan'))
    out, lse = ops.attn_raw(_graph('hub', 64), pd['q'], pd['k'], pd['v'], pd['skip'], relu=relu)
    _status_ok()
    out, lse = out.cpu(), lse.cpu()
    want = torch.relu(o['skip']) if relu else o['skip']
    assert torch.equal(out[no_in], want[no_in]) and bool((lse[no_in] == float('-inf')).all())
    hit = nc.readers(ei, n, idx[0])
    assert bool(torch.isnan(out[hit]).all()) and bool(torch.isnan(lse[hit]).all())
    assert bool(torch.isfinite(out[~hit]).all()) and bool(torch.isfinite(lse[~hit & ~no_in]).all())


@pytest.mark.parametrize('d', [4, 64, 256])
def test_relu_on_a_value_table(d):
    """A graph of N self loops: the adjacency is the identity and spmm(h, relu=True) == relu(h) exactly (0 + h, times 1, plus 0).  d = 4 / 64: the narrow
    groups; 256: the wide rows.  Off NaN the output bits are the ones fmaxf(v, 0.f) gave on the device — +0.0 for -0.0 and for every negative, the value
    itself above zero, subnormals and infinities included — compared as integers against nonfinite_cases.relu_bits_restated; a NaN stays a NaN."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    bits = nc.relu_table_bits()
    n = 131      # three row blocks of 64, the last one ragged; every pattern meets every column phase (131 * d is no multiple of the table's length)
    flat = np.resize(bits, n * d)
    h = torch.from_numpy(flat.view(np.int32).copy()).view(torch.float32).reshape(n, d).to(DEV)
    G = CSRGraph(torch.arange(n, device=DEV).repeat(2, 1), n)
    y = G.spmm(h, relu=True)
    _status_ok()
    got = y.cpu().view(torch.int32).numpy().view(np.uint32).reshape(-1)
    nan = nc.bf16_ref.is_nan_bits(flat)
    want = nc.relu_bits_restated(flat)
    bad = np.nonzero(got[~nan] != want[~nan])[0]
    lost = int((~nc.bf16_ref.is_nan_bits(got[nan])).sum())
    print(f'd={d}: {len(bad)} of {int((~nan).sum())} non-NaN patterns differ, {lost} of {int(nan.sum())} NaNs lost')
    assert len(bad) == 0, [(hex(int(flat[~nan][i])), hex(int(got[~nan][i]))) for i in bad[:8]]
    assert lost == 0


def test_consumers_of_the_unread_rows():
    """The rows a rows-only training forward may not be asked for come back as ops.unread_rows_fill() (NaN).  A consumer that reads them through a fused
    ReLU anyway — graph.spmm(relu=True), ops.sage_layer(relu=True) — gets NaN in every destination row that has such a row among its in-neighbours (the
    layer's self block: in those rows themselves too), never a plausible zero."""
    from helpers import product_model
    from conftest import load_golden
    from gnn_tail_generalization_amd import ops, tuning
    g = load_golden('case_r_initialbn_h256_L3_train10')
    args, model = product_model(g['cfg'], g['sd'], DEV)
    x, ei, mask = g['x'].to(DEV), g['edge_index'].to(DEV), g['train_mask'].to(DEV)
    model.train()
    G = model.model.model._graph(ei)
    G.rowsparse_small_ok = True
    keep_min, tuning.T.rows_only_min_nodes = tuning.T.rows_only_min_nodes, 0
    try:
        res = model.get_3_embs(x, ei, mask, loss_rows=(mask, int(mask.sum())), rows_only=True)
    finally:
        tuning.T.rows_only_min_nodes = keep_min
    h = res.emb4classi_full.detach()
    n, c = h.shape
    assert math.isnan(ops.unread_rows_fill()) and bool(torch.isnan(h[~mask]).all()) and bool(torch.isfinite(h[mask]).all())
    unread = (~mask).cpu()
    src, dst = g['edge_index'][0], g['edge_index'][1]
    reads_unread = torch.zeros(n, dtype=torch.bool)
    reads_unread[dst[unread[src]]] = True
    assert bool(reads_unread.any()) and not bool(reads_unread.all())
    gen = torch.Generator().manual_seed(3)
    bias = (torch.randn(c, generator=gen) * 0.5).to(DEV)
    y = G.spmm(h, row_scale=G.norm_in, bias=bias, relu=True).cpu()
    assert torch.equal(torch.isnan(y).all(1), reads_unread) and torch.equal(torch.isnan(y).any(1), reads_unread)
    W_n, W_s = (torch.randn(8, c, generator=gen) * 0.3).to(DEV), (torch.randn(8, c, generator=gen) * 0.3).to(DEV)
    b8 = (torch.randn(8, generator=gen) * 0.5).to(DEV)
    z = ops.sage_layer(G, h, W_n, W_s, b8, mode='SAGE', relu=True).cpu()
    _status_ok()
    want = reads_unread | unread
    assert torch.equal(torch.isnan(z).all(1), want) and torch.equal(torch.isnan(z).any(1), want)
    assert not bool(want.all())

