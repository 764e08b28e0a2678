"""The non-finite cases of tests/test_nonfinite_host.py (CPU) and tests/test_gpu_nonfinite.py (device): one NaN, +Inf or -Inf in an operand of every
fused ReLU epilogue and of the attention kernel, the float64 restatement of each operation in plain torch (torch.relu keeps a NaN; the product's own
keep-masks are injected where an operation has a dropout) and its STRUCTURAL dependency set — which output elements the poisoned element reaches, read
off the shapes and the edge list alone, never off computed values.

A case is (operation, poison kind, poison position).  The position is one interior element of the operation's main input matrix ('input') or one
element of its bias ('bias').  An operation is an object with

    operands()                      seeded float32 / int64 CPU tensors by name (graph operations add 'ei', the int64 [2, E] edge list, and 'n')
    keep(o, mask_fn)                the keep-masks of its dropouts by name; mask_fn(shape, p, seed, offset) -> bool tensor (the host restatement of
                                    Philox in the CPU test, ops.dropout_keep_mask on the device)
    position(o, where, keep)        (operand name, index tuple) of the poisoned element — on an element the operand-side dropout keeps
    ref(o, keep)                    float64 outputs by name, the first one the primary output
    dep(o, where, pos)              bool masks by output name: the dependency set
    undecided(o, keep, where, pos)  bool masks by output name: elements this case's own dropout drops (a dropped NaN may be NaN or 0: not asserted)
    by                              'rows' or, for a bias, 'cols': the axis along which a case must leave something poisoned and something clean

Dependency sets assume what the seeded operands guarantee (test_nonfinite_host.py checks it through the NaN pattern of the restatement): no weight,
factor or edge value is exactly zero, so a poisoned term never meets a structural zero except a dropped element or a missing edge."""
import functools
import math

import numpy as np
import torch

import bf16_ref
import sage_ref as sr
from conftest import load_golden

KINDS = {'nan': float('nan'), 'pinf': float('inf'), 'ninf': float('-inf')}
SEED_A, SEED_Y = 0x1234ABCD5, 0x77      # operand-side and output-side dropout seeds


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _pos(g, *shape):
    return torch.rand(*shape, generator=g) + 0.5


def _f64(o):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in o.items()}


def _rows(shape, rows):
    m = torch.zeros(shape, dtype=torch.bool)
    m[rows] = True
    return m


def _cols(shape, cols):
    m = torch.zeros(shape, dtype=torch.bool)
    m[..., cols] = True
    return m


def _elem(shape, idx):
    m = torch.zeros(shape, dtype=torch.bool)
    m[idx] = True
    return m


def readers(ei, n, u):
    """bool [n]: the destination rows that have source u among their in-neighbours."""
    m = torch.zeros(n, dtype=torch.bool)
    m[ei[1][ei[0] == u]] = True
    return m


def pick_source(ei, n, into=None):
    """An interior node with out-edges that does not reach every row; with `into`, an in-neighbour of that row (the poison then crosses its — hub — sum)."""
    outdeg = torch.bincount(ei[0], minlength=n)
    for u in range(1, n - 1):
        r = readers(ei, n, u)
        if outdeg[u] > 0 and not r.all() and (into is None or r[into]):
            return u
    raise AssertionError('no usable source row')


def agg(ei, n, x, w=None):
    """A x (A_w x with edge values w) in the dtype of x, over the edge list."""
    src = x[ei[0]] if w is None else x[ei[0]] * w[:, None]
    return torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add(0, ei[1], src)


class Op:
    main, bias, by_bias = 'a', 'bias', 'cols'
    has_bias = True

    def keep(self, o, mask_fn):
        return {}

    def undecided(self, o, keep, where, pos):
        return {}

    def position(self, o, where, keep):
        if where == 'bias':
            return self.bias, (o[self.bias].shape[0] // 2,)
        r, c = o[self.main].shape
        return self.main, (r // 2, c // 2)

    def __repr__(self):
        return self.id


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dense epilogues
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Dense(Op):
    """y = relu(rowscale * (a @ b) + addend + bias): gemm.mm_nn / gemm.linear.  epi: 'plain' (no epilogue operand), 'bias', 'full' (all three)."""

    def __init__(self, M, K, N, epi, entry='mm_nn', path=''):
        self.M, self.K, self.N, self.epi, self.entry, self.path = M, K, N, epi, entry, path
        self.has_bias = epi != 'plain'
        self.id = f'{entry}-{M}x{K}x{N}-{epi}'

    def operands(self):
        g = _gen(self.M * 7 + self.K * 3 + self.N)
        o = {'a': _randn(g, self.M, self.K), 'b': _randn(g, self.K, self.N, scale=0.3)}
        if self.epi != 'plain':
            o['bias'] = _randn(g, self.N, scale=0.5)
        if self.epi == 'full':
            o['rowscale'], o['addend'] = _pos(g, self.M), _randn(g, self.M, self.N)
        return o

    def ref(self, o, keep):
        o = _f64(o)
        y = o['a'] @ o['b']
        if 'rowscale' in o:
            y = y * o['rowscale'][:, None] + o['addend']
        if 'bias' in o:
            y = y + o['bias']
        return {'y': torch.relu(y)}

    def dep(self, o, where, pos):
        shape = (self.M, self.N)
        return {'y': _cols(shape, pos[0]) if where == 'bias' else _rows(shape, pos[0])}


class Drop2(Op):
    """(y, yd) = (relu(a' @ b + bias), dropout(y)) with a' = dropout_{SEED_A}(a) (indrop) or a: gemm.mm_nn_indrop_drop2 / gemm.mm_nn_drop2 on the wide
    three-limb tile, which exists from 256 tiles of 128 rows on: M = 255 * 128 + 1."""

    def __init__(self, M, K, N, p, indrop):
        self.M, self.K, self.N, self.p, self.indrop = M, K, N, p, indrop
        self.id = f'{"mm_nn_indrop_drop2" if indrop else "mm_nn_drop2"}-{M}x{K}x{N}'

    def operands(self):
        g = _gen(self.M + self.K + int(self.indrop))
        return {'a': _randn(g, self.M, self.K), 'b': _randn(g, self.K, self.N, scale=0.3), 'bias': _randn(g, self.N, scale=0.5)}

    def keep(self, o, mask_fn):
        k = {'y': mask_fn((self.M, self.N), self.p, SEED_Y, 0)}
        if self.indrop:
            k['a'] = mask_fn((self.M, self.K), self.p, SEED_A, 0)
        return k

    def position(self, o, where, keep):
        name, idx = super().position(o, where, keep)
        if where == 'input' and self.indrop:      # the first kept element of the middle row from its middle column on
            r, c = idx
            c = c + int(torch.nonzero(keep['a'][r, c:])[0])
            idx = (r, c)
        return name, idx

    def ref(self, o, keep):
        o = _f64(o)
        a = o['a'] * keep['a'].double() / (1 - self.p) if self.indrop else o['a']
        y = torch.relu(a @ o['b'] + o['bias'])
        return {'y': y, 'yd': y * keep['y'].double() / (1 - self.p)}

    def dep(self, o, where, pos):
        shape = (self.M, self.N)
        m = _cols(shape, pos[0]) if where == 'bias' else _rows(shape, pos[0])
        return {'y': m, 'yd': m.clone()}

    def undecided(self, o, keep, where, pos):
        return {'yd': ~keep['y']}


class Front(Op):
    """(x0, z0): x0 = relu(dropout_{SEED_A}(x) @ w_in^T + b_in), z0 = rowscale * (dropout_{SEED_Y}(x0) @ w0) + addend — gemm.trunk_front, the forward
    front kernel (input width 64 / 128, hidden 256)."""
    main, bias = 'x', 'b_in'

    def __init__(self, M, K, p):
        self.M, self.K, self.p = M, K, p
        self.id = f'trunk_front-{M}x{K}-p{p}'

    def operands(self):
        g = _gen(self.M + self.K)
        return {'x': _randn(g, self.M, self.K), 'w_in': _randn(g, 256, self.K, scale=0.1), 'b_in': _randn(g, 256, scale=0.5),
                'w0': _randn(g, 256, 256, scale=0.07), 'rowscale': _pos(g, self.M), 'addend': _randn(g, self.M, 256)}

    def keep(self, o, mask_fn):
        if not self.p:
            return {'x': torch.ones(self.M, self.K, dtype=torch.bool), 'x0': torch.ones(self.M, 256, dtype=torch.bool)}
        return {'x': mask_fn((self.M, self.K), self.p, SEED_A, 0), 'x0': mask_fn((self.M, 256), self.p, SEED_Y, 0)}

    def position(self, o, where, keep):
        name, idx = super().position(o, where, keep)
        if where == 'input':
            r, c = idx
            idx = (r, c + int(torch.nonzero(keep['x'][r, c:])[0]))
        return name, idx

    def ref(self, o, keep):
        o = _f64(o)
        f = 1.0 / (1 - self.p)
        x0 = torch.relu((o['x'] * keep['x'].double() * f) @ o['w_in'].t() + o['b_in'])
        z0 = ((x0 * keep['x0'].double() * f) @ o['w0']) * o['rowscale'][:, None] + o['addend']
        return {'x0': x0, 'z0': z0}

    def dep(self, o, where, pos):
        shape = (self.M, 256)
        if where == 'bias':      # column n of x0 in every row; z0 = x0 @ w0 reads it in every row
            return {'x0': _cols(shape, pos[0]), 'z0': torch.ones(shape, dtype=torch.bool)}
        return {'x0': _rows(shape, pos[0]), 'z0': _rows(shape, pos[0])}

    def undecided(self, o, keep, where, pos):
        if where == 'bias':      # a row of z0 reads the poisoned x0[., n] through the second dropout: undecided where that element is dropped
            return {'z0': _rows((self.M, 256), ~keep['x0'][:, pos[0]])}
        return {}


def _store(act, mix_rows, keep, c_act, c_mix, p):
    """The trunk's store: dropout(c_act * act + c_mix * mix)."""
    return (c_act * act + c_mix * mix_rows) * keep.double() / (1 - p)


class StoreRowsGemm(Op):
    """(out, act): act = relu(rowscale * (a @ b) + bias), out = dropout(c_act * act + c_mix * mix[idx]) at the node rows idx — gemm.mm_nn_store_rows,
    the three-limb wide tile with the trunk's store as its epilogue (N = 256)."""
    C_ACT, C_MIX = 0.9, 0.1

    def __init__(self, M, K, n_nodes, p):
        self.M, self.K, self.n, self.p = M, K, n_nodes, p
        self.id = f'mm_nn_store_rows-{M}x{K}-p{p}'

    def operands(self):
        g = _gen(self.M + self.K + 1)
        idx = torch.sort(torch.randperm(self.n, generator=g)[:self.M])[0]
        return {'a': _randn(g, self.M, self.K), 'b': _randn(g, self.K, 256, scale=0.1), 'bias': _randn(g, 256, scale=0.5), 'rowscale': _pos(g, self.M),
                'idx': idx, 'mix': _randn(g, self.n, 256)}

    def keep(self, o, mask_fn):
        full = mask_fn((self.n, 256), self.p, SEED_Y, 0) if self.p else torch.ones(self.n, 256, dtype=torch.bool)
        return {'out': full[o['idx']]}

    def ref(self, o, keep):
        idx, o = o['idx'], _f64(o)
        act = torch.relu((o['a'] @ o['b']) * o['rowscale'][:, None] + o['bias'])
        return {'out': _store(act, o['mix'][idx], keep['out'], self.C_ACT, self.C_MIX, self.p), 'act': act}

    def dep(self, o, where, pos):
        shape = (self.M, 256)
        m = _cols(shape, pos[0]) if where == 'bias' else _rows(shape, pos[0])
        return {'out': m, 'act': m.clone()}

    def undecided(self, o, keep, where, pos):
        return {'out': ~keep['out']}


class StoreRows(StoreRowsGemm):
    """(out, act): act = relu(y), out = dropout(c_act * act + c_mix * mix[idx]) — trunk._store_rows (cb_trunk_store_rows_f32), the store as a row pass over
    the compact rows of a dense transform's output.  Elementwise: a poisoned y[i, c] reaches (i, c) alone."""
    main, has_bias = 'y', False

    def __init__(self, M, n_nodes, p):
        self.M, self.n, self.p = M, n_nodes, p
        self.id = f'trunk_store_rows-{M}-p{p}'

    def operands(self):
        g = _gen(self.M + 2)
        idx = torch.sort(torch.randperm(self.n, generator=g)[:self.M])[0]
        return {'y': _randn(g, self.M, 256), 'idx': idx, 'mix': _randn(g, self.n, 256)}

    def ref(self, o, keep):
        idx, o = o['idx'], _f64(o)
        act = torch.relu(o['y'])
        return {'out': _store(act, o['mix'][idx], keep['out'], self.C_ACT, self.C_MIX, self.p), 'act': act}

    def dep(self, o, where, pos):
        m = _elem((self.M, 256), pos)
        return {'out': m, 'act': m.clone()}

    def position(self, o, where, keep):      # an element the store's dropout keeps, so that the stored value is decided too
        r, c = self.M // 2, 128
        return 'y', (r, c + int(torch.nonzero(keep['out'][r, c:])[0]))


class GatherLinear(Op):
    """y = relu(A @ weight^T + bias) with A gathered while the GEMM stages it: form 'pair' A = h[u] * h[v] (ops.pair_linear), form 'rows'
    A = [h[i] | h[j]] (ops.rows_linear, idx [2, R]).  A poisoned h[j, c] reaches every output row whose index pair names j."""
    main = 'h'

    def __init__(self, form, n, D, R, out):
        self.form, self.n, self.D, self.R, self.out = form, n, D, R, out
        self.id = f'{form}_linear-{n}x{D}-R{R}-out{out}'

    def operands(self):
        g = _gen(self.n + self.R)
        idx = torch.randint(0, self.n, (2, self.R), generator=g)
        idx[0, 3] = idx[1, 5] = idx[0, self.R - 2] = idx[1, self.R - 2] = self.n // 2      # the poisoned row on either side, once on both
        k = self.D if self.form == 'pair' else 2 * self.D
        return {'h': _randn(g, self.n, self.D), 'idx': idx, 'weight': _randn(g, self.out, k, scale=0.3), 'bias': _randn(g, self.out, scale=0.5)}

    def ref(self, o, keep):
        idx, o = o['idx'], _f64(o)
        hu, hv = o['h'][idx[0]], o['h'][idx[1]]
        a = hu * hv if self.form == 'pair' else torch.cat([hu, hv], 1)
        return {'y': torch.relu(a @ o['weight'].t() + o['bias'])}

    def dep(self, o, where, pos):
        shape = (self.R, self.out)
        if where == 'bias':
            return {'y': _cols(shape, pos[0])}
        return {'y': _rows(shape, (o['idx'] == pos[0]).any(0))}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# aggregation epilogues and layers
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph_edges(which):
    """(ei int64 [2, E] on the CPU, n, the row the poison should cross or None)."""
    if which == 'powerlaw':      # tests/golden: 200 nodes, in-degrees up to 80 — 86 hub rows at hub_threshold 4, none at 256
        ei = load_golden('case_graph_powerlaw_d7_d64')['edge_index'].long()
        n = 200
        return ei, n, int(torch.bincount(ei[1], minlength=n).argmax())
    if which == 'small':         # tests/test_gpu_sage.py: N 165, no hub rows, three rows without in-edges
        return sr.make_graph(165, 900, seed=11, no_in=(5, 70, 140)), 165, None
    if which == 'hub':           # tests/test_gpu_sage.py / test_gpu_attn.py: N 300, a row of in-degree >= 200 (node 7) and one of out-degree >= 200
        return sr.make_graph(300, 1500, seed=12, no_in=(3, 130, 290), hub_in=(7, 200), hub_out=(11, 200)), 300, 7
    if which == 'tiles':         # the aggregation + GEMM kernel: 11 tiles of 64 rows, the last one ragged, a hub row at hub_threshold 16
        return sr.make_graph(700, 4000, seed=13, no_in=(9, 650), hub_in=(7, 90)), 700, 7
    raise KeyError(which)


class GraphOp(Op):
    main = 'h'

    def _graph(self):
        ei, n, into = graph_edges(self.which)
        return ei, n, pick_source(ei, n, into)

    def position(self, o, where, keep):
        if where == 'bias':
            return self.bias, (o[self.bias].shape[0] // 2,)
        return self.main, (self._graph()[2], o[self.main].shape[1] // 2)


class Spmm(GraphOp):
    """y = relu(row_scale * (A h) + bias) (CSRGraph.spmm), with edge values y = relu(row_scale * (A_w h) + bias) (CSRGraph.spmm_weighted).  Columns do not
    mix: a poisoned h[u, c] reaches column c of the rows that read u."""

    def __init__(self, which, d, hub_threshold, weighted=False, path=''):
        self.which, self.d, self.T, self.weighted, self.path = which, d, hub_threshold, weighted, path
        self.id = f'{"spmm_weighted" if weighted else "spmm"}-{which}-d{d}-T{hub_threshold}'

    def operands(self):
        ei, n, _ = self._graph()
        g = _gen(self.d + self.T)
        o = {'ei': ei, 'n': n, 'h': _randn(g, n, self.d), 'row_scale': _pos(g, n), 'bias': _randn(g, self.d, scale=0.5)}
        if self.weighted:
            o['w'] = _pos(g, ei.shape[1])
        return o

    def ref(self, o, keep):
        ei, n, o = o['ei'], o['n'], _f64(o)
        return {'y': torch.relu(agg(ei, n, o['h'], o.get('w')) * o['row_scale'][:, None] + o['bias'])}

    def dep(self, o, where, pos):
        shape = (o['n'], self.d)
        if where == 'bias':
            return {'y': _cols(shape, pos[0])}
        return {'y': _rows(shape, readers(o['ei'], o['n'], pos[0])) & _cols(shape, pos[1])}


class SpmmGemm(GraphOp):
    """(out, g_out) = (relu(row_scale * (A h) + bias), g_rowscale * (out @ w) + g_addend): CSRGraph.spmm_gemm, the aggregation + GEMM kernel (d = 256)."""

    def __init__(self, which, hub_threshold):
        self.which, self.T = which, hub_threshold
        self.id = f'spmm_gemm-{which}-T{hub_threshold}'

    def operands(self):
        ei, n, _ = self._graph()
        g = _gen(n + self.T)
        return {'ei': ei, 'n': n, 'h': _randn(g, n, 256), 'row_scale': _pos(g, n), 'bias': _randn(g, 256, scale=0.5), 'w': _randn(g, 256, 256, scale=0.07),
                'g_rowscale': _pos(g, n), 'g_addend': _randn(g, n, 256)}

    def ref(self, o, keep):
        ei, n, o = o['ei'], o['n'], _f64(o)
        out = torch.relu(agg(ei, n, o['h']) * o['row_scale'][:, None] + o['bias'])
        return {'out': out, 'g_out': (out @ o['w']) * o['g_rowscale'][:, None] + o['g_addend']}

    def dep(self, o, where, pos):
        shape = (o['n'], 256)
        if where == 'bias':
            return {'out': _cols(shape, pos[0]), 'g_out': torch.ones(shape, dtype=torch.bool)}
        r = readers(o['ei'], o['n'], pos[0])
        return {'out': _rows(shape, r) & _cols(shape, pos[1]), 'g_out': _rows(shape, r)}


class SpmmGemmStoreRows(GraphOp):
    """(H, out, act): H = (A (col_scale * h))[idx], act = relu(rowscale * (H @ w) + bias), out = dropout(c_act * act + c_mix * mix[idx]) — the sum-first
    layer of the rows-only forward in one kernel (CSRGraph.spmm_gemm_store_rows on the forward orientation restricted to the rows idx)."""
    C_ACT, C_MIX = 0.9, 0.1

    def __init__(self, which, hub_threshold, n_rows, p):
        self.which, self.T, self.M, self.p = which, hub_threshold, n_rows, p
        self.id = f'spmm_gemm_store_rows-{which}-T{hub_threshold}-rows{n_rows}-p{p}'

    def operands(self):
        ei, n, u = self._graph()
        g = _gen(n + self.M)
        rd = torch.nonzero(readers(ei, n, u)).reshape(-1)
        rest = torch.nonzero(~readers(ei, n, u)).reshape(-1)
        # the subset holds readers of the poisoned row (the heavy row among them), rows that do not read it, and the rows without in-edges
        idx = torch.unique(torch.cat([rd[:max(2, self.M // 8)], rest[torch.randperm(rest.numel(), generator=g)[:self.M]]]))[:self.M]
        idx = torch.unique(torch.cat([idx, torch.tensor([graph_edges(self.which)[2]])]))
        m = idx.numel()
        return {'ei': ei, 'n': n, 'h': _randn(g, n, 256), 'col_scale': _pos(g, n), 'w': _randn(g, 256, 256, scale=0.07), 'rowscale': _pos(g, m),
                'bias': _randn(g, 256, scale=0.5), 'idx': idx, 'mix': _randn(g, n, 256)}

    def keep(self, o, mask_fn):
        full = mask_fn((o['n'], 256), self.p, SEED_Y, 0) if self.p else torch.ones(o['n'], 256, dtype=torch.bool)
        return {'out': full[o['idx']]}

    def ref(self, o, keep):
        ei, n, idx, o = o['ei'], o['n'], o['idx'], _f64(o)
        H = agg(ei, n, o['h'] * o['col_scale'][:, None])[idx]
        act = torch.relu((H @ o['w']) * o['rowscale'][:, None] + o['bias'])
        return {'out': _store(act, o['mix'][idx], keep['out'], self.C_ACT, self.C_MIX, self.p), 'act': act, 'H': H}

    def dep(self, o, where, pos):
        shape = (o['idx'].numel(), 256)
        if where == 'bias':
            m = _cols(shape, pos[0])
            return {'out': m, 'act': m.clone(), 'H': torch.zeros(shape, dtype=torch.bool)}
        r = readers(o['ei'], o['n'], pos[0])[o['idx']]
        return {'out': _rows(shape, r), 'act': _rows(shape, r), 'H': _rows(shape, r) & _cols(shape, pos[1])}

    def undecided(self, o, keep, where, pos):
        return {'out': ~keep['out']}


class Sage(GraphOp):
    """out = relu((s * (A x)) W_n^T + x W_s^T + b): ops.sage_layer_raw, fused (cb_sage_layer_f32 / cb_ewlayer_f32) and composed (spmm + one GEMM).
    adj 'csr': s = 1 / in-degree (mode SAGE); adj 'weighted': A carries edge values, s = 1 (mode WSAGE).  A poisoned x[u, c] reaches every column of
    row u (the self block) and of the rows that read u."""
    main, bias = 'x', 'b'

    def __init__(self, which, adj, fused):
        self.which, self.adj, self.fused = which, adj, fused
        self.id = f'sage_layer-{which}-{adj}-{"fused" if fused else "composed"}'

    def operands(self):
        ei, n, _ = self._graph()
        g = _gen(n + len(self.adj))
        o = {'ei': ei, 'n': n, 'x': _randn(g, n, 256), 'W_n': _randn(g, 256, 256, scale=1 / 16), 'W_s': _randn(g, 256, 256, scale=1 / 16),
             'b': _randn(g, 256, scale=0.25)}
        if self.adj == 'weighted':
            o['w'] = _pos(g, ei.shape[1])
        return o

    def ref(self, o, keep):
        ei, n, o = o['ei'], o['n'], _f64(o)
        a = agg(ei, n, o['x'], o.get('w'))
        if self.adj == 'csr':
            a = a * sr.row_factor(ei, n, 'SAGE')[:, None]
        return {'out': torch.relu(a @ o['W_n'].t() + o['x'] @ o['W_s'].t() + o['b'])}

    def dep(self, o, where, pos):
        shape = (o['n'], 256)
        if where == 'bias':
            return {'out': _cols(shape, pos[0])}
        r = readers(o['ei'], o['n'], pos[0])
        r[pos[0]] = True
        return {'out': _rows(shape, r)}


class Attn(GraphOp):
    """(out, lse) = ops.attn_raw: out[v] = act(sum_j a_j V[u_j] + skip[v]), a = softmax of <Q[v], K[u_j]> / sqrt(D) over the in-edges of v, lse[v] = log
    sum_j exp(s_j); a row without in-edges gives act(skip[v]) and lse = -inf.  `operand` names the poisoned matrix: q (row v's scores: its whole row
    and lse), k (the scores of the rows that read u), v (column c of those rows, lse untouched) or skip (the element alone)."""
    has_bias = False

    def __init__(self, which, hub_threshold, d, relu, operand):
        self.which, self.T, self.d, self.relu, self.main = which, hub_threshold, d, relu, operand
        self.id = f'attn-{which}-T{hub_threshold}-d{d}-{"relu" if relu else "linear"}-{operand}'

    def operands(self):
        ei, n, _ = self._graph()
        g = _gen(n + self.d)
        return {'ei': ei, 'n': n, 'q': _randn(g, n, self.d), 'k': _randn(g, n, self.d), 'v': _randn(g, n, self.d), 'skip': _randn(g, n, self.d)}

    def position(self, o, where, keep):
        ei, n, into = graph_edges(self.which)
        if self.main in ('q', 'skip'):      # the heavy destination row itself, else the first interior row with in-edges: its q is read
            row = into if into is not None else int(torch.nonzero(torch.bincount(ei[1], minlength=n)[1:] > 0)[0]) + 1
            return self.main, (row, self.d // 2)
        return self.main, (self._graph()[2], self.d // 2)

    def ref(self, o, keep):
        ei, n, o = o['ei'], o['n'], _f64(o)
        src, dst = ei[0], ei[1]
        s = (o['q'][dst] * o['k'][src]).sum(-1) / math.sqrt(self.d)
        out, lse = torch.empty(n, self.d, dtype=torch.float64), torch.empty(n, dtype=torch.float64)
        for v in range(n):      # row by row, torch.softmax / logsumexp on the row's scores: no scatter, nothing shared with the kernel's running maximum
            e = torch.nonzero(dst == v).reshape(-1)
            if e.numel() == 0:
                out[v], lse[v] = o['skip'][v], float('-inf')
                continue
            a = torch.softmax(s[e], 0)
            out[v] = (a[:, None] * o['v'][src[e]]).sum(0) + o['skip'][v]
            lse[v] = torch.logsumexp(s[e], 0)
        return {'out': torch.relu(out) if self.relu else out, 'lse': lse}

    def dep(self, o, where, pos):
        n, shape = o['n'], (o['n'], self.d)
        none = torch.zeros(n, dtype=torch.bool)
        if self.main == 'q':
            has_in = bool((o['ei'][1] == pos[0]).any())
            r = _elem((n,), pos[0]) if has_in else none
            return {'out': _rows(shape, r), 'lse': r}
        if self.main == 'k':
            r = readers(o['ei'], n, pos[0])
            return {'out': _rows(shape, r), 'lse': r}
        if self.main == 'v':
            return {'out': _rows(shape, readers(o['ei'], n, pos[0])) & _cols(shape, pos[1]), 'lse': none}
        return {'out': _elem(shape, pos), 'lse': none}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------------------------------------
DENSE = [
    Dense(200, 9, 33, 'bias', path='fp32-input 4 x 1 tile (K % 4 != 0, N <= 64), scalar stores'),
    Dense(130, 17, 129, 'plain', path='fp32-input 2 x 2 tile, unaligned, two column blocks'),
    Dense(130, 17, 129, 'full', path='fp32-input 2 x 2 tile, unaligned, two column blocks'),
    Dense(65, 8, 4, 'plain', path='three-limb 4 x 1 tile, two row blocks of 64'),
    Dense(65, 8, 4, 'full', path='three-limb 4 x 1 tile, two row blocks of 64'),
    Dense(130, 16, 132, 'full', path='three-limb 128 x 128 tile, two row and two column blocks'),
    Dense(32641, 8, 256, 'bias', path='three-limb wide 128 x 256 tile (256 tiles: one per CU)'),
    Dense(257, 1433, 64, 'plain', path='fp32-input 4 x 1 tile, split-K: k_splitk_finish applies the epilogue'),
    Dense(257, 1433, 64, 'full', path='fp32-input 4 x 1 tile, split-K: k_splitk_finish applies the epilogue'),
    Dense(130, 16, 132, 'bias', entry='linear', path='gemm.linear on the three-limb 128 x 128 tile'),
    Dense(200, 9, 33, 'bias', entry='linear', path='gemm.linear on the fp32-input 4 x 1 tile'),
]
FUSED_DENSE = [
    Drop2(32641, 8, 256, 0.5, indrop=False), Drop2(32641, 8, 256, 0.5, indrop=True),
    Front(70, 128, 0.0), Front(513, 64, 0.2),
    StoreRowsGemm(77, 8, 300, 0.0), StoreRowsGemm(77, 8, 300, 0.5), StoreRows(77, 300, 0.0), StoreRows(77, 300, 0.5),
    GatherLinear('pair', 50, 16, 70, 8), GatherLinear('rows', 50, 16, 70, 8),
]
SPMM = [Spmm('powerlaw', d, T, path=p) for T in (256, 4) for d, p in ((7, 'narrow group, scalar rows'), (16, 'narrow group, float4 rows'),
                                                                        (40, 'narrow group, 40 columns'), (256, 'wide rows, one wavefront per row'))]
SPMM += [Spmm('powerlaw', 96, 256, weighted=True, path='cb_spmm_csr_weighted_f32, one wavefront per row')]
AGG_GEMM = [SpmmGemm('tiles', 16), SpmmGemm('tiles', 256), SpmmGemmStoreRows('tiles', 16, 150, 0.0), SpmmGemmStoreRows('tiles', 256, 150, 0.5)]
LAYERS = [Sage(which, adj, fused) for which in ('small', 'hub') for adj in ('csr', 'weighted') for fused in (True, False)]
ATTN = [Attn('hub', 64, 64, relu, operand) for relu in (True, False) for operand in ('q', 'k', 'v', 'skip')]
ATTN += [Attn('hub', 4096, 64, True, 'k'), Attn('small', 4096, 256, True, 'q'), Attn('small', 4096, 256, True, 'v')]
OPS = DENSE + FUSED_DENSE + SPMM + AGG_GEMM + LAYERS + ATTN


def _cases():
    out = []
    for op in OPS:
        for where in ('input', 'bias'):
            if where == 'bias' and not op.has_bias:
                continue
            for kind in KINDS:
                out.append((op, kind, where))
    return out


CASES = _cases()


def case_id(c):
    return f'{c[0].id}-{c[2]}-{c[1]}'


@functools.lru_cache(maxsize=4)
def operands_of(op):
    """op.operands(), made once and shared: read-only (poisoned() copies the one tensor it changes)."""
    return op.operands()


def poisoned(o, name, idx, kind):
    """A copy of the operands with o[name][idx] = the poison; the clean operands stay as they are."""
    p = dict(o)
    p[name] = o[name].clone()
    p[name][idx] = KINDS[kind]
    return p


def host_mask(shape, p, seed, offset=0):
    """The product's keep-mask from the host restatement of Philox4x32-10 (oracle/coldbrew_oracle.py; pinned to the device bit for bit elsewhere)."""
    import coldbrew_oracle as orc
    return torch.from_numpy(np.ascontiguousarray(orc.dropout_keep_mask(tuple(shape), p, seed, offset)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# ReLU on a value table
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def relu_table_bits():
    """uint32 fp32 patterns: +-0, +-smallest subnormal, +-largest subnormal, +-smallest normal, +-1, +-FLT_MAX, +-Inf, and the NaNs of tests/bf16_ref.py
    (quiet, all-ones and payload NaNs of either sign, and the NaNs whose upper half is an infinity's)."""
    finite = [m | s for m in (0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000) for s in (0, 0x80000000)]
    nan = bf16_ref.edge_table([0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7FFF, 0xFFFF])
    nan = nan[bf16_ref.is_nan_bits(nan)]
    return np.concatenate([np.asarray(finite, dtype=np.uint32), nan.astype(np.uint32)])


def relu_bits_restated(u32):
    """The bits ReLU leaves of every pattern that is not a NaN, on integers: a set sign bit (negative values and -0.0) gives +0.0, everything else itself —
    what fmaxf(v, 0.f) returned on the device.  For a NaN the requirement is "a NaN", not a pattern."""
    u = np.asarray(u32, dtype=np.uint32)
    return np.where((u >> np.uint32(31)) == 1, np.uint32(0), u).astype(np.uint32)
