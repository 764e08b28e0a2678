"""Host-side checks (no GPU) of the edge-weighted encoder layers and the adjacency normalisations: the float64 restatement of tests/ew_ref.py against a
dense-matrix form, set_diag's semantics, the restatement's fp32 normalisations against the dense torch expression of the reference's lines
(Link_prediction_model/utils.py:93-106), the C ABI of the new entries, what is refused on CPU tensors, and the tool's --normalize_adj."""
import ctypes
import os
import re
import sys

import pytest
import torch

import ew_ref as er
import sage_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_spmm_csr_ew_f32', 'cb_ewlayer_f32', 'cb_adjnorm_rowsum_f64', 'cb_adjnorm_scale_f32']
PLUMBING = ['--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1']


def _dense(ei, n, w):
    """A[dst, src] = the sum of the values stored at (src -> dst), float64."""
    return torch.zeros((n, n), dtype=torch.float64).index_put((ei[1], ei[0]), w.double(), accumulate=True)


def _weights(e, seed):
    """k / 1024 with 1 <= k <= 8192: every summation order gives the same sum."""
    return torch.randint(1, 8193, (e,), generator=torch.Generator().manual_seed(seed)).float() / 1024


@pytest.mark.parametrize('has_self', [True, False])
def test_the_restatement_equals_a_dense_formulation(has_self):
    n = 30
    ei = sr.make_graph(n, 90, seed=4, no_in=(2, 9, 20), n_self=4, n_dup=9)
    g = torch.Generator().manual_seed(0)
    w = torch.randn(ei.shape[1], generator=g, dtype=torch.float64)
    w[::7] = 0.0
    x = torch.randn(n, 6, generator=g, dtype=torch.float64, requires_grad=True)
    W_n = torch.randn(5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    W_s = torch.randn(5, 6, generator=g, dtype=torch.float64, requires_grad=True) if has_self else None
    b = torch.randn(5, generator=g, dtype=torch.float64, requires_grad=True)
    A = _dense(ei, n, w)
    got, agg = er.layer(ei, n, w, x, W_n, W_s, b, relu=True)
    want = (A @ x) @ W_n.t() + b
    if has_self:
        want = want + x @ W_s.t()
    want = torch.relu(want)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13) and torch.allclose(agg, A @ x, rtol=1e-13, atol=1e-13)
    assert (agg[[2, 9, 20]] == 0).all()
    leaves = [t for t in (x, W_n, W_s, b) if t is not None]
    g1, g2 = torch.autograd.grad(got.sum(), leaves), torch.autograd.grad(want.sum(), leaves)
    assert all(torch.allclose(a, c, rtol=1e-12, atol=1e-12) for a, c in zip(g1, g2))
    assert torch.allclose(er.agg_t(ei, n, w, x.detach()), A.t() @ x.detach(), rtol=1e-13, atol=1e-13)
    # with every value 1 it is sage_ref's unweighted sum
    assert torch.equal(er.agg(ei, n, torch.ones_like(w), x.detach()), sr.agg_sum(ei, n, x.detach()))


def test_set_diag_semantics():
    """An existing self loop of value 3 becomes 1; a repeated self loop becomes one entry; a node without one gains it; nothing else moves."""
    n = 4
    ei = torch.tensor([[0, 0, 1, 1, 2, 3], [0, 1, 1, 1, 0, 2]])      # (0,0) once with value 3; (1,1) twice; 2 and 3 without a loop
    w = torch.tensor([3.0, 0.5, 2.0, 4.0, 0.25, 8.0])
    ei2, w2 = er.set_diag(ei, n, w)
    loops = ei2[0] == ei2[1]
    assert int(loops.sum()) == n and sorted(ei2[0][loops].tolist()) == [0, 1, 2, 3] and (w2[loops] == 1).all()
    rest = sorted(zip(ei2[0][~loops].tolist(), ei2[1][~loops].tolist(), w2[~loops].tolist()))
    assert rest == [(0, 1, 0.5), (2, 0, 0.25), (3, 2, 8.0)]
    A = _dense(ei, n, w)
    A.fill_diagonal_(1.0)
    assert torch.equal(_dense(ei2, n, w2), A)


def _simple_graph(n, seed):
    """A directed graph without repeated edges (so that a dense matrix holds each value in an element of its own), with self loops and empty rows."""
    ei = sr.make_graph(n, 150, seed=seed, no_in=(1, 17), n_self=5, n_dup=0)
    key = torch.unique(ei[1] * n + ei[0])
    return torch.stack([key % n, key // n])


@pytest.mark.parametrize('kind', ['adj', 'gcn'])
def test_the_fp32_normalisations_against_the_dense_torch_expression(kind):
    """utils.py:93-106 on a dense fp32 matrix.  Structure: exact.  deg: the same bits (the weights k / 1024 sum exactly in any order).  The factor, where
    torch's pow enters: within 1 ulp of the restatement's rounded float64 form.  The values, where it does not (the reference's products fed the
    restatement's factor): the same bits."""
    n = 40
    ei = _simple_graph(n, 8)
    w = _weights(ei.shape[1], 3)
    ei2, w2, deg, f = er.normalize(ei, n, w, kind)
    A = torch.zeros((n, n), dtype=torch.float32).index_put((ei[1], ei[0]), w, accumulate=True)
    if kind == 'gcn':
        A.fill_diagonal_(1.0)                                   # set_diag
    d = A.sum(dim=1).to(torch.float)
    assert torch.equal(d, deg)
    t = d.pow(-0.5 if kind == 'gcn' else -1)
    t[t == float('inf')] = 0
    ulps = er.ulp_distance(t, f)
    print(f'{kind}: factor differs from torch pow in {int((ulps > 0).sum())} of {n} rows, at most {int(ulps.max())} ulp')
    assert int(ulps.max()) <= 1
    if kind == 'adj':
        assert int((deg == 0).sum()) >= 2 and (f[deg == 0] == 0).all()      # rows without in-edges: inf -> 0
    want = f.view(-1, 1) * A
    if kind == 'gcn':
        want = want * f.view(1, -1)
    got = torch.zeros((n, n), dtype=torch.float32).index_put((ei2[1], ei2[0]), w2, accumulate=True)
    stored = torch.zeros((n, n), dtype=torch.bool).index_put((ei2[1], ei2[0]), torch.ones(ei2.shape[1], dtype=torch.bool))
    assert torch.equal(stored, A != 0)
    assert torch.equal(got, want)


def test_the_factor_arithmetic_is_not_torchs_pow_everywhere():
    """Why the tests compare against the float64 form: fp32 pow(-0.5) differs from the rounded float64 1 / sqrt(d) on a fair share of degrees, by 1 ulp."""
    d = torch.rand(20000, generator=torch.Generator().manual_seed(1)) * 1000 + 0.5
    ulps = er.ulp_distance(d.pow(-0.5), er.inv_factor(d, 'gcn'))
    assert int(ulps.max()) <= 1
    assert int(er.ulp_distance(d.pow(-1), er.inv_factor(d, 'adj')).max()) <= 1


def test_c_abi_of_the_new_entries():
    from gnn_tail_generalization_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'coldbrew_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(cb_[a-z0-9_]+)\s*\(', hdr))
    assert os.path.isfile(_lib.LIB_PATH), 'build the extension first: python __graft_entry__.py'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        n_args = len([a for a in re.search(name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',') if a.strip() and a.strip() != 'void'])
        assert n_args == len(_lib.SIGNATURES[name][1]), (name, n_args, len(_lib.SIGNATURES[name][1]))


def test_bad_arguments_are_answered_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    P16, P4 = ctypes.c_void_p(256), ctypes.c_void_p(260)
    view = _lib.CsrView(16, 16, 0, 64, 10, 256, 0, 0, None, None, None, 0)
    ew = lambda v, w, h, d, ld: lib.cb_spmm_csr_ew_f32(ctypes.byref(v) if v is not None else None, w, h, ld, d, P16, ld, None)
    assert ew(None, P16, P16, 256, 256) == -1 and b'cb_spmm_csr_ew_f32' in lib.cb_last_error()
    assert ew(view, None, P16, 256, 256) == -1                        # edges without values
    assert ew(view, P16, P16, 128, 128) == -1 and b'cb_spmm_csr_weighted_f32' in lib.cb_last_error()      # other widths: the plain kernel
    assert ew(view, P16, P4, 256, 256) == -1 and ew(view, P16, P16, 256, 258) == -1
    assert ew(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, None, 0), P16, P16, 256, 256) == -3      # hub plan without its workspace
    empty = _lib.CsrView(None, None, 0, 0, 0, 256, 0, 0, None, None, None, 0)
    assert ew(empty, None, None, 256, 256) == 0
    layer = lambda v, w, h, p, relu, agg_only=0: lib.cb_ewlayer_f32(ctypes.byref(v), w, h, 256, h, 256, P16, None, relu, p, ctypes.c_uint64(0), None, 0, None, 0,
                                                                   agg_only, P16, 256, None)
    assert layer(view, None, P16, 0.0, 0) == -1 and b'cb_ewlayer_f32' in lib.cb_last_error()
    assert layer(view, P16, P4, 0.0, 0) == -1 and b'cb_sage_layer_supported' in lib.cb_last_error()
    assert layer(view, P16, P16, 0.5, 0) == -1 and layer(view, P16, P16, 0.0, 0, agg_only=1) == -1
    assert layer(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, 16, 1 << 20), P16, P16, 0.0, 0) == -1      # hub rows need agg_out
    assert layer(empty, None, None, 0.0, 0) == 0
    assert lib.cb_adjnorm_rowsum_f64(None, P16, 4, 4, 1, P16, P16, P16, None) == -1
    assert lib.cb_adjnorm_rowsum_f64(P16, P16, 4, 4, 1, P16, P16, None, None) == -1
    assert lib.cb_adjnorm_rowsum_f64(P16, P16, 2 ** 31, 4, 1, P16, P16, P16, None) == -2
    assert lib.cb_adjnorm_rowsum_f64(None, None, 0, 0, 1, None, None, None, None) == 0
    assert lib.cb_adjnorm_scale_f32(P16, None, P16, 4, 4, P16, None, P16, None) == -1
    assert lib.cb_adjnorm_scale_f32(P16, P16, P16, 4, -1, P16, None, P16, None) == -1
    assert lib.cb_adjnorm_scale_f32(None, None, None, 4, 0, None, None, None, None) == 0


def test_cpu_tensors_are_refused():
    from gnn_tail_generalization_amd import _lib, ops
    from gnn_tail_generalization_amd.graph import WeightedAdj
    from gnn_tail_generalization_amd.Link_prediction_model import utils as lp_utils
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    with pytest.raises(_lib.HipExtensionError):
        WeightedAdj(None, torch.ones(3))
    with pytest.raises(_lib.HipExtensionError):
        WeightedAdj.from_edges(ei, torch.ones(3), 3)
    with pytest.raises(ValueError, match='kind'):
        ops.adj_normalize(None, 'sym')
    for f in (lp_utils.gcn_normalization, lp_utils.adj_normalization):
        with pytest.raises(TypeError, match='WeightedAdj'):
            f(object())
    x, W = torch.ones(3, 8), torch.ones(8, 8)
    with pytest.raises(_lib.HipExtensionError):
        ops.sage_layer(None, x, W, W, None, mode='WSAGE')


def test_the_tool_parses_normalize_adj():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import run_linkpred
    base = ['--dataset=S-tiny', '--encoder=GCN', '--predictor=MLP'] + PLUMBING
    a = run_linkpred.parse_args(base)
    assert a.normalize_adj == 0 and a.encoder == 'GCN' and a.edge_lp_mode == ''
    a = run_linkpred.parse_args(base + ['--normalize_adj=1'])
    assert a.normalize_adj == 1
    # it is the tool's own option: the package's parser, whose results a golden file pins, does not know it
    from gnn_tail_generalization_amd.base_options import BaseOptions
    assert not hasattr(BaseOptions().get_arguments(['--dataset=S-tiny', '--encoder=SAGE', '--predictor=MLP'] + PLUMBING), 'normalize_adj')
    assert run_linkpred.parse_args(['--dataset=S-tiny', '--encoder=wsage'] + PLUMBING).encoder == 'WSAGE'


def test_the_scope_documents_no_longer_list_the_normalisations_as_missing():
    tool = open(os.path.join(ROOT, 'tools', 'run_linkpred.py')).read()
    assert 'Not applied' not in tool and '--normalize_adj' in tool
    from gnn_tail_generalization_amd.Link_prediction_model import utils as lp_utils
    assert 'adjacency as given' not in lp_utils.__doc__ and callable(lp_utils.gcn_normalization) and callable(lp_utils.adj_normalization)
