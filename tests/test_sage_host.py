"""Host-side checks (no GPU) of the link-prediction encoders: constructor signatures, PyG's parameter names and [out, in] shapes, create_encoder_layer's
table and refusals, create_input_layer's three modes, CPU tensors refused, the C ABI of csrc/cb_sage.hip declared / exported / bound with matching
argument counts and refusing bad arguments before any launch, the float64 restatement of tests/sage_ref.py against a dense formulation, and the pinned
refusal of layer.SAGE / GCN / WSAGE / MLP."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import sage_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_sage_image_bytes', 'cb_sage_image_f32', 'cb_sage_layer_supported', 'cb_sage_layer_f32']
ARGS = ['self', 'in_channels', 'hidden_channels', 'out_channels', 'num_layers', 'dropout']


def _names(prefix, per_layer, n):
    return {f'{prefix}.{i}.{w}' for i in range(n) for w in per_layer}


def test_encoder_signatures_and_parameter_names():
    from gnn_tail_generalization_amd import Link_prediction_model as lpm
    from gnn_tail_generalization_amd.Link_prediction_model import encoder
    table = {'SAGEEncoder': {'lin_l.weight': (0, 1), 'lin_l.bias': (0,), 'lin_r.weight': (0, 1)},
             'WSAGEEncoder': {'lin_rel.weight': (0, 1), 'lin_rel.bias': (0,), 'lin_root.weight': (0, 1)},
             'GCNEncoder': {'lin.weight': (0, 1), 'bias': (0,)},
             'MLPEncoder': {'weight': (0, 1), 'bias': (0,)}}
    for name, per_layer in table.items():
        cls = getattr(encoder, name)
        assert getattr(lpm, name) is cls
        assert list(inspect.signature(cls.__init__).parameters) == ARGS, name
        assert list(inspect.signature(cls.forward).parameters) == ['self', 'x', 'graph'] and callable(cls.reset_parameters)
        m = cls(12, 20, 8, 3, 0.25)
        sd = m.state_dict()
        assert set(sd) == _names('convs', per_layer, 3), name
        assert m.dropout == 0.25
        widths = [(20, 12), (20, 20), (8, 20)]      # [out, in] per layer
        for i, (o, k) in enumerate(widths):
            for w, dims in per_layer.items():
                assert tuple(sd[f'convs.{i}.{w}'].shape) == ((o, k) if len(dims) == 2 else (o,)), (name, i, w)
        torch.manual_seed(1)
        m.reset_parameters()
        a = {k: v.clone() for k, v in m.state_dict().items()}
        torch.manual_seed(1)
        m.reset_parameters()
        assert all(torch.equal(a[k], v) for k, v in m.state_dict().items())
        assert all(float(v.abs().sum()) > 0 for k, v in a.items())
    # SAGE's names in PyG's order, created layer by layer
    assert list(encoder.SAGEEncoder(4, 4, 4, 2, 0.0).state_dict()) == [f'convs.{i}.{w}' for i in (0, 1) for w in ('lin_l.weight', 'lin_l.bias', 'lin_r.weight')]


def test_create_encoder_layer_table_and_refusals():
    from gnn_tail_generalization_amd.Link_prediction_model import encoder, layer, model
    assert list(inspect.signature(model.create_encoder_layer).parameters)[:5] == ['input_channels', 'hidden_channels', 'num_layers', 'dropout', 'encoder_name']
    assert inspect.signature(model.create_encoder_layer).parameters['encoder_name'].default == 'SAGE'
    for name, cls in (('SAGE', encoder.SAGEEncoder), ('sage', encoder.SAGEEncoder), ('WSAGE', encoder.WSAGEEncoder), ('Gcn', encoder.GCNEncoder),
                      ('mlp', encoder.MLPEncoder)):
        m = model.create_encoder_layer(16, 24, 3, 0.5, name)
        assert type(m) is cls and len(m.convs) == 3 and m.dropout == 0.5
        first = m.convs[0]
        w = first.weight if cls is encoder.MLPEncoder else first.params()[0]
        assert tuple(w.shape) == (24, 16)
        last = m.convs[-1]
        assert tuple((last.weight if cls is encoder.MLPEncoder else last.params()[0]).shape) == (24, 24)
    for name in ('CN', 'AA', 'PPR'):
        h = model.create_encoder_layer(16, 24, 3, 0.5, name, data='d')
        assert type(h) is layer.Heuristics and h.name == name and h.data == 'd'
    with pytest.raises(NotImplementedError, match='TRANSFORMER'):
        model.create_encoder_layer(16, 24, 3, 0.5, 'Transformer')
    for name in ('nope', 'cn'):      # (the reference matches the heuristics' names case-sensitively)
        with pytest.raises(NotImplementedError, match='not implemented'):
            model.create_encoder_layer(16, 24, 3, 0.5, name)


def test_the_pyg_names_keep_raising():
    from gnn_tail_generalization_amd.Link_prediction_model import layer
    for name in ('SAGE', 'GCN', 'WSAGE', 'MLP'):
        with pytest.raises(NotImplementedError, match=f'{name} is not built.*needs'):
            getattr(layer, name)(4, 4, 4, 2, 0.0)


def test_create_input_layer_modes():
    from gnn_tail_generalization_amd.Link_prediction_model import model
    torch.manual_seed(0)
    dim, emb = model.create_input_layer(50, 7, 16, use_node_feats=False)
    assert dim == 16 and isinstance(emb, torch.nn.Embedding) and tuple(emb.weight.shape) == (50, 16) and emb.weight.requires_grad
    model.reset_input_layer(emb)
    bound = (6.0 / (50 + 16)) ** 0.5      # xavier_uniform_
    assert float(emb.weight.detach().abs().max()) <= bound and float(emb.weight.detach().abs().max()) > 0.8 * bound
    assert model.create_input_feat(emb, None, use_node_feats=False) is emb.weight
    dim, emb = model.create_input_layer(50, 7, 16, use_node_feats=True)
    x = torch.arange(350, dtype=torch.float64).reshape(50, 7)
    feat = model.create_input_feat(emb, x, use_node_feats=True)
    assert dim == 7 and emb is None and feat.dtype == torch.float32 and torch.equal(feat, x.float())
    dim, emb = model.create_input_layer(50, 7, 16, use_node_feats=True, train_node_emb=True)
    feat = model.create_input_feat(emb, x, use_node_feats=True)
    assert dim == 23 and tuple(feat.shape) == (50, 23) and torch.equal(feat[:, :16], emb.weight) and torch.equal(feat[:, 16:], x.float())
    for kw in ({'use_node_feats': False}, {'use_node_feats': True}):
        with pytest.raises(NotImplementedError, match='pretrain_emb'):
            model.create_input_layer(50, 7, 16, pretrain_emb='emb.pt', **kw)
    assert model.create_input_layer(50, 7, 16, use_node_feats=False, pretrain_emb='')[0] == 16


def test_cpu_tensors_are_refused():
    from gnn_tail_generalization_amd import _lib, ops
    from gnn_tail_generalization_amd.Link_prediction_model import GCNEncoder, MLPEncoder, SAGEEncoder, WSAGEEncoder
    x = torch.ones(6, 8)
    for cls in (SAGEEncoder, WSAGEEncoder, GCNEncoder, MLPEncoder):
        with pytest.raises(_lib.HipExtensionError):
            cls(8, 8, 8, 2, 0.0)(x, None)
    W = torch.ones(8, 8)
    with pytest.raises(_lib.HipExtensionError):
        ops.sage_layer(None, x, W, W, None, mode='SAGE')
    with pytest.raises(_lib.HipExtensionError):
        ops.sage_layer_raw(None, x, W, W)
    with pytest.raises(ValueError, match='mode'):
        ops.sage_layer(None, x, W, W, None, mode='GAT')


def test_c_abi_of_the_sage_kernel():
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
    assert {n for n in declared if n.startswith('cb_sage_')} == set(NEW_ENTRIES)


def test_bad_arguments_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    P16, P4 = ctypes.c_void_p(16), ctypes.c_void_p(20)      # non-null pointers that are never dereferenced: the checks answer before any launch
    one = 16 * 8 * 3 * 64 * 16
    assert lib.cb_sage_image_bytes(0) == one and lib.cb_sage_image_bytes(1) == 2 * one
    assert lib.cb_sage_image_f32(P16, 256, P16, 256, 1, P16, one, None) == -3           # two blocks need twice the bytes
    assert lib.cb_sage_image_f32(P16, 128, None, 0, 1, P16, one, None) == -1            # leading dimension below 256
    assert lib.cb_sage_image_f32(None, 256, None, 0, 1, P16, one, None) == -1
    sup = lib.cb_sage_layer_supported
    assert sup(256, 256, 0, P16, 256, P16, 256, None, 0, P16, 256) == 1 and sup(256, 256, 0, P16, 260, None, 0, P16, 512, P16, 260) == 1
    assert sup(128, 256, 0, P16, 256, P16, 256, None, 0, P16, 256) == 0 and sup(256, 64, 0, P16, 256, P16, 256, None, 0, P16, 256) == 0
    assert sup(256, 256, 1, P16, 256, P16, 256, None, 0, P16, 256) == 0
    assert sup(256, 256, 0, P4, 256, P16, 256, None, 0, P16, 256) == 0 and sup(256, 256, 0, P16, 256, P16, 256, None, 0, P4, 256) == 0
    assert sup(256, 256, 0, P16, 254, P16, 256, None, 0, P16, 256) == 0 and sup(256, 256, 0, P16, 256, P16, 256, P16, 252, P16, 256) == 0
    view = _lib.CsrView(16, 16, 0, 64, 10, 256, 0, 0, None, None, None, 0)
    call = lambda h, p, relu, agg_only=0: lib.cb_sage_layer_f32(ctypes.byref(view), h, 256, h, 256, None, None, P16, None, relu, p, ctypes.c_uint64(0), None, 0,
                                                               None, 0, agg_only, P16, 256, None)
    assert call(P4, 0.0, 0) == -1 and b'cb_sage_layer_supported' in lib.cb_last_error()
    assert call(P16, 0.5, 0) == -1                                                      # dropout without the ReLU
    assert call(P16, 1.0, 1) == -1
    assert call(P16, 0.0, 0, agg_only=1) == -1                                          # hub rows only, but no agg_out
    hub = _lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, 16, 1 << 20)
    assert lib.cb_sage_layer_f32(ctypes.byref(hub), P16, 256, P16, 256, None, None, P16, None, 0, 0.0, ctypes.c_uint64(0), None, 0, None, 0, 0, P16, 256,
                                 None) == -1                                            # a plan with hub rows needs agg_out
    # the view itself (check_csr_view, as for every aggregation entry): null view, negative / oversized counts, null arrays, hub plan without its workspace
    def with_view(v):
        return lib.cb_sage_layer_f32(ctypes.byref(v) if v is not None else None, P16, 256, P16, 256, None, None, P16, None, 0, 0.0, ctypes.c_uint64(0), None, 0,
                                     P16, 256, 0, P16, 256, None)
    assert with_view(None) == -1
    assert with_view(_lib.CsrView(16, 16, 0, -1, 10, 256, 0, 0, None, None, None, 0)) == -1
    assert with_view(_lib.CsrView(16, 16, 0, 2 ** 31, 10, 256, 0, 0, None, None, None, 0)) == -2
    assert with_view(_lib.CsrView(None, 16, 0, 64, 10, 256, 0, 0, None, None, None, 0)) == -1
    assert with_view(_lib.CsrView(16, None, 0, 64, 10, 256, 0, 0, None, None, None, 0)) == -1
    assert with_view(_lib.CsrView(16, 16, 0, 64, 10, 0, 0, 0, None, None, None, 0)) == -1
    assert with_view(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, None, 0)) == -3
    assert with_view(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, 16, 2 * 256 * 4 - 1)) == -3
    empty = _lib.CsrView(None, None, 0, 0, 0, 256, 0, 0, None, None, None, 0)
    assert lib.cb_sage_layer_f32(ctypes.byref(empty), None, 0, None, 0, None, None, None, None, 0, 0.0, ctypes.c_uint64(0), None, 0, None, 0, 0, None, 0, None) == 0


@pytest.mark.parametrize('mode', sr.MODES)
def test_the_restatement_equals_a_dense_formulation(mode):
    """index_add_ over the edge list == the dense adjacency product (multiplicity, self loops, empty rows), its autograd included."""
    n = 23
    ei = sr.make_graph(n, 70, seed=4, no_in=(2, 9, 20), n_self=4, n_dup=9)
    g = torch.Generator().manual_seed(0)
    x, W_n, W_s, b = [torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True) for s in ((n, 6), (5, 6), (5, 6), (5,))]
    Ws = None if mode == 'GCN' else W_s
    A = torch.zeros(n, n, dtype=torch.float64).index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    assert float(A.max()) >= 2 and float(A.diagonal().sum()) >= 4 and not torch.equal(A, A.t())
    deg = A.sum(1)
    assert all(float(deg[v]) == 0 for v in (2, 9, 20))
    agg = A @ x
    if mode == 'SAGE':
        agg = torch.where(deg[:, None] > 0, agg / deg.clamp(min=1)[:, None], torch.zeros_like(agg))
    want = torch.relu(agg @ W_n.t() + (x @ Ws.t() if Ws is not None else 0) + b)
    got, agg_got = sr.layer(ei, n, x, W_n, Ws, b, mode, relu=True)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13) and torch.allclose(agg_got, agg, rtol=1e-13, atol=1e-13)
    assert (agg_got[[2, 9, 20]] == 0).all()
    leaves = [t for t in (x, W_n, Ws, b) if t is not None]
    g1 = torch.autograd.grad(got.sum(), leaves)
    g2 = torch.autograd.grad(want.sum(), leaves)
    assert all(torch.allclose(a, c, rtol=1e-12, atol=1e-12) for a, c in zip(g1, g2))
    assert torch.allclose(sr.agg_sum_t(ei, n, x.detach()), A.t() @ x.detach(), rtol=1e-13, atol=1e-13)


def test_the_new_hip_file_compiles_clean_under_wall_without_scratch(tmp_path):
    """The cross-compile for gfx950 with the Makefile's flags and -Werror; the sixteen layer kernels (self x source factor x stored aggregate x gather
    policy) report 0 bytes of scratch, fit two wavefronts per SIMD (eight per block, one block per CU) and stay inside the CU's 160 KiB of LDS."""
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    src = os.path.join(ROOT, 'gnn-tail-generalization_amd', 'csrc', 'cb_sage.hip')
    flags = re.search(r'^FLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    assert '-Wall' in flags
    r = subprocess.run([hipcc] + flags + ['-Werror', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / 'cb_sage.o')],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0 and 'warning:' not in r.stderr, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    occ = [int(v) for v in re.findall(r'Occupancy \[waves/SIMD\]: (\d+)', r.stderr)]
    lds = [int(v) for v in re.findall(r'LDS Size \[bytes/block\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == len(occ) == len(lds) and sum('k_sage_layer' in n for n in names) == 16
    assert not any(scratch), dict(zip(names, scratch))
    for n, o, l in zip(names, occ, lds):
        if 'k_sage_layer' in n:
            assert o >= 2 and l <= 160 * 1024, (n, o, l)
            assert l == (64 * 516 + 4 * 8 * 68) * 4 if 'k_sage_layerILb1E' in n else l == (64 * 260 + 4 * 8 * 68) * 4, (n, l)
