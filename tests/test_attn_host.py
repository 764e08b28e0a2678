"""Host-side checks (no GPU) of the Transformer link-prediction encoder: the float64 restatement of tests/attn_ref.py against a dense formulation and
its closed-form gradients against autograd, the constructor signature / parameter names and order / shapes of encoder.TransformerEncoder, CPU tensors
refused, the C ABI of csrc/cb_attn.hip declared / exported / bound with matching argument counts and refusing bad arguments before any launch, and the
gfx950 cross-compile of the file under -Wall -Werror with 0 bytes of scratch in every kernel."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import attn_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_attn_supported', 'cb_attn_workspace_bytes', 'cb_attn_fwd_f32', 'cb_attn_bwd_dst_f32', 'cb_attn_bwd_src_f32']
NO_IN = (2, 9, 20)


def _small():
    n = 23
    ei = ar.make_graph(n, 70, seed=4, no_in=NO_IN, n_self=4, n_dup=9)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, 6, generator=g, dtype=torch.float64)
    params = ar.make_params(6, 8, seed=1, dtype=torch.float64)
    dY = torch.randn(n, 8, generator=g, dtype=torch.float64)
    return n, ei, x, params, dY


def _dense_layer(ei, n, x, params, relu):
    """Masked dense scores; a pair (v, u) of multiplicity k appears in k of the column blocks, so that every copy is its own softmax term."""
    Q, K, V, S = ar.project(x, params)
    C = torch.zeros(n, n, dtype=torch.int64).index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=torch.int64), accumulate=True)
    kmax = int(C.max())
    assert kmax >= 2 and int(C.diagonal().sum()) >= 4 and not torch.equal(C, C.t())
    scores = Q @ K.t() / math.sqrt(Q.shape[1])
    has = C.sum(1) > 0
    assert not has[list(NO_IN)].any() and int((~has).sum()) == len(NO_IN)
    blocks = [torch.where(C > k, scores, torch.full_like(scores, float('-inf'))) for k in range(kmax)]
    wide = torch.cat(blocks, 1)
    wide = torch.where(has[:, None], wide, torch.zeros_like(wide))      # (a row of -inf alone would make softmax a NaN; its probabilities are dropped below)
    P = torch.softmax(wide, 1) * has[:, None].to(wide.dtype)
    out = P @ torch.cat([V] * kmax, 0) + S
    lse = torch.where(has, torch.logsumexp(wide, 1), torch.full((n,), float('-inf'), dtype=wide.dtype))
    return (torch.relu(out) if relu else out), lse


@pytest.mark.parametrize('relu', [False, True])
def test_the_restatement_equals_a_dense_formulation(relu):
    n, ei, x, params, dY = _small()
    leaves = [x.clone().requires_grad_(True)] + [params[k].clone().requires_grad_(True) for k in ar.NAMES]
    p = dict(zip(ar.NAMES, leaves[1:]))
    got, lse = ar.layer(ei, n, leaves[0], p, relu)
    want, lse_d = _dense_layer(ei, n, leaves[0], p, relu)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert ar.max_err(lse, lse_d) <= 1e-12 and bool(torch.isinf(lse[list(NO_IN)]).all())
    S = ar.project(leaves[0], p)[3]
    assert torch.equal(got[list(NO_IN)], (torch.relu(S) if relu else S)[list(NO_IN)])      # a row without in-edges gives S[v]
    g1 = torch.autograd.grad((got * dY).sum(), leaves)
    g2 = torch.autograd.grad((want * dY).sum(), leaves)
    assert all(torch.allclose(a, c, rtol=1e-12, atol=1e-12) for a, c in zip(g1, g2))


@pytest.mark.parametrize('relu', [False, True])
def test_the_closed_form_gradients_equal_autograd(relu):
    n, ei, x, params, dY = _small()
    leaves = [x.clone().requires_grad_(True)] + [params[k].clone().requires_grad_(True) for k in ar.NAMES]
    out, _ = ar.layer(ei, n, leaves[0], dict(zip(ar.NAMES, leaves[1:])), relu)
    auto = dict(zip(('x',) + ar.NAMES, torch.autograd.grad((out * dY).sum(), leaves)))
    closed = ar.grads(ei, n, x, params, dY, relu)
    assert torch.allclose(closed['out'], out, rtol=1e-13, atol=1e-13)
    for k, v in auto.items():
        assert torch.allclose(closed[k], v, rtol=1e-12, atol=1e-12), k
    assert float(closed['delta'][list(NO_IN)].abs().max()) == 0.0


def test_encoder_signature_and_parameter_names():
    from gnn_tail_generalization_amd import Link_prediction_model as lpm
    from gnn_tail_generalization_amd.Link_prediction_model import encoder
    assert lpm.TransformerEncoder is encoder.TransformerEncoder and lpm.TransformerConv is encoder.TransformerConv
    cls = encoder.TransformerEncoder
    assert cls.conv is encoder.TransformerConv and issubclass(cls, encoder._Encoder)
    assert list(inspect.signature(cls.__init__).parameters) == ['self', 'in_channels', 'hidden_channels', 'out_channels', 'num_layers', 'dropout']
    assert list(inspect.signature(cls.forward).parameters) == ['self', 'x', 'graph']
    assert list(inspect.signature(encoder.TransformerConv.forward).parameters) == ['self', 'x', 'graph', 'relu', 'p']
    m = cls(12, 20, 8, 3, 0.25)
    sd = m.state_dict()
    assert list(sd) == [f'convs.{i}.{w}' for i in range(3) for w in ar.NAMES]
    assert ar.NAMES == ('lin_key.weight', 'lin_key.bias', 'lin_query.weight', 'lin_query.bias', 'lin_value.weight', 'lin_value.bias', 'lin_skip.weight',
                        'lin_skip.bias')
    assert m.dropout == 0.25
    for i, (o, k) in enumerate([(20, 12), (20, 20), (8, 20)]):      # [out, in] per layer
        for w in ar.NAMES:
            assert tuple(sd[f'convs.{i}.{w}'].shape) == ((o, k) if w.endswith('weight') else (o,)), (i, w)
    torch.manual_seed(1)
    m.reset_parameters()
    a = {k: v.clone() for k, v in m.state_dict().items()}
    torch.manual_seed(1)
    m.reset_parameters()
    assert all(torch.equal(a[k], v) for k, v in m.state_dict().items()) and all(float(v.abs().sum()) > 0 for v in a.values())


def test_the_pyg_name_keeps_raising():
    from gnn_tail_generalization_amd.Link_prediction_model import layer, model
    with pytest.raises(NotImplementedError, match='Transformer is not built.*needs'):
        layer.Transformer(4, 4, 4, 2, 0.0)
    with pytest.raises(NotImplementedError, match='TRANSFORMER'):
        model.create_encoder_layer(16, 24, 3, 0.5, 'Transformer')


def test_cpu_tensors_are_refused():
    from gnn_tail_generalization_amd import _lib, ops
    from gnn_tail_generalization_amd.Link_prediction_model import TransformerEncoder
    x, W, b = torch.ones(6, 8), torch.ones(8, 8), torch.ones(8)
    with pytest.raises(_lib.HipExtensionError):
        TransformerEncoder(8, 8, 8, 2, 0.0)(x, None)
    with pytest.raises(_lib.HipExtensionError):
        ops.transformer_conv(None, x, W, b, W, b, W, b, W, b)
    with pytest.raises(_lib.HipExtensionError):
        ops.attn_raw(None, x, x, x, x)
    with pytest.raises(_lib.HipExtensionError):
        ops.attn_bwd_raw(None, x, x, x, x, torch.ones(6), x, x, x)


def test_c_abi_of_the_attention_kernels():
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
    assert {n for n in declared if n.startswith('cb_attn_')} == set(NEW_ENTRIES)


def test_bad_arguments_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    P16, P4 = ctypes.c_void_p(16), ctypes.c_void_p(20)      # non-null pointers that are never dereferenced: the checks answer before any launch
    sup = lib.cb_attn_supported
    assert sup(64, P16, 64) == 1 and sup(256, P16, 1024) == 1 and sup(4, P16, 16) == 1 and sup(512, P16, 2048) == 1 and sup(36, P16, 40) == 1
    assert sup(6, P16, 8) == 0 and sup(516, P16, 516) == 0 and sup(0, P16, 4) == 0 and sup(1024, P16, 1024) == 0      # unsupported D
    assert sup(64, P4, 64) == 0 and sup(64, P16, 66) == 0 and sup(64, P16, 60) == 0 and sup(64, None, 64) == 0          # misaligned rows, ld < D, null
    assert lib.cb_attn_workspace_bytes(3, 64) == 3 * (2 * 64 + 4) * 4 and lib.cb_attn_workspace_bytes(0, 64) == 0
    plain = _lib.CsrView(16, 16, 0, 64, 10, 256, 0, 0, None, None, None, 0)

    def fwd(view, d=64, q=P16, ld=256, out=P16):
        return lib.cb_attn_fwd_f32(ctypes.byref(view) if view is not None else None, d, q, ld, P16, ld, P16, ld, P16, ld, 0, out, ld, None, None)

    def dst(view, d=64, q=P16, ld=256, lse=P16):
        return lib.cb_attn_bwd_dst_f32(ctypes.byref(view) if view is not None else None, d, q, ld, P16, ld, P16, ld, P16, ld, lse, P16, ld, P16, None)

    def src(view, d=64, q=P16, ld=256, dv=P16):
        return lib.cb_attn_bwd_src_f32(ctypes.byref(view) if view is not None else None, d, q, ld, P16, ld, P16, ld, P16, ld, P16, P16, P16, ld, dv, ld, None)

    for call in (fwd, dst, src):
        assert call(plain, d=6) == -1 and b'cb_attn_supported' in lib.cb_last_error()      # unsupported D
        assert call(plain, d=1024) == -1
        assert call(plain, q=P4) == -1 and b'cb_attn_supported' in lib.cb_last_error()     # misaligned rows
        assert call(plain, ld=60) == -1 and call(plain, ld=66) == -1                        # ld < D, ld % 4
        assert call(plain, q=None) == -1
        assert call(None) == -1                                                             # null view
        # the view itself (check_csr_view, as for every aggregation entry)
        assert call(_lib.CsrView(16, 16, 0, -1, 10, 256, 0, 0, None, None, None, 0)) == -1
        assert call(_lib.CsrView(16, 16, 0, 2 ** 31, 10, 256, 0, 0, None, None, None, 0)) == -2
        assert call(_lib.CsrView(None, 16, 0, 64, 10, 256, 0, 0, None, None, None, 0)) == -1
        assert call(_lib.CsrView(16, None, 0, 64, 10, 256, 0, 0, None, None, None, 0)) == -1
        assert call(_lib.CsrView(16, 16, 0, 64, 10, 0, 0, 0, None, None, None, 0)) == -1
        need = lib.cb_attn_workspace_bytes(2, 64)
        assert call(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, None, 0)) == -3       # a hub plan without its workspace
        assert call(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, 16, need - 1)) == -3  # ... or with one a byte short
        assert call(_lib.CsrView(16, 16, 0, 64, 10, 4, 1, 2, 16, 16, 20, need)) == -3      # ... or misaligned
    assert fwd(plain, out=None) == -1 and dst(plain, lse=None) == -1 and src(plain, dv=P4) == -1
    empty = _lib.CsrView(None, None, 0, 0, 0, 256, 0, 0, None, None, None, 0)
    assert lib.cb_attn_fwd_f32(ctypes.byref(empty), 64, None, 0, None, 0, None, 0, None, 0, 0, None, 0, None, None) == 0
    assert lib.cb_attn_bwd_dst_f32(ctypes.byref(empty), 64, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None) == 0
    assert lib.cb_attn_bwd_src_f32(ctypes.byref(empty), 64, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None) == 0


def test_the_new_hip_file_compiles_clean_under_wall_without_scratch(tmp_path):
    """The cross-compile for gfx950 with the Makefile's flags and -Werror: every kernel of the file reports 0 bytes of scratch, and the row kernels of the
    widths up to 256 fit at least two wavefronts per SIMD."""
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    src = os.path.join(ROOT, 'gnn-tail-generalization_amd', 'csrc', 'cb_attn.hip')
    flags = re.search(r'^FLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    assert '-Wall' in flags
    r = subprocess.run([hipcc] + flags + ['-Werror', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / 'cb_attn.o')],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0 and 'warning:' not in r.stderr, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    occ = [int(v) for v in re.findall(r'Occupancy \[waves/SIMD\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == len(occ)
    # rows: 3 kernel modes x 4 widths x 2 gather policies; hub chunks: 4 modes x 4 x 2; hub finish: 4 modes x 4
    assert sum('k_attn_rows' in n for n in names) == 24 and sum('k_attn_hub_chunks' in n for n in names) == 32 and sum('k_attn_hub_finish' in n for n in names) == 16
    assert len(names) == 72 and not any(scratch), dict(zip(names, scratch))
    for n, o in zip(names, occ):
        if 'k_attn_rows' in n and 'Li8E' not in n:
            assert o >= 2, (n, o)
