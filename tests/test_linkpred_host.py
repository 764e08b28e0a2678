"""Host-side checks (no GPU) of the link predictors and ranking losses: the Link_prediction_model package imports and carries the reference's
names, signatures and parameter names (same-seed initialisation included); what is not built says so; CPU tensors are refused; the C ABI of
csrc/cb_linkpred.hip is declared, exported and bound with matching argument counts and refuses bad arguments before any launch; the float64
restatement of tests/linkpred_ref.py equals the recordings of the unmodified reference (tests/golden/linkpred_*.pt); calculate_loss dispatches as
BaseModel.calculate_loss does; the new HIP file compiles clean under -Wall."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import linkpred_ref as lr
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_pair_gemm_nn_supported', 'cb_pair_gemm_nn_f32', 'cb_pair_dot_f32', 'cb_pair_scatter_workspace_bytes', 'cb_pair_scatter_f32',
               'cb_rank_loss_workspace_bytes', 'cb_rank_loss_fwd_f32', 'cb_rank_loss_bwd_f32']
P8 = ctypes.c_void_p(16)      # a non-null, 16-byte aligned pointer that is never dereferenced: the checks below answer before any launch


def test_package_names_and_signatures():
    from gnn_tail_generalization_amd import Link_prediction_model as lpm
    from gnn_tail_generalization_amd.Link_prediction_model import layer, loss, model
    want = {'auc_loss': ['pos_out', 'neg_out', 'num_neg'], 'adaptive_auc_loss': ['pos_out', 'neg_out', 'num_neg', 'weight'],
            'log_rank_loss': ['pos_out', 'neg_out', 'num_neg'], 'ce_loss': ['pos_out', 'neg_out'], 'info_nce_loss': ['pos_out', 'neg_out', 'num_neg']}
    assert set(want) == set(lr.KINDS)
    for name, params in want.items():
        assert list(inspect.signature(getattr(loss, name)).parameters) == params, name
        assert getattr(lpm, name) is getattr(loss, name)
    assert list(inspect.signature(layer.MLPPredictor.__init__).parameters) == ['self', 'in_channels', 'hidden_channels', 'out_channels', 'num_layers', 'dropout']
    assert list(inspect.signature(layer.DotPredictor.__init__).parameters) == ['self']
    assert list(inspect.signature(layer.Heuristics.__init__).parameters) == ['self', 'name', 'data']
    for cls in (layer.MLPPredictor, layer.DotPredictor):
        assert list(inspect.signature(cls.forward).parameters) == ['self', 'x_i', 'x_j']
        assert list(inspect.signature(cls.score_pairs).parameters) == ['self', 'h', 'pairs']
        assert callable(cls.reset_parameters)
    assert list(inspect.signature(model.create_predictor_layer).parameters) == ['hidden_channels', 'num_layers', 'dropout', 'predictor_name']
    assert list(inspect.signature(model.calculate_loss).parameters) == ['loss_func_name', 'pos_out', 'neg_out', 'num_neg', 'margin']
    assert type(model.create_predictor_layer(8, 2, 0.1, 'dot')) is layer.DotPredictor
    m = model.create_predictor_layer(8, 3, 0.25, 'mlp')
    assert type(m) is layer.MLPPredictor and m.dropout == 0.25 and [tuple(l.weight.shape) for l in m.lins] == [(8, 8), (8, 8), (1, 8)]
    h = layer.Heuristics('CN', object())
    assert h.reset_parameters() is None and h.forward(3, None) == 3


@pytest.mark.parametrize('L', [1, 2, 3])
def test_parameter_names_and_same_seed_initialisation_match_the_reference(L):
    from gnn_tail_generalization_amd.Link_prediction_model import MLPPredictor
    rec = load_golden('linkpred_predictors')['mlp'][L]
    torch.manual_seed(rec['seed'])
    m = MLPPredictor(32, 32, 1, L, 0.5)
    sd = m.state_dict()
    assert list(sd) == list(rec['state_dict']) == [f'lins.{i}.{w}' for i in range(L) for w in ('weight', 'bias')]
    for k, v in rec['state_dict'].items():
        assert torch.equal(sd[k], v), k
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
    torch.manual_seed(rec['seed'])
    m.reset_parameters()
    for k, v in rec['state_dict'].items():
        assert torch.equal(m.state_dict()[k], v), k


def test_what_is_not_built_says_what_it_needs():
    from gnn_tail_generalization_amd.Link_prediction_model import layer, model
    for name, args in (('MLP', (4, 4, 4, 2, 0.0)), ('SAGE', (4, 4, 4, 2, 0.0)), ('GCN', (4, 4, 4, 2, 0.0)), ('WSAGE', (4, 4, 4, 2, 0.0)),
                       ('Transformer', (4, 4, 4, 2, 0.0)), ('MLPCatPredictor', (4, 4, 1, 2, 0.0)), ('MLPDotPredictor', (4, 1, 2, 0.0)),
                       ('MLPBilPredictor', (4, 1, 2, 0.0)), ('BilinearPredictor', (4,))):
        with pytest.raises(NotImplementedError, match=f'{name} is not built.*needs'):
            getattr(layer, name)(*args)
    for name in ('BIL', 'MLPDOT', 'MLPBIL', 'MLPCAT'):
        with pytest.raises(NotImplementedError, match='needs'):
            model.create_predictor_layer(8, 2, 0.0, name)
    with pytest.raises(NotImplementedError, match='not implemented'):
        model.create_predictor_layer(8, 2, 0.0, 'nope')


def test_cpu_tensors_are_refused():
    from gnn_tail_generalization_amd import _lib, ops
    from gnn_tail_generalization_amd.Link_prediction_model import DotPredictor, MLPPredictor, calculate_loss, loss
    h, pairs = torch.ones(6, 8), torch.zeros((2, 4), dtype=torch.int64)
    m = MLPPredictor(8, 8, 1, 2, 0.0)
    for fn in (lambda: DotPredictor()(h[:4], h[:4]), lambda: DotPredictor().score_pairs(h, pairs), lambda: m(h[:4], h[:4]), lambda: m.score_pairs(h, pairs),
               lambda: ops.pair_dot(h, pairs), lambda: ops.pair_linear(h, pairs, m.lins[0].weight, m.lins[0].bias),
               lambda: ops.rank_loss('auc_loss', torch.ones(2), torch.ones(4), 2), lambda: loss.ce_loss(torch.ones(2), torch.ones(4)),
               lambda: calculate_loss('log_rank_loss', torch.ones(2), torch.ones(4), 2)):
        with pytest.raises(_lib.HipExtensionError):
            fn()
    with pytest.raises(ValueError, match='kind'):
        ops.rank_loss('hinge', torch.ones(2), torch.ones(4), 2)
    assert ops.pair_dot.check is ops.pair_check and ops.pair_linear.check is ops.pair_check and ops.rank_loss.check is ops.pair_check


def test_c_abi_of_the_linkpred_kernels():
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
    assert {n for n in declared if n.startswith('cb_pair_') or n.startswith('cb_rank_loss')} == set(NEW_ENTRIES)
    from gnn_tail_generalization_amd import ops
    kinds = {k: int(re.search(r'#define CB_RANK_' + k[:-5].upper() + r' (\d+)', hdr).group(1)) for k in lr.KINDS}
    assert kinds == ops.RANK_KINDS


def test_bad_arguments_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    # pair GEMM: the predicate and the entry
    assert lib.cb_pair_gemm_nn_supported(P8, 256, P8, 256, 256, 256) == 1
    assert lib.cb_pair_gemm_nn_supported(P8, 12, P8, 8, 8, 10) == 0            # K % 4
    assert lib.cb_pair_gemm_nn_supported(P8, 256, P8, 1, 1, 256) == 0          # Nout % 4
    assert lib.cb_pair_gemm_nn_supported(P8, 258, P8, 256, 256, 256) == 0      # ld % 4
    assert lib.cb_pair_gemm_nn_supported(ctypes.c_void_p(20), 256, P8, 256, 256, 256) == 0      # misaligned rows
    assert lib.cb_pair_gemm_nn_supported(None, 256, P8, 256, 256, 256) == 0

    def gemm(h=P8, ld=16, N=5, pairs=P8, S=3, B=P8, ldb=8, C=P8, ldc=8, C2=None, ldc2=8, Nout=8, K=16, p=0.0, status=P8):
        return lib.cb_pair_gemm_nn_f32(h, ld, N, pairs, S, B, ldb, C, ldc, C2, ldc2, Nout, K, None, 0, p, 1, None, 0, status, None)
    assert gemm(status=None) == -1 and b'status' in lib.cb_last_error()
    assert gemm(N=0) == -1 and gemm(S=-1) == -1 and gemm(p=1.0) == -1 and gemm(N=2 ** 31) == -2
    # pair dot / scatter
    assert lib.cb_pair_dot_f32(P8, 4, 5, 8, P8, 3, P8, P8, None) == -1 and b'ld >= D' in lib.cb_last_error()
    assert lib.cb_pair_dot_f32(P8, 8, 5, 8, P8, 3, P8, None, None) == -1 and b'status' in lib.cb_last_error()
    assert lib.cb_pair_dot_f32(P8, 8, 5, 8, P8, 2 ** 30, P8, P8, None) == -2
    assert lib.cb_pair_scatter_workspace_bytes(0) == 0 and lib.cb_pair_scatter_workspace_bytes(3) >= 2 * 6 * 8
    assert lib.cb_pair_scatter_f32(P8, 8, 5, 8, P8, 3, P8, 4, P8, 8, P8, 1 << 20, None) == -1 and b'ldcoef' in lib.cb_last_error()
    assert lib.cb_pair_scatter_f32(P8, 8, 5, 8, P8, 3, P8, 0, P8, 4, P8, 1 << 20, None) == -1 and b'ldd' in lib.cb_last_error()
    assert lib.cb_pair_scatter_f32(P8, 8, 5, 8, P8, 3, None, 0, P8, 8, P8, 1 << 20, None) == -1 and b'null' in lib.cb_last_error()
    assert lib.cb_pair_scatter_f32(P8, 8, 5, 8, P8, 3, P8, 0, P8, 8, P8, 8, None) == -3      # workspace too small
    # ranking losses
    assert lib.cb_rank_loss_workspace_bytes() == 4096
    assert lib.cb_rank_loss_fwd_f32(5, P8, 2, P8, 2, None, P8, P8, 4096, None) == -1 and b'kind' in lib.cb_last_error()
    assert lib.cb_rank_loss_fwd_f32(0, P8, 0, P8, 2, None, P8, P8, 4096, None) == -1
    assert lib.cb_rank_loss_fwd_f32(0, P8, 2, P8, 0, None, P8, P8, 4096, None) == -1
    assert lib.cb_rank_loss_fwd_f32(1, P8, 2, P8, 2, None, P8, P8, 4096, None) == -1 and b'null' in lib.cb_last_error()      # adaptive without a weight
    assert lib.cb_rank_loss_fwd_f32(0, P8, 2, P8, 2, None, P8, P8, 8, None) == -3
    assert lib.cb_rank_loss_fwd_f32(0, P8, 2 ** 20, P8, 2 ** 20, None, P8, P8, 4096, None) == -2
    assert lib.cb_rank_loss_bwd_f32(2, P8, 2, P8, 2, None, None, P8, P8, None) == -1 and b'null' in lib.cb_last_error()


def test_the_restatement_equals_the_float64_recordings_of_the_losses():
    cases = load_golden('linkpred_losses')
    assert [(c['span'], c['P'], c['k']) for c in cases] == [(s, P, k) for s in (20.0, 3.0) for P, k in ((1, 1), (5, 3), (257, 7))]
    for c in cases:
        assert c['pos'].dtype == torch.float32 and c['pos'].abs().max() <= c['span'] and tuple(c['neg'].shape) == (c['P'] * c['k'],)
        for kind in lr.KINDS:
            rec = c['kinds'][kind]
            assert rec['f64'].dtype == torch.float64 and rec['f32'].dtype == torch.float32
            assert torch.equal(lr.rank_loss64(kind, c['pos'], c['neg'], c['k'], c['weight']), rec['f64']), (kind, c['span'], c['P'])
            loss, dp, dn = lr.rank_loss_grads64(kind, c['pos'], c['neg'], c['k'], c['weight'])
            assert torch.equal(loss, rec['f64']) and torch.equal(dp, rec['dpos64']) and torch.equal(dn, rec['dneg64'])
            _, dp3, _ = lr.rank_loss_grads64(kind, c['pos'], c['neg'], c['k'], c['weight'], g=3.0)
            torch.testing.assert_close(dp3, 3 * rec['dpos64'], rtol=1e-12, atol=1e-15)
    # the deviation DESIGN.md documents: on saturated scores the reference's fp32 evaluation is far from its own float64 one
    big = next(c for c in cases if c['span'] == 20.0 and c['P'] == 257)['kinds']['ce_loss']
    assert abs(float(big['f32']) - float(big['f64'])) > 0.05 * float(big['f64'])


def test_the_restatement_equals_the_float64_recordings_of_the_predictors():
    rec = load_golden('linkpred_predictors')
    h, pairs, gout = rec['h'], rec['pairs'], rec['gout']
    N = h.shape[0]
    assert int((pairs[0] == 3).sum()) >= 60 and int((pairs[0] == pairs[1]).sum()) >= 10 and int((pairs == N - 1).sum()) >= 10
    for L in (1, 2, 3):
        m = rec['mlp'][L]
        torch.testing.assert_close(lr.mlp_predictor64(m['state_dict'], h[pairs[0]], h[pairs[1]]), m['out64'], rtol=1e-12, atol=1e-14)
        assert tuple(m['out32'].shape) == (pairs.shape[1], 1) and set(m['grads64']) == set(m['state_dict'])
    d = rec['dot']
    torch.testing.assert_close(lr.pair_dot64(h, pairs), d['out64'], rtol=1e-12, atol=1e-14)
    dh, sa = lr.pair_scatter64(h, pairs, gout.reshape(-1))
    torch.testing.assert_close(dh, d['dh64'], rtol=1e-12, atol=1e-14)
    assert bool((sa >= dh.abs() - 1e-12).all())
    # row coefficients: the MLP predictor's dX scattered = the recorded dh of the one-layer module
    m1 = rec['mlp'][1]
    dx = gout @ m1['state_dict']['lins.0.weight'].double()
    torch.testing.assert_close(lr.pair_scatter64(h, pairs, dx)[0], m1['dh64'], rtol=1e-12, atol=1e-14)
    # unusable pairs: NaN score, no contribution
    bad = pairs.clone()
    bad[0, 0], bad[1, 5] = -1, N
    s = lr.pair_dot64(h, bad)
    assert bool(torch.isnan(s[[0, 5]]).all()) and int(torch.isnan(s).sum()) == 2
    keep = torch.ones(pairs.shape[1], dtype=torch.bool)
    keep[[0, 5]] = False
    torch.testing.assert_close(lr.pair_scatter64(h, bad, gout.reshape(-1))[0], lr.pair_scatter64(h, pairs[:, keep], gout.reshape(-1)[keep])[0], rtol=1e-13, atol=1e-15)


def test_calculate_loss_dispatches_as_the_reference_does(monkeypatch):
    from gnn_tail_generalization_amd.Link_prediction_model import model
    calls = []
    for name in lr.KINDS:
        monkeypatch.setattr(model, name, lambda *a, _n=name: calls.append((_n, len(a))) or _n)
    w = object()
    assert model.calculate_loss('ce_loss', 1, 2, 3) == 'ce_loss'
    assert model.calculate_loss('info_nce_loss', 1, 2, 3) == 'info_nce_loss'
    assert model.calculate_loss('log_rank_loss', 1, 2, 3) == 'log_rank_loss'
    assert model.calculate_loss('adaptive_auc_loss', 1, 2, 3, margin=w) == 'adaptive_auc_loss'
    assert model.calculate_loss('adaptive_auc_loss', 1, 2, 3) == 'auc_loss'      # no margin: model.py:115-118
    assert model.calculate_loss('AUC', 1, 2, 3) == 'auc_loss' and model.calculate_loss('anything', 1, 2, 3, margin=w) == 'auc_loss'
    assert calls == [('ce_loss', 2), ('info_nce_loss', 3), ('log_rank_loss', 3), ('adaptive_auc_loss', 4), ('auc_loss', 3), ('auc_loss', 3), ('auc_loss', 3)]


def test_options_mirror_the_reference_defaults():
    from gnn_tail_generalization_amd.base_options import BaseOptions
    a = BaseOptions().get_arguments(['--dataset=S-tiny'])
    assert (a.predictor, a.loss_func, a.num_neg, a.batch_size, a.grad_clip_norm, a.mlp_num_layers, a.mlp_hidden_channels) == ('DOT', 'ce_loss', 3, 65536, 2.0, 2, 256)


@pytest.mark.parametrize('name', ['cb_linkpred', 'cb_linkp'])
def test_the_new_hip_file_compiles_clean_under_wall_without_scratch(name, tmp_path):
    """The cross-compile for gfx950 with the Makefile's flags and -Werror, code generation included, of the two files that share cb_pair_core.h;
    every kernel of either file reports 0 bytes of scratch, and the pair GEMM's 128 x 128 instantiations fit three wavefronts per SIMD."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    src = os.path.join(ROOT, 'gnn-tail-generalization_amd', 'csrc', name + '.hip')
    flags = re.search(r'^FLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    assert '-Wall' in flags
    r = subprocess.run([hipcc] + flags + ['-Werror', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / (name + '.o'))],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0 and 'warning:' not in r.stderr, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    occ = [int(v) for v in re.findall(r'Occupancy \[waves/SIMD\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == len(occ) >= 1
    assert not any(scratch), dict(zip(names, scratch))
    if name == 'cb_linkpred':
        pair = [n for n in names if 'k_gather_gemm_nn_l3' in n and 'PairRowOperand' in n]      # (the kernel template of cb_gather_gemm.h over the pair operand)
        assert len(names) >= 12 and len(pair) == 3 and sum('k_gather_gemm_nn_l3' in n for n in names) == 3
        for n, o in zip(names, occ):
            if 'k_gather_gemm_nn_l3ILi2ELi2ELi2E' in n:
                assert o >= 3, (n, o)


def test_the_status_ledger_adds_up_and_forgets():
    """ops._Ledger behind pair_check() / pair_scores_check(): two words added, one drain returns their fold, the next drain finds nothing."""
    from gnn_tail_generalization_amd import ops
    led = ops._Ledger()
    assert led.drain() == 0
    first = torch.tensor([2], dtype=torch.int32)
    led.add(first)
    led.add(torch.tensor([3], dtype=torch.int32))
    assert int(first) == 2                      # the caller's own status tensor is not accumulated into
    assert led.drain() == 5 and led.drain() == 0
    top = ops._Ledger(torch.fmax, max)
    top.add(torch.tensor([4.0]))
    top.add(torch.tensor([9.0]))
    top.add(torch.tensor([1.0]))
    assert top.drain() == 9.0 and top.drain() == 0
