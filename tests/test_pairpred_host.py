"""Host-side checks (no GPU) of the BIL / MLPDOT / MLPBIL / MLPCAT link predictors: the C ABI of csrc/cb_pairpred.hip is declared, exported and bound
with matching argument counts, its predicates answer as documented and its entries refuse bad arguments before any launch; the classes of
Link_prediction_model/pair_predictor.py carry the reference's parameter names, shapes and same-seed initialisation (tests/golden/pairpred_predictors.pt,
recorded from the unmodified reference by tools/gen_pairpred_golden.py); the factory maps the six names; CPU tensors are refused; the float64
restatement of tests/pairpred_ref.py equals the recordings; the new HIP file compiles clean under -Wall without scratch."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import pairpred_ref as pr
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_rows_gemm_nn_supported', 'cb_rows_gemm_nn_f32', 'cb_rows_bilinear_supported', 'cb_rows_bilinear_workspace_bytes', 'cb_rows_bilinear_f32',
               'cb_rows_scatter_f32']
P8 = ctypes.c_void_p(16)      # a non-null, 16-byte aligned pointer that is never dereferenced: the checks below answer before any launch
BAD = ctypes.c_void_p(20)     # ... and one that is not 16-byte aligned


def _classes():
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    return {'bil': lambda L, w=16: pp.BilinearPairPredictor(16), 'mlpdot': lambda L, w=16: pp.MLPDotPairPredictor(16, w, L, 0.5),
            'mlpbil': lambda L, w=16: pp.MLPBilPairPredictor(16, w, L, 0.5), 'mlpcat': lambda L, w=16: pp.MLPCatPairPredictor(16, w, 1, L, 0.5)}


def test_c_abi_of_the_pairpred_kernels():
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
    from gnn_tail_generalization_amd import ops
    for fn in (ops.rows_linear, ops.pair_bilinear, ops.pair_scatter_rows, ops.rows_linear_supported, ops.pair_bilinear_supported):
        assert callable(fn)
    assert ops.rows_linear.check is ops.pair_check and ops.pair_bilinear.check is ops.pair_check
    assert list(inspect.signature(ops.rows_linear).parameters) == ['h', 'idx', 'weight', 'bias', 'relu', 'p', 'seed', 'row0', 'return_status', 'fused']
    assert list(inspect.signature(ops.pair_bilinear).parameters) == ['h', 'pairs', 'weight', 'return_status']
    assert list(inspect.signature(ops.pair_scatter_rows).parameters) == ['pairs', 'g0', 'g1', 'n_rows', 'out']


def test_the_fused_form_exists_where_documented():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    sup = lib.cb_rows_gemm_nn_supported      # (h, ld, D, nseg, B, ldb, Nout)
    assert sup(P8, 16, 16, 2, P8, 8, 8) == 1           # two segments, D = 16: a K step ends at the seam
    assert sup(P8, 20, 20, 2, P8, 8, 8) == 0           # D = 20: a K step would straddle it
    assert sup(P8, 20, 20, 1, P8, 8, 8) == 1           # one segment needs D % 4 only
    assert sup(P8, 18, 18, 1, P8, 8, 8) == 0           # D % 4
    assert sup(P8, 256, 256, 1, P8, 6, 6) == 0         # Nout % 4
    assert sup(P8, 258, 256, 1, P8, 8, 8) == 0         # ld % 4
    assert sup(P8, 256, 256, 1, P8, 10, 8) == 0        # ldb % 4
    assert sup(P8, 8, 16, 1, P8, 8, 8) == 0            # ld < D
    assert sup(BAD, 256, 256, 1, P8, 8, 8) == 0 and sup(P8, 256, 256, 1, BAD, 8, 8) == 0      # misaligned rows
    assert sup(None, 256, 256, 1, P8, 8, 8) == 0 and sup(P8, 256, 256, 1, None, 8, 8) == 0
    assert sup(P8, 256, 256, 3, P8, 8, 8) == 0 and sup(P8, 256, 256, 0, P8, 8, 8) == 0        # nseg
    bil = lib.cb_rows_bilinear_supported     # (h, ld, D, Wt, ldw)
    assert bil(P8, 16, 16, P8, 16) == 1 and bil(P8, 132, 132, P8, 132) == 1
    assert bil(P8, 6, 6, P8, 6) == 0 and bil(BAD, 16, 16, P8, 16) == 0 and bil(P8, 16, 16, None, 16) == 0
    wsb = lib.cb_rows_bilinear_workspace_bytes
    assert wsb(0, 16) == 0 and wsb(5, 0) == 0
    assert wsb(5, 64) == 5 * 4 and wsb(5, 128) == 5 * 4 and wsb(5, 132) == 5 * 2 * 4 and wsb(65536, 256) == 65536 * 2 * 4


def test_bad_arguments_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()

    def gemm(h=P8, ld=16, N=5, D=16, idx=P8, nseg=1, R=3, B=P8, ldb=8, C=P8, ldc=8, C2=None, ldc2=8, Nout=8, p=0.0, status=P8):
        return lib.cb_rows_gemm_nn_f32(h, ld, N, D, idx, nseg, R, B, ldb, C, ldc, C2, ldc2, Nout, None, 0, p, 1, None, 0, status, None)
    assert gemm(status=None) == -1 and b'status' in lib.cb_last_error()
    assert gemm(N=0) == -1 and gemm(R=-1) == -1 and gemm(p=1.0) == -1 and gemm(nseg=3) == -1 and b'nseg' in lib.cb_last_error()
    assert gemm(N=2 ** 31) == -2 and gemm(R=2 ** 30) == -2

    def bil(h=P8, ld=16, N=5, D=16, pairs=P8, S=3, Wt=P8, ldw=16, scores=P8, status=P8, ws=P8, wsb=1 << 20):
        return lib.cb_rows_bilinear_f32(h, ld, N, D, pairs, S, Wt, ldw, scores, status, ws, wsb, None)
    assert bil(ld=8) == -1 and b'ld >= D' in lib.cb_last_error()
    assert bil(ldw=8) == -1 and bil(N=0) == -1 and bil(S=-1) == -1
    assert bil(status=None) == -1 and b'status' in lib.cb_last_error()
    assert bil(S=2 ** 30) == -2 and bil(N=2 ** 31) == -2

    def scat(N=5, D=8, pairs=P8, S=3, G0=P8, ld0=8, G1=P8, ld1=8, dh=P8, ldd=8, ws=P8, wsb=1 << 20):
        return lib.cb_rows_scatter_f32(N, D, pairs, S, G0, ld0, G1, ld1, dh, ldd, ws, wsb, None)
    assert scat(ld0=4) == -1 and b'ld0' in lib.cb_last_error()
    assert scat(ld1=4) == -1 and scat(ldd=4) == -1 and scat(N=0) == -1 and scat(D=0) == -1 and scat(S=-1) == -1
    assert scat(G1=None) == -1 and b'null' in lib.cb_last_error()
    assert scat(dh=None) == -1 and scat(pairs=None) == -1
    assert scat(wsb=8) == -3 and scat(ws=None) == -3      # workspace too small / missing
    assert scat(S=2 ** 30) == -2


@pytest.mark.parametrize('kind', pr.KINDS)
@pytest.mark.parametrize('L', [1, 2, 3])
def test_parameter_names_shapes_and_same_seed_initialisation(kind, L):
    rec = load_golden('pairpred_predictors')[kind][L]
    torch.manual_seed(rec['seed'])
    m = _classes()[kind](L)
    assert list(m.state_dict()) == list(rec['state_dict'])      # names in the reference's creation order (lins.* before bilin.weight)
    for k, v in rec['state_dict'].items():
        assert m.state_dict()[k].shape == v.shape and torch.equal(m.state_dict()[k], v), k
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
    torch.manual_seed(rec['seed'])
    m.reset_parameters()
    for k, v in rec['state_dict'].items():
        assert torch.equal(m.state_dict()[k], v), k


def test_constructor_arguments_are_the_references():
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    sig = lambda c: list(inspect.signature(c.__init__).parameters)      # noqa: E731
    assert sig(pp.BilinearPairPredictor) == ['self', 'hidden_channels']
    assert sig(pp.MLPDotPairPredictor) == sig(pp.MLPBilPairPredictor) == ['self', 'in_channels', 'hidden_channels', 'num_layers', 'dropout']
    assert sig(pp.MLPCatPairPredictor) == ['self', 'in_channels', 'hidden_channels', 'out_channels', 'num_layers', 'dropout']
    for c in (pp.BilinearPairPredictor, pp.MLPDotPairPredictor, pp.MLPBilPairPredictor, pp.MLPCatPairPredictor):
        assert list(inspect.signature(c.forward).parameters) == ['self', 'x_i', 'x_j'] and list(inspect.signature(c.score_pairs).parameters) == ['self', 'h', 'pairs']


def test_the_factory_maps_six_names_and_keeps_the_width_one_quirk():
    from gnn_tail_generalization_amd import Link_prediction_model as lpm
    from gnn_tail_generalization_amd.Link_prediction_model import layer, pair_predictor as pp
    make = lpm.create_pair_predictor_layer
    assert make is pp.create_pair_predictor_layer
    assert list(inspect.signature(make).parameters) == ['hidden_channels', 'num_layers', 'dropout', 'predictor_name']
    assert type(make(8, 2, 0.1, 'dot')) is layer.DotPredictor
    m = make(8, 3, 0.25, 'MLP')
    assert type(m) is layer.MLPPredictor and [tuple(l.weight.shape) for l in m.lins] == [(8, 8), (8, 8), (1, 8)]
    b = make(8, 2, 0.1, 'bil')
    assert type(b) is pp.BilinearPairPredictor and tuple(b.bilin.weight.shape) == (8, 8) and b.bilin.bias is None
    d = make(8, 3, 0.25, 'MLPDOT')
    assert type(d) is pp.MLPDotPairPredictor and d.dropout == 0.25 and [tuple(l.weight.shape) for l in d.lins] == [(1, 8), (1, 1), (1, 1)]
    q = make(8, 2, 0.25, 'mlpbil')
    assert type(q) is pp.MLPBilPairPredictor and [tuple(l.weight.shape) for l in q.lins] == [(1, 8), (1, 1)] and tuple(q.bilin.weight.shape) == (1, 1)
    c = make(8, 3, 0.5, 'MLPCat')
    assert type(c) is pp.MLPCatPairPredictor and [tuple(l.weight.shape) for l in c.lins] == [(8, 16), (8, 8), (1, 8)]
    with pytest.raises(NotImplementedError, match='not implemented'):
        make(8, 2, 0.0, 'nope')
    wo = load_golden('pairpred_predictors')['width_one']
    for kind in ('mlpdot', 'mlpbil'):      # the recording of the reference under the factory's widths
        torch.manual_seed(wo[kind]['seed'])
        m = make(16, 2, 0.5, kind)
        assert all(torch.equal(m.state_dict()[k], v) for k, v in wo[kind]['state_dict'].items()) and list(m.state_dict()) == list(wo[kind]['state_dict'])


def test_cpu_tensors_are_refused():
    from gnn_tail_generalization_amd import _lib, ops
    h, pairs = torch.ones(6, 16), torch.zeros((2, 4), dtype=torch.int64)
    mods = [make(2) for make in _classes().values()]
    fns = [lambda: ops.rows_linear(h, pairs, torch.ones(8, 32)), lambda: ops.rows_linear(h, pairs[:1], torch.ones(8, 16)),
           lambda: ops.pair_bilinear(h, pairs, torch.ones(16, 16)), lambda: ops.pair_scatter_rows(pairs, torch.ones(4, 16), torch.ones(4, 16), 6)]
    fns += [lambda m=m: m.score_pairs(h, pairs) for m in mods] + [lambda m=m: m(h[:4], h[:4]) for m in mods]
    for fn in fns:
        with pytest.raises(_lib.HipExtensionError):
            fn()


def test_the_restatement_equals_the_float64_recordings():
    rec = load_golden('pairpred_predictors')
    h, pairs, gout = rec['h'], rec['pairs'], rec['gout']
    assert (rec['N'], rec['D'], rec['S']) == (40, 16, 50) and tuple(h.shape) == (40, 16) and tuple(pairs.shape) == (2, 50) and h.dtype == torch.float32
    assert int((pairs[0] == 3).sum()) >= 12 and int((pairs[0] == pairs[1]).sum()) >= 5 and int((pairs == 39).sum()) >= 4
    cases = [(kind, L, rec[kind][L]) for kind in pr.KINDS for L in (1, 2, 3)] + [(kind, 2, rec['width_one'][kind]) for kind in ('mlpdot', 'mlpbil')]
    for kind, L, r in cases:
        out, dh, grads = pr.predictor_grads64(kind, r['state_dict'], h, pairs, gout)
        assert r['out64'].dtype == torch.float64 and r['out32'].dtype == torch.float32
        assert tuple(r['out64'].shape) == ((50, 1) if kind == 'mlpcat' else (50,)) and set(r['grads64']) == set(r['state_dict'])
        torch.testing.assert_close(out, r['out64'], rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(dh, r['dh64'], rtol=1e-11, atol=1e-13)
        for k in grads:
            torch.testing.assert_close(grads[k], r['grads64'][k], rtol=1e-11, atol=1e-13)
        # the magnitude network bounds the real one entry by entry
        a_out, a_dh, _ = pr.predictor_abs64(kind, r['state_dict'], h, pairs, gout)
        assert bool((a_out >= out.abs() - 1e-12).all()) and bool((a_dh >= dh.abs() - 1e-12).all())
    # the bilinear form and the row scatter of the restatement against the recorded BIL module
    r = rec['bil'][1]
    s, scale = pr.bilinear64(h, pairs, r['state_dict']['bilin.weight'])
    torch.testing.assert_close(s, r['out64'], rtol=1e-12, atol=1e-14)
    assert bool((scale >= s.abs()).all())
    W, g = r['state_dict']['bilin.weight'].double(), gout.double()
    dh, sa = pr.scatter_rows64(pairs, g * (h.double()[pairs[1]] @ W), g * (h.double()[pairs[0]] @ W.t()), 40)
    torch.testing.assert_close(dh, r['dh64'], rtol=1e-11, atol=1e-13)
    bad = pairs.clone()
    bad[0, 0], bad[1, 5] = -1, 40
    s = pr.bilinear64(h, bad, W)[0]
    assert bool(torch.isnan(s[[0, 5]]).all()) and int(torch.isnan(s).sum()) == 2
    keep = torch.ones(50, dtype=torch.bool)
    keep[[0, 5]] = False
    g0, g1 = torch.ones(50, 3), torch.full((50, 3), 2.0)
    assert torch.equal(pr.scatter_rows64(bad, g0, g1, 40)[0], pr.scatter_rows64(pairs[:, keep], g0[keep], g1[keep], 40)[0])


def test_the_trainer_options_name_the_six_predictors():
    from gnn_tail_generalization_amd.base_options import BaseOptions
    for name in ('DOT', 'MLP', 'BIL', 'MLPDOT', 'MLPBIL', 'MLPCAT'):
        assert BaseOptions().get_arguments(['--dataset=S-tiny', f'--predictor={name}']).predictor == name


def test_the_new_hip_file_compiles_clean_under_wall_without_scratch(tmp_path):
    """The cross-compile for gfx950 with the Makefile's flags and -Werror, code generation included: every kernel reports 0 bytes of scratch and no
    spilled register (the wide 128 x 256 tile of the indexed-row GEMM included), and the 128 x 128 instantiations fit three wavefronts per SIMD."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    src = os.path.join(ROOT, 'gnn-tail-generalization_amd', 'csrc', 'cb_pairpred.hip')
    flags = re.search(r'^FLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    assert '-Wall' in flags
    r = subprocess.run([hipcc] + flags + ['-Werror', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / 'cb_pairpred.o')],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0 and 'warning:' not in r.stderr, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    spill = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', r.stderr)]
    occ = [int(v) for v in re.findall(r'Occupancy \[waves/SIMD\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) == len(spill) == len(occ) >= 1
    assert not any(scratch) and not any(spill), dict(zip(names, zip(scratch, spill)))
    rows = [n for n in names if 'k_gather_gemm_nn_l3' in n and 'IndexedRowOperand' in n]      # (the kernel template of cb_gather_gemm.h over the indexed operand)
    assert len(rows) == 10 and sum('k_gather_gemm_nn_l3' in n for n in names) == 10 and sum('k_pair_bilinear_l3' in n for n in names) == 2      # 2 segment counts x (256x64, two 128-row tiles x 2 epilogues)
    assert sum('k_gather_gemm_nn_l3ILi2ELi2ELi4E' in n for n in rows) == 4
    for n, o in zip(names, occ):
        if 'k_gather_gemm_nn_l3ILi2ELi2ELi2E' in n or 'k_pair_bilinear_l3ILi2ELi2ELi2E' in n:
            assert o >= 3, (n, o)
        elif 'k_gather_gemm_nn_l3' in n or 'k_pair_bilinear_l3' in n:
            assert o >= 2, (n, o)
