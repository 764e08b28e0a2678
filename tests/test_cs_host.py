"""Host-side checks of Correct & Smooth (no GPU): the fp64 restatement tests/cs_ref.py against the fixtures the unmodified reference wrote
(tests/golden/cs_*.pt, tests/golden/make_cs_golden.py), the option values of set_labprop_configs, the C ABI of the new entries and their
argument checks, and the Label_propagation_model package surface."""
import contextlib
import ctypes
import io
import os
import re

import pytest
import torch

import cs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_spmm_csr_prop_f32', 'cb_cs_workspace_bytes', 'cb_cs_residual_init_f32', 'cb_cs_correct_snap_f32']
EXPECTED_CASES = {f'cs_{f}_{a1}_{a2}_c{c}' for f in ('autoscale', 'fixed', 'only') for a1, a2 in (('DA', 'AD'), ('DAD', 'DAD'), ('AD', 'DA')) for c in (3, 7)} | {
    'cs_autoscale_DA_AD_c47', 'cs_branch_autoscale', 'cs_general_noalpha_identity', 'cs_general_clamp_1e-6'}


def test_the_fixture_set_is_complete():
    assert set(cs_ref.cs_cases()) == EXPECTED_CASES
    for name in cs_ref.cs_cases():
        assert os.path.getsize(os.path.join(cs_ref.GOLDEN, name + '.pt')) < 363333      # (the smallest student fixture with weights)
        assert cs_ref.load_case(name)['y'].shape[0] <= 512


@pytest.mark.parametrize('name', sorted(EXPECTED_CASES))
def test_restatement_reproduces_the_reference(name):
    """Pins tests/cs_ref.py to the unmodified reference: every recorded output to 1e-5 (the generator measured <= 1e-6)."""
    g = cs_ref.load_case(name)
    got = cs_ref.case_outputs64(g)
    for k, v in got.items():
        err = float((v - g[k].double()).abs().max())
        print(name, k, 'max |fp64 - reference| =', err, '(recorded', g['ref_err64'], ')')
        torch.testing.assert_close(v, g[k].double(), atol=1e-5, rtol=1e-5)
        assert err <= g['ref_err64'] * 1.0000001 + 1e-12
    if g['kind'] == 'cs':
        acc = [cs_ref.accuracy(m, g['y'], g[k]) for m in (g['model_out'], got['result']) for k in ('train_mask', 'test_mask')]
        assert acc == g['acc'].tolist()


def test_branch_case_has_the_margin_it_promises():
    g = cs_ref.load_case('cs_branch_autoscale')
    n = g['y'].shape[0]
    ei = cs_ref.to_undirected(g['edge_index'], n)
    _, _, parts = cs_ref.correct_and_smooth64(g['fn'], ei, n, g['y'], g['model_out'], g['label_idx'], g['A1'], g['alpha1'], g['num_propagations1'],
                                              g['A2'], g['alpha2'], g['num_propagations2'], want_parts=True)
    ratio = parts['ratio'].reshape(-1)
    fin = ratio[torch.isfinite(ratio)]
    assert int(ratio.isinf().sum()) == g['n_inf'] >= 1 and int((fin > 1000).sum()) == g['n_big'] >= 1
    assert float(((fin - 1000).abs() / 1000).min()) > 0.05
    assert n == 370 and not bool((g['train_mask'] | g['valid_mask'])[300:].any())


def _product_args(argv):
    from gnn_tail_generalization_amd.base_options import BaseOptions
    with contextlib.redirect_stdout(io.StringIO()):
        return BaseOptions().get_arguments(['--dataset=Cora', '--manual_assign_GPU=0'] + list(argv))


@pytest.mark.parametrize('key', ['default', 'overrides'])
def test_set_labprop_configs_reproduces_the_reference(key):
    ref = torch.load(os.path.join(cs_ref.GOLDEN, 'cs_options.pt'), weights_only=False)[key]
    args = _product_args(ref['argv'])
    assert args.lp_has_prep == ref['lp_has_prep'] and args.correct_and_smooth == 0
    for group in ('lpStep', 'preStep', 'midStep'):
        assert vars(getattr(args, group)) == ref[group], group
    # the one new flag: Correct & Smooth instead of plain label propagation, nothing else moves
    on = _product_args(ref['argv'] + ['--correct_and_smooth=1'])
    assert on.lpStep.no_prep == 0 and {k: v for k, v in vars(on.lpStep).items() if k != 'no_prep'} == {k: v for k, v in ref['lpStep'].items() if k != 'no_prep'}


def test_c_abi_of_the_correct_and_smooth_entries():
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
    L = _lib.load()
    assert L.cb_version() == 5
    inf = float('inf')
    p8 = ctypes.c_void_p(8)
    # cb_spmm_csr_prop_f32: argument checks answer before anything is launched
    def view(n_rows, rowptr=None, hub=(1, 0, 0, None, None)):
        return _lib.CsrView(rowptr=rowptr, col=None, col_flags=0, n_rows=n_rows, n_edges=0, hub_threshold=hub[0], n_hubs=hub[1], n_chunks=hub[2],
                            hub_rows=hub[3], hub_chunk_ptr=hub[4], ws=None, ws_bytes=0)
    assert L.cb_spmm_csr_prop_f32(view(-1), None, 0, 0, None, None, 0, 0.5, 0.0, 1.0, None, None, None, 0, None) == -1
    assert L.cb_spmm_csr_prop_f32(view(4), None, 0, 4, None, None, 0, 0.5, 1.0, 0.0, None, None, None, 0, None) == -1
    assert b'lo <= hi' in L.cb_last_error()
    assert L.cb_spmm_csr_prop_f32(view(4), None, 0, 4, None, None, 0, 0.5, float('nan'), inf, None, None, None, 0, None) == -1
    assert L.cb_spmm_csr_prop_f32(view(4), None, 4, 4, None, None, 4, 0.5, -inf, inf, None, None, None, 4, None) == -1
    assert b'null pointer' in L.cb_last_error()
    assert L.cb_spmm_csr_prop_f32(view(4, p8), p8, 3, 4, None, p8, 4, 0.5, 0.0, 1.0, None, None, p8, 4, None) == -1
    assert b'leading dimension' in L.cb_last_error()
    assert L.cb_spmm_csr_prop_f32(view(4, p8, (64, 2, 3, p8, p8)), p8, 4, 4, None, p8, 4, 0.5, 0.0, 1.0, None, None, p8, 4, None) == -3
    assert L.cb_spmm_csr_prop_f32(view(2 ** 31), None, 0, 4, None, None, 0, 0.5, 0.0, 1.0, None, None, None, 0, None) == -2
    # the row kernels: workspace query, missing workspace, bad mode / shapes
    assert L.cb_cs_workspace_bytes(0, 7) == 0 and L.cb_cs_workspace_bytes(100, 7) == 4 * 4 and L.cb_cs_workspace_bytes(10 ** 7, 48) == 4 * 1024
    assert L.cb_cs_residual_init_f32(p8, 7, p8, p8, 100, 7, 7, None, p8, None, p8, None, 0, None) == -3
    assert b'workspace' in L.cb_last_error()
    assert L.cb_cs_residual_init_f32(p8, 7, p8, p8, 100, 7, 6, None, p8, None, p8, p8, 64, None) == -1
    assert b'Cp' in L.cb_last_error()
    assert L.cb_cs_residual_init_f32(p8, 7, p8, p8, 100, 7, 7, None, p8, None, None, p8, 64, None) == -1
    assert L.cb_cs_residual_init_f32(p8, 6, p8, p8, 100, 7, 7, None, p8, None, p8, p8, 64, None) == -1
    assert L.cb_cs_correct_snap_f32(3, p8, 7, p8, 7, p8, p8, 100, 7, 7, p8, 10, 1.0, None, p8, 7, p8, None, None) == -1
    assert b'mode' in L.cb_last_error()
    assert L.cb_cs_correct_snap_f32(0, p8, 7, None, 7, p8, p8, 100, 7, 7, p8, 10, 1.0, None, p8, 7, p8, None, None) == -1
    assert L.cb_cs_correct_snap_f32(0, p8, 7, p8, 7, p8, p8, 100, 7, 7, None, 10, 1.0, None, p8, 7, p8, None, None) == -1
    assert L.cb_cs_correct_snap_f32(0, p8, 7, p8, 7, p8, p8, 100, 7, 7, p8, 0, 1.0, None, p8, 7, p8, None, None) == -1
    assert L.cb_cs_correct_snap_f32(1, p8, 7, p8, 6, p8, p8, 100, 7, 7, None, 0, 1.0, None, p8, 7, p8, None, None) == -1
    assert L.cb_cs_correct_snap_f32(2, p8, 7, None, 0, p8, p8, 0, 7, 7, None, 0, 1.0, None, p8, 7, p8, None, None) == 0      # empty: nothing to do


def _lpstep_args(**over):
    args = _product_args(['--correct_and_smooth=1'])
    args.device = torch.device('cpu')
    for k, v in over.items():
        setattr(args.lpStep, k, v)
    return args


def test_label_propagation_model_surface_and_name_resolution():
    from gnn_tail_generalization_amd import Label_propagation_model as lpm, ops
    from gnn_tail_generalization_amd.Label_propagation_model import LP_Adj, outcome_correlation as oc
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    for name in ('process_adj', 'gen_normalized_adjs', 'get_labels_from_name', 'pre_residual_correlation', 'pre_outcome_correlation',
                 'general_outcome_correlation', 'label_propagation', 'double_correlation_autoscale', 'double_correlation_fixed', 'only_outcome_correlation'):
        assert callable(getattr(oc, name)) and getattr(lpm, name) is getattr(oc, name), name
    for name in ('Clamp', 'Identity', 'FixRows'):
        assert isinstance(getattr(lpm, name), type)
    assert callable(ops.propagate) and callable(ops.correct_and_smooth) and callable(trainer.correct_and_smooth)
    g = cs_ref.load_case('cs_autoscale_DA_AD_c7')
    data = type('Data', (), {})()
    data.edge_index, data.y, data.x = g['edge_index'], g['y'], torch.zeros(g['y'].shape[0], 2)
    masks = {'train': g['train_mask'], 'valid': g['valid_mask'], 'test': g['test_mask']}
    step = LP_Adj.LPStep(_lpstep_args(), data, masks)           # no device: the graph is built at the first forward
    assert step.fn is oc.double_correlation_autoscale and step.adj_names == {'A': 'DAD', 'A1': 'DA', 'A2': 'AD'} and not step.no_prep and step.adjs is None
    assert torch.equal(step.split_idx['train'], g['label_idx']) and step.lp_dict['train_only'] is True
    assert (step.lp_dict['alpha1'], step.lp_dict['num_propagations2']) == (g['alpha1'], 50)
    step = LP_Adj.LPStep(_lpstep_args(fn='only_outcome_correlation', A1='AD', A2='DAD'), data, masks)
    assert step.fn is oc.only_outcome_correlation and step.adj_names['A1'] == 'AD'
    # a table, not eval: a name that is not one of the reference's is refused, code in an option string is never run
    for bad in (dict(fn='__import__("os").getcwd'), dict(A1='DAD.t()'), dict(A='D')):
        with pytest.raises(ValueError, match='one of'):
            LP_Adj.LPStep(_lpstep_args(**bad), data, masks)
    assert torch.equal(oc.get_labels_from_name(['train', 'valid'], step.split_idx), torch.cat([step.split_idx['train'], step.split_idx['valid']]))
    with pytest.raises(ValueError, match='one of'):
        ops.adj_scales(torch.ones(3), 'DD')
    R, S = ops.adj_scales(torch.tensor([0.5, 0.25]), 'AD')
    assert R is None and S.tolist() == [0.25, 0.0625]


def test_refusals_name_what_is_missing():
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.dist import ShardedTrainer
    from gnn_tail_generalization_amd.graph import CSRGraph, SegmentedCSRGraph
    with pytest.raises(ValueError, match='segmented'):
        SegmentedCSRGraph.spmm_prop(SegmentedCSRGraph.__new__(SegmentedCSRGraph), None)
    with pytest.raises(ValueError, match='shards'):
        ops._prop_graph(object())
    assert callable(CSRGraph.spmm_prop)
    t = ShardedTrainer.__new__(ShardedTrainer)
    t.args = _product_args(['--correct_and_smooth=1'])
    with pytest.raises(NotImplementedError, match='correct_and_smooth'):
        t.main()
