"""GPU: the column sums of every trunk-backward entry and of cb_act_bwd_f32 against the HOST restatement of their two-stage order
(oracle/coldbrew_oracle.py colsum_two_stage; tests/test_colsum_host.py shows it can be told from its neighbouring orders on these inputs) — torch.equal,
no tolerances.  include/coldbrew_hip.h promises that cb_trunk_layer_bwd_f32, its _rows / _fold forms and cb_trunk_input_bwd_multi_cs_f32 sum in the same
order; csrc/cb_rowpass.h block_colsum and csrc/cb_reduce.hip k_colsum_finish are that order, and this test holds them to it.

Inputs: tests/colsum_cases.py (summands that do not depend on how a kernel forms them).  Where an entry stores exactly what it sums (no row scale) its
own output is the summand matrix handed to the restatement (and equals the host-built one); the bf16 and the sums-only form, and the second sums,
are held to the summands built on the host from orc.dropout_keep_mask."""
import ctypes

import pytest
import torch

import colsum_cases as cc
import coldbrew_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROW_IDS = [f'{r}x{d}-p{p}' for r, d, p in cc.ROW_CASES]


def _dev(t):
    return t.to(DEV) if t is not None else None


def _pinned(summands, row_lanes=4):
    """The restatement of the summands (a device tensor the entry wrote, or the host's numpy array) as a device tensor."""
    x = summands.cpu().numpy() if isinstance(summands, torch.Tensor) else summands
    return torch.from_numpy(orc.colsum_two_stage(x, row_lanes)).to(DEV)


def _same(t, host):
    return torch.equal(t, torch.from_numpy(host).to(DEV))


def _layer_bwd(c, p, out, out_bf16, g2, g2_pos, gx0):
    """cb_trunk_layer_bwd_f32 itself (trunk._layer_bwd always hands it an output): out may be None — column sums only."""
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    g, bits = _dev(c['g']), _dev(c['bits'])
    rows, d = g.shape
    colsum = torch.empty(d, device=DEV)
    wsb = lib.cb_colsum_workspace_bytes(rows, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_trunk_layer_bwd_f32(_lib.ptr(g), _lib.ptr(bits), None, _lib.ptr(out), int(out_bf16), _lib.ptr(gx0), 0, rows, d, float(p),
                                              ctypes.c_uint64(c['seed']), None, cc.ROW0, cc.C_ACT, cc.C_MIX, _lib.ptr(g2), ctypes.c_uint64(c['seed2']),
                                              cc.C2 if g2 is not None else 0.0, _lib.ptr(g2_pos), _lib.ptr(colsum), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                   'cb_trunk_layer_bwd_f32')
    return colsum


@pytest.mark.parametrize('rows,d,p', cc.ROW_CASES, ids=ROW_IDS)
def test_layer_backward_column_sums(rows, d, p):
    """cb_trunk_layer_bwd_f32: fp32 out, bf16 out and no out; without g2, with a dense and with a compact one."""
    c = cc.make('layer', rows, d, p)
    for kind, g2, pos in (('none', None, None), ('dense', _dev(c['g2']), None), ('compact', _dev(c['g2c']), _dev(c['g2_pos']))):
        host = c['sum_' + kind]
        out, gx0 = torch.empty(rows, d, device=DEV), torch.empty(rows, d, device=DEV)
        cs = _layer_bwd(c, p, out, False, g2, pos, gx0)
        assert _same(out, host) and _same(gx0, c['gx0']), kind
        assert torch.equal(cs, _pinned(out)), kind
        out16 = torch.empty(rows, d, dtype=torch.bfloat16, device=DEV)
        cs16 = _layer_bwd(c, p, out16, True, g2, pos, None)
        assert torch.equal(out16, torch.from_numpy(host).to(DEV).to(torch.bfloat16)), kind
        assert torch.equal(cs16, _pinned(host)), kind
        assert torch.equal(_layer_bwd(c, p, None, False, g2, pos, None), _pinned(host)), kind


@pytest.mark.parametrize('rows,d,p', cc.ROW_CASES, ids=ROW_IDS)
def test_layer_backward_on_compact_rows_column_sums(rows, d, p):
    from gnn_tail_generalization_amd import trunk
    c = cc.make('layer_rows', rows, d, p)
    out, cs = trunk._layer_bwd_rows(_dev(c['g']), _dev(c['idx']), _dev(c['bits']), None, p, c['seed'], cc.ROW0, cc.C_ACT, True, g2=_dev(c['g2c']),
                                    seed2=c['seed2'], c2=cc.C2, g2_pos=_dev(c['g2_pos']))
    assert _same(out, c['sum'])
    assert torch.equal(cs, _pinned(out))


@pytest.mark.parametrize('rows,d,p', cc.ROW_CASES, ids=ROW_IDS)
def test_layer_backward_fold_column_sums(rows, d, p):
    """cb_trunk_layer_bwd_fold_f32: the layer's sum and the second one, through the mask words of another store."""
    from gnn_tail_generalization_amd import trunk
    c = cc.make('fold', rows, d, p)
    out, cs, m, cs2 = trunk._layer_bwd_fold(_dev(c['g']), _dev(c['bits']), None, p, c['seed'], cc.ROW0, cc.C_ACT, cc.C_MIX, True, [_dev(c['dense']), _dev(c['comp'])],
                                            [None, _dev(c['pos'])], c['seeds'], cs=(1, _dev(c['cs_bits']), cc.CS_C))
    assert _same(out, c['sum']) and _same(m, c['m'])
    assert torch.equal(cs, _pinned(out))
    assert torch.equal(cs2, _pinned(c['sum2']))


@pytest.mark.parametrize('rows,d,p', cc.ROW_CASES, ids=ROW_IDS)
def test_input_backward_column_sums(rows, d, p):
    from gnn_tail_generalization_amd import trunk
    c = cc.make('input', rows, d, p)
    out, cs = trunk._input_bwd(_dev(c['g']), _dev(c['add']), _dev(c['act']), p, c['seed'], cc.ROW0)
    assert _same(out, c['sum'])
    assert torch.equal(cs, _pinned(out))


@pytest.mark.parametrize('rows,d,p', cc.ROW_CASES, ids=ROW_IDS)
def test_input_backward_multi_column_sums(rows, d, p):
    """cb_trunk_input_bwd_multi_cs_f32: three mixed-in gradients (the second compact) and both extra sums."""
    from gnn_tail_generalization_amd import trunk
    c = cc.make('multi', rows, d, p)
    out, cs, cs2 = trunk._input_bwd_multi(_dev(c['g']), c['seed'], [_dev(c['d0']), _dev(c['comp']), _dev(c['d2'])], c['seeds'], cc.C_MIX, None, p, cc.ROW0,
                                          act_bits=_dev(c['act_bits']), mix_pos=[None, _dev(c['pos']), None],
                                          cs=[(1, _dev(c['cs_bits'][0]), cc.CS_C), (2, _dev(c['cs_bits'][1]), cc.CS_C)])
    assert _same(out, c['sum'])
    assert torch.equal(cs, _pinned(out))
    for q in range(2):
        assert torch.equal(cs2[q], _pinned(c['sum2'][q])), q


@pytest.mark.parametrize('rows,d', cc.ACT_SHAPES)
def test_act_backward_column_sums(rows, d):
    """cb_act_bwd_f32: 256 // min(64, ceil(d / 4)) row lanes per block."""
    from gnn_tail_generalization_amd import ops
    c = cc.make_act(rows, d)
    out, cs = ops.act_bwd(_dev(c['g']), _dev(c['act']), None, want_out=True, want_colsum=True)
    assert _same(out, c['sum'])
    assert torch.equal(cs, _pinned(out, cc.act_row_lanes(d)))
