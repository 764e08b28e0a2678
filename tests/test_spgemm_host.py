"""Host-side checks (no GPU) of the device sparse x sparse product's Python surface: the chunk planner ops.spgemm_plan (pure host), the
refusal of CPU tensors (there is no CPU fallback) and the default of tuning.T.power_on_device, under which GraphMLP.power() keeps the host build."""
import pytest
import torch

import ncloss_ref as nr


def _tiles(chunks, m):
    assert chunks[0][0] == 0 and chunks[-1][1] == m
    assert all(a < b for a, b in chunks) and all(chunks[i][1] == chunks[i + 1][0] for i in range(len(chunks) - 1))


def test_plan_boundaries():
    from gnn_tail_generalization_amd import ops
    rp = [3, 0, 5, 1, 1, 0, 0, 9, 2, 2, 4]
    m = len(rp)
    # budget 1: one row per chunk (every row alone exceeds or meets it; an empty row joins nothing that is full)
    chunks, _ = ops.spgemm_plan([2] * 7, 10, 1)
    assert chunks == [(i, i + 1) for i in range(7)]
    # a row larger than the budget gets a chunk of its own; the others are maximal runs that fit
    chunks, (pb, rb, cb) = ops.spgemm_plan(rp, 300, 6)
    _tiles(chunks, m)
    assert chunks == [(0, 2), (2, 4), (4, 7), (7, 8), (8, 10), (10, 11)]      # 3+0 | 5+1 | 1+0+0 | the 9 alone | 2+2 | 4
    assert (pb, rb, cb) == (3, 2, 9)                                   # [0, 6) in 3 bits, 3 rows in 2, 300 columns in 9
    for a, b in chunks:
        assert sum(rp[a:b]) <= 6 or b - a == 1
        assert b == m or sum(rp[a:b + 1]) > 6                          # maximal
    # tensors and arrays are accepted; one chunk where everything fits; no rows, no chunks
    assert ops.spgemm_plan(torch.tensor(rp), 300, 1 << 26)[0] == [(0, m)]
    assert ops.spgemm_plan([], 300, 8)[0] == []
    assert ops.spgemm_plan([0, 0, 0], 1, 8)[0] == [(0, 3)]


def test_plan_caps_the_rows_of_a_chunk_by_the_key_bits():
    from gnn_tail_generalization_amd import ops
    # 31 column bits + 30 product bits leave 3: at most 8 rows, however few products they hold
    chunks, (pb, rb, cb) = ops.spgemm_plan([1] * 50, 2 ** 31 - 1, 2 ** 30)
    _tiles(chunks, 50)
    assert (pb, rb, cb) == (30, 3, 31) and max(b - a for a, b in chunks) == 8 and chunks[:2] == [(0, 8), (8, 16)]
    assert pb + rb + cb <= 64
    # no split fits 64 bits
    with pytest.raises(ValueError, match='64-bit key'):
        ops.spgemm_plan([1] * 4, 2 ** 31 - 1, 2 ** 40)
    with pytest.raises(ValueError):
        ops.spgemm_plan([1, -1], 10, 4)
    with pytest.raises(ValueError):
        ops.spgemm_plan([1, 1], 10, 0)


def test_cpu_tensors_are_refused():
    from gnn_tail_generalization_amd import _lib, ops
    rowptr, col, val = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), torch.ones(2)
    with pytest.raises(_lib.HipExtensionError):
        ops.spgemm_csr(rowptr, col, val, rowptr, col, val, 2)
    with pytest.raises(_lib.HipExtensionError):
        ops.csr_transpose(rowptr, col, val, 2)
    with pytest.raises(_lib.HipExtensionError):
        ops.SparsePower.from_adjacency(nr.power('powerlaw', 1), 2, 'cpu')


def test_power_on_device_is_off_by_default(monkeypatch):
    from gnn_tail_generalization_amd import ops, tuning
    from gnn_tail_generalization_amd.MLP_model import GraphMLP
    assert tuning.T.power_on_device is False and tuning.Tuning().power_on_device is False
    assert tuning.Tuning().spgemm_chunk_products == 1 << 26

    def refuse(*a, **k):
        raise AssertionError('from_adjacency called with power_on_device off')
    monkeypatch.setattr(ops.SparsePower, 'from_adjacency', classmethod(refuse))
    args = type('A', (), {})()
    args.num_feats, args.num_classes_bkup, args.device, args.batch_size, args.graphMLP_r = 20, 4, torch.device('cpu'), 16, 2
    mask = torch.zeros(300, dtype=torch.bool)
    mask[:30] = True
    ei, _n = nr.graph('powerlaw')
    sp = GraphMLP(args, mask).power(ei)
    assert isinstance(sp, ops.SparsePower) and sp.nnz == nr.power('powerlaw', 2)._nnz()
    # ... and a model on the CPU keeps the host build even with the switch on
    monkeypatch.setattr(tuning.T, 'power_on_device', True)
    assert GraphMLP(args, mask).power(ei).nnz == sp.nnz
