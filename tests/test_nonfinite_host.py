"""CPU: the cases of tests/nonfinite_cases.py are what tests/test_gpu_nonfinite.py needs them to be.  For every case, with the NaN poison, the float64
restatement is NaN exactly on the structural dependency set (so neither is vacuous or wrong about the other: the restatement computes, the set is read off
shapes and edges), something is poisoned and something stays clean along the case's axis (rows; columns for a bias, which reaches every row), the
poison sits on an interior element that the operand-side dropout keeps, and the +-Inf variants leave every element outside the set finite."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nc


def _setup(op, kind, where):
    o = nc.operands_of(op)
    keep = op.keep(o, nc.host_mask)
    name, idx = op.position(o, where, keep)
    return o, keep, name, idx, op.ref(nc.poisoned(o, name, idx, kind), keep), op.dep(o, where, idx)


@pytest.mark.parametrize('case', [c for c in nc.CASES if c[1] == 'nan'], ids=nc.case_id)
def test_restatement_is_nan_exactly_on_the_dependency_set(case):
    op, kind, where = case
    o, keep, name, idx, ref, dep = _setup(op, kind, where)
    assert set(ref) == set(dep)
    for out in ref:
        assert ref[out].dtype == torch.float64 and ref[out].shape == dep[out].shape, out
        assert torch.equal(torch.isnan(ref[out]), dep[out]), (out, int(torch.isnan(ref[out]).sum()), int(dep[out].sum()))
    # not vacuous: along the case's axis the primary output has a poisoned line and an entirely finite one
    first = next(iter(ref))
    d = dep[first] if dep[first].dim() == 2 else dep[first][:, None]
    lines = d.any(0) if where == 'bias' else d.any(1)
    assert bool(lines.any()) and not bool(lines.all()), first
    # the position: interior, and kept by the dropout in front of it
    t = o[name]
    if where == 'input':
        assert all(0 < i < s - 1 for i, s in zip(idx, t.shape)), idx
        if name in keep:
            assert bool(keep[name][idx])
    # the elements a dropout leaves undecided lie inside the dependency set's outputs and never cover all of it
    for out, und in op.undecided(o, keep, where, idx).items():
        assert und.shape == dep[out].shape and bool((dep[out] & ~und).any()), out


@pytest.mark.parametrize('case', [c for c in nc.CASES if c[1] != 'nan'], ids=nc.case_id)
def test_infinity_stays_inside_the_dependency_set(case):
    op, kind, where = case
    o, keep, name, idx, ref, dep = _setup(op, kind, where)
    clean = op.ref(o, keep)
    hit = False
    for out in ref:
        outside = ~dep[out]
        assert torch.equal(ref[out][outside], clean[out][outside]), out      # (lse = -inf of a row without in-edges is the clean value too)
        hit = hit or bool((~torch.isfinite(ref[out][dep[out]])).any())
    # +Inf reaches the output somewhere (-Inf may not: ReLU clears a -Inf bias in every row; the clean elements are what such a case still checks)
    assert hit or kind == 'ninf'


def test_clean_restatements_are_finite_and_signed():
    """Every clean restatement is finite (but lse = -inf on rows without in-edges) and its ReLU outputs hold both zeros and positive values: a ReLU that
    did nothing, or cleared everything, would not be noticed otherwise."""
    for op in nc.OPS:
        o = nc.operands_of(op)
        ref = op.ref(o, op.keep(o, nc.host_mask))
        for out, r in ref.items():
            if out == 'lse':
                assert bool((torch.isfinite(r) | (r == float('-inf'))).all()) and bool((r == float('-inf')).any()), op
                continue
            assert bool(torch.isfinite(r).all()), (op, out)
        first = ref.get('act', next(iter(ref.values())))      # (the stores' primary output is the mix; their ReLU output is 'act')
        if not (isinstance(op, nc.Attn) and not op.relu):
            assert bool((first == 0).any()) and bool((first > 0).any()), op


def test_relu_table():
    bits = nc.relu_table_bits()
    v = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    nan = torch.isnan(v).numpy()
    assert nan.sum() >= 20 and (~nan).sum() == 14 and len(set(bits.tolist())) == len(bits)
    want = nc.relu_bits_restated(bits)
    got = torch.relu(v).view(torch.int32).numpy().view(np.uint32)
    # torch.relu on the CPU agrees with the integer restatement off NaN, up to the sign of a zero (which torch.relu(-0.0) keeps), and keeps every NaN
    assert np.array_equal(got[~nan] & np.uint32(0x7FFFFFFF), want[~nan]) and bool(torch.isnan(torch.relu(v))[torch.from_numpy(nan)].all())
    assert want[~nan].tolist().count(0) == 8      # +-0 and the six negative values
