"""The host reference of the top-K replacement (tests/topk_ref.py) against the oracle's per-node restatement where there are no ties,
and against a selection written out by hand where there are."""
import math

import numpy as np
import torch

import coldbrew_oracle as orc
import topk_ref


def test_matches_the_oracle_on_tie_free_data():
    for b, n, d, k, seed in [(1, 5, 3, 1, 0), (40, 300, 17, 2, 1), (33, 129, 64, 8, 2), (7, 8, 4, 8, 3)]:
        gen = torch.Generator().manual_seed(seed)
        q, t = torch.randn(b, d, generator=gen, dtype=torch.float64), torch.randn(n, d, generator=gen, dtype=torch.float64)
        rk = topk_ref.Ranking(q.numpy(), t.numpy())
        assert float(rk.min_gap(k).min()) > 0 and not rk.boundary_ties(k).any()       # tie-free: the two argsorts must agree
        want, sel, w = orc.semlp_replacement(q, t, k)
        out, idx, wgt = rk.select(k)
        assert np.array_equal(idx, sel.numpy()), (b, n, d, k)
        np.testing.assert_allclose(wgt, w.numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(out, want.numpy(), rtol=1e-12, atol=1e-14)
        out2, idx2, wgt2 = topk_ref.replacement(q.numpy(), t.numpy(), k)
        assert np.array_equal(idx2, idx) and np.array_equal(out2, out) and np.array_equal(wgt2, wgt)


def test_ties_go_to_the_larger_index():
    t = np.array([[1.0], [1.0], [2.0], [1.0]])
    q = np.array([[1.0], [-1.0], [0.0]])
    # scores: row 0 = (1, 1, 2, 1), row 1 = (-1, -1, -2, -1), row 2 = (0, 0, 0, 0)
    # stable ascending orders:   0 1 3 2              2 0 1 3              0 1 2 3
    rk = topk_ref.Ranking(q, t)
    assert rk.select(1)[1].tolist() == [[2], [3], [3]]
    assert rk.select(2)[1].tolist() == [[3, 2], [1, 3], [2, 3]]
    assert rk.select(3)[1].tolist() == [[1, 3, 2], [0, 1, 3], [1, 2, 3]]
    assert rk.select(4)[1].tolist() == [[0, 1, 3, 2], [2, 0, 1, 3], [0, 1, 2, 3]]
    assert rk.boundary_ties(1).tolist() == [False, True, True]
    assert rk.boundary_ties(2).tolist() == [True, True, True]
    assert rk.boundary_ties(3).tolist() == [True, False, True]
    assert rk.boundary_ties(4).tolist() == [False, False, False]
    assert rk.min_gap(1).tolist() == [1.0, 0.0, 0.0] and rk.min_gap(4).tolist() == [0.0, 0.0, 0.0]
    out, idx, wgt = rk.select(2)
    e = math.e
    np.testing.assert_allclose(wgt, [[1 / (1 + e), e / (1 + e)], [0.5, 0.5], [0.5, 0.5]], rtol=1e-15)
    np.testing.assert_allclose(out, [[(1 + 2 * e) / (1 + e)], [1.0], [1.5]], rtol=1e-15)


def test_small_integer_scores_are_exact():
    rng = np.random.default_rng(0)
    q = rng.integers(-3, 4, size=(64, 16)).astype(np.float32)
    t = rng.integers(-3, 4, size=(700, 16)).astype(np.float32)
    s = topk_ref.scores_f64(q, t)
    assert np.array_equal(s, (q.astype(np.int64) @ t.astype(np.int64).T).astype(np.float64))
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)            # and representable in fp32
    assert topk_ref.Ranking(q, t).boundary_ties(8).mean() > 0.25                    # such data ties at the selection boundary
