"""Helpers of the CN / AA and Hits@K / AUC tests: a dense float64 restatement of the reference's `CN` / `AA`
(Link_prediction_baseline/heuristics.py:107-129), brute-force rank counts, the purpose-built `heur_rows` graph, and the loader of the fixtures
tests/golden/heur_*.pt that tools/gen_heur_golden.py recorded from the unmodified reference functions.  Needs neither scipy nor a GPU.

    A[s, k] = multiplicity of the edge s -> k;  CN(s, d) = sum_k A[s, k] A[d, k];  AA(s, d) = sum_k A[s, k] A[d, k] w_k,
    w_k = 1 / log(c_k) with c_k the column sum of A, 0 where c_k <= 1."""
import os
from fractions import Fraction

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
U24 = 2.0 ** -24
AA_REL_BOUND = U24 * (1.0 + 2.0 ** -16)      # one fp32 rounding; the float64 summation order, log and division: n * 2^-53 with n far below 2^37
ROW_LENGTHS = (0, 1, 63, 64, 65, 130, 200)   # out-row lengths of nodes 0..6 of `heur_rows`


def dense_adjacency(edge_index, n):
    ei = np.asarray(edge_index, dtype=np.int64)
    A = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (ei[0], ei[1]), 1.0)
    return A


def aa_weights(A):
    c = A.sum(axis=0)
    w = np.zeros_like(c)
    w[c > 1] = 1.0 / np.log(c[c > 1])
    return w


def cn64(A, pairs):
    p = np.asarray(pairs, dtype=np.int64)
    return (A[p[0]] * A[p[1]]).sum(axis=1)


def weighted64(A, pairs, w):
    p = np.asarray(pairs, dtype=np.int64)
    return (A[p[0]] * A[p[1]] * w[None, :]).sum(axis=1)


def aa64(A, pairs):
    return weighted64(A, pairs, aa_weights(A))


def within_aa_bound(score, r):
    """|score - r| <= 2^-24 r (1 + 2^-16), element-wise (r >= 0)."""
    score, r = np.asarray(score, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return np.abs(score - r) <= AA_REL_BOUND * r


def rank_counts_brute(pos, neg):
    """gt[i] = #{j: neg[j] > pos[i]}, eq[i] = #{j: neg[j] == pos[i]} by comparing every pair in float64 (-0.0 == +0.0, infinities compare as numbers)."""
    p, q = np.asarray(pos, dtype=np.float64).reshape(-1, 1), np.asarray(neg, dtype=np.float64).reshape(1, -1)
    return (q > p).sum(axis=1).astype(np.int64), (q == p).sum(axis=1).astype(np.int64)


def hits_brute(pos, neg, k):
    """OGB's rule: a positive is a hit if it lies strictly above the K-th largest negative; with fewer than K negatives every positive is one."""
    neg = np.sort(np.asarray(neg, dtype=np.float64))[::-1]
    if len(neg) < k:
        return 1.0
    return float((np.asarray(pos, dtype=np.float64) > neg[k - 1]).mean())


def auc_brute(pos, neg):
    """P(pos > neg) + P(pos == neg) / 2 over all pairs, as an exactly rounded float."""
    gt, eq = rank_counts_brute(pos, neg)
    P, Nn = len(gt), np.asarray(neg).size
    wins2 = sum(2 * (Nn - int(g) - int(e)) + int(e) for g, e in zip(gt, eq))
    return float(Fraction(wins2, 2 * P * Nn))


def heur_rows_graph():
    """(edge_index int64 [2, E], N = 260).  Nodes 0..6 have out-rows of exactly ROW_LENGTHS entries.  Rows 5 (130) and 6 (200) share the 45 columns
    10..54, column 10 + i stored 1 + i % 3 times in row 5 and 1 + (i // 3) % 3 times in row 6 (every combination of 1..3 on either side); rows 3 and 5
    hold a self loop; node 250 has in-degree 1 (from node 1 alone); nodes 251..259 have in-degree 0."""
    n = 260
    rng = np.random.default_rng(20251019)
    src, dst = [], []

    def add(s, cols):
        src.extend([s] * len(cols))
        dst.extend(int(c) for c in cols)
    add(1, [250])
    add(2, rng.choice(np.arange(7, 250), 63, replace=False))
    add(3, [3] + list(rng.choice(np.arange(7, 250), 63, replace=False)))
    add(4, rng.choice(np.arange(7, 250), 65, replace=False))
    for i in range(45):
        add(5, [10 + i] * (1 + i % 3))
        add(6, [10 + i] * (1 + (i // 3) % 3))
    add(5, [5] + list(range(60, 99)))
    add(6, list(range(100, 210)))
    for s in range(7, n):
        add(s, rng.integers(0, 250, 3))
    ei = np.stack([np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)])
    perm = rng.permutation(ei.shape[1])      # the edge list in no particular order
    return ei[:, perm], n


def heur_rows_pairs():
    """Every combination of the rows 0..6 in both orders, (s, s) included: 49 pairs."""
    return np.array([[s, d] for s in range(7) for d in range(7)], dtype=np.int64).T


def golden_cases():
    return sorted(f[:-3] for f in os.listdir(os.path.join(HERE, 'golden')) if f.startswith('heur_') and f.endswith('.pt'))


_CACHE = {}


def load_case(name):
    """{'edge_index' int64 [2, E], 'N', 'pairs' int64 [2, P], 'cn' fp32 [P], 'aa' fp32 [P]} plus, computed once and shared, 'A' (dense float64),
    'cn64' and 'aa64' (the restatement)."""
    c = _CACHE.get(name)
    if c is None:
        c = torch.load(os.path.join(HERE, 'golden', name + '.pt'), weights_only=False)
        c['A'] = dense_adjacency(c['edge_index'].numpy(), int(c['N']))
        c['cn64'] = cn64(c['A'], c['pairs'].numpy())
        c['aa64'] = aa64(c['A'], c['pairs'].numpy())
        _CACHE[name] = c
    return c
