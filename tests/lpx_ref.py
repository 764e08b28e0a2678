"""Helpers of the link-prediction experiment's tests: NumPy / float64 restatements of what csrc/cb_lpx.hip computes.  The three negative samplers and
the seeded permutation stand on tests/linkp_ref.py's `draw2` and the host Philox4x32-10 of oracle/coldbrew_oracle.py, so the device output is compared
bit for bit; the row ranks are brute force; the MRR is the OGB evaluator's rule (rank = the mean of the optimistic and the pessimistic rank); `cal_recall`
(utils.py:568-586) is a stable descending sort of [positives above 0 | negatives], which is what the reference's `sorted(..., reverse=True)` of its
concatenation does.  No GPU is needed to import this module."""
import os

import numpy as np
import torch

import linkp_ref as lr

orc = lr.orc
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_TRIES = 64
GRAPHS = ['case_graph_powerlaw_d7_d64', 'case_graph_asym_multi']
RECALL_SIZES = [(1, 0), (3, 5), (8, 12), (40, 100)]
RECALL_TOPKS = [None, '0', '0.8', '1', '1.25', '7', '200']
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def golden_graph(name):
    g = torch.load(os.path.join(HERE, 'golden', name + '.pt'), weights_only=False)
    return g['edge_index'], int(g['x'].shape[0])


def load_golden():
    return torch.load(os.path.join(HERE, 'golden', 'lpx_reference.pt'), weights_only=False)


# ---- samplers ---------------------------------------------------------------------------------------------------------------------------
def neg_global(edge_index, n, S, seed):
    """int32 [2, S] and the number of failed slots: slot s, try t takes the two integers of draw s * 64 + t; accepted iff u != v and u -> v is no edge."""
    ei = np.asarray(edge_index, dtype=np.int64)
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    out = np.full((2, S), -1, dtype=np.int32)
    if S == 0:
        return out, 0
    ctr = (np.arange(S, dtype=np.uint64) * np.uint64(MAX_TRIES))[:, None] + np.arange(MAX_TRIES, dtype=np.uint64)[None, :]
    a, b = lr.draw2(seed, ctr, n)
    failed = 0
    for s in range(S):
        for t in range(MAX_TRIES):
            u, v = int(a[s, t]), int(b[s, t])
            if u == v or (u, v) in edges:
                continue
            out[:, s] = (u, v)
            break
        else:
            failed += 1
    return out, failed


def neg_local(pos, n, k, seed):
    """int32 [2, P k]: the source of positive s // k and the first integer of draw s * 64."""
    pos = np.asarray(pos)
    S = pos.shape[1] * k
    slot = np.arange(S, dtype=np.uint64)
    a, _ = lr.draw2(seed, slot * np.uint64(MAX_TRIES), n)
    return np.stack([pos[0][np.arange(S) // max(k, 1)].astype(np.int32), a.astype(np.int32)]) if S else np.zeros((2, 0), dtype=np.int32)


def permutation(n, seed):
    """int32 [n]: the low words of the sorted keys (r0(draw i) << 32) | i."""
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    s = int(seed) % (1 << 64)
    i = np.arange(n, dtype=np.uint64)
    w = orc.philox4x32_10(i & _M32, i >> _S32, orc.DROPOUT_C2, orc.DROPOUT_C3, s & 0xFFFFFFFF, s >> 32).astype(np.uint64)
    keys = (w[..., 0] << _S32) | i
    assert len(np.unique(keys)) == n
    return (np.sort(keys) & _M32).astype(np.int32)


def neg_global_perm(edge_index, n, num_samples, k, seed):
    """Copy 0 = neg_global(num_samples, seed); copy j >= 1 = copy 0 permuted by permutation(num_samples, seed + j); column i k + j = base[perm_j[i]]."""
    base, failed = neg_global(edge_index, n, num_samples, seed)
    cols = [np.arange(num_samples)] + [permutation(num_samples, int(seed) + j).astype(np.int64) for j in range(1, k)]
    return base[:, np.stack(cols, axis=1).reshape(-1)], failed


# ---- ranks / MRR ------------------------------------------------------------------------------------------------------------------------
def row_ranks_brute(pos, neg2d):
    """(gt, eq, status): per row, the entries above and equal to the positive; a NaN in pos[i] or row i gives -1 / -1 and counts in status."""
    pos, neg2d = np.asarray(pos, dtype=np.float32), np.asarray(neg2d, dtype=np.float32)
    P, K = neg2d.shape
    gt, eq, status = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32), 0
    for i in range(P):
        nans = int(np.isnan(pos[i])) + int(np.isnan(neg2d[i]).sum())
        if nans:
            gt[i] = eq[i] = -1
            status += nans
            continue
        g = e = 0
        for j in range(K):
            g += int(neg2d[i, j] > pos[i])
            e += int(neg2d[i, j] == pos[i])
        gt[i], eq[i] = g, e
    return gt, eq, status


def mrr_ogb(gt, eq):
    """The OGB evaluator's MRR on counts, one float64 term after the other: rank = (optimistic + pessimistic) / 2 = 1 + gt + eq / 2."""
    rank = [0.5 * ((g + 1) + (g + e + 1)) for g, e in zip(np.asarray(gt).tolist(), np.asarray(eq).tolist())]
    out = {'MRR': float(np.mean([1.0 / r for r in rank]))}
    for k in (1, 3, 10):
        out[f'hits@{k}'] = float(np.mean([1.0 if r <= k else 0.0 for r in rank]))
    return out


# ---- cal_recall ---------------------------------------------------------------------------------------------------------------------------
def recall_parts(pos, neg, topk):
    """(numerator, P) of cal_recall as integers: the recall is numerator / P."""
    pos, neg = np.asarray(pos, dtype=np.float32).reshape(-1), np.asarray(neg, dtype=np.float32).reshape(-1)
    P = len(pos)
    if topk is None or float(topk) == 0:
        return int((pos > 0).sum()), P
    k = int(topk) if float(topk) > 5 else int(float(topk) * P)
    kept = pos[pos > 0]
    scores = np.concatenate([kept, neg]).astype(np.float64)
    labels = np.concatenate([np.ones(len(kept), dtype=np.int64), np.zeros(len(neg), dtype=np.int64)])
    if len(scores) == 0:
        raise ValueError('nothing to rank')
    order = np.argsort(-scores, kind='stable')      # descending, the concatenation's order among equals: positives first
    return int(labels[order][:k].sum()), P


def recall_threshold_form(pos, neg, k):
    """The same numerator from the k-th largest value t of M: #{pos > t} + min(#{pos == t}, k - #{M > t})."""
    pos, neg = np.asarray(pos, dtype=np.float32).reshape(-1), np.asarray(neg, dtype=np.float32).reshape(-1)
    kept = pos[pos > 0]
    M = np.concatenate([kept, neg])
    if k <= 0:
        return 0
    if k >= len(M):
        return len(kept)
    t = np.sort(M)[::-1][k - 1]
    return int((kept > t).sum() + min(int((kept == t).sum()), k - int((M > t).sum())))


def half_integer_scores(rng, n, lo, hi):
    """n float32 scores from the integer and half-integer grid of [lo, hi]."""
    return (rng.integers(int(2 * lo), int(2 * hi) + 1, n) / 2.0).astype(np.float32)
