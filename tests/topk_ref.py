"""Host reference of the top-K replacement (cb_topk_replace_f32, `SEMLP.replacement`) in float64, with the tie order
include/coldbrew_hip.h promises: larger score first, then larger index — a STABLE ascending argsort followed by [-K:].
`coldbrew_oracle.semlp_replacement` sorts with torch's default (unstable) argsort and so cannot judge ties; this can.

Everything here is numpy on the host.  `replacement` is the whole operation; `Ranking` sorts the score matrix once and keeps
the last `keep` places of every query, so that tests which run several K on the same inputs sort once and hold little."""
import numpy as np

KEEP = 9      # the kernel's largest K, plus the runner-up that decides whether the selection was a close call


def scores_f64(q, t):
    """[B, N] float64 scores <q_i, t_j>.  Integer-valued inputs give exact scores (every partial sum is an integer < 2^53)."""
    return np.asarray(q, dtype=np.float64) @ np.asarray(t, dtype=np.float64).T


class Ranking:
    """The float64 scores of q against t, ranked once (stable, ascending); the last min(keep, N) places are kept."""

    def __init__(self, q, t, keep=KEEP):
        self.t = np.asarray(t, dtype=np.float64)
        s = scores_f64(q, t)
        self.n = s.shape[1]
        self.order = np.ascontiguousarray(np.argsort(s, axis=1, kind='stable')[:, -keep:])      # [B, kept] indices, ascending score
        self.values = np.take_along_axis(s, self.order, axis=1)                                  # [B, kept] their scores

    def select(self, k):
        """(out [B,D] f64, idx [B,k] int64 in ascending score order, wgt [B,k] f64): the k last of the stable ascending order,
        softmax over their scores, weighted sum of the selected teacher rows."""
        assert 1 <= k <= self.order.shape[1]
        idx, v = self.order[:, -k:], self.values[:, -k:]
        e = np.exp(v - v.max(axis=1, keepdims=True))
        wgt = e / e.sum(axis=1, keepdims=True)
        out = np.einsum('bk,bkd->bd', wgt, self.t[idx])
        return out, idx.astype(np.int64), wgt

    def top_values(self, k):
        """[B, k] float64: the k largest scores of every query, ascending."""
        assert 1 <= k <= self.order.shape[1]
        return self.values[:, -k:]

    def boundary_ties(self, k):
        """[B] bool: the K-th and the (K+1)-th best score are equal, i.e. only the index rule decides the selection."""
        if self.n <= k:
            return np.zeros(self.order.shape[0], dtype=bool)
        v = self.top_values(k + 1)
        return v[:, 0] == v[:, 1]

    def min_gap(self, k):
        """[B] float64: the smallest difference between consecutive scores among the top k+1 (top k when N == k)."""
        v = self.top_values(min(k + 1, self.n))
        if v.shape[1] < 2:
            return np.full(v.shape[0], np.inf)
        return np.diff(v, axis=1).min(axis=1)


def replacement(q, t, k):
    return Ranking(q, t, keep=k).select(k)
