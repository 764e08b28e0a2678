"""Helpers of the link-prediction tests: a NumPy restatement of the two edge samplers of csrc/cb_linkp.hip on the host restatement of
Philox4x32-10 (oracle/coldbrew_oracle.py), and a float64 restatement of the reference's loss / MRR / gradient (utils.py:754-791).  The
samplers are pure functions of (graph, mask, mode, seed, slot, try), so the device output is compared bit for bit.  No GPU is needed to
import this module.

Draw number d = slot * MAX_TRIES + try; words r0..r3 = philox(counter = (lo32(d), hi32(d), C2, C3), key = (lo32(seed), hi32(seed)));
first integer = hi64((r0 << 32 | r1) * n), second = hi64((r2 << 32 | r3) * n)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, 'golden'), os.path.join(os.path.dirname(HERE), 'oracle')):
    if p not in sys.path:
        sys.path.insert(0, p)
import coldbrew_oracle as orc  # noqa: E402

MAX_TRIES = 64
MODES = ('train', 'test')
EPS24 = 2.0 ** -24
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def mulhi64(x, n):
    """hi64(x * n) for uint64 x and n < 2^32, without leaving uint64."""
    x = np.asarray(x, dtype=np.uint64)
    n = np.uint64(n)
    assert int(n) < 2 ** 32
    return ((x >> _S32) * n + (((x & _M32) * n) >> _S32)) >> _S32


def draw2(seed, ctr, n):
    """The two integers of [0, n) of the draws `ctr` (uint64 array) under the 64-bit seed."""
    s = int(seed) % (1 << 64)
    c = np.asarray(ctr, dtype=np.uint64)
    w = orc.philox4x32_10(c & _M32, c >> _S32, orc.DROPOUT_C2, orc.DROPOUT_C3, s & 0xFFFFFFFF, s >> 32).astype(np.uint64)
    return mulhi64((w[..., 0] << _S32) | w[..., 1], n).astype(np.int64), mulhi64((w[..., 2] << _S32) | w[..., 3], n).astype(np.int64)


def csr(edge_index, n):
    """The by-dst CSR of the package's ingest: row v lists the sources of the edges u -> v, ascending, duplicates kept."""
    ei = np.asarray(edge_index, dtype=np.int64)
    order = np.lexsort((ei[0], ei[1]))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei[1], minlength=n), out=rowptr[1:])
    return rowptr, ei[0][order]


def node_ok(mask, mode):
    mask = np.asarray(mask, dtype=bool)
    return mask if mode == 'train' else ~mask


def valid_edges(edge_index, n, mask, mode):
    """(src, dst) of the valid edges of `mode` in CSR order: the k-th of them is what draw k picks."""
    rowptr, col = csr(edge_index, n)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    ok = node_ok(mask, mode)
    keep = ok[row] & ok[col]
    return col[keep], row[keep]


def positives(edge_index, n, mask, mode, P, seed):
    src, dst = valid_edges(edge_index, n, mask, mode)
    V = len(src)
    if V == 0:
        raise ValueError('no valid edge')
    k, _ = draw2(seed, np.arange(P, dtype=np.uint64) * np.uint64(MAX_TRIES), V)
    return np.stack([src[k], dst[k]]).astype(np.int32), k


def negatives(edge_index, n, mask, mode, Nn, seed):
    """int32 [2, Nn] (Nn even) and the number of failed slots."""
    assert Nn % 2 == 0
    mask = np.asarray(mask, dtype=bool)
    ei = np.asarray(edge_index, dtype=np.int64)
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    train_nodes = np.nonzero(mask)[0]
    slots = Nn // 2
    m = len(train_nodes) if mode == 'train' else n
    ctr = (np.arange(slots, dtype=np.uint64) * np.uint64(MAX_TRIES))[:, None] + np.arange(MAX_TRIES, dtype=np.uint64)[None, :]
    a, b = draw2(seed, ctr, m)
    out = np.full((2, Nn), -1, dtype=np.int32)
    failed = 0
    for s in range(slots):
        for t in range(MAX_TRIES):
            u, v = int(a[s, t]), int(b[s, t])
            if mode == 'train':
                u, v = int(train_nodes[u]), int(train_nodes[v])
            elif mask[u] and mask[v]:
                continue
            if u == v or (u, v) in edges or (v, u) in edges:
                continue
            out[:, 2 * s] = (u, v)
            out[:, 2 * s + 1] = (v, u)
            break
        else:
            failed += 1
    return out, failed


# ---- loss / MRR / gradient in float64 -------------------------------------------------------------------------------------------------
def scores64(emb, pairs):
    e = emb.double()
    return (e[pairs[0].long()] * e[pairs[1].long()]).sum(-1)


def mrr_exact(pos_score, neg_score):
    """cal_MRR with ties counting for the positive, as a float64 mean of 1 / rank."""
    P, Nn = len(pos_score), len(neg_score)
    k = Nn // P
    grp = neg_score[:k * P].reshape(P, k)
    rank = 1 + (grp > pos_score.reshape(P, 1)).sum(1)
    return float((1.0 / rank.double()).mean()), rank


def loss_mrr_grad64(emb, pos, neg):
    """(loss, mrr, d loss / d emb [N, D], scores [P + Nn]) of utils.linkp_loss_eva on emb[pos[0]], emb[pos[1]], emb[neg[0]], emb[neg[1]], all
    float64, the loss in torch's stable form max(s, 0) - s y + log1p(exp(-|s|))."""
    e = emb.detach().double().clone().requires_grad_(True)
    ps = (e[pos[0].long()] * e[pos[1].long()]).sum(-1)
    ns = (e[neg[0].long()] * e[neg[1].long()]).sum(-1)
    s = torch.cat([ps, ns])
    y = torch.cat([torch.ones_like(ps), torch.zeros_like(ns)])
    loss = (s.clamp(min=0) - s * y + torch.log1p(torch.exp(-s.abs()))).mean()
    (g,) = torch.autograd.grad(loss, e)
    mrr, _ = mrr_exact(ps.detach(), ns.detach())
    return float(loss.detach()), mrr, g, s.detach()


def abs_dot(emb, pairs):
    """sum_i |h_i t_i| per pair in float64: the magnitude the rounding bounds are stated in."""
    e = emb.double().abs()
    return (e[pairs[0].long()] * e[pairs[1].long()]).sum(-1)


def gamma(n):
    return n * EPS24 / (1 - n * EPS24)


def golden_graph(name):
    g = torch.load(os.path.join(HERE, 'golden', name + '.pt'), weights_only=False)
    return g['edge_index'], int(g['x'].shape[0]), g['train_mask']


def golden_cases():
    return sorted(f[:-3] for f in os.listdir(os.path.join(HERE, 'golden')) if f.startswith('linkp_') and f.endswith('.pt'))


def load_case(name):
    return torch.load(os.path.join(HERE, 'golden', name + '.pt'), weights_only=False)
