"""Inputs and host summands shared by the column-sum order tests (tests/test_colsum_host.py on the CPU, tests/test_gpu_colsum_order.py on the device).

Every entry that returns column sums adds, per column, one float32 summand per row; the ORDER of those additions is what the tests pin
(oracle/coldbrew_oracle.py colsum_two_stage).  So the summands themselves must not depend on how the kernel forms them: gradients are random normal
float32, mask words random, every factor a power of two and p in {0, 0.5} (keep scale 1 or 2) — every product is exact and a summand holds at most
one rounded addition of two exact products, the same with or without FMA contraction.  The device seed word is absent.

A case is built once (lru_cache) on the CPU and never changed; the GPU test copies the operands to the device."""
import functools

import numpy as np
import torch

import coldbrew_oracle as orc

C_ACT, C_MIX, C2, CS_C = 0.5, 0.25, 0.125, 0.5
ROW0 = 3                                       # global row of local row 0: the masks are not the ones of an unsharded matrix
PS = (0.0, 0.5)
# rows: fewer rows than wavefronts (1, 3), one more than wavefronts (5), one full slab (64), a slab boundary (65 -> blocks of 33 and 32 rows),
# ragged slabs (1037 -> 17 blocks of 61); d = 512: a second tile pass reusing the LDS buffer; 16449 rows -> 258 partials: the finish kernel's second trip
ROW_SHAPES = [(r, d) for r in (1, 3, 5, 64, 65, 1037) for d in (256, 512)] + [(16449, 256)]
# cb_act_bwd_f32: d = 7 scalar path, 128 row lanes; d = 40: 25 row lanes and 6 idle threads; d = 256: 4 row lanes
ACT_SHAPES = [(r, d) for d in (7, 40, 256) for r in (5, 65, 1037)]
# (rows, d, p): both p at every small shape; the 16449-row case is there for the finish kernel, which sees partials and no mask: p = 0 only (drawing
# up to eight host masks of that size would take the case over a second)
ROW_CASES = [(r, d, p) for r, d in ROW_SHAPES for p in PS if p == 0 or r < 16449]
ENTRIES = ('layer', 'layer_rows', 'fold', 'input', 'multi')


def act_row_lanes(d):
    return 256 // min(64, -(-d // 4))


def _gen(*key):
    s = 0
    for k in key:
        s = s * 1000003 + int(k)
    return torch.Generator().manual_seed(s)


def _words(gen, rows, d):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (rows, d // 256, 4), dtype=torch.int64, generator=gen)


def word_bits(w):
    """int64 mask words [rows, t, 4] -> bool [rows, 256 t]: word k of tile j, bit l <-> column 256 j + 4 l + k."""
    u = w.numpy().view(np.uint64)
    b = (u[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return b.transpose(0, 1, 3, 2).reshape(w.shape[0], -1).astype(bool)


def keep_factor(n_rows, d, p, seed):
    """float32 [n_rows, d]: keep ? 1 / (1 - p) : 0 of the host mask of the matrix whose row 0 is global row ROW0."""
    if p == 0:
        return np.ones((n_rows, d), dtype=np.float32)
    return orc.dropout_keep_mask((n_rows, d), p, seed, offset=ROW0 * d).astype(np.float32) * orc.dropout_scale(p)


def _compact(gen, n, d, frac=0.4):
    """A compact operand: (its rows [m, d], int32 positions [n] with -1 where the row is absent, the operand scattered to [n, d])."""
    member = torch.rand(n, generator=gen) < frac
    member[0] = True
    pos = torch.where(member, torch.cumsum(member, 0, dtype=torch.int32) - 1, torch.full((n,), -1, dtype=torch.int32)).contiguous()
    rows = torch.randn(int(member.sum()), d, generator=gen)
    full = np.zeros((n, d), dtype=np.float32)
    full[member.numpy()] = rows.numpy()
    return rows, pos, full


def _f32(*factors):
    out = np.float32(1)
    for f in factors:
        out = out * np.asarray(f, dtype=np.float32)
    return out


@functools.lru_cache(maxsize=None)
def make(entry, rows, d, p):
    """dict of the CPU operands of a case (torch tensors) and its host summands (numpy float32 [rows, d]; 'sum*' keys)."""
    gen = _gen(ENTRIES.index(entry), rows, d, int(p * 2))
    seed, seed2 = 0x1234ABCD5 + rows, 2 ** 40 + 12345 + d
    c = {'seed': seed, 'seed2': seed2}
    zero = np.float32(0)
    if entry == 'layer':
        # cb_trunk_layer_bwd_f32: gy = bit ? c_act * dropout_bwd(g) [+ c2 * dropout_bwd_seed2(g2)] : 0
        c['g'], c['g2'], c['bits'] = torch.randn(rows, d, generator=gen), torch.randn(rows, d, generator=gen), _words(gen, rows, d)
        c['g2c'], c['g2_pos'], g2c_full = _compact(gen, rows, d)
        bit, k1, k2 = word_bits(c['bits']), keep_factor(rows, d, p, seed), keep_factor(rows, d, p, seed2)
        first = _f32(C_ACT, c['g'].numpy(), k1)
        c['gx0'] = _f32(C_MIX, c['g'].numpy(), k1)
        c['sum_none'] = np.where(bit, first, zero)
        c['sum_dense'] = np.where(bit, first + _f32(C2, c['g2'].numpy(), k2), zero)
        c['sum_compact'] = np.where(bit, first + _f32(C2, g2c_full, k2), zero)
    elif entry == 'layer_rows':
        # cb_trunk_layer_bwd_rows_f32: the same on the compact rows idx of n nodes, everything but g / out taken at the node row
        n = 2 * rows + 3
        c['n'] = n
        idx = torch.sort(torch.randperm(n, generator=gen)[:rows])[0].contiguous()
        c['idx'], c['g'], c['bits'] = idx, torch.randn(rows, d, generator=gen), _words(gen, n, d)
        c['g2c'], c['g2_pos'], g2c_full = _compact(gen, n, d, frac=0.5)
        i = idx.numpy()
        bit, k1, k2 = word_bits(c['bits'])[i], keep_factor(n, d, p, seed)[i], keep_factor(n, d, p, seed2)[i]
        c['sum'] = np.where(bit, _f32(C_ACT, c['g'].numpy(), k1) + _f32(C2, g2c_full[i], k2), zero)
    elif entry == 'fold':
        # cb_trunk_layer_bwd_fold_f32: the layer sum, and the second sum cs_c * dropout_bwd(mix_g[1]) through other mask words
        c['g'], c['bits'], c['cs_bits'] = torch.randn(rows, d, generator=gen), _words(gen, rows, d), _words(gen, rows, d)
        c['dense'] = torch.randn(rows, d, generator=gen)
        c['comp'], c['pos'], comp_full = _compact(gen, rows, d)
        c['seeds'] = [seed2, seed + 7]
        gm = _f32(c['g'].numpy(), keep_factor(rows, d, p, seed))
        u0, u1 = _f32(c['dense'].numpy(), keep_factor(rows, d, p, seed2)), _f32(comp_full, keep_factor(rows, d, p, seed + 7))
        c['sum'] = np.where(word_bits(c['bits']), _f32(C_ACT, gm), zero)
        c['sum2'] = np.where(word_bits(c['cs_bits']), _f32(CS_C, u1), zero)
        c['m'] = (_f32(C_MIX, u0) + _f32(C_MIX, u1)) + _f32(C_MIX, gm)
    elif entry == 'input':
        # cb_trunk_input_bwd_f32: gy = (add + dropout_bwd(g)) * (act > 0)
        c['g'], c['add'], c['act'] = (torch.randn(rows, d, generator=gen) for _ in range(3))
        c['sum'] = np.where(c['act'].numpy() > 0, c['add'].numpy() + _f32(c['g'].numpy(), keep_factor(rows, d, p, seed)), zero)
    elif entry == 'multi':
        # cb_trunk_input_bwd_multi_cs_f32: gy = (((dropout_bwd(g) + c_mix u_0) + c_mix u_1) + c_mix u_2) * act bit; extra sums of cs_c * u_1, cs_c * u_2
        c['g'], c['act_bits'] = torch.randn(rows, d, generator=gen), _words(gen, rows, d)
        c['d0'], c['d2'] = torch.randn(rows, d, generator=gen), torch.randn(rows, d, generator=gen)
        c['comp'], c['pos'], comp_full = _compact(gen, rows, d)
        c['cs_bits'] = [_words(gen, rows, d), _words(gen, rows, d)]
        c['seeds'] = [seed2, seed + 7, seed2 + 11]
        u = [_f32(t, keep_factor(rows, d, p, s)) for t, s in zip((c['d0'].numpy(), comp_full, c['d2'].numpy()), c['seeds'])]
        t = _f32(c['g'].numpy(), keep_factor(rows, d, p, seed))
        for ul in u:
            t = t + _f32(C_MIX, ul)
        c['sum'] = np.where(word_bits(c['act_bits']), t, zero)
        c['sum2'] = [np.where(word_bits(c['cs_bits'][q]), _f32(CS_C, u[q + 1]), zero) for q in range(2)]
    else:
        raise KeyError(entry)
    return c


@functools.lru_cache(maxsize=None)
def make_act(rows, d):
    """cb_act_bwd_f32: gm = g * (act > 0)."""
    gen = _gen(99, rows, d)
    g, act = torch.randn(rows, d, generator=gen), torch.randn(rows, d, generator=gen)
    return {'g': g, 'act': act, 'sum': np.where(act.numpy() > 0, g.numpy(), np.float32(0))}


def summands(entry, rows, d, p):
    """Every (name, summands) pair of a case."""
    out = []
    for k, v in make(entry, rows, d, p).items():
        if k.startswith('sum'):
            out += [(f'{k}[{q}]', s) for q, s in enumerate(v)] if isinstance(v, list) else [(k, v)]
    return out
