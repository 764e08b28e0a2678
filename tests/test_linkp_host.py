"""Host-side checks (no GPU) of the link-prediction path: the C ABI of csrc/cb_linkp.hip is declared, exported and bound with matching
argument counts and refuses bad arguments before any launch; the NumPy restatement of the two samplers (tests/linkp_ref.py) has the properties
the device samplers are then compared against bit for bit; the golden fixtures of the reference's utils.linkp_loss_eva / cal_MRR load and agree
with the float64 restatement of loss / MRR / gradient."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import linkp_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_linkp_max_tries', 'cb_linkp_valid_counts_i32', 'cb_linkp_positives_i32', 'cb_linkp_negatives_i32', 'cb_linkp_loss_fwd_f32',
               'cb_linkp_mrr_f32', 'cb_linkp_bwd_workspace_bytes', 'cb_linkp_loss_bwd_f32']
P8 = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: the checks below answer before any launch
GRAPHS = ['case_graph_powerlaw_d7_d64', 'case_graph_asym_multi']


def test_c_abi_of_the_linkp_kernels():
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
    assert {n for n in declared if 'linkp' in n} == set(NEW_ENTRIES)
    assert _lib.load().cb_linkp_max_tries() == lr.MAX_TRIES == int(re.search(r'#define CB_LINKP_MAX_TRIES (\d+)', hdr).group(1))


def test_bad_arguments_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()

    def view(**over):
        f = dict(rowptr=P8, col=P8, col_flags=0, n_rows=4, n_edges=4, hub_threshold=1, n_hubs=0, n_chunks=0, hub_rows=None, hub_chunk_ptr=None, ws=None,
                 ws_bytes=0)
        f.update(over)
        return ctypes.byref(_lib.CsrView(**f))
    assert lib.cb_linkp_valid_counts_i32(None, P8, 0, P8, None) == -1
    assert lib.cb_linkp_valid_counts_i32(view(col_flags=1), P8, 0, P8, None) == -1 and b'flags' in lib.cb_last_error()
    assert lib.cb_linkp_valid_counts_i32(view(n_rows=2 ** 31), P8, 0, P8, None) == -2
    assert lib.cb_linkp_valid_counts_i32(view(), P8, 2, P8, None) == -1 and b'mode' in lib.cb_last_error()
    assert lib.cb_linkp_valid_counts_i32(view(), None, 0, P8, None) == -1 and b'null' in lib.cb_last_error()
    assert lib.cb_linkp_positives_i32(view(), P8, 0, P8, 0, 3, 1, None, P8, None) == -1      # n_valid == 0
    assert lib.cb_linkp_positives_i32(view(), P8, 0, P8, 5, 3, 1, None, P8, None) == -1      # n_valid > n_edges
    assert lib.cb_linkp_positives_i32(view(), P8, 0, None, 4, 3, 1, None, P8, None) == -1
    assert lib.cb_linkp_positives_i32(view(), P8, 0, P8, 4, 0, 1, None, None, None) == 0     # nothing to draw
    assert lib.cb_linkp_negatives_i32(view(), P8, 0, P8, 2, 3, 1, None, P8, P8, None) == -1 and b'even' in lib.cb_last_error()
    assert lib.cb_linkp_negatives_i32(view(), P8, 0, P8, 0, 4, 1, None, P8, P8, None) == -1   # train mode without train nodes
    assert lib.cb_linkp_negatives_i32(view(), P8, 0, P8, 5, 4, 1, None, P8, P8, None) == -1   # more train nodes than nodes
    assert lib.cb_linkp_negatives_i32(view(), P8, 1, None, 0, 4, 1, None, P8, None, None) == -1 and b'null' in lib.cb_last_error()
    assert lib.cb_linkp_negatives_i32(view(), P8, 1, None, 0, 0, 1, None, None, None, None) == 0
    fwd = [P8, 8, 10, 8, P8, 3, P8, 4, P8, P8, P8, P8, None]
    for at, val in ((1, 7), (2, 0), (3, 0), (5, 0), (7, -1), (4, None), (6, None), (11, None)):      # ld < D, N, D, P, Nn, pos, neg, status
        bad = list(fwd)
        bad[at] = val
        assert lib.cb_linkp_loss_fwd_f32(*bad) == -1, (at, val)
    bad = list(fwd)
    bad[5] = 2 ** 30
    assert lib.cb_linkp_loss_fwd_f32(*bad) == -2
    assert lib.cb_linkp_mrr_f32(P8, 0, P8, 4, P8, None) == -1
    assert lib.cb_linkp_mrr_f32(P8, 3, None, 4, P8, None) == -1
    assert lib.cb_linkp_bwd_workspace_bytes(0, 0) == 0
    need = lib.cb_linkp_bwd_workspace_bytes(3, 4)
    assert need >= 2 * 14 * 8
    bwd = [P8, 8, 10, 8, P8, 3, P8, 4, P8, P8, P8, 8]
    assert lib.cb_linkp_loss_bwd_f32(*bwd, None, 0, None) == -3 and b'workspace' in lib.cb_last_error()
    assert lib.cb_linkp_loss_bwd_f32(*bwd, P8, need - 1, None) == -3
    bad = list(bwd)
    bad[11] = 7                                                                              # ldd < D
    assert lib.cb_linkp_loss_bwd_f32(*bad, P8, need, None) == -1
    bad = list(bwd)
    bad[9] = None                                                                            # g
    assert lib.cb_linkp_loss_bwd_f32(*bad, P8, need, None) == -1


def test_the_operators_refuse_what_they_document():
    from gnn_tail_generalization_amd import _lib, ops, utils
    emb = torch.zeros(4, 8)
    pairs = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(_lib.HipExtensionError):                                              # no CPU fallback
        ops.linkp_loss_eva(emb, pairs, pairs)
    with pytest.raises(_lib.HipExtensionError):
        ops.cal_MRR(torch.zeros(3), torch.zeros(6))
    with pytest.raises(_lib.HipExtensionError):
        utils.linkp_loss_eva(emb[:2], emb[:2], emb, emb)
    with pytest.raises(ValueError, match='whole square'):
        ops.LinkSampler(object(), torch.zeros(4, dtype=torch.bool))


def test_mulhi_and_draws_are_exact():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2 ** 64, 2000, dtype=np.uint64)
    for n in (1, 2, 3, 200, 2 ** 31 - 1, 2 ** 31 + 12345):
        assert [int(v) for v in lr.mulhi64(x, n)] == [(int(v) * n) >> 64 for v in x]
    a, b = lr.draw2(2 ** 40 + 7, np.arange(5000, dtype=np.uint64) * np.uint64(lr.MAX_TRIES), 10)
    assert a.min() == 0 and a.max() == 9 and b.min() == 0 and b.max() == 9
    a2, _ = lr.draw2(2 ** 40 + 8, np.arange(5000, dtype=np.uint64) * np.uint64(lr.MAX_TRIES), 10)
    assert (a != a2).mean() > 0.8                                                            # another seed, another stream


@pytest.mark.parametrize('name', GRAPHS)
@pytest.mark.parametrize('mode', lr.MODES)
def test_sampler_restatement_properties(name, mode):
    ei, n, mask = lr.golden_graph(name)
    ei_np, m = ei.numpy(), mask.numpy()
    edges = set(zip(ei_np[0].tolist(), ei_np[1].tolist()))
    ok = lr.node_ok(m, mode)
    # the valid edges are the reference's valid_edge_index (:512-517) as a multiset
    ref_valid = ei[:, (mask[ei[0]] & mask[ei[1]]) if mode == 'train' else (~mask[ei[0]] & ~mask[ei[1]])]
    src, dst = lr.valid_edges(ei_np, n, m, mode)
    assert sorted(zip(src.tolist(), dst.tolist())) == sorted(zip(ref_valid[0].tolist(), ref_valid[1].tolist()))
    pos, k = lr.positives(ei_np, n, m, mode, 500, seed=2 ** 33 + 11)
    assert pos.dtype == np.int32 and pos.shape == (2, 500) and 0 <= k.min() and k.max() < len(src)
    for u, v in pos.T.tolist():
        assert (u, v) in edges and ok[u] and ok[v]
    neg, failed = lr.negatives(ei_np, n, m, mode, 400, seed=2 ** 35 + 3)
    assert failed == 0 and neg.min() >= 0
    assert np.array_equal(neg[:, 0::2], neg[::-1, 1::2])                                     # mirrored pairs
    for u, v in neg.T.tolist():
        assert u != v and (u, v) not in edges and (v, u) not in edges
        assert (m[u] and m[v]) if mode == 'train' else not (m[u] and m[v])
    again, _ = lr.negatives(ei_np, n, m, mode, 400, seed=2 ** 35 + 3)
    assert np.array_equal(neg, again)


def _chernoff_interval(mu, delta):
    """[lo, hi] with P(X < lo) + P(X > hi) <= delta for a sum X of independent indicators with mean mu (the multiplicative Chernoff bounds
    P(X <= (1 - d) mu) <= exp(-d^2 mu / 2) and P(X >= (1 + d) mu) <= exp(-d^2 mu / (2 + d)), each solved for d at delta / 2)."""
    L = math.log(2.0 / delta)
    d_lo = math.sqrt(2.0 * L / mu)
    d_hi = (L + math.sqrt(L * L + 8.0 * L * mu)) / (2.0 * mu)
    return max(0.0, (1.0 - d_lo) * mu), (1.0 + d_hi) * mu


def test_positive_draws_cover_every_valid_edge_in_proportion_to_its_multiplicity():
    """20 000 draws over the valid edges of one mode of the asymmetric multigraph (about 200): every valid position is drawn (a given one of V is
    missed with probability (1 - 1/V)^20000 < e^-60), and a multi-edge is drawn in proportion to its multiplicity: the count of an edge stored m
    times is Binomial(n, m / V) and must lie in the Chernoff interval of its mean at delta = 1e-9; so must the total over all multi-edges, whose
    larger mean makes the interval narrow in relative terms.  The seed is fixed: the intervals are statements about the generator, no tuned
    constants."""
    ei, n, mask = lr.golden_graph('case_graph_asym_multi')
    mode = min(lr.MODES, key=lambda m_: abs(len(lr.valid_edges(ei.numpy(), n, mask.numpy(), m_)[0]) - 200))
    src, dst = lr.valid_edges(ei.numpy(), n, mask.numpy(), mode)
    V = len(src)
    assert 100 <= V <= 300, V
    draws = 20000
    pos, k = lr.positives(ei.numpy(), n, mask.numpy(), mode, draws, seed=12345)
    assert len(np.unique(k)) == V                                                            # every valid position drawn at least once
    mult = {}
    for e in zip(src.tolist(), dst.tolist()):
        mult[e] = mult.get(e, 0) + 1
    assert max(mult.values()) >= 2, 'no multi-edge among the valid edges'
    got = {}
    for e in zip(pos[0].tolist(), pos[1].tolist()):
        got[e] = got.get(e, 0) + 1
    assert set(got) == set(mult)
    for e, m_ in mult.items():
        lo, hi = _chernoff_interval(draws * m_ / V, 1e-9)
        assert lo <= got[e] <= hi, (e, m_, got[e], lo, hi)
    multi_positions = sum(m_ for m_ in mult.values() if m_ >= 2)
    lo, hi = _chernoff_interval(draws * multi_positions / V, 1e-9)
    total = sum(got[e] for e, m_ in mult.items() if m_ >= 2)
    print(f'V {V} mode {mode}: multi-edges hold {multi_positions} positions, drawn {total} times, interval [{lo:.0f}, {hi:.0f}]')
    assert lo <= total <= hi
    # what the distinct multi-edges would collect if multiplicity were ignored lies outside the interval: the check can tell the two apart
    assert draws * sum(1 for m_ in mult.values() if m_ >= 2) / len(mult) < lo


@pytest.mark.parametrize('name', lr.golden_cases())
def test_golden_fixtures_agree_with_the_float64_restatement(name):
    c = lr.load_case(name)
    emb, pos, neg = c['emb'], c['pos'], c['neg']
    P, Nn = pos.shape[1], neg.shape[1]
    loss, mrr, grad, s = lr.loss_mrr_grad64(emb, pos, neg)
    assert mrr == pytest.approx(c['mrr'], abs=1e-12)
    # the reference evaluates in float32 on the CPU: each score within gamma_D sum|h t|, the loss is 1-Lipschitz in every score / (P + Nn)
    ad = torch.cat([lr.abs_dot(emb, pos), lr.abs_dot(emb, neg)])
    D = emb.shape[1]
    bound = float(lr.gamma(D) * ad.mean()) + 8 * lr.EPS24 * abs(loss)
    assert abs(float(c['loss']) - loss) <= bound, (float(c['loss']), loss, bound)
    assert torch.allclose(c['grad'].double(), grad, rtol=1e-4, atol=1e-7)
    touched = torch.zeros(emb.shape[0], dtype=torch.bool)
    touched[pos.reshape(-1)] = True
    touched[neg.reshape(-1)] = True
    assert bool((grad[~touched] == 0).all()) and bool((c['grad'][~touched] == 0).all())


def test_golden_cases_are_the_ones_the_issue_names():
    shapes = {n: (lr.load_case(n)['emb'].shape[0], lr.load_case(n)['emb'].shape[1], lr.load_case(n)['pos'].shape[1], lr.load_case(n)['neg'].shape[1])
              for n in lr.golden_cases()}
    assert shapes['linkp_n50_d10_p7_n30'] == (50, 10, 7, 30) and shapes['linkp_n50_d7_p5_n3_k0'] == (50, 7, 5, 3)
    assert shapes['linkp_n300_d256_p64_n1280'] == (300, 256, 64, 1280)
    assert lr.load_case('linkp_n50_d7_p5_n3_k0')['mrr'] == 1.0
    hub = lr.load_case('linkp_hub_selfloop')
    assert int((hub['pos'] == 0).sum() + (hub['neg'] == 0).sum()) >= 100 and bool((hub['pos'][0] == hub['pos'][1]).any())
