"""The BIL / MLPDOT / MLPBIL / MLPCAT link predictors on the device (csrc/cb_pairpred.hip, ops.rows_linear / pair_bilinear / pair_scatter_rows,
Link_prediction_model/pair_predictor.py) against gemm.mm_nn on materialised operands, the float64 restatement of tests/pairpred_ref.py and the
recordings of the unmodified reference (tests/golden/pairpred_predictors.pt).  Bounds are derived, with u = 2^-24 the unit roundoff of fp32:
  rows GEMM   bit-equality with gemm.mm_nn / mm_nn_drop2 on the materialised A: the values are staged as they stand, the same K loop — no tolerance
  bilinear    the GEMM part as test_gpu_linkpred.py bounds the same core, 8 u scale with scale = sum_jk |W_jk h[u, k] h[v, j]|; the dot adds D u
              sum_j |z_j h[v, j]| (fewer than D additions per score: four per lane, a butterfly of at most five levels, the column blocks)
  scatter     a float64 sum rounded once: 2^-23 |r| + 2^-40 sum|terms|
  predictors  first order in u, every operation perturbs the monomials that pass through it by its own relative bound, so an entry errs by at most
              (the sum of the bounds of the operations on its longest path) x (the sum of the absolute values of its monomials, which
              pairpred_ref.predictor_abs64 computes by running the network on absolute values).  In units of u: a three-limb GEMM 8, the dot or
              the bilinear epilogue D, an elementwise product or sum 1, the scatter 2.  With G GEMMs in the forward (L Linear layers, + 1 for bilin)
              the forward's longest path is 8 G + D + 2 and a gradient's 16 G + 8 + D + 6 (the forward's GEMMs behind the activations it multiplies
              by, as many backward GEMMs, the weight gradient's own GEMM, the dot, the products with g and the scatter).  ReLU is 1-Lipschitz; a
              pre-activation within rounding of zero would flip a mask, which the analysis leaves out."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

import pairpred_ref as pr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
PLUMBING = ['--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1']


@pytest.fixture(scope='module')
def rec():
    return load_golden('pairpred_predictors')


@contextlib.contextmanager
def _tuned(**kw):
    from gnn_tail_generalization_amd import tuning
    keep = {k: getattr(tuning.T, k) for k in kw}
    for k, v in kw.items():
        setattr(tuning.T, k, v)
    try:
        yield
    finally:
        for k, v in keep.items():
            setattr(tuning.T, k, v)


def _status_ok():
    from gnn_tail_generalization_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().cb_device_status() == 0


def _operand(h, idx):
    return torch.cat([h[idx[s].long()] for s in range(idx.shape[0])], dim=1)


def _keep_scale(p):
    """1 / (1 - p) as the kernels form it: in fp32."""
    return float(1.0 / (1.0 - torch.tensor(p, dtype=torch.float32)))


def _module(kind, L, sd, dropout=0.5, width=16):
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    m = {'bil': lambda: pp.BilinearPairPredictor(16), 'mlpdot': lambda: pp.MLPDotPairPredictor(16, width, L, dropout),
         'mlpbil': lambda: pp.MLPBilPairPredictor(16, width, L, dropout), 'mlpcat': lambda: pp.MLPCatPairPredictor(16, width, 1, L, dropout)}[kind]().to(DEV)
    m.load_state_dict(sd)
    return m


def _units(kind, L, D=16):
    """(forward, gradient) path bounds in units of u: see the module docstring."""
    G = {'bil': 1, 'mlpdot': L, 'mlpbil': L + 1, 'mlpcat': L}[kind]
    return 8 * G + D + 2, 16 * G + 8 + D + 6


# ---- 1. indexed-row GEMM: bit equality ------------------------------------------------------------------------------------------------
def _check_rows_gemm(h, idx, Nout, gen, bias_on, relu, p=0.3):
    from gnn_tail_generalization_amd import gemm, ops
    nseg, R = idx.shape
    K = nseg * h.shape[1]
    w = (torch.randn(Nout, K, generator=gen) / K ** 0.5).to(DEV)
    bias = torch.randn(Nout, generator=gen).to(DEV) if bias_on else None
    b = w.t().contiguous()
    a = _operand(h, idx)
    want = gemm.mm_nn(a, b, bias=bias, relu=relu)
    got, st = ops.rows_linear(h, idx, w, bias, relu=relu, fused=True, return_status=True)
    assert torch.equal(got, want) and int(st.item()) == 0, (nseg, K, Nout, R)
    seed, row0 = 7654321 + K, 3
    y, yd = gemm.mm_nn_drop2(a, b, p, seed, row0, bias=bias, relu=relu)
    e = h if h.stride(1) == 1 and h.stride(0) >= h.shape[1] else h.contiguous()
    y2, yd2, st = ops._rows_linear_raw(e, idx.to(torch.int32).contiguous(), b, bias, relu, p, seed, row0)
    assert torch.equal(y2, y) and torch.equal(yd2, yd) and torch.equal(y2, want) and int(st.item()) == 0, (nseg, K, Nout, R)
    assert torch.equal(ops.rows_linear(h, idx, w, bias, relu=relu, p=p, seed=seed, row0=row0), yd)


@pytest.mark.parametrize('nseg', [1, 2])
@pytest.mark.parametrize('D', [16, 48, 256])
def test_rows_gemm_has_the_bits_of_the_gemm_on_the_materialised_operand(nseg, D):
    """D: one K step per segment, three, the workload width.  Nout: both sides of the Nout <= 64 tile choice (4, 64 | 68) and two column blocks (256
    on the 128 x 128 tile).  R: the row-tile tails of the 128- and 256-row tiles.  Bias and ReLU on and off."""
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(100 * nseg + D)
    N = 90
    h = torch.randn(N, D, generator=gen).to(DEV)
    flags = [(False, False), (True, True), (True, False), (False, True)]
    i = 0
    for Nout in (4, 64, 68, 256):
        for R in (1, 127, 128, 129, 257):
            idx = torch.randint(0, N, (nseg, R), generator=gen).to(DEV)
            assert ops.rows_linear_supported(h, idx, torch.empty(Nout, nseg * D, device=DEV))
            _check_rows_gemm(h, idx, Nout, gen, *flags[i % 4])
            i += 1
    ops.pair_check()
    _status_ok()


@pytest.mark.parametrize('nseg', [1, 2])
def test_rows_gemm_on_the_wide_tile(nseg):
    """R = 128 * 256 + 5 rows at Nout = 256 make one 128 x 256 tile per CU: the launcher takes the wide tile there (and its dual-output epilogue with
    p > 0); D = 16 keeps the run short.  One row more than a whole number of tiles."""
    gen = torch.Generator().manual_seed(nseg)
    N, D, R = 500, 16, 128 * 256 + 5
    h = torch.randn(N, D, generator=gen).to(DEV)
    idx = torch.randint(0, N, (nseg, R), generator=gen).to(DEV)
    _check_rows_gemm(h, idx, 256, gen, True, True)
    _status_ok()


# ---- 2. index patterns ----------------------------------------------------------------------------------------------------------------
def test_rows_gemm_index_patterns_and_unusable_indices():
    from gnn_tail_generalization_amd import _lib, gemm, ops
    gen = torch.Generator().manual_seed(2)
    N, D, R, Nout = 30, 16, 200, 68
    h = torch.randn(N, D, generator=gen).to(DEV)
    one = torch.full((2, R), 7, dtype=torch.int64, device=DEV)                       # all indices one node
    same = torch.randint(0, N, (1, R), generator=gen).to(DEV).repeat(2, 1)           # idx0 == idx1
    for idx in (one, one[:1], same):
        _check_rows_gemm(h, idx, Nout, gen, True, True)
    _check_rows_gemm(h[:1], torch.zeros((2, R), dtype=torch.int64, device=DEV), Nout, gen, True, False)      # N = 1
    wide = torch.randn(N, D + 8, generator=gen).to(DEV)
    for nseg in (1, 2):                                                              # h as a column slice of a wider matrix (ld = D + 8)
        _check_rows_gemm(wide[:, 4:4 + D], torch.randint(0, N, (nseg, R), generator=gen).to(DEV), Nout, gen, False, True)
    # one index -1 and one equal to N: NaN rows in both outputs, counted; every other row as in the clean run
    for nseg in (1, 2):
        for Nout_ in (8, 68):      # the two-kernel and the one-kernel form of the dropped copy
            w = (torch.randn(Nout_, nseg * D, generator=gen) / 4).to(DEV)
            b = w.t().contiguous()
            idx = torch.randint(0, N, (nseg, R), generator=gen).to(torch.int32)
            bad = idx.clone()
            bad[0, 3], bad[nseg - 1, 150] = -1, N
            clean = ops._rows_linear_raw(h, idx.to(DEV), b, None, True, 0.3, 99, 0)
            y, yd, st = ops._rows_linear_raw(h, bad.to(DEV), b, None, True, 0.3, 99, 0)
            rows = torch.ones(R, dtype=torch.bool, device=DEV)
            rows[[3, 150]] = False
            assert int(st.item()) == 2 and int(clean[2].item()) == 0
            for got, want in ((y, clean[0]), (yd, clean[1])):
                assert bool(torch.isnan(got[~rows]).all()) and torch.equal(got[rows], want[rows])
            got, st2 = ops.rows_linear(h, bad.to(DEV), w, relu=True, return_status=True)
            assert int(st2.item()) == 2 and torch.equal(got[rows], clean[0][rows]) and bool(torch.isnan(got[~rows]).all())
            comp, st3 = ops.rows_linear(h, bad.to(DEV), w, relu=True, return_status=True, fused=False)
            assert int(st3.item()) == 2 and torch.equal(comp[rows], clean[0][rows]) and bool(torch.isnan(comp[~rows]).all())
    with pytest.raises(RuntimeError, match='pair'):
        ops.rows_linear.check()
    # outside the fused form the same operators run one after the other; fused=True refuses
    h20 = torch.randn(N, 20, generator=gen).to(DEV)
    for hh, nseg, Nout_ in ((h20, 2, 8), (h, 2, 6), (h, 1, 6)):
        idx = torch.randint(0, N, (nseg, R), generator=gen).to(DEV)
        w = torch.randn(Nout_, nseg * hh.shape[1], generator=gen).to(DEV)
        assert not ops.rows_linear_supported(hh, idx, w)
        got = ops.rows_linear(hh, idx, w, relu=True)
        assert torch.equal(got, ops.rows_linear(hh, idx, w, relu=True, fused=False))
        assert torch.equal(got, gemm.mm_nn(_operand(hh, idx), w.t().contiguous(), relu=True))
        with pytest.raises(_lib.HipExtensionError, match='fused form'):
            ops.rows_linear(hh, idx, w, fused=True)
    assert ops.rows_linear_supported(h20, torch.zeros((1, 4), dtype=torch.int64, device=DEV), torch.empty(8, 20, device=DEV))      # one segment: D % 4
    ops.pair_check()
    _status_ok()


def test_rows_linear_gradients_against_float64():
    """sum(y * g) for both segment counts, an odd and an even number of rows: dH through the row scatter, dW through mm_tn, db; the bound of a
    two-operation path (GEMM 8 u, then the scatter's 2 u, or the TN GEMM alone) on the sum of absolute terms."""
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(3)
    N, D, Nout = 25, 16, 8
    for nseg, R in ((1, 101), (1, 64), (2, 77)):
        h = torch.randn(N, D, generator=gen)
        idx = torch.randint(0, 20, (nseg, R), generator=gen)      # rows 20 .. 24 stay untouched
        w, b, g = torch.randn(Nout, nseg * D, generator=gen) / 4, torch.randn(Nout, generator=gen), torch.randn(R, Nout, generator=gen)
        hd, wd, bd = h.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        (ops.rows_linear(hd, idx.to(DEV), wd, bd, relu=True) * g.to(DEV)).sum().backward()
        got = (hd.grad, wd.grad, bd.grad)

        def run(hh, ww, bb, gg, relu_mask=None):
            hh, ww, bb = hh.double().requires_grad_(True), ww.double().requires_grad_(True), bb.double().requires_grad_(True)
            z = _operand(hh, idx) @ ww.t() + bb
            mask = (z > 0) if relu_mask is None else relu_mask
            (torch.where(mask, z, torch.zeros_like(z)) * gg.double()).sum().backward()
            return (hh.grad, ww.grad, bb.grad), mask
        want, mask = run(h, w, b, g)
        mags, _ = run(h.abs(), w.abs(), b.abs(), g.abs(), mask)
        for name, a, r, s in zip(('dh', 'dw', 'db'), got, want, mags):
            err = (a.cpu().double() - r).abs()
            bound = 10 * U * s + 2.0 ** -23 * r.abs()
            print(f'nseg {nseg} R {R} {name}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
            assert bool((err <= bound).all()), (nseg, R, name)
        assert bool((hd.grad[20:] == 0).all())
    _status_ok()


# ---- 3. bilinear pair score -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [4, 16, 132, 256])
def test_pair_bilinear_against_float64(D):
    """D: one lane group partly filled (4), the 256 x 64 tile (16), two column blocks with a tail (132), the workload width (256).  S: one pair, one
    row past the 128-row tile, a batch whose permutation crosses the row tiles."""
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(D)
    N = 60
    h = torch.randn(N, D, generator=gen)
    W = torch.randn(D, D, generator=gen) / D ** 0.5
    hd, Wd = h.to(DEV), W.to(DEV)
    assert ops.pair_bilinear_supported(hd, Wd)
    for S in (1, 129, 300):
        pairs = torch.randint(0, N, (2, S), generator=gen)
        if S > 20:
            pairs[0, :10] = 5
            pairs[1, 10:15] = pairs[0, 10:15]
        s, st = ops.pair_bilinear(hd, pairs.to(DEV), Wd, return_status=True)
        want, scale = pr.bilinear64(h, pairs, W)
        z = h.double()[pairs[0]] @ W.double().t()
        bound = 8 * U * scale + D * U * (z * h.double()[pairs[1]]).abs().sum(-1)
        err = (s.cpu().double() - want).abs()
        print(f'D {D} S {S}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}')
        assert int(st.item()) == 0 and s.dtype == torch.float32 and tuple(s.shape) == (S,)
        assert bool((err <= bound).all())
        assert torch.equal(ops.pair_bilinear(hd, pairs.to(DEV), Wd), s)                  # two calls: the same bits
        perm = torch.randperm(S, generator=gen)
        assert torch.equal(ops.pair_bilinear(hd, pairs[:, perm].to(DEV), Wd), s[perm.to(DEV)])      # a score does not depend on its place
        if S > 20:      # unusable pairs: NaN, counted; the others unchanged
            bad = pairs.clone()
            bad[0, 2], bad[1, 128], bad[0, 17] = -1, N, N + 5
            sb, stb = ops.pair_bilinear(hd, bad.to(DEV), Wd, return_status=True)
            ok = pr.usable(bad, N).to(DEV)
            assert int(stb.item()) == 3 and bool(torch.isnan(sb[~ok]).all()) and torch.equal(sb[ok], s[ok])
            with pytest.raises(RuntimeError, match='3 pair'):
                ops.pair_bilinear.check()
    ops.pair_check()
    _status_ok()


def test_pair_bilinear_gradients_and_the_composed_shape():
    """Autograd of sum(s * g): dH = scatter of g (h[v] W) into u and g (h[u] W^T) into v, dW = (g h[v])^T h[u]; a GEMM (8 u), the product with g (1 u)
    and the scatter (2 u) or the TN GEMM (8 u) on the sum of absolute terms.  D = 6 lies outside the fused form: the composed value, same bounds."""
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(8)
    N, S = 30, 150
    for D in (16, 132, 6):
        h, W, g = torch.randn(N, D, generator=gen), torch.randn(D, D, generator=gen) / D ** 0.5, torch.randn(S, generator=gen)
        pairs = torch.randint(0, 25, (2, S), generator=gen)
        pairs[1, :6] = pairs[0, :6]
        hd, Wd = h.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
        assert ops.pair_bilinear_supported(hd, Wd) == (D != 6)
        s = ops.pair_bilinear(hd, pairs.to(DEV), Wd)
        (s * g.to(DEV)).sum().backward()

        def run(hh, ww, gg):
            hh, ww = hh.double().requires_grad_(True), ww.double().requires_grad_(True)
            out = ((hh[pairs[0]] @ ww.t()) * hh[pairs[1]]).sum(-1)
            (out * gg.double()).sum().backward()
            return out.detach(), hh.grad, ww.grad
        want = run(h, W, g)
        mags = run(h.abs(), W.abs(), g.abs())
        for name, a, r, m, units in (('s', s.detach(), want[0], mags[0], 8 + D), ('dh', hd.grad, want[1], mags[1], 8 + 1 + 2), ('dW', Wd.grad, want[2], mags[2], 8 + 1)):
            err = (a.cpu().double() - r).abs()
            print(f'D {D} {name}: worst error / bound {float((err / (units * U * m).clamp_min(1e-300)).max()):.3f}')
            assert bool((err <= units * U * m).all()), (D, name)
        assert bool((hd.grad[25:] == 0).all())
    _status_ok()


def test_pair_bilinear_allocates_nothing_of_size_s_by_d():
    """S = 65 536, D = 256 under torch.no_grad(): after one warm-up call, a call's peak over its start stays below S D 4 / 2 bytes.  The honest
    need is the scores (S 4), the column-block partials (S 2 4) and the transposed weight (D D 4)."""
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(9)
    N, D, S = 1000, 256, 65536
    h, W = torch.randn(N, D, generator=gen).to(DEV), (torch.randn(D, D, generator=gen) / 16).to(DEV)
    pairs = torch.randint(0, N, (2, S), generator=gen).to(DEV).to(torch.int32)
    with torch.no_grad():
        first = ops.pair_bilinear(h, pairs, W)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        s = ops.pair_bilinear(h, pairs, W)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - start
    print(f'peak over start {peak} bytes; S D 4 / 2 = {S * D * 4 // 2}; S 4 + S 2 4 + D D 4 = {S * 4 + S * 8 + D * D * 4}')
    assert peak < S * D * 4 // 2
    assert torch.equal(s, first) and bool(torch.isfinite(s).all())
    _status_ok()


# ---- 4. row scatter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [4, 260])
def test_row_scatter_against_float64(D):
    """D = 260 crosses the 256-column chunk.  One node in all 2000 pairs (as u), self pairs, nodes 40 .. 48 untouched, unusable pairs, sources with
    leading dimensions of their own (the halves of one [2 S, D] matrix, the column halves of one [S, 2 D + 3] matrix), out wider than D."""
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(D)
    N, S = 50, 2000
    pairs = torch.randint(0, 40, (2, S), generator=gen)
    pairs[0, :] = 11                                   # one node present in all the pairs
    pairs[1, 100:140] = 11                             # self pairs: both rows go into one node
    pairs[1, 140:150] = N - 1
    bad = pairs.clone()
    bad[0, 2], bad[1, 301], bad[1, 120] = -1, N, -7
    tall = torch.randn(2 * S, D, generator=gen)
    flat = torch.randn(S, 2 * D + 3, generator=gen)
    talld, flatd = tall.to(DEV), flat.to(DEV)
    for prs in (pairs, bad):
        pd = prs.to(DEV)
        for (g0, g1), (d0, d1) in (((tall[:S], tall[S:]), (talld[:S], talld[S:])), ((flat[:, :D], flat[:, D:2 * D]), (flatd[:, :D], flatd[:, D:2 * D]))):
            want, sa = pr.scatter_rows64(prs, g0, g1, N)
            got = ops.pair_scatter_rows(pd, d0, d1, N)
            err = (got.cpu().double() - want).abs()
            bound = 2.0 ** -23 * want.abs() + 2.0 ** -40 * sa
            print(f'D {D}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
            assert bool((err <= bound).all()), (D, float((err - bound).max()))
            touched = torch.zeros(N, dtype=torch.bool)
            touched[prs[:, pr.usable(prs, N)].reshape(-1)] = True
            assert not bool(touched[40:N - 1].any()) and bool((got.cpu()[~touched] == 0).all()) and not bool(torch.isnan(got).any())
            out = torch.full((N, D + 5), 7.0, device=DEV)      # ldd > D: the padding stays; two calls give identical bits
            again = ops.pair_scatter_rows(pd, d0, d1, N, out=out[:, :D])
            assert torch.equal(again, got) and bool((out[:, D:] == 7.0).all())
    empty = ops.pair_scatter_rows(torch.zeros((2, 0), dtype=torch.int64, device=DEV), talld[:0], talld[:0], N)
    assert tuple(empty.shape) == (N, D) and bool((empty == 0).all())
    _status_ok()


# ---- 5. the predictors against the recording ------------------------------------------------------------------------------------------
def _check_against_recording(kind, L, r, h, pairs, gout, mod, tag):
    fu, gu = _units(kind, L)
    a_out, a_dh, a_g = pr.predictor_abs64(kind, r['state_dict'], h, pairs, gout)
    hd = h.to(DEV).requires_grad_(True)
    out = mod.score_pairs(hd, pairs.to(DEV))
    assert tuple(out.shape) == tuple(r['out64'].shape) and out.dtype == torch.float32
    (out.reshape(pairs.shape[1], -1) * gout.to(DEV).float()).sum().backward()

    def check(got, want, scale, units, name):
        err = (got.cpu().double() - want).abs()
        bound = units * U * scale
        print(f'{tag} {kind} L {L} {name}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
        assert bool((err <= bound).all()), (kind, L, name)
    check(out.detach(), r['out64'], a_out, fu, 'out')
    d32 = float((r['out32'].double() - r['out64']).abs().max())
    print(f'    the reference fp32 module is {d32:.3e} from its float64 run')
    check(hd.grad, r['dh64'], a_dh, gu, 'dh')
    for k, p in mod.named_parameters():
        check(p.grad, r['grads64'][k], a_g[k], gu, k)
    return out.detach()


@pytest.mark.parametrize('kind', pr.KINDS)
@pytest.mark.parametrize('L', [1, 2, 3])
def test_predictors_against_the_reference_recording(kind, L, rec):
    """score_pairs on the per-pair route (the kernels of cb_pairpred.hip) and its gradients with respect to h and every parameter against the float64
    run of the reference module, eval mode; bounds: the module docstring's path bounds."""
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    r, h, pairs, gout = rec[kind][L], rec['h'], rec['pairs'], rec['gout']
    mod = _module(kind, L, r['state_dict']).eval()
    hd, pd = h.to(DEV), pairs.to(DEV)
    with _tuned(score_pairs_fused=True, pair_predictor_per_node=False):
        pp.routes.clear()
        out = _check_against_recording(kind, L, r, h, pairs, gout, mod, 'per-pair')
        assert list(pp.routes) == ['per_pair']
        with torch.no_grad():
            fwd = mod(hd[pd[0]], hd[pd[1]])
            if kind == 'mlpcat':      # every row of the fused first layer has the bits of the gathered one, and the rest is the same code
                assert torch.equal(fwd, out)
            if kind in ('mlpdot', 'mlpbil'):      # the activations before the final reduction are those of the composed stack
                z = mod.endpoint_rows(hd, pd)
                assert torch.equal(z, mod._stack(torch.cat([hd[pd[0]], hd[pd[1]]], dim=0)))
        with _tuned(score_pairs_fused=False):
            with torch.no_grad():
                gathered = mod.score_pairs(hd, pd)
            assert pp.routes[-1] == 'gathered' and torch.equal(gathered, fwd)
        # fused against gathered: the same activations, two ways of taking the final reduction, each within the dot's bound
        if kind in ('mlpdot', 'mlpbil', 'bil'):
            S, D = pairs.shape[1], 16
            with torch.no_grad():
                zi, zj = (z[:S], z[S:]) if kind != 'bil' else (hd[pd[0]], hd[pd[1]])
                if kind != 'mlpdot':
                    zi = zi @ mod.bilin.weight.t()
            sabs = (zi.double() * zj.double()).abs().sum(-1).cpu()
            # (bilin(x_i) has the same bits on either side: the same K loop on the same values.)  Fused: fewer than D additions; gathered: D
            # rounded products and D - 1 additions
            err = (out.cpu().double() - gathered.cpu().double()).abs()
            print(f'{kind} L {L} fused - gathered: worst error / bound {float((err / ((2 * D + 2) * U * sabs).clamp_min(1e-300)).max()):.3f}')
            assert bool((err <= (2 * D + 2) * U * sabs).all())
    ops.pair_check()
    _status_ok()


@pytest.mark.parametrize('kind', ['mlpdot', 'mlpbil'])
def test_the_factory_width_one_predictors_run_composed_and_match_their_recording(kind, rec):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.Link_prediction_model import create_pair_predictor_layer
    r, h, pairs, gout = rec['width_one'][kind], rec['h'], rec['pairs'], rec['gout']
    mod = create_pair_predictor_layer(16, 2, 0.5, kind).to(DEV).eval()
    mod.load_state_dict(r['state_dict'])
    assert not ops.rows_linear_supported(h.to(DEV), pairs.to(DEV).reshape(1, -1), mod.lins[0].weight)      # Nout = 1: the composed operators
    fu, gu = _units(kind, 2, D=1)
    a_out, a_dh, a_g = pr.predictor_abs64(kind, r['state_dict'], h, pairs, gout)
    for per_node in (False, True):
        with _tuned(score_pairs_fused=True, pair_predictor_per_node=per_node):
            hd = h.to(DEV).requires_grad_(True)
            out = mod.score_pairs(hd, pairs.to(DEV))
            (out * gout.reshape(-1).to(DEV).float()).sum().backward()
        assert bool(((out.detach().cpu().double() - r['out64']).abs() <= fu * U * a_out).all())
        assert bool(((hd.grad.cpu().double() - r['dh64']).abs() <= gu * U * a_dh).all())
        for k, p in mod.named_parameters():
            assert bool(((p.grad.cpu().double() - r['grads64'][k]).abs() <= gu * U * a_g[k]).all()), k
            p.grad = None
    ops.pair_check()
    _status_ok()


# ---- 6. dropout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mlpdot', 'mlpbil', 'mlpcat'])
def test_dropout_uses_the_host_restatement_of_the_keep_masks(kind, rec):
    """Training mode, p = 0.5, two layers: one seed per layer that is followed by dropout, each for the keep-mask of the [2 S, width] matrix whose
    rows e are the x_i side (x1) and rows S + e the x_j side (x2), offset 0.  The output equals the composed evaluation with the host's masks, bit
    for bit, and the two sides of a self pair are dropped differently."""
    import coldbrew_oracle as orc
    from gnn_tail_generalization_amd import gemm, ops
    r, h, pairs = rec[kind][2], rec['h'].to(DEV), rec['pairs'].to(DEV)
    S, p = pairs.shape[1], 0.5
    mod = _module(kind, 2, r['state_dict'], dropout=p).train()
    seeds = [4242, 977] if kind != 'mlpcat' else [4242]
    with _tuned(score_pairs_fused=True, pair_predictor_per_node=None):
        ops._seed_override.extend(seeds)
        out = mod.score_pairs(h, pairs)
        assert not ops._seed_override

    def dropped(x, seed):
        keep = torch.from_numpy(orc.dropout_keep_mask(tuple(x.shape), p, seed)).to(DEV)
        return torch.where(keep, x * _keep_scale(p), torch.zeros_like(x)), keep
    hu, hv = h[pairs[0]], h[pairs[1]]
    l0, l1 = mod.lins
    if kind == 'mlpcat':
        x = torch.cat([torch.cat([hu, hv], -1), torch.cat([hv, hu], -1)], 0)
        x, keep = dropped(gemm.mm_nn(x, l0.weight.t().contiguous(), bias=l0.bias, relu=True), seeds[0])
        y = gemm.mm_nn(x, l1.weight.t().contiguous(), bias=l1.bias)
        assert torch.equal(out.detach(), (y[:S] + y[S:]) / 2)
    else:
        x, _ = dropped(gemm.mm_nn(torch.cat([hu, hv], 0), l0.weight.t().contiguous(), bias=l0.bias, relu=True), seeds[0])
        x, keep = dropped(gemm.mm_nn(x, l1.weight.t().contiguous(), bias=l1.bias, relu=True), seeds[1])
        halves = torch.arange(2 * S, dtype=torch.int32, device=DEV).reshape(2, S)
        want = ops.pair_dot(x, halves) if kind == 'mlpdot' else ops.pair_bilinear(x, halves, mod.bilin.weight)
        assert torch.equal(out.detach(), want.detach())
    selfs = (pairs[0] == pairs[1]).nonzero().reshape(-1)
    assert selfs.numel() >= 5
    for e in selfs.tolist():      # the same node on both sides: the two rows never share a mask ...
        assert not torch.equal(keep[e], keep[S + e])
    assert not torch.equal(x[selfs], x[S + selfs])      # ... and their dropped activations differ (where both masks keep only what the ReLU left, a row pair can agree)
    # forward() on the gathered rows draws the same masks from the same seeds
    ops._seed_override.extend(seeds)
    fwd = mod(hu, hv)
    assert not ops._seed_override
    if kind == 'mlpcat':
        assert torch.equal(fwd.detach(), out.detach())
    # the backward regenerates the masks: dH against float64 autograd of the restatement with the host's masks
    gout = rec['gout']
    hd = rec['h'].to(DEV).requires_grad_(True)
    ops._seed_override.extend(seeds)
    with _tuned(score_pairs_fused=True):
        (mod.score_pairs(hd, pairs).reshape(S, -1) * gout.to(DEV).float()).sum().backward()
    widths = [16, 16]
    masks = [(torch.from_numpy(orc.dropout_keep_mask((2 * S, w), p, s)), p) for w, s in zip(widths, seeds)]
    _, dh, _ = pr.predictor_grads64(kind, r['state_dict'], rec['h'], rec['pairs'], gout, keep=masks)
    _, a_dh, _ = pr.predictor_abs64(kind, r['state_dict'], rec['h'], rec['pairs'], gout)
    _, gu = _units(kind, 2)
    err = (hd.grad.cpu().double() - dh).abs()
    bound = gu * U * a_dh / (1.0 - p) ** 2      # every kept entry carries 1 / (1 - p) per dropout it passed
    print(f'{kind} dropout dh: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert bool((err <= bound).all())
    ops.pair_check()
    _status_ok()


# ---- 7. per-node route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mlpdot', 'mlpbil', 'bil'])
def test_the_per_node_route_gives_the_same_bits(kind, rec):
    """N = 40, S = 120, eval mode: the stack applied to the N rows of h once, against the stack applied to the 2 S endpoint rows."""
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    r, h = rec[kind][2], rec['h']
    gen = torch.Generator().manual_seed(31)
    N, S = h.shape[0], 120
    pairs = torch.randint(0, N, (2, S), generator=gen)
    pairs[1, :7] = pairs[0, :7]
    gout = (torch.rand(S, 1, generator=gen) * 2 - 1).double()
    mod = _module(kind, 2, r['state_dict']).eval()
    fu, gu = _units(kind, 2)
    want = pr.predictor_grads64(kind, r['state_dict'], h, pairs, gout)
    mags = pr.predictor_abs64(kind, r['state_dict'], h, pairs, gout)
    outs = {}
    for route in (True, False):
        with _tuned(score_pairs_fused=True, pair_predictor_per_node=route):
            pp.routes.clear()
            hd = h.to(DEV).requires_grad_(True)
            out = mod.score_pairs(hd, pairs.to(DEV))
            assert list(pp.routes) == ['per_node' if route else 'per_pair']
            (out * gout.reshape(-1).to(DEV).float()).sum().backward()
        outs[route] = out.detach()
        assert bool(((out.detach().cpu().double() - want[0]).abs() <= fu * U * mags[0]).all())
        err = (hd.grad.cpu().double() - want[1]).abs()
        print(f'{kind} per_node={route} dh: worst error / bound {float((err / (gu * U * mags[1]).clamp_min(1e-300)).max()):.3f}')
        assert bool((err <= gu * U * mags[1]).all())
        for k, p in mod.named_parameters():
            assert bool(((p.grad.cpu().double() - want[2][k]).abs() <= gu * U * mags[2][k]).all()), (route, k)
            p.grad = None
    assert torch.equal(outs[True], outs[False])
    # the rule: a row count.  2 S >= N takes the per-node route, fewer endpoint rows than nodes the per-pair one; dropout in training takes neither
    with _tuned(score_pairs_fused=True, pair_predictor_per_node=None), torch.no_grad():
        pp.routes.clear()
        assert torch.equal(mod.score_pairs(h.to(DEV), pairs.to(DEV)), outs[True])
        mod.score_pairs(h.to(DEV), pairs[:, :10].to(DEV))
        mod.score_pairs(h.to(DEV), pairs[:, :20].to(DEV))
        assert list(pp.routes) == ['per_node', 'per_pair', 'per_node']
        if kind != 'bil':
            pp.routes.clear()
            mod.train()
            mod.score_pairs(h.to(DEV), pairs.to(DEV))
            mod.eval()
            assert list(pp.routes) == ['per_pair']
    ops.pair_check()
    _status_ok()


# ---- 8. training and tools ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('predictor', ['BIL', 'MLPDOT', 'MLPBIL', 'MLPCAT'])
def test_training_with_the_new_predictors(predictor, tmp_path, monkeypatch):
    """Twenty epochs of trainer.setup_linkpred_encoder / train_linkpred_encoder on S-tiny (MLP encoder over the trainable embedding, log_rank_loss):
    finite losses, predictor and encoder parameters that moved, metrics in [0, 1], the last epoch's loss below the first."""
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkpred_encoder
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    first = {}
    setup = trainer.setup_linkpred_encoder

    def recording_setup(self):
        setup(self)
        first['pred'] = [p.detach().clone() for p in self.predictor.parameters()]
        first['enc'] = [p.detach().clone() for p in self.encoder.parameters()]
    monkeypatch.setattr(trainer, 'setup_linkpred_encoder', recording_setup)
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkpred_encoder.main(['--dataset=S-tiny', '--encoder=MLP', f'--predictor={predictor}', '--loss_func=log_rank_loss', '--num_neg=3',
                                            '--epochs=20'] + PLUMBING)
    _status_ok()
    losses, metrics = recs[0]
    print(f'{predictor}: loss by epoch {np.round(losses, 4).tolist()}; {metrics}')
    t = train_linkpred_encoder.main.last_trainer
    want = {'BIL': pp.BilinearPairPredictor, 'MLPDOT': pp.MLPDotPairPredictor, 'MLPBIL': pp.MLPBilPairPredictor, 'MLPCAT': pp.MLPCatPairPredictor}[predictor]
    assert type(t.predictor) is want
    if predictor != 'BIL':      # input width = the embedding width, hidden width = --mlp_hidden_channels: not the factory's width one
        assert t.predictor.lins[0].weight.shape[0] == t.args.mlp_hidden_channels and t.predictor.lins[0].weight.shape[1] in (t.args.gnn_hidden_channels, 2 * t.args.gnn_hidden_channels)
    assert len(recs) == 1 and losses.shape == (20,) and np.isfinite(losses).all()
    assert set(metrics) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and all(0.0 <= float(v) <= 1.0 for v in metrics.values())
    assert any(not torch.equal(a, b.detach()) for a, b in zip(first['pred'], t.predictor.parameters()))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(first['enc'], t.encoder.parameters()))
    assert losses[-1] < losses[0]


def test_tool_end_to_end_with_the_concatenating_predictor(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkpred
    import train_linkpred_encoder
    from gnn_tail_generalization_amd.Link_prediction_model import pair_predictor as pp
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkpred_encoder.main(['--dataset=S-tiny', '--encoder=SAGE', '--predictor=MLPCAT', '--epochs=2'] + PLUMBING)
    _status_ok()
    losses, metrics = recs[0]
    assert len(recs) == 1 and losses.shape == (2,) and np.isfinite(losses).all() and 0.0 <= metrics['AUC'] <= 1.0
    assert type(train_linkpred_encoder.main.last_trainer.predictor) is pp.MLPCatPairPredictor
    with contextlib.redirect_stdout(io.StringIO()):      # the teacher's trainer builds them too, over its own embedding width
        recs = train_linkpred.main(['--dataset=S-tiny', '--predictor=MLPBIL', '--loss_func=log_rank_loss', '--num_neg=3', '--epochs=2', '--batch_size=128'] + PLUMBING)
    _status_ok()
    assert len(recs) == 1 and recs[0][0].shape == (2,) and np.isfinite(recs[0][0]).all() and 0.0 <= recs[0][1]['AUC'] <= 1.0
