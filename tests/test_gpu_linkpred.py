"""The link predictors and ranking losses on the device (csrc/cb_linkpred.hip, ops.pair_dot / pair_linear / rank_loss,
Link_prediction_model/) against the recordings of the unmodified reference (tests/golden/linkpred_*.pt) and the float64 restatement of
tests/linkpred_ref.py.  Bounds are derived, with u = 2^-24 the unit roundoff of fp32:
  losses      every kind is a float64 sum of non-negative terms rounded to fp32 once: |dev - r| <= 2^-23 |r|
  gradients   a float64 sum of at most 7 signed terms of size at most 82 (|s| <= 20, k <= 7) errs by under 1e-13; rounded once: 2^-23 |r| + 1e-10
  pair GEMM   bit-equality with gemm.mm_nn / mm_nn_drop2 on the materialised product: one rounded multiply, the same K loop — no tolerance
  scatter     a float64 sum rounded once: 2^-23 |r| + 2^-40 sum|terms|
  pair dot    a chain of 4 ceil(D / 256) fused multiply-adds per lane, then a 6-level butterfly: gamma_n sum|terms|, n = 4 ceil(D / 256) + 6
"""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

import linkpred_ref as lr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24


@pytest.fixture(scope='module')
def loss_cases():
    return load_golden('linkpred_losses')


@pytest.fixture(scope='module')
def pred_rec():
    return load_golden('linkpred_predictors')


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', lr.KINDS)
def test_losses_and_gradients_against_the_float64_recording(kind, loss_cases):
    from gnn_tail_generalization_amd import ops
    for c in loss_cases:      # spans 20 and 3; (P, k) = (1, 1), (5, 3), (257, 7)
        rec = c['kinds'][kind]
        pos, neg, w = c['pos'].to(DEV).requires_grad_(True), c['neg'].to(DEV).requires_grad_(True), c['weight'].to(DEV)
        loss = ops.rank_loss(kind, pos, neg, c['k'], w if kind == 'adaptive_auc_loss' else None)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        r, dev, f32 = float(rec['f64']), float(loss.detach().double()), float(rec['f32'].double())
        print(f'{kind} span {c["span"]:g} P {c["P"]} k {c["k"]}: dev {dev:.9g} f64 {r:.9g} rel {abs(dev - r) / abs(r):.3e}; reference fp32 rel {abs(f32 - r) / abs(r):.3e}')
        assert abs(dev - r) <= 2.0 ** -23 * abs(r)
        assert abs(dev - r) <= abs(f32 - r) + 2.0 ** -23 * abs(r)
        loss.backward()
        for got, want, name in ((pos.grad, rec['dpos64'], 'dpos'), (neg.grad, rec['dneg64'], 'dneg')):
            err = (got.cpu().double() - want).abs()
            bound = 2.0 ** -23 * want.abs() + 1e-10
            print(f'    {name}: worst error / bound {float((err / bound).max()):.3f}')
            assert bool((err <= bound).all()), (kind, c['span'], c['P'], name)
        # two calls give identical bits; an upstream scalar scales the gradient
        p2, n2 = c['pos'].to(DEV).requires_grad_(True), c['neg'].to(DEV).requires_grad_(True)
        loss2 = ops.rank_loss(kind, p2, n2, c['k'], w if kind == 'adaptive_auc_loss' else None)
        (loss2 * 0.5).backward()
        assert torch.equal(loss2.detach(), loss.detach())
        err = (p2.grad.cpu().double() - 0.5 * rec['dpos64']).abs()
        assert bool((err <= 2.0 ** -23 * (0.5 * rec['dpos64']).abs() + 1e-10).all())
        p3, n3 = c['pos'].to(DEV).requires_grad_(True), c['neg'].to(DEV).requires_grad_(True)
        ops.rank_loss(kind, p3, n3, c['k'], w if kind == 'adaptive_auc_loss' else None).backward()
        assert torch.equal(p3.grad, pos.grad) and torch.equal(n3.grad, neg.grad)


def test_loss_functions_shapes_and_more_blocks_than_one():
    """The reference's names on [P, 1] predictor outputs; P = 70 000 rows spread over the 256 partial blocks of the two-stage sum, against the
    float64 restatement; shapes that do not reshape are refused."""
    from gnn_tail_generalization_amd.Link_prediction_model import calculate_loss, loss
    g = torch.Generator().manual_seed(5)
    P, k = 70_000, 3
    pos, neg = (torch.rand(P, 1, generator=g) * 6 - 3), (torch.rand(P * k, 1, generator=g) * 6 - 3)
    for kind in lr.KINDS:
        w = torch.rand(P, generator=g) + 0.5
        r = float(lr.rank_loss64(kind, pos, neg, k, w))
        if kind == 'ce_loss':
            dev = loss.ce_loss(pos.to(DEV), neg.to(DEV))
        elif kind == 'adaptive_auc_loss':
            dev = loss.adaptive_auc_loss(pos.to(DEV), neg.to(DEV), k, w.to(DEV))
        else:
            dev = getattr(loss, kind)(pos.to(DEV), neg.to(DEV), k)
        assert abs(float(dev.double()) - r) <= 2.0 ** -23 * abs(r), kind
    assert torch.equal(calculate_loss('AUC', pos.to(DEV), neg.to(DEV), k), loss.auc_loss(pos.to(DEV), neg.to(DEV), k))
    with pytest.raises(ValueError, match='reshape'):
        loss.auc_loss(pos[:5].to(DEV), neg[:14].to(DEV), 3)
    with pytest.raises(ValueError, match='reshape'):
        loss.ce_loss(pos[:4].to(DEV), neg[:6].to(DEV))


def _keep_scale(p):
    """1 / (1 - p) as the kernels form it: in fp32."""
    return float(1.0 / (1.0 - torch.tensor(p, dtype=torch.float32)))


# ---- pair GEMM ------------------------------------------------------------------------------------------------------------------------
def _pairs(S, N, gen, pattern=False):
    p = torch.randint(0, N, (2, S), generator=gen)
    if pattern:      # one node in 300 pairs, self pairs, node N - 1
        p[0, :300] = 7
        p[1, 300:320] = p[0, 300:320]
        p[0, 320:330] = N - 1
        p[1, 330:340] = N - 1
    return p


def _check_pair_gemm(h, pairs, K, Nout, gen, relu):
    from gnn_tail_generalization_amd import gemm, ops
    w = (torch.randn(Nout, K, generator=gen) / K ** 0.5).to(DEV)
    bias = torch.randn(Nout, generator=gen).to(DEV)
    pd = pairs.to(DEV)
    x = h[pd[0]] * h[pd[1]]
    b = w.t().contiguous()
    want = gemm.mm_nn(x, b, bias=bias, relu=relu)
    got, st = ops.pair_linear(h, pd, w, bias, relu=relu, fused=True, return_status=True)
    assert torch.equal(got, want) and int(st.item()) == 0
    seed, row0 = 1234567 + K, 5
    y, yd = gemm.mm_nn_drop2(x, b, 0.3, seed, row0, bias=bias, relu=relu)
    e = h if h.stride(0) >= K and h.stride(1) == 1 else h.contiguous()
    py, pyd, st = ops._pair_linear_raw(e, pd.to(torch.int32).contiguous(), b, bias, relu, 0.3, seed, row0)
    assert torch.equal(y, want) and torch.equal(py, y) and torch.equal(pyd, yd) and int(st.item()) == 0
    return w, bias, want


@pytest.mark.parametrize('K', [4, 16, 20, 256])
@pytest.mark.parametrize('Nout', [8, 100, 256])
def test_pair_gemm_is_bit_equal_to_the_gemm_on_the_materialised_product(K, Nout):
    gen = torch.Generator().manual_seed(K * 1000 + Nout)
    N = 50
    h = torch.randn(N, K, generator=gen).to(DEV)
    for S in (1, 63, 64, 65, 127, 128, 129, 257):
        _check_pair_gemm(h, _pairs(S, N, gen), K, Nout, gen, relu=bool(S & 1))


@pytest.mark.parametrize('K,Nout', [(20, 100), (256, 256)])
def test_pair_gemm_index_patterns_strided_rows_and_unusable_pairs(K, Nout):
    from gnn_tail_generalization_amd import ops
    import coldbrew_oracle as orc
    gen = torch.Generator().manual_seed(K + Nout)
    N, S = 50, 400
    wide = torch.randn(N, K + 8, generator=gen).to(DEV)
    h = wide[:, 4:4 + K]      # ld = K + 8 > K, rows 16-byte aligned
    assert h.stride(0) == K + 8 and h.data_ptr() % 16 == 0
    pairs = _pairs(S, N, gen, pattern=True)
    w, bias, want = _check_pair_gemm(h, pairs, K, Nout, gen, relu=True)
    # two pairs holding -1 (a failed sampler slot): exactly those rows are NaN, status == 2, every other row bit-equal
    bad = pairs.clone()
    bad[0, 3], bad[1, 3], bad[0, 257], bad[1, 257] = -1, -1, -1, -1
    got, st = ops.pair_linear(h, bad.to(DEV), w, bias, relu=True, fused=True, return_status=True)
    nan_rows = torch.isnan(got).all(1)
    assert int(st.item()) == 2 and nan_rows.nonzero().reshape(-1).tolist() == [3, 257] and not bool(torch.isnan(got[~nan_rows]).any())
    assert torch.equal(got[~nan_rows], want[~nan_rows])
    with pytest.raises(RuntimeError, match='2 pair'):
        ops.pair_linear.check()
    ops.pair_linear.check()      # cleared
    # an endpoint at N is unusable too, and the dropped copy carries the NaN
    bad2 = pairs.clone()
    bad2[1, 0] = N
    py, pyd, st = ops._pair_linear_raw(h, bad2.to(DEV).to(torch.int32).contiguous(), w.t().contiguous(), bias, True, 0.3, 99, 0)
    assert int(st.item()) == 1 and bool(torch.isnan(py[0]).all()) and bool(torch.isnan(pyd[0]).all()) and torch.equal(py[1:], want[1:])
    # the dropped output uses the keep-mask of the host Philox restatement for (seed, row0)
    seed, row0, p = 424242, 11, 0.3
    py, pyd, _ = ops._pair_linear_raw(h, pairs.to(DEV).to(torch.int32).contiguous(), w.t().contiguous(), bias, True, p, seed, row0)
    keep = torch.from_numpy(orc.dropout_keep_mask((S, Nout), p, seed, offset=row0 * Nout)).to(DEV)
    assert torch.equal(pyd, torch.where(keep, py * _keep_scale(p), torch.zeros_like(py)))
    # two calls give identical bits
    again, _ = ops.pair_linear(h, bad.to(DEV), w, bias, relu=True, fused=True, return_status=True)
    assert torch.equal(torch.nan_to_num(again), torch.nan_to_num(got))
    with pytest.raises(RuntimeError):
        ops.pair_check()


def test_pair_linear_outside_the_fused_form_composes_existing_operators():
    from gnn_tail_generalization_amd import _lib, gemm, ops
    gen = torch.Generator().manual_seed(10)
    N, K, Nout, S = 50, 10, 8, 129
    h = torch.randn(N, K, generator=gen).to(DEV)
    w, bias = torch.randn(Nout, K, generator=gen).to(DEV), torch.randn(Nout, generator=gen).to(DEV)
    pairs = _pairs(S, N, gen).to(DEV)
    assert not ops.pair_linear_supported(h, w) and ops.pair_linear_supported(torch.randn(N, 12, device=DEV), torch.randn(8, 12, device=DEV))
    got = ops.pair_linear(h, pairs, w, bias, relu=True)
    assert torch.equal(got, gemm.mm_nn(h[pairs[0]] * h[pairs[1]], w.t().contiguous(), bias=bias, relu=True))
    with pytest.raises(_lib.HipExtensionError, match='fused form'):
        ops.pair_linear(h, pairs, w, bias, fused=True)
    # K = 12 through both paths: the same bits
    h12, w12 = torch.randn(N, 12, generator=gen).to(DEV), torch.randn(Nout, 12, generator=gen).to(DEV)
    assert torch.equal(ops.pair_linear(h12, pairs, w12, bias, fused=True), ops.pair_linear(h12, pairs, w12, bias, fused=False))
    ops.pair_check()


def test_unusable_pairs_in_the_narrow_dropped_copy_and_in_the_weight_gradient():
    """Nout = 8 takes the two-kernel form of the dropped copy: the whole row of an unusable pair is NaN there too.  In the backward such a pair adds
    nothing to dW (relu off, finite upstream gradient): dW is mm_tn on the product with those rows zero, bit for bit."""
    from gnn_tail_generalization_amd import gemm, ops
    gen = torch.Generator().manual_seed(77)
    N, K, Nout, S = 50, 16, 8, 130
    h = torch.randn(N, K, generator=gen).to(DEV)
    w, bias = torch.randn(Nout, K, generator=gen).to(DEV), torch.randn(Nout, generator=gen).to(DEV)
    pairs = _pairs(S, N, gen)
    bad = pairs.clone()
    bad[0, 5], bad[1, 129] = -1, N
    py, pyd, st = ops._pair_linear_raw(h, bad.to(DEV).to(torch.int32).contiguous(), w.t().contiguous(), bias, False, 0.5, 31337, 0)
    assert int(st.item()) == 2
    for out in (py, pyd):
        assert bool(torch.isnan(out[[5, 129]]).all()) and int(torch.isnan(out).any(1).sum()) == 2
    # dW: the unusable pairs' rows of the product are zero
    g = torch.randn(S, Nout, generator=gen).to(DEV)
    wl = w.clone().requires_grad_(True)
    hl = h.clone().requires_grad_(True)
    ops.pair_linear(hl, bad.to(DEV), wl, bias, fused=True).backward(g)      # (a finite upstream gradient on every row)
    keep = lr.usable(bad, N)
    x = (h[pairs[0].to(DEV)] * h[pairs[1].to(DEV)]) * keep.to(DEV)[:, None]
    want = gemm.mm_tn(g, x)
    assert torch.equal(wl.grad, want)
    dh, _ = lr.pair_scatter64(h.cpu(), bad, g.cpu().double() @ w.cpu().double())
    _, sa = lr.pair_scatter64(h.cpu().abs(), bad, g.cpu().double().abs() @ w.cpu().double().abs())
    # dX = g @ W from a three-limb GEMM (8 u sum|terms|), rounded to fp32 (u), then the scatter's float64 sum rounded once
    assert bool(((hl.grad.cpu().double() - dh).abs() <= 2.0 ** -23 * dh.abs() + 10 * U * sa).all())
    with pytest.raises(RuntimeError, match='2 pair'):
        ops.pair_check()


# ---- pair dot and scatter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [4, 10, 256, 300])
def test_pair_dot_and_scatter_against_float64(D):
    from gnn_tail_generalization_amd import ops
    gen = torch.Generator().manual_seed(D)
    N, S = 50, 400
    wide = torch.randn(N, D + 4, generator=gen)
    hc = wide[:, :D]
    hd = wide.to(DEV)[:, :D]      # ld = D + 4
    pairs = _pairs(S, 40, gen, pattern=True)      # nodes 40 .. N - 2 stay untouched (N - 1 is part of the pattern, written as 39 below)
    pairs[pairs == 39] = N - 1
    bad = pairs.clone()
    bad[0, 2], bad[1, 301] = -1, N
    for prs in (pairs, bad):
        pd = prs.to(DEV)
        s, st = ops.pair_dot(hd, pd, return_status=True)
        r = lr.pair_dot64(hc, prs)
        ok = lr.usable(prs, N)
        assert int(st.item()) == int((~ok).sum()) and bool(torch.isnan(s.cpu()[~ok]).all())
        u, v = prs[0].clamp(0, N - 1), prs[1].clamp(0, N - 1)
        sabs = (hc[u].double() * hc[v].double()).abs().sum(-1)
        n = 4 * ((D + 255) // 256) + 6
        gamma = n * U / (1 - n * U)
        assert bool(((s.cpu().double() - r).abs()[ok] <= gamma * sabs[ok]).all())
        assert torch.equal(ops.pair_dot(hd, pd)[ok.to(DEV)], s[ok.to(DEV)])
        for base in (torch.randn(S, generator=gen), torch.randn(S, D + 3, generator=gen)):      # a scalar / a row per pair (ld = D + 3)
            coef, cd = (base, base.to(DEV)) if base.dim() == 1 else (base[:, :D], base.to(DEV)[:, :D])
            want, sa = lr.pair_scatter64(hc, prs, coef)
            p32 = pd.to(torch.int32).contiguous()
            got = ops._pair_scatter_raw(hd, p32, cd)
            err = (got.cpu().double() - want).abs()
            bound = 2.0 ** -23 * want.abs() + 2.0 ** -40 * sa
            assert bool((err <= bound).all()), (D, coef.dim(), float((err - bound).max()))
            touched = torch.zeros(N, dtype=torch.bool)
            touched[prs[:, ok].reshape(-1)] = True
            assert not bool(touched[40:N - 1].any()) and bool((got.cpu()[~touched] == 0).all()) and not bool(torch.isnan(got).any())
            # ldd > D: the padding stays as it was; two calls give identical bits
            out = torch.full((N, D + 5), 7.0, device=DEV)
            again = ops._pair_scatter_raw(hd, p32, cd, out=out[:, :D])
            assert torch.equal(again, got) and bool((out[:, D:] == 7.0).all())
    with pytest.raises(RuntimeError, match='pair'):
        ops.pair_dot.check()
    # autograd: the gradient of sum(s * g) is the scatter with scalar coefficients
    h2 = hd.detach().clone().requires_grad_(True)
    g = torch.randn(S, generator=gen)
    (ops.pair_dot(h2, pairs.to(DEV)) * g.to(DEV)).sum().backward()
    want, sa = lr.pair_scatter64(hc, pairs, g)
    assert bool(((h2.grad.cpu().double() - want).abs() <= 2.0 ** -23 * want.abs() + 2.0 ** -40 * sa).all())
    ops.pair_check()


def test_pair_dot_of_no_pairs_forward_and_backward():
    """S = 0 through the shared launchers: an empty score vector, a zero status, and a gradient of the full shape that is exactly zero."""
    from gnn_tail_generalization_amd import ops
    h = torch.randn(9, 12, generator=torch.Generator().manual_seed(0)).to(DEV).requires_grad_(True)
    s, st = ops.pair_dot(h, torch.zeros((2, 0), dtype=torch.int64, device=DEV), return_status=True)
    assert tuple(s.shape) == (0,) and s.dtype == torch.float32 and int(st.item()) == 0
    s.sum().backward()
    assert tuple(h.grad.shape) == (9, 12) and bool((h.grad == 0).all())
    ops.pair_check()


# ---- predictors -----------------------------------------------------------------------------------------------------------------------
def _absnet(sd, h, pairs, gout):
    """sum|terms| of the output and of every gradient: the float64 network on absolute values, ReLU left out."""
    n = len(sd) // 2
    hh = h.double().abs().requires_grad_(True)
    ps = {k: v.double().abs().requires_grad_(True) for k, v in sd.items()}
    x = hh[pairs[0]] * hh[pairs[1]]
    for i in range(n):
        x = x @ ps[f'lins.{i}.weight'].t() + ps[f'lins.{i}.bias']
    (x * gout.abs()).sum().backward()
    return x.detach(), hh.grad, {k: p.grad for k, p in ps.items()}


@pytest.mark.parametrize('L', [1, 2, 3])
def test_mlp_predictor_against_the_reference_recording(L, pred_rec):
    """score_pairs and its gradients against the float64 run of the reference's MLPPredictor(32, 32, 1, L, .).  Bound per element:
    8 u sum|terms| — what tests/test_gpu_kernels.py::test_gemm_three_limb_error_is_fp32_level allows a three-limb GEMM at any K — with sum|terms|
    taken through the whole network on absolute values, plus (L - 1) times the distance of the reference's own fp32 run to its float64 run as the
    fixture stores it.  From the fixture, the largest bounds are: output 5.4e-7 / 2.1e-6 / 6.4e-6 for L = 1 / 2 / 3 (the fp32 module itself is
    5.2e-8 / 3.2e-8 / 1.8e-8 away), dH 1.2e-6 / 2.8e-6 / 8.9e-6 (fp32 module 5.8e-8 / 6.5e-8 / 1.6e-8), weights and biases 3.6e-6 to 1.4e-4
    (fp32 module 1.0e-7 to 1.2e-6)."""
    from gnn_tail_generalization_amd.Link_prediction_model import MLPPredictor
    m = pred_rec['mlp'][L]
    h, pairs, gout = pred_rec['h'], pred_rec['pairs'], pred_rec['gout']
    a_out, a_dh, a_g = _absnet(m['state_dict'], h, pairs, gout)
    outs = []
    for dropout, train in ((0.5, False), (0.0, True)):      # eval mode, and train mode at dropout 0: the same numbers
        mod = MLPPredictor(32, 32, 1, L, dropout).to(DEV)
        mod.load_state_dict(m['state_dict'])
        mod.train(train)
        hd = h.to(DEV).requires_grad_(True)
        out = mod.score_pairs(hd, pairs.to(DEV))
        assert tuple(out.shape) == (pairs.shape[1], 1)
        (out * gout.to(DEV).float()).sum().backward()
        outs.append(out.detach())

        def check(got, want, scale, ref32, name):
            d = (ref32.double() - want).abs().max().item()
            err = (got.cpu().double() - want).abs()
            bound = 8 * U * scale + (L - 1) * d
            print(f'L {L} {name}: worst error {float(err.max()):.3e}, worst error / bound {float((err / bound).max()):.3f}, fp32 module {d:.3e}')
            assert bool((err <= bound).all()), name
        check(out.detach(), m['out64'], a_out, m['out32'], 'out')
        check(hd.grad, m['dh64'], a_dh, m['dh32'], 'dh')
        for k, p in mod.named_parameters():
            check(p.grad, m['grads64'][k], a_g[k], m['grads32'][k], k)
        # the fused path equals the reference's surface on gathered rows, bit for bit
        with torch.no_grad():
            fwd = mod(h.to(DEV)[pairs[0].to(DEV)], h.to(DEV)[pairs[1].to(DEV)])
        assert torch.equal(fwd, out.detach())
    assert torch.equal(outs[0], outs[1])


def test_mlp_predictor_dropout_uses_the_host_restatement_of_the_keep_mask(pred_rec):
    from gnn_tail_generalization_amd import gemm, ops
    from gnn_tail_generalization_amd.Link_prediction_model import MLPPredictor
    import coldbrew_oracle as orc
    m = pred_rec['mlp'][2]
    h, pairs = pred_rec['h'].to(DEV), pred_rec['pairs'].to(DEV)
    mod = MLPPredictor(32, 32, 1, 2, 0.4).to(DEV).train()
    mod.load_state_dict(m['state_dict'])
    seed = 777
    ops._seed_override.append(seed)
    out = mod.score_pairs(h, pairs)
    assert not ops._seed_override
    l0, l1 = mod.lins
    x1 = gemm.mm_nn(h[pairs[0]] * h[pairs[1]], l0.weight.t().contiguous(), bias=l0.bias, relu=True)
    keep = torch.from_numpy(orc.dropout_keep_mask(tuple(x1.shape), 0.4, seed)).to(DEV)
    xd = torch.where(keep, x1 * _keep_scale(0.4), torch.zeros_like(x1))
    assert torch.equal(out.detach(), gemm.mm_nn(xd, l1.weight.t().contiguous(), bias=l1.bias))
    # the backward regenerates the same mask: dH through the dropped activations against autograd on the composed operators
    hd = h.detach().clone().requires_grad_(True)
    ops._seed_override.append(seed)
    mod.score_pairs(hd, pairs).sum().backward()
    h64 = h.detach().double().requires_grad_(True)
    sd = {k: v.double() for k, v in m['state_dict'].items()}
    z = torch.relu((h64[pairs[0]] * h64[pairs[1]]) @ sd['lins.0.weight'].to(DEV).t() + sd['lins.0.bias'].to(DEV))
    (torch.where(keep, z / (1.0 - 0.4), torch.zeros_like(z)) @ sd['lins.1.weight'].to(DEV).t()).sum().backward()
    # two three-limb GEMMs in a chain, 8 u sum|terms| each, sum|terms| through the network on absolute values and the kept entries' 1 / (1 - p)
    _, a_dh, _ = _absnet(m['state_dict'], pred_rec['h'], pred_rec['pairs'], torch.ones(pairs.shape[1], 1, dtype=torch.float64))
    assert bool(((hd.grad.cpu().double() - h64.grad.cpu()).abs() <= 16 * U * a_dh / (1.0 - 0.4)).all())


def test_dot_predictor_against_the_reference_recording(pred_rec):
    from gnn_tail_generalization_amd.Link_prediction_model import DotPredictor
    h, pairs, g = pred_rec['h'], pred_rec['pairs'], pred_rec['gout'].reshape(-1)
    d = pred_rec['dot']
    mod = DotPredictor().to(DEV)
    hd = h.to(DEV).requires_grad_(True)
    out = mod.score_pairs(hd, pairs.to(DEV))
    (out * g.to(DEV).float()).sum().backward()
    sabs = (h[pairs[0]].double() * h[pairs[1]].double()).abs().sum(-1)
    n = 4 + 6
    assert bool(((out.detach().cpu().double() - d['out64']).abs() <= n * U / (1 - n * U) * sabs).all())
    _, sa = lr.pair_scatter64(h, pairs, g)
    # (the recorded upstream gradient is float64 and reaches the device rounded to fp32: u sum|terms| on top of the scatter's bound)
    assert bool(((hd.grad.cpu().double() - d['dh64']).abs() <= 2.0 ** -23 * d['dh64'].abs() + 2.0 ** -40 * sa + U * sa).all())
    with torch.no_grad():      # the reference's surface: a 32-term fp32 sum in torch's order against the 10-step one of the kernel
        fwd = mod(h.to(DEV)[pairs[0].to(DEV)], h.to(DEV)[pairs[1].to(DEV)])
    assert bool(((fwd.cpu().double() - out.detach().cpu().double()).abs() <= (33 + n) * U * sabs).all())


# ---- trainer --------------------------------------------------------------------------------------------------------------------------
def _trainer(extra, epochs=20, seed=0):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(['--dataset=S-tiny', '--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0',
                                            '--batch_size=4096', '--lr=0.01', '--has_proj2class=1', f'--epochs={epochs}'] + list(extra))
        args.random_seed = seed
        torch.manual_seed(seed)
        np.random.seed(seed)
        t = trainer(args, seed)
    ops.set_graph_seed(None)
    return t


@pytest.mark.parametrize('predictor,loss_func,num_neg', [('MLP', 'log_rank_loss', 3), ('DOT', 'ce_loss', 2)])
def test_training_lowers_the_loss_and_the_metrics_are_in_range(predictor, loss_func, num_neg, tmp_path, monkeypatch):
    """20 epochs on S-tiny.  Every epoch's loss is an estimate over a fresh sample of P (1 + k) pairs, so the first and the last are compared at
    P = 4096 (sampling noise of the mean about 3e-4, as the flat stretches show) and at lr = 0.01.  The teacher starts with embeddings of size 0.1,
    whose products are 0.01: the loss then sits at ln 2 (2 ln 2 for ce_loss) for a number of steps that depends on the initial weights before it
    falls — measured with the MLP and log_rank_loss at this lr and P: 0.6938 -> 0.6671 over 20 epochs under one seed and 0.6933 -> 0.6936 under
    another at the 4-wide embedding (the class logits), 0.6932 -> 0.6143 with the fall from epoch 6 on at the 128-wide one.  The test therefore
    trains the 128-wide embedding (--has_proj2class=1), which also takes the fused first layer at K = 128; at the default lr = 0.001 and 65 536
    positives 20 epochs end inside the plateau (0.6933 -> 0.6933)."""
    monkeypatch.chdir(tmp_path)
    t = _trainer([f'--predictor={predictor}', f'--loss_func={loss_func}', f'--num_neg={num_neg}'])
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(0)
        losses, metrics = t.train_teacherGNN_linkpred()
    print(predictor, loss_func, 'loss by epoch', np.round(losses, 4).tolist(), metrics)
    assert losses.shape == (20,) and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert set(metrics) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and all(0.0 <= v <= 1.0 for v in metrics.values())
    assert type(t.predictor).__name__ == ('MLPPredictor' if predictor == 'MLP' else 'DotPredictor')
    if predictor == 'MLP':
        assert all(p.grad is not None for p in t.predictor.parameters())
    # the gradient reaches the teacher through score_pairs -> res.commonEmb
    moved = [float(p.grad.abs().max()) for p in t.teacherGNN.parameters() if p.grad is not None]
    assert moved and max(moved) > 0 and all(np.isfinite(moved))


def test_check_raises_on_a_failed_slot_and_odd_counts_are_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    t = _trainer(['--predictor=DOT', '--loss_func=AUC', '--num_neg=3'], epochs=1)
    with contextlib.redirect_stdout(io.StringIO()):
        t.setup_teacherGNN_linkpred()
    real = t.gen_linkpred_edge_index

    def with_failed_slot(mode):
        pos, neg = real(mode)
        neg = neg.clone()
        neg[:, 4:6] = -1      # what a negative slot that found no pair writes
        return pos, neg
    monkeypatch.setattr(t, 'gen_linkpred_edge_index', with_failed_slot)
    with pytest.raises(RuntimeError, match='2 pair'):
        t.run_trainSet_linkpred()
    monkeypatch.setattr(t, 'gen_linkpred_edge_index', real)
    t.args.batch_size = 255      # 255 * 3 is odd
    with pytest.raises(ValueError, match='even'):
        t.training_loss_linkpred()
    # the refusals of the node-classification entry points stay
    t.args.has_loss_component_edgewise = True
    with pytest.raises(NotImplementedError, match='I2_GTL'):
        t.run_trainSet()


def test_tool_end_to_end(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkpred
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkpred.main(['--dataset=S-tiny', '--predictor=MLP', '--loss_func=log_rank_loss', '--num_neg=3', '--epochs=3', '--batch_size=128',
                                    '--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1'])
    assert len(recs) == 1 and recs[0][0].shape == (3,) and np.isfinite(recs[0][0]).all() and 0.0 <= recs[0][1]['AUC'] <= 1.0
