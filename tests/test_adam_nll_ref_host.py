"""Host: the restatement of tests/adam_nll_ref.py against torch in float64, and — on the inputs of EVERY case of tests/test_gpu_adam_nll.py — its float32
evaluation inside the bounds that file asserts of the kernels: the bounds can be met by a correct float32 evaluation of the same formulas."""
import math

import pytest
import torch
import torch.nn.functional as F

import adam_nll_ref as ar


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def _torch_adam(p, g, m, v, t, lr, b1, b2, eps, wd):
    """One torch.optim.Adam step number t from the given state, in float64."""
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[q] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
    q.grad = g.clone()
    opt.step()
    return q.detach(), opt.state[q]['exp_avg'], opt.state[q]['exp_avg_sq']


def test_adam_restatement_is_torch_adam():
    """Hyper-parameters that float32 holds exactly and whose bias corrections it holds exactly too (t = 1: bc1 = 1/8, sqrt(bc2) = 1/4), so that the
    restatement's float32 roundings change nothing: 1e-12 relative, weight_decay > 0, a warm state."""
    h = dict(lr=2.0 ** -7, b1=0.875, b2=0.9375, eps=2.0 ** -27, wd=2.0 ** -11)
    p, g, m, v = (x.double() for x in ar.adam_inputs('warm', 4099))
    mine = ar.adam_step(p, g, m, v, 1, **h)
    ref = _torch_adam(p, g, m, v, 1, **h)
    for a, b in zip(mine, ref):
        assert _rel(a, b) <= 1e-12


@pytest.mark.parametrize('t', ar.ADAM_STEPS)
def test_adam_restatement_with_the_kernel_constants_is_torch_adam_to_float32_rounding(t):
    """The constants of the GPU cases (0.01, 0.9, 0.999, 1e-8, 5e-4): torch is given their float32 roundings; what is left is the float32 rounding of the
    two bias corrections, each 2^-24 relative in the update p' - p (m', v' do not see them)."""
    h = {k: float(torch.tensor(x, dtype=torch.float32)) for k, x in ar.ADAM_HYPER.items()}
    p, g, m, v = (x.double() for x in ar.adam_inputs('warm', 1023))
    mine = ar.adam_step(p, g, m, v, t, **h)
    ref = _torch_adam(p, g, m, v, t, **h)
    assert _rel(mine[1], ref[1]) <= 1e-12 and _rel(mine[2], ref[2]) <= 1e-12
    assert _rel(mine[0] - p, ref[0] - p) <= 2.0 ** -22


def test_adam_extra_decay_counts_only_when_finite():
    p, g, m, v = (x.double() for x in ar.adam_inputs('warm', 257))
    h = ar.ADAM_HYPER
    base = ar.adam_step(p, g, m, v, 3, **h)
    for extra in (math.inf, -math.inf, math.nan):
        assert all(torch.equal(a, b) for a, b in zip(ar.adam_step(p, g, m, v, 3, extra=extra, **h), base))
    h2 = dict(h, wd=float(torch.tensor(h['wd'], dtype=torch.float32) + torch.tensor(0.25, dtype=torch.float32).double()))
    with_extra = ar.adam_step(p, g, m, v, 3, extra=0.25, **h)
    assert not torch.equal(with_extra[0], base[0])
    assert _rel(with_extra[0], ar.adam_step(p, g, m, v, 3, **h2)[0]) <= 1e-7      # (h2's wd is rounded to float32 once more)


@pytest.mark.parametrize('family', ['randn3', 'randn1e4', 'shift3e4', 'equal', 'dominant', 'neginf30', 'tiny'])
@pytest.mark.parametrize('rows,C', [(1, 2), (300, 7), (513, 40), (70, 128)])
def test_nll_restatement_is_torch_nll(rows, C, family):
    """F.nll_loss(F.log_softmax(z[mask], 1), y[mask]) and its autograd, float64, 1e-12 relative.  The restatement multiplies by the kernel's
    float32(1 / float32(count)) where torch divides by count: the exact factor count * inv is taken out."""
    z, y = ar.nll_inputs(rows, C, family)
    for kind in ('none', 'some', 'one'):
        mask, count = ar.nll_mask(rows, kind)
        sel = torch.ones(rows, dtype=torch.bool) if mask is None else mask
        zt = z.double().requires_grad_(True)
        ref = F.nll_loss(F.log_softmax(zt[sel], 1), y[sel])
        ref.backward()
        inv = float(torch.tensor(1.0) / torch.tensor(float(count)))
        loss, grad = ar.nll(z.double(), y, mask, count)
        k = count * inv
        # (relative to the operands of lse - z[y], not to a difference that may cancel: torch subtracts in another order)
        zs = z.double()[sel]
        scale = abs(float(ref.detach())) + float(zs[torch.isfinite(zs)].abs().max())
        assert abs(float(loss) - k * float(ref.detach())) <= 1e-12 * scale
        assert float((grad - k * zt.grad).abs().max()) <= 1e-12 * float(zt.grad.abs().max())


def test_nll_restatement_ignores_unmasked_labels_and_poisons_bad_masked_ones():
    z, y = ar.nll_inputs(300, 7, 'randn3')
    mask, count = ar.nll_mask(300, 'some')
    base = ar.nll(z.double(), y, mask, count)
    junk = y.clone()
    junk[~mask] = torch.tensor([-1, 7, 2 ** 40])[torch.arange(int((~mask).sum())) % 3]
    assert all(torch.equal(a, b) for a, b in zip(ar.nll(z.double(), junk, mask, count), base))
    bad = y.clone()
    rows = torch.nonzero(mask).flatten()[[1, 5]]
    bad[rows] = torch.tensor([-1, 7])
    loss, grad = ar.nll(z.double(), bad, mask, count)
    assert math.isnan(float(loss))
    nan_rows = torch.isnan(grad).any(1)
    assert torch.equal(torch.nonzero(nan_rows).flatten(), rows) and bool(torch.isnan(grad[rows]).all())
    assert torch.equal(grad[~nan_rows], base[1][~nan_rows])


@pytest.mark.parametrize('family', ar.NLL_FAMILIES)
@pytest.mark.parametrize('rows,C', ar.NLL_SHAPES)
def test_float32_nll_sits_inside_the_bounds_of_every_gpu_case(rows, C, family):
    for kind in ar.NLL_MASKS:
        c = ar.nll_case(rows, C, family, kind)
        assert ar.same_specials(c['grad32'], c['grad64']) and ar.same_specials(c['loss32'], c['loss64'])
        if kind == 'empty':
            assert float(c['loss64']) == 0.0 and float(c['loss32']) == 0.0 and not bool(c['grad32'].any())
        if c['B'] is not None:
            err = abs(float(c['loss32']) - float(c['loss64']))
            print(f'{rows}x{C} {family} {kind}: |loss32 - loss64| = {err:.3e}, B = {c["B"]:.3e}, ratio = {err / max(c["B"], 1e-300):.3f}')
            assert err <= c['B']
        else:
            assert family == 'infrows' and math.isnan(float(c['loss64']))
        # the yardstick itself is a tight one: the float32 restatement is within a few roundings of the reference at the scale of softmax / count (the
        # subtraction of the one-hot may cancel below it), down to the spacing of the float32 denormals
        assert ar.max_err(c['grad32'], c['grad64']) <= 2.0 ** -24 * (C + 8) / max(c['count'], 1) + 2.0 ** -126


@pytest.mark.parametrize('t', ar.ADAM_STEPS)
@pytest.mark.parametrize('n', ar.ADAM_SIZES)
def test_float32_adam_is_finite_and_close_on_every_gpu_case(n, t):
    """No case leaves the normal float32 range, and the yardstick 4 * e32 + 2^-22 max|T| is not a loose one: e32 itself is a few roundings of max|T|."""
    for family in ar.ADAM_FAMILIES:
        c = ar.adam_case(family, n, t)
        for name, r64, r32 in zip('pmv', c['r64'], c['r32']):
            assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), (family, name)
            top = float(r64.abs().max())
            e32 = ar.max_err(r32, r64)
            assert e32 <= 2.0 ** -21 * top + 1e-300, (family, name, e32, top)
            nz = r32[r32 != 0]
            assert nz.numel() == 0 or float(nz.abs().min()) >= 2.0 ** -126, (family, name)      # no float32 denormal among the results
        if family == 'gzero':      # the update is driven by wd * p alone
            assert bool((c['r64'][0] != c['p'].double()).all())


@pytest.mark.parametrize('scale', ar.NORM_SCALES)
@pytest.mark.parametrize('n', ar.NORM_SIZES)
def test_float32_sum_of_squares_sits_inside_the_norm_bound(n, scale):
    x = ar.norm_input(n, scale)
    nrm64, sq64 = ar.sumsq_norm(x.double())
    nrm32, sq32 = ar.sumsq_norm(x)
    assert n == 0 or float((x * x).min()) >= 2.0 ** -126
    assert math.isfinite(float(sq32))
    b_n, b_sq = ar.norm_rel_bounds(n, ar.grid_for(-(-n // 4)) if n else 0)
    assert abs(float(sq32) - float(sq64)) <= b_sq * float(sq64)
    assert abs(float(nrm32) - float(nrm64)) <= b_n * float(nrm64)
