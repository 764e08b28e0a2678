"""The student MLP's row kernels, its part-1 loss and its part-2 input (csrc/cb_mlp.hip through ops.py) against the float64
restatement of tests/student_ref.py with the product's keep masks injected.

Tolerance (the project's form for kernels measured against torch's own float32, tests/test_gpu_kernels.py:341-350): on the same
inputs the error of torch's float32 composition (F.layer_norm -> F.gelu -> mask, and its autograd) against float64 is err32; the
kernel's error must satisfy err <= max(2 * err32, 8 * 2^-24), both relative to the largest magnitude of the compared tensor's row
(factor 2: another, equally valid summation order; the floor keeps the check meaningful where torch happens to be exact).
Every figure is printed before it is asserted (run with -s to collect them; profiles/student_mlp.md holds a recorded run)."""
import pytest
import torch

import student_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

WIDTHS = [256, 194, 386, 20, 1]
ROWS = [1, 63, 65537]
MODES = [('train', 0.0), ('train', 0.2), ('eval', 0.2)]


def _inputs(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, d, generator=g) * 1.5 + 0.3
    gamma = 1.0 + 0.2 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g)
    return z, gamma, beta, dy


def _run(fn, z, gamma, beta, dy):
    z, gamma, beta = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    out = fn(z, gamma, beta)
    out.backward(dy)
    return out.detach(), z.grad, gamma.grad, beta.grad


@pytest.mark.parametrize('mode,p', MODES)
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('d', WIDTHS)
def test_ln_gelu_dropout_forward_backward(d, rows, mode, p):
    from gnn_tail_generalization_amd import ops
    training = mode == 'train'
    z, gamma, beta, dy = _inputs(rows, d, 1000 * d + rows)
    seed = 12345 + d
    active = training and p > 0
    keep = ops.dropout_keep_mask((rows, d), p, seed, DEV).cpu() if active else None
    dev = [t.to(DEV) for t in (z, gamma, beta, dy)]
    got = _run(lambda a, b, c: ops.ln_gelu_dropout(a, b, c, 1e-5, p, training, seed=seed), *dev)
    ref = _run(lambda a, b, c: sr.ln_gelu_drop(a, b, c, 1e-5, keep, p), *(t.double() for t in (z, gamma, beta, dy)))
    keep_dev = keep.to(DEV) if keep is not None else None
    t32 = _run(lambda a, b, c: sr.ln_gelu_drop(a, b, c, 1e-5, keep_dev, p), *dev)
    if active:      # the regenerated mask IS ops.dropout_keep_mask's: zero exactly where the mask drops
        # (float32 erf saturates at -1 below u ~ -5.5, where gelu is exactly 0 on its own: such elements say nothing about the mask)
        o = got[0].cpu()
        assert not bool((o[~keep] != 0).any())
        live = sr.ln_gelu_drop(z.double(), gamma.double(), beta.double(), 1e-5).abs() > 1e-5
        assert torch.equal((o != 0)[live], keep[live])
    bad = []
    for name, a, b32, r in zip(('out', 'dz', 'dgamma', 'dbeta'), got, t32, ref):
        err, err32 = sr.rel_err(a, r), sr.rel_err(b32, r)
        print(f'ln_gelu_drop d={d} rows={rows} {mode} p={p} {name}: err={err / sr.EPS24:.2f} err32={err32 / sr.EPS24:.2f} (x 2^-24)')
        if not sr.within(err, err32):
            bad.append((name, err / sr.EPS24, err32 / sr.EPS24))
    assert not bad, bad


@pytest.mark.parametrize('d', WIDTHS)
def test_linear_group_bias_gradient_and_bitwise_repeat(d):
    """The fused group's backward: colsum(dz) is the Linear's bias gradient; dgamma, dbeta and the bias gradient are bitwise equal across
    two calls (fixed-order column sums, no atomics)."""
    from gnn_tail_generalization_amd import ops
    rows, k, p, seed = 4099, 24, 0.2, 77
    g = torch.Generator().manual_seed(d)
    x, w, b = torch.randn(rows, k, generator=g), torch.randn(d, k, generator=g) / 5, torch.randn(d, generator=g)
    _, gamma, beta, dy = _inputs(rows, d, d + 5)
    keep = ops.dropout_keep_mask((rows, d), p, seed, DEV).cpu()

    def run(dtype, device, fn):
        ts = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in (x, w, b, gamma, beta)]
        out = fn(*ts)
        out.backward(dy.to(device=device, dtype=dtype))
        return [out.detach()] + [t.grad for t in ts]

    prod = lambda x_, w_, b_, ga, be: ops.linear_ln_gelu_dropout(x_, w_, b_, ga, be, 1e-5, p, True, seed=seed)   # noqa: E731
    a, a2 = run(torch.float32, DEV, prod), run(torch.float32, DEV, prod)
    for u, v in zip(a, a2):
        assert torch.equal(u, v)
    ref = run(torch.float64, 'cpu', lambda x_, w_, b_, ga, be: sr.ln_gelu_drop(torch.nn.functional.linear(x_, w_, b_), ga, be, 1e-5, keep, p))
    kd = keep.to(DEV)
    t32 = run(torch.float32, DEV, lambda x_, w_, b_, ga, be: sr.ln_gelu_drop(torch.nn.functional.linear(x_, w_, b_), ga, be, 1e-5, kd, p))
    bad = []
    for name, u, v, r in zip(('out', 'dx', 'dw', 'dbias', 'dgamma', 'dbeta'), a, t32, ref):
        err, err32 = sr.rel_err(u, r), sr.rel_err(v, r)
        print(f'linear group d={d} {name}: err={err / sr.EPS24:.2f} err32={err32 / sr.EPS24:.2f} (x 2^-24)')
        if not sr.within(err, err32):
            bad.append((name, err / sr.EPS24, err32 / sr.EPS24))
    assert not bad, bad


@pytest.mark.parametrize('B,D,N', [(1, 1, 3), (63, 20, 40), (4097, 36, 500), (65537, 256, 3000), (129, 771, 200)])
def test_mse_rows(B, D, N):
    from gnn_tail_generalization_amd import ops
    g = torch.Generator().manual_seed(B + D)
    pred, target = torch.randn(B, D, generator=g), torch.randn(N, D, generator=g)
    idx = torch.randint(0, N, (B,), generator=g)
    pd = pred.to(DEV).requires_grad_(True)
    loss = ops.mse_rows(pd, target.to(DEV), idx.to(DEV))
    loss.backward()
    loss2 = ops.mse_rows(pd.detach(), target.to(DEV), idx.to(DEV))
    assert torch.equal(loss.detach(), loss2)
    p64 = pred.double().requires_grad_(True)
    ref = torch.nn.functional.mse_loss(p64, target.double()[idx])
    ref.backward()
    p32 = pred.to(DEV).requires_grad_(True)
    l32 = torch.nn.functional.mse_loss(p32, target.to(DEV)[idx.to(DEV)])
    l32.backward()
    bad = []
    for name, u, v, r in (('loss', loss, l32, ref), ('grad', pd.grad, p32.grad, p64.grad)):
        err, err32 = sr.rel_err(u, r), sr.rel_err(v, r)
        print(f'mse_rows B={B} D={D} {name}: err={err / sr.EPS24:.2f} err32={err32 / sr.EPS24:.2f} (x 2^-24)')
        if not sr.within(err, err32):
            bad.append((name, err / sr.EPS24, err32 / sr.EPS24))
    assert not bad, bad


@pytest.mark.parametrize('B,F,D,N,K', [(1, 3, 5, 9, 2), (63, 20, 36, 120, 2), (4097, 128, 72, 900, 3), (300, 7, 33, 64, 8)])
def test_part2_input_and_alpha_gradients(B, F, D, N, K):
    from gnn_tail_generalization_amd import ops
    g = torch.Generator().manual_seed(B + F + D)
    x, p1, se = torch.randn(B, F, generator=g), torch.randn(B, D, generator=g), torch.randn(N, D, generator=g)
    al = torch.tensor([0.7, -1.3])
    gout = torch.randn(B, F + 2 * D, generator=g)
    ad = al.to(DEV).requires_grad_(True)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.semlp_part2_input(ad, xd, p1.to(DEV), se.to(DEV), K)
    out.backward(gout.to(DEV))
    assert xd.grad is None
    rep_dev = ops.se_topk_replace(out[:, F + D:].detach(), se.to(DEV), K)      # the very call the assembly makes
    # the assembled matrix, block by block: x verbatim, the replacement kernel's rows times alpha1, the guess times alpha0 (float32 products)
    assert torch.equal(out[:, :F].detach().cpu(), x)
    assert torch.equal(out[:, F + D:].detach().cpu(), (p1 * al[0]))
    torch.testing.assert_close(out[:, F:F + D].detach(), rep_dev * ad.detach()[1], rtol=0, atol=0)
    a64 = al.double().requires_grad_(True)
    guess = p1.double() * a64[0]
    rep, _, _ = sr.replacement(guess.detach(), se.double(), K)
    ref = torch.cat([x.double(), rep * a64[1], guess], -1)
    ref.backward(gout.double())
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), atol=1e-4, rtol=1e-4)      # (the replacement kernel's own bound)
    # float32 composition on the device from the kernel's replacement rows
    a32 = al.to(DEV).requires_grad_(True)
    t32 = torch.cat([x.to(DEV), rep_dev * a32[1], p1.to(DEV) * a32[0]], -1)
    t32.backward(gout.to(DEV))
    r64 = al.double().requires_grad_(True)
    torch.cat([x.double(), rep_dev.cpu().double() * r64[1], p1.double() * r64[0]], -1).backward(gout.double())
    err, err32 = sr.rel_err(ad.grad, r64.grad), sr.rel_err(a32.grad, r64.grad)
    print(f'part2 input B={B} F={F} D={D} dalphas: err={err / sr.EPS24:.2f} err32={err32 / sr.EPS24:.2f} (x 2^-24)')
    assert sr.within(err, err32), (err / sr.EPS24, err32 / sr.EPS24)
    torch.testing.assert_close(ad.grad.cpu().double(), a64.grad, atol=1e-4 * float(gout.abs().sum()) / B, rtol=1e-3)
