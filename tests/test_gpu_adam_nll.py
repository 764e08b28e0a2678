"""GPU: the three kernels that end every training step (csrc/cb_reduce.hip) — the fused log-softmax + NLL loss, the fused multi-tensor Adam and the
Frobenius norm it leaves behind — against the float64 restatement of tests/adam_nll_ref.py, at the edges of their launch shapes and inputs.

Tensors (gradient, p, m, v) are held to the project's yardstick (tests/test_gpu_attn.py), per tensor:
    max |T_gpu - T_64|  <=  4 * max |T_cpu32 - T_64|  +  2^-22 * max |T_64|
the scalar loss to the derived bound of adam_nll_ref.nll_loss_bound, the norm pair to adam_nll_ref.norm_rel_bounds; NaN / Inf must sit where the float64
reference has them.  tests/test_adam_nll_ref_host.py shows on the same inputs that a correct float32 evaluation meets these bounds.  Where the header
promises the same bits (vector and scalar NLL kernel, aligned and unaligned Adam, single and multi-tensor Adam, the norm by-product of the largest
tensor of a launch) the assertion is torch.equal.  No hipGraph anywhere: the device-resident step count is reached through the C ABI."""
import ctypes
import math

import pytest
import torch

import adam_nll_ref as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 12345.0
H = ar.ADAM_HYPER


def _libs():
    from gnn_tail_generalization_amd import _lib
    return _lib, _lib.load()


def _status_ok():
    _lib, lib = _libs()
    torch.cuda.synchronize()
    assert lib.cb_device_status() == 0


def _check(name, got, r64, r32):
    """The yardstick on one tensor; prints err, err32 and their ratio first."""
    assert ar.same_specials(got, r64), name
    err, e32, bnd = ar.max_err(got, r64), ar.max_err(r32, r64), ar.bound(r64, r32)
    print(f'{name}: err = {err:.3e}, err32 = {e32:.3e}, err / err32 = {err / max(e32, 1e-300):.3g}, err / bound = {err / max(bnd, 1e-300):.3f}')
    assert err <= bnd, (name, err, bnd)


def _place(x, off):
    """x copied to elements [off, off + n) of a sentinel-filled device buffer whose start is 16-byte aligned: off = 4 keeps the alignment, off = 5 is
    one float past it.  (buffer, view)."""
    n = x.numel()
    buf = torch.full((n + 16,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n]
    view.copy_(x)
    return buf, view


def _sentinels_kept(buf, off, n):
    return bool((buf[:off] == SENTINEL).all()) and bool((buf[off + n:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# log-softmax + NLL
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _nll(z, ld, y, mask, rows, C, count, want_grad=True):
    """cb_nll_logsoftmax_f32 on device tensors: z is whatever tensor starts at the first logit (row stride ld floats).  (loss [1], grad [rows, C] or None)."""
    _lib, lib = _libs()
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=DEV)
    grad = torch.full((rows, C), SENTINEL, dtype=torch.float32, device=DEV) if want_grad else None
    wsb = lib.cb_reduce_workspace_bytes()
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    m8 = mask.view(torch.uint8) if mask is not None else None
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_nll_logsoftmax_f32(_lib.ptr(z), ld, _lib.ptr(y), _lib.ptr(m8), rows, C, int(count), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), wsb,
                                             _lib.stream_ptr()), 'cb_nll_logsoftmax_f32')
    return loss, grad


def _dev(t):
    return t.to(DEV) if t is not None else None


def _scalar_path_views(z):
    """The same logits where the vector kernels cannot run: as the first C columns of a [rows, C + 1] matrix (ld % 4 == 1), and contiguous but starting
    one float past a 16-byte boundary.  [(tensor at the first logit, ld)]; the owners are kept alive by the views."""
    rows, C = z.shape
    wide = torch.full((rows, C + 1), SENTINEL, dtype=torch.float32, device=DEV)
    wide[:, :C] = z
    buf = torch.full((rows * C + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    shifted = buf[1:1 + rows * C]
    shifted.copy_(z.reshape(-1))
    return [(wide, C + 1), (shifted, C)]


@pytest.mark.parametrize('family', ar.NLL_FAMILIES)
@pytest.mark.parametrize('rows,C', ar.NLL_SHAPES, ids=[f'{r}x{c}' for r, c in ar.NLL_SHAPES])
def test_nll_loss_and_gradient_against_float64(rows, C, family):
    """Every mask of one (shape, input family): the loss inside its derived bound (NaN where the reference is NaN, exactly 0 under the empty mask), the
    gradient inside the yardstick with its NaN rows in place; the loss has the same bits when no gradient is wanted, and ops.nll_logsoftmax is that call."""
    from gnn_tail_generalization_amd import ops
    for kind in ar.NLL_MASKS:
        c = ar.nll_case(rows, C, family, kind)
        z, y, mask = _dev(c['z']), _dev(c['y']), _dev(c['mask'])
        loss, grad = _nll(z, C, y, mask, rows, C, c['count'])
        name = f'nll {rows}x{C} {family} mask={kind}'
        got = float(loss[0])
        if c['B'] is None:
            assert math.isnan(float(c['loss64'])) and math.isnan(got), name
        else:
            err = abs(got - float(c['loss64']))
            print(f'{name}: loss err = {err:.3e}, B = {c["B"]:.3e}, err / B = {err / max(c["B"], 1e-300):.3f}')
            assert err <= c['B'], (name, err, c['B'])
        if kind == 'empty':
            assert got == 0.0 and not bool(grad.any()), name
        _check(name + ' grad', grad, c['grad64'], c['grad32'])
        loss_only, _ = _nll(z, C, y, mask, rows, C, c['count'], want_grad=False)
        assert torch.equal(loss_only.view(torch.int32), loss.view(torch.int32)), name
        zg = z.clone().requires_grad_(True)
        l_ops = ops.nll_logsoftmax(zg, y, mask, c['count'], unit_grad=True)
        l_ops.backward()
        assert torch.equal(l_ops.detach().reshape(1).view(torch.int32), loss.view(torch.int32)) and torch.equal(zg.grad.view(torch.int32), grad.view(torch.int32)), name
    _status_ok()


@pytest.mark.parametrize('family', ['randn3', 'randn1e4', 'dominant', 'neginf30', 'infrows'])
@pytest.mark.parametrize('C', ar.NLL_VEC_C)
def test_nll_vector_and_scalar_kernels_give_the_same_bits(C, family):
    """k_nll_fused_v4 (contiguous, aligned) and k_nll_fused (ld % 4 != 0; base one float off) on the same logits: "the same arithmetic, expression for
    expression"."""
    rows = 301
    z, y = ar.nll_inputs(rows, C, family)
    for kind in ('none', 'some'):
        mask, count = ar.nll_mask(rows, kind)
        zd, yd, md = _dev(z), _dev(y), _dev(mask)
        loss_v, grad_v = _nll(zd, C, yd, md, rows, C, count)
        for view, ld in _scalar_path_views(zd):
            loss_s, grad_s = _nll(view, ld, yd, md, rows, C, count)
            assert torch.equal(loss_s.view(torch.int32), loss_v.view(torch.int32)), (C, family, kind, ld)
            assert torch.equal(grad_s.view(torch.int32), grad_v.view(torch.int32)), (C, family, kind, ld)
    _status_ok()


@pytest.mark.parametrize('C', [7, 40])
def test_nll_never_reads_the_labels_of_rows_outside_the_mask(C):
    """Unlabeled nodes carry -1; C and 2^40 are no better.  Bit-equal to the run with valid labels there."""
    rows = 300
    z, y = ar.nll_inputs(rows, C, 'randn3')
    mask, count = ar.nll_mask(rows, 'some')
    junk = y.clone()
    junk[~mask] = torch.tensor([-1, C, 2 ** 40])[torch.arange(int((~mask).sum())) % 3]
    zd, md = _dev(z), _dev(mask)
    loss_a, grad_a = _nll(zd, C, _dev(y), md, rows, C, count)
    loss_b, grad_b = _nll(zd, C, _dev(junk), md, rows, C, count)
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)
    assert bool(torch.isfinite(loss_a).all()) and bool(torch.isfinite(grad_a).all())
    _status_ok()


@pytest.mark.parametrize('C,scalar', [(4, False), (8, False), (40, False), (48, False), (64, False), (7, True), (47, True), (40, True)])
def test_nll_label_outside_the_classes_on_a_masked_row_is_a_nan_row(C, scalar):
    """A label outside [0, C) on a row that counts is never an index and never narrowed: the loss is NaN, exactly those gradient rows are NaN, every other
    row has the bits of the run in which the bad rows do not count.  (Before the range check the scalar kernel read z[r][label], the vector kernels took
    2^32 + 3 for class 3 and let -1 or C contribute lse - 0: a finite loss, which this test rejects.)  The bad labels are -1, -2, C, C + 1 on interior rows
    of a 64-row matrix; 2^32 + 3 only where the vector kernel runs, which compares the label and never forms an address from it."""
    rows = 64
    z, y = ar.nll_inputs(rows, C, 'randn3')
    mask, _ = ar.nll_mask(rows, 'some')
    bad_rows = [20, 21, 33, 40] + ([45] if not scalar else [])
    bad_labels = [-1, -2, C, C + 1] + ([2 ** 32 + 3] if not scalar else [])
    mask[bad_rows] = True
    count = int(mask.sum())
    bad = y.clone()
    bad[bad_rows] = torch.tensor(bad_labels)
    without = mask.clone()
    without[bad_rows] = False
    zd = _dev(z)
    view, ld = (_scalar_path_views(zd)[0] if scalar and C % 4 == 0 else (zd, C))
    loss_ref, grad_ref = _nll(view, ld, _dev(y), _dev(without), rows, C, count)
    loss, grad = _nll(view, ld, _dev(bad), _dev(mask), rows, C, count)
    assert bool(torch.isfinite(loss_ref).all()) and bool(torch.isnan(loss).all())
    nan_rows = torch.isnan(grad).any(1).cpu()
    assert torch.equal(torch.nonzero(nan_rows).flatten(), torch.tensor(bad_rows)) and bool(torch.isnan(grad[bad_rows]).all())
    keep = _dev(~nan_rows)
    assert torch.equal(grad[keep], grad_ref[keep]) and not bool(grad_ref[bad_rows].any())
    # the restatement says the same
    l64, g64 = ar.nll(z.double(), bad, mask, count)
    assert math.isnan(float(l64)) and ar.same_specials(grad, g64)
    _status_ok()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _arr(vals, ty=ctypes.c_void_p):
    return (ty * len(vals))(*vals)


def _p(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _adam_multi(tensors, t, extras=None, norms=None, step_dev=None, guard=None):
    """cb_adam_multi_norm_f32 on [(p, g, m, v)] device views (updated in place).  extras: per tensor a [1] device tensor or None; norms: per tensor True
    to ask for the norm pair.  Returns the list of [2] device tensors (None where not asked)."""
    _lib, lib = _libs()
    k = len(tensors)
    outs = [torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV) if norms and norms[i] else None for i in range(k)]
    n_norms = sum(o is not None for o in outs)
    wsb = lib.cb_adam_norm_workspace_bytes(n_norms)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_adam_multi_norm_f32(k, _arr([_p(x[0]) for x in tensors]), _arr([_p(x[1]) for x in tensors]), _arr([_p(x[2]) for x in tensors]),
                                              _arr([_p(x[3]) for x in tensors]), _arr([x[0].numel() if x[0] is not None else 0 for x in tensors], ctypes.c_int64),
                                              _arr([e.data_ptr() if e is not None else None for e in extras]) if extras else None,
                                              _arr([o.data_ptr() if o is not None else None for o in outs]) if n_norms else None,
                                              H['lr'], H['b1'], H['b2'], H['eps'], H['wd'], 0 if step_dev is not None else t, _lib.ptr(step_dev), _lib.ptr(guard),
                                              _lib.ptr(ws) if n_norms else None, wsb, _lib.stream_ptr()), 'cb_adam_multi_norm_f32')
    return outs


def _adam_single(p, g, m, v, t, step_dev=None):
    _lib, lib = _libs()
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_adam_step_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), H['lr'], H['b1'], H['b2'], H['eps'], H['wd'], 0 if step_dev is not None else t,
                                        _lib.ptr(step_dev), _lib.stream_ptr()), 'cb_adam_step_f32')


def _frobenius(x):
    """cb_frobenius_norm_f32 of a device view: the [2] pair."""
    _lib, lib = _libs()
    out2 = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEV)
    wsb = lib.cb_reduce_workspace_bytes()
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_frobenius_norm_f32(_p(x), x.numel(), _lib.ptr(out2), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_frobenius_norm_f32')
    return out2


def _check_norm(name, out2, x, nb):
    """The pair {||x||, ||x||^2} a launch of nb blocks left for the float32 device values x, against their float64 sum of squares."""
    n = x.numel()
    sq64 = float((x.double() * x.double()).sum()) if n else 0.0
    b_n, b_sq = ar.norm_rel_bounds(n, nb)
    got = out2.double().cpu()
    if sq64 == 0.0:
        assert float(got[0]) == 0.0 and float(got[1]) == 0.0, name
        return
    r_sq, r_n = abs(float(got[1]) - sq64) / sq64, abs(float(got[0]) - math.sqrt(sq64)) / math.sqrt(sq64)
    print(f'{name}: ||x||^2 rel err = {r_sq:.3e} ({r_sq / b_sq:.3f} of its bound), ||x|| rel err = {r_n:.3e} ({r_n / b_n:.3f} of its bound)')
    assert r_sq <= b_sq and r_n <= b_n, (name, r_sq, b_sq, r_n, b_n)


def _eq(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize('t', ar.ADAM_STEPS)
@pytest.mark.parametrize('n', ar.ADAM_SIZES)
def test_adam_one_step_against_float64(n, t):
    """One step from the prescribed state of every family, one launch for all six (each tensor at its own scale against its own reference): the yardstick;
    cb_adam_step_f32 on the same inputs: the same bits; each of p / g / m / v in turn one float off 16-byte alignment (the scalar path): the same bits;
    the floats before and after every tensor keep their sentinel."""
    cases = [ar.adam_case(f, n, t) for f in ar.ADAM_FAMILIES]
    dev_in = [tuple(c[k].to(DEV) for k in 'pgmv') for c in cases]

    def run(off_of, single=False):
        placed = [[_place(x, off_of(j)) for j, x in enumerate(d)] for d in dev_in]
        views = [tuple(v for _, v in pl) for pl in placed]
        if single:
            for vw in views:
                _adam_single(*vw, t)
        else:
            _adam_multi(views, t)
        for pl, d in zip(placed, dev_in):
            assert all(_sentinels_kept(buf, off_of(j), n) for j, (buf, _) in enumerate(pl))
            assert torch.equal(pl[1][1], d[1])      # the gradient is read only
        return [(vw[0], vw[2], vw[3]) for vw in views]

    aligned = run(lambda j: 4)
    for f, c, got in zip(ar.ADAM_FAMILIES, cases, aligned):
        for name, x, r64, r32 in zip('pmv', got, c['r64'], c['r32']):
            _check(f'adam n={n} t={t} {f} {name}', x, r64, r32)
    for f, a, b in zip(ar.ADAM_FAMILIES, aligned, run(lambda j: 4, single=True)):
        assert _eq(a, b), ('single', f)
    # (the largest size moves one operand per step count, the others each of the four)
    for which in (range(4) if n <= 4099 else [ar.ADAM_STEPS.index(t) % 4]):
        for f, a, b in zip(ar.ADAM_FAMILIES, aligned, run(lambda j: 5 if j == which else 4)):
            assert _eq(a, b), ('unaligned ' + 'pgmv'[which], f)
    for f, a, b in zip(ar.ADAM_FAMILIES, aligned, run(lambda j: 5 if j == 0 else 4, single=True)):
        assert _eq(a, b), ('single unaligned', f)
    _status_ok()


@pytest.mark.parametrize('k', [25, 49])
def test_adam_chunks_of_24_tensors(k):
    """More tensors than one launch's table holds (24), of mixed sizes, some empty: every tensor has the bits of its single-tensor run; norms requested in
    the first, second and third launch meet their bound for the grid of THAT launch, are {0, 0} for an empty tensor, and have cb_frobenius_norm_f32's
    bits where the tensor is the largest of its launch."""
    t = 3
    sizes = ar.CHUNK_SIZES[:k]
    inputs = [tuple(x.to(DEV) for x in ar.adam_inputs(ar.ADAM_FAMILIES[i % len(ar.ADAM_FAMILIES)], n, seed=i)) for i, n in enumerate(sizes)]
    multi = [tuple(x.clone() for x in d) for d in inputs]
    want = [i in ar.CHUNK_NORMS[k] for i in range(k)]
    norms = _adam_multi(multi, t, norms=want)
    for i, d in enumerate(inputs):
        one = tuple(x.clone() for x in d)
        _adam_single(*one, t)
        assert _eq(multi[i], one), i
    for i in ar.CHUNK_NORMS[k]:
        lo = i - i % ar.K_ADAM_MAX
        nmax = max(sizes[lo:lo + ar.K_ADAM_MAX])
        _check_norm(f'chunked adam k={k} tensor {i} (n={sizes[i]})', norms[i], multi[i][0], ar.grid_for(-(-nmax // 4)))
        if sizes[i] == nmax:
            assert torch.equal(norms[i].view(torch.int32), _frobenius(multi[i][0]).view(torch.int32)), i
    assert any(i >= 2 * ar.K_ADAM_MAX for i in ar.CHUNK_NORMS[k]) == (k > 2 * ar.K_ADAM_MAX)
    _status_ok()


@pytest.mark.parametrize('t', ar.ADAM_STEPS)
def test_adam_reads_the_step_count_from_device_memory(t):
    """step_dev: an int64 in device memory holding t, `step` argument 0 (what a captured step does; no capture here): the bias corrections are then formed
    on the device, in double — inside the yardstick of the reference for the same t, through both entry points."""
    n = 4099
    step_dev = torch.tensor([t], dtype=torch.int64, device=DEV)
    for f in ar.ADAM_FAMILIES:
        c = ar.adam_case(f, n, t)
        for entry in ('multi', 'single'):
            d = tuple(c[k].to(DEV) for k in 'pgmv')
            if entry == 'multi':
                _adam_multi([d], t, step_dev=step_dev)
            else:
                _adam_single(*d, t, step_dev=step_dev)
            for name, x, r64, r32 in zip('pmv', (d[0], d[2], d[3]), c['r64'], c['r32']):
                _check(f'adam step_dev {entry} t={t} {f} {name}', x, r64, r32)
    assert int(step_dev.item()) == t
    _status_ok()


def test_adam_extra_decay_counts_only_when_finite():
    """The per-tensor coefficient read from device memory: a finite one is added to weight_decay; +inf and NaN (an all-zero table's se_reg / ||le||) count
    as 0 — the bits of the tensor without a coefficient."""
    n, t = 4099, 2
    coefs = [0.25, math.inf, math.nan, None]
    cases = [ar.adam_case('warm', n, t, extra=e) for e in coefs]
    devs = [tuple(c[k].to(DEV) for k in 'pgmv') for c in cases]
    extras = [torch.tensor([e], dtype=torch.float32, device=DEV) if e is not None else None for e in coefs]
    _adam_multi(devs, t, extras=extras)
    for e, c, d in zip(coefs, cases, devs):
        for name, x, r64, r32 in zip('pmv', (d[0], d[2], d[3]), c['r64'], c['r32']):
            _check(f'adam extra_decay={e} {name}', x, r64, r32)
    for i in (1, 2):
        assert _eq((devs[i][0], devs[i][2], devs[i][3]), (devs[3][0], devs[3][2], devs[3][3])), coefs[i]
    assert not torch.equal(devs[0][0], devs[3][0])
    _status_ok()


def test_a_guard_skipped_adam_step_leaves_no_stale_norm(monkeypatch):
    """The guard word set (a failed gradient-row check): optim.Adam.step() leaves parameters and moments bit-unchanged, and what it records as the
    parameters' norms afterwards is the norm of those unchanged values (or nothing) — never what the norm workspace held before, here 1e30 in every
    float.  The word is set directly and cleared again; the device error word is not touched."""
    from gnn_tail_generalization_amd import _lib, ops
    from gnn_tail_generalization_amd.optim import Adam
    lib = _lib.load()
    shapes = [(3000, 64), (77,), (513, 40), (5,)]
    wanted = (0, 2, 3)
    gen = torch.Generator().manual_seed(11)
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen).to(DEV)) for s in shapes]
    opt = Adam(params, lr=H['lr'], weight_decay=H['wd'])
    for i in wanted:
        ops.frobenius_norm(params[i])                      # a forward asked for these norms
    for p in params:
        p.grad = torch.randn(*p.shape, generator=gen).to(DEV)
    opt.step()                                             # an ordinary step: the moments are warm, the norms known
    assert all(ops.known_norm(params[i]) is not None for i in wanted)
    before = [(p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for p in params]
    for p in params:
        p.grad = torch.randn(*p.shape, generator=gen).to(DEV)
    wsb = lib.cb_adam_norm_workspace_bytes(len(wanted))
    real_ws, poisoned = ops._ws, []

    def ws_of_1e30(nbytes, device):                        # the step's norm workspace, every float 1e30 before the launch (same stream)
        ws = real_ws(nbytes, device)
        if nbytes == wsb:
            ws.view(torch.float32).fill_(1e30)
            poisoned.append(nbytes)
        return ws
    monkeypatch.setattr(ops, '_ws', ws_of_1e30)
    guard = _lib.grad_guard(torch.device(DEV))
    try:
        guard.fill_(1)
        opt.step()
        torch.cuda.synchronize()
    finally:
        guard.zero_()
        monkeypatch.setattr(ops, '_ws', real_ws)
    assert poisoned == [wsb]
    for p, (p0, m0, v0) in zip(params, before):
        assert _eq((p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']), (p0, m0, v0))
    nb_launch = ar.grid_for(-(-max(p.numel() for p in params) // 4))
    for i in wanted:
        p = params[i]
        known = ops.known_norm(p)
        nb = nb_launch
        if known is not None:
            _check_norm(f'guarded step, known norm of parameter {i}', known, p.detach().reshape(-1), nb_launch)
        else:
            nb = ar.grid_for(-(-p.numel() // 4))
        nrm = ops.frobenius_norm(p).detach()
        ref = float(p.detach().double().norm())
        assert abs(float(nrm) - ref) <= ar.norm_rel_bounds(p.numel(), nb)[0] * ref, (i, float(nrm), ref)
    _status_ok()


def test_a_guard_skipped_launch_through_the_abi_writes_only_the_norms():
    """cb_adam_multi_norm_f32 itself with the guard set: aligned and unaligned tensors, with and without a norm request; sentinels, inputs and moments
    untouched, the requested pairs are the norms of the values that stayed."""
    t = 2
    sizes, offs = [4099, 5, 70001, 1023, 0], [4, 5, 5, 4, 4]
    placed = [[_place(x.to(DEV), off) for x in ar.adam_inputs('warm', n, seed=i)] for i, (n, off) in enumerate(zip(sizes, offs))]
    views = [tuple(v for _, v in pl) for pl in placed]
    before = [tuple(v.clone() for v in vw) for vw in views]
    guard = torch.ones(1, dtype=torch.int32, device=DEV)
    want = [True, True, False, True, True]
    norms = _adam_multi(views, t, norms=want, guard=guard)
    nb = ar.grid_for(-(-max(sizes) // 4))
    for i, (pl, vw, b) in enumerate(zip(placed, views, before)):
        assert _eq(vw, b), i
        assert all(_sentinels_kept(buf, offs[i], sizes[i]) for buf, _ in pl), i
        if want[i]:
            _check_norm(f'guarded launch, tensor {i} (n={sizes[i]})', norms[i], vw[0], nb)
    _status_ok()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Frobenius norm
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', ar.NORM_SCALES)
@pytest.mark.parametrize('n', ar.NORM_SIZES)
def test_frobenius_norm_against_float64(n, scale):
    """cb_frobenius_norm_f32 from one element to the grid-stride loop's second trip, at an aligned and at an offset pointer, at magnitudes whose squares
    sit at both ends of the normal float32 range; ops.frobenius_norm is that call."""
    from gnn_tail_generalization_amd import ops
    x = ar.norm_input(n, scale).to(DEV)
    nb = ar.grid_for(-(-n // 4)) if n else 0
    for off in (4, 5):
        buf, view = _place(x, off)
        out2 = _frobenius(view)
        _check_norm(f'frobenius n={n} scale={scale:g} off={off}', out2, view, nb)
        assert _sentinels_kept(buf, off, n) and torch.equal(view, x)
    if n:
        assert torch.equal(ops.frobenius_norm(x).reshape(1).view(torch.int32), _frobenius(x)[:1].view(torch.int32))
    _status_ok()
