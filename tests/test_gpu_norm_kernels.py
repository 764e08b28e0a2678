"""The five norm kernels of csrc/cb_norms.hip (cb_node_norm_fwd/bwd_f32, cb_colstats_f32, cb_col_affine_f32, cb_col_bwd_combine_f32)
through norms_hip.py and through the C ABI, against float64 on the CPU, at the sizes where their loops take a second trip: d > 64 per
lane and ragged d in the node-norm kernels, d > 256 and row slabs longer than 64 rows in the column statistics, more than 256 partials
in the finish kernel, more than 2048 x 256 elements in the element-wise pair.

Rule (the project's form for kernels measured against torch's own float32, tests/test_gpu_kernels.py:341-350; the form of
tests/test_gpu_student_kernels.py): on the same inputs the error of torch's float32 composition of the same operation on the device
against float64 is err32; the kernel's error must satisfy err <= max(2 * err32, 8 * 2^-24), both relative to the largest magnitude of
the compared tensor's row (student_ref.rel_err / within).  Everything else is compared bit for bit.  Every figure is printed before it is
asserted (run with -s to collect them; profiles/norm_kernels.md holds a recorded run)."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import coldbrew_oracle as orc
import norm_cases as nc
import student_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _judge(tag, rows):
    """rows: (name, got, torch32, ref64).  Prints each figure, then asserts the rule on all of them."""
    bad = []
    for name, u, v, r in rows:
        err, err32 = sr.rel_err(u, r), sr.rel_err(v, r)
        print(f'{tag} {name}: err={err / sr.EPS24:.2f} err32={err32 / sr.EPS24:.2f} (x 2^-24)')
        if not sr.within(err, err32):
            bad.append((name, round(err / sr.EPS24, 2), round(err32 / sr.EPS24, 2)))
    assert not bad, (tag, bad)


def _lib():
    from gnn_tail_generalization_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------------------------------------------------------------
# node_norm
# ---------------------------------------------------------------------------------------------------------------------
NODE_KINDS = ['n', 'v', 'm', 'srv', 'pr']
NODE_D = [1, 16, 63, 64, 65, 256, 1000, 1025]
NODE_ROWS = [1, 63, 65537]        # 65537 wavefronts > the capped grid's 2048 * 4: the grid-stride trip runs


def _node_inputs(rows, d):
    """Rows alternate between a row mean of 0 and of 20 x the row's std (a single row: the latter); the row std varies from 0.5 to 2."""
    g = torch.Generator().manual_seed(7 * d + rows)
    std = 0.5 + 1.5 * torch.rand(rows, 1, generator=g)
    z = torch.randn(rows, d, generator=g)
    if d > 1:
        z = z - z.mean(1, keepdim=True)
    odd = (torch.arange(rows).reshape(-1, 1) % 2 == 1) | (rows == 1)
    off = torch.where(odd, 20.0 * std, torch.zeros_like(std))
    return (z * std + off).contiguous(), torch.randn(rows, d, generator=g)


def _fwd_bwd(fn, x, g):
    x = x.detach().clone().requires_grad_(True)
    y = fn(x)
    y.backward(g)
    return y.detach(), x.grad


@pytest.mark.parametrize('rows', NODE_ROWS)
@pytest.mark.parametrize('d', NODE_D)
def test_node_norm_forward_backward_and_stats(d, rows):
    from gnn_tail_generalization_amd import norms_hip
    L, lib = _lib()
    x, g = _node_inputs(rows, d)
    xd, gd, x64, g64 = x.to(DEV), g.to(DEV), x.double(), g.double()
    figures = []
    for kind in NODE_KINDS:
        got = _fwd_bwd(lambda t: norms_hip.node_norm(t, kind), xd, gd)
        t32 = _fwd_bwd(lambda t: orc.node_norm(t, kind), xd, gd)
        ref = _fwd_bwd(lambda t: orc.node_norm(t, kind), x64, g64)
        figures += [(f'{kind} y', got[0], t32[0], ref[0]), (f'{kind} dx', got[1], t32[1], ref[1])]
    # stats = (mean, sqrt(biased var + eps)) of the row, as the backward reads them; the kernel forms them before c and q come into play,
    # so one call (c = 1, q = 1) stands for all five kinds
    y = torch.empty_like(xd)
    stats = torch.full((rows, 2), float('nan'), device=DEV)
    L.check(lib.cb_node_norm_fwd_f32(L.ptr(xd), L.ptr(y), L.ptr(stats), rows, d, 1.0, 1.0, 1e-5, L.stream_ptr()), 'cb_node_norm_fwd_f32')

    def st(t):
        return torch.stack([t.mean(1), (t.var(1, unbiased=False) + 1e-5).sqrt()], 1)
    figures.append(('stats', stats, st(xd), st(x64)))
    _judge(f'node_norm d={d} rows={rows}', figures)


@pytest.mark.parametrize('kind', NODE_KINDS)
def test_node_norm_non_contiguous_input_and_gradient(kind):
    """A strided x and a strided incoming gradient give bit for bit what their contiguous copies give."""
    from gnn_tail_generalization_amd import norms_hip
    x, g = _node_inputs(257, 2 * 65)
    base = x.to(DEV).requires_grad_(True)
    xs, gs = base[:, ::2], g.to(DEV)[:, 1::2]
    assert not xs.is_contiguous() and not gs.is_contiguous()
    y = norms_hip.node_norm(xs, kind)
    y.backward(gs)
    assert bool((base.grad[:, 1::2] == 0).all())
    a = y.detach(), base.grad[:, ::2]
    b = _fwd_bwd(lambda t: norms_hip.node_norm(t, kind), xs.detach().contiguous(), gs.contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    xs, gs = xs.detach().contiguous(), gs.contiguous()
    ref = _fwd_bwd(lambda t: orc.node_norm(t, kind), xs.double().cpu(), gs.double().cpu())
    t32 = _fwd_bwd(lambda t: orc.node_norm(t, kind), xs, gs)
    _judge(f'node_norm strided {kind}', [('y', a[0], t32[0], ref[0]), ('dx', a[1], t32[1], ref[1])])


def test_node_norm_unknown_kind_and_power_root():
    from gnn_tail_generalization_amd import norms_hip
    from gnn_tail_generalization_amd.GNN_model.norm_tricks import node_norm
    x = torch.randn(5, 7, device=DEV)
    assert norms_hip.node_norm(x, 'q') is x
    assert node_norm(node_norm_type='other')(x) is x
    with pytest.raises(NotImplementedError):
        node_norm(node_norm_type='pr', power_root=3)(x)
    with pytest.raises(NotImplementedError):
        norms_hip.node_norm(x, 'pr', power=1 / 3)
    assert torch.equal(node_norm(node_norm_type='pr', power_root=2)(x), norms_hip.node_norm(x, 'srv'))


# ---------------------------------------------------------------------------------------------------------------------
# cb_colstats_f32
# ---------------------------------------------------------------------------------------------------------------------
# every value of rows {0, 1, 64, 65, 4099, 131073, 300001} and of d {1, 40, 255, 256, 257, 640, 1000}; the cross product pruned to what
# runs in a few seconds.  131073 rows = 2048 slabs of 65 rows (64 + 1); 300001 rows = slabs of 147; d > 256: the column loop's second trip.
COLSTATS_SHAPES = [(0, 40), (0, 257), (1, 1), (1, 1000), (64, 255), (64, 1), (65, 256), (65, 257), (4099, 40), (4099, 640), (4099, 1000),
                   (131073, 1), (131073, 257), (131073, 640), (300001, 40), (300001, 256), (300001, 1)]


def _colstats(x, w, shift, short=0, out=None):
    """cb_colstats_f32 through the C ABI; `short` bytes are withheld from the workspace size that is declared."""
    L, lib = _lib()
    rows, d = x.shape
    s1, s2 = out if out is not None else (torch.full((d,), float('nan'), device=DEV), torch.full((d,), float('nan'), device=DEV))
    wsb = lib.cb_colstats_workspace_bytes(max(rows, 1), d)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    rc = lib.cb_colstats_f32(L.ptr(x) if rows else None, L.ptr(w) if rows else None, L.ptr(shift), rows, d, L.ptr(s1), L.ptr(s2), L.ptr(ws),
                             wsb - short, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, s1, s2


def _colstats_ref(x, w, shift):
    """The definition (include/coldbrew_hip.h) in x's dtype."""
    sh = shift if shift is not None else torch.zeros(x.shape[1], dtype=x.dtype, device=x.device)
    if w is None:
        return (x - sh).sum(0), ((x - sh) * (x - sh)).sum(0)
    return x.sum(0), (x * (w - sh)).sum(0)


@pytest.mark.parametrize('use_shift', [False, True], ids=['noshift', 'shift'])
@pytest.mark.parametrize('use_w', [False, True], ids=['squares', 'weighted'])
@pytest.mark.parametrize('rows,d', COLSTATS_SHAPES)
def test_colstats_against_float64(rows, d, use_w, use_shift):
    g = torch.Generator().manual_seed(rows + 31 * d)
    x = torch.randn(rows, d, generator=g) * 1.5 + 3.0
    w = torch.randn(rows, d, generator=g) + 2.0 if use_w else None
    # a pivot near the column mean (of x, or of w), never on it: the centred sums stay well away from zero
    shift = (2.0 + (w is None) + 0.3 * (torch.rand(d, generator=g) + 0.2)) if use_shift else None
    xd, wd, sd = (t.to(DEV) if t is not None else None for t in (x, w, shift))
    rc, s1, s2 = _colstats(xd, wd, sd)
    assert rc == 0
    rc2, t1, t2 = _colstats(xd, wd, sd)
    assert rc2 == 0 and torch.equal(s1, t1) and torch.equal(s2, t2)          # fixed-order sums: two launches are bitwise equal
    if rows == 0:
        assert bool((s1 == 0).all()) and bool((s2 == 0).all())
        return
    r1, r2 = _colstats_ref(x.double(), w.double() if use_w else None, shift.double() if use_shift else None)
    a1, a2 = _colstats_ref(xd, wd, sd)
    _judge(f'colstats rows={rows} d={d} w={int(use_w)} shift={int(use_shift)}', [('sum', s1, a1, r1), ('sum2', s2, a2, r2)])


@pytest.mark.parametrize('rows,d', [(1, 1), (65, 257), (4099, 640), (131073, 40), (300001, 255), (300001, 1000)])
def test_colstats_integer_inputs_are_exact(rows, d):
    """Integer-valued inputs whose partial sums all stay below 2^24 (|x| <= 4, |w| <= 2, |shift| <= 1: at most 25 * 300001 < 2^23) are
    summed without any rounding, so the result is the exact integer sum in every one of the four forms."""
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randint(-4, 5, (rows, d), generator=g)
    w = torch.randint(-2, 3, (rows, d), generator=g)
    shift = torch.randint(-1, 2, (d,), generator=g)
    xd = x.float().to(DEV)
    for uw, us in itertools.product((None, w), (None, shift)):
        rc, s1, s2 = _colstats(xd, uw.float().to(DEV) if uw is not None else None, us.float().to(DEV) if us is not None else None)
        r1, r2 = _colstats_ref(x, uw, us)
        assert rc == 0
        assert torch.equal(s1.cpu().double(), r1.double()), (uw is not None, us is not None)
        assert torch.equal(s2.cpu().double(), r2.double()), (uw is not None, us is not None)


@pytest.mark.parametrize('rows,d', [(1, 1), (4099, 257), (300001, 40)])
def test_colstats_short_workspace_is_refused_before_any_launch(rows, d):
    L, lib = _lib()
    x = torch.ones(rows, d, device=DEV)
    out = (torch.full((d,), -7.0, device=DEV), torch.full((d,), -9.0, device=DEV))
    rc, s1, s2 = _colstats(x, None, None, short=1, out=out)
    assert rc == -3 and b'workspace' in lib.cb_last_error()               # CB_E_WORKSPACE
    assert bool((s1 == -7.0).all()) and bool((s2 == -9.0).all())          # nothing was launched: the outputs are untouched
    rc, s1, s2 = _colstats(x, None, None, out=out)
    assert rc == 0 and bool((s1 == rows).all()) and bool((s2 == rows).all())


# ---------------------------------------------------------------------------------------------------------------------
# cb_col_affine_f32, cb_col_bwd_combine_f32
# ---------------------------------------------------------------------------------------------------------------------
# both sides of 2048 blocks x 256 threads (one element per thread up to there, the grid-stride trip beyond), d that does not divide the
# grid stride of 524288 (40, 257, 5)
ELEMENTWISE_SHAPES = [(3, 5), (2047, 256), (2049, 256), (13107, 40), (13109, 40), (2041, 257), (4099, 257)]


def _opt(mask, *ts):
    return [t if m else None for m, t in zip(mask, ts)]


def _affine_expr(x, shift, scale, bias, gscale):
    v = x - shift if shift is not None else x
    v = v * scale if scale is not None else v
    v = v * gscale
    return v + bias if bias is not None else v


def _combine_expr(g, xh, xs, a, b, e, ga, gb):
    one = torch.ones((), dtype=g.dtype, device=g.device)
    v = (a if a is not None else one) * ga * g
    if xh is not None:
        v = v + (b if b is not None else one) * gb * (xh - xs if xs is not None else xh)
    return v + e if e is not None else v


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


@pytest.mark.parametrize('rows,d', ELEMENTWISE_SHAPES)
def test_col_affine_every_operand_combination(rows, d):
    """y = ((x - shift) * scale) * gscale + bias.  Where bias is absent no step can be contracted into a fused multiply-add, and the result
    is the float32 expression evaluated in that order bit for bit; with bias the compiler fuses `* gscale + bias` (one rounding instead of
    two), so bit equality with torch's two-step evaluation cannot hold and the rule against float64 is used."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g) + 1.0
    vec = [torch.randn(d, generator=g) + 0.5 for _ in range(3)]
    gscale = 1.7
    xd = x.to(DEV)
    figures = []
    for mask in itertools.product((False, True), repeat=3):
        shift, scale, bias = _opt(mask, *vec)
        sd, cd, bd = (t.to(DEV) if t is not None else None for t in (shift, scale, bias))
        y = torch.full_like(xd, float('nan'))
        L.check(lib.cb_col_affine_f32(L.ptr(xd), L.ptr(sd), L.ptr(cd), L.ptr(bd), gscale, L.ptr(y), rows, d, L.stream_ptr()), 'cb_col_affine_f32')
        t32 = _affine_expr(xd, sd, cd, bd, _f32(gscale).to(DEV))
        if bias is None:
            assert torch.equal(y, t32), mask
        else:
            ref = _affine_expr(x.double(), *(t.double() if t is not None else None for t in (shift, scale, bias)), _f32(gscale).double())
            figures.append((f'shift,scale,bias={tuple(int(m) for m in mask)}', y, t32, ref))
    _judge(f'col_affine rows={rows} d={d}', figures)


@pytest.mark.parametrize('rows,d', ELEMENTWISE_SHAPES)
def test_col_bwd_combine_every_operand_combination(rows, d):
    """dx = a * ga * g + b * gb * (xh - xs) + e.  With neither xh nor e there is no sum to fuse a product into, and the float32 expression
    in that order is reproduced bit for bit; otherwise the compiler forms fused multiply-adds (one rounding instead of two), bit equality
    with torch's step-by-step evaluation cannot hold, and the rule against float64 is used."""
    L, lib = _lib()
    gen = torch.Generator().manual_seed(rows + 3 * d)
    g, xh = torch.randn(rows, d, generator=gen), torch.randn(rows, d, generator=gen) + 2.0
    vec = [torch.randn(d, generator=gen) + 0.5 for _ in range(4)]
    ga, gb = 0.75, -1.3
    gd, xhd = g.to(DEV), xh.to(DEV)
    figures = []
    for has_xh in (False, True):
        for mask in itertools.product((False, True), repeat=4):
            xs, a, b, e = _opt(mask, *vec)
            dev = [t.to(DEV) if t is not None else None for t in (xs, a, b, e)]
            dx = torch.full_like(gd, float('nan'))
            L.check(lib.cb_col_bwd_combine_f32(L.ptr(gd), L.ptr(xhd) if has_xh else None, L.ptr(dev[0]), L.ptr(dev[1]), L.ptr(dev[2]),
                                               L.ptr(dev[3]), ga, gb, L.ptr(dx), rows, d, L.stream_ptr()), 'cb_col_bwd_combine_f32')
            t32 = _combine_expr(gd, xhd if has_xh else None, *dev, _f32(ga).to(DEV), _f32(gb).to(DEV))
            if not has_xh and e is None:                       # (xs and b given without xh are not read)
                assert torch.equal(dx, t32), mask
            else:
                ref = _combine_expr(g.double(), xh.double() if has_xh else None, *(t.double() if t is not None else None for t in (xs, a, b, e)),
                                    _f32(ga).double(), _f32(gb).double())
                figures.append((f'xh={int(has_xh)} xs,a,b,e={tuple(int(m) for m in mask)}', dx, t32, ref))
    _judge(f'col_bwd_combine rows={rows} d={d}', figures)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm1d, pair_norm, mean_norm through norms_hip
# ---------------------------------------------------------------------------------------------------------------------
NORM_SHAPES = [(4099, 16), (65537, 256), (300001, 40), (3000, 640)]
# (affine, momentum, track_running_stats)
BN_CONFIGS = [(True, 0.1, True), (False, 0.1, True), (True, 0.3, True), (False, 0.3, True), (True, None, True), (False, None, True),
              (True, 0.1, False), (False, 0.1, False)]


def _bn_step(bn, fn, x, gout):
    for p in bn.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(True)
    y = fn(bn, x)
    y.backward(gout)
    return [y.detach(), x.grad] + [p.grad for p in bn.parameters()]


def _torch_module(m, t):
    return m(t)


@pytest.mark.parametrize('affine,momentum,track', BN_CONFIGS)
@pytest.mark.parametrize('rows,d', NORM_SHAPES)
def test_batch_norm_three_training_steps_then_eval(rows, d, affine, momentum, track):
    from gnn_tail_generalization_amd import norms_hip
    gen = torch.Generator().manual_seed(rows + d)
    ref = torch.nn.BatchNorm1d(d, affine=affine, momentum=momentum, track_running_stats=track).double()
    if affine:
        with torch.no_grad():
            ref.weight.copy_(torch.rand(d, generator=gen) + 0.5)
            ref.bias.copy_(torch.randn(d, generator=gen))
    got, t32 = copy.deepcopy(ref).float().to(DEV), copy.deepcopy(ref).float().to(DEV)
    names = nc.NAMES[:4 if affine else 2]
    x0 = torch.randn(rows, d, generator=gen) * 1.5 + 0.3
    figures = []

    def step(label, x, gout):
        a = _bn_step(got, norms_hip.batch_norm, x.to(DEV), gout.to(DEV))
        b = _bn_step(t32, _torch_module, x.to(DEV), gout.to(DEV))
        r = _bn_step(ref, _torch_module, x.double(), gout.double())
        figures.extend((f'{label} {nm}', u, v, w) for nm, u, v, w in zip(names, a, b, r))

    for k in range(3):
        step(f'step{k}', x0 * (1.0 + 0.25 * k) - 0.4 * k, torch.randn(rows, d, generator=gen))
    if track:
        assert int(got.num_batches_tracked) == 3 == int(ref.num_batches_tracked)
        # (copies: the buffers themselves are overwritten below, and the figures are judged at the end)
        figures += [('running_mean', got.running_mean.clone(), t32.running_mean.clone(), ref.running_mean.clone()),
                    ('running_var', got.running_var.clone(), t32.running_var.clone(), ref.running_var.clone())]
        # eval mode on frozen statistics, the same float32 values in all three modules: y = (x - running_mean) * rsqrt(running_var + eps)
        # * weight + bias through _AffineEvalFn; the affine pair still gets its gradients, as in torch
        with torch.no_grad():
            for m in (got, t32, ref):
                m.running_mean.copy_(ref.running_mean.float())
                m.running_var.copy_(ref.running_var.float())
        frozen = got.running_mean.clone(), got.running_var.clone()
    else:
        assert got.running_mean is None and got.num_batches_tracked is None      # eval then normalises with the batch's statistics
    for m in (got, t32, ref):
        m.eval()
    step('eval', x0 + 0.1, torch.randn(rows, d, generator=gen))
    if track:
        assert int(got.num_batches_tracked) == 3
        assert torch.equal(got.running_mean, frozen[0]) and torch.equal(got.running_var, frozen[1])
    _judge(f'batch_norm {rows}x{d} affine={int(affine)} momentum={momentum} track={int(track)}', figures)


def column_norm_figures(norms_hip, kind, x, gout, w, b):
    """(name, product, torch float32 on the device, float64 on the CPU) of one column norm on one input; train-mode BatchNorm1d with affine."""
    xd = x.to(DEV).requires_grad_(True)
    if kind == 'batch':
        bn = torch.nn.BatchNorm1d(x.shape[1]).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(w)
            bn.bias.copy_(b)
        y = norms_hip.batch_norm(bn, xd)
    else:
        y = {'pair': norms_hip.pair_norm, 'mean': norms_hip.mean_norm}[kind](xd)
    y.backward(gout.to(DEV))
    got = [y.detach(), xd.grad] + ([bn.weight.grad, bn.bias.grad] if kind == 'batch' else [])
    t32 = nc.torch_norm(kind, x.to(DEV), gout.to(DEV), w.to(DEV), b.to(DEV))
    ref = nc.torch_norm(kind, x.double(), gout, w, b)
    return list(zip(nc.NAMES, got, t32, ref))


@pytest.mark.parametrize('kind', ['pair', 'mean'])
@pytest.mark.parametrize('rows,d', NORM_SHAPES)
def test_pair_norm_and_mean_norm(rows, d, kind):
    from gnn_tail_generalization_amd import norms_hip
    gen = torch.Generator().manual_seed(rows + d + 1)
    x, gout = torch.randn(rows, d, generator=gen) * 1.5 + 0.3, torch.randn(rows, d, generator=gen)
    _judge(f'{kind}_norm {rows}x{d}', column_norm_figures(norms_hip, kind, x, gout, torch.ones(d), torch.zeros(d)))


@pytest.mark.parametrize('kind', nc.KINDS)
@pytest.mark.parametrize('name', list(nc.CASES))
def test_column_norms_on_ill_conditioned_columns(name, kind):
    """Columns whose mean is up to 10^5 times their std (tests/norm_cases.py), and one matrix that mixes means {0, 1, 30} with stds
    {1, 0.1, 0.01} column by column.  With one-pass s2/n - mu^2 statistics and a backward written on the raw x these cases miss the rule
    by factors of 10 to 10^5 (profiles/norm_kernels.md has both sets of figures)."""
    from gnn_tail_generalization_amd import norms_hip
    x, gout, w, b = nc.make(name)
    _judge(f'ill-conditioned {name} {kind}', column_norm_figures(norms_hip, kind, x, gout, w, b))


# ---------------------------------------------------------------------------------------------------------------------
# group_norm module (GNN_model/norm_tricks.py): softmax gates, G scaled copies, one BatchNorm1d over G * hidden columns
# ---------------------------------------------------------------------------------------------------------------------
def _group_norm_restated(m, x):
    """group_norm.forward in plain torch, in the dtype and on the device of m and x (the module itself runs only on the device)."""
    if m.num_groups == 1:
        t = m.bn(x)
    else:
        score = F.softmax(F.linear(x, m.group_func.weight, m.group_func.bias), dim=1)
        t = (score.unsqueeze(2) * x.unsqueeze(1)).reshape(x.shape[0], -1)
        t = m.bn(t).view(-1, m.num_groups, m.dim_hidden).sum(dim=1)
    return x + t * m.skip_weight


@pytest.mark.parametrize('hidden', [64, 256])
@pytest.mark.parametrize('groups', [1, 5, 10])
def test_group_norm_module(groups, hidden):
    from gnn_tail_generalization_amd.GNN_model.norm_tricks import group_norm
    rows = 2003
    torch.manual_seed(groups + hidden)
    ref = group_norm(dim_hidden=hidden, num_groups=groups, skip_weight=0.7).double()
    gen = torch.Generator().manual_seed(groups * hidden)
    with torch.no_grad():
        ref.bn.weight.copy_(torch.rand(groups * hidden, generator=gen) + 0.5)
        ref.bn.bias.copy_(torch.randn(groups * hidden, generator=gen))
    got, t32 = copy.deepcopy(ref).float().to(DEV), copy.deepcopy(ref).float().to(DEV)
    x, gout = torch.randn(rows, hidden, generator=gen) + 0.5, torch.randn(rows, hidden, generator=gen)

    def run(m, fn, x_, g_):
        x_ = x_.clone().requires_grad_(True)
        y = fn(m.train(), x_)
        y.backward(g_)
        return [y.detach(), x_.grad, m.bn.weight.grad, m.bn.bias.grad, m.bn.running_mean, m.bn.running_var]
    a = run(got, _torch_module, x.to(DEV), gout.to(DEV))
    b = run(t32, _group_norm_restated, x.to(DEV), gout.to(DEV))
    r = run(ref, _group_norm_restated, x.double(), gout.double())
    _judge(f'group_norm groups={groups} hidden={hidden}', list(zip(('y', 'dx', 'dbn_weight', 'dbn_bias', 'running_mean', 'running_var'), a, b, r)))
