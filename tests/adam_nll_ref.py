"""Restatement of the three kernels that end a training step (csrc/cb_reduce.hip): the fused log-softmax + NLL loss with its gradient, one fused Adam
step, and the sum of squares behind the Frobenius norm.  Plain torch, generic in the dtype: evaluated in float64 it is the reference of
tests/test_gpu_adam_nll.py, evaluated in float32 on the CPU it is the yardstick (tests/test_adam_nll_ref_host.py holds the float64 form to torch.optim.Adam
and F.nll_loss, and the float32 form to the bounds below).  Every constant the kernels receive as a float (learning rate, betas, eps, weight decay,
1 / count, the bias corrections) is rounded to float32 FIRST and then cast to the working dtype: the float64 reference and the kernel evaluate the same
function of the same numbers.

Also here: the inputs of every case of both test files (one place, so the host file checks exactly what the GPU file runs)."""
import functools
import math

import torch

K_BLOCK, K_MAX_BLOCKS, K_ADAM_MAX = 256, 2048, 24      # csrc/cb_reduce.h kBlock, kMaxBlocks; csrc/cb_reduce.hip kAdamMax
NAN = float('nan')


def grid_for(work_items):
    """csrc/cb_reduce.h grid_for: blocks of a grid-stride launch over `work_items` items."""
    return min(K_MAX_BLOCKS, max(1, -(-int(work_items) // K_BLOCK)))


def _f32(x, dtype):
    """The float32 rounding of a host number, in the working dtype."""
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# log-softmax + NLL
# ---------------------------------------------------------------------------------------------------------------------------------------------
def nll_rows(z, y):
    """(lse_r - z_r[y_r], softmax(z_r)) per row, in z's dtype, the kernels' formulas: mx = max_c z, e = exp(z - mx), se = sum e, lse = mx + log(se),
    softmax = e * (1 / se).  A label outside [0, C) is never an index: that row's loss term is NaN (the softmax is what it is)."""
    C = z.shape[1]
    mx = z.max(1, keepdim=True).values
    e = torch.exp(z - mx)
    se = e.sum(1, keepdim=True)
    lse = (mx + torch.log(se)).squeeze(1)
    ok = (y >= 0) & (y < C)
    zt = z.gather(1, torch.where(ok, y, torch.zeros_like(y)).unsqueeze(1)).squeeze(1)
    return torch.where(ok, lse - zt, torch.full_like(lse, NAN)), e * (1.0 / se)


def nll(z, y, mask, count):
    """(loss, grad) of cb_nll_logsoftmax_f32: loss = (sum over the rows with mask != 0 of nll_rows) * inv, grad = (softmax - onehot) * inv on those rows and
    0 elsewhere, inv = float32(1 / float32(count)) (0 when count <= 0).  mask None: all rows.  Rows outside the mask are never looked at (their labels may
    be anything); a masked row with a label outside [0, C) is NaN in the loss and in its whole gradient row."""
    rows, C = z.shape
    inv = _f32(1.0, torch.float32).div(_f32(count, torch.float32)).to(z.dtype) if count > 0 else torch.zeros((), dtype=z.dtype)
    sel = torch.ones(rows, dtype=torch.bool) if mask is None else mask.bool()
    grad = torch.zeros_like(z)
    if not bool(sel.any()):
        return torch.zeros((), dtype=z.dtype), grad
    zs, ys = z[sel], y[sel]
    per_row, sm = nll_rows(zs, ys)
    ok = (ys >= 0) & (ys < C)
    onehot = torch.zeros_like(zs)
    onehot[ok, ys[ok]] = 1.0
    g = (sm - onehot) * inv
    g[~ok] = NAN
    grad[sel] = g
    return per_row.sum() * inv, grad


def nll_loss_bound(z64, y, mask, count):
    """Bound on |loss_fp32 - loss_fp64| for ANY correct float32 evaluation of nll() on finite rows:

        B = 2 * mean_r [ 2^-24 * (C + |lse_r| + |z_r[y_r]| + 2 + ln C) ]  +  2^-20 * mean_r |nll_r|        (r over the masked rows, float64 values)

    Per row (unit roundoff u = 2^-24): z - mx is exact or rounded once and exp amplifies that by |d| e^d <= 1/e per term; the C terms of se are each one
    exp (about an ulp) and enter C - 1 roundings of the sum, together at most C u relative in se, which log() turns into C u ABSOLUTE in log(se)
    (the first C); log(se) itself is in [0, ln C] and costs its own ulps (the ln C and the 2); mx + log(se) rounds once at |lse_r| and the subtraction of
    z_r[y_r] once at no more than |lse_r| + |z_r[y_r]|.  The factor 2 in front leaves room for a library exp / log of two ulps and for fused multiply-adds
    that round elsewhere.  The rows are then summed: in float32 partial sums of depth <= 16 roundings (a thread's rows, the wavefront and block trees;
    the kernels finish in double) — 2^-20 = 16 u on the mean of |nll_r|, which also covers the float32 rounding of 1 / count (one u) and of the result.
    `mean` divides by `count` as the kernel does.  Rows that are NaN in the reference make the loss NaN; there is nothing to bound then."""
    sel = torch.ones(z64.shape[0], dtype=torch.bool) if mask is None else mask.bool()
    if not bool(sel.any()) or count <= 0:
        return 0.0
    zs, ys = z64[sel].double(), y[sel]
    C = zs.shape[1]
    per_row, _ = nll_rows(zs, ys)
    zt = zs.gather(1, ys.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    lse = per_row + zt
    term = 2.0 ** -24 * (C + lse.abs() + zt.abs() + 2.0 + math.log(C))
    return float(2.0 * term.sum() / count + 2.0 ** -20 * per_row.abs().sum() / count)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, t, lr, b1, b2, eps, wd, extra=None):
    """(p', m', v') after step number t >= 1 from the state (p, m, v) with gradient g — k_adam / k_adam_multi, expression for expression:
        gg = g + wd p;  m' = b1 m + (1 - b1) gg;  v' = b2 v + ((1 - b2) gg) gg;  denom = sqrt(v') / bc2_sqrt + eps;  p' = p - (lr / bc1) (m' / denom)
    bc1 = 1 - b1^t and bc2_sqrt = sqrt(1 - b2^t) are formed in double from the float32 betas and rounded to float32, as the host side of the launch does.
    extra: the per-tensor coefficient added to wd, only when it is finite."""
    dt = p.dtype
    lr_, b1_, b2_, eps_, wd_ = (_f32(x, dt) for x in (lr, b1, b2, eps, wd))
    b1d, b2d = float(_f32(b1, torch.float64)), float(_f32(b2, torch.float64))
    bc1 = _f32(1.0 - b1d ** float(t), dt)
    bc2_sqrt = _f32(math.sqrt(1.0 - b2d ** float(t)), dt)
    step = lr_ / bc1
    if extra is not None and math.isfinite(float(_f32(extra, torch.float64))):
        wd_ = wd_ + _f32(extra, dt)
    gg = g + wd_ * p
    m2 = b1_ * m + (1.0 - b1_) * gg
    v2 = b2_ * v + (1.0 - b2_) * gg * gg
    denom = torch.sqrt(v2) / bc2_sqrt + eps_
    return p - step * (m2 / denom), m2, v2


def sumsq_norm(x):
    """(||x||, ||x||^2) in x's dtype."""
    s = (x * x).sum()
    return torch.sqrt(s), s


def norm_rel_bounds(n, nb):
    """(relative bound on ||x||, on ||x||^2) of a float32 sum of squares over n elements by a launch of nb blocks of 256 threads (k_sumsq, k_adam_multi)
    against the float64 sum of the same float32 values:  ||x||^2: 2^-24 * (4 * ceil(nq / (nb * 256)) + 16),  nq = ceil(n / 4);  ||x||: half that + 2^-24.
    All terms are non-negative, so the relative error of the sum is at most the number of roundings on the longest path from a term to the result times
    u = 2^-24 (to first order): a thread adds one group of four squares per trip of its grid-stride loop — four roundings each (three products that are
    not fused, the adds) — then 6 levels of the wavefront butterfly, 4 adds over the block's wavefronts, the rounding of the square itself and of the
    final conversions (the finish sums the block partials in double): 16 covers them.  sqrt halves a relative error and rounds once more."""
    nq = -(-int(n) // 4)
    trips = -(-nq // (max(int(nb), 1) * K_BLOCK))
    sq = 2.0 ** -24 * (4 * trips + 16)
    return sq / 2 + 2.0 ** -24, sq


# ---------------------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------------------
def same_specials(got, ref):
    """NaN and +-Inf sit at the same positions (and the infinities have the same sign)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return False
    inf = torch.isinf(ref)
    return torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf])


def max_err(got, ref):
    """max |got - ref| in float64 over the positions where the reference is finite (same_specials() is asserted separately)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    fin = torch.isfinite(ref)
    d = (got[fin] - ref[fin]).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)
    return float(d.max()) if d.numel() else 0.0


def bound(r64, r32):
    """4 * max |T_cpu32 - T_64| + 2^-22 * max |T_64| (tests/test_gpu_attn.py): four times the error of the same formulas in float32 on the CPU, plus one
    rounding of the result itself.  Per tensor."""
    fin = r64[torch.isfinite(r64)]
    top = float(fin.abs().max()) if fin.numel() else 0.0
    return 4.0 * max_err(r32, r64) + 2.0 ** -22 * top


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases: NLL
# ---------------------------------------------------------------------------------------------------------------------------------------------
NLL_SHAPES = [(1, 2), (257, 2), (300, 7), (301, 8), (513, 40), (300, 47), (130, 64), (515, 48), (70, 128), (9, 4096), (524288 + 77, 4)]
NLL_FAMILIES = ['randn3', 'randn1e4', 'shift3e4', 'equal', 'dominant', 'neginf30', 'infrows', 'tiny']
NLL_MASKS = ['none', 'some', 'one', 'empty']
NLL_VEC_C = [4, 8, 40, 48, 64]      # classes with a k_nll_fused_v4 instance


def _gen(*key):
    """A generator seeded by a tuple of ints (the same stream in every process)."""
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31) + 1)


_FAMILY_ID = {f: i for i, f in enumerate(NLL_FAMILIES)}


def nll_inputs(rows, C, family):
    """(z float32 [rows, C], y int64 [rows]) of one input family; every label is valid."""
    gen = _gen(rows, C, _FAMILY_ID[family])
    r = torch.randn(rows, C, generator=gen)
    y = torch.randint(0, C, (rows,), generator=gen)
    ar = torch.arange(rows)
    if family == 'randn3':
        z = 3.0 * r
    elif family == 'randn1e4':
        z = 1e4 * r
    elif family == 'shift3e4':
        z = r + 3e4
    elif family == 'equal':
        z = torch.full((rows, C), 0.7)
    elif family == 'dominant':      # one logit of 80 per row; the label on it in even rows and off it in odd ones
        z = r.clone()
        top = torch.randint(0, C, (rows,), generator=gen)
        z[ar, top] = 80.0
        y = torch.where(ar % 2 == 0, top, (top + 1 + torch.randint(0, C - 1, (rows,), generator=gen)) % C)
    elif family == 'neginf30':      # about 30 % of the entries are -inf, never the label's column
        z = r.clone()
        z[torch.rand(rows, C, generator=gen) < 0.3] = -math.inf
        z[ar, y] = r[ar, y]
    elif family == 'infrows':       # row 0 is all -inf; the middle row (if there is another) holds one +inf: NaN rows in every evaluation
        z = r.clone()
        z[0] = -math.inf
        if rows > 1:
            z[rows // 2, C // 2] = math.inf
    elif family == 'tiny':          # 1e-30 scale, every entry a normal float32
        z = 1e-30 * torch.sign(r) * (0.1 + r.abs())
    else:
        raise KeyError(family)
    return z.float().contiguous(), y


def nll_mask(rows, kind):
    """(mask bool [rows] or None, count)."""
    if kind == 'none':
        return None, rows
    if kind == 'some':       # about 40 % of the rows, at least one
        m = torch.rand(rows, generator=_gen(rows, 40)) < 0.4
        m[rows // 2] = True
        return m, int(m.sum())
    if kind == 'one':
        m = torch.zeros(rows, dtype=torch.bool)
        m[rows // 3] = True
        return m, 1
    if kind == 'empty':      # the node-sharded rank without loss rows: count is the global number of loss rows
        return torch.zeros(rows, dtype=torch.bool), 5
    raise KeyError(kind)


@functools.lru_cache(maxsize=8)
def nll_case(rows, C, family, mask_kind):
    """dict: z, y, mask, count, and the restatement in both precisions (loss64, grad64, loss32, grad32) with the loss bound B.  Shared, never written."""
    z, y = nll_inputs(rows, C, family)
    mask, count = nll_mask(rows, mask_kind)
    loss64, grad64 = nll(z.double(), y, mask, count)
    loss32, grad32 = nll(z, y, mask, count)
    return dict(z=z, y=y, mask=mask, count=count, loss64=loss64, grad64=grad64, loss32=loss32, grad32=grad32,
                B=nll_loss_bound(z.double(), y, mask, count) if bool(torch.isfinite(loss64)) else None)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases: Adam
# ---------------------------------------------------------------------------------------------------------------------------------------------
ADAM_HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=5e-4)
ADAM_FAMILIES = ['fresh', 'warm', 'g1e-9', 'g1e6', 'gzero', 'cancel']
ADAM_STEPS = [1, 2, 1000, 10 ** 6]
ADAM_SIZES = [1, 3, 4, 5, 1023, 4099, 2097152 + 5]


def _away(r, scale):
    """scale * r pushed away from zero: |.| >= 0.1 * scale (no square or product in the float32 denormal range)."""
    return scale * torch.sign(r) * (0.1 + r.abs())


def adam_inputs(family, n, seed=0):
    """The prescribed state (p, g, m, v), float32 [n], of one family."""
    gen = _gen(n, ADAM_FAMILIES.index(family), seed)
    rp, rg, rm, rv = (torch.randn(n, generator=gen) for _ in range(4))
    rp = torch.where(rp == 0, torch.ones_like(rp), rp)
    rg = torch.where(rg == 0, torch.ones_like(rg), rg)
    p, g = _away(rp, 1.0), _away(rg, 1.0)
    m, v = torch.zeros(n), torch.zeros(n)
    if family == 'fresh':
        pass
    elif family == 'warm':
        m, v = 0.3 * rm, 0.05 * rv * rv + 1e-6
    elif family == 'g1e-9':     # a table of 1e-6 scale so that wd * p does not drown the gradient
        p, g = _away(rp, 1e-6), _away(rg, 1e-9)
        m, v = 1e-10 * rm, 1e-18 * (rv * rv + 0.01)
    elif family == 'g1e6':
        g = _away(rg, 1e6)
        m, v = 1e5 * rm, 1e11 * (rv * rv + 0.01)
    elif family == 'gzero':
        g = torch.zeros(n)
    elif family == 'cancel':    # g = -wd p to three digits: gg = g + wd p cancels
        g = -(ADAM_HYPER['wd'] * p) * (1.0 + 1e-3 * rg)
        m, v = 1e-4 * rm, 1e-8 * (rv * rv + 0.01)
    else:
        raise KeyError(family)
    return p.float(), g.float(), m.float(), v.float()


def adam_case(family, n, t, extra=None, seed=0):
    """dict: the inputs p, g, m, v and the restated step in both precisions: r64 = (p', m', v'), r32 likewise."""
    p, g, m, v = adam_inputs(family, n, seed)
    r64 = adam_step(p.double(), g.double(), m.double(), v.double(), t, extra=extra, **ADAM_HYPER)
    r32 = adam_step(p, g, m, v, t, extra=extra, **ADAM_HYPER)
    return dict(p=p, g=g, m=m, v=v, r64=r64, r32=r32)


CHUNK_SIZES = [70001, 0, 1, 3, 4, 5, 64, 257, 1023, 1024, 4099, 0, 2, 7, 8, 100, 511, 513, 33, 12, 6, 1025, 31, 9,      # first launch (24 tensors)
               4099, 5, 0, 300, 4100, 17, 1, 4, 63, 65, 255, 256, 1000, 0, 3, 11, 2048, 77, 19, 640, 13, 2, 10, 129,    # second
               9000]                                                                                                       # third (the 49th tensor)
CHUNK_NORMS = {25: [0, 1, 10, 24], 49: [0, 1, 10, 24, 26, 28, 48]}      # tensors whose norm is requested: the largest of a launch, others, an empty one


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cases: Frobenius norm
# ---------------------------------------------------------------------------------------------------------------------------------------------
NORM_SIZES = [0, 1, 3, 5, 4099, 768000, 2097152 * 4 + 7]
NORM_SCALES = [1e-15, 1.0, 1e15]


def norm_input(n, scale):
    """float32 [n] at magnitude `scale`, |x| >= 0.5 * scale: every square is a normal float32 and the sum stays finite."""
    r = torch.randn(n, generator=_gen(n, int(math.log10(scale)) + 100))
    return (scale * torch.where(r < 0, -torch.ones_like(r), torch.ones_like(r)) * (0.5 + r.abs())).float()
