"""Inputs and float64 references shared by the norm tests (tests/test_norms_host.py on the CPU, tests/test_gpu_norm_kernels.py on the
device, the row-sharded part of tests/test_dist_gloo.py): columns whose mean is small or large against their spread.  A column mean
that is large against the column's std is the usual state after ReLU and in a deep, over-smoothed GCN; one-pass s2/n - mu^2 column
statistics lose (mean/std)^2 of their digits there."""
import torch
import torch.nn.functional as F

import coldbrew_oracle as orc

# name -> (rows, d, column mean, column std); None: drawn per column from MIXED_MEAN x MIXED_STD inside one matrix
CASES = {
    'n4099_d64_m0.5_s2': (4099, 64, 0.5, 2.0),
    'n100003_d40_m1_s0.1': (100003, 40, 1.0, 0.1),
    'n100003_d40_m3_s0.01': (100003, 40, 3.0, 0.01),
    'n100003_d40_m10_s0.01': (100003, 40, 10.0, 0.01),
    'n3000_d16_m30_s0.1': (3000, 16, 30.0, 0.1),
    'n65537_d40_m100_s0.001': (65537, 40, 100.0, 1e-3),
    'n20011_d45_mixed_columns': (20011, 45, None, None),
}
WELL = ['n4099_d64_m0.5_s2']
ILL = [k for k in CASES if k not in WELL]
MIXED_MEAN, MIXED_STD = (0.0, 1.0, 30.0), (1.0, 0.1, 0.01)
KINDS = ('batch', 'pair', 'mean')


def make(name, seed=0):
    """x, gout, weight, bias (float32, CPU) of a case."""
    rows, d, mean, std = CASES[name]
    g = torch.Generator().manual_seed(seed + rows + d)
    z = torch.randn(rows, d, generator=g)
    if mean is None:                                      # every (mean, std) pair occurs: 9 combinations over 45 columns
        c = torch.arange(d)
        mean = torch.tensor(MIXED_MEAN)[c % 3]
        std = torch.tensor(MIXED_STD)[(c // 3) % 3]
    x = (z * std + mean).contiguous()
    gout = torch.randn(rows, d, generator=g)
    weight = torch.rand(d, generator=g) + 0.5
    bias = torch.randn(d, generator=g)
    return x, gout, weight, bias


def torch_norm(kind, x, gout, weight=None, bias=None, eps=1e-5):
    """The norm in plain torch in x's dtype and on x's device with its autograd: (y, dx[, dweight, dbias])."""
    x = x.detach().clone().requires_grad_(True)
    params = []
    if kind == 'batch':
        params = [t.detach().to(x).clone().requires_grad_(True) for t in (weight, bias) if t is not None]
        w, b = (params + [None, None])[:2] if weight is not None else (None, None)
        y = F.batch_norm(x, None, None, w, b, True, 0.1, eps)
    elif kind == 'pair':
        y = orc.pair_norm(x)
    else:
        y = orc.mean_norm(x)
    y.backward(gout.to(x))
    return [y.detach(), x.grad] + [p.grad for p in params]


NAMES = ('y', 'dx', 'dweight', 'dbias')
