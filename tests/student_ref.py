"""Helpers of the student-MLP tests: the CPU restatement the HIP path is compared against (plain torch in float64, with the
product's dropout keep masks injected), the error measure of the kernel tests, a stand-in teacher and the trainer set-up of
the golden trajectories.  No GPU is needed to import this module."""
import contextlib
import io
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STUDENT_CASES = ['student_semlp_2layer_headtail_iso', 'student_semlp_residual', 'student_semlp_downgraded', 'student_basemlp']
EPS24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------
def ln_gelu_drop(z, gamma, beta, eps, keep=None, p=0.0):
    """dropout(gelu(layer_norm(z))) in z's dtype; keep: bool mask of the kept elements (None: no dropout)."""
    y = F.gelu(F.layer_norm(z, (z.shape[1],), gamma, beta, eps))
    if keep is not None:
        y = y * keep.to(y.dtype) / (1.0 - p)
    return y


def rel_err(got, ref):
    """max over rows of max|got - ref| / max|ref[row]| (a vector counts as one row); ref in float64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if ref.dim() < 2:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    scale = ref.abs().amax(dim=1, keepdim=True)
    diff = (got - ref).abs()
    exact = (scale == 0) & (diff.amax(dim=1, keepdim=True) == 0)         # an all-zero row reproduced exactly
    return float((diff / torch.where(exact, torch.ones_like(scale), scale)).max()) if ref.numel() else 0.0


def within(err, err32):
    """The project's form for kernels against torch's own float32 (tests/test_gpu_kernels.py:341-350)."""
    return err <= max(2 * err32, 8 * EPS24)


class Masks:
    """Keep masks in the order the modules consume them; `draw(shape, p)` is given by the caller (product masks by seed)."""

    def __init__(self, masks=None):
        self.masks = list(masks or [])

    def pop(self):
        return self.masks.pop(0) if self.masks else None


def seq_forward(sd, prefix, x, training, p_of, masks):
    """A getMLP stack (utils.py:885-908) from its state_dict entries `prefix + '<i>.weight'`: Linear at 0, 4, 8, ..., LayerNorm at 1, 5, ...;
    p_of(i) = dropout probability of the Dropout child i (None if there is none)."""
    idx = sorted({int(k[len(prefix):].split('.')[0]) for k in sd if k.startswith(prefix) and k[len(prefix):].split('.')[0].isdigit()})
    if not idx:                                # a single Linear (len(neurons) == 2)
        return F.linear(x, sd[prefix + 'weight'], sd.get(prefix + 'bias'))
    linears = [i for i in idx if i % 4 == 0]
    for i in linears:
        x = F.linear(x, sd[f'{prefix}{i}.weight'], sd.get(f'{prefix}{i}.bias'))
        if i + 1 in idx:
            p = p_of(i + 3) or 0.0
            keep = masks.pop() if (training and p > 0) else None
            x = ln_gelu_drop(x, sd[f'{prefix}{i + 1}.weight'], sd[f'{prefix}{i + 1}.bias'], 1e-5, keep, p)
    p_last = p_of(linears[-1] + 1)
    if p_last is not None and training and p_last > 0:
        x = x * masks.pop().to(x.dtype) / (1.0 - p_last)
    return x


def module_forward(module, sd, prefix, x, training, masks):
    """Restatement of a built student part (StudentSequential, HipLinear or BlockResMLP) from `sd` (float64 tensors, may require grad)."""
    import torch.nn as nn

    def p_of_seq(seq):
        return lambda i: (seq[i].p if i < len(seq) and isinstance(seq[i], nn.Dropout) else None)

    if hasattr(module, 'blocks'):
        if prefix + 'in_proj.weight' in sd:
            x = F.linear(x, sd[prefix + 'in_proj.weight'], sd[prefix + 'in_proj.bias'])
        for b, block in enumerate(module.blocks):
            x = x + seq_forward(sd, f'{prefix}blocks.{b}.', x, training, p_of_seq(block), masks)
        if prefix + 'out_proj.weight' in sd:
            x = F.linear(x, sd[prefix + 'out_proj.weight'], sd[prefix + 'out_proj.bias'])
        return x
    if isinstance(module, nn.Sequential):
        return seq_forward(sd, prefix, x, training, p_of_seq(module), masks)
    return seq_forward(sd, prefix, x, training, lambda i: None, masks)


def replacement(le_guess, teacher_se, k):
    """SEMLP.replacement (MLP_model/__init__.py:143-156) for all rows."""
    attn = le_guess @ teacher_se.t()
    val, sel = attn.topk(k, dim=1)
    w = torch.softmax(val, dim=1)
    return (w.unsqueeze(-1) * teacher_se[sel]).sum(1), sel, val


# ---------------------------------------------------------------------------------------------------------------------
# stand-in teacher and trainer set-up of the golden cases
# ---------------------------------------------------------------------------------------------------------------------
class _SE:
    def __init__(self, se):
        self.se = se

    def collect_SE(self, x, edge_index):
        return self.se.clone()

    def get_se_dim(self, x, edge_index):
        return self.se.shape[1]


class StandInTeacher:
    """What train_seMLP_part1 touches of a teacher: model.model.collect_SE / get_se_dim (a fixed matrix), train()."""

    def __init__(self, se):
        self.model = type('M', (), {})()
        self.model.model = _SE(se)

    def train(self, mode=True):
        return self


def load_case(name):
    return torch.load(os.path.join(GOLDEN, name + '.pt'), weights_only=False)


def student_args(g, extra=()):
    """The product's option pipeline for a golden case (its argv is stored in the fixture)."""
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.utils import set_arch_configs
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(list(g['argv']) + list(extra))
    for k, v in g['args_set'].items():
        setattr(args, k, v)
    set_arch_configs(args)
    for k, v in g['args_after'].items():
        setattr(args, k, v)
    return args


def student_trainer(g, device, workdir, extra=()):
    """trainer.__new__ with hand-set fields, as the fixture generator drives the reference (tests/golden/make_student_golden.py)."""
    from gnn_tail_generalization_amd import optim
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    dev = torch.device(device)
    args = student_args(g, extra)
    args.device = dev
    data = type('Data', (), {})()
    data.x, data.y = g['x'].to(dev), g['y'].to(dev)
    data.edge_index = g['edge_index'].to(dev)
    data.train_mask, data.test_mask = g['train_mask'].to(dev), (~g['train_mask']).to(dev)
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    for k in ('zero_deg_idx', 'small_deg_idx', 'large_deg_idx'):
        setattr(data, k, g[k].numpy())
    t = trainer.__new__(trainer)
    t.args, t.data, t.device, t.epochs, t.bag = args, data, dev, g['epochs'], {}
    t.optfun = optim.resolve(args.optfun)
    t.modeldir, t.resdir = os.path.join(workdir, 'models'), 'student_case'
    os.makedirs(t.modeldir, exist_ok=True)
    t.teacherGNN = StandInTeacher(g['teacherSE'].to(dev)) if g.get('teacherSE') is not None else None
    t.train_teacherGNN = lambda: None
    t.load_teacherGNN = lambda keyw='': None
    return t


def run_case(g, device, workdir, no_block_dropout=True):
    """Runs the case's trainers the way main() dispatches them; returns (trainer, part-1 rows or None, part-2 rows, states after each build).
    no_block_dropout: the fixture was written with every nn.Dropout switched off (see make_student_golden.py: BlockResMLP hard-codes
    p = 0.1 and torch's dropout stream cannot be matched by a counter-based generator); the built modules get p = 0 likewise."""
    import torch.nn as nn
    from gnn_tail_generalization_amd import MLP_model
    built = {}

    def on_build(name, module):
        init = {k[len(name) + 1:]: v for k, v in g['sd_after_' + name].items() if k.startswith(name + '.')}
        mine = module.state_dict()
        assert set(mine) == set(init), (sorted(mine), sorted(init))
        built[name] = all(torch.equal(mine[k].cpu(), init[k]) for k in init)
        module.load_state_dict({k: v.to(device) for k, v in init.items()}, strict=True)
        if no_block_dropout:
            for m in module.modules():
                if isinstance(m, nn.Dropout):
                    m.p = 0.0

    t = student_trainer(g, device, workdir)
    real = MLP_model.SEMLP

    class Hooked(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.on_build = on_build

    from gnn_tail_generalization_amd import trainer_node_classification as tn
    cwd = os.getcwd()
    os.chdir(workdir)
    tn.SEMLP = Hooked
    try:
        torch.manual_seed(g['seed'])
        np.random.seed(g['seed'])
        rows1 = None
        with contextlib.redirect_stdout(io.StringIO()):
            if g['train_which'] == 'StudentBaseMLP':
                t.args.SEMLP__downgrade_to_MLP = 1
            if g['train_which'] == 'SEMLP' and not t.args.SEMLP__downgrade_to_MLP:
                rows1 = t.train_seMLP_part1()
            rows2 = t.train_seMLP_part2()
    finally:
        tn.SEMLP = real
        os.chdir(cwd)
    return t, rows1, rows2, built
