"""Times the student MLP path at an ogbn-arxiv-like shape (N = 169 343, F = 128, batch 65 536, teacher width 2 * 256 + 40 = 552: what
collect_SE gives for L = 3, H = 256, C = 40), each item once on the HIP row kernel (cb_ln_gelu_drop_*) and once with the row stage
forced through torch's operators (F.layer_norm -> F.gelu -> ops.dropout) in the same process, alternating, median and spread of
`--rounds` rounds:
  (a) the two row kernels alone (forward, backward) at [65 536, 256], with achieved bytes/s on the byte model of DESIGN.md §3
      (forward 8 d + 8 B per row + 8 d B of parameters, backward 12 d + 8 B per row);
  (b) one part-1 step (forward, MSE, backward, Adam);  (c) one part-2 step with its replacement;
  (d) one epoch's head + tail evaluation (two eval-mode forward_part2 over N / 8 nodes each).
usage: python tools/bench_student.py [--rounds 7] [--nodes 169343] [--batch 65536]
Needs an MI355X: there is no CPU path."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gnn_tail_generalization_amd import MLP_model, ops, optim  # noqa: E402
from gnn_tail_generalization_amd.base_options import BaseOptions  # noqa: E402
from gnn_tail_generalization_amd.utils import set_arch_configs  # noqa: E402

DEV = 'cuda:0'


def torch_rows_forward(self, x):
    """StudentSequential.forward with the row stage on torch's operators (the yardstick; never used by the package itself)."""
    for m in self:
        if isinstance(m, nn.LayerNorm):
            x = F.layer_norm(x, m.normalized_shape, m.weight, m.bias, m.eps)
        elif isinstance(m, nn.GELU):
            x = F.gelu(x)
        elif isinstance(m, nn.Dropout):
            x = ops.dropout(x, m.p, self.training, seed=MLP_model.next_seed() if (self.training and m.p > 0) else None)
        else:
            x = m(x)
    return x


@contextlib.contextmanager
def row_stage(which):
    real = MLP_model.StudentSequential.forward
    if which == 'torch':
        MLP_model.StudentSequential.forward = torch_rows_forward
    try:
        yield
    finally:
        MLP_model.StudentSequential.forward = real


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def ab(name, fns, rounds, inner, extra=None):
    """fns: {'hip': fn, 'torch': fn}; alternates the two within every round."""
    for fn in fns.values():
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, inner))
    rec = {'item': name}
    for k, v in ms.items():
        rec[k + '_ms_median'], rec[k + '_ms_min'], rec[k + '_ms_max'] = statistics.median(v), min(v), max(v)
    rec['torch_over_hip'] = rec['torch_ms_median'] / rec['hip_ms_median']
    if extra:
        rec.update(extra(rec))
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--nodes', type=int, default=169343)
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--se_dim', type=int, default=552)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_student.py needs an MI355X (no CPU path)')
    assert a.rounds >= 5
    N, B, Fd, D, C = a.nodes, a.batch, 128, a.se_dim, 40
    g = torch.Generator().manual_seed(0)
    # (a) the row kernels alone
    d, p, seed = 256, 0.2, 1234
    z = torch.randn(B, d, generator=g).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    dy = torch.randn(B, d, generator=g).to(DEV)
    out, stats = ops._ln_gelu_drop_fwd_raw(z, gamma, beta, 1e-5, p, seed, True)
    fwd_bytes, bwd_bytes = B * (8 * d + 8) + 8 * d, B * (12 * d + 8)

    def torch_fwd():
        return ops._dropout_raw(F.gelu(F.layer_norm(z, (d,), gamma, beta, 1e-5)), p, seed)

    zt, gt, bt = (t.clone().requires_grad_(True) for t in (z, gamma, beta))
    yt = ops.dropout(F.gelu(F.layer_norm(zt, (d,), gt, bt, 1e-5)), p, True, seed=seed)

    def torch_bwd():
        return torch.autograd.grad(yt, (zt, gt, bt), dy, retain_graph=True)

    ab('row_forward[65536x256,p=0.2]', {'hip': lambda: ops._ln_gelu_drop_fwd_raw(z, gamma, beta, 1e-5, p, seed, True), 'torch': torch_fwd}, a.rounds, 50,
       lambda r: {'hip_TBps': fwd_bytes / r['hip_ms_median'] / 1e9, 'model_bytes': fwd_bytes})
    ab('row_backward[65536x256,p=0.2]', {'hip': lambda: ops._ln_gelu_drop_bwd_raw(dy, z, stats, gamma, beta, p, seed, True), 'torch': torch_bwd}, a.rounds, 50,
       lambda r: {'hip_TBps': bwd_bytes / r['hip_ms_median'] / 1e9, 'model_bytes': bwd_bytes, 'note': 'torch side has no bias column sum'})
    del out, z, dy, zt, yt
    # (b)-(d) the trainer's steps
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(['--dataset=S-arxiv', '--train_which=SEMLP', '--manual_assign_GPU=0', f'--batch_size={B}', '--use_special_split=0'])
    args.num_feats, args.num_classes, args.N_nodes, args.device = Fd, C, N, torch.device(DEV)
    set_arch_configs(args)
    data = type('Data', (), {})()
    data.x = torch.rand(N, Fd, generator=g).to(DEV)
    data.y = torch.randint(0, C, (N,), generator=g).to(DEV)
    data.train_mask = (torch.rand(N, generator=g) < 0.54).to(DEV)
    data.test_mask = ~data.train_mask
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    se = torch.randn(N, D, generator=g).to(DEV)
    teacher = type('T', (), {})()
    teacher.model = type('M', (), {})()
    teacher.model.model = type('S', (), {'get_se_dim': staticmethod(lambda x, ei: D)})()
    rs = np.random.RandomState(0)
    train_idx, perm = data.train_idx.cpu().numpy(), rs.permutation(N)
    batch = rs.choice(train_idx, B)
    head, tail = np.sort(perm[:N // 8]), np.sort(perm[N // 8:N // 4])
    models = {}
    for which in ('hip', 'torch'):
        torch.manual_seed(0)
        m = MLP_model.SEMLP(args, data, teacher).to(DEV)
        m.optfun, m.teacherSE = optim.resolve(args.optfun), se
        with row_stage(which):
            m.build_part1(D)
            m.build_part2(Fd + 2 * D)
        models[which] = m

    def part1_step(which):
        m = models[which]
        with row_stage(which):
            m.train()
            o = m.forward_part1(data.x, batch_idx=batch)
            loss = ops.mse_rows(o, se, m.index_on_device(batch, o.device))
            m.opt.zero_grad()
            loss.backward()
            m.opt.step()

    def part2_step(which):
        m = models[which]
        with row_stage(which):
            m.train()
            o = m.forward_part2(data.x, batch_idx=batch)
            idx = m.index_on_device(batch, o.device)
            loss = ops.nll_logsoftmax(o, data.y[idx].contiguous(), None, B)
            m.opt.zero_grad()
            loss.backward()
            m.opt.step()

    def headtail(which):
        m = models[which]
        with row_stage(which), torch.no_grad():
            m.eval()
            for idx in (head, tail):
                m.forward_part2(data.x, batch_idx=idx)

    ab('part1_step', {k: (lambda k=k: part1_step(k)) for k in models}, a.rounds, 10)
    ab('part2_step_with_replacement', {k: (lambda k=k: part2_step(k)) for k in models}, a.rounds, 3)
    ab('head_tail_eval', {k: (lambda k=k: headtail(k)) for k in models}, a.rounds, 2)


if __name__ == '__main__':
    main()
