"""Generates the student-MLP fixtures tests/golden/student_*.pt from the *unmodified* reference (build container only).

    python tests/golden/make_student_golden.py

Each case drives the reference's own trainer.train_seMLP_part1 / train_seMLP_part2 the way make_golden.run_trainer_case drives
run_trainSet: trainer.__new__, args through the reference's option pipeline + set_arch_configs, hand-set data / device / epochs /
optfun / modeldir / resdir, a stand-in teacher whose model.model.collect_SE / get_se_dim return a seeded matrix, and
train_teacherGNN / load_teacherGNN replaced by no-ops on the instance.

All cases run with --dropout_MLP=0, so that the trajectory is a function of the weights and the batches.  BlockResMLP does not
take that option: it builds its blocks with a hard-coded p = 0.1 (MLP_model/__init__.py:23,38-39), and torch's dropout stream
cannot be reproduced by the product's counter-based generator.  nn.Dropout.forward is therefore the identity while a case runs
(no mask is drawn, no generator state consumed); tests/student_ref.run_case sets p = 0 on the product's built modules likewise.

While a fixture is written, every recorded forward is checked for decisions a float32 rounding could flip: the gap between the
largest two logits of every row, and the gap between the K-th and (K+1)-th replacement score, must be at least 100 x the float32
error bound of the dot product behind them (D 2^-24 |q| |t|).  A case that fails this picks its next seed.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import ref_import  # noqa: E402
import student_ref as sr  # noqa: E402

N, F_, SE_DIM, C, BATCH, EPOCHS = 120, 20, 36, 4, 32, 5

CASES = [
    dict(name='student_semlp_2layer_headtail_iso', train_which='SEMLP', extra=['--SEMLP_part1_arch=2layer'], want_headtail=1, special=1),
    dict(name='student_semlp_residual', train_which='SEMLP', extra=['--SEMLP_part1_arch=residual'], want_headtail=1, special=0),
    dict(name='student_semlp_downgraded', train_which='SEMLP', extra=['--SEMLP_topK_2_replace=-99'], want_headtail=0, special=0),
    dict(name='student_basemlp', train_which='StudentBaseMLP', extra=[], want_headtail=1, special=0),
]


class TooClose(Exception):
    pass


def make_inputs(seed):
    g = torch.Generator().manual_seed(4000 + seed)
    ei, n = mg.make_graph('powerlaw', N, seed)
    x = torch.rand(n, F_, generator=g)
    y = (x @ torch.randn(F_, C, generator=g)).argmax(1)
    se = torch.tanh(x @ torch.randn(F_, SE_DIM, generator=g)) + 0.1 * torch.randn(n, SE_DIM, generator=g)
    train_mask = torch.rand(n, generator=g) < 0.5
    train_mask[0] = True
    deg = torch.bincount(ei[1], minlength=n)
    order = torch.argsort(deg, stable=True)
    return dict(x=x, y=y, edge_index=ei, teacherSE=se, train_mask=train_mask, zero_deg_idx=order[:10].clone(),
                small_deg_idx=order[10:40].clone(), large_deg_idx=order[-30:].clone())


def run_student_case(ns, c, seed):
    argv = [f'--train_which={c["train_which"]}', '--dropout_MLP=0', f'--epochs={EPOCHS}', f'--batch_size={BATCH}',
            f'--want_headtail={c["want_headtail"]}', f'--use_special_split={c["special"]}'] + c['extra']
    args = mg.ref_args(ns, 'Cora', argv)
    # (a narrow residual model: three state_dicts of the default width would not fit a fixture file)
    args_set = dict(N_nodes=N, num_feats=F_, num_classes=C, StudentMLP__dim_model=32, studentMLP__skip_conn_T_and_res_blks='2&3')
    for k, v in args_set.items():
        setattr(args, k, v)
    ns.utils.set_arch_configs(args)
    inp = make_inputs(seed)
    Data = sys.modules['torch_geometric.data.data'].Data
    data = Data(x=inp['x'], y=inp['y'], edge_index=inp['edge_index'], train_mask=inp['train_mask'], test_mask=~inp['train_mask'])
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    for k in ('zero_deg_idx', 'small_deg_idx', 'large_deg_idx'):
        setattr(data, k, inp[k].numpy())
    t = ns.trainer.trainer.__new__(ns.trainer.trainer)
    t.args, t.data, t.device, t.epochs, t.bag = args, data, torch.device('cpu'), EPOCHS, {}
    t.optfun = torch.optim.Adam if args.optfun == 'torch.optim.Adam' else torch.optim.SGD
    t.modeldir, t.resdir = 'student_models', 'student_case'
    t.teacherGNN = sr.StandInTeacher(inp['teacherSE'])
    t.train_teacherGNN = lambda: None
    t.load_teacherGNN = lambda keyw='': None

    SEMLP = ns.trainer.SEMLP
    snaps, recs, state = {}, {}, {'hook': None, 'h': None}
    real_p1, real_p2, real_rep, real_rec, real_drop = SEMLP.forward_part1, SEMLP.forward_part2, SEMLP.replacement, ns.trainer.wzRec, nn.Dropout.forward

    def snap(m):
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    def forward_part1(self, *a, **k):
        out = real_p1(self, *a, **k)
        snaps.setdefault('sd_after_part1', {k: v for k, v in snap(self).items() if k.startswith('part1.')})
        return out

    def forward_part2(self, *a, **k):
        out = real_p2(self, *a, **k)
        if 'sd_after_part2' not in snaps:
            snaps['sd_after_part2'] = {k: v for k, v in snap(self).items() if k.startswith('part2.')}
            last = [m for m in self.part2.modules() if isinstance(m, nn.Linear)][-1]
            state['w'] = last
            last.register_forward_pre_hook(lambda mod, inp_: state.__setitem__('h', inp_[0].detach()))
            out = real_p2(self, *a, **k)          # (pure: no dropout, no running statistics) once more, with the hook in place
        top2 = out.detach().topk(2, dim=1)[0]
        gap = (top2[:, 0] - top2[:, 1]).double()
        h, w = state['h'].double(), state['w'].weight.detach().double()
        bound = w.shape[1] * sr.EPS24 * h.norm(dim=1) * w.norm(dim=1).max()
        if bool((gap < 100 * bound).any()):
            raise TooClose(f'argmax margin {float((gap / bound).min()):.1f} x bound')
        return out

    def replacement(self, le_guess, node_idx=None):
        q, se, K = le_guess.detach().double(), self.teacherSE.double(), self.topK_2_replace
        val = (q @ se.t()).topk(K + 1, dim=1)[0]
        gap = val[:, K - 1] - val[:, K]
        bound = se.shape[1] * sr.EPS24 * q.norm(dim=1) * se.norm(dim=1).max()
        if bool((gap < 100 * bound).any()):
            raise TooClose(f'top-K gap {float((gap / bound).min()):.1f} x bound')
        return real_rep(self, le_guess, node_idx)

    def wzRec(datas, ttl='', **kw):
        recs[ttl.split('@')[0]] = torch.as_tensor(np.asarray(datas), dtype=torch.float64).clone()
        return real_rec(datas, ttl, **kw)

    SEMLP.forward_part1, SEMLP.forward_part2, SEMLP.replacement, ns.trainer.wzRec = forward_part1, forward_part2, replacement, wzRec
    nn.Dropout.forward = lambda self, x: x
    rows1 = None
    try:
        with ref_import.in_scratch(), contextlib.redirect_stdout(io.StringIO()):
            os.makedirs(t.modeldir, exist_ok=True)
            torch.manual_seed(seed)
            np.random.seed(seed)
            if c['train_which'] == 'StudentBaseMLP':
                args.SEMLP__downgrade_to_MLP = 1
            if c['train_which'] == 'SEMLP' and not args.SEMLP__downgrade_to_MLP:
                rows1 = t.train_seMLP_part1()
            rows2 = t.train_seMLP_part2()
            sd_final = snap(t.seMLP)
    finally:
        SEMLP.forward_part1, SEMLP.forward_part2, SEMLP.replacement, ns.trainer.wzRec = real_p1, real_p2, real_rep, real_rec
        nn.Dropout.forward = real_drop
    out = dict(inp)
    if rows1 is None:
        out['teacherSE'] = None
    out.update(snaps)
    out.update(name=c['name'], argv=['--dataset=Cora', '--manual_assign_GPU=0'] + argv, train_which=c['train_which'], seed=seed, epochs=EPOCHS,
               args_set=args_set,
               args_after=dict(lr=float(args.lr), weight_decay=float(args.weight_decay), batch_size=int(args.batch_size), optfun=str(args.optfun),
                               dropout_MLP=float(args.dropout_MLP), SEMLP_topK_2_replace=int(args.SEMLP_topK_2_replace),
                               SEMLP_part1_arch=str(args.SEMLP_part1_arch), StudentMLP__dim_model=int(args.StudentMLP__dim_model),
                               SEMLP__include_part1out=int(args.SEMLP__include_part1out)),
               student_cfg=dict(skip_conn_period=int(args.StudentBaseMLP.skip_conn_period), num_blocks=int(args.StudentBaseMLP.num_blocks),
                                dim_model=int(args.StudentBaseMLP.dim_model)),
               sd_final=sd_final, rows_part1=None if rows1 is None else torch.as_tensor(rows1, dtype=torch.float64),
               rows_part2=torch.as_tensor(rows2, dtype=torch.float64),
               loss_train=recs.get('loss_train'), loss_test=recs.get('loss_test'), acc_test=recs.get('acc_test'))
    return out


def main():
    ns = ref_import.load_reference()
    torch.set_num_threads(1)
    for c in CASES:
        for seed in range(3, 40):
            try:
                out = run_student_case(ns, c, seed)
            except TooClose as e:
                print(c['name'], 'seed', seed, 'rejected:', e)
                continue
            again = run_student_case(ns, c, seed)
            assert all(torch.equal(out['sd_final'][k], again['sd_final'][k]) for k in out['sd_final']) and torch.equal(out['rows_part2'], again['rows_part2'])
            path = os.path.join(HERE, c['name'] + '.pt')
            torch.save(out, path)
            print('wrote', c['name'], 'seed', seed, os.path.getsize(path), 'bytes; rows', out['rows_part2'][:, -1].tolist(),
                  None if out['loss_test'] is None else out['loss_test'].tolist())
            break
        else:
            raise SystemExit(f'{c["name"]}: no seed passes the margin checks')


if __name__ == '__main__':
    main()
