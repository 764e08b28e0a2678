"""Generates the GraphMLP fixtures from the *unmodified* reference (build container only):

    python tests/golden/make_graphmlp_golden.py

  tests/golden/graphutils_<graph>.pt   utils.graphUtils.normalize_adj / sparse_power (r = 2, 3) / crop_adj_to_subgraph on the two graphs of the
                                       kernel tests and on a graph with self loops and multi-edges in its input.  A coalesced matrix is stored as
                                       its pattern (bool [n, n]) and its values in row-major order, which is the order of its indices.
  tests/golden/graphmlp_<case>.pt      the reference's SEMLP(..., teacherGNN=None) / GraphMLP / train_seMLP_part2 with --train_which=GraphMLP, driven
                                       the way make_student_golden.py drives the students: N = 150, F = 20, C = 4, 5 epochs, batch 32;
                                       nn.Dropout.forward is the identity while recording (torch's dropout stream cannot be matched by a
                                       counter-based generator; GraphMLP hard-codes p = 0.6).

While a model fixture is written, the maker asserts — and otherwise takes its next seed — that the reference's cropped matrix equals the
last-occurrence rule on every recorded batch, that at least one training batch has duplicates, that M >= 1 in every epoch, and the
logit-gap condition of make_student_golden.py (no argmax may flip under a float32 rounding).  Fixtures are data only."""
import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import ncloss_ref as nr  # noqa: E402
import ref_import  # noqa: E402
import student_ref as sr  # noqa: E402

N, F_, C, BATCH, EPOCHS = 150, 20, 4, 32, 5

CASES = [
    dict(name='graphmlp_powerlaw_tau2_r3_reg10', graph='powerlaw', tau=2.0, r=3, reg=10.0, want_headtail=1),
    dict(name='graphmlp_asym_multi_tau05_r2_reg1', graph='asym_multi', tau=0.5, r=2, reg=1.0, want_headtail=0),
]


class Rejected(Exception):
    pass


def pack(sp):
    sp = sp.coalesce()
    pattern = torch.zeros(tuple(sp.shape), dtype=torch.bool)
    pattern[sp.indices()[0], sp.indices()[1]] = True
    assert torch.equal(pattern.nonzero().t(), sp.indices())
    return pattern, sp.values().clone()


def loops_multi_graph():
    ei, n = mg.make_graph('asym_multi', 100, 5)
    g = torch.Generator().manual_seed(9)
    loops = torch.randint(0, n, (25,), generator=g)
    dup = torch.randint(0, ei.shape[1], (40,), generator=g)
    ei = torch.cat([ei, torch.stack([loops, loops]), ei[:, dup], torch.stack([loops[:5], loops[:5]])], dim=1)
    return ei[:, torch.randperm(ei.shape[1], generator=g)], n


def write_graphutils(ns):
    gu = ns.utils.graphUtils
    graphs = {name: mg.make_graph(*spec) for name, spec in nr.GRAPHS.items()}
    graphs['loops_multi'] = loops_multi_graph()
    for name, (ei, n) in graphs.items():
        assert int(ei.max()) + 1 == n
        adj = gu.normalize_adj(ei)
        out = dict(edge_index=ei, shape=(n, n))
        out['adj_pattern'], out['adj_val'] = pack(adj)
        for r in (2, 3):
            out[f'pow{r}_pattern'], out[f'pow{r}_val'] = pack(gu.sparse_power(adj, r))
        sub = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:n // 3]
        out['subset'] = sub
        out['crop_pattern'], out['crop_val'] = pack(gu.crop_adj_to_subgraph(gu.sparse_power(adj, 2), sub))
        path = os.path.join(HERE, f'graphutils_{name}.pt')
        torch.save(out, path)
        print('wrote', path, os.path.getsize(path), 'bytes; nnz', int(out['adj_pattern'].sum()), int(out['pow2_pattern'].sum()), int(out['pow3_pattern'].sum()))


def make_inputs(c, seed):
    g = torch.Generator().manual_seed(6000 + seed)
    ei, n = mg.make_graph(c['graph'], N, seed)
    x = torch.rand(n, F_, generator=g)
    y = (x @ torch.randn(F_, C, generator=g)).argmax(1)
    train_mask = torch.rand(n, generator=g) < 0.5
    train_mask[0] = True
    deg = torch.bincount(ei[1], minlength=n)
    order = torch.argsort(deg, stable=True)
    return dict(x=x, y=y, edge_index=ei, train_mask=train_mask, zero_deg_idx=order[:10].clone(), small_deg_idx=order[10:40].clone(),
                large_deg_idx=order[-30:].clone())


def run_case(ns, c, seed):
    argv = ['--train_which=GraphMLP', f'--epochs={EPOCHS}', f'--batch_size={BATCH}', f'--want_headtail={c["want_headtail"]}', '--use_special_split=0']
    args = mg.ref_args(ns, 'Cora', argv)
    args_set = dict(N_nodes=N, num_feats=F_, num_classes=C, graphMLP_tau=c['tau'], graphMLP_r=c['r'], graphMLP_reg=c['reg'])
    for k, v in args_set.items():
        setattr(args, k, v)
    ns.utils.set_arch_configs(args)
    for k, v in args_set.items():
        setattr(args, k, v)
    inp = make_inputs(c, seed)
    Data = sys.modules['torch_geometric.data.data'].Data
    data = Data(x=inp['x'], y=inp['y'], edge_index=inp['edge_index'], train_mask=inp['train_mask'], test_mask=~inp['train_mask'])
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    for k in ('zero_deg_idx', 'small_deg_idx', 'large_deg_idx'):
        setattr(data, k, inp[k].numpy())
    t = ns.trainer.trainer.__new__(ns.trainer.trainer)
    t.args, t.data, t.device, t.epochs, t.bag = args, data, torch.device('cpu'), EPOCHS, {}
    rec = dict(batches=[], nc=[], emb=[], M=[], grads=None, sd_init=None)

    class RecAdam(torch.optim.Adam):
        def step(self, *a, **k):
            if rec['grads'] is None:
                rec['grads'] = {n_: p.grad.detach().clone() for n_, p in t.seMLP.named_parameters() if p.grad is not None}
            return super().step(*a, **k)

    assert args.optfun == 'torch.optim.Adam'
    t.optfun = RecAdam
    t.modeldir, t.resdir = 'graphmlp_models', 'student_case'
    import MLP_model as ref_mlp
    GraphMLP = ref_mlp.GraphMLP
    real_fwd, real_rec, real_drop = GraphMLP.forward, ns.trainer.wzRec, nn.Dropout.forward
    recs = {}

    def forward(self, x, edge_index=None, batch_idx=None):
        if rec['sd_init'] is None:
            rec['sd_init'] = {k: v.detach().clone() for k, v in self.state_dict().items()}
        info = real_fwd(self, x, edge_index=edge_index, batch_idx=batch_idx)
        with torch.no_grad():
            z = self.model(x)                                  # (pure: dropout is the identity here)
            top2 = info.emb.detach().topk(2, dim=1)[0]
            gap = (top2[:, 0] - top2[:, 1]).double()
            w = self.out_proj.weight.detach().double()
            bound = w.shape[1] * sr.EPS24 * z.double().norm(dim=1) * w.norm(dim=1).max()
            if bool((gap < 100 * bound).any()):
                raise Rejected(f'argmax margin {float((gap / bound).min()):.1f} x bound')
            bi = torch.as_tensor(np.asarray(batch_idx), dtype=torch.long)
            want = nr.crop_dense(self.adj_pow, bi, torch.float32)
            got = ns.utils.graphUtils.crop_adj_to_subgraph(self.adj_pow, batch_idx).to_dense()
            if not torch.equal(got, want):
                raise Rejected('the cropped matrix is not the last-occurrence rule')
            if self.training:
                _, _, _, nz = nr.parts(z.double(), want.double(), self.args.graphMLP_tau)
                if len(nz) < 1:
                    raise Rejected('M == 0')
                rec['batches'].append(bi.clone())
                rec['nc'].append(info.loss_NContrastive.detach().clone())
                rec['emb'].append(info.emb.detach().clone())
                rec['M'].append(len(nz))
        return info

    def wzRec(datas, ttl='', **kw):
        recs[ttl.split('@')[0]] = torch.as_tensor(np.asarray(datas), dtype=torch.float64).clone()
        return real_rec(datas, ttl, **kw)

    GraphMLP.forward, ns.trainer.wzRec = forward, wzRec
    nn.Dropout.forward = lambda self, x: x
    try:
        with ref_import.in_scratch(), contextlib.redirect_stdout(io.StringIO()):
            os.makedirs(t.modeldir, exist_ok=True)
            torch.manual_seed(seed)
            np.random.seed(seed)
            args.SEMLP__downgrade_to_MLP = 1                   # main(), trainer_node_classification.py:27-29
            rows2 = t.train_seMLP_part2()
            sd_final = {k: v.detach().clone() for k, v in t.seMLP.state_dict().items()}
    finally:
        GraphMLP.forward, ns.trainer.wzRec = real_fwd, real_rec
        nn.Dropout.forward = real_drop
    if not any(len(torch.unique(b)) < len(b) for b in rec['batches']):
        raise Rejected('no training batch with duplicates')
    assert len(rec['batches']) == EPOCHS
    loss_train = torch.stack([F.cross_entropy(e, inp['y'][b]) + n_ * args.graphMLP_reg for e, b, n_ in zip(rec['emb'], rec['batches'], rec['nc'])])
    out = dict(inp)
    out.update(name=c['name'], argv=['--dataset=Cora', '--manual_assign_GPU=0'] + argv, train_which='GraphMLP', seed=seed, epochs=EPOCHS,
               args_set=args_set, teacherSE=None,
               args_after=dict(lr=float(args.lr), weight_decay=float(args.weight_decay), batch_size=int(args.batch_size), optfun=str(args.optfun),
                               graphMLP_tau=float(args.graphMLP_tau), graphMLP_r=int(args.graphMLP_r), graphMLP_reg=float(args.graphMLP_reg)),
               sd_init=rec['sd_init'], sd_final=sd_final, rows_part2=torch.as_tensor(rows2, dtype=torch.float64), acc_test=recs.get('acc_test'),
               batches=torch.stack(rec['batches']), loss_nc=torch.stack(rec['nc']).double(), emb0=rec['emb'][0], M=rec['M'],
               loss_train=loss_train.double(), grads0=rec['grads'])
    return out


def main():
    ns = ref_import.load_reference()
    torch.set_num_threads(1)
    write_graphutils(ns)
    for ci, c in enumerate(CASES):
        for seed in range(3 + 20 * ci, 60 + 20 * ci):
            try:
                out = run_case(ns, c, seed)
            except Rejected as e:
                print(c['name'], 'seed', seed, 'rejected:', e)
                continue
            again = run_case(ns, c, seed)
            assert all(torch.equal(out['sd_final'][k], again['sd_final'][k]) for k in out['sd_final']) and torch.equal(out['rows_part2'], again['rows_part2'])
            path = os.path.join(HERE, c['name'] + '.pt')
            torch.save(out, path)
            print('wrote', c['name'], 'seed', seed, os.path.getsize(path), 'bytes; acc', out['rows_part2'][0].tolist(), 'loss', out['loss_train'].tolist(),
                  'nc', out['loss_nc'].tolist(), 'M', out['M'], 'duplicates', [len(b) - len(torch.unique(b)) for b in out['batches']])
            break
        else:
            raise SystemExit(f'{c["name"]}: no seed passes the checks')


if __name__ == '__main__':
    main()
