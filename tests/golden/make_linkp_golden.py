"""Generates the link-prediction fixtures from the *unmodified* reference (build container only):

    python tests/golden/make_linkp_golden.py

  tests/golden/linkp_<case>.pt   inputs (emb [N, D] float32, pos [2, P], neg [2, Nn] int64) and what the reference's utils.linkp_loss_eva /
                                 utils.cal_MRR make of emb[pos[0]], emb[pos[1]], emb[neg[0]], emb[neg[1]] on the CPU: loss (float32), mrr (Python
                                 float), and emb.grad of loss.backward().  (`gen_pn_edges` itself cannot run here: PyG's negative_sampling is
                                 stubbed absent; the samplers are tested against tests/linkp_ref.py.)

Cases: (N, D, P, Nn) = (50, 10, 7, 30): k = 4 negatives per positive, two dropped; (50, 7, 5, 3): k = 0, MRR 1.0; (300, 256, 64, 1280); and a
hub case in which node 0 takes part in at least 100 contributions and one positive is a self loop.  Inputs are drawn so that no negative score
comes within four float32 summation bounds (gamma_D * max sum|h t|) of its positive's (otherwise the maker takes its next seed): the reference's rank then depends neither
on the stability of its sort nor on the order of a float32 summation.  Fixtures are data only."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import linkp_ref as lr  # noqa: E402
import ref_import  # noqa: E402

CASES = [
    dict(name='linkp_n50_d10_p7_n30', N=50, D=10, P=7, Nn=30, seed=1),
    dict(name='linkp_n50_d7_p5_n3_k0', N=50, D=7, P=5, Nn=3, seed=2),
    dict(name='linkp_n300_d256_p64_n1280', N=300, D=256, P=64, Nn=1280, seed=3, scale=0.08),
    dict(name='linkp_hub_selfloop', N=40, D=12, P=70, Nn=140, seed=4, hub=True),
]


class Rejected(Exception):
    pass


def make_inputs(c, seed):
    g = torch.Generator().manual_seed(8100 + seed)
    emb = torch.randn(c['N'], c['D'], generator=g) * c.get('scale', 0.5)
    pos = torch.randint(0, c['N'], (2, c['P']), generator=g)
    neg = torch.randint(0, c['N'], (2, c['Nn']), generator=g)
    if c.get('hub'):
        pos[0, ::2] = 0                  # node 0: the head of every second positive ...
        neg[1, ::2] = 0                  # ... and the tail of every second negative
        pos[:, 1] = 5                    # a self-loop positive (two contributions to one row)
        pos[:, 2] = 0                    # and one on the hub itself
    return emb, pos, neg


def run_case(ns, c, seed):
    emb, pos, neg = make_inputs(c, seed)
    e = emb.clone().requires_grad_(True)
    loss, mrr = ns.utils.linkp_loss_eva(e[pos[0]], e[pos[1]], e[neg[0]], e[neg[1]])
    loss.backward()
    ps, nsc = lr.scores64(emb, pos), lr.scores64(emb, neg)
    k = c['Nn'] // c['P']
    grp = nsc[:k * c['P']].reshape(c['P'], k)
    # each float32 score is within gamma_D * sum|h t| of the float64 one in any summation order: with a gap of twice the sum of the two bounds, float32 ranks as float64 does
    margin = 4 * lr.gamma(c['D']) * float(max(lr.abs_dot(emb, pos).max(), lr.abs_dot(emb, neg).max()))
    if k and float((grp - ps.reshape(-1, 1)).abs().min()) <= margin:
        raise Rejected('a negative ties (or nearly ties) its positive')
    ps32 = (emb[pos[0]] * emb[pos[1]]).sum(-1)
    ns32 = (emb[neg[0]] * emb[neg[1]]).sum(-1)
    assert not bool((ns32[:k * c['P']].reshape(c['P'], k) == ps32.reshape(-1, 1)).any()), 'a negative ties its positive in float32'
    assert float(ns.utils.cal_MRR(ps32, ns32)) == float(mrr)
    mrr64, rank = lr.mrr_exact(ps, nsc)
    assert abs(mrr64 - float(mrr)) < 1e-12, (mrr64, mrr)
    if c.get('hub'):
        touches = int((pos == 0).sum() + (neg == 0).sum())
        assert touches >= 100 and bool((pos[0] == pos[1]).any()), touches
    if k == 0:
        assert float(mrr) == 1.0
    return dict(name=c['name'], seed=seed, emb=emb, pos=pos, neg=neg, loss=loss.detach().clone(), mrr=float(mrr), rank=rank.clone(), grad=e.grad.detach().clone())


def main():
    ns = ref_import.load_reference()
    torch.set_num_threads(1)
    for c in CASES:
        for seed in range(c['seed'], c['seed'] + 400, 10):
            try:
                out = run_case(ns, c, seed)
            except Rejected as e:
                print(c['name'], 'seed', seed, 'rejected:', e)
                continue
            break
        else:
            raise SystemExit(f'{c["name"]}: no seed passes the checks')
        path = os.path.join(HERE, c['name'] + '.pt')
        torch.save(out, path)
        print('wrote', path, os.path.getsize(path), 'bytes; loss', float(out['loss']), 'mrr', out['mrr'])


if __name__ == '__main__':
    main()
