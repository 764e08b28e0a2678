"""Records tests/golden/linkpred_*.pt from the UNMODIFIED reference: the five losses of Link_prediction_model/loss.py and `MLPPredictor` /
`DotPredictor` of Link_prediction_model/layer.py.  Runs only where the reference tree exists (COLDBREW_REFERENCE_ROOT, or --reference PATH), on the
CPU; never from a test.  layer.py imports torch_geometric.nn and Link_prediction_baseline.heuristics at its top, which the two predictors do not
use: the files are loaded by path with stand-in modules for those imports, and no bytecode is written.

  linkpred_losses      scores uniform in [-20, 20] and in [-3, 3]; (P, k) in {(1, 1), (5, 3), (257, 7)}; per kind the fp32 result, the result on
                       .double() inputs and its float64 autograd gradients (upstream gradient 1)
  linkpred_predictors  h [50, 32] uniform in [-1, 1], 200 pairs (one node in 60 of them, self pairs, node N - 1); MLPPredictor(32, 32, 1, L, .)
                       for L = 1, 2, 3 in eval mode with dropout 0.5 and in train mode with dropout 0 (the same numbers): state_dict, the seed
                       it was constructed under, fp32 outputs and gradients, float64 outputs and gradients of sum(out * gout); DotPredictor
Before writing, every recording is compared with the restatement of tests/linkpred_ref.py.
    usage: python tools/gen_linkpred_golden.py [--reference PATH]"""
import argparse
import importlib.util
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import linkpred_ref as lr  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute exists (the names the reference imports and the recorded classes never touch)."""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


def _load(path, name, stand_ins):
    if not os.path.isfile(path):
        raise SystemExit(f'reference tree not found: {path}')
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def load_reference(root):
    loss = _load(os.path.join(root, 'Link_prediction_model', 'loss.py'), '_reference_lp_loss', {})
    names = ('torch_geometric', 'torch_geometric.nn', 'Link_prediction_baseline', 'Link_prediction_baseline.heuristics')
    layer = _load(os.path.join(root, 'Link_prediction_model', 'layer.py'), '_reference_lp_layer', {n: _Anything(n) for n in names})
    return loss, layer


def _call(loss_mod, kind, pos, neg, k, w):
    if kind == 'ce_loss':
        return loss_mod.ce_loss(pos, neg)
    if kind == 'adaptive_auc_loss':
        return loss_mod.adaptive_auc_loss(pos, neg, k, w)
    return getattr(loss_mod, kind)(pos, neg, k)


def record_losses(loss_mod):
    gen = torch.Generator().manual_seed(2024)
    cases = []
    for span in (20.0, 3.0):
        for P, k in ((1, 1), (5, 3), (257, 7)):
            pos = ((torch.rand(P, generator=gen) * 2 - 1) * span).float()
            neg = ((torch.rand(P * k, generator=gen) * 2 - 1) * span).float()
            w = (torch.rand(P, generator=gen) + 0.5).float()
            case = {'span': span, 'P': P, 'k': k, 'pos': pos, 'neg': neg, 'weight': w, 'kinds': {}}
            for kind in lr.KINDS:
                f32 = _call(loss_mod, kind, pos, neg, k, w).detach()
                p64, n64 = pos.double().requires_grad_(True), neg.double().requires_grad_(True)
                f64 = _call(loss_mod, kind, p64, n64, k, w.double())
                f64.backward()
                case['kinds'][kind] = {'f32': f32.clone(), 'f64': f64.detach().clone(), 'dpos64': p64.grad.clone(), 'dneg64': n64.grad.clone()}
                r, dp, dn = lr.rank_loss_grads64(kind, pos, neg, k, w)
                assert torch.equal(r, f64.detach()) and torch.equal(dp, p64.grad) and torch.equal(dn, n64.grad), (kind, span, P, k)
            cases.append(case)
            worst = max(abs(float(c['f32']) - float(c['f64'])) / max(abs(float(c['f64'])), 1e-300) for c in case['kinds'].values())
            print(f'losses span {span:g} P {P} k {k}: worst fp32 distance to float64 {worst:.3e} (relative)')
    out = os.path.join(ROOT, 'tests', 'golden', 'linkpred_losses.pt')
    torch.save(cases, out)
    print(f'linkpred_losses: {len(cases)} cases, {os.path.getsize(out)} bytes')


def predictor_inputs():
    gen = torch.Generator().manual_seed(7)
    N, D, S = 50, 32, 200
    h = (torch.rand(N, D, generator=gen) * 2 - 1).float()
    pairs = torch.randint(0, N, (2, S), generator=gen)
    pairs[0, :60] = 3                      # one node in many pairs
    pairs[1, 60:70] = pairs[0, 60:70]      # self pairs
    pairs[0, 70:75] = N - 1
    pairs[1, 75:80] = N - 1
    gout = (torch.rand(S, 1, generator=gen) * 2 - 1).double()
    return h, pairs, gout


def _run(module, h, pairs, gout, dtype):
    m = module.to(dtype)
    hh = h.detach().to(dtype).clone().requires_grad_(True)
    out = m(hh[pairs[0]], hh[pairs[1]])
    (out.reshape(gout.shape[0], -1) * gout.to(dtype)).sum().backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    return out.detach().clone(), hh.grad.clone(), grads


def record_predictors(layer_mod):
    h, pairs, gout = predictor_inputs()
    rec = {'h': h, 'pairs': pairs, 'gout': gout, 'mlp': {}}
    for L in (1, 2, 3):
        seed = 100 + L
        torch.manual_seed(seed)
        m_eval = layer_mod.MLPPredictor(32, 32, 1, L, 0.5).eval()
        torch.manual_seed(seed)
        m_p0 = layer_mod.MLPPredictor(32, 32, 1, L, 0.0).train()
        sd = {k: v.detach().clone() for k, v in m_eval.state_dict().items()}
        assert all(torch.equal(v, m_p0.state_dict()[k]) for k, v in sd.items())
        out32, dh32, g32 = _run(m_eval, h, pairs, gout, torch.float32)
        out32b, _, _ = _run(m_p0, h, pairs, gout, torch.float32)
        assert torch.equal(out32, out32b)
        torch.manual_seed(seed)
        m64 = layer_mod.MLPPredictor(32, 32, 1, L, 0.5).eval()
        out64, dh64, g64 = _run(m64, h, pairs, gout, torch.float64)
        assert torch.allclose(out64, lr.mlp_predictor64(sd, h[pairs[0]], h[pairs[1]]), rtol=1e-12, atol=1e-14)
        rec['mlp'][L] = {'seed': seed, 'state_dict': sd, 'out32': out32, 'dh32': dh32, 'grads32': g32, 'out64': out64, 'dh64': dh64, 'grads64': g64}
        print(f'MLPPredictor L {L}: fp32 distance to float64: out {float((out32.double() - out64).abs().max()):.3e}, dh {float((dh32.double() - dh64).abs().max()):.3e}')
    dot = layer_mod.DotPredictor()
    g1 = gout.reshape(-1)
    h32 = h.clone().requires_grad_(True)
    o32 = dot(h32[pairs[0]], h32[pairs[1]])
    (o32 * g1.float()).sum().backward()
    h64 = h.double().requires_grad_(True)
    o64 = dot(h64[pairs[0]], h64[pairs[1]])
    (o64 * g1).sum().backward()
    assert torch.allclose(o64.detach(), lr.pair_dot64(h, pairs), rtol=1e-12, atol=1e-14)
    assert torch.allclose(h64.grad, lr.pair_scatter64(h, pairs, g1)[0], rtol=1e-12, atol=1e-14)
    rec['dot'] = {'out32': o32.detach().clone(), 'dh32': h32.grad.clone(), 'out64': o64.detach().clone(), 'dh64': h64.grad.clone()}
    out = os.path.join(ROOT, 'tests', 'golden', 'linkpred_predictors.pt')
    torch.save(rec, out)
    print(f'linkpred_predictors: {os.path.getsize(out)} bytes')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('COLDBREW_REFERENCE_ROOT', ''))
    a = ap.parse_args()
    if not a.reference:
        raise SystemExit('name the reference tree: --reference PATH or COLDBREW_REFERENCE_ROOT')
    loss_mod, layer_mod = load_reference(a.reference)
    record_losses(loss_mod)
    record_predictors(layer_mod)


if __name__ == '__main__':
    main()
