"""Records tests/golden/pairpred_predictors.pt from the UNMODIFIED reference: `BilinearPredictor`, `MLPDotPredictor`, `MLPBilPredictor` and
`MLPCatPredictor` of Link_prediction_model/layer.py.  Runs only where the reference tree exists (COLDBREW_REFERENCE_ROOT, or --reference PATH), on
the CPU; never from a test.  layer.py is loaded by path with stand-in modules for the imports the predictors do not use, exactly as
tools/gen_linkpred_golden.py does, and no bytecode is written.

  inputs   h [40, 16] uniform in [-1, 1]; 50 pairs: one node in 12 of them, 5 self pairs, node N - 1 on either side; gout [50, 1]
  modules  for L = 1, 2, 3: BilinearPredictor(16) (L does not enter: recorded once per L under its own seed), MLPDotPredictor(16, 16, L, 0.5),
           MLPBilPredictor(16, 16, L, 0.5), MLPCatPredictor(16, 16, 1, L, 0.5), each constructed under a recorded seed, in eval mode
  records  the seed, the state_dict, the fp32 CPU output, the float64 output and the float64 gradients of sum(out * gout) with respect to h and
           every parameter; and the factory's width-one MLPDOT / MLPBIL (create_predictor_layer's argument mapping: hidden_channels = 1) for L = 2
Before writing, every recording is compared with the restatement of tests/pairpred_ref.py.
    usage: python tools/gen_pairpred_golden.py [--reference PATH]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import pairpred_ref as pr  # noqa: E402
from gen_linkpred_golden import _run, load_reference  # noqa: E402

N, D, S = 40, 16, 50


def predictor_inputs():
    gen = torch.Generator().manual_seed(11)
    h = (torch.rand(N, D, generator=gen) * 2 - 1).float()
    pairs = torch.randint(0, N, (2, S), generator=gen)
    pairs[0, :12] = 3                      # one node in many pairs
    pairs[1, 12:17] = pairs[0, 12:17]      # self pairs
    pairs[0, 17:19] = N - 1
    pairs[1, 19:21] = N - 1
    gout = (torch.rand(S, 1, generator=gen) * 2 - 1).double()
    return h, pairs, gout


def makers(layer_mod, width):
    return {'bil': lambda L: layer_mod.BilinearPredictor(D), 'mlpdot': lambda L: layer_mod.MLPDotPredictor(D, width, L, 0.5),
            'mlpbil': lambda L: layer_mod.MLPBilPredictor(D, width, L, 0.5), 'mlpcat': lambda L: layer_mod.MLPCatPredictor(D, width, 1, L, 0.5)}


def _record(make, kind, L, seed, h, pairs, gout):
    torch.manual_seed(seed)
    m32 = make(L).eval()
    sd = {k: v.detach().clone() for k, v in m32.state_dict().items()}
    out32, _, _ = _run(m32, h, pairs, gout, torch.float32)
    torch.manual_seed(seed)
    out64, dh64, g64 = _run(make(L).eval(), h, pairs, gout, torch.float64)
    o, dh, g = pr.predictor_grads64(kind, sd, h, pairs, gout)
    assert torch.allclose(out64, o, rtol=1e-12, atol=1e-14) and torch.allclose(dh64, dh, rtol=1e-11, atol=1e-13), (kind, L)
    assert all(torch.allclose(g64[k], g[k], rtol=1e-11, atol=1e-13) for k in g64), (kind, L)
    print(f'{kind} L {L}: fp32 distance to float64: out {float((out32.double() - out64).abs().max()):.3e}')
    return {'seed': seed, 'state_dict': sd, 'out32': out32, 'out64': out64, 'dh64': dh64, 'grads64': g64}


def record_predictors(layer_mod):
    h, pairs, gout = predictor_inputs()
    rec = {'h': h, 'pairs': pairs, 'gout': gout, 'N': N, 'D': D, 'S': S}
    for i, kind in enumerate(pr.KINDS):
        rec[kind] = {L: _record(makers(layer_mod, D)[kind], kind, L, 200 + 10 * i + L, h, pairs, gout) for L in (1, 2, 3)}
    rec['width_one'] = {}
    for i, kind in enumerate(('mlpdot', 'mlpbil')):      # a width-one stack ends in one ReLU: the first seed under which it is not dead on every pair
        seed = 300 + 50 * i
        while True:
            r = _record(makers(layer_mod, 1)[kind], kind, 2, seed, h, pairs, gout)
            if int((r['out64'] != 0).sum()) >= S // 2:
                break
            seed += 1
        rec['width_one'][kind] = r
    out = os.path.join(ROOT, 'tests', 'golden', 'pairpred_predictors.pt')
    torch.save(rec, out)
    print(f'pairpred_predictors: {os.path.getsize(out)} bytes')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('COLDBREW_REFERENCE_ROOT', ''))
    a = ap.parse_args()
    if not a.reference:
        raise SystemExit('name the reference tree: --reference PATH or COLDBREW_REFERENCE_ROOT')
    _, layer_mod = load_reference(a.reference)
    record_predictors(layer_mod)


if __name__ == '__main__':
    main()
