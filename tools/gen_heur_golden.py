"""Records tests/golden/heur_*.pt from the UNMODIFIED reference functions `CN` and `AA` (Link_prediction_baseline/heuristics.py:107-129).
Runs only where the reference tree exists (COLDBREW_REFERENCE_ROOT, or --reference PATH) and scipy + tqdm import; never
from a test.  The reference module imports torch_geometric and ogb at its top, which its `CN` / `AA` bodies do not use (they use scipy, numpy,
tqdm and a `DataLoader`): the file is loaded with stand-in modules for the absent imports, torch's own DataLoader in place of PyG's.  The pairs
are passed as numpy arrays because scipy >= 1.15 refuses torch tensors as indices.

Two graphs:
  heur_asym_multi   the asymmetric multigraph tests/golden/case_graph_asym_multi.pt (96 nodes, duplicates and self loops), 200 pairs, the first
                    ten of them self pairs
  heur_rows         tests/heur_ref.py heur_rows_graph(): out-rows of exactly 0, 1, 63, 64, 65, 130 and 200 entries, every combination of
                    them in both orders and with itself
Each file: edge_index, N, pairs, cn, aa.  Before writing, the recorded scores are compared with the dense restatement of tests/heur_ref.py
(CN exactly, AA within one fp32 rounding).
    usage: python tools/gen_heur_golden.py [--reference PATH]"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import heur_ref as hr  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute exists (the names the reference imports and its CN / AA never touch)."""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


def load_reference_heuristics(root):
    path = os.path.join(root, 'Link_prediction_baseline', 'heuristics.py')
    if not os.path.isfile(path):
        raise SystemExit(f'reference tree not found: {path}')
    import torch.utils.data
    data_mod = _Anything('torch_geometric.data')
    data_mod.DataLoader = torch.utils.data.DataLoader
    stand_ins = {'torch_geometric': _Anything('torch_geometric'), 'torch_geometric.utils': _Anything('torch_geometric.utils'),
                 'torch_geometric.data': data_mod, 'ogb': _Anything('ogb'), 'ogb.linkproppred': _Anything('ogb.linkproppred')}
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location('_reference_heuristics', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def record(ref, name, edge_index, n, pairs):
    import scipy.sparse as ssp
    ei = np.asarray(edge_index, dtype=np.int64)
    A = ssp.csr_matrix((np.ones(ei.shape[1], dtype=int), (ei[0], ei[1])), shape=(n, n))      # as eva_heuristics_v2_dec25 builds it (:19-24)
    pairs = np.asarray(pairs, dtype=np.int64)
    cn, _ = ref.CN(A, pairs)
    aa, _ = ref.AA(A, pairs)
    dense = hr.dense_adjacency(ei, n)
    assert np.array_equal(cn.numpy().astype(np.float64), hr.cn64(dense, pairs)), name
    assert hr.within_aa_bound(aa.numpy(), hr.aa64(dense, pairs)).all(), name
    out = os.path.join(ROOT, 'tests', 'golden', name + '.pt')
    torch.save({'edge_index': torch.from_numpy(ei), 'N': int(n), 'pairs': torch.from_numpy(pairs), 'cn': cn.clone(), 'aa': aa.clone()}, out)
    bits = int((aa.numpy() == hr.aa64(dense, pairs).astype(np.float32)).sum())
    print(f'{name}: N {n}, E {ei.shape[1]}, {pairs.shape[1]} pairs, CN max {int(cn.max())}, AA max {float(aa.max()):.4f}; '
          f'AA equals the rounded restatement bit for bit in {bits} of {pairs.shape[1]}; {os.path.getsize(out)} bytes')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('COLDBREW_REFERENCE_ROOT', ''))
    a = ap.parse_args()
    if not a.reference:
        raise SystemExit('name the reference tree: --reference PATH or COLDBREW_REFERENCE_ROOT')
    ref = load_reference_heuristics(a.reference)
    g = torch.load(os.path.join(ROOT, 'tests', 'golden', 'case_graph_asym_multi.pt'), weights_only=False)
    n = int(g['x'].shape[0])
    rng = np.random.default_rng(96)
    pairs = rng.integers(0, n, (2, 200))
    pairs[1, :10] = pairs[0, :10]
    record(ref, 'heur_asym_multi', g['edge_index'].numpy(), n, pairs)
    ei, n = hr.heur_rows_graph()
    record(ref, 'heur_rows', ei, n, hr.heur_rows_pairs())


if __name__ == '__main__':
    main()
