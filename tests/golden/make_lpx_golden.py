"""Generates the fixtures of the link-prediction experiment's host pieces from the *unmodified* reference (build container only):

    python tests/golden/make_lpx_golden.py

  tests/golden/lpx_reference.pt   data only:
    recall     utils.cal_recall on integer / half-integer scores (positives in [-1, 2], negatives in [-1, 1.5]) at (P, Nn) = (1, 0), (3, 5), (8, 12),
               (40, 100) for topk in None, '0', '0.8', '1', '1.25', '7', '200', plus one case without a positive above 0: inputs, topk, the value as
               a Python float.  The maker asserts that at least one case has positives and negatives tied at its cut.
    edges      Link_prediction_model.utils.get_pos_neg_edges for 'valid' and 'test' in the 'edge' / 'edge_neg' form and in the 'source_node' /
               'target_node' / 'target_node_neg' form: the split and the two returned tensors.
    logger     Link_prediction_model.logger.Logger.print_statistics: the text for a 2-run, 3-evaluation record with a repeated maximum, per run and
               over all runs, for both values of last_best.
    shapes     local_neg_sample (shape, and [i, j, 0] == pos[i, 0]) and sample_perm_copy (every copy a permutation of copy 0) outputs.
`global_neg_sample` / `global_perm_neg_sample` cannot run here (PyG's negative_sampling is stubbed absent): the device samplers are tested against
tests/lpx_ref.py alone."""
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import lpx_ref as xr  # noqa: E402
import ref_import  # noqa: E402


def recall_cases(ns):
    rng = np.random.default_rng(4100)
    cases, tied_at_cut = [], 0
    sizes = list(xr.RECALL_SIZES) + [('nopos', 6, 9)]
    for size in sizes:
        if size[0] == 'nopos':
            P, Nn = size[1:]
            pos = -np.abs(xr.half_integer_scores(rng, P, -1, 1))      # nothing above 0 (zeros included)
        else:
            P, Nn = size
            pos = xr.half_integer_scores(rng, P, -1, 2)
            if Nn == 0:
                pos = np.clip(np.abs(pos), np.float32(0.5), np.float32(2))      # (1, 0): the reference indexes an empty array otherwise
        neg = xr.half_integer_scores(rng, Nn, -1, 1.5)
        for topk in xr.RECALL_TOPKS:
            val = ns.utils.cal_recall(torch.from_numpy(pos), torch.from_numpy(neg), topk=topk)
            num, P_ = xr.recall_parts(pos, neg, topk)
            assert float(val) == num / P_, (size, topk, float(val), num, P_)
            if topk is not None and float(topk) != 0:
                k = int(topk) if float(topk) > 5 else int(float(topk) * P)
                M = np.sort(np.concatenate([pos[pos > 0], neg]))[::-1]
                if 0 < k < len(M) and M[k - 1] == M[k] and (pos[pos > 0] == M[k]).any() and (neg == M[k]).any():
                    tied_at_cut += 1
            cases.append(dict(pos=torch.from_numpy(pos.copy()), neg=torch.from_numpy(neg.copy()), topk=topk, value=float(val)))
    assert tied_at_cut >= 3, tied_at_cut
    return cases


def edge_cases(lp_utils):
    g = torch.Generator().manual_seed(4200)
    out = {}
    edge_form = {s: {'edge': torch.randint(0, 30, (n, 2), generator=g), 'edge_neg': torch.randint(0, 30, (m, 2), generator=g)}
                 for s, n, m in (('train', 9, 9), ('valid', 5, 7), ('test', 6, 4))}
    src_form = {'train': {'source_node': torch.randint(0, 30, (8,), generator=g), 'target_node': torch.randint(0, 30, (8,), generator=g)}}
    for s, n, k in (('valid', 4, 3), ('test', 5, 2)):
        src_form[s] = {'source_node': torch.randint(0, 30, (n,), generator=g), 'target_node': torch.randint(0, 30, (n,), generator=g),
                       'target_node_neg': torch.randint(0, 30, (n, k), generator=g)}
    for name, split_edge in (('edge', edge_form), ('source_node', src_form)):
        res = {}
        for s in ('valid', 'test'):
            pos, neg = lp_utils.get_pos_neg_edges(s, split_edge)
            res[s] = (pos.clone(), neg.clone())
        out[name] = dict(split_edge=split_edge, result=res)
    return out


def logger_case(Logger):
    record = [[(0.50, 0.40), (0.70, 0.45), (0.70, 0.60)], [(0.30, 0.20), (0.30, 0.35), (0.10, 0.50)]]      # each run repeats its maximum
    lg = Logger(2)
    for run, rows in enumerate(record):
        for r in rows:
            lg.add_result(run, r)
    text = {}
    for last_best in (False, True):
        for run in (0, 1, None):
            f = io.StringIO()
            lg.print_statistics(run, f=f, last_best=last_best)
            text[(run, last_best)] = f.getvalue()
    assert text[(0, False)] != text[(0, True)]
    return dict(record=record, text=text)


def shape_cases(nsamp):
    g = torch.Generator().manual_seed(4300)
    pos = torch.randint(0, 50, (11, 2), generator=g)
    torch.manual_seed(4301)
    local = nsamp.local_neg_sample(pos, num_nodes=50, num_neg=3)
    assert tuple(local.shape) == (11, 3, 2) and bool((local[:, :, 0] == pos[:, :1]).all()) and int(local[:, :, 1].max()) < 50
    ei = torch.stack([torch.arange(13), torch.arange(13) + 100])
    torch.manual_seed(4302)
    copies = nsamp.sample_perm_copy(ei, 13, 4)
    return dict(local=dict(pos=pos, num_nodes=50, num_neg=3, out=local), perm_copy=dict(edge_index=ei, target_num_sample=13, num_perm_copy=4, out=copies))


def main():
    ns = ref_import.load_reference()
    torch.set_num_threads(1)
    import Link_prediction_model.logger as ref_logger
    import Link_prediction_model.negative_sample as ref_nsamp
    import Link_prediction_model.utils as ref_lp_utils
    out = dict(recall=recall_cases(ns), edges=edge_cases(ref_lp_utils), logger=logger_case(ref_logger.Logger), shapes=shape_cases(ref_nsamp))
    path = os.path.join(HERE, 'lpx_reference.pt')
    torch.save(out, path)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out['recall']), 'recall cases')


if __name__ == '__main__':
    main()
