"""GraphMLP on the HIP path against the unmodified reference's fixtures (tests/golden/graphmlp_*.pt, written by
tests/golden/make_graphmlp_golden.py with nn.Dropout.forward as the identity): same-seed construction bit for bit, the first training step
(loss_NContrastive, logits and all gradients: atol 1e-5, rtol 1e-4), the 5-epoch trajectory at the project's trajectory tolerances
(tests/test_gpu_student.py:4-5: losses rtol 1e-5, accuracies atol 1e-3, final weights atol 2e-5 / rtol 2e-4), the checkpoint's keys, the
eval forward, and tools/train_graphmlp.py end to end."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import student_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = ['graphmlp_powerlaw_tau2_r3_reg10', 'graphmlp_asym_multi_tau05_r2_reg1']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def eager_seeds():
    from gnn_tail_generalization_amd import ops
    ops.set_graph_seed(None)


def _no_dropout(module):
    for m in module.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0


def _trainer(g, tmp_path):
    t = sr.student_trainer(g, DEV, str(tmp_path))
    assert t.args.graphMLP_tau == g['args_after']['graphMLP_tau'] and t.args.graphMLP_r == g['args_after']['graphMLP_r']
    assert t.args.graphMLP_reg == g['args_after']['graphMLP_reg'] and t.args.lr == g['args_after']['lr']
    return t


@pytest.mark.parametrize('name', CASES)
def test_first_step_matches_the_reference(name, tmp_path):
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.MLP_model import GraphMLPStudent
    g = sr.load_case(name)
    t = _trainer(g, tmp_path)
    torch.manual_seed(g['seed'])
    m = GraphMLPStudent(t.args, t.data).to(DEV)
    m.train()
    batch = g['batches'][0].numpy()
    built = []
    m.on_build = lambda name_, mod: (built.append({k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}), _no_dropout(mod))
    emb = m.forward_part2(t.data.x, batch_idx=batch, edge_index=t.data.edge_index)
    # same seed, same order of construction: the reference's initial tensors bit for bit, under the reference's keys
    assert list(built[0]) == list(g['sd_init'])
    for k, v in g['sd_init'].items():
        assert torch.equal(built[0][k], v), k
    assert list(m.state_dict()) == list(g['sd_final'])
    nc = m.loss_NContrastive
    print(name, 'first step loss_NContrastive', float(nc), 'reference', float(g['loss_nc'][0]))
    torch.testing.assert_close(nc.detach().cpu().double(), g['loss_nc'][0], atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(emb.detach().cpu(), g['emb0'], atol=1e-5, rtol=1e-4)
    idx = m.index_on_device(batch, emb.device)
    loss = ops.nll_logsoftmax(emb, t.data.y[idx].contiguous(), None, len(batch)) + nc * t.args.graphMLP_reg
    torch.testing.assert_close(loss.detach().cpu().double(), g['loss_train'][0], atol=0, rtol=1e-5)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(g['grads0']) == {k for k, p in named.items() if p.grad is not None} and 'alphas' not in g['grads0']
    for k, r in g['grads0'].items():
        worst = float(((named[k].grad.cpu() - r).abs() / (1e-5 + 1e-4 * r.abs())).max())
        print(name, k, 'grad: worst |diff| / (atol + rtol |ref|) =', worst)
        torch.testing.assert_close(named[k].grad.cpu(), r, atol=1e-5, rtol=1e-4, msg=lambda s, k=k: f'{k}: {s}')
    # an eval forward does not evaluate the loss
    m.eval()
    with torch.no_grad():
        m.forward_part2(t.data.x, batch_idx=batch, edge_index=t.data.edge_index)
    assert m.loss_NContrastive is None


@pytest.mark.parametrize('name', CASES)
def test_trajectory_matches_the_reference(name, tmp_path):
    from gnn_tail_generalization_amd import MLP_model
    from gnn_tail_generalization_amd import trainer_node_classification as tn
    g = sr.load_case(name)
    t = _trainer(g, tmp_path)
    real = MLP_model.GraphMLPStudent
    seen = []

    class Hooked(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.on_build = lambda name_, mod: (seen.append(all(torch.equal(v.cpu(), g['sd_init'][k]) for k, v in mod.state_dict().items())),
                                                _no_dropout(mod))

    cwd = os.getcwd()
    os.chdir(tmp_path)
    tn.GraphMLPStudent = Hooked
    try:
        torch.manual_seed(g['seed'])
        np.random.seed(g['seed'])
        with contextlib.redirect_stdout(io.StringIO()):
            rows = t.train_graphMLP()
    finally:
        tn.GraphMLPStudent = real
        os.chdir(cwd)
    assert seen == [True]
    want = g['rows_part2'].numpy()
    print(name, 'rows', np.asarray(rows).tolist(), 'reference', want.tolist())
    assert np.asarray(rows).shape == want.shape == ((4, g['epochs']) if t.args.want_headtail else (1, g['epochs']))
    np.testing.assert_allclose(np.asarray(rows, dtype=np.float64), want, atol=1e-3, rtol=0)
    losses = np.asarray(t.bag['graphMLP_loss_train'], dtype=np.float64)
    print(name, 'training losses', losses.tolist(), 'reference', g['loss_train'].tolist())
    np.testing.assert_allclose(losses, g['loss_train'].numpy(), rtol=1e-5, atol=0)
    sd = {k: v.cpu() for k, v in t.seMLP.state_dict().items()}
    assert set(sd) == set(g['sd_final'])
    worst = max(float(((sd[k] - v).abs() / (2e-5 + 2e-4 * v.abs())).max()) for k, v in g['sd_final'].items())
    print(name, 'final weights: worst |diff| / (atol + rtol |ref|) =', worst)
    for k, v in g['sd_final'].items():
        torch.testing.assert_close(sd[k], v, atol=2e-5, rtol=2e-4, msg=lambda s, k=k: f'{k}: {s}')
    # the saved checkpoint has the reference's keys, and the reference's state_dict loads strict=True
    saved = torch.load(os.path.join(t.modeldir, 'seMLP'), map_location='cpu')
    assert list(saved) == list(g['sd_final']) and {'alphas', 'part2.model.0.weight', 'part2.model.1.bias', 'part2.model.4.weight', 'part2.out_proj.bias'} <= set(saved)
    t.seMLP.load_state_dict({k: v.to(DEV) for k, v in g['sd_final'].items()}, strict=True)
    assert torch.equal(t.seMLP.alphas.detach().cpu(), torch.tensor([0.0001, 0.0001]))      # never given a gradient


def test_tool_runs_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train_graphmlp
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with contextlib.redirect_stdout(io.StringIO()) as out:
            recs = train_graphmlp.main(['--dataset=S-tiny', '--epochs=3', '--batch_size=64', '--graphMLP_reg=1', '--graphMLP_tau=0.5', '--graphMLP_r=2',
                                        '--want_headtail=1', '--use_special_split=1', '--manual_assign_GPU=0'])
    finally:
        os.chdir(cwd)
    rows = np.asarray(recs)
    assert rows.shape == (1, 4, 3) and np.isfinite(rows[0, 0]).all()
    saved = torch.load(tmp_path / 'saved_models' / 'nodeC' / 'S-tiny' / 'seMLP', map_location='cpu')
    assert 'part2.out_proj.weight' in saved and 'alphas' in saved
    assert 'GraphMLP (reg' in out.getvalue()
