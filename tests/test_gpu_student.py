"""The student MLP trainers on the HIP path: trajectories against the unmodified reference's fixtures (tests/golden/student_*.pt),
one dropout-active step of each part against the float64 restatement with the product's masks injected, and main.py end to end.

Tolerances are the project's own for teacher trajectories (tests/test_gpu_trainer.py:27-32): losses rtol 1e-5, final weights
atol 2e-5 / rtol 2e-4, accuracies atol 1e-3 (the reference rounds them in float32).  No node may flip: the fixture generator
asserted that every argmax margin and top-K gap of the recorded forwards is >= 100 x the float32 bound of its dot product."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import student_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def eager_seeds():
    """A --hip_graph test that ran earlier in this process leaves its device seed word (and its running site number) installed; these
    tests run eagerly, with seeds drawn from torch's generator."""
    from gnn_tail_generalization_amd import ops
    ops.set_graph_seed(None)


@pytest.mark.parametrize('name', sr.STUDENT_CASES)
def test_trajectory_matches_the_reference(name, tmp_path):
    g = sr.load_case(name)
    t, rows1, rows2, built = sr.run_case(g, DEV, str(tmp_path))
    # the lazily built modules were the reference's, bit for bit, before the fixture's tensors were (re)loaded into them
    assert built and all(built.values()), built
    assert set(built) == ({'part1', 'part2'} if g['rows_part1'] is not None else {'part2'})
    want2 = g['rows_part2'].numpy()
    print(name, 'rows', np.asarray(rows2).tolist(), 'reference', want2.tolist())
    assert np.asarray(rows2).shape == want2.shape
    np.testing.assert_allclose(np.asarray(rows2, dtype=np.float64), want2, atol=1e-3, rtol=0)
    if g['rows_part1'] is not None:
        rec_dir = os.path.join(str(tmp_path), 'wIns', 'Recs', 'student_case', 'seMLP')
        for key in ('loss_train', 'loss_test'):
            mine = np.load(os.path.join(rec_dir, f'{key}@student_case@seMLP.npy'))
            want = g[key].numpy()
            print(name, key, mine.tolist(), 'reference', want.tolist())
            np.testing.assert_allclose(np.exp(mine), np.exp(want), rtol=1e-5, atol=0)
        np.testing.assert_allclose(np.exp(np.asarray(rows1, dtype=np.float64)), np.exp(g['rows_part1'].numpy()), rtol=1e-5, atol=0)
        assert np.asarray(rows1).shape == (1, g['epochs'])
    sd = {k: v.cpu() for k, v in t.seMLP.state_dict().items()}
    assert set(sd) == set(g['sd_final'])
    worst = max(float(((sd[k] - v).abs() / (2e-5 + 2e-4 * v.abs())).max()) for k, v in g['sd_final'].items())
    print(name, 'final weights: worst |diff| / (atol + rtol |ref|) =', worst)
    for k, v in g['sd_final'].items():
        torch.testing.assert_close(sd[k], v, atol=2e-5, rtol=2e-4, msg=lambda m, k=k: f'{k}: {m}')
    files = set(os.listdir(t.modeldir))
    assert 'seMLP' in files and (('seMLP-part-1' in files) == (g['rows_part1'] is not None))
    # a checkpoint written here loads strict=True where the reference's keys are expected
    saved = torch.load(os.path.join(t.modeldir, 'seMLP'), map_location='cpu')
    assert list(saved) == list(g['sd_final'])


def _grads_close(named, ref, tag):
    for k, r in ref.items():
        got = named[k].grad
        assert got is not None, (tag, k)
        torch.testing.assert_close(got.cpu().double(), r, atol=1e-5, rtol=1e-4, msg=lambda m, k=k: f'{tag} {k}: {m}')


@pytest.mark.parametrize('name', ['student_semlp_2layer_headtail_iso', 'student_semlp_residual'])
def test_dropout_active_steps_against_the_restatement(name, tmp_path):
    """One part-1 and one part-2 training step with --dropout_MLP=0.2 (BlockResMLP keeps its own p = 0.1): loss and every gradient against
    the float64 restatement that is handed the product's keep masks; part 2 moves part2 and the alphas only."""
    from gnn_tail_generalization_amd import MLP_model, ops
    g = sr.load_case(name)
    t = sr.student_trainer(g, DEV, str(tmp_path))
    t.args.dropout_MLP = 0.2
    t._new_student(t.teacherGNN)
    m = t.seMLP
    m.optfun = t.optfun
    se = g['teacherSE']
    m.teacherSE = se.to(DEV)
    x = t.data.x.requires_grad_(True)
    torch.manual_seed(11)
    batch = np.random.RandomState(5).choice(m.train_idx, 48)
    drawn, real = [], MLP_model.next_seed
    MLP_model.next_seed = lambda: drawn.append(real()) or drawn[-1]

    def masks_for(module_list, B):
        """Keep masks of the seeds drawn, in the order the modules consumed them: one per Dropout child with p > 0."""
        shapes = []
        for mod in module_list:
            for seq in ([mod] if isinstance(mod, torch.nn.Sequential) else (list(mod.blocks) if hasattr(mod, 'blocks') else [])):
                for i, ch in enumerate(seq):
                    if isinstance(ch, torch.nn.Dropout) and ch.p > 0:
                        width = seq[i - 3].out_features if isinstance(seq[i - 1], torch.nn.GELU) else seq[i - 1].out_features
                        shapes.append(((B, width), ch.p))
        assert len(shapes) == len(drawn), (shapes, len(drawn))
        return sr.Masks([ops.dropout_keep_mask(sh, p, s, DEV).cpu() for (sh, p), s in zip(shapes, drawn)])

    try:
        # ---- part 1 ---------------------------------------------------------------------------------------------------------------
        m.train()
        out = m.forward_part1(x, batch_idx=batch)
        loss = ops.mse_rows(out, m.teacherSE, m.index_on_device(batch, out.device))
        loss.backward()
        assert len(drawn) > 0
        sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
        ref_out = sr.module_forward(m.part1, sd64, 'part1.', g['x'].double()[batch], True, masks_for([m.part1], len(batch)))
        ref_loss = F.mse_loss(ref_out, se.double()[batch])
        ref_loss.backward()
        print(name, 'part-1 loss', float(loss.detach()), 'restatement', float(ref_loss.detach()))
        torch.testing.assert_close(loss.detach().cpu().double(), ref_loss.detach(), atol=1e-5, rtol=1e-4)
        _grads_close(dict(m.named_parameters()), {k: v.grad for k, v in sd64.items() if k.startswith('part1.')}, 'part 1')
        assert m.alphas.grad is None and x.grad is None
        # ---- part 2 ---------------------------------------------------------------------------------------------------------------
        m.zero_grad(set_to_none=True)
        with torch.no_grad():
            m.alphas.copy_(torch.tensor([0.8, 1.2]))
        del drawn[:]
        logits = m.forward_part2(x, batch_idx=batch, edge_index=t.data.edge_index)
        idx = m.index_on_device(batch, logits.device)
        loss = ops.nll_logsoftmax(logits, t.data.y[idx].contiguous(), None, len(batch))
        loss.backward()
        sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
        masks = masks_for([m.part1, m.part2], len(batch))
        xb = g['x'].double()[batch]
        guess = sr.module_forward(m.part1, sd64, 'part1.', xb, True, masks).detach() * sd64['alphas'][0]
        rep, _, val = sr.replacement(guess.detach(), se.double(), m.topK_2_replace)
        ref_logits = sr.module_forward(m.part2, sd64, 'part2.', torch.cat([xb, rep * sd64['alphas'][1], guess], -1), True, masks)
        ref_loss = F.cross_entropy(ref_logits, g['y'][batch])
        ref_loss.backward()
        print(name, 'part-2 loss', float(loss.detach()), 'restatement', float(ref_loss.detach()), 'alphas.grad', m.alphas.grad.tolist(), sd64['alphas'].grad.tolist())
        torch.testing.assert_close(loss.detach().cpu().double(), ref_loss.detach(), atol=1e-5, rtol=1e-4)
        named = dict(m.named_parameters())
        _grads_close(named, {k: v.grad for k, v in sd64.items() if k.startswith('part2.') or k == 'alphas'}, 'part 2')
        for k, p in named.items():
            if k.startswith('part1.'):
                assert p.grad is None, k
        assert x.grad is None
        assert all(v.grad is None for k, v in sd64.items() if k.startswith('part1.'))
    finally:
        MLP_model.next_seed = real


@pytest.mark.parametrize('which', ['SEMLP', 'StudentBaseMLP'])
def test_main_end_to_end(which, tmp_path):
    """main.py --dataset=S-tiny --train_which=<which>: checkpoints, record shapes, strict reload with bit-identical eval logits, and a
    second identically seeded run with bitwise-equal final weights."""
    import main as cli
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.MLP_model import SEMLP
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    argv = ['--dataset=S-tiny', f'--train_which={which}', '--epochs=4', '--whetherHasSE=111', '--se_reg=0.5', '--want_headtail=1',
            '--use_special_split=1', '--manual_assign_GPU=0']
    cwd = os.getcwd()
    finals = []
    try:
        for run in ('a', 'b'):
            d = tmp_path / run
            d.mkdir()
            os.chdir(d)
            with contextlib.redirect_stdout(io.StringIO()):
                if run == 'a':
                    args = BaseOptions().get_arguments(argv)
                    args.random_seed = 0
                    cli.set_seed(args)
                    t = trainer(args, 0)
                    rows = np.asarray(t.main())
                else:
                    rows_b = np.asarray(cli.main(argv))
            files = set(os.listdir(d / 'saved_models' / 'nodeC' / 'S-tiny'))
            assert 'seMLP' in files and (('seMLP-part-1' in files and 'teacherSE.pt' in files) == (which == 'SEMLP')), files
            finals.append(torch.load(d / 'saved_models' / 'nodeC' / 'S-tiny' / 'seMLP', map_location='cpu'))
        assert rows.shape == (4, 4) and rows_b.shape == (1, 4, 4) and np.array_equal(rows, rows_b[0], equal_nan=True)
        assert np.isfinite(rows[0]).all() and (rows[0] >= 0).all() and (rows[0] <= 100).all()
        rec = d / 'wIns' / 'Recs' / 'nodeC' / 'S-tiny' / 'seMLP'
        assert np.load(rec / 'acc_test@nodeC@S-tiny@seMLP.npy').shape == (4,)
        if which == 'SEMLP':
            assert np.load(rec / 'loss_train@nodeC@S-tiny@seMLP.npy').shape == (4,) and np.load(rec / 'loss_test@nodeC@S-tiny@seMLP.npy').shape == (4,)
        assert list(finals[0]) == list(finals[1])
        for k in finals[0]:
            assert torch.equal(finals[0][k], finals[1][k]), k
        # strict reload into a fresh module reproduces the eval-mode logits bit for bit
        m = t.seMLP.eval()
        idx = m.test_idx.numpy()
        with torch.no_grad():
            want = m.forward_part2(t.data.x, batch_idx=idx, edge_index=t.data.edge_index).clone()
        fresh = SEMLP(t.args, t.data, t.teacherGNN if which == 'SEMLP' else None).to(DEV)
        if which == 'SEMLP':
            fresh.teacherSE = m.teacherSE
            fresh.build_part1(m.teacherSE.shape[1])
        fresh.build_part2(t.args.num_feats + (2 * m.teacherSE.shape[1] if which == 'SEMLP' else 0))
        fresh.load_state_dict(finals[0], strict=True)
        fresh.eval()
        with torch.no_grad():
            got = fresh.forward_part2(t.data.x, batch_idx=idx, edge_index=t.data.edge_index)
        assert torch.equal(got, want)
        if which == 'SEMLP':
            assert float(m.alphas.detach().sub(1e-4).abs().max()) > 0        # part 2 moved the alphas
    finally:
        os.chdir(cwd)
