"""GPU: the complete node-sharded HIP path (per-rank ingest of the row blocks on the device, halo plans, interior / halo
two-pass aggregation incl. the fused trunk store on top of the interior sums, global dropout indices, sharded structural
embeddings, gradient / regulariser all-reduces, cross-rank BatchNorm statistics) run by TWO processes that share the single
GPU of the test box, against the single-process trainer.  Collectives go through gloo with host staging (dist._staged)
because RCCL refuses two ranks on one device; everything else is the production code."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = ['--dataset=S-pubmed', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=111', '--se_reg=0.5',
        '--num_layers=2', '--manual_assign_GPU=0', '--do_deg_analyze=0']
ARGV_BN = ['--dataset=S-pubmed', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=000', '--num_layers=2',
           '--manual_assign_GPU=0', '--do_deg_analyze=0', '--force_set_to_best_config=0', '--type_trick=BatchNorm']   # norm runs (bare name)
ARGV_RES = ['--dataset=S-pubmed', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=000', '--num_layers=3',
            '--manual_assign_GPU=0', '--do_deg_analyze=0', '--force_set_to_best_config=0', '--type_trick=Residual']   # 'Residual' trunk (round 5)
ARGV_NR = ['--dataset=S-pubmed', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=111', '--se_reg=0.5', '--num_layers=3',
           '--manual_assign_GPU=0', '--do_deg_analyze=0', '--force_set_to_best_config=0', '--type_trick=NoResNodeNorm']   # non-residual stack (round 5)
ARGV_I0 = ['--dataset=S-pubmed', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=000', '--num_layers=3',
           '--manual_assign_GPU=0', '--do_deg_analyze=0']      # 'Initial' without tables: the rows-only forward on shards (round 5)
ARGV_ARX = ['--dataset=S-arxiv', '--use_special_split=0', '--want_headtail=0', '--whetherHasSE=000', '--num_layers=3',
            '--manual_assign_GPU=0', '--do_deg_analyze=0']     # 128 input features, ~85 k rows per rank: the input stage folded into the weight gradient (round 6)
SEEDS = list(range(7000, 7040))
STEPS = 3


def _full_state(argv):
    import contextlib
    import io
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.GNN_model import TeacherGNN
    from gnn_tail_generalization_amd.utils import set_arch_configs
    with contextlib.redirect_stdout(io.StringIO()):
        a = BaseOptions().get_arguments(argv)
    set_arch_configs(a)
    torch.manual_seed(0)
    return {k: v.detach().clone() for k, v in TeacherGNN(a).state_dict().items()}


def _worker(rank, world, port, exchange, overlap, partition, argv, q, wire='f32', slices='', cover='1', backend='gloo'):
    sys.path.insert(0, ROOT)
    import contextlib
    import io
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), COLDBREW_EXCHANGE=exchange, COLDBREW_OVERLAP=overlap,
                      COLDBREW_PARTITION=partition, COLDBREW_HALO_WIRE=wire,
                      COLDBREW_HALO_COVER='force' if cover == '1' else cover)      # force: the cover plan whatever it saves on this small graph
    if slices:
        os.environ['COLDBREW_HALO_SLICES'] = slices
    dev_id = rank if backend == 'nccl' else 0          # nccl (= RCCL): one GPU per rank; gloo: the ranks share the test box's single GPU
    if backend == 'nccl':
        argv = [a_ for a_ in argv if not a_.startswith('--manual_assign_GPU')] + [f'--manual_assign_GPU={dev_id}']
        torch.cuda.set_device(dev_id)
        from gnn_tail_generalization_amd.dist import init_rccl
        init_rccl(rank, world, f'cuda:{dev_id}')
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from gnn_tail_generalization_amd import ops
        from gnn_tail_generalization_amd.base_options import BaseOptions
        from gnn_tail_generalization_amd.dist import ShardedTrainer
        torch.cuda.set_device(dev_id)
        with contextlib.redirect_stdout(io.StringIO()):
            args = BaseOptions().get_arguments(argv)
            t = ShardedTrainer(args, 0)
            t.setup_teacherGNN()
        t.load_full_state_dict({k: v.cuda() for k, v in _full_state(argv).items()})
        assert t.sgraph.cover == (cover == '1' and overlap == '1' and exchange == 'halo')
        assert t.sgraph.f.plan is None or bool(t.sgraph.f.plan.cover) == t.sgraph.cover
        assert t.sgraph.exchange_kind == exchange and t.sgraph.overlap == (overlap == '1') and t.part.kind == partition
        assert t.sgraph.wire == wire
        if slices:
            assert t.sgraph.f.plan.n_slices == int(slices) and len(t.sgraph.f.halo) == int(slices)
        conv0 = t.teacherGNN.model.model.layers_GCN[0]
        assert (not conv0.whetherHasSE) or conv0.le.shape[0] == t.part.n_local
        from gnn_tail_generalization_amd import stack
        stack_calls, real_apply = [], stack._StackFn.apply
        stack._StackFn.apply = staticmethod(lambda *a_, **k_: (stack_calls.append(1), real_apply(*a_, **k_))[1])
        ops._seed_override[:] = list(SEEDS)
        losses = [float(t.train_step()) for _ in range(STEPS)]
        nores = '--type_trick=NoResNodeNorm' in argv
        if nores:
            assert stack_calls, 'the non-residual stack did not run as its fused node on the shards'
        if '--dataset=S-arxiv' in argv:
            # round 6: layer 0's store backward folded the mix gradients on the rank's rows (cb_trunk_layer_bwd_fold_f32) and the input stage ran inside the
            # input Linear's weight gradient (cb_gemm_tn_instage_f32), whose slab sums are all-reduced like any other gradient
            assert getattr(t.sgraph, 'instage_folds', 0) == (STEPS if os.environ.get('CB_INSTAGE_FOLD', '1') != '0' else 0), getattr(t.sgraph, 'instage_folds', 0)
        if (argv is ARGV or argv is ARGV_I0 or '--whetherHasSE=111' in argv or '--type_trick=Residual' in argv) and not nores:
            # the fused trunk (S-pubmed: hidden 256, 'Initial'): its backward went through the level orientations of the row-sparse backward
            # (dist.ShardedGraph.support_orients: 10 % train rows -> level 0 keeps a tenth of the reverse edges)
            assert t.sgraph._support_cache is not None and len(t.sgraph._support_cache[2]) >= 1, 'row-sparse level orientations not used'
            # round 5: where the last halo pass can be the aggregation + GEMM kernel (fp32 wire, cover plan or one slice) the levels are also COMPACT
            # in the rank's rows: head, store backward, weight gradients and GEMM tails of those levels ran on the support's rows only
            from gnn_tail_generalization_amd import trunk
            lv0 = t.sgraph._support_cache[2][0]
            assert (lv0.src is not None) == bool(trunk.agg_gemm_eligible(t.sgraph, 256, False)), 'compact levels not used where the plan allows them'
            if lv0.src is not None:
                assert 0 < lv0.src.n < t.part.n_local
                # ... and the training forward evaluated its last layer on the rank's loss rows (rows-only forward: the last exchange ships only the
                # in-neighbours of those rows; a structural-embedding table on that layer travels the same way)
                assert t.sgraph.rows_only_forwards == STEPS, t.sgraph.rows_only_forwards
        if overlap == '1' and exchange == 'halo' and wire == 'f32' and (argv is ARGV or argv is ARGV_I0 or '--whetherHasSE=111' in argv or '--type_trick=Residual' in argv):
            # round 5: the trunk allocates the matrices it exchanges with room behind them (dist.alloc_exchanged), so the interior pass and the first
            # halo slice ran as ONE pass ([local | slice 0], dist._Orientation.first) wherever a producer of the trunk wrote the matrix
            assert t.sgraph.merged_passes > 0, (t.sgraph.merged_passes, t.sgraph.interior_passes)
        accs = t.run_testSet()
        w = t.teacherGNN.model.model.layers_GCN[1].weight.detach().cpu()
        le = conv0.le.detach().cpu() if conv0.whetherHasSE else torch.zeros(1)
        bn = t.teacherGNN.state_dict().get('model.model.layers_norm.0.running_var', torch.zeros(1)).cpu()
        q.put((rank, 'ok', losses, w.numpy(), le.numpy(), t.part.lo(), t.part.hi(), bn.numpy(), (accs[0], accs[2])))   # by value: the child may exit first
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, 'FAIL ' + traceback.format_exc()[-2500:], None, None, None, 0, 0, None, None))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('exchange,overlap,partition,argv,wire,world,slices,cover', [
    ('halo', '1', 'edges', ARGV, 'f32', 2, '', '1'), ('halo', '0', 'rows', ARGV, 'f32', 2, '', '1'), ('allgather', '0', 'rows', ARGV, 'f32', 2, '', '1'),
    ('halo', '1', 'edges', ARGV_BN, 'f32', 2, '', '1'), ('halo', '1', 'edges', ARGV, 'bf16', 2, '', '1'), ('halo', '1', 'edges', ARGV, 'f32', 3, '', '1'),
    ('halo', '1', 'edges', ARGV, 'f32', 2, '3', '1'), ('halo', '1', 'edges', ARGV, 'f32', 3, '4', '1'), ('halo', '1', 'edges', ARGV, 'bf16', 2, '2', '1'),
    ('halo', '1', 'edges', ARGV_BN, 'f32', 2, '2', '1'),
    # the pull-only plan (COLDBREW_HALO_COVER=0): sliced by owner row chunk with row-chunked producers; unsliced with the aggregation + GEMM
    # kernel as its last halo pass
    ('halo', '1', 'edges', ARGV, 'f32', 2, '3', '0'), ('halo', '1', 'edges', ARGV, 'f32', 3, '', '0'), ('halo', '1', 'edges', ARGV, 'bf16', 2, '2', '0'),
    # the 'Residual' trunk on shards: cumulative supports, the second gradient of a store backward compact (cover) / row-chunked (pull, sliced)
    ('halo', '1', 'edges', ARGV_RES, 'f32', 2, '', '1'), ('halo', '1', 'edges', ARGV_RES, 'f32', 3, '2', '0'),
    # 'Initial' without tables: the rows-only forward on shards (last layer on the rank's loss rows through loss_rows_forward), cover / three ranks sliced / pull unsliced
    ('halo', '1', 'edges', ARGV_I0, 'f32', 2, '', '1'), ('halo', '1', 'edges', ARGV_I0, 'f32', 3, '3', '1'), ('halo', '1', 'edges', ARGV_I0, 'f32', 2, '', '0'),
    # the non-residual stack (stack.py) on shards: widths F -> H -> H -> C, SE tables on every layer, dropout on the logits
    ('halo', '1', 'edges', ARGV_NR, 'f32', 2, '', '1'), ('halo', '1', 'edges', ARGV_NR, 'f32', 3, '2', '0'), ('halo', '0', 'rows', ARGV_NR, 'f32', 2, '', '1'),
    # the ogbn-arxiv shape (BASELINE config 3) on two ranks: the round-6 input stage (fold pass + weight gradient with the stage inside) on row shards
    ('halo', '1', 'edges', ARGV_ARX, 'f32', 2, '', '1')],
    ids=['cover-overlap-edges', 'halo-singlepass-rows', 'allgather', 'batchnorm-cover-overlap', 'cover-bf16-wire', 'three-ranks-cover',
         'cover-sliced3', 'three-ranks-cover-sliced4', 'cover-sliced2-bf16-wire', 'batchnorm-cover-sliced2',
         'pull-sliced3', 'pull-three-ranks', 'pull-sliced2-bf16-wire-chunked-producers', 'residual-cover', 'residual-three-ranks-pull-sliced2',
         'rows-only-cover', 'rows-only-three-ranks-cover-sliced3', 'rows-only-pull',
         'nores-cover', 'nores-three-ranks-pull-sliced2', 'nores-singlepass-rows', 'arxiv-instage-fold-cover'])
def test_two_ranks_on_one_gpu_match_single_process(exchange, overlap, partition, argv, wire, world, slices, cover):
    _ranks_match_single_process(exchange, overlap, partition, argv, wire, world, slices, cover, 'gloo')


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs: RCCL refuses two ranks on one device')
@pytest.mark.parametrize('slices,cover', [('', '1'), ('3', '1'), ('3', '0')], ids=['cover', 'cover-sliced3', 'pull-sliced3'])
def test_two_gpus_rccl_halo_exchange(slices, cover):
    """the first box with two GPUs runs the halo exchange on RCCL itself — torch.distributed `nccl` with
    all_to_all_single on uneven splits, asynchronous work handles and device_id= initialisation, one rank per GPU — and must reproduce the
    single-GPU trainer exactly as the gloo-staged ranks on one GPU do.  Skipped on the one-GPU test boxes (the driver's 8-GPU node runs it)."""
    _ranks_match_single_process('halo', '1', 'edges', ARGV, 'f32', 2, slices, cover, 'nccl')


def _ranks_match_single_process(exchange, overlap, partition, argv, wire, world, slices, cover, backend):
    import contextlib
    import io
    sys.path.insert(0, ROOT)
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    # single-process reference on the same data, parameters and dropout seeds
    ops.set_graph_seed(None)       # (a --hip_graph test that ran earlier in this process leaves its device seed word installed: the eager reference must not add it)
    with contextlib.redirect_stdout(io.StringIO()):
        args = BaseOptions().get_arguments(argv)
        ref = trainer(args, 0)
        ref.setup_teacherGNN()
    ref.teacherGNN.load_state_dict({k: v.cuda() for k, v in _full_state(argv).items()})
    ops._seed_override[:] = list(SEEDS)
    want = [float(ref.train_step()) for _ in range(STEPS)]
    ops._seed_override[:] = []
    acc_ref = ref.run_testSet()
    n_nodes = ref.data.x.shape[0]
    conv0 = ref.teacherGNN.model.model.layers_GCN[0]
    w_ref = ref.teacherGNN.model.model.layers_GCN[1].weight.detach().cpu()
    le_ref = conv0.le.detach().cpu() if conv0.whetherHasSE else None
    bn_ref = ref.teacherGNN.state_dict().get('model.model.layers_norm.0.running_var')
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, exchange, overlap, partition, argv, q, wire, slices, cover, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=120)
    for rank, msg, losses, w, le, lo, hi, bn, accs in res:
        assert msg == 'ok', f'rank {rank}: {msg}'
        # accuracy = all-reduced hit counts / global mask sizes (eval forward on the shards); an argmax tie may flip a node or two
        assert abs(accs[0] - acc_ref[0]) <= 3.0 / n_nodes * 10 and abs(accs[1] - acc_ref[2]) <= 3.0 / n_nodes * 10, (accs, acc_ref)
        if wire == 'bf16':       # opt-in bfloat16 halo wire: every remote neighbour row rounded to 8 significand bits — its own, looser bound
            np.testing.assert_allclose(losses, want, rtol=5e-3)
            assert 0 < float((torch.from_numpy(w) - w_ref).abs().max()) <= 2e-2      # Adam steps of size lr: tiny gradient differences move a weight by up to lr per step
            continue
        np.testing.assert_allclose(losses, want, rtol=2e-5)
        if '--dataset=S-arxiv' in argv:
            # 1.7 * 10^5 rows: the two runs associate their sums differently (per-rank slabs, halo passes), and where a weight's gradient is zero to rounding
            # Adam's first steps move it by up to lr either way — a handful of elements; everything else agrees as on the small graphs
            dw = (torch.from_numpy(w) - w_ref).abs()
            assert float(dw.max()) <= 3e-3 and float((dw > 1e-5 + 1e-4 * w_ref.abs()).float().mean()) <= 0.01, (float(dw.max()), float((dw > 1e-5).float().mean()))
            assert float(dw.norm()) <= 2e-3 * float(w_ref.norm())
            continue
        torch.testing.assert_close(torch.from_numpy(w), w_ref, atol=1e-5, rtol=1e-4)
        if le_ref is not None:
            torch.testing.assert_close(torch.from_numpy(le), le_ref[lo:hi], atol=1e-5, rtol=1e-4)
        if bn_ref is not None:
            torch.testing.assert_close(torch.from_numpy(bn), bn_ref.cpu(), atol=1e-6, rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference epoch on row shards: head/tail metrics forward, records, sharded checkpoint / resume, single-file artifact
# ---------------------------------------------------------------------------------------------------------------------------
def _spawn(target, world, *args):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert r[1] == 'ok', f'rank {r[0]}: {r[1]}'
    return sorted(res, key=lambda r: r[0])


def _golden_epoch_worker(rank, world, port, q, name, slices):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import contextlib
    import io
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), COLDBREW_HALO_SLICES=slices)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from conftest import load_golden
        from helpers import product_args
        from gnn_tail_generalization_amd import norms_hip
        from gnn_tail_generalization_amd.data import Data
        from gnn_tail_generalization_amd.dist import ShardedTrainer
        torch.cuda.set_device(0)
        g = load_golden(name)
        args = product_args(g['cfg'], extra=[f'--want_headtail={g["want_headtail"]}', f'--use_special_split={g["use_special_split"]}'])
        args.lr, args.weight_decay, args.cuda_num = 0.01, 5e-4, 0
        args.has_loss_component_nodewise, args.has_loss_component_edgewise = True, False
        data = None
        if rank == 0:        # only the loading rank ever sees the whole graph
            data = Data(x=g['x'], y=g['y'], edge_index=g['edge_index'], train_mask=g['train_mask'], test_mask=~g['train_mask']).to('cuda:0')
            data.zero_deg_idx, data.small_deg_idx, data.large_deg_idx = (g[k].numpy() for k in ['zero_deg_idx', 'small_deg_idx', 'large_deg_idx'])
        with contextlib.redirect_stdout(io.StringIO()):
            t = ShardedTrainer(args, 0, data=data)
            t.setup_teacherGNN()
        assert t.x.shape[0] == t.part.n_local < g['x'].shape[0]
        t.load_full_state_dict({k: v.cuda() for k, v in g['sd'].items()})
        rec, bags = [], []
        for ep in range(g['steps']):
            with norms_hip.row_sharding(None, t.global_nodes()):
                loss, _, _ = t.run_trainSet()
            acc_train, _, acc_test, _ = t.run_testSet()
            rec.append([loss, acc_train, acc_test])
            bags.append([float(v) for v in t.bag['head_tail_iso']])
        sd = t.full_state_dict()
        q.put((rank, 'ok', np.array(rec), np.array(bags), {k: v.numpy() for k, v in sd.items()} if rank == 0 else None))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, 'FAIL ' + traceback.format_exc()[-2500:], None, None, None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('name,world,slices', [('trainer_headtail1_se100_cora', 2, '1'), ('trainer_headtail1_se100_cora', 3, '2'),
                                               ('trainer_headtail0_se111_pubmed', 2, '2')])
def test_sharded_epoch_reproduces_reference_trajectory(name, world, slices):
    """the node-sharded trainer runs the reference's epoch (run_trainSet incl. the head/tail metrics forward,
    run_testSet) and reproduces the trajectory the UNMODIFIED reference trainer produced on the same inputs — losses 1e-5 rel,
    accuracies and head/tail/isolation rows exactly, final weights (gathered from the shards) to the single-GPU tolerance."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from conftest import load_golden
    g = load_golden(name)
    res = _spawn(_golden_epoch_worker, world, name, slices)
    want = g['trajectory'].numpy()
    for rank, _, rec, bags, sd in res:
        np.testing.assert_allclose(rec[:, 0], want[:, 0], rtol=1e-5)
        np.testing.assert_array_equal(rec[:, 1:], want[:, 1:])
        np.testing.assert_allclose(bags.reshape(want.shape[0], -1), g['head_tail_iso'].numpy().reshape(want.shape[0], -1), atol=1e-3)
    sd = res[0][4]
    for k, v in g['sd_final'].items():
        if v.dtype.is_floating_point:
            torch.testing.assert_close(torch.from_numpy(sd[k]), v, atol=2e-5, rtol=2e-4, msg=lambda m, k=k: f'{k}: {m}')


CKPT_ARGV = ['--dataset=S-tiny', '--use_special_split=1', '--want_headtail=1', '--whetherHasSE=111', '--se_reg=0.5', '--num_layers=2',
             '--manual_assign_GPU=0']


def _ckpt_worker(rank, world, port, q, workdir, phases):
    sys.path.insert(0, ROOT)
    import contextlib
    import io
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from gnn_tail_generalization_amd.base_options import BaseOptions
        from gnn_tail_generalization_amd.dist import ShardedTrainer
        torch.cuda.set_device(0)
        os.chdir(workdir)
        out = None
        for epochs, resume in phases:
            with contextlib.redirect_stdout(io.StringIO()):
                args = BaseOptions().get_arguments(CKPT_ARGV + [f'--epochs={epochs}'] + (['--resume'] if resume else []))
                args.cuda_num, args.random_seed = 0, 0
                torch.manual_seed(0)
                np.random.seed(0)
                t = ShardedTrainer(args, 0)
                out = t.train_teacherGNN()
        le = t.teacherGNN.model.model.layers_GCN[0].le.detach().cpu().numpy()
        w = t.teacherGNN.model.model.layers_GCN[1].weight.detach().cpu().numpy()
        q.put((rank, 'ok', np.asarray(out), le, w, (t.part.lo(), t.part.hi())))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, 'FAIL ' + traceback.format_exc()[-2500:], None, None, None, None))
    finally:
        dist.destroy_process_group()


def test_sharded_checkpoint_resume_and_model_artifact(tmp_path):
    """ADVICE r02 (medium) / VERDICT item 4: `torchrun main.py --resume` on the node-sharded trainer continues from per-rank shard
    files bit for bit (records, structural-embedding rows, replicated weights, dropout seeds drawn from the restored RNG), and
    the final model is written as the reference's single-file artifact that the single-GPU trainer loads."""
    import contextlib
    import io
    a, b = tmp_path / 'straight', tmp_path / 'resumed'
    a.mkdir()
    b.mkdir()
    straight = _spawn(_ckpt_worker, 2, str(a), [(6, False)])
    resumed = _spawn(_ckpt_worker, 2, str(b), [(3, False), (6, True)])
    for s_, r_ in zip(straight, resumed):
        assert s_[2].shape == (4, 6) and np.isfinite(s_[2][0]).all()
        np.testing.assert_array_equal(s_[2], r_[2])          # records incl. the epochs before the restart
        np.testing.assert_array_equal(s_[3], r_[3])          # this rank's rows of the structural-embedding table
        np.testing.assert_array_equal(s_[4], r_[4])          # a replicated weight
    files = sorted(os.listdir(b / 'saved_models' / 'nodeC' / 'S-tiny'))
    assert files == ['teacherGNN', 'teacherGNN-ckpt.shard0of2', 'teacherGNN-ckpt.shard1of2'], files
    # the artifact = the shards re-assembled, loadable by the single-GPU trainer (utils.load_model, as the student stage does)
    sys.path.insert(0, ROOT)
    from gnn_tail_generalization_amd.base_options import BaseOptions
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    cwd = os.getcwd()
    os.chdir(a)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            args = BaseOptions().get_arguments(CKPT_ARGV + ['--epochs=1'])
            ref = trainer(args, 0)
            ref.load_teacherGNN()
    finally:
        os.chdir(cwd)
    le_full = ref.teacherGNN.model.model.layers_GCN[0].le.detach().cpu().numpy()
    for _, _, _, le, w, (lo, hi) in straight:
        np.testing.assert_array_equal(le_full[lo:hi], le)
        np.testing.assert_array_equal(ref.teacherGNN.model.model.layers_GCN[1].weight.detach().cpu().numpy(), w)


def test_bench_gpus_n_without_a_launcher_runs_n_ranks():
    """`python bench.py --gpus 2` started WITHOUT torch.distributed.run (no WORLD_SIZE) re-executes itself as two ranks (here: gloo
    dry run, both on the box's single GPU) and prints ONE JSON line that says n_gpus = 2, with the sharding self-diagnosis: both ranks seen, the
    sharded loss equal to the single-GPU loss of the same weights and seeds, row-sparse levels and the merged first pass in use."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env['COLDBREW_DIST_BACKEND'] = 'gloo'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dataset', 'S-arxiv', '--steps', '3', '--warmup', '1', '--full',
                        '--cpu-baseline', '0', '--pmc-traffic', '0', '--ref-epochs', '0'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 3 and d['value'] > 0
    sh = d['sharding']
    assert sh['ranks_seen'] == [0, 1] and sh['backend'] == 'gloo' and sh['loss_matches_n1'] is True, sh
    assert sum(sh['rows_per_rank']) == 169343
    ro = sh['rows_only_forward_rank0']      # where the plan allows compact levels the training forward ran its last layer on the rank's loss rows: a fraction of the forward halo
    compact = any(lv['rows_read'] is not None for lv in sh['row_sparse_levels_rank0'])
    assert (ro['forwards'] >= 3 and 0 < ro['halo_rows'] < ro['halo_rows_full_forward']) if compact else ro['forwards'] == 0, (ro, sh['row_sparse_levels_rank0'])



@pytest.mark.gpu
@pytest.mark.parametrize('extra', ['', '--force_set_to_best_config=0 --type_trick=Residual', '--force_set_to_best_config=0 --type_trick=NoResNodeNorm'])
def test_bench_sharded_path_on_rccl_with_one_rank(extra):
    """The N > 1 leg of bench.py (ShardedTrainer, the sharding report, the edge all-reduce, barrier-bracketed timing) on the backend the driver's SCALE runs
    use — torch.distributed `nccl` = RCCL —, as far as one GPU allows: world size 1 (`COLDBREW_FORCE_SHARDED=1`), for the three default trunk shapes."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'COLDBREW_DIST_BACKEND')}
    env['COLDBREW_FORCE_SHARDED'] = '1'
    env['MASTER_PORT'] = '29547'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--dataset', 'S-arxiv', '--steps', '3', '--warmup', '1', '--cpu-baseline', '0',
           '--pmc-traffic', '0', '--ref-epochs', '0']
    if extra:
        cmd.append('--extra=' + extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and d['value'] > 0 and d['sharding']['backend'] == 'nccl', d.get('sharding')
    assert d['roofline']['frac'] > 0 and d['final_loss'] == d['final_loss']
