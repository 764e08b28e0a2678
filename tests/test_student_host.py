"""Host-side checks of the student MLPs (no GPU): the package surface, construction that is bit-identical to the unmodified
reference's under the same seed (fixtures tests/golden/student_*.pt, written by tests/golden/make_student_golden.py), the C ABI
entries of csrc/cb_mlp.hip, and the refusals of what is not built."""
import ctypes
import os
import re

import pytest
import torch

import student_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_ln_gelu_drop_fwd_f32', 'cb_ln_gelu_drop_bwd_workspace_bytes', 'cb_ln_gelu_drop_bwd_f32', 'cb_mse_rows_f32',
               'cb_part2_assemble_f32', 'cb_part2_assemble_bwd_f32']


def test_package_exposes_the_student_models():
    from gnn_tail_generalization_amd import MLP_model
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    for name in ('SEMLP', 'BlockResMLP', 'StudentBaseMLP'):
        assert isinstance(getattr(MLP_model, name), type) and issubclass(getattr(MLP_model, name), torch.nn.Module)
    for name in ('train_seMLP_part1', 'train_seMLP_part2', 'eval_headtail__traintest_v2'):
        assert callable(getattr(trainer, name))


def _student(g):
    from gnn_tail_generalization_amd.MLP_model import SEMLP
    args = sr.student_args(g)
    args.device = torch.device('cpu')
    if g['train_which'] == 'StudentBaseMLP':
        args.SEMLP__downgrade_to_MLP = 1
    data = type('Data', (), {})()
    data.train_mask, data.test_mask = g['train_mask'], ~g['train_mask']
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    return args, SEMLP(args, data, None)


@pytest.mark.parametrize('name', sr.STUDENT_CASES)
def test_lazy_builds_match_the_reference_bit_for_bit(name):
    """Same seed, same order of construction on the CPU -> the reference's keys and initial tensors (no dropout draw lies between the
    two builds of a fixture run, so building part 2 right after part 1 sees the generator state the reference saw)."""
    g = sr.load_case(name)
    args, m = _student(g)
    for k, v in g['args_after'].items():
        assert getattr(args, k) == v, (k, getattr(args, k), v)       # the product's option pipeline arrives where the reference's did
    assert args.batch_size == g['args_after']['batch_size'] and args.StudentBaseMLP.num_blocks == g['student_cfg']['num_blocks']
    torch.manual_seed(g['seed'])
    part1_keys = set()
    if g.get('sd_after_part1'):
        m.build_part1(g['teacherSE'].shape[1])
        sd = m.state_dict()
        part1_keys = set(g['sd_after_part1'])
        assert {k for k in sd if k.startswith('part1.')} == part1_keys
        for k, v in g['sd_after_part1'].items():
            assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k
        dim_in = args.num_feats + 2 * g['teacherSE'].shape[1]
    else:
        dim_in = args.num_feats
    m.build_part2(dim_in)
    sd = m.state_dict()
    assert set(sd) == set(g['sd_final']) == part1_keys | set(g['sd_after_part2']) | {'alphas'}
    for k, v in g['sd_after_part2'].items():
        assert torch.equal(sd[k], v), k
    assert torch.equal(sd['alphas'], torch.tensor([0.0001, 0.0001]))
    m.load_state_dict(g['sd_final'], strict=True)                      # a reference checkpoint loads strict=True


def test_state_dict_keys_of_both_forms():
    g = sr.load_case('student_semlp_2layer_headtail_iso')
    assert {'alphas', 'part1.0.weight', 'part1.1.weight', 'part1.4.bias', 'part2.0.weight', 'part2.1.bias', 'part2.4.weight'} <= set(g['sd_final'])
    g = sr.load_case('student_semlp_residual')
    assert {'part1.in_proj.weight', 'part1.blocks.0.0.weight', 'part1.blocks.0.1.weight', 'part1.blocks.0.4.bias', 'part1.out_proj.bias'} <= set(g['sd_final'])
    _, m = _student(g)
    m.build_part1(g['teacherSE'].shape[1])
    assert len(m.part1.blocks[0]) == 6 and len(m.part1.blocks[-1]) == 5      # last_dropout on all blocks but the last (:38-39)


def test_c_abi_of_the_student_kernels():
    from gnn_tail_generalization_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'coldbrew_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(cb_[a-z0-9_]+)\s*\(', hdr))
    assert os.path.isfile(_lib.LIB_PATH), 'build the extension first: python __graft_entry__.py'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        n_args = len([a for a in re.search(name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1).split(',') if a.strip() and a.strip() != 'void'])
        assert n_args == len(_lib.SIGNATURES[name][1]), (name, n_args, len(_lib.SIGNATURES[name][1]))
    loaded = _lib.load()
    assert loaded.cb_version() == 5
    assert loaded.cb_ln_gelu_drop_bwd_workspace_bytes(65536, 256) == 2048 * 3 * 256 * 4
    # argument checks answer before anything is launched: a width the row kernels do not hold in registers, a missing workspace
    assert loaded.cb_ln_gelu_drop_fwd_f32(None, 4, 513, None, None, 1e-5, 0.0, 0, None, None, None, None) == -1
    assert b'd <= 512' in loaded.cb_last_error()
    assert loaded.cb_mse_rows_f32(None, 0, 4, None, 4, 0, None, ctypes.c_void_p(8), None, None, 0, None) == -3


def test_what_is_not_built_says_so():
    from gnn_tail_generalization_amd.MLP_model import SEMLP
    g = sr.load_case('student_semlp_2layer_headtail_iso')
    data = type('Data', (), {})()
    data.train_mask, data.test_mask = g['train_mask'], ~g['train_mask']
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    args = sr.student_args(g)
    args.train_which = 'GraphMLP'
    with pytest.raises(NotImplementedError, match='contrastive'):
        SEMLP(args, data, None)
    args = sr.student_args(g)
    args.SEMLP__include_part1out = 0
    with pytest.raises(NotImplementedError, match='second'):
        SEMLP(args, data, None)
    args = sr.student_args(g)
    args.SEMLP_topK_2_replace = 9
    m = SEMLP(args, data, None)
    m.teacherSE = g['teacherSE']
    with pytest.raises(NotImplementedError, match='K <= 8'):
        m.replacement(g['teacherSE'][:3])
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    t = trainer.__new__(trainer)
    t.args = sr.student_args(g)
    t.args.train_which, t.args.do_deg_analyze = 'GraphMLP', 0
    with pytest.raises(NotImplementedError, match='GraphMLP'):
        t.main()


def test_batch_size_is_clipped_to_the_train_nodes():
    g = sr.load_case('student_semlp_downgraded')
    args = sr.student_args(g, extra=['--batch_size=65536'])
    for k, v in g['args_after'].items():
        if k != 'batch_size':
            setattr(args, k, v)
    args.batch_size = 65536
    data = type('Data', (), {})()
    data.train_mask, data.test_mask = g['train_mask'], ~g['train_mask']
    data.train_idx, data.test_idx = torch.where(data.train_mask)[0], torch.where(data.test_mask)[0]
    from gnn_tail_generalization_amd.MLP_model import SEMLP
    SEMLP(args, data, None)
    assert args.batch_size == int(g['train_mask'].sum())
