"""Host-side checks (no GPU) of the C ABI of csrc/cb_ncloss.hip: every entry is declared, exported and bound with matching argument
counts; bad sizes and short workspaces are refused before anything is launched; the operator refuses what it documents."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ['cb_ncloss_positions_i64', 'cb_ncloss_row_norms_f32', 'cb_cosine_scale_f32', 'cb_ncloss_uses_limb_core', 'cb_ncloss_workspace_bytes',
               'cb_ncloss_fwd_f32', 'cb_ncloss_normalize_rows_f32', 'cb_ncloss_bwd_slab_f32', 'cb_ncloss_bwd_finish_f32']
P8 = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: the checks below answer before any launch


def test_c_abi_of_the_ncloss_kernels():
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
    assert {n for n in declared if 'ncloss' in n or 'cosine' in n} == set(NEW_ENTRIES)
    assert _lib.load().cb_version() == 5


def test_bad_sizes_and_short_workspaces_are_refused_before_any_launch():
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    # one slab of 128 columns per split; the cap limits the splits
    assert lib.cb_ncloss_workspace_bytes(0, 0) == 0
    assert lib.cb_ncloss_workspace_bytes(127, 0) == 127 * 4
    assert lib.cb_ncloss_workspace_bytes(640, 0) == 5 * 640 * 4
    assert lib.cb_ncloss_workspace_bytes(640, 2) == 2 * 640 * 4
    assert lib.cb_ncloss_workspace_bytes(65536, 0) == 2 * 65536 * 4      # 512 row blocks: ceil(1024 / 512) = 2 splits
    assert lib.cb_ncloss_positions_i64(None, -1, 5, None, None, None) == -1
    assert lib.cb_ncloss_positions_i64(P8, 4, 2 ** 31, P8, P8, None) == -2
    assert lib.cb_ncloss_positions_i64(None, 4, 5, P8, P8, None) == -1 and b'null' in lib.cb_last_error()
    assert lib.cb_ncloss_row_norms_f32(P8, 3, 4, 8, P8, None, None) == -1      # ldx < D
    assert lib.cb_ncloss_row_norms_f32(P8, 8, 4, 8, None, None, None) == -1    # nothing to write
    assert lib.cb_cosine_scale_f32(P8, 3, 4, P8, None) == -1
    assert lib.cb_cosine_scale_f32(P8, 70000, 70000, P8, None) == -2
    fwd = [P8, 8, 4, 8, 0.5, P8, P8, P8, 10, P8, P8, P8, 0, P8, P8, P8, P8, P8, P8, P8]

    def call_fwd(args, ws=P8, wsb=4 * 4):
        return lib.cb_ncloss_fwd_f32(*args, ws, wsb, None)
    assert call_fwd(fwd, None, 0) == -3 and b'workspace' in lib.cb_last_error()
    assert call_fwd(fwd, P8, 4 * 4 - 1) == -3
    bad = list(fwd)
    bad[4] = 0.0                                                               # tau
    assert call_fwd(bad) == -1 and b'tau' in lib.cb_last_error()
    bad = list(fwd)
    bad[1] = 7                                                                 # ldz < D
    assert call_fwd(bad) == -1
    bad = list(fwd)
    bad[2] = 0                                                                 # B
    assert call_fwd(bad) == -1
    bad = list(fwd)
    bad[5] = None                                                              # rowptr
    assert call_fwd(bad) == -1 and b'null' in lib.cb_last_error()
    bad = list(fwd)
    bad[3] = 1 << 24                                                           # D
    bad[1] = 1 << 24
    assert call_fwd(bad) == -2
    slab = [P8, 8, 300, 8, 0.5, P8, P8, 128, 128, 0, P8, 300, None]
    for pos, val in ((7, 64), (8, 0), (8, 173), (11, 299), (4, -1.0), (10, None)):      # row0 not a tile multiple, no rows, past B, ldp < B, tau, P
        bad = list(slab)
        bad[pos] = val
        assert lib.cb_ncloss_bwd_slab_f32(*bad) == -1, (pos, val)
    assert lib.cb_ncloss_normalize_rows_f32(P8, 8, 4, 8, None, P8, None) == -1
    fin = [P8, 8, P8, 4, 8, 0.5, P8, P8, P8, P8, P8, P8, P8, P8, 10, P8, P8, P8, P8, P8, P8, None]
    for pos, val in ((11, None), (18, None), (14, 0), (5, 0.0), (1, 7)):               # rowptr_t, g, n, tau, ldz
        bad = list(fin)
        bad[pos] = val
        assert lib.cb_ncloss_bwd_finish_f32(*bad) == -1, (pos, val)
    assert lib.cb_ncloss_uses_limb_core(ctypes.c_void_p(1 << 20), 256, 256) == (0 if os.environ.get('CB_GEMM_PLAIN_F32') else 1)
    assert lib.cb_ncloss_uses_limb_core(ctypes.c_void_p(1 << 20), 30, 30) == 0
    assert lib.cb_ncloss_uses_limb_core(ctypes.c_void_p((1 << 20) + 4), 256, 256) == 0


def test_the_operator_refuses_what_it_documents():
    from gnn_tail_generalization_amd import _lib, ops, tuning
    import ncloss_ref as nr
    with pytest.raises(_lib.HipExtensionError):                                # no CPU fallback
        ops.neighbor_contrastive_loss(torch.zeros(4, 8), ops.SparsePower(nr.power('powerlaw', 2), 'cpu'), torch.arange(4), 0.5)
    with pytest.raises(_lib.HipExtensionError):
        ops.cosine_sim(torch.zeros(4, 8))
    with pytest.raises(ValueError, match='square'):
        ops.SparsePower(torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (2, 3)), 'cpu')
    keep = tuning.T.ncloss_slab_rows
    try:
        tuning.T.ncloss_slab_rows = 100
        with pytest.raises(ValueError, match='multiple of 128'):
            ops._ncloss_slab_rows(640)
        tuning.T.ncloss_slab_rows = 0
        assert ops._ncloss_slab_rows(65536) == 4096 and ops._ncloss_slab_rows(4096) == 65536 and ops._ncloss_slab_rows(1 << 22) == 128
    finally:
        tuning.T.ncloss_slab_rows = keep
