"""Host-side contract (no GPU) of the dense GEMM entries (cb_gemm_*_f32, include/coldbrew_hip.h): every entry answers a bad size, an out-of-range size,
a null operand, a short leading dimension, a bad dropout, a missing workspace and an operand outside its fused form with the documented code before
anything is launched, and says which entry was called; empty problems need no pointers; the `_supported` predicates and the workspace sizes are pinned
over a fixed grid.  Only paths that return before any launch or memset are called.

The grid's expected values (tests/golden/gemm_host_grid.json) were recorded once, by running this file as a script, from a library built from the
commit BEFORE the entries were folded into one NN and one TN host core (2b19daa), never from the code under test: a later GEMM variant that changes a
value there changes a launch decision or an allocation and has to say so."""
import ctypes
import json
import os

import pytest

from gnn_tail_generalization_amd import _lib

P = ctypes.c_void_p(256)      # a non-null, 16-byte aligned stand-in: the checks under test never dereference it
Q = ctypes.c_void_p(260)      # the same, misaligned
D = 256
STORE = _lib.TrunkStore(c_act=1.0)

_NN = dict(A=P, lda=D, B=P, ldb=D, C=P, ldc=D)
_NN2 = dict(_NN, C2=P, ldc2=D)
_MNK = dict(M=4, N=D, K=D)
_EPI = dict(rowscale=None, addend=None, ld_add=0, bias=None)
_WS = dict(ws=None, ws_bytes=0, stream=None)
_TN = dict(A=P, lda=D, G=P, ldg=D)
_DEV = dict(seed_dev=None, row0=0)

# entry -> all its arguments in the ABI's order, valid for M = 4 and N = K = 256 (K1 = K2 = 256).  cb_gemm_tn_instage_f32 exists from 32 768 rows on
# (256 row slabs) and for 64 < K2 <= 128: its tuple is the smallest shape it accepts.
ENTRIES = {
    'cb_gemm_nn_f32': dict(_NN, **_MNK, **_EPI, relu=1, **_WS),
    'cb_gemm_nn_bf16out_f32': dict(_NN, **_MNK, **_EPI, relu=1, **_WS),
    'cb_gemm_nn_drop2_f32': dict(_NN2, **_MNK, **_EPI, relu=1, drop_p=0.5, seed=1, **_DEV, **_WS),
    'cb_gemm_nn_indrop_drop2_f32': dict(_NN2, **_MNK, bias=None, relu=1, a_drop_p=0.5, a_seed=1, drop_p=0.5, seed=2, **_DEV, relu_bits=None, stream=None),
    'cb_gemm_nn_indrop_f32': dict(_NN, **_MNK, **_EPI, relu=1, a_drop_p=0.5, a_seed=1, **_DEV, relu_bits=None, stream=None),
    'cb_gemm_nn_store_rows_f32': dict(_NN, **_MNK, **_EPI, row_index=P, store=STORE, **_WS),
    'cb_gemm_tn_f32': dict(_TN, rowscale=None, C=P, M=4, K1=D, K2=D, **_WS),
    'cb_gemm_tn_gdrop_f32': dict(_TN, C=P, M=4, K1=D, K2=D, g_drop_p=0.5, g_seed=1, **_DEV, **_WS),
    'cb_gemm_tn_adrop_f32': dict(_TN, rowscale=None, C=P, M=4, K1=D, K2=D, a_drop_p=0.5, a_seed=1, **_DEV, **_WS),
    'cb_gemm_tn_instage_f32': dict(g=P, mfold=P, x0_bits=P, X=P, ldx=128, C=P, colsum=P, M=32768, K2=128, g_drop_p=0.5, g_seed=1, x_drop_p=0.5, x_seed=2,
                                   **_DEV, **_WS),
}
NN = sorted(n for n in ENTRIES if '_nn_' in n)
TN = sorted(n for n in ENTRIES if '_tn_' in n)
INSTAGE = 'cb_gemm_tn_instage_f32'
STORE_ROWS = 'cb_gemm_nn_store_rows_f32'
# the entries that exist in a fused form only -> the predicate their refusal names (the two TN operand dropouts name only themselves)
FUSED_ONLY = {
    'cb_gemm_nn_indrop_drop2_f32': b'cb_gemm_nn_indrop_supported',
    'cb_gemm_nn_indrop_f32': b'cb_gemm_nn_indrop_supported',
    STORE_ROWS: b'cb_gemm_nn_store_rows_supported',
    'cb_gemm_tn_gdrop_f32': b'',
    'cb_gemm_tn_adrop_f32': b'',
    INSTAGE: b'cb_gemm_tn_instage_supported',
}
# the dropouts that must be active (0 < p): the entry without them is another entry
ACTIVE_P = [(n, k) for n in sorted(FUSED_ONLY) for k in ENTRIES[n] if k.endswith('drop_p')]
ANY_P = [(n, k) for n in sorted(ENTRIES) for k in ENTRIES[n] if k.endswith('drop_p')]
# the first operand of each entry and the leading dimension that goes with its row length
FIRST = {n: ('g', 'ldx') if n == INSTAGE else ('A', 'lda') for n in ENTRIES}


def _call(name, **over):
    lib = _lib.load()
    args = {**ENTRIES[name], **over}
    assert len(args) == len(ENTRIES[name]), set(over) - set(ENTRIES[name])
    rc = getattr(lib, name)(*args.values())
    return rc, lib.cb_last_error() or b''


def _refused(name, code, says=b'', **over):
    rc, msg = _call(name, **over)
    assert rc == code and name.encode() in msg and says in msg, (name, over, rc, msg)


def test_the_table_covers_every_gemm_entry():
    entries = {n for n in _lib.SIGNATURES if n.startswith('cb_gemm_') and n.endswith('_f32')}
    assert entries == set(ENTRIES) and len(entries) == 10
    for name, args in ENTRIES.items():
        assert len(args) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_a_bad_size_a_null_operand_and_a_short_row_are_refused(name):
    _refused(name, -1, M=-1)
    _refused(name, -1, **{'K2' if name in TN else 'N': -1})
    _refused(name, -1, C=None)
    _refused(name, -1, **{FIRST[name][0]: None})
    ld = FIRST[name][1]
    _refused(name, -1, **{ld: ENTRIES[name][ld] - 4})
    if 'ldc' in ENTRIES[name]:
        _refused(name, -1, ldc=D - 4)
    if 'ldc2' in ENTRIES[name]:
        _refused(name, -1, C2=None)
        _refused(name, -1, ldc2=D - 4)
    if 'addend' in ENTRIES[name]:
        _refused(name, -1, addend=P, ld_add=D - 4)
    if 'row_index' in ENTRIES[name]:
        _refused(name, -1, row_index=None)


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_a_size_past_the_range_is_a_range_error(name):
    """N, K < 2^24 (NN) and K1, K2 < 2^20 (TN), reported before any pointer is looked at.  Two entries fix their width and answer it as a bad size:
    cb_gemm_nn_store_rows_f32 (N == 256; its K is ranged) and cb_gemm_tn_instage_f32 (K1 == 256, 64 < K2 <= 128 by its predicate)."""
    if name == INSTAGE:
        _refused(name, -1, b'cb_gemm_tn_instage_supported', K2=2 ** 20, ldx=2 ** 20)
    elif name == STORE_ROWS:
        _refused(name, -1, N=2 ** 24)
        _refused(name, -2, K=2 ** 24, A=None)
    elif name in TN:
        _refused(name, -2, K1=2 ** 20, A=None)
        _refused(name, -2, K2=2 ** 20, C=None)
    else:
        _refused(name, -2, N=2 ** 24, C=None)
        _refused(name, -2, K=2 ** 24, A=None)
        _refused(name, -2, M=2 ** 30 * 64, C=None)
    if name != INSTAGE:
        _refused(name, -1, M=-1, **{'K1' if name in TN else 'K': 2 ** 24})      # a negative size is answered first


@pytest.mark.parametrize('name', sorted(n for n in ENTRIES if 'row0' in ENTRIES[n]))
def test_a_negative_row_offset_is_refused(name):
    _refused(name, -1, row0=-1)


@pytest.mark.parametrize('name,p', ANY_P, ids=[f'{n}-{k}' for n, k in ANY_P])
def test_a_dropout_of_everything_is_refused(name, p):
    _refused(name, -1, **{p: 1.0})
    _refused(name, -1, **{p: -0.25})


@pytest.mark.parametrize('name,p', ACTIVE_P, ids=[f'{n}-{k}' for n, k in ACTIVE_P])
def test_the_fused_dropouts_must_be_active(name, p):
    _refused(name, -1, **{p: 0.0})


@pytest.mark.parametrize('name', sorted(n for n in ENTRIES if 'relu_bits' in ENTRIES[n]))
def test_relu_mask_words_exist_for_256_columns_with_relu_only(name):
    _refused(name, -1, relu_bits=P, N=128)
    _refused(name, -1, relu_bits=P, relu=0)
    _refused(name, -1, relu_bits=ctypes.c_void_p(260))


@pytest.mark.parametrize('name', TN)
def test_a_tn_contraction_needs_its_workspace(name):
    lib = _lib.load()
    a = ENTRIES[name]
    need = lib.cb_gemm_tn_instage_workspace_bytes(a['M'], a['K2']) if name == INSTAGE else lib.cb_gemm_tn_workspace_bytes(a['M'], a['K1'], a['K2'])
    assert need > 0
    _refused(name, -3, b'workspace', ws=None, ws_bytes=need)
    _refused(name, -3, b'workspace', ws=P, ws_bytes=need - 1)


@pytest.mark.parametrize('name', sorted(FUSED_ONLY))
def test_an_operand_outside_the_fused_form_is_refused(name):
    _refused(name, -1, FUSED_ONLY[name], **{FIRST[name][0]: Q})
    second = {'cb_gemm_tn_gdrop_f32': 'G', 'cb_gemm_tn_adrop_f32': 'G', INSTAGE: 'X'}.get(name, 'B')
    _refused(name, -1, FUSED_ONLY[name], **{second: Q})
    if 'addend' in ENTRIES[name]:
        _refused(name, -1, FUSED_ONLY[name], addend=Q, ld_add=D)
        _refused(name, -1, FUSED_ONLY[name], addend=P, ld_add=D + 1)
    if name == 'cb_gemm_tn_adrop_f32':      # the dropped operand is staged by the 128-row tile only
        _refused(name, -1, K1=64, lda=64)


_NULLS = dict(A=None, B=None, G=None, C=None, C2=None, row_index=None, store=None)


@pytest.mark.parametrize('name', sorted(set(ENTRIES) - {INSTAGE}))
def test_an_empty_problem_needs_no_pointers(name):
    nulls = {k: v for k, v in _NULLS.items() if k in ENTRIES[name]}
    empty = ['K1', 'K2'] if name in TN else ['M'] if name == STORE_ROWS else ['M', 'N']
    for k in empty:
        assert _call(name, **nulls, **{k: 0})[0] == 0, (name, k)
    if name in TN:      # no rows: the output is still written (zeros), so it must exist
        _refused(name, -1, M=0, C=None)


def test_the_input_stage_gemm_has_no_empty_form():
    _refused(INSTAGE, -1, M=0)
    _refused(INSTAGE, -1, K2=0)


# ---- the pure host functions over a fixed grid -------------------------------------------------------------------------------------------------------------
MS = [1, 300, 2708, 32768, 10 ** 7]
WIDTHS = [8, 40, 64, 68, 128, 132, 256, 1433]
# (first operand, second operand, added to every leading dimension)
ALIGN = [(256, 256, 0), (260, 256, 0), (256, 260, 0), (256, 256, 1)]


def host_values(lib):
    """name -> the function over the grid, in a fixed order: predicates as a string of 0 / 1, sizes as a list."""
    bits = lambda xs: ''.join(str(int(x)) for x in xs)
    v = {
        'cb_gemm_nn_workspace_bytes': [lib.cb_gemm_nn_workspace_bytes(n, k) for n in WIDTHS for k in WIDTHS],
        'cb_gemm_nn_splitk_workspace_bytes': [lib.cb_gemm_nn_splitk_workspace_bytes(m, n, k) for m in MS for n in WIDTHS for k in WIDTHS],
        'cb_gemm_tn_workspace_bytes': [lib.cb_gemm_tn_workspace_bytes(m, k1, k2) for m in MS for k1 in WIDTHS for k2 in WIDTHS],
        'cb_gemm_tn_instage_workspace_bytes': [lib.cb_gemm_tn_instage_workspace_bytes(m, k2) for m in MS for k2 in WIDTHS],
        'cb_gemm_nn_indrop_supported': bits(lib.cb_gemm_nn_indrop_supported(a, k + e, b, n + e, 256, n + e, 256, n + e, m, n, k)
                                            for a, b, e in ALIGN for m in MS for n in WIDTHS for k in WIDTHS),
        'cb_gemm_nn_store_rows_supported': bits(lib.cb_gemm_nn_store_rows_supported(a, k + e, b, n + e, 256, n + e, m, n, k)
                                                for a, b, e in ALIGN for m in MS for n in WIDTHS for k in WIDTHS),
        'cb_gemm_tn_gdrop_supported': bits(lib.cb_gemm_tn_gdrop_supported(a, k1 + e, g, k2 + e, k1, k2) for a, g, e in ALIGN for k1 in WIDTHS for k2 in WIDTHS),
        'cb_gemm_tn_adrop_supported': bits(lib.cb_gemm_tn_adrop_supported(a, k1 + e, g, k2 + e, k1, k2) for a, g, e in ALIGN for k1 in WIDTHS for k2 in WIDTHS),
        'cb_gemm_tn_instage_supported': bits(lib.cb_gemm_tn_instage_supported(g, g, x, k2 + e, m, k2) for g, x, e in ALIGN for m in MS for k2 in WIDTHS),
    }
    # zero and negative sizes need no workspace
    v['no_workspace'] = [lib.cb_gemm_nn_splitk_workspace_bytes(0, 64, 1433), lib.cb_gemm_nn_splitk_workspace_bytes(2708, -1, 1433),
                         lib.cb_gemm_tn_workspace_bytes(0, 256, 256), lib.cb_gemm_tn_workspace_bytes(300, 256, -1),
                         lib.cb_gemm_tn_instage_workspace_bytes(0, 128), lib.cb_gemm_tn_instage_workspace_bytes(32768, 0)]
    return v


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_host_grid.json')) as _f:
    EXPECTED = json.load(_f)


def test_the_table_of_host_functions_is_complete():
    pure = {n for n in _lib.SIGNATURES if n.startswith('cb_gemm_') and (n.endswith('_supported') or n.endswith('_workspace_bytes'))}
    assert pure == set(EXPECTED) - {'no_workspace'} and len(pure) == 9


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_predicates_and_workspace_sizes_over_the_grid(name):
    got = host_values(_lib.load())[name]
    assert len(got) == len(EXPECTED[name]) and got == EXPECTED[name], [i for i, (a, b) in enumerate(zip(got, EXPECTED[name])) if a != b][:8]


if __name__ == '__main__':      # prints the recorded values (see the docstring: from the build they are pinned to, not from the one under test)
    print(json.dumps(host_values(_lib.load()), indent=0))
