"""Host-side checks (no GPU) of the aggregation ABI's struct arguments: every entry that takes a `const cb_csr_view*` (include/coldbrew_hip.h) answers
a bad view, every entry that takes a `const cb_trunk_store*` a bad store, and both the option combinations no kernel exists for, with the documented
code before anything is launched — and says which entry was called."""
import ctypes

import pytest

from gnn_tail_generalization_amd import _lib

P = ctypes.c_void_p(256)      # a non-null, 16-byte aligned stand-in: the checks under test never dereference it
D = 256


def _store(**over):
    f = dict(mix_src=None, ld_mix=0, mix_index=None, c_act=1.0, c_mix=0.0, drop_p=0.0, seed=0, seed_dev=None, row0=0, relu_bits=None, bits_relu_only=0,
             out_act=None, ld_act=0)
    f.update(over)
    return _lib.TrunkStore(**f)


STORE = _store()

# entry -> its arguments after the view, all valid for a 4-row graph of 256-wide rows
ENTRIES = {
    'cb_spmm_csr_f32': dict(h=P, h_bf16=0, ld_h=D, d=D, col_scale=None, row_scale=None, bias=None, relu=0, acc_init=None, ld_init=0, out=P, ld_out=D, stream=None),
    'cb_spmm_csr_fused_f32': dict(row_ids=None, h=P, h_bf16=0, ld_h=D, d=D, row_scale=None, bias=None, acc_init=None, ld_init=0, store=STORE, out_next=P,
                                  ld_next=D, stream=None),
    'cb_spmm_csr_lp_f32': (P, D, D, None, P, D, 0.5, None, P, D, None),
    'cb_spmm_csr_prop_f32': (P, D, D, None, P, D, 0.5, 0.0, 1.0, None, None, P, D, None),
    'cb_spmm_csr_store_bwd_f32': (P, D, D, None, P, None, 1.0, 0.0, 0, None, 0, None, 0, P, D, None),
    'cb_spmm_csr_store_bwd_mix_f32': (P, D, D, None, P, None, 1.0, 0.0, 0, None, 0, P, D, P, D, 0, None, None, None, 0.0, None, None, 0, None),
    'cb_spmm_gemm_f32': (P, D, D, None, None, 0, None, 0, P, D, P, None, None, 0, P, D, None),
    'cb_spmm_gemm_fused_f32': dict(acc_init=None, ld_init=0, h=P, ld_h=D, d=D, row_scale=None, bias=None, store=STORE, out_next=P, ld_next=D, skip_next=0, image=P,
                                   g_rowscale=None, g_addend=None, ld_add=0, g_out=P, ld_gout=D, stream=None),
    'cb_spmm_gemm_fused_head_f32': dict(acc_init=None, ld_init=0, h=P, ld_h=D, d=D, row_scale=None, bias=None, store=STORE, out_next=P, ld_next=D, skip_next=0,
                                        head_image=P, head_bias=None, C=8, logits=P, ld_logits=8, stream=None),
    'cb_spmm_gemm_store_rows_f32': dict(h=P, ld_h=D, d=D, col_scale=P, out=P, ld_out=D, image=P, g_rowscale=None, bias=None, row_ids=P, store=STORE, g_out=P,
                                        ld_gout=D, stream=None),
}

# the entries that apply the trunk's store without a graph (4 rows of 256 floats): name -> all their arguments
ROW_ENTRIES = {
    'cb_trunk_store_rows_f32': dict(y=P, row_index=P, n_rows=4, d=D, store=STORE, out=P, stream=None),
    'cb_gemm_nn_store_rows_f32': dict(A=P, lda=D, B=P, ldb=D, C=P, ldc=D, M=4, N=D, K=D, rowscale=None, addend=None, ld_add=0, bias=None, row_index=P, store=STORE,
                                      ws=None, ws_bytes=0, stream=None),
}
STORE_TAKERS = sorted([n for n, a in ENTRIES.items() if isinstance(a, dict) and 'store' in a] + list(ROW_ENTRIES))

# a store no kernel can apply: CB_E_INVALID from every entry that takes one
BAD_STORES = {
    'null': None,
    'drop_p=1': _store(drop_p=1.0),
    'row0=-1': _store(row0=-1),
    'ld_mix<d': _store(mix_src=P, ld_mix=D - 4),
}

# the combinations of the merged entries that stay unreachable: CB_E_INVALID
INVALID = [
    ('cb_spmm_csr_f32', dict(col_scale=P, h_bf16=1)),
    ('cb_spmm_csr_f32', dict(col_scale=P, acc_init=P, ld_init=D)),
    ('cb_spmm_csr_f32', dict(col_scale=P, bias=P)),
    ('cb_spmm_csr_f32', dict(col_scale=P, relu=1)),
    ('cb_spmm_csr_fused_f32', dict(row_ids=P, acc_init=P, ld_init=D)),
    ('cb_spmm_csr_fused_f32', dict(row_ids=P, h_bf16=1)),
    # the mix of the stores inside an aggregation over all node rows is taken at the node row
    ('cb_spmm_csr_fused_f32', dict(store=_store(mix_src=P, ld_mix=D, mix_index=P))),
    ('cb_spmm_gemm_fused_f32', dict(store=_store(mix_src=P, ld_mix=D, mix_index=P))),
    ('cb_spmm_gemm_fused_head_f32', dict(store=_store(mix_src=P, ld_mix=D, mix_index=P))),
    # the kernel writes a row's mask words as 16-byte vectors
    ('cb_spmm_gemm_store_rows_f32', dict(store=_store(relu_bits=ctypes.c_void_p(264)))),
]


def _view(**over):
    f = dict(rowptr=P, col=P, col_flags=0, n_rows=4, n_edges=4, hub_threshold=64, n_hubs=0, n_chunks=0, hub_rows=None, hub_chunk_ptr=None, ws=None, ws_bytes=0)
    f.update(over)
    return _lib.CsrView(**f)


def _call(name, view, **over):
    lib = _lib.load()
    if name in ROW_ENTRIES:      # (no graph: `view` is ignored)
        rc = getattr(lib, name)(*{**ROW_ENTRIES[name], **over}.values())
        return rc, lib.cb_last_error() or b''
    args = ENTRIES[name]
    args = tuple({**args, **over}.values()) if isinstance(args, dict) else args
    rc = getattr(lib, name)(view, *args)
    return rc, lib.cb_last_error() or b''


def test_the_table_covers_every_view_taking_entry():
    takers = {n for n, (_res, args) in _lib.SIGNATURES.items() if args and args[0] is ctypes.POINTER(_lib.CsrView)}
    assert takers == set(ENTRIES) and len(takers) == 10
    for name, args in ENTRIES.items():
        assert len(args) + 1 == len(_lib.SIGNATURES[name][1]), name
    # the struct mirrors the header's field for field (88 bytes with the C compiler's padding after col_flags and n_chunks)
    assert [f for f, _ in _lib.CsrView._fields_] == ['rowptr', 'col', 'col_flags', 'n_rows', 'n_edges', 'hub_threshold', 'n_hubs', 'n_chunks', 'hub_rows',
                                                    'hub_chunk_ptr', 'ws', 'ws_bytes']
    assert ctypes.sizeof(_lib.CsrView) == 88
    # so does the trunk store's (96 bytes: padding after drop_p and bits_relu_only), and the table names every entry that takes one
    assert [f for f, _ in _lib.TrunkStore._fields_] == ['mix_src', 'ld_mix', 'mix_index', 'c_act', 'c_mix', 'drop_p', 'seed', 'seed_dev', 'row0', 'relu_bits',
                                                       'bits_relu_only', 'out_act', 'ld_act']
    assert ctypes.sizeof(_lib.TrunkStore) == 96
    store_takers = {n for n, (_res, args) in _lib.SIGNATURES.items() if ctypes.POINTER(_lib.TrunkStore) in args}
    assert store_takers == set(STORE_TAKERS) and len(store_takers) == 6
    for name, args in ROW_ENTRIES.items():
        assert len(args) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_a_bad_view_is_answered_before_any_launch(name):
    key = name.encode()
    rc, msg = _call(name, None)
    assert rc == -1 and key in msg, (rc, msg)
    rc, msg = _call(name, _view(n_rows=2 ** 31))
    assert rc == -2 and key in msg, (rc, msg)
    rc, msg = _call(name, _view(hub_threshold=0))
    assert rc == -1 and key in msg and b'hub plan' in msg, (rc, msg)
    rc, msg = _call(name, _view(n_hubs=2, n_chunks=3, hub_rows=P, hub_chunk_ptr=P, ws=None))
    assert rc == -3 and key in msg and b'workspace' in msg, (rc, msg)
    # a workspace sized for narrower rows is refused too (3 chunks of 256 floats are needed)
    rc, msg = _call(name, _view(n_hubs=2, n_chunks=3, hub_rows=P, hub_chunk_ptr=P, ws=P, ws_bytes=3 * 255 * 4))
    assert rc == -3 and key in msg, (rc, msg)
    # an empty graph is not an error and needs no pointers
    assert _call(name, _lib.CsrView(n_rows=0, hub_threshold=0))[0] == 0


@pytest.mark.parametrize('name', STORE_TAKERS)
@pytest.mark.parametrize('bad', sorted(BAD_STORES))
def test_a_bad_store_is_answered_before_any_launch(name, bad):
    rc, msg = _call(name, _view(), store=BAD_STORES[bad])
    assert rc == -1 and name.encode() in msg, (rc, msg)


@pytest.mark.parametrize('name', sorted(set(STORE_TAKERS) - set(ROW_ENTRIES)))
def test_an_empty_graph_needs_no_store(name):
    assert _call(name, _lib.CsrView(n_rows=0, hub_threshold=0), store=None)[0] == 0


@pytest.mark.parametrize('name,over', INVALID, ids=[f'{n}-{"-".join(sorted(set(o) - {"ld_init"}))}' for n, o in INVALID])
def test_option_combinations_without_a_kernel_are_invalid(name, over):
    rc, msg = _call(name, _view(), **over)
    assert rc == -1 and name.encode() in msg, (rc, msg)
