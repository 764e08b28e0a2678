"""GPU: the sum-first layer of the rows-only forward in one kernel (cb_spmm_gemm_store_rows_f32: aggregation with the source-row factor, the 256 x 256
transform on the matrix cores and the trunk's store on a subset of the node rows) against the composition it replaces — CSRGraph.spmm(col_scale=...)
followed by gemm.mm_nn_store_rows — BIT FOR BIT: H, the stored rows, the ReLU output and the mask words (and the mask words of every other node row
left as they were).  Then one rows-only training step with each form: the same loss and gradients, bit for bit."""
import contextlib
import gc
import io
import os

import pytest
import torch

from gnn_tail_generalization_amd import tuning

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


class _Rows:
    def __init__(self, idx):
        self.idx, self.n = idx, int(idx.numel())


def _graph(n, n_isolated, T):
    """Power-law graph on n nodes + n_isolated nodes without edges (rows whose sum is empty)."""
    from gnn_tail_generalization_amd.data import synthetic_data
    from gnn_tail_generalization_amd.graph import CSRGraph
    ei = synthetic_data('S-pl1M', seed=7, device=DEV, n_override=n).edge_index
    return CSRGraph(ei, n + n_isolated, hub_threshold=T)


def _check_status():
    from gnn_tail_generalization_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().cb_device_status() == 0


# (n nodes, isolated nodes, hub threshold, rows of the subset): hub rows (threshold 16 / 64), a ragged last tile, |S| < 64, 1100 tiles on the persistent
# blocks (both LDS buffers and both mask-word buffers re-used many times)
@pytest.mark.parametrize('n,n_iso,T,n_rows', [(5003, 40, 16, 1013), (20000, 100, 256, 37), (20000, 0, 64, 19999), (90000, 300, 256, 70401)])
@pytest.mark.parametrize('conn', ['Initial', 'Residual'])
@pytest.mark.parametrize('p,seed_dev,row0', [(0.0, False, 0), (0.5, False, 0), (0.5, True, 4096)])
@pytest.mark.parametrize('compact_mix', [False, True])
def test_store_rows_kernel_equals_aggregation_then_store_rows(n, n_iso, T, n_rows, conn, p, seed_dev, row0, compact_mix, monkeypatch):
    from gnn_tail_generalization_amd import gemm, ops
    from gnn_tail_generalization_amd.graph import weight_image
    G = _graph(n, n_iso, T)
    N = G.N
    gen = torch.Generator(device=DEV).manual_seed(n + n_rows)
    idx = torch.sort(torch.randperm(N, device=DEV, generator=gen)[:n_rows])[0]
    if n_iso:      # at least one row without edges in the subset
        idx = torch.unique(torch.cat([idx[:-1], torch.tensor([N - 1], device=DEV)]))
    fwd = G._support_fwd(_Rows(idx), N, force=True)
    if T <= 64:
        assert fwd._plan.n_hubs > 0
    M = idx.numel()
    if seed_dev:
        monkeypatch.setattr(ops, '_graph_seed', torch.tensor([987654321], dtype=torch.int64, device=DEV))
    h = torch.randn(N, 256, device=DEV, generator=gen)
    a = torch.rand(N, device=DEV, generator=gen) + 0.5
    w = torch.randn(256, 256, device=DEV, generator=gen) * 0.07
    bias = torch.randn(256, device=DEV, generator=gen) * 0.1
    b_rows = torch.rand(M, device=DEV, generator=gen) + 0.5
    if compact_mix:      # the mix source is itself compact (the last layer reading the layer below's ReLU output on S_1)
        mix = torch.randn(M + 11, 256, device=DEV, generator=gen)
        mix_index = torch.randperm(M + 11, device=DEV, generator=gen)[:M].contiguous()
    else:
        mix, mix_index = torch.randn(N, 256, device=DEV, generator=gen), None
    relu_only = conn == 'Residual'
    want_act = relu_only
    c_act, c_mix, seed = 0.9, 0.1, 1234567
    bits_ref = torch.full((N, 1, 4), -7, dtype=torch.int64, device=DEV)
    bits_new = bits_ref.clone()
    h_ref = fwd.spmm(h, col_scale=a)
    out_ref, act_ref = gemm.mm_nn_store_rows(h_ref, w, b_rows, None, bias, idx, mix, mix_index, c_act, c_mix, p, seed, row0, bits_ref, relu_only, want_act)
    h_new, out_new, act_new = fwd.spmm_gemm_store_rows(h, a, weight_image(w), b_rows, bias, idx, mix, mix_index, c_act, c_mix, p, seed, row0, bits_new,
                                                       relu_only, want_act)
    _check_status()
    assert torch.equal(h_new, h_ref)
    assert torch.equal(out_new, out_ref)
    assert (act_new is None) == (act_ref is None)
    if act_ref is not None:
        assert torch.equal(act_new, act_ref)
    assert torch.equal(bits_new, bits_ref)      # the subset's rows and, untouched, every other row
    outside = torch.ones(N, dtype=torch.bool, device=DEV)
    outside[idx] = False
    assert bool((bits_new[outside] == -7).all())
    if p > 0:
        assert bool((out_new == 0).any())      # (the dropout is on)


def _rows_only_step(dataset, extra, layers=3):
    import bench
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd import trainer_node_classification as tnc
    args = bench.make_args(dataset, ['--manual_assign_GPU=0'] + list(extra), se='000', layers=layers)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        t = tnc.trainer(args, 0)
        t.setup_teacherGNN()
    t.teacherGNN.train()
    ops._seed_override[:] = [11, 12, 13, 14, 15]
    try:
        loss = t.training_loss()
        loss.backward()
    finally:
        ops._seed_override[:] = []
    _check_status()
    res = float(loss.detach()), {k: p.grad.detach().clone() for k, p in t.teacherGNN.named_parameters() if p.grad is not None}
    del t, loss
    gc.collect()
    torch.cuda.empty_cache()
    return res


@pytest.mark.parametrize('dataset,conn', [('S-pl1M', 'Initial'), ('S-pl1M', 'Residual'), ('S-pl10M', 'Initial')])
def test_rows_only_step_is_bit_identical_with_either_form(dataset, conn, monkeypatch):
    """One rows-only training step (the trainer's default) from the same state with the sum-first layers as one kernel and as aggregation + transform:
    the loss and every gradient are bitwise equal.  S-pl10M: the real S_1 / S_0 orientations of the benchmark's step."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    monkeypatch.setenv('CB_LOSS_ROWS', '1')
    monkeypatch.setenv('CB_ROWS_ONLY_FWD', '1')
    monkeypatch.delenv('CB_ROWS_ONLY_BELOW', raising=False)
    if dataset == 'S-pl1M':
        monkeypatch.setattr(tuning.T, 'sum_first_below_min_edges', 0)      # (S-pl1M sits below the break-even of the sum-first layer below)
    calls = []
    real = CSRGraph.spmm_gemm_store_rows
    monkeypatch.setattr(CSRGraph, 'spmm_gemm_store_rows', lambda self, *a, **k: (calls.append(self.N), real(self, *a, **k))[1])
    extra = () if conn == 'Initial' else ('--force_set_to_best_config=0', '--type_trick=Residual')
    loss_f, g_f = _rows_only_step(dataset, extra)
    assert len(calls) == 2      # the layer below the last one on S_1 and the last layer on S_0
    monkeypatch.setattr(tuning.T, 'agg_gemm_store_rows_min_edges', 1 << 62)
    loss_t, g_t = _rows_only_step(dataset, extra)
    assert len(calls) == 2
    assert loss_f == loss_t and set(g_f) == set(g_t)
    for k in g_t:
        assert torch.equal(g_f[k], g_t[k]), k
    assert os.environ.get('CB_ROWS_ONLY_FWD') == '1'
