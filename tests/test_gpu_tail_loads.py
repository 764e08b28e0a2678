"""GPU: the matrix-core tails after their per-row loads moved out of the store loops (csrc/cb_agg_gemm.hip, csrc/cb_front.hip; profiles/tail_loads.md).
The tails now take a row's scale / node row id / mixed-in row index from a register of lane `row` (loaded once per tile, before the K loop) and the
forward front prefetches the next tile's x and row scales, so what can break is the lane <-> row mapping (a shifted or clamped lane), a read past
the last row, and the prefetch past a block's last tile.  Everything is compared BIT FOR BIT (torch.equal) with the two-kernel compositions of
test_gpu_agg_gemm.py, test_gpu_agg_gemm_store_rows.py and test_gpu_kernels.py::test_forward_front_kernel_equals_the_two_gemms, at row counts
around the 64-row tile and the persistent grids, with a random scale per row; and one rows-only and one dense training step at S-pl1M reproduce
the digests recorded with the build before the change (tests/golden/tail_loads_steps_S-pl1M.json)."""
import contextlib
import functools
import gc
import hashlib
import io
import json
import os

import pytest
import torch

from gnn_tail_generalization_amd import tuning

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tail_loads_steps_S-pl1M.json')


def _status_ok():
    from gnn_tail_generalization_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().cb_device_status() == 0


@functools.lru_cache(maxsize=4)
def _graph(n, T):
    """Directed random multigraph on n rows, ~12 edges a row, a self-loop on every row (no empty degree), a few rows of 300+ in-edges: hub rows under
    either threshold, and under threshold 8 most rows."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    gen = torch.Generator(device=DEV).manual_seed(1000 + n)
    e = 12 * n
    src = torch.randint(0, n, (e,), device=DEV, generator=gen)
    dst = torch.randint(0, n, (e,), device=DEV, generator=gen)
    hub_dst = torch.randint(0, n, (4,), device=DEV, generator=gen).repeat_interleave(300)
    hub_src = torch.randint(0, n, (hub_dst.numel(),), device=DEV, generator=gen)
    loops = torch.arange(n, device=DEV)
    ei = torch.stack([torch.cat([src, hub_src, loops]), torch.cat([dst, hub_dst, loops])])
    G = CSRGraph(ei, n, hub_threshold=T)
    assert G._plan.n_hubs > 0
    return G


# 70 001 rows = 1094 tiles on one persistent block per CU: every block re-uses both LDS buffers
@pytest.mark.parametrize('T', [8, 256])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 127, 70001])
def test_spmm_gemm_row_scale_and_addend_follow_their_rows(n, T):
    """cb_spmm_gemm_f32, plain and reverse orientation, with and without a row scale and an addend for the tail: g_out bit-identical to cb_spmm_csr_f32
    followed by cb_gemm_nn_f32.  The row scale is random per row (a lane off by one shows in every row) and holds exactly n elements."""
    from gnn_tail_generalization_amd import gemm
    from gnn_tail_generalization_amd.graph import weight_image
    G = _graph(n, T)
    gen = torch.Generator(device=DEV).manual_seed(5 + n)
    h = torch.randn(n, 256, device=DEV, generator=gen)
    w = torch.randn(256, 256, device=DEV, generator=gen) * 0.07
    a = (torch.rand(n, device=DEV, generator=gen) + 0.5).clone()
    le = torch.randn(n, 256, device=DEV, generator=gen)
    assert a.numel() == n and a.untyped_storage().nbytes() == 4 * n
    img = weight_image(w)
    for transpose in (False, True):
        ref = G.spmm(h, transpose=transpose)
        for rs, addend in ((a, None), (None, None), (a, le), (None, le)):
            out, g = G.spmm_gemm(h, img, transpose=transpose, g_rowscale=rs, g_addend=addend)
            assert torch.equal(out, ref)
            assert torch.equal(g, gemm.mm_nn(ref, w, rowscale=rs, addend=addend)), (transpose, rs is not None, addend is not None)
    _status_ok()


@pytest.mark.parametrize('C', [3, 40, 64])
@pytest.mark.parametrize('n', [65, 777, 70001])
def test_fused_store_gemm_and_head_tails(n, C):
    """cb_spmm_gemm_fused_f32 (row scale, with and without an addend) and cb_spmm_gemm_fused_head_f32 (non-zero bias, loaded once per wavefront now):
    mask words, stored rows, Z_next / logits bit-identical to cb_spmm_csr_fused_f32 followed by cb_gemm_nn_f32.  C = 3: cb_gemm_nn_f32 has no limb
    kernel for rows of 3 floats, so the reference is the 4-column product with a zero fourth column (an output column depends on its own weight
    column alone), whose first three columns are the same bits."""
    from gnn_tail_generalization_amd import gemm, trunk
    from gnn_tail_generalization_amd.graph import head_image, weight_image
    G = _graph(n, 64)
    gen = torch.Generator(device=DEV).manual_seed(6 + n + C)
    z = torch.randn(n, 256, device=DEV, generator=gen)
    x0 = torch.randn(n, 256, device=DEV, generator=gen)
    w = torch.randn(256, 256, device=DEV, generator=gen) * 0.07
    bias = torch.randn(256, device=DEV, generator=gen)
    le = torch.randn(n, 256, device=DEV, generator=gen)
    a = (torch.rand(n, device=DEV, generator=gen) + 0.5).clone()
    p = 0.2
    bits_r, nxt_r, _ = trunk._fused_spmm(G, z, bias, x0, 0.9, 0.1, p, 4242)
    for addend in (le, None):
        bits, nxt, zn = trunk._fused_gemm_launch(G, z, bias, x0, 0.9, 0.1, p, 4242, weight_image(w), a, addend)
        assert torch.equal(bits, bits_r) and torch.equal(nxt, nxt_r)
        assert torch.equal(zn, gemm.mm_nn(nxt_r, w, rowscale=a, addend=addend))
    w_out = torch.randn(C, 256, device=DEV, generator=gen) * 0.07          # nn.Linear layout
    b_out = torch.randn(C, device=DEV, generator=gen) + 0.25
    assert bool((b_out != 0).all())
    C4 = (C + 3) // 4 * 4
    w_pad = torch.zeros(C4, 256, device=DEV)
    w_pad[:C] = w_out
    b_pad = torch.zeros(C4, device=DEV)
    b_pad[:C] = b_out
    want = gemm.mm_nn(nxt_r, w_pad.t().contiguous(), bias=b_pad)[:, :C]
    bits, nxt, logits = trunk._fused_gemm_launch(G, z, bias, x0, 0.9, 0.1, p, 4242, head_image(w_out), None, None, head=(b_out, C))
    assert logits.shape == (n, C) and torch.equal(bits, bits_r) and torch.equal(nxt, nxt_r)
    assert torch.equal(logits, want)
    _status_ok()


class _Rows:
    def __init__(self, idx):
        self.idx, self.n = idx, int(idx.numel())


# (rows of the subset): one row, a full tile, a tile and one row, two tiles less one, 1101 tiles (both LDS buffers and both mask-word buffers re-used)
@pytest.mark.parametrize('compact_mix', [False, True])
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('n_rows', [1, 64, 65, 127, 70401])
def test_store_rows_tail_takes_row_id_scale_and_mix_row_from_the_right_lane(n_rows, p, compact_mix):
    """cb_spmm_gemm_store_rows_f32 on a 90 000-row graph against CSRGraph.spmm(col_scale=...) followed by gemm.mm_nn_store_rows: H, the stored rows, the
    ReLU output and the mask words.  The node row ids have irregular gaps (a sorted random subset), the row scale is random per subset row, the mix
    comes by node row or through a permuted mix_index; the mask words of every node row outside the subset keep their sentinel."""
    from gnn_tail_generalization_amd import gemm
    from gnn_tail_generalization_amd.graph import weight_image
    N = 90000
    G = _graph(N, 256)
    gen = torch.Generator(device=DEV).manual_seed(N + n_rows)
    idx = torch.sort(torch.randperm(N, device=DEV, generator=gen)[:n_rows])[0].contiguous()
    fwd = G._support_fwd(_Rows(idx), N, force=True)
    M = idx.numel()
    h = torch.randn(N, 256, device=DEV, generator=gen)
    a = torch.rand(N, device=DEV, generator=gen) + 0.5
    w = torch.randn(256, 256, device=DEV, generator=gen) * 0.07
    bias = torch.randn(256, device=DEV, generator=gen) * 0.1
    b_rows = (torch.rand(M, device=DEV, generator=gen) + 0.5).clone()
    if compact_mix:
        mix = torch.randn(M + 11, 256, device=DEV, generator=gen)
        mix_index = torch.randperm(M + 11, device=DEV, generator=gen)[:M].contiguous()
    else:
        mix, mix_index = torch.randn(N, 256, device=DEV, generator=gen), None
    c_act, c_mix, seed, row0 = 0.9, 0.1, 1234567, 4096
    bits_ref = torch.full((N, 1, 4), -7, dtype=torch.int64, device=DEV)
    bits_new = bits_ref.clone()
    h_ref = fwd.spmm(h, col_scale=a)
    out_ref, act_ref = gemm.mm_nn_store_rows(h_ref, w, b_rows, None, bias, idx, mix, mix_index, c_act, c_mix, p, seed, row0, bits_ref, False, True)
    h_new, out_new, act_new = fwd.spmm_gemm_store_rows(h, a, weight_image(w), b_rows, bias, idx, mix, mix_index, c_act, c_mix, p, seed, row0, bits_new,
                                                       False, True)
    _status_ok()
    assert torch.equal(h_new, h_ref)
    assert torch.equal(out_new, out_ref)
    assert torch.equal(act_new, act_ref)
    assert torch.equal(bits_new, bits_ref)
    outside = torch.ones(N, dtype=torch.bool, device=DEV)
    outside[idx] = False
    assert bool((bits_new[outside] == -7).all()) and bool((bits_new[idx] != -7).any())


def _front_grid():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count      # the persistent grid of cb_trunk_front_f32: two blocks per CU


# M in units of the persistent grid B: no second tile anywhere; the prefetched tile absent, ragged (one row) or full for some blocks; a block's third tile
_FRONT_M = {'1': lambda B: 1, '64': lambda B: 64, '65': lambda B: 65, '64B': lambda B: 64 * B, '64B+1': lambda B: 64 * B + 1,
            '64(B+1)-1': lambda B: 64 * (B + 1) - 1, '128B+3': lambda B: 128 * B + 3}


@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('K', [64, 128])
@pytest.mark.parametrize('m_of', sorted(_FRONT_M))
def test_front_kernel_prefetch_of_the_next_tile(m_of, K, p):
    """cb_trunk_front_f32 with the next tile's x and row scales prefetched: X0, mask words and Z0 bit-identical to dropout + cb_gemm_nn_f32 (bias, ReLU)
    + dropout + cb_gemm_nn_f32 (row scale, addend), with and without the row scale and the addend."""
    from gnn_tail_generalization_amd import gemm, ops
    M = _FRONT_M[m_of](_front_grid())
    gen = torch.Generator(device=DEV).manual_seed(M + K)
    x = torch.rand(M, K, device=DEV, generator=gen)
    w_in = torch.randn(256, K, device=DEV, generator=gen) * 0.1
    b_in = torch.randn(256, device=DEV, generator=gen) * 0.1
    w0 = torch.randn(256, 256, device=DEV, generator=gen) * 0.07
    a = (torch.rand(M, device=DEV, generator=gen) + 0.5).clone()
    le = torch.randn(M, 256, device=DEV, generator=gen)
    sx, s0, row0 = 0x1234ABCD5, 0x77, 77
    xd = ops._dropout_raw(x, p, sx, row0 * K) if p > 0 else x
    x0_ref = gemm.mm_nn(xd, w_in.t().contiguous(), bias=b_in, relu=True)
    x0d_ref = ops._dropout_raw(x0_ref, p, s0, row0 * 256) if p > 0 else x0_ref
    pos = x0_ref > 0
    sh = torch.arange(64, device=DEV, dtype=torch.int64)
    bits_ref = torch.stack([(pos[:, kk::4].to(torch.int64) << sh).sum(dim=1) for kk in range(4)], dim=1)
    for rs, addend in ((a, None), (None, None), (a, le), (None, le)):
        fr = gemm.trunk_front(x, w_in, b_in, w0, rs, addend, p, sx, s0, row0, want_bits=True, want_drop=False)
        assert fr is not None
        x0, bits, _, z0 = fr
        assert torch.equal(x0, x0_ref)
        assert torch.equal(bits[:, 0, :], bits_ref)
        assert torch.equal(z0, gemm.mm_nn(x0d_ref, w0, rowscale=rs, addend=addend)), (rs is not None, addend is not None)
    _status_ok()


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def step_digests(kind):
    """sha256 of the loss and of every gradient of one training step at S-pl1M from the initial weights with fixed dropout seeds: kind 'rows_only' (the
    trainer's default: rows-only forward through cb_spmm_gemm_store_rows_f32, row-sparse backward) or 'dense' (CB_LOSS_ROWS=0: every row of every layer,
    the dense backward levels through cb_spmm_gemm_f32).  Also returns how many launches of the two entries the step made."""
    import bench
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd import trainer_node_classification as tnc
    from gnn_tail_generalization_amd.graph import CSRGraph
    calls = {'spmm_gemm_store_rows': 0, 'spmm_gemm': 0}
    real = {k: getattr(CSRGraph, k) for k in calls}
    keep_env = {k: os.environ.get(k) for k in ('CB_LOSS_ROWS', 'CB_ROWS_ONLY_FWD', 'CB_ROWS_ONLY_BELOW')}
    keep_min = tuning.T.sum_first_below_min_edges

    def counted(name):
        def f(self, *a, **k):
            calls[name] += 1
            return real[name](self, *a, **k)
        return f
    try:
        for k in calls:
            setattr(CSRGraph, k, counted(k))
        os.environ['CB_LOSS_ROWS'] = '1' if kind == 'rows_only' else '0'
        os.environ['CB_ROWS_ONLY_FWD'] = '1'
        os.environ.pop('CB_ROWS_ONLY_BELOW', None)
        tuning.T.sum_first_below_min_edges = 0      # (S-pl1M sits below the break-even of the sum-first layer below the last one)
        args = bench.make_args('S-pl1M', ['--manual_assign_GPU=0'], se='000', layers=3)
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
        _status_ok()
        out = {'loss': _digest(loss.float().reshape(1))}
        for k, p in t.teacherGNN.named_parameters():
            if p.grad is not None:
                out['grad.' + k] = _digest(p.grad)
        del t, loss
    finally:
        for k in calls:
            setattr(CSRGraph, k, real[k])
        tuning.T.sum_first_below_min_edges = keep_min
        for k, v in keep_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        gc.collect()
        torch.cuda.empty_cache()
    return out, calls


@pytest.mark.parametrize('kind', ['rows_only', 'dense'])
def test_training_step_reproduces_the_digests_of_the_build_before(kind):
    """One rows-only and one dense training step at S-pl1M: the loss and every gradient carry the sha256 recorded with the build before the loads moved
    (same graph, weights and dropout seeds; the step is deterministic), and the step went through the kernels in question."""
    with open(GOLDEN) as f:
        want = json.load(f)[kind]
    got, calls = step_digests(kind)
    assert calls['spmm_gemm_store_rows' if kind == 'rows_only' else 'spmm_gemm'] > 0, calls
    assert set(got) == set(want)
    assert [k for k in got if got[k] != want[k]] == []
