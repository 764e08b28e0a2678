"""The attention kernels of csrc/cb_attn.hip, ops.transformer_conv and the TransformerEncoder on the device against the float64 restatement of
tests/attn_ref.py.  The yardstick of every compared tensor T is the SAME restatement in float32 on the CPU:
    max |T_gpu - T_64|  <=  4 * max |T_cpu32 - T_64|  +  2^-22 * max |T_64|
(both are fp32 evaluations of the same formulas that differ in the order of the sums and in exp; the floor is one rounding of the result itself).
The graph: 300 nodes, about 3 000 directed edges, not symmetric, three nodes without in-edges, two without out-edges, self loops, duplicate edges, one
node of in-degree >= 300 and one of out-degree >= 300.  It is built without hub rows (hub_threshold = 4096: the library's default of 256 would already
cut the two heavy rows) and with hub_threshold = 64, where both heavy rows are hub rows of >= 5 chunks whose last chunk is partial."""
import functools
import math

import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, IN_CH = 300, 40
NO_IN, NO_OUT, HUB_IN, HUB_OUT = (3, 130, 290), (17, 200), 7, 11
PLUMBING = ['--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1']


@functools.lru_cache(maxsize=None)
def _edges():
    ei = ar.make_graph(N, 2300, seed=21, no_in=NO_IN, hub_in=(HUB_IN, 300), hub_out=(HUB_OUT, 297), n_self=12, n_dup=40)
    ei = ei[:, ~torch.isin(ei[0], torch.tensor(NO_OUT))]
    # (the two silenced sources are missing from the heavy row, and the heavy source reaches the 297 nodes that may have in-edges once: a few more of each)
    extra_in = torch.stack([torch.arange(20, 32), torch.full((12,), HUB_IN)])
    extra_out = torch.stack([torch.full((12,), HUB_OUT), torch.arange(40, 52)])
    return torch.cat([ei, extra_in, extra_out], 1).contiguous()


@functools.lru_cache(maxsize=None)
def _graph(which):
    """'whole': no hub rows; 'hub': hub_threshold 64; 'flags': as 'whole' with hot-column flags (a hot set small enough for 300 nodes)."""
    from gnn_tail_generalization_amd import tuning
    from gnn_tail_generalization_amd.graph import CSRGraph
    ei = _edges().to(DEV)
    if which == 'flags':
        keep = tuning.T.hot_bytes
        tuning.T.hot_bytes = 64 << 10      # (read when the graph is built and when a row size is first flagged: both happen here)
        try:
            G = CSRGraph(ei, N, hub_threshold=4096)
            for d in (64, 256):
                for transpose in (False, True):
                    assert G.flagged_cols(transpose, (2 * d + 4) * 4) is not None
            G._hot_count = lambda row_bytes: max(1, min((64 << 10) // max(int(row_bytes), 1), G.n_cols))      # ... and the later look-ups find the same sets
        finally:
            tuning.T.hot_bytes = keep
        return G
    return CSRGraph(ei, N, hub_threshold=4096 if which == 'whole' else 64)


@functools.lru_cache(maxsize=None)
def _case(d, relu=False, x_scale=1.0, zero_query=False):
    """(x, params, dY) float32 on the CPU, the float64 closed form and the float32 one; shared and left unchanged."""
    g = torch.Generator().manual_seed(1000 + d)
    x = torch.randn(N, IN_CH, generator=g) * x_scale
    params = ar.make_params(IN_CH, d, seed=d)
    if zero_query:
        params['lin_query.weight'].zero_()
        params['lin_query.bias'].zero_()
    dY = torch.randn(N, d, generator=g)
    ei = _edges()
    r64 = ar.grads(ei, N, x.double(), ar.cast(params, torch.float64), dY.double(), relu)
    r32 = ar.grads(ei, N, x, params, dY, relu)
    return x, params, dY, r64, r32


def _status_ok():
    from gnn_tail_generalization_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().cb_device_status() == 0


def _check(name, got, r64, r32):
    err, bnd = ar.max_err(got, r64), ar.bound(r64, r32)
    print(f'{name}: max |gpu - f64| = {err:.3e}, bound = {bnd:.3e}, e32 = {ar.max_err(r32, r64):.3e}, err / e32 = {err / max(ar.max_err(r32, r64), 1e-300):.3f}')
    assert err <= bnd, (name, err, bnd)


def _run_layer(G, x, params, dY, relu):
    """{'out', 'x', names...}: ops.transformer_conv forward and backward on the device."""
    from gnn_tail_generalization_amd import ops
    xd = x.to(DEV).requires_grad_(True)
    pd = {k: v.to(DEV).requires_grad_(True) for k, v in params.items()}
    y = ops.transformer_conv(G, xd, *[pd[k] for k in ar.NAMES], relu=relu)
    y.backward(dY.to(DEV))
    res = {'out': y.detach(), 'x': xd.grad}
    res.update({k: v.grad for k, v in pd.items()})
    return res


def _projection(x, params, pad=0):
    """[Q | K | V | S] on the device through the library's GEMM, optionally as a slice of a wider matrix."""
    from gnn_tail_generalization_amd import gemm
    order = ('lin_query', 'lin_key', 'lin_value', 'lin_skip')
    W = torch.cat([params[f'{l}.weight'] for l in order]).to(DEV)
    b = torch.cat([params[f'{l}.bias'] for l in order]).to(DEV)
    P = gemm.mm_nn(x.to(DEV), W.t().contiguous(), bias=b)
    if pad:
        wide = torch.full((P.shape[0], P.shape[1] + 2 * pad), 7.0, device=DEV)
        wide[:, pad:pad + P.shape[1]] = P
        P = wide[:, pad:pad + W.shape[0]]
    d = W.shape[0] // 4
    return [P[:, i * d:(i + 1) * d] for i in range(4)]


def test_the_graph_is_what_the_cases_need():
    ei = _edges()
    indeg, outdeg = torch.bincount(ei[1], minlength=N), torch.bincount(ei[0], minlength=N)
    assert 2800 <= ei.shape[1] <= 3200
    assert all(int(indeg[v]) == 0 for v in NO_IN) and int((indeg == 0).sum()) == 3
    assert all(int(outdeg[v]) == 0 for v in NO_OUT) and int((outdeg == 0).sum()) == 2
    assert int((ei[0] == ei[1]).sum()) >= 4
    pair = ei[0] * N + ei[1]
    assert pair.unique().numel() < pair.numel()                      # duplicate edges
    assert int(indeg[HUB_IN]) >= 300 and int(outdeg[HUB_OUT]) >= 300
    assert int(indeg[HUB_IN]) % 64 and int(outdeg[HUB_OUT]) % 64     # the last chunk is partial
    whole, hub = _graph('whole'), _graph('hub')
    assert not whole.symmetric and whole._plan.n_hubs == 0 and whole._plan_t.n_hubs == 0
    assert hub._plan.n_hubs >= 1 and hub._plan_t.n_hubs >= 1
    for plan, deg, v in ((hub._plan, indeg, HUB_IN), (hub._plan_t, outdeg, HUB_OUT)):
        rows, ptr = plan.hub_rows[:plan.n_hubs].tolist(), plan.hub_chunk_ptr.tolist()
        i = rows.index(v)
        assert ptr[i + 1] - ptr[i] == -(-int(deg[v]) // 64) >= 5


@pytest.mark.parametrize('which', ['whole', 'hub'])
@pytest.mark.parametrize('d,relu', [(64, False), (64, True), (256, True)])
def test_layer_forward_and_backward(which, d, relu):
    """Forward output, lse, dX and all eight parameter gradients; two calls are bit-equal."""
    from gnn_tail_generalization_amd import ops
    G = _graph(which)
    x, params, dY, r64, r32 = _case(d, relu)
    got = _run_layer(G, x, params, dY, relu)
    again = _run_layer(G, x, params, dY, relu)
    _status_ok()
    for k in ('out', 'x') + ar.NAMES:
        assert torch.equal(got[k], again[k]), k
        assert bool(torch.isfinite(got[k]).all()), k
        _check(f'{which} D={d} relu={relu} {k}', got[k], r64[k], r32[k])
    q, k_, v, s = _projection(x, params)
    out, lse = ops.attn_raw(G, q, k_, v, s, relu=relu)
    out2, lse2 = ops.attn_raw(G, q, k_, v, s, relu=relu)
    assert torch.equal(out, got['out']) and torch.equal(out, out2) and torch.equal(lse, lse2)
    assert bool(torch.isinf(lse[list(NO_IN)]).all()) and bool(torch.isfinite(lse).sum() == N - len(NO_IN))
    _check(f'{which} D={d} lse', lse, r64['lse'], r32['lse'])
    assert ops.attn_raw(G, q, k_, v, s, relu=relu, want_lse=False)[1] is None
    _status_ok()


@pytest.mark.parametrize('which', ['whole', 'hub'])
def test_forward_at_width_4(which):
    from gnn_tail_generalization_amd import ops
    x, params, dY, r64, r32 = _case(4)
    q, k, v, s = _projection(x, params)
    out, lse = ops.attn_raw(_graph(which), q, k, v, s)
    _status_ok()
    _check(f'{which} D=4 out', out, r64['out'], r32['out'])
    _check(f'{which} D=4 lse', lse, r64['lse'], r32['lse'])


@pytest.mark.parametrize('which', ['whole', 'hub'])
def test_large_scores(which):
    """A row whose largest score exceeds 100: exp of it without the maximum subtracted is inf in fp32."""
    x, params, dY, r64, r32 = _case(64, True, 6.0)
    ei = _edges()
    Q, K, _, _ = ar.project(x.double(), ar.cast(params, torch.float64))
    s = (Q[ei[1]] * K[ei[0]]).sum(-1) / math.sqrt(64)
    assert float(s.max()) > 100.0 and math.isinf(float(torch.exp(s.max().float())))
    got = _run_layer(_graph(which), x, params, dY, True)
    _status_ok()
    for k in ('out', 'x') + ar.NAMES:
        assert bool(torch.isfinite(got[k]).all()), k
        _check(f'{which} large scores {k}', got[k], r64[k], r32[k])


def test_equal_scores_give_the_neighbour_mean():
    """W_query = 0, b_query = 0: every score is 0, the output is the in-neighbour mean of V plus S."""
    x, params, dY, r64, r32 = _case(64, False, 1.0, True)
    ei = _edges()
    _, _, V, S = ar.project(x.double(), ar.cast(params, torch.float64))
    indeg = torch.bincount(ei[1], minlength=N).double()
    mean = torch.zeros(N, 64, dtype=torch.float64).index_add(0, ei[1], V[ei[0]]) / indeg.clamp(min=1)[:, None]
    assert ar.max_err(r64['out'], mean + S) < 1e-12
    for which in ('whole', 'hub'):
        got = _run_layer(_graph(which), x, params, dY, False)
        _check(f'{which} equal scores out', got['out'], mean + S, r32['out'])
        for k in ('x',) + ar.NAMES:
            _check(f'{which} equal scores {k}', got[k], r64[k], r32[k])
    _status_ok()


@pytest.mark.parametrize('d', [64, 256])
def test_flags_and_padded_rows_do_not_change_a_bit(d):
    """Results with the hot-column flags on and off are bit-equal; operands that are slices of a wider matrix (ld > 4 D) give the bits of contiguous ones."""
    from gnn_tail_generalization_amd import ops
    x, params, dY, r64, r32 = _case(d, True)
    G, F = _graph('whole'), _graph('flags')
    assert ops._attn_view(F, d, False, True).col_flags == 1 and ops._attn_view(F, d, True, True).col_flags == 1
    assert ops._attn_view(F, d, False, False).col_flags == 0 and ops._attn_view(G, d, False, True).col_flags == 0
    q, k, v, s = _projection(x, params)
    dO = dY.to(DEV)

    def run(graph, ops4, use_flags, pad=0):
        out, lse = ops.attn_raw(graph, *ops4, relu=False, use_flags=use_flags)
        wide = torch.full((N, 3 * d + 2 * pad), -3.0, device=DEV)
        dq, dk, dv = [wide[:, pad + i * d:pad + (i + 1) * d] for i in range(3)]
        delta = ops.attn_bwd_raw(graph, ops4[0], ops4[1], ops4[2], dO, lse, dq, dk, dv, use_flags=use_flags)
        if pad:
            assert bool((wide[:, :pad] == -3.0).all()) and bool((wide[:, -pad:] == -3.0).all())
        return out, lse, delta, dq.clone(), dk.clone(), dv.clone()

    base = run(G, (q, k, v, s), True)
    for name, other in (('flags on', run(F, (q, k, v, s), True)), ('flags off', run(F, (q, k, v, s), False)),
                        ('padded', run(G, _projection(x, params, pad=4), True, pad=4))):
        assert all(torch.equal(a, b) for a, b in zip(base, other)), name
    _status_ok()


def test_unsupported_shapes_name_the_constraint():
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.graph import CSRGraph
    G = _graph('whole')
    x = torch.randn(N, 6, device=DEV)
    with pytest.raises(ValueError, match='D % 4 == 0'):
        ops.attn_raw(G, x, x, x, x)
    wide = torch.randn(N, 70, device=DEV)
    with pytest.raises(ValueError, match='16-byte aligned'):
        ops.attn_raw(G, wide[:, 1:65], wide[:, 1:65], wide[:, 1:65], wide[:, 1:65])
    W, b = torch.randn(516, IN_CH, device=DEV), torch.randn(516, device=DEV)
    with pytest.raises(ValueError, match='D <= 512'):
        ops.transformer_conv(G, torch.randn(N, IN_CH, device=DEV), W, b, W, b, W, b, W, b)
    fwd_only = CSRGraph.from_csr(G.rowptr, G.col, N)
    assert fwd_only.rowptr_t is None
    xr = torch.randn(N, IN_CH, device=DEV, requires_grad=True)
    p = {k_: v_.to(DEV) for k_, v_ in ar.make_params(IN_CH, 64, seed=3).items()}
    y = ops.transformer_conv(fwd_only, xr, *[p[k_] for k_ in ar.NAMES])
    with pytest.raises(ValueError, match='reverse'):
        y.sum().backward()
    _status_ok()


def test_encoder_end_to_end():
    """Two layers 40 -> 64 -> 64 in eval mode against the restatement stacked twice with the ReLU between."""
    from gnn_tail_generalization_amd.Link_prediction_model import TransformerEncoder
    torch.manual_seed(5)
    m = TransformerEncoder(IN_CH, 64, 64, 2, 0.5).to(DEV).eval()
    x = _case(64)[0]
    ei = _edges()
    with torch.no_grad():
        got = m(x.to(DEV), _graph('hub'))
        again = m(x.to(DEV), _graph('hub'))
    _status_ok()
    assert torch.equal(got, again)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = {}
    for dt in (torch.float64, torch.float32):
        h = x.to(dt)
        for i in (0, 1):
            h, _ = ar.layer(ei, N, h, {k: sd[f'convs.{i}.{k}'].to(dt) for k in ar.NAMES}, relu=(i == 0))
        ref[dt] = h
    _check('encoder', got, ref[torch.float64], ref[torch.float32])


def _args(extra=()):
    from gnn_tail_generalization_amd.base_options import BaseOptions
    args = BaseOptions().get_arguments(['--dataset=S-tiny', '--predictor=MLP', '--loss_func=log_rank_loss', '--num_neg=3', '--epochs=3'] + PLUMBING + list(extra))
    return args


def test_trainer(tmp_path, monkeypatch):
    import contextlib
    import io
    import os
    import sys

    import numpy as np
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import main as cb_main
    from gnn_tail_generalization_amd.Link_prediction_model import TransformerEncoder
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    runs = []
    for _ in range(2):
        args = _args()
        args.encoder = 'TRANSFORMER'
        args.random_seed = 0
        cb_main.set_seed(args)
        with contextlib.redirect_stdout(io.StringIO()):
            t = trainer(args, 0)
            losses, metrics = t.train_linkpred_encoder()
            again = t.evaluate_linkpred_encoder('test')
        _status_ok()
        assert type(t.encoder) is TransformerEncoder and len(t.encoder.convs) == args.gnn_num_layers
        assert losses.shape == (3,) and np.isfinite(losses).all()
        for res in (metrics, again):
            assert set(res) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and all(0.0 <= float(v) <= 1.0 for v in res.values())
        runs.append(losses)
    print(f'losses {runs[0]}')
    assert np.array_equal(runs[0], runs[1])
    for name in ('CN', 'AA', 'PPR'):
        args = _args()
        args.encoder = name
        args.random_seed = 0
        with contextlib.redirect_stdout(io.StringIO()):
            t = trainer(args, 0)
        with pytest.raises(NotImplementedError, match='heuristic'):
            t.setup_linkpred_encoder()


def test_training_tool(tmp_path, monkeypatch):
    import contextlib
    import io
    import os
    import sys

    import numpy as np
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkpred_encoder
    from gnn_tail_generalization_amd.Link_prediction_model import TransformerEncoder
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkpred_encoder.main(['--dataset=S-tiny', '--encoder=TRANSFORMER', '--epochs=2'] + PLUMBING)
    _status_ok()
    losses, metrics = recs[0]
    assert len(recs) == 1 and losses.shape == (2,) and np.isfinite(losses).all()
    assert set(metrics) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'}
    assert type(train_linkpred_encoder.main.last_trainer.encoder) is TransformerEncoder
    with contextlib.redirect_stdout(io.StringIO()):      # the reference's own choices still go through the package's parser
        recs = train_linkpred_encoder.main(['--dataset=S-tiny', '--encoder=MLP', '--predictor=DOT', '--epochs=2'] + PLUMBING)
    assert len(recs) == 1 and not isinstance(train_linkpred_encoder.main.last_trainer.encoder, TransformerEncoder)
