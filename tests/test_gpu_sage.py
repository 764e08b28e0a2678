"""GPU: the SAGE / WSAGE / GCN encoder layers (ops.sage_layer, csrc/cb_sage.hip) against the float64 restatement of tests/sage_ref.py within its derived
bounds, and the one-kernel layer against the composed path (graph.spmm + cb_gemm_nn_f32 on the materialised [agg | x] + ops.dropout) bit for bit:
forward, backward (dX, dW_n, dW_s, db), the dropout epilogue against the host restatement of Philox, hub rows in both orientations, rows without
in-edges, padded leading dimensions, the encoders end to end, what cb_sage_layer_supported refuses, and the training tool."""
import ctypes
import functools

import pytest
import torch

import coldbrew_oracle as orc
import sage_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NO_IN_165 = (5, 70, 140)      # rows without an in-edge; 140 lies in the partial tile (rows 128 .. 164)
NO_IN_300 = (3, 130, 290)


@functools.lru_cache(maxsize=None)
def _graph(which):
    """(edge_index cpu int64, n, CSRGraph): 'small' = N 165 (two full 64-row tiles and one of 37), 'hub' = N 300 with hub_threshold 16, a row of in-degree
    >= 200 and one of out-degree >= 200."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    if which == 'small':
        n, ei = 165, sr.make_graph(165, 900, seed=11, no_in=NO_IN_165)
        G = CSRGraph(ei.to(DEV), n)
    else:
        n, ei = 300, sr.make_graph(300, 1500, seed=12, no_in=NO_IN_300, hub_in=(7, 200), hub_out=(11, 200))
        G = CSRGraph(ei.to(DEV), n, hub_threshold=16)
    return ei, n, G


@functools.lru_cache(maxsize=None)
def _operands(which, mode, seed=0):
    """float32 cpu (x, W_n, W_s, b, dY), shared and left unchanged."""
    n = _graph(which)[1]
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(n, 256, generator=g)
    W_n, W_s = torch.randn(256, 256, generator=g) / 16, torch.randn(256, 256, generator=g) / 16
    b = torch.randn(256, generator=g) / 4
    dY = torch.randn(n, 256, generator=g)
    return x, W_n, (None if mode == 'GCN' else W_s), b, dY


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _f64(*ts):
    return [None if t is None else t.double() for t in ts]


def _scale(G, mode):
    from gnn_tail_generalization_amd import ops
    return ops.inv_indeg(G) if mode == 'SAGE' else None


def _status_ok():
    from gnn_tail_generalization_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().cb_device_status() == 0


def _check(name, got, ref, bound):
    ok, worst = sr.within(got, ref, bound)
    print(f'{name}: worst |err| / bound = {worst:.4f}')
    assert ok, (name, worst)


def test_graphs_are_what_the_cases_need():
    ei, n, G = _graph('small')
    indeg, outdeg = sr.degrees(ei, n)
    assert n == 165 and all(int(indeg[v]) == 0 for v in NO_IN_165) and int((indeg == 0).sum()) >= 3
    assert not G.symmetric and int((ei[0] == ei[1]).sum()) >= 12
    keys = ei[1] * n + ei[0]
    assert keys.unique().numel() < keys.numel()      # duplicate edges
    assert G._plan.n_hubs == 0 and G._plan_t.n_hubs == 0
    ei, n, G = _graph('hub')
    indeg, outdeg = sr.degrees(ei, n)
    assert int(indeg[7]) >= 200 and int(outdeg[11]) >= 200 and G._plan.n_hubs > 0 and G._plan_t.n_hubs > 0
    assert all(int(indeg[v]) == 0 for v in NO_IN_300)


@pytest.mark.parametrize('mode', sr.MODES)
@pytest.mark.parametrize('which,padded', [('small', False), ('small', True), ('hub', False)])
def test_layer_forward(which, padded, mode):
    """1, 2: the forward of the three modes within the float64 bound, fused == composed bit for bit; exact zeros in agg on rows without in-edges."""
    from gnn_tail_generalization_amd import ops
    ei, n, G = _graph(which)
    x, W_n, W_s, b, _ = _operands(which, mode)
    xd, Wn, Ws, bd = _dev(x, W_n, W_s, b)
    if padded:      # ld_h = ld_out = 260
        xd = torch.zeros((n, 260), device=DEV)[:, :256].copy_(xd)
        outs = [torch.full((n, 260), float('nan'), device=DEV)[:, :256] for _ in range(2)]
        assert xd.stride(0) == 260 and outs[0].stride(0) == 260
    else:
        outs = [None, None]
    s = _scale(G, mode)
    yf, _, pf = ops.sage_layer_raw(G, xd, Wn, Ws, bd, s, fused=True, out=outs[0])
    yc, _, pc = ops.sage_layer_raw(G, xd, Wn, Ws, bd, s, fused=False, out=outs[1])
    _status_ok()
    assert (pf, pc) == ('fused', 'composed')
    assert torch.isfinite(yf).all() and torch.equal(yf, yc)
    ref, _ = sr.layer(ei, n, *_f64(x, W_n, W_s, b), mode)
    _check(f'Y {which} {mode}', yf, ref, sr.bound_forward(ei, n, *_f64(x, W_n, W_s, b), mode))
    # the aggregated rows themselves (backward orientation of the SAME launch form writes them; here: the forward orientation with agg_out)
    _, aggf, _ = ops.sage_layer_raw(G, xd, Wn, Ws, bd, s, fused=True, want_agg=True)
    _, aggc, _ = ops.sage_layer_raw(G, xd, Wn, Ws, bd, s, fused=False, want_agg=True)
    assert torch.equal(aggf, aggc)
    no_in = torch.tensor(NO_IN_165 if which == 'small' else NO_IN_300, device=DEV)
    assert (aggf[no_in] == 0).all() and torch.isfinite(yf[no_in]).all()


@pytest.mark.parametrize('p', [0.0, 0.5])
def test_dropout_epilogue_is_ops_dropout_of_the_relu_output(p):
    """4: fused output == ops.dropout(relu(y), p, seed) of the composed path at row0 = 0, and the kept set is the host Philox mask's."""
    from gnn_tail_generalization_amd import ops
    ei, n, G = _graph('small')
    x, W_n, W_s, b, _ = _operands('small', 'SAGE')
    xd, Wn, Ws, bd = _dev(x, W_n, W_s, b)
    s, seed = _scale(G, 'SAGE'), 2 ** 40 + 12345
    yf, _, pf = ops.sage_layer_raw(G, xd, Wn, Ws, bd, s, relu=True, p=p, seed=seed, fused=True)
    y0, _, _ = ops.sage_layer_raw(G, xd, Wn, Ws, bd, s, relu=True, fused=False)
    want = ops.dropout(y0, p, seed=seed)
    _status_ok()
    assert pf == 'fused' and torch.equal(yf, want)
    if p:
        keep = torch.from_numpy(orc.dropout_keep_mask((n, 256), p, seed)).to(DEV)
        assert torch.equal(yf != 0, keep & (y0 > 0))
        assert torch.equal(yf[keep], (y0 * 2.0)[keep])


def _backward(G, mode, ops, xd, Wn, Ws, bd, dYd, relu, p, seed, fused):
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (xd, Wn, Ws, bd)]
    n0 = len(ops.sage_paths)
    y = ops.sage_layer(G, leaves[0], leaves[1], leaves[2], leaves[3], mode=mode, relu=relu, p=p, seed=seed, fused=fused)
    y.backward(dYd)
    paths = list(ops.sage_paths)[-2:]
    assert len(ops.sage_paths) >= min(n0 + 2, ops.sage_paths.maxlen)
    return y.detach(), [None if t is None else t.grad for t in leaves], paths


@pytest.mark.parametrize('mode', sr.MODES)
@pytest.mark.parametrize('which', ['small', 'hub'])
@pytest.mark.parametrize('last', [False, True])
def test_layer_backward(which, mode, last):
    """3: dX, dW_n, dW_s, db with ReLU + dropout 0.5 and in the last-layer form, against autograd of the float64 restatement fed the mask the device
    drew (read back from Y != 0 and checked against the host Philox mask); fused == composed for all four."""
    from gnn_tail_generalization_amd import ops
    ei, n, G = _graph(which)
    x, W_n, W_s, b, dY = _operands(which, mode)
    xd, Wn, Ws, bd, dYd = _dev(x, W_n, W_s, b, dY)
    relu, p, seed = (False, 0.0, 0) if last else (True, 0.5, 987654321)
    yf, gf, pf = _backward(G, mode, ops, xd, Wn, Ws, bd, dYd, relu, p, seed, True)
    yc, gc, pc = _backward(G, mode, ops, xd, Wn, Ws, bd, dYd, relu, p, seed, False)
    _status_ok()
    assert pf == [('fwd', 'fused'), ('bwd', 'fused')] and pc == [('fwd', 'composed'), ('bwd', 'composed')]
    assert torch.equal(yf, yc)
    for name, a, c in zip(('dX', 'dW_n', 'dW_s', 'db'), gf, gc):
        assert (a is None) == (c is None) and (a is None or torch.equal(a, c)), name
    # the oracle, with the device's mask
    xr, Wnr, Wsr, br = [None if t is None else t.double().requires_grad_(True) for t in (x, W_n, W_s, b)]
    mask = None
    if not last:
        live = (yf != 0).cpu()
        keep = torch.from_numpy(orc.dropout_keep_mask((n, 256), p, seed))
        pre, _ = sr.layer(ei, n, *_f64(x, W_n, W_s, b), mode)
        fb = sr.bound_forward(ei, n, *_f64(x, W_n, W_s, b), mode)
        assert not (live & ~keep).any()                       # nothing the host mask drops survives
        assert live[keep & (pre > fb)].all()                  # everything it keeps and the ReLU clearly passes is there
        assert not live[pre < -fb].any()
        mask = live.double() / (1.0 - p)
    yr, _ = sr.layer(ei, n, xr, Wnr, Wsr, br, mode, relu=relu, mask=mask)
    _check(f'Y {which} {mode}', yf, yr.detach(), sr.bound_forward(ei, n, *_f64(x, W_n, W_s, b), mode, factor=1.0 / (1.0 - p)))
    yr.backward(dY.double())
    Gm = dY.double() * (mask if mask is not None else 1.0)      # G of the operator's docstring, in float64
    _check('dX', gf[0], xr.grad, sr.bound_dx(ei, n, Gm, *_f64(W_n, W_s), mode))
    bn, bs = sr.bound_dw(ei, n, Gm, x.double(), mode)
    _check('dW_n', gf[1], Wnr.grad, bn)
    if W_s is not None:
        _check('dW_s', gf[2], Wsr.grad, bs)
    _check('db', gf[3], br.grad, sr.bound_db(n, Gm))


@pytest.mark.parametrize('in_ch,p', [(256, 0.5), (32, 0.0)])
def test_encoder_end_to_end(in_ch, p, monkeypatch):
    """5: two-layer SAGEEncoder, fused == composed in the forward and in every parameter gradient; the path each layer took; the forward within the bound
    of the oracle layer by layer (each oracle layer is fed the device's previous activation, so bounds do not compound)."""
    from gnn_tail_generalization_amd import ops, tuning
    from gnn_tail_generalization_amd.Link_prediction_model import SAGEEncoder
    ei, n, G = _graph('small')
    torch.manual_seed(3)
    enc = SAGEEncoder(in_ch, 256, 256, 2, p).to(DEV)
    enc.train()
    x = torch.randn(n, in_ch, generator=torch.Generator().manual_seed(5)).to(DEV)
    dY = torch.randn(n, 256, generator=torch.Generator().manual_seed(6)).to(DEV)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(tuning.T, 'sage_fused', fused)
        enc.zero_grad()
        xin = x.clone().requires_grad_(True)
        ops._seed_override[:] = [424242]
        ops.sage_paths.clear()
        acts = []
        h = enc.convs[0](xin, G, relu=True, p=p)
        acts.append(h.detach())
        y = enc.convs[1](h, G)
        ops._seed_override[:] = []
        y.backward(dY)
        res[fused] = (y.detach(), xin.grad, {k: v.grad.clone() for k, v in enc.named_parameters()}, list(ops.sage_paths), acts)
    _status_ok()
    first = 'fused' if in_ch == 256 else 'composed'
    assert res[True][3] == [('fwd', first), ('fwd', 'fused'), ('bwd', 'fused'), ('bwd', first)]
    assert res[False][3] == [('fwd', 'composed'), ('fwd', 'composed'), ('bwd', 'composed'), ('bwd', 'composed')]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert set(res[True][2]) == {f'convs.{i}.{w}' for i in (0, 1) for w in ('lin_l.weight', 'lin_l.bias', 'lin_r.weight')}
    for k in res[True][2]:
        assert torch.equal(res[True][2][k], res[False][2][k]), k
    # enc(x, G) is the same two calls
    monkeypatch.setattr(tuning.T, 'sage_fused', True)
    ops._seed_override[:] = [424242]
    assert torch.equal(enc(x, G).detach(), res[True][0])
    ops._seed_override[:] = []
    # layer by layer against the oracle
    sd = {k: v.detach().cpu().double() for k, v in enc.state_dict().items()}
    h0 = res[True][4][0]
    mask = None
    if p:
        keep = torch.from_numpy(orc.dropout_keep_mask((n, 256), p, 424242))
        assert not ((h0 != 0).cpu() & ~keep).any()
        mask = (h0 != 0).cpu().double() / (1.0 - p)
    args0 = (x.cpu().double(), sd['convs.0.lin_l.weight'], sd['convs.0.lin_r.weight'], sd['convs.0.lin_l.bias'])
    r0, _ = sr.layer(ei, n, *args0, 'SAGE', relu=True, mask=mask)
    _check('layer 0', h0, r0, sr.bound_forward(ei, n, *args0, 'SAGE', factor=1.0 / (1.0 - p)))
    args1 = (h0.cpu().double(), sd['convs.1.lin_l.weight'], sd['convs.1.lin_r.weight'], sd['convs.1.lin_l.bias'])
    r1, _ = sr.layer(ei, n, *args1, 'SAGE')
    _check('layer 1', res[True][0], r1, sr.bound_forward(ei, n, *args1, 'SAGE'))


def test_what_the_kernel_does_not_cover_is_refused_and_composed():
    """7: cb_sage_layer_supported is 0 for width 128, a misaligned pointer and bf16 rows; the direct call returns CB_E_INVALID; the operator composes."""
    from gnn_tail_generalization_amd import _lib, ops
    lib = _lib.load()
    ei, n, G = _graph('small')
    x, W_n, W_s, b, _ = _operands('small', 'SAGE')
    xd, Wn, Ws, bd = _dev(x, W_n, W_s, b)
    out = torch.empty((n, 256), device=DEV)
    P = _lib.ptr

    def sup(d_in, d_out, bf16, h, ld):
        return lib.cb_sage_layer_supported(d_in, d_out, bf16, h, ld, h, ld, None, 0, P(out), 256)
    assert sup(256, 256, 0, P(xd), 256) == 1
    assert sup(128, 256, 0, P(xd), 128) == 0 and sup(256, 128, 0, P(xd), 256) == 0
    assert sup(256, 256, 1, P(xd), 256) == 0
    mis = torch.empty(n * 256 + 1, device=DEV)[1:].view(n, 256)      # 4 bytes off a 16-byte boundary
    mis.copy_(xd)
    assert mis.data_ptr() % 16 == 4 and sup(256, 256, 0, P(mis), 256) == 0
    assert sup(256, 256, 0, P(xd), 258) == 0                          # ld not a multiple of 4
    img = ops._sage_image(Wn, Ws, True)
    view = G._view(256, False, use_flags=True)
    rc = lib.cb_sage_layer_f32(ctypes.byref(view), P(mis), 256, P(mis), 256, None, P(ops.inv_indeg(G)), P(img), P(bd), 0, 0.0, ctypes.c_uint64(0), None, 0, None, 0, 0,
                               P(out), 256, _lib.stream_ptr())
    assert rc == -1 and b'cb_sage_layer_supported' in lib.cb_last_error()      # CB_E_INVALID (include/coldbrew_hip.h)
    # the operator on the misaligned rows and on width 128: the composed result
    ym, _, pm = ops.sage_layer_raw(G, mis, Wn, Ws, bd, ops.inv_indeg(G), fused=True)
    ya, _, _ = ops.sage_layer_raw(G, xd, Wn, Ws, bd, ops.inv_indeg(G), fused=False)
    assert pm == 'composed' and torch.equal(ym, ya)
    x128, W128 = xd[:, :128].contiguous(), Wn[:, :128].contiguous()
    y128, _, p128 = ops.sage_layer_raw(G, x128, W128, W128, bd, ops.inv_indeg(G), fused=True)
    assert p128 == 'composed'
    ref, _ = sr.layer(ei, n, x[:, :128].double(), W_n[:, :128].double(), W_n[:, :128].double(), b.double(), 'SAGE')
    _check('width 128', y128, ref, sr.bound_forward(ei, n, x[:, :128].double(), W_n[:, :128].double(), W_n[:, :128].double(), b.double(), 'SAGE'))
    _status_ok()


PLUMBING = ['--use_special_split=0', '--want_headtail=0', '--manual_assign_GPU=0', '--do_deg_analyze=0', '--N_exp=1']


@pytest.mark.parametrize('encoder,predictor', [('SAGE', 'MLP'), ('MLP', 'DOT')])
def test_training_tool(encoder, predictor, tmp_path, monkeypatch):
    """6: twenty steps of tools/train_linkpred_encoder on S-tiny: finite losses that go down, the four metrics in [0, 1], an embedding that moved."""
    import contextlib
    import io
    import os
    import sys

    import numpy as np
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkpred_encoder
    from gnn_tail_generalization_amd import ops
    from gnn_tail_generalization_amd.trainer_node_classification import trainer
    first = {}
    setup = trainer.setup_linkpred_encoder

    def recording_setup(self):
        setup(self)
        first['emb'] = self.emb.weight.detach().clone()
    monkeypatch.setattr(trainer, 'setup_linkpred_encoder', recording_setup)
    ops.sage_paths.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkpred_encoder.main(['--dataset=S-tiny', f'--encoder={encoder}', f'--predictor={predictor}', '--loss_func=log_rank_loss', '--num_neg=3',
                                            '--epochs=20'] + PLUMBING)
    _status_ok()
    assert len(recs) == 1
    losses, metrics = recs[0]
    print(f'{encoder} / {predictor}: losses {losses[:5]} ... {losses[-5:]}; {metrics}')
    assert losses.shape == (20,) and np.isfinite(losses).all()
    assert losses[-5:].mean() < losses[:5].mean()
    assert set(metrics) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and all(0.0 <= float(v) <= 1.0 for v in metrics.values())
    t = train_linkpred_encoder.main.last_trainer
    assert tuple(t.emb.weight.shape) == tuple(first['emb'].shape) and not torch.equal(t.emb.weight.detach(), first['emb'])
    assert (len(ops.sage_paths) > 0) == (encoder == 'SAGE')      # the SAGE run went through ops.sage_layer, the MLP run did not


def test_the_teacher_tool_is_unchanged(tmp_path, monkeypatch):
    """6, last item: tools/train_linkpred on the same arguments still runs and returns the same shapes and keys."""
    import contextlib
    import io
    import os
    import sys

    import numpy as np
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_linkpred
    with contextlib.redirect_stdout(io.StringIO()):
        recs = train_linkpred.main(['--dataset=S-tiny', '--encoder=SAGE', '--predictor=MLP', '--loss_func=log_rank_loss', '--num_neg=3', '--epochs=20'] + PLUMBING)
    losses, metrics = recs[0]
    assert len(recs) == 1 and losses.shape == (20,) and np.isfinite(losses).all()
    assert set(metrics) == {'Hits@20', 'Hits@50', 'Hits@100', 'AUC'} and all(0.0 <= float(v) <= 1.0 for v in metrics.values())
