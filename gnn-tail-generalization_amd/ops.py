"""Autograd-visible operators of the TeacherGNN hot path, each backed by the C ABI
(include/coldbrew_hip.h).  One torch.autograd.Function per fused stage; tensors must live
on the MI355X (no CPU fallback — _lib.require_device raises otherwise).

Stage map (reference lines are GNN_model/GCN.py unless noted):
  dropout     Xd = X * keep / (1-p)                  :104,:110,:133  (counter-based RNG, mask never stored)
  transform   Z  = (Xd * a) @ W + E ; ||E||_F        :213,:225,:230-232  (dense, MFMA-bound)
  aggregate   Y  = act(b * (A^T Z) + bias)           :238,:250,:253(+:128)  (sparse, HBM-bound)
  res_mix     X' = (1-alpha) * Y + alpha * R         res_tricks.py:14,23
  nll_logsoftmax  mean nll(log_softmax(out[mask]))   trainer_node_classification.py:390-391
Student MLPs (reference lines are MLP_model/__init__.py / utils.py / the trainer):
  ln_gelu_dropout   dropout(gelu(layer_norm(z)))     utils.py:898-903 (one row kernel per getMLP group; linear_ln_gelu_dropout: + its Linear)
  mse_rows          mse(pred, target[row_index])     trainer_node_classification.py:96,108
  semlp_part2_input [x | a1 * replaced | a0 * guess] MLP_model/__init__.py:102-108
GraphMLP (MLP_model/__init__.py:158-208):
  neighbor_contrastive_loss  -mean log(num / den) over the cropped adjacency power   :190-198 (Gram sweep, no [B, B] matrix in the forward)
  cosine_sim        (x @ x.T) / (|x_i| |x_j|)        :200-208
  spgemm_csr / csr_transpose / SparsePower.from_adjacency   the adjacency power A~^r on the device (utils.py:1242-1248; expand - sort - compress)
The teacher's edge-wise term (trainer_node_classification.py:417-438, 507-563; utils.py:754-791):
  LinkSampler       positive / negative edge samples on the device CSR (binary search in a row; counter-based draws)
  linkp_loss_eva    BCE-with-logits of the DistMult scores + MRR over index pairs; gradient as one [N, D] matrix, no atomics
  cal_MRR           the MRR of held scores
Link-prediction baselines and tie-safe metrics (Link_prediction_baseline/heuristics.py:51-62, 107-129; Link_prediction_model/utils.py:43-59):
  pair_scores       CN / AA of index pairs by sorted-row intersection on the by-src CSR (CN exact, AA in float64 rounded once)
  rank_counts       per positive, the negatives above it and equal to it; hits_at_k / auc derive from the two integers
Link predictors and ranking losses (Link_prediction_model/layer.py:85-106, 182-191; loss.py:4-30; model.py:152-158):
  pair_dot          <h[u], h[v]> per index pair (DotPredictor); gradient through the sorted inverted index, no atomics
  pair_linear       act((h[u] * h[v]) @ W^T + b) (+ dropout): MLPPredictor's first layer, its A operand formed while the GEMM stages it
  rank_loss         auc / adaptive_auc / log_rank / ce / info_nce over pos [P] and neg [P, k], every term in float64, rounded once
  rows_linear       act(h[idx] @ W^T + b) or act([h[idx0] | h[idx1]] @ W^T + b) (+ dropout): the first layer of the MLP-dot / MLP-bilinear /
                    concatenating predictors (layer.py:108-180), the gathered operand formed while the GEMM stages it
  pair_bilinear     sum(bilin(h[u]) * h[v], -1) (BilinearPredictor, layer.py:193-203): the dot taken in the GEMM's epilogue, no [S, D] matrix
  pair_scatter_rows the backward of the two gathers: rows as they stand through the sorted inverted index, no atomics
Encoders of the link-prediction experiment (Link_prediction_model/layer.py:19-75; model.py:290-304):
  sage_layer        act((s * (A X)) W_n^T + X W_s^T + b): one SAGEConv / GraphConv / GCNConv(normalize=False) layer with the ReLU and dropout after it; one
                    kernel per direction at 256 -> 256 (aggregation into an on-chip tile, the GEMM from there), the composed kernels elsewhere
The link-prediction experiment's protocol (Link_prediction_model/negative_sample.py:5-57; model.py:121-266; utils.py:568-586):
  NegativeSampler   global / local / permuted-global negatives on the device CSR (a binary search in the destination's row, counter-based tries)
  seeded_permutation  a permutation that is a pure function of (n, seed): the epoch shuffle and the permuted copies
  row_rank_counts   per positive, the entries of ITS row of negatives above it and equal to it; mrr_from_counts: the OGB rule on those counts
  recall_at_topk    `cal_recall` exactly: the positives among the top k of [positives above 0 | negatives], positives first among equals
"""
import collections
import ctypes
import functools
import operator
import os

import torch

from . import _lib


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------
_seed_override = []
_graph_seed = None      # hipGraph mode: int64 device tensor [1]; kernels add its value to the per-site host seed


_graph_site = 0         # hipGraph mode: running number of the dropout site whose host seed is being fixed


def next_seed():
    """63-bit seed drawn from torch's CPU generator: follows torch.manual_seed, costs no device sync.  In hipGraph mode the per-site
    host seeds are baked into the captured kernels and all variation comes from the device seed word, so they are taken from a fixed
    sequence instead: a resumed run then captures the very same graphs as the run that wrote the checkpoint."""
    global _graph_site
    if _seed_override:
        return _seed_override.pop(0)
    if _graph_seed is not None:
        _graph_site += 1
        return (0x9E3779B97F4A7C15 * _graph_site) % (2 ** 62)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def set_graph_seed(t):
    """Install (or clear with None) the device-resident per-step seed word used while a training step is
    captured / replayed as a hipGraph: the captured kernels keep their per-site host seeds and add *t."""
    global _graph_seed, _graph_site
    _graph_seed = t
    _graph_site = 0


def seed_dev_ptr():
    return _lib.ptr(_graph_seed) if _graph_seed is not None else None


def store_args(mix, mix_index, c_act, c_mix, p, seed, row0, bits, relu_only, act):
    """The trunk's store as the one argument the entries take (cb_trunk_store, include/coldbrew_hip.h): mix (+ mix_index: its row per stored row, where
    it is a compact matrix), the mix factors, the dropout (p, seed, the graph-replay seed word, row0 = global index of node row 0), the mask words `bits`
    (relu_only: ReLU mask alone) and the activation output `act`; tensors may be None.  The struct holds on to the tensors, so they live as long as it."""
    st = _lib.TrunkStore(mix.data_ptr() if mix is not None else None, mix.stride(0) if mix is not None else 0,
                         mix_index.data_ptr() if mix_index is not None else None, float(c_act), float(c_mix), float(p), int(seed),
                         _graph_seed.data_ptr() if _graph_seed is not None else None, int(row0), bits.data_ptr() if bits is not None else None,
                         int(bool(relu_only)), act.data_ptr() if act is not None else None, act.stride(0) if act is not None else 0)
    st._keep = (mix, mix_index, bits, act, _graph_seed)
    return st


def _dropout_raw(x, p, seed, offset=0):
    lib = _lib.load()
    x = _c(x)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.cb_dropout_f32(_lib.ptr(x), _lib.ptr(out), x.numel(), float(p), ctypes.c_uint64(seed), seed_dev_ptr(),
                                      int(offset), _lib.stream_ptr()), 'cb_dropout_f32')
    return out


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        ctx.p, ctx.seed, ctx.offset = p, seed, offset
        return _dropout_raw(x, p, seed, offset)

    @staticmethod
    def backward(ctx, g):
        return _dropout_raw(g, ctx.p, ctx.seed, ctx.offset), None, None, None


def dropout(x, p, training=True, seed=None, offset=0):
    """F.dropout semantics; the keep-mask is a pure function of (seed, flat element index)."""
    if not training or p == 0.0:
        return x
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise TypeError('dropout expects float32')
    if p >= 1.0:
        return x * 0
    if seed is None:
        seed = next_seed()
    return _DropoutFn.apply(x, float(p), int(seed), int(offset))


def dropout_keep_mask(shape, p, seed, device, offset=0):
    """The boolean keep-mask `dropout` uses for (seed, shape) — for parity tests that inject the same
    mask into the oracle.  The mask is pinned bit for bit to the host restatement of Philox4x32-10
    (oracle/coldbrew_oracle.py dropout_keep_mask) over offsets up to 2^40, seeds up to 2^62 and the device seed word
    (tests/test_philox_host.py, tests/test_gpu_philox.py)."""
    ones = torch.ones(shape, dtype=torch.float32, device=device)
    return _dropout_raw(ones, p, seed, offset) > 0


# ---------------------------------------------------------------------------------------------
# aggregation
# ---------------------------------------------------------------------------------------------
def act_bwd(g, act=None, row_scale=None, want_out=True, want_colsum=False):
    """gm = g * (act > 0); returns (gm * row_scale[:,None] or None, colsum(gm) or None) in one pass."""
    lib = _lib.load()
    g = _c(g)
    rows, d = g.shape
    if act is not None:
        act = _c(act)
    out = torch.empty_like(g) if want_out else None
    colsum = torch.empty(d, dtype=torch.float32, device=g.device) if want_colsum else None
    wsb = lib.cb_colsum_workspace_bytes(rows, d) if want_colsum else 0
    ws = _ws(wsb, g.device) if want_colsum else None
    with torch.cuda.device(g.device):
        _lib.check(lib.cb_act_bwd_f32(_lib.ptr(g), _lib.ptr(act), _lib.ptr(row_scale), _lib.ptr(out), rows, d,
                                      _lib.ptr(colsum), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_act_bwd_f32')
    return out, colsum


class _AggregateFn(torch.autograd.Function):
    """Forward: by-dst CSR SpMM with fused `* norm_in`, `+ bias`, optional ReLU.
    Backward (autograd of DGL's gspmm = SpMM on the reverse graph):
        dY' = dY * (Y > 0) if relu;  dbias = colsum(dY');  dZ = A (b * dY').
    grad_rows (bool mask over the rows, or None): the loss_rows promise below for the gradient this node receives.  The backward then works on
    the rows of the mask only: it checks the claim on the device (check_rows_zero), takes dY' and dbias on the compact rows and gathers over
    the edges that leave them (CSRGraph.grad_support_plan with one level: rows S_0 -> all rows) — level 0 of the fused trunk's row-sparse
    backward for the one-operator-per-stage path."""

    @staticmethod
    def forward(ctx, graph, h, row_scale, bias, relu, grad_rows=None):
        out = graph.spmm(h, transpose=False, row_scale=row_scale, bias=bias, relu=relu)
        ctx.graph, ctx.relu, ctx.grad_rows = graph, relu, grad_rows
        ctx.has_bias = bias is not None
        ctx.save_for_backward(out if relu else None, row_scale)
        return out

    @staticmethod
    def backward(ctx, g):
        out, row_scale = ctx.saved_tensors
        need_h, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[3]
        if ctx.grad_rows is not None and need_h:
            check_rows_zero(g, ctx.grad_rows)
            plan = ctx.graph.grad_support_plan(ctx.grad_rows, 1, max_frac=0.0)
            idx = plan.space0.idx
            gc = gather_rows_by_index(g, idx)
            if ctx.relu or row_scale is not None or need_b:
                rs = None
                if row_scale is not None:
                    rs = getattr(plan, '_row_scale0', None)
                    if rs is None or rs[0] is not row_scale:
                        rs = plan._row_scale0 = (row_scale, row_scale[idx].contiguous())
                    rs = rs[1]
                gc, dbias = act_bwd(gc, gather_rows_by_index(out, idx) if ctx.relu else None, rs, want_out=True, want_colsum=need_b)
            else:
                dbias = None
            return None, plan.levels[0][0].spmm(gc, transpose=False), None, dbias, None, None
        if not (ctx.relu or row_scale is not None or need_b):
            gs, dbias = _c(g), None
        else:
            gs, dbias = act_bwd(g, out if ctx.relu else None, row_scale, want_out=need_h, want_colsum=need_b)
        dh = ctx.graph.spmm(gs, transpose=True) if need_h else None
        return None, dh, None, dbias, None, None


class _WeightedAggregateFn(torch.autograd.Function):
    """The `edge_weight` form of the aggregation (GCN.py:199-202, fn.u_mul_e + fn.sum): Y = act(b * (sum_e w_e h[src_e]) + bias).
    edge_weight is indexed like the columns of edge_index (as graph.edata in DGL).  Backward: dh = sum over the reverse CSR with the
    same weights; dw_e = <h[src_e], b[dst_e] * dY'[dst_e]>."""

    @staticmethod
    def forward(ctx, graph, h, edge_weight, row_scale, bias, relu):
        w = edge_weight.detach().to(torch.float32)
        out = graph.spmm_weighted(h, w[graph.edge_perm(False)], False, row_scale=row_scale, bias=bias, relu=relu)
        ctx.graph, ctx.relu, ctx.has_bias = graph, relu, bias is not None
        ctx.save_for_backward(h, w, out if relu else None, row_scale)
        return out

    @staticmethod
    def backward(ctx, g):
        h, w, out, row_scale = ctx.saved_tensors
        graph = ctx.graph
        need_h, need_w, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[4]
        if ctx.relu or row_scale is not None or need_b:
            gs, dbias = act_bwd(g, out if ctx.relu else None, row_scale, want_out=True, want_colsum=need_b)
        else:
            gs, dbias = _c(g), None
        dh = graph.spmm_weighted(gs, w[graph.edge_perm(True)], True) if need_h else None
        dw = None
        if need_w:
            dw = torch.empty_like(w)
            dw[graph.edge_perm(False)] = graph.edge_dot(h, gs, False)
        return None, dh, dw, None, dbias, None


def aggregate(graph, h, row_scale=None, bias=None, relu=False, edge_weight=None, grad_rows=None):
    """grad_rows: see _AggregateFn (ignored by the weighted and the node-sharded forms: their backward is dense)."""
    _lib.require_device(h)
    if edge_weight is not None:
        if hasattr(graph, 'part'):
            raise NotImplementedError('edge_weight on a node-sharded graph (never passed by TricksComb, GCN.py:115)')
        return _WeightedAggregateFn.apply(graph, h, edge_weight, row_scale, bias, bool(relu))
    if hasattr(graph, 'part'):      # node-sharded graph: all-gather exchange + local rows (dist.py)
        from .dist import sharded_aggregate
        return sharded_aggregate(graph, h, row_scale, bias, relu)
    return _AggregateFn.apply(graph, h, row_scale, bias, bool(relu), grad_rows)


# ---------------------------------------------------------------------------------------------
# structural-embedding regulariser
# ---------------------------------------------------------------------------------------------
class _FrobeniusFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, known):
        if known is not None:      # left by the fused Adam when it wrote x (optim.Adam.step): no pass over the table
            norm = known[0].clone()
        else:
            lib = _lib.load()
            xc = _c(x)
            out2 = torch.empty(2, dtype=torch.float32, device=x.device)
            wsb = lib.cb_reduce_workspace_bytes()
            ws = _ws(wsb, x.device)
            with torch.cuda.device(x.device):
                _lib.check(lib.cb_frobenius_norm_f32(_lib.ptr(xc), xc.numel(), _lib.ptr(out2), _lib.ptr(ws), wsb,
                                                     _lib.stream_ptr()), 'cb_frobenius_norm_f32')
            norm = out2[0]
        ctx.save_for_backward(x, norm)
        return norm.clone()

    @staticmethod
    def backward(ctx, g):
        x, norm = ctx.saved_tensors
        # d||x||/dx = x / ||x||; 0 at x = 0 (the subgradient torch.norm's backward picks), not NaN
        return x * torch.where(norm > 0, g / norm, torch.zeros_like(norm)), None


# Norms the fused Adam left behind: parameter._cb_norm = (parameter._version at that time, [2] device tensor {||p||_F, ||p||_F^2}).  The Adam kernel
# computes the sum of squares of the values it writes (cb_adam_multi_norm_f32) for every parameter whose norm a forward has asked for
# (`_cb_want_norm`), so the next forward's th.norm(le) (GCN.py:232) reads two floats instead of the table.  An entry is trusted only while
# the parameter's version counter is the one recorded — every torch in-place write (load_state_dict, copy_, another optimiser) bumps it —,
# never during a hipGraph capture, and never for a parameter a captured graph updates behind Python's back (`_cb_norm_off`).
# (A write through `p.data` has a version counter of its own and is not seen: code that edits a table that way calls forget_norms.)
ADAM_NORMS = True


def forget_norms(module_or_params):
    """Drops the norms the fused Adam left for these parameters (after writing them through a path that does not bump their version)."""
    params = module_or_params.parameters() if hasattr(module_or_params, 'parameters') else module_or_params
    for p in params:
        p._cb_norm = None


def known_norm(x):
    if not ADAM_NORMS or getattr(x, '_cb_norm_off', False) or torch.cuda.is_current_stream_capturing():
        return None
    hit = getattr(x, '_cb_norm', None)
    return hit[1] if hit is not None and hit[0] == x._version else None


def frobenius_norm(x):
    _lib.require_device(x)
    known = None
    if isinstance(x, torch.nn.Parameter) and x.is_leaf:
        x._cb_want_norm = True
        known = known_norm(x)
    return _FrobeniusFn.apply(x, known)


def fold_se_reg(model, optimizer, coef, se_reg_all):
    """The regulariser term `coef * sum_l ||le_l||_F` of the training loss (trainer_node_classification.py:393) WITHOUT its autograd
    path: returns the detached value to add to the loss and hands `coef / ||le_l||` to the fused Adam (optim.Adam.extra_decay_buffer),
    whose kernel then adds `coef * le / ||le||` — the term's gradient — to the data gradient it reads anyway (a non-finite
    coefficient, i.e. an all-zero table, counts as 0: the subgradient torch.norm's backward picks).  Mathematically the update of
    `loss.backward()` through `th.norm` (GCN.py:232); what is saved per table and step is the `le / ||le||` tensor (8 B/element)
    and autograd's accumulation of it into le.grad (12 B/element).  One extra launch per table.  None if the model has no SE layer
    or the optimiser is not the fused Adam (the caller then keeps the autograd path).  CB_SE_REG_FOLD=0 switches it off."""
    import os
    from . import optim
    if not isinstance(optimizer, optim.Adam):
        return None
    convs = [m for m in model.modules() if getattr(m, 'whetherHasSE', False) and getattr(m, 'se_norm', None) is not None]
    if (os.environ.get('CB_SE_REG_FOLD', '1') == '0' or not convs
            or any(c.le.grad_fn is not None or not c.le.requires_grad for c in convs)):
        # the caller keeps the autograd path for this step: coefficients left over from an earlier folded step must not act again
        for buf in optimizer._extra_decay.values():
            buf.zero_()
        return None
    for conv in convs:
        buf = optimizer.extra_decay_buffer(conv.le)
        c0 = getattr(conv, '_se_coef', None)
        if c0 is None or float(conv._se_coef_val) != float(coef) or c0.device != buf.device:
            c0 = conv._se_coef = torch.tensor(float(coef), dtype=torch.float32, device=buf.device)
            conv._se_coef_val = float(coef)
        torch.div(c0, conv.se_norm, out=buf.view(()))
    return coef * se_reg_all.detach()


def transform(feat, norm_out, weight, le=None, graph=None):
    """Z = (feat * a[:,None]) @ W (+ le) and se_reg = ||le||_F (GCN.py:213,225,230-236).  With a
    node-sharded graph `le` holds the local rows and the norm is taken over all ranks."""
    _lib.require_device(feat, weight)
    from . import gemm
    z = gemm.linear_rowscale(feat, weight, norm_out, le)
    if le is None:
        return z, None
    reg = frobenius_norm(le)
    if graph is not None and hasattr(graph, 'part'):
        from .dist import allreduce_sum
        reg = allreduce_sum(reg * reg, graph.group).sqrt()
    return z, reg


# ---------------------------------------------------------------------------------------------
# residual mixes
# ---------------------------------------------------------------------------------------------
def _axpby_raw(a, x, b, y):
    lib = _lib.load()
    x, y = _c(x), _c(y)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.cb_axpby_f32(float(a), _lib.ptr(x), float(b), _lib.ptr(y), _lib.ptr(out), x.numel(),
                                    _lib.stream_ptr()), 'cb_axpby_f32')
    return out


class _AxpbyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, x, b, y):
        ctx.a, ctx.b = a, b
        return _axpby_raw(a, x, b, y)

    @staticmethod
    def backward(ctx, g):
        gx = _axpby_raw(ctx.a, g, 0.0, g) if ctx.needs_input_grad[1] else None
        gy = _axpby_raw(ctx.b, g, 0.0, g) if ctx.needs_input_grad[3] else None
        return None, gx, None, gy


def axpby(a, x, b, y):
    """a*x + b*y for same-shape float32 device tensors."""
    _lib.require_device(x, y)
    if x.shape != y.shape or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError('axpby expects same-shape float32 tensors')
    return _AxpbyFn.apply(float(a), x, float(b), y)


# ---------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------
# Row-sparse backward: the masked loss's gradient w.r.t. the logits is zero outside the loss rows, and so is everything row-wise stages
# make of it.  The caller that builds such an objective SAYS so: `loss_rows=(mask, count)` handed to the forward (TeacherGNN.get_3_embs ->
# TricksComb.forward -> trunk) is the promise that the logits of that forward receive gradient in the rows of `mask` only; the trunk's
# backward then may skip the other rows — after check_rows_zero() has put the claim under the device's own eyes: a violation ends in the
# device error word AND in the guard word that keeps the optimiser launch of that step from writing (_lib.grad_guard), never in silent wrong
# gradients or updated weights.  CB_LOSS_ROWS=0 makes every backward dense.
def loss_rows_enabled():
    return os.environ.get('CB_LOSS_ROWS', '1') != '0'


def check_rows_zero(g, mask):
    """Device-side check that every row of g outside `mask` is exactly zero (cb_rows_zero_outside_mask_f32).  A violation is recorded in
    the device error word (the trainers raise where they read the loss) and in the device's guard word: the fused Adam launch that follows
    on the stream then leaves parameters and moments untouched (_lib.grad_guard)."""
    lib = _lib.load()
    _lib.require_device(g, mask)
    if g.stride(1) != 1:
        g = g.contiguous()
    m8 = mask.view(torch.uint8)
    with torch.cuda.device(g.device):
        _lib.check(lib.cb_rows_zero_outside_mask_f32(_lib.ptr(g), g.stride(0) if g.shape[0] > 1 else g.shape[1], g.shape[0], g.shape[1], _lib.ptr(m8),
                                                     _lib.ptr(_lib.grad_guard(g.device)), _lib.stream_ptr()), 'cb_rows_zero_outside_mask_f32')


class _NllFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, y, mask, count, unit_grad=False):
        ctx.unit_grad = bool(unit_grad)
        lib = _lib.load()
        z = logits if logits.stride(1) == 1 else logits.contiguous()
        rows, C = z.shape
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        grad = torch.empty((rows, C), dtype=torch.float32, device=z.device) if ctx.needs_input_grad[0] else None
        wsb = lib.cb_reduce_workspace_bytes()
        ws = _ws(wsb, z.device)
        m8 = mask.view(torch.uint8) if mask is not None else None
        with torch.cuda.device(z.device):
            _lib.check(lib.cb_nll_logsoftmax_f32(_lib.ptr(z), z.stride(0), _lib.ptr(y), _lib.ptr(m8), rows, C, int(count),
                                                 _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                       'cb_nll_logsoftmax_f32')
        ctx.save_for_backward(grad)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        # unit_grad: the caller promised that this loss enters its objective with coefficient 1 and that backward() is seeded
        # with 1 (the trainers' own step): the [N, C] pass that would multiply by that 1 is skipped
        # (rows outside the mask are exactly zero: what a forward called with loss_rows=(mask, count) relies on)
        return (grad if ctx.unit_grad else grad * g), None, None, None, None


def nll_logsoftmax(logits, y, mask=None, count=None, unit_grad=False):
    """mean_{r: mask[r]} nll(log_softmax(logits[r]), y[r]) without materialising logits[mask].
    `count` = number of masked rows (precomputed once per dataset to avoid a per-step host sync).
    unit_grad=True: promise that the upstream gradient of this loss is exactly 1 (loss used with coefficient 1, backward() called on
    the objective without a seed) — the backward then hands the stored gradient on without a pass over [N, C]."""
    _lib.require_device(logits, y, mask)
    if logits.dtype != torch.float32 or y.dtype != torch.int64:
        raise TypeError('nll_logsoftmax expects float32 logits and int64 labels')
    if mask is not None and mask.dtype != torch.bool:
        raise TypeError('mask must be a bool tensor')
    if count is None:
        count = int(mask.sum().item()) if mask is not None else logits.shape[0]
    return _NllFn.apply(logits, _c(y), _c(mask) if mask is not None else None, count, bool(unit_grad))


def gather_rows_by_index(x, idx, out_bf16=False):
    """x[idx] for a float32 device matrix and an int64 index vector (row pack of the halo exchange).  out_bf16: the rows are
    narrowed to bfloat16 (round-to-nearest-even) by the same kernel — the send buffer of the bf16 halo wire."""
    lib = _lib.load()
    _lib.require_device(x, idx)
    if x.stride(1) != 1:
        x = x.contiguous()
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty((idx.numel(), x.shape[1]), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    fn = lib.cb_gather_rows_bf16_f32 if out_bf16 else lib.cb_gather_rows_f32
    with torch.cuda.device(x.device):
        _lib.check(fn(_lib.ptr(x), x.stride(0) if x.shape[0] > 1 else x.shape[1], _lib.ptr(idx), idx.numel(),
                      x.shape[1], _lib.ptr(out), _lib.stream_ptr()), 'cb_gather_rows_f32')
    return out


def expand_rows(src, pos, fill=0.0):
    """[len(pos), d] matrix whose row r is src[pos[r]] where pos[r] >= 0 and `fill` elsewhere (cb_expand_rows_f32): a compact matrix over a
    row subset (graph.RowSpace: pos int32 [N]) written back to all rows."""
    lib = _lib.load()
    _lib.require_device(src, pos)
    if src.dtype != torch.float32 or src.dim() != 2 or src.shape[1] % 4 or pos.dtype != torch.int32:
        raise ValueError('expand_rows: float32 [n, d] matrix with d % 4 == 0 and an int32 position vector expected')
    src = src.contiguous()
    out = torch.empty((pos.numel(), src.shape[1]), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.cb_expand_rows_f32(_lib.ptr(src), _lib.ptr(pos.contiguous()), pos.numel(), src.shape[1], float(fill), _lib.ptr(out), _lib.stream_ptr()),
                   'cb_expand_rows_f32')
    return out


def unread_rows_fill():
    """What a rows-only training forward writes into the rows of its output that the caller promised not to read (trunk.py "Rows-only forward"):
    NaN (tuning.T.rows_only_poison, the default) — a consumer that reads them after all (TeacherGNN.out, res.commonEmb, an edge-wise loss) gets NaN
    instead of a plausible zero / bias-only row; 0.0 otherwise."""
    from .tuning import T
    return float('nan') if T.rows_only_poison else 0.0


def expand_unread(rows, space, n):
    """[n, C] output of a rows-only forward: `rows` on the loss rows (graph.RowSpace `space`), unread_rows_fill() elsewhere."""
    if rows.shape[1] % 4 == 0:
        return expand_rows(rows, space.pos, unread_rows_fill())
    return torch.full((n, rows.shape[1]), unread_rows_fill(), dtype=torch.float32, device=rows.device).index_copy_(0, space.idx, rows)


def label_propagation(graph, y0, deg_inv_sqrt, alpha, num_propagations):
    """result <- clamp(alpha * D^-1/2 A D^-1/2 result + (1 - alpha) * y0, 0, 1), `num_propagations` times, starting from
    y0 (Label_propagation_model/outcome_correlation.py:128-156 with post_step = clamp(0,1), alpha_term=True).
    Every product with the adjacency is the aggregation kernel on the cached CSR (symmetric graph)."""
    _lib.require_device(y0, deg_inv_sqrt)
    y0 = _c(y0.float())
    dis = _c(deg_inv_sqrt.float())
    a_dis = _c(dis * float(alpha))
    T = int(num_propagations)
    if T <= 0:
        return y0.clone()
    if not hasattr(graph, 'spmm_lp'):            # (a graph object without the fused step: three passes per step)
        result = y0.clone()
        for _ in range(T):
            h, _ = act_bwd(result, None, dis, want_out=True, want_colsum=False)          # D^-1/2 result
            prop = graph.spmm(h, row_scale=a_dis)                                        # alpha * D^-1/2 A (.)
            result = _axpby_raw(1.0, prop, 1.0 - float(alpha), y0).clamp_(0, 1)
        return result
    # rows padded to a multiple of 16 floats (64-byte rows: a 47-class row of 188 bytes straddles sectors — 5.16 vs 4.26 ms per
    # aggregation on the ogbn-products shape, profiles/r03_spmm_narrow_widths.md); the padding columns stay exactly zero
    c = y0.shape[1]
    cp = (c + 15) // 16 * 16 if c > 16 else c
    if cp != c:
        y0 = torch.nn.functional.pad(y0, (0, cp - c))
    # the state carried from step to step is h_t = D^-1/2 result_t: the aggregation's store forms clamp(alpha D^-1/2 (A h_t) + (1 - alpha) y0,
    # 0, 1) and scales it by D^-1/2 for the next gather (cb_spmm_csr_lp_f32); the last step leaves the scale off and returns result_T
    h, _ = act_bwd(y0, None, dis, want_out=True, want_colsum=False)                      # h_0 = D^-1/2 y0
    buf = torch.empty_like(h)
    for t in range(T):
        last = t == T - 1
        graph.spmm_lp(h, a_dis, y0, 1.0 - float(alpha), None if last else dis, out=buf)
        h, buf = buf, h
    return h[:, :c].contiguous() if cp != c else h


# ---------------------------------------------------------------------------------------------
# Correct & Smooth (Label_propagation_model/outcome_correlation.py:95-213)
# ---------------------------------------------------------------------------------------------
ADJ_FORMS = ('DAD', 'DA', 'AD')
CS_MODES = {'double_correlation_autoscale': 0, 'double_correlation_fixed': 1, 'only_outcome_correlation': 2}


def padded_classes(c):
    """Row width of the matrices a propagation gathers (label_propagation: rows of more than 16 classes are padded to 64-byte multiples)."""
    return (c + 15) // 16 * 16 if c > 16 else c


def adj_scales(deg_inv_sqrt, adj):
    """(R, S) of A_norm = diag(R) A diag(S) for gen_normalized_adjs' three forms (:51-55); None stands for the all-ones vector."""
    if adj not in ADJ_FORMS:
        raise ValueError(f"normalised adjacency '{adj}': one of {ADJ_FORMS}")
    dis = _c(deg_inv_sqrt.float())
    if adj == 'DAD':
        return dis, dis
    dis2 = dis * dis
    return (dis2, None) if adj == 'DA' else (None, dis2)


def _prop_graph(graph):
    if not hasattr(graph, 'spmm_prop'):
        raise ValueError(f'{type(graph).__name__} has no spmm_prop: propagation runs on one whole CSRGraph (a node-sharded graph would need the '
                         'exchange of the state rows between the shards at every step, which is missing)')
    if not getattr(graph, 'symmetric', True):
        raise ValueError('propagation needs a symmetric graph (to_undirected, outcome_correlation.py:41): the by-dst CSR then serves DAD, DA and AD alike')
    return graph


def rows_mask(rows, n, device):
    """uint8 [n] mask of a row set given as an index tensor, a bool mask or already as such a mask (no host synchronisation)."""
    if rows is None:
        return None
    rows = torch.as_tensor(rows, device=device)
    if rows.dtype == torch.uint8 and rows.shape == (n,):
        return _c(rows)
    if rows.dtype == torch.bool:
        return rows.to(torch.uint8).contiguous()
    return torch.zeros(n, dtype=torch.uint8, device=device).index_fill_(0, rows.long().reshape(-1), 1)


def _scaled_rows(y, s):
    if s is None:
        return y
    return act_bwd(y, None, s, want_out=True, want_colsum=False)[0]


def _propagate_padded(graph, y, h, R, S, alpha, T, clamp, alpha_term, fix):
    """T steps from the state h = S * y over the padded mix matrix y; returns result_T (padded).  y is never written; h may be y itself."""
    a_r = _c(R * float(alpha)) if R is not None else torch.full((y.shape[0],), float(alpha), dtype=torch.float32, device=y.device)
    c_mix = 1.0 - float(alpha) if alpha_term else 1.0
    bufs = [torch.empty_like(y), torch.empty_like(y) if T > 1 else None]
    for t in range(T):
        out = bufs[t & 1]
        graph.spmm_prop(h, a_r, y, c_mix, clamp=clamp, fix_rows=fix, post_scale=None if t == T - 1 else S, out=out)
        h = out
    return h


def propagate(graph, y, deg_inv_sqrt, alpha, num_propagations, adj='DAD', clamp=(0.0, 1.0), alpha_term=True, fixed_rows=None):
    """general_outcome_correlation (:128-145) on the device: result <- post(alpha * A_norm result + (1 - alpha | 1) * y), `num_propagations` times from
    result = y, with A_norm one of DAD / DA / AD (:51-55) and post = clamp(lo, hi), the identity (clamp=None) and / or fix_inputs (fixed_rows: index
    tensor or mask of the rows that are reset to their rows of y after every step, :194-199).  Every step is ONE launch of cb_spmm_csr_prop_f32: the
    state carried between steps is S * result_t (see adj_scales), so no normalised copy of the adjacency and no elementwise pass exists."""
    _lib.require_device(y, deg_inv_sqrt)
    graph = _prop_graph(graph)
    y = _c(y.float())
    T = int(num_propagations)
    if T <= 0:
        return y.clone()
    R, S = adj_scales(deg_inv_sqrt, adj)
    c = y.shape[1]
    cp = padded_classes(c)
    if cp != c:
        y = torch.nn.functional.pad(y, (0, cp - c))
    fix = rows_mask(fixed_rows, y.shape[0], y.device)
    out = _propagate_padded(graph, y, _scaled_rows(y, S), R, S, alpha, T, None if clamp is None else (float(clamp[0]), float(clamp[1])), alpha_term, fix)
    return out[:, :c].contiguous() if cp != c else out


def cs_residual_init(model_out, labels, label_rows, state_scale=None, want_state=False):
    """pre_residual_correlation (:95-110) as one row kernel: (E0 padded [N, Cp], state = state_scale * E0 or None, sum |E0| as a device scalar [1])."""
    lib = _lib.load()
    _lib.require_device(model_out, labels, label_rows, state_scale)
    p = _c(model_out.float())
    n, c = p.shape
    cp = padded_classes(c)
    e0 = torch.empty((n, cp), dtype=torch.float32, device=p.device)
    state = torch.empty_like(e0) if (want_state or state_scale is not None) else None
    abs_sum = torch.empty(1, dtype=torch.float32, device=p.device)
    wsb = lib.cb_cs_workspace_bytes(n, cp)
    ws = _ws(wsb, p.device)
    with torch.cuda.device(p.device):
        _lib.check(lib.cb_cs_residual_init_f32(_lib.ptr(p), c, _lib.ptr(_c(labels.long().reshape(-1))), _lib.ptr(label_rows), n, c, cp, _lib.ptr(state_scale),
                                               _lib.ptr(e0), _lib.ptr(state), _lib.ptr(abs_sum), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                   'cb_cs_residual_init_f32')
    return e0, state, abs_sum


def cs_correct_snap(mode, model_out, resid, labels, label_rows, abs_sum=None, n_label=0, scale=1.0, state_scale=None):
    """The "correct" combine of `mode` (a key of CS_MODES or its number) and pre_outcome_correlation (:112-126) as one row kernel:
    (res_result [N, C], y2 padded [N, Cp], state = state_scale * y2 or None).  `resid` is the padded result of the first propagation (None for
    only_outcome_correlation); abs_sum the device scalar of cs_residual_init — read on the device, never on the host."""
    lib = _lib.load()
    mode = CS_MODES[mode] if isinstance(mode, str) else int(mode)
    _lib.require_device(model_out, resid, labels, label_rows, abs_sum, state_scale)
    p = _c(model_out.float())
    n, c = p.shape
    cp = padded_classes(c)
    if resid is not None and (resid.dtype != torch.float32 or resid.shape[0] != n or resid.shape[1] < c or resid.stride(1) != 1):
        raise ValueError('cs_correct_snap: resid is a float32 [N, >= C] matrix with contiguous rows')
    res = torch.empty((n, c), dtype=torch.float32, device=p.device)
    y2 = torch.empty((n, cp), dtype=torch.float32, device=p.device)
    state = torch.empty_like(y2) if state_scale is not None else None
    with torch.cuda.device(p.device):
        _lib.check(lib.cb_cs_correct_snap_f32(mode, _lib.ptr(p), c, _lib.ptr(resid), resid.stride(0) if resid is not None else 0,
                                              _lib.ptr(_c(labels.long().reshape(-1))), _lib.ptr(label_rows), n, c, cp, _lib.ptr(abs_sum), int(n_label),
                                              float(scale), _lib.ptr(state_scale), _lib.ptr(res), c, _lib.ptr(y2), _lib.ptr(state), _lib.stream_ptr()),
                   'cb_cs_correct_snap_f32')
    return res, y2, state


def correct_and_smooth(graph, model_out, labels, label_idx, fn, A1, alpha1, num_propagations1, A2, alpha2, num_propagations2, scale=1.0,
                       deg_inv_sqrt=None):
    """Correct & Smooth on the device -> (res_result, result), both [N, C].  fn names the reference function (:158-213):
      double_correlation_autoscale   E0 = onehot - P on the label rows; resid = propagate(E0, A1, clamp(-1, 1)); res = P + autoscale * resid
      double_correlation_fixed       resid = propagate(E0, A1, label rows fixed); res = P + scale * resid
      only_outcome_correlation       res = P (A1 / alpha1 / num_propagations1 unused; the smoothing runs with A2 / alpha2 / num_propagations2)
    then result = propagate(res with the label rows snapped to one-hot, A2, clamp(0, 1)).  label_idx: the label rows (residual_idx == label_idx in
    every reference call; indices are taken as distinct).  2 row kernels + one aggregation launch per step on the graph's by-dst CSR (symmetric graph),
    no host synchronisation between the first and the last launch.  deg_inv_sqrt defaults to the graph's in-degrees ^ -1/2 with inf -> 0 (:46-48)."""
    if fn not in CS_MODES:
        raise ValueError(f"correct_and_smooth: fn '{fn}' is not one of {sorted(CS_MODES)}")
    graph = _prop_graph(graph)
    _lib.require_device(model_out, labels, label_idx)
    mode = CS_MODES[fn]
    p = _c(model_out.float())
    n = p.shape[0]
    if deg_inv_sqrt is None:
        deg_inv_sqrt = graph.in_degrees().to(torch.float32).pow(-0.5)
        deg_inv_sqrt = torch.where(torch.isinf(deg_inv_sqrt), torch.zeros_like(deg_inv_sqrt), deg_inv_sqrt)
    label_idx = torch.as_tensor(label_idx, device=p.device)
    n_label = int(label_idx.sum().item()) if label_idx.dtype in (torch.bool, torch.uint8) else int(label_idx.numel())      # (a mask: counted before the first launch)
    rows = rows_mask(label_idx, n, p.device)
    R2, S2 = adj_scales(deg_inv_sqrt, A2)
    resid = abs_sum = None
    if mode != 2:
        R1, S1 = adj_scales(deg_inv_sqrt, A1)
        e0, h0, abs_sum = cs_residual_init(p, labels, rows, state_scale=S1)
        T1 = int(num_propagations1)
        if T1 <= 0:
            resid = e0
        elif mode == 0:
            resid = _propagate_padded(graph, e0, h0 if h0 is not None else e0, R1, S1, alpha1, T1, (-1.0, 1.0), True, None)
        else:
            resid = _propagate_padded(graph, e0, h0 if h0 is not None else e0, R1, S1, alpha1, T1, None, True, rows)
    res, y2, h2 = cs_correct_snap(mode, p, resid, labels, rows, abs_sum=abs_sum, n_label=n_label, scale=scale, state_scale=S2)
    T2 = int(num_propagations2)
    c = p.shape[1]
    if T2 <= 0:
        return res, y2[:, :c].contiguous()
    out = _propagate_padded(graph, y2, h2 if h2 is not None else y2, R2, S2, alpha2, T2, (0.0, 1.0), True, None)
    return res, (out[:, :c].contiguous() if out.shape[1] != c else out)


def se_topk_replace(le_guess, teacher_se, k, return_selection=False):
    """`SEMLP.replacement` (MLP_model/__init__.py:143-156) for all rows of `le_guess` at once: softmax-weighted mix of the K
    teacher structural embeddings with the largest inner product.  No gradient (the reference detaches both sides)."""
    lib = _lib.load()
    _lib.require_device(le_guess, teacher_se)
    q = le_guess.detach().float()
    t = teacher_se.detach().float()
    if q.stride(1) != 1:
        q = q.contiguous()
    if t.stride(1) != 1:
        t = t.contiguous()
    B, D = q.shape
    N = t.shape[0]
    if t.shape[1] != D:
        raise ValueError(f'embedding widths differ: {tuple(q.shape)} vs {tuple(t.shape)}')
    out = torch.empty((B, D), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=q.device) if return_selection else None
    wgt = torch.empty((B, k), dtype=torch.float32, device=q.device) if return_selection else None
    wsb = lib.cb_topk_replace_workspace_bytes(B, N, k)
    ws = _ws(wsb, q.device)
    with torch.cuda.device(q.device):
        _lib.check(lib.cb_topk_replace_f32(_lib.ptr(q), q.stride(0) if B > 1 else D, _lib.ptr(t), t.stride(0) if N > 1 else D, B, N, D,
                                           int(k), _lib.ptr(out), _lib.ptr(idx), _lib.ptr(wgt), _lib.ptr(ws), wsb, _lib.stream_ptr()),
                   'cb_topk_replace_f32')
    return (out, idx, wgt) if return_selection else out


# ---------------------------------------------------------------------------------------------
# student MLPs (MLP_model/__init__.py): the [LayerNorm, GELU, Dropout] row stage, the part-1 loss, the part-2 input
# ---------------------------------------------------------------------------------------------
def _ln_gelu_drop_fwd_raw(z, gamma, beta, eps, p, seed, want_stats):
    lib = _lib.load()
    rows, d = z.shape
    out = torch.empty_like(z)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=z.device) if want_stats else None
    with torch.cuda.device(z.device):
        _lib.check(lib.cb_ln_gelu_drop_fwd_f32(_lib.ptr(z), rows, d, _lib.ptr(gamma), _lib.ptr(beta), float(eps), float(p), ctypes.c_uint64(seed),
                                               seed_dev_ptr(), _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr()), 'cb_ln_gelu_drop_fwd_f32')
    return out, stats


def _ln_gelu_drop_bwd_raw(dy, z, stats, gamma, beta, p, seed, want_dbias=False):
    """(dz, dgamma, dbeta, colsum(dz) or None) — one pass + the fixed-order finish of the column sums."""
    lib = _lib.load()
    rows, d = z.shape
    dy = _c(dy)
    dz = torch.empty_like(z)
    dgamma = torch.empty(d, dtype=torch.float32, device=z.device)
    dbeta = torch.empty(d, dtype=torch.float32, device=z.device)
    dbias = torch.empty(d, dtype=torch.float32, device=z.device) if want_dbias else None
    wsb = lib.cb_ln_gelu_drop_bwd_workspace_bytes(rows, d)
    ws = _ws(wsb, z.device)
    with torch.cuda.device(z.device):
        _lib.check(lib.cb_ln_gelu_drop_bwd_f32(_lib.ptr(dy), _lib.ptr(z), _lib.ptr(stats), rows, d, _lib.ptr(gamma), _lib.ptr(beta), float(p),
                                               ctypes.c_uint64(seed), seed_dev_ptr(), _lib.ptr(dz), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dbias),
                                               _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_ln_gelu_drop_bwd_f32')
    return dz, dgamma, dbeta, dbias


def _ln_args(d, gamma, beta, p, training, seed):
    _lib.require_device(gamma, beta)
    if gamma.shape != (d,) or beta.shape != (d,) or gamma.dtype != torch.float32 or beta.dtype != torch.float32:
        raise ValueError(f'ln_gelu_dropout expects float32 [{d}] LayerNorm parameters')
    p = float(p) if training else 0.0
    if p >= 1.0:
        raise ValueError('ln_gelu_dropout: p must be < 1')
    if p > 0.0 and seed is None:
        seed = next_seed()
    return p, int(seed or 0)


class _LnGeluDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gamma, beta, eps, p, seed):
        z, gamma, beta = _c(z), _c(gamma), _c(beta)
        need = any(ctx.needs_input_grad[:3])
        out, stats = _ln_gelu_drop_fwd_raw(z, gamma, beta, eps, p, seed, need)
        ctx.p, ctx.seed = p, seed
        if need:
            ctx.save_for_backward(z, stats, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        z, stats, gamma, beta = ctx.saved_tensors
        dz, dgamma, dbeta, _ = _ln_gelu_drop_bwd_raw(g, z, stats, gamma, beta, ctx.p, ctx.seed)
        return dz, dgamma, dbeta, None, None, None


def ln_gelu_dropout(z, gamma, beta, eps=1e-5, p=0.0, training=True, seed=None):
    """dropout(gelu(layer_norm(z))) — `nn.LayerNorm(d), nn.GELU(), nn.Dropout(p)` of a getMLP group (utils.py:898-903) in one pass over z
    (cb_ln_gelu_drop_fwd_f32); the backward recomputes the normalised row and the keep mask from z, 8 bytes of row statistics and the seed
    (cb_ln_gelu_drop_bwd_f32).  The mask is ops.dropout_keep_mask(z.shape, p, seed, device)."""
    _lib.require_device(z)
    if z.dim() != 2 or z.dtype != torch.float32:
        raise ValueError('ln_gelu_dropout expects a float32 [rows, d] matrix')
    p, seed = _ln_args(z.shape[1], gamma, beta, p, training, seed)
    return _LnGeluDropFn.apply(z, gamma, beta, float(eps), p, seed)


class _LinearLnGeluDropFn(torch.autograd.Function):
    """One [Linear, LayerNorm, GELU, Dropout] group: GEMM (bias in its epilogue) + the row kernel; the backward's row kernel also leaves
    colsum(dz) = the Linear's bias gradient, then the two backward contractions of gemm.linear."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, eps, p, seed):
        from . import gemm
        z = gemm.mm_nn(x, weight.t().contiguous(), bias=bias)
        gamma, beta = _c(gamma), _c(beta)
        need = any(ctx.needs_input_grad[:5])
        out, stats = _ln_gelu_drop_fwd_raw(z, gamma, beta, eps, p, seed, need)
        ctx.p, ctx.seed, ctx.has_bias = p, seed, bias is not None
        if need:
            ctx.save_for_backward(x, weight, z, stats, gamma, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import gemm
        x, weight, z, stats, gamma, beta = ctx.saved_tensors
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        dz, dgamma, dbeta, dbias = _ln_gelu_drop_bwd_raw(g, z, stats, gamma, beta, ctx.p, ctx.seed, want_dbias=need_b)
        dx = gemm.mm_nn(dz, weight) if ctx.needs_input_grad[0] else None
        dw = gemm.mm_tn(dz, x) if ctx.needs_input_grad[1] else None
        return dx, dw, dbias, dgamma, dbeta, None, None, None


def linear_ln_gelu_dropout(x, weight, bias, gamma, beta, eps=1e-5, p=0.0, training=True, seed=None):
    """ln_gelu_dropout(x @ weight.T + bias, ...) as one autograd node (see _LinearLnGeluDropFn)."""
    _lib.require_device(x, weight, bias)
    if x.dim() != 2 or x.dtype != torch.float32 or weight.shape[1] != x.shape[1]:
        raise ValueError('linear_ln_gelu_dropout expects a float32 [rows, in] matrix and an [out, in] weight')
    p, seed = _ln_args(weight.shape[0], gamma, beta, p, training, seed)
    return _LinearLnGeluDropFn.apply(x, weight, bias, gamma, beta, float(eps), p, seed)


class _MseRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, row_index):
        lib = _lib.load()
        pred = _c(pred)
        B, D = pred.shape
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        wsb = lib.cb_reduce_workspace_bytes()
        ws = _ws(wsb, pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(lib.cb_mse_rows_f32(_lib.ptr(pred), B, D, _lib.ptr(target), target.stride(0) if target.shape[0] > 1 else D, target.shape[0],
                                           _lib.ptr(row_index), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_mse_rows_f32')
        ctx.save_for_backward(grad)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def mse_rows(pred, target, row_index=None):
    """nn.MSELoss()(pred, target[row_index]) (trainer_node_classification.py:96,108) without the gathered copy; the gradient
    2 (pred - target[row_index]) / numel is written by the same pass.  target is not differentiated (the reference's targets are detached)."""
    _lib.require_device(pred, target, row_index)
    if pred.dim() != 2 or target.dim() != 2 or pred.dtype != torch.float32 or target.dtype != torch.float32 or pred.shape[1] != target.shape[1]:
        raise ValueError('mse_rows expects float32 [B, D] predictions and [N, D] targets')
    if target.stride(1) != 1:
        target = target.contiguous()
    if row_index is not None:
        if row_index.dtype != torch.int64 or row_index.numel() != pred.shape[0]:
            raise ValueError('mse_rows: row_index must be an int64 vector with one entry per prediction row')
        row_index = _c(row_index)
    elif target.shape[0] != pred.shape[0]:
        raise ValueError('mse_rows: without row_index the targets need one row per prediction row')
    return _MseRowsFn.apply(pred, target.detach(), row_index)


def _part2_assemble_raw(out, x, replaced, part1_out, alphas, F, D):
    lib = _lib.load()
    with torch.cuda.device(out.device):
        _lib.check(lib.cb_part2_assemble_f32(_lib.ptr(x), F, _lib.ptr(replaced), _lib.ptr(part1_out), D, _lib.ptr(alphas), out.shape[0], _lib.ptr(out),
                                             _lib.stream_ptr()), 'cb_part2_assemble_f32')


class _Part2InputFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alphas, x, part1_out, teacher_se, k):
        B, F = x.shape
        D = part1_out.shape[1]
        a = _c(alphas.detach())
        out = torch.empty((B, F + 2 * D), dtype=torch.float32, device=x.device)
        _part2_assemble_raw(out, x, None, part1_out, a, F, D)               # x and alphas[0] * part1_out
        replaced = se_topk_replace(out[:, F + D:], teacher_se, k)           # replacement() reads the scaled guess (:103-104)
        _part2_assemble_raw(out, None, replaced, None, a, F, D)             # alphas[1] * replaced
        ctx.F, ctx.D = F, D
        ctx.save_for_backward(replaced, part1_out)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        replaced, part1_out = ctx.saved_tensors
        g = _c(g)
        dal = torch.empty(2, dtype=torch.float32, device=g.device)
        wsb = 2 * lib.cb_reduce_workspace_bytes()
        ws = _ws(wsb, g.device)
        with torch.cuda.device(g.device):
            _lib.check(lib.cb_part2_assemble_bwd_f32(_lib.ptr(g), ctx.F, _lib.ptr(replaced), _lib.ptr(part1_out), ctx.D, g.shape[0], _lib.ptr(dal),
                                                     _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_part2_assemble_bwd_f32')
        return dal, None, None, None, None


def semlp_part2_input(alphas, x, part1_out, teacher_se, k):
    """torch.cat([x, replacement(alphas[0] * part1_out) * alphas[1], alphas[0] * part1_out], -1) (MLP_model/__init__.py:102-108) written
    into one [B, F + 2 D] matrix: the scaled guess goes straight into its block, the top-K kernel reads its queries from there, the scaled
    virtual neighbours fill the middle.  Gradient reaches `alphas` only (x, part1_out and the replacement are detached in the reference;
    the path of alphas[0] through the replacement is cut by its detach())."""
    _lib.require_device(alphas, x, part1_out, teacher_se)
    if x.dim() != 2 or part1_out.dim() != 2 or x.shape[0] != part1_out.shape[0] or alphas.shape != (2,):
        raise ValueError('semlp_part2_input expects x [B, F], part1_out [B, D] and the two alphas')
    return _Part2InputFn.apply(alphas, _c(x.detach().float()), _c(part1_out.detach().float()), teacher_se, int(k))


# ---------------------------------------------------------------------------------------------
# GraphMLP (MLP_model/__init__.py:158-208): the sparse adjacency power on the device, the neighbour-contrastive loss, cosine_sim
# ---------------------------------------------------------------------------------------------
class SparsePower:
    """Device form of the adjacency power A~^r (utils.py:1242-1248), built once from the coalesced COO tensor: int32 `rowptr` [n + 1] / `col`
    and fp32 `val` with ascending columns, for the matrix and (`rowptr_t` / `col_t` / `val_t`) for its transpose — the graph need not be
    symmetric and the backward of the loss reads columns.  `n` = number of nodes."""

    def __init__(self, adj_pow, device):
        adj = adj_pow.detach().coalesce().cpu()
        if adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
            raise ValueError('SparsePower expects a square sparse matrix')
        self.n, self.nnz = int(adj.shape[0]), int(adj._nnz())
        if self.nnz >= 2 ** 31:
            raise ValueError(f'SparsePower: {self.nnz} non-zeros do not fit the int32 index contract (nnz < 2^31)')
        idx, val = adj.indices(), adj.values().float()
        self.device = torch.device(device)
        self.rowptr, self.col, self.val = self._csr(idx[0], idx[1], val)
        self.rowptr_t, self.col_t, self.val_t = self._csr(idx[1], idx[0], val)

    def _csr(self, r, c, v):
        order = torch.argsort(r * self.n + c, stable=True)
        rowptr = torch.zeros(self.n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=self.n), 0)
        return (rowptr.to(torch.int32).to(self.device), c[order].to(torch.int32).to(self.device), v[order].contiguous().to(self.device))

    @classmethod
    def from_adjacency(cls, adj, r, device):
        """The same object built on the device from A~ itself (`adj`: coalesced square sparse COO tensor, host or device): A~ is uploaded once as
        int32 CSR, r - 1 products P <- P A~ (spgemm_csr; the association of graphUtils.sparse_power) give the power, csr_transpose the
        second orientation.  r = 1 is the upload plus the transpose.  No host build, no CPU fallback."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.HipExtensionError('SparsePower.from_adjacency builds the power on an MI355X device; there is no CPU fallback '
                                         '(SparsePower(graphUtils.sparse_power(adj, r), device) is the host build)')
        if int(r) < 1:
            raise ValueError(f'SparsePower.from_adjacency: r = {r} (r >= 1)')
        if not adj.is_sparse or adj.dim() != 2 or adj.shape[0] != adj.shape[1]:
            raise ValueError('SparsePower expects a square sparse matrix')
        if not adj.is_coalesced():
            raise ValueError('SparsePower.from_adjacency expects a coalesced tensor (row-major sorted, no duplicates)')
        n, nnz = int(adj.shape[0]), int(adj._nnz())
        if nnz >= 2 ** 31 or n >= 2 ** 31:
            raise ValueError(f'SparsePower: {nnz} non-zeros / {n} nodes do not fit the int32 index contract (< 2^31)')
        _stage('upload')
        idx, val = adj.indices().to(device), adj.values().detach().to(device).float().contiguous()
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
        rowptr[1:] = torch.cumsum(torch.bincount(idx[0], minlength=n), 0)
        a = (rowptr.to(torch.int32), idx[1].to(torch.int32).contiguous(), val)
        p = a
        for _ in range(int(r) - 1):
            p = spgemm_csr(*p, *a, n)
        self = cls.__new__(cls)
        self.n, self.nnz, self.device = n, int(p[1].numel()), device
        self.rowptr, self.col, self.val = p
        self.rowptr_t, self.col_t, self.val_t = csr_transpose(*p, n)
        _stage('end')
        return self


_stage_hook = None      # tools/bench_power.py: called with the name of a stage of the device build where it begins


def _stage(name):
    if _stage_hook is not None:
        _stage_hook(name)


def _check_range(rc, what):
    """CB_E_RANGE (a size beyond the int32 index contract) is the caller's ValueError; everything else goes through _lib.check."""
    if rc == -2:
        msg = _lib.load().cb_last_error()
        raise ValueError(f'{what}: {msg.decode() if msg else "size exceeds the int32 index contract"}')
    _lib.check(rc, what)


def _bits(n):
    """Bits that hold every value of [0, n)."""
    return max(int(n) - 1, 0).bit_length()


def spgemm_plan(row_products, n_cols, chunk_products):
    """Host planner of spgemm_csr: cuts the rows of A into chunks, each a maximal run of consecutive rows whose products (row_products[i] of
    row i) fit `chunk_products`, at least one row (a row with more products than the budget is a chunk of its own).  A chunk's sort key holds
    the product number, the row inside the chunk and the column: bits(chunk_products) + bits(rows) + bits(n_cols) <= 64, so a chunk holds at
    most 2^(64 - pb - cb) rows.  Returns (chunks, (pb, rb, cb)): [(row0, row1), ...] tiling [0, m) in order, and the bits of product number,
    row (of the largest chunk) and column.  ValueError where no split fits 64 bits."""
    import numpy as np
    rp = row_products.detach().cpu().numpy() if torch.is_tensor(row_products) else np.asarray(row_products)
    rp = rp.astype(np.int64).reshape(-1)
    budget, n_cols = int(chunk_products), int(n_cols)
    if budget < 1 or n_cols < 0 or (rp < 0).any():
        raise ValueError('spgemm_plan: chunk_products >= 1, n_cols >= 0 and row_products >= 0 expected')
    pb, cb = _bits(budget), _bits(max(n_cols, 2))
    if pb + cb > 64:
        raise ValueError(f'spgemm_plan: {pb} product bits (chunk_products = {budget}) and {cb} column bits (n_cols = {n_cols}) do not fit a 64-bit key')
    max_rows = 1 << min(64 - pb - cb, 31)
    m = int(rp.size)
    cum = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(rp)])
    chunks, r0 = [], 0
    while r0 < m:
        r1 = int(np.searchsorted(cum, cum[r0] + budget, side='right')) - 1      # the last r1 with cum[r1] - cum[r0] <= budget
        r1 = min(max(r1, r0 + 1), r0 + max_rows, m)
        chunks.append((r0, r1))
        r0 = r1
    return chunks, (pb, _bits(max((b - a for a, b in chunks), default=1)), cb)


def _csr_args(who, rowptr, col, val, n_cols):
    """int32 / int32 / fp32 contiguous device CSR + the checks that keep the kernels' indices inside their arrays (one host read)."""
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or val.shape != col.shape:
        raise ValueError(f'{who}: rowptr [m + 1], col [nnz] and val [nnz] expected')
    rowptr, col, val = _c(rowptr.to(torch.int32)), _c(col.to(torch.int32)), _c(val.float())
    nnz, n_cols = int(col.numel()), int(n_cols)
    if not 0 <= n_cols < 2 ** 31:
        raise ValueError(f'{who}: {n_cols} columns do not fit the int32 index contract')
    bad = [rowptr[0] != 0, rowptr[-1] != nnz, (rowptr[1:] < rowptr[:-1]).any()]
    if nnz:
        bad += [col.min() < 0, col.max() >= n_cols]
    if bool(torch.stack(bad).any()):
        raise ValueError(f'{who}: not a CSR matrix with {n_cols} columns (rowptr must ascend from 0 to nnz, columns lie in [0, n_cols))')
    return rowptr, col, val


def spgemm_csr(rowptr_a, col_a, val_a, rowptr_b, col_b, val_b, n_cols, chunk_products=None):
    """C = A B of two device CSR matrices (int32 rowptr / col, fp32 val; B has n_cols columns and as many rows as A has columns) as
    (rowptr, col, val) with ascending columns (cb_spgemm.hip: expand - sort - compress).  C[i, j] is the sequential fp32 sum of its
    separately rounded products in the order of A's entries in row i; an entry exists where a product exists, even if the sum is 0.0; the bits
    depend neither on the call nor on `chunk_products` (default tuning.T.spgemm_chunk_products), which bounds the workspace: the rows are
    walked in the chunks of spgemm_plan, one host read per chunk.  nnz(C) >= 2^31 raises ValueError from the running count."""
    lib = _lib.load()
    _lib.require_device(rowptr_a, col_a, val_a, rowptr_b, col_b, val_b)
    from .tuning import T
    budget = int(T.spgemm_chunk_products if chunk_products is None else chunk_products)
    if not 1 <= budget < 2 ** 31:
        raise ValueError(f'spgemm_csr: chunk_products = {budget} (a chunk\'s products are int32-indexed: 1 <= chunk_products < 2^31)')
    _stage('checks + entry offsets')
    dev = rowptr_a.device
    m, k, n_cols = int(rowptr_a.numel()) - 1, int(rowptr_b.numel()) - 1, int(n_cols)
    rowptr_a, col_a, val_a = _csr_args('spgemm_csr (A)', rowptr_a, col_a, val_a, k)
    rowptr_b, col_b, val_b = _csr_args('spgemm_csr (B)', rowptr_b, col_b, val_b, n_cols)
    nnz_a = int(col_a.numel())
    ent_off = torch.empty(nnz_a + 1, dtype=torch.int64, device=dev)
    n_bad = torch.empty(1, dtype=torch.int32, device=dev)
    rowptr = torch.empty(m + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        wsb = lib.cb_spgemm_offsets_workspace_bytes(nnz_a)
        ws = _ws(wsb, dev)
        _check_range(lib.cb_spgemm_entry_offsets_i64(_lib.ptr(col_a), nnz_a, _lib.ptr(rowptr_b), k, _lib.ptr(ent_off), _lib.ptr(n_bad),
                                                     _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_spgemm_entry_offsets_i64')
        if int(n_bad.item()):
            raise ValueError('spgemm_csr: an entry of A points outside B')
        _stage('plan (host)')
        row_off = ent_off[rowptr_a.long()].cpu()                  # products in front of every row of A
        chunks, _ = spgemm_plan(row_off[1:] - row_off[:-1], n_cols, budget)
        row_off = row_off.tolist()
        wsb = lib.cb_spgemm_chunk_workspace_bytes(max((row_off[r1] - row_off[r0] for r0, r1 in chunks), default=0))
        ws = _ws(wsb, dev)
        cols, vals, base = [], [], 0
        for r0, r1 in chunks:
            prods, cnt = row_off[r1] - row_off[r0], 0
            if prods:
                _stage('expand + sort + head scan')
                _check_range(lib.cb_spgemm_chunk_count_f32(_lib.ptr(rowptr_a), _lib.ptr(col_a), _lib.ptr(val_a), _lib.ptr(rowptr_b), _lib.ptr(col_b),
                                                           _lib.ptr(val_b), _lib.ptr(ent_off), r0, r1, k, n_cols, prods, _lib.ptr(count),
                                                           _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_spgemm_chunk_count_f32')
                cnt = int(count.item())
            if base + cnt >= 2 ** 31:      # before anything of that size is allocated
                raise ValueError(f'spgemm_csr: the product holds at least {base + cnt} entries after row {r1}: beyond the int32 index contract (nnz < 2^31)')
            _stage('compress + rowptr')
            c = torch.empty(cnt, dtype=torch.int32, device=dev)
            v = torch.empty(cnt, dtype=torch.float32, device=dev)
            _check_range(lib.cb_spgemm_chunk_emit_f32(_lib.ptr(ws), wsb, r0, r1, n_cols, prods, cnt, base, _lib.ptr(rowptr), _lib.ptr(c), _lib.ptr(v),
                                                      _lib.stream_ptr()), 'cb_spgemm_chunk_emit_f32')
            cols.append(c)
            vals.append(v)
            base += cnt
        rowptr[m:] = base
    _stage('concatenate')
    if len(cols) == 1:
        return rowptr, cols[0], vals[0]
    if not cols:
        return rowptr, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
    return rowptr, torch.cat(cols), torch.cat(vals)


def csr_transpose(rowptr, col, val, n_cols):
    """The transpose of a device CSR matrix with n_cols columns as (rowptr_t [n_cols + 1], col_t, val_t), columns ascending; val_t is a
    bit-exact permutation of val (cb_csr_transpose_f32)."""
    lib = _lib.load()
    _lib.require_device(rowptr, col, val)
    _stage('transpose')
    rowptr, col, val = _csr_args('csr_transpose', rowptr, col, val, n_cols)
    dev, m, n, nnz = rowptr.device, int(rowptr.numel()) - 1, int(n_cols), int(col.numel())
    rowptr_t = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col_t = torch.empty(nnz, dtype=torch.int32, device=dev)
    val_t = torch.empty(nnz, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        wsb = lib.cb_csr_transpose_workspace_bytes(nnz)
        ws = _ws(wsb, dev)
        _check_range(lib.cb_csr_transpose_f32(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), m, n, nnz, _lib.ptr(rowptr_t), _lib.ptr(col_t),
                                              _lib.ptr(val_t), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_csr_transpose_f32')
    return rowptr_t, col_t, val_t


def _ncloss_slab_rows(B):
    from .tuning import T
    rows = int(T.ncloss_slab_rows)
    if rows <= 0:
        rows = max(((1 << 28) // max(int(B), 1)) // 128 * 128, 128)
    if rows % 128:
        raise ValueError(f'tuning.T.ncloss_slab_rows={rows} must be a multiple of 128')
    return rows


class _NCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, power, idx, tau):
        from .tuning import T
        lib = _lib.load()
        z = _c(z)
        B, D = z.shape
        dev = z.device
        f32 = dict(dtype=torch.float32, device=dev)
        pos = torch.empty(power.n, dtype=torch.int32, device=dev)
        rep = torch.empty(B, dtype=torch.int32, device=dev)
        rinv, num, den, w, u = (torch.empty(B, **f32) for _ in range(5))
        loss = torch.empty(1, **f32)
        m_count = torch.empty(1, dtype=torch.int32, device=dev)
        cap = int(T.ncloss_max_splits)
        wsb = lib.cb_ncloss_workspace_bytes(B, cap)
        ws = _ws(wsb, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.cb_ncloss_positions_i64(_lib.ptr(idx), B, power.n, _lib.ptr(pos), _lib.ptr(rep), _lib.stream_ptr()), 'cb_ncloss_positions_i64')
            _lib.check(lib.cb_ncloss_fwd_f32(_lib.ptr(z), D, B, D, float(tau), _lib.ptr(power.rowptr), _lib.ptr(power.col), _lib.ptr(power.val), power.n,
                                             _lib.ptr(idx), _lib.ptr(pos), _lib.ptr(rep), cap, _lib.ptr(rinv), _lib.ptr(num), _lib.ptr(den), _lib.ptr(w),
                                             _lib.ptr(u), _lib.ptr(loss), _lib.ptr(m_count), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_ncloss_fwd_f32')
        ctx.power, ctx.tau, ctx.cap = power, float(tau), cap
        ctx.save_for_backward(z, idx, pos, rep, rinv, w, u)
        m_count = m_count.reshape(())
        ctx.mark_non_differentiable(num, den, m_count)
        return loss.reshape(()), num, den, m_count

    @staticmethod
    def backward(ctx, g, *_unused):
        from . import gemm
        lib = _lib.load()
        z, idx, pos, rep, rinv, w, u = ctx.saved_tensors
        p = ctx.power
        B, D = z.shape
        dev = z.device
        g = g.detach().reshape(1).to(torch.float32).contiguous()
        zhat = torch.empty_like(z)
        dzh = torch.empty_like(z)
        dz = torch.empty_like(z)
        slab = min(_ncloss_slab_rows(B), (B + 127) // 128 * 128)
        P = torch.empty((min(slab, B), B), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.cb_ncloss_normalize_rows_f32(_lib.ptr(z), D, B, D, _lib.ptr(rinv), _lib.ptr(zhat), _lib.stream_ptr()), 'cb_ncloss_normalize_rows_f32')
            for r0 in range(0, B, slab):
                rows = min(slab, B - r0)
                _lib.check(lib.cb_ncloss_bwd_slab_f32(_lib.ptr(z), D, B, D, ctx.tau, _lib.ptr(rinv), _lib.ptr(w), r0, rows, ctx.cap, _lib.ptr(P), B,
                                                      _lib.stream_ptr()), 'cb_ncloss_bwd_slab_f32')
                gemm.mm_nn(P[:rows], zhat, out=dzh[r0:r0 + rows])
            _lib.check(lib.cb_ncloss_bwd_finish_f32(_lib.ptr(z), D, _lib.ptr(zhat), B, D, ctx.tau, _lib.ptr(rinv), _lib.ptr(u), _lib.ptr(p.rowptr), _lib.ptr(p.col),
                                                    _lib.ptr(p.val), _lib.ptr(p.rowptr_t), _lib.ptr(p.col_t), _lib.ptr(p.val_t), p.n, _lib.ptr(idx), _lib.ptr(pos),
                                                    _lib.ptr(rep), _lib.ptr(g), _lib.ptr(dzh), _lib.ptr(dz), _lib.stream_ptr()), 'cb_ncloss_bwd_finish_f32')
        return dz, None, None, None


def neighbor_contrastive_loss(z, power, batch_idx, tau, return_parts=False):
    """GraphMLP's neighbour-contrastive loss of the batch embeddings z [B, D] (MLP_model/__init__.py:190-198) against the adjacency power
    `power` (SparsePower) cropped to the nodes batch_idx (int64 vector, host or device; numpy accepted):
        loss = -mean_{num_i != 0} log(num_i / den_i),  den_i = sum_{j != i} exp(cos_ij / tau),  num_i = sum_{j != i} power[b_i, b_j] exp(cos_ij / tau)
    with no B x B matrix in the forward (cb_ncloss_fwd_f32) and a slab of one in the backward (tuning.T.ncloss_slab_rows).  A node drawn more
    than once is represented by its last position (the reference's CPU behaviour).  Returns the 0-dim loss; with return_parts also
    (num [B], den [B], M 0-dim int32), detached.  M == 0 gives NaN, the reference's mean of an empty tensor.
    Deviation: a batch_idx entry outside [0, power.n) raises ValueError (the reference fails with an IndexError inside its crop); for a device
    batch_idx this check reads one number back."""
    _lib.require_device(z)
    if not isinstance(power, SparsePower):
        raise TypeError('neighbor_contrastive_loss expects an ops.SparsePower (MLP_model.get_neighbor_contrastive_loss converts a torch sparse tensor)')
    if z.dim() != 2 or z.dtype != torch.float32 or z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError('neighbor_contrastive_loss expects a float32 [B, D] matrix with B >= 1')
    if not torch.is_tensor(batch_idx):
        import numpy as np
        batch_idx = torch.as_tensor(np.asarray(batch_idx))
    if batch_idx.dim() != 1 or batch_idx.dtype not in (torch.int64, torch.int32) or batch_idx.numel() != z.shape[0]:
        raise ValueError('neighbor_contrastive_loss: batch_idx must be an integer vector with one node id per row of z')
    lo, hi = int(batch_idx.min()), int(batch_idx.max())
    if lo < 0 or hi >= power.n:
        raise ValueError(f'neighbor_contrastive_loss: batch_idx holds node ids in [{lo}, {hi}], the adjacency power has {power.n} nodes')
    if power.device != z.device:
        raise ValueError('neighbor_contrastive_loss: the SparsePower lives on another device than z')
    idx = _c(batch_idx.to(device=z.device, dtype=torch.int64))
    loss, num, den, m = _NCLossFn.apply(z, power, idx, float(tau))
    return (loss, num, den, m) if return_parts else loss


def ncloss_core(z):
    """'limb' or 'fp32': the MFMA core the sweeps of neighbor_contrastive_loss take for this z (cb_ncloss_uses_limb_core)."""
    z = _c(z)
    return 'limb' if _lib.load().cb_ncloss_uses_limb_core(_lib.ptr(z), z.shape[1], z.shape[1]) else 'fp32'


def cosine_sim(x):
    """Pair-wise cosine similarity [N, N] of the rows of x (MLP_model/__init__.py:200-208): x @ x.T on the MFMA GEMM, then one pass that
    scales element (i, j) by 1 / (|x_i| |x_j|).  Materialises [N, N], as its definition says; no gradient (the loss has its own operator)."""
    from . import gemm
    lib = _lib.load()
    _lib.require_device(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError('cosine_sim expects a float32 [N, D] matrix')
    x = _c(x.detach())
    N, D = x.shape
    s = gemm.mm_nn(x, x.t().contiguous())
    nrm = torch.empty(N, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.cb_ncloss_row_norms_f32(_lib.ptr(x), D, N, D, _lib.ptr(nrm), None, _lib.stream_ptr()), 'cb_ncloss_row_norms_f32')
        _lib.check(lib.cb_cosine_scale_f32(_lib.ptr(s), N, N, _lib.ptr(nrm), _lib.stream_ptr()), 'cb_cosine_scale_f32')
    return s


# ---------------------------------------------------------------------------------------------
# the teacher's edge-wise (link-prediction) term: trainer_node_classification.py:417-438, 507-563; utils.py:754-791  (cb_linkp.hip)
# ---------------------------------------------------------------------------------------------
LINKP_MODES = {'train': 0, 'test': 1}


def _linkp_view(graph):
    v = _lib.CsrView(graph.rowptr.data_ptr(), graph.col.data_ptr(), 0, graph.N, graph.E, 1, 0, 0, None, None, None, 0)
    v._keep = (graph.rowptr, graph.col)
    return v


class LinkSampler:
    """Positive and negative edge samples of `gen_pn_edges` / `my_negative_sampling` (trainer_node_classification.py:507-563) drawn on the device
    CSR: a positive is one of the edges whose endpoints are both inside (mode 'train') or both outside (mode 'test') the train mask, uniform with
    replacement, multiplicity and self loops as edge_index has them; a negative is a pair that is no edge in either direction and no self pair,
    with both endpoints train nodes ('train') or at least one endpoint outside the train split ('test').  Built once per (graph, train_mask): the
    per-mode prefix arrays of valid edges per row (one host read each: V = 0 raises ValueError), the ascending list of train nodes and the int32
    counter of failed negative slots.  Every draw is a pure function of (seed, slot, try): Philox4x32-10, restated on the host in
    tests/linkp_ref.py.  Deviations from the reference, which loops on the host until at least samp_size_n pairs survive its mask filter and then
    uses all of them (a variable count, one synchronisation per batch): the count is exactly n rounded up to even (fixed shapes, no
    synchronisation), and the endpoints are drawn from the allowed node set instead of filtering uniform non-edges by the mask, which gives the
    same conditional distribution."""

    def __init__(self, graph, train_mask):
        from .graph import CSRGraph
        if type(graph) is not CSRGraph or graph.n_cols != graph.N or graph.row_offset != 0:
            raise ValueError('LinkSampler needs a whole square graph.CSRGraph (segmented and node-sharded graphs are out of scope)')
        _lib.require_device(train_mask)
        if train_mask.dtype != torch.bool or train_mask.dim() != 1 or train_mask.numel() != graph.N or train_mask.device != graph.device:
            raise ValueError(f'LinkSampler: train_mask must be a bool vector of {graph.N} nodes on the device of the graph')
        lib = _lib.load()
        self.graph, self.mask = graph, _c(train_mask)
        self._m8 = self.mask.view(torch.uint8)
        self.train_nodes = torch.nonzero(self.mask).reshape(-1).to(torch.int32)      # ascending
        self.n_train = int(self.train_nodes.numel())
        self.failed = torch.zeros(1, dtype=torch.int32, device=graph.device)
        self._prefix = {}
        self._lib = lib

    def _valid(self, mode):
        hit = self._prefix.get(mode)
        if hit is None:
            g = self.graph
            counts = torch.empty(g.N, dtype=torch.int32, device=g.device)
            with torch.cuda.device(g.device):
                _lib.check(self._lib.cb_linkp_valid_counts_i32(ctypes.byref(_linkp_view(g)), _lib.ptr(self._m8), LINKP_MODES[mode], _lib.ptr(counts),
                                                               _lib.stream_ptr()), 'cb_linkp_valid_counts_i32')
            prefix = torch.zeros(g.N + 1, dtype=torch.int32, device=g.device)
            prefix[1:] = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)      # E < 2^31
            V = int(prefix[-1].item())
            if V == 0:
                raise ValueError(f'LinkSampler: no edge has both endpoints {"inside" if mode == "train" else "outside"} the train split (mode {mode!r})')
            hit = self._prefix[mode] = (prefix, V)
        return hit

    @staticmethod
    def _mode(mode):
        if mode not in LINKP_MODES:
            raise NotImplementedError(f"mode must be 'train' or 'test', got {mode!r}")      # (:519-520)
        return LINKP_MODES[mode]

    def positives(self, mode, n, seed=None):
        """int32 [2, n]: row 0 = source, row 1 = destination of n valid edges of `mode`."""
        m = self._mode(mode)
        prefix, V = self._valid(mode)
        g = self.graph
        n = int(n)
        if n < 0:
            raise ValueError('LinkSampler.positives: n >= 0 required')
        seed = next_seed() if seed is None else int(seed)
        out = torch.empty((2, n), dtype=torch.int32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(self._lib.cb_linkp_positives_i32(ctypes.byref(_linkp_view(g)), _lib.ptr(self._m8), m, _lib.ptr(prefix), V, n,
                                                        ctypes.c_uint64(seed % 2 ** 64), seed_dev_ptr(), _lib.ptr(out), _lib.stream_ptr()),
                       'cb_linkp_positives_i32')
        return out

    def negatives(self, mode, n, seed=None):
        """int32 [2, n rounded up to even]: columns 2 s and 2 s + 1 hold (u, v) and (v, u).  A slot that found no pair holds -1 and counts in
        `failed` (check())."""
        m = self._mode(mode)
        g = self.graph
        n = int(n)
        if n < 0:
            raise ValueError('LinkSampler.negatives: n >= 0 required')
        n += n & 1
        if mode == 'train' and self.n_train == 0:
            raise ValueError('LinkSampler.negatives: the train split is empty')
        seed = next_seed() if seed is None else int(seed)
        out = torch.empty((2, n), dtype=torch.int32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(self._lib.cb_linkp_negatives_i32(ctypes.byref(_linkp_view(g)), _lib.ptr(self._m8), m, _lib.ptr(self.train_nodes), self.n_train, n,
                                                        ctypes.c_uint64(seed % 2 ** 64), seed_dev_ptr(), _lib.ptr(out), _lib.ptr(self.failed),
                                                        _lib.stream_ptr()), 'cb_linkp_negatives_i32')
        return out

    def check(self):
        """Reads the counter of failed negative slots (a host synchronisation: call it where the loss is read anyway), clears it, and raises
        RuntimeError if any slot of the draws since the last check found no pair in its tries."""
        n = int(self.failed.item())
        if n:
            self.failed.zero_()
            raise RuntimeError(f'LinkSampler: {n} negative slot(s) found no non-edge in {int(self._lib.cb_linkp_max_tries())} tries (their columns hold -1)')


def _pairs_arg(who, t, device, n='P'):
    """The index pairs of every operator on pairs: an int32 / int64 [2, n] device tensor on `device`, handed back as contiguous int32.  who: the
    caller and its argument ('pair_dot: pairs'), for the messages."""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != 2 or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'{who} must be an int32 / int64 [2, {n}] tensor')
    _lib.require_device(t)
    if t.device != device:
        raise ValueError(f'{who} must live on {device}, the device of the embeddings or graph they index (got {t.device})')
    return _c(t.to(torch.int32))


def _pair_rows(h):
    """h with contiguous rows (a column slice of a wider matrix stays where it is: the kernels take its leading dimension)."""
    return h if h.stride(1) == 1 and h.stride(0) >= h.shape[1] else h.contiguous()


class _Ledger:
    """Status words kept on their devices between two host reads.  add(word) folds a [1] tensor into the word of its device (no synchronisation);
    drain() reads every device's word (a host synchronisation), forgets them all and returns their fold as a Python number, 0 if nothing was added."""

    def __init__(self, fold=torch.add, host_fold=operator.add):
        self._fold, self._host_fold, self._words = fold, host_fold, {}

    def add(self, word):
        have = self._words.get(word.device)
        self._words[word.device] = word.clone() if have is None else self._fold(have, word)

    def drain(self):
        words, self._words = list(self._words.values()), {}
        return functools.reduce(self._host_fold, (w.item() for w in words), 0)


class _LinkpLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, pos, neg):
        lib = _lib.load()
        e = _pair_rows(emb)
        N, D = e.shape
        P, Nn = pos.shape[1], neg.shape[1]
        dev = e.device
        scores = torch.empty(P + Nn, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        mrr = torch.empty(1, dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.cb_linkp_loss_fwd_f32(_lib.ptr(e), e.stride(0), N, D, _lib.ptr(pos), P, _lib.ptr(neg) if Nn else None, Nn, _lib.ptr(scores),
                                                 _lib.ptr(loss), _lib.ptr(mrr), _lib.ptr(status), _lib.stream_ptr()), 'cb_linkp_loss_fwd_f32')
        ctx.save_for_backward(e, pos, neg, scores)
        mrr, status = mrr.reshape(()), status.reshape(())
        ctx.mark_non_differentiable(mrr, scores, status)
        return loss.reshape(()), mrr, scores, status

    @staticmethod
    def backward(ctx, g, *_unused):
        lib = _lib.load()
        e, pos, neg, scores = ctx.saved_tensors
        N, D = e.shape
        P, Nn = pos.shape[1], neg.shape[1]
        dev = e.device
        g = g.detach().reshape(1).to(torch.float32).contiguous()
        demb = torch.empty((N, D), dtype=torch.float32, device=dev)
        wsb = lib.cb_linkp_bwd_workspace_bytes(P, Nn)
        ws = _ws(wsb, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.cb_linkp_loss_bwd_f32(_lib.ptr(e), e.stride(0), N, D, _lib.ptr(pos), P, _lib.ptr(neg) if Nn else None, Nn, _lib.ptr(scores),
                                                 _lib.ptr(g), _lib.ptr(demb), D, _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_linkp_loss_bwd_f32')
        return demb, None, None


def linkp_loss_eva(h_src, pos, neg, return_parts=False):
    """`linkp_loss_eva` (utils.py:759-774) of the DistMult scores <h_src[h], h_src[t]> over the positive pairs pos [2, P] (P >= 1) and the negative
    pairs neg [2, Nn] (int32 or int64, narrowed): (loss, mrr), loss = binary_cross_entropy_with_logits(scores, [1] * P + [0] * Nn) as a 0-dim tensor
    with an autograd node, mrr = cal_MRR as a 0-dim device tensor (no host read in here).  h_src is the full [N, D] float32 embedding matrix (rows
    may be strided); the four gathered [S, D] matrices of the reference are never materialised, and the gradient arrives as one [N, D] matrix whose
    untouched rows are exactly zero, built without atomics: bit-identical from call to call.  Ties between a negative and its positive count for the
    positive (the reference's sort + nonzero gives that when its sort happens to be stable and is undefined otherwise).  A pair with an index
    outside [0, N) — the -1 of a failed LinkSampler slot — is never used as an index: loss and mrr are then NaN and `status` counts such pairs.
    return_parts: also (scores [P + Nn], status 0-dim int32), detached."""
    _lib.require_device(h_src)
    if h_src.dim() != 2 or h_src.dtype != torch.float32 or h_src.shape[0] < 1 or h_src.shape[1] < 1:
        raise ValueError('linkp_loss_eva expects a float32 [N, D] embedding matrix')
    pos = _pairs_arg('linkp_loss_eva: pos', pos, h_src.device)
    neg = _pairs_arg('linkp_loss_eva: neg', neg, h_src.device, 'Nn')
    if pos.shape[1] < 1:
        raise ValueError('linkp_loss_eva: at least one positive pair is required (the MRR is a mean over the positives)')
    loss, mrr, scores, status = _LinkpLossFn.apply(h_src, pos, neg)
    return (loss, mrr, scores, status) if return_parts else (loss, mrr)


def cal_MRR(pos_score, neg_score):
    """`cal_MRR` (utils.py:776-791) as a 0-dim device tensor: k = len(neg) // len(pos) negatives per positive (the rest is dropped),
    rank_i = 1 + #{negatives of group i above pos_i}, mean of 1 / rank in float64, rounded once.  Ties count for the positive."""
    lib = _lib.load()
    _lib.require_device(pos_score, neg_score)
    ps, ns = _c(pos_score.detach().reshape(-1)), _c(neg_score.detach().reshape(-1))
    if ps.dtype != torch.float32 or ns.dtype != torch.float32 or ps.numel() < 1:
        raise ValueError('cal_MRR expects float32 scores and at least one positive')
    mrr = torch.empty(1, dtype=torch.float32, device=ps.device)
    with torch.cuda.device(ps.device):
        _lib.check(lib.cb_linkp_mrr_f32(_lib.ptr(ps), ps.numel(), _lib.ptr(ns) if ns.numel() else None, ns.numel(), _lib.ptr(mrr), _lib.stream_ptr()),
                   'cb_linkp_mrr_f32')
    return mrr.reshape(())


# ---------------------------------------------------------------------------------------------
# link-prediction baselines CN / AA and the counts behind Hits@K / AUC: Link_prediction_baseline/heuristics.py:51-62, 107-129;
# Link_prediction_model/utils.py:43-59  (cb_heur.hip)
# ---------------------------------------------------------------------------------------------
HEUR_KINDS = ('CN', 'AA')
CN_EXACT_BELOW = float(2 ** 24)      # a CN score is an integer held in fp32

_heur_bad, _heur_top = _Ledger(), _Ledger(torch.fmax, max)      # out-of-range pairs / the largest CN score since the last pair_scores_check()


def _out_view(graph):
    v = _lib.CsrView(graph.rowptr_t.data_ptr(), graph.col_t.data_ptr(), 0, graph.N, graph.E, 1, 0, 0, None, None, None, 0)
    v._keep = (graph.rowptr_t, graph.col_t)
    return v


def aa_weights(graph):
    """float64 [N]: 1 / log(in-degree with multiplicity), 0 where the in-degree is <= 1 (heuristics.py:119-120).  Built once per graph and kept on it."""
    w = getattr(graph, '_heur_aa_w', None)
    if w is None:
        lib = _lib.load()
        w = torch.empty(graph.N, dtype=torch.float64, device=graph.device)
        with torch.cuda.device(graph.device):
            _lib.check(lib.cb_heur_aa_weights_f64(ctypes.byref(_linkp_view(graph)), _lib.ptr(w), _lib.stream_ptr()), 'cb_heur_aa_weights_f64')
        graph._heur_aa_w = w
    return w


def pair_scores(graph, pairs, kind='CN', weight=None, return_status=False, group=None):
    """fp32 [P]: the common-neighbour ('CN') or Adamic-Adar ('AA') score of every pair (pairs[0, i], pairs[1, i]) on the graph as given —
    `CN` / `AA` of Link_prediction_baseline/heuristics.py:107-129 with A[s, k] the multiplicity of the edge s -> k: CN = sum_k A[s, k] A[d, k]
    exactly (an integer in fp32; pair_scores_check() raises if one reached 2^24), AA = sum_k A[s, k] A[d, k] / log(c_k) summed in float64 and rounded
    once, c_k the in-degree of k with multiplicity, terms with c_k <= 1 dropped.  No special case for s == d, self loops or pairs that are edges.
    `weight` (float64 [N], kind 'AA' only) replaces 1 / log(c): resource allocation is weight = 1 / c.  pairs: int32 or int64 [2, P] on the graph's
    device; P = 0 returns an empty tensor without a launch.  A pair with an endpoint outside [0, N) is never used as an index: its score is NaN and
    it counts in the status word, which pair_scores_check() reads where the caller reads the scores anyway (return_status: also hand back the int32
    [1] status of this call).  group: 16 or 64 lanes per pair (default: the library's choice); the results do not hinge on it."""
    from .graph import CSRGraph
    if kind == 'PPR':
        raise NotImplementedError("pair_scores: 'PPR' is not built (the reference's PPR needs the fast_pagerank package, which is absent)")
    if kind not in HEUR_KINDS:
        raise ValueError(f"pair_scores: kind must be 'CN' or 'AA', got {kind!r}")
    if type(graph) is not CSRGraph or graph.n_cols != graph.N or graph.row_offset != 0 or getattr(graph, 'rowptr_t', None) is None:
        raise ValueError('pair_scores needs a whole square graph.CSRGraph (segmented and node-sharded graphs are out of scope)')
    if weight is not None and kind == 'CN':
        raise ValueError("pair_scores: `weight` belongs to kind='AA' (CN counts common neighbours unweighted)")
    if group not in (None, 16, 64):
        raise ValueError('pair_scores: group is 16 or 64')
    p32 = _pairs_arg('pair_scores: pairs', pairs, graph.device)
    if weight is not None:
        _lib.require_device(weight)
        if weight.dtype != torch.float64 or weight.dim() != 1 or weight.numel() != graph.N or weight.device != graph.device:
            raise ValueError(f'pair_scores: weight must be a float64 vector of {graph.N} nodes on the device of the graph')
        weight = _c(weight)
    P = int(p32.shape[1])
    dev = graph.device
    score = torch.empty(P, dtype=torch.float32, device=dev)
    if P == 0:
        return (score, torch.zeros(1, dtype=torch.int32, device=dev)) if return_status else score
    lib = _lib.load()
    w = None if kind == 'CN' else (aa_weights(graph) if weight is None else weight)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if group is None:
            rc = lib.cb_heur_pair_scores_f32(ctypes.byref(_out_view(graph)), _lib.ptr(w), _lib.ptr(p32), P, _lib.ptr(score), _lib.ptr(status), _lib.stream_ptr())
        else:
            rc = lib.cb_heur_pair_scores_width_f32(ctypes.byref(_out_view(graph)), _lib.ptr(w), _lib.ptr(p32), P, group, _lib.ptr(score), _lib.ptr(status),
                                                   _lib.stream_ptr())
        _lib.check(rc, 'cb_heur_pair_scores_f32')
    _heur_bad.add(status)
    if kind == 'CN':
        _heur_top.add(torch.nan_to_num(score, nan=0.0).max().reshape(1))
    return (score, status) if return_status else score


def pair_scores_check():
    """Reads the status words of the pair_scores() calls since the last check (a host synchronisation: call it where the scores are read anyway),
    clears them, and raises RuntimeError if a pair had an endpoint outside the graph (its score is NaN) or OverflowError if a CN score reached 2^24
    (fp32 no longer holds every integer there)."""
    bad, top = _heur_bad.drain(), float(_heur_top.drain())
    if bad:
        raise RuntimeError(f'pair_scores: {bad} pair(s) with an endpoint outside [0, N) (their scores are NaN)')
    if top >= CN_EXACT_BELOW:
        raise OverflowError(f'pair_scores: a CN score reached {top:.0f} >= 2^24, beyond which fp32 does not hold every integer')


def rank_counts(pos, neg, return_status=False):
    """(gt, eq) int32 [P]: gt[i] = #{j : neg[j] > pos[i]}, eq[i] = #{j : neg[j] == pos[i]} over all negatives; -0.0 equals +0.0, +-inf compare as
    numbers.  A NaN on either side never compares: the int32 [1] status (return_status) counts them and every gt / eq is then -1; hits_at_k() and
    auc() raise on it.  Nn = 0 gives zeros."""
    _lib.require_device(pos, neg)
    if not torch.is_tensor(pos) or not torch.is_tensor(neg) or pos.dtype != torch.float32 or neg.dtype != torch.float32 or pos.device != neg.device:
        raise ValueError('rank_counts expects float32 scores on one device')
    lib = _lib.load()
    ps, ns = _c(pos.detach().reshape(-1)), _c(neg.detach().reshape(-1))
    P, Nn, dev = ps.numel(), ns.numel(), ps.device
    gt = torch.empty(P, dtype=torch.int32, device=dev)
    eq = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = lib.cb_rank_counts_workspace_bytes(P, Nn)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cb_rank_counts_f32(_lib.ptr(ps) if P else None, P, _lib.ptr(ns) if Nn else None, Nn, _lib.ptr(gt) if P else None,
                                          _lib.ptr(eq) if P else None, _lib.ptr(status), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_rank_counts_f32')
    return (gt, eq, status) if return_status else (gt, eq)


def hits_from_counts(gt, eq, ks):
    """{'Hits@K': mean(gt + eq < K)} in float64 from the integer counts: the OGB rule `pos > K-th largest negative` stated on counts (a tie with the
    K-th largest negative is no hit), 1.0 when there are fewer than K negatives, as OGB gives."""
    if gt.numel() == 0:
        raise ValueError('Hits@K is a mean over the positives: at least one is required')
    worse = gt.to(torch.int64) + eq.to(torch.int64)
    return {f'Hits@{int(k)}': float((worse < int(k)).to(torch.float64).mean().item()) for k in ks}


def auc_from_counts(gt, eq, n_neg):
    """sum_i (Nn - gt_i - eq_i + eq_i / 2) / (P Nn): the Mann-Whitney form of the AUC, equal to roc_auc_score under ties.  The numerator is summed as
    the integer sum_i 2 (Nn - gt_i - eq_i) + eq_i and divided once."""
    P, Nn = int(gt.numel()), int(n_neg)
    if P == 0 or Nn == 0:
        raise ValueError('the AUC needs at least one positive and one negative')
    g, e = gt.to(torch.int64), eq.to(torch.int64)
    return int((2 * (Nn - g - e) + e).sum().item()) / (2 * P * Nn)


def _checked_counts(pos, neg, who):
    gt, eq, status = rank_counts(pos, neg, return_status=True)
    n = int(status.item())
    if n:
        raise ValueError(f'{who}: {n} NaN score(s): a NaN has no rank')
    return gt, eq


def hits_at_k(pos, neg, ks=(20, 50, 100)):
    """{'Hits@K': share of the positives with fewer than K negatives at or above them} (Link_prediction_model/utils.py:43-52 with the OGB evaluator's
    rule); well defined under ties, unlike cal_MRR, which counts ties for the positive."""
    gt, eq = _checked_counts(pos, neg, 'hits_at_k')
    return hits_from_counts(gt, eq, ks)


def auc(pos, neg):
    """The AUC of positives against negatives (Link_prediction_model/utils.py:54-59 `roc_auc_score`), ties counting one half."""
    if pos.numel() == 0 or neg.numel() == 0:
        raise ValueError('the AUC needs at least one positive and one negative')
    gt, eq = _checked_counts(pos, neg, 'auc')
    return auc_from_counts(gt, eq, neg.numel())


# ---------------------------------------------------------------------------------------------
# link predictors and ranking losses: Link_prediction_model/layer.py:85-106, 182-191; loss.py:4-30; model.py:152-158  (cb_linkpred.hip)
# ---------------------------------------------------------------------------------------------
RANK_KINDS = {'auc_loss': 0, 'adaptive_auc_loss': 1, 'log_rank_loss': 2, 'ce_loss': 3, 'info_nce_loss': 4}

_pair_bad = _Ledger()      # unusable pairs since the last pair_check()


def _embedding_arg(who, h):
    if not torch.is_tensor(h) or h.dim() != 2 or h.dtype != torch.float32 or h.shape[0] < 1 or h.shape[1] < 1:
        raise ValueError(f'{who} expects a float32 [N, D] embedding matrix')


def _pair_args(who, h, pairs):
    _embedding_arg(who, h)
    _lib.require_device(h)
    return _pairs_arg(f'{who}: pairs', pairs, h.device, 'S')


def _scatter_out(who, out, N, D, S, dev, of):
    """(dH, workspace, its size) of the two scatters: out validated, or a fresh [N, D]."""
    dh = torch.empty((N, D), dtype=torch.float32, device=dev) if out is None else out
    if tuple(dh.shape) != (N, D) or dh.dtype != torch.float32 or dh.stride(1) != 1 or dh.stride(0) < D or dh.device != dev:
        raise ValueError(f'{who}: out must be a float32 [{N}, {D}] matrix with contiguous rows on the device of {of}')
    wsb = _lib.load().cb_pair_scatter_workspace_bytes(S)
    return dh, _ws(wsb, dev), wsb


def pair_check():
    """Reads the status words of the pair_dot() / pair_linear() calls since the last check (a host synchronisation: call it where the loss is read
    anyway), clears them, and raises RuntimeError if a pair had an endpoint outside [0, N) — the -1 of a failed LinkSampler slot.  Its score, and
    any loss taken over it, is NaN.  Also reachable as pair_dot.check, pair_linear.check and rank_loss.check."""
    bad = _pair_bad.drain()
    if bad:
        raise RuntimeError(f'link predictor: {bad} pair(s) with an endpoint outside [0, N) (their scores are NaN)')


def _pair_scatter_raw(h, pairs, coef, out=None):
    """dH [N, D] = sum_e (coef_e * h[v_e] into row u_e, coef_e * h[u_e] into row v_e); coef [S] (a scalar per pair) or [S, D] (a row per pair).
    h: rows contiguous (any leading dimension); pairs: int32 [2, S], contiguous; out: optional [N, D] destination with contiguous rows."""
    lib = _lib.load()
    N, D = h.shape
    S = pairs.shape[1]
    coef = _pair_rows(coef) if coef.dim() == 2 else _c(coef)
    ldcoef = 0 if coef.dim() == 1 else (coef.stride(0) if S > 1 else D)
    dh, ws, wsb = _scatter_out('pair scatter', out, N, D, S, h.device, 'h')
    with torch.cuda.device(h.device):
        _lib.check(lib.cb_pair_scatter_f32(_lib.ptr(h), h.stride(0), N, D, _lib.ptr(pairs), S, _lib.ptr(coef), ldcoef, _lib.ptr(dh), dh.stride(0) if N > 1 else D, _lib.ptr(ws), wsb,
                                           _lib.stream_ptr()), 'cb_pair_scatter_f32')
    return dh


class _PairDotFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, pairs):
        lib = _lib.load()
        e = _pair_rows(h)
        N, D = e.shape
        S = pairs.shape[1]
        scores = torch.empty(S, dtype=torch.float32, device=e.device)
        status = torch.empty(1, dtype=torch.int32, device=e.device)
        with torch.cuda.device(e.device):
            _lib.check(lib.cb_pair_dot_f32(_lib.ptr(e), e.stride(0), N, D, _lib.ptr(pairs), S, _lib.ptr(scores), _lib.ptr(status), _lib.stream_ptr()),
                       'cb_pair_dot_f32')
        ctx.save_for_backward(e, pairs)
        ctx.mark_non_differentiable(status)
        return scores, status

    @staticmethod
    def backward(ctx, g, _unused):
        e, pairs = ctx.saved_tensors
        return _pair_scatter_raw(e, pairs, g.detach().to(torch.float32)), None


def pair_dot(h, pairs, return_status=False):
    """fp32 [S]: <h[pairs[0, e]], h[pairs[1, e]]> — `DotPredictor.forward(h[u], h[v])` (layer.py:189-191) without the two gathered [S, D] matrices.
    h: the full [N, D] float32 embedding matrix (rows may be strided); pairs: int32 / int64 [2, S] on its device.  The gradient arrives as one
    [N, D] matrix built through a sorted inverted index: no atomics, bit-identical from call to call, untouched rows exactly zero.  A pair with an
    endpoint outside [0, N) is never used as an index: its score is NaN, it contributes no gradient, and pair_dot.check() raises where the
    caller reads the loss (return_status: also hand back the int32 [1] count of this call)."""
    pairs = _pair_args('pair_dot', h, pairs)
    scores, status = _PairDotFn.apply(h, pairs)
    _pair_bad.add(status)
    return (scores, status) if return_status else scores


def _pair_product(h, pairs):
    """h[u] * h[v] materialised; the row of an unusable pair is zero (its endpoints are never used as indices: they are replaced by node 0 first)."""
    N = h.shape[0]
    ok = ((pairs >= 0) & (pairs < N)).all(0)
    u, v = torch.where(ok, pairs[0], 0).long(), torch.where(ok, pairs[1], 0).long()
    return (h[u] * h[v]) * ok[:, None].to(h.dtype)


class _RankLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, pos, neg, k, weight):
        lib = _lib.load()
        P, dev = pos.numel(), pos.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        wsb = lib.cb_rank_loss_workspace_bytes()
        ws = _ws(wsb, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.cb_rank_loss_fwd_f32(kind, _lib.ptr(pos), P, _lib.ptr(neg), k, _lib.ptr(weight), _lib.ptr(loss), _lib.ptr(ws), wsb,
                                                _lib.stream_ptr()), 'cb_rank_loss_fwd_f32')
        ctx.kind, ctx.k = kind, k
        ctx.save_for_backward(pos, neg, weight)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        pos, neg, weight = ctx.saved_tensors
        P, dev = pos.numel(), pos.device
        g = g.detach().reshape(1).to(torch.float32).contiguous()
        dpos, dneg = torch.empty_like(pos), torch.empty_like(neg)
        with torch.cuda.device(dev):
            _lib.check(lib.cb_rank_loss_bwd_f32(ctx.kind, _lib.ptr(pos), P, _lib.ptr(neg), ctx.k, _lib.ptr(weight), _lib.ptr(g), _lib.ptr(dpos),
                                                _lib.ptr(dneg), _lib.stream_ptr()), 'cb_rank_loss_bwd_f32')
        return None, dpos, dneg, None, None


def rank_loss(kind, pos, neg, num_neg=None, weight=None):
    """The pairwise losses of Link_prediction_model/loss.py as a 0-dim tensor with an autograd node: kind is 'auc_loss', 'adaptive_auc_loss'
    (weight [P]), 'log_rank_loss', 'ce_loss' or 'info_nce_loss'; pos holds P >= 1 scores and neg P * num_neg, read as [P, num_neg] exactly as
    loss.py reshapes them (num_neg None: len(neg) / len(pos), which must divide).  Every term is evaluated in float64 from the fp32 scores by the
    reference's formula as written, its + 1e-15 included, summed in float64 in one fixed order and rounded once; the gradients are float64 sums
    rounded once, from the upstream scalar on the device — no host synchronisation.  The reference evaluates in fp32: on saturated scores its
    1 - sigmoid(s) cancels and its exp(s) overflows above s = 88; this is the float64 value of the same formula."""
    if kind not in RANK_KINDS:
        raise ValueError(f'rank_loss: kind must be one of {sorted(RANK_KINDS)}, got {kind!r}')
    _lib.require_device(pos, neg, weight)
    if not torch.is_tensor(pos) or not torch.is_tensor(neg) or pos.dtype != torch.float32 or neg.dtype != torch.float32 or pos.device != neg.device:
        raise ValueError('rank_loss expects float32 scores on one device')
    P, Nn = pos.numel(), neg.numel()
    k = Nn // P if (num_neg is None and P) else int(num_neg or 0)
    if P < 1 or k < 1 or P * k != Nn:
        raise ValueError(f'rank_loss: {Nn} negatives do not reshape to [{P}, {k}] (at least one positive and one negative per positive are required)')
    if kind == 'adaptive_auc_loss':
        if weight is None or weight.dtype != torch.float32 or weight.numel() != P or weight.device != pos.device:
            raise ValueError(f'rank_loss: adaptive_auc_loss needs a float32 weight of {P} elements on the device of the scores')
        weight = _c(weight.detach().reshape(-1))
    else:
        weight = None
    return _RankLossFn.apply(RANK_KINDS[kind], _c(pos.reshape(-1)), _c(neg.reshape(-1)), k, weight)


# ---------------------------------------------------------------------------------------------
# the predictors that take their endpoint rows one at a time: Link_prediction_model/layer.py:108-180, 193-203  (cb_pairpred.hip)
# ---------------------------------------------------------------------------------------------
def pair_scatter_rows(pairs, g0, g1, n_rows, out=None):
    """fp32 [n_rows, D]: sum_e (g0[e] into row pairs[0, e], g1[e] into row pairs[1, e]) — the backward of the two gathers h[u], h[v], built through
    the sorted inverted index of pair_dot's gradient: no atomics, float64 sums in ascending contribution order rounded once, bit-identical from call
    to call, untouched rows exactly zero, pairs with an endpoint outside [0, n_rows) skipped.  g0, g1: float32 [S, D] with contiguous rows and leading
    dimensions of their own (halves or column halves of one matrix pass without a copy).  out: optional [n_rows, D] destination with contiguous
    rows (a wider leading dimension leaves the columns beyond D untouched)."""
    _lib.require_device(pairs, g0, g1, out)
    if not torch.is_tensor(g0) or not torch.is_tensor(g1) or g0.dim() != 2 or g0.shape != g1.shape or g0.dtype != torch.float32 or g1.dtype != torch.float32:
        raise ValueError('pair_scatter_rows: g0 and g1 must be float32 [S, D] matrices of one shape')
    pairs = _pairs_arg('pair_scatter_rows: pairs', pairs, g0.device, 'S')
    S, D = g0.shape
    N = int(n_rows)
    if pairs.shape[1] != S or N < 1 or D < 1 or g1.device != g0.device:
        raise ValueError(f'pair_scatter_rows: {pairs.shape[1]} pairs for {S} rows, or n_rows < 1, or an empty row')
    lib = _lib.load()
    g0, g1 = _pair_rows(g0), _pair_rows(g1)
    dh, ws, wsb = _scatter_out('pair_scatter_rows', out, N, D, S, g0.device, 'the rows')
    with torch.cuda.device(g0.device):
        _lib.check(lib.cb_rows_scatter_f32(N, D, _lib.ptr(pairs), S, _lib.ptr(g0), g0.stride(0) if S > 1 else D, _lib.ptr(g1), g1.stride(0) if S > 1 else D,
                                                _lib.ptr(dh), dh.stride(0) if N > 1 else D, _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_rows_scatter_f32')
    return dh


def _rows_idx_arg(who, h, idx):
    _embedding_arg(who, h)
    _lib.require_device(h, idx)
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.shape[0] not in (1, 2) or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f'{who}: idx must be an int32 / int64 [nseg, R] tensor, nseg 1 or 2')
    if idx.device != h.device:
        raise ValueError(f'{who}: idx must live on {h.device}, the device of the embeddings it indexes (got {idx.device})')
    return _c(idx.to(torch.int32))


def _rows_ok(h, idx):
    """bool [R]: every index of the row lies in [0, N)."""
    return ((idx >= 0) & (idx < h.shape[0])).all(0)


def _rows_operand(h, idx):
    """The A operand materialised: [h[idx[0]] | h[idx[1]] ...]; the row of an unusable index is zero (its indices are replaced by node 0 first)."""
    ok = _rows_ok(h, idx)
    safe = torch.where(ok[None, :], idx, torch.zeros_like(idx)).long()
    return torch.cat([h[safe[s]] for s in range(idx.shape[0])], dim=1) * ok[:, None].to(h.dtype)


def _scatter_segments(idx, dx, D, n_rows):
    """dH of a rows GEMM from dX [R, nseg * D].  Two segments: the column halves of dX go to idx[0] and idx[1].  One segment: rows r < R / 2 and
    r >= R / 2 are the two sides of R / 2 pairs (an odd R gets one zero row with the last index once more)."""
    if idx.shape[0] == 2:
        return pair_scatter_rows(idx, dx[:, :D], dx[:, D:], n_rows)
    R = idx.shape[1]
    if R % 2:
        idx = torch.cat([idx, idx[:, -1:]], dim=1)
        dx = torch.cat([dx, torch.zeros_like(dx[-1:])], dim=0)
        R += 1
    return pair_scatter_rows(idx.reshape(2, R // 2), dx[:R // 2], dx[R // 2:], n_rows)


class _GatherForm:
    """What differs between the two linears whose A operand is gathered while the GEMM stages it (csrc/cb_gather_gemm.h): the product form
    (h[u] * h[v], cb_pair_gemm_nn_f32) and the rows form (h[i] or [h[i] | h[j]], cb_rows_gemm_nn_f32)."""

    def __init__(self, who, entry, args, query, idx_arg, ktot, operand, scatter):
        self.who, self.entry = who, entry      # the public function's name (messages); the C entry
        self.args = args                       # (e, idx, out) -> the entry's arguments up to bias, out = (b, ldb, y, ldc, yd, ldc2, Nout)
        self.query = query                     # (lib, e, idx, b) -> the entry's *_supported answer
        self.idx_arg = idx_arg                 # (who, h, idx) -> the validated int32 index tensor
        self.ktot = ktot                       # (h, idx) -> columns of A
        self.operand = operand                 # (e, idx) -> A materialised (zero rows for unusable indices)
        self.scatter = scatter                 # (e, idx, dX) -> dH

    def supported(self, e, idx, b):
        return bool(self.query(_lib.load(), e, idx, b))

    def raw(self, e, idx, b, bias, relu, p, seed, row0):
        """(y, dropout_p(y) | None, status) of the fused entry: y = act(A @ b + bias), b [Ktot, Nout] contiguous, idx int32 and contiguous."""
        lib = _lib.load()
        R, Nout = idx.shape[1], b.shape[1]
        dev = e.device
        y = torch.empty((R, Nout), dtype=torch.float32, device=dev)
        yd = torch.empty((R, Nout), dtype=torch.float32, device=dev) if p > 0.0 else None
        status = torch.empty(1, dtype=torch.int32, device=dev)
        out = (_lib.ptr(b), Nout, _lib.ptr(y), Nout, _lib.ptr(yd), Nout, Nout)
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, self.entry)(*self.args(e, idx, out), _lib.ptr(bias), int(bool(relu)), float(p), ctypes.c_uint64(seed), seed_dev_ptr(),
                                                int(row0), _lib.ptr(status), _lib.stream_ptr()), self.entry)
        return y, yd, status

    def any(self, e, idx, b, bias=None, relu=False, p=0.0, seed=0, row0=0, fused=None):
        """raw() where the fused form exists (and fused is not False), else the same operators one after the other; no autograd."""
        from . import gemm
        Nout = b.shape[1]
        can = idx.shape[1] > 0 and self.supported(e, idx, b)
        if fused and not can:
            raise _lib.HipExtensionError(f'{self.who}: the fused form does not exist for this shape ({self.who}_supported)')
        if can and fused is not False:
            return self.raw(e, idx, b, bias, relu, p, seed, row0)
        ok = _rows_ok(e, idx)
        y = gemm.mm_nn(self.operand(e, idx), b, bias=bias, relu=relu)
        y = torch.where(ok[:, None], y, torch.full_like(y, float('nan')))
        status = (~ok).sum().to(torch.int32).reshape(1)
        return y, (_dropout_raw(y, p, seed, row0 * Nout) if p > 0.0 else None), status


_PRODUCT = _GatherForm(
    'pair_linear', 'cb_pair_gemm_nn_f32',
    lambda e, pairs, out: (_lib.ptr(e), e.stride(0), e.shape[0], _lib.ptr(pairs), pairs.shape[1], *out, e.shape[1]),
    lambda lib, e, pairs, b: lib.cb_pair_gemm_nn_supported(_lib.ptr(e), e.stride(0), _lib.ptr(b), b.shape[1], b.shape[1], b.shape[0]),
    _pair_args, lambda h, pairs: h.shape[1], _pair_product, lambda e, pairs, dx: _pair_scatter_raw(e, pairs, dx))
_ROWS = _GatherForm(
    'rows_linear', 'cb_rows_gemm_nn_f32',
    lambda e, idx, out: (_lib.ptr(e), e.stride(0), e.shape[0], e.shape[1], _lib.ptr(idx), idx.shape[0], idx.shape[1], *out),
    lambda lib, e, idx, b: lib.cb_rows_gemm_nn_supported(_lib.ptr(e), e.stride(0), e.shape[1], idx.shape[0], _lib.ptr(b), b.shape[1], b.shape[1]),
    _rows_idx_arg, lambda h, idx: idx.shape[0] * h.shape[1], _rows_operand, lambda e, idx, dx: _scatter_segments(idx, dx, e.shape[1], e.shape[0]))
_pair_linear_raw, _rows_linear_raw, _rows_linear_any = _PRODUCT.raw, _ROWS.raw, _ROWS.any


def pair_linear_supported(h, weight):
    """The fused first layer exists for this shape (cb_pair_gemm_nn_supported): in and out widths multiples of 4, 16-byte aligned rows."""
    e, b = _pair_rows(h), weight.t().contiguous()
    return e.shape[1] == b.shape[0] and _PRODUCT.supported(e, None, b)


def rows_linear_supported(h, idx, weight):
    """The fused form exists for this shape (cb_rows_gemm_nn_supported): out width a multiple of 4, row length a multiple of 4 (one segment) or of 16
    (two segments: no K step straddles the seam), 16-byte aligned rows."""
    e, b = _pair_rows(h), weight.t().contiguous()
    return _ROWS.ktot(e, idx) == b.shape[0] and _ROWS.supported(e, idx, b)


class _GatherLinearFn(torch.autograd.Function):
    """Y = act(A @ W^T + b) with A the form's gathered operand, nn.Linear's weight layout [out, in]; returns dropout_p(Y) when p > 0."""

    @staticmethod
    def forward(ctx, form, h, idx, weight, bias, relu, p, seed, row0, fused):
        e = _pair_rows(h)
        y, yd, status = form.any(e, idx, weight.t().contiguous(), bias, relu, p, seed, row0, fused)
        ctx.form, ctx.relu, ctx.p, ctx.seed, ctx.row0, ctx.has_bias = form, bool(relu), float(p), int(seed), int(row0), bias is not None
        ctx.save_for_backward(e, idx, weight, y if relu else None)
        ctx.mark_non_differentiable(status)
        return (yd if p > 0.0 else y), status

    @staticmethod
    def backward(ctx, g, _unused):
        from . import gemm
        e, idx, weight, y = ctx.saved_tensors
        Nout = weight.shape[0]
        g = _c(g)
        if ctx.p > 0.0:
            g = _dropout_raw(g, ctx.p, ctx.seed, ctx.row0 * Nout)
        need_b = ctx.has_bias and ctx.needs_input_grad[4]
        if ctx.relu or need_b:
            gm, db = act_bwd(g, y if ctx.relu else None, None, want_out=ctx.relu, want_colsum=need_b)
            if gm is None:
                gm = g
        else:
            gm, db = g, None
        dh = ctx.form.scatter(e, idx, gemm.mm_nn(gm, weight)) if ctx.needs_input_grad[1] else None      # dX = gm @ W, scattered by the form
        dw = gemm.mm_tn(gm, ctx.form.operand(e, idx)) if ctx.needs_input_grad[3] else None             # A exists here only
        return None, dh, None, dw, db, None, None, None, None, None


def _gather_linear(form, h, idx, weight, bias, relu, p, seed, row0, return_status, fused):
    idx = form.idx_arg(form.who, h, idx)
    _lib.require_device(weight, bias)
    if weight.dim() != 2 or weight.dtype != torch.float32 or weight.shape[1] != form.ktot(h, idx):
        raise ValueError(f'{form.who}: weight must be a float32 [out, {form.ktot(h, idx)}] matrix')
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'{form.who}: 0 <= p < 1 required')
    if p > 0.0 and seed is None:
        seed = next_seed()
    y, status = _GatherLinearFn.apply(form, h, idx, weight, bias, bool(relu), p, int(seed or 0), int(row0), None if fused is None else bool(fused))
    _pair_bad.add(status)
    return (y, status) if return_status else y


def pair_linear(h, pairs, weight, bias=None, relu=False, p=0.0, seed=None, row0=0, return_status=False, fused=None):
    """act((h[u] * h[v]) @ weight^T + bias), then F.dropout(p) when p > 0: the first Linear of `MLPPredictor.forward(h[u], h[v])` (layer.py:99-104)
    on index pairs.  The product is formed while the three-limb GEMM stages its A operand (cb_pair_gemm_nn_f32): neither gathered matrix nor the
    product is written in the forward, and the output has the bits of gemm.mm_nn(h[u] * h[v], weight.t(), bias, relu) — with p > 0 those of
    gemm.mm_nn_drop2 for (seed, row0).  Backward: act_bwd, dX = gm @ W on mm_nn, dH through the sorted inverted index with row coefficients (no
    atomics), dW = gm^T @ (h[u] * h[v]) on mm_tn over a product matrix materialised there.  Where the fused form does not exist for the shape
    (pair_linear_supported) the same operators run one after the other; fused=False asks for that.  Unusable pairs: as pair_dot."""
    return _gather_linear(_PRODUCT, h, pairs, weight, bias, relu, p, seed, row0, return_status, fused)


def rows_linear(h, idx, weight, bias=None, relu=False, p=0.0, seed=None, row0=0, return_status=False, fused=None):
    """act(A @ weight^T + bias), then F.dropout(p) when p > 0, with A the gather h[idx[0]] (idx [1, R]) or the concatenation [h[idx[0]] | h[idx[1]]]
    (idx [2, R]); weight [out, nseg * D].  A is formed while the three-limb GEMM stages it (cb_rows_gemm_nn_f32) and never written in the forward;
    the output has the bits of gemm.mm_nn(A, weight.t(), bias, relu) — with p > 0 those of gemm.mm_nn_drop2 for (seed, row0).  Backward: act_bwd,
    dX = gm @ W on mm_nn, dH through pair_scatter_rows (no atomics; with one segment row r is scattered as one side of the pair (r, r + R / 2), so
    an unusable index drops that pair's two rows), dW = gm^T @ A on mm_tn over an A materialised there.  Where the fused form does not exist for
    the shape (rows_linear_supported) the same operators run one after the other; fused=False asks for that, fused=True raises there.  A row with
    an index outside [0, N) is NaN and counts in the status that pair_check() reads."""
    return _gather_linear(_ROWS, h, idx, weight, bias, relu, p, seed, row0, return_status, fused)


def pair_bilinear_supported(h, weight):
    """The fused bilinear score exists for this shape (cb_rows_bilinear_supported): D a multiple of 4, 16-byte aligned rows."""
    lib = _lib.load()
    e, wt = _pair_rows(h), weight.t().contiguous()
    D = e.shape[1]
    return tuple(weight.shape) == (D, D) and bool(lib.cb_rows_bilinear_supported(_lib.ptr(e), e.stride(0), D, _lib.ptr(wt), D))


class _PairBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, pairs, weight):
        lib = _lib.load()
        e = _pair_rows(h)
        N, D = e.shape
        S = pairs.shape[1]
        dev = e.device
        wt = weight.t().contiguous()
        if S > 0 and bool(lib.cb_rows_bilinear_supported(_lib.ptr(e), e.stride(0), D, _lib.ptr(wt), D)):
            scores = torch.empty(S, dtype=torch.float32, device=dev)
            status = torch.empty(1, dtype=torch.int32, device=dev)
            wsb = lib.cb_rows_bilinear_workspace_bytes(S, D)
            ws = _ws(wsb, dev)
            with torch.cuda.device(dev):
                _lib.check(lib.cb_rows_bilinear_f32(_lib.ptr(e), e.stride(0), N, D, _lib.ptr(pairs), S, _lib.ptr(wt), D, _lib.ptr(scores), _lib.ptr(status),
                                                    _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_rows_bilinear_f32')
        else:      # the shape is outside the fused form: the rows GEMM (itself composed there), then the dot
            ok = _rows_ok(e, pairs)
            z, _, _ = _rows_linear_any(e, pairs[:1], wt)
            safe_v = torch.where(ok, pairs[1], torch.zeros_like(pairs[1])).long()
            scores = torch.where(ok, (z * e[safe_v]).sum(-1), torch.full((S,), float('nan'), dtype=torch.float32, device=dev))
            status = (~ok).sum().to(torch.int32).reshape(1)
        ctx.save_for_backward(e, pairs, weight)
        ctx.mark_non_differentiable(status)
        return scores, status

    @staticmethod
    def backward(ctx, g, _unused):
        from . import gemm
        e, pairs, weight = ctx.saved_tensors
        g = _c(g.detach().to(torch.float32))[:, None]
        dh = dw = None
        if ctx.needs_input_grad[0]:
            g0 = _rows_linear_any(e, pairs[1:], _c(weight))[0] * g                      # g * (h[v] @ W) into row u
            g1 = _rows_linear_any(e, pairs[:1], weight.t().contiguous())[0] * g         # g * (h[u] @ W^T) into row v
            dh = pair_scatter_rows(pairs, g0, g1, e.shape[0])
        if ctx.needs_input_grad[2]:
            ok = _rows_ok(e, pairs)
            gz = torch.where(ok[:, None], g, torch.zeros_like(g))                        # (an unusable pair's g is the NaN score's: it adds nothing)
            dw = gemm.mm_tn(_rows_operand(e, pairs[1:]) * gz, _rows_operand(e, pairs[:1]))
        return dh, None, dw


def pair_bilinear(h, pairs, weight, return_status=False):
    """fp32 [S]: sum_j (weight @ h[u_e])_j h[v_e, j] — `BilinearPredictor.forward(h[u], h[v])` (layer.py:201-203), sum(bilin(x_i) * x_j, -1), without
    the gathered matrices and without bilin(x_i): the dot against row v_e is taken in the epilogue of the indexed-row GEMM over u
    (cb_rows_bilinear_f32), so under torch.no_grad() nothing of size S x D is allocated.  weight: float32 [D, D].  The backward saves nothing of
    size S x D either: it RECOMPUTES the two products with the indexed-row GEMM (g * (h[v] @ W) goes into row u, g * (h[u] @ W^T) into row v,
    through pair_scatter_rows) and forms dW = (g * h[v])^T @ h[u] on mm_tn over gathers materialised there.  A pair's score does not depend on its
    place in the batch.  Where the fused form does not exist (pair_bilinear_supported: D % 4, alignment) the same value is composed from the rows
    GEMM and a torch reduction.  Unusable pairs: as pair_dot."""
    pairs = _pair_args('pair_bilinear', h, pairs)
    _lib.require_device(weight)
    if not torch.is_tensor(weight) or weight.dim() != 2 or weight.dtype != torch.float32 or tuple(weight.shape) != (h.shape[1], h.shape[1]):
        raise ValueError(f'pair_bilinear: weight must be a float32 [{h.shape[1]}, {h.shape[1]}] matrix')
    scores, status = _PairBilinearFn.apply(h, pairs, weight)
    _pair_bad.add(status)
    return (scores, status) if return_status else scores


pair_dot.check = pair_linear.check = rank_loss.check = rows_linear.check = pair_bilinear.check = pair_check


# ---------------------------------------------------------------------------------------------
# one layer of the link-prediction encoders (Link_prediction_model/layer.py:8-35; csrc/cb_sage.hip)
# ---------------------------------------------------------------------------------------------
SAGE_MODES = ('SAGE', 'WSAGE', 'GCN')
sage_paths = collections.deque(maxlen=256)      # ('fwd' | 'bwd', 'fused' | 'composed') per layer launch, newest last (tests, tools/bench_sage.py)


def inv_indeg(graph):
    """1 / in-degree as float32 [N], 0 where a node has no in-edge (its mean is 0, not NaN); made once per graph."""
    s = getattr(graph, '_inv_indeg', None)
    if s is None:
        deg = (graph.rowptr[1:] - graph.rowptr[:-1]).to(torch.float32)
        s = graph._inv_indeg = torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg)).contiguous()
    return s


def _sage_image(W_n, W_s, transpose):
    lib = _lib.load()
    nb = lib.cb_sage_image_bytes(int(W_s is not None))
    img = torch.empty(nb, dtype=torch.uint8, device=W_n.device)
    with torch.cuda.device(W_n.device):
        _lib.check(lib.cb_sage_image_f32(_lib.ptr(W_n), W_n.stride(0), _lib.ptr(W_s), W_s.stride(0) if W_s is not None else 0, int(bool(transpose)),
                                         _lib.ptr(img), nb, _lib.stream_ptr()), 'cb_sage_image_f32')
    return img


def _sage_supported(h, d_out, has_self, agg, out):
    lib = _lib.load()
    return bool(lib.cb_sage_layer_supported(h.shape[1], d_out, int(h.dtype == torch.bfloat16), _lib.ptr(h), h.stride(0), _lib.ptr(h if has_self else None),
                                            h.stride(0), _lib.ptr(agg), agg.stride(0) if agg is not None else 0, _lib.ptr(out), out.stride(0)))


def sage_layer_raw(graph, h, W_n, W_s=None, bias=None, scale=None, relu=False, p=0.0, seed=0, backward=False, want_agg=False, fused=None, out=None, row0=0):
    """(out, agg or None, path): one encoder layer without autograd.  forward (backward=False): by-dst CSR, agg = scale * (A h) by row,
    out = epi([agg | h] @ [W_n^T ; W_s^T] + bias).  backward=True: by-src CSR, agg = A^T (scale * h) by source row, out = [agg | h] @ [W_n ; W_s].
    W_s None: no self block.  fused (None: tuning.T.sage_fused): the one-kernel layer where cb_sage_layer_supported allows, else — and for
    fused=False — the composed path: graph.spmm, the materialised [agg | h], one cb_gemm_nn_f32 with K = 2 d, ops.dropout's kernel.  The two give the
    same bits.  out: optional [N, d_out] float32 destination with contiguous rows.
    graph may be a graph.WeightedAdj (an adjacency with one value per stored edge; scale must be None): agg = A_w h, resp. A_w^T h — the fused path is
    cb_ewlayer_f32, the composed one WeightedAdj.spmm_ew + the same GEMM; the same bits again."""
    from . import gemm
    from .graph import CSRGraph, WeightedAdj
    from .tuning import T
    lib = _lib.load()
    _lib.require_device(h, W_n, W_s, bias, scale, out)
    adj = None
    if isinstance(graph, WeightedAdj):
        if scale is not None:
            raise ValueError('sage_layer: an adjacency with values takes no row / source factor beside them (mode SAGE reads its .graph)')
        adj, graph = graph, graph.graph
    if not isinstance(graph, CSRGraph) or graph.n_cols != graph.N or (backward and graph.rowptr_t is None):
        raise ValueError('sage_layer: the whole square graph on this device (a CSRGraph with both orientations) is required; node-sharded and segmented '
                         'graphs are not built for the encoders')
    if h.dim() != 2 or h.shape[0] != graph.N or (h.shape[1] > 1 and h.stride(1) != 1):
        raise ValueError(f'sage_layer: rows [{graph.N}, d] with contiguous elements expected, got {tuple(h.shape)}')
    if p and not relu:
        raise ValueError('sage_layer: dropout follows the ReLU (layer.py:29-35)')
    N, d = h.shape
    has_self = W_s is not None
    d_out = W_n.shape[1] if backward else W_n.shape[0]
    if tuple(W_n.shape) != ((d, d_out) if backward else (d_out, d)) or (has_self and W_s.shape != W_n.shape) or W_n.dtype != torch.float32:
        raise ValueError(f'sage_layer: weights [out, in] float32 expected, got {tuple(W_n.shape)} for rows of {d}')
    W_n = _c(W_n)
    W_s = _c(W_s) if has_self else None
    if out is None:
        out = torch.empty((N, d_out), dtype=torch.float32, device=h.device)
    elif tuple(out.shape) != (N, d_out) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError(f'sage_layer: out must be a float32 [{N}, {d_out}] matrix with contiguous rows')
    want_fused = T.sage_fused if fused is None else bool(fused)
    if want_fused and N > 0 and _sage_supported(h, d_out, has_self, None, out):
        plan = graph._plan_t if backward else graph._plan
        agg, hubs_only = None, 0
        if want_agg or plan.n_hubs > 0:      # (hub rows reach the kernel's tile through memory: an [N, 256] allocation of which only those rows are written)
            agg, hubs_only = torch.empty((N, 256), dtype=torch.float32, device=h.device), int(not want_agg)
        img = _sage_image(W_n, W_s, transpose=not backward)
        view = graph._view(256, backward, use_flags=True)
        with torch.cuda.device(h.device):
            if adj is not None:
                _lib.check(lib.cb_ewlayer_f32(ctypes.byref(view), _lib.ptr(adj.val_t if backward else adj.val), _lib.ptr(h), h.stride(0),
                                              _lib.ptr(h if has_self else None), h.stride(0), _lib.ptr(img), _lib.ptr(bias), int(bool(relu)), float(p),
                                              ctypes.c_uint64(int(seed)), seed_dev_ptr(), int(row0), _lib.ptr(agg), 256 if agg is not None else 0, hubs_only,
                                              _lib.ptr(out), out.stride(0), _lib.stream_ptr()), 'cb_ewlayer_f32')
                sage_paths.append(('bwd' if backward else 'fwd', 'fused'))
                return out, (agg if want_agg else None), 'fused'
            _lib.check(lib.cb_sage_layer_f32(ctypes.byref(view), _lib.ptr(h), h.stride(0), _lib.ptr(h if has_self else None), h.stride(0),
                                             _lib.ptr(scale if backward else None), _lib.ptr(None if backward else scale), _lib.ptr(img), _lib.ptr(bias),
                                             int(bool(relu)), float(p), ctypes.c_uint64(int(seed)), seed_dev_ptr(), int(row0), _lib.ptr(agg),
                                             256 if agg is not None else 0, hubs_only, _lib.ptr(out), out.stride(0), _lib.stream_ptr()), 'cb_sage_layer_f32')
        sage_paths.append(('bwd' if backward else 'fwd', 'fused'))
        return out, (agg if want_agg else None), 'fused'
    K = 2 * d if has_self else d
    cat = torch.empty((N, K), dtype=torch.float32, device=h.device)
    aggv = cat[:, :d]
    if adj is not None:
        adj.spmm_ew(h, transpose=backward, out=aggv)
    elif backward and scale is not None and d % 256:      # (the source-row factor exists at d % 256 == 0: elsewhere a row-scaled copy of h is gathered)
        graph.spmm(act_bwd(h, None, scale)[0], transpose=True, out=aggv)
    else:
        graph.spmm(h, transpose=backward, row_scale=None if backward else scale, col_scale=scale if backward else None, out=aggv)
    if has_self:
        cat[:, d:].copy_(h)
        B = torch.cat([W_n, W_s]) if backward else torch.cat([W_n.t(), W_s.t()])
    else:
        B = W_n if backward else W_n.t()
    if p:
        y = gemm.mm_nn(cat, B.contiguous(), bias=bias, relu=relu)
        out.copy_(_dropout_raw(y, p, seed, offset=int(row0) * d_out))
    else:
        gemm.mm_nn(cat, B.contiguous(), bias=bias, relu=relu, out=out)
    sage_paths.append(('bwd' if backward else 'fwd', 'composed'))
    return out, (aggv if want_agg else None), 'composed'


class _SageLayerFn(torch.autograd.Function):
    """Y = epi((s * (A X)) W_n^T + X W_s^T + b).  With G = dY * 1[Y > 0] / (1 - p) (the stored activation is the mask: dropout(relu(y)) > 0 exactly where the
    ReLU passed and the mask kept; G = dY on a layer without ReLU) and R = A^T (s * G):  dX = R W_n + G W_s,  dW_n = R^T X,  dW_s = G^T X,  db = colsum(G).
    The forward stores neither the aggregated matrix nor mask words.  graph a graph.WeightedAdj (WSAGE / GCN): A is A_w, the values are data (no gradient)."""

    @staticmethod
    def forward(ctx, graph, x, W_n, W_s, bias, mode, relu, p, seed, fused):
        if mode == 'SAGE':
            graph = getattr(graph, 'graph', graph)      # (PyG's SAGEConv drops the values of adj_t)
        scale = inv_indeg(graph) if mode == 'SAGE' else None
        y, _, _ = sage_layer_raw(graph, x, W_n, W_s, bias, scale, relu, p, seed, False, False, fused)
        ctx.graph, ctx.scale, ctx.relu, ctx.p, ctx.fused, ctx.has_bias = graph, scale, relu, p, fused, bias is not None
        ctx.save_for_backward(x, W_n, W_s, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import gemm
        x, W_n, W_s, y = ctx.saved_tensors
        need_b = ctx.has_bias and ctx.needs_input_grad[4]
        dy = _c(dy)
        keep = 1.0 / (1.0 - ctx.p) if ctx.p else 1.0
        if ctx.relu:
            rs = torch.full((dy.shape[0],), keep, dtype=torch.float32, device=dy.device) if ctx.p else None
            G, db = act_bwd(dy, y, rs, want_out=True, want_colsum=need_b)
            if db is not None and ctx.p:
                db = db * keep
        else:
            G, db = dy, (act_bwd(dy, None, None, want_out=False, want_colsum=True)[1] if need_b else None)
        dx, R, _ = sage_layer_raw(ctx.graph, G, W_n, W_s, None, ctx.scale, False, 0.0, 0, True, True, ctx.fused)
        dWn = gemm.mm_tn(R, x) if ctx.needs_input_grad[2] else None
        dWs = gemm.mm_tn(G, x) if (W_s is not None and ctx.needs_input_grad[3]) else None
        return None, (dx if ctx.needs_input_grad[1] else None), dWn, dWs, db, None, None, None, None, None


def sage_layer(graph, x, W_n, W_s=None, bias=None, mode='SAGE', relu=False, p=0.0, seed=None, fused=None):
    """One layer of the SAGE / WSAGE / GCN encoders with its autograd: act((s * (A X)) W_n^T + X W_s^T + b), A X the sum over the in-neighbours as the
    by-dst CSR lists them; mode 'SAGE': s = 1 / indeg (0 where indeg = 0), 'WSAGE': s = 1, 'GCN': s = 1 and no W_s.  relu: ReLU, then dropout p with
    ops.dropout's keep-mask for `seed` (None: next_seed()).  Weights are [out, in].  fused (None: tuning.T.sage_fused) asks for the one-kernel layer
    (256 -> 256 fp32 rows); other shapes and fused=False take the composed path — ops.sage_paths records which.
    graph may be a graph.WeightedAdj: 'WSAGE' and 'GCN' then aggregate with its values, agg[v] = sum over the in-edges e of w_e * x[u_e] (GraphConv /
    GCNConv(normalize=False) on an adj_t with values); 'SAGE' ignores them, bit for bit."""
    mode = str(mode).upper()
    if mode not in SAGE_MODES:
        raise ValueError(f'sage_layer: mode must be one of {SAGE_MODES}, got {mode!r}')
    _lib.require_device(x, W_n, W_s, bias)
    if (mode == 'GCN') != (W_s is None):
        raise ValueError('sage_layer: SAGE / WSAGE take a self weight W_s, GCN takes none')
    if x.dtype != torch.float32:
        raise TypeError('sage_layer expects float32 rows')
    p = float(p) if relu else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f'sage_layer: 0 <= p < 1 expected, got {p}')
    if p and seed is None:
        seed = next_seed()
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return _SageLayerFn.apply(graph, x, W_n, W_s, bias, mode, bool(relu), p, int(seed or 0), fused)


ADJ_NORMALIZATIONS = ('gcn', 'adj')


def adj_normalize(adj, kind):
    """The reference's two normalisations of an adjacency with values (Link_prediction_model/utils.py:93-106) as a new graph.WeightedAdj:
    'adj': D^-1 A — deg = row sums, f = 1 / deg (inf -> 0), w' = f[v] * w;
    'gcn': D^-1/2 (A with its diagonal set to 1) D^-1/2 — torch_sparse's set_diag first (every stored (v, v) dropped, one (v, v) of value 1 per node: a new
           CSRGraph, built with torch and the ingest), then deg = row sums, dis = deg^-1/2 (inf -> 0), w' = (dis[v] * w) * dis[u].  A negative row sum raises.
    Rows are destinations (adj_t).  deg: float64 sum rounded once to fp32; the factor in float64 from that fp32, rounded once (csrc/cb_adjnorm.hip).  The
    result carries .deg and .factor.  Runs once per graph; one host read (the status word)."""
    from .graph import CSRGraph, WeightedAdj
    lib = _lib.load()
    if kind not in ADJ_NORMALIZATIONS:
        raise ValueError(f'adj_normalize: kind must be one of {ADJ_NORMALIZATIONS}, got {kind!r}')
    if not isinstance(adj, WeightedAdj):
        raise TypeError('adj_normalize expects a graph.WeightedAdj (graph.WeightedAdj.from_edges(edge_index, edge_weight, num_nodes))')
    g, w = adj.graph, adj.edge_weight
    if kind == 'gcn':
        ei = g._ei
        keep = ei[0] != ei[1]
        diag = torch.arange(g.N, dtype=torch.int64, device=g.device)
        ei = torch.cat([ei[:, keep], torch.stack([diag, diag])], dim=1)
        w = torch.cat([w[keep], torch.ones(g.N, dtype=torch.float32, device=g.device)])
        g = CSRGraph(ei, g.N, hub_threshold=g.hub_threshold, keep_edge_order=True)
    val = w[g.edge_perm(False)].contiguous()
    deg = torch.empty(g.N, dtype=torch.float32, device=g.device)
    fac = torch.empty(g.N, dtype=torch.float32, device=g.device)
    out = torch.empty(g.E, dtype=torch.float32, device=g.device)
    status = torch.zeros(1, dtype=torch.int32, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(lib.cb_adjnorm_rowsum_f64(_lib.ptr(g.rowptr), _lib.ptr(val), g.N, g.E, int(kind == 'gcn'), _lib.ptr(deg), _lib.ptr(fac), _lib.ptr(status),
                                             _lib.stream_ptr()), 'cb_adjnorm_rowsum_f64')
        _lib.check(lib.cb_adjnorm_scale_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(val), g.N, g.E, _lib.ptr(fac), _lib.ptr(fac if kind == 'gcn' else None),
                                            _lib.ptr(out), _lib.stream_ptr()), 'cb_adjnorm_scale_f32')
    bad = int(status.item())
    if bad:
        raise ValueError(f'adj_normalize: {bad} rows have a negative sum of values: deg^-1/2 is undefined there')
    res = WeightedAdj.from_csr_values(g, out)
    res.deg, res.factor = deg, fac
    return res


# ---------------------------------------------------------------------------------------------
# attention over the rows of the CSR: PyG TransformerConv(heads=1) (Link_prediction_model/layer.py:77-83; csrc/cb_attn.hip)
# ---------------------------------------------------------------------------------------------
ATTN_MAX_D = 512


def _attn_rows(who, d, **named):
    """Every operand an fp32 [N, d] matrix whose rows the kernels can take (cb_attn_supported); ValueError naming the constraint otherwise."""
    lib = _lib.load()
    for name, t in named.items():
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != d:
            raise ValueError(f'{who}: {name} must be a float32 [N, {d}] matrix, got {t.dtype} {tuple(t.shape)}')
        if not lib.cb_attn_supported(d, _lib.ptr(t), t.stride(0)) or (d > 1 and t.stride(1) != 1):
            raise ValueError(f'{who}: {name}: rows of D = {d} floats at stride {t.stride(0)} are not built: D % 4 == 0, D <= {ATTN_MAX_D}, 16-byte aligned rows '
                             f'with contiguous elements and a row stride that is a multiple of 4 and >= D are required')


def _attn_graph(who, graph, n):
    from .graph import CSRGraph
    if not isinstance(graph, CSRGraph) or graph.n_cols != graph.N or graph.N != n:
        raise ValueError(f'{who}: the whole square graph on this device (a graph.CSRGraph over the {n} rows) is required')


def _attn_view(graph, d, transpose, use_flags):
    """The view of one orientation with the workspace of the attention kernels' hub partials: 2 d + 4 floats per chunk (cb_attn_workspace_bytes), which is
    what the aggregation's view holds for rows of 2 d + 4 elements — also the bytes of the K | V pair a gather brings in, for the hot-row count."""
    view = graph._view(2 * d + 4, transpose, use_flags=use_flags)
    assert view.ws_bytes >= _lib.load().cb_attn_workspace_bytes(view.n_chunks, d)
    return view


def attn_raw(graph, q, k, v, skip, relu=False, want_lse=True, use_flags=True):
    """(out, lse): out[v] = act(sum_j a_j V[u_j] + skip[v]) with a = the softmax of <Q[v], K[u_j]> / sqrt(D) over the in-edges of v as the by-dst CSR lists
    them (each copy of a duplicate edge its own term; a row without in-edges gives act(skip[v]) and lse = -inf), lse[v] = log sum_j exp(s_j) as fp32 [N]
    (None with want_lse=False: evaluation).  The operands are fp32 [N, D] matrices or column slices of a wider one.  No autograd."""
    lib = _lib.load()
    _lib.require_device(q, k, v, skip)
    d = q.shape[1] if q.dim() == 2 else -1
    _attn_rows('attn_raw', d, q=q, k=k, v=v, skip=skip)
    _attn_graph('attn_raw', graph, q.shape[0])
    n = graph.N
    out = torch.empty((n, d), dtype=torch.float32, device=q.device)
    lse = torch.empty(n, dtype=torch.float32, device=q.device) if want_lse else None
    view = _attn_view(graph, d, False, use_flags)
    with torch.cuda.device(q.device):
        _lib.check(lib.cb_attn_fwd_f32(ctypes.byref(view), d, _lib.ptr(q), q.stride(0), _lib.ptr(k), k.stride(0), _lib.ptr(v), v.stride(0), _lib.ptr(skip),
                                       skip.stride(0), int(bool(relu)), _lib.ptr(out), out.stride(0), _lib.ptr(lse), _lib.stream_ptr()), 'cb_attn_fwd_f32')
    return out, lse


def attn_bwd_raw(graph, q, k, v, dout, lse, dq, dk, dv, use_flags=True, parts=('dst', 'src'), delta_in=None):
    """The gradients of attn_raw's sum with respect to Q, K, V written into dq, dk, dv (fp32 [N, D], column slices allowed) from dout = the gradient of
    the sum (the ReLU mask already applied; the skip's gradient is dout itself).  Returns delta [N].  Needs both orientations of the graph.
    parts / delta_in (tools/bench_attn.py): one of the two kernels alone — 'dst' writes dq and delta, 'src' reads delta_in and writes dk, dv."""
    lib = _lib.load()
    _lib.require_device(q, k, v, dout, lse, dq, dk, dv)
    d = q.shape[1] if q.dim() == 2 else -1
    _attn_rows('attn_bwd_raw', d, q=q, k=k, v=v, dout=dout, dq=dq, dk=dk, dv=dv)
    _attn_graph('attn_bwd_raw', graph, q.shape[0])
    if graph.rowptr_t is None:
        raise ValueError('attn_bwd_raw: this graph holds the forward orientation only; the backward gathers along the reverse one')
    delta = torch.empty(graph.N, dtype=torch.float32, device=q.device)
    ops_ = (_lib.ptr(q), q.stride(0), _lib.ptr(k), k.stride(0), _lib.ptr(v), v.stride(0), _lib.ptr(dout), dout.stride(0), _lib.ptr(lse))
    with torch.cuda.device(q.device):
        if 'dst' in parts:
            view = _attn_view(graph, d, False, use_flags)
            _lib.check(lib.cb_attn_bwd_dst_f32(ctypes.byref(view), d, *ops_, _lib.ptr(dq), dq.stride(0), _lib.ptr(delta), _lib.stream_ptr()),
                       'cb_attn_bwd_dst_f32')
        elif delta_in is not None:
            delta = delta_in
        if 'src' in parts:
            view = _attn_view(graph, d, True, use_flags)
            _lib.check(lib.cb_attn_bwd_src_f32(ctypes.byref(view), d, *ops_, _lib.ptr(delta), _lib.ptr(dk), dk.stride(0), _lib.ptr(dv), dv.stride(0),
                                               _lib.stream_ptr()), 'cb_attn_bwd_src_f32')
    return delta


class _TransformerConvFn(torch.autograd.Function):
    """P = X [W_q ; W_k ; W_v ; W_s]^T + [b_q ; b_k ; b_v ; b_s] = [Q | K | V | S], one GEMM; Y = act(attention(Q, K, V) + S), one kernel.  Saved: X, P, lse and,
    under the ReLU, Y (its mask).  Backward: dO = dY * 1[Y > 0]; the two attention kernels fill [dQ | dK | dV] of one [N, 4 D] matrix whose last block is
    dS = dO; dX = dP W, dW = dP^T X and db = colsum(dP), each one GEMM / one pass over dP, split back to the eight parameters."""

    @staticmethod
    def forward(ctx, graph, x, W, b, relu):
        from . import gemm
        d = W.shape[0] // 4
        P = gemm.mm_nn(x, W.t().contiguous(), bias=b)
        y, lse = attn_raw(graph, P[:, :d], P[:, d:2 * d], P[:, 2 * d:3 * d], P[:, 3 * d:], relu=relu, want_lse=True)
        ctx.graph, ctx.relu, ctx.d = graph, relu, d
        ctx.save_for_backward(x, W, P, lse, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import gemm
        x, W, P, lse, y = ctx.saved_tensors
        d, graph = ctx.d, ctx.graph
        if graph.rowptr_t is None:
            raise ValueError('transformer_conv: this graph holds the forward orientation only; the backward gathers along the reverse one')
        dy = _c(dy)
        dP = torch.empty_like(P)
        dS = dP[:, 3 * d:]
        if ctx.relu:
            dS.copy_(act_bwd(dy, y, None, want_out=True, want_colsum=False)[0])
        else:
            dS.copy_(dy)
        attn_bwd_raw(graph, P[:, :d], P[:, d:2 * d], P[:, 2 * d:3 * d], dS, lse, dP[:, :d], dP[:, d:2 * d], dP[:, 2 * d:3 * d])
        dx = gemm.mm_nn(dP, W) if ctx.needs_input_grad[1] else None          # [N, 4D] @ [4D, in]
        dW = gemm.mm_tn(dP, x) if ctx.needs_input_grad[2] else None          # [4D, in]
        db = act_bwd(dP, None, None, want_out=False, want_colsum=True)[1] if ctx.needs_input_grad[3] else None
        return None, dx, dW, db, None


def transformer_conv(graph, x, W_key, b_key, W_query, b_query, W_value, b_value, W_skip, b_skip, relu=False):
    """One PyG TransformerConv(in, out) layer with every default (heads = 1, concat, no beta, no edge features, no attention dropout, bias, root weight) and
    its autograd: with Q, K, V, S = the four Linears of x (weights [out, in]),  out[v] = act(sum_j softmax_j(<Q[v], K[u_j]> / sqrt(out)) V[u_j] + S[v])  over
    the in-edges of v as the by-dst CSR lists them.  Deviation from PyG: its 1e-16 in the softmax's denominator is dropped (the maximum is subtracted, the
    denominator is >= 1, the addition is invisible in fp32).  The backward needs both orientations of the graph."""
    params = (W_query, b_query, W_key, b_key, W_value, b_value, W_skip, b_skip)      # stacked as [Q | K | V | S]: K and V of a row adjacent
    _lib.require_device(x, *params)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError('transformer_conv expects float32 rows')
    d = W_query.shape[0]
    for w, b in zip(params[0::2], params[1::2]):
        if tuple(w.shape) != (d, x.shape[1]) or tuple(b.shape) != (d,) or w.dtype != torch.float32 or b.dtype != torch.float32:
            raise ValueError(f'transformer_conv: four float32 [out, in] = [{d}, {x.shape[1]}] weights with [{d}] biases expected')
    if d % 4 or d > ATTN_MAX_D:
        raise ValueError(f'transformer_conv: out_channels = {d} is not built: D % 4 == 0 and D <= {ATTN_MAX_D} are required')
    _attn_graph('transformer_conv', graph, x.shape[0])
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return _TransformerConvFn.apply(graph, x, torch.cat(params[0::2]), torch.cat(params[1::2]), bool(relu))


# ---------------------------------------------------------------------------------------------
# the link-prediction experiment's samplers, epoch shuffle and ranking metrics: Link_prediction_model/negative_sample.py:5-57; model.py:121-266;
# utils.py:568-586; Link_prediction_model/utils.py:61-91  (cb_lpx.hip)
# ---------------------------------------------------------------------------------------------
def _seed64(seed):
    return ctypes.c_uint64((next_seed() if seed is None else int(seed)) % 2 ** 64)


def seeded_permutation(n, seed=None, device=None):
    """int32 [n]: the permutation of range(n) that sorts the keys (first Philox word of draw i) << 32 | i — a pure function of (n, seed), restated in
    tests/lpx_ref.py.  The epoch shuffle of the link-prediction experiment (where the reference's DataLoader draws a host randperm) and the copies of
    `sample_perm_copy`.  n < 2^31."""
    n = int(n)
    if n < 0:
        raise ValueError('seeded_permutation: n >= 0 required')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise _lib.HipExtensionError('seeded_permutation draws on an MI355X device; there is no CPU fallback')
    lib = _lib.load()
    seed = _seed64(seed)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return perm
    wsb = lib.cb_lpx_permutation_workspace_bytes(n)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cb_lpx_permutation_i32(n, seed, _lib.ptr(perm), _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_lpx_permutation_i32')
    return perm


def local_negatives(pos, num_nodes, num_neg, seed=None):
    """int32 [2, P * num_neg] of `local_neg_sample(random_src=False)` (negative_sample.py:28-40): column i * num_neg + j = (pos[0, i], a uniform node of
    [0, num_nodes)), no rejection.  pos: int32 / int64 [2, P] on the device."""
    if not torch.is_tensor(pos):
        raise ValueError('local_negatives: pos must be an int32 / int64 [2, P] tensor')
    _lib.require_device(pos)
    p32 = _pairs_arg('local_negatives: pos', pos, pos.device)
    P, num_neg = NegativeSampler._count('local', p32.shape[1], num_neg)
    seed = _seed64(seed)
    out = torch.empty((2, P * num_neg), dtype=torch.int32, device=p32.device)
    with torch.cuda.device(p32.device):
        _lib.check(_lib.load().cb_lpx_neg_local_i32(_lib.ptr(p32), P, num_neg, int(num_nodes), seed, _lib.ptr(out), _lib.stream_ptr()),
                   'cb_lpx_neg_local_i32')
    return out


def perm_copies(base, num_copies, seed):
    """[2, n * num_copies] from base [2, n] (`sample_perm_copy`, negative_sample.py:50-57): copy 0 = base, copy j >= 1 = base permuted by
    seeded_permutation(n, seed + j); column i * num_copies + j = copy j's column i = base column perm_j[i]."""
    _lib.require_device(base)
    n, k = int(base.shape[1]), int(num_copies)
    if k < 0:
        raise ValueError('perm_copies: num_copies >= 0 required')
    if k == 0:
        return base[:, :0].contiguous()
    if k == 1:
        return base
    cols = [torch.arange(n, dtype=torch.int32, device=base.device)] + [seeded_permutation(n, int(seed) + j, base.device) for j in range(1, k)]
    return base[:, torch.stack(cols, dim=1).reshape(-1).long()].contiguous()


class NegativeSampler:
    """The negative samplers of Link_prediction_model/negative_sample.py on the device CSR.  Every method returns int32 [2, S], S = num_samples *
    num_neg, row 0 = source, row 1 = destination; column i * num_neg + j is negative j of positive i (the reference's [num_samples, num_neg, 2] is
    `out.t().view(num_samples, num_neg, 2)`).  Every draw is a pure function of (seed, slot, try), restated in tests/lpx_ref.py.
      global_       `global_neg_sample`: uniform pairs (u, v), u != v, u -> v not an edge of the graph (the directed pair only, as PyG's negative_sampling
                    tests it after add_self_loops).  Deviation: the reference asks PyG for the count and pads a short result with repeats; here every
                    slot tries up to 64 times, and a slot that found nothing holds -1 and counts in `failed` (check()).
      local         `local_neg_sample(random_src=False)`: the positive's source with a uniform destination, no rejection.
      global_perm   `global_perm_neg_sample`: copy 0 = global_(num_samples, 1, seed); copy j >= 1 = copy 0 permuted by
                    seeded_permutation(num_samples, seed + j)."""

    def __init__(self, graph):
        from .graph import CSRGraph
        if type(graph) is not CSRGraph or graph.n_cols != graph.N or graph.row_offset != 0:
            raise ValueError('NegativeSampler needs a whole square graph.CSRGraph (segmented and node-sharded graphs are out of scope)')
        _lib.require_device(graph.rowptr, graph.col)
        self._lib = _lib.load()
        self.graph = graph
        self.failed = torch.zeros(1, dtype=torch.int32, device=graph.device)

    @staticmethod
    def _count(who, num_samples, num_neg):
        num_samples, num_neg = int(num_samples), int(num_neg)
        if num_samples < 0 or num_neg < 0:
            raise ValueError(f'NegativeSampler.{who}: num_samples >= 0 and num_neg >= 0 required')
        return num_samples, num_neg

    def global_(self, num_samples, num_neg, seed=None):
        num_samples, num_neg = self._count('global_', num_samples, num_neg)
        g, S = self.graph, num_samples * num_neg
        seed = _seed64(seed)
        out = torch.empty((2, S), dtype=torch.int32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(self._lib.cb_lpx_neg_global_i32(ctypes.byref(_linkp_view(g)), S, seed, _lib.ptr(out), _lib.ptr(self.failed), _lib.stream_ptr()),
                       'cb_lpx_neg_global_i32')
        return out

    def local(self, pos, num_neg, seed=None):
        """pos: int32 / int64 [2, P] positives (row 0 = source) on the graph's device."""
        if not torch.is_tensor(pos) or pos.device != self.graph.device:
            _lib.require_device(pos)
            raise ValueError('NegativeSampler.local: pos must live on the device of the graph')
        return local_negatives(pos, self.graph.N, num_neg, seed)

    def global_perm(self, num_samples, num_neg, seed=None):
        num_samples, num_neg = self._count('global_perm', num_samples, num_neg)
        seed = next_seed() if seed is None else int(seed)
        return perm_copies(self.global_(num_samples, 1, seed), num_neg, seed)

    def check(self):
        """Reads the counter of failed slots (a host synchronisation: call it where the loss is read anyway), clears it, and raises RuntimeError if a
        slot of the draws since the last check found no non-edge in its tries."""
        n = int(self.failed.item())
        if n:
            self.failed.zero_()
            raise RuntimeError(f'NegativeSampler: {n} negative slot(s) found no non-edge in {int(self._lib.cb_lpx_max_tries())} tries (their columns hold -1)')


def row_rank_counts(pos, neg2d, return_status=False):
    """(gt, eq) int32 [P] for pos [P] and neg2d [P, K] (rows may be strided, elements contiguous): gt[i] = #{j : neg2d[i, j] > pos[i]},
    eq[i] = #{j : neg2d[i, j] == pos[i]}; -0.0 equals +0.0, +-inf compare as numbers.  A NaN in pos[i] or in row i gives gt[i] = eq[i] = -1 and counts
    in the int32 [1] status (return_status); mrr_from_counts raises on it.  rank_counts() with each positive ranked among its own negatives."""
    _lib.require_device(pos, neg2d)
    if (not torch.is_tensor(pos) or not torch.is_tensor(neg2d) or pos.dtype != torch.float32 or neg2d.dtype != torch.float32 or pos.device != neg2d.device
            or pos.dim() != 1 or neg2d.dim() != 2 or neg2d.shape[0] != pos.shape[0]):
        raise ValueError('row_rank_counts expects float32 pos [P] and neg [P, K] on one device')
    lib = _lib.load()
    ps = _c(pos.detach())
    ns = neg2d.detach()
    P, K = ns.shape
    if K > 1 and ns.stride(1) != 1 or (P > 1 and ns.stride(0) < K):
        ns = ns.contiguous()
    ld = ns.stride(0) if P > 1 else max(K, 1)
    dev = ps.device
    gt = torch.empty(P, dtype=torch.int32, device=dev)
    eq = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cb_lpx_row_ranks_f32(_lib.ptr(ps) if P else None, P, _lib.ptr(ns) if P * K else None, max(ld, K), K, _lib.ptr(gt) if P else None,
                                            _lib.ptr(eq) if P else None, _lib.ptr(status), _lib.stream_ptr()), 'cb_lpx_row_ranks_f32')
    return (gt, eq, status) if return_status else (gt, eq)


def mrr_from_counts(gt, eq, status=None):
    """The OGB evaluator's rule on counts: rank = 1 + gt + eq / 2 (the mean of the optimistic and the pessimistic rank); {'MRR': mean(1 / rank) in
    float64, 'hits@1' | 'hits@3' | 'hits@10': the share with rank <= K}.  Raises ValueError on a non-zero NaN status (given, or read off the -1 of
    the counts)."""
    if gt.numel() == 0:
        raise ValueError('the MRR is a mean over the positives: at least one is required')
    bad = int(status.item()) if status is not None else int((gt < 0).sum().item())
    if bad:
        raise ValueError(f'mrr_from_counts: {bad} NaN score(s) / row(s) with a NaN: a NaN has no rank')
    rank = 1.0 + gt.to(torch.float64) + eq.to(torch.float64) / 2
    out = {'MRR': float((1.0 / rank).mean().item())}
    for k in (1, 3, 10):
        out[f'hits@{k}'] = float((rank <= k).to(torch.float64).mean().item())
    return out


def recall_k(topk, P):
    """The cut of `cal_recall` (utils.py:569-574): None for 'the threshold 0' (topk None or 0), int(topk) above 5, else int(float(topk) * P)."""
    if topk is None or float(topk) == 0:
        return None
    return int(topk) if float(topk) > 5 else int(float(topk) * P)


def recall_numerator(pos, neg, k):
    """The integer numerator of `cal_recall` as an int64 [1] device tensor (-1 on a NaN) and the int32 [1] NaN status: the positives among the first
    min(k, |M|) of M = {pos > 0} + neg by descending score, positives first among equals.  k None: all of M (= #{pos > 0})."""
    _lib.require_device(pos, neg)
    if not torch.is_tensor(pos) or not torch.is_tensor(neg) or pos.dtype != torch.float32 or neg.dtype != torch.float32 or pos.device != neg.device:
        raise ValueError('recall_at_topk expects float32 scores on one device')
    lib = _lib.load()
    ps, ns = _c(pos.detach().reshape(-1)), _c(neg.detach().reshape(-1))
    P, Nn, dev = ps.numel(), ns.numel(), ps.device
    k = P + Nn if k is None else int(k)
    if k < 0:
        raise ValueError('recall_at_topk: the cut must not be negative')
    result = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = lib.cb_lpx_recall_topk_workspace_bytes(P, Nn)
    ws = _ws(wsb, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cb_lpx_recall_topk_f32(_lib.ptr(ps) if P else None, P, _lib.ptr(ns) if Nn else None, Nn, k, _lib.ptr(result), _lib.ptr(status),
                                              _lib.ptr(ws), wsb, _lib.stream_ptr()), 'cb_lpx_recall_topk_f32')
    return result, status


def recall_at_topk(pos, neg, topk):
    """`cal_recall` (utils.py:568-586) as a Python float: numerator / P with P counted before the `> 0` filter.  topk None or 0: mean(pos > 0);
    float(topk) > 5: k = int(topk); otherwise k = int(float(topk) * P).  Where the reference's host sort leaves the order of equal scores to the
    order of its concatenation (positives first, a stable sort), the device order states it: a positive before a negative among equals.  An empty M
    (no positive above 0 and no negative) under a cut raises ValueError, as the reference's indexing of an empty array does; so does a NaN."""
    P = int(pos.numel())
    if P == 0:
        raise ValueError('recall_at_topk: at least one positive is required (the recall is a share of the positives)')
    k = recall_k(topk, P)
    result, status = recall_numerator(pos, neg, k)
    num = int(result.item())
    if num < 0:
        raise ValueError(f'recall_at_topk: {int(status.item())} NaN score(s): a NaN has no rank')
    if k is not None and neg.numel() == 0:
        m, _ = recall_numerator(pos, neg, None)
        if int(m.item()) == 0:
            raise ValueError('recall_at_topk: no positive above 0 and no negative: nothing to rank')
    return num / P
