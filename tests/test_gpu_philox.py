"""GPU: every kernel that draws a dropout keep-mask against the HOST restatement of Philox4x32-10 (oracle/coldbrew_oracle.py dropout_keep_mask, itself
pinned to Random123's known answers in tests/test_philox_host.py) — bit for bit, no tolerances.

(a) cb_dropout_f32 over sizes, offsets up to 2^40, seeds up to 2^62, thresholds, the scalar branch, the backward and the device seed word.
(b) every fused site at flat indices the rest of the suite never reaches: `row0` / `offset` are parameters, so a few hundred rows placed at
    row0 = ceil(B / width) - 3 straddle B = 2^31, 2^32 and 2^34 (the first rows below B, the rest above); one case with a seed above 2^32 at row0 = 0
    and one with the device seed word carrying into the high key word.

Where the arithmetic around the mask is reproduced elsewhere bit for bit (GEMMs with operand dropout = the plain GEMM on the masked operand; the
stores = the ReLU output they also write, a mix with power-of-two factors, then the mask) the inputs are arbitrary reals and p = 0.3.  The backward kernels mix several masked gradients;
there the inputs are small integers, the factors powers of two and p = 0.5, so every product and sum is exact in fp32 and the float64 formula on the
host masks must be met bit for bit whatever the order of the kernel's sums.  ReLUs see strictly positive values and backward kernels all-ones mask
words, so every element shows its mask bit.

`row0` enters index arithmetic only, at every entry point (mask words, row scales and mix rows are addressed by the local / node row), so no site limits it.

Call sites of keep4 (csrc/) and the test that reaches each:
  cb_elementwise.hip  k_dropout, aligned quad / straddling quad       test_dropout_equals_the_host_mask (offsets with offset & 3 == 0 / != 0), _scalar_branch_,
                                                                      _backward_, _adds_the_device_seed_word; two-kernel cases of test_gemm_output_dropout
  cb_trunk_bwd.hip    k_trunk_bwd seed / seed2                        test_layer_backward_draws_both_host_masks, _on_compact_rows_ (RIDX), test_single_operand_input_backward_ (MODE 1)
                      k_trunk_bwd_fold seed / fo.seed[q]              test_layer_backward_fold_draws_three_host_masks
                      k_trunk_input_bwd_multi seed / mt.seed[l]       test_input_backward_draws_four_host_masks
                      k_trunk_store_rows                              test_store_rows_draws_the_host_mask
  cb_gemm_core.h      nn_epilogue EPI == 1 (dual output)              test_gemm_output_dropout (fused shapes), test_gemm_input_and_output_dropout
                      nn_epilogue EPI == 2 (row subset)               test_gemm_store_rows_draws_the_host_mask
  cb_limb_core.h      RowOperand (A of an NN product)                 test_gemm_input_and_output_dropout, test_gemm_input_dropout
                      ColOperand (A or G of a TN product, x of the    test_weight_gradient_with_dropout_of_the_a_operand / _g_operand (all three tiles),
                      instage form)                                   test_instage_weight_gradient_draws_both_host_masks
                      ColOperandInStage (g of the instage form)       test_instage_weight_gradient_draws_both_host_masks
  cb_front.hip        x (P0) and X0 (P3)                              test_trunk_front_draws_both_host_masks (K = 64 and 128)
  cb_spmm_core.h      fused_store forward                             test_aggregation_store_draws_the_host_mask (row and hub kernels), _on_a_row_subset_,
                                                                      test_aggregation_store_with_gemm_tail_draws_the_host_mask (plain and head form)
                      fused_store bwd                                 test_reverse_aggregation_store_backward_draws_the_host_masks[None]
                      fused_store_bwd_mix seed / mx_seed[q]           test_reverse_aggregation_store_backward_draws_the_host_masks[0 / 2]
  cb_agg_gemm.hip     store on the node rows row_ids                  test_aggregation_gemm_store_rows_draws_the_host_mask
  cb_mlp.hip          keep4_flat, aligned / straddling                test_ln_gelu_dropout_zero_pattern_is_the_host_mask (forward; backward through dbeta at one row)"""
import ctypes
import functools

import pytest
import torch

import coldbrew_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# name -> (B, host seed, device seed word): row0 = ceil(B / width) - 3, or 0 / 5 without B
CASES = {'B31': (2 ** 31, 1234567, None), 'B32': (2 ** 32, 2 ** 62 - 1, None), 'B34': (2 ** 34, 0x1234ABCD5, None),
         'seed_hi': (0, 2 ** 40 + 12345, None), 'seed_dev': (0, 0x1234ABCD5, 2 ** 32 - 1)}
ONE_WIDTH = [(c, 0) for c in CASES]
TWO_WIDTHS = ONE_WIDTH + [(c, 1) for c in CASES if CASES[c][0]]      # (the second width moves row0 only where B is set)


def _case(name, width, monkeypatch):
    """(row0, seed, device seed word) of a case for a mask of row width `width`; installs the device seed word."""
    from gnn_tail_generalization_amd import ops
    B, seed, sd = CASES[name]
    row0 = -(-B // width) - 3 if B else (5 if sd else 0)
    if sd:
        monkeypatch.setattr(ops, '_graph_seed', torch.tensor([sd], dtype=torch.int64, device=DEV))
    if B:
        assert row0 * width < B < (row0 + 4) * width
    return row0, seed, sd or 0


@functools.lru_cache(maxsize=16)
def _keep_np(shape, p, seed, offset, seed_dev):
    return orc.dropout_keep_mask(shape, p, seed, offset=offset, seed_dev=seed_dev)


def _keep(shape, p, seed, offset=0, seed_dev=0):
    """The host keep-mask as a bool device tensor."""
    return torch.from_numpy(_keep_np(tuple(shape), float(p), int(seed), int(offset), int(seed_dev))).to(DEV)


def _keep_rows(idx, n_nodes, width, p, seed, row0, seed_dev=0):
    """Rows idx of the host mask of the [n_nodes, width] matrix whose row 0 is global row row0."""
    return _keep((n_nodes, width), p, seed, row0 * width, seed_dev)[idx]


def _drop(x, keep, p):
    """where(keep, x * scale, 0) in float32: the one rounded product the kernels form."""
    return torch.where(keep, x * float(orc.dropout_scale(p)), torch.zeros((), device=x.device))


def _mask_words(active):
    """[rows, 256 t] bool -> int64 [rows, t, 4]: word k of tile j, bit l <-> column 256 j + 4 l + k (the layout of the fused stores' mask words)."""
    rows, d = active.shape
    a = active.view(rows, d // 256, 64, 4).permute(0, 1, 3, 2).to(torch.int64)
    w = (a << torch.arange(64, device=active.device, dtype=torch.int64)).sum(-1)      # bit 63 wraps into the sign: the same 64 bits
    return w.contiguous()


def _ones_words(rows, tiles=1):
    return torch.full((rows, tiles, 4), -1, dtype=torch.int64, device=DEV)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _pos(gen, *shape, lo=0.25):
    return torch.rand(*shape, device=DEV, generator=gen) + lo


def _ints(gen, lo, hi, *shape, nonzero=False):
    t = torch.randint(lo, hi + 1, shape, device=DEV, generator=gen)
    if nonzero:
        t = torch.where(t == 0, torch.full_like(t, hi), t)
    return t.float()


def _pow2(gen, n):
    return torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 3, (n,), device=DEV, generator=gen)].contiguous()


def _status_ok():
    from gnn_tail_generalization_amd import _lib
    torch.cuda.synchronize()
    assert _lib.load().cb_device_status() == 0


# ---------------------------------------------------------------------------------------------
# (a) cb_dropout_f32
# ---------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 1023, 4099, 4096 * 37 + 5]
OFFSETS = [0, 1, 2, 3, 2 ** 31 - 3, 2 ** 32 - 2, 2 ** 34 - 5, 2 ** 34 + 1, 2 ** 40 + 3]
SEEDS = [0, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 62 - 1]
PS = [2.4e-10, 0.1, 0.5, 0.999]


def _dropout_grid():
    """Every (size, offset) pair; seeds and thresholds cycle so that every value of either meets every offset's alignment class and every size."""
    return [(n, off, SEEDS[(i + j) % len(SEEDS)], PS[(i + 3 * j) % len(PS)]) for j, off in enumerate(OFFSETS) for i, n in enumerate(SIZES)]


def test_dropout_grid_keeps_every_value_of_every_axis():
    grid = _dropout_grid()
    for axis, values in enumerate((SIZES, OFFSETS, SEEDS, PS)):
        assert {g[axis] for g in grid} == set(values)
    for n in SIZES:      # every size meets every seed's high / low word pattern and every threshold
        assert {g[3] for g in grid if g[0] == n} == set(PS) and len({g[2] for g in grid if g[0] == n}) >= 4


@pytest.mark.parametrize('offset', OFFSETS)
def test_dropout_equals_the_host_mask(offset):
    from gnn_tail_generalization_amd import ops
    for n, off, seed, p in _dropout_grid():
        if off != offset:
            continue
        x = (torch.rand(n, generator=torch.Generator().manual_seed(n)) + 0.5).to(DEV)
        keep = _keep((n,), p, seed, off)
        y = ops._dropout_raw(x, p, seed, off)
        assert torch.equal(y, _drop(x, keep, p)), (n, off, seed, p)
        assert torch.equal(y != 0, keep), (n, off, seed, p)
        assert torch.equal(ops.dropout_keep_mask((n,), p, seed, DEV, offset=off), keep)


@pytest.mark.parametrize('n', [5, 4099])
@pytest.mark.parametrize('mis_src,mis_dst', [(1, 0), (0, 1), (1, 1)])
def test_dropout_scalar_branch_on_misaligned_buffers(n, mis_src, mis_dst):
    """A source or destination that starts one float past a 16-byte boundary: no float4 access (vec_ok = 0)."""
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    p, seed, off = 0.3, 2 ** 32 + 1, 2 ** 34 - 5
    buf = (torch.rand(n + 8, generator=torch.Generator().manual_seed(n)) + 0.5).to(DEV)
    out = torch.full((n + 8,), -1.0, device=DEV)
    x, y = buf[mis_src:mis_src + n], out[mis_dst:mis_dst + n]
    assert x.data_ptr() % 16 == 4 * mis_src and y.data_ptr() % 16 == 4 * mis_dst
    with torch.cuda.device(DEV):
        _lib.check(lib.cb_dropout_f32(_lib.ptr(x), _lib.ptr(y), n, float(p), ctypes.c_uint64(seed), None, off, _lib.stream_ptr()), 'cb_dropout_f32')
    assert torch.equal(y, _drop(x, _keep((n,), p, seed, off), p))
    assert bool((out[:mis_dst] == -1).all()) and bool((out[mis_dst + n:] == -1).all())      # nothing written outside [0, n)


@pytest.mark.parametrize('offset', [0, 3, 2 ** 34 + 1])
def test_dropout_backward_draws_the_same_host_mask(offset):
    from gnn_tail_generalization_amd import ops
    n, p, seed = 4099, 0.1, 2 ** 62 - 1
    x = (torch.rand(n, generator=torch.Generator().manual_seed(1)) + 0.5).to(DEV).requires_grad_(True)
    g = (torch.rand(n, generator=torch.Generator().manual_seed(2)) + 0.5).to(DEV)
    keep = _keep((n,), p, seed, offset)
    y = ops.dropout(x, p, True, seed=seed, offset=offset)
    y.backward(g)
    assert torch.equal(y.detach(), _drop(x.detach(), keep, p)) and torch.equal(x.grad, _drop(g, keep, p))


@pytest.mark.parametrize('seed_dev', [987654321, 2 ** 32 - 1])
@pytest.mark.parametrize('n,offset', [(4099, 0), (1023, 2 ** 34 - 5)])
def test_dropout_adds_the_device_seed_word(seed_dev, n, offset, monkeypatch):
    """hipGraph mode: the kernel adds *seed_dev to the host seed; 2^32 - 1 on an odd host seed carries into the high key word."""
    from gnn_tail_generalization_amd import ops
    p, seed = 0.5, 0x1234ABCD5
    assert seed & 1 and ((seed & 0xFFFFFFFF) + seed_dev >= 2 ** 32) == (seed_dev == 2 ** 32 - 1)
    x = (torch.rand(n, generator=torch.Generator().manual_seed(n)) + 0.5).to(DEV)
    plain = ops._dropout_raw(x, p, seed, offset)
    monkeypatch.setattr(ops, '_graph_seed', torch.tensor([seed_dev], dtype=torch.int64, device=DEV))
    y = ops._dropout_raw(x, p, seed, offset)
    assert torch.equal(y, _drop(x, _keep((n,), p, seed, offset, seed_dev), p))
    assert torch.equal(y, _drop(x, _keep((n,), p, seed + seed_dev, offset), p))
    assert not torch.equal(y, plain)


# ---------------------------------------------------------------------------------------------
# (b) GEMM epilogue and operand dropout
# ---------------------------------------------------------------------------------------------
def _dual_form(a, b, M, N, K):
    """The dual-output / operand-dropout form of the three-limb kernel exists for this shape (cb_gemm_nn_indrop_supported: its predicate + K % 4 == 0)."""
    from gnn_tail_generalization_amd import _lib
    y = torch.empty((M, N), dtype=torch.float32, device=DEV)
    return bool(_lib.load().cb_gemm_nn_indrop_supported(_lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0), _lib.ptr(y), N, _lib.ptr(y), N, M, N, K))


# 32641 rows = 256 tiles of 128 x 256, the fewest at which the dual-output epilogue is taken (ragged last tile); 16257 x 260: two column tiles, a width
# that is no power of two; below: cb_gemm_nn_f32 followed by cb_dropout_f32
@pytest.mark.parametrize('M,N,K,fused', [(32641, 256, 8, True), (16257, 260, 8, True), (301, 256, 8, False), (77, 36, 12, False)])
@pytest.mark.parametrize('case', list(CASES))
def test_gemm_output_dropout(M, N, K, fused, case, monkeypatch):
    from gnn_tail_generalization_amd import gemm
    p = 0.3
    row0, seed, sd = _case(case, N, monkeypatch)
    gen = _gen(M)
    a, b, bias = _pos(gen, M, K), _pos(gen, K, N), _pos(gen, N)
    assert _dual_form(a, b, M, N, K) == fused
    y, yd = gemm.mm_nn_drop2(a, b, p, seed, row0, bias=bias, relu=True)
    _status_ok()
    assert torch.equal(y, gemm.mm_nn(a, b, bias=bias, relu=True)) and bool((y > 0).all())
    keep = _keep((M, N), p, seed, row0 * N, sd)
    assert torch.equal(yd != 0, keep)
    assert torch.equal(yd, _drop(y, keep, p))


@pytest.mark.parametrize('case,wsel', TWO_WIDTHS)
def test_gemm_input_and_output_dropout(case, wsel, monkeypatch):
    """cb_gemm_nn_indrop_drop2_f32: A's mask while it is staged (K = 36: two whole K steps and a tail of four) and the output's in the epilogue."""
    from gnn_tail_generalization_amd import gemm
    M, K, N, p = 32641, 36, 256, 0.3
    row0, seed, sd = _case(case, (N, K)[wsel], monkeypatch)
    a_seed = seed ^ 0x5DEECE66D
    gen = _gen(11)
    a, b, bias = _pos(gen, M, K), _pos(gen, K, N), _pos(gen, N)
    res = gemm.mm_nn_indrop_drop2(a, b, p, a_seed, seed, row0, bias=bias, relu=True, want_bits=True)
    assert res is not None
    y, yd, bits = res
    _status_ok()
    a_d = _drop(a, _keep((M, K), p, a_seed, row0 * K, sd), p)
    assert torch.equal(y, gemm.mm_nn(a_d, b, bias=bias, relu=True)) and bool((y > 0).all())
    assert torch.equal(yd, _drop(y, _keep((M, N), p, seed, row0 * N, sd), p))
    assert bool((bits == -1).all())


@pytest.mark.parametrize('case', list(CASES))
def test_gemm_input_dropout(case, monkeypatch):
    from gnn_tail_generalization_amd import gemm
    M, K, N, p = 32641, 36, 256, 0.3
    row0, seed, sd = _case(case, K, monkeypatch)
    gen = _gen(12)
    a, b = torch.randn(M, K, device=DEV, generator=gen), torch.randn(K, N, device=DEV, generator=gen)
    rs, add, bias = _pos(gen, M), torch.randn(M, N, device=DEV, generator=gen), torch.randn(N, device=DEV, generator=gen)
    y = gemm.mm_nn_indrop(a, b, p, seed, row0, rowscale=rs, addend=add, bias=bias, relu=False)
    assert y is not None
    _status_ok()
    a_d = _drop(a, _keep((M, K), p, seed, row0 * K, sd), p)
    assert torch.equal(y, gemm.mm_nn(a_d, b, rowscale=rs, addend=add, bias=bias))


@pytest.mark.parametrize('case', list(CASES))
def test_weight_gradient_with_dropout_of_the_a_operand(case, monkeypatch):
    from gnn_tail_generalization_amd import gemm
    M, K1, K2, p = 1037, 132, 68, 0.3      # the 128 x 128 tile (the only one with this form), ragged in both directions, nine row slabs
    row0, seed, sd = _case(case, K1, monkeypatch)
    gen = _gen(13)
    a, g, rs = torch.randn(M, K1, device=DEV, generator=gen), torch.randn(M, K2, device=DEV, generator=gen), _pos(gen, M)
    out = gemm.mm_tn_adrop(a, g, p, seed, row0, rowscale=rs)
    assert out is not None
    _status_ok()
    assert torch.equal(out, gemm.mm_tn(_drop(a, _keep((M, K1), p, seed, row0 * K1, sd), p), g, rowscale=rs))


# one shape per tile of the TN contraction: 64 x 256 (K1 <= 64), 256 x 64 (K2 <= 64), 128 x 128
@pytest.mark.parametrize('K1,K2', [(36, 132), (132, 36), (132, 68)])
@pytest.mark.parametrize('case', list(CASES))
def test_weight_gradient_with_dropout_of_the_g_operand(K1, K2, case, monkeypatch):
    from gnn_tail_generalization_amd import gemm
    M, p = 1037, 0.3
    row0, seed, sd = _case(case, K2, monkeypatch)
    gen = _gen(14)
    a, g = torch.randn(M, K1, device=DEV, generator=gen), torch.randn(M, K2, device=DEV, generator=gen)
    out = gemm.mm_tn_gdrop(a, g, p, seed, row0)
    assert out is not None
    _status_ok()
    assert torch.equal(out, gemm.mm_tn(a, _drop(g, _keep((M, K2), p, seed, row0 * K2, sd), p)))


@pytest.mark.parametrize('case,wsel', TWO_WIDTHS)
def test_instage_weight_gradient_draws_both_host_masks(case, wsel, monkeypatch):
    """cb_gemm_tn_instage_f32: gy = (X0 > 0) * (dropout_bwd_{g_seed}(g) + mfold) and dropout_{x_seed}(x), both while they are staged.  32641 rows = 256 row
    slabs, the fewest the form exists for.  Integer operands, p = 0.5: every sum is exact (|.| < 2^24), so the float64 products of the host-masked operands
    are the answer bit for bit."""
    from gnn_tail_generalization_amd import gemm
    M, F, p = 32641, 100, 0.5
    row0, g_seed, sd = _case(case, (256, F)[wsel], monkeypatch)
    x_seed = g_seed ^ 0x5DEECE66D
    gen = _gen(15)
    g, mfold, x = _ints(gen, -3, 3, M, 256, nonzero=True), _ints(gen, -2, 2, M, 256), _ints(gen, 1, 3, M, F)
    assert gemm.mm_tn_instage_supported(g, x, M) and not gemm.mm_tn_instage_supported(g[:32640], x[:32640], 32640)
    dw, db = gemm.mm_tn_instage(g, mfold, _ones_words(M), x, p, g_seed, p, x_seed, row0)
    _status_ok()
    gy = 2.0 * g.double() * _keep((M, 256), p, g_seed, row0 * 256, sd) + mfold.double()
    xd = 2.0 * x.double() * _keep((M, F), p, x_seed, row0 * F, sd)
    want = gy.t() @ xd
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(dw.double(), want) and torch.equal(db.double(), gy.sum(0))
    assert torch.equal(dw, gemm.mm_tn(gy.float(), xd.float()))      # the plain contraction of the host-masked operands


@pytest.mark.parametrize('K', [64, 128])
@pytest.mark.parametrize('case,wsel', TWO_WIDTHS)
def test_trunk_front_draws_both_host_masks(K, case, wsel, monkeypatch):
    from gnn_tail_generalization_amd import gemm
    M, p = 64 * 5 + 7, 0.3
    row0, seed_x, sd = _case(case, (256, K)[wsel], monkeypatch)
    seed_x0 = seed_x ^ 0x5DEECE66D
    gen = _gen(K)
    x, w_in, b_in = _pos(gen, M, K), _pos(gen, 256, K) * 0.1, _pos(gen, 256)
    w0, a, le = torch.randn(256, 256, device=DEV, generator=gen) * 0.07, _pos(gen, M), torch.randn(M, 256, device=DEV, generator=gen)
    fr = gemm.trunk_front(x, w_in, b_in, w0, a, le, p, seed_x, seed_x0, row0, want_bits=True, want_drop=True)
    assert fr is not None
    x0, bits, x0d, z0 = fr
    _status_ok()
    x0_ref = gemm.mm_nn(_drop(x, _keep((M, K), p, seed_x, row0 * K, sd), p), w_in.t().contiguous(), bias=b_in, relu=True)
    assert torch.equal(x0, x0_ref) and bool((x0 > 0).all()) and bool((bits == -1).all())
    x0d_ref = _drop(x0, _keep((M, 256), p, seed_x0, row0 * 256, sd), p)
    assert torch.equal(x0d, x0d_ref)
    assert torch.equal(z0, gemm.mm_nn(x0d_ref, w0, rowscale=a, addend=le))


# ---------------------------------------------------------------------------------------------
# (b) fused stores: act = relu(.) > 0 everywhere, out = dropout(c_act * act + c_mix * mix), mask words = the keep-mask itself
# ---------------------------------------------------------------------------------------------
C_ACT, C_MIX = 0.5, 0.25      # powers of two: both products are exact, so c_act * act + c_mix * mix is one rounding however the kernel forms it


def _hubby_graph(n, T=2):
    """Directed graph: every node has one in-edge, the first quarter many more — with hub threshold 2 both the row kernels and the hub kernels store rows."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    gen = _gen(n)
    dst = torch.cat([torch.arange(n, device=DEV), torch.randint(0, n // 4, (6 * n,), device=DEV, generator=gen)])
    src = torch.randint(0, n, (dst.numel(),), device=DEV, generator=gen)
    G = CSRGraph(torch.stack([src, dst]), n, hub_threshold=T)
    assert 0 < G._plan.n_hubs < n
    return G


def _stored(act, mix, keep, p):
    """What a fused store writes for the ReLU output act: the mix (one rounding, see C_ACT), then the masked product."""
    x = C_ACT * act + C_MIX * mix if mix is not None else act
    return _drop(x, keep, p)


def _subset(n_nodes, m, seed):
    idx = torch.sort(torch.randperm(n_nodes, device=DEV, generator=_gen(seed))[:m])[0]
    idx[0], idx[-1] = 0, n_nodes - 1      # both sides of B
    return torch.unique(idx)


@pytest.mark.parametrize('with_mix', [True, False])
@pytest.mark.parametrize('case', list(CASES))
def test_aggregation_store_draws_the_host_mask(case, with_mix, monkeypatch):
    """cb_spmm_csr_fused_f32 on all rows (row0 = the graph's row offset): row kernel and hub finish."""
    from gnn_tail_generalization_amd import trunk
    n, p = 777, 0.3
    G = _hubby_graph(n)
    row0, seed, sd = _case(case, 256, monkeypatch)
    monkeypatch.setattr(G, 'row_offset', row0)
    gen = _gen(21)
    z, bias, x0 = _pos(gen, n, 256), _pos(gen, 256), (torch.randn(n, 256, device=DEV, generator=gen) if with_mix else None)
    bits, out, act = trunk._fused_spmm(G, z, bias, x0, C_ACT, C_MIX, p, seed, want_act=True)
    _status_ok()
    keep = _keep((n, 256), p, seed, row0 * 256, sd)
    assert bool((act > 0).all())
    assert torch.equal(bits, _mask_words(keep))
    assert torch.equal(out, _stored(act, x0, keep, p))
    if not with_mix:
        assert torch.equal(out != 0, keep)


@pytest.mark.parametrize('case', list(CASES))
def test_aggregation_store_on_a_row_subset_draws_the_host_mask(case, monkeypatch):
    """cb_spmm_csr_fused_f32 with row_ids: the CSR's rows are a subset of the node rows; mask and mask words at the node row."""
    from gnn_tail_generalization_amd import _lib, trunk
    n, p = 777, 0.3
    G = _hubby_graph(n)
    row0, seed, sd = _case(case, 256, monkeypatch)
    monkeypatch.setattr(G, 'row_offset', row0)
    idx = _subset(n, 300, 5)
    fwd = G._support_fwd(type('S', (), {'idx': idx, 'n': int(idx.numel())})(), n, force=True)
    assert fwd._plan.n_hubs > 0
    gen = _gen(22)
    z, bias, x0 = _pos(gen, n, 256), _pos(gen, 256), torch.randn(n, 256, device=DEV, generator=gen)
    b_rows = G.norm_in[idx].contiguous()
    bits, out, act = trunk._fused_launch(_lib.load(), G, fwd, z, None, bias, x0, C_ACT, C_MIX, p, seed, True, row_ids=idx.to(torch.int32).contiguous(),
                                         row_scale=b_rows)
    _status_ok()
    keep = _keep_rows(idx, n, 256, p, seed, row0, sd)
    assert bool((act > 0).all())
    assert torch.equal(bits[idx], _mask_words(keep))
    assert torch.equal(out, _stored(act, x0[idx], keep, p))


@pytest.mark.parametrize('d,relu_only,with_index', [(256, False, False), (512, True, True)])
@pytest.mark.parametrize('case', list(CASES))
def test_store_rows_draws_the_host_mask(d, relu_only, with_index, case, monkeypatch):
    """cb_trunk_store_rows_f32: the mask is drawn at row0 + row_ids[m]."""
    from gnn_tail_generalization_amd import trunk
    n_nodes, p = 1500, 0.3
    row0, seed, sd = _case(case, d, monkeypatch)
    idx = _subset(n_nodes, 413, d)
    M = idx.numel()
    gen = _gen(23)
    y = _pos(gen, M, d)
    mix = torch.randn(M + 9 if with_index else n_nodes, d, device=DEV, generator=gen)
    mix_index = torch.randperm(M + 9, device=DEV, generator=gen)[:M].contiguous() if with_index else None
    bits = torch.full((n_nodes, d // 256, 4), -7, dtype=torch.int64, device=DEV)
    out, act = trunk._store_rows(y, idx, mix, C_ACT, C_MIX, p, seed, row0, bits, relu_only, mix_index, want_act=True)
    _status_ok()
    keep = _keep_rows(idx, n_nodes, d, p, seed, row0, sd)
    assert torch.equal(act, y)
    assert torch.equal(out, _stored(y, mix[mix_index] if with_index else mix[idx], keep, p))
    assert torch.equal(bits[idx], _ones_words(M, d // 256) if relu_only else _mask_words(keep))
    outside = torch.ones(n_nodes, dtype=torch.bool, device=DEV)
    outside[idx] = False
    assert bool((bits[outside] == -7).all())


@pytest.mark.parametrize('case', list(CASES))
def test_gemm_store_rows_draws_the_host_mask(case, monkeypatch):
    """cb_gemm_nn_store_rows_f32 (the fused form exists for every M > 0 at N = 256 on aligned operands: cb_gemm_nn_store_rows_supported)."""
    from gnn_tail_generalization_amd import gemm
    n_nodes, K, p = 1500, 36, 0.3
    row0, seed, sd = _case(case, 256, monkeypatch)
    idx = _subset(n_nodes, 413, 7)
    M = idx.numel()
    gen = _gen(24)
    a, b, rs, add, bias = _pos(gen, M, K), _pos(gen, K, 256), _pos(gen, M), _pos(gen, M, 256), _pos(gen, 256)
    mix = torch.randn(n_nodes, 256, device=DEV, generator=gen)
    bits = torch.full((n_nodes, 1, 4), -7, dtype=torch.int64, device=DEV)
    res = gemm.mm_nn_store_rows(a, b, rs, add, bias, idx, mix, None, C_ACT, C_MIX, p, seed, row0, bits, False, want_act=True)
    assert res is not None
    out, act = res
    _status_ok()
    keep = _keep_rows(idx, n_nodes, 256, p, seed, row0, sd)
    assert torch.equal(act, gemm.mm_nn(a, b, rowscale=rs, addend=add, bias=bias, relu=True)) and bool((act > 0).all())
    assert torch.equal(out, _stored(act, mix[idx], keep, p))
    assert torch.equal(bits[idx], _mask_words(keep))


@pytest.mark.parametrize('case', list(CASES))
def test_aggregation_gemm_store_rows_draws_the_host_mask(case, monkeypatch):
    """cb_spmm_gemm_store_rows_f32: aggregation, 256 x 256 transform and the store on the node rows row_ids from one kernel."""
    from gnn_tail_generalization_amd import gemm
    from gnn_tail_generalization_amd.graph import weight_image
    n, p = 777, 0.3
    G = _hubby_graph(n)
    row0, seed, sd = _case(case, 256, monkeypatch)
    idx = _subset(n, 300, 9)
    M = idx.numel()
    fwd = G._support_fwd(type('S', (), {'idx': idx, 'n': int(M)})(), n, force=True)
    gen = _gen(25)
    h, a, w = _pos(gen, n, 256), _pos(gen, n), _pos(gen, 256, 256) * 0.05
    b_rows, bias, mix = _pos(gen, M), _pos(gen, 256), torch.randn(n, 256, device=DEV, generator=gen)
    bits = torch.full((n, 1, 4), -7, dtype=torch.int64, device=DEV)
    h_agg, out, act = fwd.spmm_gemm_store_rows(h, a, weight_image(w), b_rows, bias, idx, mix, None, C_ACT, C_MIX, p, seed, row0, bits, False, True)
    _status_ok()
    keep = _keep_rows(idx, n, 256, p, seed, row0, sd)
    assert torch.equal(h_agg, fwd.spmm(h, col_scale=a))
    assert torch.equal(act, gemm.mm_nn(h_agg, w, rowscale=b_rows, bias=bias, relu=True)) and bool((act > 0).all())
    assert torch.equal(out, _stored(act, mix[idx], keep, p))
    assert torch.equal(bits[idx], _mask_words(keep))


@pytest.mark.parametrize('head', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_aggregation_store_with_gemm_tail_draws_the_host_mask(case, head, monkeypatch):
    """cb_spmm_gemm_fused_f32 and its head form: the trunk store inside the aggregation + GEMM kernel (row0 = the graph's row offset)."""
    from gnn_tail_generalization_amd import gemm, trunk
    from gnn_tail_generalization_amd.graph import head_image, weight_image
    n, p, C = 777, 0.3, 40
    G = _hubby_graph(n)
    row0, seed, sd = _case(case, 256, monkeypatch)
    monkeypatch.setattr(G, 'row_offset', row0)
    gen = _gen(26)
    z, bias, x0 = _pos(gen, n, 256), _pos(gen, 256), torch.randn(n, 256, device=DEV, generator=gen)
    if head:
        w_out, b_out = torch.randn(C, 256, device=DEV, generator=gen) * 0.07, torch.randn(C, device=DEV, generator=gen)
        bits, out, tail, act = trunk._fused_gemm_launch(G, z, bias, x0, C_ACT, C_MIX, p, seed, head_image(w_out), None, None, want_act=True, head=(b_out, C))
    else:
        w, le = torch.randn(256, 256, device=DEV, generator=gen) * 0.07, torch.randn(n, 256, device=DEV, generator=gen)
        bits, out, tail, act = trunk._fused_gemm_launch(G, z, bias, x0, C_ACT, C_MIX, p, seed, weight_image(w), G.norm_out, le, want_act=True)
    _status_ok()
    keep = _keep((n, 256), p, seed, row0 * 256, sd)
    assert bool((act > 0).all())
    assert torch.equal(bits, _mask_words(keep))
    assert torch.equal(out, _stored(act, x0, keep, p))
    want = gemm.mm_nn(out, w_out.t().contiguous(), bias=b_out) if head else gemm.mm_nn(out, w, rowscale=G.norm_out, addend=le)
    assert torch.equal(tail, want)


# ---------------------------------------------------------------------------------------------
# (b) backward kernels: integer gradients, power-of-two factors, p = 0.5 (scale 2), all-ones mask words — exact arithmetic
# ---------------------------------------------------------------------------------------------
P2 = 0.5


def _k(shape, seed, row0, sd):
    return _keep(shape, P2, seed, row0 * shape[1], sd).double() * 2.0      # keep ? 1 / (1 - p) : 0


def _compact(gen, n, frac, d):
    """A compact operand over a random row subset: (rows [m, d], int32 positions [n] (-1: absent), the operand scattered to [n, d] in float64)."""
    member = torch.rand(n, device=DEV, generator=gen) < frac
    pos = torch.where(member, torch.cumsum(member, 0, dtype=torch.int32) - 1, torch.full((n,), -1, dtype=torch.int32, device=DEV)).contiguous()
    rows = _ints(gen, 1, 3, int(member.sum()), d)
    full = torch.zeros(n, d, dtype=torch.float64, device=DEV)
    full[member] = rows.double()
    return rows, pos, full


@pytest.mark.parametrize('d', [256, 512])
@pytest.mark.parametrize('case', list(CASES))
def test_layer_backward_draws_both_host_masks(d, case, monkeypatch):
    """cb_trunk_layer_bwd_f32 with the 'Residual' second gradient (g2 / seed2), dense and compact."""
    from gnn_tail_generalization_amd import trunk
    n = 1037
    row0, seed, sd = _case(case, d, monkeypatch)
    seed2 = seed ^ 0x5DEECE66D
    gen = _gen(31)
    g, g2, rs = _ints(gen, -4, 4, n, d, nonzero=True), _ints(gen, 1, 3, n, d), _pow2(gen, n)
    g2c, g2_pos, g2c_full = _compact(gen, n, 0.4, d)
    bits = _ones_words(n, d // 256)
    k1, k2 = _k((n, d), seed, row0, sd), _k((n, d), seed2, row0, sd)
    for second, second_full, pos in ((g2, g2.double(), None), (g2c, g2c_full, g2_pos), (None, None, None)):
        gx0 = torch.empty(n, d, device=DEV)
        out, cs = trunk._layer_bwd(g, bits, rs, gx0, False, P2, seed, row0, 0.5, 0.25, True, g2=second, seed2=seed2 if second is not None else 0,
                                   c2=0.125 if second is not None else 0.0, g2_pos=pos)
        _status_ok()
        gm = g.double() * k1
        gy = 0.5 * gm + (0.125 * second_full * k2 if second is not None else 0.0)
        assert torch.equal(gx0.double(), 0.25 * gm)
        assert torch.equal(out.double(), gy * rs.double().unsqueeze(1)) and torch.equal(cs.double(), gy.sum(0))
    assert torch.equal(gx0 != 0, k1 != 0)


@pytest.mark.parametrize('case', list(CASES))
def test_layer_backward_on_compact_rows_draws_both_host_masks(case, monkeypatch):
    """cb_trunk_layer_bwd_rows_f32: mask words, row scale and both masks at the node row rows_idx[r]."""
    from gnn_tail_generalization_amd import trunk
    n_nodes, d = 1500, 256
    row0, seed, sd = _case(case, d, monkeypatch)
    seed2 = seed ^ 0x5DEECE66D
    idx = _subset(n_nodes, 413, 3)
    M = idx.numel()
    gen = _gen(32)
    g, rs = _ints(gen, -4, 4, M, d, nonzero=True), _pow2(gen, n_nodes)
    g2c, g2_pos, g2_full = _compact(gen, n_nodes, 0.5, d)
    out, cs = trunk._layer_bwd_rows(g, idx, _ones_words(n_nodes), rs, P2, seed, row0, 0.5, True, g2=g2c, seed2=seed2, c2=0.125, g2_pos=g2_pos)
    _status_ok()
    k1, k2 = _k((n_nodes, d), seed, row0, sd)[idx], _k((n_nodes, d), seed2, row0, sd)[idx]
    gy = 0.5 * g.double() * k1 + 0.125 * g2_full[idx] * k2
    assert torch.equal(out.double(), gy * rs[idx].double().unsqueeze(1)) and torch.equal(cs.double(), gy.sum(0))
    out1, _ = trunk._layer_bwd_rows(g, idx, _ones_words(n_nodes), rs, P2, seed, row0, 0.5, False)
    assert torch.equal(out1 != 0, k1 != 0)


@pytest.mark.parametrize('case', list(CASES))
def test_layer_backward_fold_draws_three_host_masks(case, monkeypatch):
    """cb_trunk_layer_bwd_fold_f32: the store's own mask and one per folded mix gradient (a dense and a compact operand), and the second column sum."""
    from gnn_tail_generalization_amd import trunk
    n, d = 1037, 256
    row0, seed, sd = _case(case, d, monkeypatch)
    seeds = [seed ^ 0x5DEECE66D, seed + 3]
    gen = _gen(33)
    g, rs = _ints(gen, -4, 4, n, d, nonzero=True), _pow2(gen, n)
    dense = _ints(gen, 1, 3, n, d)
    comp, pos, comp_full = _compact(gen, n, 0.4, d)
    out, cs, m, cs2 = trunk._layer_bwd_fold(g, _ones_words(n), rs, P2, seed, row0, 0.5, 0.25, True, [dense, comp], [None, pos], seeds,
                                            cs=(1, _ones_words(n), 0.5))
    _status_ok()
    gm = g.double() * _k((n, d), seed, row0, sd)
    u0, u1 = dense.double() * _k((n, d), seeds[0], row0, sd), comp_full * _k((n, d), seeds[1], row0, sd)
    assert torch.equal(out.double(), 0.5 * gm * rs.double().unsqueeze(1)) and torch.equal(cs.double(), (0.5 * gm).sum(0))
    assert torch.equal(m.double(), 0.25 * (gm + u0 + u1))
    assert torch.equal(cs2.double(), (0.5 * u1).sum(0))


@pytest.mark.parametrize('with_cs', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_input_backward_draws_four_host_masks(case, with_cs, monkeypatch):
    """cb_trunk_input_bwd_multi_f32 / _cs_f32: the gradient's own mask and three mixed-in ones (two dense operands, one compact)."""
    from gnn_tail_generalization_amd import trunk
    n, d = 1037, 256
    row0, seed, sd = _case(case, d, monkeypatch)
    seeds = [seed ^ 0x5DEECE66D, seed + 3, (seed * 7 + 1) % 2 ** 62]
    gen = _gen(34)
    g = _ints(gen, -4, 4, n, d, nonzero=True)
    d0, d1 = _ints(gen, 1, 3, n, d), _ints(gen, 1, 3, n, d)
    comp, pos, comp_full = _compact(gen, n, 0.4, d)
    act = _pos(gen, n, d)
    res = trunk._input_bwd_multi(g, seed, [d0, comp, d1], seeds, 0.25, act, P2, row0, act_bits=_ones_words(n) if with_cs else None,
                                 mix_pos=[None, pos, None], cs=[(1, _ones_words(n), 0.5), (2, _ones_words(n), 2.0)] if with_cs else None)
    _status_ok()
    u = [d0.double() * _k((n, d), seeds[0], row0, sd), comp_full * _k((n, d), seeds[1], row0, sd), d1.double() * _k((n, d), seeds[2], row0, sd)]
    want = g.double() * _k((n, d), seed, row0, sd) + 0.25 * (u[0] + u[1] + u[2])
    assert torch.equal(res[0].double(), want) and torch.equal(res[1].double(), want.sum(0))
    if with_cs:
        assert torch.equal(res[2][0].double(), (0.5 * u[1]).sum(0)) and torch.equal(res[2][1].double(), (2.0 * u[2]).sum(0))


@pytest.mark.parametrize('case', list(CASES))
def test_single_operand_input_backward_draws_the_host_mask(case, monkeypatch):
    """cb_trunk_input_bwd_f32: (add + dropout_bwd(g)) * (act > 0)."""
    from gnn_tail_generalization_amd import trunk
    n, d = 1037, 256
    row0, seed, sd = _case(case, d, monkeypatch)
    gen = _gen(35)
    g, add, act = _ints(gen, 1, 4, n, d), _ints(gen, -2, 2, n, d), _pos(gen, n, d)
    out, cs = trunk._input_bwd(g, add, act, P2, seed, row0)
    _status_ok()
    want = add.double() + g.double() * _k((n, d), seed, row0, sd)
    assert torch.equal(out.double(), want) and torch.equal(cs.double(), want.sum(0))


@pytest.mark.parametrize('n_mix', [None, 0, 2])
@pytest.mark.parametrize('case', list(CASES))
def test_reverse_aggregation_store_backward_draws_the_host_masks(case, n_mix, monkeypatch):
    """cb_spmm_csr_store_bwd_f32 and its _mix form (n_mix operands folded), row kernel and hub finish."""
    n, d = 777, 256
    G = _hubby_graph(n)
    row0, seed, sd = _case(case, d, monkeypatch)
    gen = _gen(36)
    h, rs, brs = _ints(gen, 1, 2, n, d), _pow2(gen, n), _pow2(gen, n)
    raw = G.spmm(h, row_scale=rs).double()      # integer sums times a power of two: exact
    assert float(raw.abs().max()) < 2 ** 20
    gm = raw * _k((n, d), seed, row0, sd)
    want_gr = 0.5 * gm * brs.double().unsqueeze(1)
    if n_mix is None:
        g_raw, gr = G.spmm_store_bwd(h, rs, _ones_words(n), brs, 0.5, P2, seed, row0)
        _status_ok()
        assert torch.equal(g_raw.double(), raw) and torch.equal(gr.double(), want_gr)
        assert torch.equal(gr != 0, gm != 0)
        return
    ops_, pos_, seeds_, fold = [], [], [], gm.clone()
    for q in range(n_mix):
        rows, pos, full = _compact(gen, n, (0.2, 0.6)[q], d)
        ops_.append(rows), pos_.append(pos), seeds_.append(seed + 11 + q)
        fold += full * _k((n, d), seeds_[q], row0, sd)
    m, gr, db = G.spmm_store_bwd(h, rs, _ones_words(n), brs, 0.5, P2, seed, row0, mix=(ops_, pos_, seeds_, 0.25, True))
    _status_ok()
    assert torch.equal(gr.double(), want_gr) and torch.equal(m.double(), 0.25 * fold) and torch.equal(db.double(), (0.5 * gm).sum(0))


# ---------------------------------------------------------------------------------------------
# (b) student row kernel: no row0; flat index r * d + c
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [256, 194, 386, 20, 1])
@pytest.mark.parametrize('rows', [1, 63])
@pytest.mark.parametrize('seed,seed_dev', [(2 ** 40 + 12345, None), (0x1234ABCD5, 2 ** 32 - 1)])
def test_ln_gelu_dropout_zero_pattern_is_the_host_mask(d, rows, seed, seed_dev, monkeypatch):
    """gamma = 0, beta = 1: every pre-dropout value is gelu(1) > 0, so the output is zero exactly where the mask drops (widths that are no multiple of four
    start rows inside a quad).  One row: the backward's beta gradient dy * keep * gelu'(1) shows the regenerated mask."""
    from gnn_tail_generalization_amd import ops
    p = 0.3
    if seed_dev:
        monkeypatch.setattr(ops, '_graph_seed', torch.tensor([seed_dev], dtype=torch.int64, device=DEV))
    z = torch.randn(rows, d, device=DEV, generator=_gen(d))
    gamma, beta = torch.zeros(d, device=DEV), torch.ones(d, device=DEV).requires_grad_(True)
    out = ops.ln_gelu_dropout(z, gamma, beta, p=p, training=True, seed=seed)
    keep = _keep((rows, d), p, seed, 0, seed_dev or 0)
    kept = out.detach()[keep]
    assert torch.equal(out.detach() != 0, keep)
    assert kept.numel() == 0 or (torch.equal(kept, kept[:1].expand_as(kept)) and 1.2 < float(kept[0]) < 1.21)      # gelu(1) / 0.7 = 1.2019
    if rows == 1:
        out.backward(torch.ones_like(out))
        assert torch.equal(beta.grad != 0, keep[0])
