"""The fused neighbour-contrastive loss (ops.neighbor_contrastive_loss, csrc/cb_ncloss.hip) against the float64 restatement of the reference
formula (tests/ncloss_ref.py: dense [B, B], last-occurrence rule).

Tolerance: the project's form (tests/student_ref.within): err32 is the error against float64 of torch's own float32 composition of the reference
formula on the device; the operator's error must satisfy err <= max(2 err32, 8 * 2^-24), err = student_ref.rel_err.  num and den are compared as
[B, 1] columns (every row its own scale), dz row-wise.  The scalar loss is one number and torch's own error on it can be small by luck, so it is
bounded from the parts: |loss - loss64| <= tol_num + tol_den + 8 * 2^-24 (1 + |loss64|).  M and the set {i : num_i != 0} are exact."""
import math

import pytest
import torch

import ncloss_ref as nr
import student_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_powers = {}


def dev_power(name, r, extra_nodes=0):
    from gnn_tail_generalization_amd import ops
    key = (name, r, extra_nodes)
    if key not in _powers:
        _powers[key] = ops.SparsePower(nr.power(name, r, extra_nodes), DEV)
    return _powers[key]


def check(tag, z, pw_host, power, b, tau, want_grad=True):
    """One forward (+ backward) of the operator on z [B, D] for the batch b, every figure printed before it is asserted."""
    from gnn_tail_generalization_amd import ops
    B = len(b)
    adj64 = nr.crop_dense(pw_host, b)
    loss64, num64, den64, nz64, dz64 = nr.with_grad(z.double(), adj64, tau)
    loss32, num32, den32, nz32, dz32 = nr.with_grad(z.to(DEV), adj64.float().to(DEV), tau)
    zd = z.to(DEV).requires_grad_(True)
    loss, num, den, m = ops.neighbor_contrastive_loss(zd, power, b, tau, return_parts=True)
    assert loss.dim() == 0 and not num.requires_grad and not den.requires_grad
    tol = {}
    for name, got, ref32, ref64 in (('num', num, num32, num64), ('den', den, den32, den64)):
        err, err32 = sr.rel_err(got.reshape(B, 1), ref64.reshape(B, 1)), sr.rel_err(ref32.reshape(B, 1), ref64.reshape(B, 1))
        tol[name] = max(2 * err32, 8 * sr.EPS24)
        print(f'{tag} {name}: err {err:.3e} torch-fp32 err {err32:.3e} bound {tol[name]:.3e}')
        assert sr.within(err, err32), (tag, name, err, err32)
    mine = torch.where(num.cpu() != 0)[0]
    print(f'{tag} M: {int(m)} reference {len(nz64)}; core {ops.ncloss_core(zd.detach())}')
    assert int(m) == len(nz64) and torch.equal(mine, nz64)
    if len(nz64) == 0:
        assert math.isnan(float(loss))
        return None
    bound = tol['num'] + tol['den'] + 8 * sr.EPS24 * (1 + abs(float(loss64)))
    print(f'{tag} loss: {float(loss):.9f} float64 {float(loss64):.9f} |diff| {abs(float(loss) - float(loss64)):.3e} bound {bound:.3e} (torch-fp32 {float(loss32):.9f})')
    assert abs(float(loss) - float(loss64)) <= bound
    if not want_grad:
        return loss.detach(), None, num, m
    g = torch.tensor(1.7, device=DEV)
    (dz,) = torch.autograd.grad(loss * g, zd)
    err, err32 = sr.rel_err(dz, 1.7 * dz64), sr.rel_err(dz32, dz64)
    print(f'{tag} dz: err {err:.3e} torch-fp32 err {err32:.3e} bound {max(2 * err32, 8 * sr.EPS24):.3e}')
    assert sr.within(err, err32), (tag, 'dz', err, err32)
    return loss.detach(), dz, num, m


CASES = [('powerlaw', 127, 256, 0.5, 2), ('asym_multi', 128, 36, 2.0, 3), ('asym_multi', 129, 30, 0.5, 2), ('powerlaw', 257, 30, 2.0, 3),
         ('asym_multi', 257, 256, 0.5, 3), ('powerlaw', 129, 36, 0.5, 3), ('powerlaw', 128, 256, 2.0, 2), ('asym_multi', 127, 30, 2.0, 2)]


@pytest.mark.parametrize('name,B,D,tau,r', CASES)
def test_loss_parts_and_gradient(name, B, D, tau, r):
    from gnn_tail_generalization_amd import ops
    z = nr.embeddings(B, D)
    b = nr.batch(name, B)
    assert len(torch.unique(b)) < B
    assert ops.ncloss_core(z.to(DEV)) == ('fp32' if D == 30 else 'limb')        # D = 30 takes the non-float4 core
    check(f'{name} B={B} D={D} tau={tau} r={r}', z, nr.power(name, r), dev_power(name, r), b, tau)


@pytest.mark.parametrize('name,D', [('powerlaw', 256), ('asym_multi', 30)])
def test_one_row_gives_nan(name, D):
    from gnn_tail_generalization_amd import ops
    z = nr.embeddings(1, D)
    assert check(f'{name} B=1 D={D}', z, nr.power(name, 2), dev_power(name, 2), nr.batch(name, 1), 0.5) is None
    loss = ops.neighbor_contrastive_loss(z.to(DEV), dev_power(name, 2), nr.batch(name, 1), 0.5)
    assert math.isnan(float(loss))


def test_no_duplicates_and_duplicates_across_a_row_block_boundary():
    name, r, tau, D = 'powerlaw', 2, 0.5, 36
    g = torch.Generator().manual_seed(4)
    b = torch.randperm(300, generator=g)[:257]
    assert len(torch.unique(b)) == 257
    check('no duplicates', nr.embeddings(257, D), nr.power(name, r), dev_power(name, r), b, tau)
    b = b.clone()
    b[200] = b[100]          # the representative (200) and its earlier copy (100) lie in different 128-row blocks
    b[130] = b[5]
    b[256] = b[127]
    b[3] = b[250]            # ... and one whose representative comes first in block order of the copy's block
    check('duplicates across the boundary', nr.embeddings(257, D), nr.power(name, r), dev_power(name, r), b, tau)


def test_a_node_without_batch_neighbours_is_left_out_of_the_mean():
    """Node 300 is isolated (only its self loop, which the diagonal mask removes): in the batch once and twice."""
    from gnn_tail_generalization_amd import ops
    name, r, tau = 'asym_multi', 2, 2.0
    pw, power = nr.power(name, r, 1), dev_power(name, r, 1)
    assert power.n == 301
    for B, where in ((129, [7]), (130, [7, 129])):
        b = nr.batch(name, B)
        b[where] = 300
        z = nr.embeddings(B, 256)
        check(f'isolated node at {where}', z, pw, power, b, tau)
        _, num, _, m = ops.neighbor_contrastive_loss(z.to(DEV), power, b, tau, return_parts=True)
        assert all(float(num[i]) == 0.0 for i in where) and int(m) < B
    with pytest.raises(ValueError, match='301 nodes'):
        ops.neighbor_contrastive_loss(nr.embeddings(4, 8).to(DEV), power, torch.tensor([0, 301, 2, 3]), tau)


@pytest.fixture
def knobs():
    from gnn_tail_generalization_amd import tuning
    keep = (tuning.T.ncloss_max_splits, tuning.T.ncloss_slab_rows)
    yield tuning.T
    tuning.T.ncloss_max_splits, tuning.T.ncloss_slab_rows = keep


@pytest.mark.parametrize('D', [256, 30])
def test_one_block_folds_several_tiles_and_several_backward_slabs(knobs, D):
    """B = 640 is five column tiles: with the split cap at 2 a block folds three of them; with slab height 128 the backward runs five slabs.
    Every setting is held to the bound against float64 (check); num and M do not depend on either knob (bit-equal), the forward not on the slab height
    (bit-equal loss); the capped sweep associates den's sum differently and the slabs the backward's GEMM, so those are compared by the bound only."""
    from gnn_tail_generalization_amd import ops
    name, r, tau, B = 'asym_multi', 3, 0.5, 640
    z, b = nr.embeddings(B, D), nr.batch(name, B)
    base = check(f'B=640 D={D} default', z, nr.power(name, r), dev_power(name, r), b, tau)
    knobs.ncloss_max_splits = 2
    capped = check(f'B=640 D={D} split cap 2', z, nr.power(name, r), dev_power(name, r), b, tau)
    knobs.ncloss_max_splits, knobs.ncloss_slab_rows = 0, 128
    slabs = check(f'B=640 D={D} slab 128', z, nr.power(name, r), dev_power(name, r), b, tau)
    assert torch.equal(base[0], slabs[0])                         # the slab height does not touch the forward
    for other in (capped, slabs):
        assert torch.equal(base[2], other[2]) and int(base[3]) == int(other[3])
    print('dz default vs slab 128: max |diff|', float((base[1] - slabs[1]).abs().max()), '; loss default vs cap 2', float(base[0]), float(capped[0]))


def test_many_row_blocks():
    name, r, tau, B, D = 'powerlaw', 2, 2.0, 4099, 256
    check('B=4099', nr.embeddings(B, D), nr.power(name, r), dev_power(name, r), nr.batch(name, B), tau)


def test_two_identical_calls_give_the_same_bits():
    from gnn_tail_generalization_amd import ops
    name, r, tau, B, D = 'asym_multi', 2, 0.5, 257, 256
    b, power = nr.batch(name, B), dev_power(name, r)
    outs = []
    for _ in range(2):
        z = nr.embeddings(B, D).to(DEV).requires_grad_(True)
        loss = ops.neighbor_contrastive_loss(z, power, b.to(DEV), tau)
        loss.backward()
        outs.append((loss.detach().clone(), z.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][1]).all()) and float(outs[0][1].abs().max()) > 0


def test_sparse_tensor_is_converted_by_the_reference_named_function():
    from gnn_tail_generalization_amd import MLP_model, ops
    name, r, tau, B, D = 'powerlaw', 2, 2.0, 129, 36
    z, b = nr.embeddings(B, D).to(DEV), nr.batch(name, B)
    a = MLP_model.get_neighbor_contrastive_loss(z, nr.power(name, r), b.numpy(), tau)
    c = MLP_model.get_neighbor_contrastive_loss(z, dev_power(name, r), b, tau)
    assert torch.equal(a, c) and torch.equal(a, ops.neighbor_contrastive_loss(z, dev_power(name, r), b, tau))


@pytest.mark.parametrize('N,D', [(257, 256), (130, 30), (1, 7)])
def test_cosine_sim(N, D):
    from gnn_tail_generalization_amd import MLP_model
    x = nr.embeddings(N, D, seed=3)

    def ref(v):
        n = torch.norm(v, p=2, dim=1, keepdim=True)
        return (v @ v.T) * ((n @ n.T) ** (-1))
    got, ref64, ref32 = MLP_model.cosine_sim(x.to(DEV)), ref(x.double()), ref(x.to(DEV))
    err, err32 = sr.rel_err(got, ref64), sr.rel_err(ref32, ref64)
    print(f'cosine_sim N={N} D={D}: err {err:.3e} torch-fp32 err {err32:.3e}')
    assert tuple(got.shape) == (N, N) and sr.within(err, err32)
