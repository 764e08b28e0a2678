"""GPU: the forward front after its dropout keep-masks moved under the K loops (csrc/cb_front.hip, csrc/cb_tile_gemm.h, csrc/cb_philox.h;
profiles/mask_draws.md).  k_front now draws the keep decisions of dropout(x) of a block's NEXT tile under the input Linear's K loop and those of
dropout(X0) of the next tile under layer 0's K loop, one Philox quad per K step, and carries them as bits in two shift registers; the first tile's
are drawn before the tile loop.  What can break: the quad counter of a draw (a wrong tile, row or stride; its upper half past 2^32), the place of a
draw in its word (4-bit fields, K = 64 fills half a word), the hand-over from tile to tile (blocks that run 0, 1, 2 and 3 tiles; the draw past a
block's last tile), and the seed taken through the device seed word.  Everything is compared BIT FOR BIT (torch.equal) with the composition
test_gpu_kernels.py::test_forward_front_kernel_equals_the_two_gemms uses: dropout + cb_gemm_nn_f32 (bias, ReLU) + dropout + cb_gemm_nn_f32."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SX, S0 = 0x1234ABCD5, 0x77F3A1    # the seeds the two dropouts see
WORD = 0xABCDE                     # a device seed word (< both seeds)


@functools.lru_cache(maxsize=1)
def _grid():
    """k_front's persistent grid: two blocks per CU."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _rows(name):
    G = _grid()
    return {'1': 1, '63': 63, '64': 64, '65': 65, '64G-1': 64 * G - 1, '64G+1': 64 * G + 1, '128G+17': 128 * G + 17}[name]


@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
@pytest.mark.parametrize('K', [64, 128])
@pytest.mark.parametrize('rows', ['1', '63', '64', '65', '64G-1', '64G+1', '128G+17'])
def test_front_with_masks_drawn_under_the_k_loops_equals_the_two_gemms(rows, K, p, monkeypatch):
    """X0, its mask words, the dropped copy and Z0 of cb_trunk_front_f32 against the two-kernel composition: blocks with 0 .. 3 tiles (G = the persistent
    grid), both input widths, p = 0 (nothing drawn) / 0.1 / 0.5, row0 = 0 and 2^26 + 3 (quad counters past 32 bits), the seed given directly and
    through the device seed word, with and without the dropped copy (and with / without row scale and addend)."""
    from gnn_tail_generalization_amd import gemm, ops
    M = _rows(rows)
    monkeypatch.setattr(ops, '_graph_seed', None)
    gen = torch.Generator(device=DEV).manual_seed(31 * M + K)
    x = torch.rand(M, K, device=DEV, generator=gen)
    w_in = torch.randn(256, K, device=DEV, generator=gen) * 0.1
    b_in = torch.randn(256, device=DEV, generator=gen) * 0.1
    w0 = torch.randn(256, 256, device=DEV, generator=gen) * 0.07
    a = torch.rand(M, device=DEV, generator=gen) + 0.5
    le = torch.randn(M, 256, device=DEV, generator=gen)
    wt = w_in.t().contiguous()
    shifts = torch.arange(64, device=DEV, dtype=torch.int64)
    for row0 in (0, 2 ** 26 + 3):
        monkeypatch.setattr(ops, '_graph_seed', None)
        xd = ops._dropout_raw(x, p, SX, row0 * K) if p > 0 else x
        x0_ref = gemm.mm_nn(xd, wt, bias=b_in, relu=True)
        x0d_ref = ops._dropout_raw(x0_ref, p, S0, row0 * 256) if p > 0 else x0_ref
        z_ref = {True: gemm.mm_nn(x0d_ref, w0, rowscale=a, addend=le), False: gemm.mm_nn(x0d_ref, w0)}
        pos = x0_ref > 0
        words = torch.stack([(pos[:, kk::4].to(torch.int64) << shifts).sum(dim=1) for kk in range(4)], dim=1)
        if p > 0:
            kept = (x0d_ref != 0).sum().item() / max(1, int(pos.sum()))
            assert M < 1000 or abs(kept - (1 - p)) < 0.02      # (the reference itself drops what it should)
        for through_word in (False, True):
            monkeypatch.setattr(ops, '_graph_seed', torch.tensor([WORD], dtype=torch.int64, device=DEV) if through_word else None)
            sx, s0 = (SX - WORD, S0 - WORD) if through_word else (SX, S0)
            for full in (True, False):
                fr = gemm.trunk_front(x, w_in, b_in, w0, a if full else None, le if full else None, p, sx, s0, row0, want_bits=True, want_drop=full)
                assert fr is not None
                x0, bits, x0d, z0 = fr
                what = (row0, through_word, full)
                assert torch.equal(x0, x0_ref), what
                assert torch.equal(bits[:, 0, :], words), what
                assert (x0d is None) == (not full) and (x0d is None or torch.equal(x0d, x0d_ref)), what
                assert torch.equal(z0, z_ref[full]), what
    torch.cuda.synchronize()
