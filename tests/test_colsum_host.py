"""Host: the oracle's restatement of the two-stage column-sum order (oracle/coldbrew_oracle.py colsum_two_stage).  It is exact where every order is,
and on the float summands of tests/test_gpu_colsum_order.py (tests/colsum_cases.py: same seeds, built on the CPU) it can be told from a plain
float32 sum and from the same order with the row lanes of a block reversed — so the device test, which holds the kernels to it with torch.equal,
does tell one order from another."""
import numpy as np
import pytest

import colsum_cases as cc
import coldbrew_oracle as orc

BIG_ROW = [s for s in cc.ROW_CASES if s[0] >= 65]
BIG_ACT = [s for s in cc.ACT_SHAPES if s[0] >= 65]


@pytest.mark.parametrize('row_lanes', [4, 25, 128])
@pytest.mark.parametrize('rows,d', [(1, 7), (5, 256), (64, 40), (65, 256), (1037, 40), (16449, 8), (2048 * 64 + 77, 4)])
def test_integer_summands_give_the_exact_column_sums(rows, d, row_lanes):
    x = np.random.default_rng(rows + d).integers(-9, 10, (rows, d))
    got = orc.colsum_two_stage(x.astype(np.float32), row_lanes)
    assert got.dtype == np.float32 and got.shape == (d,)
    assert np.array_equal(got.astype(np.int64), x.sum(0, dtype=np.int64))
    assert np.array_equal(got, orc.colsum_two_stage(x.astype(np.float32), row_lanes, reverse_lanes=True))


def test_block_and_lane_layout():
    """65 rows -> blocks of 33 and 32 rows; with 4 row lanes, lane j of block 0 holds rows j, j + 4, ...: powers of two that only one order adds without loss."""
    x = np.zeros((65, 1), dtype=np.float32)
    x[0], x[4], x[1] = 2.0 ** 24, 1.0, 1.0      # lane 0: 2^24 + 1 -> 2^24 (lost); lane 1: 1; partial = 2^24 + 1 -> 2^24
    assert orc.colsum_two_stage(x, 4)[0] == 2.0 ** 24
    x[:] = 0
    x[1], x[5], x[0] = 1.0, 1.0, 2.0 ** 24      # lane 1: 2; partial = 2^24 + 2, exact
    assert orc.colsum_two_stage(x, 4)[0] == 2.0 ** 24 + 2
    x[:] = 0
    x[32], x[33] = 2.0 ** 24, 1.0               # rows 32 (block 0) and 33 (block 1) meet in the finish only: 2^24 + 1 -> 2^24
    assert orc.colsum_two_stage(x, 4)[0] == 2.0 ** 24
    assert cc.act_row_lanes(7) == 128 and cc.act_row_lanes(40) == 25 and cc.act_row_lanes(256) == 4


def _told_apart(x, row_lanes):
    pinned = orc.colsum_two_stage(x, row_lanes)
    assert np.any(pinned != x.sum(0, dtype=np.float32)), 'equals the plain float32 column sum'
    assert np.any(pinned != orc.colsum_two_stage(x, row_lanes, reverse_lanes=True)), 'equals the reversed lane order'


@pytest.mark.parametrize('rows,d,p', BIG_ROW)
@pytest.mark.parametrize('entry', cc.ENTRIES)
def test_trunk_summands_tell_the_order_apart(entry, rows, d, p):
    for _name, x in cc.summands(entry, rows, d, p):
        _told_apart(x, 4)


@pytest.mark.parametrize('rows,d', BIG_ACT)
def test_act_bwd_summands_tell_the_order_apart(rows, d):
    _told_apart(cc.make_act(rows, d)['sum'], cc.act_row_lanes(d))
