"""Host: tests/bf16_ref.py (the integer restatement of the bf16 storage conversion the GPU tests hold the kernels to) against torch's own CPU
float32 -> bfloat16 conversion at every rounding edge, and the record of the defect the library's first formula had on NaN."""
import numpy as np
import torch

import bf16_ref as br


def _torch_bf16_bits(u32):
    x = torch.from_numpy(np.ascontiguousarray(u32).view(np.int32)).view(torch.float32)
    return x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_tables_hold_what_they_name():
    t = br.edge_table(br.ALL)
    assert t.dtype == np.uint32 and t.size == 65536 * 6 == 1536 * 256 and np.unique(t).size == t.size
    assert int(t[6 * 0x3F7F + 5]) == 0x3F7FFFFF and (~br.is_nan_bits(t)).sum() == 391682
    g = br.edge_table(br.GEMM_OPERAND)
    e = (g >> 23) & 0xFF
    assert g.size == 360 and e.min() == 27 and e.max() == 253 and not br.is_nan_bits(g).any()
    assert ((br.rne_bits(g) & 0x7FFF) < 0x7F80).all()                      # their bf16 rounding is finite
    a = br.addend_table()
    assert a.size == 402 and set(g.tolist()) <= set(a.tolist())
    r = br.rne_bits(a)
    for lo in (0x8000, 0x8001, 0xFFFF):                                      # finite values that round up to infinity, both signs
        assert 0x7F7F0000 | lo in a and 0xFF7F0000 | lo in a
        assert br.rne_bits(np.uint32(0x7F7F0000 | lo)) == 0x7F80 and br.rne_bits(np.uint32(0xFF7F0000 | lo)) == 0xFF80
    assert 0x7F800000 in a and 0xFF800000 in a and br.is_nan_bits(a).sum() == 5 * 5 + 3 and br.is_nan_bits16(r[br.is_nan_bits(a)]).all()
    for nan in (0x7F800001, 0xFF800001, 0x7FC00000, 0x7FFF8000, 0xFFFFFFFF):
        assert nan in a


def test_rne_bits_is_torch_conversion_at_every_edge():
    t = br.edge_table(br.ALL)
    nan = br.is_nan_bits(t)
    want, got = _torch_bf16_bits(t), br.rne_bits(t)
    assert np.array_equal(got[~nan], want[~nan]), br.describe(br.same(got, want, nan), t, got, want)
    assert br.is_nan_bits16(want[nan]).all() and br.is_nan_bits16(got[nan]).all()        # torch keeps every NaN a NaN; so does the restatement
    assert br.same(got, want, nan).all() and br.same_or_zero(got, want, nan).all()
    # the edges by name
    for src, dst in ((0x3F7FFFFF, 0x3F80), (0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81), (0x7F7F8000, 0x7F80),
                     (0x7F7F7FFF, 0x7F7F), (0xFF7FFFFF, 0xFF80), (0x00008000, 0x0000), (0x00018000, 0x0002), (0x007FFFFF, 0x0080), (0x80000000, 0x8000),
                     (0x7F800000, 0x7F80), (0xFF800000, 0xFF80)):
        assert int(br.rne_bits(np.uint32(src))) == dst, hex(src)


def test_same_tells_a_lost_nan_and_a_wrong_sign():
    src = np.asarray([0x7FFF8000, 0x80000000, 0x3F800000], dtype=np.uint32)
    nan = br.is_nan_bits(src)
    want = br.rne_bits(src)
    assert br.same(want, want, nan).all()
    assert br.same(np.asarray([0x7FC0, 0x8000, 0x3F80], dtype=np.uint16), want, nan).all()              # any NaN is a NaN
    assert br.same(np.asarray([0x8000, 0x8000, 0x3F80], dtype=np.uint16), want, nan).tolist() == [False, True, True]
    assert br.same(np.asarray([0x7FFF, 0x0000, 0x3F80], dtype=np.uint16), want, nan).tolist() == [True, False, True]
    assert br.same_or_zero(np.asarray([0x7FFF, 0x0000, 0x3F81], dtype=np.uint16), want, nan).tolist() == [True, True, False]
    assert not br.same_or_zero(np.asarray([0x0000], dtype=np.uint16), np.asarray([0x7FC0], dtype=np.uint16), np.asarray([True]))[0]


def test_widen_inverts_the_rounding_of_exact_values():
    x = br.widen_bits(np.arange(0x10000, dtype=np.uint32).astype(np.uint16))
    assert x.dtype == np.uint32 and np.array_equal(x, np.arange(0x10000, dtype=np.uint32) << 16)
    nan = br.is_nan_bits(x)
    assert np.array_equal(br.widen_bits(br.rne_bits(x))[~nan], x[~nan])
    # (a NaN comes back quieted: the same pattern but for bit 22)
    assert np.array_equal(br.widen_bits(br.rne_bits(x))[nan] | np.uint32(0x00400000), x[nan] | np.uint32(0x00400000))


def test_first_formula_loses_nan():
    """The record of the defect: u += 0x7FFF + ((u >> 16) & 1); u >> 16 carries a NaN into an infinity or, through the sign bit, into a zero.
    An assertion about that arithmetic — the library no longer computes it for a NaN (tests/test_gpu_bf16_storage.py holds the kernels to that)."""
    for src, dst in ((0x7F800001, 0x7F80), (0xFF800001, 0xFF80), (0x7FFF8000, 0x8000), (0xFFFFFFFF, 0x0000)):
        got = int(br.current_formula_bits(np.uint32(src)))
        assert got == dst and br.is_nan_bits(np.uint32(src)) and not br.is_nan_bits16(np.uint16(got)), hex(src)
    assert int(br.current_formula_bits(np.uint32(0x7FC00000))) == 0x7FC0                  # the canonical quiet NaN survives it
    # which NaNs it loses, exactly: the upper half of an infinity while the sum does not carry (low half up to the tie: the upper half is even, 0x7FFF
    # is added), and the upper half all ones when it does (low half from the tie on: the upper half is odd, 0x8000 is added)
    t = br.edge_table(br.ALL)
    nan = br.is_nan_bits(t)
    lost = nan & ~br.is_nan_bits16(br.current_formula_bits(t))
    up, lo = (t >> 16) & 0x7FFF, t & 0xFFFF
    assert np.array_equal(lost, nan & (((up == 0x7F80) & (lo <= 0x8000)) | ((up == 0x7FFF) & (lo >= 0x8000))))
    # and it is right wherever the source is not a NaN
    assert np.array_equal(br.current_formula_bits(t)[~nan], _torch_bf16_bits(t)[~nan])
