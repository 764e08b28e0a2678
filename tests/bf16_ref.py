"""Host restatement of the fp32 -> bfloat16 storage conversion (csrc/cb_common.h f32_to_bf16 / pack4_bf16) and of its inverse, on bit patterns:
numpy, integers only — no floating-point unit, no denormal mode and no NaN canonicalisation of the host takes part.

rne_bits is round-to-nearest-even of the fp32 pattern to its upper 16 bits; every NaN gives a NaN (the quieted upper half).  The tables are the
fp32 patterns at the edges where such a conversion goes wrong: for a set of upper halves H, every low half L at which the rounding decision changes
(0x0000 exact, 0x0001 just above, 0x7FFF just below the tie, 0x8000 the tie, 0x8001 just above it, 0xFFFF the largest)."""
import numpy as np

LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def is_nan_bits(u32):
    """fp32 patterns that are NaNs: exponent all ones, significand not zero."""
    return (np.asarray(u32, dtype=np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def is_nan_bits16(u16):
    return (np.asarray(u16, dtype=np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def current_formula_bits(u32):
    """The formula the library used before it kept NaN: u += 0x7FFF + ((u >> 16) & 1); return u >> 16 — in uint32 arithmetic (the sum wraps).
    Right for every non-NaN pattern; a NaN whose sum carries out of the significand comes back as an infinity or a zero."""
    u = np.asarray(u32, dtype=np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFFFFFF)
    return (u >> np.uint64(16)).astype(np.uint16)


def rne_bits(u32):
    """uint32 fp32 patterns -> uint16 bf16 patterns, round to nearest, ties to even.  Carries run into the exponent (0x3F7FFFFF -> 0x3F80) and on to
    infinity (0x7F7F8000 -> 0x7F80); subnormals round like every other value (the significand is just bits); NaN -> upper half | 0x0040 (a quiet NaN)."""
    u = np.asarray(u32, dtype=np.uint32)
    out = current_formula_bits(u)
    return np.where(is_nan_bits(u), ((u >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), out).astype(np.uint16)


def widen_bits(u16):
    """uint16 bf16 patterns -> the uint32 fp32 patterns of the same values (exact)."""
    return np.asarray(u16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)


def edge_table(uppers):
    """The fp32 patterns H << 16 | L for H in uppers (in their order) and L in LOW_HALVES: uint32 [len(uppers) * 6], L fastest."""
    h = np.asarray(list(uppers) if not isinstance(uppers, np.ndarray) else uppers, dtype=np.uint32)
    low = np.asarray(LOW_HALVES, dtype=np.uint32)
    return ((h[:, None] << np.uint32(16)) | low[None, :]).reshape(-1)


# ---- the named sets of upper halves ------------------------------------------------------------------------------------------------------------------
ALL = np.arange(0x10000, dtype=np.uint32)

# normal values of at least 2^-100 whose bf16 rounding is finite: both signs, exponent field in {27, 126, 127, 128, 253}, the seven significand bits of
# the upper half in {0x00, 0x01, 0x3F, 0x40, 0x7E, 0x7F}.  Such a value crosses the GEMMs' three-limb split exactly (every limb is a normal fp32).
GEMM_EXPONENTS = (27, 126, 127, 128, 253)
GEMM_MANTISSAS = (0x00, 0x01, 0x3F, 0x40, 0x7E, 0x7F)
GEMM_OPERAND = np.asarray([(s << 15) | (e << 7) | m for s in (0, 1) for e in GEMM_EXPONENTS for m in GEMM_MANTISSAS], dtype=np.uint32)

# what may only be ADDED in a GEMM epilogue, never multiplied on the matrix cores: 0x7F7F / 0xFF7F (with the low halves at or above 0x8000 these are the
# finite values that round up to infinity), the infinities' upper halves 0x7F80 / 0xFF80 (low half 0: the infinity; any other low half: a NaN whose
# upper half is an infinity's) and further NaN upper halves.
ADDEND_ONLY = np.asarray([0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x7FFF, 0xFFFF], dtype=np.uint32)


def addend_table():
    """edge_table(GEMM_OPERAND + ADDEND_ONLY): 402 patterns.  (The 0x7F7F / 0xFF7F rows also hold the three low halves below the tie: finite values
    within 2^-8 of FLT_MAX that stay finite — as addends they are as good as any.)"""
    return edge_table(np.concatenate([GEMM_OPERAND, ADDEND_ONLY]))


def same(got_u16, want_u16, src_nan):
    """Bit equality where the source is not a NaN, "is a NaN" where it is.  Returns the boolean array of agreeing elements."""
    got, want = np.asarray(got_u16, dtype=np.uint16), np.asarray(want_u16, dtype=np.uint16)
    return np.where(np.asarray(src_nan, dtype=bool), is_nan_bits16(got), got == want)


def same_or_zero(got_u16, want_u16, src_nan):
    """same(), except that a zero may have either sign (a sum 0 + (-0) is +0)."""
    got, want = np.asarray(got_u16, dtype=np.uint16), np.asarray(want_u16, dtype=np.uint16)
    both_zero = ((got & np.uint16(0x7FFF)) == 0) & ((want & np.uint16(0x7FFF)) == 0)
    return same(got, want, src_nan) | (both_zero & ~np.asarray(src_nan, dtype=bool))


def describe(ok, src_u32, got_u16, want_u16, limit=8):
    """The first disagreements as text: source pattern -> got (want)."""
    bad = np.flatnonzero(~np.asarray(ok).reshape(-1))
    s, g, w = np.asarray(src_u32).reshape(-1), np.asarray(got_u16).reshape(-1), np.asarray(want_u16).reshape(-1)
    return f'{bad.size} wrong: ' + ', '.join(f'{int(s[i]):#010x} -> {int(g[i]):#06x} (want {int(w[i]):#06x})' for i in bad[:limit])
