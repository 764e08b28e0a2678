"""GPU: every kernel that stores or reads bf16 rows against the integer restatement of the conversion (tests/bf16_ref.py; tests/test_bf16_ref_host.py
holds that to torch's CPU conversion), on bit patterns at the rounding edges: ties to even and to odd, low halves next to the tie, carries into the
exponent and on to infinity, subnormals, signed zeros, infinities and NaN.  bf16 results are compared as uint16 (torch.equal on bf16 tensors sees
neither a NaN nor the sign of a zero): bit for bit where the source is not a NaN, "is a NaN" where it is.

  a. the row pack cb_gather_rows_bf16_f32 (send buffer of the bf16 halo wire): vector path, every reason for the scalar path, both grid-stride loops;
  b. cb_gemm_nn_bf16out_f32, one case per kernel instantiation (asserted from the dispatch predicates of cb_gemm.hip / cb_gemm_limb.hip, restated
     here), vector and scalar store tails: exact products, the addend route (infinities, NaN, round-up-to-infinity), random operands;
  c. the layer backward's bf16 output (k_trunk_bwd<0, true>);
  d. the readers: cb_spmm_csr_f32 over bf16 rows widens every pattern exactly, at every lane width, in the row-block and in the hub kernels."""
import functools
import os

import numpy as np
import pytest
import torch

import bf16_ref as br

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _f32(u32):
    """CPU float32 tensor with exactly these bits (no floating-point operation touches them)."""
    a = np.ascontiguousarray(u32, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).view(torch.float32)


def _u16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _bits_of(x):
    """float32 numpy array -> its uint32 patterns."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _table():
    """edge_table(ALL) as uint32 [1536, 256] on the host and as the float32 device matrix with those bits.  Shared; nobody writes to either."""
    t = br.edge_table(br.ALL).reshape(1536, 256)
    dev = _f32(t).to(DEV)
    t.setflags(write=False)
    return t, dev


# ---- a. the row pack ------------------------------------------------------------------------------------------------------------------------------------
GRID_CAP = 2048 * 256      # csrc/cb_reduce.h grid_for: at most kMaxBlocks = 2048 blocks of kBlock = 256 threads; more work items than this loop


def _pack_vec_ok(src, ld, d, out, bf16):
    """vec_ok of cb_gather_rows_bf16_f32 / cb_gather_rows_f32 (csrc/cb_elementwise.hip)."""
    return src.data_ptr() % 16 == 0 and out.data_ptr() % (8 if bf16 else 16) == 0 and d % 4 == 0 and ld % 4 == 0


def _check_pack(src_bits, src, ld, d, idx, want_vec, out_offset=0):
    """Both forms of the row pack through the C ABI.  src_bits: the logical [rows, d] matrix as uint32; src: the device tensor whose first element is
    the matrix's (rows ld apart); the output starts out_offset elements into a buffer whose other elements must come back untouched."""
    from gnn_tail_generalization_amd import _lib
    lib = _lib.load()
    n = int(idx.numel())
    want32 = src_bits[idx.numpy()].reshape(-1)
    nan = br.is_nan_bits(want32)
    idx_d = idx.to(DEV)
    for bf16 in (True, False):
        dt, fill = (torch.int16, 0x5A5A) if bf16 else (torch.int32, 0x5A5A5A5A)
        buf = torch.full((out_offset + n * d + 8,), fill, dtype=dt, device=DEV)
        out = buf[out_offset:out_offset + n * d]
        assert _pack_vec_ok(src, ld, d, out, bf16) == want_vec, (bf16, src.data_ptr() % 16, out.data_ptr() % 16, d, ld)
        fn = lib.cb_gather_rows_bf16_f32 if bf16 else lib.cb_gather_rows_f32
        with torch.cuda.device(DEV):
            _lib.check(fn(_lib.ptr(src), ld, _lib.ptr(idx_d), n, d, _lib.ptr(out), _lib.stream_ptr()), 'cb_gather_rows')
        got = buf.cpu().numpy()
        assert (got[:out_offset] == fill).all() and (got[out_offset + n * d:] == fill).all(), 'wrote outside its output'
        got = got[out_offset:out_offset + n * d]
        if bf16:
            want = br.rne_bits(want32)
            ok = br.same(got.view(np.uint16), want, nan)
            assert ok.all(), br.describe(ok, want32, got.view(np.uint16), want)
        else:
            assert np.array_equal(got.view(np.uint32), want32)      # the fp32 form copies bits


def _reshaped(d):
    """The table as a [rows, d] matrix, zero-padded at the end (uint32)."""
    flat = _table()[0].reshape(-1)
    rows = -(-flat.size // d)
    out = np.zeros(rows * d, dtype=np.uint32)
    out[:flat.size] = flat
    return out.reshape(rows, d)


def _shuffled_rows(rows, seed, extra=64):
    """Every row once in a random order, `extra` of them again, and a reversed run."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(rows, generator=g)
    return torch.cat([perm, perm[:extra], torch.arange(min(rows, 300) - 1, -1, -1)])


def test_row_pack_vector_path():
    from gnn_tail_generalization_amd import ops
    bits, x = _table()
    idx = _shuffled_rows(1536, 1)
    assert len(set(idx.tolist())) == 1536 and idx.numel() > 1536
    _check_pack(bits, x, 256, 256, idx, want_vec=True)
    assert bits[765, 0] == 0x7F800000
    _check_pack(bits, x, 256, 256, torch.tensor([765]), want_vec=True)             # n_idx = 1 (row 765: upper halves from 0x7F80 - an infinity, then NaN)
    # the Python entry: the same rows, one row, no row
    for sel in (idx, idx[:1], idx[:0]):
        want32 = bits[sel.numpy()]
        out = ops.gather_rows_by_index(x, sel.to(DEV), out_bf16=True)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (sel.numel(), 256)
        ok = br.same(_u16(out).reshape(want32.shape), br.rne_bits(want32), br.is_nan_bits(want32))
        assert ok.all(), br.describe(ok, want32, _u16(out), br.rne_bits(want32))
        assert np.array_equal(_u32(ops.gather_rows_by_index(x, sel.to(DEV))).reshape(want32.shape), want32)


@pytest.mark.parametrize('why', ['d7', 'd8_ld9', 'src_off1', 'out_off1', 'd1'])
def test_row_pack_scalar_path(why):
    bits, x = _table()
    if why == 'd7':            # d % 4 != 0
        m = _reshaped(7)
        _check_pack(m, _f32(m).to(DEV), 7, 7, _shuffled_rows(m.shape[0], 2), want_vec=False)
    elif why == 'd8_ld9':      # ld % 4 != 0
        m = _reshaped(8)
        wide = np.zeros((m.shape[0], 9), dtype=np.uint32)
        wide[:, :8] = m
        _check_pack(m, _f32(wide).to(DEV), 9, 8, _shuffled_rows(m.shape[0], 3), want_vec=False)
    elif why == 'src_off1':    # src one float off a 16-byte boundary
        buf = _f32(np.concatenate([np.zeros(1, dtype=np.uint32), bits.reshape(-1)])).to(DEV)
        _check_pack(bits, buf[1:], 256, 256, _shuffled_rows(1536, 4), want_vec=False)
    elif why == 'out_off1':    # out one element off: out % 8 != 0 (bf16), out % 16 != 0 (fp32)
        _check_pack(bits, x, 256, 256, _shuffled_rows(1536, 5), want_vec=False, out_offset=1)
    else:                      # d = 1
        m = bits.reshape(-1, 1)
        _check_pack(m, x.reshape(-1, 1), 1, 1, _shuffled_rows(m.shape[0], 6), want_vec=False)


def test_row_pack_grid_stride_loops():
    """More work items than the capped grid has threads: every thread of the vector path (quads) and of the scalar path (elements) takes a second turn."""
    g = torch.Generator().manual_seed(7)
    m = _table()[0].reshape(384, 1024)
    n_idx, d = 2100, 1024
    assert n_idx * (d // 4) == 537600 > GRID_CAP
    _check_pack(m, _table()[1].reshape(384, 1024), d, d, torch.randint(0, 384, (n_idx,), generator=g), want_vec=True)
    m = _reshaped(7)
    n_idx, d = 75000, 7
    assert n_idx * d == 525000 > GRID_CAP
    _check_pack(m, _f32(m).to(DEV), d, d, torch.randint(0, m.shape[0], (n_idx,), generator=g), want_vec=False)


# ---- b. the GEMM with bf16 output -----------------------------------------------------------------------------------------------------------------------
def _limb3_nn_eligible(a, lda, b, ldb, N, K):
    """limb3_nn_eligible (csrc/cb_gemm_limb.hip) behind use_limb3() (csrc/cb_gemm.hip: the three-limb path unless CB_GEMM_PLAIN_F32 is set)."""
    return (os.environ.get('CB_GEMM_PLAIN_F32') is None and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and lda % 4 == 0 and ldb % 4 == 0
            and K % 4 == 0 and N % 4 == 0 and K > 0 and lda < (1 << 22) and ldb < (1 << 22))


def _nn_kernel(a, lda, b, ldb, M, N, K):
    """The kernel cb_gemm_nn_bf16out_f32 launches, from its dispatch (csrc/cb_gemm.hip cb_gemm_nn_bf16out_f32: limb3_nn_eligible, then N <= 64;
    csrc/cb_gemm_limb.hip launch_nn_limb3: N <= 64, then N > 128 and the `fills` product, no second output / operand dropout / row subset here)."""
    if _limb3_nn_eligible(a, lda, b, ldb, N, K):
        if N <= 64:
            return 'k_gemm_nn_l3<4,1,true>'
        fills = ((M + 127) // 128) * ((N + 255) // 256) >= 256
        return 'k_gemm_nn_l3<2,2,true,4>' if N > 128 and fills else 'k_gemm_nn_l3<2,2,true>'
    return 'launch_nn<4,1,true>' if N <= 64 else 'launch_nn<2,2,true>'


def _c_vec_ok(c, ldc, addend, ld_add, bf16):
    """c_vec_ok of launch_nn_l3_t / launch_nn: vector stores (and vector addend loads) in nn_epilogue; 0 = the scalar tail."""
    return c.data_ptr() % (8 if bf16 else 16) == 0 and ldc % 4 == 0 and (addend is None or (addend.data_ptr() % 16 == 0 and ld_add % 4 == 0))


class _Gemm:
    """One shape's operands on the device and its output placement: how = 'plain' (ldc = N), 'ldc+2' (ldc = N + 2) or 'c+1' (C one element off)."""

    def __init__(self, M, K, N, how, kernel):
        self.M, self.K, self.N, self.how = M, K, N, how
        self.ldc = N + 2 if how == 'ldc+2' else N
        self.off = 1 if how == 'c+1' else 0
        self.kernel = kernel

    def run(self, a, b, rowscale=None, addend=None, relu=False, bf16=True):
        """cb_gemm_nn_bf16out_f32 (or cb_gemm_nn_f32) through the C ABI without a workspace -> the [M, N] output's bit patterns."""
        from gnn_tail_generalization_amd import _lib
        lib = _lib.load()
        M, K, N, ldc = self.M, self.K, self.N, self.ldc
        assert lib.cb_gemm_nn_splitk_workspace_bytes(M, N, K) == 0
        assert _nn_kernel(a, K, b, N, M, N, K) == self.kernel
        dt, fill = (torch.int16, 0x5A5A) if bf16 else (torch.int32, 0x5A5A5A5A)
        buf = torch.full((self.off + M * ldc + 8,), fill, dtype=dt, device=DEV)
        c = buf[self.off:]
        ld_add = N if addend is not None else 0
        assert _c_vec_ok(c, ldc, addend, ld_add, bf16) == (self.how == 'plain' and N % 4 == 0), self.how
        fn = lib.cb_gemm_nn_bf16out_f32 if bf16 else lib.cb_gemm_nn_f32
        with torch.cuda.device(DEV):
            _lib.check(fn(_lib.ptr(a), K, _lib.ptr(b), N, _lib.ptr(c), ldc, M, N, K, _lib.ptr(rowscale), _lib.ptr(addend), ld_add, None, int(relu),
                          None, 0, _lib.stream_ptr()), 'cb_gemm_nn')
        got = buf.cpu().numpy()
        body = got[self.off:self.off + M * ldc].reshape(M, ldc)
        assert (got[:self.off] == fill).all() and (got[self.off + M * ldc:] == fill).all() and (body[:, N:] == fill).all(), 'wrote outside its output'
        return np.ascontiguousarray(body[:, :N]).view(np.uint16 if bf16 else np.uint32)


# (M, K, N, kernel): one shape per instantiation of the bf16-output NN kernels
GEMM_SHAPES = [(300, 64, 256, 'k_gemm_nn_l3<2,2,true>'),
               (130, 16, 64, 'k_gemm_nn_l3<4,1,true>'), (65, 8, 4, 'k_gemm_nn_l3<4,1,true>'),
               (16257, 16, 260, 'k_gemm_nn_l3<2,2,true,4>'),      # 128 row tiles x 2 column tiles = 256 wide tiles, overhang in M and in N
               (130, 17, 129, 'launch_nn<2,2,true>'), (65, 5, 7, 'launch_nn<4,1,true>')]      # K, N not multiples of 4: fp32-input MFMA kernels
# ... and the scalar store tail of nn_epilogue (c_vec_ok == 0) of the <2, 2> and <4, 1> three-limb kernels
GEMM_CASES = [s + ('plain',) for s in GEMM_SHAPES] + [s + (how,) for s in GEMM_SHAPES[:3] for how in ('ldc+2', 'c+1')]
GEMM_IDS = [f'{M}x{K}x{N}-{how}' for M, K, N, _k, how in GEMM_CASES]


@functools.lru_cache(maxsize=None)
def _exact_operands(M, K, N):
    """A[m, m % K] = s_m (cycling over 1, -1, 2, 0.5), zeros elsewhere; B[k, n] = edge_table(GEMM_OPERAND)[(k * N + n) % T].  Every product is a
    power of two times a table value and every sum has one non-zero term: fp32(A @ B)[m, n] = s_m * B[m % K, n] whatever the summation order."""
    tbl = br.edge_table(br.GEMM_OPERAND)
    b_bits = tbl[np.arange(K * N) % tbl.size].reshape(K, N)
    s = np.asarray([1.0, -1.0, 2.0, 0.5], dtype=np.float32)[np.arange(M) % 4]
    a = np.zeros((M, K), dtype=np.float32)
    a[np.arange(M), np.arange(M) % K] = s
    return s, b_bits, torch.from_numpy(a).to(DEV), _f32(b_bits).to(DEV)


def _exact_acc(s, b_bits, K, limb):
    """The fp32 accumulator of the exact product: s_m * B[m % K, n].  On the three-limb path the high limb of B (its bf16 rounding) meets s_m first:
    where that product alone overflows (s_m = 2 against a high limb of 2^127: B within 2^-8 of 2^127) the accumulator is that infinity — the limit
    of the split profiles/bf16_rounding.md notes; the value itself rounds to the same bf16 infinity, only a row scale below one tells the two."""
    rows = np.arange(s.size) % K
    with np.errstate(over='ignore'):
        acc = s[:, None] * b_bits[rows].view(np.float32)
        if limb:
            hi = s[:, None] * br.widen_bits(br.rne_bits(b_bits[rows])).view(np.float32)
            acc = np.where(np.isinf(hi), hi, acc)
    return acc.astype(np.float32)


@pytest.mark.parametrize('M,K,N,kernel,how', GEMM_CASES, ids=GEMM_IDS)
def test_gemm_bf16out_exact_products(M, K, N, kernel, how):
    g = _Gemm(M, K, N, how, kernel)
    s, b_bits, a, b = _exact_operands(M, K, N)
    acc = _exact_acc(s, b_bits, K, limb=kernel.startswith('k_gemm_nn_l3'))
    assert np.isfinite(s[:, None] * b_bits[np.arange(M) % K].view(np.float32)).all() and not np.isnan(acc).any()
    # no epilogue
    want = br.rne_bits(_bits_of(acc))
    got = g.run(a, b)
    assert np.array_equal(got, want), br.describe(got == want, _bits_of(acc), got, want)
    # a power-of-two row scale: one more exact product (or an overflow to infinity, the same on both sides)
    rs = np.asarray([0.5, 2.0, 0.25, 1.0, 4.0], dtype=np.float32)[np.arange(M) % 5]
    with np.errstate(over='ignore'):
        scaled = (acc * rs[:, None]).astype(np.float32)
    want = br.rne_bits(_bits_of(scaled))
    got = g.run(a, b, rowscale=torch.from_numpy(rs).to(DEV))
    assert np.array_equal(got, want), br.describe(got == want, _bits_of(scaled), got, want)
    # ReLU: a negative result becomes a zero of either sign
    relu = np.where(acc < 0, np.float32(0), acc).astype(np.float32)
    want = br.rne_bits(_bits_of(relu))
    got = g.run(a, b, relu=True)
    ok = br.same_or_zero(got, want, np.zeros(want.shape, dtype=bool))
    assert ok.all() and (got[acc < 0] & 0x7FFF == 0).all(), br.describe(ok, _bits_of(relu), got, want)


@pytest.mark.parametrize('M,K,N,kernel,how', GEMM_CASES, ids=GEMM_IDS)
def test_gemm_bf16out_addend_route(M, K, N, kernel, how):
    """B = 0 and a finite A: the accumulator is a zero and the stored value is the addend — finite edges, values that round up to infinity, infinities
    and NaN (no subnormals: whether the epilogue's fp32 additions keep them is the compiler's denormal mode, not the conversion's business)."""
    g = _Gemm(M, K, N, how, kernel)
    tbl = br.addend_table()
    add_bits = tbl[np.arange(M * N) % tbl.size].reshape(M, N)
    assert set(tbl.tolist()) == set(add_bits.reshape(-1).tolist()) or M * N < tbl.size
    a = torch.randn(M, K, generator=torch.Generator().manual_seed(1)).to(DEV)
    b = torch.zeros(K, N, device=DEV)
    nan = br.is_nan_bits(add_bits)
    want = br.rne_bits(add_bits)
    got = g.run(a, b, addend=_f32(add_bits).to(DEV))
    ok = br.same_or_zero(got, want, nan)
    assert ok.all(), br.describe(ok, add_bits, got, want)


@pytest.mark.parametrize('M,K,N,kernel', GEMM_SHAPES, ids=[f'{M}x{K}x{N}' for M, K, N, _k in GEMM_SHAPES])
def test_gemm_bf16out_random_operands_round_the_fp32_result(M, K, N, kernel):
    """randn operands, row scale and addend (the seeds of test_gpu_kernels.py::test_bf16_storage_kernels).  cb_gemm_nn_f32 and cb_gemm_nn_bf16out_f32
    run the same template up to OUT_BF16 on every shape here, so the bf16 output is the rounding of the fp32 output bit for bit:
      * three-limb path: both entries call launch_nn_limb3 with the same arguments but out_bf16, and each of its three returns
        (csrc/cb_gemm_limb.hip, `return out_bf16 ? launch_nn_l3_t<WM, WN, true...> : launch_nn_l3_t<WM, WN, false...>`) picks the same WM, WN, WTN for
        both; launch_nn_l3_t launches k_gemm_nn_l3<WM, WN, OUT_BF16, WTN, 1> for both (no second output, operand dropout or row subset here);
      * fp32-input path: launch_nn<4, 1> / launch_nn<2, 2> against launch_nn<4, 1, true> / launch_nn<2, 2, true> (csrc/cb_gemm.hip, the last two lines
        of both entries); without a workspace launch_nn's split-K branch is not taken, so both launch k_gemm_nn<WM, WN, ALIGNED, OUT_BF16, BK, WTN>.
    OUT_BF16 only chooses the store in nn_epilogue.  The fp32 kernel is held to fp64 by test_gpu_kernels.py; the bound of test_bf16_storage_kernels
    against the fp64 product is kept here as well."""
    g = _Gemm(M, K, N, 'plain', kernel)

    def rand(*shape, seed):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    a, b = rand(M, K, seed=1), rand(K, N, seed=2)
    rs, add = torch.rand(M, generator=torch.Generator().manual_seed(5)) + 0.5, rand(M, N, seed=3)
    ad, bd, rsd, addd = a.to(DEV), b.to(DEV), rs.to(DEV), add.to(DEV)
    for kw in (dict(), dict(rowscale=rsd, addend=addd), dict(rowscale=rsd, addend=addd, relu=True)):
        z32 = g.run(ad, bd, bf16=False, **kw)
        z16 = g.run(ad, bd, bf16=True, **kw)
        want = br.rne_bits(z32)
        assert np.array_equal(z16, want), (sorted(kw), br.describe(z16 == want, z32, z16, want))
        ref = a.double() @ b.double()
        if kw:
            ref = ref * rs.double().unsqueeze(1) + add.double()
        if kw.get('relu'):
            ref = torch.relu(ref)
        val = torch.from_numpy(br.widen_bits(z16).view(np.int32)).view(torch.float32).double()
        err = (val - ref).abs()
        print(f'{M}x{K}x{N} {sorted(kw)}: max |err| / (|ref| 2^-8 + 1e-6) = {(err / (ref.abs() * 2.0 ** -8 + 1e-6)).max().item():.4f}')
        assert (err <= ref.abs() * 2.0 ** -8 + 1e-6).all()


# ---- c. the layer backward's bf16 output ------------------------------------------------------------------------------------------------------------------
def test_layer_backward_bf16_output_rounds_the_gradient():
    """cb_trunk_layer_bwd_f32 with out_bf16 (k_trunk_bwd<0, true>, csrc/cb_trunk_bwd.hip) at p = 0, c_act = 1, c_mix = 0, no row scale, no second
    gradient, every ReLU bit set: thresh == 0 leaves gm = g, gy = bit ? c_act * gm : 0 = 1.0f * g, and the value handed to pack4_bf16 is gy * sc with
    sc = 1.0f — g itself (two exact products with one; a signalling NaN may come out quiet, a NaN it stays)."""
    from gnn_tail_generalization_amd import trunk
    rows, d = 201, 256                                   # four blocks of wave-per-row slabs, the last one ragged
    tbl = br.addend_table()
    g_bits = tbl[np.arange(rows * d) % tbl.size].reshape(rows, d)
    bits = torch.full((rows, d // 256, 4), -1, dtype=torch.int64, device=DEV)
    out, colsum = trunk._layer_bwd(_f32(g_bits).to(DEV), bits, None, None, False, 0.0, 1234, 0, 1.0, 0.0, False, out_bf16=True)
    assert out.dtype == torch.bfloat16 and colsum is None
    got, want = _u16(out).reshape(rows, d), br.rne_bits(g_bits)
    ok = br.same(got, want, br.is_nan_bits(g_bits))
    assert ok.all(), br.describe(ok, g_bits, got, want)
    # the fp32 form of the same call hands g through
    out32, _ = trunk._layer_bwd(_f32(g_bits).to(DEV), bits, None, None, False, 0.0, 1234, 0, 1.0, 0.0, False)
    nan = br.is_nan_bits(g_bits)
    got32 = _u32(out32).reshape(rows, d)
    assert np.array_equal(got32[~nan], g_bits[~nan]) and br.is_nan_bits(got32[nan]).all()


# ---- d. the readers widen exactly -------------------------------------------------------------------------------------------------------------------------
def _spmm_bf16_vec(h, ld_h, d, out, ld_out):
    """The lane width cb_spmm_csr_f32 picks for bf16 rows without running sums (csrc/cb_spmm.hip: al8 / al4, then d >= 256 / d >= 128)."""
    al8 = h.data_ptr() % 8 == 0 and out.data_ptr() % 16 == 0 and ld_h % 4 == 0 and ld_out % 4 == 0 and d % 4 == 0
    al4 = h.data_ptr() % 4 == 0 and out.data_ptr() % 8 == 0 and ld_h % 2 == 0 and ld_out % 2 == 0 and d % 2 == 0
    return 4 if al8 and d >= 256 else 2 if al4 and d >= 128 else 1


@pytest.mark.parametrize('d,view,vec', [(256, False, 4), (128, False, 2), (130, False, 2), (40, False, 1), (129, False, 1), (255, True, 1)],
                         ids=['d256-vec4', 'd128-vec2', 'd130-vec2', 'd40-vec1', 'd129-vec1', 'd255-view-vec1'])
def test_spmm_widens_every_bf16_pattern(d, view, vec):
    """Source rows: all 65 536 bf16 patterns (zero-padded to whole rows) and one row of zeros.  Output row i <= R has the single edge i -> i (row-block
    kernel); output row R + 1 + j has 40 edges to the zero row and one to pattern row j — above hub_threshold = 16, so the hub kernels sum it: both
    sum "zeros plus one value".  Expected fp32 bits: the pattern << 16 for normal values and infinities, a NaN for a NaN, a zero of either sign for a
    zero; subnormal patterns are not asserted (whether 0 + x keeps one is the kernels' denormal mode)."""
    from gnn_tail_generalization_amd.graph import CSRGraph
    width = d + 1 if view else d                         # view: columns 1.. of the 256-wide table (rows 2 bytes off a 4-byte boundary, ld = 256)
    R = -(-65536 // width)
    pat = np.zeros((R + 1) * width, dtype=np.uint16)
    pat[:65536] = np.arange(65536, dtype=np.uint16)
    pat = pat.reshape(R + 1, width)
    base = torch.from_numpy(pat.view(np.int16)).to(DEV).view(torch.bfloat16)
    h = base[:, 1:] if view else base
    src = pat[:, 1:] if view else pat
    T, n_rows = 16, 2 * R + 1
    rows = torch.cat([torch.arange(R + 1), (R + 1 + torch.arange(R)).repeat_interleave(41)])
    cols = torch.cat([torch.arange(R + 1), torch.cat([torch.full((R, 40), R), torch.arange(R).unsqueeze(1)], 1).reshape(-1)])
    G = CSRGraph.from_pairs(rows.to(DEV), cols.to(DEV), n_rows, R + 1, hub_threshold=T)
    deg = G.in_degrees().cpu()
    assert (deg[:R + 1] == 1).all() and (deg[R + 1:] == 41).all() and 41 > T and G._plan.n_hubs == R      # row-block rows and hub rows
    out = torch.full((n_rows, d), float('nan'), device=DEV)
    out.view(torch.int32).fill_(0x5A5A5A5A)
    assert h.stride(0) == width and _spmm_bf16_vec(h, h.stride(0), d, out, d) == vec
    assert G.spmm(h, out=out) is out
    got = _u32(out).reshape(n_rows, d)
    want = br.widen_bits(np.concatenate([src, src[:R]], 0))
    p = np.concatenate([src, src[:R]], 0)
    mag = p & np.uint16(0x7FFF)
    nan, zero, subnormal = br.is_nan_bits16(p), mag == 0, (mag != 0) & (mag < 0x0080)
    ok = np.where(nan, br.is_nan_bits(got), np.where(zero, (got & np.uint32(0x7FFFFFFF)) == 0, got == want)) | subnormal
    assert ok.all(), br.describe(ok, want, got >> 16, want >> 16)
    assert nan.sum() >= 254 and zero.sum() >= 2 and (~(nan | zero | subnormal)).sum() >= 2 * 64000      # nothing was masked away wholesale
