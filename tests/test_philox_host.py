"""Host: the oracle's restatement of the dropout keep-mask (Philox4x32-10 keyed by the 64-bit seed, counter = flat element index / 4) against the
published known answers of Random123 and against the project's own parameterisation; thresholds, keep rate, shard property and the bits of the seed and
of the counter that nothing else in the suite reaches.  tests/test_gpu_philox.py then holds every mask-drawing kernel to this restatement."""
import numpy as np
import pytest

import coldbrew_oracle as orc


def _words(s):
    return np.array([int(w, 16) for w in s.split()], dtype=np.uint32)


# Random123 kat_vectors, philox4x32 10 rounds: counter words ; key words -> output words
@pytest.mark.parametrize('ctr,key,out', [
    ('0 0 0 0', '0 0', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_random123_known_answers(ctr, key, out):
    got = orc.philox4x32_10(*_words(ctr), *_words(key))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert np.array_equal(got, _words(out))


def test_philox_is_vectorised():
    c = np.array([[0, 0xffffffff, 0x243f6a88]], dtype=np.uint64).T * np.ones((1, 2), dtype=np.uint64)      # [3, 2]
    got = orc.philox4x32_10(c, [[0], [0xffffffff], [0x85a308d3]], [[0], [0xffffffff], [0x13198a2e]], [[0], [0xffffffff], [0x03707344]],
                            [[0], [0xffffffff], [0xa4093822]], [[0], [0xffffffff], [0x299f31d0]])
    assert got.shape == (3, 2, 4)
    assert np.array_equal(got[0, 1], _words('6627e8d5 e169c58d bc57ac4c 9b00dbd8'))
    assert np.array_equal(got[2, 0], _words('d16cfe09 94fdcceb 5001e420 24126ea1'))


# the project's parameterisation: counter (lo32(quad), hi32(quad), 0x243F6A88, 0x85A308D3), key (lo32(seed), hi32(seed))
@pytest.mark.parametrize('seed,quad,out', [
    (0, 0, '79cd4f3f c8cececd 51770eac a4080f77'),
    (123456789, 0, '2edd1389 947b49be 4231af6c 252ae05a'),
    (0x1234ABCD5, 1, '59cb393c 73087173 f27d4c22 b2cdaa71'),
    (0x1234ABCD5, 2 ** 32 + 7, 'c44264ff 7905d2ae 75d03d29 e3d4e925'),
    (2 ** 64 - 1, 2 ** 40, 'a551b859 6338683f 771656e0 6b535b83'),
])
def test_project_parameterisation(seed, quad, out):
    assert np.array_equal(orc.dropout_words(seed, quad), _words(out))
    assert np.array_equal(orc.philox4x32_10(quad & 0xFFFFFFFF, quad >> 32, 0x243F6A88, 0x85A308D3, seed & 0xFFFFFFFF, seed >> 32), _words(out))
    # the mask reads word i & 3 of quad i >> 2
    for p in (0.1, 0.5, 0.9):
        keep = orc.dropout_keep_mask((4,), p, seed, offset=4 * quad)
        assert np.array_equal(keep, _words(out) >= orc.dropout_threshold(p))


@pytest.mark.parametrize('p,thresh', [(0.1, 429496736), (0.3, 1288490240), (0.5, 2147483648), (1e-10, 0), (2.4e-10, 1), (0.99999999, 0xFFFFFFFF)])
def test_thresholds(p, thresh):
    assert orc.dropout_threshold(p) == thresh


def test_scale_is_float32_arithmetic():
    for p in (0.1, 0.3, 0.5, 0.999, 2.4e-10):
        s = orc.dropout_scale(p)
        assert isinstance(s, np.float32)
        assert s == np.float32(1) / (np.float32(1) - np.float32(p))
    assert orc.dropout_scale(0.5) == np.float32(2)


def test_word_equal_to_threshold_is_kept():
    """`>=`, not `>`: a word whose low eight bits are zero is float32(p) * 2^32 for an exact float32 p; at that p its element is kept, and at the next
    float32 above it is dropped."""
    seed = 20240607
    words = orc.dropout_words(seed, np.arange(4096)).reshape(-1)
    hits = np.flatnonzero(((words & np.uint32(0xFF)) == 0) & (words >= np.uint32(1 << 31)))
    assert hits.size > 0
    for i in hits[:8]:
        w = int(words[i])
        p = np.float32(w / 4294967296.0)
        assert orc.dropout_threshold(p) == w
        assert orc.dropout_keep_mask((1,), p, seed, offset=int(i))[0]
        p_up = np.nextafter(p, np.float32(1))
        assert orc.dropout_threshold(p_up) == w + 256
        assert not orc.dropout_keep_mask((1,), p_up, seed, offset=int(i))[0]


@pytest.mark.parametrize('p', [0.1, 0.3, 0.5])
def test_keep_rate_beyond_2_to_34(p):
    n = 1 << 20
    keep = orc.dropout_keep_mask((n,), p, 0x1234ABCD5, offset=2 ** 34 - 5)
    assert keep.dtype == np.bool_ and keep.shape == (n,)
    assert abs(float(keep.mean()) - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5      # fixed inputs: 0.47, 0.79 and 0.02 sigma


@pytest.mark.parametrize('offset', [0, 5, 2 ** 31 - 3, 2 ** 34 - 5, 2 ** 40 + 3])
def test_shards_reproduce_the_full_mask(offset):
    n, p, seed = 1027, 0.3, 0x1234ABCD5
    full = orc.dropout_keep_mask((n,), p, seed, offset=offset)
    for k in range(1, 9):
        assert np.array_equal(full[k:], orc.dropout_keep_mask((n - k,), p, seed, offset=offset + k))
    assert np.array_equal(full[:1024].reshape(4, 256), orc.dropout_keep_mask((4, 256), p, seed, offset=offset)[:, :])


def test_high_seed_and_counter_bits_matter():
    n, p = 4096, 0.5
    a = orc.dropout_keep_mask((n,), p, 0x1234ABCD5)
    assert not np.array_equal(a, orc.dropout_keep_mask((n,), p, 0x1234ABCD5 ^ (1 << 40)))
    assert not np.array_equal(a, orc.dropout_keep_mask((n,), p, 0x1234ABCD5 ^ (1 << 62)))
    assert not np.array_equal(a, orc.dropout_keep_mask((n,), p, 0x1234ABCD5, offset=4 << 32))      # quads differ in bit 32 only
    assert not np.array_equal(orc.dropout_words(7, 5), orc.dropout_words(7, 5 + (1 << 32)))
    assert not np.array_equal(orc.dropout_words(7, 5), orc.dropout_words(7 + (1 << 40), 5))


def test_device_seed_word_adds_mod_2_to_64():
    n, p = 1024, 0.5
    for seed, sd in [(1234567, 987654321), (0x1234ABCD5, 2 ** 32 - 1), (2 ** 64 - 1, 2), (2 ** 62 - 1, 2 ** 63)]:
        got = orc.dropout_keep_mask((n,), p, seed, seed_dev=sd)
        assert np.array_equal(got, orc.dropout_keep_mask((n,), p, (seed + sd) % 2 ** 64))
    # a carry out of the low key word reaches the high one
    assert np.array_equal(orc.dropout_words(0xFFFFFFFF + 1, 3), orc.philox4x32_10(3, 0, 0x243F6A88, 0x85A308D3, 0, 1))
