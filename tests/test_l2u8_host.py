"""The arithmetic the uint8 L2 descriptor rows (sf_params.desc_type 2) rest on, without a GPU: for rows of integers in
0 .. 255 the oracle's float32 squared distance -- the ordered, unfused sum of the squared differences, sfo_l2sq_row -- is
the integer sum, because every partial sum of at most 258 squares of at most 255^2 is an integer below 2^24; and that
integer is |s_a|^2 + |s_b|^2 - 2 s_a . s_b on the rows shifted by 128 into int8, which is what k_match_u8.hip computes on
the int8 matrix cores."""
import numpy as np

from multi_robot_slam_separators_amd import _abi, synth


def _f32_ordered_sum(a, b):
    """float32 sum over the dimensions in order, multiply and add rounded separately (the oracle's loop)."""
    a, b = a.astype(np.float32), b.astype(np.float32)
    s = np.zeros(a.shape[0], np.float32)
    for c in range(a.shape[1]):
        d = (a[:, c] - b[:, c]).astype(np.float32)
        s = (s + (d * d).astype(np.float32)).astype(np.float32)
    return s


def _int_sum(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).sum(axis=1)


def _rows(seed, n, dims):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, dims), dtype=np.uint8)
    b = rng.integers(0, 256, size=(n, dims), dtype=np.uint8)
    a[0] = 0; b[0] = 255            # the largest distance there is
    a[1] = 255; b[1] = 0
    a[2] = b[2]                     # ... and the smallest
    a[3] = 0; b[3] = 1
    return a, b


def test_float32_ordered_sum_of_128_squares_is_the_integer_sum():
    a, b = _rows(1, 400, 128)
    want = _int_sum(a, b)
    got = _f32_ordered_sum(a, b)
    assert want[0] == 128 * 255 * 255 == 8323200 and want[2] == 0 and want[3] == 128
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))
    # any other summation order gives the same float32: reversed, and pairwise
    assert np.array_equal(_f32_ordered_sum(a[:, ::-1], b[:, ::-1]), got)
    d = (a.astype(np.float32) - b.astype(np.float32)) ** 2
    while d.shape[1] > 1:
        d = (d[:, 0::2] + d[:, 1::2]).astype(np.float32)
    assert np.array_equal(d[:, 0], got)


def test_shifted_int8_identity_equals_the_integer_sum():
    a, b = _rows(2, 400, 128)
    sa, sb = (a ^ 0x80).view(np.int8).astype(np.int32), (b ^ 0x80).view(np.int8).astype(np.int32)
    assert np.array_equal(sa, a.astype(np.int32) - 128)                 # XOR 0x80 per byte is x - 128 as int8
    i32 = dict(axis=1, dtype=np.int32)                                  # all of it fits int32, as in the kernel
    na, nb, dot = (sa * sa).sum(**i32), (sb * sb).sum(**i32), (sa * sb).sum(**i32)
    assert (na + nb - 2 * dot).dtype == np.int32 and na.max() <= 128 * 128 * 128 and np.abs(dot).max() <= 128 * 128 * 128
    assert np.array_equal((na + nb - 2 * dot).astype(np.int64), _int_sum(a, b))
    assert (na + nb - 2 * dot).max() == 8323200


def test_258_dimensions_is_the_last_exact_width():
    assert 258 * 255 * 255 < 2 ** 24 <= 259 * 255 * 255
    for dims, exact in ((258, True), (259, False)):
        a, b = np.zeros((1, dims), np.uint8), np.full((1, dims), 255, np.uint8)
        assert (int(_f32_ordered_sum(a, b)[0]) == int(_int_sum(a, b)[0])) == exact
    a, b = _rows(3, 50, 258)
    assert np.array_equal(_f32_ordered_sum(a, b).astype(np.int64), _int_sum(a, b))


def test_synthetic_uint8_rows():
    rng = np.random.default_rng(4)
    fa = synth.make_keyframe(rng, 40, 32)
    plain = synth.u8_descriptors(fa, 128)
    assert plain.desc.dtype == np.uint8 and plain.desc.shape == (40, 128) == (40, _abi.SF_DESC_BYTES_U8)
    bits = np.unpackbits(fa.desc, axis=1)[:, :128]
    assert np.array_equal(plain.desc, np.where(bits == 1, 192, 64))    # 128 +- 64 by the bits of the binary twin
    assert plain.xyz is fa.xyz or np.array_equal(plain.xyz, fa.xyz)
    jit = synth.u8_descriptors(fa, 128, rng, 70)                       # (64 - 70 < 0 and 192 + 70 > 255: the clip is reached)
    assert jit.desc.dtype == np.uint8 and jit.desc.shape == (40, 128)
    delta = jit.desc.astype(np.int32) - plain.desc.astype(np.int32)
    assert np.abs(delta).max() <= 70 and len(np.unique(delta)) > 100
    assert jit.desc.min() == 0 and jit.desc.max() == 255
    assert plain.c_struct().cols == 128
