"""The argument for the matrix-core scan's lazy second best (k_match.hip: top2_update16, mf_repair_d2), in numpy.

The scan keeps, per column, the best row exactly (distance first, the lower index second) and, instead of the exact
second-best distance d2, the best distance d2' among the rows outside the best row's CLASS.  The class map is the kernel's:
register i of a lane's accumulator tuple holds row (i & 3) + 8 * (i >> 2) + 4 * h of a 32-row "from" tile (h = the lane
half); registers 0..14 form one class, register 15 (rows 27 and 31 of the tile) a class of its own.  Two properties make
the result the exact one:
  1. d2' >= d2, so with nndr >= 0 a column rejected against d2' is rejected against d2: no real accept is lost;
  2. min(d2', minimum over the other rows of the best row's class) == d2: the repair of an accepting column is exact.
(A negative nndr turns property 1 round; the kernel then repairs every column, which property 2 covers.)
Both are asserted on random frames, on frames with planted near neighbours and duplicated rows, and on frames made so that
the second best always sits in the best row's class."""
import numpy as np
import pytest

NONE = 0xFFFF


def class_of(row):
    """(tile, lane half, register 15 or not) of a "from" row: the kernel's register-to-row map inverted."""
    row = np.asarray(row)
    in_tile = row & 31
    return (row >> 5) * 4 + ((in_tile >> 2) & 1) * 2 + ((in_tile & 27) == 27)


def test_class_map_is_the_register_map():
    for h in (0, 1):
        rows = [(i & 3) + 8 * (i >> 2) + 4 * h for i in range(16)]
        assert sorted(rows + [r ^ 4 for r in rows]) == list(range(32))
        assert len(set(class_of(np.array(rows[:15])).tolist())) == 1
        assert class_of(rows[15]) != class_of(rows[0]) and rows[15] == 27 + 4 * h
        # the repair walks base + g + k, g = 0, 8, 16, 24, k = 0..3, base = (idx & ~31) + (idx & 4), without g + k == 27
        for idx in rows[:15]:
            base = (idx & ~31) + (idx & 4)
            walked = [base + g + k for g in (0, 8, 16, 24) for k in range(4) if g + k != 27]
            assert sorted(walked) == sorted(rows[:15])


def hamming(a, b):
    """[Kf, Kt] Hamming distances of uint8 descriptor rows."""
    x = a[:, None, :] ^ b[None, :, :]
    return np.unpackbits(x, axis=2).sum(axis=2).astype(np.int64)


def scan_model(D):
    """Per column of the distance table D [Kf, Kt]: best row (lower index on ties), d1, exact d2, the scan's optimistic d2'
    and the repaired value."""
    kf, kt = D.shape
    idx = np.argmin(D, axis=0)                       # numpy takes the first minimum: the BFMatcher tie rule
    cols = np.arange(kt)
    d1 = D[idx, cols]
    others = D.copy()
    others[idx, cols] = 1 << 20
    d2 = others.min(axis=0) if kf >= 2 else np.full(kt, NONE)
    cls = class_of(np.arange(kf))
    outside = cls[:, None] != cls[idx][None, :]      # [Kf, Kt]: rows outside the best row's class
    d2_opt = np.where(outside, D, 1 << 20).min(axis=0)
    d2_opt = np.where(d2_opt == 1 << 20, NONE, d2_opt)
    inside = ~outside
    inside[idx, cols] = False
    in_class = np.where(inside, D, 1 << 20).min(axis=0)
    return idx, d1, d2, d2_opt, np.minimum(d2_opt, in_class)


def accepts(kf, d1, d2, nndr):
    # the kernel's test, in float32 as there
    return (kf >= 2) & ~(d1.astype(np.float32) > np.float32(nndr) * d2.astype(np.float32))


def check(a, b, nndrs=(0.0, 0.3, 0.6, 0.8, 0.999, 1.0, 1.5)):
    D = hamming(a, b)
    kf = D.shape[0]
    idx, d1, d2, d2_opt, d2_rep = scan_model(D)
    assert np.all(d2_opt >= d2)
    if kf >= 2:
        assert np.array_equal(d2_rep, d2)
    for nndr in nndrs:
        exact, opt = accepts(kf, d1, d2, nndr), accepts(kf, d1, d2_opt, nndr)
        assert np.all(exact <= opt), nndr                        # property 1: a real accept is never rejected
        final = opt & accepts(kf, d1, d2_rep, nndr)              # repaired columns decide again
        assert np.array_equal(final, exact), nndr
    return int((d2_opt != d2).sum())


def rows(rng, k, cols=32):
    return rng.integers(0, 256, size=(k, cols), dtype=np.uint8)


def near(rng, row, n):
    out = row.copy()
    for bit in rng.choice(row.size * 8, size=n, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


@pytest.mark.parametrize("kf", [1, 2, 3, 15, 16, 17, 27, 28, 31, 32, 33, 60, 64, 100, 500])
def test_random_frames(kf):
    rng = np.random.default_rng(7000 + kf)
    check(rows(rng, kf), rows(rng, 96))


def test_true_pairs_with_noise():
    # every column has a near "from" row and a less near one, placed anywhere
    rng = np.random.default_rng(7100)
    b = rows(rng, 200)
    a = rows(rng, 500)
    for t in range(200):
        r1, r2 = rng.choice(500, size=2, replace=False)
        a[r1] = near(rng, b[t], int(rng.integers(0, 40)))
        a[r2] = near(rng, b[t], int(rng.integers(20, 70)))
    check(a, b)


@pytest.mark.parametrize("kf", [17, 64, 500])
def test_second_best_always_in_the_best_rows_class(kf):
    # adversarial: for every column the two nearest rows share a class; the optimistic value is wrong in every column
    rng = np.random.default_rng(7200 + kf)
    a = rows(rng, kf)
    cls = class_of(np.arange(kf))
    big = [c for c in np.unique(cls) if (cls == c).sum() >= 2]
    b = rows(rng, 2 * len(big))
    for n, c in enumerate(big):
        members = np.flatnonzero(cls == c)
        r1, r2 = rng.choice(members, size=2, replace=False)
        a[r1] = near(rng, b[2 * n], 30)
        a[r2] = near(rng, b[2 * n], 40)
    wrong = check(a, b[0::2])
    assert wrong == len(big)


def test_ties_and_duplicates():
    rng = np.random.default_rng(7300)
    a = rows(rng, 500)
    for r in range(492):
        if not r & 8:
            a[r + 8] = a[r]                          # twins in one lane half (rows 19 / 23 pair with the single rows 27 / 31)
    check(a, rows(rng, 128))
    same = np.repeat(rows(rng, 1), 77, axis=0)       # all rows identical
    check(same, rows(rng, 40))
    check(a, a[:97].copy())                          # d1 = 0 everywhere, d2 = 0 where the twin exists
