"""The argument for the matcher's certified repair (k_match.hip: mf_repair_accept) and for the unshifted second-best score,
in numpy with the kernel's float32 arithmetic.

A column that passes NNDR against the scan's optimistic second best d2' is decided on its best row's class
(docs/match_second_best.md).  The decision needs no exact d2 (docs/match_repair_once.md):
  * for nndr >= 0 the test acc = !((float)d1 > nndr * (float)d2) is monotone non-decreasing in d2;
  * the Hamming distance p over a row's first four dwords is <= the row's distance d;
so with pmin = the minimum of p over the class's other rows, a column that passes against min(d2', pmin) passes against the
exact d2 = min(d2', dmin): it is CERTIFIED.  One that does not is not rejected, it is decided exactly.  The rule "certificate,
else exact" is asserted against the exact top-2 decision: exhaustively on the integers, and on random, planted and
adversarial frames through the kernel's class map and its one-instruction form of the exclusions (a mask of rows left out,
rotated, whose bits start the popcount chains at 512 or more).

The last part is the four lane permutations that hand pass 1's columns to lanes without a pass-0 repair, on 64 lanes.

In between: the decode of the second-best SCORE if it no longer moved with the scan's origin (a further cut that
docs/match_repair_once.md measured and did not take; the property is pinned here for a change that does): every value that
reaches the final merge is (an even integer) + (a fraction in (-32/2048, 63 * 32/2048]), and 2 * ceil((ns - 1) / 2) is the
integer that 2 * ceil((ns_shifted - org) / 2) was."""
import numpy as np
import pytest

from test_match_lazy_second_model import NONE, accepts, class_of, hamming, near, rows, scan_model

NNDRS = (0.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)


def test_certificate_never_accepts_what_the_exact_test_rejects_exhaustive():
    """d1 in 0..256 and every pair m <= d2 in 0..256 (and d2 absent, 0xFFFF): accept against m implies accept against d2.
    m stands for min(d2', pmin), d2 for min(d2', dmin): p <= d row by row gives m <= d2."""
    vals = np.concatenate([np.arange(257), [NONE]]).astype(np.int64)
    m, d2 = np.meshgrid(vals, vals, indexing="ij")
    keep = m <= d2
    m, d2 = m[keep], d2[keep]
    for nndr in NNDRS:
        for d1 in range(257):
            d1v = np.full(m.shape, d1, np.int64)
            cert, exact = accepts(2, d1v, m, nndr), accepts(2, d1v, d2, nndr)
            assert np.all(cert <= exact), (nndr, d1)


def test_the_predicate_is_not_monotone_below_zero():
    # why a negative nndr keeps the exact path: d1 = 0 passes against d2 = 0 and fails against d2 = 1
    d1 = np.zeros(2, np.int64)
    a = accepts(2, d1, np.array([0, 1]), -0.5)
    assert a[0] and not a[1]


def _excluded_by_the_kernels_mask(idx, kf):
    """The rows base + j, j = 0..27 over the four trips g = 0, 8, 16, 24, k = 0..3, that mf_repair_accept leaves out, from
    its own bit arithmetic: ok = rows < Kf, not the best row, not bit 27; no = ~ok rotated left by 9, right by 8 per trip;
    row g + k is left out when bit 9 + k is set."""
    base = (idx & ~31) + (idx & 4)
    ok = ((1 << min(kf - base, 31)) - 1) & ~(1 << (idx - base)) & ~(1 << 27) & 0xFFFFFFFF
    rot = lambda x, r: ((x >> r) | (x << (32 - r))) & 0xFFFFFFFF
    no = rot(~ok & 0xFFFFFFFF, 23)
    out = {}
    for g in (0, 8, 16, 24):
        for k in range(4):
            seed = no & (512 << k)
            assert seed == 0 or seed >= 512
            out[base + g + k] = seed != 0
        no = rot(no, 8)
    return out


@pytest.mark.parametrize("kf", [1, 2, 3, 27, 28, 32, 33, 60, 64, 500, 2048])
def test_the_mask_form_of_the_exclusions(kf):
    cls = class_of(np.arange(kf))
    for idx in range(max(0, kf - 70), kf):
        if (idx & 27) == 27:
            continue                                  # register 15's class: the kernel does not walk it
        ex = _excluded_by_the_kernels_mask(idx, kf)
        walked = sorted(r for r, e in ex.items() if not e)
        want = sorted(int(r) for r in np.flatnonzero(cls == cls[idx]) if r != idx)
        assert walked == want, (kf, idx)


def repair_rule(a, b, nndr):
    """(final decision, exact decision, columns that repair, columns left uncertified) per column of the pair."""
    D, P = hamming(a, b), hamming(a[:, :16], b[:, :16])
    kf, kt = D.shape
    assert np.all(P <= D)
    idx, d1, d2, d2_opt, d2_rep = scan_model(D)
    exact = accepts(kf, d1, d2, nndr)
    opt = accepts(kf, d1, d2_opt, nndr)
    if kf < 2:
        return opt, exact, 0, 0
    if not nndr >= 0:                                 # the exact path as a whole: every column repairs
        return accepts(kf, d1, d2_rep, nndr), exact, kt, kt
    cls = class_of(np.arange(kf))
    inside = cls[:, None] == cls[idx][None, :]
    inside[idx, np.arange(kt)] = False
    pmin = np.where(inside, P, 1 << 20).min(axis=0)
    # a best row in register 15's class is not walked: the minimum is d2'.  Elsewhere a row left out counts 512 or more in
    # the kernel: with every row left out the minimum is d2', or 512 where d2' is absent
    single = (idx & 27) == 27
    m = np.where(single, d2_opt, np.minimum(d2_opt, np.where(pmin == 1 << 20, 512, pmin)))
    cert = opt & accepts(kf, d1, m, nndr)
    need = opt & ~cert
    final = cert | (need & accepts(kf, d1, d2_rep, nndr))
    return final, exact, int(opt.sum()), int(need.sum())


def check(a, b, nndrs=NNDRS + (-0.5, 0.3, 0.999, 1.5)):
    tot = 0
    for nndr in nndrs:
        final, exact, _, need = repair_rule(a, b, nndr)
        assert np.array_equal(final, exact), nndr
        tot += need if nndr >= 0 else 0
    return tot


@pytest.mark.parametrize("kf", [1, 2, 3, 15, 16, 17, 27, 28, 31, 32, 33, 60, 64, 100, 500])
def test_random_frames(kf):
    rng = np.random.default_rng(8000 + kf)
    check(rows(rng, kf), rows(rng, 96))


def test_true_pairs_are_certified():
    """The benchmark's kind of pair: d1 about 13 of 256 bits, everything else unrelated (p = 64 +- 5.7): every repairing
    column is certified on the half rows."""
    rng = np.random.default_rng(8100)
    b = rows(rng, 200)
    a = rows(rng, 500)
    for t, r in enumerate(rng.choice(500, size=200, replace=False)):
        a[r] = near(rng, b[t], int(rng.integers(5, 22)))
    final, exact, repairing, need = repair_rule(a, b, 0.8)
    assert np.array_equal(final, exact) and repairing >= 190 and need == 0
    check(a, b)


def _class_mates(kf):
    cls = class_of(np.arange(kf))
    return [np.flatnonzero(cls == c) for c in np.unique(cls) if (cls == c).sum() >= 2]


def _near_in(rng, row, lo, hi, n):
    """`row` with n distinct bits of its bytes lo..hi-1 inverted."""
    out = row.copy()
    for bit in rng.choice(np.arange(lo * 8, hi * 8), size=n, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


@pytest.mark.parametrize("kf", [17, 64, 500])
@pytest.mark.parametrize("kind", ["equal_first_half_far_rest", "far_first_half_equal_rest", "close_everywhere"])
def test_adversarial_class_rows(kf, kind):
    """For every class with two rows or more: the best at distance 20, and a class mate that is
      * equal to the column in its first 128 bits and 100 away in the rest (p = 0: never certified, the exact test accepts
        at 0.6: 20 <= 0.6 * 100 -- the certificate's failure must not reject),
      * 60 away in the first 128 bits and equal in the rest (p = d = 60: certified at 0.6, as 20 <= 36),
      * 24 away in all (p about 12; exact: 20 > 0.6 * 24 rejects)."""
    rng = np.random.default_rng(8200 + kf)
    a = rows(rng, kf)
    groups = _class_mates(kf)
    b = rows(rng, len(groups))
    for n, members in enumerate(groups):
        r1, r2 = rng.choice(members, size=2, replace=False)
        a[r1] = near(rng, b[n], 20)
        if kind == "equal_first_half_far_rest":
            a[r2] = _near_in(rng, b[n], 16, 32, 100)
        elif kind == "far_first_half_equal_rest":
            a[r2] = _near_in(rng, b[n], 0, 16, 60)
        else:
            a[r2] = near(rng, b[n], 24)
    final, exact, repairing, need = repair_rule(a, b, 0.6)
    assert np.array_equal(final, exact) and repairing == len(groups)
    if kind == "equal_first_half_far_rest":
        assert need == len(groups) and exact.all()
    elif kind == "far_first_half_equal_rest":
        assert need == 0 and exact.all()
    else:
        assert need == len(groups) and not exact.any()
    check(a, b)


def test_ties_and_duplicates():
    rng = np.random.default_rng(8300)
    a = rows(rng, 500)
    for r in range(492):
        if not r & 8:
            a[r + 8] = a[r]
    check(a, rows(rng, 128))
    check(np.repeat(rows(rng, 1), 77, axis=0), rows(rng, 40))
    check(a, a[:97].copy())


# ---- the second-best score left unshifted -------------------------------------------------------------------------------

FR = np.float32(1.0 / 2048.0)


def _ceil2(x):
    return np.float32(2.0) * np.ceil(x * np.float32(0.5))


def test_unshifted_second_best_decodes_to_the_same_integer_exhaustive():
    """Every even score in range (|dot| <= 1100 covers 256- and 512-bit rows) and every fraction of the window
    (-32/2048, 63 * 32/2048] in steps of 1/2048: the new decode 2 * ceil((ns - 1) / 2) gives the score, and so does the
    old decode of the value shifted to the last tile's origin, for every row 0..2047 and every last tile behind it."""
    dots = np.arange(-1100, 1101, 2, dtype=np.float32)[:, None]
    k = np.arange(-31, 63 * 32 + 1, dtype=np.float32)[None, :]
    assert (k.max() - k.min()) * FR < 2                    # narrower than the step between two scores: maxima order by distance
    ns = dots + k * FR                                     # exact in float32: 11 bits of integer, 11 of fraction
    assert np.array_equal(ns.astype(np.float64), dots.astype(np.float64) + k.astype(np.float64) / 2048.0)
    assert np.array_equal(_ceil2(ns - np.float32(1.0)), np.broadcast_to(dots, ns.shape))
    # two values a distance step apart keep their order whatever their fractions
    assert np.all(ns[1:].min(axis=1) > ns[:-1].max(axis=1))
    row = np.arange(2048, dtype=np.float32)[None, :]
    for last in (None, 63):                                # the row's own tile as the last one, and tile 63
        t_last = np.floor(row / 32) if last is None else np.float32(last)
        org = np.float32(32) * t_last * FR
        shifted = dots - (row - np.float32(32) * t_last) * FR      # what the shifted s held at the end of the scan
        assert np.array_equal(_ceil2(shifted - org), np.broadcast_to(dots, shifted.shape))
        # the same value unshifted lies in the window of the tile it was taken in, up to the last one
        frac = (np.float32(32) * t_last - row) * FR
        assert frac.min() > -32 * FR and frac.max() <= 63 * 32 * FR


def test_absent_second_best_stays_absent():
    ninf = np.float32(-np.inf)
    assert ninf - np.float32(1.0) == ninf


# ---- the hand-over of pass 1's columns to lanes without a pass-0 repair ------------------------------------------------------

def _hand_over(redo0, redo1):
    """The four lane permutations of the `group` lambda (k_match.hip) on 64 lanes; returns (tgt, mine, recv): the lane a
    lane's column travels to, whether a lane holds a received column, and whose."""
    n0, n1 = sum(redo0), sum(redo1)
    dest, q, rank_free = [0] * 64, [0] * 64, [0] * 64
    for lane in range(64):
        jf = sum(1 for i in range(lane) if not redo0[i])            # mbcnt of the inverted pass-0 ballot
        r1 = sum(1 for i in range(lane) if redo1[i])                # mbcnt of the pass-1 ballot
        rank_free[lane] = jf
        dest[lane] = 64 - n0 + lane - jf if redo0[lane] else jf
        q[lane] = r1 if redo1[lane] else n1 + lane - r1
    assert sorted(dest) == list(range(64)) and sorted(q) == list(range(64))      # every exchange is a bijection
    slot = [None] * 64
    for lane in range(64):
        slot[dest[lane]] = lane                                     # ds_permute: a lane pushes to lane dest
    tgt = [slot[q[lane]] for lane in range(64)]                     # ds_bpermute: a lane pulls from lane q
    assert sorted(tgt) == list(range(64))
    recv = [None] * 64
    for lane in range(64):
        recv[tgt[lane]] = lane
    mine = [not redo0[lane] and rank_free[lane] < n1 for lane in range(64)]
    return tgt, mine, recv


def test_hand_over_is_a_bijection_onto_free_lanes():
    rng = np.random.default_rng(8400)
    shapes = [(1, 63), (63, 1), (32, 32), (1, 1), (40, 24)] + [None] * 2000
    for shape in shapes:
        n0 = int(rng.integers(1, 64)) if shape is None else shape[0]
        n1 = int(rng.integers(1, 65 - n0)) if shape is None else shape[1]
        redo0, redo1 = [False] * 64, [False] * 64
        for i in rng.choice(64, size=n0, replace=False):
            redo0[i] = True
        for i in rng.choice(64, size=n1, replace=False):
            redo1[i] = True
        tgt, mine, recv = _hand_over(redo0, redo1)
        assert sum(mine) == n1
        for lane in range(64):
            if redo1[lane]:                # its column lands in a lane with no pass-0 repair that knows it holds one
                assert mine[tgt[lane]] and not redo0[tgt[lane]] and recv[tgt[lane]] == lane
            if mine[lane]:                 # ... and such a lane holds a pass-1 column, never a stray one
                assert redo1[recv[lane]]
