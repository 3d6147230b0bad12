"""The matcher's second-best distance where the matrix-core scan does not keep it exactly, against the CPU oracle byte for
byte (result record and pass-1 correspondence list), through the split form (k_match_split: pipelined scan, four resident
"to" tiles) and the fused kernel (unpipelined scan, two tiles).

The scan keeps the best score exactly and, as second best, the best score among the rows OUTSIDE the best row's class
(k_match.hip, top2_update16: a class is the 15 rows 4 h + {0..3, 8..11, 16..19, 24..26} of one 32-row "from" tile, h = 0, 1,
or the single row 27 + 4 h); a column that passes NNDR against that has the other rows of the class looked at again
(mf_repair_d2).  The cases here plant, for chosen columns, a best row at distance d1, a second best at d2 and a third at
d3 with nothing else nearer than about 90 (random 256-bit rows), and put the second best where the repair has to find it:
in the best row's class (a full tile and the ragged one, both halves), or where the scan already has it (row 27 / 31, the
other half, another tile).  With (d1, d2, d3) = (30, 40, 60) at nndr 0.6 the exact test rejects (30 > 24) and a second
best taken from outside the class would accept (30 <= 36); with (20, 40, 60) both accept.  Unplanted columns are random
against random: all rejected at 0.6.  The recorded correspondence counts are the oracle's.
The file pins behaviour and defines none: every case passes on the exact top-2 scan this one replaced."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi

from test_gpu_match_edges import _check, _params

pytestmark = pytest.mark.gpu

REJ, ACC = (30, 40, 60), (20, 40, 60)


def _frame(rng, k, cols):
    from test_gpu_fuzz import random_frame
    return random_frame(rng, k, cols)


def _flipped(rng, row, n):
    """`row` (uint8 bytes) with n distinct bits inverted."""
    out = row.copy()
    for bit in rng.choice(row.size * 8, size=n, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def _planted(seed, kf, kt, plants, cols=32):
    """A random pair in which column t of the "to" frame has "from" row rows[i] at Hamming distance dist[i], for every
    (t, rows, dist) of `plants`."""
    rng = np.random.default_rng(seed)
    a, b = _frame(rng, kf, cols), _frame(rng, kt, cols)
    da, used = a.desc.copy(), set()
    for t, rows, dist in plants:
        for r, d in zip(rows, dist):
            assert r < kf and t < kt and r not in used
            used.add(r)
            da[r] = _flipped(rng, b.desc[t], d)
    return _abi.FeatureArrays(da, a.xyz, a.kpts), b


def _cases_nndr06():
    """[(name, from, to, expected pass-1 correspondences)]"""
    c = []
    # best and second best in one class, third elsewhere: full tile (half 0: rows 65, 73; half 1: rows 102, 116) and the
    # ragged tile of Kf = 500 (half 0: rows 480, 497; half 1: rows 485, 494); columns in both lane halves' tiles
    same = [(3, (65, 73, 200)), (40, (102, 116, 7)), (333, (480, 497, 100)), (499, (485, 494, 3))]
    for i, (t, rows) in enumerate(same):
        c.append(("same_class_reject_%d" % i, *_planted(5100 + i, 500, 500, [(t, rows, REJ)]), 0))
    c.append(("same_class_reject_all", *_planted(5110, 500, 500, [(t, rows, REJ) for t, rows in same]), 0))
    c.append(("same_class_accept", *_planted(5111, 500, 500, [(t, rows, ACC) for t, rows in same]), 4))
    # best in register 15's single-row class (rows 27 and 31 of a tile), second best in the same tile and half; and the
    # other way round
    slot15 = [(5, (91, 88, 300)), (70, (127, 125, 301)), (130, (152, 155, 302)), (260, (479, 476, 9))]
    c.append(("slot15_reject", *_planted(5120, 500, 500, [(t, rows, REJ) for t, rows in slot15]), 0))
    c.append(("slot15_accept", *_planted(5121, 500, 500, [(t, rows, ACC) for t, rows in slot15]), 4))
    # second best in the other half of the best row's tile, and in another tile
    other = [(9, (65, 69, 200)), (77, (102, 98, 7)), (140, (161, 300, 201)), (450, (485, 2, 100))]
    c.append(("other_half_or_tile_reject", *_planted(5130, 500, 500, [(t, rows, REJ) for t, rows in other]), 0))
    c.append(("other_half_or_tile_accept", *_planted(5131, 500, 500, [(t, rows, ACC) for t, rows in other]), 4))
    # few "from" rows, all in one tile (Kf = 1: no second best, nothing is accepted)
    for kf, b0, s0 in ((2, 0, 1), (3, 0, 2), (15, 0, 11), (16, 4, 15), (17, 16, 0)):
        c.append(("kf_%d_reject" % kf, *_planted(5140 + kf, kf, 40, [(0, (b0, s0), REJ[:2])]), 0))
        c.append(("kf_%d_accept" % kf, *_planted(5160 + kf, kf, 40, [(1, (s0, b0), ACC[:2])]), 1))
    c.append(("kf_1", *_planted(5141, 1, 40, [(0, (0,), (20,))]), 0))
    # Kf = 33: the best in row 32, alone in its tile; and the other way round
    c.append(("kf_33_reject", *_planted(5150, 33, 40, [(0, (32, 5), REJ[:2])]), 0))
    c.append(("kf_33_accept", *_planted(5151, 33, 40, [(1, (32, 5), ACC[:2])]), 1))
    c.append(("kf_33_reject_b", *_planted(5152, 33, 40, [(2, (5, 32), REJ[:2])]), 0))
    # K = 1000 (two column groups per wavefront): a full tile and the ragged tile (rows 992 ... 999)
    k1000 = [(3, (641, 649, 50), REJ), (700, (992, 995, 51), REJ), (999, (997, 999, 52), REJ), (515, (650, 642, 53), ACC)]
    c.append(("k1000", *_planted(5190, 1000, 1000, k1000), 1))
    return c


def _cases_512bit():
    # 512-bit descriptors (one resident tile, unpipelined scan in both forms); ragged tile = rows 288 ... 299
    p = [(3, (65, 73, 200), REJ), (40, (102, 116, 7), REJ), (130, (289, 297, 8), REJ), (299, (294, 293, 9), REJ),
         (200, (169, 161, 10), ACC)]
    return [("w16", *_planted(5170, 300, 300, p, cols=64), 1)]


def _twins(seed, kf):
    """Every "from" row r with (r & 8) == 0 copied to row r + 8 (the same lane half: the same class, but for rows 19 / 23
    whose twins 27 / 31 are classes of their own), against random columns: d1 == d2 in every column whose best row has
    its twin (all of them when Kf is a multiple of 16)."""
    rng = np.random.default_rng(seed)
    a, b = _frame(rng, kf, 32), _frame(rng, 500, 32)
    d = a.desc.copy()
    for r in range(kf - 8):
        if not r & 8:
            d[r + 8] = d[r]
    return _abi.FeatureArrays(d, a.xyz, a.kpts), b


def _get(builder, cache={}):
    if builder not in cache:
        cache[builder] = builder()
    return cache[builder]


def _run(monkeypatch, oracle, split, nndr, cases):
    A, B = [c[1] for c in cases], [c[2] for c in cases]
    expect = {i: c[3] for i, c in enumerate(cases) if c[3] is not None}
    _check(monkeypatch, oracle, split, _params(nndr), A, B, expect)


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_second_best_in_the_best_rows_class(monkeypatch, oracle, split):
    # the first case of the list alone, so that it fails on its own when the repair is missing
    _run(monkeypatch, oracle, split, 0.6, _get(_cases_nndr06)[:1])


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_planted_second_best_everywhere(monkeypatch, oracle, split):
    _run(monkeypatch, oracle, split, 0.6, _get(_cases_nndr06)[1:])


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_planted_second_best_512_bit(monkeypatch, oracle, split):
    _run(monkeypatch, oracle, split, 0.6, _get(_cases_512bit))


@pytest.mark.parametrize("nndr,expect", [(1.0, (73, 64)), (0.999, (0, 0))], ids=["1.0", "below"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_ties_inside_a_class(monkeypatch, oracle, split, nndr, expect):
    """nndr = 1.0: every column passes and repairs, the LOWER index of each twin is kept (the lists are compared with the
    oracle's; 73 and 64 "from" rows are claimed by exactly one column).  Just below 1.0 a tie is rejected: no
    correspondence (at Kf = 500 no column's best row is one of the untwinned rows 496 ... 499)."""
    cases = [("twins_512", *_twins(5180, 512), expect[0]), ("twins_500", *_twins(5181, 500), expect[1])]
    _run(monkeypatch, oracle, split, nndr, cases)
