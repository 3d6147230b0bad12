"""Edges of the matrix-core matcher's code paths around its scan, against the CPU oracle byte for byte (result record and
pass-1 correspondence list), once through the split pipeline (k_match_split: four resident "to" tiles, pipelined scan)
and once through the fused kernel (two tiles, unpipelined scan; its WIDE form at K = 1000).

test_gpu_verify.py::test_pipelined_scan_at_its_tile_boundaries walks Kf and Kt over 1 ... 520 around the 32-row tiles.
This file adds what the code around the scan turns on and that test does not reach:
  * the ragged last "from" tile (its missing rows are masked in the accumulator's origin tuple) with 1, 20 and 31 rows,
    with no full tile in front of it and with fifteen;
  * Kt = 97 (a 3-tile column group run as 4 with an empty tile, whose columns repeat the frame's last row) and Kt = 33
    (one column in the tile that the upper lane half decides: a decode pass takes two tiles, one per lane half);
  * K = 1000 and 1013 (two column groups per wavefront: the origin tuple is rebuilt between them);
  * 512-bit descriptors (the unpipelined scan with one resident tile);
  * duplicated "from" rows (exact ties of the best and second-best distance: NNDR rejects them below 1.0 and takes the
    LOWER index at 1.0) and duplicated "to" rows (two columns claim one row: neither is kept);
  * a pair in which every column is rejected and one in which none is; empty frames on either side.
The test pins behaviour, it defines none: every case passes on the code before these paths were rewritten."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, synth

pytestmark = pytest.mark.gpu


def _cut(fa, n):
    return _abi.FeatureArrays(fa.desc[:n], fa.xyz[:n], fa.kpts[:n])


def _with_rows_copied(fa, pairs):
    """The frame with descriptor row dst replaced by row src for every (src, dst)."""
    d = fa.desc.copy()
    for src, dst in pairs:
        d[dst] = d[src]
    return _abi.FeatureArrays(d, fa.xyz, fa.kpts)


def _empty(cols):
    return _abi.FeatureArrays(np.zeros((0, cols), np.uint8), np.zeros((0, 3), np.float32), np.zeros(0, _abi.KEYPOINT_DTYPE))


def _params(nndr=None):
    p = synth.camera_params()
    p.iterations = 200
    p.min_inliers = 5
    if nndr is not None:
        p.nndr = nndr
    return p


def _check(monkeypatch, oracle, split, p, A, B, expect=None):
    """Every pair of (A "from", B "to") against the oracle; expect: {pair: number of pass-1 correspondences}."""
    from multi_robot_slam_separators_amd import lib
    if split:
        monkeypatch.setenv("SF_FUSED", "2")
    else:
        monkeypatch.delenv("SF_FUSED", raising=False)
    monkeypatch.setenv("SF_DEBUG_CORR", "1")
    with lib.SeparatorFinder(p) as f:
        f.prof_enable(True)
        got = f.estimate_transform_batch(A, B)
        if split:
            assert f.prof_get()["k_match_global"][0] >= 1          # (the split form's matching launch)
        for i in range(len(A)):
            o, c1, _ = oracle.estimate_transform(p, A[i], B[i], debug=True)
            g1 = f.debug_correspondences(i, 1)
            ctx = (i, len(A[i].desc), len(B[i].desc))
            assert np.array_equal(g1[0], c1[0]) and np.array_equal(g1[1], c1[1]), ctx
            assert got[i].tobytes() == o.tobytes(), ctx
            if expect and i in expect:
                assert len(c1[0]) == expect[i], ctx
    return got


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_ragged_from_tiles_and_short_column_groups(monkeypatch, oracle, split):
    from test_gpu_fuzz import random_frame
    rng = np.random.default_rng(4101)
    base_a, base_b, _, _ = synth.make_pairs(93, 1, k=520, cols=32, true_frac=1.0)
    a, b = base_a[0], base_b[0]
    A, B = [], []
    for kf in (1, 20, 31, 481, 500, 511):          # ragged tiles of 1, 20, 31 rows behind 0 and behind 15 full tiles
        for kt in (500, 97, 33, 20):
            A.append(_cut(a, kf)); B.append(_cut(b, kt))
        A.append(random_frame(rng, kf, 32)); B.append(random_frame(rng, 97, 32))
    for kf in (32, 64, 480, 512):                  # no ragged tile, the same short column groups
        for kt in (97, 33):
            A.append(_cut(a, kf)); B.append(_cut(b, kt))
    for kf, kt in ((0, 200), (200, 0), (0, 0), (0, 33), (31, 0)):
        A.append(_cut(a, kf) if kf else _empty(32)); B.append(_cut(b, kt) if kt else _empty(32))
    got = _check(monkeypatch, oracle, split, _params(), A, B)
    assert sum(int(g["success"]) for g in got) >= 3


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_two_column_groups_per_wavefront(monkeypatch, oracle, split):
    from test_gpu_fuzz import random_frame
    rng = np.random.default_rng(4102)
    base_a, base_b, _, _ = synth.make_pairs(94, 1, k=1013, cols=32, true_frac=1.0)
    a, b = base_a[0], base_b[0]
    A, B = [], []
    for kf, kt in ((1000, 1000), (1013, 1013), (1013, 1000), (1000, 1013), (20, 1013), (1013, 97), (481, 993), (1013, 33)):
        A.append(_cut(a, kf)); B.append(_cut(b, kt))
    A.append(random_frame(rng, 1013, 32)); B.append(random_frame(rng, 1000, 32))
    got = _check(monkeypatch, oracle, split, _params(), A, B)
    assert sum(int(g["success"]) for g in got) >= 3


@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_512_bit_descriptors(monkeypatch, oracle, split):
    from test_gpu_fuzz import random_frame
    rng = np.random.default_rng(4103)
    base_a, base_b, _, _ = synth.make_pairs(95, 1, k=300, cols=64, true_frac=1.0)
    a, b = base_a[0], base_b[0]
    A, B = [], []
    for kf, kt in ((300, 300), (1, 300), (20, 97), (31, 33), (257, 97), (288, 33), (300, 0), (0, 300)):
        A.append(_cut(a, kf) if kf else _empty(64)); B.append(_cut(b, kt) if kt else _empty(64))
    A.append(random_frame(rng, 275, 64)); B.append(random_frame(rng, 161, 64))
    got = _check(monkeypatch, oracle, split, _params(), A, B)
    assert sum(int(g["success"]) for g in got) >= 1


@pytest.mark.parametrize("nndr", [0.8, 1.0])
@pytest.mark.parametrize("split", [True, False], ids=["split", "fused"])
def test_ties_and_all_or_nothing(monkeypatch, oracle, split, nndr):
    from test_gpu_fuzz import random_frame
    rng = np.random.default_rng(4104)
    base_a, base_b, _, _ = synth.make_pairs(96, 1, k=500, cols=32, true_frac=1.0)
    a, b = base_a[0], base_b[0]
    A, B, expect = [], [], {}
    # some "from" rows twice, inside a tile, across a tile edge, in the ragged tile, far apart: the columns that match
    # them see d1 == d2 exactly
    dup_from = ((5, 6), (31, 32), (40, 300), (480, 499), (490, 3), (127, 128))
    A.append(_with_rows_copied(a, dup_from)); B.append(b)
    # some "to" rows twice (also across the lane halves' tiles and the wavefronts' groups): one "from" row, two claims
    dup_to = ((7, 8), (31, 32), (33, 64), (96, 127), (200, 499), (470, 471))
    A.append(a); B.append(_with_rows_copied(b, dup_to))
    A.append(_with_rows_copied(a, dup_from)); B.append(_with_rows_copied(b, dup_to))
    # every "from" row twice against unrelated columns: d1 == d2 > 0 everywhere, every column rejected below 1.0 and none
    # at 1.0 (the lower index of each twin is taken, by many columns at once)
    twins = _with_rows_copied(a, [(2 * i, 2 * i + 1) for i in range(250)])
    A.append(twins); B.append(random_frame(rng, 500, 32))
    if nndr < 1.0:
        expect[len(A) - 1] = 0
    # the "to" frame IS the "from" frame: d1 = 0 in every column, none rejected, every row claimed exactly once
    A.append(a); B.append(_abi.FeatureArrays(a.desc.copy(), b.xyz, b.kpts))
    expect[len(A) - 1] = 500
    # ... and with 481 rows on one side and 97 on the other
    A.append(_cut(a, 481)); B.append(_abi.FeatureArrays(a.desc[:97].copy(), b.xyz[:97], b.kpts[:97]))
    expect[len(A) - 1] = 97
    # all rows of a frame identical
    same = _with_rows_copied(a, [(0, i) for i in range(1, 500)])
    A.append(same); B.append(b)
    A.append(a); B.append(_with_rows_copied(b, [(0, i) for i in range(1, 500)]))
    _check(monkeypatch, oracle, split, _params(nndr), A, B, expect)
