"""uint8 descriptor rows compared by L2 (sf_params.desc_type 2: 128 dimensions, desc_bytes 128) through the store and the
verification path.  The global matching pass runs on the int8 matrix cores (k_match_u8.hip: shifted rows, d^2 = |f|^2 +
|t|^2 - 2 f.t in int32), the guided passes take the integer sum on the VALU (k_guided<32, L2, U8>).  Since a squared
distance of 128 differences of integers in -255 .. 255 is an integer below 2^24, every result must equal, byte for byte,
what the oracle computes for desc_type 1 on the float twin of the rows (rows.astype(float32), desc_bytes 512): the oracle
itself knows desc_type 0 and 1 only and is always asked that way here.  The scan alone is read through sf_debug_knn2_u8
against a NumPy integer kNN-2 with the sequential tie rule (strict comparisons in "from" order)."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth

pytestmark = pytest.mark.gpu

DIMS = 128
NONE = 2 ** 31 - 1


def _params(est=0, iterations=100):
    p = synth.camera_params()
    p.iterations = iterations
    p.estimation_type = est
    p.desc_type = 2
    p.desc_bytes = DIMS
    p.max_features = 256
    return p


def _float_params(p):
    """The parameters the oracle is asked with: the same, float32 rows."""
    q = _abi.copy_params(p)
    q.desc_type = 1
    q.desc_bytes = 4 * DIMS
    return q


def _float(fa):
    """The float twin of a keyframe of uint8 rows."""
    return _abi.FeatureArrays(fa.desc.astype(np.float32).reshape(-1, DIMS), fa.xyz, fa.kpts)


def _pairs(seed, n, k, jitter, true_frac=0.5):
    A, B, is_true, Ts = synth.make_pairs(seed, n, k=k, cols=32, true_frac=true_frac)
    rng = np.random.default_rng(seed + 1)
    return ([synth.u8_descriptors(a, DIMS, rng, jitter) for a in A],
            [synth.u8_descriptors(b, DIMS, rng, jitter) for b in B], is_true, Ts)


def _keyframe(rows):
    """A keyframe of the given uint8 rows; the scan looks at nothing else."""
    n = rows.shape[0]
    kp = np.zeros(n, _abi.KEYPOINT_DTYPE)
    return _abi.FeatureArrays(np.ascontiguousarray(rows, np.uint8).reshape(n, DIMS), np.zeros((n, 3), np.float32), kp)


def _knn2_ref(F, T):
    """Integer kNN-2 of every "to" row over the "from" rows as the sequential scan leaves it: strict comparisons in "from"
    order, so the best index is the lowest at the smallest distance and the second best is the second smallest of the
    distances as a multiset.  -> (d_best, d_second, i_best) per "to" row; NONE / -1 where there is no such row."""
    F, T = F.astype(np.int64), T.astype(np.int64)
    kt, kf = T.shape[0], F.shape[0]
    d1, d2, i1 = np.full(kt, NONE, np.int64), np.full(kt, NONE, np.int64), np.full(kt, -1, np.int64)
    if kf == 0 or kt == 0:
        return d1, d2, i1
    d = (T * T).sum(1)[:, None] + (F * F).sum(1)[None, :] - 2 * (T @ F.T)
    i1 = d.argmin(axis=1)                                  # (the first occurrence)
    d1 = d[np.arange(kt), i1]
    if kf >= 2:
        d2 = np.partition(d, 1, axis=1)[:, 1]
    return d1, d2, i1


def _rows_from(n):
    r, c = np.arange(n)[:, None], np.arange(DIMS)[None, :]
    return ((7 * r + 13 * c + (r * c) % 251 + (r * r) % 17) % 256).astype(np.uint8)


def _rows_to(n):
    r, c = np.arange(n)[:, None], np.arange(DIMS)[None, :]
    return ((11 * r + 5 * c * c + 3 * (r * c) % 239 + 101) % 256).astype(np.uint8)


def _check_scan(f, sf, st, F, T, what):
    got = f.debug_knn2_u8(sf, st, T.shape[0])
    want = _knn2_ref(F, T)
    for g, w, name in zip(got, want, ("d_best", "d_second", "i_best")):
        bad = np.nonzero(g.astype(np.int64) != w)[0]
        assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])


SIZES = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 200)


def test_operand_map_on_asymmetric_rows():
    """Row r, byte c of the "from" frames and of the "to" frames are two different functions of (r, c), neither symmetric in
    r and c nor in the byte's place inside its dword, both reaching 0 and 255: a swapped row / column of the tile, a wrong
    byte order inside a k-step or a k-step against the wrong half changes the distances.  Every Kf x Kt of the sizes
    around the 16-row tile and the 64-row sweep of a wavefront; then a keyframe of 600 rows, which grows the capacity
    past 512 (the slots are re-pitched) and makes the block loop over the "from" rows run more than once, against itself
    and against the short frames on either side.  Exact equality on all three outputs."""
    Fa, Ta = _rows_from(600), _rows_to(600)
    assert Fa.min() == 0 and Fa.max() == 255 and Ta.min() == 0 and Ta.max() == 255
    assert not np.array_equal(Fa[:DIMS, :], Fa[:DIMS, :].T) and not np.array_equal(Fa[:200], Ta[:200])
    with lib.SeparatorFinder(_params()) as f:
        sf = {n: f.store_add_keyframe(_keyframe(Fa[:n])) for n in SIZES}
        st = {n: f.store_add_keyframe(_keyframe(Ta[:n])) for n in SIZES}
        for kf in SIZES:
            for kt in SIZES:
                _check_scan(f, sf[kf], st[kt], Fa[:kf], Ta[:kt], (kf, kt))
        big_f, big_t = f.store_add_keyframe(_keyframe(Fa)), f.store_add_keyframe(_keyframe(Ta))
        _check_scan(f, big_f, big_t, Fa, Ta, (600, 600))
        _check_scan(f, big_f, st[200], Fa, Ta[:200], (600, 200))      # (the short frames after the re-pitch)
        _check_scan(f, sf[200], big_t, Fa[:200], Ta, (200, 600))
        _check_scan(f, sf[17], big_t, Fa[:17], Ta, (17, 600))


def test_ties_keep_the_lower_from_row(oracle):
    rng = np.random.default_rng(11)
    p = _params()
    with lib.SeparatorFinder(p) as f:
        # all rows identical: every distance 0, the best is row 0 and the second best is 0 too
        a, b, _, _ = _pairs(21, 1, 120, 0, true_frac=1.0)
        same = _abi.FeatureArrays(np.tile(a[0].desc[:1], (120, 1)), a[0].xyz, a[0].kpts)
        s = f.store_add_keyframe(same)
        d1, d2, i1 = f.debug_knn2_u8(s, s, 120)
        assert not d1.any() and not d2.any() and not i1.any()
        # ... so every "to" row names "from" row 0 (0 > 0.6 x 0 is false), none of them is its only match: no
        # correspondence, no transform -- the oracle's record on the float twin
        got = f.verify_pairs(np.array([s], np.int32), np.array([s], np.int32))[0]
        assert got.tobytes() == oracle.estimate_transform(_float_params(p), _float(same), _float(same)).tobytes()
        assert got["success"] == 0 and got["matches"] == 0
        # duplicated "from" rows astride a 16-row tile (15, 16) and astride two lane groups of a tile (3, 7)
        F = rng.integers(0, 256, size=(40, DIMS), dtype=np.uint8)
        F[16] = F[15]
        F[7] = F[3]
        T = rng.integers(0, 256, size=(20, DIMS), dtype=np.uint8)
        T[0] = F[15]
        T[1] = F[3]; T[1, 5] ^= 3                           # (near, not equal)
        T[2] = F[16]; T[2, 100] ^= 1
        sf, st = f.store_add_keyframe(_keyframe(F)), f.store_add_keyframe(_keyframe(T))
        d1, d2, i1 = f.debug_knn2_u8(sf, st, 20)
        assert (i1[0], d1[0], d2[0]) == (15, 0, 0)
        assert i1[1] == 3 and d1[1] == d2[1] > 0
        assert i1[2] == 15 and d1[2] == d2[2] == 1
        _check_scan(f, sf, st, F, T, "duplicates")


def test_extreme_distance():
    lo, hi = np.zeros((1, DIMS), np.uint8), np.full((1, DIMS), 255, np.uint8)
    with lib.SeparatorFinder(_params()) as f:
        s_lo, s_hi = f.store_add_keyframe(_keyframe(lo)), f.store_add_keyframe(_keyframe(hi))
        s_both = f.store_add_keyframe(_keyframe(np.concatenate([hi, lo, hi])))
        for a, b in ((s_lo, s_hi), (s_hi, s_lo)):
            d1, d2, i1 = f.debug_knn2_u8(a, b, 1)
            assert (d1[0], d2[0], i1[0]) == (128 * 255 * 255, NONE, 0) and d1[0] == 8323200
        d1, d2, i1 = f.debug_knn2_u8(s_both, s_lo, 1)
        assert (d1[0], d2[0], i1[0]) == (0, 8323200, 1)
        d1, d2, i1 = f.debug_knn2_u8(s_lo, s_both, 3)
        assert d1.tolist() == [8323200, 0, 8323200] and d2.tolist() == [NONE] * 3 and i1.tolist() == [0, 0, 0]


def _oracle_batch(oracle, p, A, B):
    q = _float_params(p)
    return [oracle.estimate_transform(q, _float(a), _float(b)) for a, b in zip(A, B)]


# seeds: 24 pairs of K = 200 at true_frac 0.5.  For each (est, jitter) below the ORACLE alone, run on the CPU on the
# float twin, accepts all but at most 2 of the true pairs and not every pair (the condition of test_gpu_l2.py):
#   (0, 0): seed 500, 9 true pairs, 9 accepted       (0, 12): seed 512, 16 true pairs, 16 accepted
#   (1, 0): seed 501, 11 true pairs, 11 accepted     (1, 12): seed 513, 12 true pairs, 12 accepted
# (the option runs below, seeds 640 / 641: 6 of 8 and 7 of 8 pairs true, all of them accepted and guided by the oracle)
@pytest.mark.parametrize("est", [0, 1])
@pytest.mark.parametrize("jitter", [0, 12])
def test_u8_rows_equal_the_oracle_on_the_float_twin(oracle, jitter, est):
    """Host keyframes (estimate_transform_batch), the same pairs on store slots (verify_pairs) and through one
    sf_step_issue / sf_step_retire, whose NetVLAD rows pair received keyframe i with local keyframe i."""
    import torch
    p = _params(est)
    n, dim = 24, 128
    p.netvlad_dimensions = dim
    p.netvlad_max_matches_nb = n
    A, B, is_true, Ts = _pairs(500 + jitter + est, n, 200, jitter)
    want = _oracle_batch(oracle, p, A, B)
    accepted = sum(int(o["success"]) for o in want)
    assert accepted >= np.sum(is_true) - 2 and accepted < n             # (the oracle alone: see the seeds above)
    rng = np.random.default_rng(9)
    nv_a = rng.normal(size=(n, dim)); nv_a /= np.linalg.norm(nv_a, axis=1, keepdims=True)
    nv_b = nv_a + 0.002 * rng.normal(size=(n, dim)); nv_b /= np.linalg.norm(nv_b, axis=1, keepdims=True)
    with lib.SeparatorFinder(p) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        got = f.estimate_transform_batch(A, B)
        for i in range(n):
            assert got[i].tobytes() == want[i].tobytes(), (i, {k: (got[i][k], want[i][k]) for k in ("success", "inliers", "matches", "inliers_pass1", "pass2_guided")})
            if is_true[i] and got[i]["success"]:
                assert synth.pose_error(got[i], Ts[i])[0] < (0.1 if est == 0 else 0.4)
        sa = [f.store_add_keyframe(a) for a in A]
        sb = [f.store_add_keyframe(b) for b in B]
        assert sa == list(range(sa[0], sa[0] + n)) and sb == list(range(sb[0], sb[0] + n))
        slots = f.verify_pairs(np.array(sa, np.int32), np.array(sb, np.int32))
        for i in range(n):
            assert slots[i].tobytes() == want[i].tobytes(), i
        f.nn_append_received(nv_a)
        f.nn_append_local(nv_b)
        f.step_issue(sa[0], sb[0])
        m, rom, recs, info = f.step_retire(copy=True)
        assert info["n_matches"] == n and sorted(m["idx_local"].tolist()) == list(range(n))
        assert np.array_equal(m["idx_local"], m["idx_other"])
        assert info["n_accepted"] == accepted
        for j in range(n):
            i = int(m["idx_local"][j])
            assert (rom[j] >= 0) == bool(want[i]["success"]), i
            if rom[j] >= 0:
                assert recs[rom[j]].tobytes() == want[i].tobytes(), i


def test_u8_edge_frames(oracle):
    """Empty / single-row / two-row frames, frames of different sizes around the 16-row tile, identical rows on both
    sides, and an empty first keyframe on a handle created with the width sf_default_params leaves."""
    p = _params()
    A, B, _, _ = _pairs(77, 2, 120, 4, true_frac=1.0)
    a, b = A[0], B[0]
    cut = lambda fa, n: _abi.FeatureArrays(fa.desc[:n] if n else np.zeros((0, DIMS), np.uint8), fa.xyz[:n], fa.kpts[:n])
    cases = [(cut(a, 0), b), (a, cut(b, 0)), (cut(a, 1), b), (cut(a, 2), cut(b, 2)), (cut(a, 120), cut(b, 50))]
    cases += [(cut(a, n), b) for n in (15, 16, 17, 33)]
    cases += [(a, cut(b, n)) for n in (15, 16, 17, 33)]
    same = _abi.FeatureArrays(np.tile(a.desc[:1], (120, 1)), a.xyz, a.kpts)
    cases.append((same, same))
    cases.append((A[1], B[1]))
    with lib.SeparatorFinder(p) as f:
        got = f.estimate_transform_batch([c[0] for c in cases], [c[1] for c in cases])
        want = _oracle_batch(oracle, p, [c[0] for c in cases], [c[1] for c in cases])
        for i in range(len(cases)):
            assert got[i].tobytes() == want[i].tobytes(), i
        assert got[-1]["success"] == 1
    q = _params()
    q.desc_bytes = 32                       # (what sf_default_params writes)
    empty = _abi.FeatureArrays(np.zeros((0, 0), np.uint8), a.xyz[:0], a.kpts[:0])
    with lib.SeparatorFinder(q) as f:
        s0 = f.store_add_keyframe(empty)
        s1 = f.store_add_keyframe(a)
        s2 = f.store_add_keyframe(b)
        got = f.verify_pairs(np.array([s1, s0], np.int32), np.array([s2, s2], np.int32))
        o = oracle.estimate_transform(_float_params(p), _float(a), _float(b))
        assert got[0].tobytes() == o.tobytes() and got[0]["success"] == 1
        assert got[1]["success"] == 0 and got[1]["matches"] == 0


@pytest.mark.parametrize("option", ["bundle_adjustment", "backward_estimate", "match_to_projection"])
@pytest.mark.parametrize("est", [0, 1])
def test_u8_rows_under_the_options_of_the_float_route(oracle, est, option):
    p = _params(est)
    if option == "bundle_adjustment":
        p.bundle_adjustment = 1
        p.stereo_baseline = 0.12
    elif option == "backward_estimate":
        p.forward_est_only = 0
    else:
        p.guess_match_to_projection = 1
    A, B, is_true, _ = _pairs(640 + est, 8, 200, 6, true_frac=0.75)
    want = _oracle_batch(oracle, p, A, B)
    if option == "match_to_projection":
        # sfo_estimate_transform has no Vis/CorGuessMatchToProjection (oracle/sf_oracle.c never reads the field): for a
        # guided pair the record is the one tests/test_gpu_guided_tp.py holds that option to -- pass 1 by the oracle, the
        # pass-2 list by the restatement tests/guided_tp_ref.py, both motion estimates by the oracle's estimators -- on the
        # float twin, byte for byte all the same.  (A pair that is not guided never reaches the option.)
        from tests.test_gpu_guided_tp import _restated
        q = _float_params(p)
        for i in range(len(A)):
            guided, _, _, rec = _restated(oracle, q, _float(A[i]), _float(B[i]))
            if guided:
                want[i] = rec
        assert sum(int(w["pass2_guided"]) for w in want) >= 4
    with lib.SeparatorFinder(p) as f:
        got = f.estimate_transform_batch(A, B)
    for i in range(len(A)):
        assert got[i].tobytes() == want[i].tobytes(), (i, {k: (got[i][k], want[i][k]) for k in ("success", "inliers", "matches", "inliers_pass1", "pass2_guided")})
    assert sum(int(g["success"]) for g in got) >= 4


def test_refusals_leave_the_handle_as_it_was():
    for width in (64, 256):
        p = _params()
        p.desc_bytes = width
        with pytest.raises(lib.SepfinderError) as e:
            lib.SeparatorFinder(p)
        assert e.value.code == _abi.SF_EINVAL
    A, B, _, _ = _pairs(5, 1, 60, 3, true_frac=1.0)
    with lib.SeparatorFinder(_params()) as f:
        s0 = f.store_add_keyframe(A[0])
        narrow = _abi.FeatureArrays(A[0].desc[:, :64].copy(), A[0].xyz, A[0].kpts)
        with pytest.raises(lib.SepfinderError) as e:
            f.store_add_keyframe(narrow)
        assert e.value.code == _abi.SF_ERANGE and f.store_size() == 1
        before = f.get_feature_type()[0]
        with pytest.raises(lib.SepfinderError) as e:
            f.set_feature_type(6)
        assert e.value.code == _abi.SF_EINVAL and "GFTT/BRIEF writes binary descriptors: a handle with desc_type 2 cannot store them" in str(e.value)
        assert f.get_feature_type()[0] == before and f.store_size() == 1
        with pytest.raises(lib.SepfinderError) as e:
            f.set_feature_type_surf()
        assert e.value.code == _abi.SF_EINVAL and f.get_feature_type()[0] == before
        # the handle still works
        s1 = f.store_add_keyframe(B[0])
        d1, d2, i1 = f.debug_knn2_u8(s0, s1, 60)
        w1, w2, wi = _knn2_ref(A[0].desc, B[0].desc)
        assert np.array_equal(d1, w1) and np.array_equal(d2, w2) and np.array_equal(i1, wi)
    with lib.SeparatorFinder(synth.camera_params()) as f:                  # the scan's debug call on another handle kind
        with pytest.raises(lib.SepfinderError) as e:
            f.debug_knn2_u8(0, 0, 1)
        assert e.value.code == _abi.SF_EINVAL
