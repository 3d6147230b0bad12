"""A camera model per keyframe (sf_camera_add / sf_camera_select / sf_store_set_camera): verification across the
keyframes of unlike cameras against the one-camera CPU oracle, wherever one camera decides the result, and against a
composition of the oracle's parts where the reference reads two.

The handle's camera is C0 (tests/camera_cases.py); C1 and C2 are added (and their mono twins).  Slots [0, n) hold the "from" keyframes, slots
[n, 2 n) the "to" keyframes; pair i = (i, n + i)."""
import ctypes as C
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from oracle import pyoracle
from tests import camera_cases as cc
import test_gpu_guided_tp as tp          # (its restatement of one pair under Vis/CorGuessMatchToProjection = true)

PER_COMBINATION = 2       # pairs per (X, Y): 18 pairs per call
# ids 3 and 4: C1 and C2 as mono cameras (no baseline: the adjustment reads no depth of their views)
C1_MONO = cc.Camera(cc.C1.fx, cc.C1.fy, cc.C1.cx, cc.C1.cy, cc.C1.width, cc.C1.height, cc.C1.L, 0.0)
C2_MONO = cc.Camera(cc.C2.fx, cc.C2.fy, cc.C2.cx, cc.C2.cy, cc.C2.width, cc.C2.height, cc.C2.L, 0.0)
ALL_CAMERAS = cc.CAMERAS + (C1_MONO, C2_MONO)


@functools.lru_cache(maxsize=None)
def nine_combinations(seed=4100, noise=0.02):
    """Pairs of all nine (X, Y) combinations: (cams_from, cams_to, A, B, T_gt)."""
    rng = np.random.default_rng(seed)
    xs, ys, A, B, Ts = [], [], [], [], []
    for x in range(3):
        for y in range(3):
            for _ in range(PER_COMBINATION):
                a, b, T = cc.make_pair(rng, cc.CAMERAS[x], cc.CAMERAS[y], noise=noise)
                xs.append(x); ys.append(y); A.append(a); B.append(b); Ts.append(T)
    return tuple(xs), tuple(ys), tuple(A), tuple(B), tuple(Ts)


@functools.lru_cache(maxsize=None)
def equal_cameras(seed=4200):
    """X = Y in {C1, C2} mixed with X = Y = C0 pairs."""
    rng = np.random.default_rng(seed)
    xs, A, B, Ts = [], [], [], []
    for x in (1, 0, 2, 0, 1, 2):
        a, b, T = cc.make_pair(rng, cc.CAMERAS[x], cc.CAMERAS[x])
        xs.append(x); A.append(a); B.append(b); Ts.append(T)
    return tuple(xs), tuple(xs), tuple(A), tuple(B), tuple(Ts)


@functools.lru_cache(maxsize=None)
def oracle_results(case, cam_of, estimation_type, gmtp, **kw):
    """The one-camera reference's result of every pair of `case` with camera cam_of ('to': the pair's Y; an int: that
    camera) in p: pyoracle.estimate_transform -- and with guess_match_to_projection = 1, which the C oracle does not
    carry (it runs the other sub-branch whatever the flag says), the reference tests/test_gpu_guided_tp.py holds the
    library to: pass 1 by the oracle, the pass-2 list by tests/guided_tp_ref.py, the oracle's estimator on that list,
    assembled into an sf_result (None where that pair's second pass would not be guided)."""
    xs, ys, A, B, _ = case()
    base = cc.base_params(estimation_type, guess_match_to_projection=gmtp, **kw)
    out = []
    for i in range(len(A)):
        cam = ALL_CAMERAS[ys[i]] if cam_of == "to" else ALL_CAMERAS[cam_of]
        if gmtp:
            assert not kw
            out.append(tp._restated(pyoracle, cam.params(base), A[i], B[i])[3])
        else:
            out.append(pyoracle.estimate_transform(cam.params(base), A[i], B[i]))
    return out


def open_store(p, case, tag=True):
    """A handle with the cameras behind C0 added and the case's keyframes in its store, each slot stamped with its camera."""
    xs, ys, A, B, _ = case()
    f = lib.SeparatorFinder(p, device=0)
    ids = [0] + [f.camera_add(cam.model()) for cam in ALL_CAMERAS[1:]]
    assert ids == list(range(len(ALL_CAMERAS)))
    for cams, feats in ((xs, A), (ys, B)):
        for x, fa in zip(cams, feats):
            if tag:
                f.camera_select(ids[x])
            f.store_add_keyframe(fa)
    return f


def assert_precondition(case, estimation_type, gmtp):
    """The inputs can tell the cameras apart (asserted on the oracle's side): under the To keyframe's own camera every pair
    succeeds with a guided second pass, and for Y != C0 the result under C0 differs in bytes."""
    xs, ys, A, _, _ = case()
    right = oracle_results(case, "to", estimation_type, gmtp)
    wrong = oracle_results(case, 0, estimation_type, gmtp)
    for i in range(len(A)):
        assert right[i] is not None, (i, xs[i], ys[i])
        assert right[i]["success"] == 1 and right[i]["pass2_guided"] == 1, (i, xs[i], ys[i])
        if ys[i] != 0:
            assert wrong[i] is None or right[i].tobytes() != wrong[i].tobytes(), (i, xs[i], ys[i])


MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]       # (estimation_type, guess_match_to_projection)


@pytest.mark.gpu
@pytest.mark.parametrize("estimation_type,gmtp", MODES)
def test_verify_pairs_reads_the_to_keyframes_camera(estimation_type, gmtp):
    """Tier 1, sf_verify_pairs and sf_verify_pairs_device: forward only, no adjustment -- the To camera decides, and every
    sf_result equals the oracle's with camera Y in p, byte for byte."""
    import torch
    assert_precondition(nine_combinations, estimation_type, gmtp)
    want = oracle_results(nine_combinations, "to", estimation_type, gmtp)
    n = len(want)
    p = cc.base_params(estimation_type, guess_match_to_projection=gmtp)
    with open_store(p, nine_combinations) as f:
        fr, to = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
        got = f.verify_pairs(fr, to)
        for i in range(n):
            assert got[i].tobytes() == want[i].tobytes(), ("verify_pairs", i, got[i], want[i])
        dev = torch.device("cuda:0")
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        d_from, d_to = torch.from_numpy(fr).to(dev), torch.from_numpy(to).to(dev)
        d_out = torch.zeros(n * _abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        f.verify_pairs_device(d_from.data_ptr(), d_to.data_ptr(), n, d_out.data_ptr())
        torch.cuda.synchronize()
        got_d = d_out.cpu().numpy().view(_abi.RESULT_DTYPE)
        for i in range(n):
            assert got_d[i].tobytes() == want[i].tobytes(), ("verify_pairs_device", i)


@pytest.mark.gpu
@pytest.mark.parametrize("estimation_type,gmtp", MODES)
def test_step_reads_the_to_keyframes_camera(estimation_type, gmtp):
    """Tier 1 through one sf_step_issue / sf_step_retire: the records of the accepted matches are the oracle's."""
    assert_precondition(nine_combinations, estimation_type, gmtp)
    want = oracle_results(nine_combinations, "to", estimation_type, gmtp)
    n = len(want)
    rng = np.random.default_rng(77)
    nv_a = rng.normal(size=(n, 128)); nv_a /= np.linalg.norm(nv_a, axis=1, keepdims=True)
    nv_b = nv_a + 0.002 * rng.normal(size=(n, 128)); nv_b /= np.linalg.norm(nv_b, axis=1, keepdims=True)
    p = cc.base_params(estimation_type, guess_match_to_projection=gmtp)
    p.netvlad_dimensions = 128
    p.netvlad_max_matches_nb = n
    with open_store(p, nine_combinations) as f:
        f.nn_append_received(nv_a)         # "other" = the from keyframes, slots [0, n)
        f.nn_append_local(nv_b)            # "local" = the to keyframes, slots [n, 2 n)
        f.step_issue(0, n)
        matches, rom, recs, info = f.step_retire(copy=True)
        assert info["n_matches"] == n
        seen = set()
        for i in range(n):
            il, io = int(matches["idx_local"][i]), int(matches["idx_other"][i])
            assert il == io
            seen.add(il)
            assert rom[i] >= 0, ("step", il)
            assert recs[rom[i]].tobytes() == want[il].tobytes(), ("step record", il)
        assert seen == set(range(n))


@pytest.mark.gpu
@pytest.mark.parametrize("estimation_type,option", [(1, "forward_est_only"), (0, "bundle_adjustment"), (1, "bundle_adjustment")])
def test_both_directions_and_adjustment_with_equal_cameras(estimation_type, option):
    """Tier 2: X = Y in {C1, C2} beside X = Y = C0 pairs in one call, where the From camera is read too but equals the To
    camera -- PnP with forward_est_only = 0, and the bundle adjustment with both estimators (a baseline per camera).  The
    results are the oracle's with that camera in p."""
    kw = {option: 0 if option == "forward_est_only" else 1}
    xs = equal_cameras()[0]
    n = len(xs)
    want = oracle_results(equal_cameras, "to", estimation_type, 0, **kw)
    assert sum(int(w["success"]) for w in want) == n
    p = cc.base_params(estimation_type, **kw)
    with open_store(p, equal_cameras) as f:
        got = f.verify_pairs(np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32))
    for i in range(n):
        assert got[i].tobytes() == want[i].tobytes(), (i, xs[i], got[i], want[i])


# Tier 3 (a)'s pairs, as (X, Y) indices into ALL_CAMERAS.  BOUND: the planted pose is the minimum of the reference's own
# cost, so the 1e-3 bound against it applies -- view 1 reads no depth (X mono: C0, or C1 / C2 without their baseline, ids
# 3 / 4), or the depth :1253 takes with the TO model's local transform is the right one because both cameras share the
# mounting (C1 -> C0).  QUIRK: X stereo and mounted unlike Y; the reference's invLocalTransformFrom =
# stereoCameraModelTo.localTransform().inverse() (:1253, restated as it stands) then takes view 1's observed depths in the
# wrong frame, its stereo rows disagree with its pixel rows and the minimum of the reference's cost is not the planted pose
# (millimetres off with C1's 0.11 m baseline, centimetres with C2's 0.54 m).  Every X != Y pair, BOUND and QUIRK, is held
# within 1e-3 m / 1e-3 rad of THAT minimum, found by SciPy (camera_cases.two_view_reference), and to its word count; the
# QUIRK pairs also to the minimum lying off the planted pose, where the cost with view 1's depths in the From model's own
# frame has its minimum: a silent correction of :1253 fails them.  EQUAL: X = Y, the oracle's bytes.
# (Every BOUND pair has a stereo view with a right depth: two mono views leave the scale free -- tests/test_oracle_ba.py --
#  and the oracle's own adjustment of a (C0, C0) pair drifts centimetres along it; that pair is held to the oracle's bytes.)
BOUND = ((0, 1), (0, 2), (1, 0), (3, 2), (4, 1))
QUIRK = ((1, 2), (2, 0), (2, 1))
EQUAL = ((0, 0), (1, 1), (2, 2))


@functools.lru_cache(maxsize=None)
def noise_free(seed=4300):
    """Noise-free planted pairs (no noise in 3D, none in pixels), one per combination of BOUND + QUIRK + EQUAL."""
    rng = np.random.default_rng(seed)
    xs, ys, A, B, Ts = [], [], [], [], []
    for x, y in BOUND + QUIRK + EQUAL:
        a, b, T = cc.make_pair(rng, ALL_CAMERAS[x], ALL_CAMERAS[y], noise=0.0)
        xs.append(x); ys.append(y); A.append(a); B.append(b); Ts.append(T)
    return tuple(xs), tuple(ys), tuple(A), tuple(B), tuple(Ts)


def pose_error(res, T_gt):
    """(metres, radians) between an sf_result's pose and the planted one."""
    x, y, z, w = (float(v) for v in res["orientation"])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    dt = float(np.linalg.norm(np.asarray(res["position"], dtype=np.float64) - T_gt[:3, 3]))
    dR = R.T @ T_gt[:3, :3]
    return dt, float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("estimation_type", [0, 1])
def test_adjustment_projects_each_view_with_its_own_model(estimation_type):
    """Tier 3 (a): the bundle adjustment on X != Y, where the oracle (one camera) cannot follow.  On noise-free planted
    pairs the result succeeds and lies within 1e-3 m and 1e-3 rad -- the bound tests/test_oracle_ba.py holds the oracle's
    adjustment to -- of the minimum of the reference's two-view cost with one model per view and :1253 as written, found
    by SciPy on the planted words of the library's own pass-2 list; it keeps as many words as that minimum leaves inside
    the robust kernel.  On the BOUND pairs the planted pose is that minimum: the result is within the bound of it too and
    no word is thrown out as an sbaOutlier (the inlier count of the same call without the adjustment, which tier 1 pins).
    On the QUIRK pairs :1253 moves the minimum off the planted pose (asserted on the reference's side: > 2e-3 m from the
    minimum with the From model's own depth frame, which is the planted pose), and the result follows it.  The oracle's
    X = Y runs on these inputs show bound and count (asserted on the oracle's side); the library's are the oracle's bytes.
    Measured on an MI355X, both estimators: every X != Y result 3e-8 .. 2.4e-7 m from the SciPy minimum; the QUIRK minima
    8.8e-3 m (C1, C2), 5.7e-2 m (C2, C0), 6.0e-2 m (C2, C1) off the planted pose, every planted word kept."""
    xs, ys, A, B, Ts = noise_free()
    n = len(A)
    off = oracle_results(noise_free, "to", estimation_type, 0)
    on = oracle_results(noise_free, "to", estimation_type, 0, bundle_adjustment=1)
    for i in range(n):
        if (xs[i], ys[i]) in EQUAL:
            assert on[i]["success"] == 1 and on[i]["inliers"] == off[i]["inliers"], (i, xs[i])
            dt, dr = pose_error(on[i], Ts[i])
            assert xs[i] == 0 or (dt < 1e-3 and dr < 1e-3), (i, dt, dr)
    fr, to = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
    with open_store(cc.base_params(estimation_type), noise_free) as f:
        plain = f.verify_pairs(fr, to)
    p_ba = cc.base_params(estimation_type, bundle_adjustment=1)
    with open_store(p_ba, noise_free) as f:
        got = f.verify_pairs(fr, to)
        lists = [f.debug_correspondences(i, 2) for i in range(n)]    # (the stage kernels keep pass 2's lists)
    bad = []
    for i in range(n):
        combo = (xs[i], ys[i])
        assert plain[i].tobytes() == off[i].tobytes(), i             # (tier 1 once more, on these inputs)
        dt, dr = pose_error(got[i], Ts[i]) if got[i]["success"] else (float("inf"), float("inf"))
        ok = got[i]["success"] == 1
        if combo not in QUIRK:
            ok = ok and got[i]["inliers"] == plain[i]["inliers"]
        if combo in BOUND or (combo in EQUAL and combo != (0, 0)):
            ok = ok and dt < 1e-3 and dr < 1e-3
        note = ""
        if combo in EQUAL:
            ok = ok and got[i].tobytes() == on[i].tobytes()
        else:
            # X != Y against the reference's own cost, minimised by SciPy over the planted words of the library's pass-2
            # list: the result within the bound of the minimum, and as many words left as the minimum leaves inside the kernel
            X, Y = ALL_CAMERAS[xs[i]], ALL_CAMERAS[ys[i]]
            T_ref, words, outside, on_edge = cc.two_view_reference(X, Y, A[i], B[i], lists[i][0], lists[i][1], Ts[i], p_ba)
            et, er = pose_error(got[i], T_ref)
            ok = ok and et < 1e-3 and er < 1e-3 and abs(int(got[i]["inliers"]) - (words - outside)) <= (1 if on_edge else 0)
            note = "; off the reference's minimum %.3e m %.3e rad, it keeps %d of %d words" % (et, er, words - outside, words)
            if combo in QUIRK:
                # :1253 as it stands moves the minimum off the planted pose, and off the minimum of the cost with view 1's depths
                # taken with the From model's own transform -- which IS the planted pose: a silent correction of the line fails here
                T_own = cc.two_view_reference(X, Y, A[i], B[i], lists[i][0], lists[i][1], Ts[i], p_ba, False)[0]
                moved = np.linalg.norm(T_ref[:3, 3] - T_own[:3, 3])
                own_off = np.linalg.norm(T_own[:3, 3] - Ts[i][:3, 3])
                ok = ok and moved > 2e-3 and own_off < 1e-3 and dt > 1e-3
                note += "; :1253 moves the minimum %.3e m" % moved
        print("pair %d (X %d, Y %d): %.3e m %.3e rad off the planted pose, inliers %d / %d%s" % (
            i, xs[i], ys[i], dt, dr, got[i]["inliers"], plain[i]["inliers"], note))
        if not ok:
            bad.append((combo, dt, dr, int(got[i]["inliers"]), int(plain[i]["inliers"]), note))
    assert not bad, bad


def _rigid_inverse(T):
    """sf_oracle.c: sfo_rigid_inverse (double arithmetic in the order written, float results)."""
    R = T.reshape(3, 4)[:, :3].astype(np.float64)
    t = T.reshape(3, 4)[:, 3].astype(np.float64)
    out = np.zeros((3, 4), dtype=np.float32)
    for i in range(3):
        for j in range(3):
            out[i, j] = np.float32(R[j, i])
        out[i, 3] = np.float32(-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]))
    return out.reshape(-1)


def _compose_pass1(p_to, p_from, a, b, valid_to=True, valid_from=True):
    """Pass 1 of PnP with forward_est_only = 0 from the oracle's parts: estimateMotion3DTo2D forward with the To camera
    and backward with the From camera on the oracle's own pass-1 correspondences, merged as sf_oracle.c:1026-1082 does
    (every gate open: both keyframes have K 3D points and min_inliers <= K).  Returns (T [12] float32, is_null, inliers,
    matches)."""
    _, (cf, ct), _ = pyoracle.estimate_transform(p_to, a, b, debug=True)
    mo0, m0 = pyoracle.estimate_motion_3d2d(p_to, a.xyz, b.kpts, b.xyz, cf, ct)
    mo1, m1 = pyoracle.estimate_motion_3d2d(p_from, b.xyz, a.kpts, a.xyz, ct, cf)
    # (valid_to / valid_from False: camera B of that direction is not valid for projection, its gate is closed -- :1059)
    if not valid_to:
        mo0.is_null, m0 = 1, np.zeros_like(m0)
    if not valid_from:
        mo1.is_null, m1 = 1, np.zeros_like(m1)
    inliers = int(np.count_nonzero(m0 | m1))
    matches = int(np.count_nonzero((np.isfinite(a.xyz[cf]).all(axis=1) & valid_to) | (np.isfinite(b.xyz[ct]).all(axis=1) & valid_from)))
    T = np.zeros(12, dtype=np.float32)
    is_null = 1
    if not mo0.is_null:
        T = np.array(mo0.transform, dtype=np.float32)
        is_null = 0
    if not mo1.is_null:
        inv = _rigid_inverse(np.array(mo1.transform, dtype=np.float32))
        if is_null:
            T, is_null = inv, 0
        else:
            A = np.ascontiguousarray(T); Bm = np.ascontiguousarray(inv); mid = np.zeros(12, dtype=np.float32)
            pyoracle.lib().sfo_interpolate_half(C.c_void_p(A.ctypes.data), C.c_void_p(Bm.ctypes.data), C.c_void_p(mid.ctypes.data))
            T = mid
    return T, is_null, inliers, matches


@pytest.mark.gpu
def test_backward_pnp_reads_the_from_keyframes_camera():
    """Tier 3 (b): PnP with forward_est_only = 0 on X != Y.  The oracle has one camera, so pass 1 is composed in the test
    from the oracle's estimateMotion3DTo2D with camera Y forward and camera X backward.  The composition is first held
    against the library on the X = Y pairs of the same call (whose end result tier 2 pins), then applied to X != Y."""
    xs, ys, A, B, _ = nine_combinations()
    n = len(A)
    base = cc.base_params(1, forward_est_only=0)
    with open_store(base, nine_combinations) as f:
        f.set_option(_abi.SF_OPT_DEBUG_CORR, 1)
        f.verify_pairs(np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32))
        states = [f.debug_pass_state(i, 1) for i in range(n)]
    differs = 0
    for equal in (True, False):
        for i in range(n):
            if (xs[i] == ys[i]) != equal:
                continue
            T, is_null, inliers, matches = _compose_pass1(cc.CAMERAS[ys[i]].params(base), cc.CAMERAS[xs[i]].params(base), A[i], B[i])
            gT, g_null, g_inl, g_m = states[i]
            assert (g_null, g_inl, g_m) == (is_null, inliers, matches), (equal, i, xs[i], ys[i])
            assert np.asarray(gT, dtype=np.float32).tobytes() == T.tobytes(), (equal, i, xs[i], ys[i])
            assert not is_null
            if not equal:
                # (the From camera matters: composed with the To camera in both directions the pose is another)
                T2 = _compose_pass1(cc.CAMERAS[ys[i]].params(base), cc.CAMERAS[ys[i]].params(base), A[i], B[i])[0]
                differs += T2.tobytes() != T.tobytes()
    assert differs > 0


@pytest.mark.gpu
def test_a_model_that_is_not_valid_for_projection_closes_its_own_gates():
    """image_width = image_height = 0 in a model, as in sf_params: the guided pass is not eligible towards such a To
    camera (:474), and a PnP direction whose camera B it is does not run (:1059-1065) -- per pair, beside pairs of valid
    cameras in the same call.  Forward only, every result is the oracle's with the To camera (valid or not) in p; with
    both directions pass 1 is the composition of tier 3 (b) with the closed direction left out."""
    rng = np.random.default_rng(4400)
    blind = cc.Camera(cc.C1.fx, cc.C1.fy, cc.C1.cx, cc.C1.cy, 0, 0, cc.C1.L, cc.C1.baseline)
    cams = (cc.C0, cc.C1, blind)
    combos = ((1, 2), (2, 1), (0, 2), (2, 0), (1, 1), (2, 2))
    A, B = [], []
    for x, y in combos:                       # (the keyframes of the model without an image size are C1's)
        a, b, _ = cc.make_pair(rng, cams[min(x, 1)], cams[min(y, 1)])
        A.append(a); B.append(b)
    n = len(combos)
    fr, to = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)

    def store(p):
        f = lib.SeparatorFinder(p, device=0)
        assert [f.camera_add(c.model()) for c in cams[1:]] == [1, 2]
        for k, feats in ((0, A), (1, B)):
            for combo, fa in zip(combos, feats):
                f.camera_select(combo[k])
                f.store_add_keyframe(fa)
        return f

    for estimation_type in (0, 1):
        base = cc.base_params(estimation_type)
        with store(base) as f:
            got = f.verify_pairs(fr, to)
        guided = 0
        for i, (x, y) in enumerate(combos):
            want = pyoracle.estimate_transform(cams[y].params(base), A[i], B[i])
            assert got[i].tobytes() == want.tobytes(), (estimation_type, x, y, got[i], want)
            assert want["pass2_guided"] == (y != 2) and want["success"] == (estimation_type == 0 or y != 2), (estimation_type, x, y)
            guided += int(want["pass2_guided"])
        assert guided == 3
    base = cc.base_params(1, forward_est_only=0)
    with store(base) as f:
        f.set_option(_abi.SF_OPT_DEBUG_CORR, 1)
        got = f.verify_pairs(fr, to)
        states = [f.debug_pass_state(i, 1) for i in range(n)]
    for i, (x, y) in enumerate(combos):
        T, is_null, inliers, matches = _compose_pass1(cams[y].params(base), cams[x].params(base), A[i], B[i], y != 2, x != 2)
        gT, g_null, g_inl, g_m = states[i]
        assert (g_null, g_inl, g_m) == (is_null, inliers, matches), (x, y)
        assert np.asarray(gT, dtype=np.float32).tobytes() == T.tobytes(), (x, y)
        assert is_null == (x == 2 and y == 2)
        assert got[i]["pass2_guided"] == (y != 2) and got[i]["pass1_success"] == (not is_null), (x, y)


@pytest.mark.gpu
def test_camera_ids_follow_every_append_path_and_survive_growth():
    """sf_camera_select stamps the host add, the device add, one extraction call, one batch call and the import; the ids
    survive the store's growth; sf_store_clear drops them and keeps the table and the selection."""
    import torch
    from multi_robot_slam_separators_amd import synth
    dev = torch.device("cuda:0")
    p = cc.base_params(0)
    p.store_capacity = 4                  # the store grows while the test appends
    rng = np.random.default_rng(5)
    with lib.SeparatorFinder(p, device=0) as f:
        assert f.camera_count() == 0 and f.store_size() == 0
        c1, c2 = f.camera_add(cc.C1.model()), f.camera_add(cc.C2.model())
        assert (c1, c2) == (1, 2) and f.camera_count() == 2
        m = f.camera_get(2)
        assert bytes(m) == bytes(cc.C2.model())
        m0 = f.camera_get(0)
        assert (m0.fx, m0.fy, m0.cx, m0.cy, m0.image_width, m0.image_height) == (600.0, 600.0, 320.0, 240.0, 640, 480)
        want = []
        f.store_add_keyframe(cc.make_keyframe(rng, cc.C0)); want += [0]        # a fresh handle selects 0
        f.camera_select(1)
        f.store_add_keyframe(cc.make_keyframe(rng, cc.C1)); want += [1]        # host add
        f.camera_select(2)
        k = 64
        feats = synth.make_store_batch(3, 3, k=k, cols=32)
        T = {key: torch.from_numpy(np.ascontiguousarray(feats[key]).view(np.uint8) if feats[key].dtype.fields else
                                   np.ascontiguousarray(feats[key])).to(dev) for key in ("desc_a", "xyz_a", "kp_a")}
        first = f.store_add_keyframes_device(3, k, 32, T["desc_a"].data_ptr(), T["xyz_a"].data_ptr(), T["kp_a"].data_ptr())
        assert first == 2; want += [2, 2, 2]                                    # device add
        f.camera_select(1)
        # one extraction call (host images) and one batch call (device images, two keyframes): a textured stereo pair
        h, w = 96, 128
        tex = np.kron(rng.integers(0, 256, size=(h // 8, w // 8 + 1), dtype=np.uint8), np.ones((8, 8), dtype=np.uint8))
        left, right = np.ascontiguousarray(tex[:, 4:4 + w]), np.ascontiguousarray(tex[:, :w])
        cam = _abi.stereo_camera(100.0, 100.0, w / 2.0, h / 2.0, 0.1)
        slot = f.get_features_and_descriptor(left, right, cam)[3]
        assert slot == len(want); want += [1]
        f.camera_select(0)
        d_left = torch.from_numpy(np.stack([left, left])).to(dev)
        d_right = torch.from_numpy(np.stack([right, right])).to(dev)
        first = f.get_features_and_descriptor_batch_device(d_left.data_ptr(), d_right.data_ptr(), 2, w, h, w, w * h, cam)
        assert first == len(want); want += [0, 0]
        f.synchronize()
        f.camera_select(2)
        # import: the blob of slots [0, 2) comes back as two more slots, stamped with the selection, not with their old ids
        total, max_rows = f.export_plan(0, 2)
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        f.export_keyframes_device(0, 2, blob.data_ptr(), total)
        f.import_keyframes_device(blob.data_ptr(), total, 2, max_rows, 32)
        f.wire_status()
        want += [2, 2]
        assert f.store_size() == len(want) > p.store_capacity
        assert [f.store_get_camera(s) for s in range(len(want))] == want
        f.store_set_camera(1, 3, 0)
        want[1:4] = [0, 0, 0]
        assert [f.store_get_camera(s) for s in range(len(want))] == want
        # refusals leave everything as it is
        bad = cc.C1.model(); bad.fx = float("nan")
        neg = cc.C1.model(); neg.stereo_baseline = -1.0
        nonf = cc.C1.model(); nonf.local_transform[3] = float("inf")
        for call in (lambda: f.camera_add(bad), lambda: f.camera_add(neg), lambda: f.camera_add(nonf),
                     lambda: f.camera_select(3), lambda: f.camera_select(-1), lambda: f.camera_get(3),
                     lambda: f.store_set_camera(0, len(want) + 1, 1), lambda: f.store_set_camera(-1, 1, 1),
                     lambda: f.store_set_camera(0, 1, 9), lambda: f.store_get_camera(len(want))):
            with pytest.raises(lib.SepfinderError) as e:
                call()
            assert e.value.code == _abi.SF_EINVAL
        assert f.camera_count() == 2
        assert [f.store_get_camera(s) for s in range(len(want))] == want
        f.store_add_keyframe(cc.make_keyframe(rng, cc.C2)); want += [2]         # (the selection is still 2)
        assert f.store_get_camera(len(want) - 1) == 2
        f.store_clear()
        assert f.store_size() == 0 and f.camera_count() == 2
        f.store_add_keyframe(cc.make_keyframe(rng, cc.C2))
        assert f.store_get_camera(0) == 2                                       # the table and the selection stay
        f.store_set_camera(0, 1, 0)
        assert f.store_get_camera(0) == 0


@pytest.mark.gpu
def test_a_store_without_ids_keeps_its_launch_form_and_its_bytes():
    """Cameras in the table but no slot tagged: the call plans as before (the fused kernel keeps its correspondence lists
    in LDS: sf_debug_correspondences refuses) and gives the handle's-camera results, those of a handle without a table.
    The first non-zero id sends the same call to the stage kernels (the lists are in HBM)."""
    xs, ys, A, B, _ = equal_cameras()
    n = len(A)
    fr, to = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
    p = cc.base_params(0)
    with lib.SeparatorFinder(p, device=0) as f:
        for fa in A + B:
            f.store_add_keyframe(fa)
        plain = f.verify_pairs(fr, to)
    with open_store(p, equal_cameras, tag=False) as f:
        got = f.verify_pairs(fr, to)
        assert got.tobytes() == plain.tobytes()
        with pytest.raises(lib.SepfinderError):
            f.debug_correspondences(0, 1)
        f.store_set_camera(0, 1, 1)
        f.verify_pairs(fr, to)
        f.debug_correspondences(0, 1)
        f.store_set_camera(0, 1, 0)
        again = f.verify_pairs(fr, to)
        assert again.tobytes() == plain.tobytes()
        with pytest.raises(lib.SepfinderError):
            f.debug_correspondences(0, 1)
        # sf_estimate_transform keeps the reference's cam_, cam_: its scratch slots carry id 0 whatever is selected
        f.camera_select(2)
        one = f.estimate_transform(A[1], B[1])
        assert one.tobytes() == pyoracle.estimate_transform(p, A[1], B[1]).tobytes()
