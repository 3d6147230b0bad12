"""GPU: what the five detectors (GFTT, FAST, ORB, SURF, SIFT) return, pinned where "a batch equals the single calls" cannot
pin it.  Every detector has ONE launcher for one image and for many, so the batch tests compare a code path with itself;
here a batch is compared with the restatements directly, and the single calls are held to what only they do: no limit with
a short output, the refusal of an overflow, and leaving the batch status and the SIFT pyramid as their callers expect.

1. one batch call on three images -- two textured images of the detector's own test module (the 160 x 120 class), one of
   them cut at max_features and one not, and a flat image -- against restatement detector -> the oracle's stereo
   correspondence -> restatement extraction, byte for byte (rows, 3D points, keypoints, row counts);
2. max_features = 0 (no limit) with cap below the number found: the count is the restatement's, the first cap rows are
   its rows, nothing behind row cap is touched (FAST, GFTT, SURF, SIFT; ORB demands max_features >= 1);
3. SURF and SIFT single calls under a candidate capacity one below the image's count: SF_ERANGE with count and capacity
   (SIFT: the stage) in the message, n_out 0, the output untouched; at the count itself: the restatement's bytes;
4. a single call after a batch with an overflowed keyframe: sf_*_batch_status still reports the batch's 1; a single SIFT
   call after a batch makes sf_debug_sift_plane work again.
k_gftt_select, the selection of an image past the LDS bitmap, runs in tests/test_gpu_gftt.py (1920 x 1080)."""
import ctypes as C
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from oracle import pyoracle
from tests import extract_cases as ec
from tests import fast_ref, orb2_ref, orb_ref, sift_ref, surf_ref
from tests import sift_batch_cases, surf_batch_cases
from tests import test_gpu_orb2, test_gpu_sift_batch, test_gpu_surf, test_gpu_surf_batch
from tests.test_gpu_orb import assert_same as assert_same_binary
from tests.test_gpu_orb2_batch import batch_pairs, run_batch as run_batch_binary

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
SENTINEL = 0xEE
FAST_T, FAST_LIMIT = 10, 300                        # tests/test_gpu_fast.py "odd pitch t10 limit 300"
GFTT = (50, 0.01, 7.0)                              # tests/test_gpu_gftt.py: max_corners of seed 5, the rest of seed 2
ORB = (202, 170, 1.2, 8, 1, 200)                    # tests/test_gpu_orb2_batch.py "202x170 s1.2 l8", FAST score, MAXF


def _cam(w, h):
    return _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)


def _binary_finder():
    import torch
    p = synth.camera_params()
    p.max_features = 2048
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


@functools.lru_cache(maxsize=None)
def corner_pairs(kind):
    """Three pairs of one size: A an image of the detector's test module, B = A with the columns from w // 3 on set to 128
    (fewer corners than the limit), C flat; the right image is the left one shifted by 6 pixels.
    B is derived, not a second case image: a batch takes images of ONE size, and the small case images of
    tests/test_gpu_gftt.py (160 x 120, 131 x 97, 64 x 64, 70 x 50, 35 x 33) each have a size of their own, while
    tests/test_gpu_fast.py has a single small one (131 x 97, pitch 134).  What B is for -- an image that max_features does
    not cut, next to one that it does -- is asserted on the restatement's counts (_assert_cut_and_uncut)."""
    a = np.ascontiguousarray(ec.make_case(13, n=1, width=131, height=97, pad=3)[0] if kind == "fast" else
                             ec.make_case(2, n=1, width=131, height=97)[0])
    b = a.copy()
    b[:, a.shape[1] // 3:] = 128
    out = [(l, np.ascontiguousarray(np.roll(l, -6, axis=1))) for l in (a, b, np.full_like(a, 77))]
    for l, r in out:
        l.setflags(write=False)
        r.setflags(write=False)
    return out


def _stereo(left, right, kp):
    xy, st, _ = pyoracle.stereo_correspondences(left, right, kp, None)
    return np.ascontiguousarray(xy[:, 0]), st


def _brief_chain(kp, left, right, cam, tests):
    if len(kp) == 0:
        return np.zeros((0, tests.shape[0] // 8), np.uint8), np.zeros((0, 3), np.float32), kp
    rx, st = _stereo(left, right, kp)
    return pyoracle.extract_keyframe(left, kp, rx, st, cam, tests)


def _float_chain(ref, kp, left, right, cam, dims):
    if len(kp) == 0:
        return np.zeros((0, dims), np.float32), np.zeros((0, 3), np.float32), kp
    rx, st = _stereo(left, right, kp)
    return ref.extract_keyframe(left, kp, rx, st, cam, ref.Params())


def _assert_cut_and_uncut(found, limit):
    """The precondition of every batch below, on the restatement's counts alone."""
    print("restatement keypoints before the cut %s, max_features %d" % (found, limit))
    assert found[0] > limit and 0 < found[1] <= limit and found[2] == 0


# ---- 1. a batch against the restatements ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fast", "gftt"])
def test_corner_batch_equals_restatement(kind):
    import torch
    pairs = corner_pairs(kind)
    h, w = pairs[0][0].shape
    cam, tests = _cam(w, h), ec.brief_tests(5, 32)
    if kind == "fast":
        limit = FAST_LIMIT
        found = [len(fast_ref.detect(l, FAST_T, 1, 0)) for l, _ in pairs]
        kps = [fast_ref.detect(l, FAST_T, 1, limit) for l, _ in pairs]
        det = _abi.detector_params(limit)
    else:
        limit, q, md = GFTT
        found = [len(pyoracle.detect_corners(l, 0, q, md)) if l.min() != l.max() else 0 for l, _ in pairs]
        kps = [pyoracle.detect_corners(l, limit, q, md) if l.min() != l.max() else np.zeros(0, KP) for l, _ in pairs]
        det = _abi.detector_params(limit, q, md)
    _assert_cut_and_uncut(found, limit)
    assert [len(k) for k in kps] == [limit, found[1], 0]
    f = _binary_finder()
    try:
        f.brief_set_pattern(tests)
        if kind == "fast":
            f.set_feature_type(_abi.FEATURE_FAST_BRIEF)
            f.fast_set_params(_abi.fast_params(FAST_T))
        first, got = run_batch_binary(f, torch, pairs, w, h, w + 3, (w + 3) * h + 40, cam, det,
                                      call=f.get_features_and_descriptor_batch_device)
    finally:
        f.close()
    for i, (l, r) in enumerate(pairs):
        want = _brief_chain(kps[i], l, r, cam, tests)
        assert len(got[i][0]) == len(want[0]), i
        assert_same_binary(got[i], want)
    assert len(got[0][0]) > len(got[1][0]) > 0 and len(got[2][0]) == 0


def test_orb_batch_equals_restatement():
    import torch
    w, h, sf, nl, score, maxf = ORB
    pairs = batch_pairs(w, h)[:3]                                               # A, B, flat C
    found = [sum(len(d["kp"]) for d in orb2_ref.detect_levels(l, maxf, sf, nl, 19, score, 20)) for l, _ in pairs]
    _assert_cut_and_uncut(found, maxf)
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    f = lib.SeparatorFinder(test_gpu_orb2._params(), device=0)
    try:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        f.set_feature_type_orb(_abi.orb_detector_params(sf, nl, 0, score, 20))
        first, got = run_batch_binary(f, torch, pairs, w, h, w + 8, (w + 8) * h + 72, cam, det)
    finally:
        f.close()
    for i, (l, r) in enumerate(pairs):
        if found[i] == 0:
            assert len(got[i][0]) == 0
            continue
        want = test_gpu_orb2._chain(l, r, cam, orb_ref.default_pattern(), maxf, sf, nl, score)
        assert len(got[i][0]) == len(want[0]), i
        assert_same_binary(got[i], want)
    assert len(got[0][0]) > len(got[1][0]) > 0


@pytest.mark.parametrize("kind", ["surf", "sift"])
def test_float_batch_equals_restatement(kind):
    import torch
    cases, ref, mod, dims = ((surf_batch_cases, surf_ref, test_gpu_surf_batch, 64) if kind == "surf" else
                             (sift_batch_cases, sift_ref, test_gpu_sift_batch, 128))
    shape = "160x120"
    pairs, maxf = cases.pairs(shape)[:3], cases.MAXF[shape]                     # A, B, flat C
    _assert_cut_and_uncut(cases.COUNTS[shape][0][:3], maxf)
    kps = [ref.detect(l, ref.Params(), maxf) for l, _ in pairs]
    assert [len(k) for k in kps] == [maxf, cases.COUNTS[shape][0][1], 0]
    h, w = pairs[0][0].shape
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    f = test_gpu_surf._finder(dims)
    try:
        if kind == "surf":
            f.set_feature_type_surf()
        else:
            f.set_feature_type_sift()
        first, got = mod.run_batch(f, torch, pairs, w, h, 173, 173 * h + 72, cam, det)
        status = f.surf_batch_status() if kind == "surf" else f.sift_batch_status()
    finally:
        f.close()
    assert status == 0
    for i, (l, r) in enumerate(pairs):
        want = _float_chain(ref, kps[i], l, r, cam, dims)
        assert len(got[i][0]) == len(want[0]), i
        test_gpu_surf.assert_same(got[i], want, dims)
    assert len(got[0][0]) > 0 and len(got[1][0]) > 0 and len(got[2][0]) == 0


# ---- 2. no limit and a short output -----------------------------------------------------------------------------------
def _single(call, torch, image, cap):
    """A single detector call with a sentinel-filled output of cap + 4 rows: (n_out, the first cap rows, the rest)."""
    dev = torch.device("cuda:0")
    h, w = image.shape
    d_img = torch.from_numpy(np.array(image)).to(dev)                          # (a copy: the cached images are read-only)
    out = torch.full((cap + 4, KP.itemsize), SENTINEL, dtype=torch.uint8, device=dev)
    n = call(d_img.data_ptr(), w, h, w, out.data_ptr(), cap)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    return n, np.frombuffer(raw[:cap].tobytes(), dtype=KP), raw[cap:]


@pytest.mark.parametrize("kind", ["fast", "gftt", "surf", "sift"])
def test_no_limit_and_a_short_output(kind):
    import torch
    f = _binary_finder()
    try:
        if kind == "fast":
            image = corner_pairs("fast")[0][0]
            want = fast_ref.detect(image, FAST_T, 1, 0)
            call = lambda p, w, h, pitch, out, cap: f.detect_fast_device(p, w, h, pitch, 0, out, cap, _abi.fast_params(FAST_T, 1))
        elif kind == "gftt":
            image = corner_pairs("gftt")[0][0]
            want = pyoracle.detect_corners(image, 0, GFTT[1], GFTT[2])
            call = lambda p, w, h, pitch, out, cap: f.detect_corners_device(p, w, h, pitch, 0, GFTT[1], GFTT[2], out, cap)
        elif kind == "surf":
            image = surf_batch_cases.left_images("160x120")[0]
            want = surf_batch_cases.detected("160x120", 0, "defaults")
            call = lambda p, w, h, pitch, out, cap: f.detect_surf(p, w, h, pitch, 0, out, cap, _abi.surf_params())
        else:
            image = sift_batch_cases.left_images("160x120")[0]
            want = sift_batch_cases.detected("160x120", 0)[0]
            call = lambda p, w, h, pitch, out, cap: f.detect_sift(p, w, h, pitch, 0, out, cap, _abi.sift_params())
        cap = len(want) // 3
        assert cap >= 5
        n, rows, rest = _single(call, torch, image, cap)
    finally:
        f.close()
    print("%s: %d found, cap %d" % (kind, len(want), cap))
    assert n == len(want)                                                       # the number found, unclipped by cap
    assert rows.tobytes() == want[:cap].tobytes()
    assert (rest == SENTINEL).all()                                             # nothing behind row cap


# ---- 3. refusal leaves the output alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,stage", [("surf", "maxima"), ("sift", "extrema"), ("sift", "keypoints")])
def test_refusal_leaves_the_output_alone(kind, stage):
    import torch
    if kind == "surf":
        image = surf_batch_cases.left_images("160x120")[0]
        want = surf_batch_cases.detected("160x120", 0, "defaults")
        count = len(want)
    else:
        image = sift_batch_cases.left_images("160x120")[0]
        want, extrema = sift_batch_cases.detected("160x120", 0)
        # (182 keypoints of 163 extrema: a capacity of 181 holds the extrema and refuses the keypoints)
        count = extrema if stage == "extrema" else len(want)
        assert extrema < len(want)
    f = _binary_finder()
    try:
        limits = f.debug_surf_limits if kind == "surf" else f.debug_sift_limits
        call = ((lambda p, w, h, pitch, out, cap: f.detect_surf(p, w, h, pitch, 0, out, cap, _abi.surf_params())) if kind == "surf" else
                (lambda p, w, h, pitch, out, cap: f.detect_sift(p, w, h, pitch, 0, out, cap, _abi.sift_params())))
        limits(count - 1)
        with pytest.raises(lib.SepfinderError) as e:
            _single(call, torch, image, len(want))
        msg = str(e.value)
        print(msg)
        assert e.value.code == _abi.SF_ERANGE
        assert "%d %s" % (count, stage) in msg and "capacity %d" % (count - 1) in msg
        # the refused call again, by hand: n_out stays 0 and the sentinels stay
        dev = torch.device("cuda:0")
        h, w = image.shape
        d_img = torch.from_numpy(np.array(image)).to(dev)
        out = torch.full((len(want) + 4, KP.itemsize), SENTINEL, dtype=torch.uint8, device=dev)
        n = C.c_int32(-5)
        sym = f._L.sf_detect_surf_device if kind == "surf" else f._L.sf_detect_sift_device
        rc = sym(f._h, C.c_void_p(d_img.data_ptr()), w, h, w, 0, None, C.c_void_p(out.data_ptr()), len(want), C.byref(n))
        torch.cuda.synchronize()
        assert rc == _abi.SF_ERANGE and n.value == 0
        assert (out.cpu().numpy() == SENTINEL).all()
        if stage != "extrema":                                                  # the capacity equal to the count: no refusal
            limits(count)
            n, rows, rest = _single(call, torch, image, len(want))
            assert n == len(want) and rows.tobytes() == want.tobytes() and (rest == SENTINEL).all()
    finally:
        f.close()


# ---- 4. single calls do not disturb the batch status ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["surf", "sift"])
def test_single_calls_leave_the_batch_status(kind):
    import torch
    cases, mod, dims = ((surf_batch_cases, test_gpu_surf_batch, 64) if kind == "surf" else
                        (sift_batch_cases, test_gpu_sift_batch, 128))
    shape = "160x120"
    pairs, maxf = cases.pairs(shape)[:3], cases.MAXF[shape]                     # A overflows, B and the flat C fit
    counts = cases.COUNTS[shape][0]
    cap = counts[1] + 1
    assert counts[0] > cap > counts[1] > 0
    if kind == "sift":
        assert sift_batch_cases.EXTREMA[shape][1] <= cap
    h, w = pairs[0][0].shape
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    image = pairs[1][0]                                                         # B: a fitting image for the single call
    want = (surf_batch_cases.detected(shape, 1, "defaults") if kind == "surf" else sift_batch_cases.detected(shape, 1)[0])
    dev = torch.device("cuda:0")
    f = test_gpu_surf._finder(dims)
    try:
        if kind == "surf":
            f.set_feature_type_surf()
            f.debug_surf_limits(cap, 0)
            status = lambda: f.surf_batch_status(check=False)
            call = lambda p, w, h, pitch, out, n: f.detect_surf(p, w, h, pitch, 0, out, n)
        else:
            f.set_feature_type_sift()
            f.debug_sift_limits(cap)
            status = lambda: f.sift_batch_status(check=False)
            call = lambda p, w, h, pitch, out, n: f.detect_sift(p, w, h, pitch, 0, out, n)
        first, got = mod.run_batch(f, torch, pairs, w, h, w, w * h, cam, det)
        assert [len(g[0]) > 0 for g in got] == [False, True, False]
        assert status() == 1
        if kind == "sift":                                                      # a batch retires the single call's pyramid
            plane = torch.zeros((2 * h, 2 * w), dtype=torch.int16, device=dev)
            with pytest.raises(lib.SepfinderError):
                f.debug_sift_plane(0, 0, 0, plane.data_ptr())
        n, rows, rest = _single(call, torch, image, len(want))
        assert n == len(want) and rows.tobytes() == want.tobytes()
        assert status() == 1                                                    # still the batch's count
        if kind == "sift":
            f.debug_sift_plane(0, 0, 0, plane.data_ptr())                       # ... and the pyramid is the single call's
            torch.cuda.synchronize()
            trace = {}
            sift_ref.detect(image, sift_ref.Params(), 0, trace)
            assert np.array_equal(plane.cpu().numpy(), trace["gauss"][0][0])
    finally:
        f.close()
