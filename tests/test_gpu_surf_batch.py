"""GPU: the batch form of SURF (Vis/FeatureType 0): sf_get_features_and_descriptor_surf_batch_device through the C-ABI.  The
yardstick is the single call on a second handle -- keyframe i of a batch carries the bytes of
sf_get_features_and_descriptor on pair i (row count, float32 rows, 3D points with their NaNs, keypoints with all seven
fields, and the store slot through the verification path) -- which tests/test_gpu_surf.py pins to the restatement
tests/surf_ref.py.  The images are tests/surf_batch_cases.py's; the preconditions that make them worth running are asserted
on the restatement alone.  Every test calls a symbol that the library did not have before the batch form."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import extract_cases as ec
from tests import surf_batch_cases as cases
from tests.test_gpu_orb2_batch import SENTINEL, pack
from tests.test_gpu_surf import PARAM_SETS, _finder, assert_same

pytestmark = pytest.mark.gpu

# name: (parameter set of tests/test_gpu_surf.py or None, further sf_surf_params, dimensions)
SETS = {
    "defaults": ("defaults", {}, 64),
    "threshold 0": ("threshold 0", {}, 64),
    "upright": (None, dict(upright=1), 64),
    "extended": (None, dict(extended=1), 128),
}
REFINE = (3, 5, 0.02)


def _surf(name):
    pset, extra, dims = SETS[name]
    return _abi.surf_params(**dict(PARAM_SETS[pset] if pset else {}, **extra)), dims


def _cam(w, h):
    return _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)


def _layout(shape, padded):
    h, w = cases.left_images(shape)[0].shape
    pitch = 173 if shape == "160x120" and padded else w
    return w, h, pitch, pitch * h + (72 if padded else 0)                  # padded: a stride that leaves a gap


def assert_preconditions(shape, name):
    """On the restatement alone (the detector does not read upright / extended: those sets detect as the defaults)."""
    pset = SETS[name][0] or "defaults"
    kps = [cases.detected(shape, i, pset) for i in range(len(cases.left_images(shape)))]
    n = [len(k) for k in kps]
    maxf = cases.MAXF[shape]
    want = cases.COUNTS[shape][1 if pset == "threshold 0" else 0]
    print("%s, %s: restatement keypoints %s, max_features %d" % (shape, name, n, maxf))
    assert n == want
    if shape == "160x120":
        resp = kps[0]["response"]
        assert n[0] > maxf and n[4] > maxf                                  # A, E: limitKeypoints cuts
        assert (np.diff(resp) <= 0).all() and resp[maxf - 1] == resp[maxf]  # ... between two equal responses
        assert 0 < n[1] < maxf and 0 < n[3] < maxf and n[2] == 0            # B, D: under the limit; C: nothing
        if pset == "defaults":
            assert n[0] - len(np.unique(resp)) == 35
    else:
        assert n[0] > maxf and n[1] == 0


def run_batch(f, torch, pairs, w, h, pitch, stride, cam, det):
    """The batch call on `pairs` with sentinel-filled outputs one row longer than the call may write.  Returns the first
    slot and, per keyframe, (desc bytes, xyz, kp) cut to its rows."""
    dev = torch.device("cuda:0")
    n, maxf, nb = len(pairs), det.max_features, f.descriptor_bytes()
    L = pack(torch, [p[0] for p in pairs], w, h, pitch, stride)
    R = pack(torch, [p[1] for p in pairs], w, h, pitch, stride)
    ksz = _abi.KEYPOINT_DTYPE.itemsize
    rows = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    desc = torch.full((n * maxf + 1, nb), SENTINEL, dtype=torch.uint8, device=dev)
    xyz = torch.full((n * maxf + 1, 12), SENTINEL, dtype=torch.uint8, device=dev)
    kp = torch.full((n * maxf + 1, ksz), SENTINEL, dtype=torch.uint8, device=dev)
    first = f.get_features_and_descriptor_surf_batch_device(L.data_ptr(), R.data_ptr(), n, w, h, pitch, stride, cam, det, None,
                                                            rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
    torch.cuda.synchronize()
    rows, desc, xyz, kp = (t.cpu().numpy() for t in (rows, desc, xyz, kp))
    assert rows[n] == -7                                                    # nothing behind the blocks
    assert (desc[n * maxf:] == SENTINEL).all() and (xyz[n * maxf:] == SENTINEL).all() and (kp[n * maxf:] == SENTINEL).all()
    out = []
    for i in range(n):
        r = int(rows[i])
        assert 0 <= r <= maxf
        blk = slice(i * maxf, (i + 1) * maxf)
        for a in (desc[blk], xyz[blk], kp[blk]):
            assert (a[r:] == SENTINEL).all(), "keyframe %d: written past its %d rows" % (i, r)
        out.append((desc[blk][:r].copy(), np.frombuffer(xyz[blk][:r].tobytes(), np.float32).reshape(r, 3),
                    np.frombuffer(kp[blk][:r].tobytes(), dtype=_abi.KEYPOINT_DTYPE)))
    return first, out


def _configure(f, name, bm=False, refine=None):
    f.set_feature_type_surf(_surf(name)[0])
    if bm:
        f.stereo_set_params(_abi.stereo_params(0, 1))
    if refine:
        f.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), *refine))


@functools.lru_cache(maxsize=None)
def singles(shape, name, bm=False, refine=None):
    """The single calls on every pair of a shape, on a handle of their own: computed once, shared, left unchanged."""
    w, h = _layout(shape, False)[:2]
    f = _finder(_surf(name)[1])
    try:
        _configure(f, name, bm, refine)
        out = [f.get_features_and_descriptor(l, r, _cam(w, h), _abi.detector_params(cases.MAXF[shape]))
               for l, r in cases.pairs(shape)]
    finally:
        f.close()
    for s in out:
        for a in s[:3]:
            a.setflags(write=False)
    return out


def batch_on_fresh_handle(torch, shape, name, pairs, padded=True, bm=False, refine=None, limits=None):
    w, h, pitch, stride = _layout(shape, padded)
    f = _finder(_surf(name)[1])
    try:
        _configure(f, name, bm, refine)
        if limits:
            f.debug_surf_limits(*limits)
        before = f.store_size()
        first, got = run_batch(f, torch, pairs, w, h, pitch, stride, _cam(w, h), _abi.detector_params(cases.MAXF[shape]))
        assert first == before and f.store_size() == before + len(pairs)   # the first slot is returned
        assert f.surf_batch_status() == 0
    finally:
        f.close()
    return got


def assert_batch_equals(got, want, dims):
    assert len(got) == len(want)
    for i, (g, s) in enumerate(zip(got, want)):
        assert len(g[0]) == len(s[0]), "keyframe %d: %d rows, the single call %d" % (i, len(g[0]), len(s[0]))
        assert_same(g, s[:3], dims)


@pytest.mark.parametrize("shape,name", [("160x120", n) for n in SETS] + [("97x61", "defaults")])
def test_batch_equals_single_calls(shape, name):
    import torch
    assert_preconditions(shape, name)
    dims = _surf(name)[1]
    want = singles(shape, name)
    pset = SETS[name][0] or "defaults"
    for i, s in enumerate(want):                                            # the yardstick saw what the restatement sees
        assert len(s[0]) <= cases.MAXF[shape] and len(s[0]) <= len(cases.detected(shape, i, pset))
    assert len(want[0][0]) > 0 and s[0].shape[1] == 4 * dims
    assert len(want[0][2]) and (want[0][2]["angle"] == 270.0).all() == (name == "upright")
    got = batch_on_fresh_handle(torch, shape, name, cases.pairs(shape))
    assert_batch_equals(got, want, dims)
    assert len(got[2 if shape == "160x120" else 1][0]) == 0                 # the flat pair in the middle: no rows
    assert_same(got[-1], got[0], dims)                                      # the last pair is the first again
    again = batch_on_fresh_handle(torch, shape, name, cases.pairs(shape))   # a fresh handle: the same bytes
    for a, g in zip(again, got):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, g))


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunks_do_not_show(chunk):
    """Forced chunks of 1 (five launches) and 2 (2, 2 and 1 images) give the bytes of the automatic plan (one chunk)."""
    import torch
    assert lib.surf_batch_plan(160, 120, 5)[1] == 5                         # the automatic plan: all five in one chunk
    auto = batch_on_fresh_handle(torch, "160x120", "defaults", cases.pairs("160x120"))
    got = batch_on_fresh_handle(torch, "160x120", "defaults", cases.pairs("160x120"), limits=(0, chunk))
    for a, g in zip(auto, got):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, g))
    assert_batch_equals(got, singles("160x120", "defaults"), 64)


def test_overflow_is_reported_not_truncated():
    """candidate_cap 40 under the defaults: A and E (86 maxima) hold no rows and empty slots, B, C and D the bytes of the
    uncapped run; the status call reports 2 with SF_ERANGE; the single call refuses A and accepts B; with the limits back
    at their defaults the next batch on the same handle reports 0 and equals the single calls."""
    import torch
    shape, cap = "160x120", 40
    counts = cases.COUNTS[shape][0]
    assert counts[0] > cap and counts[4] > cap and max(counts[1:4]) <= cap
    w, h, pitch, stride = _layout(shape, True)
    cam, det = _cam(w, h), _abi.detector_params(cases.MAXF[shape])
    want = singles(shape, "defaults")
    pairs = cases.pairs(shape)
    f = _finder(64)
    try:
        f.set_feature_type_surf()
        f.debug_surf_limits(cap, 0)
        first, got = run_batch(f, torch, pairs, w, h, pitch, stride, cam, det)
        assert f.store_size() == first + 5
        assert [len(g[0]) for g in got] == [0, len(want[1][0]), 0, len(want[3][0]), 0]
        for i in (1, 2, 3):
            assert_same(got[i], want[i][:3], 64)
        assert f.surf_batch_status(check=False) == 2
        with pytest.raises(lib.SepfinderError) as e:
            f.surf_batch_status()
        assert e.value.code == _abi.SF_ERANGE and "hessian_threshold" in str(e.value)
        res = f.verify_pairs([first, first + 4, first + 2], [first, first + 4, first + 2])   # A, E as empty as the flat C
        for k in ("success", "matches", "inliers"):
            assert res[k].tolist() == [0, 0, 0], k
        size = f.store_size()
        with pytest.raises(lib.SepfinderError) as e:                        # the single call under the same cap
            f.get_features_and_descriptor(*pairs[0], cam, det)
        assert e.value.code == _abi.SF_ERANGE and "hessian_threshold" in str(e.value) and f.store_size() == size
        b = f.get_features_and_descriptor(*pairs[1], cam, det)
        assert_same(b[:3], want[1][:3], 64)
        f.debug_surf_limits(0, 0)
        first2, got2 = run_batch(f, torch, pairs, w, h, pitch, stride, cam, det)
        assert first2 == size + 1 and f.surf_batch_status() == 0
        assert_batch_equals(got2, want, 64)
    finally:
        f.close()


@pytest.mark.parametrize("bm,refine", [(True, None), (False, REFINE)])
def test_block_matching_and_refinement(bm, refine):
    import torch
    want = singles("160x120", "defaults", bm, refine)[:3]
    plain = singles("160x120", "defaults")
    assert len(want[0][0]) > 0 and len(want[1][0]) > 0 and len(want[2][0]) == 0
    if refine:                                                              # not vacuous: the refinement moved keypoints
        assert want[0][2].tobytes() != plain[0][2].tobytes()
    else:                                                                   # ... block matching gave other 3D points
        assert want[0][1].tobytes() != plain[0][1].tobytes() and np.isfinite(want[0][1]).all(axis=1).any()
    got = batch_on_fresh_handle(torch, "160x120", "defaults", cases.pairs("160x120")[:3], bm=bm, refine=refine)
    assert_batch_equals(got, want, 64)


def _state(f):
    return f.get_feature_type()[0], bytes(f.get_surf_params()), f.store_size(), f.nn_sizes()


def _refused(f, call, code, *words):
    before = _state(f)
    with pytest.raises(lib.SepfinderError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for word in words:
        assert word in str(e.value), str(e.value)
    assert _state(f) == before
    return str(e.value)


def test_refusals_change_nothing():
    import torch
    dev = torch.device("cuda:0")
    w, h = 64, 48
    cam, det = _cam(w, h), _abi.detector_params(50)
    p = torch.zeros((2, h * w), dtype=torch.uint8, device=dev).data_ptr()
    rgb = torch.zeros((2, h * 3 * w), dtype=torch.uint8, device=dev).data_ptr()
    f = _finder(64)
    try:
        surf, add = f.get_features_and_descriptor_surf_batch_device, f.add_keyframes_surf_u8_batch_device
        # a handle that is not of type 0 (a fresh one: 6): SF_EINVAL, the right call named, n = 0 included
        assert f.get_feature_type()[0] == 6
        for n in (2, 0):
            _refused(f, lambda: surf(p, p, n, w, h, w, w * h, cam, det), _abi.SF_EINVAL, "sf_get_features_and_descriptor_batch_device")
            _refused(f, lambda: add(rgb, rgb, None, 0, n, w, h, 3 * w, 3 * w * h, cam, det), _abi.SF_EINVAL,
                     "sf_add_keyframes_u8_batch_device")
        f.set_feature_type_surf(_abi.surf_params(hessian_threshold=400.0))
        assert _state(f)[0] == 0
        # the four existing batch calls keep refusing type 0, and name the new ones
        for call in (f.get_features_and_descriptor_batch_device, f.get_features_and_descriptor_orb_batch_device):
            _refused(f, lambda: call(p, p, 2, w, h, w, w * h, cam, det), _abi.SF_EINVAL,
                     "sf_get_features_and_descriptor_surf_batch_device", "sf_add_keyframes_surf_u8_batch_device")
        for call in (f.add_keyframes_u8_batch_device, f.add_keyframes_orb_u8_batch_device):
            _refused(f, lambda: call(rgb, rgb, None, 0, 2, w, h, 3 * w, 3 * w * h, cam, det), _abi.SF_EINVAL,
                     "sf_get_features_and_descriptor_surf_batch_device", "sf_add_keyframes_surf_u8_batch_device")
        # arguments
        _refused(f, lambda: surf(None, p, 2, w, h, w, w * h, cam, det), _abi.SF_EINVAL)
        _refused(f, lambda: surf(p, None, 2, w, h, w, w * h, cam, det), _abi.SF_EINVAL)
        _refused(f, lambda: surf(p, p, 2, w, h, w, w * h - 1, cam, det), _abi.SF_EINVAL, "stride")
        _refused(f, lambda: surf(p, p, 2, w, h, w - 1, w * h, cam, det), _abi.SF_EINVAL)
        _refused(f, lambda: surf(p, p, 2, w, h, w, w * h, cam, _abi.detector_params(0)), _abi.SF_ERANGE, "max_features")
        _refused(f, lambda: surf(p, p, 2, w, h, w, w * h, cam, _abi.detector_params(40000)), _abi.SF_ERANGE)
        _refused(f, lambda: surf(p, p, 2, w, h, w, w * h, cam, det, _abi.stereo_flow_params(win_width=2)), _abi.SF_EINVAL, "flow")
        # the image is a grid dimension
        _refused(f, lambda: surf(p, p, 65536, w, h, w, w * h, cam, det), _abi.SF_ERANGE, "65535")
        # what the detector refuses of an image's size (nothing is read: the call ends before its first launch)
        _refused(f, lambda: surf(p, p, 2, 4096, 4096, 4096, 4096 * 4096, _cam(4096, 4096), det), _abi.SF_ERANGE, "integral")
        # a ROI and a grid stay refused under type 0
        f.front_set_params(_abi.front_params((0.1, 0.0, 0.0, 0.0), 3, 0, 0.02))
        _refused(f, lambda: surf(p, p, 2, w, h, w, w * h, cam, det), _abi.SF_EINVAL, "RoiRatios")
        f.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), 3, 0, 0.02))
        f.grid_set_params(_abi.grid_params(2, 2))
        _refused(f, lambda: surf(p, p, 2, w, h, w, w * h, cam, det), _abi.SF_EINVAL, "Grid")
        f.grid_set_params(_abi.grid_params(1, 1))
        # the diagnostics' own ranges
        _refused(f, lambda: f.debug_surf_limits(-1, 0), _abi.SF_EINVAL)
        _refused(f, lambda: f.debug_surf_limits(0, 65536), _abi.SF_EINVAL)
        # n = 0: SF_OK with the first slot, nothing else; the status of a handle that has run no batch is 0
        before = _state(f)
        assert surf(None, None, 0, w, h, w, w * h, cam, det) == f.store_size() and _state(f) == before
        assert f.surf_batch_status() == 0
        # ... and after all that the call works
        first, got = run_batch(f, torch, [(np.full((h, w), 77, np.uint8),) * 2] * 2, w, h, w, w * h, cam, det)
        assert first == before[2] and f.store_size() == before[2] + 2 and all(len(g[0]) == 0 for g in got)
    finally:
        f.close()


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_of_batch_keyframes(estimation_type):
    """Two keyframes written by ONE batch call, verified against each other with both estimators: the sf_result bytes of the
    same two keyframes written by two single calls (tests/test_gpu_surf.py pins those to the oracle)."""
    import torch
    h, w = 240, 320
    wide_l, wide_r, _ = ec.make_stereo_pair(700, width=w + 8, height=h, max_disp=40.0)
    views = [(np.ascontiguousarray(wide_l[:, o:o + w]), np.ascontiguousarray(wide_r[:, o:o + w])) for o in (0, 8)]
    cam, det = _cam(w, h), _abi.detector_params(400)
    f = _finder(64, estimation_type=estimation_type)
    try:
        f.set_feature_type_surf(_abi.surf_params(hessian_threshold=200.0))
        s = [f.get_features_and_descriptor(l, r, cam, det) for l, r in views]
        first, got = run_batch(f, torch, views, w, h, w, w * h, cam, det)
        assert_batch_equals(got, s, 64)
        assert all(len(g[0]) > 100 for g in got)
        single = f.verify_pairs([s[0][3], s[1][3], s[0][3]], [s[1][3], s[0][3], s[0][3]])
        batch = f.verify_pairs([first, first + 1, first], [first + 1, first, first])
        assert single[2]["success"] == 1 and single[2]["inliers"] > 20      # a keyframe against itself
        assert batch.tobytes() == single.tobytes()
    finally:
        f.close()
