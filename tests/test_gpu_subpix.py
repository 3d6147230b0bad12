"""GPU: sub-pixel corner refinement and Vis/RoiRatios around every detector (csrc/k_subpix.hip, sf_front_params) through
the C-ABI, byte for byte: sf_corner_subpix_device against the NumPy restatement tests/subpix_ref.py; the host handler
and the batch forms with refinement and / or a ROI against the explicit chain sf_detect_*_device -> restatement ->
sf_stereo_correspondences_device -> sf_extract_keyframe_device (calls that existing tests pin); the defaults; and a pair
of refined keyframes through the verification path against the oracle."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from tests import extract_cases as ec
from tests import fast_ref
from tests import subpix_ref as ref
from tests.test_gpu_image import RGB8, _finder, _weights, colourise
from tests.test_gpu_orb import assert_result_parity, assert_same
from tests.test_gpu_orb2 import _pair, _params
from tests.test_gpu_orb2_batch import SENTINEL, _cam, _self_pairs, batch_pairs, run_batch
from tests.test_subpix_host import leaving_case

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
W, H = 202, 170
REFINE = (3, 5, 0.02)
ROI_RATIOS = (0.13, 0.2, 0.1, 0.15)


@pytest.fixture()
def finder():
    import torch
    f = lib.SeparatorFinder(_params(w=W, h=H), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    yield f
    f.close()


def _dev_image(torch, image):
    """A host image (any row stride) on the device as it lies in memory: (tensor, width, height, pitch)."""
    h, w = image.shape
    pitch = image.strides[0]
    base = np.lib.stride_tricks.as_strided(image, shape=(h, pitch), strides=(pitch, 1)) if pitch != w else image
    return torch.from_numpy(np.ascontiguousarray(base)).to(torch.device("cuda:0")), w, h, pitch


def records(points, seed=5):
    """Keypoint records at `points` whose 20 other bytes are noise of their own."""
    rng = np.random.default_rng(seed)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    raw = rng.integers(0, 256, size=(len(pts), 28), dtype=np.uint8)
    kp = np.frombuffer(raw.tobytes(), dtype=KP).copy()
    kp["x"], kp["y"] = pts[:, 0], pts[:, 1]
    return kp


def run_subpix(f, torch, image, kp, win, iterations, eps, n=None):
    """sf_corner_subpix_device on the first n of `kp`; one guard record of 0xEE behind the buffer.  Returns all records."""
    d_img, w, h, pitch = _dev_image(torch, image)
    n = len(kp) if n is None else n
    buf = np.full((len(kp) + 1, 28), 0xEE, np.uint8)
    buf[:len(kp)] = np.frombuffer(kp.tobytes(), np.uint8).reshape(-1, 28)
    d_kp = torch.from_numpy(buf.copy()).to(torch.device("cuda:0"))
    try:
        f.corner_subpix_device(d_img.data_ptr(), w, h, pitch, d_kp.data_ptr(), n, win, iterations, eps)
    finally:
        torch.cuda.synchronize()
        raw = d_kp.cpu().numpy()
        assert raw[n:].tobytes() == buf[n:].tobytes()            # nothing written behind n, the guard included
    return np.frombuffer(raw[:len(kp)].tobytes(), dtype=KP)


def restated(image, kp, win, iterations, eps):
    xy, info = ref.corner_subpix(image, np.stack([kp["x"], kp["y"]], axis=1), win, iterations, eps)
    want = kp.copy()
    want["x"], want["y"] = xy[:, 0], xy[:, 1]
    return want, info


@functools.lru_cache(maxsize=None)
def _image(name):
    if name == "stereo3":
        return ec.make_stereo_pair(3)[0]                     # 752 x 480, pitch 760: pitch != width
    if name == "small":
        return np.ascontiguousarray(_pair(W, H, 1)[0])
    if name == "constant":
        return np.full((40, 50), 93, np.uint8)
    if name == "leaving":
        return leaving_case()[0]
    raise KeyError(name)


def _near(limit):
    lo = [0.0, 0.5, 1.25, 2.0, 3.5, 4.0]
    return lo + [limit - 1 - v for v in lo]


@functools.lru_cache(maxsize=None)
def _points(name):
    if name == "fast300":                                    # the first 300 FAST corners of the 752 x 480 image, raster order
        kp = fast_ref.detect(_image("stereo3"), 20, 1, 0)[:300]
        return records(np.stack([kp["x"], kp["y"]], axis=1))
    if name == "random":
        rng = np.random.default_rng(11)
        return records(np.stack([rng.uniform(0, W - 1, 200), rng.uniform(0, H - 1, 200)], axis=1))
    if name == "edges":                                      # within win + 1 of each edge and of each image corner
        xe, ye, xm, ym = _near(W), _near(H), [40.3, 101.0, 160.7], [33.3, 85.0, 120.7]
        pts = [(x, y) for x in xe for y in ym] + [(x, y) for x in xm for y in ye] + [(x, y) for x in xe for y in ye]
        return records(pts)
    if name == "constant":
        return records([(20.0, 20.0), (3.5, 7.25), (49.0, 39.0)])
    if name == "leaving":
        return records(leaving_case()[1])
    raise KeyError(name)


# name: (image, points, win, iterations, eps)
CASES = {
    "fast300 3 1": ("stereo3", "fast300", 3, 1, 0.02),
    "fast300 3 5": ("stereo3", "fast300", 3, 5, 0.02),
    "fast300 3 30": ("stereo3", "fast300", 3, 30, 0.02),
    "fast300 3 30 eps 0": ("stereo3", "fast300", 3, 30, 0.0),
    "fast300 1 10": ("stereo3", "fast300", 1, 10, 0.02),
    "fast300 5 10": ("stereo3", "fast300", 5, 10, 0.02),
    "fast300 15 3": ("stereo3", "fast300", 15, 3, 0.02),
    "random starts": ("small", "random", 3, 10, 0.02),
    "edges and corners": ("small", "edges", 3, 10, 0.02),
    "edges and corners win 5": ("small", "edges", 5, 4, 0.02),
    "constant image": ("constant", "constant", 3, 30, 0.02),
    "leaving corner": ("leaving", "leaving", 3, 30, 0.02),
}


@functools.lru_cache(maxsize=None)
def _reference(case):
    image, points, win, it, eps = CASES[case]
    return restated(_image(image), _points(points), win, it, eps)


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_restatement(finder, case):
    import torch
    image, points, win, it, eps = CASES[case]
    want, info = _reference(case)
    kp = _points(points)
    got = run_subpix(finder, torch, _image(image), kp, win, it, eps)
    moved = ((want["x"] != kp["x"]) | (want["y"] != kp["y"])).sum()
    diff = np.flatnonzero((got["x"] != want["x"]) | (got["y"] != want["y"]))
    print("%s: %d corners, %d moved; stops %s, reverted %d; %d differ from the restatement%s" % (
        case, len(kp), moved, {ref.STOP_NAMES[s]: int((info["stop"] == s).sum()) for s in range(4)}, info["reverted"].sum(),
        len(diff), "" if not len(diff) else " (first: %d got (%r, %r) want (%r, %r))" % (
            diff[0], got["x"][diff[0]], got["y"][diff[0]], want["x"][diff[0]], want["y"][diff[0]])))
    assert got.tobytes() == want.tobytes()                   # x, y equal; the 20 other bytes of each record unchanged


def test_cases_reach_every_branch():
    stops = {c: _reference(c)[1] for c in CASES}
    for c in ("fast300 3 5", "fast300 3 30"):
        i = stops[c]
        assert (i["stop"] == ref.STOP_EPS).any() and (i["stop"] == ref.STOP_CAP).any() and i["reverted"].any(), c
    assert (stops["constant image"]["stop"] == ref.STOP_DET).all()
    assert (stops["leaving corner"]["stop"] == ref.STOP_LEFT).all()
    assert (stops["fast300 3 1"]["iterations"] == 1).all()
    e = _reference("edges and corners")
    assert ((e[0]["x"] != _points("edges")["x"]) | (e[0]["y"] != _points("edges")["y"])).sum() > 20


def test_n_zero_prefix_and_repeat(finder):
    import torch
    img, kp = _image("small"), _points("random")
    assert run_subpix(finder, torch, img, kp, 3, 10, 0.02, n=0).tobytes() == kp.tobytes()
    d_img = _dev_image(torch, img)[0]
    finder.corner_subpix_device(d_img.data_ptr(), W, H, W, None, 0, 3, 10, 0.02)           # n = 0 needs no records at all
    part = run_subpix(finder, torch, img, kp, 3, 10, 0.02, n=37)
    want = _reference("random starts")[0]
    assert part[:37].tobytes() == want[:37].tobytes() and part[37:].tobytes() == kp[37:].tobytes()
    a = run_subpix(finder, torch, img, kp, 3, 10, 0.02)
    b = run_subpix(finder, torch, img, kp, 3, 10, 0.02)
    assert a.tobytes() == b.tobytes() == want.tobytes()


def test_refusals_leave_the_buffer(finder):
    import torch
    kp = records([(5.0, 5.0), (4.5, 6.0)])
    tiny = np.random.default_rng(2).integers(0, 256, size=(10, 10), dtype=np.uint8)
    for image, win, it in ((tiny, 3, 5), (_image("small"), 0, 5), (_image("small"), 16, 5), (_image("small"), 3, 0),
                           (_image("small"), -1, 5), (_image("small"), 3, -2)):
        d_img, w, h, pitch = _dev_image(torch, image)
        d_kp = torch.from_numpy(np.frombuffer(kp.tobytes(), np.uint8).copy()).to(torch.device("cuda:0"))
        with pytest.raises(lib.SepfinderError) as e:
            finder.corner_subpix_device(d_img.data_ptr(), w, h, pitch, d_kp.data_ptr(), 2, win, it, 0.02)
        assert e.value.code == _abi.SF_EINVAL
        torch.cuda.synchronize()
        assert d_kp.cpu().numpy().tobytes() == kp.tobytes()          # the buffer is untouched
    ok = np.random.default_rng(2).integers(0, 256, size=(11, 11), dtype=np.uint8)   # 2 win + 5: the smallest image accepted
    got = run_subpix(finder, torch, ok, kp, 3, 5, 0.02)
    assert got.tobytes() == restated(ok, kp, 3, 5, 0.02)[0].tobytes()


# ---- the extraction calls ----------------------------------------------------------------------------------------------
def _set_type(f, ftype):
    if ftype == 2:
        f.set_feature_type_orb()
    else:
        f.set_feature_type(ftype)


def _detect(f, torch, image, ftype, det):
    """The explicit detector call of a feature type on a contiguous host image: KEYPOINT_DTYPE records."""
    d_img, w, h, pitch = _dev_image(torch, np.ascontiguousarray(image))
    maxf = det.max_features
    d_kp = torch.zeros((maxf, 28), dtype=torch.uint8, device=d_img.device)
    if ftype == 4:
        n = f.detect_fast_device(d_img.data_ptr(), w, h, pitch, maxf, d_kp.data_ptr(), maxf)
    elif ftype == 2:
        n = f.detect_orb_device(d_img.data_ptr(), w, h, pitch, maxf, d_kp.data_ptr(), maxf)
    else:
        n = f.detect_corners_device(d_img.data_ptr(), w, h, pitch, maxf, det.quality_level, det.min_distance, d_kp.data_ptr(), maxf)
    torch.cuda.synchronize()
    return np.frombuffer(d_kp.cpu().numpy()[:min(n, maxf)].tobytes(), dtype=KP).copy()


def chain(f, torch, left, right, cam, det, ftype, refine, ratios=None):
    """detector on a contiguous copy of the ROI -> offset and restatement -> sf_stereo_correspondences_device ->
    sf_extract_keyframe_device.  Returns ((desc, xyz, kpts), slot, the keypoints before refinement)."""
    dev = torch.device("cuda:0")
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    x, y, rw, rh = ref.compute_roi(w, h, ratios) if ratios else (0, 0, w, h)
    found = _detect(f, torch, left[y:y + rh, x:x + rw], ftype, det)
    before = ref.refine_keypoints(left, found, 0, 0, 0.0, (x, y))
    win, it, eps = refine if refine else (0, 0, 0.0)
    kp = ref.refine_keypoints(left, found, win, it, eps, (x, y))
    n, nb = len(kp), f.descriptor_bytes()
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_kp = torch.from_numpy(np.frombuffer(kp.tobytes(), np.uint8).copy()).to(dev)
    d_xy = torch.zeros((max(n, 1), 2), dtype=torch.float32, device=dev)
    d_rx = torch.zeros((max(n, 1),), dtype=torch.float32, device=dev)
    d_st = torch.zeros((max(n, 1),), dtype=torch.uint8, device=dev)
    f.stereo_correspondences_device(d_l.data_ptr(), d_r.data_ptr(), w, h, w, d_kp.data_ptr(), n, d_xy.data_ptr(),
                                    d_st.data_ptr(), d_rx.data_ptr())
    desc = torch.zeros((max(n, 1), nb), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    kpo = torch.zeros((max(n, 1), 28), dtype=torch.uint8, device=dev)
    slot, rows = f.extract_keyframe_device(d_l.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), n, cam,
                                           desc.data_ptr(), xyz.data_ptr(), kpo.data_ptr())
    torch.cuda.synchronize()
    out = (desc.cpu().numpy()[:rows], xyz.cpu().numpy()[:rows], np.frombuffer(kpo.cpu().numpy()[:rows].tobytes(), dtype=KP))
    return out, slot, before


def _fractional(kp):
    return (kp["x"] != np.floor(kp["x"])) | (kp["y"] != np.floor(kp["y"]))


@pytest.mark.parametrize("ftype", [6, 8, 4, 2])
def test_host_handler_with_refinement(finder, ftype):
    import torch
    left, right = batch_pairs(W, H)[0]
    cam, det = _cam(W, H), _abi.detector_params(300)
    _set_type(finder, ftype)
    want, _, before = chain(finder, torch, left, right, cam, det, ftype, REFINE)
    plain, _, _ = chain(finder, torch, left, right, cam, det, ftype, None)
    finder.front_set_params(_abi.front_params(subpix_iterations=REFINE[1]))
    assert bytes(finder.front_get_params()) == bytes(_abi.front_params((0, 0, 0, 0), *REFINE))
    d, p, k, slot = finder.get_features_and_descriptor(left, right, cam, det)
    frac = _fractional(k)
    print("type %d with refinement %s: %d keypoints found, %d rows (%d without refinement), %d fractional, octaves %s" % (
        ftype, REFINE, len(before), len(d), len(plain[0]), frac.sum(), np.unique(k["octave"]).tolist()))
    assert_same((d, p, k), want)
    assert len(d) > 50 and frac.sum() * 4 >= len(k)                       # not vacuous
    assert finder.store_size() == slot + 1
    if ftype == 2:
        assert (frac & (k["octave"] > 0)).any()                              # refinement of level-0 positions of higher octaves
    else:
        assert not _fractional(before).any()                                 # GFTT and FAST corners are integers
    assert k.tobytes() != plain[2].tobytes()


def test_host_handler_u8_with_refinement(finder):
    import torch
    left, right = batch_pairs(W, H)[0]
    cam, det = _cam(W, H), _abi.detector_params(300)
    finder.set_feature_type(4)
    finder.front_set_params(_abi.front_params(subpix_iterations=REFINE[1]))
    mono = finder.get_features_and_descriptor(left, right, cam, det)
    u8 = finder.get_features_and_descriptor_u8(left, right, _abi.SF_IMAGE_MONO8, cam, det)
    assert len(mono[0]) > 50 and _fractional(mono[2]).any()
    assert_same(u8[:3], mono[:3])


def _three_pairs():
    p = batch_pairs(W, H)
    return [p[0], p[2], p[1]]                                                # a constant pair in the middle


@pytest.mark.parametrize("ftype", [6, 4, 2])
def test_batch_forms_with_refinement(finder, ftype):
    import torch
    cam, det = _cam(W, H), _abi.detector_params(200)
    pairs = _three_pairs()
    _set_type(finder, ftype)
    finder.front_set_params(_abi.front_params(subpix_iterations=REFINE[1]))
    call = finder.get_features_and_descriptor_orb_batch_device if ftype == 2 else finder.get_features_and_descriptor_batch_device
    singles = [finder.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
    assert len(singles[0][0]) > 50 and _fractional(singles[0][2]).any() and len(singles[1][0]) == 0 and len(singles[2][0]) > 5
    before = finder.store_size()
    first, got = run_batch(finder, torch, pairs, W, H, W + 6, (W + 6) * H + 32, cam, det, call=call)
    assert first == before and finder.store_size() == before + 3
    for i, s in enumerate(singles):
        assert_same(got[i], s[:3])
    assert _self_pairs(finder, range(first, first + 3)) == _self_pairs(finder, [s[3] for s in singles])
    state = (finder.store_size(), bytes(finder.front_get_params()))
    assert call(0, 0, 0, W, H, W, W * H, cam, det) == state[0]              # n_keyframes = 0 leaves everything as it was
    assert (finder.store_size(), bytes(finder.front_get_params())) == state


def test_u8_batch_with_refinement():
    import torch
    dev = torch.device("cuda:0")
    cam, det, maxf = _cam(W, H), _abi.detector_params(200), 200
    gray = _three_pairs()
    pairs = [(colourise(l, 10 + i, RGB8), colourise(r, 20 + i, RGB8)) for i, (l, r) in enumerate(gray)]
    flat = np.empty((H, W, 3), np.uint8)
    flat[...] = (120, 77, 30)                                                # (colourise adds noise: the constant pair is made here)
    pairs[1] = (flat, flat)
    pitch, stride = 3 * W + 5, (3 * W + 5) * H + 64

    def packed(images):
        buf = np.full((len(images), stride), 0xA5, np.uint8)
        for i, c in enumerate(images):
            np.lib.stride_tricks.as_strided(buf[i], shape=(H, W, 3), strides=(pitch, 3, 1))[...] = c
        return torch.from_numpy(buf).to(dev)

    d_l, d_r = packed([p[0] for p in pairs]), packed([p[1] for p in pairs])
    f = _finder(torch, w=W, h=H, dims=128)
    try:
        f.netvlad_load(_weights())
        f.front_set_params(_abi.front_params(subpix_iterations=REFINE[1]))
        singles = [f.get_features_and_descriptor_u8(l, r, RGB8, cam, det) for l, r in pairs]
        assert len(singles[0][0]) > 50 and _fractional(singles[0][2]).any() and len(singles[1][0]) == 0
        rows = torch.full((3,), -7, dtype=torch.int32, device=dev)
        desc = torch.full((3 * maxf, 32), SENTINEL, dtype=torch.uint8, device=dev)
        xyz = torch.full((3 * maxf, 12), SENTINEL, dtype=torch.uint8, device=dev)
        kp = torch.full((3 * maxf, 28), SENTINEL, dtype=torch.uint8, device=dev)
        first, row = f.add_keyframes_u8_batch_device(d_l.data_ptr(), d_r.data_ptr(), None, RGB8, 3, W, H, pitch, stride, cam, det,
                                                     None, rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
        torch.cuda.synchronize()
        assert (first, row) == (3, 0) and f.store_size() == 6 and f.nn_sizes() == (3, 0)
        rows, desc, xyz, kp = (t.cpu().numpy() for t in (rows, desc, xyz, kp))
        for i, (d0, p0, k0, _) in enumerate(singles):
            r = int(rows[i])
            blk = slice(i * maxf, i * maxf + r)
            assert r == len(d0), i
            assert_same((desc[blk], np.frombuffer(xyz[blk].tobytes(), np.float32).reshape(r, 3),
                         np.frombuffer(kp[blk].tobytes(), dtype=KP)), (d0, p0, k0))
            assert (kp[i * maxf + r:(i + 1) * maxf] == SENTINEL).all()
        assert _self_pairs(f, range(3, 6)) == _self_pairs(f, [s[3] for s in singles])
    finally:
        f.close()


# (width, ratios): the issue's ratios on 202 x 170 give the ROI (26, 17, 135, 127); on 208 x 170 roi.x = 27 is odd while
# the pitch stays a multiple of 4: the sub-image starts off a dword boundary on an image whose rows would allow dword loads
ROI_SHAPES = {"202": (W, ROI_RATIOS), "208 odd x": (208, ROI_RATIOS)}


@pytest.mark.parametrize("refine", [None, REFINE], ids=["roi alone", "roi and refinement"])
@pytest.mark.parametrize("ftype", [6, 8, 4])
@pytest.mark.parametrize("shape", list(ROI_SHAPES))
def test_roi_single_and_batch(finder, shape, ftype, refine):
    import torch
    w, ratios = ROI_SHAPES[shape]
    cam, det = _cam(w, H), _abi.detector_params(200)
    pairs = [batch_pairs(w, H)[i] for i in (0, 2, 1)]
    roi = ref.compute_roi(w, H, ratios)
    assert finder.compute_roi(w, H, ratios) == roi and (w != W or roi == (26, 17, 135, 127)) and (w != 208 or roi[0] == 27)
    x, y, rw, rh = roi
    _set_type(finder, ftype)
    want = [chain(finder, torch, l, r, cam, det, ftype, refine, ratios) for l, r in pairs]
    whole, _, _ = chain(finder, torch, *pairs[0], cam, det, ftype, refine)
    finder.front_set_params(_abi.front_params(ratios, refine[0] if refine else 3, refine[1] if refine else 0, 0.02))
    singles = [finder.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
    print("ROI %s of %d x %d, type %d, refinement %s: rows %s (whole image %d)" % (
        roi, w, H, ftype, refine, [len(s[0]) for s in singles], len(whole[0])))
    for s, (wnt, _, before) in zip(singles, want):
        assert_same(s[:3], wnt)
        assert ((before["x"] >= x) & (before["x"] < x + rw) & (before["y"] >= y) & (before["y"] < y + rh)).all()
    assert len(singles[0][0]) > 20 and len(singles[1][0]) == 0 and singles[0][2].tobytes() != whole[2].tobytes()
    if not refine:
        k = singles[0][2]
        assert ((k["x"] >= x) & (k["x"] < x + rw) & (k["y"] >= y) & (k["y"] < y + rh)).all() and not _fractional(k).any()
    first, got = run_batch(finder, torch, pairs, w, H, w, w * H, cam, det, call=finder.get_features_and_descriptor_batch_device)
    for i, s in enumerate(singles):
        assert_same(got[i], s[:3])
    assert _self_pairs(finder, range(first, first + 3)) == _self_pairs(finder, [s[3] for s in singles])


def test_roi_refusals(finder):
    import torch
    cam, det = _cam(W, H), _abi.detector_params(200)
    left, right = batch_pairs(W, H)[0]
    d_l, d_r = torch.from_numpy(left).to("cuda:0"), torch.from_numpy(right).to("cuda:0")
    finder.set_feature_type_orb()
    finder.front_set_params(_abi.front_params(ROI_RATIOS))                   # accepted: the handle's type may change later
    state = lambda: (finder.store_size(), finder.get_feature_type()[0], bytes(finder.get_feature_type()[1]),  # noqa: E731
                     bytes(finder.get_orb_detector()), bytes(finder.front_get_params()))
    before = state()
    calls = (lambda: finder.get_features_and_descriptor(left, right, cam, det),
             lambda: finder.get_features_and_descriptor_u8(left, right, _abi.SF_IMAGE_MONO8, cam, det),
             lambda: finder.get_features_and_descriptor_orb_batch_device(d_l.data_ptr(), d_r.data_ptr(), 1, W, H, W, W * H, cam, det))
    for call in calls:
        with pytest.raises(lib.SepfinderError) as e:
            call()
        assert e.value.code == _abi.SF_EINVAL and "RoiRatios" in str(e.value) and "not built" in str(e.value)
        assert state() == before
    for one in ((0.1, 0, 0, 0), (0, 0, 0, 0.5)):                              # any ratio != 0
        finder.front_set_params(_abi.front_params(one))
        with pytest.raises(lib.SepfinderError) as e:
            calls[0]()
        assert e.value.code == _abi.SF_EINVAL
    finder.front_set_params(_abi.front_params())
    assert len(calls[0]()[0]) > 50                                            # no ROI: type 2 runs
    # a ROI of 2 x 2
    finder.set_feature_type(6)
    tiny = np.zeros((5, 5), np.uint8)
    finder.front_set_params(_abi.front_params((0.3, 0.3, 0.3, 0.3)))
    size = finder.store_size()
    with pytest.raises(lib.SepfinderError) as e:
        finder.get_features_and_descriptor(tiny, tiny, _cam(5, 5), det)
    assert e.value.code == _abi.SF_EINVAL and "2 x 2" in str(e.value) and finder.store_size() == size
    with pytest.raises(lib.SepfinderError) as e:
        finder.compute_roi(5, 5, (0.3, 0.3, 0.3, 0.3))
    assert e.value.code == _abi.SF_EINVAL
    # refinement needs 2 win + 5 pixels a side
    finder.front_set_params(_abi.front_params(subpix_win_size=3, subpix_iterations=5))
    ten = np.zeros((10, 10), np.uint8)
    with pytest.raises(lib.SepfinderError) as e:
        finder.get_features_and_descriptor(ten, ten, _cam(10, 10), det)
    assert e.value.code == _abi.SF_EINVAL and finder.store_size() == size


def test_defaults(finder):
    left, right = batch_pairs(W, H)[0]
    cam, det = _cam(W, H), _abi.detector_params(200)
    default = _abi.front_params()
    filled = _abi.FrontParams()
    lib.load().sf_front_defaults(filled)
    assert bytes(filled) == bytes(default) == bytes(finder.front_get_params())           # a fresh handle: both steps off
    fresh = finder.get_features_and_descriptor(left, right, cam, det)
    finder.front_set_params(_abi.front_params(ROI_RATIOS, 3, 5, 0.02))
    changed = finder.get_features_and_descriptor(left, right, cam, det)
    assert changed[2].tobytes() != fresh[2].tobytes()
    finder.front_set_params(default)
    assert_same(finder.get_features_and_descriptor(left, right, cam, det)[:3], fresh[:3])
    # iterations 0 or window 0: no refinement, whatever the other says (upstream's condition)
    for p in (_abi.front_params(subpix_win_size=0, subpix_iterations=9), _abi.front_params(subpix_win_size=7, subpix_iterations=0)):
        finder.front_set_params(p)
        assert_same(finder.get_features_and_descriptor(left, right, cam, det)[:3], fresh[:3])
    good = _abi.front_params((0.1, 0.0, 0.2, 0.0), 5, 7, 0.5)
    finder.front_set_params(good)
    for bad in (_abi.front_params((1.5, 0, 0, 0)), _abi.front_params((0, -0.1, 0, 0)), _abi.front_params((0, 0, float("nan"), 0)),
                _abi.front_params(subpix_win_size=-1), _abi.front_params(subpix_win_size=16),
                _abi.front_params(subpix_iterations=-1), _abi.front_params(subpix_eps=float("nan"))):
        with pytest.raises(lib.SepfinderError) as e:
            finder.front_set_params(bad)
        assert e.value.code == _abi.SF_EINVAL
        assert bytes(finder.front_get_params()) == bytes(good)                             # a refused call changes nothing


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_of_refined_keyframes(estimation_type):
    """Two keyframes of one scene, the second pair's disparity field shifted (max_disp 40 -> 37), both refined; the oracle
    runs on the downloaded features."""
    import torch
    from oracle import pyoracle
    h, w = 240, 320
    p = _params(w=w, h=h, estimation_type=estimation_type)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11, local_transform=synth.LOCAL_TRANSFORM)
    det = _abi.detector_params(400)
    with lib.SeparatorFinder(p, device=0) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        f.front_set_params(_abi.front_params(subpix_iterations=REFINE[1]))
        a = f.get_features_and_descriptor(*_pair(w, h, 1, 40.0), cam, det)
        b = f.get_features_and_descriptor(*_pair(w, h, 1, 37.0), cam, det)
        assert _fractional(a[2]).sum() > 50 and _fractional(b[2]).sum() > 50
        res = f.verify_pairs([a[3]], [b[3]])
        o = pyoracle.estimate_transform(f.params, _abi.FeatureArrays(*a[:3]), _abi.FeatureArrays(*b[:3]))
        print("estimator %d: success gpu %d oracle %d, inliers %d / %d, matches %d / %d" % (
            estimation_type, res[0]["success"], o["success"], res[0]["inliers"], o["inliers"], res[0]["matches"], o["matches"]))
        assert_result_parity(res[0], o, "estimator %d" % estimation_type)
        assert res[0]["success"] == 1 and res[0]["inliers"] > 20
