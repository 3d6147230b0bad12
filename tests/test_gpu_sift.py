"""GPU: SIFT (Vis/FeatureType 1; csrc/k_sift.hip) against the NumPy restatement tests/sift_ref.py, byte for byte -- planes
of the int16 pyramids through sf_debug_sift_plane, the detector with all seven keypoint fields in order under the cuts of
n_features and max_features, then float32 rows on given keypoints with the 3D points and their NaNs in place -- then the
full extraction calls against the explicit chain detector -> refinement -> stereo correspondence -> extraction, the
refusals, and two SIFT keyframes through the verification path against the oracle.  Every test fails without the feature:
the symbols it calls are new."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from tests import orb2_ref
from tests import sift_ref as ref
from tests.test_gpu_surf import _image_up, texture

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
PARAM_SETS = {
    "defaults": {},
    "contrast 0.01": dict(contrast_threshold=0.01),
    "1 layer": dict(n_octave_layers=1),
    "5 layers": dict(n_octave_layers=5),
    "edge 3": dict(edge_threshold=3.0),
    "sigma 1.2": dict(sigma=1.2),
    "40 features": dict(n_features=40),
}
SMALL = ["64x48", "97x61", "160x120 padded"]


@pytest.fixture()
def finder():
    import torch
    f = lib.SeparatorFinder(synth.camera_params(), device=0)          # a binary (desc_type 0) handle: the detector runs on any
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def detected(name, pset):
    """The restatement's keypoints of an image under a parameter set before any cut, and its pyramids: computed once."""
    kw = dict(PARAM_SETS[pset])
    kw.pop("n_features", None)
    trace = {}
    kp = ref.detect(texture(name), ref.Params(**kw), 0, trace)
    kp.setflags(write=False)
    return kp, trace["gauss"], trace["dog"]


def run_detect(f, torch, image, max_features, cap, prm=None):
    dev = torch.device("cuda:0")
    h, w = image.shape
    d_img, pitch = _image_up(torch, image, dev)
    out = torch.full((max(cap, 1), 28), 0xEE, dtype=torch.uint8, device=dev)
    n = f.detect_sift(d_img.data_ptr(), w, h, pitch, max_features, out.data_ptr(), cap, prm)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[min(n, cap):] == 0xEE).all()                                    # nothing behind the result is touched
    return n, np.frombuffer(raw[:min(n, cap)].tobytes(), dtype=KP)


def plane_of(f, torch, octave, layer, dog, w, h):
    out = torch.full((h * w + 8,), 0x5A5A, dtype=torch.int16, device="cuda:0")
    f.debug_sift_plane(octave, layer, dog, out.data_ptr())
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[h * w:] == 0x5A5A).all()
    return a[:h * w].reshape(h, w)


@pytest.mark.parametrize("name", SMALL)
def test_planes_equal_restatement(finder, name):
    """The base, the last Gaussian plane and one difference plane of octaves 0, 1 and the top: 64 x 48, 97 x 61 (odd sides
    through the enlargement and every halving, the top octave 6 x 3: the kernels reflect repeatedly), 160 x 120 with pitch 173."""
    import torch
    image = texture(name)
    _, gauss, dog = detected(name, "defaults")
    n_oct, sizes = ref.plan(image.shape[1], image.shape[0])
    assert len(gauss) == n_oct and lib.sift_plan(image.shape[1], image.shape[0])[:2] == (n_oct, sizes)
    run_detect(finder, torch, image, 0, 4, None)
    n = 3
    for o in (0, 1, n_oct - 1):
        w, h = sizes[o]
        for layer, is_dog in ((0, 0), (n + 2, 0), (2, 1)):
            got = plane_of(finder, torch, o, layer, is_dog, w, h)
            want = (dog if is_dog else gauss)[o][layer]
            bad = np.argwhere(got != want)
            assert not len(bad), "octave %d %s plane %d: %d samples differ, first at %s: %d != %d" % (
                o, "DoG" if is_dog else "Gaussian", layer, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    with pytest.raises(lib.SepfinderError):
        finder.debug_sift_plane(n_oct, 0, 0, 0)
    with pytest.raises(lib.SepfinderError):
        finder.debug_sift_plane(0, n + 2, 1, 0)


@pytest.mark.parametrize("name,pset", [(i, p) for i in SMALL for p in PARAM_SETS] + [("320x240", "defaults")])
def test_detector_equals_restatement(finder, name, pset):
    """All seven fields of every keypoint, in order, for max_features 0, 1, 50 and n - 1 (the cut reorders equal responses),
    and a cap below the result.  The images at least 160 wide repeat their left half: exact ties."""
    import torch
    image = texture(name)
    all_kp = detected(name, pset)[0]
    N = len(all_kp)
    prm = ref.Params(**PARAM_SETS[pset])
    cprm = _abi.sift_params(**PARAM_SETS[pset])
    print("%s, %s: %d keypoints, octave bytes %s, sizes %s .. %s, %d equal responses" % (
        name, pset, N, sorted(set((all_kp["octave"] & 255).tolist())), all_kp["size"].min() if N else None,
        all_kp["size"].max() if N else None, N - len(np.unique(all_kp["response"]))))
    assert N >= 3
    if image.shape[1] >= 160:
        assert N - len(np.unique(all_kp["response"])) > 10
    for maxf in (0, 1, 50, N - 1):
        want = orb2_ref.limit_keypoints(all_kp, ref.cut_of(prm, maxf))
        n, got = run_detect(finder, torch, image, maxf, max(N, 1), cprm)
        assert n == len(want), (maxf, n, len(want))
        assert got.tobytes() == want.tobytes(), (maxf, np.argwhere(got != want)[:3])
    want = orb2_ref.limit_keypoints(all_kp, ref.cut_of(prm, 0))
    n, got = run_detect(finder, torch, image, 0, len(want) // 3, cprm)          # cap < result: the count is still the result's
    assert n == len(want) and got.tobytes() == want[:len(want) // 3].tobytes()
    assert (all_kp["class_id"] == -1).all() and (np.diff(all_kp["response"]) <= 0).all()
    assert ((all_kp["angle"] >= 0) & (all_kp["angle"] < 360)).all()


def test_constant_image_limits_and_small_images(finder):
    """A constant image has no extrema; a capacity below the number of keypoints is SF_ERANGE and writes nothing; an image
    whose enlarged side is below 13 gives no keypoint and no error; a side below 3 is refused."""
    import torch
    flat = np.full((48, 64), 77, np.uint8)
    n, got = run_detect(finder, torch, flat, 0, 16, _abi.sift_params(contrast_threshold=0.0))
    assert n == 0 and len(got) == 0
    assert len(ref.detect(flat, ref.Params(contrast_threshold=0.0))) == 0
    image = texture("97x61")
    want = detected("97x61", "defaults")[0]
    assert len(want) > 8
    finder.debug_sift_limits(8)
    with pytest.raises(lib.SepfinderError) as e:
        run_detect(finder, torch, image, 0, len(want), None)
    assert e.value.code == _abi.SF_ERANGE
    dev = torch.device("cuda:0")
    d_img, pitch = _image_up(torch, image, dev)
    out = torch.full((len(want), 28), 0xEE, dtype=torch.uint8, device=dev)
    with pytest.raises(lib.SepfinderError):
        finder.detect_sift(d_img.data_ptr(), image.shape[1], image.shape[0], pitch, 0, out.data_ptr(), len(want), None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xEE).all()
    with pytest.raises(lib.SepfinderError):
        finder.debug_sift_limits(-1)
    finder.debug_sift_limits(0)
    n, got = run_detect(finder, torch, image, 0, len(want), None)
    assert n == len(want) and got.tobytes() == want.tobytes()
    rng = np.random.default_rng(5)
    tiny = rng.integers(0, 256, (6, 5), dtype=np.uint8)                          # enlarged 10 x 12: no sample is 5 pixels inside
    n, got = run_detect(finder, torch, tiny, 0, 4, _abi.sift_params(contrast_threshold=0.0))
    assert n == 0 and len(ref.detect(tiny, ref.Params(contrast_threshold=0.0))) == 0
    with pytest.raises(lib.SepfinderError) as e:
        run_detect(finder, torch, rng.integers(0, 256, (2, 40), dtype=np.uint8), 0, 4, None)
    assert e.value.code == _abi.SF_EINVAL
    assert finder.get_feature_type()[0] == 6


# ---- Vis/FeatureType 1: extraction on given keypoints -----------------------------------------------------------------
from oracle import pyoracle                                                      # noqa: E402
from tests import extract_cases as ec                                            # noqa: E402
from tests import subpix_ref                                                     # noqa: E402
from tests.test_gpu_surf import _device_chain, _finder, _params, assert_result_parity, assert_same, run_extract  # noqa: E402


@pytest.fixture()
def sift_finder():
    f = _finder(128)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def extract_reference(seed, n, depth):
    """extract_cases.make_case at 200 x 150 with the fields SIFT::compute reads drawn anew: octave bytes -1, 0, 1 and the top
    octave, layers 1 and n; angles 0, 90, 359.9 and (the first quarter) the detector's own keypoints; sizes from 1.6 to 400,
    whose window exceeds every plane and is clamped by the diagonal; a sixth of the positions 2 pixels off an edge; and a few
    keypoints that name no plane or carry no angle (dropped)."""
    kw = dict(n=n, **(dict(min_depth=0.8, max_depth=12.0) if depth else {}))
    image, kp, rx, st, cam = ec.make_case(seed, width=200, height=150, **kw)
    h, w = image.shape
    prm = ref.Params()
    n_oct = ref.plan(w, h)[0]
    rng = np.random.default_rng(3000 + seed)
    m = len(kp)
    octave = rng.choice(np.array([-1, 0, 1, n_oct - 2]), m)
    layer = rng.choice(np.array([1, prm.n_octave_layers]), m)
    kp["octave"] = (octave & 255) | (layer << 8)
    kp["angle"] = rng.choice(np.array([0.0, 90.0, 359.9], np.float32), m)
    kp["size"] = rng.choice(np.array([1.6, 3.2, 7.5, 20.0, 60.0], np.float32), m)
    kp["size"][::64] = 400.0

    def move(i, axis, value):
        if rx is not None and axis == "x":
            rx[i] += np.float32(value) - kp["x"][i]                              # the disparity goes along
        kp[axis][i] = value
    for i in np.nonzero(rng.random(m) < 1 / 6)[0]:
        axis, side = ("x", w) if rng.random() < 0.5 else ("y", h)
        move(i, axis, [2.0, side - 3.0][rng.integers(2)])
    own = ref.detect(image, prm)
    for i in range(min(len(own), m // 4)):
        x = own["x"][i]
        move(i, "x", x)
        keep_rx = None if rx is None else rx[i]
        kp[i] = own[i]
        if rx is not None:
            rx[i] = keep_rx
    if m >= 16:
        kp["octave"][m - 1] = ((n_oct - 1) & 255) | (1 << 8)                     # no such octave
        kp["octave"][m - 2] = 0 | ((prm.n_octave_layers + 3) << 8)               # no such layer
        kp["angle"][m - 3] = -1.0
        kp["size"][m - 4] = 0.0
        kp["octave"][m - 5] = (-2 & 255) | (1 << 8)
    want = ref.extract_keyframe(image, kp, rx, st, cam, prm)
    return (image, kp, rx, st, cam), want


@pytest.mark.parametrize("seed,n,depth", [(9, 257, False), (2, 257, True), (6, 0, False), (13, 1, False)])
def test_extraction_equals_restatement(sift_finder, seed, n, depth):
    """Rows, kept keypoints and 3D points with their NaNs in place."""
    import torch
    (image, kp, rx, st, cam), want = extract_reference(seed, n, depth)
    f = sift_finder
    f.set_feature_type_sift()
    assert f.get_feature_type()[0] == 1 and f.descriptor_bytes() == 512
    slot, rows, desc, xyz, kout = run_extract(f, torch, image, kp, rx, st, cam)
    print("seed %d: %d of %d rows, octave bytes %s, sizes %s" % (seed, rows, len(kp), sorted(set((kp["octave"] & 255).tolist())),
                                                                   sorted(set(kp["size"].tolist()))[:8]))
    assert rows == len(want[0])
    assert_same((desc.reshape(rows, 128), xyz, kout), want, 128)
    assert f.store_size() == slot + 1
    if n >= 257:
        assert 0 < rows < n
        if not depth:
            assert rows == n - 5                                                 # exactly the five that name no plane, angle or size
            assert (want[2]["size"] == 400.0).any() and {255, 0, 1, 5} <= set((want[2]["octave"] & 255).tolist())
        d, top = want[0], (want[2]["octave"] & 255) == 5
        assert (d == np.rint(d)).all() and d.min() >= 0 and d.max() <= 255
        assert (d[~top].max(axis=1) > 0).all()                                   # a keypoint inside its plane has samples that vote
        assert (d[top].max(axis=1) > 0).any() and (d[top].max(axis=1) == 0).any()   # (the 6 x 4 plane has 8 interior samples)


# ---- the full calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm,refine", [(False, None), (True, None), (False, (3, 5, 0.02)), (True, (3, 5, 0.02))])
def test_full_calls_equal_the_explicit_chain(sift_finder, bm, refine):
    """sf_get_features_and_descriptor = the restated detector (-> the restated cornerSubPix) -> the device's LK or block
    matching -> the restated SIFT::compute on the chain's keypoints."""
    import torch
    f = sift_finder
    h, w = 120, 160
    det = _abi.detector_params(100)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(700, width=w, height=h, max_disp=20.0)[:2])
    cprm, prm = _abi.sift_params(contrast_threshold=0.02), ref.Params(contrast_threshold=0.02)
    f.set_feature_type_sift(cprm)
    found = ref.detect(left, prm, det.max_features)
    n, got_kp = run_detect(f, torch, left, det.max_features, det.max_features)   # (sift None: the handle's parameters)
    assert n == len(found) and got_kp.tobytes() == found.tobytes()
    assert len(found) == det.max_features                                        # limitKeypoints cut the list
    kp = subpix_ref.refine_keypoints(left, found, *refine, (0, 0)) if refine else found
    chain, (kp, rx, st) = _device_chain(f, torch, left, right, cam, kp, bm)
    assert len(chain[0]) > 50
    assert_same(chain, ref.extract_keyframe(left, kp, rx, st, cam, prm), 128)
    if refine:
        f.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), *refine))
        assert (kp["x"] != found["x"]).any()
    if bm:
        f.stereo_set_params(_abi.stereo_params(0, 1))
    single = f.get_features_and_descriptor(left, right, cam, det)
    assert_same(single[:3], chain, 128)
    assert np.isfinite(single[1]).all(axis=1).sum() > 20                         # 3D points came out of the stereo step
    if not refine and not bm:
        u8 = f.get_features_and_descriptor_u8(left, right, _abi.SF_IMAGE_MONO8, cam, det)
        assert_same(u8[:3], single[:3], 128)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _state(f):
    return f.get_feature_type()[0], bytes(f.get_sift_params()), bytes(f.get_surf_params()), f.store_size()


def test_refusals_change_nothing(sift_finder):
    import torch
    f = sift_finder
    S = _abi.sift_params
    f.set_feature_type_sift(S(contrast_threshold=0.03, n_octave_layers=4))
    before = _state(f)
    assert before[0] == 1
    bad = [S(n_features=-1), S(n_octave_layers=0), S(n_octave_layers=9), S(contrast_threshold=-0.01),
           S(contrast_threshold=float("nan")), S(contrast_threshold=float("inf")), S(edge_threshold=0.0),
           S(edge_threshold=float("nan")), S(edge_threshold=float("inf")), S(sigma=0.79), S(sigma=8.01), S(sigma=float("nan"))]
    dev = torch.device("cuda:0")
    d_img = torch.zeros((48, 64), dtype=torch.uint8, device=dev)
    out = torch.zeros((16, 28), dtype=torch.uint8, device=dev)
    for prm in bad:
        with pytest.raises(lib.SepfinderError) as e:
            f.set_feature_type_sift(prm)
        assert e.value.code == _abi.SF_EINVAL and _state(f) == before, bytes(prm)
        with pytest.raises(lib.SepfinderError) as e:                             # the detector refuses the same parameters
            f.detect_sift(d_img.data_ptr(), 64, 48, 64, 0, out.data_ptr(), 16, prm)
        assert e.value.code == _abi.SF_EINVAL and _state(f) == before
    with pytest.raises(lib.SepfinderError) as e:                                 # the generic call names the SIFT one
        f.set_feature_type(1)
    assert e.value.code == _abi.SF_EINVAL and "sf_set_feature_type_sift" in str(e.value) and _state(f) == before
    for ft in (4, 6, 8):                                                         # the binary types stay refused on this handle
        with pytest.raises(lib.SepfinderError) as e:
            f.set_feature_type(ft)
        assert e.value.code == _abi.SF_EINVAL and _state(f) == before
    with pytest.raises(lib.SepfinderError):
        f.set_feature_type_orb()
    with pytest.raises(lib.SepfinderError):
        f.set_feature_type_freak(5)
    with pytest.raises(lib.SepfinderError):
        f.set_feature_type_surf()                                                # 64 dimensions on a 512-byte handle
    assert _state(f) == before
    # ROI, grid and every batch form under type 1
    h, w = 120, 160
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(3, width=w, height=h, max_disp=20.0)[:2])
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    f.front_set_params(_abi.front_params((0.1, 0.0, 0.0, 0.0), 3, 0, 0.02))
    with pytest.raises(lib.SepfinderError) as e:
        f.get_features_and_descriptor(left, right, cam)
    assert e.value.code == _abi.SF_EINVAL and "RoiRatios" in str(e.value) and "not built" in str(e.value) and _state(f) == before
    f.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), 3, 0, 0.02))
    f.grid_set_params(_abi.grid_params(2, 2))
    with pytest.raises(lib.SepfinderError) as e:
        f.get_features_and_descriptor(left, right, cam)
    assert e.value.code == _abi.SF_EINVAL and "Grid" in str(e.value) and "not built" in str(e.value) and _state(f) == before
    f.grid_set_params(_abi.grid_params(1, 1))
    for call in (f.get_features_and_descriptor_batch_device, f.get_features_and_descriptor_orb_batch_device,
                 f.get_features_and_descriptor_surf_batch_device):
        with pytest.raises(lib.SepfinderError) as e:
            call(None, None, 0, w, h, w, w * h, cam)
        assert e.value.code == _abi.SF_EINVAL and "not built" in str(e.value) and _state(f) == before
    for call in (f.add_keyframes_u8_batch_device, f.add_keyframes_orb_u8_batch_device, f.add_keyframes_surf_u8_batch_device):
        with pytest.raises(lib.SepfinderError) as e:
            call(None, None, None, _abi.SF_IMAGE_MONO8, 0, w, h, w, w * h, cam)
        assert e.value.code == _abi.SF_EINVAL and "not built" in str(e.value) and _state(f) == before
    # a handle with desc_type 0, and one whose rows are 256 bytes
    with lib.SeparatorFinder(synth.camera_params(), device=0) as g:
        with pytest.raises(lib.SepfinderError) as e:
            g.set_feature_type_sift()
        assert e.value.code == _abi.SF_EINVAL and "desc_type" in str(e.value) and g.get_feature_type()[0] == 6
    with lib.SeparatorFinder(_params(64), device=0) as g:
        with pytest.raises(lib.SepfinderError) as e:
            g.set_feature_type_sift()
        assert e.value.code == _abi.SF_EINVAL and g.get_feature_type()[0] == 6
    # SIFT -> SURF extended -> SIFT: the same bytes again
    a = f.get_features_and_descriptor(left, right, cam)
    f.set_feature_type_surf(_abi.surf_params(extended=1))
    s = f.get_features_and_descriptor(left, right, cam)
    assert f.get_feature_type()[0] == 0 and s[0].shape[1] == 512
    f.set_feature_type_sift(f.get_sift_params())
    b = f.get_features_and_descriptor(left, right, cam)
    assert len(a[0]) > 20 and b[3] == a[3] + 2
    assert_same(b[:3], a[:3], 128)
    assert a[0].tobytes() != s[0][:len(a[0])].tobytes()


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_of_sift_keyframes(estimation_type):
    """Two views of one scene (a stereo pair and its copy shifted by 8 pixels) under type 1: verify_pairs on the store's
    float32 rows equals the oracle's L2 path on the wire copies, 3D-3D and PnP; a keyframe against itself succeeds."""
    h, w = 240, 320
    wide_l, wide_r, _ = ec.make_stereo_pair(700, width=w + 8, height=h, max_disp=40.0)
    views = [(np.ascontiguousarray(wide_l[:, o:o + w]), np.ascontiguousarray(wide_r[:, o:o + w])) for o in (0, 8)]
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(400)
    f = _finder(128, estimation_type=estimation_type)
    try:
        f.set_feature_type_sift(_abi.sift_params(contrast_threshold=0.02))
        a = f.get_features_and_descriptor(*views[0], cam, det)
        b = f.get_features_and_descriptor(*views[1], cam, det)
        a2 = f.get_features_and_descriptor(*views[0], cam, det)
        assert_same(a2[:3], a[:3], 128)
        assert a[0].shape[1] == 512 and len(a[0]) > 100 and len(b[0]) > 100
        host = {s[3]: (s[0].view(np.float32), s[1], s[2]) for s in (a, b, a2)}
        fr, to = [a[3], a[3], b[3]], [a2[3], b[3], a2[3]]
        res = f.verify_pairs(fr, to)
        for j, (x, y) in enumerate(zip(fr, to)):
            o = pyoracle.estimate_transform(f.params, _abi.FeatureArrays(*host[x]), _abi.FeatureArrays(*host[y]))
            print("pair %d: success gpu %d oracle %d, inliers %d / %d, matches %d / %d" % (
                j, res[j]["success"], o["success"], res[j]["inliers"], o["inliers"], res[j]["matches"], o["matches"]))
            assert_result_parity(res[j], o, "pair %d" % j)
        assert res[0]["success"] == 1 and res[0]["inliers"] > 20               # the keyframe against itself
    finally:
        f.close()
