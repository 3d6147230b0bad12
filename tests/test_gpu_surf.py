"""GPU: SURF (Vis/FeatureType 0; csrc/k_surf.hip) against the NumPy restatement tests/surf_ref.py, byte for byte -- the
fast-Hessian detector with all seven keypoint fields, then orientation and float32 rows on given keypoints with the 3D
points and their NaNs in place -- then the full extraction calls against the explicit chain detector -> refinement ->
stereo correspondence -> extraction, the refusals, and two SURF keyframes through the verification path against the
oracle.  Every test fails without the feature: the symbols it calls are new."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from oracle import pyoracle
from tests import extract_cases as ec
from tests import image_ref, orb2_ref, subpix_ref
from tests import surf_ref as ref

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
POS_TOL = 1e-4   # metres   (BASELINE.json north_star, as tests/test_gpu_verify.py)
ROT_TOL = 1e-3   # radians
# keypoint sizes of the extraction cases (300 x 200 images): the detector's smallest (9), a fractional one, sizes whose
# (int)(21 s) window is 28 .. 170 pixels, 150 (a 420-pixel window: wider than the image, clamped sampling), 370 (a wavelet of
# 198 pixels: it fits, but nearly every sample falls outside), 400 (a wavelet of 214 > 201: dropped), -1 and 0 (dropped)
SIZES = np.array([9, 12.5, 20, 33, 61, 150, 370, 400, -1, 0], np.float32)
PARAM_SETS = {
    "defaults": {},
    "threshold 0": dict(hessian_threshold=0.0),
    "1 octave, 1 layer": dict(n_octaves=1, n_octave_layers=1),
    "5 octaves, 4 layers": dict(n_octaves=5, n_octave_layers=4, hessian_threshold=100.0),
}
IMAGES = {"64x48": (64, 48, 0), "97x61": (97, 61, 0), "160x120 padded": (160, 120, 13), "320x240": (320, 240, 0)}


def _params(dims=64, estimation_type=0, w=320, h=240):
    p = synth.camera_params()
    p.max_features = 2048
    p.fx, p.fy, p.cx, p.cy = 460.0, 458.0, w / 2.0, h / 2.0
    p.image_width, p.image_height = w, h
    p.estimation_type = estimation_type
    p.desc_type, p.desc_bytes = 1, 4 * dims
    return p


def _finder(dims=64, **kw):
    import torch
    f = lib.SeparatorFinder(_params(dims, **kw), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


@pytest.fixture()
def finder():
    f = _finder(64)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def texture(name):
    """Blobs on blocky noise at several scales, uint8 with pitch = width + pad.  Images at least 160 wide repeat their left
    half on the right, so that interior keypoints come in pairs of exactly equal response: the order of ties is tested."""
    w, h, pad = IMAGES[name]
    tw = w // 2 if w >= 160 else w
    rng = np.random.default_rng(len(name) * 131 + w)
    img = np.zeros((h, tw))
    for s in (2, 4, 8, 16):
        img += np.kron(rng.normal(size=(h // s + 1, tw // s + 1)), np.ones((s, s)))[:h, :tw] * s
    yy, xx = np.mgrid[0:h, 0:tw]
    for _ in range(12):
        cx, cy, r = rng.uniform(8, tw - 8), rng.uniform(8, h - 8), rng.uniform(2.0, 9.0)
        img += rng.choice([-60.0, 60.0]) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))
    img = np.clip(128 + 2.5 * img, 0, 255).astype(np.uint8)
    buf = np.full((h, w + pad), 0xA5, np.uint8)
    buf[:, :tw] = img
    buf[:, tw:2 * tw] = img[:, :w - tw]
    buf.setflags(write=False)
    return buf[:, :w]


@functools.lru_cache(maxsize=None)
def detected(name, pset):
    """The restatement's keypoints of an image under a parameter set, before limitKeypoints: computed once."""
    kp = ref.detect(texture(name), ref.Params(**PARAM_SETS[pset]), 0)
    kp.setflags(write=False)
    return kp


def _up(torch, a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        a = a.view(np.uint8)
    return torch.from_numpy(a).to(dev)


def _image_up(torch, image, dev):
    h, w = image.shape
    pitch = image.strides[0]
    base = np.lib.stride_tricks.as_strided(image, shape=(h, pitch), strides=(pitch, 1)) if pitch != w else image
    return _up(torch, np.array(base), dev), pitch                               # (a copy: the cached images are read-only)


def run_detect(f, torch, image, max_features, cap, prm=None):
    dev = torch.device("cuda:0")
    h, w = image.shape
    d_img, pitch = _image_up(torch, image, dev)
    out = torch.full((max(cap, 1), 28), 0xEE, dtype=torch.uint8, device=dev)
    n = f.detect_surf(d_img.data_ptr(), w, h, pitch, max_features, out.data_ptr(), cap, prm)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[min(n, cap):] == 0xEE).all()                                    # nothing behind the result is touched
    return n, np.frombuffer(raw[:min(n, cap)].tobytes(), dtype=KP)


@pytest.mark.parametrize("name,pset", [(i, p) for i in IMAGES for p in PARAM_SETS if p != "5 octaves, 4 layers" or i == "64x48"])
def test_detector_equals_restatement(finder, name, pset):
    """All seven fields of every keypoint, in order, for max_features = no limit, below, at and above the number found
    (limitKeypoints cuts and reorders equal responses), and a cap below the result."""
    import torch
    image = texture(name)
    all_kp = detected(name, pset)
    N = len(all_kp)
    cprm = _abi.surf_params(**PARAM_SETS[pset])
    print("%s, %s: %d keypoints, octaves %s, sizes %s .. %s, %d equal responses" % (
        name, pset, N, np.bincount(all_kp["octave"]).tolist(), all_kp["size"].min() if N else None,
        all_kp["size"].max() if N else None, N - len(np.unique(all_kp["response"]))))
    assert N >= 3
    if image.shape[1] >= 160:
        assert N > 50 and N - len(np.unique(all_kp["response"])) > 10            # the repeated half: pairs of equal responses
    if pset == "5 octaves, 4 layers":
        # layers of 96 .. 528 pixels do not fit 64 x 48: skipped, and octaves 2 .. 4 have no middle layer with a neighbourhood
        assert N > 0 and all_kp["octave"].max() <= 1
    for maxf in (0, max(N // 2, 1), N, N + 10):
        want = orb2_ref.limit_keypoints(all_kp, maxf)
        n, got = run_detect(finder, torch, image, maxf, max(N, 1), cprm)
        assert n == len(want), (maxf, n, len(want))
        assert got.tobytes() == want.tobytes(), maxf
    if N >= 4:
        n, got = run_detect(finder, torch, image, 0, N // 3, cprm)              # cap < result: the count is still the result's
        assert n == N and got.tobytes() == all_kp[:N // 3].tobytes()
    if N:
        assert (all_kp["angle"] == -1).all() and set(np.unique(all_kp["class_id"])) <= {-1, 0, 1}
        assert (np.diff(all_kp["response"]) <= 0).all() and all_kp["response"].min() > cprm.hessian_threshold


def test_detector_on_any_handle_and_without_maxima():
    """The detector writes no descriptor: a binary handle runs it with the parameters it is given (and with the defaults of
    its own); a constant image has no maxima."""
    import torch
    p = synth.camera_params()
    with lib.SeparatorFinder(p, device=0) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        image = texture("97x61")
        want = detected("97x61", "defaults")
        n, got = run_detect(f, torch, image, 0, len(want), None)
        assert n == len(want) and got.tobytes() == want.tobytes()
        flat = np.full((48, 64), 77, np.uint8)
        n, got = run_detect(f, torch, flat, 0, 16, _abi.surf_params(hessian_threshold=0.0))
        assert n == 0 and len(got) == 0
        assert len(ref.detect(flat, ref.Params(hessian_threshold=0.0))) == 0
        assert f.get_feature_type()[0] == 6


# ---- extraction on given keypoints ------------------------------------------------------------------------------------
def surf_case(seed, **kw):
    """extract_cases.make_case at 300 x 200 with the sizes drawn from SIZES, a sixth of the keypoints moved onto / half a
    pixel inside the image border, and a few outside the image (every orientation sample falls outside: dropped)."""
    image, kp, rx, st, cam = ec.make_case(seed, width=300, height=200, **kw)
    h, w = image.shape
    rng = np.random.default_rng(2000 + seed)
    n = len(kp)
    kp["size"] = rng.choice(SIZES, n)
    kp["angle"] = rng.choice(np.array([-1.0, 0.0, 45.0], np.float32), n)         # overwritten either way
    for i in np.nonzero(rng.random(n) < 1 / 6)[0]:
        axis, side = ("x", w) if rng.random() < 0.5 else ("y", h)
        lim = [0.0, 0.5, side - 1.0, side - 0.5, -300.0, side + 300.0][rng.integers(6)]
        if rx is not None and axis == "x":
            rx[i] += np.float32(lim) - kp["x"][i]                                # the disparity goes along
        kp[axis][i] = lim
    return image, kp, rx, st, cam


@functools.lru_cache(maxsize=None)
def extract_reference(seed, n, upright, extended, depth):
    kw = dict(n=n, **(dict(min_depth=0.8, max_depth=12.0) if depth else {}))
    image, kp, rx, st, cam = surf_case(seed, **kw)
    trace = {}
    want = ref.extract_keyframe(image, kp, rx, st, cam, ref.Params(upright=upright, extended=extended), trace)
    return (image, kp, rx, st, cam), want, trace


def run_extract(f, torch, image, kp, rx, st, cam):
    dev = torch.device("cuda:0")
    h, w = image.shape
    d_img, pitch = _image_up(torch, image, dev)
    n = len(kp)
    d_kp = _up(torch, kp, dev) if n else None
    d_rx = _up(torch, rx, dev) if rx is not None and n else None
    d_st = _up(torch, st, dev) if st is not None and n else None
    nb = f.descriptor_bytes()
    d_desc = torch.zeros((max(n, 1), nb), dtype=torch.uint8, device=dev)
    d_xyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    d_kout = torch.zeros((max(n, 1), 28), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    slot, rows = f.extract_keyframe_device(ptr(d_img), w, h, pitch, ptr(d_kp), ptr(d_rx), ptr(d_st), n, cam,
                                           d_desc.data_ptr(), d_xyz.data_ptr(), d_kout.data_ptr())
    torch.cuda.synchronize()
    desc = d_desc.cpu().numpy()[:rows].view(np.float32)
    xyz = d_xyz.cpu().numpy()[:rows]
    kout = np.frombuffer(d_kout.cpu().numpy().tobytes(), dtype=KP)[:rows]
    return slot, rows, desc, xyz, kout


def assert_same(got, want, dims=None):
    desc, xyz, kout = got
    d, p, k = want
    desc = np.asarray(desc).view(np.float32) if np.asarray(desc).dtype == np.uint8 else np.asarray(desc)
    d = np.asarray(d).view(np.float32) if np.asarray(d).dtype == np.uint8 else np.asarray(d)
    assert len(desc) == len(d)
    if dims is not None:
        assert desc.shape[1] == dims
    assert kout.tobytes() == k.tobytes()
    if desc.tobytes() != d.tobytes():
        bad = np.nonzero((desc.view(np.int32) != d.view(np.int32)).any(axis=1))[0]
        raise AssertionError("rows differ at %s of %d: max |diff| %g, keypoint %s" % (
            bad[:8].tolist(), len(d), np.abs(desc - d).max(), k[bad[0]]))
    assert np.array_equal(np.isnan(xyz), np.isnan(p))
    assert xyz[~np.isnan(xyz)].tobytes() == p[~np.isnan(p)].tobytes()


@pytest.mark.parametrize("upright,extended", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("seed,n,depth", [(9, 257, False), (2, 257, True), (6, 0, False), (13, 1, False)])
def test_extraction_equals_restatement(seed, n, depth, upright, extended):
    import torch
    (image, kp, rx, st, cam), want, trace = extract_reference(seed, n, upright, extended, depth)
    dims = 128 if extended else 64
    f = _finder(dims)
    try:
        f.set_feature_type_surf(_abi.surf_params(upright=upright, extended=extended))
        assert f.get_feature_type()[0] == 0 and f.descriptor_bytes() == 4 * dims
        slot, rows, desc, xyz, kout = run_extract(f, torch, image, kp, rx, st, cam)
        print("seed %d upright %d extended %d: %d of %d rows, windows %s .. %s" % (
            seed, upright, extended, rows, len(kp), min(trace.get("win", [0])), max(trace.get("win", [0]))))
        assert rows == len(want[0])
        assert_same((desc.reshape(rows, dims), xyz, kout), want, dims)
        assert f.store_size() == slot + 1
    finally:
        f.close()
    if n >= 257:
        h, w = image.shape
        assert 0 < rows < n
        kept = set(zip(want[2]["x"].tolist(), want[2]["y"].tolist()))
        sizes_kept = set(want[2]["size"].tolist())
        assert 400.0 not in sizes_kept and -1.0 not in sizes_kept and 0.0 not in sizes_kept
        if not depth:
            assert 150.0 in sizes_kept and max(trace["win"]) > w                # a window wider than the image was sampled
            for axis, side in (("x", w), ("y", h)):                            # keypoints on the border were among the kept
                assert ((want[2][axis] == 0.0) | (want[2][axis] == side - 1.0) | (want[2][axis] == 0.5) |
                        (want[2][axis] == side - 0.5)).any()
        assert (kp["x"] == -300.0).any()
        if upright:                                                            # (no orientation: nothing is sampled, nothing dropped)
            assert (want[2]["angle"] == 270.0).all()
            assert depth or any(x == -300.0 for x, _ in kept)                  # (with a depth range they have no 3D point)
        else:
            assert not any(x == -300.0 for x, _ in kept)                       # every orientation sample outside: dropped
            assert len(np.unique(want[2]["angle"])) > rows // 2
            assert min(trace["ori_samples"]) < ref.ORI_SAMPLES                  # some orientation samples fell outside
        norms = np.linalg.norm(want[0].astype(np.float64), axis=1)
        assert np.allclose(norms, 1.0, atol=1e-5)


# ---- the full calls ---------------------------------------------------------------------------------------------------
def _device_chain(f, torch, left, right, cam, kp, bm=False):
    """Given keypoints -> the device's stereo correspondence -> the device's extraction, and what the stereo step gave.
    Returns ((desc, xyz, kpts), (kp, rx, st))."""
    dev = torch.device("cuda:0")
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    n, nb = len(kp), f.descriptor_bytes()
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_kp = _up(torch, kp, dev) if n else torch.zeros((28,), dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((max(n, 1), 2), dtype=torch.float32, device=dev)
    d_rx = torch.zeros((max(n, 1),), dtype=torch.float32, device=dev)
    d_st = torch.zeros((max(n, 1),), dtype=torch.uint8, device=dev)
    stereo = f.stereo_block_match_device if bm else f.stereo_correspondences_device
    stereo(d_l.data_ptr(), d_r.data_ptr(), w, h, w, d_kp.data_ptr(), n, d_xy.data_ptr(), d_st.data_ptr(), d_rx.data_ptr())
    desc = torch.zeros((max(n, 1), nb), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    kpo = torch.zeros((max(n, 1), 28), dtype=torch.uint8, device=dev)
    slot, rows = f.extract_keyframe_device(d_l.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), n, cam,
                                           desc.data_ptr(), xyz.data_ptr(), kpo.data_ptr())
    torch.cuda.synchronize()
    got = (desc.cpu().numpy()[:rows], xyz.cpu().numpy()[:rows], np.frombuffer(kpo.cpu().numpy()[:rows].tobytes(), dtype=KP))
    return got, (kp, d_rx.cpu().numpy()[:n], d_st.cpu().numpy()[:n])


@pytest.mark.parametrize("bm,refine", [(False, None), (True, None), (False, (3, 5, 0.02)), (True, (3, 5, 0.02))])
def test_full_calls_equal_the_explicit_chain(finder, bm, refine):
    """sf_get_features_and_descriptor = the restated detector (-> the restated cornerSubPix) -> the device's LK or block
    matching -> the restated SURF::compute on the chain's keypoints; the rgb8 form = the gray form on image_ref's planes."""
    import torch
    h, w = 240, 320
    det = _abi.detector_params(300)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(700, width=w, height=h, max_disp=40.0)[:2])
    cprm, prm = _abi.surf_params(hessian_threshold=300.0), ref.Params(hessian_threshold=300.0)
    finder.set_feature_type_surf(cprm)
    found = ref.detect(left, prm, det.max_features)
    n, got_kp = run_detect(finder, torch, left, det.max_features, det.max_features)
    assert n == len(found) and got_kp.tobytes() == found.tobytes()
    assert len(found) == det.max_features                                      # limitKeypoints cut the list
    kp = subpix_ref.refine_keypoints(left, found, *refine, (0, 0)) if refine else found
    chain, (kp, rx, st) = _device_chain(finder, torch, left, right, cam, kp, bm)
    assert len(chain[0]) > 100
    assert_same(chain, ref.extract_keyframe(left, kp, rx, st, cam, prm), 64)
    if refine:
        finder.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), *refine))
        assert (kp["x"] != found["x"]).any()
    if bm:
        finder.stereo_set_params(_abi.stereo_params(0, 1))
    single = finder.get_features_and_descriptor(left, right, cam, det)
    assert_same(single[:3], chain, 64)
    assert np.isfinite(single[1]).all(axis=1).sum() > 50                       # 3D points came out of the stereo step
    if not refine:
        # the camera's rgb8 images: converted on the device, then the same as the gray call on the restated planes
        from tests.test_gpu_image import colourise
        cl, cr = colourise(left, 31), colourise(right, 32)
        u8 = finder.get_features_and_descriptor_u8(cl, cr, _abi.SF_IMAGE_RGB8, cam, det)
        gl, gr = image_ref.gray(cl, _abi.SF_IMAGE_RGB8, 0), image_ref.gray(cr, _abi.SF_IMAGE_RGB8, 0)
        plain = finder.get_features_and_descriptor(np.ascontiguousarray(gl), np.ascontiguousarray(gr), cam, det)
        assert len(u8[0]) > 100
        assert_same(u8[:3], plain[:3], 64)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _state(f):
    return f.get_feature_type()[0], bytes(f.get_surf_params()), f.store_size()


def test_refusals_change_nothing(finder):
    import torch
    S = _abi.surf_params
    finder.set_feature_type_surf(S(hessian_threshold=400.0, n_octave_layers=3))
    before = _state(finder)
    assert before[0] == 0
    bad = [S(hessian_threshold=-1.0), S(hessian_threshold=float("nan")), S(hessian_threshold=float("inf")), S(n_octaves=0),
           S(n_octaves=9), S(n_octave_layers=0), S(n_octave_layers=9), S(upright=2), S(extended=-1),
           S(extended=1)]                                                      # (the last: 512-byte rows on a 256-byte handle)
    for prm in bad:
        with pytest.raises(lib.SepfinderError) as e:
            finder.set_feature_type_surf(prm)
        assert e.value.code == _abi.SF_EINVAL, bytes(prm)
        assert _state(finder) == before
    dev = torch.device("cuda:0")
    d_img = torch.zeros((48, 64), dtype=torch.uint8, device=dev)
    out = torch.zeros((16, 28), dtype=torch.uint8, device=dev)
    for prm in bad[:-1]:                                                       # the detector refuses the same parameters
        with pytest.raises(lib.SepfinderError) as e:
            finder.detect_surf(d_img.data_ptr(), 64, 48, 64, 0, out.data_ptr(), 16, prm)
        assert e.value.code == _abi.SF_EINVAL and _state(finder) == before
    with pytest.raises(lib.SepfinderError) as e:                               # the generic call names the SURF one
        finder.set_feature_type(0)
    assert e.value.code == _abi.SF_EINVAL and "sf_set_feature_type_surf" in str(e.value) and _state(finder) == before
    for ft in (4, 6, 8):                                                       # the binary types stay refused on this handle
        with pytest.raises(lib.SepfinderError) as e:
            finder.set_feature_type(ft)
        assert e.value.code == _abi.SF_EINVAL and _state(finder) == before
    with pytest.raises(lib.SepfinderError):
        finder.set_feature_type_orb()
    with pytest.raises(lib.SepfinderError):
        finder.set_feature_type_freak(5)
    assert _state(finder) == before
    # ROI, grid and every batch form under type 0
    h, w = 120, 160
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(3, width=w, height=h, max_disp=20.0)[:2])
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    finder.front_set_params(_abi.front_params((0.1, 0.0, 0.0, 0.0), 3, 0, 0.02))
    with pytest.raises(lib.SepfinderError) as e:
        finder.get_features_and_descriptor(left, right, cam)
    assert e.value.code == _abi.SF_EINVAL and "RoiRatios" in str(e.value) and _state(finder) == before
    finder.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), 3, 0, 0.02))
    finder.grid_set_params(_abi.grid_params(2, 2))
    with pytest.raises(lib.SepfinderError) as e:
        finder.get_features_and_descriptor(left, right, cam)
    assert e.value.code == _abi.SF_EINVAL and "Grid" in str(e.value) and _state(finder) == before
    finder.grid_set_params(_abi.grid_params(1, 1))
    for call in (finder.get_features_and_descriptor_batch_device, finder.get_features_and_descriptor_orb_batch_device):
        with pytest.raises(lib.SepfinderError) as e:
            call(None, None, 0, w, h, w, w * h, cam)
        assert e.value.code == _abi.SF_EINVAL and _state(finder) == before
    for call in (finder.add_keyframes_u8_batch_device, finder.add_keyframes_orb_u8_batch_device):
        with pytest.raises(lib.SepfinderError) as e:
            call(None, None, None, _abi.SF_IMAGE_MONO8, 0, w, h, w, w * h, cam)
        assert e.value.code == _abi.SF_EINVAL and _state(finder) == before
    # a handle with desc_type 0, and one whose rows are 512 bytes
    with lib.SeparatorFinder(synth.camera_params(), device=0) as g:
        with pytest.raises(lib.SepfinderError) as e:
            g.set_feature_type_surf()
        assert e.value.code == _abi.SF_EINVAL and "desc_type" in str(e.value) and g.get_feature_type()[0] == 6
    with lib.SeparatorFinder(_params(128), device=0) as g:
        assert g.get_feature_type()[0] == 6
        with pytest.raises(lib.SepfinderError) as e:
            g.set_feature_type_surf()                                          # 64 dimensions on a 512-byte handle
        assert e.value.code == _abi.SF_EINVAL and g.get_feature_type()[0] == 6
        g.set_feature_type_surf(S(extended=1))
        assert g.get_feature_type()[0] == 0 and g.descriptor_bytes() == 512
    # 0 -> 6 refused -> 0: the same bytes again
    a = finder.get_features_and_descriptor(left, right, cam)
    with pytest.raises(lib.SepfinderError):
        finder.set_feature_type(6)
    finder.set_feature_type_surf(finder.get_surf_params())
    b = finder.get_features_and_descriptor(left, right, cam)
    assert len(a[0]) > 20 and b[3] == a[3] + 1
    assert_same(b[:3], a[:3], 64)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def assert_result_parity(g, o, ctx=""):
    for k in ("success", "pass1_success", "pass2_guided", "inliers", "matches", "inliers_pass1", "matches_pass1"):
        assert g[k] == o[k], "%s %s: gpu %s oracle %s" % (ctx, k, g[k], o[k])
    if o["success"]:
        assert np.linalg.norm(g["position"] - o["position"]) <= POS_TOL, ctx
        d = abs(float(np.dot(g["orientation"], o["orientation"])))
        d /= max(np.linalg.norm(g["orientation"]) * np.linalg.norm(o["orientation"]), 1e-300)
        assert 2.0 * np.arccos(np.clip(d, -1.0, 1.0)) <= ROT_TOL, ctx
    assert np.allclose(g["covariance"], o["covariance"], rtol=1e-9, atol=0), ctx


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_of_surf_keyframes(estimation_type):
    """Two views of one scene (a stereo pair and its copy shifted by 8 pixels) under type 0: verify_pairs on the store's
    float32 rows equals the oracle on the wire copies, 3D-3D and PnP; a keyframe against itself succeeds."""
    h, w = 240, 320
    wide_l, wide_r, _ = ec.make_stereo_pair(700, width=w + 8, height=h, max_disp=40.0)
    views = [(np.ascontiguousarray(wide_l[:, o:o + w]), np.ascontiguousarray(wide_r[:, o:o + w])) for o in (0, 8)]
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(400)
    f = _finder(64, estimation_type=estimation_type)
    try:
        f.set_feature_type_surf(_abi.surf_params(hessian_threshold=200.0))
        a = f.get_features_and_descriptor(*views[0], cam, det)
        b = f.get_features_and_descriptor(*views[1], cam, det)
        a2 = f.get_features_and_descriptor(*views[0], cam, det)
        assert_same(a2[:3], a[:3], 64)
        assert a[0].shape[1] == 256 and len(a[0]) > 100 and len(b[0]) > 100
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
