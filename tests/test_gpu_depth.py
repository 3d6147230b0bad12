"""GPU: depth keyframes through the C-ABI, byte for byte against the NumPy restatement tests/depth_ref.py -- the mask and the 3D
points of a depth image (csrc/k_depth.hip), the two corner detectors under a mask, sf_get_features_and_descriptor_depth
against the explicit chain (restated corners -> sf_extract_keyframe_depth_device), its batch forms against the single call,
and the refusals.  Images are 64 x 48 and 97 x 131, depth a seeded piecewise-planar scene with holes and steps in both
formats, pitches greater than a row.  Every test calls a symbol the library did not have before the depth path."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from tests import depth_cases as cases
from tests import depth_ref as ref
from tests import grid_ref

pytestmark = pytest.mark.gpu

U16, F32M = _abi.SF_DEPTH_U16_MM, _abi.SF_DEPTH_F32_M
FORMATS = {"u16": U16, "f32": F32M}
SENTINEL = 0xEE
KSZ = _abi.KEYPOINT_DTYPE.itemsize
W, H = 97, 131                                              # the size of the extraction tests (64 x 48 holds no BRIEF patch)


def _params(float_dims=0):
    p = synth.camera_params()
    p.max_features = 2048
    p.netvlad_dimensions = 128
    if float_dims:
        p.desc_type, p.desc_bytes = 1, 4 * float_dims
    return p


def _finder(float_dims=0):
    import torch
    f = lib.SeparatorFinder(_params(float_dims), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


@pytest.fixture()
def finder():
    f = _finder()
    yield f
    f.close()


def upload(torch, view):
    """A pitched 2-D view (ref.pitched) on the device: (tensor of the whole buffer, pitch in bytes)."""
    base = view.base if view.base is not None else view
    return torch.from_numpy(np.ascontiguousarray(base).view(np.uint8).reshape(base.shape[0], -1)).to("cuda:0"), base.strides[0]


def upload_kp(torch, kp):
    return torch.from_numpy(np.frombuffer(kp.tobytes(), np.uint8).copy().reshape(-1, KSZ) if len(kp) else np.zeros((1, KSZ), np.uint8)).to("cuda:0")


def keypoints(xy):
    kp = np.zeros(len(xy), _abi.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = np.asarray(xy, np.float32).T
    kp["size"], kp["angle"], kp["octave"], kp["class_id"] = 7.0, -1.0, 0, -1
    return kp


def configure(f, ftype):
    if ftype in (3, 5):
        f.set_feature_type_freak(ftype)
    elif ftype == 2:
        f.set_feature_type_orb()
    elif ftype == 0:
        f.set_feature_type_surf()
    elif ftype == 1:
        f.set_feature_type_sift()
    else:
        f.set_feature_type(ftype)


def finder_of(ftype):
    f = _finder({0: 64, 1: 128}.get(ftype, 0))
    configure(f, ftype)
    return f


def state(f):
    return f.store_size(), f.nn_sizes(), f.get_feature_type()[0], f.depth_get_params().depth_as_mask


# ---- the mask ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: "%dx%d" % s)
def test_depth_mask_equals_restatement(finder, size, fmt):
    import torch
    w, h = size
    n, elem = 3, 2 if fmt == "u16" else 4
    scenes = [ref.scene(w, h, 40, FORMATS[fmt]), ref.scene(w, h, 41, FORMATS[fmt], dead=True), ref.scene(w, h, 42, FORMATS[fmt])]
    # rows and bases that are not aligned; planes aligned for the wide loads and stores; a mask base off by one
    for pad, mask_pitch, base_off in ((5, w + 3, 0), ((-w) % 4 + 4, (w + 7) & ~3, 0), (3, w, 1)):
        pitch = (w + pad) * elem
        stride = pitch * h + 16 * elem
        buf = np.full((n, stride), 0xA5, np.uint8)
        for i, s in enumerate(scenes):
            np.lib.stride_tricks.as_strided(buf[i].view(s.dtype), shape=(h, w), strides=(pitch, elem))[...] = s
        d_depth = torch.from_numpy(buf).to("cuda:0")
        mask_stride = mask_pitch * h + 9
        for mn, mx in ((0.0, 0.0), (0.8, 4.5), (-1.0, 0.0)):
            d_mask = torch.full((n * mask_stride + 8,), SENTINEL, dtype=torch.uint8, device="cuda:0")
            finder.depth_mask_device(d_depth.data_ptr(), FORMATS[fmt], w, h, pitch, stride, n, mn, mx, d_mask.data_ptr() + base_off,
                                     mask_pitch, mask_stride)
            torch.cuda.synchronize()
            got = d_mask.cpu().numpy()
            want = np.full_like(got, SENTINEL)
            for i, s in enumerate(scenes):
                np.lib.stride_tricks.as_strided(want[base_off + i * mask_stride:], shape=(h, w), strides=(mask_pitch, 1))[...] = \
                    ref.depth_mask(s, mn, mx)
            assert got.tobytes() == want.tobytes(), (pad, mask_pitch, base_off, mn, mx)   # the masks, and nothing outside them
    # one image: strides are ignored
    d1, p1 = upload(torch, ref.pitched(scenes[0], 5))
    d_mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda:0")
    finder.depth_mask_device(d1.data_ptr(), FORMATS[fmt], w, h, p1, 1, 1, 0.5, 0.0, d_mask.data_ptr(), w, 3)
    torch.cuda.synchronize()
    assert d_mask.cpu().numpy().tobytes() == ref.depth_mask(scenes[0], 0.5, 0.0).tobytes()


# ---- the 3D points -------------------------------------------------------------------------------------------------------
def point_cases(w, h, depth, seed):
    """Coordinates that take every path of the pixel rule and of the smoothing."""
    rng = np.random.default_rng(seed)
    v = ref.values(depth)
    with np.errstate(invalid="ignore"):
        hy, hx = np.nonzero(~(np.isfinite(v) & (v != 0)))
    xy = [(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (2.5, 3.5), (10.5, 7.49999), (w - 1.5, h - 1.5), (w - 0.4, 5), (5, h - 0.4),
          (w - 0.5, h - 0.5), (w, 4), (4, h), (w + 0.2, h + 3), (-0.5, 3), (-0.7, -0.7), (-1.5, 2), (3, -1.6), (-1.4999, 0),
          (np.nan, 3), (4, np.nan), (np.inf, 3), (3, -np.inf), (3e38, 2), (-3e38, 2), (2.0 ** 31, 1), (-2.0 ** 31 - 1024, 1)]
    xy += [(float(x), float(y)) for x, y in zip(hx[:12], hy[:12])]                         # on holes
    xy += [(float(x) + 0.3, float(y) - 0.2) for x, y in zip(hx[12:40:3] + 1, hy[12:40:3])]  # beside holes
    xy += list(zip(rng.uniform(-2, w + 2, 300), rng.uniform(-2, h + 2, 300)))
    xy += list(zip(rng.integers(0, w, 100).astype(float), rng.integers(0, h, 100).astype(float)))
    return keypoints(xy)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: "%dx%d" % s)
def test_depth_points_equal_restatement(finder, size, fmt):
    import torch
    w, h = size
    depth = ref.scene(w, h, 50, FORMATS[fmt])
    kp = point_cases(w, h, depth, 51)
    d_depth, pitch = upload(torch, ref.pitched(depth, 5))
    d_kp = upload_kp(torch, kp)
    n = len(kp)
    seen = set()
    for cam in (ref.camera(w, h), ref.camera(w, h, local=True), ref.camera(w, h, min_depth=0.8, max_depth=4.5),
                ref.camera(w, h, local=True, min_depth=-1.0, max_depth=3.0), ref.camera(w, h, cx=0.0, cy=-2.0)):
        d_xyz = torch.full((n * 12 + 12,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        d_valid = torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        finder.depth_points_device(d_depth.data_ptr(), FORMATS[fmt], w, h, pitch, d_kp.data_ptr(), n, cam, d_xyz.data_ptr(),
                                   d_valid.data_ptr())
        torch.cuda.synchronize()
        got, valid = d_xyz.cpu().numpy(), d_valid.cpu().numpy()
        want = ref.keypoints3d_depth(kp, depth, cam)
        assert (got[n * 12:] == SENTINEL).all() and valid[n] == SENTINEL
        bad = np.flatnonzero((np.frombuffer(got[:n * 12].tobytes(), np.uint32).reshape(n, 3) != want.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (bad[:5], kp[bad[:5]], want[bad[:5]])
        assert valid[:n].tobytes() == ref.points_valid(want).tobytes()
        seen.add((int(valid[:n].sum()) > 50, int((valid[:n] == 0).sum()) > 50))
        # without the optional output
        finder.depth_points_device(d_depth.data_ptr(), FORMATS[fmt], w, h, pitch, d_kp.data_ptr(), n, cam, d_xyz.data_ptr(), None)
    torch.cuda.synchronize()
    assert seen == {(True, True)}                           # points and non-points in every run
    finder.depth_points_device(d_depth.data_ptr(), FORMATS[fmt], w, h, pitch, None, 0, ref.camera(w, h), None, None)   # n = 0


# ---- the detectors under a mask ------------------------------------------------------------------------------------------
def run_detector(f, torch, kind, img, mask, limit, extra, cap=None):
    """One masked (mask an array) or unmasked (mask None) detector call on pitched copies: (n, keypoints)."""
    h, w = img.shape
    d_img, pitch = upload(torch, ref.pitched(img, 7))
    cap = w * h if cap is None else cap
    d_kp = torch.full((cap + 1, KSZ), SENTINEL, dtype=torch.uint8, device="cuda:0")
    if mask is not None:
        d_mask, mpitch = upload(torch, ref.pitched(np.ascontiguousarray(mask), 11, fill=0x00))
    if kind == "gftt":
        if mask is None:
            n = f.detect_corners_device(d_img.data_ptr(), w, h, pitch, limit, cases.QUALITY, cases.MIN_DISTANCE, d_kp.data_ptr(), cap)
        else:
            n = f.detect_corners_masked_device(d_img.data_ptr(), w, h, pitch, d_mask.data_ptr(), mpitch, limit, cases.QUALITY,
                                               cases.MIN_DISTANCE, d_kp.data_ptr(), cap)
    else:
        prm = _abi.fast_params(*extra)
        if mask is None:
            n = f.detect_fast_device(d_img.data_ptr(), w, h, pitch, limit, d_kp.data_ptr(), cap, prm)
        else:
            n = f.detect_fast_masked_device(d_img.data_ptr(), w, h, pitch, d_mask.data_ptr(), mpitch, limit, d_kp.data_ptr(), cap, prm)
    torch.cuda.synchronize()
    raw = d_kp.cpu().numpy()
    assert (raw[min(n, cap):] == SENTINEL).all()
    return n, np.frombuffer(raw[:min(n, cap)].tobytes(), dtype=_abi.KEYPOINT_DTYPE)


@pytest.mark.parametrize("case", list(cases.GFTT_CASES))
def test_masked_gftt_equals_restatement(finder, case):
    import torch
    _, _, _, _, _, (block, harris), maxc, _ = cases.GFTT_CASES[case]
    finder.gftt_set_params(_abi.gftt_params(block, harris, 0.04))
    img, mask, _ = cases.gftt_inputs(case)
    want = cases.gftt_want(case)
    n, kp = run_detector(finder, torch, "gftt", img, mask, maxc, None)
    print("%s: %d corners under the mask, gpu %d" % (case, len(want), n))
    assert n == len(want) >= 20 and kp.tobytes() == want.tobytes()          # all seven fields
    # a mask of 255: the unmasked call's bytes; a mask of 0: no corner, no error
    n_full, kp_full = run_detector(finder, torch, "gftt", img, np.full_like(mask, 255), maxc, None)
    n_plain, kp_plain = run_detector(finder, torch, "gftt", img, None, maxc, None)
    assert n_full == n_plain > 0 and kp_full.tobytes() == kp_plain.tobytes() == cases.gftt_want(case, "full").tobytes()
    assert kp_full.tobytes() != kp.tobytes()
    n_empty, kp_empty = run_detector(finder, torch, "gftt", img, np.zeros_like(mask), maxc, None)
    assert n_empty == 0 and len(kp_empty) == 0
    n_cap, kp_cap = run_detector(finder, torch, "gftt", img, mask, maxc, None, cap=7)       # cap below the result
    assert n_cap == n and kp_cap.tobytes() == want[:7].tobytes()


@pytest.mark.parametrize("case", list(cases.FAST_CASES))
def test_masked_fast_equals_restatement(finder, case):
    import torch
    _, _, _, _, _, prm, limit = cases.FAST_CASES[case]
    img, mask = cases.fast_inputs(case)
    want = cases.fast_want(case)
    n, kp = run_detector(finder, torch, "fast", img, mask, limit, prm)
    print("%s: %d corners under the mask, gpu %d" % (case, len(want), n))
    assert n == len(want) >= 20 and kp.tobytes() == want.tobytes()
    n_full, kp_full = run_detector(finder, torch, "fast", img, np.full_like(mask, 255), limit, prm)
    n_plain, kp_plain = run_detector(finder, torch, "fast", img, None, limit, prm)
    assert n_full == n_plain > 0 and kp_full.tobytes() == kp_plain.tobytes() == cases.fast_want(case, "full").tobytes()
    assert kp_full.tobytes() != kp.tobytes()
    n_empty, kp_empty = run_detector(finder, torch, "fast", img, np.zeros_like(mask), limit, prm)
    assert n_empty == 0 and len(kp_empty) == 0


# ---- the single call against the explicit chain --------------------------------------------------------------------------
MAXF = 150
LIMITS = (0.6, 5.0)                                         # Vis/MinDepth, Vis/MaxDepth of the chain tests: mask and filter both bite


@functools.lru_cache(maxsize=None)
def frame(seed, fmt, dead=False):
    img = ref.image(W, H, seed)
    depth = ref.scene(W, H, seed + 100, fmt, dead=dead)
    img.setflags(write=False)
    depth.setflags(write=False)
    return img, depth


def restated_corners(img, mask, ftype, maxf, grid=(1, 1), roi=(0.0, 0.0, 0.0, 0.0), gftt=(3, 0), fast=(20, 1)):
    """Feature2D::generateKeypoints with a mask for the two corner detectors: the ROI and the cells of grid_ref, in each the
    masked detector of depth_ref on the cropped image and the cropped mask (mask None: 255 everywhere)."""
    h, w = img.shape
    mask = np.full((h, w), 255, np.uint8) if mask is None else mask
    boxes, quota = grid_ref.cells(w, h, roi, grid[0], grid[1], maxf)
    out = []
    for x, y, cw, ch in boxes:
        ci, cm = np.ascontiguousarray(img[y:y + ch, x:x + cw]), np.ascontiguousarray(mask[y:y + ch, x:x + cw])
        if ftype in (4, 3):
            kp = ref.detect_fast_masked(ci, cm, fast[0], fast[1], quota)
        else:
            kp = ref.detect_corners_masked(ci, cm, quota, 0.001, 3.0, gftt[0], gftt[1], 0.04)
        kp = np.array(kp[:quota], copy=True)
        kp["x"] += np.float32(x)
        kp["y"] += np.float32(y)
        out.append(kp)
    return np.concatenate(out)


def device_corners(f, torch, img, maxf):
    """The handle's own detector (types 2, 0, 1 take no mask) on a device copy: its keypoints."""
    h, w = img.shape
    d_img = torch.from_numpy(np.array(img)).to("cuda:0")
    d_kp = torch.zeros((maxf, KSZ), dtype=torch.uint8, device="cuda:0")
    ftype = f.get_feature_type()[0]
    call = {2: f.detect_orb_device, 0: f.detect_surf, 1: f.detect_sift}[ftype]
    n = call(d_img.data_ptr(), w, h, w, maxf, d_kp.data_ptr(), maxf)
    torch.cuda.synchronize()
    return np.frombuffer(d_kp.cpu().numpy()[:min(n, maxf)].tobytes(), dtype=_abi.KEYPOINT_DTYPE)


def chain(f, torch, img, depth, kp, cam):
    """sf_extract_keyframe_depth_device on device copies with pitches greater than a row: (desc, xyz, kp, slot)."""
    h, w = img.shape
    n, nb = len(kp), f.descriptor_bytes()
    d_img, pitch = upload(torch, ref.pitched(img, 7))
    d_depth, dpitch = upload(torch, ref.pitched(depth, 5))
    d_kp = upload_kp(torch, kp)
    desc = torch.full((n + 1, nb), SENTINEL, dtype=torch.uint8, device="cuda:0")
    xyz = torch.full((n + 1, 12), SENTINEL, dtype=torch.uint8, device="cuda:0")
    out = torch.full((n + 1, KSZ), SENTINEL, dtype=torch.uint8, device="cuda:0")
    slot, rows = f.extract_keyframe_depth_device(d_img.data_ptr(), w, h, pitch, d_kp.data_ptr(), d_depth.data_ptr(),
                                                 _abi.depth_format_of(depth), dpitch, n, cam, desc.data_ptr(), xyz.data_ptr(),
                                                 out.data_ptr())
    torch.cuda.synchronize()
    desc, xyz, out = (t.cpu().numpy() for t in (desc, xyz, out))
    assert 0 <= rows <= n and (desc[rows:] == SENTINEL).all() and (xyz[rows:] == SENTINEL).all() and (out[rows:] == SENTINEL).all()
    return (desc[:rows].copy(), np.frombuffer(xyz[:rows].tobytes(), np.float32).reshape(rows, 3),
            np.frombuffer(out[:rows].tobytes(), dtype=_abi.KEYPOINT_DTYPE), slot)


def assert_same_keyframe(a, b):
    assert len(a[0]) == len(b[0])
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()


def check_points(out, depth, cam, filtered):
    """The 3D points of a keyframe are the restatement's for its keypoints; with the filter on every kept point is finite."""
    want = ref.keypoints3d_depth(out[2], depth, cam)
    assert out[1].tobytes() == want.tobytes()
    if filtered:
        assert np.isfinite(out[1]).all()


@pytest.mark.parametrize("dam", [1, 0])
@pytest.mark.parametrize("ftype,fmt", [(6, "u16"), (4, "f32"), (8, "f32"), (5, "u16")])
def test_single_call_equals_the_explicit_chain(ftype, fmt, dam):
    import torch
    img, depth = frame(60 + ftype, FORMATS[fmt])
    cam = ref.camera(W, H, local=(ftype in (4, 5)), min_depth=LIMITS[0], max_depth=LIMITS[1])
    det = _abi.detector_params(MAXF)
    fa, fb = finder_of(ftype), finder_of(ftype)
    try:
        fa.depth_set_params(_abi.depth_params(dam))
        assert fa.depth_get_params().depth_as_mask == dam and fb.depth_get_params().depth_as_mask == 1
        got = fa.get_features_and_descriptor_depth(ref.pitched(img, 7), ref.pitched(depth, 5), cam, det)
        mask = ref.depth_mask(depth, *LIMITS) if dam else None
        corners = restated_corners(img, mask, ftype, MAXF)
        want = chain(fb, torch, img, depth, corners, cam)
        print("type %d, DepthAsMask %d: %d corners, %d rows" % (ftype, dam, len(corners), len(want[0])))
        assert len(corners) >= 20 and len(want[0]) >= 5 and len(want[0]) < len(corners)
        assert_same_keyframe(got, want)
        assert got[3] == want[3] == 0 and fa.store_size() == fb.store_size() == 1
        check_points(got, depth, cam, True)
        if dam:                                             # every kept corner lies on the mask
            assert (mask[corners["y"].astype(int), corners["x"].astype(int)] != 0).all()
        ra, rb = fa.verify_pairs([0], [0]), fb.verify_pairs([0], [0])      # the store slots, through the verification path
        assert ra.tobytes() == rb.tobytes()
    finally:
        fa.close()
        fb.close()


@pytest.mark.parametrize("ftype,fmt", [(2, "u16"), (0, "f32"), (1, "u16")])
def test_types_with_their_own_detector_run_without_the_mask(ftype, fmt):
    import torch
    img, depth = frame(70 + ftype, FORMATS[fmt])
    cam = ref.camera(W, H, min_depth=LIMITS[0], max_depth=LIMITS[1])
    det = _abi.detector_params(MAXF)
    fa, fb = finder_of(ftype), finder_of(ftype)
    try:
        before = state(fa)
        with pytest.raises(lib.SepfinderError) as e:        # Vis/DepthAsMask 1 (a fresh handle): refused, nothing changes
            fa.get_features_and_descriptor_depth(img, depth, cam, det)
        assert e.value.code == _abi.SF_EINVAL and "DepthAsMask" in str(e.value) and "not built" in str(e.value)
        assert "sf_depth_set_params" in str(e.value) and state(fa) == before
        fa.depth_set_params(_abi.depth_params(0))
        got = fa.get_features_and_descriptor_depth(ref.pitched(img, 7), ref.pitched(depth, 5), cam, det)
        corners = device_corners(fb, torch, img, MAXF)
        want = chain(fb, torch, img, depth, corners, cam)
        print("type %d: %d keypoints, %d rows" % (ftype, len(corners), len(want[0])))
        assert len(want[0]) >= 3
        assert_same_keyframe(got, want)
        check_points(got, depth, cam, True)
        assert fa.store_size() == fb.store_size() == 1
    finally:
        fa.close()
        fb.close()


@pytest.mark.parametrize("front", ["roi", "grid", "roi+grid+subpix"])
@pytest.mark.parametrize("ftype", [6, 4])
def test_roi_and_grid_crop_the_mask_like_the_image(ftype, front):
    import torch
    img, depth = frame(80 + ftype, U16 if ftype == 6 else F32M)
    cam = ref.camera(W, H, min_depth=LIMITS[0], max_depth=LIMITS[1])
    det = _abi.detector_params(MAXF)
    roi = (0.1, 0.0, 0.2, 0.0) if "roi" in front else (0.0, 0.0, 0.0, 0.0)
    grid = (2, 2) if "grid" in front else (1, 1)
    fa, fb = finder_of(ftype), finder_of(ftype)
    try:
        fa.front_set_params(_abi.front_params(roi, 3, 4 if "subpix" in front else 0, 0.02))
        fa.grid_set_params(_abi.grid_params(*grid))
        got = fa.get_features_and_descriptor_depth(img, depth, cam, det)
        mask = ref.depth_mask(depth, *LIMITS)
        corners = restated_corners(img, mask, ftype, MAXF, grid, roi)
        plain = restated_corners(img, None, ftype, MAXF, grid, roi)
        assert len(corners) >= 20 and corners.tobytes() != plain.tobytes()
        if "subpix" in front:                               # the refinement moves x and y on the device: the existing call, on fb
            d_img = torch.from_numpy(np.array(img)).to("cuda:0")
            d_kp = upload_kp(torch, corners)
            fb.corner_subpix_device(d_img.data_ptr(), W, H, W, d_kp.data_ptr(), len(corners), 3, 4, 0.02)
            torch.cuda.synchronize()
            corners = np.frombuffer(d_kp.cpu().numpy().tobytes(), dtype=_abi.KEYPOINT_DTYPE)
        want = chain(fb, torch, img, depth, corners, cam)
        print("type %d, %s: %d corners (%d without the mask), %d rows" % (ftype, front, len(corners), len(plain), len(want[0])))
        assert len(want[0]) >= 5
        assert_same_keyframe(got, want)
        check_points(got, depth, cam, True)
    finally:
        fa.close()
        fb.close()


@pytest.mark.parametrize("ftype", [6, 4, 8])
def test_without_mask_and_limits_rows_and_keypoints_are_the_stereo_calls(ftype):
    """The tie to existing behaviour: depth_as_mask 0 and both depth limits 0 -- descriptor rows and keypoints equal
    sf_get_features_and_descriptor on the same left image with any right image; only xyz differs."""
    img, depth = frame(90 + ftype, F32M)
    right = ref.image(W, H, 7)
    cam = ref.camera(W, H)
    det = _abi.detector_params(MAXF)
    fa, fb = finder_of(ftype), finder_of(ftype)
    try:
        fa.depth_set_params(_abi.depth_params(0))
        got = fa.get_features_and_descriptor_depth(img, depth, cam, det)
        stereo_cam = _abi.stereo_camera(cam.fx, cam.fy, cam.cx, cam.cy, 0.1)
        want = fb.get_features_and_descriptor(img, right, stereo_cam, det)
        assert len(got[0]) == len(want[0]) >= 20
        assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert got[1].tobytes() != want[1].tobytes()
        check_points(got, depth, cam, False)
        assert np.isfinite(got[1]).any()
    finally:
        fa.close()
        fb.close()


def colour(gray):
    """A camera image whose gray plane is not the input's: red and green carry it, blue its negative."""
    return np.stack([gray, gray, 255 - gray], axis=2)


@pytest.mark.parametrize("ftype,grid", [(6, (2, 2)), (4, (1, 1))])
def test_interleaved_stereo_and_depth_calls_on_one_handle_equal_fresh_handles(ftype, grid):
    """The stereo and the depth host calls are one path: they share the handle's image planes, colour source, counts and
    response buffer.  Four calls in turn on one handle, each the bytes of the same call on a fresh handle."""
    img, d16 = frame(60 + ftype, U16)
    d32 = frame(60 + ftype, F32M)[1]
    right = np.ascontiguousarray(np.roll(img, -3, axis=1))
    cam = ref.camera(W, H, min_depth=LIMITS[0], max_depth=LIMITS[1])
    stereo_cam = _abi.stereo_camera(cam.fx, cam.fy, cam.cx, cam.cy, 0.1)
    det = _abi.detector_params(200)
    calls = [
        lambda f: f.get_features_and_descriptor_u8(colour(img), colour(right), _abi.SF_IMAGE_RGB8, stereo_cam, det),
        lambda f: f.get_features_and_descriptor_depth(img, d16, cam, det, _abi.SF_IMAGE_MONO8),
        lambda f: f.get_features_and_descriptor(img, right, stereo_cam, det),
        lambda f: f.get_features_and_descriptor_depth(colour(img), d32, cam, det, _abi.SF_IMAGE_RGB8),
    ]

    def fresh():
        f = finder_of(ftype)
        f.grid_set_params(_abi.grid_params(*grid))
        assert f.depth_get_params().depth_as_mask == 1
        return f

    fa = fresh()
    try:
        for i, call in enumerate(calls):
            got = call(fa)
            fb = fresh()
            try:
                want = call(fb)
            finally:
                fb.close()
            print("type %d, grid %d x %d, call %d: %d rows" % (ftype, grid[0], grid[1], i, len(want[0])))
            assert len(want[0]) >= 5
            assert_same_keyframe(got, want)
            assert got[3] == i and want[3] == 0
        assert fa.store_size() == len(calls)
    finally:
        fa.close()


# ---- the batch forms -----------------------------------------------------------------------------------------------------
def pack_planes(torch, planes, pitch, stride):
    """n 2-D arrays of one shape and dtype as one device buffer: rows `pitch` bytes, planes `stride` bytes apart."""
    h, w = planes[0].shape
    buf = np.full((len(planes), stride), 0xA5, np.uint8)
    for i, p in enumerate(planes):
        np.lib.stride_tricks.as_strided(buf[i].view(p.dtype), shape=(h, w), strides=(pitch, p.itemsize))[...] = p
    return torch.from_numpy(buf).to("cuda:0")


def batch_outputs(torch, n, maxf, nb):
    return (torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0"),
            torch.full((n * maxf + 1, nb), SENTINEL, dtype=torch.uint8, device="cuda:0"),
            torch.full((n * maxf + 1, 12), SENTINEL, dtype=torch.uint8, device="cuda:0"),
            torch.full((n * maxf + 1, KSZ), SENTINEL, dtype=torch.uint8, device="cuda:0"))


def read_batch(outs, n, maxf):
    rows, desc, xyz, kp = (t.cpu().numpy() for t in outs)
    assert rows[n] == -7 and (desc[n * maxf:] == SENTINEL).all() and (xyz[n * maxf:] == SENTINEL).all() and (kp[n * maxf:] == SENTINEL).all()
    res = []
    for i in range(n):
        r = int(rows[i])
        assert 0 <= r <= maxf
        blk = slice(i * maxf, (i + 1) * maxf)
        for a in (desc[blk], xyz[blk], kp[blk]):
            assert (a[r:] == SENTINEL).all(), "keyframe %d: written past its %d rows" % (i, r)
        res.append((desc[blk][:r].copy(), np.frombuffer(xyz[blk][:r].tobytes(), np.float32).reshape(r, 3),
                    np.frombuffer(kp[blk][:r].tobytes(), dtype=_abi.KEYPOINT_DTYPE)))
    return res


def batch_frames(fmt):
    """Three frames whose depths differ; the one in the middle has no valid depth."""
    return [frame(110, fmt), frame(111, fmt, dead=True), frame(112, fmt)]


@pytest.mark.parametrize("ftype,fmt,dam", [(6, "u16", 1), (4, "f32", 1), (2, "u16", 0), (1, "f32", 0), (6, "f32", 0)])
def test_batch_equals_three_single_calls(ftype, fmt, dam):
    import torch
    frames = batch_frames(FORMATS[fmt])
    n, elem = len(frames), 2 if fmt == "u16" else 4
    cam = ref.camera(W, H, local=True, min_depth=LIMITS[0], max_depth=LIMITS[1])
    det = _abi.detector_params(MAXF)
    fa, fb = finder_of(ftype), finder_of(ftype)
    try:
        for f in (fa, fb):
            f.depth_set_params(_abi.depth_params(dam))
        if ftype == 1:
            fa.debug_sift_batch_chunk(2)                    # two chunks: 2 + 1 images
        singles = [fb.get_features_and_descriptor_depth(img, depth, cam, det) for img, depth in frames]
        pitch, dpitch = W + 7, (W + 5) * elem
        stride, dstride = pitch * H + 33, dpitch * H + 12 * elem
        d_img = pack_planes(torch, [f[0] for f in frames], pitch, stride)
        d_depth = pack_planes(torch, [f[1] for f in frames], dpitch, dstride)
        outs = batch_outputs(torch, n, MAXF, fa.descriptor_bytes())
        first = fa.get_features_and_descriptor_depth_batch_device(d_img.data_ptr(), d_depth.data_ptr(), FORMATS[fmt], n, W, H, pitch,
                                                                  stride, dpitch, dstride, cam, det, *(t.data_ptr() for t in outs))
        torch.cuda.synchronize()
        got = read_batch(outs, n, MAXF)
        print("type %d: rows %s" % (ftype, [len(g[0]) for g in got]))
        assert first == 0 and fa.store_size() == fb.store_size() == n
        assert len(got[0][0]) >= 3 and len(got[2][0]) >= 3 and len(got[1][0]) == 0     # no valid depth: the filter drops every row
        for g, s in zip(got, singles):
            assert_same_keyframe(g, s)
        slots = list(range(n))
        assert fa.verify_pairs(slots, slots[::-1]).tobytes() == fb.verify_pairs(slots, slots[::-1]).tobytes()
        assert fa.get_features_and_descriptor_depth_batch_device(None, None, FORMATS[fmt], 0, W, H, pitch, stride, dpitch, dstride, cam,
                                                                 det) == n          # n = 0: the next slot, nothing touched
    finally:
        fa.close()
        fb.close()


def test_add_keyframes_depth_batch_gives_the_single_calls_slots_and_the_networks_rows():
    import torch
    from oracle import netvlad_torch
    from tests import image_ref
    from tests.test_gpu_image import colourise
    RGB8 = _abi.SF_IMAGE_RGB8
    n, dims = 2, 128
    frames = [frame(120, U16), frame(121, U16)]
    cam = ref.camera(W, H, min_depth=LIMITS[0], max_depth=LIMITS[1])
    det = _abi.detector_params(MAXF)
    weights = netvlad_torch.random_weights(3, clusters=64, pca_dim=512)
    fa, fb = _finder(), _finder()
    try:
        for f in (fa, fb):
            f.netvlad_load(weights)
        colour = [np.ascontiguousarray(colourise(img, 5 + i, RGB8)) for i, (img, _) in enumerate(frames)]
        pitch, dpitch = 3 * W + 5, (W + 3) * 2
        stride, dstride = pitch * H + 64, dpitch * H + 8
        buf = np.zeros((n, stride), np.uint8)
        for i, c in enumerate(colour):
            np.lib.stride_tricks.as_strided(buf[i], shape=(H, W, 3), strides=(pitch, 3, 1))[...] = c
        d_rgb = torch.from_numpy(buf).to("cuda:0")
        d_depth = pack_planes(torch, [f[1] for f in frames], dpitch, dstride)
        outs = batch_outputs(torch, n, MAXF, 32)
        first, row = fa.add_keyframes_depth_batch_device(d_rgb.data_ptr(), RGB8, d_depth.data_ptr(), U16, n, W, H, pitch, stride, dpitch,
                                                         dstride, cam, det, *(t.data_ptr() for t in outs))
        torch.cuda.synchronize()
        assert (first, row) == (0, 0) and fa.store_size() == n and fa.nn_sizes() == (n, 0)
        got = read_batch(outs, n, MAXF)
        # handle B: the single call on the colour images, and the network's rows appended by hand
        singles = [fb.get_features_and_descriptor_depth(c, depth, cam, det, image_format=RGB8) for c, (_, depth) in zip(colour, frames)]
        gray = [fb.get_features_and_descriptor_depth(image_ref.gray(c, RGB8, 0), depth, cam, det) for c, (_, depth) in zip(colour, frames)]
        d_desc = torch.zeros((n, dims), dtype=torch.float32, device="cuda:0")
        fb.netvlad_infer_u8_batch_device(d_rgb.data_ptr(), RGB8, n, W, H, pitch, stride, d_desc.data_ptr(), dims)
        fb.store_clear()
        for c, (_, depth) in zip(colour, frames):
            fb.get_features_and_descriptor_depth(c, depth, cam, det, image_format=RGB8)
        fb.nn_append_local_device(d_desc.data_ptr(), n, dims)
        torch.cuda.synchronize()
        for g, s, m in zip(got, singles, gray):
            assert len(g[0]) >= 5
            assert_same_keyframe(g, s)
            assert_same_keyframe(s, m)                      # the colour image is converted as the _u8 call converts it
        rng = np.random.default_rng(2)
        recv = d_desc.cpu().numpy().astype(np.float64) + 1e-5 * rng.normal(size=(n, dims))
        for f in (fa, fb):
            f.nn_append_received(recv)
        ma, mb = fa.nn_find_matches(), fb.nn_find_matches()
        assert ma.tobytes() == mb.tobytes()
        (da, ia), (db, ib) = fa.nn_last_row_minima(), fb.nn_last_row_minima()
        assert da.tobytes() == db.tobytes() and ia.tobytes() == ib.tobytes()   # the NN rows are the network's
        assert fa.verify_pairs([0, 1], [1, 0]).tobytes() == fb.verify_pairs([0, 1], [1, 0]).tobytes()
    finally:
        fa.close()
        fb.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _refused(f, call, needle=None, codes=(_abi.SF_EINVAL,)):
    before = state(f)
    with pytest.raises(lib.SepfinderError) as e:
        call()
    assert e.value.code in codes, str(e.value)
    text = str(e.value).split(": ", 1)[1]
    assert len(text) > 10 and (needle is None or needle in text), str(e.value)
    assert state(f) == before
    return text


def test_refusals_leave_everything_as_it_was():
    import torch
    from oracle import netvlad_torch
    img, depth = frame(130, U16)
    cam = ref.camera(W, H)
    f = _finder()
    try:
        f.netvlad_load(netvlad_torch.random_weights(3, clusters=64, pca_dim=512))
        f.get_features_and_descriptor_depth(img, depth, cam)                  # one keyframe, one local row: a state to keep
        f.nn_append_local(np.eye(1, 128))
        d_img = torch.from_numpy(np.array(img)).to("cuda:0")
        d_rgb = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda:0")
        d_depth = torch.zeros((2 * H * W * 4,), dtype=torch.uint8, device="cuda:0")
        d_mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
        d_kp = torch.zeros((64, KSZ), dtype=torch.uint8, device="cuda:0")
        d_xyz = torch.zeros((64, 3), dtype=torch.float32, device="cuda:0")
        pi, pd, pm, pk, px, pr = (t.data_ptr() for t in (d_img, d_depth, d_mask, d_kp, d_xyz, d_rgb))
        # sf_depth_set_params: any other value
        for v in (2, -1, 255):
            _refused(f, lambda: f.depth_set_params(_abi.depth_params(v)), "DepthAsMask")
        # every call: an unknown depth format, a depth pitch below a row, a pitch or stride that is no multiple of the element
        calls = {
            "sf_depth_mask_device": lambda fmt=U16, dp=2 * W, ds=2 * W * H, n=2: f.depth_mask_device(pd, fmt, W, H, dp, ds, n, 0.0, 0.0, pm, W, W * H),
            "sf_depth_points_device": lambda fmt=U16, dp=2 * W, ds=0, n=1: f.depth_points_device(pd, fmt, W, H, dp, pk, 8, cam, px),
            "sf_extract_keyframe_depth_device": lambda fmt=U16, dp=2 * W, ds=0, n=1: f.extract_keyframe_depth_device(pi, W, H, W, pk, pd, fmt, dp, 8, cam),
            "sf_get_features_and_descriptor_depth_batch_device": lambda fmt=U16, dp=2 * W, ds=2 * W * H, n=2: f.get_features_and_descriptor_depth_batch_device(
                pi, pd, fmt, n, W, H, W, W * H if n > 1 else W * H, dp, ds, cam),
            "sf_add_keyframes_depth_batch_device": lambda fmt=U16, dp=2 * W, ds=2 * W * H, n=2: f.add_keyframes_depth_batch_device(
                pr, 0, pd, fmt, n, W, H, 3 * W, 3 * W * H, dp, ds, cam),
        }
        for name, call in calls.items():
            assert name in _refused(f, lambda: call(fmt=2), "format")
            assert name in _refused(f, lambda: call(fmt=-1), "format")
            assert name in _refused(f, lambda: call(dp=2 * W - 2), "depth_pitch")
            assert name in _refused(f, lambda: call(fmt=F32M, dp=4 * W - 4), "depth_pitch")
            assert name in _refused(f, lambda: call(dp=2 * W + 1), "multiple")
            assert name in _refused(f, lambda: call(fmt=F32M, dp=4 * W + 2), "multiple")
            if "batch" in name or "mask" in name:
                assert name in _refused(f, lambda: call(ds=2 * W * H + 1), "multiple")
                assert name in _refused(f, lambda: call(ds=2 * W * H - 2), "stride")
        rows, slot = lib.C.c_int32(), lib.C.c_int32()
        host_depth = np.ascontiguousarray(depth)
        for fmt, dp, needle in ((2, 2 * W, "format"), (U16, 2 * W - 2, "depth_pitch"), (U16, 2 * W + 1, "multiple")):
            before = state(f)
            rc = f._L.sf_get_features_and_descriptor_depth(f._h, img.ctypes.data, 2, host_depth.ctypes.data, fmt, W, H, W, dp,
                                                           lib.C.byref(cam), None, None, None, None, 0, lib.C.byref(rows), lib.C.byref(slot))
            text = f._L.sf_last_error(f._h).decode()
            assert rc == _abi.SF_EINVAL and needle in text and "sf_get_features_and_descriptor_depth" in text and state(f) == before
        # missing pointers, a malformed image or mask
        _refused(f, lambda: f.depth_mask_device(None, U16, W, H, 2 * W, 0, 1, 0.0, 0.0, pm, W, 0), "sf_depth_mask_device")
        _refused(f, lambda: f.depth_mask_device(pd, U16, W, H, 2 * W, 0, 1, 0.0, 0.0, pm, W - 1, 0), "mask")
        _refused(f, lambda: f.depth_points_device(pd, U16, W, H, 2 * W, None, 8, cam, px), "sf_depth_points_device")
        _refused(f, lambda: f.detect_corners_masked_device(pi, W, H, W, None, W, 100, 0.01, 3.0, pk, 64), "sf_detect_corners_masked_device")
        _refused(f, lambda: f.detect_corners_masked_device(pi, W, H, W, pm, W - 1, 100, 0.01, 3.0, pk, 64), "mask_pitch")
        _refused(f, lambda: f.detect_fast_masked_device(pi, W, H, W, None, W, 100, pk, 64), "sf_detect_fast_masked_device")
        _refused(f, lambda: f.detect_fast_masked_device(pi, W, H, W, pm, 3, 100, pk, 64), "mask_pitch")
        _refused(f, lambda: f.detect_corners_masked_device(pi, W, H, W, pm, W, 100, 0.0, 3.0, pk, 64), "qualityLevel")
        _refused(f, lambda: f.extract_keyframe_depth_device(pi, W, H, W, pk, None, U16, 2 * W, 8, cam), "sf_extract_keyframe_depth_device")
        _refused(f, lambda: f.get_features_and_descriptor_depth_batch_device(None, pd, U16, 2, W, H, W, W * H, 2 * W, 2 * W * H, cam), "images")
        _refused(f, lambda: f.get_features_and_descriptor_depth_batch_device(pi, pd, U16, 2, W, H, W, W * H - 1, 2 * W, 2 * W * H, cam), "stride")
        _refused(f, lambda: f.add_keyframes_depth_batch_device(pr, 3, pd, U16, 2, W, H, 3 * W, 3 * W * H, 2 * W, 2 * W * H, cam), "format")
        _refused(f, lambda: f.add_keyframes_depth_batch_device(pr, 0, pd, U16, 2, W, H, 3 * W - 1, 3 * W * H, 2 * W, 2 * W * H, cam),
                 "sf_add_keyframes_depth_batch_device")
        _refused(f, lambda: f.get_features_and_descriptor_depth(img, depth, cam, _abi.detector_params(0)), "max_features", (_abi.SF_ERANGE,))
        # Vis/DepthAsMask 1 under a type whose detector takes no mask: every call that detects
        f.set_feature_type_orb()
        for name, call in (("sf_get_features_and_descriptor_depth", lambda: f.get_features_and_descriptor_depth(img, depth, cam)),
                           ("sf_get_features_and_descriptor_depth_batch_device", lambda: calls["sf_get_features_and_descriptor_depth_batch_device"]()),
                           ("sf_add_keyframes_depth_batch_device", lambda: calls["sf_add_keyframes_depth_batch_device"]())):
            text = _refused(f, call, "DepthAsMask")
            assert name in text and "not built" in text and "sf_depth_set_params" in text
        f.set_feature_type(6)
        # no model: the batch call with the network refuses before anything is touched
        g = _finder()
        try:
            _refused(g, lambda: g.add_keyframes_depth_batch_device(pr, 0, pd, U16, 2, W, H, 3 * W, 3 * W * H, 2 * W, 2 * W * H, cam), "model")
        finally:
            g.close()
        assert state(f) == (1, (1, 0), 6, 1)
        # and the calls the refusals stood in front of do run
        first, row = f.add_keyframes_depth_batch_device(pr, 0, pd, U16, 2, W, H, 3 * W, 3 * W * H, 2 * W, 2 * W * H, cam)
        torch.cuda.synchronize()
        assert (first, row) == (1, 1) and f.store_size() == 3 and f.nn_sizes() == (3, 0)
    finally:
        f.close()
