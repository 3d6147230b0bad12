"""Rectification of raw camera images, the part that needs no GPU: checks that the NumPy restatement the GPU tests compare
with (tests/rectify_ref.py) IS rectification and not merely consistent with itself -- identities, shifts with known answers,
the rounding rules on planted values, the model against cv::undistortPoints' iteration and the taps against an independent
interpolator -- and the host side of the C-ABI: the block's layout, the refusals, the plan's inverse, the camera of the
rectified pair."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import image_ref
from tests import rectify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_rectify_plan_create", "sf_rectify_plan_from_maps", "sf_rectify_plan_count", "sf_rectify_plan_get",
       "sf_rectify_plan_clear", "sf_rectify_maps_device", "sf_image_rectify_device", "sf_stereo_camera_from_info"]
K0 = [[310.5, 0, 47.25], [0, 305.0, 30.5], [0, 0, 1]]


def abi_info(info):
    return _abi.camera_info(info["width"], info["height"], info["K"], info["D"], info["R"], info["P"], info["model"],
                            info["out_width"], info["out_height"])


def random_image(seed, h, w, ch):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)


# ---- the restatement is rectification --------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3])
def test_identity_plan_returns_the_image(ch):
    img = random_image(1, 61, 97, ch)
    info = ref.camera_info(97, 61, K0)
    mx, my = ref.maps(info)
    assert np.array_equal(mx, np.tile(np.arange(97, dtype=np.float32), (61, 1)))
    assert np.array_equal(my, np.tile(np.arange(61, dtype=np.float32)[:, None], (1, 97)))
    assert np.array_equal(ref.rectify(img, info), img)


@pytest.mark.parametrize("ch", [1, 3])
def test_integer_shift_of_the_principal_point(ch):
    """P's cx moved by +3: output column j shows source column j - 3, zeros come in from the left."""
    img = random_image(2, 61, 97, ch)
    P = np.hstack([np.array(K0), np.zeros((3, 1))])
    P[0, 2] += 3.0
    out = ref.rectify(img, ref.camera_info(97, 61, K0, P=P))
    assert np.array_equal(out[:, 3:], img[:, :-3]) and not out[:, :3].any()


def test_quarter_pixel_shift_blends_two_neighbours():
    """P's cx moved by +0.25: output column j looks at source x = j - 0.25, i.e. ix = j - 1 with a = 24: the pixel is
    (8 p[j - 1] + 24 p[j] + 16) >> 5 -- in the issue's words (24 p[c] + 8 p[c + 1] + 16) >> 5 with c = j and the
    neighbour c + 1 standing for the one on the side the image moved from, j - 1."""
    img = random_image(3, 61, 97, 1)
    P = np.hstack([np.array(K0), np.zeros((3, 1))])
    P[0, 2] += 0.25
    info = ref.camera_info(97, 61, K0, P=P)
    sx, sy = ref.fixed(*ref.maps(info))
    assert np.array_equal(sx[0], 32 * np.arange(97) - 8) and np.array_equal(sy[:, 0], 32 * np.arange(61))
    out = ref.rectify(img, info)
    p = img.astype(np.int32)
    assert np.array_equal(out[:, 1:], ((24 * p[:, 1:] + 8 * p[:, :-1] + 16) >> 5).astype(np.uint8))
    assert np.array_equal(out[:, 0], ((24 * p[:, 0] + 16) >> 5).astype(np.uint8))          # the left neighbour is outside


def test_ties_round_to_the_even_neighbour():
    k = np.array([0, 1, 2, 3, 100, 101, -1, -2, -3, -4, -101, -100, 40000, -40001], np.int64)
    mapx = ((2 * k + 1) / 64.0).astype(np.float32)
    assert np.array_equal(mapx.astype(np.float64) * 32.0, k + 0.5)                         # planted exactly
    sx, sy = ref.fixed(mapx[None], np.zeros_like(mapx)[None])
    want = np.where(k % 2 == 0, k, k + 1)                                                  # (also for negative k: -1 -> 0, -3 -> -2)
    assert np.array_equal(sx[0], want) and (sx[0] % 2 == 0).all() and not sy.any()
    assert (np.abs(sx[0] - (k + 0.5)) == 0.5).all()


def test_negative_coordinates_shift_and_mask_as_floor():
    """Map values in (-2, 0): ix = floor(x) through the arithmetic shift, a = the fraction above it through the mask."""
    img = random_image(4, 5, 7, 1)
    p = img.astype(np.int64)
    mapx = np.array([[-0.25, -1.0, -1.5, -0.25, 2.0, -0.5]], np.float32)
    mapy = np.array([[0.0, 0.0, 1.0, -0.5, -0.75, -1.25]], np.float32)
    sx, sy = ref.fixed(mapx, mapy)
    assert sx.tolist() == [[-8, -32, -48, -8, 64, -16]] and sy.tolist() == [[0, 0, 32, -16, -24, -40]]
    assert (sx >> 5).tolist() == [[-1, -1, -2, -1, 2, -1]] and (sx & 31).tolist() == [[24, 0, 16, 24, 0, 16]]
    assert (sy >> 5).tolist() == [[0, 0, 1, -1, -1, -2]] and (sy & 31).tolist() == [[0, 0, 0, 16, 8, 24]]
    out = ref.rectify_maps(img, mapx, mapy)[0]
    want = [(32 * 24 * 32 * p[0, 0] + 16384) >> 15,          # one tap: (0, 0) with a = 24, b = 0
            0,                                               # ix = -1, a = 0: the inside tap has weight 0
            0,                                               # ix = -2: both columns outside
            (32 * 24 * 16 * p[0, 0] + 16384) >> 15,          # one tap: left and top neighbours outside
            (32 * 32 * 8 * p[0, 2] + 16384) >> 15,           # top edge: (2, -1) outside, (2, 0) with b = 8
            0]                                               # iy = -2: both rows outside
    assert out.tolist() == [int(v) for v in want]
    two = ref.rectify_maps(img, np.array([[1.5]], np.float32), np.array([[-0.5]], np.float32))   # two taps of row 0
    assert int(two[0, 0]) == (32 * 16 * 16 * (p[0, 1] + p[0, 2]) + 16384) >> 15


def test_non_finite_and_huge_map_values_give_zero():
    img = np.full((9, 9), 200, np.uint8)
    bad = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 2.0 ** 25, 3.0], np.float32)
    for mapx, mapy in ((bad[None], np.full((1, 7), 3.0, np.float32)), (np.full((1, 7), 3.0, np.float32), bad[None])):
        sx, sy = ref.fixed(mapx, mapy)
        assert (sx[0, :6] == ref.INVALID).all() and (sy[0, :6] == ref.INVALID).all() and (sx[0, 6], sy[0, 6]) == (96, 96)
        assert ref.rectify_maps(img, mapx, mapy).tolist() == [[0, 0, 0, 0, 0, 0, 200]]


def undistort_points(u, v, info):
    """cv::undistortPoints with R and P, as remembered: normalise by K, remove the distortion by the fixed-point iteration
    x <- (x0 - dx(x)) / kr(x) (here to a step below 1e-12), rotate by R, project by P.  float64."""
    K, P, R = info["K"], info["P"], info["R"]
    k1, k2, p1, p2, k3, k4, k5, k6 = ref.plan(info)[2]
    x0, y0 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for it in range(2000):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        xn, yn = (x0 - dx) * icdist, (y0 - dy) * icdist
        step = max(np.abs(xn - x).max(), np.abs(yn - y).max())
        x, y = xn, yn
        if step < 1e-12:
            break
    assert step < 1e-12, step
    q = P[:, :3] @ R @ np.stack([x, y, np.ones_like(x)])
    return q[0] / q[2], q[1] / q[2]


@pytest.mark.parametrize("kind", ["barrel", "rational"])
def test_the_model_inverts_to_the_output_pixel(kind):
    """The map sends output pixel (j, i) to the raw pixel that undistorts back to (j, i).  Tolerance 1e-6 px: the iteration
    stops at a 1e-12 step in normalised coordinates (x focal length: 1e-9 px) and the comparison uses the float64 map value,
    before its rounding to float32 (which alone would be up to 2^-11 px at these magnitudes)."""
    info = ref.case_info(kind, 752, 480)
    mx, my = ref.maps64(info)
    rng = np.random.default_rng(11)
    jj, ii = rng.integers(0, 752, 500), rng.integers(0, 480, 500)
    u, v = mx[ii, jj], my[ii, jj]
    assert np.abs(u - jj).max() > 3.0                                            # the distortion is visible
    assert not np.allclose(info["R"], np.eye(3), atol=1e-3)
    bj, bi = undistort_points(u, v, info)
    err = max(np.abs(bj - jj).max(), np.abs(bi - ii).max())
    print("%s: round trip within %.3g px" % (kind, err))
    assert err <= 1e-6
    m32 = ref.maps(info)
    assert np.abs(m32[0].astype(np.float64) - mx).max() <= 2.0 ** -11 and np.abs(m32[1].astype(np.float64) - my).max() <= 2.0 ** -11


def test_taps_against_scipy_at_the_quantised_coordinates():
    from scipy.ndimage import map_coordinates
    img = random_image(12, 61, 97, 1)
    info = ref.case_info("strong", 97, 61)
    sx, sy = ref.fixed(*ref.maps(info))
    assert 0.05 <= ref.border_share(sx, sy, 97, 61) <= 0.5
    got = ref.remap(img, sx, sy).astype(np.float64)
    # scipy's "constant" mode does not interpolate beyond the edges: a sample is cval as soon as its coordinate leaves
    # [0, n - 1], where upstream blends the border pixel with the zero beside it.  A ring of zeros around the image (and
    # coordinates moved by one) puts that blend inside scipy's image, so that EVERY output pixel is compared.
    padded = np.pad(img.astype(np.float64), 1)
    want = map_coordinates(padded, [sy / 32.0 + 1.0, sx / 32.0 + 1.0], order=1, mode="constant", cval=0.0)
    diff = np.abs(got - want)
    print("largest difference from scipy %.6f" % diff.max())
    assert diff.max() <= 0.5 + 1e-9
    inside = ref.taps(sx, sy, 97, 61)[3].all(axis=0)                              # and scipy on the image as it is agrees there
    plain = map_coordinates(img.astype(np.float64), [sy / 32.0, sx / 32.0], order=1, mode="constant", cval=0.0)
    assert np.abs(got - plain)[inside].max() <= 0.5 + 1e-9 and 0.5 < inside.mean() < 0.95


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("format", [image_ref.RGB8, image_ref.BGR8])
def test_fused_gray_is_the_gray_of_the_rectified_colour_image(format, rule):
    img = random_image(13, 61, 97, 3)
    info = ref.case_info("strong", 97, 61)
    rect = ref.rectify(img, info)
    g = ref.to_gray(rect, format, rule)
    assert np.array_equal(g, image_ref.gray(rect, format, rule)) and g.shape == (61, 97)
    # and it is NOT the rectification of the gray image: the two roundings do not commute everywhere
    assert (g != ref.rectify(image_ref.gray(img, format, rule), info)).any()


# ---- the host side of the C-ABI --------------------------------------------------------------------------------------
def test_header_abi_and_binding_agree(tmp_path):
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    exp = open(os.path.join(ROOT, "include", "sf_experimental.h")).read()
    for name in NEW + ["sf_rectify_check_info"]:
        assert hasattr(L, name) and name in lib.EXPORTED and getattr(L, name).argtypes is not None, name
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"\bsf_rectify_check_info\s*\(", exp)
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _abi.SF_ABI_VERSION == 8 and L.sf_abi_version() == 8
    for method in ("rectify_plan_create", "rectify_plan_from_maps", "rectify_plan_count", "rectify_plan_get",
                   "rectify_plan_clear", "rectify_maps_device", "image_rectify_device"):
        assert hasattr(lib.SeparatorFinder, method)
    fields = [name for name, _ in _abi.CameraInfo._fields_]
    src = tmp_path / "info.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sepfinder.h"\n'
                   'int main(void){printf("%zu %d %d %zu", sizeof(sf_camera_info), SF_MAX_RECTIFY_PLANS, (int)SF_OPT_RECTIFY_TABLE,'
                   " sizeof(sf_params));\n" +
                   "".join('printf(" %%zu", offsetof(sf_camera_info, %s));\n' % f for f in fields) +
                   'printf("\\n"); return 0;}\n')
    exe = tmp_path / "info"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_abi.CameraInfo), _abi.SF_MAX_RECTIFY_PLANS, _abi.SF_OPT_RECTIFY_TABLE, C.sizeof(_abi.Params)] + \
        [getattr(_abi.CameraInfo, f).offset for f in fields]
    assert got[0] == 328 and got[1] >= 64 and got[3] == 232


def refusals():
    """(name, block) of every block sf_rectify_plan_create refuses; the GPU test runs the same list through the call."""
    def make(**kw):
        info = ref.case_info("barrel", 320, 240)
        for key, (idx, val) in kw.items():
            if idx is None:
                info[key] = val
            else:
                info[key][idx] = val
        return info
    out = [("nan in K", make(K=((0, 2), np.nan))), ("inf in D", make(D=(1, np.inf))), ("nan in R", make(R=((1, 1), np.nan))),
           ("inf in P", make(P=((0, 3), -np.inf))), ("nan in an unused D", make(D=(7, np.nan))),
           ("fx 0 in K", make(K=((0, 0), 0.0))), ("fy < 0 in K", make(K=((1, 1), -400.0))),
           ("fx 0 in P", make(P=((0, 0), 0.0))), ("fy < 0 in P", make(P=((1, 1), -1.0))),
           ("skew", make(K=((0, 1), 0.5))),
           ("singular", make(R=(None, np.array([[1.0, 0, 0], [0, 1, 0], [1, 1, 0]])))),
           ("width 0", make(width=(None, 0))), ("height 8193", make(height=(None, 8193))),
           ("out_width -1", make(out_width=(None, -1))), ("out_height 8193", make(out_height=(None, 8193))),
           ("model 2", make(model=(None, 2))), ("model -1", make(model=(None, -1)))]
    reserved = abi_info(make())
    reserved.reserved = 1
    return [(name, abi_info(info), ref.check(info)) for name, info in out] + [("reserved", reserved, "reserved")]


def test_plan_validation_refuses_what_the_restatement_refuses():
    L = lib.load()
    cases = refusals()
    assert len(cases) == 18 and all(why for _, _, why in cases)                   # the restatement refuses each of them
    for name, block, _ in cases:
        assert L.sf_rectify_check_info(C.byref(block), None) == _abi.SF_EINVAL, name
        assert len(L.sf_last_error(None)) > 10, name
    for kind in ("barrel", "rational", "strong"):
        for side in (0, 1):
            info = ref.case_info(kind, 320, 240, 300, 200, side)
            rc, iR = lib.rectify_check_info(abi_info(info))
            assert rc == _abi.SF_OK and ref.check(info) is None
            assert np.array_equal(iR, ref.plan(info)[0])                          # the written-down order, bit for bit
            assert np.allclose(iR @ (info["P"][:, :3] @ info["R"]), np.eye(3), atol=1e-12)
    edge = ref.camera_info(8192, 1, K0, out_width=1, out_height=8192)
    assert lib.rectify_check_info(abi_info(edge))[0] == _abi.SF_OK


def test_stereo_camera_from_info():
    left, right = ref.case_info("barrel", 752, 480, side=0), ref.case_info("barrel", 752, 480, side=1)
    lt = np.arange(12, dtype=np.float32) / 7
    cam = lib.stereo_camera_from_info(abi_info(left), abi_info(right), lt)
    fx, fy, cx, cy, cx_right, baseline = ref.stereo_camera_from_info(left, right)
    assert abs(baseline - 0.11) < 1e-12
    want = [np.float32(v) for v in (fx, fy, cx, cy, cx_right, baseline)]
    assert [cam.fx, cam.fy, cam.cx, cam.cy, cam.cx_right, cam.baseline] == [float(v) for v in want]
    assert list(cam.local_transform) == lt.tolist() and (cam.min_depth, cam.max_depth) == (0.0, 0.0)
    ident = lib.stereo_camera_from_info(abi_info(left), abi_info(right))
    assert list(ident.local_transform) == np.eye(4, dtype=np.float32)[:3].ravel().tolist()
    # the left block as the right one has P[3] = 0: no baseline; exchanged signs: a negative one
    for bad_right in (left, dict(right, P=right["P"] * np.array([1, 1, 1, -1.0]))):
        assert ref.stereo_camera_from_info(left, bad_right) is None
        with pytest.raises(lib.SepfinderError) as e:
            lib.stereo_camera_from_info(abi_info(left), abi_info(bad_right))
        assert e.value.code == _abi.SF_EINVAL and "baseline" in str(e.value)


def test_finder_backend_rectify_is_off_by_default():
    from multi_robot_slam_separators_amd.data_handler import FinderBackend

    class Recorder:
        def __init__(self):
            self.calls = []

        def rectify_pair(self, left, right, fmt, pl, pr):
            self.calls.append(("rectify", fmt, pl, pr))
            return left + 1, right + 1

        def get_features_and_descriptor_u8(self, left, right, fmt, cam, det, flow):
            self.calls.append(("features", int(left[0, 0, 0]), int(right[0, 0, 0]), fmt))
            return "d", "x", "k", 5
    img = np.zeros((4, 6, 3), np.uint8)
    plain, rect = Recorder(), Recorder()
    assert FinderBackend(plain, cam=object()).rectify is None
    FinderBackend(plain, cam=object()).get_features_u8(img, img + 9)
    assert plain.calls == [("features", 0, 9, _abi.SF_IMAGE_RGB8)]
    be = FinderBackend(rect, cam=object(), rectify=(2, 3))
    assert be.get_features_u8(img, img + 9, _abi.SF_IMAGE_BGR8) == ("d", "x", "k") and be.slots == [5]
    assert rect.calls == [("rectify", _abi.SF_IMAGE_BGR8, 2, 3), ("features", 1, 10, _abi.SF_IMAGE_BGR8)]
