"""CPU: the NumPy restatement of cv::cornerSubPix and Feature2D::computeRoi (tests/subpix_ref.py) against what it has to
find -- the centre of a blurred saddle -- against its own branch report, and against a hand-computed ROI table; the
layout of sf_front_params."""
import ctypes as C
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from tests import extract_cases as ec
from tests import fast_ref
from tests import subpix_ref as ref


def saddle(tx, ty, size=41):
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    return np.clip(np.rint(128.0 + 100.0 * np.tanh((x - tx) / 1.2) * np.tanh((y - ty) / 1.2)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("tx,ty", [(20.3, 19.6), (20.5, 20.5), (19.75, 20.1)])
def test_saddle_centre_within_a_twentieth_of_a_pixel(tx, ty):
    """Bound 0.05 px: twice the worst error of the prototype (0.024, 0.001, 0.025 px on the three centres)."""
    xy, info = ref.corner_subpix(saddle(tx, ty), [(20.0, 20.0)], 3, 30, 0.02)
    e = float(np.hypot(float(xy[0, 0]) - tx, float(xy[0, 1]) - ty))
    print("saddle (%.2f, %.2f): found (%.4f, %.4f), error %.4f px, %d iterations, stop %s" % (
        tx, ty, xy[0, 0], xy[0, 1], e, info["iterations"][0], ref.STOP_NAMES[int(info["stop"][0])]))
    assert e <= 0.05
    assert not info["reverted"][0]


@functools.lru_cache(maxsize=None)
def stereo3_corners():
    left = np.ascontiguousarray(ec.make_stereo_pair(3)[0])
    kp = fast_ref.detect(left, 20, 1, 0)[:300]
    return left, np.stack([kp["x"], kp["y"]], axis=1)


@pytest.mark.parametrize("iterations", [5, 30])
def test_branches_on_real_corners(iterations):
    left, pts = stereo3_corners()
    xy, info = ref.corner_subpix(left, pts, 3, iterations, 0.02)
    eps, cap, rev = info["stop"] == ref.STOP_EPS, info["stop"] == ref.STOP_CAP, info["reverted"]
    print("iterations %d: eps stop %d (then reverted %d), iteration cap %d (then reverted %d), det %d, left %d" % (
        iterations, eps.sum(), (eps & rev).sum(), cap.sum(), (cap & rev).sum(), (info["stop"] == ref.STOP_DET).sum(),
        (info["stop"] == ref.STOP_LEFT).sum()))
    assert len(pts) == 300
    assert eps.sum() > 0 and cap.sum() > 0 and rev.sum() > 0
    assert (info["iterations"][cap] == iterations).all() and (info["iterations"] <= iterations).all()
    assert (xy != pts).any(axis=1).sum() > 100             # most corners do move
    assert (np.abs(xy - pts) <= 3.0).all()                 # the revert rule
    assert (xy[rev] == pts[rev]).all()


def test_det_branch_on_a_constant_image():
    img = np.full((40, 50), 93, np.uint8)
    xy, info = ref.corner_subpix(img, [(20.0, 20.0), (3.5, 7.25)], 3, 30, 0.02)
    assert (info["stop"] == ref.STOP_DET).all() and (info["iterations"] == 1).all()
    assert xy.tolist() == [[20.0, 20.0], [3.5, 7.25]]


def leaving_case():
    """A saddle whose centre lies just outside the left edge: a step from (1, 20) crosses x = 0."""
    return saddle(-1.0, 20.0), [(1.0, 20.0)]


def test_left_the_image_branch():
    img, pts = leaving_case()
    xy, info = ref.corner_subpix(img, pts, 3, 30, 0.02)
    print("leaving corner: (%.3f, %.3f) after %d iterations, reverted %d" % (xy[0, 0], xy[0, 1], info["iterations"][0],
                                                                              info["reverted"][0]))
    assert info["stop"][0] == ref.STOP_LEFT


ROI_TABLE = [
    # width, height, ratios {left, right, top, bottom} -> x, y, w, h (by hand, float32 products truncated)
    (752, 480, (0.0, 0.0, 0.0, 0.0), (0, 0, 752, 480)),
    (752, 480, (0.0, 0.1, 0.0, 0.0), (0, 0, 676, 480)),       # (int)(752.f - 75.2f): the float compound assignment
    (752, 480, (0.6, 0.5, 0.0, 0.0), (0, 0, 752, 480)),       # 0.6 < 1 - 0.5 and 0.5 < 1 - 0.6 are both false
    (752, 480, (0.25, 0.0, 0.5, 0.0), (188, 240, 564, 240)),
    (202, 170, (0.13, 0.2, 0.1, 0.15), (26, 17, 135, 127)),   # 26.26, 176 - 40.4 = 135.6, 17.0, 153 - 25.5 = 127.5
    (208, 170, (0.13, 0.2, 0.1, 0.15), (27, 17, 139, 127)),   # 27.04, 181 - 41.6 = 139.4
    (752, 480, (1.0, 0.0, 0.0, 0.0), (0, 0, 752, 480)),       # a ratio of 1 never passes r < 1 - other
    (752, 480, (0.0, 1.0, 0.0, 1.0), (0, 0, 752, 480)),
    (100, 100, (0.5, 0.25, 0.25, 0.5), (50, 25, 25, 25)),
]


@pytest.mark.parametrize("w,h,ratios,want", ROI_TABLE)
def test_compute_roi_table(w, h, ratios, want):
    assert ref.compute_roi(w, h, ratios) == want


def test_compute_roi_refusals():
    for bad in ((-0.1, 0, 0, 0), (0, 1.5, 0, 0), (0, 0, float("nan"), 0)):
        with pytest.raises(ValueError):
            ref.compute_roi(752, 480, bad)
    with pytest.raises(ValueError):                             # 752 * 0.499 = 375.2: x 375, w (int)(377 - 375.2) = 1
        ref.compute_roi(752, 480, (0.499, 0.499, 0.0, 0.0))
    with pytest.raises(ValueError):
        ref.compute_roi(5, 5, (0.3, 0.3, 0.3, 0.3))             # x 1, w (int)(4 - 1.5) = 2


def test_front_params_layout():
    assert C.sizeof(_abi.FrontParams) == 28
    assert _abi.FrontParams.roi_ratios.offset == 0 and _abi.FrontParams.subpix_win_size.offset == 16
    assert _abi.FrontParams.subpix_iterations.offset == 20 and _abi.FrontParams.subpix_eps.offset == 24
    p = _abi.front_params()
    assert list(p.roi_ratios) == [0.0] * 4 and (p.subpix_win_size, p.subpix_iterations) == (3, 0)
    assert p.subpix_eps == np.float32(0.02)


def test_taps_are_symmetric_and_peak_at_one():
    for win in (1, 3, 15):
        v = ref.taps(win)
        assert v[win] == 1.0 and (v == v[::-1]).all() and v[0] == np.float32(np.exp(-1.0))


def test_library_compute_roi_equals_the_restatement():
    """sf_compute_roi is pure host code: the table, the refusals and 2 000 random (size, ratios) against compute_roi."""
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    rng = np.random.default_rng(1)
    cases = [(w, h, r) for w, h, r, _ in ROI_TABLE] + [(752, 480, (0.499, 0.499, 0.0, 0.0)), (5, 5, (0.3, 0.3, 0.3, 0.3)),
                                                        (752, 480, (-0.1, 0.0, 0.0, 0.0)), (752, 480, (0.0, 0.0, float("nan"), 0.0))]
    for _ in range(2000):
        r = np.round(rng.uniform(0, 1, 4), 3) * rng.integers(0, 2, 4)
        cases.append((int(rng.integers(1, 2000)), int(rng.integers(1, 1500)), tuple(float(v) for v in r)))
    refused = 0
    for w, h, r in cases:
        out = (C.c_int32 * 4)()
        rc = L.sf_compute_roi(w, h, (C.c_float * 4)(*r), out)
        try:
            assert (rc, tuple(out)) == (_abi.SF_OK, ref.compute_roi(w, h, r)), (w, h, r)
        except ValueError:
            refused += 1
            assert rc == _abi.SF_EINVAL, (w, h, r)
    assert 4 <= refused < len(cases) // 2
