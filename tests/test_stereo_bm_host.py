"""CPU: the NumPy restatement of rtabmap's block-matching stereo correspondence (tests/stereo_bm_ref.py) against what it
has to find -- the planted disparity field of a synthetic pair -- against inputs whose answer is known by hand, and its
pyramid against the oracle's pyrDown; the layout of sf_stereo_params and the exports.  (The setters need a handle, and a
handle needs a device: what they refuse WITH a handle is in tests/test_gpu_stereo_bm.py; here, what they refuse without.)"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from oracle import pyoracle
from tests import extract_cases as ec
from tests import fast_ref
from tests import stereo_bm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_stereo_defaults", "sf_stereo_set_params", "sf_stereo_get_params", "sf_stereo_block_match_device"]


@functools.lru_cache(maxsize=None)
def stereo3():
    left, right, disp = ec.make_stereo_pair(3)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    return left, right, disp, fast_ref.detect(left, 20, 1, 0)[:300]


def test_pyramid_equals_the_oracles_pyr_down():
    left = stereo3()[0]
    for img, win, max_level in ((left, (15, 3), 5), (left[:171, :203], (7, 7), 15), (left[:50, :40], (3, 3), 5)):
        levels = ref.pyramid(img, win[0], win[1], max_level)
        assert len(levels) >= 3 and len(levels) <= max_level + 1
        for a, b in zip(levels[:-1], levels[1:]):
            assert b.tobytes() == pyoracle.pyr_down(a).tobytes() and b.shape == ((a.shape[0] + 1) // 2, (a.shape[1] + 1) // 2)
        nh, nw = (levels[-1].shape[0] + 1) // 2, (levels[-1].shape[1] + 1) // 2
        assert len(levels) == max_level + 1 or nw <= win[0] or nh <= win[1]        # the level-count rule of the LK path


def found_against_the_field(xy, st, kp, disp):
    """(corners with status 1, those within 0.5 px of the disparity field READ AT THE FOUND right-image position -- the
    generator defines the field over the right image --, the median error)."""
    ok = st == 1
    h, w = disp.shape
    xr = xy[ok, 0].astype(np.float64)
    yy = np.clip(np.rint(xy[ok, 1]).astype(int), 0, h - 1)
    x0 = np.floor(xr).astype(int)
    f = xr - x0
    d = (1 - f) * disp[yy, np.clip(x0, 0, w - 1)] + f * disp[yy, np.clip(x0 + 1, 0, w - 1)]
    err = np.abs((kp["x"][ok].astype(np.float64) - xr) - d)
    return int(ok.sum()), int((err < 0.5).sum()), float(np.median(err))


@pytest.mark.parametrize("prm,ssd,measured", [
    (dict(), 1, (289, 275)), (dict(), 0, (291, 275)), (dict(max_level=0), 1, (297, 288)),
    (dict(win_width=7, win_height=7, max_level=2), 1, (295, 286))])
def test_sanity_on_a_planted_disparity_field(prm, ssd, measured):
    """At least 270 of the 300 corners get status 1 and at least 90 % of those lie within 0.5 px of the planted field.
    Measured with the restatement: 289 / 275 (15 x 3, five levels, SSD), 291 / 275 (SAD), 297 / 288 (one level),
    295 / 286 (7 x 7, two levels); median error 0.04 px."""
    left, right, disp, kp = stereo3()
    xy, st, sc, trace = ref.block_match(left, right, kp, _abi.stereo_flow_params(**prm), ssd, want_trace=True)
    n_ok, n_close, med = found_against_the_field(xy, st, kp, disp)
    evals = np.mean([int((t["lmin"] - t["lmax"]).clip(0).sum()) for t in trace])
    print("%s ssd %d: status 1 %d, within 0.5 px %d, median %.3f px, %.1f window evaluations per corner" % (
        prm, ssd, n_ok, n_close, med, evals))
    assert len(kp) == 300
    assert n_ok >= 270 and n_close >= 0.9 * n_ok
    assert (n_ok, n_close) == measured
    assert (sc[st == 1] >= 0).all() and (xy[st == 1, 1] == kp["y"][st == 1]).all()


def test_identical_images_have_no_disparity():
    """rtabmap's defaults on all 300 corners: the zero score of d = 0 never wins, the coarse levels lead next to it, and
    the gate of the bisection rejects what is left: every status is 0.  (A one-level search over all 128 disparities does
    find a few accidental windows far away: 5 of 300 with SSD -- the pyramid is what keeps the search near d = 0.)"""
    left, _, _, kp = stereo3()
    for ssd in (1, 0):
        xy, st, sc = ref.block_match(left, left, kp, None, ssd)
        assert not st.any()


def test_constant_image_has_no_positive_score():
    flat = np.full((120, 200), 90, np.uint8)
    pts = np.array([(100.0, 60.0), (50.5, 30.25), (150.0, 100.0), (10.0, 10.0)], np.float32)
    for ssd in (1, 0):
        xy, st, sc, trace = ref.block_match(flat, flat, pts, None, ssd, want_trace=True)
        assert not st.any() and not xy.any() and (sc == -1).all()
        assert all((t["best"] == -1).all() for t in trace)


def test_stripes_pick_the_earliest_of_equal_minima():
    """Vertical stripes of period 8, the right image shifted by 3 px, one level: disparities 3, 11, 19, ... score alike
    (zero is excluded, so the stripes carry a small row ramp that makes every score positive and equal); the search runs
    from the smallest disparity up and keeps the first."""
    h, w = 40, 160
    x = np.arange(w + 3)
    row = np.where((x // 4) % 2 == 0, 60, 180).astype(np.uint8)
    left = np.tile(row[:w], (h, 1))
    right = np.tile(row[3:], (h, 1)).copy()               # right(x) = left(x + 3): disparity 3
    right[:, :] += 1                                       # |difference| 1 everywhere at the true shift: a positive score
    pts = np.array([(100.0, 20.0), (90.0, 10.0), (120.0, 30.0)], np.float32)
    prm = _abi.stereo_flow_params(max_level=0, min_disparity=0.0, max_disparity=40.0, iterations=0)
    for ssd in (1, 0):
        xy, st, sc, trace = ref.block_match(left, right, pts, prm, ssd, want_trace=True)
        assert st.all() and (pts[:, 0] - xy[:, 0] == 3.0).all() and (sc == 45.0).all()
        for t in trace:
            assert len(t) == 1 and t["level"][0] == 0 and t["lmin"][0] == 0 and t["best"][0] == 3


def test_struct_defaults_header_and_exports_agree():
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _abi.SF_ABI_VERSION == 8 and L.sf_abi_version() == 8
    body = re.search(r"typedef struct sf_stereo_params \{(.*?)\} sf_stereo_params;", hdr, re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", body) == ["optical_flow", "ssd"] == [f[0] for f in _abi.StereoParams._fields_]
    assert C.sizeof(_abi.StereoParams) == 8 and _abi.StereoParams.ssd.offset == 4
    d = _abi.StereoParams(7, 7)
    L.sf_stereo_defaults(d)
    assert (d.optical_flow, d.ssd) == (1, 1) and bytes(d) == bytes(_abi.stereo_params())
    for method in ("stereo_set_params", "stereo_get_params", "stereo_block_match_device"):
        assert callable(getattr(lib.SeparatorFinder, method))


def test_calls_refuse_a_missing_handle_or_struct():
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    p = _abi.stereo_params(0, 0)
    assert L.sf_stereo_set_params(None, p) == _abi.SF_EINVAL
    assert L.sf_stereo_get_params(None, p) == _abi.SF_EINVAL and (p.optical_flow, p.ssd) == (0, 0)
    assert L.sf_stereo_block_match_device(None, None, None, 10, 10, 10, None, 0, None, 1, None, None, None, None) == _abi.SF_EINVAL
    L.sf_stereo_defaults(None)                             # (a no-op, like the other *_defaults)
