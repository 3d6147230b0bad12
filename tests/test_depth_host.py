"""Host: the restatement of the depth keyframe path (tests/depth_ref.py) against hand-computed values, the conditions that make
the GPU test inputs (tests/depth_cases.py) worth running, asserted on the restatement alone, and the parameter validation of
the depth calls through the C-ABI (no device is touched: every call here is refused, or is pure host code)."""
import ctypes as C

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from tests import depth_cases as cases
from tests import depth_ref as ref
from tests import fast_ref, gftt_ref

F32 = np.float32


def _cam(**kw):
    d = dict(fx=50.0, fy=40.0, cx=7.5, cy=5.25, baseline=0.0)
    d.update(kw)
    return _abi.stereo_camera(d.pop("fx"), d.pop("fy"), d.pop("cx"), d.pop("cy"), d.pop("baseline"), **d)


def test_constant_plane_projects_exactly():
    Z = F32(2.5)
    depth = np.full((12, 16), Z, F32)
    cam = _cam()
    xy = np.array([[3.0, 4.0], [7.5, 5.25], [15.0, 11.0], [0.0, 0.0], [9.25, 2.75]], F32)
    got = ref.keypoints3d_depth(xy, depth, cam)
    want = np.stack([(xy[:, 0] - F32(7.5)) * Z / F32(50.0), (xy[:, 1] - F32(5.25)) * Z / F32(40.0), np.full(5, Z, F32)], axis=1)
    assert got.dtype == F32 and got.tobytes() == want.astype(F32).tobytes()
    mm = np.full((12, 16), 2500, np.uint16)                 # the same plane in millimetres: 2500 * 0.001f
    zmm = F32(2500) * F32(0.001)
    assert ref.get_depth(mm, 3.0, 4.0) == (zmm * F32(4) + zmm * F32(12)) / F32(16)


def test_two_percent_step_edge_excludes_the_far_side_with_the_hand_computed_weights():
    # columns 0 .. 3 at 2.00 m, columns 4 .. at 2.05 m: 0.05 > 0.02 * 2.00 = 0.04, so neither side sees the other
    depth = np.full((9, 9), 2.0, F32)
    depth[:, 4:] = 2.05
    d = F32(2.0)
    # pixel (3, 4): neighbours in columns 2 and 3 count -- (2,3) (2,5) corners: weight 1; (2,4) (3,3) (3,5): weight 2
    want = (d * F32(4) + ((((d + d * F32(2)) + d) + d * F32(2)) + d * F32(2))) / (F32(1 + 2 + 1 + 2 + 2) + F32(4))
    assert ref.get_depth(depth, 3.0, 4.0) == want == d
    # 1.99 / 2.00 / 2.03 across a row: of the eight neighbours of (4, 4) = 2.00 only those within 0.04 count
    depth = np.full((9, 9), 2.0, F32)
    depth[:, 3] = 1.99
    depth[:, 5] = 2.05
    a = F32(1.99)
    # loop order: uu = 3 (vv 3, 4, 5), uu = 4 (vv 3, 5), uu = 5 excluded
    sd = F32(0)
    for v in (a, a * F32(2), a, d * F32(2), d * F32(2)):
        sd = sd + v
    assert ref.get_depth(depth, 4.0, 4.0) == (d * F32(4) + sd) / (F32(8) + F32(4))
    # a step of just under 2 %: both sides count
    depth = np.full((9, 9), 2.0, F32)
    depth[:, 5:] = 2.039
    assert ref.get_depth(depth, 4.0, 4.0) != ref.get_depth(np.full((9, 9), 2.0, F32), 4.0, 4.0)


def test_invalid_depths_give_no_point():
    cam = _cam()
    mm = np.full((8, 8), 1500, np.uint16)
    mm[2, 3], mm[4, 5] = 0, 65535
    fl = np.full((8, 8), 1.5, F32)
    fl[1, 1], fl[2, 3], fl[4, 5], fl[6, 6] = 0.0, np.nan, np.inf, -np.inf
    for depth, bad in ((mm, [(3, 2), (5, 4)]), (fl, [(1, 1), (3, 2), (5, 4), (6, 6)])):
        xyz = ref.keypoints3d_depth(np.array(bad + [(3, 5)], F32), depth, cam)
        assert np.isnan(xyz[:-1]).all() and np.isfinite(xyz[-1]).all()
        assert xyz[:-1].view(np.uint32).tolist() == [[0x7FC00000] * 3] * len(bad)          # quiet NaNs, these bits
        assert ref.points_valid(xyz).tolist() == [0] * len(bad) + [1]
    # an invalid neighbour is left out of the smoothing, a valid centre beside it still has a point
    z = F32(1500) * F32(0.001)
    assert ref.get_depth(mm, 3.0, 3.0) == (z * F32(4) + z * F32(10)) / (F32(10) + F32(4))  # (3, 2) above it is missing: weight 2
    assert ref.values(mm)[2, 3] == 0 and ref.values(mm)[4, 5] == 0
    assert ref.depth_mask(mm).tolist()[2][3] == 0 and ref.depth_mask(fl)[2, 3] == 0 and ref.depth_mask(fl)[6, 6] == 0
    assert ref.depth_mask(fl)[4, 5] == 255 and ref.depth_mask(fl, 0.0, 10.0)[4, 5] == 0    # +inf passes only without max_depth
    assert ref.depth_mask(mm, -1.0, 0.0)[2, 3] == 255                                       # value 0 > min_depth -1: the rule as stated


def test_border_and_corner_pixels_use_the_reduced_window():
    depth = (np.arange(6 * 7, dtype=F32).reshape(6, 7) * F32(0.001) + F32(3.0)).astype(F32)   # all within 2 % of each other
    v = ref.values(depth)

    def by_hand(u, vv):
        sw, sd = F32(0), F32(0)
        for uu in range(max(u - 1, 0), min(u + 1, 6) + 1):
            for w in range(max(vv - 1, 0), min(vv + 1, 5) + 1):
                if (uu, w) == (u, vv):
                    continue
                cross = uu == u or w == vv
                sw = sw + (F32(2) if cross else F32(1))
                sd = sd + (v[w, uu] * F32(2) if cross else v[w, uu])
        return (v[vv, u] * F32(4) + sd) / (sw + F32(4)), sw
    for (u, vv), weights in (((0, 0), 5), ((6, 5), 5), ((0, 3), 8), ((3, 0), 8), ((6, 2), 8), ((3, 3), 12)):
        want, sw = by_hand(u, vv)
        assert sw == weights
        assert ref.get_depth(depth, float(u), float(vv)) == want


def test_rounding_of_coordinates():
    depth = (np.arange(5 * 8, dtype=F32).reshape(5, 8) + F32(1)).astype(F32)               # steps far above 2 %: no smoothing
    w, h = 8, 5
    assert ref.depth_pixel(w - 0.4, w) == w - 1 and ref.get_depth(depth, w - 0.4, 2.0) == depth[2, 7]   # x = w - 0.4: column w - 1
    assert ref.depth_pixel(float(w), w) == -1 and ref.get_depth(depth, float(w), 2.0) == 0
    assert ref.depth_pixel(2.5, w) == 3 and ref.depth_pixel(2.4999, w) == 2                 # k + 0.5 rounds up
    assert ref.depth_pixel(-0.5, w) == 0 and ref.depth_pixel(-0.7, w) == 0                  # C's truncation toward zero
    assert ref.depth_pixel(-1.5, w) == -1 and ref.depth_pixel(-1.4999, w) == 0
    assert ref.depth_pixel(np.nan, w) == -1 and ref.depth_pixel(np.inf, w) == -1 and ref.depth_pixel(-3e38, w) == -1
    assert ref.get_depth(depth, 3.0, h - 0.4) == depth[4, 3] and ref.get_depth(depth, 3.0, float(h)) == 0


def test_depth_filters_and_local_transform():
    depth = np.full((10, 10), 2.0, F32)
    depth[:, 5:] = 6.0
    xy = np.array([[2.0, 5.0], [7.0, 5.0]], F32)
    assert np.isfinite(ref.keypoints3d_depth(xy, depth, _cam())).all()
    near = ref.keypoints3d_depth(xy, depth, _cam(max_depth=4.0))
    assert np.isfinite(near[0]).all() and np.isnan(near[1]).all()
    far = ref.keypoints3d_depth(xy, depth, _cam(min_depth=3.0))
    assert np.isnan(far[0]).all() and np.isfinite(far[1]).all()
    assert np.isfinite(ref.keypoints3d_depth(xy, depth, _cam(min_depth=2.0, max_depth=6.0))[1]).all()   # Z <= max_depth keeps 6.0
    assert np.isnan(ref.keypoints3d_depth(xy, depth, _cam(min_depth=2.0, max_depth=6.0))[0]).all()      # Z > min_depth drops 2.0
    # cx, cy <= 0: the image centre, integer division
    c = ref.keypoints3d_depth(xy[:1], depth, _cam(cx=0.0, cy=-1.0))
    assert c[0, 0] == (F32(2.0) - (F32(5) - F32(0.5))) * F32(2.0) / F32(50.0) and c[0, 1] == (F32(5.0) - (F32(5) - F32(0.5))) * F32(2.0) / F32(40.0)
    # a local transform: the stated expression, row by row
    L = np.array([[0.0, 0.0, 1.0, 0.1], [-1.0, 0.0, 0.0, 0.2], [0.0, -1.0, 0.0, 0.3]], F32)
    p = ref.keypoints3d_depth(xy[:1], depth, _cam())[0]
    q = ref.keypoints3d_depth(xy[:1], depth, _cam(local_transform=L))[0]
    assert q.tolist() == [((F32(0) * p[0] + F32(0) * p[1]) + p[2]) + F32(0.1), ((-p[0] + F32(0) * p[1]) + F32(0) * p[2]) + F32(0.2),
                          ((F32(0) * p[0] - p[1]) + F32(0) * p[2]) + F32(0.3)]


def test_a_full_mask_gives_the_unmasked_detectors():
    for case in cases.GFTT_CASES:
        assert cases.gftt_want(case, "full").tobytes() == cases.gftt_unmasked(case).tobytes()
        assert len(cases.gftt_want(case, "empty")) == 0
    for case in cases.FAST_CASES:
        assert cases.fast_want(case, "full").tobytes() == cases.fast_unmasked(case).tobytes()
        assert len(cases.fast_want(case, "empty")) == 0


def test_the_gpu_test_inputs_are_worth_running():
    moved, suppressed, cut = [], 0, 0
    for case, spec in cases.GFTT_CASES.items():
        img, mask, R = cases.gftt_inputs(case)
        want, plain = cases.gftt_want(case), cases.gftt_unmasked(case)
        frac = float((mask != 0).mean())
        print("GFTT %s: %d corners under the mask (%d without), mask %.0f %% set" % (case, len(want), len(plain), 100 * frac))
        assert len(want) >= 20 and 0.3 < frac < 0.98
        assert want.tobytes() != plain.tobytes()
        assert (mask[want["y"].astype(int), want["x"].astype(int)] != 0).all()
        if ref.gftt_threshold(R, mask, cases.QUALITY) != ref.gftt_threshold(R, np.full_like(mask, 255), cases.QUALITY):
            moved.append(case)
        suppressed += cases.suppressed_by_masked_out(case)
        cut += spec[6] > 0 and len(want) == spec[6]
    assert {c for c, s in cases.GFTT_CASES.items() if s[7]} <= set(moved), moved   # the mask removes the global maximum: another threshold
    assert len(moved) < len(cases.GFTT_CASES)                               # ... and in other cases it does not
    assert suppressed >= 1                                                  # a masked-out stronger neighbour suppresses a masked-in pixel
    assert cut >= 1                                                         # max_corners cuts a list
    cut = 0
    for case, spec in cases.FAST_CASES.items():
        img, mask = cases.fast_inputs(case)
        want, plain = cases.fast_want(case), cases.fast_unmasked(case)
        print("FAST %s: %d corners under the mask (%d without)" % (case, len(want), len(plain)))
        assert len(want) >= 20 and want.tobytes() != plain.tobytes()
        assert (mask[want["y"].astype(int), want["x"].astype(int)] != 0).all()
        everything = ref.detect_fast_masked(img, mask, spec[5][0], spec[5][1], 0)
        cut += spec[6] > 0 and len(everything) > spec[6] == len(want)
    assert cut >= 2                                                         # with and without suppression


def test_scenes_hold_every_kind_of_hole():
    for w, h in ref.SIZES:
        mm, fl = ref.scene(w, h, 3, _abi.SF_DEPTH_U16_MM), ref.scene(w, h, 3, _abi.SF_DEPTH_F32_M)
        assert mm.dtype == np.uint16 and fl.dtype == F32 and mm.shape == fl.shape == (h, w)
        assert (mm == 0).any() and (mm == 65535).any() and ((mm > 0) & (mm < 65535)).mean() > 0.5
        assert (fl == 0).any() and np.isnan(fl).any() and np.isposinf(fl).any() and np.isneginf(fl).any()
        assert not ref.depth_mask(ref.scene(w, h, 3, _abi.SF_DEPTH_U16_MM, dead=True)).any()
        assert not ref.depth_mask(ref.scene(w, h, 3, _abi.SF_DEPTH_F32_M, dead=True), 0.0, 50.0).any()
        # steps: neighbouring pixels more than 2 % apart exist, so the smoothing excludes some neighbours somewhere
        v = ref.values(fl)
        with np.errstate(invalid="ignore"):
            assert (np.abs(v[:, 1:] - v[:, :-1]) > 0.02 * v[:, :-1]).any()


# ---- parameter validation through the C-ABI: refused before any device call -------------------------------------------------
def _lib():
    from multi_robot_slam_separators_amd import lib
    return lib.load()


def test_depth_defaults_and_struct_size():
    L = _lib()
    p = _abi.DepthParams()
    p.depth_as_mask = 7
    L.sf_depth_defaults(C.byref(p))
    assert p.depth_as_mask == 1 == _abi.depth_params().depth_as_mask and C.sizeof(p) == 4
    L.sf_depth_defaults(None)                               # tolerated, as the other *_defaults
    assert (_abi.SF_DEPTH_U16_MM, _abi.SF_DEPTH_F32_M) == (0, 1)


def test_null_handles_are_refused_without_a_device():
    L = _lib()
    p = _abi.depth_params()
    cam = _abi.stereo_camera(50.0, 50.0, 8.0, 8.0, 0.0)
    n = C.c_int32()
    assert L.sf_depth_set_params(None, C.byref(p)) == _abi.SF_EINVAL
    assert L.sf_depth_get_params(None, C.byref(p)) == _abi.SF_EINVAL
    assert L.sf_depth_mask_device(None, None, 0, 16, 16, 32, 0, 1, 0.0, 0.0, None, 16, 0) == _abi.SF_EINVAL
    assert L.sf_depth_points_device(None, None, 0, 16, 16, 32, None, 0, C.byref(cam), None, None) == _abi.SF_EINVAL
    assert L.sf_detect_corners_masked_device(None, None, 16, 16, 16, None, 16, 10, 0.01, 3.0, None, 0, C.byref(n)) == _abi.SF_EINVAL
    assert L.sf_detect_fast_masked_device(None, None, 16, 16, 16, None, 16, 10, None, None, 0, C.byref(n)) == _abi.SF_EINVAL
    assert L.sf_extract_keyframe_depth_device(None, None, 16, 16, 16, None, None, 0, 32, 0, C.byref(cam), None, None, None, None,
                                              None) == _abi.SF_EINVAL
    assert L.sf_get_features_and_descriptor_depth(None, None, 2, None, 0, 16, 16, 16, 32, C.byref(cam), None, None, None, None, 0,
                                                  C.byref(n), None) == _abi.SF_EINVAL
    assert L.sf_get_features_and_descriptor_depth_batch_device(None, None, None, 0, 1, 16, 16, 16, 256, 32, 512, C.byref(cam), None,
                                                               None, None, None, None, None) == _abi.SF_EINVAL
    assert L.sf_add_keyframes_depth_batch_device(None, None, 0, None, 0, 1, 16, 16, 48, 768, 32, 512, C.byref(cam), None, None, None,
                                                 None, None, None, None) == _abi.SF_EINVAL


def test_depth_format_of_arrays():
    assert _abi.depth_format_of(np.zeros((2, 2), np.uint16)) == _abi.SF_DEPTH_U16_MM
    assert _abi.depth_format_of(np.zeros((2, 2), np.float32)) == _abi.SF_DEPTH_F32_M
    with pytest.raises(ValueError):
        _abi.depth_format_of(np.zeros((2, 2), np.float64))
