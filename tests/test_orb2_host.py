"""No GPU: the restatement of ORB on a pyramid (tests/orb2_ref.py) checks itself -- literal per-pixel loops against the
vectorised forms, the quota formula, retainBest's ties, the level sizes of the GPU cases -- and the ctypes mirror of
sf_orb_detector_params is compared with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from tests import extract_cases as ec
from tests import orb2_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(seed, w, h):
    return np.ascontiguousarray(ec.make_stereo_pair(seed, width=w, height=h, max_disp=min(40.0, w / 6))[0])


@pytest.mark.parametrize("src,dst", [((67, 45), (34, 23)), ((50, 42), (42, 35)), ((40, 30), (20, 15)), ((31, 9), (8, 2)),
                                     ((5, 6), (3, 3))])
def test_bilinear_resize_equals_its_literal_loop(src, dst):
    img = np.random.default_rng(src[0]).integers(0, 256, size=(src[1], src[0]), dtype=np.uint8)
    lit = ref.resize_literal(img, dst[0], dst[1])
    if src[0] == 2 * dst[0] and src[1] == 2 * dst[1]:            # the area path: (a + b + c + d + 2) >> 2, written out
        p = img.astype(np.int64)
        want = np.array([[(p[2 * y, 2 * x] + p[2 * y, 2 * x + 1] + p[2 * y + 1, 2 * x] + p[2 * y + 1, 2 * x + 1] + 2) >> 2
                          for x in range(dst[0])] for y in range(dst[1])], np.uint8)
        assert np.array_equal(ref.resize(img, dst[0], dst[1]), want)
        # exact halving in bilinear form: f = 0.5 on both axes, the plain mean up to the fixed point's truncation
        assert np.abs(lit.astype(int) - want.astype(int)).max() <= 1
    else:
        assert np.array_equal(ref.resize(img, dst[0], dst[1]), lit)


def test_bilinear_coefficients():
    s, c0, c1 = ref.linear_axis(102, 203)
    assert ((c0 + c1) == 2048).all() and s.min() == 0 and s.max() <= 202
    assert (s[1:] >= s[:-1]).all()
    s, c0, c1 = ref.linear_axis(3, 5)                            # the last index clamps: s = src - 1, f = 0
    assert s[-1] <= 4 and c0[0] + c1[0] == 2048
    s, c0, c1 = ref.linear_axis(7, 6)                            # upscaling by a hair: the first index clamps to 0
    assert s[0] == 0 and c0[0] == 2048 and c1[0] == 0 and s[-1] == 5 and c1[-1] == 0


def test_harris_equals_its_literal_loop():
    img = _image(1, 101, 85)
    rng = np.random.default_rng(5)
    x, y = rng.integers(16, 101 - 16, 40), rng.integers(16, 85 - 16, 40)
    got = ref.harris(img, x, y)
    assert got.dtype == np.float32
    for i in range(len(x)):
        assert got[i].tobytes() == ref.harris_literal(img, int(x[i]), int(y[i])).tobytes()
    assert (got > 0).all()
    flat = np.full((40, 40), 90, np.uint8)
    edge = flat.copy()
    edge[:, 20:] = 200                                           # a straight edge: b = c = 0, -0.04 a^2 < 0
    neg = ref.harris(edge, [20], [20])[0]
    assert neg < 0 and neg.tobytes() == ref.harris_literal(edge, 20, 20).tobytes()   # a sort key must order negative floats
    assert ref.harris(flat, [20], [20])[0] == 0.0


@pytest.mark.parametrize("scale,levels,want", [(2.0, 3, [171, 86, 43]), (1.2, 8, [65, 54, 45, 38, 31, 26, 22, 19]),
                                               (1.5, 4, None)])
def test_quotas_sum_to_nfeatures(scale, levels, want):
    q = ref.quotas(300, scale, levels)
    assert sum(q) == 300 and len(q) == levels and all(a >= b for a, b in zip(q, q[1:]))
    if want:
        assert q == want
    for n in (100, 1000, 32767):
        assert sum(ref.quotas(n, scale, levels)) == n
    assert sum(ref.quotas(1, scale, levels)) >= 1                # (rounding up on several levels may exceed a tiny nfeatures)
    assert ref.quotas(300, scale, 1) == [300]


def test_retain_best_keeps_ties_at_the_cut():
    r = np.array([5, 9, 7, 7, 3, 7, 1, 9], np.float32)
    assert ref.retain_best(r, 3).tolist() == [False, True, True, True, False, True, False, True]    # 9 9 7 | 7 7 stay
    assert ref.retain_best(r, 2).tolist() == [False, True, False, False, False, False, False, True]
    assert ref.retain_best(r, 8).all() and ref.retain_best(r, 20).all()
    assert not ref.retain_best(r, 0).any()
    assert ref.retain_best(np.array([-1.0, -3.0, -2.0], np.float32), 2).tolist() == [True, False, True]
    assert ref.retain_best(np.zeros(0, np.float32), 0).shape == (0,)


def test_level_sizes():
    assert ref.level_sizes(202, 170, 2.0, 3) == [(202, 170), (101, 85), (50, 42)]          # 50.5 -> 50, 42.5 -> 42
    assert ref.level_sizes(203, 171, 2.0, 3) == [(203, 171), (102, 86), (51, 43)]          # 101.5 -> 102, 85.5 -> 86
    assert ref.level_sizes(320, 240, 2.0, 3) == [(320, 240), (160, 120), (80, 60)]
    s = ref.level_sizes(202, 170, 1.2, 8)
    assert s[0] == (202, 170) and s[-1] == (56, 47) and len(s) == 8
    lv = ref.pyramid(_image(1, 202, 170), 2.0, 3)
    assert [l.shape for l in lv] == [(170, 202), (85, 101), (42, 50)]


def test_limit_keypoints_orders_by_magnitude_then_descending_index():
    kp = np.zeros(6, _abi.KEYPOINT_DTYPE)
    kp["response"] = [1.0, -4.0, 2.0, 2.0, 0.5, 3.0]
    kp["class_id"] = np.arange(6)
    assert ref.limit_keypoints(kp, 6)["class_id"].tolist() == [0, 1, 2, 3, 4, 5]
    assert ref.limit_keypoints(kp, 4)["class_id"].tolist() == [1, 5, 3, 2]


def test_case_counts_of_the_gpu_tests():
    """FAST corners inside the border per level, and which quotas bite: what tests/test_gpu_orb2.py relies on."""
    lv = ref.detect_levels(_image(1, 202, 170), 300, 2.0, 3)
    assert [d["found"] for d in lv] == [485, 121, 3] and [d["quota"] for d in lv] == [171, 86, 43]
    assert [len(d["kp"]) for d in lv] == [171, 86, 3]
    lv = ref.detect_levels(_image(1, 203, 171), 300, 2.0, 3)
    assert [d["found"] for d in lv] == [480, 144, 3]
    lv = ref.detect_levels(_image(1, 202, 170), 300, 1.2, 8)
    assert [d["found"] for d in lv] == [485, 265, 183, 109, 69, 34, 15, 7]
    assert [d["found"] > d["quota"] for d in lv] == [True] * 6 + [False] * 2


def test_extract_groups_rows_by_level():
    image = _image(3, 202, 170)
    kp = np.zeros(8, _abi.KEYPOINT_DTYPE)
    kp["x"] = [100, 60, 80.5, 120, 30, 150, 90, 18]
    kp["y"] = [80, 60, 70, 90.5, 40, 100, 50, 80]
    kp["octave"] = [2, 0, 1, 0, 3, 1, 0x100 | 2, 0]
    kp["angle"] = [10, 20, 30, 40, 50, 60, 70, 80]
    cam = _abi.stereo_camera(460.0, 458.0, 101.0, 85.0, 0.11)
    d, p, k = ref.extract_keyframe(image, kp, None, None, cam)
    assert k["angle"].tolist() == [20, 40, 30, 60, 10, 70]        # levels 0 0 1 1 2 2; octave 3 and the border corner dropped
    assert d.shape == (6, 32) and np.isnan(p).all()


def test_abi_mirror_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    body = re.search(r"typedef struct sf_orb_detector_params \{(.*?)\} sf_orb_detector_params;", text, re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+);", body, re.M)
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(_abi.OrbDetectorParams._fields_)
    assert C.sizeof(_abi.OrbDetectorParams) == 20
    p = _abi.orb_detector_params()
    assert (p.scale_factor, p.n_levels, p.first_level, p.score_type, p.fast_threshold) == (2.0, 3, 0, 0, 20)
    for sym in ("sf_orb_detector_defaults", "sf_set_feature_type_orb", "sf_get_orb_detector", "sf_detect_orb_device"):
        assert re.search(r"\b%s\(" % sym, text), sym
    assert re.search(r"#define SF_ABI_VERSION 8\b", text) and _abi.SF_ABI_VERSION == 8 and _abi.FEATURE_ORB == 2
