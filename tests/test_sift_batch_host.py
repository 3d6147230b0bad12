"""The batch form of SIFT (Vis/FeatureType 1) without a GPU: the symbols of the feature, and sf_sift_batch_plan -- the
capacity per image, the images per chunk and the workspace -- against a statement of its arithmetic from the sample counts
of lib.sift_plan (the rule is written out in include/sf_experimental.h)."""
import ctypes as C
import os
import re

import pytest

from multi_robot_slam_separators_amd import _abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_get_features_and_descriptor_sift_batch_device", "sf_add_keyframes_sift_u8_batch_device", "sf_sift_batch_status"]
NEW_EXPERIMENTAL = ["sf_debug_sift_batch_chunk", "sf_sift_batch_plan"]
CANDIDATES = 1 << 18          # extrema, and keypoints, per image (include/sepfinder.h: 262144)
BUDGET = 1 << 30              # the chunk's workspace (include/sepfinder.h: 1 GB)
# (width, height, keyframes, n_octave_layers)
LAYOUTS = [(160, 120, 5, 3), (752, 480, 64, 3), (752, 480, 1, 3), (752, 480, 3, 3), (1600, 1200, 64, 3), (97, 61, 3, 3),
           (160, 120, 65535, 1), (320, 240, 64, 8), (3, 3, 2, 3), (1800, 1350, 4, 3)]


def test_symbols_and_bindings():
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    exp = open(os.path.join(ROOT, "include", "sf_experimental.h")).read()
    for name in NEW + NEW_EXPERIMENTAL:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED
        assert re.search(r"\b%s\(" % name, hdr if name in NEW else exp), name
        assert not re.search(r"\b%s\(" % name, exp if name in NEW else hdr), name
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8 == L.sf_abi_version()
    for method in ("get_features_and_descriptor_sift_batch_device", "add_keyframes_sift_u8_batch_device", "sift_batch_status",
                   "debug_sift_batch_chunk", "debug_sift_limits"):
        assert callable(getattr(lib.SeparatorFinder, method))
    assert callable(lib.sift_batch_plan)


def a256(x):
    return (x + 255) // 256 * 256


def plan_restated(w, h, n, layers):
    """((cap_img, chunk, workspace bytes), bytes per image): int16 Gaussian planes, int16 difference planes and the float32
    row plane of the enlarged image, each from a multiple of 256 bytes on; a bit per difference sample; key, sorted key and
    list entry per candidate; 32 bytes of counters."""
    _, sizes, gauss, dog = lib.sift_plan(w, h, _abi.sift_params(n_octave_layers=layers))
    base = sizes[0][0] * sizes[0][1]
    assert sizes[0] == (2 * w, 2 * h)
    planes = a256(a256(a256(2 * gauss) + 2 * dog) + 4 * base)
    per_image = planes + a256(4 * ((dog + 31) // 32)) + 20 * CANDIDATES + 32
    chunk = max(min(BUDGET // per_image, n, 65535, (2 ** 31 - 1) // CANDIDATES), 1)
    return (CANDIDATES, chunk, chunk * per_image), per_image


@pytest.mark.parametrize("w,h,n,layers", LAYOUTS)
def test_plan_equals_restatement(w, h, n, layers):
    want, per_image = plan_restated(w, h, n, layers)
    got = lib.sift_batch_plan(w, h, n, _abi.sift_params(n_octave_layers=layers))
    print("%d x %d, %d keyframes, %d layers: plan %s, %d bytes per image" % (w, h, n, layers, got, per_image))
    assert got == want
    cap_img, chunk, workspace = got
    assert 1 <= chunk <= n
    if chunk > 1:
        assert workspace <= BUDGET                                        # (one image runs whatever it needs)
    if chunk < n:
        assert (chunk + 1) * per_image > BUDGET or chunk == (2 ** 31 - 1) // CANDIDATES
    assert cap_img == CANDIDATES


def test_plan_on_the_named_layouts():
    assert lib.sift_batch_plan(160, 120, 5) == lib.sift_batch_plan(160, 120, 5, _abi.sift_params())   # NULL = the defaults
    assert lib.sift_batch_plan(160, 120, 5)[1] == 5                       # the GPU tests' five pairs: one chunk
    cap_img, chunk, workspace = lib.sift_batch_plan(752, 480, 64)
    assert chunk == 19 and 50 << 20 < workspace // chunk < 58 << 20       # about 54 MB per camera image: chunks of 19
    camera = (cap_img, chunk, workspace)
    cap_img, chunk, workspace = lib.sift_batch_plan(1600, 1200, 64)
    assert chunk == 4 and 250 << 20 < workspace // chunk < 256 << 20      # 255 MB per image
    # the largest images the detector takes (2^26 difference samples) need a third of the workspace: chunks of 3
    assert lib.sift_batch_plan(1800, 1350, 64)[1] == 3
    # sigma, the thresholds and n_features do not enter the layout
    assert lib.sift_batch_plan(752, 480, 64, _abi.sift_params(sigma=2.0, contrast_threshold=0.01, n_features=50)) == camera


def test_plan_refusals():
    L = lib.load()
    S = _abi.sift_params
    plan = lambda w, h, n, prm=None: L.sf_sift_batch_plan(w, h, C.byref(prm) if prm is not None else None, n, None, None, None)  # noqa: E731
    sift_plan = lambda w, h: L.sf_sift_plan(w, h, None, None, None, None, None, None)  # noqa: E731
    assert plan(160, 120, 1) == _abi.SF_OK                                # every output is optional
    for args in ((160, 120, 0), (160, 120, -1), (160, 120, 65536), (160, 120, 1, S(n_octave_layers=0)),
                 (160, 120, 1, S(n_octave_layers=9)), (160, 120, 1, S(sigma=0.5)), (160, 120, 1, S(contrast_threshold=-1.0)),
                 (160, 120, 1, S(edge_threshold=0.0)), (160, 120, 1, S(n_features=-1))):
        assert plan(*args) == _abi.SF_EINVAL, args[:3]
    for w, h in ((2, 120), (160, 2), (16385, 100), (100, 16385), (8000, 8000)):   # what sf_sift_plan refuses, with its code
        rc = sift_plan(w, h)
        assert rc != _abi.SF_OK and plan(w, h, 1) == rc, (w, h)
    assert sift_plan(2, 120) == _abi.SF_EINVAL and sift_plan(16385, 100) == _abi.SF_ERANGE and sift_plan(8000, 8000) == _abi.SF_ERANGE
