"""The FAST detector and Vis/FeatureType 4 (FAST/BRIEF) without a GPU: the C-ABI of the feature (symbols, the
sf_fast_params layout, the unchanged ABI version) and self-checks of the NumPy restatement (tests/fast_ref.py) that the
GPU tests compare with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from multi_robot_slam_separators_amd import _abi
from tests import fast_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_fast_defaults", "sf_fast_set_params", "sf_fast_get_params", "sf_detect_fast_device"]


def test_library_exports_the_fast_calls_at_abi_8():
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    for name in NEW + ["sf_set_feature_type"]:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _abi.SF_ABI_VERSION == 8 and L.sf_abi_version() == 8
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert _abi.FEATURE_FAST_BRIEF == 4
    for method in ("fast_set_params", "fast_get_params", "detect_fast_device"):
        assert hasattr(lib.SeparatorFinder, method)


def test_fast_params_layout_and_defaults_match_the_header(tmp_path):
    src = tmp_path / "fast.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sepfinder.h"\n'
        "int main(void){ sf_fast_params p; sf_fast_defaults(&p);"
        " printf(\"%zu %zu %zu %zu %d %d %d\\n\", sizeof(sf_fast_params), offsetof(sf_fast_params, threshold),"
        " offsetof(sf_fast_params, nonmax_suppression), sizeof(sf_params), p.threshold, p.nonmax_suppression,"
        " SF_ABI_VERSION); return 0; }\n")
    exe = tmp_path / "fast"
    lib_dir = os.path.join(ROOT, "multi_robot_slam_separators_amd")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                           "-lsepfinder", "-Wl,-rpath," + lib_dir, "-L", "/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _abi.FastParams
    assert got[:3] == [C.sizeof(F), F.threshold.offset, F.nonmax_suppression.offset] == [8, 0, 4]
    assert got[3] == 232 == C.sizeof(_abi.Params)                       # the FAST state is not kept in sf_params
    d = _abi.fast_params()
    assert got[4:6] == [d.threshold, d.nonmax_suppression] == [20, 1]
    assert got[6] == 8


def test_ring_is_the_radius_3_circle_in_order():
    assert len(ref.RING) == 16 and len(set(ref.RING)) == 16
    assert ref.RING[0] == (0, 3) and ref.RING[4] == (3, 0) and ref.RING[8] == (0, -3) and ref.RING[12] == (-3, 0)
    for k, (dx, dy) in enumerate(ref.RING):
        assert round((dx * dx + dy * dy) ** 0.5) == 3
        nx, ny = ref.RING[(k + 1) % 16]
        assert max(abs(nx - dx), abs(ny - dy)) == 1                    # consecutive entries are neighbours
        assert ref.RING[(k + 8) % 16] == (-dx, -dy)                    # opposite entries are opposite pixels


def test_the_restatement_agrees_with_itself_three_ways():
    """The arc definition (measure), a literal cornerScore<16> loop and a brute force over every threshold 0 .. 255 of
    the segment test itself, on every domain pixel of a seeded random image."""
    rng = np.random.default_rng(0)
    # low-contrast noise plus a few strong blobs: corners of many scores, and many non-corners
    img = rng.integers(90, 130, size=(36, 44)).astype(np.int32)
    for _ in range(25):
        y, x = rng.integers(0, 36), rng.integers(0, 44)
        img[y:y + rng.integers(1, 4), x:x + rng.integers(1, 4)] += rng.integers(-90, 120)
    img = np.clip(img, 0, 255).astype(np.uint8)
    h, w = img.shape
    m = ref.measure(img)
    assert (m[:3] == 0).all() and (m[-3:] == 0).all() and (m[:, :3] == 0).all() and (m[:, -3:] == 0).all()
    n_corners = 0
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            passing = [t for t in range(256) if ref.is_corner_brute(img, x, y, t)]
            best = max(passing) if passing else -1
            assert passing == list(range(best + 1))                    # a corner at t is a corner at every smaller t
            assert best == max(int(m[y, x]) - 1, -1), (x, y)
            for t in (1, 20, 60):
                if m[y, x] > t:
                    n_corners += t == 20
                    assert ref.corner_score_literal(img, x, y, t) == m[y, x] - 1, (x, y, t)
                else:
                    assert ref.corner_score_literal(img, x, y, t) < t, (x, y, t)
    assert n_corners > 20
    s = ref.score_plane(img, 20)
    assert s.dtype == np.uint8 and ((s > 0) == (m > 20)).all() and (s[m > 20] == m[m > 20] - 1).all()


def _one(kp, x, y, response):
    assert len(kp) == 1
    k = kp[0]
    assert (k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"], k["class_id"]) == (x, y, 7.0, -1.0, response, 0, -1)


def test_hand_worked_cases():
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = 200                                        # every d_k = 200: m = 200, score 199; its neighbours see
    _one(ref.detect(img), 4.0, 4.0, 199.0)                 # at most one bright ring pixel: no corner
    img = np.full((7, 7), 10, np.uint8)
    img[3, 3] = 100                                        # the only domain pixel: d_k = 90, score 89
    _one(ref.detect(img), 3.0, 3.0, 89.0)
    assert len(ref.detect(img, threshold=89)) == 1 and len(ref.detect(img, threshold=90)) == 0
    assert len(ref.detect(np.full((6, 6), 255, np.uint8))) == 0        # no domain
    big = np.zeros((6, 6), np.uint8)
    big[3, 3] = 255
    assert len(ref.detect(big)) == 0 and len(ref.detect(np.zeros((5, 6), np.uint8))) == 0


def test_a_square_corner_is_a_plateau():
    """The corner region of a bright axis-aligned square holds several pixels of ONE score: under the strict 3 x 3
    suppression they remove each other and nothing is left; without suppression all of them come out, response 0."""
    img = np.full((40, 40), 20, np.uint8)
    img[10:30, 10:30] = 220
    s = ref.score_plane(img, 20)
    corners = np.argwhere(s > 0)
    assert len(corners) > 0 and len(np.unique(s[s > 0])) == 1            # a plateau: every corner scores the same
    near = [(y, x) for y, x in corners if abs(y - 10) <= 2 and abs(x - 10) <= 2]
    assert len(near) >= 2
    assert len(ref.detect(img, 20, 1)) == 0
    kp = ref.detect(img, 20, 0)
    assert len(kp) == len(corners) and (kp["response"] == 0).all()
    assert sorted(zip(kp["y"].astype(int), kp["x"].astype(int))) == sorted(map(tuple, corners))


def test_order_and_limit():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(60, 80), dtype=np.uint8)
    w = img.shape[1]
    everything = ref.detect(img, 20, 1, 0)
    n = len(everything)
    assert n > 100
    idx = everything["y"].astype(np.int64) * w + everything["x"].astype(np.int64)
    assert (np.diff(idx) > 0).all()                                      # unlimited: raster order
    assert ref.detect(img, 20, 1, -3).tobytes() == everything.tobytes()
    assert ref.detect(img, 20, 1, n).tobytes() == everything.tobytes()   # count == limit: still raster
    assert ref.detect(img, 20, 1, n + 7).tobytes() == everything.tobytes()
    limit = n // 3
    top = ref.detect(img, 20, 1, limit)
    assert len(top) == limit
    r = top["response"]
    ti = top["y"].astype(np.int64) * w + top["x"].astype(np.int64)
    assert (np.diff(r) <= 0).all()
    same = np.diff(r) == 0
    assert same.any() and (np.diff(ti)[same] < 0).all()                  # ties: descending raster index
    # the cut takes the LAST (highest-index) corners of the tied score
    cut = r[-1]
    tied_all = np.sort(idx[everything["response"] == cut])
    tied_kept = np.sort(ti[r == cut])
    assert len(tied_all) > len(tied_kept) > 0, "choose a limit whose cut falls inside a tie"
    assert np.array_equal(tied_kept, tied_all[-len(tied_kept):])
    assert set(ti[r > cut]) == set(idx[everything["response"] > cut])
    # without suppression every response is 0: the limit keeps the highest raster indices, in descending order
    all0 = ref.detect(img, 20, 0, 0)
    top0 = ref.detect(img, 20, 0, 50)
    i0 = all0["y"].astype(np.int64) * w + all0["x"].astype(np.int64)
    j0 = top0["y"].astype(np.int64) * w + top0["x"].astype(np.int64)
    assert np.array_equal(j0, i0[::-1][:50]) and (top0["response"] == 0).all()
