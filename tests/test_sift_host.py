"""SIFT (Vis/FeatureType 1) without a GPU: the C-ABI of the feature (symbols, ABI version, the sf_sift_params layout), the
library's handle-free tables, plan and parameter check against the NumPy restatement (tests/sift_ref.py), the
deterministic exp, and self-checks that the restatement is SIFT -- it finds a planted blob at its position and scale, its
rows survive an in-plane rotation, and two extrema that converge to one sample give one keypoint."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import extract_cases as ec
from tests import sift_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_sift_defaults", "sf_set_feature_type_sift", "sf_get_sift_params", "sf_detect_sift_device"]
NEW_EXPERIMENTAL = ["sf_sift_check_params", "sf_sift_build_tables", "sf_sift_plan", "sf_debug_sift_limits", "sf_debug_sift_plane"]


def test_library_header_and_bindings_agree_at_abi_8():
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    exp = open(os.path.join(ROOT, "include", "sf_experimental.h")).read()
    for name in NEW + NEW_EXPERIMENTAL:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED
        assert re.search(r"\b%s\(" % name, hdr if name in NEW else exp), name
        assert not re.search(r"\b%s\(" % name, exp if name in NEW else hdr), name
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _abi.SF_ABI_VERSION == 8 and L.sf_abi_version() == 8
    assert _abi.FEATURE_SIFT == 1
    for method in ("set_feature_type_sift", "get_sift_params", "detect_sift", "debug_sift_limits", "debug_sift_plane"):
        assert callable(getattr(lib.SeparatorFinder, method))
    assert C.sizeof(_abi.SiftParams) == 20
    d = _abi.SiftParams()
    L.sf_sift_defaults(C.byref(d))
    want = (0, 3, np.float32(0.04), np.float32(10.0), np.float32(1.6))
    assert (d.n_features, d.n_octave_layers, d.contrast_threshold, d.edge_threshold, d.sigma) == want
    assert bytes(d) == bytes(_abi.sift_params())
    p = ref.Params()
    assert (p.n_features, p.n_octave_layers, np.float32(p.contrast_threshold), np.float32(p.edge_threshold),
            np.float32(p.sigma)) == want


def test_sift_params_layout_matches_the_header(tmp_path):
    src = tmp_path / "sift.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sepfinder.h"\n'
        "int main(void){ sf_sift_params p; sf_sift_defaults(&p);"
        " printf(\"%zu %zu %zu %zu %zu %zu %zu %d %d %.9g %.9g %.9g\\n\", sizeof(sf_sift_params),"
        " offsetof(sf_sift_params, n_features), offsetof(sf_sift_params, n_octave_layers),"
        " offsetof(sf_sift_params, contrast_threshold), offsetof(sf_sift_params, edge_threshold), offsetof(sf_sift_params, sigma),"
        " sizeof(sf_params), p.n_features, p.n_octave_layers, (double)p.contrast_threshold, (double)p.edge_threshold,"
        " (double)p.sigma); return 0; }\n")
    exe = tmp_path / "sift"
    lib_dir = os.path.join(ROOT, "multi_robot_slam_separators_amd")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                           "-lsepfinder", "-Wl,-rpath," + lib_dir, "-L", "/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    got = [float(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _abi.SiftParams
    assert got[:6] == [20, F.n_features.offset, F.n_octave_layers.offset, F.contrast_threshold.offset, F.edge_threshold.offset,
                       F.sigma.offset]
    assert got[6] == 232 == C.sizeof(_abi.Params)                       # the SIFT state is not kept in sf_params
    assert got[7:9] == [0, 3] and [np.float32(v) for v in got[9:]] == [np.float32(0.04), np.float32(10.0), np.float32(1.6)]


# (field, just inside, just outside) of every range, then the values no range admits
RANGES = [("n_features", [0, 1, 100000], [-1]),
          ("n_octave_layers", [1, 8], [0, 9, -3]),
          ("contrast_threshold", [0.0, 1e-6, 1e30], [-1e-6, float("nan"), float("inf"), float("-inf")]),
          ("edge_threshold", [1e-6, 1e30], [0.0, -1.0, float("nan"), float("inf")]),
          ("sigma", [0.8, 8.0, 1.6], [np.nextafter(np.float32(0.8), np.float32(0)), np.nextafter(np.float32(8), np.float32(9)),
                                      0.0, float("nan"), float("inf")])]


@pytest.mark.parametrize("field,good,bad", RANGES)
def test_parameter_validation(field, good, bad):
    L = lib.load()
    assert L.sf_sift_check_params(None) == _abi.SF_OK
    for v in good:
        p = _abi.sift_params(**{field: v})
        assert L.sf_sift_check_params(C.byref(p)) == _abi.SF_OK, (field, v)
    for v in bad:
        p = _abi.sift_params(**{field: v})
        assert L.sf_sift_check_params(C.byref(p)) == _abi.SF_EINVAL, (field, v)
        assert L.sf_sift_build_tables(C.byref(p), None, None, None) == _abi.SF_EINVAL
        assert L.sf_sift_plan(64, 48, C.byref(p), None, None, None, None, None) == _abi.SF_EINVAL


@pytest.mark.parametrize("kw", [{}, dict(n_octave_layers=1), dict(n_octave_layers=5), dict(sigma=1.2)])
def test_tables_equal_numpy(kw):
    """Both sides do the same float64 arithmetic on libm's pow, sqrt and exp and round every coefficient once: the kernels
    read the library's tables, the restatement its own, and they are compared byte for byte."""
    sig, klen, coef = lib.sift_build_tables(_abi.sift_params(**kw))
    rs, rl, rk = ref.tables(ref.Params(**kw))
    n = ref.Params(**kw).n_octave_layers
    assert len(sig) == len(rs) == n + 3 and sig.tobytes() == rs.tobytes()
    assert klen.tobytes() == rl.tobytes()
    for i, k in enumerate(rk):
        assert coef[i, :len(k)].tobytes() == k.tobytes() and (coef[i, len(k):] == 0).all()
        assert len(k) % 2 == 1 and abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6 and k.argmax() == len(k) // 2
        assert np.array_equal(k, k[::-1])
    # the published scheme: plane i of an octave has blur sigma 2^(i / n), the blurs compose in quadrature
    s0 = ref.Params(**kw).sigma
    total = s0
    for i in range(1, n + 3):
        total = math.sqrt(total * total + sig[i] * sig[i])
        assert abs(total - s0 * 2.0 ** (i / n)) < 1e-9 * total
    assert abs(math.sqrt(sig[0] ** 2 + 1.0) - s0) < 1e-12
    if not kw:
        assert klen.tolist() == [11, 11, 13, 17, 21, 27]                # (radius at most 13 at default parameters)
    assert lib.load().sf_sift_build_tables(None, None, None, None) == _abi.SF_OK


@pytest.mark.parametrize("w,h", [(64, 48), (97, 61), (752, 480), (3, 3)])
def test_plan_equals_numpy(w, h):
    n_oct, sizes, g, d = lib.sift_plan(w, h)
    assert (n_oct, sizes) == ref.plan(w, h)
    assert sizes[0] == (2 * w, 2 * h) and all(b == (a[0] // 2, a[1] // 2) for a, b in zip(sizes, sizes[1:]))
    assert g == 6 * sum(a * b for a, b in sizes) and d == 5 * sum(a * b for a, b in sizes)
    if (w, h) == (752, 480):
        assert n_oct == 9 and d < 1 << 24                               # 23 + 6 bits of the sort key's low half
    L = lib.load()
    assert L.sf_sift_plan(2, 40, None, None, None, None, None, None) == _abi.SF_EINVAL
    assert L.sf_sift_plan(16385, 40, None, None, None, None, None, None) == _abi.SF_ERANGE


def test_sift_exp_against_libm():
    """Relative error against math.exp on 10^5 points of [-40, 0]: at most 2^-23 -- one float32 rounding (2^-24) plus a
    float64 polynomial error that stays below 2^-24 (measured: 3.2e-16 before the rounding, 5.9e-8 after)."""
    x = -40.0 * np.random.default_rng(0).random(100000)
    x[:3] = (0.0, -40.0, -1e-300)
    want = np.array([math.exp(v) for v in x])
    e64 = np.abs(ref.sift_exp64(x) - want) / want
    e32 = np.abs(ref.sift_exp(x).astype(np.float64) - want) / want
    print("sift_exp: max relative error %.3g in float64, %.3g rounded to float32" % (e64.max(), e32.max()))
    assert e64.max() < 2.0 ** -24 and e32.max() <= 2.0 ** -23
    assert ref.sift_exp(np.array([0.0]))[0] == 1.0 and ref.sift_exp(np.array([-1000.0]))[0] == 0.0


def blob_image(w, h, cx, cy, sigma, amplitude):
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma))
    return np.clip(np.rint(110.0 + amplitude * g), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("s", [3.0, 6.0, 12.0])
@pytest.mark.parametrize("amplitude", [120.0, -90.0])
def test_restatement_finds_a_planted_blob(s, amplitude):
    """A planted Gaussian blob of standard deviation s comes out as the strongest keypoint, within 1 pixel of its centre,
    with a size within a factor 2^(2/n) of 2 s: one layer step for the sampling of scale, one for the pull of a difference
    of Gaussians toward its lower scale.  Measured: 0.886 .. 0.891 of 2 s for all six, 0.22 .. 0.25 pixels off (the
    enlargement's quarter-pixel phase)."""
    cx, cy = 100.0, 80.0
    kp = ref.detect(blob_image(200, 160, cx, cy, s, amplitude), ref.Params())
    assert len(kp) >= 1
    best = kp[0]
    print("blob s %g, %+.0f: %d keypoints, best %s, size / 2 s = %.3f" % (s, amplitude, len(kp), best, best["size"] / (2 * s)))
    assert abs(best["x"] - cx) <= 1.0 and abs(best["y"] - cy) <= 1.0
    f = 2.0 ** (2.0 / 3.0)
    assert 2 * s / f <= best["size"] <= 2 * s * f
    assert best["class_id"] == -1 and 0 <= best["angle"] < 360 and best["response"] >= 0.04 / 3
    o, layer, _ = ref.unpack_octave(best["octave"])
    assert 1 <= layer <= 3 and abs(1.6 * 2.0 ** (o + layer / 3.0) - best["size"] / 2) <= 0.5 * best["size"] / 2


def test_restatement_rows_survive_an_in_plane_rotation():
    """The keypoints of an image, mapped onto its np.rot90 copy with their angles turned by the same quarter, find their own
    row again as the nearest of all (L2).  Measured: a share of 1.000 of 150; without the turn of the angle 0.033."""
    left, _, _ = ec.make_stereo_pair(51, width=400, height=300)
    img = np.ascontiguousarray(left)
    rot = np.ascontiguousarray(np.rot90(img))                  # rot[i, j] = img[j, W - 1 - i]
    h, w = img.shape
    prm = ref.Params()
    n, m = 150, 60
    kp = ref.detect(img, prm)
    kp = kp[(kp["x"] > m) & (kp["x"] < w - m) & (kp["y"] > m) & (kp["y"] < h - m) & (kp["size"] <= 40)][:n]
    assert len(kp) == n
    kr = kp.copy()
    kr["x"], kr["y"] = kp["y"], np.float32(w - 1) - kp["x"]
    _, da, _ = ref.compute(img, kp, prm)

    def share(turn):
        k2 = kr.copy()
        k2["angle"] = (kp["angle"] + np.float32(turn)) % np.float32(360)
        ib, db, _ = ref.compute(rot, k2, prm)
        assert len(ib) == n
        d2 = ((db[:, None, :].astype(np.float64) - da[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
        return float((d2.argmin(axis=1) == np.arange(n)).mean())
    turned, unturned = share(270.0), share(0.0)
    print("rot90: share %.3f with the angles turned, %.3f without" % (turned, unturned))
    assert turned >= 0.9                                                # measured 1.000 (150 of 150)
    assert unturned < 0.5                                               # measured 0.033
    # the detector's own angles on the rotated copy turn by the same quarter, within 5 degrees, for most keypoints
    own = ref.detect(rot, prm)
    d = (own["x"][None, :] - kr["x"][:, None]) ** 2 + (own["y"][None, :] - kr["y"][:, None]) ** 2
    near = d.min(axis=1) < 1.0
    hits = 0
    for i in np.nonzero(near)[0]:
        cand = own[d[i] < 1.0]
        turn = (cand["angle"].astype(np.float64) - float(kp["angle"][i])) % 360.0
        hits += bool((np.abs(turn - 270.0) <= 5.0).any())
    print("rot90: %d of %d keypoints found again within a pixel, %d with the angle turned by 270 +- 5" % (near.sum(), n, hits))
    assert near.mean() >= 0.9 and hits >= 0.9 * near.sum()


def test_two_extrema_that_converge_to_one_sample_give_one_keypoint():
    """A constructed difference-of-Gaussian stack handed to the refinement directly: a smooth peak whose maximum lies
    between two samples, both of them passed as candidates -- one starts at the converged sample, the other moves onto it."""
    n = 3
    yy, xx = np.mgrid[0:21, 0:21]
    D = np.zeros((n + 2, 21, 21), np.int16)
    for l in range(n + 2):
        D[l] = np.rint(3000.0 * np.exp(-((xx - 10.3) ** 2 + (yy - 10.0) ** 2) / 18.0) * (1.0 - 0.08 * (l - 2) ** 2))
    prm = ref.Params()
    one = ref.refine(D, [2], [10], [10], prm)
    assert len(one[0]) == 1 and (one[0][0], one[1][0], one[2][0]) == (2, 10, 10)
    moved = ref.refine(D, [2], [10], [12], prm)                          # a start two samples off walks onto the same sample
    assert len(moved[0]) == 1 and (moved[0][0], moved[1][0], moved[2][0]) == (2, 10, 10)
    assert moved[3].tobytes() == one[3].tobytes() and moved[4].tobytes() == one[4].tobytes()
    both = ref.refine(D, [2, 2, 2], [10, 10, 10], [10, 12, 11], prm)
    assert len(both[0]) == 1 and both[3].tobytes() == one[3].tobytes() and both[4].tobytes() == one[4].tobytes()
    assert 0.2 < float(one[3][0][0]) < 0.4 and abs(float(one[3][0][1])) < 0.05       # the offset: 0.3 of a sample along x
    far = ref.refine(D, [2, 2], [10, 5], [10, 14], prm)                  # a sample on the peak's flank does not converge there
    assert len(far[0]) == 1
