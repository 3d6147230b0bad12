"""SURF (Vis/FeatureType 0) without a GPU: the C-ABI of the feature (symbols, ABI version, the sf_surf_params layout), the
library's handle-free Gaussian tables and parameter check against the NumPy restatement (tests/surf_ref.py), and
self-checks that the restatement is SURF -- it finds a planted blob at its position and scale, and its rows survive an
in-plane rotation -- and not merely consistent with itself."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

from multi_robot_slam_separators_amd import _abi, lib
from tests import extract_cases as ec
from tests import surf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_surf_defaults", "sf_set_feature_type_surf", "sf_get_surf_params", "sf_detect_surf_device"]
NEW_EXPERIMENTAL = ["sf_surf_build_tables", "sf_surf_check_params"]


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
    assert _abi.FEATURE_SURF == 0
    for method in ("set_feature_type_surf", "get_surf_params", "detect_surf"):
        assert callable(getattr(lib.SeparatorFinder, method))
    assert C.sizeof(_abi.SurfParams) == 20
    d = _abi.SurfParams()
    L.sf_surf_defaults(C.byref(d))
    assert (d.hessian_threshold, d.n_octaves, d.n_octave_layers, d.upright, d.extended) == (500.0, 4, 2, 0, 0)
    assert bytes(d) == bytes(_abi.surf_params())
    p = ref.Params()
    assert (p.hessian_threshold, p.n_octaves, p.n_octave_layers, p.upright, p.extended, p.dims) == (500.0, 4, 2, 0, 0, 64)


def test_surf_params_layout_matches_the_header(tmp_path):
    src = tmp_path / "surf.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sepfinder.h"\n'
        "int main(void){ sf_surf_params p; sf_surf_defaults(&p);"
        " printf(\"%zu %zu %zu %zu %zu %zu %zu %g %d %d %d %d\\n\", sizeof(sf_surf_params),"
        " offsetof(sf_surf_params, hessian_threshold), offsetof(sf_surf_params, n_octaves),"
        " offsetof(sf_surf_params, n_octave_layers), offsetof(sf_surf_params, upright), offsetof(sf_surf_params, extended),"
        " sizeof(sf_params), (double)p.hessian_threshold, p.n_octaves, p.n_octave_layers, p.upright, p.extended);"
        " return 0; }\n")
    exe = tmp_path / "surf"
    lib_dir = os.path.join(ROOT, "multi_robot_slam_separators_amd")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                           "-lsepfinder", "-Wl,-rpath," + lib_dir, "-L", "/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    got = [float(x) for x in subprocess.check_output([str(exe)]).split()]
    F = _abi.SurfParams
    assert got[:6] == [20, F.hessian_threshold.offset, F.n_octaves.offset, F.n_octave_layers.offset, F.upright.offset,
                       F.extended.offset]
    assert got[6] == 232 == C.sizeof(_abi.Params)                       # the SURF state is not kept in sf_params
    assert got[7:] == [500.0, 4, 2, 0, 0]


def test_gaussian_tables_equal_numpy():
    """Both sides build the same float64 Gaussians (exp, a sum in index order, a division, a product) and round once: the
    kernels read the library's tables, the restatement its own, and they are compared byte for byte."""
    xy, w, dw = lib.surf_build_tables()
    rxy, rw = ref.orientation_table()
    rdw = ref.descriptor_weights()
    assert xy.shape == (109, 2) and w.shape == (109,) and dw.shape == (400,)
    assert np.array_equal(xy, rxy)
    assert w.tobytes() == rw.tobytes()
    assert dw.tobytes() == rdw.tobytes()
    # independent of both: NumPy's own exp and sum, equal to the last bit or the one before
    def g(n, sigma):
        x = np.arange(n) - (n - 1) * 0.5
        t = np.exp(-0.5 / (sigma * sigma) * x * x)
        return t / t.sum()
    g13, g20 = g(13, 2.5), g(20, 3.3)
    assert np.allclose(w, (g13[xy[:, 0] + 6] * g13[xy[:, 1] + 6]).astype(np.float32), rtol=2e-7, atol=0)
    assert np.allclose(dw, np.outer(g20, g20).reshape(-1).astype(np.float32), rtol=2e-7, atol=0)
    # the sample set: the 109 lattice points strictly inside radius 6, x outer, y inner
    assert (xy.astype(int) ** 2).sum(axis=1).max() == 34 and len({tuple(p) for p in xy.tolist()}) == 109
    assert xy[0].tolist() == [-5, -3] and xy[54].tolist() == [0, 0] and xy[108].tolist() == [5, 3]
    assert np.array_equal(xy, np.array(sorted(map(tuple, xy.tolist())), np.int8))
    assert abs(float(dw.astype(np.float64).sum()) - 1.0) < 1e-6 and dw.argmax() in (9 * 20 + 9, 9 * 20 + 10, 10 * 20 + 9, 10 * 20 + 10)
    lib.load().sf_surf_build_tables(None, None, None)                  # every output is optional


def test_parameter_validation():
    L = lib.load()
    S = _abi.surf_params
    assert L.sf_surf_check_params(None) == _abi.SF_OK
    good = [S(), S(hessian_threshold=0.0), S(n_octaves=1, n_octave_layers=1), S(n_octaves=8, n_octave_layers=8),
            S(upright=1, extended=1), S(hessian_threshold=1e30)]
    bad = [S(hessian_threshold=-0.5), S(hessian_threshold=float("nan")), S(hessian_threshold=float("inf")),
           S(n_octaves=0), S(n_octaves=9), S(n_octave_layers=0), S(n_octave_layers=9), S(upright=2), S(upright=-1),
           S(extended=2), S(extended=-1)]
    for p in good:
        assert L.sf_surf_check_params(C.byref(p)) == _abi.SF_OK, bytes(p)
    for p in bad:
        assert L.sf_surf_check_params(C.byref(p)) == _abi.SF_EINVAL, bytes(p)


def test_layers_and_scale():
    """The layer sizes of the published scheme, and the quantities compute derives from a keypoint's size."""
    assert [l[2] for l in ref.layers(ref.Params())] == [9, 15, 21, 27, 18, 30, 42, 54, 36, 60, 84, 108, 72, 120, 168, 216]
    assert [l[3] for l in ref.layers(ref.Params(n_octaves=2, n_octave_layers=1))] == [1, 1, 1, 2, 2, 2]
    s, grad = ref.scale_of(9.0)
    assert abs(float(s) - 1.2) < 1e-6 and grad == 4
    assert ref.scale_of(150.0)[1] == 80 and int(np.float32(21.0) * ref.scale_of(150.0)[0]) in (419, 420)
    # the area reduction: every cell's weights sum to the window side, and every window pixel is used exactly 21 times
    for win in (5, 20, 21, 25, 42, 100):
        W = ref.area_weights(win)
        assert W.shape == (21, win) and (W.sum(axis=1) == win).all() and (W.sum(axis=0) == 21).all()
    flat = np.full((37, 37), 93, np.int64)
    assert (ref.patch_of(flat) == 93).all()


def blob_image(w, h, cx, cy, sigma, amplitude):
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma))
    return np.clip(np.rint(110.0 + amplitude * g), 0, 255).astype(np.uint8)


def box_filter_argmax(sigma):
    """The filter side L at which the box-filter Hessian of a continuous Gaussian blob of standard deviation sigma, taken at
    its centre, is largest: Dxx = the means of three lobes L / 3 wide (1, -2, 1) times the mean over the lobes' 5 L / 9
    extent along y, Dyy the same by symmetry, Dxy = 0 at the centre -- det = Dxx Dyy.  (About 5.35 sigma.)"""
    def mean(a, b):
        return sigma * math.sqrt(math.pi / 2) * (math.erf(b / (sigma * math.sqrt(2))) - math.erf(a / (sigma * math.sqrt(2)))) / (b - a)
    sides = np.arange(6.0, 120.0, 0.01)
    det = [((2 * mean(-L / 6, L / 6) - 2 * mean(L / 6, L / 2)) * mean(-5 * L / 18, 5 * L / 18)) ** 2 for L in sides]
    return float(sides[int(np.argmax(det))])


def test_restatement_finds_a_planted_blob():
    """A planted Gaussian blob comes out as the strongest keypoint, at its centre (within one sample of its octave) and
    with the size at which the box filters respond most to it (box_filter_argmax; within half the spacing of the layers of
    its octave, which is what a parabola through three layers can miss).  A bright blob has a negative trace (class_id -1),
    a dark one a positive.  Measured: sizes 22 and 33 for sigma 4 and 6, where the model says 21.4 and 32.1."""
    cx, cy = 100.0, 80.0
    for sigma, amplitude, sign, octave in ((4.0, 120.0, -1, 0), (6.0, 120.0, -1, 1), (4.0, -90.0, 1, 0)):
        kp = ref.detect(blob_image(200, 160, cx, cy, sigma, amplitude), ref.Params())
        assert len(kp) >= 1
        best = kp[0]
        want = box_filter_argmax(sigma)
        print("blob sigma %g, %+.0f: %d keypoints, best %s, model size %.2f" % (sigma, amplitude, len(kp), best, want))
        assert abs(best["x"] - cx) <= (1 << octave) and abs(best["y"] - cy) <= (1 << octave)
        assert abs(best["size"] - want) <= 0.5 * (ref.HAAR_SIZE_INC << octave)
        assert best["class_id"] == sign and best["octave"] == octave and best["angle"] == -1.0
        assert best["response"] > 10 * 500.0


def rotation_share(upright, n=150):
    """An image and its np.rot90 copy with the n strongest interior keypoints of the image mapped across: the share of
    keypoints whose row in the rotated copy has its own row in the image as the nearest of all n (L2)."""
    left, _, _ = ec.make_stereo_pair(51, width=400, height=300)
    img = np.ascontiguousarray(left)
    rot = np.ascontiguousarray(np.rot90(img))                  # rot[i, j] = img[j, W - 1 - i]
    h, w = img.shape
    kp = ref.detect(img, ref.Params())
    m = 60                                                     # every window and wavelet inside both images
    kp = kp[(kp["x"] > m) & (kp["x"] < w - m) & (kp["y"] > m) & (kp["y"] < h - m) & (kp["size"] <= 40)][:n]
    assert len(kp) == n
    kr = kp.copy()
    kr["x"], kr["y"] = kp["y"], np.float32(w - 1) - kp["x"]
    prm = ref.Params(upright=upright)
    ia, da, ka = ref.compute(img, kp, prm)
    ib, db, kb = ref.compute(rot, kr, prm)
    assert len(ia) == len(ib) == n
    d2 = ((db[:, None, :].astype(np.float64) - da[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
    share = float((d2.argmin(axis=1) == np.arange(n)).mean())
    turn = (kb["angle"].astype(np.float64) - ka["angle"].astype(np.float64)) % 360.0
    return share, turn


def test_restatement_rows_survive_an_in_plane_rotation():
    """With the orientation estimate most keypoints find their own row again after a rot90, and their angles turn by one
    and the same quarter; upright rows do not.  Measured: a share of 1.000 of 150 with upright 0 (every angle turns by 270
    degrees within 5, the orientation search's step), 0.013 with upright 1."""
    share, turn = rotation_share(0)
    err = np.minimum(np.abs(turn - 90.0), np.abs(turn - 270.0))
    print("upright 0: share %.3f, angle turns %s, within 5 degrees of a quarter turn: %d" % (
        share, np.round(np.median(turn), 1), (err <= 5.0).sum()))
    assert share >= 0.9                                                 # measured 1.000 (150 of 150)
    assert (np.abs(turn - np.median(turn)) <= 5.0).mean() >= 0.9
    assert min(abs(np.median(turn) - 90.0), abs(np.median(turn) - 270.0)) <= 5.0
    share1, _ = rotation_share(1)
    print("upright 1: share %.3f" % share1)
    assert share1 < 0.5                                                 # measured 0.013
