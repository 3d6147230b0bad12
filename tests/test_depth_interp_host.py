"""CPU: the NumPy restatement of the decimated depth path (tests/depth_interp_ref.py) against itself -- the sequential loops
of util2d::interpolate and the per-pixel form the kernel takes agree byte for byte -- and on inputs whose result is known
by hand; the scaled 3D points against depth_ref at equal sizes; the new symbols, sf_depth_size's layout and the ABI version
against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from tests import depth_interp_ref as iref
from tests import depth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, F32M = _abi.SF_DEPTH_U16_MM, _abi.SF_DEPTH_F32_M
NEW = ("sf_depth_set_size", "sf_depth_get_size", "sf_depth_interpolate_device", "sf_depth_interpolation_factor")


def random_depth(seed, w, h, fmt):
    """Smooth ramps with steps of 10 % and more, zeros, and the format's other holes (65535; NaN, inf, negative)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 1.5 + 0.02 * x + 0.015 * y + rng.normal(0.0, 0.004, (h, w))
    z[:, w // 2:] *= 1.0 + rng.uniform(0.1, 0.4)            # a step of at least 10 % down the middle
    z[h // 3:h // 3 + 2, :] *= 1.12
    hole = rng.random((h, w)) < 0.08
    kind = rng.integers(0, 4, (h, w))
    if fmt == U16:
        d = np.clip(np.rint(z * 1000.0), 1, 65534).astype(np.uint16)
        d[hole & (kind < 2)] = 0
        d[hole & (kind >= 2)] = 65535
        return d
    d = z.astype(np.float32)
    d[hole & (kind == 0)] = 0.0
    d[hole & (kind == 1)] = np.nan
    d[hole & (kind == 2)] = np.inf
    d[hole & (kind == 3)] = -1.0
    return d


@pytest.mark.parametrize("fmt", [U16, F32M], ids=["u16", "f32"])
@pytest.mark.parametrize("f", [2, 3, 4, 5])
def test_sequential_and_per_pixel_forms_agree(f, fmt):
    for seed, (w, h) in ((1, (13, 9)), (2, (8, 11))):
        d = random_depth(seed + 10 * f, w, h, fmt)
        a, b = iref.interpolate(d, f), iref.interpolate_per_pixel(d, f)
        assert a.shape == (h * f, w * f) and a.dtype == d.dtype
        assert a.tobytes() == b.tobytes()
        filled = float((iref.samples(a) > 0).mean())
        assert 0.2 < filled < 0.95, filled                  # cells written and cells refused in every image
    s = ref.scene(16, 12, 40, fmt)                          # the scenes of the GPU tests, with their four kinds of hole
    assert iref.interpolate(s, f).tobytes() == iref.interpolate_per_pixel(s, f).tobytes()


@pytest.mark.parametrize("fmt", [U16, F32M], ids=["u16", "f32"])
def test_factor_one_returns_the_input(fmt):
    d = random_depth(3, 9, 7, fmt)
    for form in (iref.interpolate, iref.interpolate_per_pixel):
        out = form(d, 1)
        assert out.tobytes() == d.tobytes() and out is not d


@pytest.mark.parametrize("f", [2, 4])
def test_an_exactly_representable_plane_interpolates_exactly(f):
    # z = 1024 + 64 a + 32 b at the samples: every slope over f = 2, 4 and every product is a small integer
    b, a = np.mgrid[0:5, 0:6]
    for dtype in (np.uint16, np.float32):
        d = (1024 + 64 * a + 32 * b).astype(dtype)
        out = iref.interpolate(d, f)
        y, x = np.mgrid[0:5 * f, 0:6 * f]
        want = np.where((x <= 5 * f) & (y <= 4 * f), 1024 + (64 // f) * x + (32 // f) * y, 0).astype(dtype)
        assert out.tobytes() == want.tobytes()


def test_a_step_leaves_a_zero_band_and_the_last_columns_and_rows_are_zero():
    f, w, h = 3, 8, 5
    d = np.full((h, w), 2000, np.uint16)
    d[:, 4:] = 2600                                         # 30 % against a bound of 10 % of the mean: cells a = 4 are invalid
    out = iref.interpolate(d, f)
    assert out.shape == (h * f, w * f)
    # the cells a = 4 cover x = 9 .. 12; x = 9 and 12 belong to their valid neighbours too: the band is x = 10, 11 (f - 1 wide)
    assert (out[:(h - 1) * f + 1, 10:12] == 0).all()
    assert (out[:(h - 1) * f + 1, :10] == 2000).all() and (out[:(h - 1) * f + 1, 12:(w - 1) * f + 1] == 2600).all()
    assert (out[:, (w - 1) * f + 1:] == 0).all() and (out[(h - 1) * f + 1:, :] == 0).all()   # the last f - 1 columns and rows
    assert out[(h - 1) * f, (w - 1) * f] == 2600            # ... and the pixel before them is written
    # a step below the bound interpolates across
    d[:, 4:] = 2100
    assert (iref.interpolate(d, f)[:(h - 1) * f + 1, :(w - 1) * f + 1] != 0).all()


def test_two_by_two_is_one_cell_and_a_single_row_or_column_is_empty():
    d = np.array([[1000, 1040], [1020, 1060]], np.uint16)
    out = iref.interpolate(d, 2)
    want = np.zeros((4, 4), np.uint16)
    want[:3, :3] = [[1000, 1020, 1040], [1010, 1030, 1050], [1020, 1040, 1060]]
    assert out.tobytes() == want.tobytes() == iref.interpolate_per_pixel(d, 2).tobytes()
    d[1, 1] = 0                                             # one corner absent: no cell at all
    assert not iref.interpolate(d, 2).any()
    for shape in ((1, 5), (5, 1)):
        line = np.full(shape, 1.5, np.float32)
        for form in (iref.interpolate, iref.interpolate_per_pixel):
            out = form(line, 2)
            assert out.shape == (2 * shape[0], 2 * shape[1]) and not out.any()


def test_the_factor_and_the_mask_of_a_size_that_does_not_divide():
    assert iref.factor(64, 48, 32, 24) == 2 and iref.factor(64, 48, 16, 12) == 4 and iref.factor(64, 48, 64, 48) == 1
    assert iref.factor(64, 48, 40, 24) == 0 and iref.factor(64, 48, 32, 12) == 0 and iref.factor(64, 48, 128, 96) == 0
    assert iref.factor(64, 48, 0, 24) == 0
    d = ref.scene(40, 24, 40, U16)
    assert iref.mask_decimated(d, 64, 48) is None
    d = ref.scene(32, 24, 40, U16)
    m = iref.mask_decimated(d, 64, 48, 0.8, 4.5)
    assert m.shape == (48, 64) and m.dtype == np.uint8
    assert m.tobytes() == ref.depth_mask(iref.interpolate(d, 2), 0.8, 4.5).tobytes()
    full = ref.scene(64, 48, 40, U16)
    assert iref.mask_decimated(full, 64, 48, 0.8, 4.5).tobytes() == ref.depth_mask(full, 0.8, 4.5).tobytes()


@pytest.mark.parametrize("fmt", [U16, F32M], ids=["u16", "f32"])
def test_scaled_points_equal_depth_ref_at_equal_sizes(fmt):
    w, h = 33, 21
    d = ref.scene(w, h, 7, fmt)
    rng = np.random.default_rng(8)
    xy = np.stack([rng.uniform(-2, w + 2, 200), rng.uniform(-2, h + 2, 200)], axis=1).astype(np.float32)
    xy[:3] = [[np.nan, 2], [w - 0.4, 3], [-0.7, -0.7]]
    for cam in (ref.camera(w, h), ref.camera(w, h, local=True, min_depth=0.8, max_depth=4.5), ref.camera(w, h, cx=0.0, cy=-2.0)):
        want = ref.keypoints3d_depth(xy, d, cam)
        got = iref.keypoints3d_depth_scaled(xy, d, cam, w, h)
        assert np.isfinite(want).any() and got.tobytes() == want.tobytes()
    # a smaller depth image: another result, finite where the small image holds a depth
    small = ref.scene(11, 7, 7, fmt)
    got = iref.keypoints3d_depth_scaled(xy, small, ref.camera(w, h), w, h)
    assert got.shape == (200, 3) and np.isfinite(got).any()


def test_new_symbols_are_declared_exported_and_bound():
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED
        assert re.search(r"\b%s\(" % name, hdr), name
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8 == L.sf_abi_version() == _abi.SF_ABI_VERSION
    for method in ("depth_set_size", "depth_get_size", "depth_interpolate_device"):
        assert callable(getattr(lib.SeparatorFinder, method))
    # the factor needs no handle and no GPU: the restatement's, case by case
    for args in ((64, 48, 32, 24), (64, 48, 16, 12), (64, 48, 64, 48), (64, 48, 40, 24), (64, 48, 32, 12), (64, 48, 128, 96),
                 (97, 131, 97, 131), (752, 480, 188, 120), (64, 48, 0, 0), (64, 48, -32, -24), (0, 0, 32, 24)):
        assert lib.depth_interpolation_factor(*args) == iref.factor(*args), args
    s = _abi.depth_size()
    assert (s.depth_width, s.depth_height) == (0, 0)
    s = _abi.depth_size(32, 24)
    assert (s.depth_width, s.depth_height) == (32, 24)


def test_depth_size_layout_matches_the_header(tmp_path):
    src = tmp_path / "depth_size.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sepfinder.h"\nint main(void){\n'
        ' printf("%zu %zu %zu %zu %d\\n", sizeof(sf_depth_size), offsetof(sf_depth_size, depth_width),'
        " offsetof(sf_depth_size, depth_height), sizeof(sf_params), SF_ABI_VERSION);\n return 0; }\n")
    exe = tmp_path / "depth_size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_abi.DepthSize), _abi.DepthSize.depth_width.offset, _abi.DepthSize.depth_height.offset,
                   C.sizeof(_abi.Params), _abi.SF_ABI_VERSION]
    assert got[0] == 8 and got[4] == 8
