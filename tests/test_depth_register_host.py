"""Depth registration, the part that needs no GPU: checks that the NumPy restatement the GPU tests compare with
(tests/depth_register_ref.py) IS registration and not merely consistent with itself -- an identity and shifts with exact
answers, the uint16 round trip, occlusion, every drop rule on planted values, independence of the scan order, the hole filling
on hand-made images -- then the host side of the C-ABI (the block's layout, defaults and refusals) and the conditions every
seeded scene of the GPU tests has to meet."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import depth_register_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ["sf_depth_registration_defaults", "sf_depth_register_check", "sf_depth_register_device", "sf_depth_fill_holes_device"]
K64 = (64.0, 64.0, 32.0, 24.0)                              # with depths that are powers of two every product is exact
W64, H48 = 64, 48


def exact_block(T=None, **kw):
    return ref.registration(W64, H48, K64, W64, H48, K64, T, **kw)


def shift_T(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(3, 4, dtype=F)
    T[:, 3] = (tx, ty, tz)
    return T


PZ_DROPPED = F(65.535)                                      # * 1000.0f = 65535.004: the smallest depth whose key is refused
PZ_KEPT = np.nextafter(PZ_DROPPED, F(0))                    # * 1000.0f = 65534.996: key 65534


def limit_T(pz):
    """The identity with T22 = pz: a sample of depth 1.0 at the principal point lands there with that depth."""
    T = np.eye(3, 4, dtype=F)
    T[2, 2] = pz
    return T


def powers_of_two(seed):
    rng = np.random.default_rng(seed)
    d = (2.0 ** rng.integers(-2, 4, size=(H48, W64))).astype(F)
    d[rng.random(d.shape) < 0.1] = 0.0
    return d


# ---- the restatement is registration -------------------------------------------------------------------------------------
def test_exact_identity_returns_the_image():
    d = powers_of_two(1)
    out = ref.register(d, exact_block())
    assert out.dtype == np.float32 and out.tobytes() == d.tobytes() and (d != 0).sum() > 2500


@pytest.mark.parametrize("s", [1, 3, -2])
def test_known_shift_moves_every_pixel_s_columns(s):
    """T03 = s / 32 at depth 2.0: u = (64 (X + s / 32)) / 2 + 32 = x + s, every step exact."""
    d = np.where(powers_of_two(2) != 0, F(2.0), F(0.0))
    out = ref.register(d, exact_block(shift_T(tx=s / 32.0)))
    want = np.zeros_like(d)
    if s > 0:
        want[:, s:] = d[:, :-s]
    else:
        want[:, :s] = d[:, -s:]
    assert out.tobytes() == want.tobytes()


def test_known_shift_of_rows_and_a_resize():
    d = np.where(powers_of_two(3) != 0, F(4.0), F(0.0))
    out = ref.register(d, exact_block(shift_T(ty=2 * 4.0 / 64.0)))          # v = y + 2
    want = np.zeros_like(d)
    want[2:] = d[:-2]
    assert out.tobytes() == want.tobytes()
    # the colour camera at twice the size: pixel (x, y) lands on (2 x, 2 y), everything else stays empty
    big = ref.registration(W64, H48, K64, 2 * W64, 2 * H48, (128.0, 128.0, 64.0, 48.0))
    out = ref.register(d, big)
    want = np.zeros((2 * H48, 2 * W64), F)
    want[::2, ::2] = d
    assert out.tobytes() == want.tobytes()


def test_uint16_round_trip_holds_for_every_value():
    """(int)(((float)v * 0.001f) * 1000.0f) == v for all 1 <= v <= 65534: a uint16 image registered under the exact identity
    block keeps its millimetres."""
    v = np.arange(1, 65535, dtype=np.uint16)
    back = np.trunc((v.astype(F) * F(0.001)) * F(1000.0)).astype(np.int64)
    assert (back == v).all()


def test_generic_identity_moves_some_pixels_to_the_left_or_upper_neighbour():
    """Truncation as upstream: with generic depths u = (rfx px) iz + rcx falls a rounding error short of x for about one pixel
    in ten, which then lands on its left (or upper) neighbour.  Documented, not repaired."""
    rng = np.random.default_rng(4)
    d = rng.integers(500, 6000, size=(H48, W64)).astype(np.uint16)
    ok, col, row, key = ref.project(d, exact_block())
    y, x = np.mgrid[0:H48, 0:W64]
    assert ok.all() and (key == d.ravel()).all()
    dx, dy = x.ravel() - col, y.ravel() - row
    assert set(np.unique(dx)) <= {0, 1} and set(np.unique(dy)) <= {0, 1}
    moved = float(((dx != 0) | (dy != 0)).mean())
    print("identity registration, generic depths: %.1f %% of the pixels land on a left or upper neighbour" % (100 * moved))
    assert 0.02 < moved < 0.25


@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_occlusion_the_near_value_wins(fmt):
    """A box at 1 m in front of a plane at 4 m, the colour camera 1 / 16 m to the side: the plane moves 1 column, the box 4.
    Where both land the box wins; where the box stood and nothing lands the image is empty."""
    d = np.full((H48, W64), 4.0, F)
    d[10:30, 20:40] = 1.0
    reg = exact_block(shift_T(tx=1.0 / 16.0))
    want = np.zeros_like(d)
    want[:, 1:] = 4.0
    want[10:30, 21:24] = 0.0                                 # behind the box in the depth image, not covered by the moved box
    want[10:30, 24:44] = 1.0                                 # columns 41 .. 43: the plane lands there too
    if fmt == "u16":
        d, want = (d * 1000).astype(np.uint16), (want * 1000).astype(np.uint16)
    out = ref.register(d, reg)
    assert out.tobytes() == want.tobytes()
    assert ref.collisions(d, reg) == 20 * 3


def planted_cases():
    """(name, depth image, block, expected image or None) of every drop rule; the GPU test runs the same list."""
    def one(value, x, y, dtype=F):
        d = np.zeros((H48, W64), dtype)
        d[y, x] = value
        return d

    def image(pixels, dtype=F):
        out = np.zeros((H48, W64), dtype)
        for (x, y), v in pixels.items():
            out[y, x] = v
        return out
    cases = [
        # u = x - 0.5: x = 0 gives u = -0.5, which truncates to column 0; x = 1 gives 0.5, column 0 as well
        ("u in (-1, 0)", one(2.0, 0, 5), exact_block(shift_T(tx=-0.5 / 32.0)), image({(0, 5): 2.0})),
        ("v in (-1, 0)", one(2.0, 7, 0), exact_block(shift_T(ty=-0.75 / 32.0)), image({(7, 0): 2.0})),
        ("u = -1 is outside", one(2.0, 0, 5), exact_block(shift_T(tx=-1.0 / 32.0)), image({})),
        ("u = W - 0.5 is inside", one(2.0, 63, 5), exact_block(shift_T(tx=0.5 / 32.0)), image({(63, 5): 2.0})),
        ("u = W is outside", one(2.0, 63, 5), exact_block(shift_T(tx=1.0 / 32.0)), image({})),
        ("v = H is outside", one(2.0, 9, 47), exact_block(shift_T(ty=1.0 / 32.0)), image({})),
        ("pz < 0", one(2.0, 30, 20), exact_block(shift_T(tz=-3.0)), image({})),
        ("pz = 0", one(2.0, 30, 20), exact_block(shift_T(tz=-2.0)), image({})),
        ("pz > 0 behind a moved camera", one(2.0, 32, 24), exact_block(shift_T(tz=-1.0)), image({(32, 24): 1.0})),
        ("uint16 key 66000", one(60000, 32, 24, np.uint16), exact_block(shift_T(tz=6.0)), image({}, np.uint16)),
        # the limit m < 65535.0f at adjacent floats: sample 1000 is dz = 1.0f exactly, so pz = T22 (limit_T)
        ("uint16 key just above 65535", one(1000, 32, 24, np.uint16), exact_block(limit_T(PZ_DROPPED)), image({}, np.uint16)),
        ("uint16 key just below 65535", one(1000, 32, 24, np.uint16), exact_block(limit_T(PZ_KEPT)), image({(32, 24): 65534}, np.uint16)),
        ("uint16 key 0", one(1, 32, 24, np.uint16), exact_block(shift_T(tz=-0.0005)), image({}, np.uint16)),
        ("float32 beyond the uint16 range", one(100.0, 32, 24), exact_block(), image({(32, 24): 100.0})),
    ]
    bad16 = np.zeros((H48, W64), np.uint16)
    bad16[::2] = 65535
    cases.append(("uint16 0 and 65535", bad16, exact_block(), image({}, np.uint16)))
    bad32 = np.zeros((H48, W64), F)
    for i, v in enumerate((np.nan, np.inf, -np.inf, -1.0, -0.0)):
        bad32[i::6] = v
    cases.append(("float32 0, NaN, inf and negative", bad32, exact_block(), image({})))
    return cases


def test_planted_cases_drop_and_land_as_written():
    for name, d, reg, want in planted_cases():
        out = ref.register(d, reg)
        assert out.dtype == d.dtype and out.shape == (reg["H"], reg["W"]), name
        if want is not None:
            assert out.tobytes() == want.tobytes(), name
    # the uint16 limit itself.  No float32 pz gives pz * 1000.0f == 65535.0f: the product steps from 65534.996 to 65535.004
    # between two adjacent floats, and those two are the planted pair -- the lower one kept with key 65534, the upper dropped
    assert np.nextafter(PZ_DROPPED, F(0)) == PZ_KEPT and F(1000) * F(0.001) == F(1.0)
    assert PZ_KEPT * F(1000.0) < F(65535.0) < PZ_DROPPED * F(1000.0)
    assert F(65535.0) - PZ_KEPT * F(1000.0) < 0.004 and PZ_DROPPED * F(1000.0) - F(65535.0) < 0.004


@pytest.mark.parametrize("fmt", [ref.U16, ref.F32M])
def test_the_result_does_not_depend_on_the_scan_order(fmt):
    name, dw, dh, W, H, _ = ref.CASES[2]                    # shrinking: nearly every pixel collides
    d, reg = ref.case_scene(name, ref.SEEDS[0], fmt), ref.case_registration(dw, dh, W, H)
    want = ref.register_unfilled(d, reg)
    n = dw * dh
    assert ref.collisions(d, reg) > 1000
    for order in (None, range(n - 1, -1, -1), np.random.default_rng(5).permutation(n)):
        assert ref.register_sequential(d, reg, order).tobytes() == want.tobytes()


# ---- the hole filling ----------------------------------------------------------------------------------------------------
def grid5(fmt, rows):
    a = np.array(rows, np.float64)
    return a.astype(np.uint16) if fmt == "u16" else (a / 1000.0).astype(F)


def val(fmt, mm):
    return np.uint16(mm) if fmt == "u16" else (np.array([mm], np.float64) / 1000.0).astype(F)[0]


@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_fill_on_hand_made_images(fmt):
    z = 0
    # a single hole between 1000 above and 1010 below: filled with their mean by the vertical pair only
    A = grid5(fmt, [[z] * 5, [z, z, 1000, z, z], [z, z, z, z, z], [z, z, 1010, z, z], [z] * 5])
    out = ref.fill_holes(A, 1, 0)
    want = A.copy()
    want[2, 2] = np.uint16(1005) if fmt == "u16" else (A[1, 2] + A[3, 2]) / F(2.0)
    assert out.tobytes() == want.tobytes()
    assert ref.fill_holes(A, 0, 1).tobytes() == A.tobytes() and ref.fill_holes(A, 0, 0).tobytes() == A.tobytes()
    assert ref.fill_holes(A.T.copy(), 0, 1).tobytes() == want.T.copy().tobytes()
    # a leaked far value (3000 between two of about 1000) is replaced; one that is not far (1015 > 1010 + 10.05 fails) stays
    B = A.copy()
    B[2, 2] = val(fmt, 3000)
    assert ref.fill_holes(B, 1, 0).tobytes() == want.tobytes()
    B[2, 2] = val(fmt, 1015)
    assert ref.fill_holes(B, 1, 1).tobytes() == B.tobytes()
    B[2, 2] = val(fmt, 900)                                  # nearer than the pair: stays
    assert ref.fill_holes(B, 1, 1).tobytes() == B.tobytes()
    # a pair that is not close (1000 and 1030: |a - c| = 30 > 0.01 * 1015) leaves the hole alone
    Cn = grid5(fmt, [[z] * 5, [z, z, 1000, z, z], [z, z, z, z, z], [z, z, 1030, z, z], [z] * 5])
    assert ref.fill_holes(Cn, 1, 1).tobytes() == Cn.tobytes()
    # border rows and columns are copied whatever their neighbours hold
    full = grid5(fmt, [[1000] * 5] * 5)
    for x, y in ((0, 2), (4, 2), (2, 0), (2, 4), (0, 0)):
        D = full.copy()
        D[y, x] = 0
        assert ref.fill_holes(D, 1, 1).tobytes() == D.tobytes(), (x, y)
    # vertical is taken before horizontal: 1000 / 1010 above and below, 2000 / 2010 left and right
    E = grid5(fmt, [[z] * 5, [z, z, 1000, z, z], [z, 2000, z, 2010, z], [z, z, 1010, z, z], [z] * 5])
    both, horizontal = ref.fill_holes(E, 1, 1), ref.fill_holes(E, 0, 1)
    assert both[2, 2] == want[2, 2] and horizontal[2, 2] == (np.uint16(2005) if fmt == "u16" else (E[2, 1] + E[2, 3]) / F(2.0))
    # ... and horizontal is taken where the vertical pair does not set the pixel
    E[3, 2] = 0
    assert ref.fill_holes(E, 1, 1)[2, 2] == horizontal[2, 2]
    # out of place: two adjacent holes stay holes (in place, the first one filled would fill the second)
    G = grid5(fmt, [[1000] * 5, [1000, 1000, 1000, 1000, 1000], [1000, z, z, 1000, 1000], [1000] * 5, [1000] * 5])
    out = ref.fill_holes(G, 0, 1)
    assert out[2, 1] == 0 and out[2, 2] == 0
    out = ref.fill_holes(G, 1, 1)                            # (each has a vertical pair of its own)
    assert out[2, 1] == val(fmt, 1000) and out[2, 2] == val(fmt, 1000)
    Gv = G.T.copy()
    out = ref.fill_holes(Gv, 1, 0)
    assert out[1, 2] == 0 and out[2, 2] == 0


def test_fill_uint16_uses_integer_means_and_float_bounds():
    A = np.zeros((3, 3), np.uint16)
    A[0, 1], A[2, 1] = 1001, 1004                            # m = 1002 (integer division), e = 10.02
    assert ref.fill_holes(A, 1, 0)[1, 1] == 1002
    A[0, 1], A[2, 1] = 100, 101                              # |a - c| = 1 <= 0.01f * 100 = 1.0 (as float32: just below or at 1)
    e = F(0.01) * F(100)
    assert (ref.fill_holes(A, 1, 0)[1, 1] == 100) == bool(F(1) <= e)
    A[0, 1], A[2, 1] = 65534, 65534                          # no wrap in the sum
    assert ref.fill_holes(A, 1, 0)[1, 1] == 65534


# ---- the host side of the C-ABI ------------------------------------------------------------------------------------------
def test_header_abi_and_binding_agree(tmp_path):
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    exp = open(os.path.join(ROOT, "include", "sf_experimental.h")).read()
    for name in NEW + ["sf_debug_depth_register_limits"]:
        assert hasattr(L, name) and name in lib.EXPORTED and getattr(L, name).argtypes is not None, name
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert re.search(r"\bsf_debug_depth_register_limits\s*\(", exp)
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _abi.SF_ABI_VERSION == 8 and L.sf_abi_version() == 8
    for method in ("depth_register_device", "depth_fill_holes_device", "depth_register"):
        assert hasattr(lib.SeparatorFinder, method)
    assert callable(lib.depth_registration) and callable(lib.depth_register_check)
    fields = [name for name, _ in _abi.DepthRegistration._fields_]
    src = tmp_path / "reg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sepfinder.h"\n'
                   'int main(void){printf("%zu %zu", sizeof(sf_depth_registration), sizeof(sf_params));\n' +
                   "".join('printf(" %%zu", offsetof(sf_depth_registration, %s));\n' % f for f in fields) +
                   'printf("\\n"); return 0;}\n')
    exe = tmp_path / "reg"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_abi.DepthRegistration), C.sizeof(_abi.Params)] + [getattr(_abi.DepthRegistration, f).offset for f in fields]
    assert got[0] == 108 and got[1] == 232


def test_defaults_are_the_identity_without_fills():
    L = lib.load()
    r = _abi.DepthRegistration()
    C.memset(C.byref(r), 0xEE, C.sizeof(r))
    L.sf_depth_registration_defaults(C.byref(r))
    assert list(r.transform) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert (r.fill_vertical, r.fill_horizontal, r.reserved) == (0, 0, 0)
    assert (r.depth_width, r.depth_height, r.width, r.height, r.fx, r.rcy) == (0, 0, 0, 0, 0.0, 0.0)
    assert lib.depth_register_check(r)[0] == _abi.SF_EINVAL           # sizes and intrinsics are the caller's to fill in
    assert list(ref.abi(exact_block()).transform) == list(r.transform)


def refusals():
    """(name, block, why the restatement refuses it) of every block sf_depth_register_check refuses; the GPU test runs the
    same list through sf_depth_register_device."""
    base = ref.case_registration(64, 48, 96, 72, 1, 1)

    def make(**kw):
        reg = dict(base, T=base["T"].copy())
        for key, value in kw.items():
            if key in ("k", "rk"):
                vals = list(reg[key])
                vals[value[0]] = F(value[1])
                reg[key] = tuple(vals)
            elif key == "T":
                reg["T"][value[0]] = value[1]
            else:
                reg[key] = value
        return reg
    out = [("depth width 0", make(dw=0)), ("depth height 8193", make(dh=8193)), ("width -1", make(W=-1)), ("height 8193", make(H=8193)),
           ("width 0", make(W=0)), ("nan fx", make(k=(0, np.nan))), ("inf cy", make(k=(3, np.inf))), ("-inf rcx", make(rk=(2, -np.inf))),
           ("nan rfy", make(rk=(1, np.nan))), ("nan in T", make(T=((1, 2), np.nan))), ("inf in T", make(T=((2, 3), np.inf))),
           ("fx 0", make(k=(0, 0.0))), ("fy < 0", make(k=(1, -50.0))), ("rfx < 0", make(rk=(0, -1.0))), ("rfy 0", make(rk=(1, 0.0))),
           ("fill_vertical 2", make(fill_vertical=2)), ("fill_horizontal -1", make(fill_horizontal=-1))]
    return [(name, ref.abi(reg), ref.check(reg)) for name, reg in out] + [("reserved", ref.abi(base, reserved=1), "reserved")]


def test_the_check_refuses_what_the_restatement_refuses():
    L = lib.load()
    cases = refusals()
    assert len(cases) == 18 and all(why for _, _, why in cases)
    assert {why for _, _, why in cases} == {"size", "finite", "focal", "flag", "reserved"}
    for name, block, _ in cases:
        assert L.sf_depth_register_check(C.byref(block)) == _abi.SF_EINVAL, name
        assert len(L.sf_last_error(None)) > 10 and b"sf_depth_register_check" in L.sf_last_error(None), name
        rc, text = lib.depth_register_check(block)
        assert rc == _abi.SF_EINVAL and text, name
    assert L.sf_depth_register_check(None) == _abi.SF_EINVAL
    for fills in ((0, 0), (1, 0), (0, 1), (1, 1)):
        reg = ref.case_registration(64, 48, 96, 72, *fills)
        assert ref.check(reg) is None and lib.depth_register_check(ref.abi(reg)) == (_abi.SF_OK, "")
    edge = ref.registration(8192, 1, (1e-3, 1e6, -5.0, 1e9), 1, 8192, (0.5, 0.5, 0.0, 0.0))
    assert lib.depth_register_check(ref.abi(edge))[0] == _abi.SF_OK and ref.check(edge) is None


def test_the_binding_builds_the_block_the_restatement_describes():
    reg = ref.case_registration(67, 45, 93, 71, 1, 0)
    r = ref.abi(reg)
    assert (r.depth_width, r.depth_height, r.width, r.height) == (67, 45, 93, 71)
    assert (F(r.fx), F(r.fy), F(r.cx), F(r.cy)) == reg["k"] and (F(r.rfx), F(r.rfy), F(r.rcx), F(r.rcy)) == reg["rk"]
    assert np.array_equal(np.array(list(r.transform), F).reshape(3, 4), reg["T"])
    assert (r.fill_vertical, r.fill_horizontal, r.reserved) == (1, 0, 0)


# ---- the seeded scenes of the GPU tests ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [ref.U16, ref.F32M])
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c[0])
def test_every_scene_of_the_gpu_tests_meets_its_conditions(case, fmt):
    """At least 20 output pixels with two or more contributors of unlike key in every scene, and under every combination of
    flags at least 20 empty pixels filled and at least 5 values replaced."""
    name, dw, dh, W, H, _ = case
    reg = ref.case_registration(dw, dh, W, H)
    for seed in ref.SEEDS:
        d = ref.case_scene(name, seed, fmt)
        A = ref.register_unfilled(d, reg)
        n = ref.collisions(d, reg)
        stats = {fl: ref.fill_stats(A, ref.fill_holes(A, fl & 1, fl >> 1)) for fl in (1, 2, 3)}
        print("%s format %d seed %d: %d collisions, %d pixels set, (filled, replaced) %s" % (name, fmt, seed, n, int((A != 0).sum()), stats))
        assert n >= 20 and (A != 0).sum() > W * H // 4
        for fl, (filled, replaced) in stats.items():
            assert filled >= 20 and replaced >= 5, (seed, fl, filled, replaced)
        # the image has every kind of absent sample
        if fmt == ref.U16:
            assert (d == 0).any() and (d == 65535).any()
        else:
            assert (d == 0).any() and np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d < 0).any()
