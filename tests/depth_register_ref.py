"""NumPy restatement of depth registration (include/sepfinder.h, "depth registration"; csrc/k_depth_register.hip): upstream
rtabmap's util2d::registerDepth and util2d::fillRegisteredDepthHoles(fillDoubleHoles = false), as remembered -- neither is in
the reference tree.  A depth image measured in the depth camera's frame is projected pixel by pixel into the colour camera
and every output pixel keeps the nearest point that lands on it; then single holes are filled from the pair above and below
or left and right, and a value far behind such a pair (background seen through a sparser foreground) is replaced.

All arithmetic is float32, one rounded operation per step in the order written (NumPy's float32 operators are exactly that).
What this restatement decides where upstream differs:
  * a sample is present under the depth calls' rule (uint16 0 < v < 65535; float32 finite and > 0); upstream takes dz >= 0,
    so every empty pixel projects the camera origin;
  * a point with pz <= 0 is dropped; upstream does not test pz;
  * a uint16 key of 65535 or more is dropped; upstream lets the cast wrap;
  * a key of 0 is dropped; upstream lets it reset a pixel, which makes its result depend on the scan order;
  * the fill is out of place: it reads the unfilled image only; upstream fills in place, columns outer;
  * double holes are not filled;
  * (int)u and (int)v truncate toward zero as upstream: values in (-1, 0) land in column or row 0, and an identity
    registration moves about one pixel in ten to its left or upper neighbour, because u falls a rounding error short of x."""
import numpy as np

from multi_robot_slam_separators_amd import _abi

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
U16, F32M = _abi.SF_DEPTH_U16_MM, _abi.SF_DEPTH_F32_M


def registration(dw, dh, depth_k, W, H, colour_k, T=None, fill_vertical=0, fill_horizontal=0):
    """The block as a dict: sizes, (fx, fy, cx, cy), (rfx, rfy, rcx, rcy), T [3, 4] float32 (None: identity), the fill flags."""
    T = np.eye(3, 4, dtype=F) if T is None else np.asarray(T, F).reshape(3, 4).copy()
    return {"dw": int(dw), "dh": int(dh), "W": int(W), "H": int(H), "k": tuple(F(v) for v in depth_k), "rk": tuple(F(v) for v in colour_k),
            "T": T, "fill_vertical": int(fill_vertical), "fill_horizontal": int(fill_horizontal)}


def abi(reg, **over):
    """The _abi.DepthRegistration of a block (over: fields set afterwards, for the refusals)."""
    r = _abi.depth_registration(reg["dw"], reg["dh"], reg["k"], reg["W"], reg["H"], reg["rk"], reg["T"], reg["fill_vertical"],
                                reg["fill_horizontal"])
    for name, value in over.items():
        if name.startswith("transform"):
            r.transform[int(name[9:])] = value
        else:
            setattr(r, name, value)
    return r


def check(reg):
    """None, or why sf_depth_register_check refuses the block."""
    for name in ("dw", "dh", "W", "H"):
        if not 1 <= reg[name] <= 8192:
            return "size"
    if not all(np.isfinite(v) for v in reg["k"] + reg["rk"]) or not np.isfinite(reg["T"]).all():
        return "finite"
    if not (reg["k"][0] > 0 and reg["k"][1] > 0 and reg["rk"][0] > 0 and reg["rk"][1] > 0):
        return "focal"
    if reg["fill_vertical"] not in (0, 1) or reg["fill_horizontal"] not in (0, 1):
        return "flag"
    return None


def project(depth, reg):
    """Every depth pixel in row-major order: (landed [n] bool, column [n], row [n], key [n] uint32); column, row and key are
    meaningful where landed."""
    depth = np.asarray(depth)
    dh, dw = depth.shape
    assert (dw, dh) == (reg["dw"], reg["dh"]) and depth.dtype in (np.uint16, np.float32)
    fx, fy, cx, cy = reg["k"]
    rfx, rfy, rcx, rcy = reg["rk"]
    T = reg["T"]
    y, x = np.mgrid[0:dh, 0:dw]
    x, y = x.ravel().astype(F), y.ravel().astype(F)
    v = depth.ravel()
    with np.errstate(all="ignore"):
        if depth.dtype == np.uint16:
            present = (v > 0) & (v < 65535)
            dz = v.astype(F) * F(0.001)
        else:
            present = np.isfinite(v) & (v > 0)
            dz = v.astype(F)
        dz = np.where(present, dz, F(1.0))                  # (any value: the point is dropped)
        X = ((x - cx) * dz) / fx
        Y = ((y - cy) * dz) / fy
        px = ((T[0, 0] * X + T[0, 1] * Y) + T[0, 2] * dz) + T[0, 3]
        py = ((T[1, 0] * X + T[1, 1] * Y) + T[1, 2] * dz) + T[1, 3]
        pz = ((T[2, 0] * X + T[2, 1] * Y) + T[2, 2] * dz) + T[2, 3]
        assert px.dtype == py.dtype == pz.dtype == F
        ok = present & (pz > 0)
        iz = F(1.0) / np.where(ok, pz, F(1.0))
        u = (rfx * px) * iz + rcx
        w = (rfy * py) * iz + rcy
        assert u.dtype == w.dtype == F
        ok &= (u > -1) & (u < F(reg["W"])) & (w > -1) & (w < F(reg["H"]))
        col = np.trunc(np.where(ok, u, F(0))).astype(np.int64)
        row = np.trunc(np.where(ok, w, F(0))).astype(np.int64)
        if depth.dtype == np.uint16:
            m = pz * F(1000.0)
            ok &= m < F(65535.0)
            key = np.trunc(np.where(ok, m, F(0))).astype(np.int64)
            ok &= key != 0
            key = key.astype(np.uint32)
        else:
            key = pz.view(np.uint32).copy()
    return ok, col, row, key


def from_keys(keys, dtype, W, H):
    out = np.where(keys == EMPTY, np.uint32(0), keys).reshape(H, W)
    return out.astype(np.uint16) if dtype == np.uint16 else out.view(np.float32)


def register_unfilled(depth, reg):
    """The registered image before the hole filling: per output pixel the smallest key, or 0."""
    ok, col, row, key = project(depth, reg)
    keys = np.full(reg["W"] * reg["H"], EMPTY, np.uint32)
    np.minimum.at(keys, (row * reg["W"] + col)[ok], key[ok])
    return from_keys(keys, np.asarray(depth).dtype, reg["W"], reg["H"])


def register_sequential(depth, reg, order=None):
    """The same as upstream's loop writes it: the points visited one by one in `order` (indices into the row-major scan; None:
    row-major), each written where the pixel is empty or holds a larger value."""
    ok, col, row, key = project(depth, reg)
    out = np.zeros((reg["H"], reg["W"]), np.uint32)
    for i in (range(len(ok)) if order is None else order):
        if ok[i] and (out[row[i], col[i]] == 0 or key[i] < out[row[i], col[i]]):
            out[row[i], col[i]] = key[i]
    return out.astype(np.uint16) if np.asarray(depth).dtype == np.uint16 else out.view(np.float32)


def _pair(a, b, c):
    """(sets, m) of one pair (a, c) around b, elementwise."""
    with np.errstate(all="ignore"):
        if a.dtype == np.uint16:
            ia, ib, ic = a.astype(np.int64), b.astype(np.int64), c.astype(np.int64)
            m = (ia + ic) // 2
            e = F(0.01) * m.astype(F)
            close = np.abs(ia - ic).astype(F) <= e
            far = (ib.astype(F) > ia.astype(F) + e) & (ib.astype(F) > ic.astype(F) + e)
            return (ia != 0) & (ic != 0) & close & ((ib == 0) | far), m.astype(np.uint16)
        m = (a + c) / F(2.0)
        e = F(0.01) * m
        close = np.abs(a - c) <= e
        far = (b > a + e) & (b > c + e)
        assert m.dtype == e.dtype == F
        return (a != 0) & (c != 0) & close & ((b == 0) | far), m


def fill_holes(A, fill_vertical, fill_horizontal):
    """fillRegisteredDepthHoles(fillDoubleHoles = false), out of place: every pixel from the unfilled image A alone."""
    A = np.asarray(A)
    out = A.copy()
    H, W = A.shape
    if H < 3 or W < 3:
        return out
    b = A[1:-1, 1:-1]
    done = np.zeros(b.shape, bool)
    inner = out[1:-1, 1:-1]
    if fill_vertical:
        sets, m = _pair(A[:-2, 1:-1], b, A[2:, 1:-1])
        inner[sets] = m[sets]
        done = sets
    if fill_horizontal:
        sets, m = _pair(A[1:-1, :-2], b, A[1:-1, 2:])
        sets = sets & ~done
        inner[sets] = m[sets]
    return out


def register(depth, reg):
    """sf_depth_register_device on one image."""
    return fill_holes(register_unfilled(depth, reg), reg["fill_vertical"], reg["fill_horizontal"])


def collisions(depth, reg):
    """Output pixels on which two or more points of unlike key land."""
    ok, col, row, key = project(depth, reg)
    pairs = np.unique(((row * reg["W"] + col)[ok] << 32) | key[ok].astype(np.int64))     # (pixel, key), each once
    return int((np.bincount(pairs >> 32) >= 2).sum())


def fill_stats(A, filled):
    """(zero pixels filled, non-zero pixels replaced) between an unfilled image and its filled form."""
    a, f = A.view(np.uint32) if A.dtype == np.float32 else A, filled.view(np.uint32) if filled.dtype == np.float32 else filled
    return int(((a == 0) & (f != 0)).sum()), int(((a != 0) & (f != a)).sum())


# ---- seeded inputs -------------------------------------------------------------------------------------------------------
# (name, depth width, depth height, W, H, whether the scene is the lattice one): the smallest sizes at which each path can
# still go wrong -- enlarging gives a sparse result on which the fill matters; shrinking makes nearly every pixel collide; the
# odd size runs the element-wise loads and stores; the last one feeds the depth keyframe calls at the smallest image that holds
# BRIEF patches (tests/test_gpu_depth.py).  Every case runs under every combination of fill flags.  Shrinking by two covers
# single-pixel holes and leaves nothing to fill, so that case takes the lattice scene: a foreground of bars two pixels wide
# with the background visible between them, and holes in blocks of 3 x 3
CASES = (("64x48_96x72", 64, 48, 96, 72, False), ("80x60_80x60", 80, 60, 80, 60, False), ("96x64_48x32", 96, 64, 48, 32, True),
         ("67x45_93x71", 67, 45, 93, 71, False), ("80x108_97x131", 80, 108, 97, 131, False))
SEEDS = (70, 71, 72)                                        # the three scenes of a batch


def case_scene(name, seed, fmt=U16):
    """The seeded scene of a case of CASES."""
    _, dw, dh, _, _, lattice = [c for c in CASES if c[0] == name][0]
    return scene(dw, dh, seed, fmt, lattice)


def case_registration(dw, dh, W, H, fill_vertical=0, fill_horizontal=0):
    """Two cameras of the same field of view, the colour camera 8 cm to the side, 4 cm below and turned by one degree about
    its y axis: with the scenes below every condition tests/test_depth_register_host.py sets (collisions, pixels filled and
    replaced under each flag) holds on every case."""
    a = np.deg2rad(1.0)
    T = np.array([[np.cos(a), 0.0, np.sin(a), -0.08], [0.0, 1.0, 0.0, 0.04], [-np.sin(a), 0.0, np.cos(a), 0.002]], F)
    return registration(dw, dh, (0.9 * dw, 0.92 * dw, dw / 2.0 - 0.25, dh / 2.0 + 0.5), W, H,
                        (0.9 * W, 0.92 * W, W / 2.0 - 0.25, H / 2.0 + 0.5), T, fill_vertical, fill_horizontal)


def scene(dw, dh, seed, fmt=U16, lattice=False):
    """A sloped plane at about 3 m with a box at about 0.6 m in front of it and 5 % holes of every kind (uint16: 0 and 65535;
    float32: 0, NaN, +inf, -inf and a negative value).  lattice: the box is bars two pixels wide, two apart -- upright in its
    left half, level in its right half -- with the plane seen between them, and 15 % of the 3 x 3 blocks are holes too."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    z = 3.0 + rng.uniform(-0.2, 0.2) + 0.4 * x / dw + 0.25 * y / dh
    x0, y0 = int(dw * rng.uniform(0.2, 0.35)), int(dh * rng.uniform(0.15, 0.25))
    box = (x >= x0) & (x < x0 + int(0.5 * dw)) & (y >= y0) & (y < y0 + int(0.65 * dh))
    if lattice:
        box &= np.where(x < x0 + int(0.25 * dw), (x // 2) % 2 == 0, (y // 2) % 2 == 0)
    z[box] = 0.6 + rng.uniform(-0.05, 0.05) + 0.05 * x[box] / dw + 0.04 * y[box] / dh
    z = z + rng.normal(0.0, 0.002, z.shape)
    holes = rng.random((dh, dw)) < 0.05
    if lattice:
        by, bx = np.mgrid[0:dh, 0:dw] // 3
        holes |= rng.random((dh // 3 + 1, dw // 3 + 1))[by, bx] < 0.15
    kind = np.where(holes, rng.integers(1, 6, size=(dh, dw)), 0)
    if fmt == U16:
        d = np.clip(np.rint(z * 1000.0), 1, 65534).astype(np.uint16)
        d[(kind == 1) | (kind == 3) | (kind == 5)] = 0
        d[(kind == 2) | (kind == 4)] = 65535
        return d
    d = z.astype(np.float32)
    for k, value in ((1, 0.0), (2, np.nan), (3, np.inf), (4, -np.inf), (5, -1.5)):
        d[kind == k] = value
    return d
