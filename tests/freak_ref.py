"""NumPy restatement of the FREAK descriptors (Vis/FeatureType 3 and 5, csrc/k_freak.hip): cv::xfeatures2d::FREAK::compute
on given keypoints (DESIGN.md section 3 item 17g lists what the restatement decides).

Float64 where upstream's buildPattern is double (every table value rounded to float32 once), float32 where its
per-keypoint arithmetic is float (the sampling positions, the box limits before the + 0.5), integers where it is integer
(the field means, the orientation sums with their truncating divisions, the comparisons).  The one log and the one atan2
of a keypoint are float64, rounded to float32 once."""
import math

import numpy as np

from tests import orb_ref

F32 = np.float32
F64 = np.float64
SCALES, ORIENTATIONS, POINTS, PAIRS, ORIENT_PAIRS, ALL_PAIRS, BYTES = 64, 256, 43, 512, 45, 903, 64
SMALLEST_KP_SIZE = 7
LOG2 = 0.693147180559945
RING_POINTS = [6, 6, 6, 6, 6, 6, 6, 1]
DEFAULT_PAIRS_SEED = 0x46524B21


class Params:
    def __init__(self, orientation_normalized=1, scale_normalized=1, pattern_scale=22.0, n_octaves=4):
        self.orientation_normalized = int(orientation_normalized)
        self.scale_normalized = int(scale_normalized)
        self.pattern_scale = float(F32(pattern_scale))
        self.n_octaves = int(n_octaves)


def rings():
    """(radius [8], sigma [8]) of the rings, outer to inner, in units of the pattern scale."""
    big, small = 2.0 / 3.0, 2.0 / 24.0
    unit = (big - small) / 21.0
    radius = [big, big - 6 * unit, big - 11 * unit, big - 15 * unit, big - 18 * unit, big - 20 * unit, small, 0.0]
    sigma = [r / 2.0 for r in radius[:7]] + [radius[6] / 2.0]
    return radius, sigma


def size_products(params):
    """The real-valued (radius + sigma) f pattern_scale of every scale and ring, [64, 8]: sizes = ceil of it, + 1."""
    radius, sigma = rings()
    step = math.pow(2.0, params.n_octaves / float(SCALES))
    return np.array([[(radius[i] + sigma[i]) * math.pow(step, float(s)) * params.pattern_scale for i in range(8)]
                     for s in range(SCALES)])


def build_pattern(params):
    """FREAK::buildPattern: table float32 [64, 256, 43, 3] = (x, y, sigma), sizes int32 [64]."""
    radius, sigma = rings()
    step = math.pow(2.0, params.n_octaves / float(SCALES))
    theta = np.arange(ORIENTATIONS, dtype=F64) * 2 * np.pi / float(ORIENTATIONS)
    table = np.zeros((SCALES, ORIENTATIONS, POINTS, 3), F32)
    for s in range(SCALES):
        f = math.pow(step, float(s))
        p = 0
        for i in range(8):
            n = RING_POINTS[i]
            beta = np.pi / n * (i % 2)
            for k in range(n):
                alpha = float(k) * 2 * np.pi / float(n) + beta + theta
                table[s, :, p, 0] = (radius[i] * np.cos(alpha) * f * params.pattern_scale).astype(F32)
                table[s, :, p, 1] = (radius[i] * np.sin(alpha) * f * params.pattern_scale).astype(F32)
                table[s, :, p, 2] = F32(sigma[i] * f * params.pattern_scale)
                p += 1
    sizes = (np.ceil(size_products(params)).astype(np.int64).max(axis=1) + 1).astype(np.int32)
    return table, sizes


def orientation_pair_indices():
    base = [(0, 3), (1, 4), (2, 5), (0, 2), (1, 3), (2, 4), (3, 5), (4, 0), (5, 1)]
    out = [(i + 6 * r, j + 6 * r) for r in range(4) for i, j in base]
    out += [(24, 27), (25, 28), (26, 29), (30, 33), (31, 34), (32, 35), (36, 39), (37, 40), (38, 41)]
    return out


def orientation_pairs(table):
    """[45, 4] = i, j, weight_dx, weight_dy from the float32 points of scale 0 / orientation 0 ((int) truncates)."""
    pts = np.asarray(table, F32)[0, 0]
    out = np.zeros((ORIENT_PAIRS, 4), np.int64)
    for m, (i, j) in enumerate(orientation_pair_indices()):
        dx = F32(pts[i, 0] - pts[j, 0])
        dy = F32(pts[i, 1] - pts[j, 1])
        nsq = F32(F32(dx * dx) + F32(dy * dy))
        out[m] = (i, j, int(float(F32(dx / nsq)) * 4096.0 + 0.5), int(float(F32(dy / nsq)) * 4096.0 + 0.5))
    return out


def all_pairs():
    """The 903 pairs in upstream's enumeration: for i in 1..42: for j in 0..i-1; index = i (i - 1) / 2 + j."""
    return np.array([(i, j) for i in range(1, POINTS) for j in range(i)], np.int64)


def default_pairs():
    """The generated selection of a fresh handle: a[k] <-> a[k + next() % (903 - k)] for k = 0 .. 511 on a = 0 .. 902, next()
    the low word of cv::RNG's multiply-with-carry state from DEFAULT_PAIRS_SEED; the first 512 of a.  NOT FREAK_DEF_PAIRS."""
    s = DEFAULT_PAIRS_SEED
    a = list(range(ALL_PAIRS))
    for k in range(PAIRS):
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) & 0xFFFFFFFFFFFFFFFF
        r = k + (s & 0xFFFFFFFF) % (ALL_PAIRS - k)
        a[k], a[r] = a[r], a[k]
    return np.array(a[:PAIRS], np.int32)


def bit_position(c):
    """(byte, bit) of description pair c: upstream's SSE order, c = 128 q + 16 r + u -> bit r of byte 16 q + 15 - u."""
    q, r, u = c >> 7, (c >> 4) & 7, c & 15
    return 16 * q + 15 - u, r


def size_cst(params):
    return F32(SCALES / (LOG2 * params.n_octaves))


def scale_index(size, params):
    """The scale of every keypoint size; a size that is no positive number gives scale 0."""
    size = np.asarray(size, F32)
    cst = size_cst(params)
    if not params.scale_normalized:
        fixed = min(max(int(1.0986122886681 * float(cst) + 0.5), 0), SCALES - 1)
        return np.full(size.shape, fixed, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.log((size / F32(SMALLEST_KP_SIZE)).astype(F64)).astype(F32)
        v = (lg * cst).astype(F32).astype(F64) + 0.5
    v = np.where(v > 0.0, v, 0.0)                         # (int) of anything up to 0 is clamped to 0; NaN likewise
    return np.trunc(np.minimum(v, 63.0)).astype(np.int64)


def integral(image):
    h, w = image.shape
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(np.asarray(image).astype(np.int64), axis=0), axis=1)
    return S


def means(image, S, kx, ky, pts):
    """FREAK's meanIntensity for m keypoints (kx, ky float32 [m]) and their fields pts float32 [m, 43, 3]: int64 [m, 43]
    (values of a uint8) and the mask of the fields that took the interpolation branch."""
    img = np.asarray(image).astype(np.int64)
    h, w = img.shape
    xf = (pts[..., 0] + kx[:, None]).astype(F32)
    yf = (pts[..., 1] + ky[:, None]).astype(F32)
    sg = pts[..., 2].astype(F32)
    interp = sg < F32(0.5)
    out = np.zeros(xf.shape, np.int64)
    if interp.any():
        x, y = xf[interp], yf[interp]
        ix, iy = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
        rx = np.trunc((x - ix.astype(F32)).astype(F32) * F32(1024)).astype(np.int64)
        ry = np.trunc((y - iy.astype(F32)).astype(F32) * F32(1024)).astype(np.int64)
        assert ix.min() >= 0 and iy.min() >= 0 and ix.max() <= w - 2 and iy.max() <= h - 2
        v = ((1024 - rx) * (1024 - ry) * img[iy, ix] + rx * (1024 - ry) * img[iy, ix + 1] + rx * ry * img[iy + 1, ix + 1]
             + (1024 - rx) * ry * img[iy + 1, ix])
        assert v.max() < 2 ** 32 - 2 * 1024 * 1024                      # (upstream sums in an unsigned int)
        out[interp] = ((v + 2 * 1024 * 1024) // (4 * 1024 * 1024)) & 255
    box = ~interp
    if box.any():
        x, y, s = xf[box], yf[box], sg[box]
        xl = np.trunc((x - s).astype(F32).astype(F64) + 0.5).astype(np.int64)
        yt = np.trunc((y - s).astype(F32).astype(F64) + 0.5).astype(np.int64)
        xr = np.trunc((x + s).astype(F32).astype(F64) + 1.5).astype(np.int64)
        yb = np.trunc((y + s).astype(F32).astype(F64) + 1.5).astype(np.int64)
        assert xl.min() >= 0 and yt.min() >= 0 and xr.max() <= w and yb.max() <= h
        v = S[yb, xr] - S[yb, xl] + S[yt, xl] - S[yt, xr]
        area = (xr - xl) * (yb - yt)
        out[box] = ((v + area // 2) // area) & 255
    return out, interp


def _trunc_div(a, d):
    return np.sign(a) * (np.abs(a) // d)


def angles(vals, opairs):
    """The keypoint angle (float32 degrees) and the orientation index from the 43 means at orientation 0."""
    delta = vals[:, opairs[:, 0]] - vals[:, opairs[:, 1]]
    d0 = _trunc_div(delta * opairs[None, :, 2], 2048).sum(axis=1)
    d1 = _trunc_div(delta * opairs[None, :, 3], 2048).sum(axis=1)
    angle = (np.arctan2(d1.astype(F64), d0.astype(F64)) * (180.0 / np.pi)).astype(F32)
    s = (F32(ORIENTATIONS) * angle).astype(F32).astype(F64) * (1 / 360.0)
    t = np.where(angle < 0, np.trunc(s - 0.5), np.trunc(s + 0.5)).astype(np.int64)
    t = np.where(t < 0, t + ORIENTATIONS, t)
    return angle, np.where(t >= ORIENTATIONS, t - ORIENTATIONS, t)


def inside(kp, w, h, idx, sizes):
    """Upstream drops on x <= P, y <= P, x >= w - P, y >= h - P (float against int); a NaN position is dropped too."""
    P = np.asarray(sizes, np.int64)[idx]
    x, y = kp["x"].astype(F32), kp["y"].astype(F32)
    with np.errstate(invalid="ignore"):
        return (x > P.astype(F32)) & (y > P.astype(F32)) & (x < (w - P).astype(F32)) & (y < (h - P).astype(F32))


def describe(vals, pairs):
    """[m, 64] uint8 from the means [m, 43] and the 512 selected pair indices."""
    ij = all_pairs()[np.asarray(pairs, np.int64)]
    bits = vals[:, ij[:, 0]] >= vals[:, ij[:, 1]]
    desc = np.zeros((len(vals), BYTES), np.uint8)
    for c in range(PAIRS):
        byte, bit = bit_position(c)
        desc[:, byte] |= (bits[:, c].astype(np.uint8) << bit).astype(np.uint8)
    return desc


def compute(image, kp, params, pairs, table, sizes, trace=None):
    """FREAK::compute: (indices of the kept keypoints, their rows [m, 64], their keypoints with the angle overwritten)."""
    image = np.asarray(image)
    h, w = image.shape
    kp = np.array(kp, copy=True)
    scale = scale_index(kp["size"], params)
    idx = np.nonzero(inside(kp, w, h, scale, sizes))[0]
    out = kp[idx]
    if not len(idx):
        return idx, np.zeros((0, BYTES), np.uint8), out
    S = integral(image)
    kx, ky = out["x"].astype(F32), out["y"].astype(F32)
    table = np.asarray(table, F32)
    n_interp = 0
    if params.orientation_normalized:
        v0, m0 = means(image, S, kx, ky, table[scale[idx], 0])
        n_interp += int(m0.sum())
        angle, t = angles(v0, orientation_pairs(table))
    else:
        angle, t = np.zeros(len(idx), F32), np.zeros(len(idx), np.int64)
    out["angle"] = angle
    vals, m1 = means(image, S, kx, ky, table[scale[idx], t])
    n_interp += int(m1.sum())
    if trace is not None:
        trace.update(interpolated=n_interp, angles=angle.copy(), scales=scale[idx].copy(), orientations=t.copy())
    return idx, describe(vals, pairs), out


def extract_keyframe(image, kp, right_x, status, cam, params, pairs, table, sizes, trace=None):
    """What sf_extract_keyframe_device keeps with feature type 3 or 5: (descriptors [rows, 64], xyz [rows, 3], keypoints);
    the 3D point and the depth filter are the existing restatement's (orb_ref.points3d)."""
    idx, desc, kept = compute(image, kp, params, pairs, table, sizes, trace)
    p = orb_ref.points3d(np.asarray(kp), right_x, status, cam, idx)
    keep = np.ones(len(idx), bool)
    if cam.min_depth > 0 or cam.max_depth > 0:
        keep = np.isfinite(p).all(axis=1)
    return desc[keep], p[keep], kept[keep]
