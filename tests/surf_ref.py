"""NumPy restatement of SURF (Vis/FeatureType 0, csrc/k_surf.hip): cv::xfeatures2d::SURF of OpenCV 3.2 as rtabmap drives
it -- the fast-Hessian detector (detect) and orientation + descriptors on given keypoints (compute, extract_keyframe).
Written from the published algorithm; DESIGN.md section 3 item 17h lists what it decides where upstream leaves something
open and where it deviates.  The kernels are compared with it byte for byte, so this file is the specification.

Arithmetic: float32 in the order written wherever upstream computes in float; float64 where upstream's accumulators are
double (the Haar sums, the squared magnitude, the window's sampling positions); integers for the box sums and for the area
reduction of the window.  The two Gaussian tables are float64, every weight rounded to float32 once."""
import math

import numpy as np

from multi_robot_slam_separators_amd import _abi
from tests import orb2_ref, orb_ref

F32 = np.float32
F64 = np.float64
I64 = np.int64
ORI_RADIUS, ORI_WIN, ORI_SEARCH_INC, PATCH_SZ = 6, 60, 5, 20
ORI_SIGMA, DESC_SIGMA = 2.5, 3.3
HAAR_SIZE0, HAAR_SIZE_INC = 9, 6
ORI_SAMPLES = 109
MAX_CANDIDATES = 1 << 18          # the detector's candidate capacity per image: more maxima than this is an error
MAX_SIZE = 1.0e6                  # a keypoint size outside (0, MAX_SIZE) is dropped by compute

# the box filters in the 9 x 9 frame: {x1, y1, x2, y2, weight}
DX_BOXES = [(0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1)]
DY_BOXES = [(2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1)]
DXY_BOXES = [(1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1)]
# the gradient wavelets of orientation, in the 4 x 4 frame
GX_BOXES = [(0, 0, 2, 4, -1), (2, 0, 4, 4, 1)]
GY_BOXES = [(0, 0, 4, 2, 1), (0, 2, 4, 4, -1)]


class Params:
    def __init__(self, hessian_threshold=500.0, n_octaves=4, n_octave_layers=2, upright=0, extended=0):
        self.hessian_threshold = float(F32(hessian_threshold))
        self.n_octaves = int(n_octaves)
        self.n_octave_layers = int(n_octave_layers)
        self.upright = int(upright)
        self.extended = int(extended)

    @property
    def dims(self):
        return 128 if self.extended else 64


# ---- tables ------------------------------------------------------------------------------------------------------------
def gaussian(n, sigma):
    """cv::getGaussianKernel(n, sigma) kept in float64: exp(-x^2 / (2 sigma^2)) over the sum taken in index order."""
    t = [math.exp(-0.5 / (sigma * sigma) * (i - (n - 1) * 0.5) * (i - (n - 1) * 0.5)) for i in range(n)]
    s = 0.0
    for v in t:
        s += v
    return [v / s for v in t]


def orientation_table():
    """(offsets int8 [109, 2] = (x, y), weights float32 [109]) of the orientation samples: the lattice points with
    x^2 + y^2 < 36, x outer, y inner, weight = g[x + 6] g[y + 6] of the 13-tap Gaussian, sigma 2.5."""
    g = gaussian(2 * ORI_RADIUS + 1, ORI_SIGMA)
    pts, wts = [], []
    for i in range(-ORI_RADIUS, ORI_RADIUS + 1):
        for j in range(-ORI_RADIUS, ORI_RADIUS + 1):
            if i * i + j * j < ORI_RADIUS * ORI_RADIUS:
                pts.append((i, j))
                wts.append(g[i + ORI_RADIUS] * g[j + ORI_RADIUS])
    assert len(pts) == ORI_SAMPLES
    return np.array(pts, np.int8), np.array(wts, F64).astype(F32)


def descriptor_weights():
    """float32 [400]: g[i] g[j] of the 20-tap Gaussian, sigma 3.3, at index 20 i + j."""
    g = gaussian(PATCH_SZ, DESC_SIGMA)
    return np.array([g[i] * g[j] for i in range(PATCH_SZ) for j in range(PATCH_SZ)], F64).astype(F32)


# ---- shared arithmetic -------------------------------------------------------------------------------------------------
def integral(image):
    h, w = image.shape
    S = np.zeros((h + 1, w + 1), I64)
    S[1:, 1:] = np.cumsum(np.cumsum(np.asarray(image).astype(I64), axis=0), axis=1)
    return S


def cv_round(v):
    """cvRound: to the nearest integer, halves to even."""
    return np.rint(v).astype(I64)


def resize_boxes(boxes, old, new):
    """resizeHaarPattern: the corners scaled by the float32 ratio and rounded; weight = w / ((float)(x2 - x1) * (y2 - y1))."""
    ratio = F32(F32(new) / F32(old))
    out = []
    for x1, y1, x2, y2, wt in boxes:
        a, b, c, d = (int(cv_round(F32(ratio * F32(v)))) for v in (x1, y1, x2, y2))
        out.append((a, b, c, d, F32(F32(wt) / F32(F32(c - a) * F32(d - b)))))
    return out


def haar(S, boxes, y, x):
    """calcHaarPattern at the integral-image origins (y, x): the terms (float)box * weight are float32 products, summed
    in float64 in the boxes' order, the sum rounded to float32."""
    d = np.zeros(np.broadcast(y, x).shape, F64)
    for x1, y1, x2, y2, wt in boxes:
        box = S[y + y1, x + x1] + S[y + y2, x + x2] - S[y + y2, x + x1] - S[y + y1, x + x2]
        d = d + (box.astype(F32) * wt).astype(F32).astype(F64)
    return d.astype(F32)


# ---- the fast-Hessian detector -----------------------------------------------------------------------------------------
def layers(params):
    """[(octave, layer, size, step)] of all n_octaves (n_octave_layers + 2) layers, in index order."""
    return [(o, l, (HAAR_SIZE0 + HAAR_SIZE_INC * l) << o, 1 << o) for o in range(params.n_octaves)
            for l in range(params.n_octave_layers + 2)]


def layer_planes(S, size, step):
    """calcLayerDetAndTrace: (det, trace) float32 [h // step, w // step]; samples whose filter leaves the image -- or all
    of them, when the filter is larger than the image -- are zero."""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    det = np.zeros((h // step, w // step), F32)
    trace = np.zeros_like(det)
    if size > h or size > w:
        return det, trace
    ni, nj = 1 + (h - size) // step, 1 + (w - size) // step
    margin = (size // 2) // step
    y = (np.arange(ni, dtype=I64) * step)[:, None]
    x = (np.arange(nj, dtype=I64) * step)[None, :]
    dx = haar(S, resize_boxes(DX_BOXES, 9, size), y, x)
    dy = haar(S, resize_boxes(DY_BOXES, 9, size), y, x)
    dxy = haar(S, resize_boxes(DXY_BOXES, 9, size), y, x)
    det[margin:margin + ni, margin:margin + nj] = (dx * dy).astype(F32) - ((F32(0.81) * dxy).astype(F32) * dxy).astype(F32)
    trace[margin:margin + ni, margin:margin + nj] = dx + dy
    return det, trace


def solve3(A, b):
    """x of A x = b for [m, 3, 3] / [m, 3] float32 by Cramer's rule in the order written (no pivoting); ok is False where
    the determinant is zero or not finite."""
    a = lambda r, c: A[:, r, c]
    m0 = a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)
    m1 = a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0)
    m2 = a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)
    det = (a(0, 0) * m0 - a(0, 1) * m1) + a(0, 2) * m2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = F32(1.0) / det
        p = b[:, 1] * a(2, 2) - a(1, 2) * b[:, 2]
        q = b[:, 1] * a(2, 1) - a(1, 1) * b[:, 2]
        r = a(1, 0) * b[:, 2] - b[:, 1] * a(2, 0)
        x0 = d * ((b[:, 0] * m0 - a(0, 1) * p) + a(0, 2) * q)
        x1 = d * ((a(0, 0) * p - b[:, 0] * m1) + a(0, 2) * r)
        x2 = d * ((b[:, 0] * m2 - a(0, 1) * r) - a(0, 0) * q)
    x = np.stack([x0, x1, x2], axis=1).astype(F32)
    return x, (det != 0) & np.isfinite(x).all(axis=1)


def interpolate(N, step, ds):
    """interpolateKeypoint on the 3 x 3 x 3 neighbourhoods N float32 [m, 3 (layer), 3 (row), 3 (column)]: the offsets
    x [m, 3] = (column, row, layer) and whether the keypoint stays."""
    h = F32(0.5)
    q = F32(0.25)
    b = np.stack([-((N[:, 1, 1, 2] - N[:, 1, 1, 0]) * h), -((N[:, 1, 2, 1] - N[:, 1, 0, 1]) * h),
                  -((N[:, 2, 1, 1] - N[:, 0, 1, 1]) * h)], axis=1).astype(F32)
    c2 = F32(2.0) * N[:, 1, 1, 1]
    dxx = (N[:, 1, 1, 0] - c2) + N[:, 1, 1, 2]
    dyy = (N[:, 1, 0, 1] - c2) + N[:, 1, 2, 1]
    dss = (N[:, 0, 1, 1] - c2) + N[:, 2, 1, 1]
    dxy = (((N[:, 1, 2, 2] - N[:, 1, 2, 0]) - N[:, 1, 0, 2]) + N[:, 1, 0, 0]) * q
    dxs = (((N[:, 2, 1, 2] - N[:, 2, 1, 0]) - N[:, 0, 1, 2]) + N[:, 0, 1, 0]) * q
    dys = (((N[:, 2, 2, 1] - N[:, 2, 0, 1]) - N[:, 0, 2, 1]) + N[:, 0, 0, 1]) * q
    A = np.stack([np.stack([dxx, dxy, dxs], axis=1), np.stack([dxy, dyy, dys], axis=1),
                  np.stack([dxs, dys, dss], axis=1)], axis=1).astype(F32)
    x, ok = solve3(A, b)
    with np.errstate(invalid="ignore"):
        ok &= (x != 0).any(axis=1) & (np.abs(x) <= 1).all(axis=1)
    return x, ok


def find_maxima(S, params, trace=None):
    """Every keypoint of the detector, unsorted: (keypoints, middle-layer position) -- position = the offset of the sample
    in the enumeration of all middle layers' planes, the tie-break of the sort."""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    L = layers(params)
    planes = [layer_planes(S, size, step) for _, _, size, step in L]
    thr = F32(params.hessian_threshold)
    out, positions, base = [], [], 0
    for index, (o, l, size, step) in enumerate(L):
        if l == 0 or l > params.n_octave_layers:
            continue
        rows, cols = h // step, w // step
        plane_base, base = base, base + rows * cols
        margin = (L[index + 1][2] // 2) // step + 1
        if rows - margin <= margin or cols - margin <= margin:
            continue
        det3 = [planes[index - 1][0], planes[index][0], planes[index + 1][0]]
        c = det3[1][margin:rows - margin, margin:cols - margin]
        is_max = c > thr
        for k in range(3):
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if k == 1 and di == 0 and dj == 0:
                        continue
                    is_max &= c > det3[k][margin + di:rows - margin + di, margin + dj:cols - margin + dj]
        ii, jj = np.nonzero(is_max)
        if not len(ii):
            continue
        ii, jj = ii + margin, jj + margin
        N = np.stack([np.stack([np.stack([det3[k][ii + di, jj + dj] for dj in (-1, 0, 1)], axis=1) for di in (-1, 0, 1)],
                               axis=1) for k in range(3)], axis=1)
        x, ok = interpolate(N, step, size - L[index - 1][2])
        half = (size // 2) // step
        sum_i, sum_j = step * (ii - half), step * (jj - half)
        centre = F32(size - 1) * F32(0.5)
        kp = np.zeros(len(ii), _abi.KEYPOINT_DTYPE)
        with np.errstate(invalid="ignore", over="ignore"):
            kp["x"] = (sum_j.astype(F32) + centre) + x[:, 0] * F32(step)
            kp["y"] = (sum_i.astype(F32) + centre) + x[:, 1] * F32(step)
            kp["size"] = np.rint(F32(size) + x[:, 2] * F32(size - L[index - 1][2]))
        kp["angle"] = -1.0
        kp["response"] = N[:, 1, 1, 1]
        kp["octave"] = o
        t = planes[index][1][ii, jj]
        kp["class_id"] = (t > 0).astype(np.int32) - (t < 0).astype(np.int32)
        out.append(kp[ok])
        positions.append((plane_base + ii * cols + jj)[ok])
        if trace is not None:
            trace.setdefault("maxima", []).append((index, int(len(ii)), int(ok.sum())))
    if not out:
        return np.zeros(0, _abi.KEYPOINT_DTYPE), np.zeros(0, I64)
    return np.concatenate(out), np.concatenate(positions)


def detect(image, params, max_features=0, trace=None):
    """sf_detect_surf_device: the maxima in descending response -- equal responses by ascending layer, then ascending sample
    (upstream's order of those depends on its threads) -- then rtabmap's limitKeypoints."""
    kp, pos = find_maxima(integral(np.asarray(image)), params, trace)
    if len(kp) > MAX_CANDIDATES:
        raise OverflowError("%d maxima exceed the candidate capacity %d" % (len(kp), MAX_CANDIDATES))
    order = np.lexsort((pos, -kp["response"].astype(F64)))
    return orb2_ref.limit_keypoints(kp[order], max_features)


# ---- orientation and descriptors (SURF::compute) ---------------------------------------------------------------------
def scale_of(size):
    """s = size * 1.2f / 9.0f and the gradient wavelet's side 2 cvRound(2 s)."""
    s = F32(F32(F32(size) * F32(1.2)) / F32(9.0))
    return s, 2 * int(cv_round(F32(F32(2.0) * s)))


def orientation(S, cx, cy, s, grad, tables, trace=None):
    """The dominant direction in degrees (float32), or None when no sample lies inside the image."""
    pts, wts = tables
    h1, w1 = S.shape
    half = F32(F32(grad - 1) / F32(2.0))
    x = cv_round(((cx + pts[:, 0].astype(F32) * s).astype(F32) - half).astype(F32))
    y = cv_round(((cy + pts[:, 1].astype(F32) * s).astype(F32) - half).astype(F32))
    ok = (y >= 0) & (y < h1 - grad) & (x >= 0) & (x < w1 - grad)
    if not ok.any():
        return None
    x, y, wt = x[ok], y[ok], wts[ok]
    X = haar(S, resize_boxes(GX_BOXES, 4, grad), y, x) * wt
    Y = haar(S, resize_boxes(GY_BOXES, 4, grad), y, x) * wt
    ang = cv_round(orb_ref.fast_atan2(Y, X))
    d = np.abs(ang[None, :] - np.arange(0, 360, ORI_SEARCH_INC, dtype=I64)[:, None])
    inwin = (d < ORI_WIN // 2) | (d > 360 - ORI_WIN // 2)
    # (float32 sums in sample order; a sample outside the window adds +0, which changes no float32 sum that started at +0)
    sumx = np.cumsum(np.where(inwin, X[None, :], F32(0)), axis=1, dtype=F32)[:, -1]
    sumy = np.cumsum(np.where(inwin, Y[None, :], F32(0)), axis=1, dtype=F32)[:, -1]
    mod = (sumx * sumx).astype(F32) + (sumy * sumy).astype(F32)
    best = int(np.argmax(mod))                       # the first of equal maxima, as upstream's strict >
    bx, by = (sumx[best], sumy[best]) if mod[best] > 0 else (F32(0), F32(0))
    if trace is not None:
        trace["ori_samples"] = trace.get("ori_samples", []) + [int(ok.sum())]
    return F32(orb_ref.fast_atan2(-by, bx))


def area_weights(win):
    """int64 [21, win]: the overlap of patch cell r with window pixel i, in units of 1 / 21 pixel (rows sum to win)."""
    r = np.arange(PATCH_SZ + 1, dtype=I64)[:, None]
    i = np.arange(win, dtype=I64)[None, :]
    return np.maximum(np.minimum((r + 1) * win, 21 * i + 21) - np.maximum(r * win, 21 * i), 0)


def window(image, cx, cy, win, direction, upright):
    """The win x win window around the keypoint, uint8 values as int64: rotated and sampled bilinearly (positions in float64
    from the float32 start and steps, values in float32), or upright and nearest; positions outside are clamped."""
    img = np.asarray(image).astype(I64)
    h, w = img.shape
    i = np.arange(win, dtype=I64)[:, None]
    j = np.arange(win, dtype=I64)[None, :]
    off = F32(-(F32(win - 1) / F32(2.0)))
    if upright:
        sx, sy = int(cv_round(F32(cx + off))), int(cv_round(F32(cy - off)))
        return img[np.clip(sy - j, 0, h - 1), np.clip(sx + i, 0, w - 1)]
    rad = F32(direction * F32(np.pi / 180.0))
    sin_dir, cos_dir = F32(-F32(math.sin(float(rad)))), F32(math.cos(float(rad)))
    start_x = F32(F32(cx + F32(off * cos_dir)) + F32(off * sin_dir))
    start_y = F32(F32(cy - F32(off * sin_dir)) + F32(off * cos_dir))
    px = (F64(start_x) + i.astype(F64) * F64(sin_dir)) + j.astype(F64) * F64(cos_dir)
    py = (F64(start_y) + i.astype(F64) * F64(cos_dir)) - j.astype(F64) * F64(sin_dir)
    fx, fy = np.floor(px), np.floor(py)
    inside = (fx >= 0) & (fx < w - 1) & (fy >= 0) & (fy < h - 1)
    ix = np.clip(fx, 0, max(w - 2, 0)).astype(I64)
    iy = np.clip(fy, 0, max(h - 2, 0)).astype(I64)
    a, b = (px - fx).astype(F32), (py - fy).astype(F32)
    one = F32(1.0)
    x1, y1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    v = ((img[iy, ix].astype(F32) * (one - a)) * (one - b) + (img[iy, x1].astype(F32) * a) * (one - b)) \
        + (img[y1, ix].astype(F32) * (one - a)) * b
    v = v + (img[y1, x1].astype(F32) * a) * b
    near = img[np.clip(cv_round(py), 0, h - 1), np.clip(cv_round(px), 0, w - 1)]
    return np.where(inside, cv_round(v), near)


def patch_of(win_pixels):
    """The 21 x 21 patch: the exact area average of every cell, rounded half up -- integer arithmetic throughout."""
    win = win_pixels.shape[0]
    W = area_weights(win)
    num = W @ win_pixels @ W.T
    den = win * win                                    # (the weights of a cell sum to win along each axis)
    return (2 * num + den) // (2 * den)


def descriptor(P, params, dw):
    """float32 [64 | 128] from the patch P int64 [21, 21]."""
    dw = dw.reshape(PATCH_SZ, PATCH_SZ)
    vx = ((P[:-1, 1:] - P[:-1, :-1] + P[1:, 1:] - P[1:, :-1]).astype(F32) * dw).astype(F32)
    vy = ((P[1:, :-1] - P[:-1, :-1] + P[1:, 1:] - P[:-1, 1:]).astype(F32) * dw).astype(F32)
    zero = F32(0)
    vec = []
    for i in range(4):
        for j in range(4):
            tx = vx[5 * i:5 * i + 5, 5 * j:5 * j + 5].reshape(-1)
            ty = vy[5 * i:5 * i + 5, 5 * j:5 * j + 5].reshape(-1)
            if params.extended:
                up, right = ty >= 0, tx >= 0
                parts = [np.where(up, tx, zero), np.where(up, np.abs(tx), zero), np.where(~up, tx, zero),
                         np.where(~up, np.abs(tx), zero), np.where(right, ty, zero), np.where(right, np.abs(ty), zero),
                         np.where(~right, ty, zero), np.where(~right, np.abs(ty), zero)]
            else:
                parts = [tx, ty, np.abs(tx), np.abs(ty)]
            vec += [np.cumsum(p, dtype=F32)[-1] for p in parts]      # 25 float32 additions in raster order, from +0
    vec = np.array(vec, F32)
    mag = np.cumsum((vec * vec).astype(F32).astype(F64))[-1]        # float32 squares, summed in float64 in row order
    scale = F32(1.0 / (math.sqrt(float(mag)) + float(np.finfo(F32).eps)))
    return (vec * scale).astype(F32)


def compute(image, kp, params, trace=None):
    """SURF::compute: (indices of the kept keypoints, rows float32 [m, dims], the kept keypoints with their angle)."""
    image = np.asarray(image)
    h, w = image.shape
    kp = np.array(kp, copy=True)
    S = integral(image)
    tables, dw = orientation_table(), descriptor_weights()
    idx, rows = [], []
    for n in range(len(kp)):
        size = F32(kp["size"][n])
        if not (size > 0 and size < F32(MAX_SIZE)):
            continue
        s, grad = scale_of(size)
        if grad < 2 or h + 1 < grad or w + 1 < grad:
            continue
        cx, cy = F32(kp["x"][n]), F32(kp["y"][n])
        if not (np.isfinite(cx) and np.isfinite(cy) and abs(cx) < F32(MAX_SIZE) and abs(cy) < F32(MAX_SIZE)):
            continue
        direction = F32(270.0)
        if not params.upright:
            direction = orientation(S, cx, cy, s, grad, tables, trace)
            if direction is None:
                continue
        kp["angle"][n] = direction
        win = int(F32(F32(PATCH_SZ + 1) * s))
        P = patch_of(window(image, cx, cy, win, direction, params.upright))
        idx.append(n)
        rows.append(descriptor(P, params, dw))
        if trace is not None:
            trace["win"] = trace.get("win", []) + [win]
    idx = np.array(idx, I64)
    desc = np.array(rows, F32).reshape(len(idx), params.dims)
    return idx, desc, kp[idx]


def extract_keyframe(image, kp, right_x, status, cam, params, trace=None):
    """What sf_extract_keyframe_device keeps with feature type 0: (rows float32 [rows, dims], xyz [rows, 3], keypoints);
    the 3D point and the depth filter are the existing restatement's (orb_ref.points3d)."""
    idx, desc, kept = compute(image, kp, params, trace)
    p = orb_ref.points3d(np.asarray(kp), right_x, status, cam, idx)
    keep = np.ones(len(idx), bool)
    if cam.min_depth > 0 or cam.max_depth > 0:
        keep = np.isfinite(p).all(axis=1)
    return desc[keep], p[keep], kept[keep]
