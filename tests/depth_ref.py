"""NumPy restatement of the depth keyframe path (csrc/k_depth.hip, the masked forms of csrc/k_gftt.hip and csrc/k_fast.hip):
what rtabmap does with a registered depth image -- the detector mask of Feature2D::generateKeypoints (Vis/DepthAsMask) and
util3d::generateKeypoints3DDepth -> projectDepthTo3D(smoothing = true) -> util2d::getDepth(depthErrorRatio 0.02,
estWithNeighborsIfNull false) -- and cv::goodFeaturesToTrack / FastFeatureDetector::detect with a mask.  Written down from
memory of the upstream sources, which are not part of the reference tree; the GPU is compared with
this byte for byte (tests/test_gpu_depth.py).  All arithmetic is float32 in the order written.

  value     uint16 millimetres: float32(v) * float32(0.001) for 0 < v < 65535, else 0; float32 metres: the float itself
  mask      255 iff value > min_depth and (max_depth == 0 or value <= max_depth), else 0; NaN compares false
  pixel     u = (int)(x + 0.5f), C's truncation toward zero (x = -0.7 gives 0); u == width and x < width: u = width - 1;
            outside 0 .. width - 1: no depth.  A coordinate that is not finite, or whose x + 0.5f is not inside
            (-1, width + 1), is outside (where C leaves the cast undefined); the same for v
  depth     d = value at (u, v); 0 or not finite: no point.  Neighbours uu = max(u-1, 0) .. min(u+1, w-1) (outer loop), vv
            likewise (inner loop), centre skipped: dn counts iff dn != 0, finite and |dn - d| < 0.02f * d -- with weight 2 and
            value dn * 2 when uu == u or vv == v, else weight 1 and value dn; sums start at 0 and add in loop order;
            depth = (d * 4 + sum_values) / (sum_weights + 4)
  point     cx_ = cx > 0 ? cx : float32(width // 2) - 0.5 (cy_ likewise); X = (x - cx_) * depth / fx, Y = (y - cy_) * depth /
            fy, Z = depth; kept iff Z finite, (min_depth < 0 or Z > min_depth), (max_depth <= 0 or Z <= max_depth); then
            local_transform as the stereo points (the identity is skipped, not multiplied through); else three quiet NaNs
  GFTT      the maximum that scales quality_level over mask != 0 only (max(0, ..)); a candidate lies on mask != 0; the
            thresholded 3 x 3 maximum sees every pixel; the rest is gftt_ref.select
  FAST      fast_ref.detect with the corners on mask == 0 dropped before the limit"""
import numpy as np

from multi_robot_slam_separators_amd import _abi
from tests import fast_ref, gftt_ref

F32 = np.float32
QNAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]


def values(depth):
    """The depth image in metres, float32 [h, w]."""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return np.where((depth > 0) & (depth < 65535), depth.astype(F32) * F32(0.001), F32(0)).astype(F32)
    assert depth.dtype == np.float32, depth.dtype
    return depth


def depth_mask(depth, min_depth=0.0, max_depth=0.0):
    """uint8 [h, w]: what k_depth_mask writes."""
    v = values(depth)
    with np.errstate(invalid="ignore"):
        ok = (v > F32(min_depth)) & ((F32(max_depth) == F32(0)) | (v <= F32(max_depth)))
    return np.where(ok, 255, 0).astype(np.uint8)


def depth_pixel(x, n):
    """The pixel of coordinate x on a side of n pixels; -1: outside."""
    x = F32(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r = x + F32(0.5)
        if not (r > F32(-1) and r < F32(n + 1)):
            return -1
    u = int(r)                                             # toward zero
    if u == n and x < F32(n):
        u = n - 1
    return u if u < n else -1


def get_depth(depth, x, y):
    """util2d::getDepth(smoothing = true): the smoothed depth at (x, y) in metres, float32; 0: none."""
    v = values(depth)
    h, w = v.shape
    u, vv0 = depth_pixel(x, w), depth_pixel(y, h)
    if u < 0 or vv0 < 0:
        return F32(0)
    d = v[vv0, u]
    if d == 0 or not np.isfinite(d):
        return F32(0)
    sum_w, sum_d = F32(0), F32(0)
    err = F32(0.02) * d
    for uu in range(max(u - 1, 0), min(u + 1, w - 1) + 1):
        for vv in range(max(vv0 - 1, 0), min(vv0 + 1, h - 1) + 1):
            if uu == u and vv == vv0:
                continue
            dn = v[vv, uu]
            if dn != 0 and np.isfinite(dn) and np.abs(dn - d) < err:
                if uu == u or vv == vv0:
                    sum_w = sum_w + F32(2)
                    dn = dn * F32(2)
                else:
                    sum_w = sum_w + F32(1)
                sum_d = sum_d + dn
    with np.errstate(over="ignore"):
        return F32((d * F32(4) + sum_d) / (sum_w + F32(4)))


def keypoints3d_depth(xy, depth, cam):
    """xyz float32 [n, 3] of the coordinates xy [n, 2] (or KEYPOINT_DTYPE records): what k_depth_points writes for an
    _abi.StereoCamera (fx, fy, cx, cy, local_transform, min_depth, max_depth)."""
    if getattr(xy, "dtype", None) == _abi.KEYPOINT_DTYPE:
        xy = np.stack([xy["x"], xy["y"]], axis=1)
    xy = np.asarray(xy, F32).reshape(-1, 2)
    h, w = np.asarray(depth).shape
    L = np.array(list(cam.local_transform), F32)
    identity = bool((L == np.eye(4, dtype=F32)[:3].ravel()).all())
    fx, fy, mn, mx = F32(cam.fx), F32(cam.fy), F32(cam.min_depth), F32(cam.max_depth)
    cx = F32(cam.cx) if cam.cx > 0 else F32(w // 2) - F32(0.5)
    cy = F32(cam.cy) if cam.cy > 0 else F32(h // 2) - F32(0.5)
    out = np.full((len(xy), 3), QNAN, F32)
    with np.errstate(all="ignore"):
        for i, (x, y) in enumerate(xy):
            z = get_depth(depth, x, y)
            if z == 0:
                continue
            px, py = (x - cx) * z / fx, (y - cy) * z / fy
            if np.isfinite(z) and (mn < 0 or z > mn) and (mx <= 0 or z <= mx):
                if identity:
                    out[i] = px, py, z
                else:
                    for r in range(3):
                        out[i, r] = ((L[4 * r] * px + L[4 * r + 1] * py) + L[4 * r + 2] * z) + L[4 * r + 3]
    assert out.dtype == F32
    return out


def points_valid(xyz):
    return np.isfinite(xyz).all(axis=1).astype(np.uint8)


# ---- the two corner detectors under a mask -----------------------------------------------------------------------------
def gftt_threshold(R, mask, quality_level):
    sel = R[np.asarray(mask) != 0]
    vmax = max(F32(0), sel.max()) if sel.size else F32(0)
    return F32(np.float64(vmax) * quality_level)


def gftt_candidates(R, mask, quality_level):
    """(ys, xs, thr, M): the candidates of the masked detector, the threshold and the thresholded 3 x 3 maximum plane
    [h - 2, w - 2] of the interior."""
    h, w = R.shape
    thr = gftt_threshold(R, mask, quality_level)
    T = np.where(R > thr, R, F32(0))
    M = np.zeros((h - 2, w - 2), F32)
    for dy in range(3):
        for dx in range(3):
            M = np.maximum(M, T[dy:dy + h - 2, dx:dx + w - 2])
    inner = R[1:h - 1, 1:w - 1]
    ys, xs = np.nonzero((inner > thr) & (inner == M) & (np.asarray(mask)[1:h - 1, 1:w - 1] != 0))
    return ys + 1, xs + 1, thr, M


def detect_corners_masked(image, mask, max_corners=1000, quality_level=0.001, min_distance=3.0, block=3, harris=0, k=0.04):
    """sf_detect_corners_masked_device: gftt_ref's response, the masked candidates, gftt_ref.select's order and minDistance
    rule (the same cells of cvRound(minDistance))."""
    R = gftt_ref.response(image, block, harris, k)
    h, w = R.shape
    ys, xs, _, _ = gftt_candidates(R, mask, quality_level)
    v, idx = R[ys, xs], ys * w + xs
    order = np.lexsort((-idx, -v.astype(np.float64)))
    taken = []
    if min_distance >= 1.0:
        cell = int(np.rint(min_distance))
        md2 = F32(min_distance * min_distance)
        grid = {}
        for i in order:
            if max_corners > 0 and len(taken) >= max_corners:
                break
            x, y = int(xs[i]), int(ys[i])
            cx, cy = x // cell, y // cell
            good = True
            for gy in range(cy - 1, cy + 2):
                for gx in range(cx - 1, cx + 2):
                    for qx, qy in grid.get((gx, gy), ()):
                        ddx, ddy = F32(x - qx), F32(y - qy)
                        if ddx * ddx + ddy * ddy < md2:
                            good = False
            if good:
                grid.setdefault((cx, cy), []).append((x, y))
                taken.append((x, y))
    else:
        for i in order:
            if max_corners > 0 and len(taken) >= max_corners:
                break
            taken.append((int(xs[i]), int(ys[i])))
    kp = np.zeros(len(taken), _abi.KEYPOINT_DTYPE)
    if taken:
        kp["x"], kp["y"] = np.array(taken, F32).T
    kp["size"], kp["angle"], kp["response"], kp["octave"], kp["class_id"] = float(block), -1.0, 0.0, 0, -1
    return kp


def detect_fast_masked(image, mask, threshold=20, nonmax_suppression=1, max_features=0):
    """sf_detect_fast_masked_device: every corner of fast_ref.detect (no limit: raster order), those on mask == 0 dropped,
    then fast_ref's limitKeypoints order."""
    img = np.asarray(image)
    w = img.shape[1]
    kp = fast_ref.detect(img, threshold, nonmax_suppression, 0)
    kp = kp[np.asarray(mask)[kp["y"].astype(int), kp["x"].astype(int)] != 0]
    if max_features > 0 and len(kp) > max_features:
        idx = kp["y"].astype(np.int64) * w + kp["x"].astype(np.int64)
        order = np.lexsort((-idx, -kp["response"].astype(np.float64)))
        kp = kp[order][:max_features]
    return kp


# ---- seeded inputs -------------------------------------------------------------------------------------------------------
SIZES = ((64, 48), (97, 131))                    # (width, height) of every GPU test image


def image(width, height, seed):
    """A textured uint8 image: blocky noise at 4 px and at 2 px plus fine noise -- corners for both detectors all over it."""
    rng = np.random.default_rng(seed)
    coarse = np.kron(rng.integers(30, 226, ((height + 3) // 4, (width + 3) // 4)), np.ones((4, 4), np.int64))[:height, :width]
    mid = np.kron(rng.integers(-40, 41, ((height + 1) // 2, (width + 1) // 2)), np.ones((2, 2), np.int64))[:height, :width]
    return np.clip(coarse + mid + rng.integers(-8, 9, (height, width)), 0, 255).astype(np.uint8)


def scene(width, height, seed, fmt=_abi.SF_DEPTH_U16_MM, holes=(), dead=False):
    """A piecewise-planar depth scene: blocks of tilted planes between 0.4 m and 6 m with steps between them, rectangular and
    single-pixel holes (uint16: 0 and 65535; float32: 0, NaN, +inf, -inf), extra holes at the pixels `holes` = ((x, y), ..).
    dead: an image with no valid depth at all.  Returns the image in `fmt`."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    bw, bh = max(width // 4, 8), max(height // 3, 8)
    block = (y // bh).astype(int) * 8 + (x // bw).astype(int)
    z = np.zeros((height, width))
    for b in np.unique(block):
        base, gx, gy = rng.uniform(0.4, 6.0), rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004)
        sel = block == b
        z[sel] = base + gx * x[sel] + gy * y[sel]
    z = np.clip(z + rng.normal(0.0, 0.002, z.shape), 0.05, 60.0)
    kind = np.zeros((height, width), np.int8)            # 0 = depth, 1 .. 4 = the kinds of hole
    for _ in range(4):
        x0, y0 = int(rng.integers(0, width - 6)), int(rng.integers(0, height - 6))
        kind[y0:y0 + int(rng.integers(3, 12)), x0:x0 + int(rng.integers(3, 12))] = int(rng.integers(1, 5))
    speck = rng.random((height, width)) < 0.06
    kind[speck] = rng.integers(1, 5, size=int(speck.sum()))
    for hx, hy in holes:
        kind[hy, hx] = 1
    if dead:
        kind[:] = rng.integers(1, 5, size=kind.shape)
    if fmt == _abi.SF_DEPTH_U16_MM:
        d = np.clip(np.rint(z * 1000.0), 1, 65534).astype(np.uint16)
        d[(kind == 1) | (kind == 3)] = 0
        d[(kind == 2) | (kind == 4)] = 65535
        return d
    d = z.astype(np.float32)
    d[kind == 1] = 0.0
    d[kind == 2] = np.nan
    d[kind == 3] = np.inf
    d[kind == 4] = -np.inf
    return d


def pitched(array, extra_elems=5, fill=0xA5):
    """The 2-D array as a view of a buffer whose rows are extra_elems elements longer, the padding filled with bytes `fill`."""
    h, w = array.shape
    buf = np.empty((h, w + extra_elems), array.dtype)
    buf.view(np.uint8)[:] = fill
    buf[:, :w] = array
    return buf[:, :w]


def camera(width, height, local=False, min_depth=0.0, max_depth=0.0, cx=None, cy=None):
    """A pinhole model for a width x height image; local: a non-identity local_transform (optical frame to base)."""
    lt = None
    if local:
        lt = np.array([[0.0, -0.1736482, 0.9848078, 0.12], [-1.0, 0.0, 0.0, -0.03], [0.0, -0.9848078, -0.1736482, 0.45]], np.float32)
    return _abi.stereo_camera(0.9 * width, 0.92 * width, width / 2.0 - 0.25 if cx is None else cx,
                              height / 2.0 + 0.5 if cy is None else cy, 0.0, local_transform=lt, min_depth=min_depth,
                              max_depth=max_depth)
