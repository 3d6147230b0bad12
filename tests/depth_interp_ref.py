"""NumPy restatement of the decimated depth path (k_depth_interp and the scaled form of k_depth_points in csrc/k_depth.hip):
what rtabmap does with a depth image whose size divides the image's -- util2d::interpolate(depth, factor, 0.1f) for the
detector mask (myRegistrationVis.cpp:271-284) and generateKeypoints3D on the small image with scaled intrinsics.  The rule is
as remembered from upstream rtabmap, not from the reference tree (include/sepfinder.h); the GPU is
compared with this byte for byte (tests/test_gpu_depth_decimated.py).  All arithmetic is float32 in the order written.

  present   uint16: 0 < v < 65535, value float32(v) (raw millimetres); float32: finite and > 0
  cell      (a, b), 1 <= a < dw, 1 <= b < dh: TL = D[b-1][a-1], TR = D[b-1][a], BL = D[b][a-1], BR = D[b][a]; valid iff all
            four are present and every pairwise |difference| <= e = 0.1f * (((TL + TR) + BL) + BR) / 4.0f
  value     at x = (a-1) f + p, y = (b-1) f + q, p and q in 0 .. f: st = (TR - TL) / f, sb = (BR - BL) / f, top = TL + st * p,
            bot = BL + sb * p, value = top + ((bot - top) / f) * q; uint16 output: (uint16_t)(int)value
  order     b outer, a inner, a later cell overwrites an earlier one (interpolate); per pixel the last valid cell among the
            at most four that cover it (interpolate_per_pixel)
  points    rx = 1 / (width / dw), the keypoint at (x * rx, y * ry) on the small image, cx * rx (not > 0: dw // 2 - 0.5),
            fx * rx; the rest is depth_ref.keypoints3d_depth"""
import numpy as np

from tests import depth_ref

F32 = np.float32


def samples(depth):
    """float32 [h, w]: the value the cell test reads of every sample, 0 = absent."""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return np.where((depth > 0) & (depth < 65535), depth.astype(F32), F32(0)).astype(F32)
    assert depth.dtype == np.float32, depth.dtype
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(depth) & (depth > 0), depth, F32(0)).astype(F32)


def cell_valid(tl, tr, bl, br):
    if not (tl > 0 and tr > 0 and bl > 0 and br > 0):
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        e = F32(0.1) * (((tl + tr) + bl) + br) / F32(4.0)
        return bool(abs(tl - tr) <= e and abs(tl - bl) <= e and abs(tl - br) <= e and abs(tr - bl) <= e and abs(tr - br) <= e
                    and abs(bl - br) <= e)


def cell_value(tl, tr, bl, br, f, p, q):
    """float32; p and q may be arrays."""
    ff = F32(f)
    with np.errstate(over="ignore", invalid="ignore"):
        st, sb = (tr - tl) / ff, (br - bl) / ff
        top, bot = tl + st * F32(p), bl + sb * F32(p)
        return F32(top + ((bot - top) / ff) * F32(q))


def stored(value, dtype):
    """What the enlarged image holds of a float32 value (array or scalar)."""
    if dtype == np.uint16:
        return np.asarray(value).astype(np.int32).astype(np.uint16)     # (uint16_t)(int)value, by truncation
    return np.asarray(value, F32)


def interpolate(depth, f):
    """util2d::interpolate(depth, f, 0.1f), the literal sequential loops: [dh f, dw f] in the input's dtype."""
    depth = np.asarray(depth)
    if f == 1:
        return depth.copy()
    assert f >= 2
    D = samples(depth)
    dh, dw = D.shape
    out = np.zeros((dh * f, dw * f), depth.dtype)
    for b in range(1, dh):
        for a in range(1, dw):
            tl, tr, bl, br = D[b - 1, a - 1], D[b - 1, a], D[b, a - 1], D[b, a]
            if not cell_valid(tl, tr, bl, br):
                continue
            for q in range(f + 1):
                for p in range(f + 1):
                    out[(b - 1) * f + q, (a - 1) * f + p] = stored(cell_value(tl, tr, bl, br, f, p, q), depth.dtype)
    return out


def interpolate_per_pixel(depth, f):
    """The same image pixel by pixel, as the kernel makes it: of the cells that cover (x, y) -- columns a = x // f + 1 at p =
    x % f and, when x % f == 0 and x > 0, a = x // f at p = f; rows alike -- the last valid one in the loops' order."""
    depth = np.asarray(depth)
    if f == 1:
        return depth.copy()
    D = samples(depth)
    dh, dw = D.shape
    valid = np.zeros((dh, dw), bool)
    for b in range(1, dh):
        for a in range(1, dw):
            valid[b, a] = cell_valid(D[b - 1, a - 1], D[b - 1, a], D[b, a - 1], D[b, a])
    out = np.zeros((dh * f, dw * f), depth.dtype)
    for y in range(dh * f):
        rows = [(y // f + 1, y % f)] + ([(y // f, f)] if y % f == 0 and y > 0 else [])
        for x in range(dw * f):
            cols = [(x // f + 1, x % f)] + ([(x // f, f)] if x % f == 0 and x > 0 else [])
            for b, q in rows:                               # the later row of cells first, in it the later column
                hit = [(a, p) for a, p in cols if b < dh and a < dw and valid[b, a]]
                if hit:
                    a, p = hit[0]
                    out[y, x] = stored(cell_value(D[b - 1, a - 1], D[b - 1, a], D[b, a - 1], D[b, a], f, p, q), depth.dtype)
                    break
    return out


def factor(width, height, dw, dh):
    """sf_depth_interpolation_factor."""
    if min(width, height, dw, dh) < 1 or height % dh or width % dw or height // dh != width // dw:
        return 0
    return height // dh


def mask_decimated(depth, width, height, min_depth=0.0, max_depth=0.0):
    """uint8 [height, width]: the detector mask the depth keyframe calls make of a depth image of its own size; None when the
    size does not divide the image's (no mask: the detector runs unmasked)."""
    dh, dw = np.asarray(depth).shape
    f = factor(width, height, dw, dh)
    if f == 0:
        return None
    return depth_ref.depth_mask(interpolate(depth, f), min_depth, max_depth)


def keypoints3d_depth_scaled(xy, depth, cam, width, height):
    """xyz float32 [n, 3]: depth_ref.keypoints3d_depth for a depth image of its own size under a width x height image."""
    from multi_robot_slam_separators_amd import _abi
    if getattr(xy, "dtype", None) == _abi.KEYPOINT_DTYPE:
        xy = np.stack([xy["x"], xy["y"]], axis=1)
    xy = np.asarray(xy, F32).reshape(-1, 2)
    dh, dw = np.asarray(depth).shape
    rx, ry = F32(1.0) / (F32(width) / F32(dw)), F32(1.0) / (F32(height) / F32(dh))
    with np.errstate(all="ignore"):
        scaled = np.stack([xy[:, 0] * rx, xy[:, 1] * ry], axis=1).astype(F32)
        cx, cy = F32(cam.cx) * rx, F32(cam.cy) * ry
        small = _abi.stereo_camera(float(F32(cam.fx) * rx), float(F32(cam.fy) * ry), float(cx) if cx > 0 else 0.0,
                                   float(cy) if cy > 0 else 0.0, 0.0, min_depth=cam.min_depth, max_depth=cam.max_depth)
    small.local_transform = cam.local_transform
    return depth_ref.keypoints3d_depth(scaled, depth, small)
