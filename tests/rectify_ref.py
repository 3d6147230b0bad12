"""NumPy restatement of what the rectification calls do on the device (csrc/k_rectify.hip, csrc/sf_rectify.hip):
cv::initUndistortRectifyMap (float32 maps) followed by cv::remap(INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit images of one
or three channels [upstream OpenCV 3.2; neither function is in the reference tree, both restated from memory: DESIGN.md
section 3].  What the restatement decides, where upstream does otherwise:

  the inverse    iR = (P[:, :3] R)^-1 is the adjugate over the determinant in the order written in `inverse3` (upstream:
                 an LU inverse); a determinant that is 0 or not finite is refused
  X, Y, W        the closed form ((iR_0 j) + (iR_1 i)) + iR_2 per pixel (upstream: running sums along the row), so that
                 every pixel is computed on its own
  the model      k1 k2 p1 p2 k3 (plumb_bob) and k4 k5 k6 (rational_polynomial); no thin-prism, no tilt terms
  non-finite     a map value that is not finite, or whose 32-fold is >= 2^30 in magnitude, gives the pixel 0
  saturation     upstream saturates the integer coordinates to int16; with both image sizes <= 8192 a saturated
                 coordinate lies outside the source either way, so nothing is saturated here

Every float64 step is one rounded operation in the order written (no fused multiply-add); NumPy evaluates it so."""
import numpy as np

from tests import image_ref

PLUMB_BOB, RATIONAL = 0, 1
MAX_SIDE = 8192
INVALID = -(1 << 30)          # the fixed-point coordinate of a pixel the non-finite rule sets to 0: every tap is outside


def camera_info(width, height, K, D=(), R=None, P=None, model=PLUMB_BOB, out_width=0, out_height=0):
    """A sensor_msgs/CameraInfo-shaped block as a dict of float64 arrays; P None = [K | 0], R None = I."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.zeros(8, np.float64)
    d[:len(D)] = np.asarray(D, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    P = np.hstack([K, np.zeros((3, 1))]) if P is None else np.asarray(P, np.float64).reshape(3, 4)
    return dict(width=int(width), height=int(height), out_width=int(out_width), out_height=int(out_height), model=int(model),
                K=K.copy(), D=d, R=R.copy(), P=P.copy(), reserved=0)


def out_size(info):
    return (info["out_width"] or info["width"]), (info["out_height"] or info["height"])


def inverse3(m):
    """The adjugate over the determinant, every product and difference in the order written; None when the determinant is
    0 or not finite."""
    m = np.asarray(m, np.float64)
    (a, b, c), (d, e, f), (g, h, i) = m
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    if not np.isfinite(det) or det == 0.0:
        return None
    adj = np.array([[c00, c * h - b * i, b * f - c * e],
                    [c01, a * i - c * g, c * d - a * f],
                    [c02, b * g - a * h, a * e - b * d]], np.float64)
    return adj / det


def product3(p, r):
    """P[:, :3] R with every entry as ((p0 r0) + (p1 r1)) + (p2 r2)."""
    out = np.zeros((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (p[i, 0] * r[0, j] + p[i, 1] * r[1, j]) + p[i, 2] * r[2, j]
    return out


def check(info):
    """None, or the reason sf_rectify_plan_create refuses the block with."""
    vals = np.concatenate([info["K"].ravel(), info["D"], info["R"].ravel(), info["P"].ravel()])
    if not np.isfinite(vals).all():
        return "non-finite"
    if info["reserved"] != 0:
        return "reserved"
    if info["model"] not in (PLUMB_BOB, RATIONAL):
        return "model"
    ow, oh = out_size(info)
    if info["out_width"] < 0 or info["out_height"] < 0:
        return "size"
    for v in (info["width"], info["height"], ow, oh):
        if not 1 <= v <= MAX_SIDE:
            return "size"
    K, P = info["K"], info["P"]
    if not (K[0, 0] > 0 and K[1, 1] > 0 and P[0, 0] > 0 and P[1, 1] > 0):
        return "focal"
    if K[0, 1] != 0:
        return "skew"
    if inverse3(product3(P[:, :3], info["R"])) is None:
        return "singular"
    return None


def plan(info):
    """The constants a computed plan keeps: (iR [3, 3], (fx, fy, cx, cy), D [8] with k4 k5 k6 zero under plumb_bob)."""
    why = check(info)
    if why:
        raise ValueError("refused: " + why)
    iR = inverse3(product3(info["P"][:, :3], info["R"]))
    K = info["K"]
    D = info["D"].copy()
    if info["model"] == PLUMB_BOB:
        D[5:] = 0.0
    return iR, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), D


def maps64(info):
    """(mapx, mapy) float64 [out_h, out_w]: the value of every output pixel before its rounding to float32."""
    iR, (fx, fy, cx, cy), D = plan(info)
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    ow, oh = out_size(info)
    j = np.arange(ow, dtype=np.float64)[None, :]
    i = np.arange(oh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = ((iR[0, 0] * j) + (iR[0, 1] * i)) + iR[0, 2]
        Y = ((iR[1, 0] * j) + (iR[1, 1] * i)) + iR[1, 2]
        W = ((iR[2, 0] * j) + (iR[2, 1] * i)) + iR[2, 2]
        w = 1.0 / W
        x = X * w
        y = Y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        t = 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * t + p2 * (r2 + 2.0 * x2)
        yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * t
        return fx * xd + cx, fy * yd + cy


def maps(info):
    """(mapx, mapy) float32 [out_h, out_w]: what sf_rectify_maps_device writes."""
    mx, my = maps64(info)
    with np.errstate(all="ignore"):
        return mx.astype(np.float32), my.astype(np.float32)


def fixed(mapx, mapy):
    """float32 maps -> (sx, sy) int32 in 1/32 pixel: round-half-even of the float32 product; INVALID in both where a value
    is not finite or its 32-fold reaches 2^30."""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    with np.errstate(all="ignore"):
        vx, vy = mapx * np.float32(32.0), mapy * np.float32(32.0)
        ok = (np.abs(vx) < np.float32(2.0 ** 30)) & (np.abs(vy) < np.float32(2.0 ** 30))     # (NaN compares false)
        sx = np.where(ok, np.rint(np.where(ok, vx, 0)), INVALID).astype(np.int32)
        sy = np.where(ok, np.rint(np.where(ok, vy, 0)), INVALID).astype(np.int32)
    return sx, sy


def taps(sx, sy, src_w, src_h):
    """(ix, iy, weights [4, ...], inside [4, ...]) of the taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1)."""
    ix, iy = sx >> 5, sy >> 5                      # arithmetic shifts: floor for negatives
    a, b = (sx & 31).astype(np.int64), (sy & 31).astype(np.int64)
    wts = np.stack([32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b])
    xs = np.stack([ix, ix + 1, ix, ix + 1]).astype(np.int64)
    ys = np.stack([iy, iy, iy + 1, iy + 1]).astype(np.int64)
    inside = (xs >= 0) & (xs < src_w) & (ys >= 0) & (ys < src_h)
    return xs, ys, wts, inside


def remap(src, sx, sy):
    """src uint8 [h, w] or [h, w, ch] -> uint8 [out_h, out_w(, ch)]: (sum of weight x tap + 16384) >> 15, a tap outside
    the source reads 0."""
    src = np.asarray(src, np.uint8)
    planar = src.ndim == 2
    s = (src[..., None] if planar else src).astype(np.int64)
    h, w = s.shape[:2]
    xs, ys, wts, inside = taps(sx, sy, w, h)
    assert (wts.sum(axis=0) == 32768).all()
    acc = np.zeros(sx.shape + (s.shape[2],), np.int64)
    for k in range(4):
        px = s[np.clip(ys[k], 0, h - 1), np.clip(xs[k], 0, w - 1)] * inside[k][..., None]
        acc += wts[k][..., None] * px
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out[..., 0] if planar else out


def border_share(sx, sy, src_w, src_h):
    """The share of output pixels with at least one tap outside the source."""
    inside = taps(sx, sy, src_w, src_h)[3]
    return float((~inside.all(axis=0)).mean())


def rectify(src, info):
    """A raw image under a computed plan."""
    src = np.asarray(src, np.uint8)
    assert src.shape[:2] == (info["height"], info["width"])
    return remap(src, *fixed(*maps(info)))


def rectify_maps(src, mapx, mapy):
    """A raw image under caller maps (sf_rectify_plan_from_maps)."""
    return remap(src, *fixed(mapx, mapy))


def to_gray(img, format, rule=0):
    """The fused gray output: the handle's gray rule on the rectified colour pixel (tests/image_ref.py)."""
    return image_ref.gray(img, format, rule)


def rotation(rx, ry, rz):
    """Rz Ry Rx of three small angles (radians): a rectification rotation for the cases below."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def case_info(kind, width, height, out_width=0, out_height=0, side=0):
    """The calibrations the tests share, scaled from a 752 x 480 head to width x height; side 0 / 1 = left / right camera
    (another rotation, other coefficients, P with the baseline term).
      "barrel"    plumb_bob with visible barrel distortion (the magnitudes of a EuRoC-style cam0), a rotation of a few
                  degrees, P close to K
      "rational"  all eight terms
      "strong"    the barrel set seen through a P of 0.62 times the focal length and a larger rotation: the rectified image
                  looks past the raw one, so a fair share of the output has taps outside the source"""
    s = width / 752.0
    fx, fy, cx, cy = 458.654 * s, 457.296 * s, 367.215 * s, 248.375 * height / 480.0
    K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
    ow, oh = out_width or width, out_height or height
    sgn = -1.0 if side else 1.0
    if kind == "barrel":
        D = [-0.28340811 + 0.01 * side, 0.07395907, 0.00019359, 1.76187114e-05 * sgn, 0.0]
        R, f, model = rotation(0.012 * sgn, -0.021, 0.016), 0.97, PLUMB_BOB
    elif kind == "rational":
        D = [0.51, 0.12 - 0.01 * side, 3.1e-4, -2.3e-4 * sgn, 0.011, 0.83, 0.21, 0.018]
        R, f, model = rotation(-0.015, 0.018 * sgn, -0.011), 1.02, RATIONAL
    elif kind == "strong":
        D = [-0.28340811, 0.07395907 + 0.004 * side, 0.0012 * sgn, -0.0009, 0.0]
        R, f, model = rotation(0.03 * sgn, -0.045, 0.05), 0.62, PLUMB_BOB
    else:
        raise ValueError(kind)
    pfx, pfy = f * fx, f * fy
    P = [[pfx, 0, ow / 2.0 + 1.7, -0.11 * pfx * side], [0, pfy, oh / 2.0 - 2.3, 0], [0, 0, 1, 0]]
    return camera_info(width, height, K, D, R, P, model, out_width, out_height)


def stereo_camera_from_info(left, right):
    """(fx, fy, cx, cy, cx_right, baseline) of the rectified pair, float64; None where the baseline is not positive."""
    Pl, Pr = left["P"], right["P"]
    baseline = -Pr[0, 3] / Pr[0, 0]
    if not baseline > 0:
        return None
    return Pl[0, 0], Pl[1, 1], Pl[0, 2], Pl[1, 2], Pr[0, 2], baseline
