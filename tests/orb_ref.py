"""NumPy restatement of the GFTT/ORB descriptors (Vis/FeatureType 8, csrc/k_extract.hip k_orb_*): cv::ORB::compute on
given keypoints as rtabmap's GFTT_ORB::generateDescriptorsImpl calls it, one pyramid level.

Integer arithmetic where OpenCV's is integer (the 8-bit fixed-point blur, the intensity-centroid moments), float32 where
it is float (the rotated sample offsets: products and differences without contraction, then np.rint = cvRound; the
angle's cos / sin in float64 rounded to float32 once; fastAtan2)."""
import numpy as np

F32 = np.float32
HALF = 15            # ORB/PatchSize 31 // 2
BYTES = 32           # ORB/WTA_K 2


def default_pattern():
    """OpenCV's makeRandomPattern(31, 512): cv::RNG(0x34985739) (multiply-with-carry), uniform(-15, 16) for x then y of
    every point; test k = (point 2k, point 2k + 1).  int8 [256, 4].  NOT bit_pattern_31_."""
    s = 0x34985739
    out = np.zeros(512 * 2, np.int8)
    for t in range(out.size):
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) & 0xFFFFFFFFFFFFFFFF
        out[t] = (s & 0xFFFFFFFF) % 31 - 15
    return out.reshape(256, 4)


def blur_taps():
    """getGaussianKernel(7, 2, CV_32F) (float taps, float64 normalisation), each tap * 256 rounded to an integer."""
    cf = [F32(np.exp((-0.5 / (2.0 * 2.0)) * (i - 3.0) ** 2)) for i in range(7)]
    inv = 1.0 / sum(float(c) for c in cf)
    return np.array([int(np.rint(float(F32(float(c) * inv)) * 256.0)) for c in cf], np.int64)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101), vectorised."""
    p = np.array(p, np.int64, copy=True)
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def blur(img):
    """GaussianBlur(7 x 7, sigma 2, BORDER_REFLECT_101) in OpenCV 3.x's 8-bit fixed point: integer row sums, then
    (column sum + 2^15) >> 16 saturated to u8."""
    img = np.asarray(img)
    h, w = img.shape
    t = blur_taps()
    src = img.astype(np.int64)
    xs = np.arange(w)
    rows = sum(t[d] * src[:, reflect101(xs + d - 3, w)] for d in range(7))
    ys = np.arange(h)
    cols = sum(t[d] * rows[reflect101(ys + d - 3, h), :] for d in range(7))
    return np.minimum((cols + (1 << 15)) >> 16, 255).astype(np.uint8)


def umax():
    """ORB's half widths of the radius-15 circular patch rows (with the symmetry fix-up), [16]."""
    u = [0] * (HALF + 2)
    vmax = int(np.floor(F32(HALF) * np.sqrt(F32(2.0)) / F32(2) + F32(1)))
    vmin = int(np.ceil(F32(HALF) * np.sqrt(F32(2.0)) / F32(2)))
    for v in range(vmax + 1):
        u[v] = int(np.rint(np.sqrt(float(HALF * HALF - v * v))))
    v0 = 0
    for v in range(HALF, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u[:HALF + 1]


def fast_atan2(y, x):
    """cv::fastAtan2 (OpenCV 3.x) in float32: degrees in [0, 360)."""
    y = np.asarray(y, F32)
    x = np.asarray(x, F32)
    deg = F32(180.0 / np.pi)
    p1, p3 = F32(0.9997878412794807) * deg, F32(-0.3258083974640975) * deg
    p5, p7 = F32(0.1555786518463281) * deg, F32(-0.04432655554792128) * deg
    eps = F32(np.finfo(np.float64).eps)
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(first, ay / (ax + eps), ax / (ay + eps)).astype(F32)
    c2 = c * c
    poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(first, poly, F32(90.0) - poly).astype(F32)
    a = np.where(x < 0, F32(180.0) - a, a).astype(F32)
    return np.where(y < 0, F32(360.0) - a, a).astype(F32)


def ic_moments(img, cx, cy):
    """ORB's intensity-centroid moments (m01, m10) of the radius-15 patch around integer centres, int64."""
    img = np.asarray(img).astype(np.int64)
    cx, cy = np.asarray(cx, np.int64), np.asarray(cy, np.int64)
    um = umax()
    m01 = np.zeros(cx.shape, np.int64)
    m10 = np.zeros(cx.shape, np.int64)
    for v in range(-HALF, HALF + 1):
        d = um[abs(v)]
        u = np.arange(-d, d + 1)
        vals = img[(cy + v)[:, None], cx[:, None] + u[None, :]]
        m10 += (vals * u[None, :]).sum(axis=1)
        m01 += v * vals.sum(axis=1)
    return m01, m10


def inside(kp, w, h, edge):
    """KeyPointsFilter::runByImageBorder(edge) on cvRound(pt), and octave & 255 == 0."""
    if w <= 2 * edge or h <= 2 * edge:
        return np.zeros(len(kp), bool)
    rx, ry = np.rint(kp["x"].astype(F32)), np.rint(kp["y"].astype(F32))
    with np.errstate(invalid="ignore"):
        ok = (rx >= F32(edge)) & (rx < F32(w - edge)) & (ry >= F32(edge)) & (ry < F32(h - edge))
    return ok & ((kp["octave"] & 255) == 0)


def descriptors(img, blurred, x, y, angle, tests):
    """computeOrbDescriptors for corners at (x, y) with angles in degrees: [m, 32] u8, bits LSB first.  Samples inside
    the image read `blurred`, the others the (unblurred) reflect-101 padding of img."""
    img = np.asarray(img)
    h, w = img.shape
    cx = np.rint(np.asarray(x, F32)).astype(np.int64)
    cy = np.rint(np.asarray(y, F32)).astype(np.int64)
    ang = np.asarray(angle, F32) * F32(np.pi / 180.0)
    a = np.cos(ang.astype(np.float64)).astype(F32)[:, None]
    b = np.sin(ang.astype(np.float64)).astype(F32)[:, None]
    T = np.asarray(tests, np.int64).reshape(-1, 4)

    def sample(px, py):
        fx, fy = px.astype(F32)[None, :], py.astype(F32)[None, :]
        ix = np.rint((fx * a) - (fy * b)).astype(np.int64)
        iy = np.rint((fx * b) + (fy * a)).astype(np.int64)
        X, Y = cx[:, None] + ix, cy[:, None] + iy
        inimg = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        out = img[reflect101(Y, h), reflect101(X, w)].astype(np.int64)
        out[inimg] = blurred[Y[inimg], X[inimg]]
        return out
    bits = (sample(T[:, 0], T[:, 1]) < sample(T[:, 2], T[:, 3])).astype(np.uint8)
    return np.packbits(bits.reshape(len(cx), -1, 8), axis=2, bitorder="little").reshape(len(cx), -1)


def points3d(kp, right_x, status, cam, idx):
    """The 3D point of every corner in idx (NaN without one), as sf_extract_keyframe_device computes it."""
    f32 = F32
    p = np.full((len(idx), 3), np.nan, f32)
    if right_x is None:
        return p
    xi, yi = kp["x"][idx], kp["y"][idx]
    disp = xi - right_x[idx]
    ok = (disp > 0) if status is None else ((disp > 0) & (status[idx] != 0))
    c = f32(cam.cx_right - cam.cx) if (cam.cx_right > 0 and cam.cx > 0) else f32(0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = f32(cam.baseline) / (disp + c)
        X, Y, Z = (xi - f32(cam.cx)) * W, (yi - f32(cam.cy)) * W, f32(cam.fx) * W
    ok &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
    ok &= (cam.min_depth < 0) | (Z > f32(cam.min_depth))
    ok &= (cam.max_depth <= 0) | (Z <= f32(cam.max_depth))
    L = np.array(list(cam.local_transform), f32).reshape(3, 4)
    if np.array_equal(L, np.eye(4, dtype=f32)[:3]):
        q = np.stack([X, Y, Z], axis=1)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.stack([((L[r, 0] * X + L[r, 1] * Y) + L[r, 2] * Z) + L[r, 3] for r in range(3)], axis=1)
    p[ok] = q[ok].astype(f32)
    return p


def extract_keyframe(image, kp, right_x, status, cam, tests=None, edge=19, orientation=0):
    """What sf_extract_keyframe_device keeps with feature type 8: (descriptors [rows, 32], xyz [rows, 3], keypoints)."""
    image = np.asarray(image)
    h, w = image.shape
    tests = default_pattern() if tests is None else tests
    kp = np.array(kp, copy=True)
    idx = np.nonzero(inside(kp, w, h, edge))[0]
    if orientation and len(idx):
        m01, m10 = ic_moments(image, np.rint(kp["x"][idx]).astype(np.int64), np.rint(kp["y"][idx]).astype(np.int64))
        kp["angle"][idx] = fast_atan2(m01.astype(F32), m10.astype(F32))
    if len(idx):
        desc = descriptors(image, blur(image), kp["x"][idx], kp["y"][idx], kp["angle"][idx], tests)
    else:
        desc = np.zeros((0, BYTES), np.uint8)
    p = points3d(kp, right_x, status, cam, idx)
    keep = np.ones(len(idx), bool)
    if cam.min_depth > 0 or cam.max_depth > 0:
        keep = np.isfinite(p).all(axis=1)
    return desc[keep], p[keep], kp[idx][keep]
