"""NumPy restatement of the guided pass with Vis/CorGuessMatchToProjection = true (myRegistrationVis.cpp:476-666): every
"to" keypoint is matched to the projections of the "from" points inside its guess_win_size-pixel window.  Written from
the reference text, not from the kernel (k_guided_tp, multi_robot_slam_separators_amd/csrc/k_guided.hip).

Arithmetic follows the project's canonical order (DESIGN.md sections 3-4): the pose composition and the depth test in
float32, cv::projectPoints in double, the window test as the exact float32 d2 < r^2 of the other branch, float32 rows
compared by NORM_L2SQR (:580) summed in dimension order without a square root, binary rows by Hamming distance.
"""
import numpy as np

F32 = np.float32


def octave(o):
    """:560-561 (and :574-575 for "from"): the low byte, sign-extended."""
    v = np.asarray(o, dtype=np.int64) & 255
    return np.where(v < 128, v, -128 | v)


def camera(params, guess):
    """:486-487 guessCameraRef = (guess * localTransform).inverse() in float32: (Rc [3][3], tc [3])."""
    g = np.asarray(guess, dtype=F32).reshape(12)
    L = np.array([params.local_transform[i] for i in range(12)], dtype=F32)
    GR = np.zeros(9, dtype=F32)
    Gt = np.zeros(3, dtype=F32)
    for i in range(3):
        for j in range(3):
            GR[3 * i + j] = F32(F32(g[4 * i] * L[j]) + F32(g[4 * i + 1] * L[4 + j])) + F32(g[4 * i + 2] * L[8 + j])
        Gt[i] = F32(F32(F32(g[4 * i] * L[3]) + F32(g[4 * i + 1] * L[7])) + F32(g[4 * i + 2] * L[11])) + g[4 * i + 3]
    Rc = np.zeros(9, dtype=F32)
    for i in range(3):
        for j in range(3):
            Rc[3 * i + j] = GR[3 * j + i]
    tc = np.zeros(3, dtype=F32)
    for i in range(3):
        tc[i] = -(F32(F32(Rc[3 * i] * Gt[0]) + F32(Rc[3 * i + 1] * Gt[1])) + F32(Rc[3 * i + 2] * Gt[2]))
    return Rc, tc


def project(params, guess, xyz):
    """:488-515: (u, v) float32 of every "from" point, whether it is finite, and whether it is kept (inside the image,
    z > 0 in the camera frame)."""
    Rc, tc = camera(params, guess)
    P = np.asarray(xyz, dtype=F32).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(all="ignore"):
        zf = ((Rc[6] * x + Rc[7] * y) + Rc[8] * z) + tc[2]
        Rd, td = Rc.astype(np.float64), tc.astype(np.float64)
        xd, yd, zd = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        X = ((Rd[0] * xd + Rd[1] * yd) + Rd[2] * zd) + td[0]
        Y = ((Rd[3] * xd + Rd[4] * yd) + Rd[5] * zd) + td[1]
        Z = ((Rd[6] * xd + Rd[7] * yd) + Rd[8] * zd) + td[2]
        iz = np.where(Z != 0.0, 1.0 / np.where(Z != 0.0, Z, 1.0), 1.0)
        u = ((X * iz) * params.fx + params.cx).astype(F32)
        v = ((Y * iz) * params.fy + params.cy).astype(F32)
        wlim, hlim = F32(params.image_width - 1), F32(params.image_height - 1)
        kept = (finite & np.isfinite(u) & np.isfinite(v) & ~(u < 0) & ~(u >= wlim) & ~(v < 0) & ~(v >= hlim) &
                (zf > 0))
    return u, v, finite, kept


def distance(desc_type, row_to, rows_from):
    """Distances of one "to" row to several "from" rows (float32): Hamming for binary rows (uint8), NORM_L2SQR for float32
    rows -- sum of squared differences in dimension order, rounded after every operation, no square root (:580)."""
    if desc_type == 1:
        a = np.asarray(row_to).view(F32).reshape(-1)
        b = np.asarray(rows_from).view(F32).reshape(len(rows_from), -1)
        acc = np.zeros(len(b), dtype=F32)
        for c in range(a.size):
            d = (a[c] - b[:, c]).astype(F32)
            acc = (acc + (d * d).astype(F32)).astype(F32)
        return acc
    x = np.bitwise_xor(np.asarray(rows_from, dtype=np.uint8), np.asarray(row_to, dtype=np.uint8)[None, :])
    return np.unpackbits(x, axis=1).sum(axis=1).astype(F32)


def eligible(params, guess, guess_is_null, f_from, f_to):
    """:476-479 (and stereoCamGeometricTools.cpp:153-164): pass 2 is the guided pass."""
    g = np.asarray(guess, dtype=F32).reshape(12)
    ident = np.array_equal(g, np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F32))
    calibrated = params.image_width > 0 and params.image_height > 0 and params.fx > 0 and params.fy > 0
    return (not guess_is_null and not ident and params.guess_win_size > 0 and f_from.xyz.shape[0] > 0 and calibrated and
            f_from.desc.shape[0] > 0 and f_to.desc.shape[0] > 0)


def match_to_projection(params, guess, f_from, f_to):
    """The pass-2 correspondence list of an eligible pair: (corr_from uint16, corr_to uint16, words_from, words_to,
    words_to_2d).  f_from / f_to: _abi.FeatureArrays."""
    kf, kt = f_from.desc.shape[0], f_to.desc.shape[0]
    u, v, finite, kept = project(params, guess, f_from.xyz)
    n_finite = int(finite.sum())
    P = np.nonzero(kept)[0]                         # the projected list, ascending "from" index (:500-512)
    if P.size == 0:                                 # :820-823: no word at all
        return np.zeros(0, np.uint16), np.zeros(0, np.uint16), 0, 0, 0
    oct_from = octave(f_from.kpts["octave"])
    oct_to = octave(f_to.kpts["octave"])
    r2 = F32(params.guess_win_size) * F32(params.guess_win_size)
    nndr = F32(params.nndr)
    tx = f_to.kpts["x"].astype(F32)
    ty = f_to.kpts["y"].astype(F32)
    accepted_by = {}                                # "from" index -> the "to" keypoints that accepted it
    for i in range(kt):
        with np.errstate(invalid="ignore", over="ignore"):
            dx = (u[P] - tx[i]).astype(F32)
            dy = (v[P] - ty[i]).astype(F32)
            d2 = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
        cand = P[d2 < r2]                           # :532-534 radius search (exact)
        same = cand[oct_from[cand] == oct_to[i]]    # :564-573 / :593-597
        m = -1
        if same.size >= 2:                          # :575-585 kNN-2 + NNDR
            d = distance(params.desc_type, f_to.desc[i], f_from.desc[same])
            order = np.lexsort((same, d))           # (distance, then lowest index)
            if d[order[0]] < nndr * d[order[1]]:
                m = int(same[order[0]])
        elif same.size == 1:                        # :587-590 and :593-602: no descriptor test
            m = int(same[0])
        if m >= 0:
            accepted_by.setdefault(m, []).append(i)
    # :604-625 first match -> words3From, later ones only duplicate wordsTo entries; uMultimapToMapUnique keeps the ids
    # with exactly one entry
    ids = sorted(k for k, t in accepted_by.items() if len(t) == 1)
    cf = np.array(ids, dtype=np.uint16)
    ct = np.array([accepted_by[k][0] for k in ids], dtype=np.uint16)
    words_from = n_finite                           # :652-665 + the matched ones: every finite "from" point
    words_to = kt if f_to.xyz.shape[0] > 0 else 0
    return cf, ct, words_from, words_to, kt
