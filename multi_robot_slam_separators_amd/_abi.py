"""ctypes mirror of include/sepfinder.h (POD structs + constants of the C-ABI boundary).

Layouts follow the reference's wire types (PKG = ros_ws/src/multi_robot_separators):
PKG/msg/Descriptors.msg:1-3, KeyPoint3DVec.msg:1-2, KeyPointVec.msg:1-2,
PKG/srv/EstTransform.srv:1-9, PKG/srv/ReceiveSeparators.srv:1-10.
"""
import ctypes as C

import numpy as np

SF_OK, SF_EINVAL, SF_EHIP, SF_ENOMEM, SF_ERANGE, SF_ENODEV, SF_ERCCL = range(7)
SF_MAX_FEATURES = 32767
SF_MAX_DESC_BYTES = 64
SF_MAX_DESC_BYTES_F32 = 512
SF_DESC_BYTES_U8 = 128     # uint8 rows compared by L2 (sf_params.desc_type 2)

(SF_K_MATCH, SF_K_RANSAC1, SF_K_GUIDED, SF_K_RANSAC2, SF_K_NN, SF_K_NN_SELECT, SF_K_NN_FILTER,
 SF_K_NN_REFINE, SF_K_FUSED, SF_K_NN_WALK, SF_K_BA, SF_K_GUIDED_TP, SF_K_COUNT) = range(13)
(SF_OPT_MATCH_MFMA, SF_OPT_FUSED, SF_OPT_OVERLAP, SF_OPT_CHAIN_WAVES, SF_OPT_DEBUG_CORR, SF_OPT_NN_FULL_FILTER,
 SF_OPT_STEP_OVERLAP, SF_OPT_STEP_SPLIT, SF_OPT_STEP_DEPTH, SF_OPT_STEP_LANES, SF_OPT_STEP_DEVICE_WALK,
 SF_OPT_STEP_SPECULATE, SF_OPT_CHAIN_NARROW_EST) = range(13)      # sf_set_option
SF_OPT_RECTIFY_TABLE = 13      # computed rectification plans: 1 (default) the table form, 0 the computed form

STATUS_NAMES = {0: "SF_OK", 1: "SF_EINVAL", 2: "SF_EHIP", 3: "SF_ENOMEM", 4: "SF_ERANGE", 5: "SF_ENODEV", 6: "SF_ERCCL"}


class Params(C.Structure):
    _fields_ = [
        ("netvlad_distance", C.c_double),
        ("netvlad_dimensions", C.c_int32),
        ("netvlad_max_matches_nb", C.c_int32),
        ("nn_precision", C.c_int32),
        ("min_inliers", C.c_int32),
        ("inlier_distance", C.c_float),
        ("iterations", C.c_int32),
        ("refine_iterations", C.c_int32),
        ("refine_sigma", C.c_double),
        ("estimation_type", C.c_int32),
        ("nndr", C.c_float),
        ("guess_win_size", C.c_int32),
        ("ransac_adaptive_stop", C.c_int32),
        ("max_sample_checks", C.c_int32),
        ("seed", C.c_uint64),
        ("fx", C.c_double),
        ("fy", C.c_double),
        ("cx", C.c_double),
        ("cy", C.c_double),
        ("image_width", C.c_int32),
        ("image_height", C.c_int32),
        ("local_transform", C.c_float * 12),
        ("store_capacity", C.c_int32),
        ("max_features", C.c_int32),
        ("desc_bytes", C.c_int32),
        ("pnp_reproj_error", C.c_float),
        ("pnp_flags", C.c_int32),
        ("pnp_refine_iterations", C.c_int32),
        ("bundle_adjustment", C.c_int32),
        ("ba_iterations", C.c_int32),
        ("ba_robust_kernel_delta", C.c_float),
        ("ba_pixel_variance", C.c_float),
        ("stereo_baseline", C.c_float),
        ("force_3dof", C.c_int32),
        ("forward_est_only", C.c_int32),
        ("desc_type", C.c_int32),
        ("guess_match_to_projection", C.c_int32),
    ]


class Keypoint(C.Structure):
    _fields_ = [
        ("x", C.c_float),
        ("y", C.c_float),
        ("size", C.c_float),
        ("angle", C.c_float),
        ("response", C.c_float),
        ("octave", C.c_int32),
        ("class_id", C.c_int32),
    ]


KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")]
)
assert KEYPOINT_DTYPE.itemsize == C.sizeof(Keypoint) == 28


class StereoCamera(C.Structure):
    """sf_stereo_camera (include/sepfinder.h): the stereo model of sf_extract_keyframe_device."""
    _fields_ = [
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("cx_right", C.c_float), ("baseline", C.c_float),
        ("local_transform", C.c_float * 12),
        ("min_depth", C.c_float), ("max_depth", C.c_float),
    ]


def stereo_camera(fx, fy, cx, cy, baseline, cx_right=0.0, local_transform=None, min_depth=0.0, max_depth=0.0):
    cam = StereoCamera()
    cam.fx, cam.fy, cam.cx, cam.cy, cam.cx_right, cam.baseline = fx, fy, cx, cy, cx_right, baseline
    lt = np.eye(4, dtype=np.float32)[:3] if local_transform is None else np.asarray(local_transform, np.float32).reshape(3, 4)
    for i, v in enumerate(lt.ravel()):
        cam.local_transform[i] = float(v)
    cam.min_depth, cam.max_depth = min_depth, max_depth
    return cam


class CameraModel(C.Structure):
    """sf_camera_model (include/sepfinder.h): one entry of the handle's camera table (sf_camera_add)."""
    _fields_ = [
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("image_width", C.c_int32), ("image_height", C.c_int32),
        ("local_transform", C.c_float * 12),
        ("stereo_baseline", C.c_float),
        ("reserved", C.c_int32),
    ]


assert C.sizeof(CameraModel) == 96
SF_MAX_CAMERAS = 255


def camera_model(fx, fy, cx, cy, image_width, image_height, local_transform=None, stereo_baseline=0.0):
    m = CameraModel()
    m.fx, m.fy, m.cx, m.cy = fx, fy, cx, cy
    m.image_width, m.image_height = int(image_width), int(image_height)
    lt = np.eye(4, dtype=np.float32)[:3] if local_transform is None else np.asarray(local_transform, np.float32).reshape(3, 4)
    for i, v in enumerate(lt.ravel()):
        m.local_transform[i] = float(v)
    m.stereo_baseline = stereo_baseline
    m.reserved = 0
    return m


class StereoFlowParams(C.Structure):
    """sf_stereo_flow_params (include/sepfinder.h): cv::calcOpticalFlowPyrLK + disparity gate of the stereo correspondence."""
    _fields_ = [
        ("win_width", C.c_int32), ("win_height", C.c_int32), ("max_level", C.c_int32), ("iterations", C.c_int32),
        ("epsilon", C.c_double), ("min_disparity", C.c_float), ("max_disparity", C.c_float),
        ("min_eig_threshold", C.c_float),
    ]


def stereo_flow_params(win_width=15, win_height=3, max_level=5, iterations=30, epsilon=0.01, min_disparity=0.5,
                       max_disparity=128.0, min_eig_threshold=1e-4):
    """rtabmap's Stereo/* defaults (what sf_stereo_flow_defaults fills)."""
    p = StereoFlowParams()
    p.win_width, p.win_height, p.max_level, p.iterations = win_width, win_height, max_level, iterations
    p.epsilon, p.min_disparity, p.max_disparity, p.min_eig_threshold = epsilon, min_disparity, max_disparity, min_eig_threshold
    return p


class DetectorParams(C.Structure):
    """sf_detector_params (include/sepfinder.h): cv::goodFeaturesToTrack's arguments in sf_get_features_and_descriptor."""
    _fields_ = [("max_features", C.c_int32), ("quality_level", C.c_double), ("min_distance", C.c_double)]


def detector_params(max_features=1000, quality_level=0.001, min_distance=3.0):
    """rtabmap's Vis/MaxFeatures, GFTT/QualityLevel, GFTT/MinDistance defaults (what sf_detector_defaults fills)."""
    p = DetectorParams()
    p.max_features, p.quality_level, p.min_distance = max_features, quality_level, min_distance
    return p


class OrbParams(C.Structure):
    """sf_orb_params (include/sepfinder.h): rtabmap's ORB/ parameters of the GFTT/ORB extraction (Vis/FeatureType 8)."""
    _fields_ = [("edge_threshold", C.c_int32), ("patch_size", C.c_int32), ("wta_k", C.c_int32), ("orientation", C.c_int32)]


def orb_params(edge_threshold=19, patch_size=31, wta_k=2, orientation=0):
    """ORB/EdgeThreshold, ORB/PatchSize, ORB/WTA_K defaults (what sf_orb_defaults fills); orientation 1 = ORB's
    intensity-centroid angle instead of the keypoint's own."""
    p = OrbParams()
    p.edge_threshold, p.patch_size, p.wta_k, p.orientation = edge_threshold, patch_size, wta_k, orientation
    return p


class FastParams(C.Structure):
    """sf_fast_params (include/sepfinder.h): rtabmap's FAST/ parameters of the FAST detector (Vis/FeatureType 4)."""
    _fields_ = [("threshold", C.c_int32), ("nonmax_suppression", C.c_int32)]


def fast_params(threshold=20, nonmax_suppression=1):
    """FAST/Threshold, FAST/NonmaxSuppression defaults (what sf_fast_defaults fills)."""
    p = FastParams()
    p.threshold, p.nonmax_suppression = threshold, nonmax_suppression
    return p


class GfttParams(C.Structure):
    """sf_gftt_params (include/sepfinder.h): rtabmap's GFTT/BlockSize, GFTT/UseHarrisDetector and GFTT/K -- the response of
    the GFTT detector (detect_corners_device; Vis/FeatureType 5, 6 and 8)."""
    _fields_ = [("block_size", C.c_int32), ("use_harris_detector", C.c_int32), ("k", C.c_double)]


def gftt_params(block_size=3, use_harris_detector=0, k=0.04):
    """GFTT/BlockSize, GFTT/UseHarrisDetector, GFTT/K defaults (what sf_gftt_defaults fills)."""
    p = GfttParams()
    p.block_size, p.use_harris_detector, p.k = block_size, use_harris_detector, k
    return p


class FrontParams(C.Structure):
    """sf_front_params (include/sepfinder.h): what rtabmap's Feature2D::generateKeypoints puts around every detector --
    Vis/RoiRatios {left, right, top, bottom} and cv::cornerSubPix (Vis/SubPixWinSize, SubPixIterations, SubPixEps)."""
    _fields_ = [("roi_ratios", C.c_float * 4), ("subpix_win_size", C.c_int32), ("subpix_iterations", C.c_int32),
                ("subpix_eps", C.c_float)]


assert C.sizeof(FrontParams) == 28


def front_params(roi_ratios=(0.0, 0.0, 0.0, 0.0), subpix_win_size=3, subpix_iterations=0, subpix_eps=0.02):
    """rtabmap's defaults (what sf_front_defaults fills): no ROI, no refinement (0 iterations)."""
    p = FrontParams()
    for k in range(4):
        p.roi_ratios[k] = roi_ratios[k]
    p.subpix_win_size, p.subpix_iterations, p.subpix_eps = subpix_win_size, subpix_iterations, subpix_eps
    return p


class StereoParams(C.Structure):
    """sf_stereo_params (include/sepfinder.h): which stereo correspondence the extraction calls run -- Stereo/OpticalFlow
    (1 = pyramidal LK, 0 = block matching) and Stereo/SSD (block matching: 1 = squared, 0 = absolute differences)."""
    _fields_ = [("optical_flow", C.c_int32), ("ssd", C.c_int32)]


assert C.sizeof(StereoParams) == 8


def stereo_params(optical_flow=1, ssd=1):
    """rtabmap's defaults (what sf_stereo_defaults fills): pyramidal LK; squared differences where block matching runs."""
    p = StereoParams()
    p.optical_flow, p.ssd = optical_flow, ssd
    return p


SF_DEPTH_U16_MM, SF_DEPTH_F32_M = 0, 1          # sf_depth_format: uint16 millimetres / float32 metres
DEPTH_DTYPES = {SF_DEPTH_U16_MM: np.dtype(np.uint16), SF_DEPTH_F32_M: np.dtype(np.float32)}


class DepthParams(C.Structure):
    """sf_depth_params (include/sepfinder.h): Vis/DepthAsMask of the depth keyframe calls."""
    _fields_ = [("depth_as_mask", C.c_int32)]


assert C.sizeof(DepthParams) == 4


def depth_params(depth_as_mask=1):
    """rtabmap's default (what sf_depth_defaults fills): the detector sees the mask of the depth image."""
    p = DepthParams()
    p.depth_as_mask = depth_as_mask
    return p


class DepthSize(C.Structure):
    """sf_depth_size (include/sepfinder.h): the depth images' own size in the depth calls; {0, 0}: the image's."""
    _fields_ = [("depth_width", C.c_int32), ("depth_height", C.c_int32)]


assert C.sizeof(DepthSize) == 8


def depth_size(w=0, h=0):
    """A fresh handle's value: the depth image has the image's width and height."""
    s = DepthSize()
    s.depth_width, s.depth_height = w, h
    return s


class DepthRegistration(C.Structure):
    """sf_depth_registration (include/sepfinder.h): the depth camera, the colour camera with its image size, the transform
    between them and the two flags of the hole filling; what sf_depth_register_device takes."""
    _fields_ = [
        ("depth_width", C.c_int32), ("depth_height", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("rfx", C.c_float), ("rfy", C.c_float), ("rcx", C.c_float), ("rcy", C.c_float),
        ("transform", C.c_float * 12),
        ("fill_vertical", C.c_int32), ("fill_horizontal", C.c_int32), ("reserved", C.c_int32),
    ]


assert C.sizeof(DepthRegistration) == 108


def depth_registration(depth_width, depth_height, depth_k, width, height, colour_k, transform=None, fill_vertical=0,
                       fill_horizontal=0):
    """depth_k = (fx, fy, cx, cy) of the depth camera, colour_k = (rfx, rfy, rcx, rcy) of the colour camera whose images are
    width x height; transform [3, 4] takes a point of the depth camera's frame into the colour camera's (None: identity)."""
    r = DepthRegistration()
    r.depth_width, r.depth_height, r.width, r.height = int(depth_width), int(depth_height), int(width), int(height)
    r.fx, r.fy, r.cx, r.cy = (float(v) for v in depth_k)
    r.rfx, r.rfy, r.rcx, r.rcy = (float(v) for v in colour_k)
    t = np.eye(3, 4, dtype=np.float32) if transform is None else np.asarray(transform, np.float32).reshape(3, 4)
    r.transform[:] = t.ravel().tolist()
    r.fill_vertical, r.fill_horizontal, r.reserved = int(fill_vertical), int(fill_horizontal), 0
    return r


def depth_format_of(depth):
    """The sf_depth_format of a depth image given as a uint16 or float32 array."""
    for fmt, dt in DEPTH_DTYPES.items():
        if depth.dtype == dt:
            return fmt
    raise ValueError("depth images are uint16 (millimetres) or float32 (metres), not %s" % depth.dtype)


def compute_roi(width, height, ratios):
    """Feature2D::computeRoi restated: (x, y, w, h) of the sub-image the detector sees for Vis/RoiRatios {left, right,
    top, bottom}.  Float32 arithmetic with C++'s truncating assignment; ValueError for what sf_compute_roi refuses (a
    ratio outside [0, 1], an empty image, a ROI side below 3)."""
    f = np.float32
    r = [f(v) for v in ratios]
    if len(r) != 4 or width < 1 or height < 1 or not all(f(0) <= v <= f(1) for v in r):
        raise ValueError("Vis/RoiRatios %s on %d x %d" % (list(ratios), width, height))

    def side(n, lo, hi):
        o = 0
        if lo > 0 and lo < f(1) - hi:
            o = int(f(n) * lo)
        m = n - o
        if hi > 0 and hi < f(1) - lo:
            m = int(f(m) - f(n) * hi)
        return o, m

    x, w = side(width, r[0], r[1])
    y, h = side(height, r[2], r[3])
    if w < 3 or h < 3:
        raise ValueError("Vis/RoiRatios %s leave %d x %d of %d x %d" % (list(ratios), w, h, width, height))
    return x, y, w, h


class GridParams(C.Structure):
    """sf_grid_params (include/sepfinder.h): Vis/GridRows x Vis/GridCols of Feature2D::generateKeypoints -- the detector of
    feature types 4, 6 and 8 runs on every cell of the ROI and keeps ceil(max_features / cells) keypoints there."""
    _fields_ = [("grid_rows", C.c_int32), ("grid_cols", C.c_int32)]


assert C.sizeof(GridParams) == 8


def grid_params(grid_rows=1, grid_cols=1):
    """rtabmap's defaults (what sf_grid_defaults fills): 1 x 1, no cells."""
    p = GridParams()
    p.grid_rows, p.grid_cols = grid_rows, grid_cols
    return p


def compute_grid(width, height, roi_ratios, grid_rows, grid_cols, max_features):
    """The cells of Vis/GridRows x Vis/GridCols restated: (x, y, col_size, row_size, quota, rows_cap) -- the first cell's
    origin (the ROI's), the cells' size (integer division: the remainder columns and rows belong to no cell), the
    keypoints a cell may keep, ceil(max_features / cells) in float32, and the rows a keyframe can hold.  ValueError for what
    sf_compute_grid answers with SF_EINVAL (compute_roi's refusals, a grid value outside 1 .. 16, max_features < 1, a cell
    side below 3), OverflowError for its SF_ERANGE (rows_cap > SF_MAX_FEATURES)."""
    if not (1 <= grid_rows <= 16 and 1 <= grid_cols <= 16) or max_features < 1:
        raise ValueError("Vis/GridRows %d, Vis/GridCols %d, %d features" % (grid_rows, grid_cols, max_features))
    x, y, w, h = compute_roi(width, height, roi_ratios)
    cells = grid_rows * grid_cols
    quota = int(np.ceil(np.float32(max_features) / np.float32(cells)))
    col_size, row_size = w // grid_cols, h // grid_rows
    if col_size < 3 or row_size < 3:
        raise ValueError("%d x %d cells of %d x %d in a ROI of %d x %d" % (grid_rows, grid_cols, col_size, row_size, w, h))
    if cells * quota > SF_MAX_FEATURES:
        raise OverflowError("%d cells of %d keypoints > %d" % (cells, quota, SF_MAX_FEATURES))
    return x, y, col_size, row_size, quota, cells * quota


class OrbDetectorParams(C.Structure):
    """sf_orb_detector_params (include/sepfinder.h): rtabmap's ORB/ parameters of the ORB detector (Vis/FeatureType 2)."""
    _fields_ = [("scale_factor", C.c_float), ("n_levels", C.c_int32), ("first_level", C.c_int32), ("score_type", C.c_int32),
                ("fast_threshold", C.c_int32)]


def orb_detector_params(scale_factor=2.0, n_levels=3, first_level=0, score_type=0, fast_threshold=20):
    """ORB/ScaleFactor, ORB/NLevels, ORB/FirstLevel, ORB/ScoreType (0 = Harris, 1 = FAST), ORB/FastThreshold: rtabmap's
    defaults (what sf_orb_detector_defaults fills)."""
    p = OrbDetectorParams()
    p.scale_factor, p.n_levels, p.first_level, p.score_type, p.fast_threshold = (scale_factor, n_levels, first_level,
                                                                                 score_type, fast_threshold)
    return p


FEATURE_GFTT_BRIEF = 6   # Vis/FeatureType values of sf_set_feature_type
FEATURE_GFTT_ORB = 8
FEATURE_FAST_BRIEF = 4
FEATURE_ORB = 2          # ... and of sf_set_feature_type_orb
FEATURE_FAST_FREAK = 3   # ... and of sf_set_feature_type_freak
FEATURE_GFTT_FREAK = 5


class FreakParams(C.Structure):
    """sf_freak_params (include/sepfinder.h): rtabmap's FREAK/ parameters (Vis/FeatureType 3 and 5)."""
    _fields_ = [("orientation_normalized", C.c_int32), ("scale_normalized", C.c_int32), ("pattern_scale", C.c_float),
                ("n_octaves", C.c_int32)]


def freak_params(orientation_normalized=1, scale_normalized=1, pattern_scale=22.0, n_octaves=4):
    """FREAK/OrientationNormalized, FREAK/ScaleNormalized, FREAK/PatternScale, FREAK/NOctaves: rtabmap's defaults (what
    sf_freak_defaults fills)."""
    p = FreakParams()
    p.orientation_normalized, p.scale_normalized, p.pattern_scale, p.n_octaves = (orientation_normalized, scale_normalized,
                                                                                  pattern_scale, n_octaves)
    return p


FREAK_SCALES, FREAK_ORIENTATIONS, FREAK_POINTS, FREAK_PAIRS, FREAK_ALL_PAIRS, FREAK_BYTES = 64, 256, 43, 512, 903, 64
FEATURE_SURF = 0         # ... and of sf_set_feature_type_surf (a handle with desc_type 1)


class SurfParams(C.Structure):
    """sf_surf_params (include/sepfinder.h): rtabmap's SURF/ parameters (Vis/FeatureType 0)."""
    _fields_ = [("hessian_threshold", C.c_float), ("n_octaves", C.c_int32), ("n_octave_layers", C.c_int32),
                ("upright", C.c_int32), ("extended", C.c_int32)]


def surf_params(hessian_threshold=500.0, n_octaves=4, n_octave_layers=2, upright=0, extended=0):
    """SURF/HessianThreshold, SURF/Octaves, SURF/OctaveLayers, SURF/Upright, SURF/Extended: rtabmap's defaults (what
    sf_surf_defaults fills)."""
    p = SurfParams()
    p.hessian_threshold, p.n_octaves, p.n_octave_layers, p.upright, p.extended = (hessian_threshold, n_octaves,
                                                                                  n_octave_layers, upright, extended)
    return p


SURF_ORI_SAMPLES, SURF_PATCH = 109, 20
FEATURE_SIFT = 1         # ... and of sf_set_feature_type_sift (a handle with desc_type 1 and desc_bytes 512, or desc_type 2)


class SiftParams(C.Structure):
    """sf_sift_params (include/sepfinder.h): rtabmap's SIFT/ parameters."""
    _fields_ = [("n_features", C.c_int32), ("n_octave_layers", C.c_int32), ("contrast_threshold", C.c_float),
                ("edge_threshold", C.c_float), ("sigma", C.c_float)]


def sift_params(n_features=0, n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
    """SIFT/NFeatures, SIFT/NOctaveLayers, SIFT/ContrastThreshold, SIFT/EdgeThreshold, SIFT/Sigma: rtabmap's defaults (what
    sf_sift_defaults fills)."""
    p = SiftParams()
    p.n_features, p.n_octave_layers, p.contrast_threshold, p.edge_threshold, p.sigma = (n_features, n_octave_layers,
                                                                                          contrast_threshold, edge_threshold, sigma)
    return p


SIFT_MAX_OCTAVES, SIFT_MAX_LAYERS, SIFT_MAX_KLEN = 16, 8, 520


SF_IMAGE_RGB8, SF_IMAGE_BGR8, SF_IMAGE_MONO8 = range(3)   # sf_image_format: the camera's images (cv_bridge encodings)
GRAY_RULE_OPENCV3, GRAY_RULE_OPENCV4 = 0, 1               # sf_image_set_gray_rule
# (kr, kg, kb, shift) of gray = (R kr + G kg + B kb + (1 << (shift - 1))) >> shift
GRAY_RULES = {GRAY_RULE_OPENCV3: (4899, 9617, 1868, 14), GRAY_RULE_OPENCV4: (9798, 19235, 3735, 15)}


class CameraInfo(C.Structure):
    """sf_camera_info (include/sepfinder.h): a sensor_msgs/CameraInfo-shaped block, what sf_rectify_plan_create takes."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("out_width", C.c_int32), ("out_height", C.c_int32),
        ("model", C.c_int32), ("reserved", C.c_int32),
        ("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 12),
    ]


assert C.sizeof(CameraInfo) == 328
SF_MAX_RECTIFY_PLANS = 64
DISTORTION_PLUMB_BOB, DISTORTION_RATIONAL_POLYNOMIAL = 0, 1


def camera_info(width, height, K, D=(), R=None, P=None, model=DISTORTION_PLUMB_BOB, out_width=0, out_height=0):
    """K [3, 3], D up to 8 values (k1 k2 p1 p2 k3 k4 k5 k6), R [3, 3] (None: identity), P [3, 4] (None: [K | 0])."""
    m = CameraInfo()
    m.width, m.height, m.out_width, m.out_height, m.model, m.reserved = int(width), int(height), int(out_width), int(out_height), int(model), 0
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    P = np.hstack([K, np.zeros((3, 1))]) if P is None else np.asarray(P, np.float64).reshape(3, 4)
    d = np.zeros(8, np.float64)
    d[:len(D)] = np.asarray(D, np.float64)
    m.K[:], m.D[:], m.R[:], m.P[:] = K.ravel().tolist(), d.tolist(), R.ravel().tolist(), P.ravel().tolist()
    return m


class NetvladWeights(C.Structure):
    """sf_netvlad_weights (include/sepfinder.h): host pointers to the NetVLAD network's weights, TensorFlow layouts."""
    _fields_ = [
        ("conv_kernel", C.c_void_p * 13), ("conv_bias", C.c_void_p * 13),
        ("average_rgb", C.c_void_p), ("assignment", C.c_void_p), ("cluster_centers", C.c_void_p),
        ("wpca_kernel", C.c_void_p), ("wpca_bias", C.c_void_p),
        ("clusters", C.c_int32), ("pca_dim", C.c_int32),
    ]


VGG16_CONVS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
               (512, 512), (512, 512), (512, 512), (512, 512)]          # (Cin, Cout) of conv1_1 ... conv5_3


class Features(C.Structure):
    _fields_ = [
        ("desc", C.c_void_p),
        ("rows", C.c_uint16),
        ("cols", C.c_uint16),
        ("xyz", C.c_void_p),
        ("n3d", C.c_int32),
        ("kpts", C.c_void_p),
        ("nkp", C.c_int32),
    ]


class Result(C.Structure):
    _fields_ = [
        ("position", C.c_double * 3),
        ("orientation", C.c_double * 4),
        ("covariance", C.c_double * 36),
        ("inliers", C.c_int32),
        ("matches", C.c_int32),
        ("inliers_pass1", C.c_int32),
        ("matches_pass1", C.c_int32),
        ("success", C.c_uint8),
        ("pass1_success", C.c_uint8),
        ("pass2_guided", C.c_uint8),
        ("pad", C.c_uint8 * 5),
    ]


RESULT_DTYPE = np.dtype(
    [("position", "<f8", (3,)), ("orientation", "<f8", (4,)), ("covariance", "<f8", (36,)),
     ("inliers", "<i4"), ("matches", "<i4"), ("inliers_pass1", "<i4"), ("matches_pass1", "<i4"),
     ("success", "u1"), ("pass1_success", "u1"), ("pass2_guided", "u1"), ("pad", "u1", (5,))]
)
assert RESULT_DTYPE.itemsize == C.sizeof(Result) == 368


class Separator(C.Structure):
    _fields_ = [
        ("robot_from_id", C.c_int8),
        ("robot_to_id", C.c_int8),
        ("kf_id_from", C.c_int16),
        ("kf_id_to", C.c_int16),
        ("frame_id_from", C.c_int16),
        ("frame_id_to", C.c_int16),
        ("transform_est_success", C.c_uint8),
        ("pad", C.c_uint8 * 5),
        ("position", C.c_double * 3),
        ("orientation", C.c_double * 4),
        ("covariance", C.c_double * 36),
    ]


SEPARATOR_DTYPE = np.dtype(
    [("robot_from_id", "i1"), ("robot_to_id", "i1"), ("kf_id_from", "<i2"), ("kf_id_to", "<i2"),
     ("frame_id_from", "<i2"), ("frame_id_to", "<i2"), ("transform_est_success", "u1"),
     ("pad", "u1", (5,)), ("position", "<f8", (3,)), ("orientation", "<f8", (4,)),
     ("covariance", "<f8", (36,))]
)
assert SEPARATOR_DTYPE.itemsize == C.sizeof(Separator) == 360


class Match(C.Structure):
    _fields_ = [("idx_local", C.c_int32), ("idx_other", C.c_int32), ("distance", C.c_double)]


MATCH_DTYPE = np.dtype([("idx_local", "<i4"), ("idx_other", "<i4"), ("distance", "<f8")])
assert MATCH_DTYPE.itemsize == C.sizeof(Match) == 16


class StepResult(C.Structure):
    """sf_step_result (include/sepfinder.h): what sf_step_retire hands back; the pointers belong to the handle."""
    _fields_ = [("matches", C.c_void_p), ("record_of_match", C.c_void_p), ("records", C.c_void_p),
                ("n_matches", C.c_int32), ("n_records", C.c_int32), ("n_accepted", C.c_int32), ("streamed", C.c_int32),
                ("d_records", C.c_void_p)]


SF_ABI_VERSION = 8      # include/sepfinder.h
# the four counts of sf_debug_live_resources (include/sf_experimental.h), in its order
LIVE_RESOURCES = ("device_blocks", "device_bytes", "pinned_blocks", "events")

# store slots as one block of bytes (sf_store_export_* / sf_store_import_keyframes_device): [header][entry x n][blocks]
SF_KFBLOB_MAGIC = 0x424B4653      # "SFKB"
SF_KFBLOB_VERSION = 1
WIRE_EXPORT_OVERFLOW, WIRE_BAD_HEADER, WIRE_BAD_ENTRY = 1, 2, 4      # bits of sf_store_wire_status' first word


class KfBlobHeader(C.LittleEndianStructure):
    """sf_kfblob_header (include/sepfinder.h)."""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint16), ("desc_type", C.c_uint8), ("reserved", C.c_uint8),
                ("n_keyframes", C.c_int32), ("max_rows", C.c_int32), ("total_bytes", C.c_uint64), ("reserved2", C.c_uint64)]


class KfBlobEntry(C.LittleEndianStructure):
    """sf_kfblob_entry (include/sepfinder.h): one keyframe of the table behind the header."""
    _fields_ = [("rows", C.c_int32), ("n3d", C.c_int32), ("cols", C.c_int32), ("reserved", C.c_int32),
                ("offset", C.c_uint64), ("bytes", C.c_uint64)]


KFBLOB_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u2"), ("desc_type", "u1"), ("reserved", "u1"),
                                ("n_keyframes", "<i4"), ("max_rows", "<i4"), ("total_bytes", "<u8"), ("reserved2", "<u8")])
KFBLOB_ENTRY_DTYPE = np.dtype([("rows", "<i4"), ("n3d", "<i4"), ("cols", "<i4"), ("reserved", "<i4"), ("offset", "<u8"),
                               ("bytes", "<u8")])
assert KFBLOB_HEADER_DTYPE.itemsize == C.sizeof(KfBlobHeader) == 32
assert KFBLOB_ENTRY_DTYPE.itemsize == C.sizeof(KfBlobEntry) == 32


def default_params() -> Params:
    """Defaults: multi_robot_separators.launch:19-23 for the reference's own knobs; rtabmap
    compiled-in defaults [upstream, SURVEY.md section 9] for the Vis/* values; estimation type
    0 (3D->3D) as BASELINE.json's north_star names.  Mirrors sf_default_params()."""
    p = Params()
    p.netvlad_distance = 0.13
    p.netvlad_dimensions = 128
    p.netvlad_max_matches_nb = 20
    p.nn_precision = 1
    p.min_inliers = 5
    p.inlier_distance = 0.1
    p.iterations = 300
    p.refine_iterations = 5
    p.refine_sigma = 3.0
    p.estimation_type = 0
    p.nndr = 0.6
    p.guess_win_size = 20
    p.ransac_adaptive_stop = 1
    p.max_sample_checks = 1000
    p.seed = 12345
    p.fx = p.fy = 0.0
    p.cx = p.cy = 0.0
    p.image_width = p.image_height = 0
    for i, v in enumerate([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]):
        p.local_transform[i] = float(v)
    p.store_capacity = 1024
    p.max_features = 512
    p.desc_bytes = 32
    p.pnp_reproj_error = 2.0
    p.pnp_flags = 0
    p.pnp_refine_iterations = 0
    p.bundle_adjustment = 0
    p.ba_iterations = 20
    p.ba_robust_kernel_delta = 8.0
    p.ba_pixel_variance = 1.0
    p.stereo_baseline = 0.0
    p.force_3dof = 0
    p.forward_est_only = 1
    p.desc_type = 0
    p.guess_match_to_projection = 0
    return p


def copy_params(p: Params) -> Params:
    q = Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(Params))
    return q


class FeatureArrays:
    """One keyframe's geometric features as numpy arrays, with a ctypes `Features` view that
    borrows them (zero copy, like descriptorsFromROS at MsgConversion.cpp:113-116)."""

    def __init__(self, desc, xyz, kpts):
        desc = np.asarray(desc)
        if desc.dtype == np.float32:       # float32 descriptor rows (sf_params.desc_type 1): handed over as their bytes
            desc = np.ascontiguousarray(desc).view(np.uint8).reshape(desc.shape[0], 4 * desc.shape[1])
        self.desc = np.ascontiguousarray(desc, dtype=np.uint8)
        if self.desc.ndim != 2:
            raise ValueError("desc must be rows x cols uint8 (or rows x dims float32)")
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        kpts = np.asarray(kpts)
        if kpts.dtype != KEYPOINT_DTYPE:
            raise ValueError("kpts must have KEYPOINT_DTYPE")
        self.kpts = np.ascontiguousarray(kpts)

    def c_struct(self) -> Features:
        f = Features()
        f.rows, f.cols = self.desc.shape
        f.desc = self.desc.ctypes.data if self.desc.size else None
        f.n3d = self.xyz.shape[0]
        f.xyz = self.xyz.ctypes.data if self.xyz.size else None
        f.nkp = self.kpts.shape[0]
        f.kpts = self.kpts.ctypes.data if self.kpts.size else None
        return f


def features_array(feats):
    """ctypes array of Features for a list of FeatureArrays (keeps borrowing the numpy data)."""
    arr = (Features * len(feats))()
    for i, f in enumerate(feats):
        arr[i] = f.c_struct()
    return arr
