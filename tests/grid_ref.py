"""NumPy restatement of the cell loop of rtabmap's Feature2D::generateKeypoints, Vis/GridRows x Vis/GridCols (rtabmap 0.19 /
0.20, restated from memory: neither rtabmap nor OpenCV is in the reference tree; DESIGN.md section 3 item 17f lists what
this decides).  It is the specification of what the extraction calls do under a grid:

    (X, Y, W, H) = computeRoi(image, Vis/RoiRatios)
    row_size = H / R;  col_size = W / C             integer division: the W % C right-most columns and the H % R bottom
                                                    rows of the ROI are seen by no cell
    quota    = ceil((float)max_features / (float)(R * C))
    for i in 0 .. R-1, for j in 0 .. C-1:           row-major
        cell = a COPY of image[Y + i row_size : +row_size, X + j col_size : +col_size]
        kpts = detector(cell) limited to quota;  kpts += the cell's origin;  append

The detector of a cell is the restatement an existing test already pins the product's detector calls to: fast_ref.detect
(type 4, limitKeypoints = its max_features) or the oracle's detect_corners (types 6 and 8) with max_corners = quota -- the
cell's strongest corners against the cell's own quality_level x max, the cell edge reflecting.  That is the listed
deviation from upstream, which runs GFTT with the whole Vis/MaxFeatures per cell and lets limitKeypoints keep the LAST
quota of a list of zero responses.  Nothing is truncated behind the loop: a keyframe can hold R C quota keypoints."""
import numpy as np

from multi_robot_slam_separators_amd import _abi
from tests import fast_ref

compute_grid = _abi.compute_grid          # (x, y, col_size, row_size, quota, rows_cap); ValueError / OverflowError


def cells(width, height, roi_ratios, grid_rows, grid_cols, max_features):
    """The cells in the loop's order: [(x, y, col_size, row_size)], and the quota."""
    x, y, cw, ch, quota, _ = compute_grid(width, height, roi_ratios, grid_rows, grid_cols, max_features)
    return [(x + j * cw, y + i * ch, cw, ch) for i in range(grid_rows) for j in range(grid_cols)], quota


def generate_keypoints(image, feature_type, max_features, grid_rows=1, grid_cols=1, roi_ratios=(0.0, 0.0, 0.0, 0.0),
                       quality_level=0.001, min_distance=3.0, fast_threshold=20, nonmax_suppression=1):
    """The keypoints of a keyframe before refinement (KEYPOINT_DTYPE, full-image coordinates, cell order) and how many each
    cell gave."""
    img = np.asarray(image)
    h, w = img.shape
    boxes, quota = cells(w, h, roi_ratios, grid_rows, grid_cols, max_features)
    out, counts = [], []
    for x, y, cw, ch in boxes:
        cell = np.ascontiguousarray(img[y:y + ch, x:x + cw]).copy()
        if feature_type == 4:
            kp = fast_ref.detect(cell, fast_threshold, nonmax_suppression, quota)
        elif feature_type in (6, 8):
            from oracle import pyoracle
            kp = pyoracle.detect_corners(cell, quota, quality_level, min_distance)
        else:
            raise ValueError("a grid under Vis/FeatureType %d is not built" % feature_type)
        kp = np.array(kp[:quota], copy=True)
        kp["x"] = kp["x"] + np.float32(x)
        kp["y"] = kp["y"] + np.float32(y)
        out.append(kp)
        counts.append(len(kp))
    return (np.concatenate(out) if out else np.zeros(0, _abi.KEYPOINT_DTYPE)), counts
