"""Host: the cells of Vis/GridRows x Vis/GridCols (tests/grid_ref.py, sf_compute_grid) -- the restatement against a table
computed by hand, the library's pure host function against the restatement, and the refusals of both."""
import ctypes as C

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from tests import grid_ref as ref

NO_ROI = (0.0, 0.0, 0.0, 0.0)
GRID_TABLE = [
    # width, height, ratios, rows, cols, max_features -> x, y, col_size, row_size, quota, rows_cap (by hand)
    (752, 480, NO_ROI, 1, 1, 1000, (0, 0, 752, 480, 1000, 1000)),
    (752, 480, NO_ROI, 3, 3, 1000, (0, 0, 250, 160, 112, 1008)),           # 752 = 3 * 250 + 2; 1000 / 9 = 111.1 -> 112
    (752, 480, NO_ROI, 4, 4, 1000, (0, 0, 188, 120, 63, 1008)),            # 62.5 -> 63
    (752, 480, NO_ROI, 2, 2, 1000, (0, 0, 376, 240, 250, 1000)),
    (97, 61, NO_ROI, 2, 3, 300, (0, 0, 32, 30, 50, 300)),                  # remainder: one column (97 - 96), one row (61 - 60)
    (97, 61, NO_ROI, 3, 2, 300, (0, 0, 48, 20, 50, 300)),                  # remainder: one column, one row
    (208, 170, (0.13, 0.2, 0.1, 0.15), 2, 2, 10, (27, 17, 69, 63, 3, 12)),  # ROI (27, 17, 139, 127): odd x, remainders 1 and 1
    (101, 61, (0.01, 0.0, 0.0, 0.0), 2, 4, 100, (1, 0, 25, 30, 13, 104)),  # (int)(101 * 0.01f) = 1: ROI x 1, w 100; 12.5 -> 13
    (752, 480, NO_ROI, 16, 16, 1, (0, 0, 47, 30, 1, 256)),                 # one keypoint per cell: 256 rows for max_features 1
]
EINVAL_CASES = [
    (752, 480, NO_ROI, 0, 1, 1000), (752, 480, NO_ROI, 1, 17, 1000), (752, 480, NO_ROI, -1, 2, 1000), (752, 480, NO_ROI, 17, 0, 1000),
    (752, 480, NO_ROI, 2, 2, 0),                                           # max_features < 1
    (8, 8, NO_ROI, 3, 3, 100), (40, 8, NO_ROI, 3, 1, 100), (8, 40, NO_ROI, 1, 3, 100),   # a cell side of 2
    (752, 480, (1.5, 0.0, 0.0, 0.0), 2, 2, 1000), (5, 5, (0.3, 0.3, 0.3, 0.3), 1, 1, 10),    # what compute_roi refuses
]
ERANGE_CASES = [
    (752, 480, NO_ROI, 2, 2, 32767),                                       # 4 * 8192 = 32768
    (752, 480, NO_ROI, 16, 16, 32767),                                     # 256 * 128 = 32768
]


@pytest.mark.parametrize("w,h,ratios,rows,cols,maxf,want", GRID_TABLE)
def test_compute_grid_table(w, h, ratios, rows, cols, maxf, want):
    assert ref.compute_grid(w, h, ratios, rows, cols, maxf) == want
    boxes, quota = ref.cells(w, h, ratios, rows, cols, maxf)
    assert len(boxes) == rows * cols and quota == want[4] and boxes[0][:2] == want[:2]
    assert boxes[-1] == (want[0] + (cols - 1) * want[2], want[1] + (rows - 1) * want[3], want[2], want[3])   # row-major
    if cols > 1:
        assert boxes[1] == (want[0] + want[2], want[1], want[2], want[3])


def test_compute_grid_limits():
    assert ref.compute_grid(752, 480, NO_ROI, 3, 3, 32760)[4:] == (3640, 32760)       # 9 * 3640: under the limit
    assert ref.compute_grid(9, 9, NO_ROI, 3, 3, 5) == (0, 0, 3, 3, 1, 9)               # a cell side of 3 is the smallest
    for case in EINVAL_CASES:
        with pytest.raises(ValueError):
            ref.compute_grid(*case)
    for case in ERANGE_CASES:
        with pytest.raises(OverflowError):
            ref.compute_grid(*case)


def test_grid_params_layout():
    assert C.sizeof(_abi.GridParams) == 8
    assert _abi.GridParams.grid_rows.offset == 0 and _abi.GridParams.grid_cols.offset == 4
    p = _abi.grid_params()
    assert (p.grid_rows, p.grid_cols) == (1, 1)


def _library(L, w, h, ratios, rows, cols, maxf):
    out = (C.c_int32 * 6)()
    rc = L.sf_compute_grid(w, h, (C.c_float * 4)(*ratios), C.byref(_abi.grid_params(rows, cols)), maxf, out)
    return rc, tuple(out)


def test_library_compute_grid_equals_the_restatement():
    """sf_compute_grid is pure host code: the table, the refusals and 2 000 random cases against compute_grid."""
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    filled = _abi.GridParams(7, 7)
    L.sf_grid_defaults(filled)
    assert bytes(filled) == bytes(_abi.grid_params())
    for w, h, ratios, rows, cols, maxf, want in GRID_TABLE:
        assert _library(L, w, h, ratios, rows, cols, maxf) == (_abi.SF_OK, want)
    for case in EINVAL_CASES:
        assert _library(L, *case)[0] == _abi.SF_EINVAL, case
    for case in ERANGE_CASES:
        assert _library(L, *case)[0] == _abi.SF_ERANGE, case
    out = (C.c_int32 * 6)()                                                  # NULL ratios = no ROI, NULL grid = 1 x 1
    assert L.sf_compute_grid(752, 480, None, None, 1000, out) == _abi.SF_OK and tuple(out) == (0, 0, 752, 480, 1000, 1000)
    assert L.sf_compute_grid(752, 480, None, None, 1000, None) == _abi.SF_EINVAL
    rng = np.random.default_rng(3)
    refused = ranged = 0
    for _ in range(2000):
        r = tuple(float(v) for v in np.round(rng.uniform(0, 0.6, 4), 3) * rng.integers(0, 2, 4))
        case = (int(rng.integers(1, 900)), int(rng.integers(1, 700)), r, int(rng.integers(0, 18)), int(rng.integers(0, 18)),
                int(rng.choice([1, 7, 10, 100, 1000, 5000, 32767, int(rng.integers(1, 32768))])))
        rc, out = _library(L, *case)
        try:
            assert (rc, out) == (_abi.SF_OK, ref.compute_grid(*case)), case
        except ValueError:
            refused += 1
            assert rc == _abi.SF_EINVAL, case
        except OverflowError:
            ranged += 1
            assert rc == _abi.SF_ERANGE, case
    assert 50 < refused < 1500 and ranged > 20
