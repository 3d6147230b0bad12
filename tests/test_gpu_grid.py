"""GPU: Vis/GridRows x Vis/GridCols, the detector per cell of the ROI (csrc/k_grid.hip, the cell addressing of k_fast.hip and
k_gftt.hip, sf_grid_params) through the C-ABI, byte for byte against the NumPy restatement tests/grid_ref.py: the host
handler and the batch forms under a grid against the chain restatement (grid_ref -> subpix_ref) ->
sf_stereo_correspondences_device -> sf_extract_keyframe_device, calls that existing tests pin.

What a keyframe shows of its detector is what passes the descriptor's border filter: 28 px for BRIEF (types 4 and 6), which
on the 61-row images leaves five rows.  So type 8 runs with ORB/EdgeThreshold 1 here -- nearly every keypoint of every cell
reaches the output -- and the BRIEF types also run on 203 x 171 images whose texture keeps 30 px from the image border, where
every keypoint does."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import grid_ref as ref
from tests import subpix_ref
from tests.test_gpu_image import RGB8, _finder, _weights, colourise
from tests.test_gpu_orb import assert_same
from tests.test_gpu_orb2 import _pair, _params
from tests.test_gpu_orb2_batch import SENTINEL, _cam, _self_pairs, batch_pairs, pack

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
NO_ROI = (0.0, 0.0, 0.0, 0.0)
ROI_RATIOS = (0.13, 0.2, 0.1, 0.15)
REFINE = (3, 5, 0.02)
GAINS = (1.8, 0.8, 1.4, 0.7, 1.1, 0.9)                  # contrast of consecutive cells: very different quality thresholds


@pytest.fixture()
def finder():
    import torch
    f = lib.SeparatorFinder(_params(w=203, h=171), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    yield f
    f.close()


def _set_type(f, ftype):
    if ftype == 2:
        f.set_feature_type_orb()
    elif ftype == 8:
        f.set_feature_type(8, _abi.orb_params(edge_threshold=1))      # (the module docstring)
    else:
        f.set_feature_type(ftype)


def _scaled(image, gain):
    return np.clip(128.0 + (image.astype(np.float64) - 128.0) * gain, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def grid_pair(w, h, rows, cols, ratios=NO_ROI, flat=(), margin=0, seed=1):
    """A stereo pair whose texture has the contrast GAINS[q % 6] in cell q of the grid, cells in `flat` constant; `margin`
    pixels along the image border constant.  Contiguous uint8 [h][w]."""
    boxes, _ = ref.cells(w, h, ratios, rows, cols, 1)
    gain = np.ones((h, w))
    for q, (x, y, cw, ch) in enumerate(boxes):
        gain[y:y + ch, x:x + cw] = 0.0 if q in flat else GAINS[q % len(GAINS)]
    if margin:
        keep = np.zeros((h, w))
        keep[margin:h - margin, margin:w - margin] = 1.0
        gain *= keep
    return tuple(_scaled(np.ascontiguousarray(x), gain) for x in _pair(w, h, seed))


def chain(f, torch, left, right, cam, found, refine=None):
    """The restated keypoints of a keyframe -> cv::cornerSubPix restated on the full image -> the device's stereo
    correspondence and extraction.  Returns (desc, xyz, kpts) and the slot."""
    dev = torch.device("cuda:0")
    h, w = left.shape
    win, it, eps = refine if refine else (0, 0, 0.0)
    kp = subpix_ref.refine_keypoints(left, found, win, it, eps, (0, 0))
    n, nb = len(kp), f.descriptor_bytes()
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_kp = torch.from_numpy(np.frombuffer(kp.tobytes(), np.uint8).copy()).to(dev) if n else torch.zeros((28,), dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((max(n, 1), 2), dtype=torch.float32, device=dev)
    d_rx = torch.zeros((max(n, 1),), dtype=torch.float32, device=dev)
    d_st = torch.zeros((max(n, 1),), dtype=torch.uint8, device=dev)
    f.stereo_correspondences_device(d_l.data_ptr(), d_r.data_ptr(), w, h, w, d_kp.data_ptr(), n, d_xy.data_ptr(), d_st.data_ptr(),
                                    d_rx.data_ptr())
    desc = torch.zeros((max(n, 1), nb), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    kpo = torch.zeros((max(n, 1), 28), dtype=torch.uint8, device=dev)
    slot, rows = f.extract_keyframe_device(d_l.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), n, cam,
                                           desc.data_ptr(), xyz.data_ptr(), kpo.data_ptr())
    torch.cuda.synchronize()
    return (desc.cpu().numpy()[:rows], xyz.cpu().numpy()[:rows], np.frombuffer(kpo.cpu().numpy()[:rows].tobytes(), dtype=KP)), slot


@functools.lru_cache(maxsize=None)
def _found(key, ftype, maxf, rows, cols, ratios):
    """grid_ref's keypoints of grid_pair(*key)'s left image, computed once per case (read-only afterwards)."""
    det = _abi.detector_params(maxf)
    kp, counts = ref.generate_keypoints(grid_pair(*key)[0], ftype, maxf, rows, cols, ratios, det.quality_level, det.min_distance)
    kp.setflags(write=False)
    return kp, tuple(counts)


def cell_of(kp, w, h, rows, cols, ratios, maxf):
    """The cell index of every keypoint (by its integer position before refinement)."""
    x, y, cw, ch, _, _ = ref.compute_grid(w, h, ratios, rows, cols, maxf)
    return ((kp["y"].astype(int) - y) // ch) * cols + (kp["x"].astype(int) - x) // cw


def run_batch(f, torch, pairs, w, h, pitch, stride, cam, det, rows_cap):
    """sf_get_features_and_descriptor_batch_device with sentinel-filled outputs of rows_cap rows per keyframe and one row
    more.  Returns the first slot and, per keyframe, (desc, xyz, kp) cut to its rows."""
    dev = torch.device("cuda:0")
    n = len(pairs)
    L, R = pack(torch, [p[0] for p in pairs], w, h, pitch, stride), pack(torch, [p[1] for p in pairs], w, h, pitch, stride)
    rows = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    desc = torch.full((n * rows_cap + 1, 32), SENTINEL, dtype=torch.uint8, device=dev)
    xyz = torch.full((n * rows_cap + 1, 12), SENTINEL, dtype=torch.uint8, device=dev)
    kp = torch.full((n * rows_cap + 1, 28), SENTINEL, dtype=torch.uint8, device=dev)
    first = f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n, w, h, pitch, stride, cam, det, None,
                                                       rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
    torch.cuda.synchronize()
    rows, desc, xyz, kp = (t.cpu().numpy() for t in (rows, desc, xyz, kp))
    assert rows[n] == -7
    out = []
    for i in range(n):
        r = int(rows[i])
        assert 0 <= r <= rows_cap
        blk = slice(i * rows_cap, (i + 1) * rows_cap)
        for a in (desc[blk], xyz[blk], kp[blk]):
            assert (a[r:] == SENTINEL).all(), "keyframe %d: written past its %d rows" % (i, r)
        out.append((desc[blk][:r].copy(), np.frombuffer(xyz[blk][:r].tobytes(), np.float32).reshape(r, 3),
                    np.frombuffer(kp[blk][:r].tobytes(), dtype=KP)))
    assert (desc[n * rows_cap:] == SENTINEL).all() and (xyz[n * rows_cap:] == SENTINEL).all() and (kp[n * rows_cap:] == SENTINEL).all()
    return first, out


# name: (w, h, rows, cols, ratios, max_features, margin)
SHAPES = {
    "97x61 2x3": (97, 61, 2, 3, NO_ROI, 60, 0),                    # cells 32 x 30: a remainder column and row
    "97x61 3x2": (97, 61, 3, 2, NO_ROI, 60, 0),                    # cells 48 x 20
    "101x61 2x4 roi x 1": (101, 61, 2, 4, (0.01, 0.0, 0.0, 0.0), 80, 0),   # cells 25 x 30 from x = 1: bases 1, 26, 51, 76 --
                                                                   # the byte path beside the dword path in one launch
    "203x171 3x2 inner": (203, 171, 3, 2, NO_ROI, 90, 30),         # every keypoint passes BRIEF's border; > 1 block per cell
    "203x171 9x9": (203, 171, 9, 9, NO_ROI, 400, 0),               # 81 cells: two passes of the gather's scan
    "203x171 16x16": (203, 171, 16, 16, NO_ROI, 512, 0),           # 256 cells of 12 x 10, two keypoints apiece: four passes
}


@pytest.mark.parametrize("ftype", [4, 6, 8])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_grid_equals_restatement(finder, shape, ftype):
    import torch
    w, h, rows, cols, ratios, maxf, margin = SHAPES[shape]
    key = (w, h, rows, cols, ratios, (), margin)
    left, right = grid_pair(*key)
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    found, counts = _found(key, ftype, maxf, rows, cols, ratios)
    x0, y0, cw, ch, quota, rows_cap = ref.compute_grid(w, h, ratios, rows, cols, maxf)
    print("%s type %d: cells of %d x %d from (%d, %d), quota %d; the restatement finds %s" % (shape, ftype, cw, ch, x0, y0, quota, list(counts)))
    # on the restatement alone: corners in every cell, some cells at their quota and some below it
    assert max(counts) == quota
    if rows * cols <= 8 or ftype != 4:
        assert min(counts) > 0
    else:                                                        # (FAST sees 16 x 13 pixels of a 22 x 19 cell, 6 x 4 of a 12 x 10 one)
        assert sum(c > 0 for c in counts) >= (rows * cols // 2 if rows == 9 else 20)
    assert (np.diff(cell_of(found, w, h, rows, cols, ratios, maxf)) >= 0).all()      # cell order
    if shape.startswith("101"):
        assert x0 == 1 and cw % 4 == 1 and {(x0 + j * cw) % 4 for j in range(cols)} == {0, 1, 2, 3}
    _set_type(finder, ftype)
    want, _ = chain(finder, torch, left, right, cam, found)
    if ratios != NO_ROI:
        finder.front_set_params(_abi.front_params(ratios))
    finder.grid_set_params(_abi.grid_params(rows, cols))
    assert finder.compute_grid(w, h, ratios, rows, cols, maxf) == (x0, y0, cw, ch, quota, rows_cap)
    d, p, k, slot = finder.get_features_and_descriptor(left, right, cam, det)
    shown = np.unique(cell_of(k, w, h, rows, cols, ratios, maxf))
    print("  %d of %d keypoints reach the output, from %d of %d cells" % (len(k), len(found), len(shown), rows * cols))
    assert_same((d, p, k), want)
    assert finder.store_size() == slot + 1
    if ftype == 8 or margin:
        assert len(shown) == rows * cols and len(k) >= len(found) - (0 if margin else len(found) // 4)
    first, got = run_batch(finder, torch, [(left, right)] * 2, w, h, w + 5, (w + 5) * h + 19, cam, det, rows_cap)
    assert first == slot + 1
    for g in got:                                                # (an odd pitch: the cells' alignment differs from the single call's)
        assert_same(g, (d, p, k))


@pytest.mark.parametrize("ftype", [4, 6, 8])
def test_quota_and_order(finder, ftype):
    """max_features 10 at 2 x 2: quota 3, a keyframe of 12 rows -- more than max_features."""
    import torch
    w, h, rows, cols, maxf = 203, 171, 2, 2, 10
    key = (w, h, rows, cols, NO_ROI, (), 30)
    left, right = grid_pair(*key)
    found, counts = _found(key, ftype, maxf, rows, cols, NO_ROI)
    assert counts == (3, 3, 3, 3) and ref.compute_grid(w, h, NO_ROI, rows, cols, maxf)[4:] == (3, 12)
    _set_type(finder, ftype)
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    want, _ = chain(finder, torch, left, right, cam, found)
    finder.grid_set_params(_abi.grid_params(rows, cols))
    d, p, k, _ = finder.get_features_and_descriptor(left, right, cam, det)
    assert_same((d, p, k), want)
    assert len(k) == 12 and cell_of(k, w, h, rows, cols, NO_ROI, maxf).tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert np.array_equal(k["x"], found["x"]) and np.array_equal(k["y"], found["y"])          # the order inside a cell: the detector's
    if ftype == 4:                                               # limitKeypoints cut every cell: descending response
        assert all((np.diff(k["response"][q * 3:q * 3 + 3]) <= 0).all() for q in range(4)) and (k["response"] > 0).all()
    # cap_rows works as before: the first cap_rows rows, the count of all
    L = lib.load()
    import ctypes as C
    kp = np.zeros(5, KP)
    n, slot = C.c_int32(), C.c_int32()
    l2, r2 = np.ascontiguousarray(left), np.ascontiguousarray(right)
    assert L.sf_get_features_and_descriptor(finder._h, C.c_void_p(l2.ctypes.data), C.c_void_p(r2.ctypes.data), w, h, w, C.byref(cam),
                                            C.byref(det), None, None, None, C.c_void_p(kp.ctypes.data), 5, C.byref(n),
                                            C.byref(slot)) == _abi.SF_OK
    assert n.value == 12 and kp.tobytes() == k[:5].tobytes()


@pytest.mark.parametrize("ftype", [4, 6])
def test_empty_cells(finder, ftype):
    import torch
    w, h, rows, cols, maxf = 203, 171, 2, 3, 12
    key = (w, h, rows, cols, NO_ROI, (1, 3), 30)                  # cells 1 and 3 flat, between cells that fill their quota of 2
    left, right = grid_pair(*key)
    found, counts = _found(key, ftype, maxf, rows, cols, NO_ROI)
    assert counts == (2, 0, 2, 0, 2, 2)
    _set_type(finder, ftype)
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    want, _ = chain(finder, torch, left, right, cam, found)
    finder.grid_set_params(_abi.grid_params(rows, cols))
    d, p, k, _ = finder.get_features_and_descriptor(left, right, cam, det)
    assert_same((d, p, k), want)
    assert cell_of(k, w, h, rows, cols, NO_ROI, maxf).tolist() == [0, 0, 2, 2, 4, 4, 5, 5]
    # every cell empty: no rows, no error, a (empty) keyframe in the store
    flat = np.full((h, w), 93, np.uint8)
    size = finder.store_size()
    d, p, k, slot = finder.get_features_and_descriptor(flat, flat, cam, det)
    assert len(d) == len(p) == len(k) == 0 and slot == size and finder.store_size() == size + 1
    first, got = run_batch(finder, torch, [(flat, flat), (left, right), (flat, flat)], w, h, w, w * h, cam, det, 12)
    assert [len(g[0]) for g in got] == [0, 8, 0]
    assert_same(got[1], want)


def test_small_cells(finder):
    """FAST cells below 7 x 7 give no corners and no error (56 cells of 6 x 6, 256 cells of 3 x 3: the smallest accepted)."""
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 256, size=(48, 48), dtype=np.uint8)
    cam = _cam(48, 48)
    finder.set_feature_type(4)
    for rows, cols in ((8, 7), (16, 16)):                          # cells 6 x 6 and 3 x 3
        finder.grid_set_params(_abi.grid_params(rows, cols))
        det = _abi.detector_params(rows * cols * 2)
        size = finder.store_size()
        d, p, k, slot = finder.get_features_and_descriptor(noise, noise, cam, det)
        assert len(k) == 0 and slot == size
        assert ref.generate_keypoints(noise, 4, det.max_features, rows, cols)[1] == [0] * (rows * cols)


@pytest.mark.parametrize("ftype", [4, 6, 8])
def test_grid_with_roi_and_refinement(finder, ftype):
    import torch
    w, h, rows, cols, maxf = 208, 170, 2, 3, 120
    roi = ref.compute_grid(w, h, ROI_RATIOS, rows, cols, maxf)
    assert roi == (27, 17, 46, 63, 20, 120)                        # ROI (27, 17, 139, 127): an odd x; cells of 46 x 63
    key = (w, h, rows, cols, ROI_RATIOS, (), 0)
    left, right = grid_pair(*key)
    found, counts = _found(key, ftype, maxf, rows, cols, ROI_RATIOS)
    assert min(counts) > 0
    assert ((found["x"] >= 27) & (found["x"] < 27 + 3 * 46) & (found["y"] >= 17) & (found["y"] < 17 + 2 * 63)).all()
    _set_type(finder, ftype)
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    want, _ = chain(finder, torch, left, right, cam, found, REFINE)
    plain, _ = chain(finder, torch, left, right, cam, found)
    finder.front_set_params(_abi.front_params(ROI_RATIOS, *REFINE))
    finder.grid_set_params(_abi.grid_params(rows, cols))
    single = finder.get_features_and_descriptor(left, right, cam, det)
    k = single[2]
    frac = (k["x"] != np.floor(k["x"])) | (k["y"] != np.floor(k["y"]))
    print("type %d, ROI and refinement under a grid: restatement %s, %d rows, %d fractional" % (ftype, list(counts), len(k), frac.sum()))
    assert_same(single[:3], want)
    assert len(k) > 20 and frac.sum() * 4 >= len(k) and k.tobytes() != plain[2].tobytes()
    first, got = run_batch(finder, torch, [(left, right)] * 2, w, h, w, w * h, cam, det, 120)
    for g in got:
        assert_same(g, single[:3])
    # the ROI alone under a grid: the gather shifts, nothing refines
    finder.front_set_params(_abi.front_params(ROI_RATIOS))
    assert_same(finder.get_features_and_descriptor(left, right, cam, det)[:3], plain)


def _three_pairs(w, h):
    p = batch_pairs(w, h)
    return [p[0], p[1], p[3]]          # texture everywhere; the right two thirds flat; flat but for one 48 x 48 patch


@pytest.mark.parametrize("ftype", [4, 6, 8])
def test_batch_of_three_images(finder, ftype):
    import torch
    w, h, rows, cols, maxf = 203, 171, 3, 3, 200
    x0, y0, cw, ch, quota, rows_cap = ref.compute_grid(w, h, NO_ROI, rows, cols, maxf)
    assert (quota, rows_cap) == (23, 207)                          # the stride of the outputs: 207 rows, not 200
    pairs = _three_pairs(w, h)
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    _set_type(finder, ftype)
    wants = []
    for l, r in pairs:
        found, counts = ref.generate_keypoints(l, ftype, maxf, rows, cols, NO_ROI, det.quality_level, det.min_distance)
        wants.append((chain(finder, torch, l, r, cam, found)[0], counts))
    assert min(wants[0][1]) > 0 and 0 in wants[1][1] and max(wants[1][1]) > 0 and 0 in wants[2][1] and max(wants[2][1]) > 0
    finder.grid_set_params(_abi.grid_params(rows, cols))
    singles = [finder.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
    for s, (wnt, _) in zip(singles, wants):
        assert_same(s[:3], wnt)
    assert len(singles[0][0]) > 30
    before = finder.store_size()
    first, got = run_batch(finder, torch, pairs, w, h, w + 6, (w + 6) * h + 32, cam, det, rows_cap)
    assert first == before and finder.store_size() == before + 3
    for g, s in zip(got, singles):
        assert_same(g, s[:3])
    assert _self_pairs(finder, range(first, first + 3)) == _self_pairs(finder, [s[3] for s in singles])   # the store's rows
    # the camera-image form of the single call: mono8 is the plain call
    u8 = finder.get_features_and_descriptor_u8(pairs[0][0], pairs[0][1], _abi.SF_IMAGE_MONO8, cam, det)
    assert_same(u8[:3], singles[0][:3])


def test_u8_batch_under_a_grid():
    import torch
    dev = torch.device("cuda:0")
    w, h, rows, cols, maxf = 203, 171, 3, 3, 200
    rows_cap = ref.compute_grid(w, h, NO_ROI, rows, cols, maxf)[5]
    cam, det = _cam(w, h), _abi.detector_params(maxf)
    pairs = [(colourise(l, 10 + i, RGB8), colourise(r, 20 + i, RGB8)) for i, (l, r) in enumerate(_three_pairs(w, h))]
    pitch, stride = 3 * w + 5, (3 * w + 5) * h + 64

    def packed(images):
        buf = np.full((len(images), stride), 0xA5, np.uint8)
        for i, c in enumerate(images):
            np.lib.stride_tricks.as_strided(buf[i], shape=(h, w, 3), strides=(pitch, 3, 1))[...] = c
        return torch.from_numpy(buf).to(dev)

    d_l, d_r = packed([p[0] for p in pairs]), packed([p[1] for p in pairs])
    f = _finder(torch, w=w, h=h, dims=128)
    try:
        f.netvlad_load(_weights())
        plain = f.get_features_and_descriptor_u8(*pairs[0], RGB8, cam, det)
        f.grid_set_params(_abi.grid_params(rows, cols))
        singles = [f.get_features_and_descriptor_u8(l, r, RGB8, cam, det) for l, r in pairs]
        assert len(singles[0][0]) > 30 and singles[0][2].tobytes() != plain[2].tobytes()
        size = f.store_size()
        n_rows = torch.full((3,), -7, dtype=torch.int32, device=dev)
        desc = torch.full((3 * rows_cap, 32), SENTINEL, dtype=torch.uint8, device=dev)
        xyz = torch.full((3 * rows_cap, 12), SENTINEL, dtype=torch.uint8, device=dev)
        kp = torch.full((3 * rows_cap, 28), SENTINEL, dtype=torch.uint8, device=dev)
        first, row = f.add_keyframes_u8_batch_device(d_l.data_ptr(), d_r.data_ptr(), None, RGB8, 3, w, h, pitch, stride, cam, det,
                                                     None, n_rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
        torch.cuda.synchronize()
        assert (first, row) == (size, 0) and f.store_size() == size + 3 and f.nn_sizes() == (3, 0)
        n_rows, desc, xyz, kp = (t.cpu().numpy() for t in (n_rows, desc, xyz, kp))
        for i, (d0, p0, k0, _) in enumerate(singles):
            r = int(n_rows[i])
            blk = slice(i * rows_cap, i * rows_cap + r)
            assert r == len(d0), i
            assert_same((desc[blk], np.frombuffer(xyz[blk].tobytes(), np.float32).reshape(r, 3),
                         np.frombuffer(kp[blk].tobytes(), dtype=KP)), (d0, p0, k0))
            assert (kp[i * rows_cap + r:(i + 1) * rows_cap] == SENTINEL).all()
        assert _self_pairs(f, range(first, first + 3)) == _self_pairs(f, [s[3] for s in singles])
    finally:
        f.close()


@pytest.mark.parametrize("ftype", [4, 6, 8, 2])
def test_one_by_one_is_a_fresh_handle(finder, ftype):
    import torch
    w, h = 203, 171
    pairs = _three_pairs(w, h)
    cam, det = _cam(w, h), _abi.detector_params(150)
    if ftype == 2:
        finder.set_feature_type_orb()
    else:
        finder.set_feature_type(ftype)
    filled = _abi.GridParams(5, 5)
    lib.load().sf_grid_defaults(filled)
    assert bytes(filled) == bytes(_abi.grid_params()) == bytes(finder.grid_get_params())
    from tests.test_gpu_orb2_batch import run_batch as run_batch_plain
    call = finder.get_features_and_descriptor_orb_batch_device if ftype == 2 else finder.get_features_and_descriptor_batch_device
    fresh = [finder.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
    _, fresh_batch = run_batch_plain(finder, torch, pairs, w, h, w + 6, (w + 6) * h + 32, cam, det, call=call)
    finder.grid_set_params(_abi.grid_params(2, 2))
    finder.grid_set_params(_abi.grid_params(1, 1))
    again = [finder.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
    _, again_batch = run_batch_plain(finder, torch, pairs, w, h, w + 6, (w + 6) * h + 32, cam, det, call=call)
    assert len(fresh[0][0]) > 30
    for a, b in zip(fresh, again):
        assert_same(b[:3], a[:3])
    for a, b in zip(fresh_batch, again_batch):
        assert_same(b, a)


def test_refusals(finder):
    import torch
    w, h = 203, 171
    cam, det = _cam(w, h), _abi.detector_params(200)
    left, right = batch_pairs(w, h)[0]
    d_l, d_r = torch.from_numpy(left).to("cuda:0"), torch.from_numpy(right).to("cuda:0")
    state = lambda f: (f.store_size(), f.nn_sizes(), bytes(f.grid_get_params()), f.get_feature_type()[0])  # noqa: E731
    # the setter
    good = _abi.grid_params(3, 2)
    finder.grid_set_params(good)
    for bad in ((0, 1), (1, 0), (17, 1), (1, 17), (-3, 2), (2, 1000)):
        with pytest.raises(lib.SepfinderError) as e:
            finder.grid_set_params(_abi.grid_params(*bad))
        assert e.value.code == _abi.SF_EINVAL and bytes(finder.grid_get_params()) == bytes(good)
    finder.grid_set_params(_abi.grid_params(16, 16))
    assert bytes(finder.grid_get_params()) == bytes(_abi.grid_params(16, 16))
    # type 2 under a grid: the single call, its _u8 form and both _orb_ batch calls
    f2 = _finder(torch, w=w, h=h, dims=128)
    try:
        f2.netvlad_load(_weights())
        f2.set_feature_type_orb()
        f2.grid_set_params(_abi.grid_params(2, 2))                 # accepted: the handle's type may change later
        before = state(f2)
        rgb = torch.from_numpy(np.ascontiguousarray(colourise(left, 3, RGB8))).to("cuda:0")
        calls = (lambda: f2.get_features_and_descriptor(left, right, cam, det),
                 lambda: f2.get_features_and_descriptor_u8(left, right, _abi.SF_IMAGE_MONO8, cam, det),
                 lambda: f2.get_features_and_descriptor_orb_batch_device(d_l.data_ptr(), d_r.data_ptr(), 1, w, h, w, w * h, cam, det),
                 lambda: f2.add_keyframes_u8_batch_device(rgb.data_ptr(), rgb.data_ptr(), None, RGB8, 1, w, h, 3 * w, 3 * w * h, cam, det,
                                                          _call="sf_add_keyframes_orb_u8_batch_device"))
        for call in calls:
            with pytest.raises(lib.SepfinderError) as e:
                call()
            assert e.value.code == _abi.SF_EINVAL and "Grid" in str(e.value) and "not built" in str(e.value)
            assert state(f2) == before
        f2.grid_set_params(_abi.grid_params(1, 1))
        assert len(calls[0]()[0]) > 30                              # 1 x 1: type 2 runs
        # types 4 / 6 on the same handle: cells below 3 px, and more rows than a keyframe may hold
        f2.set_feature_type(6)
        f2.grid_set_params(_abi.grid_params(16, 16))
        before = state(f2)
        tiny = np.ascontiguousarray(left[:40, :47])                 # 47 / 16 = 2
        d_t = torch.from_numpy(tiny).to("cuda:0")
        t_rgb = torch.from_numpy(np.ascontiguousarray(colourise(tiny, 3, RGB8))).to("cuda:0")
        small = (lambda: f2.get_features_and_descriptor(tiny, tiny, _cam(47, 40), det),
                 lambda: f2.get_features_and_descriptor_batch_device(d_t.data_ptr(), d_t.data_ptr(), 1, 47, 40, 47, 47 * 40, _cam(47, 40), det),
                 lambda: f2.add_keyframes_u8_batch_device(t_rgb.data_ptr(), t_rgb.data_ptr(), None, RGB8, 1, 47, 40, 3 * 47, 3 * 47 * 40,
                                                          _cam(47, 40), det))
        for call in small:
            with pytest.raises(lib.SepfinderError) as e:
                call()
            assert e.value.code == _abi.SF_EINVAL and "2 x 2" in str(e.value), str(e.value)
            assert state(f2) == before
        with pytest.raises(lib.SepfinderError) as e:
            f2.compute_grid(47, 40, NO_ROI, 16, 16, 200)
        assert e.value.code == _abi.SF_EINVAL
        f2.grid_set_params(_abi.grid_params(2, 2))
        before = state(f2)
        big = _abi.detector_params(32767)                           # 4 * 8192 = 32768 rows
        many = (lambda: f2.get_features_and_descriptor(left, right, cam, big),
                lambda: f2.get_features_and_descriptor_batch_device(d_l.data_ptr(), d_r.data_ptr(), 1, w, h, w, w * h, cam, big),
                lambda: f2.add_keyframes_u8_batch_device(rgb.data_ptr(), rgb.data_ptr(), None, RGB8, 1, w, h, 3 * w, 3 * w * h, cam, big))
        for call in many:
            with pytest.raises(lib.SepfinderError) as e:
                call()
            assert e.value.code == _abi.SF_ERANGE and "32768" in str(e.value), str(e.value)
            assert state(f2) == before
        assert len(f2.get_features_and_descriptor(left, right, cam, det)[0]) > 30        # the handle still works
    finally:
        f2.close()
