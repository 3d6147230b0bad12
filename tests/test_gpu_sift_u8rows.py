"""GPU: SIFT (Vis/FeatureType 1) straight into uint8 rows -- a handle with sf_params.desc_type 2 (desc_bytes 128).  A SIFT row
is 128 integers in 0 .. 255; the handle with desc_type 1 / desc_bytes 512 stores them as float32 (tests/test_gpu_sift.py pins
those bytes to the restatement tests/sift_ref.py), this one as bytes.  Every call that makes a keyframe must leave the same
keypoints and 3D points, byte for byte, and the same row values; two such keyframes must verify like their float twins.
One 160 x 120 textured stereo pair (and a second one for the batches): the generator and the size at which
test_gpu_sift.py::test_full_calls_equal_the_explicit_chain asserts more than 50 rows."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from oracle import pyoracle
from tests import extract_cases as ec
from tests.test_gpu_image import MONO8, _weights
from tests.test_gpu_orb2_batch import SENTINEL, pack
from tests.test_gpu_surf import _device_chain, _params, assert_result_parity

pytestmark = pytest.mark.gpu

W, H, DIMS, MAXF = 160, 120, 128, 100


def _finder(u8, estimation_type=0):
    import torch
    p = _params(DIMS, estimation_type=estimation_type, w=W, h=H)
    if u8:
        p.desc_type, p.desc_bytes = 2, DIMS
    p.netvlad_dimensions = 128
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    f.set_feature_type_sift(_abi.sift_params(contrast_threshold=0.02))
    return f


def _cam():
    return _abi.stereo_camera(460.0, 458.0, W / 2.0, H / 2.0, 0.11)


@pytest.fixture(scope="module")
def pairs():
    out = []
    for seed in (700, 701, 700):
        l, r = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(seed, width=W, height=H, max_disp=20.0)[:2])
        l.setflags(write=False); r.setflags(write=False)
        out.append((l, r))
    return out


@pytest.fixture(scope="module")
def float_singles(pairs):
    """get_features_and_descriptor on every pair on the desc_type 1 / 512 handle: computed once, shared, left unchanged."""
    f = _finder(False)
    try:
        out = [f.get_features_and_descriptor(l, r, _cam(), _abi.detector_params(MAXF)) for l, r in pairs]
    finally:
        f.close()
    for s in out:
        assert s[0].shape[1] == 4 * DIMS and len(s[0]) >= 50
        for a in s[:3]:
            a.setflags(write=False)
    return out


def assert_u8_equals_float(got, want, what=""):
    """(rows uint8 [n, 128], xyz, kpts) of the desc_type 2 handle against (rows as bytes of float32 [n, 512], xyz, kpts)."""
    d8, xyz, kp = got
    df = np.asarray(want[0]).view(np.float32).reshape(len(want[0]), DIMS)
    d8 = np.asarray(d8)
    assert d8.dtype == np.uint8 and d8.shape == (len(df), DIMS), (what, d8.shape, df.shape)
    assert kp.tobytes() == want[2].tobytes(), what
    assert np.asarray(xyz).tobytes() == np.asarray(want[1]).tobytes(), what
    assert np.array_equal(d8.astype(np.float32), df), what


def test_single_calls_give_the_float_rows_as_bytes(pairs, float_singles):
    import torch
    (l, r), want = pairs[0], float_singles[0]
    cam, det = _cam(), _abi.detector_params(MAXF)
    f = _finder(True)
    try:
        assert f.get_feature_type()[0] == 1 and f.descriptor_bytes() == DIMS
        a = f.get_features_and_descriptor(l, r, cam, det)
        assert_u8_equals_float(a[:3], want, "sf_get_features_and_descriptor")
        assert 0 < a[0].max() <= 255 and np.isfinite(a[1]).all(axis=1).sum() > 20
        b = f.get_features_and_descriptor_u8(l, r, MONO8, cam, det)
        assert_u8_equals_float(b[:3], want, "sf_get_features_and_descriptor_u8")
        assert (a[3], b[3]) == (0, 1) and f.store_size() == 2
        # sf_extract_keyframe_device on keypoints of the detector (before the stereo step dropped any), on both handles
        d_l =torch.from_numpy(np.array(l)).to("cuda:0")
        d_kp = torch.zeros((MAXF, 28), dtype=torch.uint8, device="cuda:0")
        n = f.detect_sift(d_l.data_ptr(), W, H, W, MAXF, d_kp.data_ptr(), MAXF)
        kp = np.frombuffer(d_kp.cpu().numpy()[:n].tobytes(), dtype=_abi.KEYPOINT_DTYPE)
        assert n >= 50
        got, _ = _device_chain(f, torch, l, r, cam, kp)
        g = _finder(False)
        try:
            ref, _ = _device_chain(g, torch, l, r, cam, kp)
        finally:
            g.close()
        assert len(ref[0]) >= 50
        assert_u8_equals_float(got, ref, "sf_extract_keyframe_device")
    finally:
        f.close()


def test_batch_calls_give_each_keyframe_the_single_calls_bytes(pairs, float_singles):
    import torch
    dev = torch.device("cuda:0")
    cam, det = _cam(), _abi.detector_params(MAXF)
    n, ksz = len(pairs), _abi.KEYPOINT_DTYPE.itemsize
    pitch, stride = W + 13, (W + 13) * H + 72
    L = pack(torch, [p[0] for p in pairs], W, H, pitch, stride)
    R = pack(torch, [p[1] for p in pairs], W, H, pitch, stride)
    f = _finder(True)
    try:
        f.netvlad_load(_weights())
        f.debug_sift_batch_chunk(2)                                            # two chunks: 2 images, then 1
        singles = [f.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
        for s, w in zip(singles, float_singles):
            assert_u8_equals_float(s[:3], w, "single")
        for name in ("get_features_and_descriptor_sift_batch_device", "add_keyframes_sift_u8_batch_device"):
            rows = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
            desc = torch.full((n * MAXF + 1, DIMS), SENTINEL, dtype=torch.uint8, device=dev)
            xyz = torch.full((n * MAXF + 1, 12), SENTINEL, dtype=torch.uint8, device=dev)
            kp = torch.full((n * MAXF + 1, ksz), SENTINEL, dtype=torch.uint8, device=dev)
            before = f.store_size()
            if name.startswith("get"):
                first = f.get_features_and_descriptor_sift_batch_device(L.data_ptr(), R.data_ptr(), n, W, H, pitch, stride, cam, det,
                                                                        None, rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(),
                                                                        kp.data_ptr())
            else:
                first, _ = f.add_keyframes_sift_u8_batch_device(L.data_ptr(), R.data_ptr(), None, MONO8, n, W, H, pitch, stride, cam,
                                                                det, None, rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(),
                                                                kp.data_ptr())
            torch.cuda.synchronize()
            assert first == before and f.store_size() == before + n and f.sift_batch_status() == 0
            h_rows, h_desc, h_xyz, h_kp = (t.cpu().numpy() for t in (rows, desc, xyz, kp))
            assert h_rows[n] == -7 and (h_desc[n * MAXF:] == SENTINEL).all()
            for i, s in enumerate(singles):
                r = int(h_rows[i])
                assert r == len(s[0]), (name, i)
                blk = slice(i * MAXF, i * MAXF + r)
                assert h_desc[blk].tobytes() == s[0].tobytes(), (name, i)
                assert h_xyz[blk].tobytes() == s[1].tobytes() and h_kp[blk].tobytes() == s[2].tobytes(), (name, i)
                assert (h_desc[i * MAXF + r:(i + 1) * MAXF] == SENTINEL).all(), (name, i)
            # ... and the slots hold them: every keyframe against its single call's slot, like that slot against itself
            own = [s[3] for s in singles]
            assert f.verify_pairs(own, list(range(first, first + n))).tobytes() == f.verify_pairs(own, own).tobytes()
    finally:
        f.close()


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_equals_the_float_twin_and_the_oracle(estimation_type):
    """Two views of one scene (a stereo pair and its copy shifted by 8 pixels): verify_pairs on the uint8 rows gives the
    records of the desc_type 1 handle on the same keyframes byte for byte, and they agree with the oracle asked with
    desc_type 1 on the float twin of the rows; a keyframe against itself succeeds."""
    wide_l, wide_r, _ = ec.make_stereo_pair(700, width=W + 8, height=H, max_disp=20.0)
    views = [(np.ascontiguousarray(wide_l[:, o:o + W]), np.ascontiguousarray(wide_r[:, o:o + W])) for o in (0, 8)]
    cam, det = _cam(), _abi.detector_params(MAXF)
    records, frames = {}, {}
    for u8 in (True, False):
        f = _finder(u8, estimation_type)
        try:
            frames[u8] = [f.get_features_and_descriptor(*views[k], cam, det) for k in (0, 1, 0)]
            slots = [s[3] for s in frames[u8]]
            fr, to = [slots[0], slots[0], slots[1]], [slots[2], slots[1], slots[2]]
            records[u8] = f.verify_pairs(fr, to)
            params = f.params
        finally:
            f.close()
    for s8, sf in zip(frames[True], frames[False]):
        assert_u8_equals_float(s8[:3], sf)
        assert len(s8[0]) >= 50
    assert records[True].tobytes() == records[False].tobytes()
    twin = [_abi.FeatureArrays(s[0].astype(np.float32), s[1], s[2]) for s in frames[True]]
    for j, (x, y) in enumerate(((0, 2), (0, 1), (1, 2))):
        o = pyoracle.estimate_transform(params, twin[x], twin[y])               # (params: the desc_type 1 handle's)
        g = records[True][j]
        print("pair %d: success gpu %d oracle %d, inliers %d / %d, matches %d / %d, bytes equal %s" % (
            j, g["success"], o["success"], g["inliers"], o["inliers"], g["matches"], o["matches"], g.tobytes() == o.tobytes()))
        assert_result_parity(g, o, "pair %d" % j)
        assert g.tobytes() == o.tobytes(), j
    assert records[True][0]["success"] == 1 and records[True][0]["inliers"] > 20


def test_roi_grid_and_the_other_families_are_refused(pairs):
    l, r = pairs[0]
    cam = _cam()
    f = _finder(True)
    try:
        state = lambda: (f.get_feature_type()[0], bytes(f.get_sift_params()), f.store_size())   # noqa: E731
        before = state()
        f.front_set_params(_abi.front_params((0.1, 0.0, 0.0, 0.0), 3, 0, 0.02))
        with pytest.raises(lib.SepfinderError) as e:
            f.get_features_and_descriptor(l, r, cam)
        assert e.value.code == _abi.SF_EINVAL and "RoiRatios" in str(e.value) and state() == before
        f.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), 3, 0, 0.02))
        f.grid_set_params(_abi.grid_params(2, 2))
        with pytest.raises(lib.SepfinderError) as e:
            f.get_features_and_descriptor(l, r, cam)
        assert e.value.code == _abi.SF_EINVAL and "Grid" in str(e.value) and state() == before
        f.grid_set_params(_abi.grid_params(1, 1))
        for call in (f.get_features_and_descriptor_batch_device, f.get_features_and_descriptor_orb_batch_device,
                     f.get_features_and_descriptor_surf_batch_device):
            with pytest.raises(lib.SepfinderError) as e:
                call(None, None, 0, W, H, W, W * H, cam)
            assert e.value.code == _abi.SF_EINVAL and "not built" in str(e.value) and state() == before
        for call in (f.add_keyframes_u8_batch_device, f.add_keyframes_orb_u8_batch_device, f.add_keyframes_surf_u8_batch_device):
            with pytest.raises(lib.SepfinderError) as e:
                call(None, None, None, MONO8, 0, W, H, W, W * H, cam)
            assert e.value.code == _abi.SF_EINVAL and "not built" in str(e.value) and state() == before
        for ft in (4, 6, 8):                                                     # the binary types stay refused on this handle
            with pytest.raises(lib.SepfinderError) as e:
                f.set_feature_type(ft)
            assert e.value.code == _abi.SF_EINVAL and state() == before
        with pytest.raises(lib.SepfinderError) as e:
            f.set_feature_type_surf(_abi.surf_params(extended=1))                # float rows: not on this handle
        assert e.value.code == _abi.SF_EINVAL and state() == before
        assert len(f.get_features_and_descriptor(l, r, cam, _abi.detector_params(MAXF))[0]) >= 50      # and it still works
    finally:
        f.close()
