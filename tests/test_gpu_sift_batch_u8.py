"""GPU: sf_add_keyframes_sift_u8_batch_device -- keyframes of Vis/FeatureType 1 from the camera's rgb8 / bgr8 / mono8 images
in one launch sequence.  Slot i holds what sf_get_features_and_descriptor_u8 gives for pair i, local NN row i what
sf_netvlad_infer_u8_batch_device gives for image i, byte for byte; the store and the NN database grow together."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import sift_batch_cases as cases
from tests.test_gpu_image import BGR8, MONO8, RGB8, _weights, colourise
from tests.test_gpu_orb2_batch import SENTINEL
from tests.test_gpu_surf import _params, assert_same

pytestmark = pytest.mark.gpu

W, H, N, DIMS, MAXF = 97, 61, 3, 128, 20


def _finder(torch):
    p = _params(128, w=W, h=H)
    p.netvlad_dimensions = DIMS
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


def _cam():
    return _abi.stereo_camera(460.0, 458.0, W / 2.0, H / 2.0, 0.11)


def _camera_pairs(fmt):
    """The three pairs of "97x61" (A', flat, A') as the camera's images in `fmt`: [h][w][3], or [h][w] for mono8."""
    gray = cases.pairs("97x61")
    assert gray[0][0].shape == (H, W) and len(gray) == N
    if fmt == MONO8:
        return gray
    return [(colourise(l, 10 + i, fmt), colourise(r, 20 + i, fmt)) for i, (l, r) in enumerate(gray)]


def _pack(torch, images, bpp, pitch, stride):
    buf = np.full((len(images), stride), 0xA5, np.uint8)
    for i, c in enumerate(images):
        np.lib.stride_tricks.as_strided(buf[i], shape=(H, W * bpp), strides=(pitch, 1))[...] = np.asarray(c).reshape(H, W * bpp)
    return torch.from_numpy(buf).to(torch.device("cuda:0"))


def _self_pairs(f, slots):
    return f.verify_pairs(list(slots), list(slots)).tobytes()


@pytest.mark.parametrize("fmt,rule", [(RGB8, 0), (BGR8, 1), (MONO8, 0)])
def test_batch_ingestion_equals_single_u8_calls(fmt, rule):
    import torch
    dev = torch.device("cuda:0")
    cases.check_preconditions("97x61")
    cam, det = _cam(), _abi.detector_params(MAXF)
    pairs = _camera_pairs(fmt)
    bpp = 1 if fmt == MONO8 else 3
    pitch = bpp * W + 5
    stride = pitch * H + 64
    d_l = _pack(torch, [p[0] for p in pairs], bpp, pitch, stride)
    d_r = _pack(torch, [p[1] for p in pairs], bpp, pitch, stride)
    f = _finder(torch)
    try:
        f.netvlad_load(_weights())
        f.image_set_gray_rule(rule)
        f.set_feature_type_sift()
        f.debug_sift_batch_chunk(2)                                               # two chunks: 2 images, then 1
        singles = [f.get_features_and_descriptor_u8(l, r, fmt, cam, det) for l, r in pairs]
        assert len(singles[0][0]) > 5 and len(singles[2][0]) > 5                  # not vacuous
        want_nn = torch.zeros((N, DIMS), dtype=torch.float32, device=dev)
        f.netvlad_infer_u8_batch_device(d_l.data_ptr(), fmt, N, W, H, pitch, stride, want_nn.data_ptr(), DIMS)
        f.nn_append_local_device(want_nn.data_ptr(), N, DIMS)                     # rows 0 .. 2: the reference rows
        assert f.store_size() == N and f.nn_sizes() == (N, 0)
        ksz = _abi.KEYPOINT_DTYPE.itemsize
        rows = torch.full((N,), -7, dtype=torch.int32, device=dev)
        desc = torch.full((N * MAXF, 512), SENTINEL, dtype=torch.uint8, device=dev)
        xyz = torch.full((N * MAXF, 12), SENTINEL, dtype=torch.uint8, device=dev)
        kp = torch.full((N * MAXF, ksz), SENTINEL, dtype=torch.uint8, device=dev)
        first, row = f.add_keyframes_sift_u8_batch_device(d_l.data_ptr(), d_r.data_ptr(), None, fmt, N, W, H, pitch, stride, cam,
                                                          det, None, rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(),
                                                          kp.data_ptr())
        torch.cuda.synchronize()
        assert (first, row) == (N, N) and f.store_size() == 2 * N and f.nn_sizes() == (2 * N, 0)   # grown together, by 3
        assert f.sift_batch_status() == 0
        rows, desc, xyz, kp = (t.cpu().numpy() for t in (rows, desc, xyz, kp))
        for i, (d0, p0, k0, _) in enumerate(singles):
            r = int(rows[i])
            blk = slice(i * MAXF, i * MAXF + r)
            assert r == len(d0), i
            assert_same((desc[blk], np.frombuffer(xyz[blk].tobytes(), np.float32).reshape(r, 3),
                         np.frombuffer(kp[blk].tobytes(), dtype=_abi.KEYPOINT_DTYPE)), (d0, p0, k0), 128)
            assert (desc[i * MAXF + r:(i + 1) * MAXF] == SENTINEL).all()
        assert _self_pairs(f, range(first, first + N)) == _self_pairs(f, [s[3] for s in singles])
        # the NN rows: rows 3 .. 5 are rows 0 .. 2 again -- received copies of the reference rows find both at distance 0
        f.nn_append_received(want_nn.cpu().numpy().astype(np.float64))
        f.nn_find_matches()
        dist, idx = f.nn_last_row_minima()
        assert len(dist) == 2 * N and dist[:N].tobytes() == dist[N:].tobytes() and idx[:N].tobytes() == idx[N:].tobytes()
    finally:
        f.close()


def test_refused_call_leaves_both_sizes_and_n0():
    import torch
    dev = torch.device("cuda:0")
    cam, det = _cam(), _abi.detector_params(MAXF)
    p = torch.zeros((2, H * 3 * W), dtype=torch.uint8, device=dev).data_ptr()
    f = _finder(torch)
    try:
        add = lambda **kw: f.add_keyframes_sift_u8_batch_device(p, p, None, RGB8, kw.get("n", 2), W, H, kw.get("pitch", 3 * W),  # noqa: E731
                                                                3 * W * H, cam, kw.get("det", det))
        state = lambda: (f.store_size(), f.nn_sizes(), f.get_feature_type()[0], bytes(f.get_sift_params()))  # noqa: E731
        before = state()
        with pytest.raises(lib.SepfinderError) as e:                          # another feature type: the generic call is named
            add()
        assert e.value.code == _abi.SF_EINVAL and "sf_add_keyframes_u8_batch_device" in str(e.value) and state() == before
        f.set_feature_type_sift()
        before = state()
        with pytest.raises(lib.SepfinderError) as e:                          # no model loaded
            add()
        assert e.value.code == _abi.SF_EINVAL and "model" in str(e.value) and state() == before
        f.netvlad_load(_weights())
        f.nn_append_local(np.zeros((1, DIMS), np.float64))                    # an NN database that is not empty
        before = state()
        assert before[1] == (1, 0)
        for kw, code in ((dict(pitch=3 * W - 1), _abi.SF_EINVAL), (dict(det=_abi.detector_params(0)), _abi.SF_ERANGE),
                         (dict(n=65536), _abi.SF_ERANGE)):
            with pytest.raises(lib.SepfinderError) as e:
                add(**kw)
            assert e.value.code == code and state() == before, kw
        assert add(n=0) == (0, 1) and state() == before                       # n = 0: the first slot and the first NN row
    finally:
        f.close()
