"""GPU: GFTT/BlockSize, GFTT/UseHarrisDetector and GFTT/K (sf_gftt_params; k_gftt_response in csrc/k_gftt.hip) against the
NumPy restatement tests/gftt_ref.py, byte for byte: the detector call on every (block, Harris) pair, the defaults, the
extraction calls that detect with GFTT (types 6, 8, 5; single, batch, ROI, grid) against the explicit chain on the restated
corners, the refusals, the types that do not read the block, and Harris keyframes through the verification path."""
import itertools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from oracle import pyoracle
from tests import extract_cases as ec
from tests import gftt_ref as ref
from tests import grid_ref
from tests.test_gpu_freak import _device_chain, _params, assert_result_parity

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
PAIRS = list(itertools.product((2, 3, 4, 5, 7, 15), (0, 1)))
ARGS = (200, 0.001, 3.0)                                    # max_corners, quality_level, min_distance
IMAGES = {"noise": ref.noise_image, "checkerboard": ref.checkerboard}


@pytest.fixture()
def finder():
    import torch
    f = lib.SeparatorFinder(_params(), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    yield f
    f.close()


def detect(f, torch, image, max_corners, quality, min_distance):
    """sf_detect_corners_device on `image` uploaded with its own pitch (a view of a wider buffer keeps its padding)."""
    h, w = image.shape
    pitch = image.strides[0]
    base = np.lib.stride_tricks.as_strided(image, shape=(h, pitch), strides=(pitch, 1)) if pitch != w else image
    d_img = torch.from_numpy(np.ascontiguousarray(base)).to("cuda:0")
    cap = max_corners if max_corners > 0 else w * h
    out = torch.zeros((cap, 28), dtype=torch.uint8, device="cuda:0")
    n = f.detect_corners_device(d_img.data_ptr(), w, h, pitch, max_corners, quality, min_distance, out.data_ptr(), cap)
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy()[:min(n, cap)].tobytes(), dtype=KP).copy()


def same_keypoints(got, want, ctx):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for name in FIELDS:
        assert got[name].tobytes() == want[name].tobytes(), (ctx, name)
    assert got.tobytes() == want.tobytes(), ctx


def same_rows(got, want, ctx=""):
    (desc, xyz, kp), (d, p, k) = got, want
    assert len(desc) == len(d), (ctx, len(desc), len(d))
    assert desc.tobytes() == d.tobytes(), ctx
    assert kp.tobytes() == k.tobytes(), ctx
    assert np.array_equal(np.isnan(xyz), np.isnan(p)), ctx
    assert xyz[~np.isnan(xyz)].tobytes() == p[~np.isnan(p)].tobytes(), ctx


def state(f):
    return bytes(f.gftt_get_params()), f.store_size(), f.get_feature_type()[0]


@pytest.mark.parametrize("name", ["noise", "checkerboard"])
def test_detector_equals_restatement_for_every_pair(finder, name):
    import torch
    image = ref.pitched(IMAGES[name]())
    assert image.strides[0] > image.shape[1]
    seen = {}
    cases = [(b, hd, 0.04) for b, hd in PAIRS] + [(5, 1, 0.0), (5, 1, 0.15)]
    for b, hd, k in cases:
        finder.gftt_set_params(_abi.gftt_params(b, hd, k))
        got = detect(finder, torch, image, *ARGS)
        want = ref.detect_corners(image, *ARGS, block=b, harris=hd, k=k)
        print("%s block %d harris %d k %g: %d corners (restatement %d)" % (name, b, hd, k, len(got), len(want)))
        same_keypoints(got, want, (b, hd, k))
        assert len(got) >= 50 and (got["size"] == b).all()
        seen[(b, hd, k)] = got[["x", "y"]].tobytes()
    assert len(set(seen.values())) == len(seen)               # no parameter is ignored: every case has corners of its own


def test_defaults(finder):
    import torch
    d = finder.gftt_get_params()
    assert (d.block_size, d.use_harris_detector, d.k) == (3, 0, 0.04)
    assert bytes(d) == bytes(_abi.gftt_params())
    for make in IMAGES.values():
        image = ref.pitched(make())
        fresh = detect(finder, torch, image, *ARGS)
        same_keypoints(fresh, pyoracle.detect_corners(np.ascontiguousarray(image), *ARGS), "fresh handle")
        finder.gftt_set_params(_abi.gftt_params(7, 1, 0.1))
        assert detect(finder, torch, image, *ARGS).tobytes() != fresh.tobytes()
        finder.gftt_set_params(_abi.gftt_params(3, 0, 0.04))
        same_keypoints(detect(finder, torch, image, *ARGS), fresh, "defaults set explicitly")
        assert bytes(finder.gftt_get_params()) == bytes(d)


def test_no_limit_no_distance_and_a_harris_image_without_corners(finder):
    """max_corners 0 with min_distance 0 (every candidate, in the sorted order) and the image whose Harris maximum is <= 0."""
    import torch
    image = ref.pitched(ref.noise_image())
    for b, hd in ((4, 1), (15, 0)):
        finder.gftt_set_params(_abi.gftt_params(b, hd, 0.04))
        got = detect(finder, torch, image, 0, 0.01, 0.0)
        same_keypoints(got, ref.detect_corners(image, 0, 0.01, 0.0, b, hd, 0.04), (b, hd))
        assert len(got) > 200
    ramp = np.tile(np.arange(0, 240, 4, dtype=np.uint8), (30, 1))
    finder.gftt_set_params(_abi.gftt_params(5, 1, 0.04))
    assert len(detect(finder, torch, ramp, 100, 0.001, 3.0)) == 0
    # sides equal to the block: every window index reflects
    tiny = ref.pitched(ref.noise_image()[:15, :15])
    finder.gftt_set_params(_abi.gftt_params(15, 0, 0.04))
    same_keypoints(detect(finder, torch, tiny, 0, 0.001, 0.0), ref.detect_corners(tiny, 0, 0.001, 0.0, 15, 0, 0.04), "15 x 15")


def restated_keypoints(left, det, prm, rows=1, cols=1, ratios=(0.0, 0.0, 0.0, 0.0)):
    """The keypoints of a keyframe under a grid / ROI as tests/grid_ref.py states them, with the restated detector."""
    h, w = left.shape
    boxes, quota = grid_ref.cells(w, h, ratios, rows, cols, det.max_features)
    out = []
    for x, y, cw, ch in boxes:
        cell = np.ascontiguousarray(left[y:y + ch, x:x + cw])
        kp = ref.detect_corners(cell, quota, det.quality_level, det.min_distance, prm.block_size, prm.use_harris_detector, prm.k)
        kp["x"] += np.float32(x)
        kp["y"] += np.float32(y)
        out.append(kp)
    return np.concatenate(out)


def set_type(f, ftype):
    f.store_clear()
    if ftype == 5:
        f.set_feature_type_freak(5, _abi.freak_params(pattern_scale=12.0))
    else:
        f.set_feature_type(ftype)


@pytest.mark.parametrize("ftype", [6, 8, 5])
def test_single_call_equals_the_explicit_chain(finder, ftype):
    import torch
    h, w = 240, 320
    det = _abi.detector_params(300, 0.01, 5.0)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(700, width=w, height=h, max_disp=40.0)[:2])
    set_type(finder, ftype)
    results = {}
    for b, hd in ((5, 1), (4, 0)):
        prm = _abi.gftt_params(b, hd, 0.04)
        finder.gftt_set_params(prm)
        single = finder.get_features_and_descriptor(left, right, cam, det)
        kp = restated_keypoints(left, det, prm)
        assert len(kp) > 50 and (kp["size"] == b).all()
        chain, _ = _device_chain(finder, torch, left, right, cam, kp)
        print("type %d block %d harris %d: %d corners, %d rows" % (ftype, b, hd, len(kp), len(single[0])))
        assert len(single[0]) > 50
        same_rows(single[:3], chain, (ftype, b, hd))
        u8 = finder.get_features_and_descriptor_u8(left, right, _abi.SF_IMAGE_MONO8, cam, det)
        same_rows(u8[:3], single[:3], "mono8 form")
        results[(b, hd)] = single[2][["x", "y"]].tobytes()
    assert results[(5, 1)] != results[(4, 0)]


def batch(f, torch, pairs, cam, det, rows_cap):
    h, w = pairs[0][0].shape
    n_kf, nb = len(pairs), f.descriptor_bytes()
    L = torch.from_numpy(np.stack([l for l, _ in pairs]).reshape(n_kf, -1)).to("cuda:0")
    R = torch.from_numpy(np.stack([r for _, r in pairs]).reshape(n_kf, -1)).to("cuda:0")
    rows = torch.full((n_kf,), -1, dtype=torch.int32, device="cuda:0")
    desc = torch.full((n_kf, rows_cap, nb), 0xEE, dtype=torch.uint8, device="cuda:0")
    xyz = torch.zeros((n_kf, rows_cap, 3), dtype=torch.float32, device="cuda:0")
    kp = torch.zeros((n_kf, rows_cap, 28), dtype=torch.uint8, device="cuda:0")
    before = f.store_size()
    first = f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, h * w, cam, det, None,
                                                       rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
    torch.cuda.synchronize()
    assert first == before and f.store_size() == before + n_kf
    rows, out = rows.cpu().numpy(), []
    for i in range(n_kf):
        n = int(rows[i])
        assert (desc[i, n:] == 0xEE).all()
        out.append((desc[i, :n].cpu().numpy(), xyz[i, :n].cpu().numpy(), np.frombuffer(kp[i, :n].cpu().numpy().tobytes(), dtype=KP)))
    return out


@pytest.mark.parametrize("front", ["plain", "grid 2 x 2", "roi"])
def test_batch_equals_single_calls(finder, front):
    """Three different pairs under (7, 0) and (3, 1): every keyframe of the batch = its single call = the explicit chain on
    the restated corners of the image, of the ROI (Vis/RoiRatios 0.1 0.1 0 0) or of the 2 x 2 cells, whose edges reflect
    with the block's halo."""
    import torch
    h, w, maxf = 150, 203, 200
    det = _abi.detector_params(maxf, 0.01, 3.0)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    pairs = [tuple(np.ascontiguousarray(a) for a in ec.make_stereo_pair(710 + i, width=w, height=h, max_disp=30.0)[:2])
             for i in range(3)]
    rows, cols = (2, 2) if front.startswith("grid") else (1, 1)
    ratios = (0.1, 0.1, 0.0, 0.0) if front == "roi" else (0.0, 0.0, 0.0, 0.0)
    rows_cap = grid_ref.compute_grid(w, h, ratios, rows, cols, maxf)[5]
    for b, hd in ((7, 0), (3, 1)):
        prm = _abi.gftt_params(b, hd, 0.04)
        finder.store_clear()
        finder.gftt_set_params(prm)
        finder.front_set_params(_abi.front_params())
        finder.grid_set_params(_abi.grid_params(1, 1))
        chains = []
        for l, r in pairs:
            kp = restated_keypoints(l, det, prm, rows, cols, ratios)
            chains.append(_device_chain(finder, torch, l, r, cam, kp)[0])
        finder.front_set_params(_abi.front_params(ratios))
        finder.grid_set_params(_abi.grid_params(rows, cols))
        singles = [finder.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
        got = batch(finder, torch, pairs, cam, det, rows_cap)
        for i in range(3):
            print("%s block %d harris %d keyframe %d: %d rows" % (front, b, hd, i, len(singles[i][0])))
            assert len(singles[i][0]) > 30 and (singles[i][2]["size"] == b).all()
            same_rows(singles[i][:3], chains[i], (front, b, hd, i, "single = chain"))
            same_rows(got[i], singles[i][:3], (front, b, hd, i, "batch = single"))
        assert singles[0][2].tobytes() != singles[1][2].tobytes()


def test_u8_batch_equals_single_calls():
    """sf_add_keyframes_u8_batch_device reads the handle's block as well: rgb8 camera images under (5, 1), every slot what
    sf_get_features_and_descriptor_u8 gives for its pair."""
    import torch
    from tests.test_gpu_image import _finder, _weights, colourise
    w, h, maxf = 203, 150, 150
    cam, det = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11), _abi.detector_params(maxf, 0.01, 3.0)
    grays = [ec.make_stereo_pair(720 + i, width=w, height=h, max_disp=30.0)[:2] for i in range(2)]
    pairs = [(colourise(l, 10 + i), colourise(r, 20 + i)) for i, (l, r) in enumerate(grays)]
    pitch, stride = 3 * w + 5, (3 * w + 5) * h + 64

    def packed(images):
        buf = np.full((len(images), stride), 0xA5, np.uint8)
        for i, c in enumerate(images):
            np.lib.stride_tricks.as_strided(buf[i], shape=(h, w, 3), strides=(pitch, 3, 1))[...] = c
        return torch.from_numpy(buf).to("cuda:0")

    d_l, d_r = packed([p[0] for p in pairs]), packed([p[1] for p in pairs])
    f = _finder(torch, w=w, h=h, dims=128)
    try:
        f.netvlad_load(_weights())
        f.gftt_set_params(_abi.gftt_params(5, 1, 0.04))
        singles = [f.get_features_and_descriptor_u8(l, r, _abi.SF_IMAGE_RGB8, cam, det) for l, r in pairs]
        assert min(len(s[0]) for s in singles) > 30 and (singles[0][2]["size"] == 5).all()
        nb = f.descriptor_bytes()
        n_rows = torch.full((2,), -7, dtype=torch.int32, device="cuda:0")
        desc = torch.full((2 * maxf, nb), 0xEE, dtype=torch.uint8, device="cuda:0")
        xyz = torch.zeros((2 * maxf, 3), dtype=torch.float32, device="cuda:0")
        kp = torch.zeros((2 * maxf, 28), dtype=torch.uint8, device="cuda:0")
        f.add_keyframes_u8_batch_device(d_l.data_ptr(), d_r.data_ptr(), None, _abi.SF_IMAGE_RGB8, 2, w, h, pitch, stride, cam,
                                        det, None, n_rows.data_ptr(), desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
        torch.cuda.synchronize()
        n_rows, desc, xyz, kp = (t.cpu().numpy() for t in (n_rows, desc, xyz, kp))
        for i, s in enumerate(singles):
            blk = slice(i * maxf, i * maxf + int(n_rows[i]))
            same_rows((desc[blk], xyz[blk], np.frombuffer(kp[blk].tobytes(), dtype=KP)), s[:3], i)
    finally:
        f.close()


def test_refusals_change_nothing(finder):
    import torch
    finder.gftt_set_params(_abi.gftt_params(7, 1, 0.06))
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(3, width=96, height=64, max_disp=10.0)[:2])
    cam, det = _abi.stereo_camera(460.0, 458.0, 48.0, 32.0, 0.11), _abi.detector_params(100)
    assert len(finder.get_features_and_descriptor(left, right, cam, det)[0]) >= 0     # (a keyframe in the store)
    before = state(finder)
    assert before[1] == 1
    bad = [(1, 0, 0.04), (16, 0, 0.04), (0, 0, 0.04), (3, 2, 0.04), (3, 1, float("nan")), (3, 1, -0.1), (3, 1, 1.5)]
    for b, hd, k in bad:
        with pytest.raises(lib.SepfinderError) as e:
            finder.gftt_set_params(_abi.gftt_params(b, hd, k))
        assert e.value.code == _abi.SF_EINVAL, (b, hd, k)
        assert str(e.value) and state(finder) == before
    with pytest.raises(lib.SepfinderError) as e:
        finder.gftt_set_params(_abi.gftt_params(16, 0, 0.04))
    assert "not built" in str(e.value)

    def refused(call):
        with pytest.raises(lib.SepfinderError) as e:
            call()
        assert e.value.code == _abi.SF_EINVAL and "block_size" in str(e.value), str(e.value)
        assert state(finder) == before

    # an image side below the block: the detector call and the extraction calls, single and batch
    for shape in ((6, 40), (40, 6)):
        small = np.ascontiguousarray(ref.noise_image()[:shape[0], :shape[1]])
        refused(lambda: detect(finder, torch, small, *ARGS))
        refused(lambda: finder.get_features_and_descriptor(small, small, cam, det))
        d = torch.from_numpy(small).to("cuda:0")
        refused(lambda: finder.get_features_and_descriptor_batch_device(d.data_ptr(), d.data_ptr(), 1, shape[1], shape[0],
                                                                        shape[1], small.size, cam, det))
    assert len(detect(finder, torch, np.ascontiguousarray(ref.noise_image()[:7, :40]), *ARGS)) >= 0   # 7 rows: taken
    d_l, d_r = torch.from_numpy(left).to("cuda:0"), torch.from_numpy(right).to("cuda:0")
    run_batch = lambda: finder.get_features_and_descriptor_batch_device(d_l.data_ptr(), d_r.data_ptr(), 1, 96, 64, 96, 96 * 64, cam, det)
    # a ROI side below the block (and not below 3, which has a refusal of its own)
    finder.front_set_params(_abi.front_params((0.0, 0.0, 0.46, 0.46)))
    assert 3 <= finder.compute_roi(96, 64, (0.0, 0.0, 0.46, 0.46))[3] < 7
    refused(lambda: finder.get_features_and_descriptor(left, right, cam, det))
    refused(run_batch)
    finder.front_set_params(_abi.front_params())
    # a cell side below the block: 96 / 16 = 6 columns
    finder.grid_set_params(_abi.grid_params(2, 16))
    refused(lambda: finder.get_features_and_descriptor(left, right, cam, det))
    refused(run_batch)
    # ... which the default block takes
    finder.gftt_set_params(_abi.gftt_params())
    finder.get_features_and_descriptor(left, right, cam, det)
    assert finder.store_size() == 2


def test_fast_types_do_not_read_the_block(finder):
    h, w = 240, 320
    det = _abi.detector_params(300)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(700, width=w, height=h, max_disp=40.0)[:2])
    finder.set_feature_type(4)
    first = finder.get_features_and_descriptor(left, right, cam, det)
    finder.gftt_set_params(_abi.gftt_params(7, 1, 0.2))
    again = finder.get_features_and_descriptor(left, right, cam, det)
    assert len(first[0]) > 50 and (first[2]["size"] == 7.0).all()
    same_rows(again[:3], first[:3], "type 4")
    # a side below the block is no refusal under a type that does not detect with GFTT
    finder.gftt_set_params(_abi.gftt_params(15, 0, 0.04))
    finder.front_set_params(_abi.front_params((0.48, 0.48, 0.0, 0.0)))
    assert 3 <= finder.compute_roi(w, h, (0.48, 0.48, 0.0, 0.0))[2] < 15
    finder.get_features_and_descriptor(left, right, cam, det)


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_of_harris_keyframes(estimation_type):
    """Two views of one scene (a stereo pair and its copy shifted by 8 pixels) with Harris corners of block 5 under type 6:
    verify_pairs equals the oracle on the wire copies of the rows, 3D-3D and PnP; a keyframe against itself succeeds."""
    import torch
    h, w = 240, 320
    wide_l, wide_r, _ = ec.make_stereo_pair(700, width=w + 8, height=h, max_disp=40.0)
    views = [(np.ascontiguousarray(wide_l[:, o:o + w]), np.ascontiguousarray(wide_r[:, o:o + w])) for o in (0, 8)]
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(400)
    with lib.SeparatorFinder(_params(w, h, estimation_type), device=0) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        f.gftt_set_params(_abi.gftt_params(5, 1, 0.04))
        a = f.get_features_and_descriptor(*views[0], cam, det)
        b = f.get_features_and_descriptor(*views[1], cam, det)
        a2 = f.get_features_and_descriptor(*views[0], cam, det)
        same_rows(a2[:3], a[:3])
        assert len(a[0]) > 100 and len(b[0]) > 100 and (a[2]["size"] == 5).all()
        host = {s[3]: s[:3] for s in (a, b, a2)}
        fr, to = [a[3], a[3], b[3]], [a2[3], b[3], a2[3]]
        res = f.verify_pairs(fr, to)
        for j, (x, y) in enumerate(zip(fr, to)):
            o = pyoracle.estimate_transform(f.params, _abi.FeatureArrays(*host[x]), _abi.FeatureArrays(*host[y]))
            print("pair %d: success gpu %d oracle %d, inliers %d / %d, matches %d / %d" % (
                j, res[j]["success"], o["success"], res[j]["inliers"], o["inliers"], res[j]["matches"], o["matches"]))
            assert_result_parity(res[j], o, "pair %d" % j)
        assert res[0]["success"] == 1 and res[0]["inliers"] > 20               # the keyframe against itself
