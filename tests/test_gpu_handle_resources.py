"""Ownership of the handle's resources on the device: every device block, pinned block and event a handle takes is a member
of an owning type, so sf_destroy returns all of them whatever the handle has done -- held against the process-wide counts of
sf_debug_live_resources (include/sf_experimental.h), which do not move under other work on a shared card."""
import functools
import gc

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from tests import depth_ref
from tests import extract_cases as ec
from tests import rectify_ref
from tests.test_rectify_host import abi_info

pytestmark = pytest.mark.gpu

W, H = 97, 131                      # the size of the depth extraction tests (tests/test_gpu_depth.py)
SW, SH = 96, 64                     # the stereo pair (tests/test_gpu_gftt_params.py), also the rectification's raw pair
MAXF = 64
RESULT_BYTES = _abi.RESULT_DTYPE.itemsize


def _finder():
    import torch
    p = synth.camera_params()
    p.max_features = MAXF
    p.store_capacity = 2            # the third keyframe makes sf_store_reserve reallocate
    p.netvlad_dimensions = 128
    p.iterations = 100
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


def _baseline():
    gc.collect()                    # (a handle an earlier test dropped without closing goes now, not in the middle)
    return lib.debug_live_resources()


@functools.lru_cache(maxsize=None)
def _depth_frame(seed):
    img, depth = depth_ref.image(W, H, seed), depth_ref.scene(W, H, seed + 100, _abi.SF_DEPTH_U16_MM)
    img.setflags(write=False)
    depth.setflags(write=False)
    return img, depth


def _depth_keyframe(f, seed=60):
    img, depth = _depth_frame(seed)
    cam = depth_ref.camera(W, H, min_depth=0.6, max_depth=5.0)
    return f.get_features_and_descriptor_depth(img, depth, cam, _abi.detector_params(MAXF))


@functools.lru_cache(maxsize=None)
def _netvlad_rows():
    """8 local and 8 received rows of 128 dimensions: rows 0 .. 3 of either side are neighbours, the rest are not."""
    rng = np.random.default_rng(5)
    a = rng.normal(size=(8, 128))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.normal(size=(8, 128))
    b[:4] = a[:4] + 0.002 * rng.normal(size=(4, 128))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return a, b


def test_destroy_returns_everything():
    import torch
    base = _baseline()
    f = _finder()
    try:
        det = _abi.detector_params(MAXF)
        # one host stereo keyframe
        left, right = (np.ascontiguousarray(a) for a in ec.make_stereo_pair(3, width=SW, height=SH, max_disp=10.0)[:2])
        f.get_features_and_descriptor(left, right, _abi.stereo_camera(460.0, 458.0, SW / 2.0, SH / 2.0, 0.11), det)
        # one host depth keyframe with Vis/DepthAsMask on: the device copy of the depth image and the mask plane
        f.depth_set_params(_abi.depth_params(1))
        _depth_keyframe(f)
        assert f.store_size() == 2
        # one depth batch call: keyframes three and four, the store grows past its two slots
        frames = [_depth_frame(110), _depth_frame(112)]
        d_img = torch.from_numpy(np.stack([fr[0] for fr in frames])).to("cuda:0")
        d_depth = torch.from_numpy(np.stack([fr[1] for fr in frames]).view(np.uint8)).to("cuda:0")
        torch.cuda.synchronize()
        first = f.get_features_and_descriptor_depth_batch_device(d_img.data_ptr(), d_depth.data_ptr(), _abi.SF_DEPTH_U16_MM, 2, W, H,
                                                                 W, W * H, 2 * W, 2 * W * H, depth_ref.camera(W, H), det)
        assert first == 2 and f.store_size() == 4
        # one rectification plan per camera, in the table form (SF_OPT_RECTIFY_TABLE as a handle starts)
        il, ir = (rectify_ref.case_info("barrel", SW, SH, side=s) for s in (0, 1))
        pl, pr = f.rectify_plan_create(abi_info(il)), f.rectify_plan_create(abi_info(ir))
        f.rectify_pair(left, right, _abi.SF_IMAGE_MONO8, pl, pr)
        # the NN stage
        local, received = _netvlad_rows()
        f.nn_append_local(local)
        f.nn_append_received(received)
        m = f.nn_find_matches()
        assert sorted(m["idx_local"]) == [0, 1, 2, 3]
        # two pairs from host matches
        pairs = np.zeros(2, _abi.MATCH_DTYPE)
        pairs["idx_local"], pairs["idx_other"] = [0, 1], [2, 3]
        d_out = torch.zeros(2 * RESULT_BYTES, dtype=torch.uint8, device="cuda:0")
        f.verify_matches_device(pairs, 0, 0, d_out.data_ptr())
        # one step
        f.step_issue(0, 0)
        matches, _, _, info = f.step_retire(copy=True)
        assert info["n_matches"] == 4 and sorted(matches["idx_local"]) == [0, 1, 2, 3]
        f.synchronize()
        live = lib.debug_live_resources()
        # what those calls are known to reserve: the work-list counters of sf_create (1), the store's four arenas, dp_depth and
        # dp_mask, rect_blocks and a table per plan (3), rows and norms of both databases (4), the append's device staging (1),
        # pair_from and pair_to (2), the step block's two device buffers (2); pinned: the append's staging, the pair lists, the
        # step block; events: nn_stage_done, pairs_staged, the step block's `done`
        print("live with the handle open:", {k: live[k] - base[k] for k in live})
        assert live["device_blocks"] - base["device_blocks"] >= 19
        assert live["device_bytes"] > base["device_bytes"]
        assert live["pinned_blocks"] - base["pinned_blocks"] >= 3
        assert live["events"] - base["events"] >= 3
    finally:
        f.close()
    assert lib.debug_live_resources() == base


def test_two_handles_are_independent():
    base = _baseline()
    fa, fb = _finder(), _finder()
    try:
        _depth_keyframe(fa)
        before = _depth_keyframe(fb)
        fa.close()
        after = _depth_keyframe(fb)
        assert len(before[0]) >= 5 and (before[3], after[3]) == (0, 1)
        for x, y in zip(before[:3], after[:3]):
            assert x.tobytes() == y.tobytes()
    finally:
        fa.close()
        fb.close()
    assert lib.debug_live_resources() == base
