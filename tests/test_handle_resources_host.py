"""Ownership of the handle's resources, without a GPU: the device-free context that sf_debug_plan_workspace builds and
drops (a whole sf_context: every buffer, pinned block and event of the handle as a member of an owning type) constructs and
destructs without touching the counts of sf_debug_live_resources, and plans the same thing every time."""
import ctypes as C

from multi_robot_slam_separators_amd import _abi, lib, synth


def _plan(L, p, kcap, words, n_pairs, overl, dbg):
    out = (C.c_int64 * 22)()
    assert L.sf_debug_plan_workspace(C.byref(p), kcap, words, n_pairs, overl, dbg, out, 22) == 0
    return tuple(int(v) for v in out)


def test_device_free_context_holds_nothing():
    L = lib.load()
    before = lib.debug_live_resources()
    assert tuple(before) == _abi.LIVE_RESOURCES
    # the arguments of tests/test_host_logic.py::test_workspace_reservation_covers_what_every_launch_form_writes
    p = synth.camera_params()
    p.estimation_type = 1
    p.bundle_adjustment = 1
    p.stereo_baseline = 0.12
    p.forward_est_only = 0
    first = _plan(L, p, 1024, 8, 20000, 1, 1)
    assert 1 <= first[3] <= 131072
    for _ in range(100):
        assert _plan(L, p, 1024, 8, 20000, 1, 1) == first
        assert lib.debug_live_resources() == before
