"""The three-launch form of the 3D-3D survivors' chains (SF_OPT_CHAIN_NARROW_EST: k_chain_est pass 1, k_chain part 3,
k_chain_est pass 2) against the CPU oracle byte for byte, and against the same handle with the option off.

The one-wavefront estimates take lists of up to 256 correspondences; a longer list keeps the wide kernel, which then
either finishes the pair or hands it on.  The frames below put the counts of both passes on every side of that cap:
pass 1 with exactly 3, 63, 64, 65, 255, 256 and 257 correspondences (tests/test_gpu_chain_sum_shapes.py's pairs), pass 1
under the cap with pass 2 over it (descriptor bit flips keep the global ratio test from what the guided windows still
find), the reverse and both over it (a wide turn moves shared features out of the other image; planar motions, so
that the counts hold with Reg/Force3DoF on as well), a first estimate that comes out null (shared descriptors on
unrelated 3D points: guided matching is not eligible), a guided pass that leaves too few correspondences for a second
estimate, and pairs that never reach a chain.  The oracle's counts are asserted, so a generator that drifts fails here
and not silently."""
import ctypes as C

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, synth
from test_gpu_chain_sum_shapes import _pairs

pytestmark = pytest.mark.gpu

CAP = 256
EDGES = (3, 63, 64, 65, 255, 256, 257)
_made = {}


def _planar(rng, angle, trans):
    """A motion Reg/Force3DoF keeps: yaw and a translation in the plane (so that the guided pass finds its windows)."""
    T = np.eye(4)
    yaw = np.deg2rad(rng.uniform(-angle, angle))
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = rng.uniform(-trans, trans, size=2)
    return T


def _partner(seed, shared, flip, angle, trans=1.0, k=500, planar=False):
    rng = np.random.default_rng(seed)
    a = synth.make_keyframe(rng, k, 32)
    T = _planar(rng, angle, trans) if planar else synth.random_transform(rng, angle, trans)
    b, _ = synth.make_true_partner(rng, a, T, overlap=shared / k, noise=0.02, flip=flip)
    return a, b


def _edge_pairs(k):
    """test_gpu_chain_sum_shapes' pairs with exactly EDGES pass-1 correspondences (K = 130: those up to K)."""
    from test_gpu_chain_sum_shapes import TARGETS
    A, B = _pairs(k)
    keep = [i for i, t in enumerate(TARGETS[k]) if t in EDGES or t == 130]
    return [A[i] for i in keep], [B[i] for i in keep], [TARGETS[k][i] for i in keep]


def _cap_pairs():
    """(pass 1, pass 2) = (under, over), (over, under), (over, over) the cap."""
    if "cap" not in _made:
        _made["cap"] = [_partner(7501, 400, 0.25, 5.0, planar=True), _partner(7501, 300, 0.0, 40.0, planar=True),
                        _partner(7501, 400, 0.0, 5.0, planar=True)]
    return [a for a, _ in _made["cap"]], [b for _, b in _made["cap"]]


def _null_pairs():
    """With min_inliers = 20: a null first estimate (100 matches on unrelated points), then three guided passes that
    end without a second estimate (19, 14 and 0 correspondences)."""
    if "null" not in _made:
        rng = np.random.default_rng(7100)
        a = synth.make_keyframe(rng, 500, 32)
        b, _ = synth.make_true_partner(rng, a, synth.random_transform(rng, 20.0, 1.0), overlap=0.2, noise=0.02, flip=0.0)
        out = [(a, _abi.FeatureArrays(b.desc, synth.make_points(rng, (500,)), b.kpts))]
        out += [_partner(7300 + s, 22, 0.0, 70.0, 3.0) for s in (5, 8, 1)]
        _made["null"] = out
    return [a for a, _ in _made["null"]], [b for _, b in _made["null"]]


def _params(min_inliers=3, force_3dof=0):
    p = synth.camera_params()
    p.iterations = 200
    p.min_inliers = min_inliers
    p.force_3dof = force_3dof
    return p


def _plans_narrow(p, kcap=512):
    from multi_robot_slam_separators_amd import lib
    out = (C.c_int64 * 23)()
    assert lib.load().sf_debug_plan_workspace(C.byref(p), kcap, 8, 12, 0, 0, out, 23) == 0
    return int(out[0]) == 2 and int(out[22]) == 1


def _on_and_off(monkeypatch, p, A, B, kcap=512):
    """The pairs through the split form of ONE handle with the option on, then off."""
    from multi_robot_slam_separators_amd import lib
    monkeypatch.setenv("SF_FUSED", "2")
    monkeypatch.setenv("SF_CHAIN_NARROW_EST", "1")
    monkeypatch.delenv("SF_CHAIN_NW", raising=False)
    assert _plans_narrow(p, kcap)                        # (what the handle below plans: the form under test runs)
    with lib.SeparatorFinder(p) as f:
        on = f.estimate_transform_batch(A, B)
        f.set_option(_abi.SF_OPT_CHAIN_NARROW_EST, 0)
        off = f.estimate_transform_batch(A, B)
        f.set_option(_abi.SF_OPT_CHAIN_NARROW_EST, 1)
        again = f.estimate_transform_batch(A, B)
    assert on.tobytes() == again.tobytes()
    return on, off


def _check(on, off, ref, what):
    for i in range(len(ref)):
        assert off[i].tobytes() == ref[i].tobytes(), ("option off", what[i])
        assert on[i].tobytes() == ref[i].tobytes(), ("option on", what[i])


@pytest.mark.parametrize("force_3dof", [0, 1])
def test_counts_around_the_cap_in_both_passes(monkeypatch, oracle, force_3dof):
    A, B, counts = _edge_pairs(500)
    Ac, Bc = _cap_pairs()
    A, B = A + Ac, B + Bc
    assert len(A) <= 12
    p = _params(3, force_3dof)
    ref = oracle.estimate_transform_batch(p, A, B, oracle.num_threads())
    m1 = [int(r["matches_pass1"]) for r in ref]
    m2 = [int(r["matches"]) for r in ref]
    assert m1[:len(counts)] == list(EDGES)
    assert all(int(r["pass2_guided"]) for r in ref[len(counts):])
    assert m1[-3] <= CAP < m2[-3] and m2[-2] <= CAP < m1[-2] and m1[-1] > CAP and m2[-1] > CAP
    assert sum(int(r["success"]) for r in ref) >= (len(A) - 2 if not force_3dof else 3)
    on, off = _on_and_off(monkeypatch, p, A, B)
    _check(on, off, ref, list(zip(m1, m2)))


def test_small_keyframes(monkeypatch, oracle):
    A, B, counts = _edge_pairs(130)
    p = _params(3)
    ref = oracle.estimate_transform_batch(p, A, B, oracle.num_threads())
    assert [int(r["matches_pass1"]) for r in ref] == counts == [3, 63, 64, 65, 130]
    on, off = _on_and_off(monkeypatch, p, A, B, kcap=192)
    _check(on, off, ref, counts)


def test_null_first_estimate_and_no_second_estimate(monkeypatch, oracle):
    A, B = _null_pairs()
    p = _params(20)
    ref = oracle.estimate_transform_batch(p, A, B, oracle.num_threads())
    assert int(ref[0]["matches_pass1"]) == 100 and int(ref[0]["inliers_pass1"]) == 0 and int(ref[0]["pass2_guided"]) == 0
    for r in ref[1:]:       # guided matching ran and left fewer than min_inliers correspondences
        assert int(r["inliers_pass1"]) >= 20 and int(r["pass2_guided"]) == 1 and int(r["matches"]) < 20 and int(r["inliers"]) == 0
    assert sorted(int(r["matches"]) for r in ref[1:]) == [0, 14, 19]
    on, off = _on_and_off(monkeypatch, p, A, B)
    _check(on, off, ref, ["null first estimate", "19 in pass 2", "14 in pass 2", "0 in pass 2"])


def _mixed():
    """Every kind of pair above beside pairs that never reach a chain, in a fixed shuffled order."""
    if "mixed" not in _made:
        A, B, _ = _edge_pairs(500)              # (the pair with 3 correspondences: a non-survivor at min_inliers = 20)
        for more in (_cap_pairs(), _null_pairs()):
            A, B = A + more[0], B + more[1]
        rng = np.random.default_rng(7400)
        A = A + [synth.make_keyframe(rng, 500, 32) for _ in range(3)]
        B = B + [synth.make_keyframe(rng, 500, 32) for _ in range(3)]
        order = np.random.default_rng(7401).permutation(len(A))
        _made["mixed"] = ([A[i] for i in order], [B[i] for i in order])
    return _made["mixed"]


def test_mixed_batch_with_non_survivors(monkeypatch, oracle):
    A, B = _mixed()
    assert len(A) == 17
    p = _params(20)
    ref = oracle.estimate_transform_batch(p, A, B, oracle.num_threads())
    m1 = [int(r["matches_pass1"]) for r in ref]
    assert sum(m < 20 for m in m1) == 4                          # never reach a chain
    assert sum(20 <= m <= CAP for m in m1) >= 9 and sum(m > CAP for m in m1) == 3
    assert 6 <= sum(int(r["success"]) for r in ref) < len(A)
    on, off = _on_and_off(monkeypatch, p, A, B)
    _check(on, off, ref, m1)


def test_through_the_step_pipeline(monkeypatch, oracle):
    """sf_step_issue / sf_step_retire on the three-launch form: the records k_chain_est streams to the host and
    record_of_match, two steps in flight, against the oracle's verdict and bytes for every match."""
    import torch
    from multi_robot_slam_separators_amd import lib
    monkeypatch.setenv("SF_FUSED", "2")
    monkeypatch.setenv("SF_CHAIN_NARROW_EST", "1")
    n_kf, k = 16, 500
    feats = synth.make_store_batch(11, n_kf, k=k, cols=32, true_frac=0.5)
    rng = np.random.default_rng(12)
    nv_a = rng.normal(size=(n_kf, 128)); nv_a /= np.linalg.norm(nv_a, axis=1, keepdims=True)
    nv_b = nv_a + 0.002 * rng.normal(size=(n_kf, 128)); nv_b /= np.linalg.norm(nv_b, axis=1, keepdims=True)
    r = _params(20)
    r.netvlad_dimensions = 128
    r.netvlad_max_matches_nb = n_kf
    r.max_features = k
    assert _plans_narrow(r)
    dev = torch.device("cuda:0")
    with lib.SeparatorFinder(r, device=0) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        T = {key: torch.from_numpy(np.ascontiguousarray(feats[key]).view(np.uint8) if feats[key].dtype.fields else
                                   np.ascontiguousarray(feats[key])).to(dev)
             for key in ("desc_a", "xyz_a", "kp_a", "desc_b", "xyz_b", "kp_b")}
        sa = f.store_add_keyframes_device(n_kf, k, 32, T["desc_a"].data_ptr(), T["xyz_a"].data_ptr(), T["kp_a"].data_ptr())
        sb = f.store_add_keyframes_device(n_kf, k, 32, T["desc_b"].data_ptr(), T["xyz_b"].data_ptr(), T["kp_b"].data_ptr())
        torch.cuda.synchronize()
        f.nn_append_received(nv_a)
        f.nn_append_local(nv_b)
        f.step_issue(sa, sb)
        f.step_issue(sa, sb)
        for _ in range(2):
            matches, rom, recs, info = f.step_retire(copy=True)
            assert info["n_matches"] == n_kf
            n_ok = 0
            for i in range(n_kf):
                il, io = int(matches["idx_local"][i]), int(matches["idx_other"][i])
                o = oracle.estimate_transform(
                    r, _abi.FeatureArrays(feats["desc_a"][io], feats["xyz_a"][io], feats["kp_a"][io]),
                    _abi.FeatureArrays(feats["desc_b"][il], feats["xyz_b"][il], feats["kp_b"][il]))
                assert (rom[i] >= 0) == bool(o["success"]), ("step", i)
                if o["success"]:
                    n_ok += 1
                    assert recs[rom[i]].tobytes() == o.tobytes(), ("step record", i)
            assert n_ok >= 3
