"""The code of k_match_split around its scan -- the staging loop, the list compaction with all of a wavefront's ballots in
front of one barrier, and the record of a pair without an estimate written sixteen bytes per lane (docs/match_tail.md) --
against the CPU oracle byte for byte, through the C ABI with SF_FUSED=2 so that k_match_split runs.

Every slot of a launch is compared: the whole 368-byte sf_result, the pass-1 correspondence list (order included: the
compaction's ascending "from" index) and the pass states of both passes as the debug outputs expose them.  A void slot
(pair index -1 or >= the store's size) must hold the record of a pair that has nothing: the oracle's for two empty frames.
  * (Kf, Kt) out of 0, 1, 2, 31, 32, 33, 255, 256, 257, 500, 512 at kcap 512: one and two compaction trips, a ragged and a
    full last trip, one staging trip that is ragged or full;
  * pairs that stop at each gate of match_gates: too few features on either side, too few matches, and a motion estimate
    that is due but has fewer correspondences than it needs, so that `matches` is the count of finite points;
  * survivors, void slots, and a shuffled mix of all of them;
  * K = 1000 at kcap 1024 (four trips) and K up to 2048 at kcap 2048 (eight, and six with a ragged one);
  * two steps in flight through sf_step_issue / sf_step_retire: record_of_match and the streamed records."""
import numpy as np
import pytest
import torch

from multi_robot_slam_separators_amd import _abi, lib, synth

pytestmark = pytest.mark.gpu

RB = _abi.RESULT_DTYPE.itemsize
KS = (0, 1, 2, 31, 32, 33, 255, 256, 257, 500, 512)


def _cut(fa, n):
    if n == 0:
        cols = fa.desc.shape[1]
        return _abi.FeatureArrays(np.zeros((0, cols), np.uint8), np.zeros((0, 3), np.float32), np.zeros(0, _abi.KEYPOINT_DTYPE))
    return _abi.FeatureArrays(fa.desc[:n], fa.xyz[:n], fa.kpts[:n])


def _params(max_features):
    p = synth.camera_params()
    p.iterations = 100
    p.min_inliers = 5
    p.max_features = max_features
    return p


@pytest.fixture(scope="module")
def base():
    """One true pair of 520 rows and one unrelated frame: every case at kcap 512 is cut from them."""
    A, B, _, _ = synth.make_pairs(5201, 1, k=520, cols=32, true_frac=1.0)
    rng = np.random.default_rng(5202)
    return A[0], B[0], synth.make_keyframe(rng, 512, 32)


def _planted(a, other, rows, nan_rows=()):
    """`other` with its first len(rows) descriptors replaced by rows `rows` of a: that many certain matches."""
    d, x = other.desc.copy(), other.xyz.copy()
    for j, r in enumerate(rows):
        d[j] = a.desc[r]
    for j in nan_rows:
        x[j] = np.nan
    return _abi.FeatureArrays(d, x, other.kpts)


def _verify(f, fs, ts):
    dev = torch.device("cuda:0")
    n = len(fs)
    d_from = torch.tensor(fs, dtype=torch.int32, device=dev)
    d_to = torch.tensor(ts, dtype=torch.int32, device=dev)
    out = torch.full((n, RB), 0x5A, dtype=torch.uint8, device=dev)      # (a byte nobody writes would show)
    f.verify_pairs_device(d_from.data_ptr(), d_to.data_ptr(), n, out.data_ptr())
    f.synchronize()
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), dtype=_abi.RESULT_DTYPE)


def _run(monkeypatch, oracle, p, A, B, void_at=(), order=None):
    """Pairs (A[j] "from", B[j] "to") in `order`, with void slots inserted at the positions `void_at` of the launch, against
    the oracle.  Returns the oracle's records of the pairs, in the order of A."""
    assert len(A) + len(void_at) <= 64
    monkeypatch.setenv("SF_FUSED", "2")
    monkeypatch.setenv("SF_DEBUG_CORR", "1")
    order = list(range(len(A))) if order is None else list(order)
    want = {j: oracle.estimate_transform(p, A[j], B[j], debug=True) for j in set(order)}
    nothing = oracle.estimate_transform(p, _cut(A[0], 0), _cut(B[0], 0))
    with lib.SeparatorFinder(p) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        f.prof_enable(True)
        sa = [f.store_add_keyframe(a) for a in A]
        sb = [f.store_add_keyframe(b) for b in B]
        size = f.store_size()
        src = list(order)
        for k, pos in enumerate(sorted(void_at)):
            src.insert(pos, None if k % 2 == 0 else -1)          # None: from = -1; -1: to = one past the last slot
        fs = [-1 if j is None else sa[0] if j == -1 else sa[j] for j in src]
        ts = [sb[0] if j is None else size if j == -1 else sb[j] for j in src]
        got = _verify(f, fs, ts)
        assert f.prof_get()["k_match_global"][0] >= 1              # (the split form's matching launch)
        for i, j in enumerate(src):
            if j is None or j == -1:
                assert got[i].tobytes() == nothing.tobytes(), ("void slot", i)
                _, is_null, inl, m = f.debug_pass_state(i, 1)
                assert (is_null, inl, m) == (1, 0, 0), ("void slot", i)
                continue
            o, c1, _ = want[j]
            ctx = (i, j, len(A[j].desc), len(B[j].desc))
            assert got[i].tobytes() == o.tobytes(), ctx
            g1 = f.debug_correspondences(i, 1)
            assert np.array_equal(g1[0], c1[0]) and np.array_equal(g1[1], c1[1]), ctx
            _, is_null, inl, m = f.debug_pass_state(i, 1)
            assert (is_null == 0, inl, m) == (bool(o["pass1_success"]), o["inliers_pass1"], o["matches_pass1"]), ctx
            _, is_null, inl, m = f.debug_pass_state(i, 2)
            assert (is_null == 0, inl, m) == (bool(o["success"]), o["inliers"], o["matches"]), ctx
    return [want[j][0] if j in want else None for j in range(len(A))]


def test_row_counts_around_the_trips(monkeypatch, oracle, base):
    a, b, _ = base
    combos = [(kf, kt) for kf in KS for kt in (0, 2, 33, 256, 500)]
    combos += [(512, 512), (257, 512), (1, 1), (31, 31), (255, 255), (256, 257), (500, 512), (512, 500), (32, 32)]
    assert len(combos) == 64
    res = _run(monkeypatch, oracle, _params(512), [_cut(a, kf) for kf, _ in combos], [_cut(b, kt) for _, kt in combos])
    assert sum(int(r["success"]) for r in res) >= 5


def _gate_cases(base):
    a, b, other = base
    a5, b5 = _cut(a, 500), _cut(b, 500)
    A, B, kind = [], [], []
    for fa, fb, k in (
            (_cut(a, 4), b5, "few features"), (a5, _cut(b, 4), "few features"), (_cut(a, 3), _cut(b, 3), "few features"),
            (a5, _cut(other, 500), "few matches"), (_cut(a, 257), _cut(other, 300), "few matches"),
            (a5, _planted(a, _cut(other, 500), (10, 300, 499, 256)), "counted"),
            (a5, _planted(a, _cut(other, 500), (10, 300, 499, 256), nan_rows=(1, 2)), "counted"),
            (_cut(a, 300), _planted(a, _cut(other, 40), (0, 255, 256, 299), nan_rows=(0,)), "counted"),
            (a5, b5, "survivor"), (_cut(a, 257), _cut(b, 257), "survivor"), (_cut(a, 512), _cut(b, 512), "survivor")):
        A.append(fa); B.append(fb); kind.append(k)
    return A, B, kind


def test_every_gate_of_the_motion_estimate(monkeypatch, oracle, base):
    A, B, kind = _gate_cases(base)
    res = _run(monkeypatch, oracle, _params(512), A, B, void_at=(0, 5, 13))
    for r, k in zip(res, kind):
        if k == "survivor":
            assert r["success"] == 1, k
        else:
            assert r["success"] == 0 and r["pass1_success"] == 0, k
        if k == "few features":
            assert r["matches"] == 0, k
    counted = [int(r["matches"]) for r, k in zip(res, kind) if k == "counted"]
    # (the count of finite points of a pair whose estimate is due and cannot run: non-zero, and smaller with NaN points)
    assert counted[0] > 0 and 0 < counted[1] < counted[0] and counted[2] > 0, counted


def test_shuffled_mix(monkeypatch, oracle, base):
    A, B, _ = _gate_cases(base)
    rng = np.random.default_rng(5203)
    order = [int(j) for j in rng.permutation(np.repeat(np.arange(len(A)), 5))]           # 55 pairs, each case five times
    _run(monkeypatch, oracle, _params(512), A, B, void_at=(0, 7, 8, 20, 31, 40, 41, 58, 63), order=order)


def test_four_trips_at_kcap_1024(monkeypatch, oracle):
    A, B, _, _ = synth.make_pairs(5204, 2, k=1000, cols=32, true_frac=1.0)
    rng = np.random.default_rng(5205)
    A += [_cut(A[0], 769), synth.make_keyframe(rng, 1000, 32)]
    B += [_cut(B[0], 1000), synth.make_keyframe(rng, 1000, 32)]
    res = _run(monkeypatch, oracle, _params(1024), A, B, void_at=(1, 5))
    assert res[0]["success"] == 1 and res[3]["success"] == 0


def test_eight_trips_at_kcap_2048(monkeypatch, oracle):
    A, B, _, _ = synth.make_pairs(5206, 1, k=2048, cols=32, true_frac=1.0)
    rng = np.random.default_rng(5207)
    A += [_cut(A[0], 1500), synth.make_keyframe(rng, 2048, 32)]
    B += [_cut(B[0], 2048), synth.make_keyframe(rng, 1281, 32)]
    res = _run(monkeypatch, oracle, _params(2048), A, B, void_at=(0, 4))
    assert res[0]["success"] == 1 and res[2]["success"] == 0


def test_two_steps_in_flight(monkeypatch, oracle):
    monkeypatch.setenv("SF_FUSED", "2")
    n_kf, k = 40, 257
    feats = synth.make_store_batch(5208, n_kf, k=k, cols=32, true_frac=0.3)
    rng = np.random.default_rng(5209)
    nv_a = rng.normal(size=(n_kf, 128)); nv_a /= np.linalg.norm(nv_a, axis=1, keepdims=True)
    nv_b = nv_a + 0.002 * rng.normal(size=(n_kf, 128)); nv_b /= np.linalg.norm(nv_b, axis=1, keepdims=True)
    r = _params(512)
    r.netvlad_dimensions = 128
    r.netvlad_max_matches_nb = n_kf
    dev = torch.device("cuda:0")
    with lib.SeparatorFinder(r) as f:
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
        want = {}
        for step in range(2):
            matches, rom, recs, info = f.step_retire(copy=True)
            assert info["n_matches"] == n_kf
            n_ok = 0
            for i in range(n_kf):
                il, io = int(matches["idx_local"][i]), int(matches["idx_other"][i])
                if (il, io) not in want:
                    want[(il, io)] = oracle.estimate_transform(
                        r, _abi.FeatureArrays(feats["desc_a"][io], feats["xyz_a"][io], feats["kp_a"][io]),
                        _abi.FeatureArrays(feats["desc_b"][il], feats["xyz_b"][il], feats["kp_b"][il]))
                o = want[(il, io)]
                assert (rom[i] >= 0) == bool(o["success"]), (step, i)
                if o["success"]:
                    n_ok += 1
                    assert recs[rom[i]].tobytes() == o.tobytes(), (step, i)
            assert info["n_records"] >= n_ok and 0 < n_ok < n_kf, (step, n_ok, info)
