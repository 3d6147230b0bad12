"""Every verification launcher above 64 KB of dynamic LDS per workgroup, against the oracle.

A launch that asks for more than 64 KB goes through the handle's one attribute path (sf_dyn_lds, sf_internal.hpp); below
that size the path does nothing, and most launchers had no test above it.  The shapes follow from the *_lds_bytes
functions of the kernels' sources, with kcap = K rounded up to a multiple of 64:

  K = 1500 (kcap 1536)  matcher (1536 * 8 + 2 * 1536 + 16) * 4 = 61 504 B <= 64 KB, so the fused and the split form apply;
                        list + guided stage (1536 + 9 * 1536 + 2048 + 20 + cells) * 4 > 66 KB: k_verify_fused, k_chain
  K = 1700 (kcap 1728)  matcher (1728 * 10 + 16) * 4 = 69 184 B: k_match_split; k_chain_pnp about 70 KB; K <= MF_MAX_ROWS
  K = 1000 (kcap 1024)  k_pnp about 68 KB
  K =  700 (kcap  704)  k_merge_directions_ba: 21 B + 72 B per feature, about 67 KB
  K = 3300 (kcap 3328)  k_guided_tp (5 * 3328 + 20 + 2 * cells) * 4 > 66 KB, k_ransac about 144 KB (under the CU's 160 KB)

2 to 4 pairs, 32-byte rows, 100 iterations.  The profiler slots show which form ran (as in
test_gpu_verify.py::test_scalar_load_matcher_at_512_bit_rows)."""
import numpy as np
import pytest

from multi_robot_slam_separators_amd import synth

from test_gpu_verify import assert_result_parity

pytestmark = pytest.mark.gpu


def _pairs(seed, n, k):
    """n pairs of K features, 32-byte rows: the even ones true partners, the odd ones unrelated frames."""
    rng = np.random.default_rng(seed)
    A, B, is_true = [], [], np.zeros(n, dtype=bool)
    for i in range(n):
        a = synth.make_keyframe(rng, k, 32)
        if i % 2 == 0:
            b, _ = synth.make_true_partner(rng, a, synth.random_transform(rng), 0.4, 0.02, 0.05)
            is_true[i] = True
        else:
            b = synth.make_keyframe(rng, k, 32)
        A.append(a); B.append(b)
    return A, B, is_true


def _params(k, est=0):
    p = synth.camera_params()
    p.iterations = 100
    p.max_features = k
    p.estimation_type = est
    return p


def _run(p, A, B, calls=1):
    from multi_robot_slam_separators_amd import lib
    with lib.SeparatorFinder(p) as f:
        f.prof_enable(True)
        got = [f.estimate_transform_batch(A, B) for _ in range(calls)]
        prof = {name: n for name, (n, _) in f.prof_get().items()}
    for g in got[1:]:
        assert g.tobytes() == got[0].tobytes()
    return got[0], prof


def _check(oracle, p, A, B, is_true, got, ctx):
    for i in range(len(A)):
        assert_result_parity(got[i], oracle.estimate_transform(p, A[i], B[i]), "%s pair %d" % (ctx, i))
    assert is_true.any() and got["success"][is_true].all(), ctx


@pytest.fixture(scope="module")
def k1500(oracle):
    """The K = 1500 pairs and the oracle's results, shared by the fused and the chain cases."""
    A, B, is_true = _pairs(1500, 3, 1500)
    p = _params(1500)
    return p, A, B, is_true, [oracle.estimate_transform(p, a, b) for a, b in zip(A, B)]


def _check_k1500(case, got, ctx):
    _, A, _, is_true, want = case
    for i in range(len(A)):
        assert_result_parity(got[i], want[i], "%s pair %d" % (ctx, i))
    assert got["success"][is_true].all(), ctx


def test_fused_kernel(monkeypatch, k1500):
    """K = 1500, 3D-3D, the default form of a batch call: k_verify_fused with list + guided stage above 66 KB."""
    monkeypatch.delenv("SF_FUSED", raising=False)
    got, prof = _run(k1500[0], k1500[1], k1500[2])
    assert prof["k_verify_fused"] == 1 and prof["k_match_global"] == 0 and prof["k_ransac(pass1)"] == 0, prof
    _check_k1500(k1500, got, "fused")


@pytest.mark.parametrize("nw", [None, "4"])
def test_chain_kernel(monkeypatch, k1500, nw):
    """K = 1500, 3D-3D, SF_FUSED=2: k_match_split (its slot is the matcher's) and k_chain (its slot is the fused
    kernel's) over the survivors, at the default chain width and with SF_CHAIN_NW=4."""
    monkeypatch.setenv("SF_FUSED", "2")
    if nw is None:
        monkeypatch.delenv("SF_CHAIN_NW", raising=False)
    else:
        monkeypatch.setenv("SF_CHAIN_NW", nw)
    got, prof = _run(k1500[0], k1500[1], k1500[2])
    assert prof["k_match_global"] == 1 and prof["k_verify_fused"] == 1 and prof["k_ransac(pass1)"] == 0, prof
    _check_k1500(k1500, got, "chain nw %s" % nw)


def test_pnp_split_matcher_and_chain(monkeypatch, oracle):
    """K = 1700, PnP, the default form: k_match_split asks 69 184 B and k_chain_pnp about 70 KB."""
    monkeypatch.delenv("SF_FUSED", raising=False)
    monkeypatch.delenv("SF_CHAIN_PNP", raising=False)
    A, B, is_true = _pairs(1700, 2, 1700)
    p = _params(1700, est=1)
    got, prof = _run(p, A, B)
    assert prof["k_match_global"] == 1 and prof["k_verify_fused"] == 1 and prof["k_ransac(pass1)"] == 0, prof
    _check(oracle, p, A, B, is_true, got, "pnp chain")


def test_pnp_stage_kernel(monkeypatch, oracle):
    """K = 1000, PnP, SF_FUSED=0: the stage kernel k_pnp asks about 68 KB."""
    monkeypatch.setenv("SF_FUSED", "0")
    A, B, is_true = _pairs(1000, 3, 1000)
    p = _params(1000, est=1)
    got, prof = _run(p, A, B)
    assert prof["k_ransac(pass1)"] == 1 and prof["k_ransac(pass2)"] == 1 and prof["k_verify_fused"] == 0, prof
    _check(oracle, p, A, B, is_true, got, "pnp stages")


@pytest.mark.parametrize("est", [0, 1])
def test_merge_directions_with_bundle_adjustment(monkeypatch, oracle, est):
    """K = 700, Vis/ForwardEstOnly = false with the bundle adjustment: k_merge_directions_ba asks 93 B per feature, about
    67 KB.  Both directions run on the stage kernels; the adjustment is the merge kernel's, not k_ba_pass's."""
    monkeypatch.delenv("SF_FUSED", raising=False)
    A, B, is_true = _pairs(700 + est, 4, 700)
    p = _params(700, est=est)
    p.forward_est_only = 0
    p.bundle_adjustment = 1
    p.stereo_baseline = 0.12
    got, prof = _run(p, A, B)
    assert prof["k_ransac(pass1)"] == 1 and prof["k_verify_fused"] == 0 and prof["k_ba_pass"] == 0, prof
    _check(oracle, p, A, B, is_true, got, "merge ba est %d" % est)


def test_guided_tp_and_ransac_twice_on_one_handle(monkeypatch, oracle):
    """K = 3300, Vis/CorGuessMatchToProjection = true, 3D-3D: k_guided_tp above 66 KB and k_ransac at about 144 KB, two
    calls on one handle so that the second launch of each finds the kernel's attribute already set.
    The oracle has only the other guided branch, so a guided pair is compared (assert_result_parity) with the record the
    oracle's estimators give on the restated pass-2 list, as test_gpu_guided_tp.py does; every other pair with the
    oracle's whole result."""
    from test_gpu_guided_tp import _restated
    monkeypatch.delenv("SF_FUSED", raising=False)
    A, B, is_true = _pairs(3300, 2, 3300)
    p = _params(3300)
    p.guess_win_size = 20
    p.guess_match_to_projection = 1
    got, prof = _run(p, A, B, calls=2)
    assert prof["k_guided_tp"] == 2 and prof["k_guided"] == 0, prof
    assert prof["k_ransac(pass1)"] == 2 and prof["k_ransac(pass2)"] == 2 and prof["k_verify_fused"] == 0, prof
    for i in range(len(A)):
        guided, _, _, rec = _restated(oracle, p, A[i], B[i])
        assert bool(got[i]["pass2_guided"]) == guided, i
        want = rec if guided else oracle.estimate_transform(p, A[i], B[i])
        assert_result_parity(got[i], want, "guided tp pair %d" % i)
    assert got["success"][is_true].all()
