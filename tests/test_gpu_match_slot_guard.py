"""The slot guard of pass 1 (k_match_global, k_match_global_u8: match_slot_outside and match_report_outside of
sf_match_device.hpp; match_v2_body: the same test and report spelt out): a pair whose "from" or "to" slot lies outside
the store is reported as a failed estimation and touches nothing else.

The host calls refuse such slots before any launch (sf_verify_pairs, sf_verify_matches_device); sf_verify_pairs_device
takes its slots from device memory and relies on the guard, as sf_step's k_spec_pairs does when it writes -1 for a
candidate outside the databases.  Here one list of pairs holds a pair with from = -1 and one with to = store_size: both
records must be the null result (no success, no inliers, no matches), and every other record the same bytes as in the
call without the two.

One case per form of the global matcher.  Each form's launches that run over ALL pairs (not over a survivor list) check
the slots before they index the store, or read only headers / pass states: k_verify_fused (match_v2_body's guard, then
guided_body's bad_slot), k_match_global / k_match_global_u8 (the guard), k_guided (bad_slot), k_finalize (pass states
and flags only); k_ransac and the chains walk the survivor list, which a guarded pair never joins."""
import numpy as np
import pytest
import torch

from multi_robot_slam_separators_amd import _abi, lib, synth

pytestmark = pytest.mark.gpu

K = 200
N_GOOD = 6
RB = _abi.RESULT_DTYPE.itemsize


def _binary():
    p = synth.camera_params()
    p.iterations = 100
    p.max_features = 256
    A, B, _, _ = synth.make_pairs(611, N_GOOD, k=K, cols=32, true_frac=0.5)
    return p, A, B


def _float32():
    p, A, B = _binary()
    p.desc_type, p.desc_bytes = 1, 4 * 64
    rng = np.random.default_rng(612)
    return p, [synth.float_descriptors(a, 64, rng, 0.02) for a in A], [synth.float_descriptors(b, 64, rng, 0.02) for b in B]


def _uint8():
    p, A, B = _binary()
    p.desc_type, p.desc_bytes = 2, 128
    rng = np.random.default_rng(613)
    return p, [synth.u8_descriptors(a, 128, rng, 12) for a in A], [synth.u8_descriptors(b, 128, rng, 12) for b in B]


def _verify(f, fs, ts):
    dev = torch.device("cuda:0")
    n = len(fs)
    d_from = torch.tensor(fs, dtype=torch.int32, device=dev)
    d_to = torch.tensor(ts, dtype=torch.int32, device=dev)
    out = torch.full((n, RB), 0x5A, dtype=torch.uint8, device=dev)      # (a record nobody writes would show)
    f.verify_pairs_device(d_from.data_ptr(), d_to.data_ptr(), n, out.data_ptr())
    f.synchronize()
    torch.cuda.synchronize()
    return np.frombuffer(out.cpu().numpy().tobytes(), dtype=_abi.RESULT_DTYPE)


@pytest.mark.parametrize("form", ["default", "mfma_off", "float32", "uint8"])
def test_slots_outside_the_store_give_the_null_result(monkeypatch, form):
    if form == "mfma_off":
        monkeypatch.setenv("SF_MATCH_MFMA", "0")
    p, A, B = {"default": _binary, "mfma_off": _binary, "float32": _float32, "uint8": _uint8}[form]()
    with lib.SeparatorFinder(p) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        sa = [f.store_add_keyframe(a) for a in A]
        sb = [f.store_add_keyframe(b) for b in B]
        size = f.store_size()
        assert size == 2 * N_GOOD
        good = _verify(f, sa, sb)
        # the two bad pairs in the middle of the list: from = -1 (what k_spec_pairs writes), to = one past the last slot
        fs = sa[:2] + [-1] + sa[2:4] + [sa[4]] + sa[4:]
        ts = sb[:2] + [sb[2]] + sb[2:4] + [size] + sb[4:]
        got = _verify(f, fs, ts)
    bad = (2, 5)
    for i in bad:
        r = got[i]
        assert r["success"] == 0 and r["pass1_success"] == 0 and r["inliers"] == 0 and r["matches"] == 0, (form, i, r)
        assert r["inliers_pass1"] == 0 and r["matches_pass1"] == 0, (form, i, r)
    rest = [i for i in range(len(fs)) if i not in bad]
    assert len(rest) == N_GOOD
    for j, i in enumerate(rest):
        assert got[i].tobytes() == good[j].tobytes(), (form, i)
    assert int(good["success"].sum()) >= 1          # (the matcher did run on the good pairs)
