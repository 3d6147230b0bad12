"""GPU: block-matching stereo correspondence (csrc/k_stereo_bm.hip, Stereo/OpticalFlow false) through the C-ABI, byte for
byte: sf_stereo_block_match_device against the NumPy restatement tests/stereo_bm_ref.py (position, status, right_x,
score; a guard record behind n stays unwritten); the extraction calls with optical_flow = 0 against the explicit chain
sf_detect_*_device -> restatement -> sf_extract_keyframe_device; the batch forms against the single calls; the default
path after a round trip through block matching; the setters; and a pair of block-matched keyframes through the
verification path against the oracle."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from tests import extract_cases as ec
from tests import fast_ref
from tests import image_ref
from tests import stereo_bm_ref as ref
from tests import subpix_ref
from tests.test_gpu_image import RGB8, _finder, _weights, colourise
from tests.test_gpu_orb import assert_result_parity, assert_same
from tests.test_gpu_orb2 import _pair, _params
from tests.test_gpu_orb2_batch import SENTINEL, _cam, _self_pairs, batch_pairs, run_batch
from tests.test_gpu_subpix import _detect, _dev_image, _fractional, _set_type, records

pytestmark = pytest.mark.gpu

KP = _abi.KEYPOINT_DTYPE
W, H = 202, 170
REFINE = (3, 5, 0.02)


@pytest.fixture()
def finder():
    import torch
    f = lib.SeparatorFinder(_params(w=W, h=H), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def _images(name):
    if name == "small":                                      # 202 x 170, pitch 210, disparities 2 .. 24
        return ec.make_stereo_pair(5, W, H, max_disp=24)[:2]
    if name == "big":                                        # 752 x 480, pitch 760: pitch != width
        return ec.make_stereo_pair(3)[:2]
    raise KeyError(name)


def _edge_points(w, h, ww, wh, max_disp):
    """Every place where the search takes another path for a ww x wh window on a w x h image."""
    hw, hh, maxD = (ww - 1) // 2, (wh - 1) // 2, int(max_disp)
    ym, xm = float(h // 2), float(min(w - hw - 3, hw + maxD + 20))
    pts = [(float(x), ym) for x in range(max(hw - 1, 0), min(hw + 3 + maxD, w))]      # the minCol clamp: empty range .. full range
    pts += [(x + 0.5, ym + 0.25) for x in range(max(hw - 1, 0), min(hw + 3 + maxD, w), 3)]
    pts += [(float(x), ym - 1) for x in range(w - hw - 2, w)]                         # the last hw + 2 columns
    pts += [(xm, float(y)) for y in range(0, hh + 2)] + [(xm, float(y)) for y in range(h - hh - 2, h)]   # first / last hh + 1 rows
    pts += [(xm + 0.5, hh - 0.5), (xm, h - hh - 0.75)]
    pts += [(float(w - hw - 3), ym), (float(w - hw - 3), float(h - hh - 1))]          # inside at level 0, outside at level 2
    return records(pts, seed=9)


@functools.lru_cache(maxsize=None)
def _points(image, name, ww=15, wh=3, max_disp=32):
    left = _images(image)[0]
    h, w = left.shape
    if name == "fast":                                       # all FAST corners of the image, raster order
        kp = fast_ref.detect(left, 20, 1, 0)
        return records(np.stack([kp["x"], kp["y"]], axis=1))
    if name == "fast600":                                    # 600 FAST corners spread over the 752 x 480 image
        kp = fast_ref.detect(left, 20, 1, 0)
        kp = kp[:: max(len(kp) // 600, 1)][:600]
        return records(np.stack([kp["x"], kp["y"]], axis=1))
    if name == "random":                                     # 200 fractional positions
        rng = np.random.default_rng(11)
        return records(np.stack([rng.uniform(0, w - 1, 200), rng.uniform(0, h - 1, 200)], axis=1))
    if name == "int x":                                      # integer x with fractional y: the start score is not recomputed
        rng = np.random.default_rng(12)
        return records(np.stack([np.floor(rng.uniform(0, w - 1, 120)), rng.uniform(0, h - 1, 120)], axis=1))
    if name == "edges":
        return _edge_points(w, h, ww, wh, max_disp)
    if name == "tall":                                       # 40 positions a 3 x 341 window fits around
        rng = np.random.default_rng(13)
        return records(np.stack([rng.uniform(100, w - 4, 40), rng.uniform(168, h - 172, 40)], axis=1))
    raise KeyError(name)


# name: (images, points, (ww, wh), max_level, iterations, min_disparity, max_disparity, ssd)
CASES = {
    "fast 15x3 l5 ssd": ("small", "fast", (15, 3), 5, 30, 0.5, 32.0, 1),
    "fast 15x3 l5 sad": ("small", "fast", (15, 3), 5, 30, 0.5, 32.0, 0),
    "fast 21x5 l5 200 steps": ("small", "fast", (21, 5), 5, 200, 1.0, 32.0, 1),
    "random 15x3 l2": ("small", "random", (15, 3), 2, 30, 1.0, 32.0, 1),
    "random 7x7 l2 1 step sad": ("small", "random", (7, 7), 2, 1, 2.5, 32.0, 0),
    "random 31x31 l5 200 steps sad": ("small", "random", (31, 31), 5, 200, 0.5, 32.0, 0),
    "int x 15x3 l5": ("small", "int x", (15, 3), 5, 30, 0.5, 32.0, 1),
    "edges 15x3 l0": ("small", "edges", (15, 3), 0, 30, 0.5, 32.0, 1),
    "edges 15x3 l2": ("small", "edges", (15, 3), 2, 30, 0.5, 32.0, 1),
    "edges 15x3 l5 min 2.5": ("small", "edges", (15, 3), 5, 30, 2.5, 32.0, 1),
    "edges 7x7 l5 no steps sad": ("small", "edges", (7, 7), 5, 0, 0.5, 32.0, 0),
    "edges 21x5 l2": ("small", "edges", (21, 5), 2, 30, 1.0, 32.0, 1),
    "edges 31x31 l2": ("small", "edges", (31, 31), 2, 30, 0.5, 32.0, 1),
    "big fast 15x3 l5": ("big", "fast600", (15, 3), 5, 30, 0.5, 128.0, 1),
    "big fast 15x3 l0 128 candidates sad": ("big", "fast600", (15, 3), 0, 30, 0.5, 128.0, 0),
    "big random 21x5 l0 127 candidates": ("big", "random", (21, 5), 0, 30, 1.0, 128.0, 1),
    "big edges 15x3 l5": ("big", "edges", (15, 3), 5, 30, 0.5, 128.0, 1),
    "big 3x341 strip beyond LDS": ("big", "tall", (3, 341), 0, 5, 0.5, 128.0, 1),
}


def _case(case):
    image, points, win, max_level, it, dmin, dmax, ssd = CASES[case]
    prm = _abi.stereo_flow_params(win_width=win[0], win_height=win[1], max_level=max_level, iterations=it, min_disparity=dmin,
                                  max_disparity=dmax)
    kp = _points(image, points, win[0], win[1], int(dmax)) if points == "edges" else _points(image, points)
    return _images(image), kp, prm, ssd


@functools.lru_cache(maxsize=None)
def _reference(case):
    (left, right), kp, prm, ssd = _case(case)
    return ref.block_match(left, right, kp, prm, ssd, want_trace=True)


def run_bm(f, torch, left, right, kp, prm, ssd, n=None, optional=True):
    """sf_stereo_block_match_device on the first n of `kp`; every output has one guard record behind len(kp).  Returns
    (xy, status, right_x, score) cut to n after checking that nothing behind n was written."""
    dev = torch.device("cuda:0")
    assert left.strides == right.strides
    d_l, w, h, pitch = _dev_image(torch, left)
    d_r = _dev_image(torch, right)[0]
    n = len(kp) if n is None else n
    m = len(kp) + 1
    d_kp = torch.from_numpy(np.frombuffer(kp.tobytes() + b"\xEE" * 28, np.uint8).copy()).to(dev)
    d_xy = torch.full((m, 2), -7.0, dtype=torch.float32, device=dev)
    d_st = torch.full((m,), 9, dtype=torch.uint8, device=dev)
    d_rx = torch.full((m,), -7.0, dtype=torch.float32, device=dev)
    d_sc = torch.full((m,), -7.0, dtype=torch.float32, device=dev)
    try:
        f.stereo_block_match_device(d_l.data_ptr(), d_r.data_ptr(), w, h, pitch, d_kp.data_ptr(), n, d_xy.data_ptr(),
                                    d_st.data_ptr(), d_rx.data_ptr() if optional else None,
                                    d_sc.data_ptr() if optional else None, params=prm, ssd=ssd)
    finally:
        torch.cuda.synchronize()
    xy, st, rx, sc = d_xy.cpu().numpy(), d_st.cpu().numpy(), d_rx.cpu().numpy(), d_sc.cpu().numpy()
    assert (xy[n:] == -7.0).all() and (st[n:] == 9).all() and (rx[n:] == -7.0).all() and (sc[n:] == -7.0).all()
    if not optional:
        assert (rx == -7.0).all() and (sc == -7.0).all()
    return xy[:n], st[:n], rx[:n], sc[:n]


def _report(case, kp, got, want, trace):
    xy, st, rx, sc = got
    xy0, st0, sc0 = want
    bad = np.flatnonzero((xy != xy0).any(axis=1) | (st != st0) | (rx != xy0[:, 0]) | (sc != sc0))
    levels = sorted({int(l) for t in trace for l in t["level"]})
    cands = max([int((t["lmin"] - t["lmax"]).max()) for t in trace if len(t)] + [0])
    msg = "%s: %d corners, %d with status 1, %d without a winner, levels searched %s, at most %d candidates, %d differ" % (
        case, len(kp), int(st0.sum()), int((sc0 == -1).sum()), levels, cands, len(bad))
    if len(bad):
        i = bad[0]
        msg += "; first %d at (%r, %r): got %s %d %r, want %s %d %r, trace %s" % (
            i, kp["x"][i], kp["y"][i], xy[i], st[i], sc[i], xy0[i], st0[i], sc0[i], trace[i].tolist())
    print(msg)
    return len(bad)


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_restatement(finder, case):
    import torch
    (left, right), kp, prm, ssd = _case(case)
    xy0, st0, sc0, trace = _reference(case)
    got = run_bm(finder, torch, left, right, kp, prm, ssd)
    assert _report(case, kp, got, (xy0, st0, sc0), trace) == 0
    xy, st, rx, sc = got
    assert xy.tobytes() == xy0.tobytes() and st.tobytes() == st0.tobytes()
    assert rx.tobytes() == np.ascontiguousarray(xy0[:, 0]).tobytes() and sc.tobytes() == sc0.tobytes()


def test_cases_reach_every_path():
    """On the restatement alone: what makes the cases worth running."""
    t = {c: _reference(c) for c in CASES}
    cands = lambda c: max(int((x["lmin"] - x["lmax"]).max()) for x in t[c][3] if len(x))  # noqa: E731
    levels = lambda c: max(len(x) for x in t[c][3])  # noqa: E731
    assert cands("big fast 15x3 l0 128 candidates sad") == 128 and cands("big random 21x5 l0 127 candidates") == 127   # (min_disparity 1: d = 0 is not a candidate)
    assert levels("fast 15x3 l5 ssd") == 4 and levels("big fast 15x3 l5") == 6 and levels("random 15x3 l2") == 3   # 5 is cut by 202 x 170
    for c in ("fast 15x3 l5 ssd", "fast 15x3 l5 sad", "big fast 15x3 l5"):
        st = t[c][1]
        assert st.mean() > 0.8, c                                            # the search does find the planted disparities
    e = t["edges 15x3 l0"]
    first = [x for x in e[3][:8]]                                            # columns hw - 1 ..: window test fails, then the clamp
    assert len(first[0]) == 0 and len(first[1]) == 0 and len(first[2]) == 1 and first[2]["lmin"][0] <= first[2]["lmax"][0]
    assert any(len(x) and (x["lmin"] - x["lmax"])[0] == 32 for x in e[3])    # ... up to the full range
    assert (e[2] == -1).any() and (e[1] == 1).any()
    e5 = t["edges 15x3 l5 min 2.5"][3]
    assert any(len(x) and 0 in x["level"] and 2 not in x["level"] for x in e5)   # inside at level 0, outside at level 2
    assert (t["edges 7x7 l5 no steps sad"][1] == (t["edges 7x7 l5 no steps sad"][2] >= 0)).all()    # no steps: no gate
    tall = t["big 3x341 strip beyond LDS"]
    assert tall[1].sum() > 20 and 341 * (128 + 3) > 32768
    frac_y = t["int x 15x3 l5"]
    assert (frac_y[2][frac_y[1] == 1] >= 0).all()
    rej = t["random 7x7 l2 1 step sad"]
    assert ((rej[1] == 0) & (rej[2] >= 0)).any()                             # the gate inside the loop rejects some


def test_n_zero_one_prefix_optional_outputs_and_defaults(finder):
    import torch
    (left, right), kp, prm, ssd = _case("fast 15x3 l5 ssd")
    xy0, st0, sc0, _ = _reference("fast 15x3 l5 ssd")
    assert len(run_bm(finder, torch, left, right, kp, prm, ssd, n=0)[0]) == 0
    d_l, w, h, pitch = _dev_image(torch, left)
    finder.stereo_block_match_device(d_l.data_ptr(), d_l.data_ptr(), w, h, pitch, None, 0, None, None)   # n = 0 needs no arrays
    for n in (1, 37):
        xy, st, rx, sc = run_bm(finder, torch, left, right, kp, prm, ssd, n=n)
        assert xy.tobytes() == xy0[:n].tobytes() and st.tobytes() == st0[:n].tobytes() and sc.tobytes() == sc0[:n].tobytes()
    xy, st, _, _ = run_bm(finder, torch, left, right, kp, prm, ssd, optional=False)
    assert xy.tobytes() == xy0.tobytes() and st.tobytes() == st0.tobytes()
    # params NULL = sf_stereo_flow_defaults (maximum disparity 128)
    few = kp[:60]
    want = ref.block_match(left, right, few, None, 1)
    xy, st, rx, sc = run_bm(finder, torch, left, right, few, None, 1)
    assert xy.tobytes() == want[0].tobytes() and st.tobytes() == want[1].tobytes() and sc.tobytes() == want[2].tobytes()
    # corners that are not numbers, infinite or far outside: no winner
    odd = kp[:6].copy()
    odd["x"] = [np.nan, np.inf, -np.inf, 3e9, -1e5, 50.0]
    odd["y"] = [10.0, 10.0, np.nan, 10.0, 1e7, np.inf]
    both = np.concatenate([odd, few])
    xy, st, rx, sc = run_bm(finder, torch, left, right, both, None, 1)
    w6 = ref.block_match(left, right, both, None, 1)
    assert xy.tobytes() == w6[0].tobytes() and st.tobytes() == w6[1].tobytes() and sc.tobytes() == w6[2].tobytes()
    assert not st[:6].any() and not xy[:6].any() and (sc[:6] == -1).all()


def test_refusals_change_nothing(finder):
    import torch
    (left, right), kp, prm, ssd = _case("fast 15x3 l5 ssd")
    P = _abi.stereo_flow_params
    nan, inf = float("nan"), float("inf")
    bad = [P(win_width=14), P(win_height=4), P(win_width=0), P(win_width=33, win_height=33), P(min_disparity=nan),
           P(max_disparity=inf), P(min_disparity=-1.0), P(min_disparity=9.0, max_disparity=8.0), P(max_disparity=1025.0)]
    for b in bad:
        with pytest.raises(lib.SepfinderError) as e:
            run_bm(finder, torch, left, right, kp[:5], b, 1)
        assert e.value.code == _abi.SF_EINVAL, str(e.value)
    with pytest.raises(lib.SepfinderError) as e:
        run_bm(finder, torch, left, right, kp[:5], prm, 2)
    assert e.value.code == _abi.SF_EINVAL
    for b in (P(max_level=16), P(max_level=-1)):
        with pytest.raises(lib.SepfinderError):
            run_bm(finder, torch, left, right, kp[:5], b, 1)
    run_bm(finder, torch, left, right, kp[:5], P(max_disparity=1024.5, win_width=1, win_height=1), 1)   # the bounds themselves pass
    # the setters
    assert bytes(finder.stereo_get_params()) == bytes(_abi.stereo_params(1, 1))          # a fresh handle
    finder.stereo_set_params(_abi.stereo_params(0, 0))
    for o, s in ((2, 1), (-1, 0), (0, 2), (1, -1)):
        with pytest.raises(lib.SepfinderError) as e:
            finder.stereo_set_params(_abi.stereo_params(o, s))
        assert e.value.code == _abi.SF_EINVAL
        assert bytes(finder.stereo_get_params()) == bytes(_abi.stereo_params(0, 0))      # a refused call changes nothing


# ---- the extraction calls ----------------------------------------------------------------------------------------------
def chain(f, torch, left, right, cam, det, ftype, flow, ssd, refine=None):
    """detector call -> (cv::cornerSubPix restated) -> block matching RESTATED -> sf_extract_keyframe_device.  Returns
    ((desc, xyz, kpts), slot, the statuses)."""
    dev = torch.device("cuda:0")
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    found = _detect(f, torch, left, ftype, det)
    win, it, eps = refine if refine else (0, 0, 0.0)
    kp = subpix_ref.refine_keypoints(left, found, win, it, eps)
    n, nb = len(kp), f.descriptor_bytes()
    xy, st, _ = ref.block_match(left, right, kp, flow, ssd)
    d_l = torch.from_numpy(left).to(dev)
    d_kp = torch.from_numpy(np.frombuffer(kp.tobytes() + b"\0" * 28, np.uint8).copy()).to(dev)
    d_rx = torch.from_numpy(np.concatenate([xy[:, 0], np.zeros(1, np.float32)])).to(dev)
    d_st = torch.from_numpy(np.concatenate([st, np.zeros(1, np.uint8)])).to(dev)
    desc = torch.zeros((max(n, 1), nb), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((max(n, 1), 3), dtype=torch.float32, device=dev)
    kpo = torch.zeros((max(n, 1), 28), dtype=torch.uint8, device=dev)
    slot, rows = f.extract_keyframe_device(d_l.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), n, cam,
                                           desc.data_ptr(), xyz.data_ptr(), kpo.data_ptr())
    torch.cuda.synchronize()
    out = (desc.cpu().numpy()[:rows], xyz.cpu().numpy()[:rows], np.frombuffer(kpo.cpu().numpy()[:rows].tobytes(), dtype=KP))
    return out, slot, st


FLOW = _abi.stereo_flow_params(max_disparity=48.0)


@pytest.mark.parametrize("ftype,ssd,refine", [(6, 1, None), (6, 0, REFINE), (8, 1, None), (4, 0, None), (2, 1, None)])
def test_host_handlers_equal_the_explicit_chain(finder, ftype, ssd, refine):
    import torch
    left, right = batch_pairs(W, H)[0]
    cam, det = _cam(W, H), _abi.detector_params(300)
    _set_type(finder, ftype)
    want, _, st = chain(finder, torch, left, right, cam, det, ftype, FLOW, ssd, refine)
    lk = finder.get_features_and_descriptor(left, right, cam, det, FLOW)
    finder.stereo_set_params(_abi.stereo_params(0, ssd))
    if refine:
        finder.front_set_params(_abi.front_params(subpix_iterations=refine[1]))
    d, p, k, slot = finder.get_features_and_descriptor(left, right, cam, det, FLOW)
    with_depth = int((~np.isnan(p[:, 2])).sum())
    print("type %d ssd %d refinement %s: %d rows, %d with depth, %d corners matched of %d, %d fractional" % (
        ftype, ssd, refine, len(d), with_depth, int(st.sum()), len(st), int(_fractional(k).sum())))
    assert_same((d, p, k), want)
    assert len(d) > 50 and with_depth > 30 and finder.store_size() == slot + 1            # not vacuous
    assert p.tobytes() != lk[1].tobytes()                                                # and not the LK path's points
    if refine:
        assert _fractional(k).sum() * 4 >= len(k)                                        # fractional corners: the start score is recomputed
    u8 = finder.get_features_and_descriptor_u8(left, right, _abi.SF_IMAGE_MONO8, cam, det, FLOW)
    assert_same(u8[:3], want)
    # NULL flow = the defaults on both sides
    want0, _, _ = chain(finder, torch, left, right, cam, det, ftype, None, ssd, refine)
    assert_same(finder.get_features_and_descriptor(left, right, cam, det)[:3], want0)


def _three_pairs():
    p = batch_pairs(W, H)
    return [p[0], p[2], p[3]]                                                # differing corner counts, a constant pair in the middle


@pytest.mark.parametrize("ftype,ssd", [(6, 1), (8, 0), (4, 1), (2, 0)])
def test_batch_forms_equal_the_single_calls(finder, ftype, ssd):
    import torch
    cam, det = _cam(W, H), _abi.detector_params(200)
    pairs = _three_pairs()
    _set_type(finder, ftype)
    finder.stereo_set_params(_abi.stereo_params(0, ssd))
    call = finder.get_features_and_descriptor_orb_batch_device if ftype == 2 else finder.get_features_and_descriptor_batch_device
    singles = [finder.get_features_and_descriptor(l, r, cam, det, FLOW) for l, r in pairs]
    rows = [len(s[0]) for s in singles]
    print("type %d ssd %d: rows of the single calls %s" % (ftype, ssd, rows))
    assert rows[0] > 50 and rows[1] == 0 and 0 < rows[2] != rows[0]
    want0, _, _ = chain(finder, torch, *pairs[0], cam, det, ftype, FLOW, ssd)
    assert_same(singles[0][:3], want0)
    before = finder.store_size()
    with_flow = lambda *a: call(*a[:9], FLOW, *a[10:])  # noqa: E731  (run_batch passes flow = None: hand the call this flow)
    first, got = run_batch(finder, torch, pairs, W, H, W + 6, (W + 6) * H + 32, cam, det, call=with_flow)
    assert first == before and finder.store_size() == before + 3
    for i, s in enumerate(singles):
        assert_same(got[i], s[:3])
    assert _self_pairs(finder, range(first, first + 3)) == _self_pairs(finder, [s[3] for s in singles])
    # a window block matching refuses: SF_EINVAL, the store as it was
    d_l = torch.zeros((H * W,), dtype=torch.uint8, device="cuda:0")
    size = finder.store_size()
    for bad in (_abi.stereo_flow_params(win_width=14), _abi.stereo_flow_params(max_disparity=2000.0)):
        with pytest.raises(lib.SepfinderError) as e:
            call(d_l.data_ptr(), d_l.data_ptr(), 1, W, H, W, W * H, cam, det, bad)
        assert e.value.code == _abi.SF_EINVAL and finder.store_size() == size
        with pytest.raises(lib.SepfinderError) as e:
            finder.get_features_and_descriptor(*pairs[0], cam, det, bad)
        assert e.value.code == _abi.SF_EINVAL and finder.store_size() == size


@pytest.mark.parametrize("ftype", [6, 2])
def test_u8_batch_equals_the_single_calls(ftype):
    import torch
    dev = torch.device("cuda:0")
    cam, det, maxf = _cam(W, H), _abi.detector_params(200), 200
    gray = _three_pairs()
    pairs = [(colourise(l, 10 + i, RGB8), colourise(r, 20 + i, RGB8)) for i, (l, r) in enumerate(gray)]
    flat = np.empty((H, W, 3), np.uint8)
    flat[...] = (120, 77, 30)
    pairs[1] = (flat, flat)
    pitch, stride = 3 * W + 5, (3 * W + 5) * H + 64

    def packed(images):
        buf = np.full((len(images), stride), 0xA5, np.uint8)
        for i, c in enumerate(images):
            np.lib.stride_tricks.as_strided(buf[i], shape=(H, W, 3), strides=(pitch, 3, 1))[...] = c
        return torch.from_numpy(buf).to(dev)

    d_l, d_r = packed([p[0] for p in pairs]), packed([p[1] for p in pairs])
    f = _finder(torch, w=W, h=H, dims=128)
    try:
        f.netvlad_load(_weights())
        _set_type(f, ftype)
        f.stereo_set_params(_abi.stereo_params(0, 1))
        add = f.add_keyframes_orb_u8_batch_device if ftype == 2 else f.add_keyframes_u8_batch_device
        singles = [f.get_features_and_descriptor_u8(l, r, RGB8, cam, det, FLOW) for l, r in pairs]
        assert len(singles[0][0]) > 50 and len(singles[1][0]) == 0 and len(singles[2][0]) > 0
        # the single call on colour images = the explicit chain on the gray planes of the restated conversion
        want0, _, _ = chain(f, torch, image_ref.gray(pairs[0][0], RGB8, 0), image_ref.gray(pairs[0][1], RGB8, 0), cam, det, ftype, FLOW, 1)
        assert_same(singles[0][:3], want0)
        base = f.store_size()
        # refused: nothing changes, the NN database included
        with pytest.raises(lib.SepfinderError) as e:
            add(d_l.data_ptr(), d_r.data_ptr(), None, RGB8, 3, W, H, pitch, stride, cam, det, _abi.stereo_flow_params(win_height=4))
        assert e.value.code == _abi.SF_EINVAL and f.store_size() == base and f.nn_sizes() == (0, 0)
        rows = torch.full((3,), -7, dtype=torch.int32, device=dev)
        desc = torch.full((3 * maxf, 32), SENTINEL, dtype=torch.uint8, device=dev)
        xyz = torch.full((3 * maxf, 12), SENTINEL, dtype=torch.uint8, device=dev)
        kp = torch.full((3 * maxf, 28), SENTINEL, dtype=torch.uint8, device=dev)
        first, row = add(d_l.data_ptr(), d_r.data_ptr(), None, RGB8, 3, W, H, pitch, stride, cam, det, FLOW, rows.data_ptr(),
                         desc.data_ptr(), xyz.data_ptr(), kp.data_ptr())
        torch.cuda.synchronize()
        assert (first, row) == (base, 0) and f.store_size() == base + 3 and f.nn_sizes() == (3, 0)
        rows, desc, xyz, kp = (t.cpu().numpy() for t in (rows, desc, xyz, kp))
        for i, (d0, p0, k0, _) in enumerate(singles):
            r = int(rows[i])
            blk = slice(i * maxf, i * maxf + r)
            assert r == len(d0), i
            assert_same((desc[blk], np.frombuffer(xyz[blk].tobytes(), np.float32).reshape(r, 3),
                         np.frombuffer(kp[blk].tobytes(), dtype=KP)), (d0, p0, k0))
            assert (kp[i * maxf + r:(i + 1) * maxf] == SENTINEL).all()
        assert _self_pairs(f, range(base, base + 3)) == _self_pairs(f, [s[3] for s in singles])
    finally:
        f.close()


def test_default_path_after_a_round_trip(finder):
    """optical_flow = 1 after block matching ran on the handle (it shares the pyramid buffer with LK): the bytes of an
    untouched handle, single call and batch."""
    import torch
    cam, det = _cam(W, H), _abi.detector_params(200)
    pairs = _three_pairs()
    with lib.SeparatorFinder(_params(w=W, h=H), device=0) as fresh:
        fresh.set_stream(torch.cuda.current_stream().cuda_stream)
        want = [fresh.get_features_and_descriptor(l, r, cam, det) for l, r in pairs]
        _, want_batch = run_batch(fresh, torch, pairs, W, H, W, W * H, cam, det, call=fresh.get_features_and_descriptor_batch_device)
    finder.stereo_set_params(_abi.stereo_params(0, 0))
    bm = finder.get_features_and_descriptor(*pairs[0], cam, det)
    run_batch(finder, torch, pairs, W, H, W, W * H, cam, det, call=finder.get_features_and_descriptor_batch_device)
    assert bm[1].tobytes() != want[0][1].tobytes()
    finder.stereo_set_params(_abi.stereo_params(1, 0))                        # (ssd is not read by the LK path)
    for (l, r), w0 in zip(pairs, want):
        assert_same(finder.get_features_and_descriptor(l, r, cam, det)[:3], w0[:3])
    _, got = run_batch(finder, torch, pairs, W, H, W, W * H, cam, det, call=finder.get_features_and_descriptor_batch_device)
    for g, w0 in zip(got, want_batch):
        assert_same(g, w0)


@pytest.mark.parametrize("estimation_type", [0, 1])
def test_verification_of_block_matched_keyframes(estimation_type):
    """Two keyframes of one scene, the second pair's disparity field shifted (max_disp 40 -> 37), both block matched; the
    oracle runs on the downloaded features."""
    import torch
    from oracle import pyoracle
    h, w = 240, 320
    p = _params(w=w, h=h, estimation_type=estimation_type)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11, local_transform=synth.LOCAL_TRANSFORM)
    det = _abi.detector_params(400)
    with lib.SeparatorFinder(p, device=0) as f:
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        f.stereo_set_params(_abi.stereo_params(0, 1))
        a = f.get_features_and_descriptor(*_pair(w, h, 1, 40.0), cam, det)
        b = f.get_features_and_descriptor(*_pair(w, h, 1, 37.0), cam, det)
        assert (~np.isnan(a[1][:, 2])).sum() > 100 and (~np.isnan(b[1][:, 2])).sum() > 100
        res = f.verify_pairs([a[3]], [b[3]])
        o = pyoracle.estimate_transform(f.params, _abi.FeatureArrays(*a[:3]), _abi.FeatureArrays(*b[:3]))
        print("estimator %d: success gpu %d oracle %d, inliers %d / %d, matches %d / %d" % (
            estimation_type, res[0]["success"], o["success"], res[0]["inliers"], o["inliers"], res[0]["matches"], o["matches"]))
        assert_result_parity(res[0], o, "estimator %d" % estimation_type)
        assert res[0]["success"] == 1 and res[0]["inliers"] > 20
