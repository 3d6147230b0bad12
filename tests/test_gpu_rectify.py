"""GPU: raw camera images rectified on the device (csrc/k_rectify.hip, csrc/sf_rectify.hip) through the C-ABI against the
NumPy restatement tests/rectify_ref.py.  The maps are float64 steps in one written order rounded once to float32, the rest is
integer work: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from multi_robot_slam_separators_amd.data_handler import FinderBackend
from oracle import netvlad_torch
from tests import extract_cases as ec
from tests import image_ref
from tests import rectify_ref as ref
from tests.test_rectify_host import abi_info, refusals

pytestmark = pytest.mark.gpu

RGB8, BGR8, MONO8 = _abi.SF_IMAGE_RGB8, _abi.SF_IMAGE_BGR8, _abi.SF_IMAGE_MONO8
FILL = 0xA5


def _finder(w=320, h=240, dims=128):
    import torch
    p = synth.camera_params()
    p.max_features = 2048
    p.fx, p.fy, p.cx, p.cy = 460.0, 458.0, w / 2.0, h / 2.0
    p.image_width, p.image_height = w, h
    p.netvlad_dimensions = dims
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


@pytest.fixture()
def finder():
    f = _finder()
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def _weights():
    return netvlad_torch.random_weights(3, clusters=64, pca_dim=512)


def channels(fmt):
    return 1 if fmt == MONO8 else 3


@functools.lru_cache(maxsize=None)
def caller_maps(w, h):
    """Caller maps of w x h into a w x h source: the strong plan's own floats with NaN, +-inf, 1e12 and negative fractions
    planted, the kind of table a vendor's tool may hand over."""
    mx, my = (m.copy() for m in ref.maps(ref.case_info("strong", w, h)))
    mx[0:4, 0:9] = np.nan
    my[5:8, 3:20] = np.inf
    mx[9:11, :] = -np.inf
    my[12, 40:60] = 1e12
    mx[13, 1:30] = -1e12
    mx[20:30, 10:50] = -np.linspace(0.01, 1.99, 40, dtype=np.float32)[None, :]
    my[30:40, 60:100] = -np.linspace(0.03, 1.97, 40, dtype=np.float32)[None, :]
    mx[30:40, 60:100] = np.linspace(-1.5, 20.0, 40, dtype=np.float32)[None, :]
    return mx, my


class Plans:
    """The plans of one handle by name, with the restatement's fixed-point maps of each."""

    def __init__(self, f):
        self.f, self.ids, self.fixed, self.sizes = f, {}, {}, {}

    def get(self, key):
        kind, w, h, ow, oh, side = key
        if key not in self.ids:
            if kind == "maps":
                mx, my = caller_maps(w, h)
                self.ids[key] = self.f.rectify_plan_from_maps(mx, my, w, h)
            else:
                info = ref.case_info(kind, w, h, ow, oh, side)
                self.ids[key] = self.f.rectify_plan_create(abi_info(info))
            self.fixed[key] = _fixed(key)
        return self.ids[key]


@functools.lru_cache(maxsize=None)
def _fixed(key):
    kind, w, h, ow, oh, side = key
    if kind == "maps":
        return ref.fixed(*caller_maps(w, h))
    return ref.fixed(*ref.maps(ref.case_info(kind, w, h, ow, oh, side)))


def packed(rng, n, h, row, spare, offset):
    """n images of h rows of `row` random bytes in one buffer: pitch = row + spare, the first image `offset` bytes in."""
    pitch = row + spare
    stride = pitch * h + 13
    buf = rng.integers(0, 256, size=offset + n * stride + 7, dtype=np.uint8)
    return buf, pitch, stride


def run_rectify(f, plans, key_a, key_b, fmt, out_fmt, n, seed, spare=5, offset=1):
    """One sf_image_rectify_device call on random raw images; returns (device destination buffers as host arrays, the
    buffers the restatement expects, with every byte outside the images still at FILL)."""
    import torch
    dev = torch.device("cuda:0")
    _, w, h, ow, oh, _ = key_a
    ow, oh = ow or w, oh or h
    ch, och = channels(fmt), channels(out_fmt)
    rng = np.random.default_rng(seed)
    ids, srcs, d_srcs, d_dsts, wants = [], [], [], [], []
    for key in (key_a, key_b):
        if key is None:
            ids.append(0)
            d_srcs.append(None)
            d_dsts.append(None)
            continue
        ids.append(plans.get(key))
        buf, sp, ss = packed(rng, n, h, ch * w, spare, offset)
        d_srcs.append(torch.from_numpy(buf).to(dev))
        dp = och * ow + spare
        ds = dp * oh + 11
        want = np.full(offset + n * ds + 5, FILL, np.uint8)
        sx, sy = plans.fixed[key]
        for i in range(n):
            img = np.lib.stride_tricks.as_strided(buf[offset + i * ss:], shape=(h, w, ch), strides=(sp, ch, 1))
            rect = ref.remap(img if ch == 3 else img[..., 0], sx, sy)
            if och != ch:
                rect = ref.to_gray(rect, fmt, f.image_get_gray_rule())
            rows = rect.reshape(oh, och * ow)
            for y in range(oh):
                at = offset + i * ds + y * dp
                want[at:at + och * ow] = rows[y]
        wants.append(want)
        d_dsts.append(torch.full((len(want),), FILL, dtype=torch.uint8, device=dev))
        srcs.append(buf)
    f.image_rectify_device(ids[0], d_srcs[0].data_ptr() + offset, ids[1], d_srcs[1].data_ptr() + offset if key_b else None,
                           fmt, out_fmt, n, sp, ss, d_dsts[0].data_ptr() + offset,
                           d_dsts[1].data_ptr() + offset if key_b else None, dp, ds)
    torch.cuda.synchronize()
    gots = [d.cpu().numpy() for d in d_dsts if d is not None]
    for d, s in zip([d for d in d_srcs if d is not None], srcs):
        assert np.array_equal(d.cpu().numpy(), s)                                  # the sources are unchanged
    return gots, wants


# ---- maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["barrel", "rational", "strong"])
@pytest.mark.parametrize("size", [(67, 35, 0, 0), (320, 240, 300, 200)])
def test_maps_equal_the_restatement_bit_for_bit(finder, kind, size):
    import torch
    dev = torch.device("cuda:0")
    w, h, ow, oh = size
    info = ref.case_info(kind, w, h, ow, oh, side=1)
    ow, oh = ref.out_size(info)
    plan = finder.rectify_plan_create(abi_info(info))
    cols = ow + 3                                                                 # a pitch with spare floats
    d = torch.full((2, oh, cols), -7.0, dtype=torch.float32, device=dev)
    finder.rectify_maps_device(plan, d[0].data_ptr(), d[1].data_ptr(), 4 * cols)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    mx, my = ref.maps(info)
    assert got[0, :, :ow].tobytes() == mx.tobytes() and got[1, :, :ow].tobytes() == my.tobytes()
    assert (got[:, :, ow:] == -7.0).all()
    assert np.abs(mx - np.arange(ow)[None, :]).max() > 1.0                        # not an identity


# ---- images ----------------------------------------------------------------------------------------------------------
S, M, L = (67, 35, 0, 0), (320, 240, 0, 0), (752, 480, 0, 0)
IMAGE_CASES = [
    # (format, out_format, plan a, plan b, n_images, gray rule)
    (MONO8, MONO8, ("barrel",) + S + (0,), None, 1, 0),
    (RGB8, RGB8, ("barrel",) + S + (0,), ("rational",) + S + (1,), 3, 0),
    (BGR8, MONO8, ("strong",) + S + (0,), ("barrel",) + S + (1,), 3, 1),
    (RGB8, RGB8, ("strong", 320, 240, 300, 200, 0), ("strong", 320, 240, 300, 200, 1), 3, 0),
    (RGB8, MONO8, ("strong",) + M + (0,), ("rational",) + M + (1,), 1, 0),
    (BGR8, BGR8, ("rational",) + M + (0,), None, 3, 0),
    (MONO8, MONO8, ("strong",) + M + (0,), ("maps",) + M + (0,), 3, 0),
    (RGB8, MONO8, ("maps",) + M + (0,), None, 1, 1),
    (RGB8, MONO8, ("barrel",) + L + (0,), ("barrel",) + L + (1,), 1, 0),
    (BGR8, BGR8, ("strong",) + L + (0,), None, 1, 0),
    (MONO8, MONO8, ("rational",) + L + (0,), ("strong",) + L + (1,), 3, 0),
]


@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("case", range(len(IMAGE_CASES)))
def test_images_equal_the_restatement_and_nothing_else_is_written(finder, case, table):
    fmt, out_fmt, key_a, key_b, n, rule = IMAGE_CASES[case]
    finder.image_set_gray_rule(rule)
    finder.set_option(_abi.SF_OPT_RECTIFY_TABLE, table)          # (plans of caller maps run the table form either way)
    plans = Plans(finder)
    gots, wants = run_rectify(finder, plans, key_a, key_b, fmt, out_fmt, n, seed=100 + case)
    for got, want in zip(gots, wants):
        assert (want != FILL).mean() > 0.5
        assert np.array_equal(got, want), (case, int((got != want).sum()))
    for key in (key_a, key_b):
        if key and key[0] == "strong":                                            # the border path is really exercised
            share = ref.border_share(*plans.fixed[key], key[1], key[2])
            assert 0.05 <= share <= 0.5, share
        if key and key[0] == "maps":
            sx, _ = plans.fixed[key]
            assert (sx == ref.INVALID).sum() > 100 and ((sx < 0) & (sx > -64)).sum() > 100


def test_plans_from_caller_maps_are_kept_apart(finder):
    plans = Plans(finder)
    a, b = plans.get(("maps",) + M + (0,)), plans.get(("strong",) + M + (0,))
    assert (a, b) == (1, 2) and finder.rectify_plan_count() == 2
    info, from_maps = finder.rectify_plan_get(a)
    assert from_maps and (info.width, info.height, info.out_width, info.out_height) == (320, 240, 320, 240) and not any(info.K)
    want = abi_info(ref.case_info("strong", 320, 240))
    info, from_maps = finder.rectify_plan_get(b)
    assert not from_maps and bytes(info) == bytes(want)
    with pytest.raises(lib.SepfinderError) as e:
        finder.rectify_maps_device(a, 16, 16, 4 * 320)                            # (refused before anything is touched)
    assert e.value.code == _abi.SF_EINVAL
    finder.store_clear()
    assert finder.rectify_plan_count() == 2                                       # sf_store_clear keeps the plans
    finder.rectify_plan_clear()
    assert finder.rectify_plan_count() == 0
    assert finder.rectify_plan_create(want) == 1                                  # ids start again
    for i in range(2, _abi.SF_MAX_RECTIFY_PLANS + 1):
        assert finder.rectify_plan_create(want) == i
    with pytest.raises(lib.SepfinderError) as e:
        finder.rectify_plan_create(want)
    assert e.value.code == _abi.SF_ERANGE and finder.rectify_plan_count() == _abi.SF_MAX_RECTIFY_PLANS


# ---- both forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,out_fmt", [(RGB8, RGB8), (RGB8, MONO8), (MONO8, MONO8)])
def test_computed_and_table_forms_write_the_same_bytes(finder, fmt, out_fmt):
    plans = Plans(finder)
    key_a, key_b = ("strong",) + M + (0,), ("strong",) + M + (1,)
    results = []
    for table in (0, 1, 0):
        finder.set_option(_abi.SF_OPT_RECTIFY_TABLE, table)
        gots, wants = run_rectify(finder, plans, key_a, key_b, fmt, out_fmt, 2, seed=7)
        for got, want in zip(gots, wants):
            assert np.array_equal(got, want), table
        results.append(gots)
    assert all(np.array_equal(x, y) for x, y in zip(results[0], results[1]))


# ---- composition -------------------------------------------------------------------------------------------------------
def colourise(gray_image, seed):
    rng = np.random.default_rng(seed)
    g = np.asarray(gray_image, np.int32)
    rgb = np.stack([g + 40, g, g - 50], axis=-1) + rng.integers(-20, 21, size=g.shape + (3,))
    return np.clip(rgb, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def raw_pairs(n, w, h):
    """n raw colour stereo pairs [n, h, w, 3] (left, right): textured images the extraction finds corners in."""
    pairs = [ec.make_stereo_pair(700 + i, width=w, height=h, max_disp=25.0)[:2] for i in range(n)]
    left = np.stack([colourise(p[0], 10 + i) for i, p in enumerate(pairs)])
    right = np.stack([colourise(p[1], 20 + i) for i, p in enumerate(pairs)])
    return left, right


def test_rectified_images_feed_the_batch_calls_on_one_stream():
    import torch
    dev = torch.device("cuda:0")
    n, w, h, maxf, dims = 3, 160, 128, 300, 128
    fa, fb = _finder(w, h), _finder(w, h)
    try:
        for f in (fa, fb):
            f.netvlad_load(_weights())
        il, ir = ref.case_info("barrel", w, h, side=0), ref.case_info("barrel", w, h, side=1)
        cam = lib.stereo_camera_from_info(abi_info(il), abi_info(ir))
        det = _abi.detector_params(maxf)
        left, right = raw_pairs(n, w, h)
        d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        pl, pr = fa.rectify_plan_create(abi_info(il)), fa.rectify_plan_create(abi_info(ir))

        def outputs():
            return (torch.full((n,), -1, dtype=torch.int32, device=dev), torch.zeros((n, maxf, 32), dtype=torch.uint8, device=dev),
                    torch.zeros((n, maxf, 3), dtype=torch.float32, device=dev),
                    torch.zeros((n, maxf, _abi.KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device=dev))
        oa, ob, ga, gb = outputs(), outputs(), outputs(), outputs()
        # handle A: raw -> rectified rgb8 -> keyframes, and raw -> fused gray -> keyframes, nothing waited for in between
        d_rl, d_rr = torch.zeros_like(d_l), torch.zeros_like(d_r)
        d_gl, d_gr = (torch.zeros((n, h, w), dtype=torch.uint8, device=dev) for _ in range(2))
        fa.image_rectify_device(pl, d_l.data_ptr(), pr, d_r.data_ptr(), RGB8, RGB8, n, 3 * w, 3 * w * h, d_rl.data_ptr(),
                                d_rr.data_ptr(), 3 * w, 3 * w * h)
        first, row = fa.add_keyframes_u8_batch_device(d_rl.data_ptr(), d_rr.data_ptr(), d_l.data_ptr(), RGB8, n, w, h, 3 * w,
                                                      3 * w * h, cam, det, None, *(t.data_ptr() for t in oa))
        fa.image_rectify_device(pl, d_l.data_ptr(), pr, d_r.data_ptr(), RGB8, MONO8, n, 3 * w, 3 * w * h, d_gl.data_ptr(),
                                d_gr.data_ptr(), w, w * h)
        first_g = fa.get_features_and_descriptor_batch_device(d_gl.data_ptr(), d_gr.data_ptr(), n, w, h, w, w * h, cam, det, None,
                                                              *(t.data_ptr() for t in ga))
        assert (first, row, first_g) == (0, 0, n)
        # handle B: the restatement's rectified images through the same calls
        sl, sr = ref.fixed(*ref.maps(il)), ref.fixed(*ref.maps(ir))
        rl = np.stack([ref.remap(im, *sl) for im in left])
        rr = np.stack([ref.remap(im, *sr) for im in right])
        assert (rl != left).mean() > 0.3
        d_bl, d_br = torch.from_numpy(rl).to(dev), torch.from_numpy(rr).to(dev)
        assert fb.add_keyframes_u8_batch_device(d_bl.data_ptr(), d_br.data_ptr(), d_l.data_ptr(), RGB8, n, w, h, 3 * w, 3 * w * h,
                                                cam, det, None, *(t.data_ptr() for t in ob)) == (0, 0)
        d_bgl = torch.from_numpy(np.stack([image_ref.gray(im, RGB8, 0) for im in rl])).to(dev)
        d_bgr = torch.from_numpy(np.stack([image_ref.gray(im, RGB8, 0) for im in rr])).to(dev)
        assert fb.get_features_and_descriptor_batch_device(d_bgl.data_ptr(), d_bgr.data_ptr(), n, w, h, w, w * h, cam, det, None,
                                                           *(t.data_ptr() for t in gb)) == n
        torch.cuda.synchronize()
        assert np.array_equal(d_rl.cpu().numpy(), rl) and np.array_equal(d_gr.cpu().numpy(), d_bgr.cpu().numpy())
        rows = ob[0].cpu().numpy()
        print("rows per keyframe", rows.tolist())
        assert rows.sum() > 20
        for xs, ys in ((oa, ob), (ga, gb), (oa, ga)):                              # (the gray route holds the same keyframes)
            for a, b in zip(xs, ys):
                assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        # the store slots, through the keyframe export
        assert fa.store_size() == fb.store_size() == 2 * n
        assert bytes(fa.export_keyframes(0, 2 * n)) == bytes(fb.export_keyframes(0, 2 * n))
        # the NN rows are those of the same d_rgb -- the raw left images, as the reference feeds the network
        assert fa.nn_sizes() == fb.nn_sizes() == (n, 0)
        rng = np.random.default_rng(5)
        recv = rng.normal(size=(4, dims))
        recv /= np.linalg.norm(recv, axis=1, keepdims=True)
        for f in (fa, fb):
            f.nn_append_received(recv)
            f.nn_find_matches()
        (da, ia), (db, ib) = fa.nn_last_row_minima(), fb.nn_last_row_minima()
        assert da.tobytes() == db.tobytes() and ia.tobytes() == ib.tobytes() and len(da) == n
    finally:
        fa.close()
        fb.close()


def test_finder_backend_rectifies_the_raw_pair_first():
    w, h = 320, 240
    fa, fb, fc = _finder(w, h), _finder(w, h), _finder(w, h)
    try:
        il, ir = ref.case_info("barrel", w, h, side=0), ref.case_info("barrel", w, h, side=1)
        cam = lib.stereo_camera_from_info(abi_info(il), abi_info(ir))
        det = _abi.detector_params(300)
        gl, gr, _ = ec.make_stereo_pair(21, width=w, height=h, max_disp=40.0)
        left, right = colourise(gl, 3), colourise(gr, 4)
        plans = (fa.rectify_plan_create(abi_info(il)), fa.rectify_plan_create(abi_info(ir)))
        got = FinderBackend(fa, cam, det, rectify=plans).get_features_u8(left, right, RGB8)
        rl, rr = ref.rectify(left, il), ref.rectify(right, ir)
        want = FinderBackend(fb, cam, det).get_features_u8(rl, rr, RGB8)
        assert len(want[0]) > 20
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        # off by default: the call of the class as it was
        plain = FinderBackend(fc, cam, det).get_features_u8(left, right, RGB8)
        direct = fb.get_features_and_descriptor_u8(left, right, RGB8, cam, det)[:3]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, direct))
        assert plain[0].tobytes() != got[0].tobytes()
    finally:
        for f in (fa, fb, fc):
            f.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _refused(call, codes=(_abi.SF_EINVAL,)):
    with pytest.raises(lib.SepfinderError) as e:
        call()
    assert e.value.code in codes, str(e.value)
    assert len(str(e.value).split(": ", 1)[1]) > 10, str(e.value)
    return str(e.value)


def test_refusals_touch_nothing(finder):
    import torch
    dev = torch.device("cuda:0")
    w, h = 67, 35
    good = finder.rectify_plan_create(abi_info(ref.case_info("barrel", w, h)))
    other = finder.rectify_plan_create(abi_info(ref.case_info("barrel", w, h, 60, 30)))
    # every block the restatement refuses, through the call itself: SF_EINVAL, and the table is as it was
    for name, block, _ in refusals():
        pid = C.c_int32(-5)
        assert finder._L.sf_rectify_plan_create(finder._h, C.byref(block), C.byref(pid)) == _abi.SF_EINVAL, name
        assert len(finder._L.sf_last_error(finder._h)) > 10 and pid.value == -5 and finder.rectify_plan_count() == 2, name
    src = torch.zeros((2, h, 3 * w), dtype=torch.uint8, device=dev)
    dst = torch.full((2, h, 3 * w), FILL, dtype=torch.uint8, device=dev)
    s, d = src.data_ptr(), dst.data_ptr()

    def call(pa=good, pb=good, fmt=RGB8, out=RGB8, n=1, sp=3 * w, dp=3 * w, sb=s, db=d):
        finder.image_rectify_device(pa, s, pb, sb, fmt, out, n, sp, 3 * w * h, d, db, dp, 3 * w * h)
    _refused(lambda: call(pa=0))                                                  # plan ids outside the table
    _refused(lambda: call(pa=3))
    _refused(lambda: call(pb=-1))
    _refused(lambda: call(pb=other))                                              # plans of unlike sizes
    _refused(lambda: call(fmt=MONO8, out=MONO8 + 1))                              # unknown output format
    _refused(lambda: call(fmt=MONO8, out=RGB8, sp=w))                             # rgb8 from mono8
    _refused(lambda: call(fmt=RGB8, out=BGR8))                                    # a colour format from the other one
    _refused(lambda: call(fmt=3, out=3))
    _refused(lambda: call(sp=3 * w - 1))                                          # a pitch below a row
    _refused(lambda: call(dp=3 * w - 1))
    _refused(lambda: call(out=MONO8, dp=w - 1))
    _refused(lambda: call(db=None))                                               # a second source without a destination
    _refused(lambda: call(n=2, sp=3 * w + 1))                                     # a stride below an image
    _refused(lambda: finder.rectify_plan_get(3))
    _refused(lambda: finder.rectify_maps_device(good, s, s, 4 * w - 4))
    mx = np.zeros((4, 4), np.float32)
    _refused(lambda: finder.rectify_plan_from_maps(mx, mx, 0, 5))
    _refused(lambda: finder.rectify_plan_from_maps(mx, mx, 5, 8193))
    call(n=0)                                                                     # SF_OK, nothing launched
    call(n=0, sp=0, dp=0)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all() and finder.rectify_plan_count() == 2
    # gray from mono8 is mono8 itself: out_format = format, accepted
    call(fmt=MONO8, out=MONO8, sp=w, dp=w)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() != FILL).any()
