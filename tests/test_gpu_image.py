"""GPU: keyframes from the camera's rgb8 / bgr8 / mono8 images (csrc/k_image.hip, the uint8 form of k_conv3x3_first in
csrc/k_cnn.hip) through the C-ABI against the NumPy restatement tests/image_ref.py and against the parent's path -- the
restatement's gray planes and float images through the MONO8 / float32 calls.  Everything here is integer work or the
same float code on the same values, so every comparison is exact."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib, synth
from oracle import netvlad_torch
from tests import extract_cases as ec
from tests import image_ref as ref

pytestmark = pytest.mark.gpu

RGB8, BGR8, MONO8 = _abi.SF_IMAGE_RGB8, _abi.SF_IMAGE_BGR8, _abi.SF_IMAGE_MONO8


def _params(w=320, h=240, dims=128):
    p = synth.camera_params()
    p.max_features = 2048
    p.fx, p.fy, p.cx, p.cy = 460.0, 458.0, w / 2.0, h / 2.0
    p.image_width, p.image_height = w, h
    p.netvlad_dimensions = dims
    return p


def _finder(torch, **kw):
    f = lib.SeparatorFinder(_params(**kw), device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


@pytest.fixture()
def finder():
    import torch
    f = _finder(torch)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def _weights():
    return netvlad_torch.random_weights(3, clusters=64, pca_dim=512)


@pytest.fixture(scope="module")
def model():
    import torch
    f = _finder(torch)
    f.netvlad_load(_weights())
    yield f
    f.close()


def colourise(gray_image, seed, format=RGB8, pad=5):
    """A colour image [h, w, 3] (a view with `pad` spare bytes per row) whose structure is the gray image's: the channels
    are the image shifted apart plus noise of their own, so that no channel is the gray plane."""
    rng = np.random.default_rng(seed)
    g = np.asarray(gray_image, np.int32)
    rgb = np.stack([g + 40, g, g - 50], axis=-1) + rng.integers(-20, 21, size=g.shape + (3,))
    rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    want = ref.gray(rgb, RGB8, 0)
    for ch in range(3):
        assert (want != rgb[..., ch]).mean() > 0.5            # the gray plane is none of the channels
    h, w = g.shape
    buf = np.full((h, 3 * w + pad), 0xA5, np.uint8)
    view = buf[:, :3 * w].reshape(h, w, 3)
    view[...] = rgb[..., ::-1] if format == BGR8 else rgb
    return view


# ---- gray, exhaustive ----------------------------------------------------------------------------------------------
def test_gray_of_every_triple_equals_the_restatement(finder):
    import torch
    dev = torch.device("cuda:0")
    triples = np.ascontiguousarray(np.arange(1 << 24, dtype=np.uint32).view(np.uint8).reshape(-1, 4)[:, :3])   # all 2^24
    img = triples.reshape(4096, 4096, 3)
    d_src = torch.from_numpy(img).to(dev)
    d_dst = torch.zeros((4096, 4096), dtype=torch.uint8, device=dev)
    for rule, format in ((0, RGB8), (1, RGB8), (0, BGR8), (1, BGR8)):
        finder.image_set_gray_rule(rule)
        assert finder.image_get_gray_rule() == rule
        d_dst.zero_()
        finder.image_to_gray_device(d_src.data_ptr(), format, 4096, 4096, 3 * 4096, 0, 1, d_dst.data_ptr(), 4096, 0)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        want = ref.gray(img, format, rule)
        assert np.array_equal(got, want), (rule, format, int((got != want).sum()))
    assert torch.equal(d_src.cpu(), torch.from_numpy(img))


# ---- gray, layout --------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 5, 15, 16, 17, 31, 33, 131)


@pytest.mark.parametrize("n_images", [1, 3])
@pytest.mark.parametrize("format", [RGB8, BGR8, MONO8])
def test_gray_layouts_write_the_planes_and_nothing_else(finder, format, n_images):
    import torch
    dev = torch.device("cuda:0")
    ch = 1 if format == MONO8 else 3
    rng = np.random.default_rng(10 * format + n_images)
    combos = 0
    for w in WIDTHS:
        for h in (1, 3):
            for sp in (ch * w, ch * w + 1, ch * w + 7):
                for dp in (w, w + 3):
                    s_stride, d_stride = sp * h + 5, dp * h + 9          # slack in both strides
                    src = rng.integers(0, 256, size=3 + n_images * s_stride, dtype=np.uint8)
                    d_src_all = torch.from_numpy(src).to(dev)
                    imgs = [[np.lib.stride_tricks.as_strided(src[so + i * s_stride:], shape=(h, w, ch), strides=(sp, ch, 1))
                             for i in range(n_images)] for so in range(4)]
                    for so in range(4):
                        for do in range(4):
                            rule = combos & 1
                            combos += 1
                            finder.image_set_gray_rule(rule)
                            d_dst_all = torch.full((3 + n_images * d_stride + 16,), 0xEE, dtype=torch.uint8, device=dev)
                            d_src, d_dst = d_src_all[so:], d_dst_all[do:]
                            finder.image_to_gray_device(d_src.data_ptr(), format, w, h, sp, s_stride, n_images,
                                                        d_dst.data_ptr(), dp, d_stride)
                            got = d_dst_all.cpu().numpy()
                            want = np.full_like(got, 0xEE)
                            for i in range(n_images):
                                plane = ref.gray(imgs[so][i] if ch == 3 else imgs[so][i][..., 0], format, rule)
                                for y in range(h):
                                    at = do + i * d_stride + y * dp
                                    want[at:at + w] = plane[y]
                            assert np.array_equal(got, want), (w, h, sp, dp, so, do, rule)
                    assert np.array_equal(d_src_all.cpu().numpy(), src), (w, h, sp)           # the source is unchanged
    assert combos == len(WIDTHS) * 2 * 3 * 2 * 16


# ---- NetVLAD from uint8 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 48), (120, 160), (128, 160)])
def test_netvlad_from_uint8_carries_the_bits_of_the_float_call(model, shape):
    import torch
    dev = torch.device("cuda:0")
    h, w = shape
    rng = np.random.default_rng(h)
    for n_img in (1, 3, 5):                                   # a single image, a stacked group, a group split of 4 + 1
        for format in (RGB8, BGR8, MONO8):
            ch = 1 if format == MONO8 else 3
            pitch = ch * w + 5
            stride = pitch * h + 11
            buf = rng.integers(0, 256, size=n_img * stride, dtype=np.uint8)
            imgs = [np.lib.stride_tricks.as_strided(buf[i * stride:], shape=(h, w, ch), strides=(pitch, ch, 1)) for i in range(n_img)]
            floats = np.stack([ref.netvlad_input(im if ch == 3 else im[..., 0], format) for im in imgs])
            d_f = torch.from_numpy(floats).to(dev)
            want = torch.zeros((n_img, 128), dtype=torch.float32, device=dev)
            model.netvlad_infer_batch_device(d_f.data_ptr(), n_img, w, h, want.data_ptr(), 128)
            d_u8 = torch.from_numpy(buf).to(dev)
            got = torch.full((n_img, 128), -7.0, dtype=torch.float32, device=dev)
            model.netvlad_infer_u8_batch_device(d_u8.data_ptr(), format, n_img, w, h, pitch, stride, got.data_ptr(), 128)
            torch.cuda.synchronize()
            got, want = got.cpu().numpy(), want.cpu().numpy()
            assert np.isfinite(want).all() and (np.linalg.norm(want, axis=1) > 0.05).all()
            assert np.array_equal(got, want), (shape, n_img, format, float(np.abs(got - want).max()))
    # the host helper: the same bits from host images
    got = model.netvlad_u8([np.ascontiguousarray(im) for im in imgs], MONO8 if ch == 1 else format, 128)
    assert np.array_equal(got, want)


# ---- features from colour ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _colour_cases():
    a = ec.make_case(13, n=1, width=131, height=97, pad=3)[0]
    a_right = np.roll(a, -4, axis=1)
    bl, br, _ = ec.make_stereo_pair(21, width=320, height=240, max_disp=40.0)
    return ((colourise(a, 1, RGB8, pad=3), colourise(a_right, 2, RGB8, pad=3), RGB8, (131, 97)),
            (colourise(bl, 3, BGR8), colourise(br, 4, BGR8), BGR8, (320, 240)))


def _select(f, ft):
    if ft == 2:
        f.set_feature_type_orb()
    else:
        f.set_feature_type(ft)


@pytest.mark.parametrize("ft,rule", [(6, 0), (8, 0), (4, 0), (2, 0), (6, 1)])
def test_features_from_colour_equal_features_from_the_gray_planes(ft, rule):
    import torch
    fa, fb = _finder(torch), _finder(torch)
    try:
        _select(fa, ft)
        _select(fb, ft)
        fa.image_set_gray_rule(rule)
        total = 0
        for left, right, format, (w, h) in _colour_cases():
            cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
            det = _abi.detector_params(300)
            gl, gr = ref.gray(left, format, rule), ref.gray(right, format, rule)
            if rule == 1:
                assert (gl != ref.gray(left, format, 0)).any()
            da, pa, ka, sa = fa.get_features_and_descriptor_u8(left, right, format, cam, det)
            db, pb, kb, sb = fb.get_features_and_descriptor(gl, gr, cam, det)
            print("type %d rule %d %dx%d: %d rows" % (ft, rule, w, h, len(db)))
            assert sa == sb and len(da) == len(db)
            assert da.tobytes() == db.tobytes() and pa.tobytes() == pb.tobytes() and ka.tobytes() == kb.tobytes()
            total += len(db)
            if w == 320:
                assert len(db) > 20
        assert total > 20 and fa.store_size() == fb.store_size() == 2
    finally:
        fa.close()
        fb.close()


def test_mono8_camera_images_and_verification_of_ingested_slots():
    """Two keyframes from colour on one handle, from the restatement's gray planes on another: sf_verify_pairs on the two
    slots gives the same record; and mono8 through the camera call is the MONO8 call."""
    import torch
    fa, fb = _finder(torch), _finder(torch)
    try:
        left, right, format, (w, h) = _colour_cases()[1]
        cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
        gl, gr = ref.gray(left, format, 0), ref.gray(right, format, 0)
        sa = [fa.get_features_and_descriptor_u8(left, right, format, cam)[3] for _ in range(2)]
        sb = [fb.get_features_and_descriptor(gl, gr, cam)[3] for _ in range(2)]
        ra, rb = fa.verify_pairs([sa[0]], [sa[1]]), fb.verify_pairs([sb[0]], [sb[1]])
        assert ra.tobytes() == rb.tobytes() and ra[0]["success"] and ra[0]["inliers"] > 20
        m = fa.get_features_and_descriptor_u8(gl, gr, MONO8, cam)
        g = fb.get_features_and_descriptor(gl, gr, cam)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(m[:3], g[:3])) and len(m[0]) > 20
    finally:
        fa.close()
        fb.close()


# ---- batch ingestion -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_rgb", [False, True])
def test_batch_ingestion_equals_gray_batch_plus_float_netvlad(own_rgb):
    import torch
    dev = torch.device("cuda:0")
    n, w, h, maxf, dims = 3, 160, 128, 300, 128
    fa, fb = _finder(torch, w=w, h=h), _finder(torch, w=w, h=h)
    try:
        for f in (fa, fb):
            f.netvlad_load(_weights())
        cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
        det = _abi.detector_params(maxf)
        pairs = [ec.make_stereo_pair(700 + i, width=w, height=h, max_disp=25.0)[:2] for i in range(n)]
        # both handles already hold one keyframe: a store slot and a local row
        rng = np.random.default_rng(5)
        row0 = rng.normal(size=(1, dims))
        row0 /= np.linalg.norm(row0)
        for f in (fa, fb):
            f.get_features_and_descriptor(pairs[0][0], pairs[0][1], cam, det)
            f.nn_append_local(row0)
        pitch = 3 * w + 5
        stride = pitch * h + 64

        def pack(images, seed0):
            buf = np.zeros((n, stride), np.uint8)
            views = []
            for i, g in enumerate(images):
                c = colourise(g, seed0 + i, RGB8)
                v = np.lib.stride_tricks.as_strided(buf[i], shape=(h, w, 3), strides=(pitch, 3, 1))
                v[...] = c
                views.append(v)
            return buf, views
        bl, vl = pack([p[0] for p in pairs], 10)
        br, vr = pack([p[1] for p in pairs], 20)
        bc, vc = pack([p[1][::-1] for p in pairs], 30) if own_rgb else (bl, vl)      # the colour camera sees something else
        d_l, d_r, d_c = (torch.from_numpy(b).to(dev) for b in (bl, br, bc))

        def outputs():
            return (torch.full((n,), -1, dtype=torch.int32, device=dev), torch.zeros((n, maxf, 32), dtype=torch.uint8, device=dev),
                    torch.zeros((n, maxf, 3), dtype=torch.float32, device=dev),
                    torch.zeros((n, maxf, _abi.KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device=dev))
        oa, ob = outputs(), outputs()
        # handle A: the one call
        first, row = fa.add_keyframes_u8_batch_device(d_l.data_ptr(), d_r.data_ptr(), d_c.data_ptr() if own_rgb else None, RGB8,
                                                      n, w, h, pitch, stride, cam, det, None, *(t.data_ptr() for t in oa))
        assert (first, row) == (1, 1) and fa.store_size() == 1 + n and fa.nn_sizes() == (1 + n, 0)
        # handle B: the restatement's planes and float images through the parent's calls
        gl = torch.from_numpy(np.stack([ref.gray(v, RGB8, 0) for v in vl])).to(dev)
        gr = torch.from_numpy(np.stack([ref.gray(v, RGB8, 0) for v in vr])).to(dev)
        assert fb.get_features_and_descriptor_batch_device(gl.data_ptr(), gr.data_ptr(), n, w, h, w, w * h, cam, det, None,
                                                           *(t.data_ptr() for t in ob)) == 1
        d_f = torch.from_numpy(np.stack([ref.netvlad_input(v, RGB8) for v in vc])).to(dev)
        d_desc = torch.zeros((n, dims), dtype=torch.float32, device=dev)
        fb.netvlad_infer_batch_device(d_f.data_ptr(), n, w, h, d_desc.data_ptr(), dims)
        fb.nn_append_local_device(d_desc.data_ptr(), n, dims)
        torch.cuda.synchronize()
        assert fb.store_size() == 1 + n and fb.nn_sizes() == (1 + n, 0)
        rows = ob[0].cpu().numpy()
        assert (rows > 20).all()
        for a, b in zip(oa, ob):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        # the same received rows on both: the queries agree, and find the keyframes of the batch
        desc = d_desc.cpu().numpy().astype(np.float64)
        recv = desc + 1e-5 * rng.normal(size=(n, dims))
        for f in (fa, fb):
            f.nn_append_received(recv)
        ma, mb = fa.nn_find_matches(), fb.nn_find_matches()
        assert ma.tobytes() == mb.tobytes() and len(ma) >= 1
        apart = min(np.linalg.norm(desc[i] - desc[j]) for i in range(n) for j in range(i))
        print("descriptors of different keyframes are at least %.3g apart" % apart)
        if apart > 1e-3:                                                              # (random weights decide this)
            assert sorted(ma["idx_local"].tolist()) == [1, 2, 3]
            assert all(int(m["idx_other"]) == int(m["idx_local"]) - 1 for m in ma)    # local row first_row + i <-> keyframe i
        (da, ia), (db, ib) = fa.nn_last_row_minima(), fb.nn_last_row_minima()
        assert da.tobytes() == db.tobytes() and ia.tobytes() == ib.tobytes()
        # slot first_slot + i holds keyframe i on both handles
        ra = fa.verify_pairs([first + i for i in range(n)], [first + i for i in range(n)])
        rb = fb.verify_pairs([1 + i for i in range(n)], [1 + i for i in range(n)])
        assert ra.tobytes() == rb.tobytes()
    finally:
        fa.close()
        fb.close()


# ---- refusals ------------------------------------------------------------------------------------------------------
def _refused(call, codes=(_abi.SF_EINVAL,)):
    with pytest.raises(lib.SepfinderError) as e:
        call()
    assert e.value.code in codes, str(e.value)
    assert len(str(e.value).split(": ", 1)[1]) > 10, str(e.value)               # with a message
    return str(e.value)


def test_refusals_change_nothing(model):
    import torch
    dev = torch.device("cuda:0")
    w, h = 64, 48
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    img = torch.zeros((4, h, 3 * w), dtype=torch.uint8, device=dev)
    out = torch.zeros((4, h, w), dtype=torch.float32, device=dev)
    host = np.zeros((h, w, 3), np.uint8)
    p, o = img.data_ptr(), out.data_ptr()
    plain = _finder(torch)                                                     # no model loaded
    wide = _finder(torch, dims=1024)                                           # more dimensions than the model has
    try:
        wide.netvlad_load(_weights())
        for f in (model, plain, wide):
            state = (f.store_size(), f.nn_sizes(), f.get_feature_type()[0], f.image_get_gray_rule())
            add = lambda fmt=RGB8, l=p, r=p, pitch=3 * w, n=2, f=f: f.add_keyframes_u8_batch_device(   # noqa: E731
                l, r, None, fmt, n, w, h, pitch, 3 * w * h, cam)
            # unknown format, unknown rule
            _refused(lambda: f.image_to_gray_device(p, 3, w, h, 3 * w, 0, 1, o, w, 0))
            _refused(lambda: f.netvlad_infer_u8_batch_device(p, 7, 1, w, h, 3 * w, 0, o, 16))
            _refused(lambda: f.get_features_and_descriptor_u8(host, host, -1, cam))
            _refused(lambda: add(fmt=3))
            _refused(lambda: f.image_set_gray_rule(2))
            _refused(lambda: f.image_set_gray_rule(-1))
            # a pitch below a row of pixels
            _refused(lambda: f.image_to_gray_device(p, RGB8, w, h, 3 * w - 1, 0, 1, o, w, 0))
            _refused(lambda: f.image_to_gray_device(p, RGB8, w, h, 3 * w, 0, 1, o, w - 1, 0))
            _refused(lambda: f.netvlad_infer_u8_batch_device(p, BGR8, 1, w, h, 3 * w - 1, 0, o, 16))
            _refused(lambda: add(pitch=3 * w - 1))
            rows, slot = lib.C.c_int32(), lib.C.c_int32()
            assert f._L.sf_get_features_and_descriptor_u8(f._h, host.ctypes.data, host.ctypes.data, RGB8, w, h, 3 * w - 1,
                                                          lib.C.byref(cam), None, None, None, None, None, 0, lib.C.byref(rows),
                                                          lib.C.byref(slot)) == _abi.SF_EINVAL
            assert len(f._L.sf_last_error(f._h)) > 10
            # missing pointers
            _refused(lambda: f.image_to_gray_device(None, RGB8, w, h, 3 * w, 0, 1, o, w, 0))
            _refused(lambda: f.image_to_gray_device(p, RGB8, w, h, 3 * w, 0, 1, None, w, 0))
            _refused(lambda: f.netvlad_infer_u8_batch_device(None, RGB8, 1, w, h, 3 * w, 0, o, 16))
            _refused(lambda: add(r=None))
            _refused(lambda: add(l=None))
            # the batch form's own refusal of feature type 2: the gray call's code and message
            f.set_feature_type_orb()
            gray_msg = _refused(lambda: f.get_features_and_descriptor_batch_device(p, p, 2, w, h, w, w * h, cam))
            assert _refused(add) == gray_msg
            f.set_feature_type(state[2])
            assert (f.store_size(), f.nn_sizes(), f.get_feature_type()[0], f.image_get_gray_rule()) == state
        # no model loaded
        assert "model" in _refused(lambda: plain.add_keyframes_u8_batch_device(p, p, None, RGB8, 2, w, h, 3 * w, 3 * w * h, cam))
        assert "model" in _refused(lambda: plain.netvlad_infer_u8_batch_device(p, RGB8, 1, w, h, 3 * w, 0, o, 16))
        # netvlad_dimensions above the model's width
        assert "1024" in _refused(lambda: wide.add_keyframes_u8_batch_device(p, p, None, RGB8, 2, w, h, 3 * w, 3 * w * h, cam))
        # the float call's limits, with its codes
        _refused(lambda: model.netvlad_infer_u8_batch_device(p, RGB8, 1, w, h, 3 * w, 0, o, 4096), (_abi.SF_ERANGE,))
        _refused(lambda: model.netvlad_infer_u8_batch_device(p, RGB8, 1, 8, 8, 24, 0, o, 16), (_abi.SF_ERANGE,))
        for f in (model, plain, wide):
            assert f.store_size() == 0 and f.nn_sizes() == (0, 0)
        # and the calls the refusals stood in front of do run
        first, row = model.add_keyframes_u8_batch_device(p, p, None, RGB8, 2, w, h, 3 * w, 3 * w * h, cam)
        torch.cuda.synchronize()
        assert (first, row) == (0, 0) and model.store_size() == 2 and model.nn_sizes() == (2, 0)
        model.store_clear()
        model.nn_reset()
    finally:
        plain.close()
        wide.close()
