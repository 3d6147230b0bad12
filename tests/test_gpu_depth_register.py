"""GPU: depth registration (sf_depth_register_device, sf_depth_fill_holes_device; csrc/k_depth_register.hip), byte for byte
against the NumPy restatement tests/depth_register_ref.py on buffers prefilled with a sentinel, so that the bytes outside the
planes are compared too: the seeded scenes of ref.CASES in both formats under every combination of fill flags, one image and
three, aligned planes (the 8- and 16-byte loads and stores) and odd pitches with bases off by one element (the element-wise
ones); the planted cases of the host test; the same call twice; the fill alone against the fused call; a batch in several
chunks; the composition with the depth keyframe batch call; n_images = 0 and the refusals.  Every test calls a symbol the
library did not have before sf_depth_register_device."""
import functools

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi, lib
from tests import depth_ref as dref
from tests import depth_register_ref as ref
from tests import test_depth_register_host as host
from tests import test_gpu_depth as gd

pytestmark = pytest.mark.gpu

SENTINEL = gd.SENTINEL
FMT = {"u16": ref.U16, "f32": ref.F32M}
CASES = {c[0]: c for c in ref.CASES}
FILLS = {"00": (0, 0), "10": (1, 0), "01": (0, 1), "11": (1, 1)}
# (case, fill) of the comparison: every case under every combination of flags (every scene meets the fill's conditions: the
# host test)
CASE_FILLS = [(c[0], fill) for c in ref.CASES for fill in FILLS]
# the layouts: (input padding in elements, output padding, offset of both bases in elements, extra elements between planes)
ALIGNED, ODD = (0, 0, 0, 0), (5, 3, 1, 9)


@pytest.fixture(scope="module")
def finder():
    f = gd._finder()
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def scenes(case, fmt):
    return tuple(ref.case_scene(case, seed, FMT[fmt]) for seed in ref.SEEDS)


@functools.lru_cache(maxsize=None)
def unfilled(case, fmt):
    """The restated registration of the case's three scenes before the fill: computed once, shared, never changed."""
    name, dw, dh, W, H, _ = CASES[case]
    out = tuple(ref.register_unfilled(d, ref.case_registration(dw, dh, W, H)) for d in scenes(case, fmt))
    for a in out:
        a.setflags(write=False)
    return out


def pack(torch, planes, pitch, stride, offset):
    """n 2-D arrays of one shape as one device buffer: the first element `offset` bytes in, rows `pitch` and planes `stride`
    bytes apart; everything else 0xA5."""
    h, w = planes[0].shape
    elem = planes[0].itemsize
    buf = np.full(offset + len(planes) * stride + 8 * elem, 0xA5, np.uint8)
    for i, p in enumerate(planes):
        at = offset + i * stride
        np.lib.stride_tricks.as_strided(buf[at:at + pitch * h].view(p.dtype), shape=(h, w), strides=(pitch, elem))[...] = p
    return torch.from_numpy(buf).to("cuda:0")


def expected(length, planes, pitch, stride, offset):
    want = np.full(length, SENTINEL, np.uint8)
    h, w = planes[0].shape
    elem = planes[0].itemsize
    for i, p in enumerate(planes):
        at = offset + i * stride
        np.lib.stride_tricks.as_strided(want[at:at + pitch * h].view(p.dtype), shape=(h, w), strides=(pitch, elem))[...] = p
    return want


def geometry(w_in, h_in, w_out, h_out, elem, layout):
    in_pad, out_pad, off, gap = layout
    pitch, out_pitch = (w_in + in_pad) * elem, (w_out + out_pad) * elem
    return pitch, pitch * h_in + gap * elem, out_pitch, out_pitch * h_out + 2 * gap * elem, off * elem


def register(f, torch, planes, reg, layout=ALIGNED):
    """sf_depth_register_device on the planes under a layout: (the whole output buffer as bytes, what it should hold given the
    expected planes -> bytes)."""
    n, elem = len(planes), planes[0].itemsize
    pitch, stride, out_pitch, out_stride, off = geometry(reg["dw"], reg["dh"], reg["W"], reg["H"], elem, layout)
    d_in = pack(torch, planes, pitch, stride, off)
    d_out = torch.full((off + n * out_stride + 8 * elem,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    f.depth_register_device(ref.abi(reg), d_in.data_ptr() + off, _abi.depth_format_of(planes[0]), pitch, stride, n,
                            d_out.data_ptr() + off, out_pitch, out_stride)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    return got, lambda want_planes: expected(len(got), want_planes, out_pitch, out_stride, off)


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return None if len(bad) == 0 else (int(bad[0]), len(bad), got[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- the registration against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("case,fill", CASE_FILLS, ids=lambda v: str(v))
def test_register_equals_restatement(finder, case, fill, fmt, n):
    import torch
    name, dw, dh, W, H, _ = CASES[case]
    fv, fh = FILLS[fill]
    reg = ref.case_registration(dw, dh, W, H, fv, fh)
    planes = scenes(case, fmt)[:n]
    want = [ref.fill_holes(a, fv, fh) for a in unfilled(case, fmt)[:n]]
    assert all(w.any() for w in want) and (n == 1 or want[0].tobytes() != want[2].tobytes())
    for layout in (ALIGNED, ODD):                           # (at an odd width neither has aligned rows)
        got, layout_of = register(finder, torch, planes, reg, layout)
        assert first_difference(got, layout_of(want)) is None, layout     # the images, and nothing outside them


@pytest.mark.parametrize("fmt", list(FMT))
def test_one_image_ignores_the_strides(finder, fmt):
    import torch
    name, dw, dh, W, H, _ = CASES["64x48_96x72"]
    reg = ref.case_registration(dw, dh, W, H, 1, 1)
    plane = scenes(name, fmt)[1]
    elem = plane.itemsize
    d_in = pack(torch, [plane], dw * elem, dw * dh * elem, 0)
    d_out = torch.full((H, W * elem), SENTINEL, dtype=torch.uint8, device="cuda:0")
    finder.depth_register_device(ref.abi(reg), d_in.data_ptr(), FMT[fmt], dw * elem, 3, 1, d_out.data_ptr(), W * elem, 1)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == ref.fill_holes(unfilled(name, fmt)[1], 1, 1).tobytes()


def test_planted_cases_on_the_device(finder):
    import torch
    for name, d, reg, want in host.planted_cases():
        restated = ref.register(d, reg)
        assert want is None or restated.tobytes() == want.tobytes(), name
        for layout in (ALIGNED, ODD):
            got, layout_of = register(finder, torch, [d], reg, layout)
            assert first_difference(got, layout_of([restated])) is None, (name, layout)


@pytest.mark.parametrize("fmt", list(FMT))
def test_the_same_call_twice_gives_the_same_bytes(finder, fmt):
    import torch
    name, dw, dh, W, H, _ = CASES["96x64_48x32"]            # nearly every pixel collides: the order of arrival differs
    reg = ref.case_registration(dw, dh, W, H)
    first, _ = register(finder, torch, scenes(name, fmt), reg)
    second, _ = register(finder, torch, scenes(name, fmt), reg)
    assert first.tobytes() == second.tobytes()


def test_the_host_convenience_uploads_runs_and_downloads(finder):
    name, dw, dh, W, H, _ = CASES["67x45_93x71"]
    reg = ref.case_registration(dw, dh, W, H, 1, 1)
    for fmt in FMT:
        out = finder.depth_register(scenes(name, fmt)[0], ref.abi(reg))
        want = ref.fill_holes(unfilled(name, fmt)[0], 1, 1)
        assert out.dtype == want.dtype and out.shape == want.shape and out.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        finder.depth_register(np.zeros((dh + 1, dw), np.uint16), ref.abi(reg))


# ---- the fill alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("case", [c[0] for c in ref.CASES])
def test_fill_alone_on_the_unfilled_result_equals_the_fused_call(finder, case, fmt):
    import torch
    name, dw, dh, W, H, _ = CASES[case]
    n, elem = 3, 2 if fmt == "u16" else 4
    planes = scenes(case, fmt)
    for layout in (ALIGNED, ODD):
        plain, plain_of = register(finder, torch, planes, ref.case_registration(dw, dh, W, H), layout)
        assert first_difference(plain, plain_of(list(unfilled(case, fmt)))) is None
        _, _, out_pitch, out_stride, off = geometry(dw, dh, W, H, elem, layout)
        d_plain = torch.from_numpy(plain).to("cuda:0")
        for fill, (fv, fh) in FILLS.items():
            fused, fused_of = register(finder, torch, planes, ref.case_registration(dw, dh, W, H, fv, fh), layout)
            d_out = torch.full((len(plain),), SENTINEL, dtype=torch.uint8, device="cuda:0")
            finder.depth_fill_holes_device(d_plain.data_ptr() + off, FMT[fmt], W, H, out_pitch, out_stride, n, fv, fh,
                                           d_out.data_ptr() + off, out_pitch, out_stride)
            torch.cuda.synchronize()
            alone = d_out.cpu().numpy()
            assert first_difference(alone, fused) is None, (layout, fill)
            assert first_difference(fused, fused_of([ref.fill_holes(a, fv, fh) for a in unfilled(case, fmt)])) is None, (layout, fill)


@pytest.mark.parametrize("fmt", list(FMT))
def test_fill_alone_on_hand_made_and_tiny_images(finder, fmt):
    import torch
    rng = np.random.default_rng(9)
    images = []
    for h, w in ((5, 5), (3, 3), (2, 7), (7, 2), (1, 1), (3, 9), (6, 4)):
        a = rng.integers(990, 1012, size=(h, w)).astype(np.float64)
        a[rng.random((h, w)) < 0.3] = 0
        a[rng.random((h, w)) < 0.1] = 3000
        images.append(a.astype(np.uint16) if fmt == "u16" else (a / 1000.0).astype(np.float32))
    for a in images:
        h, w = a.shape
        elem = a.itemsize
        for layout in (ALIGNED, ODD):
            pitch, stride, out_pitch, out_stride, off = geometry(w, h, w, h, elem, layout)
            d_in = pack(torch, [a], pitch, stride, off)
            for fv, fh in FILLS.values():
                d_out = torch.full((off + out_stride + 8 * elem,), SENTINEL, dtype=torch.uint8, device="cuda:0")
                finder.depth_fill_holes_device(d_in.data_ptr() + off, FMT[fmt], w, h, pitch, 0, 1, fv, fh, d_out.data_ptr() + off, out_pitch, 0)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                want = expected(len(got), [ref.fill_holes(a, fv, fh)], out_pitch, out_stride, off)
                assert first_difference(got, want) is None, (a.shape, layout, fv, fh)


# ---- chunks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 2])
def test_a_batch_in_several_chunks_equals_the_unchunked_bytes(chunk):
    import torch
    name, dw, dh, W, H, _ = CASES["67x45_93x71"]
    reg = ref.case_registration(dw, dh, W, H, 1, 1)
    f = gd._finder()
    try:
        whole, whole_of = register(f, torch, scenes(name, "u16"), reg, ODD)
        f.debug_depth_register_limits(chunk, 0)
        parts, _ = register(f, torch, scenes(name, "u16"), reg, ODD)
        assert parts.tobytes() == whole.tobytes()
        assert first_difference(whole, whole_of([ref.fill_holes(a, 1, 1) for a in unfilled(name, "u16")])) is None
        with pytest.raises(lib.SepfinderError):
            f.debug_depth_register_limits(-1, 0)
        with pytest.raises(lib.SepfinderError):
            f.debug_depth_register_limits(0, 8)
    finally:
        f.close()


# ---- in front of the depth keyframe calls --------------------------------------------------------------------------------
def test_registered_scenes_feed_the_depth_keyframe_batch_call():
    import torch
    name, dw, dh, W, H, _ = CASES["80x108_97x131"]
    assert (W, H) == (gd.W, gd.H)
    n, fmt, elem = 3, "u16", 2
    reg = ref.case_registration(dw, dh, W, H, 1, 1)
    images = [dref.image(W, H, seed) for seed in ref.SEEDS]
    restated = [ref.fill_holes(a, 1, 1) for a in unfilled(name, fmt)]
    cam = dref.camera(W, H, local=True, min_depth=gd.LIMITS[0], max_depth=gd.LIMITS[1])
    det = _abi.detector_params(gd.MAXF)
    fa, fb = gd.finder_of(6), gd.finder_of(6)
    try:
        pitch, stride = W + 7, (W + 7) * H + 33
        d_img = gd.pack_planes(torch, images, pitch, stride)
        dpitch, dstride = (W + 3) * elem, (W + 3) * elem * H + 10 * elem
        # the registration writes the planes the keyframe call reads, on one stream with no host wait between them
        d_src = pack(torch, scenes(name, fmt), dw * elem, dw * dh * elem, 0)
        d_reg = torch.zeros((n * dstride,), dtype=torch.uint8, device="cuda:0")
        fa.depth_register_device(ref.abi(reg), d_src.data_ptr(), FMT[fmt], dw * elem, dw * dh * elem, n, d_reg.data_ptr(), dpitch, dstride)
        outs_a = gd.batch_outputs(torch, n, gd.MAXF, fa.descriptor_bytes())
        first = fa.get_features_and_descriptor_depth_batch_device(d_img.data_ptr(), d_reg.data_ptr(), FMT[fmt], n, W, H, pitch, stride, dpitch,
                                                                  dstride, cam, det, *(t.data_ptr() for t in outs_a))
        d_want = gd.pack_planes(torch, restated, dpitch, dstride)
        outs_b = gd.batch_outputs(torch, n, gd.MAXF, fb.descriptor_bytes())
        fb.get_features_and_descriptor_depth_batch_device(d_img.data_ptr(), d_want.data_ptr(), FMT[fmt], n, W, H, pitch, stride, dpitch, dstride,
                                                          cam, det, *(t.data_ptr() for t in outs_b))
        torch.cuda.synchronize()
        got, want = gd.read_batch(outs_a, n, gd.MAXF), gd.read_batch(outs_b, n, gd.MAXF)
        print("rows %s" % [len(g[0]) for g in got])
        assert first == 0 and fa.store_size() == fb.store_size() == n
        for g, w in zip(got, want):
            assert len(g[0]) >= 5 and np.isfinite(g[1]).all()
            gd.assert_same_keyframe(g, w)                   # rows, xyz and keypoints
    finally:
        fa.close()
        fb.close()


# ---- n_images = 0 and the refusals ---------------------------------------------------------------------------------------
def _refused(f, d_out, call, needle):
    with pytest.raises(lib.SepfinderError) as e:
        call()
    assert e.value.code == _abi.SF_EINVAL, str(e.value)
    text = str(e.value).split(": ", 1)[1]
    assert len(text) > 10 and needle in text, str(e.value)
    assert bool((d_out == SENTINEL).all()), "a refused call wrote to the output"
    return text


def test_no_image_is_ok_and_refusals_change_nothing():
    import torch
    dw, dh, W, H = 64, 48, 96, 72
    reg = ref.abi(ref.case_registration(dw, dh, W, H, 1, 1))
    f = gd._finder()
    try:
        d_in = torch.zeros((2 * W * H * 4 + 64,), dtype=torch.uint8, device="cuda:0")    # (room for two planes of either size and format)
        d_out = torch.full((2 * W * H * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        pi, po = d_in.data_ptr(), d_out.data_ptr()
        f.depth_register_device(reg, None, ref.U16, 0, 0, 0, None, 0, 0)                      # n = 0
        f.depth_fill_holes_device(None, ref.F32M, W, H, 0, 0, 0, 1, 1, None, 0, 0)
        U, Fm = ref.U16, ref.F32M

        def run(block=reg, src=pi, fmt=U, dp=2 * dw, ds=2 * dw * dh, n=2, dst=po, op=2 * W, os_=2 * W * H):
            f.depth_register_device(block, src, fmt, dp, ds, n, dst, op, os_)

        def fill(src=pi, fmt=U, w=W, h=H, dp=2 * W, ds=2 * W * H, n=2, fv=1, fh=1, dst=po, op=2 * W, os_=2 * W * H):
            f.depth_fill_holes_device(src, fmt, w, h, dp, ds, n, fv, fh, dst, op, os_)
        for name, block, _ in host.refusals():
            assert "sf_depth_register_device" in _refused(f, d_out, lambda: run(block=block), ""), name
        for kw, needle in (({"fmt": 2}, "format"), ({"fmt": -1}, "format"), ({"dp": 2 * dw - 2}, "pitch"), ({"op": 2 * W - 2}, "pitch"),
                           ({"dp": 2 * dw + 1}, "multiple"), ({"op": 2 * W + 1}, "multiple"), ({"ds": 2 * dw * dh + 1}, "multiple"),
                           ({"os_": 2 * W * H + 1}, "multiple"), ({"src": pi + 1}, "address"), ({"dst": po + 1}, "address"),
                           ({"fmt": Fm, "dp": 4 * dw, "ds": 4 * dw * dh, "op": 4 * W, "os_": 4 * W * H, "dst": po + 2}, "address"),
                           ({"ds": 2 * dw * dh - 2}, "stride"), ({"os_": 2 * W * H - 2}, "stride"), ({"src": None}, "missing"),
                           ({"dst": None}, "missing"), ({"src": po + 2 * W * H}, "overlaps"), ({"src": po - 2 * dw * dh * 2 + 2}, "overlaps"),
                           ({"n": 1, "src": po + 2 * W * (H - 1) + 2 * W - 2}, "overlaps")):
            assert "sf_depth_register_device" in _refused(f, d_out, lambda: run(**kw), needle), kw
        for kw, needle in (({"fmt": 5}, "format"), ({"fv": 2}, "fill_vertical"), ({"fh": -1}, "fill_horizontal"), ({"w": 0}, "image of"),
                           ({"h": 8193}, "image of"), ({"dp": 2 * W - 2}, "pitch"), ({"op": 2 * W + 1}, "multiple"),
                           ({"ds": 2 * W * H - 2}, "stride"), ({"os_": 2 * W * H + 1}, "multiple"), ({"src": pi + 1}, "address"),
                           ({"src": None}, "missing"), ({"dst": None}, "missing"), ({"src": po}, "overlaps"),
                           ({"src": po + 2 * W * H * 2 - 2}, "overlaps")):
            assert "sf_depth_fill_holes_device" in _refused(f, d_out, lambda: fill(**kw), needle), kw
        # buffers that touch without overlapping are taken, and the calls the refusals stood in front of do run
        run(n=1, src=po + 2 * W * H)
        run()
        fill()
        torch.cuda.synchronize()
        assert not bool((d_out[:2 * W * H * 2] == SENTINEL).all())
    finally:
        f.close()
