"""Keyframes from the camera's rgb8 / bgr8 / mono8 images, without a GPU: self-checks of the NumPy restatement
(tests/image_ref.py) that the GPU tests compare with, the C-ABI of the feature (symbols, enum values, the unchanged ABI
version) and DataHandler.compute_descriptors on a recording backend."""
import os
import re
import subprocess

import numpy as np
import pytest

from multi_robot_slam_separators_amd import _abi
from multi_robot_slam_separators_amd.data_handler import DataHandler
from tests import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_image_set_gray_rule", "sf_image_get_gray_rule", "sf_image_to_gray_device", "sf_netvlad_infer_u8_batch_device",
       "sf_get_features_and_descriptor_u8", "sf_add_keyframes_u8_batch_device"]


def opencv_table_gray(src, blue_idx, rule):
    """OpenCV's RGB2Gray<uchar> as written upstream: one 3 x 256 table of the channel products, the rounding term folded
    into the third part, coefficients {B2Y, G2Y, R2Y} exchanged at the ends when blue is not the first channel; a pixel is
    (tab[c0] + tab[c1 + 256] + tab[c2 + 512]) >> shift."""
    r2y, g2y, b2y, shift = ref.RULES[rule]
    coeffs = [b2y, g2y, r2y]
    if blue_idx != 0:
        coeffs[0], coeffs[2] = coeffs[2], coeffs[0]
    tab = np.zeros(256 * 3, np.int32)
    b, g, r = 0, 0, 1 << (shift - 1)
    for i in range(256):
        tab[i], tab[i + 256], tab[i + 512] = b, g, r
        b += coeffs[0]
        g += coeffs[1]
        r += coeffs[2]
    src = np.asarray(src, np.uint8).astype(np.int64)
    return ((tab[src[..., 0]] + tab[src[..., 1] + 256] + tab[src[..., 2] + 512]) >> shift).astype(np.uint8)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("format", [ref.RGB8, ref.BGR8])
def test_gray_equals_the_table_form(format, rule):
    rng = np.random.default_rng(100 + 2 * rule + format)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    triples = np.concatenate([rng.integers(0, 256, size=(100000, 3), dtype=np.uint8), corners])
    got = ref.gray(triples, format, rule)
    want = opencv_table_gray(triples, 2 if format == ref.RGB8 else 0, rule)     # rgb8: blue is the third channel
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got[-8] == 0 and got[-1] == 255                                      # black, white
    # the two channel orders see one pixel: the bgr8 view of the reversed triple is the rgb8 value
    assert np.array_equal(ref.gray(triples[:, ::-1], ref.BGR8 if format == ref.RGB8 else ref.RGB8, rule), got)


@pytest.mark.parametrize("rule", [0, 1])
def test_gray_of_a_gray_pixel_is_the_pixel(rule):
    v = np.arange(256, dtype=np.uint8)
    vvv = np.stack([v, v, v], axis=1)
    assert sum(ref.RULES[rule][:3]) == 1 << ref.RULES[rule][3]
    for format in (ref.RGB8, ref.BGR8):
        assert np.array_equal(ref.gray(vvv, format, rule), v)
    assert np.array_equal(ref.gray(v, ref.MONO8, rule), v)
    x = ref.netvlad_input(v.reshape(16, 16), ref.MONO8)
    assert x.dtype == np.float32 and x.shape == (16, 16, 3) and np.array_equal(x[..., 1], v.reshape(16, 16).astype(np.float32))
    rgb = np.arange(16 * 16 * 3, dtype=np.uint8).reshape(16, 16, 3)
    assert np.array_equal(ref.netvlad_input(rgb[..., ::-1], ref.BGR8), ref.netvlad_input(rgb, ref.RGB8))
    assert np.array_equal(ref.netvlad_input(rgb, ref.RGB8), rgb.astype(np.float32))             # unscaled


def test_the_rules_differ_somewhere():
    """Rule 1 is not rule 0 doubled (9798 = 2 x 4899, but 19235 != 2 x 9617 and 3735 != 2 x 1868): a test of one rule must
    be able to tell it from the other."""
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, size=(100000, 3), dtype=np.uint8)
    assert (ref.gray(t, ref.RGB8, 0) != ref.gray(t, ref.RGB8, 1)).any()


def test_header_abi_and_binding_agree(tmp_path):
    from multi_robot_slam_separators_amd import lib
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "sepfinder.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTED
        assert getattr(L, name).argtypes is not None, name                   # bound with a signature
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert int(re.search(r"#define SF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _abi.SF_ABI_VERSION == 8 and L.sf_abi_version() == 8
    for method in ("image_set_gray_rule", "image_get_gray_rule", "image_to_gray_device", "netvlad_infer_u8_batch_device",
                   "get_features_and_descriptor_u8", "add_keyframes_u8_batch_device", "netvlad_u8"):
        assert hasattr(lib.SeparatorFinder, method)
    assert _abi.GRAY_RULES == ref.RULES
    # the enum values, from the compiler
    src = tmp_path / "img.c"
    src.write_text('#include <stdio.h>\n#include "sepfinder.h"\n'
                   'int main(void){ printf("%d %d %d %d %zu %d\\n", (int)SF_IMAGE_RGB8, (int)SF_IMAGE_BGR8, (int)SF_IMAGE_MONO8,'
                   ' SF_ABI_VERSION, sizeof(sf_params), sf_abi_version()); return 0; }\n')
    exe = tmp_path / "img"
    lib_dir = os.path.join(ROOT, "multi_robot_slam_separators_amd")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir,
                           "-lsepfinder", "-Wl,-rpath," + lib_dir, "-L", "/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-lamdhip64"])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [_abi.SF_IMAGE_RGB8, _abi.SF_IMAGE_BGR8, _abi.SF_IMAGE_MONO8] == [ref.RGB8, ref.BGR8, ref.MONO8] == [0, 1, 2]
    assert got[3:] == [8, 232, 8]


class RecordingBackend:
    """What DataHandler needs of a backend for the image path; image i is a constant image of value i."""

    def __init__(self, width=8):
        self.width = width
        self.netvlad_calls, self.appended, self.feature_calls = [], [], []

    def get_features_u8(self, left, right, format):
        self.feature_calls.append((int(left[0, 0, 0]), int(right[0, 0, 0]), format))
        k = int(left[0, 0, 0])
        return np.full((2, 32), k, np.uint8), np.full((2, 3), k, np.float32), np.zeros(2, _abi.KEYPOINT_DTYPE)

    def netvlad_u8(self, images, format):
        ids = [int(im[0, 0, 0]) for im in images]
        self.netvlad_calls.append(ids)
        return np.array([[100.0 * i + d for d in range(self.width)] for i in ids], np.float32).reshape(len(ids), self.width)

    def nn_append_local(self, rows):
        self.appended.append(np.array(rows, copy=True))


def test_compute_descriptors_batches_from_the_left_and_keeps_indices_aligned():
    be = RecordingBackend(width=8)
    dh = DataHandler(be, 0, 1, netvlad_dimensions=4, netvlad_batch_size=3)
    for i in range(7):
        img = np.full((4, 6, 3), i, np.uint8)
        assert dh.add_keyframe_images(img, np.full((4, 6, 3), 50 + i, np.uint8))
    assert be.feature_calls == [(i, 50 + i, _abi.SF_IMAGE_RGB8) for i in range(7)]
    assert len(dh.geometric_feats) == 7 and len(dh.images_rgb_kf) == 7 and dh.kf_ids_of_frames_kept == list(range(7))
    assert [dh.compute_descriptors() for _ in range(3)] == [3, 3, 1]
    assert be.netvlad_calls == [[0, 1, 2], [3, 4, 5], [6]]
    assert len(dh.images_rgb_kf) == 0
    before = (len(dh.local_descriptors), len(be.appended), len(be.netvlad_calls))
    assert dh.compute_descriptors() == 0                                      # the empty call changes nothing
    assert (len(dh.local_descriptors), len(be.appended), len(be.netvlad_calls)) == before == (7, 3, 3)
    # the first netvlad_dimensions values, in queue order, the same rows in the backend's database
    want = np.array([[100.0 * i + d for d in range(4)] for i in range(7)])
    assert np.array_equal(np.array(dh.local_descriptors), want)
    assert np.array_equal(np.concatenate(be.appended), want) and [len(a) for a in be.appended] == [3, 3, 1]
    # geometric_feats[i] <-> local_descriptors[i] (data_handler.py:268, :157-158)
    for i in range(7):
        assert int(dh.get_geom_features(i).descriptors[0, 0]) == i == int(dh.local_descriptors[i][0] // 100)


def test_compute_descriptors_refuses_a_short_descriptor_and_takes_an_rgb_image_of_its_own():
    be = RecordingBackend(width=3)
    dh = DataHandler(be, 0, 1, netvlad_dimensions=4)
    assert dh.add_keyframe_images(np.full((4, 6, 3), 1, np.uint8), np.full((4, 6, 3), 2, np.uint8),
                                  image_rgb=np.full((4, 6, 3), 9, np.uint8))
    with pytest.raises(ValueError):
        dh.compute_descriptors()
    assert len(dh.local_descriptors) == 0 and be.appended == [] and len(dh.images_rgb_kf) == 1
    assert be.netvlad_calls == [[9]]                                          # the rgb camera's image, not the left one
