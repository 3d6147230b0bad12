"""The images of the SURF batch tests (tests/test_gpu_surf_batch.py, tests/test_surf_batch_host.py) and the restatement's
keypoints on them, computed once.  Two shapes:

  "160x120"  pitch 173, five pairs A .. E that differ so that per-image state cannot leak: A = texture("160x120 padded")
             of tests/test_gpu_surf.py (its right half repeats the left: pairs of exactly equal response), B = A with the
             columns from w // 3 on set to 128, C flat 77, D flat 128 with A's [30:78, 30:78] patch, E = A again
  "97x61"    pitch = width, three pairs A', flat 77, A' with A' = texture("97x61")

The right image of every pair is the left one shifted by 6 pixels."""
import functools

import numpy as np

from tests import surf_ref as ref
from tests.test_gpu_surf import PARAM_SETS, texture

MAXF = {"160x120": 50, "97x61": 8}
# the restatement's keypoints before limitKeypoints, per image: under the defaults / at hessian_threshold 0
COUNTS = {"160x120": ([86, 29, 0, 16, 86], [100, 32, 0, 29, 100]), "97x61": ([11, 0, 11], None)}


@functools.lru_cache(maxsize=None)
def left_images(shape):
    if shape == "97x61":
        a = np.ascontiguousarray(texture("97x61"))
        out = [a, np.full_like(a, 77), a]
    else:
        a = np.ascontiguousarray(texture("160x120 padded"))
        h, w = a.shape
        b = a.copy()
        b[:, w // 3:] = 128
        c = np.full_like(a, 77)
        d = np.full_like(a, 128)
        d[30:78, 30:78] = a[30:78, 30:78]
        out = [a, b, c, d, a]
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pairs(shape):
    return [(l, np.ascontiguousarray(np.roll(l, -6, axis=1))) for l in left_images(shape)]


@functools.lru_cache(maxsize=None)
def detected(shape, i, pset):
    """The restatement's keypoints of left image i under PARAM_SETS[pset], before limitKeypoints."""
    kp = ref.detect(left_images(shape)[i], ref.Params(**PARAM_SETS[pset]), 0)
    kp.setflags(write=False)
    return kp


def batch_bound(width, height, n_octaves=4, n_octave_layers=2):
    """The bound B of include/sf_experimental.h (sf_surf_batch_plan) on the maxima of one image, restated: two maxima of a
    layer are never 8-adjacent, so an r x c interior holds at most ceil(r / 2) ceil(c / 2)."""
    total = 0
    for o in range(n_octaves):
        for l in range(1, n_octave_layers + 1):
            margin = (((ref.HAAR_SIZE0 + ref.HAAR_SIZE_INC * (l + 1)) << o) // 2 >> o) + 1
            r, c = max((height >> o) - 2 * margin, 0), max((width >> o) - 2 * margin, 0)
            total += -(-r // 2) * -(-c // 2)
    return total
