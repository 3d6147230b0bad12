"""The images of the SIFT batch tests (tests/test_gpu_sift_batch.py, tests/test_gpu_sift_batch_u8.py) and the restatement's
keypoints on them, computed once.  The images are tests/surf_batch_cases.py's: "160x120" (five pairs A .. E: A's right half
repeats its left, B = A with two thirds set to 128, C flat, D a patch of A on a flat ground, E = A again) and "97x61" (A',
flat, A').  What makes them worth running is asserted on the restatement alone (COUNTS, EXTREMA, check_preconditions)."""
import functools

import numpy as np

from tests import sift_ref as ref
from tests.surf_batch_cases import left_images, pairs  # noqa: F401  (the tests take both from here)

MAXF = {"160x120": 80, "97x61": 20}
# the restatement's keypoints before the cut, per image: (under the defaults, at contrast_threshold 0.01)
COUNTS = {"160x120": ([182, 66, 0, 33, 182], [214, 78, 0, 36, 214]), "97x61": ([45, 0, 45], [68, 0, 68])}
# ... and its refined extrema (the first-stage count of the detector) under the defaults
EXTREMA = {"160x120": [163, 57, 0, 30, 163], "97x61": [39, 0, 39]}
PARAM_SETS = {"defaults": {}, "contrast 0.01": dict(contrast_threshold=0.01)}


@functools.lru_cache(maxsize=None)
def detected(shape, i, pset="defaults"):
    """(keypoints of left image i under PARAM_SETS[pset] before any cut, its refined extrema)."""
    trace = {}
    kp = ref.detect(left_images(shape)[i], ref.Params(**PARAM_SETS[pset]), 0, trace)
    kp.setflags(write=False)
    return kp, sum(trace["extrema"])


def check_preconditions(shape, pset="defaults"):
    """On the restatement alone, before anything runs on the GPU."""
    found = [detected(shape, i, pset) for i in range(len(left_images(shape)))]
    n = [len(k) for k, _ in found]
    maxf = MAXF[shape]
    print("%s, %s: restatement keypoints %s, extrema %s, max_features %d" % (shape, pset, n, [e for _, e in found], maxf))
    assert n == COUNTS[shape][1 if pset == "contrast 0.01" else 0]
    if pset == "defaults":
        assert [e for _, e in found] == EXTREMA[shape]
    if shape == "160x120":
        resp = found[0][0]["response"]
        assert n[0] > maxf and n[4] > maxf                                  # A, E: the cut applies
        assert 0 < n[1] < maxf and 0 < n[3] < maxf and n[2] == 0            # B, D: under the limit; C: nothing
        assert (np.diff(resp) <= 0).all()
        if pset == "defaults":
            assert resp[maxf - 1] == resp[maxf]                             # the cut falls between two equal responses
            assert n[0] - len(np.unique(resp)) == 79
    else:
        assert n[0] > maxf and n[1] == 0
