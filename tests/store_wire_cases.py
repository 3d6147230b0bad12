"""Inputs the keyframe-blob tests share (tests/test_store_wire_host.py, tests/test_gpu_store_wire.py): random keyframes of
the shapes at which the copy kernels change path, and the malformed blobs with the status each must get."""
import numpy as np

from multi_robot_slam_separators_amd import _abi
from tests import store_wire_ref as ref

ROWS = (0, 1, 63, 64, 65, 257)      # around a wavefront, a 16 KB piece (257 rows of 64 bytes), and none at all
OCTAVES = (-1, 0, 3, 127)
# (desc_type, desc_bytes of the handle, the widths of its keyframes): one width class per handle
HANDLES = [(0, 32, (1, 7, 32)), (0, 64, (33, 64)), (1, 256, (256,)), (1, 512, (512,)), (2, 128, (128,))]


def rand_features(rng, rows, cols, with_3d):
    """_abi.FeatureArrays of `rows` random rows: xyz with NaN in it, octaves of OCTAVES, and the four keypoint fields the
    store drops filled with noise."""
    desc = rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)
    xyz = rng.normal(size=(rows, 3)).astype(np.float32)
    xyz[rng.random((rows, 3)) < 0.2] = np.nan
    kp = np.zeros(rows, _abi.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.uniform(0, 700, rows), rng.uniform(0, 400, rows)
    kp["size"], kp["angle"], kp["response"] = rng.uniform(1, 30, rows), rng.uniform(0, 360, rows), rng.random(rows)
    kp["octave"] = rng.choice(OCTAVES, rows)
    kp["class_id"] = rng.integers(-1, 5, rows)
    return _abi.FeatureArrays(desc, xyz if with_3d else np.zeros((0, 3), np.float32), kp)


def mixed_features(seed, widths, rows=ROWS):
    """Every row count of ROWS with and without 3D points, the widths in turn."""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(rows):
        for with_3d in (True, False):
            out.append(rand_features(rng, r, widths[(len(out) + i) % len(widths)], with_3d))
    return out


# ---- malformed blobs -----------------------------------------------------------------------------------------------------
MAL_ROWS = (5, 64, 0, 17)           # keyframes of the blob every case is cut from; 32-byte rows, binary handle
MAL_N, MAL_MAX_ROWS, MAL_COLS, MAL_DESC_TYPE = 4, 64, 32, 0


def malformed_base(seed=11):
    rng = np.random.default_rng(seed)
    feats = [rand_features(rng, r, MAL_COLS, i != 3) for i, r in enumerate(MAL_ROWS)]
    return feats, ref.pack([ref.of_features(f) for f in feats], MAL_DESC_TYPE)


def malformed_cases():
    """[(name, blob bytes, (n, max_rows, cols, desc_type) of the import, status bits, emptied keyframes)]: one rule broken
    per case.  No planted offset or length exceeds twice the blob's bytes."""
    _, good = malformed_base()
    nbytes = len(good)
    args = (MAL_N, MAL_MAX_ROWS, MAL_COLS, MAL_DESC_TYPE)
    every = list(range(MAL_N))
    cases = []

    def case(name, edit, bits, emptied, call=args):
        raw = np.frombuffer(good, np.uint8).copy()
        edit(raw[:32].view(ref.HEADER), raw[32: 32 + 32 * MAL_N].view(ref.ENTRY))
        cases.append((name, raw.tobytes(), call, bits, emptied))

    def put(view, i, field, value):
        view[field][i] = value

    H, E = ref.BAD_HEADER, ref.BAD_ENTRY
    case("wrong magic", lambda h, t: put(h, 0, "magic", 0x424B4654), H, every)
    case("version 2", lambda h, t: put(h, 0, "version", 2), H, every)
    case("desc_type of another handle kind", lambda h, t: put(h, 0, "desc_type", 1), H, every)
    case("n_keyframes != n", lambda h, t: put(h, 0, "n_keyframes", MAL_N - 1), H, every)
    case("total_bytes > bytes", lambda h, t: put(h, 0, "total_bytes", nbytes + 16), H, every)
    case("rows = max_rows + 1", lambda h, t: None, E, [1], call=(MAL_N, MAL_MAX_ROWS - 1, MAL_COLS, MAL_DESC_TYPE))
    case("rows = -1", lambda h, t: (put(t, 1, "rows", -1), put(t, 1, "n3d", -1)), E, [1])
    case("n3d = rows - 1", lambda h, t: put(t, 1, "n3d", MAL_ROWS[1] - 1), E, [1])
    case("unaligned offset", lambda h, t: put(t, 1, "offset", int(t["offset"][1]) + 8), E, [1])
    case("offset inside the table", lambda h, t: put(t, 0, "offset", 32), E, [0])
    case("offset + bytes one past total_bytes", lambda h, t: put(h, 0, "total_bytes", nbytes - 1), E, [3])
    case("bytes inconsistent with rows", lambda h, t: put(t, 1, "bytes", int(t["bytes"][1]) + 16), E, [1])
    case("cols of another width class", lambda h, t: put(t, 0, "cols", 33), E, [0])
    return cases
