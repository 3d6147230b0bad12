"""What the feature front end refuses, and what it lets through, call by call: a deterministic list of cases and run_all(),
which runs them through the C-ABI and returns [case id, return code, sf_last_error text, feature type after, store size
after] per case.  tests/test_gpu_front_refusals.py compares that list with tests/golden/front_refusals.json, byte for byte:
the texts are the interface a caller reads, and the other tests look at them by substring only.

The fixture is recorded from the library of the commit BEFORE a change to the front end's host code, never from the code
under test: build that commit's csrc/ into a second file, then
    SEPFINDER_LIB=<that file> python tests/front_refusal_cases.py --record --commit <its hash>

Four handles: binary rows (desc_type 0) of 32 and of 64 bytes (FREAK's) and float rows (desc_type 1) of 256 and of 512
bytes, each with a NetVLAD model of random weights.  Every image is 64 x 48 and zero-filled, so a call that is let through
adds empty keyframes: its text is recorded as "" (sf_last_error keeps the text of an earlier refusal).  Every case is a
refusal or such a run:
  - sf_set_feature_type(t), t = -1 .. 9, on each handle;
  - each built type, on a handle that can hold it, against all eight batch calls with n_keyframes 2 and 0;
  - each built type with Vis/RoiRatios (0.1, 0, 0, 0), then with a 2 x 2 grid, on its own batch call and on
    sf_get_features_and_descriptor;
  - a 4096 x 4096 shape on each family's batch call (refused before anything is read: the integral image);
  - n_keyframes 65536 on each family.  The ORB, SURF and SIFT calls refuse more than 65535 keyframes.  The generic calls
    have no such limit of their own -- there the case would be a launch sequence over 65 536 images, not a refusal -- so the
    generic family is asked under a 2 x 2 grid, where the limit of 65535 cells per call refuses it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "front_refusals.json")
W, H = 64, 48
HANDLES = {"binary 32": (0, 32), "binary 64": (0, 64), "float 256": (1, 256), "float 512": (1, 512)}   # name: (desc_type, desc_bytes)
FAMILIES = {"generic": "", "orb": "orb_", "surf": "surf_", "sift": "sift_"}          # family: infix of its two batch calls
TYPES = {0: ("float 256", "surf"), 1: ("float 512", "sift"), 2: ("binary 32", "orb"), 3: ("binary 64", "generic"),
         4: ("binary 32", "generic"), 5: ("binary 64", "generic"), 6: ("binary 32", "generic"), 8: ("binary 32", "generic")}


def _finder(desc_type, desc_bytes):
    import torch
    from oracle import netvlad_torch
    p = synth.camera_params()
    p.max_features = 2048
    p.fx, p.fy, p.cx, p.cy = 460.0, 458.0, W / 2.0, H / 2.0
    p.image_width, p.image_height = W, H
    p.desc_type, p.desc_bytes = desc_type, desc_bytes
    p.netvlad_dimensions = 128
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    f.netvlad_load(netvlad_torch.random_weights(3, clusters=64, pca_dim=128))
    return f


def _select(f, t):
    if t == 0:
        f.set_feature_type_surf()
    elif t == 1:
        f.set_feature_type_sift()
    elif t == 2:
        f.set_feature_type_orb()
    elif t in (3, 5):
        f.set_feature_type_freak(t)
    else:
        f.set_feature_type(t)


def run_all():
    """Every case, in order, on four fresh handles.  Needs a GPU."""
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    gray = torch.zeros((2, H * W), dtype=torch.uint8, device=dev).data_ptr()
    rgb = torch.zeros((2, H * 3 * W), dtype=torch.uint8, device=dev).data_ptr()
    blank = np.zeros((H, W), np.uint8)
    cam, det = _abi.stereo_camera(460.0, 458.0, W / 2.0, H / 2.0, 0.11), _abi.detector_params(64)
    finders = {name: _finder(*kind) for name, kind in HANDLES.items()}
    out = []

    def record(f, case, fn):
        try:
            fn()
            rc, text = 0, ""
        except lib.SepfinderError as e:
            rc, text = e.code, (f._L.sf_last_error(f._h) or b"").decode()
        out.append([case, rc, text, f.get_feature_type()[0], f.store_size()])

    def get(f, family, n, w=W, h=H):
        call = getattr(f, "get_features_and_descriptor_%sbatch_device" % FAMILIES[family])
        return lambda: call(gray, gray, n, w, h, w, w * h, cam, det)

    def add(f, family, n):
        call = getattr(f, "add_keyframes_%su8_batch_device" % FAMILIES[family])
        return lambda: call(rgb, rgb, None, _abi.SF_IMAGE_RGB8, n, W, H, 3 * W, 3 * W * H, cam, det)

    try:
        for name, f in finders.items():
            for t in range(-1, 10):
                record(f, "%s: sf_set_feature_type(%d)" % (name, t), lambda: f.set_feature_type(t))
        for t, (name, own) in TYPES.items():
            f = finders[name]
            _select(f, t)
            for family in FAMILIES:
                for n in (2, 0):
                    record(f, "type %d: %s get_features batch, n %d" % (t, family, n), get(f, family, n))
                    record(f, "type %d: %s add_keyframes batch, n %d" % (t, family, n), add(f, family, n))
            for what, front, grid in (("roi", (0.1, 0.0, 0.0, 0.0), (1, 1)), ("grid 2 x 2", (0.0, 0.0, 0.0, 0.0), (2, 2))):
                f.front_set_params(_abi.front_params(front, 3, 0, 0.02))
                f.grid_set_params(_abi.grid_params(*grid))
                record(f, "type %d: %s, own batch call" % (t, what), get(f, own, 2))
                record(f, "type %d: %s, sf_get_features_and_descriptor" % (t, what),
                       lambda: f.get_features_and_descriptor(blank, blank, cam, det))
            f.front_set_params(_abi.front_params((0.0, 0.0, 0.0, 0.0), 3, 0, 0.02))
            f.grid_set_params(_abi.grid_params(1, 1))
        for t in (6, 2, 0, 1):                                                       # one type per family
            name, family = TYPES[t]
            f = finders[name]
            _select(f, t)
            record(f, "%s family: 4096 x 4096" % family, get(f, family, 2, 4096, 4096))   # (refused: nothing is read)
            if family == "generic":
                f.grid_set_params(_abi.grid_params(2, 2))
            record(f, "%s family: n 65536" % family, get(f, family, 65536))
            f.grid_set_params(_abi.grid_params(1, 1))
    finally:
        for f in finders.values():
            f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", help="write tests/golden/front_refusals.json from the loaded library")
    ap.add_argument("--commit", default=None, help="the commit whose library is loaded (stored in the fixture)")
    a = ap.parse_args()
    cases = run_all()
    if a.record:
        if not a.commit:
            ap.error("--record needs --commit: the fixture says which commit's library it was recorded from")
        with open(GOLDEN, "w") as fh:
            json.dump({"recorded_at": a.commit, "cases": cases}, fh, indent=0)
            fh.write("\n")
    for c in cases:
        print(json.dumps(c))
    print("%d cases" % len(cases))


if __name__ == "__main__":
    main()
