"""Latency of one SIFT keyframe (Vis/FeatureType 1) against SURF (0), both on handles with desc_type 1, on 752 x 480 stereo
pairs with 1 000 features, single calls, the two types alternating round by round in one process:
  detect   the detector call alone on a device image (sf_detect_surf_device / sf_detect_sift_device); it waits for the
           keypoint count (SIFT: for the count of extrema too), so it is timed by the wall clock
  extract  sf_extract_keyframe_device on that detector's keypoints (SURF: integral image, descriptors; SIFT: the pyramid
           built again, descriptors; 3D points, commit), asynchronous calls back to back, HIP events
  full     sf_get_features_and_descriptor on host images (upload, detector, LK, extraction, download), wall clock
Prints one line per type with the medians over the rounds and writes all rounds as JSON to --out.
usage: python tools/sift_latency.py [--features 1000] [--reps 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402
from tests import extract_cases as ec  # noqa: E402

KINDS = (("surf", 0), ("sift", 1))


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps     # us per call


def events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps            # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.features
    left, right = (np.ascontiguousarray(x) for x in ec.make_stereo_pair(800, pad=0)[:2])
    h, w = left.shape
    d_left = torch.from_numpy(left).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(n)
    handles, kpts = {}, {}
    for name, ft in KINDS:
        p = synth.camera_params()
        p.max_features = max(1024, n)
        p.store_capacity = 2 * a.reps + 64
        p.desc_type, p.desc_bytes = 1, 512 if ft == 1 else 256
        f = lib.SeparatorFinder(p, device=0)
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        if ft == 1:
            f.set_feature_type_sift()
        else:
            f.set_feature_type_surf()
        handles[name] = f
        kpts[name] = torch.zeros((n, 28), dtype=torch.uint8, device=dev)
    out = {"tool": "tools/sift_latency.py", "image": [w, h], "features": n, "rounds": a.rounds, "reps": a.reps,
           "unit": "us per call", "cases": {name: [] for name, _ in KINDS}}
    for _ in range(a.rounds):
        for name, ft in KINDS:
            f, d_kp = handles[name], kpts[name]
            f.store_clear()
            call = f.detect_sift if ft == 1 else f.detect_surf
            detect = lambda: call(d_left.data_ptr(), w, h, w, n, d_kp.data_ptr(), n)
            found = min(detect(), n)
            us_detect = wall(detect, a.reps)

            def extract():
                f.extract_keyframe_device(d_left.data_ptr(), w, h, w, d_kp.data_ptr(), None, None, found, cam, want_rows=False)
            us_extract = events(extract, a.reps)
            _, kept = f.extract_keyframe_device(d_left.data_ptr(), w, h, w, d_kp.data_ptr(), None, None, found, cam)
            f.store_clear()
            rows = len(f.get_features_and_descriptor(left, right, cam, det)[0])
            f.store_clear()
            us_full = wall(lambda: f.get_features_and_descriptor(left, right, cam, det), max(a.reps // 4, 3))
            out["cases"][name].append({"detect_us": round(us_detect, 1), "found": found, "extract_us": round(us_extract, 1),
                                       "kept": kept, "full_us": round(us_full, 1), "full_rows": rows})
    out["medians"] = {}
    for name, _ in KINDS:
        r = out["cases"][name]
        med = lambda k: float(np.median([x[k] for x in r]))
        out["medians"][name] = {k: med(k) for k in ("detect_us", "extract_us", "full_us")}
        print("%-6s detect %8.1f us (%d keypoints)   extract %8.1f us (%d kept)   full call %8.1f us (%d rows); medians of %d "
              "rounds" % (name, med("detect_us"), r[0]["found"], med("extract_us"), r[0]["kept"], med("full_us"),
                          r[0]["full_rows"], a.rounds), flush=True)
    for f in handles.values():
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
