"""Latency of a GFTT/BRIEF keyframe (Vis/FeatureType 6) under the handle's GFTT parameters (sf_gftt_set_params: block
size, Harris or minimum eigenvalue) on 752 x 480 images, the configurations alternating round by round in one process
on one handle:
  detect  sf_detect_corners_device alone on a device image (it waits for the candidate and the result count), wall clock
  single  sf_get_features_and_descriptor on a host pair (upload, detector, stereo flow, extraction, download), wall clock
  batch   sf_get_features_and_descriptor_batch_device on 64 device pairs, per keyframe, HIP events
(3, 0) is the default configuration, which runs the kernels the detector had before the parameters existed: its batch
figure is the one to hold beside the GFTT/BRIEF row of tools/freak_latency.py.  Prints one line per configuration with
the medians over the rounds and writes all rounds as JSON to --out.
usage: python tools/gftt_latency.py [--features 1000] [--reps 50] [--batch-reps 10] [--rounds 5] [--out FILE]"""
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

CONFIGS = ((3, 0), (3, 1), (7, 0), (7, 1), (15, 0))


def wall(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps   # us per call


def events(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n_kf, maxf = 64, a.features
    pairs = [tuple(np.ascontiguousarray(x) for x in ec.make_stereo_pair(800 + i, pad=0)[:2]) for i in range(n_kf)]
    h, w = pairs[0][0].shape
    L = torch.from_numpy(np.stack([l for l, _ in pairs]).reshape(n_kf, -1)).to(dev)
    R = torch.from_numpy(np.stack([r for _, r in pairs]).reshape(n_kf, -1)).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(maxf)
    rows_dev = torch.zeros(n_kf, dtype=torch.int32, device=dev)
    d_kp = torch.zeros((maxf, 28), dtype=torch.uint8, device=dev)
    p = synth.camera_params()
    p.max_features = max(1024, maxf)
    p.store_capacity = max(a.reps + 8, (a.batch_reps + 2) * n_kf) + 64
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    name = lambda c: "block %d, %s" % (c[0], "Harris" if c[1] else "min eigenvalue")
    out = {"image": [w, h], "features": maxf, "batch": n_kf, "rounds": a.rounds, "feature_type": 6,
           "cases": {name(c): [] for c in CONFIGS}}
    for _ in range(a.rounds):
        for c in CONFIGS:
            f.gftt_set_params(_abi.gftt_params(c[0], c[1], 0.04))
            found = [0]

            def detect():
                found[0] = f.detect_corners_device(L.data_ptr(), w, h, w, maxf, det.quality_level, det.min_distance,
                                                   d_kp.data_ptr(), maxf)
            us_detect = wall(detect, a.reps)
            f.store_clear()
            kept = [0]

            def single():
                kept[0] = len(f.get_features_and_descriptor(pairs[0][0], pairs[0][1], cam, det)[0])
            us_single = wall(single, a.reps)
            f.store_clear()

            def batch():
                f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, cam, det,
                                                           d_rows_out=rows_dev.data_ptr())
            us_batch = events(batch, a.batch_reps)
            rows = rows_dev.cpu().numpy()
            out["cases"][name(c)].append({"detect_us": round(us_detect, 2), "corners": found[0],
                                          "single_us": round(us_single, 2), "single_rows": kept[0],
                                          "batch_us_per_keyframe": round(us_batch / n_kf, 2),
                                          "batch_mean_rows": round(float(rows.mean()), 1)})
    f.close()
    out["medians"] = {}
    for c in CONFIGS:
        r = out["cases"][name(c)]
        med = {k: float(np.median([x[k] for x in r])) for k in ("detect_us", "single_us", "batch_us_per_keyframe")}
        out["medians"][name(c)] = med
        print("%-26s detector %7.1f us (%d corners)   single call %7.1f us (%d rows)   batch of %d: %7.1f us per keyframe "
              "(%.0f rows on average); medians of %d rounds" % (name(c), med["detect_us"], r[0]["corners"], med["single_us"],
                                                                r[0]["single_rows"], n_kf, med["batch_us_per_keyframe"],
                                                                r[0]["batch_mean_rows"], a.rounds), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
