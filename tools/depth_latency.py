"""Latency of a depth keyframe against a stereo keyframe on 752 x 480 images, 1 000 features, under Vis/FeatureType 6
(GFTT/BRIEF) and 4 (FAST/BRIEF), the two alternating round by round in one process on one handle:
  single  sf_get_features_and_descriptor on a host pair (upload, detector, stereo flow, extraction, download) against
          sf_get_features_and_descriptor_depth on a host image and a uint16 depth image (upload, mask, detector under the
          mask, extraction with depth points, download), wall clock
  batch   sf_get_features_and_descriptor_batch_device against sf_get_features_and_descriptor_depth_batch_device on 64
          device keyframes, per keyframe, HIP events
The depth images are the seeded piecewise-planar scenes of tests/depth_ref.py (holes and steps), Vis/DepthAsMask 1, no
depth limits.  Prints one line per type with the medians over the rounds and writes all rounds as JSON to --out.  One
run on one machine: no claim beyond it.
usage: python tools/depth_latency.py [--features 1000] [--reps 30] [--batch-reps 10] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402
from tests import depth_ref  # noqa: E402
from tests import extract_cases as ec  # noqa: E402

KINDS = (("gftt_brief", 6), ("fast_brief", 4))


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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n_kf, maxf = 64, a.features
    pairs = [tuple(np.ascontiguousarray(x) for x in ec.make_stereo_pair(800 + i, pad=0)[:2]) for i in range(n_kf)]
    h, w = pairs[0][0].shape
    depths = [depth_ref.scene(w, h, 900 + i, _abi.SF_DEPTH_U16_MM) for i in range(n_kf)]
    L = torch.from_numpy(np.stack([l for l, _ in pairs]).reshape(n_kf, -1)).to(dev)
    R = torch.from_numpy(np.stack([r for _, r in pairs]).reshape(n_kf, -1)).to(dev)
    D = torch.from_numpy(np.stack(depths).view(np.uint8).reshape(n_kf, -1)).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(maxf)
    rows_dev = torch.zeros(n_kf, dtype=torch.int32, device=dev)
    p = synth.camera_params()
    p.max_features = max(1024, maxf)
    p.store_capacity = max(a.reps + 8, (a.batch_reps + 2) * n_kf) + 64
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"image": [w, h], "features": maxf, "batch": n_kf, "rounds": a.rounds, "depth_format": "uint16 mm",
           "depth_as_mask": 1, "cases": {name: [] for name, _ in KINDS}}
    for _ in range(a.rounds):
        for name, ft in KINDS:
            f.set_feature_type(ft)
            kept = {}

            def stereo_single():
                kept["stereo"] = len(f.get_features_and_descriptor(pairs[0][0], pairs[0][1], cam, det)[0])

            def depth_single():
                kept["depth"] = len(f.get_features_and_descriptor_depth(pairs[0][0], depths[0], cam, det)[0])

            def stereo_batch():
                f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, cam, det,
                                                           d_rows_out=rows_dev.data_ptr())

            def depth_batch():
                f.get_features_and_descriptor_depth_batch_device(L.data_ptr(), D.data_ptr(), _abi.SF_DEPTH_U16_MM, n_kf, w, h, w,
                                                                 w * h, 2 * w, 2 * w * h, cam, det, d_rows_out=rows_dev.data_ptr())
            r = {}
            for key, fn, timer, reps in (("stereo_single_us", stereo_single, wall, a.reps), ("depth_single_us", depth_single, wall, a.reps),
                                         ("stereo_batch_us_per_keyframe", stereo_batch, events, a.batch_reps),
                                         ("depth_batch_us_per_keyframe", depth_batch, events, a.batch_reps)):
                f.store_clear()
                us = timer(fn, reps)
                r[key] = round(us / n_kf if "batch" in key else us, 2)
                if "batch" in key:
                    r[key.split("_")[0] + "_batch_mean_rows"] = round(float(rows_dev.cpu().numpy().mean()), 1)
            r["stereo_single_rows"], r["depth_single_rows"] = kept["stereo"], kept["depth"]
            out["cases"][name].append(r)
    f.close()
    out["medians"] = {}
    keys = ("stereo_single_us", "depth_single_us", "stereo_batch_us_per_keyframe", "depth_batch_us_per_keyframe")
    for name, ft in KINDS:
        rr = out["cases"][name]
        med = {k: float(np.median([x[k] for x in rr])) for k in keys}
        out["medians"][name] = med
        print("type %d %-11s single call: stereo %7.1f us (%d rows), depth %7.1f us (%d rows)   batch of %d, per keyframe: stereo "
              "%6.1f us, depth %6.1f us; medians of %d rounds" % (ft, name, med["stereo_single_us"], rr[0]["stereo_single_rows"],
                                                                  med["depth_single_us"], rr[0]["depth_single_rows"], n_kf,
                                                                  med["stereo_batch_us_per_keyframe"],
                                                                  med["depth_batch_us_per_keyframe"], a.rounds), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
