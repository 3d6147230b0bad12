"""Latency of a depth keyframe from a decimated depth image against the full-size depth path of the same build, on 752 x 480
images, 1 000 features, under Vis/FeatureType 6 (GFTT/BRIEF) and 4 (FAST/BRIEF).  The depth sizes 752 x 480 (factor 1: the
existing kernels), 376 x 240 (factor 2) and 188 x 120 (factor 4) alternate round by round in one process on one handle
(sf_depth_set_size between them):
  single  sf_get_features_and_descriptor_depth on a host image and a host uint16 depth image (upload, mask of the
          interpolated image, detector under the mask, extraction with depth points, download), wall clock
  batch   sf_get_features_and_descriptor_depth_batch_device on 64 device keyframes, per keyframe, HIP events
The depth images are the seeded piecewise-planar scenes of tests/depth_ref.py, made at each size (not one scene decimated:
the masks, and so the corners, differ between the sizes; the rows kept are printed), Vis/DepthAsMask 1, no depth limits.
Prints one line per type and size with the medians over the rounds and writes all rounds as JSON to --out.  One run on one
machine: no claim beyond it.
usage: python tools/depth_decimated_latency.py [--features 1000] [--reps 30] [--batch-reps 10] [--rounds 5] [--out FILE]"""
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
FACTORS = (1, 2, 4)


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
    images = [np.ascontiguousarray(ec.make_stereo_pair(800 + i, pad=0)[0]) for i in range(n_kf)]
    h, w = images[0].shape
    L = torch.from_numpy(np.stack(images).reshape(n_kf, -1)).to(dev)
    sizes, depths, D = {}, {}, {}
    for fac in FACTORS:
        assert w % fac == 0 and h % fac == 0
        dw, dh = w // fac, h // fac
        assert lib.depth_interpolation_factor(w, h, dw, dh) == fac
        sizes[fac] = (dw, dh)
        depths[fac] = [depth_ref.scene(dw, dh, 900 + i, _abi.SF_DEPTH_U16_MM) for i in range(n_kf)]
        D[fac] = torch.from_numpy(np.stack(depths[fac]).view(np.uint8).reshape(n_kf, -1)).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(maxf)
    rows_dev = torch.zeros(n_kf, dtype=torch.int32, device=dev)
    p = synth.camera_params()
    p.max_features = max(1024, maxf)
    p.store_capacity = max(a.reps + 8, (a.batch_reps + 2) * n_kf) + 64
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"image": [w, h], "depth_sizes": {str(fac): list(sizes[fac]) for fac in FACTORS}, "features": maxf, "batch": n_kf,
           "rounds": a.rounds, "depth_format": "uint16 mm", "depth_as_mask": 1,
           "cases": {name: {str(fac): [] for fac in FACTORS} for name, _ in KINDS}}
    for _ in range(a.rounds):
        for name, ft in KINDS:
            f.set_feature_type(ft)
            for fac in FACTORS:
                dw, dh = sizes[fac]
                f.depth_set_size(_abi.depth_size(dw, dh) if fac > 1 else None)
                kept = {}

                def single():
                    kept["rows"] = len(f.get_features_and_descriptor_depth(images[0], depths[fac][0], cam, det)[0])

                def batch():
                    f.get_features_and_descriptor_depth_batch_device(L.data_ptr(), D[fac].data_ptr(), _abi.SF_DEPTH_U16_MM, n_kf, w, h,
                                                                     w, w * h, 2 * dw, 2 * dw * dh, cam, det,
                                                                     d_rows_out=rows_dev.data_ptr())
                r = {}
                f.store_clear()
                r["single_us"] = round(wall(single, a.reps), 2)
                r["single_rows"] = kept["rows"]
                f.store_clear()
                r["batch_us_per_keyframe"] = round(events(batch, a.batch_reps) / n_kf, 2)
                r["batch_mean_rows"] = round(float(rows_dev.cpu().numpy().mean()), 1)
                out["cases"][name][str(fac)].append(r)
    f.close()
    out["medians"] = {}
    for name, ft in KINDS:
        out["medians"][name] = {}
        for fac in FACTORS:
            rr = out["cases"][name][str(fac)]
            med = {k: float(np.median([x[k] for x in rr])) for k in ("single_us", "batch_us_per_keyframe")}
            med["min_max"] = {k: [min(x[k] for x in rr), max(x[k] for x in rr)] for k in ("single_us", "batch_us_per_keyframe")}
            out["medians"][name][str(fac)] = med
            print("type %d %-11s depth %3d x %3d (factor %d)  single call %7.1f us (%d rows)   batch of %d, per keyframe %6.1f us "
                  "(%.1f rows); medians of %d rounds" % (ft, name, sizes[fac][0], sizes[fac][1], fac, med["single_us"], rr[0]["single_rows"],
                                                        n_kf, med["batch_us_per_keyframe"], rr[0]["batch_mean_rows"], a.rounds), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
