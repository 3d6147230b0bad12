"""What a keyframe costs with each of the two stereo correspondences -- pyramidal LK (Stereo/OpticalFlow true,
csrc/k_lk.hip) and block matching (false, csrc/k_stereo_bm.hip; SSD and SAD) -- on 752 x 480 stereo pairs, 1 000
corners, rtabmap's Stereo/* defaults (15 x 3 window, 5 levels, 30 iterations, disparities (0.5, 128]), under
Vis/FeatureType 6 (GFTT/BRIEF) and 4 (FAST/BRIEF):
  single  sf_get_features_and_descriptor on host images (upload, detector, stereo correspondence, extraction,
          download): a wall-clock figure of a synchronous call, per keyframe
  batch   sf_get_features_and_descriptor_batch_device on 64 device pairs, HIP events around the launches, per keyframe
The three settings alternate inside every round of one process on the same images; every figure is the median over
--rounds rounds with the spread (min .. max) beside it.  The figures are whole keyframes: the difference between two
settings is the difference between their stereo stages.  The store is emptied every 16 batches / 512 single calls, which
waits for the stream once.
usage: python tools/stereo_bm_latency.py [--features 1000] [--reps 300] [--batch-reps 100] [--rounds 5] [--out FILE]"""
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

TYPES = (("gftt_brief", 6), ("fast_brief", 4))
SETTINGS = (("lk", (1, 1)), ("bm_ssd", (0, 1)), ("bm_sad", (0, 0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--batch-reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, n_kf = a.features, 64
    p = synth.camera_params()
    p.max_features = max(1024, n)
    p.store_capacity = 17 * n_kf + 600
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    pairs = [tuple(np.ascontiguousarray(x) for x in ec.make_stereo_pair(800 + i, pad=0)[:2]) for i in range(n_kf)]
    h, w = pairs[0][0].shape
    L = torch.from_numpy(np.stack([l for l, _ in pairs]).reshape(n_kf, -1)).to(dev)
    R = torch.from_numpy(np.stack([r for _, r in pairs]).reshape(n_kf, -1)).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(n)
    rows_dev = torch.zeros(n_kf, dtype=torch.int32, device=dev)

    def single_us(reps):
        f.store_clear()
        for i in range(3):
            f.get_features_and_descriptor(*pairs[i], cam, det)
        t0 = time.perf_counter()
        for i in range(reps):
            f.get_features_and_descriptor(*pairs[i % n_kf], cam, det)
            if (i + 1) % 512 == 0:
                f.store_clear()
        return (time.perf_counter() - t0) * 1e6 / reps

    def batch_us(reps):
        def run():
            f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, cam, det,
                                                       d_rows_out=rows_dev.data_ptr())
        f.store_clear()
        run()
        run()
        f.store_clear()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            run()
            if (i + 1) % 16 == 0:
                f.store_clear()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps / n_kf

    rounds = {(t, s): [] for t, _ in TYPES for s, _ in SETTINGS}
    rows = {}
    for r in range(a.rounds):
        for tname, ft in TYPES:
            f.set_feature_type(ft)
            for sname, (optical_flow, ssd) in SETTINGS:
                f.stereo_set_params(_abi.stereo_params(optical_flow, ssd))
                us_b = batch_us(a.batch_reps)
                rows[(tname, sname)] = float(rows_dev.cpu().numpy().mean())
                us_s = single_us(a.reps)
                rounds[(tname, sname)].append((us_s, us_b))
                print("round %d %-10s stereo %-7s single %7.1f us   batch of %d: %6.1f us per keyframe (%.0f rows on "
                      "average)" % (r, tname, sname, us_s, n_kf, us_b, rows[(tname, sname)]), flush=True)
    f.close()
    out = {"image": [w, h], "features": n, "batch": n_kf, "reps": a.reps, "batch_reps": a.batch_reps, "rounds": a.rounds,
           "cases": {}}
    for (tname, sname), v in rounds.items():
        v = np.array(v)
        case = {"batch_mean_rows": round(rows[(tname, sname)], 1)}
        for j, key in enumerate(("single_us", "batch_us_per_keyframe")):
            case[key] = round(float(np.median(v[:, j])), 2)
            case[key + "_min_max"] = [round(float(v[:, j].min()), 2), round(float(v[:, j].max()), 2)]
        out["cases"]["%s %s" % (tname, sname)] = case
        print("%-10s stereo %-7s median of %d rounds: single %.1f us, batch %.1f us per keyframe" % (
            tname, sname, a.rounds, case["single_us"], case["batch_us_per_keyframe"]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
