"""Latency of one GFTT/FREAK keyframe (Vis/FeatureType 5) against GFTT/BRIEF (6) on a 752 x 480 image, the two types
alternating round by round in one process:
  single  sf_extract_keyframe_device with given corners (integral image, descriptors, 3D points, commit), asynchronous
          calls back to back, HIP events
  batch   sf_get_features_and_descriptor_batch_device on 64 stereo pairs (detector + stereo flow + extraction), per
          keyframe
The corners of the single case carry size 7 (scale 0 of the default pattern: a border of 23 pixels, close to BRIEF's 28).
Each type keeps a handle of its own (the store holds rows of one width).  Prints one line per type with the median over
the rounds and writes all rounds as JSON to --out.
usage: python tools/freak_latency.py [--corners 1000] [--reps 200] [--batch-reps 10] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402
from tests import extract_cases as ec  # noqa: E402

KINDS = (("brief", 6), ("freak", 5))


def timed(fn, reps, warm=3):
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
    ap.add_argument("--corners", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.corners
    image, kp, rx, st, cam = ec.make_case(3, n=n, pad=0)
    kp["size"] = 7.0
    h, w = image.shape
    n_kf = 64
    d_img = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
    d_kp = torch.from_numpy(kp.view(np.uint8)).to(dev)
    d_rx = torch.from_numpy(rx).to(dev)
    d_st = torch.from_numpy(st).to(dev)
    pairs = [ec.make_stereo_pair(800 + i, pad=0)[:2] for i in range(n_kf)]
    L = torch.from_numpy(np.stack([np.ascontiguousarray(l) for l, _ in pairs]).reshape(n_kf, -1)).to(dev)
    R = torch.from_numpy(np.stack([np.ascontiguousarray(r) for _, r in pairs]).reshape(n_kf, -1)).to(dev)
    bcam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    rows_dev = torch.zeros(n_kf, dtype=torch.int32, device=dev)
    handles = {}
    for name, ft in KINDS:
        p = synth.camera_params()
        p.max_features = max(1024, n)
        p.store_capacity = max(a.reps, a.batch_reps * n_kf) + 3 * n_kf + 64
        f = lib.SeparatorFinder(p, device=0)
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        if ft == 5:
            f.set_feature_type_freak(5)
        else:
            f.set_feature_type(ft)
        handles[name] = f
    out = {"image": [w, h], "corners": n, "batch": n_kf, "rounds": a.rounds, "cases": {name: [] for name, _ in KINDS}}
    for _ in range(a.rounds):
        for name, ft in KINDS:
            f = handles[name]
            f.store_clear()

            def single():
                f.extract_keyframe_device(d_img.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), n,
                                          cam, want_rows=False)
            us_single = timed(single, a.reps)
            _, kept = f.extract_keyframe_device(d_img.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(),
                                                d_st.data_ptr(), n, cam)
            f.store_clear()

            def batch():
                f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, bcam,
                                                           d_rows_out=rows_dev.data_ptr())
            us_batch = timed(batch, a.batch_reps, warm=2)
            rows = rows_dev.cpu().numpy()
            out["cases"][name].append({"single_us": round(us_single, 2), "single_kept": kept,
                                       "batch_us_per_keyframe": round(us_batch / n_kf, 2),
                                       "batch_mean_rows": round(float(rows.mean()), 1)})
    for name, _ in KINDS:
        r = out["cases"][name]
        print("%-6s single: %7.1f us per keyframe (%d of %d corners kept)   batch of %d: %7.1f us per keyframe (%.0f rows on "
              "average); medians of %d rounds" % (name, np.median([x["single_us"] for x in r]), r[0]["single_kept"], n, n_kf,
                                                  np.median([x["batch_us_per_keyframe"] for x in r]), r[0]["batch_mean_rows"],
                                                  a.rounds), flush=True)
    for f in handles.values():
        f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
