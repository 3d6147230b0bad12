"""Latency of FAST/BRIEF keyframes (Vis/FeatureType 4) against GFTT/BRIEF (6) on 752 x 480 stereo pairs, 1 000 features:
  detect  the detector alone on one image: sf_detect_fast_device (4) / sf_detect_corners_device (6); both wait for the
          host twice, so this is a wall-clock figure of a synchronous call (HIP events around it agree)
  single  sf_extract_keyframe_device with given corners (the same code under both types: the sanity figure that
          profiles/orb_latency.json recorded as "brief")
  batch   sf_get_features_and_descriptor_batch_device on 64 stereo pairs (detector + stereo flow + extraction), per
          keyframe
The two types alternate in one process over --rounds rounds on the same images; every figure is the median over the
rounds, the spread (min .. max) is kept beside it.  Prints one line per round and writes JSON to --out.
Every timed window is about a second (5 000 detector calls, 20 000 extractions, 400 batches); the store is emptied
every 1 000 extractions / 16 batches, which waits for the stream once (a few microseconds per 40 ms of work).
usage: python tools/fast_latency.py [--features 1000] [--detect-reps 5000] [--reps 20000] [--batch-reps 400]
                                    [--rounds 5] [--out FILE]
       --profile [--only 4|6]: --batch-reps batches per type and nothing else, untimed (the workload of a rocprofv3
       run; one type per process keeps the shared sort kernels of the two apart)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402
from tests import extract_cases as ec  # noqa: E402

KINDS = (("fast_brief", 4), ("gftt_brief", 6))


def timed(fn, reps, warm=3, every=0, between=None):
    """us per call; `between` (the store's clear, which waits for the stream) runs after every `every` calls."""
    for _ in range(warm):
        fn()
    if between:
        between()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn()
        if every and (i + 1) % every == 0:
            between()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--detect-reps", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=20000)
    ap.add_argument("--batch-reps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--only", type=int, default=0, help="with --profile: this feature type alone (4 or 6)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.features
    image, kp, rx, st, cam = ec.make_case(3, n=n, pad=0)
    kp["octave"] = 0
    h, w = image.shape
    n_kf = 64
    p = synth.camera_params()
    p.max_features = max(1024, n)
    p.store_capacity = 1000 + 19 * n_kf + 64          # (emptied every 1 000 extractions / 16 batches)
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    d_kp = torch.from_numpy(kp.view(np.uint8)).to(dev)
    d_rx = torch.from_numpy(rx).to(dev)
    d_st = torch.from_numpy(st).to(dev)
    pairs = [ec.make_stereo_pair(800 + i, pad=0)[:2] for i in range(n_kf)]
    L = torch.from_numpy(np.stack([np.ascontiguousarray(l) for l, _ in pairs]).reshape(n_kf, -1)).to(dev)
    R = torch.from_numpy(np.stack([np.ascontiguousarray(r) for _, r in pairs]).reshape(n_kf, -1)).to(dev)
    d_img = L[0]                                      # the detector's image: the first left image of the batch
    d_case = torch.from_numpy(np.ascontiguousarray(image)).to(dev)   # the extraction's: the one its corners were made for
    bcam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(n)
    rows_dev = torch.zeros(n_kf, dtype=torch.int32, device=dev)
    d_det = torch.zeros((n, 28), dtype=torch.uint8, device=dev)
    found = {}

    def detect(ft):
        if ft == 4:
            found[ft] = f.detect_fast_device(d_img.data_ptr(), w, h, w, n, d_det.data_ptr(), n)
        else:
            found[ft] = f.detect_corners_device(d_img.data_ptr(), w, h, w, n, det.quality_level, det.min_distance,
                                                d_det.data_ptr(), n)

    def single():
        f.extract_keyframe_device(d_case.data_ptr(), w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), n, cam,
                                  want_rows=False)

    def batch():
        f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, bcam, det,
                                                   d_rows_out=rows_dev.data_ptr())

    if a.profile:
        for name, ft in KINDS:
            if a.only and ft != a.only:
                continue
            f.set_feature_type(ft)
            f.store_clear()
            for i in range(a.batch_reps):
                batch()
                if (i + 1) % 16 == 0:
                    f.store_clear()
            torch.cuda.synchronize()
            print("%s: %d batches of %d" % (name, a.batch_reps, n_kf), flush=True)
        f.close()
        return
    rounds = {name: [] for name, _ in KINDS}
    rows_mean = {}
    for r in range(a.rounds):
        for name, ft in KINDS:
            f.set_feature_type(ft)
            f.store_clear()
            us_detect = timed(lambda: detect(ft), a.detect_reps)
            us_single = timed(single, a.reps, every=1000, between=f.store_clear)
            f.store_clear()
            us_batch = timed(batch, a.batch_reps, warm=2, every=16, between=f.store_clear) / n_kf
            rows_mean[name] = float(rows_dev.cpu().numpy().mean())
            rounds[name].append((us_detect, us_single, us_batch))
            print("round %d %-11s detect %7.1f us (%d corners)   single extract %6.1f us   batch of %d: %6.1f us per "
                  "keyframe (%.0f rows on average)" % (r, name, us_detect, found[ft], us_single, n_kf, us_batch,
                                                       rows_mean[name]), flush=True)
    f.close()
    out = {"image": [w, h], "features": n, "batch": n_kf, "detect_reps": a.detect_reps, "reps": a.reps,
           "batch_reps": a.batch_reps, "rounds": a.rounds, "cases": {}}
    for name, _ in KINDS:
        v = np.array(rounds[name])
        case = {"corners_detected": int(found[dict(KINDS)[name]]), "batch_mean_rows": round(rows_mean[name], 1)}
        for j, key in enumerate(("detect_us", "single_us", "batch_us_per_keyframe")):
            case[key] = round(float(np.median(v[:, j])), 2)
            case[key + "_min_max"] = [round(float(v[:, j].min()), 2), round(float(v[:, j].max()), 2)]
        out["cases"][name] = case
        print("%-11s median of %d rounds: detect %.1f us, single extract %.1f us, batch %.1f us per keyframe" % (
            name, a.rounds, case["detect_us"], case["single_us"], case["batch_us_per_keyframe"]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
