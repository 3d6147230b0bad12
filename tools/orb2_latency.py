"""Latency of ORB keyframes on a pyramid (Vis/FeatureType 2) against GFTT/ORB (8) on 752 x 480 stereo pairs, 1 000
features.  The single call:
  detect   the detector alone on one device image: sf_detect_orb_device (2) / sf_detect_corners_device (8); both wait
           for the host twice, so this is the duration of a synchronous call
  extract  sf_extract_keyframe_device on the detector's own keypoints (type 2: pyramid + one blur per level + rows on
           each keypoint's level; type 8: one blur + rows)
  handler  sf_get_features_and_descriptor on host images: upload, detector, stereo correspondence, extraction, download
The two types alternate in one process over --rounds rounds on the same images; every figure is the median over the
rounds with its spread (min .. max).  Prints one line per round and writes a text report to --out.

With --batch-json FILE the tool times the batch form instead, for score types 0 and 1, per keyframe, on --batch (64) pairs
in device memory (8 different pairs, repeated), wall clock from the first call to the end of the stream:
  single_host    --batch calls of sf_get_features_and_descriptor on host images (upload and download included)
  single_device  --batch times sf_detect_orb_device -> sf_stereo_correspondences_device -> sf_extract_keyframe_device on
                 device images: the single call without its copies
  batch          ONE sf_get_features_and_descriptor_orb_batch_device
  batch_type8    ONE sf_get_features_and_descriptor_batch_device under GFTT/ORB, as the scale
The four alternate in one process over --rounds rounds; the JSON holds every round and the medians.
usage: python tools/orb2_latency.py [--features 1000] [--detect-reps 300] [--reps 2000] [--handler-reps 100]
                                    [--rounds 5] [--score-type 0] [--out FILE]
       python tools/orb2_latency.py --batch-json FILE [--batch 64] [--batch-reps 5] [--rounds 5] [--features 1000]"""
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

KINDS = (("orb_pyramid", 2), ("gftt_orb", 8))


def timed(fn, reps, warm=3, every=0, between=None):
    """us per call (HIP events around the loop); `between` runs after every `every` calls."""
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
    return e0.elapsed_time(e1) * 1e3 / reps


def batch_main(a):
    dev = torch.device("cuda:0")
    n_kf, maxf = a.batch, a.features
    distinct = [tuple(np.ascontiguousarray(x) for x in ec.make_stereo_pair(800 + i, pad=0)[:2]) for i in range(min(8, n_kf))]
    pairs = [distinct[i % len(distinct)] for i in range(n_kf)]
    h, w = pairs[0][0].shape
    p = synth.camera_params()
    p.max_features = max(1024, maxf)
    p.store_capacity = 2 * n_kf + 8
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    L = torch.from_numpy(np.stack([q[0].reshape(-1) for q in pairs])).to(dev)
    R = torch.from_numpy(np.stack([q[1].reshape(-1) for q in pairs])).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(maxf)
    d_kp = torch.zeros((maxf, 28), dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((maxf, 2), dtype=torch.float32, device=dev)
    d_rx = torch.zeros((maxf,), dtype=torch.float32, device=dev)
    d_st = torch.zeros((maxf,), dtype=torch.uint8, device=dev)

    def single_host():
        for l, r in pairs:
            f.get_features_and_descriptor(l, r, cam, det)

    def single_device():
        for i in range(n_kf):
            l, r = L[i].data_ptr(), R[i].data_ptr()
            k = min(f.detect_orb_device(l, w, h, w, maxf, d_kp.data_ptr(), maxf), maxf)
            f.stereo_correspondences_device(l, r, w, h, w, d_kp.data_ptr(), k, d_xy.data_ptr(), d_st.data_ptr(),
                                            d_rx.data_ptr())
            f.extract_keyframe_device(l, w, h, w, d_kp.data_ptr(), d_rx.data_ptr(), d_st.data_ptr(), k, cam, want_rows=False)

    def batch():
        f.get_features_and_descriptor_orb_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, cam, det)

    def batch_type8():
        f.get_features_and_descriptor_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, cam, det)

    def ms_per_keyframe(fn, reps):
        f.store_clear()
        fn()                                            # warm: buffers, the sorts' temporary storage
        torch.cuda.synchronize()
        f.store_clear()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            f.store_clear()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (reps * n_kf)

    report = {"tool": "tools/orb2_latency.py --batch-json", "image": [w, h], "features": maxf, "batch": n_kf,
              "rounds": a.rounds, "batch_reps": a.batch_reps, "unit": "ms per keyframe, wall clock", "score_types": {}}
    for score_type in (0, 1):
        forms = (("single_host", single_host, 2, 1), ("single_device", single_device, 2, 1), ("batch", batch, 2, a.batch_reps),
                 ("batch_type8", batch_type8, 8, a.batch_reps))
        per_round = {name: [] for name, _, _, _ in forms}
        for r in range(a.rounds):
            for name, fn, ft, reps in forms:
                if ft == 2:
                    f.set_feature_type_orb(_abi.orb_detector_params(score_type=score_type))
                else:
                    f.set_feature_type(ft)
                per_round[name].append(ms_per_keyframe(fn, reps))
            print("score type %d round %d: %s" % (score_type, r, "   ".join(
                "%s %.4f" % (name, per_round[name][-1]) for name, _, _, _ in forms)), flush=True)
        report["score_types"][str(score_type)] = {
            name: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": v}
            for name, v in per_round.items()}
    f.close()
    print(json.dumps({k: {n: v["median"] for n, v in d.items()} for k, d in report["score_types"].items()}), flush=True)
    with open(a.batch_json, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-json", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--detect-reps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--handler-reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--score-type", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.batch_json:
        return batch_main(a)
    dev = torch.device("cuda:0")
    n = a.features
    left, right, _ = ec.make_stereo_pair(800, pad=0)
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    p = synth.camera_params()
    p.max_features = max(1024, n)
    p.store_capacity = 1064
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    d_img = torch.from_numpy(left).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(n)
    d_kp = torch.zeros((n, 28), dtype=torch.uint8, device=dev)
    found = {}

    def select(ft):
        if ft == 2:
            f.set_feature_type_orb(_abi.orb_detector_params(score_type=a.score_type))
        else:
            f.set_feature_type(ft)

    def detect(ft):
        if ft == 2:
            found[ft] = f.detect_orb_device(d_img.data_ptr(), w, h, w, n, d_kp.data_ptr(), n)
        else:
            found[ft] = f.detect_corners_device(d_img.data_ptr(), w, h, w, n, det.quality_level, det.min_distance,
                                                d_kp.data_ptr(), n)

    def extract(ft):
        f.extract_keyframe_device(d_img.data_ptr(), w, h, w, d_kp.data_ptr(), None, None, min(found[ft], n), cam,
                                  want_rows=False)

    def handler():
        f.get_features_and_descriptor(left, right, cam, det)

    def wall(fn, reps):
        fn()
        f.store_clear()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e6 / reps

    rounds = {name: [] for name, _ in KINDS}
    rows = {}
    for r in range(a.rounds):
        for name, ft in KINDS:
            select(ft)
            f.store_clear()
            us_detect = timed(lambda: detect(ft), a.detect_reps)
            us_extract = timed(lambda: extract(ft), a.reps, every=1000, between=f.store_clear)
            f.store_clear()
            us_handler = wall(handler, a.handler_reps)
            rows[name] = len(f.get_features_and_descriptor(left, right, cam, det)[0])
            f.store_clear()
            rounds[name].append((us_detect, us_extract, us_handler))
            print("round %d %-11s detect %7.1f us (%d keypoints)   extract %6.1f us   host handler %7.1f us (%d rows)" % (
                r, name, us_detect, found[ft], us_extract, us_handler, rows[name]), flush=True)
    f.close()
    lines = ["tools/orb2_latency.py: %d x %d, %d features, score type %d, %d rounds (detect %d, extract %d, handler %d calls "
             "per round); median [min .. max] in us" % (w, h, n, a.score_type, a.rounds, a.detect_reps, a.reps, a.handler_reps)]
    for name, ft in KINDS:
        v = np.array(rounds[name])
        cells = ["%s %.1f [%.1f .. %.1f]" % (key, np.median(v[:, j]), v[:, j].min(), v[:, j].max())
                 for j, key in enumerate(("detect", "extract", "handler"))]
        lines.append("%-11s (Vis/FeatureType %d, %d keypoints, %d rows): %s" % (name, ft, found[ft], rows[name], "   ".join(cells)))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
