"""Latency of one SIFT keyframe (Vis/FeatureType 1) against SURF (0), both on handles with desc_type 1, on 752 x 480 stereo
pairs with 1 000 features, single calls, the two types alternating round by round in one process:
  detect   the detector call alone on a device image (sf_detect_surf_device / sf_detect_sift_device); it waits for the
           keypoint count (SIFT: for the count of extrema too), so it is timed by the wall clock
  extract  sf_extract_keyframe_device on that detector's keypoints (SURF: integral image, descriptors; SIFT: the pyramid
           built again, descriptors; 3D points, commit), asynchronous calls back to back, HIP events
  full     sf_get_features_and_descriptor on host images (upload, detector, LK, extraction, download), wall clock
Prints one line per type with the medians over the rounds and writes all rounds as JSON to --out.

With --batch-json FILE the tool times the batch form of SIFT instead, per keyframe, on --batch (64) pairs of 752 x 480 with
--features (1 000) features, the forms alternating round by round in one process, wall clock, every timed span ended by a
synchronise:
  single_host    --batch calls of sf_get_features_and_descriptor on host images (upload and download included): the
                 basis of comparison, measured in the same run
  batch          ONE sf_get_features_and_descriptor_sift_batch_device on device images
and writes the medians of --rounds (5) rounds, the rounds themselves and the batch's plan (sf_sift_batch_plan) to FILE.
usage: python tools/sift_latency.py [--features 1000] [--reps 20] [--rounds 5] [--out FILE]
       python tools/sift_latency.py --batch-json FILE [--batch 64] [--batch-reps 3] [--rounds 5] [--features 1000]"""
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


def batch_main(a):
    dev = torch.device("cuda:0")
    n_kf, maxf = a.batch, a.features
    distinct = [tuple(np.ascontiguousarray(x) for x in ec.make_stereo_pair(800 + i, pad=0)[:2]) for i in range(min(8, n_kf))]
    pairs = [distinct[i % len(distinct)] for i in range(n_kf)]
    h, w = pairs[0][0].shape
    p = synth.camera_params()
    p.max_features = max(1024, maxf)
    p.store_capacity = 2 * n_kf + 8
    p.desc_type, p.desc_bytes = 1, 512
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    f.set_feature_type_sift()
    L = torch.from_numpy(np.stack([q[0].reshape(-1) for q in pairs])).to(dev)
    R = torch.from_numpy(np.stack([q[1].reshape(-1) for q in pairs])).to(dev)
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(maxf)
    d_rows = torch.zeros((n_kf,), dtype=torch.int32, device=dev)

    def single_host():
        for l, r in pairs:
            f.get_features_and_descriptor(l, r, cam, det)

    def batch():
        f.get_features_and_descriptor_sift_batch_device(L.data_ptr(), R.data_ptr(), n_kf, w, h, w, w * h, cam, det, None,
                                                        d_rows.data_ptr())

    def ms_per_keyframe(fn, reps):
        f.store_clear()
        fn()                                            # warm: buffers, the sorts' temporary storage, the blur tables
        torch.cuda.synchronize()
        f.store_clear()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            f.store_clear()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (reps * n_kf)

    forms = (("single_host", single_host, 1), ("batch", batch, a.batch_reps))
    per_round = {name: [] for name, _, _ in forms}
    for r in range(a.rounds):
        for name, fn, reps in forms:
            per_round[name].append(ms_per_keyframe(fn, reps))
        print("round %d: %s" % (r, "   ".join("%s %.4f" % (name, per_round[name][-1]) for name, _, _ in forms)), flush=True)
    batch()
    overflowed = f.sift_batch_status(check=False)
    rows_batch = d_rows.cpu().numpy().tolist()
    f.store_clear()
    rows_single = [len(f.get_features_and_descriptor(l, r, cam, det)[0]) for l, r in pairs[:len(distinct)]]
    f.close()
    cap_img, chunk, workspace = lib.sift_batch_plan(w, h, n_kf)
    report = {"tool": "tools/sift_latency.py --batch-json", "image": [w, h], "features": maxf, "batch": n_kf,
              "rounds": a.rounds, "batch_reps": a.batch_reps, "unit": "ms per keyframe, wall clock",
              "plan": {"cap_img": cap_img, "chunk": chunk, "workspace_bytes": workspace}, "overflowed": overflowed,
              "rows_single": rows_single, "rows_batch": rows_batch[:len(distinct)],
              "forms": {name: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": v}
                        for name, v in per_round.items()}}
    print(json.dumps({n: v["median"] for n, v in report["forms"].items()}), flush=True)
    with open(a.batch_json, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-json", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.batch_json:
        return batch_main(a)
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
