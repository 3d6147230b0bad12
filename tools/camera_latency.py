#!/usr/bin/env python3
"""What a camera id per store slot costs a verification call: 10 000 candidate pairs of the bench shape (BASELINE
configs[1]: K = 500 features, 500 iterations, a fifth of the pairs true) through sf_verify_pairs_device,

  fused     all slots id 0, the handle's default launch form (what a store without camera ids runs);
  stages    all slots id 0, SF_OPT_FUSED = 0: the stage kernels;
  table     all slots tagged with a camera EQUAL to the handle's: the stage kernels' camera forms, same arithmetic,
            the camera read through the table (the results are checked to be the same bytes).

The three alternate, `--rounds` times; the medians go to profiles/camera_latency.json for the 3D-3D and the PnP
estimator.  stages against table is the cost of the table path itself, fused against stages the cost of leaving the
fused form.  Needs a GPU.

usage: python tools/camera_latency.py [--pairs 10000] [--base 2000] [--rounds 5] [--out profiles/camera_latency.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--base", type=int, default=2000, help="generated keyframe pairs (the pair list cycles over them)")
    ap.add_argument("--features", type=int, default=500)
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_latency.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from multi_robot_slam_separators_amd import _abi, lib, synth

    dev = torch.device("cuda:0")
    n, k = args.base, args.features
    feats = synth.make_store_batch(12345, n, k=k, cols=32, true_frac=0.2)
    T = {key: torch.from_numpy(np.ascontiguousarray(feats[key]).view(np.uint8) if feats[key].dtype.fields else
                               np.ascontiguousarray(feats[key])).to(dev)
         for key in ("desc_a", "xyz_a", "kp_a", "desc_b", "xyz_b", "kp_b")}
    idx = np.arange(args.pairs, dtype=np.int32) % n
    d_from, d_to = torch.from_numpy(idx).to(dev), torch.from_numpy(idx + n).to(dev)
    d_out = torch.zeros(args.pairs * _abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    report = {"pairs": args.pairs, "generated_pairs": n, "features": k, "iterations": args.iterations, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "estimators": {}}
    for name, est in (("3d3d", 0), ("pnp", 1)):
        p = synth.camera_params()
        p.iterations = args.iterations
        p.max_features = k
        p.estimation_type = est
        p.store_capacity = 2 * n
        with lib.SeparatorFinder(p, device=0) as f:
            f.set_stream(torch.cuda.current_stream().cuda_stream)
            f.store_add_keyframes_device(n, k, 32, T["desc_a"].data_ptr(), T["xyz_a"].data_ptr(), T["kp_a"].data_ptr())
            f.store_add_keyframes_device(n, k, 32, T["desc_b"].data_ptr(), T["xyz_b"].data_ptr(), T["kp_b"].data_ptr())
            cam = f.camera_add(f.camera_get(0))            # a model equal to the handle's own

            def run(form):
                f.set_option(_abi.SF_OPT_FUSED, 1 if form == "fused" else 0)
                f.store_set_camera(0, 2 * n, cam if form == "table" else 0)
                # (one pair, not timed: the call that follows a change of ids uploads them, once, and waits for the copy)
                f.verify_pairs_device(d_from.data_ptr(), d_to.data_ptr(), 1, d_out.data_ptr())
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f.verify_pairs_device(d_from.data_ptr(), d_to.data_ptr(), args.pairs, d_out.data_ptr())
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b), d_out.cpu().numpy().tobytes()

            forms = ("fused", "stages", "table")
            ref = {form: run(form)[1] for form in forms}            # warm-up; and the three forms agree byte for byte
            assert ref["fused"] == ref["stages"] == ref["table"], "the launch forms disagree"
            ms = {form: [] for form in forms}
            for _ in range(args.rounds):
                for form in forms:
                    ms[form].append(run(form)[0])
            accepted = int(np.frombuffer(ref["table"], dtype=_abi.RESULT_DTYPE)["success"].sum())
            report["estimators"][name] = {
                "accepted": accepted,
                **{form + "_ms": [round(v, 4) for v in ms[form]] for form in forms},
                **{"median_" + form + "_ms": round(statistics.median(ms[form]), 4) for form in forms}}
            print(name, {form: round(statistics.median(ms[form]), 4) for form in forms}, "ms; accepted", accepted)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
