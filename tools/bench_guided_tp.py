#!/usr/bin/env python3
"""Cost of Vis/CorGuessMatchToProjection = true (k_guided_tp) against the default sub-branch (k_guided) on configs[1]-
shaped candidates: 10 000 pairs of K = 500 keypoints with 256-bit descriptors, 20 % true revisits, both handles on the
stage kernels (SF_FUSED=0) in one process, the two verify calls alternating.  Reports the call time of each and the
per-launch time of the two guided kernels (hipEvents around each launch), and writes profiles/guided_tp_bench.json.
usage: python tools/bench_guided_tp.py [--pairs 10000] [--k 500] [--reps 10] [--out profiles/guided_tp_bench.json]
(under `rocprofv3 --kernel-trace --stats`, pass --reps 3 --no-prof: the kernel trace then times the launches.)"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
os.environ["SF_FUSED"] = "0"          # both flags on the stage kernels (read at sf_create)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--kf", type=int, default=2500, help="keyframes per robot (pairs cycle over them)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_tp_bench.json"))
    a = ap.parse_args()
    n, k, n_kf = a.pairs, a.k, min(a.kf, a.pairs)
    feats = synth.make_store_batch(20261016, n_kf, k=k, cols=32, true_frac=0.2)
    dev = torch.device("cuda:0")
    T = {key: torch.from_numpy(np.ascontiguousarray(feats[key]).view(np.uint8) if feats[key].dtype.fields else
                               np.ascontiguousarray(feats[key])).to(dev)
         for key in ("desc_a", "xyz_a", "kp_a", "desc_b", "xyz_b", "kp_b")}
    handles, d_io = [], []
    for flag in (0, 1):
        p = synth.camera_params()
        p.max_features = k
        p.store_capacity = 2 * n_kf
        p.guess_match_to_projection = flag
        f = lib.SeparatorFinder(p, device=0)
        f.set_stream(torch.cuda.current_stream().cuda_stream)
        sa = f.store_add_keyframes_device(n_kf, k, 32, T["desc_a"].data_ptr(), T["xyz_a"].data_ptr(), T["kp_a"].data_ptr())
        sb = f.store_add_keyframes_device(n_kf, k, 32, T["desc_b"].data_ptr(), T["xyz_b"].data_ptr(), T["kp_b"].data_ptr())
        idx = np.arange(n) % n_kf
        d_from = torch.tensor(sa + idx, dtype=torch.int32, device=dev)
        d_to = torch.tensor(sb + idx, dtype=torch.int32, device=dev)
        d_out = torch.empty((n, _abi.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        handles.append(f)
        d_io.append((d_from, d_to, d_out))
    torch.cuda.synchronize()

    def call(j):
        d_from, d_to, d_out = d_io[j]
        handles[j].verify_pairs_device(d_from.data_ptr(), d_to.data_ptr(), n, d_out.data_ptr())

    for j in (0, 1):                       # warm-up: workspaces, code objects
        call(j); call(j)
    torch.cuda.synchronize()
    if not a.no_prof:
        for f in handles:
            f.prof_select(["k_guided", "k_guided_tp"])
            f.prof_reset()
            f.prof_enable(True)
    ms = [[], []]
    for _ in range(a.reps):
        for j in (0, 1):                   # alternating, one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(j); e1.record()
            torch.cuda.synchronize()
            ms[j].append(e0.elapsed_time(e1))
    res = [np.frombuffer(d_io[j][2].cpu().numpy().tobytes(), dtype=_abi.RESULT_DTYPE) for j in (0, 1)]
    out = {"pairs": n, "k": k, "desc_bits": 256, "keyframes_per_robot": n_kf, "reps": a.reps, "form": "stages (SF_FUSED=0)",
           "call_ms": {}, "guided_launch_ms": {}, "pass2_guided": int(res[1]["pass2_guided"].sum()),
           "success": {"flag0": int(res[0]["success"].sum()), "flag1": int(res[1]["success"].sum())},
           "records_differing": int(sum(res[0][i].tobytes() != res[1][i].tobytes() for i in range(n)))}
    for j, name in ((0, "flag0"), (1, "flag1")):
        v = np.array(ms[j])
        out["call_ms"][name] = {"mean": float(v.mean()), "median": float(np.median(v)), "min": float(v.min()),
                                "max": float(v.max())}
    if not a.no_prof:
        for j, kname in ((0, "k_guided"), (1, "k_guided_tp")):
            launches, total = handles[j].prof_get()[kname]
            out["guided_launch_ms"][kname] = {"launches": launches, "mean": total / max(launches, 1)}
        g0 = out["guided_launch_ms"]["k_guided"]["mean"]
        out["ratio_tp_over_guided"] = out["guided_launch_ms"]["k_guided_tp"]["mean"] / g0 if g0 > 0 else None
    for f in handles:
        f.close()
    print(json.dumps(out))
    if not a.no_prof:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
