#!/usr/bin/env python3
"""The uint8 L2 descriptor route (sf_params.desc_type 2, 128-byte rows: global matching on the int8 matrix cores,
csrc/k_match_u8.hip) beside the float32 route (desc_type 1, 512-byte rows: exact L2 on the VALU) on the SAME integer rows:
n candidate pairs of K rows of 128 integers in 0 .. 255 (synth.u8_descriptors), resident in the store of one handle of
each kind, both of this build, in one process.  Timed: one verify call over all pairs (stage kernels: global matching,
motion estimation, guided matching, motion estimation), HIP events around `reps` calls, the two routes alternating,
medians over `rounds` rounds.  Then, in a pass of its own with the launches bracketed, the global matching kernel alone.
The records of the two routes must be the same bytes, and the first `check` equal the oracle asked with desc_type 1.
Writes profiles/l2u8_match.json.
usage: python tools/bench_l2u8.py [n_pairs=2048] [k=500] [check=24] [rounds=5]"""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402
from oracle import pyoracle  # noqa: E402

DIMS = 128


def params(n, k, u8):
    p = synth.camera_params()
    p.iterations = 500
    p.max_features = k
    p.store_capacity = 2 * n
    p.desc_type, p.desc_bytes = (2, DIMS) if u8 else (1, 4 * DIMS)
    return p


class Route:
    def __init__(self, name, n, k, u8, A, B):
        dev = torch.device("cuda:0")
        self.name, self.n = name, n
        self.p = params(n, k, u8)
        self.f = lib.SeparatorFinder(self.p, device=0)
        self.f.set_stream(torch.cuda.current_stream().cuda_stream)
        conv = (lambda fa: fa) if u8 else (lambda fa: _abi.FeatureArrays(fa.desc.astype(np.float32), fa.xyz, fa.kpts))
        sa = [self.f.store_add_keyframe(conv(a)) for a in A]
        sb = [self.f.store_add_keyframe(conv(b)) for b in B]
        self.d_from = torch.tensor(sa, dtype=torch.int32, device=dev)
        self.d_to = torch.tensor(sb, dtype=torch.int32, device=dev)
        self.d_out = torch.empty((n, _abi.RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)

    def call(self):
        self.f.verify_pairs_device(self.d_from.data_ptr(), self.d_to.data_ptr(), self.n, self.d_out.data_ptr())

    def timed(self, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            self.call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def match_kernel_ms(self, reps):
        self.f.prof_select(["k_match_global"])
        self.f.prof_enable(True)
        self.f.prof_reset()
        for _ in range(reps):
            self.call()
        torch.cuda.synchronize()
        launches, ms = self.f.prof_get()["k_match_global"]
        self.f.prof_enable(False)
        return ms / max(launches, 1), launches // reps

    def records(self):
        torch.cuda.synchronize()
        return np.frombuffer(self.d_out.cpu().numpy().tobytes(), dtype=_abi.RESULT_DTYPE)


def main():
    a = [int(x) for x in sys.argv[1:]]
    n, k, check, rounds = (a + [2048, 500, 24, 5][len(a):])[:4]
    reps = 5
    A, B, is_true, _ = synth.make_pairs(4242, n, k=k, cols=32, true_frac=0.2)       # (the frames of tools/bench_l2.py)
    rng = np.random.default_rng(7)
    A = [synth.u8_descriptors(x, DIMS, rng, 12) for x in A]
    B = [synth.u8_descriptors(x, DIMS, rng, 12) for x in B]
    routes = [Route("float32 x 128 (desc_type 1)", n, k, False, A, B), Route("uint8 x 128 (desc_type 2)", n, k, True, A, B)]
    try:
        for r in routes:
            for _ in range(2):
                r.call()
        torch.cuda.synchronize()
        times = {r.name: [] for r in routes}
        for _ in range(rounds):
            for r in routes:                                                         # alternating
                times[r.name].append(r.timed(reps))
        recs = [r.records() for r in routes]
        same_routes = int(sum(recs[0][i].tobytes() == recs[1][i].tobytes() for i in range(n)))
        q = params(n, k, False)
        twin = lambda fa: _abi.FeatureArrays(fa.desc.astype(np.float32), fa.xyz, fa.kpts)   # noqa: E731
        same_oracle = sum(int(recs[1][i].tobytes() == pyoracle.estimate_transform(q, twin(A[i]), twin(B[i])).tobytes())
                          for i in range(check))
        kern = {r.name: r.match_kernel_ms(reps) for r in routes}
    finally:
        for r in routes:
            r.f.close()
    out = {"n_pairs": n, "k": k, "dims": DIMS, "reps_per_round": reps, "rounds": rounds,
           "records_equal_between_routes": same_routes, "checked_against_oracle": check, "equal_to_oracle": same_oracle,
           "decisions_equal_ground_truth": int(((recs[1]["success"] != 0) == is_true).sum()), "routes": {}}
    for r in routes:
        med = statistics.median(times[r.name])
        out["routes"][r.name] = {"verify_ms_per_call_rounds": [round(t, 4) for t in times[r.name]], "verify_ms_median": round(med, 4),
                                 "pairs_per_s": round(n / (med * 1e-3)), "match_kernel_ms_per_launch": round(kern[r.name][0], 4),
                                 "match_launches_per_call": kern[r.name][1]}
        print("%-30s %5d pairs x K = %d: %8.3f ms per verify call (median of %d) = %9.0f pairs/s; global matching %8.3f ms per launch"
              % (r.name, n, k, med, rounds, n / (med * 1e-3), kern[r.name][0]))
    print("records equal between the routes: %d / %d; first %d equal to the oracle: %d" % (same_routes, n, check, same_oracle))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "l2u8_match.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
