"""Latency of sf_depth_register_device on uint16 depth images, both fills on, at two shapes: 640 x 480 -> 752 x 480 and
848 x 480 -> 1280 x 720 (a sloped plane with a box in front and 5 % holes, the colour camera 8 cm to the side and turned by
one degree: tests/depth_register_ref.py), the forms alternating round by round in one process on one handle:
  single  one image per call
  batch   64 images per call, per image
  call    the whole call: the z-buffer's initialisation, the scatter, the resolve with the fill
  init / scatter / resolve   each stage alone (sf_debug_depth_register_limits), HIP events around `reps` calls of it.  The
          scatter alone runs on keys that earlier repetitions have already lowered: every atomic is still issued, to the same
          addresses
  copy    one hipMemcpyAsync (device to device) of the bytes the call reads plus writes, 2 dw dh + 2 W H per image
Prints the medians over the rounds and writes all rounds as JSON to --out.  One run on one machine: no claim beyond it.
usage: python tools/depth_register_latency.py [--reps 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import lib, synth  # noqa: E402
from tests import depth_register_ref as ref  # noqa: E402

SHAPES = ((640, 480, 752, 480), (848, 480, 1280, 720))
STAGES = (("call", 0), ("init", 1), ("scatter", 2), ("resolve", 4))


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
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n_img = 64
    f = lib.SeparatorFinder(synth.camera_params(), device=0)
    stream = torch.cuda.current_stream().cuda_stream
    f.set_stream(stream)
    out = {"format": "uint16 millimetres", "fill": "vertical + horizontal", "batch": n_img, "reps": a.reps, "rounds": a.rounds, "shapes": []}
    for dw, dh, W, H in SHAPES:
        reg = ref.case_registration(dw, dh, W, H, 1, 1)
        block = ref.abi(reg)
        scene = ref.scene(dw, dh, 70, ref.U16)
        stats = ref.fill_stats(ref.register_unfilled(scene, reg), ref.register(scene, reg))
        d_in = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(scene, (n_img, dh, dw))).view(np.int16)).to(dev)
        d_out = torch.zeros((n_img, H, W), dtype=torch.int16, device=dev)
        image_bytes = 2 * dw * dh + 2 * W * H
        copy_src = torch.zeros(n_img * image_bytes, dtype=torch.uint8, device=dev)
        copy_dst = torch.zeros_like(copy_src)

        def register(n):
            f.depth_register_device(block, d_in.data_ptr(), ref.U16, 2 * dw, 2 * dw * dh, n, d_out.data_ptr(), 2 * W, 2 * W * H)

        def copy(n):
            assert f._L.sf_memcpy_device_async(f._h, copy_dst.data_ptr(), copy_src.data_ptr(), n * image_bytes, stream) == 0
        shape = {"depth": [dw, dh], "registered": [W, H], "bytes_per_image": image_bytes, "key_bytes_per_image": 4 * W * H,
                 "collisions": ref.collisions(scene, reg), "pixels_filled": stats[0], "pixels_replaced": stats[1], "runs": []}
        register(1)
        torch.cuda.synchronize()
        assert d_out[0].cpu().numpy().view(np.uint16).tobytes() == ref.register(scene, reg).tobytes()      # what is timed is the call
        for _ in range(a.rounds):
            r = {}
            for name, stages in STAGES:
                f.debug_depth_register_limits(0, stages)
                r[name + "_single_us"] = round(events(lambda: register(1), a.reps), 2)
                r[name + "_batch_us_per_image"] = round(events(lambda: register(n_img), a.reps) / n_img, 3)
            f.debug_depth_register_limits(0, 0)
            r["copy_single_us"] = round(events(lambda: copy(1), a.reps), 2)
            r["copy_batch_us_per_image"] = round(events(lambda: copy(n_img), a.reps) / n_img, 3)
            shape["runs"].append(r)
        keys = list(shape["runs"][0])
        med = {k: float(np.median([x[k] for x in shape["runs"]])) for k in keys}
        shape["medians"] = med
        shape["min_max"] = {k: [min(x[k] for x in shape["runs"]), max(x[k] for x in shape["runs"])] for k in keys}
        shape["batch_ratio_to_copy"] = round(med["call_batch_us_per_image"] / med["copy_batch_us_per_image"], 2)
        # the scatter as a rate of atomic bytes (4 per point that lands), and its time against the key plane's initialisation
        shape["atomics_per_image"] = int(ref.project(scene, reg)[0].sum())
        shape["scatter_batch_atomic_gb_per_s"] = round(4 * shape["atomics_per_image"] / med["scatter_batch_us_per_image"] / 1e3, 1)
        shape["scatter_over_init_batch"] = round(med["scatter_batch_us_per_image"] / med["init_batch_us_per_image"], 2)
        out["shapes"].append(shape)
        print("%d x %d -> %d x %d, single: call %.1f us (init %.1f, scatter %.1f, resolve %.1f), copy %.1f us" % (
            dw, dh, W, H, med["call_single_us"], med["init_single_us"], med["scatter_single_us"], med["resolve_single_us"], med["copy_single_us"]))
        print("  batch of %d, per image: call %.2f us (init %.2f, scatter %.2f, resolve %.2f), copy %.2f us, ratio %.2f; medians of %d rounds" % (
            n_img, med["call_batch_us_per_image"], med["init_batch_us_per_image"], med["scatter_batch_us_per_image"],
            med["resolve_batch_us_per_image"], med["copy_batch_us_per_image"], shape["batch_ratio_to_copy"], a.rounds), flush=True)
        del d_in, d_out, copy_src, copy_dst
    f.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
