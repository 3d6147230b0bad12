"""Latency of a keyframe from the camera's rgb8 images against the parent's path, 752 x 480 stereo pairs + one rgb image,
1 000 features, a 64-cluster / 4096-wide NetVLAD model of random weights:
  single  u8      sf_get_features_and_descriptor_u8 on the host rgb8 pair + the network on the uploaded rgb8 image
                  (upload of uint8, sf_netvlad_infer_u8_batch_device)
          parent  a NumPy colour-to-gray of both images on the host (tests/image_ref.gray) + sf_get_features_and_descriptor,
                  a NumPy float32 conversion of the rgb image + upload of float32 + sf_netvlad_infer_batch_device
  batch   u8      sf_add_keyframes_u8_batch_device on 64 keyframes already in device memory as rgb8, per keyframe
          parent  the same 64 keyframes from host rgb8: NumPy gray of 128 images, NumPy float32 of 64, their uploads,
                  sf_get_features_and_descriptor_batch_device + sf_netvlad_infer_batch_device +
                  sf_nn_append_local_f32_device, per keyframe.  The u8 side's upload of the rgb8 bytes is timed too
                  ("u8+upload"), so that both sides start from host memory.
Wall-clock per call (the host conversions are host work), the two sides alternating in one process over --rounds
rounds; every figure is the median over the rounds with its spread (min .. max).  Writes a text report to --out.
usage: python tools/u8_latency.py [--features 1000] [--reps 20] [--batch-reps 3] [--rounds 5] [--batch 64] [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from multi_robot_slam_separators_amd import _abi, lib, synth  # noqa: E402
from oracle import netvlad_torch  # noqa: E402
from tests import extract_cases as ec  # noqa: E402
from tests import image_ref  # noqa: E402

RGB8 = _abi.SF_IMAGE_RGB8


def colour(gray, seed):
    rng = np.random.default_rng(seed)
    g = np.asarray(gray, np.int32)
    rgb = np.stack([g + 40, g, g - 50], axis=-1) + rng.integers(-20, 21, size=g.shape + (3,))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def wall(fn, reps, after=None):
    fn()
    if after:
        after()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) * 1e6 / reps
    if after:
        after()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--pca-dim", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nb = a.features, a.batch
    left, right, _ = ec.make_stereo_pair(800, pad=0)
    h, w = left.shape
    L, R, C3 = colour(left, 1), colour(right, 2), colour(left[::-1], 3)
    p = synth.camera_params()
    p.max_features = max(1024, n)
    p.store_capacity = 2 * nb + 64
    p.netvlad_dimensions = 128
    f = lib.SeparatorFinder(p, device=0)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    f.netvlad_load(netvlad_torch.random_weights(3, clusters=64, pca_dim=a.pca_dim))
    cam = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11)
    det = _abi.detector_params(n)
    dims = p.netvlad_dimensions
    d_out = torch.zeros((nb, dims), dtype=torch.float32, device=dev)

    def clear():
        f.store_clear()
        f.nn_reset()

    def single_u8():
        f.get_features_and_descriptor_u8(L, R, RGB8, cam, det)
        d = torch.from_numpy(C3).to(dev)
        f.netvlad_infer_u8_batch_device(d.data_ptr(), RGB8, 1, w, h, 3 * w, 3 * w * h, d_out.data_ptr(), dims)
        f.nn_append_local_device(d_out.data_ptr(), 1, dims)
        torch.cuda.synchronize()

    def single_parent():
        f.get_features_and_descriptor(image_ref.gray(L, RGB8), image_ref.gray(R, RGB8), cam, det)
        d = torch.from_numpy(C3.astype(np.float32)).to(dev)
        f.netvlad_infer_batch_device(d.data_ptr(), 1, w, h, d_out.data_ptr(), dims)
        f.nn_append_local_device(d_out.data_ptr(), 1, dims)
        torch.cuda.synchronize()

    Lb, Rb, Cb = (np.ascontiguousarray(np.broadcast_to(x, (nb,) + x.shape)) for x in (L, R, C3))
    d_Lb, d_Rb, d_Cb = (torch.from_numpy(x).to(dev) for x in (Lb, Rb, Cb))

    def batch_u8():
        f.add_keyframes_u8_batch_device(d_Lb.data_ptr(), d_Rb.data_ptr(), d_Cb.data_ptr(), RGB8, nb, w, h, 3 * w, 3 * w * h,
                                        cam, det)
        torch.cuda.synchronize()

    def batch_u8_upload():
        l, r, c = (torch.from_numpy(x).to(dev) for x in (Lb, Rb, Cb))
        f.add_keyframes_u8_batch_device(l.data_ptr(), r.data_ptr(), c.data_ptr(), RGB8, nb, w, h, 3 * w, 3 * w * h, cam, det)
        torch.cuda.synchronize()

    def batch_parent():
        gl = torch.from_numpy(image_ref.gray(Lb, RGB8)).to(dev)
        gr = torch.from_numpy(image_ref.gray(Rb, RGB8)).to(dev)
        fl = torch.from_numpy(Cb.astype(np.float32)).to(dev)
        f.get_features_and_descriptor_batch_device(gl.data_ptr(), gr.data_ptr(), nb, w, h, w, w * h, cam, det)
        f.netvlad_infer_batch_device(fl.data_ptr(), nb, w, h, d_out.data_ptr(), dims)
        f.nn_append_local_device(d_out.data_ptr(), nb, dims)
        torch.cuda.synchronize()

    kinds = (("single u8", single_u8, a.reps, 1), ("single parent", single_parent, a.reps, 1),
             ("batch u8", batch_u8, a.batch_reps, nb), ("batch u8+upload", batch_u8_upload, a.batch_reps, nb),
             ("batch parent", batch_parent, a.batch_reps, nb))
    rounds = {name: [] for name, _, _, _ in kinds}
    for r in range(a.rounds):
        for name, fn, reps, per in kinds:
            us = wall(fn, reps, after=clear) / per
            rounds[name].append(us)
            print("round %d %-16s %9.1f us per keyframe" % (r, name, us), flush=True)
    f.close()
    lines = ["tools/u8_latency.py: %d x %d rgb8, %d features, NetVLAD 64 clusters / %d outputs, batch of %d, %d rounds "
             "(single %d, batch %d calls per round); wall clock, median [min .. max] in us per keyframe" % (
                 w, h, n, a.pca_dim, nb, a.rounds, a.reps, a.batch_reps)]
    med = {}
    for name, _, _, _ in kinds:
        v = np.array(rounds[name])
        med[name] = float(np.median(v))
        lines.append("%-16s %9.1f [%.1f .. %.1f]" % (name, med[name], v.min(), v.max()))
    lines.append("ratio parent / u8: single %.2f, batch (both from host memory) %.2f, batch (u8 images already on the device) %.2f" % (
        med["single parent"] / med["single u8"], med["batch parent"] / med["batch u8+upload"], med["batch parent"] / med["batch u8"]))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
