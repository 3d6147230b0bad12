"""Store slots as one block of bytes on the device (sf_store_export_plan, sf_store_export_keyframes_device,
sf_store_import_keyframes_device, sf_store_wire_status; csrc/k_store_wire.hip) against the NumPy restatement
tests/store_wire_ref.py: what export writes equals pack() byte for byte, an imported store exports the same bytes and
verifies to the same results, malformed blobs are refused by result, and KeyframeExchange replicates a store."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from multi_robot_slam_separators_amd import _abi, dist, lib, synth
from tests import store_wire_cases as cases
from tests import store_wire_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CLEAN = [0, 0, -1, 0]


def _params(desc_type=0, desc_bytes=32, max_features=64):
    p = synth.camera_params()
    p.iterations = 100
    p.desc_type, p.desc_bytes, p.max_features = desc_type, desc_bytes, max_features      # (64 features: kcap 64)
    return p


def _finder(p):
    f = lib.SeparatorFinder(p)
    f.set_stream(torch.cuda.current_stream().cuda_stream)
    return f


def _export(f, first, n, guard=64):
    """(bytes of the blob, the plan): through a tensor with `guard` bytes of 0xC3 on either side, which must survive."""
    total, max_rows = f.export_plan(first, n)
    t = torch.full((total + 2 * guard,), 0xC3, dtype=torch.uint8, device=DEV)
    f.export_keyframes_device(first, n, t.data_ptr() + guard, total)
    assert f.wire_status() == CLEAN
    raw = t.cpu().numpy()
    assert (raw[:guard] == 0xC3).all() and (raw[guard + total:] == 0xC3).all()
    return raw[guard: guard + total].tobytes(), (total, max_rows)


def _import(f, blob, n, max_rows, cols, factor=1, nbytes=None, check=True):
    """The blob in a zero-filled tensor `factor` times its length; returns (first slot, status)."""
    raw = np.frombuffer(blob, np.uint8)
    t = torch.zeros(max(factor * raw.size, 32), dtype=torch.uint8, device=DEV)
    t[: raw.size] = torch.from_numpy(raw.copy()).to(DEV)
    first = f.import_keyframes_device(t.data_ptr(), raw.size if nbytes is None else nbytes, n, max_rows, cols)
    return first, f.wire_status(check=check)


@pytest.mark.parametrize("desc_type,desc_bytes,widths", cases.HANDLES)
def test_export_equals_the_restatement_and_round_trips(desc_type, desc_bytes, widths):
    feats = cases.mixed_features(7 + desc_bytes, widths)
    kfs = [ref.of_features(x) for x in feats]
    with _finder(_params(desc_type, desc_bytes)) as a, _finder(_params(desc_type, desc_bytes)) as b:
        for x in feats:
            a.store_add_keyframe(x)
        n = len(feats)
        for first, cnt in ((0, n), (2, 3), (n - 1, 1), (5, 0), (0, 0)):                  # whole, sub-ranges, one, none
            want = ref.pack(kfs[first: first + cnt], desc_type)
            got, plan = _export(a, first, cnt)
            assert plan == ref.plan(kfs[first: first + cnt]) and plan[0] == len(want)
            assert got == want, (first, cnt)
        blob, (total, max_rows) = _export(a, 0, n)
        assert max_rows == 257
        # into a store that holds one small keyframe at the default capacity of 64 rows: the import makes it grow
        small = cases.rand_features(np.random.default_rng(3), 10, widths[0], True)
        b.store_add_keyframe(small)
        before, _ = _export(b, 0, 1)
        first, status = _import(b, blob, n, max_rows, max(widths))
        assert (first, status, b.store_size()) == (1, CLEAN, 1 + n)
        assert _export(b, 1, n)[0] == blob
        assert _export(b, 0, 1)[0] == before == ref.pack([ref.of_features(small)], desc_type)
        # the host conveniences: bytes out, bytes in
        assert a.export_keyframes(2, 3) == ref.pack(kfs[2:5], desc_type)
        assert b.import_keyframes(a.export_keyframes(2, 3)) == (1 + n, 3) and b.store_size() == n + 4
        assert _export(b, 1 + n, 3)[0] == ref.pack(kfs[2:5], desc_type)
        for bad in ((-1, 1), (0, n + 1), (n, 1)):
            with pytest.raises(lib.SepfinderError) as e:
                a.export_plan(*bad)
            assert e.value.code == _abi.SF_ERANGE


def test_three_hundred_keyframes_take_more_than_one_pass_of_the_scan():
    rng = np.random.default_rng(21)
    feats = [cases.rand_features(rng, int(rng.integers(0, 21)), 32, bool(i % 3)) for i in range(300)]
    kfs = [ref.of_features(x) for x in feats]
    with _finder(_params()) as a, _finder(_params()) as b:
        for x in feats:
            a.store_add_keyframe(x)
        blob, (total, max_rows) = _export(a, 0, 300)
        assert blob == ref.pack(kfs) and (total, max_rows) == ref.plan(kfs)
        assert _export(a, 250, 50)[0] == ref.pack(kfs[250:])
        first, status = _import(b, blob, 300, max_rows, 32)
        assert (first, status, b.store_size()) == (0, CLEAN, 300)
        assert _export(b, 0, 300)[0] == blob


@pytest.mark.parametrize("kind", ["binary", "float32", "uint8"])
def test_verification_is_indifferent_to_the_route(kind):
    A, B, is_true, _ = synth.make_pairs(90, 6, k=200, cols=32, true_frac=0.5)
    rng = np.random.default_rng(91)
    if kind == "float32":
        p, cols = _params(1, 256, 256), 256
        A, B = [synth.float_descriptors(x, 64, rng, 0.05) for x in A], [synth.float_descriptors(x, 64, rng, 0.05) for x in B]
    elif kind == "uint8":
        p, cols = _params(2, 128, 256), 128
        A, B = [synth.u8_descriptors(x, 128, rng, 8) for x in A], [synth.u8_descriptors(x, 128, rng, 8) for x in B]
    else:
        p, cols = _params(0, 32, 256), 32
    with _finder(p) as a, _finder(p) as b:
        for x in A + B:
            a.store_add_keyframe(x)
        blob, (_, max_rows) = _export(a, 0, 12)
        assert _import(b, blob, 12, max_rows, cols) == (0, CLEAN)
        res_a = a.verify_pairs(range(6), range(6, 12))
        res_b = b.verify_pairs(range(6), range(6, 12))
        assert res_a.tobytes() == res_b.tobytes()
        assert 1 <= int(res_a["success"].sum()) == int(is_true.sum())


def _rgb(gray, seed):
    """An rgb8 image [h, w, 3] with the structure of a gray one: the channels shifted apart, plus noise of their own."""
    rng = np.random.default_rng(seed)
    g = np.asarray(gray, np.int32)
    rgb = np.stack([g + 40, g, g - 50], axis=-1) + rng.integers(-20, 21, size=g.shape + (3,))
    return np.ascontiguousarray(np.clip(rgb, 0, 255).astype(np.uint8))


def test_front_end_to_wire():
    """Keyframes written by sf_add_keyframes_u8_batch_device (Vis/FeatureType 6) leave through the blob and come back."""
    from oracle import netvlad_torch
    from tests import extract_cases as ec
    w, h, maxf = 160, 120, 200
    cam, det = _abi.stereo_camera(460.0, 458.0, w / 2.0, h / 2.0, 0.11), _abi.detector_params(maxf)
    grays = [ec.make_stereo_pair(60 + i, width=w, height=h, max_disp=20.0)[:2] for i in range(2)]
    d_l = torch.from_numpy(np.stack([_rgb(l, 5 + i) for i, (l, r) in enumerate(grays)])).to(DEV)
    d_r = torch.from_numpy(np.stack([_rgb(r, 8 + i) for i, (l, r) in enumerate(grays)])).to(DEV)
    p = _params(0, 32, maxf)
    p.fx, p.fy, p.cx, p.cy = 460.0, 458.0, w / 2.0, h / 2.0
    p.image_width, p.image_height, p.netvlad_dimensions = w, h, 128
    with _finder(p) as f, _finder(_params(0, 32, maxf)) as b:
        f.netvlad_load(netvlad_torch.random_weights(3, clusters=64, pca_dim=512))
        first, _ = f.add_keyframes_u8_batch_device(d_l.data_ptr(), d_r.data_ptr(), None, _abi.SF_IMAGE_RGB8, 2, w, h, 3 * w,
                                                   3 * w * h, cam, det)
        blob, (total, max_rows) = _export(f, first, 2)
        hdr = np.frombuffer(blob[:32], ref.HEADER)[0]
        table = np.frombuffer(blob[32:96], ref.ENTRY)
        assert int(hdr["n_keyframes"]) == 2 and 10 < int(table["rows"].min()) <= max_rows <= maxf
        assert (table["cols"] == 32).all() and (table["n3d"] == table["rows"]).all()
        assert _import(b, blob, 2, max_rows, 32) == (0, CLEAN)
        assert _export(b, 0, 2)[0] == blob
        kfs, status = ref.unpack(blob, 2, max_rows, 32, 0)
        assert status == CLEAN and ref.pack(kfs) == blob


def test_malformed_blobs_are_refused_by_result():
    """Every bad blob sits in a tensor four times its stated bytes and plants nothing beyond twice of them: a missing check
    would read allocated memory and show in the slots.  Expected: the restatement's status words and emptied slots, every
    other slot intact, sf_store_size advanced by n."""
    feats, good = cases.malformed_base()
    kfs = [ref.of_features(x) for x in feats]
    with _finder(_params()) as b:
        assert _import(b, good, cases.MAL_N, cases.MAL_MAX_ROWS, cases.MAL_COLS, factor=4) == (0, CLEAN)
        assert _export(b, 0, cases.MAL_N)[0] == good
        for name, blob, (n, max_rows, cols, desc_type), bits, emptied in cases.malformed_cases():
            want_kfs, want_status = ref.unpack(blob + bytes(3 * len(blob)), n, max_rows, cols, desc_type, nbytes=len(blob))
            assert want_status == [bits, len(emptied), emptied[0], 0], name
            size = b.store_size()
            first, status = _import(b, blob, n, max_rows, cols, factor=4, check=False)
            print("%s: status %s, restatement %s" % (name, status, want_status))
            assert first == size and b.store_size() == size + n, name
            assert status == want_status, name
            with pytest.raises(lib.SepfinderError) as e:
                b.wire_status()
            assert e.value.code == _abi.SF_ERANGE
            assert _export(b, first, n)[0] == ref.pack(want_kfs), name
            for i in range(n):
                assert ref.same(want_kfs[i], ref.empty_keyframe(cols) if i in emptied else kfs[i]), (name, i)
        assert _export(b, 0, cases.MAL_N)[0] == good                       # the slots of before are as they were
        # a blob shorter than its own table; and the status is that of the LAST call
        first, status = _import(b, good, cases.MAL_N, cases.MAL_MAX_ROWS, cases.MAL_COLS, factor=4, nbytes=96, check=False)
        assert status == [ref.BAD_HEADER, cases.MAL_N, 0, 0]
        assert _import(b, good, cases.MAL_N, cases.MAL_MAX_ROWS, cases.MAL_COLS)[1] == CLEAN
        # what the host refuses, before anything is touched
        size = b.store_size()
        t = torch.zeros(len(good) + 16, dtype=torch.uint8, device=DEV)
        for args, code in (((t.data_ptr() + 4, len(good), 4, 64, 32), _abi.SF_EINVAL), ((0, len(good), 4, 64, 32), _abi.SF_EINVAL),
                           ((t.data_ptr(), len(good), 65536, 64, 32), _abi.SF_ERANGE),
                           ((t.data_ptr(), len(good), 4, 64, 65), _abi.SF_ERANGE),       # no such binary row
                           ((t.data_ptr(), len(good), 4, 64, 64), _abi.SF_EINVAL)):     # the store holds the other width class
            with pytest.raises(lib.SepfinderError) as e:
                b.import_keyframes_device(*args)
            assert e.value.code == code and b.store_size() == size, args[2:]


def test_export_overflow_is_reported_and_writes_nothing_behind_the_capacity():
    feats = cases.mixed_features(5, (32,))
    with _finder(_params()) as a:
        for x in feats:
            a.store_add_keyframe(x)
        total, _ = a.export_plan(0, len(feats))
        for cap in (total - 16, 16):
            t = torch.full((total + 64,), 0xC3, dtype=torch.uint8, device=DEV)
            a.export_keyframes_device(0, len(feats), t.data_ptr(), cap)
            status = a.wire_status(check=False)
            raw = t.cpu().numpy()
            assert status == [ref.OVERFLOW, 0, -1, 0]
            assert (raw[cap:] == 0xC3).all() and (raw[min(cap, 32): cap] == 0xC3).all()
            if cap >= 32:
                hdr = raw[:32].view(ref.HEADER)[0]
                assert int(hdr["magic"]) == 0 and int(hdr["total_bytes"]) == total      # ... and says what it would take
            with pytest.raises(lib.SepfinderError) as e:
                a.wire_status()
            assert e.value.code == _abi.SF_ERANGE
        assert _export(a, 0, len(feats))[0] == ref.pack([ref.of_features(x) for x in feats])      # (the status is reset)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _filled(p, feats):
    f = _finder(p)
    for x in feats:
        f.store_add_keyframe(x)
    return f


def test_keyframe_exchange_over_self_collective():
    """World size 1 without a process group: main equals a store filled directly, front is cleared, twice in a row.  The
    keyframes are 33 .. 64 bytes wide on handles whose desc_bytes is 32: the width the receivers size their stores with is
    read off the blob's table, not off that parameter."""
    assert isinstance(dist.collective(), dist.SelfCollective)
    rounds = [cases.mixed_features(40, (64, 33)), cases.mixed_features(41, (33, 48))[:5]]
    p = _params()
    assert p.desc_bytes == 32
    with _finder(p) as front, _finder(p) as main, _filled(p, rounds[0] + rounds[1]) as direct:
        ex = dist.KeyframeExchange(front, main)
        at = 0
        for feats, check, waits in zip(rounds, (True, False), (2, 3)):
            for x in feats:
                front.store_add_keyframe(x)
            assert ex.exchange(check=check) == [(at, len(feats))]
            assert main.wire_status() == CLEAN and front.store_size() == 0 and ex.waits == waits
            at += len(feats)
        assert main.store_size() == at == direct.store_size()
        assert _export(main, 0, at)[0] == _export(direct, 0, at)[0]
        # the size question leaves the status of the last export or import alone
        t = torch.zeros(64, dtype=torch.uint8, device=DEV)
        main.export_keyframes_device(0, at, t.data_ptr(), 64)
        main.export_plan(0, at)
        assert main.wire_status(check=False) == [ref.OVERFLOW, 0, -1, 0]


_RCCL_WORKER = r"""
import os, sys
import torch, torch.distributed as td
sys.path.insert(0, %(root)r)
from multi_robot_slam_separators_amd import dist
from tests import store_wire_cases as cases, store_wire_ref as ref
from tests.test_gpu_store_wire import _export, _filled, _finder, _params
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[1]
torch.cuda.set_device(0)
td.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
assert dist.collective() is td
feats = cases.mixed_features(50, (32, 7))
p = _params()
with _finder(p) as front, _finder(p) as main, _filled(p, feats) as direct:
    for x in feats:
        front.store_add_keyframe(x)
    ex = dist.KeyframeExchange(front, main)
    assert ex.world == 1 and ex.exchange(check=True) == [(0, len(feats))]
    assert front.store_size() == 0 and main.store_size() == len(feats)
    assert _export(main, 0, len(feats))[0] == _export(direct, 0, len(feats))[0] == ref.pack([ref.of_features(x) for x in feats])
torch.cuda.synchronize()
td.destroy_process_group()
print("rccl world 1 ok")
"""


def test_keyframe_exchange_over_rccl_world_1(tmp_path):
    """The same through ncclAllGather: a world-1 RCCL process group, in a process of its own (this one has none)."""
    script = tmp_path / "worker.py"
    script.write_text(_RCCL_WORKER % {"root": ROOT})
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(script), str(_free_port())], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "rccl world 1 ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
