"""NumPy restatement of the keyframe blob (include/sepfinder.h: sf_kfblob_header, sf_kfblob_entry, the keyframe block) --
what sf_store_export_keyframes_device writes and what sf_store_import_keyframes_device accepts -- and a handle made of it
for the exchanges that run without a GPU.

A keyframe is (desc uint8 [rows, cols], xyz float32 [rows, 3] or None, x float32 [rows], y float32 [rows], octave int32
[rows]); float32 descriptor rows are given as their bytes.  Everything is compared bit for bit (same())."""
import ctypes as C

import numpy as np

from multi_robot_slam_separators_amd import _abi

HEADER, ENTRY = _abi.KFBLOB_HEADER_DTYPE, _abi.KFBLOB_ENTRY_DTYPE
OVERFLOW, BAD_HEADER, BAD_ENTRY = _abi.WIRE_EXPORT_OVERFLOW, _abi.WIRE_BAD_HEADER, _abi.WIRE_BAD_ENTRY
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])


def pad16(v):
    return (int(v) + 15) & ~15


def block_bytes(rows, cols, n3d):
    return pad16(rows * cols) + (pad16(rows * 12) if n3d > 0 else 0) + pad16(rows * 12)


def stored_octave(octave):
    """The byte the store keeps of an octave, sign-extended (k_ingest)."""
    o = np.asarray(octave, np.int64) & 255
    return np.where(o < 128, o, o - 256).astype(np.int32)


def desc_dwords(cols, desc_type):
    """Dwords of a stored row: the store's width class."""
    return cols // 4 if desc_type != 0 else (8 if cols <= 32 else 16)


def cols_in_class(cols, w, desc_type):
    if desc_type == 0:
        return 1 <= cols <= _abi.SF_MAX_DESC_BYTES and desc_dwords(cols, 0) == w
    if desc_type == 1:
        return cols in (256, 512) and cols // 4 == w
    return cols == _abi.SF_DESC_BYTES_U8 and cols // 4 == w


def keyframe(desc, xyz, x, y, octave):
    desc = np.ascontiguousarray(desc)
    if desc.dtype == np.float32:
        desc = desc.view(np.uint8).reshape(desc.shape[0], 4 * desc.shape[1])
    rows = desc.shape[0]
    return (desc.astype(np.uint8, copy=False), None if xyz is None else np.ascontiguousarray(xyz, np.float32).reshape(rows, 3),
            np.ascontiguousarray(x, np.float32).reshape(rows), np.ascontiguousarray(y, np.float32).reshape(rows),
            stored_octave(octave).reshape(rows))


def empty_keyframe(cols):
    return keyframe(np.zeros((0, cols), np.uint8), None, [], [], [])


def same(a, b):
    """Two keyframes (or lists of them) hold the same bits; an absent xyz equals only an absent one, except at 0 rows."""
    if isinstance(a, list) or isinstance(b, list):
        return len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    if a[0].shape != b[0].shape or a[0].tobytes() != b[0].tobytes():
        return False
    if a[0].shape[0] and (a[1] is None) != (b[1] is None):
        return False
    if a[0].shape[0] and a[1] is not None and a[1].tobytes() != b[1].tobytes():
        return False
    return all(a[i].tobytes() == b[i].tobytes() for i in (2, 3, 4))


def plan(keyframes):
    """(total bytes, max rows) of the canonical blob."""
    return 32 + 32 * len(keyframes) + sum(block_bytes(k[0].shape[0], k[0].shape[1], 0 if k[1] is None else k[0].shape[0])
                                           for k in keyframes), max([k[0].shape[0] for k in keyframes] + [0])


def pack(keyframes, desc_type=0):
    """The canonical blob: blocks in order and tight behind the table, padding and reserved bytes zero."""
    keyframes = [keyframe(*k) for k in keyframes]
    n = len(keyframes)
    total, max_rows = plan(keyframes)
    out = np.zeros(total, np.uint8)
    hdr = out[:32].view(HEADER)
    hdr["magic"], hdr["version"], hdr["desc_type"] = _abi.SF_KFBLOB_MAGIC, _abi.SF_KFBLOB_VERSION, desc_type
    hdr["n_keyframes"], hdr["max_rows"], hdr["total_bytes"] = n, max_rows, total
    table = out[32: 32 + 32 * n].view(ENTRY)
    off = 32 + 32 * n
    for i, (desc, xyz, x, y, octave) in enumerate(keyframes):
        rows, cols = desc.shape
        n3d = rows if xyz is not None else 0
        e = table[i]
        e["rows"], e["n3d"], e["cols"], e["offset"], e["bytes"] = rows, n3d, cols, off, block_bytes(rows, cols, n3d)
        at = off
        out[at: at + rows * cols] = desc.reshape(-1)
        at += pad16(rows * cols)
        if n3d:
            out[at: at + rows * 12] = xyz.view(np.uint8).reshape(-1)
            at += pad16(rows * 12)
        kp = np.zeros(rows, KP)
        kp["x"], kp["y"], kp["octave"] = x, y, octave
        out[at: at + rows * 12] = kp.view(np.uint8).reshape(-1)
        off += block_bytes(rows, cols, n3d)
    assert off == total
    return out.tobytes()


def unpack(blob, n, max_rows, cols, desc_type, nbytes=None):
    """The import's rules on blob[:nbytes] (default: all of it) -> (n keyframes, [bits, emptied, first emptied or -1, 0]).
    A bad header empties every keyframe, a bad entry its own; an emptied keyframe has 0 rows of `cols` bytes."""
    raw = np.frombuffer(bytes(blob), np.uint8)
    nbytes = raw.size if nbytes is None else int(nbytes)
    assert nbytes <= raw.size
    w = desc_dwords(cols, desc_type)
    tend = 32 + 32 * n
    ok = nbytes >= tend
    if ok:
        h = raw[:32].view(HEADER)[0]
        total = int(h["total_bytes"])
        ok = (int(h["magic"]) == _abi.SF_KFBLOB_MAGIC and int(h["version"]) == _abi.SF_KFBLOB_VERSION
              and int(h["desc_type"]) == desc_type and int(h["n_keyframes"]) == n and tend <= total <= nbytes)
    if not ok:
        return [empty_keyframe(cols) for _ in range(n)], [BAD_HEADER, n, 0 if n else -1, 0] if n else [0, 0, -1, 0]
    table = raw[32:tend].view(ENTRY)
    out, emptied = [], []
    for i in range(n):
        e = table[i]
        rows, n3d, c, off, size = int(e["rows"]), int(e["n3d"]), int(e["cols"]), int(e["offset"]), int(e["bytes"])
        good = (0 <= rows <= max_rows and n3d in (0, rows) and cols_in_class(c, w, desc_type) and off % 16 == 0 and off >= tend
                and off + size <= total and size == block_bytes(rows, c, n3d))
        if not good:
            out.append(empty_keyframe(cols))
            emptied.append(i)
            continue
        at = off
        desc = raw[at: at + rows * c].reshape(rows, c).copy()
        at += pad16(rows * c)
        xyz = None
        if n3d:
            xyz = raw[at: at + rows * 12].view(np.float32).reshape(rows, 3).copy()
            at += pad16(rows * 12)
        kp = raw[at: at + rows * 12].view(KP)
        out.append(keyframe(desc, xyz, kp["x"].copy(), kp["y"].copy(), kp["octave"].copy()))
    return out, [BAD_ENTRY if emptied else 0, len(emptied), emptied[0] if emptied else -1, 0]


def of_features(fa):
    """The keyframe a store slot keeps of an _abi.FeatureArrays."""
    return keyframe(fa.desc, fa.xyz if fa.xyz.shape[0] else None, fa.kpts["x"], fa.kpts["y"], fa.kpts["octave"])


class RefHandle:
    """The store calls KeyframeExchange uses, on a Python list and host pointers: the restatement as a backend."""

    class _Params:
        def __init__(self, desc_type, desc_bytes):
            self.desc_type, self.desc_bytes = desc_type, desc_bytes

    def __init__(self, desc_type=0, desc_bytes=32):
        self.params = RefHandle._Params(desc_type, desc_bytes)
        self.device = 0
        self.slots = []
        self.status = [0, 0, -1, 0]

    def add(self, kf):
        self.slots.append(keyframe(*kf))

    def store_size(self):
        return len(self.slots)

    def store_clear(self):
        self.slots = []

    def export_plan(self, first, n):
        return plan(self.slots[first: first + n])

    def export_keyframes_device(self, first, n, ptr, cap):
        blob = pack(self.slots[first: first + n], self.params.desc_type)
        self.status = [0, 0, -1, 0]
        if len(blob) > cap:
            self.status[0] = OVERFLOW
            return
        C.memmove(ptr, blob, len(blob))

    def import_keyframes_device(self, ptr, nbytes, n, max_rows, cols):
        got, self.status = unpack(C.string_at(ptr, nbytes), n, max_rows, cols, self.params.desc_type)
        first = len(self.slots)
        self.slots += got
        return first

    def wire_status(self, check=True):
        if check and self.status[0]:
            raise RuntimeError("store wire status %s" % self.status)
        return list(self.status)
