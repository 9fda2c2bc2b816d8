"""The LAS layout (ASPRS LAS 1.0 - 1.4) and this project's reading and writing rules, restated with numpy and struct from the format's
tables; nothing of the package is imported.  laspy is not installed, so parity with it is unpinned: this file is the
yardstick of csrc/tl_las.hip and treelearn_amd/util/las.py.

Reading: x = X * scale + offset, a multiply and then an add in float64 (what numpy computes for the reference's load_data); with a
`treeID` extra dimension (any of the ten scalar types, widened to float64) a label column: 1, then treeID where treeID != 0, then 0 where
the classification is 1 or 2, then -1 where the point is neither.
Writing: LAS 1.2, point format 3, one extra dimension treeID u32: X = rint((x - offset) / scale); intensity 0, return byte 0x09,
classification 2 for label 0 and 4 otherwise, scan angle / user data / source 0, GPS time 0.0, treeID = label mod 2^32, and the colour
of `label_rgb`."""
import struct

import numpy as np

BASE_LENGTH = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}
EXTRA_TYPES = {1: "u1", 2: "i1", 3: "<u2", 4: "<i2", 5: "<u4", 6: "<i4", 7: "<u8", 8: "<i8", 9: "<f4", 10: "<f8"}
HEADER = "<4sHH16sBB32s32sHHHIIBHI5I3d3d6d"               # 227 bytes: LAS 1.0 - 1.2
VLR = "<H16sHH32s"                                        # 54 bytes
DESCRIPTOR = "<2sBB32s4s24s24s24s24s24s32s"               # 192 bytes
assert struct.calcsize(HEADER) == 227 and struct.calcsize(VLR) == 54 and struct.calcsize(DESCRIPTOR) == 192
assert struct.calcsize(HEADER + "Q") == 235 and struct.calcsize(HEADER + "QQIQ15Q") == 375
SYSTEM_IDENTIFIER = b"treelearn_amd"
GENERATING_SOFTWARE = b"treelearn_amd.util.las"


def _cstr(b):
    return b.split(b"\0", 1)[0].decode("latin-1")


def parse(buf, name=""):
    """The header of a LAS file held in `buf` (bytes) as a dict; ValueError for the malformed files of the issue; compressed files are
    only recognised (point-format bit 7, a 'laszip encoded' VLR, a .laz name)."""
    if buf[:4] != b"LASF":
        raise ValueError("no LASF signature")
    if len(buf) < 227:
        raise ValueError("shorter than its header")
    f = struct.unpack_from(HEADER, buf, 0)
    h = dict(version=(f[4], f[5]), header_size=f[10], offset_to_points=f[11], n_vlr=f[12], record_length=f[14], count=f[15],
             scale=f[21:24], offset=f[24:27], maxs=(f[27], f[29], f[31]), mins=(f[28], f[30], f[32]))
    if h["header_size"] < 227 or len(buf) < h["header_size"]:
        raise ValueError("shorter than its header")
    if h["version"] >= (1, 4) and h["header_size"] >= 375 and h["count"] == 0:
        h["count"] = struct.unpack_from("<Q", buf, 247)[0]
    h["compressed"] = bool(f[13] & 0x80) or name.lower().endswith(".laz")
    h["point_format"] = f[13] & 0x3f
    if h["offset_to_points"] < h["header_size"]:
        raise ValueError("offset to the point data inside the header")
    extras, at = [], h["header_size"]
    for _ in range(h["n_vlr"]):
        if at + 54 > h["offset_to_points"]:
            raise ValueError("variable length record past the offset to the point data")
        _, user, rid, length, _ = struct.unpack_from(VLR, buf, at)
        if _cstr(user) == "laszip encoded":
            h["compressed"] = True
        if _cstr(user) == "LASF_Spec" and rid == 4:
            for k in range(length // 192):
                d = struct.unpack_from(DESCRIPTOR, buf, at + 54 + 192 * k)
                extras.append((_cstr(d[3]), d[1], d[2]))
        at += 54 + length
    if at > h["offset_to_points"]:
        raise ValueError("variable length records past the offset to the point data")
    if h["point_format"] not in BASE_LENGTH:
        raise ValueError("unknown point format")
    base = BASE_LENGTH[h["point_format"]]
    if not h["compressed"]:
        if h["record_length"] < base:
            raise ValueError("record length below the base length of the format")
        if len(buf) < h["offset_to_points"] + h["count"] * h["record_length"]:
            raise ValueError("shorter than its point data")
    dims, off = [], base
    for nm, t, options in extras:
        dims.append((nm, t, off))
        off += np.dtype(EXTRA_TYPES[t]).itemsize if t in EXTRA_TYPES else options
    h["extra_dims"] = dims
    return h


def field(buf, h, offset, dtype):
    """One field of every record as an array."""
    n, rl = h["count"], h["record_length"]
    raw = np.frombuffer(buf, np.uint8, n * rl, h["offset_to_points"]).reshape(n, rl)
    w = np.dtype(dtype).itemsize
    return np.ascontiguousarray(raw[:, offset:offset + w]).view(dtype).reshape(n)


def classification(buf, h):
    if h["point_format"] <= 5:
        return field(buf, h, 15, "u1") & 0x1f                   # the low five bits; the flags sit above them
    return field(buf, h, 16, "u1")


def read(buf, name=""):
    """N x 3 or N x 4 float64 of an uncompressed LAS file."""
    h = parse(buf, name)
    if h["compressed"]:
        raise ImportError("a compressed file needs laspy")
    cols = []
    for a in range(3):
        X = field(buf, h, 4 * a, "<i4")
        cols.append(X * np.float64(h["scale"][a]) + np.float64(h["offset"][a]))
    tid = [(t, off) for nm, t, off in h["extra_dims"] if nm == "treeID" and t in EXTRA_TYPES]
    if not tid:
        return np.stack(cols, 1)
    tree_id = field(buf, h, tid[0][1], EXTRA_TYPES[tid[0][0]])
    classes = classification(buf, h)
    tree, non_tree = tree_id != 0, np.isin(classes, [1, 2])
    labels = np.ones(h["count"])
    labels[tree] = tree_id[tree]
    labels[non_tree] = 0
    labels[~tree & ~non_tree] = -1
    return np.stack(cols + [labels], 1)


# ------------------------------------------------------------------------------------------------ writing
def label_rgb(labels):
    """u16 [N, 3]: black for label 0, else 257 * the three low bytes of an integer mix of the label's low 32 bits."""
    h = (np.asarray(labels, np.int64).astype(np.uint64) & np.uint64(0xffffffff)) * np.uint64(2654435761) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(15)
    h = h * np.uint64(2246822519) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    rgb = np.stack([h & np.uint64(0xff), (h >> np.uint64(8)) & np.uint64(0xff), (h >> np.uint64(16)) & np.uint64(0xff)], 1) * np.uint64(257)
    rgb[np.asarray(labels) == 0] = 0
    return rgb.astype(np.uint16)


def quantise(coords, scale, offset):
    """rint((x - offset) / scale) as float64 [N, 3] (numpy's rint rounds half to even), and which rows can be written."""
    q = np.rint((np.asarray(coords)[:, :3].astype(np.float64) - np.asarray(offset, np.float64)) / np.asarray(scale, np.float64))
    with np.errstate(invalid="ignore"):
        ok = ((q >= -2147483648.0) & (q <= 2147483647.0)).all(1)
    return q, ok


def records(coords, labels, scale=(0.001,) * 3, offset=(0.0,) * 3):
    """u8 [N, 38]; ValueError when a row cannot be written."""
    q, ok = quantise(coords, scale, offset)
    if not ok.all():
        raise ValueError("a coordinate cannot be written")
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    rec = np.zeros(n, dtype=np.dtype([("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2"), ("returns", "u1"), ("cls", "u1"),
                                      ("angle", "i1"), ("user", "u1"), ("source", "<u2"), ("gps", "<f8"), ("rgb", "<u2", 3), ("treeID", "<u4")]))
    assert rec.dtype.itemsize == 38
    rec["X"], rec["Y"], rec["Z"] = q[:, 0].astype(np.int32), q[:, 1].astype(np.int32), q[:, 2].astype(np.int32)
    rec["returns"] = 0x09
    rec["cls"] = np.where(labels == 0, 2, 4)
    rec["rgb"] = label_rgb(labels)
    rec["treeID"] = (labels.astype(np.uint64) & np.uint64(0xffffffff)).astype(np.uint32)
    return rec.view(np.uint8).reshape(n, 38)


def extremes(rec):
    """i32 [6]: min X Y Z, max X Y Z of u8 [n, 38] records (the sentinels for none)."""
    if len(rec) == 0:
        return np.array([2 ** 31 - 1] * 3 + [-2 ** 31] * 3, np.int32)
    xyz = np.ascontiguousarray(rec[:, :12]).view("<i4").reshape(-1, 3)
    return np.concatenate([xyz.min(0), xyz.max(0)]).astype(np.int32)


def header(count, offset, ext, created, scale=(0.001,) * 3):
    """The 473 bytes before the records: header (227), VLR header (54), the treeID descriptor (192)."""
    scale, offset = np.asarray(scale, np.float64), np.asarray(offset, np.float64)
    if count:
        e = np.asarray(ext, np.float64)
        lo, hi = e[:3] * scale + offset, e[3:] * scale + offset                    # the de-quantised extreme integers
    else:
        lo = hi = np.zeros(3)
    head = struct.pack(HEADER, b"LASF", 0, 0, b"", 1, 2, SYSTEM_IDENTIFIER, GENERATING_SOFTWARE, created[0], created[1], 227, 473, 1, 3, 38,
                       count, count, 0, 0, 0, 0, *scale, *offset, hi[0], lo[0], hi[1], lo[1], hi[2], lo[2])
    vlr = struct.pack(VLR, 0, b"LASF_Spec", 4, 192, b"extra bytes")
    desc = struct.pack(DESCRIPTOR, b"", 5, 0, b"treeID", b"", b"", b"", b"", b"", b"", b"")
    return head + vlr + desc


def write(coords, labels, offset, created):
    """The whole file as bytes."""
    rec = records(coords, labels, offset=offset)
    return header(len(rec), offset, extremes(rec), created) + rec.tobytes()


def fma_read_x(X, scale, offset):
    """What a contracted multiply-add would give: X * scale + offset with ONE rounding (exact product in integers of 2^-k)."""
    from fractions import Fraction
    return np.array([float(Fraction(int(v)) * Fraction(float(scale)) + Fraction(float(offset))) for v in X])
