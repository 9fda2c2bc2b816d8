"""LAS point clouds read and written natively: the headers on the host, the point records on the device (csrc/tl_las.hip).

  read_header        the public header block, the VLRs that matter (extra bytes, laszip) and the consistency checks; pure Python
  read_las           <- load_data's .las branch (tree_learn/util/data_preparation.py:28-49): x y z [label] as float64
  write_las          <- save_data's .las branch (util/pipeline.py:339-384): LAS 1.2, point format 3, scale 1 mm, u32 treeID
  write_las_segments one encode of a cloud in a given row order, one file per contiguous range of it (save_treewise)

laspy is not a dependency, so byte parity with it is unpinned; the yardstick is the ASPRS layout as tests/las_restatement.py restates it.
Compressed files (.laz) are not decoded here: they go through laspy when it is importable and raise ImportError otherwise.
The record passes have no CPU fallback."""
import datetime
import os
import struct

import numpy as np

__all__ = ["read_header", "read_las", "write_las", "write_las_segments", "LasHeader", "PATHS"]

BASE_LENGTH = (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67)                      # point formats 0 .. 10
# extra-bytes data types 1 .. 10 -> (numpy name, width)
EXTRA_TYPES = {1: ("u1", 1), 2: ("i1", 1), 3: ("<u2", 2), 4: ("<i2", 2), 5: ("<u4", 4), 6: ("<i4", 4), 7: ("<u8", 8), 8: ("<i8", 8),
               9: ("<f4", 4), 10: ("<f8", 8)}
PATHS = {"auto": 0, "plain": 1, "staged": 2}
STAGED_MAX_RECORD = 128
RECORD_LENGTH = 38                                                               # what the writer writes: format 3 + u32 treeID
HEADER_12 = struct.Struct("<4sHH16sBB32s32sHHHIIBHI5I3d3d6d")                    # 227 bytes
VLR_HEADER = struct.Struct("<H16sHH32s")                                         # 54 bytes
EXTRA_DESCRIPTOR = struct.Struct("<2sBB32s4s24s24s24s24s24s32s")                 # 192 bytes
SYSTEM_IDENTIFIER = b"treelearn_amd"
GENERATING_SOFTWARE = b"treelearn_amd.util.las"
SCALE = 0.001
_NO_GPU = "the LAS record passes run on the GPU (csrc/tl_las.hip) and there is no CPU fallback: no HIP device is available"


class LasHeader:
    """What read_header returns: version (major, minor), point_format, record_length, count, scale / offset (3 floats each), mins / maxs
    (3 floats each), extra_dims [(name, type code, byte offset in the record)], compressed, header_size, offset_to_points."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "LasHeader(" + ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items()) + ")"

    def extra(self, name):
        """(type code, byte offset) of the extra dimension `name` when it is one of the ten scalar types, else None."""
        for n, t, off in self.extra_dims:
            if n == name and t in EXTRA_TYPES:
                return t, off
        return None


def _cstr(b):
    return b.split(b"\0", 1)[0].decode("latin-1")


def read_header(path):
    """Parse and check the header of a LAS file; touches no GPU.  ValueError names the cause: no LASF signature, a file shorter than its
    header, an unknown point format, a record length below the format's base length, a file shorter than its point data."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(375)
        if head[:4] != b"LASF":
            raise ValueError(f"{path}: not a LAS file (no 'LASF' signature)")
        if len(head) < 227:
            raise ValueError(f"{path}: file of {size} bytes is shorter than a LAS header (227 bytes)")
        major, minor = head[24], head[25]
        header_size, offset_to_points, n_vlr = struct.unpack_from("<HII", head, 94)
        if header_size < 227 or size < header_size:
            raise ValueError(f"{path}: file of {size} bytes is shorter than its header ({header_size} bytes)")
        fmt_byte, record_length, count = struct.unpack_from("<BHI", head, 104)
        scale = struct.unpack_from("<3d", head, 131)
        offset = struct.unpack_from("<3d", head, 155)
        box = struct.unpack_from("<6d", head, 179)
        if (major, minor) >= (1, 4) and header_size >= 375 and len(head) >= 375 and count == 0:
            count = struct.unpack_from("<Q", head, 247)[0]
        compressed = bool(fmt_byte & 0x80) or path.lower().endswith(".laz")
        point_format = fmt_byte & 0x3f
        if offset_to_points < header_size:
            raise ValueError(f"{path}: the offset to the point data ({offset_to_points}) lies inside the {header_size}-byte header")
        extra_dims = []
        at = header_size
        for k in range(n_vlr):
            if at + 54 > offset_to_points:
                raise ValueError(f"{path}: variable length record {k + 1} of {n_vlr} runs past the offset to the point data ({offset_to_points})")
            f.seek(at)
            vh = f.read(54)
            if len(vh) < 54:
                raise ValueError(f"{path}: a variable length record runs past the end of the file")
            _, user, record_id, length, _ = VLR_HEADER.unpack(vh)
            user = _cstr(user)
            if user == "laszip encoded":
                compressed = True
            if user == "LASF_Spec" and record_id == 4:
                body = f.read(length)
                if len(body) < length:
                    raise ValueError(f"{path}: the extra-bytes record runs past the end of the file")
                for d in range(length // 192):
                    _, dtype, options, name = EXTRA_DESCRIPTOR.unpack_from(body, d * 192)[:4]
                    extra_dims.append((_cstr(name), dtype, options))
            at += 54 + length
        if at > offset_to_points:
            raise ValueError(f"{path}: the variable length records end at byte {at}, past the offset to the point data ({offset_to_points})")
    if point_format > 10:
        raise ValueError(f"{path}: unknown point format {point_format}")
    base = BASE_LENGTH[point_format]
    if not compressed:
        if record_length < base:
            raise ValueError(f"{path}: record length {record_length} is below the {base} bytes of point format {point_format}")
        if size < offset_to_points + count * record_length:
            raise ValueError(f"{path}: file of {size} bytes is shorter than its point data ({count} records of {record_length} bytes "
                             f"from byte {offset_to_points})")
    dims, off = [], base
    for name, dtype, options in extra_dims:
        if dtype in EXTRA_TYPES:
            width = EXTRA_TYPES[dtype][1]
        elif dtype == 0:
            width = options                                                       # an undocumented block: its width sits in `options`
        elif 11 <= dtype <= 30:
            width = EXTRA_TYPES[(dtype - 1) % 10 + 1][1] * ((dtype - 1) // 10 + 1)    # the deprecated 2- and 3-element types
        else:
            raise ValueError(f"{path}: extra dimension {name!r} has the unknown data type {dtype}")
        if not compressed and off + width > record_length:
            raise ValueError(f"{path}: extra dimension {name!r} lies outside the {record_length}-byte record")
        dims.append((name, dtype, off))
        off += width
    return LasHeader(version=(major, minor), point_format=point_format, record_length=record_length, count=count, scale=tuple(scale),
                     offset=tuple(offset), maxs=(box[0], box[2], box[4]), mins=(box[1], box[3], box[5]), extra_dims=dims,
                     compressed=compressed, header_size=header_size, offset_to_points=offset_to_points)


def _read_compressed(path):
    """A compressed file exactly as the reference reads it, through laspy."""
    try:
        import laspy
    except ImportError as e:
        raise ImportError(f"{path}: a compressed LAS file needs the 'laspy' module, which is not installed") from e
    las = laspy.read(path)
    sc, of = las.header.scales, las.header.offsets
    pts = np.vstack([las.X * sc[0] + of[0], las.Y * sc[1] + of[1], las.Z * sc[2] + of[2]]).T
    if not (hasattr(las, "treeID") and hasattr(las, "classification")):
        return pts
    tree_id, classes = np.array(las.treeID), np.array(las.classification)
    labels = np.ones(len(pts))
    tree, non_tree = tree_id != 0, np.isin(classes, [1, 2])
    labels[tree] = tree_id[tree]
    labels[non_tree] = 0
    labels[~tree & ~non_tree] = -1
    return np.hstack([pts, labels[:, None]])


def _vec3(v):
    from .. import _hip
    return (_hip._c.c_double * 3)(*[float(x) for x in v])


def decode_records(records, n, header, out, first_row=0, path="auto"):
    """Decode n records of a device uint8 tensor (base aligned to 16) into rows first_row.. of the device f64 tensor `out` [N, 3 or 4]."""
    from .. import _hip
    tid = header.extra("treeID") if out.shape[1] == 4 else None
    cls_off, cls_mask = (15, 0x1f) if header.point_format <= 5 else (16, 0xff)
    _hip.check(_hip.lib().tl_las_decode(_hip.ptr(records), n, header.record_length, cls_off, cls_mask, tid[1] if tid else 0, tid[0] if tid else 0,
                                        _vec3(header.scale), _vec3(header.offset), _hip.ptr(out), out.shape[1], first_row, PATHS[path],
                                        _hip.stream()), "tl_las_decode")


_STAGING_BYTES = 8 << 20
_staging = []                                                                     # [pinned buffer, event of its last copy] x 2, made once per process


def _upload(src, dev):
    """Host bytes `src` to the front of the device tensor `dev` through two pinned buffers of 8 MB that the process keeps (a pinned
    allocation per call costs more than the copy): the host fills one while the other is in flight."""
    import torch
    if not _staging:
        _staging.extend([torch.empty(_STAGING_BYTES, dtype=torch.uint8, pin_memory=True), None] for _ in range(2))
    for i, a in enumerate(range(0, len(src), _STAGING_BYTES)):
        slot = _staging[i % 2]
        if slot[1] is not None:
            slot[1].synchronize()
        b = min(a + _STAGING_BYTES, len(src))
        slot[0].numpy()[:b - a] = src[a:b]
        dev[a:b].copy_(slot[0][:b - a], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()


def read_las(path, chunk_records=1 << 22, device_out=False, path_mode="auto"):
    """x y z [label] float64 of a LAS file: N x 4 when it has a `treeID` extra dimension (label = treeID where it is not 0, 0 where the
    classification is 1 or 2 -- applied second --, -1 for a point that is neither), else N x 3.  The file is mapped, uploaded in chunks of
    whole records and decoded on the device; the result is a numpy array, or the device tensor with device_out=True."""
    h = read_header(path)
    if h.compressed:
        data = _read_compressed(path)
        if device_out:
            import torch
            return torch.from_numpy(data).cuda()
        return data
    if path_mode not in PATHS:
        raise ValueError(f"path_mode must be one of {tuple(PATHS)}, got {path_mode!r}")
    if int(chunk_records) < 1:
        raise ValueError(f"chunk_records must be >= 1, got {chunk_records!r}")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    cols = 4 if h.extra("treeID") else 3
    n, rl = h.count, h.record_length
    out = torch.empty((n, cols), dtype=torch.float64, device="cuda")
    if n:
        mm = np.memmap(path, dtype=np.uint8, mode="r", offset=h.offset_to_points, shape=(n * rl,))
        per = min(int(chunk_records), n)
        dev = torch.empty(per * rl, dtype=torch.uint8, device="cuda")
        for r0 in range(0, n, per):
            k = min(per, n - r0)
            _upload(mm[r0 * rl:(r0 + k) * rl], dev)
            decode_records(dev, k, h, out, r0, path_mode)
        del mm
    return out if device_out else out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ writing
def _device_cloud(coords, labels):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    c = coords if torch.is_tensor(coords) else torch.from_numpy(np.asarray(coords))
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError(f"coordinates must have shape [N, 3] or [N, 4], got {tuple(c.shape)}")
    if c.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"coordinates must be float32 or float64, got {c.dtype}")
    c = c.to("cuda")
    if len(c) and (c.stride(1) != 1 or c.stride(0) not in (3, 4)):
        c = c.contiguous()
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels))
    lab = lab.reshape(-1)
    if lab.shape[0] != c.shape[0]:
        raise ValueError(f"mismatched lengths: {c.shape[0]} coordinates for {lab.shape[0]} labels")
    return c, lab.to("cuda", torch.int64).contiguous()                            # (a float label is truncated, as numpy's astype does)


def encode_records(coords, labels, order=None, starts=None, offset=(0.0, 0.0, 0.0), scale=(SCALE, SCALE, SCALE)):
    """The writer's records of a cloud on the device.  coords [N, 3 or 4] f32 / f64 and labels [N] (host or device); order: i64 [n] source
    rows in output order, or None; starts: ascending i64 [S + 1] from 0 to n, or None for one segment.  Returns (records u8 [n * 38]
    device tensor, extremes i32 [S, 6] numpy: min X Y Z, max X Y Z).  ValueError when a row cannot be written; nothing is returned then."""
    import torch
    from .. import _hip
    c, lab = _device_cloud(coords, labels)
    n_src = c.shape[0]
    o = None
    if order is not None:
        o = (order if torch.is_tensor(order) else torch.from_numpy(np.asarray(order))).reshape(-1).to("cuda", torch.int64).contiguous()
    n = n_src if o is None else o.shape[0]
    s, n_seg = None, 1
    if starts is not None:
        sh = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts, dtype=np.int64).reshape(-1)
        if len(sh) < 2 or sh[0] != 0 or sh[-1] != n or (np.diff(sh) < 0).any():
            raise ValueError(f"starts must ascend from 0 to the {n} output rows")
        s, n_seg = torch.from_numpy(sh).cuda(), len(sh) - 1
    if n == 0:                                                                    # nothing to launch: no record, every segment empty
        return torch.empty(0, dtype=torch.uint8, device="cuda"), np.tile(np.array([2 ** 31 - 1] * 3 + [-2 ** 31] * 3, np.int32), (n_seg, 1))
    rec = torch.empty(n * RECORD_LENGTH, dtype=torch.uint8, device="cuda")
    err = torch.empty(1, dtype=torch.int32, device="cuda")
    ext = torch.empty((n_seg, 6), dtype=torch.int32, device="cuda")
    _hip.check(_hip.lib().tl_las_encode(_hip.ptr(c), int(c.dtype == torch.float64), c.stride(0), n_src, _hip.ptr(lab),
                                        _hip.ptr(o), n, _vec3(scale), _vec3(offset), _hip.ptr(s), n_seg, _hip.ptr(rec), _hip.ptr(err),
                                        _hip.ptr(ext), _hip.stream()), "tl_las_encode")
    if int(err.item()):
        raise ValueError("a coordinate is not finite, or (x - offset) / scale does not fit the 32-bit integers of a LAS record "
                         "(or an order entry is not a row): nothing was written")
    return rec[:n * RECORD_LENGTH], ext.cpu().numpy()


def _created(created):
    if created is None:
        today = datetime.date.today()
        return today.timetuple().tm_yday, today.year
    day, year = created
    return int(day), int(year)


def header_bytes(count, offset, extremes, created=None, scale=(SCALE, SCALE, SCALE)):
    """The 473 bytes before the records: the LAS 1.2 header, and the extra-bytes VLR that declares `treeID` as u32.  extremes: the six
    integers min X Y Z, max X Y Z of the records (ignored when count is 0); the box is their de-quantised value X * scale + offset."""
    count = int(count)
    if count >= 1 << 32:
        raise ValueError(f"{count} points do not fit the 32-bit point count of LAS 1.2")
    scale, offset = np.asarray(scale, np.float64), np.asarray(offset, np.float64)
    if count:
        e = np.asarray(extremes, np.int32).astype(np.float64)
        lo, hi = e[:3] * scale + offset, e[3:] * scale + offset
    else:
        lo = hi = np.zeros(3)
    day, year = _created(created)
    head = HEADER_12.pack(b"LASF", 0, 0, b"", 1, 2, SYSTEM_IDENTIFIER, GENERATING_SOFTWARE, day, year, 227, 227 + 54 + 192, 1, 3,
                          RECORD_LENGTH, count, count, 0, 0, 0, 0, *scale.tolist(), *offset.tolist(),
                          hi[0], lo[0], hi[1], lo[1], hi[2], lo[2])
    vlr = VLR_HEADER.pack(0, b"LASF_Spec", 4, 192, b"extra bytes")
    desc = EXTRA_DESCRIPTOR.pack(b"", 5, 0, b"treeID", b"", b"", b"", b"", b"", b"", b"")
    return head + vlr + desc


def _mean_offset(coords, use_offset):
    import torch
    if not use_offset or len(coords) == 0:
        return np.zeros(3)
    if torch.is_tensor(coords):
        return coords[:, :3].to(torch.float64).mean(0).cpu().numpy()
    return np.asarray(coords)[:, :3].astype(np.float64, copy=False).mean(0)


def write_las(path, coords, labels, use_offset=True, created=None):
    """Write a cloud as the reference's LAS file: version 1.2, point format 3, scale 1 mm, offsets = the f64 mean of the coordinates (0 with
    use_offset=False), treeID = the label's low 32 bits, classification 2 for label 0 and 4 otherwise, a fixed colour per label.
    created = (day of year, year) of the header, today by default.  ValueError, and no file, when a coordinate cannot be written."""
    offset = _mean_offset(coords, use_offset)
    rec, ext = encode_records(coords, labels, offset=offset)
    head = header_bytes(rec.shape[0] // RECORD_LENGTH, offset, ext[0], created)
    body = rec.cpu().numpy()
    with open(path, "wb") as f:
        f.write(head)
        f.write(memoryview(body))
    return path


def write_las_segments(paths, coords, labels, order, starts, offset=None, created=None):
    """One encode of the cloud in `order`; file s = its own header (count and box of its rows) + the records of output rows
    starts[s] .. starts[s + 1] - 1, a contiguous byte range of that one encode.  paths: S names, None to skip a segment.  All files share
    `offset` (3 values, default 0) and the 1 mm scale.  Returns the written paths."""
    starts = np.asarray(starts, np.int64).reshape(-1)
    if len(paths) != len(starts) - 1:
        raise ValueError(f"{len(paths)} paths for {len(starts) - 1} segments")
    offset = np.zeros(3) if offset is None else np.asarray(offset, np.float64).reshape(3)
    rec, ext = encode_records(coords, labels, order=order, starts=starts, offset=offset)
    body = rec.cpu().numpy()
    written = []
    for s, p in enumerate(paths):
        if p is None:
            continue
        a, b = int(starts[s]), int(starts[s + 1])
        with open(p, "wb") as f:
            f.write(header_bytes(b - a, offset, ext[s], created))
            f.write(memoryview(body[a * RECORD_LENGTH:b * RECORD_LENGTH]))
        written.append(p)
    return written
