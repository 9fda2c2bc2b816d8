"""Stage times of reading and writing a LAS file on one GPU, on the labelled bench tile (synth.make_tile() defaults: about
1.89 M points): file read, upload, decode, encode, download, file write -- wall clock, each stage closed by a device synchronise, median
of 5 after a warm-up -- and beside them the numpy restatement of tests/las_restatement.py on the host's cores (a CPU-host number).

The kernels are a few tens of microseconds, below what a host clock around one launch resolves, so they are timed with device events
around 20 back-to-back launches, the variants alternating, 5 such batches each after a warm-up: median, lowest and highest per launch.
Decode, plain against staged, at record lengths 34 (point format 3, x y z) and 38 (+ u32 treeID, x y z label); encode (one path; the
staged form that was measured against it is not kept) for the whole cloud and in label order with one segment per label.

    python tools/dev_las.py [restatement=1]"""
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from treelearn_amd.synth import make_tile
from treelearn_amd.util import las

RESTATEMENT = int(sys.argv[1]) if len(sys.argv) > 1 else 1
REPS, BATCH = 5, 20

t = make_tile()
xyz_h = np.ascontiguousarray(t["points"][:, :3])
lab_h = t["instance_label"].astype(np.int64)
n = len(xyz_h)
res = {"n_points": n, "coords_dtype": str(xyz_h.dtype)}
tmp = tempfile.mkdtemp(prefix="dev_las_")
path38 = os.path.join(tmp, "tile38.las")
path34 = os.path.join(tmp, "tile34.las")
las.write_las(path38, xyz_h, lab_h, use_offset=False)
h38 = las.read_header(path38)
raw38 = np.fromfile(path38, np.uint8, offset=h38.offset_to_points).reshape(n, 38)
import las_cases                                                                  # the 34-byte file: the same records without the extra dimension
with open(path34, "wb") as f:
    f.write(las_cases.las_file((1, 2), 3, [np.ascontiguousarray(raw38[:, :34]).tobytes()], h38.scale, h38.offset, count=n, record_length=34))
h34 = las.read_header(path34)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def median_ms(fn):
    fn()
    return round(1e3 * float(np.median([timed(fn)[1] for _ in range(REPS)])), 3)


def per_launch_us(fns):
    """{name: (median, lowest, highest) microseconds per launch}: REPS batches of BATCH launches per function, alternating, device events."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                fn()
            b.record(); b.synchronize()
            got[k].append(1e3 * a.elapsed_time(b) / BATCH)
    return {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


# ---- stages of reading (record length 38)
nbytes = n * 38
pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
out4 = torch.empty((n, 4), dtype=torch.float64, device="cuda")
out3 = torch.empty((n, 3), dtype=torch.float64, device="cuda")


def file_read():
    mm = np.memmap(path38, dtype=np.uint8, mode="r", offset=h38.offset_to_points, shape=(nbytes,))
    pinned.numpy()[:] = mm


res["read_header_ms"] = median_ms(lambda: las.read_header(path38))
res["file_read_ms"] = median_ms(file_read)
res["upload_ms"] = median_ms(lambda: dev.copy_(pinned))
for mode in ("plain", "staged"):
    res[f"decode_{mode}_ms"] = median_ms(lambda: las.decode_records(dev, n, h38, out4, 0, mode))
res["download_rows_ms"] = median_ms(lambda: out4.cpu())
res["read_las_ms"] = median_ms(lambda: las.read_las(path38))

# ---- stages of writing
xyz = torch.from_numpy(xyz_h).cuda()
lab = torch.from_numpy(lab_h).cuda()
res["encode_ms"] = median_ms(lambda: las.encode_records(xyz, lab))                # with the read-back of the error flag and the table
rec, ext = las.encode_records(xyz, lab)
res["download_records_ms"] = median_ms(lambda: rec.cpu())
body = rec.cpu().numpy()


def file_write():
    with open(os.path.join(tmp, "out.las"), "wb") as f:
        f.write(las.header_bytes(n, np.zeros(3), ext[0]))
        f.write(memoryview(body))


res["file_write_ms"] = median_ms(file_write)
res["write_las_ms"] = median_ms(lambda: las.write_las(os.path.join(tmp, "out.las"), xyz, lab, use_offset=False))

# ---- the kernels alone: plain against staged
dev34 = torch.from_numpy(np.ascontiguousarray(raw38[:, :34]).reshape(-1)).cuda()
from treelearn_amd import _hip
L, one = _hip.lib(), las._vec3((las.SCALE,) * 3)
zero = las._vec3((0.0,) * 3)
recbuf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
err = torch.empty(1, dtype=torch.int32, device="cuda")
extbuf = torch.empty((1, 6), dtype=torch.int32, device="cuda")


sl, order = torch.sort(lab, stable=True)                                          # per-tree files: rows in label order, one segment per label
starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.unique_consecutive(sl, return_counts=True)[1], 0)])
n_seg = len(starts) - 1
extseg = torch.empty((n_seg, 6), dtype=torch.int32, device="cuda")
res["n_segments"] = n_seg


def enc(segments=False):
    o, s, k, e = (order, starts, n_seg, extseg) if segments else (None, None, 1, extbuf)
    return lambda: _hip.check(L.tl_las_encode(_hip.ptr(xyz), 0, xyz.stride(0), n, _hip.ptr(lab), _hip.ptr(o), n, one, zero, _hip.ptr(s), k,
                                              _hip.ptr(recbuf), _hip.ptr(err), _hip.ptr(e), _hip.stream()), "tl_las_encode")


assert xyz.dtype == torch.float32
res["kernel_us_median_low_high"] = {
    "decode_34": per_launch_us({m: (lambda m=m: las.decode_records(dev34, n, h34, out3, 0, m)) for m in ("plain", "staged")}),
    "decode_38": per_launch_us({m: (lambda m=m: las.decode_records(dev, n, h38, out4, 0, m)) for m in ("plain", "staged")}),
    "encode_38": per_launch_us({"whole_cloud": enc(), "label_order_segments": enc(True)}),
}
res["encode_paths"] = "one (plain); the staged encode measured in DESIGN.md section 18 was slower and is not in the tree"
res["decode_bytes"] = n * (38 + 32)                                              # a record read, four f64 written
res["encode_bytes"] = n * (3 * 4 + 8 + 38)                                       # x y z f32 + the label read, a record written

if RESTATEMENT:
    import las_restatement as ref
    buf = open(path38, "rb").read()
    t0 = time.perf_counter(); want = ref.read(buf); res["numpy_read_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    t0 = time.perf_counter(); wrec = ref.records(xyz_h, lab_h); res["numpy_records_cpu_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["decode_equal"] = bool((las.read_las(path38).view(np.uint64) == want.view(np.uint64)).all())
    res["encode_equal"] = bool(body.tobytes() == wrec.tobytes())
for f in os.listdir(tmp):
    os.remove(os.path.join(tmp, f))
os.rmdir(tmp)
print(json.dumps(res))
