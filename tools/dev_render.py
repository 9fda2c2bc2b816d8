"""Stage times of the renderer on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m, about 1.89 M
points, 64 trees, centred f32 coordinates and i64 labels resident on the device): the clear of the canvas, tl_splat by labels for the top
and the south view at 1024^2 and 2048^2 with k = 1, 2, 3, the shade pass, the contact sheet (render_trees, host work included), the copy
of a picture to the host and write_png -- and, for comparison, the same splat written with torch alone (i64 keys through
scatter_reduce("amax")), the only other renderer there is.

Device stages are timed with device events around INNER back-to-back calls, one warm-up first, the median of REPS such windows, with the
least and the largest beside it; everything in one process.  A splat on a canvas that already holds its picture issues no atomic (every
key it reads is already as large), so a timed splat is always clear + splat and the clear is listed on its own to subtract.  Bytes: a row
is 12 B of coordinates and 8 B of label, read once; the canvas stays in cache.

The atomics a splat issues are counted in a build of csrc/tl_render.hip with -DTL_RENDER_COUNT (two atomicAdd per visited pixel: never
the timed kernel), compiled into treelearn_amd/lib/ on first use: `visited` = footprint pixels inside the viewport, `atomics` = those
whose key as read was lower, `pixels` = distinct pixels of the finished picture.

    python tools/dev_render.py [torch_compare=1]
    python tools/dev_render.py --build-only          (compiles the counting build; needs no GPU)"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from treelearn_amd import _hip, build
from treelearn_amd.synth import make_tile
from treelearn_amd.util import render

TORCH_COMPARE = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1
REPS, INNER = 7, 5
COUNT_LIB = os.path.join(build.LIBDIR, "libtl_render_count.so")
PNG = os.path.join(tempfile.gettempdir(), "dev_render.png")


def count_lib():
    src = os.path.join(build.CSRC, "tl_render.hip")
    if not os.path.exists(COUNT_LIB) or os.path.getmtime(COUNT_LIB) < os.path.getmtime(src):
        os.makedirs(build.LIBDIR, exist_ok=True)
        subprocess.run([build.HIPCC] + build.FLAGS + ["-DTL_RENDER_COUNT", "-shared", src, "-o", COUNT_LIB], check=True)
    L = ctypes.CDLL(COUNT_LIB)
    L.tl_splat.restype, L.tl_splat.argtypes = _hip.PROTOTYPES["tl_splat"]
    return L


def timed(fn, inner=INNER):
    """ms per call: median, least, largest of REPS windows of `inner` calls between two device events."""
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return [round(float(v), 4) for v in (np.median(ms), min(ms), max(ms))]


def wall(fn):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [round(float(v), 3) for v in (np.median(ms), min(ms), max(ms))]


if __name__ == "__main__":
    if "--build-only" in sys.argv:                                                    # compile the counting build without a GPU
        count_lib()
        sys.exit(0)
    t = make_tile()
    xyz = torch.from_numpy(t["points"]).cuda()
    lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
    n = len(xyz)
    lo, hi = (v.double().cpu().numpy() for v in torch.aminmax(xyz, dim=0))
    pal = torch.from_numpy(render.default_palette().view(np.int32)).cuda()
    row_bytes = n * (3 * xyz.element_size() + 8)
    res = {"n_points": n, "n_trees": int(lab.max()), "row_bytes": row_bytes, "reps": REPS, "inner": INNER, "columns": "median, least, largest (ms)"}
    lib, counting = _hip.lib(), count_lib()

    def splat(L, keys, flags, view, k, size):
        _hip.check(L.tl_splat(_hip.ptr(xyz), 0, 3, n, None, _hip.ptr(view), 1, 1, 0, _hip.ptr(lab), 0, _hip.ptr(pal), 258, 0.0, 1.0, 0, k, _hip.ptr(keys), size,
                              size, _hip.ptr(flags), _hip.stream()), "tl_splat")

    for size in (1024, 2048):
        keys = torch.zeros((size, size), dtype=torch.int64, device="cuda")
        flags = torch.zeros(4, dtype=torch.int32, device="cuda")
        res[f"clear_{size}_ms"] = timed(keys.zero_)
        for name in ("top", "south"):
            view = torch.from_numpy(render.fit_view(name, lo, hi, (0, 0, size, size))).cuda()
            for k in (1, 2, 3):
                tag = f"{name}_{size}_k{k}"
                both = timed(lambda: (keys.zero_(), splat(lib, keys, flags, view, k, size)))
                only = round(both[0] - res[f"clear_{size}_ms"][0], 4)
                res[f"clear+splat_{tag}_ms"] = both
                res[f"splat_{tag}_ms"] = only
                res[f"splat_{tag}_GBps"] = round(row_bytes / (only * 1e-3) / 1e9, 1)
                keys.zero_(); flags.zero_()
                splat(counting, keys, flags, view, k, size)
                f = flags.tolist()
                res[f"count_{tag}"] = dict(visited=f[2], atomics=f[1], pixels=int((keys != 0).sum()))
                flags.zero_()
        out = torch.empty((size, size, 3), dtype=torch.uint8, device="cuda")
        res[f"shade_{size}_ms"] = timed(lambda: _hip.check(lib.tl_render_shade(_hip.ptr(keys), size, size, 1, 1.0, 0, _hip.ptr(out), None, _hip.stream()),
                                                           "tl_render_shade"))
        res[f"shade_{size}_GBps"] = round(size * size * (8 + 3) / (res[f"shade_{size}_ms"][0] * 1e-3) / 1e9, 1)
        if size == 1024:
            res["copy_to_host_1024_ms"] = wall(lambda: out.cpu())
            img = out.cpu().numpy()
            res["write_png_1024_cpu_host_ms"] = wall(lambda: render.write_png(PNG, img))
            res["png_1024_bytes"] = os.path.getsize(PNG)
    res["contact_sheet_ms"] = wall(lambda: render.render_trees(xyz, lab))
    res["render_cloud_top_south_1024_ms"] = wall(lambda: render.render_cloud(xyz, lab))

    if TORCH_COMPARE:
        size = 1024
        v = render.fit_view("top", lo, hi, (0, 0, size, size))
        view = torch.from_numpy(v).cuda()
        keys = torch.zeros((size, size), dtype=torch.int64, device="cuda")
        flags = torch.zeros(4, dtype=torch.int32, device="cuda")
        lut = torch.from_numpy(render.default_palette().astype(np.int64)).cuda()
        lowest = torch.iinfo(torch.int64).min

        def torch_splat(k):
            """The same picture with torch alone: keys with the top bit flipped so that they order as signed i64; the lowest value = empty."""
            q = xyz.double() - view[9:12]
            a, b, d = ((view[3 * i] * q[:, 0] + view[3 * i + 1] * q[:, 1]) + view[3 * i + 2] * q[:, 2] for i in range(3))
            px = torch.floor(a * view[12] + (view[13] + view[15] / 2.0)).long()
            py = torch.floor((view[14] + view[16] / 2.0) - b * view[12]).long()
            bits = (d + 0.0).float().view(torch.int32).long() & 0xFFFFFFFF
            image = torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF, bits | 0x80000000)
            rgb = lut[torch.where(lab < 0, 0, torch.where(lab == 0, 1, 2 + (lab.clamp_min(1) - 1) % 256))]
            key = ((image - 0x80000000) << 32) | rgb
            out = torch.full((size * size,), lowest, dtype=torch.int64, device="cuda")
            for oy in range(-((k - 1) // 2), k // 2 + 1):
                for ox in range(-((k - 1) // 2), k // 2 + 1):
                    X, Y = px + ox, py + oy
                    keep = (X >= 0) & (X < size) & (Y >= 0) & (Y < size)
                    out.scatter_reduce_(0, (Y * size + X)[keep], key[keep], "amax")
            return out.view(size, size)

        for k in (1, 2, 3):
            res[f"torch_scatter_reduce_top_1024_k{k}_ms"] = timed(lambda: torch_splat(k), inner=2)
            keys.zero_()
            splat(lib, keys, flags, view, k, size)
            tk = torch_splat(k)
            mine = torch.where(keys == 0, torch.full_like(keys, lowest), keys ^ lowest)                # (flip the top bit: u64 order as i64)
            res[f"torch_equal_k{k}"] = bool(torch.equal(mine, tk))
    print(json.dumps(res))
