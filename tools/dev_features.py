"""Stage times of the geometric point features on one GPU, on the bench tile (synth.make_tile() defaults: 40 x 40 m, about
1.89 M points, f64 coordinates resident on the device), search radius 0.6 m.  In one process, interleaved, median of REPS after a warm-up,
every stage closed by a device synchronise (wall clock):

    tl_verticality            the one-column path of compute_features(["verticality"]): keys + sort, kernel
    tl_eigen_features  1 col  ["verticality"]                                          keys + sort, work table, kernel
                       5 col  ["linearity", "planarity", "sphericity", "nz", "verticality"]
                       27 col every feature

and the largest difference between the two verticality columns.  The measurement runs in a child process under its own time limit; a
child that faults or runs out of time ends the tool (nothing else is started on the device).

    python tools/dev_features.py [reps=5]"""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LIMIT_S = 240
FIVE = ["linearity", "planarity", "sphericity", "nz", "verticality"]


def measure(reps):
    import ctypes
    import numpy as np
    import torch
    from treelearn_amd import _hip
    from treelearn_amd.synth import make_tile
    from treelearn_amd.util import prepare
    from treelearn_amd.util.features import FEATURE_NAMES, feature_ids

    R = 0.6
    xyz = torch.from_numpy(make_tile()["points"].astype(np.float64)).cuda()
    n = len(xyz)
    L = _hip.lib()

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def old_path():
        def keys_sort():
            origin = float(xyz.min()) - R
            keys, ext = prepare._keys(xyz, R, origin, False)
            skeys, perm = torch.sort(keys)
            return xyz.index_select(0, perm).contiguous(), skeys, perm, ext
        (sx, skeys, perm, ext), t_sort = timed(keys_sort)

        def kernel():
            v = torch.empty(n, dtype=torch.float32, device=xyz.device)
            _hip.check(L.tl_verticality(_hip.ptr(sx), _hip.ptr(skeys), n, R, (ctypes.c_int64 * 2)(ext[0], ext[1]), _hip.ptr(v), _hip.stream()), "tl_verticality")
            return v
        v, t_kernel = timed(kernel)
        out = torch.empty_like(v); out[perm] = v
        return out, {"keys_sort": t_sort, "table": 0.0, "kernel": t_kernel}

    def new_path(names):
        ids = feature_ids(names)
        (sx, skeys, perm, ext), t_sort = timed(lambda: prepare.sorted_cells(xyz, R))
        pieces, t_table = timed(lambda: prepare.feature_pieces(skeys))
        v, t_kernel = timed(lambda: prepare.eigen_features_sorted(sx, skeys, ext, pieces, R, ids))
        out = torch.empty_like(v); out[perm] = v
        return out, {"keys_sort": t_sort, "table": t_table, "kernel": t_kernel, "pieces": len(pieces)}

    variants = {"tl_verticality": old_path, "eigen_1": lambda: new_path(["verticality"]), "eigen_5": lambda: new_path(FIVE),
                "eigen_27": lambda: new_path(list(FEATURE_NAMES))}
    outs = {k: f()[0] for k, f in variants.items()}                     # warm-up: code objects, torch's sort and scan
    runs = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():                                   # interleaved
            runs[k].append(f()[1])
    res = {"n_points": n, "radius": R, "reps": reps, "pieces": runs["eigen_27"][0]["pieces"]}
    for k, rs in runs.items():
        for stage in ("keys_sort", "table", "kernel"):
            res[f"{k}_{stage}_ms"] = round(1e3 * float(np.median([r[stage] for r in rs])), 3)
        res[f"{k}_kernel_min_max_ms"] = [round(1e3 * min(r["kernel"] for r in rs), 3), round(1e3 * max(r["kernel"] for r in rs), 3)]
    a, b = outs["tl_verticality"], outs["eigen_1"][:, 0]
    both = ~(torch.isnan(a) | torch.isnan(b))
    res["nan_sets_equal"] = bool(torch.equal(torch.isnan(a), torch.isnan(b)))
    res["verticality_max_abs_difference"] = float((a[both].double() - b[both].double()).abs().max())
    res["verticality_bits_equal_27_vs_1"] = bool(torch.equal(outs["eigen_27"][:, FEATURE_NAMES.index("verticality")].view(torch.int32), b.view(torch.int32)))
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure(int(sys.argv[2]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", str(reps)], timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"the measurement did not finish within {LIMIT_S} s", file=sys.stderr)
        sys.exit(124)
    sys.exit(p.returncode)
