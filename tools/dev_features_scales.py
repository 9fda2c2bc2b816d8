"""Stage times of the multi-scale geometric features on one GPU, on the bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, f64 coordinates resident on the device), radii 0.2 / 0.4 / 0.6 m, the four columns the leaf-wood seed reads.  In one
process, interleaved, median of REPS after a warm-up, every stage closed by a device synchronise (wall clock):

    one_launch     one sorted_cells at 0.6, one feature_pieces, one tl_eigen_features_scales                 (the new path)
    separate       per radius: sorted_cells at that radius, feature_pieces, tl_eigen_features                (today's path, S times)
    shared_sort    one sorted_cells at 0.6, one feature_pieces, S launches of tl_eigen_features at r_k       (the old kernel on the new sort)

and that every scale of one_launch is the bits of shared_sort.  Then the leaf-wood stage on the labelled tile, stage by stage: one scale
(today) against scales (0.1, 0.3, 0.4) with scales_min 2.  The measurement runs in a child process under its own time limit; a child that
faults or runs out of time ends the tool (nothing else is started on the device).

    python tools/dev_features_scales.py [reps=7]"""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LIMIT_S = 420
RADII = (0.2, 0.4, 0.6)
NAMES = ["linearity", "planarity", "verticality", "number_of_neighbors"]
LEAFWOOD_SCALES, LEAFWOOD_SCALES_MIN = (0.1, 0.3, 0.4), 2


def measure(reps):
    import numpy as np
    import torch
    from treelearn_amd.synth import make_tile
    from treelearn_amd.util import prepare
    from treelearn_amd.util.features import feature_ids
    from treelearn_amd.util.inventory import tree_inventory
    from treelearn_amd.util.leafwood import check_params, stages_of

    tile = make_tile()
    xyz = torch.from_numpy(tile["points"].astype(np.float64)).cuda()
    ids = feature_ids(NAMES)

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def one_launch():
        (sx, skeys, perm, ext), t_sort = timed(lambda: prepare.sorted_cells(xyz, RADII[-1]))
        pieces, t_table = timed(lambda: prepare.feature_pieces(skeys))
        v, t_kernel = timed(lambda: prepare.eigen_features_scales_sorted(sx, skeys, ext, pieces, RADII, ids))
        return v, {"keys_sort": t_sort, "table": t_table, "kernel": t_kernel}

    def separate():
        t = {"keys_sort": 0.0, "table": 0.0, "kernel": 0.0}
        for r in RADII:
            (sx, skeys, perm, ext), a = timed(lambda: prepare.sorted_cells(xyz, r))
            pieces, b = timed(lambda: prepare.feature_pieces(skeys))
            v, c = timed(lambda: prepare.eigen_features_sorted(sx, skeys, ext, pieces, r, ids))
            t["keys_sort"] += a; t["table"] += b; t["kernel"] += c
            t[f"kernel_{r}"] = c
        return None, t

    def shared_sort():
        (sx, skeys, perm, ext), t_sort = timed(lambda: prepare.sorted_cells(xyz, RADII[-1]))
        pieces, t_table = timed(lambda: prepare.feature_pieces(skeys))
        t = {"keys_sort": t_sort, "table": t_table, "kernel": 0.0}
        outs = []
        for r in RADII:
            v, c = timed(lambda: prepare.eigen_features_sorted(sx, skeys, ext, pieces, r, ids))
            t["kernel"] += c
            t[f"kernel_{r}"] = c
            outs.append(v)
        return torch.stack(outs, 1), t

    variants = {"one_launch": one_launch, "separate": separate, "shared_sort": shared_sort}
    outs = {k: f()[0] for k, f in variants.items()}                     # warm-up: code objects, torch's sort and scan
    runs = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():                                   # interleaved
            runs[k].append(f()[1])
    res = {"n_points": len(xyz), "radii": list(RADII), "columns": NAMES, "reps": reps}
    for k, rs in runs.items():
        for stage in sorted(rs[0]):
            res[f"{k}_{stage}_ms"] = round(1e3 * float(np.median([r[stage] for r in rs])), 3)
        res[f"{k}_total_ms"] = round(1e3 * float(np.median([r["keys_sort"] + r["table"] + r["kernel"] for r in rs])), 3)
        res[f"{k}_kernel_min_max_ms"] = [round(1e3 * min(r["kernel"] for r in rs), 3), round(1e3 * max(r["kernel"] for r in rs), 3)]
    res["one_launch_bits_equal_shared_sort"] = bool(torch.equal(outs["one_launch"].view(torch.int32), outs["shared_sort"].view(torch.int32)))
    print(json.dumps(res), flush=True)

    # the leaf-wood stage, one scale against the recommended scales
    lab = torch.from_numpy(tile["instance_label"].astype(np.int64)).cuda()
    pts = torch.from_numpy(tile["points"]).cuda()
    cfg = check_params()
    calls = {"one_scale": {}, "scales": dict(leafwood_scales=LEAFWOOD_SCALES, leafwood_scales_min=LEAFWOOD_SCALES_MIN)}
    for kw in calls.values():
        tree_inventory(pts, lab, leafwood=True, **kw)
    stage_runs = {k: [] for k in calls}
    for _ in range(min(reps, 3)):
        for k, kw in calls.items():
            st = []
            tree_inventory(pts, lab, leafwood=True, stages=st, **kw)
            stage_runs[k].append(dict(st))
    lw = {"leafwood_scales": list(LEAFWOOD_SCALES), "leafwood_scales_min": LEAFWOOD_SCALES_MIN, "rows_of_trees": int((lab >= 1).sum())}
    for k, rs in stage_runs.items():
        for stage in stages_of(cfg):
            lw[f"{k}_{stage.replace(' + ', '_').replace(' ', '_')}_ms"] = round(1e3 * float(np.median([r[stage] for r in rs])), 3)
        lw[f"{k}_wood_rows"] = int(tree_inventory(pts, lab, leafwood=True, **calls[k])["lw_wood_points"].sum())
    print(json.dumps(lw), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--measure":
        measure(int(sys.argv[2]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", str(reps)], timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"the measurement did not finish within {LIMIT_S} s", file=sys.stderr)
        sys.exit(124)
    sys.exit(p.returncode)
