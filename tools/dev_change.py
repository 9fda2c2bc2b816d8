"""Stage times of the two-epoch comparison on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m,
about 1.89 M points, 64 trees, centred f32 coordinates resident on the device) against a copy of itself, moved by the inverse of a known
transform (yaw 0.5 deg, pitch 0.1 deg, t = (0.08, -0.05, 0.03)) and thinned to every other row: the reference grid (tl_outlier_keys, the
sort, the gather), one tl_cross_nn and one tl_rigid_sums with its read-back at max_dist 1.0 and 0.3, the whole of register, cloud_distance
and match_trees.  HIP events around each stage, median of REPS calls (2 or 3 for the long stages) after a warm-up call of the same
shapes.  For tl_cross_nn also queries per second and the candidate rows a query looks at (the 27 cells, counted on a sample).  For
orientation only, the same search by chunked torch.cdist (f64) on a 200 k-row subsample of both clouds, next to tl_cross_nn on that
subsample.

    python tools/dev_change.py [out.json]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from treelearn_amd.synth import make_tile
from treelearn_amd.util import change as C

REPS = 5
t = make_tile()
ref = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
yaw, pitch = np.deg2rad(0.5), np.deg2rad(0.1)
Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
Ry = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
TRUE = np.eye(4)
TRUE[:3, :3] = Rz @ Ry; TRUE[:3, 3] = (0.08, -0.05, 0.03)
half = ref[1::2].to(torch.float64)
mov = ((half - torch.from_numpy(TRUE[:3, 3]).cuda()) @ torch.from_numpy(TRUE[:3, :3]).cuda()).contiguous()
mov_lab = lab[1::2].contiguous()
res = {"n_ref": len(ref), "n_moving": len(mov), "n_trees": int(lab.max()), "reps": REPS}


def event_ms(fn, reps=REPS):
    fn()                                                                  # warm-up: the same shapes as the timed calls
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); b.synchronize()
        times.append(a.elapsed_time(b))
    return out, round(float(np.median(times)), 3), round(float(max(times) - min(times)), 3)


for max_dist, tag in ((1.0, "1p0"), (0.3, "0p3")):
    R, res[f"grid_{tag}_ms"], res[f"grid_{tag}_spread_ms"] = event_ms(lambda: C._Reference(ref, 1.001 * max_dist))
    (nn, d2), ms, spread = event_ms(lambda: C._cross_nn(R, mov, None, max_dist))
    res[f"cross_nn_{tag}_ms"], res[f"cross_nn_{tag}_spread_ms"] = ms, spread
    res[f"cross_nn_{tag}_queries_per_s"] = round(len(mov) / (ms * 1e-3))
    res[f"cross_nn_{tag}_with_neighbour"] = float((nn >= 0).double().mean())
    # candidate rows of a query: the rows of the 27 cells around it, on a sample, from the sorted keys
    pick = torch.randperm(len(mov), device="cuda", generator=torch.Generator("cuda").manual_seed(0))[:4096]
    lo = torch.tensor(list(R.lo), dtype=torch.float64, device="cuda")
    cell = torch.floor((mov[pick] - lo) / R.h).to(torch.int64)
    rcell = torch.floor((R.ref - lo) / R.h).to(torch.int64)
    key = lambda c: (c[:, 0] * 4096 + c[:, 1]) * 4096 + c[:, 2]           # noqa: E731  (a plain key: only the counts are wanted)
    uk, cnt = torch.unique(key(rcell), return_counts=True)
    cand = torch.zeros(len(pick), dtype=torch.int64, device="cuda")
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = key(cell + torch.tensor([dx, dy, dz], device="cuda"))
                at = torch.searchsorted(uk, k).clamp(max=len(uk) - 1)
                cand += torch.where(uk[at] == k, cnt[at], torch.zeros_like(k))
    res[f"cross_nn_{tag}_candidates_per_query"] = round(float(cand.double().mean()), 1)
    res[f"cross_nn_{tag}_candidates_per_s"] = round(float(cand.double().mean()) * len(mov) / (ms * 1e-3))
    _, res[f"rigid_sums_{tag}_ms"], res[f"rigid_sums_{tag}_spread_ms"] = event_ms(lambda: C._rigid_sums(R, mov, None, nn, d2, max_dist * max_dist))
    st = []
    reg, res[f"register_{tag}_ms"], res[f"register_{tag}_spread_ms"] = event_ms(lambda: (st.clear(), C.register(ref, mov, max_dist=max_dist, stages=st))[1], reps=2)
    res[f"register_{tag}_iterations"] = len(reg.iterations)
    res[f"register_{tag}_converged"] = reg.converged
    res[f"register_{tag}_rms"] = reg.rms
    res[f"register_{tag}_inlier_share"] = reg.inlier_share
    res[f"register_{tag}_max_abs_T_error"] = float(np.abs(reg.T - TRUE).max())
    for name in ("cross_nn", "rigid_sums"):                               # of the last call: the launches alone, the rest is the grid and the host
        res[f"register_{tag}_{name}_total_ms"] = round(float(sum(ms for n, ms in st if n == name)), 3)
    print(tag, {k: v for k, v in res.items() if tag in k}, flush=True)
    if max_dist == 1.0:
        reg1 = reg

reg = reg1
_, res["cloud_distance_1p0_ms"], _ = event_ms(lambda: C.cloud_distance(ref, mov, reg.T, 1.0))
m, res["match_trees_ms"], _ = event_ms(lambda: C.match_trees(ref, lab, mov, mov_lab, reg.T), reps=3)
res["match_pairs"], res["match_unmatched"] = len(m["pairs"]), len(m["unmatched_ref"]) + len(m["unmatched_mov"])

# orientation only: chunked torch.cdist (f64) on a 200 k-row subsample of both clouds
g = torch.Generator("cuda").manual_seed(1)
rs = ref[torch.randperm(len(ref), device="cuda", generator=g)[:200000]].to(torch.float64).contiguous()
qs = mov[torch.randperm(len(mov), device="cuda", generator=g)[:200000]].contiguous()


def by_cdist():
    best = []
    for a in range(0, len(qs), 2048):
        best.append(torch.cdist(qs[a:a + 2048], rs).min(1))
    return torch.cat([b.values for b in best]), torch.cat([b.indices for b in best])


(dist, _), res["cdist_200k_ms"], _ = event_ms(by_cdist, reps=3)
Rs = C._Reference(rs, 1.001)
(nn_s, d2_s), res["cross_nn_200k_ms"], _ = event_ms(lambda: C._cross_nn(Rs, qs, None, 1.0))
near = nn_s >= 0
res["cdist_200k_max_abs_diff"] = float((dist[near] - d2_s[near].sqrt()).abs().max())     # cdist expands |a|^2 + |b|^2 - 2ab: not bit-equal
print(json.dumps(res))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
