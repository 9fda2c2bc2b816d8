"""Stage times of the light stage on one GPU, on the labelled bench tile (synth.make_tile() defaults: 40 x 40 m, about
1.89 M points, 64 trees, centred f32 coordinates resident on the device) with its terrain built beforehand: the voxel grid
(tl_light_voxels), the sensor grid (terrain sample and tl_light_march over the default 9 x 36 sky table), the derived rasters on the host,
the tree columns (tops by torch plumbing, then tl_light_march), point_light with 64 directions (one march per occupied voxel) and the
marches of a 512 x 512 hemisphere and of the occupied voxels alone -- wall
clock, each stage closed by a device synchronise, median of 3 calls after a warm-up.  For every march also the rays, an estimate of the
voxel steps they take (the planes between a ray's start and its end, from `first` or the exit, on a sample of 4096 origins) and steps per
second.

    python tools/dev_light.py [out.json]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from treelearn_amd.synth import make_tile
from treelearn_amd.util import light as L
from treelearn_amd.util.terrain import terrain_model

REPS = 3
t = make_tile()
xyz = torch.from_numpy(t["points"]).cuda()
lab = torch.from_numpy(t["instance_label"].astype(np.int64)).cuda()
res = {"n_points": len(xyz), "n_trees": int(lab.max())}


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def median_ms(fn):
    fn()
    runs = [timed(fn) for _ in range(REPS)]
    return runs[-1][0], round(1e3 * float(np.median([r[1] for r in runs])), 3)


def steps_of(vox, origins, dirs, skip=None):
    """Voxel steps of a march, without walking again: the planes a ray crosses until it ends are the integer index differences between
    its start and its end, and its end is o + t d at t = first, the exit from the grid or max_range.  Here: an upper estimate from the
    rays' codes and `first` on a sample of at most 4096 origins, scaled to all of them."""
    P = len(origins)
    pick = torch.randperm(P, device=origins.device)[:4096]
    m = L.march(vox, origins[pick], dirs, np.zeros(len(dirs), np.int32), 1, skip=None if skip is None else skip[pick], max_range=p["max_range"], rays=True)
    o = origins[pick][:, None, :]
    d = torch.from_numpy(dirs).to(o.device)[None, :, :]
    lo = torch.tensor([vox.ix0, vox.iy0, vox.iz0], dtype=torch.float64, device=o.device) * vox.voxel
    hi = lo + torch.tensor([vox.nx, vox.ny, vox.nz], dtype=torch.float64, device=o.device) * vox.voxel
    with torch.no_grad():
        t_exit = torch.where(d > 0, (hi - o) / d, torch.where(d < 0, (lo - o) / d, torch.full_like(d + o, float("inf")))).amin(2)
        t_end = torch.where(m["code"] == 0, m["first"], torch.clamp(t_exit, max=p["max_range"]))
        t_end = torch.nan_to_num(t_end, nan=0.0)
        crossed = (torch.floor((o + t_end[:, :, None] * d) / vox.voxel) - torch.floor(o / vox.voxel)).abs().sum(2)
        crossed = torch.where(m["code"] == 255, torch.zeros_like(crossed), crossed)
    return float(crossed.sum()) * P / max(len(pick), 1)


p = L.check_params()
dtm = terrain_model(xyz, lab)
vox, res["voxels_ms"] = median_ms(lambda: L.light_voxels(xyz, lab, p["voxel"]))
res["grid"] = [vox.nx, vox.ny, vox.nz]
res["occ_bytes"] = int(vox.occ.numel() * 4)
res["occupied_voxels"] = int(sum(int(((vox.occ >> b) & 1).sum()) for b in range(32)))
res["rows_per_s"] = round(len(xyz) / (res["voxels_ms"] * 1e-3))

runs = []
for _ in range(REPS + 1):
    st = []
    light = L.light_model(xyz, dtm, lab, stages=st)
    runs.append(dict(st))
for name in runs[0]:
    res["model_" + name.replace(" ", "_") + "_ms"] = round(1e3 * float(np.median([r[name] for r in runs[1:]])), 3)
res["sensors"] = [light.sensor_nx, light.sensor_ny]
res["sensor_rays"] = light.sensor_nx * light.sensor_ny * len(light.sky[0])
known = light.openness[np.isfinite(light.openness)]
res["mean_openness"], res["mean_lai_e"] = float(known.mean()), float(np.nanmean(light.lai_e))
res["n_outside"], res["n_no_ground"] = light.n_outside, light.n_no_ground

dirs, ring, lo, hi = light.sky
gx, gy = np.meshgrid(np.arange(light.sensor_nx), np.arange(light.sensor_ny))
sens = torch.from_numpy(np.column_stack([((light.sensor_ix0 + gx.reshape(-1)) + 0.5) * p["sensor_cell"], ((light.sensor_iy0 + gy.reshape(-1)) + 0.5) * p["sensor_cell"],
                                         light.sensor_z.reshape(-1)])).cuda()
_, res["sensor_march_ms"] = median_ms(lambda: L.march(vox, sens, dirs, ring, len(lo), max_range=p["max_range"]))
res["sensor_steps"] = round(steps_of(vox, sens, dirs))
res["sensor_steps_per_s"] = round(res["sensor_steps"] / (res["sensor_march_ms"] * 1e-3))

T = int(lab.max())
cols, res["tree_columns_ms"] = median_ms(lambda: L.tree_columns(vox, xyz, lab, T, light.sky, p))
res["tree_columns"] = int(cols["light_columns"].sum())
res["tree_rays"] = res["tree_columns"] * len(dirs)
res["tree_mean_gap_zenith"] = float(np.nanmean(cols["light_gap_zenith"]))
st = []
L.tree_columns(vox, xyz, lab, T, light.sky, p, mark=lambda name: (torch.cuda.synchronize(), st.append((name, time.perf_counter()))))
res["tree_columns_march_ms"] = round(1e3 * (st[1][1] - st[0][1]), 3)
hd = L.hemi_directions(512, p["max_zenith"])[0]
one = torch.tensor([[0.0, 0.0, float(dtm.sample(torch.zeros((1, 2), dtype=torch.float64))[0]) + p["sensor_height"]]], dtype=torch.float64)
_, res["hemi_march_512_ms"] = median_ms(lambda: L.march(vox, one, hd, np.zeros(len(hd), np.int32), 1, max_range=p["max_range"], rays=True))
res["hemi_rays"] = len(hd)

pl, res["point_light_64_ms"] = median_ms(lambda: light.point_light(n_rings=2, n_azimuth=32))
res["point_light_origins"] = res["occupied_voxels"]
res["point_light_rays"] = res["occupied_voxels"] * 64
d64, r64 = L.sky_directions(2, 32, p["max_zenith"])[:2]
centres = vox.centres(torch.unique(vox.index(xyz), dim=0))
_, res["point_march_64_ms"] = median_ms(lambda: L.march(vox, centres, d64, r64, 2, max_range=p["max_range"]))
res["point_light_steps"] = round(steps_of(vox, centres, d64))
res["point_light_steps_per_s"] = round(res["point_light_steps"] / (res["point_march_64_ms"] * 1e-3))
res["point_light_mean_openness"] = float(np.nanmean(pl))
_, res["hemi_512_ms"] = median_ms(lambda: light.hemi_picture(0.0, 0.0, 512))
print(json.dumps(res))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
