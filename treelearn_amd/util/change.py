"""Two scans of one plot: rigid registration, cloud-to-cloud distances, and which trees survived, were lost or grew in.

    python -m treelearn_amd.util.change --ref a.las --moving b.las --out change [--dof 4|6] [--max-dist 1] [--reject-min 0.1]
        [--match-dist 0.2] [--min-overlap 0.3] [--stable-band 0.5 4] [--init dx,dy,dz,yaw] [--no-register] [--terrain]
        [--write-registered npy|las]

The semantics are the project's own; tests/change_restatement.py states them in numpy float64 and is the specification.

  register        iterative closest point, one iteration after the other.  The reference is binned ONCE (cell 1.001 * max_dist, the grid of
                  util.outlier).  Per iteration: one tl_cross_nn (the nearest reference row of every moving row under the current T, capped
                  at max_dist), one tl_rigid_sums (17 sums over the pairs with d2 < reject^2, a fixed tree) and one read-back of 17 doubles;
                  then on the host H = S - s_a s_b^T / m, the rotation from numpy's SVD of H with the reflection guard (dof 6) or the yaw
                  atan2(H01 - H10, H00 + H11) (dof 4: levelled scans), the translation b_mean - R a_mean carried back from the centred
                  frame, T <- dT . T.  reject_0 = max_dist, reject_{t+1} = max(reject_min, 3 rms_t), rms_t = sqrt(sum d2 / m).  It stops
                  when dT turns by less than tol_angle and moves the centre by less than tol_shift, else after max_iters.
  cloud_distance  per moving row the distance to the nearest reference row under T, inf beyond max_dist.
  match_trees     tl_cross_nn in both directions at match_dist, every row's neighbour turned into that neighbour's label, two contingency
                  tables (tl_eval_contingency), score(r, m) = (rows of m whose neighbour is in r + rows of r whose neighbour is in m) /
                  (n_r + n_m), Hungarian assignment maximising the score, pairs kept from min_overlap on.  Trees are the labels
                  1 .. max(label) that have rows.
  compare_forests all of it: N x 3 clouds are registered and get the distances; N x 4 clouds (x y z label) also get both inventories, the
                  matching and the change table.

The clouds must agree to within max_dist at the start, or the caller passes `init`: there is no coarse alignment.  Kernels:
csrc/tl_change.hip; there is no CPU fallback."""
import argparse
import csv
import ctypes
import json
import os

import numpy as np

MIN_PAIRS = {4: 3, 6: 6}
STATUSES = ("survivor", "lost", "ingrowth")
_COMPARED = ("height", "dbh", "crown_area")
_COMPARED_GROUND = ("height_ag", "dbh_ag")
_NO_GPU = "treelearn_amd.util.change runs on the GPU (tl_cross_nn); there is no CPU fallback"

__all__ = ["register", "cloud_distance", "match_trees", "compare_forests", "change_table", "write_change", "parse_init", "solve", "Registration"]


# ------------------------------------------------------------------------------------------------ host side of one step
def parse_init(init):
    """A 4 x 4 f64 transform from None (identity), a 4 x 4 matrix or (dx, dy, dz, yaw in degrees)."""
    if init is None:
        return np.eye(4)
    a = np.asarray(init, np.float64)
    if a.shape == (4, 4):
        if not np.isfinite(a).all() or not np.array_equal(a[3], (0.0, 0.0, 0.0, 1.0)):
            raise ValueError("init: a 4 x 4 transform must be finite with the last row 0 0 0 1")
        return a.copy()
    if a.shape != (4,) or not np.isfinite(a).all():
        raise ValueError(f"init must be a 4 x 4 matrix or (dx, dy, dz, yaw_deg), got shape {a.shape}")
    dx, dy, dz, yaw = a
    th = np.deg2rad(yaw)
    T = np.eye(4)
    T[0, 0] = np.cos(th); T[0, 1] = -np.sin(th); T[1, 0] = np.sin(th); T[1, 1] = np.cos(th)
    T[:3, 3] = (dx, dy, dz)
    return T


def solve(sums, c, dof):
    """(dT 4 x 4, angle, shift) of one ICP step from the 17 sums of tl_rigid_sums taken about the centre c."""
    sums = np.asarray(sums, np.float64); c = np.asarray(c, np.float64)
    m = sums[0]
    sa, sb, S = sums[1:4], sums[4:7], sums[7:16].reshape(3, 3)
    H = S - np.outer(sa, sb) / m
    if dof == 6:
        U, _, Vt = np.linalg.svd(H)
        R = Vt.T @ U.T
        if np.linalg.det(R) < 0:                                         # a reflection: flip the axis of the smallest singular value
            Vt = Vt.copy(); Vt[2] = -Vt[2]
            R = Vt.T @ U.T
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        angle = float(np.arctan2(0.5 * np.sqrt(w @ w), 0.5 * (np.trace(R) - 1.0)))       # (arccos of the trace has no resolution near 0)
    else:
        th = np.arctan2(H[0, 1] - H[1, 0], H[0, 0] + H[1, 1])
        R = np.eye(3)
        R[0, 0] = np.cos(th); R[0, 1] = -np.sin(th); R[1, 0] = np.sin(th); R[1, 1] = np.cos(th)
        angle = float(abs(th))
    tc = sb / m - R @ (sa / m)                                            # in the centred frame: where the centre goes
    dT = np.eye(4)
    dT[:3, :3] = R
    dT[:3, 3] = tc + c - R @ c
    return dT, angle, float(np.sqrt(tc @ tc))


def invert(T):
    """The inverse of a rigid 4 x 4 transform: R^T and -(R^T t)."""
    T = np.asarray(T, np.float64)
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


class Registration:
    """T (4 x 4 f64, moving -> reference), iterations (a list of dicts: pairs, rms, reject, angle, shift), converged, inlier_share."""

    def __init__(self, T, iterations, converged, inlier_share):
        self.T, self.iterations, self.converged, self.inlier_share = T, iterations, bool(converged), float(inlier_share)

    @property
    def rms(self):
        return self.iterations[-1]["rms"] if self.iterations else float("nan")


# ------------------------------------------------------------------------------------------------ device side
def _validated(points, name):
    """A host or device array as a tensor of shape [N, 3 or 4], f32 / f64, every coordinate finite.  Touches no GPU for a host array."""
    import torch
    c = points if torch.is_tensor(points) else torch.from_numpy(np.asarray(points))
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError(f"{name} must have shape [N, 3] (or [N, 4], the first three columns are used), got {tuple(c.shape)}")
    if c.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, got {c.dtype}")
    if len(c) and not bool(torch.isfinite(c[:, :3]).all()):
        raise ValueError(f"{name}: a coordinate is not finite")
    return c


def _clouds(*named):
    """Device tensors the kernels read in place (unit column stride), every one validated before the first goes to the device."""
    import torch
    cs = [_validated(p, name) for p, name in named]
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    out = []
    for c in cs:
        c = c.to("cuda")
        out.append(c.contiguous() if len(c) and (c.stride(1) != 1 or c.stride(0) < 3) else c)
    return out


def _rows(c, mask, name):
    import torch
    if mask is None:
        return c
    m = mask if torch.is_tensor(mask) else torch.from_numpy(np.asarray(mask))
    m = m.reshape(-1).to(c.device)
    if m.dtype != torch.bool or m.shape[0] != c.shape[0]:
        raise ValueError(f"{name} must hold one bool per row")
    return c[m].contiguous()


class _Reference:
    """The reference cloud binned once: f64 rows in original order (`ref`), and the Morton-sorted grid of util.outlier."""

    def __init__(self, c, cell):
        import torch
        from .. import _hip
        from .outlier import _D3, _Grid
        self.ref = c[:, :3].to(torch.float64).contiguous()
        self.n = len(self.ref)
        if self.n:
            g = _Grid(self.ref, cell)
            g.check()
            self.xyz, self.keys, self.perm, self.lo, self.h, self.dims = g.xyz, g.keys, g.perm, g.lo, g.h, g.dims
            lo = np.array(list(g.lo)); hi = self.ref.amax(0).cpu().numpy()
            self.centre = (lo + hi) * 0.5
        else:
            self.xyz = self.keys = self.perm = None
            self.lo, self.h, self.dims, self.centre = _D3(0.0, 0.0, 0.0), float(cell), _hip.dims3([1, 1, 1]), np.zeros(3)


def _t12(T):
    return None if T is None else (ctypes.c_double * 12)(*np.asarray(T, np.float64)[:3].reshape(-1))


def _cross_nn(R, q, T, max_dist):
    """(nn i64[nq], d2 f64[nq]) on the device: tl_cross_nn of the rows of q against the reference R."""
    import torch
    from .. import _hip
    nq = len(q)
    nn = torch.empty(nq, dtype=torch.int64, device="cuda"); d2 = torch.empty(nq, dtype=torch.float64, device="cuda")
    if nq:
        _hip.check(_hip.lib().tl_cross_nn(_hip.ptr(R.xyz), _hip.ptr(R.keys), _hip.ptr(R.perm), R.n, R.lo, R.h, R.dims, _hip.ptr(q),
                                          int(q.dtype == torch.float64), q.stride(0), nq, _t12(T), float(max_dist), _hip.ptr(nn), _hip.ptr(d2),
                                          _hip.stream()), "tl_cross_nn")
    return nn, d2


def _rigid_sums(R, q, T, nn, d2, reject2, ws=None, out=None):
    """f64[17] on the host: tl_rigid_sums about the reference's centre and the read-back."""
    import torch
    from .. import _hip
    L, nq = _hip.lib(), len(q)
    if nq == 0:
        return np.zeros(17)
    ws = torch.empty(int(L.tl_rigid_sums_ws_doubles(nq)), dtype=torch.float64, device="cuda") if ws is None else ws
    out = torch.empty(17, dtype=torch.float64, device="cuda") if out is None else out
    from .outlier import _D3
    _hip.check(L.tl_rigid_sums(_hip.ptr(q), int(q.dtype == torch.float64), q.stride(0), nq, _t12(T), _hip.ptr(nn), _hip.ptr(d2), _hip.ptr(R.ref),
                               R.n, _D3(*[float(v) for v in R.centre]), float(reject2), _hip.ptr(out), _hip.ptr(ws), _hip.stream()), "tl_rigid_sums")
    return out.cpu().numpy()


def _check_search(max_dist, name="max_dist"):
    max_dist = float(max_dist)
    if not (max_dist > 0 and np.isfinite(max_dist)):
        raise ValueError(f"{name} must be > 0, got {max_dist!r}")
    return max_dist


def register(ref, moving, *, dof=6, max_dist=1.0, reject_min=0.1, max_iters=50, tol_angle=1e-7, tol_shift=1e-6, init=None, ref_mask=None,
             moving_mask=None, stages=None):
    """ICP of `moving` onto `ref` ([N, 3] or [N, 4] f32 / f64, numpy arrays or tensors).  Returns a Registration.  `ref_mask` /
    `moving_mask` (one bool per row) choose the rows that register, a stem band for example.  ValueError for a coordinate that is not
    finite (before any launch) and for fewer than 3 (dof 4) or 6 (dof 6) pairs.  `stages`: a list that receives (name, HIP-event
    milliseconds) per launch (tools/dev_change.py)."""
    import torch
    if dof not in MIN_PAIRS:
        raise ValueError(f"dof must be 4 or 6, got {dof!r}")
    max_dist = _check_search(max_dist)
    reject_min = float(reject_min)
    if not reject_min > 0 or int(max_iters) < 1:
        raise ValueError("reject_min must be > 0 and max_iters >= 1")
    T = parse_init(init)
    r, q = _clouds((ref, "ref"), (moving, "moving"))
    r, q = _rows(r, ref_mask, "ref_mask"), _rows(q, moving_mask, "moving_mask")
    R = _Reference(r, 1.001 * max_dist)
    from .. import _hip
    ws = torch.empty(int(_hip.lib().tl_rigid_sums_ws_doubles(max(1, len(q)))), dtype=torch.float64, device="cuda")
    out = torch.empty(17, dtype=torch.float64, device="cuda")

    def timed(name, fn):
        if stages is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); res = fn(); b.record(); b.synchronize()
        stages.append((name, a.elapsed_time(b)))
        return res

    reject, log, converged = max_dist, [], False
    for _ in range(int(max_iters)):
        nn, d2 = timed("cross_nn", lambda: _cross_nn(R, q, T, max_dist))
        sums = timed("rigid_sums", lambda: _rigid_sums(R, q, T, nn, d2, reject * reject, ws, out))
        m = int(sums[0])
        if m < MIN_PAIRS[dof]:
            raise ValueError(f"{m} pairs within max_dist = {max_dist} (dof {dof} needs {MIN_PAIRS[dof]}): the clouds do not overlap at the "
                             "start; pass init or a larger max_dist")
        dT, angle, shift = solve(sums, R.centre, dof)
        T = dT @ T
        rms = float(np.sqrt(sums[16] / sums[0]))
        log.append(dict(pairs=m, rms=rms, reject=reject, angle=angle, shift=shift))
        reject = max(reject_min, 3.0 * rms)
        if angle < tol_angle and shift < tol_shift:
            converged = True
            break
    return Registration(T, log, converged, log[-1]["pairs"] / max(1, len(q)))


def cloud_distance(ref, moving, T=None, max_dist=1.0):
    """(dist f64[nq], nn i64[nq]) on the device: per moving row the distance to its nearest reference row under T (4 x 4, None =
    identity) and that row; inf and -1 where none lies within max_dist."""
    max_dist = _check_search(max_dist)
    T = None if T is None else parse_init(T)
    r, q = _clouds((ref, "ref"), (moving, "moving"))
    nn, d2 = _cross_nn(_Reference(r, 1.001 * max_dist), q, T, max_dist)
    return d2.sqrt(), nn


def _labels(a, n, name):
    import torch
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)).astype(np.int64, copy=False))
    t = t.reshape(-1).to("cuda", torch.int64).contiguous()
    if t.shape[0] != n:
        raise ValueError(f"mismatched lengths: {n} coordinates for {t.shape[0]} {name}")
    return t


def _neighbour_table(own, other, nn, n_own, n_other):
    """i64 [n_own + 1, n_other + 2] on the host: row t = the rows of own tree t (row 0: no tree); column 0 = no neighbour, column 1 = a
    neighbour that is no tree, column 1 + u = a neighbour in the other epoch's tree u."""
    import torch
    from .eval import _contingency
    if own.numel() == 0:
        return np.zeros((n_own + 1, n_other + 2), np.int64)
    code = torch.full_like(nn, -1) if other.numel() == 0 else torch.where(nn >= 0, other.clamp(min=0)[nn.clamp(min=0)], torch.full_like(nn, -1))
    return _contingency(torch.where(own > 0, own - 1, torch.full_like(own, -1)), code, n_own, n_other + 1, -1)


def match_trees(ref_xyz, ref_labels, mov_xyz, mov_labels, T, match_dist=0.2, min_overlap=0.3):
    """Pair the trees of two epochs.  T (4 x 4, None = identity) takes the moving cloud to the reference.  Returns a dict: pairs (a list of
    (ref id, moving id, score), ascending ref id), unmatched_ref, unmatched_mov (ids), lost_points i64[max ref label] (per reference tree
    the rows with no moving row within match_dist), gained_points i64[max moving label] (the same on the moving side), n_ref, n_mov (rows
    per tree).  Label 0 and negative labels are not trees."""
    from scipy.optimize import linear_sum_assignment
    match_dist = _check_search(match_dist, "match_dist")
    T = parse_init(T)
    r, q = _clouds((ref_xyz, "ref_xyz"), (mov_xyz, "mov_xyz"))
    rl, ml = _labels(ref_labels, len(r), "ref_labels"), _labels(mov_labels, len(q), "mov_labels")
    nn_m, _ = _cross_nn(_Reference(r, 1.001 * match_dist), q, T, match_dist)                   # per moving row: a reference row
    nn_r, _ = _cross_nn(_Reference(q, 1.001 * match_dist), r, invert(T), match_dist)           # per reference row: a moving row
    Tr = max(int(rl.max()), 0) if len(rl) else 0
    Tm = max(int(ml.max()), 0) if len(ml) else 0
    A = _neighbour_table(ml, rl, nn_m, Tm, Tr)                                                 # [Tm + 1, Tr + 2]
    B = _neighbour_table(rl, ml, nn_r, Tr, Tm)                                                 # [Tr + 1, Tm + 2]
    n_r, n_m = B[1:].sum(1), A[1:].sum(1)
    den = (n_r[:, None] + n_m[None, :]).astype(np.float64)
    score = np.where(den > 0, (A[1:, 2:].T + B[1:, 2:]) / np.maximum(den, 1.0), 0.0)           # [Tr, Tm]
    pairs = []
    if Tr and Tm:
        rows, cols = linear_sum_assignment(score, maximize=True)
        pairs = [(int(a) + 1, int(b) + 1, float(score[a, b])) for a, b in zip(rows, cols)
                 if n_r[a] > 0 and n_m[b] > 0 and score[a, b] >= min_overlap]
    mr, mm = {p[0] for p in pairs}, {p[1] for p in pairs}
    return dict(pairs=pairs, unmatched_ref=[t for t in range(1, Tr + 1) if n_r[t - 1] > 0 and t not in mr],
                unmatched_mov=[t for t in range(1, Tm + 1) if n_m[t - 1] > 0 and t not in mm],
                lost_points=B[1:, 0].astype(np.int64), gained_points=A[1:, 0].astype(np.int64), n_ref=n_r.astype(np.int64), n_mov=n_m.astype(np.int64))


# ------------------------------------------------------------------------------------------------ the change table
def table_columns(ground=False):
    cols = ["status", "ref_id", "mov_id", "overlap", "d_position"]
    for k in _COMPARED + (_COMPARED_GROUND if ground else ()):
        cols += [f"{k}_ref", f"{k}_mov", f"d_{k}"]
    return tuple(cols + ["gained_points", "lost_points"])


def change_table(match, inv_ref, inv_mov, T):
    """One row per tree of either epoch, as a dict of lists keyed by table_columns(): the survivors by ascending ref id, then the lost
    trees, then the ingrowth by ascending moving id.  d_position is the horizontal distance between the reference tree's position and
    the moving tree's position carried over by T; d_* = moving - reference.  A missing side holds NaN and the id -1."""
    T = parse_init(T)
    ground = all(k in inv_ref and k in inv_mov for k in _COMPARED_GROUND)
    cols = table_columns(ground)
    out = {k: [] for k in cols}
    nan = float("nan")

    def value(inv, k, t):
        return float(inv[k][t - 1]) if t > 0 and t <= len(inv[k]) else nan

    def row(status, r, m, score):
        out["status"].append(status); out["ref_id"].append(r); out["mov_id"].append(m); out["overlap"].append(score)
        d = nan
        if r > 0 and m > 0:
            p = np.array([value(inv_mov, k, m) for k in ("x", "y", "z")])
            p = T[:3, :3] @ p + T[:3, 3]
            d = float(np.hypot(p[0] - value(inv_ref, "x", r), p[1] - value(inv_ref, "y", r)))
        out["d_position"].append(d)
        for k in _COMPARED + (_COMPARED_GROUND if ground else ()):
            a, b = value(inv_ref, k, r), value(inv_mov, k, m)
            out[f"{k}_ref"].append(a); out[f"{k}_mov"].append(b); out[f"d_{k}"].append(b - a)
        out["gained_points"].append(int(match["gained_points"][m - 1]) if m > 0 else 0)
        out["lost_points"].append(int(match["lost_points"][r - 1]) if r > 0 else 0)

    for r, m, s in sorted(match["pairs"]):
        row("survivor", int(r), int(m), float(s))
    for r in sorted(match["unmatched_ref"]):
        row("lost", int(r), -1, nan)
    for m in sorted(match["unmatched_mov"]):
        row("ingrowth", -1, int(m), nan)
    return out


def _band_mask(points, band, terrain_cfg):
    """bool[N] (device): the rows whose height above the cloud's own terrain lies in [band[0], band[1])."""
    from .terrain import cloud_terrain
    terrain, centred = cloud_terrain(points, **(terrain_cfg or {}))
    hag = terrain.height_above_ground(centred)
    return (hag >= float(band[0])) & (hag < float(band[1]))


def compare_forests(ref_points, moving_points, *, dof=6, max_dist=1.0, reject_min=0.1, max_iters=50, tol_angle=1e-7, tol_shift=1e-6, init=None,
                    registration=True, match_dist=0.2, min_overlap=0.3, stable_band=None, terrain=False, terrain_cfg=None, **inventory_params):
    """Everything at once for two N x 3 or two N x 4 (x y z label) clouds.  Returns a dict: T, T_inv (4 x 4), registration (a Registration,
    None with registration=False: T is then `init`), distance_moving / distance_ref (f64 device tensors: per row of one cloud the distance
    to the other, inf beyond max_dist) and, for N x 4 clouds, inventory_ref, inventory_mov (util.inventory.cloud_inventory, with the ground
    columns when terrain=True), match (match_trees) and table (change_table).  stable_band = (lo, hi) registers on the rows whose height
    above ground (util.terrain) lies in the band, on both sides."""
    import torch
    from .inventory import check_params as check_inventory
    check_inventory(**inventory_params)
    if terrain or stable_band is not None:
        from .terrain import check_params as check_terrain
        terrain_cfg = check_terrain(terrain_cfg)
    if stable_band is not None and not (len(stable_band) == 2 and float(stable_band[0]) < float(stable_band[1])):
        raise ValueError(f"stable_band must be (lo, hi) with lo < hi, got {stable_band!r}")
    ref_t = ref_points if torch.is_tensor(ref_points) else torch.from_numpy(np.ascontiguousarray(ref_points))
    mov_t = moving_points if torch.is_tensor(moving_points) else torch.from_numpy(np.ascontiguousarray(moving_points))
    if ref_t.ndim != 2 or mov_t.ndim != 2 or ref_t.shape[1] not in (3, 4) or ref_t.shape[1] != mov_t.shape[1]:
        raise ValueError(f"expected two N x 3 or two N x 4 clouds, got {tuple(ref_t.shape)} and {tuple(mov_t.shape)}")
    labelled = ref_t.shape[1] == 4
    r, q = _clouds((ref_t, "ref_points"), (mov_t, "moving_points"))
    rx, qx = r[:, :3].to(torch.float64).contiguous(), q[:, :3].to(torch.float64).contiguous()
    reg = None
    T = parse_init(init)
    if registration:
        masks = {}
        if stable_band is not None:
            masks = dict(ref_mask=_band_mask(r, stable_band, terrain_cfg), moving_mask=_band_mask(q, stable_band, terrain_cfg))
        reg = register(rx, qx, dof=dof, max_dist=max_dist, reject_min=reject_min, max_iters=max_iters, tol_angle=tol_angle, tol_shift=tol_shift,
                       init=T, **masks)
        T = reg.T
    Ti = invert(T)
    res = dict(T=T, T_inv=Ti, registration=reg, max_dist=float(max_dist))
    res["distance_moving"], res["nn_moving"] = cloud_distance(rx, qx, T, max_dist)
    res["distance_ref"], res["nn_ref"] = cloud_distance(qx, rx, Ti, max_dist)
    if labelled:
        from .inventory import cloud_inventory
        rl, ml = r[:, 3].to(torch.int64), q[:, 3].to(torch.int64)
        res["inventory_ref"] = cloud_inventory(r, terrain=terrain, terrain_cfg=terrain_cfg if terrain else None, **inventory_params)
        res["inventory_mov"] = cloud_inventory(q, terrain=terrain, terrain_cfg=terrain_cfg if terrain else None, **inventory_params)
        res["match"] = match_trees(rx, rl, qx, ml, T, match_dist=match_dist, min_overlap=min_overlap)
        res["table"] = change_table(res["match"], res["inventory_ref"], res["inventory_mov"], T)
    return res


def write_table(path, table):
    """change.csv: a header row, then one row per tree; floats as repr, NaN as `nan`."""
    cols = [k for k in table_columns(ground="height_ag_ref" in table)]
    ints = ("ref_id", "mov_id", "gained_points", "lost_points")
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for i in range(len(table["status"])):
            w.writerow([table[k][i] if k == "status" else str(int(table[k][i])) if k in ints else repr(float(table[k][i])) for k in cols])
    return path


def write_change(out_dir, result, write_registered=None, moving_points=None):
    """Writes transform.json (T, its inverse, the iteration log, rms and inlier share), change.csv (labelled clouds), distance_moving.npy
    and distance_ref.npy, and with write_registered = "npy" or "las" the moving cloud carried over by T (registered.npy / .las; needs
    moving_points).  Returns the paths."""
    import torch
    if write_registered not in (None, "npy", "las"):
        raise ValueError(f"write_registered must be 'npy' or 'las', got {write_registered!r}")
    if write_registered and moving_points is None:
        raise ValueError("write_registered needs moving_points")
    os.makedirs(out_dir, exist_ok=True)
    reg = result.get("registration")
    meta = dict(T=np.asarray(result["T"]).tolist(), T_inv=np.asarray(result["T_inv"]).tolist(), registered=reg is not None,
                iterations=reg.iterations if reg else [], converged=reg.converged if reg else None, rms=reg.rms if reg else None,
                inlier_share=reg.inlier_share if reg else None, max_dist=result.get("max_dist"))
    paths = [os.path.join(out_dir, "transform.json")]
    with open(paths[0], "w") as f:
        json.dump(meta, f, indent=1)
    for k in ("distance_moving", "distance_ref"):
        v = result[k]
        paths.append(os.path.join(out_dir, k + ".npy"))
        np.save(paths[-1], v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
    if "table" in result:
        paths.append(write_table(os.path.join(out_dir, "change.csv"), result["table"]))
    if write_registered:
        pts = moving_points.cpu().numpy() if torch.is_tensor(moving_points) else np.asarray(moving_points)
        T = np.asarray(result["T"], np.float64)
        x, y, z = (pts[:, a].astype(np.float64) for a in range(3))
        moved = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)
        lab = pts[:, 3].astype(np.int64) if pts.shape[1] == 4 else np.zeros(len(pts), np.int64)
        if write_registered == "npy":
            paths.append(os.path.join(out_dir, "registered.npy"))
            np.save(paths[-1], np.column_stack([moved, lab.astype(np.float64)]) if pts.shape[1] == 4 else moved)
        else:
            from .las import write_las
            paths.append(write_las(os.path.join(out_dir, "registered.las"), moved, lab))
    return paths


# ------------------------------------------------------------------------------------------------ command line
def _init_arg(s):
    try:
        v = [float(x) for x in s.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected dx,dy,dz,yaw, got {s!r}")
    if len(v) != 4 or not np.isfinite(v).all():
        raise argparse.ArgumentTypeError(f"expected four finite numbers dx,dy,dz,yaw, got {s!r}")
    return tuple(v)


def parse_args(argv=None):
    ap = argparse.ArgumentParser("python -m treelearn_amd.util.change", description="compare two scans of one plot: registration, distances, tree matching")
    ap.add_argument("--ref", required=True, help="the first epoch: .npy / .npz / .txt / .las, N x 3 or N x 4 (x y z label)")
    ap.add_argument("--moving", required=True, help="the second epoch, same kind; it is carried into the frame of --ref")
    ap.add_argument("--out", required=True, help="directory for transform.json, change.csv and the distances")
    ap.add_argument("--dof", type=int, choices=(4, 6), default=6, help="6: any rigid motion; 4: yaw and translation (levelled scans)")
    ap.add_argument("--max-dist", type=float, default=1.0, help="pairs farther apart than this are never formed, metres")
    ap.add_argument("--reject-min", type=float, default=0.1, help="the rejection distance never falls below this, metres")
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--match-dist", type=float, default=0.2, help="rows closer than this count as the same surface when trees are paired")
    ap.add_argument("--min-overlap", type=float, default=0.3, help="a pair of trees is kept from this score on")
    ap.add_argument("--stable-band", type=float, nargs=2, metavar=("LO", "HI"), help="register on the rows this high above ground only, metres")
    ap.add_argument("--init", type=_init_arg, help="starting guess dx,dy,dz,yaw (metres, degrees)")
    ap.add_argument("--no-register", action="store_true", help="take --init (or the identity) as the transform")
    ap.add_argument("--terrain", action="store_true", help="compare height and DBH from the ground as well")
    ap.add_argument("--write-registered", choices=("npy", "las"), help="also write the moving cloud in the frame of --ref")
    a = ap.parse_args(argv)
    for k in ("max_dist", "reject_min", "match_dist"):
        if not (getattr(a, k) > 0 and np.isfinite(getattr(a, k))):
            ap.error(f"--{k.replace('_', '-')} must be > 0")
    if not 0 <= a.min_overlap <= 1:
        ap.error("--min-overlap must lie in 0 .. 1")
    if a.max_iters < 1:
        ap.error("--max-iters must be >= 1")
    if a.stable_band and not a.stable_band[0] < a.stable_band[1]:
        ap.error("--stable-band LO HI needs LO < HI")
    for k in ("ref", "moving"):
        if not os.path.exists(getattr(a, k)):
            ap.error(f"--{k} {getattr(a, k)}: no such file")
    return ap, a


def main(argv=None):
    ap, a = parse_args(argv)
    from .segment import load_forest
    ref, mov = load_forest(a.ref), load_forest(a.moving)
    if ref.shape[1] != mov.shape[1]:
        ap.error(f"--ref has {ref.shape[1]} columns and --moving {mov.shape[1]}: both need labels, or neither")
    res = compare_forests(ref, mov, dof=a.dof, max_dist=a.max_dist, reject_min=a.reject_min, max_iters=a.max_iters, init=a.init,
                          registration=not a.no_register, match_dist=a.match_dist, min_overlap=a.min_overlap, stable_band=a.stable_band,
                          terrain=a.terrain)
    write_change(a.out, res, write_registered=a.write_registered, moving_points=mov)
    reg = res["registration"]
    line = f"{a.ref} <- {a.moving}: " + (f"{len(reg.iterations)} iterations, rms {reg.rms:.4f} m, inlier share {reg.inlier_share:.3f}" if reg else "not registered")
    if "table" in res:
        st = res["table"]["status"]
        line += "; " + ", ".join(f"{st.count(s)} {s}" for s in STATUSES)
    print(line + f" -> {a.out}")


if __name__ == "__main__":
    main()
