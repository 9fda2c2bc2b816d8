"""The light stage restated in numpy float64: the voxel grid of a cloud, the direction table, the walk of a ray through the
grid, the counts per origin and ring, and the derived quantities.  Written from the semantics, not from the kernels: the walk is run for
all rays at once, one step of every unfinished ray per iteration, and every formula is the stated expression in numpy's f64 (IEEE
operations, nothing fused)."""
import numpy as np

DEFAULTS = dict(voxel=0.25, sensor_cell=2.0, sensor_height=1.3, n_rings=9, n_azimuth=36, max_zenith=90.0, max_range=60.0, min_hits=1,
                lai_max_zenith=75.0, zenith_cone=30.0)
MAX_SIDE, MAX_VOXELS, MAX_OWNED = 8192, 1 << 31, 1 << 28


def sky_directions(n_rings=9, n_azimuth=36, max_zenith=90.0):
    """dirs f64[D, 3], ring i32[D], theta_lo, theta_hi f64[R] in degrees; ray r * n_azimuth + a has zenith (r + 0.5) * max_zenith /
    n_rings and azimuth (a + 0.5) * 360 / n_azimuth."""
    dirs, ring = [], []
    for r in range(n_rings):
        th = np.deg2rad((r + 0.5) * max_zenith / n_rings)
        for a in range(n_azimuth):
            ph = np.deg2rad((a + 0.5) * 360.0 / n_azimuth)
            dirs.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
            ring.append(r)
    lo = np.array([r * max_zenith / n_rings for r in range(n_rings)], np.float64)
    hi = np.array([(r + 1) * max_zenith / n_rings for r in range(n_rings)], np.float64)
    return np.array(dirs, np.float64).reshape(-1, 3), np.array(ring, np.int32), lo, hi


def light_voxels(xyz, labels=None, voxel=0.25):
    """dict: i0 (3 ints: ix0, iy0, iz0), n (3 ints: nx, ny, nz), voxel, occ u32[nz, ny, ceil(nx / 32)], full bool[nz, ny, nx] (the same
    bits, one per element), owner i32[nz, ny, nx] or None."""
    xyz = np.asarray(xyz)[:, :3].astype(np.float64)
    v = np.float64(voxel)
    if not np.isfinite(xyz).all():
        raise ValueError("a coordinate is not finite")
    if len(xyz) == 0:
        i0, n = np.zeros(3, np.int64), np.zeros(3, np.int64)
    else:
        i0 = np.floor(xyz.min(0) / v).astype(np.int64)
        n = np.floor(xyz.max(0) / v).astype(np.int64) - i0 + 1
    cells = int(n[0]) * int(n[1]) * int(n[2])
    if n.max() > MAX_SIDE or cells > (MAX_VOXELS if labels is None else MAX_OWNED):
        raise ValueError("the grid is beyond the limits")
    nx, ny, nz = (int(k) for k in n)
    full = np.zeros((nz, ny, nx), bool)
    owner = None if labels is None else np.full((nz, ny, nx), -1, np.int32)
    idx = (np.floor(xyz / v).astype(np.int64) - i0) if len(xyz) else np.zeros((0, 3), np.int64)
    full[idx[:, 2], idx[:, 1], idx[:, 0]] = True
    if labels is not None:
        lab = np.asarray(labels, np.int64)
        for (ix, iy, iz), l in zip(idx, lab):
            if l >= 0 and l > owner[iz, iy, ix]:
                owner[iz, iy, ix] = l
    wx = (nx + 31) // 32
    occ = np.zeros((nz, ny, wx), np.uint32)
    for b in range(nx):
        occ[:, :, b // 32] |= full[:, :, b].astype(np.uint32) << np.uint32(b % 32)
    return dict(i0=[int(k) for k in i0], n=[nx, ny, nz], voxel=float(v), occ=occ, full=full, owner=owner)


def march(vox, origins, dirs, ring, n_rings, skip=None, max_range=60.0, min_hits=1):
    """dict: counts i32[P, R, 4], status i32[P], code u8[P, D] (255 for an origin outside the grid), first f64[P, D]."""
    origins = np.asarray(origins, np.float64).reshape(-1, 3)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    ring = np.asarray(ring, np.int64)
    P, D, R = len(origins), len(dirs), int(n_rings)
    v = np.float64(vox["voxel"])
    i0, n = np.array(vox["i0"], np.int64), np.array(vox["n"], np.int64)
    full, owner = vox["full"], vox["owner"]
    sk = np.full(P, -1, np.int64) if (skip is None or owner is None) else np.asarray(skip, np.int64)
    counts = np.zeros((P, R, 4), np.int32)
    code = np.full((P, D), 255, np.uint8)
    first = np.full((P, D), np.nan)
    with np.errstate(invalid="ignore"):
        fi = np.floor(origins / v) - i0.astype(np.float64)
        inside = ((fi >= 0) & (fi < n.astype(np.float64))).all(1)
    status = np.where(inside, 0, 1).astype(np.int32)
    pi, di = np.meshgrid(np.nonzero(inside)[0], np.arange(D), indexing="ij")
    pi, di = pi.reshape(-1), di.reshape(-1)                                # the rays of the origins inside the grid
    K = len(pi)
    if K == 0:
        return dict(counts=counts, status=status, code=code, first=first)
    o, d = origins[pi], dirs[di]
    i = fi[pi].astype(np.int64)
    s = np.where(d > 0, 1, np.where(d < 0, -1, 0)).astype(np.int64)

    def plane_time(rows, a):
        """t_a of the rays `rows` from their integer index, +inf where the ray does not move along the axis."""
        plane = (i0[a] + i[rows, a] + (s[rows, a] > 0)).astype(np.float64) * v
        t = np.full(len(rows), np.inf)
        mv = s[rows, a] != 0
        t[mv] = (plane[mv] - o[rows[mv], a]) / d[rows[mv], a]
        return t

    everyone = np.arange(K)
    t = np.stack([plane_time(everyone, a) for a in range(3)], axis=1)
    hits = np.zeros(K, np.int64)
    out = np.full(K, -1, np.int64)
    t_first = np.full(K, np.nan)
    act = everyone
    steps = 0
    while len(act):
        steps += 1
        assert steps <= int(n.sum()) + 1, "a walk is bounded by nx + ny + nz steps"
        ta = t[act]
        a = np.zeros(len(act), np.int64)
        a[ta[:, 1] < ta[:, 0]] = 1
        a[ta[:, 2] < ta[np.arange(len(act)), a]] = 2                       # ties go to x, then y, then z
        t_enter = ta[np.arange(len(act)), a]
        far = t_enter > max_range
        out[act[far]] = 2
        act, a, t_enter = act[~far], a[~far], t_enter[~far]
        i[act, a] += s[act, a]
        left = (i[act, a] < 0) | (i[act, a] >= n[a])
        out[act[left]] = np.where((a[left] == 2) & (s[act[left], 2] > 0), 1, 3)
        act, a, t_enter = act[~left], a[~left], t_enter[~left]
        for ax in range(3):
            rows = act[a == ax]
            t[rows, ax] = plane_time(rows, ax)
        hit = full[i[act, 2], i[act, 1], i[act, 0]]
        if owner is not None:
            hit &= (sk[pi[act]] < 0) | (owner[i[act, 2], i[act, 1], i[act, 0]] != sk[pi[act]])
        hits[act[hit]] += 1
        done = hits[act] >= min_hits
        out[act[done]] = 0
        t_first[act[done]] = t_enter[done]
        act = act[~done]
    code[pi, di] = out.astype(np.uint8)
    first[pi, di] = t_first
    ok = (ring[di] >= 0) & (ring[di] < R)
    np.add.at(counts, (pi[ok], ring[di][ok], out[ok]), 1)
    return dict(counts=counts, status=status, code=code, first=first)


def derive(counts, rays, theta_lo, theta_hi, lai_max_zenith=75.0, zenith_cone=30.0):
    """The derived quantities of one set of counts i32[R, 4] with rays[r] rays per ring: dict of gap f64[R], openness, lai_e, gap_zenith,
    edge_share."""
    counts, rays = np.asarray(counts, np.int64), np.asarray(rays, np.int64)
    R = len(rays)
    nan = float("nan")
    gap = np.full(R, nan)
    for r in range(R):
        known = rays[r] - counts[r, 3]
        if known > 0:
            gap[r] = np.float64(counts[r, 1] + counts[r, 2]) / np.float64(known)
    total = int(rays.sum())
    edge = np.float64(counts[:, 3].sum()) / np.float64(total) if total else nan
    lo, hi = np.deg2rad(np.asarray(theta_lo, np.float64)), np.deg2rad(np.asarray(theta_hi, np.float64))
    w = np.cos(lo) - np.cos(hi)
    num = den = 0.0
    for r in range(R):
        if not np.isnan(gap[r]):
            num, den = num + gap[r] * w[r], den + w[r]
    openness = num / den if den > 0 else nan
    mid = (np.asarray(theta_lo, np.float64) + np.asarray(theta_hi, np.float64)) / 2.0
    used = [r for r in range(R) if not np.isnan(gap[r]) and mid[r] <= lai_max_zenith]
    usum = 0.0
    for r in used:
        usum = usum + np.sin(np.deg2rad(mid[r]))
    lai = nan
    if used and usum > 0:
        acc = 0.0
        for r in used:
            g = max(gap[r], 1.0 / (2.0 * np.float64(rays[r])))
            acc = acc + (-np.log(g)) * np.cos(np.deg2rad(mid[r])) * (np.sin(np.deg2rad(mid[r])) / usum)
        lai = 2.0 * acc
    cone = [r for r in range(R) if theta_hi[r] <= zenith_cone]
    open_c = sum(int(counts[r, 1] + counts[r, 2]) for r in cone)
    known_c = sum(int(rays[r] - counts[r, 3]) for r in cone)
    gz = np.float64(open_c) / np.float64(known_c) if known_c > 0 else nan
    return dict(gap=gap, openness=float(openness), lai_e=float(lai), gap_zenith=float(gz), edge_share=float(edge))


def tree_columns(vox, labels_max, sky, **params):
    """The five light columns per tree 1 .. T: one origin per (tree, x, y column) of the grid at the centre of the tree's highest voxel of
    the column -- found from per-tree voxel sets handed in as vox["tree_voxels"]: dict label -> int array [k, 3] of (ix, iy, iz); sky =
    (dirs, ring, theta_lo, theta_hi)."""
    p = dict(DEFAULTS, **params)
    dirs, ring, theta_lo, theta_hi = sky
    n_rings = len(theta_lo)
    T = int(labels_max)
    v = np.float64(vox["voxel"])
    i0 = np.array(vox["i0"], np.int64)
    rays = np.bincount(np.asarray(ring, np.int64), minlength=n_rings)
    out = dict(light_columns=np.zeros(T, np.int64), light_openness=np.full(T, np.nan), light_gap_zenith=np.full(T, np.nan),
               light_lai_above=np.full(T, np.nan), light_edge_share=np.full(T, np.nan))
    for lab in range(1, T + 1):
        vx = vox["tree_voxels"].get(lab)
        if vx is None or len(vx) == 0:
            continue
        tops = {}
        for ix, iy, iz in vx:
            tops[(ix, iy)] = max(tops.get((ix, iy), -1), iz)
        idx = np.array([[ix, iy, iz] for (ix, iy), iz in sorted(tops.items())], np.int64)
        origins = ((i0 + idx).astype(np.float64) + 0.5) * v
        m = march(vox, origins, dirs, ring, n_rings, skip=np.full(len(idx), lab), max_range=p["max_range"], min_hits=p["min_hits"])
        d = derive(m["counts"].astype(np.int64).sum(0), rays * len(idx), theta_lo, theta_hi, p["lai_max_zenith"], p["zenith_cone"])
        out["light_columns"][lab - 1] = len(idx)
        out["light_openness"][lab - 1], out["light_gap_zenith"][lab - 1] = d["openness"], d["gap_zenith"]
        out["light_lai_above"][lab - 1], out["light_edge_share"][lab - 1] = d["lai_e"], d["edge_share"]
    return out


def tree_voxels(xyz, labels, vox):
    """dict label -> unique (ix, iy, iz) of the rows with that label >= 1."""
    xyz = np.asarray(xyz)[:, :3].astype(np.float64)
    idx = np.floor(xyz / np.float64(vox["voxel"])).astype(np.int64) - np.array(vox["i0"], np.int64)
    lab = np.asarray(labels, np.int64)
    return {int(l): np.unique(idx[lab == l], axis=0) for l in np.unique(lab) if l >= 1}
