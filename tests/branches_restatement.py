"""Branch structure of a labelled cloud, restated in plain Python and numpy float64.  The yardstick of csrc/tl_skeleton.hip
and util/branches.py: a heap Dijkstra over a dict of voxels, a flood fill for the nodes, recursion-free passes over the node table for the
branches.  It imports nothing from the package.

Per tree t (label t + 1): the position (px, py) and a reference height z_ref.
  voxels    (ix, iy, iz) = floor(coordinate / voxel); (ipx, ipy, izr) = floor((px, py, z_ref) / voxel); the tree's voxels are the distinct
            voxels of its rows with iz >= izr.  ValueError for a row of a tree with a coordinate that is not finite, or a row with iz >= izr
            and |ix - ipx| > 2047, |iy - ipy| > 2047 or iz - izr >= 2047.  A tree whose px, py or z_ref is not finite has no voxels.  More
            than max_voxels voxels: skel_voxels and no skeleton.
  graph     an edge between two voxels of the tree with max(|dx|, |dy|, |dz|) <= reach, weight floor(sqrt(10000 * (dx^2 + dy^2 + dz^2))).
  sources   of the voxels with max(|ix - ipx|, |iy - ipy|) <= base_reach, those with iz - iz0 < base_layers, iz0 the lowest of them.
  distance  d(v): the shortest path from the sources; -1 where no path leads.
  nodes     bin(v) = d(v) // (100 * level); a node is a connected component of reached voxels of one bin, numbered in ascending (bin, smallest
            voxel), voxels ordered as tuples (ix, iy, iz).  Centroid ((double)sum / (double)count + 0.5) * voxel.  Parent of a node of bin > 0:
            the node of the predecessor u of its voxel v* of the smallest (d, voxel): d(u) + w(u, v*) = d(v*), the smallest such voxel.
  branches  seg, path, down, the continuation child, orders, branch ids, the axis and the columns as the issue of DESIGN §23 states them
            (see util/branches.py's docstring; the sums here are math.fsum, the kernels' host side adds in index order).
`offset` is added to the skeleton's xyz at the end; heights are relative and get none.

Margins.  The integer results depend on float decisions only through px, py and z_ref (which differ between implementations in the last
bits) and through the three float comparisons of the branch rules.  `margins` holds the smallest distance of each kind (inf where no such
decision was taken); a fixture is admissible only when min(margins.values()) > 1e-6.  Kinds: voxel (the distance of px / voxel and py / voxel
from an integer, in voxels, over the trees with rows), z_ref (the same for z_ref / voxel; tree_branches sets it to inf without a terrain,
where z_ref = z_low is a rank of the rows' own z: the same bits everywhere), min_branch (|length - min_branch| over the branches of order >=
1), min_height (|attachment height - min_height| over the counted order-1 branches that leave the axis), continuation (the lead of the
best child's seg + down over the runner-up's, and of the axis' root over the other roots; an exact tie, the mirror case, is decided by
the index and is not counted)."""
import heapq
import math

import numpy as np

BRANCH_DEFAULTS = dict(voxel=0.1, reach=1, base_reach=10, base_layers=5, level=3, min_branch=0.5, min_height=1.0, max_voxels=1 << 20)
BRANCH_COLUMNS = ("skel_voxels", "skel_reached", "skel_nodes", "skel_tips", "skel_length", "axis_length", "axis_top_h", "path_mean_tips",
                  "branch_count", "branch_count_1", "branch_length", "branch_order_max", "first_branch_h")
BRANCH_INT = ("skel_voxels", "skel_reached", "skel_nodes", "skel_tips", "branch_count", "branch_count_1", "branch_order_max")
SKELETON_KEYS = ("node_start", "xyz", "parent", "bin", "count", "order", "branch")
MARGIN_KINDS = ("voxel", "z_ref", "min_branch", "min_height", "continuation")
MIN_MARGIN = 1e-6
HALF, Z_MAX = 2048, 2047


def weight(dx, dy, dz):
    return int(math.floor(math.sqrt(10000 * (dx * dx + dy * dy + dz * dz))))


def offsets(reach):
    r = range(-reach, reach + 1)
    return [(dx, dy, dz, weight(dx, dy, dz)) for dx in r for dy in r for dz in r if (dx, dy, dz) != (0, 0, 0)]


def geodesic(vox, base, cfg):
    """{voxel: d} of the reached voxels of the set `vox` (tuples), base = (ipx, ipy); None without a source."""
    near = [v for v in vox if max(abs(v[0] - base[0]), abs(v[1] - base[1])) <= cfg["base_reach"]]
    if not near:
        return None
    iz0 = min(v[2] for v in near)
    d = {v: 0 for v in near if v[2] - iz0 < cfg["base_layers"]}
    heap = [(0, v) for v in d]
    heapq.heapify(heap)
    offs = offsets(cfg["reach"])
    done = set()
    while heap:
        dv, v = heapq.heappop(heap)
        if v in done:
            continue
        done.add(v)
        for dx, dy, dz, w in offs:
            u = (v[0] + dx, v[1] + dy, v[2] + dz)
            if u in vox and dv + w < d.get(u, 1 << 62):
                d[u] = dv + w
                heapq.heappush(heap, (dv + w, u))
    return d


def nodes_of(d, cfg):
    """The node table of one tree from {voxel: d}: a list of dicts (bin, voxels sorted, first = v*), in node order, and {voxel: node}."""
    step, offs = 100 * cfg["level"], offsets(cfg["reach"])
    seen, nodes = set(), []
    for v in sorted(d):
        if v in seen:
            continue
        b, comp, stack = d[v] // step, [], [v]
        seen.add(v)
        while stack:
            a = stack.pop()
            comp.append(a)
            for dx, dy, dz, _ in offs:
                u = (a[0] + dx, a[1] + dy, a[2] + dz)
                if u in d and u not in seen and d[u] // step == b:
                    seen.add(u)
                    stack.append(u)
        comp.sort()
        nodes.append(dict(bin=b, voxels=comp, first=min(comp, key=lambda a: (d[a], a))))
    nodes.sort(key=lambda nd: (nd["bin"], nd["voxels"][0]))
    owner = {a: i for i, nd in enumerate(nodes) for a in nd["voxels"]}
    for nd in nodes:
        nd["parent"] = -1
        if nd["bin"] > 0:
            v = nd["first"]
            pred = [(v[0] + dx, v[1] + dy, v[2] + dz) for dx, dy, dz, w in offs if d.get((v[0] + dx, v[1] + dy, v[2] + dz), -10 ** 9) + w == d[v]]
            nd["parent"] = owner[min(pred)]
    return nodes


def branches_of(xyz, parent, z_ref, cfg, margins):
    """The branch rules on one tree's node table (xyz [n, 3] f64, parent: list).  Returns (columns of the tree, order, branch)."""
    n = len(parent)
    seg = [0.0] * n
    for i, q in enumerate(parent):
        if q >= 0:
            dx, dy, dz = (float(xyz[i][k]) - float(xyz[q][k]) for k in range(3))
            seg[i] = math.sqrt(dx * dx + dy * dy + dz * dz)
    kids = [[] for _ in range(n)]
    for i, q in enumerate(parent):
        if q >= 0:
            kids[q].append(i)
    path, down, cont = [0.0] * n, [0.0] * n, [-1] * n
    for i in range(n):
        if parent[i] >= 0:
            path[i] = path[parent[i]] + seg[i]
    for i in range(n - 1, -1, -1):
        if kids[i]:
            vals = sorted(((seg[j] + down[j], -j) for j in kids[i]), reverse=True)
            down[i], cont[i] = vals[0][0], -vals[0][1]
            for v, _ in vals[1:]:
                if v != vals[0][0]:
                    margins["continuation"] = min(margins["continuation"], vals[0][0] - v)
    order, branch, b_nodes = [0] * n, [0] * n, []
    for i in range(n):
        q = parent[i]
        if q >= 0 and cont[q] == i:
            order[i], branch[i] = order[q], branch[q]
            b_nodes[branch[i]].append(i)
        else:
            order[i], branch[i] = (0 if q < 0 else order[q] + 1), len(b_nodes)
            b_nodes.append([i])
    roots = [i for i in range(n) if parent[i] < 0]
    top = max(down[i] for i in roots)
    axis_root = min(i for i in roots if down[i] == top)
    for i in roots:
        if down[i] != top:
            margins["continuation"] = min(margins["continuation"], top - down[i])
    axis = branch[axis_root]
    b_len = [math.fsum(seg[i] for i in nodes) for nodes in b_nodes]
    b_order = [order[nodes[0]] for nodes in b_nodes]
    for k in range(len(b_nodes)):
        if b_order[k] >= 1:
            margins["min_branch"] = min(margins["min_branch"], abs(b_len[k] - cfg["min_branch"]))
    counted = [k for k in range(len(b_nodes)) if b_order[k] >= 1 and b_len[k] >= cfg["min_branch"]]
    heights = []
    for k in counted:
        q = parent[b_nodes[k][0]]
        if b_order[k] == 1 and branch[q] == axis:
            h = float(xyz[q][2]) - z_ref
            margins["min_height"] = min(margins["min_height"], abs(h - cfg["min_height"]))
            if h >= cfg["min_height"]:
                heights.append(h)
    tips = [i for i in range(n) if not kids[i]]
    col = dict(skel_tips=len(tips), skel_length=math.fsum(seg), axis_length=b_len[axis], axis_top_h=float(xyz[b_nodes[axis][-1]][2]) - z_ref,
               path_mean_tips=math.fsum(path[i] for i in tips) / len(tips), branch_count=len(counted),
               branch_count_1=sum(1 for k in counted if b_order[k] == 1), branch_length=math.fsum(b_len[k] for k in counted),
               branch_order_max=max([b_order[k] for k in counted], default=0), first_branch_h=min(heights) if heights else np.nan)
    return col, order, branch


def branch_structure(xyz, lab, px, py, z_ref, offset=None, **cfg):
    """xyz f64 [N, 3], lab i64 [N], px, py, z_ref f64 [T] (T >= max(lab)).  Returns BRANCH_COLUMNS ([T] each), "skeleton" (SKELETON_KEYS),
    "keys" i64 [U] and "d" i32 [U] (every tree's voxels in (tree, ix, iy, iz) order under the key packing of include/treelearn_hip.h, and
    their distance) and "margins"."""
    unknown = set(cfg) - set(BRANCH_DEFAULTS)
    assert not unknown, unknown
    cfg = dict(BRANCH_DEFAULTS, **cfg)
    xyz, lab = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(lab, np.int64).reshape(-1)
    T, vs = len(px), np.float64(cfg["voxel"])
    out = {k: (np.zeros(T, np.int64) if k in BRANCH_INT else np.full(T, np.nan)) for k in BRANCH_COLUMNS}
    margins = {k: np.inf for k in MARGIN_KINDS}
    sk = dict(node_start=np.zeros(T + 1, np.int64), xyz=[], parent=[], bin=[], count=[], order=[], branch=[])
    keys, dist = [], []
    for t in range(T):
        sk["node_start"][t + 1] = sk["node_start"][t]
        rows = xyz[lab == t + 1]
        if len(rows) == 0:
            continue
        if not np.isfinite(rows).all():
            raise ValueError("a coordinate of a tree is not finite")
        anchor = np.array([px[t], py[t], z_ref[t]], np.float64)
        if not np.isfinite(anchor).all():
            continue
        q = anchor / vs
        base = np.floor(q)
        gap = np.minimum(q - base, base + 1.0 - q)
        margins["voxel"], margins["z_ref"] = min(margins["voxel"], float(gap[:2].min())), min(margins["z_ref"], float(gap[2]))
        ipx, ipy, izr = (int(v) for v in base)
        idx = np.floor(rows / vs).astype(np.int64)
        idx = idx[idx[:, 2] >= izr]
        if len(idx) and (np.abs(idx[:, 0] - ipx).max() > 2047 or np.abs(idx[:, 1] - ipy).max() > 2047 or (idx[:, 2] - izr).max() >= Z_MAX):
            raise ValueError("a row lies beyond the voxel key of its tree")
        vox = set(map(tuple, idx.tolist()))
        out["skel_voxels"][t] = len(vox)
        order_v = sorted(vox)
        keys += [(t << 35) | ((v[0] - ipx + HALF) << 23) | ((v[1] - ipy + HALF) << 11) | (v[2] - izr) for v in order_v]
        d = geodesic(vox, (ipx, ipy), cfg) if len(vox) <= cfg["max_voxels"] else None
        dist += [(-1 if d is None else d.get(v, -1)) for v in order_v]
        if d is None:
            continue
        nodes = nodes_of(d, cfg)
        cen = np.array([[(np.float64(sum(v[k] for v in nd["voxels"])) / np.float64(len(nd["voxels"])) + 0.5) * vs for k in range(3)] for nd in nodes],
                       np.float64).reshape(-1, 3)
        parent = [nd["parent"] for nd in nodes]
        col, order, branch = branches_of(cen, parent, float(z_ref[t]), cfg, margins)
        for k, v in col.items():
            out[k][t] = v
        out["skel_reached"][t], out["skel_nodes"][t] = len(d), len(nodes)
        sk["node_start"][t + 1] += len(nodes)
        sk["xyz"].append(cen); sk["parent"] += parent; sk["order"] += order; sk["branch"] += branch
        sk["bin"] += [nd["bin"] for nd in nodes]; sk["count"] += [len(nd["voxels"]) for nd in nodes]
    sk["xyz"] = np.concatenate(sk["xyz"]) if sk["xyz"] else np.zeros((0, 3), np.float64)
    if offset is not None:
        sk["xyz"] = sk["xyz"] + np.asarray(offset, np.float64).reshape(1, 3)
    for k in ("parent", "bin", "order", "branch"):
        sk[k] = np.asarray(sk[k], np.int32).reshape(-1)
    sk["count"] = np.asarray(sk["count"], np.int64).reshape(-1)
    out["skeleton"] = {k: sk[k] for k in SKELETON_KEYS}
    out["keys"], out["d"] = np.asarray(keys, np.int64).reshape(-1), np.asarray(dist, np.int32).reshape(-1)
    out["margins"] = margins
    return out


def tree_branches(coords, labels, terrain=None, offset=None, branch_cfg=None, **inventory_params):
    """The inventory of the restatements (with the ground columns with a terrain: a terrain_restatement.terrain_model dict in the frame of
    coords) followed by BRANCH_COLUMNS, "skeleton", "keys", "d" and "margins"; z_ref = z_ground with a terrain, z_low without."""
    import inventory_restatement as inv_ref
    if terrain is None:
        base = inv_ref.tree_inventory(coords, labels, **inventory_params)
        z_ref = base["z_low"]
        full = base if offset is None else inv_ref.tree_inventory(coords, labels, offset=offset, **inventory_params)
    else:
        import terrain_restatement as ter_ref
        base = ter_ref.tree_inventory(coords, labels, terrain, **inventory_params)
        z_ref = base["z_ground"]
        full = base if offset is None else ter_ref.tree_inventory(coords, labels, terrain, offset=offset, **inventory_params)
    br = branch_structure(coords, labels, base["x"], base["y"], z_ref, offset=offset, **(branch_cfg or {}))
    if terrain is None:
        br["margins"]["z_ref"] = np.inf
    res = dict(full)
    res.update(br)
    return res
