"""Two epochs of one plot, restated in numpy float64.  This file is the specification of csrc/tl_change.hip and
treelearn_amd/util/change.py; it imports nothing from the package and finds neighbours by brute force.

  moved query   x'_a = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3], f32 input widened first, every operation rounded on its own
  cross_nn      per query the reference row of smallest d2 = (dx*dx + dy*dy) + dz*dz among those with d2 < max_dist * max_dist (strict);
                equal d2: the smaller row (np.argmin over the original order); none, or a moved query that is not finite: -1 / +inf
  rigid sums    17 values per row (1, a, b, a b^T row-major, d2 with a = x' - c, b = ref[nn] - c; +0.0 for a row that does not take
                part), summed by the halving tree over chunks of 2048 rows, then by the same tree over the chunk partials
  ICP           H = S - s_a s_b^T / m; rotation from the SVD of H (dof 6, reflection guard) or the yaw atan2(H01 - H10, H00 + H11)
                (dof 4); translation b_mean - R a_mean carried back from the centred frame; T <- dT . T
  matching      nearest neighbours in both directions, two tables, score = (both counts) / (n_r + n_m), Hungarian assignment"""
import numpy as np

CHUNK = 2048
TERMS = 17
MIN_PAIRS = {4: 3, 6: 6}


def move(T, q):
    q = np.asarray(q)[:, :3].astype(np.float64)
    T = np.eye(4)[:3] if T is None else np.asarray(T, np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)


def cross_nn(ref, q, T=None, max_dist=1.0, block=256):
    """(nn i64[nq], d2 f64[nq]) by brute force."""
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        p = move(T, q)
    nq = len(p)
    nn = np.full(nq, -1, np.int64); d2 = np.full(nq, np.inf)
    if len(ref) == 0:
        return nn, d2
    r2 = np.float64(max_dist) * np.float64(max_dist)
    for a in range(0, nq, block):
        pb = p[a:a + block]
        with np.errstate(all="ignore"):
            dx = ref[None, :, 0] - pb[:, None, 0]; dy = ref[None, :, 1] - pb[:, None, 1]; dz = ref[None, :, 2] - pb[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
        d = np.where(d < r2, d, np.inf)                                   # NaN (a moved query that is not finite) fails the comparison
        j = np.argmin(d, 1)                                               # the first of equal minima: the smaller row
        best = d[np.arange(len(pb)), j]
        ok = np.isfinite(pb).all(1) & (best < np.inf)
        nn[a:a + block] = np.where(ok, j, -1); d2[a:a + block] = np.where(ok, best, np.inf)
    return nn, d2


def rigid_terms(ref, q, T, nn, d2, c, reject2):
    """f64[nq, 17]: what every row contributes."""
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    p = move(T, q)
    c = np.asarray(c, np.float64)
    take = (nn >= 0) & (nn < len(ref)) & (d2 < reject2)
    out = np.zeros((len(p), TERMS))
    a = p[take] - c
    b = ref[nn[take]] - c
    out[take, 0] = 1.0
    out[take, 1:4] = a
    out[take, 4:7] = b
    out[take, 7:16] = (a[:, :, None] * b[:, None, :]).reshape(-1, 9)
    out[take, 16] = d2[take]
    return out


def tree_sum(v):
    """The documented tree over the rows of v [n, k]: chunks of 2048, s[i] += s[i + stride] for stride 1024 .. 1 with missing rows at +0.0,
    then the same over the chunk partials until one is left."""
    v = np.asarray(v, np.float64)
    while True:
        n, k = v.shape
        nch = max(1, -(-n // CHUNK))
        s = np.zeros((nch * CHUNK, k)); s[:n] = v
        s = s.reshape(nch, CHUNK, k)
        stride = CHUNK // 2
        while stride:
            s[:, :stride] += s[:, stride:2 * stride]
            stride //= 2
        v = s[:, 0].copy()
        if nch == 1:
            return v[0]


def rigid_sums(ref, q, T, nn, d2, c, reject2):
    return tree_sum(rigid_terms(ref, q, T, nn, d2, c, reject2))


def parse_init(init):
    if init is None:
        return np.eye(4)
    a = np.asarray(init, np.float64)
    if a.shape == (4, 4):
        return a.copy()
    dx, dy, dz, yaw = a.reshape(4)
    th = np.deg2rad(yaw)
    T = np.eye(4)
    T[0, 0] = np.cos(th); T[0, 1] = -np.sin(th); T[1, 0] = np.sin(th); T[1, 1] = np.cos(th)
    T[:3, 3] = (dx, dy, dz)
    return T


def solve(sums, c, dof):
    """(dT 4x4, angle, shift) of one step from the 17 sums."""
    sums = np.asarray(sums, np.float64); c = np.asarray(c, np.float64)
    m = sums[0]
    sa, sb, S = sums[1:4], sums[4:7], sums[7:16].reshape(3, 3)
    H = S - np.outer(sa, sb) / m
    if dof == 6:
        U, _, Vt = np.linalg.svd(H)
        R = Vt.T @ U.T
        if np.linalg.det(R) < 0:
            Vt = Vt.copy(); Vt[2] = -Vt[2]
            R = Vt.T @ U.T
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        angle = float(np.arctan2(0.5 * np.sqrt(w @ w), 0.5 * (np.trace(R) - 1.0)))
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


def register(ref, moving, dof=6, max_dist=1.0, reject_min=0.1, max_iters=50, tol_angle=1e-7, tol_shift=1e-6, init=None):
    ref = np.asarray(ref)[:, :3].astype(np.float64)
    if not (np.isfinite(ref).all() and np.isfinite(np.asarray(moving)[:, :3]).all()):
        raise ValueError("a coordinate is not finite")
    T = parse_init(init)
    c = (ref.min(0) + ref.max(0)) * 0.5
    reject = float(max_dist)
    log, converged = [], False
    for _ in range(max_iters):
        nn, d2 = cross_nn(ref, moving, T[:3], max_dist)
        sums = rigid_sums(ref, moving, T[:3], nn, d2, c, reject * reject)
        m = int(sums[0])
        if m < MIN_PAIRS[dof]:
            raise ValueError(f"{m} pairs within max_dist = {max_dist}")
        dT, angle, shift = solve(sums, c, dof)
        T = dT @ T
        rms = float(np.sqrt(sums[16] / sums[0]))
        log.append(dict(pairs=m, rms=rms, reject=reject, angle=angle, shift=shift))
        reject = max(float(reject_min), 3.0 * rms)
        if angle < tol_angle and shift < tol_shift:
            converged = True
            break
    return dict(T=T, iterations=log, converged=converged, inlier_share=log[-1]["pairs"] / max(1, len(moving)))


def invert(T):
    T = np.asarray(T, np.float64)
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return Ti


def match_trees(ref_xyz, ref_labels, mov_xyz, mov_labels, T, match_dist=0.2, min_overlap=0.3):
    """Trees are the labels 1 .. max(label) that have rows; label 0 and negative labels are not trees."""
    from scipy.optimize import linear_sum_assignment
    rl = np.asarray(ref_labels).astype(np.int64).reshape(-1); ml = np.asarray(mov_labels).astype(np.int64).reshape(-1)
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    nn_m, _ = cross_nn(ref_xyz, mov_xyz, T[:3], match_dist)              # per moving row: a reference row
    nn_r, _ = cross_nn(mov_xyz, ref_xyz, invert(T)[:3], match_dist)      # per reference row: a moving row
    Tr, Tm = max(int(rl.max(initial=0)), 0), max(int(ml.max(initial=0)), 0)
    nb_m = np.where(nn_m >= 0, rl[np.clip(nn_m, 0, None)] if len(rl) else -1, -1)
    nb_r = np.where(nn_r >= 0, ml[np.clip(nn_r, 0, None)] if len(ml) else -1, -1)
    A = np.zeros((Tm + 1, Tr + 1), np.int64); B = np.zeros((Tr + 1, Tm + 1), np.int64)
    k = (ml > 0) & (nb_m > 0)
    np.add.at(A, (ml[k], nb_m[k]), 1)                                     # rows of m whose neighbour is in r
    k = (rl > 0) & (nb_r > 0)
    np.add.at(B, (rl[k], nb_r[k]), 1)                                     # rows of r whose neighbour is in m
    n_r = np.bincount(rl[rl > 0], minlength=Tr + 1); n_m = np.bincount(ml[ml > 0], minlength=Tm + 1)
    gained = np.bincount(ml[(ml > 0) & (nn_m < 0)], minlength=Tm + 1)[1:].astype(np.int64)
    lost = np.bincount(rl[(rl > 0) & (nn_r < 0)], minlength=Tr + 1)[1:].astype(np.int64)
    den = (n_r[1:, None] + n_m[None, 1:]).astype(np.float64)
    score = np.where(den > 0, (A[1:, 1:].T + B[1:, 1:]) / np.maximum(den, 1.0), 0.0)        # [Tr, Tm]
    pairs = []
    if Tr and Tm:
        rows, cols = linear_sum_assignment(score, maximize=True)
        pairs = [(int(r) + 1, int(m) + 1, float(score[r, m])) for r, m in zip(rows, cols)
                 if n_r[r + 1] > 0 and n_m[m + 1] > 0 and score[r, m] >= min_overlap]
    mr, mm = {p[0] for p in pairs}, {p[1] for p in pairs}
    return dict(pairs=pairs, unmatched_ref=[t for t in range(1, Tr + 1) if n_r[t] > 0 and t not in mr],
                unmatched_mov=[t for t in range(1, Tm + 1) if n_m[t] > 0 and t not in mm], lost_points=lost, gained_points=gained,
                n_ref=n_r[1:].astype(np.int64), n_mov=n_m[1:].astype(np.int64))
