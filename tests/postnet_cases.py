"""Seeded inputs for the post-network stages (k-NN vote, group mean / ensemble, eps-grouping), shared by test_host_postnet.py and
test_gpu_postnet.py.  Every case is small enough for the O(n^2) restatements of postnet_restatement.py (k-NN: nr * nq <= 1e7,
grouping: n <= 4000); the one n = 524 289 group-mean case is a single pass.  All arrays are returned read-only.

The shapes sit at the launch edges of the kernels: the 256-row LDS tile and 256-thread block of k_knn_vote, its k templates 1, 3, 5
against the 8-wide default, the 8-column chunk and the 2048-row scan tile of k_group_mean."""
import functools

import numpy as np

H_MIN = np.float32(0.05)          # smallest cell edge of the k-NN grid (util/postprocess.knn_vote)
RING_MARGIN = 0.999               # k_knn_vote_grid stops after ring r once the k-th best distance is below RING_MARGIN * r * h
MAX_OUTSIDE_CELLS = 4096          # furthest an outside-the-box query is placed, in cells


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ============================================================================================ k-NN
def grid_edge(ref):
    """The cell edge util/postprocess.knn_vote chooses for a reference set (its first two terms: the third only matters for boxes
    longer than 50 km)."""
    ref = np.asarray(ref, dtype=np.float32)
    ext = np.maximum((ref.max(0) - ref.min(0)).astype(np.float64), 1e-3)
    return np.float32(max(0.05, float((ext.prod() * 8.0 / len(ref)) ** (1.0 / 3.0))))


def _knn(name, ref, lab, qry, k, tie_free=True, sklearn=True):
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3); qry = np.asarray(qry, dtype=np.float32).reshape(-1, 3)
    lab = np.asarray(lab, dtype=np.int64)
    assert len(ref) == len(lab) and len(ref) * len(qry) <= 10_000_000, name
    return dict(id=name, ref=_ro(ref), lab=_ro(lab), qry=_ro(qry), k=int(k), tie_free=bool(tie_free), sklearn=bool(sklearn))


NR = (1, 5, 255, 256, 257, 513)
NQ = (1, 255, 256, 257)
K_OF_NR = {1: 1, 5: 5, 255: 3, 256: 8, 257: 1, 513: 5}


def _cell32(x, lo, inv_h):
    """floorf((x - lo) * inv_h) in float32: the binning the ring bound was written for."""
    return np.floor((np.asarray(x, dtype=np.float32) - np.float32(lo)) * np.float32(inv_h)).astype(np.int64)


def ring_bound_points(lo, window=(1.0, 1.5)):
    """(q, p, p2, c, h): over every float32 x in the window, with the anchor at `lo` and the 5 cm cell, a cell c for which
    min{x : cell(x) = c + 2} - max{x : cell(x) = c} < RING_MARGIN * h in float32 binning; q is that maximum, p that minimum and
    p2 = q - d with |p - q| < d < RING_MARGIN * h.  The preconditions are asserted here, so the case can never be a harmless one."""
    h = H_MIN; inv_h = np.float32(1.0) / h
    a, b = np.float32(window[0]).view(np.int32), np.float32(window[1]).view(np.int32)
    x = np.arange(a, b, dtype=np.int32).view(np.float32)              # every float32 in [window[0], window[1]), ascending
    cell = _cell32(x, lo, inv_h)
    assert (np.diff(cell) >= 0).all()                                 # the binning is monotone
    cells, first = np.unique(cell, return_index=True)
    last = np.concatenate([first[1:], [len(x)]]) - 1
    hd = float(h)
    for i in range(1, len(cells) - 3):
        if cells[i + 2] != cells[i] + 2:
            continue
        q, p = x[last[i]], x[first[i + 2]]
        gap = float(p) - float(q)
        if not gap < (RING_MARGIN - 1e-4) * hd:
            continue
        d = 0.5 * (gap + RING_MARGIN * hd)
        p2 = np.float32(float(q) - d)
        c = int(cells[i])
        # preconditions, in the float32 arithmetic of the binning and the float64 arithmetic of the distances
        assert int(_cell32(q, lo, inv_h)) == c and int(_cell32(p, lo, inv_h)) == c + 2
        assert int(_cell32(p2, lo, inv_h)) in (c - 1, c)
        assert gap < float(q) - float(p2) < RING_MARGIN * hd
        return q, p, p2, c, h
    raise AssertionError(f"no cell with a gap below {RING_MARGIN} h in the window for lo = {lo}")


def _ring_case(axis, lo):
    """ref = [anchor ..., p2, p] along one axis, query q, k = 1: the nearest point is p.  The anchor at `lo` fixes the box; it is
    repeated until the wrapper's eight-points-per-cell rule (box volume with the 1 mm clamp on the two flat axes) keeps the 5 cm cell."""
    q, p, p2, _, _ = ring_bound_points(lo)
    m = int(np.ceil((abs(lo) + 2.0) * 1e-6 * 8.0 / float(H_MIN) ** 3)) + 8
    ref = np.zeros((m + 2, 3), dtype=np.float32); qry = np.zeros((1, 3), dtype=np.float32)
    ref[:m, axis] = lo; ref[m, axis] = p2; ref[m + 1, axis] = p; qry[0, axis] = q
    assert grid_edge(ref) == H_MIN                                     # the wrapper keeps the 5 cm cell for this box
    return _knn(f"ring-axis{axis}-lo{int(lo)}", ref, [7] * m + [5, 3], qry, 1, tie_free=True, sklearn=False)


def ring_bound_cases():
    return [_ring_case(0, -5000.0), _ring_case(1, -5000.0), _ring_case(2, -5000.0), _ring_case(0, -50000.0)]


def _outside_case(rng):
    """600 reference points in a 20 cm cube (5 cm cells, 4 per axis); queries 1, 100 and 4000 cells outside each of the six faces
    and outside one corner."""
    ref = rng.uniform(0.0, 0.2, size=(600, 3)).astype(np.float32)
    h = float(grid_edge(ref))
    assert h == float(H_MIN)
    qs = []
    for cells in (1, 100, 4000):
        assert cells <= MAX_OUTSIDE_CELLS
        for axis in range(3):
            for side in (-1, 1):
                q = rng.uniform(0.0, 0.2, size=3)
                q[axis] = (0.2 + cells * h) if side > 0 else -cells * h
                qs.append(q)
        qs.append(np.full(3, 0.2 + cells * h)); qs.append(np.full(3, -cells * h))
    qry = np.asarray(qs, dtype=np.float32)
    lo = ref.min(0)
    assert np.abs(np.floor((qry - lo) / np.float32(h))).max() <= MAX_OUTSIDE_CELLS
    return ref, qry


@functools.lru_cache(maxsize=None)
def knn_cases():
    rng = np.random.default_rng(20240)
    out = []
    uni = lambda n, s=4.0: rng.uniform(-s, s, size=(n, 3)).astype(np.float32)          # noqa: E731
    labs = lambda n, hi=7: rng.integers(0, hi, size=n)                                  # noqa: E731
    # --- shapes: the 256-row LDS tile x the 256-thread block
    for nr in NR:
        for nq in NQ:
            out.append(_knn(f"shape-nr{nr}-nq{nq}", uni(nr), labs(nr), uni(nq, 4.5), K_OF_NR[nr]))
    # --- every k, with nr == k and with nr = 300 (1, 3, 5: own templates; 2, 4, 6, 7, 8: the 8-wide one)
    for k in range(1, 9):
        out.append(_knn(f"k{k}-nr-equals-k", uni(k), labs(k, 3), uni(33), k))
        out.append(_knn(f"k{k}-nr300", uni(300), labs(300, 4), uni(300), k))
    # --- data
    base = uni(200)
    for k in (3, 4, 5):
        out.append(_knn(f"triplicate-k{k}", np.concatenate([base, base, base]), np.repeat([4, 2, 9], 200), uni(257), k, tie_free=(k == 3)))      # k = 3: exactly the three copies of the nearest point
    g = (np.arange(8) * 0.1).astype(np.float32)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    mid = ((g[:-1] + g[1:]) * np.float32(0.5)).astype(np.float32)
    latq = np.concatenate([lat[rng.permutation(len(lat))[:150]], np.stack(np.meshgrid(mid, mid, mid, indexing="ij"), -1).reshape(-1, 3)[:150],
                           np.stack([g, g, g], 1)])
    for k in (1, 5, 6):
        out.append(_knn(f"lattice-k{k}", lat, labs(len(lat), 5), latq, k, tie_free=False))
    for k in (2, 4, 6):
        out.append(_knn(f"two-labels-k{k}", uni(400), rng.choice([3, 7], size=400), uni(300), k))
    out.append(_knn("negative-labels-k4", uni(400), rng.choice([-5, -1, 0, 2], size=400), uni(300), 4))
    out.append(_knn("negative-labels-k2", uni(400), rng.choice([-5, -1, -3], size=400), uni(300), 2))
    r = uni(513)
    for k in (1, 3):
        out.append(_knn(f"queries-are-references-k{k}", r, labs(513), r[:300], k))
    one = np.tile(np.array([[1.25, -2.5, 0.75]], dtype=np.float32), (300, 1))
    for k in (1, 5, 8):
        out.append(_knn(f"all-identical-k{k}", one, labs(300, 4), np.concatenate([one[:1], uni(40)]), k, tie_free=False))
    t = rng.uniform(-3, 3, size=500).astype(np.float32)
    out.append(_knn("line-k3", np.stack([t, np.float32(2) * t, -t], 1), labs(500), uni(200), 3))
    pl = uni(500); pl[:, 2] = 1.5
    out.append(_knn("plane-k5", pl, labs(500), uni(200), 5))
    shift = np.array([431000.0, 5520000.0, 300.0])
    out.append(_knn("shifted-k5", (rng.uniform(-10, 10, size=(600, 3)) + shift).astype(np.float32), labs(600),
                    (rng.uniform(-11, 11, size=(300, 3)) + shift).astype(np.float32), 5))
    oref, oqry = _outside_case(rng)
    for k in (1, 5):
        out.append(_knn(f"outside-k{k}", oref, labs(600), oqry, k))
    out.extend(ring_bound_cases())
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


# ============================================================================================ group mean
GM_C = (1, 7, 8, 9, 42)
GM_N = (1, 2047, 2048, 2049, 4097)
GM_BIG_N = 524_289                # 257 scan tiles: more partials than one wave holds, one workgroup scans them
SCAN_TILE = 2048


def _mixed(rng, shape):
    return (rng.normal(size=shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(np.float32)


def _runs_to_groups(run_lengths):
    return np.repeat(np.arange(len(run_lengths), dtype=np.int64), run_lengths)


def _group_ids(rng, n, structure):
    """Group number of every sorted row."""
    if structure == "singletons":
        return np.arange(n, dtype=np.int64)
    if structure == "one-group":
        return np.zeros(n, dtype=np.int64)
    if structure == "runs-1-5":
        runs = rng.integers(1, 6, size=n)
        return _runs_to_groups(runs)[:n]
    assert structure == "straddle" and n > SCAN_TILE                   # a run that starts on the last row of a scan tile
    runs, at = [], 0
    while at < n:
        edge = (at // SCAN_TILE + 1) * SCAN_TILE - 1                   # last row of the tile `at` is in
        if at == edge and at + 1 < n:
            length = min(3, n - at)                                    # ... and ends in the next tile
        else:
            length = min(int(rng.integers(1, 4)), max(edge - at, 1), n - at)
        runs.append(length); at += length
    g = _runs_to_groups(runs)
    for edge in range(SCAN_TILE - 1, n - 1, SCAN_TILE):
        assert g[edge] != g[edge - 1] and g[edge] == g[edge + 1]
    return g


def _gm(name, rng, src, g_sorted):
    """Rows are scattered: row perm[s] of src belongs to the group of sorted position s; within a group perm ascends (stable sort)."""
    n = len(g_sorted)
    scatter = rng.permutation(n)
    g_row = np.empty(n, dtype=np.int64); g_row[scatter] = g_sorted
    perm = np.argsort(g_row, kind="stable").astype(np.int64)
    keys = g_row[perm] * 3 + 5                                         # any ascending int64 keys
    assert (np.diff(keys) >= 0).all()
    return dict(id=name, src=_ro(src), keys=_ro(keys), perm=_ro(perm))


def run_length_case(rng):
    """A run of every length 1..100 (49 and 98 among them); every row of a run carries the same integer label from 0..3000 in columns
    0 and 2, column 1 is a float."""
    lengths = rng.permutation(np.arange(1, 101))
    g = _runs_to_groups(lengths)
    label = rng.integers(0, 3001, size=(100, 2))
    label[lengths == 49] = (7, 2999); label[lengths == 98] = (12, 1)   # labels the reciprocal form gets wrong at 49 rows
    src = np.empty((len(g), 3), dtype=np.float32)
    src[:, 0] = label[g, 0]; src[:, 2] = label[g, 1]; src[:, 1] = _mixed(rng, len(g))
    return _gm("runs-1-100-constant-labels", rng, src, g)


@functools.lru_cache(maxsize=None)
def group_mean_cases():
    rng = np.random.default_rng(4711)
    out = []
    structures = ("singletons", "one-group", "runs-1-5", "straddle")
    i = 0
    for C in GM_C:
        for n in GM_N:
            s = structures[i % 4]; i += 1
            if s == "straddle" and n <= SCAN_TILE:
                s = "runs-1-5"
            out.append(_gm(f"C{C}-n{n}-{s}", rng, _mixed(rng, (n, C)), _group_ids(rng, n, s)))
    for s, n, C in (("straddle", 2049, 9), ("straddle", 4097, 8), ("one-group", 2049, 7), ("singletons", 4097, 42), ("one-group", 1, 9)):
        out.append(_gm(f"C{C}-n{n}-{s}-extra", rng, _mixed(rng, (n, C)), _group_ids(rng, n, s)))
    out.append(run_length_case(rng))
    out.append(_gm(f"C1-n{GM_BIG_N}-runs-1-5", rng, _mixed(rng, (GM_BIG_N, 1)), _group_ids(rng, GM_BIG_N, "runs-1-5")))
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)


# ============================================================================================ ensemble
ENSEMBLE_KEYS = ("coords", "semantic_scores", "semantic_labels", "offset_predictions", "offset_labels", "instance_labels", "feats", "input_feats")


def _ensemble(name, rng, cm, counts, f_in, mixed=False):
    """cm: integer centimetre coordinates [G, 3] (distinct rows); group i has counts[i] members, each within 4 mm of its centimetre on
    either side, with constant integer labels per group; rows shuffled."""
    G = len(cm)
    g = np.repeat(np.arange(G), counts)
    n = len(g)
    coords = (cm[g] / 100.0 + rng.uniform(-0.004, 0.004, size=(n, 3))).astype(np.float32)
    assert (np.rint(coords * np.float32(100.0)).astype(np.int64) == cm[g]).all()      # both sides round to the group's centimetre
    sem_l = rng.integers(0, 2, size=G)[g]; inst_l = rng.integers(0, 3001, size=G)[g]
    # float columns: multiples of 2^-10 below 8, so that a group's sum is exact in float32 as well (pandas adds float32 columns in
    # float32): its mean and the float64 mean then differ by the rounding of the division alone, the one float32 ulp the host test allows.
    # mixed=True: random float32 of mixed magnitude instead, where the order and the precision of the sum show; pandas' float32 sums
    # are then several ulp off, so such a case is compared on the GPU only (`pandas` False)
    pos = lambda w: (rng.integers(-8191, 8192, size=(n, w)) / 1024.0).astype(np.float32)                         # noqa: E731
    if mixed:
        pos = lambda w: _mixed(rng, (n, w))                                                                      # noqa: E731
    d = dict(coords=coords, semantic_scores=pos(2), semantic_labels=sem_l.astype(np.int64), offset_predictions=pos(3),
             offset_labels=pos(3), instance_labels=inst_l.astype(np.int64), feats=pos(32), input_feats=pos(f_in))
    p = rng.permutation(n)
    return dict(id=name, n_groups=G, pandas=not mixed, **{k: _ro(v[p]) for k, v in d.items()})


@functools.lru_cache(maxsize=None)
def ensemble_cases():
    rng = np.random.default_rng(99)
    def cms(G, lo, hi):
        while True:
            cm = np.unique(rng.integers(lo, hi, size=(2 * G, 3)), axis=0)
            if len(cm) >= G:
                return cm[rng.permutation(len(cm))[:G]]
    out = [_ensemble("counts-1-100-f1", rng, cms(100, -3000, 3000), rng.permutation(np.arange(1, 101)), 1),
           _ensemble("counts-1-100-f4", rng, cms(100, -3000, 3000), rng.permutation(np.arange(1, 101)), 4),
           _ensemble("negative-coords-f4", rng, cms(700, -2500, 0), rng.integers(1, 6, size=700), 4),
           _ensemble("around-zero-f1", rng, cms(300, -4, 5), rng.integers(1, 5, size=300), 1),
           _ensemble("single-row-f1", rng, cms(1, -10, 10), np.array([1]), 1),
           _ensemble("49-rows-f4", rng, cms(40, -500, 500), np.full(40, 49), 4),
           _ensemble("mixed-magnitude-counts-1-100-f4", rng, cms(100, -3000, 3000), rng.permutation(np.arange(1, 101)), 4, mixed=True)]
    return tuple(out)


# ============================================================================================ DBSCAN(eps, min_samples = 2)
def _db(name, xy, eps):
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    assert len(xy) <= 4000, name
    return dict(id=name, xy=_ro(xy), eps=float(eps))


@functools.lru_cache(maxsize=None)
def dbscan_cases():
    rng = np.random.default_rng(31337)
    out = []
    three = np.array([[0.0, 0.0], [0.1, 0.0], [3.0, 3.0]], dtype=np.float32)
    for n in (1, 2, 3):
        out.append(_db(f"n{n}", three[:n], 0.15))
    out.append(_db("two-far", three[[0, 2]], 0.15))
    out.append(_db("all-identical", np.tile(np.array([[2.5, -1.25]], dtype=np.float32), (300, 1)), 0.15))
    g = (np.arange(-6, 7) * 0.25).astype(np.float32)                  # exact in float32; both sides of 0
    lat = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    out.append(_db("lattice-pitch-equals-eps", lat[rng.permutation(len(lat))], 0.25))            # d == eps joins (<=)
    out.append(_db("lattice-pitch-equals-eps-with-holes", lat[rng.permutation(len(lat))[:110]], 0.25))
    pitch = np.nextafter(np.float32(0.25), np.float32(1))
    g2 = (np.array([-2, -1, 0, 1, 2], dtype=np.float32) * pitch).astype(np.float32)
    assert (np.diff(g2.astype(np.float64)) == float(pitch)).all()      # multiples 0, 1, 2 of the pitch are exact in float32
    out.append(_db("lattice-pitch-one-ulp-above-eps", np.stack(np.meshgrid(g2, g2, indexing="ij"), -1).reshape(-1, 2), 0.25))
    out.append(_db("both-sides-of-zero", rng.uniform(-1, 1, size=(1500, 2)), 0.05))
    near = np.array([[1e5, -1e5]]) + rng.uniform(-3, 3, size=(1500, 2))
    out.append(_db("near-1e5", near, 0.15))
    out.append(_db("near-minus-1e5", -near, 0.15))
    chain = np.stack([np.arange(3000) * (0.9 * 0.15) - 200.0, np.full(3000, 0.3)], 1)
    out.append(_db("chain-3000", chain[rng.permutation(3000)], 0.15))
    out.append(_db("chain-3000-in-order", chain, 0.15))
    out.append(_db("scattered-4000", rng.uniform(-50, 50, size=(4000, 2)), 0.15))
    c = rng.uniform(-8, 8, size=(60, 2))
    clumps = c[rng.integers(0, 60, 1000)] + rng.normal(size=(1000, 2)) * 0.05
    out.append(_db("eps015-clumps", np.concatenate([clumps, rng.uniform(-8, 8, size=(2000, 2))])[rng.permutation(3000)], 0.15))
    assert len({c["id"] for c in out}) == len(out)
    return tuple(out)
