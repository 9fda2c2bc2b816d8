"""Inputs for which the INPUT gradient of the sparse convs has one right answer, real rulebooks to run it over, the float64 reference, a
restatement of what treelearn_amd/backward.py launches, and the case list of tests/test_host_dgrad.py and tests/test_gpu_dgrad_exact.py.
Plain numpy; of the package only `oracle` is imported.

    forward   y[o]            = sum_k W[:, k, :] x[table[o, k]]            (table[o, k] = input row of tap k, -1 = absent)
    reference gx[table[o, k]] += gout[o] @ W[:, k, :]                      (W = the parameter [Cout, k, k, k, Cin] read as [Cout, K, Cin])

The reference is the scatter form over the FORWARD table with the parameter in its own layout; it knows nothing of the transposed
table, the flipped taps or the [K][Cin][Cout] layout that backward.py relies on.  `transposed_path` restates backward.py: a gather over
`t_table` with W[k]^T, taps flipped for SubM, in column slices of `step`, each written into a column view of one buffer.

Geometries are real voxel sets (unique cells of a box at roughly 30 % occupancy, some with two batch items): `nbr` from
oracle.voxel.rulebook_subm, `child` / `parent` from oracle.voxel.rulebook_down, `inv[k][i] = parent[i]` where tap(i) == k.  SubM's backward
is only right on a symmetric table, so random tables would test nothing.  The row count on the side that RECEIVES the gradient takes the
values of ROWS of tests/test_gpu_conv_epilogue.py: 1, 31, 33 (partial 32-row block), 257 (partial wave / 256-row workgroup), 513
(partial 512-row workgroup).  Asserted here for every geometry:  nbr[o][k] == i  <=>  nbr[i][K-1-k] == o;  inv has exactly one valid
entry per fine row that has a parent and none for the others;  child / inv are transposes of each other.

Set A (dyadic; wgrad_cases.dyadic): every element of gout and of W is m / 8, |m| <= 8 -- exact in bf16, f16 and fp32.  Every product is a
multiple of 1/64 of magnitude <= 1.  An entry of gx sums at most 27 taps x 448 output channels = 12 096 of them: a multiple of 1/64 of
magnitude < 2^14, under 20 significant bits, so every partial sum in any order and any grouping is exact in fp32.  A kernel that
accumulates in fp32 and rounds once must therefore return round_to(reference, dtype) with no difference at all, in fp32, bf16 and f16
(|gx| < 2^14 is far inside f16's range).

Set B (gaussian): values rounded to the dtype, weights scaled by 1 / sqrt(0.6 K Cout); compared with float64 under TOL of
tests/test_gpu_conv_epilogue.py.  Catches a wrong scale or a lost low-order contribution that small integers could mask.
"""
import numpy as np

from oracle import voxel as ov
from wgrad_cases import dyadic, round_to

ROWS = (1, 31, 33, 257, 513)                     # = ROWS of tests/test_gpu_conv_epilogue.py (asserted in tests/test_host_dgrad.py)
DTYPES = ("f32", "bf16", "f16")
PRE_MARGIN = 1e-3                                # no BatchNorm pre-activation of a case lies this close to zero


# ------------------------------------------------------------------------------------------------------------------------ geometries
def _cells(rng, n, batches, odd=False):
    """n unique cells (b, x, y, z) of a box at ~30 % occupancy, ascending key, and the box.  `odd`: odd extents, so the cells of the last
    planes have no parent; the last row is then a lone cell in a plane of its own that HAS a parent (a row left out at the end of a
    partial block must not be one whose gradient is zero anyway)."""
    side = max(2, int(np.ceil((n / 0.3 / batches) ** (1 / 3))))
    if odd:
        side |= 1
        n -= 1
    else:
        side += side & 1                          # even extents: every cell has a parent
    while batches * side ** 3 < n:
        side += 2
    pick = np.sort(rng.choice(batches * side ** 3, size=n, replace=False))
    b, r = np.divmod(pick, side ** 3)
    x, r = np.divmod(r, side * side)
    y, z = np.divmod(r, side)
    c = np.stack([b, x, y, z], axis=1).astype(np.int32)
    shape = np.array([side] * 3)
    if odd:
        c = np.concatenate([c, np.array([[batches - 1, side + 1, 0, 0]], np.int32)])
        shape[0] = side + 3
    return c[np.argsort(ov.pack_key(c), kind="stable")], shape


class Geometry:
    """fine level `coords` [n, 4] + the coarse level under it.  Oracle layout: nbr [n, 27], child [m, 8], parent [n]; kernel layout (taps
    first, as the library takes them): nbr_k [27, n], child_k [8, m], inv_k [8, n]."""

    def __init__(self, coords, shape):
        self.coords, self.shape = coords, shape
        self.n = len(coords)
        self.nbr = ov.rulebook_subm(coords)
        self.ccoords, self.parent, self.child, self.cshape = ov.rulebook_down(coords, shape)
        self.m = len(self.ccoords)
        c = coords.astype(np.int64)
        self.tap = ((c[:, 1] & 1) * 4 + (c[:, 2] & 1) * 2 + (c[:, 3] & 1)).astype(np.int64)
        inv = np.full((8, self.n), -1, np.int32)
        has = self.parent >= 0
        inv[self.tap[has], np.nonzero(has)[0]] = self.parent[has]
        self.inv_k = inv
        self.nbr_k = np.ascontiguousarray(self.nbr.T)
        self.child_k = np.ascontiguousarray(self.child.T)
        self._check()

    def _check(self):
        n, m, K = self.n, self.m, 27
        o, k = np.nonzero(self.nbr >= 0)
        i = self.nbr[o, k]
        assert np.array_equal(self.nbr[i, K - 1 - k], o), "nbr[o][k] == i  =>  nbr[i][K-1-k] == o"
        assert np.array_equal(self.nbr[:, 13], np.arange(n)), "the centre tap is the row itself"
        has = self.parent >= 0
        assert np.array_equal((self.inv_k >= 0).sum(0), has.astype(np.int64)), "inv: one valid entry per fine row with a parent, none otherwise"
        back = np.full((m, 8), -1, np.int32)
        kk, ii = np.nonzero(self.inv_k >= 0)
        back[self.inv_k[kk, ii], kk] = ii
        assert np.array_equal(back, self.child), "child / inv are transposes of each other"
        assert (self.child >= 0).sum() == has.sum() and ((self.child >= 0).sum(1) >= 1).all()


def _coarse_first(rng, m, batches):
    """a geometry with exactly m COARSE rows: m coarse cells, each with a random non-empty set of its eight children"""
    cc, side = _cells(rng, m, batches)
    keep = rng.uniform(size=(m, 8)) < 0.3
    keep[np.arange(m), rng.integers(0, 8, size=m)] = True
    q, t = np.nonzero(keep)
    f = cc[q].copy()
    f[:, 1] = 2 * f[:, 1] + (t >> 2); f[:, 2] = 2 * f[:, 2] + ((t >> 1) & 1); f[:, 3] = 2 * f[:, 3] + (t & 1)
    f = f[np.argsort(ov.pack_key(f), kind="stable")]
    return Geometry(f, 2 * side)


_GEOMS = {}


def geometry(name):
    """'fine<n>' / 'fine<n>b2' (n fine rows; b2: two batch items), 'coarse<m>' / 'coarse<m>b2' (m coarse rows), 'orphans' (513 fine rows in a box of odd
    extent: the fine rows of the last planes have no parent, and some coarse rows have one child only).  Built once, never changed."""
    if name not in _GEOMS:
        rng = np.random.default_rng(sum(name.encode()) * 7919)
        batches = 2 if name.endswith("b2") else 1
        base = name[:-2] if batches == 2 else name
        if base == "orphans":
            g = Geometry(*_cells(rng, 513, 1, odd=True))
            assert (g.parent < 0).any() and ((g.child >= 0).sum(1) == 1).any() and (g.parent >= 0).sum() > 100 and g.parent[-1] >= 0 and g.n == 513
        elif base.startswith("fine"):
            g = Geometry(*_cells(rng, int(base[4:]), batches))
            assert g.n == int(base[4:])
        else:
            g = _coarse_first(rng, int(base[6:]), batches)
            assert g.m == int(base[6:]) and (g.parent >= 0).all()
        if batches == 2:
            assert set(g.coords[:, 0]) == {0, 1}
        _GEOMS[name] = g
    return _GEOMS[name]


GEOMETRIES = ["fine1", "fine31", "fine33b2", "fine257", "fine513b2", "coarse1", "coarse31", "coarse33", "coarse257b2", "coarse513", "orphans"]


# ------------------------------------------------------------------------------------------------------------------------ layer kinds
def tables(kind, geom):
    """-> (table [n_out, K] of the FORWARD conv in the oracle's layout or None, n_out, t_table [K, n_in] that backward.py gathers over or
    None, n_in, flip, t_one_hot).  n_in rows receive the gradient.  kind: subm | 1x1 | linear | down | inverse."""
    if kind in ("1x1", "linear"):
        return None, geom.n, None, geom.n, False, False
    if kind == "subm":
        return geom.nbr, geom.n, geom.nbr_k, geom.n, True, False
    if kind == "down":                            # strided k2s2: coarse rows out, the gradient goes to the fine rows over inv
        return geom.child, geom.m, geom.inv_k, geom.n, False, True
    assert kind == "inverse"                      # inverse conv: fine rows out over inv, the gradient goes to the coarse rows over child
    return np.ascontiguousarray(geom.inv_k.T), geom.n, geom.child_k, geom.m, False, False


def taps(kind):
    return {"subm": 27, "down": 8, "inverse": 8, "1x1": 1, "linear": 1}[kind]


# -------------------------------------------------------------------------------------------------------------------------- reference
def reference(gout, weight, table, n_in):
    """float64 [n_in, Cin]: gx[table[o, k]] += gout[o] @ W[:, k, :] over the forward table (None: K = 1, every row with itself)."""
    co, ci = weight.shape[0], weight.shape[-1]
    W = np.asarray(weight, np.float64).reshape(co, -1, ci)
    g = np.asarray(gout, np.float64)
    gx = np.zeros((n_in, ci))
    if table is None:
        assert W.shape[1] == 1 and n_in == g.shape[0]
        return g @ W[:, 0, :]
    assert table.shape == (g.shape[0], W.shape[1])
    for k in range(W.shape[1]):
        o = np.nonzero(table[:, k] >= 0)[0]
        if len(o):
            i = table[o, k]
            assert len(np.unique(i)) == len(i)                         # (one tap of a real rulebook never maps two output rows to one input row)
            gx[i] += g[o] @ W[:, k, :]
    return gx


# ---------------------------------------------------------------------------------------------------- what backward.py launches, restated
MUTANTS = ("no_flip", "no_transpose", "slice_right", "child_for_inv", "skip_last_row", "drop_tap")


def conv_step(ci):
    """slice width of backward.conv_backward for `ci` transposed output channels"""
    return ci if ci <= 224 else (128 if ci % 128 == 0 else (96 if ci % 96 == 0 else 32))


def bn_step(ci, co, K, blocked=False):
    """slice width of backward.bn_conv_backward"""
    if ci > 224:
        return conv_step(ci)
    if K == 27 and ci == 2 * co and (ci >= 128 or blocked):
        return co
    return ci


def dgrad_weight(weight, flip, transpose=True):
    """[K][Cin][Cout] weights of the input-gradient conv: W[k]^T, taps reversed when `flip` (float32 in, float32 out)"""
    co, ci = weight.shape[0], weight.shape[-1]
    W = np.asarray(weight).reshape(co, -1, ci)
    wt = np.ascontiguousarray(W.transpose(1, 2, 0)) if transpose else np.ascontiguousarray(W.transpose(1, 0, 2))
    return np.ascontiguousarray(wt[::-1]) if flip else wt


def mutant_applies(mutant, kind, ci, co, step, n_in):
    if mutant == "no_flip":                       # (a level of one row has the centre tap only, and the centre tap is its own flip)
        return kind == "subm" and n_in > 1
    if mutant == "no_transpose":
        return ci == co
    if mutant == "slice_right":
        return step < ci
    if mutant == "child_for_inv":                 # (one fine row has one parent: child and inv are then the same table)
        return kind == "down" and n_in > 1
    if mutant == "skip_last_row":
        return n_in % 32 != 0
    return mutant == "drop_tap"


def transposed_path(gout, weight, t_table, n_in, flip, step, mutant=None, child=None):
    """float64 [n_in, Cin] as backward.py computes it: per column slice [s0, s0 + step) of the transposed weights one gather-GEMM over
    t_table [K, n_in] (None: K = 1, identity), written into that slice's column view of one buffer.  `mutant`: one of MUTANTS --
      no_flip        taps not reversed (SubM)
      no_transpose   W[k] where W[k]^T belongs (square layers)
      slice_right    every slice written one slice to the right (the last one wraps round to the first)
      child_for_inv  the strided conv's gradient gathers over the wrong table of the pair: `child` [K, m] read as if it had n_in columns
                     (columns past m absent, entries that are no row of gout absent)
      skip_last_row  the last row of the last, partial 32-row block is not written
      drop_tap       one tap left out: the centre tap of 27, the fullest tap of 8, the only tap of a 1x1."""
    co, ci = weight.shape[0], weight.shape[-1]
    g = np.asarray(gout, np.float64)
    wt = dgrad_weight(np.asarray(weight, np.float64), flip and mutant != "no_flip", transpose=mutant != "no_transpose")       # [K][ci][co]
    K = wt.shape[0]
    if mutant == "child_for_inv":
        t = np.full((K, n_in), -1, np.int32)
        w = min(n_in, child.shape[1])
        t[:, :w] = child[:, :w]
        t[t >= g.shape[0]] = -1
        t_table = t
    dropped = None
    if mutant == "drop_tap":
        dropped = 13 if K == 27 else (0 if t_table is None else int(np.argmax((t_table >= 0).sum(1))))
    buf = np.zeros((n_in, ci))
    assert ci % step == 0
    for s0 in range(0, ci, step):
        d0 = (s0 + step) % ci if mutant == "slice_right" else s0
        out = buf[:, d0:d0 + step]                                        # a column view of the one buffer
        wsl = wt[:, s0:s0 + step]
        for k in range(K):
            if k == dropped:
                continue
            if t_table is None:
                out += g @ wsl[k].T
            else:
                i = np.nonzero(t_table[k] >= 0)[0]
                if len(i):
                    out[i] += g[t_table[k][i]] @ wsl[k].T
    if mutant == "skip_last_row" and n_in % 32:
        buf[n_in - 1] = 0.0
    return buf


# --------------------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """one layer: kind, forward Cin -> Cout, geometry; `conv_step` / `bn_step` = the slice widths backward.py must choose for the two
    entry points (bn_step None: the layer never sits behind a fused BatchNorm in these tests)"""

    def __init__(self, kind, ci, co, geom, bn=False, dtypes=DTYPES):
        self.kind, self.ci, self.co, self.geom, self.dtypes = kind, ci, co, geom, dtypes
        self.K = taps(kind)
        self.conv_step = conv_step(ci)
        self.bn_step = bn_step(ci, co, self.K) if bn else None
        self.id = f"{kind}-{ci}to{co}-{geom}"

    def tables(self):
        return tables(self.kind, geometry(self.geom))

    def seed(self):
        return sum(self.id.encode()) * 31 + self.ci * 7 + self.co

    def weight_shape(self):
        k = round(self.K ** (1 / 3))
        return (self.co, k, k, k, self.ci)

    def set_a(self):
        """(gout [n_out, Cout], weight [Cout, k, k, k, Cin]) float32, dyadic"""
        rng = np.random.default_rng(self.seed())
        _, n_out, _, _, _, _ = self.tables()
        return dyadic(rng, (n_out, self.co)), dyadic(rng, self.weight_shape())

    def set_b(self, dtype):
        rng = np.random.default_rng(self.seed() + 1)
        _, n_out, _, _, _, _ = self.tables()
        g = round_to(rng.normal(size=(n_out, self.co)).astype(np.float32), dtype)
        w = round_to((rng.normal(size=self.weight_shape()) / np.sqrt(0.6 * self.K * self.co)).astype(np.float32), dtype)
        return g, w

    def bn_input(self, dtype):
        return make_bn_input(self.seed() + 2, self.tables()[3], self.ci, dtype)


def make_bn_input(seed, n, ci, dtype):
    """(x [n, ci] float32 rounded to `dtype`, gamma, beta float32) for the BatchNorm in front of a layer: after training-mode statistics
    no pre-activation gamma * xhat + beta lies within PRE_MARGIN of zero (asserted with a tenfold reserve, in float64: the kernels' fp32
    statistics move a pre-activation by some 1e-6), so the float64 ReLU mask and the kernel's cannot disagree."""
    rng = np.random.default_rng(seed)
    gamma = rng.uniform(0.5, 1.5, ci).astype(np.float32)
    beta = rng.normal(0, 0.3, ci).astype(np.float32)
    x = round_to((rng.normal(size=(n, ci)) * 2 + rng.normal(size=ci)).astype(np.float32), dtype)
    assert n > 1
    for _ in range(50):
        pre = bn_pre(x, gamma, beta)
        close = np.abs(pre) < 20 * PRE_MARGIN
        if not close.any():
            break
        x = round_to(np.where(close, x + np.where(pre >= 0, 0.25, -0.25).astype(np.float32), x), dtype)
    assert np.abs(bn_pre(x, gamma, beta)).min() > 10 * PRE_MARGIN
    return x, gamma, beta


BN_EPS = 1e-4


def bn_pre(x, gamma, beta):
    """float64 pre-activations of the training-mode BatchNorm (biased variance, eps = BN_EPS)"""
    xd = np.asarray(x, np.float64)
    mean, var = xd.mean(0), xd.var(0)
    return (xd - mean) / np.sqrt(var + BN_EPS) * gamma.astype(np.float64) + beta.astype(np.float64)


G = "fine513b2"
CASES = (
    # SubM, 27 taps, square: one launch, flip
    [Case("subm", c, c, G, bn=True) for c in (32, 64, 96, 128, 160, 224)]
    # SubM 2C -> C
    + [Case("subm", 2 * c, c, G, bn=True, dtypes=DTYPES if c != 144 else ("f32", "bf16")) for c in (32, 64, 96, 128, 192, 144, 160, 224)]
    # 1x1 skip
    + [Case("1x1", 2 * c, c, G, bn=True) for c in (32, 64, 128, 224)]
    # strided, 8 taps: the gradient arrives at the fine rows over inv (t_one_hot)
    + [Case("down", 32, 64, G, bn=True), Case("down", 96, 128, G), Case("down", 192, 224, "orphans")]
    # inverse, 8 taps: the gradient arrives at the coarse rows over child
    + [Case("inverse", 64, 32, "coarse513", bn=True), Case("inverse", 128, 96, "coarse513"), Case("inverse", 224, 192, "orphans")]
    # head Linears (autograd._LinearSmallFn.backward: a conv with 3 or 2 INPUT channels when transposed) and the input conv
    + [Case("linear", 32, 32, G), Case("linear", 32, 3, G), Case("linear", 32, 2, G)]
    + [Case("subm", 4, 32, G, dtypes=("f32", "bf16"))]
    # the smaller row counts, one channel pair per kernel family (tests/test_host_dgrad.py names the family each pair reaches)
    + [Case(kind, ci, co, g) for kind, ci, co, gs in (
        ("subm", 32, 32, ("fine1", "fine31", "fine33b2", "fine257")),
        ("subm", 64, 64, ("fine1", "fine31", "fine33b2", "fine257")),
        ("subm", 96, 96, ("fine1", "fine31", "fine33b2", "fine257")),
        ("subm", 224, 224, ("fine1", "fine31", "fine33b2", "fine257")),
        ("subm", 256, 128, ("fine1", "fine31", "fine33b2", "fine257")),
        ("1x1", 64, 32, ("fine1", "fine31", "fine33b2", "fine257")),
        ("down", 32, 64, ("fine1", "fine31", "fine33b2", "fine257", "orphans")),
        ("inverse", 64, 32, ("coarse1", "coarse31", "coarse33", "coarse257b2", "orphans"))) for g in gs]
)
# (case, dtype) the dispatch has no kernel for -- 144 or 32 transposed INPUT channels with 96 or 4 output channels exist only in the generic
# kernel, which the IEEE-half compilation does not carry: backward.conv_backward raises there, nothing is launched (asserted by both test files)
UNSERVED = (("subm-288to144-fine513b2", "f16"), ("subm-4to32-fine513b2", "f16"))
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the slice widths the issue's table records
_WANT = {("subm", 64, 32): (64, 64), ("subm", 128, 64): (128, 64), ("subm", 192, 96): (192, 96), ("subm", 256, 128): (128, 128), ("subm", 384, 192): (128, 128),
         ("subm", 288, 144): (96, 96), ("subm", 320, 160): (32, 32), ("subm", 448, 224): (32, 32), ("1x1", 256, 128): (128, 128), ("1x1", 448, 224): (32, 32),
         ("1x1", 128, 64): (128, 128), ("subm", 224, 224): (224, 224)}
for _c in CASES:
    if (_c.kind, _c.ci, _c.co) in _WANT and _c.bn_step is not None:
        assert (_c.conv_step, _c.bn_step) == _WANT[(_c.kind, _c.ci, _c.co)], _c.id
BN_CASES = [c for c in CASES if c.bn_step is not None]
