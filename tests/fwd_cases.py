"""One case per kernel instantiation the FORWARD conv launches of the net reach (the non-dgrad routes of the `network` section of
tests/golden/conv_routes.json), inputs for which the launch has one right answer, the float64 reference, and mutants of that reference.
The case list of tests/test_host_fwd.py (which proves it on the CPU) and tests/test_gpu_fwd_exact.py (which runs the kernels).  Plain numpy;
of the package only `oracle` is imported (through dgrad_cases).

    reference   y[o] = sum_k W[:, k, :] . pro(x[table[o, k]]) (+ residual[o])        table[o, k] = input row of tap k, -1 = absent: adds 0
                pro(v) = relu(v * scale + shift) where the case has a prologue, v otherwise

over the table in the oracle's layout with the parameter [Cout, k, k, k, Cin] in its own layout.  It knows nothing of fragment-order or
split-bf16 weight copies, channel slices, the column form of a table, scatter forms, presence masks or the block-local row order.

A case names the instantiation it claims (`k_name<template args>`, `/f16` for the IEEE-half compilation), dtype (`x3`: fp32 rows with the
split-bf16 weight copy, the bf16x3 mode), K, Cin, Cout, the table form (none | plain | compact | one_hot | packed | scatter | blk), the residual /
second and third raw view / prologue / `epi` / input column view that the instantiation's template flags require and no more (the epilogue
has tests/test_gpu_conv_epilogue.py), whether tl_conv_fwd's small-level threshold is lowered to 0 (`small0`) or left at 16384, and its
row counts.  The fragment-order weight copy is not a choice: ops.pack_weight makes it whenever Cin and Cout are multiples of 32 and K > 1.
The packed one-hot table i32[n] = (parent row << 3) | tap, -1 = no parent (tl_conv_args.table_one_hot = 2; what tl_forward passes for the
inverse conv of level 1) is read by a run-time branch of the gather-once instantiations of k_conv_direct, so it does not show in a route:
the `packed` cases claim those instantiations a second time and launch through the C ABI, which ops.conv_fwd does not offer it through.

Row counts: ROWS of tests/test_gpu_conv_epilogue.py -- 1, 31, 33 (partial 32-row block), 257 (partial wave / 256-row workgroup), 513
(partial 512-row workgroup) -- on the OUTPUT side, for every instantiation that tl_conv_fwd reaches there with the threshold at 0.  The
forms of k_conv_small are chosen by size (tl_launch_conv_small, nrt = ceil(n / 32) row tiles):
    8 waves x 32 columns   while nrt * Cout / 32 <= 512 and K * Cin / 32 >= 32:  160 -> 192 (K = 8) up to 2720 rows, 128 -> 160 up to 3264,
                           160 -> 128 up to 4096
    full width (16-bit)    Cout / 32 in {3, 5, 7}, a fragment-order copy and nrt >= 128: from 4065 rows
    4 waves x 64 / x 32    otherwise
so those cases run at ROWS + 2720, at 3265 / 4064 / 4065 / 4097 and at 4097 / 4129 rows as the form requires.

Geometries are the real voxel sets of dgrad_cases.geometry: SubM over `nbr`, strided over `child` (output = coarse rows), inverse over
`inv` (output = fine rows; one valid entry per row, none for a row without a parent: the 513-row inverse cases run on `orphans`) with
`child` as its scatter form and Case.packed as its packed form.  Every geometry has absent taps.

Set A (exact): x, W and residual = m / 8, |m| <= 8 (wgrad_cases.dyadic); all-ones cases x = 1; prologue cases scale in {+-1/2, +-1, +-2},
shift = j / 4, |j| <= 8, so pro(x) is a multiple of 1/16 of magnitude <= 4, exact in bf16.  Every product is then a multiple of 1/128 and
every sum of at most 27 x Cin of them, in any order and grouping, stays under 24 significant bits (check_exact asserts it per case from
the sum of the magnitudes), so a kernel that accumulates in fp32 and rounds once must return round_to(reference, dtype) with no difference
in fp32, bf16, f16 and bf16x3 (the lo parts of a split are zero on such data).  Some shifts are positive, so an absent tap that
contributes relu(shift) instead of 0 shows.

Set B: gaussian values rounded to the dtype, weights scaled 1 / sqrt(0.6 K Cin); compared with float64 under TOL (TOL_X3 for bf16x3) of
tests/test_gpu_conv_epilogue.py.
"""
import re

import numpy as np

from dgrad_cases import geometry
from wgrad_cases import dyadic, round_to

ROWS = (1, 31, 33, 257, 513)                     # = ROWS of tests/test_gpu_conv_epilogue.py (asserted in tests/test_host_fwd.py)
MUTANTS = ("skip_last_row", "drop_tap", "swap_taps", "in_block_shift", "out_block_swap", "next_row_table", "absent_gets_shift", "halves_swapped")
BLK_ROWS = (257, 513)                            # block-local clouds: 257 rows (n % 64 == 1), 513 rows in a batch of two (also with split units)
FINE = {1: "fine1", 31: "fine31", 33: "fine33b2", 257: "fine257", 513: "fine513b2"}
COARSE = {1: "coarse1", 31: "coarse31", 33: "coarse33", 257: "coarse257b2", 513: "coarse513"}
SCALES = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32)


# ------------------------------------------------------------------------------------------------------------------------- reference
def prologue(x, scale, shift):
    return x if scale is None else np.maximum(x * scale + shift, 0.0)


def drop_of(table, K):
    """the tap `drop_tap` leaves out and `swap_taps` exchanges with its neighbour: the centre of 27, the fullest of 8, the only one of 1"""
    return 13 if K == 27 else (0 if table is None else int(np.argmax((table >= 0).sum(0))))


def reference(x, weight, table, scale=None, shift=None, residual=None, mutant=None, x_other=None):
    """float64 [n_out, Cout].  table [n_out, K] in the oracle's layout (None: K = 1, every row with itself).  `mutant`: one of MUTANTS --
      skip_last_row      the last row of the last, partial 32-row block gets no sums
      drop_tap           one tap left out (drop_of)
      swap_taps          the weights of that tap and of the next one exchanged
      in_block_shift     input channels read 32 to the right, wrapping
      out_block_swap     the first two 32-column blocks of the weights exchanged
      next_row_table     row r gathers with the table row of r + 1 (the last with that of row 0)
      absent_gets_shift  an absent tap contributes pro(0) = relu(shift) instead of 0
      halves_swapped     the launch reads the other column half of the wide input buffer (`x_other`)"""
    co, ci = weight.shape[0], weight.shape[-1]
    W = np.array(weight, np.float64).reshape(co, -1, ci)
    K = W.shape[1]
    xs = np.asarray(x_other if mutant == "halves_swapped" else x, np.float64)
    if mutant == "in_block_shift":
        xs = np.roll(xs, -32, axis=1)
    sc = None if scale is None else np.asarray(scale, np.float64)
    sh = None if shift is None else np.asarray(shift, np.float64)
    xp = prologue(xs, sc, sh)
    if mutant == "out_block_swap":
        W[:64] = np.concatenate([W[32:64], W[:32]])
    drop = drop_of(table, K)
    if mutant == "swap_taps":
        W[:, [drop, (drop + 1) % K]] = W[:, [(drop + 1) % K, drop]]
    if table is None:
        assert K == 1
        y = np.zeros((xp.shape[0], co)) if mutant == "drop_tap" else xp @ W[:, 0, :].T
    else:
        assert table.shape[1] == K
        t = np.roll(table, -1, axis=0) if mutant == "next_row_table" else table
        y = np.zeros((t.shape[0], co))
        for k in range(K):
            if mutant == "drop_tap" and k == drop:
                continue
            o = np.nonzero(t[:, k] >= 0)[0]
            y[o] += xp[t[o, k]] @ W[:, k, :].T
            if mutant == "absent_gets_shift":
                a = np.nonzero(t[:, k] < 0)[0]
                y[a] += np.maximum(sh, 0.0) @ W[:, k, :].T
    if mutant == "skip_last_row" and y.shape[0] % 32:
        y[-1] = 0.0
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return y


# ----------------------------------------------------------------------------------------------------------------------------- cases
class Data:
    """the operands of one case at one row count: x [n_in, Cin] (the column half the launch reads; `x_other` the other half of an input
    view), w [Cout, k, k, k, Cin], table [n_out, K] or None, scale / shift [Cin] or None, residual [n_out, Cout] or None; float32"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def ref(self, mutant=None):
        return reference(self.x, self.w, self.table, self.scale, self.shift, self.residual, mutant, self.x_other)


class Case:
    def __init__(self, inst, dt, K, ci, co, table, rows=ROWS, small0=True, x3=False, res=False, pro=False, views=1, epi=None, in_view=None,
                 ones=False, tag=""):
        self.inst, self.dt, self.K, self.ci, self.co, self.table = inst, dt, K, ci, co, table
        self.rows, self.small0, self.x3, self.res, self.pro, self.views, self.epi, self.in_view, self.ones = rows, small0, x3, res, pro, views, epi, in_view, ones
        self.kind = {27: "subm", 1: "1x1"}.get(K) or ("down" if table == "plain" else "inverse")
        assert (table == "none") == (K == 1) and (table in ("compact", "blk")) <= (K == 27) and (table in ("one_hot", "scatter", "packed")) <= (K == 8)
        self.frag = co % 32 == 0 and ci % 32 == 0 and K > 1                     # (what ops.pack_weight does)
        self.mode = "bf16x3" if x3 else dt
        s = inst.replace("k_conv_", "").replace("true", "T").replace("false", "F").replace("/f16", "")
        self.id = re.sub(r"[^A-Za-z0-9]+", "-", s).strip("-") + tag + "-" + self.mode

    def geom(self, n):
        """the geometry whose OUTPUT side has n rows"""
        if self.kind == "down":
            return geometry(COARSE.get(n, f"coarse{n}"))
        if self.kind == "inverse" and n == 513:
            return geometry("orphans")
        return geometry(FINE.get(n, f"fine{n}"))

    def tables(self, n):
        """-> (table [n, K] in the oracle's layout or None, kernel table [K, n] or None, scatter form [K, n_in] or None, n_in)"""
        g = self.geom(n)
        if self.kind == "1x1":
            return None, None, None, n
        if self.kind == "subm":
            assert g.n == n
            return g.nbr, g.nbr_k, None, n
        if self.kind == "down":
            assert g.m == n
            return g.child, g.child_k, None, g.n
        assert g.n == n
        return np.ascontiguousarray(g.inv_k.T), g.inv_k, (g.child_k if self.table == "scatter" else None), g.m

    def packed(self, n):
        """the inverse table of n output rows in its packed form i32[n]: (parent row << 3) | tap, -1 for a row without a parent"""
        g = self.geom(n)
        assert self.kind == "inverse" and g.n == n
        return np.where(g.parent >= 0, (g.parent.astype(np.int64) << 3) | g.tap, -1).astype(np.int32)

    def seed(self, n):
        return sum(self.id.encode()) * 131 + n

    def _data(self, n, rng, values, wscale, aff):
        table, _, _, n_in = self.tables(n)
        k = round(self.K ** (1 / 3))
        x = np.ones((n_in, self.ci), np.float32) if self.ones else values((n_in, self.ci))
        x_other = values((n_in, self.ci)) if self.in_view else None
        w = values((self.co, k, k, k, self.ci), wscale)
        scale, shift = aff() if self.pro else (None, None)
        residual = values((n, self.co)) if self.res else None
        return Data(n=n, n_in=n_in, x=x, x_other=x_other, w=w, table=table, scale=scale, shift=shift, residual=residual)

    def set_a(self, n):
        rng = np.random.default_rng(self.seed(n))
        return self._data(n, rng, lambda shape, s=None: dyadic(rng, shape),
                          None, lambda: (rng.choice(SCALES, self.ci).astype(np.float32), (rng.integers(-8, 9, self.ci) / 4.0).astype(np.float32)))

    def set_b(self, n):
        rng = np.random.default_rng(self.seed(n) + 1)
        val = lambda shape, s=1.0: round_to((rng.normal(size=shape) * s).astype(np.float32), self.dt)          # noqa: E731
        return self._data(n, rng, val, 1.0 / np.sqrt(0.6 * self.K * self.ci),
                          lambda: ((rng.uniform(0.5, 1.5, self.ci) * rng.choice([-1.0, 1.0], self.ci)).astype(np.float32), rng.normal(0, 0.3, self.ci).astype(np.float32)))

    def mutant_applies(self, m, d):
        if m == "skip_last_row":
            return d.n % 32 != 0
        if m in ("drop_tap", "swap_taps"):
            return m == "drop_tap" or self.K > 1
        if m == "in_block_shift":
            return self.ci >= 64
        if m == "out_block_swap":
            return self.co >= 64
        if m == "next_row_table":
            return d.table is not None and d.n > 1
        if m == "absent_gets_shift":
            return self.pro and bool((d.shift > 0).any()) and bool((d.table < 0).any())
        assert m == "halves_swapped"
        return self.in_view is not None


def check_exact(c, d):
    """Set A of case c: every product a multiple of 1/128, every sum under 24 significant bits whatever the order -> float64 reference"""
    xp = prologue(d.x.astype(np.float64), d.scale, d.shift)
    assert np.array_equal(xp * 16, np.rint(xp * 16)) and np.abs(xp).max() <= 4.0
    assert np.array_equal(d.w * 8.0, np.rint(d.w * 8.0)) and np.abs(d.w).max() <= 1.0
    for dt in ("bf16", "f16"):
        assert np.array_equal(round_to(xp.astype(np.float32), dt), xp) and np.array_equal(round_to(d.x, dt), d.x) and np.array_equal(round_to(d.w, dt), d.w)
    mag = reference(np.abs(xp), np.abs(d.w), d.table, residual=None if d.residual is None else np.abs(d.residual))
    assert mag.max() * 128 < 2.0 ** 24, (c.id, d.n, mag.max())                   # the largest partial sum possible, in units of 1/128
    ref = d.ref()
    assert np.array_equal(ref * 128, np.rint(ref * 128)) and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    assert np.isfinite(round_to(ref.astype(np.float32), "f16")).all()
    return ref


def C(*a, **kw):
    return Case(*a, **kw)


def _h16(inst, *a, **kw):
    """the bf16 case and its IEEE-half twin"""
    return [Case(inst, "bf16", *a, **kw), Case(inst + "/f16", "f16", *a, **kw)]


SMALL8 = ROWS + (2720,)
CASES = sum([
    # ---- 16-bit, eval forward: level 1 on block-local rows
    _h16("k_conv_ones27<true>", 27, 4, 32, "blk", rows=BLK_ROWS, ones=True),
    _h16("k_conv_blk<8, false, 1, false, false>", 27, 32, 32, "blk", rows=BLK_ROWS),
    _h16("k_conv_blk<8, false, 1, false, true>", 27, 32, 32, "blk", rows=BLK_ROWS, pro=True),
    _h16("k_conv_blk<8, true, 1, false, false>", 27, 32, 32, "blk", rows=BLK_ROWS, res=True),
    _h16("k_conv_blk<8, true, 2, false, false>", 27, 32, 32, "blk", rows=BLK_ROWS, res=True, views=2),
    _h16("k_conv_blk<8, true, 3, false, false>", 27, 32, 32, "blk", rows=BLK_ROWS, res=True, views=3),
    _h16("k_conv_blk<8, true, 1, false, true>", 27, 32, 32, "blk", rows=BLK_ROWS, res=True, pro=True, in_view=(32, 64)),     # conv1.hi of the split 64 -> 32
    _h16("k_conv_blk<8, false, 1, false, true>", 27, 32, 32, "blk", rows=BLK_ROWS, pro=True, in_view=(0, 64), tag="-lo"),  # conv1.lo
    _h16("k_conv_in4<8, true, false>", 27, 4, 32, "compact"),
    # ---- levels 2 .. 4
    _h16("k_conv_stream<true, 8, 2, 1, 3, 2, 2, false, false>", 8, 32, 64, "plain"),
    _h16("k_conv_streamq<27, 2, 1, 2, 8, 1, 2, 1, false, false>", 27, 64, 64, "compact"),
    _h16("k_conv_streamq<8, 3, 1, 2, 8, 1, 2, 1, false, false>", 8, 64, 96, "plain"),
    _h16("k_conv_stream<true, 27, 3, 3, 1, 2, 2, false, false>", 27, 96, 96, "compact"),
    _h16("k_conv_stream<true, 8, 4, 3, 2, 1, 2, false, false>", 8, 96, 128, "plain"),
    _h16("k_conv_streamq<27, 4, 2, 2, 8, 1, 2, 1, false, false>", 27, 128, 128, "plain"),
    _h16("k_conv_streamq<27, 4, 2, 2, 8, 1, 2, 2, false, false>", 27, 256, 128, "plain"),
    _h16("k_conv_streamq<27, 3, 3, 2, 8, 1, 2, 1, false, false>", 27, 192, 96, "compact"),
    _h16("k_conv_streamq<27, 2, 2, 2, 8, 1, 2, 1, false, false>", 27, 128, 64, "compact"),
    _h16("k_conv_bf16<4, 2, 2, true>", 8, 160, 128, "scatter"),
    _h16("k_conv_stream<true, 8, 3, 4, 1, 1, 4, true, false>", 8, 128, 96, "scatter"),
    _h16("k_conv_up<3, 2, 12>", 8, 96, 64, "scatter"),
    _h16("k_conv_direct<true, 8, 1, 2, 2, 16, false, false, true, false>", 8, 64, 32, "scatter"),
    _h16("k_conv_direct<true, 8, 1, 2, 2, 16, false, false, true, false>", 8, 64, 32, "packed", tag="-packed"),
    _h16("k_conv_direct<true, 1, 3, 6, 1, 8, false, false, false, false>", 1, 192, 96, "none"),
    _h16("k_conv_direct<true, 1, 2, 4, 1, 16, false, false, false, false>", 1, 128, 64, "none"),
    _h16("k_conv_direct<true, 1, 1, 2, 1, 16, false, false, false, false>", 1, 64, 32, "none"),
    # ---- the small levels (threshold at its default)
    _h16("k_conv_small<true, 5, 4, true, false>", 8, 128, 160, "plain", rows=(4065, 4097), small0=False),
    _h16("k_conv_small<true, 1, 8, true, false>", 8, 160, 192, "plain", rows=SMALL8, small0=False),
    _h16("k_conv_small<true, 2, 4, false, false>", 1, 384, 192, "none", rows=ROWS + (4065,), small0=False),
    _h16("k_conv_small<true, 1, 4, false, false>", 1, 320, 160, "none", rows=ROWS + (4065,), small0=False),
    # ---- training forward
    _h16("k_conv_direct<true, 27, 1, 1, 3, 16, true, true, false, false>", 27, 32, 32, "compact", epi="stats"),
    _h16("k_conv_direct<true, 27, 1, 2, 3, 8, true, true, false, false>", 27, 64, 32, "compact", epi="stats"),
    _h16("k_conv_direct<true, 1, 1, 2, 1, 16, false, true, false, false>", 1, 64, 32, "none", epi="stats"),
    _h16("k_conv_direct<true, 8, 1, 2, 2, 16, false, true, true, false>", 8, 64, 32, "one_hot", epi="stats"),
    _h16("k_conv_direct<true, 27, 1, 1, 3, 16, true, false, false, false>", 27, 32, 32, "compact"),
    _h16("k_conv_direct<true, 27, 1, 2, 3, 8, true, false, false, false>", 27, 64, 32, "compact"),
    _h16("k_conv_stream<true, 8, 2, 3, 1, 1, 4, true, false>", 8, 96, 64, "one_hot", epi="stats"),
    _h16("k_conv_in4<8, true, true>", 27, 4, 32, "compact", epi="stats"),
], []) + [
    # ---- fp32, eval forward
    C("k_conv_ones27<false>", "f32", 27, 4, 32, "compact", ones=True),
    C("k_conv_ones27<false>", "f32", 27, 4, 32, "blk", rows=BLK_ROWS, ones=True, tag="-blk"),             # (the bf16x3 plan: presence masks of the units)
    C("k_conv_tinycin<float, 4>", "f32", 27, 4, 32, "compact"),
    C("k_conv_direct<false, 27, 1, 1, 2, 8, false, false, false, false>", "f32", 27, 32, 32, "compact"),
    C("k_conv_direct<false, 8, 2, 1, 2, 8, false, false, false, false>", "f32", 8, 32, 64, "plain"),
    C("k_conv_stream<false, 27, 2, 2, 2, 1, 2, false, false>", "f32", 27, 64, 64, "compact"),
    C("k_conv_stream<false, 8, 3, 2, 2, 1, 2, false, false>", "f32", 8, 64, 96, "plain"),
    C("k_conv_stream<false, 27, 3, 3, 1, 1, 2, false, false>", "f32", 27, 96, 96, "compact"),
    C("k_conv_stream<false, 8, 4, 3, 1, 1, 2, false, false>", "f32", 8, 96, 128, "plain"),
    C("k_conv_stream<false, 27, 4, 4, 1, 1, 2, false, false>", "f32", 27, 128, 128, "plain"),
    C("k_conv_stream<false, 8, 3, 4, 1, 1, 2, false, false>", "f32", 8, 128, 96, "scatter"),
    C("k_conv_stream<false, 27, 3, 6, 1, 1, 2, false, false>", "f32", 27, 192, 96, "compact"),
    C("k_conv_mfma_f32<3>", "f32", 1, 192, 96, "none"),
    C("k_conv_stream<false, 8, 2, 3, 1, 1, 4, false, false>", "f32", 8, 96, 64, "scatter"),
    C("k_conv_stream<false, 27, 2, 4, 1, 1, 2, false, false>", "f32", 27, 128, 64, "compact"),
    C("k_conv_direct<false, 1, 2, 4, 1, 8, false, false, false, false>", "f32", 1, 128, 64, "none"),
    C("k_conv_direct<false, 8, 1, 2, 2, 8, false, false, false, false>", "f32", 8, 64, 32, "scatter"),
    C("k_conv_stream<false, 27, 1, 2, 2, 1, 2, false, false>", "f32", 27, 64, 32, "compact"),
    C("k_conv_direct<false, 1, 1, 2, 1, 8, false, false, false, false>", "f32", 1, 64, 32, "none"),
    C("k_conv_small<false, 1, 4, true, false>", "f32", 8, 128, 160, "plain", rows=(3265, 4064, 4065, 4097), small0=False),
    C("k_conv_small<false, 1, 8, true, false>", "f32", 8, 160, 192, "plain", rows=SMALL8, small0=False),
    C("k_conv_small<false, 2, 4, false, false>", "f32", 1, 384, 192, "none", rows=ROWS + (4065,), small0=False),
    C("k_conv_small<false, 1, 4, false, false>", "f32", 1, 320, 160, "none", rows=ROWS + (4065,), small0=False),
    C("k_conv_small<false, 2, 4, true, false>", "f32", 8, 160, 128, "scatter", rows=(4097, 4129), small0=False),
    # ---- fp32, training forward
    C("k_conv_stream<false, 27, 1, 1, 2, 1, 4, false, false>", "f32", 27, 32, 32, "compact", epi="stats"),
    C("k_conv_stream<false, 8, 2, 1, 2, 1, 4, false, false>", "f32", 8, 32, 64, "plain", epi="stats"),
    C("k_conv_stream<false, 8, 1, 2, 2, 1, 4, false, false>", "f32", 8, 64, 32, "one_hot", epi="stats"),
    # ---- bf16x3: fp32 rows, split-bf16 weights
    C("k_conv_blk_x3<8, false, 1>", "f32", 27, 32, 32, "blk", rows=BLK_ROWS, x3=True, pro=True, in_view=(0, 64)),       # conv1.lo
    C("k_conv_blk_x3<8, true, 1>", "f32", 27, 32, 32, "blk", rows=BLK_ROWS, x3=True, res=True),
    C("k_conv_blk_x3<8, true, 1>", "f32", 27, 32, 32, "blk", rows=BLK_ROWS, x3=True, res=True, pro=True, in_view=(32, 64), tag="-hi"),   # conv1.hi
    C("k_conv_blk_x3<8, true, 2>", "f32", 27, 32, 32, "blk", rows=BLK_ROWS, x3=True, res=True, views=2),
    C("k_conv_direct<false, 8, 2, 1, 2, 8, false, false, false, true>", "f32", 8, 32, 64, "plain", x3=True),
    C("k_conv_streamq<27, 2, 2, 1, 8, 1, 2, 1, true, true>", "f32", 27, 64, 64, "compact", x3=True),
    C("k_conv_stream<false, 8, 3, 2, 1, 1, 4, false, true>", "f32", 8, 64, 96, "plain", x3=True),
    C("k_conv_stream<false, 27, 3, 3, 1, 1, 2, false, true>", "f32", 27, 96, 96, "compact", x3=True),
    C("k_conv_stream<false, 8, 4, 3, 1, 1, 2, false, true>", "f32", 8, 96, 128, "plain", x3=True),
    C("k_conv_stream<false, 27, 4, 4, 1, 1, 2, false, true>", "f32", 27, 128, 128, "plain", x3=True),
    C("k_conv_stream<false, 8, 3, 4, 1, 1, 2, true, true>", "f32", 8, 128, 96, "scatter", x3=True),
    C("k_conv_streamq<27, 3, 3, 2, 8, 1, 2, 2, true, false>", "f32", 27, 192, 96, "compact", x3=True),
    C("k_conv_stream<false, 8, 2, 3, 1, 1, 2, true, true>", "f32", 8, 96, 64, "scatter", x3=True),
    C("k_conv_streamq<27, 2, 2, 1, 8, 1, 2, 2, true, false>", "f32", 27, 128, 64, "compact", x3=True),
    C("k_conv_direct<false, 1, 2, 4, 1, 8, false, false, false, true>", "f32", 1, 128, 64, "none", x3=True),
    C("k_conv_direct<false, 8, 1, 2, 2, 12, false, false, true, true>", "f32", 8, 64, 32, "scatter", x3=True),
    C("k_conv_direct<false, 8, 1, 2, 2, 12, false, false, true, true>", "f32", 8, 64, 32, "packed", x3=True, tag="-packed"),
    C("k_conv_direct<false, 1, 1, 2, 1, 8, false, false, false, true>", "f32", 1, 64, 32, "none", x3=True),
    C("k_conv_small<false, 1, 4, true, true>", "f32", 8, 128, 160, "plain", rows=(3265, 4064, 4065, 4097), small0=False, x3=True),
    C("k_conv_small<false, 1, 8, true, true>", "f32", 8, 160, 192, "plain", rows=SMALL8, small0=False, x3=True),
    C("k_conv_small<false, 2, 4, true, true>", "f32", 8, 160, 128, "scatter", rows=(4097, 4129), small0=False, x3=True),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# instantiations of the golden network routes that no row count below 20 000 reaches, with the dispatch condition that prevents it
UNREACHED = {}
