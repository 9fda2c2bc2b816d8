"""Inputs for which the weight gradient of the sparse convs has ONE right answer in fp32, the tables that put pairs on the kernels' tile
edges, the float64 reference and the case lists of tests/test_gpu_wgrad_exact.py.  Plain numpy; nothing of the package is imported.

    gW[k][co][ci] = sum over output rows o with table[k][o] >= 0 of  gout[o][co] * x[table[k][o]][ci]

Set A (dyadic): every element of x and gout is m / 8 with an integer m in [-8, 8] -- exact in bf16, f16 and fp32.  Every product is a multiple
of 1/64 of magnitude <= 1, so a sum of at most 2^18 of them, in any order and any grouping into partial sums, is a multiple of 1/64 of
magnitude <= 2^18: 24 significant bits, exactly representable in fp32.  A kernel that accumulates in fp32 must return float32(reference)
with no difference at all.  PAIR_CAP = 2^18 present pairs per tap is asserted by reference().

Set B (one pair per tap, full mantissa; 16-bit types): gaussian values rounded to the type, 2^-4 <= |v| <= 2^4.  With one present pair per tap every
entry of gW is one product of two 8-bit (bf16) or 11-bit (f16) significands: 16 or 22 bits, exact in fp32; every other entry is exactly 0.
"""
import numpy as np

PAIR_CAP = 1 << 18
KNOB_DEFAULTS = dict(wgrad_dense=1, wgrad_dma=1, wgrad_rows=1, wgrad_dense_min_rows=60000)


# ------------------------------------------------------------------------------------------------------------------------------ data
def dyadic(rng, shape):
    """Set A: m / 8, m uniform in [-8, 8], as float32 (exact in every dtype the kernels take)."""
    return (rng.integers(-8, 9, size=shape).astype(np.float32) / np.float32(8)).astype(np.float32)


def round_to(a, dtype):
    """float32 array rounded (to nearest, ties to even) to `dtype` ('bf16', 'f16' or 'f32'), returned as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "f32":
        return a
    if dtype == "f16":
        return a.astype(np.float16).astype(np.float32)
    assert dtype == "bf16"
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def mantissa(rng, shape, dtype):
    """Set B: gaussian values rounded to the 16-bit dtype, magnitudes clipped to [2^-4, 2^4] (no subnormals, no overflow of a product)."""
    assert dtype in ("bf16", "f16")
    v = rng.normal(size=shape).astype(np.float32)
    v = np.where(v < 0, -1.0, 1.0).astype(np.float32) * np.clip(np.abs(v), 2.0 ** -4, 2.0 ** 4)
    return round_to(v, dtype)


# ---------------------------------------------------------------------------------------------------------------------------- tables
def random_table(rng, K, n_out, n_in, presence):
    """int32 [K][n_out]: every entry present with probability `presence`, pointing at a uniform input row."""
    t = rng.integers(0, n_in, size=(K, n_out)).astype(np.int32)
    t[rng.uniform(size=t.shape) >= presence] = -1
    return t


def special_table(rng, K, n_out, n_in):
    """Random at 0.3, then (as far as K reaches):
    tap 0 absent; tap 1 every row -> itself modulo n_in; tap 2 one pair, last row -> input row n_in - 1; tap 3 one pair, row 0 -> input row 0;
    tap 4 every row -> the SAME input row; taps 5 / 6 / 7 exactly 15 / 16 / 17 pairs inside the first 64 rows (one MFMA batch of 16, one less,
    one more; fewer where n_out is smaller); taps 24 / 25 / 26 (the last group of four waves of the shared-gout kernel, one wave idle) one pair
    each: a middle row -> input row 0, the last row -> input row 0, row 0 -> input row n_in - 1."""
    t = random_table(rng, K, n_out, n_in, 0.3)
    rows = np.arange(n_out)
    if K > 0: t[0] = -1
    if K > 1: t[1] = (rows % n_in).astype(np.int32)
    if K > 2: t[2] = -1; t[2, n_out - 1] = n_in - 1
    if K > 3: t[3] = -1; t[3, 0] = 0
    if K > 4: t[4] = n_in // 2
    first = min(64, n_out)
    for k, cnt in ((5, 15), (6, 16), (7, 17)):
        if K > k:
            t[k] = -1
            sel = np.sort(rng.choice(first, size=min(cnt, first), replace=False))
            t[k, sel] = rng.integers(0, n_in, size=len(sel)).astype(np.int32)
    for k, (o, i) in ((24, (n_out // 2, 0)), (25, (n_out - 1, 0)), (26, (0, n_in - 1))):
        if K > k:
            t[k] = -1; t[k, o] = i
    return t


def edge_rows(K, n_out, tiles, rng):
    """K output rows for the one-pair table: 0, n_out - 1, then t - 1 and t for every tile size t (then 2t - 1, 2t, ...), as far as n_out
    reaches; distinct while n_out >= K (filled up with seeded random rows), cycled otherwise."""
    rows = [0, n_out - 1]
    for mult in (1, 2, 3):
        for t in tiles:
            rows += [mult * t - 1, mult * t]
    out = []
    for r in rows:
        if 0 <= r < n_out and r not in out:
            out.append(r)
    if len(out) < K and n_out >= K:
        rest = np.setdiff1d(np.arange(n_out), np.array(out))
        out += [int(v) for v in rng.choice(rest, size=K - len(out), replace=False)]
    return [out[k % len(out)] for k in range(K)]


def one_pair_table(rng, K, n_out, n_in, tiles):
    """Set B's table: exactly one present pair per tap, on the rows of edge_rows(); input rows 0 and n_in - 1 for the first two taps, uniform after."""
    t = np.full((K, n_out), -1, np.int32)
    rows = edge_rows(K, n_out, tiles, rng)
    for k in range(K):
        t[k, rows[k]] = 0 if k == 0 else (n_in - 1 if k == 1 else int(rng.integers(0, n_in)))
    return t


# ------------------------------------------------------------------------------------------------------------------------- reference
def reference(x, g, table, K):
    """float64 [K][Cout][Cin]: per tap, g[m].T @ x[t[m]] over the present rows m (table None: K = 1, every row with itself)."""
    x = np.asarray(x, np.float64); g = np.asarray(g, np.float64)
    ref = np.zeros((K, g.shape[1], x.shape[1]))
    if table is None:
        assert K == 1 and x.shape[0] == g.shape[0] and g.shape[0] <= PAIR_CAP
        ref[0] = g.T @ x
        return ref
    assert table.shape == (K, g.shape[0]) and table.dtype == np.int32
    for k in range(K):
        m = table[k] >= 0
        assert int(m.sum()) <= PAIR_CAP, (k, int(m.sum()))            # beyond the cap fp32 partial sums of Set A are no longer exact
        assert int(table[k].max(initial=-1)) < x.shape[0]
        if m.any():
            ref[k] = g[m].T @ x[table[k][m]]
    return ref


def reference_int64(x, g, table, K):
    """The same sum in integers for Set A data (x = mx / 8, g = mg / 8): (sum mg * mx) / 64, no rounding anywhere."""
    mx = np.rint(np.asarray(x, np.float64) * 8).astype(np.int64); mg = np.rint(np.asarray(g, np.float64) * 8).astype(np.int64)
    assert np.array_equal(mx / 8.0, x) and np.array_equal(mg / 8.0, g)
    ref = np.zeros((K, g.shape[1], x.shape[1]), np.int64)
    for k in range(K):
        if table is None:
            ref[k] = mg.T @ mx
        else:
            m = table[k] >= 0
            ref[k] = mg[m].T @ mx[table[k][m]]
    return ref


def make_case(seed, cin, cout, K, n_out, kind, dtype="bf16", tiles=(64, 128, 256, 4096), n_in=None):
    """(x, g, table, reference) for one case.  kind: 'r05' / 'r30' / 'r90' (random presence), 'special', 'identity' (table None, K = 1) -- all Set
    A -- or 'one' (Set B in `dtype`, the one-pair table over `tiles`)."""
    rng = np.random.default_rng(seed)
    if n_in is None:
        n_in = n_out + 50 if K > 1 else n_out
    if kind == "one":
        x = mantissa(rng, (n_in, cin), dtype); g = mantissa(rng, (n_out, cout), dtype)
        table = one_pair_table(rng, K, n_out, n_in, tiles)
    else:
        x = dyadic(rng, (n_in, cin)); g = dyadic(rng, (n_out, cout))
        if kind == "identity":
            assert K == 1 and n_in == n_out
            table = None
        elif kind == "special":
            table = special_table(rng, K, n_out, n_in)
        else:
            table = random_table(rng, K, n_out, n_in, {"r05": 0.05, "r30": 0.3, "r90": 0.9}[kind])
    return x, g, table, reference(x, g, table, K)


# ------------------------------------------------------------------------------------------------------------------------ case lists
# 1. generic k_wgrad<NBO, NBI, BF16> (tl_wgrad.hip): fp32, and 16-bit rows that are not 16-B aligned.  tiles(c) = 1 (c <= 32), 2 (33..64 and
#    > 96), 3 (65..96): all nine (tiles(Cout), tiles(Cin)) pairs of the TL_W switch, each at two or more row counts; widths 24 / 40 / 72 (not
#    multiples of 32), 100 (two 64-wide blocks, the second masked), 6 -> 5 (Cin % 4 != 0: the scalar k_wgrad_reduce).  Row counts: 64 = one
#    ballot group, 4096 = rows per wave, 16384 = rows per workgroup (4 waves).  (cin, cout, K, n_out, 16-bit layout)
GENERIC = [
    (24, 32, 8, 1, "ld4"), (6, 5, 27, 65, "ld4"), (32, 24, 1, 4097, "col4"),                 # <1,1>
    (40, 24, 27, 63, "col4"), (64, 32, 8, 4096, "ld4"),                                      # <1,2>
    (72, 32, 8, 2, "ld4"), (96, 24, 1, 16385, "col4"),                                       # <1,3>
    (32, 40, 27, 64, "col4"), (24, 64, 8, 4095, "ld4"),                                      # <2,1>
    (40, 64, 8, 4097, "col4"), (100, 40, 27, 65, "ld4"), (64, 100, 1, 16384, "ld4"),         # <2,2>
    (72, 40, 27, 4095, "ld4"), (96, 64, 8, 16385, "col4"),                                   # <2,3>
    (32, 72, 1, 63, "ld4"), (24, 96, 27, 4096, "col4"),                                      # <3,1>
    (40, 96, 8, 64, "ld4"), (64, 72, 27, 1, "col4"),                                         # <3,2>
    (72, 72, 27, 2, "col4"), (96, 96, 8, 16384, "ld4"), (72, 96, 1, 4097, "ld4"),            # <3,3>
]
GENERIC_TILES = (64, 4096, 16384)

# 2. pair-list k_wgrad_bf16<NBO, NBI> (aligned 16-bit rows): 16 pairs = one MFMA batch, 256 rows = one compaction super-group (kSG), 4096 rows per
#    wave, 16384 per workgroup.  (cin, cout, K) x n_out; K = 27 with a 32-wide side stays here below the dense form's row threshold.
PAIR_SHAPES = [(32, 64, 8), (64, 32, 8), (64, 64, 8), (32, 32, 27), (64, 32, 27)]            # <2,1> <1,2> <2,2> <1,1> <1,2>
PAIR_ROWS = [1, 15, 16, 17, 255, 256, 257, 4096, 4097, 16385]
PAIR_TILES = (16, 64, 256, 4096, 16384)
PAIR_WIDE = [(96, 96, 8, 100000, "r30"), (96, 96, 8, 100001, "special")]                     # <3,3>: multiples of 96 at >= 100 000 rows

# 3. shared-gout k_wgrad_bf16s<2,2,1,128> (K = 27, both sides > 32 channels): 128 rows per super-group (R), chunks of 4096 rows at these sizes
SHARED_SHAPES = [(64, 64), (128, 64), (40, 72)]                                              # 40 -> 72: one masked block per side
SHARED_ROWS = [1, 127, 128, 129, 4095, 4096, 4097, 8193]
SHARED_TILES = (64, 128, 4096)
SHARED_WIDE = [(96, 96, 100001, "r90"), (96, 96, 100000, "special"), (192, 96, 100000, "r30"), (192, 96, 100001, "special")]   # <3,3,1,128,true,1>, wgrad_dense = 0

# 4. dense over taps (wgrad_dense_min_rows = 1): (cin, cout) -> (KS, slots gx with wgrad_dma 1 and 0, slots with wgrad_dma 2 or None); a macro
#    block is MBR = 64 KS rows
DENSE = {(32, 32): (2, 128, None), (64, 32): (1, 128, None), (64, 64): (1, 80, 128), (128, 64): (1, 40, 64),
         (96, 96): (2, 40, None), (192, 96): (2, 64, None), (128, 128): (1, 32, None), (256, 128): (1, 16, None)}
DENSE_KINDS = ("r05", "special", "one")


def dense_rows(cin, cout):
    ks, gx, gx2 = DENSE[(cin, cout)]
    mbr = 64 * ks
    rows = [1, mbr - 1, mbr, mbr + 1, 8 * mbr - 1, 8 * mbr + 1, (gx + 8) * mbr + 1]
    if gx2:
        rows.append((gx2 + 8) * mbr + 1)
    return rows


# 5. row-streaming k_wgrad_rows (K = 1, no table, >= 30 000 rows): steps of 32 rows (KS = 2: Cout 32, 64) or 16 rows (Cout 96, 128)
ROWS_SHAPES = [(32, 32), (64, 32), (96, 64), (128, 64), (192, 96), (32, 96), (256, 128), (96, 128)]   # <1,1,2,2> <1,2,2,2> <2,1,2,2> <2,2,2,2> <3,1,1,2> x 2, <4,1,1,2> x 2
ROWS_ROWS = [30000 + d for d in (0, 1, 15, 16, 17, 31, 32, 33)] + [70001]

# 6. k_wgrad_in4 (K = 27, 4 -> 32, >= 30 000 rows; 29 999 rows: the generic kernel): steps of 16 rows
IN4_ROWS = [29999, 30000, 30001, 50001]
IN4_KINDS = ("special", "r30")


def smallest_cases():
    """Every generator at its smallest size, Set A: (name, x, g, table, K) for the CPU self-check."""
    out = []
    for name, (cin, cout, K, n_out, kind) in {
            "generic": (24, 32, 8, 1, "special"), "generic K=27": (6, 5, 27, 65, "special"), "generic K=1": (32, 72, 1, 63, "identity"),
            "pair list": (32, 64, 8, 17, "special"), "shared gout": (40, 72, 27, 129, "special"), "dense r05": (32, 32, 27, 129, "r05"),
            "dense special": (64, 32, 27, 65, "special"), "r30": (4, 32, 27, 300, "r30"), "r90": (96, 96, 27, 200, "r90")}.items():
        x, g, t, _ = make_case(7, cin, cout, K, n_out, kind)
        out.append((name, x, g, t, K))
    return out
