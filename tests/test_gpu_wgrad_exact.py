"""The weight-gradient kernels against float64 on inputs for which fp32 accumulation is EXACT (tests/wgrad_cases.py): no tolerance anywhere.

Set A: x, gout = m / 8 with |m| <= 8, at most 2^18 present pairs per tap -> every partial sum is a multiple of 1/64 with 24 significant bits, so
the kernel must return float32(float64 reference) whatever its summation order.  Set B (16-bit types): one pair per tap on the rows of the
case's tile edges, full-mantissa values -> every entry is one exact product, everything else 0.  A dropped, doubled or misrouted pair, a stale
tile, a wrong widening or a 16-bit accumulator all change the result.

Every case goes through _run(): the C entry point with a NaN-filled workspace and output and a sentinel guard behind
tl_conv_wgrad_ws_floats() floats (idle workgroups must still write their partials; nothing may be written past the documented size), twice for
equal bits, tl_conv_wgrad_ref for the parameter layout [Cout][K][Cin] (Cin % 4 == 0; TL_ERR_UNSUPPORTED otherwise for K > 1), exact equality
of values with the reference, and ops.conv_wgrad (what autograd calls) for the same bits.  Tuning keys are set inside _knobs() and restored;
they hold for the f16 compilation too (tests/test_host_train.py checks that both compilations size the workspace alike under every key).

Which kernel serves which test (bf16 and, through the TL_F16_BUILD compilation of the same unit, f16; row counts come from the kernels' constants):

tl_wgrad.hip
  k_wgrad<1..3, 1..3, false> (fp32)          test_generic, all nine (tiles(Cout), tiles(Cin)) pairs at two or more row counts.  kRowsPerWave =
  k_wgrad<1..3, 1..3, true> (16-bit rows       4096, kWaves = 4: n_out 4095 / 4096 / 4097 and 16384 / 16385; 64-row ballot groups: 63 / 64 / 65;
    that are not 16-B aligned)                 x_ld = Cin + 4 or a view starting at element 4; 6 -> 5 ends in the scalar k_wgrad_reduce, every other
                                               case in k_wgrad_reduce_par; also 4 -> 32 at 29 999 rows (test_in4)
  k_wgrad_bf16<2,1> <1,2> <2,2> <1,1>        test_pair_list (K = 8: 32->64, 64->32, 64->64; K = 27: 32->32, 64->32); 16-pair batches: taps with 15 / 16 /
                                               17 pairs, n_out 15 / 16 / 17; kSG = 256-row super-groups: 255 / 256 / 257; 4096 / 4097, 16385;
                                               <1,1> with K = 1 at 29 999 rows: test_rows_floor
  k_wgrad_bf16<3,3>                          test_pair_list_wide (K = 8, 96->96, 100 000 and 100 001 rows: `wide` needs n_out >= 100 000)
  k_wgrad_bf16s<2,2,1,128>                   test_shared_gout (K = 27: 64->64, 128->64, 40->72 masked); R = 128-row super-groups: 127 / 128 / 129;
                                               4096-row chunks at these sizes: 4095 / 4096 / 4097, 8193; taps 24..26 (three waves of the last group)
  k_wgrad_bf16s<3,3,1,128,true,1>            test_shared_gout_wide -- ONLY with tuning key wgrad_dense = 0 (96->96 and 192->96 at >= 100 000 rows
                                               belong to the dense form by default)
  k_wgrad_reduce / k_wgrad_reduce_par        behind every case above; the [Cout][K][Cin] form of the latter wherever Cin % 4 == 0
tl_wgrad_dense.hip                          test_dense_over_taps, tuning key wgrad_dense_min_rows = 1 (default 60 000); MBR = 64 KS rows per macro
                                               block, gx row slots: n_out 1, MBR -/+ 1, 8 MBR -/+ 1 (one block per XCD) and (gx + 8) MBR + 1 (some
                                               workgroups walk two blocks, some one, some none)
  k_wgrad_dense_dma<1,1,2,4,14> 32->32       wgrad_dma 1 (default)          k_wgrad_dense<1,1,2,4,14>   wgrad_dma 0
  k_wgrad_dense<1,2,1,4,14> 64->32           wgrad_dma 1 and 0 (no DMA form)
  k_wgrad_dense_dma<2,2,1,7,9> 64->64, 128->64   wgrad_dma 1                k_wgrad_dense<2,2,1,4,9>    wgrad_dma 0
  k_wgrad_dense_dma<2,2,1,4,14> 64->64, 128->64  ONLY with tuning key wgrad_dma = 2
  k_wgrad_dense_dma<3,1,2,4,14> 96->96, 192->96  wgrad_dma 1                k_wgrad_dense<3,1,2,4,14>   wgrad_dma 0
  k_wgrad_dense_dma<4,1,1,8,14> 128->128, 256->128   wgrad_dma 1            k_wgrad_dense<4,1,1,4,14>   wgrad_dma 0
  k_wgrad_blk                                test_blk_all_taps (tile, deep split, batch of two)
tl_wgrad_rows.hip
  k_wgrad_rows<1,1,2,2> <1,2,2,2> <2,1,2,2>  test_row_streaming (32->32, 64->32, 96->64, 128->64, 192->96 and 32->96, 256->128 and 96->128); steps of
    <2,2,2,2> <3,1,1,2> <4,1,1,2>              32 or 16 rows: 30 000 + 0 / 1 / 15 / 16 / 17 / 31 / 32 / 33, and 70 001; the floor of 30 000 rows is
                                               crossed by test_rows_floor
  k_wgrad_in4                                test_in4 (30 000, 30 001, 50 001 rows; x_ld 4 and 8)
The K = 1, Cout <= 4 kernels of tl_linear_small.hip are pinned by tests/test_gpu_pointwise_train.py.
"""
import contextlib

import numpy as np
import pytest
import torch

import wgrad_cases as C

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 4096
SENTINEL = -12345.5


@contextlib.contextmanager
def _knobs(**kv):
    from treelearn_amd import _hip
    L = _hip.lib()
    assert set(kv) <= set(C.KNOB_DEFAULTS)
    try:
        for k, v in kv.items():
            assert L.tl_set_tuning(k.encode(), v) == 0
        yield
    finally:
        for k, v in C.KNOB_DEFAULTS.items():
            L.tl_set_tuning(k.encode(), v)


def _rows(a, dtype, layout="contig"):
    """float32 numpy [n][c] (exact in `dtype`) -> device tensor in `dtype`: contiguous, with a row pitch of c + 4 ('ld4'), as the columns 4 .. 4 + c
    of a [n][c + 8] buffer ('col4') or as the first c columns of a [n][2 c] buffer ('wide').  The padding columns hold NaN."""
    t = torch.from_numpy(a).to(TORCH[dtype])
    n, c = t.shape
    if layout == "contig":
        return t.cuda()
    width, c0 = {"ld4": (c + 4, 0), "col4": (c + 8, 4), "wide": (2 * c, 0)}[layout]
    buf = torch.full((n, width), float("nan"), dtype=TORCH[dtype], device="cuda")
    buf[:, c0:c0 + c] = t.cuda()
    return buf[:, c0:c0 + c]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _exact(got, ref, what):
    got = got.cpu().numpy().astype(np.float64)
    bad = got != ref                                              # values: -0 equals +0, a NaN differs from everything
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ; first at [k, co, ci] = {i}: got {got[i]!r}, want {ref[i]!r}")


def _run(x, g, table, K, ref, what, ws_parts=None):
    """x [n_in][Cin], g [n_out][Cout] device tensors of one dtype, table int32 [K][n_out] on the host or None, ref float64 [K][Cout][Cin]."""
    from treelearn_amd import _hip, ops
    L = _hip.lib()
    (n_in, ci), (n_out, co) = x.shape, g.shape
    per = K * co * ci
    code = _hip.dtype_code(x.dtype)
    tab = None if table is None else torch.from_numpy(table).cuda()
    nws = int(L.tl_conv_wgrad_ws_floats(n_out, K, ci, co))
    if ws_parts is not None:                                      # the partial-set count says which form the dispatch takes
        assert nws == ws_parts * per, (what, nws // per, ws_parts)
    buf = torch.empty(nws + GUARD, dtype=torch.float32, device="cuda")

    def call(fn, out):
        buf[:nws] = float("nan"); buf[nws:] = SENTINEL; out.fill_(float("nan"))
        rc = fn(_hip.ptr(x), x.stride(0), _hip.ptr(g), g.stride(0), code, _hip.ptr(tab), n_out, n_in, K, ci, co, _hip.ptr(out), _hip.ptr(buf), _hip.stream())
        torch.cuda.synchronize()
        assert bool((buf[nws:] == SENTINEL).all()), f"{what}: written past tl_conv_wgrad_ws_floats"
        return rc

    gw = torch.empty((K, co, ci), dtype=torch.float32, device="cuda")
    assert call(L.tl_conv_wgrad, gw) == _hip.TL_OK, what
    a = gw.clone()
    assert not bool(torch.isnan(a).any()), f"{what}: {int(torch.isnan(a).sum())} NaN from the poisoned workspace / output"
    assert call(L.tl_conv_wgrad, gw) == _hip.TL_OK and torch.equal(_bits(gw), _bits(a)), f"{what}: second call differs"
    gr = torch.empty((co, K, ci), dtype=torch.float32, device="cuda")
    if ci % 4 == 0:
        assert call(L.tl_conv_wgrad_ref, gr) == _hip.TL_OK and torch.equal(_bits(gr), _bits(a.permute(1, 0, 2))), f"{what}: parameter layout"
    elif K > 1:
        assert call(L.tl_conv_wgrad_ref, gr) == _hip.TL_ERR_UNSUPPORTED, what
    _exact(a, ref, what)
    o = ops.conv_wgrad(x, g, tab, n_out, K)
    assert torch.equal(_bits(o), _bits(a)), f"{what}: ops.conv_wgrad"
    return a


def _cdiv(a, b):
    return -(-a // b)


def _generic_parts(n):
    return _cdiv(n, 16384) * 4


# ------------------------------------------------------------------------------------------------------------------ 1. generic k_wgrad
@pytest.mark.parametrize("i", range(len(C.GENERIC)), ids=[f"{c[0]}to{c[1]}-K{c[2]}-n{c[3]}" for c in C.GENERIC])
def test_generic(i):
    cin, cout, K, n, lay16 = C.GENERIC[i]
    kinds = ["identity"] if K == 1 else ["special", ("r05", "r30", "r90")[i % 3]]
    for kind in kinds:
        x, g, t, ref = C.make_case(100 + i, cin, cout, K, n, kind, tiles=C.GENERIC_TILES)
        for dt in ("f32", "bf16", "f16"):
            lay = lay16 if dt != "f32" else ("contig", "col4")[i % 2]
            _run(_rows(x, dt, lay), _rows(g, dt), t, K, ref, f"{dt} {kind} {lay}", ws_parts=_generic_parts(n))
    if K > 1:
        for dt in ("bf16", "f16"):
            x, g, t, ref = C.make_case(200 + i, cin, cout, K, n, "one", dt, tiles=C.GENERIC_TILES)
            _run(_rows(x, dt, lay16), _rows(g, dt), t, K, ref, f"{dt} one pair {lay16}")


# ------------------------------------------------------------------------------------------------------- 2. pair list k_wgrad_bf16
def _both_16bit(seed, cin, cout, K, n, kinds, tiles, ws_parts=None, x_layout="contig", forms=None):
    """Every kind in bf16 and f16 (Set A data is generated once and shared by the two); forms: [(tuning keys, partial sets)] to run each under."""
    out = {}
    for kind in kinds:
        if kind != "one":
            x, g, t, ref = C.make_case(seed, cin, cout, K, n, kind, tiles=tiles)
        for dt in ("bf16", "f16"):
            if kind == "one":
                x, g, t, ref = C.make_case(seed + 1, cin, cout, K, n, kind, dt, tiles=tiles)
            xd, gd = _rows(x, dt, x_layout), _rows(g, dt)
            for f, (keys, parts) in enumerate(forms or [({}, ws_parts)]):
                with _knobs(**keys):
                    out[f, kind, dt] = _run(xd, gd, t, K, ref, f"{dt} {kind} {keys}", ws_parts=parts)
    return out


@pytest.mark.parametrize("n", C.PAIR_ROWS)
@pytest.mark.parametrize("cin,cout,K", C.PAIR_SHAPES)
def test_pair_list(cin, cout, K, n):
    _both_16bit(300 + n, cin, cout, K, n, ("special", "one"), C.PAIR_TILES, ws_parts=_generic_parts(n))


@pytest.mark.parametrize("cin,cout,K,n,kind", C.PAIR_WIDE)
def test_pair_list_wide(cin, cout, K, n, kind):
    _both_16bit(400 + n, cin, cout, K, n, (kind, "one"), C.PAIR_TILES, ws_parts=_generic_parts(n))


# ---------------------------------------------------------------------------------------------------- 3. shared gout k_wgrad_bf16s
@pytest.mark.parametrize("n", C.SHARED_ROWS)
@pytest.mark.parametrize("cin,cout", C.SHARED_SHAPES)
def test_shared_gout(cin, cout, n):
    _both_16bit(500 + n, cin, cout, 27, n, ("special", "one"), C.SHARED_TILES, ws_parts=_generic_parts(n))


@pytest.mark.parametrize("cin,cout,n,kind", C.SHARED_WIDE)
def test_shared_gout_wide(cin, cout, n, kind):
    from treelearn_amd import _hip
    per = 27 * cin * cout
    assert _hip.lib().tl_conv_wgrad_ws_floats(n, 27, cin, cout) == C.DENSE[(cin, cout)][1] * per         # the default belongs to the dense form
    _both_16bit(600 + n + cin, cin, cout, 27, n, (kind,), C.SHARED_TILES, forms=[(dict(wgrad_dense=0), _generic_parts(n))])


# ------------------------------------------------------------------------------------------------------------ 4. dense over taps
@pytest.mark.parametrize("kind", C.DENSE_KINDS)
@pytest.mark.parametrize("cin,cout,n", [(ci, co, n) for (ci, co) in C.DENSE for n in C.dense_rows(ci, co)])
def test_dense_over_taps(cin, cout, n, kind):
    ks, gx, gx2 = C.DENSE[(cin, cout)]
    tiles = (64, 128, 256, 4096, 8 * 64 * ks)
    forms = [(dict(wgrad_dense_min_rows=1, wgrad_dma=dma), slots) for dma, slots in [(1, gx), (0, gx)] + ([(2, gx2)] if gx2 else [])]
    got = _both_16bit(700 + n, cin, cout, 27, n, (kind,), tiles, forms=forms)
    for (f, k, dt), a in got.items():                            # "same results bit for bit": DMA against register-staged (and wgrad_dma = 2)
        assert torch.equal(_bits(a), _bits(got[0, k, dt])), (forms[f][0], dt)


# --------------------------------------------------------------------------------------------------------------- 5. row streaming
def _rows_parts(n, cin, cout):
    ns = cin // (32 if cout >= 96 else (64 if cin % 64 == 0 else 32))
    return max(_generic_parts(n), min(max(512 // ns, 16), (n // 32 + 7) // 8))


@pytest.mark.parametrize("n", C.ROWS_ROWS)
@pytest.mark.parametrize("cin,cout", C.ROWS_SHAPES)
def test_row_streaming(cin, cout, n):
    _both_16bit(800 + n, cin, cout, 1, n, ("identity",), (), ws_parts=_rows_parts(n, cin, cout))


def test_rows_floor():
    """29 999 rows go to the pair-list kernel, 30 000 to the row-streaming one: both exact, so they differ by exactly the last row's outer product."""
    x, g, _, ref = C.make_case(900, 32, 32, 1, 30000, "identity")
    for dt in ("bf16", "f16"):
        xd, gd = _rows(x, dt), _rows(g, dt)
        hi = _run(xd, gd, None, 1, ref, f"{dt} 30000", ws_parts=_rows_parts(30000, 32, 32))
        lo = _run(xd[:29999], gd[:29999], None, 1, C.reference(x[:29999], g[:29999], None, 1), f"{dt} 29999", ws_parts=_generic_parts(29999))
        last = torch.outer(gd[29999].double(), xd[29999].double())[None]
        assert torch.equal(hi.double() - lo.double(), last)
    with _knobs(wgrad_rows=0):                                   # the same rows through the pair-list kernel: same values
        for dt in ("bf16", "f16"):
            _run(_rows(x, dt), _rows(g, dt), None, 1, ref, f"{dt} 30000, wgrad_rows = 0", ws_parts=_generic_parts(30000))


# ------------------------------------------------------------------------------------------------------------------ 6. k_wgrad_in4
@pytest.mark.parametrize("layout", ["contig", "wide"])
@pytest.mark.parametrize("kind", C.IN4_KINDS)
@pytest.mark.parametrize("n", C.IN4_ROWS)
def test_in4(n, kind, layout):
    parts = max(_generic_parts(n), min(512, (n // 16 + 7) // 8) if n >= 30000 else 0)
    _both_16bit(1000 + n, 4, 32, 27, n, (kind,), (), ws_parts=parts, x_layout=layout)


# -------------------------------------------------------------------------------------------------------------------- 7. k_wgrad_blk
@pytest.mark.parametrize("case", ["tile", "deep split", "batch of two"])
def test_blk_all_taps(case):
    """tl_conv_wgrad_blk over real block-local rulebooks (the geometries of test_blk_weight_gradient_equals_the_plain_table_kernel; the batch of two
    takes 9 m tiles so that its centre tap stays under the 2^18-pair cap), Set A, all 27 taps against float64 over nn_table, both layouts."""
    import treelearn_amd.geometry as G
    from test_gpu_blk import _batch, _geoms
    from treelearn_amd import _hip, ops
    batch = _batch(9.0, [3, 5]) if case == "batch of two" else _batch(14.0, [3])
    old = G.BLK_HALO_MAX
    if case == "deep split":
        G.BLK_HALO_MAX = 26
    try:
        _, blk = _geoms(batch, blk_min_rows=1, nn_table=True)
    finally:
        G.BLK_HALO_MAX = old
    r = blk.levels[0].nbr
    n = r.n
    rng = np.random.default_rng(1100)
    x, g = C.dyadic(rng, (n, 32)), C.dyadic(rng, (n, 32))
    table = r.nn_table.cpu().numpy()
    ref = C.reference(x, g, table, 27)
    assert int((table[13] >= 0).sum()) == n                      # real rulebooks hold the centre tap on every row
    L = _hip.lib()
    nws = int(L.tl_conv_wgrad_blk_ws_floats())
    buf = torch.empty(nws + GUARD, dtype=torch.float32, device="cuda")
    for dt in ("bf16", "f16"):
        _blk_one(L, r, n, _rows(x, dt, "wide"), _rows(g, dt), buf, nws, ref, f"{case} {dt}")


def _blk_one(L, r, n, xd, gd, buf, nws, ref, what):
    from treelearn_amd import _hip, ops
    outs = []
    for ref_layout in (0, 1, 0):
        buf[:nws] = float("nan"); buf[nws:] = SENTINEL
        gw = torch.full((32, 27, 32) if ref_layout else (27, 32, 32), float("nan"), dtype=torch.float32, device="cuda")
        rc = L.tl_conv_wgrad_blk(_hip.ptr(xd), xd.stride(0), _hip.ptr(gd), gd.stride(0), _hip.dtype_code(xd.dtype), _hip.ptr(r.unit), _hip.ptr(r.counter),
                                 _hip.ptr(r.halo), _hip.ptr(r.lrb), n, 32, 32, _hip.ptr(gw), ref_layout, _hip.ptr(buf), _hip.stream())
        torch.cuda.synchronize()
        assert rc == _hip.TL_OK and bool((buf[nws:] == SENTINEL).all()) and not bool(torch.isnan(gw).any())
        outs.append(gw.permute(1, 0, 2).contiguous() if ref_layout else gw)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
    _exact(outs[0], ref, what)
    o = ops.conv_wgrad(xd, gd, r, n, 27)
    assert torch.equal(_bits(o), _bits(outs[0]))
