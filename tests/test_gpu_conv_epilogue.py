"""The conv epilogue (tl_conv_internal.h) of every kernel family tl_conv_fwd's dispatch reaches, at the edges of its row tiling: up to three
output views with their own BatchNorm affine / ReLU, the residual, column-view destinations.

The stream and stream-q kernels read the views' affines from a workgroup copy in LDS and request the residual rows ahead of their first
store; the other families load them per view.  Either way a view must get ITS affine of ITS column block, the arithmetic (residual add,
fmaf, fmaxf, one rounding) must be the one of a one-view launch bit for bit, and nothing outside the n_out x C destination may be touched.

Rows: 1, 31, 33 (partial 32-row block), 257 (partial wave / 256-row workgroup), 513 (partial 512-row workgroup).  The large-level
families are reached at these sizes by lowering tl_conv_fwd's small-level threshold (tl_set_tuning "small_rows") for the test.
Tolerances against float64: those of tests/test_gpu_parity.py (fp32 2e-5, bf16 8e-3 = two units of a bf16 rounding, 2 * 2^-8); float16 by
the same rule from its precision, 2 * 2^-11; fp32 rows with split-bf16 weights (bf16x3): the 5e-5 of tests/test_gpu_x3.py."""
import numpy as np
import pytest
import torch

from oracle import sparse_ops as osp

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 8e-3, torch.float16: 2 * 2.0 ** -11}
TOL_X3 = 5e-5
ROWS = (1, 31, 33, 257, 513)
SENT = -1024.0                      # exact in every dtype
H16 = (torch.bfloat16, torch.float16)
ALL = (torch.bfloat16, torch.float16, torch.float32)

# (family the dispatch serves the shape with -- asserted through ops.conv_route: the label's first word names the kernel, KERNEL_OF --,
#  Cin, Cout, K, rulebook kind, small-level threshold left on, dtypes)
KERNEL_OF = {"stream-q": "k_conv_streamq", "stream": "k_conv_stream", "direct": "k_conv_direct", "k_conv_up": "k_conv_up", "small-level": "k_conv_small",
             "k_conv_bf16": "k_conv_bf16"}
FAMILIES = [
    ("stream-q 64->64", 64, 64, 27, "table", False, H16),
    ("stream-q 128->64", 128, 64, 27, "table", False, H16),
    ("stream-q 192->96", 192, 96, 27, "table", False, H16),
    ("stream-q 128->128", 128, 128, 27, "table", False, H16),
    ("stream 96->96", 96, 96, 27, "table", False, ALL),
    ("stream strided 32->64", 32, 64, 8, "table", False, H16),
    ("direct strided 32->64", 32, 64, 8, "table", False, (torch.float32,)),
    ("direct 1x1 128->64", 128, 64, 1, "none", False, ALL),
    ("direct one-hot inverse 64->32", 64, 32, 8, "one_hot", False, H16),
    ("k_conv_up 96->64", 96, 64, 8, "up", False, H16),
    ("small-level 160->160", 160, 160, 27, "table", True, ALL),
    ("k_conv_bf16 224->224", 224, 224, 27, "table", False, H16),
]
CASES = [pytest.param(f, dt, id=f"{f[0]}-{str(dt).split('.')[1]}") for f in FAMILIES for dt in f[6]]
# fp32 rows with the split-bf16 weight copy (ops.PACK_X3): the fp32-row instantiations of the stream-q and stream kernels
X3_FAMILIES = [
    ("stream-q bf16x3 64->64", 64, 64, 27, "table", False, (torch.float32,)),
    ("stream-q bf16x3 128->64", 128, 64, 27, "table", False, (torch.float32,)),
    ("stream-q bf16x3 192->96", 192, 96, 27, "table", False, (torch.float32,)),
    ("stream bf16x3 96->96", 96, 96, 27, "table", False, (torch.float32,)),
    ("stream bf16x3 one-hot inverse 96->64", 96, 64, 8, "one_hot", False, (torch.float32,)),
]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda")


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


class _small_rows:
    """tl_conv_fwd's small-level threshold lowered to 0 (and restored): the large-level families serve tiny row counts."""
    def __init__(self, keep):
        self.keep = keep

    def __enter__(self):
        from treelearn_amd import _hip
        if not self.keep:
            _hip.check(_hip.lib().tl_set_tuning(b"small_rows", 0), "small_rows")

    def __exit__(self, *exc):
        from treelearn_amd import _hip
        _hip.lib().tl_set_tuning(b"small_rows", 16384)


def _rulebook(rng, kind, K, n_out):
    """-> (n_in, table i32[n_out, K] for the oracle or None, scatter i32[K, n_in] or None)"""
    if kind == "none":
        return n_out, None, None
    if kind == "table":                                       # random sparse rulebook with absent entries
        n_in = n_out + 37
        t = rng.integers(0, n_in, size=(n_out, K)).astype(np.int32)
        t[rng.uniform(size=t.shape) < 0.4] = -1
        return n_in, t, None
    n_in = n_out // 3 + 2                                     # inverse conv: every output row has one parent and one tap, a (tap, parent) pair at most one child
    pair = rng.permutation(K * n_in)[:n_out]
    t = np.full((n_out, K), -1, np.int32)
    t[np.arange(n_out), pair % K] = (pair // K).astype(np.int32)
    sc = np.full((K, n_in), -1, np.int32)
    sc[pair % K, pair // K] = np.arange(n_out, dtype=np.int32)
    return n_in, t, (sc if kind == "up" else None)


def _views(rng, cout, d):
    """three view specs (scale, shift, relu), each with its own parameters: raw; affine of mixed sign + ReLU; negative affine, ReLU off"""
    T = lambda a: torch.from_numpy(a.astype(np.float32)).to(d)
    a = rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout); b = rng.normal(0, 0.3, cout)
    c = -rng.uniform(0.5, 1.5, cout); e = rng.normal(0, 0.3, cout)
    return [(None, None, False), (T(a), T(b), True), (T(c), T(e), False)]


def _dest(n_out, cout, dtype, d):
    buf = torch.full((n_out + 3, 2 * cout), SENT, dtype=dtype, device=d)
    return buf, buf[:n_out, cout:]


def _intact(buf, n_out, cout):
    return bool((buf[:, :cout] == SENT).all()) and bool((buf[n_out:] == SENT).all())


def _launch(ops, x, w, tab, n_out, specs, cout, dtype, d, **kw):
    """one launch writing the views `specs` (1..3) -> their tensors; asserts the sentinels around every destination"""
    bufs = [_dest(n_out, cout, dtype, d) for _ in specs]
    s0 = specs[0]
    extra = {}
    for name, (buf, view), s in zip(("out2", "out3"), bufs[1:], specs[1:]):
        extra[name] = (view, s[0], s[1], s[2])
    kernel = kw.pop("kernel", None)
    if kernel is not None:                                    # the family under test is the one the dispatch serves these very arguments with
        route = ops.conv_route(x, w, tab, n_out, out=bufs[0][1], out_scale=s0[0], out_shift=s0[1], out_relu=s0[2], **extra, **kw)
        assert route.startswith(kernel + "<") and ("/f16<<<" in route) == (dtype == torch.float16), (kernel, route)
    ops.conv_fwd(x, w, tab, n_out, out=bufs[0][1], out_scale=s0[0], out_shift=s0[1], out_relu=s0[2], **extra, **kw)
    for buf, _ in bufs:
        assert _intact(buf, n_out, cout), "a store outside the n_out x C destination"
    return [view.clone(memory_format=torch.contiguous_format) for _, view in bufs]


def _same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("fam,dtype", CASES)
def test_conv_epilogue_views_residual_edges(fam, dtype):
    _run_family(fam, dtype, TOL[dtype], x3=False)


@pytest.mark.parametrize("fam", X3_FAMILIES, ids=[f[0] for f in X3_FAMILIES])
def test_conv_epilogue_views_residual_edges_bf16x3(fam):
    _run_family(fam, torch.float32, TOL_X3, x3=True)


def _pack(ops, w, dtype, x3):
    if not x3:
        return ops.pack_weight(w, dtype)
    ops.PACK_X3 = True
    try:
        wp = ops.pack_weight(w, dtype)
    finally:
        ops.PACK_X3 = False
    assert getattr(wp, "_tl_x3", None) is not None
    return wp


def _run_family(fam, dtype, tol, x3):
    from treelearn_amd import ops
    name, cin, cout, K, kind, keep_small, _ = fam
    d = _dev()
    rng = np.random.default_rng(cin * 131 + cout * 7 + K)
    k = round(K ** (1 / 3))
    rnd = lambda a: torch.from_numpy(a.astype(np.float32)).to(dtype).double().numpy()      # the dtype's rounding, as float64
    w64 = rnd(rng.normal(size=(cout, k, k, k, cin)) / np.sqrt(cin * K * 0.6))
    views = _views(rng, cout, d)
    raw, act, neg = views
    sets = ([raw], [act], [raw, act], [raw, act, neg])
    with _small_rows(keep_small):
        wp = _pack(ops, torch.from_numpy(w64).float().to(d), dtype, x3)
        for n_out in ROWS:
            n_in, table, scatter = _rulebook(rng, kind, K, n_out)
            x64 = rnd(rng.normal(size=(n_in, cin)))
            res64 = rnd(rng.normal(size=(n_out, cout)))
            x = torch.from_numpy(x64).to(d).to(dtype)
            resbuf = torch.zeros((n_out, cout + 8), dtype=dtype, device=d)                 # res_ld > C
            resbuf[:, :cout] = torch.from_numpy(res64).to(d).to(dtype)
            res = resbuf[:, :cout]
            tab = None if table is None else torch.from_numpy(np.ascontiguousarray(table.T)).to(d)
            kw = {"kernel": KERNEL_OF[name.split()[0]]}
            if kind in ("one_hot", "up"):
                kw["one_hot"] = True
            if scatter is not None:
                kw["scatter"] = torch.from_numpy(scatter).to(d)
            tbl = table if table is not None else np.arange(n_out, dtype=np.int32)[:, None]
            ref = osp.conv_table(torch.from_numpy(x64), torch.from_numpy(w64), tbl, n_out).numpy()
            for residual in ((None,) if kind == "up" else (None, res)):                     # (k_conv_up takes no residual)
                kr = dict(kw, residual=residual) if residual is not None else kw
                y64 = ref + (res64 if residual is not None else 0.0)
                single = {}                                                                 # the one-view launch of each spec, once
                for i, s in enumerate(views):
                    single[i] = _launch(ops, x, wp, tab, n_out, [s], cout, dtype, d, **kr)[0]
                    want = y64 if s[0] is None else y64 * s[0].double().cpu().numpy() + s[1].double().cpu().numpy()
                    if s[2]:
                        want = np.maximum(want, 0.0)
                    err = rel_err(single[i].double().cpu().numpy(), want)
                    assert err < tol, (name, n_out, residual is not None, i, err)
                for specs in sets:
                    got = _launch(ops, x, wp, tab, n_out, specs, cout, dtype, d, **kr)
                    for g, s in zip(got, specs):
                        i = [j for j, v in enumerate(views) if v is s][0]
                        assert _same_bits(g, single[i]), (name, n_out, residual is not None, len(specs), i)
                if dtype == torch.float32 and residual is not None:
                    # fp32: the kernel's own sums are observable -- with the residual it must store exactly sums + residual
                    plain = _launch(ops, x, wp, tab, n_out, [raw], cout, dtype, d, **kw)[0]
                    assert torch.equal(single[0], plain + res), (name, n_out)


# (name, Cin, Cout, K, rows per workgroup and 32-row blocks per wave of the stream kernels -- their partial rows are pinned exactly)
TRAIN = [("stream-q 64->64", 64, 64, 27, 256, 1), ("stream 96->96", 96, 96, 27, 512, 2), ("direct 1x1 64->32", 64, 32, 1, None, None),
         ("direct 64->32", 64, 32, 27, None, None)]


def _stream_partial_sums(t32, n, rows_wg, rb_per_wave):
    """The first partial row of every workgroup of a stream / stream-q training launch, operation for operation: per wave and 32-row block each
    column's rows 0..15 and 16..31 are added in order in fp32, the two halves are added, the wave's blocks are added in order (fp32), and
    the workgroup's eight waves are added in wave order in fp64 (tile_colsum, epi_block32, epi_finish_wg).  t32 = the summand as stored."""
    nwg = -(-n // rows_wg)
    c = t32.shape[1]
    pad = np.zeros((nwg * rows_wg, c), np.float32); pad[:n] = t32
    out = np.zeros((nwg, c), np.float64)
    for g in range(nwg):
        for w in range(8):
            red = np.zeros(c, np.float32)
            for rb in range(rb_per_wave):
                blk = pad[g * rows_wg + (w * rb_per_wave + rb) * 32:][:32]
                half = []
                for h in range(2):
                    a = np.zeros(c, np.float32)
                    for j in range(16):
                        a = a + blk[16 * h + j]
                    half.append(a)
                red = red + (half[0] + half[1])
            out[g] += red.astype(np.float64)
    return out


@pytest.mark.parametrize("name,cin,cout,K,rows_wg,rbw", TRAIN, ids=[t[0] for t in TRAIN])
def test_conv_epilogue_training_modes(name, cin, cout, K, rows_wg, rbw):
    """epi_mode on the families that carry it, with a second (activated) view and a residual of res_ld > C, 513 rows.  No kernel outside these
    families has the training epilogues, so the reference is what tests/test_gpu_train_fused.py uses: the stored tensors equal the plain
    launch's bit for bit (the first, raw view; an activated view of a training launch is formed from the ROUNDED result and equals the
    one-view training launch of its affine), the fp64 partial rows add up to the column sums of the STORED tensor (1e-6, fp32 partial sums inside a tile) and
    are the same on a second run; TL_EPI_BN_BWD (with a residual and a second, activated view) stores dy masked by the ReLU of the BatchNorm in front.  For
    the stream kernels the first partial row of every workgroup (sum of y, sum of g) is also pinned exactly against a host evaluation in the
    kernels' own order of operations (_stream_partial_sums)."""
    from treelearn_amd import ops
    d = _dev()
    n = 513
    rng = np.random.default_rng(cin + cout + K)
    dtype = torch.bfloat16
    k = round(K ** (1 / 3))
    n_in, table, _ = _rulebook(rng, "table" if K > 1 else "none", K, n)
    x = torch.from_numpy(rng.normal(size=(n_in, cin)).astype(np.float32)).to(d).to(dtype)
    views = _views(rng, cout, d)
    resbuf = torch.from_numpy(rng.normal(size=(n, cout + 8)).astype(np.float32)).to(d).to(dtype)
    res = resbuf[:, :cout]
    tab = None if table is None else torch.from_numpy(np.ascontiguousarray(table.T)).to(d)
    with _small_rows(False):
        w = ops.pack_weight(torch.from_numpy((rng.normal(size=(cout, k, k, k, cin)) / np.sqrt(cin * K * 0.6)).astype(np.float32)).to(d), dtype)
        for residual in (None, res):
            plain = _launch(ops, x, w, tab, n, [views[0], views[1]], cout, dtype, d, residual=residual)
            b0, v0 = _dest(n, cout, dtype, d); b1, v1 = _dest(n, cout, dtype, d)
            r = ops.conv_fwd(x, w, tab, n, out=v0, out2=(v1, views[1][0], views[1][1], True), residual=residual, epi="stats")
            assert r is not None, "this shape is expected on a kernel family with the training epilogue"
            _, parts, nparts = r
            assert _intact(b0, n, cout) and _intact(b1, n, cout)
            assert _same_bits(v0, plain[0])
            b2, v2 = _dest(n, cout, dtype, d)
            r1 = ops.conv_fwd(x, w, tab, n, out=v2, out_scale=views[1][0], out_shift=views[1][1], out_relu=True, residual=residual, epi="stats")
            assert r1 is not None and _intact(b2, n, cout) and _same_bits(v1, v2)
            assert 0 < nparts <= parts.shape[0]
            s = parts[:nparts].sum(0).cpu().numpy()
            y = v0.double().cpu().numpy()
            np.testing.assert_allclose(s[0], y.sum(0), rtol=1e-6, atol=1e-6 * np.abs(y).sum(0).max())
            np.testing.assert_allclose(s[1], (y * y).sum(0), rtol=1e-6)
            r2 = ops.conv_fwd(x, w, tab, n, out=v0, out2=(v1, views[1][0], views[1][1], True), residual=residual, epi="stats")
            assert torch.equal(r2[1][:nparts], parts[:nparts])
            if rows_wg:
                want = _stream_partial_sums(v0.float().cpu().numpy(), n, rows_wg, rbw)
                assert nparts == want.shape[0] and np.array_equal(parts[:nparts, 0].cpu().numpy(), want)
        # TL_EPI_BN_BWD
        xb = torch.from_numpy((rng.normal(size=(n, cout)) * 2 + 0.5).astype(np.float32)).to(d).to(dtype)
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32)).to(d); beta = torch.from_numpy(rng.normal(0, 0.3, cout).astype(np.float32)).to(d)
        st = ops.bn_train_stats(xb, gamma, beta, 1e-4, 0.1)
        dy = ops.conv_fwd(x, w, tab, n, residual=res)
        bg, g = _dest(n, cout, dtype, d); bg2, g2 = _dest(n, cout, dtype, d)
        r = ops.conv_fwd(x, w, tab, n, out=g, out2=(g2, views[1][0], views[1][1], True), residual=res, epi=("bn_bwd", xb, st, True))
        assert r is not None and _intact(bg, n, cout) and _intact(bg2, n, cout)
        _, parts, nparts = r
        keep = (xb.double() * st[2].double() + st[3].double()) > 0
        assert torch.equal(g, torch.where(keep, dy, torch.zeros_like(dy)))
        bg3, g3 = _dest(n, cout, dtype, d)
        r1 = ops.conv_fwd(x, w, tab, n, out=g3, out_scale=views[1][0], out_shift=views[1][1], out_relu=True, residual=res, epi=("bn_bwd", xb, st, True))
        assert r1 is not None and _same_bits(g2, g3)                       # the second view = the one-view launch of its affine
        if rows_wg:
            want = _stream_partial_sums(g.float().cpu().numpy(), n, rows_wg, rbw)
            assert nparts == want.shape[0] and np.array_equal(parts[:nparts, 0].cpu().numpy(), want)
        xhat = (xb.double() - st[0].double()) * st[1].double()
        s = parts[:nparts].sum(0).cpu().numpy()
        gd = g.double()
        np.testing.assert_allclose(s[0], gd.sum(0).cpu().numpy(), rtol=1e-5, atol=1e-6 * float(gd.abs().sum(0).max()))
        np.testing.assert_allclose(s[1], (gd * xhat).sum(0).cpu().numpy(), rtol=1e-5, atol=1e-5 * float((gd * xhat).abs().sum(0).max()))
