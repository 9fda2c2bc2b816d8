"""The input gradient of every conv layer kind (treelearn_amd/backward.py: tl_conv_fwd over the transposed rulebook with W[k]^T) against float64
on real rulebooks, with NO tolerance where exactness can be had (tests/dgrad_cases.py; its cases are proved on the CPU by
tests/test_host_dgrad.py).

Set A: gout and W = m / 8, |m| <= 8 -> every partial sum of an input-gradient entry is a multiple of 1/64 under 2^14, exact in fp32 in any
order, so gx must equal round_to(float64 reference, dtype) exactly in fp32, bf16 and f16.  Set B: gaussian values rounded to the dtype,
within TOL of tests/test_gpu_conv_epilogue.py (the project's bound for a conv against float64).  The BatchNorm backward behind the fused
path is held to the bounds tests/test_gpu_pointwise_train.py uses for the same kernels (TOL_DX per dtype, 2e-5 for dgamma / dbeta).
No kernel family needed a tolerance on Set A.

Every case runs with the small-level threshold of tl_conv_fwd at its default (16384 rows: k_conv_small serves everything at these sizes)
and lowered to 0 (the large-level families serve a few hundred rows).  Which kernel serves which test -- asserted per launch through
ops.conv_route on the very tensors of the call, against the routes tests/test_host_dgrad.py computes without a GPU:

  kernel family (dgrad routes of golden/conv_routes.json)   test that reaches it (small_rows = 0 unless said otherwise)
  k_conv_small<.., false, false> (no fragment-order copy)   test_conv_backward, every case, small_rows at its default
  k_conv_direct (27 / 8 / 1 taps, plain)                    test_conv_backward[subm-32to32-*], [1x1-64to32-*], [down-32to64-*], [linear-32to32-*]
  k_conv_direct + BatchNorm-backward epilogue, 27 taps      test_bn_conv_backward[subm-32to32-*-bf16 / f16]; 1 tap: [1x1-64to32-*]; 8 taps: [down-32to64-*]
  k_conv_stream                                             test_conv_backward[subm-96to96-*], [subm-64to32-*], [down-96to128-*], [inverse-*]; fp32:
                                                            [subm-64to64-*], [subm-128to128-*], [subm-256to128-*]; with the epilogue: test_bn_conv_backward
                                                            [subm-96to96-*], [subm-192to96-*] (two 96-wide launches), [inverse-64to32-*]
  k_conv_streamq                                            test_conv_backward[subm-64to64-*], [subm-128to128-*], [subm-128to64-*], [subm-256to128-*]
                                                            (16-bit); with the epilogue: test_bn_conv_backward of the same (128 -> 64 as two launches)
  k_conv_bf16<4|6,2,2,true>, K = 27 / 8 / 1                 test_conv_backward[subm-160to160-*], [subm-224to224-*], [subm-192to96-*], [subm-384to192-*],
                                                            [subm-320to160-*], [subm-448to224-*], [1x1-128to64-*] .. [1x1-448to224-*], [down-192to224-*],
                                                            [inverse-224to192-*] (16-bit); no epilogue: test_bn_conv_backward takes the plain path there
  k_conv_mfma_f32<4|6>                                      the same cases in fp32, and [subm-128to64-*-f32], [subm-192to96-*-f32]
  k_conv_blk (block-local level 1)                          test_block_local_level
 outside the golden routes: k_conv_generic [subm-288to144-*], [subm-4to32-*] (fp32, bf16; float16: test_unserved_shapes_raise),
 k_conv_tinycin [linear-32to3-*], [linear-32to2-*] and test_linear_small_backward.
  k_pack_weight_dgrad                                       test_pack_weight_dgrad_bits;  k_pack_batch forms 0 .. 3: test_pack_plan
Row counts 1 / 31 / 33 / 257 on the receiving side run one channel pair per family (test_host_dgrad.FAMILY_OF_SMALL_ROW_PAIRS); everything
else has 513 rows.  An inverse conv's gradient is RECEIVED by the coarse rows; the fine side of those geometries is larger.
"""
import numpy as np
import pytest
import torch

import dgrad_cases as C
from test_gpu_conv_epilogue import TOL, _small_rows, rel_err
from test_gpu_pointwise_train import EPS, TOL_DX, _bn_ref, _relmax
from test_host_dgrad import TORCH, _kernel, launches, routes_of
from wgrad_cases import dyadic, round_to

pytestmark = pytest.mark.gpu

assert EPS == C.BN_EPS
TOL_DGB = 2e-5            # dgamma / dbeta: test_bn_train_bwd_from_parts_on_synthetic_partials, test_bn_backward_every_dtype_pair_and_kernel_form
MOM = 0.1


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH[dt]).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _exact(got, ref, dt, what):
    """got (device tensor) == round_to(ref float64, dt), value for value; reports the first differing [row, channel]"""
    got = got.float().cpu().numpy().astype(np.float64)
    want = round_to(ref.astype(np.float32), dt).astype(np.float64)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    bad = got != want                                             # -0 equals +0, a NaN differs from everything
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ; first at [row, channel] = {i}: got {got[i]!r}, want {want[i]!r}")


_REFS = {}


def _table_ref(c):
    """the case's TableRef with its tables on the device (built once per geometry and kind)"""
    from treelearn_amd.backward import TableRef
    key = (c.kind, c.geom)
    if key not in _REFS:
        table, n_out, t_table, n_in, flip, t_one_hot = c.tables()
        fwd = None if table is None else torch.from_numpy(np.ascontiguousarray(table.T)).cuda()
        tt = fwd if c.kind == "subm" else (None if t_table is None else torch.from_numpy(t_table).cuda())       # (SubM: lv.nbr is its own transpose)
        _REFS[key] = TableRef(fwd, n_out, tt, n_in, flip, one_hot=c.kind == "inverse", t_one_hot=t_one_hot)
    return _REFS[key]


_REF_A = {}


def _set_a(c):
    """Set A of a case and its float64 reference, computed once and shared by the dtypes and tests"""
    if c.id not in _REF_A:
        g, w = c.set_a()
        table, _, _, n_in, _, _ = c.tables()
        ref = C.reference(g, w, table, n_in)
        ref.setflags(write=False)
        _REF_A[c.id] = (g, w, ref)
    return _REF_A[c.id]


def _actual_routes(c, ref, gout, wt, step):
    from treelearn_amd import ops
    buf = torch.empty((ref.n_in, c.ci), dtype=gout.dtype, device="cuda")
    return [ops.conv_route(gout, wt[:, s0:s0 + step].contiguous(), ref.t_table, ref.n_in, out=buf[:, s0:s0 + step], one_hot=ref.t_one_hot)
            for s0 in range(0, c.ci, step)]


def _poisoned_empty(monkeypatch):
    """torch.empty hands out NaN-filled floating tensors: a column no launch wrote shows"""
    orig = torch.empty

    def empty(*a, **kw):
        t = orig(*a, **kw)
        if t.is_floating_point() and t.is_cuda:
            t.fill_(float("nan"))
        return t
    monkeypatch.setattr(torch, "empty", empty)


def _wgrad_alone(x, gout, ref, K, weight):
    from treelearn_amd import ops
    gw = ops.conv_wgrad(x, gout, ref.table, ref.n_out, K, ref_layout=True)
    if not gw._tl_ref_layout:
        gw = gw.permute(1, 0, 2)
    return gw.reshape(weight.shape).to(weight.dtype)


CONV_PARAMS = [pytest.param(c.id, dt, id=f"{c.id}-{dt}") for c in C.CASES for dt in c.dtypes]


# ------------------------------------------------------------------------------------------------------------------- conv_backward
@pytest.mark.parametrize("cid,dt", CONV_PARAMS)
def test_conv_backward(cid, dt, monkeypatch):
    """backward.conv_backward, Set A exactly and Set B within TOL, at both settings of the small-level threshold: the family of every
    launch as the host test computed it; a second call and the call with the weight gradient on the side stream give the same bits;
    that weight gradient equals ops.conv_wgrad called alone; with torch.empty poisoned no column stays unwritten."""
    from treelearn_amd import backward as bw, ops
    c = C.BY_ID[cid]
    ref = _table_ref(c)
    g, w, want = _set_a(c)
    gout, weight = _t(g, dt), _t(w, "f32")
    x = _t(dyadic(np.random.default_rng(c.seed() + 5), (ref.n_in, c.ci)), dt)
    gb, wb = c.set_b(dt)
    want_b = C.reference(gb, wb, c.tables()[0], ref.n_in)
    gout_b, weight_b = _t(gb, dt), _t(wb, "f32")
    wt = ops.pack_weight_dgrad(weight, TORCH[dt], ref.flip)
    gw_alone = _wgrad_alone(x, gout, ref, c.K, weight)
    for small_default in (True, False):
        host = routes_of(c, dt, "conv", small_default)                   # (sets and restores the threshold itself: not inside the block below)
        with _small_rows(small_default):
            routes = _actual_routes(c, ref, gout, wt, c.conv_step)
            assert all(r.startswith("k_") for r in routes) and [_kernel(r) for r in routes] == [_kernel(r) for r in host], (routes, host)
            assert all(("/f16<<<" in r) == (dt == "f16") for r in routes)
            with monkeypatch.context() as m:
                _poisoned_empty(m)
                gx, gw = bw.conv_backward(x, weight, ref, gout, True, False)
            assert gw is None and gx.dtype == TORCH[dt] and tuple(gx.shape) == (ref.n_in, c.ci)
            _exact(gx, want, dt, f"{cid} {dt} small_rows default={small_default}")
            gx2, _ = bw.conv_backward(x, weight, ref, gout, True, False)
            assert _same_bits(gx, gx2), "second call differs"
            gx3, gw3 = bw.conv_backward(x, weight, ref, gout, True, True)
            torch.cuda.synchronize()
            assert _same_bits(gx, gx3), "input gradient differs with the weight gradient on the side stream"
            assert gw3.shape == weight.shape and _same_bits(gw3, gw_alone), "weight gradient differs from ops.conv_wgrad alone"
            gxb, _ = bw.conv_backward(x, weight_b, ref, gout_b, True, False)
            err = rel_err(gxb.float().cpu().numpy(), want_b)
            print(f"{cid} {dt} small_rows default={small_default}: Set B rel err {err:.2e} (bound {TOL[TORCH[dt]]:.1e}) {[_kernel(r) for r in routes]}")
            assert err < TOL[TORCH[dt]], err


@pytest.mark.parametrize("cid,dt", C.UNSERVED)
def test_unserved_shapes_raise(cid, dt):
    """no kernel for the shape in this dtype: a RuntimeError from the dispatch, nothing launched, at both threshold settings"""
    from treelearn_amd import backward as bw
    c = C.BY_ID[cid]
    ref = _table_ref(c)
    g, w, _ = _set_a(c)
    for small_default in (True, False):
        with _small_rows(small_default):
            with pytest.raises(RuntimeError):
                bw.conv_backward(None, _t(w, "f32"), ref, _t(g, dt), True, False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- bn_conv_backward
class _BNSpy:
    """ops.bn_train_bwd_from_parts / ops.bn_train_bwd record their operands and call through"""

    def __init__(self, m):
        from treelearn_amd import ops
        self.parts, self.bwd = [], []
        p0, b0 = ops.bn_train_bwd_from_parts, ops.bn_train_bwd

        def from_parts(x, g, st, parts, nparts, **kw):
            r = p0(x, g, st, parts, nparts, **kw)
            self.parts.append((g, r is not None))
            return r

        def bn_train_bwd(x, dy, st, relu, dx_add=None):
            self.bwd.append((dy, relu))
            return b0(x, dy, st, relu, dx_add=dx_add)
        m.setattr(ops, "bn_train_bwd_from_parts", from_parts)
        m.setattr(ops, "bn_train_bwd", bn_train_bwd)

    def fused_g(self):
        g = self.parts[0][0]
        return g._base if g._base is not None else g


def _bn_setup(x_np, gamma_np, beta_np, dt, relu):
    """x as the right column half of a [n, 2C] buffer (NaN in the left half), st and a = relu?(bn(x)) from the kernels, the float64 mask"""
    from treelearn_amd import ops
    n, ci = x_np.shape
    wide = torch.full((n, 2 * ci), float("nan"), dtype=TORCH[dt], device="cuda")
    wide[:, ci:] = _t(x_np, dt)
    x = wide[:, ci:]
    gamma, beta = _t(gamma_np, "f32"), _t(beta_np, "f32")
    st = ops.bn_train_stats(x, gamma, beta, EPS, MOM)
    a = ops.affine_relu(x, st[2], st[3], relu)
    pre = C.bn_pre(x_np, gamma_np, beta_np)
    assert np.abs(pre).min() > C.PRE_MARGIN
    mask = (pre > 0) if relu else np.ones_like(pre, bool)
    if relu:
        assert np.array_equal((a > 0).cpu().numpy(), mask), "the kernel's ReLU decisions differ from the float64 ones"
    return wide, x, gamma, beta, st, a, mask


def _check_bn(res, x, dy, gskip, gamma, beta, relu, a, dt, what):
    r = _bn_ref(x.contiguous(), dy, gskip, gamma, beta, torch.zeros_like(gamma), torch.ones_like(gamma), relu, a)
    errs = dict(dx=_relmax(res[0], r["dx"]), dgamma=_relmax(res[1], r["dgamma"]), dbeta=_relmax(res[2], r["dbeta"]))
    print(f"{what}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert res[0].dtype == x.dtype and errs["dx"] < TOL_DX[TORCH[dt]] and errs["dgamma"] < TOL_DGB and errs["dbeta"] < TOL_DGB, (what, errs)


BN_PARAMS = [pytest.param(c.id, dt, id=f"{c.id}-{dt}") for c in C.BN_CASES for dt in c.dtypes]


@pytest.mark.parametrize("cid,dt", BN_PARAMS)
def test_bn_conv_backward(cid, dt, monkeypatch):
    """backward.bn_conv_backward behind relu?(bn(x)), x a column half of a wider buffer, with and without gskip, ReLU on and off, at both
    threshold settings.  Whether the fused path runs is what the dispatch answers for the epilogue (routes_of(..., epi=True)): with an
    epilogue for every slice, tl_bn_train_bwd_from_parts runs once per slice and tl_bn_train_bwd never; otherwise the plain path.  The
    masked input gradient g equals round_to(reference) * mask exactly and has the same bits with autograd.FUSE_BN off; dx / dgamma /
    dbeta of both paths against the float64 BatchNorm backward of tests/test_gpu_pointwise_train.py under that file's bounds."""
    from treelearn_amd import autograd, backward as bw
    c = C.BY_ID[cid]
    ref = _table_ref(c)
    gnp, wnp, want = _set_a(c)
    gout, weight = _t(gnp, dt), _t(wnp, "f32")
    x_np, gamma_np, beta_np = c.bn_input(dt)
    n = ref.n_in
    skip = _t(dyadic(np.random.default_rng(c.seed() + 9), (n, c.ci)), dt)
    dy = _t(round_to(want.astype(np.float32), dt), dt)                           # the conv's result as the kernels hold it (Set A: exact)
    nsl = len(launches(c, "bn"))
    for relu in (True, False):
        wide, x, gamma, beta, st, a, mask = _bn_setup(x_np, gamma_np, beta_np, dt, relu)
        want_g = want * mask
        for small_default in (True, False):
            epi_routes = routes_of(c, dt, "bn", small_default, epi=True)
            fused = all(epi_routes)
            with _small_rows(small_default):
                got = {}
                for gskip in (None, skip):
                    for fuse in (True, False):
                        what = f"{cid} {dt} relu={relu} small_rows default={small_default} gskip={gskip is not None} FUSE_BN={fuse}"
                        with monkeypatch.context() as m:
                            spy = _BNSpy(m)
                            m.setattr(autograd, "FUSE_BN", fuse)
                            res = bw.bn_conv_backward(x, a, st, relu, weight, ref, gout, False, gskip)
                        assert res[3] is None
                        if fuse and fused:
                            assert len(spy.parts) == nsl and all(ok for _, ok in spy.parts) and not spy.bwd, (what, epi_routes)
                            g = spy.fused_g()
                            assert tuple(g.shape) == (n, c.ci)
                        else:
                            assert len(spy.bwd) == 1 and spy.bwd[0][1] == relu and len(spy.parts) <= (nsl if fuse else 0), (what, epi_routes)
                            ga = spy.bwd[0][0]
                            _exact(ga, want, dt, what + " (unmasked)")
                            g = torch.where(torch.from_numpy(mask).cuda(), ga, torch.zeros_like(ga))
                        _exact(g, want_g, dt, what)
                        got[gskip is not None, fuse] = g
                        _check_bn(res, x, dy, gskip, gamma, beta, relu, a, dt, what + (" [fused]" if fuse and fused else " [plain]"))
                        assert bool(torch.isnan(wide[:, :c.ci]).all()), "the other column half of x's buffer was written"
                for k in got:
                    assert _same_bits(got[k], got[False, True]), (k, "g differs between the fused and the separate passes")


def test_bn_conv_backward_mixed_dtypes_take_the_plain_path(monkeypatch):
    """x in fp32 behind a bf16 gradient (mixed precision): the plain conv + tl_bn_train_bwd, same exact g, dx in x's dtype"""
    from treelearn_amd import backward as bw
    c = C.BY_ID[f"subm-64to64-{C.G}"]
    ref = _table_ref(c)
    gnp, wnp, want = _set_a(c)
    x_np, gamma_np, beta_np = c.bn_input("f32")
    wide, x, gamma, beta, st, a, mask = _bn_setup(x_np, gamma_np, beta_np, "f32", True)
    assert all(routes_of(c, "bf16", "bn", False, epi=True))                     # the shape has the epilogue: only the dtypes keep it off
    with _small_rows(False):
        with monkeypatch.context() as m:
            spy = _BNSpy(m)
            res = bw.bn_conv_backward(x, a, st, True, _t(wnp, "f32"), ref, _t(gnp, "bf16"), False, None)
    assert not spy.parts and len(spy.bwd) == 1 and spy.bwd[0][0].dtype == torch.bfloat16
    _exact(spy.bwd[0][0], want, "bf16", "mixed dtypes")
    _check_bn(res, x, _t(round_to(want.astype(np.float32), "bf16"), "bf16"), None, gamma, beta, True, a, "f32", "mixed dtypes")


# ---------------------------------------------------------------------------------------------------------------- block-local level
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_block_local_level(dt, monkeypatch):
    """A BlockedRulebook as t_table (the smallest tile of tests/test_gpu_blk.py with the blocked geometry forced on): 32 -> 32 through
    conv_backward on k_conv_blk and 64 -> 32 through conv_backward and bn_conv_backward (two 32-wide launches on k_conv_blk), Set A:
    the same bits as over the plain table of the same rows, and exactly the reference over the canonical table permuted to the
    block-local order."""
    from test_gpu_blk import _batch, _geoms
    from treelearn_amd import backward as bw, ops
    from treelearn_amd.backward import TableRef
    from treelearn_amd.geometry import BlockedRulebook
    can, blk = _geoms(_batch(2.5, [1], n_trees=1), blk_min_rows=1, nn_table=True)
    r = blk.levels[0].nbr
    assert blk.blocked and isinstance(r, BlockedRulebook) and r.nn_table is not None
    n = r.n
    perm = r.perm.long()
    nbr_can = np.ascontiguousarray(can.levels[0].nbr.cpu().numpy().T)             # [n, 27], canonical order
    ref_blk, ref_plain = TableRef(r, n, r, n, True), TableRef(r.nn_table, n, r.nn_table, n, True)
    for ci, co in ((32, 32), (64, 32)):
        rng = np.random.default_rng(ci)
        g_can, w = dyadic(rng, (n, co)), dyadic(rng, (co, 3, 3, 3, ci))
        want = C.reference(g_can, w, nbr_can, n)[perm.cpu().numpy()]
        gout, weight = _t(g_can, dt)[perm].contiguous(), _t(w, "f32")
        wt = ops.pack_weight_dgrad(weight, TORCH[dt], True)
        if ci == 32:
            assert _kernel(ops.conv_route(gout, wt, r, n)) == "k_conv_blk"
        a = bw.conv_backward(None, weight, ref_blk, gout, True, False)[0]
        b = bw.conv_backward(None, weight, ref_plain, gout, True, False)[0]
        assert _same_bits(a, b), f"{ci}->{co}: block-local and plain-table results differ"
        _exact(a, want, dt, f"block-local {ci}->{co} {dt}")
        if ci == 64:
            for s0 in (0, 32):
                assert _kernel(ops.conv_route(gout, wt[:, s0:s0 + 32].contiguous(), r, n)) == "k_conv_blk"
            x_np, gamma_np, beta_np = C.make_bn_input(77, n, ci, dt)
            wide, x, gamma, beta, st, act, mask = _bn_setup(x_np, gamma_np, beta_np, dt, True)
            gs = []
            for ref in (ref_blk, ref_plain):
                with monkeypatch.context() as m:
                    spy = _BNSpy(m)
                    res = bw.bn_conv_backward(x, act, st, True, weight, ref, gout, False, None)
                if ref is ref_blk:
                    assert len(spy.parts) == 2 and all(ok for _, ok in spy.parts) and not spy.bwd      # two 32-wide launches with the epilogue
                g = spy.fused_g() if spy.parts and not spy.bwd else torch.where(torch.from_numpy(mask).cuda(), spy.bwd[0][0], torch.zeros_like(spy.bwd[0][0]))
                _exact(g, want * mask, dt, f"block-local bn 64->32 {dt}")
                _check_bn(res, x, _t(round_to(want.astype(np.float32), dt), dt), None, gamma, beta, True, act, dt, f"block-local bn {dt}")
                gs.append(g)
            assert _same_bits(gs[0], gs[1])


# -------------------------------------------------------------------------------------------------------------------------- packing
PACK_SHAPES = [(32, 27, 32), (40, 27, 24), (3, 1, 32), (2, 1, 32), (32, 27, 4), (64, 8, 32), (32, 1, 64), (5, 8, 7), (128, 27, 256)]      # (Cout, K, Cin)


def _dgrad_layout(w, K, dtype, flip):
    co, ci = w.shape[0], w.shape[-1]
    t = w.reshape(co, K, ci).permute(1, 2, 0)
    if flip:
        t = t.flip(0)
    return t.contiguous().to(dtype)


def _weight(shape, seed):
    co, K, ci = shape
    k = round(K ** (1 / 3))
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((co, k, k, k, ci), generator=gen).cuda()


@pytest.mark.parametrize("dt", C.DTYPES)
def test_pack_weight_dgrad_bits(dt):
    """k_pack_weight_dgrad: [K][Cin][Cout] = w.reshape(Cout, K, Cin).permute(1, 2, 0), taps reversed when flip, cast ONCE -- bit for bit;
    element counts that are no multiple of 4096, 2 / 3 / 4 channels on either side, K = 1, 8, 27"""
    from treelearn_amd import ops
    assert any((co * K * ci) % 4096 for co, K, ci in PACK_SHAPES)
    for i, shape in enumerate(PACK_SHAPES):
        w = _weight(shape, i)
        for flip in (False, True):
            got = ops.pack_weight_dgrad(w, TORCH[dt], flip)
            assert _same_bits(got, _dgrad_layout(w, shape[1], TORCH[dt], flip)), (shape, flip)
            assert _same_bits(got, ops.pack_weight_dgrad(w, TORCH[dt], flip))


@pytest.mark.parametrize("dt", C.DTYPES)
def test_pack_plan(dt):
    """autograd.PackPlan (tl_pack_weights_batch, forms 0 .. 3) over weights of mixed shapes: the same bits as the per-layer pack_weight,
    pack_weight_frag and pack_weight_dgrad; refresh() after an in-place change updates that parameter; a second refresh() with nothing
    changed launches nothing (the plan's sig stands, a poisoned output stays poisoned); a new pack epoch packs again."""
    from treelearn_amd import autograd, ops
    dtype = TORCH[dt]
    convs = [(_weight(s, 20 + i), flip) for i, (s, flip) in enumerate(zip(PACK_SHAPES, [True, True, False, False, True, False, False, False, True]))]
    plan = autograd.PackPlan(convs, dtype)
    assert plan.sig is None and plan.valid_for(convs, dtype)

    def check(which):
        for i in which:
            (w, flip), (pk, fr, dg, fl) = convs[i], plan.out[i]
            one = ops.pack_weight(w, dtype)
            assert fl == flip and _same_bits(pk, one), (i, "packed")
            assert (fr is None) == (getattr(one, "_tl_frag", None) is None) and (fr is None or _same_bits(fr, one._tl_frag)), (i, "frag")
            assert _same_bits(dg, ops.pack_weight_dgrad(w, dtype, flip)) and _same_bits(dg, _dgrad_layout(w, PACK_SHAPES[i][1], dtype, flip)), (i, "dgrad")
    plan.refresh()
    assert plan.sig is not None
    check(range(len(convs)))
    assert sum(fr is not None for _, fr, _, _ in plan.out) >= 3
    for (w, flip), (pk, fr, dg, _) in zip(convs, plan.out):                        # the per-parameter caches are hits now
        assert autograd._packed(w, dtype) is pk and autograd._packed_dgrad(w, dtype, flip) is dg
    before = [dg.clone() for _, _, dg, _ in plan.out]
    with torch.no_grad():
        convs[1][0].mul_(-1.5)
    plan.refresh()
    check(range(len(convs)))
    assert not _same_bits(plan.out[1][2], before[1]) and all(_same_bits(plan.out[i][2], before[i]) for i in range(len(convs)) if i != 1)
    sig = plan.sig
    plan.out[0][2].fill_(7.0)                                                       # nothing changed: nothing launched
    plan.refresh()
    torch.cuda.synchronize()
    assert plan.sig == sig and bool((plan.out[0][2] == 7.0).all())
    autograd.new_pack_epoch()
    plan.refresh()
    assert plan.sig != sig
    check(range(len(convs)))


# ----------------------------------------------------------------------------------------------------------------- autograd wiring
def _odd_view(g):
    """g's values as a column view whose row stride (C + 4) is not divisible by 8"""
    buf = torch.zeros((g.shape[0], g.shape[1] + 4), dtype=g.dtype, device=g.device)
    buf[:, :g.shape[1]] = g
    v = buf[:, :g.shape[1]]
    assert v.stride(0) % 8 != 0
    return v


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_sparse_conv_autograd_slots(dt):
    """autograd.sparse_conv under torch.autograd with every combination of requires_grad on features / weight / residual: each gradient
    in its slot -- features: the exact Set A reference; weight: ops.conv_wgrad alone; residual: grad_out itself -- None elsewhere; a
    grad_out that is a column view with an odd row stride takes the .contiguous() branch and gives the same bits."""
    from treelearn_amd import autograd
    c = C.BY_ID["subm-64to64-fine257"]
    ref = _table_ref(c)
    gnp, wnp, want = _set_a(c)
    gout = _t(gnp, dt)
    x0 = _t(dyadic(np.random.default_rng(3), (ref.n_in, c.ci)), dt)
    first = None
    for rx, rw, rr in [(a, b, r) for a in (True, False) for b in (True, False) for r in (True, False, None) if a or b or r]:
        for view in (False, True):
            x = x0.clone().requires_grad_(rx)
            weight = _t(wnp, "f32").requires_grad_(rw)
            res = None if rr is None else torch.zeros((ref.n_out, c.co), dtype=TORCH[dt], device="cuda").requires_grad_(rr)
            y = autograd.sparse_conv(x, weight, ref, res)
            y.backward(_odd_view(gout) if view else gout)
            torch.cuda.synchronize()
            what = (rx, rw, rr, view)
            assert (x.grad is not None) == rx and (weight.grad is not None) == rw and (res is None or (res.grad is not None) == bool(rr)), what
            if rx:
                _exact(x.grad, want, dt, f"sparse_conv {what}")
                first = first if first is not None else x.grad.clone()
                assert _same_bits(x.grad, first), what
            if rw:
                assert _same_bits(weight.grad, _wgrad_alone(x0, gout, ref, c.K, weight)), what
            if rr:
                assert _same_bits(res.grad, gout), what


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_bn_relu_conv_autograd_slots(dt):
    """autograd.bn_relu_conv under torch.autograd: (dx, dgamma, dbeta, gw, residual gradient) each arrive in their slot with the bits
    backward.bn_conv_backward returns for the same operands (dgamma and dbeta differ, so a swap shows), the residual's gradient is
    grad_out, for every combination of requires_grad; an odd-stride grad_out gives the same bits."""
    from treelearn_amd import autograd, backward as bw
    c = C.BY_ID[f"subm-64to32-{C.G}"]
    ref = _table_ref(c)
    gnp, wnp, _ = _set_a(c)
    gout = _t(gnp, dt)
    x_np, gamma_np, beta_np = c.bn_input(dt)
    with _small_rows(False):
        for rx, rb, rw, rr in [(True, True, True, True), (True, False, False, None), (False, True, False, False), (False, False, True, None),
                               (True, True, False, False), (False, False, False, True)]:
            for view in (False, True):
                bn = torch.nn.BatchNorm1d(c.ci, eps=EPS, momentum=MOM).cuda().train()
                with torch.no_grad():
                    bn.weight.copy_(_t(gamma_np, "f32")); bn.bias.copy_(_t(beta_np, "f32"))
                bn.weight.requires_grad_(rb); bn.bias.requires_grad_(rb)
                x = _t(x_np, dt).requires_grad_(rx)
                weight = _t(wnp, "f32").requires_grad_(rw)
                res = None if rr is None else torch.zeros((ref.n_out, c.co), dtype=TORCH[dt], device="cuda").requires_grad_(rr)
                y = autograd.bn_relu_conv(x, bn, True, weight, ref, residual=res)
                y.backward(_odd_view(gout) if view else gout)
                torch.cuda.synchronize()
                xd = x.detach()
                from treelearn_amd import ops
                st = ops.bn_train_stats(xd, bn.weight.detach(), bn.bias.detach(), EPS, MOM)
                a = ops.affine_relu(xd, st[2], st[3], True)
                dx, dgamma, dbeta, gw = bw.bn_conv_backward(xd, a, st, True, weight.detach(), ref, gout, True, None)
                torch.cuda.synchronize()
                what = (rx, rb, rw, rr, view)
                assert not _same_bits(dgamma, dbeta)
                for got, wanted, on in ((x.grad, dx, rx), (bn.weight.grad, dgamma, rb), (bn.bias.grad, dbeta, rb), (weight.grad, gw, rw)):
                    assert (got is not None) == on, what
                    if on:
                        assert _same_bits(got, wanted), what
                if res is not None:
                    assert (res.grad is not None) == bool(rr) and (not rr or _same_bits(res.grad, gout)), what


@pytest.mark.parametrize("co", [3, 2])
@pytest.mark.parametrize("dt", C.DTYPES)
def test_linear_small_backward(dt, co):
    """autograd.linear_small_f32's backward (the heads' 32 -> 3 / 32 -> 2): the fp32 incoming gradient m / 8 * (1 + e), e below half a unit
    in the last place of x's dtype, is rounded once to that dtype (= m / 8); the input gradient is then exact on Set A and the weight
    gradient equals ops.conv_wgrad alone on the rounded gradient."""
    from treelearn_amd import autograd
    c = C.BY_ID[f"linear-32to{co}-{C.G}"]
    ref = _table_ref(c)
    gnp, wnp, want = _set_a(c)
    e = {"f32": 0.0, "bf16": 2.0 ** -10, "f16": 2.0 ** -13}[dt]
    g32 = (gnp.astype(np.float64) * (1.0 + e)).astype(np.float32)
    assert np.array_equal(round_to(g32, dt), gnp) and (dt == "f32" or not np.array_equal(g32, gnp))
    x0 = _t(dyadic(np.random.default_rng(co), (ref.n_in, 32)), dt)
    x = x0.clone().requires_grad_(True)
    weight = _t(wnp, "f32").requires_grad_(True)
    assert _kernel(routes_of(c, dt, "conv", True)[0]) == "k_conv_tinycin"
    with _small_rows(True):
        y = autograd.linear_small_f32(x, weight)
        assert y is not None and y.dtype == torch.float32 and tuple(y.shape) == (ref.n_in, co)
        y.backward(torch.from_numpy(g32).cuda())
        torch.cuda.synchronize()
    assert x.grad.dtype == TORCH[dt]
    _exact(x.grad, want, dt, f"linear 32->{co} {dt}")
    assert _same_bits(weight.grad, _wgrad_alone(x0, _t(gnp, dt), ref, 1, weight))
