"""The cases of tests/dgrad_cases.py proved on the CPU, before tests/test_gpu_dgrad_exact.py runs a kernel over them:

  * the reference (scatter over the forward table, the parameter in its own layout) equals float64 torch.autograd through
    oracle.sparse_ops.conv_table / inverse_conv on every geometry;
  * the restatement of what backward.py launches (transposed table, W[k]^T, flipped taps, column slices) equals it exactly on Set A;
  * six mutants of that restatement -- a flip dropped, a transpose dropped, a slice written one slice to the right, the wrong table of the
    child / inv pair, the last row of a partial 32-row block left out, one tap dropped -- each differ from the reference on every case
    they apply to: the inputs can tell a wrong kernel path from a right one;
  * every launch backward.py makes for a case is served by the dispatch (ops.conv_route on CPU tensors), and the kernel names reached
    cover every kernel name of the */train/*.dgrad.* entries of tests/golden/conv_routes.json;
  * conv_backward and bn_conv_backward pass the slice starts and widths the case list records, into the right columns of one buffer.

Kernel families of the dgrad routes and the 513-row cases that reach them (small_rows = the small-level threshold of tl_conv_fwd, 16384 by
default; lowered to 0 through tl_set_tuning, the large-level families serve a few hundred rows):
    k_conv_small      small_rows at its default: every case but those of k_conv_generic and k_conv_tinycin below
    k_conv_direct     small_rows 0: SubM 32 -> 32 (16-bit: with the BatchNorm-backward epilogue on its 27 taps), 1x1 64 -> 32, strided
                      32 -> 64, Linear 32 -> 32; fp32 inverse 64 -> 32
    k_conv_stream     small_rows 0: SubM 96 -> 96 and 64 -> 32, 192 -> 96 as two 96-wide launches (bn_conv_backward), 8 taps 96 -> 128 and
                      128 -> 96, 16-bit inverse 64 -> 32; fp32 also 64 -> 64, 128 -> 128, 256 -> 128 in slices
    k_conv_streamq    small_rows 0, 16-bit: SubM 64 -> 64, 128 -> 128, 128 -> 64, 256 -> 128 in slices of 128
    k_conv_bf16       small_rows 0, 16-bit: SubM 160, 224, 192 -> 96 in one launch, 384 -> 192 in slices of 128, 320 -> 160 and 448 -> 224
                      in slices of 32, 1x1 from 128 -> 64 on, 8 taps 192 -> 224 and 224 -> 192
    k_conv_mfma_f32   small_rows 0, fp32: the shapes k_conv_bf16 serves in 16 bits, and 128 -> 64 / 192 -> 96 in one launch
and, outside the golden dgrad routes (the net has no such layer): k_conv_generic for 288 -> 144 in slices of 96 and for the input conv
4 -> 32 (fp32 and bf16; float16 has no kernel for either: dgrad_cases.UNSERVED), k_conv_tinycin for the heads' 32 -> 3 and 32 -> 2.
test_route_coverage asserts that no family of the golden routes is left unreached; none is.
"""
import json
import os

import numpy as np
import pytest
import torch

import dgrad_cases as C
from oracle import sparse_ops as osp
from wgrad_cases import round_to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
IDS = [c.id for c in C.CASES]


def test_rows_are_those_of_the_conv_epilogue_test():
    from test_gpu_conv_epilogue import ROWS
    assert tuple(C.ROWS) == tuple(ROWS)
    recv = {C.tables(k, C.geometry(g))[3] for k, g in [("subm", n) for n in C.GEOMETRIES if n.startswith("fine")]
            + [("inverse", n) for n in C.GEOMETRIES if n.startswith("coarse")]}
    assert recv == set(ROWS)
    assert all(c.tables()[3] <= 513 for c in C.CASES)


# ----------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", C.GEOMETRIES)
def test_reference_equals_float64_autograd(name):
    """gx of the reference = d(sum(y * gout)) / dx of the oracle's forward conv, float64, for SubM, strided, inverse and 1x1 layers"""
    geom = C.geometry(name)
    rng = np.random.default_rng(len(name))
    for kind, ci, co in (("subm", 5, 3), ("down", 3, 6), ("inverse", 6, 3), ("1x1", 5, 2)):
        table, n_out, _, n_in, _, _ = C.tables(kind, geom)
        K = C.taps(kind)
        k = round(K ** (1 / 3))
        w = rng.normal(size=(co, k, k, k, ci))
        g = rng.normal(size=(n_out, co))
        x = torch.from_numpy(rng.normal(size=(n_in, ci))).requires_grad_(True)
        if kind == "inverse":
            y = osp.inverse_conv(x, torch.from_numpy(w), geom.parent, geom.coords)
        else:
            t = table if table is not None else np.arange(n_out, dtype=np.int32)[:, None]
            y = osp.conv_table(x, torch.from_numpy(w), t, n_out)
        assert y.dtype == torch.float64 and y.shape == (n_out, co)
        (y * torch.from_numpy(g)).sum().backward()
        ref = C.reference(g, w, table, n_in)
        np.testing.assert_allclose(ref, x.grad.numpy(), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------- the restatement and its mutants
@pytest.mark.parametrize("cid", IDS)
def test_restatement_exact_and_mutants_killed(cid):
    c = C.BY_ID[cid]
    g, w = c.set_a()
    table, n_out, t_table, n_in, flip, _ = c.tables()
    ref = C.reference(g, w, table, n_in)
    assert np.abs(ref).max() < 2.0 ** 14 and np.array_equal(ref * 64, np.rint(ref * 64))           # Set A: a multiple of 1/64 under 2^14
    for dt in C.DTYPES:
        r = round_to(ref.astype(np.float32), dt)
        assert np.isfinite(r).all()
    geom = C.geometry(c.geom)
    steps = {c.conv_step} | ({c.bn_step} if c.bn_step else set())
    for step in steps:
        assert np.array_equal(C.transposed_path(g, w, t_table, n_in, flip, step), ref), (cid, step)
        for m in C.MUTANTS:
            if C.mutant_applies(m, c.kind, c.ci, c.co, step, n_in):
                got = C.transposed_path(g, w, t_table, n_in, flip, step, mutant=m, child=geom.child_k)
                assert not np.array_equal(got, ref), f"{cid}: mutant {m} survives (step {step})"
    gb, wb = c.set_b("bf16")                                           # Set B: the restatement within float64 rounding of the reference
    np.testing.assert_allclose(C.transposed_path(gb, wb, t_table, n_in, flip, c.conv_step), C.reference(gb, wb, table, n_in), rtol=1e-12, atol=1e-12)


def test_every_mutant_has_cases():
    for m in C.MUTANTS:
        n = sum(C.mutant_applies(m, c.kind, c.ci, c.co, c.conv_step, c.tables()[3]) for c in C.CASES)
        assert n >= 3, (m, n)


def test_bn_inputs_keep_clear_of_the_relu_kink():
    for c in C.BN_CASES:
        for dt in c.dtypes:
            x, gamma, beta = c.bn_input(dt)
            assert np.abs(C.bn_pre(x, gamma, beta)).min() > C.PRE_MARGIN and np.array_equal(x, round_to(x, dt))


# --------------------------------------------------------------------------------------------------------------------- the routes
def launches(c, entry):
    """[(s0, width)] of the conv launches backward.conv_backward ('conv') or backward.bn_conv_backward ('bn') makes for the case"""
    step = c.conv_step if entry == "conv" else c.bn_step
    return [(s0, step) for s0 in range(0, c.ci, step)]


def routes_of(c, dt, entry, small_default, epi=False):
    """The route of every launch of the case, as ops.conv_route reports it on CPU tensors filled as backward.py fills them: the transposed
    conv has Cin = the layer's Cout and per launch `width` output channels written into a column view of [n_in, Cin of the layer].
    -> list of routes; a launch the dispatch refuses with an error is the string 'error: ...'; '' = no such epilogue (epi only)."""
    from test_gpu_conv_epilogue import _small_rows
    from treelearn_amd import ops
    dtype = TORCH[dt]
    _, n_out, t_table, n_in, _, t_one_hot = c.tables()
    gout = torch.zeros((n_out, c.co), dtype=dtype)
    tab = None if t_table is None else torch.from_numpy(t_table)
    buf = torch.zeros((n_in, c.ci), dtype=dtype)
    xbuf = torch.zeros((n_in, 2 * c.ci), dtype=dtype)
    st = torch.zeros((4, c.ci))
    out = []
    with _small_rows(small_default):
        for s0, w_ in launches(c, entry):
            wsl = torch.zeros((c.K, w_, c.co), dtype=dtype)
            kw = dict(out=buf[:, s0:s0 + w_], one_hot=t_one_hot)
            if epi:
                kw["epi"] = ("bn_bwd", xbuf[:, c.ci + s0:c.ci + s0 + w_], st[:, s0:s0 + w_], True)
            try:
                out.append(ops.conv_route(gout, wsl, tab, n_in, **kw))
            except RuntimeError as e:
                out.append(f"error: {e}")
    return out


def _kernel(route):
    return route.split("<")[0]


def golden_dgrad_kernels():
    with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as f:
        net = json.load(f)["network"]
    names = set()
    for key, val in net.items():
        mode, tag, name = key.split("/")
        if mode in ("bf16", "f16", "f32") and tag == "train" and ".dgrad." in name and val.startswith("0:"):
            names.add(_kernel(val[2:]))
    return names


def test_route_coverage():
    """Every launch of every case is served in every dtype the case lists, at both settings of the small-level threshold (the pairs of
    dgrad_cases.UNSERVED are refused with an error: tests/test_gpu_dgrad_exact.py expects that error from conv_backward), and the
    kernels reached cover the kernel names of the golden dgrad routes."""
    want = golden_dgrad_kernels()
    assert want == {"k_conv_direct", "k_conv_stream", "k_conv_streamq", "k_conv_bf16", "k_conv_small", "k_conv_mfma_f32"}, want
    reached, reached_epi = {}, {}
    for cid, dt in C.UNSERVED:
        assert dt not in C.BY_ID[cid].dtypes
        for small_default in (True, False):
            assert all(r.startswith("error") for r in routes_of(C.BY_ID[cid], dt, "conv", small_default)), (cid, dt)
    for c in C.CASES:
        for dt in c.dtypes:
            for small_default in (True, False):
                for entry in ("conv",) + (("bn",) if c.bn_step else ()):
                    for r in routes_of(c, dt, entry, small_default):
                        assert r.startswith("k_"), (c.id, dt, entry, small_default, r)
                        assert ("/f16<<<" in r) == (dt == "f16"), (c.id, dt, r)
                        reached.setdefault(_kernel(r), []).append((c.id, dt, small_default))
                if c.bn_step:
                    for r in routes_of(c, dt, "bn", small_default, epi=True):
                        assert r == "" or r.startswith("k_"), (c.id, dt, r)
                        if r:
                            reached_epi.setdefault(_kernel(r), []).append((c.id, dt, small_default))
    assert want <= set(reached), f"dgrad kernel families no case reaches: {sorted(want - set(reached))}"
    # the BatchNorm-backward epilogue on k_conv_direct with 27 taps at 32 -> 32, and on the stream families
    assert any(cid.startswith("subm-32to32-") for cid, _, _ in reached_epi.get("k_conv_direct", [])), reached_epi.keys()
    assert {"k_conv_stream", "k_conv_streamq"} <= set(reached_epi), reached_epi.keys()
    # the small-row cases (one channel pair per family) reach the family their pair is there for
    for cid, dt, fam in FAMILY_OF_SMALL_ROW_PAIRS:
        for g in ("fine257", "coarse257b2"):
            if f"{cid}-{g}" in C.BY_ID:
                r = routes_of(C.BY_ID[f"{cid}-{g}"], dt, "conv", False)
                assert all(_kernel(x) == fam for x in r), (cid, dt, r)


# (channel pair, dtype, family that serves it with small_rows = 0) of the cases that run at 1 / 31 / 33 / 257 rows
FAMILY_OF_SMALL_ROW_PAIRS = [
    ("subm-32to32", "bf16", "k_conv_direct"), ("subm-64to64", "bf16", "k_conv_streamq"), ("subm-96to96", "bf16", "k_conv_stream"),
    ("subm-224to224", "bf16", "k_conv_bf16"), ("subm-224to224", "f32", "k_conv_mfma_f32"), ("subm-256to128", "bf16", "k_conv_streamq"),
    ("subm-256to128", "f32", "k_conv_stream"), ("subm-96to96", "f32", "k_conv_stream"),
    ("1x1-64to32", "bf16", "k_conv_direct"), ("down-32to64", "bf16", "k_conv_direct"), ("inverse-64to32", "bf16", "k_conv_stream"),
]


# --------------------------------------------------------------------------------------------------------------- the slice choice
class _Spy:
    """ops.conv_fwd / ops.bn_train_bwd_from_parts / ops.bn_train_bwd / ops.pack_weight_dgrad replaced by recorders (nothing launched)"""

    def __init__(self, monkeypatch, epi_ok=True, refuse_at=None):
        from treelearn_amd import ops
        self.conv, self.parts, self.bwd = [], [], []
        self.epi_ok, self.refuse_at = epi_ok, refuse_at
        monkeypatch.setattr(ops, "conv_fwd", self.conv_fwd)
        monkeypatch.setattr(ops, "bn_train_bwd_from_parts", self.from_parts)
        monkeypatch.setattr(ops, "bn_train_bwd", self.bn_train_bwd)
        monkeypatch.setattr(ops, "pack_weight_dgrad", lambda w, dtype, flip: torch.from_numpy(C.dgrad_weight(w.detach().float().numpy(), flip)).to(dtype))

    def conv_fwd(self, x, w, table, n_out, out=None, one_hot=False, epi=None, **kw):
        assert not kw, kw
        self.conv.append(dict(x=x, w=w, table=table, n_out=n_out, out=out, one_hot=one_hot, epi=epi))
        if out is None:
            out = torch.zeros((n_out, w.shape[1]), dtype=x.dtype)
        if epi is not None:
            if not self.epi_ok or self.refuse_at == len(self.conv) - 1:
                return None
            return out, torch.zeros((1, 2, w.shape[1]), dtype=torch.float64), 1
        return out

    def from_parts(self, x, g, st, parts, nparts, dx_add=None, dx=None, dgb=None):
        self.parts.append(dict(x=x, g=g, st=st, dx_add=dx_add, dx=dx, dgb=dgb))
        return dx, dgb[0], dgb[1]

    def bn_train_bwd(self, x, dy, st, relu, dx_add=None):
        self.bwd.append(dict(x=x, dy=dy, st=st, relu=relu, dx_add=dx_add))
        return torch.zeros_like(x), torch.zeros(x.shape[1]), torch.zeros(x.shape[1])


def _is_columns(view, base, s0, w_):
    """`view` is the columns [s0, s0 + w_) of `base`, sharing its memory"""
    return (tuple(view.shape) == (base.shape[0], w_) and view.stride() == (base.stride(0), 1)
            and view.data_ptr() == base.data_ptr() + s0 * base.element_size() and view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr())


def _ref_of(c):
    from treelearn_amd.backward import TableRef
    table, n_out, t_table, n_in, flip, t_one_hot = c.tables()
    tt = None if t_table is None else torch.from_numpy(t_table)
    return TableRef(None if table is None else torch.from_numpy(np.ascontiguousarray(table.T)), n_out, tt, n_in, flip, t_one_hot=t_one_hot), tt


def _bases(views):
    """the one buffer a list of column views belongs to"""
    ptrs = {v.untyped_storage().data_ptr() for v in views}
    assert len(ptrs) == 1
    return views[0]._base if views[0]._base is not None else views[0]


@pytest.mark.parametrize("cid", [c.id for c in C.CASES if c.geom == C.G])
def test_conv_backward_slices(cid, monkeypatch):
    from treelearn_amd import backward as bw
    c = C.BY_ID[cid]
    spy = _Spy(monkeypatch)
    g, w = c.set_a()
    ref, tt = _ref_of(c)
    weight = torch.from_numpy(w)
    gout = torch.from_numpy(g)
    gx, gw = bw.conv_backward(torch.zeros((ref.n_in, c.ci)), weight, ref, gout, True, False)
    assert gw is None and tuple(gx.shape) == (ref.n_in, c.ci)
    want = launches(c, "conv")
    assert len(spy.conv) == len(want)
    wt = torch.from_numpy(C.dgrad_weight(w, ref.flip))
    for rec, (s0, w_) in zip(spy.conv, want):
        assert rec["x"] is gout and rec["table"] is tt and rec["n_out"] == ref.n_in and rec["one_hot"] == ref.t_one_hot and rec["epi"] is None
        assert rec["w"].is_contiguous() and torch.equal(rec["w"], wt[:, s0:s0 + w_]), (cid, s0)
        if len(want) == 1:
            assert rec["out"] is None
        else:
            assert _is_columns(rec["out"], gx, s0, w_), (cid, s0)
    assert sum(w_ for _, w_ in want) == c.ci and want[0][1] == c.conv_step


@pytest.mark.parametrize("epi_ok", [True, False], ids=["fused", "plain"])
@pytest.mark.parametrize("cid", [c.id for c in C.BN_CASES])
def test_bn_conv_backward_slices(cid, epi_ok, monkeypatch):
    from treelearn_amd import backward as bw
    c = C.BY_ID[cid]
    spy = _Spy(monkeypatch, epi_ok=epi_ok)
    g, w = c.set_a()
    ref, tt = _ref_of(c)
    n = ref.n_in
    wide = torch.zeros((n, 2 * c.ci))
    x = wide[:, c.ci:]
    st = torch.zeros((4, c.ci))
    gskip = torch.zeros((n, c.ci))
    gout = torch.from_numpy(g)
    res = bw.bn_conv_backward(x, torch.zeros((n, c.ci)), st, True, torch.from_numpy(w), ref, gout, False, gskip)
    assert res[3] is None
    want = launches(c, "bn")
    assert want[0][1] == c.bn_step
    wt = torch.from_numpy(C.dgrad_weight(w, ref.flip))
    fused = spy.conv[:len(want)] if epi_ok else spy.conv[:1]
    plain = [] if epi_ok else spy.conv[1:]
    assert len(spy.conv) == (len(want) if epi_ok else 1 + len(want))            # the first refusal ends the fused attempt: the plain launches follow
    for rec, (s0, w_) in zip(fused, want):
        kind, xb, stb, relu = rec["epi"]
        assert kind == "bn_bwd" and relu is True and _is_columns(xb, wide, c.ci + s0, w_) and _is_columns(stb, st, s0, w_)
    for recs in (fused, plain):
        for rec, (s0, w_) in zip(recs, want):
            assert rec["x"] is gout and rec["table"] is tt and rec["n_out"] == n and rec["one_hot"] == ref.t_one_hot
            assert rec["w"].is_contiguous() and torch.equal(rec["w"], wt[:, s0:s0 + w_]), (cid, s0)
        if recs:
            base = _bases([r["out"] for r in recs])
            assert tuple(base.shape) == (n, c.ci)
            for rec, (s0, w_) in zip(recs, want):
                assert _is_columns(rec["out"], base, s0, w_)
    if epi_ok:
        assert len(spy.parts) == len(want) and not spy.bwd
        gbase, dxbase, dgbase = _bases([p["g"] for p in spy.parts]), _bases([p["dx"] for p in spy.parts]), _bases([p["dgb"] for p in spy.parts])
        assert gbase.data_ptr() == _bases([r["out"] for r in fused]).data_ptr() and res[0].data_ptr() == dxbase.data_ptr()
        for p, (s0, w_) in zip(spy.parts, want):
            assert _is_columns(p["x"], wide, c.ci + s0, w_) and _is_columns(p["g"], gbase, s0, w_) and _is_columns(p["st"], st, s0, w_)
            assert _is_columns(p["dx"], dxbase, s0, w_) and _is_columns(p["dx_add"], gskip, s0, w_)
            assert tuple(p["dgb"].shape) == (2, w_) and p["dgb"].data_ptr() == dgbase.data_ptr() + s0 * 4
        assert res[1].data_ptr() == dgbase.data_ptr() and res[2].data_ptr() == dgbase.data_ptr() + c.ci * 4
    else:
        assert not spy.parts and len(spy.bwd) == 1
        b = spy.bwd[0]
        assert b["x"] is x and b["st"] is st and b["relu"] is True and b["dx_add"] is gskip
        assert b["dy"].data_ptr() == _bases([r["out"] for r in plain]).data_ptr() and tuple(b["dy"].shape) == (n, c.ci)


def test_bn_conv_backward_refusal_at_a_later_slice_restarts_on_the_plain_path(monkeypatch):
    """the second of two slices has no epilogue: every slice runs again without it, into a fresh buffer, and tl_bn_train_bwd follows"""
    from treelearn_amd import backward as bw
    c = C.BY_ID[f"subm-256to128-{C.G}"]
    spy = _Spy(monkeypatch, refuse_at=1)
    g, w = c.set_a()
    ref, _ = _ref_of(c)
    n = ref.n_in
    x = torch.zeros((n, c.ci))
    bw.bn_conv_backward(x, x, torch.zeros((4, c.ci)), False, torch.from_numpy(w), ref, torch.from_numpy(g), False, None)
    assert [r["epi"] is not None for r in spy.conv] == [True, True, False, False]
    assert len(spy.parts) == 1 and len(spy.bwd) == 1 and spy.bwd[0]["relu"] is False and spy.bwd[0]["dx_add"] is None
    assert spy.bwd[0]["dy"].data_ptr() == spy.conv[2]["out"].data_ptr()


def test_bn_conv_backward_mixed_dtypes_take_the_plain_path(monkeypatch):
    from treelearn_amd import backward as bw
    c = C.BY_ID[f"subm-64to32-{C.G}"]
    spy = _Spy(monkeypatch)
    g, w = c.set_a()
    ref, _ = _ref_of(c)
    x = torch.zeros((ref.n_in, c.ci))
    bw.bn_conv_backward(x, x, torch.zeros((4, c.ci)), True, torch.from_numpy(w), ref, torch.from_numpy(g).to(torch.bfloat16), False, None)
    assert all(r["epi"] is None for r in spy.conv) and len(spy.conv) == 1 and not spy.parts and len(spy.bwd) == 1
    assert spy.conv[0]["w"].dtype == torch.bfloat16                 # the transposed weights follow grad_out's dtype
