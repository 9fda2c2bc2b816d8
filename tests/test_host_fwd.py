"""The cases of tests/fwd_cases.py proved on the CPU, before tests/test_gpu_fwd_exact.py runs a kernel over them:

  * route check: filled as ops.conv_fwd fills them (ops.conv_route on CPU tensors; a block-local case passes a BlockedRulebook of CPU
    tensors -- route mode reads no memory), the arguments of every case at every one of its row counts, under the case's setting of the
    small-level threshold, are served by the instantiation the case claims (the `k_name<...>` part and the `/f16` mark of every launch
    of the route, not the grid); the packed one-hot form goes through test_host_conv_route.conv_args(table="packed");
  * ratchet: the claimed instantiations are exactly those of the non-dgrad entries of the `network` section of
    tests/golden/conv_routes.json, minus fwd_cases.UNREACHED.  A change that adds an instantiation and regenerates the fixture fails here
    until it brings a case;
  * data: Set A of every case is exact in fp32 in any order of summation (fwd_cases.check_exact), every mutant of the reference changes
    Set A's float64 result in every case and row count it applies to and has cases, ROWS are those of the epilogue test, the column form
    of a table may be derived from every geometry a compact case uses, and the reference equals float64 torch (oracle.sparse_ops).
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import fwd_cases as F
from oracle import sparse_ops as osp
from test_host_dgrad import TORCH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.id for c in F.CASES]


# ----------------------------------------------------------------------------------------------- the call, as both test files make it
def insts(route):
    """['k_name<template args>' + '/f16' where marked] of every launch of a route"""
    out = []
    for part in route.split(" + "):
        m = re.match(r"(k_\w+<.*>)(/f16)?<<<", part)
        assert m, route
        out.append(m.group(1) + (m.group(2) or ""))
    return out


def claimed_in(c, route):
    """the route is one launch of the claimed instantiation -- or the two 16-channel launches of the staged-unit kernel for fp32 rows, the
    second of which (the one that adds the residual, where there is one) is the claimed instantiation"""
    parts = insts(route)
    if len(parts) == 2 and c.inst.startswith("k_conv_blk_x3<"):
        return parts[1] == c.inst and parts[0].startswith("k_conv_blk_x3<")
    return parts == [c.inst]


def operands(c, d, dev, table=None, compact=None, blk=None):
    """The tensors of case c over the data d on `dev`: x (a column view of a NaN-filled wider buffer where the case has an input view),
    table [K, n] (`blk`: the BlockedRulebook to pass instead; `compact`: its column form, attached where the case has one), scatter,
    scale / shift, residual (a column view with res_ld > Cout)."""
    dtype = TORCH[c.dt]
    T = lambda a, dt=dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)          # noqa: E731
    o = {}
    if c.in_view:
        off, ld = c.in_view
        wide = torch.full((d.n_in, ld), float("nan"), dtype=dtype, device=dev)
        wide[:, off:off + c.ci] = T(d.x)
        o["wide"], o["x"] = wide, wide[:, off:off + c.ci]
    else:
        o["x"] = T(d.x)
    _, ktab, scatter, _ = c.tables(d.n) if table is None else table
    o["table"] = blk if blk is not None else (None if ktab is None else T(ktab, torch.int32))
    if c.table == "compact" and compact is not None:
        o["table"]._tl_compact = compact
    o["scatter"] = None if scatter is None else T(scatter, torch.int32)
    o["scale"] = None if d.scale is None else T(d.scale, torch.float32)
    o["shift"] = None if d.shift is None else T(d.shift, torch.float32)
    if d.residual is not None:
        rb = torch.zeros((d.n, c.co + 8), dtype=dtype, device=dev)
        rb[:, :c.co] = T(d.residual)
        o["residual"] = rb[:, :c.co]
    return o


def conv_kwargs(c, o, outs, scatter=True):
    """keyword arguments of ops.conv_fwd / ops.conv_route for case c: `outs` = the destination views (one per view of the case)"""
    kw = dict(out=outs[0])
    if c.pro:
        kw.update(in_scale=o["scale"], in_shift=o["shift"], in_relu=True)
    if c.res:
        kw["residual"] = o["residual"]
    for name, t in zip(("out2", "out3"), outs[1:]):
        kw[name] = (t, None, None, False)
    if c.table in ("one_hot", "scatter", "packed"):          # (a packed case through ops.conv_fwd: its [8][n] launch, the one to equal)
        kw["one_hot"] = True
    if c.table == "scatter" and scatter:
        kw["scatter"] = o["scatter"]
    if c.epi:
        kw["epi"] = c.epi
    if c.ones:
        kw["all_ones"] = True
    return kw


def _cpu_weight(c):
    dtype = TORCH[c.dt]
    w = torch.zeros((c.K, c.co, c.ci), dtype=dtype)
    if c.frag:
        w._tl_frag = torch.zeros(c.K * c.co * c.ci, dtype=dtype)
    if c.x3 and c.ci % 32 == 0:
        w._tl_x3 = torch.zeros(c.K * c.co * c.ci, dtype=torch.float32)
    return w


def _cpu_blk(n):
    from treelearn_amd.geometry import BlockedRulebook
    z = lambda *s: torch.zeros(s, dtype=torch.int32)          # noqa: E731
    return BlockedRulebook(n, z(n), z(n), z(n, 4), z(n, 4), z(64), z(32 * n), z(n, 9), z(n))


class _Shapes:
    """stands for the data of a case at n rows where only shapes matter"""

    def __init__(self, c, n):
        self.n, self.n_in = n, c.tables(n)[3]
        self.x = np.zeros((self.n_in, c.ci), np.float32)
        self.scale = self.shift = np.zeros(c.ci, np.float32) if c.pro else None
        self.residual = np.zeros((n, c.co), np.float32) if c.res else None


def cpu_route(c, n):
    from test_gpu_conv_epilogue import _dest, _small_rows
    from treelearn_amd import ops
    if c.table == "packed":                               # table_one_hot = 2: only the C ABI takes it
        from test_host_conv_route import conv_args, route
        with _small_rows(not c.small0):
            rc, r = route(conv_args(c.dt, c.K, c.ci, c.co, n, n_in=c.tables(n)[3], table="packed", frag=c.frag, x3=c.x3, affine=False, out_view=(c.co, 2 * c.co)))
        assert rc == 0, (c.id, n, rc)
        return r
    d = _Shapes(c, n)
    o = operands(c, d, "cpu", compact=torch.zeros((10, n), dtype=torch.int32), blk=_cpu_blk(n) if c.table == "blk" else None)
    outs = [_dest(n, c.co, TORCH[c.dt], "cpu")[1] for _ in range(c.views)]
    with _small_rows(not c.small0):
        return ops.conv_route(o["x"], _cpu_weight(c), o["table"], n, **conv_kwargs(c, o, outs))


# ------------------------------------------------------------------------------------------------------------------------ the routes
@pytest.mark.parametrize("cid", IDS)
def test_route_names_the_claimed_instantiation(cid):
    c = F.BY_ID[cid]
    assert c.inst.endswith("/f16") == (c.dt == "f16")
    for n in c.rows:
        r = cpu_route(c, n)
        assert r and claimed_in(c, r), (cid, n, r)


def golden_fwd_instantiations():
    with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as f:
        net = json.load(f)["network"]
    names = {}
    for key, val in net.items():
        if ".dgrad." not in key and val.startswith("0:k_"):
            for i in insts(val[2:]):
                names.setdefault(i, key)
    return names


def test_ratchet_every_forward_instantiation_of_the_net_has_a_case():
    want = golden_fwd_instantiations()
    assert len(want) > 100
    claimed = {c.inst for c in F.CASES}
    assert set(F.UNREACHED) <= set(want) and not (set(F.UNREACHED) & claimed) and all(F.UNREACHED.values())
    missing = {i: want[i] for i in set(want) - claimed - set(F.UNREACHED)}
    assert not missing, f"instantiations of the net's forward launches without a row-edge case in tests/fwd_cases.py: {missing}"
    assert claimed <= set(want), f"cases that claim an instantiation no launch of the net has: {sorted(claimed - set(want))}"
    # every mode of the fixture is claimed in the mode it occurs in
    for c in F.CASES:
        modes = {k.split("/")[0] for k, v in _net().items() if ".dgrad." not in k and v.startswith("0:k_") and c.inst in insts(v[2:])}
        assert (c.mode in modes) or (c.mode == "f32" and "bf16x3" in modes), (c.id, modes)


def test_coverage_table_of_the_gpu_test_lists_every_case():
    import test_gpu_fwd_exact as G
    for c in F.CASES:
        assert f"[{c.id}]" in G.__doc__ and c.inst.replace("/f16", "") in G.__doc__, c.id


_NET = {}


def _net():
    if not _NET:
        with open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")) as f:
            _NET.update(json.load(f)["network"])
    return _NET


# -------------------------------------------------------------------------------------------------------------------------- the data
def test_rows_are_those_of_the_conv_epilogue_test():
    from test_gpu_conv_epilogue import ROWS
    assert tuple(F.ROWS) == tuple(ROWS)
    for c in F.CASES:
        if c.small0 and c.table != "blk":
            assert tuple(c.rows) == tuple(ROWS), c.id
        assert max(c.rows) < 20000
    assert {n % 64 for n in F.BLK_ROWS} == {1}


@pytest.mark.parametrize("cid", IDS)
def test_set_a_is_exact_and_mutants_are_killed(cid):
    c = F.BY_ID[cid]
    for n in c.rows:
        d = c.set_a(n)
        assert d.n == n and (d.table is None or ((d.table < 0).any() and d.table.shape == (n, c.K)))
        ref = F.check_exact(c, d)
        for m in F.MUTANTS:
            if c.mutant_applies(m, d):
                assert not np.array_equal(d.ref(m), ref), f"{cid} at {n} rows: mutant {m} survives"
        if c.pro:
            assert (d.shift > 0).any() and (d.shift < 0).any() and len(set(np.abs(d.scale))) == 3


def test_every_mutant_has_cases():
    for m in F.MUTANTS:
        k = sum(c.mutant_applies(m, c.set_a(c.rows[-1])) for c in F.CASES)
        assert k >= 3, (m, k)


def test_set_b_is_rounded_to_the_dtype():
    from wgrad_cases import round_to
    for c in F.CASES:
        d = c.set_b(c.rows[0])
        for a in (d.x, d.w) + ((d.residual,) if c.res else ()):
            assert np.array_equal(round_to(a, c.dt), a)
        assert abs(float(np.std(d.w)) * np.sqrt(0.6 * c.K * c.ci) - 1.0) < 0.2


def test_packed_table_decodes_to_the_one_hot_table():
    cs = [c for c in F.CASES if c.table == "packed"]
    assert {c.mode for c in cs} == {"bf16", "f16", "bf16x3"}
    for n in F.ROWS:
        v = cs[0].packed(n).astype(np.int64)
        table = cs[0].tables(n)[0]                               # [n, 8]
        dec = np.full_like(table, -1)
        has = v >= 0
        dec[np.nonzero(has)[0], v[has] & 7] = v[has] >> 3
        assert np.array_equal(dec, table) and v.shape == (n,)
    assert (cs[0].packed(513) < 0).sum() > 10                    # rows without a parent


def test_column_form_may_be_derived_from_the_geometries():
    """tl_rulebook_compact relies on the present dz neighbours of a (dx, dy) column being consecutive rows (tests/test_host_cpu.py)"""
    for n in sorted({n for c in F.CASES if c.table == "compact" for n in c.rows}):
        nbr = F.geometry(F.FINE.get(n, f"fine{n}")).nbr
        for col9 in range(9):
            col = nbr[:, 3 * col9:3 * col9 + 3].astype(np.int64)
            present = col >= 0
            base = np.where(present.any(1), np.where(present, col, np.iinfo(np.int64).max).min(1), -1)
            rank = np.cumsum(present, 1) - present
            np.testing.assert_array_equal(np.where(present, base[:, None] + rank, -1), col)


@pytest.mark.parametrize("cid,n", [("stream-T-27-3-3-1-2-2-F-F-bf16", 33), ("blk-8-F-1-F-T-bf16", 257), ("direct-F-8-1-2-2-8-F-F-F-F-f32", 513)])
def test_reference_equals_float64_torch(cid, n):
    """the reference = the oracle's float64 conv over the same table on pro(x); the inverse case also through oracle.inverse_conv"""
    c = F.BY_ID[cid]
    d = c.set_b(n)
    xp = torch.from_numpy(F.prologue(d.x.astype(np.float64), d.scale, d.shift))
    y = osp.conv_table(xp, torch.from_numpy(d.w.astype(np.float64)), d.table, n)
    assert y.dtype == torch.float64
    np.testing.assert_allclose(d.ref(), y.numpy(), rtol=1e-12, atol=1e-12)
    if c.kind == "inverse":
        g = c.geom(n)
        y2 = osp.inverse_conv(xp, torch.from_numpy(d.w.astype(np.float64)), g.parent, g.coords)
        np.testing.assert_allclose(d.ref(), y2.numpy(), rtol=1e-12, atol=1e-12)
