"""Which kernel tl_conv_fwd's dispatch serves a conv with, pinned without a GPU (tl_conv_route: the same host code with every launch
replaced by a record).  tests/golden/conv_routes.json holds

  network : the full route of every launch the engine (model/engine.py) and the training step (autograd.py / backward.py) issue for the
            32-channel, 7-level net at the level sizes of the config-2 tile, in bf16, fp16, fp32 and bf16x3;
  grid    : per (dtype, K, Cin, Cout) one case count and one SHA-256 over "return code:route" of a few thousand argument combinations
            (row counts on both sides of the small-level thresholds, every table form, weight copies, residual, prologue, views,
            training epilogues, one misalignment at a time, every tl_set_tuning switch off in turn).

A rung of the dispatch moved by mistake changes a layer's kernel -- another speed, other low bits -- and nothing else on the CPU
notices.  The pointers in the arguments are made-up, suitably aligned integers: route mode reads no memory behind them.

When a digest moves:   python tests/test_host_conv_route.py --dump FILE   writes every case with its full route; diff the dumps of the two
checkouts.  The fixture is regenerated deliberately (--write-fixture) with a reviewed diff, when a kernel's template parameters or a
tuning decision change.
"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from treelearn_amd import _hip  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
HEADER = ("Routes of tl_conv_fwd (tests/test_host_conv_route.py).  Regenerated deliberately -- python tests/test_host_conv_route.py "
          "--write-fixture -- with a reviewed diff, when a kernel's template parameters or a tuning decision change "
          "(the convention of tools/conv_epilogue_baseline.txt).")

# rows per level of the config-2 tile (synth.make_tile(**CONFIGS["config2"], seed=0) at voxel 0.1: unique(coords >> level))
LEVEL_N = (1849940, 1105126, 254417, 38447, 6437, 1159, 223)
COMPACT_MIN_ROWS = 65536          # levels of at least this many rows carry the column form of their 27-tap table
DTYPES = {"f32": _hip.TL_F32, "bf16": _hip.TL_BF16, "f16": _hip.TL_F16}
SMALL_ROWS = 16384

# made-up addresses, one 4 GB-spaced region per argument (nothing is read behind them)
_FIELDS = ("in_", "weight", "table", "in_scale", "in_shift", "residual", "out_scale", "out_shift", "out", "out2", "out2_scale", "out2_shift",
           "out3", "out3_scale", "out3_shift", "weight_frag", "table_compact", "red_part", "bn_x", "bn_mean", "bn_rstd", "bn_scale", "bn_shift",
           "blk_unit", "blk_counter", "blk_halo", "blk_lrb", "blk_pmask", "table_scatter", "weight_x3")
ADDR = {f: (i + 1) << 32 for i, f in enumerate(_FIELDS)}


def conv_args(dtype, K, Cin, Cout, n_out, n_in=None, table="plain", frag=False, x3=False, ones=False, residual=None, pro=None, views=1,
              affine=True, epi=0, bad=None, in_view=None, out_view=None, out2_view=None, res_view=None):
    """tl_conv_args as ops.conv_fwd would fill them.  table: none | plain | compact | blk | blk_nn | one_hot | packed | scatter;
    residual: None | "aligned" | "odd_ld"; pro: None | "scale_relu" | "relu"; views: 1 | 2 | 3 | "3no2"; bad: one misalignment;
    *_view = (column offset, row stride) of a column view of a wider buffer."""
    es = 4 if dtype == "f32" else 2
    a = _hip.ConvArgs()
    a.dtype = DTYPES[dtype]; a.K = K; a.Cin = Cin; a.Cout = Cout; a.n_out = n_out; a.n_in = n_out if n_in is None else n_in

    def view(field, ld_field, width, v):
        off, ld = v if v is not None else (0, width)
        setattr(a, field, ADDR[field] + off * es); setattr(a, ld_field, ld)

    view("in_", "in_ld", Cin, in_view)
    view("out", "out_ld", Cout, out_view)
    a.weight = ADDR["weight"]
    if table in ("plain", "compact", "blk_nn", "one_hot", "packed", "scatter"):
        a.table = ADDR["table"]
    if table == "compact":
        a.table_compact = ADDR["table_compact"]
    if table in ("blk", "blk_nn"):
        for f in ("blk_unit", "blk_counter", "blk_halo", "blk_lrb", "blk_pmask"):
            setattr(a, f, ADDR[f])
    a.table_one_hot = {"one_hot": 1, "scatter": 1, "packed": 2}.get(table, 0)
    if table == "scatter":
        a.table_scatter = ADDR["table_scatter"]
    if frag:
        a.weight_frag = ADDR["weight_frag"]
    if x3:
        a.weight_x3 = ADDR["weight_x3"]
    a.in_all_ones = int(ones)
    if residual is not None:
        view("residual", "res_ld", Cout, res_view)
        if residual == "odd_ld":
            a.res_ld = Cout + 4
    if pro == "scale_relu":
        a.in_scale = ADDR["in_scale"]; a.in_shift = ADDR["in_shift"]
    a.in_relu = int(pro is not None)
    if affine:
        a.out_scale = ADDR["out_scale"]; a.out_shift = ADDR["out_shift"]; a.out_relu = 1
    if views in (2, 3):
        view("out2", "out2_ld", Cout, out2_view)
        a.out2_scale = ADDR["out2_scale"]; a.out2_shift = ADDR["out2_shift"]; a.out2_relu = 1
    if views in (3, "3no2"):
        view("out3", "out3_ld", Cout, None)
        a.out3_scale = ADDR["out3_scale"]; a.out3_shift = ADDR["out3_shift"]; a.out3_relu = 1
    a.epi_mode = epi
    if epi:
        a.red_part = ADDR["red_part"]                                   # (red_nparts, the one HOST pointer, stays NULL)
    if epi == _hip.TL_EPI_BN_BWD:
        a.bn_x = ADDR["bn_x"]; a.bn_x_ld = Cout; a.bn_relu = 1
        for f in ("bn_mean", "bn_rstd", "bn_scale", "bn_shift"):
            setattr(a, f, ADDR[f])
    if bad == "in":
        a.in_ += 8
    elif bad == "weight":
        a.weight += 8
    elif bad == "out_ld":
        a.out_ld = Cout + 4
    elif bad == "out_scale" and affine:
        a.out_scale += 4
    elif bad == "in_ld":
        a.in_ld = Cin + 4
    return a


_BUF = ctypes.create_string_buffer(2048)


def route(a):
    """(return code, route) of one tl_conv_args"""
    rc = _hip.lib().tl_conv_route(ctypes.byref(a), _BUF, len(_BUF))
    return rc, _BUF.value.decode()


# ------------------------------------------------------------------------------------------------------------ the network
def network_cases():
    """(name, tl_conv_args) of every conv launch of the net, in the engine's order per mode."""
    out = []
    for mode in ("bf16", "f16", "f32", "bf16x3"):
        dt = "f32" if mode == "bf16x3" else mode
        x3m = mode == "bf16x3"
        blocked_ok = mode != "f32"                     # InferencePlan.supports_blocked

        def W(K, ci, co):                              # the copies ops.pack_weight makes
            return dict(frag=(co % 32 == 0 and ci % 32 == 0 and K > 1), x3=(x3m and ci % 32 == 0))

        def subm_table(li, blocked):
            if blocked and li == 0:
                return "blk"
            return "compact" if LEVEL_N[li] >= COMPACT_MIN_ROWS else "plain"

        def add(tag, name, K, ci, co, n_out, **kw):
            w = W(K, ci, co)
            w.update(kw)
            out.append((f"{mode}/{tag}/{name}", conv_args(dt, K, ci, co, n_out, **w)))

        def res_block(tag, pre, li, C, cin, blocked, last_views, staged=False, cat=False):
            """a residual block cin -> C of level li: conv1, the 1x1 skip conv when cin != C, conv2 (+ residual) with `last_views`"""
            n, t = LEVEL_N[li], subm_table(li, blocked)
            src = (0, 2 * C) if cat else None             # reads the skip concat [n, 2C]
            if cin == 2 * C and t == "blk" and (dt != "f32" or x3m):        # the two input-channel halves on block-local rows
                pro = "scale_relu" if staged else None
                add(tag, pre + ".conv1.lo", 27, 32, 32, n, table=t, pro=pro, affine=False, in_view=(0, 64))
                add(tag, pre + ".conv1.hi", 27, 32, 32, n, table=t, pro=pro, residual="aligned", in_view=(32, 64))
            else:
                add(tag, pre + ".conv1", 27, cin, C, n, table=t, pro="scale_relu" if staged else None, in_view=src)
            if cin != C:
                add(tag, pre + ".skip1x1", 1, cin, C, n, table="none", affine=False, in_view=src)
            add(tag, pre + ".conv2", 27, C, C, n, table=t, residual="aligned", **last_views)

        RAW1 = dict(views=1, affine=False)
        ACT1 = dict(views=1, affine=True)
        RAW_ACT = dict(views=2, affine=False)

        def ublock(tag, li, blocked, staged, top_views):
            C, n = 32 * (li + 1), LEVEL_N[li]
            st = staged and li == 0
            if li == len(LEVEL_N) - 1:
                res_block(tag, f"L{li + 1}.b0", li, C, C, blocked, RAW_ACT)
                res_block(tag, f"L{li + 1}.b1", li, C, C, blocked, top_views)
                return
            res_block(tag, f"L{li + 1}.b0", li, C, C, blocked, RAW1 if st else RAW_ACT, staged=st)
            if st:       # raw into the concat + the activated input of the strided conv
                res_block(tag, f"L{li + 1}.b1", li, C, C, blocked, dict(views=2, affine=False, out_view=(0, 2 * C)), staged=True)
            else:        # raw and activated halves of the concat + the activated input of the strided conv
                res_block(tag, f"L{li + 1}.b1", li, C, C, blocked, dict(views=3, affine=False, out_view=(0, 2 * C), out2_view=(0, 2 * C)))
            add(tag, f"L{li + 1}.down", 8, C, C + 32, LEVEL_N[li + 1], n_in=n, table="plain", **RAW_ACT)
            ublock(tag, li + 1, blocked, staged, ACT1)
            if st:
                add(tag, f"L{li + 1}.up", 8, C + 32, C, n, n_in=LEVEL_N[li + 1], table="scatter", views=1, affine=False, out_view=(C, 2 * C))
            else:
                add(tag, f"L{li + 1}.up", 8, C + 32, C, n, n_in=LEVEL_N[li + 1], table="scatter", views=2, affine=False, out_view=(C, 2 * C),
                    out2_view=(C, 2 * C))
            res_block(tag, f"L{li + 1}.t0", li, C, 2 * C, blocked, RAW1 if st else RAW_ACT, staged=st, cat=True)
            res_block(tag, f"L{li + 1}.t1", li, C, C, blocked, top_views, staged=st)

        forms = [("staged", True, True), ("twoview", True, False)] if blocked_ok else [("plain", False, False)]
        for form, blocked, staged in forms:
            for feats in ("ones", "real"):
                tag = f"{form}.{feats}"
                # the input conv 4 -> 32: all-ones through the presence masks; real features through the canonical table (a blocked geometry
                # carries it beside the units)
                t_in = ("blk" if blocked else "compact") if feats == "ones" else "compact"
                add(tag, "input", 27, 4, 32, LEVEL_N[0], table=t_in, ones=(feats == "ones"), **(RAW1 if staged else RAW_ACT))
                ublock(tag, 0, blocked, staged, RAW1)

        # ---- the training step (16-bit and exact fp32; canonical tables): forward convs that also sum the batch statistics, input-gradient
        # convs over the transposed rulebook with the BatchNorm backward in the epilogue, and the same shapes without an epilogue
        if x3m:
            continue
        for li in range(len(LEVEL_N)):
            C, n = 32 * (li + 1), LEVEL_N[li]
            t = subm_table(li, False)
            for epi, en in ((_hip.TL_EPI_STATS, "stats"), (0, "plain")):
                kw = dict(affine=False, epi=epi)
                add("train", f"L{li + 1}.fwd.{en}.subm", 27, C, C, n, table=t, **kw)
                add("train", f"L{li + 1}.fwd.{en}.subm_res", 27, C, C, n, table=t, residual="aligned", **kw)
                if li + 1 < len(LEVEL_N):
                    add("train", f"L{li + 1}.fwd.{en}.subm_cat", 27, 2 * C, C, n, table=t, **kw)
                    add("train", f"L{li + 1}.fwd.{en}.skip1x1", 1, 2 * C, C, n, table="none", **kw)
                    add("train", f"L{li + 1}.fwd.{en}.down", 8, C, C + 32, LEVEL_N[li + 1], n_in=n, table="plain", **kw)
                    add("train", f"L{li + 1}.fwd.{en}.up", 8, C + 32, C, n, n_in=LEVEL_N[li + 1], table="one_hot", **kw)
            for epi, en in ((_hip.TL_EPI_BN_BWD, "bn_bwd"), (0, "plain")):
                kw = dict(affine=False, epi=epi, frag=False)             # (ops.pack_weight_dgrad: no fragment-order copy)
                add("train", f"L{li + 1}.dgrad.{en}.subm", 27, C, C, n, table=t, **kw)
                if li + 1 < len(LEVEL_N):
                    # C -> 2C: at most 224 transposed output channels per launch (backward.py), else column slices of 128 / 96 / 32
                    step = 2 * C if 2 * C <= 224 else (128 if (2 * C) % 128 == 0 else (96 if (2 * C) % 96 == 0 else 32))
                    add("train", f"L{li + 1}.dgrad.{en}.subm_cat", 27, C, step, n, table=t, out_view=(0, 2 * C), **kw)
                    add("train", f"L{li + 1}.dgrad.{en}.skip1x1", 1, C, step, n, table="none", out_view=(0, 2 * C), **kw)
                    add("train", f"L{li + 1}.dgrad.{en}.down", 8, C + 32, C, n, n_in=LEVEL_N[li + 1], table="one_hot", **kw)
                    add("train", f"L{li + 1}.dgrad.{en}.up", 8, C, C + 32, LEVEL_N[li + 1], n_in=n, table="plain", **kw)
        add("train", "input.fwd.stats", 27, 4, 32, LEVEL_N[0], table="compact", affine=False, epi=_hip.TL_EPI_STATS)
    return out


# ------------------------------------------------------------------------------------------------------------ the grid
N_OUTS = (1, SMALL_ROWS, SMALL_ROWS + 1, 4 * SMALL_ROWS, 4 * SMALL_ROWS + 1, 2_000_000)
KS = (1, 8, 27)
TABLES = {1: ("none", "plain"), 8: ("plain", "one_hot", "packed", "scatter"), 27: ("plain", "compact", "blk", "blk_nn")}
TUNINGS = (("direct", 0), ("direct_oh", 0), ("blk", 0), ("up", 0), ("stream", 0), ("streamq", 0), ("streamq_x3", 0),
           ("small_mode", 1), ("small_mode", 2), ("small_mode", 3))
TUNING_DEFAULTS = {"direct": 1, "direct_oh": 1, "blk": 1, "up": 1, "stream": 1, "streamq": 1, "streamq_x3": 1, "small_mode": 0}
# one departure from the default arguments at a time
VARIANTS = (dict(), dict(ones=True), dict(residual="aligned"), dict(residual="odd_ld"), dict(pro="scale_relu"), dict(pro="relu"),
            dict(views=2), dict(views=3), dict(views="3no2"), dict(affine=False), dict(affine=False, views=2),
            dict(bad="in"), dict(bad="weight"), dict(bad="out_ld"), dict(bad="out_scale"), dict(bad="in_ld"))
TRAIN_VARIANTS = (dict(), dict(residual="aligned"), dict(affine=False), dict(affine=False, residual="aligned"), dict(views=2), dict(pro="scale_relu"),
                  dict(bad="in_ld"))
TUNED_VARIANTS = (dict(), dict(ones=True), dict(affine=False, residual="aligned"))


def channel_pairs():
    pairs = []
    for C in range(32, 225, 32):
        pairs += [(C, C), (2 * C, C), (C, C + 32), (C + 32, C)]
    pairs += [(4, 32), (1, 32), (32, 2), (32, 3), (24, 40), (256, 128), (320, 160), (256, 256)]
    return list(dict.fromkeys(pairs))            # (2C -> C and C + 32 -> C coincide at C = 32, ...)


def grid_slice(dtype, K, Cin, Cout):
    """yields (label, tl_conv_args) of one slice, in the order the digest runs over; tunes the library while it runs (restored at the end)"""
    L = _hip.lib()
    wforms = ((False, False), (True, False), (False, True), (True, True)) if dtype == "f32" else ((False, False), (True, False))

    def n_in_of(table, n_out):
        # a strided conv gathers from the finer level, an inverse conv from the coarser one (ops.conv_fwd: a block-local conv maps the
        # level onto itself)
        return 4 * n_out if (K == 8 and table == "plain") else (max(1, n_out // 4) if K == 8 else n_out)

    try:
        for tuning in (None,) + TUNINGS:
            if tuning is not None:
                assert L.tl_set_tuning(tuning[0].encode(), tuning[1]) == 0
            for n_out in N_OUTS:
                for table in TABLES[K]:
                    for frag, x3 in (wforms if tuning is None else (wforms[0], wforms[-1])):
                        for epi in ((0, 1, 2) if tuning is None else (0, 1)):
                            variants = TUNED_VARIANTS if tuning is not None else (VARIANTS if epi == 0 else TRAIN_VARIANTS)
                            for v in variants:
                                if v.get("ones") and K != 27:
                                    continue
                                label = f"{tuning} n={n_out} {table} frag={int(frag)} x3={int(x3)} epi={epi} {v}"
                                yield label, conv_args(dtype, K, Cin, Cout, n_out, n_in=n_in_of(table, n_out), table=table, frag=frag, x3=x3, epi=epi, **v)
            if tuning is not None:
                L.tl_set_tuning(tuning[0].encode(), TUNING_DEFAULTS[tuning[0]])
    finally:
        for k, v in TUNING_DEFAULTS.items():
            L.tl_set_tuning(k.encode(), v)


def grid_slices():
    for dtype in DTYPES:
        for K in KS:
            for Cin, Cout in channel_pairs():
                yield f"{dtype} K={K} {Cin}->{Cout}", (dtype, K, Cin, Cout)


def slice_digest(key):
    h, n = hashlib.sha256(), 0
    for _, a in grid_slice(*key):
        rc, r = route(a)
        h.update(f"{rc}:{r}\n".encode())
        n += 1
    return [n, h.hexdigest()]


def compute():
    return {"about": HEADER,
            "network": {name: "%d:%s" % route(a) for name, a in network_cases()},
            "grid": {name: slice_digest(key) for name, key in grid_slices()}}


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------ the tests
def test_network_routes():
    """every launch of the net's forward (both level-1 forms, all-ones and real features, four modes) and of the training step"""
    want = _fixture()["network"]
    got = {name: "%d:%s" % route(a) for name, a in network_cases()}
    assert list(got) == list(want)
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, f"{len(diff)} routes moved, e.g. {next(iter(diff.items()))}"
    served = [k for k, v in got.items() if v.startswith("0:k_")]
    assert len(served) > 0.9 * len(got)                        # (the fixture pins kernels, not refusals)


def test_grid_digests():
    """the dispatch over the argument grid, one digest per (dtype, K, Cin, Cout)"""
    want = _fixture()["grid"]
    names = [name for name, _ in grid_slices()]
    assert names == list(want)
    moved = []
    for name, key in grid_slices():
        if slice_digest(key) != want[name]:
            moved.append(name)
    assert not moved, f"{len(moved)} slices moved (python tests/test_host_conv_route.py --dump FILE shows every case): {moved[:8]}"


def test_route_is_per_call_joins_two_launches_and_reports_errors():
    """a second call starts from an empty buffer; the two-launch convs are joined by ' + '; errors come back with an empty route; a buffer
    too small is an error; the float16 compilation of a kernel is marked"""
    a = conv_args("f32", 27, 256, 128, 100000, table="plain", x3=True, affine=False)      # the wide bf16x3 split: two half-width launches
    rc, r = route(a)
    assert rc == 0 and r.count(" + ") == 1 and r.count("k_conv_stream<") == 2
    assert route(a) == (rc, r)
    b = conv_args("f32", 27, 32, 32, 100000, table="blk", x3=True)                           # the staged-unit kernel for fp32 rows: two 16-channel launches
    rc, r = route(b)
    assert rc == 0 and r.count(" + ") == 1 and r.count("k_conv_blk_x3<") == 2
    bad = conv_args("bf16", 27, 32, 32, 1000, table="none")
    assert route(bad) == (_hip.TL_ERR_ARG, "")
    tiny = ctypes.create_string_buffer(8)
    assert _hip.lib().tl_conv_route(ctypes.byref(a), tiny, len(tiny)) == _hip.TL_ERR_ARG     # a route that does not fit is not reported as whole
    f16 = conv_args("f16", 27, 64, 64, 100000, table="plain")
    assert "/f16<<<" in route(f16)[1] and "/f16" not in route(conv_args("bf16", 27, 64, 64, 100000, table="plain"))[1]


def test_ops_conv_route_fills_the_same_arguments():
    """ops.conv_route goes through ops.conv_fwd's argument filling: tensors anywhere, nothing launched"""
    import torch
    from treelearn_amd import ops
    n = 40
    x = torch.zeros((n, 64), dtype=torch.bfloat16); w = torch.zeros((27, 64, 64), dtype=torch.bfloat16)
    table = torch.zeros((27, n), dtype=torch.int32)
    sc = torch.ones(64); sh = torch.zeros(64)
    got = ops.conv_route(x, w, table, n, out_scale=sc, out_shift=sh, out_relu=True)
    want = route(conv_args("bf16", 27, 64, 64, n, table="plain"))
    assert want[0] == 0 and got == want[1] and got.startswith("k_conv_small<")
    assert ops.conv_route(x, w, table, n, epi="stats") == ""             # small levels: no training epilogue, conv_fwd returns None


# ------------------------------------------------------------------------------------------------------------ as a script
def _dump(path):
    with open(path, "w") as f:
        for name, a in network_cases():
            f.write("network %s  %d:%s\n" % ((name,) + route(a)))
        for name, key in grid_slices():
            for label, a in grid_slice(*key):
                f.write("grid %s | %s  %d:%s\n" % ((name, label) + route(a)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        _dump(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "--write-fixture":
        doc = compute()
        with open(FIXTURE, "w") as f:
            f.write("{\n")
            f.write(' "about": %s,\n' % json.dumps(doc["about"]))
            for sec in ("network", "grid"):
                f.write(' "%s": {\n' % sec)
                f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in doc[sec].items()))
                f.write("\n }%s\n" % ("," if sec == "network" else ""))
            f.write("}\n")
    else:
        sys.exit("usage: python tests/test_host_conv_route.py --dump FILE | --write-fixture")
