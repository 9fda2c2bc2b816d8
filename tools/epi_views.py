"""What an output view costs: the level-2 / level-3 SubM convs of config 2 (real rulebooks), the same launch with one raw view, one activated
view, + residual, + a second and a third activated view (column views of 2C-wide buffers, as the concat fusion writes them), against what
the bytes of a view cost at 6 TB/s.  python tools/epi_views.py > profiles/<tag>/epi_views.txt"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from treelearn_amd import geometry as G, ops
from treelearn_amd.synth import CONFIGS, make_batch, make_tile

b = make_batch([make_tile(**CONFIGS["config2"], seed=0)])
geom = G.build_geometry(b["coords"].cuda().float(), b["batch_ids"].cuda().long(), 1, 0.1, 7, [500, 500, 1000], blocked=True)


def t(f, n=20, rounds=3):
    """best round mean of n back-to-back launches (ms): the variants of a shape are measured in turn, so clock drift hits all of them alike"""
    f(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / n)
    return best


print(f"{'conv':30s} {'variant':34s} {'ms':>7s} {'+ms vs act':>10s} {'view MB':>8s} {'MB at 6 TB/s, ms':>16s}")
for li, ci, co in ((1, 64, 64), (1, 128, 64), (2, 96, 96), (2, 192, 96)):
    lv = geom.levels[li]
    n = lv.n
    x = torch.randn(n, ci, device="cuda").bfloat16()
    w = ops.pack_weight(torch.randn(co, 3, 3, 3, ci, device="cuda") * 0.05, torch.bfloat16)
    res = torch.randn(n, co, device="cuda").bfloat16()
    out = torch.empty(n, co, device="cuda", dtype=torch.bfloat16)
    wide2 = torch.empty(n, 2 * co, device="cuda", dtype=torch.bfloat16); wide3 = torch.empty_like(wide2)
    aff = [(torch.rand(co, device="cuda") + 0.5, torch.randn(co, device="cuda")) for _ in range(3)]
    v2 = (wide2[:, co:], aff[1][0], aff[1][1], True); v3 = (wide3[:, co:], aff[2][0], aff[2][1], True)
    act = dict(out_scale=aff[0][0], out_shift=aff[0][1], out_relu=True)
    variants = [("1 raw view", {}), ("1 activated view", act), ("act + residual", dict(act, residual=res)),
                ("raw + residual + 2nd act view", dict(residual=res, out2=v2)),
                ("raw + residual + 2nd + 3rd act view", dict(residual=res, out2=v2, out3=v3))]
    mb = n * co * 2 / 1e6
    base = None
    for name, kw in variants:
        ms = t(lambda: ops.conv_fwd(x, w, lv.nbr, n, out=out, **kw))
        if name == "1 activated view":
            base = ms
        d = "" if base is None else f"{ms - base:+10.3f}"
        print(f"l{li + 1} {ci:3d}->{co:3d} n={n:8d}".ljust(30), f"{name:34s} {ms:7.3f} {d:>10s} {mb:8.1f} {mb / 6e3:16.4f}", flush=True)
