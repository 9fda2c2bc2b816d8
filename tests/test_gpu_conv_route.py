"""Route mode (tl_conv_route / ops.conv_route: tl_conv_fwd's dispatch with every launch replaced by a record) must not leak into launching:
a route query launches nothing and leaves the next conv_fwd of the same arguments -- on the same thread or on another one meanwhile --
exactly what it was.  The stream-q 64 -> 64 kernel in bf16, reached at 33 and 257 rows by lowering the small-level threshold as
tests/test_gpu_conv_epilogue.py does; helpers, sentinels and the bf16 tolerance against float64 (8e-3) are that file's."""
import threading

import numpy as np
import pytest
import torch

from oracle import sparse_ops as osp

import test_gpu_conv_epilogue as E

pytestmark = pytest.mark.gpu


def test_route_query_then_launch_and_two_threads():
    from treelearn_amd import ops
    d = E._dev()
    dtype, cin, cout, K = torch.bfloat16, 64, 64, 27
    rng = np.random.default_rng(64 * 131 + 64 * 7 + 27)
    rnd = lambda a: torch.from_numpy(a.astype(np.float32)).to(dtype).double().numpy()      # noqa: E731  (the dtype's rounding, as float64)
    w64 = rnd(rng.normal(size=(cout, 3, 3, 3, cin)) / np.sqrt(cin * K * 0.6))

    def case(n_out):
        n_in, table, _ = E._rulebook(rng, "table", K, n_out)
        x64 = rnd(rng.normal(size=(n_in, cin)))
        ref = osp.conv_table(torch.from_numpy(x64), torch.from_numpy(w64), table, n_out).numpy()
        return torch.from_numpy(x64).to(d).to(dtype), torch.from_numpy(np.ascontiguousarray(table.T)).to(d), ref

    with E._small_rows(False):
        wp = ops.pack_weight(torch.from_numpy(w64).float().to(d), dtype)
        # ---- one thread, 33 rows: the query launches nothing, the launch after it is right
        x, tab, ref = case(33)
        buf, view = E._dest(33, cout, dtype, d)
        route = ops.conv_route(x, wp, tab, 33, out=view)
        assert route.startswith("k_conv_streamq<") and " + " not in route, route
        torch.cuda.synchronize()
        assert bool((buf == E.SENT).all()), "a route query wrote to the destination"
        ops.conv_fwd(x, wp, tab, 33, out=view)
        err = E.rel_err(view.double().cpu().numpy(), ref)
        assert err < E.TOL[dtype], err
        assert E._intact(buf, 33, cout), "a store outside the n_out x C destination"

        # ---- two threads, 257 rows: 1000 route queries on one while the other launches 20 times
        x, tab, ref = case(257)
        buf0, view0 = E._dest(257, cout, dtype, d)
        ops.conv_fwd(x, wp, tab, 257, out=view0)
        assert E.rel_err(view0.double().cpu().numpy(), ref) < E.TOL[dtype] and E._intact(buf0, 257, cout)
        want_route = ops.conv_route(x, wp, tab, 257, out=view0)
        qbuf, qview = E._dest(257, cout, dtype, d)
        dests = [E._dest(257, cout, dtype, d) for _ in range(20)]
        torch.cuda.synchronize()
        failures = []

        def query():
            try:
                for _ in range(1000):
                    r = ops.conv_route(x, wp, tab, 257, out=qview)
                    if r != want_route:
                        failures.append(("route", r))
                        return
            except Exception as e:                            # noqa: BLE001  (reported by the main thread)
                failures.append(("query", repr(e)))

        def launch():
            try:
                for _, v in dests:
                    ops.conv_fwd(x, wp, tab, 257, out=v)
                torch.cuda.synchronize()
            except Exception as e:                            # noqa: BLE001
                failures.append(("launch", repr(e)))

        threads = [threading.Thread(target=query), threading.Thread(target=launch)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not failures, failures
        assert bool((qbuf == E.SENT).all()), "a route query wrote to its destination"
        for b, v in dests:
            assert E._same_bits(v, view0), "a launch beside route queries differs from the single-threaded launch"
            assert E._intact(b, 257, cout)
