"""Every kernel instantiation the forward conv launches of the net reach (the non-dgrad routes of the `network` section of
tests/golden/conv_routes.json), launched at the edges of its row tiling on real rulebooks and compared with float64, with NO tolerance
where exactness can be had (tests/fwd_cases.py; its cases are proved on the CPU by tests/test_host_fwd.py).

Per case and row count: ops.conv_route on the very tensors of the call names the claimed instantiation; the launch writes into
sentinel-framed column views (nothing outside the n_out x C destination is touched; an input column view leaves the other half of its
buffer alone); Set A (dyadic) equals round_to(float64 reference, dtype) value for value -- the first differing [row, channel] is
reported --; Set B (gaussian) lies within TOL / TOL_X3 of tests/test_gpu_conv_epilogue.py; a second launch gives the same bits; a table
with its column form gives the bits of the plain table, an inverse conv with its scatter form or over its packed table (launched through
the C ABI: ops.conv_fwd does not offer table_one_hot = 2) those of the gather form over the [8][n] table; a training
launch (epi = "stats") stores the same exact tensor and its partial rows add up to the column sums of the STORED tensor under the 1e-6 of
test_conv_epilogue_training_modes.  Block-local cases build their geometry with build_geometry(blocked=True, blk_min_rows=1) over the
voxel sets of the case list -- 257 rows (n % 64 == 1), 513 rows in a batch of two, and the latter with BLK_HALO_MAX lowered to 26 so that
units split -- and compare in canonical order through o2n.  No instantiation needed a tolerance on Set A.

One comparison has no subject as stated: k_conv_ones27 reads presence masks only, so "its plain-table launch" is another kernel
(k_conv_tinycin), which adds the 27 x Cin products one by one where k_conv_ones27 adds the Cin weights of a tap first.  In 16 bits and on
Set A the two give the same bits (asserted); on Set B in fp32 they differ by one unit in the last place (measured 6.7e-8 of the largest
value at 31 rows), so there the gather kernel's result is held to float64 under TOL like the case's own, and k_conv_ones27 is compared bit
for bit with ITSELF over the two forms it does read, column form and block-local presence masks (test_blk_instantiation, all-ones cases).

Defect found by these cases and fixed with them: k_conv_up (the inverse conv that walks the coarse rows) left fine rows WITHOUT a parent
unwritten -- whatever the destination held stayed there -- where the gather forms store epi(0); the 513-row inverse cases run on a
geometry of odd extent that has such rows (64 of 513).  The kernel now stores zeros through every view for rows whose one-hot table has
no tap present.

Instantiation -> test (16-bit kernels: the bf16 compilation, and `/f16` the IEEE-half one):
  k_conv_ones27<true>, /f16                                                test_blk_instantiation[ones27-T-bf16], [ones27-T-f16]
  k_conv_blk<8, false, 1, false, false>, /f16                              test_blk_instantiation[blk-8-F-1-F-F-bf16], [blk-8-F-1-F-F-f16]
  k_conv_blk<8, false, 1, false, true>, /f16                               test_blk_instantiation[blk-8-F-1-F-T-bf16], [blk-8-F-1-F-T-f16]; as conv1.lo of the
                                                                           split 64 -> 32: [blk-8-F-1-F-T-lo-bf16], [blk-8-F-1-F-T-lo-f16]
  k_conv_blk<8, true, 1, false, false>, /f16                               test_blk_instantiation[blk-8-T-1-F-F-bf16], [blk-8-T-1-F-F-f16]
  k_conv_blk<8, true, 2, false, false>, /f16                               test_blk_instantiation[blk-8-T-2-F-F-bf16], [blk-8-T-2-F-F-f16]
  k_conv_blk<8, true, 3, false, false>, /f16                               test_blk_instantiation[blk-8-T-3-F-F-bf16], [blk-8-T-3-F-F-f16]
  k_conv_blk<8, true, 1, false, true>, /f16 (conv1.hi)                     test_blk_instantiation[blk-8-T-1-F-T-bf16], [blk-8-T-1-F-T-f16]
  k_conv_in4<8, true, false>, /f16                                         test_fwd_instantiation[in4-8-T-F-bf16], [in4-8-T-F-f16]
  k_conv_stream<true, 8, 2, 1, 3, 2, 2, false, false>, /f16                test_fwd_instantiation[stream-T-8-2-1-3-2-2-F-F-bf16], [stream-T-8-2-1-3-2-2-F-F-f16]
  k_conv_streamq<27, 2, 1, 2, 8, 1, 2, 1, false, false>, /f16              test_fwd_instantiation[streamq-27-2-1-2-8-1-2-1-F-F-bf16], [streamq-27-2-1-2-8-1-2-1-F-F-f16]
  k_conv_streamq<8, 3, 1, 2, 8, 1, 2, 1, false, false>, /f16               test_fwd_instantiation[streamq-8-3-1-2-8-1-2-1-F-F-bf16], [streamq-8-3-1-2-8-1-2-1-F-F-f16]
  k_conv_stream<true, 27, 3, 3, 1, 2, 2, false, false>, /f16               test_fwd_instantiation[stream-T-27-3-3-1-2-2-F-F-bf16], [stream-T-27-3-3-1-2-2-F-F-f16]
  k_conv_stream<true, 8, 4, 3, 2, 1, 2, false, false>, /f16                test_fwd_instantiation[stream-T-8-4-3-2-1-2-F-F-bf16], [stream-T-8-4-3-2-1-2-F-F-f16]
  k_conv_streamq<27, 4, 2, 2, 8, 1, 2, 1, false, false>, /f16              test_fwd_instantiation[streamq-27-4-2-2-8-1-2-1-F-F-bf16], [streamq-27-4-2-2-8-1-2-1-F-F-f16]
  k_conv_streamq<27, 4, 2, 2, 8, 1, 2, 2, false, false>, /f16              test_fwd_instantiation[streamq-27-4-2-2-8-1-2-2-F-F-bf16], [streamq-27-4-2-2-8-1-2-2-F-F-f16]
  k_conv_streamq<27, 3, 3, 2, 8, 1, 2, 1, false, false>, /f16              test_fwd_instantiation[streamq-27-3-3-2-8-1-2-1-F-F-bf16], [streamq-27-3-3-2-8-1-2-1-F-F-f16]
  k_conv_streamq<27, 2, 2, 2, 8, 1, 2, 1, false, false>, /f16              test_fwd_instantiation[streamq-27-2-2-2-8-1-2-1-F-F-bf16], [streamq-27-2-2-2-8-1-2-1-F-F-f16]
  k_conv_bf16<4, 2, 2, true>, /f16                                         test_fwd_instantiation[bf16-4-2-2-T-bf16], [bf16-4-2-2-T-f16]
  k_conv_stream<true, 8, 3, 4, 1, 1, 4, true, false>, /f16                 test_fwd_instantiation[stream-T-8-3-4-1-1-4-T-F-bf16], [stream-T-8-3-4-1-1-4-T-F-f16]
  k_conv_up<3, 2, 12>, /f16                                                test_fwd_instantiation[up-3-2-12-bf16], [up-3-2-12-f16]
  k_conv_direct<true, 8, 1, 2, 2, 16, false, false, true, false>, /f16     test_fwd_instantiation[direct-T-8-1-2-2-16-F-F-T-F-bf16], [direct-T-8-1-2-2-16-F-F-T-F-f16]
   ... over the packed one-hot table (table_one_hot = 2)                   test_fwd_instantiation[direct-T-8-1-2-2-16-F-F-T-F-packed-bf16], [direct-T-8-1-2-2-16-F-F-T-F-packed-f16]
  k_conv_direct<true, 1, 3, 6, 1, 8, false, false, false, false>, /f16     test_fwd_instantiation[direct-T-1-3-6-1-8-F-F-F-F-bf16], [direct-T-1-3-6-1-8-F-F-F-F-f16]
  k_conv_direct<true, 1, 2, 4, 1, 16, false, false, false, false>, /f16    test_fwd_instantiation[direct-T-1-2-4-1-16-F-F-F-F-bf16], [direct-T-1-2-4-1-16-F-F-F-F-f16]
  k_conv_direct<true, 1, 1, 2, 1, 16, false, false, false, false>, /f16    test_fwd_instantiation[direct-T-1-1-2-1-16-F-F-F-F-bf16], [direct-T-1-1-2-1-16-F-F-F-F-f16]
  k_conv_small<true, 5, 4, true, false>, /f16 (4065 and 4097 rows)         test_fwd_instantiation[small-T-5-4-T-F-bf16], [small-T-5-4-T-F-f16]
  k_conv_small<true, 1, 8, true, false>, /f16 (ROWS and 2720 rows)         test_fwd_instantiation[small-T-1-8-T-F-bf16], [small-T-1-8-T-F-f16]
  k_conv_small<true, 2, 4, false, false>, /f16                             test_fwd_instantiation[small-T-2-4-F-F-bf16], [small-T-2-4-F-F-f16]
  k_conv_small<true, 1, 4, false, false>, /f16                             test_fwd_instantiation[small-T-1-4-F-F-bf16], [small-T-1-4-F-F-f16]
 training forward, 16-bit:
  k_conv_direct<true, 27, 1, 1, 3, 16, true, true, false, false>, /f16     test_fwd_instantiation[direct-T-27-1-1-3-16-T-T-F-F-bf16], [direct-T-27-1-1-3-16-T-T-F-F-f16]
  k_conv_direct<true, 27, 1, 2, 3, 8, true, true, false, false>, /f16      test_fwd_instantiation[direct-T-27-1-2-3-8-T-T-F-F-bf16], [direct-T-27-1-2-3-8-T-T-F-F-f16]
  k_conv_direct<true, 1, 1, 2, 1, 16, false, true, false, false>, /f16     test_fwd_instantiation[direct-T-1-1-2-1-16-F-T-F-F-bf16], [direct-T-1-1-2-1-16-F-T-F-F-f16]
  k_conv_direct<true, 8, 1, 2, 2, 16, false, true, true, false>, /f16      test_fwd_instantiation[direct-T-8-1-2-2-16-F-T-T-F-bf16], [direct-T-8-1-2-2-16-F-T-T-F-f16]
  k_conv_direct<true, 27, 1, 1, 3, 16, true, false, false, false>, /f16    test_fwd_instantiation[direct-T-27-1-1-3-16-T-F-F-F-bf16], [direct-T-27-1-1-3-16-T-F-F-F-f16]
  k_conv_direct<true, 27, 1, 2, 3, 8, true, false, false, false>, /f16     test_fwd_instantiation[direct-T-27-1-2-3-8-T-F-F-F-bf16], [direct-T-27-1-2-3-8-T-F-F-F-f16]
  k_conv_stream<true, 8, 2, 3, 1, 1, 4, true, false>, /f16                 test_fwd_instantiation[stream-T-8-2-3-1-1-4-T-F-bf16], [stream-T-8-2-3-1-1-4-T-F-f16]
  k_conv_in4<8, true, true>, /f16                                          test_fwd_instantiation[in4-8-T-T-bf16], [in4-8-T-T-f16]
 fp32:
  k_conv_ones27<false>                                                     test_fwd_instantiation[ones27-F-f32] (column form), test_blk_instantiation[ones27-F-blk-f32]
  k_conv_tinycin<float, 4>                                                 test_fwd_instantiation[tinycin-float-4-f32]
  k_conv_direct<false, 27, 1, 1, 2, 8, false, false, false, false>         test_fwd_instantiation[direct-F-27-1-1-2-8-F-F-F-F-f32]
  k_conv_direct<false, 8, 2, 1, 2, 8, false, false, false, false>          test_fwd_instantiation[direct-F-8-2-1-2-8-F-F-F-F-f32]
  k_conv_stream<false, 27, 2, 2, 2, 1, 2, false, false>                    test_fwd_instantiation[stream-F-27-2-2-2-1-2-F-F-f32]
  k_conv_stream<false, 8, 3, 2, 2, 1, 2, false, false>                     test_fwd_instantiation[stream-F-8-3-2-2-1-2-F-F-f32]
  k_conv_stream<false, 27, 3, 3, 1, 1, 2, false, false>                    test_fwd_instantiation[stream-F-27-3-3-1-1-2-F-F-f32]
  k_conv_stream<false, 8, 4, 3, 1, 1, 2, false, false>                     test_fwd_instantiation[stream-F-8-4-3-1-1-2-F-F-f32]
  k_conv_stream<false, 27, 4, 4, 1, 1, 2, false, false>                    test_fwd_instantiation[stream-F-27-4-4-1-1-2-F-F-f32]
  k_conv_stream<false, 8, 3, 4, 1, 1, 2, false, false>                     test_fwd_instantiation[stream-F-8-3-4-1-1-2-F-F-f32]
  k_conv_stream<false, 27, 3, 6, 1, 1, 2, false, false>                    test_fwd_instantiation[stream-F-27-3-6-1-1-2-F-F-f32]
  k_conv_mfma_f32<3>                                                       test_fwd_instantiation[mfma-f32-3-f32]
  k_conv_stream<false, 8, 2, 3, 1, 1, 4, false, false>                     test_fwd_instantiation[stream-F-8-2-3-1-1-4-F-F-f32]
  k_conv_stream<false, 27, 2, 4, 1, 1, 2, false, false>                    test_fwd_instantiation[stream-F-27-2-4-1-1-2-F-F-f32]
  k_conv_direct<false, 1, 2, 4, 1, 8, false, false, false, false>          test_fwd_instantiation[direct-F-1-2-4-1-8-F-F-F-F-f32]
  k_conv_direct<false, 8, 1, 2, 2, 8, false, false, false, false>          test_fwd_instantiation[direct-F-8-1-2-2-8-F-F-F-F-f32]
  k_conv_stream<false, 27, 1, 2, 2, 1, 2, false, false>                    test_fwd_instantiation[stream-F-27-1-2-2-1-2-F-F-f32]
  k_conv_direct<false, 1, 1, 2, 1, 8, false, false, false, false>          test_fwd_instantiation[direct-F-1-1-2-1-8-F-F-F-F-f32]
  k_conv_small<false, 1, 4, true, false> (3265, 4064, 4065, 4097 rows)     test_fwd_instantiation[small-F-1-4-T-F-f32]
  k_conv_small<false, 1, 8, true, false> (ROWS and 2720 rows)              test_fwd_instantiation[small-F-1-8-T-F-f32]
  k_conv_small<false, 2, 4, false, false>                                  test_fwd_instantiation[small-F-2-4-F-F-f32]
  k_conv_small<false, 1, 4, false, false>                                  test_fwd_instantiation[small-F-1-4-F-F-f32]
  k_conv_small<false, 2, 4, true, false> (4097 and 4129 rows)              test_fwd_instantiation[small-F-2-4-T-F-f32]
  k_conv_stream<false, 27, 1, 1, 2, 1, 4, false, false> (training)         test_fwd_instantiation[stream-F-27-1-1-2-1-4-F-F-f32]
  k_conv_stream<false, 8, 2, 1, 2, 1, 4, false, false> (training)          test_fwd_instantiation[stream-F-8-2-1-2-1-4-F-F-f32]
  k_conv_stream<false, 8, 1, 2, 2, 1, 4, false, false> (training)          test_fwd_instantiation[stream-F-8-1-2-2-1-4-F-F-f32]
 bf16x3 (fp32 rows, split-bf16 weights):
  k_conv_blk_x3<8, false, 1> (conv1.lo)                                    test_blk_instantiation[blk-x3-8-F-1-bf16x3]
  k_conv_blk_x3<8, true, 1>                                                test_blk_instantiation[blk-x3-8-T-1-bf16x3]; as conv1.hi of the split 64 -> 32
                                                                           (prologue, residual, columns 32 .. 63 of a 64-wide buffer): [blk-x3-8-T-1-hi-bf16x3]
  k_conv_blk_x3<8, true, 2>                                                test_blk_instantiation[blk-x3-8-T-2-bf16x3]
  k_conv_direct<false, 8, 2, 1, 2, 8, false, false, false, true>           test_fwd_instantiation[direct-F-8-2-1-2-8-F-F-F-T-bf16x3]
  k_conv_streamq<27, 2, 2, 1, 8, 1, 2, 1, true, true>                      test_fwd_instantiation[streamq-27-2-2-1-8-1-2-1-T-T-bf16x3]
  k_conv_stream<false, 8, 3, 2, 1, 1, 4, false, true>                      test_fwd_instantiation[stream-F-8-3-2-1-1-4-F-T-bf16x3]
  k_conv_stream<false, 27, 3, 3, 1, 1, 2, false, true>                     test_fwd_instantiation[stream-F-27-3-3-1-1-2-F-T-bf16x3]
  k_conv_stream<false, 8, 4, 3, 1, 1, 2, false, true>                      test_fwd_instantiation[stream-F-8-4-3-1-1-2-F-T-bf16x3]
  k_conv_stream<false, 27, 4, 4, 1, 1, 2, false, true>                     test_fwd_instantiation[stream-F-27-4-4-1-1-2-F-T-bf16x3]
  k_conv_stream<false, 8, 3, 4, 1, 1, 2, true, true>                       test_fwd_instantiation[stream-F-8-3-4-1-1-2-T-T-bf16x3]
  k_conv_streamq<27, 3, 3, 2, 8, 1, 2, 2, true, false>                     test_fwd_instantiation[streamq-27-3-3-2-8-1-2-2-T-F-bf16x3]
  k_conv_stream<false, 8, 2, 3, 1, 1, 2, true, true>                       test_fwd_instantiation[stream-F-8-2-3-1-1-2-T-T-bf16x3]
  k_conv_streamq<27, 2, 2, 1, 8, 1, 2, 2, true, false>                     test_fwd_instantiation[streamq-27-2-2-1-8-1-2-2-T-F-bf16x3]
  k_conv_direct<false, 1, 2, 4, 1, 8, false, false, false, true>           test_fwd_instantiation[direct-F-1-2-4-1-8-F-F-F-T-bf16x3]
  k_conv_direct<false, 8, 1, 2, 2, 12, false, false, true, true>           test_fwd_instantiation[direct-F-8-1-2-2-12-F-F-T-T-bf16x3]
   ... over the packed one-hot table (table_one_hot = 2)                   test_fwd_instantiation[direct-F-8-1-2-2-12-F-F-T-T-packed-bf16x3]
  k_conv_direct<false, 1, 1, 2, 1, 8, false, false, false, true>           test_fwd_instantiation[direct-F-1-1-2-1-8-F-F-F-T-bf16x3]
  k_conv_small<false, 1, 4, true, true> (3265, 4064, 4065, 4097 rows)      test_fwd_instantiation[small-F-1-4-T-T-bf16x3]
  k_conv_small<false, 1, 8, true, true> (ROWS and 2720 rows)               test_fwd_instantiation[small-F-1-8-T-T-bf16x3]
  k_conv_small<false, 2, 4, true, true> (4097 and 4129 rows)               test_fwd_instantiation[small-F-2-4-T-T-bf16x3]
Unless a row count is named, a case runs at 1 / 31 / 33 / 257 / 513 output rows with the small-level threshold of tl_conv_fwd lowered to 0
(the k_conv_small cases leave it at 16384); block-local cases at 257 and 513 rows.  tests/test_host_fwd.py asserts that every case id
stands in this table.
"""
import numpy as np
import pytest
import torch

import fwd_cases as F
from test_gpu_conv_epilogue import TOL, TOL_X3, _dest, _intact, _pack, _small_rows, rel_err
from test_gpu_dgrad_exact import _exact, _same_bits
from test_host_dgrad import TORCH
from test_host_fwd import claimed_in, conv_kwargs, operands

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _compact_of(tab):
    """the column form i32[10][n] of a 27-tap table on the device (tl_rulebook_compact)"""
    from treelearn_amd import _hip
    n = tab.shape[1]
    ct = torch.empty((10, n), dtype=torch.int32, device=tab.device)
    _hip.check(_hip.lib().tl_rulebook_compact(_hip.ptr(tab), n, _hip.ptr(ct), _hip.stream()), "tl_rulebook_compact")
    return ct


def _launch(c, o, w, n, check_route=True, scatter=True):
    """one launch of case c into sentinel-framed destinations -> (the views' contents, the partial rows of a training launch or None)"""
    from treelearn_amd import ops
    dtype = TORCH[c.dt]
    bufs = [_dest(n, c.co, dtype, DEV) for _ in range(c.views)]
    kw = conv_kwargs(c, o, [v for _, v in bufs], scatter=scatter)
    if check_route:
        route = ops.conv_route(o["x"], w, o["table"], n, **kw)
        assert route and claimed_in(c, route), (c.id, n, route)
    r = ops.conv_fwd(o["x"], w, o["table"], n, **kw)
    parts = None
    if c.epi:
        assert r is not None, "the claimed instantiation carries the training epilogue"
        _, parts, nparts = r
        assert 0 < nparts <= parts.shape[0]
        parts = parts[:nparts].clone()
    for buf, _ in bufs:
        assert _intact(buf, n, c.co), f"{c.id} at {n} rows: a store outside the n_out x C destination"
    if "wide" in o:
        off, ld = c.in_view
        rest = torch.cat([o["wide"][:, :off], o["wide"][:, off + c.ci:]], 1)
        assert bool(torch.isnan(rest).all()), "the other column half of the input's buffer was written"
    return [v.clone(memory_format=torch.contiguous_format) for _, v in bufs], parts


def _launch_packed(c, o, w, n, packed):
    """case c over the packed one-hot table i32[n] (tl_conv_args.table_one_hot = 2), filled as ops.conv_fwd fills the rest"""
    import ctypes
    from treelearn_amd import _hip
    buf, view = _dest(n, c.co, TORCH[c.dt], DEV)
    x = o["x"]
    assert tuple(packed.shape) == (n,) and packed.dtype == torch.int32 and packed.is_contiguous() and c.views == 1 and not (c.res or c.pro or c.epi)
    assert int(packed.max()) >> 3 < x.shape[0]
    a = _hip.ConvArgs()
    a.in_ = x.data_ptr(); a.in_ld = x.stride(0); a.weight = w.data_ptr()
    a.weight_frag = _hip.ptr(getattr(w, "_tl_frag", None)); a.weight_x3 = _hip.ptr(getattr(w, "_tl_x3", None))
    a.table = packed.data_ptr(); a.table_one_hot = 2
    a.n_out = n; a.n_in = x.shape[0]; a.K = c.K; a.Cin = c.ci; a.Cout = c.co; a.dtype = _hip.dtype_code(TORCH[c.dt])
    a.out = view.data_ptr(); a.out_ld = view.stride(0)
    rbuf = ctypes.create_string_buffer(1024)
    _hip.check(_hip.lib().tl_conv_route(ctypes.byref(a), rbuf, len(rbuf)), "tl_conv_route")
    assert claimed_in(c, rbuf.value.decode()), (c.id, n, rbuf.value)
    _hip.check(_hip.lib().tl_conv_fwd(ctypes.byref(a), _hip.stream()), "packed one-hot conv")
    assert _intact(buf, n, c.co), f"{c.id} at {n} rows: a store outside the n_out x C destination"
    return [view.clone(memory_format=torch.contiguous_format)]


def _check(c, got, parts, ref, exact, what):
    dtype = TORCH[c.dt]
    for i, g in enumerate(got):
        assert g.dtype == dtype and tuple(g.shape) == ref.shape
        if exact:
            _exact(g, ref, c.dt, f"{what} view {i}")
        else:
            tol = TOL_X3 if c.x3 else TOL[dtype]
            err = rel_err(g.double().cpu().numpy(), ref)
            print(f"{what} view {i}: Set B rel err {err:.2e} (bound {tol:.1e})")
            assert err < tol, (what, i, err)
    if parts is not None:                                    # the bounds of test_conv_epilogue_training_modes
        s = parts.sum(0).cpu().numpy()
        y = got[0].double().cpu().numpy()
        np.testing.assert_allclose(s[0], y.sum(0), rtol=1e-6, atol=1e-6 * np.abs(y).sum(0).max(), err_msg=what)
        np.testing.assert_allclose(s[1], (y * y).sum(0), rtol=1e-6, err_msg=what)


def _twice(c, o, w, n, ref, exact, what):
    got, parts = _launch(c, o, w, n)
    _check(c, got, parts, ref, exact, what)
    got2, parts2 = _launch(c, o, w, n)
    assert all(_same_bits(a, b) for a, b in zip(got, got2)), f"{what}: the second launch differs"
    assert parts is None or torch.equal(parts, parts2), f"{what}: the partial rows of the second launch differ"
    return got


def _weight(c, d):
    from treelearn_amd import ops
    w = _pack(ops, torch.from_numpy(d.w).to(DEV), TORCH[c.dt], c.x3)
    assert (getattr(w, "_tl_frag", None) is not None) == c.frag
    return w


@pytest.mark.parametrize("cid", [c.id for c in F.CASES if c.table != "blk"])
def test_fwd_instantiation(cid):
    c = F.BY_ID[cid]
    for n in c.rows:
        ct = None
        for name, d in (("A", c.set_a(n)), ("B", c.set_b(n))):
            ref = d.ref()
            what = f"{cid} at {n} rows, Set {name}"
            w = _weight(c, d)
            o = operands(c, d, DEV)
            if c.table == "compact":
                ct = _compact_of(o["table"]) if ct is None else ct
                o["table"]._tl_compact = ct
            with _small_rows(not c.small0):                 # (restores the threshold on the way out)
                if c.table == "packed":
                    pk = torch.from_numpy(c.packed(n)).to(DEV)
                    got = _launch_packed(c, o, w, n, pk)
                    _check(c, got, None, ref, name == "A", what)
                    assert _same_bits(got[0], _launch_packed(c, o, w, n, pk)[0]), f"{what}: the second launch differs"
                    gather, _ = _launch(c, o, w, n)          # the [8][n] table through ops.conv_fwd: the same instantiation
                    assert _same_bits(got[0], gather[0]), f"{what}: the packed table and the [8][n] table differ"
                    continue
                got = _twice(c, o, w, n, ref, name == "A", what)
                if c.table == "compact":
                    plain, _ = _launch(c, operands(c, d, DEV), w, n, check_route=False)
                    if c.ones and c.dt == "f32" and name == "B":
                        # k_conv_ones27<false> has no plain-table launch (it reads presence masks only): without the column form the gather
                        # kernel k_conv_tinycin serves the conv, which adds the 27 x Cin products one by one where k_conv_ones27 adds the Cin
                        # weights of a tap first -- two orders of fp32 summation, the same bits only where sums are exact (Set A).  On Set B
                        # the gather kernel's result is held to float64 like the case's own; measured difference between the two: one unit
                        # in the last place (6.7e-8 of the largest value at 31 rows).  The same kernel over the two forms it does read --
                        # column form and block-local presence masks -- is compared bit for bit in test_blk_instantiation[ones27-F-blk-f32].
                        _check(c, plain, None, ref, False, what + " (plain table: k_conv_tinycin)")
                    else:
                        assert all(_same_bits(a, b) for a, b in zip(got, plain)), f"{what}: the column form and the plain table differ"
                if c.table == "scatter":
                    gather, _ = _launch(c, o, w, n, check_route=False, scatter=False)
                    assert all(_same_bits(a, b) for a, b in zip(got, gather)), f"{what}: the scatter form and the gather form differ"


# ------------------------------------------------------------------------------------------------------------------ block-local rows
_BLK = {}


def _blk_geometry(n, split):
    """The voxel set of the case list's n-row geometry as a block-local level (one point per voxel at unit voxel size) -> (BlockedRulebook,
    g2o: row of the case list's geometry of every canonical row of the built level, the level's canonical table i32[27, n]).  `split`: BLK_HALO_MAX = 26, units split."""
    import treelearn_amd.geometry as G
    if (n, split) not in _BLK:
        g = F.geometry(F.FINE[n])
        cells = g.coords.astype(np.int64)
        nb = int(cells[:, 0].max()) + 1
        pts = torch.from_numpy((cells[:, 1:] + 0.5).astype(np.float32)).to(DEV)
        old = G.BLK_HALO_MAX
        G.BLK_HALO_MAX = 26 if split else old
        try:
            geo = G.build_geometry(pts, torch.from_numpy(cells[:, 0].copy()).to(DEV), nb, 1.0, 2, [64, 64, 64], blocked=True, ref_table=True, blk_min_rows=1)
        finally:
            G.BLK_HALO_MAX = old
        lv = geo.levels[0]
        r = lv.nbr
        assert geo.blocked and isinstance(r, G.BlockedRulebook) and r.n == n == lv.n
        # canonical rows of the built level -> rows of the case list's geometry (the builder shifts every batch item to its own origin)
        got = lv.coords.cpu().numpy().astype(np.int64)
        for b in range(nb):
            got[got[:, 0] == b, 1:] += cells[cells[:, 0] == b, 1:].min(0)
        key = lambda a: ((a[:, 0] * 4096 + a[:, 1]) * 4096 + a[:, 2]) * 4096 + a[:, 3]          # noqa: E731
        order = np.argsort(key(cells))
        g2o = order[np.searchsorted(key(cells)[order], key(got))]
        assert np.array_equal(cells[g2o], got)
        ref_tab = lv.nbr_ref.cpu().numpy().T                                                    # [n, 27] canonical
        want = g.nbr[g2o]
        assert np.array_equal(np.where(ref_tab >= 0, g2o[np.maximum(ref_tab, 0)], -1), want), "the built level's rulebook is not the oracle's"
        nu = int(r.counter[0])
        assert (nu > (n + 63) // 64) if split else (nu >= (n + 63) // 64), (n, split, nu)
        _BLK[n, split] = (geo, r, g2o, lv.nbr_ref)
    return _BLK[n, split][1:]


@pytest.mark.parametrize("cid", [c.id for c in F.CASES if c.table == "blk"])
def test_blk_instantiation(cid):
    c = F.BY_ID[cid]
    assert c.small0 and tuple(c.rows) == F.BLK_ROWS
    for n, split in ((257, False), (513, False), (513, True)):
        r, g2o, canon = _blk_geometry(n, split)
        new = g2o[r.perm.cpu().numpy().astype(np.int64)]            # row of the case list's geometry of every block-local row
        o2n = r.o2n.long()
        for name, d in (("A", c.set_a(n)), ("B", c.set_b(n))):
            ref = d.ref()[g2o]                                      # canonical order of the built level
            what = f"{cid} at {n} rows{' (split units)' if split else ''}, Set {name}"
            dn = F.Data(n=n, n_in=n, x=d.x[new], x_other=None, w=d.w, table=None, scale=d.scale, shift=d.shift,
                        residual=None if d.residual is None else d.residual[new])
            w = _weight(c, d)
            o = operands(c, dn, DEV, blk=r)
            with _small_rows(False):
                got, parts = _launch(c, o, w, n)
                got = [g[o2n] for g in got]
                _check(c, got, None, ref, name == "A", what)
                got2, _ = _launch(c, o, w, n)
                assert all(_same_bits(a, b[o2n]) for a, b in zip(got, got2)), f"{what}: the second launch differs"
                if c.ones:
                    # the same kernel over the other table form it reads: the column form of the level's canonical table, canonical rows
                    tab = canon.contiguous()
                    tab._tl_compact = _compact_of(tab)
                    oc = dict(o, table=tab)
                    from treelearn_amd import ops
                    assert claimed_in(c, ops.conv_route(oc["x"], w, tab, n, **conv_kwargs(c, oc, [_dest(n, c.co, TORCH[c.dt], DEV)[1]])))
                    col, _ = _launch(c, oc, w, n, check_route=False)
                    assert _same_bits(got[0], col[0]), f"{what}: presence masks of the units and the column form differ"
