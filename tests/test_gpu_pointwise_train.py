"""The kernels BETWEEN the convs of a training step -- BatchNorm statistics / apply / backward (tl_bn.hip), tl_affine_relu, row gather /
scatter-add (tl_rows.hip), the heads' small Linears (tl_linear_small.hip) and the bias gradient -- against plain float64 on the same,
already rounded, inputs, at the shapes, dtypes and views where their dispatch takes another path.  Every case runs twice and asserts
equal bits: these kernels promise determinism.

Which kernel a case reaches is argued from the dispatch conditions in the sources (nothing reports it):
  * launch_apply_v8 (tl_bn.hip) takes a call iff C % 8 == 0, every leading dimension % 8 == 0 and every pointer % 16 == 0; else the
    4-channel k_bn_bwd_apply runs.  View form "v8" (columns 8.. of a buffer 8 wider) keeps the vector kernel, "v4" (columns 4.. of a
    buffer 4 wider) fails ld % 8 (and, for 16-bit rows, pointer % 16) -> the fallback.  C in {4, 12, 36} fails C % 8 in every form.
  * tl_affine_relu: the same conditions choose k_affine_relu_v8 / k_affine_relu.
  * sum_partials' unrolled loop runs when more than 768 partial rows come in, its tail loop for the rest.

Coverage map:
  k_bn_bwd_apply<TX, TG>           test_bn_partition_edges (C in {4, 12, 36} and every case with a 'v4' operand), the '*v4*' cases of
                                   test_bn_backward_every_dtype_pair_and_kernel_form (all seven dtype pairs), test_bn_data_conditions[36]
  k_bn_bwd_apply_v8<XB, GB, MASK>  test_bn_backward_every_dtype_pair_and_kernel_form 'c-c-c' / 'v8-v8-v8' / 'v8-c-c': XB, GB from the pair,
                                   MASK = relu -- (f32|bf16) x (f32|bf16) x relu = the eight instantiations of the bf16 build; (f16, f16),
                                   (f32, f16), (f16, f32) x relu = the six the f16 build serves; MASK = false also from
                                   test_bn_train_bwd_from_parts_on_synthetic_partials (f32, bf16, f16)
  k_affine_relu_v8<0|1|2>          test_affine_relu_vs_float64[dtype-8], [dtype-64], forms 'c' and 'v8'
  k_affine_relu<T>                 the same tests' 'v4' form, and [dtype-12], [dtype-36] in every form
  sum_partials, tail loop only     nparts <= 768 of the two finishing tests, every BatchNorm case of at most 768 blocks
  sum_partials, unrolled loop      nparts in {769, 1024, 1025, 4100}; the n = 1024 * 8 * rl + 1 cases of test_bn_partition_edges (911 to 1024 blocks)
  k_conv_tinycout<T, CO, OF32>     test_linear_small_f32_vs_float64: CO = 1 .. 8, three dtypes (the fp32-result form on 16-bit input included)
  k_conv_tinycout<T, CO>           test_conv_fwd_one_tap_tiny_cout_vs_float64: CO = 1 .. 8 for f32 / bf16 (CO = 8 at Cin = 8 is the tiny-Cin kernel's)
  k_wgrad_tinycout<T, CO>          test_conv_wgrad_one_tap_tiny_cout_vs_float64 [dtype-8|32|256]: CO = 1 .. 4; the row-block cap in
                                   test_conv_wgrad_tiny_cout_past_the_row_block_cap; [dtype-24|40] fall through to k_wgrad
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-4, 0.1
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
# one rounding of the output type, relative to max |reference|: (y, dx) -- the constants of test_bn_train_kernels_vs_torch /
# test_f16_batchnorm_train_kernels_vs_torch and the conv tests
TOL_Y = {F32: 2e-5, BF16: 8e-3, F16: 1.5e-3}
TOL_DX = {F32: 1e-4, BF16: 1e-2, F16: 5e-3}
MANT = {F32: 23, BF16: 7, F16: 10}
EMIN = {F32: -126, BF16: -126, F16: -14}


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _view(t, form):
    """t [n, C] -> (a view holding t's values, its buffer or None): 'c' contiguous, 'v8' / 'v4' = the columns from 8 / 4 on of a NaN-filled
    buffer 8 / 4 columns wider."""
    if form == "c":
        return t.contiguous(), None
    off = 8 if form == "v8" else 4
    buf = torch.full((t.shape[0], t.shape[1] + off), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, off:] = t
    return buf[:, off:], buf


def _pad_untouched(buf, C):
    return buf is None or bool(torch.isnan(buf[:, :buf.shape[1] - C]).all())


def _relmax(a, b):
    """max |a - b| / max(|b|max, 1e-6), b the float64 reference"""
    return float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-6)


def _ulp(v, dt):
    """unit in the last place of dtype dt at |v| (float64 tensor in, float64 out)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** (EMIN[dt] - 1)))
    return torch.ldexp(torch.ones_like(v), (e - 1).clamp_min(EMIN[dt]) - MANT[dt])


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
def _bn_data(n, C, gen, xdt, gdt, add):
    """Well-conditioned on purpose (|mean| / std of a few units at the most, so the plain fp32 bounds apply; conditioning is the subject of
    test_bn_data_conditions): randn * 2 + a column offset, and for n <= 16 rows of alternating sign with magnitude >= 1, so that no column
    of a short matrix has nearly equal values.
    Two rows are a degenerate BatchNorm: the centred g and the xhat term are both +-d, and the exact dx is scale * d * eps / (var + eps).
    With var >> eps that is a cancellation residue 1e-4 the size of its terms, which no fp32 evaluation holds to 1e-4 of ITSELF; the
    two-row cases therefore have a spread of sqrt(eps), where dx is a well-conditioned result (var = 1 .. 4 eps, xhat = 0.7 .. 0.9)."""
    off = torch.randn(C, device="cuda", generator=gen)
    if n == 2:
        sign = torch.tensor([[1.0], [-1.0]], device="cuda")
        x = EPS ** 0.5 * (off + sign * (1.0 + torch.rand((n, C), device="cuda", generator=gen)))
    elif n <= 16:
        sign = (1.0 - 2.0 * (torch.arange(n, device="cuda") % 2)).unsqueeze(1)
        x = off + sign * (1.0 + torch.rand((n, C), device="cuda", generator=gen))
    else:
        x = torch.randn((n, C), device="cuda", generator=gen) * 2.0 + off
    dy = torch.randn((n, C), device="cuda", generator=gen)
    a = torch.randn((n, C), device="cuda", generator=gen).to(xdt) if add else None
    return x.to(xdt), dy.to(gdt), a


def _bn_params(C, gen):
    gamma = torch.rand(C, device="cuda", generator=gen) + 0.5
    beta = torch.randn(C, device="cuda", generator=gen) * 0.3
    rm = torch.randn(C, device="cuda", generator=gen)
    rv = torch.rand(C, device="cuda", generator=gen) + 0.5
    return gamma, beta, rm, rv


def _bn_ours(x, dy, add, gamma, beta, rm, rv, relu):
    from treelearn_amd import ops
    rm, rv = rm.clone(), rv.clone()
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    st = ops.bn_train_stats(x, gamma, beta, EPS, MOM, rm, rv, nbt)
    y = ops.affine_relu(x, st[2], st[3], relu)
    dx, dgamma, dbeta = ops.bn_train_bwd(x, dy, st, relu, dx_add=add)
    return dict(st=st, y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, rm=rm, rv=rv, nbt=nbt)


def _bn_ref(x, dy, add, gamma, beta, rm, rv, relu, y_ours, kink=None):
    """float64 batch_norm + ReLU with the kink pinned: the mask is OUR y > 0 (as test_bn_train_kernels_vs_torch does)"""
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rmd, rvd = rm.double().clone(), rv.double().clone()
    yl = torch.nn.functional.batch_norm(xd, rmd, rvd, gd, bd, True, MOM, EPS)
    if relu:
        mask = (y_ours > 0)
        lim = torch.full_like(yl[0].detach(), 1e-5 * float(yl.detach().abs().max()))                                   # masks differ only at the kink
        assert bool(((torch.relu(yl) - yl * mask).abs().amax(0) < (lim if kink is None else torch.maximum(lim, kink))).all())
        yr = yl * mask.double()
    else:
        yr = yl
    yr.backward(dy.double())
    xdet = xd.detach()
    mean = xdet.mean(0); var = xdet.var(0, unbiased=False)
    dx = xd.grad + (add.double() if add is not None else 0.0)
    return dict(y=yr.detach(), dx=dx, dgamma=gd.grad, dbeta=bd.grad, mean=mean, var=var, rstd=1.0 / torch.sqrt(var + EPS), rm=rmd, rv=rvd)


def _bn_case(n, C, xdt, gdt, relu, add, forms, seed):
    gen = _gen(seed)
    x0, dy0, a0 = _bn_data(n, C, gen, xdt, gdt, add)
    gamma, beta, rm, rv = _bn_params(C, gen)
    (x, xb), (dy, dyb) = _view(x0, forms[0]), _view(dy0, forms[1])
    a, ab = _view(a0, forms[2]) if add else (None, None)
    o = _bn_ours(x, dy, a, gamma, beta, rm, rv, relu)
    o2 = _bn_ours(x, dy, a, gamma, beta, rm, rv, relu)
    for k in ("st", "y", "dx", "dgamma", "dbeta", "rm", "rv"):
        assert torch.equal(o[k], o2[k]), f"{k} differs between two runs"
    assert _pad_untouched(xb, C) and _pad_untouched(dyb, C) and _pad_untouched(ab, C)
    assert torch.equal(x, x0) and torch.equal(dy, dy0)
    assert o["y"].dtype == xdt and o["dx"].dtype == xdt and int(o["nbt"]) == 1
    r = _bn_ref(x0, dy0, a0, gamma, beta, rm, rv, relu, o["y"])
    err = dict(y=_relmax(o["y"], r["y"]), dx=_relmax(o["dx"], r["dx"]), dgamma=_relmax(o["dgamma"], r["dgamma"]), dbeta=_relmax(o["dbeta"], r["dbeta"]),
               mean=_relmax(o["st"][0], r["mean"]), rstd=_relmax(o["st"][1], r["rstd"]), rm=_relmax(o["rm"], r["rm"]), rv=_relmax(o["rv"], r["rv"]))
    print(f"bn n={n} C={C} x={NAME[xdt]} dy={NAME[gdt]} relu={relu} add={add} forms={forms}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    bound = dict(y=TOL_Y[xdt], dx=TOL_DX[xdt], dgamma=2e-5, dbeta=2e-5, mean=2e-5, rstd=2e-5, rm=2e-5, rv=2e-5)
    bad = {k: (v, bound[k]) for k, v in err.items() if not v < bound[k]}
    assert not bad, bad


PAIRS = [(F32, F32), (BF16, BF16), (F16, F16), (F32, BF16), (BF16, F32), (F32, F16), (F16, F32)]
FORMS = ("c", "v8", "v4")


def _bn_shape_cases():
    cases = []
    for C in (4, 12, 36, 96, 520, 1024):
        rl = 256 // (C // 4)
        ns = sorted({m for m in (2, rl - 1, rl, 8 * rl, 8 * rl + 1, 1024 * 8 * rl + 1) if m >= 2})      # (n = 1: torch refuses it; test_bn_kernel_level)
        cases += [(n, C) for n in ns]
    out = []
    for i, (n, C) in enumerate(cases):
        xdt, gdt = PAIRS[i % 7]
        out.append(pytest.param(n, C, xdt, gdt, (i // 2) % 2 == 0, (i // 4) % 2 == 0, (FORMS[i % 3], FORMS[(i // 3) % 3], FORMS[(i // 9 + i) % 3]), i,
                                id=f"n{n}-C{C}-{NAME[xdt]}-{NAME[gdt]}-{i}"))
    return out


@pytest.mark.parametrize("n,C,xdt,gdt,relu,add,forms,seed", _bn_shape_cases())
def test_bn_partition_edges(n, C, xdt, gdt, relu, add, forms, seed):
    """partition()'s edges in k_bn_stats / k_bn_bwd_reduce: cg = C / 4 from 1 (C = 4, 256 row lanes) to 256 (C = 1024, one row lane), cg
    that does not divide 256 (C = 12, 36, 96, 520: idle threads), n below the row lanes, at and one past the single-block size 8 * rl,
    one past the 1024-block cap; dtype pairs, ReLU, dx_add and the three view forms rotate over the cases.  C % 8 != 0 or a 'v4' operand
    -> k_bn_bwd_apply, else k_bn_bwd_apply_v8."""
    _bn_case(n, C, xdt, gdt, relu, add, forms, 1000 + seed)


@pytest.mark.parametrize("forms", [("c", "c", "c"), ("v8", "v8", "v8"), ("v4", "v4", "v4"), ("c", "v8", "v4"), ("v8", "c", "c")], ids="-".join)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("xdt,gdt", PAIRS, ids=lambda d: NAME[d])
def test_bn_backward_every_dtype_pair_and_kernel_form(xdt, gdt, relu, forms):
    """C = 64, n = 1031 (five workgroups of the vector kernel): with every operand 'c' or 'v8' the call reaches
    k_bn_bwd_apply_v8<XB, GB, MASK> with XB / GB = x / dy 16-bit and MASK = relu -- the pairs (f32|bf16) x (f32|bf16) x relu are the eight
    instantiations of the bf16 build, the pairs with f16 the six mixed and 16-bit ones the f16 build serves; with a 'v4' operand it reaches
    k_bn_bwd_apply<TX, TG> of the same build."""
    add = forms != ("c", "c", "c") or relu
    _bn_case(1031, 64, xdt, gdt, relu, add, forms, 7 + PAIRS.index((xdt, gdt)))


def test_bn_mixed_16_bit_types_raise():
    from treelearn_amd import ops
    gen = _gen(5)
    x, dy, _ = _bn_data(64, 32, gen, BF16, F16, False)
    gamma, beta, _, _ = _bn_params(32, gen)
    st = ops.bn_train_stats(x, gamma, beta, EPS, MOM)
    with pytest.raises(RuntimeError):
        ops.bn_train_bwd(x, dy, st, True)
    with pytest.raises(RuntimeError):
        ops.bn_train_bwd(dy, x, st, False)


# Measured on an MI355X, max over the column.  c = error in units of 2^-24 * |mean| / std * size of the term (the derived bound is c = 8);
# err/bound = error over the asserted max(fp32 bound, derived bound).
#   C = 32 (k_bn_bwd_apply_v8)   |mean|/std = 989:  dx c = 0.46, y c = 0.04, dgamma c = 0.002   (err/bound 0.002, 0.006, < 0.001)
#   C = 36 (k_bn_bwd_apply)      |mean|/std = 992:  dx c = 0.22, y c = 0.13, dgamma c = 0.006   (err/bound 0.001, 0.016, 0.001)
#   |mean|/std = 30: the cancelling term is a small part of dx there, so its error is the ordinary fp32 rounding of the other terms and
#   sits under the fp32 bound, not the derived one: err/bound 0.001 (C = 32) and 0.002 (C = 36); in the derived term's units that is
#   c = 54 and c = 28, which is why the assertion takes the maximum of the two bounds.
# The vector form's fused coefficients cost a factor of two over (x - mean) * rstd at |mean|/std = 1000 and stay 17 times under c = 8.
@pytest.mark.parametrize("C", [32, 36])
def test_bn_data_conditions(C):
    """fp32, n = 4097, C = 32 (vector kernel) and 36 (4-channel kernel): a zero column (a dead channel), columns constant at 1 and -0.5,
    columns with |mean| / std = 30 and 1000 among ordinary ones.  Bounds PER COLUMN (a constant column's dx is 1 / sqrt(eps) = 100 times
    larger than its neighbours': a dx bound relative to the matrix maximum would hide them).
    Constant columns: var exactly 0 (running_var with momentum 1 takes the value), rstd = 1 / sqrt(eps).
    Ill-conditioned columns: the mean is stored in fp32 and x enters an fp32 fma, so y, dx and dgamma carry an error of at most
    c * 2^-24 * |mean| / std times the size of the cancelling term, c = 8: the term is gamma * xhat for y, scale * xhat * dgamma / n for dx
    and sum |g * xhat| for dgamma.  y, dgamma and dbeta are held against the matrix maximum, dx per column."""
    from treelearn_amd import ops
    n = 4097
    gen = _gen(40 + C)
    x = torch.randn((n, C), device="cuda", generator=gen) * 2.0 + torch.randn(C, device="cuda", generator=gen)
    ZERO, ONE, MHALF, R30, R1000 = 1, 2, 5, 9, 14
    x[:, ZERO] = 0.0; x[:, ONE] = 1.0; x[:, MHALF] = -0.5
    x[:, R30] = 30.0 + torch.randn(n, device="cuda", generator=gen)
    x[:, R1000] = -1000.0 + torch.randn(n, device="cuda", generator=gen)
    dy = torch.randn((n, C), device="cuda", generator=gen)
    gamma, beta, rm, rv = _bn_params(C, gen)
    o = _bn_ours(x, dy, None, gamma, beta, rm, rv, True)
    o2 = _bn_ours(x, dy, None, gamma, beta, rm, rv, True)
    for k in ("st", "y", "dx", "dgamma", "dbeta", "rm", "rv"):
        assert torch.equal(o[k], o2[k]), k
    xd = x.double()
    mean_d, var_d = xd.mean(0), xd.var(0, unbiased=False)
    ratio = torch.where(var_d > 0, mean_d.abs() / torch.sqrt(var_d).clamp_min(1e-30), torch.zeros_like(var_d))
    cond = 8.0 * 2.0 ** -24 * ratio
    xhat = (xd - mean_d) / torch.sqrt(var_d + EPS)
    t_y = gamma.double().abs() * xhat.abs().amax(0)
    r = _bn_ref(x, dy, None, gamma, beta, rm, rv, True, o["y"], kink=cond * t_y)      # (our y is that far from the reference's: so is its kink)
    # constant columns
    rv1 = torch.full((C,), 3.0, device="cuda"); rm1 = torch.zeros(C, device="cuda")
    st1 = ops.bn_train_stats(x, gamma, beta, EPS, 1.0, rm1, rv1)
    rs_eps = np.float32(1.0) / np.sqrt(np.float32(EPS))
    for c in (ZERO, ONE, MHALF):
        assert float(rv1[c]) == 0.0, (c, float(rv1[c]))
        assert abs(float(st1[1, c]) - float(rs_eps)) <= float(np.spacing(rs_eps)), (c, float(st1[1, c]))
        assert float(o["st"][0, c]) == float(x[0, c])
        assert float(o["dgamma"][c]) == 0.0                                     # xhat = 0 exactly in both kernels
    # bounds: y and dx per column, dgamma / dbeta against the matrix maximum
    mask = (o["y"] > 0).double()
    g = dy.double() * mask
    scale = gamma.double() * r["rstd"]
    colmax = lambda t: t.abs().amax(0).clamp_min(1e-6)                       # noqa: E731
    e_y = (o["y"].double() - r["y"]).abs().amax(0)
    e_dx = (o["dx"].double() - r["dx"]).abs().amax(0)
    e_dg = (o["dgamma"].double() - r["dgamma"]).abs()
    e_db = (o["dbeta"].double() - r["dbeta"]).abs()
    t_dx = (scale * r["dgamma"] / n).abs() * xhat.abs().amax(0)
    t_dg = (g * xhat).abs().sum(0)
    b_y = torch.maximum(2e-5 * r["y"].abs().max().clamp_min(1e-6), cond * t_y)
    b_dx = torch.maximum(1e-4 * colmax(r["dx"]), cond * t_dx)
    b_dg = torch.maximum(2e-5 * r["dgamma"].abs().max().clamp_min(1e-6), cond * t_dg)
    b_db = (2e-5 * r["dbeta"].abs().max().clamp_min(1e-6)).expand_as(e_db)
    for c in (R30, R1000):                                                       # c: in units of 2^-24 * |mean| / std * term
        print(f"bn conditions C={C} |mean|/std={float(ratio[c]):.0f}: dx c={float(e_dx[c] / (cond[c] / 8 * t_dx[c])):.2f} err/bound={float(e_dx[c] / b_dx[c]):.3f}  "
              f"dgamma c={float(e_dg[c] / (cond[c] / 8 * t_dg[c])):.3f} err/bound={float(e_dg[c] / b_dg[c]):.3f}  "
              f"y c={float(e_y[c] / (cond[c] / 8 * t_y[c])):.2f} err/bound={float(e_y[c] / b_y[c]):.3f}")
    for name, e, b in (("y", e_y, b_y), ("dx", e_dx, b_dx), ("dgamma", e_dg, b_dg), ("dbeta", e_db, b_db)):
        bad = torch.nonzero(~(e <= b)).flatten().tolist()
        assert not bad, (name, [(c, float(e[c]), float(b[c])) for c in bad])
    assert _relmax(o["st"][0], r["mean"]) < 2e-5 and float(((o["st"][1].double() - r["rstd"]).abs() / r["rstd"]).max()) < 2e-5


def test_bn_kernel_level():
    """n = 1 (torch refuses it): mean = x, var = 0, running_var moves toward 0 with the biased value; ld % 4, C % 4 and C = 1028 are refused."""
    from treelearn_amd import ops
    gen = _gen(3)
    C = 36
    x = torch.randn((1, C), device="cuda", generator=gen)
    gamma, beta, rm, rv = _bn_params(C, gen)
    rm0, rv0 = rm.clone(), rv.clone()
    st = ops.bn_train_stats(x, gamma, beta, EPS, MOM, rm, rv)
    rs = np.float32(1.0) / np.sqrt(np.float32(EPS))
    assert torch.equal(st[0], x[0])
    assert float((st[1] - float(rs)).abs().max()) <= float(np.spacing(rs))
    assert _relmax(rm, (0.9 * rm0.double() + 0.1 * x[0].double())) < 2e-5
    assert _relmax(rv, 0.9 * rv0.double()) < 2e-5
    assert _relmax(st[2], gamma.double() * float(rs)) < 2e-5
    ok = lambda n, c: _bn_params(c, gen)[:2] + (torch.randn((n, c), device="cuda", generator=gen),)      # noqa: E731
    g6, b6, x6 = ok(64, 6)
    with pytest.raises(RuntimeError):
        ops.bn_train_stats(x6, g6, b6, EPS, MOM)                              # C % 4
    g8, b8, x8 = ok(64, 10)
    with pytest.raises(RuntimeError):
        ops.bn_train_stats(x8[:, :8], g8[:8], b8[:8], EPS, MOM)               # ld = 10
    gw, bw, xw = ok(16, 1028)
    with pytest.raises(RuntimeError):
        ops.bn_train_stats(xw, gw, bw, EPS, MOM)                              # C > 1024
    st8 = ops.bn_train_stats(x8[:, :8].contiguous(), g8[:8], b8[:8], EPS, MOM)
    with pytest.raises(RuntimeError):
        ops.bn_train_bwd(x8[:, :8], x8[:, :8].contiguous(), st8, True)       # ld = 10
    with pytest.raises(RuntimeError):
        ops.bn_train_bwd(x8[:, :8].contiguous(), x8[:, 2:10], st8, True)     # dy: ld = 10


@pytest.mark.parametrize("entry", ["stats", "bwd", "from_parts"])
def test_bn_entry_points_refuse_a_column_stride(entry):
    """A transposed (or column-strided) operand would be read as if its columns were adjacent: ValueError before any launch."""
    from treelearn_amd import ops
    gen = _gen(11)
    C, n = 32, 40
    x = torch.randn((n, C), device="cuda", generator=gen)
    xt = torch.randn((C, n), device="cuda", generator=gen).t()
    wide = torch.randn((n, 2 * C), device="cuda", generator=gen)[:, ::2]
    gamma, beta, _, _ = _bn_params(C, gen)
    st = ops.bn_train_stats(x, gamma, beta, EPS, MOM)
    parts = torch.zeros((4, 2, C), dtype=torch.float64, device="cuda")
    if entry == "stats":
        calls = [lambda: ops.bn_train_stats(xt, gamma, beta, EPS, MOM), lambda: ops.bn_train_stats(wide, gamma, beta, EPS, MOM)]
    elif entry == "bwd":
        calls = [lambda: ops.bn_train_bwd(xt, x, st, True), lambda: ops.bn_train_bwd(x, xt, st, True), lambda: ops.bn_train_bwd(x, x, st, False, dx_add=wide)]
    else:
        calls = [lambda: ops.bn_train_bwd_from_parts(xt, x, st, parts, 4), lambda: ops.bn_train_bwd_from_parts(x, wide, st, parts, 4),
                 lambda: ops.bn_train_bwd_from_parts(x, x, st, parts, 4, dx_add=xt), lambda: ops.bn_train_bwd_from_parts(x, x, st, parts, 4, dx=wide)]
    for f in calls:
        with pytest.raises(ValueError):
            f()


# ------------------------------------------------------------------------------------------------ finishing kernels on synthetic partials
NPARTS = (1, 2, 255, 256, 257, 768, 769, 1024, 1025, 4100)        # sum_partials: tail loop only up to 768 rows, the unrolled loop beyond


def _ulps32(got, want, scale=None):
    """|got - want| in units of the fp32 spacing at max(|want|, scale)"""
    got = got.astype(np.float64); w = want.astype(np.float64)
    ref = np.abs(want) if scale is None else np.maximum(np.abs(want), np.abs(scale))
    return np.abs(got - w) / np.spacing(ref.astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("nparts", NPARTS)
def test_bn_train_finish_on_integer_partials(nparts):
    """tl_bn_train_finish over two segments (32 and 64 channels of one 96-channel BatchNorm, the skip concat) of integer-valued fp64
    partials (any summation order gives the same sum); the parts tensors are 37 NaN rows longer than nparts."""
    from treelearn_amd import ops
    rng = np.random.default_rng(nparts)
    n = 16 * nparts + 3
    segs, s_all, ss_all = [], [], []
    for Ci in (32, 64):
        p = np.full((nparts + 37, 2, Ci), np.nan)
        p[:nparts, 0] = rng.integers(-40, 41, size=(nparts, Ci))
        p[:nparts, 1] = rng.integers(200, 601, size=(nparts, Ci))
        s_all.append(p[:nparts, 0].sum(0)); ss_all.append(p[:nparts, 1].sum(0))
        segs.append((torch.from_numpy(p).cuda(), nparts, Ci))
    s, ss = np.concatenate(s_all), np.concatenate(ss_all)
    gen = _gen(nparts)
    gamma, beta, rm, rv = _bn_params(96, gen)
    outs = []
    for _ in range(2):
        rm_, rv_ = rm.clone(), rv.clone()
        nbt = torch.full((), 5, dtype=torch.int64, device="cuda")
        st = ops.bn_train_finish(segs, n, gamma, beta, EPS, MOM, rm_, rv_, nbt)
        outs.append((st, rm_, rv_, nbt))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    st, rm_, rv_, nbt = (t.cpu().numpy() for t in outs[0])
    assert int(nbt) == 6                                                        # one step for the whole call, not one per segment
    assert np.isfinite(st).all() and np.isfinite(rm_).all() and np.isfinite(rv_).all()          # a NaN = a row beyond nparts was read
    f32 = np.float32
    m = s / n
    var = ss / n - m * m
    mf, vf = m.astype(f32), var.astype(f32)
    assert np.array_equal(st[0], mf)                                            # bit for bit
    g, b = gamma.cpu().numpy(), beta.cpu().numpy()
    rs = f32(1.0) / np.sqrt(vf + f32(EPS))
    sc = g * rs
    sh = b - mf * sc
    assert _ulps32(st[1], rs).max() <= 2 and _ulps32(st[2], sc).max() <= 2
    assert _ulps32(st[3], sh, scale=np.maximum(np.abs(b), np.abs(mf * sc))).max() <= 2          # (a fused or a separate multiply: the largest term's spacing)
    rm0, rv0 = rm.cpu().numpy(), rv.cpu().numpy()
    unb = (var * n / (n - 1)).astype(f32)
    want_rm = f32(1.0 - MOM) * rm0 + f32(MOM) * mf
    want_rv = f32(1.0 - MOM) * rv0 + f32(MOM) * unb
    assert _ulps32(rm_, want_rm, scale=np.maximum(np.abs(rm0), np.abs(mf))).max() <= 2
    assert _ulps32(rv_, want_rv, scale=np.maximum(np.abs(rv0), np.abs(unb))).max() <= 2


@pytest.mark.parametrize("nparts,dt", list(zip(NPARTS, [F32, BF16, F16] * 4)), ids=lambda v: NAME.get(v, str(v)))
def test_bn_train_bwd_from_parts_on_synthetic_partials(nparts, dt):
    """tl_bn_train_bwd_from_parts the way backward.bn_conv_backward calls it: x, g, dx, dx_add are the columns 32..96 of 128-wide tensors,
    st and dgb sliced alike; the partials are the float64 sums of g and g * xhat over nparts row chunks, followed by 37 NaN rows.  Against
    tl_bn_train_bwd(relu=False) on the same masked g and against float64."""
    from treelearn_amd import ops
    C, W = 64, 128
    n = 3 * nparts + 5
    gen = _gen(100 + nparts)
    sl = slice(32, 96)
    xw = (torch.randn((n, W), device="cuda", generator=gen) * 2.0 + torch.randn(W, device="cuda", generator=gen)).to(dt)
    gw = (torch.randn((n, W), device="cuda", generator=gen) * (torch.rand((n, W), device="cuda", generator=gen) > 0.4)).to(dt)      # a masked gradient
    aw = torch.randn((n, W), device="cuda", generator=gen).to(dt)
    gamma, beta, _, _ = _bn_params(C, gen)
    stw = torch.full((4, W), float("nan"), device="cuda")
    stw[:, sl] = ops.bn_train_stats(xw[:, sl], gamma, beta, EPS, MOM)                                   # (a column view: ld = 128)
    st = stw[:, sl]
    xd, gd = xw[:, sl].double(), gw[:, sl].double()
    xhat = (xd - st[0].double()) * st[1].double()
    chunk = (torch.arange(n, device="cuda") * nparts) // n
    parts = torch.full((nparts + 37, 2, C), float("nan"), dtype=torch.float64, device="cuda")
    parts[:nparts] = 0.0
    parts[:nparts, 0] = torch.zeros((nparts, C), dtype=torch.float64, device="cuda").index_add_(0, chunk, gd)
    parts[:nparts, 1] = torch.zeros((nparts, C), dtype=torch.float64, device="cuda").index_add_(0, chunk, gd * xhat)
    res = []
    for _ in range(2):
        dxw = torch.full((n, W), float("nan"), dtype=dt, device="cuda")
        dgbw = torch.full((2, W), float("nan"), device="cuda")
        out = ops.bn_train_bwd_from_parts(xw[:, sl], gw[:, sl], st, parts, nparts, dx_add=aw[:, sl], dx=dxw[:, sl], dgb=dgbw[:, sl])
        assert out is not None
        res.append((dxw, dgbw))
    assert torch.equal(res[0][0][:, sl], res[1][0][:, sl]) and torch.equal(res[0][1][:, sl], res[1][1][:, sl])
    dxw, dgbw = res[0]
    for t in (dxw, dgbw):                                                        # nothing written outside the slice
        assert bool(torch.isnan(t[:, :32]).all()) and bool(torch.isnan(t[:, 96:]).all())
    dx, dgamma, dbeta = dxw[:, sl], dgbw[0, sl], dgbw[1, sl]
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dgbw[:, sl]).all())                 # a NaN = nparts not honoured
    # float64: dx = scale * (g - sum g / n - xhat * sum(g xhat) / n) + add, with the statistics as stored (fp32 mean / rstd / scale)
    r_db, r_dg = gd.sum(0), (gd * xhat).sum(0)
    r_dx = st[2].double() * (gd - r_db / n - xhat * r_dg / n) + aw[:, sl].double()
    o_dx, o_dg, o_db = ops.bn_train_bwd(xw[:, sl].contiguous(), gw[:, sl].contiguous(), st.contiguous(), False, dx_add=aw[:, sl].contiguous())
    for name, a, b, ref, tol in (("dx", dx, o_dx, r_dx, TOL_DX[dt]), ("dgamma", dgamma, o_dg, r_dg, 2e-5), ("dbeta", dbeta, o_db, r_db, 2e-5)):
        ea, eb, eab = _relmax(a, ref), _relmax(b, ref), _relmax(a, b.double())
        print(f"from_parts nparts={nparts} {NAME[dt]} {name}: from_parts {ea:.2e} bn_train_bwd {eb:.2e} mutual {eab:.2e}")
        assert ea < tol and eb < tol and eab < 2 * tol, (name, ea, eb, eab)
    # a view the vector kernel cannot take: None (the caller runs tl_bn_train_bwd)
    x132 = torch.zeros((n, C + 4), dtype=dt, device="cuda")
    assert ops.bn_train_bwd_from_parts(x132[:, 4:], gw[:, sl], st, parts, nparts) is None


# ------------------------------------------------------------------------------------------------------------------ tl_affine_relu
@pytest.mark.parametrize("C", [8, 12, 36, 64])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_affine_relu_vs_float64(dt, C):
    """relu?(x * scale + shift) against float64 within one unit in the last place of the output type (the kernel's fp32 fma is one
    rounding of the exact value; float64 then the output type is a double rounding).  C in {8, 64} in form 'c' / 'v8' runs
    k_affine_relu_v8<dtype>, everything else k_affine_relu<dtype>; where both forms serve a width they agree bit for bit."""
    from treelearn_amd import ops
    n = 1031
    gen = _gen(C)
    x0 = (torch.randn((n, C), device="cuda", generator=gen) * 3.0).to(dt)
    scale = torch.randn(C, device="cuda", generator=gen) + 0.2
    shift = torch.randn(C, device="cuda", generator=gen)
    for relu in (True, False):
        for sc, sh in ((scale, shift), (None, None)):
            ref = x0.double() * sc.double() + sh.double() if sc is not None else x0.double()
            if relu:
                ref = torch.relu(ref)
            ys = {}
            for form in FORMS:
                x, buf = _view(x0, form)
                y = ops.affine_relu(x, sc, sh, relu)
                assert torch.equal(y, ops.affine_relu(x, sc, sh, relu))
                assert _pad_untouched(buf, C) and torch.equal(x, x0) and y.dtype == dt
                err = (y.double() - ref).abs()
                ulp = _ulp(torch.maximum(ref.abs(), y.double().abs()), dt)
                assert bool((err <= ulp).all()), (form, relu, sc is not None, float((err / ulp).max()))
                ys[form] = y
            assert torch.equal(ys["c"], ys["v8"]) and torch.equal(ys["c"], ys["v4"])        # vector against scalar kernel: the same fmaf / max / round


# ------------------------------------------------------------------------------------------------------------- row gather / scatter-add
def _int_rows(n, C, dt, gen, lim=None):
    lim = lim or (1000 if dt == F32 else 8)
    return torch.randint(-lim, lim + 1, (n, C), device="cuda", generator=gen).to(dt)


def _esize(dt):
    return 4 if dt == F32 else 2


def _scatter_ref(g, idx, n_rows):
    """float64 index_add_, rounded once to g's dtype: exact for the integer-valued data of these tests"""
    ii = torch.where(idx < 0, idx + n_rows, idx)
    return torch.zeros((n_rows, g.shape[1]), dtype=torch.float64, device=g.device).index_add_(0, ii, g.double()).to(g.dtype)


def _index_sets():
    rng = np.random.default_rng(17)
    mixed = np.concatenate([np.arange(0, 100), np.repeat(np.arange(100, 200), 2), np.repeat(np.arange(200, 300), 3), np.repeat(np.arange(300, 310), 50)])
    rng.shuffle(mixed)                                                             # voxels 310 .. 2999 stay without a point
    return {"mixed": (mixed, 3000), "one_voxel": (np.full(5000, 3), 7), "single": (np.array([0]), 1)}


GATHER_CASES = [(F32, 4), (F32, 36), (BF16, 8), (BF16, 24), (BF16, 32), (F16, 8), (F16, 24), (F16, 32), (BF16, 4)]


@pytest.mark.parametrize("dt,C", GATHER_CASES, ids=lambda v: NAME.get(v, str(v)))
@pytest.mark.parametrize("which", ["mixed", "one_voxel", "single"])
def test_gather_rows_and_gradient_exact(which, dt, C):
    """autograd.gather_rows forward and backward on integer-valued data (every fp32 partial sum exact -> equality with the float64
    index_add_ rounded once): 1, 2, 3, 50 and all 5000 points in one voxel, voxels without a point, N = 1 / n_rows = 1; the gradient as a
    contiguous tensor, as a row-strided view and as a view with a column stride.  bf16 with C = 4 (8-byte rows) takes feats[idx]."""
    from treelearn_amd import autograd, ops
    idx_np, n_rows = _index_sets()[which]
    gen = _gen(C + n_rows)
    idx = torch.from_numpy(idx_np.astype(np.int64)).cuda()
    N = idx.shape[0]
    # (the feats[idx] fallback differentiates through ATen's index_put, which rounds its running sum to bf16 after every point: values in
    # {-1, 0, 1} keep those sums exactly representable too)
    lim = 1 if (C * _esize(dt)) % 16 else None
    feats = _int_rows(n_rows, C, dt, gen).requires_grad_(True)
    g0 = _int_rows(N, C, dt, gen, lim)
    want = _scatter_ref(g0, idx, n_rows)
    wide = torch.full((N, C + 8), float("nan"), dtype=dt, device="cuda"); wide[:, :C] = g0
    strided = torch.zeros((N, 2 * C), dtype=dt, device="cuda"); strided[:, ::2] = g0
    for g in (g0, wide[:, :C], strided[:, ::2]):
        grads = []
        for _ in range(2):
            cache = {}
            y = autograd.gather_rows(feats, idx, cache)
            assert torch.equal(y.detach(), feats.detach()[idx])
            feats.grad = None
            y.backward(g)
            grads.append(feats.grad.clone())
        assert torch.equal(grads[0], grads[1])
        assert torch.equal(grads[0], want), int((grads[0] != want).any(1).sum())
    if (C * g0.element_size()) % 16 == 0:                                          # the kernels directly
        sidx, order = torch.sort(idx, stable=True)
        assert torch.equal(ops.gather_rows(feats.detach(), idx), feats.detach()[idx])
        for g in (g0, wide[:, :C]):
            assert torch.equal(ops.scatter_add_rows(g, order, sidx, n_rows), want)


@pytest.mark.parametrize("dt,C", [(F32, 4), (F32, 36), (BF16, 32), (F16, 8)], ids=lambda v: NAME.get(v, str(v)))
def test_gather_rows_gradient_with_aliasing_negative_indices(dt, C):
    """Negative indices count from the end, as torch indexing does -- also where -1 meets n_rows - 1 and -n_rows meets 0 in one index
    vector: the gradient of feats[idx] adds all of them into one row."""
    from treelearn_amd import autograd
    n_rows, N = 50, 400
    gen = _gen(C)
    idx = torch.randint(1, n_rows - 1, (N,), device="cuda", generator=gen)
    idx[3] = -1; idx[10] = n_rows - 1; idx[200] = -1; idx[201] = n_rows - 1
    idx[5] = -n_rows; idx[6] = 0; idx[300] = 0; idx[399] = -n_rows
    idx[7] = -7; idx[8] = n_rows - 7
    feats = _int_rows(n_rows, C, dt, gen).requires_grad_(True)
    g = _int_rows(N, C, dt, gen)
    want = _scatter_ref(g, idx, n_rows)
    grads = []
    for _ in range(2):
        cache = {}
        y = autograd.gather_rows(feats, idx, cache)
        assert torch.equal(y.detach(), feats.detach()[idx])
        feats.grad = None
        y.backward(g)
        grads.append(feats.grad.clone())
        assert int(cache["v2p_sort"][1].min()) >= 0                               # the cached sort holds normalised indices
    assert torch.equal(grads[0], grads[1])
    bad = torch.nonzero((grads[0] != want).any(1)).flatten().tolist()
    assert not bad, (bad, grads[0][bad[0]].tolist(), want[bad[0]].tolist())


# ---------------------------------------------------------------------------------------------------------------------- head Linears
NS_FWD = (1, 255, 256, 257, 70001)


@pytest.mark.parametrize("Cin", [8, 32, 40, 1024])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_linear_small_f32_vs_float64(dt, Cin):
    """tl_linear_small_f32 (k_conv_tinycout<dtype, CO, OF32 = true>, CO = 1 .. 8: the fp32-result form, also on 16-bit input) for every
    n in NS_FWD, on contiguous rows and on an aligned column view; a misaligned view is refused (None), never served wrongly."""
    from treelearn_amd import ops
    gen = _gen(Cin)
    nmax = NS_FWD[-1]
    x0 = torch.randn((nmax, Cin), device="cuda", generator=gen).to(dt)
    xd = x0.double()
    xv, buf = _view(x0[:257], "v8")
    x4, _ = _view(x0[:257], "v4")
    for co in range(1, 9):
        w = (torch.randn((1, co, Cin), device="cuda", generator=gen) / Cin ** 0.5).to(dt)
        wd = w[0].double()
        for n in NS_FWD:
            out = ops.linear_small_f32(x0[:n], w)
            assert out is not None and out.dtype == F32 and torch.equal(out, ops.linear_small_f32(x0[:n], w))
            err = _relmax(out, xd[:n] @ wd.T)
            assert err < 2e-5, (co, n, err)
        out = ops.linear_small_f32(xv, w)
        assert out is not None and _relmax(out, xd[:257] @ wd.T) < 2e-5 and _pad_untouched(buf, Cin)
        assert ops.linear_small_f32(x4, w) is None


@pytest.mark.parametrize("Cin", [8, 32, 40, 1024])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_conv_fwd_one_tap_tiny_cout_vs_float64(dt, Cin):
    """ops.conv_fwd with K = 1 and Cout = 1 .. 8 (k_conv_tinycout<dtype, CO> for fp32 / bf16 rows; Cin = Cout = 8 belongs to the tiny-Cin
    kernel) with and without out_scale / out_shift / out_relu, for every n in NS_FWD, on contiguous rows, an aligned column view and a
    misaligned one (which must fall back to another kernel and still be right).  The dispatch has no 1 x 1 kernel with fewer than eight
    output channels for IEEE half rows (the model sends those through tl_linear_small_f32): such a call must either be right or be refused
    with an error -- never a silent wrong result."""
    from treelearn_amd import ops
    gen = _gen(Cin + 1)
    nmax = NS_FWD[-1]
    x0 = torch.randn((nmax, Cin), device="cuda", generator=gen).to(dt)
    xd = x0.double()
    xv, buf = _view(x0[:257], "v8")
    x4, buf4 = _view(x0[:257], "v4")
    tol = TOL_Y[dt]
    for co in range(1, 9):
        w = (torch.randn((1, co, Cin), device="cuda", generator=gen) / Cin ** 0.5).to(dt)
        wd = w[0].double()
        osc = torch.randn(co, device="cuda", generator=gen) + 1.5
        osh = torch.randn(co, device="cuda", generator=gen)
        for i, n in enumerate(NS_FWD):
            epi = (i + co) % 3                                                     # 0: plain, 1: scale / shift, 2: scale / shift / relu
            kw = {} if epi == 0 else dict(out_scale=osc, out_shift=osh, out_relu=epi == 2)
            ref = xd[:n] @ wd.T
            if epi:
                ref = ref * osc.double() + osh.double()
            if epi == 2:
                ref = torch.relu(ref)
            try:
                out = ops.conv_fwd(x0[:n], w, None, n, **kw)
            except RuntimeError:
                assert dt == F16                                                   # refused loudly: fine for IEEE half only
                continue
            assert out.dtype == dt and torch.equal(out, ops.conv_fwd(x0[:n], w, None, n, **kw))
            err = _relmax(out, ref)
            assert err < tol, (co, n, epi, err)
        for xx in (xv, x4):
            try:
                out = ops.conv_fwd(xx, w, None, 257)
            except RuntimeError:
                assert dt == F16
                continue
            assert _relmax(out, xd[:257] @ wd.T) < tol
        assert _pad_untouched(buf, Cin) and _pad_untouched(buf4, Cin)


@pytest.mark.parametrize("Cin", [8, 32, 256, 24, 40])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_conv_wgrad_one_tap_tiny_cout_vs_float64(dt, Cin):
    """ops.conv_wgrad(x, g, None, n, 1) with Cout = 1 .. 4: k_wgrad_tinycout<dtype, CO> for Cin in {8, 32, 256}; Cin = 24 and 40
    (256 % (Cin / 8) != 0) fall through to another weight-gradient kernel; n around the 2048-row workgroup."""
    from treelearn_amd import ops
    gen = _gen(Cin + 2)
    nmax = 2049
    x0 = torch.randn((nmax, Cin), device="cuda", generator=gen).to(dt)
    xd = x0.double()
    for co in range(1, 5):
        g0 = torch.randn((nmax, co), device="cuda", generator=gen).to(dt)
        gd = g0.double()
        for n in (1, 2047, 2048, 2049):
            gw = ops.conv_wgrad(x0[:n], g0[:n], None, n, 1)
            assert gw.shape == (1, co, Cin) and gw.dtype == F32
            assert torch.equal(gw, ops.conv_wgrad(x0[:n], g0[:n], None, n, 1))
            err = _relmax(gw[0], gd[:n].T @ xd[:n])
            assert err < 2e-5, (co, n, err)


@pytest.mark.parametrize("dt,co", [(F32, 3), (BF16, 2), (F16, 4), (F32, 1)], ids=lambda v: NAME.get(v, str(v)))
def test_conv_wgrad_tiny_cout_past_the_row_block_cap(dt, co):
    """n = 1024 * 2048 + 1 rows at Cin = 8: the workgroup count of k_wgrad_tinycout is capped at 1024 and a workgroup owns 2049 rows."""
    from treelearn_amd import ops
    n, Cin = 1024 * 2048 + 1, 8
    gen = _gen(co)
    x = torch.randn((n, Cin), device="cuda", generator=gen).to(dt)
    g = torch.randn((n, co), device="cuda", generator=gen).to(dt)
    gw = ops.conv_wgrad(x, g, None, n, 1)
    assert torch.equal(gw, ops.conv_wgrad(x, g, None, n, 1))
    err = _relmax(gw[0], g.double().T @ x.double())
    assert err < 2e-5, err


# --------------------------------------------------------------------------------------------------------------------- bias gradient
def _bias_grad_data(n, C, dt, gen):
    """randn rounded to dt; column 0 cancels: its second half is the negated, shuffled first half, one element = 1e-6 of the absolute sum"""
    g = torch.randn((n, C), device="cuda", generator=gen)
    h = n // 2
    if h >= 1:
        a = g[:h, 0].clone(); a[0] = 0.0
        perm = torch.randperm(h, device="cuda", generator=gen)
        g[:h, 0] = a; g[h:2 * h, 0] = -a[perm]
        if n > 2 * h:
            g[-1, 0] = 0.0
        g = g.to(dt)
        g[h + int(torch.nonzero(perm == 0)[0]), 0] = 1e-6 * float(g[:, 0].double().abs().sum())
    return g.to(dt)


def _check_colsum(got, g):
    ref = g.double().sum(0)
    assert got.dtype == F32 and got.shape == ref.shape
    err = (got.double() - ref).abs()
    bad = torch.nonzero(~(err <= 2.0 ** -22 * ref.abs())).flatten().tolist()
    assert not bad, [(c, float(got[c]), float(ref[c])) for c in bad[:4]]


BIAS_CASES = [(C, n) for C in (2, 3) for n in (63, 64, 65, 66, 67, 100003)] + [(C, n) for C in (4, 32, 1028) for n in (1, 2, 100003)]


@pytest.mark.parametrize("C,n", BIAS_CASES)
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_bias_gradient_vs_float64(dt, C, n):
    """autograd.bias_add's bias gradient (ops.column_sum on the statistics kernel; 2 and 3 columns folded into a 4- / 12-wide matrix plus
    the left-over rows; the n < 64 and C > 1024 branches) and ops.column_sum itself against the float64 column sum, within 2^-22 of the
    sum itself -- also for a column whose sum cancels to 1e-6 of its absolute sum (the accumulation is fp64)."""
    from treelearn_amd import autograd, ops
    gen = _gen(1000 * C + n)
    g = _bias_grad_data(n, C, dt, gen)
    if n > 2:
        s0 = g[:, 0].double()
        assert 0 < abs(float(s0.sum())) < 1e-5 * float(s0.abs().sum())
    got = []
    for _ in range(2):
        bias = torch.zeros(C, device="cuda", requires_grad=True)
        y = autograd.bias_add(torch.zeros((n, C), dtype=dt, device="cuda"), bias)
        y.backward(g)
        got.append(bias.grad.clone())
    assert torch.equal(got[0], got[1])
    _check_colsum(got[0], g)
    if C % 4 == 0 and C <= 1024:
        cs = ops.column_sum(g)
        assert torch.equal(cs, ops.column_sum(g))
        _check_colsum(cs, g)
