"""Forward mode through the general square root and logarithm and any-order reverse mode of the root on the GPU
(GAAST_FLAG_GSQRT_GLOG_JVP; GAAST_OP_GSQRT_JVP / GAAST_OP_GLOG_JVP, kernels k_mv_gsqrt_jvp<T, N> and k_mv_jvp_glog<T, N>), against
root_log_jvp_numpy.py.

Accuracy.  The reference of both kernels is the numpy restatement in numpy.longdouble on the reference forward (roots run to their
own floor; theta = 1/16 and 12 nodes for the logarithm), never the code under test.  Units per item: N eps kappa_inf(L_X + R_X)
||u||_inf for the root's tangent u, N eps max(1, sum |log A|) ||J||_inf ||h||_inf for the logarithm's.  The bound is
4 x root_log_jvp_numpy.SQRT_JVP_SCALE / LOG_JVP_SCALE -- the worst error of the restatement in the program's dtype on the CPU
(tests/test_root_log_jvp_host.py measures it on every run; N = 2 has scales of its own), times the project's 4 for the device's
fused multiply-adds and pivot ties on other roundings.  The worst measured value per case is printed (the record of DESIGN.md
sections 16.1 and 17.1).

Inputs: glog_numpy.operands(metric, grades, 2, default_rng([20261021, N])): twelve items (nine at N = 64) whose logarithm takes
0 ... 5 roots and whose roots take differing numbers of steps, in one workgroup, the batch no multiple of 256 / N; R^1 draws 43 per
kind and keeps 257.  Values are rounded to float32 so that both dtypes see the same numbers."""
import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import glog_numpy as gl
import gsqrt_numpy as gs
import inverse_numpy as inu
import root_log_jvp_numpy as rl
from layouts import place, place_out
from test_gpu_gexp2 import dl, only, raw_program
from test_gpu_glog import CGA_GRAM, DTYPES, EPS, IDS, NP, PGA, TY, inp, op_rows, out_s, run
from test_gpu_vjp2 import _check_vjp2

pytestmark = pytest.mark.gpu

SEED = 20261021
FLAG = ga.FLAG_GSQRT_GLOG_JVP
KINDS = ("sqrt", "log")
_DATA = {}


def data(name):
    """(A, h, g over S; then the longdouble tangents, reverse modes and the units' factors): drawn and computed once per case, read-only"""
    if name not in _DATA:
        metric, grades, N = rl.CASES[name]
        A, h, g = rl.case_operands(name)
        X = gs.root_reference(metric, grades, A)
        d = dict(A=A, h=h, g=g, u=rl.sqrt_jvp_reference(metric, grades, A, h).astype(np.float64), l=rl.log_jvp_reference(metric, grades, A, h).astype(np.float64),
                 ra=gs.reverse(metric, grades, A.astype(np.longdouble), g, np.longdouble, X=X).astype(np.float64),
                 rl=gl.reverse_reference(metric, grades, A, g).astype(np.float64),
                 kappa=rl.sum_condition(metric, grades, X.astype(np.float64)), kappa_t=gs.sum_condition(metric, grades, X.astype(np.float64)),
                 ref=gl.log_reference(metric, grades, A).astype(np.float64), jn=gl.jacobian_norm(metric, grades, A, of_j=True),
                 jtn=gl.jacobian_norm(metric, grades, A))
        for a in d.values():
            a.setflags(write=False)
        _DATA[name] = d
    return _DATA[name]


def spec_of(name, kind, dtype, flags=FLAG):
    metric, grades, N = rl.CASES[name]
    x = inp(0, grades, len(metric))
    return (x.gsqrt() if kind == "sqrt" else x.glog()).specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=flags)


def tangent(name, kind, dtype, A=None, h=None):
    """the device's tangent over S, float64"""
    metric, grades, N = rl.CASES[name]
    d = data(name)
    A, h = d["A"] if A is None else A, d["h"] if h is None else h
    got = dl(spec_of(name, kind, dtype).jvp(0).eval_batch([op_rows(metric, grades, A, dtype)], op_rows(metric, grades, h, dtype), len(A)))
    return out_s(metric, grades, got.astype(np.float64))


def errors(name, kind, dtype, got, sel=slice(None)):
    d, eps = data(name), EPS[dtype]
    if kind == "sqrt":
        return rl.sqrt_jvp_error(got, d["u"][sel], eps, d["kappa"][sel])
    return rl.log_jvp_error(got, d["l"][sel], eps, d["ref"][sel], d["jn"][sel], d["h"][sel])


def bound_of(name, kind, dtype):
    return 4 * rl.scale_of(rl.SQRT_JVP_SCALE if kind == "sqrt" else rl.LOG_JVP_SCALE, rl.CASES[name][2], NP[dtype])


# ---- 1. both kernels against the longdouble restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(rl.CASES))
def test_tangents_against_the_longdouble_restatement(name, kind, dtype):
    N = rl.CASES[name][2]
    got = tangent(name, kind, dtype)
    e = errors(name, kind, dtype, got)
    print(f"{kind.upper()}_JVP {name} {TY[dtype]} N={N}: worst {e.max():.3f} units (bound {bound_of(name, kind, dtype):.2f}), {len(got)} items")
    assert np.isfinite(got).all() and e.max() <= bound_of(name, kind, dtype), (name, kind, e.max(), int(np.argmax(e)))
    assert np.abs(data(name)["u" if kind == "sqrt" else "l"]).max() > 0.1
    # an item's result does not depend on the batch it is part of
    d = data(name)
    assert np.array_equal(tangent(name, kind, dtype, d["A"][:5], d["h"][:5]), got[:5])


@pytest.mark.parametrize("kind", KINDS)
def test_the_grid_stride_loop_runs_twice_f32_n2(kind):
    """more items than 8 workgroups per CU x 128 items on any part with at most 512 CUs: the 257 items of the case repeated; the first,
    the last and 64 sampled items against the restatement, and bit for bit what the small batch gives"""
    name, dtype = "R1", ga.F32
    d = data(name)
    B = 2 * 262144 + 77
    idx = np.arange(B) % 257
    small = tangent(name, kind, dtype)
    big = tangent(name, kind, dtype, d["A"][idx], d["h"][idx])
    sample = np.concatenate([[0, B - 1], np.random.default_rng(SEED).integers(1, B - 1, 64)])
    assert np.array_equal(big[sample], small[idx[sample]])
    assert errors(name, kind, dtype, big[sample], idx[sample]).max() <= bound_of(name, kind, dtype)
    assert np.isfinite(big).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["R3-even", "PGA3D", "R7-even"])
def test_transposition_on_the_device(name, kind, dtype):
    """<g, JVP(h, A)> = <ADJ(g, A), h> from the existing adjoint launch, within the sum of the two accuracy bounds: each side's error
    per component times the 1-norm of the vector it is contracted with (the two longdouble references are transposes to 1e-18)"""
    metric, grades, N = rl.CASES[name]
    d, eps, ndt = data(name), EPS[dtype], np.dtype(NP[dtype])
    A, h, g = d["A"], d["h"], d["g"]
    jv = tangent(name, kind, dtype)
    vj = spec_of(name, kind, dtype).vjp(0)
    assert len(only(vj.launches(), "k_mv_gsqrt_adj<" if kind == "sqrt" else "k_mv_glog_adj<")) == 1
    ad = gx.to_s(metric, grades, dl(vj.eval_batch([op_rows(metric, grades, A, dtype)], op_rows(metric, grades, g, dtype), len(A))).astype(np.float64))
    if kind == "sqrt":
        bound = N * eps * (bound_of(name, kind, dtype) * d["kappa"] * np.abs(d["u"]).max(axis=1) * np.abs(g).sum(axis=1) +
                           4 * gs.GRAD_SCALE[ndt] * d["kappa_t"] * np.abs(d["ra"]).max(axis=1) * np.abs(h).sum(axis=1))
    else:
        unit = N * eps * np.maximum(1.0, np.abs(d["ref"]).sum(axis=1))
        bound = unit * (bound_of(name, kind, dtype) * d["jn"] * np.abs(h).max(axis=1) * np.abs(g).sum(axis=1) +
                        4 * gl.GRAD_SCALE[ndt] * d["jtn"] * np.abs(g).max(axis=1) * np.abs(h).sum(axis=1))
    diff = np.abs((g * jv).sum(axis=1) - (ad * h).sum(axis=1))
    assert np.all(diff <= bound), (diff / bound).max()


# ---- 2. spec.jvp(slot) against central differences of the forward GPU program, f64 ---------------------------------------------------
def _check_jvp(spec, rows, rng, B, step=1e-5, tol=1e-6):
    for slot in range(len(rows)):
        j = spec.jvp(slot)
        grad_g = rng.uniform(-1, 1, (B, spec.output_info()[1]))
        grad = dl(spec.vjp(slot).eval_batch(rows, grad_g, B))
        for _ in range(2):
            v = rng.uniform(-1, 1, rows[slot].shape)
            jv = dl(j.eval_batch(rows, v, B))
            plus = run(spec, rows[:slot] + [rows[slot] + step * v] + rows[slot + 1:], B)
            minus = run(spec, rows[:slot] + [rows[slot] - step * v] + rows[slot + 1:], B)
            scale = 1.0 + np.abs(jv) + np.abs(plus + minus) / 2
            assert np.all(np.isfinite(jv)) and np.all(np.abs((plus - minus) / (2 * step) - jv) <= tol * scale), (slot, np.max(np.abs((plus - minus) / (2 * step) - jv) / scale))
            an = np.sum(grad_g * jv, axis=1)
            assert np.all(np.abs(an - np.sum(grad * v, axis=1)) <= tol * (1.0 + np.abs(an)))      # <g, J v> = <J^T g, v>


def _rows(name, sel=slice(0, 8)):
    """graded f64 rows of the case's operands for the tests against central differences: the eight items of magnitude one (gexp(B)
    with sum |B| up to 2.5, and a dominant scalar).  The step 1e-5 truncates at (step / |A|)^2 relative, which is the tolerance 1e-6
    itself for the kind scaled by 0.01; the scaled kinds are left to the accuracy tests above, which hold them"""
    metric, grades, N = rl.CASES[name]
    return np.ascontiguousarray(gx.from_s(metric, grades, data(name)["A"][sel], grades))


def test_jvp_of_gsqrt_and_glog_in_every_slot():
    rng = np.random.default_rng(SEED + 1)
    R3, alg3, algp = [1.0] * 3, ga.MetricAlgebra([1.0] * 3), ga.MetricAlgebra(PGA)
    a3, ap = _rows("R3-even"), _rows("PGA3D")
    B3, Bp = len(a3), len(ap)
    _check_jvp(inp(0, [0, 2], 3).gsqrt().specialize(alg3, flags=FLAG), [a3], rng, B3)
    r = inp(0, [0, 2], 3).gsqrt()
    _check_jvp((r * inp(1, [1], 3) * r.rev()).g(1).specialize(alg3, flags=FLAG), [a3, rng.uniform(-1, 1, (B3, 3))], rng, B3)
    _check_jvp(inp(0, list(range(5)), 4).glog().specialize(algp, flags=FLAG), [ap], rng, Bp)
    # the PGA3D pose error glog(m * t.inv()): motors gexp(B) with sum |B| = 0.1 and 1.0, so the relative motor stays far from the cut
    mot = _rows("PGA3D-even", slice(0, 4))
    pose = (inp(0, [0, 2, 4], 4) * inp(1, [0, 2, 4], 4).inv()).glog().specialize(algp, flags=FLAG)
    _check_jvp(pose, [mot, mot[::-1].copy()], rng, 4)
    assert pose.domain_errors() == 0
    # geodesic midpoint: gexp(0.5 * glog(a)) needs the exponential's flag as well
    mid = (0.5 * inp(0, [0, 2, 4], 4).glog()).gexp().specialize(algp, flags=FLAG | ga.FLAG_GEXP_GRAD2)
    _check_jvp(mid, [_rows("PGA3D-even")], rng, len(_rows("PGA3D-even")))


def test_the_jvp_program_is_the_tangents_copy_and_one_launch():
    for dtype in DTYPES:
        for name in ("R1", "PGA3D-even", "R7-even"):
            N = rl.CASES[name][2]
            for kind, label, kern, others in (("sqrt", "general_sqrt_jvp[", "k_mv_gsqrt_jvp<", ("k_mv_gsqrt<", "k_mv_gsqrt_adj<")),
                                              ("log", "general_log_jvp[", "k_mv_jvp_glog<", ("k_mv_glog<", "k_mv_glog_adj<"))):
                spec = spec_of(name, kind, dtype)
                launches = spec.jvp(0).launches()
                print("LAUNCHES", name, kind, TY[dtype], launches)
                (one,) = only(launches, label)
                assert one.endswith(f":: {kern}{TY[dtype]},{N}>") and f"{N}" in one and "produced" in one, one
                assert not any(only(launches, o) for o in others) and len(launches) <= 2, launches
                # with the flag the forward and the first-order programs launch what they launch without it
                plain = spec_of(name, kind, dtype, flags=0)
                assert spec.launches() == plain.launches() and spec.vjp(0).launches() == plain.vjp(0).launches()


# ---- 3. any order through gsqrt -------------------------------------------------------------------------------------------------------
def _gsqrt_times(flags=FLAG, dtype=ga.F64):
    return (inp(0, [0, 2], 3).gsqrt() * inp(1, [0, 2], 3)).specialize(ga.MetricAlgebra([1.0] * 3), dtype=dtype, flags=flags)


def _pga_root_sandwich(flags=FLAG, dtype=ga.F64):
    r = inp(0, [0, 2, 4], 4).gsqrt()
    return (r * inp(1, [3], 4) * r.rev()).g(3).specialize(ga.MetricAlgebra(PGA), dtype=dtype, flags=flags)


def test_second_and_third_order_of_gsqrt_against_central_differences():
    rng = np.random.default_rng(SEED + 2)
    a = _rows("R3-even")
    B = len(a)
    spec = inp(0, [0, 2], 3).gsqrt().specialize(ga.MetricAlgebra([1.0] * 3), flags=FLAG)
    g = rng.uniform(-1, 1, (B, 4))
    v = spec.vjp(0)
    _check_vjp2(v, [a, g], rng, B, h=1e-5, tol=1e-6)                 # vjp(0).vjp(0) and vjp(0).vjp(n_fwd)
    assert only(v.vjp(0).launches(), "k_mv_gsqrt_jvp<double,4>") and len(only(v.vjp(0).launches(), "k_mv_gsqrt_adj<double,4>")) == 2
    k = rng.uniform(-1, 1, (B, 4))
    _check_vjp2(v.vjp(0), [a, g, k], rng, B, h=1e-5, tol=1e-6)       # the third order against differences of the second
    times = _gsqrt_times()
    y, g2 = rng.uniform(-1, 1, (B, 4)), rng.uniform(-1, 1, (B, times.output_info()[1]))
    for s1 in range(2):
        _check_vjp2(times.vjp(s1), [a, y, g2], rng, B, h=1e-5, tol=1e-6)
    # a PGA3D operand: the even motors
    m = _rows("PGA3D-even")
    pg = inp(0, [0, 2, 4], 4).gsqrt().specialize(ga.MetricAlgebra(PGA), flags=FLAG)
    _check_vjp2(pg.vjp(0), [m, rng.uniform(-1, 1, m.shape)], rng, len(m), h=1e-5, tol=1e-6)


def _near_one(gen, shape, torch):
    x = torch.rand(shape, generator=gen, dtype=torch.float64).sub(0.5).mul(0.4)
    x[:, 0] += 1.0
    return x


def test_torch_gradgradcheck_through_gsqrt():
    import torch
    gen = torch.Generator().manual_seed(0)
    f = _gsqrt_times().torch_fn()
    xs = [_near_one(gen, (3, 4), torch).cuda().requires_grad_(), torch.rand((3, 4), generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_()]
    assert torch.autograd.gradgradcheck(f, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    f = _pga_root_sandwich().torch_fn()      # a shared (batch-1) motor
    xs = [_near_one(gen, (1, 8), torch).cuda().requires_grad_(), torch.rand((3, 4), generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_()]
    assert torch.autograd.gradgradcheck(f, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


def test_torch_hvp_f32_runs_and_is_finite():
    import torch
    gen = torch.Generator().manual_seed(1)
    m = _near_one(gen, (64, 8), torch).float().cuda().requires_grad_()
    X = torch.rand((64, 4), generator=gen, dtype=torch.float64).float().cuda()
    vec = torch.rand((64, 8), generator=gen, dtype=torch.float64).float().cuda()
    y = _pga_root_sandwich(dtype=ga.F32).torch_fn()(m, X)
    gm, = torch.autograd.grad(y.sum(), m, create_graph=True)
    hv, = torch.autograd.grad((gm * vec).sum(), m)
    assert torch.isfinite(hv).all() and hv.abs().max() > 0


# ---- 4. glog ----------------------------------------------------------------------------------------------------------------------------
def test_jvp_of_glog_in_the_cga_null_basis():
    alg = ga.GramAlgebra(CGA_GRAM)
    assert not alg.identity_basis()
    spec = inp(0, list(range(6)), 5).glog().specialize(alg, flags=FLAG)
    rng = np.random.default_rng(SEED + 3)
    x = rng.uniform(-1, 1, (4, 32)) * 0.4 / 32
    x[:, 0] += 1.0                       # a dominant positive scalar, in any basis
    _check_jvp(spec, [x], rng, 4)
    assert only(spec.jvp(0).launches(), "k_mv_jvp_glog<double,32>") and any(l.startswith("linmap[") for l in spec.jvp(0).launches())


def test_double_backward_through_glog_is_refused_by_name_and_the_cotangent_path_works():
    import torch
    spec = (inp(0, [0, 2], 3).glog() * inp(1, [0, 2], 3)).specialize(ga.MetricAlgebra([1.0] * 3), flags=FLAG)
    gen = torch.Generator().manual_seed(3)
    x, y = _near_one(gen, (4, 4), torch).cuda().requires_grad_(), torch.rand((4, 4), generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_()
    gxv, = torch.autograd.grad(spec.torch_fn()(x, y).sum(), x, create_graph=True)
    with pytest.raises(ga.GaastError) as ei:
        torch.autograd.grad(gxv.sum(), x)
    assert ei.value.status_name == "UNIMPLEMENTED" and "GAAST_OP_GLOG_ADJ" in str(ei.value) and "with respect to its operand" in str(ei.value)
    # y and the first cotangent reach the adjoint node through its child0 alone: those two programs build and agree with central
    # differences of the first-order GPU gradient (the torch binding asks for every input that required grad at once, x among them)
    v = spec.vjp(0)
    rng = np.random.default_rng(SEED + 5)
    rows = [x.detach().cpu().numpy(), y.detach().cpu().numpy(), rng.uniform(-1, 1, (4, spec.output_info()[1]))]
    k2 = rng.uniform(-1, 1, (4, 4))
    base = lambda r: dl(v.eval_batch(r[:2], r[2], 4))
    for slot, i in ((1, 1), (v.n_fwd, 2)):
        w = v.vjp(slot)
        assert only(w.launches(), "k_mv_jvp_glog<double,4>") and not only(w.launches(), "k_mv_glog_adj<")
        grad = dl(w.eval_batch(rows, k2, 4))
        dvec = rng.uniform(-1, 1, rows[i].shape)
        plus, minus = base(rows[:i] + [rows[i] + 1e-5 * dvec] + rows[i + 1:]), base(rows[:i] + [rows[i] - 1e-5 * dvec] + rows[i + 1:])
        fd, an = np.sum(k2 * (plus - minus), axis=1) / 2e-5, np.sum(grad * dvec, axis=1)
        assert np.all(np.abs(fd - an) <= 1e-6 * (1.0 + np.abs(an) + np.sum(np.abs(k2) * np.abs(plus + minus), axis=1) / 2))
    # without the flag the refusal is today's
    plain = inp(0, [0, 2], 3).glog().specialize(ga.MetricAlgebra([1.0] * 3))
    with pytest.raises(ga.GaastError) as ei:
        plain.jvp(0)
    assert ei.value.status_name == "UNIMPLEMENTED" and "second-order reverse mode through GAAST_OP_GLOG_ADJ" in str(ei.value)


# ---- 5. row forms, flags, domain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["PGA3D", "R7-even"])
def test_strided_misaligned_and_shared_rows(name, kind, dtype):
    metric, grades, N = rl.CASES[name]
    n, d = len(metric), data(name)
    B = len(d["A"])
    arow, hrow = op_rows(metric, grades, d["A"], dtype), op_rows(metric, grades, d["h"], dtype)
    j = spec_of(name, kind, dtype).jvp(0)
    want = dl(j.eval_batch([arow], hrow, B))
    for lin, lout in (("pad_odd", "contig"), ("shift", "contig"), ("contig", "pad_odd"), ("contig", "shift"), ("shift_pad16", "pad16")):
        pa, ph = place(arow, lin, dtype, n, grades), place(hrow, lin, dtype, n, grades)
        o = place_out(B, want.shape[1], lout, dtype, n, grades)
        j.eval_batch([pa.mv], ph.mv, B, out=o.mv)
        for p in (pa, ph, o):
            p.check()
        assert np.array_equal(o.rows().view(np.uint8), want.view(np.uint8)), (lin, lout)
    # a shared operand (stride 0) with batched tangents: what the same operand gives when it is repeated per item
    Bs = 257
    hm = np.random.default_rng(SEED + 4).uniform(-1, 1, (Bs, hrow.shape[1])).astype(NP[dtype])
    shared = ga.DeviceMV.from_rows(n, grades, arow[:1], dtype)
    per = dl(j.eval_batch([shared], hm, Bs))
    assert np.isfinite(per).all() and np.array_equal(per.view(np.uint8), dl(j.eval_batch([np.repeat(arow[:1], Bs, axis=0)], hm, Bs)).view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_flags_wanted_grades_and_absent_tangent_grades(kind, dtype):
    name = "PGA3D"
    metric, grades, N = rl.CASES[name]
    d = data(name)
    B = len(d["A"])
    arow, hrow = op_rows(metric, grades, d["A"], dtype), op_rows(metric, grades, d["h"], dtype)
    whole = dl(spec_of(name, kind, dtype).jvp(0).eval_batch([arow], hrow, B))
    for f in (ga.FLAG_EXACT_ORDER, ga.FLAG_NO_FUSION, ga.FLAG_NO_JIT):     # these flags change no bit
        assert np.array_equal(dl(spec_of(name, kind, dtype, flags=FLAG | f).jvp(0).eval_batch([arow], hrow, B)).view(np.uint8), whole.view(np.uint8))
    # a hand-built node: the tangent holds grades 1 and 3 only (absent blades read as 0), the result is wanted in grades 2 and 4
    op = _lib.OP_GSQRT_JVP if kind == "sqrt" else _lib.OP_GLOG_JVP
    hpart = gx.restrict(metric, [1, 3], d["h"])
    prog = raw_program(metric, dtype, [0b01010, 0b11111], (op, 0, 1, -1, 0b10100))
    out = dl(prog.eval_batch([np.ascontiguousarray(gx.from_s(metric, grades, hpart, [1, 3]).astype(NP[dtype])), arow], B))
    assert out.shape == (B, 7)
    full = tangent(name, kind, dtype, d["A"], hpart)
    assert np.array_equal(out.astype(np.float64), gx.from_s(metric, grades, full, [2, 4]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_domain_error_items_are_nan_uncounted_and_leave_their_neighbours_alone(kind, dtype):
    """returned values only: the operand -1, PGA3D's ideal element e01 alone and an item with a NaN component, among good items"""
    name = "PGA3D"
    metric, grades, N = rl.CASES[name]
    d = data(name)
    A = np.array(d["A"])
    B = len(A)
    j = spec_of(name, kind, dtype).jvp(0)
    hrow = op_rows(metric, grades, d["h"], dtype)
    good = dl(j.eval_batch([op_rows(metric, grades, A, dtype)], hrow, B))
    bad = [0, 5, 11]
    A[[0, 5], :] = 0
    A[0, 0] = -1.0
    A[5, 3] = 1.0                          # e01 alone
    A[11, 2] = np.nan
    got = dl(j.eval_batch([op_rows(metric, grades, A, dtype)], hrow, B))
    nan_rows = np.isnan(got).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == bad and not np.isnan(got[~nan_rows]).any()
    assert np.array_equal(got[~nan_rows].view(np.uint8), good[~nan_rows].view(np.uint8))      # neighbours in the same wave: untouched
    assert j.vjp2.domain_errors() == 0                                                       # no forward step: nothing is counted
    assert inu.blade_set(4, tuple(grades))[3] == 0b0011
