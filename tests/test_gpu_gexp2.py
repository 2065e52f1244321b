"""Second order through the general exponential on the GPU (GAAST_FLAG_GEXP_GRAD2; GAAST_OP_GEXP_JVP / GAAST_OP_GEXP_ADJ2, kernels
k_mv_gexp_jvp<T, N> and k_mv_gexp_adj2<T, N>), against gexp2_numpy.py.

Accuracy.  The reference of both kernels is the numpy restatement in numpy.longdouble with the program's s and Taylor degree, never the
code under test.  Units per item: N eps max(1, theta) ||h||_inf ||exp A||_inf for the tangent, the same times ||g||_inf for the
second-order adjoint; exp A is gexp_numpy.forward in longdouble with degree 20.  The bound is 4 x gexp2_numpy.JVP_SCALE / ADJ2_SCALE -- the worst
error of the restatement in the program's dtype on the CPU (tests/test_gexp2_host.py measures it on every run; N = 2 has scales of its
own), times the project's 4 for the device's association and its fused multiply-adds.  The worst measured value per case is printed
(the record of DESIGN.md section 15.1).

Inputs: default_rng([20261021, N, k]); every batch mixes theta in {0.1, 1, 3, 8} across consecutive items, so one workgroup holds
items with s = 0 ... 4; values are rounded to float32 so that both dtypes see the same numbers."""
import math

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp2_numpy as g2
import gexp_numpy as gx
import inverse_numpy as inu
from layouts import place, place_out
from test_gpu_gexp import CGA, CGA_GRAM, DTYPES, EPS, IDS, NP, PGA, TY, VB, even, full, inp, op_rows, out_s, run
from test_gpu_vjp2 import _check_vjp2

pytestmark = pytest.mark.gpu

SEED = 20261021
FLAG = ga.FLAG_GEXP_GRAD2
THETAS = np.array([0.1, 1.0, 3.0, 8.0])
# name -> (metric, operand grades, N, batch): N = 2 runs more than one workgroup (128 items each) with a tail; N = 64: three groups of 4
CASES = {"R1": ([1.0], full(1), 2, 257), "R3-even": ([1.0] * 3, even(3), 4, VB), "PGA3D-even": (PGA, even(4), 8, VB),
         "PGA3D": (PGA, full(4), 16, VB), "CGA": (CGA, full(5), 32, VB), "R7-even": ([1.0] * 7, even(7), 64, VB),
         "R3": ([1.0] * 3, full(3), 8, 9), "R33": ([1.0] * 3 + [-1.0] * 3, full(6), 64, 9)}
ACCURACY = ["R1", "R3-even", "PGA3D-even", "PGA3D", "CGA", "R7-even"]
_REF = {}


def data(name):
    """(A, h, g over S, theta per item, exp A in longdouble): drawn once per case, read-only"""
    if name not in _REF:
        metric, grades, N, B = CASES[name]
        rng = np.random.default_rng([SEED, N, B])
        th = THETAS[np.arange(B) % 4]
        A = (gx.random_operand(metric, grades, B, 1.0, rng, np.float64) * th[:, None]).astype(np.float32).astype(np.float64)
        h = gx.restrict(metric, grades, rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64))
        g = rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
        theta = np.asarray(gx.theta_of(A, gx.structure(*gx._key(metric, grades))[2]))
        y = gx.forward(metric, grades, A, np.longdouble, degree=20)[0].astype(np.float64)
        for a in (A, h, g, theta, y):
            a.setflags(write=False)
        _REF[name] = (A, h, g, theta, y)
    return _REF[name]


def gexp_spec(name, dtype, flags=FLAG):
    metric, grades, N, B = CASES[name]
    return inp(0, grades, len(metric)).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=flags)


def rows_of(name, dtype):
    """the graded rows of A, h (operand grades) and g (result grades) in the program's dtype"""
    metric, grades, N, B = CASES[name]
    A, h, g, _, _ = data(name)
    return (op_rows(metric, grades, A, dtype), op_rows(metric, grades, h, dtype), np.ascontiguousarray(gx.from_s(metric, grades, g).astype(NP[dtype])))


def dl(x):
    ga.lib().gaast_hip_synchronize()
    return x.download_rows()


def raw_program(metric, dtype, input_masks, node):
    """a program of the raw ABI: one batched input node per mask (slot i = node i), then `node` = (opcode, child0, child1, third
    child, mask) as the root; through the wire format, as a ProgramImage"""
    import ctypes as C
    n, k = len(metric), len(input_masks)
    nodes = (_lib.NodeDesc * (k + 1))()
    inputs = (_lib.InputDesc * k)()
    for i, m in enumerate(input_masks):
        nodes[i].opcode, nodes[i].child0, nodes[i].child1, nodes[i].minimal_grade_mask = _lib.OP_INPUT, -1, -1, m
        nodes[i].vec_space_dim, nodes[i].input_slot, nodes[i].product_kind = n, i, _lib.PROD_EXPLICIT
        inputs[i].grade_mask, inputs[i].storage_dim, inputs[i].is_const = m, n, 0
    r = nodes[k]
    r.opcode, r.child0, r.child1, r.input_slot, r.minimal_grade_mask = node
    r.vec_space_dim, r.product_kind = n, _lib.PROD_EXPLICIT
    d = _lib.ProgramDesc()
    md = (C.c_double * n)(*metric)
    d.vec_space_dim, d.metric_diag, d.dtype, d.n_nodes, d.nodes, d.root, d.n_inputs, d.inputs, d.flags = n, md, dtype, k + 1, nodes, k, k, inputs, 0
    need = _lib.lib().gaast_program_serialize(C.byref(d), None, 0)
    buf = (C.c_ubyte * need)()
    assert _lib.lib().gaast_program_serialize(C.byref(d), buf, need) == need
    return ga.ast.ProgramImage(bytes(buf))


def only(launches, what):
    return [s for s in launches if what in s]


# ---- 1. both kernels against the longdouble restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ACCURACY)
def test_jvp_and_adj2_against_the_longdouble_restatement(name, dtype):
    metric, grades, N, B = CASES[name]
    A, h, g, theta, y = data(name)
    arow, hrow, grow = rows_of(name, dtype)
    spec = gexp_spec(name, dtype)
    ndt = np.dtype(NP[dtype])
    got = out_s(metric, grades, dl(spec.jvp(0).eval_batch([arow], hrow, B)).astype(np.float64))
    want = g2.jvp(metric, grades, A, h, np.longdouble, s_dtype=NP[dtype]).astype(np.float64)
    ej = g2.jvp_error(got, want, N, EPS[dtype], theta, h, y)
    bound_j = 4 * g2.scale_of(g2.JVP_SCALE, N, ndt)
    print(f"JVP {name} {TY[dtype]} N={N}: worst {ej.max():.3f} N eps max(1, theta) |h| |y| (bound {bound_j:.2f})")
    w = spec.vjp(0).vjp(0)
    got2 = gx.to_s(metric, grades, dl(w.eval_batch([arow, grow], hrow, B)).astype(np.float64))
    want2 = gx.restrict(metric, grades, g2.adj2(metric, grades, A, h, g, np.longdouble, s_dtype=NP[dtype]).astype(np.float64))
    ea = g2.adj2_error(got2, want2, N, EPS[dtype], theta, g, h, y)
    bound_a = 4 * g2.scale_of(g2.ADJ2_SCALE, N, ndt)
    print(f"ADJ2 {name} {TY[dtype]} N={N}: worst {ea.max():.3f} N eps max(1, theta) |g| |h| |y| (bound {bound_a:.2f})")
    assert np.isfinite(got).all() and ej.max() <= bound_j, (name, ej.max(), int(np.argmax(ej)))
    assert np.isfinite(got2).all() and ea.max() <= bound_a, (name, ea.max(), int(np.argmax(ea)))
    assert np.abs(want).max() > 0.1 and np.abs(want2).max() > 0.1
    # an item's result does not depend on the batch it is part of
    assert np.array_equal(dl(spec.jvp(0).eval_batch([arow[:5]], hrow[:5], 5)).view(np.uint8), dl(spec.jvp(0).eval_batch([arow], hrow, B))[:5].view(np.uint8))
    assert np.array_equal(dl(w.eval_batch([arow[:5], grow[:5]], hrow[:5], 5)).view(np.uint8), dl(w.eval_batch([arow, grow], hrow, B))[:5].view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3-even", "PGA3D", "R7-even"])
def test_adjointness_on_the_device(name, dtype):
    """<g, jvp(h)> = <vjp(g), h> within the sum of the two accuracy bounds: each side's error per component, times the 1-norm of the
    vector it is contracted with (the two longdouble restatements are adjoint to 1e-18)"""
    metric, grades, N, B = CASES[name]
    A, h, g, theta, y = data(name)
    arow, hrow, grow = rows_of(name, dtype)
    spec = gexp_spec(name, dtype)
    ndt = np.dtype(NP[dtype])
    jv = out_s(metric, grades, dl(spec.jvp(0).eval_batch([arow], hrow, B)).astype(np.float64))
    vj = gx.to_s(metric, grades, dl(spec.vjp(0).eval_batch([arow], grow, B)).astype(np.float64))
    unit = N * EPS[dtype] * np.maximum(1.0, theta) * np.abs(y).max(axis=1)
    bound = unit * (4 * g2.scale_of(g2.JVP_SCALE, N, ndt) * np.abs(h).max(axis=1) * np.abs(g).sum(axis=1) +
                    4 * gx.GRAD_SCALE[ndt] * np.abs(g).max(axis=1) * np.abs(h).sum(axis=1))
    diff = np.abs((g * jv).sum(axis=1) - (vj * h).sum(axis=1))
    assert np.all(diff <= bound), (diff / bound).max()


# ---- 2. second-order programs against central differences of the first-order GPU gradient, f64 ------------------------------------
def _sandwich(flags=FLAG, dtype=ga.F64):
    b, X = inp(0, [2], 4), inp(1, [3], 4)
    R = b.gexp()
    return (R * X * R.rev()).g(3).specialize(ga.MetricAlgebra(PGA), dtype=dtype, flags=flags)


def _gexp_times(flags=FLAG, dtype=ga.F64):
    return (inp(0, [0, 2], 3).gexp() * inp(1, [0, 2], 3)).specialize(ga.MetricAlgebra([1.0] * 3), dtype=dtype, flags=flags)


def test_second_order_of_gexp_x_times_y_in_r3_even():
    spec = _gexp_times()
    rng = np.random.default_rng(SEED + 1)
    x, y = rng.uniform(-1, 1, (VB, 4)), rng.uniform(-1, 1, (VB, 4))
    g = rng.uniform(-1, 1, (VB, spec.output_info()[1]))
    for s1 in range(2):
        _check_vjp2(spec.vjp(s1), [x, y, g], rng, VB, h=1e-5, tol=1e-6)


def test_second_order_of_the_pga3d_motor_sandwich():
    """gexp(B) X ~gexp(B) projected on grade 3, B a screw bivector with Euclidean and ideal part"""
    spec = _sandwich()
    rng = np.random.default_rng(SEED + 2)
    B = gx.from_s(PGA, [2], gx.random_operand(PGA, [2], VB, 1.0, rng, np.float64) * THETAS[np.arange(VB) % 4][:, None] / 2, [2])
    assert np.all(np.abs(B[:, :3]).sum(axis=1) > 0) and np.all(np.abs(B[:, 3:]).sum(axis=1) > 0)
    X = rng.uniform(-1, 1, (VB, 4))
    g = rng.uniform(-1, 1, (VB, 4))
    for s1 in range(2):
        _check_vjp2(spec.vjp(s1), [B, X, g], rng, VB, h=1e-5, tol=1e-6)
    assert only(spec.vjp(0).vjp(0).launches(), "k_mv_gexp_adj2<double,8>") and only(spec.vjp(0).vjp(2).launches(), "k_mv_gexp_jvp<double,8>")


def test_second_order_of_a_cga_bivector_exponential():
    spec = inp(0, [2], 5).gexp().specialize(ga.MetricAlgebra(CGA), flags=FLAG)
    rng = np.random.default_rng(SEED + 3)
    B = gx.from_s(CGA, [2], gx.random_operand(CGA, [2], VB, 1.0, rng, np.float64) * THETAS[np.arange(VB) % 4][:, None] / 2, [2])
    g = rng.uniform(-1, 1, (VB, spec.output_info()[1]))
    _check_vjp2(spec.vjp(0), [B, g], rng, VB, h=1e-5, tol=1e-6)
    assert only(spec.vjp(0).vjp(0).launches(), "k_mv_gexp_adj2<double,16>")


# ---- 3. row forms and bookkeeping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "R33"])
def test_strided_misaligned_and_shared_rows(name, dtype):
    """the layouts of test_gpu_gexp.test_strided_misaligned_and_shared_rows on all three operand rows of GEXP_ADJ2 and on its result"""
    metric, grades, N, B = CASES[name]
    n = len(metric)
    arow, hrow, grow = rows_of(name, dtype)
    out_grades = inu.result_grades(n, tuple(grades))
    w = gexp_spec(name, dtype).vjp(0).vjp(0)
    want = dl(w.eval_batch([arow, grow], hrow, B))
    for lin, lout in (("pad_odd", "contig"), ("shift", "contig"), ("contig", "pad_odd"), ("contig", "shift"), ("shift_pad16", "pad16")):
        pa, pg, ph = place(arow, lin, dtype, n, grades), place(grow, lin, dtype, n, out_grades), place(hrow, lin, dtype, n, grades)
        o = place_out(B, want.shape[1], lout, dtype, n, grades)
        w.eval_batch([pa.mv, pg.mv], ph.mv, B, out=o.mv)
        for p in (pa, pg, ph, o):
            p.check()
        assert np.array_equal(o.rows().view(np.uint8), want.view(np.uint8)), (lin, lout)
    # a shared generator (stride 0) with batched g and h: what the same generator gives when it is repeated per item
    Bs = 257
    rng = np.random.default_rng(SEED + 4)
    gm = rng.uniform(-1, 1, (Bs, grow.shape[1])).astype(NP[dtype])
    hm = rng.uniform(-1, 1, (Bs, hrow.shape[1])).astype(NP[dtype])
    shared = ga.DeviceMV.from_rows(n, grades, arow[:1], dtype)
    per = dl(w.eval_batch([shared, gm], hm, Bs))
    assert np.array_equal(per.view(np.uint8), dl(w.eval_batch([np.repeat(arow[:1], Bs, axis=0), gm], hm, Bs)).view(np.uint8))
    tot = dl(w.eval_batch([shared, gm], hm, Bs, reduce=True)).astype(np.float64)
    assert per.shape == (Bs, arow.shape[1]) and tot.shape == (1, arow.shape[1])
    per = per.astype(np.float64)
    exact = np.array([math.fsum(per[:, j]) for j in range(per.shape[1])])
    bound = (1024 + math.ceil(Bs / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)      # tests/test_gpu_gram_vjp.py: the row sum's bound
    assert np.all(np.abs(tot[0] - exact) <= bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_absent_grades_wanted_grades_and_beta(dtype):
    metric, N, B = PGA, 8, 13
    alg = ga.MetricAlgebra(metric)
    ev = even(4)
    rng = np.random.default_rng(SEED + 5)
    ndt = np.dtype(NP[dtype])
    # hand-built programs (the expression layer gives a tangent the operand's own grades): g lacks grade 4, h is a bivector, the
    # operand holds every even grade; and a tangent node wanted in grades 2 and 4 only
    A = gx.random_operand(metric, ev, B, 1.0, rng, np.float64) * THETAS[np.arange(B) % 4][:, None]
    A = A.astype(np.float32).astype(np.float64)
    h = gx.restrict(metric, [2], rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64))
    g = gx.restrict(metric, [0, 2], rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64))
    theta = np.asarray(gx.theta_of(A, 1.0))
    yref = gx.forward(metric, ev, A, np.longdouble, degree=20)[0].astype(np.float64)
    arow, hrow, grow = op_rows(metric, ev, A, dtype), np.ascontiguousarray(gx.from_s(metric, ev, h, [2]).astype(NP[dtype])), np.ascontiguousarray(gx.from_s(metric, ev, g, [0, 2]).astype(NP[dtype]))
    adj2 = raw_program(metric, dtype, [0b00101, 0b00100, 0b10101], (_lib.OP_GEXP_ADJ2, 0, 1, 2, 0b10101))
    got = gx.to_s(metric, ev, dl(adj2.eval_batch([grow, hrow, arow], B)).astype(np.float64), ev)
    want = gx.restrict(metric, ev, g2.adj2(metric, ev, A, h, g, np.longdouble, s_dtype=NP[dtype]).astype(np.float64))
    assert np.abs(want).max() > 0.1 and g2.adj2_error(got, want, N, EPS[dtype], theta, g, h, yref).max() <= 4 * g2.scale_of(g2.ADJ2_SCALE, N, ndt)
    jvp = raw_program(metric, dtype, [0b00100, 0b10101], (_lib.OP_GEXP_JVP, 0, 1, -1, 0b10100))
    out = dl(jvp.eval_batch([hrow, arow], B)).astype(np.float64)
    assert out.shape == (B, 7)
    want = gx.from_s(metric, ev, g2.jvp(metric, ev, A, h, np.longdouble, s_dtype=NP[dtype]).astype(np.float64), [2, 4])
    unit = N * EPS[dtype] * np.maximum(1.0, theta) * np.abs(h).max(axis=1) * np.abs(yref).max(axis=1)
    assert np.abs(want).max() > 0.1 and np.all(np.abs(out - want).max(axis=1) <= 4 * g2.scale_of(g2.JVP_SCALE, N, ndt) * unit)
    # a wanted subset of the tangent's grades: one launch, the bits of the whole result's columns
    Af = gx.random_operand(metric, full(4), B, 3.0, rng)
    hf = rng.uniform(-1, 1, Af.shape).astype(np.float32).astype(np.float64)
    arow, hrow = op_rows(metric, full(4), Af, dtype), op_rows(metric, full(4), hf, dtype)
    whole_spec = inp(0, full(4), 4).gexp().specialize(alg, dtype=dtype, flags=FLAG)
    whole = dl(whole_spec.jvp(0).eval_batch([arow], hrow, B))
    part = inp(0, full(4), 4).gexp().g(2).specialize(alg, dtype=dtype, flags=FLAG).jvp(0)
    (one,) = only(part.launches(), "k_mv_gexp_jvp<")
    assert "16 blades, 6 produced" in one, one
    assert np.array_equal(dl(part.eval_batch([arow], hrow, B)).view(np.uint8), whole[:, 5:11].view(np.uint8))
    # beta: e + e adds the same node twice into one buffer: the second launch is not the first writer, and x + x is exact
    e = inp(0, full(4), 4).gexp()
    twice = (e + e).specialize(alg, dtype=dtype, flags=FLAG)
    assert len(only(twice.jvp(0).launches(), "k_mv_gexp_jvp<")) == 2
    assert np.array_equal(dl(twice.jvp(0).eval_batch([arow], hrow, B)).view(np.uint8), (2 * whole).view(np.uint8))
    grow = rng.uniform(-1, 1, (B, 16)).astype(NP[dtype])
    w1, w2 = whole_spec.vjp(0).vjp(0), twice.vjp(0).vjp(0)
    assert len(only(w1.launches(), "k_mv_gexp_adj2<")) == 1 and len(only(w2.launches(), "k_mv_gexp_adj2<")) == 2
    assert np.array_equal(dl(w2.eval_batch([arow, grow], hrow, B)).view(np.uint8), (2 * dl(w1.eval_batch([arow, grow], hrow, B))).view(np.uint8))
    for f in (ga.FLAG_NO_FUSION, ga.FLAG_NO_JIT, ga.FLAG_EXACT_ORDER):     # these flags change nothing
        sx = inp(0, full(4), 4).gexp().specialize(alg, dtype=dtype, flags=FLAG | f)
        assert np.array_equal(dl(sx.jvp(0).eval_batch([arow], hrow, B)).view(np.uint8), whole.view(np.uint8))
        assert np.array_equal(dl(sx.vjp(0).vjp(0).eval_batch([arow, grow], hrow, B)).view(np.uint8), dl(w1.eval_batch([arow, grow], hrow, B)).view(np.uint8))


def test_launch_names_and_counts():
    """one new launch per node, with the kernel and N; neither program runs a forward or a first-order adjoint kernel of its own"""
    for dtype in DTYPES:
        for name in ("R1", "PGA3D-even", "R33"):
            metric, grades, N, _ = CASES[name]
            spec = gexp_spec(name, dtype)
            j, w = spec.jvp(0).launches(), spec.vjp(0).vjp(0).launches()
            (one,) = only(j, "k_mv_gexp")
            assert one.startswith("general_exponential_jvp[") and one.endswith(f":: k_mv_gexp_jvp<{TY[dtype]},{N}>"), one
            (two,) = only(w, "k_mv_gexp")
            assert two.startswith("general_exponential_adjoint2[") and two.endswith(f":: k_mv_gexp_adj2<{TY[dtype]},{N}>"), two
            # with the flag the forward and the first-order programs launch what they launch without it
            plain = gexp_spec(name, dtype, flags=0)
            assert spec.launches() == plain.launches() and spec.vjp(0).launches() == plain.vjp(0).launches()


# ---- 4. domain errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["PGA3D-even", "R7-even"])
def test_domain_error_items_are_nan_uncounted_and_leave_their_neighbours_alone(name, dtype):
    """returned values only: theta > 2048, an infinite and a NaN component"""
    metric, grades, N, B = CASES[name]
    A = np.array(data(name)[0])
    arow, hrow, grow = rows_of(name, dtype)
    spec = gexp_spec(name, dtype)
    j, w = spec.jvp(0), spec.vjp(0).vjp(0)
    good_j, good_w = dl(j.eval_batch([arow], hrow, B)), dl(w.eval_batch([arow, grow], hrow, B))
    bad = [0, 5, 6, 11]
    col = [c for c in range(A.shape[1]) if np.abs(A[:, c]).max() > 0][:3]
    A[0, :] = 0
    A[0, col[0]] = 4096.0                  # theta = 4096 > 2048
    A[5, col[1]] = np.inf
    A[[6, 11], col[2]] = np.nan
    brow = op_rows(metric, grades, A, dtype)
    for prog, rows, cot, good in ((j.vjp2, [brow, None], hrow, good_j), (w, [brow, grow], hrow, good_w)):
        got = dl(prog.eval_batch(rows, cot, B))
        nan_rows = np.isnan(got).all(axis=1)
        assert sorted(np.flatnonzero(nan_rows)) == bad and not np.isnan(got[~nan_rows]).any()
        assert np.array_equal(got[~nan_rows].view(np.uint8), good[~nan_rows].view(np.uint8))      # neighbours in the same wave: untouched
        assert prog.domain_errors() == 0                                                        # no forward GEXP step: nothing is counted


def test_a_second_order_program_counts_only_through_its_forward_gexp_steps():
    spec = _sandwich()
    w = spec.vjp(0).vjp(0)
    n_fwd = len(only(w.launches(), "k_mv_gexp<"))
    assert n_fwd >= 1 and only(w.launches(), "k_mv_gexp_adj2<")
    rng = np.random.default_rng(SEED + 6)
    B = rng.uniform(-0.5, 0.5, (VB, 6))
    B[3, 2] = 5000.0
    X, g, h = rng.uniform(-1, 1, (VB, 4)), rng.uniform(-1, 1, (VB, 4)), rng.uniform(-1, 1, (VB, 6))
    got = dl(w.eval_batch([B, X, g], h, VB))
    assert np.isnan(got[3]).all() and np.isfinite(np.delete(got, 3, axis=0)).all()
    assert w.domain_errors() == n_fwd


# ---- 5. torch -----------------------------------------------------------------------------------------------------------------------
def test_torch_gradgradcheck_through_gexp():
    import torch
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    f = _gexp_times().torch_fn()
    xs = [torch.rand((3, 4), generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_() for _ in range(2)]
    assert torch.autograd.gradgradcheck(f, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    f = _sandwich().torch_fn()      # a shared (batch-1) generator
    xs = [torch.rand(s, generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_() for s in ((1, 6), (3, 4))]
    assert torch.autograd.gradgradcheck(f, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


def test_torch_hvp_f32_agrees_with_f64():
    """Hessian-vector product of sum(gexp(B) X ~gexp(B)) in the generator, one generator per item, sum |B_i| <= 1.
    Bound per item: the product is a sum of compositions of at most six kernels (gexp, its three derivative kernels, two products), each
    within 4 ADJ2_SCALE N eps max(1, theta) of the magnitude scale of its operands (the largest of the family's bounds; the products'
    4 eps sum |terms| is below it); every term of the HVP is bounded by 4 components x sum |X| x sum |v| x e^(2 theta) (two factors that
    are exp(B) or a derivative of it, each at most e^theta in 1-norm): tolerance = 6 x 4 ADJ2_SCALE N eps32 x that scale."""
    import torch
    gen = torch.Generator().manual_seed(1)
    Bn = 64
    gens = torch.rand((Bn, 6), generator=gen, dtype=torch.float64).mul(2).sub(1)
    gens = gens / gens.abs().sum(dim=1, keepdim=True) * torch.linspace(0.1, 1.0, Bn, dtype=torch.float64)[:, None]
    X = torch.rand((Bn, 4), generator=gen, dtype=torch.float64).mul(2).sub(1)
    vec = torch.rand((Bn, 6), generator=gen, dtype=torch.float64).mul(2).sub(1)
    gens, X, vec = gens.float().double(), X.float().double(), vec.float().double()
    hv = {}
    for dtype, dt in ((ga.F64, torch.float64), (ga.F32, torch.float32)):
        b, x = gens.to(dt).cuda().requires_grad_(), X.to(dt).cuda()
        yv = _sandwich(dtype=dtype).torch_fn()(b, x)
        gb, = torch.autograd.grad(yv.sum(), b, create_graph=True)
        hv[dt], = torch.autograd.grad((gb * vec.to(dt).cuda()).sum(), b)
    a, c = hv[torch.float64].cpu(), hv[torch.float32].double().cpu()
    assert a.abs().max() > 0.5
    theta = gens.abs().sum(dim=1)
    scale = 4 * X.abs().sum(dim=1) * vec.abs().sum(dim=1) * torch.exp(2 * theta)
    tol = 6 * 4 * g2.scale_of(g2.ADJ2_SCALE, 8, np.float32) * 8 * 2.0 ** -23 * scale
    assert torch.all((a - c).abs().max(dim=1).values <= tol), float(((a - c).abs().max(dim=1).values / tol).max())


def test_jvp_through_gexp_against_central_differences():
    spec = _sandwich()
    rng = np.random.default_rng(SEED + 7)
    B, X = rng.uniform(-0.5, 0.5, (VB, 6)), rng.uniform(-1, 1, (VB, 4))
    g = rng.uniform(-1, 1, (VB, 4))
    j = spec.jvp(0)
    assert only(j.launches(), "k_mv_gexp_jvp<double,8>")
    grad = dl(spec.vjp(0).eval_batch([B, X], g, VB))
    for _ in range(2):
        v = rng.uniform(-1, 1, B.shape)
        jv = dl(j.eval_batch([B, X], v, VB))
        plus, minus = run(spec, [B + 1e-5 * v, X], VB), run(spec, [B - 1e-5 * v, X], VB)
        cscale = 1.0 + np.abs(jv) + np.abs(plus + minus) / 2
        assert np.all(np.abs((plus - minus) / 2e-5 - jv) <= 1e-6 * cscale)
        an = np.sum(g * jv, axis=1)
        assert np.all(np.abs(an - np.sum(grad * v, axis=1)) <= 1e-6 * (1.0 + np.abs(an)))      # <g, J v> = <J^T g, v>


def test_without_the_flag_the_second_derivative_still_raises():
    import torch
    f = _gexp_times(flags=0).torch_fn()
    gen = torch.Generator().manual_seed(3)
    xs = [torch.rand((4, 4), generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_() for _ in range(2)]
    gxv, = torch.autograd.grad(f(*xs).sum(), xs[0], create_graph=True)
    with pytest.raises(ga.GaastError) as ei:
        torch.autograd.grad(gxv.sum(), xs[0])
    assert ei.value.status_name == "UNIMPLEMENTED" and "GAAST_OP_GEXP_ADJ" in str(ei.value)
    with pytest.raises(ga.GaastError) as ei:
        _gexp_times(flags=0).jvp(0)
    assert ei.value.status_name == "UNIMPLEMENTED"
    # with the flag the same second derivative is a number
    f = _gexp_times().torch_fn()
    gxv, = torch.autograd.grad(f(*xs).sum(), xs[0], create_graph=True)
    hx, = torch.autograd.grad(gxv.sum(), xs[0])
    assert torch.isfinite(hx).all() and hx.abs().max() > 0


# ---- 6. a Gram basis ----------------------------------------------------------------------------------------------------------------
def test_hvp_in_the_cga_null_basis():
    """a bivector generator in the null basis of CGA (GramAlgebra, n = 5): every level of the second-order program is created in the
    forward's basis, and its Hessian-vector product matches central differences of the first-order gradient"""
    alg = ga.GramAlgebra(CGA_GRAM)
    assert not alg.identity_basis()
    spec = inp(0, [2], 5).gexp().specialize(alg, flags=FLAG)
    rng = np.random.default_rng(SEED + 8)
    B = rng.uniform(-0.2, 0.2, (VB, 10))
    g = rng.uniform(-1, 1, (VB, spec.output_info()[1]))
    v = spec.vjp(0)
    _check_vjp2(v, [B, g], rng, VB, h=1e-5, tol=1e-6)
    assert only(v.vjp(0).launches(), "k_mv_gexp_adj2<double,16>") and any(l.startswith("linmap[") for l in v.vjp(0).launches())
