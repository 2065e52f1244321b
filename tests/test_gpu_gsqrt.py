"""The general multivector square root (Expr.gsqrt(), GAAST_OP_GSQRT / GAAST_OP_GSQRT_ADJ; kernels k_mv_gsqrt<T, N> and
k_mv_gsqrt_adj<T, N>) on the GPU, against gsqrt_numpy.py (the numpy restatement, its longdouble reference and mpmath's sqrtm).

Inputs (gsqrt_numpy.operands, default_rng(20261021)): 257 items per case, A = gexp(B) with sum |B| in {0.1, 1, 2.5} and items with a
dominant positive scalar, rounded to float32 so that both dtypes see the same values; the restatement in the program's dtype converges
on every one of them (asserted on the CPU).

Forward bound: the residual ||X X - A||_inf / (||L_X||_inf ||X||_inf) of every item and the error against the longdouble root on the
leading items of every kind, both in units of N eps, may be 4 x gsqrt_numpy.FWD_SCALE -- the worst of the same two measures of the
restatement in the program's dtype on the CPU (tests/test_gsqrt_host.py), times 4 for the GPU's sums being contracted into fused
multiply-adds and its pivot ties falling on other roundings.  Gradient bound: the longdouble solve on the longdouble root is the
reference; the error in units of N eps kappa_inf(L_X + R_X) ||a||_inf may be 4 x gsqrt_numpy.GRAD_SCALE.  The worst measured value per
case is printed (a record)."""
import math

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import gsqrt_numpy as gs
import inverse_numpy as inu
from clifford_gram import GramClifford
from layouts import place, place_out

pytestmark = pytest.mark.gpu

NP = {ga.F64: np.float64, ga.F32: np.float32}
EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
TY = {ga.F64: "double", ga.F32: "float"}
DTYPES = [ga.F64, ga.F32]
IDS = ["f64", "f32"]
SEED = 20261021
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
R33 = [1.0] * 3 + [-1.0] * 3
CGA_GRAM = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)
BATCH = 257          # the last workgroup is ragged; several items share a wave at small N
PER_KIND = 65        # items per theta and of the dominant-scalar kind (4 x 65 drawn, the first 257 used)
LEAD = 6             # leading items of every kind with a longdouble reference


def even(n):
    return list(range(0, n + 1, 2))


def full(n):
    return list(range(n + 1))


# name -> (metric, operand grades: every grade of the blade set, N): one or two algebras per kernel size
CASES = {
    "R1": ([1.0], full(1), 2), "R2": ([1.0] * 2, full(2), 4), "R3-even": ([1.0] * 3, even(3), 4), "R3": ([1.0] * 3, full(3), 8),
    "PGA3D-even": (PGA, even(4), 8), "PGA3D": (PGA, full(4), 16), "CGA-even": (CGA, even(5), 16), "CGA": (CGA, full(5), 32),
    "R33-even": (R33, even(6), 32), "R33": (R33, full(6), 64), "R7-even": ([1.0] * 7, even(7), 64),
}
_REF = {}
_CPU = {}


def inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def run(spec, rows, batch):
    out = spec.eval_batch(rows, batch)
    ga.lib().gaast_hip_synchronize()
    return out.download_rows()


def op_rows(metric, grades, A, dtype):
    """vectors over S -> the operand's graded rows in the program's dtype"""
    return np.ascontiguousarray(gx.from_s(metric, grades, A, grades).astype(NP[dtype]))


def out_s(metric, grades, got, out_grades=None):
    n = len(metric)
    return gx.to_s(metric, grades, got, inu.result_grades(n, tuple(sorted(grades))) if out_grades is None else out_grades)


def reference(name):
    """(A over S, theta per item, indices of the leading items, their longdouble roots): computed once, never written to"""
    if name not in _REF:
        metric, grades, N = CASES[name]
        A, th = gs.operands(metric, grades, PER_KIND, np.random.default_rng([SEED, N, len(metric)]))
        A, th = A[:BATCH], th[:BATCH]
        lead = np.concatenate([np.arange(k * PER_KIND, k * PER_KIND + LEAD) for k in range(4)])
        ld = gs.root_reference(metric, grades, A[lead])
        for a in (A, th, lead, ld):
            a.setflags(write=False)
        _REF[name] = (A, th, lead, ld)
    return _REF[name]


def restatement_converges(name, dtype):
    """the restatement in the program's dtype on every item of the case: no domain error (once per case and dtype)"""
    if (name, dtype) not in _CPU:
        metric, grades, N = CASES[name]
        X, steps, bad = gs.forward(metric, grades, reference(name)[0], NP[dtype])
        _CPU[(name, dtype)] = (not bad.any(), int(steps.max()))
    return _CPU[(name, dtype)]


def root_condition(metric, grades, X):
    """||(L_X + R_X)^-1||_inf per item: a perturbation dA of the operand moves the root by at most this times ||dA||_inf"""
    metric, grades = gx._key(metric, grades)
    T = gs.transposed_sum_matrix(gx.structure(metric, grades)[1], np.asarray(X, dtype=np.float64))
    return np.abs(np.linalg.inv(T)).sum(axis=1).max(axis=1)       # (T is the transpose: its inverse's column sums)


def gsqrt_launches(spec, adj=False):
    return [s for s in spec.launches() if ("k_mv_gsqrt_adj<" if adj else "k_mv_gsqrt<") in s]


# ---- 1. the forward bound -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_residual_and_error(name, dtype):
    metric, grades, N = CASES[name]
    n = len(metric)
    A, th, lead, ld = reference(name)
    converged, steps = restatement_converges(name, dtype)
    assert converged and steps <= 8
    spec = inp(0, grades, n).gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    (one,) = spec.launches()            # one launch per evaluation
    assert one.startswith("general_sqrt[") and one.endswith(f":: k_mv_gsqrt<{TY[dtype]},{N}>"), one
    rows = op_rows(metric, grades, A, dtype)
    got = run(spec, [rows], BATCH)
    assert got.shape == (BATCH, len(inu.row_blades(n, inu.result_grades(n, tuple(grades))))) and np.all(np.isfinite(got))
    assert spec.domain_errors() == 0
    X = out_s(metric, grades, got)
    res = gs.residual(metric, grades, X, A, EPS[dtype])
    err = gs.forward_error(X[lead], ld, EPS[dtype])
    bound = 4 * gs.FWD_SCALE[np.dtype(NP[dtype])]
    print(f"FORWARD {name} {TY[dtype]} N={N}: residual {res.max():.3f} error {err.max():.3f} N eps (bound {bound:.1f}); CPU steps <= {steps}")
    assert res.max() <= bound and err.max() <= bound, (name, res.max(), err.max())
    for batch in (1, 5):      # an item's result does not depend on the batch it is part of
        assert np.array_equal(run(spec, [rows[:batch]], batch).view(np.uint8), got[:batch].view(np.uint8))


# ---- 2. cross-checks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gsqrt_of_gexp_b_is_gexp_of_half_b_for_pga3d_screws(dtype):
    """gexp's contract on A = gexp(B) (2 N eps max(1, theta) ||A||_inf), carried to the root by ||(L_X + R_X)^-1||_inf, plus the root's own
    4 FWD_SCALE N eps ||X||_inf"""
    metric, N, B, theta = PGA, 8, 33, 2.0
    Bv = gx.random_operand(metric, [2], B, theta, np.random.default_rng(SEED + 1))
    spec = inp(0, [2], 4).gexp().gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(gsqrt_launches(spec)) == 1 and len(spec.launches()) == 2
    got = out_s(metric, [2], run(spec, [op_rows(metric, [2], Bv, dtype)], B).astype(np.float64))
    assert spec.domain_errors() == 0
    half = gx.forward(metric, [2], Bv / 2, np.longdouble, degree=20)[0].astype(np.float64)
    whole = gx.forward(metric, [2], Bv, np.longdouble, degree=20)[0].astype(np.float64)
    tol = EPS[dtype] * N * (4 * gs.FWD_SCALE[np.dtype(NP[dtype])] * np.abs(half).max(axis=1) + root_condition(metric, [2], half) * 2 * theta * np.abs(whole).max(axis=1))
    err = np.abs(got - half).max(axis=1)
    assert np.all(err <= tol), (err / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_root_of_the_root_squared_twice(dtype):
    """q = gsqrt(gsqrt(a)), ((q q) (q q)) against a.  The inner root X is off by e ||X||_inf, e = 4 FWD_SCALE N eps; the outer root carries
    that over with ||(L_q + R_q)^-1||_inf and adds its own e ||q||_inf: dq.  The fourth power moves by 4 ||q||_1^3 dq (|coeff| <= 1), and the
    three products round within 4 eps of their absolute sums, 3 x 4 eps ||q||_1^4 at most"""
    name = "PGA3D-even"
    metric, grades, N = CASES[name]
    A = reference(name)[0][:65]
    a = inp(0, grades, 4)
    q = a.gsqrt().gsqrt()
    spec = ((q * q) * (q * q)).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = out_s(metric, grades, run(spec, [op_rows(metric, grades, A, dtype)], 65).astype(np.float64))
    assert spec.domain_errors() == 0
    X = gs.root_reference(metric, grades, A)
    qr = gs.root_reference(metric, grades, X.astype(np.float64)).astype(np.float64)
    X = X.astype(np.float64)
    e = 4 * gs.FWD_SCALE[np.dtype(NP[dtype])] * N * EPS[dtype]
    dq = root_condition(metric, grades, qr) * e * np.abs(X).max(axis=1) + e * np.abs(qr).max(axis=1)
    q1 = np.abs(qr).sum(axis=1)
    tol = 4 * q1 ** 3 * dq + 12 * EPS[dtype] * q1 ** 4
    err = np.abs(got - A).max(axis=1)
    assert np.all(err <= tol), (err / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_study_number_of_a_drifted_pga3d_motor(dtype):
    """M ~M = a + b e0123 for any even M of PGA3D; its principal root is sqrt(a) (1 + b / (2 a) e0123).  The product rounds within 4 eps of
    its absolute sum (||M||_1^2 at most), carried to the root by ||(L_X + R_X)^-1||_inf; the root adds 4 FWD_SCALE N eps ||X||_inf"""
    metric, grades, N, B = PGA, even(4), 8, 65
    rng = np.random.default_rng(SEED + 2)
    M = rng.uniform(-1, 1, (B, 8))
    M[:, 0] += 1.5                      # not normalised, scalar part away from 0: a > 0
    M = M.astype(np.float32).astype(np.float64)
    m = inp(0, grades, 4)
    spec = (m * m.rev()).gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = out_s(metric, grades, run(spec, [op_rows(metric, grades, M, dtype)], B).astype(np.float64))
    assert spec.domain_errors() == 0 and len(gsqrt_launches(spec)) == 1
    rows = gx.from_s(metric, grades, M, grades)
    sign = np.array([-1.0 if inu.grade(b) % 4 in (2, 3) else 1.0 for b in inu.row_blades(4, tuple(grades))])
    study = gx.to_s(metric, grades, inu.gp_rows(metric, grades, rows, grades, rows * sign[None], grades))
    a, b = study[:, 0], study[:, 7]
    assert np.abs(study[:, 1:7]).max() <= 1e-15 * np.abs(M).sum(axis=1).max() ** 2      # a Study number: only 1 and e0123
    want = np.zeros_like(study)
    want[:, 0], want[:, 7] = np.sqrt(a), b / (2 * np.sqrt(a))
    tol = EPS[dtype] * (4 * gs.FWD_SCALE[np.dtype(NP[dtype])] * N * np.abs(want).max(axis=1) + root_condition(metric, grades, want) * 4 * np.abs(M).sum(axis=1) ** 2)
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= tol), (err / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sqrt_is_wrong_where_gsqrt_is_right(dtype):
    """a PGA3D screw motor gexp(0.7 e12 + 1.3 e03) and gexp(0.3 e12 + 0.7 e34) in R^4: sqrt() is a closed form for <A>_0 + <A>_2 whose
    bivector part squares to a scalar, so it can only be given those two grades, and its square misses A at order 1; gsqrt's residual
    is within the bound"""
    for metric, comps in ((PGA, {0b0110: 0.7, 0b1001: 1.3}), ([1.0] * 4, {0b0011: 0.3, 0b1100: 0.7})):
        n, N, grades = 4, 8, even(4)
        S = gx.structure(*gx._key(metric, grades))[0]
        Bv = np.zeros((1, 8))
        for m, v in comps.items():
            Bv[0, S.index(m)] = v
        A = gx.forward(metric, grades, Bv, np.float64)[0].astype(np.float32).astype(np.float64)
        rows = op_rows(metric, grades, A, dtype)
        a = inp(0, grades, n)
        ss = inp(0, [0, 2], n).sqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=ga.FLAG_EXP_LOG)
        mask = ss.output_info()[0]
        rows02 = np.ascontiguousarray(gx.from_s(metric, grades, A, [0, 2]).astype(NP[dtype]))
        ys = gx.to_s(metric, grades, run(ss, [rows02], 1).astype(np.float64), [k for k in range(n + 1) if (mask >> k) & 1])
        Cd = gx.structure(*gx._key(metric, grades))[1]
        assert np.abs(gx._gp(Cd, ys, ys) - A).max() > 0.1, np.abs(gx._gp(Cd, ys, ys) - A).max()
        sg = a.gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
        yg = out_s(metric, grades, run(sg, [rows], 1))
        assert sg.domain_errors() == 0
        assert gs.residual(metric, grades, yg, A, EPS[dtype]).max() <= 4 * gs.FWD_SCALE[np.dtype(NP[dtype])]
        half = gx.forward(metric, grades, Bv / 2, np.float64)[0]
        assert np.abs(yg - half).max() <= 1e-5          # ... and it is the half motion gexp(B / 2)


# ---- 3. domain errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "PGA3D", "R7-even"])
def test_domain_errors_are_nan_counted_and_leave_their_neighbours_alone(name, dtype):
    """-1, a vector (e1, PGA3D's ideal e0), 0 and an item with a NaN or an infinity among good items: NaN in every produced component,
    counted once each, the other items bit-identical to a batch without them"""
    metric, grades, N = CASES[name]
    n, B = len(metric), 70
    A = np.array(reference(name)[0][:B])
    spec = inp(0, grades, n).gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    good = run(spec, [op_rows(metric, grades, A, dtype)], B)
    assert spec.domain_errors() == 0
    bad = [0, 3, 4, 5, 37, 64, 69]
    A[[0, 3, 37, 64], :] = 0
    A[0, 0] = -1.0                                   # -1
    if 1 in grades:
        A[3, 1] = 1.0                                # e1 in R^3 (eigenvalues +-1); e0 in PGA3D (e0 e0 = 0: singular)
        A[64, 2] = 1.0                               # e2
    A[4, 1] = np.nan                                 # (items 37, and 3 / 64 of an even case: 0)
    A[5, N - 1] = np.inf
    A[69, 0] = -np.inf
    got = run(spec, [op_rows(metric, grades, A, dtype)], B)
    nan_rows = np.isnan(got).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == bad and not np.isnan(got[~nan_rows]).any()
    assert spec.domain_errors() == len(bad) and spec.domain_errors() == 0
    assert np.array_equal(got[~nan_rows].view(np.uint8), good[~nan_rows].view(np.uint8))     # neighbours in the same wave: untouched
    assert gs.forward(metric, grades, A, NP[dtype])[2].tolist() == nan_rows.tolist()         # the restatement names the same items


# ---- 4. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "R33"])
def test_strided_misaligned_and_shared_rows(name, dtype):
    metric, grades, N = CASES[name]
    n, B = len(metric), 9
    rows = op_rows(metric, grades, reference(name)[0][60:60 + B], dtype)      # (items of two thetas)
    spec = inp(0, grades, n).gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    want = run(spec, [rows], B)
    for lin, lout in (("pad_odd", "contig"), ("shift", "contig"), ("contig", "pad_odd"), ("contig", "shift"), ("shift_pad16", "pad16")):
        p = place(rows, lin, dtype, n, grades)
        o = place_out(B, want.shape[1], lout, dtype, n, grades)
        spec.eval_batch([p.mv], B, out=o.mv)
        p.check()
        o.check()
        assert np.array_equal(o.rows().view(np.uint8), want.view(np.uint8)), (lin, lout)
    assert spec.launch_variants() == [0]
    many = run(spec, [ga.DeviceMV.from_rows(n, grades, rows[:1], dtype)], 257)      # stride 0: one operand shared by every item
    assert many.shape == (257, want.shape[1]) and np.array_equal(many.view(np.uint8), np.repeat(want[:1], 257, axis=0).view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wanted_grades_beta_and_flags(dtype):
    metric, grades, N = CASES["PGA3D"]
    alg, B = ga.MetricAlgebra(metric), 37
    rows = op_rows(metric, grades, reference("PGA3D")[0][:B], dtype)
    sf = inp(0, grades, 4).gsqrt().specialize(alg, dtype=dtype)
    whole = run(sf, [rows], B)
    # a .g(2) selection of the result: the other blades' offsets are -1; one launch, the same bits
    s2 = inp(0, grades, 4).gsqrt().g(2).specialize(alg, dtype=dtype)
    assert s2.output_info() == (1 << 2, 6) and len(gsqrt_launches(s2)) == 1 and len(s2.launches()) == 1
    assert np.array_equal(run(s2, [rows], B).view(np.uint8), whole[:, 5:11].view(np.uint8))
    # beta: the first writer of its buffer (the zero fill folded in: one launch), and not the first (b + gsqrt(a): added into b's copy)
    assert len(sf.launches()) == 1
    brow = np.random.default_rng(SEED + 3).uniform(-1, 1, (B, 16)).astype(NP[dtype])
    sb = (inp(1, grades, 4) + inp(0, grades, 4).gsqrt()).specialize(alg, dtype=dtype)
    assert len(gsqrt_launches(sb)) == 1 and len(sb.launches()) >= 2, sb.launches()
    assert np.array_equal(run(sb, [rows, brow], B).view(np.uint8), (brow + whole).view(np.uint8))
    for f in (_lib.FLAG_NO_FUSION, _lib.FLAG_NO_JIT, _lib.FLAG_EXACT_ORDER):
        sx = inp(0, grades, 4).gsqrt().specialize(alg, dtype=dtype, flags=f)
        assert len(gsqrt_launches(sx)) == 1 and np.array_equal(run(sx, [rows], B).view(np.uint8), whole.view(np.uint8))
        gx_ = sx.vjp(0)
        assert len(gsqrt_launches(gx_, adj=True)) == 1


def test_launch_names_and_counts():
    for dtype in DTYPES:
        for name in ("R1", "PGA3D-even", "R33"):
            metric, grades, N = CASES[name]
            spec = inp(0, grades, len(metric)).gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
            (one,) = spec.launches()
            assert one.startswith("general_sqrt[") and one.endswith(f":: k_mv_gsqrt<{TY[dtype]},{N}>"), one
            (adj,) = gsqrt_launches(spec.vjp(0), adj=True)
            assert not gsqrt_launches(spec.vjp(0))      # the adjoint kernel recomputes the forward itself
            assert adj.startswith("general_sqrt_adjoint[") and adj.endswith(f":: k_mv_gsqrt_adj<{TY[dtype]},{N}>"), adj


def test_unsupported_sizes_are_unimplemented():
    for n, grades in ((7, [0, 1]), (7, full(7)), (8, [2])):
        spec = inp(0, grades, n).gsqrt().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed
        with pytest.raises(_lib.GaastError) as e:
            spec.program()
        assert e.value.status_name == "UNIMPLEMENTED"


# ---- 5. gradients -------------------------------------------------------------------------------------------------------------------
VJP_CASES = ["R3-even", "PGA3D-even", "PGA3D", "CGA-even", "R7-even"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_against_the_longdouble_solve(name, dtype):
    metric, grades, N = CASES[name]
    n = len(metric)
    A, th, lead, ld = reference(name)
    A = A[lead]
    VB = len(lead)
    spec = inp(0, grades, n).gsqrt().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    g = np.random.default_rng(SEED + 4).uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
    grows = np.ascontiguousarray(gx.from_s(metric, grades, g).astype(NP[dtype]))
    grad = spec.vjp(0).eval_batch([op_rows(metric, grades, A, dtype)], grows, VB).download_rows()
    got = gx.to_s(metric, grades, grad.astype(np.float64))
    want = gs.reverse(metric, grades, A, g, np.longdouble, X=ld)
    kappa = gs.sum_condition(metric, grades, np.asarray(ld, dtype=np.float64))
    worst = gs.gradient_error(got, want, EPS[dtype], kappa).max()
    bound = 4 * gs.GRAD_SCALE[np.dtype(NP[dtype])]
    print(f"GRADIENT {name} {TY[dtype]} N={N}: worst {worst:.3f} N eps kappa |a| (bound {bound:.2f}), kappa up to {kappa.max():.1f}")
    assert np.isfinite(got).all() and worst <= bound, (name, worst)


@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_against_central_differences_f64(name):
    """the adjoint identity <g, J v> = <J^T g, v> (inverse_numpy.adjoint_identity), J v by central differences of the longdouble root"""
    metric, grades, N = CASES[name]
    n = len(metric)
    A, th, lead, ld = reference(name)
    A = np.array(A[lead])
    rng = np.random.default_rng(SEED + 5)
    g, v = rng.uniform(-1, 1, A.shape), rng.uniform(-1, 1, A.shape)
    spec = inp(0, grades, n).gsqrt().specialize(ga.MetricAlgebra(metric))
    grad = gx.to_s(metric, grades, spec.vjp(0).eval_batch([op_rows(metric, grades, A, ga.F64)], gx.from_s(metric, grades, g), len(lead)).download_rows())
    f = lambda Z: gs.forward(metric, grades, Z, np.longdouble, max_steps=40)[0].astype(np.float64)
    lhs, rhs, scale = inu.adjoint_identity(f, A, v, g, grad)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


def _sandwich_numpy(a_s, x):
    """(gsqrt(a) x ~gsqrt(a)).g(1) in R^3, a over the even blades, x vectors: the longdouble root, then float64 products"""
    metric, ev = [1.0] * 3, even(3)
    X = gx.from_s(metric, ev, gs.forward(metric, ev, a_s, np.longdouble, max_steps=40)[0].astype(np.float64))
    sign = np.array([-1.0 if inu.grade(m) % 4 in (2, 3) else 1.0 for m in inu.row_blades(3, tuple(ev))])
    return inu.gp_rows(metric, [1, 3], inu.gp_rows(metric, ev, X, [1], x, [1, 3]), ev, X * sign[None], [1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_composed_program_vjp_reduce_and_torch(dtype):
    """(gsqrt(a) * x * gsqrt(a).rev()).g(1) in R^3: the gradient with respect to a against central differences of the numpy sandwich
    (f64: 1e-6), reduce=True against the sum of the per-item gradients of a shared a, and torch_fn() giving the same gradient"""
    import torch
    metric, ev, B = [1.0] * 3, even(3), 1025
    rng = np.random.default_rng(SEED + 6)
    a_s = np.array(reference("R3-even")[0][[3 * PER_KIND + 1]])          # a dominant scalar and a bivector: rotor-like
    arow = op_rows(metric, ev, a_s, dtype)
    x = rng.uniform(-1, 1, (B, 3)).astype(np.float32).astype(NP[dtype])
    g = rng.uniform(-1, 1, (B, 3)).astype(np.float32).astype(NP[dtype])
    a, X = inp(0, ev, 3), inp(1, [1], 3)
    R = a.gsqrt()
    spec = (R * X * R.rev()).g(1).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(gsqrt_launches(spec)) >= 1 and spec.output_info() == (1 << 1, 3)
    shared = ga.DeviceMV.from_rows(3, ev, arow, dtype)
    per = spec.vjp(0).eval_batch([shared, x], g, B).download_rows().astype(np.float64)
    tot = spec.vjp(0).eval_batch([shared, x], g, B, reduce=True).download_rows().astype(np.float64)
    assert per.shape == (B, 4) and tot.shape == (1, 4) and np.isfinite(per).all()
    exact = np.array([math.fsum(per[:, j]) for j in range(4)])
    bound = (1024 + math.ceil(B / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)      # tests/test_gpu_gram_vjp.py: the row sum's bound
    assert np.all(np.abs(tot[0] - exact) <= bound)
    if dtype == ga.F64:
        k = 16
        v = rng.uniform(-1, 1, (1, 4))
        f = lambda z: _sandwich_numpy(np.repeat(z, k, axis=0), x[:k].astype(np.float64))
        jv = (f(a_s + 1e-6 * v) - f(a_s - 1e-6 * v)) / 2e-6
        lhs, rhs = (g[:k] * jv).sum(axis=1), (gx.to_s(metric, ev, per[:k]) * v).sum(axis=1)
        assert np.all(np.abs(lhs - rhs) <= 1e-6 * (np.abs(g[:k]) * np.abs(jv)).sum(axis=1).max())
    if dtype == ga.F64:
        fn = spec.torch_fn()
        at = torch.tensor(np.repeat(arow, 8, axis=0), device="cuda", requires_grad=True)
        out = fn(at, torch.tensor(x[:8], device="cuda"))
        (out * torch.tensor(g[:8], device="cuda")).sum().backward()
        torch.cuda.synchronize()
        assert np.allclose(at.grad.cpu().numpy(), per[:8], rtol=1e-10, atol=1e-12)


# ---- 6. a Gram basis ----------------------------------------------------------------------------------------------------------------
def test_gsqrt_in_the_cga_null_basis():
    """an algebra isomorphism maps principal roots to principal roots: forward against the principal root of the caller-basis
    left-multiplication matrix (Chevalley's recursion, tests/clifford_gram.py: no diagonalisation; the matrix Denman-Beavers iteration
    with numpy's inverse), and the adjoint identity.  The rows go through the compounds of Q on the way in and out: the allowance of
    the existing Gram tests (1e-12 in f64, norm-wise) on top of the forward bound"""
    n, N, B = 5, 32, 4
    alg, cl = ga.GramAlgebra(CGA_GRAM), GramClifford(CGA_GRAM)
    assert not alg.identity_basis()
    order = np.array(inu.row_blades(n, tuple(full(n))))
    rng = np.random.default_rng(SEED + 7)
    x = rng.uniform(-1, 1, (B, 32)) * 0.4 / 32
    x[:, 0] += 1.0                       # a dominant positive scalar, in any basis
    to_bits = lambda r: np.stack([np.bincount(order, weights=row, minlength=1 << n) for row in r])
    left = [cl.left(S) for S in range(1 << n)]

    def root_rows(rows):
        out = np.zeros((rows.shape[0], 1 << n))
        for i, r in enumerate(to_bits(rows)):
            L = sum(r[S] * left[S] for S in range(1 << n))
            Y, Z = L.copy(), np.eye(1 << n)
            for _ in range(12):
                Y, Z = 0.5 * (Y + np.linalg.inv(Z)), 0.5 * (Z + np.linalg.inv(Y))
            assert np.abs(Y @ Y - L).max() <= 1e-13
            out[i] = Y[:, 0]
        return out[:, order]

    spec = inp(0, full(n), n).gsqrt().specialize(alg)
    got = run(spec, [x], B)
    assert len(gsqrt_launches(spec)) == 1 and spec.domain_errors() == 0
    want = root_rows(x)
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= (4 * gs.FWD_SCALE[np.dtype(np.float64)] * N * EPS[ga.F64] + 1e-12) * np.abs(want).max(axis=1)), (err / np.abs(want).max(axis=1)).max()
    v, g = rng.uniform(-1, 1, x.shape), rng.uniform(-1, 1, got.shape)
    grad = spec.vjp(0).eval_batch([x], g, B).download_rows()
    lhs, rhs, scale = inu.adjoint_identity(root_rows, x, v, g, grad)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()
