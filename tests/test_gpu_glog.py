"""The general multivector logarithm (Expr.glog(), GAAST_OP_GLOG / GAAST_OP_GLOG_ADJ; kernels k_mv_glog<T, N> and k_mv_glog_adj<T, N>) on
the GPU, against glog_numpy.py (the numpy restatement and its longdouble reference, itself checked against mpmath's logm on the CPU).

Inputs (glog_numpy.operands, default_rng([20261021, N, n])): 257 items per case, A = gexp(B) with sum |B| in {0.1, 1, 2.5}, items with a
dominant positive scalar, and the first kind scaled by 37.5 and by 0.01 (up to 5 roots), rounded to float32 so that both dtypes see the
same values; the restatement in the program's dtype reports no domain error and at most 6 roots on every one of them (asserted).

Forward bound: ||Y - ref||_inf / (N eps max(1, sum_i |ref_i|)) against the longdouble reference on the 6 leading items of every kind may
be 4 x glog_numpy.FWD_SCALE -- the worst of the restatement in the program's dtype on the CPU (tests/test_glog_host.py), times 4 for the
GPU's sums being contracted into fused multiply-adds and its pivot ties falling on other roundings.  Gradient bound: the longdouble
reverse of the reference is the reference; the error in units of N eps max(1, sum |ref_i|) ||J^T||_inf ||g||_inf may be
4 x glog_numpy.GRAD_SCALE.  The worst measured value per case is printed (a record)."""
import ctypes as C
import math

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import glog_numpy as gl
import gsqrt_numpy as gs
import inverse_numpy as inu
from clifford_gram import GramClifford
from layouts import place, place_out
from test_gpu_gsqrt import CASES

pytestmark = pytest.mark.gpu

NP = {ga.F64: np.float64, ga.F32: np.float32}
EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
TY = {ga.F64: "double", ga.F32: "float"}
DTYPES = [ga.F64, ga.F32]
IDS = ["f64", "f32"]
SEED = 20261021
PGA = [0.0, 1.0, 1.0, 1.0]
CGA_GRAM = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)
BATCH = 257          # the last workgroup is ragged; several items share a wave at small N
PER_KIND = 43        # items per kind (6 x 43 drawn, the first 257 used)
LEAD = 6             # leading items of every kind with a longdouble reference
_REF = {}
_CPU = {}
_GRAD = {}
GLOG_OPS = (_lib.OP_GLOG, _lib.OP_GLOG_ADJ)      # (the module is about these two: without them it does not load)


def even(n):
    return list(range(0, n + 1, 2))


def full(n):
    return list(range(n + 1))


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


def fwd_bound(dtype):
    return 4 * gl.FWD_SCALE[np.dtype(NP[dtype])]


def reference(name):
    """(A over S, kind per item, indices of the leading items, their longdouble logarithms): computed once, never written to"""
    if name not in _REF:
        metric, grades, N = CASES[name]
        A, kind = gl.operands(metric, grades, PER_KIND, np.random.default_rng([SEED, N, len(metric)]))
        A, kind = A[:BATCH], kind[:BATCH]
        lead = np.concatenate([np.arange(k * PER_KIND, k * PER_KIND + LEAD) for k in range(gl.KINDS)])
        ld = gl.log_reference(metric, grades, A[lead])
        for a in (A, kind, lead, ld):
            a.setflags(write=False)
        _REF[name] = (A, kind, lead, ld)
    return _REF[name]


def restatement(name, dtype):
    """the restatement in the program's dtype on every item of the case: (no domain error, the most roots), once per case and dtype"""
    if (name, dtype) not in _CPU:
        metric, grades, N = CASES[name]
        Y, s, bad = gl.forward(metric, grades, reference(name)[0], NP[dtype])
        _CPU[(name, dtype)] = (not bad.any(), int(s.max()))
    return _CPU[(name, dtype)]


def glog_launches(spec, adj=False):
    return [s for s in spec.launches() if ("k_mv_glog_adj<" if adj else "k_mv_glog<") in s]


# ---- 1. the forward bound -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_error(name, dtype):
    metric, grades, N = CASES[name]
    n = len(metric)
    A, kind, lead, ld = reference(name)
    clean, roots = restatement(name, dtype)
    assert clean and roots <= 6
    spec = inp(0, grades, n).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    (one,) = spec.launches()            # one launch per evaluation
    assert one.startswith("general_log[") and one.endswith(f":: k_mv_glog<{TY[dtype]},{N}>"), one
    rows = op_rows(metric, grades, A, dtype)
    got = run(spec, [rows], BATCH)
    assert got.shape == (BATCH, len(inu.row_blades(n, inu.result_grades(n, tuple(grades))))) and np.all(np.isfinite(got))
    assert spec.domain_errors() == 0
    Y = out_s(metric, grades, got)
    err = gl.forward_error(Y[lead], ld, EPS[dtype])
    print(f"FORWARD {name} {TY[dtype]} N={N}: error {err.max():.3f} N eps max(1, sum |log A|) (bound {fwd_bound(dtype):.1f}); CPU roots <= {roots}")
    assert err.max() <= fwd_bound(dtype), (name, err.max())
    for batch in (1, 5):      # an item's result does not depend on the batch it is part of
        assert np.array_equal(run(spec, [rows[:batch]], batch).view(np.uint8), got[:batch].view(np.uint8))


# ---- 2. cross-checks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_glog_of_gexp_b_is_b_for_pga3d_screws(dtype):
    """screw bivectors with a Euclidean and an ideal part, sum |B| <= 2.5.  The logarithm of what gexp gave (the same kernel on its own:
    the same bits) is met within the forward bound; B itself within that plus gexp's contract (2 N eps max(1, theta) ||A||_inf), carried
    by ||J||_inf of the logarithm"""
    metric, N, B = PGA, 8, 33
    rng = np.random.default_rng(SEED + 1)
    Bv = np.concatenate([gx.random_operand(metric, [2], B // 3, theta, rng) for theta in (0.3, 1.2, 2.5)])
    S = gx.structure(*gx._key(metric, [2]))[0]
    ideal = np.array([bool(b & 1) and inu.grade(b) == 2 for b in S])
    assert np.all(np.abs(Bv[:, ideal]).sum(axis=1) > 0) and np.all(np.abs(Bv[:, ~ideal]).sum(axis=1) > 0)
    rows = op_rows(metric, [2], Bv, dtype)
    spec = inp(0, [2], 4).gexp().glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(glog_launches(spec)) == 1 and len(spec.launches()) == 2
    got = out_s(metric, [2], run(spec, [rows], B).astype(np.float64))
    assert spec.domain_errors() == 0
    A = out_s(metric, [2], run(inp(0, [2], 4).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], B).astype(np.float64))
    err = gl.forward_error(got, gl.log_reference(metric, [0, 2, 4], A), EPS[dtype])
    assert err.max() <= fwd_bound(dtype), err.max()
    theta = np.abs(Bv).sum(axis=1)
    tol = N * EPS[dtype] * (fwd_bound(dtype) * np.maximum(1.0, theta) + gl.jacobian_norm(metric, [0, 2, 4], A, of_j=True) * 2 * np.maximum(1.0, theta) * np.abs(A).max(axis=1))
    assert np.all(np.abs(got - Bv).max(axis=1) <= tol), (np.abs(got - Bv).max(axis=1) / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "PGA3D-even"])
def test_gexp_of_glog_a_is_a(name, dtype):
    """the sum of both bounds: the logarithm's error dY = 4 FWD_SCALE N eps max(1, sum |Y|) moves the exponential by at most
    ||L_dY||_inf e^theta <= N wmax dY e^theta (theta = wmax sum |Y_i| >= ||L_Y||_inf), and gexp adds 2 N eps max(1, theta) ||A||_inf"""
    metric, grades, N = CASES[name]
    n, B = len(metric), 65
    A = reference(name)[0][:B]
    wmax = gx.structure(*gx._key(metric, grades))[2]
    spec = inp(0, grades, n).glog().gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = out_s(metric, grades, run(spec, [op_rows(metric, grades, A, dtype)], B).astype(np.float64))
    assert spec.domain_errors() == 0 and len(glog_launches(spec)) == 1
    Y = gl.log_reference(metric, grades, A).astype(np.float64)
    ysum = np.abs(Y).sum(axis=1)
    theta = wmax * ysum
    dY = fwd_bound(dtype) * N * EPS[dtype] * np.maximum(1.0, ysum)
    tol = N * wmax * dY * np.exp(theta) + 2 * N * EPS[dtype] * np.maximum(1.0, theta) * np.abs(A).max(axis=1)
    err = np.abs(got - A).max(axis=1)
    assert np.all(err <= tol), (err / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "PGA3D-even"])
def test_glog_a_is_twice_glog_of_gsqrt_a(name, dtype):
    """both bounds: each logarithm within its forward bound of its exact value, the root within 4 gsqrt FWD_SCALE N eps ||X||_inf of
    the principal root, which ||J||_inf of the logarithm at X carries over"""
    metric, grades, N = CASES[name]
    n, B = len(metric), 65
    A = reference(name)[0][:B]
    rows = op_rows(metric, grades, A, dtype)
    a = inp(0, grades, n)
    y1 = out_s(metric, grades, run(a.glog().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], B).astype(np.float64))
    s2 = a.gsqrt().glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(glog_launches(s2)) == 1 and len(s2.launches()) == 2
    y2 = out_s(metric, grades, run(s2, [rows], B).astype(np.float64))
    assert s2.domain_errors() == 0
    Y = gl.log_reference(metric, grades, A).astype(np.float64)
    X = gs.root_reference(metric, grades, A).astype(np.float64)
    unit = N * EPS[dtype]
    tol = unit * fwd_bound(dtype) * (np.maximum(1.0, np.abs(Y).sum(axis=1)) + 2 * np.maximum(1.0, np.abs(Y).sum(axis=1) / 2)) \
        + 2 * gl.jacobian_norm(metric, grades, X, of_j=True) * unit * 4 * gs.FWD_SCALE[np.dtype(NP[dtype])] * np.abs(X).max(axis=1)
    err = np.abs(y1 - 2 * y2).max(axis=1)
    assert np.all(err <= tol), (err / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_logarithm_of_a_pga_translator_is_its_generator(dtype):
    """glog(1 + t e01) = t e01 for t up to 1000 (about ten roots, each halving t exactly), within the forward bound"""
    metric, grades, N = PGA, even(4), 8
    ts = np.array([1e-3, 0.25, 0.5, 3.0, 100.0, 999.0, 1000.0])
    A = np.zeros((len(ts), N))
    A[:, 0], A[:, 1] = 1.0, ts            # the even blades of PGA3D: index 1 is e01
    assert gx.structure(*gx._key(metric, grades))[0][1] == 0b0011
    spec = inp(0, [0, 2], 4).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = out_s(metric, [0, 2], run(spec, [np.ascontiguousarray(gx.from_s(metric, grades, A, [0, 2]).astype(NP[dtype]))], len(ts)).astype(np.float64))
    assert spec.domain_errors() == 0
    want = np.zeros_like(A)
    want[:, 1] = ts
    err = gl.forward_error(got, want, EPS[dtype])
    assert err.max() <= fwd_bound(dtype), err


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_log_is_wrong_where_glog_is_right(dtype):
    """gexp(0.3 e12 + 0.7 e34) in R^4, a rotor with two unequal angles: log() is a closed form for <A>_0 + <A>_2 whose bivector part
    squares to a scalar, so it can only be given those two grades, and it misses the generator at order 0.01; glog is within its bound"""
    metric, n, N, grades = [1.0] * 4, 4, 8, even(4)
    S = gx.structure(*gx._key(metric, grades))[0]
    Bv = np.zeros((1, 8))
    Bv[0, S.index(0b0011)], Bv[0, S.index(0b1100)] = 0.3, 0.7
    A = gx.forward(metric, grades, Bv, np.float64)[0].astype(np.float32).astype(np.float64)
    sl = inp(0, [0, 2], n).log().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=ga.FLAG_EXP_LOG)
    mask = sl.output_info()[0]
    rows02 = np.ascontiguousarray(gx.from_s(metric, grades, A, [0, 2]).astype(NP[dtype]))
    yl = gx.to_s(metric, grades, run(sl, [rows02], 1).astype(np.float64), [k for k in range(n + 1) if (mask >> k) & 1])
    assert np.abs(yl - Bv).max() > 0.02, np.abs(yl - Bv).max()
    sg = inp(0, grades, n).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    yg = out_s(metric, grades, run(sg, [op_rows(metric, grades, A, dtype)], 1))
    assert sg.domain_errors() == 0
    assert gl.forward_error(yg, gl.log_reference(metric, grades, A), EPS[dtype]).max() <= fwd_bound(dtype)
    assert np.abs(yg - Bv).max() <= 1e-5          # ... and it is the generator


# ---- 3. domain errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "PGA3D", "R7-even"])
def test_domain_errors_are_nan_counted_and_leave_their_neighbours_alone(name, dtype):
    """-1, a vector (e1 in R^3; PGA3D's e0), 0, PGA3D's ideal element e01 alone, an item with a NaN component and the unipotent
    1 + 1e5 e01 among good items: NaN in every produced component, counted once each, the other items bit-identical to a batch
    without them"""
    metric, grades, N = CASES[name]
    n, B = len(metric), 70
    A = np.array(reference(name)[0][:B])
    spec = inp(0, grades, n).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    good = run(spec, [op_rows(metric, grades, A, dtype)], B)
    assert spec.domain_errors() == 0
    bad = [0, 3, 4, 37, 64, 69]
    A[[0, 3, 37, 64, 69], :] = 0                     # (item 37: 0)
    A[0, 0] = -1.0                                   # -1
    A[4, 1] = np.nan
    if 1 in grades:
        A[3, 1] = 1.0                                # e1 in R^3 (eigenvalues +-1); e0 in PGA3D (e0 e0 = 0: singular)
    if name == "PGA3D":
        A[64, 3] = 1.0                               # e01 alone
        A[69, 0], A[69, 3] = 1.0, 1e5                # 1 + 1e5 e01: more than 16 roots
    else:
        A[69, 0] = -np.inf
    got = run(spec, [op_rows(metric, grades, A, dtype)], B)
    nan_rows = np.isnan(got).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == bad and not np.isnan(got[~nan_rows]).any()
    assert spec.domain_errors() == len(bad) and spec.domain_errors() == 0
    assert np.array_equal(got[~nan_rows].view(np.uint8), good[~nan_rows].view(np.uint8))     # neighbours in the same wave: untouched
    assert gl.forward(metric, grades, A, NP[dtype])[2].tolist() == nan_rows.tolist()         # the restatement names the same items


# ---- 4. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "R33"])
def test_strided_misaligned_and_shared_rows(name, dtype):
    metric, grades, N = CASES[name]
    n, B = len(metric), 9
    rows = op_rows(metric, grades, reference(name)[0][38:38 + B], dtype)      # (items of two kinds)
    spec = inp(0, grades, n).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
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
    sf = inp(0, grades, 4).glog().specialize(alg, dtype=dtype)
    whole = run(sf, [rows], B)
    # a .g(2) selection of the result: the other blades' offsets are -1; one launch, the same bits
    s2 = inp(0, grades, 4).glog().g(2).specialize(alg, dtype=dtype)
    assert s2.output_info() == (1 << 2, 6) and len(glog_launches(s2)) == 1 and len(s2.launches()) == 1
    assert np.array_equal(run(s2, [rows], B).view(np.uint8), whole[:, 5:11].view(np.uint8))
    # beta: the first writer of its buffer (the zero fill folded in: one launch), and not the first (b + glog(a): added into b's copy)
    assert len(sf.launches()) == 1
    brow = np.random.default_rng(SEED + 3).uniform(-1, 1, (B, 16)).astype(NP[dtype])
    sb = (inp(1, grades, 4) + inp(0, grades, 4).glog()).specialize(alg, dtype=dtype)
    assert len(glog_launches(sb)) == 1 and len(sb.launches()) >= 2, sb.launches()
    assert np.array_equal(run(sb, [rows, brow], B).view(np.uint8), (brow + whole).view(np.uint8))
    for f in (_lib.FLAG_NO_FUSION, _lib.FLAG_NO_JIT, _lib.FLAG_EXACT_ORDER):
        sx = inp(0, grades, 4).glog().specialize(alg, dtype=dtype, flags=f)
        assert len(glog_launches(sx)) == 1 and np.array_equal(run(sx, [rows], B).view(np.uint8), whole.view(np.uint8))
        assert len(glog_launches(sx.vjp(0), adj=True)) == 1


def test_launch_names_and_counts():
    for dtype in DTYPES:
        for name in ("R1", "PGA3D-even", "R33"):
            metric, grades, N = CASES[name]
            spec = inp(0, grades, len(metric)).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
            (one,) = spec.launches()
            assert one.startswith("general_log[") and one.endswith(f":: k_mv_glog<{TY[dtype]},{N}>"), one
            (adj,) = glog_launches(spec.vjp(0), adj=True)
            assert not glog_launches(spec.vjp(0))      # the adjoint kernel recomputes the forward itself
            assert adj.startswith("general_log_adjoint[") and adj.endswith(f":: k_mv_glog_adj<{TY[dtype]},{N}>"), adj
    # a scalar operand is evaluated over the even blades: no scalar lowering
    (one,) = inp(0, [0], 3).glog().specialize(ga.MetricAlgebra([1.0] * 3)).launches()
    assert one.endswith(":: k_mv_glog<double,4>"), one


def test_unsupported_sizes_are_unimplemented():
    for n, grades in ((7, [0, 1]), (7, full(7)), (8, [2]), (1, [0])):
        spec = inp(0, grades, n).glog().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed
        with pytest.raises(_lib.GaastError) as e:
            spec.program()
        assert e.value.status_name == "UNIMPLEMENTED"


# ---- 5. gradients -------------------------------------------------------------------------------------------------------------------
VJP_CASES = ["R3-even", "PGA3D-even", "PGA3D", "CGA-even", "R7-even"]


def grad_reference(name):
    """(A, g, the longdouble cotangent, ||J^T||_inf, log A) of the leading items of a case: once per case"""
    if name not in _GRAD:
        metric, grades, N = CASES[name]
        A, kind, lead, ld = reference(name)
        A = A[lead]
        g = np.random.default_rng(SEED + 4).uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
        _GRAD[name] = (A, g, gl.reverse_reference(metric, grades, A, g), gl.jacobian_norm(metric, grades, A), ld)
    return _GRAD[name]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_against_the_longdouble_reverse(name, dtype):
    metric, grades, N = CASES[name]
    n = len(metric)
    A, g, want, jn, ld = grad_reference(name)
    VB = len(A)
    spec = inp(0, grades, n).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    vj = spec.vjp(0)
    assert len(glog_launches(vj, adj=True)) == 1 and not glog_launches(vj)
    grows = np.ascontiguousarray(gx.from_s(metric, grades, g).astype(NP[dtype]))
    grad = vj.eval_batch([op_rows(metric, grades, A, dtype)], grows, VB).download_rows()
    got = gx.to_s(metric, grades, grad.astype(np.float64))
    worst = gl.gradient_error(got, want, EPS[dtype], ld, jn, g).max()
    bound = 4 * gl.GRAD_SCALE[np.dtype(NP[dtype])]
    print(f"GRADIENT {name} {TY[dtype]} N={N}: worst {worst:.3f} N eps max(1, sum |log A|) |J^T| |g| (bound {bound:.2f}), |J^T| up to {jn.max():.1f}")
    assert np.isfinite(got).all() and worst <= bound, (name, worst)


@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_against_central_differences_of_the_gpu_forward_f64(name):
    """the adjoint identity <g, J v> = <J^T g, v> (inverse_numpy.adjoint_identity), J v by central differences (h = 1e-6) of the GPU's
    own forward; v relative to the item (the items span 0.01 ... 37.5)"""
    metric, grades, N = CASES[name]
    n = len(metric)
    A = np.array(grad_reference(name)[0])
    rng = np.random.default_rng(SEED + 5)
    g = rng.uniform(-1, 1, A.shape)
    v = rng.uniform(-1, 1, A.shape) * np.abs(A).max(axis=1, keepdims=True)
    spec = inp(0, grades, n).glog().specialize(ga.MetricAlgebra(metric))
    grad = gx.to_s(metric, grades, spec.vjp(0).eval_batch([op_rows(metric, grades, A, ga.F64)], gx.from_s(metric, grades, g), len(A)).download_rows())
    f = lambda Z: out_s(metric, grades, run(spec, [op_rows(metric, grades, Z, ga.F64)], len(Z)))
    lhs, rhs, scale = inu.adjoint_identity(f, A, v, g, grad)
    assert spec.domain_errors() == 0
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_forward_item_gives_a_nan_cotangent_and_no_count(dtype):
    metric, grades, N = CASES["PGA3D-even"]
    A = np.array(reference("PGA3D-even")[0][:9])
    A[2, :] = 0
    A[2, 0] = -1.0                                   # -1: no principal logarithm
    A[5, :] = 0
    A[5, 1] = 1.0                                    # e01 alone
    A[7, 3] = np.nan
    spec = inp(0, grades, 4).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    vj = spec.vjp(0)
    g = np.ones((9, N), dtype=NP[dtype])
    grad = vj.eval_batch([op_rows(metric, grades, A, dtype)], g, 9).download_rows()
    nan_rows = np.isnan(grad).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == [2, 5, 7] and np.isfinite(grad[~nan_rows]).all()
    count = C.c_int64(-1)      # the VJP program holds no GLOG step: it owns no counter, and nothing was counted
    _lib.check(_lib.lib().gaast_hip_program_domain_errors(vj.program(), C.byref(count)))
    assert count.value == 0
    fw = run(spec, [op_rows(metric, grades, A, dtype)], 9)      # the forward of the same items: NaN and counted
    assert np.isnan(fw).all(axis=1).tolist() == nan_rows.tolist() and spec.domain_errors() == 3


# ---- 6. a composed program, a Gram basis --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pose_error_loss_vjp_reduce_and_torch(dtype):
    """(glog(a * b.inv())).g(2) in PGA3D-even, the generator of the motion between two motors: the gradient with respect to a against
    central differences of the GPU forward (f64: 1e-6), reduce=True against the sum of the per-item gradients of a shared a, and
    torch_fn() giving the same gradient"""
    import torch
    metric, ev, B = PGA, even(4), 1025
    rng = np.random.default_rng(SEED + 6)
    motors = gx.forward(metric, ev, gx.random_operand(metric, [2], B + 1, 1.0, rng, np.float64), np.float64)[0].astype(np.float32)
    arow = op_rows(metric, ev, motors[:1].astype(np.float64), dtype)
    brow = op_rows(metric, ev, motors[1:].astype(np.float64), dtype)
    g = rng.uniform(-1, 1, (B, 6)).astype(np.float32).astype(NP[dtype])
    a, b = inp(0, ev, 4), inp(1, ev, 4)
    spec = (a * b.inv()).glog().g(2).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(glog_launches(spec)) == 1 and spec.output_info() == (1 << 2, 6)
    shared = ga.DeviceMV.from_rows(4, ev, arow, dtype)
    vj = spec.vjp(0)
    assert len(glog_launches(vj, adj=True)) == 1
    per = vj.eval_batch([shared, brow], g, B).download_rows().astype(np.float64)
    tot = vj.eval_batch([shared, brow], g, B, reduce=True).download_rows().astype(np.float64)
    assert per.shape == (B, 8) and tot.shape == (1, 8) and np.isfinite(per).all()
    exact = np.array([math.fsum(per[:, j]) for j in range(8)])
    bound = (1024 + math.ceil(B / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)      # tests/test_gpu_gram_vjp.py: the row sum's bound
    assert np.all(np.abs(tot[0] - exact) <= bound)
    if dtype == ga.F64:
        k = 16
        v = rng.uniform(-1, 1, (1, 8))
        f = lambda z: run(spec, [np.repeat(z, k, axis=0), brow[:k]], k)
        jv = (f(arow + 1e-6 * v) - f(arow - 1e-6 * v)) / 2e-6
        lhs, rhs = (g[:k] * jv).sum(axis=1), (per[:k] * v).sum(axis=1)
        assert np.all(np.abs(lhs - rhs) <= 1e-6 * (np.abs(g[:k]) * np.abs(jv)).sum(axis=1).max())
        fn = spec.torch_fn()
        at = torch.tensor(np.repeat(arow, 8, axis=0), device="cuda", requires_grad=True)
        out = fn(at, torch.tensor(brow[:8], device="cuda"))
        (out * torch.tensor(g[:8], device="cuda")).sum().backward()
        torch.cuda.synchronize()
        assert np.allclose(at.grad.cpu().numpy(), per[:8], rtol=1e-10, atol=1e-12)


def test_glog_in_the_cga_null_basis():
    """an algebra isomorphism maps principal logarithms to principal logarithms: forward against the principal logarithm of the
    caller-basis left-multiplication matrix (Chevalley's recursion, tests/clifford_gram.py: no diagonalisation; the matrix logarithm by
    inverse scaling and squaring with numpy's inverse and a long Mercator series), against the same program in the diagonal basis of
    the same items, and the adjoint identity.  The rows go through the compounds of Q on the way in and out: the allowance of the
    existing Gram tests (1e-12 in f64, norm-wise) on top of the forward bound"""
    n, N, B = 5, 32, 4
    alg, cl = ga.GramAlgebra(CGA_GRAM), GramClifford(CGA_GRAM)
    assert not alg.identity_basis()
    order = np.array(inu.row_blades(n, tuple(full(n))))
    rng = np.random.default_rng(SEED + 7)
    x = rng.uniform(-1, 1, (B, 32)) * 0.4 / 32
    x[:, 0] += 1.0                       # a dominant positive scalar, in any basis
    to_bits = lambda r: np.stack([np.bincount(order, weights=row, minlength=1 << n) for row in r])
    left = [cl.left(S) for S in range(1 << n)]

    def log_rows(rows):
        out = np.zeros((rows.shape[0], 1 << n))
        eye = np.eye(1 << n)
        for i, r in enumerate(to_bits(rows)):
            L = sum(r[S] * left[S] for S in range(1 << n))
            for _ in range(6):           # six Denman-Beavers roots: ||L - 1|| falls below 0.02
                Y, Z = L.copy(), eye.copy()
                for _ in range(12):
                    Y, Z = 0.5 * (Y + np.linalg.inv(Z)), 0.5 * (Z + np.linalg.inv(Y))
                L = Y
            E, term, acc = L - eye, L - eye, np.zeros_like(L)
            for k in range(1, 12):       # log(1 + E) = E - E^2 / 2 + ...: 0.02^12 / 12 is below 1e-21
                acc += term / k if k % 2 else -term / k
                term = term @ E
            out[i] = 64 * acc[:, 0]
        return out[:, order]

    spec = inp(0, full(n), n).glog().specialize(alg)
    got = run(spec, [x], B)
    assert len(glog_launches(spec)) == 1 and spec.domain_errors() == 0
    want = log_rows(x)
    scale = np.maximum(1.0, np.abs(want).sum(axis=1))
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= (fwd_bound(ga.F64) * N * EPS[ga.F64] + 1e-12) * scale), (err / scale).max()
    # the diagonal-basis result: the rows moved into f = e Q by the compounds of Q^-1 (numpy), the plain program of the diagonal
    # metric, and back by the compounds of Q
    def move(rows, M):
        out = np.zeros_like(rows)
        for k in range(n + 1):
            idx = [i for i, b in enumerate(order) if inu.grade(b) == k]
            sets = [[j for j in range(n) if (order[i] >> j) & 1] for i in idx]
            Ck = np.array([[np.linalg.det(M[np.ix_(J, I)]) if k else 1.0 for I in sets] for J in sets])
            out[:, idx] = rows[:, idx] @ Ck.T
        return out

    plain = inp(0, full(n), n).glog().specialize(ga.MetricAlgebra(alg.diag))
    back = move(run(plain, [move(x, np.linalg.inv(alg.basis))], B), alg.basis)
    assert plain.domain_errors() == 0
    err = np.abs(got - back).max(axis=1)
    assert np.all(err <= (2 * fwd_bound(ga.F64) * N * EPS[ga.F64] + 1e-12) * scale), (err / scale).max()
    v, g = rng.uniform(-1, 1, x.shape), rng.uniform(-1, 1, got.shape)
    grad = spec.vjp(0).eval_batch([x], g, B).download_rows()
    lhs, rhs, scale = inu.adjoint_identity(log_rows, x, v, g, grad)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()
