"""The general multivector exponential (Expr.gexp(), GAAST_OP_GEXP / GAAST_OP_GEXP_ADJ; kernels k_mv_gexp<T, N> and
k_mv_gexp_adj<T, N>) on the GPU, against gexp_numpy.py (the numpy restatement and its mpmath reference).

Forward contract (include/gaast_hip.h): ||y - exp(A)||_inf <= 2 N eps max(1, theta) ||exp(A)||_inf per item that is no domain error,
theta = wmax sum |A_a|.  Inputs: default_rng(20261019), U(-1, 1) on the operand's grades, normalised to sum |A| = theta for theta in
{0.1, 1, 3, 8}, rounded to float32 so that both dtypes see the same values.  exp(A) is mpmath's (50 digits) on the leading items of
every batch and, on every item, gexp_numpy.forward in numpy.longdouble with Taylor degree 20 (rounded to float64 it is within two ulps
of mpmath's on the leading items, asserted).  The worst measured value per case is printed (a record).

Gradient bound: gexp_numpy.reverse in numpy.longdouble with the program's s and Taylor degree is the reference; the error, in units of
N eps max(1, theta) ||g||_inf ||exp(A)||_inf, may be 4 x gexp_numpy.GRAD_SCALE -- the worst error of the same sweep in the program's dtype
on the CPU (tests/test_gexp_host.py), times 4 for the GPU's sums being contracted into fused multiply-adds.  Central differences are a
sanity check at 1e-6 relative in f64 only."""
import math

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import inverse_numpy as inu
from clifford_gram import GramClifford
from layouts import place, place_out

pytestmark = pytest.mark.gpu

NP = {ga.F64: np.float64, ga.F32: np.float32}
EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
TY = {ga.F64: "double", ga.F32: "float"}
DTYPES = [ga.F64, ga.F32]
IDS = ["f64", "f32"]
SEED = 20261019
THETAS = [0.1, 1.0, 3.0, 8.0]
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
STA = [1.0, -1.0, -1.0, -1.0]
CGA_GRAM = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)
B_CONTRACT = 257     # items per (case, theta); batches 1 and 5 are its leading rows


def even(n):
    return list(range(0, n + 1, 2))


def full(n):
    return list(range(n + 1))


# name -> (metric, operand grades, N, leading items with an mpmath reference)
CASES = {
    "R1": ([1.0], full(1), 2, 5), "R2": ([1.0] * 2, full(2), 4, 5), "R3": ([1.0] * 3, full(3), 8, 5), "R3-even": ([1.0] * 3, even(3), 4, 5),
    "PGA3D": (PGA, full(4), 16, 5), "PGA3D-even": (PGA, even(4), 8, 5), "CGA": (CGA, full(5), 32, 2),
    "R33": ([1.0] * 3 + [-1.0] * 3, full(6), 64, 1), "R7-even": ([1.0] * 7, even(7), 64, 1),
}
_REF = {}


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


def reference(name, theta):
    """(A over S, exp(A) by longdouble degree 20 on every item, exp(A) by mpmath on the leading items): computed once"""
    if (name, theta) not in _REF:
        metric, grades, N, lead = CASES[name]
        rng = np.random.default_rng([SEED, int(theta * 10), N])
        A = gx.random_operand(metric, grades, B_CONTRACT, theta, rng)
        ld = gx.forward(metric, grades, A, np.longdouble, degree=20)[0].astype(np.float64)
        mp_ref = gx.exp_reference(metric, grades, A[:lead])
        for a in (A, ld, mp_ref):
            a.setflags(write=False)
        _REF[(name, theta)] = (A, ld, mp_ref)
    return _REF[(name, theta)]


def gexp_launches(spec, adj=False):
    return [s for s in spec.launches() if ("k_mv_gexp_adj<" if adj else "k_mv_gexp<") in s]


# ---- 1. the contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_contract(name, dtype):
    metric, grades, N, lead = CASES[name]
    n = len(metric)
    spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert spec.launches() == gexp_launches(spec) and len(spec.launches()) == 1 and f"k_mv_gexp<{TY[dtype]},{N}>" in spec.launches()[0], spec.launches()
    for theta in THETAS:
        A, ld, mp_ref = reference(name, theta)
        assert np.all(np.abs(ld[:lead] - mp_ref).max(axis=1) <= 2 * EPS[ga.F64] * np.abs(mp_ref).max(axis=1))    # the longdouble reference is mpmath's, both rounded to float64
        rows = op_rows(metric, grades, A, dtype)
        got = run(spec, [rows], B_CONTRACT)
        assert got.shape == (B_CONTRACT, len(inu.row_blades(n, inu.result_grades(n, tuple(grades))))) and np.all(np.isfinite(got))
        assert spec.domain_errors() == 0
        y = out_s(metric, grades, got)
        worst_mp = gx.forward_error(y[:lead], mp_ref, N, EPS[dtype], theta).max()
        worst = gx.forward_error(y, ld, N, EPS[dtype], theta).max()
        print(f"CONTRACT {name} {TY[dtype]} N={N} theta={theta}: worst {worst:.3f} (mpmath items {worst_mp:.3f}) N eps max(1, theta) |y|")
        assert worst_mp <= 2.0 and worst <= 2.0, (name, theta, worst_mp, worst)
        for batch in (1, 5):      # an item's result does not depend on the batch it is part of
            assert np.array_equal(run(spec, [rows[:batch]], batch).view(np.uint8), got[:batch].view(np.uint8))
    big = run(spec, [np.tile(rows, (4, 1))[:1000]], 1000)
    assert np.array_equal(big[:B_CONTRACT].view(np.uint8), got.view(np.uint8)) and np.array_equal(big[B_CONTRACT:2 * B_CONTRACT].view(np.uint8), got.view(np.uint8))


# ---- 2. gexp and exp ---------------------------------------------------------------------------------------------------------------
def wedge_rows(metric, batch, rng):
    """simple bivectors a ^ b of random vectors with coordinates k / 8, as rows of grade 2: exact in float32, so B ^ B = 0 in both dtypes"""
    n = len(metric)
    a, b = rng.integers(-8, 9, (batch, n)) / 8.0, rng.integers(-8, 9, (batch, n)) / 8.0
    blades = inu.row_blades(n, (2,))
    rows = np.zeros((batch, len(blades)))
    for c, m in enumerate(blades):
        i, j = [k for k in range(n) if (m >> k) & 1]
        rows[:, c] = a[:, i] * b[:, j] - a[:, j] * b[:, i]
    assert np.array_equal(rows, rows.astype(np.float32))
    return rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("metric", [[1.0] * 3, CGA, STA], ids=["R3", "R41", "STA"])
def test_gexp_equals_exp_on_simple_bivectors(metric, dtype):
    """within the sum of both contracts: gexp's, and exp's 8 eps (f64) / 64 eps (f32) of the row's largest magnitude (test_gpu_explog.py)"""
    n, B = len(metric), 33
    N = 1 << (n - 1)
    rows = wedge_rows(metric, B, np.random.default_rng(SEED + 3)).astype(NP[dtype])
    b = inp(0, [2], n)
    e = run(b.exp().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=ga.FLAG_EXP_LOG), [rows], B).astype(np.float64)
    sg = b.gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    g = run(sg, [rows], B).astype(np.float64)
    assert sg.domain_errors() == 0
    ye = gx.to_s(metric, [2], e, [0, 2])
    yg = out_s(metric, [2], g)
    theta = np.abs(rows.astype(np.float64)).sum(axis=1)
    top = np.abs(yg).max(axis=1)
    tol = (2 * N * np.maximum(1.0, theta) + (64 if dtype == ga.F32 else 8)) * EPS[dtype] * top
    assert np.all(np.abs(yg - ye).max(axis=1) <= tol), (np.abs(yg - ye).max(axis=1) / tol).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exp_is_wrong_where_gexp_is_right(dtype):
    """a PGA3D screw bivector a e12 + b e03 (its square has an e0123 part) and e12 + 2 e34 in R^4 (a grade-4 part): exp() evaluates its
    closed form on <B B>_0 and misses the mpmath reference at order 1; gexp meets its contract"""
    for metric, comps in ((PGA, {0b0110: 0.7, 0b1001: 1.3}), ([1.0] * 4, {0b0011: 1.0, 0b1100: 2.0})):
        n, N = 4, 8
        blades = inu.row_blades(n, (2,))
        rows = np.zeros((1, 6), dtype=NP[dtype])
        for m, v in comps.items():
            rows[0, blades.index(m)] = v
        A = gx.to_s(metric, [2], rows.astype(np.float64))
        ref = gx.exp_reference(metric, [2], A, method="expm")
        theta = np.abs(A).sum(axis=1)
        b = inp(0, [2], n)
        se = b.exp().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=ga.FLAG_EXP_LOG)
        ye = gx.to_s(metric, [2], run(se, [rows], 1).astype(np.float64), [0, 2])
        assert np.abs(ye - ref).max() > 0.3, np.abs(ye - ref).max()
        sg = b.gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
        yg = out_s(metric, [2], run(sg, [rows], 1))
        assert gx.forward_error(yg, ref, N, EPS[dtype], theta).max() <= 2.0 and sg.domain_errors() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gexp_of_b_times_gexp_of_minus_b_is_one(dtype):
    metric, grades, N, _ = CASES["PGA3D-even"]
    theta, B = 3.0, 65
    A = reference("PGA3D-even", theta)[0][:B]
    rows = op_rows(metric, grades, A, dtype)
    b = inp(0, grades, 4)
    spec = (b.gexp() * (-b).gexp()).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(gexp_launches(spec)) == 2
    got = out_s(metric, grades, run(spec, [rows], B).astype(np.float64))
    yp = gx.forward(metric, grades, A, np.longdouble, degree=20)[0].astype(np.float64)
    ym = gx.forward(metric, grades, -A, np.longdouble, degree=20)[0].astype(np.float64)
    # each factor within its contract, then a product of two N-component rows (4 eps sum |terms|, as the product kernels' tests allow)
    dy = 2 * N * EPS[dtype] * theta
    bound = dy * (np.abs(yp).max(axis=1) * np.abs(ym).sum(axis=1) + np.abs(ym).max(axis=1) * np.abs(yp).sum(axis=1)) + 4 * EPS[dtype] * np.abs(yp).sum(axis=1) * np.abs(ym).max(axis=1)
    got[:, 0] -= 1.0
    assert np.all(np.abs(got).max(axis=1) <= bound), (np.abs(got).max(axis=1) / bound).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_motor_sandwich_in_pga3d(dtype):
    """gexp(B) X ~gexp(B) for screw bivectors B and points X (grade 3), against numpy: the longdouble exponential, then float64 products"""
    metric, B = PGA, 40
    rng = np.random.default_rng(SEED + 4)
    A = gx.random_operand(metric, [2], B, 2.0, rng)
    brow = op_rows(metric, [2], A, dtype)
    x = rng.uniform(-1, 1, (B, 4)).astype(np.float32).astype(NP[dtype])
    b, X = inp(0, [2], 4), inp(1, [3], 4)
    R = b.gexp()
    spec = (R * X * R.rev()).g(3).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert len(gexp_launches(spec)) >= 1 and spec.output_info()[1] == 4
    got = run(spec, [brow, x], B).astype(np.float64)
    y = gx.from_s(metric, [2], gx.forward(metric, [2], A, np.longdouble, degree=20)[0].astype(np.float64))
    ev = even(4)
    sign = np.array([-1.0 if inu.grade(m) % 4 in (2, 3) else 1.0 for m in inu.row_blades(4, tuple(ev))])
    rx = inu.gp_rows(metric, ev, y, [3], x, [1, 3])
    want = inu.gp_rows(metric, [1, 3], rx, ev, y * sign[None], [3])
    scale = inu.gp_rows([1.0] * 4, [1, 3], inu.gp_rows([1.0] * 4, ev, np.abs(y), [3], np.abs(x), [1, 3], absolute=True), ev, np.abs(y), [3], absolute=True)
    tol = (2 * 2 * 8 * 2.0 + 8) * EPS[dtype] * scale.max(axis=1, keepdims=True)     # two factors within the contract (N = 8, theta = 2), two products
    assert np.all(np.abs(got - want) <= tol), (np.abs(got - want) / tol).max()


# ---- 3. domain errors and mixed scalings --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["PGA3D-even", "R7-even"])
def test_domain_errors_are_nan_counted_and_leave_their_neighbours_alone(name, dtype):
    metric, grades, N, _ = CASES[name]
    n, B = len(metric), 70
    A = np.array(reference(name, 1.0)[0][:B])
    good = run(inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype), [op_rows(metric, grades, A, dtype)], B)
    bad = [0, 3, 4, 5, 37, 64, 69]
    col = [j for j in range(A.shape[1]) if np.abs(A[:, j]).max() > 0][:3]
    A[[0, 37], :] = 0
    A[[0, 37], col[0]] = [4096.0, -4096.0]                  # theta = 4096 > 2048
    A[[3, 64], col[1]] = [np.inf, -np.inf]
    A[[4, 5, 69], col[2]] = np.nan
    rows = op_rows(metric, grades, A, dtype)
    spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = run(spec, [rows], B)
    nan_rows = np.isnan(got).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == bad and not np.isnan(got[~nan_rows]).any()
    assert spec.domain_errors() == len(bad) and spec.domain_errors() == 0
    assert np.array_equal(got[~nan_rows].view(np.uint8), good[~nan_rows].view(np.uint8))     # neighbours in the same wave: untouched
    # theta = 2048 exactly is inside the domain (s = 12)
    edge = np.zeros((1, A.shape[1]))
    edge[0, gx.structure(*gx._key(metric, grades))[0].index(0b0110)] = 2048.0      # a rotation: finite
    assert np.isfinite(run(spec, [op_rows(metric, grades, edge, dtype)], 1)).all() and spec.domain_errors() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "R7-even"])
def test_items_of_one_workgroup_need_different_numbers_of_squarings(name, dtype):
    """s = 0, 1, 5 and 12 side by side (N = 8: 32 items per workgroup; N = 64: 4), several workgroups: each item against the longdouble
    reference under the contract, and bitwise what it is when evaluated alone"""
    metric, grades, N, _ = CASES[name]
    n, B = len(metric), 257
    rng = np.random.default_rng(SEED + 5)
    thetas = np.array([0.4, 0.9, 12.0, 1500.0])[np.arange(B) % 4]
    # bivector parts only at the large thetas: e^1500 overflows, a rotation does not
    S = gx.structure(*gx._key(metric, grades))[0]
    biv = np.array([inu.grade(m) == 2 for m in S])
    A = rng.uniform(-1, 1, (B, len(S))) * np.where((thetas > 10)[:, None], biv[None], np.array([inu.grade(m) in grades for m in S])[None])
    A = (A * (thetas / np.abs(A).sum(axis=1))[:, None]).astype(np.float32).astype(np.float64)
    s_want = gx.squarings_of(gx.theta_of(A.astype(NP[dtype]), 1.0))[0]
    assert set(s_want.tolist()) == {0, 1, 5, 12}
    rows = op_rows(metric, grades, A, dtype)
    spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = run(spec, [rows], B)
    assert spec.domain_errors() == 0
    ld = gx.forward(metric, grades, A, np.longdouble, degree=20)[0].astype(np.float64)
    err = gx.forward_error(out_s(metric, grades, got), ld, N, EPS[dtype], thetas)
    assert np.all(err <= 2.0), (err.max(), int(np.argmax(err)))
    for i in (0, 1, 2, 3, 255, 256):
        assert np.array_equal(run(spec, [rows[i:i + 1]], 1).view(np.uint8), got[i:i + 1].view(np.uint8)), i


# ---- 4. rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "R33"])
def test_strided_misaligned_and_shared_rows(name, dtype):
    metric, grades, N, _ = CASES[name]
    n, B = len(metric), 9
    rows = op_rows(metric, grades, reference(name, 3.0)[0][:B], dtype)
    spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    want = run(spec, [rows], B)
    out_grades = inu.result_grades(n, tuple(grades))
    for lin, lout in (("pad_odd", "contig"), ("shift", "contig"), ("contig", "pad_odd"), ("contig", "shift"), ("shift_pad16", "pad16")):
        p = place(rows, lin, dtype, n, grades)
        o = place_out(B, want.shape[1], lout, dtype, n, out_grades)
        spec.eval_batch([p.mv], B, out=o.mv)
        p.check()
        o.check()
        assert np.array_equal(o.rows().view(np.uint8), want.view(np.uint8)), (lin, lout)
    assert spec.launch_variants() == [0]
    many = run(spec, [ga.DeviceMV.from_rows(n, grades, rows[:1], dtype)], 257)      # stride 0: one operand shared by every item
    assert many.shape == (257, want.shape[1]) and np.array_equal(many.view(np.uint8), np.repeat(want[:1], 257, axis=0).view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_absent_grades_wanted_grades_and_beta(dtype):
    metric, N, B = PGA, 16, 37
    alg = ga.MetricAlgebra(metric)
    rng = np.random.default_rng(SEED + 6)
    # an operand of grades 1 and 3: grades 0, 2, 4 of the full blade set read as 0
    A13 = gx.random_operand(metric, [1, 3], B, 3.0, rng)
    s13 = inp(0, [1, 3], 4).gexp().specialize(alg, dtype=dtype)
    got13 = run(s13, [op_rows(metric, [1, 3], A13, dtype)], B)
    ld = gx.forward(metric, [1, 3], A13, np.longdouble, degree=20)[0].astype(np.float64)
    assert got13.shape == (B, 16) and np.all(gx.forward_error(out_s(metric, [1, 3], got13), ld, N, EPS[dtype], 3.0) <= 2.0)
    # the same values padded with explicit zeros give the same bits
    full_rows = op_rows(metric, full(4), A13, dtype)
    sf = inp(0, full(4), 4).gexp().specialize(alg, dtype=dtype)
    whole = run(sf, [full_rows], B)
    assert np.array_equal(whole.view(np.uint8), got13.view(np.uint8))
    # a subset of the result grades: one launch, the same bits
    s2 = inp(0, full(4), 4).gexp().g(2).specialize(alg, dtype=dtype)
    assert s2.output_info() == (1 << 2, 6) and len(gexp_launches(s2)) == 1 and len(s2.launches()) == 1
    assert np.array_equal(run(s2, [full_rows], B).view(np.uint8), whole[:, 5:11].view(np.uint8))
    # beta: the first writer of its buffer (the zero fill folded in: one launch), and not the first (b + gexp(a): added into b's copy)
    assert len(sf.launches()) == 1
    brow = rng.uniform(-1, 1, (B, 16)).astype(NP[dtype])
    sb = (inp(1, full(4), 4) + inp(0, full(4), 4).gexp()).specialize(alg, dtype=dtype)
    assert len(gexp_launches(sb)) == 1 and len(sb.launches()) >= 2, sb.launches()
    assert np.array_equal(run(sb, [full_rows, brow], B).view(np.uint8), (brow + whole).view(np.uint8))
    for f in (_lib.FLAG_NO_FUSION, _lib.FLAG_NO_JIT, _lib.FLAG_EXACT_ORDER):
        sx = inp(0, full(4), 4).gexp().specialize(alg, dtype=dtype, flags=f)
        assert len(gexp_launches(sx)) == 1 and np.array_equal(run(sx, [full_rows], B).view(np.uint8), whole.view(np.uint8))


def test_launch_names_and_counts():
    for dtype in DTYPES:
        for name in ("R1", "PGA3D-even", "R33"):
            metric, grades, N, _ = CASES[name]
            spec = inp(0, grades, len(metric)).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
            (one,) = spec.launches()
            assert one.startswith("general_exponential[") and one.endswith(f":: k_mv_gexp<{TY[dtype]},{N}>"), one
            (adj,) = gexp_launches(spec.vjp(0), adj=True)
            assert adj.startswith("general_exponential_adjoint[") and adj.endswith(f":: k_mv_gexp_adj<{TY[dtype]},{N}>"), adj
            assert not gexp_launches(spec.vjp(0))      # the adjoint kernel recomputes the forward itself


def test_unsupported_sizes_are_unimplemented():
    for n, grades in ((7, [0, 1]), (7, full(7)), (8, [2]), (1, [0]), (0, [0])):
        spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed
        with pytest.raises(_lib.GaastError) as e:
            spec.program()
        assert e.value.status_name == "UNIMPLEMENTED"


# ---- 5. gradients -----------------------------------------------------------------------------------------------------------------
VJP_CASES = ["R3", "PGA3D-even", "PGA3D", "CGA", "R7-even"]
VB = 12


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_against_the_longdouble_sweep(name, dtype):
    metric, grades, N, _ = CASES[name]
    n = len(metric)
    spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    rng = np.random.default_rng(SEED + 7)
    worst = 0.0
    for theta in THETAS:
        A, ld, _ = reference(name, theta)
        A, ld = A[:VB], ld[:VB]
        g = rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
        grows = np.ascontiguousarray(gx.from_s(metric, grades, g).astype(NP[dtype]))
        grad = spec.vjp(0).eval_batch([op_rows(metric, grades, A, dtype)], grows, VB).download_rows()
        got = gx.to_s(metric, grades, grad.astype(np.float64))
        want = gx.restrict(metric, grades, gx.reverse(metric, grades, A, g, np.longdouble, s_dtype=NP[dtype]).astype(np.float64))
        worst = max(worst, gx.gradient_error(got, want, N, EPS[dtype], theta, g, ld).max())
    print(f"GRADIENT {name} {TY[dtype]} N={N}: worst {worst:.3f} N eps max(1, theta) |g| |y| (bound {4 * gx.GRAD_SCALE[np.dtype(NP[dtype])]:.2f})")
    assert worst <= 4 * gx.GRAD_SCALE[np.dtype(NP[dtype])], (name, worst)


@pytest.mark.parametrize("name", VJP_CASES)
def test_vjp_against_central_differences_f64(name):
    metric, grades, N, _ = CASES[name]
    n = len(metric)
    A = np.array(reference(name, 3.0)[0][:VB])
    rng = np.random.default_rng(SEED + 8)
    g = rng.uniform(-1, 1, A.shape)
    v = gx.restrict(metric, grades, rng.uniform(-1, 1, A.shape))
    spec = inp(0, grades, n).gexp().specialize(ga.MetricAlgebra(metric))
    grad = gx.to_s(metric, grades, spec.vjp(0).eval_batch([op_rows(metric, grades, A, ga.F64)], gx.from_s(metric, grades, g), VB).download_rows())
    f = lambda X: gx.forward(metric, grades, X, np.longdouble, s_dtype=np.float64)[0].astype(np.float64)
    jv = (f(A + 1e-6 * v) - f(A - 1e-6 * v)) / 2e-6
    lhs, rhs, scale = (g * jv).sum(axis=1), (grad * v).sum(axis=1), (np.abs(g) * np.abs(jv)).sum(axis=1)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reduce_sums_the_gradient_of_a_shared_generator(dtype):
    metric, B = PGA, 1025
    rng = np.random.default_rng(SEED + 9)
    brow = op_rows(metric, [2], gx.random_operand(metric, [2], 1, 2.0, rng), dtype)
    x = rng.uniform(-1, 1, (B, 4)).astype(NP[dtype])
    b, X = inp(0, [2], 4), inp(1, [3], 4)
    R = b.gexp()
    spec = (R * X * R.rev()).g(3).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    g = rng.uniform(-1, 1, (B, 4)).astype(NP[dtype])
    shared = ga.DeviceMV.from_rows(4, [2], brow, dtype)
    per = spec.vjp(0).eval_batch([shared, x], g, B).download_rows().astype(np.float64)
    tot = spec.vjp(0).eval_batch([shared, x], g, B, reduce=True).download_rows().astype(np.float64)
    assert per.shape == (B, 6) and tot.shape == (1, 6)
    exact = np.array([math.fsum(per[:, j]) for j in range(6)])
    bound = (1024 + math.ceil(B / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)      # tests/test_gpu_gram_vjp.py: the row sum's bound
    assert np.all(np.abs(tot[0] - exact) <= bound)


def test_torch_fits_a_motor_generator_from_five_point_correspondences():
    import torch
    metric = PGA
    rng = np.random.default_rng(SEED + 10)
    pts = np.concatenate([rng.uniform(-1, 1, (5, 3)), np.ones((5, 1))], axis=1)      # grade 3 of PGA3D: e012, e013, e023 and the weight e123
    b_true = gx.from_s(metric, [2], gx.random_operand(metric, [2], 1, 1.5, rng), [2])
    b0 = gx.from_s(metric, [2], gx.random_operand(metric, [2], 1, 0.5, rng), [2])
    b, X = inp(0, [2], 4), inp(1, [3], 4)
    R = b.gexp()
    spec = (R * X * R.rev()).g(3).specialize(ga.MetricAlgebra(metric))
    fn = spec.torch_fn()
    xt = torch.tensor(pts, device="cuda")
    target = fn(torch.tensor(b_true, device="cuda"), xt).detach()
    gen = torch.tensor(b0, device="cuda", requires_grad=True)
    loss = ((fn(gen, xt) - target) ** 2).sum()
    loss.backward()
    torch.cuda.synchronize()
    grad = gen.grad.cpu().numpy()
    assert grad.shape == (1, 6) and np.isfinite(grad).all() and np.abs(grad).max() > 0
    # gradcheck-style: the directional derivative of the loss against central differences
    def loss_at(rows):
        with torch.no_grad():
            return float(((fn(torch.tensor(rows, device="cuda"), xt) - target) ** 2).sum())
    v = rng.uniform(-1, 1, (1, 6))
    num = (loss_at(b0 + 1e-6 * v) - loss_at(b0 - 1e-6 * v)) / 2e-6
    assert abs(num - float((grad * v).sum())) <= 1e-6 * max(1.0, np.abs(grad * v).sum())
    # the per-item gradient through vjp + reduce is the same number
    res = (fn(gen, xt) - target).detach().cpu().numpy()
    tot = spec.vjp(0).eval_batch([ga.DeviceMV.from_rows(4, [2], b0), pts], 2.0 * res, 5, reduce=True).download_rows()
    assert np.allclose(tot, grad, rtol=1e-10, atol=1e-12)
    # one gradient step decreases the loss
    l0 = float(loss.detach())
    step = 0.1 * l0 / float((grad ** 2).sum())
    assert loss_at(b0 - step * grad) < l0


# ---- 6. a Gram basis ----------------------------------------------------------------------------------------------------------------
def test_gexp_in_the_cga_null_basis():
    """exp commutes with the change of basis: forward against mpmath.expm of the caller-basis left-multiplication matrix (Chevalley's
    recursion, tests/clifford_gram.py: no diagonalisation), and the adjoint identity.  On top of the contract the rows go through the
    compounds of Q on the way in and out: the allowance of the existing Gram tests (1e-12 in f64, norm-wise)"""
    import mpmath as mp
    n, N, B, theta = 5, 32, 4, 2.0
    alg, cl = ga.GramAlgebra(CGA_GRAM), GramClifford(CGA_GRAM)
    assert not alg.identity_basis()
    order = np.array(inu.row_blades(n, tuple(full(n))))
    rng = np.random.default_rng(SEED + 11)
    x = rng.uniform(-1, 1, (B, 32))
    x *= theta / np.abs(x).sum(axis=1, keepdims=True)
    to_bits = lambda r: np.stack([np.bincount(order, weights=row, minlength=1 << n) for row in r])

    def expm_rows(rows, exact):
        out = np.zeros((rows.shape[0], 1 << n))
        for i, r in enumerate(to_bits(rows)):
            L = sum(r[S] * cl.left(S) for S in range(1 << n))
            if exact:
                with mp.workdps(50):
                    E = mp.expm(mp.matrix(L.tolist()))
                    out[i] = [float(E[k, 0]) for k in range(1 << n)]
            else:      # float64 Taylor after scaling by 2^-10: smooth in the operand, for central differences
                M, T, P = L / 1024.0, np.eye(1 << n), np.eye(1 << n)
                for k in range(1, 12):
                    P = P @ M / k
                    T = T + P
                for _ in range(10):
                    T = T @ T
                out[i] = T[:, 0]
        return out[:, order]

    spec = inp(0, full(n), n).gexp().specialize(alg)
    got = run(spec, [x], B)
    assert len(gexp_launches(spec)) == 1 and spec.domain_errors() == 0
    want = expm_rows(x, True)
    # theta of the orthogonal basis: the null vectors are (e+ +- e-) / sqrt 2 combinations, |components| grow by at most 2^(k/2) <= 4
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= (2 * N * EPS[ga.F64] * 4 * theta + 1e-12) * np.abs(want).max(axis=1)), (err / np.abs(want).max(axis=1)).max()
    v, g = rng.uniform(-1, 1, x.shape), rng.uniform(-1, 1, got.shape)
    grad = spec.vjp(0).eval_batch([x], g, B).download_rows()
    lhs, rhs, scale = inu.adjoint_identity(lambda r: expm_rows(r, False), x, v, g, grad)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()
