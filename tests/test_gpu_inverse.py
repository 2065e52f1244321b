"""The general multivector inverse (Expr.inv(), a / b, GAAST_OP_INV; kernel k_mv_inverse<T, N>) on the GPU, against the numpy
reference of inverse_numpy.py (numpy.linalg.solve on the left-multiplication matrix built from bitmasks).

Bounds.  The contract of include/gaast_hip.h: per non-singular item the normwise backward error
||L_A y - e||_inf / (||L_A||_inf ||y||_inf) is at most 2 N eps -- the scale of Gaussian elimination with partial pivoting, N the
size of the blade set, eps that of the dtype.  The residual is evaluated in float64 on the operand exactly as the kernel saw it
(rounded to the dtype).  Inputs: default_rng(20261019), components U(-1, 1), the scalar part replaced by +-U(1, 2); for this recipe,
at batch 1000, no item is singular, condition numbers stay below 9e4, and LAPACK's own backward error in the same dtype is at most
0.52 N eps.  The ratio of the GPU's worst backward error to LAPACK's is printed per case (a record), never
asserted.  Forward comparisons (inv against vinv, f32 against f64 gradients) use the forward bound the contract implies,
backward error times the 2-norm condition number from numpy.  Signed permutations and scalar rows are exact: bits.
Reverse mode: the adjoint identity <g, J v> = <J^T g, v> with J v by central differences of the numpy reference in float64 (step
1e-6 on O(1) data: the differencing error, about 1e-10 cond, dominates), relative tolerance 1e-6 of sum |g_i (J v)_i|."""
import math

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

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
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
CGA_GRAM = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)


def even(n):
    return list(range(0, n + 1, 2))


def full(n):
    return list(range(n + 1))


# name -> (metric, operand grades, N)
CASES = {
    "R1": ([1.0], full(1), 2),
    "R2": ([1.0] * 2, full(2), 4),
    "R3": ([1.0] * 3, full(3), 8),
    "R3-even": ([1.0] * 3, even(3), 4),
    "PGA3D": (PGA, full(4), 16),
    "PGA3D-even": (PGA, even(4), 8),
    "CGA": (CGA, full(5), 32),
    "R33": ([1.0] * 3 + [-1.0] * 3, full(6), 64),
    "R7-even": ([1.0] * 7, even(7), 64),
}
_ROWS = {}


def inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def rows_of(name, batch=1000):
    """the issue's recipe, drawn once per case at batch 1000 (float64); smaller batches are its leading rows"""
    if name not in _ROWS:
        metric, grades, _ = CASES[name]
        rng = np.random.default_rng(SEED)
        rows = rng.uniform(-1, 1, (1000, len(inu.row_blades(len(metric), tuple(grades)))))
        rows[:, 0] = rng.choice([-1.0, 1.0], 1000) * rng.uniform(1, 2, 1000)     # grade 0 is the first component of every case
        rows.setflags(write=False)
        _ROWS[name] = rows
    return _ROWS[name][:batch]


def run(spec, rows, batch):
    out = spec.eval_batch(rows, batch)
    ga.lib().gaast_hip_synchronize()
    return out.download_rows()


def inverse_launches(spec):
    return [s for s in spec.launches() if "k_mv_inverse<" in s]


def check_contract(metric, grades, rows_dt, got, N, dtype, out_grades=None):
    """backward error of every item against 2 N eps; returns the worst"""
    n = len(metric)
    y = inu.full_y(n, tuple(grades), got, out_grades)
    be = inu.backward_error(metric, grades, np.asarray(rows_dt, dtype=np.float64), y)
    assert np.all(np.isfinite(got))
    assert np.all(be <= 2 * N * EPS[dtype]), (be.max() / (N * EPS[dtype]), int(np.argmax(be)))
    return float(be.max())


# ---- 1. the contract --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_error_contract(name, dtype):
    metric, grades, N = CASES[name]
    n = len(metric)
    spec = inp(0, grades, n).inv().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    hits = inverse_launches(spec)
    assert len(hits) == 1 and f"k_mv_inverse<{TY[dtype]},{N}>" in hits[0], spec.launches()
    assert len(spec.launches()) == 1
    for batch in (1, 7, 64 // N + 1, 1000):
        rows = rows_of(name, batch).astype(NP[dtype])
        got = run(spec, [rows], batch)
        assert got.shape == (batch, len(inu.row_blades(n, inu.result_grades(n, tuple(grades)))))
        worst = check_contract(metric, grades, rows, got, N, dtype)
        assert spec.domain_errors() == 0
        if batch == 1000:
            lap = inu.inverse_rows(metric, grades, rows, dtype=NP[dtype])
            lap_be = inu.backward_error(metric, grades, rows.astype(np.float64), inu.full_y(n, tuple(grades), lap)).max()
            print(f"RATIO {name} {TY[dtype]} N={N}: gpu {worst / (N * EPS[dtype]):.4f} N eps, lapack {lap_be / (N * EPS[dtype]):.4f} N eps, "
                  f"ratio {worst / lap_be:.3f}")


# ---- 2. exact cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scalar_in_a_mixed_row_is_exact(dtype):
    n, grades = 3, full(3)
    s = np.array([3.0, -7.0, 0.3, 1e-3, -1.7e5], dtype=NP[dtype])
    rows = np.zeros((len(s), 8), dtype=NP[dtype])
    rows[:, 0] = s
    got = run(inp(0, grades, n).inv().specialize(ga.MetricAlgebra([1.0] * n), dtype=dtype), [rows], len(s))
    assert np.array_equal(np.ascontiguousarray(got[:, 0]).view(np.uint8), (NP[dtype](1) / s).view(np.uint8))
    assert np.all(got[:, 1:] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "CGA", "R33"])
def test_unit_square_blades_are_their_own_inverse_up_to_the_sign_of_the_square(name, dtype):
    metric, grades, N = CASES[name]
    n = len(metric)
    blades = inu.row_blades(n, tuple(grades))
    rows = np.eye(len(blades), dtype=NP[dtype])
    got = run(inp(0, grades, n).inv().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], len(blades))
    want = np.diag([inu.coeff(b, b, metric) for b in blades]).astype(NP[dtype])    # e_b e_b = +-1: inv(e_b) = e_b / (e_b e_b)
    assert np.all(np.abs(np.diag(want)) == 1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_inverse_of_twice_e12(dtype):
    rows = np.array([[0.0, 0.0, 0.0, 2.0]], dtype=NP[dtype])
    got = run(inp(0, full(2), 2).inv().specialize(ga.MetricAlgebra([1.0, 1.0]), dtype=dtype), [rows], 1)
    assert np.array_equal(got, np.array([[0.0, 0.0, 0.0, -0.5]], dtype=NP[dtype]))


# ---- 3. agreement with vinv -------------------------------------------------------------------------------------------------------
def rotors(n, k, batch, seed):
    """normalised products of k vectors, as rows over the even grades up to k (float64)"""
    rng = np.random.default_rng(seed)
    metric = [1.0] * n
    grades = list(range(0, k + 1, 2))
    acc, ag = rng.uniform(-1, 1, (batch, n)), [1]
    for i in range(1, k):
        ng = sorted({g for a in ag for g in (a - 1, a + 1) if 0 <= g <= n})
        acc, ag = inu.gp_rows(metric, ag, acc, [1], rng.uniform(-1, 1, (batch, n)), ng), ng
    assert ag == grades
    norm = np.sqrt(np.abs(inu.gp_rows(metric, ag, acc, ag, reverse_rows(n, ag, acc), [0])[:, 0]))
    return acc / norm[:, None], grades


def reverse_rows(n, grades, rows):
    sign = np.array([-1.0 if inu.grade(b) % 4 in (2, 3) else 1.0 for b in inu.row_blades(n, tuple(grades))])
    return rows * sign[None]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,k", [(3, 2), (5, 4), (6, 4)])
def test_inv_agrees_with_vinv_on_rotors(n, k, dtype):
    metric = [1.0] * n
    rows64, grades = rotors(n, k, 33, 100 + n)
    rows = rows64.astype(NP[dtype])
    N = 1 << (n - 1)
    a = inp(0, grades, n)
    y = run(a.inv().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], 33).astype(np.float64)
    v = run(a.vinv().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], 33).astype(np.float64)
    _, cond = inu.norms(metric, grades, rows)
    yv = inu.full_y(n, tuple(grades), v, grades)      # vinv holds the operand's grades; the others of the even set are 0
    yi = inu.full_y(n, tuple(grades), y)
    err = np.abs(yi - yv).max(axis=1)
    assert np.all(err <= 2 * N * EPS[dtype] * cond * np.abs(yi).max(axis=1)), (err / (N * EPS[dtype] * cond)).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vinv_is_wrong_where_inv_is_right(dtype):
    """1 + e12 + e34 in R^4 is no versor (e12 and e34 commute, A ~A is not scalar): A vinv(A) is far from 1, inv meets the contract"""
    n, grades, metric = 4, even(4), [1.0] * 4
    blades = inu.row_blades(n, tuple(grades))
    rows = np.zeros((1, len(blades)), dtype=NP[dtype])
    for b in (0, 0b0011, 0b1100):
        rows[0, blades.index(b)] = 1.0
    a = inp(0, grades, n)
    v = run(a.vinv().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], 1)
    y = run(a.inv().specialize(ga.MetricAlgebra(metric), dtype=dtype), [rows], 1)
    one = np.zeros((1, len(blades)))
    one[0, 0] = 1.0
    assert np.abs(inu.gp_rows(metric, grades, rows, grades, v, grades) - one).max() > 0.1
    check_contract(metric, grades, rows, y, 8, dtype)
    norm_l, _ = inu.norms(metric, grades, rows)
    assert np.abs(inu.gp_rows(metric, grades, rows, grades, y, grades) - one).max() <= 2 * 8 * EPS[dtype] * norm_l[0] * np.abs(y).max()


# ---- 4. singular items ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_singular_items_are_nan_and_counted(dtype):
    metric, grades, N = CASES["PGA3D"]
    rows = np.array(rows_of("PGA3D", 40), dtype=NP[dtype])
    e0 = inu.row_blades(4, tuple(grades)).index(0b0001)
    bad = [3, 4, 17, 39]
    rows[bad] = 0
    rows[[3, 39], e0] = [1.0, -2.5]            # the ideal vector e0 (e0 e0 = 0); rows 4 and 17 stay the zero multivector
    spec = inp(0, grades, 4).inv().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    got = run(spec, [rows], 40)
    nan_rows = np.isnan(got).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == bad and not np.isnan(got[~nan_rows]).any()
    assert spec.domain_errors() == len(bad)
    assert spec.domain_errors() == 0
    check_contract(metric, grades, rows[~nan_rows], got[~nan_rows], N, dtype)
    # the null sum 1 + e1 in R^1, (1 + e1)(1 - e1) = 0: the second pivot is an exact zero
    r1 = np.array([[1.0, 1.0], [1.5, 0.25], [-2.0, 2.0], [1.0, -1.0], [0.5, 3.0]], dtype=NP[dtype])
    s1 = inp(0, [0, 1], 1).inv().specialize(ga.MetricAlgebra([1.0]), dtype=dtype)
    g1 = run(s1, [r1], 5)
    assert list(np.isnan(g1).all(axis=1)) == [True, False, True, True, False] and not np.isnan(g1[[1, 4]]).any()
    assert s1.domain_errors() == 3 and s1.domain_errors() == 0
    check_contract([1.0], [0, 1], r1[[1, 4]], g1[[1, 4]], 2, dtype)


# ---- 5. wanted grades and composition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wanted_grades_and_division(dtype):
    metric, grades, N = CASES["PGA3D"]
    alg = ga.MetricAlgebra(metric)
    B = 37
    rows = rows_of("PGA3D", B).astype(NP[dtype])
    brow = np.random.default_rng(5).uniform(-1, 1, (B, 16)).astype(NP[dtype])
    a, b = inp(0, grades, 4), inp(1, grades, 4)
    whole = run(a.inv().specialize(alg, dtype=dtype), [rows], B)
    s2 = a.inv().g(2).specialize(alg, dtype=dtype)
    g2 = run(s2, [rows], B)
    assert s2.output_info() == (1 << 2, 6) and len(inverse_launches(s2)) == 1
    assert np.array_equal(g2, whole[:, 5:11])
    # b / a and 1 / a are b * inv(a) and 1 * inv(a)
    ref = run((b * a.inv()).specialize(alg, dtype=dtype), [rows, brow], B)
    assert np.array_equal(run((b / a).specialize(alg, dtype=dtype), [rows, brow], B), ref)
    one = run((1 / a).specialize(alg, dtype=dtype), [rows], B)
    assert np.array_equal(one, run((ga.Expr._lift(1.0) * a.inv()).specialize(alg, dtype=dtype), [rows], B))
    check_contract(metric, grades, rows, one, N, dtype)
    # a * inv(a) = 1 within the contract times ||L_A|| ||y||
    prod = run((a * a.inv()).specialize(alg, dtype=dtype), [rows], B).astype(np.float64)
    norm_l, _ = inu.norms(metric, grades, rows)
    prod[:, 0] -= 1.0
    assert np.all(np.abs(prod).max(axis=1) <= 2 * N * EPS[dtype] * norm_l * np.abs(whole).max(axis=1))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_inverse_inside_a_program_under_every_plan_form(dtype):
    """(a + b).inv() * c: the INV step is a launch of its own whatever the flags, its contribution has the same bits in every plan,
    and the whole stays within the product kernels' tolerance (4 eps sum |terms|) of the product of that inverse with c"""
    metric, grades, N = CASES["PGA3D"]
    alg = ga.MetricAlgebra(metric)
    B = 67
    rng = np.random.default_rng(6)
    ar = rows_of("PGA3D", B).astype(NP[dtype])
    br = (0.25 * rng.uniform(-1, 1, (B, 16)) * (np.arange(16) != 0)[None]).astype(NP[dtype])      # a perturbation off the scalar part
    cr = rng.uniform(-1, 1, (B, 16)).astype(NP[dtype])
    a, b, c = inp(0, grades, 4), inp(1, grades, 4), inp(2, grades, 4)
    flags = [0, _lib.FLAG_NO_FUSION, _lib.FLAG_NO_JIT, _lib.FLAG_DEBUG_JIT_FAILS]
    invs, outs = [], []
    for f in flags:
        si = (a + b).inv().specialize(alg, dtype=dtype, flags=f)
        assert len(inverse_launches(si)) == 1
        invs.append(run(si, [ar, br], B))
        sp = ((a + b).inv() * c).specialize(alg, dtype=dtype, flags=f)
        assert len(inverse_launches(sp)) == 1 and len(sp.launches()) >= 2, sp.launches()
        outs.append(run(sp, [ar, br, cr], B))
        assert sp.domain_errors() == 0
    for y in invs[1:]:
        assert np.array_equal(y.view(np.uint8), invs[0].view(np.uint8))
    check_contract(metric, grades, ar + br, invs[0], N, dtype)
    y64 = invs[0].astype(np.float64)
    want = inu.gp_rows(metric, grades, y64, grades, cr, grades)
    bound = 4 * EPS[dtype] * inu.gp_rows([abs(m) for m in metric], grades, np.abs(y64), grades, np.abs(cr), grades, absolute=True)
    for o in outs:
        assert np.all(np.abs(o - want) <= bound)


# ---- 6. row layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["R3", "R33"])
def test_strided_and_misaligned_rows(name, dtype):
    metric, grades, N = CASES[name]
    n, B = len(metric), 9
    rows = rows_of(name, B).astype(NP[dtype])
    spec = inp(0, grades, n).inv().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    want = run(spec, [rows], B)
    out_grades = inu.result_grades(n, tuple(grades))
    for lin, lout in (("pad_odd", "contig"), ("shift", "contig"), ("contig", "pad_odd"), ("contig", "shift")):
        p = place(rows, lin, dtype, n, grades)
        o = place_out(B, want.shape[1], lout, dtype, n, out_grades)
        spec.eval_batch([p.mv], B, out=o.mv)
        p.check()
        o.check()
        assert np.array_equal(o.rows().view(np.uint8), want.view(np.uint8)), (lin, lout)
    assert spec.launch_variants() == [0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shared_operand(dtype):
    metric, grades, N = CASES["PGA3D"]
    rows = rows_of("PGA3D", 1).astype(NP[dtype])
    spec = inp(0, grades, 4).inv().specialize(ga.MetricAlgebra(metric), dtype=dtype)
    one = run(spec, [rows], 1)
    many = run(spec, [ga.DeviceMV.from_rows(4, grades, rows, dtype)], 257)
    assert many.shape == (257, 16)
    assert np.array_equal(many.view(np.uint8), np.repeat(one, 257, axis=0).view(np.uint8))
    check_contract(metric, grades, rows, one, N, dtype)


# ---- 7. unsupported sizes ---------------------------------------------------------------------------------------------------------
def test_more_than_64_blades_is_unimplemented():
    for n, grades in ((7, [0, 1]), (7, full(7)), (8, even(8))):
        spec = inp(0, grades, n).inv().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed
        with pytest.raises(_lib.GaastError) as e:
            spec.program()
        assert e.value.status_name == "UNIMPLEMENTED"
    metric, grades, N = CASES["R3"]
    rows = rows_of("R3", 5)
    got = run(inp(0, grades, 3).inv().specialize(ga.MetricAlgebra(metric)), [rows], 5)
    check_contract(metric, grades, rows, got, N, ga.F64)


# ---- 8. reverse mode --------------------------------------------------------------------------------------------------------------
VJP_CASES = ["PGA3D-even", "PGA3D", "CGA"]
VB = 12   # items of the reverse-mode cases (leading rows of the recipe: condition numbers of a few tens)


def vjp_inputs(name):
    metric, grades, N = CASES[name]
    n = len(metric)
    rng = np.random.default_rng(SEED + 1)
    x = np.array(rows_of(name, VB))
    out_len = len(inu.row_blades(n, inu.result_grades(n, tuple(grades))))
    return x, rng.uniform(-1, 1, x.shape), rng.uniform(-1, 1, (VB, out_len))


@pytest.mark.parametrize("name", VJP_CASES)
def test_adjoint_identity_f64(name):
    metric, grades, N = CASES[name]
    n = len(metric)
    x, v, g = vjp_inputs(name)
    spec = inp(0, grades, n).inv().specialize(ga.MetricAlgebra(metric))
    grad = spec.vjp(0).eval_batch([x], g, VB).download_rows()
    assert len([s for s in spec.vjp(0).launches() if "k_mv_inverse<double," in s]) == 1
    lhs, rhs, scale = inu.adjoint_identity(lambda r: inu.inverse_rows(metric, grades, r), x, v, g, grad)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


@pytest.mark.parametrize("name", VJP_CASES)
def test_f32_gradient_rows_against_f64(name):
    metric, grades, N = CASES[name]
    n = len(metric)
    x, _, g = vjp_inputs(name)
    x32, g32 = x.astype(np.float32), g.astype(np.float32)
    a = inp(0, grades, n)
    g64 = a.inv().specialize(ga.MetricAlgebra(metric)).vjp(0).eval_batch([x32.astype(np.float64)], g32.astype(np.float64), VB).download_rows()
    got = a.inv().specialize(ga.MetricAlgebra(metric), dtype=ga.F32).vjp(0).eval_batch([x32], g32, VB).download_rows().astype(np.float64)
    _, cond = inu.norms(metric, grades, x32)
    err = np.abs(got - g64).max(axis=1)
    assert np.all(err <= 64 * N * EPS[ga.F32] * cond * np.abs(g64).max(axis=1)), (err / (N * EPS[ga.F32] * cond * np.abs(g64).max(axis=1))).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reduce_sums_the_gradient_of_a_shared_divisor(dtype):
    metric, grades, N = CASES["PGA3D-even"]
    B = 1025
    rng = np.random.default_rng(9)
    a_row = rows_of("PGA3D-even", 1).astype(NP[dtype])
    x = rng.uniform(-1, 1, (B, 4)).astype(NP[dtype])
    g = rng.uniform(-1, 1, (B, 8)).astype(NP[dtype])
    spec = (inp(0, [1], 4) / inp(1, grades, 4)).specialize(ga.MetricAlgebra(metric), dtype=dtype)
    assert spec.output_info()[1] == 8      # vector times even: grades 1 and 3
    shared = ga.DeviceMV.from_rows(4, grades, a_row, dtype)
    per = spec.vjp(1).eval_batch([x, shared], g, B).download_rows().astype(np.float64)
    tot = spec.vjp(1).eval_batch([x, shared], g, B, reduce=True).download_rows().astype(np.float64)
    assert per.shape == (B, 8) and tot.shape == (1, 8)
    exact = np.array([math.fsum(per[:, j]) for j in range(8)])
    bound = (1024 + math.ceil(B / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)      # tests/test_gpu_gram_vjp.py: the row sum's bound
    assert np.all(np.abs(tot[0] - exact) <= bound)


def test_torch_backward_of_a_quotient():
    import torch
    metric, grades, N = CASES["PGA3D-even"]
    B = 19
    rng = np.random.default_rng(10)
    a_rows, x_rows = np.array(rows_of("PGA3D-even", B)), rng.uniform(-1, 1, (B, 4))
    spec = (inp(0, [1], 4) / inp(1, grades, 4)).specialize(ga.MetricAlgebra(metric))
    x = torch.tensor(x_rows, device="cuda", requires_grad=True)
    a = torch.tensor(a_rows, device="cuda", requires_grad=True)
    spec.torch_fn()(x, a).sum().backward()
    torch.cuda.synchronize()
    ones = np.ones((B, 8))
    gx = spec.vjp(0).eval_batch([x_rows, a_rows], ones, B).download_rows()
    gA = spec.vjp(1).eval_batch([x_rows, a_rows], ones, B).download_rows()
    assert np.array_equal(x.grad.cpu().numpy(), gx) and np.array_equal(a.grad.cpu().numpy(), gA)
    # ... and they are the gradient: d/dA sum(x inv(A)) against central differences of the numpy reference
    f = lambda r: inu.gp_rows(metric, [1], x_rows, grades, inu.inverse_rows(metric, grades, r), [1, 3])
    v = rng.uniform(-1, 1, a_rows.shape)
    jv = inu.jvp_central(f, a_rows, v)
    lhs, rhs = jv.sum(axis=1), np.einsum("ij,ij->i", gA, v)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * np.abs(jv).sum(axis=1))


def gram_solve(cl, n, rows):
    """the inverse in the caller's (non-orthogonal) basis by numpy: the left-multiplication matrix of tests/clifford_gram.py"""
    out = np.zeros((rows.shape[0], 1 << n))
    conds = []
    for i, r in enumerate(rows):
        L = sum(r[S] * cl.left(S) for S in range(1 << n))
        e = np.zeros(1 << n)
        e[0] = 1.0
        out[i] = np.linalg.solve(L, e)
        conds.append(np.linalg.cond(L))
    return out, np.array(conds)


def test_inverse_in_the_cga_null_basis():
    """forward against numpy in the caller's basis, and the adjoint identity.  The rows also go through the compounds of the
    orthogonal Q on the way in and out: on top of the contract's forward bound 2 N eps cond, the allowance of the existing Gram
    tests (tests/test_gpu_gram_metric.py: TOL = 1e-12 in f64, norm-wise)"""
    n, N, B = 5, 32, 8
    alg, cl = ga.GramAlgebra(CGA_GRAM), GramClifford(CGA_GRAM)
    assert not alg.identity_basis()
    order = np.array(inu.row_blades(n, tuple(full(n))))
    x = np.array(rows_of("CGA", B))
    to_bits = lambda r: np.stack([np.bincount(order, weights=row, minlength=1 << n) for row in r])
    spec = inp(0, full(n), n).inv().specialize(alg)
    got = run(spec, [x], B)
    assert len(inverse_launches(spec)) == 1 and spec.domain_errors() == 0
    want_bits, cond = gram_solve(cl, n, to_bits(x))
    want = want_bits[:, order]
    err = np.abs(got - want).max(axis=1)
    assert np.all(err <= (2 * N * EPS[ga.F64] * cond + 1e-12) * np.abs(want).max(axis=1)), (err / np.abs(want).max(axis=1)).max()
    rng = np.random.default_rng(SEED + 2)
    v, g = rng.uniform(-1, 1, x.shape), rng.uniform(-1, 1, got.shape)
    grad = spec.vjp(0).eval_batch([x], g, B).download_rows()
    lhs, rhs, scale = inu.adjoint_identity(lambda r: gram_solve(cl, n, to_bits(r))[0][:, order], x, v, g, grad)
    assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()
