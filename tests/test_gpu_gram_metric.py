"""Programs in non-diagonal (Gram) metrics on the GPU against the independent oracle of tests/clifford_gram.py, which works in the
caller's basis and never diagonalises."""
import ctypes as C

import numpy as np
import pytest

import gaast_amd as ga
from clifford_gram import GramClifford, blades_of_grade, mv_to_row, row_blades, row_to_mv

pytestmark = pytest.mark.gpu
NP = {ga.F32: np.float32, ga.F64: np.float64}
TOL = {ga.F64: 1e-12, ga.F32: 2e-5}
CGA_GRAM = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)


def random_gram(rng, n, kind):
    a = rng.uniform(-1, 1, (n, n))
    if kind == "indefinite":
        g = (a + a.T) / 2
    else:   # degenerate, indefinite, rank n - 2
        b = a[:, :n - 2]
        g = b @ np.diag(rng.choice([-1.0, 1.0], n - 2)) @ b.T
    g = (g + g.T) / 2
    return g / np.linalg.norm(g, 2)      # |G|_2 = 1: the row norms bound the products


def inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def rows_for(rng, n, grades, batch):
    return rng.uniform(-1, 1, (batch, len(row_blades(n, grades))))


def versor_rows(rng, cl, n, batch, k=2):
    """products of k vectors with |v.v| >= 0.2 |v|^2 (well-conditioned inverses), as full rows"""
    out = np.zeros((batch, 1 << n))
    for i in range(batch):
        v = np.zeros(1 << n)
        v[0] = 1.0
        for _ in range(k):
            while True:
                x = rng.uniform(-1, 1, n)
                if abs(x @ cl.B @ x) >= 0.2 * (x @ x):
                    break
            u = np.zeros(1 << n)
            u[[1 << j for j in range(n)]] = x
            v = cl.gp(v, u)
        out[i] = mv_to_row(n, range(n + 1), v)
    return out


# (name, input grades per slot, expression, oracle, how many operand norms the bound multiplies)
def cases(n):
    full, vec = list(range(n + 1)), [1]
    return [
        ("gp", [full, full], lambda a, b: a * b, lambda c, a, b: c.product(a, b, "gp")),
        ("op", [full, [1, 2]], lambda a, b: a ^ b, lambda c, a, b: c.product(a, b, "op")),
        ("ip", [[1, 2], full], lambda a, b: a & b, lambda c, a, b: c.product(a, b, "ip")),
        ("lc", [vec, full], lambda a, b: a << b, lambda c, a, b: c.product(a, b, "lc")),
        ("rc", [full, [2]], lambda a, b: a >> b, lambda c, a, b: c.product(a, b, "rc")),
        ("rev", [full], lambda a: a.rev(), lambda c, a: c.rev(a)),
        ("ginvol", [full], lambda a: a.ginvol(), lambda c, a: c.ginvol(a)),
        ("norm_sq", [full], lambda a: a.norm_sq(), lambda c, a: c.norm_sq(a)),
        ("a_plus_bc_g2", [full, full, full], lambda a, b, c: (a + b * c).g(2), lambda o, a, b, c: o.g(a + o.gp(b, c), 2)),
        ("sandwich_g1", [[0, 2], vec], lambda r, x: (r * x * r.rev()).g(1), lambda o, r, x: o.g(o.gp(o.gp(r, x), o.rev(r)), 1)),
    ]


def run_case(alg, cl, n, grades, build, oracle, dtype, batch, rng, rows=None):
    exprs = [inp(s, g, n) for s, g in enumerate(grades)]
    spec = build(*exprs).specialize(alg, dtype=dtype)
    if rows is None:
        rows = [rows_for(rng, n, g, batch) for g in grades]
    out = spec.eval_batch([r.astype(NP[dtype]) for r in rows], batch)
    ga.lib().gaast_hip_synchronize()
    got = out.download_rows().astype(np.float64)
    out_grades = [k for k in range(n + 1) if (out.mask >> k) & 1]
    for i in range(batch):
        args = [row_to_mv(n, g, r[i]) for g, r in zip(grades, rows)]
        want_mv = oracle(cl, *args)
        want = mv_to_row(n, out_grades, want_mv)
        assert np.abs(want_mv).sum() - np.abs(want).sum() <= 1e-12 * (1 + np.abs(want_mv).sum())   # nothing outside the mask
        bound = np.prod([np.linalg.norm(r[i]) for r in rows])
        yield got[i], want, bound, spec


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("kind", ["indefinite", "degenerate"])
@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_products_against_the_gram_oracle(n, kind, dtype):
    rng = np.random.default_rng(n * 7 + len(kind) + dtype)
    g = random_gram(rng, n, kind)
    alg, cl = ga.GramAlgebra(g), GramClifford(g)
    assert not alg.identity_basis()
    worst = {}
    for name, grades, build, oracle in cases(n):
        for got, want, bound, spec in run_case(alg, cl, n, grades, build, oracle, dtype, 9, rng):
            err = np.linalg.norm(got - want)
            worst[name] = max(worst.get(name, 0.0), err / bound)
            assert err <= TOL[dtype] * bound, (name, err, bound)
        assert any(l.startswith("linmap[") for l in spec.launches())


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("n", [3, 5])
def test_versor_inverse_in_a_gram_metric(n, dtype):
    rng = np.random.default_rng(n)
    g = random_gram(rng, n, "indefinite")
    alg, cl = ga.GramAlgebra(g), GramClifford(g)
    rows = versor_rows(rng, cl, n, 7)
    full = list(range(n + 1))
    for got, want, _, _ in run_case(alg, cl, n, [full], lambda a: a.vinv(), lambda c, a: c.vinv(a), dtype, 7, rng, rows=[rows]):
        assert np.linalg.norm(got - want) <= 100 * TOL[dtype] * np.linalg.norm(want)


def up_rows(xs):
    """conformal points e_o + x + x^2/2 e_inf as grade-1 rows of the null basis {e1, e2, e3, e_o, e_inf}"""
    return np.array([[x[0], x[1], x[2], 1.0, 0.5 * float(x @ x)] for x in xs])


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_cga_in_the_null_basis(dtype):
    rng = np.random.default_rng(11)
    alg = ga.GramAlgebra(CGA_GRAM)
    xs, ys = rng.uniform(-1, 1, (33, 3)), rng.uniform(-1, 1, (33, 3))
    X, Y = inp(0, [1], 5), inp(1, [1], 5)
    tol = TOL[dtype] * 10
    sq = (X * X).specialize(alg, dtype=dtype).eval_batch([up_rows(xs).astype(NP[dtype])], 33)
    assert np.abs(sq.download_rows()).max() <= tol
    dot = (X & Y).specialize(alg, dtype=dtype).eval_batch([up_rows(xs).astype(NP[dtype]), up_rows(ys).astype(NP[dtype])], 33)
    want = -0.5 * ((xs - ys) ** 2).sum(axis=1)
    assert np.abs(dot.download_rows()[:, 0] - want).max() <= tol
    # constant inputs (basis_vectors): e_o . e_inf = -1, e_o^2 = 0
    e = ga.Expr.basis_vectors(5)
    assert (e[3] & e[4]).specialize(alg, dtype=dtype).eval().grade_slice(0)[0] == pytest.approx(-1.0, abs=tol)
    assert np.abs((e[3] * e[3]).specialize(alg, dtype=dtype).eval().row()).max() <= tol
    # a constant times a batched input: e_inf . up(x) = -1
    r = (e[4] & X).specialize(alg, dtype=dtype).eval_batch([up_rows(xs).astype(NP[dtype])], 33).download_rows()
    assert np.abs(r[:, 0] + 1.0).max() <= tol


def test_shared_batch1_inputs():
    rng = np.random.default_rng(2)
    n = 4
    g = random_gram(rng, n, "indefinite")
    alg, cl = ga.GramAlgebra(g), GramClifford(g)
    full = list(range(n + 1))
    a_rows, b_row = rows_for(rng, n, full, 21), rows_for(rng, n, full, 1)
    spec = (inp(0, full, n) * inp(1, full, n)).specialize(alg)
    shared = ga.DeviceMV.from_rows(n, full, b_row)
    got = spec.eval_batch([a_rows, shared], 21).download_rows()
    for i in range(21):
        want = mv_to_row(n, full, cl.gp(row_to_mv(n, full, a_rows[i]), row_to_mv(n, full, b_row[0])))
        assert np.linalg.norm(got[i] - want) <= 1e-12 * np.linalg.norm(a_rows[i]) * np.linalg.norm(b_row[0])


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_diagonal_gram_is_the_plain_program(dtype):
    diag = [1.0, -1.0, 0.0, 2.0, 1.0]
    n = len(diag)
    rng = np.random.default_rng(4)
    full = list(range(n + 1))
    rows = [rows_for(rng, n, full, 50).astype(NP[dtype]) for _ in range(2)]
    build = lambda: (inp(0, full, n) * inp(1, full, n) + inp(0, full, n).rev()).g(2)
    s1 = build().specialize(ga.GramAlgebra(np.diag(diag)), dtype=dtype)
    s2 = build().specialize(ga.MetricAlgebra(diag), dtype=dtype)
    assert s1.launches() == s2.launches()
    assert not any("linmap" in l for l in s1.launches())
    assert np.array_equal(s1.eval_batch(rows, 50).download_rows(), s2.eval_batch(rows, 50).download_rows())


def compounds(m):
    n = m.shape[0]
    out = []
    for k in range(n + 1):
        d = len(blades_of_grade(n, k))
        c = np.zeros((d, d))
        mm = np.ascontiguousarray(m)
        assert ga.lib().gaast_compound_matrix(n, mm.ctypes.data_as(C.POINTER(C.c_double)), k, c.ctypes.data_as(C.POINTER(C.c_double))) == 0
        out.append(c)
    return out


def move(cs, rows):
    out, pos = np.empty_like(rows), 0
    for c in cs:
        d = c.shape[0]
        out[:, pos:pos + d] = rows[:, pos:pos + d] @ c.T
        pos += d
    return out


def test_r12_f32_full_product_against_the_plain_program():
    n, batch = 12, 64
    rng = np.random.default_rng(12)
    g = random_gram(rng, n, "indefinite")
    alg = ga.GramAlgebra(g)
    full = list(range(n + 1))
    q = alg.basis
    a, b = (rng.uniform(-1, 1, (batch, 1 << n)) for _ in range(2))
    build = lambda: inp(0, full, n) * inp(1, full, n)
    got = build().specialize(alg, dtype=ga.F32).eval_batch([a.astype(np.float32), b.astype(np.float32)], batch).download_rows()
    to_f, to_e = compounds(q.T), compounds(q)
    af, bf = move(to_f, a), move(to_f, b)
    plain = build().specialize(ga.MetricAlgebra(alg.diag), dtype=ga.F64).eval_batch([af, bf], batch).download_rows()
    want = move(to_e, plain)
    for i in range(batch):
        assert np.linalg.norm(got[i] - want[i]) <= TOL[ga.F32] * np.linalg.norm(a[i]) * np.linalg.norm(b[i])
