"""Non-diagonal metrics on the host: gaast_metric_diagonalize, gaast_compound_matrix, GramAlgebra, and the independent Clifford
oracle of tests/clifford_gram.py.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gaast_amd as ga
from clifford_gram import GEOMETRIC, GramClifford, blades_of_grade

PD = C.POINTER(C.c_double)
CGA_GRAM = np.array([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, -1], [0, 0, 0, -1, 0]], dtype=np.float64)


def diagonalize(g):
    g = np.ascontiguousarray(g, dtype=np.float64)
    n = g.shape[0]
    d = np.zeros(max(n, 1))
    q = np.zeros((max(n, 1), max(n, 1)))
    st = ga.lib().gaast_metric_diagonalize(n, g.ctypes.data_as(PD), d.ctypes.data_as(PD), q.ctypes.data_as(PD))
    return st, d[:n], q[:n, :n]


def compound(m, k):
    m = np.ascontiguousarray(m, dtype=np.float64)
    n = m.shape[0]
    d = len(blades_of_grade(n, k))
    out = np.zeros((d, d))
    assert ga.lib().gaast_compound_matrix(n, m.ctypes.data_as(PD), k, out.ctypes.data_as(PD)) == 0
    return out


def random_gram(rng, n, kind):
    a = rng.uniform(-1, 1, (n, n))
    if kind == "definite":
        return a @ a.T + 0.1 * np.eye(n)
    if kind == "indefinite":
        return (a + a.T) / 2
    # degenerate: rank n - 2 (n - 1 at n = 2), indefinite
    r = max(1, n - 2)
    b = a[:, :r]
    s = np.diag(rng.choice([-1.0, 1.0], r))
    return b @ s @ b.T


@pytest.mark.parametrize("n", range(2, 13))
@pytest.mark.parametrize("kind", ["definite", "indefinite", "degenerate"])
def test_diagonalize_random(n, kind):
    rng = np.random.default_rng(100 * n + len(kind))
    g = random_gram(rng, n, kind)
    g = (g + g.T) / 2          # exactly symmetric
    st, d, q = diagonalize(g)
    assert st == 0
    norm = np.linalg.norm(g, 2)
    assert np.abs(q.T @ g @ q - np.diag(d)).max() <= 1e-13 * norm
    assert np.abs(q.T @ q - np.eye(n)).max() <= 1e-13
    if kind == "degenerate":
        r = max(1, n - 2)
        assert np.count_nonzero(d == 0.0) == n - r, d
    # deterministic: identical bits on a second call
    st2, d2, q2 = diagonalize(g)
    assert d.tobytes() == d2.tobytes() and q.tobytes() == q2.tobytes()
    # sign convention: every column's largest-magnitude entry is positive
    for j in range(n):
        assert q[np.argmax(np.abs(q[:, j])), j] > 0


def test_diagonalize_cga_null_basis():
    st, d, q = diagonalize(CGA_GRAM)
    assert st == 0
    assert np.abs(q.T @ CGA_GRAM @ q - np.diag(d)).max() <= 1e-15
    assert sorted(d) == pytest.approx([-1, 1, 1, 1, 1])


@pytest.mark.parametrize("diag", [[1.0, -1.0, 0.0, 2.5], [3.0], [0.0, 0.0, 1e-300, -7.0, 1.0]])
def test_diagonal_gram_is_kept_bitwise(diag):
    g = np.diag(diag)
    st, d, q = diagonalize(g)
    assert st == 0
    assert np.array(diag).tobytes() == d.tobytes()
    assert np.eye(len(diag)).tobytes() == q.tobytes()


def test_bad_gram_is_refused():
    g = np.eye(3)
    g[0, 1] = 0.5
    assert diagonalize(g)[0] == 6                     # asymmetric
    g = np.eye(3)
    g[1, 1] = np.nan
    assert diagonalize(g)[0] == 6
    assert diagonalize(np.zeros((0, 0)))[0] == 6
    assert diagonalize(np.eye(17))[0] == 6
    with pytest.raises(ga.GaastError):
        ga.GramAlgebra([[1.0, 0.5], [0.25, 1.0]])


@pytest.mark.parametrize("n", range(1, 7))
def test_compound_matches_numpy_minors(n):
    rng = np.random.default_rng(n)
    m = rng.uniform(-1, 1, (n, n))
    L = ga.lib()
    for k in range(n + 1):
        c = compound(m, k)
        blades = [L.gaast_component_to_blade(n, k, i) for i in range(c.shape[0])]
        for I, bi in enumerate(blades):
            rows = [p for p in range(n) if (bi >> p) & 1]
            for J, bj in enumerate(blades):
                cols = [p for p in range(n) if (bj >> p) & 1]
                want = np.linalg.det(m[np.ix_(rows, cols)]) if k else 1.0
                assert c[I, J] == pytest.approx(want, abs=1e-13)


def test_compound_cauchy_binet():
    n = 8
    rng = np.random.default_rng(8)
    a, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    for k in range(n + 1):
        assert np.abs(compound(a @ b, k) - compound(a, k) @ compound(b, k)).max() <= 1e-11


def test_compound_bad_arguments():
    m = np.eye(3)
    out = np.zeros(9)
    L = ga.lib()
    assert L.gaast_compound_matrix(3, m.ctypes.data_as(PD), 4, out.ctypes.data_as(PD)) == 6
    assert L.gaast_compound_matrix(0, m.ctypes.data_as(PD), 0, out.ctypes.data_as(PD)) == 6


def test_gram_algebra_semantics():
    g = np.array([[2.0, 0.5, 0.0], [0.5, -1.0, 0.25], [0.0, 0.25, 0.0]])
    alg = ga.GramAlgebra(g)
    assert alg.vec_space_dim() == 3
    for i, j in itertools.product(range(3), repeat=2):
        assert alg.base_vec_dot(i, j) == g[i, j]
    st, d, q = diagonalize(g)
    assert list(alg.diag) == list(d) and np.array_equal(alg.basis, q)
    assert not alg.identity_basis()
    with pytest.raises(ValueError):
        alg.ortho_basis_blades_gp(1, 2)
    assert ga.algebra.as_algebra(alg) is alg
    # a diagonal Gram matrix is a MetricAlgebra of its diagonal
    dg = ga.GramAlgebra(np.diag([1.0, -1.0, 0.0]))
    assert dg.identity_basis() and dg.diag == [1.0, -1.0, 0.0]
    assert dg.ortho_basis_blades_gp(3, 2) == ga.MetricAlgebra([1.0, -1.0, 0.0]).ortho_basis_blades_gp(3, 2)
    # existing inputs of as_algebra behave as before
    assert type(ga.algebra.as_algebra(3)) is ga.OrthoEuclidN
    assert type(ga.algebra.as_algebra([1.0, -1.0])) is ga.MetricAlgebra


def test_gram_program_refuses_serialize():
    alg = ga.GramAlgebra(CGA_GRAM)
    a = ga.mv(ga.Input(0, [1], 5))
    b = ga.mv(ga.Input(1, [1], 5))
    spec = (a * b).specialize(alg)
    with pytest.raises(ValueError):
        spec.serialize()
    # Q == I: the wire format holds the whole program
    assert (a * b).specialize(ga.GramAlgebra(np.eye(5))).serialize()


# ---- the independent oracle checks itself --------------------------------------------------------------------------------

@pytest.mark.parametrize("diag", [[1.0, 1.0, 1.0], [1.0, -1.0, 0.0, 2.0], [0.5, -2.0, 1.0, 1.0, -1.0]])
def test_oracle_matches_blades_gp_on_diagonal_metrics(diag):
    n = len(diag)
    cl = GramClifford(np.diag(diag))
    alg = ga.MetricAlgebra(diag)
    for a in range(1 << n):
        for b in range(1 << n):
            res, coeff = alg.ortho_basis_blades_gp(a, b)
            want = np.zeros(1 << n)
            want[res] = coeff
            got = cl.gp(np.eye(1 << n)[a], np.eye(1 << n)[b])
            assert np.allclose(got, want, atol=1e-15), (a, b)


def test_oracle_cga_identities():
    cl = GramClifford(CGA_GRAM)
    e = [cl.basis_vector(i) for i in range(5)]
    eo, ei = e[3], e[4]
    assert cl.product(eo, ei, "ip")[0] == -1.0
    assert not cl.gp(eo, eo).any() and not cl.gp(ei, ei).any()
    rng = np.random.default_rng(5)

    def up(x):
        return x[0] * e[0] + x[1] * e[1] + x[2] * e[2] + 0.5 * float(x @ x) * ei + eo

    x, y = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    assert np.abs(cl.gp(up(x), up(x))).max() <= 1e-15
    assert cl.product(up(x), up(y), "ip")[0] == pytest.approx(-0.5 * float((x - y) @ (x - y)), abs=1e-15)
    # associativity and the vector rule in a random symmetric form
    g = random_gram(rng, 4, "indefinite")
    g = (g + g.T) / 2
    cl = GramClifford(g)
    a, b, c = (rng.uniform(-1, 1, 16) for _ in range(3))
    assert np.abs(cl.gp(cl.gp(a, b), c) - cl.gp(a, cl.gp(b, c))).max() <= 1e-13
    u, v = rng.uniform(-1, 1, 4), rng.uniform(-1, 1, 4)
    U = sum(u[i] * cl.basis_vector(i) for i in range(4))
    V = sum(v[i] * cl.basis_vector(i) for i in range(4))
    assert cl.gp(U, V)[0] == pytest.approx(float(u @ g @ v), abs=1e-15)
    assert cl.product(U, V, GEOMETRIC)[0] == pytest.approx(float(u @ g @ v), abs=1e-15)
