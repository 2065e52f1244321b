"""gaast_compound_matrix_vjp on the host: the reverse mode of the k-th compound with respect to the matrix, against an
independent numpy evaluation whose cofactors are np.linalg.det of the deleted sub-minors, and against central differences.
No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga

PD = C.POINTER(C.c_double)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blades(n, k):
    """the vectors of every grade-k blade, in the library's component order (colex rank = ascending bit mask)"""
    masks = sorted(sum(1 << i for i in c) for c in itertools.combinations(range(n), k))
    return [[i for i in range(n) if (m >> i) & 1] for m in masks]


def compound(m, k):
    n = m.shape[0]
    d = len(blades(n, k))
    out = np.zeros((d, d))
    m = np.ascontiguousarray(m, dtype=np.float64)
    assert ga.lib().gaast_compound_matrix(n, m.ctypes.data_as(PD), k, out.ctypes.data_as(PD)) == 0
    return out


def vjp(m, k, w, into=None):
    n = m.shape[0]
    dm = np.zeros((n, n)) if into is None else into
    m = np.ascontiguousarray(m, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    assert ga.lib().gaast_compound_matrix_vjp(n, k, m.ctypes.data_as(PD), w.ctypes.data_as(PD), dm.ctypes.data_as(PD)) == 0
    return dm


def numpy_vjp(m, k, w):
    """(dM, sum |w| |minor| per entry) from np.linalg.det of the deleted sub-minors"""
    n = m.shape[0]
    dm, mag = np.zeros((n, n)), np.zeros((n, n))
    bl = blades(n, k)
    for (a, I), (b, J) in itertools.product(enumerate(bl), repeat=2):
        for (pi, i), (pj, j) in itertools.product(enumerate(I), enumerate(J)):
            rows, cols = [r for r in I if r != i], [c for c in J if c != j]
            minor = np.linalg.det(m[np.ix_(rows, cols)]) if rows else 1.0
            dm[i, j] += (-1.0) ** (pi + pj) * minor * w[a, b]
            mag[i, j] += abs(minor * w[a, b])
    return dm, mag


def matrices(n, rng):
    out = [("random", rng.uniform(-1, 1, (n, n)))]
    # rank n - 1 (det = 0 up to rounding) with generic sub-minors: a minor that vanishes EXACTLY (two equal columns) would leave
    # np.linalg.det's LU rounding noise as both the reference value and its own magnitude
    s = rng.uniform(-1, 1, (n, n - 1)) @ rng.uniform(-1, 1, (n - 1, n)) if n > 1 else np.zeros((1, 1))
    out.append(("singular", s))
    z = rng.uniform(-1, 1, (n, n))
    z[n // 2, :] = 0.0
    out.append(("zero_row", z))
    return out


@pytest.mark.parametrize("n", range(1, 7))
def test_against_determinants_of_the_deleted_minors(n):
    rng = np.random.default_rng(100 + n)
    for name, m in matrices(n, rng):
        for k in range(n + 1):
            d = len(blades(n, k))
            w = rng.uniform(-1, 1, (d, d))
            got = vjp(m, k, w)
            want, mag = numpy_vjp(m, k, w) if k else (np.zeros((n, n)), np.zeros((n, n)))
            err = np.abs(got - want)
            assert np.all(err <= 1e-12 * mag), (name, n, k, err.max(), mag.max())


def test_it_adds_to_dmatrix_and_grade_zero_adds_nothing():
    rng = np.random.default_rng(7)
    m = rng.uniform(-1, 1, (3, 3))
    base = rng.uniform(-1, 1, (3, 3))
    assert np.array_equal(vjp(m, 0, np.ones((1, 1)), into=base.copy()), base)
    w = rng.uniform(-1, 1, (3, 3))
    assert np.array_equal(vjp(m, 1, w, into=base.copy()), base + w)     # C_0 = 1: grade 1 adds W itself
    one = vjp(m, 2, w)
    assert np.allclose(vjp(m, 2, w, into=base.copy()), base + one, rtol=0, atol=1e-15)


def test_sum_over_grades_is_the_central_difference_at_n_2():
    """L(M) = sum_k <W_k, C_k(M)> is a polynomial of degree <= 2 in the entries at n = 2: central differences are exact up to
    rounding.  |L| <= ~8, h = 2^-10: the rounding of the quotient is ~ 8 * 2^-53 / 2^-10 = 2^-40; tolerance 2^-36."""
    rng = np.random.default_rng(11)
    n, h = 2, 2.0 ** -10
    m = rng.uniform(-1, 1, (n, n))
    ws = [rng.uniform(-1, 1, (len(blades(n, k)),) * 2) for k in range(n + 1)]
    L = lambda mm: sum(float(np.sum(ws[k] * compound(mm, k))) for k in range(n + 1))
    dm = np.zeros((n, n))
    for k in range(n + 1):
        vjp(m, k, ws[k], into=dm)
    for i, j in itertools.product(range(n), repeat=2):
        e = np.zeros((n, n))
        e[i, j] = h
        fd = (L(m + e) - L(m - e)) / (2 * h)
        assert abs(fd - dm[i, j]) <= 2.0 ** -36, (i, j, fd, dm[i, j])


def test_bad_arguments():
    m = np.eye(3)
    w = np.zeros((3, 3))
    dm = np.zeros((3, 3))
    f = ga.lib().gaast_compound_matrix_vjp
    assert f(3, 4, m.ctypes.data_as(PD), w.ctypes.data_as(PD), dm.ctypes.data_as(PD)) == 6
    assert f(0, 0, m.ctypes.data_as(PD), w.ctypes.data_as(PD), dm.ctypes.data_as(PD)) == 6
    assert f(3, 1, None, w.ctypes.data_as(PD), dm.ctypes.data_as(PD)) == 6


def test_term_table_under_sanitizers(tmp_path):
    """tests/cpp/linmap_vjp_driver.cpp: the host function and the term-table builder for n = 1 ... 8 as a stand-alone program
    compiled with -fsanitize=address,undefined (every (I, J, i, j) exactly once, every index in range)."""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path / "linmap_vjp_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(csrc, "common"),
           os.path.join(ROOT, "tests", "cpp", "linmap_vjp_driver.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("ALL OK")
