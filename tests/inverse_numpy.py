"""Independent numpy reference of the general multivector inverse (GAAST_OP_INV), on blade bitmasks.

For a multivector A of an algebra with diagonal metric `metric`, inv(A) is the Y with A Y = 1.  With S the even blades when A holds
only even grades and every blade otherwise, Y solves L_A y = e_scalar, where L_A is the left-multiplication matrix on S:

    L_A[c][b] = coeff(a, b) A[a],  a = c xor b,    e_a e_b = coeff(a, b) e_{a xor b}

coeff(a, b) = (-1)^#{(i in a, j in b): i > j} (the swaps that sort the product) times the metric entry of every basis vector a and
b share.  Everything here is computed from these lines by counting; nothing is shared with gaast_amd/csrc and no library call is
made.  Rows are the library's graded rows: grades ascending, ascending bitmask (colex order) within a grade.
"""
import functools

import numpy as np


def swaps(a, b, n):
    """#{(i in a, j in b): i > j}"""
    c = 0
    for i in range(n):
        if (a >> i) & 1:
            c += bin(b & ((1 << i) - 1)).count("1")
    return c


def coeff(a, b, metric):
    n = len(metric)
    c = -1.0 if swaps(a, b, n) & 1 else 1.0
    for i in range(n):
        if (a >> i) & (b >> i) & 1:
            c *= float(metric[i])
    return c


def grade(b):
    return bin(b).count("1")


@functools.lru_cache(maxsize=None)
def row_blades(n, grades):
    """bitmask of every component of a graded row holding `grades` (a tuple)"""
    out = []
    for k in sorted(grades):
        out.extend(m for m in range(1 << n) if grade(m) == k)
    return tuple(out)


def is_even(grades):
    return all(k % 2 == 0 for k in grades)


def blade_set(n, grades):
    """S: the blades the inverse of an operand holding `grades` lives in, ascending bitmask"""
    if is_even(grades):
        return tuple(m for m in range(1 << n) if grade(m) % 2 == 0)
    return tuple(range(1 << n))


def result_grades(n, grades):
    return tuple(k for k in range(n + 1) if k % 2 == 0) if is_even(grades) else tuple(range(n + 1))


@functools.lru_cache(maxsize=None)
def _structure(metric, grades):
    """(S, coefficient matrix C[c][b], source index src[c][b] into the operand row or -1): L_A = C * A[src]"""
    n = len(metric)
    S = blade_set(n, grades)
    where = {b: i for i, b in enumerate(row_blades(n, tuple(grades)))}
    N = len(S)
    C = np.zeros((N, N))
    src = np.full((N, N), -1, dtype=np.int64)
    for ci, c in enumerate(S):
        for bi, b in enumerate(S):
            a = c ^ b
            if a in where:
                C[ci, bi] = coeff(a, b, metric)
                src[ci, bi] = where[a]
    return S, C, src


def left_matrices(metric, grades, rows, dtype=np.float64):
    S, C, src = _structure(tuple(float(g) for g in metric), tuple(sorted(grades)))
    rows = np.asarray(rows, dtype=dtype)
    a = np.concatenate([rows, np.zeros((rows.shape[0], 1), dtype=dtype)], axis=1)
    return (C.astype(dtype)[None] * a[:, src]).astype(dtype)


def scalar_rhs(N, dtype=np.float64):
    e = np.zeros(N, dtype=dtype)
    e[0] = 1   # the scalar blade 0 is the first of S
    return e


def s_to_row(n, grades, out_grades):
    """for every component of a graded row holding out_grades: its index in S"""
    S = blade_set(n, grades)
    pos = {b: i for i, b in enumerate(S)}
    return np.array([pos[b] for b in row_blades(n, tuple(sorted(out_grades)))], dtype=np.int64)


def inverse_rows(metric, grades, rows, out_grades=None, dtype=np.float64):
    """numpy.linalg.solve per item, in `dtype`; returns rows holding out_grades (default: every grade of the result)"""
    n = len(metric)
    out_grades = result_grades(n, grades) if out_grades is None else out_grades
    L = left_matrices(metric, grades, rows, dtype)
    e = np.broadcast_to(scalar_rhs(L.shape[1], dtype)[None, :, None], (L.shape[0], L.shape[1], 1))
    y = np.linalg.solve(L, e)[..., 0].astype(dtype)
    return y[:, s_to_row(n, tuple(sorted(grades)), out_grades)]


def full_y(n, grades, out_rows, out_grades=None):
    """rows holding out_grades (default every grade of the result) -> vectors over S, float64 (grades not held: 0)"""
    out_grades = result_grades(n, grades) if out_grades is None else out_grades
    idx = s_to_row(n, tuple(sorted(grades)), out_grades)
    out_rows = np.asarray(out_rows, dtype=np.float64)
    y = np.zeros((out_rows.shape[0], len(blade_set(n, grades))))
    y[:, idx] = out_rows
    return y


def backward_error(metric, grades, rows, y):
    """per item ||L_A y - e||_inf / (||L_A||_inf ||y||_inf), all in float64; y over S; ||L_A||_inf the largest absolute row sum"""
    L = left_matrices(metric, grades, np.asarray(rows, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    r = np.einsum("icb,ib->ic", L, y) - scalar_rhs(L.shape[1])[None]
    return np.abs(r).max(axis=1) / (np.abs(L).sum(axis=2).max(axis=1) * np.abs(y).max(axis=1))


def norms(metric, grades, rows):
    """per item (||L_A||_inf, 2-norm condition number of L_A)"""
    L = left_matrices(metric, grades, np.asarray(rows, dtype=np.float64))
    return np.abs(L).sum(axis=2).max(axis=1), np.linalg.cond(L)


def gp_rows(metric, lgrades, lrows, rgrades, rrows, out_grades, absolute=False):
    """geometric product of graded rows, float64, term by term; absolute: the sum of |term| instead (for error bounds)"""
    n = len(metric)
    lb, rb = row_blades(n, tuple(sorted(lgrades))), row_blades(n, tuple(sorted(rgrades)))
    ob = {b: i for i, b in enumerate(row_blades(n, tuple(sorted(out_grades))))}
    lrows, rrows = np.asarray(lrows, dtype=np.float64), np.asarray(rrows, dtype=np.float64)
    out = np.zeros((max(lrows.shape[0], rrows.shape[0]), len(ob)))
    for i, a in enumerate(lb):
        for j, b in enumerate(rb):
            if (a ^ b) in ob:
                c = coeff(a, b, metric)
                if c != 0.0:
                    t = c * lrows[:, i] * rrows[:, j]
                    out[:, ob[a ^ b]] += np.abs(t) if absolute else t
    return out


# ---- reverse mode ---------------------------------------------------------------------------------------------------------------
def jvp_central(f, x, v, h=1e-6):
    """J v of f at x by central differences (float64)"""
    return (f(x + h * v) - f(x - h * v)) / (2.0 * h)


def adjoint_identity(f, x, v, g, vjp_rows, h=1e-6):
    """per item (<g, J v>, <J^T g, v>, sum |g_i (J v)_i|): the two sides of the adjoint identity and the scale their difference is
    judged against; J v by central differences of f, vjp_rows = J^T g from the code under test"""
    jv = jvp_central(f, x, v, h)
    return (np.einsum("ij,ij->i", g, jv), np.einsum("ij,ij->i", np.asarray(vjp_rows, dtype=np.float64), v),
            np.einsum("ij,ij->i", np.abs(g), np.abs(jv)))
