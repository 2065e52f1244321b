"""Independent numpy restatement of the tangents of the general square root and logarithm (GAAST_OP_GSQRT_JVP / GAAST_OP_GLOG_JVP,
include/gaast_hip.h) on top of gsqrt_numpy / glog_numpy, and of the composed second-order rule of gsqrt (gaast_expr.h).

    sqrt_jvp(A, h)   X = gsqrt_numpy.forward(A);  the u with (L_X + R_X) u = h  (gsqrt_numpy.solve: the elimination of the kernels,
                     pivot test |p| > N eps max_i |X_i|)
    log_jvp(A, h)    the forward of glog_numpy keeping X_1 ... X_s;  t = h;  for i = 1 ... s: (L_(X_i) + R_(X_i)) t' = t;
                     for j = 1 ... 7: L_(M_j) p = t, R_(M_j) q = p, acc += alpha_j q, M_j = e_0 + beta_j E;  the result 2^s acc
    sqrt_adj2(A, g, h)   the gradient in A of <g, sqrt_jvp(A, h)>:  -reverse(ADJL(w, u) + ADJR(w, u), A), w = reverse(A, g), u = sqrt_jvp(A, h)

in a chosen dtype, every sum over j ascending, one rounding per operation.  The references run the same solves in numpy.longdouble on
the reference forward of the two files (roots run to their own floor; theta = 1/16 and 12 nodes for the logarithm).  Nothing is
shared with gaast_amd/csrc."""
import numpy as np

import gexp_numpy as gx
import glog_numpy as gl
import gsqrt_numpy as gs

EPS = gs.EPS
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)


def sum_matrix(Cd, X):
    """L_X + R_X: (X u + u X)[r] = sum_j (L_X + R_X)[r][j] u[j]"""
    return gs.left_matrix(Cd, X) + gl.right_matrix(Cd, X)


def _structure(metric, grades, dt):
    metric, grades = gx._key(metric, grades)
    return metric, grades, gx.structure(metric, grades)[1].astype(dt)


def sqrt_jvp(metric, grades, A, h, dtype=np.float64, max_steps=gs.MAX_STEPS):
    """the tangent of gsqrt at A in direction h, both over S, in `dtype`; NaN rows for domain errors of the root and failed pivots"""
    dt = np.dtype(dtype)
    metric, grades, Cd = _structure(metric, grades, dt)
    X = gs.forward(metric, grades, A, dt, max_steps=max_steps)[0]
    N = X.shape[1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u, sing = gs.solve(sum_matrix(Cd, X), np.asarray(h).astype(dt), dt.type(N) * dt.type(EPS[dt]) * np.abs(X).max(axis=1))
    u[sing | ~np.isfinite(X).all(axis=1)] = np.nan
    return u


def sqrt_jvp_reference(metric, grades, A, h):
    return sqrt_jvp(metric, grades, np.asarray(A, dtype=np.longdouble), h, np.longdouble, max_steps=40)


def log_jvp(metric, grades, A, h, dtype=np.float64, drop_scale=False, both_left=False, **kw):
    """the tangent of glog at A in direction h, both over S, in `dtype`.  drop_scale / both_left: the two mutations the host tests
    must catch (the 2^s left out; L's sign word in both Pade passes, M_j^-2 t in the place of M_j^-1 t M_j^-1.  Exchanging the two
    words is no mutation: left and right multiplications commute, so R^-1 L^-1 = L^-1 R^-1)"""
    dt = np.dtype(dtype)
    _, s, bad, state = gl.forward(metric, grades, A, dt, keep=True, **kw)
    Cd, E, chain, beta, alpha, e0, eps = state
    n_eps = dt.type(E.shape[1]) * eps
    bad = bad.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = np.asarray(h).astype(dt)
        for i in range(1, len(chain) + 1):
            Xi = chain[i - 1]
            sol, sing = gs.solve(sum_matrix(Cd, Xi), t, n_eps * np.abs(Xi).max(axis=1))
            mine = i <= s
            t = np.where(mine[:, None], sol, t)
            bad |= mine & sing
        acc = np.zeros_like(t)
        first, second = gs.left_matrix, (gs.left_matrix if both_left else gl.right_matrix)
        for j in range(len(beta)):
            M = e0 + beta[j] * E
            tol = n_eps * np.abs(M).max(axis=1)
            p, sing1 = gs.solve(first(Cd, M), t, tol)
            q, sing2 = gs.solve(second(Cd, M), p, tol)
            bad |= sing1 | sing2
            acc = acc + alpha[j] * q
        out = acc if drop_scale else np.ldexp(acc, s[:, None].astype(np.int32))
    out[bad] = np.nan
    return out


def log_jvp_reference(metric, grades, A, h):
    return log_jvp(metric, grades, np.asarray(A, dtype=np.longdouble), h, np.longdouble, **gl._ref_kw())


def sqrt_adj2(metric, grades, A, g, h, dtype=np.longdouble):
    """the gradient in A (over S) of <g, sqrt_jvp(A, h)> = <gsqrt_numpy.reverse(A, g), h>: the composed rule of gaast_expr.h"""
    dt = np.dtype(dtype)
    metric, grades, Cd = _structure(metric, grades, dt)
    A = np.asarray(A).astype(dt)
    X = gs.forward(metric, grades, A, dt, max_steps=40)[0]
    w = gs.reverse(metric, grades, A, g, dt, X=X)
    u, _ = gs.solve(sum_matrix(Cd, X), np.asarray(h).astype(dt), np.zeros(len(A), dtype=dt))
    return -gs.reverse(metric, grades, A, gx._adjl(Cd, w, u) + gx._adjr(Cd, w, u), dt, X=X)


# ---- error units --------------------------------------------------------------------------------------------------------------------
def sum_condition(metric, grades, X):
    """kappa_inf(L_X + R_X) per item (float64)"""
    metric, grades = gx._key(metric, grades)
    T = sum_matrix(gx.structure(metric, grades)[1], np.asarray(X, dtype=np.float64))
    return np.abs(T).sum(axis=2).max(axis=1) * np.abs(np.linalg.inv(T)).sum(axis=2).max(axis=1)


def sqrt_jvp_error(got, want, eps, kappa):
    """per item ||got - want||_inf in units of N eps kappa_inf(L_X + R_X) ||want||_inf (gsqrt_numpy.gradient_error's unit)"""
    return gs.gradient_error(got, want, eps, kappa)


def log_jvp_error(got, want, eps, ref, j_norm, h):
    """per item ||got - want||_inf in units of N eps max(1, sum_i |(log A)_i|) ||J||_inf ||h||_inf (ref = log A;
    j_norm = glog_numpy.jacobian_norm(..., of_j=True))"""
    return gl.gradient_error(got, want, eps, ref, j_norm, h)


# The worst error of the restatement in the program's dtype against the longdouble reference over case_operands (below) of every case
# -- glog_numpy.operands(metric, grades, 2, rng): 0 ... 5 roots, over R^1, R^3 even, PGA3D even, PGA3D, CGA, R^7 even; R^1 with the 257
# items of the GPU test --, rounded up; tests/test_root_log_jvp_host.py measures it on every run.  The GPU's bound is 4 x this: the same
# recurrences, other roundings.  N = 2 has scales of its own: its unit is two ulps and among 257 items single ones cancel badly
# (twelve items of the same kinds give 0.49 / 0.56 and 0.96 / 1.11), which would loosen the others (as gexp2_numpy does it).
SQRT_JVP_SCALE = {"N2": {_F32: 1.35, _F64: 1.4}, "N>=4": {_F32: 0.45, _F64: 0.55}}   # measured 1.305 / 1.361 (R^1); 0.416 (PGA3D even) / 0.503 (R^3 even)
LOG_JVP_SCALE = {"N2": {_F32: 4.9, _F64: 4.8}, "N>=4": {_F32: 0.65, _F64: 0.75}}     # measured 4.806 / 4.702 (R^1); 0.612 / 0.726 (R^3 even)


def scale_of(table, N, dtype):
    return table["N2" if N == 2 else "N>=4"][np.dtype(dtype)]


# name -> (metric, operand grades, N): the sweep of the scales and of the GPU tests
CASES = {"R1": ([1.0], [0, 1], 2), "R3-even": ([1.0] * 3, [0, 2], 4), "PGA3D-even": ([0.0, 1.0, 1.0, 1.0], [0, 2, 4], 8),
         "PGA3D": ([0.0, 1.0, 1.0, 1.0], [0, 1, 2, 3, 4], 16), "CGA": ([1.0, 1.0, 1.0, 1.0, -1.0], [0, 1, 2, 3, 4, 5], 32),
         "R7-even": ([1.0] * 7, [0, 2, 4, 6], 64)}
NINE_OF_TWELVE = np.array([0, 2, 4, 6, 8, 10, 9, 11, 1])   # N = 64: nine items of the twelve, every kind of operand among them


def sweep_operands(name, rng, dtype=np.float32):
    """(A, h, g): glog_numpy.operands(..., 2, rng) -- twelve items, s = 0 ... 5 roots in one batch (nine at N = 64) -- with a tangent and a
    cotangent U(-1, 1) on every blade of S, float64 values representable in `dtype`"""
    metric, grades, N = CASES[name]
    A, _ = gl.operands(metric, grades, 2, rng, dtype)
    if N == 64:
        A = A[NINE_OF_TWELVE]
    h = rng.uniform(-1, 1, A.shape).astype(dtype).astype(np.float64)
    g = rng.uniform(-1, 1, A.shape).astype(dtype).astype(np.float64)
    return A, h, g


def case_operands(name):
    """(A, h, g) of a case, the one draw that both the CPU scales and the GPU tests use (default_rng([20261021, N])): sweep_operands,
    except at N = 2, where 43 items per kind are drawn and the first 257 kept -- more than one workgroup of 128 items with a tail, and a
    population in which single items cancel badly, so the scale of N = 2 is measured on the very items the GPU is held to"""
    metric, grades, N = CASES[name]
    rng = np.random.default_rng([20261021, N])
    if N != 2:
        return sweep_operands(name, rng)
    A = gl.operands(metric, grades, 43, rng)[0][:257]
    h = rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
    g = rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
    return A, h, g
