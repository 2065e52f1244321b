"""Independent numpy restatement of the second-order adjoint of the general logarithm (GAAST_OP_GLOG_ADJ2, include/gaast_hip.h) on top
of glog_numpy / gsqrt_numpy / gexp_numpy.

    log_adj2(A, g, h)   the gradient in A of <g, log_jvp(A, h)> = <glog_numpy.reverse(A, g), h>, the roots X_1 ... X_s and s of A held
                        fixed.  With S_i = L_(X_i) + R_(X_i), E = X_s - e_0, M_j = e_0 + beta_j E:
        t_0 = h;  S_i t_i = t_(i-1), i = 1 ... s (every t_i kept);   g' = 2^s g;
        for j = 1 ... 7:  R_(M_j)^T v1 = g';  L_(M_j)^T u = v1;  L_(M_j)^T v2 = g';  L_(M_j) p = t_s;  R_(M_j) q = p;
                          a += alpha_j u;   gamma -= alpha_j beta_j (ADJR(v1, q) + ADJL(v2, q));
        w = a, e = gamma;  for i = s ... 1:  w <- S_i^-T w;  e <- S_i^-T (e - (ADJR(w, t_i) + ADJL(w, t_i)));   the result e

in a chosen dtype, every solve gsqrt_numpy.solve with the kernels' pivot tests, every sum over j ascending, one rounding per
operation.  The reference runs the same recurrences in numpy.longdouble on the reference forward of glog_numpy (theta = 1/16, 12 nodes,
roots run to their own floor).  Nothing is shared with gaast_amd/csrc."""
import numpy as np

import gexp_numpy as gx
import glog_numpy as gl
import gsqrt_numpy as gs
import root_log_jvp_numpy as rl

EPS = gs.EPS
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)


def _recurrences(state, s, g, h, solve, drop_gamma=False, drop_chain_term=False, drop_scale=False):
    """the recurrences of the module's head on state = glog_numpy.forward(..., keep=True)[3]; solve(T, b, amax) -> (x, singular) solves
    T x = b, amax = max_i |M_i| of the multivector whose matrix T is.  Returns (e, singular).  drop_*: the three mutations the host
    tests must catch"""
    Cd, E, chain, beta, alpha, e0, _ = state
    dt = E.dtype
    bad = np.zeros(E.shape[0], dtype=bool)
    tr = lambda T: np.ascontiguousarray(T.transpose(0, 2, 1))
    t = np.asarray(h).astype(dt)
    ts = []
    for i in range(1, len(chain) + 1):
        Xi = chain[i - 1]
        sol, sing = solve(rl.sum_matrix(Cd, Xi), t, np.abs(Xi).max(axis=1))
        mine = i <= s
        t = np.where(mine[:, None], sol, t)
        bad |= mine & sing
        ts.append(t)
    gp = np.asarray(g).astype(dt) if drop_scale else np.ldexp(np.asarray(g).astype(dt), s[:, None].astype(np.int32))
    a = np.zeros_like(gp)
    gamma = np.zeros_like(gp)
    for j in range(len(beta)):
        M = e0 + beta[j] * E
        amax = np.abs(M).max(axis=1)
        LM, RM = gs.left_matrix(Cd, M), gl.right_matrix(Cd, M)
        v1, s1 = solve(tr(RM), gp, amax)
        u, s2 = solve(tr(LM), v1, amax)
        v2, s3 = solve(tr(LM), gp, amax)
        p, s4 = solve(LM, t, amax)
        q, s5 = solve(RM, p, amax)
        bad |= s1 | s2 | s3 | s4 | s5
        a = a + alpha[j] * u
        if not drop_gamma:
            gamma = gamma - (alpha[j] * beta[j]) * (gx._adjr(Cd, v1, q) + gx._adjl(Cd, v2, q))
    w, e = a, gamma
    for i in range(len(chain), 0, -1):
        Xi = chain[i - 1]
        T = gs.transposed_sum_matrix(Cd, Xi)
        amax = np.abs(Xi).max(axis=1)
        mine = i <= s
        wn, sing1 = solve(T, w, amax)
        w = np.where(mine[:, None], wn, w)
        rhs = e if drop_chain_term else e - (gx._adjr(Cd, w, ts[i - 1]) + gx._adjl(Cd, w, ts[i - 1]))
        en, sing2 = solve(T, rhs, amax)
        e = np.where(mine[:, None], en, e)
        bad |= mine & (sing1 | sing2)
    return e, bad


def log_adj2(metric, grades, A, g, h, dtype=np.float64, drop_gamma=False, drop_chain_term=False, drop_scale=False, **kw):
    """GLOG_ADJ2(g, h, A) over S in `dtype` (the forward recomputed in `dtype`); NaN rows for domain errors and failed pivots"""
    dt = np.dtype(dtype)
    _, s, bad, state = gl.forward(metric, grades, A, dt, keep=True, **kw)
    n_eps = dt.type(state[1].shape[1]) * state[6]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e, sing = _recurrences(state, s, g, h, lambda T, b, amax: gs.solve(T, b, n_eps * amax), drop_gamma, drop_chain_term, drop_scale)
    e[bad | sing] = np.nan
    return e


def log_adj2_reference(metric, grades, A, g, h, **mut):
    return log_adj2(metric, grades, np.asarray(A, dtype=np.longdouble), g, h, np.longdouble, **mut, **gl._ref_kw())


# ---- error unit ---------------------------------------------------------------------------------------------------------------------
def hessian_norm(metric, grades, A, g):
    """||G||_inf per item, G the item's N x N matrix with log_adj2(A, g, h) = G h: the recurrences on the N unit tangents, in float64
    (the forward of the restatement, every system solved by numpy.linalg.solve), the analogue of glog_numpy.jacobian_norm and computed
    as that one is.  It is a factor of the error unit, not a reference value: float64 and LAPACK's solves give it to some 1e-13
    relative where the longdouble reference on the N unit tangents would give it to 1e-18, at N times the cost of every test that
    needs it; a bound that moves by 1e-13 of itself decides no test."""
    A = np.asarray(A, dtype=np.float64)
    B, N = A.shape
    _, s, bad, state = gl.forward(metric, grades, A, np.float64, keep=True)
    assert not bad.any()
    solve = lambda T, b, amax: (np.linalg.solve(T, b[..., None])[..., 0], np.zeros(B, dtype=bool))
    G = np.zeros((B, N, N))
    for k in range(N):
        G[:, :, k] = _recurrences(state, s, g, np.tile(np.eye(N)[k], (B, 1)), solve)[0]
    return np.abs(G).sum(axis=2).max(axis=1)


def log_adj2_error(got, want, eps, ref, g_norm, h):
    """per item ||got - want||_inf in units of N eps max(1, sum_i |(log A)_i|) ||G||_inf ||h||_inf (ref = log A; g_norm = hessian_norm)"""
    return gl.gradient_error(got, want, eps, ref, g_norm, h)


# The worst error of the restatement in the program's dtype against the longdouble reference over root_log_jvp_numpy.case_operands of all
# six cases (none of those items is a domain error), rounded up; tests/test_glog_adj2_host.py measures it on every run.  The GPU's bound
# is 4 x this: the same recurrences, other roundings.  N = 2 has scales of its own, as in root_log_jvp_numpy: among its 257 items single
# ones cancel badly in one component.
LOG_ADJ2_SCALE = {"N2": {_F32: 8.8, _F64: 98.0}, "N>=4": {_F32: 0.75, _F64: 0.75}}   # measured 8.576 / 96.82 (R^1); 0.735 / 0.711 (R^3 even)

scale_of = rl.scale_of
CASES = rl.CASES
case_operands = rl.case_operands
sweep_operands = rl.sweep_operands
