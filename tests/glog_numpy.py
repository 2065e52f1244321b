"""Independent numpy restatement of the general multivector logarithm and its reverse mode (GAAST_OP_GLOG / GAAST_OP_GLOG_ADJ,
include/gaast_hip.h), on blade bitmasks, plus references of the principal logarithm in numpy.longdouble and in mpmath.

glog(A) is the principal Y with gexp(Y) = A.  With S, L_A and the butterfly sums of gsqrt_numpy / gexp_numpy, `forward` restates
inverse scaling and squaring in a chosen dtype (float32, float64, longdouble), every sum over j ascending, one rounding per
operation (no fused multiply-add):

    X = A;  s = 0
    while wmax * sum_r |(X - e_0)_r| > 1/4:         (not finite -> a domain error)
        s == 16  -> a domain error
        X = gsqrt_numpy.forward(X)                  (its domain errors are domain errors);   s += 1
    E = X - e_0
    Y = sum_(j = 1 ... 7) alpha_j y_j,   L_(e_0 + beta_j E) y_j = E     (gsqrt_numpy.solve; a pivot that fails
                                                                        |p| > N eps max_i |(e_0 + beta_j E)_i| is a domain error)
    result 2^s Y

alpha_j, beta_j: numpy.polynomial.legendre.leggauss(7) mapped to [0, 1] (the [7/7] Pade approximant of log(1 + x) in partial
fractions).  `reverse` recomputes the forward keeping X_1 ... X_s and runs
    g' = 2^s g;   a = sum_j alpha_j u_j,  R_(M_j)^T v_j = g',  L_(M_j)^T u_j = v_j,  M_j = e_0 + beta_j E;
    for i = s ... 1:  a <- the solution of (L_(X_i) + R_(X_i))^T a' = a.
Nothing is shared with gaast_amd/csrc."""
import functools

import numpy as np

import gexp_numpy as gx
import gsqrt_numpy as gs

EPS = gs.EPS
THETA = 0.25
TERMS = 7
MAX_ROOTS = 16


def pade_table(terms=TERMS):
    """(beta, alpha): nodes and weights of `terms`-point Gauss-Legendre quadrature on [0, 1], float64, as numpy gives them"""
    x, w = np.polynomial.legendre.leggauss(terms)
    return (x + 1.0) / 2.0, w / 2.0


@functools.lru_cache(maxsize=None)
def pade_table_longdouble(terms):
    """the same in longdouble, from mpmath at 40 digits (Newton on the Legendre polynomial from numpy's nodes): numpy's own weights are
    only good to a few 1e-15, far above longdouble eps"""
    import mpmath as mp
    x0, _ = np.polynomial.legendre.leggauss(terms)
    beta, alpha = [], []
    with mp.workdps(40):
        for xv in x0:
            x = mp.mpf(float(xv))
            for _ in range(4):
                p, p1 = mp.legendre(terms, x), mp.legendre(terms - 1, x)
                dp = terms * (x * p - p1) / (x * x - 1)
                x = x - p / dp
            p, p1 = mp.legendre(terms, x), mp.legendre(terms - 1, x)
            dp = terms * (x * p - p1) / (x * x - 1)
            beta.append(np.longdouble(mp.nstr((x + 1) / 2, 30)))
            alpha.append(np.longdouble(mp.nstr(1 / ((1 - x * x) * dp * dp), 30)))
    return np.array(beta, dtype=np.longdouble), np.array(alpha, dtype=np.longdouble)


def right_matrix(Cd, M):
    """R_M[r][a] = C[r][a xor r] M[a xor r]: (X M)[r] = sum_a R_M[r][a] X[a]"""
    idx = np.arange(M.shape[1])
    j = idx[:, None] ^ idx[None, :]
    return Cd[idx[:, None], j][None] * M[:, j]


def forward(metric, grades, A, dtype=np.float64, keep=False, theta=THETA, table=None, max_roots=MAX_ROOTS, root_steps=gs.MAX_STEPS):
    """A: vectors over S.  Returns (Y, s, bad) -- or (Y, s, bad, state) with keep -- computed in `dtype`: the logarithm, the number of
    roots each item took, and the domain errors, whose every component is NaN"""
    metric, grades = gx._key(metric, grades)
    _, C, wmax = gx.structure(metric, grades)
    dt = np.dtype(dtype)
    eps = dt.type(EPS[dt])
    Cd = C.astype(dt)
    beta, alpha = pade_table() if table is None else table
    beta, alpha = np.asarray(beta).astype(dt), np.asarray(alpha).astype(dt)
    X = np.asarray(A).astype(dt).copy()
    B, N = X.shape
    e0 = np.zeros((1, N), dtype=dt)
    e0[0, 0] = 1
    s = np.zeros(B, dtype=np.int64)
    bad = np.zeros(B, dtype=bool)
    chain = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for it in range(max_roots + 1):
            d = gs.distance(X) * dt.type(wmax)
            bad |= ~np.isfinite(d)
            need = ~bad & (d > dt.type(theta))
            if it == max_roots:
                bad |= need
                break
            if not need.any():
                break
            Xr, _, rbad = gs.forward(metric, grades, X[need], dt, max_steps=root_steps)
            X[need] = Xr
            bad[need] |= rbad
            s += need
            chain.append(X.copy())
        E = X - e0
        acc = np.zeros_like(E)
        for j in range(len(beta)):
            M = e0 + beta[j] * E
            y, sing = gs.solve(gs.left_matrix(Cd, M), E, dt.type(N) * eps * np.abs(M).max(axis=1))
            bad |= sing
            acc = acc + alpha[j] * y
        Y = np.ldexp(acc, s[:, None].astype(np.int32))
    Y[bad] = np.nan
    if keep:
        return Y, s, bad, (Cd, E, chain, beta, alpha, e0, eps)
    return Y, s, bad


def _sweep(state, s, gp, solve):
    """the reverse sweep on the right-hand sides gp = 2^s g, [B, N] (or [B, N, K]: K cotangents per item at once);
    solve(T, b, amax) -> (x, singular) solves T x = b, amax = max_i |M_i| of the multivector whose matrix T is.  Returns (a, singular)"""
    Cd, E, chain, beta, alpha, e0, _ = state
    tail = (slice(None),) + (None,) * (gp.ndim - 1)
    bad = np.zeros(E.shape[0], dtype=bool)
    a = np.zeros_like(gp)
    for j in range(len(beta)):
        M = e0 + beta[j] * E
        amax = np.abs(M).max(axis=1)
        v, sing1 = solve(np.ascontiguousarray(right_matrix(Cd, M).transpose(0, 2, 1)), gp, amax)
        u, sing2 = solve(np.ascontiguousarray(gs.left_matrix(Cd, M).transpose(0, 2, 1)), v, amax)
        bad |= sing1 | sing2
        a = a + alpha[j] * u
    for i in range(len(chain), 0, -1):
        Xi = chain[i - 1]
        sol, sing = solve(gs.transposed_sum_matrix(Cd, Xi), a, np.abs(Xi).max(axis=1))
        mine = i <= s
        a = np.where(mine[tail], sol, a)
        bad |= mine & sing
    return a, bad


def reverse(metric, grades, A, g, dtype=np.float64, **kw):
    """cotangent of A over S for the cotangent g of glog(A) over S, in `dtype` (the forward recomputed in `dtype`)"""
    dt = np.dtype(dtype)
    _, s, bad, state = forward(metric, grades, A, dt, keep=True, **kw)
    n_eps = dt.type(state[1].shape[1]) * state[6]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gp = np.ldexp(np.asarray(g).astype(dt), s[:, None].astype(np.int32))
        a, sing = _sweep(state, s, gp, lambda T, b, amax: gs.solve(T, b, n_eps * amax))
    a[bad | sing] = np.nan
    return a


# ---- references -----------------------------------------------------------------------------------------------------------------
REF_THETA, REF_TERMS = 1.0 / 16, 12    # |r_12(-1/16) - log(15/16)| < 1e-30: the truncation lies below longdouble eps


def _ref_kw():
    return dict(theta=REF_THETA, table=pade_table_longdouble(REF_TERMS), max_roots=24, root_steps=40)


def log_reference(metric, grades, A):
    """the principal logarithm in numpy.longdouble: the same algorithm with theta = 1/16 and 12 nodes, its roots run to their own floor"""
    Y, _, bad = forward(metric, grades, np.asarray(A, dtype=np.longdouble), np.longdouble, **_ref_kw())
    assert not bad.any()
    return Y


def reverse_reference(metric, grades, A, g):
    """the cotangent in numpy.longdouble, through the reference's parameters"""
    return reverse(metric, grades, np.asarray(A, dtype=np.longdouble), g, np.longdouble, **_ref_kw())


def logm_reference(metric, grades, A, dps=40):
    """the principal logarithm per item from mpmath.logm of L_A at `dps` digits (its first column), rounded to float64.  Slow: about
    a quarter of a second per item at N = 16"""
    import mpmath as mp
    metric, grades = gx._key(metric, grades)
    _, C, _ = gx.structure(metric, grades)
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[1]
    out = np.zeros_like(A)
    with mp.workdps(dps):
        for it in range(A.shape[0]):
            L = mp.matrix(N, N)
            for r in range(N):
                for j in range(N):
                    if C[r, j] != 0.0:
                        L[r, j] = mp.mpf(float(C[r, j])) * mp.mpf(float(A[it, r ^ j]))
            R = mp.logm(L)
            out[it] = [float(mp.re(R[r, 0])) for r in range(N)]
    return out


def _ld(x):
    return np.asarray(x).astype(np.longdouble)


def forward_error(Y, ref, eps):
    """per item ||Y - ref||_inf in units of N eps max(1, sum_i |ref_i|)"""
    Y, ref = _ld(Y), _ld(ref)
    return (np.abs(Y - ref).max(axis=1) / (Y.shape[1] * eps * np.maximum(1.0, np.abs(ref).sum(axis=1)))).astype(np.float64)


def jacobian_norm(metric, grades, A, of_j=False):
    """||J^T||_inf per item (of_j: ||J||_inf, the largest absolute column sum of J^T), J the item's N x N Jacobian of glog: the sweep of `reverse` on the N unit cotangents at once, in float64
    (the forward of the restatement, the sweep's systems solved for N right-hand sides by numpy.linalg.solve)"""
    A = np.asarray(A, dtype=np.float64)
    B, N = A.shape
    _, s, bad, state = forward(metric, grades, A, np.float64, keep=True)
    assert not bad.any()
    gp = np.ldexp(np.tile(np.eye(N), (B, 1, 1)), s[:, None, None].astype(np.int32))      # column k: 2^s e_k
    jt, _ = _sweep(state, s, gp, lambda T, b, amax: (np.linalg.solve(T, b), np.zeros(B, dtype=bool)))   # column k: J^T e_k
    return np.abs(jt).sum(axis=1 if of_j else 2).max(axis=1)


def gradient_error(got, want, eps, ref, jt_norm, g):
    """per item ||got - want||_inf in units of N eps max(1, sum_i |ref_i|) ||J^T||_inf ||g||_inf (ref = log A)"""
    got, want = _ld(got), _ld(want)
    unit = got.shape[1] * eps * np.maximum(1.0, np.abs(_ld(ref)).sum(axis=1)) * jt_norm * np.abs(np.asarray(g, dtype=np.float64)).max(axis=1)
    return (np.abs(got - want).max(axis=1) / unit).astype(np.float64)


# The worst `forward_error` (FWD_SCALE) and `gradient_error` (GRAD_SCALE) of the restatement in the program's dtype over the inputs
# of tests/test_glog_host.py, rounded up (measured there on every run; the GPU's bound is 4 x this: the same recurrences, its sums
# contracted into fused multiply-adds and its pivot ties broken alike but on other roundings)
FWD_SCALE = {np.dtype(np.float32): 8.0, np.dtype(np.float64): 7.5}     # measured 7.96 / 7.19 (R^1)
GRAD_SCALE = {np.dtype(np.float32): 2.3, np.dtype(np.float64): 2.0}    # measured 2.204 / 1.950 (R^1)

KINDS = 6      # of `operands`: three thetas, the dominant scalar, the first kind times 37.5 and times 0.01


def operands(metric, grades, batch, rng, dtype=np.float32):
    """vectors over S with a principal logarithm by construction, float64 values representable in `dtype`: gsqrt_numpy.operands (for
    each theta of 0.1, 1.0, 2.5 `batch` items gexp(B) with sum |B| = theta, below pi, so B is the principal logarithm; then `batch` items
    with a dominant positive scalar), then the first `batch` of them scaled by 37.5 and by 0.01, which forces up to 5 roots.  Returns
    (A, kind per item: 0 ... 5)"""
    base, _ = gs.operands(metric, grades, batch, rng, dtype)
    A = np.concatenate([base, base[:batch] * 37.5, base[:batch] * 0.01]).astype(dtype).astype(np.float64)
    return A, np.repeat(np.arange(KINDS), batch)
