"""Independent numpy restatement of the general multivector square root and its reverse mode (GAAST_OP_GSQRT / GAAST_OP_GSQRT_ADJ,
include/gaast_hip.h), on blade bitmasks, plus references of the principal root in numpy.longdouble and in mpmath.

gsqrt(A) is the principal X with X X = A.  With S the blade set of inverse_numpy / gexp_numpy (the index of S[r] xor S[j] is
r xor j) and L_A[r][j] = coeff(r, j) A[r xor j], `forward` restates the product form of the Denman-Beavers iteration in a chosen dtype
(float32, float64, longdouble), every sum over j ascending, one rounding per operation (no fused multiply-add):

    M = A;  Y = A;  last = False
    for k = 0, 1, ... K (K = 16):
        d = sum_r |(M - e_0)_r|            (butterfly: v <- v + v[j xor m], m = N/2 ... 1)
        d not finite            -> a domain error
        d <= N eps  or  last    -> stop: the root is Y, after k steps
        k == K                  -> a domain error (not stopped)
        last = d <= sqrt(eps)              (quadratic convergence: one further step reaches the rounding floor, where d may stagnate)
        W = the solution of L_M W = e_0    (Gauss-Jordan, partial pivoting, ties to the lowest row; a pivot that fails
                                            |p| > N eps max_i |M_i| is a domain error)
        Y = 1/2 (Y (e_0 + W));   M = 1/2 (e_0 + 1/2 (M + W))

`reverse` solves the transposed system of L_X + R_X, ADJL(a, X) + ADJR(a, X) = g in gexp_numpy's operators, with numpy.linalg.solve
(the elimination of this file in longdouble, which LAPACK lacks).  Nothing is shared with gaast_amd/csrc."""
import numpy as np

import gexp_numpy as gx
import inverse_numpy as inu

EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52, np.dtype(np.longdouble): float(np.finfo(np.longdouble).eps)}
MAX_STEPS = 16


def distance(M):
    """sum_r |(M - e_0)_r| per item: the butterfly sum, in M's dtype"""
    v = M.copy()
    v[:, 0] = v[:, 0] - M.dtype.type(1)
    v = np.abs(v)
    N = M.shape[1]
    idx = np.arange(N)
    m = N // 2
    while m >= 1:
        v = v + v[:, idx ^ m]
        m //= 2
    return v[:, 0]


def solve(L, b, tol):
    """Gauss-Jordan with partial pivoting per item, in L's dtype (ties: the lowest row; a NaN is the largest).  L [B, N, N], b [B, N],
    tol [B].  Returns (y, singular): singular where some pivot fails |p| > tol"""
    L, b = L.copy(), b.copy()
    B, N, _ = L.shape
    used = np.zeros((B, N), dtype=bool)
    col_of = np.zeros((B, N), dtype=np.int64)
    piv_of = np.ones((B, N), dtype=L.dtype)
    bad = np.zeros(B, dtype=bool)
    it = np.arange(B)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(N):
            mag = np.abs(L[:, :, k])
            mag = np.where(np.isnan(mag), np.inf, mag)
            mag = np.where(used, -1.0, mag)
            who = mag.argmax(axis=1)                      # (argmax: the first of equals)
            piv = L[it, who, k]
            bad |= ~(np.abs(piv) > tol)
            used[it, who] = True
            col_of[it, who] = k
            piv_of[it, who] = piv
            f = L[:, :, k] / piv[:, None]
            f[it, who] = 0
            prow, pb = L[it, who, :].copy(), b[it, who].copy()
            L = L - f[:, :, None] * prow[:, None, :]
            b = b - f * pb[:, None]
        y = np.zeros_like(b)
        y[it[:, None], col_of] = b / piv_of
    return y, bad


def left_matrix(Cd, X):
    """L_X[r][j] = C[r][j] X[r xor j]"""
    idx = np.arange(X.shape[1])
    return Cd[None] * X[:, idx[:, None] ^ idx[None, :]]


def forward(metric, grades, A, dtype=np.float64, max_steps=MAX_STEPS):
    """A: vectors over S.  Returns (X, steps, bad) computed in `dtype`: the root, the number of steps each item took, and the domain
    errors, whose every component is NaN"""
    metric, grades = gx._key(metric, grades)
    _, C, _ = gx.structure(metric, grades)
    dt = np.dtype(dtype)
    eps = dt.type(EPS[dt])
    Cd = C.astype(dt)
    A = np.asarray(A).astype(dt)
    B, N = A.shape
    e0 = np.zeros((1, N), dtype=dt)
    e0[0, 0] = 1
    half = dt.type(0.5)
    M, Y = A.copy(), A.copy()
    done = np.zeros(B, dtype=bool)
    bad = np.zeros(B, dtype=bool)
    last = np.zeros(B, dtype=bool)
    steps = np.zeros(B, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(max_steps + 1):
            d = distance(M)
            fin = np.isfinite(d)
            bad |= ~done & ~fin
            done |= ~fin
            done |= (d <= dt.type(N) * eps) | last
            if k == max_steps or done.all():
                break
            last = d <= np.sqrt(eps)
            W, sing = solve(left_matrix(Cd, M), np.broadcast_to(e0, M.shape).copy(), dt.type(N) * eps * np.abs(M).max(axis=1))
            bad |= ~done & sing
            done |= sing
            Yn = half * gx._gp(Cd, Y, e0 + W)
            Mn = half * (e0 + half * (M + W))
            go = ~done
            Y = np.where(go[:, None], Yn, Y)
            M = np.where(go[:, None], Mn, M)
            steps += go
    bad |= ~done
    X = Y.copy()
    X[bad] = np.nan
    return X, steps, bad


def transposed_sum_matrix(Cd, X):
    """T with T a = ADJL(a, X) + ADJR(a, X): T[c][c xor t] = (C[c xor t][t] + C[c xor t][c]) X[t], the transpose of L_X + R_X"""
    N = X.shape[1]
    idx = np.arange(N)
    c, j = idx[:, None], idx[None, :]
    t = c ^ j
    return (Cd[j, t] + Cd[j, c])[None] * X[:, t]


def reverse(metric, grades, A, g, dtype=np.float64, X=None):
    """cotangent of A over S for the cotangent g of gsqrt(A) over S, in `dtype` (the root recomputed in `dtype` unless X is given)"""
    metric, grades = gx._key(metric, grades)
    _, C, _ = gx.structure(metric, grades)
    dt = np.dtype(dtype)
    if X is None:
        X = forward(metric, grades, A, dt)[0]
    X = np.asarray(X).astype(dt)
    T = transposed_sum_matrix(C.astype(dt), X)
    gb = np.asarray(g).astype(dt)
    out = np.full_like(gb, np.nan)
    ok = np.isfinite(X).all(axis=1)
    if ok.any():
        if dt == np.dtype(np.longdouble):
            out[ok] = solve(T[ok], gb[ok], np.zeros(int(ok.sum()), dtype=dt))[0]
        else:
            out[ok] = np.linalg.solve(T[ok], gb[ok][..., None])[..., 0].astype(dt)
    return out


# ---- references -----------------------------------------------------------------------------------------------------------------
def root_reference(metric, grades, A):
    """the principal root in numpy.longdouble: the same iteration run to its own floor.  (X float64-rounded is NOT returned: the
    longdouble values are, so that errors of float64 results are measured against something finer)"""
    X, steps, bad = forward(metric, grades, np.asarray(A, dtype=np.longdouble), np.longdouble, max_steps=40)
    assert not bad.any()
    return X


def sqrtm_reference(metric, grades, A, dps=50):
    """the principal root per item from mpmath.sqrtm of L_A at `dps` digits (its first column), rounded to float64"""
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
            R = mp.sqrtm(L)
            out[it] = [float(mp.re(R[r, 0])) for r in range(N)]
    return out


def _ld(x):
    return np.asarray(x).astype(np.longdouble)


def residual(metric, grades, X, A, eps):
    """per item ||X X - A||_inf / (||L_X||_inf ||X||_inf) in units of N eps, evaluated in longdouble"""
    metric, grades = gx._key(metric, grades)
    Cd = gx.structure(metric, grades)[1].astype(np.longdouble)
    X, A = _ld(X), _ld(A)
    N = X.shape[1]
    r = np.abs(gx._gp(Cd, X, X) - A).max(axis=1)
    lnorm = np.abs(left_matrix(Cd, X)).sum(axis=2).max(axis=1)
    return (r / (lnorm * np.abs(X).max(axis=1)) / (N * eps)).astype(np.float64)


def forward_error(X, ref, eps):
    """per item ||X - ref||_inf / ||ref||_inf in units of N eps"""
    X, ref = _ld(X), _ld(ref)
    return (np.abs(X - ref).max(axis=1) / np.abs(ref).max(axis=1) / (X.shape[1] * eps)).astype(np.float64)


def sum_condition(metric, grades, X):
    """kappa_inf of the transposed L_X + R_X per item (float64)"""
    metric, grades = gx._key(metric, grades)
    T = transposed_sum_matrix(gx.structure(metric, grades)[1], np.asarray(X, dtype=np.float64))
    return np.abs(T).sum(axis=2).max(axis=1) * np.abs(np.linalg.inv(T)).sum(axis=2).max(axis=1)


def gradient_error(got, want, eps, kappa):
    """per item ||got - want||_inf in units of N eps kappa_inf(L_X + R_X) ||want||_inf"""
    got, want = _ld(got), _ld(want)
    return (np.abs(got - want).max(axis=1) / (got.shape[1] * eps * kappa * np.abs(want).max(axis=1))).astype(np.float64)


# The worst `residual` / `forward_error` (FWD_SCALE) and `gradient_error` (GRAD_SCALE) of the restatement in the program's dtype over
# the inputs of tests/test_gsqrt_host.py, rounded up (measured there on every run; the GPU's bound is 4 x this: the same recurrences,
# its sums contracted into fused multiply-adds and its pivot ties broken alike but on other roundings)
FWD_SCALE = {np.dtype(np.float32): 2.3, np.dtype(np.float64): 2.3}     # measured 2.123 / 2.237 (the residual in R^1)
GRAD_SCALE = {np.dtype(np.float32): 0.55, np.dtype(np.float64): 0.8}   # measured 0.519 / 0.779 (R^1)

THETAS = (0.1, 1.0, 2.5)


def operands(metric, grades, batch, rng, dtype=np.float32):
    """vectors over S with a principal root by construction, float64 values representable in `dtype`: for each theta of THETAS `batch`
    items gexp(B), B = U(-1, 1) on `grades` normalised to sum |B| = theta (theta < pi: gexp(B / 2) is the principal root), then
    `batch` items with a dominant positive scalar, 1 + U(-1, 1) * 0.4 / N on every blade of S.  Returns (A, theta per item; 0 for the
    last kind)"""
    metric, grades = gx._key(metric, grades)
    S = gx.structure(metric, grades)[0]
    out, th = [], []
    for theta in THETAS:
        Bv = gx.random_operand(metric, grades, batch, theta, rng, np.float64)
        out.append(gx.forward(metric, grades, Bv, np.float64)[0])
        th += [theta] * batch
    dom = rng.uniform(-1.0, 1.0, (batch, len(S))) * 0.4 / len(S)
    dom[:, 0] += 1.0
    out.append(dom)
    th += [0.0] * batch
    return np.concatenate(out).astype(dtype).astype(np.float64), np.array(th)
