"""Independent numpy restatement of the general multivector exponential and its reverse sweep (GAAST_OP_GEXP / GAAST_OP_GEXP_ADJ,
include/gaast_hip.h), on blade bitmasks, plus an mpmath reference of exp(A).

For a multivector A of an algebra with diagonal metric `metric`, gexp(A) = sum_k A^k / k! under the geometric product.  With S the
even blades when A holds only even grades and every blade otherwise (ascending bitmask, as inverse_numpy.blade_set: the index of
S[r] xor S[j] is r xor j), y = exp(L_A) e_scalar for the left-multiplication matrix L_A[r][j] = coeff(r, j) A[r xor j].

`forward` / `reverse` restate the recurrences of the header in a chosen dtype (float32, float64, longdouble), every sum over j
ascending, one rounding per operation (no fused multiply-add):

    theta = wmax * sum |A_a|  (butterfly: v <- v + v[j xor m], m = N/2 ... 1);   s = least integer >= 0 with theta 2^-s <= 1/2
    q_m = e_0;  q_(k-1) = e_0 + (A_s q_k) / k,  k = m ... 1;    Y_0 = q_0;  Y_(i+1) = Y_i Y_i,  i < s
    reverse:  g <- ADJL(g, Y_i) + ADJR(g, Y_i), i = s-1 ... 0;   for k = 1 ... m: h = g / k; dA_s += ADJL(h, q_k); g <- ADJR(h, A_s)

Nothing is shared with gaast_amd/csrc; blade signs come from inverse_numpy.coeff (counting swaps).  `exp_reference` evaluates the
definition in mpmath at 50 digits: mpmath.expm of L_A (`method="expm"`), or the Taylor series of exp(L_A) e_0 summed on the vector
(`method="series"`, N^2 work per term where expm needs N^3: the only one affordable at N = 64); tests check that the two agree."""
import functools

import numpy as np

import inverse_numpy as inu

EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
DEGREE = {np.dtype(np.float32): 8, np.dtype(np.float64): 14, np.dtype(np.longdouble): 14}
MAX_SQUARINGS = 12


def taylor_degree(eps):
    """the least m with (1/2)^(m+1) / (m+1)! <= eps / 2"""
    m, t = 0, 0.5
    while t > eps / 2:
        m += 1
        t *= 0.5 / (m + 1)
    return m


@functools.lru_cache(maxsize=None)
def structure(metric, grades):
    """(S, C, wmax): the blade set, C[r][j] = coeff(S[r] xor S[j], S[j]) (float64) and the largest |metric factor| of the algebra"""
    n = len(metric)
    S = inu.blade_set(n, grades)
    N = len(S)
    pos = {b: i for i, b in enumerate(S)}
    C = np.zeros((N, N))
    for r in range(N):
        for j in range(N):
            assert pos[S[r] ^ S[j]] == r ^ j
            C[r, j] = inu.coeff(S[r] ^ S[j], S[j], metric)
    wmax = 0.0
    for sub in range(1 << n):
        w = 1.0
        for i in range(n):
            if (sub >> i) & 1:
                w *= metric[i]
        wmax = max(wmax, abs(w))
    return S, C, wmax


def _key(metric, grades):
    return tuple(float(g) for g in metric), tuple(sorted(grades))


def to_s(metric, grades, rows, row_grades=None, dtype=np.float64):
    """graded rows holding row_grades (default: `grades`) -> vectors over S (blades not held: 0)"""
    metric, grades = _key(metric, grades)
    S = structure(metric, grades)[0]
    pos = {b: i for i, b in enumerate(S)}
    rb = inu.row_blades(len(metric), tuple(sorted(grades if row_grades is None else row_grades)))
    rows = np.asarray(rows)
    out = np.zeros((rows.shape[0], len(S)), dtype=dtype)
    for i, b in enumerate(rb):
        if b in pos:
            out[:, pos[b]] = rows[:, i]
    return out


def from_s(metric, grades, y, out_grades=None):
    """vectors over S -> graded rows holding out_grades (default: every grade of the result)"""
    metric, grades = _key(metric, grades)
    n = len(metric)
    out_grades = inu.result_grades(n, grades) if out_grades is None else out_grades
    return np.asarray(y)[:, inu.s_to_row(n, grades, tuple(sorted(out_grades)))]


def theta_of(A, wmax):
    """the butterfly sum of |A| over the N components, times wmax, in A's dtype"""
    v = np.abs(A)
    N = A.shape[1]
    idx = np.arange(N)
    m = N // 2
    while m >= 1:
        v = v + v[:, idx ^ m]
        m //= 2
    return v[:, 0] * A.dtype.type(wmax)


def squarings_of(theta):
    """(s, bad) per item: the least integer s >= 0 with theta 2^-s <= 1/2; bad: theta not finite or s > 12"""
    theta = np.asarray(theta)
    with np.errstate(invalid="ignore"):
        bad = ~(theta <= 2048)
    s = np.zeros(theta.shape, dtype=np.int64)
    ok = ~bad & (theta > 0.5)
    f, e = np.frexp(np.where(ok, theta, 1.0))
    s[ok] = (e + (f != 0.5))[ok]
    return s, bad


def _gp(C, X, Z):
    """P[r] = sum_j (C[r][j] X[r xor j]) Z[j], j ascending, in the dtype of X"""
    N = X.shape[1]
    idx = np.arange(N)
    acc = np.zeros_like(X)
    for j in range(N):
        acc = acc + (C[None, :, j] * X[:, idx ^ j]) * Z[:, j:j + 1]
    return acc


def _adjl(C, G, Z):
    """ADJL(G, Z)[a] = sum_b (coeff(a, b) Z[b]) G[a xor b], coeff(a, b) = C[a xor b][b]"""
    N = G.shape[1]
    idx = np.arange(N)
    acc = np.zeros_like(G)
    for b in range(N):
        acc = acc + (C[idx ^ b, b][None] * Z[:, b:b + 1]) * G[:, idx ^ b]
    return acc


def _adjr(C, G, X):
    """ADJR(G, X)[b] = sum_a (coeff(a, b) X[a]) G[a xor b]"""
    N = G.shape[1]
    idx = np.arange(N)
    acc = np.zeros_like(G)
    for a in range(N):
        acc = acc + (C[a ^ idx, idx][None] * X[:, a:a + 1]) * G[:, a ^ idx]
    return acc


def forward(metric, grades, A, dtype=np.float64, s_dtype=None, keep=False, degree=None):
    """A: vectors over S.  Returns (Y, s, bad) -- or (Y, s, bad, state) with keep -- computed in `dtype`; theta and s are computed in
    s_dtype (default dtype), which also sets the Taylor degree: a longdouble evaluation of a float32 program keeps that program's s and m.  A domain-error item: s = 0
    and every component NaN.  degree: another Taylor degree (a longdouble evaluation
    with degree 20 is a reference of exp(A) itself, 1e-3 of a float64 ulp)"""
    metric, grades = _key(metric, grades)
    _, C, wmax = structure(metric, grades)
    dt = np.dtype(dtype)
    sdt = np.dtype(dt if s_dtype is None else s_dtype)
    A = np.asarray(A)
    s, bad = squarings_of(theta_of(A.astype(sdt), wmax))
    s[bad] = 0
    Cd = C.astype(dt)
    scale = np.ldexp(np.ones(A.shape[0], dtype=dt), -s)
    scale[bad] = np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        As = A.astype(dt) * scale[:, None]
        N = A.shape[1]
        e0 = np.zeros((1, N), dtype=dt)
        e0[0, 0] = 1
        m = DEGREE[sdt] if degree is None else degree   # (the program's degree: a longdouble evaluation of a float32 program sums its 8 terms)
        q = [None] * (m + 1)
        q[m] = np.broadcast_to(e0, As.shape).copy()
        for k in range(m, 0, -1):
            q[k - 1] = e0 + _gp(Cd, As, q[k]) / dt.type(k)
        Y = [q[0]]
        for i in range(int(s.max()) if s.size else 0):
            Y.append(np.where((i < s)[:, None], _gp(Cd, Y[i], Y[i]), Y[i]))
    out = Y[-1].copy()
    out[bad] = np.nan
    if keep:
        return out, s, bad, (Cd, As, scale, q, Y)
    return out, s, bad


def reverse(metric, grades, A, g, dtype=np.float64, s_dtype=None):
    """cotangent of A over S for the cotangent g of gexp(A) over S: the reverse sweep in `dtype` (s as forward computes it)"""
    dt = np.dtype(dtype)
    _, s, _, (Cd, As, scale, q, Y) = forward(metric, grades, A, dtype, s_dtype, keep=True)
    gb = np.asarray(g).astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(Y) - 2, -1, -1):
            gb = np.where((i < s)[:, None], _adjl(Cd, gb, Y[i]) + _adjr(Cd, gb, Y[i]), gb)
        da = np.zeros_like(gb)
        for k in range(1, len(q)):
            h = gb / dt.type(k)
            da = da + _adjl(Cd, h, q[k])
            gb = _adjr(Cd, h, As)
        return da * scale[:, None]


def restrict(metric, grades, v):
    """zero the components of vectors over S whose grade the operand does not hold"""
    metric, grades = _key(metric, grades)
    S = structure(metric, grades)[0]
    keep = np.array([inu.grade(b) in grades for b in S])
    return np.where(keep[None], v, 0)


# ---- the mpmath reference -------------------------------------------------------------------------------------------------------
def exp_reference(metric, grades, A, method="series", dps=50):
    """exp(A) over S per item, correctly rounded to float64 from an mpmath evaluation at `dps` digits"""
    import mpmath as mp
    metric, grades = _key(metric, grades)
    _, C, _ = structure(metric, grades)
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[1]
    out = np.zeros_like(A)
    with mp.workdps(dps + 15):
        tiny = mp.mpf(10) ** (-(dps + 10))
        nz = [[(j, int(C[r, j])) if C[r, j] in (1.0, -1.0) else (j, mp.mpf(float(C[r, j]))) for j in range(N) if C[r, j] != 0.0] for r in range(N)]
        for it in range(A.shape[0]):
            a = [mp.mpf(float(x)) for x in A[it]]
            if method == "expm":
                L = mp.matrix(N, N)
                for r in range(N):
                    for j, c in nz[r]:
                        L[r, j] = c * a[r ^ j]
                E = mp.expm(L)
                y = [E[r, 0] for r in range(N)]
            else:
                cols = [[j for j, _ in nz[r]] for r in range(N)]
                la = [[c * a[r ^ j] for j, c in nz[r]] for r in range(N)]
                term = [mp.mpf(1 if r == 0 else 0) for r in range(N)]
                y = list(term)
                k = 0
                while True:
                    k += 1
                    term = [mp.fdot(la[r], [term[j] for j in cols[r]]) / k for r in range(N)]
                    y = [u + t for u, t in zip(y, term)]
                    if max(abs(t) for t in term) <= tiny * max(1, max(abs(u) for u in y)) and k > 4:
                        break
            out[it] = [float(u) for u in y]
    return out


def forward_error(y, ref, N, eps, theta):
    """per item ||y - ref||_inf in units of N eps max(1, theta) ||ref||_inf"""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(y - ref).max(axis=1) / (N * eps * np.maximum(1.0, theta) * np.abs(ref).max(axis=1))


def gradient_error(got, want, N, eps, theta, g, y):
    """per item ||got - want||_inf in units of N eps max(1, theta) ||g||_inf ||y||_inf (y = exp(A))"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max(axis=1) / (N * eps * np.maximum(1.0, theta) * np.abs(g).max(axis=1) * np.abs(y).max(axis=1))


# the worst gradient_error of `reverse` in the program's dtype against `reverse` in longdouble over the inputs of
# tests/test_gexp_host.py, rounded up (measured there on every run; the GPU's bound is 4 x this)
GRAD_SCALE = {np.dtype(np.float32): 0.33, np.dtype(np.float64): 0.34}   # measured 0.320 / 0.337


def random_operand(metric, grades, batch, theta, rng, dtype=np.float32):
    """vectors over S, U(-1, 1) on the components of `grades`, normalised to sum |A| = theta (representable in `dtype`)"""
    metric, grades = _key(metric, grades)
    S = structure(metric, grades)[0]
    held = np.array([inu.grade(b) in grades for b in S])
    A = np.where(held[None], rng.uniform(-1.0, 1.0, (batch, len(S))), 0.0)
    A *= theta / np.abs(A).sum(axis=1, keepdims=True)
    return A.astype(dtype).astype(np.float64)
