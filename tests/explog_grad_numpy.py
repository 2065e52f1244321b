"""Closed-form reverse mode of exp / log in numpy float64 (GAAST_OP_EXP_ADJ / GAAST_OP_LOG_ADJ, include/gaast_hip.h), written
from the formulas alone -- the yardstick of tests/test_gpu_explog_vjp.py.  test_vjp_explog_host.py checks it against central
differences of the oracle's forward extension (OG_EVAL_EXT_EXPLOG).

Multivectors are rows over ALL 2^n blades ("bits": column = blade bitmask), one row per item; rows_to_bits / bits_to_rows move
graded rows in and out.  sigma_a = e_a e_a, s = sum sigma_a B_a^2, c0 and f as the forward computes them, branch for branch."""
import numpy as np

EXP_SERIES_BELOW = 4.0     # |s| below which h = (c0 - f) / s is summed from its series (explog_adj_series.hip.hpp: kExpAdjSeriesBelow)
LOG_SERIES_BELOW = 0.25    # |s / a^2| likewise for h = (a / D - f) / s (explog_adj_series.hip.hpp: kLogAdjSeriesBelow)


def _popcount(x):
    return bin(int(x)).count("1")


def blades_in_row_order(n, grades):
    out = []
    for k in sorted(grades):
        out.extend(m for m in range(1 << n) if _popcount(m) == k)
    return np.array(out, dtype=np.int64)


def rows_to_bits(n, grades, rows):
    rows = np.asarray(rows, dtype=np.float64)
    bits = np.zeros((rows.shape[0], 1 << n))
    bits[:, blades_in_row_order(n, grades)] = rows
    return bits


def bits_to_rows(n, grades, bits):
    return bits[:, blades_in_row_order(n, grades)]


class Algebra:
    """Geometric product of a diagonal metric as a dense tensor (n <= 5: at most 32^3 entries)."""

    def __init__(self, metric):
        self.metric = [float(g) for g in metric]
        n = self.n = len(self.metric)
        N = self.N = 1 << n
        T = np.zeros((N, N, N))
        for a in range(N):
            for b in range(N):
                swaps = sum(_popcount((a >> s) & b) for s in range(1, n))
                c = -1.0 if swaps & 1 else 1.0
                for i in range(n):
                    if (a & b) >> i & 1:
                        c *= self.metric[i]
                T[a, b, a ^ b] = c
        self.T = T
        self.sq = np.array([T[a, a, 0] for a in range(N)])              # e_a e_a
        self.grade = np.array([_popcount(a) for a in range(N)])
        self.rev_sign = np.where((self.grade % 4 == 2) | (self.grade % 4 == 3), -1.0, 1.0)

    def grade_mask(self, grades):
        return np.isin(self.grade, list(grades)).astype(np.float64)

    def gp(self, A, B):
        return np.einsum("ia,ib,abc->ic", A, B, self.T)

    def gp_vjp(self, A, B, G):
        """cotangents of A and B for C = A B with cotangent G"""
        return np.einsum("ic,ib,abc->ia", G, B, self.T), np.einsum("ic,ia,abc->ib", G, A, self.T)

    def rev(self, A):
        return A * self.rev_sign


# ---- the scalar functions -----------------------------------------------------------------------------------------------
def exp_c0_f(s):
    """c0, f of k_exp_log, branch for branch (s < 0, s > 0, s == 0, NaN)"""
    s = np.asarray(s, dtype=np.float64)
    c0, f = np.full(s.shape, np.nan), np.full(s.shape, np.nan)
    with np.errstate(all="ignore"):
        neg, pos, zero = s < 0, s > 0, s == 0
        t = np.sqrt(np.abs(s))
        c0[neg], f[neg] = np.cos(t[neg]), np.sin(t[neg]) / t[neg]
        c0[pos], f[pos] = np.cosh(t[pos]), np.sinh(t[pos]) / t[pos]
        c0[zero], f[zero] = 1.0, 1.0
    return c0, f


def log_f(a, s):
    a, s = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(s, dtype=np.float64))
    f = np.full(s.shape, np.nan)
    with np.errstate(all="ignore"):
        neg, pos, zero = s < 0, s > 0, s == 0
        m = np.sqrt(np.abs(s))
        f[neg] = np.arctan2(m[neg], a[neg]) / m[neg]
        f[pos] = np.arctanh(m[pos] / a[pos]) / m[pos]
        f[zero] = 1.0 / a[zero]
    return f


def exp_h_series(s, terms=14):
    """sum_{n >= 1} 2n / (2n + 1)! s^(n-1), Horner"""
    s = np.asarray(s, dtype=np.float64)
    h = np.zeros(s.shape)
    for n in range(terms, 0, -1):
        fact = 1.0
        for i in range(2, 2 * n + 2):
            fact *= i
        h = h * s + 2.0 * n / fact
    return h


def exp_h(s):
    s = np.asarray(s, dtype=np.float64)
    c0, f = exp_c0_f(s)
    with np.errstate(all="ignore"):
        return np.where(np.abs(s) < EXP_SERIES_BELOW, exp_h_series(s), (c0 - f) / s)


def log_h_series(a, s, terms=30):
    """a^-3 sum_{n >= 1} 2n / (2n + 1) u^(n-1), u = s / a^2"""
    with np.errstate(all="ignore"):
        u = s / (a * a)
        h = np.zeros(np.shape(u))
        for n in range(terms, 0, -1):
            h = h * u + 2.0 * n / (2.0 * n + 1.0)
        return h / (a * a * a)


def log_h(a, s):
    a, s = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(s, dtype=np.float64))
    with np.errstate(all="ignore"):
        series = (s == 0) | ((np.abs(s) < LOG_SERIES_BELOW * a * a) & ((a > 0) | (s > 0)))
        D = a * a - s
        return np.where(series, log_h_series(a, s), (a / D - log_f(a, s)) / s)


# ---- exp / log of a k-vector and their adjoints, on bits ----------------------------------------------------------------
def exp_forward(alg, k, B):
    """exp(<B>_k): c0 + f B"""
    Bk = B * alg.grade_mask([k])
    c0, f = exp_c0_f(Bk * Bk @ alg.sq)
    R = f[:, None] * Bk
    R[:, 0] += c0
    return R


def exp_adjoint(alg, k, B, G):
    """dB_i = f g_k[i] + sigma_i B_i (f g_0 + h d)"""
    mk = alg.grade_mask([k])
    Bk, Gk, g0 = B * mk, G * mk, G[:, 0]
    s = Bk * Bk @ alg.sq
    _, f = exp_c0_f(s)
    d = np.sum(Gk * Bk, axis=1)
    return f[:, None] * Gk + alg.sq * Bk * (f * g0 + exp_h(s) * d)[:, None]


def log_forward(alg, k, R):
    """log(a + <R>_k): f(a, s) B (nothing into grade 0)"""
    Bk = R * alg.grade_mask([k])
    return log_f(R[:, 0], Bk * Bk @ alg.sq)[:, None] * Bk


def log_adjoint(alg, k, R, G, with_scalar=True):
    """da = -d / D (operand holds grade 0), dB_i = f g_k[i] + sigma_i B_i h d; a reads 0 when the operand has no grade 0"""
    mk = alg.grade_mask([k])
    a = R[:, 0] if with_scalar else np.zeros(R.shape[0])
    Bk, Gk = R * mk, G * mk
    s = Bk * Bk @ alg.sq
    d = np.sum(Gk * Bk, axis=1)
    with np.errstate(all="ignore"):
        out = log_f(a, s)[:, None] * Gk + alg.sq * Bk * (log_h(a, s) * d)[:, None]
        if with_scalar:
            out[:, 0] = -d / (a * a - s)
    return out


def scale_of(alg, k, op, B):
    """max(|c0|, |f|, |h|) per item: the factor of the GPU tests' bound"""
    Bk = B * alg.grade_mask([k])
    s = Bk * Bk @ alg.sq
    if op == "exp":
        c0, f = exp_c0_f(s)
        return np.maximum(np.maximum(np.abs(c0), np.abs(f)), np.abs(exp_h(s)))
    a = B[:, 0]      # (log has no c0)
    with np.errstate(all="ignore"):
        return np.maximum(np.abs(log_f(a, s)), np.abs(log_h(a, s)))
