"""Independent numpy restatement of the second-order pair of the general multivector exponential (GAAST_OP_GEXP_JVP /
GAAST_OP_GEXP_ADJ2, include/gaast_hip.h), on top of gexp_numpy.py (imported, not edited): one rounding per operation, every sum over
j ascending, nothing shared with gaast_amd/csrc.

    jvp    the Frechet derivative L_A(h): with A_s, q_k, Y_i the forward's (s from A alone) and h_s = 2^-s h,
           qd_m = 0;  qd_(k-1) = (h_s q_k + A_s qd_k) / k,  k = m ... 1;   Yd_0 = qd_0;  Yd_(i+1) = Yd_i Y_i + Y_i Yd_i,  i < s
    adj2   the gradient in A of <g, L_A(h)>: the forward pair recomputed, then with Gd = g, G = 0
           for i = s-1 ... 0:  G <- ((ADJL(G, Y_i) + ADJR(G, Y_i)) + ADJR(Gd, Yd_i)) + ADJL(Gd, Yd_i);  Gd <- ADJL(Gd, Y_i) + ADJR(Gd, Y_i)
           for k = 1 ... m:    w = G / k, wd = Gd / k;  dA_s <- dA_s + (ADJL(w, q_k) + ADJL(wd, qd_k));
                               G <- ADJR(w, A_s) + ADJR(wd, h_s);  Gd <- ADJR(wd, A_s)
           dA = 2^-s dA_s  (restrict it to the operand's grades with gexp_numpy.restrict)

Error units, per item (theta = wmax sum |A_a|, y = exp A):
    jvp    N eps max(1, theta) ||h||_inf ||y||_inf
    adj2   N eps max(1, theta) ||g||_inf ||h||_inf ||y||_inf
JVP_SCALE / ADJ2_SCALE are the worst errors, in those units, of these functions run in the program's dtype against the same functions
in numpy.longdouble with the program's s and m, over the input sweep of tests/test_gexp2_host.py, rounded up; that test measures them
again on every run and asserts that the recorded value covers the measurement.  The GPU's bound is 4 x the recorded scale.  At
N = 2 the unit is two ulps and cancellation in one component dominates (single outliers many times the typical value), so N = 2 has
recorded scales of its own (key "N2") instead of loosening every other size."""
import numpy as np

import gexp_numpy as gx


def _pair(metric, grades, A, h, dtype, s_dtype):
    """the forward pair: (s, Cd, As, hs, scale, q, qd, Y, Yd)"""
    dt = np.dtype(dtype)
    _, s, _, (Cd, As, scale, q, Y) = gx.forward(metric, grades, A, dtype, s_dtype, keep=True)
    with np.errstate(invalid="ignore", over="ignore"):
        hs = np.asarray(h).astype(dt) * scale[:, None]
        m = len(q) - 1
        qd = [None] * (m + 1)
        qd[m] = np.zeros_like(As)
        for k in range(m, 0, -1):
            qd[k - 1] = (gx._gp(Cd, hs, q[k]) + gx._gp(Cd, As, qd[k])) / dt.type(k)
        Yd = [qd[0]]
        for i in range(len(Y) - 1):
            Yd.append(np.where((i < s)[:, None], gx._gp(Cd, Yd[i], Y[i]) + gx._gp(Cd, Y[i], Yd[i]), Yd[i]))
    return s, Cd, As, hs, scale, q, qd, Y, Yd


def jvp(metric, grades, A, h, dtype=np.float64, s_dtype=None):
    """L_A(h) over S for the tangent h over S, computed in `dtype`, s and m those of s_dtype (default dtype); a domain-error item: NaN"""
    return _pair(metric, grades, A, h, dtype, s_dtype)[8][-1]


def adj2(metric, grades, A, h, g, dtype=np.float64, s_dtype=None):
    """the gradient in A (over S, unrestricted) of <g, L_A(h)>, computed in `dtype`"""
    dt = np.dtype(dtype)
    s, Cd, As, hs, scale, q, qd, Y, Yd = _pair(metric, grades, A, h, dtype, s_dtype)
    Gd = np.asarray(g).astype(dt)
    G = np.zeros_like(Gd)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(Y) - 2, -1, -1):
            Gn = ((gx._adjl(Cd, G, Y[i]) + gx._adjr(Cd, G, Y[i])) + gx._adjr(Cd, Gd, Yd[i])) + gx._adjl(Cd, Gd, Yd[i])
            Gdn = gx._adjl(Cd, Gd, Y[i]) + gx._adjr(Cd, Gd, Y[i])
            live = (i < s)[:, None]
            G, Gd = np.where(live, Gn, G), np.where(live, Gdn, Gd)
        da = np.zeros_like(Gd)
        for k in range(1, len(q)):
            w, wd = G / dt.type(k), Gd / dt.type(k)
            da = da + (gx._adjl(Cd, w, q[k]) + gx._adjl(Cd, wd, qd[k]))
            G, Gd = gx._adjr(Cd, w, As) + gx._adjr(Cd, wd, hs), gx._adjr(Cd, wd, As)
        return da * scale[:, None]


def jvp_error(got, want, N, eps, theta, h, y):
    """per item ||got - want||_inf in units of N eps max(1, theta) ||h||_inf ||y||_inf (y = exp(A))"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max(axis=1) / (N * eps * np.maximum(1.0, theta) * np.abs(h).max(axis=1) * np.abs(y).max(axis=1))


def adj2_error(got, want, N, eps, theta, g, h, y):
    """per item ||got - want||_inf in units of N eps max(1, theta) ||g||_inf ||h||_inf ||y||_inf"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max(axis=1) / (N * eps * np.maximum(1.0, theta) * np.abs(g).max(axis=1) * np.abs(h).max(axis=1) * np.abs(y).max(axis=1))


# measured by tests/test_gexp2_host.py::test_restatement_error_defines_the_scales on every run and rounded up.  Measured worst values:
#   N >= 4   JVP 0.848 (f32, R^3) / 0.539 (f64, R^3);   ADJ2 0.980 (f32, R^3) / 1.176 (f64, R^3)
#   N = 2    JVP 1.228 (f32) / 2.294 (f64);             ADJ2 1.978 (f32) / 2.849 (f64)      (257 items per theta)
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
JVP_SCALE = {"N2": {_F32: 1.3, _F64: 2.4}, "N>=4": {_F32: 0.9, _F64: 0.6}}
ADJ2_SCALE = {"N2": {_F32: 2.0, _F64: 2.9}, "N>=4": {_F32: 1.0, _F64: 1.2}}


def scale_of(table, N, dtype):
    return table["N2" if N == 2 else "N>=4"][np.dtype(dtype)]
