"""Reverse mode through exp / log on the host (GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD).  No GPU.

  * explog_grad_numpy.py -- the closed-form adjoint in numpy f64, the yardstick of test_gpu_explog_vjp.py -- against central
    differences of the ORACLE's forward extension (OG_EVAL_EXT_EXPLOG): h = 1e-6, tolerance 1e-6 |g| max(1, |row|);
  * h(s) against exact rational / long double sums of its Taylor terms on both sides of the series thresholds;
  * the shape of the adjoint program gaast_program_vjp builds, the wire format, the refusals;
  * tests/cpp/explog_vjp_sanitize_driver.cpp (own main) under -fsanitize=address,undefined.
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import explog_grad_numpy as eg
import gaast_amd as ga
from gaast_amd import _lib
from helpers import HipBackend, oracle_eval_batch, plan_sources
from oracle import pyoracle as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = og.EVAL_EXT_EXPLOG
GRAD = ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD
R3, R11, R31, PGA, CGA, R21 = [1.0] * 3, [1.0, -1.0], [-1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0, -1.0], [1.0, 1.0, -1.0]


def wedge_rows(n, uv):
    """rows of simple bivectors u ^ v (components in the reference's order) from uv = [batch, 2 n]"""
    u, v = uv[:, :n], uv[:, n:]
    cols = [(i, j) for j in range(n) for i in range(j)]
    return np.stack([u[:, i] * v[:, j] - u[:, j] * v[:, i] for i, j in cols], axis=1)


def _directional(metric, k, op, grades_in, rows_of, params, rng, h=1e-6):
    """<g, (F(x(p + h v)) - F(x(p - h v))) / 2h> against <adjoint(g), (x(p + h v) - x(p - h v)) / 2h>: the oracle evaluates F only on
    its domain (k-vectors whose square is scalar), so the rows move along a parametrisation x(p) that stays inside it."""
    n, alg = len(metric), eg.Algebra(metric)
    build = (lambda B: B.input(0, grades_in, n).exp()) if op == "exp" else (lambda B: B.input(0, grades_in, n).log())
    batch = params.shape[0]
    rows = rows_of(params)
    y, mask = oracle_eval_batch(build, metric, {0: rows}, batch, mode=EXT)
    out_grades = [g for g in range(n + 1) if (mask >> g) & 1]
    g = rng.uniform(-1.0, 1.0, y.shape)
    bits, gbits = eg.rows_to_bits(n, grades_in, rows), eg.rows_to_bits(n, out_grades, g)
    fwd = eg.exp_forward(alg, k, bits) if op == "exp" else eg.log_forward(alg, k, bits)
    assert np.allclose(eg.bits_to_rows(n, out_grades, fwd), y, rtol=1e-13, atol=1e-13)
    adj = eg.exp_adjoint(alg, k, bits, gbits) if op == "exp" else eg.log_adjoint(alg, k, bits, gbits, 0 in grades_in)
    adj = eg.bits_to_rows(n, grades_in, adj)
    for _ in range(4):
        v = rng.uniform(-1.0, 1.0, params.shape)
        xp, xm = rows_of(params + h * v), rows_of(params - h * v)
        yp, _ = oracle_eval_batch(build, metric, {0: xp}, batch, mode=EXT)
        ym, _ = oracle_eval_batch(build, metric, {0: xm}, batch, mode=EXT)
        fd = np.sum(g * (yp - ym), axis=1) / (2 * h)
        an = np.sum(adj * (xp - xm), axis=1) / (2 * h)
        tol = 1e-6 * np.linalg.norm(g, axis=1) * np.maximum(1.0, np.linalg.norm(rows, axis=1))
        assert np.all(np.abs(fd - an) <= tol), float(np.max(np.abs(fd - an) / tol))


CASES = {
    # name: (metric, k, op, input grades, rows(params), params(rng, batch))
    "r3_bivector": (R3, 2, "exp", [2], lambda p: p, lambda r, b: r.uniform(-1.5, 1.5, (b, 3))),
    "r11_bivector": (R11, 2, "exp", [2], lambda p: p, lambda r, b: r.uniform(-1.5, 1.5, (b, 1))),
    "r31_boost": (R31, 2, "exp", [2], lambda p: np.concatenate([p, np.zeros((p.shape[0], 5))], axis=1), lambda r, b: r.uniform(-1.5, 1.5, (b, 1))),
    "pga_bivector": (PGA, 2, "exp", [2], lambda p: wedge_rows(4, p), lambda r, b: r.uniform(-1.0, 1.0, (b, 8))),
    # e_0 ^ v: every component holds e_0, s == 0 exactly
    "pga_translator": (PGA, 2, "exp", [2],
                       lambda p: wedge_rows(4, np.concatenate([np.ones((p.shape[0], 1)), np.zeros((p.shape[0], 4)), p], axis=1)),
                       lambda r, b: r.uniform(-1.0, 1.0, (b, 3))),
    "pga_series_1e-8": (PGA, 2, "exp", [2], lambda p: 1e-8 * wedge_rows(4, p), lambda r, b: r.uniform(-1.0, 1.0, (b, 8))),
    "pga_series_1e-4": (PGA, 2, "exp", [2], lambda p: 1e-4 * wedge_rows(4, p), lambda r, b: r.uniform(-1.0, 1.0, (b, 8))),
    "cga_bivector": (CGA, 2, "exp", [2], lambda p: 0.7 * wedge_rows(5, p), lambda r, b: r.uniform(-1.0, 1.0, (b, 10))),
    "cga_log": (CGA, 2, "log", [0, 2], lambda p: np.concatenate([p[:, :1], 0.5 * wedge_rows(5, p[:, 1:])], axis=1),
                lambda r, b: np.concatenate([r.uniform(1.5, 3.0, (b, 1)), r.uniform(-1.0, 1.0, (b, 10))], axis=1)),
    "cga_log_series": (CGA, 2, "log", [0, 2], lambda p: np.concatenate([p[:, :1], 0.05 * wedge_rows(5, p[:, 1:])], axis=1),
                       lambda r, b: np.concatenate([r.uniform(1.5, 3.0, (b, 1)), r.uniform(-1.0, 1.0, (b, 10))], axis=1)),
    "r3_log": (R3, 2, "log", [0, 2], lambda p: p, lambda r, b: r.uniform(-1.5, 1.5, (b, 4))),      # a of either sign: atan2's branches
    "r21_vector": (R21, 1, "exp", [1], lambda p: p, lambda r, b: r.uniform(-1.5, 1.5, (b, 3))),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_adjoint_matches_central_differences_of_the_oracle(name):
    metric, k, op, grades, rows_of, params = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    _directional(metric, k, op, grades, rows_of, params(rng, 24), rng)


def test_translator_rows_have_a_square_of_exactly_zero():
    metric, k, _, grades, rows_of, params = CASES["pga_translator"]
    rows = rows_of(params(np.random.default_rng(0), 16))
    bits = eg.rows_to_bits(4, grades, rows)
    assert np.all(bits * bits @ eg.Algebra(metric).sq == 0.0) and np.abs(rows).max() > 0.1


def _exp_h_exact(s, terms=60):
    s = Fraction(s)
    return float(sum(Fraction(2 * n, math.factorial(2 * n + 1)) * s ** (n - 1) for n in range(1, terms)))


def _log_h_exact(a, s, terms=400):
    a, u = Fraction(a), Fraction(s) / (Fraction(a) * Fraction(a))
    return float(sum(Fraction(2 * n, 2 * n + 1) * u ** (n - 1) for n in range(1, terms)) / a ** 3)


@pytest.mark.parametrize("mag", [0.0, 1e-16, 1e-8, 1e-4, 1e-2, 1.0, 3.99, 4.0, 9.0])
def test_exp_h_on_both_sides_of_the_series_threshold(mag):
    """the series below |s| = 4 (truncation below eps / 8), the quotient from there on: (|c0| + |f|) / |c0 - f| <= 3 amplifies the
    few-ulp errors of libm's cos / sin / cosh / sinh -- 16 eps covers both"""
    for s in (mag, -mag):
        got, want = float(eg.exp_h(np.array([s]))[0]), _exp_h_exact(s)
        assert abs(got - want) <= 16 * 2.0 ** -52 * abs(want), (s, got, want)
    assert float(eg.exp_h(np.array([0.0]))[0]) == 1.0 / 3.0


@pytest.mark.parametrize("mag", [0.0, 1e-16, 1e-8, 1e-4, 1e-2, 0.2499, 0.25, 0.6])
def test_log_h_on_both_sides_of_the_series_threshold(mag):
    """a = 1.25; the series below |s / a^2| = 1/4, the quotient from there on (amplification <= 10.4 at the threshold: 64 eps)"""
    a = 1.25
    for u in (mag, -mag):
        s = u * a * a
        got, want = float(eg.log_h(np.array([a]), np.array([s]))[0]), _log_h_exact(a, s)
        assert abs(got - want) <= 64 * 2.0 ** -52 * abs(want), (u, got, want)
    assert float(eg.log_h(np.array([2.0]), np.array([0.0]))[0]) == 2.0 / 3.0 / 8.0
    # a < 0 with s < 0 is not analytic at s = 0 (atan2 jumps to pi): the quotient, never the series
    got = float(eg.log_h(np.array([-1.25]), np.array([-1e-4]))[0])
    m = 1e-2
    assert np.isclose(got, (-1.25 / (1.25 ** 2 + 1e-4) - math.atan2(m, -1.25) / m) / -1e-4, rtol=1e-9)


# ---- the adjoint program ----------------------------------------------------------------------------------------------
_alive = []


def _desc(build, metric, flags):
    spec = build(HipBackend()).specialize(metric, flags=flags)
    _alive.append(spec)
    return spec.program_desc()


def _vjp(d, slot):
    img = C.c_void_p()
    return _lib.lib().gaast_program_vjp(C.byref(d), slot, C.byref(img)), img


def _explog(B):
    x, y = B.input(0, [2], 3), B.input(1, [2], 3)
    return x.exp() * y


def test_vjp_through_exp_holds_one_adjoint_node_over_cotangent_and_operand():
    d = _desc(_explog, 3, GRAD)
    st, img = _vjp(d, 0)
    assert st == 0, _lib.lib().gaast_expr_last_error()
    a = _lib.lib().gaast_program_image_desc(img).contents
    adj = [i for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_EXP_ADJ]
    assert len(adj) == 1 and not any(a.nodes[i].opcode == _lib.OP_LOG_ADJ for i in range(a.n_nodes))
    nd = a.nodes[adj[0]]
    assert 0 <= nd.child0 < adj[0] and 0 <= nd.child1 < adj[0]
    operand, cot = a.nodes[nd.child1], a.nodes[nd.child0]
    # child1: the forward operand (input 0, a bivector); the node's own mask is the operand's
    assert operand.opcode == _lib.OP_INPUT and operand.input_slot == 0 and operand.minimal_grade_mask == 1 << 2
    assert nd.minimal_grade_mask == operand.minimal_grade_mask and nd.vec_space_dim == 3
    # child0: derived from the cotangent (slot n_inputs), within the forward exp node's grades {0, 2}
    assert cot.minimal_grade_mask and cot.minimal_grade_mask & ~0b101 == 0

    def reaches_cotangent(i):
        n = a.nodes[i]
        if n.opcode == _lib.OP_INPUT:
            return n.input_slot == d.n_inputs
        return reaches_cotangent(n.child0) or (n.opcode in (_lib.OP_ADD, _lib.OP_PRODUCT) and reaches_cotangent(n.child1))
    assert reaches_cotangent(nd.child0)
    assert a.flags == d.flags and a.nodes[a.root].minimal_grade_mask == 1 << 2
    _lib.lib().gaast_program_image_free(img)


def test_exp_log_alone_still_has_no_vjp_through_exp():
    d = _desc(_explog, 3, ga.FLAG_EXP_LOG)
    st, img = _vjp(d, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED" and not img.value
    # the grad flag means nothing without GAAST_FLAG_EXP_LOG
    d = _desc(_explog, 3, ga.FLAG_EXP_LOG_GRAD)
    st, img = _vjp(d, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED" and not img.value


def test_adjoint_opcodes_round_trip_through_the_wire_format():
    L = _lib.lib()
    for build, op in ((_explog, _lib.OP_EXP_ADJ), (lambda B: B.input(0, [0, 2], 5).log(), _lib.OP_LOG_ADJ)):
        d = _desc(build, 3 if op == _lib.OP_EXP_ADJ else CGA, GRAD)
        st, img = _vjp(d, 0)
        assert st == 0
        a = L.gaast_program_image_desc(img).contents
        ops = [(a.nodes[i].opcode, a.nodes[i].child0, a.nodes[i].child1) for i in range(a.n_nodes)]
        assert sum(o[0] == op for o in ops) == 1
        n = L.gaast_program_serialize(C.byref(a), None, 0)
        buf = (C.c_ubyte * n)()
        assert L.gaast_program_serialize(C.byref(a), buf, n) == n
        img2 = C.c_void_p(L.gaast_program_deserialize(buf, n))
        assert img2.value
        a2 = L.gaast_program_image_desc(img2).contents
        assert [(a2.nodes[i].opcode, a2.nodes[i].child0, a2.nodes[i].child1) for i in range(a2.n_nodes)] == ops
        buf2 = (C.c_ubyte * n)()
        assert L.gaast_program_serialize(C.byref(a2), buf2, n) == n and bytes(buf) == bytes(buf2)
        L.gaast_program_image_free(img2)
        L.gaast_program_image_free(img)


def test_host_driver_is_clean_under_asan_and_ubsan(tmp_path):
    """the new vjp.cpp path, the lowering of the adjoint opcodes and their generated statements in a stand-alone program: also the
    refusal of an OP_EXP_ADJ program without GAAST_FLAG_EXP_LOG (plan.unsupported -> UNIMPLEMENTED at program_create), and of
    exp of a bare scalar"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path / "explog_vjp_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "explog_vjp_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("ALL OK")
