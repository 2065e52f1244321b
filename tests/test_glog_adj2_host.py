"""Second order through the general logarithm (GAAST_OP_GLOG_ADJ2, GAAST_FLAG_GLOG_GRAD2) on the host: the numpy restatement of the
node (glog_adj2_numpy.py) against central differences, the inverse-function identity and the symmetry of the second derivative, three
mutations, the error scales of the restatement that bound the GPU tests, the images gaast_program_vjp builds under the four settings
of the two flags, and the lowered Step::GLOG_ADJ2 tables.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined
(tests/cpp/glog_adj2_sanitize_driver.cpp) and run once: it must end clean, and the tables it prints from the lowered plans are what
the tests below compare with numpy.

Bounds.  The restatement checks run in numpy.longdouble (eps = 1.1e-19).  The central differences take phi(A) = <g, log_jvp_reference(A,
h)> along a direction d with the step 1e-6 max |A|: truncation is t^2 |phi'''| / 6, relative to |phi'| about 1e-12 times the ratio of
the third to the first derivative of phi, which for the operands scaled by 0.01 is some 1e4 (derivatives of log grow like |A|^-k);
rounding is the reference's 1e-18 |phi| / t.  The bound is 5e-8 relative, 1e-7 at N = 2 (measured: below 1e-9 everywhere); a wrong
formula misses by a percent at the least.  The composed identity  -GLOG_ADJ(GEXP_ADJ2(GLOG_ADJ(g, A), GLOG_JVP(h, A), glog A), A)  and
the symmetry in (h, m) compare evaluations through some fifty solves of condition below 1e3: 1e-12 relative leaves four digits.

Mutation check: dropping gamma, dropping the ADJR(w, t_i) + ADJL(w, t_i) term of the chain, or dropping the factor 2^s moves the
reference by order one on some item of every case, far beyond the bound the GPU is held to in f64 (4 x LOG_ADJ2_SCALE units)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp2_numpy as g2x
import gexp_numpy as gx
import glog_adj2_numpy as g2
import glog_numpy as gl
import inverse_numpy as inu
import root_log_jvp_numpy as rl
import test_vjp_host as H
from helpers import plan_sources
from test_vjp2_host import _image, _ok, _serialize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
ODD = [2.0, -0.5, 1.0]
SEED = 20261021
JVP, GRAD2 = ga.FLAG_GSQRT_GLOG_JVP, ga.FLAG_GLOG_GRAD2
BOTH = JVP | GRAD2
LD = np.longdouble
FIVE = ["R1", "R3-even", "PGA3D-even", "PGA3D", "CGA"]


def test_constants():
    assert (_lib.OP_GLOG_ADJ2, ga.FLAG_GLOG_GRAD2) == (26, 0x10000)
    assert _lib.MORE_OP_NAMES[26] == "GeneralLogarithmAdjoint2"
    assert _lib.op_name(26) == "GeneralLogarithmAdjoint2" and _lib.op_name(25) == "GeneralLogarithmJvp" and _lib.op_name(0) == "GradedObj"


# ---- the restatement, in longdouble -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweeps():
    """per case of FIVE: (A, h, g, m, the reference of (g, h)), computed once"""
    out = {}
    for name in FIVE:
        metric, grades, _ = rl.CASES[name]
        rng = np.random.default_rng(SEED)
        A, h, g = rl.sweep_operands(name, rng)
        m = rng.uniform(-1, 1, A.shape)
        out[name] = (A, h, g, m, g2.log_adj2_reference(metric, grades, A, g, h))
    return out


@pytest.mark.parametrize("name", FIVE)
def test_reference_against_central_differences(sweeps, name):
    metric, grades, N = rl.CASES[name]
    A, h, g, _, ref = sweeps[name]
    assert np.isfinite(ref).all()
    Al, gl_ = A.astype(LD), g.astype(LD)
    phi = lambda X: (gl_ * rl.log_jvp_reference(metric, grades, X, h)).sum(axis=1)
    rng = np.random.default_rng(SEED + 1)
    worst = 0.0
    for _ in range(3):
        d = rng.uniform(-1, 1, A.shape).astype(LD)
        t = (LD(1e-6) * np.abs(Al).max(axis=1))[:, None]
        fd = (phi(Al + t * d) - phi(Al - t * d)) / (2 * t[:, 0])
        worst = max(worst, float((np.abs(fd - (ref * d).sum(axis=1)) / (np.abs(ref) * np.abs(d)).sum(axis=1)).max()))
    print(f"ADJ2-VS-DIFFERENCES {name}: {worst:.2e}")
    assert worst <= (1e-7 if N == 2 else 5e-8)


@pytest.mark.parametrize("name", FIVE)
def test_reference_against_the_inverse_function_identity(sweeps, name):
    """exp(log A) = A differentiated twice:  GLOG_ADJ2(g, h, A) = -GLOG_ADJ(GEXP_ADJ2(w, u, log A), A),  w = GLOG_ADJ(g, A), u = GLOG_JVP(h, A)"""
    metric, grades, _ = rl.CASES[name]
    A, h, g, _, ref = sweeps[name]
    Y = gl.log_reference(metric, grades, A)
    w = gl.reverse_reference(metric, grades, A, g)
    u = rl.log_jvp_reference(metric, grades, A, h)
    z = g2x.adj2(metric, grades, Y, u, w, LD)
    want = -gl.reverse_reference(metric, grades, A, z)
    rel = float((np.abs(ref - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    print(f"ADJ2-VS-IDENTITY {name}: {rel:.2e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("name", FIVE)
def test_the_second_derivative_is_symmetric(sweeps, name):
    metric, grades, _ = rl.CASES[name]
    A, h, g, m, ref = sweeps[name]
    other = g2.log_adj2_reference(metric, grades, A, g, m)
    lhs, rhs = (ref * m.astype(LD)).sum(axis=1), (other * h.astype(LD)).sum(axis=1)
    scale = (np.abs(ref) * np.abs(m)).sum(axis=1)
    print(f"SYMMETRY {name}: {float((np.abs(lhs - rhs) / scale).max()):.2e}")
    assert np.all(np.abs(lhs - rhs) <= 1e-12 * scale)


@pytest.mark.parametrize("mutation", ["drop_gamma", "drop_chain_term", "drop_scale"])
@pytest.mark.parametrize("name", FIVE)
def test_mutations_move_the_result_beyond_the_f64_bound(sweeps, name, mutation):
    metric, grades, N = rl.CASES[name]
    A, h, g, _, ref = sweeps[name]
    mut = g2.log_adj2_reference(metric, grades, A, g, h, **{mutation: True})
    err = g2.log_adj2_error(mut, ref, g2.EPS[np.dtype(np.float64)], gl.log_reference(metric, grades, A), g2.hessian_norm(metric, grades, A, g), h)
    assert err.max() > 4 * g2.scale_of(g2.LOG_ADJ2_SCALE, N, np.float64), (name, mutation, err.max())


def test_domain_errors_of_the_restatement():
    A = np.array([[-1.0, 0, 0, 0], [1.25, 0.25, 0, 0], [1.0, np.nan, 0, 0]])
    ones = np.ones_like(A)
    out = g2.log_adj2([1.0, 1.0], [0, 1, 2], A, ones, ones)
    assert np.isnan(out[[0, 2]]).all() and np.isfinite(out[1]).all()


# ---- the scales of the GPU bounds ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references():
    """per case: (A, h, g, the reference, log A, ||G||_inf), the values the GPU tests compare with too"""
    out = {}
    for name, (metric, grades, _) in rl.CASES.items():
        A, h, g = rl.case_operands(name)
        out[name] = (A, h, g, g2.log_adj2_reference(metric, grades, A, g, h), gl.log_reference(metric, grades, A).astype(np.float64),
                     g2.hessian_norm(metric, grades, A, g))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(rl.CASES))
def test_restatement_error_defines_the_scales(references, name, dtype):
    """the worst error of the restatement in the program's dtype against the longdouble reference over the items of the GPU tests:
    covered by the recorded scale"""
    metric, grades, N = rl.CASES[name]
    A, h, g, ref, log_a, gn = references[name]
    assert np.isfinite(ref).all()
    worst = g2.log_adj2_error(g2.log_adj2(metric, grades, A, g, h, dtype), ref, g2.EPS[np.dtype(dtype)], log_a, gn, h).max()
    print(f"SCALES {name} {np.dtype(dtype).name}: LOG_ADJ2 {worst:.3f}")
    assert worst <= g2.scale_of(g2.LOG_ADJ2_SCALE, N, dtype), (name, worst)


# ---- images -------------------------------------------------------------------------------------------------------------------------
def _glog(B):
    return B.input(0, [0, 2], 3).glog()


def _pose_error(B):
    return (B.input(0, [0, 2, 4], 4) * B.input(1, [0, 2, 4], 4).inv()).glog().g(2)


def _ops(a):
    return [a.nodes[i].opcode for i in range(a.n_nodes)]


def _the_adj2(a):
    hits = [a.nodes[i] for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_GLOG_ADJ2]
    assert len(hits) == 1
    return hits[0]


def _slot_of(a, node):
    nd = a.nodes[node]
    return nd.input_slot if nd.opcode == _lib.OP_INPUT else None


def test_second_order_images_hold_exactly_one_adj2_node():
    d = H._desc(_glog, 3, flags=BOTH)
    a = _ok(d, 0)
    assert _lib.OP_GLOG_ADJ2 not in _ops(a) and _ops(a).count(_lib.OP_GLOG_ADJ) == 1
    # vjp(0).vjp(0): the GLOG_ADJ(g, A) node through its operand gives GLOG_ADJ2(g, k, A)
    h2 = _ok(a, 0)
    nd = _the_adj2(h2)
    assert (_slot_of(h2, nd.child0), _slot_of(h2, nd.child1), _slot_of(h2, nd.input_slot)) == (d.n_inputs, a.n_inputs, 0)
    assert nd.minimal_grade_mask == 0b101 and h2.nodes[nd.input_slot].minimal_grade_mask == 0b101
    assert _lib.OP_GLOG_ADJ not in _ops(h2) and _lib.OP_GLOG_JVP not in _ops(h2) and h2.flags & BOTH == BOTH
    # forward mode holds the tangent node alone; its gradient in the operand is GLOG_ADJ2(k, h, A)
    j = _ok(a, d.n_inputs)
    assert _ops(j).count(_lib.OP_GLOG_JVP) == 1 and _lib.OP_GLOG_ADJ2 not in _ops(j)
    j2 = _ok(j, 0)
    nd = _the_adj2(j2)
    assert (_slot_of(j2, nd.child0), _slot_of(j2, nd.child1), _slot_of(j2, nd.input_slot)) == (j.n_inputs, a.n_inputs, 0)
    assert nd.minimal_grade_mask == 0b101
    # the pose error, projected to its bivector: both slots, the node's mask the even grades of the operand m * t^-1
    p = H._desc(_pose_error, PGA, flags=BOTH)
    for s in H._user_slots(p):
        ap = _ok(p, s)
        nd = _the_adj2(_ok(ap, s))
        assert nd.minimal_grade_mask == 0b10101
        jp = _ok(ap, p.n_inputs)
        assert _ops(jp).count(_lib.OP_GLOG_JVP) == 1 and _lib.OP_GLOG_ADJ2 not in _ops(jp)
        for s2 in H._user_slots(p):        # mixed second derivatives build too
            assert _ops(_ok(ap, s2)).count(_lib.OP_GLOG_ADJ2) >= 1


def test_third_order_is_refused_by_name():
    d = H._desc(_glog, 3, flags=BOTH)
    h2 = _ok(_ok(d, 0), 0)
    for s in (0, 1, 2):                     # through the operand, through g and through h: the node on the path is refused
        st, _ = _image(h2, s)
        assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
        assert _lib.lib().gaast_expr_last_error().decode() == "third-order reverse mode through GAAST_OP_GLOG_ADJ2 is not implemented"


@pytest.mark.parametrize("build,metric", [(_glog, 3), (_pose_error, PGA)], ids=["glog", "pose"])
def test_with_one_flag_alone_everything_is_as_before(build, metric):
    d0, dj, dg, db = (H._desc(build, metric, flags=f) for f in (0, JVP, GRAD2, BOTH))
    for s in H._user_slots(d0):
        a0, aj, ag, ab = (_ok(d, s) for d in (d0, dj, dg, db))
        # first order: the same bytes but the flags word
        x, y, z = bytearray(_serialize(aj)), bytearray(_serialize(ab)), bytearray(_serialize(ag))
        diff = [i for i in range(len(x)) if x[i] != y[i]]
        assert len(x) == len(y) == len(z) and len(diff) == 1 and x[diff[0]] ^ y[diff[0]] == GRAD2 >> 16 and ab.flags ^ aj.flags == GRAD2
        assert [i for i in range(len(x)) if z[i] != y[i]] == [diff[0] - 1] and ag.flags ^ ab.flags == JVP
        # second order through the operand: today's status and words
        st, _ = _image(aj, s)
        assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
        assert _lib.lib().gaast_expr_last_error().decode() == "reverse mode through GAAST_OP_GLOG_ADJ with respect to its operand is not implemented"
        for a in (a0, ag):
            st, _ = _image(a, s)
            assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
            assert _lib.lib().gaast_expr_last_error().decode() == "second-order reverse mode through GAAST_OP_GLOG_ADJ is not implemented"
        # forward mode is the same image with and without GRAD2
        fj, fb = _ok(aj, d0.n_inputs), _ok(ab, d0.n_inputs)
        assert _ops(fj) == _ops(fb) and len(_serialize(fj)) == len(_serialize(fb))
        st, _ = _image(fj, s)
        assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED" and "GAAST_OP_GLOG_JVP with respect to its operand" in _lib.lib().gaast_expr_last_error().decode()


def test_images_round_trip_through_the_wire_format():
    d = H._desc(_pose_error, PGA, flags=BOTH)
    a = _ok(d, 0)
    for img in (_ok(a, 0), _ok(a, 1), _ok(_ok(a, d.n_inputs), 0)):
        assert _lib.OP_GLOG_ADJ2 in _ops(img)
        data = _serialize(img)
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        h = C.c_void_p(_lib.lib().gaast_program_deserialize(buf, len(data)))
        assert h.value
        try:
            b = _lib.lib().gaast_program_image_desc(h).contents
            assert _serialize(b) == data
            assert [(b.nodes[i].opcode, b.nodes[i].child0, b.nodes[i].child1, b.nodes[i].input_slot) for i in range(b.n_nodes)] == \
                [(img.nodes[i].opcode, img.nodes[i].child0, img.nodes[i].child1, img.nodes[i].input_slot) for i in range(img.n_nodes)]
        finally:
            _lib.lib().gaast_program_image_free(h)


# ---- the host code under sanitizers, and the lowered tables -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (a stand-alone program, compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("glog_adj2_asan") / "glog_adj2_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "glog_adj2_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")
    for n in range(1, 8):
        assert f"ok  glog(x) full n={n}\n" in driver and (n == 1 or f"ok  glog(x) even n={n}\n" in driver)
    for what in ("glog(m * t.inv())", "glog(m * t.inv()).g(2)", "raw tables", "raw malformed nodes"):
        assert f"ok  {what}\n" in driver


# tag -> (metric, operand grades, flipped grades of the operand read, grades of g, grades of h): the result holds the operand's grades
TABLES = {"pga": (PGA, [0, 1, 2, 3, 4], {2, 3}, [0, 1, 2, 4], [1, 2, 3]), "cga": (CGA, [2], set(), [0, 4], [2]),
          "odd": (ODD, [0, 1, 2, 3], set(), [0, 1, 2, 3], [0, 1, 2, 3])}


def _lines(driver, what, tag):
    return [f for f in (line.split() for line in driver.splitlines()) if len(f) > 3 and f[0] == what and f[1] == tag]


@pytest.mark.parametrize("tag", sorted(TABLES))
def test_lowered_tables_match_numpy(driver, tag):
    """the blade list, the offsets of A, g, h and res, the folded signs of the operand read, and the coefficients behind the four sign
    tables -- L, R (glog_numpy.right_matrix), and the two adjoint products (gexp_numpy._adjl / _adjr) -- entry for entry"""
    metric, grades, flip, g_grades, h_grades = TABLES[tag]
    n = len(metric)
    S, Cm, _ = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    outs = {int(f[3]): (int(f[2]),) + tuple(int(v) for v in f[4:10]) for f in _lines(driver, "GA2OUT", tag)}
    tab = {(int(f[2]), int(f[3])): tuple(float(v) for v in f[4:8]) for f in _lines(driver, "GA2TAB", tag)}
    where = lambda gr: {b: i for i, b in enumerate(inu.row_blades(n, tuple(gr)))}
    a_w, g_w, h_w = where(grades), where(g_grades), where(h_grades)
    assert sorted(outs) == list(range(N)) and len(tab) == N * N
    for j in range(N):
        Nn, blade, a_off, res_off, g_off, h_off, neg = outs[j]
        assert (Nn, blade) == (N, S[j])
        assert a_off == a_w.get(blade, -1) and res_off == a_w.get(blade, -1) and g_off == g_w.get(blade, -1) and h_off == h_w.get(blade, -1)
        assert neg == (1 if inu.grade(blade) in flip and blade in a_w else 0)
    eye = np.eye(N)
    R = np.stack([gl.right_matrix(Cm, eye[k:k + 1])[0] for k in range(N)])                  # R[k][r][j]: the coefficient of M[k] in R_M[r][j]
    AL = np.stack([np.stack([gx._adjl(Cm, eye[k:k + 1], eye[b:b + 1])[0] for b in range(N)]) for k in range(N)])   # AL[k][b][a]: of G[k] Z[b] in ADJL(G, Z)[a]
    AR = np.stack([np.stack([gx._adjr(Cm, eye[k:k + 1], eye[a:a + 1])[0] for a in range(N)]) for k in range(N)])   # AR[k][a][b]: of G[k] X[a] in ADJR(G, X)[b]
    for r in range(N):
        for j in range(N):
            cf, cr, cl, ca = tab[r, j]
            assert cf == Cm[r, j] and cr == R[r ^ j, r, j] == Cm[r, r ^ j], (r, j)
            assert cl == AL[r ^ j, j, r] == Cm[r ^ j, j], (r, j)       # ADJL(G, Z)[a = r] = sum_b coeff(r, b) Z[b] G[r xor b]
            assert ca == AR[r ^ j, j, r] == Cm[r ^ j, r], (r, j)       # ADJR(G, X)[b = r] = sum_a coeff(a, r) X[a] G[a xor r]
