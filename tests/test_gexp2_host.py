"""Second order through the general exponential (GAAST_OP_GEXP_JVP / GAAST_OP_GEXP_ADJ2, GAAST_FLAG_GEXP_GRAD2) on the host: the numpy
restatement of the two recurrences (gexp2_numpy.py) against gexp_numpy's reverse sweep and central differences, the images
gaast_program_vjp builds with and without the flag, the lowered Step::GEXP_JVP / Step::GEXP_ADJ2 tables, and the error scales of the
restatement that bound the GPU tests.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined (tests/cpp/gexp2_sanitize_driver.cpp) and
run once: it must end clean, and the tables it prints from the lowered plans are what the tests below compare with numpy.

Bounds.  The restatement checks run in numpy.longdouble (eps = 1.1e-19).  Adjointness compares two evaluations of the same
bilinear form, a few hundred rounded operations per component at most: 1e-15 of sum |g| |L_A(h)| is a thousand times that.  The
central differences use the step 1e-5 on functions whose third derivative is of the order of the function on these inputs
(theta <= 3): truncation about 1e-10 relative, rounding 1e-19 / 1e-5; the bound is 1e-8 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp2_numpy as g2
import gexp_numpy as gx
import inverse_numpy as inu
import test_vjp_host as H
from helpers import plan_sources
from test_vjp2_host import _check_shape, _image, _ok, _serialize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
SEED = 20261021
FLAG = ga.FLAG_GEXP_GRAD2
# name -> (metric, operand grades, N)
CASES = {"R1": ([1.0], [0, 1], 2), "R3-even": ([1.0] * 3, [0, 2], 4), "R3": ([1.0] * 3, [0, 1, 2, 3], 8), "PGA3D-bivector": (PGA, [2], 8),
         "PGA3D": (PGA, [0, 1, 2, 3, 4], 16), "CGA": (CGA, [0, 1, 2, 3, 4, 5], 32), "R7-even-bivector": ([1.0] * 7, [2], 64)}
FAMILY = (_lib.OP_GEXP_ADJ, _lib.OP_GEXP_JVP, _lib.OP_GEXP_ADJ2)


# ---- the restatement, in longdouble -----------------------------------------------------------------------------------------------
def _draw(metric, grades, items, theta, rng):
    """(A, h within the operand's grades, g over S), float32-representable"""
    A = gx.random_operand(metric, grades, items, theta, rng)
    h = gx.restrict(metric, grades, rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64))
    g = rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
    return A, h, g


@pytest.mark.parametrize("theta", [0.1, 0.4, 3.0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_in_longdouble(name, theta):
    metric, grades, N = CASES[name]
    ld = np.longdouble
    rng = np.random.default_rng(SEED + int(theta * 10))
    A, h, g = _draw(metric, grades, 5, theta, rng)
    # the tangent recurrence is the transpose of gexp_numpy.reverse
    jv = g2.jvp(metric, grades, A, h, ld, np.float64)
    rev = gx.reverse(metric, grades, A, g, ld, np.float64)
    lhs, rhs = (g.astype(ld) * jv).sum(axis=1), (rev * h.astype(ld)).sum(axis=1)
    scale = (np.abs(g).astype(ld) * np.abs(jv)).sum(axis=1)
    print(f"ADJOINTNESS {name} theta={theta}: {float((np.abs(lhs - rhs) / scale).max()):.2e}")
    assert np.all(np.abs(lhs - rhs) <= 1e-15 * scale)
    # ... and the derivative of the exponential: central differences of forward(..., degree=20)
    t = ld(1e-5)
    f = lambda X: gx.forward(metric, grades, X, ld, degree=20)[0]
    fd = (f(A.astype(ld) + t * h.astype(ld)) - f(A.astype(ld) - t * h.astype(ld))) / (2 * t)
    rel = float((np.abs(fd - jv).max(axis=1) / np.abs(jv).max(axis=1)).max())
    print(f"JVP-VS-DIFFERENCES {name} theta={theta}: {rel:.2e}")
    assert rel <= 1e-8
    # the second-order sweep: central differences in A of <reverse(A, g), h> along a direction d within the operand's grades
    d = gx.restrict(metric, grades, rng.uniform(-1, 1, A.shape))
    a2 = gx.restrict(metric, grades, g2.adj2(metric, grades, A, h, g, ld, np.float64))
    phi = lambda X: (gx.reverse(metric, grades, X, g, ld, np.float64) * h.astype(ld)).sum(axis=1)
    fd2 = (phi(A.astype(ld) + t * d.astype(ld)) - phi(A.astype(ld) - t * d.astype(ld))) / (2 * t)
    an = (a2 * d.astype(ld)).sum(axis=1)
    scale2 = (np.abs(a2) * np.abs(d).astype(ld)).sum(axis=1)
    rel2 = float((np.abs(fd2 - an) / scale2).max())
    print(f"ADJ2-VS-DIFFERENCES {name} theta={theta}: {rel2:.2e}")
    assert rel2 <= 1e-8


def test_domain_errors_of_the_restatement():
    A = np.array([[0.0, 4096.0, 0, 0], [0.25, 0.25, 0, 0], [0, np.nan, 0, 0]])
    ones = np.ones_like(A)
    for out in (g2.jvp([1.0, 1.0], [0, 1, 2], A, ones), g2.adj2([1.0, 1.0], [0, 1, 2], A, ones, ones)):
        assert np.isnan(out[[0, 2]]).all() and np.isfinite(out[1]).all()


# ---- the scales of the GPU bounds ---------------------------------------------------------------------------------------------------
SCALE_THETAS = [0.1, 0.4, 1.0, 3.0, 8.0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_error_defines_the_scales(name, dtype):
    """the worst error of the restatement in the program's dtype against the longdouble one with the program's s and m, over
    257 (N = 2: the GPU test's batch, where single items cancel badly), 33 or 9 (N = 64) items per theta: covered by the recorded scale"""
    metric, grades, N = CASES[name]
    eps = gx.EPS[np.dtype(dtype)]
    rng = np.random.default_rng(SEED)
    wj = wa = 0.0
    for th in SCALE_THETAS:
        A, h, g = _draw(metric, grades, 257 if N == 2 else 33 if N <= 32 else 9, th, rng)
        y = gx.forward(metric, grades, A, np.longdouble, degree=20)[0].astype(np.float64)
        wj = max(wj, g2.jvp_error(g2.jvp(metric, grades, A, h, dtype), g2.jvp(metric, grades, A, h, np.longdouble, dtype), N, eps, th, h, y).max())
        wa = max(wa, g2.adj2_error(g2.adj2(metric, grades, A, h, g, dtype), g2.adj2(metric, grades, A, h, g, np.longdouble, dtype), N, eps, th, g, h, y).max())
    print(f"SCALES {name} {np.dtype(dtype).name}: JVP {wj:.3f}  ADJ2 {wa:.3f}")
    assert wj <= g2.scale_of(g2.JVP_SCALE, N, dtype), (name, wj)
    assert wa <= g2.scale_of(g2.ADJ2_SCALE, N, dtype), (name, wa)


# ---- images -------------------------------------------------------------------------------------------------------------------------
def _gexp_times(B):
    return B.input(0, [0, 2], 3).gexp() * B.input(1, [0, 2], 3)


def _pga_sandwich(B):
    R, X = B.input(0, [2], 4).gexp(), B.input(1, [3], 4)
    return R * X * R.rev()


PROGRAMS = {"gexp(x) * y": (_gexp_times, 3), "gexp(B) X ~gexp(B)": (_pga_sandwich, PGA)}


def _ops(a):
    return [a.nodes[i].opcode for i in range(a.n_nodes)]


def _reads_slot(a, slot):
    return any(a.nodes[i].opcode == _lib.OP_INPUT and a.nodes[i].input_slot == slot for i in range(a.n_nodes))


def _check_family(a):
    """children in post-order (the third child of GEXP_ADJ2 too), masks as in the table of gaast_expr.h"""
    for i in range(a.n_nodes):
        nd = a.nodes[i]
        if nd.opcode not in FAMILY:
            continue
        assert 0 <= nd.child0 < i and 0 <= nd.child1 < i
        if nd.opcode == _lib.OP_GEXP_ADJ2:
            assert 0 <= nd.input_slot < i
            A, g, h = a.nodes[nd.input_slot], a.nodes[nd.child0], a.nodes[nd.child1]
            assert nd.minimal_grade_mask == A.minimal_grade_mask
            assert h.minimal_grade_mask & ~A.minimal_grade_mask == 0
        else:
            assert nd.input_slot == -1
            A, c0 = a.nodes[nd.child1], a.nodes[nd.child0]
            if nd.opcode == _lib.OP_GEXP_JVP:
                assert c0.minimal_grade_mask & ~A.minimal_grade_mask == 0, "the tangent holds only the operand's grades"
            else:
                assert nd.minimal_grade_mask & ~A.minimal_grade_mask == 0


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_every_slot_of_the_first_order_images_differentiates_with_the_flag(name):
    build, metric = PROGRAMS[name]
    d = H._desc(build, metric, flags=FLAG)
    seen = set()
    for s1 in H._user_slots(d):
        a = _ok(d, s1)
        _check_shape(d, s1, a)
        assert not {_lib.OP_GEXP_JVP, _lib.OP_GEXP_ADJ2} & set(_ops(a))
        for s2 in H._user_slots(a):
            a2 = _ok(a, s2)
            _check_shape(a, s2, a2)
            _check_family(a2)
            seen |= set(_ops(a2)) & set(FAMILY)
    assert seen == set(FAMILY)


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_the_jvp_image_and_its_transpose(name):
    build, metric = PROGRAMS[name]
    d = H._desc(build, metric, flags=FLAG)
    a = _ok(d, 0)                       # the generator's gradient: GEXP_ADJ
    assert _lib.OP_GEXP_ADJ in _ops(a)
    j = _ok(a, d.n_inputs)              # forward mode: the VJP of the VJP with respect to its cotangent
    _check_family(j)
    assert _lib.OP_GEXP_JVP in _ops(j) and _lib.OP_GEXP_ADJ not in _ops(j) and _lib.OP_GEXP_ADJ2 not in _ops(j)
    assert not _reads_slot(j, d.n_inputs), "the JVP image never reads the first cotangent"
    r = j.nodes[j.root]
    assert (r.minimal_grade_mask, r.vec_space_dim) == (d.nodes[d.root].minimal_grade_mask, d.vec_space_dim)
    tangent = a.n_inputs                # the second cotangent is the tangent of the JVP image
    t = _ok(j, tangent)                 # its transpose is the first-order gradient again
    _check_family(t)
    assert _lib.OP_GEXP_ADJ in _ops(t) and _lib.OP_GEXP_JVP not in _ops(t)
    # with respect to the generator the JVP node gives GEXP_ADJ2, and a third order through that is refused by name
    h = _ok(j, 0)
    _check_family(h)
    assert _lib.OP_GEXP_ADJ2 in _ops(h)
    st, _ = _image(h, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
    assert "third-order reverse mode through GAAST_OP_GEXP_ADJ2" in _lib.lib().gaast_expr_last_error().decode()


def test_the_third_child_survives_the_renumbering():
    """the PGA3D Hessian image drops and renumbers nodes: the operand index in input_slot still names the forward operand of the
    GEXP node it belongs to (the bivector input, slot 0)"""
    build, metric = PROGRAMS["gexp(B) X ~gexp(B)"]
    d = H._desc(build, metric, flags=FLAG)
    a2 = _ok(_ok(d, 0), 0)
    adj2 = [a2.nodes[i] for i in range(a2.n_nodes) if a2.nodes[i].opcode == _lib.OP_GEXP_ADJ2]
    assert adj2
    for nd in adj2:
        A = a2.nodes[nd.input_slot]
        assert (A.opcode, A.input_slot, A.minimal_grade_mask) == (_lib.OP_INPUT, 0, 1 << 2)
        assert nd.minimal_grade_mask == 1 << 2


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_without_the_flag_everything_is_as_before(name):
    build, metric = PROGRAMS[name]
    d0, d1 = H._desc(build, metric), H._desc(build, metric, flags=FLAG)
    # the forward image and the first-order images: the same bytes but the flags word
    def same_but_flags(x, y):
        bx, by = bytearray(_serialize(x)), bytearray(_serialize(y))
        diff = [i for i in range(len(bx)) if bx[i] != by[i]] if len(bx) == len(by) else None
        return diff is not None and len(diff) == 1 and (by[diff[0]] ^ bx[diff[0]]) == (FLAG >> 8) and x.flags ^ y.flags == FLAG
    assert same_but_flags(d0, d1)
    for s in H._user_slots(d0):
        assert same_but_flags(_ok(d0, s), _ok(d1, s))
    # second order through the generator: today's status and message
    a = _ok(d0, 0)
    for s in (0, d0.n_inputs):
        st, _ = _image(a, s)
        assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
        assert _lib.lib().gaast_expr_last_error().decode() == "second-order reverse mode through GAAST_OP_GEXP_ADJ is not implemented"
    # a JVP node on the path is refused by name in the same style; off the path it is carried along
    j = _ok(_ok(d1, 0), d1.n_inputs)
    nodes = (_lib.NodeDesc * j.n_nodes)(*[j.nodes[i] for i in range(j.n_nodes)])
    plain = _lib.ProgramDesc()
    C.memmove(C.byref(plain), C.byref(j), C.sizeof(plain))
    plain.nodes, plain.flags = nodes, 0
    st, _ = _image(plain, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
    assert _lib.lib().gaast_expr_last_error().decode() == "second-order reverse mode through GAAST_OP_GEXP_JVP is not implemented"
    st, off = _image(plain, 1)     # X or y: the JVP node does not depend on it
    assert st == 0 and _lib.OP_GEXP_JVP in _ops(off)


def test_second_order_image_round_trips_through_the_wire_format():
    build, metric = PROGRAMS["gexp(B) X ~gexp(B)"]
    d = H._desc(build, metric, flags=FLAG)
    a2 = _ok(_ok(d, 0), 0)
    assert _lib.OP_GEXP_ADJ2 in _ops(a2)
    data = _serialize(a2)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    img = C.c_void_p(_lib.lib().gaast_program_deserialize(buf, len(data)))
    assert img.value
    try:
        b = _lib.lib().gaast_program_image_desc(img).contents
        assert _serialize(b) == data
        assert [(b.nodes[i].opcode, b.nodes[i].input_slot) for i in range(b.n_nodes)] == [(a2.nodes[i].opcode, a2.nodes[i].input_slot) for i in range(a2.n_nodes)]
    finally:
        _lib.lib().gaast_program_image_free(img)


def test_constants():
    assert (_lib.OP_GEXP_JVP, _lib.OP_GEXP_ADJ2, ga.FLAG_GEXP_GRAD2) == (22, 23, 0x4000)
    assert _lib.OP_NAMES[22] == "GeneralExponentialJvp" and _lib.OP_NAMES[23] == "GeneralExponentialAdjoint2"


# ---- the host code under sanitizers, and the lowered tables -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (a stand-alone program, compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("gexp2_asan") / "gexp2_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "gexp2_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")
    for what in ("gexp(x) * y", "gexp(B) X ~gexp(B)", "gexp(~B) X", "raw tables", "raw malformed nodes"):
        assert f"ok  {what}\n" in driver


# tag -> kind -> (operand grades, flipped grades of the operand read, g grades or None, h grades, result grades)
TABLES = {"pga-even": {"jvp": ([0, 2, 4], set(), None, [0, 2, 4], [0, 2, 4]), "adj2": ([0, 2, 4], set(), [0, 2, 4], [0, 2, 4], [0, 2, 4])},
          "pga-part": {"jvp": ([2], {2}, None, [2], [2, 4]), "adj2": ([2], {2}, [0, 2], [2], [2])}}


@pytest.mark.parametrize("kind", ["jvp", "adj2"])
@pytest.mark.parametrize("tag", sorted(TABLES))
def test_lowered_tables_match_numpy(driver, tag, kind):
    """offsets of A, g, h and res, the folded signs of the operand read, wmax, and the coefficients of L, ADJL and ADJR"""
    grades, flip, g_grades, h_grades, res_grades = TABLES[tag][kind]
    n = 4
    S, Cm, wmax = gx.structure(tuple(PGA), tuple(grades))
    N = len(S)
    outs, tab = {}, {}
    for line in driver.splitlines():
        f = line.split()
        if len(f) > 3 and f[0] == "G2OUT" and f[1] == tag and f[2] == kind:
            outs[int(f[4])] = (int(f[3]), int(f[5])) + tuple(int(v) for v in f[6:11]) + (float(f[11]),)
        elif len(f) > 3 and f[0] == "G2TAB" and f[1] == tag and f[2] == kind:
            tab[int(f[3]), int(f[4])] = tuple(float(v) for v in f[5:8])
    where = lambda gr: {b: i for i, b in enumerate(inu.row_blades(n, tuple(gr)))}
    a_w, h_w, r_w = where(grades), where(h_grades), where(res_grades)
    g_w = where(g_grades) if g_grades is not None else None
    assert sorted(outs) == list(range(N)) and len(tab) == N * N
    for j in range(N):
        Nn, blade, a_off, res_off, g_off, h_off, neg, w = outs[j]
        assert (Nn, blade, w) == (N, S[j], wmax)
        assert a_off == a_w.get(blade, -1) and h_off == h_w.get(blade, -1) and res_off == r_w.get(blade, -1)
        assert g_off == (g_w.get(blade, -1) if g_w is not None else -2)
        assert neg == (1 if inu.grade(blade) in flip and blade in a_w else 0)
    for a in range(N):
        for b in range(N):
            cf, cl, cr = tab[a, b]
            assert cf == Cm[a, b] and cl == cr == Cm[a ^ b, b], (a, b)
