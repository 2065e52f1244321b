"""The general multivector logarithm (GAAST_OP_GLOG / GAAST_OP_GLOG_ADJ) on the host: grade inference, the phase-3 restriction, the
wire format, reverse mode, the lowered Step::GLOG / Step::GLOG_ADJ tables, the Pade table of the kernels' header, and the numpy
restatement of the algorithm (glog_numpy.py) against a numpy.longdouble reference and mpmath's logm.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined (tests/cpp/glog_sanitize_driver.cpp) and
run once: it must end clean, and the tables it prints from the lowered plans are what the tests below compare with numpy.

Accuracy of the restatement.  Inputs (glog_numpy.operands): default_rng(20261021), A = gexp(B) computed in float64 with B = U(-1, 1)
on the operand's grades normalised to sum |B| in {0.1, 1, 2.5} (below pi: B is the principal logarithm), items with a dominant positive
scalar, and the first kind scaled by 37.5 and by 0.01 (up to 5 roots); all rounded to float32, so both dtypes see the same values.
The restatement in the program's dtype is measured against the longdouble reference (theta = 1/16, 12 nodes) by
||Y - ref||_inf / (N eps max(1, sum |ref_i|)): its worst is glog_numpy.FWD_SCALE, asserted here to cover what this run measures (the
GPU is allowed 4 x that).  The reverse mode in the program's dtype is compared with the longdouble reverse of the reference in units
of N eps max(1, sum |ref_i|) ||J^T||_inf ||g||_inf: its worst is glog_numpy.GRAD_SCALE, asserted likewise."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import glog_numpy as gl
import gsqrt_numpy as gs
import inverse_numpy as inu
from helpers import plan_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
R33 = [1.0] * 3 + [-1.0] * 3
SEED = 20261021
# name -> (metric, operand grades (every grade of the blade set), N, items per kind)
ACCURACY_CASES = {
    "R1": ([1.0], [0, 1], 2, 8), "R2": ([1.0] * 2, [0, 1, 2], 4, 8), "R3-even": ([1.0] * 3, [0, 2], 4, 8), "R3": ([1.0] * 3, [0, 1, 2, 3], 8, 6),
    "PGA3D-even": (PGA, [0, 2, 4], 8, 6), "PGA3D": (PGA, [0, 1, 2, 3, 4], 16, 4), "CGA-even": (CGA, [0, 2, 4], 16, 4),
    "CGA": (CGA, [0, 1, 2, 3, 4, 5], 32, 2), "R33-even": (R33, [0, 2, 4, 6], 32, 2), "R33": (R33, list(range(7)), 64, 1),
    "R7-even": ([1.0] * 7, [0, 2, 4, 6], 64, 1),
}
LOGM_CASES = ("R1", "R3-even", "R3", "PGA3D-even", "PGA3D", "CGA-even")      # N <= 16
_GRAD_REF = {}
GLOG_OPS = (_lib.OP_GLOG, _lib.OP_GLOG_ADJ)      # (the module is about these two: without them it does not load)


def _in(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _mask(grades):
    return sum(1 << k for k in grades)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("glog_asan") / "glog_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "glog_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")


# ---- phases 2 and 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grades", [(3, [0, 2]), (4, [2]), (4, [0, 2, 4]), (5, [2]), (7, [2, 4]), (8, [2]), (3, [0]), (1, [0])])
def test_even_operand_gives_the_even_grades(n, grades):
    """GEXP's grades, by the gs_inverse rule; a scalar operand too: there is no scalar lowering"""
    spec = _in(0, grades, n).glog().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_GLOG
    assert root.maximal_grade_mask == _mask(range(0, n + 1, 2)) == root.minimal_grade_mask
    same = _in(0, grades, n).gexp().specialize(ga.MetricAlgebra([1.0] * n))
    assert same.nodes()[same.root_id()].maximal_grade_mask == root.maximal_grade_mask


@pytest.mark.parametrize("n,grades", [(1, [0, 1]), (3, [1]), (4, [0, 1, 2, 3, 4]), (4, [1, 3]), (5, [2, 3]), (7, [0, 1]), (9, [1])])
def test_mixed_operand_gives_every_grade(n, grades):
    spec = _in(0, grades, n).glog().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_GLOG
    assert root.maximal_grade_mask == _mask(range(n + 1)) == root.minimal_grade_mask


def test_phase_3_wants_the_operand_in_full_whatever_is_wanted_of_the_result():
    a, b = _in(0, [0, 1, 2, 3, 4], 4), _in(1, [0, 1, 2, 3, 4], 4)
    spec = ((a + b).glog()).g(2).specialize(ga.MetricAlgebra(PGA))
    nodes = spec.nodes()
    gq = [nd for nd in nodes if nd.opcode == _lib.OP_GLOG]
    assert len(gq) == 1
    assert gq[0].maximal_grade_mask == 0x1f and gq[0].minimal_grade_mask == 1 << 2   # produces only the wanted grade
    child = nodes[gq[0].child0]
    assert child.opcode == _lib.OP_ADD and child.minimal_grade_mask == child.maximal_grade_mask == 0x1f
    for leaf in (nodes[child.child0], nodes[child.child1]):
        assert leaf.minimal_grade_mask == leaf.maximal_grade_mask


def test_log_is_what_it_was_and_the_opcodes_are_20_and_21():
    """log() keeps its opcode and its flag; glog() is a node of its own that needs none"""
    closed = _in(0, [0, 2], 3).log().specialize(ga.MetricAlgebra([1.0] * 3))
    ops = [nd.opcode for nd in closed.nodes()]
    assert _lib.OP_GLOG not in ops and ops.count(_lib.OP_LOG) == 1
    with pytest.raises(_lib.GaastError):      # the closed form is not to be had without its flag
        closed.program()
    ops = [nd.opcode for nd in _in(0, [0, 2], 3).glog().specialize(ga.MetricAlgebra([1.0] * 3)).nodes()]
    assert _lib.OP_LOG not in ops and ops.count(_lib.OP_GLOG) == 1
    assert GLOG_OPS == (20, 21) and _lib.OP_NAMES[20] == "GeneralLogarithm" and _lib.OP_NAMES[21] == "GeneralLogarithmAdjoint"
    assert (_lib.OP_GSQRT, _lib.OP_GSQRT_ADJ, _lib.OP_GEXP, _lib.OP_GEXP_ADJ, _lib.OP_INV) == (18, 19, 16, 17, 15)
    header = open(os.path.join(ROOT, "include", "gaast_hip.h")).read()
    assert re.search(r"GAAST_OP_GLOG = 20,", header) and re.search(r"GAAST_OP_GLOG_ADJ = 21\b", header)


# ---- wire format ------------------------------------------------------------------------------------------------------------------
def _round_trip(desc, data, opcode):
    L = _lib.lib()
    img = ga.ast.ProgramImage(data)
    back = img.desc
    assert back.n_nodes == desc.n_nodes and back.root == desc.root
    ops = [back.nodes[i].opcode for i in range(back.n_nodes)]
    assert ops == [desc.nodes[i].opcode for i in range(desc.n_nodes)] and ops.count(opcode) == 1
    for i in range(desc.n_nodes):
        assert back.nodes[i].minimal_grade_mask == desc.nodes[i].minimal_grade_mask
        assert back.nodes[i].child0 == desc.nodes[i].child0 and back.nodes[i].child1 == desc.nodes[i].child1
    need = L.gaast_program_serialize(C.byref(back), None, 0)
    buf = (C.c_ubyte * need)()
    assert L.gaast_program_serialize(C.byref(back), buf, need) == need
    assert bytes(buf) == data
    for cut in range(0, len(data), len(data) // 7 + 1):
        with pytest.raises(_lib.GaastError):
            ga.ast.ProgramImage(data[:cut])


def test_wire_round_trip_of_a_program_and_of_its_vjp():
    L = _lib.lib()
    spec = ((_in(0, [0, 2], 4) + _in(1, [0, 2], 4)).glog() * _in(2, [1], 4)).specialize(ga.MetricAlgebra(PGA))
    desc = spec.program_desc()
    _round_trip(desc, spec.serialize(), _lib.OP_GLOG)
    out = C.c_void_p()
    assert L.gaast_program_vjp(C.byref(desc), 0, C.byref(out)) == 0
    d = C.cast(L.gaast_program_image_desc(out), C.POINTER(type(desc))).contents
    need = L.gaast_program_serialize(C.byref(d), None, 0)
    buf = (C.c_ubyte * need)()
    assert L.gaast_program_serialize(C.byref(d), buf, need) == need
    _round_trip(d, bytes(buf), _lib.OP_GLOG_ADJ)
    L.gaast_program_image_free(out)


# ---- reverse mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mask", [("full1", 0x3), ("full3", 0xf), ("even3", 0x5), ("pga-biv", 0x4), ("pga-full", 0x1f), ("cga-biv", 0x4),
                                      ("odd-full", 0xf), ("pga-13", 0xa)])
def test_vjp_program_of_glog_x_is_one_adjoint_node_over_g_and_x(driver, tag, mask):
    """two inputs and one GLOG_ADJ node: child0 the cotangent (slot 1), child1 the operand (slot 0), the node's mask the operand's;
    the forward is not re-evaluated by a node of its own"""
    ops = [l.split() for l in driver.splitlines() if l.startswith(f"VJPOPS {tag} ")]
    adj = [l.split() for l in driver.splitlines() if l.startswith(f"VJPADJ {tag} ")]
    assert [o[2:] for o in ops] == [["0", "3", "1", "0"]]
    assert [a[2:] for a in adj] == [["0", str(_lib.OP_INPUT), "1", str(_lib.OP_INPUT), "0", str(mask)]]


def test_vjp_through_the_c_abi_needs_no_flag():
    L = _lib.lib()
    spec = _in(0, [0, 2], 4).glog().specialize(ga.MetricAlgebra(PGA))
    desc = spec.program_desc()
    assert desc.flags == 0
    out = C.c_void_p()
    assert L.gaast_program_vjp(C.byref(desc), 0, C.byref(out)) == 0
    d = C.cast(L.gaast_program_image_desc(out), C.POINTER(type(desc))).contents
    ops = [d.nodes[i].opcode for i in range(d.n_nodes)]
    assert ops.count(_lib.OP_GLOG_ADJ) == 1 and _lib.OP_GLOG not in ops and d.n_nodes == 3 and d.flags == 0
    L.gaast_program_image_free(out)


# ---- the lowered steps ------------------------------------------------------------------------------------------------------------
CASES = {   # tag -> (metric, operand grades, produced grades or None for all)
    "full1": ([1.0], [0, 1], None), "full2": ([1.0] * 2, [0, 1, 2], None), "full3": ([1.0] * 3, [0, 1, 2, 3], None),
    "even2": ([1.0] * 2, [0, 2], None), "even3": ([1.0] * 3, [0, 2], None),
    "pga-biv": (PGA, [2], None), "pga-full": (PGA, [0, 1, 2, 3, 4], None), "cga-biv": (CGA, [2], None),
    "odd-full": ([2.0, -0.5, 1.0], [0, 1, 2, 3], None), "pga-13": (PGA, [1, 3], None), "pga-g2": (PGA, [0, 1, 2, 3, 4], [2]),
    "pga-rev": (PGA, [2], None),
}


def _tables(out, tag, prefix):
    outs, tab, adj = {}, {}, {}
    for line in out.splitlines():
        f = line.split()
        if len(f) < 2 or f[1] != tag:
            continue
        if f[0] == prefix + "OUT":
            outs.setdefault(int(f[3]), []).append((int(f[2]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), float(f[8])))
        elif f[0] == prefix + "TAB":
            tab.setdefault((int(f[2]), int(f[3])), []).append(float(f[4]))
        elif f[0] == "ADJTAB":
            adj.setdefault((int(f[2]), int(f[3])), []).append((float(f[4]), float(f[5]), int(f[6]), int(f[7])))
    return outs, tab, adj


@pytest.mark.parametrize("tag", sorted(CASES))
def test_lowered_tables_match_numpy(driver, tag):
    """The forward step's blade list, offsets, wmax and N x N coefficients, and the adjoint step's two coefficient tables, cotangent and
    result offsets, equal numpy's entry for entry (the forward program's step is printed first, then the VJP program's); the two
    single transposes the adjoint kernel builds from them are the transposes of glog_numpy's R_M and L_M"""
    metric, grades, produced = CASES[tag]
    n = len(metric)
    outs, tab, adj = _tables(driver, tag, "GLOG")
    S, Cm, wmax = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    flip = {2, 3} if tag == "pga-rev" else set()   # glog(~B): the reverse of a bound input is folded into the operand read
    where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(grades)))}
    res_grades = inu.result_grades(n, tuple(grades)) if produced is None else produced
    res_where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(res_grades)))}
    assert sorted(outs) == list(range(N))
    for j in range(N):
        Nn, blade, a_off, res_off, neg, w = outs[j][0]
        assert (Nn, blade, w) == (N, S[j], wmax)
        assert neg == (1 if inu.grade(blade) in flip and blade in where else 0)
        assert a_off == where.get(blade, -1) and res_off == res_where.get(blade, -1)
    for r in range(N):
        for j in range(N):
            assert tab[(r, j)][0] == Cm[r, j], (r, j)
    g_where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(res_grades)))}
    assert len(adj) == N * N
    M = np.random.default_rng(SEED).uniform(0.5, 1.5, (1, N))
    RT, LT = gl.right_matrix(Cm, M)[0].T, gs.left_matrix(Cm, M)[0].T
    for a in range(N):
        for b in range(N):
            cl, cr, g_off, res_off = adj[(a, b)][0]
            assert cl == cr == Cm[a ^ b, b], (a, b)
            assert g_off == g_where.get(S[a], -1)
            assert res_off == where.get(S[a], -1)     # the cotangent lands on the operand's own components
    # the rows the kernel builds: at column c xor t, ADJL's coefficient of (c, t) times M[t] is R_M^T, ADJR's of (t, c) read at row c is L_M^T
    for c in range(N):
        for t in range(N):
            assert adj[(c, t)][0][0] * M[0, t] == RT[c, c ^ t], (c, t)
            assert adj[(t, c)][0][1] * M[0, t] == LT[c, c ^ t], (c, t)


@pytest.mark.parametrize("tag", ["pga-full", "cga-biv", "odd-full"])
def test_the_inverse_gexp_and_gsqrt_tables_are_unchanged(driver, tag):
    """the driver also lowers inv(x), gexp(x) and gsqrt(x) of the same operands and prints their steps ("OLD..." lines): blade list,
    offsets, sign words and weights equal numpy's entry for entry"""
    metric, grades, _ = CASES[tag]
    S, Cm, wmax = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    where = {b: i for i, b in enumerate(inu.row_blades(len(metric), tuple(grades)))}
    res_where = {b: i for i, b in enumerate(inu.row_blades(len(metric), tuple(inu.result_grades(len(metric), tuple(grades)))))}
    for kind in ("INV", "GEXP", "GSQRT"):
        outs = {int(f[3]): f for f in (l.split() for l in driver.splitlines()) if len(f) > 3 and f[0] == "OLDOUT" and f[1] == kind and f[2] == tag}
        tab = {(int(f[3]), int(f[4])): float(f[5]) for f in (l.split() for l in driver.splitlines()) if len(f) > 5 and f[0] == "OLDTAB" and f[1] == kind and f[2] == tag}
        assert sorted(outs) == list(range(N)) and len(tab) == N * N
        for j in range(N):
            _, _, _, _, blade, a_off, res_off, a_neg = outs[j]
            assert (int(blade), int(a_off), int(res_off), int(a_neg)) == (S[j], where.get(S[j], -1), res_where[S[j]], 0)
        for r in range(N):
            for j in range(N):
                assert tab[(r, j)] == Cm[r, j], (kind, r, j)


def test_unsupported_sizes_are_refused_only_by_the_device_plan(driver):
    """N > 64 (n = 7 mixed: 128 blades, n = 8) and N = 1 (a scalar at n = 1 or n = 0: no scalar lowering) specialise and lower without
    an error, but the plan names what the back end cannot do (-> GAAST_ERR_UNIMPLEMENTED at gaast_hip_program_create); the driver asserts
    plan.unsupported for each of them and its emptiness for the supported sizes"""
    for what in ("glog(full) n=7", "glog(full) n=8", "glog(even) n=8", "glog(even) n=1", "glog(scalar) n=0", "glog(even) n=7", "glog(full) n=6",
                 "glog(scalar) n=3", "raw GLOG node over a scalar", "raw adjoint nodes"):
        assert f"ok  {what}\n" in driver
    for n, grades in ((7, [0, 1]), (7, list(range(8))), (8, [2]), (1, [0]), (0, [0])):
        _in(0, grades, n).glog().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed


# ---- the Pade table ---------------------------------------------------------------------------------------------------------------
def _header_table():
    text = open(os.path.join(ROOT, "gaast_amd", "csrc", "common", "glog_pade.hpp")).read()
    arr = lambda name: np.array([float(x) for x in re.search(name + r"\[kGlogPadeTerms\] = \{([^}]*)\}", text).group(1).replace("\n", " ").split(",") if x.strip()])
    terms = int(re.search(r"kGlogPadeTerms = (\d+);", text).group(1))
    theta = float(re.search(r"kGlogTheta = ([0-9.]+);", text).group(1))
    roots = int(re.search(r"kGlogMaxRoots = (\d+);", text).group(1))
    return terms, arr("kGlogPadeNode"), arr("kGlogPadeWeight"), theta, roots


def test_header_pade_table_is_gauss_legendre_on_the_unit_interval():
    """the literals of common/glog_pade.hpp against numpy.polynomial.legendre.leggauss(7) mapped to [0, 1], to 1 ulp; and against the
    exact nodes and weights (mpmath, 40 digits), from which leggauss itself lies up to 34 ulp: to 64 ulp"""
    terms, node, weight, theta, roots = _header_table()
    assert (terms, theta, roots) == (gl.TERMS, gl.THETA, gl.MAX_ROOTS) == (7, 0.25, 16)
    beta, alpha = gl.pade_table(7)
    assert node.shape == weight.shape == (7,)
    assert np.all(np.abs(node - beta) <= np.spacing(beta)) and np.all(np.abs(weight - alpha) <= np.spacing(alpha))
    xb, xa = gl.pade_table_longdouble(7)
    assert np.all(np.abs(node - xb.astype(np.float64)) <= 64 * np.spacing(beta)) and np.all(np.abs(weight - xa.astype(np.float64)) <= 64 * np.spacing(alpha))
    assert abs(weight.sum() - 1.0) <= 2.0 ** -52
    # the approximant itself at the edge of its range: |r_7(-1/4) - log(3/4)| is far below float64 eps (Kenney and Laub's bound)
    r7 = float(np.sum(xa * np.longdouble(-0.25) / (1 + xb * np.longdouble(-0.25))))
    assert abs(r7 - np.log(0.75)) <= 1e-16


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_inputs():
    """name -> (A over S, kind per item, longdouble logarithm): drawn and referenced once for the module"""
    out = {}
    for name, (metric, grades, N, items) in ACCURACY_CASES.items():
        A, kind = gl.operands(metric, grades, items, np.random.default_rng(SEED))
        out[name] = (A, kind, gl.log_reference(metric, grades, A))
    return out


def test_longdouble_reference_agrees_with_mpmath_logm(accuracy_inputs):
    """on one item of every kind of the cases up to N = 16: mpmath.logm of L_A at 40 digits, first column"""
    pytest.importorskip("mpmath")
    for name in LOGM_CASES:
        metric, grades, N, items = ACCURACY_CASES[name]
        A, kind, ref = accuracy_inputs[name]
        lead = [k * items for k in range(gl.KINDS)] if N <= 8 else [2 * items, 4 * items]
        want = gl.logm_reference(metric, grades, A[lead])
        assert np.abs(ref[lead].astype(np.float64) - want).max() <= 4 * 2.0 ** -52 * max(1.0, np.abs(want).max()), name


def test_restatement_agrees_with_mpmath_logm(accuracy_inputs):
    """the float64 restatement itself against logm, within its scale"""
    pytest.importorskip("mpmath")
    for name in LOGM_CASES:
        metric, grades, N, items = ACCURACY_CASES[name]
        A, kind, ref = accuracy_inputs[name]
        lead = [0, 2 * items, 4 * items] if N <= 8 else [2 * items]
        want = gl.logm_reference(metric, grades, A[lead])
        Y, s, bad = gl.forward(metric, grades, A[lead], np.float64)
        assert not bad.any()
        err = gl.forward_error(Y, want, gl.EPS[np.dtype(np.float64)])
        assert err.max() <= gl.FWD_SCALE[np.dtype(np.float64)] + 1.0 / N, (name, err.max())      # (+ the reference's own rounding to float64)


def test_the_logarithm_of_gexp_b_is_b():
    rng = np.random.default_rng(SEED + 3)
    for metric, grades in ((PGA, [2]), (CGA, [2]), ([1.0] * 3, [0, 1, 2, 3])):
        B = gx.random_operand(metric, grades, 4, 2.5, rng, np.float64)
        A = gx.forward(metric, grades, B, np.longdouble, s_dtype=np.float64, degree=24)[0]
        Y = gl.log_reference(metric, grades, A)
        assert np.abs(Y - B).max() <= 2e-17 * max(1.0, np.abs(B).sum(axis=1).max()) * A.shape[1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ACCURACY_CASES))
def test_restatement_forward_error_defines_the_scale(accuracy_inputs, name, dtype):
    metric, grades, N, items = ACCURACY_CASES[name]
    dt = np.dtype(dtype)
    A, kind, ref = accuracy_inputs[name]
    Y, s, bad = gl.forward(metric, grades, A, dtype)
    assert not bad.any() and Y.dtype == dt                 # no domain error on any input
    err = gl.forward_error(Y, ref, gl.EPS[dt])
    for k in range(gl.KINDS):
        print(f"FORWARD {name} {dt.name} kind {k}: roots {s[kind == k].min()}..{s[kind == k].max()} error {err[kind == k].max():.3f} N eps max(1, sum |log A|)")
    assert s.max() <= 6
    assert err.max() <= gl.FWD_SCALE[dt], (name, err.max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ACCURACY_CASES))
def test_restatement_gradient_error_defines_the_scale(accuracy_inputs, name, dtype):
    metric, grades, N, items = ACCURACY_CASES[name]
    dt = np.dtype(dtype)
    A, kind, ref = accuracy_inputs[name]
    if name not in _GRAD_REF:      # the cotangent, the longdouble reverse and ||J^T||_inf: once per case
        g = np.random.default_rng(SEED + 1).uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
        _GRAD_REF[name] = (g, gl.reverse_reference(metric, grades, A, g), gl.jacobian_norm(metric, grades, A))
    g, want, jn = _GRAD_REF[name]
    got = gl.reverse(metric, grades, A, g, dtype)
    worst = gl.gradient_error(got, want, gl.EPS[dt], ref, jn, g).max()
    print(f"GRADIENT {name} {dt.name}: worst {worst:.3f} N eps max(1, sum |log A|) |J^T| |g|, |J^T| up to {jn.max():.1f}")
    assert worst <= gl.GRAD_SCALE[dt], (name, worst)


def test_reverse_is_the_gradient():
    """central differences of the float64 forward (h = 1e-6) against the float64 reverse, and of the longdouble reference"""
    rng = np.random.default_rng(SEED + 2)
    for metric, grades in ((PGA, [0, 2, 4]), (PGA, [0, 1, 2, 3, 4]), ([1.0] * 3, [0, 1, 2, 3])):
        A, _ = gl.operands(metric, grades, 2, rng, np.float64)
        g = rng.uniform(-1, 1, A.shape)
        v = rng.uniform(-1, 1, A.shape) * np.abs(A).max(axis=1, keepdims=True)      # (relative steps: the items span 0.01 ... 37.5)
        da = gl.reverse(metric, grades, A, g)
        for f in (lambda Z: gl.forward(metric, grades, Z, np.float64)[0], lambda Z: gl.log_reference(metric, grades, Z).astype(np.float64)):
            jv = (f(A + 1e-6 * v) - f(A - 1e-6 * v)) / 2e-6
            lhs, rhs, scale = (g * jv).sum(axis=1), (da * v).sum(axis=1), (np.abs(g) * np.abs(jv)).sum(axis=1)
            assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


def test_domain_errors_of_the_restatement():
    """-1, a vector (eigenvalues +-1), 0, a NaN and an infinity are domain errors, and so are PGA's ideal element e0 and the unipotent
    1 + 1e5 e01 (each root only halves its nilpotent part: more than 16 roots); 4, 1 and 1 + 1000 e01 are not"""
    A = np.array([[-1.0, 0, 0, 0], [0, 1.0, 0, 0], [0.0, 0, 0, 0], [4.0, 0, 0, 0], [1.0, np.nan, 0, 0], [np.inf, 0, 0, 0], [1.0, 0, 0, 0]])
    for dtype in (np.float32, np.float64):
        Y, s, bad = gl.forward([1.0, 1.0], [0, 1, 2], A, dtype)
        assert list(bad) == [True, True, True, False, True, True, False] and np.isnan(Y[bad]).all()
        assert np.abs(Y[3] - [np.log(4.0), 0, 0, 0]).max() <= 8 * gl.EPS[np.dtype(dtype)] * 4 * gl.FWD_SCALE[np.dtype(dtype)]
        assert np.array_equal(Y[6], [0.0, 0, 0, 0]) and s[6] == 0
        d = gl.reverse([1.0, 1.0], [0, 1, 2], A, np.ones_like(A), dtype)
        assert np.isnan(d[bad]).all() and np.isfinite(d[~bad]).all()
        e0 = np.zeros((1, 16))
        e0[0, 1] = 1.0                                     # e0 alone, over every blade of PGA3D
        assert gl.forward(PGA, [0, 1, 2, 3, 4], e0, dtype)[2].all()
        T = np.zeros((3, 8))                               # the even blades of PGA3D: index 1 is e01
        T[0, 1] = 1.0                                      # e01 alone
        T[1, 0], T[1, 1] = 1.0, 1e5                        # 1 + 1e5 e01
        T[2, 0], T[2, 1] = 1.0, 1000.0                     # 1 + 1000 e01
        Y, s, bad = gl.forward(PGA, [0, 2, 4], T, dtype)
        assert list(bad) == [True, True, False]
        want = np.zeros(8)
        want[1] = 1000.0
        assert np.abs(Y[2] - want).max() <= 1000.0 * 8 * gl.EPS[np.dtype(dtype)] * gl.FWD_SCALE[np.dtype(dtype)] and s[2] >= 10
