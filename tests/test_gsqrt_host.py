"""The general multivector square root (GAAST_OP_GSQRT / GAAST_OP_GSQRT_ADJ) on the host: grade inference, the phase-3 restriction, the
scalar form, the wire format, reverse mode, the lowered Step::GSQRT / Step::GSQRT_ADJ tables, and the numpy restatement of the
algorithm (gsqrt_numpy.py) against a numpy.longdouble and an mpmath reference.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined (tests/cpp/gsqrt_sanitize_driver.cpp) and
run once: it must end clean, and the tables it prints from the lowered plans are what the tests below compare with numpy.

Accuracy of the restatement.  Inputs (gsqrt_numpy.operands): default_rng(20261021), A = gexp(B) computed in float64 with B = U(-1, 1)
on the operand's grades normalised to sum |B| in {0.1, 1, 2.5} (below pi: gexp(B / 2) is the principal root), plus items with a dominant
positive scalar; all rounded to float32, so both dtypes see the same values.  The restatement in the program's dtype is measured by
the residual ||X X - A||_inf / (||L_X||_inf ||X||_inf) and by the error against the longdouble root ||X - ref||_inf / ||ref||_inf, both
in units of N eps; the worst of the two is the scale of the GPU's forward bound (gsqrt_numpy.FWD_SCALE, asserted here to cover what
this run measures; the GPU is allowed 4 x that, its sums being contracted into fused multiply-adds).  The adjoint solve in the
program's dtype is compared with the longdouble solve on the longdouble root in units of N eps kappa_inf(L_X + R_X) ||a||_inf: its worst
is gsqrt_numpy.GRAD_SCALE, asserted likewise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
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
    "CGA": (CGA, [0, 1, 2, 3, 4, 5], 32, 3), "R33-even": (R33, [0, 2, 4, 6], 32, 3), "R33": (R33, list(range(7)), 64, 2),
    "R7-even": ([1.0] * 7, [0, 2, 4, 6], 64, 2),
}


def _in(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _mask(grades):
    return sum(1 << k for k in grades)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("gsqrt_asan") / "gsqrt_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "gsqrt_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")


# ---- phases 2 and 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grades", [(3, [0, 2]), (4, [2]), (4, [0, 2, 4]), (5, [2]), (7, [2, 4]), (8, [2])])
def test_even_operand_gives_the_even_grades(n, grades):
    spec = _in(0, grades, n).gsqrt().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_GSQRT
    assert root.maximal_grade_mask == _mask(range(0, n + 1, 2)) == root.minimal_grade_mask


@pytest.mark.parametrize("n,grades", [(1, [0, 1]), (3, [1]), (4, [0, 1, 2, 3, 4]), (4, [1, 3]), (5, [2, 3]), (7, [0, 1]), (9, [1])])
def test_mixed_operand_gives_every_grade(n, grades):
    spec = _in(0, grades, n).gsqrt().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_GSQRT
    assert root.maximal_grade_mask == _mask(range(n + 1)) == root.minimal_grade_mask


def test_phase_3_wants_the_operand_in_full_whatever_is_wanted_of_the_result():
    a, b = _in(0, [0, 1, 2, 3, 4], 4), _in(1, [0, 1, 2, 3, 4], 4)
    spec = ((a + b).gsqrt()).g(2).specialize(ga.MetricAlgebra(PGA))
    nodes = spec.nodes()
    gq = [nd for nd in nodes if nd.opcode == _lib.OP_GSQRT]
    assert len(gq) == 1
    assert gq[0].maximal_grade_mask == 0x1f and gq[0].minimal_grade_mask == 1 << 2   # produces only the wanted grade
    child = nodes[gq[0].child0]
    assert child.opcode == _lib.OP_ADD and child.minimal_grade_mask == child.maximal_grade_mask == 0x1f
    for leaf in (nodes[child.child0], nodes[child.child1]):
        assert leaf.minimal_grade_mask == leaf.maximal_grade_mask


@pytest.mark.parametrize("n", [0, 1, 3])
def test_a_scalar_operand_is_the_scalar_square_root(n):
    """as inv() of a scalar is sinv(): no GSQRT node, one ScalarSqrt"""
    ops = [nd.opcode for nd in _in(0, [0], n).gsqrt().specialize(ga.MetricAlgebra([1.0] * n)).nodes()]
    assert _lib.OP_GSQRT not in ops and ops.count(_lib.OP_SSQRT) == 1


def test_sqrt_is_what_it_was():
    """sqrt() keeps lowering through pow / exp / log; gsqrt() is a node of its own"""
    ops = [nd.opcode for nd in _in(0, [2], 3).norm_sq().sqrt().specialize(ga.MetricAlgebra([1.0] * 3)).nodes()]
    assert _lib.OP_GSQRT not in ops and ops.count(_lib.OP_SSQRT) == 1
    with pytest.raises(_lib.GaastError):      # the closed form of a k-vector through pow / exp / log is not to be had without its flag
        _in(0, [2], 3).sqrt().specialize(ga.MetricAlgebra([1.0] * 3)).program()
    assert (_lib.OP_GSQRT, _lib.OP_GSQRT_ADJ) == (18, 19) and _lib.OP_NAMES[18] == "GeneralSqrt" and _lib.OP_NAMES[19] == "GeneralSqrtAdjoint"
    assert (_lib.OP_GEXP, _lib.OP_GEXP_ADJ, _lib.OP_INV) == (16, 17, 15)


# ---- wire format ------------------------------------------------------------------------------------------------------------------
def test_wire_round_trip():
    L = _lib.lib()
    spec = ((_in(0, [0, 2], 4) + _in(1, [0, 2], 4)).gsqrt() * _in(2, [1], 4)).specialize(ga.MetricAlgebra(PGA))
    desc = spec.program_desc()
    data = spec.serialize()
    img = ga.ast.ProgramImage(data)
    back = img.desc
    assert back.n_nodes == desc.n_nodes and back.root == desc.root
    ops = [back.nodes[i].opcode for i in range(back.n_nodes)]
    assert ops == [desc.nodes[i].opcode for i in range(desc.n_nodes)] and ops.count(_lib.OP_GSQRT) == 1
    for i in range(desc.n_nodes):
        assert back.nodes[i].minimal_grade_mask == desc.nodes[i].minimal_grade_mask and back.nodes[i].child0 == desc.nodes[i].child0
    need = L.gaast_program_serialize(C.byref(back), None, 0)
    buf = (C.c_ubyte * need)()
    assert L.gaast_program_serialize(C.byref(back), buf, need) == need
    assert bytes(buf) == data
    for cut in range(0, len(data), len(data) // 7 + 1):
        with pytest.raises(_lib.GaastError):
            ga.ast.ProgramImage(data[:cut])


# ---- reverse mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mask", [("full1", 0x3), ("full3", 0xf), ("even3", 0x5), ("pga-biv", 0x4), ("pga-full", 0x1f), ("cga-biv", 0x4),
                                      ("odd-full", 0xf), ("pga-13", 0xa)])
def test_vjp_program_of_gsqrt_x_is_one_adjoint_node_over_g_and_x(driver, tag, mask):
    """two inputs and one GSQRT_ADJ node: child0 the cotangent (slot 1), child1 the operand (slot 0), the node's mask the operand's;
    the forward is not re-evaluated by a node of its own"""
    ops = [l.split() for l in driver.splitlines() if l.startswith(f"VJPOPS {tag} ")]
    adj = [l.split() for l in driver.splitlines() if l.startswith(f"VJPADJ {tag} ")]
    assert [o[2:] for o in ops] == [["0", "3", "1", "0"]]
    assert [a[2:] for a in adj] == [["0", str(_lib.OP_INPUT), "1", str(_lib.OP_INPUT), "0", str(mask)]]


def test_vjp_through_the_c_abi_needs_no_flag():
    L = _lib.lib()
    spec = _in(0, [0, 2], 4).gsqrt().specialize(ga.MetricAlgebra(PGA))
    desc = spec.program_desc()
    out = C.c_void_p()
    assert L.gaast_program_vjp(C.byref(desc), 0, C.byref(out)) == 0
    d = C.cast(L.gaast_program_image_desc(out), C.POINTER(type(desc))).contents
    ops = [d.nodes[i].opcode for i in range(d.n_nodes)]
    assert ops.count(_lib.OP_GSQRT_ADJ) == 1 and _lib.OP_GSQRT not in ops and d.n_nodes == 3
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
    """The forward step's blade list, offsets and N x N coefficients, and the adjoint step's two coefficient tables, cotangent and
    result offsets, equal numpy's entry for entry (the forward program's step is printed first, then the VJP program's)"""
    metric, grades, produced = CASES[tag]
    n = len(metric)
    outs, tab, adj = _tables(driver, tag, "GSQRT")
    S, Cm, wmax = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    flip = {2, 3} if tag == "pga-rev" else set()   # gsqrt(~B): the reverse of a bound input is folded into the operand read
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
    # the adjoint step of the VJP program with respect to slot 0: the coefficient of (a, b) in both operators is that of L[a xor b][b]
    g_where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(res_grades)))}
    assert len(adj) == N * N
    T = gs.transposed_sum_matrix(Cm, np.ones((1, N)))[0]
    for a in range(N):
        for b in range(N):
            cl, cr, g_off, res_off = adj[(a, b)][0]
            assert cl == cr == Cm[a ^ b, b], (a, b)
            assert g_off == g_where.get(S[a], -1)
            assert res_off == where.get(S[a], -1)     # the cotangent lands on the operand's own components
    # ... and the row the kernel builds from them, T[c][c xor t] = ADJL's coefficient of (c, t) + ADJR's of (t, c) read at row c
    for c in range(N):
        for t in range(N):
            assert adj[(c, t)][0][0] + adj[(t, c)][0][1] == T[c, c ^ t], (c, t)


@pytest.mark.parametrize("tag", ["pga-full", "cga-biv", "odd-full"])
def test_the_inverse_and_gexp_tables_are_unchanged(driver, tag):
    """the driver also lowers inv(x) and gexp(x) of the same operands and prints their steps ("OLD..." lines): blade list, offsets, sign
    words and weights equal numpy's entry for entry, as before this step kind shared their table builder"""
    metric, grades, _ = CASES[tag]
    S, Cm, wmax = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    where = {b: i for i, b in enumerate(inu.row_blades(len(metric), tuple(grades)))}
    res_where = {b: i for i, b in enumerate(inu.row_blades(len(metric), tuple(inu.result_grades(len(metric), tuple(grades)))))}
    for kind in ("INV", "GEXP"):
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
    """N > 64 (n = 7 mixed: 128 blades, n = 8) and N = 1 (a GSQRT node over a scalar at n = 1, raw ABI) specialise and lower without an
    error, but the plan names what the back end cannot do (-> GAAST_ERR_UNIMPLEMENTED at gaast_hip_program_create); the driver asserts
    plan.unsupported for each of them and its emptiness for the supported sizes"""
    for what in ("gsqrt(full) n=7", "gsqrt(full) n=8", "gsqrt(even) n=8", "gsqrt(even) n=1", "gsqrt(scalar) n=0", "gsqrt(even) n=7", "gsqrt(full) n=6",
                 "gsqrt(scalar) n=3", "raw GSQRT node over a scalar"):
        assert f"ok  {what}\n" in driver
    for n, grades in ((7, [0, 1]), (8, [2]), (1, [0]), (0, [0])):
        _in(0, grades, n).gsqrt().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_inputs():
    """name -> (A over S, theta per item, longdouble root): drawn and referenced once for the module"""
    out = {}
    for name, (metric, grades, N, items) in ACCURACY_CASES.items():
        A, th = gs.operands(metric, grades, items, np.random.default_rng(SEED))
        out[name] = (A, th, gs.root_reference(metric, grades, A))
    return out


def test_longdouble_reference_agrees_with_mpmath_sqrtm(accuracy_inputs):
    """on leading items of the cases up to N = 16: mpmath.sqrtm of L_A at 50 digits, first column"""
    mp = pytest.importorskip("mpmath")
    assert mp
    for name in ("R1", "R3-even", "R3", "PGA3D-even", "PGA3D", "CGA-even"):
        metric, grades, N, items = ACCURACY_CASES[name]
        A, th, ref = accuracy_inputs[name]
        lead = [0, items, 2 * items, 3 * items]      # one item of every kind
        want = gs.sqrtm_reference(metric, grades, A[lead])
        assert np.abs(ref[lead].astype(np.float64) - want).max() <= 4 * 2.0 ** -52 * np.abs(want).max(), name


def test_the_root_of_gexp_b_is_gexp_of_half_b():
    rng = np.random.default_rng(SEED + 3)
    for metric, grades in ((PGA, [2]), (CGA, [2]), ([1.0] * 3, [0, 1, 2, 3])):
        B = gx.random_operand(metric, grades, 4, 2.5, rng, np.float64)
        A = gx.forward(metric, grades, B, np.longdouble, s_dtype=np.float64, degree=24)[0]
        half = gx.forward(metric, grades, B / 2, np.longdouble, s_dtype=np.float64, degree=24)[0]
        X = gs.forward(metric, grades, A, np.longdouble, max_steps=40)[0]
        assert np.abs(X - half).max() <= 1e-16 * np.abs(half).max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ACCURACY_CASES))
def test_restatement_forward_error_defines_the_scale(accuracy_inputs, name, dtype):
    metric, grades, N, items = ACCURACY_CASES[name]
    dt = np.dtype(dtype)
    A, th, ref = accuracy_inputs[name]
    X, steps, bad = gs.forward(metric, grades, A, dtype)
    assert not bad.any() and X.dtype == dt                 # the restatement converges for every input
    res, err = gs.residual(metric, grades, X, A, gs.EPS[dt]), gs.forward_error(X, ref, gs.EPS[dt])
    for t in sorted(set(th.tolist())):
        k = th == t
        print(f"FORWARD {name} {dt.name} theta={t}: steps {steps[k].min()}..{steps[k].max()} residual {res[k].max():.3f} error {err[k].max():.3f} N eps")
    assert steps.max() <= 8
    assert max(res.max(), err.max()) <= gs.FWD_SCALE[dt], (name, res.max(), err.max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ACCURACY_CASES))
def test_restatement_gradient_error_defines_the_scale(accuracy_inputs, name, dtype):
    metric, grades, N, items = ACCURACY_CASES[name]
    dt = np.dtype(dtype)
    A, th, ref = accuracy_inputs[name]
    g = np.random.default_rng(SEED + 1).uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
    got = gs.reverse(metric, grades, A, g, dtype)
    want = gs.reverse(metric, grades, A, g, np.longdouble, X=ref)
    kappa = gs.sum_condition(metric, grades, ref.astype(np.float64))
    worst = gs.gradient_error(got, want, gs.EPS[dt], kappa).max()
    print(f"GRADIENT {name} {dt.name}: worst {worst:.3f} N eps kappa |a|, kappa up to {kappa.max():.1f}")
    assert worst <= gs.GRAD_SCALE[dt], (name, worst)


def test_adjoint_solve_is_the_gradient():
    """central differences of the longdouble forward against the float64 solve: 1e-6 relative"""
    rng = np.random.default_rng(SEED + 2)
    for metric, grades in ((PGA, [0, 2, 4]), (CGA, [0, 2, 4]), ([1.0] * 3, [0, 1, 2, 3])):
        A, _ = gs.operands(metric, grades, 2, rng, np.float64)
        g = rng.uniform(-1, 1, A.shape)
        v = rng.uniform(-1, 1, A.shape)
        da = gs.reverse(metric, grades, A, g)
        f = lambda Z: gs.forward(metric, grades, Z, np.longdouble, max_steps=40)[0].astype(np.float64)
        jv = (f(A + 1e-6 * v) - f(A - 1e-6 * v)) / 2e-6
        lhs, rhs, scale = (g * jv).sum(axis=1), (da * v).sum(axis=1), (np.abs(g) * np.abs(jv)).sum(axis=1)
        assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


def test_domain_errors_of_the_restatement():
    """-1, a vector (eigenvalues +-1), 0, a NaN and an infinity are domain errors, and so is PGA's ideal element e0; 4 and 1 are not"""
    A = np.array([[-1.0, 0, 0, 0], [0, 1.0, 0, 0], [0.0, 0, 0, 0], [4.0, 0, 0, 0], [1.0, np.nan, 0, 0], [np.inf, 0, 0, 0], [1.0, 0, 0, 0]])
    for dtype in (np.float32, np.float64):
        X, steps, bad = gs.forward([1.0, 1.0], [0, 1, 2], A, dtype)
        assert list(bad) == [True, True, True, False, True, True, False] and np.isnan(X[bad]).all()
        assert np.abs(X[3] - [2.0, 0, 0, 0]).max() <= 4 * gs.EPS[np.dtype(dtype)] and np.array_equal(X[6], [1.0, 0, 0, 0]) and steps[6] == 0
        d = gs.reverse([1.0, 1.0], [0, 1, 2], A, np.ones_like(A), dtype)
        assert np.isnan(d[bad]).all() and np.isfinite(d[~bad]).all()
    e0 = np.zeros((1, 16))
    e0[0, 1] = 1.0
    assert gs.forward(PGA, [0, 1, 2, 3, 4], e0)[2].all()
