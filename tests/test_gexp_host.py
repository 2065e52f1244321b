"""The general multivector exponential (GAAST_OP_GEXP / GAAST_OP_GEXP_ADJ) on the host: grade inference, the phase-3 restriction, the
wire format, reverse mode, the lowered Step::GEXP / Step::GEXP_ADJ tables, and the numpy restatement of the algorithm
(gexp_numpy.py) against mpmath.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined (tests/cpp/gexp_sanitize_driver.cpp) and
run once: it must end clean, and the tables it prints from the lowered plans are what the tests below compare with numpy.

Accuracy of the restatement.  Inputs: default_rng(20261019), U(-1, 1) on the operand's grades, normalised to sum |A| = theta for
theta in {0.1, 1, 3, 8} and rounded to float32 (so both dtypes see the same values).  The forward error against mpmath (50 digits), in
units of N eps max(1, theta) ||exp(A)||_inf, must stay below 0.5 -- a quarter of the contract's 2.  The reverse sweep in the program's
dtype is compared with the same sweep in numpy.longdouble (s taken from the program's dtype) in units of
N eps max(1, theta) ||g||_inf ||exp(A)||_inf: the worst value is the scale of the GPU's gradient bound (gexp_numpy.GRAD_SCALE, asserted
here to cover what this run measures; the GPU is allowed 4 x that, its sums being contracted into fused multiply-adds)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import inverse_numpy as inu
from helpers import plan_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
SEED = 20261019
THETAS = [0.1, 1.0, 3.0, 8.0]
# name -> (metric, operand grades, N, items per theta)
ACCURACY_CASES = {
    "PGA3D-bivector": (PGA, [2], 8, 3), "PGA3D-full": (PGA, [0, 1, 2, 3, 4], 16, 3), "CGA-bivector": (CGA, [2], 16, 3),
    "R3-full": ([1.0] * 3, [0, 1, 2, 3], 8, 3), "R33-bivector": ([1.0] * 3 + [-1.0] * 3, [2], 32, 2), "R7-bivector": ([1.0] * 7, [2], 64, 1),
}


def _in(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _mask(grades):
    return sum(1 << k for k in grades)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("gexp_asan") / "gexp_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "gexp_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")


# ---- phases 2 and 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grades", [(3, [0, 2]), (4, [2]), (4, [0, 2, 4]), (5, [2]), (7, [2, 4]), (8, [2]), (3, [0])])
def test_even_operand_gives_the_even_grades(n, grades):
    spec = _in(0, grades, n).gexp().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_GEXP
    assert root.maximal_grade_mask == _mask(range(0, n + 1, 2)) == root.minimal_grade_mask


@pytest.mark.parametrize("n,grades", [(1, [0, 1]), (3, [1]), (4, [0, 1, 2, 3, 4]), (4, [1, 3]), (5, [2, 3]), (7, [0, 1]), (9, [1])])
def test_mixed_operand_gives_every_grade(n, grades):
    spec = _in(0, grades, n).gexp().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_GEXP
    assert root.maximal_grade_mask == _mask(range(n + 1)) == root.minimal_grade_mask


def test_phase_3_wants_the_operand_in_full_whatever_is_wanted_of_the_result():
    a, b = _in(0, [0, 1, 2, 3, 4], 4), _in(1, [0, 1, 2, 3, 4], 4)
    spec = ((a + b).gexp()).g(2).specialize(ga.MetricAlgebra(PGA))
    nodes = spec.nodes()
    ge = [nd for nd in nodes if nd.opcode == _lib.OP_GEXP]
    assert len(ge) == 1
    assert ge[0].maximal_grade_mask == 0x1f and ge[0].minimal_grade_mask == 1 << 2   # produces only the wanted grade
    child = nodes[ge[0].child0]
    assert child.opcode == _lib.OP_ADD and child.minimal_grade_mask == child.maximal_grade_mask == 0x1f
    for leaf in (nodes[child.child0], nodes[child.child1]):
        assert leaf.minimal_grade_mask == leaf.maximal_grade_mask


def test_exp_is_what_it_was():
    """exp() keeps its opcode and its single-grade rule; gexp() is a node of its own"""
    b = _in(0, [2], 3)
    assert [nd.opcode for nd in b.exp().specialize(ga.MetricAlgebra([1.0] * 3)).nodes()].count(_lib.OP_EXP) == 1
    assert _lib.OP_GEXP not in [nd.opcode for nd in b.exp().specialize(ga.MetricAlgebra([1.0] * 3)).nodes()]
    assert (_lib.OP_GEXP, _lib.OP_GEXP_ADJ) == (16, 17) and _lib.OP_NAMES[16] == "GeneralExponential"


# ---- wire format ------------------------------------------------------------------------------------------------------------------
def test_wire_round_trip():
    L = _lib.lib()
    spec = ((_in(0, [2], 4) + _in(1, [2], 4)).gexp() * _in(2, [1], 4)).specialize(ga.MetricAlgebra(PGA))
    desc = spec.program_desc()
    data = spec.serialize()
    img = ga.ast.ProgramImage(data)
    back = img.desc
    assert back.n_nodes == desc.n_nodes and back.root == desc.root
    ops = [back.nodes[i].opcode for i in range(back.n_nodes)]
    assert ops == [desc.nodes[i].opcode for i in range(desc.n_nodes)] and ops.count(_lib.OP_GEXP) == 1
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
def test_vjp_program_of_gexp_x_is_one_adjoint_node_over_g_and_x(driver, tag, mask):
    """two inputs and one GEXP_ADJ node: child0 the cotangent (slot 1), child1 the operand (slot 0), the node's mask the operand's;
    the forward is not re-evaluated by a node of its own"""
    ops = [l.split() for l in driver.splitlines() if l.startswith(f"VJPOPS {tag} ")]
    adj = [l.split() for l in driver.splitlines() if l.startswith(f"VJPADJ {tag} ")]
    assert [o[2:] for o in ops] == [["0", "3", "1", "0"]]
    assert [a[2:] for a in adj] == [["0", str(_lib.OP_INPUT), "1", str(_lib.OP_INPUT), "0", str(mask)]]


def test_vjp_through_python_needs_no_flag():
    spec = _in(0, [2], 4).gexp().specialize(ga.MetricAlgebra(PGA))
    img = spec.vjp_image(0) if hasattr(spec, "vjp_image") else None
    if img is None:
        L = _lib.lib()
        desc = spec.program_desc()
        out = C.c_void_p()
        assert L.gaast_program_vjp(C.byref(desc), 0, C.byref(out)) == 0
        d = C.cast(L.gaast_program_image_desc(out), C.POINTER(type(desc))).contents
        assert [d.nodes[i].opcode for i in range(d.n_nodes)].count(_lib.OP_GEXP_ADJ) == 1
        L.gaast_program_image_free(out)


# ---- the lowered steps ------------------------------------------------------------------------------------------------------------
CASES = {   # tag -> (metric, operand grades, produced grades or None for all)
    "full1": ([1.0], [0, 1], None), "full2": ([1.0] * 2, [0, 1, 2], None), "full3": ([1.0] * 3, [0, 1, 2, 3], None),
    "even2": ([1.0] * 2, [0, 2], None), "even3": ([1.0] * 3, [0, 2], None),
    "pga-biv": (PGA, [2], None), "pga-full": (PGA, [0, 1, 2, 3, 4], None), "cga-biv": (CGA, [2], None),
    "odd-full": ([2.0, -0.5, 1.0], [0, 1, 2, 3], None), "pga-13": (PGA, [1, 3], None), "pga-g2": (PGA, [0, 1, 2, 3, 4], [2]),
    "pga-rev": (PGA, [2], None),
}


def _tables(driver, tag):
    outs, tab, adj = {}, {}, {}
    for line in driver.splitlines():
        f = line.split()
        if len(f) < 2 or f[1] != tag:
            continue
        if f[0] == "GEXPOUT":
            outs.setdefault(int(f[3]), []).append((int(f[2]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), float(f[8])))
        elif f[0] == "GEXPTAB":
            tab.setdefault((int(f[2]), int(f[3])), []).append(float(f[4]))
        elif f[0] == "ADJTAB":
            adj.setdefault((int(f[2]), int(f[3])), []).append((float(f[4]), float(f[5]), int(f[6]), int(f[7])))
    return outs, tab, adj


@pytest.mark.parametrize("tag", sorted(CASES))
def test_lowered_tables_match_numpy(driver, tag):
    """The forward step's blade list, offsets, wmax and N x N coefficients, and the adjoint step's two coefficient tables, cotangent
    and result offsets, equal gexp_numpy's entry for entry (the forward program's step is printed first, then the VJP program's)"""
    metric, grades, produced = CASES[tag]
    n = len(metric)
    outs, tab, adj = _tables(driver, tag)
    S, Cm, wmax = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    flip = {2, 3} if tag == "pga-rev" else set()   # gexp(~B): the reverse of a bound input is folded into the operand read
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
    # the adjoint step of the VJP program with respect to slot 0: ADJL / ADJR coefficient of (a, b) is that of L[a xor b][b]
    g_where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(res_grades)))}
    assert len(adj) == N * N
    for a in range(N):
        for b in range(N):
            cl, cr, g_off, res_off = adj[(a, b)][0]
            assert cl == cr == Cm[a ^ b, b], (a, b)
            assert g_off == g_where.get(S[a], -1)
            assert res_off == where.get(S[a], -1)     # the cotangent lands on the operand's own components


def test_unsupported_sizes_are_refused_only_by_the_device_plan(driver):
    """N > 64 (n = 7 mixed, n = 8) and N = 1 (an even operand at n = 1, a scalar at n = 0) specialise and lower without an error, but
    the plan names what the back end cannot do (-> GAAST_ERR_UNIMPLEMENTED at gaast_hip_program_create); the driver asserts
    plan.unsupported for each of them and its emptiness for the supported sizes"""
    for what in ("gexp(full) n=7", "gexp(full) n=8", "gexp(even) n=8", "gexp(even) n=1", "gexp(scalar) n=0", "gexp(even) n=7", "gexp(full) n=6", "gexp(scalar) n=3"):
        assert f"ok  {what}\n" in driver
    for n, grades in ((7, [0, 1]), (8, [2]), (1, [0]), (0, [0])):
        _in(0, grades, n).gexp().specialize(ga.MetricAlgebra([1.0] * n))      # phases 1-3 succeed


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_taylor_degrees_and_squarings():
    assert gx.taylor_degree(2.0 ** -23) == 8 == gx.DEGREE[np.dtype(np.float32)]
    assert gx.taylor_degree(2.0 ** -52) == 14 == gx.DEGREE[np.dtype(np.float64)]
    th = np.array([0.0, 0.3, 0.5, np.nextafter(0.5, 1), 1.0, np.nextafter(1.0, 2), 2048.0, np.nextafter(2048.0, 4096), 4096.0, np.inf, np.nan])
    s, bad = gx.squarings_of(th)
    assert list(s[:7]) == [0, 0, 0, 1, 1, 2, 12] and list(bad) == [False] * 7 + [True] * 4
    for t, k in zip(th[:7], s[:7]):
        assert t * 2.0 ** -int(k) <= 0.5 and (k == 0 or t * 2.0 ** -(int(k) - 1) > 0.5)


@pytest.fixture(scope="module")
def accuracy_inputs():
    """name -> theta -> (A over S, mpmath reference): drawn and referenced once for the module"""
    out = {}
    for name, (metric, grades, N, items) in ACCURACY_CASES.items():
        rng = np.random.default_rng(SEED)
        out[name] = {}
        for th in THETAS:
            A = gx.random_operand(metric, grades, items, th, rng)
            out[name][th] = (A, gx.exp_reference(metric, grades, A))
    return out


def test_series_reference_agrees_with_mpmath_expm(accuracy_inputs):
    for name in ("PGA3D-bivector", "R3-full", "CGA-bivector"):
        metric, grades, N, _ = ACCURACY_CASES[name]
        for th in THETAS:
            A, ref = accuracy_inputs[name][th]
            assert np.array_equal(gx.exp_reference(metric, grades, A[:1], method="expm"), ref[:1]), (name, th)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ACCURACY_CASES))
def test_restatement_forward_error_is_below_a_quarter_of_the_contract(accuracy_inputs, name, dtype):
    metric, grades, N, _ = ACCURACY_CASES[name]
    eps = gx.EPS[np.dtype(dtype)]
    for th in THETAS:
        A, ref = accuracy_inputs[name][th]
        y, s, bad = gx.forward(metric, grades, A, dtype)
        assert not bad.any() and y.dtype == np.dtype(dtype)
        worst = gx.forward_error(y, ref, N, eps, th).max()
        print(f"FORWARD {name} {np.dtype(dtype).name} theta={th}: s={sorted(set(s.tolist()))} worst {worst:.3f} N eps max(1, theta) |y|")
        assert worst <= 0.5, (name, th, worst)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(ACCURACY_CASES))
def test_restatement_gradient_error_defines_the_scale(accuracy_inputs, name, dtype):
    metric, grades, N, _ = ACCURACY_CASES[name]
    eps = gx.EPS[np.dtype(dtype)]
    rng = np.random.default_rng(SEED + 1)
    worst = 0.0
    for th in THETAS:
        A, ref = accuracy_inputs[name][th]
        g = rng.uniform(-1, 1, A.shape).astype(np.float32).astype(np.float64)
        got = gx.reverse(metric, grades, A, g, dtype).astype(np.float64)
        want = gx.reverse(metric, grades, A, g, np.longdouble, s_dtype=dtype).astype(np.float64)
        worst = max(worst, gx.gradient_error(got, want, N, eps, th, g, ref).max())
    print(f"GRADIENT {name} {np.dtype(dtype).name}: worst {worst:.3f} N eps max(1, theta) |g| |y|")
    assert worst <= gx.GRAD_SCALE[np.dtype(dtype)], (name, worst)


def test_reverse_sweep_is_the_gradient():
    """central differences of the longdouble forward (s held at the float64 value), float64 sweep: 1e-6 relative"""
    rng = np.random.default_rng(SEED + 2)
    for metric, grades in ((PGA, [2]), (CGA, [2]), ([1.0] * 3, [0, 1, 2, 3])):
        A = gx.random_operand(metric, grades, 4, 3.0, rng, np.float64)
        g = rng.uniform(-1, 1, A.shape)
        v = gx.restrict(metric, grades, rng.uniform(-1, 1, A.shape))
        da = gx.restrict(metric, grades, gx.reverse(metric, grades, A, g))
        f = lambda X: gx.forward(metric, grades, X, np.longdouble, s_dtype=np.float64)[0].astype(np.float64)
        jv = (f(A + 1e-6 * v) - f(A - 1e-6 * v)) / 2e-6
        lhs, rhs, scale = (g * jv).sum(axis=1), (da * v).sum(axis=1), (np.abs(g) * np.abs(jv)).sum(axis=1)
        assert np.all(np.abs(lhs - rhs) <= 1e-6 * scale), (np.abs(lhs - rhs) / scale).max()


def test_domain_errors_of_the_restatement():
    A = np.array([[0.0, 4096.0, 0, 0], [0.25, 0.25, 0, 0], [np.inf, 0, 0, 0], [0, np.nan, 0, 0], [0, 0, 0, 2048.0]])
    y, s, bad = gx.forward([1.0, 1.0], [0, 1, 2], A)
    assert list(bad) == [True, False, True, True, False] and np.isnan(y[bad]).all() and np.isfinite(y[1]).all()
    assert s[4] == 12 and y[4, 0] == pytest.approx(np.cos(2048.0), abs=1e-9) and y[4, 3] == pytest.approx(np.sin(2048.0), abs=1e-9)   # e12 e12 = -1
    d = gx.reverse([1.0, 1.0], [0, 1, 2], A, np.ones_like(A))
    assert np.isnan(d[bad]).all() and np.isfinite(d[1]).all()
