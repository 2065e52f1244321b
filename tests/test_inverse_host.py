"""The general multivector inverse (GAAST_OP_INV) on the host: grade inference, the phase-3 restriction, the scalar form, the wire
format, reverse mode and the lowered Step::INVERSE, against the numpy reference of inverse_numpy.py.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined (tests/cpp/inverse_sanitize_driver.cpp)
and run once: it must end clean, and the matrices it prints from the lowered plans are what the tests below compare with numpy
entry for entry."""
import ctypes as C
import os
import subprocess

import pytest

import gaast_amd as ga
from gaast_amd import _lib

import inverse_numpy as inu
from helpers import plan_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]


def _in(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _mask(grades):
    return sum(1 << k for k in grades)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("inverse_asan") / "inverse_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "inverse_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")


# ---- phases 2 and 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grades", [(3, [0, 2]), (4, [0, 2, 4]), (4, [2]), (5, [0, 2]), (7, [0, 2, 4, 6]), (8, [0, 2])])
def test_even_operand_gives_the_even_grades(n, grades):
    spec = _in(0, grades, n).inv().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_INV
    assert root.maximal_grade_mask == _mask(range(0, n + 1, 2)) == root.minimal_grade_mask


@pytest.mark.parametrize("n,grades", [(1, [0, 1]), (3, [1]), (4, [0, 1, 2, 3, 4]), (4, [1, 3]), (5, [0, 2, 3]), (7, [0, 1]), (9, [1])])
def test_mixed_operand_gives_every_grade(n, grades):
    spec = _in(0, grades, n).inv().specialize(ga.MetricAlgebra([1.0] * n))
    root = spec.nodes()[spec.root_id()]
    assert root.opcode == _lib.OP_INV
    assert root.maximal_grade_mask == _mask(range(n + 1)) == root.minimal_grade_mask


def test_phase_3_wants_the_operand_in_full_whatever_is_wanted_of_the_result():
    a, b = _in(0, [0, 1, 2, 3, 4], 4), _in(1, [0, 1, 2, 3, 4], 4)
    spec = ((a + b).inv()).g(2).specialize(ga.MetricAlgebra(PGA))
    nodes = spec.nodes()
    inv = [nd for nd in nodes if nd.opcode == _lib.OP_INV]
    assert len(inv) == 1
    assert inv[0].maximal_grade_mask == 0x1f and inv[0].minimal_grade_mask == 1 << 2   # produces only the wanted grade
    child = nodes[inv[0].child0]
    assert child.opcode == _lib.OP_ADD and child.minimal_grade_mask == child.maximal_grade_mask == 0x1f
    for leaf in (nodes[child.child0], nodes[child.child1]):
        assert leaf.minimal_grade_mask == leaf.maximal_grade_mask


def test_scalar_operand_lowers_to_sinv():
    for e in (_in(0, [0], 4).inv(), (_in(0, [1], 4) & _in(1, [1], 4)).inv(), ga.Expr._lift(2.0).inv()):
        spec = e.specialize(ga.MetricAlgebra(PGA))
        ops = [nd.opcode for nd in spec.nodes()]
        assert _lib.OP_INV not in ops and ops.count(_lib.OP_SINV) == 1


def test_truediv_and_rtruediv_build_products_with_the_inverse():
    a, b = _in(0, [0, 2], 3), _in(1, [1], 3)
    for e in (b / a, 1 / a, 1.0 / a):
        ops = [nd.opcode for nd in e.specialize(ga.MetricAlgebra([1.0] * 3)).nodes()]
        assert ops.count(_lib.OP_INV) == 1 and ops.count(_lib.OP_PRODUCT) == 1
    # a float divisor takes the scalar-division path it always took: no inverse node
    for e in (a / 2.0, a / 2):
        assert _lib.OP_INV not in [nd.opcode for nd in e.specialize(ga.MetricAlgebra([1.0] * 3)).nodes()]
    # vinv() is what it was: rev(a) * sinv(norm_sq(a))
    assert _lib.OP_INV not in [nd.opcode for nd in a.vinv().specialize(ga.MetricAlgebra([1.0] * 3)).nodes()]


# ---- wire format ------------------------------------------------------------------------------------------------------------------
def test_wire_round_trip():
    L = _lib.lib()
    spec = (_in(1, [1], 4) / (_in(0, [0, 2, 4], 4) + 1.0)).specialize(ga.MetricAlgebra(PGA))
    desc = spec.program_desc()
    data = spec.serialize()
    img = ga.ast.ProgramImage(data)
    back = img.desc
    assert back.n_nodes == desc.n_nodes and back.root == desc.root
    ops = [back.nodes[i].opcode for i in range(back.n_nodes)]
    assert ops == [desc.nodes[i].opcode for i in range(desc.n_nodes)] and ops.count(_lib.OP_INV) == 1
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
def _vjpops(driver):
    out = {}
    for line in driver.splitlines():
        if line.startswith("VJPOPS "):
            _, tag, inv, adj_l, adj_r, neg, prod = line.split()
            out[tag] = tuple(int(x) for x in (inv, adj_l, adj_r, neg, prod))
    return out


@pytest.mark.parametrize("tag", ["full1", "full3", "even3", "pga-full", "pga-even", "cga-full", "odd-full", "pga-13"])
def test_vjp_program_is_one_inverse_two_adjoint_products_and_a_negation(driver, tag):
    """Y = inv(A) recomputed once, ADJ_LEFT then ADJ_RIGHT geometric products with it, one Negation, no other product"""
    assert _vjpops(driver)[tag] == (1, 1, 1, 1, 2)


# ---- the lowered step -------------------------------------------------------------------------------------------------------------
CASES = {   # tag -> (metric, operand grades, produced grades or None for all)
    "full1": ([1.0], [0, 1], None), "full2": ([1.0] * 2, [0, 1, 2], None), "full3": ([1.0] * 3, [0, 1, 2, 3], None),
    "even2": ([1.0] * 2, [0, 2], None), "even3": ([1.0] * 3, [0, 2], None),
    "pga-full": (PGA, [0, 1, 2, 3, 4], None), "pga-even": (PGA, [0, 2, 4], None), "cga-full": (CGA, [0, 1, 2, 3, 4, 5], None),
    "odd-full": ([2.0, -0.5, 1.0], [0, 1, 2, 3], None), "pga-13": (PGA, [1, 3], None), "pga-g2": (PGA, [0, 1, 2, 3, 4], [2]),
    "pga-rev": (PGA, [0, 1, 2, 3, 4], None),
}


def _steps(driver):
    tabs, outs = {}, {}
    for line in driver.splitlines():
        if line.startswith("INVTAB "):
            _, tag, r, j, c, src = line.split()
            tabs.setdefault(tag, {})[(int(r), int(j))] = (float(c), int(src))
        elif line.startswith("INVOUT "):
            _, tag, N, j, blade, a_off, res_off, neg = line.split()
            outs.setdefault(tag, {})[int(j)] = (int(N), int(blade), int(a_off), int(res_off), int(neg))
    return tabs, outs


@pytest.mark.parametrize("tag", sorted(CASES))
def test_lowered_matrix_offsets_and_signs_match_numpy(driver, tag):
    """One INVERSE step whose blade list, operand / result offsets and N x N coefficients equal inverse_numpy's, entry for entry"""
    metric, grades, produced = CASES[tag]
    n = len(metric)
    tabs, outs = _steps(driver)
    S, Cm, src = inu._structure(tuple(metric), tuple(grades))
    N = len(S)
    assert len(outs[tag]) == N and len(tabs[tag]) == N * N   # exactly one step printed under the tag
    flip = {2, 3} if tag == "pga-rev" else set()   # inv(~a): the reverse of a bound input is folded into the operand read
    where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(grades)))}
    res_grades = inu.result_grades(n, tuple(grades)) if produced is None else produced
    res_where = {b: i for i, b in enumerate(inu.row_blades(n, tuple(res_grades)))}
    for j in range(N):
        Nn, blade, a_off, res_off, neg = outs[tag][j]
        assert Nn == N and blade == S[j]
        assert neg == (1 if inu.grade(blade) in flip else 0)
        assert a_off == where.get(blade, -1)
        assert res_off == res_where.get(blade, -1)
    for r in range(N):
        for j in range(N):
            c, s = tabs[tag][(r, j)]
            assert s == src[r, j], (r, j)
            if s >= 0:
                assert c == Cm[r, j], (r, j, c, Cm[r, j])


def test_unsupported_sizes_are_refused_only_by_the_device_plan(driver):
    """n = 7 mixed and n = 8 even specialise (phases 1-3) and lower without an error, but name what the back end cannot do"""
    for what in ("inv(full) n=7", "inv(full) n=8", "inv(even) n=8", "inv(even) n=7", "inv(full) n=6"):
        assert f"ok  {what}\n" in driver
