"""Complements (dual / undual) and the regressive product on the host: index rule, signs, lists, grade inference, wire format,
reverse mode and the orientation sign of a Gram basis, against the numpy reference of dual_numpy.py.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined (tests/cpp/dual_sanitize_driver.cpp)
and run once: it must end clean, and the sign tables it prints from the lowered plans (Step::DUAL, the regressive lists) are
what several tests below compare with numpy."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import dual_numpy as dn
from helpers import HipBackend, OracleBackend, plan_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]


def _in(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("dual_asan") / "dual_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "dual_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")


def _dual_tables(driver):
    """{(tag, n): {operand offset: (result offset, negate)}} of the lowered dual(x) / undual(x) over full multivectors"""
    out = {}
    for line in driver.splitlines():
        if line.startswith("DUALTAB "):
            _, tag, n, undual, r, a, neg = line.split()
            assert (tag.split("-")[0] == "undual") == (undual == "1")
            tab = out.setdefault((tag, int(n)), {})
            assert int(a) not in tab
            tab[int(a)] = (int(r), int(neg))
    return out


# ---- index rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 11))
def test_index_rule_against_the_blade_table(n):
    """component i of grade k <-> the complement blade is component C(n,k) - 1 - i of grade n - k, in the library's blade table
    and in the reference's enumeration"""
    L = _lib.lib()
    full = (1 << n) - 1
    for k in range(n + 1):
        c = math.comb(n, k)
        ref = dn.blades(n, k)
        for i in range(c):
            blade = L.gaast_component_to_blade(n, k, i)
            assert blade == ref[i]
            g = C.c_int()
            j = L.gaast_blade_to_component(n, ~blade & full, C.byref(g))
            assert (g.value, j) == (n - k, c - 1 - i)
    for k, i, j in dn.permutation_check(n):
        assert j == math.comb(n, k) - 1 - i


@pytest.mark.parametrize("n", range(1, 9))
def test_lowered_sign_tables_match_numpy(driver, n):
    tabs = _dual_tables(driver)
    src = dn.row_blades(n, range(n + 1))
    pos = {m: i for i, m in enumerate(src)}
    full = (1 << n) - 1
    for tag, sign in (("dual", dn.dual_sign), ("undual", dn.undual_sign)):
        tab, mirrored = tabs[(tag, n)], tabs[(tag + "-mirrored", n)]
        assert sorted(tab) == list(range(1 << n))
        for a, s in enumerate(src):
            assert tab[a] == (pos[~s & full], 1 if sign(n, s) < 0 else 0), (tag, n, a)
            assert mirrored[a] == (tab[a][0], 1 - tab[a][1])   # det Q = -1 negates every sign


@pytest.mark.parametrize("n", range(1, 9))
def test_undual_inverts_dual(driver, n):
    # in the reference ...
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (3, 1 << n))
    d, g = dn.complement_rows(n, range(n + 1), x)
    back, _ = dn.complement_rows(n, g, d, undual=True)
    assert np.array_equal(back, x)
    assert np.array_equal(dn.complement_rows(n, g, dn.complement_rows(n, range(n + 1), x, undual=True)[0])[0], x)
    # ... and in the lowered tables
    tabs = _dual_tables(driver)
    dual, undual = tabs[("dual", n)], tabs[("undual", n)]
    for a in range(1 << n):
        r, s1 = dual[a]
        a2, s2 = undual[r]
        assert (a2, s1 ^ s2) == (a, 0)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_euclidean_dual_is_rev_times_pseudoscalar(driver, n):
    """dual(a) == a.rev() * I in a Euclidean metric: the geometric product's list (the library's, equal to the oracle's) with the
    reverse's sign is the lowered dual table.  This check does not rest on dual_numpy."""
    grades = list(range(n + 1))

    def build(B):
        return B.input(0, grades, n).rev() * B.value({n: [1.0]}, dim=n)

    metric = [1.0] * n
    hspec = build(HipBackend()).specialize(metric)
    ospec = build(OracleBackend()).specialize(metric)
    prod = [i for i, nd in enumerate(hspec.nodes()) if nd.opcode == _lib.OP_PRODUCT]
    assert len(prod) == 1
    lst = hspec.comp_muls(prod[0])
    assert lst == ospec.comp_muls(prod[0])
    off = {k: sum(math.comb(n, j) for j in range(k)) for k in grades}
    tab = _dual_tables(driver)[("dual", n)]
    assert len(lst) == 1 << n
    for lg, li, rg, ri, og_, oi, c in lst:
        assert (rg, ri, og_) == (n, 0, n - lg)
        rev = -1.0 if lg % 4 in (2, 3) else 1.0
        assert tab[off[lg] + li] == (off[n - lg] + oi, 1 if c * rev < 0 else 0)


# ---- the regressive list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5])
def test_vee_list_matches_numpy_in_a_degenerate_metric(n):
    grades = list(range(n + 1))
    spec = _in(0, grades, n).vee(_in(1, grades, n)).specialize([0.0] + [1.0] * (n - 1), materialize_limit=0)
    root = spec.get_node(spec.root_id())
    assert root.opcode == _lib.OP_PRODUCT and root.product_kind == _lib.PROD_REGRESSIVE
    lst = spec.comp_muls(spec.root_id())
    ref = dn.vee_list(n, grades, grades)
    assert len(lst) == 3 ** n == len(ref)
    assert lst == ref
    # order T4: k_left, k_right, left index, right index, all ascending
    assert [(m[0], m[2], m[1], m[3]) for m in lst] == sorted((m[0], m[2], m[1], m[3]) for m in lst)
    assert all(abs(m[6]) == 1.0 for m in lst)
    # I v x = x
    unit = [m for m in lst if m[0] == n]
    assert len(unit) == 1 << n and all((m[2], m[3], 1.0) == (m[4], m[5], m[6]) for m in unit)


@pytest.mark.parametrize("n", range(1, 9))
def test_comp_mul_count_is_the_list_length(n):
    cases = [(list(range(n + 1)), list(range(n + 1)))]
    if n >= 3:
        cases += [([n - 1], [n - 1]), ([n - 1, n], [1, n - 2, n - 1]), ([2], [n - 1, n])]
    for lg, rg in cases:
        lg, rg = sorted(set(lg)), sorted(set(rg))
        e = _in(0, lg, n).vee(_in(1, rg, n))
        explicit = e.specialize([1.0] * n, materialize_limit=0)
        compact = e.specialize([1.0] * n, materialize_limit=1)
        want = len(dn.vee_list(n, lg, rg)) if n <= 6 else None
        node = explicit.get_node(explicit.root_id())
        lst = explicit.comp_muls(explicit.root_id())
        assert node.n_comp_muls == (len(lst) if lst is not None else 0)
        assert compact.get_node(compact.root_id()).n_comp_muls == node.n_comp_muls
        if want is not None:
            assert node.n_comp_muls == want
        if node.n_comp_muls > 1:
            assert compact.comp_muls(compact.root_id()) is None


def test_lowered_vee_list_and_its_orientation_sign(driver):
    """the plan's list rows are the numpy list grouped by result; compact descriptors regenerate the same; det Q = -1 negates"""
    tabs = {}
    for line in driver.splitlines():
        if line.startswith("VEETAB "):
            _, tag, r, lo, ro, c = line.split()
            tabs.setdefault(tag, []).append((int(r), int(lo), int(ro), float(c)))
    n, grades = 3, [0, 1, 2, 3]
    off = {k: sum(math.comb(n, j) for j in range(k)) for k in grades}
    ref = sorted(((off[g] + oi, off[kl] + li, off[kr] + ri, c) for kl, li, kr, ri, g, oi, c in dn.vee_list(n, grades, grades)),
                 key=lambda m: m[0])   # stable: list order within a result component
    assert tabs["explicit"] == ref and tabs["compact"] == ref
    flipped = [(r, lo, ro, -c) for r, lo, ro, c in ref]
    assert tabs["explicit-mirrored"] == flipped and tabs["compact-mirrored"] == flipped


# ---- grade inference, phase 3 -------------------------------------------------------------------------------------------------
def test_grade_inference_and_restriction():
    n = 4
    a, b = _in(0, [1, 2, 3], n), _in(1, [2, 3], n)
    spec = a.vee(b).specialize(PGA)
    nodes = spec.nodes()
    root = nodes[spec.root_id()]
    assert root.maximal_grade_mask == root.minimal_grade_mask == 0b0111   # 1+3, 2+2 -> 0; 2+3, 3+2 -> 1; 3+3 -> 2
    full_len = root.n_comp_muls
    g1 = a.vee(b).g(1).specialize(PGA, materialize_limit=0)
    nodes = g1.nodes()
    prod = [i for i, nd in enumerate(nodes) if nd.opcode == _lib.OP_PRODUCT][0]
    p = nodes[prod]
    assert p.minimal_grade_mask == 0b0010
    assert nodes[p.child0].minimal_grade_mask == 0b1100 and nodes[p.child1].minimal_grade_mask == 0b1100   # only (2,3) and (3,2) reach grade 1
    assert 0 < p.n_comp_muls < full_len
    assert g1.comp_muls(prod) == dn.vee_list(n, [2, 3], [2, 3], {1})
    # complements mirror the grade sets both ways
    d = _in(0, [1, 3], n).dual().g(3).specialize(PGA)
    nodes = d.nodes()
    dual = [nd for nd in nodes if nd.opcode == _lib.OP_DUAL][0]
    assert dual.maximal_grade_mask == 0b1010 and dual.minimal_grade_mask == 0b1000
    assert nodes[dual.child0].minimal_grade_mask == 0b0010
    u = _in(0, [0, 4], n).undual().specialize(PGA)
    assert u.get_node(u.root_id()).opcode == _lib.OP_UNDUAL and u.get_node(u.root_id()).minimal_grade_mask == 0b10001
    # a scalar literal (storage dimension 0) dualises to grade n of the algebra
    lit = ga.Expr._lift(2.5).dual().specialize(PGA)
    assert lit.get_node(lit.root_id()).minimal_grade_mask == 1 << n
    # the dimension-free helpers of the public header answer "nothing" for the one kind that needs the dimension
    assert _lib.lib().gaast_gs_select(_lib.PROD_REGRESSIVE, 3, 3) == 0
    lw, rw = C.c_uint64(7), C.c_uint64(7)
    _lib.lib().gaast_gs_parts_contributing_to_product(0b100, _lib.PROD_REGRESSIVE, 0b1000, 0b1000, C.byref(lw), C.byref(rw))
    assert (lw.value, rw.value) == (0, 0)


def test_empty_result_is_a_zero_program_not_an_error():
    spec = _in(0, [1], 4).vee(_in(1, [1], 4)).specialize(PGA)   # 1 + 1 - 4 < 0
    root = spec.get_node(spec.root_id())
    assert root.minimal_grade_mask == 0 and root.n_comp_muls == 0
    img = C.c_void_p()
    d = spec.program_desc()
    assert _lib.lib().gaast_program_vjp(C.byref(d), 0, C.byref(img)) == 0   # ... and so is its gradient
    _lib.lib().gaast_program_image_free(img)


# ---- wire format ----------------------------------------------------------------------------------------------------------------
def test_wire_round_trip_keeps_opcodes_and_kind():
    n = 4
    e = (_in(0, [3], n).vee(_in(1, [3], n))).dual() + _in(2, [1, 2], n).undual().g(2)
    for limit in (0, 1):
        spec = e.specialize(PGA, materialize_limit=limit)
        d = spec.program_desc()
        img = ga.ProgramImage(spec.serialize())
        assert img.desc.n_nodes == d.n_nodes and img.desc.root == d.root
        ops = [d.nodes[i].opcode for i in range(d.n_nodes)]
        assert _lib.OP_DUAL in ops and _lib.OP_UNDUAL in ops
        for i in range(d.n_nodes):
            a, b = d.nodes[i], img.desc.nodes[i]
            assert (a.opcode, a.child0, a.child1, a.minimal_grade_mask, a.product_kind, a.n_comp_muls) == \
                   (b.opcode, b.child0, b.child1, b.minimal_grade_mask, b.product_kind, b.n_comp_muls)
            assert bool(a.comp_muls) == bool(b.comp_muls)
            if a.opcode == _lib.OP_PRODUCT:
                assert a.product_kind == _lib.PROD_REGRESSIVE and bool(a.comp_muls) == (limit == 0)
                for k in range(a.n_comp_muls if a.comp_muls else 0):
                    assert bytes(a.comp_muls[k]) == bytes(b.comp_muls[k])


# ---- reverse mode -----------------------------------------------------------------------------------------------------------------
def _adjoint(spec, slot):
    d = spec.program_desc()
    img = C.c_void_p()
    st = _lib.lib().gaast_program_vjp(C.byref(d), slot, C.byref(img))
    assert st == 0, _lib.lib().gaast_expr_last_error()
    return img, _lib.lib().gaast_program_image_desc(img).contents, d


@pytest.mark.parametrize("n,lg,rg", [(3, [0, 1, 2, 3], [0, 1, 2, 3]), (4, [3], [3]), (4, [2, 3], [1, 3, 4]), (5, [4], [3, 4])])
def test_vjp_lists_are_the_numpy_transposes(n, lg, rg):
    spec = _in(0, lg, n).vee(_in(1, rg, n)).specialize([0.0] + [1.0] * (n - 1), materialize_limit=0)
    fwd = dn.vee_list(n, lg, rg)
    for slot in (0, 1):
        img, a, d = _adjoint(spec, slot)
        try:
            prods = [a.nodes[i] for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_PRODUCT]   # (the forward product is not kept)
            assert len(prods) == 1
            p = prods[0]
            assert p.product_kind == _lib.PROD_REGRESSIVE and p.comp_muls   # explicit, and still names its kind
            got = [(m.left_grade, m.left_index, m.right_grade, m.right_index, m.result_grade, m.result_index, m.coeff)
                   for m in (p.comp_muls[k] for k in range(p.n_comp_muls))]
            assert got == dn.transpose_list(fwd, right=slot == 1)
            cot, other = (p.child0, p.child1) if slot == 0 else (p.child1, p.child0)
            assert a.nodes[cot].opcode == _lib.OP_INPUT and a.nodes[cot].input_slot == d.n_inputs
            assert a.nodes[other].input_slot == 1 - slot
        finally:
            _lib.lib().gaast_program_image_free(img)
    # compact forward products get compact adjoints of the same kind
    compact = _in(0, lg, n).vee(_in(1, rg, n)).specialize([1.0] * n, materialize_limit=1)
    for slot, adj in ((0, _lib.PROD_ADJ_LEFT), (1, _lib.PROD_ADJ_RIGHT)):
        img, a, d = _adjoint(compact, slot)
        try:
            p = [a.nodes[i] for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_PRODUCT][0]
            assert p.product_kind == adj + _lib.PROD_REGRESSIVE and not p.comp_muls and p.n_comp_muls == len(fwd)
        finally:
            _lib.lib().gaast_program_image_free(img)


def test_vjp_of_a_complement_is_the_other_complement():
    n = 4
    for build, fwd_op, adj_op in ((lambda x: x.dual(), _lib.OP_DUAL, _lib.OP_UNDUAL), (lambda x: x.undual(), _lib.OP_UNDUAL, _lib.OP_DUAL)):
        spec = build(_in(0, [1, 2], n)).specialize(PGA)
        img, a, d = _adjoint(spec, 0)
        try:
            root = a.nodes[a.root]
            assert root.opcode == adj_op and root.minimal_grade_mask == 0b00110
            cot = a.nodes[root.child0]
            assert cot.opcode == _lib.OP_INPUT and cot.input_slot == d.n_inputs and cot.minimal_grade_mask == 0b01100
            assert all(a.nodes[i].opcode != fwd_op for i in range(a.n_nodes))
        finally:
            _lib.lib().gaast_program_image_free(img)
    # the cotangent is restricted to the node's grades: dual(x).g(3) of x = <x>_1 + <x>_2 only feeds grade 1 back
    spec = _in(0, [1, 2], n).dual().g(3).specialize(PGA)
    img, a, d = _adjoint(spec, 0)
    try:
        und = [a.nodes[i] for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_UNDUAL]
        assert len(und) == 1 and und[0].minimal_grade_mask == 0b00010
        assert a.inputs[d.n_inputs].grade_mask == 0b01000
    finally:
        _lib.lib().gaast_program_image_free(img)


def test_reference_transposes_are_adjoint():
    """<cot, J v> == <J^T cot, v> inside the numpy reference itself (what the GPU tests then rely on)"""
    rng = np.random.default_rng(5)
    n, lg, rg, og_ = 4, [2, 3], [3], [1, 2]
    a, b = rng.uniform(-1, 1, (2, 10)), rng.uniform(-1, 1, (2, 4))
    v, cot = rng.uniform(-1, 1, (2, 10)), rng.uniform(-1, 1, (2, 10))
    jv = dn.vee_rows(n, lg, v, rg, b, og_)
    jt = dn.vee_rows_transposed(n, lg, rg, og_, cot, b, wrt_left=True)
    assert np.allclose((cot * jv).sum(), (jt * v).sum(), rtol=1e-13)
    w = rng.uniform(-1, 1, (2, 4))
    jw = dn.vee_rows(n, lg, a, rg, w, og_)
    jt = dn.vee_rows_transposed(n, lg, rg, og_, cot, a, wrt_left=False)
    assert np.allclose((cot * jw).sum(), (jt * w).sum(), rtol=1e-13)
    x = rng.uniform(-1, 1, (2, 16))
    d, g = dn.complement_rows(n, range(5), x)
    c = rng.uniform(-1, 1, d.shape)
    assert np.allclose((c * d).sum(), (dn.complement_rows(n, g, c, undual=True)[0] * x).sum(), rtol=1e-13)
