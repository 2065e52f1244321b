"""Second-order reverse mode on the host: gaast_program_vjp accepts the programs it emits, to any depth.  The images are checked
for their shape, for the product kinds of the closure table (gaast_expr.h), and -- evaluated by the numpy evaluator of
vjp_numpy.py, not by the library -- against central differences of the image they differentiate.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib
from golden_programs import PROGRAMS
from helpers import HipBackend
from vjp_numpy import eval_desc
import test_vjp_host as H

G, L, R = _lib.PROD_GEOMETRIC, _lib.PROD_ADJ_LEFT, _lib.PROD_ADJ_RIGHT
PGA3D = [0.0, 1.0, 1.0, 1.0]
_images = []   # kept alive: a desc points into its image


def _image(d, slot):
    """(status, desc or None) of gaast_program_vjp; the image lives as long as the module."""
    st, img = H._vjp(d, slot)
    if st:
        assert not img.value
        return st, None
    _images.append(img)
    return 0, _lib.lib().gaast_program_image_desc(img).contents


def _ok(d, slot):
    st, a = _image(d, slot)
    assert st == 0, (slot, _lib.lib().gaast_expr_last_error())
    return a


def _check_shape(d, slot, a):
    """The conditions of test_vjp_host.test_adjoint_program_shape, for any program d (forward or VJP) and its image a."""
    root = d.nodes[d.root]
    for i in range(a.n_nodes):
        nd = a.nodes[i]
        if nd.opcode == _lib.OP_INPUT:
            assert 0 <= nd.input_slot < a.n_inputs
        else:
            assert 0 <= nd.child0 < i
            if nd.opcode in (_lib.OP_ADD, _lib.OP_PRODUCT, _lib.OP_EXP_ADJ, _lib.OP_LOG_ADJ, _lib.OP_GEXP_ADJ, _lib.OP_GSQRT_ADJ,
                             _lib.OP_GLOG_ADJ):
                assert 0 <= nd.child1 < i
    assert 0 <= a.root < a.n_nodes
    assert a.n_inputs in (d.n_inputs + 1, d.n_inputs + 2)
    for s in range(d.n_inputs):
        assert (a.inputs[s].grade_mask, a.inputs[s].storage_dim, a.inputs[s].is_const) == \
            (d.inputs[s].grade_mask, d.inputs[s].storage_dim, d.inputs[s].is_const)
        if d.inputs[s].is_const:
            n = H._row_len(d.inputs[s].storage_dim, d.inputs[s].grade_mask)
            assert [a.inputs[s].const_row[i] for i in range(n)] == [d.inputs[s].const_row[i] for i in range(n)]
    cot = a.inputs[d.n_inputs]
    assert (cot.grade_mask, cot.storage_dim, cot.is_const) == (root.minimal_grade_mask, d.vec_space_dim, 0)
    if a.n_inputs == d.n_inputs + 2:
        one = a.inputs[d.n_inputs + 1]
        assert (one.grade_mask, one.is_const, one.const_row[0]) == (1, 1, 1.0)
    r = a.nodes[a.root]
    assert r.minimal_grade_mask == d.inputs[slot].grade_mask
    assert r.vec_space_dim == d.inputs[slot].storage_dim
    assert a.flags == d.flags


def _r6_gp(B):
    return B.input(0, list(range(7)), 6) * B.input(1, list(range(7)), 6)


CLOSURE = [(name, metric, build, {}) for name, metric, build in H.CASES_ALL] + \
          [(name + "_compact", metric, build, dict(materialize_limit=1)) for name, metric, build in H.CASES_ALL] + \
          [("r6_gp", 6, _r6_gp, {}), ("r6_gp_compact", 6, _r6_gp, dict(materialize_limit=1))]


@pytest.mark.parametrize("name,metric,build,kw", CLOSURE, ids=[c[0] for c in CLOSURE])
def test_every_first_order_image_differentiates_in_every_slot(name, metric, build, kw):
    spec = H._spec(build, metric, **kw)
    d = spec.program_desc()
    for s1 in H._user_slots(d):
        a = _ok(d, s1)
        _check_shape(d, s1, a)
        slots = H._user_slots(a)
        assert d.n_inputs in slots, "the cotangent is a slot like any other"
        for s2 in slots:
            a2 = _ok(a, s2)
            _check_shape(a, s2, a2)
        for s in range(a.n_inputs):
            if a.inputs[s].is_const:
                st, _ = _image(a, s)
                assert _lib.STATUS_NAMES[st] == "INVALID_ARGUMENT"


def _product_kinds(a):
    """(kind, has a list) of every PRODUCT node"""
    return [(a.nodes[i].product_kind, bool(a.nodes[i].comp_muls)) for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_PRODUCT]


def _compact(a):
    return [(i, a.nodes[i]) for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_PRODUCT and not a.nodes[i].comp_muls]


def _slot_of(a, i):
    """the input slot a node reads: a bare input, or its copy (an explicit product with the constant 1: a projection)"""
    nd = a.nodes[i]
    if nd.opcode == _lib.OP_PRODUCT and nd.comp_muls and a.nodes[nd.child1].opcode == _lib.OP_INPUT and \
            a.inputs[a.nodes[nd.child1].input_slot].is_const:
        return _slot_of(a, nd.child0)
    return nd.input_slot if nd.opcode == _lib.OP_INPUT else None


def _binary(kind, n, g0, g1):
    def build(B):
        a, b = B.input(0, g0, n), B.input(1, g1, n)
        return {0: lambda: a * b, 1: lambda: a ^ b, 2: lambda: a & b, 3: lambda: a << b, 4: lambda: a >> b, 5: lambda: a.vee(b)}[kind]()
    return build


@pytest.mark.parametrize("kind", range(6))
def test_compact_product_kinds_follow_the_closure_table(kind):
    # a o b, slots (a, b) = (0, 1); the first cotangent g is slot 2, the second cotangent h slot 3, or 4 after a const 1 where
    # a cotangent has to be projected to a node's grades
    n = 4
    full = list(range(n + 1))
    d = H._desc(_binary(kind, n, full, full), [1.0, -1.0, 2.0, 0.0], materialize_limit=1)
    assert _product_kinds(d) == [(kind, False)]
    # first order: (kind, children's slots) -- the table's left column
    first = {0: (L + kind, (2, 1)), 1: (R + kind, (2, 0))}
    # second order, from the table: first slot -> {second slot: (kind, children's slots)}
    second = {0: {2: (kind, ("h", 1)), 1: (R + kind, (2, "h"))},
              1: {2: (kind, (0, "h")), 0: (L + kind, (2, "h"))}}
    for s1 in (0, 1):
        a = _ok(d, s1)
        assert a.n_inputs in (3, 4)
        h_slot = a.n_inputs
        (i, nd), = _compact(a)
        assert (nd.product_kind, (_slot_of(a, nd.child0), _slot_of(a, nd.child1))) == first[s1]
        for s2 in (0, 1, 2):
            a2 = _ok(a, s2)
            if s2 == s1:   # the first image does not read the slot it differentiates: zero rows
                assert not _compact(a2)
                continue
            (i, nd), = _compact(a2)
            want_kind, want_slots = second[s1][s2]
            assert (nd.product_kind, (_slot_of(a2, nd.child0), _slot_of(a2, nd.child1))) == \
                (want_kind, tuple(h_slot if w == "h" else w for w in want_slots)), (s1, s2)
            assert nd.minimal_grade_mask & ~a.inputs[s2].grade_mask == 0
            assert nd.n_comp_muls == d.nodes[d.root].n_comp_muls, "full grade sets: the same list, transposed"
            # third order: still within {kind, L + kind, R + kind}
            for s3 in H._user_slots(a2):
                a3 = _ok(a2, s3)
                _check_shape(a2, s3, a3)
                assert {k for k, _ in _product_kinds(a3) if k >= 0} <= {kind, L + kind, R + kind}


def test_compact_geometric_product_differentiated_twice_at_n6():
    for kw in ({}, dict(materialize_limit=1)):   # an explicit forward list at n = 6 gets compact adjoints as well
        d = H._desc(_r6_gp, 6, **kw)
        for s1 in (0, 1):
            a = _ok(d, s1)
            for s2 in H._user_slots(a):
                a2 = _ok(a, s2)
                for k, has_list in _product_kinds(a2):
                    assert has_list or k in (G, L + G, R + G), (s1, s2, k)
                if s2 != s1:
                    assert {(0, 2): G, (0, 1): R + G, (1, 2): G, (1, 0): L + G}[(s1, s2)] in [k for k, has_list in _product_kinds(a2) if not has_list]


def _inv_times(B):
    return B.input(0, [0, 2, 4], 4).inv() * B.input(1, [1], 4)


def test_inv_differentiates_in_every_pair_of_slots():
    d = H._desc(_inv_times, PGA3D)
    for s1 in (0, 1):
        a = _ok(d, s1)
        _check_shape(d, s1, a)
        assert any(a.nodes[i].opcode == _lib.OP_INV for i in range(a.n_nodes))
        for s2 in H._user_slots(a):
            a2 = _ok(a, s2)
            _check_shape(a, s2, a2)
            for s3 in H._user_slots(a2):
                _check_shape(a2, s3, _ok(a2, s3))


# ---- numbers ------------------------------------------------------------------------------------------------------------
def _explicit_only(d):
    return all(d.nodes[i].comp_muls for i in range(d.n_nodes) if d.nodes[i].opcode == _lib.OP_PRODUCT) and \
        all(d.nodes[i].opcode <= _lib.OP_SSQRT and d.nodes[i].opcode not in (_lib.OP_EXP, _lib.OP_LOG) for i in range(d.n_nodes))


def _check_image_against_differences(d, slot, rng, lo=-1.0, h=1e-5, tol=1e-6, n_dirs=3):
    """The form and constants of test_vjp_host._check_against_differences, for any program d (here a VJP image) and with a lower
    end of the inputs' range that keeps a program with 1 / |v|^2 away from its pole."""
    rows = {s: rng.uniform(lo, 1.0, H._row_len(d.inputs[s].storage_dim, d.inputs[s].grade_mask)) for s in H._user_slots(d)}
    root = d.nodes[d.root]
    g = rng.uniform(-1.0, 1.0, H._row_len(root.vec_space_dim, root.minimal_grade_mask))
    grad = eval_desc(_ok(d, slot), {**rows, d.n_inputs: g})
    for _ in range(n_dirs):
        v = rng.uniform(-1.0, 1.0, rows[slot].shape)
        plus = eval_desc(d, {**rows, slot: rows[slot] + h * v})
        minus = eval_desc(d, {**rows, slot: rows[slot] - h * v})
        fd = float(g @ (plus - minus)) / (2 * h)
        an = float(grad @ v)
        assert abs(fd - an) <= tol * (1.0 + abs(an) + float(np.abs(g) @ np.abs(plus + minus)) / 2), (slot, fd, an)


def _pga3d_sandwich(B):
    M, X = B.input(0, [0, 2, 4], 4), B.input(1, [3], 4)
    return M * X * M.rev()


def _vee(B):
    return B.input(0, [1, 3], 4).vee(B.input(1, [2, 3], 4)) * B.input(0, [1, 3], 4)


def _vinv(B):
    v = B.input(0, [1], 4)
    return v.vinv() * B.input(1, [0, 2], 4)


# polynomials of degree <= 3 on [-1, 1]: truncation ~ h^2, rounding ~ eps / h, both below 1e-9.  sta_inverse and vinv divide by
# |v|^2: vinv is checked in a Euclidean metric on [0.5, 1], where |v|^2 >= 1 keeps every derivative of order one
NUMERIC = [("golden_" + name, p["metric"], p["build"], -1.0) for name, p in PROGRAMS.items() if name != "sta_inverse"] + \
          [("pga3d_sandwich", PGA3D, _pga3d_sandwich, -1.0), ("vee", PGA3D, _vee, -1.0), ("vinv", 4, _vinv, 0.5)]


@pytest.mark.parametrize("name,metric,build,lo", NUMERIC, ids=[c[0] for c in NUMERIC])
def test_second_order_image_matches_central_differences_of_the_first(name, metric, build, lo):
    d = H._desc(build, metric)
    rng = np.random.default_rng(sum(map(ord, name)))
    checked = 0
    for s1 in H._user_slots(d):
        a = _ok(d, s1)
        if not _explicit_only(a):
            continue
        for s2 in H._user_slots(a):
            _check_image_against_differences(a, s2, rng, lo=lo)
            checked += 1
    assert checked, "an explicit-list program"


def test_third_order_image_of_the_pga3d_sandwich():
    d = H._desc(_pga3d_sandwich, PGA3D)
    rng = np.random.default_rng(33)
    a = _ok(d, 0)       # d/dM: quadratic in (M, X, g) -> the third-order images are not all zero
    a2 = _ok(a, 1)      # then d/dX
    assert _explicit_only(a2)
    for s3 in H._user_slots(a2):
        _check_image_against_differences(a2, s3, rng)
    # something is left at third order: d^3 <g, M X ~M> / dM dX dM
    a3 = _ok(a2, 0)
    rows = {s: rng.uniform(-1.0, 1.0, H._row_len(a2.inputs[s].storage_dim, a2.inputs[s].grade_mask)) for s in H._user_slots(a2)}
    root = a2.nodes[a2.root]
    k = rng.uniform(-1.0, 1.0, H._row_len(root.vec_space_dim, root.minimal_grade_mask))
    assert np.abs(eval_desc(a3, {**rows, a2.n_inputs: k})).max() > 1e-3


# ---- adjoint op nodes ---------------------------------------------------------------------------------------------------
ADJ_OPS = [("gexp", "GAAST_OP_GEXP_ADJ", _lib.OP_GEXP_ADJ, 0), ("gsqrt", "GAAST_OP_GSQRT_ADJ", _lib.OP_GSQRT_ADJ, 0),
           ("glog", "GAAST_OP_GLOG_ADJ", _lib.OP_GLOG_ADJ, 0),
           ("exp", "GAAST_OP_EXP_ADJ", _lib.OP_EXP_ADJ, ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD)]


@pytest.mark.parametrize("fn,opname,opcode,flags", ADJ_OPS, ids=[c[0] for c in ADJ_OPS])
def test_adjoint_op_nodes_are_carried_or_refused_by_name(fn, opname, opcode, flags):
    grades = [2] if fn == "exp" else [0, 2]

    def build(B):
        return getattr(B.input(0, grades, 3), fn)() * B.input(1, grades, 3)
    d = H._desc(build, 3, flags=flags)
    # with respect to x the adjoint node is the image: every slot that reaches it is refused, by name
    a = _ok(d, 0)
    ops = [a.nodes[i].opcode for i in range(a.n_nodes)]
    assert opcode in ops
    node = ops.index(opcode)
    reach = {s: _reaches(a, node, s) for s in H._user_slots(a)}
    assert reach[0] and reach[d.n_inputs], "the forward operand and the cotangent"
    for s, on_path in reach.items():
        st, a2 = _image(a, s)
        if on_path:
            assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED", (s, st)
            msg = _lib.lib().gaast_expr_last_error().decode()
            assert opname in msg and "second-order" in msg, msg
        else:
            assert st == 0
    # with respect to y the forward gexp is an operand only: the second image with respect to x carries the adjoint node, and
    # that image differentiates where the node is off the path
    b = _ok(d, 1)
    assert opcode not in [b.nodes[i].opcode for i in range(b.n_nodes)]
    for s in H._user_slots(b):
        b2 = _ok(b, s)
        _check_shape(b, s, b2)
    b2 = _ok(b, 0)
    ops = [b2.nodes[i].opcode for i in range(b2.n_nodes)]
    assert opcode in ops
    node = ops.index(opcode)
    for s in H._user_slots(b2):
        st, b3 = _image(b2, s)
        if _reaches(b2, node, s):
            assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
            assert opname in _lib.lib().gaast_expr_last_error().decode()
        else:
            assert st == 0
            _check_shape(b2, s, b3)
    # off the path the node is carried along untouched: z -> a(x, y, g) * z with one more input z (built by hand)
    even = 0b101
    node = [a.nodes[j].opcode for j in range(a.n_nodes)].index(opcode)
    nodes = (_lib.NodeDesc * (a.n_nodes + 2))(*[a.nodes[j] for j in range(a.n_nodes)])
    z = nodes[a.n_nodes]
    z.opcode, z.child0, z.child1, z.minimal_grade_mask, z.vec_space_dim, z.input_slot, z.product_kind = _lib.OP_INPUT, -1, -1, even, 3, a.n_inputs, -1
    pr = nodes[a.n_nodes + 1]
    pr.opcode, pr.child0, pr.child1, pr.minimal_grade_mask, pr.vec_space_dim, pr.input_slot, pr.product_kind = \
        _lib.OP_PRODUCT, a.root, a.n_nodes, even, 3, -1, G
    pr.n_comp_muls = 16
    inputs = (_lib.InputDesc * (a.n_inputs + 1))(*[a.inputs[j] for j in range(a.n_inputs)])
    inputs[a.n_inputs].grade_mask, inputs[a.n_inputs].storage_dim, inputs[a.n_inputs].is_const = even, 3, 0
    c = _lib.ProgramDesc()
    C.memmove(C.byref(c), C.byref(a), C.sizeof(c))
    c.nodes, c.n_nodes, c.root, c.inputs, c.n_inputs = nodes, a.n_nodes + 2, a.n_nodes + 1, inputs, a.n_inputs + 1
    cz = _ok(c, a.n_inputs)
    _check_shape(c, a.n_inputs, cz)
    kept = [cz.nodes[i] for i in range(cz.n_nodes) if cz.nodes[i].opcode == opcode]
    assert len(kept) == 1
    assert (kept[0].child0, kept[0].child1, kept[0].minimal_grade_mask) == (a.nodes[node].child0, a.nodes[node].child1, a.nodes[node].minimal_grade_mask)
    st, _ = _image(c, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED" and opname in _lib.lib().gaast_expr_last_error().decode()


def _reaches(a, node, slot):
    """does `node` read input `slot`, through either child?"""
    nd = a.nodes[node]
    if nd.opcode == _lib.OP_INPUT:
        return nd.input_slot == slot
    return _reaches(a, nd.child0, slot) or (nd.child1 >= 0 and _reaches(a, nd.child1, slot))


def test_other_product_kinds_above_7_stay_invalid():
    d = H._desc(_binary(0, 4, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]), 4, materialize_limit=1)
    a = _ok(d, 0)
    (i, _), = _compact(a)
    nodes = (_lib.NodeDesc * a.n_nodes)(*[a.nodes[j] for j in range(a.n_nodes)])
    bad = _lib.ProgramDesc()
    C.memmove(C.byref(bad), C.byref(a), C.sizeof(bad))
    bad.nodes = nodes
    for kind in (L + R, L + 6, L + 7, R + 6, R + 7, 32, 32 + L):
        nodes[i].product_kind = kind
        for s in (0, 1, 2):
            st, _ = _image(bad, s)
            assert _lib.STATUS_NAMES[st] == "INVALID_PROGRAM", (kind, s)
    nodes[i].product_kind = L + G
    assert _image(bad, 1)[0] == 0


# ---- JVP image, wire format, first order unchanged -----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_jvp_image_never_reads_the_first_cotangent(name):
    p = PROGRAMS[name]
    d = H._desc(p["build"], p["metric"])
    for slot in H._user_slots(d):
        a = _ok(d, slot)
        j = _ok(a, d.n_inputs)
        assert not any(j.nodes[i].opcode == _lib.OP_INPUT and j.nodes[i].input_slot == d.n_inputs for i in range(j.n_nodes))
        r = j.nodes[j.root]
        assert (r.minimal_grade_mask, r.vec_space_dim) == (d.nodes[d.root].minimal_grade_mask, d.vec_space_dim)


def _serialize(a):
    n = _lib.lib().gaast_program_serialize(C.byref(a), None, 0)
    buf = (C.c_ubyte * n)()
    assert _lib.lib().gaast_program_serialize(C.byref(a), buf, n) == n
    return bytes(buf)


def test_second_order_image_round_trips_through_the_wire_format():
    d = H._desc(_binary(0, 4, [0, 1, 2, 3, 4], [1, 2]), [1.0, -1.0, 2.0, 0.0], materialize_limit=1)
    a2 = _ok(_ok(d, 0), 1)
    kinds = [k for k, _ in _product_kinds(a2)]
    assert R + G in kinds
    data = _serialize(a2)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    img = C.c_void_p(_lib.lib().gaast_program_deserialize(buf, len(data)))
    assert img.value
    try:
        b = _lib.lib().gaast_program_image_desc(img).contents
        assert _serialize(b) == data
        assert [k for k, _ in _product_kinds(b)] == kinds
    finally:
        _lib.lib().gaast_program_image_free(img)


def test_first_order_images_are_unchanged_by_a_second_differentiation():
    before, after = {}, {}
    descs = {name: H._desc(p["build"], p["metric"]) for name, p in PROGRAMS.items()}
    for name, d in descs.items():
        for slot in H._user_slots(d):
            before[name, slot] = _serialize(_ok(d, slot))
    for name, d in descs.items():
        for slot in H._user_slots(d):
            a = _ok(d, slot)
            for s2 in H._user_slots(a):
                _ok(a, s2)
    for name, d in descs.items():
        for slot in H._user_slots(d):
            after[name, slot] = _serialize(_ok(d, slot))
    assert before == after
