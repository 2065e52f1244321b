"""Reverse mode on the host: gaast_program_vjp builds valid adjoint programs, and (evaluated by the numpy evaluator of
vjp_numpy.py, not by the library) they agree with central differences of the forward program.  No GPU."""
import ctypes as C
import math
from collections import Counter

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib
from exprs import CASES
from golden_programs import PROGRAMS
from helpers import HipBackend
from vjp_numpy import eval_desc


def _spec(build, metric, **kw):
    return build(HipBackend()).specialize(metric, **kw)


_alive = []


def _desc(build, metric, **kw):
    """The flat program of a specialised build (the spec, which owns the arrays, is kept alive)."""
    spec = _spec(build, metric, **kw)
    _alive.append(spec)
    return spec.program_desc()


def _cases():
    # the programs of exprs.CASES over at least one input slot (most hold fixed values only), and the golden programs
    out = []
    for name, (metric, build) in CASES.items():
        b = (lambda f: (lambda B: f(B, np.random.default_rng(7))))(build)
        if _spec(b, metric).num_user_inputs():
            out.append((name, metric, b))
    for name, p in PROGRAMS.items():
        out.append(("golden_" + name, p["metric"], p["build"]))
    return out


CASES_ALL = _cases()


def _vjp(d, slot):
    img = C.c_void_p()
    st = _lib.lib().gaast_program_vjp(C.byref(d), slot, C.byref(img))
    return st, img


def _row_len(dim, mask):
    return sum(math.comb(dim, k) for k in range(64) if (mask >> k) & 1)


def _user_slots(d):
    return [s for s in range(d.n_inputs) if not d.inputs[s].is_const]


@pytest.mark.parametrize("name,metric,build", CASES_ALL, ids=[c[0] for c in CASES_ALL])
def test_adjoint_program_shape(name, metric, build):
    spec = _spec(build, metric)
    d = spec.program_desc()
    root = d.nodes[d.root]
    for slot in _user_slots(d):
        st, img = _vjp(d, slot)
        assert st == 0, _lib.lib().gaast_expr_last_error()
        try:
            a = _lib.lib().gaast_program_image_desc(img).contents
            # valid post-order, root last reached
            for i in range(a.n_nodes):
                nd = a.nodes[i]
                if nd.opcode == _lib.OP_INPUT:
                    assert 0 <= nd.input_slot < a.n_inputs
                else:
                    assert 0 <= nd.child0 < i
                    if nd.opcode in (_lib.OP_ADD, _lib.OP_PRODUCT):
                        assert 0 <= nd.child1 < i
            assert 0 <= a.root < a.n_nodes
            # forward inputs unchanged, cotangent at slot n_inputs
            assert a.n_inputs in (d.n_inputs + 1, d.n_inputs + 2)
            for s in range(d.n_inputs):
                assert (a.inputs[s].grade_mask, a.inputs[s].storage_dim, a.inputs[s].is_const) == \
                    (d.inputs[s].grade_mask, d.inputs[s].storage_dim, d.inputs[s].is_const)
            cot = a.inputs[d.n_inputs]
            assert (cot.grade_mask, cot.storage_dim, cot.is_const) == (root.minimal_grade_mask, d.vec_space_dim, 0)
            # output in the layout of the input
            r = a.nodes[a.root]
            assert r.minimal_grade_mask == d.inputs[slot].grade_mask
            assert r.vec_space_dim == d.inputs[slot].storage_dim
            assert a.flags == d.flags
        finally:
            _lib.lib().gaast_program_image_free(img)


def _explicit_lists(d):
    out = []
    for i in range(d.n_nodes):
        nd = d.nodes[i]
        if nd.opcode == _lib.OP_PRODUCT and nd.comp_muls:
            out.append([(m.left_grade, m.left_index, m.right_grade, m.right_index, m.result_grade, m.result_index, m.coeff)
                        for m in nd.comp_muls[:nd.n_comp_muls]])
    return out


def test_explicit_adjoint_lists_are_the_transposed_forward_list():
    # a single product of two inputs: the adjoint's one list is the forward list transposed, ordered stably by result
    for kind in range(5):
        def build(B, kind=kind):
            a, b = B.input(0, [0, 1, 2, 3, 4], 4), B.input(1, [1, 2], 4)
            return {0: a * b, 1: a ^ b, 2: a & b, 3: a << b, 4: a >> b}[kind]
        d = _desc(build, [1.0, -1.0, 2.0, 0.0])
        fwd = _explicit_lists(d)[0]
        for slot, key in ((0, lambda m: (m[4], m[5], m[2], m[3], m[0], m[1], m[6])),
                          (1, lambda m: (m[0], m[1], m[4], m[5], m[2], m[3], m[6]))):
            st, img = _vjp(d, slot)
            assert st == 0
            a = _lib.lib().gaast_program_image_desc(img).contents
            adj = [l for l in _explicit_lists(a) if len(l) == len(fwd)]
            assert len(adj) == 1, "one transposed list"
            assert Counter(adj[0]) == Counter(key(m) for m in fwd)
            res = [(m[4], m[5]) for m in adj[0]]
            assert res == sorted(res)
            # stable: forward order within one result component
            want = sorted((key(m) for m in fwd), key=lambda m: (m[4], m[5]))
            assert adj[0] == want
            _lib.lib().gaast_program_image_free(img)


def _check_against_differences(spec, d, slot, rng, h=1e-5, tol=1e-6, n_dirs=3):
    rows = {s: rng.uniform(-1.0, 1.0, _row_len(d.inputs[s].storage_dim, d.inputs[s].grade_mask)) for s in _user_slots(d)}
    root = d.nodes[d.root]
    g = rng.uniform(-1.0, 1.0, _row_len(root.vec_space_dim, root.minimal_grade_mask))
    st, img = _vjp(d, slot)
    assert st == 0, _lib.lib().gaast_expr_last_error()
    a = _lib.lib().gaast_program_image_desc(img).contents
    grad = eval_desc(a, {**rows, d.n_inputs: g})
    _lib.lib().gaast_program_image_free(img)
    for _ in range(n_dirs):
        v = rng.uniform(-1.0, 1.0, rows[slot].shape)
        plus = eval_desc(d, {**rows, slot: rows[slot] + h * v})
        minus = eval_desc(d, {**rows, slot: rows[slot] - h * v})
        fd = float(g @ (plus - minus)) / (2 * h)
        an = float(grad @ v)
        assert abs(fd - an) <= tol * (1.0 + abs(an) + float(np.abs(g) @ np.abs(plus + minus)) / 2), (fd, an)


@pytest.mark.parametrize("name,metric,build", CASES_ALL, ids=[c[0] for c in CASES_ALL])
def test_adjoint_matches_central_differences(name, metric, build):
    spec = _spec(build, metric)
    d = spec.program_desc()
    rng = np.random.default_rng(abs(hash(name)) % 2**32)
    for slot in _user_slots(d):
        _check_against_differences(spec, d, slot, rng)


def test_in_place_semantics_of_sub_and_scalar_ops():
    # a - b evaluates to -(a + b) (eval.rs:55-60 negates the whole buffer); sinv / sqrt act on what was accumulated before them
    def sub(B):
        return B.input(0, [0, 1], 3) - B.input(1, [0, 1], 3)

    def scalar_chain(B):
        a, b, c = B.input(0, [0], 3), B.input(1, [0, 2], 3), B.input(2, [0], 3)
        return (a + c.sinv() + c).sqrt() * b + (b * b).g(0).sinv()
    rng = np.random.default_rng(3)
    for build in (sub, scalar_chain):
        spec = _spec(build, 3)
        d = spec.program_desc()
        for slot in _user_slots(d):
            rows = {s: rng.uniform(0.5, 1.0, _row_len(d.inputs[s].storage_dim, d.inputs[s].grade_mask)) for s in _user_slots(d)}
            root = d.nodes[d.root]
            g = rng.uniform(-1.0, 1.0, _row_len(root.vec_space_dim, root.minimal_grade_mask))
            st, img = _vjp(d, slot)
            assert st == 0
            grad = eval_desc(_lib.lib().gaast_program_image_desc(img).contents, {**rows, d.n_inputs: g})
            _lib.lib().gaast_program_image_free(img)
            h = 1e-6
            for i in range(rows[slot].size):
                e = np.zeros_like(rows[slot])
                e[i] = h
                fd = float(g @ (eval_desc(d, {**rows, slot: rows[slot] + e}) - eval_desc(d, {**rows, slot: rows[slot] - e}))) / (2 * h)
                assert abs(fd - grad[i]) <= 1e-6 * (1 + abs(fd)), (build.__name__, slot, i, fd, grad[i])


def test_errors():
    def build(B):
        return B.input(0, [1], 3) * B.input(1, [1], 3) * B.scalar(2.0)
    d = _desc(build, 3)
    const_slot = next(s for s in range(d.n_inputs) if d.inputs[s].is_const)
    for slot in (-1, d.n_inputs, const_slot):
        st, img = _vjp(d, slot)
        assert _lib.STATUS_NAMES[st] == "INVALID_ARGUMENT"
        assert not img.value
    # exp / log on the path: unimplemented; off the path: fine
    def explog(B):
        x, y = B.input(0, [2], 3), B.input(1, [2], 3)
        return x.exp() * y
    d = _desc(explog, 3, flags=ga.FLAG_EXP_LOG)
    st, img = _vjp(d, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
    st, img = _vjp(d, 1)
    assert st == 0
    _lib.lib().gaast_program_image_free(img)
    d = _desc(lambda B: B.input(0, [1], 3) * B.input(1, [1], 3), 3, flags=ga.FLAG_SPINOR_GEMM)
    st, _ = _vjp(d, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"


def test_compact_adjoint_kinds_round_trip_through_the_wire_format():
    build = lambda B: B.input(0, [0, 1, 2, 3, 4], 4) * B.input(1, [0, 1, 2, 3, 4], 4)
    d = _desc(build, 4, materialize_limit=1)
    for slot, kind in ((0, _lib.PROD_ADJ_LEFT), (1, _lib.PROD_ADJ_RIGHT)):
        st, img = _vjp(d, slot)
        assert st == 0
        a = _lib.lib().gaast_program_image_desc(img).contents
        kinds = [a.nodes[i].product_kind for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_PRODUCT]
        assert kind + _lib.PROD_GEOMETRIC in kinds
        n = _lib.lib().gaast_program_serialize(C.byref(a), None, 0)
        buf = (C.c_ubyte * n)()
        assert _lib.lib().gaast_program_serialize(C.byref(a), buf, n) == n
        img2 = C.c_void_p(_lib.lib().gaast_program_deserialize(buf, n))
        a2 = _lib.lib().gaast_program_image_desc(img2).contents
        buf2 = (C.c_ubyte * n)()
        assert _lib.lib().gaast_program_serialize(C.byref(a2), buf2, n) == n
        assert bytes(buf) == bytes(buf2)
        assert [a2.nodes[i].product_kind for i in range(a2.n_nodes) if a2.nodes[i].opcode == _lib.OP_PRODUCT] == kinds
        _lib.lib().gaast_program_image_free(img2)
        _lib.lib().gaast_program_image_free(img)
