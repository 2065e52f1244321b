"""Complements (dual / undual) and the regressive product on the GPU, against the numpy reference of dual_numpy.py.

Conventions of the cases.  The join is taken in plane-based PGA3D (n = 4, diag [0, 1, 1, 1]: planes are vectors, points
trivectors): (p1 v p2) v p3 of three points is a vector, the plane through them.  In that model the meet of two planes is the OUTER
product and `vector v vector` is empty at n = 4 (tests/test_dual_host.py), so the "meet" case here is the meet of the POINT-based
model on the same algebra, where planes are trivectors: pl1 v pl2 is a bivector, their line.  In CGA (n = 5, null basis) spheres
are 4-vectors: the meet of two is a trivector, and the join of four dual points ((p1 v p2) v p3) v p4 a vector.

Bounds.  A complement is a signed permutation: bits.  A regressive program, chained or not: the project's contract, 4 eps A per
component, A = sum |terms| of the last product evaluated over the sum |terms| of the product that made its operand (for the PGA3D
join: two terms per component, then three, coefficients +-1).  With a Gram basis the rows also go through the compounds of an
orthogonal Q on the way in and out; the existing Gram tests' norm-wise bound is used there (TOL * product of the operands' norms,
tests/test_gpu_gram_metric.py)."""
import numpy as np
import pytest

import gaast_amd as ga

import dual_numpy as dn
from layouts import BITS, NP, layouts_of, place, place_out

pytestmark = pytest.mark.gpu

EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
GRAM_TOL = {ga.F64: 1e-12, ga.F32: 2e-5}     # tests/test_gpu_gram_metric.py: TOL
PGA = [0.0, 1.0, 1.0, 1.0]
DTYPES = [ga.F64, ga.F32]
_REF = {}


def inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def rows_for(seed, n, grades, batch, dtype):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, len(dn.row_blades(n, grades)))).astype(NP[dtype])


def bits(a, dtype):
    return np.ascontiguousarray(a, dtype=NP[dtype]).view(BITS[dtype])


def run(spec, rows, batch):
    out = spec.eval_batch(rows, batch)
    ga.lib().gaast_hip_synchronize()
    return out.download_rows()


# ---- complements, bit-exact ---------------------------------------------------------------------------------------------------
SIZES = [(4, 257), (9, 67), (12, 5)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["direct", "interior", "shared"])
@pytest.mark.parametrize("undual", [False, True], ids=["dual", "undual"])
@pytest.mark.parametrize("n,batch", SIZES)
def test_complements_are_bit_exact(n, batch, undual, form, dtype):
    grades = list(range(n + 1)) if n != 4 else [0, 1, 3, 4]     # (PGA3D: a row that is not the full multivector)
    metric = PGA if n == 4 else [1.0] * n
    op = (lambda e: e.undual()) if undual else (lambda e: e.dual())
    x = rows_for(n, n, grades, 1 if form == "shared" else batch, dtype)
    if form == "interior":
        y = rows_for(n + 100, n, grades, batch, dtype)
        spec = op(inp(0, grades, n) + inp(1, grades, n)).specialize(metric, dtype=dtype)
        got = run(spec, [x, y], batch)
        operand = (NP[dtype](0) + x) + y                          # the cache buffer: zero fill, add_grades_from twice
    else:
        spec = op(inp(0, grades, n)).specialize(metric, dtype=dtype)
        got = run(spec, [x], batch)
        operand = np.repeat(x, batch, axis=0) if form == "shared" else x
    want, out_grades = dn.complement_rows(n, grades, operand, undual=undual)
    assert np.abs(want).max() > 0.5 and np.count_nonzero(want) == want.size      # the reference is not zero
    assert [k for k in range(n + 1) if (spec.output_info()[0] >> k) & 1] == out_grades
    assert np.array_equal(bits(got, dtype), bits(want, dtype))
    names = spec.launches()
    if n >= 9:
        assert any("k_dual<" in l for l in names), names
    else:
        assert len(names) == 1 and names[0].startswith("ast_jit"), names


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [ga.FLAG_NO_FUSION, ga.FLAG_NO_JIT, ga.FLAG_DEBUG_JIT_FAILS, ga.FLAG_EXACT_ORDER], ids=["no_fusion", "no_jit", "jit_fails", "exact"])
def test_small_complement_programs_under_the_plan_flags(flags, dtype):
    """undual(dual(a) ^ dual(b)) -- the regressive product spelt out -- and the scalar literal, at n = 4"""
    n, batch = 4, 257
    a, b = rows_for(1, n, [3], batch, dtype), rows_for(2, n, [3], batch, dtype)
    spec = (inp(0, [3], n).dual() ^ inp(1, [3], n).dual()).undual().specialize(PGA, dtype=dtype, flags=flags)
    got = run(spec, [a, b], batch)
    want = dn.vee_rows(n, [3], a, [3], b, [2], sequential=True)
    assert np.abs(want).max() > 0.3
    # one rounding per product term and exact complements: the outer product's two terms per component add in list order
    assert np.abs(got.astype(np.float64) - dn.vee_rows(n, [3], a, [3], b, [2])).max() <= 4 * EPS[dtype] * dn.vee_rows(n, [3], a, [3], b, [2], absolute=True).max()
    if flags & ga.FLAG_NO_FUSION:
        assert sum("k_dual<" in l for l in spec.launches()) == 3, spec.launches()
    elif flags & (ga.FLAG_NO_JIT | ga.FLAG_DEBUG_JIT_FAILS):      # still one fused launch: the interpreter's signed add / copy
        assert len(spec.launches()) == 1 and spec.launches()[0].startswith("ast_fused"), spec.launches()
    plain = (inp(0, [3], n).dual() ^ inp(1, [3], n).dual()).undual().specialize(PGA, dtype=dtype)
    assert len(plain.launches()) == 1
    assert np.array_equal(bits(run(plain, [a, b], batch), dtype), bits(got, dtype))
    assert np.array_equal(bits(got, dtype), bits(want, dtype))     # two terms per component: the order cannot matter
    lit = ga.Expr._lift(2.5).dual().specialize(PGA, dtype=dtype, flags=flags)
    assert lit.output_info()[0] == 1 << n
    assert np.array_equal(run(lit, [], 3), np.full((3, 1), 2.5, dtype=NP[dtype]))


FLAG_SETS = [0, ga.FLAG_NO_FUSION, ga.FLAG_NO_JIT, ga.FLAG_DEBUG_JIT_FAILS, ga.FLAG_EXACT_ORDER]


def _with_zeros(seed, n, grades, batch, dtype):
    """random rows in which a third of the components are +0.0 and a third -0.0"""
    x = rows_for(seed, n, grades, batch, dtype)
    pick = np.random.default_rng(seed + 1).integers(0, 3, x.shape)
    x[pick == 1] = 0.0
    x[pick == 2] = -0.0
    return x


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,batch", [(4, 257), (9, 19)])
def test_signed_zeros_have_the_same_bits_in_every_plan(n, batch, dtype):
    """-(a) + dual(b): the complement adds +-(0.0 + b) -- the operand as its cache buffer would hold it -- onto an accumulator that
    holds -0.0 where a is +0.0.  The specialised kernel, the interpreter, the element-wise pass and k_dual agree bit for bit."""
    grades = list(range(n + 1))
    a, b = _with_zeros(3, n, grades, batch, dtype), _with_zeros(5, n, grades, batch, dtype)
    zero = NP[dtype](0)
    want = dn.add_complement(-(zero + a), n, grades, zero + b)
    assert np.signbit(want[want == 0]).any() and (~np.signbit(want[want == 0])).any()     # both zeros occur in the result
    seen = set()
    for flags in FLAG_SETS:
        spec = (-inp(0, grades, n) + inp(1, grades, n).dual()).specialize([1.0] * n, dtype=dtype, flags=flags)
        assert np.array_equal(bits(run(spec, [a, b], batch), dtype), bits(want, dtype)), (flags, spec.launches())
        seen.add(spec.launches()[-1].split("[")[0].split(" ")[0])
    if n == 4:
        assert {"ast_jit", "ast_fused"} <= seen, seen
    else:
        assert "elementwise" in seen, seen
    # dual of a bare input on k_dual (no cache buffer in between): 0.0 + x before the sign
    spec = inp(0, grades, n).dual().specialize([1.0] * n, dtype=dtype, flags=ga.FLAG_NO_JIT if n == 4 else 0)
    got = run(spec, [b], batch)
    assert np.array_equal(bits(got, dtype), bits(dn.complement_rows(n, grades, zero + b)[0], dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_elementwise_pass_absorbs_a_complement(dtype):
    """x + dual(y) - ... at n = 9 (beyond a fused slab): one k_elementwise launch, the complement a statement of the pass"""
    n, batch, grades = 9, 19, list(range(10))
    x, y = rows_for(1, n, grades, batch, dtype), rows_for(2, n, grades, batch, dtype)
    spec = (-(inp(0, grades, n) + inp(1, grades, n).dual())).rev().specialize([1.0] * n, dtype=dtype)
    names = spec.launches()
    assert len(names) == 1 and names[0].startswith("elementwise[") and "k_elementwise<" in names[0], names
    acc = -dn.add_complement(NP[dtype](0) + x, n, grades, NP[dtype](0) + y)
    sign = np.concatenate([np.full(len(dn.blades(n, k)), -1.0 if k % 4 in (2, 3) else 1.0) for k in grades]).astype(NP[dtype])
    assert np.array_equal(bits(run(spec, [x, y], batch), dtype), bits(acc * sign, dtype))
    unfused = (-(inp(0, grades, n) + inp(1, grades, n).dual())).rev().specialize([1.0] * n, dtype=dtype, flags=ga.FLAG_NO_FUSION)
    assert any("k_dual<" in l for l in unfused.launches())
    assert np.array_equal(bits(run(unfused, [x, y], batch), dtype), bits(acc * sign, dtype))


# ---- k_dual on strided, padded and misaligned rows --------------------------------------------------------------------------------
def _layout_cases():
    return [(n, dtype, lay) for n in (7, 9) for dtype in DTYPES for lay in layouts_of(dtype)]


@pytest.mark.parametrize("n,dtype,layout", _layout_cases(), ids=lambda v: str(v))
def test_k_dual_row_layouts(n, dtype, layout):
    batch, grades = 33, list(range(n + 1))
    key = ("layout", n, dtype)
    if key not in _REF:
        x = rows_for(n, n, grades, batch, dtype)
        # n = 7 would be a specialised program: NO_JIT keeps the operand a directly read input and the launch k_dual
        spec = inp(0, grades, n).dual().specialize([1.0] * n, dtype=dtype, flags=ga.FLAG_NO_JIT)
        _REF[key] = (x, spec, dn.complement_rows(n, grades, x)[0])
    x, spec, want = _REF[key]
    assert len(spec.launches()) == 1 and "k_dual<" in spec.launches()[0], spec.launches()
    p = place(x, layout, dtype, n, grades)
    o = place_out(batch, 1 << n, layout, dtype, n, grades)
    spec.eval_batch([p.mv], batch, out=o.mv)
    assert spec.launch_variants() == [0]        # one kernel: scalar accesses take every layout
    p.check()
    o.check()
    assert np.array_equal(bits(o.rows(), dtype), bits(want, dtype))


# ---- PGA3D: join of three points, meet of two planes ------------------------------------------------------------------------------
def _pga_case(name, dtype):
    key = ("pga", name, dtype)
    if key not in _REF:
        n, batch = 4, 1000
        k = 3 if name == "join" else 2
        rows = [rows_for(10 + s, n, [3], batch, dtype) for s in range(k)]
        if name == "join":
            build = lambda: inp(0, [3], n).vee(inp(1, [3], n)).vee(inp(2, [3], n))
            line64 = dn.vee_rows(n, [3], rows[0], [3], rows[1], [2])
            want = dn.vee_rows(n, [2], line64, [3], rows[2], [1])
            bound = 4 * EPS[dtype] * dn.vee_rows(n, [2], dn.vee_rows(n, [3], rows[0], [3], rows[1], [2], absolute=True), [3], rows[2], [1], absolute=True)
            line = dn.vee_rows(n, [3], rows[0], [3], rows[1], [2], sequential=True)
            seq = dn.vee_rows(n, [2], line, [3], rows[2], [1], sequential=True)
        else:
            build = lambda: inp(0, [3], n).vee(inp(1, [3], n))
            want = dn.vee_rows(n, [3], rows[0], [3], rows[1], [2])
            bound = 4 * EPS[dtype] * dn.vee_rows(n, [3], rows[0], [3], rows[1], [2], absolute=True)
            seq = dn.vee_rows(n, [3], rows[0], [3], rows[1], [2], sequential=True)
        assert np.abs(want).max() > 0.5 and (np.abs(want) > 0).all()
        _REF[key] = (rows, build, want, bound, seq)
    return _REF[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["join", "meet"])
def test_pga3d_join_and_meet_are_one_launch(name, dtype):
    rows, build, want, bound, seq = _pga_case(name, dtype)
    spec = build().specialize(PGA, dtype=dtype)
    assert len(spec.launches()) == 1, spec.launches()
    got = run(spec, rows, 1000)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    exact = build().specialize(PGA, dtype=dtype, flags=ga.FLAG_EXACT_ORDER)
    assert len(exact.launches()) == 1
    assert np.array_equal(bits(run(exact, rows, 1000), dtype), bits(seq, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("flags", [ga.FLAG_NO_JIT, ga.FLAG_DEBUG_JIT_FAILS, ga.FLAG_NO_FUSION], ids=["no_jit", "jit_fails", "no_fusion"])
@pytest.mark.parametrize("name", ["join", "meet"])
def test_pga3d_join_and_meet_under_the_plan_flags(name, flags, dtype):
    rows, build, want, bound, _ = _pga_case(name, dtype)
    got = run(build().specialize(PGA, dtype=dtype, flags=flags), rows, 1000)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()


# ---- full multivectors at n = 8: the list path, and no metric factor ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_vee_at_n8_is_metric_free(dtype):
    n, batch, grades = 8, 17, list(range(9))
    a, b = rows_for(81, n, grades, batch, dtype), rows_for(82, n, grades, batch, dtype)
    e = lambda: inp(0, grades, n).vee(inp(1, grades, n))
    euclid = e().specialize([1.0] * n, dtype=dtype)
    odd = e().specialize([1.0, 0.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0], dtype=dtype)
    names = euclid.launches()
    assert euclid.get_node(euclid.root_id()).n_comp_muls == 3 ** 8
    assert len(names) == 1 and "6561 comp-muls" in names[0] and "ast_" not in names[0], names     # a list kernel, not a fused program
    got = run(euclid, [a, b], batch)
    assert np.array_equal(bits(got, dtype), bits(run(odd, [a, b], batch), dtype))
    want = dn.vee_rows(n, grades, a, grades, b, grades)
    assert np.abs(want).max() > 1.0
    assert (np.abs(got.astype(np.float64) - want) <= 4 * EPS[dtype] * dn.vee_rows(n, grades, a, grades, b, grades, absolute=True)).all()


# ---- CGA in its null basis: the orientation sign of the basis change ------------------------------------------------------------
def _cga_grams():
    """{det Q: Gram}: the null basis {e1, e2, e3, e_o, e_inf}, and the same with e_o sheared by e1 (n_o' = e_o + e1), chosen here,
    on the CPU, by the determinant of the Q that gaast_metric_diagonalize returns"""
    g = np.eye(5)
    g[3, 3] = g[4, 4] = 0.0
    g[3, 4] = g[4, 3] = -1.0
    shear = np.eye(5)
    shear[0, 3] = 1.0
    out = {}
    for gram in (g, shear.T @ g @ shear):
        alg = ga.GramAlgebra(gram)
        assert not alg.identity_basis()
        out[int(round(np.linalg.det(alg.basis)))] = alg
    assert sorted(out) == [-1, 1], "the two Gram matrices were meant to give both orientations"
    return out


def _cga_case(name):
    n = 5
    if name == "meet":      # two spheres (4-vectors) -> a circle (trivector)
        return 2, (lambda xs: xs[0].vee(xs[1])), (lambda r: dn.vee_rows(n, [4], r[0], [4], r[1], [3])), [3]
    # four dual points (4-vectors) -> a vector
    def ref(r):
        t = dn.vee_rows(n, [4], r[0], [4], r[1], [3])
        b = dn.vee_rows(n, [3], t, [4], r[2], [2])
        return dn.vee_rows(n, [2], b, [4], r[3], [1])
    return 4, (lambda xs: xs[0].vee(xs[1]).vee(xs[2]).vee(xs[3])), ref, [1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("det", [1, -1], ids=["det_plus", "det_minus"])
@pytest.mark.parametrize("name", ["meet", "join"])
def test_cga_null_basis_meet_and_join(name, det, dtype):
    n, batch = 5, 64
    alg = _cga_grams()[det]
    k, build, ref, out_grades = _cga_case(name)
    rows = [rows_for(50 + s, n, [4], batch, dtype) for s in range(k)]
    want = ref(rows)                       # the regressive product is metric-free: evaluated directly in the caller's basis
    assert np.abs(want).max() > 0.3
    spec = build([inp(s, [4], n) for s in range(k)]).specialize(alg, dtype=dtype)
    assert any(l.startswith("linmap[") for l in spec.launches())
    got = run(spec, rows, batch).astype(np.float64)
    bound = GRAM_TOL[dtype] * np.prod([np.linalg.norm(r, axis=1) for r in rows], axis=0)
    assert (np.linalg.norm(got - want, axis=1) <= bound).all(), np.abs(got - want).max()
    # the complements themselves
    x = rows_for(60, n, [1, 2], batch, dtype)
    for undual in (False, True):
        e = inp(0, [1, 2], n)
        d = run((e.undual() if undual else e.dual()).specialize(alg, dtype=dtype), [x], batch).astype(np.float64)
        w = dn.complement_rows(n, [1, 2], x.astype(np.float64), undual=undual)[0]
        assert (np.linalg.norm(d - w, axis=1) <= GRAM_TOL[dtype] * np.linalg.norm(x, axis=1)).all()


# ---- reverse mode -------------------------------------------------------------------------------------------------------------------
def _adjoint_identity(cot, jv, jt, v, dtype, scale):
    """<cot, J v> == <J^T cot, v>, both sides summed in float64; the slack is the rounding of J^T cot in the dtype"""
    lhs, rhs = float((cot.astype(np.float64) * jv).sum()), float((jt.astype(np.float64) * v.astype(np.float64)).sum())
    assert abs(lhs - rhs) <= scale, (lhs, rhs, scale)
    assert abs(lhs) > 1e-3


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_vjp_of_a_complement(dtype):
    n, batch, grades = 4, 65, [1, 2]
    x = rows_for(1, n, grades, batch, dtype)
    for undual in (False, True):
        e = inp(0, grades, n)
        spec = (e.undual() if undual else e.dual()).specialize(PGA, dtype=dtype)
        cot = rows_for(2, n, [2, 3], batch, dtype)
        g = spec.vjp(0).eval_batch([x], cot, batch).download_rows()
        want = dn.complement_rows(n, [2, 3], cot, undual=not undual)[0]      # the transpose is the other complement: bits
        assert np.array_equal(bits(g, dtype), bits(want, dtype))
        jv = dn.complement_rows(n, grades, x.astype(np.float64), undual=undual)[0]
        _adjoint_identity(cot, jv, g, x, dtype, 1e-12 * batch)      # the same products, summed in another order in float64


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("slot", [0, 1])
def test_vjp_of_vee_with_respect_to_each_side(slot, dtype):
    n, batch, lg, rg, og = 4, 65, [2, 3], [3, 4], [1, 2, 3]
    a, b = rows_for(3, n, lg, batch, dtype), rows_for(4, n, rg, batch, dtype)
    cot = rows_for(5, n, og, batch, dtype)
    spec = inp(0, lg, n).vee(inp(1, rg, n)).specialize(PGA, dtype=dtype)
    g = spec.vjp(slot).eval_batch([a, b], cot, batch).download_rows()
    want = dn.vee_rows_transposed(n, lg, rg, og, cot, b if slot == 0 else a, wrt_left=slot == 0)
    absw = dn.vee_rows_transposed(n, lg, rg, og, cot, b if slot == 0 else a, wrt_left=slot == 0, absolute=True)
    assert np.abs(want).max() > 0.5
    assert (np.abs(g.astype(np.float64) - want) <= 4 * EPS[dtype] * absw).all()
    v = a if slot == 0 else b
    jv = dn.vee_rows(n, lg, a, rg, b, og)      # linear in each side: J v is the product itself
    _adjoint_identity(cot, jv, g, v, dtype, 4 * EPS[dtype] * float((absw * np.abs(v)).sum()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_vjp_of_the_pga3d_join_reduced_over_a_shared_point(dtype):
    """p3 shared by all items: its gradient is the sum over the batch (reduce=True)"""
    n, batch = 4, 300
    p1, p2 = rows_for(6, n, [3], batch, dtype), rows_for(7, n, [3], batch, dtype)
    p3 = rows_for(8, n, [3], 1, dtype)
    cot = rows_for(9, n, [1], batch, dtype)
    spec = inp(0, [3], n).vee(inp(1, [3], n)).vee(inp(2, [3], n)).specialize(PGA, dtype=dtype)
    g = spec.vjp(2).eval_batch([p1, p2, p3], cot, batch, reduce=True).download_rows()
    assert g.shape == (1, 4)
    line = dn.vee_rows(n, [3], p1, [3], p2, [2])
    per_item = dn.vee_rows_transposed(n, [2], [3], [1], cot, line, wrt_left=False)
    absw = dn.vee_rows_transposed(n, [2], [3], [1], cot, dn.vee_rows(n, [3], p1, [3], p2, [2], absolute=True), wrt_left=False, absolute=True)
    want = per_item.sum(axis=0)
    assert np.abs(want).max() > 0.5
    # the lists (4 eps) and gaast_hip_mv_sum_rows' bound for B <= GAAST_SUM_ROWS_CHUNK rows: (B - 1 + 1) eps sum |x_i|
    assert (np.abs(g[0].astype(np.float64) - want) <= (4 + batch) * EPS[dtype] * absw.sum(axis=0)).all()
    jv = dn.vee_rows(n, [2], line, [3], p3, [1])
    _adjoint_identity(cot, jv, g, p3, dtype, (4 + batch) * EPS[dtype] * float((absw.sum(axis=0) * np.abs(p3[0])).sum()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("det", [1, -1], ids=["det_plus", "det_minus"])
def test_vjp_in_the_cga_null_basis(det, dtype):
    n, batch = 5, 33
    alg = _cga_grams()[det]
    a, b = rows_for(20, n, [4], batch, dtype), rows_for(21, n, [4], batch, dtype)
    cot = rows_for(22, n, [3], batch, dtype)
    spec = inp(0, [4], n).vee(inp(1, [4], n)).specialize(alg, dtype=dtype)
    for slot in (0, 1):
        g = spec.vjp(slot).eval_batch([a, b], cot, batch).download_rows().astype(np.float64)
        want = dn.vee_rows_transposed(n, [4], [4], [3], cot, b if slot == 0 else a, wrt_left=slot == 0)
        bound = GRAM_TOL[dtype] * np.linalg.norm(cot, axis=1) * np.linalg.norm(b if slot == 0 else a, axis=1)
        assert np.abs(want).max() > 0.3
        assert (np.linalg.norm(g - want, axis=1) <= bound).all(), np.abs(g - want).max()
    # dual of an input in the null basis: the gradient is undual of the cotangent, orientation sign included
    x, c2 = rows_for(23, n, [2], batch, dtype), rows_for(24, n, [3], batch, dtype)
    g = inp(0, [2], n).dual().specialize(alg, dtype=dtype).vjp(0).eval_batch([x], c2, batch).download_rows().astype(np.float64)
    want = dn.complement_rows(n, [3], c2.astype(np.float64), undual=True)[0]
    assert (np.linalg.norm(g - want, axis=1) <= GRAM_TOL[dtype] * np.linalg.norm(c2, axis=1)).all()


def test_torch_backward_agrees_with_vjp_eval_batch():
    import torch
    n, batch, dtype = 4, 37, ga.F64
    p = [rows_for(30 + s, n, [3], batch, dtype) for s in range(3)]
    cot = rows_for(33, n, [1], batch, dtype)
    spec = (inp(0, [3], n).vee(inp(1, [3], n)).vee(inp(2, [3], n))).dual().undual().specialize(PGA, dtype=dtype)
    ts = [torch.from_numpy(r).to("cuda").requires_grad_(True) for r in p]
    out = spec.torch_fn()(*ts)
    out.backward(torch.from_numpy(cot).to("cuda"))
    for slot in range(3):
        g = spec.vjp(slot).eval_batch(p, cot, batch).download_rows()
        assert np.abs(g).max() > 0.1
        assert np.array_equal(ts[slot].grad.cpu().numpy(), g)
