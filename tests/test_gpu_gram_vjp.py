"""Reverse mode of programs in non-diagonal (Gram) metrics on the GPU (gaast_hip_program_create_vjp_in_basis): against central
differences of the independent, non-diagonalising oracle of tests/clifford_gram.py, against the plain VJP moved by hand, and
through torch."""
import ctypes as C
import math

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib
from clifford_gram import GramClifford, mv_to_row, row_blades, row_to_mv
from helpers import linmap_compound
from test_gpu_gram_metric import CGA_GRAM, NP, TOL, cases, inp, random_gram, rows_for, versor_rows

pytestmark = pytest.mark.gpu
EPS = {ga.F32: 2.0 ** -23, ga.F64: 2.0 ** -52}
H, FD_TOL = 1e-5, 1e-6     # the step and allowance of test_gpu_vjp.py's central-difference checks
USED = ("gp", "op", "lc", "a_plus_bc_g2", "sandwich_g1")
PD = C.POINTER(C.c_double)


def grams(n):
    rng = np.random.default_rng(40 + n)
    out = [("indefinite", random_gram(rng, n, "indefinite")), ("degenerate", random_gram(rng, n, "degenerate"))]
    if n == 5:
        out.append(("cga", CGA_GRAM))
    return out


def grades_of(mask):
    return [k for k in range(64) if (mask >> k) & 1]


def oracle_gradient(cl, n, in_grades, oracle, out_grades, rows_i, g_i, slot):
    """(gradient row of input `slot`, finite-difference allowance per component) by f64 central differences of the oracle"""
    r = rows_i[slot]
    grad, allow = np.zeros(r.size), np.zeros(r.size)

    def f(row):
        args = [row_to_mv(n, gr, row if s == slot else rows_i[s]) for s, gr in enumerate(in_grades)]
        return mv_to_row(n, out_grades, oracle(cl, *args))
    for j in range(r.size):
        e = np.zeros(r.size)
        e[j] = H
        plus, minus = f(r + e), f(r - e)
        grad[j] = np.sum(g_i * (plus - minus)) / (2 * H)
        allow[j] = FD_TOL * (1.0 + abs(grad[j]) + np.sum(np.abs(g_i) * np.abs(plus + minus)) / 2)
    return grad, allow


def check_against_oracle(alg, cl, n, name, in_grades, build, oracle, dtype, rows, factor=1.0):
    batch = rows[0].shape[0]
    rng = np.random.default_rng(5)
    spec = build(*[inp(s, g, n) for s, g in enumerate(in_grades)]).specialize(alg, dtype=dtype)
    out_grades = grades_of(spec.output_info()[0])
    rows = [r.astype(NP[dtype]) for r in rows]
    g = rng.uniform(-1, 1, (batch, spec.output_info()[1])).astype(NP[dtype])
    r64, g64 = [r.astype(np.float64) for r in rows], g.astype(np.float64)
    worst = 0.0
    for slot in range(len(in_grades)):
        v = spec.vjp(slot)
        got = v.eval_batch(rows, g, batch).download_rows().astype(np.float64)
        assert any(l.startswith("linmap[") for l in v.launches())
        for i in range(batch):
            want, allow = oracle_gradient(cl, n, in_grades, oracle, out_grades, [r[i] for r in r64], g64[i], slot)
            bound = factor * TOL[dtype] * np.linalg.norm(g64[i]) * np.prod([np.linalg.norm(r[i]) for r in r64])
            err = np.linalg.norm(got[i] - want)
            worst = max(worst, err / (bound + np.linalg.norm(allow)))
            assert err <= bound + np.linalg.norm(allow), (name, slot, i, err, bound, np.linalg.norm(allow))
    print(f"{name} n = {n}: worst error / allowance = {worst:.3g}")


# ---- check 1: the independent oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("name", USED)
@pytest.mark.parametrize("n,kind", [(3, "indefinite"), (3, "degenerate"), (5, "indefinite"), (5, "degenerate"), (5, "cga")])
def test_vjp_against_central_differences_of_the_gram_oracle(n, kind, name, dtype):
    (_, in_grades, build, oracle), = [c for c in cases(n) if c[0] == name]
    g = dict(grams(n))[kind]
    alg, cl = ga.GramAlgebra(g), GramClifford(g)
    assert not alg.identity_basis()
    rng = np.random.default_rng(n * 7 + len(kind) + dtype)
    rows = [rows_for(rng, n, gr, 9) for gr in in_grades]
    check_against_oracle(alg, cl, n, f"{name}/{kind}", in_grades, build, oracle, dtype, rows)


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("n", [3, 5])
def test_vjp_of_the_versor_inverse_against_the_gram_oracle(n, dtype):
    for kind, g in grams(n):
        if kind == "degenerate":
            continue
        alg, cl = ga.GramAlgebra(g), GramClifford(g)
        rows = versor_rows(np.random.default_rng(n), cl, n, 9)
        full = list(range(n + 1))
        check_against_oracle(alg, cl, n, f"vinv/{kind}", [full], lambda a: a.vinv(), lambda c, a: c.vinv(a), dtype, [rows], factor=100.0)


# ---- check 2: the plain VJP moved by hand ------------------------------------------------------------------------------
def move(q, n, grades, rows):
    """C_k(q) on every grade slice of the rows, in float64"""
    out, pos = np.empty_like(rows, dtype=np.float64), 0
    for k in sorted(grades):
        d = math.comb(n, k)
        out[:, pos:pos + d] = rows[:, pos:pos + d].astype(np.float64) @ linmap_compound(q, k).T
        pos += d
    return out


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("name", USED)
def test_gram_vjp_is_the_moved_plain_vjp(name, dtype):
    n = 5
    (_, in_grades, build, _), = [c for c in cases(n) if c[0] == name]
    for kind, g in grams(n):
        alg = ga.GramAlgebra(g)
        q = alg.basis
        rng = np.random.default_rng(17)
        rows = [rows_for(rng, n, gr, 9).astype(NP[dtype]) for gr in in_grades]
        mk = lambda a: build(*[inp(s, gr, n) for s, gr in enumerate(in_grades)]).specialize(a, dtype=dtype)
        sg, sp = mk(alg), mk(ga.MetricAlgebra(alg.diag))
        out_grades = grades_of(sg.output_info()[0])
        cot = rng.uniform(-1, 1, (9, sg.output_info()[1])).astype(NP[dtype])
        rows_f = [move(q.T, n, gr, r) for gr, r in zip(in_grades, rows)]
        cot_f = move(q.T, n, out_grades, cot)
        for slot, gr in enumerate(in_grades):
            got = sg.vjp(slot).eval_batch(rows, cot, 9).download_rows().astype(np.float64)
            plain = sp.vjp(slot).eval_batch([r.astype(NP[dtype]) for r in rows_f], cot_f.astype(NP[dtype]), 9).download_rows()
            want = move(q, n, gr, plain)
            for i in range(9):
                bound = TOL[dtype] * np.linalg.norm(cot[i].astype(np.float64)) * np.prod([np.linalg.norm(r[i].astype(np.float64)) for r in rows])
                assert np.linalg.norm(got[i] - want[i]) <= bound, (name, kind, slot, i)


# ---- check 3: identity basis ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_diagonal_gram_vjp_is_the_plain_vjp(dtype):
    diag = [1.0, -1.0, 0.0, 2.0, 1.0]
    n, full = len(diag), list(range(len(diag) + 1))
    rng = np.random.default_rng(4)
    rows = [rows_for(rng, n, full, 50).astype(NP[dtype]) for _ in range(2)]
    build = lambda: (inp(0, full, n) * inp(1, full, n) + inp(0, full, n).rev()).g(2)
    s1 = build().specialize(ga.GramAlgebra(np.diag(diag)), dtype=dtype)
    s2 = build().specialize(ga.MetricAlgebra(diag), dtype=dtype)
    cot = rng.uniform(-1, 1, (50, s1.output_info()[1])).astype(NP[dtype])
    for slot in (0, 1):
        v1, v2 = s1.vjp(slot), s2.vjp(slot)
        assert v1.launches() == v2.launches() and not any("linmap" in l for l in v1.launches())
        assert np.array_equal(v1.eval_batch(rows, cot, 50).download_rows(), v2.eval_batch(rows, cot, 50).download_rows())


# ---- check 4: launch names -------------------------------------------------------------------------------------------------
def test_launch_names_of_a_gram_vjp():
    n, full = 4, list(range(5))
    alg = ga.GramAlgebra(random_gram(np.random.default_rng(1), n, "indefinite"))
    names = (inp(0, full, n) * inp(1, full, n)).specialize(alg).vjp(0).launches()
    # d(a b)/da reads b (slot 1) and the cotangent (slot 2), not a
    assert sum(l.startswith("linmap[input 1 ->") for l in names) == 1 and sum(l.startswith("linmap[input 2 ->") for l in names) == 1
    assert not any(l.startswith("linmap[input 0 ->") for l in names)
    assert names[-1].startswith("linmap[result ->")
    # a scalar input: its gradient holds grade 0 only and is not moved
    names = inp(0, [0], n).scal(inp(1, full, n)).specialize(alg).vjp(0).launches()
    assert not any(l.startswith("linmap[result") for l in names), names
    assert any(l.startswith("linmap[input 1 ->") for l in names), names


# ---- check 5: a shared input -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_reduce_sums_the_gradient_of_a_shared_rotor(dtype):
    n, B = 5, 1025
    alg = ga.GramAlgebra(CGA_GRAM)
    R, X = inp(0, [0, 2], n), inp(1, [1], n)
    spec = (R * X * R.rev()).g(1).specialize(alg, dtype=dtype)
    rng = np.random.default_rng(8)
    r = rng.uniform(-1, 1, (1, 11)).astype(NP[dtype])
    x = rng.uniform(-1, 1, (B, 5)).astype(NP[dtype])
    g = rng.uniform(-1, 1, (B, 5)).astype(NP[dtype])
    shared = ga.DeviceMV.from_rows(n, [0, 2], r, dtype)
    per = spec.vjp(0).eval_batch([shared, x], g, B).download_rows().astype(np.float64)
    tot = spec.vjp(0).eval_batch([shared, x], g, B, reduce=True).download_rows().astype(np.float64)
    assert tot.shape == (1, 11)
    exact = np.array([math.fsum(per[:, j]) for j in range(11)])
    bound = (1024 + math.ceil(B / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)
    assert np.all(np.abs(tot[0] - exact) <= bound)


# ---- check 6: exp / log ------------------------------------------------------------------------------------------------------
def exp_sandwich(flags, dtype=ga.F64):
    n = 5
    Bv, X = inp(0, [2], n), inp(1, [1], n)
    return (Bv.exp() * X * Bv.exp().rev()).g(1).specialize(ga.GramAlgebra(CGA_GRAM), dtype=dtype, flags=flags)


def test_exp_sandwich_gradient_of_a_shared_generator_in_the_null_basis():
    """f64 against central differences of the forward Gram program (code of the parent, pinned by its own tests).  Step and
    allowance are test_gpu_vjp.py's (h = 1e-5, 1e-6 of the magnitudes involved): the forward program's rounding error over 2 h
    is ~ 1e-11 of them, the truncation h^2 f''' / 6 ~ 1e-10."""
    spec = exp_sandwich(ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD)
    rng = np.random.default_rng(21)
    batch = 9
    b = rng.uniform(-0.5, 0.5, (1, 10))
    x = rng.uniform(-1, 1, (batch, 5))
    g = rng.uniform(-1, 1, (batch, 5))
    fwd = lambda bb: spec.eval_batch([ga.DeviceMV.from_rows(5, [2], bb), x], batch).download_rows()
    v = spec.vjp(0)
    assert any(l.startswith("linmap[") for l in v.launches())
    tot = v.eval_batch([ga.DeviceMV.from_rows(5, [2], b), x], g, batch, reduce=True).download_rows()[0]
    for _ in range(4):
        d = rng.uniform(-1, 1, (1, 10))
        plus, minus = fwd(b + H * d), fwd(b - H * d)
        fd = np.sum(g * (plus - minus)) / (2 * H)
        an = float(np.sum(tot * d[0]))
        scale = 1.0 + abs(an) + np.sum(np.abs(g) * np.abs(plus + minus)) / 2
        assert abs(fd - an) <= FD_TOL * scale, (fd, an, scale)


def test_exp_without_the_grad_flag_stays_unimplemented():
    with pytest.raises(ga.GaastError) as ei:
        exp_sandwich(ga.FLAG_EXP_LOG).vjp(0).program()
    assert ei.value.status_name == "UNIMPLEMENTED"


# ---- check 7: torch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exp_sandwich", "gp"])
def test_torch_gradcheck_in_the_null_basis(name):
    import torch
    if name == "exp_sandwich":
        spec, shapes, scale = exp_sandwich(ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD), [(1, 10), (3, 5)], 0.5
    else:
        full = list(range(6))
        spec, shapes, scale = (inp(0, full, 5) * inp(1, full, 5)).specialize(ga.GramAlgebra(CGA_GRAM)), [(3, 32), (3, 32)], 1.0
    gen = torch.Generator().manual_seed(0)
    xs = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1).mul(scale).cuda().requires_grad_() for s in shapes]
    assert torch.autograd.gradcheck(spec.torch_fn(), xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


# ---- check 8: the C ABI ----------------------------------------------------------------------------------------------------------
def test_c_abi_errors_leave_out_untouched():
    ga.init_device()
    L = ga.lib()
    n, full = 3, [0, 1, 2, 3]
    alg = ga.GramAlgebra(random_gram(np.random.default_rng(3), n, "indefinite"))
    q = np.ascontiguousarray(alg.basis)
    build = lambda flags: (inp(0, full, n) * inp(1, full, n)).specialize(alg, flags=flags)
    spec = build(0)
    d = spec.program_desc()
    sentinel = 0x1234
    h = C.c_void_p(sentinel)
    bad = q.copy()
    bad[0, 0] += 1e-6
    assert _lib.STATUS_NAMES[L.gaast_hip_program_create_vjp_in_basis(C.byref(d), bad.ctypes.data_as(PD), 0, C.byref(h))] == "INVALID_ARGUMENT"
    assert h.value == sentinel
    assert _lib.STATUS_NAMES[L.gaast_hip_program_create_vjp_in_basis(C.byref(d), q.ctypes.data_as(PD), 7, C.byref(h))] == "INVALID_ARGUMENT"
    assert h.value == sentinel
    sp = build(ga.FLAG_SPINOR_GEMM)
    ds = sp.program_desc()
    assert _lib.STATUS_NAMES[L.gaast_hip_program_create_vjp_in_basis(C.byref(ds), q.ctypes.data_as(PD), 0, C.byref(h))] == "UNIMPLEMENTED"
    assert h.value == sentinel
    # and the good call gives the program Vjp.program() runs
    assert L.gaast_hip_program_create_vjp_in_basis(C.byref(d), q.ctypes.data_as(PD), 0, C.byref(h)) == 0 and h.value != sentinel
    names = [L.gaast_hip_program_launch_name(h, i).decode() for i in range(L.gaast_hip_program_num_launches(h))]
    assert names == spec.vjp(0).launches()
    L.gaast_hip_program_destroy(h)
