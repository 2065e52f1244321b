"""The two adjoints of an outermorphism on the GPU: gaast_hip_linmap_apply_transposed (with respect to the rows) and
gaast_hip_linmap_matrix_vjp (with respect to the matrix: k_linmap_outer_sum + k_linmap_minor_contract), and the torch binding
gaast_amd.autograd.outermorphism_fn."""
import functools
import itertools
import math

import numpy as np
import pytest

import gaast_amd as ga
from helpers import linmap_compound
from layouts import layouts_of, place

pytestmark = pytest.mark.gpu
NP = {ga.F32: np.float32, ga.F64: np.float64}
EPS = {ga.F32: 2.0 ** -23, ga.F64: 2.0 ** -52}
CHUNK = 1024          # GAAST_SUM_ROWS_CHUNK
CONTRACT_DEPTH = 22   # include/gaast_hip.h: ceil(C(14,7) / 256) + 8


def grade_len(n, k):
    return math.comb(n, k)


def masks_of(n):
    """full, {1}, {2,3}, {0,n}: the grades that exist at dimension n, without duplicates"""
    out = []
    for g in (list(range(n + 1)), [1], [2, 3], [0, n]):
        g = sorted({k for k in g if k <= n})
        if g and g not in out:
            out.append(g)
    return out


def offsets(n, grades):
    out, pos = {}, 0
    for k in sorted(grades):
        out[k] = pos
        pos += grade_len(n, k)
    return out, pos


# ---- apply_transposed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("n", [3, 6, 7, 12])
def test_apply_transposed_is_the_adjoint_and_the_map_of_the_transpose(n, dtype):
    rng = np.random.default_rng(n + dtype)
    m = rng.uniform(-1, 1, (n, n)) / math.sqrt(n)
    om, omt = ga.Outermorphism(m, dtype), ga.Outermorphism(m.T.copy(), dtype)
    B = 65
    for grades in ([list(range(n + 1)), [1], [0, 2]]):
        _, rl = offsets(n, grades)
        x = rng.uniform(-1, 1, (B, rl)).astype(NP[dtype])
        g = rng.uniform(-1, 1, (B, rl)).astype(NP[dtype])
        dx, dg = ga.DeviceMV.from_rows(n, grades, x, dtype), ga.DeviceMV.from_rows(n, grades, g, dtype)
        y = om.apply(dx).download_rows().astype(np.float64)
        z = om.apply_transposed(dg).download_rows()
        # same kernel, same compounds: the bits of the map of M^T
        assert np.array_equal(z, omt.apply(dg).download_rows()), grades
        z = z.astype(np.float64)
        x64, g64 = x.astype(np.float64), g.astype(np.float64)
        lhs, rhs = np.sum(g64 * y, axis=1), np.sum(z * x64, axis=1)
        # each side: rows summed as chains of at most max C(n,k) fused multiply-adds over compounds rounded to the dtype
        mag = np.zeros(B)
        pos = 0
        for k in grades:
            d = grade_len(n, k)
            mag += np.sum(np.abs(g64[:, pos:pos + d]) * (np.abs(x64[:, pos:pos + d]) @ np.abs(linmap_compound(m, k)).T), axis=1)
            pos += d
        depth = max(grade_len(n, k) for k in grades)
        assert np.all(np.abs(lhs - rhs) <= 2 * (depth + 4) * EPS[dtype] * mag), (grades, np.max(np.abs(lhs - rhs) / mag))


# ---- matrix_vjp --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def term_index(n, k):
    """(I, J, I \\ i, J \\ j, sign, target) of every term of grade k, as arrays"""
    masks = sorted(sum(1 << i for i in c) for c in itertools.combinations(range(n), k))
    prev = {b: r for r, b in enumerate(sorted(sum(1 << i for i in c) for c in itertools.combinations(range(n), k - 1)))}
    bits = [[i for i in range(n) if (b >> i) & 1] for b in masks]
    I, J, Ir, Jr, sg, tg = [], [], [], [], [], []
    for a, bi in enumerate(masks):
        for b, bj in enumerate(masks):
            for pi, i in enumerate(bits[a]):
                for pj, j in enumerate(bits[b]):
                    I.append(a), J.append(b), Ir.append(prev[bi & ~(1 << i)]), Jr.append(prev[bj & ~(1 << j)])
                    sg.append(-1.0 if (pi + pj) & 1 else 1.0), tg.append(i * n + j)
    return tuple(np.array(v) for v in (I, J, Ir, Jr, sg, tg))


def reference(m, dtype, n, grades, x, g):
    """(dL/dM, sum |terms|) in float64 from the formula: compounds as the map holds them (rounded to the dtype), W = g^T x"""
    off, _ = offsets(n, grades)
    dm, mag = np.zeros(n * n), np.zeros(n * n)
    x, g = x.astype(np.float64), g.astype(np.float64)
    for k in grades:
        if k == 0:
            continue
        d = grade_len(n, k)
        xs, gs = x[:, off[k]:off[k] + d], g[:, off[k]:off[k] + d]
        w, wa = gs.T @ xs, np.abs(gs).T @ np.abs(xs)
        c = linmap_compound(m, k - 1).astype(NP[dtype]).astype(np.float64)
        I, J, Ir, Jr, sg, tg = term_index(n, k)
        np.add.at(dm, tg, sg * c[Ir, Jr] * w[I, J])
        np.add.at(mag, tg, np.abs(c[Ir, Jr]) * wa[I, J])
    return dm.reshape(n, n), mag.reshape(n, n)


def depth(batch):
    return min(batch, CHUNK) + math.ceil(batch / CHUNK) + CONTRACT_DEPTH


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 6, 7, 8])
def test_matrix_vjp_against_the_formula(n, dtype):
    rng = np.random.default_rng(10 * n + dtype)
    m = rng.uniform(-1, 1, (n, n))
    om = ga.Outermorphism(m, dtype)
    worst = 0.0
    for grades in masks_of(n):
        _, rl = offsets(n, grades)
        xa = rng.uniform(-1, 1, (2049, rl)).astype(NP[dtype])
        ga_ = rng.uniform(-1, 1, (2049, rl)).astype(NP[dtype])
        for B in (1, 3, 64, 65, 1024, 1025, 2049):
            x, g = xa[:B], ga_[:B]
            dx, dg = ga.DeviceMV.from_rows(n, grades, x, dtype), ga.DeviceMV.from_rows(n, grades, g, dtype)
            got = om.matrix_vjp(dx, dg)
            again = om.matrix_vjp(dx, dg)
            assert got.dtype == NP[dtype] and np.array_equal(got, again), (grades, B)
            want, mag = reference(m, dtype, n, grades, x, g)
            err = np.abs(got.astype(np.float64) - want)
            bound = (depth(B) + 4) * EPS[dtype] * mag
            assert np.all(err[mag == 0] == 0), (grades, B)
            ratio = float(np.max(err[mag > 0] / bound[mag > 0])) if np.any(mag > 0) else 0.0
            worst = max(worst, ratio)
            assert ratio <= 1.0, (grades, B, ratio)
    print(f"n = {n} dtype = {dtype}: worst |err| / ((d + 4) eps sum |terms|) = {worst:.4f}")


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_matrix_vjp_on_wrapped_rows(dtype):
    """one row form (element loads): strided, padded and misaligned rows give the bits of contiguous rows, and stay untouched"""
    n, B, grades = 5, 65, list(range(6))
    rng = np.random.default_rng(3)
    m = rng.uniform(-1, 1, (n, n))
    om = ga.Outermorphism(m, dtype)
    x, g = (rng.uniform(-1, 1, (B, 32)).astype(NP[dtype]) for _ in range(2))
    base = om.matrix_vjp(ga.DeviceMV.from_rows(n, grades, x, dtype), ga.DeviceMV.from_rows(n, grades, g, dtype))
    want, mag = reference(m, dtype, n, grades, x, g)
    assert np.all(np.abs(base.astype(np.float64) - want) <= (depth(B) + 4) * EPS[dtype] * mag)
    lays = layouts_of(dtype)
    for lx, lg in zip(lays, lays[1:] + lays[:1]):
        px, pg = place(x, lx, dtype, n, grades), place(g, lg, dtype, n, grades)
        got = om.matrix_vjp(px.mv, pg.mv)
        assert np.array_equal(got, base), (lx, lg)
        px.check()
        pg.check()


def test_matrix_vjp_above_n_8_is_unimplemented_and_writes_nothing():
    import torch
    n = 9
    om = ga.Outermorphism(np.eye(n) + 0.1, ga.F64)
    x = ga.DeviceMV.from_rows(n, [1], np.ones((4, n)))
    out = torch.full((n, n), -777.25, dtype=torch.float64, device="cuda")
    with pytest.raises(ga.GaastError) as ei:
        om.matrix_vjp(x, x, out=out)
    assert ei.value.status_name == "UNIMPLEMENTED"
    ga.lib().gaast_hip_synchronize()
    torch.cuda.synchronize()
    assert bool((out == -777.25).all())


def test_matrix_vjp_argument_checks():
    om = ga.Outermorphism(np.eye(3), ga.F64)
    a = ga.DeviceMV.from_rows(3, [1], np.ones((4, 3)))
    for other in (ga.DeviceMV.from_rows(3, [2], np.ones((4, 3))), ga.DeviceMV.from_rows(3, [1], np.ones((5, 3))),
                  ga.DeviceMV.from_rows(3, [1], np.ones((4, 3)), ga.F32)):
        with pytest.raises(ga.GaastError) as ei:
            om.matrix_vjp(a, other)
        assert ei.value.status_name == "INVALID_ARGUMENT"


def test_torch_gradcheck_outermorphism():
    import torch
    from gaast_amd.autograd import outermorphism_fn
    n, B = 4, 5
    f = outermorphism_fn(ga.F64)
    gen = torch.Generator().manual_seed(0)
    m = torch.rand((n, n), generator=gen, dtype=torch.float64).mul(2).sub(1).cuda().requires_grad_()
    rows = torch.rand((B, 16), generator=gen, dtype=torch.float64).mul(2).sub(1).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda mm, rr: f(mm, rr, n, range(n + 1)), (m, rows), eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()
