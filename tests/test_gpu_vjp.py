"""Reverse mode on the GPU: VJP programs against central differences of the forward program, compact adjoint products,
gaast_hip_mv_sum_rows, and the torch binding (gradcheck).  Expected values come from forward evaluations only."""
import math

import numpy as np
import pytest

import gaast_amd as ga
from golden_programs import PROGRAMS
from helpers import HipBackend

pytestmark = pytest.mark.gpu


def _row_len(dim, mask):
    return sum(math.comb(dim, k) for k in range(64) if (mask >> k) & 1)


def _layouts(spec):
    d = spec.program_desc()
    return [(d.inputs[s].storage_dim, d.inputs[s].grade_mask) for s in range(spec.num_user_inputs())]


def _fwd(spec, rows, batch):
    out = spec.eval_batch([rows[s] for s in range(len(rows))], batch)
    ga.lib().gaast_hip_synchronize()
    return out.download_rows().astype(np.float64)


def _check_vjp(spec, rng, batch=16, h=1e-5, tol=1e-6, n_dirs=2, lo=-1.0, hi=1.0):
    lay = _layouts(spec)
    rows = [rng.uniform(lo, hi, (batch, _row_len(*l))) for l in lay]
    mask, rl = spec.output_info()
    g = rng.uniform(-1.0, 1.0, (batch, rl))
    for slot in range(len(lay)):
        grad = spec.vjp(slot).eval_batch(rows, g, batch)
        ga.lib().gaast_hip_synchronize()
        grad = grad.download_rows()
        for _ in range(n_dirs):
            v = rng.uniform(-1.0, 1.0, rows[slot].shape)
            plus = _fwd(spec, rows[:slot] + [rows[slot] + h * v] + rows[slot + 1:], batch)
            minus = _fwd(spec, rows[:slot] + [rows[slot] - h * v] + rows[slot + 1:], batch)
            fd = np.sum(g * (plus - minus), axis=1) / (2 * h)
            an = np.sum(grad * v, axis=1)
            scale = 1.0 + np.abs(an) + np.sum(np.abs(g) * np.abs(plus + minus), axis=1) / 2
            assert np.all(np.abs(fd - an) <= tol * scale), (slot, np.max(np.abs(fd - an) / scale))


@pytest.mark.parametrize("name", sorted(PROGRAMS))
@pytest.mark.parametrize("flags", [0, ga.FLAG_EXACT_ORDER])
def test_vjp_of_golden_programs_matches_central_differences(name, flags):
    p = PROGRAMS[name]
    spec = p["build"](HipBackend()).specialize(p["metric"], flags=flags)
    _check_vjp(spec, np.random.default_rng(11), lo=0.3)


def _inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _gp(n, dtype=ga.F64, flags=0, metric=None, **kw):
    full = list(range(n + 1))
    e = _inp(0, full, n) * _inp(1, full, n)
    return e.specialize(metric if metric is not None else n, dtype=dtype, flags=flags, **kw)


def _blades(n, mask):
    """bitmask blade of every component of a row with grades `mask` (row order)"""
    L = ga.lib()
    return np.array([L.gaast_component_to_blade(n, k, i) for k in range(n + 1) if (mask >> k) & 1 for i in range(math.comb(n, k))],
                    dtype=np.int64)


def _abs_terms(n, metric, lay, rows, out_mask, g):
    """sum over the geometric product's terms |g_{a^b} m(a & b) a_a b_b| per item (the full product bounds every other kind's)."""
    N = 1 << n
    full = []
    for (dim, mask), r in zip(lay + [(n, out_mask)], rows + [g]):
        x = np.zeros((r.shape[0], N))
        x[:, _blades(n, mask)] = np.abs(r.astype(np.float64))
        full.append(x)
    A, B, G = full
    mabs = np.ones(N)
    for p in range(n):
        mabs[(np.arange(N) >> p) & 1 == 1] *= abs(metric[p])
    idx = np.arange(N)
    total = np.zeros(A.shape[0])
    for a in range(N):
        if A[:, a].any():
            total += A[:, a] * np.sum(B * mabs[a & idx] * G[:, a ^ idx], axis=1)
    return total


def _dot_test(spec, dtype, rng, metric, batch=8):
    """<g, f(a, b)> = <VJP_a(g), a> = <VJP_b(g), b> for a product linear in each slot: equal up to rounding.  Each side carries the
    library's per-component bound (at most 8 eps sum |terms| in a general metric), so the two differ by at most 16 eps sum |terms|."""
    lay = _layouts(spec)
    eps = 2.0 ** -52 if dtype == ga.F64 else 2.0 ** -23
    npt = np.float64 if dtype == ga.F64 else np.float32
    rows = [rng.uniform(-1.0, 1.0, (batch, _row_len(*l))).astype(npt) for l in lay]
    mask, rl = spec.output_info()
    g = rng.uniform(-1.0, 1.0, (batch, rl)).astype(npt)
    f = _fwd(spec, rows, batch)
    # the test's own dot products in extended precision: only the library's roundings remain
    lhs = np.sum(g.astype(np.longdouble) * f.astype(np.longdouble), axis=1)
    terms = _abs_terms(lay[0][0], metric, lay, rows, mask, g)
    for slot in range(len(lay)):
        grad = spec.vjp(slot).eval_batch(rows, g, batch)
        ga.lib().gaast_hip_synchronize()
        rhs = np.sum(grad.download_rows().astype(np.longdouble) * rows[slot].astype(np.longdouble), axis=1)
        err = np.abs(lhs - rhs).astype(np.float64)
        assert np.all(err <= 16 * eps * terms), (slot, np.max(err / terms))


@pytest.mark.parametrize("n", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("metric", ["euclid", "mixed", "scaled", "null1", "null2"])
def test_geometric_product_vjp_dot_product(n, dtype, metric):
    m = {"euclid": [1.0] * n, "mixed": [1.0] * (n - 2) + [-1.0] * 2, "scaled": [2.0, -0.5] + [1.5] * (n - 2),
         "null1": [0.0] + [1.0] * (n - 1), "null2": [0.0, 1.0, 0.0] + [-1.0] * (n - 3)}[metric]
    spec = _gp(n, dtype, metric=m)
    _dot_test(spec, dtype, np.random.default_rng(n * 31 + dtype), m)


@pytest.mark.parametrize("n", [4, 5, 6])
def test_compact_adjoint_products_equal_explicit_ones(n):
    rng = np.random.default_rng(n)
    metric = [1.0, -1.0, 0.0, 2.0, 1.0, 1.0][:n]
    for build in (lambda: _inp(0, list(range(n + 1)), n) * _inp(1, [1, 2], n),
                  lambda: _inp(0, list(range(n + 1)), n) ^ _inp(1, [1, 2], n),
                  lambda: _inp(0, list(range(n + 1)), n) << _inp(1, list(range(n + 1)), n)):
        explicit = build().specialize(metric, flags=ga.FLAG_EXACT_ORDER)
        compact = build().specialize(metric, flags=ga.FLAG_EXACT_ORDER, materialize_limit=1)
        lay = _layouts(explicit)
        rows = [rng.uniform(-1.0, 1.0, (32, _row_len(*l))) for l in lay]
        g = rng.uniform(-1.0, 1.0, (32, explicit.output_info()[1]))
        for slot in range(2):
            a = explicit.vjp(slot).eval_batch(rows, g, 32).download_rows()
            b = compact.vjp(slot).eval_batch(rows, g, 32).download_rows()
            assert np.array_equal(a, b), slot
        _dot_test(compact, ga.F64, rng, metric)


def test_exact_order_vjp_is_bitwise_repeatable():
    spec = _gp(6, ga.F32, flags=ga.FLAG_EXACT_ORDER)
    rng = np.random.default_rng(5)
    rows = [rng.uniform(-1, 1, (257, 64)).astype(np.float32) for _ in range(2)]
    g = rng.uniform(-1, 1, (257, 64)).astype(np.float32)
    for slot in range(2):
        v = spec.vjp(slot)
        first = v.eval_batch(rows, g, 257).download_rows()
        for _ in range(2):
            assert np.array_equal(v.eval_batch(rows, g, 257).download_rows(), first)
        assert not any("product_dense" in l for l in v.launches())


DENSE_METRICS = {
    "euclid": lambda n: [1.0] * n,
    "r42": lambda n: [1.0] * (n - 2) + [-1.0] * 2,
    "rpq": lambda n: [1.0] * (n // 2) + [-1.0] * (n - n // 2),
    "scaled": lambda n: [2.0, -0.5, 1.5, 0.75] + [1.0] * (n - 4),
    "null1": lambda n: [0.0] + [1.0] * (n - 1),
    "null2": lambda n: [1.0, 0.0, -1.0, 0.0] + [1.0] * (n - 4),
}


def _kernels(names):
    return sorted({l.split("::")[-1].strip().split("<")[0] for l in names if "product_dense" in l})


@pytest.mark.parametrize("n", [6, 7, 8, 10, 12])
@pytest.mark.parametrize("dtype", [ga.F32, ga.F64])
@pytest.mark.parametrize("metric", sorted(DENSE_METRICS))
def test_dense_adjoints(n, dtype, metric):
    m = DENSE_METRICS[metric](n)
    spec = _gp(n, dtype, metric=m, materialize_limit=1)
    fwd_kernels = _kernels(spec.launches())
    assert fwd_kernels, spec.launches()
    rng = np.random.default_rng(n * 7 + dtype)
    for slot in range(2):
        names = spec.vjp(slot).launches()
        assert _kernels(names) == fwd_kernels, (names, spec.launches())
        assert not any("product_csr" in l or "product_ell" in l for l in names), names
        assert any("adjoint" in l for l in names), names
    batch = 8 if n <= 10 else 4
    _dot_test(spec, dtype, rng, m, batch=batch)
    if n <= 8:   # against the same VJP on the list path (EXACT_ORDER), in the library's dense bound
        exact = _gp(n, dtype, ga.FLAG_EXACT_ORDER, metric=m, materialize_limit=1)
        eps = 2.0 ** -52 if dtype == ga.F64 else 2.0 ** -23
        npt = np.float64 if dtype == ga.F64 else np.float32
        rows = [rng.uniform(-1, 1, (batch, 1 << n)).astype(npt) for _ in range(2)]
        g = rng.uniform(-1, 1, (batch, 1 << n)).astype(npt)
        N, full_mask = 1 << n, (1 << (n + 1)) - 1
        bl = _blades(n, full_mask)
        mabs = np.ones(N)
        for p in range(n):
            mabs[(np.arange(N) >> p) & 1 == 1] *= abs(m[p])
        idx = np.arange(N)
        absr = []
        for r in rows + [g]:
            x = np.zeros((batch, N))
            x[:, bl] = np.abs(r.astype(np.float64))
            absr.append(x)
        for slot in range(2):
            a = spec.vjp(slot).eval_batch(rows, g, batch).download_rows().astype(np.float64)
            b = exact.vjp(slot).eval_batch(rows, g, batch).download_rows().astype(np.float64)
            # per component c of the gradient: sum over its terms |m(c & j) G_{c ^ j} other_j| (same form for either operand)
            other, G = absr[1 - slot], absr[2]
            tb = np.stack([np.sum(other * mabs[c & idx] * G[:, c ^ idx], axis=1) for c in range(N)], axis=1)
            t = tb[:, bl]
            assert np.all(np.abs(a - b) <= 16 * eps * t + 1e-300), (slot, np.max(np.abs(a - b) / (t + 1e-300)))


def test_compact_adjoint_list_beyond_the_budget_is_refused():
    # EXACT_ORDER keeps a compact geometric adjoint off the dense kernels; at n = 12 its list (16.7 M entries) is not built
    spec = _gp(12, ga.F32, ga.FLAG_EXACT_ORDER, materialize_limit=1)
    with pytest.raises(ga.GaastError) as ei:
        spec.vjp(0).program()
    assert ei.value.status_name == "UNIMPLEMENTED"


def test_nonlinear_programs_f64():
    rng = np.random.default_rng(9)
    x = _inp(0, [1], 4)
    for e in (x.vinv(), x.norm_sq().sinv() * x, x.norm_sq().sqrt() * x):
        _check_vjp(e.specialize([1.0, 1.0, 1.0, 1.0]), rng, h=1e-6, tol=1e-6, lo=0.5)


# ---- sum_rows -------------------------------------------------------------------------------------------------------
CHUNK = 1024


@pytest.mark.parametrize("batch,row", [(1, 1), (2, 16), (63, 32), (257, 1), (257, 4096), (4097, 16), (4097, 4096), (1 << 20, 16),
                                       (1 << 20, 1), (4097, 32)])
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_sum_rows(batch, row, dtype):
    # a row of `row` components: grade 1 of R^row (row = 1: the scalar of R^1)
    dim, grades = (1, [0]) if row == 1 else (row, [1]) if row <= 16 else (5, [0, 1, 2, 3, 4, 5]) if row == 32 else (12, list(range(13)))
    assert _row_len(dim, sum(1 << k for k in grades)) == row
    npt = np.float64 if dtype == ga.F64 else np.float32
    x = np.random.default_rng(batch + row).uniform(-1.0, 1.0, (batch, row)).astype(npt)
    mv = ga.DeviceMV.from_rows(dim, grades, x, dtype)
    a = mv.sum_rows().download_rows()
    b = mv.sum_rows().download_rows()
    assert np.array_equal(a, b)
    exact = np.array([math.fsum(x[:, j].astype(np.float64)) for j in range(row)]) if batch * row <= 1 << 22 else \
        np.sum(x.astype(np.longdouble), axis=0).astype(np.float64)
    eps = 2.0 ** -52 if dtype == ga.F64 else 2.0 ** -23
    bound = (CHUNK + math.ceil(batch / CHUNK)) * eps * np.sum(np.abs(x.astype(np.float64)), axis=0)
    assert np.all(np.abs(a[0].astype(np.float64) - exact) <= bound + 1e-300)


def test_vjp_reduce_sums_the_gradient_of_a_shared_input():
    spec = (_inp(0, [0, 2], 3) * _inp(1, [1], 3) * _inp(0, [0, 2], 3).rev()).specialize(3)
    rng = np.random.default_rng(2)
    r = rng.uniform(-1, 1, (1, 4))
    x = rng.uniform(-1, 1, (300, 3))
    g = rng.uniform(-1, 1, (300, spec.output_info()[1]))
    per = spec.vjp(0).eval_batch([r, x], g, 300).download_rows()
    tot = spec.vjp(0).eval_batch([r, x], g, 300, reduce=True).download_rows()
    assert tot.shape == (1, 4)
    assert np.allclose(tot[0], per.sum(axis=0), rtol=1e-12, atol=1e-12)


# ---- torch -----------------------------------------------------------------------------------------------------------
def _torch_case(name, dtype):
    if name == "pga3d_motor":
        n, m = 4, [0.0, 1.0, 1.0, 1.0]
        M, X = _inp(0, [0, 2, 4], n), _inp(1, [3], n)
        return (M * X * M.rev()).specialize(m, dtype=dtype), [(1, 8), (6, 4)]
    if name == "cga_n5":
        n = 5
        A, B = _inp(0, [0, 2], n), _inp(1, [1], n)
        return ((A * B) ^ B.ginvol() + (A << B)).specialize([1.0, 1.0, 1.0, 1.0, -1.0], dtype=dtype), [(3, 11), (3, 5)]
    n = 6
    return (_inp(0, list(range(7)), n) * _inp(1, list(range(7)), n)).specialize(6, dtype=dtype), [(2, 64), (2, 64)]


@pytest.mark.parametrize("name", ["pga3d_motor", "cga_n5", "r6_gp"])
def test_torch_gradcheck(name):
    import torch
    spec, shapes = _torch_case(name, ga.F64)
    f = spec.torch_fn()
    gen = torch.Generator().manual_seed(0)
    xs = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1).cuda().requires_grad_() for s in shapes]
    assert torch.autograd.gradcheck(f, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


def test_torch_f32_backward_agrees_with_f64():
    import torch
    spec64, shapes = _torch_case("pga3d_motor", ga.F64)
    spec32, _ = _torch_case("pga3d_motor", ga.F32)
    shapes = [(1, 8), (4096, 4)]
    gen = torch.Generator().manual_seed(1)
    base = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1) for s in shapes]
    grads = {}
    for spec, dt in ((spec64, torch.float64), (spec32, torch.float32)):
        xs = [b.to(dt).cuda().requires_grad_() for b in base]
        y = spec.torch_fn()(*xs)
        y.backward(torch.ones_like(y))
        grads[dt] = [x.grad.double().cpu() for x in xs]
    for a, b in zip(grads[torch.float64], grads[torch.float32]):
        # the motor's gradient sums 4096 items: f32 accumulation bound
        assert torch.allclose(a, b, rtol=0, atol=float(2 ** -23 * 64 * (1024 + 4) * a.abs().max().clamp(min=1)))
    with pytest.raises(TypeError):
        spec64.torch_fn()(*[b.float().cuda() for b in base])
