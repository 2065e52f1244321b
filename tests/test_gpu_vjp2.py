"""Second-order reverse mode on the GPU: Vjp.vjp() on the forward's dense kernels, compact against explicit lists, inv, a shared
input, SpecializedAst.jvp(), and double backward through the torch binding.  Expected values come from trilinearity, from central
differences of first-order programs evaluated on the GPU, and from torch's gradgradcheck."""
import numpy as np
import pytest

import gaast_amd as ga
from golden_programs import PROGRAMS
from helpers import HipBackend
import test_gpu_vjp as V
from test_gpu_vjp import DENSE_METRICS, _abs_terms, _gp, _inp, _kernels, _layouts, _row_len, _torch_case

pytestmark = pytest.mark.gpu
PGA3D = [0.0, 1.0, 1.0, 1.0]
EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
NPT = {ga.F64: np.float64, ga.F32: np.float32}


def _rows(x):
    ga.lib().gaast_hip_synchronize()
    return x.download_rows()


def _ld(x):
    return x.astype(np.longdouble)


# ---- dense products ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 7, 8])
@pytest.mark.parametrize("dtype", [ga.F32, ga.F64])
@pytest.mark.parametrize("metric", ["euclid", "r42", "null1"])
def test_second_order_dense_products_run_on_the_forward_kernels(n, dtype, metric):
    m = DENSE_METRICS[metric](n)
    spec = _gp(n, dtype, metric=m, materialize_limit=1)
    fwd_kernels = _kernels(spec.launches())
    assert fwd_kernels, spec.launches()
    lay = _layouts(spec)
    out_mask, _ = spec.output_info()
    rng = np.random.default_rng(n * 13 + dtype)
    batch, N = 8, 1 << n
    a, b, g, h = (rng.uniform(-1.0, 1.0, (batch, N)).astype(NPT[dtype]) for _ in range(4))
    # first slot -> (other operand's slot, the adjoint its second-order program is, rows in the roles (A, B) of <G, A B>)
    for s1, other, side, roles in ((0, 1, "adjoint right", [h, b]), (1, 0, "adjoint left", [a, h])):
        v = spec.vjp(s1)
        w_other, w_g, w_self = v.vjp(other), v.vjp(2), v.vjp(s1)
        for w in (w_other, w_g):
            names = w.launches()
            assert _kernels(names) == fwd_kernels, (names, spec.launches())
            assert not any("product_csr" in l or "product_ell" in l for l in names), names
        assert any(side in l for l in w_other.launches()), w_other.launches()
        assert not any("adjoint" in l for l in w_g.launches()), w_g.launches()
        # <h, VJP(g; other)> = <v.vjp(other)(h), other> = <v.vjp(g)(h), g>: the same trilinear form, each side within the
        # library's 8 eps sum |terms|
        ins = [a, b, g]
        first = _rows(v.eval_batch([a, b], g, batch))
        lhs = np.sum(_ld(h) * _ld(first), axis=1)
        terms = _abs_terms(n, m, lay, roles, out_mask, g)
        for w, x in ((w_other, ins[other]), (w_g, g)):
            rhs = np.sum(_ld(_rows(w.eval_batch(ins, h, batch))) * _ld(x), axis=1)
            err = np.abs(lhs - rhs).astype(np.float64)
            assert np.all(err <= 16 * EPS[dtype] * terms), (s1, w.slot, np.max(err / terms))
        assert not _rows(w_self.eval_batch(ins, h, batch)).any(), "the first-order program does not read the slot it differentiates"


def test_c_entry_points_take_a_vjp_program():
    import ctypes as C
    L = ga.lib()

    def names(h):
        out = [L.gaast_hip_program_launch_name(h, i).decode() for i in range(L.gaast_hip_program_num_launches(h))]
        L.gaast_hip_program_destroy(h)
        return out
    spec = _gp(6, ga.F32, materialize_limit=1)
    v = spec.vjp(0)
    h = C.c_void_p()
    assert L.gaast_hip_program_create_vjp(C.byref(v.desc), 1, C.byref(h)) == 0
    assert names(h) == v.vjp(1).launches()
    spec, _ = _null_gram_case()
    v = spec.vjp(1)
    q = np.ascontiguousarray(spec.alg.basis, dtype=np.float64)
    h = C.c_void_p()
    assert L.gaast_hip_program_create_vjp_in_basis(C.byref(v.desc), q.ctypes.data_as(C.POINTER(C.c_double)), 0, C.byref(h)) == 0
    got = names(h)
    assert got == v.vjp(0).launches() and any(l.startswith("linmap[") for l in got)


# ---- compact against explicit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5])
def test_second_order_compact_products_agree_with_explicit_ones(n):
    rng = np.random.default_rng(n)
    metric = [1.0, -1.0, 0.0, 2.0, 1.0, 1.0][:n]
    batch = 8
    for build in (lambda: _inp(0, list(range(n + 1)), n) * _inp(1, [1, 2], n),
                  lambda: _inp(0, list(range(n + 1)), n) ^ _inp(1, [1, 2], n),
                  lambda: _inp(0, list(range(n + 1)), n) << _inp(1, list(range(n + 1)), n)):
        explicit = build().specialize(metric, flags=ga.FLAG_EXACT_ORDER)
        compact = build().specialize(metric, flags=ga.FLAG_EXACT_ORDER, materialize_limit=1)
        lay = _layouts(explicit)
        out_mask, out_len = explicit.output_info()
        lay3 = lay + [(n, out_mask)]          # the layouts of the roles (A, B, G) of <G, A o B>
        a, b = (rng.uniform(-1.0, 1.0, (batch, _row_len(*l))) for l in lay)
        g = rng.uniform(-1.0, 1.0, (batch, out_len))
        for s1 in range(2):
            h = rng.uniform(-1.0, 1.0, (batch, _row_len(*lay[s1])))
            roles = [a, b, g]
            roles[s1] = h                     # the second cotangent takes the role of the slot differentiated first
            for s2 in range(3):
                if s2 == s1:
                    continue
                x = _rows(explicit.vjp(s1).vjp(s2).eval_batch([a, b, g], h, batch))
                y = _rows(compact.vjp(s1).vjp(s2).eval_batch([a, b, g], h, batch))
                assert x.shape == y.shape == (batch, _row_len(*lay3[s2]))
                assert np.abs(x).max() > 0.1
                # component j of the result is the form with e_j in the role of s2: its own sum |terms|
                for j in range(x.shape[1]):
                    r = list(roles)
                    r[s2] = np.zeros_like(x)
                    r[s2][:, j] = 1.0
                    terms = _abs_terms(n, metric, lay, r[:2], out_mask, r[2])
                    assert np.all(np.abs(x[:, j] - y[:, j]) <= 16 * EPS[ga.F64] * terms), (s1, s2, j)


# ---- second order against central differences of the first, on the GPU --------------------------------------------------
def _check_vjp2(v, ts, rng, batch, h=1e-5, tol=1e-6, n_dirs=2):
    """test_gpu_vjp._check_vjp with the VJP program v in the place of the forward program: ts are its bound rows (the inputs of the
    program it differentiates, then its cotangent)."""
    def f(rows):
        return _rows(v.eval_batch(rows[:-1], rows[-1], batch)).astype(np.float64)
    base = f(ts)
    assert np.all(np.isfinite(base))
    k2 = rng.uniform(-1.0, 1.0, base.shape)
    slots = list(range(len(ts) - 1)) + [v.n_fwd]
    for k, slot in enumerate(slots):
        grad = _rows(v.vjp(slot).eval_batch(ts, k2, batch))
        assert np.all(np.isfinite(grad))
        for _ in range(n_dirs):
            d = rng.uniform(-1.0, 1.0, ts[k].shape)
            plus = f(ts[:k] + [ts[k] + h * d] + ts[k + 1:])
            minus = f(ts[:k] + [ts[k] - h * d] + ts[k + 1:])
            fd = np.sum(k2 * (plus - minus), axis=1) / (2 * h)
            an = np.sum(grad * d, axis=1)
            scale = 1.0 + np.abs(an) + np.sum(np.abs(k2) * np.abs(plus + minus), axis=1) / 2
            assert np.all(np.abs(fd - an) <= tol * scale), (slot, np.max(np.abs(fd - an) / scale))


@pytest.mark.parametrize("name,metric,grades,spread", [("pga3d_even", PGA3D, [0, 2, 4], 0.1), ("r4_full", [1.0] * 4, [0, 1, 2, 3, 4], 0.05)])
def test_second_order_inv_matches_central_differences(name, metric, grades, spread):
    # A = 1 + E with sum |E_i| <= 0.7 (N = 8) or 0.75 (N = 16) < 1: every item is invertible
    spec = _inp(0, grades, 4).inv().specialize(metric)
    rng = np.random.default_rng(len(grades))
    batch = 8
    (dim, mask), = _layouts(spec)
    A = rng.uniform(-spread, spread, (batch, _row_len(dim, mask)))
    assert np.all(np.abs(A[:, 1:]).sum(axis=1) + np.abs(A[:, 0]) < 1.0)
    A[:, 0] += 1.0
    g = rng.uniform(-1.0, 1.0, (batch, spec.output_info()[1]))
    v = spec.vjp(0)
    _check_vjp2(v, [A, g], rng, batch)
    assert spec.domain_errors() == 0 and v.domain_errors() == 0
    assert v.vjp(0).domain_errors() == 0 and v.vjp(1).domain_errors() == 0


def test_second_order_inv_times_vector_in_every_pair_of_slots():
    spec = (_inp(0, [0, 2, 4], 4).inv() * _inp(1, [1], 4)).specialize(PGA3D)
    rng = np.random.default_rng(4)
    batch = 8
    A = rng.uniform(-0.1, 0.1, (batch, 8))
    A[:, 0] += 1.0
    x = rng.uniform(-1.0, 1.0, (batch, 4))
    g = rng.uniform(-1.0, 1.0, (batch, spec.output_info()[1]))
    for s1 in range(2):
        _check_vjp2(spec.vjp(s1), [A, x, g], rng, batch)
        assert spec.vjp(s1).domain_errors() == 0


# ---- shared input ----------------------------------------------------------------------------------------------------------
def test_second_order_reduce_sums_the_gradient_of_a_shared_motor():
    M, X = _inp(0, [0, 2, 4], 4), _inp(1, [3], 4)
    spec = (M * X * M.rev()).specialize(PGA3D)
    rng = np.random.default_rng(2)
    motor = rng.uniform(-1, 1, (1, 8))
    x = rng.uniform(-1, 1, (300, 4))
    g = rng.uniform(-1, 1, (300, spec.output_info()[1]))
    for s1 in range(2):
        w = spec.vjp(s1).vjp(0)
        h = rng.uniform(-1, 1, (1 if s1 == 0 else 300, 8 if s1 == 0 else 4))   # the cotangent of a shared motor's gradient is shared
        per = _rows(w.eval_batch([motor, x, g], h, 300))
        tot = _rows(w.eval_batch([motor, x, g], h, 300, reduce=True))
        assert per.shape == (300, 8) and tot.shape == (1, 8)
        assert np.abs(tot).max() > 1e-3
        assert np.allclose(tot[0], per.sum(axis=0), rtol=1e-12, atol=1e-12)


# ---- forward mode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_jvp_of_golden_programs(name, h=1e-5, tol=1e-6, batch=8):
    p = PROGRAMS[name]
    spec = p["build"](HipBackend()).specialize(p["metric"])
    rng = np.random.default_rng(11)
    lay = _layouts(spec)
    # the first items of test_vjp_of_golden_programs_matches_central_differences: [0.3, 1] keeps sta_inverse's |v|^2 off zero
    rows = [rng.uniform(0.3, 1.0, (16, _row_len(*l)))[:batch] for l in lay]
    g = rng.uniform(-1.0, 1.0, (batch, spec.output_info()[1]))
    for slot in range(len(lay)):
        j = spec.jvp(slot)
        grad = _rows(spec.vjp(slot).eval_batch(rows, g, batch))
        for _ in range(2):
            v = rng.uniform(-1.0, 1.0, rows[slot].shape)
            jv = _rows(j.eval_batch(rows, v, batch))
            plus = V._fwd(spec, rows[:slot] + [rows[slot] + h * v] + rows[slot + 1:], batch)
            minus = V._fwd(spec, rows[:slot] + [rows[slot] - h * v] + rows[slot + 1:], batch)
            assert jv.shape == plus.shape
            # per item, against the central difference of the forward program in direction v, contracted with g as _check_vjp does
            fd = np.sum(g * (plus - minus), axis=1) / (2 * h)
            an = np.sum(g * jv, axis=1)
            scale = 1.0 + np.abs(an) + np.sum(np.abs(g) * np.abs(plus + minus), axis=1) / 2
            assert np.all(np.abs(fd - an) <= tol * scale), (slot, np.max(np.abs(fd - an) / scale))
            # and per component: (plus - minus) / 2h is J v itself
            cscale = 1.0 + np.abs(jv) + np.abs(plus + minus) / 2
            assert np.all(np.abs((plus - minus) / (2 * h) - jv) <= tol * cscale), slot
            # <g, J v> = <J^T g, v>
            assert np.all(np.abs(an - np.sum(grad * v, axis=1)) <= tol * scale), slot


# ---- torch -----------------------------------------------------------------------------------------------------------------
def _null_gram_case():
    """the geometric product of full multivectors at n = 4 in a basis with two null vectors (e3 . e4 = -1)"""
    gram = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -1], [0, 0, -1, 0]], dtype=np.float64)
    alg = ga.GramAlgebra(gram)
    assert not alg.identity_basis()
    full = list(range(5))
    return (_inp(0, full, 4) * _inp(1, full, 4)).specialize(alg), [(3, 16), (3, 16)]


@pytest.mark.parametrize("name", ["pga3d_motor", "cga_n5", "r6_gp", "null_gram_n4"])
def test_torch_gradgradcheck(name):
    import torch
    spec, shapes = _null_gram_case() if name == "null_gram_n4" else _torch_case(name, ga.F64)
    f = spec.torch_fn()
    torch.manual_seed(0)    # gradgradcheck draws its grad_outputs
    gen = torch.Generator().manual_seed(0)
    xs = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1).cuda().requires_grad_() for s in shapes]
    assert torch.autograd.gradgradcheck(f, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


def test_torch_hvp_f32_agrees_with_f64():
    import torch
    spec64, _ = _torch_case("pga3d_motor", ga.F64)
    spec32, _ = _torch_case("pga3d_motor", ga.F32)
    shapes = [(1, 8), (4096, 4)]
    gen = torch.Generator().manual_seed(1)
    base = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1) for s in shapes]
    vec = torch.rand((4096, 4), generator=gen, dtype=torch.float64).mul(2).sub(1)
    hvps = {}
    for spec, dt in ((spec64, torch.float64), (spec32, torch.float32)):
        xs = [b.to(dt).cuda().requires_grad_() for b in base]
        y = spec.torch_fn()(*xs)
        gx, = torch.autograd.grad(y.sum(), xs[1], create_graph=True)
        hv = torch.autograd.grad((gx * vec.to(dt).cuda()).sum(), xs)
        hvps[dt] = [t.double().cpu() for t in hv]
    assert hvps[torch.float64][0].abs().max() > 1.0
    for a, b in zip(hvps[torch.float64], hvps[torch.float32]):
        # the motor's row sums 4096 items: f32 accumulation bound, as test_torch_f32_backward_agrees_with_f64
        assert torch.allclose(a, b, rtol=0, atol=float(2 ** -23 * 64 * (1024 + 4) * a.abs().max().clamp(min=1)))


def test_torch_first_order_gradients_with_create_graph_are_bitwise_the_same():
    import torch
    for name in ("pga3d_motor", "r6_gp"):
        for dtype, dt in ((ga.F64, torch.float64), (ga.F32, torch.float32)):
            spec, shapes = _torch_case(name, dtype)
            gen = torch.Generator().manual_seed(2)
            base = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1).to(dt) for s in shapes]
            got = []
            for create_graph in (False, True):
                xs = [b.cuda().requires_grad_() for b in base]
                y = spec.torch_fn()(*xs)
                w = torch.linspace(-1, 1, y.numel(), dtype=dt).reshape(y.shape).cuda()
                grads = torch.autograd.grad(y, xs, grad_outputs=w, create_graph=create_graph)
                assert all(gr.requires_grad == create_graph for gr in grads)
                got.append([gr.detach().cpu() for gr in grads])
            for p, q in zip(*got):
                assert torch.equal(p, q)


def test_torch_second_derivative_through_gexp_is_unimplemented():
    import torch
    spec = (_inp(0, [0, 2], 3).gexp() * _inp(1, [0, 2], 3)).specialize(3)
    gen = torch.Generator().manual_seed(3)
    xs = [torch.rand((4, 4), generator=gen, dtype=torch.float64).sub(0.5).cuda().requires_grad_() for _ in range(2)]
    y = spec.torch_fn()(*xs)
    gx, = torch.autograd.grad(y.sum(), xs[0], create_graph=True)     # the first backward builds a graph and succeeds
    assert gx.requires_grad and torch.isfinite(gx).all()
    with pytest.raises(ga.GaastError) as ei:
        torch.autograd.grad(gx.sum(), xs[0])
    assert ei.value.status_name == "UNIMPLEMENTED"
    assert "GAAST_OP_GEXP_ADJ" in str(ei.value)
    # the other operand's gradient reads gexp(x) as an operand: differentiating it with respect to x is a first derivative of gexp
    gy, = torch.autograd.grad(y.sum(), xs[1], create_graph=True)
    hx, = torch.autograd.grad(gy.sum(), xs[0])
    assert torch.isfinite(hx).all() and hx.abs().max() > 0
