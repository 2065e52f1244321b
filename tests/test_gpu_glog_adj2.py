"""Second order through the general logarithm on the GPU (GAAST_FLAG_GSQRT_GLOG_JVP | GAAST_FLAG_GLOG_GRAD2; GAAST_OP_GLOG_ADJ2, kernel
k_mv_adj2_glog<T, N>), against glog_adj2_numpy.py.  Everything runs through spec.vjp(0).vjp(0).eval_batch([A, g], h, batch).

Accuracy.  The reference is the numpy restatement in numpy.longdouble on the reference forward (roots run to their own floor;
theta = 1/16 and 12 nodes), never the code under test.  The unit per item is N eps max(1, sum |log A|) ||G||_inf ||h||_inf, G the
N x N matrix with GLOG_ADJ2(g, h, A) = G h (glog_adj2_numpy.hessian_norm).  The bound is 4 x glog_adj2_numpy.LOG_ADJ2_SCALE -- the worst
error of the restatement in the program's dtype on the CPU (tests/test_glog_adj2_host.py measures it on every run; N = 2 has scales of its
own), times the project's 4 for the device's fused multiply-adds and pivot ties on other roundings.  The worst measured value per case is
printed (the record of DESIGN.md section 17.2).

Inputs: root_log_jvp_numpy.case_operands: twelve items (nine at N = 64) whose logarithm takes 0 ... 5 roots, in one workgroup, the batch
no multiple of 256 / N; R^1 has 257 items, two workgroups of 128 and a tail.  Values are rounded to float32 so that both dtypes see the
same numbers."""
import math

import numpy as np
import pytest

import gaast_amd as ga

import gexp_numpy as gx
import glog_adj2_numpy as g2
import glog_numpy as gl
import inverse_numpy as inu
from helpers import linmap_compound
from layouts import place, place_out
from test_gpu_gexp2 import dl, only
from test_gpu_glog import CGA_GRAM, DTYPES, EPS, IDS, NP, PGA, TY, inp, op_rows
from test_gpu_vjp2 import _check_vjp2

pytestmark = pytest.mark.gpu

SEED = 20261021
FLAGS = ga.FLAG_GSQRT_GLOG_JVP | ga.FLAG_GLOG_GRAD2
_DATA = {}


def data(name):
    """(A, h, g over S; the longdouble reference and the unit's factors): drawn and computed once per case, read-only"""
    if name not in _DATA:
        metric, grades, N = g2.CASES[name]
        A, h, g = g2.case_operands(name)
        d = dict(A=A, h=h, g=g, want=g2.log_adj2_reference(metric, grades, A, g, h).astype(np.float64),
                 ref=gl.log_reference(metric, grades, A).astype(np.float64), gn=g2.hessian_norm(metric, grades, A, g))
        for a in d.values():
            a.setflags(write=False)
        _DATA[name] = d
    return _DATA[name]


def spec_of(name, dtype, flags=FLAGS):
    metric, grades, N = g2.CASES[name]
    return inp(0, grades, len(metric)).glog().specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=flags)


def rows_of(name, dtype):
    metric, grades, N = g2.CASES[name]
    d = data(name)
    return tuple(op_rows(metric, grades, d[k], dtype) for k in ("A", "g", "h"))


def errors(name, dtype, got, sel=slice(None)):
    d = data(name)
    return g2.log_adj2_error(got, d["want"][sel], EPS[dtype], d["ref"][sel], d["gn"][sel], d["h"][sel])


def bound_of(name, dtype):
    return 4 * g2.scale_of(g2.LOG_ADJ2_SCALE, g2.CASES[name][2], NP[dtype])


# ---- 1. the kernel against the longdouble restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(g2.CASES))
def test_adj2_against_the_longdouble_restatement(name, dtype):
    metric, grades, N = g2.CASES[name]
    arow, grow, hrow = rows_of(name, dtype)
    B = len(arow)
    w = spec_of(name, dtype).vjp(0).vjp(0)
    (one,) = only(w.launches(), "general_log_adjoint2[")
    assert one.endswith(f":: k_mv_adj2_glog<{TY[dtype]},{N}>") and f"{N}" in one and "produced" in one, one
    assert len(only(w.launches(), "k_mv_adj2_glog<")) == 1 and not only(w.launches(), "k_mv_glog") and not only(w.launches(), "k_mv_jvp_glog"), w.launches()
    raw = dl(w.eval_batch([arow, grow], hrow, B))
    got = gx.to_s(metric, grades, raw.astype(np.float64))
    e = errors(name, dtype, got)
    print(f"LOG_ADJ2 {name} {TY[dtype]} N={N}: worst {e.max():.3f} units (bound {bound_of(name, dtype):.2f}), {B} items")
    assert np.isfinite(got).all() and e.max() <= bound_of(name, dtype), (name, e.max(), int(np.argmax(e)))
    assert np.abs(data(name)["want"]).max() > 0.1
    # an item's result does not depend on the batch it is part of
    assert np.array_equal(dl(w.eval_batch([arow[:5], grow[:5]], hrow[:5], 5)).view(np.uint8), raw[:5].view(np.uint8))
    assert w.domain_errors() == 0
    # with the flags the forward and the first-order programs launch what they launch without them
    plain = spec_of(name, dtype, flags=0)
    assert spec_of(name, dtype).launches() == plain.launches() and spec_of(name, dtype).vjp(0).launches() == plain.vjp(0).launches()


# ---- 2. row forms and bookkeeping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strided_misaligned_and_shared_rows(dtype):
    """padded and misaligned rows on all three operand rows and on the result; a batch-1 shared A (stride 0) with reduce=True"""
    name = "PGA3D"
    metric, grades, N = g2.CASES[name]
    n = len(metric)
    arow, grow, hrow = rows_of(name, dtype)
    B = len(arow)
    w = spec_of(name, dtype).vjp(0).vjp(0)
    want = dl(w.eval_batch([arow, grow], hrow, B))
    for lin, lout in (("pad_odd", "contig"), ("shift", "contig"), ("contig", "pad_odd"), ("contig", "shift"), ("shift_pad16", "pad16")):
        pa, pg, ph = place(arow, lin, dtype, n, grades), place(grow, lin, dtype, n, grades), place(hrow, lin, dtype, n, grades)
        o = place_out(B, want.shape[1], lout, dtype, n, grades)
        w.eval_batch([pa.mv, pg.mv], ph.mv, B, out=o.mv)
        for p in (pa, pg, ph, o):
            p.check()
        assert np.array_equal(o.rows().view(np.uint8), want.view(np.uint8)), (lin, lout)
    Bs = 257
    rng = np.random.default_rng(SEED + 4)
    gm = rng.uniform(-1, 1, (Bs, grow.shape[1])).astype(NP[dtype])
    hm = rng.uniform(-1, 1, (Bs, hrow.shape[1])).astype(NP[dtype])
    shared = ga.DeviceMV.from_rows(n, grades, arow[:1], dtype)
    per = dl(w.eval_batch([shared, gm], hm, Bs))
    assert np.isfinite(per).all() and np.array_equal(per.view(np.uint8), dl(w.eval_batch([np.repeat(arow[:1], Bs, axis=0), gm], hm, Bs)).view(np.uint8))
    tot = dl(w.eval_batch([shared, gm], hm, Bs, reduce=True)).astype(np.float64)
    assert per.shape == (Bs, arow.shape[1]) and tot.shape == (1, arow.shape[1])
    per = per.astype(np.float64)
    exact = np.array([math.fsum(per[:, j]) for j in range(per.shape[1])])
    bound = (1024 + math.ceil(Bs / 1024)) * EPS[dtype] * np.sum(np.abs(per), axis=0)      # tests/test_gpu_gram_vjp.py: the row sum's bound
    assert np.all(np.abs(tot[0] - exact) <= bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_node_adds_into_a_buffer_another_term_has_written(dtype):
    """e + e adds the same node twice into one buffer: the second launch is not the first writer (beta = 1), and x + x is exact"""
    name = "PGA3D-even"
    metric, grades, N = g2.CASES[name]
    arow, grow, hrow = rows_of(name, dtype)
    B = len(arow)
    e = inp(0, grades, len(metric)).glog()
    twice = (e + e).specialize(ga.MetricAlgebra(metric), dtype=dtype, flags=FLAGS)
    w1, w2 = spec_of(name, dtype).vjp(0).vjp(0), twice.vjp(0).vjp(0)
    assert len(only(w1.launches(), "k_mv_adj2_glog<")) == 1 and len(only(w2.launches(), "k_mv_adj2_glog<")) == 2
    assert np.array_equal(dl(w2.eval_batch([arow, grow], hrow, B)).view(np.uint8), (2 * dl(w1.eval_batch([arow, grow], hrow, B))).view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_domain_error_item_is_nan_uncounted_and_leaves_its_neighbours_alone(dtype):
    """the operand -e_0 between good items of one workgroup"""
    name = "PGA3D"
    metric, grades, N = g2.CASES[name]
    A = np.array(data(name)["A"])
    arow, grow, hrow = rows_of(name, dtype)
    B = len(A)
    w = spec_of(name, dtype).vjp(0).vjp(0)
    good = dl(w.eval_batch([arow, grow], hrow, B))
    before = w.domain_errors()
    A[5, :] = 0
    A[5, 0] = -1.0
    got = dl(w.eval_batch([op_rows(metric, grades, A, dtype), grow], hrow, B))
    nan_rows = np.isnan(got).all(axis=1)
    assert list(np.flatnonzero(nan_rows)) == [5] and not np.isnan(got[~nan_rows]).any()
    assert np.array_equal(got[~nan_rows].view(np.uint8), good[~nan_rows].view(np.uint8))      # neighbours in the same wave: untouched
    assert errors(name, dtype, gx.to_s(metric, grades, got[~nan_rows].astype(np.float64)), ~nan_rows).max() <= bound_of(name, dtype)
    assert w.domain_errors() == before == 0                                                  # no forward step: nothing is counted


# ---- 3. the pose error: torch and central differences, f64 --------------------------------------------------------------------------
def _pose(flags=FLAGS, dtype=ga.F64):
    return (inp(0, [0, 2, 4], 4) * inp(1, [0, 2, 4], 4).inv()).glog().specialize(ga.MetricAlgebra(PGA), dtype=dtype, flags=flags)


def _motors(sel):
    """PGA3D motors gexp(B) with sum |B| = 0.1 and 1.0: the relative motor stays far from the cut"""
    metric, grades, N = g2.CASES["PGA3D-even"]
    return np.ascontiguousarray(gx.from_s(metric, grades, data("PGA3D-even")["A"][sel], grades))


def test_hessian_vector_products_of_the_pose_error_against_central_differences():
    """every second-order program of glog(a * b.inv()) against central differences of the GPU's own first-order gradient, 1e-6 relative"""
    rng = np.random.default_rng(SEED + 2)
    pose = _pose()
    a, b = _motors(slice(0, 3)), _motors(slice(1, 4))
    g = rng.uniform(-1, 1, (3, pose.output_info()[1]))
    for s1 in range(2):
        v = pose.vjp(s1)
        _check_vjp2(v, [a, b, g], rng, 3, h=1e-5, tol=1e-6)
        assert len(only(v.vjp(s1).launches(), "k_mv_adj2_glog<double,8>")) == 1
    assert pose.domain_errors() == 0


def test_torch_gradgradcheck_of_the_squared_pose_error():
    import torch
    f = _pose().torch_fn()
    loss = lambda a, b: (f(a, b) ** 2).sum(dim=1)
    xs = [torch.from_numpy(_motors(slice(0, 3))).cuda().requires_grad_(), torch.from_numpy(_motors(slice(1, 4))).cuda().requires_grad_()]
    assert torch.autograd.gradgradcheck(loss, xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    # a Hessian-vector product, as Newton-CG asks for it
    ga_, = torch.autograd.grad(loss(*xs).sum(), xs[0], create_graph=True)
    vec = torch.ones_like(xs[0])
    hv, = torch.autograd.grad((ga_ * vec).sum(), xs[0])
    assert torch.isfinite(hv).all() and hv.abs().max() > 0
    torch.cuda.synchronize()


def test_without_the_second_flag_double_backward_is_refused_in_todays_words():
    import torch
    f = _pose(flags=ga.FLAG_GSQRT_GLOG_JVP).torch_fn()
    xs = [torch.from_numpy(_motors(slice(0, 3))).cuda().requires_grad_(), torch.from_numpy(_motors(slice(1, 4))).cuda().requires_grad_()]
    gx_, = torch.autograd.grad(f(*xs).sum(), xs[0], create_graph=True)
    with pytest.raises(ga.GaastError) as ei:
        torch.autograd.grad(gx_.sum(), xs[0])
    assert ei.value.status_name == "UNIMPLEMENTED" and "GAAST_OP_GLOG_ADJ with respect to its operand" in str(ei.value)
    with pytest.raises(ga.GaastError) as ei:
        _pose(flags=ga.FLAG_GLOG_GRAD2).vjp(0).vjp(0)
    assert ei.value.status_name == "UNIMPLEMENTED" and "second-order reverse mode through GAAST_OP_GLOG_ADJ is not implemented" in str(ei.value)
    with pytest.raises(ga.GaastError) as ei:
        _pose().vjp(0).vjp(0).vjp(0)
    assert ei.value.status_name == "UNIMPLEMENTED" and "third-order reverse mode through GAAST_OP_GLOG_ADJ2" in str(ei.value)


# ---- 4. a Gram basis ----------------------------------------------------------------------------------------------------------------
def _move(q, n, grades, rows):
    """C_k(q) on every grade slice of the rows, in float64 (tests/test_gpu_gram_vjp.py: move)"""
    out, pos = np.empty_like(rows, dtype=np.float64), 0
    for k in sorted(grades):
        d = math.comb(n, k)
        out[:, pos:pos + d] = rows[:, pos:pos + d].astype(np.float64) @ linmap_compound(q, k).T
        pos += d
    return out


def test_second_order_in_the_cga_null_basis_is_the_moved_diagonal_program():
    """The Gram program is the diagonal-metric program between the compounds of Q: operand and both cotangents go in through C(Q^T), the
    result comes back through C(Q), every C_k(Q) orthogonal.  Bound per item, in the 2-norm: each side within 4 LOG_ADJ2_SCALE units of
    the exact value, and the 1e-12 norm-wise allowance of the existing Gram tests for the compounds on the way in and out, both times
    ||G||_inf ||h||_inf of the diagonal-metric item (the unit's factors) and sqrt N from the largest component to the 2-norm."""
    n, N, B = 5, 32, 4
    full = list(range(n + 1))
    alg = ga.GramAlgebra(CGA_GRAM)
    assert not alg.identity_basis()
    q, diag = alg.basis, [float(v) for v in alg.diag]
    rng = np.random.default_rng(SEED + 3)
    x = rng.uniform(-1, 1, (B, 32)) * 0.4 / 32
    x[:, 0] += 1.0                       # a dominant positive scalar, in any basis
    g, h = rng.uniform(-1, 1, (B, 32)), rng.uniform(-1, 1, (B, 32))
    mk = lambda a: inp(0, full, n).glog().specialize(a, flags=FLAGS)
    wg, wp = mk(alg).vjp(0).vjp(0), mk(ga.MetricAlgebra(diag)).vjp(0).vjp(0)
    assert only(wg.launches(), "k_mv_adj2_glog<double,32>") and any(l.startswith("linmap[") for l in wg.launches())
    assert only(wp.launches(), "k_mv_adj2_glog<double,32>") and not any(l.startswith("linmap[") for l in wp.launches())
    xf, gf, hf = (_move(q.T, n, full, r) for r in (x, g, h))
    got = dl(wg.eval_batch([x, g], h, B)).astype(np.float64)
    want = _move(q, n, full, dl(wp.eval_batch([xf, gf], hf, B)))
    xs, gs_, hs = (gx.to_s(diag, full, r) for r in (xf, gf, hf))
    unit = (2 * 4 * g2.scale_of(g2.LOG_ADJ2_SCALE, N, np.float64) * N * EPS[ga.F64] * np.maximum(1.0, np.abs(gl.log_reference(diag, full, xs)).sum(axis=1)).astype(np.float64) + 1e-12)
    bound = unit * g2.hessian_norm(diag, full, xs, gs_) * np.abs(hs).max(axis=1) * math.sqrt(N)
    err = np.linalg.norm(got - want, axis=1)
    assert np.isfinite(got).all() and np.abs(want).max() > 0.1 and np.all(err <= bound), (err / bound).max()
    assert inu.blade_set(n, tuple(full))[0] == 0
