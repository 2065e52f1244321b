"""Reverse mode through exp / log on the GPU (GAAST_FLAG_EXP_LOG | GAAST_FLAG_EXP_LOG_GRAD) against the closed-form numpy adjoint
of explog_grad_numpy.py in f64 (itself checked against central differences of the oracle, test_vjp_explog_host.py).

Bound, per component of the gradient:  C * eps(dtype) * Gamma * (1 + |B|_2^2) * max(|c0|, |f|, |h|)  with B the exp / log operand
of the item (log: its k-vector part), c0 / f / h of that operand (log: f, h), and Gamma = |g|_2 for a program that is ONE exp or
log.  In a composite program Gamma is the 2-norm of the cotangent that reaches the exp / log node (summed over the nodes: R and ~R
in a sandwich) and, for the gradient with respect to X, |g|_2 |R|_2^2.  f32 inputs are rounded first: both sides start from the
same f32 values.  Every case runs f64 and f32, the default / NO_FUSION / NO_JIT / DEBUG_JIT_FAILS / EXACT_ORDER plans (launch names
say whether k_exp_log_adj or the statements generated into gaast_jit ran), batches 1, 63, 257 and 1,000, contiguous and wrapped
(strided, misaligned) rows."""
import ctypes as C

import numpy as np
import pytest

import explog_grad_numpy as eg
import gaast_amd as ga
from gaast_amd import _lib
from layouts import place, place_out

pytestmark = pytest.mark.gpu
GRAD = ga.FLAG_EXP_LOG | ga.FLAG_EXP_LOG_GRAD
# NOT MEASURED.  The issue defines C as the next power of two at least 4x above the worst ratio measured on an MI355X; no run of
# this module on the GPU has been recorded yet, so C is PROVISIONAL and comes from a worst-case count of roundings instead, in units
# of eps * Gamma * (1 + |B|^2) * max(|c0|, |f|, |h|):
#   h by its quotient: the errors of the two transcendental results (<= 2 ulp each), of a / D (2 roundings), the subtraction and the
#     division, amplified by at most 10.4 (log at |u| = 1/4; exp: 3) ...................................... <= 10.4 * 4.5 = 47
#   d = sum g_k[i] B_i and s = sum sigma_i B_i^2, m terms each, s entering f and h with condition <= 1 ......... <= 2 m (m <= 10: 20)
#   f, the products and sums that assemble dB_i and da ............................................................ <= 8
# 75 for m <= 10, so C_BOUND = 128; for the m = 66 rows of the wide-row test 47 + 132 + 8 = 187, C_BOUND_WIDE = 256.  The same
# statements run on the host against glibc stay below 1.0.  Once measured: record the worst ratio here and in DESIGN.md section 11
# and replace both by the issue's rule (teardown_module prints the ratios).
C_BOUND = 128.0
C_BOUND_WIDE = 256.0
R3, R11, R31, PGA, CGA, R21 = [1.0] * 3, [1.0, -1.0], [-1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0, -1.0], [1.0, 1.0, -1.0]
PLANS = {"default": (0, "jit"), "no_fusion": (ga.FLAG_NO_FUSION, "kernel"), "no_jit": (ga.FLAG_NO_JIT, "kernel"),
         "jit_fails": (ga.FLAG_DEBUG_JIT_FAILS, "kernel"), "exact_order": (ga.FLAG_EXACT_ORDER, "jit")}
BATCHES = (1, 63, 257, 1000)
NPT = {ga.F64: np.float64, ga.F32: np.float32}
EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
WORST = {}


def teardown_module(module):
    for k in sorted(WORST):
        print(f"\nexp / log vjp worst ratio {k}: {WORST[k]:.3f} (C = {C_BOUND})")


def _wedge(n, rng, batch, scale=1.0):
    u, v = rng.uniform(-1, 1, (batch, n)), rng.uniform(-1, 1, (batch, n))
    cols = [(i, j) for j in range(n) for i in range(j)]
    return scale * np.stack([u[:, i] * v[:, j] - u[:, j] * v[:, i] for i, j in cols], axis=1)


def _translator(rng, batch):
    rows = np.zeros((batch, 6))       # components e01, e02, e03 (the ones that hold e_0): s == 0 exactly
    rows[:, [0, 1, 3]] = rng.uniform(-1, 1, (batch, 3))
    return rows


def _screw(rng, batch):
    rows = _wedge(4, rng, batch, 0.8)  # a general screw: a simple bivector plus a translation along its axis (square not scalar:
    rows[:, [0, 1, 3]] += rng.uniform(-0.5, 0.5, (batch, 3))   # the closed form applies to <B B>_0, the forward counts the item)
    return rows


def _boost(rng, batch):
    rows = np.zeros((batch, 6))
    rows[:, 0] = rng.uniform(-2.5, 2.5, batch)                  # e01, e_0 time-like: s > 0, on both sides of |s| = 4
    return rows


# name: (metric, k, op, input grades, rows(rng, batch))
SINGLE = {
    "r3_bivector": (R3, 2, "exp", [2], lambda r, b: r.uniform(-1.5, 1.5, (b, 3))),
    "r11_bivector": (R11, 2, "exp", [2], lambda r, b: r.uniform(-2.5, 2.5, (b, 1))),       # s up to 6.25: series and quotient
    "r31_boost": (R31, 2, "exp", [2], _boost),
    "pga_bivector": (PGA, 2, "exp", [2], lambda r, b: _wedge(4, r, b, 0.8)),
    "pga_translator": (PGA, 2, "exp", [2], _translator),
    "pga_screw": (PGA, 2, "exp", [2], _screw),
    "pga_series_1e-8": (PGA, 2, "exp", [2], lambda r, b: _wedge(4, r, b, 1e-8)),
    "pga_series_1e-4": (PGA, 2, "exp", [2], lambda r, b: _wedge(4, r, b, 1e-4)),
    "cga_bivector": (CGA, 2, "exp", [2], lambda r, b: _wedge(5, r, b, 0.7)),
    "cga_log": (CGA, 2, "log", [0, 2], lambda r, b: np.concatenate([r.uniform(1.5, 3.0, (b, 1)), _wedge(5, r, b, 0.5)], axis=1)),
    # a of either sign over s < 0 (a < 0: atan2 beyond pi / 2, the quotient only), and a < 0 over s > 0 (atanh of a negative ratio)
    "r3_log_any_sign": (R3, 2, "log", [0, 2], lambda r, b: np.concatenate([r.uniform(-2.0, 2.0, (b, 1)), r.uniform(-1.5, 1.5, (b, 3))], axis=1)),
    "r11_log_negative_a": (R11, 2, "log", [0, 2], lambda r, b: np.concatenate([r.uniform(-3.0, -1.5, (b, 1)), r.uniform(-1.2, 1.2, (b, 1))], axis=1)),
    "r21_vector": (R21, 1, "exp", [1], lambda r, b: r.uniform(-1.5, 1.5, (b, 3))),
}


def _inp(slot, grades, n):
    return ga.mv(ga.Input(slot, grades, n))


def _grades(mask):
    return [k for k in range(17) if (mask >> k) & 1]


def _assert_form(v, form):
    names = v.launches()
    if form == "jit":
        assert len(names) == 1 and names[0].startswith("ast_jit"), names
    else:
        assert any("_adjoint[" in l and ":: k_exp_log_adj<" in l for l in names), names
        assert not any("ast_jit" in l for l in names), names


def _run(v, n, in_grades, rows, out_grades, g, wrt_grades, batch, dtype, wrapped, shared=()):
    """gradient rows of Vjp `v`: rows[slot] / g as host arrays; wrapped: every batched buffer strided and misaligned"""
    if not wrapped:
        out = v.eval_batch(rows, g, batch)
        ga.lib().gaast_hip_synchronize()
        return out.download_rows().astype(np.float64)
    lay_in, lay_out = ("shift_pad16", "pad_odd") if dtype == ga.F64 else ("shift3", "pad_odd3")
    ins = [place(r, "shared" if s in shared else lay_in, dtype, n, in_grades[s]) for s, r in enumerate(rows)]
    cot = place(g, lay_out, dtype, n, out_grades)
    o = place_out(batch, len(eg.blades_in_row_order(n, wrt_grades)), lay_in, dtype, n, wrt_grades)
    v.eval_batch([p.mv for p in ins], cot.mv, batch, out=o.mv)
    for p in ins + [cot]:
        p.check()
    o.check()
    return o.rows().astype(np.float64)


def _check(key, got, want, gamma, Bk_norm2, scale, dtype, c=None):
    bound = EPS[dtype] * gamma * (1.0 + Bk_norm2) * scale
    finite = np.isfinite(bound) & (bound > 0)
    ratio = float(np.max(np.abs(got - want)[finite] / np.broadcast_to(bound[:, None], got.shape)[finite])) if finite.any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= (C_BOUND if c is None else c), (key, ratio)


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_one_exp_or_log(name, dtype, plan):
    metric, k, op, grades, rows_of = SINGLE[name]
    n, alg = len(metric), eg.Algebra(metric)
    flags, form = PLANS[plan]
    x = _inp(0, grades, n)
    spec = (x.exp() if op == "exp" else x.log()).specialize(metric, dtype=dtype, flags=GRAD | flags)
    out_grades = _grades(spec.output_info()[0])
    v = spec.vjp(0)
    _assert_form(v, form)
    rng = np.random.default_rng(sorted(SINGLE).index(name))
    for batch in BATCHES:
        rows = rows_of(rng, batch).astype(NPT[dtype])
        g = rng.uniform(-1, 1, (batch, spec.output_info()[1])).astype(NPT[dtype])
        bits, gbits = eg.rows_to_bits(n, grades, rows), eg.rows_to_bits(n, out_grades, g)
        want = eg.exp_adjoint(alg, k, bits, gbits) if op == "exp" else eg.log_adjoint(alg, k, bits, gbits)
        want = eg.bits_to_rows(n, grades, want)
        Bk = bits * alg.grade_mask([k])
        for wrapped in (False, True):
            got = _run(v, n, [grades], [rows], out_grades, g, grades, batch, dtype, wrapped)
            _check(f"{op} {'f64' if dtype == ga.F64 else 'f32'}", got, want, np.linalg.norm(g.astype(np.float64), axis=1),
                   np.sum(Bk * Bk, axis=1), eg.scale_of(alg, k, op, bits), dtype)


def _sandwich_reference(alg, B, X, G):
    """R = exp(B), Y = <(R X) ~R>_1; returns (dB, dX, cotangent norms reaching exp, |R|^2)"""
    R = eg.exp_forward(alg, 2, B)
    RX = alg.gp(R, X)
    G1 = G * alg.grade_mask([1])
    d_rx, d_rrev = alg.gp_vjp(RX, alg.rev(R), G1)
    d_r1, dX = alg.gp_vjp(R, X, d_rx)
    d_r2 = alg.rev(d_rrev)
    keep = alg.grade_mask([0, 2])
    dB = eg.exp_adjoint(alg, 2, B, d_r1 * keep) + eg.exp_adjoint(alg, 2, B, d_r2 * keep)
    gamma = np.linalg.norm(d_r1 * keep, axis=1) + np.linalg.norm(d_r2 * keep, axis=1)
    return dB, dX * alg.grade_mask([1]), gamma, np.sum(R * R, axis=1)


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
@pytest.mark.parametrize("name,metric", [("r3", R3), ("pga", PGA)])
def test_sandwich_with_respect_to_generator_and_point(name, metric, dtype, plan):
    n, alg = len(metric), eg.Algebra(metric)
    flags, form = PLANS[plan]
    r = _inp(0, [2], n).exp()
    spec = (r * _inp(1, [1], n) * r.rev()).g(1).specialize(metric, dtype=dtype, flags=GRAD | flags)
    vb, vx = spec.vjp(0), spec.vjp(1)
    _assert_form(vb, form)
    if plan == "default":   # one launch whenever the forward is
        assert len(spec.launches()) == 1 and len(vb.launches()) == 1
    rng = np.random.default_rng(n)
    m = n * (n - 1) // 2
    for batch in BATCHES:
        for shared in ((), (0,)):
            Brows = (rng.uniform(-1, 1, (1 if shared else batch, m)) if n == 3 else _wedge(n, rng, 1 if shared else batch, 0.8)).astype(NPT[dtype])
            Xrows = rng.uniform(-1, 1, (batch, n)).astype(NPT[dtype])
            g = rng.uniform(-1, 1, (batch, n)).astype(NPT[dtype])
            B = np.repeat(eg.rows_to_bits(n, [2], Brows), batch if shared else 1, axis=0)
            dB, dX, gamma, r2 = _sandwich_reference(alg, B, eg.rows_to_bits(n, [1], Xrows), eg.rows_to_bits(n, [1], g))
            scale, b2 = eg.scale_of(alg, 2, "exp", B), np.sum(B * B, axis=1)
            for wrapped in (False, True):
                got = _run(vb, n, [[2], [1]], [Brows, Xrows], [1], g, [2], batch, dtype, wrapped, shared)
                _check(f"sandwich dB {'f64' if dtype == ga.F64 else 'f32'}", got, eg.bits_to_rows(n, [2], dB), gamma, b2, scale, dtype)
                got = _run(vx, n, [[2], [1]], [Brows, Xrows], [1], g, [1], batch, dtype, wrapped, shared)
                _check(f"sandwich dX {'f64' if dtype == ga.F64 else 'f32'}", got, eg.bits_to_rows(n, [1], dX),
                       np.linalg.norm(g.astype(np.float64), axis=1) * r2, b2, scale, dtype)
            if shared and batch > 1:   # the gradient of the shared generator: sum_rows of the per-item rows
                tot = vb.eval_batch([Brows, Xrows], g, batch, reduce=True).download_rows().astype(np.float64)
                want = eg.bits_to_rows(n, [2], dB).sum(axis=0)
                bound = C_BOUND * EPS[dtype] * np.sum(gamma * (1 + b2) * scale) + (1024 + 2) * EPS[dtype] * np.abs(eg.bits_to_rows(n, [2], dB)).sum(axis=0)
                assert tot.shape == (1, m) and np.all(np.abs(tot[0] - want) <= bound)


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_log_of_exp_returns_the_cotangent(dtype, plan):
    flags, form = PLANS[plan]
    spec = _inp(0, [2], 3).exp().log().specialize(3, dtype=dtype, flags=GRAD | flags)
    v = spec.vjp(0)
    _assert_form(v, form)
    alg, rng = eg.Algebra(R3), np.random.default_rng(17)
    for batch in BATCHES:
        rows = rng.uniform(-0.8, 0.8, (batch, 3)).astype(NPT[dtype])     # |B| < pi: the principal branch
        g = rng.uniform(-1, 1, (batch, 3)).astype(NPT[dtype])
        B = eg.rows_to_bits(3, [2], rows)
        R = eg.exp_forward(alg, 2, B)
        d_r = eg.log_adjoint(alg, 2, R, eg.rows_to_bits(3, [2], g))
        gamma = np.linalg.norm(g.astype(np.float64), axis=1) + np.linalg.norm(d_r, axis=1)
        scale = np.maximum(eg.scale_of(alg, 2, "exp", B), eg.scale_of(alg, 2, "log", R))
        for wrapped in (False, True):
            got = _run(v, 3, [[2]], [rows], [2], g, [2], batch, dtype, wrapped)
            _check(f"log(exp) {'f64' if dtype == ga.F64 else 'f32'}", got, g.astype(np.float64), gamma, np.sum(B * B, axis=1), scale, dtype)


def _raw_unary_program(opcode, in_mask, node_mask, n, metric, dtype, flags):
    nodes = (_lib.NodeDesc * 2)()
    for nd in nodes:
        nd.child0 = nd.child1 = nd.input_slot = -1
        nd.vec_space_dim, nd.product_kind = n, _lib.PROD_EXPLICIT
    nodes[0].opcode, nodes[0].input_slot, nodes[0].minimal_grade_mask = _lib.OP_INPUT, 0, in_mask
    nodes[1].opcode, nodes[1].child0, nodes[1].minimal_grade_mask = opcode, 0, node_mask
    inputs = (_lib.InputDesc * 1)()
    inputs[0].grade_mask, inputs[0].storage_dim = in_mask, n
    m = (C.c_double * n)(*metric)
    desc = _lib.ProgramDesc()
    desc.vec_space_dim, desc.metric_diag, desc.dtype = n, m, dtype
    desc.n_nodes, desc.nodes, desc.root = 2, nodes, 1
    desc.n_inputs, desc.inputs, desc.flags = 1, inputs, flags
    return desc, (nodes, inputs, m)


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_log_of_a_bare_bivector_through_the_raw_abi(dtype, plan):
    """phases 1-3 refuse log(<A>_2) like the reference; a host can hand INPUT {2} -> LOG {2} over: the operand has no grade 0
    (a reads 0, no da).  CGA bivectors of the Euclidean part (s < 0: f = pi / (2 m))."""
    L = _lib.lib()
    _lib.init_device()
    flags, form = PLANS[plan]
    desc, keep = _raw_unary_program(_lib.OP_LOG, 1 << 2, 1 << 2, 5, CGA, dtype, GRAD | flags)
    prog = C.c_void_p()
    _lib.check(L.gaast_hip_program_create_vjp(C.byref(desc), 0, C.byref(prog)))
    names = [L.gaast_hip_program_launch_name(prog, i).decode() for i in range(L.gaast_hip_program_num_launches(prog))]
    if form == "jit":
        assert len(names) == 1 and names[0].startswith("ast_jit"), names
    else:
        assert any("logarithm_adjoint[" in x and ":: k_exp_log_adj<" in x for x in names) and not any("ast_jit" in x for x in names), names
    rng, alg = np.random.default_rng(23), eg.Algebra(CGA)
    cols = [(i, j) for j in range(5) for i in range(j)]
    lay_in, lay_out = ("shift_pad16", "pad_odd") if dtype == ga.F64 else ("shift3", "pad_odd3")
    for batch in BATCHES:
        uv = rng.uniform(-1, 1, (batch, 10))
        uv[:, [4, 9]] = 0.0
        rows = np.stack([uv[:, i] * uv[:, 5 + j] - uv[:, j] * uv[:, 5 + i] for i, j in cols], axis=1).astype(NPT[dtype])
        g = rng.uniform(-1, 1, (batch, 10)).astype(NPT[dtype])
        bits = eg.rows_to_bits(5, [2], rows)
        want = eg.bits_to_rows(5, [2], eg.log_adjoint(alg, 2, bits, eg.rows_to_bits(5, [2], g), with_scalar=False))
        for wrapped in (False, True):
            if wrapped:
                a, b = place(rows, lay_in, dtype, 5, [2]), place(g, lay_out, dtype, 5, [2])
                o = place_out(batch, 10, lay_in, dtype, 5, [2])
                ins, out = (C.c_void_p * 2)(a.mv._h, b.mv._h), o.mv
            else:
                a, b = ga.DeviceMV.from_rows(5, [2], rows, dtype=dtype), ga.DeviceMV.from_rows(5, [2], g, dtype=dtype)
                ins, out = (C.c_void_p * 2)(a._h, b._h), ga.DeviceMV.alloc(5, ga.GradeSet(1 << 2), batch, dtype)
            _lib.check(L.gaast_hip_eval(prog, ins, 2, batch, out._h))
            _lib.check(L.gaast_hip_synchronize())
            if wrapped:
                a.check(), b.check(), o.check()
                got = o.rows().astype(np.float64)
            else:
                got = out.download_rows().astype(np.float64)
            _check(f"log bare {'f64' if dtype == ga.F64 else 'f32'}", got, want, np.linalg.norm(g.astype(np.float64), axis=1),
                   np.sum(bits * bits, axis=1), eg.scale_of(alg, 2, "log", bits), dtype)
    _lib.check(L.gaast_hip_program_destroy(prog))


@pytest.mark.parametrize("dtype,suffix", [(ga.F64, "[direct rows]"), (ga.F32, "[64 items through LDS]")])
def test_wide_rows_take_the_smaller_staged_form_and_the_direct_form(dtype, suffix):
    """R^12 bivectors (m = 66; cotangent row 67): 133 elements per item leave 64 items in the 64 KiB of LDS in f32 and none in
    f64 (every thread on its own rows).  Every blade squares to -1; the closed form needs no dense product table."""
    n, m, batch = 12, 66, 257
    spec = _inp(0, [2], n).exp().specialize(n, dtype=dtype, flags=GRAD | ga.FLAG_NO_FUSION)
    v = spec.vjp(0)
    hits = [l for l in v.launches() if "exponential_adjoint[" in l]
    assert len(hits) == 1 and ":: k_exp_log_adj<" in hits[0] and hits[0].endswith(suffix), v.launches()
    rng = np.random.default_rng(12)
    rows = _wedge(n, rng, batch, 0.6).astype(NPT[dtype])
    rows[:8] *= 4.0                                               # |s| beyond 4: the quotient
    g = rng.uniform(-1, 1, (batch, m + 1)).astype(NPT[dtype])
    B, g0, gk = rows.astype(np.float64), g[:, 0].astype(np.float64), g[:, 1:].astype(np.float64)
    sq = -np.sum(B * B, axis=1)
    c0, f = eg.exp_c0_f(sq)
    h, d = eg.exp_h(sq), np.sum(gk * B, axis=1)
    want = f[:, None] * gk - B * (f * g0 + h * d)[:, None]
    scale = np.maximum(np.maximum(np.abs(c0), np.abs(f)), np.abs(h))
    for wrapped in (False, True):
        got = _run(v, n, [[2]], [rows], [0, 2], g, [2], batch, dtype, wrapped)
        _check(f"exp m=66 {'f64' if dtype == ga.F64 else 'f32'}", got, want, np.linalg.norm(g.astype(np.float64), axis=1), -sq, scale, dtype,
               c=C_BOUND_WIDE)


def test_an_adjoint_opcode_without_the_exp_log_flag_is_refused():
    L = _lib.lib()
    _lib.init_device()
    spec = (_inp(0, [2], 3).exp() * _inp(1, [2], 3)).specialize(3, flags=GRAD)
    v = spec.vjp(0)
    d = _lib.ProgramDesc()
    C.memmove(C.byref(d), C.byref(v.desc), C.sizeof(d))
    d.flags = ga.FLAG_EXP_LOG_GRAD
    prog = C.c_void_p()
    assert _lib.STATUS_NAMES[L.gaast_hip_program_create(C.byref(d), C.byref(prog))] == "UNIMPLEMENTED"
    assert not prog.value


@pytest.mark.parametrize("flags", [0, ga.FLAG_NO_FUSION])
@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_inf_and_nan_propagate_and_the_domain_counter_is_left_alone(dtype, flags):
    n, batch = 4, 130
    spec = _inp(0, [2], n).exp().specialize(PGA, dtype=dtype, flags=GRAD | flags)
    v = spec.vjp(0)
    rng = np.random.default_rng(5)
    rows = _screw(rng, batch).astype(NPT[dtype])       # squares that are not scalar: a forward would count every item
    bad = {3: np.nan, 64: np.inf, 129: -np.inf}
    for i, x in bad.items():
        rows[i, 2] = x
    g = rng.uniform(-1, 1, (batch, 7)).astype(NPT[dtype])
    got = v.eval_batch([rows], g, batch).download_rows()
    good = [i for i in range(batch) if i not in bad]
    assert np.all(np.isfinite(got[good])) and not np.any(np.isfinite(got[list(bad)]).all(axis=1))
    # the program holds only the adjoint node: no domain check, the counter stays where it was
    assert not any("exponential[" in l for l in v.launches())
    cnt = C.c_int64(-1)
    _lib.check(_lib.lib().gaast_hip_program_domain_errors(v.program(), C.byref(cnt)))
    assert cnt.value == 0


@pytest.mark.parametrize("dtype", [ga.F64, ga.F32])
def test_exact_order_gives_the_same_bits_twice(dtype):
    r = _inp(0, [2], 4).exp()
    rng = np.random.default_rng(6)
    rows = [_wedge(4, rng, 257, 0.8).astype(NPT[dtype]), rng.uniform(-1, 1, (257, 4)).astype(NPT[dtype])]
    g = rng.uniform(-1, 1, (257, 4)).astype(NPT[dtype])
    for flags in (0, ga.FLAG_NO_FUSION):
        v = (r * _inp(1, [1], 4) * r.rev()).g(1).specialize(PGA, dtype=dtype, flags=GRAD | ga.FLAG_EXACT_ORDER | flags).vjp(0)
        first = v.eval_batch(rows, g, 257).download_rows()
        assert np.array_equal(v.eval_batch(rows, g, 257).download_rows(), first)


# ---- torch -----------------------------------------------------------------------------------------------------------
def test_torch_gradcheck_motor_sandwich_with_a_shared_generator():
    import torch
    r = _inp(0, [2], 4).exp()
    spec = (r * _inp(1, [3], 4) * r.rev()).g(3).specialize(PGA, flags=GRAD)
    gen = torch.Generator().manual_seed(0)
    xs = [torch.rand(s, generator=gen, dtype=torch.float64).mul(2).sub(1).cuda().requires_grad_() for s in [(1, 6), (5, 4)]]
    assert torch.autograd.gradcheck(spec.torch_fn(), xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


def test_torch_gradcheck_log_of_exp():
    import torch
    spec = _inp(0, [2], 3).exp().log().specialize(3, flags=GRAD)
    gen = torch.Generator().manual_seed(1)
    xs = [torch.rand((4, 3), generator=gen, dtype=torch.float64).mul(1.6).sub(0.8).cuda().requires_grad_()]
    assert torch.autograd.gradcheck(spec.torch_fn(), xs, eps=1e-6, atol=1e-7, rtol=1e-6)
    torch.cuda.synchronize()


def test_torch_fn_without_the_grad_flag_still_raises():
    import torch
    spec = (_inp(0, [2], 3).exp() * _inp(1, [2], 3)).specialize(3, flags=ga.FLAG_EXP_LOG)
    xs = [torch.rand((4, 3), dtype=torch.float64).cuda().requires_grad_() for _ in range(2)]
    y = spec.torch_fn()(*xs)
    with pytest.raises(ga.GaastError) as ei:
        y.backward(torch.ones_like(y))
    assert ei.value.status_name == "UNIMPLEMENTED"
    torch.cuda.synchronize()
