"""Forward mode through the general square root and logarithm, and any-order reverse mode of the root (GAAST_OP_GSQRT_JVP /
GAAST_OP_GLOG_JVP, GAAST_FLAG_GSQRT_GLOG_JVP) on the host: the numpy restatement of the two tangents (root_log_jvp_numpy.py) against
central differences, the transposition identity and the composed second-order rule, the error scales of the restatement that bound
the GPU tests, the images gaast_program_vjp builds with and without the flag, and the lowered Step::GSQRT_JVP / Step::GLOG_JVP
tables.  No GPU.

The host code is also compiled into a stand-alone program with -fsanitize=address,undefined
(tests/cpp/root_log_jvp_sanitize_driver.cpp) and run once: it must end clean, and the tables it prints from the lowered plans are what
the tests below compare with numpy.

Bounds.  The restatement checks run in numpy.longdouble (eps = 1.1e-19).  Transposition compares two evaluations of one bilinear form
through at most 5 + 14 solves of condition below 1e3 on these operands: 1e-15 of sum |g| |J h| is a thousand times that.  The
central differences use the step 1e-6: truncation is t^2 |f'''| / 6, relative to |f'| at most 1e-12 times the ratio of the third to the
first derivative, which is about 2 / |A|^2 = 2e4 ... 1e5 for the operands scaled by 0.01 (derivatives of log grow like |A|^-k): up to
1e-7; rounding is the forward's 1e-18 |f| / t = 1e-12 |f|, with |f| / |f'| below 1e3.  The bound is 1e-6 relative (measured: up to
5e-8); a wrong formula misses by a percent at the least.

Mutation check: leaving out the factor 2^s moves log_jvp by order one on these operands, and taking L's sign word in both Pade passes
by a percent (the M_j are close to 1, where left and right multiplication nearly agree); both are asserted below to move it by more
than 1e-3, so the identities of test_restatement_in_longdouble (1e-15 and 1e-6) fail for either.  Exchanging L's and R's words between the two
passes is no mutation: left and right multiplications commute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gaast_amd as ga
from gaast_amd import _lib

import gexp_numpy as gx
import glog_numpy as gl
import gsqrt_numpy as gs
import inverse_numpy as inu
import root_log_jvp_numpy as rl
import test_vjp_host as H
from helpers import plan_sources
from test_vjp2_host import _check_shape, _image, _ok, _serialize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGA = [0.0, 1.0, 1.0, 1.0]
CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
ODD = [2.0, -0.5, 1.0]
SEED = 20261021
FLAG = ga.FLAG_GSQRT_GLOG_JVP
LD = np.longdouble


def test_constants():
    assert (_lib.OP_GSQRT_JVP, _lib.OP_GLOG_JVP, ga.FLAG_GSQRT_GLOG_JVP) == (24, 25, 0x8000)
    assert _lib.OP_NAMES[24] == "GeneralSqrtJvp" and _lib.OP_NAMES[25] == "GeneralLogarithmJvp" and len(_lib.OP_NAMES) == 26


# ---- the restatement, in longdouble -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rl.CASES))
def test_restatement_in_longdouble(name):
    metric, grades, N = rl.CASES[name]
    rng = np.random.default_rng(SEED)
    A, h, g = rl.sweep_operands(name, rng)
    Al, hl, gl_ = A.astype(LD), h.astype(LD), g.astype(LD)
    uj, lj = rl.sqrt_jvp_reference(metric, grades, A, h), rl.log_jvp_reference(metric, grades, A, h)
    assert np.isfinite(uj).all() and np.isfinite(lj).all()
    # the transposition identity against the two reverse modes
    rs = gs.reverse(metric, grades, Al, g, LD, X=gs.root_reference(metric, grades, A))
    rg = gl.reverse_reference(metric, grades, A, g)
    for tag, jv, rv in (("SQRT", uj, rs), ("LOG", lj, rg)):
        lhs, rhs = (gl_ * jv).sum(axis=1), (rv * hl).sum(axis=1)
        scale = (np.abs(gl_) * np.abs(jv)).sum(axis=1)
        print(f"TRANSPOSITION {tag} {name}: {float((np.abs(lhs - rhs) / scale).max()):.2e}")
        assert np.all(np.abs(lhs - rhs) <= 1e-15 * scale)
    # central differences of the two references
    t = LD(1e-6)
    for tag, f, jv in (("SQRT", lambda X: gs.root_reference(metric, grades, X), uj), ("LOG", lambda X: gl.log_reference(metric, grades, X), lj)):
        fd = (f(Al + t * hl) - f(Al - t * hl)) / (2 * t)
        rel = float((np.abs(fd - jv).max(axis=1) / np.abs(jv).max(axis=1)).max())
        print(f"JVP-VS-DIFFERENCES {tag} {name}: {rel:.2e}")
        assert rel <= 1e-6
    # the composed second-order rule of gsqrt: central differences in A of <reverse(A, g), h> along d
    d = rng.uniform(-1, 1, A.shape).astype(LD)
    a2 = rl.sqrt_adj2(metric, grades, A, g, h)
    phi = lambda X: (gs.reverse(metric, grades, X, g, LD, X=gs.root_reference(metric, grades, X)) * hl).sum(axis=1)
    fd2 = (phi(Al + t * d) - phi(Al - t * d)) / (2 * t)
    rel2 = float((np.abs(fd2 - (a2 * d).sum(axis=1)) / (np.abs(a2) * np.abs(d)).sum(axis=1)).max())
    print(f"ADJ2-VS-DIFFERENCES {name}: {rel2:.2e}")
    assert rel2 <= 1e-6
    # the mutations move the tangent of the logarithm by far more than the identities above allow
    for kw in (dict(drop_scale=True), dict(both_left=True)):
        if N == 2 and "both_left" in kw:
            continue                     # R^1 is commutative: L = R
        m = rl.log_jvp(metric, grades, A, h, LD, **gl._ref_kw(), **kw)
        assert float((np.abs(m - lj).max(axis=1) / np.abs(lj).max(axis=1)).max()) > 1e-3, kw


def test_domain_errors_of_the_restatement():
    A = np.array([[-1.0, 0, 0, 0], [1.25, 0.25, 0, 0], [1.0, np.nan, 0, 0]])
    ones = np.ones_like(A)
    for out in (rl.sqrt_jvp([1.0, 1.0], [0, 1, 2], A, ones), rl.log_jvp([1.0, 1.0], [0, 1, 2], A, ones)):
        assert np.isnan(out[[0, 2]]).all() and np.isfinite(out[1]).all()


# ---- the scales of the GPU bounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(rl.CASES))
def test_restatement_error_defines_the_scales(name, dtype):
    """the worst error of the restatement in the program's dtype against the longdouble reference over the sweep: covered by the
    recorded scale"""
    metric, grades, N = rl.CASES[name]
    eps = rl.EPS[np.dtype(dtype)]
    A, h, _ = rl.case_operands(name)           # the items of the GPU tests: 257 at N = 2, twelve (nine at N = 64) otherwise
    kappa = rl.sum_condition(metric, grades, gs.root_reference(metric, grades, A).astype(np.float64))
    ref = gl.log_reference(metric, grades, A).astype(np.float64)
    jn = gl.jacobian_norm(metric, grades, A, of_j=True)
    ws = rl.sqrt_jvp_error(rl.sqrt_jvp(metric, grades, A, h, dtype), rl.sqrt_jvp_reference(metric, grades, A, h), eps, kappa).max()
    wl = rl.log_jvp_error(rl.log_jvp(metric, grades, A, h, dtype), rl.log_jvp_reference(metric, grades, A, h), eps, ref, jn, h).max()
    print(f"SCALES {name} {np.dtype(dtype).name}: SQRT_JVP {ws:.3f}  LOG_JVP {wl:.3f}")
    assert ws <= rl.scale_of(rl.SQRT_JVP_SCALE, N, dtype), (name, ws)
    assert wl <= rl.scale_of(rl.LOG_JVP_SCALE, N, dtype), (name, wl)


# ---- images -------------------------------------------------------------------------------------------------------------------------
def _gsqrt(B):
    return B.input(0, [0, 2], 3).gsqrt()


def _glog(B):
    return B.input(0, [0, 2], 3).glog()


def _gsqrt_times(B):
    return B.input(0, [0, 2], 3).gsqrt() * B.input(1, [0, 2], 3)


def _pose_error(B):
    return (B.input(0, [0, 2, 4], 4) * B.input(1, [0, 2, 4], 4).inv()).glog()


def _ops(a):
    return [a.nodes[i].opcode for i in range(a.n_nodes)]


def _kinds(a):
    return sorted(a.nodes[i].product_kind for i in range(a.n_nodes) if a.nodes[i].opcode == _lib.OP_PRODUCT)


def _reads_slot(a, slot):
    return any(a.nodes[i].opcode == _lib.OP_INPUT and a.nodes[i].input_slot == slot for i in range(a.n_nodes))


def _same_but_flags(x, y):
    bx, by = bytearray(_serialize(x)), bytearray(_serialize(y))
    diff = [i for i in range(len(bx)) if bx[i] != by[i]] if len(bx) == len(by) else None
    return diff is not None and len(diff) == 1 and (by[diff[0]] ^ bx[diff[0]]) == (FLAG >> 8) and x.flags ^ y.flags == FLAG


def test_forward_mode_images_hold_exactly_one_tangent_node():
    for build, op_adj, op_jvp in ((_gsqrt, _lib.OP_GSQRT_ADJ, _lib.OP_GSQRT_JVP), (_glog, _lib.OP_GLOG_ADJ, _lib.OP_GLOG_JVP)):
        d = H._desc(build, 3, flags=FLAG)
        a = _ok(d, 0)
        j = _ok(a, d.n_inputs)            # forward mode: the VJP of the VJP with respect to its cotangent
        _check_shape(a, d.n_inputs, j)
        assert _ops(j).count(op_jvp) == 1 and op_adj not in _ops(j) and not _reads_slot(j, d.n_inputs)
        nd = next(j.nodes[i] for i in range(j.n_nodes) if j.nodes[i].opcode == op_jvp)
        assert j.nodes[nd.child1].input_slot == 0 and j.nodes[nd.child0].input_slot == a.n_inputs and nd.input_slot == -1
        assert nd.minimal_grade_mask == d.nodes[d.root].minimal_grade_mask
        t = _ok(j, a.n_inputs)            # its transpose is the first-order gradient again
        assert _ops(t).count(op_adj) == 1 and op_jvp not in _ops(t)


def test_gsqrt_differentiates_to_any_order():
    """the node census of the rule table: -GSQRT_ADJ(ADJ_LEFT(w, u) + ADJ_RIGHT(w, u), A), w = GSQRT_ADJ(g, A), u = GSQRT_JVP(-k, A)"""
    d = H._desc(_gsqrt, 3, flags=FLAG)
    a = _ok(d, 0)
    h = _ok(a, 0)
    _check_shape(a, 0, h)
    ops = _ops(h)
    assert (ops.count(_lib.OP_GSQRT_ADJ), ops.count(_lib.OP_GSQRT_JVP), ops.count(_lib.OP_NEG), ops.count(_lib.OP_ADD), ops.count(_lib.OP_PRODUCT),
            ops.count(_lib.OP_INPUT)) == (2, 1, 1, 1, 2, 3) and len(ops) == 10
    assert _kinds(h) == [_lib.PROD_GEOMETRIC + _lib.PROD_ADJ_LEFT, _lib.PROD_GEOMETRIC + _lib.PROD_ADJ_RIGHT]
    smask = 0b101
    root = h.nodes[h.root]
    assert root.opcode == _lib.OP_GSQRT_ADJ and h.nodes[root.child0].opcode == _lib.OP_ADD and h.nodes[root.child1].input_slot == 0
    for i in range(h.n_nodes):
        nd = h.nodes[i]
        if nd.opcode == _lib.OP_NEG:      # on the innermost child: the second cotangent itself
            assert h.nodes[nd.child0].opcode == _lib.OP_INPUT and h.nodes[nd.child0].input_slot == a.n_inputs
        if nd.opcode == _lib.OP_GSQRT_JVP:
            assert h.nodes[nd.child0].opcode == _lib.OP_NEG and nd.minimal_grade_mask == smask
        if nd.opcode == _lib.OP_PRODUCT:
            assert (h.nodes[nd.child0].opcode, h.nodes[nd.child1].opcode) == (_lib.OP_GSQRT_ADJ, _lib.OP_GSQRT_JVP)
    # a third order builds in every slot, and a fourth in one
    for s in H._user_slots(h):
        t3 = _ok(h, s)
        _check_shape(h, s, t3)
    assert _ok(_ok(h, 0), 0).n_nodes > h.n_nodes
    # with a second operand: every pair of slots
    d2 = H._desc(_gsqrt_times, 3, flags=FLAG)
    for s1 in H._user_slots(d2):
        a1 = _ok(d2, s1)
        for s2 in H._user_slots(a1):
            _check_shape(a1, s2, _ok(a1, s2))


def test_glog_is_refused_only_where_its_operand_is_on_the_path():
    d = H._desc(_glog, 3, flags=FLAG)
    a = _ok(d, 0)
    st, _ = _image(a, 0)
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
    msg = _lib.lib().gaast_expr_last_error().decode()
    assert "GAAST_OP_GLOG_ADJ" in msg and "with respect to its operand" in msg
    j = _ok(a, d.n_inputs)
    st, _ = _image(j, 0)                  # the tangent node's operand
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED" and "GAAST_OP_GLOG_JVP" in _lib.lib().gaast_expr_last_error().decode()
    # the pose error: forward mode in both slots
    p = H._desc(_pose_error, PGA, flags=FLAG)
    for s in H._user_slots(p):
        jp = _ok(_ok(p, s), p.n_inputs)
        assert _ops(jp).count(_lib.OP_GLOG_JVP) == 1 and _lib.OP_GLOG_ADJ not in _ops(jp)
    two = H._desc(lambda B: B.input(0, [0, 2], 3).glog() * B.input(1, [0, 2], 3), 3, flags=FLAG)
    a1 = _ok(two, 0)
    thru = _ok(a1, 1)                     # y reaches the GLOG_ADJ node through child0 alone: accepted
    assert _ops(thru).count(_lib.OP_GLOG_JVP) == 1 and _lib.OP_GLOG_ADJ not in _ops(thru)
    st, _ = _image(a1, 0)                 # x is its operand
    assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED" and "GAAST_OP_GLOG_ADJ" in _lib.lib().gaast_expr_last_error().decode()


@pytest.mark.parametrize("build,metric,opname", [(_gsqrt, 3, "GAAST_OP_GSQRT_ADJ"), (_glog, 3, "GAAST_OP_GLOG_ADJ"), (_gsqrt_times, 3, "GAAST_OP_GSQRT_ADJ"),
                                                 (_pose_error, PGA, "GAAST_OP_GLOG_ADJ")], ids=["gsqrt", "glog", "gsqrt*y", "pose"])
def test_without_the_flag_everything_is_as_before(build, metric, opname):
    d0, d1 = H._desc(build, metric), H._desc(build, metric, flags=FLAG)
    assert _same_but_flags(d0, d1)
    for s in H._user_slots(d0):
        a0, a1 = _ok(d0, s), _ok(d1, s)
        assert _same_but_flags(a0, a1)
        if not {_lib.OP_GSQRT_ADJ, _lib.OP_GLOG_ADJ} & set(_ops(a0)):
            continue                      # (the gradient in y of gsqrt(x) * y holds the forward root only)
        for s2 in (0, d0.n_inputs):       # through the operand and through the cotangent: today's status and message
            st, _ = _image(a0, s2)
            assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
            assert _lib.lib().gaast_expr_last_error().decode() == f"second-order reverse mode through {opname} is not implemented"
    # a tangent node on the path of a flagless program is refused by name in the same words; off the path it is carried along
    if build in (_gsqrt_times,):
        j = _ok(_ok(d1, 0), d1.n_inputs)
        nodes = (_lib.NodeDesc * j.n_nodes)(*[j.nodes[i] for i in range(j.n_nodes)])
        plain = _lib.ProgramDesc()
        C.memmove(C.byref(plain), C.byref(j), C.sizeof(plain))
        plain.nodes, plain.flags = nodes, 0
        st, _ = _image(plain, 0)
        assert _lib.STATUS_NAMES[st] == "UNIMPLEMENTED"
        assert _lib.lib().gaast_expr_last_error().decode() == "second-order reverse mode through GAAST_OP_GSQRT_JVP is not implemented"
        st, off = _image(plain, 1)
        assert st == 0 and _lib.OP_GSQRT_JVP in _ops(off)


def test_images_round_trip_through_the_wire_format():
    d = H._desc(_gsqrt_times, 3, flags=FLAG)
    a = _ok(d, 0)
    for img in (_ok(a, 0), _ok(a, d.n_inputs), _ok(_ok(H._desc(_glog, 3, flags=FLAG), 0), 1)):
        assert {_lib.OP_GSQRT_JVP, _lib.OP_GLOG_JVP} & set(_ops(img))
        data = _serialize(img)
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        h = C.c_void_p(_lib.lib().gaast_program_deserialize(buf, len(data)))
        assert h.value
        try:
            b = _lib.lib().gaast_program_image_desc(h).contents
            assert _serialize(b) == data
            assert [(b.nodes[i].opcode, b.nodes[i].child0, b.nodes[i].child1) for i in range(b.n_nodes)] == \
                [(img.nodes[i].opcode, img.nodes[i].child0, img.nodes[i].child1) for i in range(img.n_nodes)]
        finally:
            _lib.lib().gaast_program_image_free(h)


# ---- the host code under sanitizers, and the lowered tables -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """stdout of the sanitizer build of the host code (a stand-alone program, compiled and run once for the module)"""
    csrc = os.path.join(ROOT, "gaast_amd", "csrc")
    exe = tmp_path_factory.mktemp("root_log_jvp_asan") / "root_log_jvp_asan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(csrc, "device"), "-I", os.path.join(csrc, "common"), "-I", os.path.join(csrc, "host"),
           os.path.join(ROOT, "tests", "cpp", "root_log_jvp_sanitize_driver.cpp")]
    cmd += plan_sources(csrc)
    subprocess.run(cmd + ["-o", str(exe)], check=True, cwd=csrc)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return run.stdout


def test_host_code_is_clean_under_asan_and_ubsan(driver):
    assert driver.strip().endswith("ALL OK")
    for n in range(1, 8):
        for fn in ("gsqrt", "glog"):
            assert f"ok  {fn}(x) full n={n}\n" in driver and (n == 1 or f"ok  {fn}(x) even n={n}\n" in driver)
    for what in ("gsqrt(x) * y", "glog(m * t.inv())", "gsqrt(m ~t)", "raw tables", "raw malformed nodes"):
        assert f"ok  {what}\n" in driver


# tag -> (metric, operand grades, flipped grades of the operand read, tangent grades, result grades)
TABLES = {"pga": (PGA, [0, 1, 2, 3, 4], {2, 3}, [1, 2, 3], [0, 1, 2, 4]), "cga": (CGA, [2], set(), [0, 4], [0, 2, 4]),
          "odd": (ODD, [0, 1, 2, 3], set(), [0, 1, 2, 3], [0, 1, 2, 3])}


def _lines(driver, what, tag, kind):
    return [f for f in (line.split() for line in driver.splitlines()) if len(f) > 3 and f[0] == what and f[1] == tag and f[2] == kind]


@pytest.mark.parametrize("kind", ["sqrt", "log"])
@pytest.mark.parametrize("tag", sorted(TABLES))
def test_lowered_tables_match_numpy(driver, tag, kind):
    """the blade list, the offsets of A, h and res, the folded signs of the operand read, and the coefficients of L and of the
    right-multiplication matrix against glog_numpy.right_matrix, entry for entry"""
    metric, grades, flip, h_grades, res_grades = TABLES[tag]
    n = len(metric)
    S, Cm, _ = gx.structure(tuple(metric), tuple(grades))
    N = len(S)
    outs = {int(f[4]): (int(f[3]),) + tuple(int(v) for v in f[5:10]) for f in _lines(driver, "RLOUT", tag, kind)}
    tab = {(int(f[3]), int(f[4])): (float(f[5]), float(f[6])) for f in _lines(driver, "RLTAB", tag, kind)}
    where = lambda gr: {b: i for i, b in enumerate(inu.row_blades(n, tuple(gr)))}
    a_w, h_w, r_w = where(grades), where(h_grades), where(res_grades)
    assert sorted(outs) == list(range(N)) and len(tab) == N * N
    for j in range(N):
        Nn, blade, a_off, res_off, h_off, neg = outs[j]
        assert (Nn, blade) == (N, S[j])
        assert a_off == a_w.get(blade, -1) and h_off == h_w.get(blade, -1) and res_off == r_w.get(blade, -1)
        assert neg == (1 if inu.grade(blade) in flip and blade in a_w else 0)
    # R_M of the restatement with M the k-th unit vector has the coefficient of M[k] at [r][r xor k]
    R = np.stack([gl.right_matrix(Cm, np.eye(N)[k:k + 1])[0] for k in range(N)])
    for r in range(N):
        for j in range(N):
            cf, cr = tab[r, j]
            assert cf == Cm[r, j] and cr == R[r ^ j, r, j] == Cm[r, r ^ j], (r, j)


def test_a_gsqrt_adj_node_with_the_mask_of_the_blade_set_produces_every_blade(driver):
    """the operand is a PGA3D bivector, the node's mask the even grades: all 8 blades are written, 6 of them read from the operand"""
    rows = _lines(driver, "RLOUT", "adj-full", "sqrt_adj")
    assert len(rows) == 8
    S = gx.structure(tuple(PGA), (2,))[0]
    even = {b: i for i, b in enumerate(inu.row_blades(4, (0, 2, 4)))}
    biv = {b: i for i, b in enumerate(inu.row_blades(4, (2,)))}
    for f in rows:
        j, blade, a_off, res_off, g_off = int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8])
        assert blade == S[j] and res_off == even[blade] and g_off == even[blade] and a_off == biv.get(blade, -1)
