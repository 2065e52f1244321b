"""Every kernel's launch-time row I/O form on strided, padded and misaligned rows ("Row I/O forms").

Almost every kernel exists in two or three forms; which one runs is decided at launch from the pointers and row strides of the
bound rows.  Rows made by DeviceMV.from_rows are contiguous and generously aligned, so they only ever reach one form.  Here the
same values are evaluated under the layouts of tests/layouts.py -- applied to ONE bound row at a time (a left flag tested against
the right pointer shows only then) and to all rows at once -- against one reference evaluation per case:

  * the launch's kernel family is asserted from its label, the run-time variant from SpecializedAst.launch_variants()
    (gaast_hip_program_launch_variant): the fast one under `contig`, the general one under every layout the rule in the launcher's
    run_* function excludes, the fast one again under a layout the rule still admits.  Forms chosen INSIDE a generated kernel (gaast_jit,
    gaast_chain) or inside k_linmap_small / k_sum_rows are not visible to the host: the rule is cited where the case is defined;
  * values: the bound the project already states for the kernel (cited per case), never a new one;
  * two layouts that report the same variant give the same bits;
  * every input buffer is bitwise unchanged, every canary around and between the result rows is untouched;
  * some result component exceeds 1 in magnitude, so zeros cannot pass.

Batches: 1, and one that leaves the last workgroup partial (from the launch's items per workgroup).
"""
import math
import zlib

import numpy as np
import pytest

import gaast_amd as ga
from helpers import (HipBackend, abs_terms_bound, bits_to_row, full_grades, linmap_host_apply as host_apply, n_choose_k, oracle_eval_batch, row_to_bits, rows_of)
from layouts import BITS, NP, layouts_of, place, place_out
from oracle import pyoracle as ogm

pytestmark = pytest.mark.gpu

EVEN = lambda n: [k for k in range(n + 1) if k % 2 == 0]
EPS = {ga.F64: 2.0 ** -52, ga.F32: 2.0 ** -23}
_CACHE = {}     # one reference evaluation (and one specialised program) per case, for the whole module


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _row_len(n, grades):
    return sum(n_choose_k(n, k) for k in grades)


def _grades_of(n, mask):
    return [k for k in range(n + 1) if (mask >> k) & 1]


def _bits(a, dtype):
    return np.ascontiguousarray(a, dtype=NP[dtype]).view(BITS[dtype])


def _layout_for(r, l, shared):
    """a shared (batch-1) row has no stride: only its base can move"""
    if r not in shared:
        return l
    return ("shift" if l == "shift_pad16" else l) if l.startswith("shift") else "shared"


def _assignments(names, dtype, shared=()):
    """all `contig`; then every layout on ONE bound row, the others contig; then every layout on all rows at once"""
    lays = [l for l in layouts_of(dtype) if l != "contig"]
    base = {r: _layout_for(r, "contig", shared) for r in names}
    yield dict(base)
    for r in names:
        for l in lays:
            if r in shared and (not l.startswith("shift") or l == "shift_pad16"):
                continue
            yield {**base, r: _layout_for(r, l, shared)}
    for l in lays:
        yield {r: _layout_for(r, l, shared) for r in names}


def _aligned(p, batch):
    """the launcher's test of a bound row (runtime.hip: `rows_aligned16`): base and bound stride multiples of 16 bytes; a row
    shared by all items of a batch > 1 is bound with stride 0"""
    return p.aligned16(0 if (p.batch == 1 and batch != 1) else None)


class Case:
    """One program.  slots: grade list per input slot; reference(rows64, batch) -> (want f64 rows, out mask, aux);
    check(got, want, aux, rows64, variant, batch): the value assertions; expect(placed, batch) -> {launch index: variant}."""

    def __init__(self, name, n, dtype, alg, build, slots, family, reference, check, expect, flags=0, shared=(), ipb=1, scale=1.0,
                 label_has=(), n_launches=None):
        self.name, self.n, self.dtype, self.alg, self.build, self.slots = name, n, dtype, alg, build, slots
        self.family, self.reference, self.check, self.expect = family, reference, check, expect
        self.flags, self.shared, self.scale, self.label_has, self.n_launches = flags, tuple(shared), scale, tuple(label_has), n_launches
        self.ipb = ipb      # items per workgroup of the family's launch (see ITEMS PER WORKGROUP below): sizes the ragged batch

    def spec(self):
        return _cached(("spec", self.name), lambda: self.build(HipBackend()).specialize(self.alg, dtype=self.dtype, flags=self.flags))

    def data(self, batch):
        def make():
            rng = np.random.default_rng(zlib.crc32(f"{self.name}/{batch}".encode()))
            rows = {s: rows_of(self.n, g, 1 if s in self.shared else batch, rng, np.float32) * np.float32(self.scale)
                    for s, g in enumerate(self.slots)}     # binary32 values: the same numbers in both value types
            rows64 = {s: r.astype(np.float64) for s, r in rows.items()}
            return (rows64,) + tuple(self.reference(rows64, batch))
        return _cached(("data", self.name, batch), make)


def _run(case, batch):
    spec = case.spec()
    labels = spec.launches()
    fam = [i for i, l in enumerate(labels) if case.family in l.split(" :: ")[-1]]
    assert fam, (case.family, labels)
    if case.n_launches is not None:
        assert len(labels) == case.n_launches, labels
    for frag in case.label_has:
        assert any(frag in l for l in labels), (frag, labels)
    assert spec.launch_variants() == [-1] * len(labels) or ("evaluated", case.name) in _CACHE     # nothing recorded before the first evaluation
    rows64, want, wmask, aux = case.data(batch)
    assert np.abs(want).max() > 1.0, "the case must produce a component beyond 1 in magnitude"
    og = _grades_of(case.n, wmask)
    out_len = _row_len(case.n, og)
    names = [f"in{s}" for s in range(len(case.slots))] + ["out"]
    shared = {f"in{s}" for s in case.shared} if batch > 1 else set()
    by_variant = {}
    seen = set()
    for assign in _assignments(names, case.dtype, shared):
        placed = {f"in{s}": place(rows64[s], assign[f"in{s}"], case.dtype, case.n, g) for s, g in enumerate(case.slots)}
        placed["out"] = place_out(batch, out_len, assign["out"], case.dtype, case.n, og)
        spec.eval_batch([placed[f"in{s}"].mv for s in range(len(case.slots))], batch, out=placed["out"].mv)
        _CACHE[("evaluated", case.name)] = True
        got = placed["out"].rows()
        where = (case.name, batch, assign)
        for p in placed.values():
            p.check()
        variants = spec.launch_variants()
        expected = case.expect(placed, batch)
        for pos, i in enumerate(fam):      # expected: by position among the family's launches, None = every one of them
            exp = expected.get(pos, expected.get(None))
            assert exp is not None and variants[i] == exp, (where, labels[i], variants, expected)
        key = tuple(variants)
        seen.add(key)
        case.check(got, want, aux, rows64, [variants[i] for i in fam], batch, where)
        if key in by_variant:
            assert np.array_equal(_bits(got, case.dtype), by_variant[key][0]), (where, "differs in bits from", by_variant[key][1])
        else:
            by_variant[key] = (_bits(got, case.dtype), assign)
    return seen


# ---- value checks, each with the bound the kernel's existing test states ------------------------------------------------------
def _check_exact(dtype):
    """exact kernels: the oracle's bits (f32: its OG_EVAL_F32 mode), as test_f32_extension_of_the_exact_kernels_is_bit_exact and
    test_medium_programs_run_as_straight_line_code_over_slabs_in_lds"""
    def check(got, want, aux, rows64, variants, batch, where):
        assert got.dtype == NP[dtype] and np.array_equal(got.astype(np.float64), want), (where, float(np.abs(got.astype(np.float64) - want).max()))
    return check


def _check_terms(dtype, factor):
    """re-ordered kernels: |err| <= factor eps sum|terms| per component (4; 8 in a rescaled basis; 5 for a sum of two products):
    test_gpu_dense_oracle.py `_check`, test_n7_products_accumulate.  aux: sum|terms| per item and component."""
    def check(got, want, aux, rows64, variants, batch, where):
        bound = factor * EPS[dtype] * aux + 1e-300
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound), (where, float((err / bound).max()))
    return check


def _oracle(build, alg, dtype, exact):
    def reference(rows64, batch):
        mode = ogm.EVAL_F32 if (exact and dtype == ga.F32) else ogm.EVAL_RELEASE
        want, wmask = oracle_eval_batch(build, alg, rows64, batch, mode=mode)
        return want, wmask, None
    return reference


# ---- dense products ----------------------------------------------------------------------------------------------------
def _dense(name, n, dtype, metric, family, expect, left=None, out_sel=None, beta=False, flags=0, factor=4, ipb=1):
    lg, fg = (full_grades(n) if left is None else left), full_grades(n)
    alg = metric if any(m != 1.0 for m in metric) else n
    general = any(m not in (1.0, -1.0, 0.0) for m in metric)
    if beta:
        build = lambda B: B.input(0, lg, n) * B.input(1, fg, n) + B.input(2, fg, n) * B.input(3, fg, n)
        slots, pairs = [lg, fg, fg, fg], [(0, 1, lg), (2, 3, fg)]
    else:
        build = (lambda B: B.input(0, lg, n) * B.input(1, fg, n)) if out_sel is None else \
                (lambda B: (B.input(0, lg, n) * B.input(1, fg, n)).gselect(out_sel))
        slots, pairs = [lg, fg], [(0, 1, lg)]

    def reference(rows64, batch):
        want, wmask = oracle_eval_batch(build, alg, rows64, batch)
        og = _grades_of(n, wmask)
        S = np.stack([sum(bits_to_row(n, og, abs_terms_bound(n, row_to_bits(n, g, rows64[a][i]), row_to_bits(n, fg, rows64[b][i]),
                                                              metric if general else None)) for a, b, g in pairs) for i in range(batch)])
        return want, wmask, S
    return Case(name, n, dtype, alg, build, slots, family, reference, _check_terms(dtype, factor), expect, flags=flags, ipb=ipb)


def _const(v):
    return lambda placed, batch: {None: v}


def _both_operands_aligned(fast):
    """k_gp_mfma16x4 (runtime.hip run_dense, `prefetch`): the register-prefetch staging needs BOTH operand rows 16-byte aligned in
    base and stride; the result's layout does not enter (`whole_rows` adds out_full && !beta, properties of the program)"""
    return lambda placed, batch: {None: fast if (_aligned(placed["in0"], batch) and _aligned(placed["in1"], batch)) else 0}


# ITEMS PER WORKGROUP.  Only gaast_chain's label carries the figure (parsed there); for the others it is the launch geometry of
# runtime.hip prepare_* / run_* (per launcher), restated here -- if a geometry changes, the batch must follow:
#   k_gp_mfma6      one wave per workgroup (GAAST_MFMA6_WAVES = 1) that keeps GAAST_MFMA6_DEPTH = 4 items in flight: 4
#   k_gp_mfma7, k_gp_mfma16x4      one item per workgroup (items_per_block = 1): every batch > 1 ends in a full group; 1
#   k_gp_mfma32p, n = 10           4 waves per workgroup, 1 wave per item (threads / 64 / (1 << (n - 10))): 4
#   k_gp_dense, n = 10             256 threads, 2^(n - 4) = 64 lanes per item: 4
#   gaast_jit                      lane <-> item, 64 items per wave in both storage forms (jit_items = 64 for slabs in LDS): 64
#   k_elementwise                  a thread takes four items per step: 4
#   k_reduce_scale_wave / k_reduce_scale    4 / 64 items per workgroup (one wave per item / sixteen items per wave, four waves)
# The ragged batch is 2 * ipb + 1 (exact kernels: + 37, a partial wave): never a multiple of ipb.
T, D = "float", "double"
NULL6 = [1.0, 1.0, 1.0, 1.0, 1.0, 0.0]
MIXED10 = [1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0, 1.0]
DENSE_CASES = [
    # k_gp_mfma6: [1] straight-line (full operands, every blade, nothing accumulated), [0] general; one component per lane and
    # load, so no layout changes the form: every layout must report the program's variant and the same bits
    _dense("mfma6-f32", 6, ga.F32, [1.0] * 6, "k_gp_mfma6<float,false,", _const(1), ipb=4),
    _dense("mfma6-f64", 6, ga.F64, [1.0] * 6, "k_gp_mfma6<double,false,", _const(1), ipb=4),
    _dense("mfma6-null-f64", 6, ga.F64, NULL6, "k_gp_mfma6<double,false,", _const(1), ipb=4),
    _dense("mfma6-null-f32", 6, ga.F32, NULL6, "k_gp_mfma6<float,false,", _const(1), ipb=4),
    _dense("mfma6-general-f32", 6, ga.F32, [1.0] * 6, "k_gp_mfma6<float,false,", _const(0), left=[0, 1, 2, 3, 4, 6], ipb=4),
    # k_gp_mfma7: [2] full rows, [1] accumulating (beta), [0] a partial operand; "one component per lane and load: no alignment
    # needed" (run_dense), so again the variant is the program's under every layout
    _dense("mfma7-f32", 7, ga.F32, [1.0] * 7, "k_gp_mfma7<float,", _const(2)),
    _dense("mfma7-f64", 7, ga.F64, [1.0] * 7, "k_gp_mfma7<double,", _const(2)),
    _dense("mfma7-beta-f32", 7, ga.F32, [1.0] * 7, "k_gp_mfma7<float,", lambda p, b: {0: 2, 1: 1}, beta=True, factor=5),
    _dense("mfma7-beta-f64", 7, ga.F64, [1.0] * 7, "k_gp_mfma7<double,", lambda p, b: {0: 2, 1: 1}, beta=True, factor=5),
    _dense("mfma7-general-f64", 7, ga.F64, [1.0] * 7, "k_gp_mfma7<double,", _const(0), left=[0, 1, 2, 3, 4, 5]),
    # k_gp_mfma16x4: [2] prefetch + straight-line stores, [1] prefetch (projected result), [0] general staging
    _dense("mfma16-n8-f32", 8, ga.F32, [1.0] * 8, "k_gp_mfma16x4<float,false,8,", _both_operands_aligned(2)),
    _dense("mfma16-n9-f64", 9, ga.F64, [1.0] * 9, "k_gp_mfma16x4<double,false,9,", _both_operands_aligned(2)),
    _dense("mfma16-n10-f64", 10, ga.F64, [1.0] * 10, "k_gp_mfma16x4<double,false,10,", _both_operands_aligned(2)),
    _dense("mfma16-n8-f32-projected", 8, ga.F32, [1.0] * 8, "k_gp_mfma16x4<float,false,8,", _both_operands_aligned(1), out_sel=[0, 2, 3, 5, 8]),
    _dense("mfma16-n9-f64-projected", 9, ga.F64, [1.0] * 9, "k_gp_mfma16x4<double,false,9,", _both_operands_aligned(1), out_sel=[1, 2, 4, 6, 9]),
    # one kernel per launch; the 16-byte-piece branch of stage_operands is taken per operand INSIDE the kernel from
    # DenseArgs::left_contig / right_contig = (full, sequential map) && rows_aligned16(row), set in run_dense: contig and pad16 rows
    # take it, pad_odd and every shift take the scalar branch
    _dense("mfma32p-n10-f32", 10, ga.F32, [1.0] * 10, "k_gp_mfma32p<false,10>", _const(0), ipb=4),
    _dense("dense-n10-f32", 10, ga.F32, MIXED10, "k_gp_dense<float,false,256,", _const(0), flags=ga.FLAG_NO_MFMA, ipb=4),
    _dense("dense-n10-f64", 10, ga.F64, MIXED10, "k_gp_dense<double,false,256,", _const(0), flags=ga.FLAG_NO_MFMA, ipb=4),
    # a rescaled basis (general diagonal metric): general staging only, 8 eps (test_general_diagonal_metrics_run_on_the_dense_kernels)
    _dense("rescaled-n8-f64", 8, ga.F64, [2.0, 0.5, -3.0, 1.0, 1.0, 1.0, 1.0, 1.0], "k_gp_mfma16x4<double,false,8,0,true", _const(0), factor=8),
]


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: c.name)
def test_dense_products_under_every_row_layout(case):
    seen = set()
    for batch in (1, 2 * case.ipb + 1):
        seen |= _run(case, batch)
    if "mfma16-" in case.name:     # both sides of the launch rule were taken
        assert len(seen) == 2, seen


def test_n12_f32_dense_product_on_four_layouts():
    """k_gp_mfma32p<false,12> (the headline kernel; 940 MB oracle table, so one batch of 3 and four layouts): all contig (vector
    branch of stage_operands), right `shift`, result `pad_odd`, all `shift_pad16` (scalar branch on both sides)"""
    case = _dense("mfma32p-n12-f32", 12, ga.F32, [1.0] * 12, "k_gp_mfma32p<false,12>", _const(0))
    spec, batch = case.spec(), 3
    assert any(case.family in l for l in spec.launches()), spec.launches()
    rows64, want, wmask, S = case.data(batch)
    assert np.abs(want).max() > 1.0
    fg = full_grades(12)
    first = None
    for assign in ({}, {"in1": "shift"}, {"out": "pad_odd"}, {"in0": "shift_pad16", "in1": "shift_pad16", "out": "shift_pad16"}):
        placed = {f"in{s}": place(rows64[s], assign.get(f"in{s}", "contig"), ga.F32, 12, fg) for s in range(2)}
        placed["out"] = place_out(batch, 1 << 12, assign.get("out", "contig"), ga.F32, 12, fg)
        spec.eval_batch([placed["in0"].mv, placed["in1"].mv], batch, out=placed["out"].mv)
        got = placed["out"].rows()
        for p in placed.values():
            p.check()
        assert spec.launch_variants() == [0], (assign, spec.launch_variants())
        case.check(got, want, S, rows64, [0], batch, assign)
        first = _bits(got, ga.F32) if first is None else first
        assert np.array_equal(_bits(got, ga.F32), first), assign      # staging moves bits, it does not reorder sums


# ---- chained dense products: R X ~R, the list R X evaluated in the dense kernel's staging -----------------------------------------
def _sandwich(name, n, family, shared):
    even = EVEN(n)
    build = lambda B: (lambda r, x: r * x * r.rev())(B.input(0, even, n), B.input(1, [1], n))

    def reference(rows64, batch):
        want, wmask = oracle_eval_batch(build, n, rows64, batch)
        rx, rxmask = oracle_eval_batch(lambda B: B.input(0, even, n) * B.input(1, [1], n), n, rows64, batch)
        odd, og = _grades_of(n, rxmask), _grades_of(n, wmask)
        S = np.stack([bits_to_row(n, og, abs_terms_bound(n, row_to_bits(n, odd, rx[i]), row_to_bits(n, even, rows64[0][0 if shared else i])))
                      for i in range(batch)])
        return want, wmask, S

    def expect(placed, batch):
        # a chained step prefetches only its right operand (run_dense: `s.dense.chained || ...`), here ~R = the rows of slot 0;
        # k_gp_mfma7 needs no alignment at all.  The list's own operands (pre_left / pre_right: slots 0 and 1) are read
        # component by component with strides of their own.
        if "mfma7" in family:
            return {None: 2}
        return {None: 2 if _aligned(placed["in0"], batch) else 0}
    # bound: 4 eps sum|terms| of the second product (test_rotor_sandwich_beyond_the_fused_slab_is_one_launch)
    return Case(name, n, ga.F64, n, build, [even, [1]], family, reference, _check_terms(ga.F64, 4), expect,
                shared=(0,) if shared else (), label_has=("<- product_csr",), n_launches=1)


SANDWICH_CASES = [_sandwich("sandwich-n8", 8, "k_gp_mfma7<double,", False), _sandwich("sandwich-n8-shared-R", 8, "k_gp_mfma7<double,", True),
                  _sandwich("sandwich-n9", 9, "k_gp_mfma16x4<double,false,8,", False), _sandwich("sandwich-n9-shared-R", 9, "k_gp_mfma16x4<double,false,8,", True)]


@pytest.mark.parametrize("case", SANDWICH_CASES, ids=lambda c: c.name)
def test_chained_dense_products_under_every_row_layout(case):
    for batch in (1, 5):
        _run(case, batch)


# ---- gaast_chain: (R X ~R).g(1), two lists in one specialised launch -----------------------------------------------------------
def _chain(name, n, dtype, flags):
    even = EVEN(n)
    build = lambda B: (lambda r, x: (r * x * r.rev()).g(1))(B.input(0, even, n), B.input(1, [1], n))
    exact = bool(flags & ga.FLAG_EXACT_ORDER)

    def reference(rows64, batch):
        want, wmask = oracle_eval_batch(build, n, rows64, batch, mode=ogm.EVAL_F32 if (exact and dtype == ga.F32) else ogm.EVAL_RELEASE)
        if exact:
            return want, wmask, None
        mid, mmask = oracle_eval_batch(lambda B: B.input(0, even, n) * B.input(1, [1], n), n, rows64, batch)
        odd = _grades_of(n, mmask)
        S = np.stack([bits_to_row(n, [1], abs_terms_bound(n, row_to_bits(n, odd, mid[i]), row_to_bits(n, even, rows64[0][i]))) for i in range(batch)])
        return want, wmask, S
    # The staging form is chosen inside the generated kernel (plan_chain_jit.cpp, the kernel text: `fast = s_l1 == L1 && s_r1 == R1 && both
    # bases 16-byte aligned && whole 16-byte pieces per workgroup`): contig rows take the coalesced span, every other layout of
    # slot 0 or 1 the per-lane staging; the result rows are always stored per lane.  One kernel: variant 0.  The order of the sums
    # does not depend on the staging, so all layouts agree in bits -- with GAAST_FLAG_EXACT_ORDER with the oracle's; without, within
    # 4 eps sum|terms| of the second list (test_projected_rotor_sandwich_is_one_launch_of_two_lists).
    check = _check_exact(dtype) if exact else _check_terms(dtype, 4)
    return Case(name, n, dtype, n, build, [even, [1]], "gaast_chain<" + (T if dtype == ga.F32 else D) + ">", reference, check, _const(0),
                flags=flags, n_launches=1)


CHAIN_CASES = [_chain("chain-n8-f64", 8, ga.F64, 0), _chain("chain-n8-f64-exact", 8, ga.F64, ga.FLAG_EXACT_ORDER),
               _chain("chain-n9-f64", 9, ga.F64, 0), _chain("chain-n9-f64-exact", 9, ga.F64, ga.FLAG_EXACT_ORDER),
               _chain("chain-n8-f32", 8, ga.F32, 0), _chain("chain-n8-f32-exact", 8, ga.F32, ga.FLAG_EXACT_ORDER)]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: c.name)
def test_list_chains_under_every_row_layout(case):
    label = case.spec().launches()[0]
    ipb = int(label.split("items")[0].split("[")[-1].split(",")[-1])      # "gaast_chain<T>[<k> items, <t> threads ...]"
    for batch in (1, 2 * ipb + 1):
        _run(case, batch)


# ---- gaast_jit (specialised small programs) and the element-wise pass: exact kernels ----------------------------------------------
def _exact_case(name, n, dtype, alg, build, slots, family, flags=0, scale=1.0, label_has=(), ipb=64):
    return Case(name, n, dtype, alg, build, slots, family, _oracle(build, alg, dtype, True), _check_exact(dtype), _const(0), flags=flags,
                scale=scale, label_has=label_has, n_launches=1, ipb=ipb)


CGA = [1.0, 1.0, 1.0, 1.0, -1.0]
_vinv8 = lambda B: B.input(0, EVEN(8), 8).vinv()
_cl41 = lambda B: (lambda r, x: r * x * r.rev())(B.input(0, [0, 2, 4], 5), B.input(1, [1], 5))
_r5 = lambda B: B.input(0, full_grades(5), 5) * B.input(1, full_grades(5), 5)
_unary12 = lambda B: (-(B.input(0, [2], 12).rev()) + B.input(1, [2], 12).ginvol()).rev() * B.input(2, [0], 12)
_unary12_6 = lambda B: (-(B.input(0, [6], 12).rev()) + B.input(1, [6], 12).ginvol()).rev() * B.input(2, [0], 12)
EXACT_CASES = [
    # gaast_jit with slabs in LDS (plan_fused.cpp: LdsForm::staging, per operand `fast_cond`: stride == length && base 16-byte aligned, else the lane reads its
    # own row; the last partial wave always does).  Inputs scaled by 2^-6 so that the inverse has components beyond 1.
    _exact_case("jit-lds-vinv8-f64", 8, ga.F64, 8, _vinv8, [EVEN(8)], "ast_jit[", scale=2.0 ** -6, label_has=("ast_jit[", "slab in LDS")),
    _exact_case("jit-lds-vinv8-f32", 8, ga.F32, 8, _vinv8, [EVEN(8)], "ast_jit[", scale=2.0 ** -6, label_has=("ast_jit[",)),
    # gaast_jit in registers, f32 (plan_fused.cpp: RowIo, `full && s == len && (in & 15) == 0` span form, `line_ok` line form for rows of >= 128
    # bytes with a 16-byte-multiple stride, else per lane): the programs of test_specialised_kernels_row_io_forms_are_bit_exact.
    # Grade 1 of R^5 is a 20-byte row: `contig` rows are themselves misaligned from the second row on.
    _exact_case("jit-reg-cl41-f32", 5, ga.F32, CGA, _cl41, [[0, 2, 4], [1]], "ast_jit[", label_has=("ast_jit[",)),
    _exact_case("jit-reg-r5-f32", 5, ga.F32, 5, _r5, [full_grades(5)] * 2, "ast_jit[", flags=ga.FLAG_EXACT_ORDER, label_has=("ast_jit[",)),
    # k_elementwise: one component per thread and load, every layout the same code (inputs scaled by 4: a batch of one must still
    # produce a component beyond 1)
    _exact_case("elementwise-unary12-f64", 12, ga.F64, 12, _unary12_6, [[6], [6], [0]], "k_elementwise<double", scale=4.0, label_has=("elementwise[",), ipb=4),
    _exact_case("elementwise-unary12-f32", 12, ga.F32, 12, _unary12_6, [[6], [6], [0]], "k_elementwise<float", scale=4.0, label_has=("elementwise[",), ipb=4),
    # the same arms over bivector rows are short enough for a specialised kernel with its slabs in LDS (the `unary12` program of
    # test_medium_programs_run_as_straight_line_code_over_slabs_in_lds): 66-element rows, 264 bytes in f32
    _exact_case("jit-unary12-f64", 12, ga.F64, 12, _unary12, [[2], [2], [0]], "ast_jit[", label_has=("ast_jit[",)),
    _exact_case("jit-unary12-f32", 12, ga.F32, 12, _unary12, [[2], [2], [0]], "ast_jit[", label_has=("ast_jit[",)),
]


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: c.name)
def test_exact_kernels_under_every_row_layout(case):
    for batch in (1, 2 * case.ipb + 37):
        _run(case, batch)


# ---- REDUCE_SCALE: the versor inverse beyond a fused slab ----------------------------------------------------------------------
def _vinv_case(n):
    even = EVEN(n)
    build = lambda B: B.input(0, even, n).vinv()

    def expect(placed, batch):
        # run_reduce: k_reduce_scale_wave only if the operand rows AND the result rows are 16-byte aligned in base and stride
        # (its lanes move 16-byte pieces); anything else silently runs k_reduce_scale
        return {None: 1 if (_aligned(placed["in0"], batch) and _aligned(placed["out"], batch)) else 0}

    def check(got, want, aux, rows64, variants, batch, where):
        g64 = got.astype(np.float64)
        if variants == [1]:
            # the two bounds of test_the_versor_inverse_beyond_a_fused_slab_is_one_launch: 6 eps of the exactly summed value, 32 eps of
            # the reference's
            eps = EPS[ga.F64]
            a64 = rows64[0]
            n_true = np.array([math.fsum(r * r) for r in a64])
            true = np.sign(want) * np.abs(a64) / n_true[:, None]
            assert np.all(np.abs(g64 - true) <= 6 * eps * np.abs(true) + 1e-300), (where, float((np.abs(g64 - true) / (eps * np.abs(true) + 1e-300)).max()))
            assert np.all(np.abs(g64 - want) <= 32 * eps * np.abs(want) + 1e-300), (where, float((np.abs(g64 - want) / (eps * np.abs(want) + 1e-300)).max()))
        else:
            assert np.array_equal(g64, want), where      # k_reduce_scale: the reference's bits
    return Case(f"vinv-n{n}-f64", n, ga.F64, n, build, [even], "k_reduce_scale<double>", _oracle(build, n, ga.F64, True), check, expect,
                scale=2.0 ** -(n - 2), label_has=("reduce_scale[", "k_reduce_scale_wave<"), n_launches=1, ipb=4)


@pytest.mark.parametrize("case", [_vinv_case(9), _vinv_case(12)], ids=lambda c: c.name)
def test_reduce_scale_falls_back_to_the_exact_kernel_on_unaligned_rows(case):
    seen = set()
    for batch in (1, 2 * 64 + 4 + 1):      # partial last workgroup of both kernels (4 and 64 items per workgroup)
        seen |= _run(case, batch)
    assert seen == {(0,), (1,)}, seen


# ---- dense adjoints --------------------------------------------------------------------------------------------------------------
def _adjoint_reference(n, slot, other, g):
    """The gradient of <g, a b> with respect to slot `slot` in numpy float64, from the definition C[a ^ b] += s(a, b) A[a] B[b] in
    blade-bitmask space (Euclidean metric; s as in helpers.gp_bits): grad_A[a] = sum_b s(a, b) G[a ^ b] B[b], grad_B[b] = sum_a
    s(a, b) G[a ^ b] A[a].  Independent of the library.  Returns (gradient rows, sum|terms| rows), both [batch, 2^n] in row order."""
    from helpers import _POP16
    N, fg = 1 << n, full_grades(n)
    a = np.arange(N, dtype=np.int64)[:, None]
    b = np.arange(N, dtype=np.int64)[None, :]
    par = np.zeros((N, N), dtype=np.int64)
    for s_ in range(1, n):
        par += _POP16[(a >> s_) & b]
    sign = np.where(par & 1, -1.0, 1.0)
    if slot == 1:
        sign = sign.T.copy()          # [wrt blade, other blade]
    xor = a ^ b
    grad, terms = [], []
    for i in range(other.shape[0]):
        ob, gb = row_to_bits(n, fg, other[i]), row_to_bits(n, fg, g[i])
        gx = gb[xor]
        grad.append(bits_to_row(n, fg, (sign * gx) @ ob))
        terms.append(bits_to_row(n, fg, np.abs(gx) @ np.abs(ob)))
    return np.stack(grad), np.stack(terms)


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("n,dtype", [(8, ga.F32), (10, ga.F64)], ids=["n8-f32", "n10-f64"])
def test_dense_adjoints_under_every_row_layout(n, dtype, slot):
    """ADJ_LEFT (slot 0) and ADJ_RIGHT (slot 1) of the full product on k_gp_mfma16x4, n = 8 f32 and n = 10 f64 (8-byte elements: a
    one-element shift or an odd stride is the only way to lose alignment): the layout goes on the cotangent, on the other operand and
    on the result in turn, then on all, at batch 1 and 3 (one item per workgroup).  Reference: the gradient from the product's
    definition in numpy float64 (_adjoint_reference); bound: the 16 eps sum|terms| per component of test_dense_adjoints.  The launch
    rule is the forward one: prefetch (with straight-line stores: every component of the gradient is produced) only if both rows
    the step reads are 16-byte aligned in base and stride."""
    N, fg = 1 << n, full_grades(n)
    spec = (ga.mv(ga.Input(0, fg, n)) * ga.mv(ga.Input(1, fg, n))).specialize(n, dtype=dtype, materialize_limit=1)
    vjp = spec.vjp(slot)
    labels = vjp.launches()
    kernel = f"k_gp_mfma16x4<{'float' if dtype == ga.F32 else 'double'},false,{n},"
    fam = [i for i, l in enumerate(labels) if kernel in l and "adjoint" in l]
    assert len(fam) == 1, labels
    assert vjp.launch_variants() == [-1] * len(labels)
    for batch in (1, 3):
        rng = np.random.default_rng(80 + 10 * n + 2 * slot + batch)
        rows = [rng.uniform(-1, 1, (batch, N)).astype(np.float32) for _ in range(2)]      # binary32 values in both value types
        g = rng.uniform(-1, 1, (batch, N)).astype(np.float32)
        want, t = _adjoint_reference(n, slot, rows[1 - slot].astype(np.float64), g.astype(np.float64))
        assert np.abs(want).max() > 1.0
        by_variant = {}
        for assign in _assignments(["other", "cot", "out"], dtype):
            p_other = place(rows[1 - slot], assign["other"], dtype, n, fg)
            p_cot = place(g, assign["cot"], dtype, n, fg)
            p_out = place_out(batch, N, assign["out"], dtype, n, fg)
            ins = [None, None]
            ins[1 - slot] = p_other.mv
            ins[slot] = rows[slot]          # (the adjoint with respect to a slot does not read that slot's rows)
            vjp.eval_batch(ins, p_cot.mv, batch, out=p_out.mv)
            got = p_out.rows()
            where = (n, dtype, slot, batch, assign)
            for p in (p_other, p_cot, p_out):
                p.check()
            v = vjp.launch_variants()[fam[0]]
            assert v == (2 if (p_other.aligned16() and p_cot.aligned16()) else 0), (where, labels, vjp.launch_variants())
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= 16 * EPS[dtype] * t + 1e-300), (where, float((err / (EPS[dtype] * t + 1e-300)).max()))
            if v in by_variant:
                assert np.array_equal(_bits(got, dtype), by_variant[v]), where
            by_variant[v] = _bits(got, dtype)
        assert set(by_variant) == {0, 2}, (batch, set(by_variant))


# ---- outermorphisms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,grades,dtype", [(5, None, ga.F32), (5, [1, 2], ga.F32), (8, None, ga.F32), (8, [0, 2], ga.F32), (8, None, ga.F64), (8, [0, 2], ga.F64)],
                         ids=lambda v: "full" if v is None else str(v))
def test_linmap_under_every_row_layout(n, grades, dtype):
    """k_linmap_small (n <= 6) and k_linmap_mfma: full rows and a partial mask with an odd row length (15 elements at n = 5, 29 at n = 8,
    where `contig` rows are themselves not 16-byte aligned).  k_linmap_small takes 16-byte row I/O per side when
    `stride == row_len && base % 16 == 0 && row bytes % 16 == 0` (runtime.hip `rows_packed_aligned16`, launch_linmap: in_vec / out_vec, flags of the kernel's
    arguments, not a kernel table); k_linmap_mfma has one form.  Bound: the norm-wise one of test_gpu_linmap.py `check`.  The order
    of the sums does not depend on the row I/O: every layout gives the same bits."""
    grades = full_grades(n) if grades is None else grades
    rl = _row_len(n, grades)
    rng = np.random.default_rng(n * 100 + rl)
    m = rng.uniform(-1, 1, (n, n))
    om = ga.Outermorphism(m, dtype)
    for batch in (1, 2 * 64 + 37):
        rows = rng.uniform(-1, 1, (batch, rl)).astype(np.float32)
        want = host_apply(m, grades, rows)
        assert np.abs(want).max() > 1.0
        scale = max(1.0, np.linalg.norm(m, 2)) ** n * np.linalg.norm(rows.astype(np.float64), axis=1)
        first = None
        for assign in _assignments(["in", "out"], dtype):
            p_in = place(rows, assign["in"], dtype, n, grades)
            p_out = place_out(batch, rl, assign["out"], dtype, n, grades)
            om.apply(p_in.mv, p_out.mv)
            got = p_out.rows()
            p_in.check()
            p_out.check()
            err = np.linalg.norm(got.astype(np.float64) - want, axis=1)
            assert (err <= 64 * EPS[dtype] * scale + 1e-300).all(), (assign, batch, float((err / scale).max()))
            first = _bits(got, dtype) if first is None else first
            assert np.array_equal(_bits(got, dtype), first), (assign, batch)


# ---- sum_rows --------------------------------------------------------------------------------------------------------------------
SUM_ROWS = {3: (3, [1]), 10: (5, [2]), 55: (11, [2]), 300: (13, [0, 1, 3]), 462: (11, [5])}


@pytest.mark.parametrize("dtype", [ga.F32, ga.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("row", sorted(SUM_ROWS))
def test_sum_rows_under_every_input_layout(row, dtype):
    """k_sum_rows stages a tile of rows as one vector span (`stride == row_len` and a 16-byte aligned tile start), one scalar span
    (back to back, misaligned) or a strided gather (kernels_reduce.hip.hpp); rows of 300 leave a ragged last 256-column tile.  The
    summation order does not depend on the staging: every layout gives the same bits, and each is within
    (1024 + ceil(B / 1024)) eps sum|x| of math.fsum (test_sum_rows)."""
    dim, grades = SUM_ROWS[row]
    assert _row_len(dim, grades) == row
    for batch in (1, 1023, 1025, 4097):
        x = (np.random.default_rng(batch * 1000 + row).uniform(-4.0, 4.0, (batch, row))).astype(np.float32)
        exact = np.array([math.fsum(x[:, j].astype(np.float64)) for j in range(row)])
        assert np.abs(exact).max() > 1.0
        bound = (1024 + math.ceil(batch / 1024)) * EPS[dtype] * np.sum(np.abs(x.astype(np.float64)), axis=0)
        first = None
        for assign in _assignments(["in", "out"], dtype):
            p_in = place(x, assign["in"], dtype, dim, grades)
            p_out = place_out(1, row, assign["out"], dtype, dim, grades)
            p_in.mv.sum_rows(p_out.mv)
            got = p_out.rows()
            p_in.check()
            p_out.check()
            assert np.all(np.abs(got[0].astype(np.float64) - exact) <= bound + 1e-300), (assign, batch)
            first = _bits(got, dtype) if first is None else first
            assert np.array_equal(_bits(got, dtype), first), (assign, batch)


# ---- gaast_hip_mv_wrap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,off", [(ga.F64, 4), (ga.F64, 1), (ga.F32, 2), (ga.F32, 3)])
def test_mv_wrap_refuses_a_base_that_is_not_a_multiple_of_the_element_size(dtype, off):
    import ctypes as C
    import torch
    ga.init_device()
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    h = C.c_void_p()
    st = ga.lib().gaast_hip_mv_wrap(C.c_void_p(t.data_ptr() + off), 3, 0xF, 2, dtype, 8, C.byref(h))
    assert st == 6 and not h.value, (st, h.value)        # GAAST_ERR_INVALID_ARGUMENT, nothing created
    assert b"element size" in ga.lib().gaast_hip_last_error()
    assert ga.lib().gaast_hip_mv_wrap(C.c_void_p(t.data_ptr() + (8 if dtype == ga.F64 else 4)), 3, 0xF, 2, dtype, 8, C.byref(h)) == 0
    assert h.value
    ga.lib().gaast_hip_mv_free(h)


def test_launch_variant_of_a_bad_index_is_negative():
    spec = (ga.mv(ga.Input(0, [1], 3)) * ga.mv(ga.Input(1, [1], 3))).specialize(3)
    L, p = ga.lib(), spec.program()
    n = L.gaast_hip_program_num_launches(p)
    assert spec.launch_variants() == [-1] * n                      # before any evaluation
    assert L.gaast_hip_program_launch_variant(p, -1) < 0 and L.gaast_hip_program_launch_variant(p, n) < 0
    assert L.gaast_hip_program_launch_variant(None, 0) < 0
    spec.eval_batch([np.ones((2, 3)), np.ones((2, 3))], 2)
    assert spec.launch_variants() == [0] * n                       # single-kernel launches
