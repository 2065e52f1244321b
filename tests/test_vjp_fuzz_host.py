"""Reverse-mode fuzz on the host: the VJP images gaast_program_vjp builds for random programs (tests/fuzz.py, leaves bound as
inputs), evaluated by the plain numpy evaluator of vjp_numpy.py, against a longdouble dual-number evaluation of the FORWARD image
(vjp_dual_numpy.py), per component, within C eps scale -- scale being the reference's magnitude channel, so a wrong small term
shows.  First order in f64 and f32, with explicit forward lists and with materialize_limit=1 (every adjoint compact); second order
in a forward slot and in the cotangent slot against the dual reference applied to the first-order image.  No GPU.

Measured here (numpy against longdouble, seeds as below, CPU): worst ratio 2.627 (f64 first order), 3.987 (f64 second order), 3.371
(f32); left out 2.33 % (first order) and 1.68 % (second order) of the checks.  By the rule of DESIGN.md section 11 -- the next power
of two at least 4 x above the worst ratio -- C64 = 16 (4 x 3.987 = 15.9) and C32 = 16 (4 x 3.371 = 13.5), in vjp_fuzz.py.  The module
prints its worst ratios and left-out shares when it ends (pytest -s)."""
import numpy as np
import pytest

from gaast_amd import _lib
from vjp_fuzz import (C32, C64, EPS32, EPS64, Tally, bound_program, cotangent, explicit_program, panics, reference, vjp_image)
from vjp_numpy import Program, eval_desc

ITEMS = 2
FIRST = range(1000, 2500)      # 1500 seeds, in chunks of 250
SECOND = range(3000, 3420)     # about 300 of these have n <= 5
TOTAL = {"f64": Tally(), "f32": Tally(), "second": Tally()}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, t in TOTAL.items():
        print(f"\n[vjp fuzz host] {name}: {t}")
    for t in TOTAL.values():     # over the whole seed range of the module: at most 5 % left out
        if t.checked:
            assert t.left_out <= 0.05 * (t.checked + t.left_out), str(t)


def _first_order(seeds, tally, dtype, eps, Cb):
    for seed in seeds:
        n, metric, build, rows = bound_program(seed, ITEMS)
        tally.programs += 1
        if not rows:
            tally.unbound += 1
            continue
        try:
            prog, keep = explicit_program(build, metric)
        except _lib.GaastError:
            tally.skipped += 1
            continue
        if panics(prog, rows):
            tally.skipped += 1
            continue
        rounded = None if dtype is np.float64 else dtype
        if rounded is not None:
            rows = {s: r.astype(dtype).astype(np.float64) for s, r in rows.items()}
        g = cotangent(seed, ITEMS, prog.out_len())
        if rounded is not None:
            g = g.astype(dtype).astype(np.float64)
        refs = {(s, i): reference(prog, rows, i, s, rounded=rounded) for s in prog.user_slots() for i in range(ITEMS)}
        for mode, limit in (("explicit", 1 << 24), ("compact", 1)):
            spec = build().specialize(metric, materialize_limit=limit)
            d = spec.program_desc()
            assert [s for s in range(d.n_inputs) if not d.inputs[s].is_const] == prog.user_slots()
            for slot in prog.user_slots():
                st, a = vjp_image(d, slot)
                assert st == 0, (seed, mode, slot, _lib.lib().gaast_expr_last_error())
                img = Program(a)
                for i in range(ITEMS):
                    got = eval_desc(img, {**{s: r[i] for s, r in rows.items()}, d.n_inputs: g[i]}, dtype=dtype)
                    tally.compare(got, refs[slot, i], g[i], eps, Cb, f"seed {seed} {mode} slot {slot} item {i}")


@pytest.mark.parametrize("chunk", range(6))
def test_first_order_f64(chunk):
    t = Tally()
    try:
        _first_order(FIRST[chunk * 250:(chunk + 1) * 250], t, np.float64, EPS64, C64)
        t.caps()
    finally:
        TOTAL["f64"].merge(t)


@pytest.mark.parametrize("chunk", range(6))
def test_first_order_f32(chunk):
    t = Tally()
    try:
        _first_order(FIRST[chunk * 250:(chunk + 1) * 250], t, np.float32, EPS32, C32)
        t.caps()
    finally:
        TOTAL["f32"].merge(t)


@pytest.mark.parametrize("kind", range(6))
def test_evaluator_regenerates_compact_kinds_as_the_explicit_lists(kind):
    """vjp_numpy evaluates a compact node (forward kind, ADJ_LEFT, ADJ_RIGHT) from the regenerated list in forward order: the same bits
    as the explicit image at first order, the same values up to rounding at second order, for all six kinds"""
    import gaast_amd as ga
    n, metric, full = 4, [1.0, -1.0, 2.0, 0.0], [0, 1, 2, 3, 4]

    def build():
        a, b = ga.mv(ga.Input(0, full, n)), ga.mv(ga.Input(1, [1, 2, 4], n))
        return {0: lambda: a * b, 1: lambda: a ^ b, 2: lambda: a & b, 3: lambda: a << b, 4: lambda: a >> b, 5: lambda: a.vee(b)}[kind]()
    out = {}
    for mode, limit in (("explicit", 1 << 24), ("compact", 1)):
        spec = build().specialize(metric, materialize_limit=limit)
        d = spec.program_desc()
        rows = {0: np.random.default_rng(1).uniform(-1, 1, 16), 1: np.random.default_rng(2).uniform(-1, 1, 11)}
        fwd = Program(d)
        rows[2] = np.random.default_rng(3).uniform(-1, 1, fwd.out_len())
        kinds = []
        for s1 in (0, 1):
            st, a = vjp_image(d, s1)
            assert st == 0
            first = Program(a)
            kinds += [nd.kind for nd in first.nodes if nd.opcode == _lib.OP_PRODUCT and nd.lst is None and nd.n_comp_muls]
            out[mode, s1] = eval_desc(first, rows)
            h = np.random.default_rng(4 + s1).uniform(-1, 1, first.out_len())
            for s2 in (0, 1, 2):
                st, a2 = vjp_image(a, s2)
                assert st == 0
                out[mode, s1, s2] = eval_desc(Program(a2), {**rows, a.n_inputs: h})
        if mode == "compact":
            assert sorted(kinds) == [_lib.PROD_ADJ_LEFT + kind, _lib.PROD_ADJ_RIGHT + kind], kinds
    for key in [k for k in out if k[0] == "explicit"]:
        if len(key) == 2 or key[2] != key[1]:     # (a bilinear product's second derivative in the same slot is zero)
            assert np.any(out[key] != 0), key
        if len(key) == 2:
            assert np.array_equal(out[key], out[("compact",) + key[1:]]), key
        else:
            # an explicit list transposed twice is ordered by two stable sorts, the regenerated one is in forward order: other roundings.
            # A component sums at most 16 x 11 terms |c x y z| <= 2 (the metric's largest square), each side within n eps sum |terms|
            assert np.allclose(out[key], out[("compact",) + key[1:]], rtol=0, atol=2 * (16 * 11) * 2 * (16 * 11) * EPS64), key


@pytest.mark.parametrize("chunk", range(3))
def test_second_order_f64(chunk):
    """the image of vjp(slot), differentiated again in a forward slot and in its cotangent slot, against the dual reference applied
    to the first-order image (explicit lists, n <= 5).  The image is linear in its cotangent, but the scalar ops it replays still act
    on forward values: where one meets s <= 0 the image itself is NaN, so the domain rule is applied in both slots"""
    t = Tally()
    try:
        for seed in SECOND[chunk * 140:(chunk + 1) * 140]:
            n, metric, build, rows = bound_program(seed, ITEMS)
            if n > 5:
                continue
            t.programs += 1
            if not rows:
                t.unbound += 1
                continue
            try:
                prog, keep = explicit_program(build, metric)
            except _lib.GaastError:
                t.skipped += 1
                continue
            if panics(prog, rows):
                t.skipped += 1
                continue
            d = keep.program_desc()
            rng = np.random.default_rng([seed, 78])
            g = cotangent(seed, ITEMS, prog.out_len())
            for s1 in prog.user_slots():
                st, a = vjp_image(d, s1)
                assert st == 0, (seed, s1)
                first = Program(a)
                h = rng.uniform(-1.0, 1.0, (ITEMS, first.out_len()))
                fwd_slots = prog.user_slots()
                for s2 in (fwd_slots[(seed + s1) % len(fwd_slots)], d.n_inputs):
                    st, a2 = vjp_image(a, s2)
                    assert st == 0, (seed, s1, s2, _lib.lib().gaast_expr_last_error())
                    second = Program(a2)
                    for i in range(ITEMS):
                        bound = {**{s: r[i] for s, r in rows.items()}, d.n_inputs: g[i]}
                        ref = reference(first, {s: np.atleast_2d(r) for s, r in bound.items()}, 0, s2)
                        got = eval_desc(second, {**bound, a.n_inputs: h[i]})
                        t.compare(got, ref, h[i], EPS64, C64, f"seed {seed} slots {s1}, {s2} item {i}")
        t.caps()
    finally:
        TOTAL["second"].merge(t)
